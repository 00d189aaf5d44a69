"""The shading arithmetic (ndt_amd/csrc/ndt_shading.hpp) through every kernel that calls it, with and without specular lighting.

One text states what a light adds to a hit, whether a shadow answer leaves it lit, a hit's children and the blend with what they
returned; the per-bounce kernels, the light-window kernels, the frame kernel and the bottom-up combine call it.  A small frame
takes the frame kernel unless told otherwise, so each caller is selected here by option: pipeline 1 (k_shade_emit,
k_shade_finish, k_resolve) with the lighting on the light stream or not, pipeline 2 (k_frame_stream), and light windows of two
list entries and of one (k_shade_window<false>, k_shade_window<true>, k_shade_last).  All of them must give the same bytes and
ray counts, and the oracle's frame.  Needs a real MI355X: run with `pytest -m gpu`."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-9     # what differing libm ulps can explain (tests/test_gpu_parity.py)
W, H = 64, 36

DEFAULTS = {"pipeline": 0, "light_overlap": 1, "light_window": 0}
# (what the render is called, the options that differ from pipeline 1's defaults)
RENDERS = [
    ("pipeline 1", {}),
    ("pipeline 2", {"pipeline": 2}),
    ("pipeline 1, light_overlap 0", {"light_overlap": 0}),
    ("pipeline 1, light_window 2", {"light_window": 2}),
    ("pipeline 1, light_window 1", {"light_window": 1}),
]


@pytest.fixture(scope="module")
def gpu():
    from ndt_amd.hip import NdtHip
    ctx = NdtHip(0)
    yield ctx
    ctx.close()


def counts(st):
    return (st.rays_primary, st.rays_secondary, st.rays_shadow, st.rays_ref_equiv, st.levels)


def render_with(gpu, scene, options, depth, specular):
    """One render of `scene` under pipeline 1 with `options` on top; the options are back at their defaults afterwards."""
    chosen = dict(DEFAULTS, pipeline=1)
    chosen.update(options)
    try:
        for name, value in chosen.items():
            gpu.set_option(name, value)
        gpu.upload_scene(scene)
        return gpu.render(W, H, depth, specular=specular)
    finally:
        for name, value in DEFAULTS.items():
            gpu.set_option(name, value)


# zoo4d: an ambient entry in the light list, point, directional and spot lights, two transparent objects, mirrors
# c3_random4d: five point lights, eleven transparent objects
@pytest.mark.parametrize("specular", [0, 1])
@pytest.mark.parametrize("name", ["zoo4d", "c3_random4d"])
def test_every_shading_caller_gives_the_same_frame(gpu, oracle, name, specular):
    g = golden(name)
    runs = [(what, render_with(gpu, g.scene, options, g.depth, specular)) for what, options in RENDERS]
    first, first_st = runs[0][1]
    for what, (out, st) in runs[1:]:
        print("%s, specular %d, %s: %d values differ, counts %s" % (name, specular, what, int((out != first).sum()), counts(st)))
        assert out.tobytes() == first.tobytes(), what
        assert counts(st) == counts(first_st), what
    want, _ = oracle.render(g.scene, W, H, g.depth, specular=specular)
    diff = np.abs(first - want).max()
    print("%s, specular %d: max |gpu - oracle| %g, counts %s" % (name, specular, diff, counts(first_st)))
    assert diff < TOL_TIGHT, "max abs diff %g" % diff


@pytest.mark.parametrize("depth", [1, 2])
def test_deepest_bounce_blended_on_the_spot_without_specular(gpu, oracle, depth):
    """Shallow trees, whose every child is cut off (black, ndt.c:336-341), without specular lighting.  At depth 2 the per-bounce
    pipeline lights bounce 1, the deepest, and blends it in the same kernel (shade_finish_node, resolve_here); at depth 1 the
    primaries are all there is, and the kernel that finishes the pixels blends them (resolve_node)."""
    g = golden("zoo4d")
    out, st = render_with(gpu, g.scene, {}, depth, 0)
    want, wst = oracle.render(g.scene, W, H, depth, specular=0)
    diff = np.abs(out - want).max()
    print("zoo4d, depth %d, specular 0: max |gpu - oracle| %g, counts %s" % (depth, diff, counts(st)))
    assert diff < TOL_TIGHT, "max abs diff %g" % diff
    assert counts(st)[:4] == (wst.rays_primary, wst.rays_secondary, wst.rays_shadow, wst.rays_ref_equiv)
