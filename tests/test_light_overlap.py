"""Option "light_overlap" of the per-bounce pipeline: the lighting of bounce b - 1 on the context's second stream, beside
the trace launch of bounce b, with the shadow answers in two banks by bounce parity.  It changes WHEN
a kernel runs and where two arrays live, never what is computed: every frame below is rendered with the option off and
on, and the two framebuffers must be the same bytes and the ray counts equal.

pipeline = 1 everywhere: `auto` renders passes this small with the frame kernel, which has no lighting launches.
Needs a real MI355X: run with `pytest -m gpu`.
"""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    from ndt_amd.hip import NdtHip
    ctx = NdtHip(0)
    ctx.set_option("pipeline", 1)
    yield ctx
    ctx.close()


def counts(st):
    return (st.rays_primary, st.rays_secondary, st.rays_shadow, st.rays_ref_equiv, st.levels)


def off_and_on(gpu, *args, **kw):
    """The same render with light_overlap 0 and 1: (what the option-off render returned, the option-on one)."""
    res = []
    for on in (0, 1):
        gpu.set_option("light_overlap", on)
        res.append(gpu.render(*args, **kw))
    return res


def assert_same(off, on, what=""):
    assert len(off) == len(on)
    for a, b in zip(off[:-1], on[:-1]):             # the framebuffer, and the depth map if there is one
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %d values differ" % (what, int((a != b).sum()))
    assert counts(off[-1]) == counts(on[-1]), what


@pytest.mark.parametrize("size", [(240, 135), (64, 36)])
def test_benchmark_scene_four_bounces(gpu, size):
    """-l 4: both banks of the shadow answers are used twice.  64x36 is less than one row of workgroups."""
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    off, on = off_and_on(gpu, size[0], size[1], 4)
    assert on[-1].levels == 4 and on[-1].rays_shadow > 0
    assert_same(off, on)


def test_facing_mirrors_reuse_the_banks_many_times(gpu):
    g = golden("zoo3d_mirror")
    gpu.upload_scene(g.scene)
    off, on = off_and_on(gpu, 64, 36, g.depth)
    assert on[-1].levels > 8
    assert_same(off, on)


@pytest.mark.parametrize("depth", [1, 2])
def test_one_and_two_bounces(gpu, depth):
    """-l 1: no lighting launch leaves the main stream; -l 2: exactly one does."""
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    off, on = off_and_on(gpu, 64, 36, depth)
    assert on[-1].levels == depth
    assert_same(off, on)


@pytest.mark.parametrize("name,samples", [("al_zoo4d", 1), ("ns_c3_random4d", 4)])
def test_stochastic_renders(gpu, name, samples):
    """Area lights / -n samples > 1: the lighting takes the node's random stream (rng_key) and its light window's base."""
    g = golden(name)
    gpu.upload_scene(g.scene)
    off, on = off_and_on(gpu, 64, 36, g.depth, samples=samples)
    assert_same(off, on, name)


def test_with_a_depth_map(gpu):
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    off, on = off_and_on(gpu, 64, 36, 4, depth_map=True)
    assert len(on) == 3 and on[1].max() > 0.0
    assert_same(off, on)


def test_row_shard(gpu):
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    off, on = off_and_on(gpu, 64, 36, 4, row_begin=1, row_step=2)
    assert on[0].shape[0] == 18
    assert_same(off, on)


def test_overflow_rerender_with_the_light_stream_in_use(gpu):
    """A fresh context whose first node pool is too small: the frame overflows with lighting on the light stream, the pools
    are grown and the frame is rendered again."""
    from ndt_amd.hip import NdtHip
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    gpu.set_option("light_overlap", 0)
    want = gpu.render(240, 135, 4)
    small = NdtHip(0)
    try:
        small.set_option("pipeline", 1)
        small.set_option("light_overlap", 1)
        small.set_option("test_small_pool", 1)
        small.upload_scene(g.scene)
        got = small.render(240, 135, 4)
        again = small.render(240, 135, 4)
    finally:
        small.close()
    assert want[-1].rays_secondary > 64                 # the small pool (primaries + 64 nodes) cannot hold them
    assert got[-1].node_capacity >= want[-1].rays_primary + want[-1].rays_secondary
    assert_same(want, got, "first frame")
    assert_same(want, again, "second frame")


def test_thirty_frames_in_a_row(gpu):
    """An ordering edge between the two streams that is missing shows as a frame that differs now and then."""
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    gpu.set_option("light_overlap", 0)
    want = gpu.render(240, 135, 4)
    gpu.set_option("light_overlap", 1)
    for k in range(30):
        assert_same(want, gpu.render(240, 135, 4), "frame %d" % k)
