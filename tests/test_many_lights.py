"""Scenes with more lights than one window of the lighting kernels ("Light windows"): the reference's light
list has no bound, and apply_lights sums the lights in list order into three doubles (ndt.c:98); the device path lights a node
window by window, carrying the partial sum.  Needs a real MI355X: run with `pytest -m gpu`."""
import os

import numpy as np
import pytest

from conftest import golden, GOLDEN

pytestmark = pytest.mark.gpu

TOL_SPEC = 1e-4
TOL_TIGHT = 1e-9
NDT_E_UNSUPPORTED = -2
NDT_MAX_LIGHTS = 1024


@pytest.fixture(scope="module")
def gpu():
    from ndt_amd.hip import NdtHip
    ctx = NdtHip(0)
    yield ctx
    ctx.set_option("light_window", 0)
    ctx.set_option("pipeline", 0)
    ctx.close()


def fresh(name):
    """A copy of a fixture's scene of its own (golden() shares its scene)."""
    from ndt_amd import load_scene
    return load_scene(os.path.join(GOLDEN, name + ".ndtscene.gz"))


def with_many_lights(fs, n_total, seed=1):
    """fs with lights appended until the list holds n_total: points on a lattice around the scene's own non-ambient lights,
    spots aimed like the scene's spot (or down the scene's second axis), directionals, and ambient entries at list positions 0,
    64, 65 and the end, so that windows of 64 start and end on them.  Intensities are scaled so that the sum stays near the
    scene's own."""
    rng = np.random.default_rng(seed)
    d = fs.dims
    base = [dict(l) for l in fs.lights]
    own = [l for l in base if l["type"] != 0]
    anchors = [fs.vec(l["pos_off"]) for l in own if l["pos_off"] >= 0] or [np.zeros(d)]
    dirs = [fs.vec(l["dir_off"]) for l in own if l["dir_off"] >= 0]
    down = np.zeros(d)
    down[1] = -1.0
    dirs = dirs or [down]
    spot = next((l for l in own if l["type"] == 3), None)
    point = next((l for l in own if l["type"] == 1), None)
    scale = 4.0 / n_total
    lights = list(base)
    kinds = ["point", "spot", "point", "directional", "point"]
    k = 0
    while len(lights) < n_total:
        at = len(lights)
        if at in (0, 64, 65) or at == n_total - 1:
            lights.append(dict(type=0, red=0.01, green=0.012, blue=0.008, angle=0.0, pos_off=-1, dir_off=-1, area_off=-1, radius=0.0))
            continue
        kind = kinds[k % len(kinds)]
        k += 1
        c = rng.uniform(0.5, 1.5, 3)
        if kind == "directional":
            v = dirs[k % len(dirs)] + rng.uniform(-0.3, 0.3, d)
            lights.append(dict(type=2, red=0.3 * c[0] * scale, green=0.3 * c[1] * scale, blue=0.3 * c[2] * scale, angle=0.0,
                               pos_off=-1, dir_off=fs.add_vec(list(v)), area_off=-1, radius=0.0))
            continue
        a = anchors[k % len(anchors)]
        # a lattice of lamps around the anchor, 3 units apart
        idx = np.array([(k >> (2 * j)) % 4 - 1.5 for j in range(d)])
        pos = a + 3.0 * idx + rng.uniform(-0.5, 0.5, d)
        src = spot if kind == "spot" and spot is not None else point
        red, green, blue = (src["red"], src["green"], src["blue"]) if src else (200.0, 200.0, 200.0)
        if kind == "spot":
            v = dirs[k % len(dirs)] + rng.uniform(-0.2, 0.2, d)
            lights.append(dict(type=3, red=red * c[0] * scale, green=green * c[1] * scale, blue=blue * c[2] * scale,
                               angle=float(rng.uniform(15.0, 40.0)), pos_off=fs.add_vec(list(pos)), dir_off=fs.add_vec(list(v)),
                               area_off=-1, radius=0.0))
        else:
            lights.append(dict(type=1, red=red * c[0] * scale, green=green * c[1] * scale, blue=blue * c[2] * scale, angle=0.0,
                               pos_off=fs.add_vec(list(pos)), dir_off=-1, area_off=-1, radius=0.0))
    fs.lights = lights
    fs._struct = None
    fs.finalize()
    return fs


def counts(st):
    return (st.rays_primary, st.rays_secondary, st.rays_shadow, st.rays_ref_equiv)


def same_as_oracle(out, st, want, wst, what):
    diff = np.abs(out - want)
    assert diff.max() < TOL_TIGHT, "%s: max abs diff %g" % (what, diff.max())
    assert counts(st) == counts(wst), what


@pytest.mark.parametrize("name, n_lights, w, h, depth", [
    ("zoo4d", 150, 48, 27, None),               # every object type, LDS tier
    ("zoo3d_mirror", 130, 24, 18, None),        # at the fixture's full depth
    ("c5_hypercube6d", 140, 24, 14, None),      # global-memory tier (shadow rays stored with their origins)
])
def test_many_lights_vs_oracle(gpu, oracle, name, n_lights, w, h, depth):
    """More than 64 lights, points / spots / directionals / ambients interleaved: the oracle's frame and ray counts under every
    pipeline (a scene of more than one window renders with the per-bounce kernels whatever the pipeline says)."""
    g = golden(name)
    depth = depth or g.depth
    fs = with_many_lights(fresh(name), n_lights)
    assert len(fs.lights) == n_lights
    want, wst = oracle.render(fs, w, h, depth)
    try:
        for pipeline in (0, 1, 2):
            gpu.set_option("pipeline", pipeline)
            gpu.upload_scene(fs)
            out, st = gpu.render(w, h, depth)
            same_as_oracle(out, st, want, wst, "%s, pipeline %d" % (name, pipeline))
    finally:
        gpu.set_option("pipeline", 0)


@pytest.mark.parametrize("name", ["c3_random4d", "zoo4d"])
def test_light_window_is_neutral(gpu, name):
    """light_window 1, 2, 3 (windows of that many list entries) give light_window 0's images and ray counts, byte for byte."""
    g = golden(name)
    runs = {}
    try:
        for lw in (0, 1, 2, 3):
            gpu.set_option("light_window", lw)
            gpu.upload_scene(g.scene)
            runs[lw] = gpu.render(g.width, g.height, g.depth)
    finally:
        gpu.set_option("light_window", 0)
    for lw in (1, 2, 3):
        assert np.array_equal(runs[lw][0], runs[0][0]), "light_window %d" % lw
        assert counts(runs[lw][1]) == counts(runs[0][1]), "light_window %d" % lw


def _neutral(gpu, scene, render):
    runs = {}
    try:
        for lw in (0, 1, 2, 3):
            gpu.set_option("light_window", lw)
            gpu.upload_scene(scene)
            runs[lw] = render()
    finally:
        gpu.set_option("light_window", 0)
    for lw in (1, 2, 3):
        for a, b in zip(runs[lw], runs[0]):
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, b), "light_window %d" % lw
            else:
                assert counts(a) == counts(b), "light_window %d" % lw
    return runs[0]


def test_light_window_neutral_modes(gpu):
    """... and so do recursive anti-aliasing, a depth map, a stereo pair, row shards and a sampled render with area lights (whose
    random draw is keyed by the light's place in the whole list, not in its window)."""
    g = golden("c3_random4d")
    _neutral(gpu, g.scene, lambda: gpu.render(g.width, g.height, g.depth, aa=(12, 2)))
    _neutral(gpu, g.scene, lambda: gpu.render(g.width, g.height, g.depth, depth_map=True))
    _neutral(gpu, g.scene, lambda: gpu.render(g.width, g.height, g.depth, row_begin=1, row_step=3))
    z = golden("st_zoo4d_sbs")
    _neutral(gpu, z.scene, lambda: gpu.render(z.width, z.height, z.depth, stereo=z.meta["stereo"]))
    a = golden("al_zoo4d")
    try:
        gpu.set_option("sample_seed", 12345)
        _neutral(gpu, a.scene, lambda: gpu.render(a.width, a.height, a.depth, samples=3))
        _neutral(gpu, a.scene, lambda: gpu.render(a.width, a.height, a.depth))
    finally:
        gpu.set_option("sample_seed", 0)


def test_light_window_neutral_render_multi(gpu):
    from ndt_amd.hip import NdtHip, render_multi, IMAGE_F64
    g = golden("zoo4d")
    other = NdtHip(0)
    try:
        runs = {}
        for lw in (0, 2):
            for c in (gpu, other):
                c.set_option("light_window", lw)
                c.upload_scene(g.scene)
            runs[lw] = render_multi([gpu, other], g.width, g.height, g.depth, IMAGE_F64)
        assert np.array_equal(runs[2][0], runs[0][0])
        assert counts(runs[2][1]) == counts(runs[0][1])
    finally:
        gpu.set_option("light_window", 0)
        other.close()


def test_more_trace_launches_than_work_queues(gpu, oracle):
    """light_window 1 on a mirror scene with ten non-ambient lights and 60+ bounces: more trace launches than a render call has
    work queues (NDT_QUEUE_SLOTS), which are used again."""
    g = golden("zoo3d_mirror")
    fs = with_many_lights(fresh("zoo3d_mirror"), 12, seed=3)
    assert sum(1 for l in fs.lights if l["type"] != 0) >= 10
    w, h = 16, 12
    want, wst = oracle.render(fs, w, h, g.depth)
    try:
        gpu.set_option("light_window", 1)
        gpu.upload_scene(fs)
        out, st = gpu.render(w, h, g.depth, profile=1)
    finally:
        gpu.set_option("light_window", 0)
    same_as_oracle(out, st, want, wst, "zoo3d_mirror, light_window 1")
    assert st.levels >= 60, st.levels
    assert st.trace_launches > 512, st.trace_launches


def test_light_limit(gpu, oracle):
    """NDT_MAX_LIGHTS lights upload and render; one more is refused by name."""
    from ndt_amd.hip import NdtHipError
    g = golden("c3_random4d")
    fs = with_many_lights(fresh("c3_random4d"), NDT_MAX_LIGHTS, seed=5)
    want, wst = oracle.render(fs, 16, 9, 3)
    gpu.upload_scene(fs)
    out, st = gpu.render(16, 9, 3)
    same_as_oracle(out, st, want, wst, "%d lights" % NDT_MAX_LIGHTS)
    fs = with_many_lights(fresh("c3_random4d"), NDT_MAX_LIGHTS + 1, seed=5)
    with pytest.raises(NdtHipError) as e:
        gpu.upload_scene(fs)
    assert e.value.code == NDT_E_UNSUPPORTED
    assert "%d lights (max %d)" % (NDT_MAX_LIGHTS + 1, NDT_MAX_LIGHTS) in str(e.value)
    gpu.upload_scene(g.scene)
