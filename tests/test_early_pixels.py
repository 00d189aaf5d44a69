"""Option "early_pixels" of the per-bounce pipeline: the pixels of primaries that are final long before the end of the frame --
part 1, the ones that missed; part 2, the hit ones without a child -- are finished on the light stream beside the trace
launches, and the frame's last launch takes the parts that were not launched early.  It changes WHICH
launch writes a pixel and when, never what is written: every frame below is rendered with the option at 0, 1 and 2, and the
framebuffers (and depth maps) must be the same bytes and the ray counts equal.

pipeline = 1 everywhere: `auto` renders passes this small with the frame kernel, which finishes its own pixels.
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


def all_three(gpu, *args, **kw):
    """The same render with early_pixels 0, 1 and 2: what each returned."""
    res = []
    for opt in (0, 1, 2):
        gpu.set_option("early_pixels", opt)
        res.append(gpu.render(*args, **kw))
    return res


def assert_same(want, got, what=""):
    assert len(want) == len(got)
    for a, b in zip(want[:-1], got[:-1]):           # the framebuffer, and the depth map if there is one
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %d values differ" % (what, int((a != b).sum()))
    assert counts(want[-1]) == counts(got[-1]), what


def assert_all_same(res, what=""):
    for opt in (1, 2):
        assert_same(res[0], res[opt], "%s early_pixels %d" % (what, opt))


def missed_primaries(gpu, *args, **kw):
    """How many primaries of the frame hit nothing: their entry of the depth map is 0, a hit's is 1 / distance."""
    gpu.set_option("early_pixels", 0)
    _, dm, _ = gpu.render(*args, depth_map=True, **kw)
    return int((dm == 0.0).sum()), dm.size


@pytest.mark.parametrize("size", [(240, 135), (100, 52)])
def test_benchmark_scene_has_all_three_parts(gpu, size):
    """-l 4.  100x52 is no multiple of the 8x8 tiles: its padding slots (depth_left <= 0) belong to no pixel."""
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    missed, total = missed_primaries(gpu, size[0], size[1], 4)
    assert 0 < missed < total                           # part 1 and hit primaries
    res = all_three(gpu, size[0], size[1], 4)
    assert res[0][-1].levels == 4 and res[0][-1].rays_secondary > 0     # pixels with children: part 0
    assert_all_same(res)


def test_a_frame_whose_primaries_all_hit(gpu):
    """The 3-D scene: part 1 is empty.  The rows above its horizon see the background at every frame size (the top 8 of 36), so
    the frame is rows 12 .. 35 of the 64x36 one: 64x24 primaries, every one of them a hit."""
    g = golden("c1_hypercube3d")
    gpu.upload_scene(g.scene)
    missed, total = missed_primaries(gpu, 64, 36, g.depth, row_begin=12, row_step=1)
    assert missed == 0 and total == 64 * 24
    res = all_three(gpu, 64, 36, g.depth, row_begin=12, row_step=1)
    assert res[0][-1].rays_secondary > 0
    assert_all_same(res)


@pytest.mark.parametrize("depth", [1, 2])
def test_one_and_two_bounces(gpu, depth):
    """-l 1: the loop never waits for bounce 1, nothing is launched early and the final launch takes every pixel.  -l 2: the lighting
    of the primaries leaves the main stream only behind the last trace launch."""
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    res = all_three(gpu, 64, 36, depth)
    assert res[0][-1].levels == depth
    assert_all_same(res)


def test_facing_mirrors(gpu):
    """Many bounces, and children that were cut off (-2): those primaries stay with the final launch."""
    g = golden("zoo3d_mirror")
    gpu.upload_scene(g.scene)
    res = all_three(gpu, 64, 36, g.depth)
    assert res[0][-1].levels > 8
    assert_all_same(res)


def test_with_a_depth_map(gpu):
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    res = all_three(gpu, 64, 36, 4, depth_map=True)
    assert len(res[2]) == 3 and res[2][1].max() > 0.0 and res[2][1].min() == 0.0
    assert_all_same(res)


def test_row_shard(gpu):
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    res = all_three(gpu, 64, 36, 4, row_begin=1, row_step=2)
    assert res[2][0].shape[0] == 18
    assert_all_same(res)


def test_stochastic_render(gpu):
    g = golden("ns_c3_random4d")
    gpu.upload_scene(g.scene)
    assert_all_same(all_three(gpu, 64, 36, g.depth, samples=4))


def test_every_pixel_is_written(gpu):
    """Into a buffer full of NaN: whoever finishes a pixel, every one of them is written, with the bytes of the option-0 frame."""
    import torch
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    w, h = 100, 52
    buf = torch.empty(h * w * 4, dtype=torch.float64, device="cuda")
    frames, stats = [], []
    for opt in (0, 1, 2):
        gpu.set_option("early_pixels", opt)
        buf.fill_(float("nan"))
        torch.cuda.synchronize()
        stats.append(gpu.render_device(buf.data_ptr(), w, h, 4))
        torch.cuda.synchronize()
        frames.append(buf.cpu().numpy().copy())
    for opt in (0, 1, 2):
        assert not np.isnan(frames[opt]).any(), "early_pixels %d left %d values unwritten" % (opt, int(np.isnan(frames[opt]).sum()))
        assert frames[opt].tobytes() == frames[0].tobytes(), "early_pixels %d" % opt
        assert counts(stats[opt]) == counts(stats[0])


@pytest.mark.parametrize("opt", [1, 2])
def test_overflow_rerender_with_early_launches_in_flight(gpu, opt):
    """A fresh context whose first node pool is too small: the first attempt runs to its end with its early launches (the overflow
    is read from the closing record, behind the join), writes the caller's buffer, and is thrown away; the pools are grown and the
    second attempt, early launches and all, renders the frame over it."""
    from ndt_amd.hip import NdtHip
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    gpu.set_option("early_pixels", 0)
    want = gpu.render(240, 135, 4)
    small = NdtHip(0)
    try:
        small.set_option("pipeline", 1)
        small.set_option("early_pixels", opt)
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
    gpu.set_option("early_pixels", 0)
    want = gpu.render(240, 135, 4)
    gpu.set_option("early_pixels", 2)
    for k in range(30):
        assert_same(want, gpu.render(240, 135, 4), "frame %d" % k)


def test_without_light_overlap_the_option_does_nothing(gpu):
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    gpu.set_option("light_overlap", 0)
    try:
        res = all_three(gpu, 240, 135, 4)
    finally:
        gpu.set_option("light_overlap", 1)
    assert_all_same(res)
    assert res[1][-1].trace_launches == res[0][-1].trace_launches == res[2][-1].trace_launches
