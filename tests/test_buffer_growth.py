"""The context's grow-only device buffers (DeviceBuffer, ndt_buffer.hpp) over the three states a buffer can be in: allocated for
its first frame, replaced by a larger one, and reused while larger than the frame needs.

Every sink is called on ONE context at 16x9, then 64x36, then 16x9 again -- sixteen times apart, so that a buffer allocated with a
quarter of head room is outgrown as well -- and each answer is compared, bit for bit, with the same call on a fresh context that
has only ever seen that size: doubles through their bytes, images and files byte for byte, ray counts equal.  Needs a real
MI355X: run with `pytest -m gpu`.
"""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

SIZES = [(16, 9), (64, 36), (16, 9)]


def frozen(x):
    """What of an answer is compared: arrays as (dtype, shape, bytes), files as they are, of the statistics the ray counts."""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(frozen(y) for y in x)
    if hasattr(x, "rays_ref_equiv"):
        return (x.rays_primary, x.rays_secondary, x.rays_shadow, x.rays_ref_equiv)
    assert isinstance(x, bytes), type(x)
    return x


class Sink:
    """One way to call a context: `scene` is the golden case uploaded before the first call (None: none), `steps` what the
    three calls are given, `call(gpu, g, step)` the call."""

    def __init__(self, name, call, scene="c3_random4d", steps=SIZES, options=()):
        self.name, self.call, self.scene, self.steps, self.options = name, call, scene, steps, options

    def context(self):
        from ndt_amd.hip import NdtHip
        gpu = NdtHip(0)
        for name, value in self.options:
            gpu.set_option(name, value)
        g = golden(self.scene) if self.scene else None
        if g:
            gpu.upload_scene(g.scene)
        return gpu, g


def frames(method, **kw):
    return lambda gpu, g, wh: getattr(gpu, method)(wh[0], wh[1], g.depth, **kw)


def async_frames(gpu, g, wh):
    """two frames a size: both device buffers of ndt_hip_render_rgba8_async turn over"""
    import torch
    w, h = wh
    bufs = [torch.empty((h, w, 4), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    stats = [gpu.render_rgba8_async(b.data_ptr(), w, h, g.depth) for b in bufs]
    gpu.render_rgba8_wait()
    return [b.numpy().copy() for b in bufs], stats


def multi_frame(gpu, g, wh):
    from ndt_amd.hip import render_multi, IMAGE_F64
    return render_multi([gpu], wh[0], wh[1], g.depth, fmt=IMAGE_F64)


def fitted(gpu, g, n_lists):
    rng = np.random.default_rng(5)
    lists = [(rng.uniform(-3, 3, (8, 3)), rng.uniform(0.1, 1.0, 8)) for _ in range(n_lists)]
    return gpu.fit_spheres(3, lists)


def uploaded(gpu, g, name):
    other = golden(name)
    gpu.upload_scene(other.scene)
    return gpu.render(16, 9, other.depth)


AA = golden("aa_c3_random4d").meta
NS = golden("ns_zoo3d_anaglyph").meta

SINKS = [
    Sink("render_depth", frames("render", depth_map=True)),                                 # d_out
    Sink("render_rgba8", frames("render_rgba8")),                                           # d_shard, d_image
    Sink("render_rgba8_async", async_frames),                                               # d_shard, d_rgba8[2]
    Sink("render_png", frames("render_png")),
    Sink("render_png16", frames("render_png16")),
    Sink("render_png_depth", frames("render_png_depth")),
    Sink("render_png16_depth", frames("render_png16_depth")),
    Sink("render_jpeg", frames("render_jpeg")),
    Sink("render_rgba8_depth", frames("render_rgba8_depth")),
    Sink("render_ssaa", frames("render_ssaa", ssaa=2, depth_map=True)),
    Sink("render_ssaa_rgba8", frames("render_ssaa_rgba8", ssaa=2)),
    Sink("render_ssaa_png16", frames("render_ssaa_png16", ssaa=2, depth_map=True)),
    Sink("render_ssaa_png", frames("render_ssaa_png", ssaa=2)),
    Sink("render_ssaa_jpeg", frames("render_ssaa_jpeg", ssaa=2)),
    Sink("render_ssaa_rgba8_depth", frames("render_ssaa_rgba8_depth", ssaa=2)),
    Sink("render_ssaa_exr", frames("render_ssaa_exr", ssaa=2, depth_map=True)),
    Sink("render_exr", frames("render_exr", depth_map=True)),
    Sink("render_denoised", frames("render_denoised")),
    Sink("render_denoised_rgba8", frames("render_denoised", sink="rgba8")),
    Sink("render_denoised_png", frames("render_denoised", sink="png")),
    Sink("render_denoised_exr", frames("render_denoised", sink="exr")),
    Sink("render_ao_shaded", frames("render_ao_shaded", samples=4)),
    Sink("render_ao_shaded_rgba8", frames("render_ao_shaded", sink="rgba8", samples=4)),
    Sink("render_ao_shaded_jpeg", frames("render_ao_shaded", sink="jpeg", samples=4)),
    Sink("render_aa", frames("render", aa=(AA["aa_diff"], AA["aa_depth"]))),                # the AaBuffers pool
    Sink("render_multi", multi_frame),                                                      # d_image, d_shard
    Sink("fit_spheres", fitted, scene=None, steps=[4, 64, 4]),                              # d_fit
    Sink("upload_scene", uploaded, scene=None, steps=["c3_random4d", "zoo12d", "c3_random4d"]),        # d_blob
    # a stochastic render: the same streams of random numbers on every context (option "sample_seed")
    Sink("sampled_anaglyph", frames("render", samples=NS["samples"], stereo=NS["stereo"]), scene="ns_zoo3d_anaglyph",
         options=[("sample_seed", 20261)]),                                                 # d_eyes, the sampled renderer's scratch
]


@pytest.mark.parametrize("sink", SINKS, ids=[s.name for s in SINKS])
def test_a_grown_and_a_reused_buffer_give_the_frame_of_a_fresh_context(sink):
    gpu, g = sink.context()
    try:
        got = [frozen(sink.call(gpu, g, step)) for step in sink.steps]
    finally:
        gpu.close()
    want = {}
    for step in sink.steps:
        if step not in want:
            fresh, g = sink.context()
            try:
                want[step] = frozen(sink.call(fresh, g, step))
            finally:
                fresh.close()
    for k, step in enumerate(sink.steps):
        same = got[k] == want[step]             # (compared outside the assert: no report of two frames' bytes)
        assert same, "%s: call %d (%s) on the one context is not the fresh context's" % (sink.name, k + 1, step)
