"""Regular K x K supersampling of a frame on the device (ndt_ssaa.hip; `ndt_hip --ssaa K`).

The yardstick is numpy's restatement of the definition: the W x H frame is the K W x K H frame of the same scene and camera, and
per channel out = (((s[0][0] + s[0][1]) + ... + s[0][K-1]) + s[1][0] + ... + s[K-1][K-1]) / (double)(K * K), summed strictly
left to right, sub-row outer, sub-column inner.  The large frame is the device's own plain render (bit for bit) and the
reference's golden framebuffer (to the 1e-9 the project uses for framebuffers).
"""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, golden

from ndt_amd import hip as nh
from ndt_amd import RenderStats

NDT_E_INVALID = -1
HOST = os.path.join(ROOT, "ndt_amd", "host")
DRIVER = os.path.join(HOST, "ndt_hip")
NEW_SYMBOLS = ("ndt_hip_ssaa_fold_device", "ndt_hip_render_ssaa_device", "ndt_hip_render_ssaa", "ndt_hip_render_ssaa_rgba8",
               "ndt_hip_render_ssaa_png", "ndt_hip_render_ssaa_jpeg", "ndt_hip_render_ssaa_rgba8_depth", "ndt_hip_ssaa_launches",
               "ndt_hip_ssaa_ms")


# ---------------------------------------------------------------- the yardstick

def fold_model(big, k):
    """The definition, one addition at a time: big is (k * rows, k * width, 4), the result (rows, width, 4)."""
    big = np.ascontiguousarray(big, dtype=np.float64)
    rows, width = big.shape[0] // k, big.shape[1] // k
    assert big.shape == (rows * k, width * k, 4)
    s = big.reshape(rows, k, width, k, 4)
    acc = s[:, 0, :, 0].copy()
    for a in range(k):
        for b in range(k):
            if a or b:
                acc = acc + s[:, a, :, b]
    return acc / np.float64(k * k)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def read_png(data):
    """The pixels [h, w, 4] of an 8-bit RGBA PNG with filters 0 / 1 / 2 (the reader of tests/test_png_device.py)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert zlib.crc32(typ + body) == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0], typ
        if typ == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)
    out = np.zeros((h, w, 4), dtype=np.uint8)
    for r in range(h):
        row = raw[r, 1:].reshape(w, 4)
        if raw[r, 0] == 1:
            row = np.cumsum(row, axis=0, dtype=np.uint8)
        elif raw[r, 0] == 2 and r > 0:
            row = row + out[r - 1]
        out[r] = row
    return out


# ---------------------------------------------------------------- CPU

def test_declared_bound_and_exported():
    """(CPU) the header declares every new entry point, hip.py binds it, the library exports it."""
    with open(os.path.join(ROOT, "include", "ndt_hip.h")) as f:
        header = f.read()
    lib = nh.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"^(int|double) %s\(" % name, header, re.M), name
        assert name in nh.API_SYMBOLS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.ndt_hip_ssaa_ms.restype is C.c_double
    assert lib.ndt_hip_abi_version() == 3
    for method in ("ssaa_fold_device", "render_ssaa", "render_ssaa_device", "render_ssaa_rgba8", "render_ssaa_png", "render_ssaa_jpeg",
                   "render_ssaa_rgba8_depth", "ssaa_launches", "ssaa_ms"):
        assert callable(getattr(nh.NdtHip, method)), method


@pytest.mark.parametrize("k", [2, 3])
def test_sub_sample_00_is_the_plain_frame(oracle, k):
    """(CPU) the flattened scene does not depend on the resolution, and pixel (i, j) of the W x H frame is sampled where pixel
    (K i, K j) of the K W x K H frame is: the oracle's 96 / K frame is every K-th pixel of the 96 x 96 fixture, bit for bit."""
    g = golden("c1_hypercube3d")
    assert (g.width, g.height) == (96, 96)
    out, _ = oracle.render(g.scene, 96 // k, 96 // k, g.depth)
    assert np.array_equal(bits(out), bits(g.data["fb"][::k, ::k]))


def test_the_model_sums_in_order():
    """(CPU) on blocks holding 1e16, 1, -1e16, 1, where the order matters, the model gives the hand-computed value, and np.mean
    and the column-first order give others: the comparisons below can tell orders apart."""
    block = np.array([1e16, 1.0, -1e16, 1.0])
    big = np.zeros((2, 2, 4))
    big[..., 0] = block.reshape(2, 2)
    big[..., 1] = -0.0
    big[..., 2] = [[0.5, 0.25], [2.0, -1.0]]
    got = fold_model(big, 2)[0, 0]
    # ((1e16 + 1) + -1e16) + 1: the first 1 is lost in 1e16 (its ulp is 2), the second survives
    assert got[0] == 1.0 / 4.0 and got[0] == (((1e16 + 1.0) + -1e16) + 1.0) / 4.0
    # taken column by column -- the mean over the sub-rows first -- the same block gives (1e16 + -1e16) and (1 + 1): 2 / 4
    assert got[0] != block.reshape(2, 2).mean(axis=0).mean() == 0.5
    # np.mean of a 4 x 4 block holding the same four values: numpy adds sixteen numbers in eight interleaved partial sums,
    # the model one after the other -- every 1 that meets 1e16 is lost (its ulp is 2), the one that meets 0 survives, so the
    # sequential sum ends as the last 1
    big4 = np.zeros((4, 4, 4))
    big4[..., 0] = np.resize(block, 16).reshape(4, 4)
    want = 0.0
    for x in np.resize(block, 16):
        want = want + x
    assert want == 1.0 and fold_model(big4, 4)[0, 0, 0] == 1.0 / 16.0
    assert np.mean(big4[..., 0]) != 1.0 / 16.0
    assert bits(got[1]) == bits(-0.0)                                   # the first sample starts the sum: no 0.0 + -0.0
    assert got[2] == (((0.5 + 0.25) + 2.0) + -1.0) / 4.0 == 0.4375
    # three sub-samples a side, one pixel: ((((((((1 + 2) + 3) + 4) + 5) + 6) + 7) + 8) + 9) / 9
    big3 = np.arange(1.0, 10.0).reshape(3, 3, 1).repeat(4, axis=2)
    assert fold_model(big3, 3)[0, 0, 0] == 45.0 / 9.0
    # the sub-row is the outer loop: rows of the large frame, not columns, are taken first
    t = np.zeros((2, 2, 4))
    t[0, 1, 0], t[1, 0, 0], t[1, 1, 0], t[0, 0, 0] = 1e16, 1.0, -1e16, 1.0
    assert fold_model(t, 2)[0, 0, 0] == (((1.0 + 1e16) + 1.0) + -1e16) / 4.0 == 0.0


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


def _hand_made(k, width, rows):
    """A large frame of doubles of mixed magnitude and sign (values below 0 and above 1 among them), with the order-sensitive
    block in channel 0 of pixel 0 and a pixel channel of -0.0."""
    rng = np.random.default_rng(1000 * k + 10 * width + rows)
    big = rng.standard_normal((rows * k, width * k, 4)) * 10.0 ** rng.integers(-8, 9, (rows * k, width * k, 4))
    big[:k, :k, 0] = np.resize(np.array([1e16, 1.0, -1e16, 1.0]), k * k).reshape(k, k)
    big[:k, :k, 1] = -0.0
    big[-1, -1, 2] = 0.0
    return big


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("width", [1, 7, 64, 65, 257])
@pytest.mark.parametrize("k", [2, 3, 4, 5, 8])
def test_fold_known_answers(gpu, oracle, k, width, rows):
    """ndt_hip_ssaa_fold_device, pass after pass, against the model bit for bit; the bytes of the last pass are oracle.quantize of
    the result, and no earlier pass touches them.  Widths under, at and over a workgroup's 128 pixels and a wavefront's 32."""
    import torch
    big = _hand_made(k, width, rows)
    want = fold_model(big, k)
    assert (big < 0).any() and (big > 1).any()
    acc = torch.full((rows * width * 4 + 64,), -7.0, dtype=torch.float64, device="cuda")
    rgba8 = torch.full((rows * width * 4 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    for a in range(k):
        sub_row = torch.from_numpy(np.ascontiguousarray(big[a::k])).cuda()
        torch.cuda.synchronize()
        gpu.ssaa_fold_device(sub_row.data_ptr(), acc.data_ptr(), width, rows, k, a, rgba8.data_ptr())
        assert gpu.ssaa_launches() == 1
        if a < k - 1:
            assert (rgba8.cpu().numpy() == 0xA5).all()              # the planted pattern survives the earlier passes
    got = acc.cpu().numpy()
    assert (got[rows * width * 4:] == -7.0).all()
    got = got[:rows * width * 4].reshape(rows, width, 4)
    assert np.array_equal(bits(got), bits(want))
    assert bits(got[0, 0, 1]) == bits(-0.0)
    got8 = rgba8.cpu().numpy()
    assert (got8[rows * width * 4:] == 0xA5).all()
    assert np.array_equal(got8[:rows * width * 4].reshape(rows, width, 4), oracle.quantize(want))
    # without an image asked for, the doubles are the same
    acc2 = torch.zeros(rows * width * 4, dtype=torch.float64, device="cuda")
    for a in range(k):
        sub_row = torch.from_numpy(np.ascontiguousarray(big[a::k])).cuda()
        torch.cuda.synchronize()
        gpu.ssaa_fold_device(sub_row.data_ptr(), acc2.data_ptr(), width, rows, k, a)
    assert np.array_equal(bits(acc2.cpu().numpy().reshape(rows, width, 4)), bits(want))


@pytest.mark.gpu
def test_fold_refuses_bad_arguments(gpu):
    import torch
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    lib, p = gpu.lib, buf.data_ptr()
    ok = (gpu.ctx, C.c_void_p(p), C.c_void_p(p + 16384), 4, 2, 2, 0, None)
    for at, bad in ((0, None), (1, None), (2, None), (3, 0), (4, 0), (5, 0), (5, 9), (6, 2), (6, -1), (1, C.c_void_p(p + 8)),
                    (2, C.c_void_p(p + 8))):
        args = list(ok)
        args[at] = bad
        assert lib.ndt_hip_ssaa_fold_device(*args) == NDT_E_INVALID, (at, bad)
    assert (buf.cpu().numpy() == 0).all()


FRAMES = [("c1_hypercube3d", 2), ("c1_hypercube3d", 3), ("c1_hypercube3d", 4), ("c3_random4d", 2)]
_plain = {}


def _plain_frame(gpu, name, pipeline=0):
    """The device's own plain render of a fixture at its golden size (rendered once per pipeline, never modified)."""
    if (name, pipeline) not in _plain:
        g = golden(name)
        gpu.upload_scene(g.scene)
        gpu.set_option("pipeline", pipeline)
        try:
            out, st = gpu.render(g.width, g.height, g.depth)
        finally:
            gpu.set_option("pipeline", 0)
        out.setflags(write=False)
        _plain[(name, pipeline)] = (out, int(st.rays_ref_equiv))
    return _plain[(name, pipeline)]


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [0, 1, 2], ids=["auto", "levels", "stream"])
@pytest.mark.parametrize("name,k", FRAMES)
def test_frame_is_the_fold_of_the_devices_large_frame(gpu, name, k, pipeline):
    g = golden(name)
    assert g.width % k == 0 and g.height % k == 0
    big, rays = _plain_frame(gpu, name, pipeline)
    gpu.upload_scene(g.scene)
    gpu.set_option("pipeline", pipeline)
    try:
        got, st = gpu.render_ssaa(g.width // k, g.height // k, g.depth, k)
    finally:
        gpu.set_option("pipeline", 0)
    assert np.array_equal(bits(got), bits(fold_model(big, k)))
    assert st.rays_ref_equiv == rays
    assert gpu.ssaa_launches() == k
    # either pipeline gives the same bits
    assert np.array_equal(bits(big), bits(_plain_frame(gpu, name, 0)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,k", FRAMES)
def test_frame_against_the_reference(gpu, oracle, name, k):
    """The model applied to the reference's framebuffer: 1e-9 is the tolerance the project uses for framebuffers (an average of
    values that each agree to it agrees to it); a byte may fall on the other side of an integer of sqrt(x) * 255, never further."""
    g = golden(name)
    want = fold_model(g.data["fb"], k)
    gpu.upload_scene(g.scene)
    got, _ = gpu.render_ssaa(g.width // k, g.height // k, g.depth, k)
    err = float(np.abs(got - want).max())
    got8, _ = gpu.render_ssaa_rgba8(g.width // k, g.height // k, g.depth, k)
    want8 = oracle.quantize(want)
    step = np.abs(got8.astype(np.int16) - want8.astype(np.int16))
    print("%s ssaa %d: max |gpu - folded reference| = %.3g; %d of %d bytes differ from the quantised fold of the reference (largest step %d)"
          % (name, k, err, int((step != 0).sum()), want8.size, int(step.max())))
    assert err <= 1e-9
    assert step.max() <= 1
    assert np.array_equal(got8, oracle.quantize(got))


@pytest.mark.gpu
@pytest.mark.parametrize("row_begin,row_step", [(0, 1), (1, 3), (2, 3)])
def test_row_shards(gpu, row_begin, row_step):
    g = golden("c1_hypercube3d")
    gpu.upload_scene(g.scene)
    full, _ = gpu.render_ssaa(48, 48, g.depth, 2)
    part, _ = gpu.render_ssaa(48, 48, g.depth, 2, row_begin=row_begin, row_step=row_step)
    assert part.shape[0] == len(range(row_begin, 48, row_step))
    assert np.array_equal(bits(part), bits(full[row_begin::row_step]))
    part8, _ = gpu.render_ssaa_rgba8(48, 48, g.depth, 2, row_begin=row_begin, row_step=row_step)
    assert np.array_equal(part8, gpu.render_ssaa_rgba8(48, 48, g.depth, 2)[0][row_begin::row_step])


@pytest.mark.gpu
def test_k_1_is_the_plain_frame(gpu):
    g = golden("c1_hypercube3d")
    gpu.upload_scene(g.scene)
    want, st = gpu.render(g.width, g.height, g.depth)
    got, st1 = gpu.render_ssaa(g.width, g.height, g.depth, 1)
    assert np.array_equal(bits(got), bits(want))
    assert st1.rays_ref_equiv == st.rays_ref_equiv and gpu.ssaa_launches() == 0
    assert np.array_equal(bits(gpu.render(g.width, g.height, g.depth, ssaa=1)[0]), bits(want))
    assert np.array_equal(gpu.render_ssaa_rgba8(g.width, g.height, g.depth, 1)[0], gpu.render_rgba8(g.width, g.height, g.depth)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name,stereo", [("st_zoo4d_sbs", 1), ("st_zoo4d_sbs", 2), ("st_zoo3d_anaglyph", 3)],
                         ids=["side_by_side", "over_under", "anaglyph"])
def test_stereo_frames(gpu, name, stereo):
    g = golden(name)
    assert g.width % 4 == 0 and g.height % 4 == 0
    gpu.upload_scene(g.scene)
    big, st = gpu.render(g.width, g.height, g.depth, stereo=stereo)
    got, st2 = gpu.render_ssaa(g.width // 2, g.height // 2, g.depth, 2, stereo=stereo)
    assert np.array_equal(bits(got), bits(fold_model(big, 2)))
    assert st2.rays_ref_equiv == st.rays_ref_equiv


@pytest.mark.gpu
def test_stochastic_frames_are_the_large_frames(gpu):
    """samples > 1: the sampler's streams are functions of the pixel id, so the frame is still defined by the large frame."""
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    big, _ = gpu.render(64, 36, g.depth, samples=3)
    got, _ = gpu.render_ssaa(32, 18, g.depth, 2, samples=3)
    assert np.array_equal(bits(got), bits(fold_model(big, 2)))


@pytest.mark.gpu
def test_refusals_name_the_cause_and_write_nothing(gpu):
    g = golden("st_zoo4d_sbs")
    gpu.upload_scene(g.scene)
    out = np.full((18, 32, 4), -7.0)
    dm = np.full((18, 32), -7.0)
    out8 = np.full((18, 32, 4), 0xA5, dtype=np.uint8)
    st = RenderStats()

    def refused(words, k=2, width=32, height=18, rgba=out, **kw):
        p = gpu.params(width, height, g.depth, **kw)
        rc = gpu.lib.ndt_hip_render_ssaa(gpu.ctx, C.byref(p), k, rgba.ctypes.data if rgba is not None else None, dm.ctypes.data, C.byref(st))
        text = gpu.lib.ndt_hip_last_error().decode()
        assert rc == NDT_E_INVALID, (words, rc, text)
        for w in words:
            assert w in text, (words, text)
        if rgba is not None:
            assert gpu.lib.ndt_hip_render_ssaa_rgba8(gpu.ctx, C.byref(p), k, out8.ctypes.data, C.byref(st)) == NDT_E_INVALID
        assert (out == -7.0).all() and (dm == -7.0).all() and (out8 == 0xA5).all()

    refused(("NDT_STEREO_HIDEF", "not scalable"), stereo=4)
    refused(("recursive_aa",), aa=(20, 2))
    refused(("factor 0", "1 .. 8"), k=0)
    refused(("factor 9", "1 .. 8"), k=9)
    refused(("NULL",), rgba=None)
    refused(("side by side", "odd width"), width=31, stereo=1)
    refused(("over/under", "odd height"), height=17, stereo=2)
    refused(("INT32_MAX",), k=8, width=2 ** 29)
    with pytest.raises(nh.NdtHipError) as e:
        gpu.render(32, 18, g.depth, aa=(20, 2), ssaa=2)
    assert e.value.code == NDT_E_INVALID and "recursive_aa" in str(e.value)
    p = gpu.params(32, 18, g.depth)
    assert gpu.lib.ndt_hip_render_ssaa(None, C.byref(p), 2, out.ctypes.data, None, None) == NDT_E_INVALID
    assert gpu.lib.ndt_hip_render_ssaa(gpu.ctx, None, 2, out.ctypes.data, None, None) == NDT_E_INVALID
    assert gpu.lib.ndt_hip_render_ssaa_device(gpu.ctx, C.byref(p), 2, None, None, None) == NDT_E_INVALID
    assert gpu.lib.ndt_hip_render_ssaa_png(gpu.ctx, C.byref(p), 2, None, 0, None, None) == NDT_E_INVALID
    assert gpu.lib.ndt_hip_render_ssaa_jpeg(gpu.ctx, C.byref(p), 2, None, None, 0, None, None) == NDT_E_INVALID
    assert gpu.lib.ndt_hip_render_ssaa_rgba8_depth(gpu.ctx, C.byref(p), 2, out8.ctypes.data, None, None, None) == NDT_E_INVALID
    assert (out == -7.0).all() and (out8 == 0xA5).all()


@pytest.mark.gpu
def test_depth_map_is_the_plain_frames(gpu):
    import torch
    g = golden("depth_c3_random4d")
    assert (g.width, g.height) == (64, 36)
    gpu.upload_scene(g.scene)
    _, want_dm, _ = gpu.render(32, 18, g.depth, depth_map=True)
    big, big_dm, _ = gpu.render(64, 36, g.depth, depth_map=True)
    got, dm, _ = gpu.render_ssaa(32, 18, g.depth, 2, depth_map=True)
    assert (want_dm > 0).any()
    assert np.array_equal(bits(dm), bits(want_dm))
    assert np.array_equal(bits(dm), bits(big_dm[::2, ::2]))
    assert np.array_equal(bits(got), bits(fold_model(big, 2)))
    assert np.array_equal(bits(gpu.render(32, 18, g.depth, depth_map=True, ssaa=2)[1]), bits(want_dm))
    # the finished map: ndt_hip_depth_rgba8_device applied to it
    rgba8, depth8, rng, _ = gpu.render_ssaa_rgba8_depth(32, 18, g.depth, 2)
    d_dm = torch.from_numpy(dm).cuda()
    d_out = torch.zeros(dm.size * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    want_rng = gpu.depth_rgba8_device(d_dm.data_ptr(), dm.size, d_out.data_ptr())
    assert np.array_equal(depth8, d_out.cpu().numpy().reshape(18, 32, 4))
    assert bits(rng).tolist() == bits(want_rng).tolist()
    assert np.array_equal(rgba8, gpu.render_ssaa_rgba8(32, 18, g.depth, 2)[0])


@pytest.mark.gpu
def test_device_pointers(gpu):
    """ndt_hip_render_ssaa_device: the image and the map left in HBM are the host call's, and nothing is written behind them."""
    import torch
    g = golden("depth_c3_random4d")
    gpu.upload_scene(g.scene)
    want, want_dm, _ = gpu.render_ssaa(32, 18, g.depth, 3, depth_map=True, row_begin=1, row_step=2)
    rows = want.shape[0]
    d_out = torch.full((rows * 32 * 4 + 64,), -7.0, dtype=torch.float64, device="cuda")
    d_dm = torch.full((rows * 32 + 64,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_ssaa_device(d_out.data_ptr(), 32, 18, g.depth, 3, d_depth_ptr=d_dm.data_ptr(), row_begin=1, row_step=2)
    out, dm = d_out.cpu().numpy(), d_dm.cpu().numpy()
    assert (out[rows * 32 * 4:] == -7.0).all() and (dm[rows * 32:] == -7.0).all()
    assert np.array_equal(bits(out[:rows * 32 * 4].reshape(rows, 32, 4)), bits(want))
    assert np.array_equal(bits(dm[:rows * 32].reshape(rows, 32)), bits(want_dm))


@pytest.mark.gpu
def test_files(gpu, oracle):
    g = golden("c1_hypercube3d")
    big, _ = _plain_frame(gpu, "c1_hypercube3d")
    gpu.upload_scene(g.scene)
    want8 = oracle.quantize(fold_model(big, 2))
    got8, _ = gpu.render_ssaa_rgba8(48, 48, g.depth, 2)
    assert np.array_equal(got8, want8)
    png, _ = gpu.render_ssaa_png(48, 48, g.depth, 2)
    assert np.array_equal(read_png(png), want8)
    jpg, _ = gpu.render_ssaa_jpeg(48, 48, g.depth, 2)
    assert jpg == gpu.encode_jpeg(want8)
    jpg, _ = gpu.render_ssaa_jpeg(48, 48, g.depth, 2, quality=60, sampling="444")
    assert jpg == gpu.encode_jpeg(want8, quality=60, sampling="444")


# ---------------------------------------------------------------- driver

def _run(cwd, *flags):
    assert os.path.exists(DRIVER), "ndt_amd/host/ndt_hip is not built"
    os.makedirs(str(cwd), exist_ok=True)
    return subprocess.run([DRIVER, "-s", "builtin:yaml", "-d", "4", "-f", "0", "-l", "6"] + list(flags), capture_output=True, text=True,
                          cwd=str(cwd))


def test_driver_refuses_flag_combinations_before_anything_else(tmp_path):
    """(CPU) --ssaa beside -a and beside -m h ends the run with the reason, before a scene is loaded or a device asked for."""
    for flags, words in ((["--ssaa", "2", "-a", "20,4"], ("--ssaa", "-a")),
                         (["--ssaa", "2", "-m", "h"], ("--ssaa", "-m h", "not scalable")),
                         (["--ssaa", "9"], ("--ssaa", "1 .. 8")),
                         (["--ssaa", "two"], ("--ssaa", "1 .. 8"))):
        r = _run(tmp_path, "-r", "48x48", *flags)
        assert r.returncode != 0, flags
        for w in words:
            assert w in r.stderr, (flags, r.stderr)
    assert not list(tmp_path.rglob("*.p*"))


def read_ppm(data):
    magic, size, maxval, body = data.split(b"\n", 3)
    w, h = (int(x) for x in size.split())
    assert magic == b"P6" and maxval == b"255" and len(body) == w * h * 3
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 3)


@pytest.fixture(scope="module")
def zoo(tmp_path_factory):
    """tests/scenes/parity_zoo.c compiled against this repository's host headers, as tests/test_depth_device.py builds it."""
    import shutil
    d = tmp_path_factory.mktemp("zoo")
    (d / "scenes").mkdir()
    for h in os.listdir(os.path.join(HOST, "include")):
        os.symlink(os.path.join(HOST, "include", h), d / h)
    shutil.copy(os.path.join(ROOT, "tests", "scenes", "parity_zoo.c"), d / "scenes" / "parity_zoo.c")
    so = str(d / "scenes" / "parity_zoo.so")
    r = subprocess.run(["gcc", "-O2", "-std=c99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-o", so, str(d / "scenes" / "parity_zoo.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return so


@pytest.mark.gpu
def test_driver_writes_the_folded_frame(zoo, tmp_path, oracle):
    """`--ssaa 2 -r 48x48` writes the PPM of the fold of the driver's own 96x96 frame in doubles (--raw), and says what it did;
    over two contexts (-g 2) and as a PNG made on the GPU the pixels are the same."""
    def run(cwd, *flags):
        assert os.path.exists(DRIVER), "ndt_amd/host/ndt_hip is not built"
        os.makedirs(str(cwd), exist_ok=True)
        r = subprocess.run([DRIVER, "-s", zoo, "-d", "4", "-f", "0", "-l", "6"] + list(flags), capture_output=True, text=True, cwd=str(cwd))
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        return r

    run(tmp_path / "big", "-r", "96x96", "--raw", "fb.f64")
    big = np.fromfile(str(tmp_path / "big" / "fb.f64"), dtype=np.float64).reshape(96, 96, 4)
    want = oracle.quantize(fold_model(big, 2))
    r = run(tmp_path / "ssaa", "-r", "48x48", "--ssaa", "2")
    assert "supersampled 2x2 on GPU 0 in 2 launches" in r.stdout
    files = list((tmp_path / "ssaa" / "images").rglob("*.ppm"))
    assert len(files) == 1
    assert np.array_equal(read_ppm(files[0].read_bytes()), want[..., :3])
    r = run(tmp_path / "two", "-r", "48x48", "--ssaa", "2", "-g", "2", "--png", "--deflate", "gpu")
    assert "supersampled 2x2 on GPU 0 in 4 launches" in r.stdout
    files = list((tmp_path / "two" / "images").rglob("*.png"))
    assert len(files) == 1
    assert np.array_equal(read_png(files[0].read_bytes()), want)
    # the doubles of --raw are the fold itself
    run(tmp_path / "raw", "-r", "48x48", "--ssaa", "2", "--raw", "fb.f64")
    got = np.fromfile(str(tmp_path / "raw" / "fb.f64"), dtype=np.float64).reshape(48, 48, 4)
    assert np.array_equal(bits(got), bits(fold_model(big, 2)))
