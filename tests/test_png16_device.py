"""The frame and its depth map as PNG files of 16 bits a sample, made on the device (`ndt_hip --png --deflate gpu --png16`).

The reference writes 8-bit files only, so the yardsticks are Python's zlib and struct and numpy models of the definitions in
include/ndt_hip.h -- never the device's own output:
  * q16(x) = (uint16)(sqrt(m) * 65535), m = x clamped by pixel_d2c's two comparisons; a sample is stored big-endian;
  * the reader checks every chunk's CRC, inflates the IDAT with zlib and undoes filters 0 / 1 / 2 at the pixel's width;
  * the row heuristic of tests/test_png_device.py restated with the pixel's width (8 or 2 bytes) as a parameter;
  * the depth file's value is q16(hi > lo ? (d - lo) / (hi - lo) : 0) of the map's minimum and maximum.
The double framebuffers the files are compared with are those render() returns, which tests/test_gpu_parity.py pins to the
reference.
"""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, golden

from ndt_amd import hip as nh

NDT_E_INVALID, NDT_E_NOMEM = -1, -4
CHUNK = 32768
HOST = os.path.join(ROOT, "ndt_amd", "host")
DRIVER = os.path.join(HOST, "ndt_hip")
NEW_SYMBOLS = ("ndt_hip_quantize16_device", "ndt_hip_depth_grey16_device", "ndt_hip_png16_bound", "ndt_hip_encode_png16_device",
               "ndt_hip_encode_png16", "ndt_hip_render_png16", "ndt_hip_render_png16_depth", "ndt_hip_render_ssaa_png16",
               "ndt_hip_render_ssaa_png16_depth")
NEW_METHODS = ("encode_png16", "encode_png16_device", "quantize16_device", "depth_grey16_device", "render_png16", "render_png16_depth",
               "render_ssaa_png16")


# ---------------------------------------------------------------- yardsticks

def clamp01(x):
    """pixel_d2c's clamp: the same two comparisons in the same order"""
    x = np.asarray(x, dtype=np.float64)
    m = np.where(1.0 < x, 1.0, x)
    return np.where(0.0 > m, 0.0, m)


def pixel_d2c(x):
    return (np.sqrt(clamp01(x)) * 255).astype(np.uint8)


def q16(x):
    return (np.sqrt(clamp01(x)) * 65535).astype(np.uint16)


def depth_model(dm):
    """(grey samples, lo, hi) of a finite map"""
    dm = np.ascontiguousarray(dm, dtype=np.float64)
    assert np.isfinite(dm).all()
    lo, hi = dm.min(), dm.max()
    return q16((dm - lo) / (hi - lo) if hi > lo else np.zeros_like(dm)), lo, hi


def wire(samples):
    """the samples' bytes in file order: [h, bpp * w] uint8"""
    samples = np.asarray(samples, dtype=np.uint16)
    return np.ascontiguousarray(samples.astype(">u2")).view(np.uint8).reshape(samples.shape[0], -1)


def filter_rows(samples):
    """The row heuristic with bpp as a parameter: per scanline filter 0 (None), 1 (Sub: the byte bpp to the left) or 2 (Up),
    whichever has the smallest sum of |filtered byte taken as int8|, ties to the lower number, zeros above the first row.
    Returns (filters [h], the filtered stream [h, 1 + bpp w])."""
    samples = np.asarray(samples)
    bpp = 2 * (samples.shape[2] if samples.ndim == 3 else 1)
    raw = wire(samples)
    h = raw.shape[0]
    left = np.zeros_like(raw)
    left[:, bpp:] = raw[:, :-bpp]
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    cands = np.stack([raw, raw - left, raw - up])                            # uint8 arithmetic wraps
    cost = np.abs(cands.view(np.int8).astype(np.int64)).sum(axis=2)          # [3, h]
    filters = np.argmin(cost, axis=0)                                        # the first of equal minima
    stream = np.empty((h, 1 + raw.shape[1]), dtype=np.uint8)
    stream[:, 0] = filters
    stream[:, 1:] = cands[filters, np.arange(h)]
    return filters.astype(np.uint8), stream


def read_png16(data, channels):
    """(samples [h, w, 4] or [h, w] uint16, filter byte of every row, IDAT bytes) of a 16-bit PNG of colour type 6 (channels 4)
    or 0 (channels 1) with filters 0 / 1 / 2 and one IDAT."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    bpp = 2 * channels
    pos, idat, w, h, types = 8, b"", 0, 0, []
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert len(body) == n
        assert zlib.crc32(typ + body) == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0], typ
        types.append(typ)
        if typ == b"IHDR":
            w, h, bits, colour, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            assert (bits, colour, comp, filt, lace) == (16, 6 if channels == 4 else 0, 0, 0, 0)
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    assert pos == len(data) and types == [b"IHDR", b"IDAT", b"IEND"]
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8)
    assert raw.size == h * (1 + bpp * w)
    raw = raw.reshape(h, 1 + bpp * w)
    filters = raw[:, 0].copy()
    assert (filters <= 2).all()
    out = np.zeros((h, w, bpp), dtype=np.uint8)
    for r in range(h):
        row = raw[r, 1:].reshape(w, bpp)
        if filters[r] == 1:
            row = np.cumsum(row, axis=0, dtype=np.uint8)
        elif filters[r] == 2 and r > 0:
            row = row + out[r - 1]
        out[r] = row
    samples = np.ascontiguousarray(out).view(">u2").astype(np.uint16)       # [h, w, channels]
    return (samples if channels == 4 else samples[:, :, 0]), filters, idat


def model_sizes(samples):
    """(a) zlib level 6 over the filtered stream; (b) the scheme's model: Z_RLE, raw deflate, memLevel 8, 32 KiB slices with a
    sync flush after each, plus the 6 bytes of zlib header and Adler-32 (tests/test_png_device.py, for this stream)."""
    filtered = filter_rows(samples)[1].tobytes()
    a = len(zlib.compress(filtered, 6))
    b = 6
    for k in range(0, len(filtered), CHUNK):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        b += len(c.compress(filtered[k:k + CHUNK]) + c.flush(zlib.Z_SYNC_FLUSH))
    return a, b


def stored_file_size(width, rows, channels):
    """signature, IHDR, IDAT around a zlib stream of one stored block of 5 + 32768 bytes a chunk, IEND"""
    n = rows * (1 + 2 * channels * width)
    return 8 + 25 + 12 + 2 + n + 5 * ((n + CHUNK - 1) // CHUNK) + 4 + 12


# ---------------------------------------------------------------- CPU

def test_library_exports_and_binds_the_16_bit_entry_points():
    lib = nh.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in nh.API_SYMBOLS
    for name in NEW_METHODS:
        assert callable(getattr(nh.NdtHip, name, None)), name
    assert callable(nh.png16_bound)
    assert lib.ndt_hip_abi_version() == 3


def test_png16_bound_covers_the_stored_file_and_refuses_bad_sizes():
    lib = nh.load_library()
    for channels in (1, 4):
        for w, h in ((1, 1), (1920, 1080), (3840, 2160), (7, 3), (4096, 1), (16384, 1)):
            assert lib.ndt_hip_png16_bound(w, h, channels) >= stored_file_size(w, h, channels), (w, h, channels)
            assert nh.png16_bound(w, h, channels) == lib.ndt_hip_png16_bound(w, h, channels)
        for w, h in ((0, 1), (1, 0), (0, 0), (-1, 5), (5, -1), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 1), (1, 2 ** 31 - 1)):
            assert lib.ndt_hip_png16_bound(w, h, channels) < 0, (w, h, channels)
    for channels in (0, 2, 3, 5, 8, -1):
        assert lib.ndt_hip_png16_bound(16, 16, channels) < 0, channels
    # the 8-bit limit with the new stride: a filtered stream of rows * (1 + 2 channels width) <= 2^31 - 1 bytes
    assert lib.ndt_hip_png16_bound(1 << 28, 1, 4) < 0           # 2^31 + 1
    assert lib.ndt_hip_png16_bound((1 << 28) - 1, 1, 4) > 0     # 2^31 - 7
    assert lib.ndt_hip_png16_bound(1 << 30, 1, 1) < 0           # 2^31 + 1
    assert lib.ndt_hip_png16_bound((1 << 30) - 1, 1, 1) > 0     # 2^31 - 1
    assert lib.ndt_hip_png16_bound(32768, 8192, 4) < 0 and lib.ndt_hip_png16_bound(8191, 32767, 4) > 0
    with pytest.raises(ValueError):
        nh.png16_bound(4, 4, 3)
    with pytest.raises(ValueError):
        nh.png16_bound(0, 4)


def _q16_scalar(x):
    m = 1.0 if 1.0 < x else x
    m = 0.0 if 0.0 > m else m
    return int(math.sqrt(m) * 65535)


EDGES = [0.0, -0.0, 1.0, 2.0, -1.0, 5e-324, 1e-300, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), np.inf, -np.inf]


def edge_values():
    """0, 1, -0.0, 2, -1, the infinities, and for a spread of k the squares of (k -+ 1e-9) / 65535 and of (k + 0.5) / 65535:
    just either side of the step to k (1e-9 is a hundred times the spacing of doubles at 65535), and its middle"""
    ks = np.array([1, 2, 3, 255, 256, 257, 32767, 32768, 65534, 65535], dtype=np.float64)
    return np.concatenate([EDGES, ((ks - 1e-9) / 65535) ** 2, ((ks + 1e-9) / 65535) ** 2, ((ks[:-1] + 0.5) / 65535) ** 2])


def test_q16_model_is_the_definition_value_by_value():
    x = edge_values()
    got = q16(x)
    assert got.tolist() == [_q16_scalar(float(v)) for v in x]
    assert got[:len(EDGES)].tolist() == [0, 0, 65535, 65535, 0, 0, 0, 65534, 65535, 65535, 0]
    ks = [1, 2, 3, 255, 256, 257, 32767, 32768, 65534, 65535]
    below, above, middle = got[len(EDGES):len(EDGES) + 10], got[len(EDGES) + 10:len(EDGES) + 20], got[len(EDGES) + 20:]
    assert below.tolist() == [k - 1 for k in ks] and above.tolist() == ks and middle.tolist() == ks[:-1]
    rng = np.random.default_rng(16)
    y = rng.uniform(-0.25, 1.25, 2000)
    assert q16(y).tolist() == [_q16_scalar(float(v)) for v in y]


Q16_SAMPLES, Q16_SEED, Q16_LEFT_OUT_CAP = 200000, 2016, 2


def test_q16_floors_to_the_8_bit_value():
    """q16(x) // 257 == pixel_d2c(x): with s = sqrt(x) exact, floor(floor(65535 s) / 257) = floor(255 s) because 65535 = 257 * 255.
    In doubles each product is rounded once, so the identity can only break where s * 255 or s * 65535 lands within one ulp of an
    integer (for the second: of a multiple of 257, but every integer is left out to keep the rule plain).  Such samples are left
    out.  The chance of one is about 4 ulp / 1 = 4 * 65535 * 2^-52 = 6e-11 a sample, 1.2e-5 for the 200 000 drawn here: the cap is
    2 samples, a condition on the seed checked below on the CPU -- not a tolerance of anything the device computes."""
    x = np.random.default_rng(Q16_SEED).uniform(0.0, 1.0, Q16_SAMPLES)
    s = np.sqrt(x)
    left_out = np.zeros(x.size, dtype=bool)
    for scale in (255.0, 65535.0):
        y = s * scale
        left_out |= np.abs(y - np.rint(y)) <= np.spacing(y)
    assert int(left_out.sum()) <= Q16_LEFT_OUT_CAP
    keep = ~left_out
    assert np.array_equal(q16(x)[keep] // 257, pixel_d2c(x)[keep].astype(np.uint16))
    assert q16(x).max() > 65000 and q16(x).min() < 500


# width x height by channel count: head and tail bytes and a width under a wavefront; a row of 32 761 and 32 769 stream bytes,
# one under and one over a chunk, at either pixel width; several rows; rows that straddle chunks at unaligned offsets
COMMON_SHAPES = [(1, 1), (1, 5), (7, 3), (264, 31), (910, 9)]
SHAPES = [(s, 4) for s in COMMON_SHAPES + [(4095, 1), (4096, 1)]] + [(s, 1) for s in COMMON_SHAPES + [(16383, 1), (16384, 1)]]
KINDS = ["zero", "gradient", "noise", "noise_row", "runs"]
RUNS = (2, 3, 258, 259, 260)


def synthetic(kind, w, h, channels):
    """uint16 samples [h, w, 4] or [h, w]"""
    rng = np.random.default_rng(1000 * w + 10 * h + channels)
    shape = (h, w, channels)
    if kind == "zero":
        img = np.zeros(shape, dtype=np.uint16)
    elif kind == "gradient":
        # steps of a few units: the low bytes change from pixel to pixel, the high bytes run
        x, y, c = np.meshgrid(np.arange(w), np.arange(h), np.arange(channels))
        img = ((x * 3 + y * 5 + c * 4099) % 65536).astype(np.uint16)
    elif kind == "noise":
        img = rng.integers(0, 65536, shape, dtype=np.uint16)
    elif kind == "noise_row":
        img = np.full(shape, 0x4d4d, dtype=np.uint16)
        img[h // 2] = rng.integers(0, 65536, (w, channels), dtype=np.uint16)
    elif kind == "runs":
        # the Sub-filtered rows are runs of exactly 2, 3, 258, 259 and 260 equal bytes (values -1 / +1 in turn): the image's bytes
        # are their running sum at the pixel's distance
        bpp = 2 * channels
        want = np.zeros(h * bpp * w, dtype=np.uint8)
        at, k = 0, 0
        while at < want.size:
            want[at:at + RUNS[k % len(RUNS)]] = 255 if k % 2 == 0 else 1
            at += RUNS[k % len(RUNS)]
            k += 1
        raw = np.cumsum(want.reshape(h, w, bpp), axis=1, dtype=np.uint8)
        img = np.ascontiguousarray(raw).view(">u2").astype(np.uint16)
    else:
        raise ValueError(kind)
    return img if channels == 4 else img[:, :, 0]


def test_the_models_agree_with_themselves():
    """(CPU) filter_rows and read_png16 are inverse to each other through zlib, at both pixel widths; the first row's Up is None's
    cost, so Up is never chosen there; `runs` holds the runs it is named for."""
    for channels in (1, 4):
        for kind in KINDS:
            img = synthetic(kind, 37, 5, channels)
            filters, stream = filter_rows(img)
            assert filters[0] != 2
            body = zlib.compress(stream.tobytes(), 1)
            ihdr = struct.pack(">IIBBBBB", 37, 5, 16, 6 if channels == 4 else 0, 0, 0, 0)
            png = b"\x89PNG\r\n\x1a\n"
            for typ, data in ((b"IHDR", ihdr), (b"IDAT", body), (b"IEND", b"")):
                png += struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data))
            back, f2, _ = read_png16(png, channels)
            assert np.array_equal(back, img) and np.array_equal(f2, filters)
    flat = filter_rows(synthetic("runs", 4095, 1, 4))[1].reshape(-1)
    edges = np.flatnonzero(np.concatenate(([True], flat[1:] != flat[:-1], [True])))
    assert set(RUNS) <= set(np.diff(edges).tolist())
    assert len(set(filter_rows(synthetic("noise_row", 264, 31, 4))[0].tolist())) > 1


def _run_driver(cwd, *flags, scene="builtin:yaml"):
    assert os.path.exists(DRIVER), "ndt_amd/host/ndt_hip is not built"
    os.makedirs(str(cwd), exist_ok=True)
    return subprocess.run([DRIVER, "-s", scene, "-d", "4", "-f", "0", "-r", "96x54", "-l", "6"] + list(flags),
                          capture_output=True, text=True, cwd=str(cwd))


def test_driver_refuses_png16_without_its_encoder_by_name(tmp_path):
    """(CPU) --png16 alone, beside --jpeg, beside --raw and over several contexts ends the run with a message that names the flag,
    before a scene is loaded or a device asked for."""
    for flags, words in ((["--png16"], ("--png16", "--png --deflate gpu")),
                         (["--png", "--png16"], ("--png16", "--deflate gpu")),
                         (["--jpeg", "--png16"], ("--png16", "--jpeg")),
                         (["--png", "--deflate", "gpu", "--png16", "--raw", "fb.f64"], ("--png16", "--raw")),
                         (["--png", "--deflate", "gpu", "--png16", "-z"], ("--png16", "--depth-png")),
                         (["--png", "--deflate", "gpu", "--png16", "-g", "2"], ("--png16", "-g 2"))):
        r = _run_driver(tmp_path, *flags)
        assert r.returncode != 0, flags
        for w in words:
            assert w in r.stderr, (flags, r.stderr)
    assert not list(tmp_path.rglob("*.p*")) and not list(tmp_path.rglob("*.f64"))


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,channels", SHAPES, ids=["%dx%dx%d" % (s[0], s[1], c) for s, c in SHAPES])
def test_round_trip_of_synthetic_images(gpu, shape, channels, kind):
    w, h = shape
    img = synthetic(kind, w, h, channels)
    png = gpu.encode_png16(img)
    st = gpu.png_stats
    print("%dx%dx%d %s: %d bytes (IDAT %d), %d chunks, %d stored, filters %s, %.3f ms" % (
        w, h, channels, kind, len(png), st.idat_bytes, st.chunks, st.chunks_stored, list(st.rows_filter), st.encode_ms))
    samples, filters, idat = read_png16(png, channels)          # every CRC, the IHDR's 16 / 6 or 16 / 0, the inflated size
    assert np.array_equal(samples, img)
    want_filters, stream = filter_rows(img)
    assert np.array_equal(filters, want_filters)
    assert list(st.rows_filter) == [int((want_filters == f).sum()) for f in range(3)] and sum(st.rows_filter) == h
    assert st.png_bytes == len(png) <= nh.png16_bound(w, h, channels)
    assert st.idat_bytes == len(idat) and st.launches >= 1
    assert st.chunks == (stream.size + CHUNK - 1) // CHUNK
    if kind == "noise":
        assert st.chunks_stored == st.chunks


def _device_bytes(t):
    return t.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 255, 256, 257, 100003])
def test_quantize16_device_is_the_model_for_every_value(gpu, n):
    """Bit-exact, and no value is left out: sqrt and one multiply are correctly rounded on both sides."""
    import torch
    rng = np.random.default_rng(n)
    x = rng.uniform(-0.1, 1.1, 4 * n)
    edges = edge_values()
    x[:min(edges.size, x.size)] = edges[:min(edges.size, x.size)]
    if n > 200:
        x[-edges.size:] = edges                 # and in the last workgroup's lanes
    dev = torch.from_numpy(x).cuda()
    out = torch.full((8 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu.quantize16_device(dev.data_ptr(), out.data_ptr(), n)
    gpu.synchronize()
    got = _device_bytes(out)
    assert (got[8 * n:] == 0xA5).all()
    want = np.ascontiguousarray(q16(x).astype(">u2")).view(np.uint8)
    differ = int((got[:8 * n] != want).sum())
    print("quantize16 of %d pixels: %d of %d bytes differ from the model" % (n, differ, want.size))
    assert differ == 0
    # misaligned pointers are refused by name
    assert gpu.lib.ndt_hip_quantize16_device(gpu.ctx, C.c_void_p(dev.data_ptr() + 8), C.c_void_p(out.data_ptr()), 0) == NDT_E_INVALID
    assert gpu.lib.ndt_hip_quantize16_device(gpu.ctx, C.c_void_p(dev.data_ptr()), C.c_void_p(out.data_ptr() + 4), 0) == NDT_E_INVALID
    assert b"ndt_hip_quantize16_device" in gpu.lib.ndt_hip_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2049, 300007])
@pytest.mark.parametrize("kind", ["constant", "two_values", "random"])
def test_depth_grey16_device_on_hand_made_maps(gpu, n, kind):
    """odd and even sizes (the last sample of an odd map is a 2-byte store), under and over a wavefront, several trips"""
    import torch
    rng = np.random.default_rng(n)
    if kind == "constant":
        dm = np.full(n, 0.375)
    elif kind == "two_values":
        dm = np.full(n, 0.125)
        dm[n // 2] = 3.5
    else:
        dm = np.where(rng.random(n) < 0.25, 0.0, 1.0 / rng.uniform(0.01, 50.0, n))
    dev = torch.from_numpy(dm).cuda()
    out = torch.full((2 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    r = gpu.depth_grey16_device(dev.data_ptr(), n, out.data_ptr())
    got = _device_bytes(out)
    want, lo, hi = depth_model(dm)
    assert (got[2 * n:] == 0xA5).all()
    assert np.array_equal(got[:2 * n], np.ascontiguousarray(want.astype(">u2")).view(np.uint8))
    assert r.view(np.uint64).tolist() == np.array([lo, hi]).view(np.uint64).tolist()
    if kind == "constant":
        assert not got[:2 * n].any()
    assert gpu.depth_launches() == 2


@pytest.mark.gpu
def test_device_pointer_entry_is_the_host_pointer_entry(gpu):
    import torch
    for channels, (w, h) in ((4, (333, 41)), (1, (333, 41))):
        img = synthetic("gradient", w, h, channels)
        dev = torch.from_numpy(wire(img).copy()).cuda()
        torch.cuda.synchronize()
        assert gpu.encode_png16_device(dev.data_ptr(), w, h, channels) == gpu.encode_png16(img)


@pytest.mark.gpu
def test_bad_arguments_are_refused_by_name_and_a_short_buffer_is_left_alone(gpu):
    img = wire(synthetic("gradient", 2, 2, 4)).copy()
    out = np.zeros(4096, dtype=np.uint8)
    lib = gpu.lib
    assert lib.ndt_hip_encode_png16(gpu.ctx, None, 2, 2, 4, out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_png16(gpu.ctx, img.ctypes.data, 2, 2, 4, None, 4096, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_png16(None, img.ctypes.data, 2, 2, 4, out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_png16_device(gpu.ctx, None, 2, 2, 4, out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert b"ndt_hip_encode_png16" in lib.ndt_hip_last_error()
    for w, h in ((0, 2), (2, 0), (-1, 2)):
        assert lib.ndt_hip_encode_png16(gpu.ctx, img.ctypes.data, w, h, 4, out.ctypes.data, 4096, None) == NDT_E_INVALID
        assert b"ndt_hip_encode_png16" in lib.ndt_hip_last_error()
    for channels in (0, 2, 3, 5):
        assert lib.ndt_hip_encode_png16(gpu.ctx, img.ctypes.data, 2, 2, channels, out.ctypes.data, 4096, None) == NDT_E_INVALID
        assert b"channels" in lib.ndt_hip_last_error()
        assert lib.ndt_hip_encode_png16_device(gpu.ctx, img.ctypes.data, 2, 2, channels, out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_png16(gpu.ctx, img.ctypes.data, 1 << 28, 1, 4, out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert b"2^31" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_encode_png16(gpu.ctx, img.ctypes.data, 2, 2, 4, out.ctypes.data, -1, None) == NDT_E_INVALID
    assert lib.ndt_hip_render_png16(gpu.ctx, None, out.ctypes.data, 4096, None, None) == NDT_E_INVALID
    assert lib.ndt_hip_render_png16_depth(gpu.ctx, None, out.ctypes.data, 4096, out.ctypes.data, 4096, None, None, None) == NDT_E_INVALID
    assert lib.ndt_hip_render_ssaa_png16(gpu.ctx, None, 2, out.ctypes.data, 4096, None, None) == NDT_E_INVALID
    bad = gpu.params(4, 4, 1, row_step=0)
    assert lib.ndt_hip_render_png16(gpu.ctx, C.byref(bad), out.ctypes.data, 4096, None, None) == NDT_E_INVALID
    assert b"ndt_hip_render_png16: bad geometry" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_render_png16_depth(gpu.ctx, C.byref(bad), out.ctypes.data, 4096, out.ctypes.data, 4096, None, None, None) == NDT_E_INVALID
    assert b"ndt_hip_render_png16_depth: bad geometry" in lib.ndt_hip_last_error()
    assert not out.any()
    # the encoder needs no scene, and a stats pointer is optional
    assert lib.ndt_hip_encode_png16(gpu.ctx, img.ctypes.data, 2, 2, 4, out.ctypes.data, 4096, None) == 0
    assert out[:8].tobytes() == b"\x89PNG\r\n\x1a\n"
    # room one byte short: NDT_E_NOMEM with the size needed, and nothing written -- least of all behind `cap`
    for channels in (4, 1):
        pic = synthetic("gradient", 264, 31, channels)
        png = gpu.encode_png16(pic)
        cap = len(png) - 1
        buf = np.full(cap + 64, 0xA5, dtype=np.uint8)
        short = nh.PngStats()
        data = wire(pic).copy()
        rc = lib.ndt_hip_encode_png16(gpu.ctx, data.ctypes.data, 264, 31, channels, buf.ctypes.data, cap, C.byref(short))
        assert rc == NDT_E_NOMEM
        assert str(len(png)) in lib.ndt_hip_last_error().decode()
        assert short.png_bytes == len(png)
        assert (buf == 0xA5).all()


@pytest.mark.gpu
def test_the_8_bit_file_is_the_same_bytes_around_16_bit_encodes(gpu):
    """the encoder's buffers and parameters are shared between the depths: nothing of a 16-bit encode stays behind"""
    rng = np.random.default_rng(8)
    img8 = np.cumsum(rng.integers(0, 3, (31, 264, 4)), axis=1).astype(np.uint8)
    before = gpu.encode_png(img8)
    assert before[24:26] == bytes([8, 6])
    for channels in (4, 1):
        for kind in ("noise", "gradient"):
            png = gpu.encode_png16(synthetic(kind, 910, 9, channels))
            assert png[24:26] == bytes([16, 6 if channels == 4 else 0])
        assert gpu.encode_png(img8) == before
    again = gpu.encode_png16(synthetic("gradient", 910, 9, 4))
    assert again == gpu.encode_png16(synthetic("gradient", 910, 9, 4))      # the same image, the same bytes


# the smallest fixtures the 8-bit PNG and depth tests render: a mono frame, a side-by-side one, -a, and the row shard 1::3
RENDER_CASES = {"mono": ("depth_c3_random4d", {}), "side_by_side": ("st_zoo4d_sbs", {"stereo": 1}),
                "aa": ("aa_c3_random4d_depth", {"aa": (20, 3)}), "row_shard": ("c3_random4d", {"row_begin": 1, "row_step": 3})}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(RENDER_CASES))
def test_render_png16_is_q16_of_the_double_framebuffer(gpu, case):
    name, kw = RENDER_CASES[case]
    g = golden(name)
    gpu.upload_scene(g.scene)
    fb, _ = gpu.render(g.width, g.height, g.depth, **kw)
    png, _ = gpu.render_png16(g.width, g.height, g.depth, **kw)
    st = gpu.png_stats
    samples, filters, idat = read_png16(png, 4)
    want = q16(fb)
    differ = int((samples != want).sum())
    a, b = model_sizes(want)
    print("%s %s: %d of %d samples differ from q16 of the framebuffer; IDAT %d bytes: x%.3f of zlib-6 (%d), x%.3f of the model (%d); "
          "%d of %d chunks stored; %.3f ms" % (name, case, differ, want.size, len(idat), len(idat) / a, a, len(idat) / b, b,
                                               st.chunks_stored, st.chunks, st.encode_ms))
    assert samples.shape == want.shape and differ == 0
    assert np.array_equal(filters, filter_rows(want)[0])
    assert st.png_bytes == len(png) <= nh.png16_bound(g.width, samples.shape[0], 4)
    # the ceilings tests/test_png_device.py documents for the 8-bit stream: 1.15 x the scheme's model, 2 x zlib level 6
    assert len(idat) <= 1.15 * b, "x%.3f of the model" % (len(idat) / b)
    assert len(idat) <= 2 * a, "x%.3f of zlib level 6" % (len(idat) / a)


@pytest.mark.gpu
def test_render_png16_depth_is_the_model_of_the_map(gpu):
    g = golden("depth_c3_random4d")
    gpu.upload_scene(g.scene)
    fb, dm, _ = gpu.render(g.width, g.height, g.depth, depth_map=True)
    png, depth_png, rng, _ = gpu.render_png16_depth(g.width, g.height, g.depth)
    assert [s.png_bytes for s in gpu.png_stats] == [len(png), len(depth_png)]
    want, lo, hi = depth_model(dm)
    assert hi > lo and (dm > 0).any()
    grey, _, idat = read_png16(depth_png, 1)
    a, b = model_sizes(want)
    print("depth_c3_random4d: %d of %d grey samples differ from the model; %d distinct values; range [%r, %r]; IDAT %d bytes: "
          "x%.3f of zlib-6, x%.3f of the model" % (int((grey != want).sum()), want.size, np.unique(grey).size, rng[0], rng[1],
                                                   len(idat), len(idat) / a, len(idat) / b))
    assert np.array_equal(grey, want)
    assert rng.view(np.uint64).tolist() == np.array([lo, hi]).view(np.uint64).tolist()
    assert np.array_equal(read_png16(png, 4)[0], q16(fb))
    assert png == gpu.render_png16(g.width, g.height, g.depth)[0]
    # a constant map (depth 0: nothing is traced, the map is zeros): hi == lo, every sample 0
    png0, depth_png0, rng0, _ = gpu.render_png16_depth(g.width, g.height, 0)
    assert not read_png16(depth_png0, 1)[0].any() and rng0.view(np.uint64).tolist() == [0, 0]
    assert np.array_equal(read_png16(png0, 4)[0], q16(gpu.render(g.width, g.height, 0)[0]))
    # refused as render_depth refuses: -z beside a stochastic -a
    with pytest.raises(nh.NdtHipError) as want_err:
        gpu.render(g.width, g.height, g.depth, aa=(20, 2), samples=3, depth_map=True)
    with pytest.raises(nh.NdtHipError) as got_err:
        gpu.render_png16_depth(g.width, g.height, g.depth, aa=(20, 2), samples=3)
    assert got_err.value.code == want_err.value.code and str(got_err.value) == str(want_err.value)


@pytest.mark.gpu
def test_render_ssaa_png16_keeps_what_the_8_bit_file_drops(gpu):
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    fb, dm, _ = gpu.render_ssaa(g.width, g.height, g.depth, 2, depth_map=True)
    png, _ = gpu.render_ssaa_png16(g.width, g.height, g.depth, 2)
    samples = read_png16(png, 4)[0]
    assert np.array_equal(samples, q16(fb))
    assert gpu.ssaa_launches() == 2
    # the feature's point: the averaged frame has more than 256 levels in a channel, and an 8-bit file has room for 256
    png8, _ = gpu.render_ssaa_png(g.width, g.height, g.depth, 2)
    n, = struct.unpack(">I", png8[33:37])
    raw8 = np.frombuffer(zlib.decompress(png8[41:41 + n]), dtype=np.uint8)
    assert png8[24:26] == bytes([8, 6]) and raw8.size == g.height * (1 + 4 * g.width)
    raw8 = raw8.reshape(g.height, 1 + 4 * g.width)
    pixels8 = np.zeros((g.height, g.width, 4), dtype=np.uint8)             # the 8-bit file the device wrote, un-filtered
    for r in range(g.height):
        row = raw8[r, 1:].reshape(g.width, 4)
        pixels8[r] = np.cumsum(row, axis=0, dtype=np.uint8) if raw8[r, 0] == 1 else row + pixels8[r - 1] if raw8[r, 0] == 2 and r else row
    levels16 = [np.unique(samples[..., c]).size for c in range(4)]
    levels8 = [np.unique(pixels8[..., c]).size for c in range(4)]
    print("c3_random4d --ssaa 2: distinct values a channel: 16-bit file %s, 8-bit file %s" % (levels16, levels8))
    assert max(levels16) > 256
    # the two files are one frame: the 8-bit one holds the 16-bit one's samples floored to 8 bits, but for samples whose
    # sqrt * 255 or * 65535 sits within an ulp of an integer (test_q16_floors_to_the_8_bit_value; the same cap)
    assert int((pixels8 != samples // 257).sum()) <= Q16_LEFT_OUT_CAP
    assert max(levels16) > max(levels8)
    # the map beside it is the plain frame's, as documented
    png2, depth_png, rng, _ = gpu.render_ssaa_png16(g.width, g.height, g.depth, 2, depth_map=True)
    want, lo, hi = depth_model(dm)
    assert png2 == png and np.array_equal(read_png16(depth_png, 1)[0], want)
    assert rng.view(np.uint64).tolist() == np.array([lo, hi]).view(np.uint64).tolist()
    assert np.array_equal(dm, gpu.render(g.width, g.height, g.depth, depth_map=True)[1])


# ---------------------------------------------------------------- driver

@pytest.fixture(scope="module")
def zoo(tmp_path_factory):
    """tests/scenes/parity_zoo.c compiled against this repository's host headers, as tests/test_depth_device.py builds it: the
    driver tests need no binary of the reference, so they never skip."""
    d = tmp_path_factory.mktemp("zoo16")
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
def test_driver_writes_16_bit_files(zoo, tmp_path):
    """`--png --deflate gpu --png16` writes q16 of the doubles `--raw` dumps; with `-z --depth gpu --depth-png` the map's file is
    the model of the map `--raw` dumps beside them; with `--ssaa 2` it is q16 of the folded doubles."""
    r = _run_driver(tmp_path / "raw", "-z", "--raw", "fb.f64", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    fb = np.fromfile(str(tmp_path / "raw" / "fb.f64"), dtype=np.float64).reshape(54, 96, 4)
    dm = np.fromfile(str(tmp_path / "raw" / "fb.f64.depth"), dtype=np.float64).reshape(54, 96)

    r = _run_driver(tmp_path / "one", "--png", "--deflate", "gpu", "--png16", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    found = list((tmp_path / "one" / "images").rglob("*.png"))
    assert len(found) == 1 and not (tmp_path / "one" / "depth").exists()
    data = found[0].read_bytes()
    assert "compressed 16-bit PNG of %d bytes on GPU 0 in " % len(data) in r.stdout and " launches" in r.stdout
    assert np.array_equal(read_png16(data, 4)[0], q16(fb))

    r = _run_driver(tmp_path / "two", "--png", "--deflate", "gpu", "--png16", "-z", "--depth", "gpu", "--depth-png", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    image, depth = list((tmp_path / "two" / "images").rglob("*.png")), list((tmp_path / "two" / "depth").glob("*"))
    assert len(image) == 1 and len(depth) == 1 and depth[0].suffix == ".png"
    assert image[0].name == found[0].name and image[0].read_bytes() == data
    assert np.array_equal(read_png16(depth[0].read_bytes(), 1)[0], depth_model(dm)[0])
    assert "compressed 16-bit depth PNG of %d bytes on GPU 0 in " % len(depth[0].read_bytes()) in r.stdout
    assert "finished depth map [" in r.stdout

    r = _run_driver(tmp_path / "raw2", "--ssaa", "2", "--raw", "fb.f64", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    fb2 = np.fromfile(str(tmp_path / "raw2" / "fb.f64"), dtype=np.float64).reshape(54, 96, 4)
    r = _run_driver(tmp_path / "ssaa", "--png", "--deflate", "gpu", "--png16", "--ssaa", "2", "-j", "2", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    found = list((tmp_path / "ssaa" / "images").rglob("*.png"))
    assert len(found) == 1 and "supersampled 2x2 on GPU 0 in 2 launches" in r.stdout
    assert np.array_equal(read_png16(found[0].read_bytes(), 4)[0], q16(fb2))
