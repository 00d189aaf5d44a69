"""The frame's PNG file made on the device (ndt_png.hip; `ndt_hip --png --deflate gpu`).

The yardsticks are Python's zlib and a numpy restatement of the row heuristic -- never the device's own output:
  * the reader below checks every chunk's CRC, inflates the IDAT with zlib (an over-subscribed or incomplete code, a bad
    stored-block length or a wrong Adler-32 raises there) and undoes filters 0 / 1 / 2 in numpy;
  * sizes are held against zlib level 6 and against the scheme's own model (Z_RLE, raw deflate, 32 KiB slices, a sync flush
    after each), both computed here from the golden image.
"""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, golden, FULL_CASES

from ndt_amd import hip as nh

NDT_E_INVALID, NDT_E_NOMEM = -1, -4
CHUNK = 32768
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "scenes")
DRIVER = os.path.join(ROOT, "ndt_amd", "host", "ndt_hip")


# ---------------------------------------------------------------- yardsticks

def filter_rows(img):
    """The row heuristic restated: per scanline filter 0 (None), 1 (Sub, distance 4) or 2 (Up), whichever has the smallest
    sum of |filtered byte taken as int8|, ties to the lower number, zeros above the first row.
    Returns (filters [h], the filtered stream [h, 1 + 4 w])."""
    h, w, _ = img.shape
    raw = np.ascontiguousarray(img, dtype=np.uint8).reshape(h, 4 * w)
    left = np.zeros_like(raw)
    left[:, 4:] = raw[:, :-4]
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    cands = np.stack([raw, raw - left, raw - up])                            # uint8 arithmetic wraps
    cost = np.abs(cands.view(np.int8).astype(np.int64)).sum(axis=2)          # [3, h]
    filters = np.argmin(cost, axis=0)                                        # the first of equal minima
    stream = np.empty((h, 1 + 4 * w), dtype=np.uint8)
    stream[:, 0] = filters
    stream[:, 1:] = cands[filters, np.arange(h)]
    return filters.astype(np.uint8), stream


def read_png(data):
    """(pixels [h, w, 4], filter byte of every row, IDAT bytes) of an 8-bit RGBA PNG with filters 0 / 1 / 2."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h, types = 8, b"", 0, 0, []
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert len(body) == n
        assert zlib.crc32(typ + body) == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0], typ
        types.append(typ)
        if typ == b"IHDR":
            w, h, bits, colour, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            assert (bits, colour, comp, filt, lace) == (8, 6, 0, 0, 0)
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    assert pos == len(data) and types[0] == b"IHDR" and types[-1] == b"IEND"
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8)
    assert raw.size == h * (1 + 4 * w)
    raw = raw.reshape(h, 1 + 4 * w)
    filters = raw[:, 0].copy()
    assert (filters <= 2).all()
    out = np.zeros((h, w, 4), dtype=np.uint8)
    for r in range(h):
        row = raw[r, 1:].reshape(w, 4)
        if filters[r] == 1:
            row = np.cumsum(row, axis=0, dtype=np.uint8)
        elif filters[r] == 2 and r > 0:
            row = row + out[r - 1]
        out[r] = row
    return out, filters, idat


def model_sizes(img):
    """(a) zlib level 6 over the filtered stream; (b) the scheme's model: Z_RLE, raw deflate, memLevel 8, 32 KiB slices
    with a sync flush after each, plus the 6 bytes of zlib header and Adler-32."""
    _, stream = filter_rows(img)
    filtered = stream.tobytes()
    a = len(zlib.compress(filtered, 6))
    b = 6
    for k in range(0, len(filtered), CHUNK):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        b += len(c.compress(filtered[k:k + CHUNK]) + c.flush(zlib.Z_SYNC_FLUSH))
    return a, b


def stored_file_size(width, rows):
    """What the driver's plain --png writer produces: stored blocks of up to 65535 bytes."""
    n = rows * (1 + 4 * width)
    return 57 + 2 + n + 5 * max(1, (n + 65534) // 65535) + 4


# ---------------------------------------------------------------- CPU

def test_library_exports_the_png_entry_points():
    lib = nh.load_library()
    for name in ("ndt_hip_png_bound", "ndt_hip_encode_png_device", "ndt_hip_encode_png", "ndt_hip_render_png"):
        assert hasattr(lib, name), name
        assert name in nh.API_SYMBOLS
    assert hasattr(lib, "ndt_hip_render_rgba8")


def test_png_bound_covers_the_stored_file_and_refuses_bad_sizes():
    lib = nh.load_library()
    for w, h in ((1, 1), (1920, 1080), (3840, 2160), (7, 3)):
        assert lib.ndt_hip_png_bound(w, h) >= stored_file_size(w, h), (w, h)
        assert nh.png_bound(w, h) == lib.ndt_hip_png_bound(w, h)
    for w, h in ((0, 1), (1, 0), (0, 0), (-1, 5), (5, -1)):
        assert lib.ndt_hip_png_bound(w, h) < 0, (w, h)
    # a filtered stream of more than 2^31 - 1 bytes, and products that leave 32 and 64 bits
    for w, h in ((1 << 29, 1), (65536, 8192), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 1), (1, 2 ** 31 - 1)):
        assert lib.ndt_hip_png_bound(w, h) < 0, (w, h)
    assert lib.ndt_hip_png_bound(16383, 32767) > 0        # 2 147 319 811 bytes: sizes up to the limit are taken
    with pytest.raises(ValueError):
        nh.png_bound(0, 4)


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


# width x height; the filtered stream of the last four is 32765, 32767, 32769 and 32769 bytes: 3 and 1 under, 1 over a chunk
SHAPES = [(1, 1), (1, 5), (7, 3), (8191, 1), (264, 31), (910, 9), (8192, 1)]
RUNS = (2, 3, 258, 259, 260)


def run_lengths(stream):
    flat = np.asarray(stream).reshape(-1)
    edges = np.flatnonzero(np.concatenate(([True], flat[1:] != flat[:-1], [True])))
    return set(np.diff(edges).tolist())


def synthetic(kind, w, h):
    rng = np.random.default_rng(1000 * w + h)
    if kind == "zero":
        return np.zeros((h, w, 4), dtype=np.uint8)
    if kind == "gradient":
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        return np.stack([x, y, x + y, (x * 3 + y * 5) // 7], axis=2).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if kind == "noise_row":
        img = np.full((h, w, 4), 77, dtype=np.uint8)
        img[h // 2] = rng.integers(0, 256, (w, 4), dtype=np.uint8)
        return img
    if kind == "runs":
        # the Sub-filtered rows are runs of exactly 2, 3, 258, 259 and 260 equal bytes (values +1 / -1 in turn): the image is
        # their running sum per channel
        want = np.zeros(h * 4 * w, dtype=np.uint8)
        at, k = 0, 0
        while at < want.size:
            want[at:at + RUNS[k % len(RUNS)]] = 255 if k % 2 == 0 else 1
            at += RUNS[k % len(RUNS)]
            k += 1
        return np.cumsum(want.reshape(h, w, 4), axis=1, dtype=np.uint8)
    raise ValueError(kind)


def test_the_runs_image_has_the_runs_it_is_named_for():
    """(CPU) what the `runs` image is for: with the row heuristic applied, the stream holds runs of exactly those lengths."""
    _, stream = filter_rows(synthetic("runs", 8191, 1))
    assert set(RUNS) <= run_lengths(stream)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zero", "gradient", "noise", "noise_row", "runs"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_round_trip_of_synthetic_images(gpu, shape, kind):
    w, h = shape
    img = synthetic(kind, w, h)
    png = gpu.encode_png(img)
    st = gpu.png_stats
    print("%dx%d %s: %d bytes (IDAT %d), %d chunks, %d stored, filters %s, %.3f ms" % (
        w, h, kind, len(png), st.idat_bytes, st.chunks, st.chunks_stored, list(st.rows_filter), st.encode_ms))
    pixels, filters, idat = read_png(png)
    assert np.array_equal(pixels, img)
    want_filters, stream = filter_rows(img)
    assert np.array_equal(filters, want_filters)
    assert list(st.rows_filter) == [int((want_filters == f).sum()) for f in range(3)]
    assert st.png_bytes == len(png) <= nh.png_bound(w, h)
    assert st.idat_bytes == len(idat) and st.launches >= 1
    assert st.chunks == (stream.size + CHUNK - 1) // CHUNK
    if kind == "noise":
        assert st.chunks_stored == st.chunks
    assert gpu.encode_png(img) == png                      # the same image, the same bytes
    # room one byte short: NDT_E_NOMEM with the size needed, and nothing written -- least of all behind `cap`
    cap = len(png) - 1
    buf = np.full(cap + 64, 0xA5, dtype=np.uint8)
    short = nh.PngStats()
    rc = gpu.lib.ndt_hip_encode_png(gpu.ctx, img.ctypes.data, w, h, buf.ctypes.data, cap, C.byref(short))
    assert rc == NDT_E_NOMEM
    assert str(len(png)) in gpu.lib.ndt_hip_last_error().decode()
    assert short.png_bytes == len(png)
    assert (buf == 0xA5).all()


@pytest.mark.gpu
def test_bad_arguments_are_refused_by_name(gpu):
    img = np.zeros((2, 2, 4), dtype=np.uint8)
    out = np.zeros(4096, dtype=np.uint8)
    lib = gpu.lib
    assert lib.ndt_hip_encode_png(gpu.ctx, None, 2, 2, out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_png(gpu.ctx, img.ctypes.data, 2, 2, None, 4096, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_png(None, img.ctypes.data, 2, 2, out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_png_device(gpu.ctx, None, 2, 2, out.ctypes.data, 4096, None) == NDT_E_INVALID
    for w, h in ((0, 2), (2, 0), (-1, 2)):
        assert lib.ndt_hip_encode_png(gpu.ctx, img.ctypes.data, w, h, out.ctypes.data, 4096, None) == NDT_E_INVALID
        assert lib.ndt_hip_last_error()
    assert lib.ndt_hip_encode_png(gpu.ctx, img.ctypes.data, 1 << 29, 1, out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert b"2^31" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_render_png(gpu.ctx, None, out.ctypes.data, 4096, None, None) == NDT_E_INVALID
    # the encoder needs no scene, and a stats pointer is optional
    assert lib.ndt_hip_encode_png(gpu.ctx, img.ctypes.data, 2, 2, out.ctypes.data, 4096, None) == 0
    n = len(gpu.encode_png(img))
    assert np.array_equal(read_png(out.tobytes()[:n])[0], img)


@pytest.mark.gpu
def test_device_pointer_entry_is_the_host_pointer_entry(gpu):
    import torch
    img = synthetic("gradient", 333, 41)
    dev = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    assert gpu.encode_png_device(dev.data_ptr(), 333, 41) == gpu.encode_png(img)


_rendered = {}


def rendered_golden(gpu, name):
    if name not in _rendered:
        g = golden(name)
        gpu.upload_scene(g.scene)
        png, _ = gpu.render_png(g.width, g.height, g.depth)
        st = gpu.png_stats
        _rendered[name] = (png, (st.png_bytes, st.idat_bytes, st.chunks, st.chunks_stored, st.launches, list(st.rows_filter), st.encode_ms))
    return _rendered[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", FULL_CASES)
def test_golden_frames_decode_to_the_references_image(gpu, name):
    g = golden(name)
    png, st = rendered_golden(gpu, name)
    pixels, filters, _ = read_png(png)
    ref = g.data["rgba8"]
    mism = int((pixels != ref).sum())
    print("%s: %d of %d bytes differ from the reference's image; file %d bytes, %.3f ms in %d launches" % (
        name, mism, ref.size, len(png), st[6], st[4]))
    assert mism == 0
    assert np.array_equal(filters, filter_rows(ref)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", FULL_CASES)
def test_golden_frames_are_within_reach_of_zlib(gpu, name):
    """idat_bytes <= 1.15 x the scheme's model and <= 2 x zlib level 6, both computed here from the golden image; no chunk of
    a golden frame is stored."""
    g = golden(name)
    png, st = rendered_golden(gpu, name)
    a, b = model_sizes(g.data["rgba8"])
    idat, stored = st[1], st[3]
    print("%s: IDAT %d bytes; zlib-6 %d (x%.3f); model %d (x%.3f); %d of %d chunks stored; rows by filter %s" % (
        name, idat, a, idat / a, b, idat / b, stored, st[2], st[5]))
    assert stored == 0
    assert idat <= 1.15 * b, "x%.3f of the model" % (idat / b)
    assert idat <= 2 * a, "x%.3f of zlib level 6" % (idat / a)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [("c3_random4d", {"aa": (12, 2)}), ("st_zoo4d_sbs", {"stereo": 1}),
                                     ("c3_random4d", {"row_begin": 1, "row_step": 3})],
                         ids=["aa", "side_by_side", "row_shard"])
def test_render_png_takes_every_mode_of_render_rgba8(gpu, name, kw):
    g = golden(name)
    gpu.upload_scene(g.scene)
    want, _ = gpu.render_rgba8(g.width, g.height, g.depth, **kw)
    png, _ = gpu.render_png(g.width, g.height, g.depth, **kw)
    pixels, _, _ = read_png(png)
    assert pixels.shape == want.shape
    assert np.array_equal(pixels, want)


def _run_driver(cwd, *flags):
    g = golden("c3_random4d_1080p")
    cmd = [DRIVER, "-s", os.path.join(REF_BIN, "random.so"), "-d", "4", "-f", "0", "-r", "1920x1080", "-l", str(g.depth)] + list(flags)
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run(cmd, capture_output=True, text=True, cwd=str(cwd))


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built")
def test_driver_writes_the_compressed_png(tmp_path):
    g = golden("c3_random4d_1080p")
    ref = g.data["rgba8"]
    files = {}
    for tag, flags in (("stored", ["--png"]), ("gpu", ["--png", "--deflate", "gpu"]), ("gpu_g3", ["--png", "--deflate", "gpu", "-g", "3"])):
        r = _run_driver(tmp_path / tag, *flags)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        found = list((tmp_path / tag / "images").rglob("*.png"))
        assert len(found) == 1
        files[tag] = found[0].read_bytes()
        if tag == "stored":
            assert "compressed PNG" not in r.stdout
        else:
            assert "compressed PNG of %d bytes on GPU" % len(files[tag]) in r.stdout and " launches" in r.stdout
    plain = read_png(files["stored"])[0]
    pixels = read_png(files["gpu"])[0]
    print("driver: --png %d bytes, --png --deflate gpu %d bytes" % (len(files["stored"]), len(files["gpu"])))
    assert np.array_equal(pixels, ref)
    assert np.array_equal(pixels, plain)
    assert len(files["gpu"]) * 50 < len(files["stored"])
    assert np.array_equal(read_png(files["gpu_g3"])[0], pixels)        # -g 3: gathered on the host, encoded from there
    bad = _run_driver(tmp_path / "bad", "--deflate", "gpu")
    assert bad.returncode != 0 and "--deflate gpu" in bad.stderr and "--png" in bad.stderr
    assert not list((tmp_path / "bad").rglob("*.p*"))
