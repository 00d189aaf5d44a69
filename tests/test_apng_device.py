"""A frame sequence as one animated PNG, the difference between frames found on the device (ndt_apng.hip; `ndt_hip --apng`).

The yardsticks are this file's own, never the device's output:
  * a strict APNG reader: chunk order, every CRC, acTL's count, sequence numbers 0, 1, 2, ... without gaps, every fcTL inside the
    canvas, dispose 0 and blend 0 or 1, filters 0 / 1 / 2 only; every stream is inflated by Python's zlib, and the frames are
    composed by the specification's rule (SOURCE replaces; OVER with alpha 255 replaces, with alpha 0 keeps -- any other alpha
    under OVER would need arithmetic the scheme never asks for, and fails the reader);
  * the plan of a later frame restated in numpy: changed = the 32-bit word differs from the canvas's; the tight bounding box of
    the changed pixels; nothing changed: 1 x 1 at (0, 0), SOURCE; OVER when every changed pixel has alpha 255, the unchanged
    pixels of the rectangle then sent as zeros; SOURCE otherwise, the pixels as they are.
"""
import ctypes as C
import io
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, golden

from ndt_amd import hip as nh

NDT_E_INVALID, NDT_E_NOMEM = -1, -4
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "scenes")
DRIVER = os.path.join(ROOT, "ndt_amd", "host", "ndt_hip")
SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ---------------------------------------------------------------- yardsticks

def chunks_of(data):
    """[(type, body)] of a PNG-family file; every chunk's CRC-32 is checked and nothing may follow the last chunk."""
    assert data[:8] == SIGNATURE
    pos, out = 8, []
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert len(body) == n, typ
        assert zlib.crc32(typ + body) == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0], typ
        out.append((typ, body))
        pos += 12 + n
    assert pos == len(data)
    return out


def inflate_image(stream, w, h):
    """The [h, w, 4] pixels of a zlib stream of h filtered scanlines of w RGBA pixels; filters 0 / 1 / 2 only."""
    raw = np.frombuffer(zlib.decompress(stream), dtype=np.uint8)
    assert raw.size == h * (1 + 4 * w)
    raw = raw.reshape(h, 1 + 4 * w)
    assert (raw[:, 0] <= 2).all()
    out = np.zeros((h, w, 4), dtype=np.uint8)
    for r in range(h):
        row = raw[r, 1:].reshape(w, 4)
        if raw[r, 0] == 1:
            row = np.cumsum(row, axis=0, dtype=np.uint8)
        elif raw[r, 0] == 2 and r > 0:
            row = row + out[r - 1]
        out[r] = row
    return out


def read_still(data):
    """(pixels, IDAT body) of an 8-bit RGBA PNG with one IDAT."""
    ch = chunks_of(data)
    assert [t for t, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, bits, colour, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    assert (bits, colour, comp, filt, lace) == (8, 6, 0, 0, 0)
    return inflate_image(ch[1][1], w, h), ch[1][1]


def read_apng(data):
    """(the composed frames, their fcTL records {x, y, w, h, num, den, blend}, their zlib streams) of an animated PNG as this
    library lays it out: IHDR, acTL, fcTL + IDAT, (fcTL + fdAT) ..., IEND."""
    ch = chunks_of(data)
    types = [t for t, _ in ch]
    assert types[:2] == [b"IHDR", b"acTL"] and types[-1] == b"IEND" and ch[-1][1] == b""
    W, H, bits, colour, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    assert (bits, colour, comp, filt, lace) == (8, 6, 0, 0, 0)
    n_frames, n_plays = struct.unpack(">II", ch[1][1])
    body = ch[2:-1]
    assert len(body) == 2 * n_frames and n_frames >= 1
    assert [t for t, _ in body] == [b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (n_frames - 1)
    seq, canvas, frames, records, streams = 0, np.zeros((H, W, 4), dtype=np.uint8), [], [], []
    for k in range(n_frames):
        fctl, payload = body[2 * k][1], body[2 * k + 1][1]
        assert len(fctl) == 26
        s, w, h, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", fctl)
        assert s == seq
        seq += 1
        assert w >= 1 and h >= 1 and x + w <= W and y + h <= H
        assert dispose == 0 and blend in (0, 1) and den >= 1
        if k == 0:
            assert (x, y, w, h) == (0, 0, W, H)          # the default image is the first frame
            stream = payload
        else:
            assert struct.unpack(">I", payload[:4])[0] == seq
            seq += 1
            stream = payload[4:]
        sub = inflate_image(stream, w, h)
        region = canvas[y:y + h, x:x + w]
        if blend == 0 or k == 0:
            region[...] = sub
        else:
            alpha = sub[..., 3]
            assert np.isin(alpha, (0, 255)).all()
            region[alpha == 255] = sub[alpha == 255]
        frames.append(canvas.copy())
        records.append(dict(x=x, y=y, w=w, h=h, num=num, den=den, blend=blend))
        streams.append(stream)
    return frames, records, streams, (n_frames, n_plays)


def plan(canvas, cur):
    """(x, y, w, h, blend, changed, translucent, the sub-image that is sent) of frame `cur` over `canvas`."""
    ch = (np.ascontiguousarray(canvas).view(np.uint32) != np.ascontiguousarray(cur).view(np.uint32))[..., 0]
    if not ch.any():
        return 0, 0, 1, 1, 0, 0, 0, cur[0:1, 0:1].copy()
    ys, xs = np.nonzero(ch)
    y0, y1, x0, x1 = int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1
    sub, c = cur[y0:y1, x0:x1].copy(), ch[y0:y1, x0:x1]
    translucent = int((sub[c][:, 3] != 255).sum())
    if translucent == 0:
        sub[~c] = 0
    return x0, y0, x1 - x0, y1 - y0, int(translucent == 0), int(ch.sum()), translucent, sub


# The sequence: frame 0 is opaque noise; every later frame is the one before it with one named variant applied.  A variant is
# dropped at a size that has no room for what it is named for -- two distinct corners need two pixels, a block with unchanged
# pixels around it needs 7 x 3 -- and for no other reason.
def sequence(w, h):
    rng = np.random.default_rng(5 + 1000 * w + h)
    f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    f[..., 3] = 255
    frames, names = [f.copy()], ["noise"]
    cy, cx = h // 2, w // 2

    def step(name):
        frames.append(f.copy())
        names.append(name)

    f[h // 3, w // 3] = (f[h // 3, w // 3, 0] ^ 1, 2, 3, 255)
    step("one pixel")
    step("identical")
    if w * h >= 2:
        f[0, 0] = (f[0, 0, 0] ^ 9, 9, 9, 255)
        f[h - 1, w - 1] = (f[h - 1, w - 1, 0] ^ 8, 8, 8, 255)
        step("two opposite corners")
    if w >= 7 and h >= 3:
        r0, c0 = h // 4, w // 7
        r1, c1 = r0 + max(1, h // 5), c0 + max(1, w // 3)
        f[r0:r1, c0:c1, :3] = rng.integers(0, 256, (r1 - r0, c1 - c0, 3), dtype=np.uint8)
        step("a block")
    f[cy, cx] = (4, 4, 4, 128)
    step("a translucent change")
    f[cy, cx] = (0, 0, 0, 0)
    if w * h >= 2:
        other = (cy * w + cx + 1) % (w * h)
        f[other // w, other % w] = (f[other // w, other % w, 0] ^ 1, 1, 1, 255)
    step("a change to transparent black")
    f[:, w - 1] = (3, 3, 3, 255)
    step("last column")
    f[h - 1, :] = (3, 3, 4, 255)
    step("last row")
    return frames, names


def encode_sequence(gpu, frames, **begin):
    """The whole file of `frames` through apng_add, and the ndt_apng_stats of every frame as a dict."""
    h, w, _ = frames[0].shape
    gpu.apng_begin(w, h, len(frames), **begin)
    parts, stats = [], []
    for f in frames:
        parts.append(gpu.apng_add(f))
        st = gpu.apng_stats
        assert st.bytes == len(parts[-1]) <= nh.apng_bound(w, h)
        stats.append({name: getattr(st, name) for name, _ in nh.ApngStats._fields_})
    parts.append(gpu.apng_end())
    return b"".join(parts), parts, stats


# ---------------------------------------------------------------- CPU

APNG_NAMES = ("ndt_hip_apng_bound", "ndt_hip_apng_begin", "ndt_hip_apng_add_device", "ndt_hip_apng_add", "ndt_hip_render_apng_frame",
              "ndt_hip_apng_end")


def test_library_exports_the_apng_entry_points():
    lib = nh.load_library()
    for name in APNG_NAMES:
        assert hasattr(lib, name), name
        assert name in nh.API_SYMBOLS


def test_stats_record_matches_its_ctypes_mirror():
    """sizeof(ndt_apng_stats) from a C compiler against the ctypes mirror, and the mirror against the layout written out."""
    assert C.sizeof(nh.ApngStats) == 4 * 8 + 8 * 4 + 8
    import shutil
    import tempfile
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        return
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "size.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include "ndt_hip.h"\nint main(void) { printf("%zu\\n", sizeof(ndt_apng_stats)); return 0; }\n')
        exe = os.path.join(d, "size")
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        assert int(subprocess.run([exe], capture_output=True, text=True, check=True).stdout) == C.sizeof(nh.ApngStats)


def test_apng_bound_follows_png_bound():
    lib = nh.load_library()
    for w, h in ((0, 1), (1, 0), (0, 0), (-1, 5), (5, -1), (1 << 29, 1), (65536, 8192), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 1),
                 (1, 2 ** 31 - 1)):
        assert lib.ndt_hip_png_bound(w, h) < 0 and lib.ndt_hip_apng_bound(w, h) < 0, (w, h)
    for w, h in ((1, 1), (1, 5), (7, 3), (1920, 1080), (3840, 2160), (16383, 32767)):
        assert lib.ndt_hip_png_bound(w, h) > 0
        assert lib.ndt_hip_apng_bound(w, h) >= lib.ndt_hip_png_bound(w, h) + 53 + 38 + 4, (w, h)
        assert nh.apng_bound(w, h) == lib.ndt_hip_apng_bound(w, h)
    with pytest.raises(ValueError):
        nh.apng_bound(0, 4)


def test_the_readers_and_the_plan_agree_on_a_file_made_here():
    """(CPU) the yardsticks against each other: a file laid out by this test from the numpy plan and Python's zlib reads back, frame
    for frame, as the sequence it was made from."""
    def chunk(t, b):
        return struct.pack(">I", len(b)) + t + b + struct.pack(">I", zlib.crc32(t + b))

    def stream(img):
        raw = np.zeros((img.shape[0], 1 + 4 * img.shape[1]), np.uint8)
        raw[:, 1:] = img.reshape(img.shape[0], -1)
        return zlib.compress(raw.tobytes(), 6)

    frames, names = sequence(20, 9)
    assert len(frames) == 9
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 20, 9, 8, 6, 0, 0, 0)) + chunk(b"acTL", struct.pack(">II", len(frames), 0))
    out += chunk(b"fcTL", struct.pack(">IIIIIHHBB", 0, 20, 9, 0, 0, 1, 24, 0, 0)) + chunk(b"IDAT", stream(frames[0]))
    seq, blends = 1, []
    for a, b in zip(frames, frames[1:]):
        x, y, w, h, blend, _, _, sub = plan(a, b)
        blends.append(blend)
        out += chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, x, y, 1, 24, 0, blend))
        out += chunk(b"fdAT", struct.pack(">I", seq + 1) + stream(sub))
        seq += 2
    got, _, _, _ = read_apng(out + chunk(b"IEND", b""))
    assert all(np.array_equal(g, f) for g, f in zip(got, frames))
    assert blends[names.index("a translucent change") - 1] == 0 and blends[names.index("a change to transparent black") - 1] == 0
    assert blends[names.index("one pixel") - 1] == 1 and blends[names.index("identical") - 1] == 0


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


# width x rows.  200x50: frame 0's filtered stream of 40 050 bytes spans two deflate chunks; 8191x1: one row, one workgroup, 32
# lanes short of a multiple of 256
SIZES = [(1, 1), (1, 5), (7, 3), (264, 31), (200, 50), (8191, 1)]

_encoded = {}


def encoded(gpu, size):
    if size not in _encoded:
        frames, names = sequence(*size)
        _encoded[size] = (frames, names) + encode_sequence(gpu, frames)
    return _encoded[size]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_round_trip_of_the_sequence(gpu, size):
    w, h = size
    frames, names, data, parts, stats = encoded(gpu, size)
    assert len(frames) >= 5, names
    got, records, streams, (n_frames, n_plays) = read_apng(data)
    assert (n_frames, n_plays) == (len(frames), 0)
    for k, (f, g) in enumerate(zip(frames, got)):
        assert np.array_equal(f, g), names[k]
    for k, (st, rec) in enumerate(zip(stats, records)):
        want = (0, 0, w, h, 0, 0, 0) if k == 0 else plan(frames[k - 1], frames[k])[:7]
        print("%dx%d frame %d (%s): %d x %d at %d,%d blend %d, %d changed, %d translucent, %d bytes, %d launches, %.3f ms" % (
            w, h, k, names[k], st["w"], st["h"], st["x"], st["y"], st["blend"], st["changed"], st["translucent"], st["bytes"],
            st["launches"], st["encode_ms"]))
        assert (st["x"], st["y"], st["w"], st["h"], st["blend"], st["changed"], st["translucent"]) == want, names[k]
        assert (rec["x"], rec["y"], rec["w"], rec["h"], rec["blend"]) == want[:5], names[k]
        assert (rec["num"], rec["den"]) == (1, 24)
        assert st["frame"] == k and st["zlib_bytes"] == len(streams[k]) and st["launches"] == (4 if k == 0 else 7)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(7, 3), (200, 50)], ids=lambda s: "%dx%d" % s)
def test_the_streams_are_the_still_encoders(gpu, size):
    frames, names, data, parts, stats = encoded(gpu, size)
    _, _, streams, _ = read_apng(data)
    assert streams[0] == read_still(gpu.encode_png(frames[0]))[1]
    for k in range(1, len(frames)):
        sub = plan(frames[k - 1], frames[k])[7]
        assert streams[k] == read_still(gpu.encode_png(sub))[1], names[k]


@pytest.mark.gpu
def test_the_still_encoder_is_untouched_by_a_session(gpu):
    frames, _ = sequence(264, 31)
    fixed = np.random.default_rng(77).integers(0, 256, (19, 50, 4), dtype=np.uint8)
    before = gpu.encode_png(fixed)
    assert np.array_equal(read_still(before)[0], fixed)
    gpu.apng_begin(264, 31, 3)
    first = gpu.apng_add(frames[0])
    assert gpu.encode_png(fixed) == before
    second = gpu.apng_add(frames[1])
    assert gpu.encode_png(fixed) == before
    third = gpu.apng_add(frames[3])
    tail = gpu.apng_end()
    assert gpu.encode_png(fixed) == before
    got = read_apng(first + second + third + tail)[0]
    assert all(np.array_equal(g, f) for g, f in zip(got, (frames[0], frames[1], frames[3])))


@pytest.mark.gpu
def test_an_identical_frame_appends_at_most_70_bytes(gpu):
    """38 bytes of fcTL, 16 of fdAT around the stream (length, type, sequence number, CRC-32) and a stream of at most 16: the
    zlib header, the five bytes of a 1 x 1 image stored behind a stored block's five, the Adler-32 -- ndt_hip_png_bound(1, 1)
    without the 57 bytes of a still file around its stream."""
    assert nh.png_bound(1, 1) - 57 == 16
    frames, _ = sequence(264, 31)
    gpu.apng_begin(264, 31, 2, delay_num=1, delay_den=30, n_plays=3)
    first = gpu.apng_add(frames[0])
    second = gpu.apng_add(frames[0])
    st = gpu.apng_stats
    print("an identical 264x31 frame appends %d bytes (stream %d)" % (len(second), st.zlib_bytes))
    assert len(second) <= 70 and st.zlib_bytes <= 16
    assert (st.x, st.y, st.w, st.h, st.blend, st.changed, st.translucent) == (0, 0, 1, 1, 0, 0, 0)
    got, records, _, counts = read_apng(first + second + gpu.apng_end())
    assert counts == (2, 3) and (records[1]["num"], records[1]["den"]) == (1, 30)
    assert np.array_equal(got[0], frames[0]) and np.array_equal(got[1], frames[0])


@pytest.mark.gpu
def test_device_pointer_entry_is_the_host_pointer_entry(gpu):
    import torch
    frames, _ = sequence(264, 31)
    data = encoded(gpu, (264, 31))[2]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    gpu.apng_begin(264, 31, len(frames))
    parts = [gpu.apng_add_device(d.data_ptr()) for d in dev]
    assert b"".join(parts) + gpu.apng_end() == data


def last_error(gpu):
    return gpu.lib.ndt_hip_last_error().decode()


@pytest.fixture
def fresh():
    """a context of its own: no session was ever opened on it"""
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
def test_refusals_name_their_cause(fresh):
    import torch
    gpu = fresh
    lib = gpu.lib
    img = np.zeros((2, 3, 4), dtype=np.uint8)
    out = np.zeros(4096, dtype=np.uint8)
    n = C.c_int64(0)
    # begin
    assert lib.ndt_hip_apng_begin(None, 3, 2, 2, 1, 24, 0) == NDT_E_INVALID and "NULL" in last_error(gpu)
    for w, h in ((0, 2), (3, 0), (-1, 2)):
        assert lib.ndt_hip_apng_begin(gpu.ctx, w, h, 2, 1, 24, 0) == NDT_E_INVALID and "%d x %d" % (w, h) in last_error(gpu)
    assert lib.ndt_hip_apng_begin(gpu.ctx, 1 << 29, 1, 2, 1, 24, 0) == NDT_E_INVALID and "2^31" in last_error(gpu)
    assert lib.ndt_hip_apng_begin(gpu.ctx, 3, 2, 0, 1, 24, 0) == NDT_E_INVALID and "n_frames" in last_error(gpu)
    assert lib.ndt_hip_apng_begin(gpu.ctx, 3, 2, 2, 1, 0, 0) == NDT_E_INVALID and "delay_den" in last_error(gpu)
    assert lib.ndt_hip_apng_begin(gpu.ctx, 3, 2, 2, 65536, 24, 0) == NDT_E_INVALID and "65535" in last_error(gpu)
    assert lib.ndt_hip_apng_begin(gpu.ctx, 3, 2, 2, 1, 65536, 0) == NDT_E_INVALID and "65535" in last_error(gpu)
    # a refused begin opens nothing, and a fresh context has no session
    for call in (lambda: lib.ndt_hip_apng_add(gpu.ctx, img.ctypes.data, out.ctypes.data, out.size, None),
                 lambda: lib.ndt_hip_apng_add_device(gpu.ctx, C.c_void_p(256), out.ctypes.data, out.size, None),
                 lambda: lib.ndt_hip_render_apng_frame(gpu.ctx, C.byref(gpu.params(3, 2, 1)), 1, out.ctypes.data, out.size, None, None),
                 lambda: lib.ndt_hip_apng_end(gpu.ctx, out.ctypes.data, out.size, C.byref(n))):
        assert call() == NDT_E_INVALID and "no session open" in last_error(gpu)
    # NULL arguments of the calls that take a session
    gpu.apng_begin(3, 2, 2)
    assert lib.ndt_hip_apng_add(gpu.ctx, img.ctypes.data, None, out.size, None) == NDT_E_INVALID and "NULL" in last_error(gpu)
    assert lib.ndt_hip_apng_add(None, img.ctypes.data, out.ctypes.data, out.size, None) == NDT_E_INVALID and "NULL" in last_error(gpu)
    assert lib.ndt_hip_apng_end(gpu.ctx, None, out.size, C.byref(n)) == NDT_E_INVALID and "NULL" in last_error(gpu)
    assert lib.ndt_hip_apng_add(gpu.ctx, None, out.ctypes.data, out.size, None) == NDT_E_INVALID and "NULL" in last_error(gpu)
    # ... the last one was an `add` that failed: the session is closed
    assert lib.ndt_hip_apng_add(gpu.ctx, img.ctypes.data, out.ctypes.data, out.size, None) == NDT_E_INVALID
    assert "no session open" in last_error(gpu)
    # a device pointer off its pixels
    dev = torch.zeros(64, dtype=torch.uint8, device="cuda")
    gpu.apng_begin(3, 2, 2)
    assert lib.ndt_hip_apng_add_device(gpu.ctx, C.c_void_p(dev.data_ptr() + 2), out.ctypes.data, out.size, None) == NDT_E_INVALID
    assert "aligned" in last_error(gpu)
    assert lib.ndt_hip_apng_add_device(gpu.ctx, C.c_void_p(dev.data_ptr()), out.ctypes.data, out.size, None) == NDT_E_INVALID
    assert "no session open" in last_error(gpu)
    # room one byte short: NDT_E_NOMEM with the size needed, nothing written, the session closed
    gpu.apng_begin(3, 2, 2)
    need = len(gpu.apng_add(img))
    gpu.apng_begin(3, 2, 2)
    buf = np.full(need + 64, 0xA5, dtype=np.uint8)
    st = nh.ApngStats()
    assert lib.ndt_hip_apng_add(gpu.ctx, img.ctypes.data, buf.ctypes.data, need - 1, C.byref(st)) == NDT_E_NOMEM
    assert str(need) in last_error(gpu) and st.bytes == need and (buf == 0xA5).all()
    assert lib.ndt_hip_apng_add(gpu.ctx, img.ctypes.data, out.ctypes.data, out.size, None) == NDT_E_INVALID
    assert "no session open" in last_error(gpu)
    # `end` before the last frame, and one `add` more than the session was opened for
    gpu.apng_begin(3, 2, 2)
    gpu.apng_add(img)
    assert lib.ndt_hip_apng_end(gpu.ctx, out.ctypes.data, out.size, C.byref(n)) == NDT_E_INVALID and "2 frames" in last_error(gpu)
    gpu.apng_add(img)
    assert lib.ndt_hip_apng_add(gpu.ctx, img.ctypes.data, out.ctypes.data, out.size, None) == NDT_E_INVALID
    assert "2 frames" in last_error(gpu)


@pytest.mark.gpu
def test_rendered_frames(gpu):
    a, b = golden("c1_hypercube3d"), golden("c1_hypercube3d_f37")
    w = h = 64
    gpu.upload_scene(a.scene)
    want_a, _ = gpu.render_rgba8(w, h, a.depth)
    want_a2, _ = gpu.render_ssaa_rgba8(w, h, a.depth, 2)
    gpu.upload_scene(b.scene)
    want_b, _ = gpu.render_rgba8(w, h, b.depth)
    assert not np.array_equal(want_a, want_b)
    gpu.apng_begin(w, h, 4)
    parts, rects = [], []
    for g, ssaa in ((a, 1), (b, 1), (a, 1), (a, 2)):
        gpu.upload_scene(g.scene)
        part, _ = gpu.render_apng_frame(w, h, g.depth, ssaa=ssaa)
        st = gpu.apng_stats
        rects.append((st.x, st.y, st.w, st.h))
        print("rendered frame %d: %d x %d at %d,%d blend %d, %d changed, %d bytes" % (st.frame, st.w, st.h, st.x, st.y, st.blend, st.changed, st.bytes))
        parts.append(part)
    got, records, _, _ = read_apng(b"".join(parts) + gpu.apng_end())
    for g, want in zip(got, (want_a, want_b, want_a, want_a2)):
        assert np.array_equal(g, want)
    assert rects[2] == rects[1] == (records[1]["x"], records[1]["y"], records[1]["w"], records[1]["h"])
    # a row shard, when `begin` was given the shard's rows
    kw = dict(row_begin=1, row_step=3)
    rows = len(range(1, h, 3))
    gpu.upload_scene(b.scene)
    shard_b, _ = gpu.render_rgba8(w, h, b.depth, **kw)
    gpu.upload_scene(a.scene)
    shard_a, _ = gpu.render_rgba8(w, h, a.depth, **kw)
    assert shard_a.shape == (rows, w, 4) and not np.array_equal(shard_a, shard_b)
    gpu.apng_begin(w, rows, 2)
    parts = [gpu.render_apng_frame(w, h, a.depth, **kw)[0]]
    gpu.upload_scene(b.scene)
    parts.append(gpu.render_apng_frame(w, h, b.depth, **kw)[0])
    got = read_apng(b"".join(parts) + gpu.apng_end())[0]
    assert np.array_equal(got[0], shard_a) and np.array_equal(got[1], shard_b)
    # the whole frame does not fit a session of the shard's rows
    gpu.apng_begin(w, rows, 1)
    out = np.zeros(nh.apng_bound(w, h), dtype=np.uint8)
    assert gpu.lib.ndt_hip_render_apng_frame(gpu.ctx, C.byref(gpu.params(w, h, b.depth)), 1, out.ctypes.data, out.size, None, None) == NDT_E_INVALID
    assert "%d x %d" % (w, rows) in last_error(gpu)


@pytest.mark.gpu
def test_pillow_reads_the_file(gpu):
    pytest.importorskip("PIL")
    from PIL import Image
    frames, names, data, _, _ = encoded(gpu, (200, 50))
    im = Image.open(io.BytesIO(data))
    assert im.format == "PNG" and im.n_frames == len(frames) and im.is_animated
    for k, f in enumerate(frames):
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert("RGBA")), f), names[k]


def _run_driver(cwd, *flags):
    cmd = [DRIVER, "-s", os.path.join(REF_BIN, "hypercube.so"), "-d", "3", "-r", "96x54", "-f", "0:3"] + list(flags)
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run(cmd, capture_output=True, text=True, cwd=str(cwd))


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built")
def test_driver_writes_the_animated_png(tmp_path):
    r = _run_driver(tmp_path / "apng", "--apng")
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    found = list((tmp_path / "apng" / "images").rglob("*"))
    files = [f for f in found if f.is_file()]
    assert len(files) == 1 and files[0].name.endswith("_96x54.apng")
    data = files[0].read_bytes()
    got, records, _, (n_frames, _) = read_apng(data)
    assert n_frames == 4 and (records[0]["num"], records[0]["den"]) == (1, 24)
    said = re.findall(r"animated PNG frame (\d+): (\d+) x (\d+) at (\d+),(\d+) \((\d+) bytes\) on GPU \d+ in (\d+) launches", r.stdout)
    assert [int(s[0]) for s in said] == [0, 1, 2, 3]
    assert sum(int(s[5]) for s in said) + 12 == len(data)
    for s, rec in zip(said, records):
        assert (int(s[1]), int(s[2]), int(s[3]), int(s[4])) == (rec["w"], rec["h"], rec["x"], rec["y"])
    r = _run_driver(tmp_path / "png", "--png", "--deflate", "gpu")
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    stills = sorted((tmp_path / "png" / "images").rglob("*.png"))
    assert len(stills) == 4
    for k, f in enumerate(stills):
        assert np.array_equal(read_still(f.read_bytes())[0], got[k]), k
    for k, (flags, names) in enumerate(((["--apng", "--png"], ("--apng", "--png")), (["--apng", "-j", "2"], ("--apng", "-j")),
                                        (["--apng", "-g", "2"], ("--apng", "-g")))):
        bad = _run_driver(tmp_path / ("bad%d" % k), *flags)
        assert bad.returncode != 0 and all(n in bad.stderr for n in names), bad.stderr
        assert not [f for f in (tmp_path / ("bad%d" % k)).rglob("*") if f.is_file()]
