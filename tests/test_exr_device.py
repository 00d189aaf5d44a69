"""The frame as an OpenEXR file made on the device (`ndt_hip --exr`): linear half or float samples, the depth map as the Z channel.

There is no EXR reader on the machines, so the yardsticks are a reader and a model writer written here from the definitions in
include/ndt_hip.h (the OpenEXR file layout) with Python's zlib and struct and numpy -- never the device's own output:
  * FLOAT is x.astype(float32), HALF is clip(x, -65504, 65504).astype(float16): numpy rounds a double directly to either, to
    nearest even; the reader compares bit patterns;
  * the reader checks the magic, the version, every attribute, the offset table and every block's header, inflates every block
    with zlib (which checks the deflate and the Adler-32 independently), undoes the predictor and the byte planes, and tells a raw
    block by the format's own rule: dataSize equal to the block's raw size;
  * the model writer makes a file of the same layout with zlib.compress, and the reader reads the samples back from it.
The double framebuffers the rendered files are compared with are those render() returns, which tests/test_gpu_parity.py pins to
the reference.
"""
import ctypes as C
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
LINES = 16
HOST = os.path.join(ROOT, "ndt_amd", "host")
DRIVER = os.path.join(HOST, "ndt_hip")
NEW_SYMBOLS = ("ndt_hip_exr_bound", "ndt_hip_encode_exr_device", "ndt_hip_encode_exr", "ndt_hip_render_exr", "ndt_hip_render_ssaa_exr")
NEW_METHODS = ("encode_exr", "encode_exr_device", "render_exr", "render_ssaa_exr")
HALF, FLOAT = 1, 2
PIXEL = {"half": HALF, "float": FLOAT}
DTYPE = {HALF: np.dtype("<f2"), FLOAT: np.dtype("<f4")}


# ---------------------------------------------------------------- yardsticks

def half_model(x):
    """the double rounded directly to binary16, nearest even, after the clamp to +-65504"""
    return np.clip(np.asarray(x, dtype=np.float64), -65504.0, 65504.0).astype(np.float16)


def float_model(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


def samples_model(x, pixel_type):
    return half_model(x) if pixel_type == HALF else float_model(x)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def clamp01(x):
    x = np.asarray(x, dtype=np.float64)
    m = np.where(1.0 < x, 1.0, x)
    return np.where(0.0 > m, 0.0, m)


def pixel_d2c(x):
    return (np.sqrt(clamp01(x)) * 255).astype(np.uint8)


def channel_list(pixel_type, with_z):
    """(name, pixelType, index into the R G B A framebuffer or None for the map) in the file's order"""
    chans = [("A", pixel_type, 3), ("B", pixel_type, 2), ("G", pixel_type, 1), ("R", pixel_type, 0)]
    return chans + [("Z", FLOAT, None)] if with_z else chans


def block_raw(fb, depth, pixel_type, y0, y1):
    """the raw bytes of scanlines y0 .. y1 - 1: per scanline, per channel in list order, width samples, little-endian"""
    out = []
    for y in range(y0, y1):
        for _, typ, src in channel_list(pixel_type, depth is not None):
            line = fb[y, :, src] if src is not None else depth[y]
            out.append(samples_model(line, typ).astype(DTYPE[typ]).tobytes())
    return b"".join(out)


def preprocess(raw):
    """the even bytes, then the odd ones; then out[0] = T[0], out[i] = T[i] - T[i-1] + 128 mod 256"""
    r = np.frombuffer(raw, dtype=np.uint8)
    t = np.concatenate([r[0::2], r[1::2]])
    out = t.copy()
    out[1:] = t[1:] - t[:-1] + np.uint8(128)        # uint8 arithmetic wraps
    return out.tobytes()


def unpreprocess(data):
    d = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
    d[1:] -= 128
    t = (np.cumsum(d) % 256).astype(np.uint8)
    half = (t.size + 1) // 2
    r = np.empty(t.size, dtype=np.uint8)
    r[0::2] = t[:half]
    r[1::2] = t[half:]
    return r.tobytes()


def attribute(name, typ, value):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(value)) + value


def model_header(width, rows, pixel_type, with_z):
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t, _ in channel_list(pixel_type, with_z)) + b"\0"
    window = struct.pack("<4i", 0, 0, width - 1, rows - 1)
    return (bytes([0x76, 0x2f, 0x31, 0x01]) + struct.pack("<I", 2) + attribute("channels", "chlist", chlist)
            + attribute("compression", "compression", b"\x03") + attribute("dataWindow", "box2i", window)
            + attribute("displayWindow", "box2i", window) + attribute("lineOrder", "lineOrder", b"\0")
            + attribute("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attribute("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
            + attribute("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")


def model_blocks(fb, depth, pixel_type):
    """[(raw bytes, preprocessed bytes)] of the file's blocks"""
    rows = fb.shape[0]
    raws = [block_raw(fb, depth, pixel_type, y, min(y + LINES, rows)) for y in range(0, rows, LINES)]
    return [(r, preprocess(r)) for r in raws]


def write_exr(fb, depth=None, pixel_type=HALF, level=6):
    """the model writer: the file of the layout above with zlib.compress as the deflate"""
    rows, width = fb.shape[:2]
    head = model_header(width, rows, pixel_type, depth is not None)
    chunks = []
    for k, (raw, pre) in enumerate(model_blocks(fb, depth, pixel_type)):
        z = zlib.compress(pre, level)
        data = z if len(z) < len(raw) else raw
        chunks.append(struct.pack("<ii", LINES * k, len(data)) + data)
    at, table = len(head) + 8 * len(chunks), b""
    for c in chunks:
        table += struct.pack("<Q", at)
        at += len(c)
    return head + table + b"".join(chunks)


def read_exr(data):
    """Reads a file of the layout above and accepts nothing else: returns (channels {name: [rows, width] array of its type},
    pixel type of the colour channels, [dataSize of every block], [True where the block is raw]).  Every byte of the file is
    accounted for."""
    assert data[:4] == bytes([0x76, 0x2f, 0x31, 0x01]) and struct.unpack("<I", data[4:8])[0] == 2
    pos, attrs, order = 8, {}, []
    while data[pos] != 0:
        end = data.index(b"\0", pos)
        name = data[pos:end].decode()
        pos = end + 1
        end = data.index(b"\0", pos)
        typ = data[pos:end].decode()
        pos = end + 1
        size, = struct.unpack("<i", data[pos:pos + 4])
        attrs[name] = (typ, data[pos + 4:pos + 4 + size])
        assert len(attrs[name][1]) == size
        order.append(name)
        pos += 4 + size
    pos += 1
    assert order == ["channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio", "screenWindowCenter",
                     "screenWindowWidth"]
    assert attrs["compression"] == ("compression", b"\x03") and attrs["lineOrder"] == ("lineOrder", b"\0")
    assert attrs["pixelAspectRatio"] == ("float", struct.pack("<f", 1.0)) and attrs["screenWindowWidth"] == ("float", struct.pack("<f", 1.0))
    assert attrs["screenWindowCenter"] == ("v2f", struct.pack("<2f", 0.0, 0.0))
    assert attrs["dataWindow"][0] == "box2i" and attrs["displayWindow"] == attrs["dataWindow"]
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    assert (x0, y0) == (0, 0) and x1 >= 0 and y1 >= 0
    width, rows = x1 + 1, y1 + 1
    typ, chl = attrs["channels"]
    assert typ == "chlist" and chl[-1] == 0
    chans, at = [], 0
    while at < len(chl) - 1:
        end = chl.index(b"\0", at)
        ptype, plinear, xs, ys = struct.unpack("<iB3xii", chl[end + 1:end + 17])
        assert chl[end + 6:end + 9] == b"\0\0\0" and (plinear, xs, ys) == (0, 1, 1) and ptype in (HALF, FLOAT)
        chans.append((chl[at:end].decode(), ptype))
        at = end + 17
    names = [n for n, _ in chans]
    assert names in (["A", "B", "G", "R"], ["A", "B", "G", "R", "Z"])
    pixel_type = chans[0][1]
    assert all(t == pixel_type for _, t in chans[:4]) and (len(chans) == 4 or chans[4][1] == FLOAT)
    line_bytes = sum(width * DTYPE[t].itemsize for _, t in chans)
    n_blocks = (rows + LINES - 1) // LINES
    offsets = struct.unpack("<%dQ" % n_blocks, data[pos:pos + 8 * n_blocks])
    pos += 8 * n_blocks
    out = {n: np.zeros((rows, width), dtype=DTYPE[t]) for n, t in chans}
    sizes, raw_flags = [], []
    for k in range(n_blocks):
        assert offsets[k] == pos, "block %d: the offset table says %d, the blocks so far end at %d" % (k, offsets[k], pos)
        assert k == 0 or offsets[k] > offsets[k - 1]
        y, size = struct.unpack("<ii", data[pos:pos + 8])
        lines = min(LINES, rows - LINES * k)
        n = lines * line_bytes
        assert y == LINES * k and 0 < size <= n
        body = data[pos + 8:pos + 8 + size]
        assert len(body) == size
        if size == n:
            raw = body
        else:
            z = zlib.decompressobj()
            pre = z.decompress(body)
            assert z.eof and z.unused_data == b"" and len(pre) == n, "block %d: %d bytes inflate to %d of %d" % (k, size, len(pre), n)
            raw = unpreprocess(pre)
        sizes.append(size)
        raw_flags.append(size == n)
        at = 0
        for line in range(lines):
            for name, t in chans:
                nb = width * DTYPE[t].itemsize
                out[name][LINES * k + line] = np.frombuffer(raw[at:at + nb], dtype=DTYPE[t])
                at += nb
        pos += 8 + size
    assert pos == len(data), "the blocks end at %d, the file at %d" % (pos, len(data))
    return out, pixel_type, sizes, raw_flags


def assert_decodes_to(data, fb, depth, pixel_type):
    """the file holds exactly the model's samples of fb (and depth), bit for bit; returns (block sizes, raw flags)"""
    chans, ptype, sizes, raw_flags = read_exr(data)
    assert ptype == pixel_type and ("Z" in chans) == (depth is not None)
    assert chans["R"].shape == fb.shape[:2]
    for name, _, src in channel_list(pixel_type, depth is not None):
        want = samples_model(fb[:, :, src], pixel_type) if src is not None else float_model(depth)
        differ = int((bits(chans[name]) != bits(want)).sum())
        assert differ == 0, "channel %s: %d of %d samples differ from the model" % (name, differ, want.size)
    return sizes, raw_flags


# above 1, negative, the zeros, denormal halves and the ties around them, the clamp, what a float cannot hold, NaN, and the
# double-rounding probes: as floats both are ties, as doubles neither is
SPECIALS = np.array([1.5, 7.25, -0.75, 0.0, -0.0, 2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -15, 1023.5 * 2.0 ** -24,
                     2.0 ** -14, 65504.0, 65519.0, 65520.0, -65520.0, 1e300, -1e300, np.inf, np.nan, 1 + 2.0 ** -11 + 2.0 ** -30,
                     1 + 2.0 ** -11 - 2.0 ** -30, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11 + 2.0 ** -30), 1e-40, 1e-300, 0.1, 1.0, 1000.0,
                     2.0 ** -26, 65503.99, 0.333])
WIDTHS = [1, 3, 256, 257, 300]
HEIGHTS = [1, 15, 16, 17, 33]


def aimed(width, rows):
    """a smooth image with every third value taken from SPECIALS in turn (a different start per size), and a map of the same kind"""
    rng = np.random.default_rng(1000 * width + rows)
    y, x, c = np.meshgrid(np.arange(rows), np.arange(width), np.arange(4), indexing="ij")
    fb = 0.25 + 0.003 * x + 0.01 * y + 0.2 * c + rng.uniform(0, 1e-3, (rows, width, 4))
    flat = fb.reshape(-1)
    idx = np.arange(0, flat.size, 3)
    flat[idx] = SPECIALS[(idx // 3 + width + rows) % SPECIALS.size]
    depth = 3.0 + 0.02 * x[:, :, 0] + rng.uniform(0, 1e-3, (rows, width))
    dflat = depth.reshape(-1)
    idx = np.arange(0, dflat.size, 5)
    dflat[idx] = SPECIALS[(idx // 5 + width) % SPECIALS.size]
    return fb, depth


def noise_float(width, rows, seed):
    """white noise in the bits of the floats: every exponent but those of NaN and infinity, as doubles that hold them exactly"""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2 ** 32, (rows, width, 4), dtype=np.uint64).astype(np.uint32)
    exp = (u >> 23) & 255
    u = np.where(exp == 255, u & ~np.uint32(1 << 23), u).astype(np.uint32)
    return u.view(np.float32).astype(np.float64)


# ---------------------------------------------------------------- CPU

def test_the_model_writer_and_the_reader_give_the_samples_back():
    for pixel_type in (HALF, FLOAT):
        for with_z in (False, True):
            for width, rows in ((1, 1), (3, 17), (257, 16), (300, 33)):
                fb, depth = aimed(width, rows)
                data = write_exr(fb, depth if with_z else None, pixel_type)
                sizes, _ = assert_decodes_to(data, fb, depth if with_z else None, pixel_type)
                assert len(sizes) == (rows + 15) // 16
    # white noise falls back to raw bytes in the model too; a flat image does not
    fb = noise_float(64, 20, 5)
    _, _, sizes, raw_flags = read_exr(write_exr(fb, None, FLOAT))
    assert raw_flags == [True, True] and sizes == [16 * 64 * 16, 4 * 64 * 16]
    assert read_exr(write_exr(np.full((20, 64, 4), 0.5), None, FLOAT))[3] == [False, False]
    # the two transforms are inverse to each other at odd and even lengths
    for n in (1, 2, 3, 8, 255):
        raw = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
        assert unpreprocess(preprocess(raw)) == raw
    assert preprocess(bytes([1, 10, 2, 20, 3])) == bytes([1, 129, 129, 135, 138])


def test_the_sample_models_are_the_definitions():
    h = lambda v: int(bits(half_model(np.array([v])))[0])
    assert h(1 + 2.0 ** -11 + 2.0 ** -30) == 0x3c01 and h(1 + 2.0 ** -11 - 2.0 ** -30) == 0x3c00       # 1 + 2^-10, and 1
    assert h(1 + 2.0 ** -11) == 0x3c00 and h(1 + 3 * 2.0 ** -11) == 0x3c02                           # ties to even
    # through float both probes are the tie 1 + 2^-11, which goes to the even 1: the double rounding the file must not have
    assert int(bits(float_model(np.array([1 + 2.0 ** -11 + 2.0 ** -30])).astype(np.float16))[0]) == 0x3c00
    assert [h(v) for v in (65504.0, 65519.0, 65520.0, 1e300, np.inf, -1e300)] == [0x7bff] * 5 + [0xfbff]
    assert h(np.nan) == 0x7e00 and h(0.0) == 0 and h(-0.0) == 0x8000
    assert [h(v) for v in (2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 3 * 2.0 ** -24, 2.0 ** -14, 1e-300)] == [1, 0, 1, 3, 0x0400, 0]
    f = lambda v: int(bits(float_model(np.array([v])))[0])
    assert f(1e300) == 0x7f800000 and f(1.0) == 0x3f800000 and f(-0.0) == 0x80000000 and f(1e-40) == 71362 and f(np.nan) == 0x7fc00000


def test_library_exports_and_binds_the_exr_entry_points():
    lib = nh.load_library()
    with open(os.path.join(ROOT, "include", "ndt_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in nh.API_SYMBOLS
        assert name + "(" in header
    assert "ndt_exr_params" in header and "ndt_exr_stats" in header
    for name in NEW_METHODS:
        assert callable(getattr(nh.NdtHip, name, None)), name
    assert callable(nh.exr_bound) and C.sizeof(nh.ExrParams) == 16 and C.sizeof(nh.ExrStats) == 40
    assert lib.ndt_hip_abi_version() == 3


def test_exr_bound_covers_the_all_raw_file_and_refuses_bad_arguments():
    lib = nh.load_library()
    for pixel in ("half", "float"):
        for with_z in (False, True):
            for w, h in ((1, 1), (300, 33), (1920, 1080), (7, 16)):
                head = len(model_header(w, h, PIXEL[pixel], with_z))
                line = w * (4 * DTYPE[PIXEL[pixel]].itemsize + (4 if with_z else 0))
                assert nh.exr_bound(w, h, pixel, with_z) == head + 16 * ((h + 15) // 16) + line * h
    for w, h in ((0, 1), (1, 0), (-1, 5), (5, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.ndt_hip_exr_bound(w, h, None, 0) < 0
    assert lib.ndt_hip_exr_bound(4, 4, None, 0) == nh.exr_bound(4, 4, "half")
    for bad in (3, -1, 17):
        ep = nh.ExrParams(bad)
        assert lib.ndt_hip_exr_bound(4, 4, C.byref(ep), 0) == NDT_E_INVALID
    # half RGBA is 8 bytes a pixel: raw bytes of 2^31 are refused, of 2^31 - 8 taken
    assert lib.ndt_hip_exr_bound(1 << 28, 1, None, 0) < 0 and lib.ndt_hip_exr_bound((1 << 28) - 1, 1, None, 0) > 0
    assert lib.ndt_hip_exr_bound(1 << 14, 1 << 14, None, 0) < 0 and lib.ndt_hip_exr_bound(1 << 14, (1 << 14) - 1, None, 0) > 0
    with pytest.raises(ValueError):
        nh.exr_bound(4, 4, "double")
    with pytest.raises(ValueError):
        nh.exr_bound(0, 4)


def _run_driver(cwd, *flags, scene="builtin:yaml"):
    assert os.path.exists(DRIVER), "ndt_amd/host/ndt_hip is not built"
    os.makedirs(str(cwd), exist_ok=True)
    return subprocess.run([DRIVER, "-s", scene, "-d", "4", "-f", "0", "-r", "96x54", "-l", "6"] + list(flags),
                          capture_output=True, text=True, cwd=str(cwd))


def test_driver_refuses_what_exr_does_not_go_with_by_name(tmp_path):
    """(CPU) every refusal ends the run non-zero with a message that names both options, before a scene is loaded or a device
    asked for: nothing is written."""
    for flags, words in ((["--exr", "--png"], ("--exr", "--png")),
                         (["--exr", "--jpeg"], ("--exr", "--jpeg")),
                         (["--exr", "--raw", "fb.f64"], ("--exr", "--raw")),
                         (["--exr", "--png", "--deflate", "gpu", "--png16"], ("--exr", "--png16")),
                         (["--exr", "--apng"], ("--exr", "--apng")),
                         (["--exr", "-z", "--depth", "gpu"], ("--exr", "--depth gpu")),
                         (["--exr", "-z", "--depth-png"], ("--exr", "--depth-png")),
                         (["--exr-pixel", "float"], ("--exr-pixel", "--exr")),
                         (["--exr-pixel", "half", "--png"], ("--exr-pixel", "--exr")),
                         (["--exr", "--exr-pixel", "double"], ("--exr-pixel", "half or float")),
                         (["--exr", "-g", "2"], ("--exr", "-g 2"))):
        r = _run_driver(tmp_path, *flags)
        assert r.returncode != 0, flags
        for w in words:
            assert w in r.stderr, (flags, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, (flags, r.stderr)       # the refusal and nothing else: no device was asked for
    assert not [p for p in tmp_path.rglob("*") if p.is_file()]


D2C_CROSSING_CAP = 0.001


def crossings(fb):
    """the samples whose 8-bit level changes when the double is rounded to float first"""
    return pixel_d2c(float_model(fb).astype(np.float64)) != pixel_d2c(fb)


def test_float_rounding_crosses_few_levels_of_the_golden_frame():
    """(CPU) the exception set of the driver test below, on the frame the driver renders (the golden framebuffer): pixel_d2c of the
    float samples is pixel_d2c of the doubles but where rounding to float crosses a level; under 0.1 % of the samples."""
    fb = golden("zoo4d").data["fb"]
    e = crossings(fb)
    print("zoo4d: float rounding crosses a level at %d of %d samples" % (int(e.sum()), e.size))
    assert e.sum() < D2C_CROSSING_CAP * e.size


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_z", [False, True], ids=["rgba", "rgbaz"])
@pytest.mark.parametrize("pixel", ["half", "float"])
@pytest.mark.parametrize("width", WIDTHS)
def test_encode_exr_on_aimed_arrays(gpu, width, pixel, with_z):
    """For half RGBA a full block is 128 w bytes: 256 fills exactly one deflate chunk, 257 starts a second; float with Z is 320 w.
    The heights give a short last block alone, a full block alone, and full blocks followed by a short one."""
    for rows in HEIGHTS:
        fb, depth = aimed(width, rows)
        data = gpu.encode_exr(fb, depth if with_z else None, pixel)
        st = gpu.exr_stats
        sizes, raw_flags = assert_decodes_to(data, fb, depth if with_z else None, PIXEL[pixel])
        line = width * (4 * DTYPE[PIXEL[pixel]].itemsize + (4 if with_z else 0))
        print("%dx%d %s%s: %d bytes of %d raw, blocks %s, %d raw, %.3f ms" % (width, rows, pixel, " + Z" if with_z else "", len(data),
                                                                             st.raw_bytes, sizes, st.blocks_raw, st.ms))
        assert st.file_bytes == len(data) <= nh.exr_bound(width, rows, pixel, with_z)
        assert st.raw_bytes == line * rows and st.blocks == len(sizes) == (rows + 15) // 16
        assert st.blocks_raw == sum(raw_flags) and st.launches == 4


@pytest.mark.gpu
def test_more_blocks_than_the_assembler_has_lanes(gpu):
    """1026 blocks: the assembler's 1024 lanes take two blocks each, and the last lanes none"""
    fb, depth = aimed(3, 16401)
    data = gpu.encode_exr(fb, depth, "half")
    sizes, raw_flags = assert_decodes_to(data, fb, depth, HALF)
    assert len(sizes) == gpu.exr_stats.blocks == 1026 and gpu.exr_stats.blocks_raw == sum(raw_flags)
    assert gpu.exr_stats.file_bytes == len(data) <= nh.exr_bound(3, 16401, "half", True)


@pytest.mark.gpu
def test_the_double_rounding_probes_and_the_edges_value_by_value(gpu):
    fb = np.zeros((1, (SPECIALS.size + 3) // 4, 4))
    fb.reshape(-1)[:SPECIALS.size] = SPECIALS
    chans, _, _, _ = read_exr(gpu.encode_exr(fb, None, "half"))
    got = np.stack([chans[n] for n in "RGBA"], axis=-1).reshape(-1)[:SPECIALS.size]
    want = half_model(SPECIALS)
    for v, g, w in zip(SPECIALS, bits(got), bits(want)):
        assert g == w, "%r: the file holds 0x%04x, the model 0x%04x" % (v, g, w)
    at = {float(v): int(b) for v, b in zip(SPECIALS, bits(got)) if v == v}
    assert at[1 + 2.0 ** -11 + 2.0 ** -30] == 0x3c01 and at[1 + 2.0 ** -11 - 2.0 ** -30] == 0x3c00
    assert not np.isinf(got.astype(np.float64)).any()
    assert int(bits(got)[list(np.isnan(SPECIALS)).index(True)]) == 0x7e00


@pytest.mark.gpu
def test_device_pointer_entry_is_the_host_pointer_entry(gpu):
    import torch
    fb, depth = aimed(300, 33)
    d_fb, d_depth = torch.from_numpy(fb).cuda(), torch.from_numpy(depth).cuda()
    torch.cuda.synchronize()
    for pixel in ("half", "float"):
        assert gpu.encode_exr_device(d_fb.data_ptr(), d_depth.data_ptr(), 300, 33, pixel) == gpu.encode_exr(fb, depth, pixel)
        assert gpu.encode_exr_device(d_fb.data_ptr(), None, 300, 33, pixel) == gpu.encode_exr(fb, None, pixel)
    # the same image, the same bytes, whatever was encoded in between
    assert gpu.encode_exr(fb, depth, "half") == gpu.encode_exr(fb, depth, "half")


@pytest.mark.gpu
def test_white_noise_falls_back_to_raw_bytes_and_flat_images_shrink(gpu):
    width, rows = 300, 33
    fb = noise_float(width, rows, 2024)
    data = gpu.encode_exr(fb, None, "float")
    st = gpu.exr_stats
    sizes, raw_flags = assert_decodes_to(data, fb, None, FLOAT)
    assert st.blocks_raw == st.blocks == 3 and all(raw_flags)
    assert sizes == [16 * width * 16, 16 * width * 16, 1 * width * 16]
    assert len(data) == nh.exr_bound(width, rows, "float")
    # one value: a run a chunk is about 127 length tokens (32768 / 258), a few dozen bytes against 32768: 2 % is generous
    for pixel, w, h, z in (("half", 256, 64, False), ("float", 300, 33, True)):
        flat = np.full((h, w, 4), 0.7312)
        depth = np.full((h, w), 12.5) if z else None
        data = gpu.encode_exr(flat, depth, pixel)
        st = gpu.exr_stats
        print("one value %dx%d %s: %d bytes of %d raw (%.3f %%)" % (w, h, pixel, len(data), st.raw_bytes, 100.0 * len(data) / st.raw_bytes))
        assert_decodes_to(data, flat, depth, PIXEL[pixel])
        assert st.blocks_raw == 0 and len(data) <= 0.02 * st.raw_bytes
    # half noise, half flat: both kinds of block in one file
    mixed = np.full((48, width, 4), 0.25)
    mixed[:24] = noise_float(width, 24, 7)
    data = gpu.encode_exr(mixed, None, "float")
    sizes, raw_flags = assert_decodes_to(data, mixed, None, FLOAT)
    assert raw_flags == [True, False, False] and gpu.exr_stats.blocks_raw == 1
    # block 1 is 8 lines of noise and 8 flat ones: the noise's half of the bytes at a little over 8 bits a literal, runs for the rest
    assert sizes[1] < 0.6 * 16 * width * 16 and sizes[2] < 0.02 * 16 * width * 16


@pytest.mark.gpu
def test_bad_arguments_are_refused_by_name_and_a_short_buffer_is_left_alone(gpu):
    lib = gpu.lib
    fb, depth = aimed(3, 2)
    out = np.zeros(4096, dtype=np.uint8)
    ep = nh.ExrParams(HALF)
    assert lib.ndt_hip_encode_exr(gpu.ctx, None, None, 3, 2, C.byref(ep), out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_exr(gpu.ctx, fb.ctypes.data, None, 3, 2, C.byref(ep), None, 4096, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_exr(None, fb.ctypes.data, None, 3, 2, C.byref(ep), out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_exr_device(gpu.ctx, None, None, 3, 2, C.byref(ep), out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert b"ndt_hip_encode_exr" in lib.ndt_hip_last_error()
    for w, h in ((0, 2), (3, 0), (-1, 2)):
        assert lib.ndt_hip_encode_exr(gpu.ctx, fb.ctypes.data, None, w, h, C.byref(ep), out.ctypes.data, 4096, None) == NDT_E_INVALID
    bad = nh.ExrParams(3)
    assert lib.ndt_hip_encode_exr(gpu.ctx, fb.ctypes.data, None, 3, 2, C.byref(bad), out.ctypes.data, 4096, None) == NDT_E_INVALID
    assert b"pixel type" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_render_exr(gpu.ctx, None, C.byref(ep), 0, out.ctypes.data, 4096, None, None) == NDT_E_INVALID
    assert lib.ndt_hip_render_ssaa_exr(gpu.ctx, None, 2, C.byref(ep), 0, out.ctypes.data, 4096, None, None) == NDT_E_INVALID
    geometry = gpu.params(4, 4, 1, row_step=0)
    assert lib.ndt_hip_render_exr(gpu.ctx, C.byref(geometry), C.byref(ep), 0, out.ctypes.data, 4096, None, None) == NDT_E_INVALID
    assert b"ndt_hip_render_exr: bad geometry" in lib.ndt_hip_last_error()
    assert not out.any()
    # the encoder needs no scene; params and stats are optional (NULL params: half)
    assert lib.ndt_hip_encode_exr(gpu.ctx, fb.ctypes.data, None, 3, 2, None, out.ctypes.data, 4096, None) == 0
    assert read_exr(out[:nh.exr_bound(3, 2)].tobytes()[:len(gpu.encode_exr(fb))])[1] == HALF
    # room one byte short: NDT_E_NOMEM with the size needed, and nothing written -- least of all behind `cap`
    for pixel, with_z in (("half", False), ("float", True)):
        pic, dm = aimed(300, 33)
        data = gpu.encode_exr(pic, dm if with_z else None, pixel)
        cap = len(data) - 1
        buf = np.full(cap + 64, 0xA5, dtype=np.uint8)
        short = nh.ExrStats()
        ep = nh.ExrParams(PIXEL[pixel])
        rc = lib.ndt_hip_encode_exr(gpu.ctx, pic.ctypes.data, dm.ctypes.data if with_z else None, 300, 33, C.byref(ep), buf.ctypes.data, cap,
                                    C.byref(short))
        assert rc == NDT_E_NOMEM
        assert str(len(data)) in lib.ndt_hip_last_error().decode() and short.file_bytes == len(data)
        assert (buf == 0xA5).all()


# a small golden case as tests/test_png16_device.py takes them, the driver's own frame, and a reflective one
RENDER_CASES = {"zoo4d": ("zoo4d", {}), "mirror": ("zoo3d_mirror", {}), "aa": ("aa_c3_random4d_depth", {"aa": (20, 3)}),
                "side_by_side": ("st_zoo4d_sbs", {"stereo": 1}), "row_shard": ("c3_random4d", {"row_begin": 1, "row_step": 3})}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(RENDER_CASES))
def test_render_exr_is_the_model_of_the_double_framebuffer(gpu, case):
    name, kw = RENDER_CASES[case]
    g = golden(name)
    gpu.upload_scene(g.scene)
    fb, _ = gpu.render(g.width, g.height, g.depth, **kw)
    for pixel in ("float", "half"):
        data, _ = gpu.render_exr(g.width, g.height, g.depth, pixel=pixel, **kw)
        st = gpu.exr_stats
        sizes, _ = assert_decodes_to(data, fb, None, PIXEL[pixel])
        model = sum(8 + min(len(zlib.compress(pre, 6)), len(raw)) for raw, pre in model_blocks(fb, None, PIXEL[pixel]))
        print("%s %s %s: %d bytes of %d raw; blocks %d against %d with zlib level 6 (x%.3f); %.3f ms; brightest sample %.3f" % (
            name, case, pixel, len(data), st.raw_bytes, sum(sizes) + 8 * len(sizes), model, (sum(sizes) + 8 * len(sizes)) / model, st.ms,
            float(fb.max())))
        assert st.file_bytes == len(data) and st.blocks == (fb.shape[0] + 15) // 16


@pytest.mark.gpu
def test_render_exr_with_the_map_as_its_z_channel(gpu):
    g = golden("depth_c3_random4d")
    gpu.upload_scene(g.scene)
    fb, dm, _ = gpu.render(g.width, g.height, g.depth, depth_map=True)
    assert (dm > 0).any() and dm.min() == 0.0 and dm.max() != 1.0       # a map that a stretch to 0 .. 1 would change
    for pixel in ("float", "half"):
        data, _ = gpu.render_exr(g.width, g.height, g.depth, pixel=pixel, depth_map=True)
        assert_decodes_to(data, fb, dm, PIXEL[pixel])
        z = read_exr(data)[0]["Z"]
        assert bits(z).tolist() == bits(float_model(dm)).tolist() and z.max() == np.float32(dm.max())      # unstretched
    # the colour channels do not depend on the map beside them
    with_z, without = read_exr(data)[0], read_exr(gpu.render_exr(g.width, g.height, g.depth, pixel="half")[0])[0]
    assert all(np.array_equal(bits(with_z[n]), bits(without[n])) for n in "ABGR")


@pytest.mark.gpu
def test_render_ssaa_exr_is_the_model_of_render_ssaa(gpu):
    g = golden("c3_random4d")
    gpu.upload_scene(g.scene)
    fb, dm, _ = gpu.render_ssaa(g.width, g.height, g.depth, 2, depth_map=True)
    data, _ = gpu.render_ssaa_exr(g.width, g.height, g.depth, 2, pixel="float")
    assert_decodes_to(data, fb, None, FLOAT)
    assert gpu.ssaa_launches() == 2
    data, _ = gpu.render_ssaa_exr(g.width, g.height, g.depth, 2, pixel="half", depth_map=True)
    assert_decodes_to(data, fb, dm, HALF)
    with pytest.raises(nh.NdtHipError):
        gpu.render_ssaa_exr(g.width, g.height, g.depth, 9)


# ---------------------------------------------------------------- driver

@pytest.fixture(scope="module")
def zoo(tmp_path_factory):
    """tests/scenes/parity_zoo.c compiled against this repository's host headers, as tests/test_depth_device.py builds it: the
    driver tests need no binary of the reference, so they never skip."""
    d = tmp_path_factory.mktemp("zooexr")
    (d / "scenes").mkdir()
    for h in os.listdir(os.path.join(HOST, "include")):
        os.symlink(os.path.join(HOST, "include", h), d / h)
    shutil.copy(os.path.join(ROOT, "tests", "scenes", "parity_zoo.c"), d / "scenes" / "parity_zoo.c")
    so = str(d / "scenes" / "parity_zoo.so")
    r = subprocess.run(["gcc", "-O2", "-std=c99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-o", so, str(d / "scenes" / "parity_zoo.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return so


def read_png8(data):
    """the pixels [h, w, 4] of an 8-bit RGBA PNG with filters 0 / 1 / 2"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if typ == b"IHDR":
            w, h, depth, colour = struct.unpack(">IIBB", body[:10])
            assert (depth, colour) == (8, 6)
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)
    out = np.zeros((h, w, 4), dtype=np.uint8)
    for r in range(h):
        row = raw[r, 1:].reshape(w, 4)
        out[r] = np.cumsum(row, axis=0, dtype=np.uint8) if raw[r, 0] == 1 else row + out[r - 1] if raw[r, 0] == 2 and r else row
    return out


@pytest.mark.gpu
def test_driver_writes_one_exr_with_the_map_inside(zoo, tmp_path):
    """`--exr -z` writes one .exr that the reader accepts, with the map `--raw` dumps as its Z channel, no depth/ file, and says so;
    with `--ssaa 2 -j 2 --exr-pixel float` it is the float model of the folded doubles."""
    r = _run_driver(tmp_path / "raw", "-z", "--raw", "fb.f64", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    fb = np.fromfile(str(tmp_path / "raw" / "fb.f64"), dtype=np.float64).reshape(54, 96, 4)
    dm = np.fromfile(str(tmp_path / "raw" / "fb.f64.depth"), dtype=np.float64).reshape(54, 96)

    r = _run_driver(tmp_path / "one", "--exr", "-z", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    found = [p for p in (tmp_path / "one").rglob("*") if p.is_file()]
    assert len(found) == 1 and found[0].suffix == ".exr" and not (tmp_path / "one" / "depth").exists()
    assert found[0].name == "parity_zoo_96x54_0000.exr" or found[0].name.endswith("_96x54_0000.exr")
    data = found[0].read_bytes()
    assert "encoded EXR of %d bytes on GPU 0 in 4 launches" % len(data) in r.stdout
    assert_decodes_to(data, fb, dm, HALF)

    r = _run_driver(tmp_path / "raw2", "--ssaa", "2", "--raw", "fb.f64", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    fb2 = np.fromfile(str(tmp_path / "raw2" / "fb.f64"), dtype=np.float64).reshape(54, 96, 4)
    r = _run_driver(tmp_path / "ssaa", "--exr", "--exr-pixel", "float", "--ssaa", "2", "-j", "2", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    found = list((tmp_path / "ssaa" / "images").rglob("*.exr"))
    assert len(found) == 1 and "supersampled 2x2 on GPU 0 in 2 launches" in r.stdout and "encoded EXR of " in r.stdout
    assert_decodes_to(found[0].read_bytes(), fb2, None, FLOAT)


@pytest.mark.gpu
def test_driver_exr_beside_the_png_of_the_same_frame(zoo, tmp_path):
    """pixel_d2c of the decoded float channels is the PNG's bytes, except where rounding to float crosses a level: that set is
    computed from the doubles (`--raw`), and is under 0.1 % of the samples (the CPU test above shows the model alone is)."""
    r = _run_driver(tmp_path / "raw", "--raw", "fb.f64", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    fb = np.fromfile(str(tmp_path / "raw" / "fb.f64"), dtype=np.float64).reshape(54, 96, 4)
    r = _run_driver(tmp_path / "png", "--png", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    pngs = list((tmp_path / "png" / "images").rglob("*.png"))
    r = _run_driver(tmp_path / "exr", "--exr", "--exr-pixel", "float", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    exrs = list((tmp_path / "exr" / "images").rglob("*.exr"))
    assert len(pngs) == 1 and len(exrs) == 1 and exrs[0].with_suffix(".png").name == pngs[0].name
    assert exrs[0].parent.relative_to(tmp_path / "exr") == pngs[0].parent.relative_to(tmp_path / "png")
    pixels = read_png8(pngs[0].read_bytes())
    chans = read_exr(exrs[0].read_bytes())[0]
    decoded = np.stack([chans[n] for n in "RGBA"], axis=-1).astype(np.float64)
    allowed = crossings(fb)
    differ = pixel_d2c(decoded) != pixels
    print("96x54 zoo: %d samples differ between pixel_d2c of the float file and the PNG; float rounding crosses a level at %d of %d"
          % (int(differ.sum()), int(allowed.sum()), allowed.size))
    assert allowed.sum() < D2C_CROSSING_CAP * allowed.size
    assert not (differ & ~allowed).any()
    assert decoded.max() > 1.0 or fb.max() <= 1.0       # what is brighter than 1 is still there
