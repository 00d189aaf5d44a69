"""What a pixel shows, in the frame's OpenEXR file (`ndt_hip --exr --exr-aov`): the object the primary ray hits, the hit point in
all N coordinates and the normal there, as planes (render_features) and as the channels id, P.*, N.* of the file.

The yardsticks are written here and are never the device's own output:
  * the planes are compared with trace_rays on the rays the feature pass itself returns -- the entry the aimed-ray tests pin to the
    reference bit for bit --, with the CPU oracle on the same rays, and with the depth map of the same frame: 1 / v_dist(P, ray_o),
    v_dist restated below in the oracle's order (vectNd_dot's even and odd lane sums, then the root);
  * the file is read by a strict reader of the channel-list layout (the approach of tests/test_exr_device.py, with a channel list
    instead of A B G R [Z] and UINT samples): magic, version, every attribute, a channel list sorted byte-wise, the offset table,
    every block's header, every stream through zlib, every byte of the file accounted for; a model writer makes files of the same
    layout with zlib.compress;
  * FLOAT is x.astype(float32), HALF clip(x, -65504, 65504).astype(float16), UINT the int32's bits.
"""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, GOLDEN, golden

from ndt_amd import hip as nh
from ndt_amd import load_scene

NDT_E_INVALID, NDT_E_UNSUPPORTED, NDT_E_NOMEM = -1, -2, -4
LINES = 16
EPSILON = 1e-4
HOST = os.path.join(ROOT, "ndt_amd", "host")
DRIVER = os.path.join(HOST, "ndt_hip")
NEW_SYMBOLS = ("ndt_hip_render_features", "ndt_hip_render_features_device", "ndt_hip_features_launches", "ndt_hip_exr_features_bound",
               "ndt_hip_encode_exr_features_device", "ndt_hip_render_exr_features", "ndt_hip_render_ssaa_exr_features")
NEW_METHODS = ("render_features", "features_launches", "encode_exr_features_device", "render_exr", "render_ssaa_exr")
UINT, HALF, FLOAT = 0, 1, 2
PIXEL = {"half": HALF, "float": FLOAT}
DTYPE = {UINT: np.dtype("<u4"), HALF: np.dtype("<f2"), FLOAT: np.dtype("<f4")}
ID, POSITION, NORMAL = 1, 2, 4
ALL = ("id", "position", "normal")
NAMES = {ID: "id", POSITION: "position", NORMAL: "normal"}


def names_of(mask):
    return tuple(n for bit, n in NAMES.items() if mask & bit)


# ---------------------------------------------------------------- yardsticks

def half_model(x):
    return np.clip(np.asarray(x, dtype=np.float64), -65504.0, 65504.0).astype(np.float16)


def float_model(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def channel_names(dims, mask, with_z):
    """(name, pixel type or None for the colour's) in the order include/ndt_hip.h fixes: A B G, N.*, P.*, R, Z, id"""
    out = [("A", None), ("B", None), ("G", None)]
    if mask & NORMAL:
        out += [("N.%02d" % c, FLOAT) for c in range(dims)]
    if mask & POSITION:
        out += [("P.%02d" % c, FLOAT) for c in range(dims)]
    out.append(("R", None))
    if with_z:
        out.append(("Z", FLOAT))
    if mask & ID:
        out.append(("id", UINT))
    return out


def model_channels(fb, dm, planes, mask, pixel_type):
    """[(name, pixel type, [rows, width] samples of that type)] of the file of a framebuffer, a map (or None) and feature planes"""
    dims = planes["position"].shape[0] if "position" in planes else planes["normal"].shape[0] if "normal" in planes else 0
    colour = {"R": 0, "G": 1, "B": 2, "A": 3}
    out = []
    for name, typ in channel_names(dims, mask, dm is not None):
        if name in colour:
            x = fb[:, :, colour[name]]
            out.append((name, pixel_type, (half_model(x) if pixel_type == HALF else float_model(x)).astype(DTYPE[pixel_type])))
        elif name == "Z":
            out.append((name, FLOAT, float_model(dm)))
        elif name == "id":
            out.append((name, UINT, np.ascontiguousarray(planes["id"]).view(np.uint32)))
        else:
            src = planes["normal" if name[0] == "N" else "position"][int(name[2:])]
            out.append((name, FLOAT, float_model(src)))
    return out


def preprocess(raw):
    r = np.frombuffer(raw, dtype=np.uint8)
    t = np.concatenate([r[0::2], r[1::2]])
    out = t.copy()
    out[1:] = t[1:] - t[:-1] + np.uint8(128)
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


def model_header(width, rows, chans):
    """chans: [(name, pixel type)]"""
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t in chans) + b"\0"
    window = struct.pack("<4i", 0, 0, width - 1, rows - 1)
    return (bytes([0x76, 0x2f, 0x31, 0x01]) + struct.pack("<I", 2) + attribute("channels", "chlist", chlist)
            + attribute("compression", "compression", b"\x03") + attribute("dataWindow", "box2i", window)
            + attribute("displayWindow", "box2i", window) + attribute("lineOrder", "lineOrder", b"\0")
            + attribute("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attribute("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
            + attribute("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")


def write_exr(channels, level=6):
    """the model writer: channels = [(name, pixel type, [rows, width] array)] in file order; zlib.compress is the deflate"""
    rows, width = channels[0][2].shape
    head = model_header(width, rows, [(n, t) for n, t, _ in channels])
    chunks = []
    for k, y0 in enumerate(range(0, rows, LINES)):
        raw = b"".join(np.ascontiguousarray(a[y]).astype(DTYPE[t]).tobytes() for y in range(y0, min(y0 + LINES, rows)) for _, t, a in channels)
        z = zlib.compress(preprocess(raw), level)
        data = z if len(z) < len(raw) else raw
        chunks.append(struct.pack("<ii", LINES * k, len(data)) + data)
    at, table = len(head) + 8 * len(chunks), b""
    for c in chunks:
        table += struct.pack("<Q", at)
        at += len(c)
    return head + table + b"".join(chunks)


def read_exr(data):
    """Reads a single-part ZIP scanline file with a channel list and accepts nothing else: returns ([(name, pixel type)] in file
    order, {name: [rows, width] array of its type}, [dataSize of every block], [True where the block is raw]).  The channel list
    must be sorted byte-wise, strictly; every byte of the file is accounted for."""
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
        assert 0 < end - at < 256
        ptype, plinear, xs, ys = struct.unpack("<iB3xii", chl[end + 1:end + 17])
        assert chl[end + 6:end + 9] == b"\0\0\0" and (plinear, xs, ys) == (0, 1, 1) and ptype in (UINT, HALF, FLOAT)
        chans.append((chl[at:end], ptype))
        at = end + 17
    assert at == len(chl) - 1
    raw_names = [n for n, _ in chans]
    assert all(a < b for a, b in zip(raw_names, raw_names[1:])), "the channel list is not sorted byte-wise: %r" % (raw_names,)
    chans = [(n.decode(), t) for n, t in chans]
    line_bytes = sum(width * DTYPE[t].itemsize for _, t in chans)
    n_blocks = (rows + LINES - 1) // LINES
    offsets = struct.unpack("<%dQ" % n_blocks, data[pos:pos + 8 * n_blocks])
    pos += 8 * n_blocks
    out = {n: np.zeros((rows, width), dtype=DTYPE[t]) for n, t in chans}
    sizes, raw_flags = [], []
    for k in range(n_blocks):
        assert offsets[k] == pos, "block %d: the offset table says %d, the blocks so far end at %d" % (k, offsets[k], pos)
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
            assert zlib.decompress(body) == pre
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
    return chans, out, sizes, raw_flags


def assert_file_is(data, want):
    """the file's channel list is exactly want's, and every channel holds want's samples bit for bit; returns (sizes, raw flags)"""
    chans, got, sizes, raw_flags = read_exr(data)
    assert chans == [(n, t) for n, t, _ in want], (chans, [(n, t) for n, t, _ in want])
    for name, _, samples in want:
        differ = int((bits(got[name]) != bits(samples)).sum())
        assert differ == 0, "channel %s: %d of %d samples differ from the model" % (name, differ, samples.size)
    return sizes, raw_flags


def v_dist(a, b):
    """vectNd_dist of [dims, ...] arrays in the oracle's order: v_sub, then vectNd_dot's lanes (vectNd.h:215-227: lane 0 sums the
    even components, lane 1 the odd ones, each left to right), their sum, the root"""
    d = a - b
    s0, s1 = d[0] * d[0], d[1] * d[1]
    for i in range(2, d.shape[0], 2):
        s0 = s0 + d[i] * d[i]
        if i + 1 < d.shape[0]:
            s1 = s1 + d[i + 1] * d[i + 1]
    return np.sqrt(s0 + s1)


def noise_doubles(shape, seed):
    """doubles that hold white-noise floats exactly: every exponent but those of NaN and infinity"""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)
    exp = (u >> 23) & 255
    u = np.where(exp == 255, u & ~np.uint32(1 << 23), u).astype(np.uint32)
    return u.view(np.float32).astype(np.float64)


# ---------------------------------------------------------------- CPU

def test_library_exports_and_binds_the_feature_entry_points():
    lib = nh.load_library()
    with open(os.path.join(ROOT, "include", "ndt_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in nh.API_SYMBOLS
        assert name + "(" in header
    assert "ndt_feature_planes" in header and "NDT_FEATURE_ID = 1, NDT_FEATURE_POSITION = 2, NDT_FEATURE_NORMAL = 4" in header
    for name in NEW_METHODS:
        assert callable(getattr(nh.NdtHip, name, None)), name
    assert callable(nh.exr_features_bound) and C.sizeof(nh.FeaturePlanes) == 40
    assert nh.feature_mask(ALL) == 7 and nh.feature_mask(("normal", "id", "id")) == 5
    for bad in ((), ("depth",), 0, 8):
        with pytest.raises(ValueError):
            nh.feature_mask(bad)
    assert lib.ndt_hip_abi_version() == 3 and "#define NDT_HIP_ABI_VERSION 3" in header


def test_features_bound_is_the_all_raw_file_and_refuses_bad_arguments():
    lib = nh.load_library()
    for dims in (3, 4, 12):
        for mask in range(1, 8):
            for with_z in (False, True):
                for pixel in ("half", "float"):
                    for w, h in ((1, 1), (33, 17), (257, 33)):
                        chans = [(n, PIXEL[pixel] if t is None else t) for n, t in channel_names(dims, mask, with_z)]
                        line = sum(w * DTYPE[t].itemsize for _, t in chans)
                        want = len(model_header(w, h, chans)) + 16 * ((h + 15) // 16) + line * h
                        assert nh.exr_features_bound(w, h, dims, names_of(mask), pixel, with_z) == want, (dims, mask, with_z, pixel, w, h)
    # ... which the model writer reaches with incompressible samples in every channel
    rng = np.random.default_rng(3)
    planes = {"id": rng.integers(-2 ** 31, 2 ** 31, (20, 9)).astype(np.int32), "position": noise_doubles((12, 20, 9), 4), "normal": noise_doubles((12, 20, 9), 5)}
    data = write_exr(model_channels(noise_doubles((20, 9, 4), 6), noise_doubles((20, 9), 7), planes, 7, FLOAT))
    assert read_exr(data)[3] == [True, True] and len(data) == nh.exr_features_bound(9, 20, 12, ALL, "float", True)
    ep = nh.ExrParams(HALF)
    for dims in (2, 13, 0, -1):
        assert lib.ndt_hip_exr_features_bound(4, 4, C.byref(ep), 0, dims, 7) == NDT_E_INVALID
    for mask in (0, 8, 15, -1):
        assert lib.ndt_hip_exr_features_bound(4, 4, C.byref(ep), 0, 4, mask) == NDT_E_INVALID
    for w, h in ((0, 1), (1, 0), (-1, 5), (5, -1)):
        assert lib.ndt_hip_exr_features_bound(w, h, C.byref(ep), 0, 4, 7) == NDT_E_INVALID
    bad = nh.ExrParams(3)
    assert lib.ndt_hip_exr_features_bound(4, 4, C.byref(bad), 0, 4, 7) == NDT_E_INVALID
    assert lib.ndt_hip_exr_features_bound(4, 4, None, 1, 4, 7) == nh.exr_features_bound(4, 4, 4, ALL, "half", True)
    # 12-D with everything is 4 * 2 + 26 * 4 = 112 bytes a pixel in half: raw bytes beyond 2^31 - 1 are refused
    assert lib.ndt_hip_exr_features_bound(1 << 14, 1 << 11, None, 1, 12, 7) < 0 and lib.ndt_hip_exr_features_bound(1 << 13, 1 << 11, None, 1, 12, 7) > 0


def test_the_model_writer_and_the_reader_give_thirty_channels_back():
    rng = np.random.default_rng(11)
    for pixel_type in (HALF, FLOAT):
        for width, rows in ((1, 1), (33, 17), (257, 33)):
            fb = rng.uniform(-2, 2, (rows, width, 4))
            dm = rng.uniform(0, 3, (rows, width))
            planes = {"id": rng.integers(0, 40, (rows, width)).astype(np.int32), "position": rng.normal(0, 30, (12, rows, width)),
                      "normal": rng.normal(0, 1, (12, rows, width))}
            want = model_channels(fb, dm, planes, 7, pixel_type)
            assert len(want) == 30 and [n for n, _, _ in want] == sorted(n for n, _, _ in want)
            assert [n for n, _, _ in want][:4] == ["A", "B", "G", "N.00"] and [n for n, _, _ in want][-3:] == ["R", "Z", "id"]
            sizes, _ = assert_file_is(write_exr(want), want)
            assert len(sizes) == (rows + 15) // 16
    # the reader refuses a channel list that is not sorted, and one with a repeated name
    for order in ([1, 0, 2], [0, 0, 1]):
        chans = [("A", FLOAT, np.zeros((2, 2), np.float32)), ("B", FLOAT, np.ones((2, 2), np.float32)), ("id", UINT, np.zeros((2, 2), np.uint32))]
        with pytest.raises(AssertionError, match="not sorted"):
            read_exr(write_exr([chans[k] for k in order]))
    # subsets: only the groups of the mask appear
    assert [n for n, _ in channel_names(3, ID, False)] == ["A", "B", "G", "R", "id"]
    assert [n for n, _ in channel_names(3, NORMAL, True)] == ["A", "B", "G", "N.00", "N.01", "N.02", "R", "Z"]
    # v_dist is the lane order, not a plain sum: a case where the two differ in the last bit exists among random vectors
    a, b = rng.normal(0, 1, (7, 2000)), rng.normal(0, 1, (7, 2000))
    plain = np.sqrt(((a - b) ** 2).sum(axis=0))
    assert np.allclose(v_dist(a, b), plain, rtol=1e-15) and (v_dist(a, b) != plain).any()


def _run_driver(cwd, *flags, scene="builtin:yaml", dims=4, size="96x54"):
    assert os.path.exists(DRIVER), "ndt_amd/host/ndt_hip is not built"
    os.makedirs(str(cwd), exist_ok=True)
    return subprocess.run([DRIVER, "-s", scene, "-d", str(dims), "-f", "0", "-r", size, "-l", "6"] + list(flags),
                          capture_output=True, text=True, cwd=str(cwd))


def test_driver_refuses_what_exr_aov_does_not_go_with_by_name(tmp_path):
    """(CPU) every refusal ends the run non-zero with one line on stderr that names the cause, before a scene is loaded or a device
    asked for: nothing is written."""
    for flags, words in ((["--exr-aov", "all"], ("--exr-aov", "--exr")),
                         (["--png", "--exr-aov", "id"], ("--exr-aov", "--exr")),
                         (["--exr", "--exr-aov", "id,depth"], ("--exr-aov", "'depth'", "id, position, normal")),
                         (["--exr", "--exr-aov", ""], ("--exr-aov", "empty")),
                         (["--exr", "--exr-aov", "id,,normal"], ("--exr-aov", "empty")),
                         (["--exr", "--exr-aov", "all", "-a", "20,3"], ("--exr-aov", "-a")),
                         (["--exr", "--exr-aov", "all", "-n", "4"], ("--exr-aov", "-n 4")),
                         (["--exr", "--exr-aov", "position", "-m", "a"], ("--exr-aov", "-m a")),
                         (["--exr", "--exr-aov", "position", "-m", "h"], ("--exr-aov", "-m h")),
                         (["--exr", "--exr-aov", "all", "-g", "2"], ("--exr", "-g 2")),
                         (["--exr", "--exr-aov", "all", "--png"], ("--exr", "--png"))):
        r = _run_driver(tmp_path, *flags)
        assert r.returncode != 0, flags
        for w in words:
            assert w in r.stderr, (flags, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, (flags, r.stderr)       # the refusal and nothing else: no device was asked for
    assert not [p for p in tmp_path.rglob("*") if p.is_file()]


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


def rays_of(f):
    """the (n, 2 dims + 1) batch trace_rays takes, of the rays a feature pass returned, closest hit"""
    d = f["ray_o"].shape[0]
    rays = np.empty((f["id"].size, 2 * d + 1))
    rays[:, :d] = f["ray_o"].reshape(d, -1).T
    rays[:, d:2 * d] = f["ray_v"].reshape(d, -1).T
    rays[:, 2 * d] = -1.0
    return rays


# 33 x 17: partial 8 x 8 tiles on both edges; one row, one pixel, a row shard; 3-D, 4-D, 12-D and a stereo scene
PLANE_CASES = {"mirror3d": ("zoo3d_mirror", 33, 17, {}), "zoo4d": ("zoo4d", 33, 17, {}), "random4d": ("c3_random4d", 33, 17, {}),
               "zoo12d": ("zoo12d", 33, 17, {}), "sbs4d": ("st_zoo4d_sbs", 33, 17, {"stereo": 1}), "one_row": ("zoo4d", 64, 1, {}),
               "one_pixel": ("zoo4d", 1, 1, {}), "row_shard": ("c3_random4d", 33, 17, {"row_begin": 1, "row_step": 3})}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(PLANE_CASES))
def test_planes_are_the_ray_apis_answers_for_the_pixels_own_rays(gpu, oracle, case):
    name, w, h, kw = PLANE_CASES[case]
    g = golden(name)
    d = g.scene.dims
    gpu.upload_scene(g.scene)
    f = gpu.render_features(w, h, g.depth, rays=True, **kw)
    rows = nh.shard_rows(h, kw.get("row_begin", 0), kw.get("row_step", 1))
    assert f["id"].shape == (rows, w) and f["id"].dtype == np.int32 and gpu.features_launches() == 4
    assert all(f[k].shape == (d, rows, w) for k in ("position", "normal", "ray_o", "ray_v"))
    rays = rays_of(f)
    obj, hit, nrm = gpu.trace_rays(rays)
    ident, pos, nor = f["id"].reshape(-1), f["position"].reshape(d, -1).T, f["normal"].reshape(d, -1).T
    # the EPSILON rule (ndt.c:376): an answer of the API the planes show as no hit lies within EPSILON of the ray's origin
    zeroed = (ident == 0) & (obj >= 0)
    assert (v_dist(hit[zeroed].T, rays[zeroed, :d].T) <= EPSILON).all()
    keep = ~zeroed
    assert np.array_equal(ident[keep] - 1, obj[keep])
    assert same_bits(pos[keep], hit[keep]) and same_bits(nor[keep], nrm[keep])
    assert not pos[ident == 0].any() and not nor[ident == 0].any() and same_bits(pos[ident == 0], np.zeros_like(pos[ident == 0]))
    print("%s: %d pixels, %d hits on %d objects, %d within EPSILON of the eye" % (case, ident.size, int((ident > 0).sum()),
                                                                              len(set(ident[ident > 0])), int(zeroed.sum())))
    assert (ident > 0).any() or w * h == 1
    # the rays are unit vectors from the eye; without rays the planes are the same
    assert np.allclose(v_dist(f["ray_v"], np.zeros_like(f["ray_v"])), 1.0, atol=1e-12)
    again = gpu.render_features(w, h, g.depth, **kw)
    assert sorted(again) == ["id", "normal", "position"] and all(same_bits(again[k], f[k]) for k in again)
    # ... and the CPU oracle answers these rays as the device does, to the last bit (what the aimed-ray tests require of trace_rays)
    want = oracle.trace(g.scene, rays)
    assert np.array_equal(obj, want[0]) and same_bits(hit, want[1]) and same_bits(nrm, want[2])


DEPTH_CASES = {"mirror3d": ("zoo3d_mirror", 33, 17, {}), "zoo4d": ("zoo4d", 33, 17, {}), "random4d": ("c3_random4d", 33, 17, {}),
               "zoo12d": ("zoo12d", 33, 17, {}), "side_by_side": ("st_zoo4d_sbs", 34, 17, {"stereo": 1}),
               "over_under": ("st_zoo4d_sbs", 33, 18, {"stereo": 2}), "row_shard": ("c3_random4d", 33, 17, {"row_begin": 1, "row_step": 3})}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(DEPTH_CASES))
def test_planes_tie_to_the_depth_map_of_the_same_frame(gpu, case):
    """the map is 0 exactly where id is 0, and 1 / v_dist(P, ray_o) bit for bit elsewhere: plane pixel (r, x) is image pixel (r, x)"""
    name, w, h, kw = DEPTH_CASES[case]
    g = golden(name)
    d = g.scene.dims
    gpu.upload_scene(g.scene)
    _, dm, _ = gpu.render(w, h, g.depth, depth_map=True, **kw)
    f = gpu.render_features(w, h, g.depth, rays=True, **kw)
    assert dm.shape == f["id"].shape
    assert np.array_equal(dm == 0, f["id"] == 0)
    hit = f["id"] > 0
    want = 1.0 / v_dist(f["position"][:, hit], f["ray_o"][:, hit])
    differ = int((bits(dm[hit]) != bits(want)).sum())
    print("%s: %d hits of %d pixels, %d differ from 1 / v_dist(P, ray_o)" % (case, int(hit.sum()), hit.size, differ))
    assert hit.any() and differ == 0
    # each half's rays start at that eye
    st, vecs = g.scene.struct, np.asarray(g.scene.vecs)
    if kw.get("stereo"):
        left, right = vecs[st.cam_left_eye_off:st.cam_left_eye_off + d], vecs[st.cam_right_eye_off:st.cam_right_eye_off + d]
        first = f["ray_o"][:, :, :w // 2] if kw["stereo"] == 1 else f["ray_o"][:, :h // 2, :]
        second = f["ray_o"][:, :, w // 2:] if kw["stereo"] == 1 else f["ray_o"][:, h // 2:, :]
        assert (first == left[:, None, None]).all() and (second == right[:, None, None]).all() and (left != right).any()
    else:
        eye = vecs[st.cam_pos_off:st.cam_pos_off + d]
        assert (f["ray_o"] == eye[:, None, None]).all()


@pytest.mark.gpu
def test_an_eye_on_a_surface_keeps_planes_map_and_ray_api_consistent(gpu):
    """the camera moved onto the point the centre pixel shows: rays that start on (or within EPSILON of) a surface.  Whatever the
    intersectors answer there, a hit the planes drop lies within EPSILON of the eye, the map is 0 exactly where id is 0, and the
    rest are the ray API's answers and the map's distances"""
    g = golden("zoo4d")
    d, w, h = g.scene.dims, 33, 17
    gpu.upload_scene(g.scene)
    f = gpu.render_features(w, h, g.depth)
    assert f["id"][h // 2, w // 2] > 0
    fs = load_scene(os.path.join(GOLDEN, g.meta["scene_file"]))     # a copy of its own: the cached scene stays as it is
    fs._vecs[fs.cam["pos"]:fs.cam["pos"] + d] = [float(x) for x in f["position"][:, h // 2, w // 2]]
    fs._struct = None
    fs.finalize()
    gpu.upload_scene(fs)
    _, dm, _ = gpu.render(w, h, g.depth, depth_map=True)
    f = gpu.render_features(w, h, g.depth, rays=True)
    rays = rays_of(f)
    obj, hit, nrm = gpu.trace_rays(rays)
    ident, pos, nor = f["id"].reshape(-1), f["position"].reshape(d, -1).T, f["normal"].reshape(d, -1).T
    zeroed = (ident == 0) & (obj >= 0)
    print("eye on a surface: %d of %d pixels hit, %d answers of the ray API within EPSILON of the eye" % (int((ident > 0).sum()), ident.size, int(zeroed.sum())))
    assert (v_dist(hit[zeroed].T, rays[zeroed, :d].T) <= EPSILON).all()
    assert np.array_equal(ident[~zeroed] - 1, obj[~zeroed]) and same_bits(pos[~zeroed], hit[~zeroed]) and same_bits(nor[~zeroed], nrm[~zeroed])
    assert not pos[ident == 0].any() and not nor[ident == 0].any()
    assert np.array_equal(dm == 0, f["id"] == 0)
    shown = f["id"] > 0
    assert same_bits(dm[shown], 1.0 / v_dist(f["position"][:, shown], f["ray_o"][:, shown]))
    assert (v_dist(f["position"][:, shown], f["ray_o"][:, shown]) > EPSILON).all()


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [0, 1, 2], ids=["auto", "levels", "stream"])
def test_a_feature_pass_changes_no_image_no_map_and_no_later_file(gpu, pipeline):
    g = golden("c3_random4d")
    w, h = 33, 17
    try:
        gpu.set_option("pipeline", pipeline)
        gpu.upload_scene(g.scene)
        fb, dm, _ = gpu.render(w, h, g.depth, depth_map=True)
        before, _ = gpu.render_exr(w, h, g.depth, pixel="float", depth_map=True)
        f = gpu.render_features(w, h, g.depth)
        fb2, dm2, _ = gpu.render(w, h, g.depth, depth_map=True)
        assert same_bits(fb2, fb) and same_bits(dm2, dm)
        with_features, _ = gpu.render_exr(w, h, g.depth, pixel="float", depth_map=True, features=ALL)
        sizes, _ = assert_file_is(with_features, model_channels(fb, dm, f, 7, FLOAT))
        plain = read_exr(before)[1]
        got = read_exr(with_features)[1]
        assert all(same_bits(got[n], plain[n]) for n in "ABGRZ")
        after, _ = gpu.render_exr(w, h, g.depth, pixel="float", depth_map=True)
        assert after == before
        fb3, dm3, _ = gpu.render(w, h, g.depth, depth_map=True)
        assert same_bits(fb3, fb) and same_bits(dm3, dm)
    finally:
        gpu.set_option("pipeline", 0)


FILE_SCENES = {"3d": "zoo3d_mirror", "4d": "zoo4d", "12d": "zoo12d"}


@pytest.mark.gpu
@pytest.mark.parametrize("pixel", ["half", "float"])
@pytest.mark.parametrize("dims", sorted(FILE_SCENES))
def test_the_file_carries_the_planes_beside_the_plain_files_channels(gpu, dims, pixel):
    """widths 1, 33, 257 by rows 1, 17, 33, everything with Z: the reader accepts the file, the channel list is the sorted list,
    A B G R Z hold the plain file's bits, P.* and N.* are float32 of the planes, id is the plane as uint32"""
    g = golden(FILE_SCENES[dims])
    d = g.scene.dims
    gpu.upload_scene(g.scene)
    for w in (1, 33, 257):
        for h in (1, 17, 33):
            f = gpu.render_features(w, h, g.depth)
            fb, dm, _ = gpu.render(w, h, g.depth, depth_map=True)
            data, _ = gpu.render_exr(w, h, g.depth, pixel=pixel, depth_map=True, features=ALL)
            st = gpu.exr_stats
            want = model_channels(fb, dm, f, 7, PIXEL[pixel])
            assert [n for n, _, _ in want] == [n for n, _ in channel_names(d, 7, True)] and len(want) == 6 + 2 * d
            sizes, raw_flags = assert_file_is(data, want)
            assert st.file_bytes == len(data) <= nh.exr_features_bound(w, h, d, ALL, pixel, True)
            assert st.blocks == len(sizes) == (h + 15) // 16 and st.blocks_raw == sum(raw_flags) and st.launches == 4
            assert st.raw_bytes == w * h * (4 * DTYPE[PIXEL[pixel]].itemsize + 4 + 4 + 8 * d)
            plain = read_exr(gpu.render_exr(w, h, g.depth, pixel=pixel, depth_map=True)[0])[1]
            got = read_exr(data)[1]
            assert all(same_bits(got[n], plain[n]) for n in "ABGRZ")
            assert same_bits(got["id"], f["id"].view(np.uint32)) and same_bits(got["P.%02d" % (d - 1)], f["position"][d - 1].astype(np.float32))
    # any subset writes only its groups (and without Z there is none)
    w, h = 33, 17
    f = gpu.render_features(w, h, g.depth)
    fb, dm, _ = gpu.render(w, h, g.depth, depth_map=True)
    for mask in range(1, 7):
        for with_z in (False, True):
            data, _ = gpu.render_exr(w, h, g.depth, pixel=pixel, depth_map=with_z, features=names_of(mask))
            assert_file_is(data, model_channels(fb, dm if with_z else None, f, mask, PIXEL[pixel]))
            assert len(data) <= nh.exr_features_bound(w, h, d, names_of(mask), pixel, with_z)


@pytest.mark.gpu
def test_noise_planes_fall_back_to_raw_blocks_and_a_flat_region_of_misses_compresses(gpu):
    """caller-supplied planes through ndt_hip_encode_exr_features_device: 16 rows of white noise in every channel, then 32 rows of
    misses (id 0, zeros) on a flat colour: block 0 holds its raw bytes, blocks 1 and 2 streams"""
    import torch
    w, h, d = 64, 48, 4
    rng = np.random.default_rng(99)
    fb = np.full((h, w, 4), 0.25)
    fb[:16] = noise_doubles((16, w, 4), 1)
    dm = np.zeros((h, w))
    dm[:16] = noise_doubles((16, w), 2)
    planes = {"id": np.zeros((h, w), dtype=np.int32), "position": np.zeros((d, h, w)), "normal": np.zeros((d, h, w))}
    planes["id"][:16] = rng.integers(-2 ** 31, 2 ** 31, (16, w)).astype(np.int32)
    planes["position"][:, :16] = noise_doubles((d, 16, w), 3)
    planes["normal"][:, :16] = noise_doubles((d, 16, w), 4)
    dev = {k: torch.from_numpy(v).cuda() for k, v in planes.items()}
    d_fb, d_dm = torch.from_numpy(fb).cuda(), torch.from_numpy(dm).cuda()
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in dev.items()}
    for pixel in ("float", "half"):
        data = gpu.encode_exr_features_device(d_fb.data_ptr(), d_dm.data_ptr(), ptrs, d, ALL, w, h, pixel)
        st = gpu.exr_stats
        sizes, raw_flags = assert_file_is(data, model_channels(fb, dm, planes, 7, PIXEL[pixel]))
        line = w * (4 * DTYPE[PIXEL[pixel]].itemsize + 4 + 4 + 8 * d)
        print("%s: blocks %s of %d raw bytes each, raw %s" % (pixel, sizes, 16 * line, raw_flags))
        if pixel == "float":        # (half noise clamps and rounds: only the float file is noise in every byte)
            assert raw_flags == [True, False, False] and sizes[0] == 16 * line and st.blocks_raw == 1
        assert not raw_flags[1] and not raw_flags[2] and max(sizes[1:]) < 0.02 * 16 * line and st.launches == 4
    # a subset from the same planes, no map; the planes of the mask must be there
    data = gpu.encode_exr_features_device(d_fb.data_ptr(), None, ptrs, d, ("id", "normal"), w, h, "float")
    assert_file_is(data, model_channels(fb, None, planes, ID | NORMAL, FLOAT))
    with pytest.raises(nh.NdtHipError, match="NULL"):
        gpu.encode_exr_features_device(d_fb.data_ptr(), None, {"id": ptrs["id"]}, d, ALL, w, h, "float")
    with pytest.raises(nh.NdtHipError, match="dimensions"):
        gpu.encode_exr_features_device(d_fb.data_ptr(), None, ptrs, 13, 7, w, h, "float", cap=1 << 20)


@pytest.mark.gpu
def test_ssaa_file_has_the_folded_colour_and_the_plain_frames_features(gpu):
    g = golden("c3_random4d")
    w, h = 34, 18
    gpu.upload_scene(g.scene)
    fb, dm, _ = gpu.render_ssaa(w, h, g.depth, 2, depth_map=True)
    f = gpu.render_features(w, h, g.depth)
    plain_fb, plain_dm, _ = gpu.render(w, h, g.depth, depth_map=True)
    assert same_bits(dm, plain_dm) and not same_bits(fb, plain_fb)
    for pixel in ("float", "half"):
        data, _ = gpu.render_ssaa_exr(w, h, g.depth, 2, pixel=pixel, depth_map=True, features=ALL)
        assert_file_is(data, model_channels(fb, dm, f, 7, PIXEL[pixel]))
        assert gpu.ssaa_launches() == 2 and gpu.features_launches() == 4


@pytest.mark.gpu
def test_frames_without_one_primary_ray_are_refused_and_a_short_buffer_is_left_alone(gpu):
    lib = gpu.lib
    g = golden("st_zoo4d_sbs")
    gpu.upload_scene(g.scene)
    w, h = 34, 18
    ep = nh.ExrParams(HALF)
    cap = nh.exr_features_bound(w, h, g.scene.dims, ALL, "half", True)
    for kw, word in (({"aa": (20, 3)}, "recursive_aa"), ({"samples": 2}, "samples = 2"), ({"stereo": 3}, "anaglyph"), ({"stereo": 4}, "HIDEF")):
        p = gpu.params(w, h, g.depth, **kw)
        buf = np.full(cap, 0xA5, dtype=np.uint8)
        st = nh.ExrStats()
        assert lib.ndt_hip_render_exr_features(gpu.ctx, C.byref(p), C.byref(ep), 1, 7, buf.ctypes.data, cap, C.byref(st), None) == NDT_E_UNSUPPORTED, kw
        assert word in lib.ndt_hip_last_error().decode() and b"ndt_hip_render_exr_features" in lib.ndt_hip_last_error()
        assert (buf == 0xA5).all() and st.file_bytes == 0
        assert lib.ndt_hip_render_ssaa_exr_features(gpu.ctx, C.byref(p), 2, C.byref(ep), 1, 7, buf.ctypes.data, cap, None, None) == NDT_E_UNSUPPORTED
        assert word in lib.ndt_hip_last_error().decode() and (buf == 0xA5).all()
        with pytest.raises(nh.NdtHipError, match=word) as e:
            gpu.render_features(w, h, g.depth, **kw)
        assert e.value.code == NDT_E_UNSUPPORTED
    p = gpu.params(w, h, g.depth)
    buf = np.full(cap, 0xA5, dtype=np.uint8)
    for mask in (0, 8):
        assert lib.ndt_hip_render_exr_features(gpu.ctx, C.byref(p), C.byref(ep), 1, mask, buf.ctypes.data, cap, None, None) == NDT_E_INVALID
        assert b"feature mask" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_render_features(gpu.ctx, C.byref(p), C.byref(nh.FeaturePlanes()), None) == NDT_E_INVALID
    assert (buf == 0xA5).all()
    # room one byte short: NDT_E_NOMEM with the size needed, and nothing written -- least of all behind `cap`
    for pixel in ("half", "float"):
        data, _ = gpu.render_exr(w, h, g.depth, pixel=pixel, depth_map=True, features=ALL)
        short = len(data) - 1
        buf = np.full(short + 64, 0xA5, dtype=np.uint8)
        st = nh.ExrStats()
        ep = nh.ExrParams(PIXEL[pixel])
        rc = lib.ndt_hip_render_exr_features(gpu.ctx, C.byref(p), C.byref(ep), 1, 7, buf.ctypes.data, short, C.byref(st), None)
        assert rc == NDT_E_NOMEM
        assert str(len(data)) in lib.ndt_hip_last_error().decode() and st.file_bytes == len(data)
        assert (buf == 0xA5).all()


# ---------------------------------------------------------------- driver

@pytest.mark.gpu
def test_driver_writes_the_feature_channels_and_says_so(tmp_path):
    """one `--exr --exr-aov all -z` frame of the YAML zoo (5-D): one .exr, the printed line, the library's file for the same request,
    and the colour channels of the run without `--exr-aov`"""
    y = str(tmp_path / "zoo5d.yaml")
    with gzip.open(os.path.join(GOLDEN, "yaml", "y_zoo5d.yaml.gz"), "rb") as src, open(y, "wb") as dst:
        dst.write(src.read())
    common = dict(scene="builtin:yaml", dims=5, size="48x27")
    r = _run_driver(tmp_path / "aov", "-u", y, "--exr", "--exr-aov", "normal,id,position,id", "-z", **common)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    found = [p for p in (tmp_path / "aov").rglob("*") if p.is_file()]
    assert len(found) == 1 and found[0].suffix == ".exr"
    data = found[0].read_bytes()
    assert "encoded EXR of %d bytes on GPU 0 in 4 launches" % len(data) in r.stdout
    assert "added 11 feature channels on GPU 0 in 4 launches" in r.stdout
    chans, got, _, _ = read_exr(data)
    assert chans == [(n, HALF if t is None else t) for n, t in channel_names(5, 7, True)]
    r = _run_driver(tmp_path / "plain", "-u", y, "--exr", "-z", **common)
    assert r.returncode == 0 and "feature channels" not in r.stdout
    plain = read_exr(next((tmp_path / "plain").rglob("*.exr")).read_bytes())[1]
    assert sorted(plain) == ["A", "B", "G", "R", "Z"] and all(same_bits(got[n], plain[n]) for n in plain)
    # the library's file for the same request, from the scene the driver loads
    dump = str(tmp_path / "zoo5d.ndtscene")
    r = _run_driver(tmp_path, "-u", y, "--dump-scene", dump, **common)
    assert r.returncode == 0, r.stderr[-2000:]
    gpu = nh.NdtHip(0)
    try:
        gpu.upload_scene(load_scene(dump))
        want, _ = gpu.render_exr(48, 27, 6, pixel="half", depth_map=True, features=ALL)
    finally:
        gpu.close()
    assert data == want
    assert (got["id"] > 0).any() and (got["id"] == 0).any()
