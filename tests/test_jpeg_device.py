"""The frame's JPEG file made on the device (ndt_jpeg.hip; `ndt_hip --jpeg`).

The yardsticks are Pillow's libjpeg and `model_jpeg` below -- never the device's own output:
  * `model_jpeg` restates the encoder in numpy integer arrays (colour transform, 4:2:0 averaging, libjpeg's slow integer DCT,
    quantisation) and a plain Python Huffman writer (Annex K tables, byte stuffing, one restart interval per MCU row, headers);
  * the CPU tests hold the model against Pillow's own file of the same image (same quality and sampling, `optimize=False`,
    `restart_marker_rows=1`): measured on the cases of `CASES` below, every one of the 30 model files is byte-identical to
    Pillow's, so the test asserts identity (margins m = 0 dB and s = 0);
  * the GPU tests hold the device's file against the model's, byte for byte.

Edges follow libjpeg to the letter, which is what makes the files identical: a component's blocks are filled by repeating the
last column of the source and the last row of the (down-sampled) component, and a luminance block that lies wholly outside the
image (4:2:0, odd number of 8-pixel columns or rows) is a dummy: no AC, the DC of the block before it in the MCU.
"""
import ctypes as C
import io
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, golden, FULL_CASES

from ndt_amd import hip as nh

NDT_E_INVALID, NDT_E_NOMEM = -1, -4
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "scenes")
DRIVER = os.path.join(ROOT, "ndt_amd", "host", "ndt_hip")
ENTRY_POINTS = ("ndt_hip_jpeg_bound", "ndt_hip_encode_jpeg_device", "ndt_hip_encode_jpeg", "ndt_hip_render_jpeg")
HEAD_BYTES = 629            # SOI .. SOS


# ---------------------------------------------------------------- the model

LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMA_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
     0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
     0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
     0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
     0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
     0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def _zigzag():
    """natural index of every zigzag position: the anti-diagonals of the 8 x 8 block, direction alternating"""
    order = []
    for s in range(15):
        diag = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        order += diag if s % 2 else diag[::-1]
    return np.array([8 * y + x for y, x in order])


ZIGZAG = _zigzag()


def quant_table(base, quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array(base, dtype=np.int64) * scale + 50) // 100, 1, 255)


def _huff_codes(bits, vals):
    """{symbol: (code, length)} of a DHT's counts and symbols (Annex C)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(x, first):
    """libjpeg's slow integer DCT along the last axis: CONST_BITS 13, PASS1_BITS 2"""
    x = [x[..., k] for k in range(8)]
    t0, t7, t1, t6 = x[0] + x[7], x[0] - x[7], x[1] + x[6], x[1] - x[6]
    t2, t5, t3, t4 = x[2] + x[5], x[2] - x[5], x[3] + x[4], x[3] - x[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, n)
    o[5] = _descale(t5 + z2 + z4, n)
    o[3] = _descale(t6 + z2 + z3, n)
    o[1] = _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def _edge(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def _blocks(plane, table):
    """quantised coefficients [block row, block column, 64 in zigzag order] of a plane whose sides are multiples of 8"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    b = (plane - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    b = _fdct_pass(b, True)                                             # rows
    b = _fdct_pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # columns
    qv = (table << 3).reshape(8, 8)
    q = np.where(b >= 0, (b + (qv >> 1)) // qv, -((-b + (qv >> 1)) // qv))
    return q.reshape(bh, bw, 64)[:, :, ZIGZAG]


def model_coefficients(rgb, quality, sampling):
    """(per MCU row a list of MCUs, each a list of (component, 64 coefficients in zigzag order)), the two tables, MCU side"""
    rgb = np.asarray(rgb)[..., :3].astype(np.int64)
    h, w, _ = rgb.shape
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    side = 16 if sampling == "420" else 8
    mw, mh = -(-w // side), -(-h // side)
    tables = (quant_table(LUMA_Q, quality), quant_table(CHROMA_Q, quality))
    if sampling == "420":
        def down(c):
            c = _edge(c, h + (h & 1), 16 * mw)          # the source: rows to an even count, columns to the MCU
            s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
            s = (s + 1 + (np.arange(s.shape[1]) & 1)) >> 2
            return _edge(s, 8 * mh, 8 * mw)             # the component: its last row repeated
        cb, cr = down(cb), down(cr)
    else:
        cb, cr = _edge(cb, 8 * mh, 8 * mw), _edge(cr, 8 * mh, 8 * mw)
    yq = _blocks(_edge(y, side * mh, side * mw), tables[0])
    cbq, crq = _blocks(cb, tables[1]), _blocks(cr, tables[1])
    real_w, real_h = -(-w // 8), -(-h // 8)           # luminance blocks that hold image
    rows = []
    for my in range(mh):
        row = []
        for mx in range(mw):
            mcu = []
            if sampling == "420":
                for k in range(4):
                    by, bx = 2 * my + (k >> 1), 2 * mx + (k & 1)
                    c = yq[by, bx]
                    if by >= real_h or bx >= real_w:    # a dummy block: the DC of the block before it, no AC
                        c = np.zeros(64, dtype=np.int64)
                        c[0] = mcu[-1][1][0]
                    mcu.append((0, c))
            else:
                mcu.append((0, yq[my, mx]))
            mcu.append((1, cbq[my, mx]))
            mcu.append((2, crq[my, mx]))
            row.append(mcu)
        rows.append(row)
    return rows, tables, side


def _segment(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def model_jpeg(rgb, quality=95, sampling="420", info=None):
    """The baseline JFIF file of an (h, w, 3+) uint8 image.  info (a dict) receives stuffed / zrl / intervals / mcus / scan_bytes."""
    h, w = np.asarray(rgb).shape[:2]
    rows, tables, side = model_coefficients(rgb, quality, sampling)
    dc = [_huff_codes(DC_BITS[t], DC_VALS[t]) for t in range(2)]
    ac = [_huff_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]
    out = bytearray(b"\xff\xd8")
    out += _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += _segment(0xDB, bytes([t]) + bytes(int(v) for v in tables[t][ZIGZAG]))
    hv = 0x22 if sampling == "420" else 0x11
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for t in range(2):
        out += _segment(0xC4, bytes([0x00 | t]) + bytes(DC_BITS[t]) + bytes(DC_VALS[t]))
        out += _segment(0xC4, bytes([0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t]))
    out += _segment(0xDD, len(rows[0]).to_bytes(2, "big"))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == HEAD_BYTES
    stuffed = zrl = 0
    for k, row in enumerate(rows):
        acc = nbits = 0
        raw = bytearray()
        pred = [0, 0, 0]

        def put(code, length):
            nonlocal acc, nbits
            acc = (acc << length) | code
            nbits += length
            while nbits >= 8:
                nbits -= 8
                raw.append((acc >> nbits) & 255)
            acc &= (1 << nbits) - 1

        for mcu in row:
            for comp, c in mcu:
                t = 0 if comp == 0 else 1
                diff = int(c[0]) - pred[comp]
                pred[comp] = int(c[0])
                size = abs(diff).bit_length()
                put(*dc[t][size])
                if size:
                    put((diff if diff >= 0 else diff - 1) & ((1 << size) - 1), size)
                run_from = 0
                for z in np.flatnonzero(c[1:]) + 1:
                    run = int(z) - run_from - 1
                    while run > 15:
                        put(*ac[t][0xF0])
                        zrl += 1
                        run -= 16
                    v = int(c[z])
                    size = abs(v).bit_length()
                    put(*ac[t][(run << 4) | size])
                    put((v if v >= 0 else v - 1) & ((1 << size) - 1), size)
                    run_from = int(z)
                if run_from < 63:
                    put(*ac[t][0x00])
        if nbits:
            put((1 << (8 - nbits)) - 1, 8 - nbits)
        stuffed += raw.count(0xFF)
        out += bytes(raw).replace(b"\xff", b"\xff\x00")
        if k + 1 < len(rows):
            out += bytes([0xFF, 0xD0 + (k & 7)])
    out += b"\xff\xd9"
    if info is not None:
        info.update(stuffed=stuffed, zrl=zrl, intervals=len(rows), mcus=len(rows) * len(rows[0]), scan_bytes=len(out) - HEAD_BYTES - 2)
    return bytes(out)


def rst_markers(data):
    """the m of every RSTm in the scan, in order (a 0xFF in the scan's data is followed by 0x00, so FF D0 .. D7 is a marker)"""
    return [data[k + 1] - 0xD0 for k in range(HEAD_BYTES, len(data) - 1) if data[k] == 0xFF and 0xD0 <= data[k + 1] <= 0xD7]


# ---------------------------------------------------------------- images

def synthetic(kind, w, h):
    """(h, w, 4) uint8; the alpha channel is filled, and ignored by the encoder"""
    rng = np.random.default_rng(1000 * w + h)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    if kind == "zero":
        return np.zeros((h, w, 4), dtype=np.uint8)
    if kind == "gradient":
        return np.stack([x * 3, y * 5, x + y, (x * 3 + y * 5) // 7], axis=2).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if kind == "noise_row":
        img = np.full((h, w, 4), 77, dtype=np.uint8)
        img[h // 2] = rng.integers(0, 256, (w, 4), dtype=np.uint8)
        return img
    if kind == "sparse":
        # grey 100 with a checkerboard of +2: of its DCT only the coefficient at (7, 7), the last in zigzag order, survives
        # the quantiser at quality 95 -- 62 zeros before it, three ZRL symbols a luminance block
        v = (100 + 2 * ((x + y) & 1)).astype(np.uint8)
        return np.stack([v, v, v, np.full_like(v, 255)], axis=2)
    raise ValueError(kind)


_ff_cache = {}


def ff_image(w, h, sampling):
    """Flat cells of 16 x 16 pixels in random colours: large DC differences, whose all-ones extra bits put 0xFF bytes into the
    scan.  The first seed for which the model's scan holds one (found by the model, on the CPU)."""
    key = (w, h, sampling)
    if key not in _ff_cache:
        for seed in range(4096):
            rng = np.random.default_rng(seed)
            cells = rng.integers(0, 256, (-(-h // 16), -(-w // 16), 4), dtype=np.uint8)
            img = np.ascontiguousarray(np.repeat(np.repeat(cells, 16, axis=0), 16, axis=1)[:h, :w])
            info = {}
            model_jpeg(img, 95, sampling, info)
            if info["stuffed"] > 0:
                _ff_cache[key] = img
                break
        else:
            raise AssertionError("no seed puts a 0xFF byte into the scan of a %d x %d image" % (w, h))
    return _ff_cache[key]


def make_image(kind, w, h, sampling):
    return ff_image(w, h, sampling) if kind == "ff" else synthetic(kind, w, h)


_model_cache = {}


def model_of(kind, w, h, quality, sampling):
    key = (kind, w, h, quality, sampling)
    if key not in _model_cache:
        info = {}
        _model_cache[key] = (model_jpeg(make_image(kind, w, h, sampling), quality, sampling, info), info)
    return _model_cache[key]


def crops():
    """256 x 256 pieces of three golden frames, a gradient and noise: (name, (256, 256, 3) uint8)"""
    out = []
    for name, (y0, x0) in (("c1_hypercube3d_256", (0, 0)), ("c3_random4d_1080p", (412, 832)), ("c5_hypercube6d_1080p", (412, 832))):
        out.append((name, np.ascontiguousarray(golden(name).data["rgba8"][y0:y0 + 256, x0:x0 + 256, :3])))
    out.append(("gradient", synthetic("gradient", 256, 256)[..., :3]))
    out.append(("noise", synthetic("noise", 256, 256)[..., :3]))
    return out


CASES = [(s, q) for s in ("420", "444") for q in (50, 95, 100)]


def pillow_jpeg(rgb, quality, sampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb[..., :3])).save(buf, "JPEG", quality=quality, subsampling=2 if sampling == "420" else 0,
                                                             optimize=False, restart_marker_rows=1)
    return buf.getvalue()


def psnr(a, b):
    mse = float(((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean())
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


# ---------------------------------------------------------------- CPU

def test_library_exports_the_jpeg_entry_points():
    lib = nh.load_library()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in nh.API_SYMBOLS
    assert lib.ndt_hip_abi_version() == 3


SMALL_SHAPES = [(1, 1), (16, 16), (17, 16), (16, 17), (37, 19), (8, 8), (9, 9), (16, 144)]


def test_jpeg_bound_covers_noise_and_refuses_bad_sizes():
    lib = nh.load_library()
    for w, h in SMALL_SHAPES:
        for sampling in ("420", "444"):
            jp = nh.JpegParams(100, 0 if sampling == "420" else 1)
            n = len(model_of("noise", w, h, 100, sampling)[0])
            bound = lib.ndt_hip_jpeg_bound(w, h, C.byref(jp))
            assert bound >= n, (w, h, sampling, bound, n)
            assert nh.jpeg_bound(w, h, 100, sampling) == bound
    assert lib.ndt_hip_jpeg_bound(1920, 1080, None) == nh.jpeg_bound(1920, 1080) > 0       # jp == NULL: the defaults
    assert lib.ndt_hip_jpeg_bound(65535, 65535, None) > 0
    for w, h in ((0, 1), (1, 0), (0, 0), (-1, 5), (5, -1), (65536, 1), (1, 65536), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.ndt_hip_jpeg_bound(w, h, None) < 0, (w, h)
    for quality, sampling, reserved in ((-1, 0, 0), (101, 0, 0), (95, 2, 0), (95, -1, 0), (95, 0, 1)):
        jp = nh.JpegParams(quality, sampling)
        jp.reserved[1] = reserved
        assert lib.ndt_hip_jpeg_bound(16, 16, C.byref(jp)) < 0, (quality, sampling, reserved)
    for bad in ((0, 4, 95, "420"), (4, 70000, 95, "420"), (4, 4, 0, "420"), (4, 4, 101, "420"), (4, 4, 95, "422")):
        with pytest.raises(ValueError):
            nh.jpeg_bound(*bad)


def test_the_sparse_image_takes_the_zrl_path():
    for sampling in ("420", "444"):
        _, info = model_of("sparse", 37, 19, 95, sampling)
        assert info["zrl"] >= 3 * (37 // 8) * (19 // 8)       # three ZRL a luminance block that lies wholly inside the image


def test_the_ff_image_has_stuffed_bytes():
    for w, h in SMALL_SHAPES:
        for sampling in ("420", "444"):
            data, info = model_of("ff", w, h, 95, sampling)
            assert info["stuffed"] > 0 and data.count(b"\xff\x00") >= info["stuffed"]


@pytest.mark.parametrize("sampling,quality", CASES)
def test_model_files_load_in_pillow(sampling, quality):
    pytest.importorskip("PIL")
    from PIL import Image
    for name, rgb in crops():
        data = model_jpeg(rgb, quality, sampling)
        im = Image.open(io.BytesIO(data))
        im.load()
        ref = Image.open(io.BytesIO(pillow_jpeg(rgb, quality, sampling)))
        assert im.size == (256, 256) and im.mode == "RGB", name
        hv = (2, 2) if sampling == "420" else (1, 1)
        assert [tuple(c[1:3]) for c in im.layer] == [hv, (1, 1), (1, 1)], name
        assert {k: list(v) for k, v in im.quantization.items()} == {k: list(v) for k, v in ref.quantization.items()}, name
        side = 16 if sampling == "420" else 8
        n = 256 // side - 1
        assert rst_markers(data) == [k % 8 for k in range(n)], name


def test_model_files_are_pillows_files():
    """Measured: all 30 cases byte-identical (margins m = 0 dB, s = 0), so identity is what is asserted.  Odd sizes as well: the
    edge rules are libjpeg's."""
    pytest.importorskip("PIL")
    same, total, worst_psnr, worst_size = 0, 0, 0.0, 0.0
    from PIL import Image
    for sampling, quality in CASES:
        for name, rgb in crops():
            mine, theirs = model_jpeg(rgb, quality, sampling), pillow_jpeg(rgb, quality, sampling)
            total += 1
            same += mine == theirs
            a = np.asarray(Image.open(io.BytesIO(mine)).convert("RGB"))
            b = np.asarray(Image.open(io.BytesIO(theirs)).convert("RGB"))
            worst_psnr = max(worst_psnr, psnr(b, rgb) - psnr(a, rgb))
            worst_size = max(worst_size, len(mine) / len(theirs) - 1)
    print("model against Pillow: %d of %d files byte-identical; worst PSNR shortfall %.3f dB, worst size excess %.4f" % (
        same, total, worst_psnr, worst_size))
    assert same == total
    for w, h in ((37, 19), (17, 16), (16, 17), (18, 18), (33, 50), (1, 1), (9, 9)):
        for sampling in ("420", "444"):
            for kind in ("noise", "gradient"):
                img = synthetic(kind, w, h)
                assert model_jpeg(img, 95, sampling) == pillow_jpeg(img, 95, sampling), (w, h, sampling, kind)


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


SHAPES = SMALL_SHAPES + [(4112, 16)]
KINDS = ["zero", "gradient", "noise", "noise_row", "ff", "sparse"]
GRID = [(s, k, smp, 95) for s in SHAPES for k in KINDS for smp in ("420", "444")]
GRID += [((37, 19), k, smp, q) for k in ("noise", "gradient") for smp in ("420", "444") for q in (1, 50, 100)]
GRID += [((4112, 16), "noise", smp, q) for smp in ("420", "444") for q in (1, 50, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind,sampling,quality", GRID, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_device_file_is_the_models_file(gpu, shape, kind, sampling, quality):
    w, h = shape
    img = make_image(kind, w, h, sampling)
    want, info = model_of(kind, w, h, quality, sampling)
    got = gpu.encode_jpeg(img, quality, sampling)
    st = gpu.jpeg_stats
    print("%dx%d %s %s q%d: %d bytes (model %d), %d intervals, %d stuffed, %d passes, %.3f ms" % (
        w, h, kind, sampling, quality, len(got), len(want), st.intervals, st.stuffed_bytes, st.passes_max, st.encode_ms))
    assert got == want
    assert st.jpeg_bytes == len(got) <= nh.jpeg_bound(w, h, quality, sampling)
    assert st.scan_bytes == info["scan_bytes"] and st.stuffed_bytes == info["stuffed"]
    assert st.intervals == info["intervals"] and st.mcus == info["mcus"] and st.launches >= 1 and st.passes_max >= 1
    if kind == "ff":
        assert st.stuffed_bytes > 0
    if shape == (4112, 16) and kind == "noise" and quality == 100:
        assert st.passes_max > 1
    assert gpu.encode_jpeg(img, quality, sampling) == got          # the same image, the same bytes
    # room one byte short: NDT_E_NOMEM with the size needed, and nothing written -- least of all behind `cap`
    cap = len(got) - 1
    buf = np.full(cap + 64, 0xA5, dtype=np.uint8)
    short = nh.JpegStats()
    jp = nh.JpegParams(quality, 0 if sampling == "420" else 1)
    rc = gpu.lib.ndt_hip_encode_jpeg(gpu.ctx, img.ctypes.data, w, h, C.byref(jp), buf.ctypes.data, cap, C.byref(short))
    assert rc == NDT_E_NOMEM
    assert str(len(got)) in gpu.lib.ndt_hip_last_error().decode()
    assert short.jpeg_bytes == len(got)
    assert (buf == 0xA5).all()


@pytest.mark.gpu
def test_bad_arguments_are_refused_by_name(gpu):
    img = synthetic("gradient", 20, 10)
    out = np.zeros(8192, dtype=np.uint8)
    lib = gpu.lib
    enc = lib.ndt_hip_encode_jpeg
    assert enc(gpu.ctx, None, 20, 10, None, out.ctypes.data, 8192, None) == NDT_E_INVALID
    assert enc(gpu.ctx, img.ctypes.data, 20, 10, None, None, 8192, None) == NDT_E_INVALID
    assert enc(None, img.ctypes.data, 20, 10, None, out.ctypes.data, 8192, None) == NDT_E_INVALID
    assert lib.ndt_hip_encode_jpeg_device(gpu.ctx, None, 20, 10, None, out.ctypes.data, 8192, None) == NDT_E_INVALID
    for w, h in ((0, 10), (20, 0), (-1, 10), (65536, 1), (1, 65536)):
        assert enc(gpu.ctx, img.ctypes.data, w, h, None, out.ctypes.data, 8192, None) == NDT_E_INVALID, (w, h)
        assert lib.ndt_hip_last_error()
    assert b"65535" in lib.ndt_hip_last_error()
    for quality, sampling, reserved, word in ((-1, 0, 0, b"quality"), (101, 0, 0, b"quality"), (95, 2, 0, b"sampling"), (95, -1, 0, b"sampling"),
                                              (95, 0, 7, b"reserved")):
        jp = nh.JpegParams(quality, sampling)
        jp.reserved[0] = reserved
        assert enc(gpu.ctx, img.ctypes.data, 20, 10, C.byref(jp), out.ctypes.data, 8192, None) == NDT_E_INVALID
        assert word in lib.ndt_hip_last_error()
    assert lib.ndt_hip_render_jpeg(gpu.ctx, None, None, out.ctypes.data, 8192, None, None) == NDT_E_INVALID
    # the encoder needs no scene, and the parameters and the stats are optional
    assert enc(gpu.ctx, img.ctypes.data, 20, 10, None, out.ctypes.data, 8192, None) == 0
    want = model_jpeg(img, 95, "420")
    assert out.tobytes()[:len(want)] == want
    zero = nh.JpegParams(0, 0)                 # quality 0: the default
    assert enc(gpu.ctx, img.ctypes.data, 20, 10, C.byref(zero), out.ctypes.data, 8192, None) == 0
    assert out.tobytes()[:len(want)] == want


@pytest.mark.gpu
def test_device_pointer_entry_is_the_host_pointer_entry(gpu):
    import torch
    img = synthetic("gradient", 333, 41)
    dev = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    for sampling in ("420", "444"):
        got = gpu.encode_jpeg_device(dev.data_ptr(), 333, 41, 95, sampling)
        assert got == gpu.encode_jpeg(img, 95, sampling) == model_jpeg(img, 95, sampling)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c1_hypercube3d_256", "c3_random4d_1080p"])
def test_golden_frames_are_the_models_file(gpu, name):
    assert name in FULL_CASES
    g = golden(name)
    ref = g.data["rgba8"]
    gpu.upload_scene(g.scene)
    got, _ = gpu.render_jpeg(g.width, g.height, g.depth)
    st = gpu.jpeg_stats
    line = "%s: %d bytes, %.3f ms in %d launches" % (name, len(got), st.encode_ms, st.launches)
    try:
        from PIL import Image
        line += ", PSNR %.2f dB" % psnr(np.asarray(Image.open(io.BytesIO(got)).convert("RGB")), ref[..., :3])
    except ImportError:
        pass
    print(line)
    assert got == model_jpeg(ref, 95, "420")


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [("c3_random4d", {"aa": (12, 2)}), ("st_zoo4d_sbs", {"stereo": 1}),
                                     ("c3_random4d", {"row_begin": 1, "row_step": 3})],
                         ids=["aa", "side_by_side", "row_shard"])
def test_render_jpeg_takes_every_mode_of_render_rgba8(gpu, name, kw):
    g = golden(name)
    gpu.upload_scene(g.scene)
    want, _ = gpu.render_rgba8(g.width, g.height, g.depth, **kw)
    got, _ = gpu.render_jpeg(g.width, g.height, g.depth, **kw)
    assert got == model_jpeg(want, 95, "420")
    assert gpu.render_jpeg(g.width, g.height, g.depth, quality=50, sampling="444", **kw)[0] == model_jpeg(want, 50, "444")


def read_stored_png(data):
    """the (h, w, 4) pixels of the driver's plain `--png` file: 8-bit RGBA, every row with filter 0"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, typ = int.from_bytes(data[pos:pos + 4], "big"), data[pos + 4:pos + 8]
        if typ == b"IHDR":
            w, h = int.from_bytes(data[pos + 8:pos + 12], "big"), int.from_bytes(data[pos + 12:pos + 16], "big")
        elif typ == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 4)


def _run_driver(cwd, *flags):
    g = golden("c3_random4d_1080p")
    cmd = [DRIVER, "-s", os.path.join(REF_BIN, "random.so"), "-d", "4", "-f", "0", "-r", "480x270", "-l", str(g.depth)] + list(flags)
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run(cmd, capture_output=True, text=True, cwd=str(cwd))


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built")
def test_driver_writes_the_jpeg(tmp_path):
    files = {}
    for tag, flags in (("png", ["--png"]), ("jpeg", ["--jpeg"]), ("q50", ["--jpeg", "--jpeg-quality", "50", "--jpeg-sampling", "444"]),
                       ("g3", ["--jpeg", "-g", "3"]), ("z", ["--jpeg", "-z"])):
        r = _run_driver(tmp_path / tag, *flags)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        found = list((tmp_path / tag / "images").rglob("*.png" if tag == "png" else "*.jpg"))
        assert len(found) == 1 and len(list((tmp_path / tag / "images").rglob("*.*"))) == 1
        files[tag] = found[0].read_bytes()
        if tag != "png":
            assert "encoded JPEG of %d bytes on GPU" % len(files[tag]) in r.stdout and " launches" in r.stdout
    pixels = read_stored_png(files["png"])
    assert files["jpeg"] == model_jpeg(pixels, 95, "420")
    assert files["q50"] == model_jpeg(pixels, 50, "444") and len(files["q50"]) < len(files["jpeg"])
    assert files["q50"][158:169] == b"\xff\xc0\x00\x11\x08\x01\x0e\x01\xe0\x03\x01" and files["q50"][169] == 0x11     # SOF0: luminance 1 x 1
    assert files["g3"] == files["jpeg"]             # -g 3: gathered on the host, encoded from there
    assert files["z"] == files["jpeg"]              # -z with the default --depth host: the colour image is the JPEG ...
    assert len(list((tmp_path / "z" / "depth").rglob("*.ppm"))) == 1        # ... and the map today's PPM
    refused = [(["--jpeg", "--png"], ("--jpeg", "--png")), (["--jpeg", "--raw", "x.f64"], ("--jpeg", "--raw")),
               (["--jpeg-quality", "50"], ("--jpeg-quality", "--jpeg")), (["--jpeg-sampling", "444"], ("--jpeg-sampling", "--jpeg")),
               (["--jpeg", "--jpeg-quality", "0"], ("--jpeg-quality",)), (["--jpeg", "--jpeg-quality", "101"], ("--jpeg-quality",)),
               (["--jpeg", "-z", "--depth", "gpu"], ("--jpeg", "--depth gpu"))]
    for k, (flags, words) in enumerate(refused):
        bad = _run_driver(tmp_path / ("bad%d" % k), *flags)
        assert bad.returncode != 0, flags
        for word in words:
            assert word in bad.stderr, (flags, bad.stderr)
        assert not [p for p in (tmp_path / ("bad%d" % k)).rglob("*") if p.is_file()], flags
