"""Measurements of the 16-bit PNG path; its output is committed in profiles/png16_on_device.txt.

Encode time of the 1920x1080 benchmark frame (tests/golden/c3_random4d_1080p) at 8 and at 16 bits on one context, alternating,
as medians with their spread; the files' IDAT sizes against zlib level 6 and against the Z_RLE 32 KiB-slice model over the same
filtered stream; the bytes that cross PCIe for frame + map against `--raw -z`.  Self-contained: the yardsticks are restated here.
NDT_HIP_LIB selects the library; one without the 16-bit entry points (the parent's) gets the 8-bit figures alone.
Usage: python profiles/png16_probe.py [runs]"""
import json
import os
import statistics
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ndt_amd import hip as nh, load_scene      # noqa: E402

CHUNK = 32768
FIXTURE = "c3_random4d_1080p"


def clamp01(x):
    m = np.where(1.0 < x, 1.0, x)
    return np.where(0.0 > m, 0.0, m)


def q16(x):
    return (np.sqrt(clamp01(x)) * 65535).astype(np.uint16)


def inflate(png, bpp):
    """(pixel bytes [h, w, bpp], IDAT length) of a one-IDAT PNG with filters 0 / 1 / 2"""
    w, h = struct.unpack(">II", png[16:24])
    n, = struct.unpack(">I", png[33:37])
    assert png[37:41] == b"IDAT" and zlib.crc32(png[37:41 + n]) == struct.unpack(">I", png[41 + n:45 + n])[0]
    raw = np.frombuffer(zlib.decompress(png[41:41 + n]), dtype=np.uint8).reshape(h, 1 + bpp * w)
    out = np.zeros((h, w, bpp), dtype=np.uint8)
    for r in range(h):
        row = raw[r, 1:].reshape(w, bpp)
        out[r] = np.cumsum(row, axis=0, dtype=np.uint8) if raw[r, 0] == 1 else row + out[r - 1] if raw[r, 0] == 2 and r else row
    return out, n


def model_sizes(pixel_bytes):
    """zlib level 6, and Z_RLE / raw deflate / 32 KiB slices with a sync flush each + 6 bytes, over the heuristic's filtered stream"""
    h, w, bpp = pixel_bytes.shape
    raw = pixel_bytes.reshape(h, w * bpp)
    left = np.zeros_like(raw)
    left[:, bpp:] = raw[:, :-bpp]
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    cands = np.stack([raw, raw - left, raw - up])
    filters = np.argmin(np.abs(cands.view(np.int8).astype(np.int64)).sum(axis=2), axis=0)
    stream = np.empty((h, 1 + w * bpp), dtype=np.uint8)
    stream[:, 0] = filters
    stream[:, 1:] = cands[filters, np.arange(h)]
    filtered = stream.tobytes()
    b = 6
    for k in range(0, len(filtered), CHUNK):
        c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
        b += len(c.compress(filtered[k:k + CHUNK]) + c.flush(zlib.Z_SYNC_FLUSH))
    return len(zlib.compress(filtered, 6)), b


def spread(v):
    return "median %.3f [min %.3f .. max %.3f]" % (statistics.median(v), min(v), max(v))


def say_size(what, png, bpp, st):
    pix, n = inflate(png, bpp)
    a, b = model_sizes(pix)
    print("size %s: file %d bytes, IDAT %d; zlib-6 %d (x%.3f); slice model %d (x%.3f); %d of %d chunks stored; rows by filter %s" % (
        what, len(png), n, a, n / a, b, n / b, st.chunks_stored, st.chunks, list(st.rows_filter)))
    return pix


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 31
    with open(os.path.join(ROOT, "tests", "golden", FIXTURE + ".json")) as f:
        meta = json.load(f)
    w, h, depth = meta["width"], meta["height"], meta["depth"]
    gpu = nh.NdtHip(0)
    gpu.upload_scene(load_scene(os.path.join(ROOT, "tests", "golden", meta["scene_file"])))
    have16 = hasattr(gpu.lib, "ndt_hip_render_png16")
    print("library %s (%s the 16-bit entry points), %s %dx%d -l %d, %d alternating runs after 3 warm-up rounds; encode_ms = launch "
          "of the filter to the file in host memory" % (os.path.basename(nh.LIB_PATH), "with" if have16 else "without", FIXTURE, w, h,
                                                        depth, runs))
    t8, t16, td = [], [], []
    for k in range(runs + 3):
        png8, _ = gpu.render_png(w, h, depth)
        st8, ms8 = gpu.png_stats, gpu.png_stats.encode_ms
        if have16:
            png16, _ = gpu.render_png16(w, h, depth)
            st16, ms16 = gpu.png_stats, gpu.png_stats.encode_ms
            _, dpng, rng, _ = gpu.render_png16_depth(w, h, depth)
            std, msd = gpu.png_stats[1], gpu.png_stats[1].encode_ms
        if k >= 3:
            t8.append(ms8)
            if have16:
                t16.append(ms16)
                td.append(msd)
    print("encode_ms  8-bit RGBA: %s" % spread(t8))
    say_size(" 8-bit RGBA", png8, 4, st8)
    if not have16:
        return
    print("encode_ms 16-bit RGBA: %s; ratio of the medians 16 / 8: %.3f" % (spread(t16), statistics.median(t16) / statistics.median(t8)))
    print("encode_ms 16-bit grey map: %s" % spread(td))
    pix16 = say_size("16-bit RGBA", png16, 8, st16)
    grey = say_size("16-bit grey map", dpng, 2, std)
    fb, dm, _ = gpu.render(w, h, depth, depth_map=True)
    assert np.array_equal(np.ascontiguousarray(pix16).view(">u2").astype(np.uint16), q16(fb))
    lo, hi = dm.min(), dm.max()
    got = np.ascontiguousarray(grey).view(">u2").astype(np.uint16)[:, :, 0]
    assert np.array_equal(got, q16((dm - lo) / (hi - lo)))
    print("the map: %d distinct grey values (an 8-bit map: at most 256), range [%r, %r]" % (np.unique(got).size, float(rng[0]), float(rng[1])))
    raw, two = w * h * 40, len(png16) + len(dpng)
    print("PCIe, frame + map: --raw -z %d bytes (40 a pixel); the two 16-bit files %d bytes (%.3f a pixel, 1/%.0f of it); the two "
          "8-bit images of --depth gpu %d bytes (8 a pixel)" % (raw, two, two / (w * h), raw / two, w * h * 8))
    png2, _ = gpu.render_ssaa_png16(w, h, depth, 2)
    s2 = np.ascontiguousarray(inflate(png2, 8)[0]).view(">u2").astype(np.uint16)
    print("--ssaa 2: 16-bit file %d bytes, encode_ms %.3f (one run); distinct values a channel %s, floored to 8 bits %s" % (
        len(png2), gpu.png_stats.encode_ms, [int(np.unique(s2[..., c]).size) for c in range(4)],
        [int(np.unique(s2[..., c] // 257).size) for c in range(4)]))
    gpu.close()


if __name__ == "__main__":
    main()
