"""Measurements of the OpenEXR path; its output is committed in profiles/exr_on_device.txt.

The 1920x1080 benchmark frame (tests/golden/c3_random4d_1080p) rendered once into device memory, then, alternating, as medians with
their spread: the time from the frame in HBM to the half file, to the float file, and to the doubles in host memory (what `--raw`
moves: 32 bytes a pixel) -- each to pageable host memory, launch to last byte.  The files' sizes against zlib level 6 over the same
preprocessed blocks, restated here with numpy; every block of both files is inflated and compared with that model on the way.
NDT_HIP_LIB selects the library; one without the EXR entry points (the parent's) gets the doubles' figure alone.
Usage: python profiles/exr_probe.py [runs]"""
import json
import os
import statistics
import struct
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ndt_amd import hip as nh, load_scene      # noqa: E402

FIXTURE = "c3_random4d_1080p"
LINES = 16


def samples(x, pixel):
    if pixel == "half":
        return np.clip(x, -65504.0, 65504.0).astype("<f2")
    with np.errstate(over="ignore"):
        return x.astype("<f4")


def model_blocks(fb, pixel):
    """the preprocessed bytes of every block: per scanline A B G R, the even bytes then the odd ones, the delta predictor"""
    out = []
    for y0 in range(0, fb.shape[0], LINES):
        raw = b"".join(samples(fb[y, :, c], pixel).tobytes() for y in range(y0, min(y0 + LINES, fb.shape[0])) for c in (3, 2, 1, 0))
        r = np.frombuffer(raw, dtype=np.uint8)
        t = np.concatenate([r[0::2], r[1::2]])
        pre = t.copy()
        pre[1:] = t[1:] - t[:-1] + np.uint8(128)
        out.append(pre.tobytes())
    return out


def file_blocks(data, n_blocks):
    """[(dataSize, data)] of a file of this project's layout"""
    pos = 8
    while data[pos] != 0:
        pos = data.index(b"\0", data.index(b"\0", pos) + 1) + 1
        pos += 4 + struct.unpack("<i", data[pos:pos + 4])[0]
    offsets = struct.unpack("<%dQ" % n_blocks, data[pos + 1:pos + 1 + 8 * n_blocks])
    out = []
    for off in offsets:
        size, = struct.unpack("<i", data[off + 4:off + 8])
        out.append((size, data[off + 8:off + 8 + size]))
    return out


def spread(v):
    return "median %.3f [min %.3f .. max %.3f]" % (statistics.median(v), min(v), max(v))


def main():
    import torch
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 31
    with open(os.path.join(ROOT, "tests", "golden", FIXTURE + ".json")) as f:
        meta = json.load(f)
    w, h, depth = meta["width"], meta["height"], meta["depth"]
    gpu = nh.NdtHip(0)
    gpu.upload_scene(load_scene(os.path.join(ROOT, "tests", "golden", meta["scene_file"])))
    have = hasattr(gpu.lib, "ndt_hip_encode_exr_device")
    print("library %s (%s the EXR entry points), %s %dx%d -l %d, %d alternating runs after 3 warm-up rounds; ms = the frame in HBM to the "
          "last byte in pageable host memory" % (os.path.basename(nh.LIB_PATH), "with" if have else "without", FIXTURE, w, h, depth, runs))
    dev = torch.zeros((h, w, 4), dtype=torch.float64, device="cuda")
    host = torch.zeros((h, w, 4), dtype=torch.float64)
    torch.cuda.synchronize()
    gpu.render_device(dev.data_ptr(), w, h, depth)
    gpu.synchronize()
    t = {"half": [], "float": [], "doubles": []}
    files = {}
    for k in range(runs + 3):
        if have:
            for pixel in ("half", "float"):
                files[pixel] = gpu.encode_exr_device(dev.data_ptr(), None, w, h, pixel)
                if k >= 3:
                    t[pixel].append(gpu.exr_stats.ms)
        t0 = time.perf_counter()
        host.copy_(dev)
        torch.cuda.synchronize()
        if k >= 3:
            t["doubles"].append((time.perf_counter() - t0) * 1e3)
    fb = host.numpy()
    print("doubles to host (the --raw path): %d bytes, ms %s" % (fb.nbytes, spread(t["doubles"])))
    if not have:
        return
    for pixel in ("half", "float"):
        data = files[pixel]
        model = model_blocks(fb, pixel)
        blocks = file_blocks(data, len(model))
        raw_blocks = 0
        for (size, body), pre in zip(blocks, model):
            if size == len(pre):
                raw_blocks += 1
            else:
                assert zlib.decompress(body) == pre
        ours = sum(s for s, _ in blocks)
        z6 = sum(min(len(zlib.compress(pre, 6)), len(pre)) for pre in model)
        print("%5s file: %d bytes (%.3f a pixel, 1/%.1f of the doubles), ms %s, x%.3f of the doubles' median" % (
            pixel, len(data), len(data) / (w * h), fb.nbytes / len(data), spread(t[pixel]),
            statistics.median(t[pixel]) / statistics.median(t["doubles"])))
        print("%5s blocks: %d bytes of %d raw (%.1f %%); zlib level 6 over the same preprocessed blocks %d (ours x%.3f); %d of %d blocks raw; "
              "every compressed block inflates to the model" % (pixel, ours, sum(len(p) for p in model), 100.0 * ours / sum(len(p) for p in model),
                                                                z6, ours / z6, raw_blocks, len(blocks)))
    gpu.close()


if __name__ == "__main__":
    main()
