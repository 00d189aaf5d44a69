"""Measurements of the EXR feature channels; its output is committed in profiles/exr_features_on_device.txt.

Two 1920x1080 frames (tests/golden/c3_random4d_1080p: the benchmark frame, 4-D, -l 4; c5_hypercube8d_1080p: 8-D): alternating,
as medians with their spread, the whole call -- render, encoder, the file's last byte in pageable host memory -- of
  render_exr(half)                  what `ndt_hip --exr` does per frame
  render_exr(half, features=all)    what `ndt_hip --exr --exr-aov all` does
and the feature pass alone into device memory (ndt_hip_render_features_device: primaries, trace, hit points, gather), with the
files' sizes.  Host clock around calls that end in a stream synchronise.
Usage: python profiles/exr_features_probe.py [runs]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ndt_amd import hip as nh, load_scene      # noqa: E402

FIXTURES = ("c3_random4d_1080p", "c5_hypercube8d_1080p")
ALL = ("id", "position", "normal")


def spread(v):
    return "median %.3f [min %.3f .. max %.3f]" % (statistics.median(v), min(v), max(v))


def main():
    import torch
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    gpu = nh.NdtHip(0)
    for fixture in FIXTURES:
        with open(os.path.join(ROOT, "tests", "golden", fixture + ".json")) as f:
            meta = json.load(f)
        w, h, depth, d = meta["width"], meta["height"], meta["depth"], meta["dims"]
        gpu.upload_scene(load_scene(os.path.join(ROOT, "tests", "golden", meta["scene_file"])))
        ident = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        pos = torch.zeros((d, h, w), dtype=torch.float64, device="cuda")
        nrm = torch.zeros((d, h, w), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        planes = nh.FeaturePlanes(ident.data_ptr(), pos.data_ptr(), nrm.data_ptr(), None, None)
        p = gpu.params(w, h, depth)
        t = {"plain": [], "features": [], "pass": [], "encode plain": [], "encode features": []}
        size = {}
        for k in range(runs + 3):
            for what, features in (("plain", None), ("features", ALL)):
                t0 = time.perf_counter()
                data, _ = gpu.render_exr(w, h, depth, pixel="half", features=features)
                ms = (time.perf_counter() - t0) * 1e3
                size[what] = len(data)
                if k >= 3:
                    t[what].append(ms)
                    t["encode " + what].append(gpu.exr_stats.ms)
            t0 = time.perf_counter()
            gpu._check(gpu.lib.ndt_hip_render_features_device(gpu.ctx, C.byref(p), C.byref(planes), None))
            if k >= 3:
                t["pass"].append((time.perf_counter() - t0) * 1e3)
        hits = int((ident > 0).sum().item())
        print("%s %dx%d %d-D -l %d, %d alternating runs after 3 warm-up rounds; %d of %d pixels hit something" % (fixture, w, h, d, depth, runs, hits, w * h))
        print("  --exr               (half A B G R):            %9d bytes   whole call ms %s   of it the encoder %s" % (
            size["plain"], spread(t["plain"]), spread(t["encode plain"])))
        print("  --exr --exr-aov all (+ id, P.*, N.*: %2d more):  %9d bytes   whole call ms %s   of it the encoder %s" % (
            1 + 2 * d, size["features"], spread(t["features"]), spread(t["encode features"])))
        print("  the feature pass alone, planes in device memory (%d launches): ms %s" % (gpu.features_launches(), spread(t["pass"])))
        print("  features cost: +%.3f ms a frame (x%.2f), +%d bytes (x%.2f)" % (
            statistics.median(t["features"]) - statistics.median(t["plain"]), statistics.median(t["features"]) / statistics.median(t["plain"]),
            size["features"] - size["plain"], size["features"] / size["plain"]))
    gpu.close()


if __name__ == "__main__":
    main()
