"""Measurements of the ambient-occlusion stage; its output is committed in profiles/ao_on_device.txt.

At 1920x1080, K = 16: the 4-D benchmark scene (tests/golden/c3_random4d_1080p) and the 8-D hypercube (c5_hypercube8d_1080p), for
radius 0 and for a finite radius (a fifth of the longest side of the scene's box), and for radius 0 with 1 and all 16 samples a trace
launch (option ao_batch; auto is 4 at this size).  Per case the device time of the pass
(ndt_hip_ao_ms: rays, trace, hit points, fold of every batch), its launches and the AO rays a second -- K rays from every pixel
that shows something --, beside the rays a second of the same context's plain frame (every ray of the frame over its device time,
and over the time of its trace launches alone).  Medians of `runs` calls after one warm-up, with their spread.
Usage: python profiles/ao_probe.py [runs]"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ndt_amd import hip as nh, load_scene      # noqa: E402

FIXTURES = ("c3_random4d_1080p", "c5_hypercube8d_1080p")
K = 16


def spread(v):
    return "median %.3f [min %.3f .. max %.3f]" % (statistics.median(v), min(v), max(v))


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    gpu = nh.NdtHip(0)
    print("library %s, K = %d, %d runs after one warm-up" % (os.path.basename(nh.LIB_PATH), K, runs), flush=True)
    for fixture in FIXTURES:
        with open(os.path.join(ROOT, "tests", "golden", fixture + ".json")) as f:
            meta = json.load(f)
        w, h, depth = meta["width"], meta["height"], meta["depth"]
        fs = load_scene(os.path.join(ROOT, "tests", "golden", meta["scene_file"]))
        gpu.upload_scene(fs)
        frame_ms, trace_ms, rays = [], [], 0
        for k in range(runs + 1):
            _, st = gpu.render(w, h, depth, profile=1)
            if k:
                frame_ms.append(st.frame_ms)
                trace_ms.append(st.trace_ms)
                rays = st.rays_primary + st.rays_secondary + st.rays_shadow
        shadow = st.rays_shadow
        print("%s: %d-D, %d items, %dx%d -l %d: the plain frame traces %d rays (%d of them shadow rays) in frame_ms %s, trace_ms %s: "
              "%.1f M rays/s of the frame, %.1f M rays/s of its trace launches" % (
                  fixture, fs.dims, fs.n_items, w, h, depth, rays, shadow, spread(frame_ms), spread(trace_ms),
                  rays / statistics.median(frame_ms) / 1e3, rays / statistics.median(trace_ms) / 1e3), flush=True)
        sends = int((gpu.render_features(w, h, depth)["id"] != 0).sum())
        box = np.asarray(fs.vec(fs.bb["upper"])) - np.asarray(fs.vec(fs.bb["lower"]))
        for radius, batch in ((0.0, 0), (0.2 * float(box.max()), 0), (0.0, 1), (0.0, 16)):
            gpu.set_option("ao_batch", batch)
            ms, plane = [], None
            for k in range(runs + 1):
                plane = gpu.render_ao(w, h, depth, samples=K, radius=radius)
                if k:
                    ms.append(gpu.ao_ms())
            ao_rays = K * sends
            print("  radius %-8.4g ao_batch %-2d AO pass ao_ms %s in %d launches (feature pass included); %d AO rays (%d of %d pixels send %d "
                  "each): %.1f M rays/s; mean ao %.4f, %.1f %% of the hit pixels fully open" % (
                      radius, batch, spread(ms), gpu.ao_launches(), ao_rays, sends, w * h, K, ao_rays / statistics.median(ms) / 1e3,
                      float(plane.mean()), 100.0 * float((plane == 1.0).sum() - (w * h - sends)) / max(sends, 1)), flush=True)
        gpu.set_option("ao_batch", 0)
    gpu.close()


if __name__ == "__main__":
    main()
