"""profiles/r05_light_windows.md: the 1080p 4-D random scene (config 3's objects and camera) with 5 (as shipped), 128 and 256 point lights: ms/frame, trace launches,
device memory the context holds after the render."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ndt_amd import load_scene
from ndt_amd.hip import NdtHip


def lights_scene(n):
    fs = load_scene(os.path.join(ROOT, "tests", "golden", "c3_random4d.ndtscene.gz"))
    if n <= len(fs.lights):
        return fs
    base = fs.lights
    rng = np.random.default_rng(7)
    anchors = [fs.vec(l["pos_off"]) for l in base if l["pos_off"] >= 0]
    lights = [base[0]]
    while len(lights) < n:
        a = anchors[len(lights) % len(anchors)]
        pos = a + rng.uniform(-6, 6, fs.dims)
        lights.append(dict(type=1, red=200.0 * 5 / n, green=200.0 * 5 / n, blue=200.0 * 5 / n, angle=0.0,
                           pos_off=fs.add_vec(list(pos)), dir_off=-1, area_off=-1, radius=0.0))
    fs.lights = lights
    fs._struct = None
    fs.finalize()
    return fs


res = []
for n in (5, 128, 256):
    fs = lights_scene(n)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    gpu = NdtHip(0)
    gpu.upload_scene(fs)
    for _ in range(3):
        gpu.render(1920, 1080, 4)
    free1, _ = torch.cuda.mem_get_info()
    walls, frames = [], []
    for _ in range(10):
        t = time.perf_counter()
        out, st = gpu.render(1920, 1080, 4, profile=1)
        walls.append((time.perf_counter() - t) * 1e3)
        frames.append(st.frame_ms)
    r = dict(lights=len(fs.lights), windows=(len(fs.lights) + 63) // 64, frame_ms_median=float(np.median(frames)),
             frame_ms_min=float(np.min(frames)), wall_ms_median=float(np.median(walls)), trace_launches=st.trace_launches,
             levels=st.levels, rays_shadow=st.rays_shadow, rays_secondary=st.rays_secondary, rays_ref_equiv=st.rays_ref_equiv,
             node_capacity=st.node_capacity, device_bytes_held=int(free0 - free1))
    print(json.dumps(r), flush=True)
    res.append(r)
    gpu.close()
