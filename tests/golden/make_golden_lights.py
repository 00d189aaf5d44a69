#!/usr/bin/env python3
"""Generate the many-light YAML fixtures (more lights than one 64-light window of the lighting kernels, DESIGN.md section 3
"Light windows") from the COMPILED REFERENCE.

Run in the build container only (needs /root/reference):

    make -C oracle ref
    python tests/golden/make_golden_lights.py [case ...]

Each case starts from the objects and camera of a committed YAML fixture the reference wrote (tests/golden/yaml/), keeps its
own lights, and appends a lattice of point lights, directional lights and ambient entries (at list positions 64, 65 and the
end, beside the scene's own ambient at 0, so that windows of 64 start and end on them) up to `lights` entries.  Spots are left
out: the reference's YAML reader drops a spot's `angle` (they are covered against the oracle, tests/test_many_lights.py).  The
reference then loads the file through its own scenes/yaml.so and renders it, exactly as make_golden.py:generate_yaml does:
  <name>.yaml.gz       the scene file
  <name>.ndtscene.gz   the scene the reference built from it, flattened
  <name>.npz           fb: the framebuffer the reference rendered
  <name>.json          sizes and the reference's trace_kd counts
"""
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, SHIM, run_shim  # noqa: E402

YDIR = os.path.join(HERE, "yaml")

# name -> the fixture whose objects and camera it keeps, dims, list length, render size and depth
CASES = {
    "yl_random4d_150": dict(base="y_random4d", dims=4, lights=150, render=(64, 36), depth=4, seed=11),
    "yl_hypercube6d_140": dict(base="y_hypercube6d", dims=6, lights=140, render=(48, 27), depth=8, seed=12),
}


def g16(x):
    return "%.16g" % x


def vec(v):
    return "[" + ", ".join(g16(x) for x in v) + "]"


def light_yaml(kind, color, pos=None, direction=None):
    lines = ["- type: " + kind, "  name:", "  color: {red: %s, green: %s, blue: %s}" % tuple(g16(c) for c in color)]
    if pos is not None:
        lines.append("  pos: " + vec(pos))
    if direction is not None:
        lines.append("  dir: " + vec(direction))
    return lines


def many_lights(text, dims, n_total, seed):
    """The YAML document `text` with its light list grown to n_total entries."""
    lines = text.split("\n")
    i_lights = lines.index("lights:")
    i_objects = lines.index("objects:")
    own = lines[i_lights + 1:i_objects]
    n_own = sum(1 for l in own if l.startswith("- type: "))
    rng = np.random.default_rng(seed)
    target = np.array([float(x) for x in next(l for l in lines if l.strip().startswith("viewTarget:")).split("[")[1].rstrip("]").split(",")])
    eye = np.array([float(x) for x in next(l for l in lines if l.strip().startswith("viewPoint:")).split("[")[1].rstrip("]").split(",")])
    span = float(np.linalg.norm(eye - target))
    scale = 4.0 / n_total
    new = []
    k = 0
    for at in range(n_own, n_total):
        if at in (64, 65) or at == n_total - 1:
            new += light_yaml("LIGHT_AMBIENT", (0.01, 0.012, 0.008))
            continue
        k += 1
        c = rng.uniform(0.5, 1.5, 3)
        if k % 5 == 3:
            d = -(eye - target) / span + rng.uniform(-0.4, 0.4, dims)
            new += light_yaml("LIGHT_DIRECTIONAL", 0.6 * c * scale, direction=np.round(d, 6))
            continue
        # a lattice of lamps around the point half way between the eye and the target, above the scene
        idx = np.array([(k >> (2 * j)) % 4 - 1.5 for j in range(dims)])
        pos = 0.5 * (eye + target) + 0.15 * span * idx + rng.uniform(-0.5, 0.5, dims)
        new += light_yaml("LIGHT_POINT", 150.0 * c * scale, pos=np.round(pos, 6))
    return "\n".join(lines[:i_objects] + new + lines[i_objects:])


def generate(name, case):
    print("==", name, flush=True)
    with gzip.open(os.path.join(YDIR, case["base"] + ".yaml.gz"), "rt") as f:
        text = f.read()
    text = many_lights(text, case["dims"], case["lights"], case["seed"])
    with tempfile.TemporaryDirectory() as tmp:
        yaml_path = os.path.join(tmp, name + ".yaml")
        with open(yaml_path, "w") as f:
            f.write(text)
        scene_txt = os.path.join(tmp, "scene.txt")
        base = ["--scene", os.path.join(REF, "scenes", "yaml.so"), "--config", yaml_path, "--dims", str(case["dims"]),
                "--frame", "0", "--tmp", tmp]
        run_shim(base + ["--res", "8x8", "--no-render", "--scene-out", scene_txt])
        with open(scene_txt) as f:
            n_loaded = sum(1 for l in f if l.startswith("light "))
        assert n_loaded == case["lights"], (n_loaded, case["lights"])
        for src, dst in ((yaml_path, name + ".yaml.gz"), (scene_txt, name + ".ndtscene.gz")):
            with open(src, "rb") as fi, open(os.path.join(YDIR, dst), "wb") as raw:
                with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as fo:
                    fo.write(fi.read())
        w, h = case["render"]
        info = run_shim(base + ["--res", "%dx%d" % (w, h), "--depth", str(case["depth"]), "--threads", str(os.cpu_count() or 1),
                                "--fb-out", os.path.join(tmp, "fb.bin")])
        meta = dict(name=name, scene=case["base"], dims=case["dims"], frames_written=[0], frame_loaded=0, config=None,
                    lights=case["lights"], generator="tests/golden/make_golden_lights.py via oracle/ref_shim.c")
        meta.update(info)
        meta.update(width=w, height=h, depth=case["depth"])
        np.savez_compressed(os.path.join(YDIR, name + ".npz"), fb=np.fromfile(os.path.join(tmp, "fb.bin")).reshape(h, w, 4))
        with open(os.path.join(YDIR, name + ".json"), "w") as f:
            json.dump(meta, f, indent=1, sort_keys=True)
            f.write("\n")
    print("   ", {k: v for k, v in meta.items() if k.startswith("rays")}, flush=True)


def main():
    if not os.path.exists(SHIM):
        raise SystemExit("build the reference first: make -C oracle ref")
    for name in sys.argv[1:] or list(CASES):
        generate(name, CASES[name])


if __name__ == "__main__":
    main()
