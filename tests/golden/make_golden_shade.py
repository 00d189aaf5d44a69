#!/usr/bin/env python3
"""Generate the SHADING fixtures shade3d .. shade12d from the COMPILED REFERENCE: one 48x27 frame at depth 8 of
tests/scenes/parity_shade.c per dimension, whose rays take every branch of apply_lights, get_ray_color and vectNd_refract
(tests/test_shading_known_answers.py counts them and holds the count).

    make -C oracle ref oracle
    python tests/golden/make_golden_shade.py [shade3d ...]

Every case stores the scene, the reference's double framebuffer with specular lighting (`fb`) and without (`fb_nospec`: the
shim's --specular 0 clears the flag that `ndt -p` clears, ndt.c:1583), and the reference's trace_kd counts of both renders.
Only data is written, with fixed time stamps: a second run reproduces every file byte for byte.  No other fixture is touched.
"""
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402
from make_golden_aimed import REF, SHIM, save_npz  # noqa: E402
from ndt_amd import load_scene  # noqa: E402

WIDTH, HEIGHT, DEPTH = 48, 27, 8
CASES = {"shade%dd" % n: n for n in range(3, 13)}


def generate(name, dims):
    base = ["--scene", os.path.join(REF, "scenes", "parity_shade.so"), "--dims", str(dims)]
    meta = dict(name=name, scene="parity_shade", dims=dims, frame=0, width=WIDTH, height=HEIGHT, depth=DEPTH,
                scene_file=name + ".ndtscene.gz", generator="tests/golden/make_golden_shade.py via oracle/ref_shim.c")
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        scene_txt = os.path.join(tmp, "scene.txt")
        make_golden.run_shim(base + ["--res", "8x8", "--no-render", "--tmp", tmp, "--scene-out", scene_txt])
        fs = load_scene(scene_txt)
        with open(scene_txt, "rb") as src, open(os.path.join(HERE, meta["scene_file"]), "wb") as raw:
            with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as dst:
                dst.write(src.read())
        meta["objects"] = fs.type_histogram()
        meta["kd_nodes"] = len(fs.kd_nodes)
        for specular, key, suffix in ((1, "fb", ""), (0, "fb_nospec", "_nospec")):
            info = make_golden.run_shim(base + ["--res", "%dx%d" % (WIDTH, HEIGHT), "--depth", str(DEPTH), "--threads", "4", "--tmp", tmp,
                                                "--specular", str(specular), "--fb-out", os.path.join(tmp, "fb.bin")])
            arrays[key] = np.fromfile(os.path.join(tmp, "fb.bin")).reshape(HEIGHT, WIDTH, 4)
            meta.update({k + suffix: v for k, v in info.items() if k.startswith("rays_")})
    save_npz(os.path.join(HERE, name + ".npz"), arrays)
    with open(os.path.join(HERE, name + ".json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: rays %d (specular) %d (none), %d + %d bytes" % (name, meta["rays_total"], meta["rays_total_nospec"],
                                                             os.path.getsize(os.path.join(HERE, name + ".npz")),
                                                             os.path.getsize(os.path.join(HERE, meta["scene_file"]))), flush=True)


def main():
    if not os.path.exists(SHIM):
        raise SystemExit("build the reference first: make -C oracle ref")
    for name in sys.argv[1:] or list(CASES):
        generate(name, CASES[name])


if __name__ == "__main__":
    main()
