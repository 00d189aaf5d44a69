"""profiles/r05_light_windows.md: the compiled reference's own time (oracle/_ref, built by `make -C oracle ref`) for the scenes of
many_lights_probe.py -- config 3's random 4-D objects and camera (the YAML file the reference wrote for it,
tests/golden/yaml/y_random4d.yaml.gz) with the probe's 5 / 127 / 255 point lights -- at a REDUCED size, on 16 host threads.
Host only (no GPU)."""
import gzip
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_golden import REF, run_shim  # noqa: E402

W, H, DEPTH, THREADS = 480, 270, 4, 16


def lights_yaml(fs):
    out = []
    for l in fs.lights:
        kind = {0: "LIGHT_AMBIENT", 1: "LIGHT_POINT"}[l["type"]]
        out += ["- type: " + kind, "  name:", "  color: {red: %.17g, green: %.17g, blue: %.17g}" % (l["red"], l["green"], l["blue"])]
        if l["pos_off"] >= 0:
            out.append("  pos: [" + ", ".join("%.17g" % x for x in fs.vec(l["pos_off"])) + "]")
    return out


def main():
    import importlib.util
    spec = importlib.util.spec_from_file_location("probe_scenes", os.path.join(ROOT, "profiles", "many_lights_probe.py"))
    src = open(spec.origin).read().split("res = []")[0].replace("import torch\n", "").replace("from ndt_amd.hip import NdtHip\n", "")
    scope = {"__file__": spec.origin}
    exec(src, scope)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "yaml", "y_random4d.yaml.gz"), "rt") as f:
        lines = f.read().split("\n")
    i0, i1 = lines.index("lights:"), lines.index("objects:")
    for n in (5, 128, 256):
        fs = scope["lights_scene"](n)
        with tempfile.TemporaryDirectory() as tmp:
            y = os.path.join(tmp, "s.yaml")
            with open(y, "w") as f:
                f.write("\n".join(lines[:i0 + 1] + lights_yaml(fs) + lines[i1:]))
            info = run_shim(["--scene", os.path.join(REF, "scenes", "yaml.so"), "--config", y, "--dims", "4", "--frame", "0",
                             "--tmp", tmp, "--res", "%dx%d" % (W, H), "--depth", str(DEPTH), "--threads", str(THREADS),
                             "--fb-out", os.path.join(tmp, "fb.bin")])
        print("reference %dx%d -l %d, %d lights, %d threads: %.3f s render, rays_total %d" % (
            W, H, DEPTH, len(fs.lights), info.get("ref_threads", THREADS), info["ref_render_s"], info["rays_total"]), flush=True)


if __name__ == "__main__":
    main()
