#!/usr/bin/env python3
"""Record what the `ndt_hip` driver writes and says for every output sink and every way of combining them
(tests/test_driver_matrix.py compares a later build's driver with the record).

Run ONCE, on an MI355X, on the build of the commit whose driver is the reference (the parent of a change to ndt_amd/host):

    python tests/golden/make_golden_driver.py [--driver ndt_amd/host/ndt_hip] [--out tests/golden/driver_matrix.json]

Every case is one run of the driver at 16x9 over frames 0..1 of a two-document YAML scene (the 4-D fixtures y_random4d and
y_balls4d of tests/golden/yaml/, one document each: the frames differ, and so do the scene names in the file names), in a
directory of its own.  The record holds, per case,
  files    path -> sha256 and size of everything the run left under images/, depth/ and beside them (--raw)
  stdout   its lines, with what depends on the clock or the machine masked: the seconds of `rendering took` and `N frames
           in`, and the count of visible devices of `one frame over N GPU contexts`
The recorder runs every case twice and refuses to write a record the two passes disagree on: such a file or line is
taken out of the comparison by name (UNSTABLE), with the reason beside it.
"""
import argparse
import concurrent.futures
import gzip
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DRIVER = os.path.join(ROOT, "ndt_amd", "host", "ndt_hip")
RECORD = os.path.join(HERE, "driver_matrix.json")
DOCUMENTS = ("y_random4d", "y_balls4d")
SCENE = "two_frames.yaml"       # written beside the cases' directories: the driver says the path it reads, so it is relative
BASE = ["-s", "builtin:yaml", "-d", "4", "-l", "6", "-r", "16x9", "-f", "1"]
TIMEOUT_S = 60          # one driver run: a context, two tiny frames
WORKERS = 8             # driver processes at a time

PNG_GPU = ["--png", "--deflate", "gpu"]
MAP_GPU = ["-z", "--depth", "gpu"]
RAW = ["--raw", "f.f64"]

# the stills: every colour sink, alone and beside every map sink it goes with
STILLS = [
    ("ppm", []),
    ("png_stored", ["--png"]),
    ("png", PNG_GPU),
    ("jpeg", ["--jpeg"]),
    ("jpeg_q50_444", ["--jpeg", "--jpeg-quality", "50", "--jpeg-sampling", "444"]),
    ("raw", RAW),
    ("raw_png", RAW + PNG_GPU),
    ("map_host", ["-z"]),
    ("map_host_raw", ["-z"] + RAW),
    ("map_host_jpeg", ["-z", "--jpeg"]),
    ("map_gpu", MAP_GPU),
    ("map_gpu_png", MAP_GPU + PNG_GPU),
    ("map_gpu_png_depth_png", MAP_GPU + PNG_GPU + ["--depth-png"]),
    ("png16", PNG_GPU + ["--png16"]),
    ("png16_map", PNG_GPU + ["--png16"] + MAP_GPU + ["--depth-png"]),
]
AA = ["-a", "20,2"]
SSAA = ["--ssaa", "2"]
CASES = (
    STILLS
    + [("ssaa_" + name, SSAA + flags) for name, flags in STILLS]
    + [("apng", ["--apng"]), ("apng_ssaa", ["--apng"] + SSAA)]
    + [("aa", AA), ("aa_png", AA + PNG_GPU), ("aa_png16", AA + PNG_GPU + ["--png16"]), ("aa_apng", AA + ["--apng"]),
       ("anaglyph", ["-m", "a"])]
    + [("g%d_%s" % (n, name), ["-g", str(n)] + flags) for n in (2, 3) for name, flags in (("ppm", []), ("png", PNG_GPU), ("jpeg", ["--jpeg"]))]
    + [("ssaa_g2_" + name, SSAA + ["-g", "2"] + flags) for name, flags in (("ppm", []), ("png", PNG_GPU), ("jpeg", ["--jpeg"]))]
    + [("j2_png", ["-j", "2"] + PNG_GPU)]
)
FILES_ONLY = {"j2_png"}     # the two workers' lines interleave on stdout
# "case:path" or "case:stdout" entries that two runs of one build disagree on (none was found)
UNSTABLE = set()


def write_scene(path):
    """The two-frame scene file: one YAML document per fixture."""
    with open(path, "wb") as f:
        for name in DOCUMENTS:
            with gzip.open(os.path.join(HERE, "yaml", name + ".yaml.gz"), "rb") as doc:
                f.write(doc.read())


def masked(line):
    line = re.sub(r"\d+\.\d+(?=s\b| frames/s)", "#", line)
    return re.sub(r"\(\d+ device\(s\) visible\)", "(# device(s) visible)", line)


def run_case(driver, cwd, flags):
    """What one run wrote and said; raises with the run's own words when it does not end with status 0."""
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run([driver] + BASE + ["-u", os.path.join("..", SCENE)] + flags, capture_output=True, text=True, cwd=cwd, timeout=TIMEOUT_S)
    if r.returncode != 0:
        raise RuntimeError("%s: exit status %d\n%s\n%s" % (" ".join(flags), r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    files = {}
    for top, _, names in os.walk(cwd):
        for n in names:
            with open(os.path.join(top, n), "rb") as f:
                data = f.read()
            files[os.path.relpath(os.path.join(top, n), cwd)] = {"sha256": hashlib.sha256(data).hexdigest(), "bytes": len(data)}
    return {"files": files, "stdout": [masked(s) for s in r.stdout.splitlines()]}


def run_matrix(driver, work):
    """Every case, a few at a time; the first run that fails or hangs keeps the ones not yet started from starting."""
    write_scene(os.path.join(work, SCENE))
    stop = threading.Event()

    def one(case):
        name, flags = case
        if stop.is_set():
            return name, None
        try:
            return name, run_case(driver, os.path.join(work, name), flags)
        except BaseException:
            stop.set()
            raise

    with concurrent.futures.ThreadPoolExecutor(WORKERS) as pool:
        return dict(pool.map(one, CASES))


def compared(name, got):
    """The part of a case's record that is compared."""
    files = {p: v for p, v in got["files"].items() if "%s:%s" % (name, p) not in UNSTABLE}
    lines = None if name in FILES_ONLY or name + ":stdout" in UNSTABLE else got["stdout"]
    return files, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--driver", default=DRIVER)
    ap.add_argument("--out", default=RECORD)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as a, tempfile.TemporaryDirectory() as b:
        first, second = run_matrix(os.path.abspath(args.driver), a), run_matrix(os.path.abspath(args.driver), b)
    differ = [name for name, _ in CASES if compared(name, first[name]) != compared(name, second[name])]
    for name in differ:
        print("two runs differ: %s\n  %r\n  %r" % (name, compared(name, first[name]), compared(name, second[name])))
    if differ:
        return 1
    with open(args.out, "w") as f:
        json.dump({"base": BASE, "documents": DOCUMENTS, "cases": {name: dict(first[name], flags=flags) for name, flags in CASES}}, f,
                  indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, %d files -> %s" % (len(CASES), sum(len(first[n]["files"]) for n, _ in CASES), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
