"""The bounding-sphere fits of a frame on the device: ndt_hip_fit_spheres (ndt_amd/csrc/ndt_fit.hip), `ndt_hip --fit gpu`.

The host fit (bounds_list_optimal: ndt_amd/host/src/ndt_bounding.c, ndt_nelder_mead.c) is the specification, and both
sides are sequences of correctly rounded IEEE operations: every comparison here is equality of 64-bit patterns.

About the "centroid wins" branch (ndt_bounding.c:98-101, the search ended more than EPSILON worse than it started): the
seed IS the centroid and enters the simplex with the centroid's radius; every later replacement goes to the worst or the
second worst rank of the sorted simplex (ndt_nelder_mead.c:96-146 with N >= 3), never to rank 0, so the best value of the
simplex never rises above the centroid's and the branch cannot be taken by a deterministic evaluation.  A search over
every list of these batches plus 20 000 random ones on the CPU twin found none, as that argument says;
test_batches_cover_the_search asserts the count (zero) so that a change of the host model that makes the branch
reachable shows up here, and the device code restates the branch all the same.
"""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, GOLDEN, golden
from ndt_amd import hip as nh
from ndt_amd import flat_scene as fsmod

HOST = os.path.join(ROOT, "ndt_amd", "host")
DRIVER = os.path.join(HOST, "ndt_hip")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "scenes")
ALL_DIMS = list(range(3, 13))
FULL_SEARCH = 1001          # results of a search that ran into nm_done's iteration limit (ndt_nelder_mead.c:226)


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "ndt_amd", "csrc"), "-j", "8"], check=True, capture_output=True)
    subprocess.run(["make", "-C", HOST], check=True, capture_output=True)
    assert os.path.exists(DRIVER)
    return DRIVER


@pytest.fixture(scope="module")
def host(built):
    lib = C.CDLL(os.path.join(HOST, "libndt_host.so"))
    lib.ndt_host_fit_spheres.argtypes = [C.c_int, C.c_int64] + [C.c_void_p] * 5
    lib.ndt_host_fit_spheres_traced.argtypes = [C.c_int, C.c_int64] + [C.c_void_p] * 7
    return lib


def host_fit(lib, dims, lists, traced=False):
    first, points, radii = nh.pack_point_lists(dims, lists)
    centers = np.zeros((len(lists), dims))
    out = np.zeros(len(lists))
    if not traced:
        assert lib.ndt_host_fit_spheres(dims, len(lists), first.ctypes.data, points.ctypes.data, radii.ctypes.data,
                                        centers.ctypes.data, out.ctypes.data) == 0
        return centers, out
    evals = np.zeros(len(lists), dtype=np.int32)
    won = np.zeros(len(lists), dtype=np.int32)
    assert lib.ndt_host_fit_spheres_traced(dims, len(lists), first.ctypes.data, points.ctypes.data, radii.ctypes.data,
                                           centers.ctypes.data, out.ctypes.data, evals.ctypes.data, won.ctypes.data) == 0
    return centers, out, evals, won


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def corners(rng, n, m, scale):
    """the 2^m corners pos + sum_j b_j dir_j of an m-dimensional parallelotope in n-D, non-orthogonal edges"""
    pos = rng.uniform(-1, 1, n) * scale
    dirs = rng.normal(size=(m, n)) * scale * rng.uniform(0.1, 1.0, (m, 1))
    if m > 1:
        dirs[1:] += 0.3 * dirs[0]
    b = ((np.arange(1 << m)[:, None] >> np.arange(m)) & 1).astype(np.float64)
    return pos + b @ dirs


def batch(n, seed=2026):
    """A few hundred lists of every kind a scene produces, coordinates of magnitude 1e-3 .. 1e3."""
    rng = np.random.default_rng(seed * 100 + n)
    lists = []

    def mag():
        return 10.0 ** rng.uniform(-3, 3)

    for _ in range(40):                                     # spheres: one point with its radius
        s = mag()
        lists.append((rng.uniform(-1, 1, (1, n)) * s, np.array([rng.uniform(0.01, 2) * s])))
    for kind in range(4):                                   # cylinder ends: radii equal, unequal, one zero, one negative
        for _ in range(12):
            s = mag()
            r = rng.uniform(0.01, 2) * s
            rad = [(r, r), (r, rng.uniform(0.01, 2) * s), (r, 0.0), (r, -r)][kind]
            lists.append((rng.uniform(-1, 1, (2, n)) * s, np.array(rad)))
    for _ in range(40):                                     # facets
        lists.append((rng.uniform(-1, 1, (3, n)) * mag(), np.zeros(3)))
    for m in range(1, n):                                   # orthotopes: 2^m corners
        for _ in range(8 if m <= 8 else 3):
            lists.append((corners(rng, n, m, mag()), np.zeros(1 << m)))
    for _ in range(3):                                      # an hcube's own 2^n corners
        lists.append((corners(rng, n, n, mag()), np.zeros(1 << n)))
    for k in (1, 2, 5, 70):                                 # coincident points
        p = rng.uniform(-1, 1, n) * mag()
        lists.append((np.tile(p, (k, 1)), np.zeros(k)))
        lists.append((np.tile(p, (k, 1)), np.full(k, 0.25)))
    for _ in range(12):                                     # odd lengths: neither a power of two nor a multiple of the lanes
        k = int(rng.integers(5, 200))
        s = mag()
        lists.append((rng.uniform(-1, 1, (k, n)) * s, rng.uniform(-0.1, 0.5, k) * s))
    # searches that run into the iteration limit (found on the CPU with the traced twin: wide clouds of points with large
    # radii end there from 4-D on for about every tenth seed, in 3-D for 19 of 4 000; FULL_SEEDS keeps two seeds per
    # dimension and test_batches_cover_the_search checks that they still do)
    for sd in FULL_SEEDS[n]:
        lists.append(slow_list(n, sd))
    return lists


FULL_SEEDS = {3: (157, 263), 4: (15, 20), 5: (1, 4), 6: (0, 5), 7: (0, 1), 8: (0, 1), 9: (0, 1), 10: (0, 1), 11: (0, 1), 12: (0, 1)}


def slow_list(n, sd):
    rng = np.random.default_rng(7000 * n + sd)
    k = int(rng.integers(2, 40))
    return rng.uniform(-1, 1, (k, n)) * 1e3, rng.uniform(0, 1e3, k)


# ------------------------------------------------------------------ 4. the twin, and refusals (no GPU)

@pytest.mark.parametrize("n", ALL_DIMS)
def test_host_twin_runs_and_is_deterministic(host, n):
    lists = batch(n)
    c1, r1 = host_fit(host, n, lists)
    c2, r2 = host_fit(host, n, lists)
    assert np.array_equal(bits(c1), bits(c2)) and np.array_equal(bits(r1), bits(r2))
    assert np.isfinite(c1).all() and np.isfinite(r1).all() and (r1 >= 0).all()
    # it is bounds_list_optimal: every point (with its radius, when positive) is inside the sphere it returns
    for (pts, rad), c, r in zip(lists, c1, r1):
        reach = np.sqrt(((pts - c) ** 2).sum(axis=1)) + np.where(rad > 0, rad, 0.0)
        assert reach.max() <= r * (1 + 1e-12) + 1e-300


def test_batches_cover_the_search(host):
    """Every batch holds a search that took all 1 001 results and one that ended early; no list trips "centroid wins" (module
    docstring: the branch cannot be reached; 20 000 more random lists agree)."""
    wins = 0
    for n in ALL_DIMS:
        lists = batch(n)
        _, _, evals, won = host_fit(host, n, lists, traced=True)
        assert evals.max() == FULL_SEARCH and evals.min() < FULL_SEARCH, (n, evals.min(), evals.max())
        assert (evals[-len(FULL_SEEDS[n]):] == FULL_SEARCH).all(), (n, evals[-len(FULL_SEEDS[n]):])
        wins += int(won.sum())
    rng = np.random.default_rng(5)
    for n in (3, 4, 7):
        more = []
        for _ in range(20000 // 3):
            k = int(rng.integers(1, 9))
            s = 10.0 ** rng.uniform(-3, 3)
            more.append((rng.uniform(-1, 1, (k, n)) * s, rng.uniform(-0.5, 1, k) * s))
        _, _, _, won = host_fit(host, n, more, traced=True)
        wins += int(won.sum())
    assert wins == 0


def test_fit_spheres_refuses_bad_arguments_without_a_device():
    lib = nh.load_library()
    first = np.array([0, 1], dtype=np.int64)
    pts = np.zeros((1, 16))
    rad = np.zeros(1)
    cen = np.zeros(16)
    out = np.zeros(1)
    for dims in (2, 13, 0, -1):
        assert lib.ndt_hip_fit_spheres(None, dims, 1, first.ctypes.data, pts.ctypes.data, rad.ctypes.data, cen.ctypes.data,
                                       out.ctypes.data) == fsmod.NDT_E_INVALID
        assert b"dimensions" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_fit_spheres(None, 4, 1, first.ctypes.data, pts.ctypes.data, rad.ctypes.data, cen.ctypes.data,
                                   out.ctypes.data) == fsmod.NDT_E_INVALID
    assert b"ctx is NULL" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_fit_launches(None) == 0


def _dump(driver, prog, dims, frame, out, config=None, extra=()):
    cmd = [driver, "-s", os.path.join(REF_BIN, prog + ".so"), "-d", str(dims), "-f", "%d:%d" % (frame, frame), "--dump-scene", out]
    if config:
        cmd += ["-u", config]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=os.path.dirname(out))


def _fixture_text(name):
    with gzip.open(os.path.join(GOLDEN, name + ".ndtscene.gz"), "rt") as f:
        return f.read()


@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built (make -C oracle ref)")
def test_fit_gpu_without_a_device_fails_loudly_and_the_default_is_unchanged(built, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    out = str(tmp_path / "out.ndtscene")
    r = _dump(built, "random", 4, 0, out, extra=["--fit", "gpu"])
    assert r.returncode != 0
    assert "no HIP device" in (r.stderr + r.stdout)
    assert not os.path.exists(out)
    for extra in ([], ["--fit", "host"]):
        r = _dump(built, "random", 4, 0, out, extra=extra)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "bounding spheres on GPU" not in r.stdout
        assert open(out).read() == _fixture_text("c3_random4d")
    bad = _dump(built, "random", 4, 0, out, extra=["--fit", "fpga"])
    assert bad.returncode != 0 and "--fit" in bad.stderr


# ndt_flatten_scene_fit with the CPU twin as the fitter, in a process of its own (scene programs draw from drand48): prints
# "<same|different> <objects fitted> <lists of every call>"
_FLATTEN_WITH_TWIN = r"""
import ctypes as C, gzip, os, re, sys
host, so_path, dims, frame, config, threads, fixture, out = sys.argv[1:9]
dims, frame, threads, config = int(dims), int(frame), int(threads), (None if sys.argv[5] == "-" else sys.argv[5].encode())
lib = C.CDLL(os.path.join(host, "libndt_host.so"), mode=C.RTLD_GLOBAL)
lib.ndt_host_fit_spheres.argtypes = [C.c_int, C.c_int64] + [C.c_void_p] * 5
FIT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
calls = []
def fit(arg, d, n, first, pts, rad, cen, out_r, err, err_len):
    calls.append(n)
    return lib.ndt_host_fit_spheres(d, n, first, pts, rad, cen, out_r)
fit_c = FIT(fit)
lib.register_objects(b"objects")
so = C.CDLL(so_path)
frames = so.scene_frames(dims, config) if hasattr(so, "scene_frames") else 300
for i in range(frame + 1):
    scn = C.create_string_buffer(1 << 16)       # (a `scene`, generously)
    so.scene_setup(scn, dims, i, frames, config)
fb, err, stats = C.create_string_buffer(1 << 13), C.create_string_buffer(256), C.create_string_buffer(64)
assert lib.ndt_flatten_scene_fit(scn, fb, err, 256, threads, fit_c, None, stats) == 0, err.value
want = gzip.open(fixture, "rt").read()
lib.ndt_write_ndtscene(fb, re.search(r"^name (.*)$", want, re.M).group(1).encode(), out.encode())
sys.stdout.flush()
print("\nTWIN", "same" if open(out).read() == want else "different", C.cast(stats, C.POINTER(C.c_int64))[0], *calls)
"""


@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built (make -C oracle ref)")
@pytest.mark.parametrize("threads", [1, 7])
@pytest.mark.parametrize("name", ["c1_hypercube3d", "c3_random4d", "c5_hypercube6d", "zoo4d", "zoo5d_f2", "zoo12d"])
def test_flatten_with_delegated_fits_gives_the_references_scene(built, tmp_path, name, threads):
    """ndt_flatten_scene_fit (what `--fit gpu` runs) with the CPU twin standing in for the device: the scene is the fixture's,
    the fitter is called at most three times a frame and makes the sphere of every finite object exactly once."""
    import sys
    prog, dims, frame, config = SCENES[name]
    r = subprocess.run([sys.executable, "-c", _FLATTEN_WITH_TWIN, HOST, os.path.join(REF_BIN, prog + ".so"), str(dims), str(frame),
                        config or "-", str(threads), os.path.join(GOLDEN, name + ".ndtscene.gz"), str(tmp_path / "out.ndtscene")],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    said = [line.split() for line in r.stdout.splitlines() if line.startswith("TWIN ")][-1]
    assert said[1] == "same"
    calls = [int(x) for x in said[3:]]
    assert 1 <= len(calls) <= 3
    assert int(said[2]) == _finite_objects(_fixture_text(name))


# ------------------------------------------------------------------ 1. known answers, bit for bit

@pytest.mark.gpu
@pytest.mark.parametrize("n", ALL_DIMS)
def test_device_fit_equals_the_host_fit_bit_for_bit(host, n):
    lists = batch(n)
    want_c, want_r = host_fit(host, n, lists)
    gpu = nh.NdtHip(0)
    try:
        got_c, got_r = gpu.fit_spheres(n, lists)
        launches = gpu.fit_launches()
        # the same lists in another order (other neighbours in the wavefront, other bins' boundaries), on the grown buffers
        order = np.random.default_rng(n).permutation(len(lists))
        sh_c, sh_r = gpu.fit_spheres(n, [lists[i] for i in order])
        few_c, few_r = gpu.fit_spheres(n, lists[:3])
    finally:
        gpu.close()
    bad = np.flatnonzero((bits(got_r) != bits(want_r)) | (bits(got_c) != bits(want_c)).any(axis=1))
    print("N = %d: %d lists, %d points, %d launches, %d lists differ" % (n, len(lists), sum(len(r) for _, r in lists), launches, len(bad)))
    for i in bad[:5]:
        print("  list %d (%d points): radius %r / %r" % (i, len(lists[i][1]), got_r[i], want_r[i]))
    assert len(bad) == 0
    assert 2 <= launches <= 7                              # one per group of list lengths: short lists a lane each, long ones shared
    assert np.array_equal(bits(sh_c), bits(want_c[order])) and np.array_equal(bits(sh_r), bits(want_r[order]))
    assert np.array_equal(bits(few_c), bits(want_c[:3])) and np.array_equal(bits(few_r), bits(want_r[:3]))


@pytest.mark.gpu
def test_device_fit_refuses_what_the_caller_has_to_fit_itself():
    gpu = nh.NdtHip(0)
    try:
        ok = (np.ones((2, 4)), np.zeros(2))
        for bad in ((np.zeros((0, 4)), np.zeros(0)), (np.array([[0.0, np.nan, 0, 0]]), np.zeros(1)),
                    (np.array([[0.0, np.inf, 0, 0]]), np.zeros(1)), (np.ones((1, 4)), np.array([np.nan]))):
            with pytest.raises(nh.NdtHipError) as e:
                gpu.fit_spheres(4, [ok, bad])
            assert e.value.code == fsmod.NDT_E_INVALID
        c, r = gpu.fit_spheres(4, [])
        assert c.shape == (0, 4) and r.shape == (0,) and gpu.fit_launches() == 0
    finally:
        gpu.close()


# ------------------------------------------------------------------ 2. the reference's spheres

# fixture -> (scene program, dims, frame, config)
SCENES = {
    "c1_hypercube3d": ("hypercube", 3, 0, None), "c2_balls4d": ("balls", 4, 0, None), "c3_random4d": ("random", 4, 0, None),
    "c5_hypercube6d": ("hypercube", 6, 0, None), "c5_hypercube8d": ("hypercube", 8, 0, None), "zoo4d": ("parity_zoo", 4, 0, None),
    "zoo5d_f2": ("parity_zoo", 5, 2, None), "zoo6d": ("parity_zoo", 6, 0, None), "zoo9d": ("parity_zoo", 9, 0, None),
    "zoo12d": ("parity_zoo", 12, 0, "nohcube"),
}
FITTED = re.compile(r"fitted (\d+) bounding spheres on GPU (\d+) in (\d+) launches")


def _finite_objects(text):
    """objects of an ndtscene text whose bounding sphere was fitted: a radius of -1 marks an infinite one (object.c:582-603)"""
    radii = [float.fromhex(line.split()[1]) for line in text.splitlines() if line.startswith("bounds ")]
    return sum(1 for r in radii if r != -1.0)


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built")
@pytest.mark.parametrize("threads", [1, 7])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_fit_gpu_dump_is_the_references_scene_byte_for_byte(built, tmp_path, name, threads):
    prog, dims, frame, config = SCENES[name]
    out = str(tmp_path / "out.ndtscene")
    r = _dump(built, prog, dims, frame, out, config, extra=["--fit", "gpu", "-t", str(threads)])
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    want = _fixture_text(name)
    assert open(out).read() == want
    said = FITTED.findall(r.stdout)
    assert len(said) == 1, r.stdout[-2000:]
    k, dev, launches = (int(x) for x in said[0])
    print("%s -t %d: %s" % (name, threads, said[0]))
    # K counts objects, not calls: every finite object of the fixture -- kd items and nested faces -- got its sphere from the
    # device, and nothing else did
    assert k == _finite_objects(want) > 0
    assert launches >= 1 and dev == 0


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built")
def test_fit_gpu_with_frames_in_flight(built, tmp_path):
    """frames 30 .. 33 of the 3-D hypercube: the dumps and, with -j 2 (every worker fits on its own context), the images of
    `--fit gpu` are those of `--fit host`"""
    for frame in (30, 31, 32, 33):
        texts = []
        for fit in ("host", "gpu"):
            out = str(tmp_path / ("f%d_%s.ndtscene" % (frame, fit)))
            r = _dump(built, "hypercube", 3, frame, out, extra=["--fit", fit])
            assert r.returncode == 0, r.stderr[-2000:]
            texts.append(open(out).read())
        assert texts[0] == texts[1]
    images = []
    for fit, j in (("host", 1), ("gpu", 2)):
        d = tmp_path / ("img_%s" % fit)
        d.mkdir()
        cmd = [built, "-s", os.path.join(REF_BIN, "hypercube.so"), "-d", "3", "-r", "96x64", "-l", "16", "-f", "30:33", "-j", str(j), "--fit", fit]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(d))
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        assert len(FITTED.findall(r.stdout)) == (4 if fit == "gpu" else 0)
        files = sorted(p for p in (d / "images").rglob("*.ppm"))
        assert len(files) == 4
        images.append([p.read_bytes() for p in files])
    assert images[0] == images[1] and len(set(images[0])) == 4


# ------------------------------------------------------------------ 3. to pixels

@pytest.mark.gpu
@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", ["c3_random4d", "c5_hypercube6d"])
def test_fit_gpu_to_pixels(built, tmp_path, name):
    prog, dims, frame, config = SCENES[name]
    g = golden(name)
    raw = str(tmp_path / "fb.f64")
    cmd = [built, "-s", os.path.join(REF_BIN, prog + ".so"), "-d", str(dims), "-f", "0", "-r", "%dx%d" % (g.width, g.height),
           "-l", str(g.depth), "--raw", raw, "--fit", "gpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    assert len(FITTED.findall(r.stdout)) == 1
    fb = np.fromfile(raw).reshape(g.height, g.width, 4)
    assert np.abs(fb - g.data["fb"]).max() < 1e-9          # the bound of test_end_to_end_reference_scene_to_pixels
