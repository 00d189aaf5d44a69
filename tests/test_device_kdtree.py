"""A frame's kd-tree on the device: ndt_hip_build_kdtree (ndt_amd/csrc/ndt_kd.hip), `ndt_hip --kd gpu`.

The host builder (ndt_amd/host/src/ndt_kdtree.c, behind ndt_host_build_kdtree: "the twin") is the specification, and the
golden scene dumps carry the compiled reference's tree node for node.  The search is made of one correctly rounded add per
bound, comparisons of doubles and integer scores: "equal" below always means equality of bytes.
"""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN, golden
from ndt_amd import hip as nh
from ndt_amd import flat_scene as fsmod
from test_device_fit import SCENES

HOST = os.path.join(ROOT, "ndt_amd", "host")
DRIVER = os.path.join(HOST, "ndt_hip")
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "scenes")
ALL_DIMS = list(range(3, 13))
EPS = 1e-4                  # EPSILON, ndt_host_api.h
DBL_MAX = np.finfo(np.float64).max
NODE = np.dtype(fsmod.FlatKdNode)
BUILT = re.compile(r"built kd-tree of (\d+) nodes on GPU (\d+) in (\d+) launches")
GPU_TIMEOUT = 300           # seconds a subprocess that uses the GPU may take


def kd_stack():
    """NDT_KD_STACK: the kd depth the traversal stack of the trace kernels holds"""
    with open(os.path.join(ROOT, "ndt_amd", "csrc", "ndt_device.hpp")) as f:
        return int(re.search(r"^#define NDT_KD_STACK (\d+)", f.read(), re.M).group(1))


def _stale():
    """a native piece is missing, or older than one of its sources (then, and only then, the fixture runs make: where the
    objects are gone, make would compile the whole library again)"""
    def newest(dirs, extra=()):
        files = list(extra)
        for d in dirs:
            files += [os.path.join(d, f) for f in os.listdir(d) if f.endswith((".hip", ".hpp", ".c", ".h"))]
        return max(os.path.getmtime(p) for p in files)

    header = os.path.join(ROOT, "include", "ndt_hip.h")
    lib = os.path.join(ROOT, "ndt_amd", "libndt_hip.so")
    host = [os.path.join(HOST, "libndt_host.so"), DRIVER]
    if not all(os.path.exists(p) for p in [lib] + host):
        return True
    if newest([os.path.join(ROOT, "ndt_amd", "csrc")], [header]) > os.path.getmtime(lib):
        return True
    return newest([os.path.join(HOST, "src"), os.path.join(HOST, "include")], [header]) > min(os.path.getmtime(p) for p in host)


@pytest.fixture(scope="module")
def built():
    if _stale():
        subprocess.run(["make", "-C", os.path.join(ROOT, "ndt_amd", "csrc"), "-j", "8"], check=True, capture_output=True)
        subprocess.run(["make", "-C", HOST], check=True, capture_output=True)
    assert os.path.exists(DRIVER)
    return DRIVER


class HostKdTree(C.Structure):
    _fields_ = [("n_kd_nodes", C.c_int32), ("n_leaf_refs", C.c_int32), ("n_inf", C.c_int32), ("depth", C.c_int32),
                ("nodes", C.c_void_p), ("leaf_refs", C.c_void_p), ("inf_refs", C.c_void_p), ("bb_lower", C.c_void_p),
                ("bb_upper", C.c_void_p)]


@pytest.fixture(scope="module")
def host(built):
    lib = C.CDLL(os.path.join(HOST, "libndt_host.so"))
    lib.ndt_host_build_kdtree.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.ndt_host_kdtree_free.argtypes = [C.c_void_p]
    return lib


def twin(lib, dims, lower, upper, finite):
    """ndt_host_build_kdtree: ((nodes, leaf_refs, inf_refs, bb_lower, bb_upper), depth)"""
    n, lower, upper, finite = nh.pack_boxes(dims, lower, upper, finite)
    t = HostKdTree()
    assert lib.ndt_host_build_kdtree(dims, n, lower.ctypes.data, upper.ctypes.data, finite.ctypes.data, C.addressof(t)) == 0

    def take(ptr, count, dtype):
        if count == 0:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).copy()

    out = (take(t.nodes, t.n_kd_nodes, NODE), take(t.leaf_refs, t.n_leaf_refs, np.int32), take(t.inf_refs, t.n_inf, np.int32),
           take(t.bb_lower, dims, np.float64), take(t.bb_upper, dims, np.float64))
    depth = t.depth
    lib.ndt_host_kdtree_free(C.addressof(t))
    return out, depth


def same_tree(a, b):
    return (a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
            and np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64)) and np.array_equal(a[4].view(np.uint64), b[4].view(np.uint64)))


# ------------------------------------------------------------------ the synthetic box sets

def invert(lower, upper, rows):
    lower[rows] = DBL_MAX       # a flattened cluster child without bounding points (ndt_kdtree.c: ndt_kd_add_object)
    upper[rows] = -DBL_MAX


def small_boxes(rng, n, count, spread=10.0):
    centre = rng.uniform(-spread, spread, (count, n))
    half = rng.uniform(0.05, 0.3, (count, n))
    return centre - half, centre + half


def box_sets(n, seed=2027):
    """name -> (lower, upper, finite) for dimension n"""
    rng = np.random.default_rng(seed * 100 + n)
    sets = {}
    lo, up = small_boxes(rng, n, 300)
    sets["separated"] = (lo, up, np.ones(300, dtype=np.uint8))
    lo2, up2 = lo.copy(), up.copy()
    invert(lo2, up2, rng.permutation(300)[:60])
    sets["inverted"] = (lo2, up2, np.ones(300, dtype=np.uint8))
    # lattice coordinates: many boxes share exact bound values in a dimension, candidates tie in score
    centre = rng.integers(0, 4, (200, n)).astype(np.float64)
    sets["lattice"] = (centre - 0.25, centre + 0.25, np.ones(200, dtype=np.uint8))
    one_lo, one_up = small_boxes(rng, n, 1)
    sets["identical"] = (np.tile(one_lo, (50, 1)), np.tile(one_up, (50, 1)), np.ones(50, dtype=np.uint8))
    sets["n0"] = (np.zeros((0, n)), np.zeros((0, n)), np.zeros(0, dtype=np.uint8))
    for k in (1, 2):
        lo, up = small_boxes(rng, n, k)
        sets["n%d" % k] = (lo, up, np.ones(k, dtype=np.uint8))
    lo, up = small_boxes(rng, n, 210)
    fin = np.ones(210, dtype=np.uint8)
    fin[rng.permutation(210)[:30]] = 0
    invert(lo, up, np.flatnonzero(fin == 0)[:10])           # some of the non-finite items have no box either
    invert(lo, up, np.flatnonzero(fin == 1)[:5])
    sets["nonfinite"] = (lo, up, fin)
    sets["none_finite"] = (lo[:7].copy(), up[:7].copy(), np.zeros(7, dtype=np.uint8))
    if n == 8:
        lo, up = small_boxes(rng, n, 2400)
        sets["big"] = (lo, up, np.ones(2400, dtype=np.uint8))
    return sets


_TWINS = {}


def twin_of(lib, n, name):
    """the twin's tree of a set, checked to be tame: no test depends on the growth path or the depth limit by accident"""
    if (n, name) not in _TWINS:
        lower, upper, finite = box_sets(n)[name]
        tree, depth = twin(lib, n, lower, upper, finite)
        assert len(tree[0]) < 20000 and depth < 30, (n, name, len(tree[0]), depth)
        _TWINS[(n, name)] = (tree, depth)
    return _TWINS[(n, name)]


def chain(n, m):
    """A set whose tree is a chain: m small boxes in a row along axis 0 and, from every gap between them, three long boxes
    that reach past the end.  Cutting off more than the first small box makes straddlers of the long ones that began before
    it, so the best split peels one small box a level: depth m."""
    lower, upper = [], []
    for i in range(1, m + 1):
        lower.append([float(i)] + [0.0] * (n - 1))
        upper.append([i + 0.1] + [1.0] * (n - 1))
        if i < m:
            for _ in range(3):
                lower.append([i + 0.5] + [0.0] * (n - 1))
                upper.append([m + 10.0] + [1.0] * (n - 1))
    return np.array(lower), np.array(upper), np.ones(len(lower), dtype=np.uint8)


def chain_of_depth(lib, n, depth):
    for m in range(max(2, depth - 5), depth + 6):
        lower, upper, finite = chain(n, m)
        tree, d = twin(lib, n, lower, upper, finite)
        if d == depth:
            return lower, upper, finite, tree
    raise AssertionError("no chain of depth %d" % depth)


# ------------------------------------------------------------------ 2. the twin on the synthetic sets (no GPU)

def check_tree(n, lower, upper, finite, tree):
    nodes, leaf_refs, inf_refs, bb_lower, bb_upper = tree
    assert len(nodes) >= 1 and (nodes["_pad"] == 0).all()
    assert np.array_equal(inf_refs, np.flatnonzero(finite == 0))
    fin = np.flatnonzero(finite != 0)
    if len(fin):
        assert np.array_equal(bb_lower, lower[fin].min(axis=0)) and np.array_equal(bb_upper, upper[fin].max(axis=0))
    else:
        assert (bb_lower == DBL_MAX).all() and (bb_upper == -DBL_MAX).all()
    seen = np.zeros(len(finite), dtype=bool)
    next_first = 0
    # preorder walk with the cell of every node
    stack = [(0, np.full(n, -np.inf), np.full(n, np.inf))]
    expect = 0
    while stack:
        me, clo, chi = stack.pop()
        assert me == expect         # a node, its left subtree, its right subtree: the walk meets the nodes in array order
        expect += 1
        k = nodes[me]
        if k["dim"] >= 0:
            assert k["left"] == me + 1 and k["right"] > k["left"] and k["num"] == 0 and k["first"] == 0
            d, pos = int(k["dim"]), float(k["boundary"])
            lhi, rlo = chi.copy(), clo.copy()
            lhi[d] = min(lhi[d], pos)
            rlo[d] = max(rlo[d], pos)
            stack.append((int(k["right"]), rlo, chi))
            stack.append((int(k["left"]), clo, lhi))
        else:
            assert k["dim"] == -1 and k["left"] == -1 and k["right"] == -1 and k["boundary"] == 0.0
            assert k["first"] == next_first
            ids = leaf_refs[k["first"]:k["first"] + k["num"]]
            next_first += int(k["num"])
            assert (finite[ids] != 0).all()
            seen[ids] = True
            # every regular item of a leaf reaches into the leaf's cell (the three-way test's EPSILON on either side)
            reg = ids[(lower[ids] <= upper[ids]).all(axis=1)]
            assert (lower[reg] <= chi + 1.01 * EPS).all() and (upper[reg] >= clo - 1.01 * EPS).all()
    assert expect == len(nodes) and next_first == len(leaf_refs)
    assert seen[fin].all() and not seen[finite == 0].any()


@pytest.mark.parametrize("n", ALL_DIMS)
def test_twin_on_synthetic_box_sets(host, n):
    sets = box_sets(n)
    assert ("big" in sets) == (n == 8)
    for name, (lower, upper, finite) in sets.items():
        tree, depth = twin_of(host, n, name)
        again, depth2 = twin(host, n, lower, upper, finite)
        assert same_tree(tree, again) and depth == depth2, name
        check_tree(n, lower, upper, finite, tree)
        if name in ("identical", "n0", "n1", "none_finite"):
            assert len(tree[0]) == 1 and depth == 1, name            # no valid split: one leaf holding its list
            assert tree[0][0]["num"] == int((finite != 0).sum())
        if name in ("separated", "inverted", "lattice", "big", "nonfinite", "n2"):
            assert len(tree[0]) >= 3, name
    assert len(sets["big"][2]) >= 2000 if n == 8 else True


def test_chain_sets_reach_the_depth_they_are_built_for(host):
    limit = kd_stack()
    for depth in (limit, limit + 1):
        lower, upper, finite, tree = chain_of_depth(host, 4, depth)
        check_tree(4, lower, upper, finite, tree)
        assert len(tree[0]) < 20000


# ------------------------------------------------------------------ 1. the twin is the reference's builder (no GPU)

# ndt_flatten_scene_with with the CPU twin as the kd builder (and, optionally, the CPU fit twin as the fitter), in a process of
# its own (scene programs draw from drand48): prints "KD <same|different> <builder calls>"
_FLATTEN_WITH_KD_TWIN = r"""
import ctypes as C, gzip, os, re, sys
host, so_path, dims, frame, config, threads, fixture, out, with_fit = sys.argv[1:10]
dims, frame, threads, config = int(dims), int(frame), int(threads), (None if sys.argv[5] == "-" else sys.argv[5].encode())
lib = C.CDLL(os.path.join(host, "libndt_host.so"), mode=C.RTLD_GLOBAL)
lib.ndt_host_fit_spheres.argtypes = [C.c_int, C.c_int64] + [C.c_void_p] * 5
lib.ndt_host_build_kdtree.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
FIT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
KD = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int)
calls = []
def fit(arg, d, n, first, pts, rad, cen, out_r, err, err_len):
    return lib.ndt_host_fit_spheres(d, n, first, pts, rad, cen, out_r)
def kd(arg, d, n, lower, upper, finite, tree, err, err_len):
    calls.append(n)
    return lib.ndt_host_build_kdtree(d, n, lower, upper, finite, tree)
fit_c, kd_c = FIT(fit), KD(kd)
lib.register_objects(b"objects")
so = C.CDLL(so_path)
frames = so.scene_frames(dims, config) if hasattr(so, "scene_frames") else 300
for i in range(frame + 1):
    scn = C.create_string_buffer(1 << 16)       # (a `scene`, generously)
    so.scene_setup(scn, dims, i, frames, config)
fb, err, stats, kstats = C.create_string_buffer(1 << 13), C.create_string_buffer(256), C.create_string_buffer(64), C.create_string_buffer(64)
lib.ndt_flatten_scene_with.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
assert lib.ndt_flatten_scene_with(scn, fb, err, 256, threads, C.cast(fit_c, C.c_void_p) if with_fit == "1" else None, None, stats,
                                  C.cast(kd_c, C.c_void_p), None, kstats) == 0, err.value
want = gzip.open(fixture, "rt").read()
lib.ndt_write_ndtscene(fb, re.search(r"^name (.*)$", want, re.M).group(1).encode(), out.encode())
sys.stdout.flush()
print("\nKD", "same" if open(out).read() == want else "different", len(calls))
"""


def _fixture_text(name):
    with gzip.open(os.path.join(GOLDEN, name + ".ndtscene.gz"), "rt") as f:
        return f.read()


@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built (make -C oracle ref)")
@pytest.mark.parametrize("with_fit", [0, 1])
@pytest.mark.parametrize("threads", [1, 7])
@pytest.mark.parametrize("name", ["c1_hypercube3d", "c3_random4d", "c5_hypercube6d", "zoo4d", "zoo5d_f2", "zoo12d"])
def test_flatten_with_the_twin_as_kd_builder_gives_the_references_scene(built, tmp_path, name, threads, with_fit):
    prog, dims, frame, config = SCENES[name]
    r = subprocess.run([sys.executable, "-c", _FLATTEN_WITH_KD_TWIN, HOST, os.path.join(REF_BIN, prog + ".so"), str(dims), str(frame),
                        config or "-", str(threads), os.path.join(GOLDEN, name + ".ndtscene.gz"), str(tmp_path / "out.ndtscene"),
                        str(with_fit)], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    said = [line.split() for line in r.stdout.splitlines() if line.startswith("KD ")][-1]
    assert said[1] == "same"
    assert int(said[2]) == 1            # the builder is called exactly once a frame


# ------------------------------------------------------------------ 3. refusals without a device

def test_build_kdtree_refuses_bad_arguments_without_a_device():
    lib = nh.load_library()
    lower, upper, finite = np.zeros((2, 16)), np.ones((2, 16)), np.ones(2, dtype=np.uint8)
    counts = nh.KdCounts()
    fake_ctx = C.c_void_p(0)            # NULL: every refusal below comes before the context is looked at

    def call(dims, n, lo, up, fin, cnt):
        return lib.ndt_hip_build_kdtree(fake_ctx, dims, n, lo, up, fin, cnt)

    ok = (lower.ctypes.data, upper.ctypes.data, finite.ctypes.data, C.addressof(counts))
    for dims in (2, 13, 0, -1):
        assert call(dims, 2, *ok) == fsmod.NDT_E_INVALID
        assert b"dims" in lib.ndt_hip_last_error()
    assert call(4, -1, *ok) == fsmod.NDT_E_INVALID
    assert b"n_items" in lib.ndt_hip_last_error()
    for k, arg in enumerate((b"lower", b"upper", b"finite", b"counts")):
        args = list(ok)
        args[k] = None
        assert call(4, 2, *args) == fsmod.NDT_E_INVALID
        assert arg in lib.ndt_hip_last_error()
    assert call(4, 2, *ok) == fsmod.NDT_E_INVALID
    assert b"ctx is NULL" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_kdtree_fetch(None, None, None, None, None, None) == fsmod.NDT_E_INVALID
    assert b"ctx" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_kd_launches(None) == 0


def _dump(driver, prog, dims, frame, out, config=None, extra=(), timeout=None):
    cmd = [driver, "-s", os.path.join(REF_BIN, prog + ".so"), "-d", str(dims), "-f", "%d:%d" % (frame, frame), "--dump-scene", out]
    if config:
        cmd += ["-u", config]
    return subprocess.run(cmd + list(extra), capture_output=True, text=True, cwd=os.path.dirname(out), timeout=timeout)


@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built (make -C oracle ref)")
def test_kd_flag_of_the_driver(built, tmp_path):
    """`--kd host` and no flag are the golden dump and say nothing about a GPU; `--kd fpga` is refused naming the flag"""
    out = str(tmp_path / "out.ndtscene")
    for extra in ([], ["--kd", "host"]):
        r = _dump(built, "random", 4, 0, out, extra=extra)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "on GPU" not in r.stdout
        assert open(out).read() == _fixture_text("c3_random4d")
        os.remove(out)
    bad = _dump(built, "random", 4, 0, out, extra=["--kd", "fpga"])
    assert bad.returncode != 0 and "--kd" in bad.stderr and not os.path.exists(out)


@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built (make -C oracle ref)")
def test_kd_gpu_without_a_device_fails_loudly(built, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    out = str(tmp_path / "out.ndtscene")
    for extra in (["--kd", "gpu"], ["--kd", "gpu", "--fit", "gpu"]):
        r = _dump(built, "random", 4, 0, out, extra=extra)
        assert r.returncode != 0
        assert "no HIP device" in (r.stderr + r.stdout)
        assert not os.path.exists(out)


# ------------------------------------------------------------------ 4. the device tree is the twin's

def launch_bound(depth):
    """The design's: a level is at most three launches -- score, plan, partition; the last level has no
    partition and a level without a node of two items no score."""
    return 3 * depth


@pytest.mark.gpu
@pytest.mark.parametrize("n", ALL_DIMS)
def test_device_tree_equals_the_twin(host, n):
    sets = box_sets(n)
    gpu = nh.NdtHip(0)
    bad = []
    try:
        # largest first, so that the smaller sets run in buffers a larger one grew
        for name in sorted(sets, key=lambda k: -len(sets[k][2])):
            lower, upper, finite = sets[name]
            want, depth = twin_of(host, n, name)
            got = gpu.build_kdtree(n, lower, upper, finite)
            launches, c = gpu.kd_launches(), gpu.kd_counts
            print("N = %d %-11s %5d items: %5d nodes, %6d leaf refs, depth %2d, %3d launches, %d buffers grown%s" % (
                n, name, len(finite), c.n_kd_nodes, c.n_leaf_refs, c.depth, launches, c.grows, "" if same_tree(got, want) else "  DIFFERENT"))
            if not same_tree(got, want):
                bad.append(name)
            assert c.depth == depth and launches == c.launches
            assert 0 < launches <= launch_bound(depth)
        # a larger set, then a smaller one, then the first again on the same context
        for name in ("separated", "n2", "inverted", "separated"):
            got = gpu.build_kdtree(n, *sets[name])
            if not same_tree(got, twin_of(host, n, name)[0]):
                bad.append(name + " (again)")
        # the items of a set in another order, against the twin on that order
        for name in ("inverted", "lattice", "nonfinite"):
            lower, upper, finite = sets[name]
            order = np.random.default_rng(n).permutation(len(finite))
            want, _ = twin(host, n, lower[order], upper[order], finite[order])
            if not same_tree(gpu.build_kdtree(n, lower[order], upper[order], finite[order]), want):
                bad.append(name + " (shuffled)")
    finally:
        gpu.close()
    assert bad == []


# ------------------------------------------------------------------ 5. refusals and growth on the device

@pytest.mark.gpu
def test_device_build_refuses_nan_and_too_deep_and_grows(host):
    limit = kd_stack()
    gpu = nh.NdtHip(0)
    try:
        # a fresh context sizes its buffers from the item count (ndt_kd.hip: room for 4 references an item + 1024); every level
        # of the 2 400 separated boxes holds each of them at least once, so the tree needs more, and the build has to grow them
        lower, upper, finite = box_sets(8)["big"]
        want, depth = twin_of(host, 8, "big")
        assert depth > 5
        got = gpu.build_kdtree(8, lower, upper, finite)
        print("big: %d nodes, depth %d, %d launches, %d buffers grown" % (len(got[0]), depth, gpu.kd_launches(), gpu.kd_counts.grows))
        assert gpu.kd_counts.grows >= 1
        assert same_tree(got, want)
        lo = lower.copy()
        lo[17, 3] = np.nan
        for a, b in ((lo, upper), (lower, lo)):
            with pytest.raises(nh.NdtHipError) as e:
                gpu.build_kdtree(8, a, b, finite)
            assert e.value.code == fsmod.NDT_E_INVALID and "NaN" in str(e.value)
        # as deep as the traversal stack holds: built; one level more: refused, nothing returned
        lower, upper, finite, want = chain_of_depth(host, 4, limit)
        assert same_tree(gpu.build_kdtree(4, lower, upper, finite), want)
        assert gpu.kd_counts.depth == limit and gpu.kd_launches() <= launch_bound(limit)
        lower, upper, finite, _ = chain_of_depth(host, 4, limit + 1)
        with pytest.raises(nh.NdtHipError) as e:
            gpu.build_kdtree(4, lower, upper, finite)
        assert e.value.code == fsmod.NDT_E_UNSUPPORTED and str(limit) in str(e.value)
        assert gpu.lib.ndt_hip_kdtree_fetch(gpu.ctx, None, None, None, None, None) == fsmod.NDT_E_STATE
        # the context is as good as before
        assert same_tree(gpu.build_kdtree(8, *box_sets(8)["lattice"]), twin_of(host, 8, "lattice")[0])
    finally:
        gpu.close()


# ------------------------------------------------------------------ 6. the reference's trees

@pytest.mark.gpu
@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built")
@pytest.mark.parametrize("fit", ["host", "gpu"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_kd_gpu_dump_is_the_references_scene_byte_for_byte(built, tmp_path, name, fit):
    prog, dims, frame, config = SCENES[name]
    out = str(tmp_path / "out.ndtscene")
    r = _dump(built, prog, dims, frame, out, config, extra=["--kd", "gpu", "--fit", fit, "-t", "7"], timeout=GPU_TIMEOUT)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    want = _fixture_text(name)
    assert open(out).read() == want
    said = BUILT.findall(r.stdout)
    assert len(said) == 1, r.stdout[-2000:]
    k, dev, launches = (int(x) for x in said[0])
    print("%s --fit %s: %s" % (name, fit, said[0]))
    assert k == int(re.search(r"^kdtree nodes (\d+) ", want, re.M).group(1)) and dev == 0 and launches >= 1
    assert ("bounding spheres on GPU" in r.stdout) == (fit == "gpu")


# ------------------------------------------------------------------ 7. to pixels

@pytest.mark.gpu
@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", ["c3_random4d", "c5_hypercube6d"])
def test_kd_gpu_to_pixels(built, tmp_path, name):
    prog, dims, frame, config = SCENES[name]
    g = golden(name)
    raw = str(tmp_path / "fb.f64")
    cmd = [built, "-s", os.path.join(REF_BIN, prog + ".so"), "-d", str(dims), "-f", "0", "-r", "%dx%d" % (g.width, g.height),
           "-l", str(g.depth), "--raw", raw, "--kd", "gpu", "--fit", "gpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=GPU_TIMEOUT)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    assert len(BUILT.findall(r.stdout)) == 1
    fb = np.fromfile(raw).reshape(g.height, g.width, 4)
    worst = float(np.abs(fb - g.data["fb"]).max())
    print("%s: max |--kd gpu --fit gpu - golden| = %.3g" % (name, worst))
    assert worst < 1e-9             # the bound of test_fit_gpu_to_pixels


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.isdir(REF_BIN), reason="oracle/_ref not built")
def test_kd_gpu_with_frames_in_flight(built, tmp_path):
    """frames 30 .. 33 of the 3-D hypercube with -j 2 (every worker builds on its own context): the images of `--kd host`"""
    images = []
    for kd, j in (("host", 1), ("gpu", 2)):
        d = tmp_path / ("img_%s" % kd)
        d.mkdir()
        cmd = [built, "-s", os.path.join(REF_BIN, "hypercube.so"), "-d", "3", "-r", "96x64", "-l", "16", "-f", "30:33", "-j", str(j), "--kd", kd]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(d), timeout=GPU_TIMEOUT)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        assert len(BUILT.findall(r.stdout)) == (4 if kd == "gpu" else 0)
        files = sorted(p for p in (d / "images").rglob("*.ppm"))
        assert len(files) == 4
        images.append([p.read_bytes() for p in files])
    assert images[0] == images[1] and len(set(images[0])) == 4
