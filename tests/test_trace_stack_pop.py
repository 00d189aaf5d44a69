"""The traversal stack of trace_kd ("What a stack entry holds"; section 9, round 16).  An entry of the stack is
{far child, tp}: a pop takes the child and its gate from the entry and makes the child's `tu` from the entry BELOW -- `tp + EPS` of
the nearest ancestor at which the walk went near with both children pending -- or takes the root interval's `tu` where nothing is
below.  That only holds while every step that tightens `tu` leaves an entry, so a node whose far side a closer hit already rules
out is pushed too (and dropped by the same test when it is popped).  None of it may change a bit of any answer.

Known-answer rays.  The rays are chosen on the CPU with a replay of the walk (kd_node_intersect, kd-tree.c:482-568, on the explicit
stack of trace_kd), fed with the distance at which the oracle hits every item on its own, and the test asserts that they contain

  * `root`   an answer found under a far child that was popped from a stack with nothing below (its `tu` is the root's),
  * `nested` a walk that holds three entries at once and enters a far child popped with entries below (its `tu` from the entry below),
  * `closer` a node where both children are pending while the ray already holds a hit closer than the plane: the push that is new,
  * `full`   a walk whose stack holds as many entries as the tree is deep (kd_depth - 1: every inner node of a deepest path),

each with every comparison that involves the running hit distance decided by more than MARGIN, with and without the item-set tier's
skipping of subtrees whose items have all been visited.  The device's objects, hit points and normals are the oracle's bit for bit,
in calls of 1, 63, 64 and 65 rays.

No ray can be `full` in a tree of the reference's builder: its first planes lie outside the root box (2 EPS below its lower bound:
the ray's interval ends before it meets them), and on the fixtures the fullest first descent leaves kd_depth - 3 to kd_depth - 5
entries.  The `ladder_` scenes are the fixtures' objects under a tree made here from their bounding spheres: two planes per
dimension inside the box, one deep path (kd_depth = 2 N + 1), every leaf holding the items whose sphere's box meets its cell, in
ascending order -- a superset of what lies in the cell, which is all a kd-tree needs; the oracle walks the same tree.  Their rays
meet the 2 N planes in the order leaf to root, at distances set 0.05 apart, and leave an entry at every one.

Frames.  -l 3 on the 3-D and the 4-D fixture at 16x9 and 65x33: the per-bounce pipeline with light_overlap 0 and 1, the frame
kernel, and a context whose small first pool overflows and retries -- all the same bytes and ray counts; against the oracle within
the bound test_trace_batch_head.py derives (96 ulps of max(1, largest value): the device takes acos / pow / sin / cos from ocml, the
oracle from glibc) and with equal ray counts.

Needs a real MI355X: run with `pytest -m gpu`.  (test_replay_finds_every_case runs on the CPU.)
"""
import math
import os

import numpy as np
import pytest

from conftest import golden, GOLDEN

ORACLE_ULPS = 96        # device frame against the oracle's, in ulps of max(1, largest colour value): test_trace_batch_head.py
EPS, EPS2 = 1e-4, 1e-8
DBL_MAX = float(np.finfo(np.float64).max)
MARGIN = 1e-7           # a witness ray decides every comparison against its running hit distance by more than this
# 3-D, 4-D and 6-D, zoo and benchmark scenes: the item-set tier, the register-mask tier and the global-memory tier
# (items: 15, 27, 14, 40, 81, 243, 14, 729)
# Which kernel a scene's rays run in, and what trace_walk_steps (ndt_kernels.hip) gives it today -- 1 the stack entry, 2 the leaf
# sets; ndt_hip_trace_rays launches the plain variants, the frames below the PRIM ones for their primaries as well:
#   zoo3d_mirror, c1_hypercube3d   3-D k_trace<1, true, true, false>   1 + 2        (frames: <1, true, true, true> 1 + 2)
#   zoo4d, c3_random4d             4-D k_trace<1, true, true, false>   1 + 2        (frames: <1, true, true, true> 1 + 2)
#   c5_hypercube4d                 4-D k_trace<4, true, true, false>   neither: the parent's kernel (it spills 4 -> 8 with 1)
#   c5_hypercube5d                 5-D k_trace<4, true, true, false>   1
#   zoo6d                          6-D k_trace<1, true, true, false>   1 + 2
#   c5_hypercube6d                 6-D k_trace<0, false, false, false> neither: the global-memory tier, scratch stack
# and a ladder_ scene its fixture's.  So the new entry is popped by 3-D, 4-D, 5-D and 6-D kernels, item sets and register masks;
# the scenes on unchanged kernels hold those to the same answers.  With NDT_TRACE_LSTACK=0 in the environment the item-set scenes
# run k_trace<1, true, false, false> (scratch stack, leaf sets).  Whoever changes the gate's table: keep a scene on every setting.
SCENES = ["zoo3d_mirror", "c1_hypercube3d", "zoo4d", "c3_random4d", "c5_hypercube4d", "c5_hypercube5d", "zoo6d", "c5_hypercube6d",
          "ladder_zoo3d_mirror", "ladder_c3_random4d", "ladder_c5_hypercube4d", "ladder_zoo6d", "ladder_c5_hypercube6d"]
CASES = ("root", "nested", "closer", "full")


def required(name):
    return ("full", "nested") if name.startswith("ladder_") else ("root", "nested", "closer")
N_RAYS = 130            # per scene: two calls of 65, three of 63 / 64, 130 of 1


def fresh(name):
    """A copy of a fixture's scene of its own (golden() shares its scene)."""
    from ndt_amd import load_scene
    return load_scene(os.path.join(GOLDEN, name + ".ndtscene.gz"))


def ladder(fs):
    """fs under a kd-tree of one deep path: planes c + 0.3 half of dimension 0 .. N - 1, then c - 0.2 half of 0 .. N - 1, the path
    through the lower side of each; fs.ladder_rays: rays that meet plane k of the path (root first) at distance 1 - 0.05 k."""
    d = fs.dims
    lo, hi = fs.vec(fs.bb["lower"]), fs.vec(fs.bb["upper"])
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    n_items = max(fs.leaf_refs) + 1
    centre = np.array([fs.vec(fs.objects[i]["bounds_center_off"]) for i in range(n_items)])
    radius = np.array([fs.objects[i]["bounds_radius"] for i in range(n_items)])
    anywhere = ~((radius > 0) & np.isfinite(radius))        # (no sphere: in every leaf)
    planes = [(j, float(c[j] + 0.3 * half[j])) for j in range(d)] + [(j, float(c[j] - 0.2 * half[j])) for j in range(d)]
    nodes, refs = [], []

    def leaf(a, b):
        ids = [i for i in range(n_items) if anywhere[i] or ((centre[i] + radius[i] >= a).all() and (centre[i] - radius[i] <= b).all())]
        nodes.append({"dim": -1, "boundary": 0.0, "left": -1, "right": -1, "num": len(ids), "first": len(refs)})
        refs.extend(ids)

    a, b = lo.copy(), hi.copy()
    for dim, bound in planes:
        # preorder: the inner node, its left subtree (the rest of the path), its right leaf
        nodes.append({"dim": dim, "boundary": bound, "left": len(nodes) + 1, "right": -1, "num": 0, "first": 0})
    leaf_cells = []
    for dim, bound in planes:
        ra = a.copy()
        ra[dim] = bound
        leaf_cells.append((ra, b.copy()))
        b[dim] = bound
    leaf(a, b)
    for k in range(len(planes) - 1, -1, -1):
        nodes[k]["right"] = len(nodes)
        leaf(*leaf_cells[k])
    fs.kd_nodes, fs.leaf_refs = nodes, refs
    fs._struct = None
    fs.finalize()
    rays = []
    rng = np.random.default_rng(d)
    for k in range(12):
        t = [1.0 - 0.05 * i for i in range(2 * d)]
        if k:
            t = sorted(rng.uniform(0.2, 1.0, 2 * d) + 0.05 * np.arange(2 * d), reverse=True)      # (still 0.05 apart or more)
        v = np.array([(planes[j][1] - planes[d + j][1]) / (t[j] - t[d + j]) for j in range(d)])
        o = np.array([planes[d + j][1] - v[j] * t[d + j] for j in range(d)])
        rays.append(np.concatenate([o, v / np.sqrt((v * v).sum()), [-1.0]]))
    fs.ladder_rays = rays
    return fs


_scenes = {}


def scene_of(name):
    if name not in _scenes:
        _scenes[name] = ladder(fresh(name[7:])) if name.startswith("ladder_") else golden(name).scene
    return _scenes[name]


def counts(st):
    return (st.rays_primary, st.rays_secondary, st.rays_shadow, st.rays_ref_equiv)


def same_bits(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %d values differ" % (what, int((a != b).sum()))


# ------------------------------------------------------------------ the walk, replayed

def inv_of(x):
    if 0.0 <= x < EPS2:
        return 1.0 / EPS2
    if -EPS2 < x <= 0.0:
        return -1.0 / EPS2
    return 1.0 / x


def root_interval(lo, hi, o, v):
    """aabb_intersect of the root box (kd-tree.c:84-127) as trace_kd does it: (tl, tu) or None."""
    tl, tu = -DBL_MAX, DBL_MAX
    for i in range(len(lo)):
        if not abs(v[i]) < EPS2:
            a, b = (lo[i] - o[i]) / v[i], (hi[i] - o[i]) / v[i]
            if a > b:
                a, b = b, a
            tl, tu = max(tl, a), min(tu, b)
            if tu < -EPS:
                return None
    tl -= EPS
    tu += EPS
    return (tl, tu) if tu >= -EPS and tl <= tu else None


def tree_of(fs):
    """(nodes, lists, depth, below): the kd nodes, every leaf's item list, the depth of the deepest leaf (root = 1), and the set of
    items below every node."""
    nodes = fs.kd_nodes
    lists = [fs.leaf_refs[k["first"]:k["first"] + k["num"]] if k["dim"] < 0 else [] for k in nodes]
    below = [None] * len(nodes)
    depth = 0
    todo = [(0, 1, False)]
    while todo:
        n, d, done = todo.pop()
        k = nodes[n]
        if k["dim"] < 0:
            below[n] = frozenset(lists[n])
            depth = max(depth, d)
        elif done:
            below[n] = below[k["left"]] | below[k["right"]]
        else:
            todo += [(n, d, True), (k["left"], d + 1, False), (k["right"], d + 1, False)]
    return nodes, lists, depth, below


def replay(tree, lo, hi, o, v, dist, prune):
    """kd_node_intersect on trace_kd's stack for one ray with dist_limit < 0.  dist[item]: the distance at which the ray hits the
    item on its own, or None.  prune: subtrees whose items have all been visited are not entered (the item-set tier).  Returns
    what the walk did, or None for a ray that misses the root box."""
    nodes, lists, depth, below = tree
    iv = root_interval(lo, hi, o, v)
    if iv is None or not nodes:
        return None
    v_inv = [inv_of(x) for x in v]
    lt, winner, won_under = DBL_MAX, -1, ""
    visited = set()
    stack = []                      # (far child, tp)
    res = dict(height=0, closer=0, nested=0, margin=math.inf, pops=0, dropped=0)
    node, ntl, ntu = 0, iv[0], iv[1]
    under = ""                      # how the walk got `tu` of where it stands: "root" (popped, nothing below), "below" (popped), else ""
    st = 1

    def against_lt(x):
        if lt < DBL_MAX:
            res["margin"] = min(res["margin"], abs(lt - x))

    while True:
        if st == 0:
            if not stack:
                break
            node, a = stack.pop()
            ntu = iv[1] if not stack else stack[-1][1] + EPS
            ntl = a - EPS
            against_lt(a)
            res["pops"] += 1
            if lt > a and not ntu < 0.0:
                st = 1
                under = "below" if stack else "root"
                res["nested"] += bool(stack)
            else:
                res["dropped"] += 1
            continue
        if ntu < 0.0:
            st = 0
            continue
        k = nodes[node]
        if prune and not (below[node] - visited):
            st = 0
            continue
        if k["dim"] < 0:
            min_dist, best = -1.0, -1
            for item in lists[node]:
                if item in visited:
                    continue
                visited.add(item)
                d = dist[item]
                if d is not None and d > EPS and (d + EPS < min_dist or min_dist < 0):
                    min_dist, best = d, item
            if min_dist >= 0:
                against_lt(min_dist)
                if min_dist < lt:
                    lt, winner, won_under = min_dist, best, under
            st = 0
            continue
        dim = k["dim"]
        swap = v_inv[dim] < EPS2
        near, far = (k["right"], k["left"]) if swap else (k["left"], k["right"])
        tp = (k["boundary"] - o[dim]) * v_inv[dim]
        against_lt(ntl)
        alive = lt > ntl
        near_only = ntu < tp - EPS and alive
        far_only = (not near_only) and ntl > tp + EPS and alive
        both = not near_only and not far_only
        if both and alive:
            against_lt(tp)
            res["closer"] += not lt > tp
            stack.append((far, tp))
            res["height"] = max(res["height"], len(stack))
            ntu = tp + EPS
            under = ""
            node = near
        elif near_only:
            node = near
        elif far_only:
            node = far
        else:
            st = 0
    res.update(lt=lt, winner=winner, root=won_under == "root", full=res["height"] == depth - 1)
    return res


def item_distances(oracle, name, rays):
    """dist[ray][item]: the distance at which the oracle hits the item when the tree holds nothing else (one leaf, one item)."""
    fs = fresh(name[7:] if name.startswith("ladder_") else name)
    d = fs.dims
    n_items = max(fs.leaf_refs) + 1
    out = [[None] * n_items for _ in range(len(rays))]
    for item in range(n_items):
        fs.kd_nodes = [{"dim": -1, "boundary": 0.0, "left": -1, "right": -1, "num": 1, "first": 0}]
        fs.leaf_refs = [item]
        fs.inf_refs = []
        fs._struct = None
        fs.finalize()
        obj, hit, _ = oracle.trace(fs, rays)
        for r in np.flatnonzero(obj >= 0):
            s = 0.0
            for i in range(d):
                s += (rays[r, i] - hit[r, i]) * (rays[r, i] - hit[r, i])
            out[r][item] = math.sqrt(s)
    return out


def candidate_rays(fs, tree, seed):
    """Rays with dist_limit -1: from outside the root box at points in it, from inside it, and from the cells of the deepest leaves
    across as many of their ancestors' planes as one direction can cross."""
    rng = np.random.default_rng(seed)
    nodes, lists, depth, below = tree
    d = fs.dims
    lo, hi = fs.vec(fs.bb["lower"]), fs.vec(fs.bb["upper"])
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rays = []

    def add(o, v):
        v = v / np.sqrt((v * v).sum())
        rays.append(np.concatenate([o, v, [-1.0]]))

    rays += list(getattr(fs, "ladder_rays", []))
    for k in range(900):
        o = c + rng.normal(size=d) / np.sqrt(d) * (2.0 + (k % 3)) * np.sqrt((half * half).sum())
        add(o, c + rng.uniform(-0.9, 0.9, d) * half - o)
    for k in range(200):
        add(c + rng.uniform(-0.95, 0.95, d) * half, rng.normal(size=d))
    # cells of the deepest leaves
    cells = []
    todo = [(0, 1, lo.copy(), hi.copy(), [])]
    while todo:
        n, dep, a, b, path = todo.pop()
        k = nodes[n]
        if k["dim"] < 0:
            if dep == depth:
                cells.append((a, b, path))
            continue
        la, lb, ra, rb = a.copy(), b.copy(), a.copy(), b.copy()
        lb[k["dim"]] = k["boundary"]
        ra[k["dim"]] = k["boundary"]
        todo.append((k["left"], dep + 1, la, lb, path + [(k["dim"], k["boundary"], -1.0)]))
        todo.append((k["right"], dep + 1, ra, rb, path + [(k["dim"], k["boundary"], 1.0)]))
    # A first descent that leaves an entry at every inner node: the cell on the near side of every ancestor's plane, and the
    # planes met in the order leaf to root (an ancestor met later than one above it is `near only`: no entry).  Sampled per cell,
    # tested on the planes alone -- the entries of a first descent do not depend on what the ray hits.
    for a, b, path in cells:
        m = 4096
        o = a + rng.uniform(0.02, 0.98, (m, d)) * (b - a)
        sign = np.zeros(d)
        for dim, _, side in path:
            sign[dim] -= side
        sign = np.where(sign == 0.0, rng.choice([-1.0, 1.0], d), np.sign(sign))
        v = sign * np.exp(rng.uniform(np.log(1e-3), 0.0, (m, d)))
        v /= np.sqrt((v * v).sum(axis=1))[:, None]
        t_lo, t_hi = (lo - o) / v, (hi - o) / v
        tl = np.minimum(t_lo, t_hi).max(axis=1) - EPS
        ntu = np.maximum(t_lo, t_hi).min(axis=1) + EPS
        ok = np.ones(m, dtype=bool)
        for dim, bound, side in path:
            tp = (bound - o[:, dim]) / v[:, dim]
            ok &= (sign[dim] == -side) & ~(ntu < tp - 2 * EPS) & ~(tl > tp + 2 * EPS)
            ntu = tp + EPS
        for r in np.flatnonzero(ok)[:6]:
            add(o[r], v[r])
    for k in range(400):
        a, b, path = cells[k % len(cells)]
        add(a + rng.uniform(0.05, 0.95, d) * (b - a), rng.normal(size=d))
    return np.array(rays)


_cases = {}


def case(oracle, name):
    """(scene, rays, oracle's answers, which rays are witnesses of what), made once per scene."""
    if name in _cases:
        return _cases[name]
    fs = scene_of(name)
    d = fs.dims
    tree = tree_of(fs)
    lo, hi = fs.vec(fs.bb["lower"]), fs.vec(fs.bb["upper"])
    cand = candidate_rays(fs, tree, 15)
    dist = item_distances(oracle, name, cand)
    obj, hit, nrm = oracle.trace(fs, cand)
    found = {c: [] for c in CASES}
    stats = dict(rays=0, pops=0, dropped=0, height=0)
    for r, ray in enumerate(cand):
        o, v = [float(x) for x in ray[:d]], [float(x) for x in ray[d:2 * d]]
        runs = [replay(tree, lo, hi, o, v, dist[r], prune) for prune in (False, True)]
        if runs[0] is None:
            continue
        stats["rays"] += 1
        stats["pops"] += runs[0]["pops"]
        stats["dropped"] += runs[0]["dropped"]
        if min(run["margin"] for run in runs) <= MARGIN:
            continue
        # the replay's answer is the oracle's: the item it ends on is hit, alone, at the oracle's hit point of the whole scene
        # (a ray that ends on nothing in the tree compares nothing with its hit distance)
        w = runs[0]["winner"]
        if runs[1]["winner"] != w:
            continue
        s = 0.0
        for i in range(d):
            s += (ray[i] - hit[r, i]) * (ray[i] - hit[r, i])
        if w >= 0 and (obj[r] < 0 or math.sqrt(s) != runs[0]["lt"]):
            continue
        stats["height"] = max(stats["height"], min(run["height"] for run in runs))
        if w >= 0 and all(run["root"] for run in runs):
            found["root"].append(r)
        if all(run["height"] >= 3 and run["nested"] >= 1 for run in runs):
            found["nested"].append(r)
        if all(run["closer"] >= 1 for run in runs):
            found["closer"].append(r)
        if all(run["full"] for run in runs):
            found["full"].append(r)
    keep = []
    for c in CASES:
        keep += [r for r in found[c][:8] if r not in keep]
    rest = [r for r in range(len(cand)) if r not in keep]
    step = max(1, len(rest) // (N_RAYS - len(keep)))
    keep = sorted(keep + rest[::step][:N_RAYS - len(keep)])
    witnesses = {c: [keep.index(r) for r in found[c][:8]] for c in CASES}
    sel = np.array(keep)
    _cases[name] = (fs, cand[sel], (obj[sel], hit[sel], nrm[sel]), witnesses, tree[2], stats)
    return _cases[name]


@pytest.mark.parametrize("name", SCENES)
def test_replay_finds_every_case(oracle, name):
    """On the CPU, the oracle alone: the rays of every scene hold a witness of each case (`full`: the ladder scenes), 130 rays in
    all, at least 32 of which hit something."""
    fs, rays, (obj, hit, nrm), witnesses, depth, stats = case(oracle, name)
    print("%s: kd depth %d, highest stack %d; replay of %d candidate rays: %.2f pops a ray, %.2f of them dropped; witnesses %s"
          % (name, depth, stats["height"], stats["rays"], stats["pops"] / stats["rays"], stats["dropped"] / stats["rays"],
             {c: len(w) for c, w in witnesses.items()}))
    assert len(rays) == N_RAYS and (obj >= 0).sum() >= 32
    for c in required(name):
        assert witnesses[c], "no ray of %s is a witness of the case `%s`" % (name, c)


@pytest.fixture(scope="module")
def gpu():
    from ndt_amd.hip import NdtHip
    ctx = NdtHip(0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 63, 64, 65])
@pytest.mark.parametrize("name", SCENES)
def test_known_answer_rays(gpu, oracle, name, batch):
    """ndt_hip_trace_rays, `batch` rays a call: the oracle's object, hit point and normal, bit for bit."""
    fs, rays, (obj, hit, nrm), witnesses, depth, stats = case(oracle, name)
    gpu.upload_scene(fs)
    got = [gpu.trace_rays(rays[k:k + batch]) for k in range(0, len(rays), batch)]
    g_obj, g_hit, g_nrm = (np.concatenate([g[i] for g in got]) for i in range(3))
    bad = np.flatnonzero(g_obj != obj)
    assert bad.size == 0, "objects differ at rays %s (witnesses: %s)" % (bad[:8], witnesses)
    same_bits(hit, g_hit, "%s hit points, batch %d" % (name, batch))
    same_bits(nrm, g_nrm, "%s normals, batch %d" % (name, batch))


# ------------------------------------------------------------------ frames

@pytest.mark.gpu
@pytest.mark.parametrize("size", [(16, 9), (65, 33)])
@pytest.mark.parametrize("name", ["c1_hypercube3d", "c3_random4d"])
def test_frames(gpu, oracle, name, size):
    """-l 3: per-bounce pipeline with light_overlap 0 and 1, the frame kernel, and the small-pool retry: one frame, the oracle's
    within ORACLE_ULPS, the oracle's ray counts."""
    from ndt_amd.hip import NdtHip
    fs = golden(name).scene
    w, h = size
    want, wst = oracle.render(fs, w, h, 3)
    frames = []
    try:
        for pipeline, overlap in ((1, 0), (1, 1), (2, 1)):
            gpu.set_option("pipeline", pipeline)
            gpu.set_option("light_overlap", overlap)
            gpu.upload_scene(fs)
            out, st = gpu.render(w, h, 3)
            frames.append(("pipeline %d light_overlap %d" % (pipeline, overlap), out, st))
    finally:
        gpu.set_option("light_overlap", 1)
        gpu.set_option("pipeline", 0)
    small = NdtHip(0)
    try:
        small.set_option("pipeline", 1)
        small.set_option("test_small_pool", 1)
        small.upload_scene(fs)
        out, st = small.render(w, h, 3)
        frames.append(("small pool", out, st))
        out, st = small.render(w, h, 3)
        frames.append(("the frame after the retry", out, st))
    finally:
        small.close()
    tol = ORACLE_ULPS * np.finfo(np.float64).eps * max(1.0, float(np.abs(want).max()))
    for what, out, st in frames:
        what = "%s %dx%d %s" % (name, w, h, what)
        diff = float(np.abs(out - want).max())
        print("%s: max |device - oracle| = %g, %d of %d values differ (bound %g)" % (what, diff, int((out != want).sum()), out.size, tol))
        assert diff <= tol, "%s: max abs diff %g, bound %g" % (what, diff, tol)
        assert counts(st) == counts(wst), what
        same_bits(frames[0][1], out, what + " against " + frames[0][0])
