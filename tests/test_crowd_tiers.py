"""Known-answer CROWDS: every object type in every family of trace kernels, 3-D to 12-D (tests/golden/crowd*, made by
tests/golden/make_golden_crowd.py from the compiled reference; the scene program is tests/scenes/parity_crowd.c).

The trace code picks a kernel family per scene: item sets (at most 64 items), a register mask (65 .. 256 items and a trace
section of at most 64 KB), global memory ("tier 1": more than 256 items OR a larger trace section).  The zoo scenes, the only
ones with all nine types, have 13 to 15 items: the item-set family.  A crowd is a floor and K - 1 small objects that cycle
through the other eight types on a jittered lattice, and K takes it where it is wanted:

  crowd{N}d_r   register mask.  K is the largest (of at most 256) whose trace section stays within 64 KB: three mask words
                up to 7-D.  From 8-D on no K of 130 or more fits -- an item costs about 0.5 KB there, 0.7 KB in 12-D -- so K is
                the largest that does, 126 down to 94, and the mask has two words.  Only the 3-D one keeps its hcubes: from 4-D
                on they leave room for fewer than 130 items (126 in 4-D) or do not fit at all (5-D: two hcubes' face boxes
                alone are over 100 KB).
  crowd{N}d_g   global memory, K = 320: five mask words, item boxes.  Two hcubes up to 6-D, one in 7-D and 8-D, none from
                9-D on (an hcube nests every m-face: 16 866 in 9-D, 52 904 in 10-D, a 1 MB scene file; zoo9d and zoo10d keep
                covering that intersector in the item-set family).  A leaf that holds an hcube cannot be scanned through LDS:
                these run the fallback.
  crowd{N}d_gn  N <= 8: the same without the hcubes, so that the coherent leaf scan runs at those N too.
  crowd{N}d_l   N = 10, 12: K = 200 and a trace section over 64 KB: tier 1 with four mask words and no item boxes.

The coherent leaf scan stages a record of n + 2 + max_param_words words and needs it within 128 (ndt_blob.hip).  The largest
record of a crowd is the hcylinder's, n + 1 + (n - 2)(n + 3) words: with the sphere that is 127 words in 10-D and 151 in
11-D.  So not all nine types fit at 12-D, and the crowds themselves stand on both sides of that switch -- crowd10d_g and
crowd10d_l one word under the limit, crowd11d_g and the 12-D ones over it (test_record_limit_on_both_sides); no further
scene is made for it.

Where the families MEET -- 64 | 65, 128 | 129, 192 | 193 and 256 | 257 items, mask word 3, a section on either side of 64 KB, a
traversal stack that no longer fits LDS, leaf lists of 63, 64 and 65 entries, lists that do not ascend -- is the business of
tests/test_trace_edges.py, which also renders the _r cases of this module: here they only go through trace_rays.
"""
import re

import numpy as np
import pytest

from conftest import golden
from ndt_amd.flat_scene import OBJ_TYPES, OBJ_TYPE_ID
from test_aimed_rays import (A, B, C, D, E, F, CLASSES, HAS_CLASS_B, MIN_PER_CLASS, MIN_PER_TYPE, TOL_SPEC, TOL_TIGHT, answered_types,
                             coverage, ref_dist, same_answers, scene_types)


def case(dims, items, hcubes, tier, words):
    return dict(dims=dims, items=items, hcubes=hcubes, tier=tier, words=words)


# name -> N, K, hcubes in it, and the tier and mask words the scene is built to reach
CASES = {}
for _n, _k in {3: 176, 4: 158, 5: 155, 6: 142, 7: 131, 8: 126, 9: 118, 10: 107, 11: 101, 12: 94}.items():
    CASES["crowd%dd_r" % _n] = case(_n, _k, 2 if _n == 3 else 0, 0, (_k + 63) // 64)
for _n in range(3, 13):
    CASES["crowd%dd_g" % _n] = case(_n, 320, 2 if _n <= 6 else 1 if _n <= 8 else 0, 1, 5)
    if _n <= 8:
        CASES["crowd%dd_gn" % _n] = case(_n, 320, 0, 1, 5)
for _n in (10, 12):
    CASES["crowd%dd_l" % _n] = case(_n, 200, 0, 1, 4)
ALL = list(CASES)
TIER1 = [c for c in ALL if CASES[c]["tier"] == 1]
REGISTER = [c for c in ALL if CASES[c]["tier"] == 0]

MIN_PER_WORD = 16
MIN_EARLY_ENDS = 64
LEAF_HISTORY = 4            # ndt_ctx.hpp: the default number of {leaf, cut} pairs a ray keeps before it spills into the slab


def leaf_items(fs, k):
    node = fs.kd_nodes[k]
    return fs.leaf_refs[node["first"]:node["first"] + node["num"]]


def leaves_on_segment(fs, o, v, limit):
    """The non-empty kd leaves whose cell the segment o + t v, 0 <= t <= limit (a limit <= 0: the whole ray) may touch: a plain
    walk that descends both children where the segment crosses the boundary, the reference's EPSILON to either side."""
    lo, hi = fs.vec(fs.bb["lower"]), fs.vec(fs.bb["upper"])
    t0, t1 = 0.0, limit if limit > 0 else np.inf
    for i in range(fs.dims):
        if v[i] == 0.0:
            if o[i] < lo[i] or o[i] > hi[i]:
                return []
            continue
        a, b = sorted(((lo[i] - o[i]) / v[i], (hi[i] - o[i]) / v[i]))
        t0, t1 = max(t0, a), min(t1, b)
    if t0 > t1:
        return []
    out, stack = [], [0]
    while stack:
        k = stack.pop()
        node = fs.kd_nodes[k]
        if node["dim"] < 0:
            if node["num"] > 0:
                out.append(k)
            continue
        i = node["dim"]
        xa, xb = o[i] + t0 * v[i], o[i] + t1 * v[i]
        if min(xa, xb) <= node["boundary"] + 1e-4:
            stack.append(node["left"])
        if max(xa, xb) >= node["boundary"] - 1e-4:
            stack.append(node["right"])
    return out


_walks = {}


def walks(name):
    """Per ray of the fixture: the leaves its segment may touch (computed once per case)."""
    if name not in _walks:
        g = golden(name)
        d = g.scene.dims
        _walks[name] = [leaves_on_segment(g.scene, r[:d], r[d:2 * d], r[2 * d]) for r in g.data["kat_in"]]
    return _walks[name]


# ------------------------------------------------------------------------------------------------ CPU

def test_case_table():
    assert len(ALL) == 28 and len(REGISTER) == 10 and len(TIER1) == 18
    for name, c in CASES.items():
        g = golden(name)
        assert (g.scene.dims, g.scene.n_items, g.meta["items"]) == (c["dims"], c["items"], c["items"]), name
        assert sum(o["type"] == OBJ_TYPE_ID["hcube"] for o in g.scene.objects[:g.scene.n_items]) == c["hcubes"], name
        assert (g.scene.n_items + 63) // 64 == c["words"] and (c["words"] > 4) == (c["items"] > 256), name
        assert g.meta["scene_file"] == name + ".ndtscene.gz"
        # an hcube only where its nested faces leave the scene file small; both hcubes in different mask words
        at = [i for i in range(g.scene.n_items) if g.scene.objects[i]["type"] == OBJ_TYPE_ID["hcube"]]
        assert len({i >> 6 for i in at}) == len(at)
        # types interleaved in item order: every full mask word holds every type of the scene
        types = scene_types(g)
        for w in range(g.scene.n_items // 64):
            here = {g.scene.objects[i]["type"] for i in range(64 * w, 64 * w + 64)}
            assert here >= set(types) - {OBJ_TYPE_ID["hplane"], OBJ_TYPE_ID["hcube"]}, (name, w)
        # the four kinds of light, glass and mirrors
        assert sorted(l["type"] for l in g.scene.lights) == [0, 1, 2, 3]
        small = g.scene.objects[1:g.scene.n_items]
        assert 0.05 < np.mean([o["transparent"] != 0 for o in small]) < 0.25
        assert 0.05 < np.mean([o["red_r"] > 0.4 for o in small]) < 0.25


@pytest.mark.parametrize("name", ALL)
def test_fixture_layout(name):
    g = golden(name)
    d = g.scene.dims
    rays, want = g.data["kat_in"], g.data["kat_out"]
    n = len(rays)
    assert rays.shape == (n, 2 * d + 1) and want.shape == (n, 2 * d + 2) and n == g.meta["rays"]
    item, cls, sub = g.data["aim_item"], g.data["aim_class"], g.data["aim_sub"]
    assert item.shape == cls.shape == sub.shape == (n,)
    assert item.min() >= 0 and item.max() < g.scene.n_items and cls.min() == 0 and cls.max() == 5
    assert set(item.tolist()) == set(range(g.scene.n_items))              # every kd item has rays of its own
    assert np.abs(np.linalg.norm(rays[:, d:2 * d], axis=1) - 1.0).max() < 1e-12
    # every item has classes A and F; the full items (at least 24 of a type, or all of it) have B .. E too
    full = set(g.meta["full_items"])
    by_type = {}
    for i in range(g.scene.n_items):
        by_type.setdefault(g.scene.objects[i]["type"], []).append(i)
    for ty, ids in by_type.items():
        assert len(full & set(ids)) >= min(24, len(ids)), OBJ_TYPES[ty]
    for cl in (A, F):
        assert set(item[cls == cl].tolist()) == set(range(g.scene.n_items))
    assert set(item[cls == D].tolist()) == set(item[cls == E].tolist()) == full
    assert set(item[cls == C].tolist()) <= full and len(set(item[cls == C].tolist())) >= 0.9 * len(full)
    # class C: the limits of one class-A ray stand right behind it, same origin and direction: limit 0, then -- if limit 0 was
    # answered by another, farther object that the scan meets first -- five limits around THAT object's distance, then five
    # around the distance t of the ray's own (nearest) answer, t itself included, in the reference's arithmetic
    firsts = np.flatnonzero((cls == C) & (sub == 0))
    around_first = 0
    for first in firsts:
        parent = first - 1
        assert cls[parent] == A and want[parent, 0] == 1.0 and rays[first, 2 * d] == 0.0
        k = first + 1
        if sub[k] >= 6:
            assert want[first, 0] == 1.0 and want[first, 1] != want[parent, 1]
            tx = ref_dist(rays[first, :d], want[first, 2:2 + d])
            assert tx > ref_dist(rays[parent, :d], want[parent, 2:2 + d])
            assert np.array_equal(rays[k:k + 5, 2 * d], [tx * (1 - 1e-3), tx * (1 + 1e-3), np.nextafter(tx, 0.0), np.nextafter(tx, np.inf), tx])
            assert sub[k:k + 5].tolist() == [6, 7, 8, 9, 10] and (cls[k:k + 5] == C).all()
            k += 5
            around_first += 1
        t = ref_dist(rays[parent, :d], want[parent, 2:2 + d])
        assert np.array_equal(rays[k:k + 5, 2 * d], [t * (1 - 1e-3), t * (1 + 1e-3), np.nextafter(t, 0.0), np.nextafter(t, np.inf), t])
        assert sub[k:k + 5].tolist() == [1, 2, 3, 4, 5] and (cls[k:k + 5] == C).all()
        assert np.array_equal(rays[first:k + 5, :2 * d], np.repeat(rays[parent:parent + 1, :2 * d], k + 5 - first, axis=0))
    assert (cls == C).sum() == 6 * len(firsts) + 5 * around_first
    assert around_first >= 1            # (a limit is only OBSERVABLE around an object the scan meets before a nearer one)
    # class E holds directions with exactly-zero components, and origins that are a class-A answer
    e = cls == E
    assert ((rays[:, d:2 * d] == 0.0).any(axis=1) & e).sum() >= 2 * len(full)
    assert ((rays[:, d:2 * d] == 0.0).sum(axis=1)[e] == d - 1).sum() >= len(full) - 2        # along a coordinate axis
    on_surface = np.flatnonzero(e & (sub == 3))
    assert len(on_surface) >= len(full)
    hits = {want[i, 2:2 + d].tobytes() for i in np.flatnonzero((cls == A) & (want[:, 0] == 1.0))}
    assert all(rays[i, :d].tobytes() in hits for i in on_surface)
    # the tier-1 cases carry the reference's own frame
    if CASES[name]["tier"] == 1:
        assert g.data["fb"].shape == (24, 40, 4) and (g.width, g.height, g.depth) == (40, 24, 4) and g.meta["rays_total"] > 40 * 24
    else:
        assert "fb" not in g.data.files


def early_ends(g, leaves):
    """Class-C rays whose limit ends a leaf's scan early.  The scan of a leaf's list stops at the first item that is hit within
    the limit (object.c:692-747; limit 0: at any hit) and leaves the rest of the list untested and unmarked: that is what the
    `cut` of a history entry records.  Counted here: rays with a limit that are answered within it by an item that is the last
    of NO list among the leaves the ray may touch -- wherever the scan met that item, items were left behind it."""
    d = g.scene.dims
    rays, want, cls = g.data["kat_in"], g.data["kat_out"], g.data["aim_class"]
    count = 0
    for i in np.flatnonzero((cls == C) & (rays[:, 2 * d] >= 0.0) & (want[:, 0] == 1.0)):
        x = int(want[i, 1])
        lim = rays[i, 2 * d]
        if lim > 0.0 and not ref_dist(rays[i, :d], want[i, 2:2 + d]) < lim:
            continue
        lists = [leaf_items(g.scene, k) for k in leaves[i]]
        lists = [l for l in lists if x in l]
        if lists and all(l[-1] != x for l in lists):
            count += 1
    return count


@pytest.mark.parametrize("name", ALL)
def test_coverage_is_a_condition_of_the_fixture(name):
    """Counted from the REFERENCE's answers alone, before anything is compared with them: every type of the scene answers at
    least 32 rays, at least 8 in each of the classes A, B (where the type has one), C, D, E; the items of every mask word
    answer at least 16; at least 64 class-C rays end a leaf's scan early."""
    g = golden(name)
    d = g.scene.dims
    c = CASES[name]
    present = [OBJ_TYPES[t] for t in scene_types(g)]
    assert present == [t for t in OBJ_TYPES if t != "hcube" or c["hcubes"]], present
    cov = coverage(g)
    short = []
    for ty in scene_types(g):
        total = sum(cov[ty, cl] for cl in range(6))
        if total < MIN_PER_TYPE:
            short.append("%s: %d rays" % (OBJ_TYPES[ty], total))
        for cl in (A, B, C, D, E):
            if cl == B and OBJ_TYPES[ty] not in HAS_CLASS_B:
                continue
            if cov[ty, cl] < MIN_PER_CLASS:
                short.append("%s class %s: %d rays" % (OBJ_TYPES[ty], CLASSES[cl], cov[ty, cl]))
    obj = g.data["kat_out"][:, 1].astype(np.int64)
    per_word = np.bincount(obj[obj >= 0] >> 6, minlength=c["words"])
    assert len(per_word) == c["words"]
    for w, got in enumerate(per_word):
        if got < MIN_PER_WORD:
            short.append("mask word %d: %d answers" % (w, got))
    ends = early_ends(g, walks(name))
    if ends < MIN_EARLY_ENDS:
        short.append("%d class-C rays end a leaf's scan early" % ends)
    print("%s: %d rays, per mask word %s, %d early ends" % (name, len(obj), per_word.tolist(), ends))
    assert not short, "%s: below the floor: %s" % (name, "; ".join(short))
    assert (answered_types(g) < 0).mean() <= 0.5
    lim = g.data["kat_in"][:, 2 * d]
    assert (lim < 0).any() and (lim == 0).any() and (lim > 0).any()


@pytest.mark.parametrize("name", ALL)
def test_leaves_share_items(name):
    """Conditions on the SCENE, for the rays of the fixture: a quarter of them touch five or more non-empty leaves (with the
    default of four {leaf, cut} pairs the history of such a ray overflows into the slab), a quarter touch two leaves whose
    lists share an item (what a visit mask exists for), and every list ascends in item number (the history is on)."""
    g = golden(name)
    fs = g.scene
    for k, node in enumerate(fs.kd_nodes):
        if node["dim"] < 0:
            ids = leaf_items(fs, k)
            assert all(a < b for a, b in zip(ids, ids[1:])) and all(0 <= i < fs.n_items for i in ids), k
    many = shared = 0
    leaves = walks(name)
    for ls in leaves:
        many += len(ls) > LEAF_HISTORY
        seen, again = set(), False
        for k in ls:
            ids = set(leaf_items(fs, k))
            again = again or bool(ids & seen)
            seen |= ids
        shared += again
    sizes = [node["num"] for node in fs.kd_nodes if node["dim"] < 0 and node["num"] > 0]
    print("%s: %d leaves of %d .. %d items (median %d); %.0f %% of the rays touch more than %d leaves, %.0f %% two that share an item"
          % (name, len(sizes), min(sizes), max(sizes), np.median(sizes), 100.0 * many / len(leaves), LEAF_HISTORY, 100.0 * shared / len(leaves)))
    assert 4 * many >= len(leaves) and 4 * shared >= len(leaves)
    assert np.median(sizes) >= 3 and max(sizes) >= 5


def param_words(fs, i):
    """Words of item i's parameter record as ndt_blob.hip:build_blob lays it out (hcube: not staged)."""
    n, o = fs.dims, fs.objects[i]
    name = OBJ_TYPES[o["type"]]
    if name == "orthotope":
        return n + 1 + fs._flags[o["flag_off"]] * (n + 3)
    return {"sphere": n + 1, "hplane": 2 * n + 1, "hdisk": 2 * n + 1, "cylinder": 2 * n + 4, "hcylinder": n + 1 + (n - 2) * (n + 3),
            "hfacet": 6 * n + 4, "facet": 6 * n + 7}[name]


def test_record_limit_on_both_sides():
    """The coherent leaf scan needs n + 2 + max_param_words <= 128: the crowds without an hcube are within it up to 10-D (127 words
    there) and over it in 11-D and 12-D."""
    for name, c in CASES.items():
        if c["tier"] == 1 and not c["hcubes"]:
            fs = golden(name).scene
            record = fs.dims + 2 + max(param_words(fs, i) for i in range(fs.n_items))
            assert (record <= 128) == (fs.dims <= 10), (name, record)
            assert fs.dims != 10 or record == 127


@pytest.mark.parametrize("name", ALL)
def test_oracle_reproduces_the_reference(oracle, name):
    """The CPU oracle against the compiled reference on every crowd, bit for bit, as tests/test_oracle_golden.py compares: the
    sweeps below may lean on it for frame sizes the fixtures do not hold."""
    g = golden(name)
    rays, want = g.data["kat_in"], g.data["kat_out"]
    d = g.scene.dims
    obj, hit, nrm = oracle.trace(g.scene, rays)
    bad = np.flatnonzero((obj != want[:, 1].astype(np.int32)) | (hit != want[:, 2:2 + d]).any(axis=1) | (nrm != want[:, 2 + d:]).any(axis=1))
    assert len(bad) == 0, "%d rays differ, first: ray %d item %d class %s: oracle object %d, reference %d" % (
        len(bad), bad[0], g.data["aim_item"][bad[0]], CLASSES[g.data["aim_class"][bad[0]]], obj[bad[0]], int(want[bad[0], 1]))
    assert np.array_equal((obj >= 0).astype(np.float64), want[:, 0])
    if "fb" in g.data.files:
        out, st = oracle.render(g.scene, g.width, g.height, g.depth)
        assert np.array_equal(out, g.data["fb"]), "max abs diff %g" % np.abs(out - g.data["fb"]).max()
        assert st.rays_ref_equiv == g.meta["rays_total"] and st.rays_primary == g.width * g.height
        assert st.rays_secondary > 0 and st.rays_shadow > 0


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def gpu():
    from ndt_amd.hip import NdtHip
    ctx = NdtHip(0)
    yield ctx
    ctx.close()


def answers(gpu, g):
    return gpu.trace_rays(g.data["kat_in"])


def identical(got, want, what):
    for a, b, part in zip(got, want, ("objects", "hit points", "normals")):
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b), "%s: %s differ" % (what, part)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_family_reached(gpu, capfd, name):
    """The scene lands in the kernel family it was built for: upload_scene says so under debug_levels."""
    g = golden(name)
    c = CASES[name]
    try:
        gpu.set_option("debug_levels", 1)
        capfd.readouterr()
        gpu.upload_scene(g.scene)
        err = capfd.readouterr().err
    finally:
        gpu.set_option("debug_levels", 0)
    m = re.search(r"(\d+)-D, (\d+) items .* (\d+) words staged by the trace kernels .*tier (\d+), (\d+) mask word", err)
    assert m, err
    dims, items, words, tier, mask = (int(x) for x in m.groups())
    print("%s: %d-D, %d items, trace section %d bytes: tier %d, %d mask word(s)" % (name, dims, items, 8 * words, tier, mask))
    assert (dims, items, tier, mask) == (c["dims"], c["items"], c["tier"], c["words"])
    if name.endswith("_r"):
        assert tier == 0 and 8 * words <= 65536 and mask == (3 if c["items"] > 128 else 2)
    elif name.endswith("_l"):
        assert tier == 1 and mask <= 4 and 8 * words > 65536 and c["items"] <= 256
    else:
        assert tier == 1 and mask == 5


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_device_answers_are_the_references(gpu, name):
    """trace_rays on every crowd: object ids exact, hit points and normals to the last bit; no ray is excused."""
    g = golden(name)
    gpu.upload_scene(g.scene)
    got = answers(gpu, g)
    print("%s: %d rays, 0 excused" % (name, len(got[0])))
    same_answers(got, g.data["kat_out"], g.scene.dims, name)


HCUBE_OPTIONS = [("hull_box", 0, 1), ("face_box", 0, 1), ("face_tree", 0, 1), ("face_groups", 0, 1)]
TIER1_OPTIONS = [("item_boxes", 0, 1), ("leaf_history", 0, 4), ("leaf_history", 1, 4), ("leaf_history", 2, 4), ("leaf_history", 3, 4), ("leaf_scan", 0, 1),
                 ("leaf_scan_group", 1, 64), ("leaf_scan_group", 8, 64), ("leaf_scan_group", 64, 64)]
PREPASS_OPTIONS = [("gate_prepass", 0, 2), ("gate_prepass", 1, 2), ("gate_prepass", 2, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_options_change_nothing(gpu, name):
    """One option at a time, the scene uploaded again: trace_rays gives the default's answers bit for bit (and they are the
    reference's)."""
    g = golden(name)
    c = CASES[name]
    gpu.upload_scene(g.scene)
    base = answers(gpu, g)
    same_answers(base, g.data["kat_out"], g.scene.dims, name)
    options = (TIER1_OPTIONS if c["tier"] == 1 else []) + PREPASS_OPTIONS + (HCUBE_OPTIONS if c["hcubes"] else [])
    for option, other, default in options:
        try:
            gpu.set_option(option, other)
            gpu.upload_scene(g.scene)
            identical(answers(gpu, g), base, "%s with %s = %d" % (name, option, other))
        finally:
            gpu.set_option(option, default)
    gpu.upload_scene(g.scene)
    identical(answers(gpu, g), base, name + " with the defaults restored")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_lane_company_changes_nothing(gpu, name):
    """A ray's answer is its own.  The same rays shuffled (a wavefront's lanes stand on different leaves, scan groups are
    partial), sorted by the item they are aimed at (groups are full), and cut to a count that is no multiple of 64."""
    g = golden(name)
    rays, item = g.data["kat_in"], g.data["aim_item"]
    n = len(rays)
    gpu.upload_scene(g.scene)
    base = answers(gpu, g)
    same_answers(base, g.data["kat_out"], g.scene.dims, name)
    orders = {"shuffled": np.random.default_rng(2025 + g.scene.dims).permutation(n), "sorted by item": np.argsort(item, kind="stable"),
              "cut": np.arange(n - n % 64 - 27)}
    assert len(orders["cut"]) % 64 != 0
    for what, order in orders.items():
        got = gpu.trace_rays(np.ascontiguousarray(rays[order]))
        identical(got, tuple(x[order] for x in base), "%s %s" % (name, what))


@pytest.mark.gpu
@pytest.mark.parametrize("name", TIER1)
def test_frame_vs_reference_golden(gpu, name):
    g = golden(name)
    gpu.upload_scene(g.scene)
    out, st = gpu.render(g.width, g.height, g.depth)
    diff = np.abs(out - g.data["fb"])
    assert diff.max() < TOL_SPEC, "max abs diff %g" % diff.max()
    assert (diff > TOL_TIGHT).sum() == 0, "%d values differ by more than %g (max %g)" % ((diff > TOL_TIGHT).sum(), TOL_TIGHT, diff.max())
    assert st.rays_ref_equiv == g.meta["rays_total"]
    assert st.rays_primary == g.width * g.height


@pytest.mark.gpu
@pytest.mark.parametrize("name", TIER1)
def test_frame_vs_oracle(gpu, oracle, name):
    g = golden(name)
    gpu.upload_scene(g.scene)
    w, h = 37, 19
    out, st = gpu.render(w, h, g.depth)
    want, so = oracle.render(g.scene, w, h, g.depth)
    diff = np.abs(out - want)
    assert diff.max() < TOL_TIGHT, "max abs diff %g" % diff.max()
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow, st.rays_ref_equiv) == (
        so.rays_primary, so.rays_secondary, so.rays_shadow, so.rays_ref_equiv)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TIER1)
def test_every_pipeline_renders_the_same_frame(gpu, name):
    """Per-bounce launches, the streaming frame kernel (fused or not) and the one-stream pipeline: the same image bit for bit and
    the same counts.  This is what runs the global-memory frame kernel on a crowd."""
    g = golden(name)
    gpu.upload_scene(g.scene)
    outs = []
    try:
        for pipeline, fused, overlap in ((1, 1, 1), (2, 1, 1), (2, 0, 1), (1, 1, 0)):
            gpu.set_option("pipeline", pipeline)
            gpu.set_option("stream_fused", fused)
            gpu.set_option("light_overlap", overlap)
            img, st = gpu.render(g.width, g.height, g.depth)
            outs.append((img, (st.rays_primary, st.rays_secondary, st.rays_shadow, st.rays_ref_equiv, st.levels)))
    finally:
        gpu.set_option("pipeline", 0)
        gpu.set_option("stream_fused", 1)
        gpu.set_option("light_overlap", 1)
    for img, counts in outs[1:]:
        assert np.array_equal(img.view(np.uint64), outs[0][0].view(np.uint64))
        assert counts == outs[0][1]
    assert np.abs(outs[0][0] - g.data["fb"]).max() < TOL_TIGHT
