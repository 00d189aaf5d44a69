"""The trace kernels where their families SWITCH (tests/golden/edge*, made by tests/golden/make_golden_edges.py from the
compiled reference; the scene program is tests/scenes/parity_crowd.c).

Every rule that picks a trace kernel is a comparison: the item count against 64 (item sets) and 256 (a register mask of
four words), the trace section against 64 KB, the LDS a workgroup would need for section and traversal stack against
160 KB (ndt_kernels.hip:launch_trace, ndt_stream.hpp:launch_frame_stream), a leaf's length against the 64 entries of one
window of the coherent leaf scan (ndt_device.hpp:cls_scan).  tests/test_crowd_tiers.py stands in the interior of every
family; this module stands at the values where the rules flip:

  edge{3,7,12}d_64    64 items: the most the item sets hold -- bit 63 of a leaf's set and of a node's `below` set
  edge{3,7,12}d_65    65 items: the fewest of the register kernel; item 64 is alone in mask word 1
  edge{3,7}d_128/129  two full words; item 128 alone in word 2
  edge3d_l192/l193    (sphere, hdisk, cylinder only) three full words; item 192 alone in word 3, which no other fixture fills
  edge3d_l256         (spheres only) 256 items in tier 0: all four register words full
  edge3d_l257         (spheres only) tier 1 by the COUNT alone -- the section is still under 64 KB; item 256 alone in word 4
  edge12d_257         tier 1, five words, a record over the leaf-scan limit

Their EDGE items -- item 0, the items on either side of every word boundary, the last two -- carry rays of all six classes
and rays whose line touches two leaves that both list the item.  Beside the fixtures, three pieces of plain-Python surgery
on a scene's kd-tree put a scene where no fixture is: deep() pads the tree with empty levels above the root until the
traversal stack no longer fits LDS (the scratch-stack variants of both kernels, one-word and four-word) and to the depth
the upload refuses; one_leaf() makes one list of a chosen length (63, 64, 65, 127, 128, 129: the windows of the leaf scan);
reversed_lists() turns every list round (no item sets, no leaf history: the slab from the first leaf on).

Not covered, because no such case exists: item 0 (the floor) is an infinite object, it stands in no leaf and has no mask
bit to find set.
"""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, golden
from ndt_amd import load_scene
from ndt_amd.flat_scene import OBJ_TYPES
from test_aimed_rays import A, C, D, E, F, CLASSES, MIN_PER_CLASS, TOL_SPEC, TOL_TIGHT, answered_types, coverage, ref_dist, same_answers, scene_types
from test_crowd_tiers import MIN_EARLY_ENDS, MIN_PER_WORD, PREPASS_OPTIONS, REGISTER, TIER1_OPTIONS, early_ends, identical, leaf_items, walks

NDT_E_UNSUPPORTED = -2
KD_STACK = 40               # ndt_device.hpp:NDT_KD_STACK, the deepest tree the upload takes
LDS_LIMIT = 160 * 1024      # launch_trace, launch_frame_stream: section + stack beyond this -> the stack goes to scratch
SMALL_BLOCK = 256           # the workgroup of a launch of fewer than 4096 batches (trace) / 1024 batches (frame)
FILE_LIMIT = 400 * 1024
ALL_FILES_LIMIT = 4 * 1024 * 1024


def case(dims, items, tier, mix="all", per_type=8):
    return dict(dims=dims, items=items, tier=tier, words=(items + 63) // 64, mix=mix, per_type=per_type)


# name -> N, K, the tier the scene is built to reach, its mix of types, full items per type
CASES = {}
for _n in (3, 7, 12):
    CASES["edge%dd_64" % _n] = case(_n, 64, 0)
    CASES["edge%dd_65" % _n] = case(_n, 65, 0)
for _n in (3, 7):
    CASES["edge%dd_128" % _n] = case(_n, 128, 0)
    CASES["edge%dd_129" % _n] = case(_n, 129, 0)
CASES["edge3d_l192"] = case(3, 192, 0, "light")
CASES["edge3d_l193"] = case(3, 193, 0, "light")
CASES["edge3d_l256"] = case(3, 256, 0, "spheres")
CASES["edge3d_l257"] = case(3, 257, 1, "spheres")
CASES["edge12d_257"] = case(12, 257, 1, per_type=4)
ALL = list(CASES)
SETS = [c for c in ALL if CASES[c]["items"] <= 64]
MIX_TYPES = {"all": ["hplane", "sphere", "cylinder", "hcylinder", "orthotope", "hdisk", "hfacet", "facet"],
             "light": ["hplane", "sphere", "cylinder", "hdisk"], "spheres": ["hplane", "sphere"]}

# Scenes padded to kd depth 40 for the scratch-stack variants.  A 41-level stack of 256 lanes is 125 952 bytes, so the section has
# to be over 37 888 bytes -- and, with the 16 bytes of every added node, still within 64 KB.  Four-word kernels: crowd3d_r
# (63 736 + 864 bytes), crowd6d_r (64 256 + 896), edge12d_65 (43 128 + 960), edge3d_l256 (52 592 + 896).  One-word kernels:
# c3_random4d, 40 items and 58 480 + 1 440 bytes (60 nodes and their `below` sets).
PADDED = ["crowd3d_r", "crowd6d_r", "edge12d_65", "edge3d_l256", "c3_random4d"]
# crowd7d_r (65 512 bytes) and crowd12d_r (65 488) have no room for 54 and 56 more nodes: padded, they are tier-1 scenes of 3 and 2
# mask words whose section is a few hundred bytes over 64 KB -- the other side of that rule, which no fixture stands on so closely
PADDED_OVER = ["crowd7d_r", "crowd12d_r"]
SCAN_SCENES = ["crowd3d_gn", "crowd7d_gn", "edge3d_l257"]
WINDOW_LENGTHS = [1, 63, 64, 65, 127, 128, 129, None]


def edge_items(items):
    """Item 0, the items on either side of every mask-word boundary that exists, the last two."""
    out = {0, items - 2, items - 1}
    for b in (64, 128, 192, 256):
        if b < items:
            out |= {i for i in (b - 2, b - 1, b, b + 1) if i < items}
    return sorted(out)


# ------------------------------------------------------------------------------------------------ scene surgery

def copy_of(name):
    """A scene of its own, loaded again from the fixture's file: the cached one stays as it is."""
    return load_scene(os.path.join(GOLDEN, golden(name).meta["scene_file"]))


def kd_depth(fs):
    """Levels of the tree, the root being level 1 (what ndt_hip_upload_scene reports)."""
    deepest, stack = 0, [(0, 1)]
    while stack:
        k, level = stack.pop()
        deepest = max(deepest, level)
        if fs.kd_nodes[k]["dim"] >= 0:
            stack += [(fs.kd_nodes[k]["left"], level + 1), (fs.kd_nodes[k]["right"], level + 1)]
    return deepest


def deep(fs, levels):
    """`levels` new split nodes above the root.  Node i splits dimension i % dims at bb_lower[dim] - 1: a plane outside the root
    box, which no ray's segment inside the box reaches; its left child is an empty leaf, its right child the rest."""
    lower = fs.vec(fs.bb["lower"])
    nodes = []
    for i in range(levels):
        dim = i % fs.dims
        nodes.append({"dim": dim, "boundary": float(lower[dim] - 1.0), "left": 2 * i + 1, "right": 2 * i + 2, "num": 0, "first": 0})
        nodes.append({"dim": -1, "boundary": 0.0, "left": -1, "right": -1, "num": 0, "first": 0})
    shift = 2 * levels
    for k in fs.kd_nodes:
        k = dict(k)
        if k["dim"] >= 0:
            k["left"], k["right"] = k["left"] + shift, k["right"] + shift
        nodes.append(k)
    fs.kd_nodes = nodes
    fs._struct = None
    fs.finalize()
    return fs


def padded(name, depth=KD_STACK):
    fs = copy_of(name)
    return deep(fs, depth - kd_depth(fs))


def one_leaf(fs, length):
    """The tree is a single leaf that lists the first `length` finite items in ascending order (None: all of them)."""
    ids = sorted(set(fs.leaf_refs))
    ids = ids if length is None else ids[:length]
    fs.kd_nodes = [{"dim": -1, "boundary": 0.0, "left": -1, "right": -1, "num": len(ids), "first": 0}]
    fs.leaf_refs = ids
    fs._struct = None
    fs.finalize()
    return fs


def reversed_lists(fs):
    refs = list(fs.leaf_refs)
    for k in fs.kd_nodes:
        if k["dim"] < 0:
            refs[k["first"]:k["first"] + k["num"]] = refs[k["first"]:k["first"] + k["num"]][::-1]
    fs.leaf_refs = refs
    fs._struct = None
    fs.finalize()
    return fs


def differing(got, want, d):
    """Rays whose oracle answer (obj, hit, nrm) is not the recorded reference row, bit for bit."""
    obj, hit, nrm = got
    return np.flatnonzero((obj != want[:, 1].astype(np.int32)) | (hit.view(np.uint64) != want[:, 2:2 + d].view(np.uint64)).any(axis=1)
                          | (nrm.view(np.uint64) != np.ascontiguousarray(want[:, 2 + d:]).view(np.uint64)).any(axis=1))


# ------------------------------------------------------------------------------------------------ CPU

def test_case_table():
    assert len(ALL) == 15 and len(SETS) == 3
    sizes = []
    for name, c in CASES.items():
        g = golden(name)
        assert (g.scene.dims, g.scene.n_items, g.meta["items"]) == (c["dims"], c["items"], c["items"]), name
        assert [OBJ_TYPES[t] for t in scene_types(g)] == [t for t in OBJ_TYPES if t in MIX_TYPES[c["mix"]]], name
        assert g.meta["scene_file"] == name + ".ndtscene.gz" and g.meta["edge_items"] == edge_items(c["items"])
        assert ("mix=" + c["mix"] in g.meta["config"]) == (c["mix"] != "all") and "nohcube" in g.meta["config"]
        assert sorted(l["type"] for l in g.scene.lights) == [0, 1, 2, 3]
        assert g.scene.inf_refs == [0] and 0 not in g.scene.leaf_refs           # the floor: an infinite object, in no leaf
        for ext in (".npz", ".ndtscene.gz", ".json"):
            sizes.append(os.path.getsize(os.path.join(GOLDEN, name + ext)))
            assert sizes[-1] <= FILE_LIMIT, (name + ext, sizes[-1])
    print("edge fixtures: %d files, %d bytes, the largest %d" % (len(sizes), sum(sizes), max(sizes)))
    assert sum(sizes) < ALL_FILES_LIMIT
    assert edge_items(64) == [0, 62, 63] and edge_items(65) == [0, 62, 63, 64] and edge_items(129) == [0, 62, 63, 64, 65, 126, 127, 128]
    assert edge_items(257) == [0, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 192, 193, 254, 255, 256]


@pytest.mark.parametrize("name", ALL)
def test_fixture_layout(name):
    g = golden(name)
    c = CASES[name]
    d = g.scene.dims
    rays, want = g.data["kat_in"], g.data["kat_out"]
    n = len(rays)
    assert rays.shape == (n, 2 * d + 1) and want.shape == (n, 2 * d + 2) and n == g.meta["rays"]
    item, cls, sub = g.data["aim_item"], g.data["aim_class"], g.data["aim_sub"]
    assert item.shape == cls.shape == sub.shape == (n,)
    assert item.min() >= 0 and item.max() < g.scene.n_items and cls.min() == 0 and cls.max() == 5
    assert set(item.tolist()) == set(range(g.scene.n_items))              # every kd item has rays of its own
    assert np.abs(np.linalg.norm(rays[:, d:2 * d], axis=1) - 1.0).max() < 1e-12
    # every item has classes A and F; the full items (per_type of a type, or all of it; and every edge item) have B .. E too
    full = set(g.meta["full_items"])
    assert full >= set(edge_items(c["items"]))
    by_type = {}
    for i in range(g.scene.n_items):
        by_type.setdefault(g.scene.objects[i]["type"], []).append(i)
    for ty, ids in by_type.items():
        assert len(full & set(ids)) >= min(c["per_type"], len(ids)), OBJ_TYPES[ty]
    for cl in (A, F):
        assert set(item[cls == cl].tolist()) == set(range(g.scene.n_items))
    assert set(item[cls == D].tolist()) == set(item[cls == E].tolist()) == full
    assert set(item[cls == C].tolist()) <= full and len(set(item[cls == C].tolist())) >= 0.9 * len(full)
    # class C: the limits of one class-A ray stand right behind it (tests/test_crowd_tiers.py:test_fixture_layout)
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
    assert around_first >= 1
    e = cls == E
    assert ((rays[:, d:2 * d] == 0.0).any(axis=1) & e).sum() >= 2 * len(full)
    assert ((rays[:, d:2 * d] == 0.0).sum(axis=1)[e] == d - 1).sum() >= len(full) - 2
    on_surface = np.flatnonzero(e & (sub == 3))
    assert len(on_surface) >= len(full)
    hits = {want[i, 2:2 + d].tobytes() for i in np.flatnonzero((cls == A) & (want[:, 0] == 1.0))}
    assert all(rays[i, :d].tobytes() in hits for i in on_surface)
    # the rays aimed at the edge items from nearby stand at the end: class A, the whole ray, of the finite edge items only
    extra = g.meta["edge_rays"]
    assert extra > 0 and (cls[n - extra:] == A).all() and (rays[n - extra:, 2 * d] < 0).all()
    assert set(item[n - extra:].tolist()) == set(edge_items(c["items"])) - {0}
    # every case carries the reference's own frame
    assert g.data["fb"].shape == (24, 40, 4) and (g.width, g.height, g.depth) == (40, 24, 4) and g.meta["rays_total"] > 40 * 24


@pytest.mark.parametrize("name", ALL)
def test_oracle_reproduces_the_reference(oracle, name):
    """The CPU oracle against the compiled reference on every edge case, rays and frame, bit for bit: the GPU tests below lean on it
    for the scenes and frame sizes that the fixtures do not hold."""
    g = golden(name)
    rays, want = g.data["kat_in"], g.data["kat_out"]
    bad = differing(oracle.trace(g.scene, rays), want, g.scene.dims)
    assert len(bad) == 0, "%d rays differ, first: ray %d item %d class %s" % (len(bad), bad[0], g.data["aim_item"][bad[0]], CLASSES[g.data["aim_class"][bad[0]]])
    out, st = oracle.render(g.scene, g.width, g.height, g.depth)
    assert np.array_equal(out, g.data["fb"]), "max abs diff %g" % np.abs(out - g.data["fb"]).max()
    assert st.rays_ref_equiv == g.meta["rays_total"] and st.rays_primary == g.width * g.height
    assert st.rays_secondary > 0 and st.rays_shadow > 0


@pytest.mark.parametrize("name", ALL)
def test_answer_counts_are_a_condition_of_the_fixture(name):
    """Counted from the REFERENCE's answers alone, before anything is compared with them: every edge item answers at least 16
    rays; the items of every mask word answer at least 16, the last word too where it holds a single item; every type of the
    scene answers at least 8 class-C rays, and 64 K / 320 class-C rays end a leaf's scan early."""
    g = golden(name)
    d = g.scene.dims
    c = CASES[name]
    short = []
    obj = g.data["kat_out"][:, 1].astype(np.int64)
    per_item = np.bincount(obj[obj >= 0], minlength=c["items"])
    for i in edge_items(c["items"]):
        if per_item[i] < MIN_PER_WORD:
            short.append("edge item %d: %d answers" % (i, per_item[i]))
    per_word = np.bincount(obj[obj >= 0] >> 6, minlength=c["words"])
    assert len(per_word) == c["words"]
    for w, got in enumerate(per_word):
        if got < MIN_PER_WORD:
            short.append("mask word %d: %d answers" % (w, got))
    cov = coverage(g)
    for ty in scene_types(g):
        if cov[ty, C] < MIN_PER_CLASS:
            short.append("%s class C: %d rays" % (OBJ_TYPES[ty], cov[ty, C]))
    ends = early_ends(g, walks(name))
    if ends < MIN_EARLY_ENDS * c["items"] / 320.0:
        short.append("%d class-C rays end a leaf's scan early" % ends)
    print("%s: %d rays; edge items %s answer %s; per mask word %s; %d early ends (floor %.1f)" % (
        name, len(obj), edge_items(c["items"]), per_item[edge_items(c["items"])].tolist(), per_word.tolist(), ends, MIN_EARLY_ENDS * c["items"] / 320.0))
    assert not short, "%s: below the floor: %s" % (name, "; ".join(short))
    assert (answered_types(g) < 0).mean() <= 0.5
    lim = g.data["kat_in"][:, 2 * d]
    assert (lim < 0).any() and (lim == 0).any() and (lim > 0).any()


@pytest.mark.parametrize("name", ALL)
def test_edge_items_are_met_in_two_leaves(name):
    """For every edge item the tree lists, at least 8 rays have -- among the leaves their segment may touch -- two that both list
    the item: the second of them finds the item's mask bit set.  (Item 0, the floor, is infinite: no leaf lists it.)"""
    g = golden(name)
    fs = g.scene
    c = CASES[name]
    for k, node in enumerate(fs.kd_nodes):
        if node["dim"] < 0:
            ids = leaf_items(fs, k)
            assert all(a < b for a, b in zip(ids, ids[1:])) and all(0 <= i < fs.n_items for i in ids), k
    edges = [i for i in edge_items(c["items"]) if i not in fs.inf_refs]
    assert edges == edge_items(c["items"])[1:]
    twice = dict.fromkeys(edges, 0)
    for ls in walks(name):
        lists = [leaf_items(fs, k) for k in ls]
        for i in edges:
            twice[i] += sum(i in l for l in lists) >= 2
    sizes = [node["num"] for node in fs.kd_nodes if node["dim"] < 0 and node["num"] > 0]
    print("%s: depth %d, %d leaves of %d .. %d items; rays that touch two leaves listing the edge item: %s" % (
        name, kd_depth(fs), len(sizes), min(sizes), max(sizes), twice))
    assert min(twice.values()) >= MIN_PER_CLASS, twice


@pytest.mark.parametrize("name", ALL + [c for c in PADDED + PADDED_OVER if c not in ALL])
def test_deep_changes_no_answer(oracle, name):
    """The oracle on the scene padded to kd depth 40 (and to 41, which the device refuses) gives the fixture's recorded REFERENCE
    answers bit for bit, every ray and limit: the added planes lie outside the root box."""
    g = golden(name)
    for depth in (KD_STACK, KD_STACK + 1):
        fs = padded(name, depth)
        assert kd_depth(fs) == depth and len(fs.kd_nodes) == len(g.scene.kd_nodes) + 2 * (depth - kd_depth(g.scene))
        bad = differing(oracle.trace(fs, g.data["kat_in"]), g.data["kat_out"], fs.dims)
        print("%s: kd depth %d -> %d: %d of %d rays differ from the recorded reference answers" % (name, kd_depth(g.scene), depth, len(bad), len(g.data["kat_in"])))
        assert len(bad) == 0


@pytest.mark.parametrize("name", SCAN_SCENES + ["edge3d_64", "edge3d_l256"])
def test_one_leaf_changes_only_ties(oracle, name):
    """With every finite item in one list the closest hit of a whole ray (limit < 0) is the recorded reference answer; or another
    object at the same distance to the last bit (the list is scanned in item order, the tree's leaves in the ray's); or a NEARER
    hit at a point whose leaf does not list the item: one list shows a ray all of every item, the tree only what lies in the
    leaves that the item's box reaches (7-D hfacets stick out of theirs).  Both counts are printed."""
    g = golden(name)
    d = g.scene.dims
    rays, want = g.data["kat_in"], g.data["kat_out"]
    fs = one_leaf(copy_of(name), None)
    assert len(fs.kd_nodes) == 1 and fs.leaf_refs == list(range(1, fs.n_items)) and fs.inf_refs == [0]
    got = oracle.trace(fs, rays)
    whole = rays[:, 2 * d] < 0
    bad = [i for i in differing(got, want, d) if whole[i]]
    ties = unseen = 0
    for i in bad:
        x = int(got[0][i])
        assert x >= 0 and x != int(want[i, 1]), i
        near = ref_dist(rays[i, :d], got[1][i])
        if want[i, 0] == 1.0 and near == ref_dist(rays[i, :d], want[i, 2:2 + d]):
            ties += 1
            continue
        # a nearer hit: the leaf whose cell holds the hit point does not list the item -- the box the reference's builder sorted it
        # by does not reach there, and the tree never shows that piece of it to a ray
        assert want[i, 0] == 0.0 or near < ref_dist(rays[i, :d], want[i, 2:2 + d]), i
        k = 0
        while g.scene.kd_nodes[k]["dim"] >= 0:
            node = g.scene.kd_nodes[k]
            k = node["left"] if got[1][i][node["dim"]] < node["boundary"] else node["right"]
        assert x not in leaf_items(g.scene, k), i
        unseen += 1
    print("%s: one leaf of %d items: of %d whole rays %d are answered by another object at the same distance, %d by a piece of an item "
          "(%s) that lies outside the leaves listing it" % (name, len(fs.leaf_refs), int(whole.sum()), ties, unseen,
                                                           ", ".join(sorted({OBJ_TYPES[fs.objects[int(got[0][i])]["type"]] for i in bad})) or "none"))
    short = one_leaf(copy_of(name), 63)
    assert short.leaf_refs == list(range(1, 64)) and short.kd_nodes[0]["num"] == 63


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def gpu():
    from ndt_amd.hip import NdtHip
    ctx = NdtHip(0)
    yield ctx
    ctx.close()


def upload(gpu, capfd, fs, what):
    """Upload under debug_levels and return what the library says of the scene: items, kd depth, words of the trace section,
    tier, mask words."""
    try:
        gpu.set_option("debug_levels", 1)
        capfd.readouterr()
        gpu.upload_scene(fs)
        err = capfd.readouterr().err
    finally:
        gpu.set_option("debug_levels", 0)
    m = re.search(r"(\d+)-D, (\d+) items .* kd nodes of depth (\d+); (\d+) words staged by the trace kernels .*tier (\d+), (\d+) mask word", err)
    assert m, err
    dims, items, depth, words, tier, mask = (int(x) for x in m.groups())
    stack = ((words + 1) & ~1) * 8 + SMALL_BLOCK * (depth + 1) * 12
    with capfd.disabled():          # (what is printed while capfd captures is lost with the next readouterr)
        print("%s: %d-D, %d items, kd depth %d, trace section %d bytes: tier %d, %d mask word(s)%s" % (
            what, dims, items, depth, 8 * words, tier, mask, "" if tier else "; section + stack of %d lanes %d bytes (%s 160 KB)" % (
                SMALL_BLOCK, stack, "over" if stack > LDS_LIMIT else "within")))
    return dict(dims=dims, items=items, depth=depth, words=words, tier=tier, mask=mask, stack=stack)


def counts(st):
    return (st.rays_primary, st.rays_secondary, st.rays_shadow, st.rays_ref_equiv)


_oracle_frames = {}


def oracle_frame(oracle, key, fs, depth):
    if key not in _oracle_frames:
        out, so = oracle.render(fs, 37, 19, depth)
        _oracle_frames[key] = (out, counts(so))
    return _oracle_frames[key]


def frame_equals_oracle(gpu, oracle, key, fs, depth, oracle_scene=None):
    """A 37x19 frame of the uploaded scene against the oracle's, ray counts equal."""
    out, st = gpu.render(37, 19, depth)
    want, want_counts = oracle_frame(oracle, key, oracle_scene or fs, depth)
    diff = np.abs(out - want)
    assert diff.max() < TOL_TIGHT, "%s: max abs diff %g" % (key, diff.max())
    assert counts(st) == want_counts, key


# pipeline, stream_fused, light_overlap, fuse_primaries: the default; per-bounce launches; the streaming frame kernel fused or not;
# the one-stream pipeline; the per-bounce kernels with a k_primary launch of their own, and making their own primaries
PIPELINES = [(0, 1, 1, -1), (1, 1, 1, -1), (2, 1, 1, -1), (2, 0, 1, -1), (1, 1, 0, -1), (1, 1, 1, 0), (1, 1, 1, 1)]


def every_pipeline_renders_the_same(gpu, w, h, depth, what):
    outs = []
    try:
        for pipeline, fused, overlap, primaries in PIPELINES:
            gpu.set_option("pipeline", pipeline)
            gpu.set_option("stream_fused", fused)
            gpu.set_option("light_overlap", overlap)
            gpu.set_option("fuse_primaries", primaries)
            img, st = gpu.render(w, h, depth)
            outs.append((img, counts(st) + (st.levels,)))
    finally:
        gpu.set_option("pipeline", 0)
        gpu.set_option("stream_fused", 1)
        gpu.set_option("light_overlap", 1)
        gpu.set_option("fuse_primaries", -1)
    for (img, cnt), setting in zip(outs[1:], PIPELINES[1:]):
        assert np.array_equal(img.view(np.uint64), outs[0][0].view(np.uint64)), "%s: pipeline, stream_fused, light_overlap, fuse_primaries = %s" % (what, setting)
        assert cnt == outs[0][1], (what, setting)
    return outs[0][0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_family_reached(gpu, capfd, name):
    """The scene lands in the kernel family it was built for.  edge3d_l256 is the last of tier 0, with four words; edge3d_l257 is in
    tier 1 by its count alone; a 64-item scene without item sets takes the four-word kernels (two words reported)."""
    g = golden(name)
    c = CASES[name]
    got = upload(gpu, capfd, g.scene, name)
    assert (got["dims"], got["items"], got["tier"], got["mask"]) == (c["dims"], c["items"], c["tier"], c["words"])
    assert got["depth"] == kd_depth(g.scene)
    if c["tier"] == 0:
        assert 8 * got["words"] <= 65536 and got["stack"] <= LDS_LIMIT and got["mask"] == (1 if c["items"] <= 64 else 2 if c["items"] <= 128 else 3 if c["items"] <= 192 else 4)
    if name == "edge3d_l256":
        assert (got["tier"], got["mask"]) == (0, 4)
    if name == "edge3d_l257":
        assert (got["tier"], got["mask"]) == (1, 5) and 8 * got["words"] <= 65536
    if name == "edge12d_257":
        assert (got["tier"], got["mask"]) == (1, 5) and 8 * got["words"] > 65536
    if name in SETS:
        try:
            gpu.set_option("item_sets", 0)
            lists = upload(gpu, capfd, g.scene, name + " without item sets")
        finally:
            gpu.set_option("item_sets", 1)
        assert (lists["tier"], lists["mask"]) == (0, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_device_answers_are_the_references(gpu, name):
    """trace_rays on every edge case: object ids exact, hit points and normals to the last bit, no ray excused; the same rays
    shuffled and cut to a count that is no multiple of 64; one option at a time."""
    g = golden(name)
    c = CASES[name]
    rays = g.data["kat_in"]
    n = len(rays)
    gpu.upload_scene(g.scene)
    base = gpu.trace_rays(rays)
    print("%s: %d rays, 0 excused" % (name, n))
    same_answers(base, g.data["kat_out"], g.scene.dims, name)
    orders = {"shuffled": np.random.default_rng(4242 + n).permutation(n), "cut": np.arange(n - n % 64 - 27)}
    assert len(orders["cut"]) % 64 != 0
    for what, order in orders.items():
        got = gpu.trace_rays(np.ascontiguousarray(rays[order]))
        identical(got, tuple(x[order] for x in base), "%s %s" % (name, what))
    options = PREPASS_OPTIONS + (TIER1_OPTIONS if c["tier"] == 1 else []) + ([("item_sets", 0, 1)] if name in SETS else [])
    for option, other, default in options:
        try:
            gpu.set_option(option, other)
            gpu.upload_scene(g.scene)
            identical(gpu.trace_rays(rays), base, "%s with %s = %d" % (name, option, other))
        finally:
            gpu.set_option(option, default)
    gpu.upload_scene(g.scene)
    identical(gpu.trace_rays(rays), base, name + " with the defaults restored")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_frames_of_the_edge_cases(gpu, oracle, name):
    """Every edge case rendered: the reference's own 40x24 frame and ray count, a 37x19 frame against the oracle, and the same
    image bit for bit from every pipeline."""
    g = golden(name)
    gpu.upload_scene(g.scene)
    out, st = gpu.render(g.width, g.height, g.depth)
    diff = np.abs(out - g.data["fb"])
    assert diff.max() < TOL_SPEC, "max abs diff %g" % diff.max()
    assert (diff > TOL_TIGHT).sum() == 0, "%d values differ by more than %g (max %g)" % ((diff > TOL_TIGHT).sum(), TOL_TIGHT, diff.max())
    assert st.rays_ref_equiv == g.meta["rays_total"]
    assert st.rays_primary == g.width * g.height
    frame_equals_oracle(gpu, oracle, name, g.scene, g.depth)
    first = every_pipeline_renders_the_same(gpu, g.width, g.height, g.depth, name)
    assert np.array_equal(first.view(np.uint64), out.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", REGISTER)
def test_frames_of_the_register_crowds(gpu, oracle, name):
    """The crowd*_r cases of tests/test_crowd_tiers.py have no frame of the reference's: a 37x19 frame against the oracle and every
    pipeline.  This is what shades a facet, hfacet, hdisk, hcylinder or orthotope behind a register-mask trace, 3-D to 12-D."""
    g = golden(name)
    gpu.upload_scene(g.scene)
    frame_equals_oracle(gpu, oracle, name, g.scene, g.depth)
    every_pipeline_renders_the_same(gpu, 37, 19, g.depth, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PADDED)
def test_scratch_stack_variants(gpu, oracle, capfd, name):
    """A scene padded to kd depth 40: section and a 41-level stack of 256 lanes are past 160 KB, so trace_rays and every frame
    kernel run the variants whose traversal stack is in scratch -- four mask words, and one word for c3_random4d.  The recorded
    reference answers, the oracle's frame of the scene as it was, every pipeline."""
    g = golden(name)
    fs = padded(name)
    got = upload(gpu, capfd, fs, name + " padded")
    assert got["depth"] == KD_STACK and got["tier"] == 0 and got["stack"] > LDS_LIMIT
    assert got["stack"] == ((got["words"] + 1) & ~1) * 8 + 256 * (got["depth"] + 1) * 12
    assert got["mask"] == {"c3_random4d": 1, "edge12d_65": 2, "edge3d_l256": 4}.get(name, 3) and got["items"] == g.scene.n_items
    assert len(g.data["kat_in"]) < 4096 * 64 and 37 * 19 < 1024 * 64            # (small launches: workgroups of 256 lanes)
    same_answers(gpu.trace_rays(g.data["kat_in"]), g.data["kat_out"], fs.dims, name + " padded")
    frame_equals_oracle(gpu, oracle, name, fs, g.depth, oracle_scene=g.scene)
    every_pipeline_renders_the_same(gpu, 37, 19, g.depth, name + " padded")
    # ... and as it was: the LDS-stack variants give the same answers
    plain = upload(gpu, capfd, g.scene, name)
    assert plain["stack"] <= LDS_LIMIT
    same_answers(gpu.trace_rays(g.data["kat_in"]), g.data["kat_out"], fs.dims, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PADDED_OVER)
def test_padding_past_64_kb_changes_the_tier(gpu, oracle, capfd, name):
    """The largest register crowds of 7-D and 12-D padded to kd depth 40: the added nodes take the section a few hundred bytes past
    64 KB, and the scene to tier 1 with fewer than five mask words.  Same answers, same frame."""
    g = golden(name)
    plain = upload(gpu, capfd, g.scene, name)
    fs = padded(name)
    got = upload(gpu, capfd, fs, name + " padded")
    assert plain["tier"] == 0 and 8 * plain["words"] <= 65536 < 8 * got["words"] < 65536 + 1024
    assert (got["tier"], got["mask"], got["depth"]) == (1, plain["mask"], KD_STACK)
    same_answers(gpu.trace_rays(g.data["kat_in"]), g.data["kat_out"], fs.dims, name + " padded")
    frame_equals_oracle(gpu, oracle, name, fs, g.depth, oracle_scene=g.scene)
    every_pipeline_renders_the_same(gpu, 37, 19, g.depth, name + " padded")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCAN_SCENES + ["edge3d_64", "edge3d_l256"])
def test_leaf_scan_window_edges(gpu, oracle, name):
    """One leaf of 1, 63, 64, 65, 127, 128, 129 and all items: the coherent leaf scan takes a list in windows of 64 entries.  The
    oracle's answers on that scene, whatever the smallest group that scans together, and without the scan.  On edge3d_64 the one
    list is bits 1 to 63 of an item set, on edge3d_l256 all four words of a register mask."""
    g = golden(name)
    rays = g.data["kat_in"]
    tier1 = name in SCAN_SCENES
    finite = g.scene.n_items - 1
    for length in WINDOW_LENGTHS:
        if length is not None and length >= finite:
            continue
        fs = one_leaf(copy_of(name), length)
        want = oracle.trace(fs, rays)
        assert (want[0] > 0).any()
        settings = [("leaf_scan_group", 1, 64), ("leaf_scan_group", 8, 64), ("leaf_scan_group", 64, 64), ("leaf_scan", 0, 1)] if tier1 else [("gate_prepass", 2, 2)]
        for option, other, default in settings:
            try:
                gpu.set_option(option, other)
                gpu.upload_scene(fs)
                identical(gpu.trace_rays(rays), want, "%s, one leaf of %s items, %s = %d" % (name, length, option, other))
            finally:
                gpu.set_option(option, default)
    gpu.upload_scene(g.scene)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["crowd3d_r", "crowd3d_gn"])
def test_reversed_lists_beyond_64_items(gpu, oracle, capfd, name):
    """Every leaf list reversed: another scan order, and lists that do not ascend -- no leaf history, the slab from the first leaf
    on (crowd3d_gn), the register kernel reading lists backwards (crowd3d_r).  The oracle's answers and frame for that order."""
    g = golden(name)
    rays = g.data["kat_in"]
    fs = reversed_lists(copy_of(name))
    want = oracle.trace(fs, rays)
    assert len(differing(want, g.data["kat_out"], fs.dims)) > 0              # (the order does matter to some ray)
    got = upload(gpu, capfd, fs, name + " reversed")
    assert got["tier"] == (1 if name.endswith("_gn") else 0)
    base = gpu.trace_rays(rays)
    identical(base, want, name + " reversed")
    frame_equals_oracle(gpu, oracle, name + " reversed", fs, g.depth)
    for history in (0, 1, 2, 3):
        try:
            gpu.set_option("leaf_history", history)
            gpu.upload_scene(fs)
            identical(gpu.trace_rays(rays), base, "%s reversed, leaf_history %d" % (name, history))
        finally:
            gpu.set_option("leaf_history", 4)
    gpu.upload_scene(g.scene)


@pytest.mark.gpu
def test_depth_limit_of_the_upload(gpu, capfd):
    """A tree of 40 levels uploads; one of 41 is refused with NDT_E_UNSUPPORTED and a message naming the depth, before anything of it
    reaches the device.  A refused upload leaves the context without a scene (ndt_hip_upload_scene), so nothing is rendered or traced
    until the scene from before is uploaded again: then it renders what it rendered."""
    from ndt_amd.hip import NdtHipError
    name = "edge3d_65"
    g = golden(name)
    assert upload(gpu, capfd, padded(name, KD_STACK), name + " padded")["depth"] == KD_STACK
    before, st_before = gpu.render(37, 19, g.depth)
    with pytest.raises(NdtHipError) as e:
        gpu.upload_scene(padded(name, KD_STACK + 1))
    assert e.value.code == NDT_E_UNSUPPORTED and "depth %d" % (KD_STACK + 1) in str(e.value), str(e.value)
    gpu.upload_scene(padded(name, KD_STACK))
    after, st_after = gpu.render(37, 19, g.depth)
    assert np.array_equal(after.view(np.uint64), before.view(np.uint64)) and counts(st_after) == counts(st_before)
