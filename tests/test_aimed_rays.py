"""Known-answer rays AIMED at every intersector of every dimension 3 .. 12 (tests/golden/aim_zoo*d, made by
tests/golden/make_golden_aimed.py from the compiled reference), and the zoo scenes of the two dimensions that had none.

The random / bounding-ball rays of the older fixtures do not meet thin objects above 5-D: in 10-D .. 12-D they are answered
by the hyperplane or by nothing.  These rays are aimed at the objects -- through them, from inside them, with distance limits
around the answer, grazing their silhouettes and edges, along degenerate directions, from their surfaces, from the far
side -- and the coverage they reach is asserted from the reference's own answers before anything is compared with them.
"""
import numpy as np
import pytest

from conftest import golden
from ndt_amd.flat_scene import OBJ_TYPES, OBJ_TYPE_ID

AIM_CASES = ["aim_zoo%dd" % n for n in range(3, 13)]
NEW_ZOO_CASES = ["zoo7d", "zoo8d"]          # (SMALL_CASES of conftest.py gives the older zoo cases the same checks)
CLASSES = "ABCDEF"
A, B, C, D, E, F = range(6)

MIN_PER_TYPE = 32
MIN_PER_CLASS = 8
# Class B (origin inside: the far root, the exit face) exists for the types that have an inside or a second root.  Left out,
# by name: hplane, hdisk, hfacet and facet are flat and their intersectors solve for ONE distance (hplane.c:39-75,
# hfacet.c:211-310, facet.c:166-269): there is no inside to start from and no other root to choose.  (The orthotope is flat too,
# but it is intersected as a slab of half-thickness sqrt(EPSILON) with two roots, orthotope.c:200-236: it has a class B.)
HAS_CLASS_B = ("sphere", "cylinder", "hcylinder", "orthotope", "hcube")

TOL_SPEC = 1e-4
TOL_TIGHT = 1e-9


def ref_dist(a, b):
    """|a - b| as the reference computes it (vectNd_dist: the squares summed in two lanes, even and odd components)."""
    diff = [float(x) - float(y) for x, y in zip(a, b)]
    s0, s1 = diff[0] * diff[0], diff[1] * diff[1]
    for i in range(2, len(diff), 2):
        s0 = s0 + diff[i] * diff[i]
        if i + 1 < len(diff):
            s1 = s1 + diff[i + 1] * diff[i + 1]
    return float(np.sqrt(np.float64(s0 + s1)))


def answered_types(g):
    """Type number of the object the REFERENCE answered each ray of an aimed fixture with (-1: nothing)."""
    obj = g.data["kat_out"][:, 1].astype(np.int64)
    types = np.array([o["type"] for o in g.scene.objects], dtype=np.int64)
    return np.where(obj >= 0, types[np.maximum(obj, 0)], -1)


def scene_types(g):
    return sorted({g.scene.objects[i]["type"] for i in range(g.scene.n_items)})


def coverage(g):
    """(type, class) -> rays of that class the reference answered with an object of that type."""
    t, c = answered_types(g), g.data["aim_class"]
    return {(ty, cl): int(((t == ty) & (c == cl)).sum()) for ty in scene_types(g) for cl in range(6)}


# ------------------------------------------------------------------------------------------------ CPU

@pytest.mark.parametrize("name", AIM_CASES)
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
    # the scene is the zoo case's own file, not a copy
    assert g.meta["scene_file"] == golden(g.meta["shares_scene_of"]).meta["scene_file"]
    # class C: the limits of one class-A ray stand right behind it, same origin and direction: limit 0, then -- if limit 0 was
    # answered by another, farther object that the scan meets first -- five limits around THAT object's distance, then five
    # around the distance t of the ray's own (nearest) answer, t itself included, in the reference's arithmetic
    firsts = np.flatnonzero((cls == C) & (sub == 0))
    assert len(firsts) >= g.scene.n_items
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
    assert ((rays[:, d:2 * d] == 0.0).any(axis=1) & e).sum() >= 10 * g.scene.n_items
    assert ((rays[:, d:2 * d] == 0.0).sum(axis=1)[e] == d - 1).sum() >= 2 * g.scene.n_items        # along a coordinate axis
    on_surface = np.flatnonzero(e & (sub == 3))
    assert len(on_surface) >= g.scene.n_items
    hits = {want[i, 2:2 + d].tobytes() for i in np.flatnonzero((cls == A) & (want[:, 0] == 1.0))}
    assert all(rays[i, :d].tobytes() in hits for i in on_surface)


@pytest.mark.parametrize("name", AIM_CASES)
def test_coverage_is_a_condition_of_the_fixture(name):
    """Counted from the REFERENCE's answers alone: every object type of the dimension's scene is the answer of at least 32
    rays, and of at least 8 in each of the classes A, B (where the type has one), C, D, E; at most half the rays miss."""
    g = golden(name)
    d = g.scene.dims
    present = [OBJ_TYPES[t] for t in scene_types(g)]
    expect = [t for t in OBJ_TYPES if t != "hcube" or d <= 10]           # (11-D and 12-D: the zoo without its hcube)
    assert present == expect, present
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
    assert not short, "%s: below the floor: %s" % (name, "; ".join(short))
    assert (answered_types(g) < 0).mean() <= 0.5
    # the limits of class C include every kind, and the fixture holds all three kinds of limit
    lim = g.data["kat_in"][:, 2 * d]
    assert (lim < 0).any() and (lim == 0).any() and (lim > 0).any()


def test_coverage_table():
    """type x dimension: rays of the aimed fixtures the reference answered with that type (shown under -s)."""
    rows = {t: [] for t in OBJ_TYPES + ["miss"]}
    for name in AIM_CASES:
        g = golden(name)
        t = answered_types(g)
        present = set(scene_types(g))
        for ty, tn in enumerate(OBJ_TYPES):
            rows[tn].append(int((t == ty).sum()) if ty in present else None)
        rows["miss"].append(int((t < 0).sum()))
    print("\naimed fixtures: rays answered per type (rows) and dimension (columns); -: not in that scene")
    print("%-10s" % "N" + "".join("%6d" % n for n in range(3, 13)))
    for tn, cells in rows.items():
        print("%-10s" % tn + "".join("%6s" % ("-" if c is None else c) for c in cells))
    for tn, cells in rows.items():
        if tn != "miss":
            assert all(c is None or c >= MIN_PER_TYPE for c in cells), (tn, cells)
    assert all(c is not None for tn in OBJ_TYPES if tn != "hcube" for c in rows[tn])
    assert [c is not None for c in rows["hcube"]] == [True] * 8 + [False] * 2


@pytest.mark.parametrize("name", AIM_CASES)
def test_oracle_reproduces_the_reference(oracle, name):
    """The CPU oracle against the compiled reference on every aimed ray, bit for bit (same glibc: no exception of any kind).
    Every *_vs_oracle test on the device inherits what the oracle gets wrong; this is where its blind cells are closed."""
    g = golden(name)
    rays, want = g.data["kat_in"], g.data["kat_out"]
    d = g.scene.dims
    obj, hit, nrm = oracle.trace(g.scene, rays)
    bad = np.flatnonzero((obj != want[:, 1].astype(np.int32)) | (hit != want[:, 2:2 + d]).any(axis=1) | (nrm != want[:, 2 + d:]).any(axis=1))
    assert len(bad) == 0, "%d rays differ, first: ray %d item %d class %s: oracle object %d, reference %d" % (
        len(bad), bad[0], g.data["aim_item"][bad[0]], CLASSES[g.data["aim_class"][bad[0]]], obj[bad[0]], int(want[bad[0], 1]))
    assert np.array_equal((obj >= 0).astype(np.float64), want[:, 0])


@pytest.mark.parametrize("name", NEW_ZOO_CASES)
def test_new_zoo_framebuffer_bit_exact(oracle, name):
    g = golden(name)
    out, st = oracle.render(g.scene, g.width, g.height, g.depth)
    ref = g.data["fb"]
    assert out.shape == ref.shape
    assert np.array_equal(out, ref), "max abs diff %g" % np.abs(out - ref).max()
    assert st.rays_ref_equiv == g.meta["rays_total"]
    assert st.rays_primary == g.width * g.height
    assert "hcube" in g.meta["objects"] and g.scene.dims in (7, 8)


# ------------------------------------------------------------------------------------------------ GPU

@pytest.fixture(scope="module")
def gpu():
    from ndt_amd.hip import NdtHip
    ctx = NdtHip(0)
    yield ctx
    ctx.close()


def same_answers(got, want, d, what):
    obj, hit, nrm = got
    bad = np.flatnonzero((obj != want[:, 1].astype(np.int32)) | (hit != want[:, 2:2 + d]).any(axis=1) | (nrm != want[:, 2 + d:]).any(axis=1))
    assert len(bad) == 0, "%s: %d rays differ from the reference, first: ray %d, device object %d, reference %d" % (
        what, len(bad), bad[0], obj[bad[0]], int(want[bad[0], 1]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", AIM_CASES)
def test_device_answers_are_the_references(gpu, name):
    """trace_rays on every aimed fixture: object ids exact, hit points and normals to the last bit.  (The facet's acos is
    ocml's on the device and glibc's in the reference; no ray of these fixtures is decided differently by it: no ray is
    excused.)"""
    g = golden(name)
    gpu.upload_scene(g.scene)
    got = gpu.trace_rays(g.data["kat_in"])
    print("%s: %d rays, 0 excused" % (name, len(got[0])))
    same_answers(got, g.data["kat_out"], g.scene.dims, name)


# option -> (the value that is not its default, its default).  hull_box / face_box / face_tree / face_groups act on scenes with an
# hcube (3-D .. 10-D; the tree and the groups on hcubes of more than 63 faces), item_sets on every zoo scene (at most 64 items).
# item_boxes, leaf_history and leaf_scan belong to the global-memory tier, which no zoo scene reaches (tests/test_item_boxes.py
# and test_leaf_history_changes_nothing drive them on the 6-D .. 8-D hypercubes): here they must be inert.  gate_prepass acts on
# the passes of a render, not on trace_rays: it is checked on a frame.
OPTIONS = [("hull_box", 0, 1), ("face_box", 0, 1), ("face_tree", 0, 1), ("face_groups", 0, 1), ("item_sets", 0, 1),
           ("item_boxes", 0, 1), ("leaf_history", 0, 4), ("leaf_scan", 0, 1), ("gate_prepass", 0, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", AIM_CASES)
def test_equivalent_paths_give_the_same_answers(gpu, name):
    g = golden(name)
    d = g.scene.dims
    has_hcube = any(o["type"] == OBJ_TYPE_ID["hcube"] for o in g.scene.objects[:g.scene.n_items])
    gpu.upload_scene(g.scene)
    frame, st = gpu.render(g.width, g.height, g.depth)
    counts = (st.rays_primary, st.rays_secondary, st.rays_shadow, st.rays_ref_equiv)
    for option, other, default in OPTIONS:
        if option in ("hull_box", "face_box", "face_tree", "face_groups") and not has_hcube:
            continue
        try:
            gpu.set_option(option, other)
            gpu.upload_scene(g.scene)
            same_answers(gpu.trace_rays(g.data["kat_in"]), g.data["kat_out"], d, "%s with %s = %d" % (name, option, other))
            if option == "gate_prepass":
                out, so = gpu.render(g.width, g.height, g.depth)
                assert np.array_equal(out, frame), option
                assert (so.rays_primary, so.rays_secondary, so.rays_shadow, so.rays_ref_equiv) == counts
        finally:
            gpu.set_option(option, default)
    gpu.upload_scene(g.scene)
    same_answers(gpu.trace_rays(g.data["kat_in"]), g.data["kat_out"], d, name + " with the defaults restored")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aim_zoo4d", "aim_zoo8d", "aim_zoo12d"])
def test_answers_do_not_depend_on_who_shares_the_wavefront(gpu, name):
    """A ray's answer is its own: whatever the 63 other lanes of its wavefront are doing.  The fixture in a seeded permutation;
    batches of 1, 63, 64, 65 and 127 rays cut from it; a batch of one item's rays alone (every lane in the same intersector)
    and a batch that deals all items round-robin (neighbouring lanes in different ones)."""
    g = golden(name)
    d = g.scene.dims
    rays, want, item = g.data["kat_in"], g.data["kat_out"], g.data["aim_item"]
    n = len(rays)
    gpu.upload_scene(g.scene)
    full = gpu.trace_rays(rays)
    same_answers(full, want, d, name)
    rng = np.random.default_rng(2024 + d)
    perm = rng.permutation(n)
    same_answers(gpu.trace_rays(rays[perm]), want[perm], d, name + " permuted")
    for size in (1, 63, 64, 65, 127):
        for begin in (0, 1, n // 3, int(rng.integers(0, n - size)), n - size):
            same_answers(gpu.trace_rays(rays[begin:begin + size]), want[begin:begin + size], d, "%s[%d:%d]" % (name, begin, begin + size))
    per_item = [np.flatnonzero(item == i) for i in range(g.scene.n_items)]
    alone = {}
    for i, idx in enumerate(per_item):
        got = gpu.trace_rays(rays[idx])
        same_answers(got, want[idx], d, "%s, the rays of item %d alone" % (name, i))
        for k, r in enumerate(idx):
            alone[int(r)] = (got[0][k], got[1][k], got[2][k])
    depth = min(len(idx) for idx in per_item)
    dealt = np.array([idx[k] for k in range(depth) for idx in per_item])
    assert len(set(item[dealt[:g.scene.n_items]].tolist())) == g.scene.n_items
    got = gpu.trace_rays(rays[dealt])
    same_answers(got, want[dealt], d, name + " dealt round-robin")
    for k, r in enumerate(dealt):
        a = alone[int(r)]
        assert a[0] == got[0][k] and np.array_equal(a[1], got[1][k]) and np.array_equal(a[2], got[2][k]), (name, int(r))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NEW_ZOO_CASES)
def test_new_zoo_framebuffer_vs_reference_golden(gpu, name):
    g = golden(name)
    gpu.upload_scene(g.scene)
    out, st = gpu.render(g.width, g.height, g.depth)
    ref = g.data["fb"]
    diff = np.abs(out - ref)
    assert diff.max() < TOL_SPEC, "max abs diff %g" % diff.max()
    assert (diff > TOL_TIGHT).sum() == 0, "%d values differ by more than %g (max %g)" % (
        (diff > TOL_TIGHT).sum(), TOL_TIGHT, diff.max())
    assert st.rays_ref_equiv == g.meta["rays_total"]
    assert st.rays_primary == g.width * g.height


@pytest.mark.gpu
@pytest.mark.parametrize("name", NEW_ZOO_CASES)
def test_new_zoo_framebuffer_vs_oracle(gpu, oracle, name):
    g = golden(name)
    gpu.upload_scene(g.scene)
    w, h = g.width - 3, g.height - 5             # not a multiple of the 8x8 tile
    out, st = gpu.render(w, h, g.depth)
    want, so = oracle.render(g.scene, w, h, g.depth)
    diff = np.abs(out - want)
    assert diff.max() < TOL_TIGHT, "max abs diff %g" % diff.max()
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow, st.rays_ref_equiv) == (
        so.rays_primary, so.rays_secondary, so.rays_shadow, so.rays_ref_equiv)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NEW_ZOO_CASES)
def test_new_zoo_through_every_pipeline(gpu, name):
    g = golden(name)
    gpu.upload_scene(g.scene)
    outs = []
    try:
        # (the last: the per-bounce pipeline with every launch on the one stream, light_overlap 0)
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
        assert np.array_equal(img, outs[0][0])
        assert counts == outs[0][1]
    assert np.abs(outs[0][0] - g.data["fb"]).max() < TOL_TIGHT
