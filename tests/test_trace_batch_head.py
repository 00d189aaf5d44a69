"""The head of a k_trace batch.  What moved may not change a bit of any answer:

  * the light origin of a shadow segment is found once per wavefront, lane s for segment s, and a batch takes it from that lane
    (it was found at the head of every shadow batch).  Segment number and light index differ wherever an ambient light stands in
    front of a light: the scene below has one first and one in the middle of the list.
  * the inverse directions of trace_kd are made behind the root box test, by the rays that enter the tree.
  * the LDS tiers read a batch's TracePart -- and the PRIM variant primary_node's workspace and geometry -- from the
    kernel-argument segment: every frame below goes through it.
  * frames whose first bounce is a whole number of k_shade_emit workgroups and a partial one, a single partial workgroup, and
    the overflow-and-retry path behind shade_emit(0), as plain tests of that launch.

What the frames are held to.  The parent's behaviour, bit for bit: the frame kernel (pipeline 2, k_frame_stream) takes none of the
three changes -- its rows of the resource table are the parent's -- and the suite's invariant is that every pipeline
renders the same bytes (test_gpu_parity.py: test_every_pipeline_renders_the_same_frame); so every per-bounce frame below must be
the frame kernel's frame to the last bit, and so must every option setting be every other's.  The trace_kd answers are the
oracle's bit for bit.  The oracle's FRAME is not the device's bit for bit, on the parent either: measured on the MI355X, per-bounce
pipeline, max |device - oracle| and values that differ --
    mixed lights 16x9 2.8e-17 (3 of 576), 64x36 1.1e-16 (108 of 9 216); without the spot light 1.4e-16 (6), 2.2e-16 (120);
    c1_hypercube3d 65x33 1.1e-16 (83 of 8 580), 16x9 1.1e-16 (3); c3_random4d 65x33 2.2e-16 (13), 16x9 1.7e-16 (2);
    the same frames with specular off: 8.3e-17, 3.3e-16, 5.6e-17, 2.8e-16, 1.1e-16, 1.1e-16, 5.6e-17, 1.1e-16
-- all colour values lie in [0, 1], so these are 1.5 ulps of 1.0 at the most; nine pixels in a thousand differ at all.  The device
takes acos / pow / sin / cos from ocml, the oracle from glibc (test_gpu_parity.py).  The bound is therefore in ulps, worked out and
not measured: a colour value is a sum of at most 24 lit terms (4 shadow lights x 2 libm results each, diffuse and specular, x 3
bounces that weigh more than 1 / 512 of a pixel), every term at most the value 1.0 and off by at most 4 ulps of itself (two
libraries, 2 ulps each): ORACLE_ULPS = 4 x 24 = 96 ulps of max(1, largest value), 2.1e-14.  The ray counts are equal.

Needs a real MI355X: run with `pytest -m gpu`.
"""
import os

import numpy as np
import pytest

from conftest import golden, GOLDEN

pytestmark = pytest.mark.gpu

ORACLE_ULPS = 96        # device frame against the oracle's, in ulps of max(1, largest colour value): see above
GRAZE = 1e-9


def fresh(name):
    """A copy of a fixture's scene of its own (golden() shares its scene)."""
    from ndt_amd import load_scene
    return load_scene(os.path.join(GOLDEN, name + ".ndtscene.gz"))


def counts(st):
    return (st.rays_primary, st.rays_secondary, st.rays_shadow, st.rays_ref_equiv)


def same_bits(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: %d values differ" % (what, int((a != b).sum()))


def same_as_oracle(out, st, want, wst, what):
    diff = float(np.abs(out - want).max())
    tol = ORACLE_ULPS * np.finfo(np.float64).eps * max(1.0, float(np.abs(want).max()))
    print("%s: max |device - oracle| = %g, %d of %d values differ (bound %g)" % (what, diff, int((out != want).sum()), out.size, tol))
    assert diff <= tol, "%s: max abs diff %g, bound %g" % (what, diff, tol)
    assert counts(st) == counts(wst), what


# ------------------------------------------------------------------ segment constants

def mixed_lights(fs):
    """fs with the light list ambient, point, spot, ambient, directional, point: shadow segments 0 .. 3 are list entries 1, 2, 4, 5."""
    d = fs.dims
    own = [dict(l) for l in fs.lights if l["type"] != 0]
    anchors = [fs.vec(l["pos_off"]) for l in own if l["pos_off"] >= 0] or [np.zeros(d)]
    dirs = [fs.vec(l["dir_off"]) for l in own if l["dir_off"] >= 0]
    down = np.zeros(d)
    down[1] = -1.0
    aim = dirs[0] if dirs else down
    src = own[0] if own else dict(red=200.0, green=200.0, blue=200.0)
    r, g, b = 0.3 * src["red"], 0.3 * src["green"], 0.3 * src["blue"]
    shift = np.zeros(d)
    shift[0], shift[d - 1] = 2.5, -1.5

    def ambient(k):
        return dict(type=0, red=0.01 * k, green=0.012, blue=0.008, angle=0.0, pos_off=-1, dir_off=-1, area_off=-1, radius=0.0)

    fs.lights = [
        ambient(1),
        dict(type=1, red=r, green=g, blue=b, angle=0.0, pos_off=fs.add_vec(list(anchors[0])), dir_off=-1, area_off=-1, radius=0.0),
        dict(type=3, red=1.2 * r, green=0.8 * g, blue=b, angle=35.0, pos_off=fs.add_vec(list(anchors[0] + shift)),
             dir_off=fs.add_vec(list(aim)), area_off=-1, radius=0.0),
        ambient(2),
        dict(type=2, red=0.2, green=0.25, blue=0.3, angle=0.0, pos_off=-1, dir_off=fs.add_vec(list(aim + 0.2 * shift)), area_off=-1,
             radius=0.0),
        dict(type=1, red=0.7 * r, green=g, blue=1.1 * b, angle=0.0, pos_off=fs.add_vec(list(anchors[-1] - shift)), dir_off=-1,
             area_off=-1, radius=0.0),
    ]
    fs._struct = None
    fs.finalize()
    return fs


@pytest.fixture(scope="module")
def gpu():
    from ndt_amd.hip import NdtHip
    ctx = NdtHip(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def lit_scene():
    return mixed_lights(fresh("zoo4d"))


def frame_kernel(gpu, fs, w, h, depth):
    """The frame as the frame kernel renders it (pipeline 2), which takes none of the changes to k_trace."""
    gpu.set_option("pipeline", 2)
    gpu.set_option("light_window", 0)
    gpu.upload_scene(fs)
    return gpu.render(w, h, depth)


@pytest.mark.parametrize("size", [(16, 9), (64, 36)])
def test_segment_constants(gpu, oracle, lit_scene, size):
    """-l 3 with the per-bounce pipeline: light_overlap 0 and 1, then light_window 2 (three windows: launches that trace shadow
    rays only) -- the oracle's frame and ray counts, and under every setting the bytes of the frame kernel's frame."""
    w, h = size
    want, wst = oracle.render(lit_scene, w, h, 3)
    assert wst.rays_shadow > 0
    frames = []
    try:
        gpu.set_option("pipeline", 1)
        for overlap, window in ((0, 0), (1, 0), (0, 2), (1, 2)):
            gpu.set_option("light_overlap", overlap)
            gpu.set_option("light_window", window)
            gpu.upload_scene(lit_scene)
            out, st = gpu.render(w, h, 3)
            what = "%dx%d light_overlap %d light_window %d" % (w, h, overlap, window)
            same_as_oracle(out, st, want, wst, what)
            frames.append((what, out))
        parent = frame_kernel(gpu, lit_scene, w, h, 3)
    finally:
        gpu.set_option("light_window", 0)
        gpu.set_option("light_overlap", 1)
        gpu.set_option("pipeline", 0)
    for what, out in frames:
        same_bits(parent[0], out, what + " against the frame kernel")


# ------------------------------------------------------------------ lazy inverses

def box_test(lo, hi, o, v):
    """aabb_intersect of the root box (kd-tree.c:84-127) as trace_kd does it, in the same IEEE operations."""
    EPS, EPS2 = 1e-4, 1e-8
    tl, tu = -np.finfo(np.float64).max, np.finfo(np.float64).max
    for i in range(len(lo)):
        if not abs(v[i]) < EPS2:
            a, b = (lo[i] - o[i]) / v[i], (hi[i] - o[i]) / v[i]
            if a > b:
                a, b = b, a
            tl, tu = max(tl, a), min(tu, b)
            if tu < -EPS:
                return False
    tl -= EPS
    tu += EPS
    return bool(tu >= -EPS and tl <= tu)


def margin(lo, hi, o, v):
    """How far the ray o + t v, t >= 0, stays from the surface of the box [lo, hi]: its distance to the box if it never touches
    it, else the depth it reaches inside (the largest distance to the surface of any of its points in the box).  Under GRAZE:
    the ray grazes the box."""
    n = len(lo)
    # candidates: t = 0, every crossing of a face plane, the stationary point of the distance in every piece between them, and
    # every t where two of the 2n face distances are equal (the depth, a minimum of linear functions, peaks there)
    ts = [0.0]
    planes = [(i, b) for i in range(n) for b in (lo[i], hi[i])]
    for i, b in planes:
        if v[i] != 0.0:
            ts.append((b - o[i]) / v[i])
    cuts = sorted(t for t in ts if t >= 0.0)
    for a, b in zip(cuts, cuts[1:] + [cuts[-1] + 1.0]):
        p = o + 0.5 * (a + b) * v
        out = [(i, lo[i] if p[i] < lo[i] else hi[i]) for i in range(n) if p[i] < lo[i] or p[i] > hi[i]]
        den = sum(v[i] * v[i] for i, _ in out)
        if den > 0.0:
            ts.append(-sum((o[i] - bnd) * v[i] for i, bnd in out) / den)
    lin = [(o[i] - lo[i], v[i]) for i in range(n)] + [(hi[i] - o[i], -v[i]) for i in range(n)]      # distance to a face: c + t s
    for k, (c1, s1) in enumerate(lin):
        for c2, s2 in lin[k + 1:]:
            if s1 != s2:
                ts.append((c2 - c1) / (s1 - s2))
    dist, depth = np.inf, -np.inf
    for t in ts:
        if not 0.0 <= t < 1e30:         # (a component of 1e-300 meets its face planes beyond anything a double can square)
            continue
        p = o + t * v
        gap = np.maximum(np.maximum(lo - p, p - hi), 0.0)
        dist = min(dist, float(np.sqrt((gap * gap).sum())))
        depth = max(depth, float(np.minimum(p - lo, hi - p).min()))
    return depth if dist == 0.0 else dist


def box_rays(fs, seed):
    """(rays, kinds): rays around the root box of fs.  kinds: 'miss', 'graze', 'zero' (a direction component exactly 0), 'tiny'
    (one below 1e-8 in magnitude, the clamp of inv_of, or just above it), 'inside' (origin in the box)."""
    rng = np.random.default_rng(seed)
    d = fs.dims
    lo, hi = fs.vec(fs.bb["lower"]), fs.vec(fs.bb["upper"])
    c, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    rays, kinds = [], []

    def add(kind, o, v, lim=-1.0):
        rays.append(np.concatenate([o, v, [lim]]))
        kinds.append(kind)

    def unit(v):
        return v / np.sqrt((v * v).sum())

    for k in range(40):
        # beside the box, three half-sizes out along axis i, running along axis j with a tilt that cannot bring it back
        i, j = k % d, (k + 1 + k // d) % d
        if j == i:
            j = (i + 1) % d
        sign = 1.0 if k & 1 else -1.0
        o = c + rng.uniform(-0.5, 0.5, d) * half
        o[i] = c[i] + sign * 3.0 * half[i]
        o[j] = c[j] - 4.0 * half[j]
        v = rng.uniform(-0.05, 0.05, d)
        v[j] = 1.0
        v[i] = sign * abs(v[i])
        add("miss", o, unit(v))
    for k in range(48):
        # along a face, exactly in its plane or up to 8e-10 off it on either side: parallel to the face (a zero component) or
        # past an edge at that distance (no zero component)
        i, j = k % d, (k + 1) % d
        off = (0.0, 1e-12, -1e-12, 2e-10, -2e-10, 8e-10, -8e-10, 5e-11)[k % 8]
        top = bool((k // 8) & 1)
        o = c + rng.uniform(-0.6, 0.6, d) * half
        if k % 3:
            o[i] = (hi[i] if top else lo[i]) + off
            o[j] = c[j] - 3.0 * half[j]
            v = np.zeros(d)
            v[j] = 1.0
        else:
            # through the point `off` outside the edge (i at its bound, j at its lower bound), at right angles to the outward diagonal
            s = 1.0 if top else -1.0
            q = o.copy()
            q[i] = (hi[i] if top else lo[i]) + s * off * np.sqrt(0.5)
            q[j] = lo[j] - off * np.sqrt(0.5)
            v = np.zeros(d)
            v[i], v[j] = s * np.sqrt(0.5), np.sqrt(0.5)
            o = q - 2.0 * half[j] * v
        add("graze", o, v)
    for k in range(40):
        # from outside at the box, some components exactly zero (the origin then inside the slabs of those axes)
        o = c + unit(rng.normal(size=d)) * 3.0 * np.sqrt((half * half).sum())
        zero = rng.random(d) < 0.4
        zero[k % d] = True
        zero[(k + 1) % d] = False
        o[zero] = c[zero] + rng.uniform(-0.9, 0.9, int(zero.sum())) * half[zero]
        v = c + rng.uniform(-0.5, 0.5, d) * half - o
        v[zero] = 0.0 if k & 1 else -0.0
        add("zero", o, unit(v))
    tiny = (1e-9, -1e-9, 5e-9, -5e-9, 9.9e-9, -9.9e-9, 1e-8, -1e-8, 1.1e-8, -1.1e-8, 1e-300, -1e-300)
    for k in range(48):
        o = c + unit(rng.normal(size=d)) * 3.0 * np.sqrt((half * half).sum())
        a = k % d
        o[a] = c[a] + rng.uniform(-0.9, 0.9) * half[a]
        v = unit(c + rng.uniform(-0.5, 0.5, d) * half - o)
        v[a] = tiny[k % len(tiny)]
        add("tiny", o, v)
    for k in range(48):
        o = c + rng.uniform(-0.98, 0.98, d) * half
        v = unit(rng.normal(size=d))
        if k % 4 == 1:
            v[k % d] = 0.0
        elif k % 4 == 2:
            v[k % d] = tiny[k % len(tiny)]
        add("inside", o, v, -1.0 if k % 6 else 0.5 * float(half.max()))
    return np.array(rays), kinds


_box_cases = {}


def box_case(oracle, name):
    """The rays of a scene and the oracle's answers, made once."""
    if name not in _box_cases:
        fs = golden(name).scene
        rays, kinds = box_rays(fs, 14)
        _box_cases[name] = (fs, rays, kinds, oracle.trace(fs, rays))
    return _box_cases[name]


BOX_SCENES = ["zoo3d_mirror", "zoo4d", "zoo6d"]


@pytest.mark.parametrize("name", BOX_SCENES)
def test_box_rays_cover_both_sides(oracle, name):
    """On the CPU, the oracle alone: at least 32 rays pass the root box test and at least 32 fail it, a ray that fails it hits
    nothing where the scene has no infinite objects (the 3-D scene has three: its rays scan them before the box is tested), and
    every ray that stays within 1e-9 of the box surface is in the grazing set."""
    fs, rays, kinds, (obj, hit, nrm) = box_case(oracle, name)
    d = fs.dims
    lo, hi = fs.vec(fs.bb["lower"]), fs.vec(fs.bb["upper"])
    enters = np.array([box_test(lo, hi, r[:d], r[d:2 * d]) for r in rays])
    assert enters.sum() >= 32 and (~enters).sum() >= 32, (int(enters.sum()), int((~enters).sum()))
    if not fs.inf_refs:
        assert (obj[~enters] < 0).all()
    assert (obj >= 0).sum() >= 32
    near = np.array([margin(lo, hi, r[:d], r[d:2 * d]) < GRAZE for r in rays])
    graze = np.array([k == "graze" for k in kinds])
    assert near[graze].all(), "%d rays of the grazing set are not within %g of the surface" % (int((~near[graze]).sum()), GRAZE)
    assert not near[~graze].any(), "%d rays within %g of the surface are not in the grazing set" % (int(near[~graze].sum()), GRAZE)
    for kind in ("miss", "graze", "zero", "tiny", "inside"):
        assert kinds.count(kind) >= 32, kind
    v = rays[:, d:2 * d]
    assert ((v == 0.0).any(axis=1)).sum() >= 32 and (((np.abs(v) < 1e-8) & (v != 0.0)).any(axis=1)).sum() >= 32


@pytest.mark.parametrize("batch", [1, 63, 64, 65])
@pytest.mark.parametrize("name", BOX_SCENES)
def test_lazy_inverses(gpu, oracle, name, batch):
    """ndt_hip_trace_rays, `batch` rays a call: the oracle's object, hit point and normal, bit for bit."""
    fs, rays, kinds, (obj, hit, nrm) = box_case(oracle, name)
    gpu.upload_scene(fs)
    got = [gpu.trace_rays(rays[k:k + batch]) for k in range(0, len(rays), batch)]
    g_obj, g_hit, g_nrm = (np.concatenate([g[i] for g in got]) for i in range(3))
    bad = np.flatnonzero(g_obj != obj)
    assert bad.size == 0, "objects differ at rays %s (%s)" % (bad[:8], [kinds[k] for k in bad[:8]])
    same_bits(hit, g_hit, "%s hit points, batch %d" % (name, batch))
    same_bits(nrm, g_nrm, "%s normals, batch %d" % (name, batch))


# ------------------------------------------------------------------ shade_emit of the primaries' bounce

@pytest.mark.parametrize("size", [(65, 33), (16, 9)])
@pytest.mark.parametrize("name", ["c1_hypercube3d", "c3_random4d"])
def test_emit_partial_workgroups(gpu, oracle, name, size):
    """65 x 33 = 2 145 primaries: whole workgroups of k_shade_emit and a partial one; 16 x 9: one partial workgroup."""
    g = golden(name)
    w, h = size
    want, wst = oracle.render(g.scene, w, h, g.depth)
    try:
        gpu.set_option("pipeline", 1)
        gpu.upload_scene(g.scene)
        out, st = gpu.render(w, h, g.depth)
        parent = frame_kernel(gpu, g.scene, w, h, g.depth)
    finally:
        gpu.set_option("pipeline", 0)
    same_as_oracle(out, st, want, wst, "%s %dx%d" % (name, w, h))
    same_bits(parent[0], out, "%s %dx%d against the frame kernel" % (name, w, h))
    assert counts(parent[1]) == counts(st)


@pytest.mark.parametrize("name", ["c1_hypercube3d", "c3_random4d"])
def test_emit_overflow_and_retry(gpu, oracle, name):
    """A fresh context whose first node pool holds the primaries and 64 nodes: the frame overflows behind shade_emit(0), the
    pools grow and the frame is rendered again -- the oracle's frame, and the bytes of a context that never overflowed."""
    from ndt_amd.hip import NdtHip
    g = golden(name)
    w, h = 65, 33
    want, wst = oracle.render(g.scene, w, h, g.depth)
    try:
        gpu.set_option("pipeline", 1)
        gpu.upload_scene(g.scene)
        plain, pst = gpu.render(w, h, g.depth)
        parent = frame_kernel(gpu, g.scene, w, h, g.depth)
    finally:
        gpu.set_option("pipeline", 0)
    small = NdtHip(0)
    try:
        small.set_option("pipeline", 1)
        small.set_option("test_small_pool", 1)
        small.upload_scene(g.scene)
        out, st = small.render(w, h, g.depth)
        again, ast = small.render(w, h, g.depth)
    finally:
        small.close()
    assert wst.rays_secondary > 64                      # the small pool cannot hold them
    assert st.node_capacity >= wst.rays_primary + wst.rays_secondary
    same_as_oracle(out, st, want, wst, "%s, small pool" % name)
    same_bits(parent[0], plain, "%s against the frame kernel" % name)
    same_bits(plain, out, "%s, small pool against a plain context" % name)
    same_bits(plain, again, "%s, the frame after the retry" % name)
    assert counts(ast) == counts(pst)
