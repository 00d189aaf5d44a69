#!/usr/bin/env python3
"""Generate the AIMED known-answer fixtures aim_zoo{3..12}d from the COMPILED REFERENCE.

    make -C oracle ref oracle
    python tests/golden/make_golden_aimed.py [aim_zoo7d ...]

make_golden.py's known-answer rays are drawn at random in the scene box or aimed into an item's bounding ball; above
5-D neither meets a thin object (a plate, a triangle, a disk, a face of the hcube) often enough to test its intersector.
The rays made here are aimed at the objects themselves, per kd item and, for the hcube, per face of a seeded sample of
its faces.  Every fixture reuses the scene file of that dimension's zoo case (no second copy is written) and stores

    kat_in    (n, 2 d + 1)   origin, unit direction, distance limit            } the layout of the other
    kat_out   (n, 2 d + 2)   the reference's trace_kd: ret, object, hit, normal } known-answer fixtures
    aim_item  (n,) int32     the kd item the ray was made for
    aim_class (n,) int8      0 .. 5 = A .. F, below
    aim_sub   (n,) int8      the variant inside the class (what the epsilon was, which limit, ...; SUB_* below)

Classes (per item; the rays of a class that start outside start at the camera or at seeded points outside the item's
bounding sphere and above the floor):
  A through   the target is a point of the object; limit -1
  B inside    the origin is inside the object (ball, tube, the hcube's hull, the EPS-thick slab of a plate): the far root
  C limits    a class-A ray whose reference answer lies at distance t, again with limit 0, t (1 -+ 1e-3), the doubles next
              to t on either side and t itself (the shadow-ray semantics: the limit ends the scan, ndt.c:184-188); and,
              where limit 0 is answered by a farther object that the scan meets first, the same five around ITS distance
  D grazing   closest approach r (1 +- eps) to a centre / an axis, eps = 1e-3 and 1e-9; for the flat types a point
              eps inside / outside an edge, and the vertices; for the hplane a direction eps off parallel
  E degenerate directions with exactly-zero components (kd-tree.c:583-588), exactly perpendicular to a normal that
              has zero components, along a cylinder's axis; and origins ON a surface: a class-A hit point, reflected
  F far side  a class-A ray's target from the opposite side

Only data is written (.json, .npz); the archives are written with fixed time stamps, so a second run reproduces them byte
for byte.  `answers` is the only door to the reference: oracle/_ref/ndt_ref_shim --rays-in / --rays-out.
"""
import io
import json
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from ndt_amd import load_scene  # noqa: E402
from ndt_amd.flat_scene import OBJ_TYPE_ID  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
SHIM = os.path.join(REF, "ndt_ref_shim")

# fixture -> the zoo case whose scene it shares (make_golden.py: CASES) and how the reference builds that scene
AIMED = {
    "aim_zoo3d": dict(share="zoo3d_mirror", dims=3, config="mirror"),
    "aim_zoo4d": dict(share="zoo4d", dims=4),
    "aim_zoo5d": dict(share="zoo5d_f2", dims=5, frame=2),
    "aim_zoo6d": dict(share="zoo6d", dims=6),
    "aim_zoo7d": dict(share="zoo7d", dims=7),
    "aim_zoo8d": dict(share="zoo8d", dims=8),
    "aim_zoo9d": dict(share="zoo9d", dims=9),
    "aim_zoo10d": dict(share="zoo10d", dims=10),
    "aim_zoo11d": dict(share="zoo11d", dims=11, config="nohcube"),
    "aim_zoo12d": dict(share="zoo12d", dims=12, config="nohcube"),
}

A, B, C, D, E, F = range(6)
# aim_sub: class D: the epsilon; class C: the limit; class E: the kind of degeneracy; otherwise where the ray starts
SUB_CAMERA, SUB_OUTSIDE = 0, 1
SUB_EPS3_IN, SUB_EPS3_OUT, SUB_EPS9_IN, SUB_EPS9_OUT, SUB_VERTEX = 0, 1, 2, 3, 4
SUB_LIM0, SUB_LIM_BELOW, SUB_LIM_ABOVE, SUB_LIM_PREV, SUB_LIM_NEXT, SUB_LIM_EXACT = 0, 1, 2, 3, 4, 5
SUB_FIRST_BELOW, SUB_FIRST_ABOVE, SUB_FIRST_PREV, SUB_FIRST_NEXT, SUB_FIRST_EXACT = 6, 7, 8, 9, 10
SUB_ZEROS, SUB_PERP, SUB_AXIS, SUB_SURFACE = 0, 1, 2, 3
EPS_SUBS = ((1e-3, SUB_EPS3_IN, SUB_EPS3_OUT), (1e-9, SUB_EPS9_IN, SUB_EPS9_OUT))

T = OBJ_TYPE_ID
REF_EPS = 1e-4            # the reference's EPSILON (object.h:15)
HCUBE_FACES = 96          # faces of the hcube that get rays of their own (all of them where it has fewer)
C_PER_ITEM = 14           # class-A answers per item (per face sample: 1) that get the five limits
SURF_PER_ITEM = 10        # class-A answers per item that are reused as origins


def ref_dist(a, b):
    """|a - b| in the reference's own arithmetic (vectNd_dist: the dot product summed in two lanes, even and odd components,
    vectNd.h:215-227), so that a limit can be made EQUAL to the distance the reference compares it with."""
    diff = [float(x) - float(y) for x, y in zip(a, b)]
    s0, s1 = diff[0] * diff[0], diff[1] * diff[1]
    for i in range(2, len(diff), 2):
        s0 = s0 + diff[i] * diff[i]
        if i + 1 < len(diff):
            s1 = s1 + diff[i + 1] * diff[i + 1]
    return float(np.sqrt(np.float64(s0 + s1)))


def around(t, subs):
    return list(zip((t * (1 - 1e-3), t * (1 + 1e-3), float(np.nextafter(t, 0.0)), float(np.nextafter(t, np.inf)), t), subs))


def unit(v):
    return v / np.linalg.norm(v)


def rand_unit(rng, d):
    return unit(rng.standard_normal(d))


def complement(rng, d, rows):
    """A random orthonormal basis (as rows) of the orthogonal complement of the given vectors."""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    m = np.concatenate([rows, rng.standard_normal((d - np.linalg.matrix_rank(rows), d))])
    q, _ = np.linalg.qr(m.T)
    return q.T[np.linalg.matrix_rank(rows):]


class Item:
    """What the generator knows of one kd item (or of one face of the hcube): points of it, points in it, its silhouette."""

    def __init__(self, fs, idx, owner=None):
        d = fs.dims
        o = fs.objects[idx]
        self.fs, self.d, self.idx, self.type = fs, d, idx, o["type"]
        self.item = idx if owner is None else owner
        self.pos = np.array([fs.vec(o["pos_off"] + k * d) for k in range(o["n_pos"])]).reshape(-1, d)
        self.dir = np.array([fs.vec(o["dir_off"] + k * d) for k in range(o["n_dir"])]).reshape(-1, d)
        self.size = np.array(fs._sizes[o["size_off"]:o["size_off"] + o["n_size"]])
        self.flag = list(fs._flags[o["flag_off"]:o["flag_off"] + o["n_flag"]])
        b = fs.objects[self.item]
        self.bc, self.br = fs.vec(b["bounds_center_off"]), b["bounds_radius"]
        if self.type == T["cylinder"]:
            self.axes = np.array([unit(self.pos[1] - self.pos[0])])
            self.lens = np.array([np.linalg.norm(self.pos[1] - self.pos[0])])
        elif self.type == T["hcylinder"]:
            self.axes = np.array([unit(p - self.pos[0]) for p in self.pos[1:d - 1]])
            self.lens = np.array([np.linalg.norm(p - self.pos[0]) for p in self.pos[1:d - 1]])
        elif self.type == T["orthotope"]:
            self.m = self.flag[0]
            self.axes = np.array([unit(v) for v in self.dir[:self.m]])
            self.lens = np.array([np.linalg.norm(v) for v in self.dir[:self.m]])
        if self.type in (T["cylinder"], T["hcylinder"], T["orthotope"]):
            # What the reference takes for "the part of x - pos outside the axes' span" is x - pos minus the SUM of its
            # projections on the single axes (cylinder.c, hcylinder.c:159-185, orthotope.c:175-199).  With skew axes that is
            # not the orthogonal projection: a point pos + s.axes of the span itself is left with the residual
            # axes^T (G - I) s, G the axes' Gram matrix.  So the object the reference intersects is the flat (or tube) only
            # along the null space of G - I, and bounded in the other directions of the span: the zoo's plate and the faces
            # of its skewed hcube are specks and strips, not parallelograms.  Rays are aimed at what the reference sees.
            self.gram = self.axes @ self.axes.T
            lam, vec = np.linalg.eigh(self.gram - np.eye(len(self.axes)))
            free = vec[:, np.abs(lam) < 1e-9]
            self.free = free @ free.T
            self.budget = 0.6 * self.size[0] if self.type != T["orthotope"] else 0.5 * np.sqrt(REF_EPS)

    def skew(self, s):
        """The residual the reference's sum of projections leaves of the point pos + s.axes of the axes' span."""
        return ((self.gram - np.eye(len(s))) @ s) @ self.axes

    def span_point(self, rng, lo=0.1, hi=0.9):
        """Coefficients s (along the unit axes) of a point of the axes' span that the reference counts as within the extents
        (0 < (G s)_i < length_i; hcylinder.c:101-130) and whose skew residual is within the budget: half the slab of a plate,
        0.6 of a tube's radius."""
        if self.type == T["cylinder"] and len(self.flag) > 1 and self.flag[1]:
            lo, hi = -1.5, 2.5          # the infinite one: beyond both end points too
        for attempt in range(400):
            s0 = rng.uniform(lo, hi, len(self.lens)) * self.lens
            # (the null space of G - I need not meet the box far from pos: its share shrinks from attempt to attempt, and
            # in the end the whole of s0 is scaled down into the budget)
            keep = self.free @ s0 * (0.9 ** attempt if attempt < 200 else 0.0)
            rest = s0 - keep
            res = np.linalg.norm(self.skew(rest))
            s = keep + rest * (min(1.0, self.budget / res) * rng.uniform(0.2, 1.0) if res > 0 else 1.0)
            along = self.gram @ s
            if lo < 0 or (np.all(along > 0.0) and np.all(along < self.lens)):
                return s
        raise ValueError("no point of object %d found" % self.idx)

    # ---- a point of the object: a ray through it meets the object
    def surface(self, rng):
        t, d = self.type, self.d
        if t == T["sphere"]:
            return self.pos[0] + self.size[0] * 0.9 * rng.random() ** (1.0 / d) * rand_unit(rng, d)
        if t == T["hplane"]:
            w = complement(rng, d, self.dir[0])[0]
            return self.pos[0] + rng.uniform(0.0, 25.0) * w
        if t == T["hdisk"]:
            w = complement(rng, d, self.dir[0])[0]
            return self.pos[0] + self.size[0] * rng.uniform(0.0, 0.95) * w
        if t in (T["cylinder"], T["hcylinder"]):
            w = complement(rng, d, self.axes)[0]
            sc = self.span_point(rng)
            return self.pos[0] + sc @ self.axes + self.axis_radius(sc) * rng.uniform(0.0, 0.9) * w
        if t == T["orthotope"]:
            return self.pos[0] + self.span_point(rng) @ self.axes
        if t in (T["hfacet"], T["facet"]):
            w = rng.dirichlet(np.ones(3)) * 0.94 + 0.02
            return w @ self.pos[:3]
        raise ValueError("no surface for type %d" % t)

    def axis_radius(self, sc):
        """The radius left around the point pos + sc.axes in the plane normal to every axis, after the skew residual."""
        skew = self.skew(sc)
        return np.sqrt(max(self.size[0] ** 2 - skew @ skew, 0.0))

    # ---- an origin inside (class B), or None where the type has no inside and no far root
    def inside(self, rng):
        t, d = self.type, self.d
        if t in (T["sphere"], T["cylinder"], T["hcylinder"]):
            return self.surface(rng)
        if t == T["orthotope"]:
            # inside the slab of half-thickness sqrt(EPS) = 0.01 the quadratic gives the m-flat (orthotope.c:200)
            n = complement(rng, d, self.axes)[0]
            return self.surface(rng) + rng.uniform(-0.004, 0.004) * n
        if t == T["hcube"]:
            return self.pos[0] + (rng.uniform(-0.45, 0.45, d) * self.size[:d]) @ self.dir[:d]
        return None

    # ---- class D: (origin, direction, sub) whose closest approach is r (1 -+ eps), or (origin, target, sub) at an edge
    def grazing(self, rng):
        t, d = self.type, self.d
        out = []
        for eps, sub_in, sub_out in EPS_SUBS:
            for sign, sub in ((-1.0, sub_in), (1.0, sub_out)):
                for _ in range(6):
                    if t == T["sphere"]:
                        c, r = self.pos[0], self.size[0]
                        o = outside_origin(self, rng, c)
                        e = unit(c - o)
                        w = complement(rng, d, e)[0]
                        s = r * (1.0 + sign * eps) / np.linalg.norm(c - o)
                        out.append((o, unit(np.sqrt(1.0 - s * s) * e + s * w), None, sub))
                    elif t in (T["cylinder"], T["hcylinder"]):
                        sc = self.span_point(rng, 0.25, 0.75)
                        p = self.pos[0] + sc @ self.axes
                        r = self.axis_radius(sc)
                        basis = complement(rng, d, self.axes)
                        e, w = basis[0], basis[1]
                        dist = rng.uniform(6.0, 14.0)
                        s = r * (1.0 + sign * eps) / dist
                        out.append((p - dist * e, unit(np.sqrt(1.0 - s * s) * e + s * w), None, sub))
                    elif t == T["hdisk"]:
                        w = complement(rng, d, self.dir[0])[0]
                        out.append((None, None, self.pos[0] + self.size[0] * (1.0 + sign * eps) * w, sub))
                    elif t == T["hplane"]:
                        # eps off the threshold of "parallel": |v.n| against the reference's EPS (hplane.c:56), towards the
                        # plane from just above it
                        nrm = unit(self.dir[0])
                        w = complement(rng, d, nrm)[0]
                        o = self.surface(rng) + 0.002 * nrm
                        s = REF_EPS / np.linalg.norm(self.dir[0]) * (1.0 - sign * eps)
                        out.append((o, unit(np.sqrt(1.0 - s * s) * w - s * nrm), None, sub))
                    elif t == T["orthotope"]:
                        # a point of the plate moved along one axis until the reference's extent test (G s)_k stands eps
                        # outside / inside 0 -- or, along an axis no other axis is skew to, the far end
                        sc = self.span_point(rng, 0.15, 0.85)
                        k = int(rng.integers(0, self.m))
                        far = abs(self.free[k, k] - 1.0) < 1e-9 and rng.random() < 0.5
                        want = self.lens[k] * ((1.0 + sign * eps) if far else -sign * eps)
                        sc[k] += want - (self.gram @ sc)[k]
                        if np.linalg.norm(self.skew(sc)) < 0.8 * np.sqrt(REF_EPS):
                            out.append((None, None, self.pos[0] + sc @ self.axes, sub))
                    elif t in (T["hfacet"], T["facet"]):
                        w = rng.dirichlet(np.ones(2)) * (1.0 - sign * eps)
                        w = np.insert(w, rng.integers(0, 3), sign * eps)
                        out.append((None, None, w @ self.pos[:3], sub))
        if t == T["orthotope"]:
            for _ in range(4):
                # the vertices the reference can see: the far ends only of axes no other axis is skew to
                corner = rng.integers(0, 2, self.m) * (np.abs(np.diag(self.free) - 1.0) < 1e-9)
                out.append((None, None, self.pos[0] + (corner * self.lens) @ self.axes, SUB_VERTEX))
        if t in (T["hfacet"], T["facet"]):
            for k in (0, 1, 2, int(rng.integers(0, 3))):
                out.append((None, None, self.pos[k].copy(), SUB_VERTEX))
        return out

    def normal_with_zeros(self):
        """The normal of a flat type if some of its components are exactly zero (a direction that is exactly perpendicular
        to it can then be written down: zero wherever the normal is not)."""
        if self.type in (T["hplane"], T["hdisk"], T["facet"]) and len(self.dir):
            n = self.dir[0]
            if (n == 0.0).any() and (n != 0.0).any():
                return n
        return None


def outside_origin(it, rng, target, below_ok=False):
    """A seeded origin outside the item's bounding sphere (where it has one), 8 .. 25 from the target and above the floor
    (the zoo's hplane at y = -6 would answer every ray that starts below it)."""
    d = it.d
    for _ in range(200):
        o = target + rng.uniform(8.0, 25.0) * rand_unit(rng, d)
        if it.br > 0 and np.linalg.norm(o - it.bc) <= 1.05 * it.br:
            continue
        if not below_ok and o[1] < -5.0:
            continue
        return o
    return o


def sparse_direction(rng, d, zeros):
    v = rng.standard_normal(d)
    v[rng.choice(d, zeros, replace=False)] = 0.0
    return unit(v)


def hcube_faces(fs, idx, rng):
    """A seeded sample of the hcube's faces: its children stand in the order of their dimension m = 2 .. N-1 and, inside one m,
    of their position; every m gets its share, spread evenly over that m's run (the face tree and the face groups of the
    device are built over runs of this order), plus seeded picks."""
    o = fs.objects[idx]
    kids = [fs._obj_refs[o["obj_off"] + k] for k in range(o["n_obj"])]
    if len(kids) <= HCUBE_FACES:
        return kids
    by_m = {}
    for k in kids:
        by_m.setdefault(fs._flags[fs.objects[k]["flag_off"]], []).append(k)
    share = HCUBE_FACES // len(by_m)
    picked = []
    for m in sorted(by_m):
        run = by_m[m]
        if len(run) <= share:
            picked += run
            continue
        even = [run[(2 * j + 1) * len(run) // (2 * (share // 2))] for j in range(share // 2)]
        rest = [k for k in run if k not in set(even)]
        picked += even + [rest[j] for j in sorted(rng.choice(len(rest), share - len(even), replace=False))]
    return picked


def ray(o, v, lim, item, cls, sub):
    return dict(o=np.asarray(o, dtype=np.float64), v=np.asarray(v, dtype=np.float64), lim=float(lim), item=item, cls=cls, sub=sub,
                after=[])


def towards(o, target):
    return unit(target - o)


def first_pass(fs, rng):
    """Classes A, B, D, E (but for the origins on a surface) and F, item by item."""
    d = fs.dims
    cam = fs.vec(fs.cam["pos"])
    rays = []
    for idx in range(fs.n_items):
        top = Item(fs, idx)
        more = 2 if top.type == T["hcylinder"] else 1       # (a tube that ends along d - 2 axes: half its rays leave by an end)
        if top.type == T["hcube"]:
            faces = hcube_faces(fs, idx, rng)
            per_face = max(1, HCUBE_FACES // (2 * len(faces)))
            parts = [(Item(fs, k, owner=idx), per_face, per_face) for k in faces]
        else:
            parts = [(top, 16 * more, 20 * more)]
        for part_no, (it, n_cam, n_out) in enumerate(parts):
            starts = []
            for k in range(n_cam + n_out):
                tgt = it.surface(rng)
                from_cam = k < n_cam
                o = cam if from_cam else outside_origin(it, rng, tgt)
                r = ray(o, towards(o, tgt), -1.0, it.item, A, SUB_CAMERA if from_cam else SUB_OUTSIDE)
                r["target"] = tgt
                rays.append(r)
                if not from_cam:
                    starts.append(r)
            # F: the same target from the opposite side (half the outside rays)
            for r in starts[::2]:
                o = 2.0 * r["target"] - r["o"]
                rays.append(ray(o, towards(o, r["target"]), -1.0, it.item, F, SUB_OUTSIDE))
            # D
            for o, v, tgt, sub in (it.grazing(rng) + (it.grazing(rng) if more > 1 else []) if it is top else it.grazing(rng)[part_no % 6::6]):
                if o is None:
                    o = outside_origin(it, rng, tgt) if rng.random() < 0.75 else cam
                if v is None:
                    v = towards(o, tgt)
                rays.append(ray(o, v, -1.0, it.item, D, sub))
            # E: exactly-zero components (one, half of them, all but one), aimed at a point of the object
            for zeros in ((1, d // 2, d - 1, 1, d // 2, d - 1, 2, d - 2, d - 1, d - 1, 1, d // 2, d - 1, 1) * more if it is top else (1, d - 1)):
                tgt = it.surface(rng)
                v = sparse_direction(rng, d, max(1, min(d - 1, zeros)))
                if top.type != T["hplane"] and v[1] > 0:
                    v = -v                                          # (come from above the floor)
                rays.append(ray(tgt - rng.uniform(6.0, 18.0) * v, v, -1.0, it.item, E, SUB_ZEROS))
            nz = it.normal_with_zeros()
            if nz is not None:
                for _ in range(6):
                    v = rng.standard_normal(d)
                    v[nz != 0.0] = 0.0
                    v = unit(v)
                    o = it.surface(rng) + rng.uniform(-0.5, 0.5) * unit(nz) - rng.uniform(2.0, 9.0) * v
                    rays.append(ray(o, v, -1.0, it.item, E, SUB_PERP))
            if it.type == T["cylinder"]:
                ax = it.axes[0]
                for k in range(8):
                    w = complement(rng, d, ax)[0]
                    p = (it.pos[0] + it.span_point(rng) @ it.axes) + it.size[0] * (0.5 if k % 2 == 0 else 1.0 + 1e-9) * w
                    sgn = 1.0 if k % 4 < 2 else -1.0
                    o = p - sgn * ax * (0.0 if k >= 4 else 1.5 * it.lens[0])
                    rays.append(ray(o, sgn * ax, -1.0, it.item, E, SUB_AXIS))
        # B
        if top.inside(rng) is not None:
            for k in range(24 * more):
                o = top.inside(rng)
                if top.type == T["hcube"]:
                    # from inside the hull to what the reference sees of a face (a random direction leaves the skewed
                    # cube unanswered: see Item.__init__)
                    v = towards(o, parts[(5 * k) % len(parts)][0].surface(rng))
                elif top.type == T["hcylinder"] and k % 3:
                    # mostly across the tube: along it a ray leaves by one of the d - 2 ends before it meets the wall
                    v = unit(rng.standard_normal(2) @ complement(rng, d, top.axes) + 0.1 * rand_unit(rng, d))
                else:
                    v = rand_unit(rng, d) if k % 3 else sparse_direction(rng, d, 1)
                rays.append(ray(o, v, -1.0, idx, B, 0))
    return rays


def second_pass(fs, rng, rays, out):
    """Classes C and E (origins on a surface), from the reference's answers to class A; they are stored right behind their
    class-A ray."""
    d = fs.dims
    made = []
    seen, done_c, done_s = {}, {}, {}
    for r, ans in zip(rays, out):
        if r["cls"] != A or ans[0] == 0.0:
            continue
        hit, nrm = ans[2:2 + d], ans[2 + d:2 + 2 * d]
        key = r["item"]
        t = ref_dist(r["o"], hit)
        per = C_PER_ITEM if fs.objects[key]["type"] != T["hcube"] else 4 * C_PER_ITEM
        turn = seen.get(key, 0)
        seen[key] = turn + 1
        # the answered class-A rays of an item in turn: the limits, an origin on the surface, the limits, ...
        if done_c.get(key, 0) < per and (turn % 2 == 0 or done_s.get(key, 0) >= SURF_PER_ITEM):
            done_c[key] = done_c.get(key, 0) + 1
            for lim, sub in [(0.0, SUB_LIM0)] + around(t, (SUB_LIM_BELOW, SUB_LIM_ABOVE, SUB_LIM_PREV, SUB_LIM_NEXT, SUB_LIM_EXACT)):
                c = ray(r["o"], r["v"], lim, key, C, sub)
                c["parent_obj"] = ans[1]
                r["after"].append(c)
                made.append(c)
        elif done_s.get(key, 0) < SURF_PER_ITEM and nrm @ nrm > 0:
            done_s[key] = done_s.get(key, 0) + 1
            # reflected (what every secondary ray is), and straight on through the surface (a refracted or a shadow ray)
            for v in (unit(r["v"] - 2.0 * (r["v"] @ nrm) / (nrm @ nrm) * nrm), r["v"]):
                s = ray(hit, v, -1.0, key, E, SUB_SURFACE)
                r["after"].append(s)
                made.append(s)
    return made


def third_pass(fs, second, out):
    """Class C, continued.  A limit around the NEAREST answer cannot change an answer (the scan may stop early, but nothing
    nearer is left).  It can where the scan meets a farther object first: with limit 0 the reference stops there.  Where its
    limit-0 answer is not the ray's nearest one, the same ray again with limits around the distance of THAT object -- below it
    the scan goes on to the nearer object, above it it stops (object.c:692-747: `dist < dist_limit`, strictly)."""
    d = fs.dims
    made = []
    for c, ans in zip(second, out):
        if c["cls"] == C and c["sub"] == SUB_LIM0 and ans[0] != 0.0 and ans[1] != c["parent_obj"]:
            tx = ref_dist(c["o"], ans[2:2 + d])
            for lim, sub in around(tx, (SUB_FIRST_BELOW, SUB_FIRST_ABOVE, SUB_FIRST_PREV, SUB_FIRST_NEXT, SUB_FIRST_EXACT)):
                x = ray(c["o"], c["v"], lim, c["item"], C, sub)
                c["after"].append(x)
                made.append(x)
    return made


def pack(rays, d):
    arr = np.zeros((len(rays), 2 * d + 1))
    for i, r in enumerate(rays):
        arr[i, :d], arr[i, d:2 * d], arr[i, 2 * d] = r["o"], r["v"], r["lim"]
    return arr


def build(fs, answers, seed):
    """The rays of one fixture and the answers `answers(kat_in) -> kat_out` gives: (kat_in, kat_out, aim_item, aim_class, aim_sub)."""
    rng = np.random.default_rng(seed)
    d = fs.dims
    first = first_pass(fs, rng)
    out1 = answers(pack(first, d))
    second = second_pass(fs, rng, first, out1)
    out2 = answers(pack(second, d)) if second else np.zeros((0, 2 + 2 * d))
    third = third_pass(fs, second, out2)
    out3 = answers(pack(third, d)) if third else np.zeros((0, 2 + 2 * d))
    where = {id(r): out2[i] for i, r in enumerate(second)}
    where.update({id(r): out3[i] for i, r in enumerate(third)})
    order, outs = [], []

    def put(r, ans):
        order.append(r)
        outs.append(ans)
        for c in r["after"]:
            put(c, where[id(c)])
    for r, ans in zip(first, out1):
        put(r, ans)
    return (pack(order, d), np.array(outs), np.array([r["item"] for r in order], dtype=np.int32),
            np.array([r["cls"] for r in order], dtype=np.int8), np.array([r["sub"] for r in order], dtype=np.int8))


def reference_answers(case):
    base = ["--scene", os.path.join(REF, "scenes", "parity_zoo.so"), "--dims", str(case["dims"]), "--frame", str(case.get("frame", 0)),
            "--res", "8x8", "--no-render"]
    if case.get("config"):
        base += ["--config", case["config"]]
    d = case["dims"]

    def answers(kat_in):
        with tempfile.TemporaryDirectory() as tmp:
            kat_in.tofile(os.path.join(tmp, "rays.bin"))
            subprocess.run([SHIM, "--objects", os.path.join(REF, "objects")] + base + [
                "--tmp", tmp, "--rays-in", os.path.join(tmp, "rays.bin"), "--rays-out", os.path.join(tmp, "kat.bin")],
                check=True, capture_output=True, text=True)
            return np.fromfile(os.path.join(tmp, "kat.bin")).reshape(-1, 2 + 2 * d)
    return answers


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def generate(name, case):
    print("==", name, flush=True)
    with open(os.path.join(HERE, case["share"] + ".json")) as f:
        shared = json.load(f)
    fs = load_scene(os.path.join(HERE, shared["scene_file"]))
    assert fs.dims == case["dims"]
    kat_in, kat_out, item, cls, sub = build(fs, reference_answers(case), seed=4321 + case["dims"])
    save_npz(os.path.join(HERE, name + ".npz"), dict(kat_in=kat_in, kat_out=kat_out, aim_item=item, aim_class=cls, aim_sub=sub))
    meta = dict(name=name, scene="parity_zoo", dims=case["dims"], frame=case.get("frame", 0), config=case.get("config"),
                scene_file=shared["scene_file"], shares_scene_of=case["share"], width=shared["width"], height=shared["height"],
                depth=shared["depth"], rays=int(len(kat_in)), generator="tests/golden/make_golden_aimed.py via oracle/ref_shim.c")
    with open(os.path.join(HERE, name + ".json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("    %d rays, %d answered, %d bytes" % (len(kat_in), int((kat_out[:, 0] != 0).sum()),
                                                    os.path.getsize(os.path.join(HERE, name + ".npz"))), flush=True)


def main():
    if not os.path.exists(SHIM):
        raise SystemExit("build the reference first: make -C oracle ref")
    for name in sys.argv[1:] or list(AIMED):
        generate(name, AIMED[name])


if __name__ == "__main__":
    main()
