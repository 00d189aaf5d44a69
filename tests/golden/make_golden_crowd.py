#!/usr/bin/env python3
"""Generate the CROWD fixtures crowd{3..12}d_{r,g,gn,l} from the COMPILED REFERENCE.

    make -C oracle ref oracle
    python tests/golden/make_golden_crowd.py [crowd7d_g ...]

A crowd (tests/scenes/parity_crowd.c) is one floor and K - 1 small objects of the other eight types, interleaved in item
order.  Its K decides which family of trace kernels a scene runs on the device (tests/test_crowd_tiers.py holds the table
and says why each K is what it is); the zoo's 13 to 15 items only ever reach one of them.  Every case stores

    <case>.ndtscene.gz   the scene the reference built (the shim's --scene-out)
    <case>.npz           kat_in, kat_out, aim_item, aim_class, aim_sub: aimed rays in the layout and with the classes A .. F
                         of make_golden_aimed.py, whose ray makers are used here; answered by the shim's --rays-in / --rays-out
                         fb (24, 40, 4): for the _g, _gn and _l cases the reference's own render at depth 4 (make_golden.py's path)
    <case>.json          the case, its ray count, rays_total of the render, and full_items (below)

320 items times the zoo's 200-odd rays an item is too much to keep.  Per type, 24 items spread evenly over the item
numbers (all of them where the type has fewer: the floor, the hcubes) are FULL items and get all six classes, a few rays
each; every other item gets classes A and F.  Only data is written, with fixed time stamps: a second run reproduces every
file byte for byte.
"""
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402
import make_golden_aimed as aimed  # noqa: E402
from make_golden_aimed import A, B, C, D, E, F, T, Item, ray, towards, outside_origin, sparse_direction, complement  # noqa: E402
from ndt_amd import load_scene  # noqa: E402

REF, SHIM = aimed.REF, aimed.SHIM
WIDTH, HEIGHT, DEPTH = 40, 24, 4
FULL_PER_TYPE = 24
HCUBE_FACES = 32          # faces of an hcube that get rays of their own


def crowd(dims, items, hcube, frame=False):
    return dict(dims=dims, items=items, config="items=%d%s" % (items, "" if hcube else ",nohcube"), frame=frame)


# The K of every _r case is the largest (up to 256) whose trace section stays within 64 KB, found on the CPU from the blob
# builder's own sizes; tests/test_crowd_tiers.py:CASES repeats them beside the tier each one is for.
CROWDS = {}
for _n, (_k, _hc) in {3: (176, True), 4: (158, False), 5: (155, False), 6: (142, False), 7: (131, False), 8: (126, False),
                      9: (118, False), 10: (107, False), 11: (101, False), 12: (94, False)}.items():
    CROWDS["crowd%dd_r" % _n] = crowd(_n, _k, _hc)
for _n in range(3, 13):
    CROWDS["crowd%dd_g" % _n] = crowd(_n, 320, _n <= 8, frame=True)
    if _n <= 8:
        CROWDS["crowd%dd_gn" % _n] = crowd(_n, 320, False, frame=True)
for _n in (10, 12):
    CROWDS["crowd%dd_l" % _n] = crowd(_n, 200, False, frame=True)


def full_items(fs):
    """Per type, FULL_PER_TYPE items at even steps through that type's items (in item order: every mask word has some)."""
    by_type = {}
    for i in range(fs.n_items):
        by_type.setdefault(fs.objects[i]["type"], []).append(i)
    full = []
    for ty, ids in sorted(by_type.items()):
        if len(ids) <= FULL_PER_TYPE:
            full += ids
        else:
            full += [ids[int(round(k * (len(ids) - 1) / (FULL_PER_TYPE - 1)))] for k in range(FULL_PER_TYPE)]
    return sorted(set(full))


def first_pass(fs, rng, full):
    """Classes A and F for every item; B, D and E (but for the origins on a surface) for the full ones."""
    d = fs.dims
    cam = fs.vec(fs.cam["pos"])
    rays = []
    of_type = {}
    for idx in range(fs.n_items):
        of_type[fs.objects[idx]["type"]] = of_type.get(fs.objects[idx]["type"], 0) + 1
    for idx in range(fs.n_items):
        top = Item(fs, idx)
        is_full = idx in full
        more = 6 if of_type[top.type] <= 2 else 1         # (the floor, the hcubes: one or two items have to reach the type's floor)
        if top.type == T["hcube"]:
            faces = aimed.hcube_faces(fs, idx, rng)
            faces = [faces[(2 * k + 1) * len(faces) // (2 * HCUBE_FACES)] for k in range(HCUBE_FACES)] if len(faces) > HCUBE_FACES else faces
            more = max(1, HCUBE_FACES // len(faces))
            parts = [(Item(fs, k, owner=idx), more, 2 * more) for k in faces]
        else:
            parts = [(top, more, 2 * more if is_full else 1)]
        for part_no, (it, n_cam, n_out) in enumerate(parts):
            starts = []
            for k in range(n_cam + n_out):
                tgt = it.surface(rng)
                from_cam = k < n_cam
                o = cam if from_cam else outside_origin(it, rng, tgt)
                r = ray(o, towards(o, tgt), -1.0, it.item, A, aimed.SUB_CAMERA if from_cam else aimed.SUB_OUTSIDE)
                r["target"] = tgt
                rays.append(r)
                if not from_cam:
                    starts.append(r)
            if is_full and it is top and idx > 0:
                # through a point of a neighbour in item order (they stand in neighbouring cells and share leaves) to a point of
                # this item: the neighbour is the nearer one, and of the two the leaf's scan meets the lower number first --
                # the rays whose limit-0 answer is not their nearest
                for nb in (idx + 1, idx - 1):
                    if 1 <= nb < fs.n_items and fs.objects[nb]["type"] != T["hcube"]:
                        tgt, front = it.surface(rng), Item(fs, nb).surface(rng)
                        o = front - rng.uniform(6.0, 16.0) * towards(front, tgt)
                        if o[1] > -5.0:
                            rays.append(ray(o, towards(o, tgt), -1.0, it.item, A, aimed.SUB_OUTSIDE))
            for r in starts[::2]:
                o = 2.0 * r["target"] - r["o"]
                rays.append(ray(o, towards(o, r["target"]), -1.0, it.item, F, aimed.SUB_OUTSIDE))
            if not is_full:
                continue
            graze = it.grazing(rng)
            if it.type == T["facet"]:
                # Not the facet's vertices.  The facet decides inside / outside by comparing angles (facet.c:166-269), and for a
                # point that IS vertex i the angle at vertex j is, but for rounding, the triangle's own angle there: the
                # comparison is decided by the last bit of acos, which the device's math library and glibc round differently
                # (DESIGN.md).  Measured on the reference's own hit points: 0 or 1 ulp between the two angles.  The points
                # 1e-9 and 1e-3 inside and outside every edge stay.
                graze = [x for x in graze if x[3] != aimed.SUB_VERTEX]
            for k in (sorted(rng.choice(len(graze), min(3 * more, len(graze)), replace=False)) if it is top else range(part_no % 4, len(graze), 4)):
                o, v, tgt, sub = graze[k]
                if o is None:
                    o = outside_origin(it, rng, tgt) if rng.random() < 0.75 else cam
                if v is None:
                    v = towards(o, tgt)
                rays.append(ray(o, v, -1.0, it.item, D, sub))
            # (an hcylinder is a tube in two of the d coordinates: few sparse directions meet it)
            for zeros in ((1, d - 1) * more * (4 if it.type == T["hcylinder"] else 1) if it is top else (1 + part_no % (d - 1), d - 1) * more):
                tgt = it.surface(rng)
                v = sparse_direction(rng, d, max(1, min(d - 1, zeros)))
                if top.type != T["hplane"] and v[1] > 0:
                    v = -v
                rays.append(ray(tgt - rng.uniform(6.0, 18.0) * v, v, -1.0, it.item, E, aimed.SUB_ZEROS))
            if it.type == T["cylinder"]:
                ax = it.axes[0]
                w = complement(rng, d, ax)[0]
                p = (it.pos[0] + it.span_point(rng) @ it.axes) + it.size[0] * 0.5 * w
                rays.append(ray(p - ax * 1.5 * it.lens[0], ax, -1.0, it.item, E, aimed.SUB_AXIS))
        if is_full and top.inside(rng) is not None:
            for k in range(16 if top.type == T["hcube"] else 2 * more):
                o = top.inside(rng)
                if top.type == T["hcube"]:
                    v = towards(o, parts[(5 * k) % len(parts)][0].surface(rng))
                elif top.type == T["hcylinder"]:
                    v = aimed.unit(rng.standard_normal(2) @ complement(rng, d, top.axes) + 0.1 * aimed.rand_unit(rng, d))
                else:
                    v = aimed.rand_unit(rng, d) if k % 2 else sparse_direction(rng, d, 1)
                rays.append(ray(o, v, -1.0, idx, B, 0))
    return rays


def second_pass(fs, full, rays, out, any_hit):
    """Classes C and E (origins on a surface) from the reference's answers to the class-A rays of the full items: per item two
    answered rays get the limits and another one lends its hit point (the floor, an hcube: twelve and four).  `any_hit` holds the
    reference's answers to the same rays with limit 0: where that is another object than the nearest -- the scan met a farther
    one first, the only case in which a limit can change an answer -- the ray is taken for the limits before the others (for
    half of an item's limit rays), then the rays that the item itself answers."""
    d = fs.dims
    limits = (aimed.SUB_LIM_BELOW, aimed.SUB_LIM_ABOVE, aimed.SUB_LIM_PREV, aimed.SUB_LIM_NEXT, aimed.SUB_LIM_EXACT)
    of_type = {}
    for idx in range(fs.n_items):
        of_type[fs.objects[idx]["type"]] = of_type.get(fs.objects[idx]["type"], 0) + 1
    answered = {}
    for k, (r, ans) in enumerate(zip(rays, out)):
        if r["cls"] == A and ans[0] != 0.0 and r["item"] in full:
            answered.setdefault(r["item"], []).append(k)
    made = []
    for key in sorted(answered):
        few = of_type[fs.objects[key]["type"]] <= 2
        quota_c, quota_s = (12, 4) if few else (2, 1)
        cand = answered[key]
        observable = [k for k in cand if any_hit[k][0] != 0.0 and any_hit[k][1] != out[k][1]]
        own = [k for k in cand if out[k][1] == key]
        for_c = observable[:quota_c // 2]
        for_c += [k for k in own if k not in for_c][:quota_c - len(for_c)]
        for_c += [k for k in observable + cand if k not in for_c][:max(0, min(quota_c, len(cand) - 1) - len(for_c))]
        for_s = [k for k in own + cand if k not in for_c and out[k][2 + d:2 + 2 * d] @ out[k][2 + d:2 + 2 * d] > 0]
        for_s = sorted(set(for_s), key=for_s.index)[:quota_s]
        for k in sorted(for_c + for_s):
            r, ans = rays[k], out[k]
            hit, nrm = ans[2:2 + d], ans[2 + d:2 + 2 * d]
            if k in for_c:
                for lim, sub in [(0.0, aimed.SUB_LIM0)] + aimed.around(aimed.ref_dist(r["o"], hit), limits):
                    c = ray(r["o"], r["v"], lim, key, C, sub)
                    c["parent_obj"] = ans[1]
                    r["after"].append(c)
                    made.append(c)
            else:
                for v in (aimed.unit(r["v"] - 2.0 * (r["v"] @ nrm) / (nrm @ nrm) * nrm), r["v"]):
                    x = ray(hit, v, -1.0, key, E, aimed.SUB_SURFACE)
                    r["after"].append(x)
                    made.append(x)
    return made


def build(fs, answers, seed, full):
    rng = np.random.default_rng(seed)
    d = fs.dims
    first = first_pass(fs, rng, full)
    out1 = answers(aimed.pack(first, d))
    lim0 = aimed.pack(first, d)
    lim0[:, 2 * d] = 0.0
    second = second_pass(fs, full, first, out1, answers(lim0))
    out2 = answers(aimed.pack(second, d))
    third = aimed.third_pass(fs, second, out2)
    out3 = answers(aimed.pack(third, d)) if third else np.zeros((0, 2 + 2 * d))
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
    return (aimed.pack(order, d), np.array(outs), np.array([r["item"] for r in order], dtype=np.int32),
            np.array([r["cls"] for r in order], dtype=np.int8), np.array([r["sub"] for r in order], dtype=np.int8))


def reference_answers(base, d):
    def answers(kat_in):
        with tempfile.TemporaryDirectory() as tmp:
            kat_in.tofile(os.path.join(tmp, "rays.bin"))
            make_golden.run_shim(base + ["--res", "8x8", "--no-render", "--tmp", tmp, "--rays-in", os.path.join(tmp, "rays.bin"),
                                         "--rays-out", os.path.join(tmp, "kat.bin")])
            return np.fromfile(os.path.join(tmp, "kat.bin")).reshape(-1, 2 + 2 * d)
    return answers


def generate(name, case):
    print("==", name, flush=True)
    d = case["dims"]
    base = ["--scene", os.path.join(REF, "scenes", "parity_crowd.so"), "--dims", str(d), "--config", case["config"]]
    meta = dict(name=name, scene="parity_crowd", dims=d, items=case["items"], config=case["config"], frame=0, width=WIDTH, height=HEIGHT,
                depth=DEPTH, scene_file=name + ".ndtscene.gz", generator="tests/golden/make_golden_crowd.py via oracle/ref_shim.c")
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        scene_txt = os.path.join(tmp, "scene.txt")
        make_golden.run_shim(base + ["--res", "8x8", "--no-render", "--tmp", tmp, "--scene-out", scene_txt])
        with open(scene_txt, "rb") as src, open(os.path.join(HERE, meta["scene_file"]), "wb") as raw:
            with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as dst:
                dst.write(src.read())
        fs = load_scene(scene_txt)
        assert fs.n_items == case["items"] and fs.dims == d
        meta["objects"] = fs.type_histogram()
        meta["kd_nodes"] = len(fs.kd_nodes)
        if case["frame"]:
            info = make_golden.run_shim(base + ["--res", "%dx%d" % (WIDTH, HEIGHT), "--depth", str(DEPTH), "--threads", str(min(16, os.cpu_count() or 1)),
                                                "--tmp", tmp, "--fb-out", os.path.join(tmp, "fb.bin")])
            meta.update({k: v for k, v in info.items() if k.startswith("rays_")})
            arrays["fb"] = np.fromfile(os.path.join(tmp, "fb.bin")).reshape(HEIGHT, WIDTH, 4)
    full = full_items(fs)
    kat_in, kat_out, item, cls, sub = build(fs, reference_answers(base, d), seed=8765 + 16 * d + len(name), full=set(full))
    arrays.update(kat_in=kat_in, kat_out=kat_out, aim_item=item, aim_class=cls, aim_sub=sub)
    aimed.save_npz(os.path.join(HERE, name + ".npz"), arrays)
    meta.update(rays=int(len(kat_in)), full_items=full)
    with open(os.path.join(HERE, name + ".json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("    %d rays, %d answered, %d + %d bytes" % (len(kat_in), int((kat_out[:, 0] != 0).sum()), os.path.getsize(os.path.join(HERE, name + ".npz")),
                                                       os.path.getsize(os.path.join(HERE, meta["scene_file"]))), flush=True)


def main():
    if not os.path.exists(SHIM):
        raise SystemExit("build the reference first: make -C oracle ref")
    for name in sys.argv[1:] or list(CROWDS):
        generate(name, CROWDS[name])


if __name__ == "__main__":
    main()
