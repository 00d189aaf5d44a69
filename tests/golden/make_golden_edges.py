#!/usr/bin/env python3
"""Generate the EDGE fixtures edge{N}d_{K} from the COMPILED REFERENCE: crowds (tests/scenes/parity_crowd.c) whose item
count K stands on either side of a value at which the trace code switches kernels.

    make -C oracle ref oracle
    python tests/golden/make_golden_edges.py [edge3d_64 ...]

The rules that pick a kernel compare the item count with 64 and 256 and the trace section with 64 KB
(ndt_blob.hip:build_blob); a visit mask has one bit per item, 64 to a word.  make_golden_crowd.py's cases stand in the
interior of every family; these stand where the families meet (tests/test_trace_edges.py holds the table and the tests):

    case                           N         K         config              why this K
    edge{3,7,12}d_64               3, 7, 12  64        nohcube             the most the item sets hold: bit 63 of a set and of a
                                                                           node's `below` set, pushed as two ints
    edge{3,7,12}d_65               3, 7, 12  65        nohcube             the fewest of the register kernel: item 64 is bit 0 of
                                                                           word 1, alone in it
    edge{3,7}d_128, edge{3,7}d_129 3, 7      128, 129  nohcube             two full words; item 128 alone in word 2 (129 items of all
                                                                           eight types are within 64 KB up to 7-D: 64 376 B there)
    edge3d_l192, edge3d_l193       3         192, 193  nohcube,mix=light   three full words; item 192 alone in word 3, the word that
                                                                           no other fixture populates
    edge3d_l256                    3         256       nohcube,mix=spheres the most of the register kernel, all four words full
    edge3d_l257                    3         257       nohcube,mix=spheres tier 1 by the count alone: item 256 is bit 0 of a fifth
                                                                           word, the section is still under 64 KB
    edge12d_257                    12        257       nohcube             tier 1, five words, a record over the leaf-scan limit

With all eight small types no 256 items stay within 64 KB in any dimension (176 is the most, in 3-D).  Sizes found on the
CPU from the blob builder before anything was generated: with mix=light (sphere, hdisk, cylinder) 192 items take 48 528 B
and 240 items 65 040 B, but 256 take 69 224 B -- their boxes reach into the neighbouring cells, and the leaf lists, not
the records, are what grows; 256 spheres take 52 592 B and 257 take 52 720 B.  So the two cases at 256 are spheres only.

Every case stores what a _g case of make_golden_crowd.py stores -- the scene, aimed rays of the classes A .. F with the
reference's answers, the reference's own 40x24 frame at depth 4 -- made by that module's ray makers.  FULL items (all six
classes) are 8 of a type and the EDGE items: item 0, the items on either side of every mask-word boundary the scene has
(62 63 | 64 65, 126 127 | 128 129, 190 191 | 192 193, 254 255 | 256), and the last two.  Every edge item but the floor
(an infinite object: in no leaf) also gets rays from origins close by.  Of 240 candidates an item, those are kept whose
line touches two kd leaves that both list the item -- the case in which a scan finds the item's mask bit set; decided on
the scene's geometry, with tests/test_crowd_tiers.py:leaves_on_segment -- first the ones the reference answers with that
item, and then some of the others it answers with that item.  Where the kd builder puts an edge item into one leaf only
no such ray exists: the scene program's seed is then counted up (seed=S in the stored config) to the first scene whose
every edge item has them.  In 3-D the default seed serves; 7-D and 12-D take seeds 2 to 197.
Only data is written, with fixed time stamps: a second run reproduces every file byte for byte.
"""
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import make_golden_aimed as aimed  # noqa: E402
import make_golden_crowd as crowd  # noqa: E402
from make_golden_aimed import A, Item, towards  # noqa: E402
from ndt_amd import load_scene  # noqa: E402
from test_crowd_tiers import leaf_items, leaves_on_segment  # noqa: E402

REF, SHIM = aimed.REF, aimed.SHIM
WIDTH, HEIGHT, DEPTH = crowd.WIDTH, crowd.HEIGHT, crowd.DEPTH
FULL_PER_TYPE = 8
EDGE_TRIES = 240          # candidate rays per edge item ...
EDGE_SHARED = 20          # ... of which this many whose line touches two leaves that list the item are kept,
EDGE_OTHER = 12           # and this many of the others that the reference answers with the item
MAX_SEED = 400            # seeds of the scene program that are tried


def edge(dims, items, config, per_type=FULL_PER_TYPE, shared=EDGE_SHARED, other=EDGE_OTHER, lean=False):
    return dict(dims=dims, items=items, config="items=%d,%s" % (items, config), per_type=per_type, shared=shared, other=other, lean=lean)


EDGES = {}
for _n in (3, 7, 12):
    EDGES["edge%dd_64" % _n] = edge(_n, 64, "nohcube")
    EDGES["edge%dd_65" % _n] = edge(_n, 65, "nohcube")
for _n in (3, 7):
    EDGES["edge%dd_128" % _n] = edge(_n, 128, "nohcube")
    EDGES["edge%dd_129" % _n] = edge(_n, 129, "nohcube")
EDGES["edge3d_l192"] = edge(3, 192, "nohcube,mix=light")
EDGES["edge3d_l193"] = edge(3, 193, "nohcube,mix=light")
EDGES["edge3d_l256"] = edge(3, 256, "nohcube,mix=spheres")
EDGES["edge3d_l257"] = edge(3, 257, "nohcube,mix=spheres")
# (a 12-D ray and its answer are 51 doubles, about 220 bytes of the file, and no file is to pass 400 KB: 257 items leave room
# for 4 full items a type, and the items that are not full do without their ray from the camera)
EDGES["edge12d_257"] = edge(12, 257, "nohcube", per_type=4, shared=10, other=0, lean=True)


def edge_items(items):
    """Item 0, the items on either side of every mask-word boundary that exists, the last two."""
    out = {0, items - 2, items - 1}
    for b in range(64, items, 64):
        out |= {i for i in (b - 2, b - 1, b, b + 1) if i < items}
    return sorted(out)


def full_items(fs, per_type):
    by_type = {}
    for i in range(fs.n_items):
        by_type.setdefault(fs.objects[i]["type"], []).append(i)
    full = []
    for ty, ids in sorted(by_type.items()):
        if len(ids) <= per_type:
            full += ids
        else:
            full += [ids[int(round(k * (len(ids) - 1) / (per_type - 1)))] for k in range(per_type)]
    return sorted(set(full))


def edge_candidates(fs, rng, edges):
    """Per finite edge item, EDGE_TRIES class-A rays at it from origins close by -- a tenth of a unit to four away, so that little
    or nothing stands between -- and whether each ray's line touches two leaves that both list the item."""
    rays, twice = [], []
    for idx in edges:
        if idx in fs.inf_refs:
            continue
        it = Item(fs, idx)
        for k in range(EDGE_TRIES):
            tgt = it.surface(rng)
            o = tgt + (rng.uniform(0.1, 1.0) if k % 2 else rng.uniform(1.0, 4.0)) * aimed.rand_unit(rng, fs.dims)
            o[1] = max(o[1], -5.0)                      # (above the floor)
            v = towards(o, tgt)
            lists = [leaf_items(fs, k) for k in leaves_on_segment(fs, o, v, -1.0)]
            rays.append(aimed.ray(o, v, -1.0, idx, A, aimed.SUB_OUTSIDE))
            twice.append(sum(idx in l for l in lists) >= 2)
    return rays, np.array(twice, dtype=bool)


def edge_rays(fs, rng, edges, answers, n_shared, n_other):
    """The candidates that are kept, per finite edge item: n_shared whose line touches two leaves that list the item -- first those
    that the REFERENCE answers with the item -- and n_other of the rest that it answers with the item.  None when an item has
    fewer than n_shared candidates of the first kind: this scene's tree does not put that item into two leaves a ray can meet."""
    rays, twice = edge_candidates(fs, rng, edges)
    own = answers(aimed.pack(rays, fs.dims))[:, 1] == np.array([r["item"] for r in rays])
    kept = []
    for idx in edges:
        mine = [k for k, r in enumerate(rays) if r["item"] == idx]
        if not mine:
            continue
        shared = ([k for k in mine if twice[k] and own[k]] + [k for k in mine if twice[k] and not own[k]])[:n_shared]
        if len(shared) < n_shared:
            return None
        kept += sorted(shared + [k for k in mine if own[k] and k not in shared][:n_other])
    return [rays[k] for k in kept]


def scene_for(case, tmp):
    """The first seed (1: the scene program's default, not written into the config) whose scene puts every finite edge item into
    two leaves that one ray can meet: (config, shim arguments, scene, the edge items' rays)."""
    d = case["dims"]
    for scene_seed in range(1, MAX_SEED + 1):
        config = case["config"] + (",seed=%d" % scene_seed if scene_seed > 1 else "")
        base = ["--scene", os.path.join(REF, "scenes", "parity_crowd.so"), "--dims", str(d), "--config", config]
        scene_txt = os.path.join(tmp, "scene.txt")
        make_golden.run_shim(base + ["--res", "8x8", "--no-render", "--tmp", tmp, "--scene-out", scene_txt])
        fs = load_scene(scene_txt)
        assert fs.n_items == case["items"] and fs.dims == d
        edges = edge_items(fs.n_items)
        listed = np.bincount(fs.leaf_refs, minlength=fs.n_items)
        if any(listed[i] < 2 for i in edges if i not in fs.inf_refs):
            continue
        more = edge_rays(fs, np.random.default_rng(4321 + 16 * d + fs.n_items + 1000 * scene_seed), edges, crowd.reference_answers(base, d),
                         case["shared"], case["other"])
        if more is not None:
            return config, base, fs, more
    raise SystemExit("no seed up to %d puts every edge item into two leaves" % MAX_SEED)


def generate(name, case):
    print("==", name, flush=True)
    d = case["dims"]
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        config, base, fs, more = scene_for(case, tmp)
        meta = dict(name=name, scene="parity_crowd", dims=d, items=case["items"], config=config, frame=0, width=WIDTH, height=HEIGHT,
                    depth=DEPTH, scene_file=name + ".ndtscene.gz", generator="tests/golden/make_golden_edges.py via oracle/ref_shim.c")
        with open(os.path.join(tmp, "scene.txt"), "rb") as src, open(os.path.join(HERE, meta["scene_file"]), "wb") as raw:
            with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as dst:
                dst.write(src.read())
        meta["objects"] = fs.type_histogram()
        meta["kd_nodes"] = len(fs.kd_nodes)
        info = make_golden.run_shim(base + ["--res", "%dx%d" % (WIDTH, HEIGHT), "--depth", str(DEPTH), "--threads", str(min(16, os.cpu_count() or 1)),
                                            "--tmp", tmp, "--fb-out", os.path.join(tmp, "fb.bin")])
        meta.update({k: v for k, v in info.items() if k.startswith("rays_")})
        arrays["fb"] = np.fromfile(os.path.join(tmp, "fb.bin")).reshape(HEIGHT, WIDTH, 4)
    edges = edge_items(fs.n_items)
    full = sorted(set(full_items(fs, case["per_type"])) | set(edges))
    answers = crowd.reference_answers(base, d)
    kat_in, kat_out, item, cls, sub = crowd.build(fs, answers, seed=4321 + 16 * d + fs.n_items, full=set(full))
    if case["lean"]:
        keep = ~((cls == A) & (sub == aimed.SUB_CAMERA) & ~np.isin(item, full))
        assert not (cls[np.flatnonzero(~keep) + 1] == aimed.C).any()           # (no limits stand behind a ray that leaves)
        kat_in, kat_out, item, cls, sub = kat_in[keep], kat_out[keep], item[keep], cls[keep], sub[keep]
    more_in = aimed.pack(more, d)
    kat_in = np.concatenate([kat_in, more_in])
    kat_out = np.concatenate([kat_out, answers(more_in)])
    item = np.concatenate([item, np.array([r["item"] for r in more], dtype=np.int32)])
    cls = np.concatenate([cls, np.array([r["cls"] for r in more], dtype=np.int8)])
    sub = np.concatenate([sub, np.array([r["sub"] for r in more], dtype=np.int8)])
    arrays.update(kat_in=kat_in, kat_out=kat_out, aim_item=item, aim_class=cls, aim_sub=sub)
    aimed.save_npz(os.path.join(HERE, name + ".npz"), arrays)
    meta.update(rays=int(len(kat_in)), full_items=full, edge_items=edges, edge_rays=len(more))
    with open(os.path.join(HERE, name + ".json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("    %s: %d rays, %d answered, %d + %d bytes" % (config, len(kat_in), int((kat_out[:, 0] != 0).sum()), os.path.getsize(os.path.join(HERE, name + ".npz")),
                                                           os.path.getsize(os.path.join(HERE, meta["scene_file"]))), flush=True)


def main():
    if not os.path.exists(SHIM):
        raise SystemExit("build the reference first: make -C oracle ref")
    for name in sys.argv[1:] or list(EDGES):
        generate(name, EDGES[name])


if __name__ == "__main__":
    main()
