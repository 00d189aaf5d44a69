"""What upload accepts (include/ndt_hip.h): degenerate scenes rendered right, malformed ones refused.

ndt_hip_upload_scene stands between a caller's ndt_flat_scene and kernels that follow its indices into device memory.  The other
modules stand at the large end of that contract (256 / 257 items, kd depth 40 / 41, leaves of 65 entries, more than 64 lights);
this one stands at the small end and on the refusing side.

  CPU  An independent model of the contract, model_verdict(), written from the header's text over the FlatScene's Python lists,
       judges a table of mutations of four fixtures: every index and count field of the four structs at -1, the first value out
       of range, the last value in range and 2^31 - 1, and the malformations that are not one field's value (a count over a NULL
       array, a kd child that points at its parent or into its sibling's subtree, an hcube that lists an hcube, chains of 41 and of
       200 000 levels, ...).  ndt_hip_check_scene -- which needs no device -- gives the model's verdict on every one of them, with
       the model's code, in a message that names the object, kd node or light the model names.  A field added to a struct fails
       test_every_integer_field_is_judged_or_excused until it is in the table or excused with a reason.
  GPU  One mutation of every kind of refusal is uploaded: the code and message of the check, NDT_E_STATE from the render that
       follows, and after the good scene is uploaded again the bytes rendered before.  Nothing the model refuses is ever rendered.
       Eight degenerate scenes (D1 .. D8: no lights, ambient lights only, no kd node, an empty root leaf, no infinite list, objects
       listed nowhere, no objects, one item in one leaf) in 3-D, 4-D, 7-D and 12-D, and frames of 1 x 1, 1 x 9 and 9 x 1 pixels, under
       every way the library renders a frame: the oracle's frame, map and ray counts, the same bytes from every setting, and
       trace_rays on the frame's own primary rays bit for bit the oracle's.

The scenes are made by surgery on the fixtures' Python lists, the way test_trace_edges.one_leaf and deep do it; the oracle renders
every one of them (pinned to the compiled reference by test_oracle_golden.py on the fixtures themselves)."""
import collections
import contextlib
import ctypes as C
import re

import numpy as np
import pytest

from conftest import golden
from ndt_amd import flat_scene as fsmod
from ndt_amd import hip as nh
from ndt_amd.flat_scene import FlatKdNode, FlatLight, FlatObject, FlatScene, FlatSceneStruct, OBJ_TYPE_ID
from test_sampled_replay import TOL_TIGHT
from test_view_modes import DEFAULTS as VIEW_DEFAULTS, SETTINGS, ray_counts

INVALID, UNSUPPORTED, STATE = fsmod.NDT_E_INVALID, fsmod.NDT_E_UNSUPPORTED, fsmod.NDT_E_STATE
BIG = 2 ** 31 - 1
MAX_LIGHTS = 1024           # include/ndt_hip.h:NDT_MAX_LIGHTS
KD_STACK = 40               # ndt_device.hpp:NDT_KD_STACK (test_trace_edges.py)
HANDFUL = 5                 # "more than a handful of distinct colours": a hand's count; the empty frames D6 and D7 show one
BASES = ["shade3d", "zoo4d", "zoo12d", "c3_random4d"]
W, H, DEPTH = 16, 9, 3


# ------------------------------------------------------------------------------------------------ scenes of one's own

def clone(src):
    """A scene of its own, every list and record copied: golden() shares its scene."""
    fs = FlatScene()
    for key in ("name", "dims", "cam_type", "cam_focal_distance", "cam_aperture_radius", "cam_h_fov", "cam_v_fov", "n_items"):
        setattr(fs, key, getattr(src, key))
    for key in ("ambient", "background", "_vecs", "_sizes", "_flags", "_obj_refs", "leaf_refs", "inf_refs"):
        setattr(fs, key, list(getattr(src, key)))
    for key in ("lights", "objects", "kd_nodes"):
        setattr(fs, key, [dict(r) for r in getattr(src, key)])
    fs.cam, fs.bb = dict(src.cam), dict(src.bb)
    fs.lie = {}
    return fs


def sealed(fs, lie=None):
    """finalize(), then the lies of `lie` told in the C struct alone: a count that is not its list's length, an ABI number, or None
    for an array's pointer.  The model reads the same lies from fs.lie."""
    fs._struct = None
    fs.finalize()
    fs.lie = dict(lie or {})
    for key, value in fs.lie.items():
        setattr(fs._struct, key, type(getattr(fs._struct, key))() if value is None else value)
    return fs


def base(name):
    return golden(name).scene


# ------------------------------------------------------------------------------------------------ the model

Verdict = collections.namedtuple("Verdict", "code kind index field")
# array -> its count, as the struct pairs them
ARRAYS = [("vecs", "n_vecs"), ("sizes", "n_sizes"), ("flags", "n_flags"), ("obj_refs", "n_obj_refs"), ("lights", "n_lights"),
          ("objects", "n_objects"), ("kd_nodes", "n_kd_nodes"), ("leaf_refs", "n_leaf_refs"), ("inf_refs", "n_inf")]
T = OBJ_TYPE_ID


def model_verdict(fs):
    """None, or (code, "scene" | "object" | "node" | "light" | "inf", its number, the field at fault): include/ndt_hip.h "What
    upload accepts", rule by rule in the header's order, over the Python lists a FlatScene is built from.  It follows every index
    the device would follow and nothing else of the library's."""
    lie = getattr(fs, "lie", {})
    real = {"n_vecs": len(fs._vecs), "n_sizes": len(fs._sizes), "n_flags": len(fs._flags), "n_obj_refs": len(fs._obj_refs),
            "n_lights": len(fs.lights), "n_objects": len(fs.objects), "n_items": fs.n_items, "n_kd_nodes": len(fs.kd_nodes),
            "n_leaf_refs": len(fs.leaf_refs), "n_inf": len(fs.inf_refs)}
    n = {k: (v if lie.get(k) is None else lie[k]) for k, v in real.items()}
    d = fs.dims

    def cam(key):
        return fs.cam.get(key, -1)

    def vectors(off, k):
        return off >= 0 and k >= 0 and off + k * d <= n["n_vecs"]

    def pool(off, k, count):
        return k >= 0 and off >= 0 and off + k <= n[count]

    # 1
    if lie.get("abi_version", fsmod.ABI_VERSION) != fsmod.ABI_VERSION:
        return Verdict(INVALID, "scene", None, "abi_version")
    if not fsmod.MIN_DIMS <= d <= fsmod.MAX_DIMS:
        return Verdict(UNSUPPORTED, "scene", None, "dims")
    if not 0 <= fs.cam_type <= 2:
        return Verdict(UNSUPPORTED, "scene", None, "cam_type")
    if fs.cam_type != 0 and min(cam("local_x"), cam("local_y"), cam("local_z")) < 0:
        return Verdict(INVALID, "scene", None, "local axes")
    # 2
    for key in ("n_lights", "n_objects", "n_items", "n_kd_nodes", "n_leaf_refs", "n_inf", "n_vecs", "n_sizes", "n_flags", "n_obj_refs"):
        if n[key] < 0:
            return Verdict(INVALID, "scene", None, key)
    if n["n_lights"] > MAX_LIGHTS:
        return Verdict(UNSUPPORTED, "scene", None, "n_lights")
    if n["n_items"] > n["n_objects"]:
        return Verdict(INVALID, "scene", None, "n_items")
    # 3
    for array, count in ARRAYS:
        if n[count] > 0 and array in lie and lie[array] is None:
            return Verdict(INVALID, "scene", None, array)
    # 4: a node, its left subtree, its right subtree; an entry is (node index, level, the node that holds the index)
    if n["n_kd_nodes"] > 0:
        seen, todo = set(), [(0, 1, None)]
        while todo:
            k, level, holder = todo.pop()
            if not 0 <= k < n["n_kd_nodes"]:
                return Verdict(INVALID, "node", holder, "left/right")
            if level > KD_STACK:
                return Verdict(UNSUPPORTED, "node", k, "depth")
            if k in seen:
                return Verdict(INVALID, "node", k, "reached twice")
            seen.add(k)
            node = fs.kd_nodes[k]
            if node["dim"] >= 0:
                if node["dim"] >= d:
                    return Verdict(INVALID, "node", k, "dim")
                todo += [(node["right"], level + 1, k), (node["left"], level + 1, k)]
            else:
                if not pool(node["first"], node["num"], "n_leaf_refs"):
                    return Verdict(INVALID, "node", k, "first/num")
                for item in fs.leaf_refs[node["first"]:node["first"] + node["num"]]:
                    if not 0 <= item < n["n_items"]:
                        return Verdict(INVALID, "node", k, "leaf_refs")
    # 5
    for i, item in enumerate(fs.inf_refs[:n["n_inf"]]):
        if not 0 <= item < n["n_items"]:
            return Verdict(INVALID, "inf", i, "inf_refs")
    # 6
    for i, o in enumerate(fs.objects[:n["n_objects"]]):
        ty = o["type"]
        if not 0 <= ty < len(fsmod.OBJ_TYPES):
            return Verdict(UNSUPPORTED, "object", i, "type")
        if not vectors(o["bounds_center_off"], 1):
            return Verdict(INVALID, "object", i, "bounds_center_off")
        if not vectors(o["pos_off"], o["n_pos"]):
            return Verdict(INVALID, "object", i, "pos")
        if not vectors(o["dir_off"], o["n_dir"]):
            return Verdict(INVALID, "object", i, "dir")
        if not pool(o["size_off"], o["n_size"], "n_sizes"):
            return Verdict(INVALID, "object", i, "size")
        if not pool(o["flag_off"], o["n_flag"], "n_flags"):
            return Verdict(INVALID, "object", i, "flag")
        pos, dirs, size, flag = o["n_pos"], o["n_dir"], o["n_size"], o["n_flag"]
        if ty == T["sphere"]:
            ok = pos >= 1 and size >= 1
        elif ty == T["hplane"]:
            ok = pos >= 1 and dirs >= 1
        elif ty == T["hdisk"]:
            ok = pos >= 1 and dirs >= 1 and size >= 1
        elif ty == T["cylinder"]:
            ok = pos >= 2 and size >= 1
        elif ty == T["hcylinder"]:
            ok = pos >= d - 1 and size >= 1
        elif ty == T["orthotope"]:
            ok = pos >= 1 and flag >= 1 and 0 <= fs._flags[o["flag_off"]] <= min(dirs, d)
        elif ty == T["hfacet"]:
            ok = pos >= 3 and flag >= 1 and (fs._flags[o["flag_off"]] == 0 or dirs >= 3)
        elif ty == T["facet"]:
            ok = pos >= 3 and dirs >= 1
        else:
            if o["n_obj"] < 1:
                return Verdict(UNSUPPORTED, "object", i, "n_obj")
            if not pool(o["obj_off"], o["n_obj"], "n_obj_refs"):
                return Verdict(INVALID, "object", i, "obj")
            for c in fs._obj_refs[o["obj_off"]:o["obj_off"] + o["n_obj"]]:
                if not 0 <= c < n["n_objects"] or fs.objects[c]["type"] == T["hcube"]:
                    return Verdict(INVALID, "object", i, "obj_refs")
            ok = True
        if not ok:
            return Verdict(INVALID, "object", i, "plugin")
    # 7
    for key in ("lower", "upper"):
        if not vectors(fs.bb[key], 1):
            return Verdict(INVALID, "scene", None, "bb_%s_off" % key)
    # 8
    for i, l in enumerate(fs.lights[:n["n_lights"]]):
        ty = l["type"]
        if not fsmod.LIGHT_AMBIENT <= ty <= fsmod.LIGHT_RECT:
            return Verdict(INVALID, "light", i, "type")
        area = ty in (fsmod.LIGHT_DISK, fsmod.LIGHT_RECT)
        if area and not vectors(l.get("area_off", -1), 2):
            return Verdict(INVALID, "light", i, "area_off")
        if (area or ty in (fsmod.LIGHT_POINT, fsmod.LIGHT_SPOT)) and not vectors(l["pos_off"], 1):
            return Verdict(INVALID, "light", i, "pos_off")
        if ty in (fsmod.LIGHT_DIRECTIONAL, fsmod.LIGHT_SPOT) and not vectors(l["dir_off"], 1):
            return Verdict(INVALID, "light", i, "dir_off")
    # 9
    for key in ("pos", "img_orig", "dir_x", "dir_y"):
        if not vectors(fs.cam[key], 1):
            return Verdict(INVALID, "scene", None, "cam_%s_off" % key)
    for key in ("left_eye", "right_eye", "local_x", "local_y", "local_z"):
        if cam(key) >= 0 and not vectors(cam(key), 1):
            return Verdict(INVALID, "scene", None, "cam_%s_off" % key)
    return None


def library_verdict(fs):
    """(code, message) of ndt_hip_check_scene, or None."""
    try:
        nh.check_scene(fs)
    except nh.NdtHipError as e:
        return e.code, str(e)
    return None


NAMED = {"object": "object %d", "node": "kd node %d", "light": "light %d", "inf": "infinite list entry %d"}


def scene_word(field):
    """What the message of a refusal that is about no object, node or light says of the field at fault: a count by its name, an array
    as NULL, the rest by the words of their rule.  Without it a later rule's refusal with the same code would pass for this one."""
    if field in dict(ARRAYS):
        return field + " is NULL"
    if field.startswith("cam_") and field.endswith("_off"):
        return "camera vectors"
    return {"abi_version": "ABI", "dims": "dimensions", "cam_type": "camera type", "n_lights": "lights", "bb_lower_off": "root box",
            "bb_upper_off": "root box"}.get(field, field)


def disagreement(fs, label):
    """None, or how the library's verdict on `fs` differs from the model's."""
    want, got = model_verdict(fs), library_verdict(fs)
    if want is None or got is None:
        return None if want is None and got is None else "%s: model %s, library %s" % (label, want, got)
    if got[0] != want.code:
        return "%s: model %s, library %s" % (label, want, got)
    if want.kind == "scene" and scene_word(want.field) not in got[1]:
        return "%s: the message does not say '%s': %s" % (label, scene_word(want.field), got[1])
    if want.kind in NAMED and not re.search(r"\b%s\b" % (NAMED[want.kind] % want.index), got[1]):
        return "%s: the message does not name %s: %s" % (label, NAMED[want.kind] % want.index, got[1])
    return None


# ------------------------------------------------------------------------------------------------ the mutation table

class Mutation:
    """`apply(fs)` edits a clone of fixture `base` and may return lies for sealed(); `field` = (struct, field) when the mutation is a
    value of one struct field; `kind` names the refusal it stands for on the device (one mutation a kind is uploaded there)."""

    def __init__(self, base, label, apply, field=None, kind=None):
        self.base, self.label, self.apply, self.field, self.kind = base, "%s: %s" % (base, label), apply, field, kind

    def scene(self):
        fs = clone(base(self.base))
        return sealed(fs, self.apply(fs))


def four(first_out):
    """-1, the first value out of range, the last one in range, 2^31 - 1."""
    return [-1, first_out, first_out - 1, BIG]


def set_record(rows, i, key, value):
    def apply(fs):
        getattr(fs, rows)[i][key] = value
    return apply


def set_attr(key, value):
    def apply(fs):
        setattr(fs, key, value)
    return apply


def set_in(mapping, key, value):
    def apply(fs):
        getattr(fs, mapping)[key] = value
    return apply


def set_entry(rows, i, value):
    def apply(fs):
        getattr(fs, rows)[i] = value
    return apply


def tell(**lie):
    return lambda fs: lie


def parents(fs):
    up = {}
    for k, node in enumerate(fs.kd_nodes):
        if node["dim"] >= 0:
            up[node["left"]], up[node["right"]] = k, k
    return up


def subtree(fs, k):
    out, todo = [], [k]
    while todo:
        k = todo.pop()
        out.append(k)
        if fs.kd_nodes[k]["dim"] >= 0:
            todo += [fs.kd_nodes[k]["left"], fs.kd_nodes[k]["right"]]
    return out


def chain(levels):
    """The whole tree replaced by a left-leaning chain of `levels` levels: node i < levels - 1 splits dimension 0 above the root box
    (everything is to its left), its left child is node i + 1, its right child an empty leaf of its own; the node at the last level is
    the leaf that lists every finite item."""
    def apply(fs):
        items = sorted(set(fs.leaf_refs))
        plane = float(fs.vec(fs.bb["upper"])[0] + 1.0)
        empty = {"dim": -1, "boundary": 0.0, "left": -1, "right": -1, "num": 0, "first": 0}
        nodes = [{"dim": 0, "boundary": plane, "left": i + 1, "right": levels + i, "num": 0, "first": 0} for i in range(levels - 1)]
        nodes.append(dict(empty, num=len(items)))
        nodes += [dict(empty) for _ in range(levels - 1)]
        fs.kd_nodes, fs.leaf_refs = nodes, items
    return apply


def stray_node(fs):
    """One more kd node that no node names, with a leaf range far out of bounds: not reached, so not judged, so never read."""
    fs.kd_nodes.append({"dim": -1, "boundary": 0.0, "left": BIG, "right": BIG, "num": BIG, "first": BIG})


def with_axes(cam_type):
    def apply(fs):
        for key in ("local_x", "local_y", "local_z"):
            fs.cam[key] = fs.cam["dir_x"]
        fs.cam_type = cam_type
    return apply


def area_light(area_off):
    def apply(fs):
        point = next(i for i, l in enumerate(fs.lights) if l["type"] == fsmod.LIGHT_POINT)
        fs.lights[point].update(type=fsmod.LIGHT_DISK, area_off=area_off, radius=0.5)
    return apply


def many_lights(count):
    def apply(fs):
        fs.lights = [dict(fs.lights[i % len(fs.lights)]) for i in range(count)]
    return apply


def wide_orthotope(i, flag):
    """Orthotope i with five directions (the first five vectors of the pool) and flags[flag_off] = flag: min(n_dir, dims) is dims."""
    def apply(fs):
        fs.objects[i].update(n_dir=5, dir_off=0)
        fs._flags[fs.objects[i]["flag_off"]] = flag
    return apply


def hfacet_normals(i, n_dir):
    def apply(fs):
        fs.objects[i]["n_dir"] = n_dir
        fs._flags[fs.objects[i]["flag_off"]] = 1
    return apply


def table_of(name):
    fs = base(name)
    d, nv, ns, nf, nr = fs.dims, len(fs._vecs), len(fs._sizes), len(fs._flags), len(fs._obj_refs)
    nk, nl, no = len(fs.kd_nodes), len(fs.leaf_refs), len(fs.objects)
    out = []

    def add(label, apply, field=None, kind=None):
        out.append(Mutation(name, label, apply, field, kind))

    S, O, L, K = "FlatSceneStruct", "FlatObject", "FlatLight", "FlatKdNode"
    # ---- the scene's own fields
    for v in (2, 4, -1, BIG):
        add("abi_version %d" % v, tell(abi_version=v), (S, "abi_version"), "abi" if v == 2 else None)
    for v in [-1, 2, 3, 12, 13, BIG]:
        add("dims %d" % v, set_attr("dims", v), (S, "dims"), {2: "dims below", 13: "dims above"}.get(v))
    for v in four(3):
        add("cam_type %d" % v, set_attr("cam_type", v), (S, "cam_type"), "camera type" if v == 3 else None)
        add("cam_type %d with axes" % v, with_axes(v), (S, "cam_type"))
    add("VR camera without axes", set_attr("cam_type", 1), (S, "cam_type"), "vr without axes")
    for count, length in (("n_vecs", nv), ("n_sizes", ns), ("n_flags", nf), ("n_obj_refs", nr), ("n_leaf_refs", nl)):
        # a pool's count: the library reads what is referenced, so a count beyond the memory behind an unchanged scene reads nothing new
        for v in (-1, 0, length - 1, length, BIG):
            add("%s %d" % (count, v), tell(**{count: v}), (S, count), "negative pool count" if (count, v) == ("n_vecs", -1) else None)
    for count, length in (("n_objects", no), ("n_kd_nodes", nk), ("n_inf", len(fs.inf_refs))):
        # a count of records that are all read: nothing above the real length can be told without reading beyond the array
        for v in (-1, 0, length - 1, length):
            add("%s %d" % (count, v), tell(**{count: v}), (S, count), "negative count" if (count, v) == ("n_objects", -1) else None)
    for v in (-1, MAX_LIGHTS + 1, BIG):
        add("n_lights %d" % v, tell(n_lights=v), (S, "n_lights"), "too many lights" if v == MAX_LIGHTS + 1 else None)
    add("n_lights %d" % MAX_LIGHTS, many_lights(MAX_LIGHTS), (S, "n_lights"))
    add("n_lights 0", many_lights(0), (S, "n_lights"))
    for v in four(no + 1):
        add("n_items %d" % v, set_attr("n_items", v), (S, "n_items"), "n_items > n_objects" if v == no + 1 else None)
    for key in ("pos", "img_orig", "dir_x", "dir_y", "left_eye", "right_eye", "local_x", "local_y", "local_z"):
        for v in four(nv - d + 1) + [-2]:
            kind = {("pos", nv - d + 1): "camera vector", ("left_eye", nv - d + 1): "camera eye"}.get((key, v))
            add("cam_%s_off %d" % (key, v), set_in("cam", key, v), (S, "cam_%s_off" % key), kind)
    for key in ("lower", "upper"):
        for v in four(nv - d + 1):
            add("bb_%s_off %d" % (key, v), set_in("bb", key, v), (S, "bb_%s_off" % key), "root box" if (key, v) == ("upper", nv - d + 1) else None)
    for array, count in ARRAYS:
        # a count made positive over a NULL array (c3_random4d has no infinite list: there the count is a lie too), and NULL over no entries
        lie = {array: None}
        if count == "n_inf" and not fs.inf_refs:
            lie[count] = 1
        add("%s NULL under its count" % array, tell(**lie), kind="null array" if array == "kd_nodes" else None)
        add("%s NULL, %s 0" % (array, count), tell(**{array: None, count: 0}))
    # ---- objects: the first of every type, nested ones apart
    firsts = {}
    for i, o in enumerate(fs.objects):
        firsts.setdefault((o["type"], o["parent"] >= 0), i)
    for (ty, nested), i in sorted(firsts.items()):
        o = fs.objects[i]
        who = "object %d (%s%s)" % (i, fsmod.OBJ_TYPES[ty], ", nested" if nested else "")
        first_out = {"type": len(fsmod.OBJ_TYPES), "bounds_center_off": nv - d + 1,
                     "pos_off": nv - o["n_pos"] * d + 1, "n_pos": (nv - o["pos_off"]) // d + 1,
                     "dir_off": nv - o["n_dir"] * d + 1, "n_dir": (nv - o["dir_off"]) // d + 1,
                     "size_off": ns - o["n_size"] + 1, "n_size": ns - o["size_off"] + 1,
                     "flag_off": nf - o["n_flag"] + 1, "n_flag": nf - o["flag_off"] + 1,
                     "obj_off": nr - o["n_obj"] + 1, "n_obj": nr - o["obj_off"] + 1}
        kinds = {("sphere", "type"): "object type", ("sphere", "bounds_center_off"): "bounds centre", ("sphere", "pos_off"): "vector range",
                 ("sphere", "size_off"): "size range", ("sphere", "flag_off"): "flag range", ("hcube", "obj_off"): "child range"}
        for key, edge in first_out.items():
            # (beside the four values: the counts around what a plugin reads -- 0, 1, 2, dims - 2)
            for v in four(edge) + ([0, 1, 2, d - 2] if key.startswith("n_") else []):
                kind = kinds.get((fsmod.OBJ_TYPES[ty], key)) if v == edge and not nested else None
                if (fsmod.OBJ_TYPES[ty], key, v) == ("sphere", "n_size", 0):
                    kind = "plugin parameters"
                if (fsmod.OBJ_TYPES[ty], key, v) == ("hcube", "n_obj", 0):
                    kind = "hcube without faces"
                add("%s %s %d" % (who, key, v), set_record("objects", i, key, v), (O, key), kind)
        if ty == T["orthotope"]:
            most = min(o["n_dir"], d)
            for v in four(most + 1):
                add("%s flags[flag_off] %d" % (who, v), set_entry("_flags", o["flag_off"], v))
            for v in (d, d + 1):
                add("%s five directions, flags[flag_off] %d" % (who, v), wide_orthotope(i, v))
        if ty == T["hfacet"]:
            for v in (2, 3):
                add("%s vertex normals with %d directions" % (who, v), hfacet_normals(i, v))
        if ty == T["hcube"]:
            other = next((j for j, p in enumerate(fs.objects) if p["type"] == T["hcube"] and j != i), i)
            add("%s lists hcube %d" % (who, other), set_entry("_obj_refs", o["obj_off"], other), kind="hcube lists an hcube")
            for v in four(no):
                add("%s lists object %d" % (who, v), set_entry("_obj_refs", o["obj_off"] + o["n_obj"] - 1, v),
                    kind="nested index" if v == no else None)
    # ---- lights: the first of every type, and a point light made a disk
    first_light = {}
    for i, l in enumerate(fs.lights):
        first_light.setdefault(l["type"], i)
    for ty, i in sorted(first_light.items()):
        for key, edge in (("type", fsmod.LIGHT_RECT + 1), ("pos_off", nv - d + 1), ("dir_off", nv - d + 1), ("area_off", nv - 2 * d + 1)):
            for v in four(edge):
                kind = {(fsmod.LIGHT_POINT, "type", edge): "light type", (fsmod.LIGHT_POINT, "pos_off", -1): "light position",
                        (fsmod.LIGHT_DIRECTIONAL, "dir_off", -1): "light direction"}.get((ty, key, v))
                add("light %d (type %d) %s %d" % (i, ty, key, v), set_record("lights", i, key, v), (L, key), kind)
    for v in four(nv - 2 * d + 1):
        add("a disk light's area_off %d" % v, area_light(v), (L, "area_off"), "area light without area_off" if v == -1 else None)
    # ---- the kd-tree: the root, the last interior node, the first leaf that lists something, the last leaf
    interior = [k for k, node in enumerate(fs.kd_nodes) if node["dim"] >= 0]
    leaves = [k for k, node in enumerate(fs.kd_nodes) if node["dim"] < 0]
    listing = [k for k in leaves if fs.kd_nodes[k]["num"] > 0]
    for k in sorted({interior[0], interior[-1], listing[0], leaves[-1]}):
        node = fs.kd_nodes[k]
        who = "kd node %d (%s)" % (k, "interior" if node["dim"] >= 0 else "leaf of %d" % node["num"])
        for key, edge in (("dim", d), ("left", nk), ("right", nk), ("num", nl - node["first"] + 1), ("first", nl - node["num"] + 1)):
            for v in four(edge):
                kind = {(interior[-1], "dim", d): "split dimension", (interior[-1], "left", nk): "kd child index",
                        (listing[0], "num", edge): "leaf range"}.get((k, key, v)) if v == edge else None
                add("%s %s %d" % (who, key, v), set_record("kd_nodes", k, key, v), (K, key), kind)
        if node["dim"] < 0 and node["num"] > 0:
            for v in four(fs.n_items):
                add("%s lists item %d" % (who, v), set_entry("leaf_refs", node["first"], v), kind="leaf item" if v == fs.n_items else None)
    up = parents(fs)
    k = interior[-1]
    add("kd node %d: left child is its parent %d" % (k, up[k]), set_record("kd_nodes", k, "left", up[k]), (K, "left"), "child is the parent")
    root = fs.kd_nodes[0]
    inside = next(j for j in subtree(fs, root["left"]) if fs.kd_nodes[j]["dim"] >= 0) if fs.kd_nodes[root["left"]]["dim"] >= 0 else 0
    target = subtree(fs, root["right"])[-1]
    add("kd node %d: right child %d stands in its sibling's subtree" % (inside, target), set_record("kd_nodes", inside, "right", target),
        (K, "right"), "reached twice")
    if fs.inf_refs:
        for v in four(fs.n_items):
            add("inf_refs[0] %d" % v, set_entry("inf_refs", 0, v), kind="infinite item" if v == fs.n_items else None)
    add("a node the walk does not reach, its leaf range out of bounds", stray_node)
    for levels in (KD_STACK, KD_STACK + 1):
        add("a left-leaning chain of %d levels" % levels, chain(levels), kind="chain of 41" if levels == KD_STACK + 1 else None)
    return out


_tables = {}


def table(name):
    if name not in _tables:
        _tables[name] = table_of(name)
    return _tables[name]


DEEP = Mutation("shade3d", "a left-leaning chain of 200000 levels", chain(200000), kind="chain of 200 000")
_deep = []


def deep_scene():
    """DEEP's scene, built once: 399 999 kd nodes."""
    if not _deep:
        _deep.append(DEEP.scene())
    return _deep[0]

# integer fields that are no index and no count, each with the reason
EXCUSED = {
    ("FlatObject", "transparent"): "a truth value (object.h:24): any int is one",
    ("FlatObject", "parent"): "the library does not read it (include/ndt_hip.h, rule 6)",
    ("FlatKdNode", "_pad"): "padding",
    ("FlatSceneStruct", "_pad2"): "padding",
}


# ------------------------------------------------------------------------------------------------ CPU: the table against the model

@pytest.mark.parametrize("name", BASES)
def test_fixtures_pass_model_and_library(name):
    fs = sealed(clone(base(name)))
    assert model_verdict(fs) is None and library_verdict(fs) is None
    assert library_verdict(base(name)) is None


@pytest.mark.parametrize("name", BASES)
def test_library_gives_the_models_verdict(name):
    """Every mutation of the table: accepted by both or refused by both, with the model's code, in a message that names what the
    model names.  The accepted ones -- the last values in range among them -- are judged and nothing else."""
    bad, refused, accepted = [], collections.Counter(), 0
    for m in table(name):
        fs = m.scene()
        want = model_verdict(fs)
        if want is None:
            accepted += 1
        else:
            refused[want.kind, want.field] += 1
            assert want.code in (INVALID, UNSUPPORTED)
        problem = disagreement(fs, m.label)
        if problem:
            bad.append(problem)
    print("%s: %d mutations, %d accepted, %d refused under %d rules" % (name, len(table(name)), accepted, sum(refused.values()), len(refused)))
    assert not bad, "%d of %d:\n%s" % (len(bad), len(table(name)), "\n".join(bad[:40]))
    assert accepted >= len(table(name)) // 8 and sum(refused.values()) >= len(table(name)) // 2      # (both sides of the rules are stood on)


def test_the_deep_chain_is_refused_on_the_way_down():
    """200 000 levels: refused at level 41 (the walk goes no deeper), not after a recursion as deep as the chain."""
    fs = deep_scene()
    assert len(fs.kd_nodes) == 2 * 200000 - 1
    want = model_verdict(fs)
    assert want == Verdict(UNSUPPORTED, "node", KD_STACK, "depth")
    assert disagreement(fs, DEEP.label) is None


def test_messages_of_the_four_holes():
    """The refusals upload did not make before the check was stated once (it dereferenced, recursed, or let the value through): each is one now."""
    fs = base("zoo4d")
    for lie, word in (({"kd_nodes": None}, "kd_nodes is NULL"), ({"leaf_refs": None}, "leaf_refs is NULL"), ({"inf_refs": None}, "inf_refs is NULL"),
                      ({"obj_refs": None}, "obj_refs is NULL"), ({"sizes": None}, "sizes is NULL"), ({"flags": None}, "flags is NULL"),
                      ({"n_vecs": -1}, "n_vecs -1"), ({"n_sizes": -1}, "n_sizes -1"), ({"n_flags": -1}, "n_flags -1"), ({"n_obj_refs": -1}, "n_obj_refs -1")):
        code, message = library_verdict(sealed(clone(fs), lie))
        assert code == INVALID and word in message, (lie, message)
    code, message = library_verdict(deep_scene())
    assert code == UNSUPPORTED and "kd node %d" % KD_STACK in message and "depth %d" % (KD_STACK + 1) in message


COUNTS = ["n_lights", "n_objects", "n_items", "n_kd_nodes", "n_leaf_refs", "n_inf", "n_vecs", "n_sizes", "n_flags", "n_obj_refs"]


@pytest.mark.parametrize("variant", ["D6", "D7"])
@pytest.mark.parametrize("count", COUNTS)
def test_negative_counts_of_scenes_that_list_nothing(variant, count):
    """A count of -1 where nothing is listed (D6) and where there is nothing at all (D7): no later rule meets an index it could
    refuse, so the rule about the count alone stands between -1 and the kernels."""
    fs = sealed(clone(degenerate(3, variant)), {count: -1})
    assert model_verdict(fs) == Verdict(INVALID, "scene", None, count)
    assert disagreement(fs, "%s %s -1" % (variant, count)) is None
    code, message = library_verdict(fs)
    assert code == INVALID and "%s -1" % count in message, message


def test_no_scene_at_all_is_refused():
    lib = nh.load_library()
    assert lib.ndt_hip_check_scene(None) == INVALID and b"NULL" in lib.ndt_hip_last_error()


def integer_fields(struct):
    return [name for name, ty in struct._fields_ if ty in (C.c_int32, C.c_int64)]


def test_every_integer_field_is_judged_or_excused():
    """A field added to one of the four structs fails here until it is in the table or in EXCUSED with its reason."""
    judged = {m.field for name in BASES for m in table(name) if m.field}
    structs = {"FlatSceneStruct": FlatSceneStruct, "FlatObject": FlatObject, "FlatLight": FlatLight, "FlatKdNode": FlatKdNode}
    every = {(s, f) for s, struct in structs.items() for f in integer_fields(struct)}
    assert judged <= every and set(EXCUSED) <= every, (judged - every, set(EXCUSED) - every)
    assert not judged & set(EXCUSED)
    assert every - judged - set(EXCUSED) == set(), "neither judged nor excused: %s" % sorted(every - judged - set(EXCUSED))
    assert all(len(reason) > 5 for reason in EXCUSED.values())
    # ... and every base scene stands on every field it can (zoo12d and shade3d have no hcube: obj_off / n_obj are read of none)
    for name in BASES:
        assert {m.field for m in table(name) if m.field} == judged, name


def test_every_kind_of_refusal_has_one_mutation_for_the_device():
    kinds = collections.Counter(m.kind for m in device_refusals())
    assert all(c == 1 for c in kinds.values()), kinds
    assert sorted(kinds) == sorted(KINDS), (set(KINDS) - set(kinds), set(kinds) - set(KINDS))
    for m in device_refusals():
        assert model_verdict(m.scene()) is not None, m.label


# every kind of refusal the check makes, as the table names them
KINDS = ["abi", "dims below", "dims above", "camera type", "vr without axes", "negative pool count", "negative count", "too many lights",
         "n_items > n_objects", "camera vector", "camera eye", "root box", "null array", "object type", "bounds centre", "vector range",
         "size range", "plugin parameters", "flag range", "light type", "light position", "light direction", "area light without area_off",
         "leaf range", "leaf item", "split dimension", "kd child index", "child is the parent", "reached twice", "infinite item",
         "chain of 41", "child range", "hcube without faces", "hcube lists an hcube", "nested index", "chain of 200 000"]


def device_refusals():
    """One mutation a kind: of the first base scene that has it."""
    out, have = [], set()
    for m in [m for name in BASES for m in table(name)] + [DEEP]:
        if m.kind and m.kind not in have:
            have.add(m.kind)
            out.append(m)
    return out


# ------------------------------------------------------------------------------------------------ degenerate scenes

DIM_SCENES = {3: "shade3d", 4: "zoo4d", 7: "shade7d", 12: "shade12d"}
VARIANTS = ["D1", "D2", "D3", "D4", "D5", "D6", "D7", "D8"]
EMPTY_LEAF = {"dim": -1, "boundary": 0.0, "left": -1, "right": -1, "num": 0, "first": 0}
_degenerate = {}


def degenerate(dims, variant):
    """D1 no lights; D2 ambient lights only; D3 no kd node, the infinite list kept; D4 the root is an empty leaf; D5 no infinite list;
    D6 objects present, listed nowhere; D7 no objects at all; D8 one item -- the widest of the finite spheres, the first of them
    where two are as wide -- in a one-leaf tree, nothing else listed."""
    if (dims, variant) not in _degenerate:
        fs = clone(base(DIM_SCENES[dims]))
        if variant == "D1":
            fs.lights = []
        elif variant == "D2":
            fs.lights = [l for l in fs.lights if l["type"] == fsmod.LIGHT_AMBIENT]
        elif variant == "D3":
            fs.kd_nodes, fs.leaf_refs = [], []
        elif variant == "D4":
            fs.kd_nodes, fs.leaf_refs = [dict(EMPTY_LEAF)], []
        elif variant == "D5":
            fs.inf_refs = []
        elif variant == "D6":
            fs.kd_nodes, fs.leaf_refs, fs.inf_refs = [], [], []
        elif variant == "D7":
            fs.kd_nodes, fs.leaf_refs, fs.inf_refs, fs.objects, fs.n_items = [], [], [], [], 0
            fs._sizes, fs._flags, fs._obj_refs = [], [], []
        elif variant == "D8":
            spheres = [i for i in sorted(set(fs.leaf_refs)) if fs.objects[i]["type"] == T["sphere"]]
            item = max(spheres, key=lambda i: fs.objects[i]["bounds_radius"])
            fs.kd_nodes, fs.leaf_refs, fs.inf_refs = [dict(EMPTY_LEAF, num=1)], [item], []
        _degenerate[dims, variant] = sealed(fs)
    return _degenerate[dims, variant]


CASES = [(dims, variant) for dims in DIM_SCENES for variant in VARIANTS]
SMALL_SIZES = [(1, 1), (1, 9), (9, 1)]
SMALL_SCENES = ["shade4d"] + ["D3 of %d-D" % dims for dims in DIM_SCENES]
_small = {}


def small_scene(name):
    if name not in _small:
        _small[name] = sealed(clone(base(name))) if name == "shade4d" else degenerate(int(name.split()[2].split("-")[0]), "D3")
    return _small[name]


def case_id(case):
    return "%dd-%s" % case


_oracle_frames = {}


def oracle_frame(oracle, fs, key, size=(W, H)):
    """The oracle's (rgba, depth map, stats) of a scene: computed once, shared, never written to."""
    if key not in _oracle_frames:
        img, dm, st = oracle.render(fs, size[0], size[1], DEPTH, depth_map=True)
        img.setflags(write=False)
        dm.setflags(write=False)
        _oracle_frames[key] = (img, dm, st)
    return _oracle_frames[key]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_degenerate_scenes_pass_and_show_what_they_should(oracle, case):
    """Conditions on the inputs: the model and the library take every degenerate scene; D1 .. D5 and D8 show hits in more than a
    handful of colours; D6 and D7 are the background in every pixel -- one colour, every channel within one ulp of the scene's background (the
    reference's pixel arithmetic rounds once) -- and no ray beyond the primaries is made."""
    dims, variant = case
    fs = degenerate(dims, variant)
    assert fs.dims == dims and model_verdict(fs) is None and library_verdict(fs) is None
    img, dm, st = oracle_frame(oracle, fs, case)
    assert np.isfinite(img).all() and np.isfinite(dm).all() and st.rays_primary == W * H
    colours = len(np.unique(img.reshape(-1, 4), axis=0))
    print("%s: %d pixels hit, %d colours, rays %s" % (case_id(case), int((dm > 0).sum()), colours, ray_counts(st)))
    if variant in ("D6", "D7"):
        assert colours == 1 and (np.abs(img - np.array(fs.background)) <= np.spacing(np.array(fs.background))).all()
        assert not (dm > 0).any() and (st.rays_secondary, st.rays_shadow) == (0, 0)
    else:
        assert (dm > 0).any() and colours > HANDFUL, (case, colours)
        assert (st.rays_shadow == 0) == (variant in ("D1", "D2"))
    assert (len(fs.kd_nodes), len(fs.leaf_refs)) == {"D3": (0, 0), "D4": (1, 0), "D6": (0, 0), "D7": (0, 0), "D8": (1, 1)}.get(
        variant, (len(base(DIM_SCENES[dims]).kd_nodes), len(base(DIM_SCENES[dims]).leaf_refs)))


# ------------------------------------------------------------------------------------------------ GPU

DEFAULTS = dict(VIEW_DEFAULTS, item_sets=1)
# every way of test_view_modes, and the four-word register kernels (item_sets 0) under both pipelines
RUNS = SETTINGS + [("pipeline 1, item_sets 0", {"pipeline": 1, "item_sets": 0}), ("pipeline 2, item_sets 0", {"pipeline": 2, "item_sets": 0})]
SMALL_RUNS = [("pipeline 1", {"pipeline": 1}), ("pipeline 2", {"pipeline": 2})]


@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    for name, value in DEFAULTS.items():
        ctx.set_option(name, value)
    ctx.close()


@contextlib.contextmanager
def under(gpu, fs, options):
    """The options on top of the defaults and the scene uploaded under them (light_window and item_sets are read at upload); every
    option is back at its default afterwards, whatever happened."""
    try:
        for name, value in dict(DEFAULTS, **options).items():
            gpu.set_option(name, value)
        gpu.upload_scene(fs)
        yield gpu
    finally:
        for name, value in DEFAULTS.items():
            gpu.set_option(name, value)


def hold_frames(gpu, oracle, fs, key, runs, size=(W, H)):
    """The frame of `fs` under every setting of `runs`: the oracle's image, map and ray counts at the project's tolerance with no pixel
    left out, the same bytes and counts from every setting; then trace_rays on the frame's own primary rays against oracle.trace."""
    assert model_verdict(fs) is None, key          # (nothing the model refuses reaches a kernel)
    w, h = size
    got = {}
    for what, options in runs:
        with under(gpu, fs, options):
            got[what] = gpu.render(w, h, DEPTH, depth_map=True)
    wimg, wdm, wst = oracle_frame(oracle, fs, key, size)
    first = runs[0][0]
    img, dm, st = got[first]
    d_img, d_map = float(np.abs(img - wimg).max()), float(np.abs(dm - wdm).max())
    print("%s %dx%d: max |device - oracle| image %.3g map %.3g, rays %s (oracle %s)" % (key, w, h, d_img, d_map, ray_counts(st), ray_counts(wst)))
    assert img.shape == wimg.shape and dm.shape == wdm.shape
    assert d_img < TOL_TIGHT and d_map < TOL_TIGHT, (key, first, d_img, d_map)
    assert ray_counts(st) == ray_counts(wst), (key, first)
    for what, _ in runs[1:]:
        assert got[what][0].tobytes() == img.tobytes() and got[what][1].tobytes() == dm.tobytes(), (key, what)
        assert ray_counts(got[what][2]) == ray_counts(st), (key, what)
    for options in ({}, {"item_sets": 0}):
        with under(gpu, fs, options):
            out = gpu.render_features(w, h, DEPTH, rays=True)
            rays = np.concatenate([np.moveaxis(out["ray_o"], 0, -1).reshape(-1, fs.dims), np.moveaxis(out["ray_v"], 0, -1).reshape(-1, fs.dims),
                                   -np.ones((w * h, 1))], axis=1)
            obj, hit, nrm = gpu.trace_rays(rays)
        wobj, whit, wnrm = oracle.trace(fs, rays)
        assert np.array_equal(obj, wobj), (key, options)
        assert np.array_equal(obj >= 0, dm.reshape(-1) > 0), (key, options)
        hits = obj >= 0         # (bit for bit where there is an answer; a miss leaves zeros of either sign)
        assert hit[hits].tobytes() == whit[hits].tobytes() and nrm[hits].tobytes() == wnrm[hits].tobytes(), (key, options)
        assert np.array_equal(hit[~hits], whit[~hits]) and np.array_equal(nrm[~hits], wnrm[~hits]), (key, options)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_degenerate_scenes_under_every_way_of_rendering_them(gpu, oracle, case):
    hold_frames(gpu, oracle, degenerate(*case), case, RUNS)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SMALL_SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", SMALL_SCENES)
def test_smallest_frames(gpu, oracle, name, size):
    hold_frames(gpu, oracle, small_scene(name), (name, size), SMALL_RUNS, size)


def trace_one_ray(gpu, dims):
    """ndt_hip_trace_rays itself on one ray (the binding's own guard for a context without a scene left out): its return code."""
    ray = np.zeros((3, dims))
    ray[1, 0] = 1.0
    lim, obj = -np.ones(1), np.zeros(1, dtype=np.int32)
    out = np.zeros((2, dims))
    return gpu.lib.ndt_hip_trace_rays(gpu.ctx, 1, ray[0].ctypes.data, ray[1].ctypes.data, lim.ctypes.data, obj.ctypes.data,
                                      out[0].ctypes.data, out[1].ctypes.data)


@pytest.mark.gpu
def test_no_scene_at_all_costs_the_context_its_scene(gpu):
    """ndt_hip_upload_scene(ctx, NULL): refused like any scene, and the context is without one afterwards."""
    good = base("shade3d")
    gpu.upload_scene(good)
    before = gpu.render(W, H, DEPTH, depth_map=True)
    assert gpu.lib.ndt_hip_upload_scene(gpu.ctx, None) == INVALID
    with pytest.raises(nh.NdtHipError) as e:
        gpu.render(W, H, DEPTH)
    assert e.value.code == STATE and trace_one_ray(gpu, good.dims) == STATE
    gpu.upload_scene(good)
    img, dm, st = gpu.render(W, H, DEPTH, depth_map=True)
    assert img.tobytes() == before[0].tobytes() and dm.tobytes() == before[1].tobytes() and ray_counts(st) == ray_counts(before[2])


@pytest.mark.gpu
def test_refusals_on_the_device(gpu):
    """One mutation of every kind: upload refuses it with the check's code and message; the render that follows has no scene; the good
    scene uploaded again renders the bytes it rendered before.  A scene the model refuses is never rendered: were one accepted, the
    test ends at that upload."""
    before = {}
    for m in device_refusals():
        good = base(m.base)
        if m.base not in before:
            gpu.upload_scene(good)
            before[m.base] = gpu.render(W, H, DEPTH, depth_map=True)
        bad = deep_scene() if m is DEEP else m.scene()
        assert model_verdict(bad) is not None, m.label
        want = library_verdict(bad)
        assert want is not None, m.label
        gpu.upload_scene(good)
        with pytest.raises(nh.NdtHipError) as e:
            gpu.upload_scene(bad)
        assert (e.value.code, str(e.value)) == want, m.label
        with pytest.raises(nh.NdtHipError) as e:
            gpu.render(W, H, DEPTH)
        assert e.value.code == STATE, m.label
        assert trace_one_ray(gpu, good.dims) == STATE and gpu.scene is None, m.label
        gpu.upload_scene(good)
        img, dm, st = gpu.render(W, H, DEPTH, depth_map=True)
        assert img.tobytes() == before[m.base][0].tobytes() and dm.tobytes() == before[m.base][1].tobytes(), m.label
        assert ray_counts(st) == ray_counts(before[m.base][2]), m.label


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shade3d", "c3_random4d"])
def test_a_node_the_walk_does_not_reach_is_not_read(gpu, name):
    """Accepted by the model and by the check, which do not look at it: the upload must not look at it either (with item sets and
    without), and the frame is the fixture's, byte for byte."""
    good, stray = sealed(clone(base(name))), clone(base(name))
    stray_node(stray)
    sealed(stray)
    assert model_verdict(stray) is None and library_verdict(stray) is None
    for options in ({}, {"item_sets": 0}):
        with under(gpu, good, options):
            want = gpu.render(W, H, DEPTH, depth_map=True)
        with under(gpu, stray, options):
            got = gpu.render(W, H, DEPTH, depth_map=True)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (name, options)
        assert ray_counts(got[2]) == ray_counts(want[2]), (name, options)


@pytest.mark.gpu
def test_a_good_scene_after_a_late_refusal_is_the_oracles(gpu, oracle):
    """A scene with a disk light and a VR camera, refused by the last rule there is (its last camera vector), then the planar,
    point-lit fixture: the oracle's deterministic frame under both pipelines.  This holds the sequence to the oracle; it cannot see a
    field of the refused scene lingering in the context, since the upload that follows writes every such field again.  What can be
    seen of a refusal -- no scene afterwards -- is test_refusals_on_the_device's."""
    fs = clone(base("shade3d"))
    area_light(0)(fs)
    with_axes(1)(fs)
    fs.cam["local_z"] = len(fs._vecs) - fs.dims + 1
    bad = sealed(fs)
    assert model_verdict(bad) == Verdict(INVALID, "scene", None, "cam_local_z_off")
    good = sealed(clone(base("shade3d")))
    wimg, wdm, wst = oracle_frame(oracle, good, "shade3d as it is")
    for pipeline in (1, 2):
        with under(gpu, good, {"pipeline": pipeline}):
            with pytest.raises(nh.NdtHipError) as e:
                gpu.upload_scene(bad)
            assert e.value.code == INVALID
            with pytest.raises(nh.NdtHipError) as e:
                gpu.render(W, H, DEPTH)
            assert e.value.code == STATE
            gpu.upload_scene(good)
            img, dm, st = gpu.render(W, H, DEPTH, depth_map=True)
        assert float(np.abs(img - wimg).max()) < TOL_TIGHT and float(np.abs(dm - wdm).max()) < TOL_TIGHT
        assert ray_counts(st) == ray_counts(wst)
