"""Ambient occlusion of a frame on the device (ndt_ao.hip; `ndt_hip --ao`): from the N-D hit point of every pixel's primary ray, K
rays over the hemisphere of the N-D normal there that faces the viewer, and the cosine-weighted share of them that get away.

The yardsticks are written here and are never the device's own plane:
  * the directions come from the device's log, cos and sin, whose last bits numpy need not give: every entry returns the directions
    it used, and they are checked for what the definition in include/ndt_hip.h says of them (unit length, the viewer's side of the
    normal restated here, zero where no ray is sent, the same for a shard, a prefix, a batch size) and for their distribution;
  * everything behind the directions is restated in numpy (unit_normals, cosines, fold_model) and compared bit for bit
    (view(np.uint64), never a tolerance), with the occlusion of every ray taken from NdtHip.trace_rays on exactly that ray -- the
    entry the aimed-ray tests pin to the reference -- and the CPU oracle asked about the same rays;
  * the files are read by the strict reader of tests/test_exr_features.py, with the channel AO in its place.
"""
import ctypes as C
import importlib.util
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, GOLDEN, golden

from ndt_amd import hip as nh
from ndt_amd import load_scene
import test_exr_features as xf
from test_denoise_device import read_png

NDT_E_INVALID, NDT_E_UNSUPPORTED, NDT_E_STATE = -1, -2, -5
HOST = os.path.join(ROOT, "ndt_amd", "host")
DRIVER = os.path.join(HOST, "ndt_hip")
NEW_SYMBOLS = ("ndt_hip_ao_device", "ndt_hip_render_ao_device", "ndt_hip_render_ao", "ndt_hip_ao_apply_device",
               "ndt_hip_render_ao_shaded_device", "ndt_hip_render_ao_shaded", "ndt_hip_render_ao_shaded_rgba8", "ndt_hip_render_ao_shaded_png",
               "ndt_hip_render_ao_shaded_jpeg", "ndt_hip_exr_ao_bound", "ndt_hip_encode_exr_ao_device", "ndt_hip_render_exr_ao",
               "ndt_hip_ao_launches", "ndt_hip_ao_ms")
NEW_METHODS = ("render_ao", "ao_device", "ao_apply_device", "render_ao_shaded", "render_exr", "ao_launches", "ao_ms")
ALL = ("id", "position", "normal")
AUTO_SLOTS = 1 << 23            # include/ndt_hip.h, option "ao_batch": auto takes as many samples a launch as fit these slots

_spec = importlib.util.spec_from_file_location("make_golden_driver", os.path.join(GOLDEN, "make_golden_driver.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)
# what `ndt_hip --png --deflate gpu` and `ndt_hip --exr --exr-aov all -z` left and said on the commit before --ao (the recorder's scene
# and base flags)
PARENT_RECORD = os.path.join(GOLDEN, "ao_driver_parent.json")
PLAIN_PNG = ["--png", "--deflate", "gpu"]
PLAIN_EXR = ["--exr", "--exr-aov", "all", "-z"]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------- the yardstick

def unit_normals(f):
    """(sends rays, n') of the feature planes f: n / len, negated where it looks away from the viewer; sums over the components in
    ascending order from 0.0, one operation at a time."""
    n, view = f["normal"], f["ray_v"]
    len2 = np.zeros(n.shape[1:])
    for k in range(n.shape[0]):
        len2 = len2 + n[k] * n[k]
    length = np.sqrt(len2)
    sends = (f["id"] != 0) & (length > 0) & np.isfinite(length)
    with np.errstate(all="ignore"):
        unit = np.stack([n[k] / length for k in range(n.shape[0])])
    facing = np.zeros(length.shape)
    for k in range(n.shape[0]):
        facing = facing + unit[k] * view[k]
    return sends, np.where(facing > 0, -unit, unit)


def cosines(dirs, unit):
    """c[s] = sum_k d[s][k] n'[k], ascending from 0.0"""
    c = np.zeros((dirs.shape[0],) + dirs.shape[2:])
    for k in range(dirs.shape[1]):
        c = c + dirs[:, k] * unit[k]
    return c


def fold_model(c, occluded):
    """ao of cosines c[s] and flags occluded[s], s ascending: den = sum c, num = sum of the c that get away, ao = num / den (1.0
    without a den above 0)"""
    den, num = np.zeros(c.shape[1:]), np.zeros(c.shape[1:])
    for s in range(c.shape[0]):
        den = den + c[s]
        num = np.where(occluded[s], num, num + c[s])
    with np.errstate(all="ignore"):
        return np.where(den > 0, num / den, 1.0)


def sample_rays(f, dirs, sends, limit):
    """the (K * P, 2 dims + 1) batch trace_rays takes: from every pixel that sends rays, its K directions (sample-major)"""
    d = dirs.shape[1]
    origin = f["position"][:, sends].T
    rays = np.empty((dirs.shape[0] * origin.shape[0], 2 * d + 1))
    for s in range(dirs.shape[0]):
        block = rays[s * origin.shape[0]:(s + 1) * origin.shape[0]]
        block[:, :d] = origin
        block[:, d:2 * d] = dirs[s][:, sends].T
    rays[:, 2 * d] = limit
    return rays


def plane_model(gpu, f, dirs, radius, oracle=None, scene=None):
    """The definition behind the directions: the occlusion of every ray from NdtHip.trace_rays (dist_limit 0, or -1 and the hit's
    v_dist against the radius), the rest in numpy.  With an oracle: it answers the same rays the same way, bit for bit.  Returns
    (plane, occluded rays, rays)."""
    sends, unit = unit_normals(f)
    c = cosines(dirs, unit)
    out = np.ones(f["id"].shape)
    if not sends.any():
        return out, 0, 0
    K, d = dirs.shape[0], dirs.shape[1]
    rays = sample_rays(f, dirs, sends, -1.0 if radius > 0 else 0.0)
    obj, hit, nrm = gpu.trace_rays(rays)
    if oracle is not None:
        want = oracle.trace(scene, rays)
        assert np.array_equal(obj, want[0]) and xf.same_bits(hit, want[1]) and xf.same_bits(nrm, want[2])
    occluded = obj >= 0
    if radius > 0:
        occluded = occluded & (xf.v_dist(hit.T, rays[:, :d].T) < radius)
    out[sends] = fold_model(c[:, sends], occluded.reshape(K, -1))
    return out, int(occluded.sum()), len(rays)


def apply_model(rgba, plane, strength):
    out = np.array(rgba, dtype=np.float64, copy=True)
    factor = (1.0 - strength) + strength * plane
    with np.errstate(invalid="ignore"):
        for ch in range(3):
            out[..., ch] = rgba[..., ch] * factor
    return out


def expected_launches(width, rows, K, radius, batch=0, features=True, apply=False):
    n_primary = ((width + 7) // 8) * ((rows + 7) // 8) * 64
    per = min(K, batch if batch > 0 else max(1, AUTO_SLOTS // n_primary))
    return (4 if features else 0) + ((K + per - 1) // per) * (4 if radius > 0 else 3) + (1 if apply else 0)


def ao_channels(fb, dm, planes, mask, pixel_type, plane):
    """the channel list of the file with AO: test_exr_features' model with the FLOAT channel AO behind A"""
    want = xf.model_channels(fb, dm, planes if mask else {}, mask, pixel_type)
    assert want[0][0] == "A"
    return [want[0], ("AO", xf.FLOAT, xf.float_model(plane))] + want[1:]


def plane_yaml(dims):
    """a lone hyperplane across axis 1 at -1, seen level from 4 above it: the horizon crosses the middle of the frame"""
    z = [0.0] * (dims - 3)
    return ("---\nscene: ao_plane\ndimensions: %d\nbackground: {red: 0.1, green: 0.1, blue: 0.3}\ncamera:\n  viewPoint: %r\n  viewTarget: %r\n  up: %r\n"
            "lights:\n- type: LIGHT_AMBIENT\n  name:\n  color: {red: 0.5, green: 0.5, blue: 0.5}\nobjects:\n- name: floor\n  type: hplane\n  dimensions: %d\n"
            "  material:\n    color: {red: 0.7, green: 0.7, blue: 0.7}\n  positions:\n  - %r\n  directions:\n  - %r\n"
            % (dims, [0.0, 3.0, 8.0] + z, [0.0, 3.0, 0.0] + z, [0.0, 1.0, 0.0] + z, dims, [0.0, -1.0, 0.0] + z, [0.0, 1.0, 0.0] + z))


SPHERE_RADIUS = 5.0


def sphere_yaml(dims):
    """one closed sphere of radius 5 around the origin, the camera inside it"""
    z = [0.0] * (dims - 3)
    return ("---\nscene: ao_sphere\ndimensions: %d\nbackground: {red: 0.1, green: 0.1, blue: 0.3}\ncamera:\n  viewPoint: %r\n  viewTarget: %r\n  up: %r\n"
            "lights:\n- type: LIGHT_AMBIENT\n  name:\n  color: {red: 0.5, green: 0.5, blue: 0.5}\nobjects:\n- name: shell\n  type: sphere\n  dimensions: %d\n"
            "  material:\n    color: {red: 0.7, green: 0.7, blue: 0.7}\n  positions:\n  - %r\n  sizes: [%r]\n"
            % (dims, [0.0, 0.0, 2.0] + z, [0.0, 0.0, -5.0] + z, [0.0, 1.0, 0.0] + z, dims, [0.0, 0.0, 0.0] + z, SPHERE_RADIUS))


_known = {}


def known_scene(tmp_path_factory, kind, dims):
    """the flat scene the driver makes of the YAML above (--dump-scene: host code only)"""
    if (kind, dims) not in _known:
        work = tmp_path_factory.mktemp("%s%dd" % (kind, dims))
        y, dump = str(work / "scene.yaml"), str(work / "scene.ndtscene")
        with open(y, "w") as f:
            f.write(plane_yaml(dims) if kind == "plane" else sphere_yaml(dims))
        r = subprocess.run([DRIVER, "-s", "builtin:yaml", "-d", str(dims), "-f", "0", "-r", "16x9", "-u", y, "--dump-scene", dump],
                           capture_output=True, text=True, cwd=str(work))
        assert r.returncode == 0, r.stderr[-2000:]
        _known[kind, dims] = load_scene(dump)
    return _known[kind, dims]


# ---------------------------------------------------------------- CPU

def test_declared_bound_and_exported(tmp_path):
    """(CPU) the header declares every new entry point, hip.py binds it, the library exports it; ndt_ao_params is 32 bytes to a C
    compiler and to ctypes; the ABI version stays."""
    with open(os.path.join(ROOT, "include", "ndt_hip.h")) as f:
        header = f.read()
    lib = nh.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"^(int|double|int64_t) %s\(" % name, header, re.M), name
        assert name in nh.API_SYMBOLS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.ndt_hip_ao_ms.restype is C.c_double and lib.ndt_hip_exr_ao_bound.restype is C.c_int64
    assert lib.ndt_hip_abi_version() == 3 and "#define NDT_HIP_ABI_VERSION 3" in header
    for method in NEW_METHODS:
        assert callable(getattr(nh.NdtHip, method, None)), method
    assert callable(nh.exr_ao_bound) and callable(nh.ao_params)
    assert '"ao_batch"' in header
    a = nh.ao_params()
    assert (a.samples, a.reserved, a.radius, a.seed, a.strength) == (16, 0, 0.0, 0, 1.0)
    assert C.sizeof(nh.AoParams) == 32
    assert (nh.AoParams.samples.offset, nh.AoParams.radius.offset, nh.AoParams.seed.offset, nh.AoParams.strength.offset) == (0, 8, 16, 24)
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ndt_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ndt_ao_params), offsetof(ndt_ao_params, samples),\n'
                   '    offsetof(ndt_ao_params, radius), offsetof(ndt_ao_params, seed), offsetof(ndt_ao_params, strength)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["32", "0", "8", "16", "24"]


def test_the_model_sums_in_the_stated_order():
    """(CPU) cosines 1e16, 1, 1, 1, 1 of one pixel, the large one occluded: den loses the small ones one by one behind the large one,
    and keeps them when they come first; num, which skips the large one, is 4 either way.  (A cosine is at most 1: the fold does not
    care.)"""
    c = np.array([1e16, 1.0, 1.0, 1.0, 1.0]).reshape(5, 1)
    occluded = np.array([True, False, False, False, False]).reshape(5, 1)
    got = fold_model(c, occluded)
    den = 0.0
    for s in range(5):
        den = den + float(c[s, 0])
    assert den == 1e16 and got[0] == 4.0 / den
    backwards = fold_model(c[::-1], occluded[::-1])
    assert backwards[0] == 4.0 / (4.0 + 1e16) and backwards[0] != got[0]
    # the components of a dot product likewise
    unit = np.array([1e17, 1.0, 1.0, 1.0, -1e17]).reshape(5, 1)
    dirs = np.ones((1, 5, 1))
    assert cosines(dirs, unit)[0, 0] == 0.0 and cosines(dirs[:, ::-1], unit[::-1])[0, 0] == 0.0
    unit = np.array([1.0, 1e17, -1e17, 1.0, 1.0]).reshape(5, 1)
    assert cosines(dirs, unit)[0, 0] == 2.0 and cosines(dirs, unit[::-1])[0, 0] == 1.0
    # nothing to divide by: 1.0; everything occluded: 0.0; a pixel that sends no rays has cosines of 0
    assert fold_model(np.zeros((3, 2)), np.zeros((3, 2), dtype=bool)).tolist() == [1.0, 1.0]
    assert fold_model(np.full((3, 1), 0.5), np.ones((3, 1), dtype=bool))[0] == 0.0
    # unit_normals: a zero, an infinite and a NaN normal send no rays; a normal along the view is turned round
    f = {"id": np.array([[1, 1, 1, 1, 0, 1]], dtype=np.int32), "normal": np.zeros((3, 1, 6)), "ray_v": np.zeros((3, 1, 6))}
    f["normal"][0, 0] = [0.0, np.inf, np.nan, 2.0, 2.0, -2.0]
    f["ray_v"][0] = 1.0
    sends, unit = unit_normals(f)
    assert sends.tolist() == [[False, False, False, True, False, True]] and unit[0, 0, 3] == -1.0 and unit[0, 0, 5] == -1.0


def test_exr_ao_bound_is_the_all_raw_file_and_refuses_bad_arguments():
    """(CPU) ndt_hip_exr_ao_bound is the size of the model writer's file when no block compresses: the header with AO in the channel
    list, an offset and a block header a block, the raw samples; the mask may be 0."""
    lib = nh.load_library()
    for dims in (3, 4, 12):
        for mask in range(0, 8):
            for with_z in (False, True):
                for pixel in ("half", "float"):
                    for w, h in ((1, 1), (33, 17), (67, 37)):
                        chans = [(n, xf.PIXEL[pixel] if t is None else t) for n, t in xf.channel_names(dims, mask, with_z)]
                        chans = [chans[0], ("AO", xf.FLOAT)] + chans[1:]
                        assert [n for n, _ in chans] == sorted(n for n, _ in chans)
                        line = sum(w * xf.DTYPE[t].itemsize for _, t in chans)
                        want = len(xf.model_header(w, h, chans)) + 16 * ((h + 15) // 16) + line * h
                        assert nh.exr_ao_bound(w, h, dims, xf.names_of(mask), pixel, with_z) == want, (dims, mask, with_z, pixel, w, h)
                        if mask:
                            assert want == nh.exr_features_bound(w, h, dims, xf.names_of(mask), pixel, with_z) + 4 * w * h + len(b"AO\0") + 16
    # ... which the model writer reaches with incompressible samples in every channel
    rng = np.random.default_rng(3)
    planes = {"id": rng.integers(-2 ** 31, 2 ** 31, (20, 9)).astype(np.int32), "position": xf.noise_doubles((12, 20, 9), 4),
              "normal": xf.noise_doubles((12, 20, 9), 5)}
    data = xf.write_exr(ao_channels(xf.noise_doubles((20, 9, 4), 6), xf.noise_doubles((20, 9), 7), planes, 7, xf.FLOAT, xf.noise_doubles((20, 9), 8)))
    chans, _, _, raw = xf.read_exr(data)
    assert raw == [True, True] and len(data) == nh.exr_ao_bound(9, 20, 12, ALL, "float", True) and [n for n, _ in chans][:3] == ["A", "AO", "B"]
    ep = nh.ExrParams(xf.HALF)
    for dims in (2, 13, 0, -1):
        assert lib.ndt_hip_exr_ao_bound(4, 4, C.byref(ep), 0, dims, 7) == NDT_E_INVALID
    for mask in (8, 15, -1):
        assert lib.ndt_hip_exr_ao_bound(4, 4, C.byref(ep), 0, 4, mask) == NDT_E_INVALID
    for w, h in ((0, 1), (1, 0), (-1, 5), (5, -1)):
        assert lib.ndt_hip_exr_ao_bound(w, h, C.byref(ep), 0, 4, 7) == NDT_E_INVALID
    assert lib.ndt_hip_exr_ao_bound(4, 4, C.byref(nh.ExrParams(3)), 0, 4, 7) == NDT_E_INVALID
    assert lib.ndt_hip_exr_ao_bound(4, 4, None, 1, 4, 0) == nh.exr_ao_bound(4, 4, 4, None, "half", True)
    assert lib.ndt_hip_exr_ao_bound(1 << 14, 1 << 11, None, 1, 12, 7) < 0 and lib.ndt_hip_exr_ao_bound(1 << 13, 1 << 11, None, 1, 12, 7) > 0
    with pytest.raises(ValueError):
        nh.exr_ao_bound(0, 4, 4)
    # the existing feature entries still refuse a mask of 8
    assert lib.ndt_hip_exr_features_bound(4, 4, C.byref(ep), 0, 4, 8) == NDT_E_INVALID


def _run_driver(cwd, *flags, scene="builtin:yaml", dims=4, size="16x9"):
    assert os.path.exists(DRIVER), "ndt_amd/host/ndt_hip is not built"
    os.makedirs(str(cwd), exist_ok=True)
    return subprocess.run([DRIVER, "-s", scene, "-d", str(dims), "-f", "0", "-r", size, "-l", "6"] + list(flags),
                          capture_output=True, text=True, cwd=str(cwd))


def test_driver_refuses_what_ao_does_not_go_with_by_name(tmp_path):
    """(CPU) every refusal ends the run non-zero with one line on stderr that names both flags, before a scene is loaded or a device
    asked for: nothing is written.  The usage text has the new lines; an unknown --exr-aov word is refused in the words it was."""
    for flags, words in ((["--ao", "-a", "20,3"], ("--ao", "-a")),
                         (["--ao", "4", "-m", "a"], ("--ao", "-m a")),
                         (["--ao", "-m", "h"], ("--ao", "-m h")),
                         (["--ao", "3", "-g", "2"], ("--ao", "-g 2")),
                         (["--ao", "--ssaa", "2"], ("--ao", "--ssaa 2")),
                         (["--ao", "--apng"], ("--ao", "--apng")),
                         (["--ao", "--png", "--deflate", "gpu", "--png16"], ("--ao", "--png16")),
                         (["--ao", "--denoise"], ("--ao", "--denoise")),
                         (["--ao", "8", "--denoise", "2", "-n", "2"], ("--ao", "--denoise")),
                         (["--ao", "-z", "--depth", "gpu"], ("--ao", "--depth gpu")),
                         (["--ao", "-z"], ("--ao", "-z", "--exr")),
                         (["--ao", "--png", "-z"], ("--ao", "-z", "--exr")),
                         (["--ao-radius", "2"], ("--ao-radius", "needs --ao")),
                         (["--ao-strength", "0.5", "--png"], ("--ao-strength", "needs --ao")),
                         (["--ao-seed", "7", "--jpeg"], ("--ao-seed", "needs --ao")),
                         (["--ao", "0"], ("--ao", "1 .. 256", "'0'")),
                         (["--ao", "257"], ("--ao", "1 .. 256", "'257'")),
                         (["--ao=x"], ("--ao", "1 .. 256", "'x'")),
                         (["--ao", "--ao-radius", "-1"], ("--ao-radius", "0 or above", "'-1'")),
                         (["--ao", "--ao-radius", "nan"], ("--ao-radius", "0 or above")),
                         (["--ao", "--ao-radius", "inf"], ("--ao-radius", "0 or above")),
                         (["--ao", "--ao-strength", "1.5"], ("--ao-strength", "0 .. 1", "'1.5'")),
                         (["--ao", "--ao-strength", "-0.1"], ("--ao-strength", "0 .. 1")),
                         (["--ao", "--ao-strength", "nan"], ("--ao-strength", "0 .. 1")),
                         (["--ao", "--ao-seed", "-3"], ("--ao-seed", "'-3'")),
                         (["--ao", "--ao-seed", "x"], ("--ao-seed", "'x'")),
                         (["--ao", "--exr", "--exr-aov", "id,depth"], ("--exr-aov takes a list of id, position, normal (or all), not 'depth'",))):
        r = _run_driver(tmp_path, *flags)
        assert r.returncode != 0, flags
        for w in words:
            assert w in r.stderr, (flags, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, (flags, r.stderr)       # the refusal and nothing else: no device was asked for
    assert not [p for p in tmp_path.rglob("*") if p.is_file()]
    usage = _run_driver(tmp_path, "-h")
    assert usage.returncode == 0
    for word in ("--ao [1..256]", "--ao-radius R", "--ao-strength 0..1", "--ao-seed X", "--denoise [1..6]"):
        assert word in usage.stderr, word


def test_the_parent_record_is_of_the_recorders_scene():
    """(CPU) the record of the runs without --ao was made with the driver-matrix recorder's scene and base flags."""
    with open(PARENT_RECORD) as f:
        rec = json.load(f)
    assert rec["base"] == recorder.BASE and tuple(rec["documents"]) == recorder.DOCUMENTS
    assert rec["cases"]["png"]["flags"] == PLAIN_PNG and rec["cases"]["exr"]["flags"] == PLAIN_EXR
    assert sorted(p[-4:] for p in rec["cases"]["png"]["files"]) == [".png", ".png"]
    assert sorted(p[-4:] for p in rec["cases"]["exr"]["files"]) == [".exr", ".exr"]
    assert not any("ambient occlusion" in line for c in rec["cases"].values() for line in c["stdout"])


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


W, H = 33, 17                   # partial 8 x 8 tiles on both edges; 5 x 3 tiles, 960 slots a sample
DIM_SCENES = {3: "zoo3d_mirror", 4: "zoo4d", 7: "zoo7d", 12: "zoo12d"}
# one scene for every family of trace kernels the fixtures reach (tests/test_crowd_tiers.py): item sets are the zoo scenes'
TIER_SCENES = {"register_mask": "crowd4d_r", "global_leaf_scan": "crowd7d_gn", "global_hcubes": "crowd4d_g"}
_frames = {}


def frame(gpu, name, K=5, radius=0.0, seed=0, w=W, h=H, **kw):
    """(feature planes with rays, plane, directions) of one call, made once per argument set; uploads the scene"""
    g = golden(name)
    gpu.upload_scene(g.scene)
    key = (name, K, radius, seed, w, h, tuple(sorted(kw.items())))
    if key not in _frames:
        f = gpu.render_features(w, h, g.depth, rays=True, **kw)
        plane, dirs = gpu.render_ao(w, h, g.depth, samples=K, radius=radius, seed=seed, dirs=True, **kw)
        _frames[key] = (f, plane, dirs)
    return _frames[key]


def scene_radius(g):
    """a fifth of the longest side of the scene's box: hits on both sides of it"""
    fs = g.scene
    return 0.2 * float(np.max(np.asarray(fs.vec(fs.bb["upper"])) - np.asarray(fs.vec(fs.bb["lower"]))))


@pytest.mark.gpu
@pytest.mark.parametrize("dims", sorted(DIM_SCENES))
def test_directions_are_unit_vectors_on_the_viewers_side_and_reproducible(gpu, dims):
    name = DIM_SCENES[dims]
    g = golden(name)
    f, plane, dirs = frame(gpu, name, K=8)
    assert dirs.shape == (8, dims, H, W) and plane.shape == (H, W) and gpu.ao_launches() == expected_launches(W, H, 8, 0.0)
    sends, unit = unit_normals(f)
    assert np.array_equal(sends, f["id"] != 0) and sends.any()
    assert np.isfinite(dirs).all()
    norm2 = np.zeros((8, H, W))
    for k in range(dims):
        norm2 = norm2 + dirs[:, k] * dirs[:, k]
    print("%s: %d of %d pixels send rays; max |sum d^2 - 1| = %.3g, min d . n' = %.3g" % (name, int(sends.sum()), sends.size,
          float(np.abs(norm2[:, sends] - 1.0).max()), float(cosines(dirs, unit)[:, sends].min())))
    assert (np.abs(norm2[:, sends] - 1.0) <= 1e-14).all()
    assert (cosines(dirs, unit)[:, sends] >= 0).all()
    assert not dirs[:, :, ~sends].any() and same_bits(dirs[:, :, ~sends], np.zeros_like(dirs[:, :, ~sends]))
    assert same_bits(plane[~sends], np.ones(int((~sends).sum())))
    # two calls: the same bits
    plane2, dirs2 = gpu.render_ao(W, H, g.depth, samples=8, dirs=True)
    assert same_bits(dirs2, dirs) and same_bits(plane2, plane)
    assert same_bits(gpu.render_ao(W, H, g.depth, samples=8), plane)
    # the streams do not depend on K: the 3-sample call's directions are the first three of these
    _, first3 = gpu.render_ao(W, H, g.depth, samples=3, dirs=True)
    assert same_bits(first3, dirs[:3])
    # ... nor on the shard: rows 1, 4, 7 ... are those rows of the full frame
    shard_plane, shard_dirs = gpu.render_ao(W, H, g.depth, samples=8, dirs=True, row_begin=1, row_step=3)
    assert shard_dirs.shape == (8, dims, len(range(1, H, 3)), W)
    assert same_bits(shard_dirs, dirs[:, :, 1::3]) and same_bits(shard_plane, plane[1::3])
    # another seed: other directions, for every pixel that sends any
    _, other = gpu.render_ao(W, H, g.depth, samples=8, seed=12345, dirs=True)
    assert (other[:, :, sends] != dirs[:, :, sends]).any(axis=(0, 1)).all() and not other[:, :, ~sends].any()
    # samples of one pixel differ from each other, and pixels from each other
    assert (dirs[0][:, sends] != dirs[1][:, sends]).any(axis=0).all()
    flat = dirs[0][:, sends]
    assert len({flat[:, i].tobytes() for i in range(flat.shape[1])}) == flat.shape[1]


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [0.0, 6.0], ids=["unlimited", "radius"])
def test_batches_give_the_same_bits_and_the_documented_launches(gpu, radius):
    name = "zoo4d"
    g = golden(name)
    _, plane, dirs = frame(gpu, name, K=8, radius=radius)
    try:
        for batch, launches in ((1, 4 + 8 * (4 if radius else 3)), (3, 4 + 3 * (4 if radius else 3)), (8, 4 + (4 if radius else 3)),
                                (200, 4 + (4 if radius else 3)), (0, 4 + (4 if radius else 3))):
            gpu.set_option("ao_batch", batch)
            got, used = gpu.render_ao(W, H, g.depth, samples=8, radius=radius, dirs=True)
            assert same_bits(got, plane) and same_bits(used, dirs), batch
            assert gpu.ao_launches() == launches == expected_launches(W, H, 8, radius, batch), (batch, gpu.ao_launches())
            assert gpu.ao_ms() > 0.0
        for bad in (-1, 257):
            with pytest.raises(nh.NdtHipError, match="ao_batch"):
                gpu.set_option("ao_batch", bad)
    finally:
        gpu.set_option("ao_batch", 0)


PLANE_CASES = {"%dd" % d: n for d, n in DIM_SCENES.items()}
PLANE_CASES.update(TIER_SCENES)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["unlimited", "radius"])
@pytest.mark.parametrize("case", sorted(PLANE_CASES))
def test_the_plane_is_the_model_on_the_devices_directions(gpu, oracle, case, mode):
    """bit for bit, with every ray's occlusion taken from trace_rays on exactly that ray and the CPU oracle asked the same"""
    name = PLANE_CASES[case]
    g = golden(name)
    radius = scene_radius(g) if mode == "radius" else 0.0
    f, plane, dirs = frame(gpu, name, K=5, radius=radius)
    want, occluded, n_rays = plane_model(gpu, f, dirs, radius, oracle, g.scene)
    differ = int((bits(plane) != bits(want)).sum())
    print("%s (%s, %d-D, %d items, radius %g): %d rays, %d occluded; plane in [%g, %g], %d of %d pixels differ from the model"
          % (case, name, g.scene.dims, g.scene.n_items, radius, n_rays, occluded, plane.min(), plane.max(), differ, plane.size))
    assert differ == 0
    assert ((plane >= 0) & (plane <= 1)).all() and (plane < 1).any() and 0 < occluded <= n_rays
    if mode == "radius":
        assert occluded < n_rays and (plane > 0).any()      # both answers occur (without a radius the 3-D zoo, a closed room, lets no ray out)
        # the radius decides: without it more rays are occluded
        _, everything, _ = plane_model(gpu, f, dirs, 0.0)
        assert everything > occluded


@pytest.mark.gpu
def test_the_plane_of_a_stereo_frame_and_of_a_row_shard(gpu, oracle):
    """side by side: each half's hemispheres face that eye; a shard's plane is the model of the shard's own planes"""
    g = golden("st_zoo4d_sbs")
    f, plane, dirs = frame(gpu, "st_zoo4d_sbs", K=4, w=34, h=17, stereo=1)
    want, occluded, n_rays = plane_model(gpu, f, dirs, 0.0, oracle, g.scene)
    assert same_bits(plane, want) and 0 < occluded < n_rays
    assert (f["ray_o"][:, :, :17] != f["ray_o"][:, :, 17:]).any()
    f, plane, dirs = frame(gpu, "zoo4d", K=4, radius=6.0, row_begin=2, row_step=5)
    assert plane.shape == (3, W)
    want, occluded, n_rays = plane_model(gpu, f, dirs, 6.0, oracle, golden("zoo4d").scene)
    assert same_bits(plane, want) and 0 < occluded < n_rays


@pytest.mark.gpu
@pytest.mark.parametrize("dims", sorted(DIM_SCENES))
def test_known_answers(gpu, tmp_path_factory, dims):
    """A lone hyperplane: exactly 1.0 on every hit pixel (nothing to meet on the viewer's side) and 1.0 where nothing shows.  A camera
    inside one closed sphere of radius R: exactly 0.0 with radius 0 -- every ray meets the wall again, after the chord 2 R c -- and
    exactly 1.0 with a radius below R that no chord undercuts: 2 EPSILON, since a hit within EPSILON of the origin is none
    (object.c) and a sample is occluded under that radius only with EPSILON < 2 R c < 2 EPSILON, a cosine within 1e-5 of 1e-5."""
    w, h, K = 32, 18, 8
    gpu.upload_scene(known_scene(tmp_path_factory, "plane", dims))
    f = gpu.render_features(w, h, 6)
    hit = f["id"] != 0
    assert 0.3 < hit.mean() < 0.9 and hit[-1].all() and not hit[0].any()
    for radius in (0.0, 3.0):
        plane, dirs = gpu.render_ao(w, h, 6, samples=K, radius=radius, dirs=True)
        assert same_bits(plane, np.ones((h, w))) and dirs[:, :, hit].any() and not dirs[:, :, ~hit].any()
    gpu.upload_scene(known_scene(tmp_path_factory, "sphere", dims))
    f = gpu.render_features(w, h, 6, rays=True)
    assert (f["id"] == 1).all()
    plane, dirs = gpu.render_ao(w, h, 6, samples=K, dirs=True)
    sends, unit = unit_normals(f)
    c = cosines(dirs, unit)
    print("%d-D sphere: smallest cosine %.3g (a chord of %.3g)" % (dims, c.min(), 2 * SPHERE_RADIUS * c.min()))
    assert sends.all() and same_bits(plane, np.zeros((h, w)))
    assert same_bits(gpu.render_ao(w, h, 6, samples=K, radius=2e-4), np.ones((h, w)))
    # between the two, the chord decides: a radius of R occludes the rays with c < 1 / 2, up to the rounding of the hit point
    mid = gpu.render_ao(w, h, 6, samples=K, radius=SPHERE_RADIUS)
    clear = np.abs(2.0 * SPHERE_RADIUS * c - SPHERE_RADIUS) > 1e-9
    assert clear.all()
    assert same_bits(mid, fold_model(c.reshape(K, -1), (2.0 * SPHERE_RADIUS * c < SPHERE_RADIUS).reshape(K, -1)).reshape(h, w))
    assert (mid > 0).any() and (mid < 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", sorted(DIM_SCENES))
def test_directions_are_uniform_over_the_hemisphere(gpu, tmp_path_factory, dims):
    """On the lone hyperplane at 32 x 32, K = 16, every n' is the plane's normal e_1, so c = d_1 and the other components are
    tangential.  For d uniform on the unit sphere of N dimensions, E|d_1| = Gamma(N / 2) / (sqrt(pi) Gamma((N + 1) / 2)) = E,
    E d_1^2 = 1 / N, and a tangential component of the folded direction keeps mean 0 and variance 1 / N: the mean of M independent
    samples lies within 6 standard errors, 6 sqrt((1 / N - E^2) / M) and 6 sqrt(1 / (N M)), except once in 5e8 times.  The seeds
    are fixed, so this cannot flake."""
    w = h = 32
    K = 16
    gpu.upload_scene(known_scene(tmp_path_factory, "plane", dims))
    f = gpu.render_features(w, h, 6, rays=True)
    sends, unit = unit_normals(f)
    assert same_bits(unit[:, sends], np.repeat(np.eye(dims)[1][:, None], int(sends.sum()), axis=1))
    E = math.gamma(dims / 2.0) / (math.sqrt(math.pi) * math.gamma((dims + 1) / 2.0))
    for seed in (0, 1, 0xfeedfacecafebeef):
        _, dirs = gpu.render_ao(w, h, 6, samples=K, seed=seed, dirs=True)
        d = dirs[:, :, sends]                        # K x N x pixels
        M = d.shape[0] * d.shape[2]
        assert M >= 16 * 300
        mean_c = float(d[:, 1].mean())
        bound_c = 6.0 * math.sqrt((1.0 / dims - E * E) / M)
        bound_t = 6.0 * math.sqrt(1.0 / (dims * M))
        tangential = [float(d[:, k].mean()) for k in range(dims) if k != 1]
        print("%d-D, seed %#x: M = %d; mean c = %.5f, E = %.5f (bound %.5f); tangential means within %.5f (bound %.5f)"
              % (dims, seed, M, mean_c, E, bound_c, max(abs(t) for t in tangential), bound_t))
        assert abs(mean_c - E) <= bound_c
        assert all(abs(t) <= bound_t for t in tangential)


class DeviceFrame:
    """doubles in device memory (torch) with a pattern behind them that must survive"""
    GUARD = 64

    def __init__(self, values, dtype=np.float64):
        import torch
        self.torch = torch
        values = np.ascontiguousarray(values, dtype=dtype)
        self.n, self.shape, self.dtype = values.size, values.shape, dtype
        guard = np.full(self.GUARD, -7, dtype=dtype)
        self.t = torch.from_numpy(np.concatenate([values.reshape(-1), guard])).cuda()
        torch.cuda.synchronize()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        self.torch.cuda.synchronize()
        back = self.t.cpu().numpy()
        assert (back[self.n:] == -7).all(), "something wrote behind its output"
        return back[:self.n].reshape(self.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [3, 12])
def test_the_pass_alone_from_planes_in_device_memory(gpu, dims):
    """ndt_hip_ao_device on the planes of a feature pass: the plane and the directions of render_ao, nothing written behind either,
    the planes left as they were; a shard by its own parameters"""
    name = DIM_SCENES[dims]
    g = golden(name)
    for kw in ({}, {"row_begin": 1, "row_step": 3}):
        f, plane, dirs = frame(gpu, name, K=5, radius=6.0, **kw)
        dev = {k: DeviceFrame(f[k], np.int32 if k == "id" else np.float64) for k in ("id", "position", "normal", "ray_v")}
        out, used = DeviceFrame(np.full(plane.shape, -3.0)), DeviceFrame(np.full(dirs.shape, -3.0))
        gpu.ao_device({k: v.ptr for k, v in dev.items()}, out.ptr, W, H, g.depth, samples=5, radius=6.0, d_dirs_ptr=used.ptr, **kw)
        assert gpu.ao_launches() == expected_launches(W, plane.shape[0], 5, 6.0, features=False)
        assert same_bits(out.host(), plane) and same_bits(used.host(), dirs)
        assert all(np.array_equal(dev[k].host(), f[k]) for k in dev)
        out = DeviceFrame(np.full(plane.shape, -3.0))
        gpu.ao_device({k: v.ptr for k, v in dev.items()}, out.ptr, W, H, g.depth, samples=5, radius=6.0, **kw)
        assert same_bits(out.host(), plane)


@pytest.mark.gpu
def test_apply_is_the_numpy_expression_and_strength_zero_keeps_the_bits(gpu):
    rng = np.random.default_rng(21)
    for n in (1, 255, 33 * 17):
        rgba = rng.uniform(-1.0, 3.0, (n, 4))
        rgba[0] = [np.inf, -0.0, 1e-310, np.nan]
        plane = rng.uniform(0.0, 1.0, n)
        plane[-1] = 0.0
        for strength in (1.0, 0.3, 0.0):
            src, ao, dst = DeviceFrame(rgba), DeviceFrame(plane), DeviceFrame(np.full((n, 4), -3.0))
            gpu.ao_apply_device(src.ptr, ao.ptr, n, strength, dst.ptr)
            want = apply_model(rgba, plane, strength)
            got = dst.host()
            assert same_bits(got, want) and same_bits(got[:, 3], rgba[:, 3]), (n, strength)
            assert same_bits(src.host(), rgba) and same_bits(ao.host(), plane)
            if strength == 0.0:
                assert same_bits(got[1:], rgba[1:]) and same_bits(got[0, 1:3], rgba[0, 1:3])
            gpu.ao_apply_device(src.ptr, ao.ptr, n, strength)               # in place
            assert same_bits(src.host(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["zoo4d", "al_zoo4d_n2", "zoo12d_radius"])
def test_a_shaded_frame_is_the_plane_applied_to_the_render(gpu, case):
    """render_ao_shaded equals apply(render, render_ao) of the same context bit for bit -- for a sampled frame too, whose plane is its
    deterministic twin's -- and leaves the plane it used"""
    name, samples, radius, strength = {"zoo4d": ("zoo4d", 1, 0.0, 1.0), "al_zoo4d_n2": ("al_zoo4d", 2, 0.0, 0.6),
                                       "zoo12d_radius": ("zoo12d", 1, 6.0, 1.0)}[case]
    g = golden(name)
    gpu.upload_scene(g.scene)
    fb, _ = gpu.render(W, H, g.depth, samples=samples)
    plane = gpu.render_ao(W, H, g.depth, samples=5, radius=radius, seed=9)
    assert same_bits(gpu.render_ao(W, H, g.depth, samples=5, radius=radius, seed=9, frame_samples=samples), plane)
    got, used, st = gpu.render_ao_shaded(W, H, g.depth, samples=5, radius=radius, seed=9, strength=strength, frame_samples=samples)
    assert st.rays_primary > 0
    assert same_bits(used, plane) and same_bits(got, apply_model(fb, plane, strength))
    assert gpu.ao_launches() == expected_launches(W, H, 5, radius, apply=True)
    assert not same_bits(got, fb) and same_bits(got[..., 3], fb[..., 3])
    # left on the device, behind a guard
    if samples == 1:
        out, ao = DeviceFrame(np.full((H, W, 4), -3.0)), DeviceFrame(np.full((H, W), -3.0))
        gpu.render_ao_shaded(W, H, g.depth, sink="device", samples=5, radius=radius, seed=9, strength=strength, d_rgba_ptr=out.ptr, d_ao_ptr=ao.ptr)
        assert same_bits(out.host(), got) and same_bits(ao.host(), plane)
        gpu.render_ao_shaded(W, H, g.depth, sink="device", samples=5, radius=radius, seed=9, strength=strength, d_rgba_ptr=out.ptr)
        assert same_bits(out.host(), got)


@pytest.mark.gpu
def test_the_sinks_take_the_models_image(gpu, oracle):
    """rgba8 is oracle.quantize of apply(render, plane); the PNG decodes to exactly that; the JPEG is ndt_hip_encode_jpeg of those
    pixels, byte for byte"""
    g = golden("zoo4d")
    gpu.upload_scene(g.scene)
    fb, _ = gpu.render(W, H, g.depth)
    kw = dict(samples=5, seed=3, strength=0.8)
    plane = gpu.render_ao(W, H, g.depth, samples=5, seed=3)
    want8 = oracle.quantize(apply_model(fb, plane, 0.8))
    assert not np.array_equal(want8, oracle.quantize(fb))
    got8, _ = gpu.render_ao_shaded(W, H, g.depth, sink="rgba8", **kw)
    assert np.array_equal(got8, want8)
    png, _ = gpu.render_ao_shaded(W, H, g.depth, sink="png", **kw)
    assert np.array_equal(read_png(png), want8) and gpu.png_stats.png_bytes == len(png)
    assert png == gpu.encode_png(want8)
    for quality, sampling in ((95, "420"), (50, "444")):
        jpg, _ = gpu.render_ao_shaded(W, H, g.depth, sink="jpeg", quality=quality, sampling=sampling, **kw)
        assert jpg == gpu.encode_jpeg(want8, quality, sampling)


@pytest.mark.gpu
@pytest.mark.parametrize("pixel", ["half", "float"])
@pytest.mark.parametrize("dims", [3, 4, 12])
def test_the_exr_file_has_the_channel_ao_in_its_place(gpu, dims, pixel):
    """the strict reader accepts the file; its channel list is A AO B G N.* P.* R Z id; AO is float32 of the plane; the colour is the
    render's times the factor; at strength 0 colour, Z and the feature channels carry the bits of the file without AO"""
    name = DIM_SCENES[dims]
    g = golden(name)
    gpu.upload_scene(g.scene)
    fb, dm, _ = gpu.render(W, H, g.depth, depth_map=True)
    f = gpu.render_features(W, H, g.depth)
    plane = gpu.render_ao(W, H, g.depth, samples=4, seed=5)
    without, _ = gpu.render_exr(W, H, g.depth, pixel=pixel, depth_map=True, features=ALL)
    plain = xf.read_exr(without)[1]
    for strength in (0.0, 0.7):
        data, _ = gpu.render_exr(W, H, g.depth, pixel=pixel, depth_map=True, features=ALL, ao=dict(samples=4, seed=5, strength=strength))
        st = gpu.exr_stats
        want = ao_channels(apply_model(fb, plane, strength), dm, f, 7, xf.PIXEL[pixel], plane)
        assert [n for n, _, _ in want][:4] == ["A", "AO", "B", "G"] and [n for n, _, _ in want][-3:] == ["R", "Z", "id"]
        sizes, raw = xf.assert_file_is(data, want)
        assert st.file_bytes == len(data) <= nh.exr_ao_bound(W, H, dims, ALL, pixel, True) and st.launches == 4
        assert st.raw_bytes == W * H * (4 * xf.DTYPE[xf.PIXEL[pixel]].itemsize + 4 + 4 + 4 + 8 * dims)
        assert gpu.ao_launches() == expected_launches(W, H, 4, 0.0, apply=strength != 0)
        got = xf.read_exr(data)[1]
        assert xf.same_bits(got["AO"], plane.astype(np.float32))
        same = all(xf.same_bits(got[n], plain[n]) for n in plain)
        assert sorted(got) == sorted(list(plain) + ["AO"]) and same == (strength == 0.0)
        assert all(xf.same_bits(got[n], plain[n]) for n in plain if n not in "RGB")
    # no feature group, no map: A AO B G R; and a subset
    data, _ = gpu.render_exr(W, H, g.depth, pixel=pixel, ao=dict(samples=4, seed=5))
    xf.assert_file_is(data, ao_channels(apply_model(fb, plane, 1.0), None, {}, 0, xf.PIXEL[pixel], plane))
    assert [n for n, _ in xf.read_exr(data)[0]] == ["A", "AO", "B", "G", "R"]
    data, _ = gpu.render_exr(W, H, g.depth, pixel=pixel, depth_map=True, features=("id",), ao=dict(samples=4, seed=5, radius=6.0))
    near = gpu.render_ao(W, H, g.depth, samples=4, seed=5, radius=6.0)
    xf.assert_file_is(data, ao_channels(apply_model(fb, near, 1.0), dm, f, xf.ID, xf.PIXEL[pixel], near))
    # caller-supplied planes through ndt_hip_encode_exr_ao_device
    dev = {k: DeviceFrame(f[k], np.int32 if k == "id" else np.float64) for k in ALL}
    d_fb, d_dm, d_ao = DeviceFrame(fb), DeviceFrame(dm), DeviceFrame(plane)
    ep = nh.exr_params(pixel)
    cap = nh.exr_ao_bound(W, H, dims, ALL, pixel, True)
    out = np.zeros(cap, dtype=np.uint8)
    st = nh.ExrStats()
    planes = nh.FeaturePlanes(dev["id"].ptr, dev["position"].ptr, dev["normal"].ptr, None, None)
    gpu._check(gpu.lib.ndt_hip_encode_exr_ao_device(gpu.ctx, C.c_void_p(d_fb.ptr), C.c_void_p(d_dm.ptr), C.byref(planes), C.c_void_p(d_ao.ptr),
                                                    dims, 7, W, H, C.byref(ep), out.ctypes.data, cap, C.byref(st)))
    xf.assert_file_is(out[:st.file_bytes].tobytes(), ao_channels(fb, dm, f, 7, xf.PIXEL[pixel], plane))


@pytest.mark.gpu
def test_an_ao_call_changes_no_later_render_map_feature_pass_or_denoised_frame(gpu):
    g = golden("al_zoo4d")
    gpu.upload_scene(g.scene)
    fb, dm, _ = gpu.render(W, H, g.depth, depth_map=True)
    sampled, _ = gpu.render(W, H, g.depth, samples=2)
    f = gpu.render_features(W, H, g.depth, rays=True)
    denoised, _ = gpu.render_denoised(W, H, g.depth, samples=2, iterations=2)
    exr, _ = gpu.render_exr(W, H, g.depth, pixel="float", depth_map=True, features=ALL)
    try:
        gpu.set_option("ao_batch", 3)
        gpu.render_ao(W, H, g.depth, samples=8, radius=4.0, dirs=True)
        gpu.set_option("ao_batch", 0)
        gpu.render_ao(67, 37, g.depth, samples=8)                           # a larger frame: the workspace grows
        gpu.render_ao_shaded(W, H, g.depth, sink="png", samples=3)
        gpu.render_exr(W, H, g.depth, features=ALL, depth_map=True, ao=True)
    finally:
        gpu.set_option("ao_batch", 0)
    fb2, dm2, _ = gpu.render(W, H, g.depth, depth_map=True)
    assert same_bits(fb2, fb) and same_bits(dm2, dm)
    assert same_bits(gpu.render(W, H, g.depth, samples=2)[0], sampled)
    f2 = gpu.render_features(W, H, g.depth, rays=True)
    assert np.array_equal(f2["id"], f["id"]) and all(same_bits(f2[k], f[k]) for k in ("position", "normal", "ray_o", "ray_v"))
    assert same_bits(gpu.render_denoised(W, H, g.depth, samples=2, iterations=2)[0], denoised)
    assert gpu.render_exr(W, H, g.depth, pixel="float", depth_map=True, features=ALL)[0] == exr


@pytest.mark.gpu
def test_the_library_refuses_by_code_and_cause_and_writes_nothing(gpu):
    lib = gpu.lib
    g = golden("st_zoo4d_sbs")
    gpu.upload_scene(g.scene)
    w, h = 34, 18
    ok = nh.ao_params(4)
    size = w * h * 8 * 4 * g.scene.dims

    def host_entries(p, ap, buf):
        yield "ndt_hip_render_ao", lib.ndt_hip_render_ao(gpu.ctx, C.byref(p), C.byref(ap), buf.ctypes.data, None, None)
        yield "ndt_hip_render_ao_shaded", lib.ndt_hip_render_ao_shaded(gpu.ctx, C.byref(p), C.byref(ap), buf.ctypes.data, None, None)
        yield "ndt_hip_render_ao_shaded_rgba8", lib.ndt_hip_render_ao_shaded_rgba8(gpu.ctx, C.byref(p), C.byref(ap), buf.ctypes.data, None)
        yield "ndt_hip_render_ao_shaded_png", lib.ndt_hip_render_ao_shaded_png(gpu.ctx, C.byref(p), C.byref(ap), buf.ctypes.data, buf.size, None, None)
        yield "ndt_hip_render_ao_shaded_jpeg", lib.ndt_hip_render_ao_shaded_jpeg(gpu.ctx, C.byref(p), C.byref(ap), None, buf.ctypes.data, buf.size, None, None)
        yield "ndt_hip_render_exr_ao", lib.ndt_hip_render_exr_ao(gpu.ctx, C.byref(p), None, 1, 7, C.byref(ap), buf.ctypes.data, buf.size, None, None)

    frames = [({"aa": (20, 3)}, ok, NDT_E_UNSUPPORTED, "recursive_aa"), ({"stereo": 3}, ok, NDT_E_UNSUPPORTED, "NDT_STEREO_ANAGLYPH"),
              ({"stereo": 4}, ok, NDT_E_UNSUPPORTED, "NDT_STEREO_HIDEF")]
    frames += [({}, nh.AoParams(k, 0, 0.0, 0, 1.0), NDT_E_INVALID, "%d samples" % k) for k in (0, -1, 257)]
    frames += [({}, nh.AoParams(4, 0, r, 0, 1.0), NDT_E_INVALID, "radius") for r in (-1.0, math.nan, math.inf)]
    frames += [({}, nh.AoParams(4, 0, 0.0, 0, s), NDT_E_INVALID, "strength") for s in (-0.1, 1.5, math.nan)]
    frames += [({}, nh.AoParams(4, 1, 0.0, 0, 1.0), NDT_E_INVALID, "reserved"), ({"row_begin": h}, ok, NDT_E_INVALID, "no rows")]
    for kw, ap, code, word in frames:
        p = gpu.params(w, h, g.depth, samples=2, **kw)
        buf = np.full(size, 0xA5, dtype=np.uint8)
        for name, rc in host_entries(p, ap, buf):
            assert rc == code, (name, kw, word)
            err = lib.ndt_hip_last_error().decode()
            assert word in err and name in err, (name, err)
            assert (buf == 0xA5).all()
    # the entries on device memory: the same, and NULL or misaligned pointers; the pass alone takes one frame's planes, no samples > 1
    f = gpu.render_features(w, h, g.depth, rays=True, stereo=1)
    dev = {k: DeviceFrame(f[k], np.int32 if k == "id" else np.float64) for k in ("id", "position", "normal", "ray_v")}
    out, img = DeviceFrame(np.full((h, w), -3.0)), DeviceFrame(np.full((h, w, 4), -3.0))

    def alone(ap=ok, dst=None, dirs=None, **kw):
        pl = {k: v.ptr for k, v in dev.items()}
        pl.update({k: kw.pop(k) for k in list(kw) if k in pl})
        p = gpu.params(w, h, g.depth, **dict({"stereo": 1}, **kw))
        fp = nh.FeaturePlanes(pl["id"], pl["position"], pl["normal"], None, pl["ray_v"])
        return lib.ndt_hip_ao_device(gpu.ctx, C.byref(p), C.byref(fp), C.byref(ap), C.c_void_p(out.ptr if dst is None else dst), C.c_void_p(dirs) if dirs else None)

    for call, code, word in ((lambda: alone(nh.AoParams(0, 0, 0.0, 0, 1.0)), NDT_E_INVALID, "0 samples"), (lambda: alone(nh.AoParams(4, 0, -2.0, 0, 1.0)), NDT_E_INVALID, "radius"),
                             (lambda: alone(id=None), NDT_E_INVALID, "NULL plane"), (lambda: alone(position=None), NDT_E_INVALID, "NULL plane"),
                             (lambda: alone(normal=None), NDT_E_INVALID, "NULL plane"), (lambda: alone(ray_v=None), NDT_E_INVALID, "NULL plane"),
                             (lambda: alone(id=dev["id"].ptr + 2), NDT_E_INVALID, "misaligned"), (lambda: alone(normal=dev["normal"].ptr + 4), NDT_E_INVALID, "misaligned"),
                             (lambda: alone(dst=out.ptr + 4), NDT_E_INVALID, "misaligned"), (lambda: alone(dirs=out.ptr + 4), NDT_E_INVALID, "misaligned"),
                             (lambda: alone(samples=2), NDT_E_UNSUPPORTED, "samples = 2"), (lambda: alone(stereo=3), NDT_E_UNSUPPORTED, "NDT_STEREO_ANAGLYPH"),
                             (lambda: alone(aa=(20, 3)), NDT_E_UNSUPPORTED, "recursive_aa")):
        assert call() == code, word
        err = lib.ndt_hip_last_error().decode()
        assert word in err and "ndt_hip_ao_device" in err, err
    p = gpu.params(w, h, g.depth, stereo=1)
    assert lib.ndt_hip_render_ao_device(gpu.ctx, C.byref(p), C.byref(ok), None, None, None) == NDT_E_INVALID
    assert lib.ndt_hip_render_ao_device(gpu.ctx, C.byref(p), C.byref(ok), C.c_void_p(out.ptr + 4), None, None) == NDT_E_INVALID
    assert lib.ndt_hip_render_ao_shaded_device(gpu.ctx, C.byref(p), C.byref(ok), C.c_void_p(img.ptr + 8), None, None) == NDT_E_INVALID
    assert b"misaligned" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_render_ao_shaded_device(gpu.ctx, C.byref(gpu.params(w, h, g.depth, stereo=4)), C.byref(ok), C.c_void_p(img.ptr), None, None) == NDT_E_UNSUPPORTED
    for call, word in ((lambda: lib.ndt_hip_ao_apply_device(gpu.ctx, None, C.c_void_p(out.ptr), w * h, 1.0, C.c_void_p(img.ptr)), "NULL"),
                       (lambda: lib.ndt_hip_ao_apply_device(gpu.ctx, C.c_void_p(img.ptr), C.c_void_p(out.ptr), w * h, 1.5, C.c_void_p(img.ptr)), "strength"),
                       (lambda: lib.ndt_hip_ao_apply_device(gpu.ctx, C.c_void_p(img.ptr), C.c_void_p(out.ptr), w * h, math.nan, C.c_void_p(img.ptr)), "strength"),
                       (lambda: lib.ndt_hip_ao_apply_device(gpu.ctx, C.c_void_p(img.ptr), C.c_void_p(out.ptr), -1, 1.0, C.c_void_p(img.ptr)), "-1 pixels"),
                       (lambda: lib.ndt_hip_ao_apply_device(gpu.ctx, C.c_void_p(img.ptr + 8), C.c_void_p(out.ptr), w * h, 1.0, C.c_void_p(img.ptr)), "misaligned"),
                       (lambda: lib.ndt_hip_ao_apply_device(gpu.ctx, C.c_void_p(img.ptr), C.c_void_p(out.ptr + 4), w * h, 1.0, C.c_void_p(img.ptr)), "misaligned")):
        assert call() == NDT_E_INVALID, word
        assert word in lib.ndt_hip_last_error().decode() and b"ndt_hip_ao_apply_device" in lib.ndt_hip_last_error()
    assert same_bits(out.host(), np.full((h, w), -3.0)) and same_bits(img.host(), np.full((h, w, 4), -3.0))
    assert all(np.array_equal(dev[k].host(), f[k]) for k in dev)
    # a feature mask the AO file does not know, and a pixel type
    buf = np.full(size, 0xA5, dtype=np.uint8)
    assert lib.ndt_hip_render_exr_ao(gpu.ctx, C.byref(p), None, 1, 8, C.byref(ok), buf.ctypes.data, buf.size, None, None) == NDT_E_INVALID
    assert b"feature mask 8" in lib.ndt_hip_last_error()
    assert lib.ndt_hip_render_exr_ao(gpu.ctx, C.byref(p), C.byref(nh.ExrParams(3)), 1, 7, C.byref(ok), buf.ctypes.data, buf.size, None, None) == NDT_E_INVALID
    assert (buf == 0xA5).all()
    # ... which the feature entries keep refusing
    assert lib.ndt_hip_render_exr_features(gpu.ctx, C.byref(p), None, 1, 8, buf.ctypes.data, buf.size, None, None) == NDT_E_INVALID
    # side by side and over / under work, and so does a NULL parameter block: the defaults
    plane = np.zeros((h, w))
    assert lib.ndt_hip_render_ao(gpu.ctx, C.byref(gpu.params(w, h, g.depth, stereo=2)), None, plane.ctypes.data, None, None) == 0
    assert gpu.ao_launches() == expected_launches(w, h, 16, 0.0) and ((plane >= 0) & (plane <= 1)).all()
    # without a scene: NDT_E_STATE
    fresh = nh.NdtHip(0)
    try:
        buf = np.full(size, 0xA5, dtype=np.uint8)
        pp = gpu.params(w, h, g.depth)
        assert lib.ndt_hip_render_ao(fresh.ctx, C.byref(pp), C.byref(ok), plane.ctypes.data, None, None) == NDT_E_STATE
        assert b"no scene" in lib.ndt_hip_last_error()
        assert lib.ndt_hip_render_ao_shaded(fresh.ctx, C.byref(pp), C.byref(ok), buf.ctypes.data, None, None) == NDT_E_STATE
        assert lib.ndt_hip_render_exr_ao(fresh.ctx, C.byref(pp), None, 0, 0, C.byref(ok), buf.ctypes.data, buf.size, None, None) == NDT_E_STATE
    finally:
        fresh.close()


# ---------------------------------------------------------------- driver

def _library_files(tmp_path, make):
    """what `make(gpu)` returns for the scenes of frames 0 and 1 of the recorder's file, as the driver loads them"""
    out = []
    gpu = nh.NdtHip(0)
    try:
        for k in (0, 1):
            dump = str(tmp_path / ("frame%d.ndtscene" % k))
            r = subprocess.run([DRIVER] + recorder.BASE[:-2] + ["-f", "%d:%d" % (k, k), "-u", str(tmp_path / recorder.SCENE), "--dump-scene", dump],
                               capture_output=True, text=True, cwd=str(tmp_path))
            assert r.returncode == 0, r.stderr[-2000:]
            gpu.upload_scene(load_scene(dump))
            out.append(make(gpu))
    finally:
        gpu.close()
    return out


@pytest.mark.gpu
def test_driver_shades_says_so_and_leaves_the_librarys_files(tmp_path):
    """`ndt_hip --ao 4 --png --deflate gpu` and `ndt_hip --exr --ao 4 --ao-strength 0 --exr-aov all -z` over both frames of the driver
    matrix's scene at 16 x 9: the line of each frame, and the files the library makes for the same requests.  The same runs without
    --ao say nothing of it and leave the bytes they left before there was one (tests/golden/ao_driver_parent.json)."""
    recorder.write_scene(str(tmp_path / recorder.SCENE))
    with open(PARENT_RECORD) as f:
        rec = json.load(f)
    for case, plain_flags, ao_flags, launches, make in (
            ("png", PLAIN_PNG, ["--ao", "4"] + PLAIN_PNG, 8, lambda gpu: gpu.render_ao_shaded(16, 9, 6, sink="png", samples=4)[0]),
            ("exr", PLAIN_EXR, ["--exr", "--ao", "4", "--ao-strength", "0", "--exr-aov", "all", "-z"], 7,
             lambda gpu: gpu.render_exr(16, 9, 6, depth_map=True, features=ALL, ao=dict(samples=4, strength=0.0))[0])):
        plain = recorder.run_case(DRIVER, str(tmp_path / (case + "_plain")), plain_flags)
        assert plain["files"] == rec["cases"][case]["files"] and plain["stdout"] == rec["cases"][case]["stdout"], case
        got = recorder.run_case(DRIVER, str(tmp_path / (case + "_ao")), ao_flags)
        assert got["stdout"].count("ambient occlusion of 4 samples on GPU 0 in %d launches" % launches) == 2, got["stdout"]
        assert sorted(got["files"]) == sorted(plain["files"])
        assert all(got["files"][p]["sha256"] != plain["files"][p]["sha256"] for p in plain["files"])
        # without the new line the run says what the plain one says
        assert [s for s in got["stdout"] if "ambient occlusion" not in s and not s.startswith(("compressed PNG", "encoded EXR"))] == \
               [s for s in plain["stdout"] if not s.startswith(("compressed PNG", "encoded EXR"))]
        files = [next(p for p in got["files"] if re.search(r"_%04d\.(png|exr)$" % k, p)) for k in (0, 1)]
        for k, want in enumerate(_library_files(tmp_path, make)):
            with open(os.path.join(str(tmp_path / (case + "_ao")), files[k]), "rb") as f:
                data = f.read()
            assert data == want, files[k]
            if case == "exr":
                chans, samples, _, _ = xf.read_exr(data)
                assert [n for n, _ in chans][:3] == ["A", "AO", "B"] and chans[-1][0] == "id" and len(chans) == 7 + 2 * 4
                with open(os.path.join(str(tmp_path / (case + "_plain")), files[k]), "rb") as f:
                    before = xf.read_exr(f.read())[1]
                assert all(xf.same_bits(samples[n], before[n]) for n in before)
                assert ((samples["AO"] >= 0) & (samples["AO"] <= 1)).all()
    # the other sinks and the parameters reach the library too: two frames each, each with its line
    for case, (k, launches, flags) in enumerate(((16, 8, ["--ao"]), (2, 8, ["--ao", "2", "--png"]), (5, 9, ["--ao=5", "--jpeg", "--ao-radius", "3"]),
                                                 (3, 8, ["--ao", "3", "--raw", "f.f64", "--ao-strength", "0.5", "--ao-seed", "0x10"]),
                                                 (4, 8, ["--ao", "4", "-n", "2", "-m", "s", "-j", "2", "--fit", "gpu", "--kd", "gpu"]),
                                                 (4, 8, ["--ao", "4", "--exr", "--exr-pixel", "float"]))):
        one = recorder.run_case(DRIVER, str(tmp_path / ("case%d" % case)), flags)
        assert one["stdout"].count("ambient occlusion of %d samples on GPU 0 in %d launches" % (k, launches)) == 2, (flags, one["stdout"])
        assert len(one["files"]) >= 2
