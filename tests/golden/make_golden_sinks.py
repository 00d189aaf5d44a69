"""Records what every delivering entry of libndt_hip.so hands back -- tests/golden/sink_matrix_parent.json, which
tests/test_sink_matrix.py compares a build against.  The record was made ONCE, on the build before the delivery half of the C ABI
was folded into one set of tails (ndt_render.hip); run this file on an MI355X only to extend the matrix on a build known good:

    python tests/golden/make_golden_sinks.py          # two passes, which must agree; writes the record

Scene: the golden c3_random4d at its golden depth.  Frames: 24 x 10 (no multiple of the 8 x 8 tile, less than one 32 KiB deflate
chunk) and its cyclic shard row_begin = 1, row_step = 3.  Per case: sha256 and length of every array or file returned, the four
ray counts, the stages' launch counters.  Per entry, the refusals: (return code, ndt_hip_last_error()) and whether the output
buffer, filled with a pattern before the call, is untouched.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

RECORD = os.path.join(HERE, "sink_matrix_parent.json")
SCENE = "c3_random4d"
W, H = 24, 10
SHARD = {"row_begin": 1, "row_step": 3}
BIG = (65536, 8192)         # a side above 65535; 8-bit PNG, 16-bit PNG and EXR streams beyond 2^31 - 1 bytes
SEED = 20261                # option "sample_seed" of the denoiser's context
PATTERN = 0xA5
ALL = ("id", "position", "normal")
AO = {"samples": 4, "seed": 3}
COUNTERS = ("ssaa_launches", "depth_launches", "denoise_launches", "ao_launches", "features_launches")
# bound cases left out, and why
NO_BOUND = {"apng_frame_k1, apng_frame_k2": "the frame must have the session's size, and ndt_hip_apng_begin refuses a session of the bound case's size"}


def _scene():
    from ndt_amd import load_scene
    with open(os.path.join(HERE, SCENE + ".json")) as f:
        meta = json.load(f)
    return load_scene(os.path.join(HERE, meta["scene_file"])), meta["depth"]


class Entry:
    """One delivering entry.  good(gpu, depth, geom): the call through its NdtHip method.  raw(gpu, x, p, out, cap, K): the C call
    with `out` as its first output and x's scratch for the rest.  kind: "host" (arrays), "file", "device".  K: its supersampling
    factor, or None.  samples, ao: the frame's samples and the AO parameters of the good call, which the raw calls repeat."""

    def __init__(self, name, stage, kind, good, raw, K=None, samples=1, ao=None):
        self.name, self.stage, self.kind, self.good, self.raw, self.K, self.samples, self.ao = name, stage, kind, good, raw, K, samples, ao or AO


class Scratch:
    """What a raw call needs beside its first output: records, parameters, and room for a second output"""

    def __init__(self):
        from ndt_amd import RenderStats
        from ndt_amd import hip
        self.st = RenderStats()
        self.pst = (hip.PngStats * 2)()
        self.jst, self.est, self.ast = hip.JpegStats(), hip.ExrStats(), hip.ApngStats()
        self.rng = np.zeros(2)
        self.side = np.zeros(1 << 16, dtype=np.uint8)
        self.jp, self.ep = hip.jpeg_params(), hip.exr_params("half")
        self.dp, self.ap = hip.denoise_params(), hip.ao_params(**AO)
        self.mask = hip.feature_mask(ALL)


def _m(method, **kw):
    return lambda gpu, depth, geom: getattr(gpu, method)(W, H, depth, **dict(kw, **geom))


def _device(method, planes, **kw):
    """a "device" sink: into torch buffers, which come back as arrays"""
    def call(gpu, depth, geom):
        import torch
        from ndt_amd.flat_scene import shard_rows
        rows = shard_rows(H, geom.get("row_begin", 0), geom.get("row_step", 1))
        bufs = [torch.zeros((rows, W, 4), dtype=torch.float64, device="cuda")]
        ptrs = {"d_rgba_ptr": bufs[0].data_ptr()}
        if planes:
            bufs.append(torch.zeros((rows, W), dtype=torch.float64, device="cuda"))
            ptrs["d_ao_ptr"] = bufs[1].data_ptr()
        torch.cuda.synchronize()
        st = getattr(gpu, method)(W, H, depth, sink="device", **dict(kw, **ptrs, **geom))
        gpu.synchronize()
        return tuple(b.cpu().numpy() for b in bufs) + (st,)
    return call


def _apng(ssaa):
    def call(gpu, depth, geom):
        from ndt_amd.flat_scene import shard_rows
        gpu.apng_begin(W, shard_rows(H, geom.get("row_begin", 0), geom.get("row_step", 1)), 1)
        return gpu.render_apng_frame(W, H, depth, ssaa=ssaa, **geom)
    return call


def entries():
    r = C.byref
    side = lambda x: x.side.ctypes.data
    E = []
    add = lambda *a, **kw: E.append(Entry(*a, **kw))
    # the plain frame
    add("render", "plain", "host", _m("render"), lambda g, x, p, o, cap, K: g.lib.ndt_hip_render(g.ctx, p, o, r(x.st)))
    add("render_depth", "plain", "host", _m("render", depth_map=True),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_depth(g.ctx, p, o, side(x), r(x.st)))
    add("render_rgba8", "plain", "host", _m("render_rgba8"), lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_rgba8(g.ctx, p, o, r(x.st)))
    add("render_rgba8_depth", "plain", "host", _m("render_rgba8_depth"),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_rgba8_depth(g.ctx, p, o, side(x), x.rng.ctypes.data, r(x.st)))
    add("render_png", "plain", "file", _m("render_png"), lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_png(g.ctx, p, o, cap, r(x.pst), r(x.st)))
    add("render_png_depth", "plain", "file", _m("render_png_depth"),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_png_depth(g.ctx, p, o, cap, side(x), x.side.size, None, r(x.pst), x.rng.ctypes.data, r(x.st)))
    add("render_png_depth8", "plain", "file", _m("render_png_depth", depth_png=False),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_png_depth(g.ctx, p, o, cap, None, 0, side(x), r(x.pst), x.rng.ctypes.data, r(x.st)))
    add("render_png16", "plain", "file", _m("render_png16"), lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_png16(g.ctx, p, o, cap, r(x.pst), r(x.st)))
    add("render_png16_depth", "plain", "file", _m("render_png16_depth"),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_png16_depth(g.ctx, p, o, cap, side(x), x.side.size, r(x.pst), x.rng.ctypes.data, r(x.st)))
    add("render_jpeg", "plain", "file", _m("render_jpeg"),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_jpeg(g.ctx, p, r(x.jp), o, cap, r(x.jst), r(x.st)))
    # OpenEXR
    for pixel in ("half", "float"):
        for dm in (False, True):
            def raw(g, x, p, o, cap, K, pixel=pixel, dm=dm):
                from ndt_amd import hip
                ep = hip.exr_params(pixel)
                return g.lib.ndt_hip_render_exr(g.ctx, p, r(ep), int(dm), o, cap, r(x.est), r(x.st))
            add("render_exr_%s%s" % (pixel, "_depth" if dm else ""), "exr", "file", _m("render_exr", pixel=pixel, depth_map=dm), raw)
    add("render_exr_features", "exr", "file", _m("render_exr", depth_map=True, features=ALL),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_exr_features(g.ctx, p, r(x.ep), 1, x.mask, o, cap, r(x.est), r(x.st)))
    add("render_exr_ao", "exr", "file", _m("render_exr", depth_map=True, features=ALL, ao=AO),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_exr_ao(g.ctx, p, r(x.ep), 1, x.mask, r(x.ap), o, cap, r(x.est), r(x.st)))
    add("render_exr_ao_strength0", "exr", "file", _m("render_exr", ao=dict(AO, strength=0.0)),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_exr_ao(g.ctx, p, r(x.ep), 0, 0, r(x.ap), o, cap, r(x.est), r(x.st)),
        ao=dict(AO, strength=0.0))
    # supersampled
    add("render_ssaa", "ssaa", "host", _m("render_ssaa", ssaa=2), lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ssaa(g.ctx, p, K, o, None, r(x.st)), K=2)
    add("render_ssaa_depth", "ssaa", "host", _m("render_ssaa", ssaa=2, depth_map=True),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ssaa(g.ctx, p, K, o, side(x), r(x.st)), K=2)
    for K in (2, 1):
        add("render_ssaa_rgba8_k%d" % K, "ssaa", "host", _m("render_ssaa_rgba8", ssaa=K),
            lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ssaa_rgba8(g.ctx, p, K, o, r(x.st)), K=K)
        add("render_ssaa_png_k%d" % K, "ssaa", "file", _m("render_ssaa_png", ssaa=K),
            lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ssaa_png(g.ctx, p, K, o, cap, r(x.pst), r(x.st)), K=K)
    add("render_ssaa_jpeg", "ssaa", "file", _m("render_ssaa_jpeg", ssaa=2),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ssaa_jpeg(g.ctx, p, K, r(x.jp), o, cap, r(x.jst), r(x.st)), K=2)
    add("render_ssaa_rgba8_depth", "ssaa", "host", _m("render_ssaa_rgba8_depth", ssaa=2),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ssaa_rgba8_depth(g.ctx, p, K, o, side(x), x.rng.ctypes.data, r(x.st)), K=2)
    add("render_ssaa_png16", "ssaa", "file", _m("render_ssaa_png16", ssaa=2),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ssaa_png16(g.ctx, p, K, o, cap, r(x.pst), r(x.st)), K=2)
    add("render_ssaa_png16_depth", "ssaa", "file", _m("render_ssaa_png16", ssaa=2, depth_map=True),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ssaa_png16_depth(g.ctx, p, K, o, cap, side(x), x.side.size, r(x.pst), x.rng.ctypes.data, r(x.st)), K=2)
    add("render_ssaa_exr", "ssaa", "file", _m("render_ssaa_exr", ssaa=2, depth_map=True),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ssaa_exr(g.ctx, p, K, r(x.ep), 1, o, cap, r(x.est), r(x.st)), K=2)
    add("render_ssaa_exr_features", "ssaa", "file", _m("render_ssaa_exr", ssaa=2, features=ALL),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ssaa_exr_features(g.ctx, p, K, r(x.ep), 0, x.mask, o, cap, r(x.est), r(x.st)), K=2)
    # animated PNG: a session of one frame a case.  K = 1 is the frame without supersampling (the driver's `--apng` alone): the entry
    # refuses ssaa 0, which is recorded among its refusals (k0)
    for K in (1, 2):
        add("apng_frame_k%d" % K, "apng", "file", _apng(K),
            lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_apng_frame(g.ctx, p, K, o, cap, r(x.ast), r(x.st)), K=K)
    # denoised (the shard is one of its refusals), at one sample a pixel and at four
    for n in (1, 4):
        tag = "" if n == 1 else "_n4"
        add("render_denoised" + tag, "denoise", "host", _m("render_denoised", samples=n),
            lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_denoised(g.ctx, p, r(x.dp), o, r(x.st)), samples=n)
        add("render_denoised_device" + tag, "denoise", "device", _device("render_denoised", False, samples=n),
            lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_denoised_device(g.ctx, p, r(x.dp), o, r(x.st)), samples=n)
        add("render_denoised_rgba8" + tag, "denoise", "host", _m("render_denoised", sink="rgba8", samples=n),
            lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_denoised_rgba8(g.ctx, p, r(x.dp), o, r(x.st)), samples=n)
        add("render_denoised_png" + tag, "denoise", "file", _m("render_denoised", sink="png", samples=n),
            lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_denoised_png(g.ctx, p, r(x.dp), o, cap, r(x.pst), r(x.st)), samples=n)
        add("render_denoised_jpeg" + tag, "denoise", "file", _m("render_denoised", sink="jpeg", samples=n),
            lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_denoised_jpeg(g.ctx, p, r(x.dp), r(x.jp), o, cap, r(x.jst), r(x.st)), samples=n)
        add("render_denoised_exr" + tag, "denoise", "file", _m("render_denoised", sink="exr", samples=n),
            lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_denoised_exr(g.ctx, p, r(x.dp), r(x.ep), o, cap, r(x.est), r(x.st)), samples=n)
    # ambient occlusion
    add("render_ao_shaded", "ao", "host", _m("render_ao_shaded", **AO),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ao_shaded(g.ctx, p, r(x.ap), o, side(x), r(x.st)))
    add("render_ao_shaded_device", "ao", "device", _device("render_ao_shaded", True, **AO),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ao_shaded_device(g.ctx, p, r(x.ap), o, None, r(x.st)))
    add("render_ao_shaded_rgba8", "ao", "host", _m("render_ao_shaded", sink="rgba8", **AO),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ao_shaded_rgba8(g.ctx, p, r(x.ap), o, r(x.st)))
    add("render_ao_shaded_png", "ao", "file", _m("render_ao_shaded", sink="png", **AO),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ao_shaded_png(g.ctx, p, r(x.ap), o, cap, r(x.pst), r(x.st)))
    add("render_ao_shaded_jpeg", "ao", "file", _m("render_ao_shaded", sink="jpeg", **AO),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ao_shaded_jpeg(g.ctx, p, r(x.ap), r(x.jp), o, cap, r(x.jst), r(x.st)))
    add("render_ao", "ao", "host", _m("render_ao", dirs=True, **AO),
        lambda g, x, p, o, cap, K: g.lib.ndt_hip_render_ao(g.ctx, p, r(x.ap), o, None, r(x.st)))
    return E


ENTRIES = entries()


def described(x):
    """What of an answer is recorded"""
    if isinstance(x, np.ndarray):
        return {"dtype": str(x.dtype), "shape": list(x.shape), "bytes": int(x.nbytes), "sha256": hashlib.sha256(x.tobytes()).hexdigest()}
    if isinstance(x, bytes):
        return {"bytes": len(x), "sha256": hashlib.sha256(x).hexdigest()}
    if hasattr(x, "rays_ref_equiv"):
        return {"rays": [int(x.rays_primary), int(x.rays_secondary), int(x.rays_shadow), int(x.rays_ref_equiv)]}
    assert isinstance(x, (tuple, list)), type(x)
    return [described(y) for y in x]


def good_case(gpu, depth, e, geom):
    from ndt_amd.hip import NdtHipError
    try:
        got = e.good(gpu, depth, geom)
    except NdtHipError as err:
        return {"refused": [err.code, str(err)]}, None
    out = {"returned": described(got if isinstance(got, (tuple, list)) else (got,))}
    out["counters"] = {name: getattr(gpu, name)() for name in COUNTERS}
    return out, got


def refusal(gpu, x, e, p, out_bytes, cap, K, null=False, misalign=False):
    """One refused (or empty) raw call: its return code, the library's message, and whether the output kept its pattern"""
    if e.kind == "device":
        import torch
        buf = torch.full((out_bytes + 16,), PATTERN, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ptr = None if null else C.c_void_p(buf.data_ptr() + (4 if misalign else 0))
    else:
        buf = np.full(out_bytes + 16, PATTERN, dtype=np.uint8)
        ptr = None if null else C.c_void_p(buf.ctypes.data)
    if e.stage == "apng":
        from ndt_amd.flat_scene import shard_rows
        gpu.apng_begin(W, max(shard_rows(H, p.row_begin, p.row_step), 1), 1)
    rc = int(e.raw(gpu, x, C.byref(p), ptr, int(cap), int(K)))
    message = (gpu.lib.ndt_hip_last_error() or b"").decode() if rc else ""
    if e.kind == "device":
        gpu.synchronize()
        buf = buf.cpu().numpy()
    return {"rc": rc, "message": message, "untouched": bool((buf == PATTERN).all())}


def refusals(gpu, x, depth, e, got):
    from ndt_amd import hip
    K = e.K if e.K is not None else 0
    room = 1 << 16                  # more than any output of the 24 x 10 frame
    p = gpu.params(W, H, depth, samples=e.samples)
    x.ap = hip.ao_params(**e.ao)
    out = {"null": refusal(gpu, x, e, p, room, room, K, null=True)}
    out["zero_rows"] = refusal(gpu, x, e, gpu.params(W, H, depth, row_begin=H, samples=e.samples), room, room, K)
    if e.kind == "file":
        assert isinstance(got[0], bytes)
        out["cap_short"] = refusal(gpu, x, e, p, room, len(got[0]) - 1, K)
        if e.stage != "apng":
            out["bound"] = refusal(gpu, x, e, gpu.params(BIG[0], BIG[1], depth, samples=e.samples), room, room, K)
    if e.K is not None:
        out["k0"] = refusal(gpu, x, e, p, room, room, 0)
        out["k9"] = refusal(gpu, x, e, p, room, room, 9)
    if e.kind == "device":
        out["misaligned"] = refusal(gpu, x, e, p, room, room, K, misalign=True)
    return out


def run_matrix():
    """Every case once, one context a stage; {name: record}"""
    from ndt_amd.hip import NdtHip
    scene, depth = _scene()
    x = Scratch()
    cases = {}
    for stage in dict.fromkeys(e.stage for e in ENTRIES):
        gpu = NdtHip(0)
        try:
            if stage == "denoise":
                gpu.set_option("sample_seed", SEED)
            gpu.upload_scene(scene)
            for e in ENTRIES:
                if e.stage != stage:
                    continue
                rec, got = good_case(gpu, depth, e, {})
                rec["shard"], _ = good_case(gpu, depth, e, SHARD)
                if got is not None:
                    rec["refusals"] = refusals(gpu, x, depth, e, got if isinstance(got, (tuple, list)) else (got,))
                cases[e.name] = rec
        finally:
            gpu.close()
    return cases


def differing(a, b, path=""):
    """the paths at which two records differ"""
    if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys():
        return [d for k in a for d in differing(a[k], b[k], path + "/" + k)]
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [d for k in range(len(a)) for d in differing(a[k], b[k], "%s/%d" % (path, k))]
    return [] if a == b else [path]


def masked(cases, paths):
    """`cases` without what the record names as different from one pass to the next"""
    cases = json.loads(json.dumps(cases))
    for path in paths:
        node, keys = cases, path.strip("/").split("/")
        for k in keys[:-1]:
            node = node[int(k)] if isinstance(node, list) else node[k]
        last = int(keys[-1]) if isinstance(node, list) else keys[-1]
        node[last] = "masked"
    return cases


def main():
    first, second = run_matrix(), run_matrix()
    paths = differing(first, second)
    record = {"scene": SCENE, "frame": [W, H], "shard": SHARD, "bound_size": list(BIG), "entries": [e.name for e in ENTRIES],
              "no_bound_case": NO_BOUND, "masked": paths, "cases": masked(first, paths)}
    with open(RECORD, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, %d fields differ between two passes: %s" % (len(first), len(paths), paths))


if __name__ == "__main__":
    main()
