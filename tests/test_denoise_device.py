"""A sampled frame denoised on the device (ndt_denoise.hip; `ndt_hip --denoise`): an edge-avoiding a-trous wavelet over the double
framebuffer, guided by the feature planes -- the object, N-D hit point and N-D normal of every pixel's primary ray.

The yardstick is numpy's restatement of the definition in include/ndt_hip.h, written here (atrous_model) and checked against a
scalar restatement of the same text (atrous_scalar): only + - * / and comparisons on doubles, one operation at a time, sums over
the components in ascending order, the 25 taps j outer and i inner.  The library is built with -ffp-contract=off, so the device
has to give the model's 64-bit patterns: every comparison with the device below is of view(np.uint64), never a tolerance.  Nothing
here asserts image quality on rendered frames, or a time.
"""
import ctypes as C
import importlib.util
import json
import math
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, GOLDEN, golden

from ndt_amd import hip as nh
from ndt_amd import load_scene

NDT_E_INVALID, NDT_E_UNSUPPORTED = -1, -2
HOST = os.path.join(ROOT, "ndt_amd", "host")
DRIVER = os.path.join(HOST, "ndt_hip")
NEW_SYMBOLS = ("ndt_hip_denoise_device", "ndt_hip_render_denoised_device", "ndt_hip_render_denoised", "ndt_hip_render_denoised_rgba8",
               "ndt_hip_render_denoised_png", "ndt_hip_render_denoised_jpeg", "ndt_hip_render_denoised_exr", "ndt_hip_denoise_launches",
               "ndt_hip_denoise_ms")
H = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)

_spec = importlib.util.spec_from_file_location("make_golden_driver", os.path.join(GOLDEN, "make_golden_driver.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)
# what `ndt_hip -n 2 --png --deflate gpu` left and said on the commit before the denoiser (the recorder's scene and base flags)
PARENT_RECORD = os.path.join(GOLDEN, "denoise_driver_parent.json")
SAMPLED_PNG = ["-n", "2", "--png", "--deflate", "gpu"]


# ---------------------------------------------------------------- the yardstick

def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def atrous_model(rgba, ident, position, normal, iterations=4, sigma_colour=0.25, sigma_plane=0.25, normal_power_log2=5):
    """The definition, vectorised over the pixels and nothing else: rgba (rows, width, 4), ident (rows, width) int32, position and
    normal (dims, rows, width).  Every tap is one slice shifted against another; a tap that is not taken leaves num and den as
    they are (np.where), which is what skipping it does."""
    cur = np.array(rgba, dtype=np.float64, copy=True)
    ident = np.asarray(ident)
    rows, width = ident.shape
    dims = position.shape[0]
    assert cur.shape == (rows, width, 4) and position.shape == normal.shape == (dims, rows, width)
    inv_p = 1.0 / (sigma_plane * sigma_plane)
    background = (ident == 0)[..., None]
    with np.errstate(all="ignore"):
        for it in range(iterations):
            s = 1 << it
            sc = sigma_colour / float(1 << it)
            inv_c = 1.0 / (sc * sc)
            num, den = np.zeros((rows, width, 4)), np.zeros((rows, width))
            for j in range(5):
                for i in range(5):
                    h = H[j] * H[i]
                    dy, dx = (j - 2) * s, (i - 2) * s
                    if dy == 0 and dx == 0:
                        num = num + h * cur
                        den = den + h
                        continue
                    y0, y1, x0, x1 = max(0, -dy), min(rows, rows - dy), max(0, -dx), min(width, width - dx)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    p = (slice(y0, y1), slice(x0, x1))
                    q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                    dd, nd, dot = np.zeros(den[p].shape), np.zeros(den[p].shape), np.zeros(den[p].shape)
                    for k in range(dims):
                        d = position[k][q] - position[k][p]
                        dd = dd + d * d
                        nd = nd + normal[k][p] * d
                        dot = dot + normal[k][p] * normal[k][q]
                    wn = np.where(dot > 0, dot, 0.0)
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    wp = np.where(dd > 0, 1.0 - ((nd * nd) / dd) * inv_p, 1.0)
                    dr, dg, db = cur[q][..., 0] - cur[p][..., 0], cur[q][..., 1] - cur[p][..., 1], cur[q][..., 2] - cur[p][..., 2]
                    cc = (dr * dr + dg * dg) + db * db
                    wc = 1.0 / (1.0 + cc * inv_c)
                    w = ((h * wn) * wp) * wc
                    take = (ident[q] == ident[p]) & (w > 0)
                    num[p] = np.where(take[..., None], num[p] + w[..., None] * cur[q], num[p])
                    den[p] = np.where(take, den[p] + w, den[p])
            cur = np.where(background, cur, num / den[..., None])
    return cur


def atrous_scalar(rgba, ident, position, normal, iterations=4, sigma_colour=0.25, sigma_plane=0.25, normal_power_log2=5):
    """The same text, one pixel and one tap at a time in Python floats (IEEE doubles): what the vectorised model is checked against."""
    rows, width = ident.shape
    dims = position.shape[0]
    cur = [[[float(v) for v in rgba[y, x]] for x in range(width)] for y in range(rows)]
    inv_p = 1.0 / (sigma_plane * sigma_plane)
    for it in range(iterations):
        s = 1 << it
        sc = sigma_colour / float(1 << it)
        inv_c = 1.0 / (sc * sc)
        nxt = [[None] * width for _ in range(rows)]
        for y in range(rows):
            for x in range(width):
                me = int(ident[y, x])
                if me == 0:
                    nxt[y][x] = list(cur[y][x])
                    continue
                num, den = [0.0, 0.0, 0.0, 0.0], 0.0
                for j in range(5):
                    for i in range(5):
                        qy, qx = y + (j - 2) * s, x + (i - 2) * s
                        h = H[j] * H[i]
                        if j == 2 and i == 2:
                            w = h
                        else:
                            if qy < 0 or qy >= rows or qx < 0 or qx >= width or int(ident[qy, qx]) != me:
                                continue
                            dd = nd = dot = 0.0
                            for k in range(dims):
                                d = float(position[k, qy, qx]) - float(position[k, y, x])
                                dd = dd + d * d
                                nd = nd + float(normal[k, y, x]) * d
                                dot = dot + float(normal[k, y, x]) * float(normal[k, qy, qx])
                            wn = dot if dot > 0 else 0.0
                            for _ in range(normal_power_log2):
                                wn = wn * wn
                            wp = 1.0 - ((nd * nd) / dd) * inv_p if dd > 0 else 1.0
                            a, b = cur[qy][qx], cur[y][x]
                            cc = ((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1])) + (a[2] - b[2]) * (a[2] - b[2])
                            wc = 1.0 / (1.0 + cc * inv_c)
                            w = ((h * wn) * wp) * wc
                            if not w > 0:
                                continue
                        for c in range(4):
                            num[c] = num[c] + w * cur[qy][qx][c]
                        den = den + w
                nxt[y][x] = [n / den for n in num]
        cur = nxt
    return np.array(cur, dtype=np.float64).reshape(rows, width, 4)


def random_inputs(rows, width, dims, seed):
    """Seeded inputs that take every branch: ids in 8 x 8 blocks, id 0 among them; unit normals near axis 0 and hit points near the
    hyperplane across it, so that the normal and plane weights are neither 0 nor 1; every fifth column sharing one position, so
    that dd == 0 between vertical neighbours there; colours in 0 .. 2."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 3, ((rows + 7) // 8, (width + 7) // 8)).astype(np.int32)
    blocks[0, 0] = 1                        # (a 1 x 1 frame is filtered, not copied)
    if blocks.size > 1:
        blocks.flat[blocks.size - 1] = 0
    ident = np.ascontiguousarray(np.kron(blocks, np.ones((8, 8), dtype=np.int32))[:rows, :width])
    normal = 0.15 * rng.standard_normal((dims, rows, width))
    normal[0] += 1.0
    normal = normal / np.sqrt((normal * normal).sum(axis=0))
    position = rng.standard_normal((dims, rows, width))
    position[0] *= 0.05
    position[:, :, ::5] = rng.standard_normal((dims, 1, 1))
    rgba = rng.uniform(0.0, 2.0, (rows, width, 4))
    return rgba, ident, np.ascontiguousarray(position), np.ascontiguousarray(normal)


def synthetic_frame(rows=37, width=67, seed=5, sigma=0.08):
    """A 4-D frame seen along axis 2: background (id 0) above, a shaded plane (id 1) tilted into axis 3 below, a sphere (id 2) in
    front of both; its clean colours, the same with seeded Gaussian noise of `sigma` on r, g, b, and the guides."""
    v, u = np.meshgrid(np.linspace(-1.0, 1.0, rows), np.linspace(-1.8, 1.8, width), indexing="ij")
    ident = np.zeros((rows, width), dtype=np.int32)
    position, normal = np.zeros((4, rows, width)), np.zeros((4, rows, width))
    clean = np.zeros((rows, width, 4))
    clean[..., :3] = (0.1, 0.2, 0.4)
    clean[..., 3] = 1.0
    light = np.array([0.4, -0.5, -0.7, 0.3])
    light /= np.sqrt((light * light).sum())
    plane = v > -0.2
    n_plane = np.array([0.0, -1.0, -1.0, 1.0]) / math.sqrt(3.0)         # across both tangents of the plane below
    ident[plane] = 1
    position[:, plane] = np.stack([u[plane], v[plane], 2.0 - 0.5 * v[plane], 0.5 * v[plane]])
    normal[:, plane] = n_plane[:, None]
    shade = 0.25 + 0.6 * float(n_plane @ light)
    clean[plane, :3] = shade * np.stack([0.9 - 0.2 * u[plane], 0.7 + 0.1 * v[plane], 0.5 + 0.15 * u[plane]], axis=-1)
    r2 = u * u + (v + 0.1) * (v + 0.1)
    ball = r2 < 0.49
    ident[ball] = 2
    nb = np.stack([u[ball], v[ball] + 0.1, -np.sqrt(0.49 - r2[ball]), np.zeros(int(ball.sum()))]) / 0.7
    position[:, ball] = 0.7 * nb + np.array([0.0, -0.1, 1.0, 0.0])[:, None]
    normal[:, ball] = nb
    lambert = np.maximum(nb.T @ light, 0.0)
    clean[ball, :3] = (0.15 + 0.8 * lambert)[:, None] * np.array([0.9, 0.3, 0.2])
    noisy = clean.copy()
    noisy[..., :3] += np.random.default_rng(seed).normal(0.0, sigma, (rows, width, 3))
    return clean, noisy, ident, position, normal


def read_png(data):
    """The pixels [h, w, 4] of an 8-bit RGBA PNG with filters 0 / 1 / 2 (the reader of tests/test_png_device.py)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert zlib.crc32(typ + body) == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0], typ
        if typ == b"IHDR":
            w, h = struct.unpack(">II", body[:8])
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)
    out = np.zeros((h, w, 4), dtype=np.uint8)
    for r in range(h):
        row = raw[r, 1:].reshape(w, 4)
        if raw[r, 0] == 1:
            row = np.cumsum(row, axis=0, dtype=np.uint8)
        elif raw[r, 0] == 2 and r > 0:
            row = row + out[r - 1]
        out[r] = row
    return out


# ---------------------------------------------------------------- CPU

def test_declared_bound_and_exported(tmp_path):
    """(CPU) the header declares every new entry point, hip.py binds it, the library exports it; ndt_denoise_params is 24 bytes to
    a C compiler and to ctypes."""
    with open(os.path.join(ROOT, "include", "ndt_hip.h")) as f:
        header = f.read()
    lib = nh.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"^(int|double) %s\(" % name, header, re.M), name
        assert name in nh.API_SYMBOLS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.ndt_hip_denoise_ms.restype is C.c_double
    assert lib.ndt_hip_abi_version() == 3 and "#define NDT_HIP_ABI_VERSION 3" in header
    for method in ("denoise", "render_denoised", "denoise_launches", "denoise_ms"):
        assert callable(getattr(nh.NdtHip, method, None)), method
    assert C.sizeof(nh.DenoiseParams) == 24
    d = nh.denoise_params()
    assert (d.iterations, d.normal_power_log2, d.sigma_colour, d.sigma_plane) == (4, 5, 0.25, 0.25)
    assert (nh.DenoiseParams.iterations.offset, nh.DenoiseParams.normal_power_log2.offset, nh.DenoiseParams.sigma_colour.offset,
            nh.DenoiseParams.sigma_plane.offset) == (0, 4, 8, 16)
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ndt_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ndt_denoise_params), offsetof(ndt_denoise_params, iterations),\n'
                   '    offsetof(ndt_denoise_params, normal_power_log2), offsetof(ndt_denoise_params, sigma_colour),\n'
                   '    offsetof(ndt_denoise_params, sigma_plane)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["24", "0", "4", "8", "16"]


@pytest.mark.parametrize("rows,width,dims", [(1, 1, 3), (1, 11, 4), (9, 7, 3), (6, 13, 7), (11, 5, 12)])
def test_the_vectorised_model_is_the_scalar_text(rows, width, dims):
    """(CPU) bit for bit, at 1, 3 and 5 iterations (at 5 the step of 16 exceeds every one of these frames) and other parameters
    than the defaults."""
    rgba, ident, position, normal = random_inputs(rows, width, dims, 100 * rows + width)
    for kw in ({"iterations": 1}, {"iterations": 3, "sigma_colour": 0.3}, {"iterations": 5, "sigma_plane": 0.4, "normal_power_log2": 2},
               {"iterations": 2, "normal_power_log2": 0}):
        want = atrous_scalar(rgba, ident, position, normal, **kw)
        got = atrous_model(rgba, ident, position, normal, **kw)
        assert same_bits(got, want), kw
        assert same_bits(got[ident == 0], rgba[ident == 0])
        if rows * width > 1:
            assert not same_bits(got[ident != 0], rgba[ident != 0])
    # the taps are weighed, not just counted: the weights of these inputs lie strictly between 0 and h on a good share of them
    if rows * width > 30:
        one = atrous_model(rgba, ident, position, normal, iterations=1)
        flat = atrous_model(rgba, ident, position, normal, iterations=1, normal_power_log2=0, sigma_plane=1e6, sigma_colour=1e6)
        assert not same_bits(one, flat)


def test_the_model_sums_in_the_stated_order():
    """(CPU) a row of five pixels of one object whose alphas are 1e17, 1, 1, 1, 1: the taps are added left to right, i inner -- the
    small ones are lost one by one behind the large one, and survive together in front of it."""
    ident = np.ones((1, 5), dtype=np.int32)
    position, normal = np.zeros((3, 1, 5)), np.zeros((3, 1, 5))
    normal[2] = 1.0
    rgba = np.zeros((1, 5, 4))
    rgba[0, :, 3] = [1e17, 1.0, 1.0, 1.0, 1.0]              # alpha: no part of the colour distance, so every wc is 1
    got = atrous_model(rgba, ident, position, normal, iterations=1)
    w = [H[2] * H[i] for i in range(5)]
    num = 0.0
    for i in range(5):
        num = num + w[i] * rgba[0, i, 3]
    den = 0.0
    for i in range(5):
        den = den + w[i]
    assert got[0, 2, 3] == num / den
    backwards = 0.0
    for i in reversed(range(5)):
        backwards = backwards + w[i] * rgba[0, i, 3]
    assert backwards != num


def test_the_model_denoises_leaves_the_background_and_keeps_a_nan_to_itself():
    """(CPU) on the synthetic plane, sphere and background frame with seeded noise of sigma 0.08 and 3 iterations (sigma_colour 0.3,
    sigma_plane 0.25, power 5): the mean squared error against the clean frame falls at least 4 x on each object (a floor: the
    model gives far more), id-0 pixels keep their bits, nothing leaks across an id boundary, and one NaN pixel stays one."""
    clean, noisy, ident, position, normal = synthetic_frame()
    kw = dict(iterations=3, sigma_colour=0.3, sigma_plane=0.25, normal_power_log2=5)
    out = atrous_model(noisy, ident, position, normal, **kw)
    for obj, name in ((1, "plane"), (2, "sphere")):
        m = ident == obj
        assert m.sum() > 300
        before = float(((noisy[m][:, :3] - clean[m][:, :3]) ** 2).mean())
        after = float(((out[m][:, :3] - clean[m][:, :3]) ** 2).mean())
        print("%s: %d pixels, MSE %.3g -> %.3g (%.1f x)" % (name, int(m.sum()), before, after, before / after))
        assert 5.5e-3 < before < 7.5e-3 and after * 4.0 <= before
    assert (ident == 0).sum() > 300 and same_bits(out[ident == 0], noisy[ident == 0])
    assert same_bits(out[..., 3], noisy[..., 3])                        # alpha 1 everywhere on the objects: a weighted mean of ones
    # nothing crosses an id boundary: the sphere painted another colour changes no pixel of the plane
    other = noisy.copy()
    other[ident == 2, :3] += 5.0
    out2 = atrous_model(other, ident, position, normal, **kw)
    assert same_bits(out2[ident == 1], out[ident == 1]) and not same_bits(out2[ident == 2], out[ident == 2])
    # one NaN pixel: its own centre tap keeps it a NaN; every other pixel drops the tap (w > 0 fails) and stays finite
    for y, x in ((30, 20), (18, 33)):
        assert ident[y, x] != 0
        poisoned = noisy.copy()
        poisoned[y, x, 1] = np.nan
        out3 = atrous_model(poisoned, ident, position, normal, **kw)
        bad = np.isnan(out3).any(axis=2)
        assert bad[y, x] and bad.sum() == 1
        far = np.ones_like(bad)
        far[max(0, y - 14):y + 15, max(0, x - 14):x + 15] = False       # 3 iterations reach 2 * (1 + 2 + 4) = 14 pixels
        assert same_bits(out3[far], out[far])


def _run_driver(cwd, *flags, scene="builtin:yaml", dims=4, size="16x9"):
    assert os.path.exists(DRIVER), "ndt_amd/host/ndt_hip is not built"
    os.makedirs(str(cwd), exist_ok=True)
    return subprocess.run([DRIVER, "-s", scene, "-d", str(dims), "-f", "0", "-r", size, "-l", "6"] + list(flags),
                          capture_output=True, text=True, cwd=str(cwd))


def test_driver_refuses_what_denoise_does_not_go_with_by_name(tmp_path):
    """(CPU) every refusal ends the run non-zero with one line on stderr that names the cause, before a scene is loaded or a device
    asked for: nothing is written."""
    for flags, words in ((["--denoise", "-a", "20,3"], ("--denoise", "-a")),
                         (["--denoise", "2", "-m", "s"], ("--denoise", "-m s")),
                         (["--denoise", "-m", "o"], ("--denoise", "-m o")),
                         (["--denoise", "-m", "a"], ("--denoise", "-m a")),
                         (["--denoise", "-m", "h"], ("--denoise", "-m h")),
                         (["--denoise", "3", "-g", "2"], ("--denoise", "-g 2")),
                         (["--denoise", "--ssaa", "2"], ("--denoise", "--ssaa 2")),
                         (["--denoise", "--apng"], ("--denoise", "--apng")),
                         (["--denoise", "--png", "--deflate", "gpu", "--png16"], ("--denoise", "--png16")),
                         (["--denoise", "-z"], ("--denoise", "-z")),
                         (["--denoise", "--exr", "--exr-aov", "all"], ("--denoise", "--exr-aov")),
                         (["--denoise-colour", "0.3"], ("--denoise-colour", "needs --denoise")),
                         (["--denoise-plane", "0.3", "--png"], ("--denoise-plane", "needs --denoise")),
                         (["--denoise-normal", "4", "--jpeg"], ("--denoise-normal", "needs --denoise")),
                         (["--denoise", "0"], ("--denoise", "1 .. 6", "'0'")),
                         (["--denoise", "7"], ("--denoise", "1 .. 6", "'7'")),
                         (["--denoise=x"], ("--denoise", "1 .. 6", "'x'")),
                         (["--denoise", "--denoise-colour", "0"], ("--denoise-colour", "above 0")),
                         (["--denoise", "--denoise-colour", "nan"], ("--denoise-colour", "above 0")),
                         (["--denoise", "--denoise-plane", "-1"], ("--denoise-plane", "above 0")),
                         (["--denoise", "--denoise-plane", "inf"], ("--denoise-plane", "above 0")),
                         (["--denoise", "--denoise-normal", "9"], ("--denoise-normal", "0 .. 8"))):
        r = _run_driver(tmp_path, *flags)
        assert r.returncode != 0, flags
        for w in words:
            assert w in r.stderr, (flags, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, (flags, r.stderr)       # the refusal and nothing else: no device was asked for
    assert not [p for p in tmp_path.rglob("*") if p.is_file()]
    usage = _run_driver(tmp_path, "-h")
    assert usage.returncode == 0 and "--denoise [1..6]" in usage.stderr and "--denoise-normal 0..8" in usage.stderr


def test_the_parent_record_is_of_the_recorders_scene():
    """(CPU) the record of the run without --denoise was made with the driver-matrix recorder's scene and base flags."""
    with open(PARENT_RECORD) as f:
        rec = json.load(f)
    assert rec["base"] == recorder.BASE and tuple(rec["documents"]) == recorder.DOCUMENTS and rec["flags"] == SAMPLED_PNG
    assert len(rec["files"]) == 2 and all(p.endswith(".png") for p in rec["files"])
    assert not any("denoise" in line for line in rec["stdout"])


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


class DeviceFrame:
    """inputs of the filter in device memory (torch), with room behind the image for a pattern that must survive"""
    GUARD = 64

    def __init__(self, rgba, ident, position, normal):
        import torch
        self.torch = torch
        self.n = rgba.size
        self.shape = rgba.shape
        self.rgba = torch.from_numpy(np.concatenate([rgba.reshape(-1), np.full(self.GUARD, -7.0)])).cuda()
        self.ident = torch.from_numpy(np.ascontiguousarray(ident)).cuda()
        self.position = torch.from_numpy(np.ascontiguousarray(position)).cuda()
        self.normal = torch.from_numpy(np.ascontiguousarray(normal)).cuda()
        self.out = torch.full((self.n + self.GUARD,), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        self.planes = {"id": self.ident.data_ptr(), "position": self.position.data_ptr(), "normal": self.normal.data_ptr()}

    def image(self, t):
        host = t.cpu().numpy()
        assert (host[self.n:] == -7.0).all(), "the filter wrote behind its image"
        return host[:self.n].reshape(self.shape)


FRAMES = [(1, 1), (1, 70), (37, 67), (33, 5), (19, 130)]        # rows x width


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [3, 4, 7, 12])
@pytest.mark.parametrize("rows,width", FRAMES)
def test_the_filter_alone_is_the_model_bit_for_bit(gpu, rows, width, dims):
    """ndt_hip_denoise_device at 1, 3 and 6 iterations (at 6 the step of 32 exceeds the narrow frames): a lone pixel, a single row,
    a frame narrower than the stencil, a width that is no multiple of 64, the largest N.  The input is left as it was."""
    rgba, ident, position, normal = random_inputs(rows, width, dims, 1000 * rows + 10 * width + dims)
    dev = DeviceFrame(rgba, ident, position, normal)
    for iterations, extra in ((1, {}), (3, {"sigma_colour": 0.3, "normal_power_log2": 3}), (6, {"sigma_plane": 0.4})):
        want = atrous_model(rgba, ident, position, normal, iterations=iterations, **extra)
        gpu.denoise(dev.rgba.data_ptr(), dev.planes, dims, width, rows, dev.out.data_ptr(), iterations=iterations, **extra)
        got = dev.image(dev.out)
        differ = int((bits(got) != bits(want)).sum())
        print("%d x %d, N = %d, %d iterations: %d of %d doubles differ from the model" % (rows, width, dims, iterations, differ, want.size))
        assert differ == 0
        assert gpu.denoise_launches() == iterations and gpu.denoise_ms() >= 0.0
        assert same_bits(dev.image(dev.rgba), rgba)
        assert same_bits(got[ident == 0], rgba[ident == 0])


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_in_place_gives_the_same_bits(gpu, iterations):
    rows, width, dims = 19, 130, 4
    rgba, ident, position, normal = random_inputs(rows, width, dims, 77)
    dev = DeviceFrame(rgba, ident, position, normal)
    gpu.denoise(dev.rgba.data_ptr(), dev.planes, dims, width, rows, iterations=iterations)
    assert same_bits(dev.image(dev.rgba), atrous_model(rgba, ident, position, normal, iterations=iterations))
    assert gpu.denoise_launches() == iterations


END_TO_END = {"al_zoo4d_n2": ("al_zoo4d", 2, 0), "al_zoo3d_dof_n3": ("al_zoo3d_dof_n3", 3, 0), "zoo12d_n1": ("zoo12d", 1, 0),
              "al_zoo4d_n2_levels": ("al_zoo4d", 2, 1), "al_zoo4d_n2_stream": ("al_zoo4d", 2, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(END_TO_END))
def test_a_denoised_frame_is_the_model_of_the_render_and_its_features(gpu, case):
    """render_denoised(samples=S) equals the model applied to render(samples=S) and render_features(samples=1) of the same context
    and seed, bit for bit, at 33 x 17 (partial 8 x 8 tiles on both edges), under every pipeline for the 4-D area-light scene."""
    name, samples, pipeline = END_TO_END[case]
    g = golden(name)
    w, h = 33, 17
    try:
        gpu.set_option("pipeline", pipeline)
        gpu.upload_scene(g.scene)
        fb, _ = gpu.render(w, h, g.depth, samples=samples)
        f = gpu.render_features(w, h, g.depth)
        assert (f["id"] > 0).any()
        for kw in ({}, {"iterations": 2, "sigma_colour": 0.5, "sigma_plane": 0.3, "normal_power_log2": 3}):
            want = atrous_model(fb, f["id"], f["position"], f["normal"], **kw)
            got, st = gpu.render_denoised(w, h, g.depth, samples=samples, **kw)
            differ = int((bits(got) != bits(want)).sum())
            print("%s %r: %d of %d doubles differ from the model; %d of %d pixels hit" % (case, kw, differ, want.size, int((f["id"] > 0).sum()), f["id"].size))
            assert differ == 0
            assert gpu.denoise_launches() == 4 + kw.get("iterations", 4) and gpu.features_launches() == 4
            assert st.rays_primary > 0
        assert not same_bits(want, fb)
        if samples > 1:
            # the frame is a stochastic one: its samples differ from the deterministic frame's
            assert not same_bits(fb, gpu.render(w, h, g.depth)[0])
    finally:
        gpu.set_option("pipeline", 0)


@pytest.mark.gpu
def test_a_denoised_frame_left_on_the_device(gpu):
    import torch
    g = golden("al_zoo4d")
    w, h = 33, 17
    gpu.upload_scene(g.scene)
    fb, _ = gpu.render(w, h, g.depth, samples=2)
    f = gpu.render_features(w, h, g.depth)
    out = torch.full((w * h * 4 + 64,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_denoised(w, h, g.depth, sink="device", d_rgba_ptr=out.data_ptr(), samples=2, iterations=3)
    host = out.cpu().numpy()
    assert (host[w * h * 4:] == -7.0).all()
    assert same_bits(host[:w * h * 4].reshape(h, w, 4), atrous_model(fb, f["id"], f["position"], f["normal"], iterations=3))


@pytest.mark.gpu
def test_a_denoised_frame_changes_no_later_render_map_or_feature_pass(gpu):
    g = golden("al_zoo4d")
    w, h = 33, 17
    gpu.upload_scene(g.scene)
    fb, dm, _ = gpu.render(w, h, g.depth, depth_map=True)
    sampled, _ = gpu.render(w, h, g.depth, samples=2)
    f = gpu.render_features(w, h, g.depth, rays=True)
    gpu.render_denoised(w, h, g.depth, samples=2)
    gpu.render_denoised(w, h, g.depth, sink="png", samples=3, iterations=6)
    fb2, dm2, _ = gpu.render(w, h, g.depth, depth_map=True)
    assert same_bits(fb2, fb) and same_bits(dm2, dm)
    assert same_bits(gpu.render(w, h, g.depth, samples=2)[0], sampled)
    f2 = gpu.render_features(w, h, g.depth, rays=True)
    assert np.array_equal(f2["id"], f["id"]) and all(same_bits(f2[k], f[k]) for k in ("position", "normal", "ray_o", "ray_v"))


@pytest.mark.gpu
def test_the_sinks_take_the_models_doubles(gpu, oracle):
    """rgba8 is oracle.quantize of the model's frame; the PNG decodes to exactly that; the JPEG is ndt_hip_encode_jpeg of those
    pixels and the EXR ndt_hip_encode_exr of the model's doubles, byte for byte."""
    g = golden("al_zoo4d")
    w, h, samples = 33, 17, 2
    gpu.upload_scene(g.scene)
    fb, _ = gpu.render(w, h, g.depth, samples=samples)
    f = gpu.render_features(w, h, g.depth)
    kw = dict(samples=samples, iterations=3, sigma_colour=0.3)
    want = atrous_model(fb, f["id"], f["position"], f["normal"], iterations=3, sigma_colour=0.3)
    want8 = oracle.quantize(want)
    assert not np.array_equal(want8, oracle.quantize(fb))
    got8, _ = gpu.render_denoised(w, h, g.depth, sink="rgba8", **kw)
    assert np.array_equal(got8, want8) and gpu.denoise_launches() == 7
    png, _ = gpu.render_denoised(w, h, g.depth, sink="png", **kw)
    assert np.array_equal(read_png(png), want8) and gpu.png_stats.png_bytes == len(png)
    for quality, sampling in ((95, "420"), (50, "444")):
        jpg, _ = gpu.render_denoised(w, h, g.depth, sink="jpeg", quality=quality, sampling=sampling, **kw)
        assert jpg == gpu.encode_jpeg(want8, quality, sampling)
    for pixel in ("half", "float"):
        exr, _ = gpu.render_denoised(w, h, g.depth, sink="exr", pixel=pixel, **kw)
        assert exr == gpu.encode_exr(want, pixel=pixel)


@pytest.mark.gpu
def test_the_library_refuses_by_code_and_cause_and_writes_nothing(gpu):
    import torch
    lib = gpu.lib
    g = golden("al_zoo4d")
    w, h = 33, 17
    gpu.upload_scene(g.scene)
    ok = nh.denoise_params()
    entries = (("ndt_hip_render_denoised", lambda p, dp, buf: lib.ndt_hip_render_denoised(gpu.ctx, C.byref(p), C.byref(dp), buf.ctypes.data, None)),
               ("ndt_hip_render_denoised_rgba8", lambda p, dp, buf: lib.ndt_hip_render_denoised_rgba8(gpu.ctx, C.byref(p), C.byref(dp), buf.ctypes.data, None)),
               ("ndt_hip_render_denoised_png", lambda p, dp, buf: lib.ndt_hip_render_denoised_png(gpu.ctx, C.byref(p), C.byref(dp), buf.ctypes.data, buf.size, None, None)),
               ("ndt_hip_render_denoised_jpeg", lambda p, dp, buf: lib.ndt_hip_render_denoised_jpeg(gpu.ctx, C.byref(p), C.byref(dp), None, buf.ctypes.data, buf.size, None, None)),
               ("ndt_hip_render_denoised_exr", lambda p, dp, buf: lib.ndt_hip_render_denoised_exr(gpu.ctx, C.byref(p), C.byref(dp), None, buf.ctypes.data, buf.size, None, None)))
    frames = [({"aa": (20, 3)}, ok, NDT_E_UNSUPPORTED, "recursive_aa")]
    frames += [({"stereo": m}, ok, NDT_E_UNSUPPORTED, "stereo mode %d" % m) for m in (1, 2, 3, 4)]
    frames += [({"row_begin": 1, "row_step": 3}, ok, NDT_E_UNSUPPORTED, "row shard"), ({"row_step": 2}, ok, NDT_E_UNSUPPORTED, "row shard")]
    frames += [({}, nh.DenoiseParams(k, 5, 0.25, 0.25), NDT_E_INVALID, "%d iterations" % k) for k in (0, 7)]
    frames += [({}, nh.DenoiseParams(4, 5, s, 0.25), NDT_E_INVALID, "sigma_colour") for s in (0.0, -0.25, math.nan)]
    frames += [({}, nh.DenoiseParams(4, 5, 0.25, s), NDT_E_INVALID, "sigma_plane") for s in (0.0, -0.25, math.nan, math.inf)]
    frames += [({}, nh.DenoiseParams(4, 9, 0.25, 0.25), NDT_E_INVALID, "normal_power_log2 9")]
    for kw, dp, code, word in frames:
        p = gpu.params(w, h, g.depth, samples=2, **kw)
        for name, call in entries:
            buf = np.full(w * h * 32, 0xA5, dtype=np.uint8)
            assert call(p, dp, buf) == code, (name, kw, word)
            err = lib.ndt_hip_last_error().decode()
            assert word in err and name in err, (name, err)
            assert (buf == 0xA5).all()
    # the filter alone: the same parameters, a NULL plane, a misaligned one, dimensions it is not built for
    rgba, ident, position, normal = random_inputs(9, 16, 4, 5)
    dev = DeviceFrame(rgba, ident, position, normal)

    def alone(dp=ok, dims=4, width=16, rows=9, src=None, dst=None, **planes):
        pl = dict(dev.planes, **planes)
        fp = nh.FeaturePlanes(pl["id"], pl["position"], pl["normal"], None, None)
        return lib.ndt_hip_denoise_device(gpu.ctx, C.c_void_p(dev.rgba.data_ptr() if src is None else src), C.byref(fp), dims, width, rows,
                                          C.byref(dp), C.c_void_p(dev.out.data_ptr() if dst is None else dst))

    for call, word in ((lambda: alone(nh.DenoiseParams(0, 5, 0.25, 0.25)), "0 iterations"), (lambda: alone(nh.DenoiseParams(7, 5, 0.25, 0.25)), "7 iterations"),
                       (lambda: alone(nh.DenoiseParams(4, 5, 0.0, 0.25)), "sigma_colour"), (lambda: alone(nh.DenoiseParams(4, 5, -1.0, 0.25)), "sigma_colour"),
                       (lambda: alone(nh.DenoiseParams(4, 5, math.nan, 0.25)), "sigma_colour"), (lambda: alone(nh.DenoiseParams(4, 5, 0.25, math.nan)), "sigma_plane"),
                       (lambda: alone(nh.DenoiseParams(4, 9, 0.25, 0.25)), "normal_power_log2 9"), (lambda: alone(nh.DenoiseParams(4, -1, 0.25, 0.25)), "normal_power_log2 -1"),
                       (lambda: alone(id=None), "NULL plane"), (lambda: alone(position=None), "NULL plane"), (lambda: alone(normal=None), "NULL plane"),
                       (lambda: alone(position=dev.planes["position"] + 4), "misaligned"), (lambda: alone(id=dev.planes["id"] + 2), "misaligned"),
                       (lambda: alone(dst=dev.out.data_ptr() + 8), "misaligned"), (lambda: alone(src=dev.rgba.data_ptr() + 8), "misaligned"),
                       (lambda: alone(dims=2), "2 dimensions"), (lambda: alone(dims=13), "13 dimensions"), (lambda: alone(width=0), "0 x 9"),
                       (lambda: alone(rows=-1), "16 x -1")):
        assert call() == NDT_E_INVALID, word
        err = lib.ndt_hip_last_error().decode()
        assert word in err and "ndt_hip_denoise_device" in err, err
    torch.cuda.synchronize()
    assert (dev.out.cpu().numpy() == -7.0).all() and same_bits(dev.image(dev.rgba), rgba)
    with pytest.raises(nh.NdtHipError, match="row shard") as e:
        gpu.render_denoised(w, h, g.depth, row_begin=1, row_step=2)
    assert e.value.code == NDT_E_UNSUPPORTED


# ---------------------------------------------------------------- driver

@pytest.mark.gpu
def test_driver_denoises_says_so_and_leaves_the_librarys_file(tmp_path):
    """`ndt_hip --denoise 3 -n 2 --png --deflate gpu` over both frames of the driver matrix's two-document scene at 16 x 9: the line
    of each frame, and the files the library call makes for the scenes the driver loads.  The same run without --denoise says
    nothing of a denoiser and leaves the bytes it left before there was one (tests/golden/denoise_driver_parent.json)."""
    recorder.write_scene(str(tmp_path / recorder.SCENE))
    got = recorder.run_case(DRIVER, str(tmp_path / "denoised"), ["--denoise", "3"] + SAMPLED_PNG)
    assert got["stdout"].count("denoised in 3 iterations on GPU 0 in 7 launches") == 2
    assert sum(line.startswith("compressed PNG of ") for line in got["stdout"]) == 2
    plain = recorder.run_case(DRIVER, str(tmp_path / "plain"), SAMPLED_PNG)
    with open(PARENT_RECORD) as f:
        rec = json.load(f)
    assert plain["files"] == rec["files"] and plain["stdout"] == rec["stdout"]
    assert sorted(got["files"]) == sorted(plain["files"])
    assert all(got["files"][p]["sha256"] != plain["files"][p]["sha256"] for p in plain["files"])
    # the library's files for the same requests, from the scenes the driver loads
    files = [next(p for p in got["files"] if p.endswith("_%04d.png" % k)) for k in (0, 1)]
    gpu = nh.NdtHip(0)
    try:
        for k in (0, 1):
            dump = str(tmp_path / ("frame%d.ndtscene" % k))
            r = subprocess.run([DRIVER] + recorder.BASE[:-2] + ["-f", "%d:%d" % (k, k), "-u", str(tmp_path / recorder.SCENE), "--dump-scene", dump],
                               capture_output=True, text=True, cwd=str(tmp_path))
            assert r.returncode == 0, r.stderr[-2000:]
            gpu.upload_scene(load_scene(dump))
            want, _ = gpu.render_denoised(16, 9, 6, sink="png", samples=2, iterations=3)
            assert gpu.denoise_launches() == 7
            with open(os.path.join(str(tmp_path / "denoised"), files[k]), "rb") as f:
                assert f.read() == want, files[k]
    finally:
        gpu.close()
    # the other sinks and the weights reach the library too: one frame each, each with its line
    for case, (k, flags) in enumerate(((4, ["--denoise"]), (2, ["--denoise", "2", "--png"]), (5, ["--denoise=5", "--jpeg"]),
                                       (4, ["--denoise", "--exr", "--exr-pixel", "float"]),
                                       (1, ["--denoise", "1", "--raw", "f.f64", "--denoise-colour", "0.5", "--denoise-plane", "0.3", "--denoise-normal", "2"]),
                                       (4, ["--denoise", "-n", "2", "-j", "2", "--fit", "gpu", "--kd", "gpu"]))):
        one = recorder.run_case(DRIVER, str(tmp_path / ("case%d" % case)), flags)
        assert one["stdout"].count("denoised in %d iterations on GPU 0 in %d launches" % (k, 4 + k)) == 2, (flags, one["stdout"])
        assert len(one["files"]) >= 2
