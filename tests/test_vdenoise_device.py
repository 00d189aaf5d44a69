"""The variance-guided denoiser (ndt_denoise.hip; `ndt_hip --vdenoise`), the sample moments it feeds on (ndt_hip_render_moments*,
k_sample_variance) and the sample cap (option "sample_cap", `--sample-cap C`) that lets a frame be noisy to begin with.

The yardstick is numpy's restatement of the definitions in include/ndt_hip.h, written here (vatrous_model, variance_model) and
checked against scalar restatements of the same text in Python floats (vatrous_scalar, variance_scalar): only + - * / and
comparisons on doubles, one operation at a time, in the stated order.  The library is built with -ffp-contract=off, so the device
has to give the models' 64-bit patterns: every comparison of a filter or of k_sample_variance with its model is of view(np.uint64),
never a tolerance.  The one tolerance below belongs to the test that rebuilds the second sample of a pixel from two frames, and is
what forming that difference in doubles can lose.  Nothing here asserts image quality on rendered frames, or a time.
"""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden

from ndt_amd import hip as nh
from ndt_amd import load_scene

from test_denoise_device import (DRIVER, H, PARENT_RECORD, SAMPLED_PNG, DeviceFrame, atrous_model, bits, random_inputs, read_png, recorder,
                                 same_bits, synthetic_frame)

NDT_E_INVALID, NDT_E_UNSUPPORTED = -1, -2
NEW_SYMBOLS = ("ndt_hip_render_moments_device", "ndt_hip_render_moments", "ndt_hip_sample_variance_device", "ndt_hip_vdenoise_device",
               "ndt_hip_render_vdenoised_device", "ndt_hip_render_vdenoised", "ndt_hip_render_vdenoised_rgba8", "ndt_hip_render_vdenoised_png",
               "ndt_hip_render_vdenoised_jpeg", "ndt_hip_render_vdenoised_exr")
G = (1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0)


# ---------------------------------------------------------------- the yardstick

def variance_model(rgba, count, sum_sq):
    """k_sample_variance, vectorised over the pixels: rgba (rows, width, 4), count (rows, width) int32, sum_sq (3, rows, width)."""
    count = np.asarray(count)
    n = count.astype(np.float64)
    n1 = (count - 1).astype(np.float64)
    v = np.zeros(count.shape)
    with np.errstate(all="ignore"):
        for c in range(3):
            m = rgba[..., c]
            e = sum_sq[c] / n - m * m
            e = np.where(e > 0, e, 0.0)
            v = v + e / n1
    return np.where(count < 2, 0.0, v)


def variance_scalar(rgba, count, sum_sq):
    rows, width = count.shape
    out = np.zeros((rows, width))
    for y in range(rows):
        for x in range(width):
            n = int(count[y, x])
            if n < 2:
                continue
            v = 0.0
            for c in range(3):
                m = float(rgba[y, x, c])
                e = float(sum_sq[c, y, x]) / float(n) - m * m
                e = e if e > 0 else 0.0
                v = v + e / float(n - 1)
            out[y, x] = v
    return out


def _shifted(rows, width, dy, dx):
    y0, y1, x0, x1 = max(0, -dy), min(rows, rows - dy), max(0, -dx), min(width, width - dx)
    if y0 >= y1 or x0 >= x1:
        return None, None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def vatrous_model(rgba, variance, ident, position, normal, iterations=4, k_colour=4.0, sigma_plane=0.25, normal_power_log2=5):
    """The definition, vectorised over the pixels and nothing else; returns (image, variance plane).  A tap that is not taken, and a
    pixel that is copied, leave their sums as they are (np.where)."""
    cur = np.array(rgba, dtype=np.float64, copy=True)
    vcur = np.array(variance, dtype=np.float64, copy=True)
    ident = np.asarray(ident)
    rows, width = ident.shape
    dims = position.shape[0]
    assert cur.shape == (rows, width, 4) and vcur.shape == (rows, width) and position.shape == normal.shape == (dims, rows, width)
    inv_p = 1.0 / (sigma_plane * sigma_plane)
    k2 = k_colour * k_colour
    with np.errstate(all="ignore"):
        for it in range(iterations):
            s = 1 << it
            gn, gd = np.zeros((rows, width)), np.zeros((rows, width))
            for b in range(3):
                for a in range(3):
                    g = G[b] * G[a]
                    p, q = _shifted(rows, width, b - 1, a - 1)
                    if p is None:
                        continue
                    same = ident[q] == ident[p]
                    gn[p] = np.where(same, gn[p] + g * vcur[q], gn[p])
                    gd[p] = np.where(same, gd[p] + g, gd[p])
            sp = k2 * (gn / gd)
            active = (ident != 0) & (sp > 0)
            num, den, vn = np.zeros((rows, width, 4)), np.zeros((rows, width)), np.zeros((rows, width))
            for j in range(5):
                for i in range(5):
                    h = H[j] * H[i]
                    dy, dx = (j - 2) * s, (i - 2) * s
                    if dy == 0 and dx == 0:
                        num = num + h * cur
                        den = den + h
                        vn = vn + (h * h) * vcur
                        continue
                    p, q = _shifted(rows, width, dy, dx)
                    if p is None:
                        continue
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
                    wc = 1.0 / (1.0 + cc / sp[p])
                    w = ((h * wn) * wp) * wc
                    take = (ident[q] == ident[p]) & (w > 0)
                    num[p] = np.where(take[..., None], num[p] + w[..., None] * cur[q], num[p])
                    den[p] = np.where(take, den[p] + w, den[p])
                    vn[p] = np.where(take, vn[p] + (w * w) * vcur[q], vn[p])
            cur = np.where(active[..., None], num / den[..., None], cur)
            vcur = np.where(active, vn / (den * den), vcur)
    return cur, vcur


def vatrous_scalar(rgba, variance, ident, position, normal, iterations=4, k_colour=4.0, sigma_plane=0.25, normal_power_log2=5):
    """The same text, one pixel and one tap at a time in Python floats (IEEE doubles)."""
    rows, width = ident.shape
    dims = position.shape[0]
    cur = [[[float(v) for v in rgba[y, x]] for x in range(width)] for y in range(rows)]
    vcur = [[float(variance[y, x]) for x in range(width)] for y in range(rows)]
    inv_p = 1.0 / (sigma_plane * sigma_plane)
    k2 = k_colour * k_colour
    for it in range(iterations):
        s = 1 << it
        nxt = [[None] * width for _ in range(rows)]
        vnxt = [[None] * width for _ in range(rows)]
        for y in range(rows):
            for x in range(width):
                me = int(ident[y, x])
                nxt[y][x], vnxt[y][x] = list(cur[y][x]), vcur[y][x]
                if me == 0:
                    continue
                gn = gd = 0.0
                for b in range(3):
                    for a in range(3):
                        ry, rx = y + b - 1, x + a - 1
                        g = G[b] * G[a]
                        if ry < 0 or ry >= rows or rx < 0 or rx >= width or int(ident[ry, rx]) != me:
                            continue
                        gn = gn + g * vcur[ry][rx]
                        gd = gd + g
                sp = k2 * (gn / gd)
                if not sp > 0:
                    continue
                num, den, vn = [0.0, 0.0, 0.0, 0.0], 0.0, 0.0
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
                            a_, b_ = cur[qy][qx], cur[y][x]
                            cc = ((a_[0] - b_[0]) * (a_[0] - b_[0]) + (a_[1] - b_[1]) * (a_[1] - b_[1])) + (a_[2] - b_[2]) * (a_[2] - b_[2])
                            wc = 1.0 / (1.0 + cc / sp)
                            w = ((h * wn) * wp) * wc
                            if not w > 0:
                                continue
                        for c in range(4):
                            num[c] = num[c] + w * cur[qy][qx][c]
                        den = den + w
                        vn = vn + (w * w) * vcur[qy][qx]
                nxt[y][x] = [n / den for n in num]
                vnxt[y][x] = vn / (den * den)
        cur, vcur = nxt, vnxt
    return np.array(cur, dtype=np.float64).reshape(rows, width, 4), np.array(vcur, dtype=np.float64).reshape(rows, width)


def variance_planes(rows, width, seed):
    """Seeded planes of uniform(0, 0.02) with one 8 x 8 block (clipped to the frame) at 0.0 and one pixel a NaN.  A frame of one pixel
    cannot hold all three: it gets three planes, one each."""
    plane = np.random.default_rng(seed).uniform(0.0, 0.02, (rows, width))
    if rows * width == 1:
        return [plane, np.zeros((1, 1)), np.full((1, 1), np.nan)]
    plane[rows // 3:rows // 3 + 8, width // 3:width // 3 + 8] = 0.0
    plane[rows - 1, width // 2] = np.nan
    return [plane]


# ---------------------------------------------------------------- CPU

def test_declared_bound_and_exported(tmp_path):
    """(CPU) the header declares every new entry point, hip.py binds it, the library exports it; ndt_vdenoise_params is 24 bytes to a
    C compiler and to ctypes; the ABI version is still 3."""
    with open(os.path.join(ROOT, "include", "ndt_hip.h")) as f:
        header = f.read()
    lib = nh.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in nh.API_SYMBOLS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert lib.ndt_hip_abi_version() == 3 and "#define NDT_HIP_ABI_VERSION 3" in header
    for method in ("render_moments", "sample_variance", "vdenoise", "render_vdenoised"):
        assert callable(getattr(nh.NdtHip, method, None)), method
    assert C.sizeof(nh.VDenoiseParams) == 24
    d = nh.vdenoise_params()
    assert (d.iterations, d.normal_power_log2, d.k_colour, d.sigma_plane) == (4, 5, 4.0, 0.25)
    assert (nh.VDenoiseParams.iterations.offset, nh.VDenoiseParams.normal_power_log2.offset, nh.VDenoiseParams.k_colour.offset,
            nh.VDenoiseParams.sigma_plane.offset) == (0, 4, 8, 16)
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ndt_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(ndt_vdenoise_params), offsetof(ndt_vdenoise_params, iterations),\n'
                   '    offsetof(ndt_vdenoise_params, normal_power_log2), offsetof(ndt_vdenoise_params, k_colour),\n'
                   '    offsetof(ndt_vdenoise_params, sigma_plane)); return 0; }\n')
    exe = str(tmp_path / "size")
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["24", "0", "4", "8", "16"]


@pytest.mark.parametrize("rows,width,dims", [(1, 1, 3), (1, 11, 4), (9, 7, 3), (6, 13, 7), (11, 5, 12)])
def test_the_vectorised_models_are_the_scalar_text(rows, width, dims):
    """(CPU) bit for bit, image and plane, at 1, 3 and 5 iterations and other parameters than the defaults, on variances with a block
    of zeros and a NaN; and k_sample_variance's model on counts 0, 1, 2, 7 with sums that make e negative."""
    rgba, ident, position, normal = random_inputs(rows, width, dims, 100 * rows + width)
    for variance in variance_planes(rows, width, 7 * rows + width):
        for kw in ({"iterations": 1}, {"iterations": 3, "k_colour": 1.5}, {"iterations": 5, "sigma_plane": 0.4, "normal_power_log2": 2},
                   {"iterations": 2, "normal_power_log2": 0, "k_colour": 0.5}):
            want, vwant = vatrous_scalar(rgba, variance, ident, position, normal, **kw)
            got, vgot = vatrous_model(rgba, variance, ident, position, normal, **kw)
            assert same_bits(got, want) and same_bits(vgot, vwant), kw
            assert same_bits(got[ident == 0], rgba[ident == 0]) and same_bits(vgot[ident == 0], variance[ident == 0])
            still = (variance == 0) | np.isnan(variance)
            if rows * width > 1:
                assert not same_bits(got[ident != 0], rgba[ident != 0])
                assert same_bits(got[rows - 1, width // 2], rgba[rows - 1, width // 2])         # the NaN variance: copied
            elif still.all():
                assert same_bits(got, rgba) and same_bits(vgot, variance)
    rng = np.random.default_rng(rows * 31 + width)
    count = rng.choice(np.array([0, 1, 2, 7], dtype=np.int32), (rows, width))
    sum_sq = np.stack([count * rgba[..., c] * rgba[..., c] * rng.choice([1.0 - 1e-15, 1.0, 1.5], (rows, width)) for c in range(3)])
    assert same_bits(variance_model(rgba, count, sum_sq), variance_scalar(rgba, count, sum_sq))


def noisy_half_frame():
    """synthetic_frame(37, 67) with a shadow edge the guides cannot see (the plane's columns < 20 at 0.4), and four samples a pixel
    whose noise has sigma 0.16 in columns >= 33 and none elsewhere: the frame is their mean, with its moments and variance."""
    clean, _, ident, position, normal = synthetic_frame(37, 67)
    clean = clean.copy()
    shadow = ident == 1
    shadow[:, 20:] = False
    clean[shadow, :3] *= 0.4
    sigma = np.where(np.arange(67) >= 33, 0.16, 0.0)
    s = clean[None, ..., :3] + np.random.default_rng(11).normal(0.0, 1.0, (4, 37, 67, 3)) * sigma[None, None, :, None]
    frame = clean.copy()
    frame[..., :3] = (((s[0] + s[1]) + s[2]) + s[3]) / 4.0
    sum_sq = np.ascontiguousarray(np.moveaxis(((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) + s[3] * s[3], -1, 0))
    count = np.full((37, 67), 4, dtype=np.int32)
    return clean, frame, variance_model(frame, count, sum_sq), ident, position, normal


def test_the_model_filters_the_noisy_side_and_keeps_the_converged_side_to_the_bit():
    """(CPU) the noisy object pixels of columns >= 35 (793) gain at least 4 x in mean squared error at k_colour 1, 2, 4 and 3
    iterations, and at 4 iterations with k = 4; the converged object pixels of columns < 28 (663) keep their bits at every one of
    those settings -- which the constant-width filter at its defaults does not; the propagated variance of the noisy pixels falls
    below a tenth; nothing crosses an id boundary, a NaN colour stays one pixel, a NaN variance leaves its pixel copied."""
    clean, frame, variance, ident, position, normal = noisy_half_frame()
    cols = np.broadcast_to(np.arange(67), (37, 67))
    noisy, quiet = (ident != 0) & (cols >= 35), (ident != 0) & (cols < 28)
    assert noisy.sum() == 793 and quiet.sum() == 663
    assert (variance[:, :33] == 0).all() and (variance[:, 33:] > 0).all()
    before = float(((frame[noisy][:, :3] - clean[noisy][:, :3]) ** 2).mean())
    assert 0.0060 < before < 0.0070                       # four samples of sigma 0.16: 0.16 ** 2 / 4
    out = None
    for k, iterations in ((1.0, 3), (2.0, 3), (4.0, 3), (4.0, 4)):
        out, vout = vatrous_model(frame, variance, ident, position, normal, iterations=iterations, k_colour=k)
        after = float(((out[noisy][:, :3] - clean[noisy][:, :3]) ** 2).mean())
        share = float(vout[noisy].mean() / variance[noisy].mean())
        print("k_colour %g, %d iterations: MSE %.3g -> %.3g (%.1f x), propagated variance %.3f of the input's" % (k, iterations, before, after, before / after, share))
        assert after * 4.0 <= before
        assert same_bits(out[quiet], frame[quiet]) and same_bits(vout[quiet], variance[quiet])
        assert share < 0.1
        assert same_bits(out[ident == 0], frame[ident == 0])
    old = atrous_model(frame, ident, position, normal, iterations=3)
    old_mse = float(((old[quiet][:, :3] - clean[quiet][:, :3]) ** 2).mean())
    print("the constant-width filter on the converged pixels: MSE %.3g (the frame's: 0)" % old_mse)
    assert not same_bits(old[quiet], frame[quiet]) and old_mse > 0 and same_bits(frame[quiet], clean[quiet])
    # nothing crosses an id boundary: the sphere with other colours and variances changes no pixel of the plane
    kw = dict(iterations=4, k_colour=4.0)
    other, vother = frame.copy(), variance.copy()
    other[ident == 2, :3] += 5.0
    vother[ident == 2] *= 3.0
    out2, vout2 = vatrous_model(other, vother, ident, position, normal, **kw)
    assert same_bits(out2[ident == 1], out[ident == 1]) and same_bits(vout2[ident == 1], vout[ident == 1])
    assert not same_bits(out2[ident == 2], out[ident == 2])
    # one NaN colour among noisy pixels: its own centre tap keeps it a NaN; every other pixel drops the tap and stays finite
    y, x = 30, 50
    assert ident[y, x] != 0 and variance[y, x] > 0
    poisoned = frame.copy()
    poisoned[y, x, 1] = np.nan
    out3, _ = vatrous_model(poisoned, variance, ident, position, normal, **kw)
    bad = np.isnan(out3).any(axis=2)
    assert bad[y, x] and bad.sum() == 1
    # one NaN variance: the pixel is copied (so are the neighbours whose local variance it enters), the image stays finite
    vbad = variance.copy()
    vbad[y, x] = np.nan
    out4, vout4 = vatrous_model(frame, vbad, ident, position, normal, **kw)
    assert same_bits(out4[y, x], frame[y, x]) and np.isnan(vout4[y, x]) and np.isfinite(out4).all()


def _run_driver(cwd, *flags, scene="builtin:yaml", dims=4, size="16x9"):
    assert os.path.exists(DRIVER), "ndt_amd/host/ndt_hip is not built"
    os.makedirs(str(cwd), exist_ok=True)
    return subprocess.run([DRIVER, "-s", scene, "-d", str(dims), "-f", "0", "-r", size, "-l", "6"] + list(flags),
                          capture_output=True, text=True, cwd=str(cwd))


def test_driver_refuses_what_vdenoise_does_not_go_with_by_name(tmp_path):
    """(CPU) every refusal ends the run non-zero with one line on stderr that names the cause, before a scene is loaded or a device
    asked for: nothing is written."""
    for flags, words in ((["--vdenoise", "-a", "20,3"], ("--vdenoise", "-a")),
                         (["--vdenoise", "2", "-m", "s"], ("--vdenoise", "-m s")),
                         (["--vdenoise", "-m", "o"], ("--vdenoise", "-m o")),
                         (["--vdenoise", "-m", "a"], ("--vdenoise", "-m a")),
                         (["--vdenoise", "-m", "h"], ("--vdenoise", "-m h")),
                         (["--vdenoise", "3", "-g", "2"], ("--vdenoise", "-g 2")),
                         (["--vdenoise", "--ssaa", "2"], ("--vdenoise", "--ssaa 2")),
                         (["--vdenoise", "--apng"], ("--vdenoise", "--apng")),
                         (["--vdenoise", "--png", "--deflate", "gpu", "--png16"], ("--vdenoise", "--png16")),
                         (["--vdenoise", "-z"], ("--vdenoise", "-z")),
                         (["--vdenoise", "--exr", "--exr-aov", "all"], ("--vdenoise", "--exr-aov")),
                         (["--vdenoise", "--denoise"], ("--vdenoise", "--denoise", "take one")),
                         (["--denoise", "2", "--vdenoise", "3"], ("--vdenoise", "--denoise", "take one")),
                         (["--vdenoise", "--ao"], ("--ao", "--vdenoise")),
                         (["--vdenoise-colour", "2"], ("--vdenoise-colour", "needs --vdenoise")),
                         (["--vdenoise-plane", "0.3", "--png"], ("--vdenoise-plane", "needs --vdenoise")),
                         (["--vdenoise-normal", "4", "--jpeg"], ("--vdenoise-normal", "needs --vdenoise")),
                         (["--denoise", "--vdenoise-colour", "2"], ("--vdenoise-colour", "needs --vdenoise")),
                         (["--vdenoise", "0"], ("--vdenoise", "1 .. 6", "'0'")),
                         (["--vdenoise", "7"], ("--vdenoise", "1 .. 6", "'7'")),
                         (["--vdenoise=x"], ("--vdenoise", "1 .. 6", "'x'")),
                         (["--vdenoise", "--vdenoise-colour", "0"], ("--vdenoise-colour", "above 0")),
                         (["--vdenoise", "--vdenoise-colour", "nan"], ("--vdenoise-colour", "above 0")),
                         (["--vdenoise", "--vdenoise-plane", "-1"], ("--vdenoise-plane", "above 0")),
                         (["--vdenoise", "--vdenoise-plane", "inf"], ("--vdenoise-plane", "above 0")),
                         (["--vdenoise", "--vdenoise-normal", "9"], ("--vdenoise-normal", "0 .. 8")),
                         (["--sample-cap", "0"], ("--sample-cap", "'0'")),
                         (["--sample-cap", "-3", "-n", "2"], ("--sample-cap", "'-3'")),
                         (["--sample-cap", "x"], ("--sample-cap", "'x'"))):
        r = _run_driver(tmp_path, *flags)
        assert r.returncode != 0, flags
        for w in words:
            assert w in r.stderr, (flags, r.stderr)
        assert len(r.stderr.strip().splitlines()) == 1, (flags, r.stderr)       # the refusal and nothing else: no device was asked for
    assert not [p for p in tmp_path.rglob("*") if p.is_file()]
    usage = _run_driver(tmp_path, "-h")
    assert usage.returncode == 0
    for flag in ("--sample-cap C", "--vdenoise [1..6]", "--vdenoise-colour X", "--vdenoise-plane X", "--vdenoise-normal 0..8"):
        assert flag in usage.stderr, flag


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


class VarianceFrame(DeviceFrame):
    """... and the variance plane, with the same room behind it and behind the plane that comes back"""

    def __init__(self, rgba, ident, position, normal, variance):
        super().__init__(rgba, ident, position, normal)
        torch = self.torch
        self.vn = variance.size
        self.variance = torch.from_numpy(np.concatenate([variance.reshape(-1), np.full(self.GUARD, -7.0)])).cuda()
        self.vout = torch.full((self.vn + self.GUARD,), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

    def plane(self, t):
        host = t.cpu().numpy()
        assert (host[self.vn:] == -7.0).all(), "the filter wrote behind its plane"
        return host[:self.vn].reshape(self.shape[:2])


FRAMES = [(1, 1), (1, 70), (37, 67), (33, 5), (19, 130)]        # rows x width


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [3, 4, 7, 12])
@pytest.mark.parametrize("rows,width", FRAMES)
def test_the_filter_alone_is_the_model_bit_for_bit(gpu, rows, width, dims):
    """ndt_hip_vdenoise_device at 1, 3 and 6 iterations: a lone pixel, a single row, a frame narrower than the stencil, a width that
    is no multiple of 64, the largest N; a variance plane with zeros and a NaN.  Image and plane are the model's, the guards behind
    both survive, the inputs are left as they were."""
    rgba, ident, position, normal = random_inputs(rows, width, dims, 1000 * rows + 10 * width + dims)
    for variance in variance_planes(rows, width, 3 * rows + width + dims):
        dev = VarianceFrame(rgba, ident, position, normal, variance)
        for iterations, extra in ((1, {}), (3, {"k_colour": 1.5, "normal_power_log2": 3}), (6, {"sigma_plane": 0.4})):
            want, vwant = vatrous_model(rgba, variance, ident, position, normal, iterations=iterations, **extra)
            gpu.vdenoise(dev.rgba.data_ptr(), dev.planes, dev.variance.data_ptr(), dims, width, rows, dev.out.data_ptr(), dev.vout.data_ptr(),
                         iterations=iterations, **extra)
            got, vgot = dev.image(dev.out), dev.plane(dev.vout)
            differ = int((bits(got) != bits(want)).sum()) + int((bits(vgot) != bits(vwant)).sum())
            print("%d x %d, N = %d, %d iterations: %d of %d doubles differ from the model" % (rows, width, dims, iterations, differ, want.size + vwant.size))
            assert differ == 0
            assert gpu.denoise_launches() == iterations and gpu.denoise_ms() >= 0.0
            assert same_bits(dev.image(dev.rgba), rgba) and same_bits(dev.plane(dev.variance), variance)
            assert same_bits(got[ident == 0], rgba[ident == 0])


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_in_place_and_without_a_plane_out_give_the_same_bits(gpu, iterations):
    rows, width, dims = 19, 130, 4
    rgba, ident, position, normal = random_inputs(rows, width, dims, 77)
    variance, = variance_planes(rows, width, 78)
    want, vwant = vatrous_model(rgba, variance, ident, position, normal, iterations=iterations)
    dev = VarianceFrame(rgba, ident, position, normal, variance)
    gpu.vdenoise(dev.rgba.data_ptr(), dev.planes, dev.variance.data_ptr(), dims, width, rows, dev.out.data_ptr(), None, iterations=iterations)
    assert same_bits(dev.image(dev.out), want) and gpu.denoise_launches() == iterations
    assert (dev.vout.cpu().numpy() == -7.0).all() and same_bits(dev.plane(dev.variance), variance)
    gpu.vdenoise(dev.rgba.data_ptr(), dev.planes, dev.variance.data_ptr(), dims, width, rows, None, dev.variance.data_ptr(), iterations=iterations)
    assert same_bits(dev.image(dev.rgba), want) and same_bits(dev.plane(dev.variance), vwant)
    assert gpu.denoise_launches() == iterations


@pytest.mark.gpu
def test_the_variance_kernel_is_its_model_bit_for_bit(gpu):
    """k_sample_variance on seeded counts in {0, 1, 2, 7} and sums that make e slightly negative, at a size that is no multiple of
    the workgroup; the guard behind the plane survives."""
    import torch
    rows, width = 19, 130
    rng = np.random.default_rng(19130)
    rgba = rng.uniform(0.0, 2.0, (rows, width, 4))
    count = rng.choice(np.array([0, 1, 2, 7], dtype=np.int32), (rows, width))
    sum_sq = np.stack([count * rgba[..., c] * rgba[..., c] * rng.choice([1.0 - 1e-15, 1.0, 1.0 + 1e-15, 1.5], (rows, width)) for c in range(3)])
    want = variance_model(rgba, count, sum_sq)
    assert ((count >= 2) & (want == 0)).any() and (want > 0).any() and (want[count < 2] == 0).all()
    d_rgba, d_count, d_sum_sq = torch.from_numpy(rgba).cuda(), torch.from_numpy(count).cuda(), torch.from_numpy(sum_sq).cuda()
    out = torch.full((rows * width + 64,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.sample_variance(d_rgba.data_ptr(), d_count.data_ptr(), d_sum_sq.data_ptr(), width, rows, out.data_ptr())
    host = out.cpu().numpy()
    assert (host[rows * width:] == -7.0).all()
    assert same_bits(host[:rows * width].reshape(rows, width), want)


def device_variance(gpu, rgba, count, sum_sq):
    import torch
    rows, width = count.shape
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rgba, count, sum_sq)]
    out = torch.zeros(rows * width, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.sample_variance(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), width, rows, out.data_ptr())
    return out.cpu().numpy().reshape(rows, width)


CAPPED = {"al_zoo4d": ("al_zoo4d", 0), "al_zoo4d_levels": ("al_zoo4d", 1), "al_zoo4d_stream": ("al_zoo4d", 2), "al_zoo3d_dof_n3": ("al_zoo3d_dof_n3", 0)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CAPPED))
def test_the_cap_bounds_the_loop_and_the_moments_are_the_samples(gpu, case):
    """33 x 17, samples = 2.  Without a cap (0, or one nothing reaches) the moments' frame is render's and the counts add up to
    aa_samples; cap 1 is one sample a pixel in one pass; cap 2 adds exactly the second sample; cap 5 leaves every pixel that ends
    earlier by itself as it was; the option reset, the plain render is what it was."""
    name, pipeline = CAPPED[case]
    g = golden(name)
    w, h, samples = 33, 17, 2
    pixels = w * h
    try:
        gpu.set_option("pipeline", pipeline)
        gpu.upload_scene(g.scene)
        plain, plain_st = gpu.render(w, h, g.depth, samples=samples)
        free = None
        for cap in (0, 10000):
            gpu.set_option("sample_cap", cap)
            fb, count, sum_sq, st = gpu.render_moments(w, h, g.depth, samples=samples)
            assert same_bits(fb, plain) and same_bits(gpu.render(w, h, g.depth, samples=samples)[0], plain)
            assert int(count.sum()) == st.aa_samples == plain_st.aa_samples and (count >= samples).all()
            assert (sum_sq >= 0).all() and (sum_sq > 0).any()
            free = count if free is None else free
            assert np.array_equal(count, free)
        print("%s: uncapped, %.2f samples a pixel, %d to %d" % (case, free.mean(), free.min(), free.max()))
        assert free.max() > 5, "the scene ends every pixel within 5 samples: the cap-5 case below tests nothing"
        gpu.set_option("sample_cap", 1)
        f1, count, sum_sq, st = gpu.render_moments(w, h, g.depth, samples=samples)
        assert (count == 1).all() and st.aa_samples == pixels and pixels <= st.rays_primary < 2 * pixels          # one pass of one sample
        assert same_bits(sum_sq, np.moveaxis(f1[..., :3] * f1[..., :3], -1, 0))
        assert same_bits(gpu.render(w, h, g.depth, samples=samples)[0], f1)
        assert (device_variance(gpu, f1, count, sum_sq) == 0).all()
        gpu.set_option("sample_cap", 2)
        f2, count, sum_sq, st = gpu.render_moments(w, h, g.depth, samples=samples)
        assert (count == 2).all() and st.aa_samples == 2 * pixels and 2 * pixels <= st.rays_primary < 3 * pixels  # one pass of two
        c1 = 2.0 * f2[..., :3] - f1[..., :3]
        a, b = np.moveaxis(f1[..., :3] * f1[..., :3], -1, 0), np.moveaxis(c1 * c1, -1, 0)
        tol = 16.0 * 2.0 ** -52 * np.maximum(1.0, np.maximum(a, b).max(axis=0))
        err = np.abs(sum_sq - (a + b)).max(axis=0)
        got_v = device_variance(gpu, f2, count, sum_sq)
        verr = np.abs(got_v - variance_model(f2, count, a + b))
        print("%s: cap 2: sum_sq off by at most %.3g, the variance by %.3g (allowed: %.3g)" % (case, err.max(), verr.max(), tol.min()))
        assert (err <= tol).all() and (verr <= tol).all()
        assert same_bits(got_v, variance_model(f2, count, sum_sq)) and (got_v > 0).any()
        assert not same_bits(f2, f1)
        # cap 5, and a cap in the middle of this frame's own counts, so that pixels on both sides of it exist
        middle = min(int(np.median(free)), int(free.max()) - 1)
        assert free.min() <= middle
        for cap in (5, middle):
            gpu.set_option("sample_cap", cap)
            fc, count, _, st = gpu.render_moments(w, h, g.depth, samples=samples)
            assert count.min() >= 2 and count.max() == cap and int(count.sum()) == st.aa_samples
            early = free <= cap
            print("%s: cap %d: %d pixels end earlier by themselves, %d are cut" % (case, cap, int(early.sum()), int((~early).sum())))
            assert np.array_equal(count[early], free[early]) and (count[~early] == cap).all()
            assert same_bits(fc[early], plain[early])
            assert early.any() or cap == 5
        gpu.set_option("sample_cap", 0)
        assert same_bits(gpu.render(w, h, g.depth, samples=samples)[0], plain)
        with pytest.raises(nh.NdtHipError, match="sample_cap") as e:
            gpu.set_option("sample_cap", -1)
        assert e.value.code == NDT_E_INVALID
    finally:
        gpu.set_option("sample_cap", 0)
        gpu.set_option("pipeline", 0)


@pytest.mark.gpu
def test_a_frame_without_the_loop_has_one_sample_a_pixel(gpu):
    g = golden("zoo12d")
    w, h = 33, 17
    gpu.upload_scene(g.scene)
    plain, _ = gpu.render(w, h, g.depth)
    fb, count, sum_sq, _ = gpu.render_moments(w, h, g.depth)
    assert same_bits(fb, plain) and (count == 1).all()
    assert same_bits(sum_sq, np.moveaxis(fb[..., :3] * fb[..., :3], -1, 0))
    # a row shard and side by side are fine
    part, count, _, _ = gpu.render_moments(w, h, g.depth, row_begin=1, row_step=3)
    assert same_bits(part, gpu.render(w, h, g.depth, row_begin=1, row_step=3)[0]) and count.shape == part.shape[:2]


END_TO_END = {"al_zoo4d": ("al_zoo4d", 4, 0), "al_zoo3d_dof_n3": ("al_zoo3d_dof_n3", 4, 0), "zoo12d_n1": ("zoo12d", 1, 0),
              "al_zoo4d_levels": ("al_zoo4d", 4, 1), "al_zoo4d_stream": ("al_zoo4d", 4, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(END_TO_END))
def test_a_vdenoised_frame_is_the_model_of_the_moments_and_the_features(gpu, case):
    """render_vdenoised(samples=4) under sample_cap 4 equals the model applied to render_moments and render_features of the same
    context, bit for bit, at 33 x 17, under every pipeline for the 4-D area-light scene; a frame of one sample a pixel has no
    variance and comes back as rendered."""
    name, samples, pipeline = END_TO_END[case]
    g = golden(name)
    w, h = 33, 17
    try:
        gpu.set_option("pipeline", pipeline)
        gpu.set_option("sample_cap", 4)
        gpu.upload_scene(g.scene)
        fb, count, sum_sq, _ = gpu.render_moments(w, h, g.depth, samples=samples)
        f = gpu.render_features(w, h, g.depth)
        assert (f["id"] > 0).any() and (count == samples).all()
        variance = variance_model(fb, count, sum_sq)
        want = None
        for kw in ({}, {"iterations": 2, "k_colour": 1.5, "sigma_plane": 0.3, "normal_power_log2": 3}):
            want, _ = vatrous_model(fb, variance, f["id"], f["position"], f["normal"], **kw)
            got, st = gpu.render_vdenoised(w, h, g.depth, samples=samples, **kw)
            differ = int((bits(got) != bits(want)).sum())
            print("%s %r: %d of %d doubles differ from the model; %d of %d pixels have variance" % (case, kw, differ, want.size, int((variance > 0).sum()), variance.size))
            assert differ == 0
            assert gpu.denoise_launches() == 5 + kw.get("iterations", 4) and gpu.features_launches() == 4
            assert st.rays_primary > 0 and st.aa_samples == (samples * w * h if samples > 1 else 0)
        if samples > 1:
            assert (variance > 0).any() and not same_bits(want, fb)
        else:
            assert (variance == 0).all() and same_bits(want, fb)
    finally:
        gpu.set_option("sample_cap", 0)
        gpu.set_option("pipeline", 0)


@pytest.mark.gpu
def test_the_sinks_take_the_models_doubles_and_later_calls_are_what_they_were(gpu, oracle):
    """The device sink leaves its guard intact; rgba8 is oracle.quantize of the model's frame, the PNG decodes to exactly that, the
    JPEG is ndt_hip_encode_jpeg of those pixels and the EXR ndt_hip_encode_exr of the model's doubles; a later plain render, depth
    map, feature pass and render_denoised give the bits they gave before."""
    import torch
    g = golden("al_zoo4d")
    w, h, samples = 33, 17, 4
    gpu.upload_scene(g.scene)
    before_fb, before_dm, _ = gpu.render(w, h, g.depth, depth_map=True)
    before_sampled, _ = gpu.render(w, h, g.depth, samples=2)
    before_f = gpu.render_features(w, h, g.depth, rays=True)
    before_old, _ = gpu.render_denoised(w, h, g.depth, samples=2)
    try:
        gpu.set_option("sample_cap", 4)
        fb, count, sum_sq, _ = gpu.render_moments(w, h, g.depth, samples=samples)
        f = gpu.render_features(w, h, g.depth)
        kw = dict(samples=samples, iterations=3, k_colour=2.0)
        want, _ = vatrous_model(fb, variance_model(fb, count, sum_sq), f["id"], f["position"], f["normal"], iterations=3, k_colour=2.0)
        want8 = oracle.quantize(want)
        assert not np.array_equal(want8, oracle.quantize(fb))
        out = torch.full((w * h * 4 + 64,), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        gpu.render_vdenoised(w, h, g.depth, sink="device", d_rgba_ptr=out.data_ptr(), **kw)
        host = out.cpu().numpy()
        assert (host[w * h * 4:] == -7.0).all() and same_bits(host[:w * h * 4].reshape(h, w, 4), want)
        got8, _ = gpu.render_vdenoised(w, h, g.depth, sink="rgba8", **kw)
        assert np.array_equal(got8, want8) and gpu.denoise_launches() == 8
        png, _ = gpu.render_vdenoised(w, h, g.depth, sink="png", **kw)
        assert np.array_equal(read_png(png), want8) and gpu.png_stats.png_bytes == len(png)
        for quality, sampling in ((95, "420"), (50, "444")):
            jpg, _ = gpu.render_vdenoised(w, h, g.depth, sink="jpeg", quality=quality, sampling=sampling, **kw)
            assert jpg == gpu.encode_jpeg(want8, quality, sampling)
        for pixel in ("half", "float"):
            exr, _ = gpu.render_vdenoised(w, h, g.depth, sink="exr", pixel=pixel, **kw)
            assert exr == gpu.encode_exr(want, pixel=pixel)
    finally:
        gpu.set_option("sample_cap", 0)
    fb2, dm2, _ = gpu.render(w, h, g.depth, depth_map=True)
    assert same_bits(fb2, before_fb) and same_bits(dm2, before_dm)
    assert same_bits(gpu.render(w, h, g.depth, samples=2)[0], before_sampled)
    f2 = gpu.render_features(w, h, g.depth, rays=True)
    assert np.array_equal(f2["id"], before_f["id"]) and all(same_bits(f2[k], before_f[k]) for k in ("position", "normal", "ray_o", "ray_v"))
    assert same_bits(gpu.render_denoised(w, h, g.depth, samples=2)[0], before_old) and gpu.denoise_launches() == 8


@pytest.mark.gpu
def test_the_library_refuses_by_code_and_cause_and_writes_nothing(gpu):
    import torch
    lib = gpu.lib
    g = golden("al_zoo4d")
    w, h = 33, 17
    gpu.upload_scene(g.scene)
    ok = nh.vdenoise_params()
    entries = (("ndt_hip_render_vdenoised", lambda p, vp, buf: lib.ndt_hip_render_vdenoised(gpu.ctx, C.byref(p), C.byref(vp), buf.ctypes.data, None)),
               ("ndt_hip_render_vdenoised_rgba8", lambda p, vp, buf: lib.ndt_hip_render_vdenoised_rgba8(gpu.ctx, C.byref(p), C.byref(vp), buf.ctypes.data, None)),
               ("ndt_hip_render_vdenoised_png", lambda p, vp, buf: lib.ndt_hip_render_vdenoised_png(gpu.ctx, C.byref(p), C.byref(vp), buf.ctypes.data, buf.size, None, None)),
               ("ndt_hip_render_vdenoised_jpeg", lambda p, vp, buf: lib.ndt_hip_render_vdenoised_jpeg(gpu.ctx, C.byref(p), C.byref(vp), None, buf.ctypes.data, buf.size, None, None)),
               ("ndt_hip_render_vdenoised_exr", lambda p, vp, buf: lib.ndt_hip_render_vdenoised_exr(gpu.ctx, C.byref(p), C.byref(vp), None, buf.ctypes.data, buf.size, None, None)))
    frames = [({"aa": (20, 3)}, ok, NDT_E_UNSUPPORTED, "recursive_aa")]
    frames += [({"stereo": m}, ok, NDT_E_UNSUPPORTED, "stereo mode %d" % m) for m in (1, 2, 3, 4)]
    frames += [({"row_begin": 1, "row_step": 3}, ok, NDT_E_UNSUPPORTED, "row shard"), ({"row_step": 2}, ok, NDT_E_UNSUPPORTED, "row shard")]
    frames += [({}, nh.VDenoiseParams(k, 5, 4.0, 0.25), NDT_E_INVALID, "%d iterations" % k) for k in (0, 7)]
    frames += [({}, nh.VDenoiseParams(4, 5, s, 0.25), NDT_E_INVALID, "k_colour") for s in (0.0, -4.0, math.nan, math.inf)]
    frames += [({}, nh.VDenoiseParams(4, 5, 4.0, s), NDT_E_INVALID, "sigma_plane") for s in (0.0, -0.25, math.nan, math.inf)]
    frames += [({}, nh.VDenoiseParams(4, 9, 4.0, 0.25), NDT_E_INVALID, "normal_power_log2 9")]
    for kw, vp, code, word in frames:
        p = gpu.params(w, h, g.depth, samples=2, **kw)
        for name, call in entries:
            buf = np.full(w * h * 32, 0xA5, dtype=np.uint8)
            assert call(p, vp, buf) == code, (name, kw, word)
            err = lib.ndt_hip_last_error().decode()
            assert word in err and name in err, (name, err)
            assert (buf == 0xA5).all()
    # the device sink and the moments: what they refuse by name, on buffers that stay as they were
    d_buf = torch.full((w * h * 8,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for kw, word in (({"aa": (20, 3)}, "recursive_aa"), ({"stereo": 3}, "NDT_STEREO_ANAGLYPH"), ({"stereo": 4}, "NDT_STEREO_HIDEF")):
        p = gpu.params(w, h, g.depth, samples=2, **kw)
        rgba, count, sum_sq = np.full((h, w, 4), -7.0), np.full((h, w), -7, dtype=np.int32), np.full((3, h, w), -7.0)
        assert lib.ndt_hip_render_moments(gpu.ctx, C.byref(p), rgba.ctypes.data, count.ctypes.data, sum_sq.ctypes.data, None) == NDT_E_UNSUPPORTED
        err = lib.ndt_hip_last_error().decode()
        assert word in err and "ndt_hip_render_moments" in err, err
        assert (rgba == -7.0).all() and (count == -7).all() and (sum_sq == -7.0).all()
        base = d_buf.data_ptr()
        assert lib.ndt_hip_render_moments_device(gpu.ctx, C.byref(p), C.c_void_p(base), C.c_void_p(base + w * h * 32), C.c_void_p(base + w * h * 40),
                                                 None) == NDT_E_UNSUPPORTED
        err = lib.ndt_hip_last_error().decode()
        assert word in err and "ndt_hip_render_moments_device" in err, err
        assert lib.ndt_hip_render_vdenoised_device(gpu.ctx, C.byref(p), C.byref(ok), C.c_void_p(base), None) == NDT_E_UNSUPPORTED
        assert "ndt_hip_render_vdenoised_device" in lib.ndt_hip_last_error().decode()
    p = gpu.params(w, h, g.depth, samples=2)
    assert lib.ndt_hip_render_vdenoised_device(gpu.ctx, C.byref(p), C.byref(ok), C.c_void_p(d_buf.data_ptr() + 8), None) == NDT_E_INVALID
    assert "misaligned" in lib.ndt_hip_last_error().decode()
    assert lib.ndt_hip_render_moments_device(gpu.ctx, C.byref(p), C.c_void_p(d_buf.data_ptr()), None, C.c_void_p(d_buf.data_ptr()), None) == NDT_E_INVALID
    assert "NULL" in lib.ndt_hip_last_error().decode()
    # the filter alone and the variance kernel: the same parameters, a NULL plane, a misaligned one, dimensions it is not built for
    rgba, ident, position, normal = random_inputs(9, 16, 4, 5)
    variance, = variance_planes(9, 16, 6)
    dev = VarianceFrame(rgba, ident, position, normal, variance)

    def alone(vp=ok, dims=4, width=16, rows=9, src=None, dst=None, var="given", vdst="given", **planes):
        pl = dict(dev.planes, **planes)
        fp = nh.FeaturePlanes(pl["id"], pl["position"], pl["normal"], None, None)
        var = dev.variance.data_ptr() if var == "given" else var
        vdst = dev.vout.data_ptr() if vdst == "given" else vdst
        return lib.ndt_hip_vdenoise_device(gpu.ctx, C.c_void_p(dev.rgba.data_ptr() if src is None else src), C.byref(fp), C.c_void_p(var) if var else None,
                                           dims, width, rows, C.byref(vp), C.c_void_p(dev.out.data_ptr() if dst is None else dst),
                                           C.c_void_p(vdst) if vdst else None)

    for call, word in ((lambda: alone(nh.VDenoiseParams(0, 5, 4.0, 0.25)), "0 iterations"), (lambda: alone(nh.VDenoiseParams(7, 5, 4.0, 0.25)), "7 iterations"),
                       (lambda: alone(nh.VDenoiseParams(4, 5, 0.0, 0.25)), "k_colour"), (lambda: alone(nh.VDenoiseParams(4, 5, -1.0, 0.25)), "k_colour"),
                       (lambda: alone(nh.VDenoiseParams(4, 5, math.nan, 0.25)), "k_colour"), (lambda: alone(nh.VDenoiseParams(4, 5, 4.0, math.nan)), "sigma_plane"),
                       (lambda: alone(nh.VDenoiseParams(4, 9, 4.0, 0.25)), "normal_power_log2 9"), (lambda: alone(nh.VDenoiseParams(4, -1, 4.0, 0.25)), "normal_power_log2 -1"),
                       (lambda: alone(id=None), "NULL plane"), (lambda: alone(position=None), "NULL plane"), (lambda: alone(normal=None), "NULL plane"),
                       (lambda: alone(var=None), "NULL argument"),
                       (lambda: alone(position=dev.planes["position"] + 4), "misaligned"), (lambda: alone(id=dev.planes["id"] + 2), "misaligned"),
                       (lambda: alone(dst=dev.out.data_ptr() + 8), "misaligned"), (lambda: alone(src=dev.rgba.data_ptr() + 8), "misaligned"),
                       (lambda: alone(var=dev.variance.data_ptr() + 4), "misaligned"), (lambda: alone(vdst=dev.vout.data_ptr() + 4), "misaligned"),
                       (lambda: alone(dims=2), "2 dimensions"), (lambda: alone(dims=13), "13 dimensions"), (lambda: alone(width=0), "0 x 9"),
                       (lambda: alone(rows=-1), "16 x -1")):
        assert call() == NDT_E_INVALID, word
        err = lib.ndt_hip_last_error().decode()
        assert word in err and "ndt_hip_vdenoise_device" in err, err
    for args, word in (((dev.rgba.data_ptr(), dev.ident.data_ptr(), dev.position.data_ptr(), 0, 9, dev.vout.data_ptr()), "0 x 9"),
                       ((dev.rgba.data_ptr(), None, dev.position.data_ptr(), 16, 9, dev.vout.data_ptr()), "NULL argument"),
                       ((dev.rgba.data_ptr(), dev.ident.data_ptr() + 2, dev.position.data_ptr(), 16, 9, dev.vout.data_ptr()), "misaligned"),
                       ((dev.rgba.data_ptr(), dev.ident.data_ptr(), dev.position.data_ptr(), 16, 9, dev.vout.data_ptr() + 4), "misaligned")):
        assert lib.ndt_hip_sample_variance_device(gpu.ctx, *args) == NDT_E_INVALID, word
        err = lib.ndt_hip_last_error().decode()
        assert word in err and "ndt_hip_sample_variance_device" in err, err
    torch.cuda.synchronize()
    assert (dev.out.cpu().numpy() == -7.0).all() and (dev.vout.cpu().numpy() == -7.0).all() and (d_buf.cpu().numpy() == -7.0).all()
    assert same_bits(dev.image(dev.rgba), rgba) and same_bits(dev.plane(dev.variance), variance)
    with pytest.raises(nh.NdtHipError, match="row shard") as e:
        gpu.render_vdenoised(w, h, g.depth, row_begin=1, row_step=2)
    assert e.value.code == NDT_E_UNSUPPORTED


# ---------------------------------------------------------------- driver

@pytest.mark.gpu
def test_driver_vdenoises_says_so_and_leaves_the_librarys_file(tmp_path):
    """`ndt_hip --vdenoise 3 -n 4 --sample-cap 4 --png --deflate gpu` over both frames of the driver matrix's two-document scene at
    16 x 9: the line of each frame, and the files the library call makes for the scenes the driver loads.  The same run without the
    new flags says nothing of a denoiser and leaves the bytes it left before there was one."""
    recorder.write_scene(str(tmp_path / recorder.SCENE))
    flags = ["--vdenoise", "3", "-n", "4", "--sample-cap", "4", "--png", "--deflate", "gpu"]
    got = recorder.run_case(DRIVER, str(tmp_path / "vdenoised"), flags)
    assert got["stdout"].count("variance-guided denoise in 3 iterations on GPU 0 in 8 launches") == 2
    assert sum(line.startswith("compressed PNG of ") for line in got["stdout"]) == 2
    plain = recorder.run_case(DRIVER, str(tmp_path / "plain"), SAMPLED_PNG)
    with open(PARENT_RECORD) as f:
        rec = json.load(f)
    assert plain["files"] == rec["files"] and plain["stdout"] == rec["stdout"]
    assert sorted(got["files"]) == sorted(plain["files"])
    files = [next(p for p in got["files"] if p.endswith("_%04d.png" % k)) for k in (0, 1)]
    gpu = nh.NdtHip(0)
    try:
        gpu.set_option("sample_cap", 4)
        for k in (0, 1):
            dump = str(tmp_path / ("frame%d.ndtscene" % k))
            r = subprocess.run([DRIVER] + recorder.BASE[:-2] + ["-f", "%d:%d" % (k, k), "-u", str(tmp_path / recorder.SCENE), "--dump-scene", dump],
                               capture_output=True, text=True, cwd=str(tmp_path))
            assert r.returncode == 0, r.stderr[-2000:]
            gpu.upload_scene(load_scene(dump))
            want, st = gpu.render_vdenoised(16, 9, 6, sink="png", samples=4, iterations=3)
            assert gpu.denoise_launches() == 8 and st.aa_samples == 4 * 16 * 9
            with open(os.path.join(str(tmp_path / "vdenoised"), files[k]), "rb") as f:
                assert f.read() == want, files[k]
    finally:
        gpu.close()
    # the other sinks and the weights reach the library too: one frame each, each with its line
    for case, (k, more) in enumerate(((4, ["--vdenoise"]), (2, ["--vdenoise", "2", "--png"]), (5, ["--vdenoise=5", "--jpeg", "-n", "2", "--sample-cap", "2"]),
                                      (4, ["--vdenoise", "--exr", "--exr-pixel", "float", "-n", "3"]),
                                      (1, ["--vdenoise", "1", "--raw", "f.f64", "--vdenoise-colour", "1.5", "--vdenoise-plane", "0.3", "--vdenoise-normal", "2"]),
                                      (4, ["--vdenoise", "-n", "2", "--sample-cap", "8", "-j", "2", "--fit", "gpu", "--kd", "gpu"]))):
        one = recorder.run_case(DRIVER, str(tmp_path / ("case%d" % case)), more)
        assert one["stdout"].count("variance-guided denoise in %d iterations on GPU 0 in %d launches" % (k, 5 + k)) == 2, (more, one["stdout"])
        assert len(one["files"]) >= 2
    # the cap alone: another frame than the uncapped one, and no word of a denoiser
    capped = recorder.run_case(DRIVER, str(tmp_path / "capped"), ["--sample-cap", "2"] + SAMPLED_PNG)
    assert sorted(capped["files"]) == sorted(plain["files"]) and not any("denoise" in line for line in capped["stdout"])
    assert any(capped["files"][p]["sha256"] != plain["files"][p]["sha256"] for p in plain["files"])
