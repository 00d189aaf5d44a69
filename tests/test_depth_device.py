"""The depth map of `-z` finished on the device (ndt_depth.hip; `ndt_hip -z --depth gpu`).

The yardstick is numpy's restatement of what the driver does to the map on the host (ndt_main.c:render_frame: the range loop,
the stretch to 0 .. 1 of dbl_image_normalize, pixel_d2c on the grey image), applied to the map ndt_hip_render_depth returns --
and, for the fixtures that carry the compiled reference's map, to that.
"""
import ctypes as C
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, golden

from ndt_amd import hip as nh

NDT_E_INVALID, NDT_E_UNSUPPORTED, NDT_E_NOMEM = -1, -2, -4
HOST = os.path.join(ROOT, "ndt_amd", "host")
DRIVER = os.path.join(HOST, "ndt_hip")
ZOO_SRC = os.path.join(ROOT, "tests", "scenes", "parity_zoo.c")
NEW_SYMBOLS = ("ndt_hip_depth_rgba8_device", "ndt_hip_render_rgba8_depth", "ndt_hip_render_png_depth", "ndt_hip_depth_launches",
               "ndt_hip_depth_ms")


# ---------------------------------------------------------------- yardsticks

def pixel_d2c(x):
    """image.h:36-39: (unsigned char)(sqrt(clamp01(x)) * 255)"""
    m = np.where(1.0 < x, 1.0, x)
    m = np.where(0.0 > m, 0.0, m)
    return (np.sqrt(m) * 255).astype(np.uint8)


def finish_on_host(dm):
    """The driver's host path: lo / hi by `x < lo` / `x > hi` from element 0 (the minimum and the maximum of a map without
    NaN), v = hi > lo ? (d - lo) / (hi - lo) : 0, the image v, v, v, 1 through pixel_d2c.  Returns ((.., 4) uint8, lo, hi)."""
    dm = np.ascontiguousarray(dm, dtype=np.float64)
    assert np.isfinite(dm).all()
    lo, hi = dm.min(), dm.max()
    v = (dm - lo) / (hi - lo) if hi > lo else np.zeros_like(dm)
    out = np.empty(dm.shape + (4,), dtype=np.uint8)
    out[..., 0] = out[..., 1] = out[..., 2] = pixel_d2c(v)
    out[..., 3] = pixel_d2c(np.float64(1.0))
    return out, lo, hi


def read_png(data):
    """The pixels [h, w, 4] of an 8-bit RGBA PNG with filters 0 / 1 / 2 (the reader of tests/test_png_device.py: every chunk's
    CRC checked, the IDAT inflated by zlib, the filters undone in numpy)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, w, h, types = 8, b"", 0, 0, []
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert len(body) == n
        assert zlib.crc32(typ + body) == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0], typ
        types.append(typ)
        if typ == b"IHDR":
            w, h, bits, colour, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            assert (bits, colour, comp, filt, lace) == (8, 6, 0, 0, 0)
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    assert pos == len(data) and types[0] == b"IHDR" and types[-1] == b"IEND"
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8)
    assert raw.size == h * (1 + 4 * w)
    raw = raw.reshape(h, 1 + 4 * w)
    assert (raw[:, 0] <= 2).all()
    out = np.zeros((h, w, 4), dtype=np.uint8)
    for r in range(h):
        row = raw[r, 1:].reshape(w, 4)
        if raw[r, 0] == 1:
            row = np.cumsum(row, axis=0, dtype=np.uint8)
        elif raw[r, 0] == 2 and r > 0:
            row = row + out[r - 1]
        out[r] = row
    return out


def read_ppm(data):
    magic, size, maxval, body = data.split(b"\n", 3)
    w, h = (int(x) for x in size.split())
    assert magic == b"P6" and maxval == b"255" and len(body) == w * h * 3
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 3)


def test_the_yardstick_is_the_drivers_loop():
    """(CPU) the vectorised restatement against the loop as the driver has it, element by element in Python floats."""
    rng = np.random.default_rng(5)
    dm = np.where(rng.random(300) < 0.3, 0.0, 1.0 / rng.uniform(0.5, 40.0, 300))
    lo = hi = dm[0]
    for x in dm:
        if x < lo:
            lo = x
        if x > hi:
            hi = x
    want = [int(np.sqrt(min(1.0, max(0.0, (x - lo) / (hi - lo)))) * 255) for x in dm]
    got, glo, ghi = finish_on_host(dm)
    assert (glo, ghi) == (lo, hi)
    assert got[:, 0].tolist() == want and (got[:, 3] == 255).all()
    assert (finish_on_host(np.full(7, 0.25))[0] == np.array([0, 0, 0, 255], dtype=np.uint8)).all()


def test_library_exports_the_depth_entry_points():
    lib = nh.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in nh.API_SYMBOLS


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def gpu():
    ctx = nh.NdtHip(0)
    yield ctx
    ctx.close()


# fixture -> what it is rendered with (the side-by-side frame's map is the left eye's)
CASES = {"depth_c3_random4d": {}, "aa_c3_random4d_depth": {"aa": (20, 3)}, "st_zoo4d_sbs": {"stereo": 1},
         "st_zoo3d_anaglyph": {"stereo": 3}}


def _render_both(gpu, name):
    g = golden(name)
    gpu.upload_scene(g.scene)
    _, dm, _ = gpu.render(g.width, g.height, g.depth, depth_map=True, **CASES[name])
    rgba8, depth8, rng, _ = gpu.render_rgba8_depth(g.width, g.height, g.depth, **CASES[name])
    return g, dm, rgba8, depth8, rng


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_equal_to_the_host_path_exactly(gpu, name):
    g, dm, rgba8, depth8, rng = _render_both(gpu, name)
    want, lo, hi = finish_on_host(dm)
    assert (dm > 0).any() and hi > lo
    differ = int((depth8 != want).sum())
    print("%s: %d of %d map bytes differ from the host path; range [%r, %r]" % (name, differ, want.size, rng[0], rng[1]))
    assert differ == 0
    assert rng.view(np.uint64).tolist() == np.array([lo, hi]).view(np.uint64).tolist()
    assert np.array_equal(rgba8, gpu.render_rgba8(g.width, g.height, g.depth, **CASES[name])[0])
    assert gpu.depth_launches() == 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["depth_c3_random4d", "aa_c3_random4d_depth", "st_zoo3d_anaglyph"])
def test_within_one_step_of_the_references_map(gpu, name):
    """Against the compiled reference's map (the fixture's `depth`): its values agree with the device's to about 1e-15, and the
    truncation sits on sqrt(v) * 255 -- a byte may fall on the other side of an integer, never further.  How many bytes do
    differ is printed, not bounded: profiles/depth_on_device.txt records the count once it has been measured."""
    g, _, _, depth8, _ = _render_both(gpu, name)
    want, _, _ = finish_on_host(g.data["depth"])
    step = np.abs(depth8.astype(np.int16) - want.astype(np.int16))
    print("%s: %d of %d map bytes differ from the reference's finished map (largest step %d)" % (
        name, int((step != 0).sum()), want.size, int(step.max())))
    assert step.max() <= 1


@pytest.mark.gpu
def test_depth_zero_gives_a_zeroed_map(gpu):
    g = golden("depth_c3_random4d")
    gpu.upload_scene(g.scene)
    rgba8, depth8, rng, _ = gpu.render_rgba8_depth(g.width, g.height, 0)
    assert (depth8 == np.array([0, 0, 0, 255], dtype=np.uint8)).all()
    assert rng.view(np.uint64).tolist() == [0, 0]
    assert np.array_equal(rgba8, gpu.render_rgba8(g.width, g.height, 0)[0])


def _finish_on_device(gpu, dm):
    """ndt_hip_depth_rgba8_device on a hand-made map; the output buffer starts as 0xA5 and has a guard behind it."""
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(dm, dtype=np.float64)).cuda()
    out = torch.full((dm.size * 4 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rng = np.full(2, -7.0)
    rc = gpu.lib.ndt_hip_depth_rgba8_device(gpu.ctx, C.c_void_p(dev.data_ptr()), dm.size, C.c_void_p(out.data_ptr()), rng.ctypes.data)
    got = out.cpu().numpy()
    assert (got[dm.size * 4:] == 0xA5).all()
    return rc, got[:dm.size * 4].reshape(dm.size, 4), rng


# 1, 63 .. 65: under, at and over a wavefront; 2049: one over what a workgroup of the reduction takes a trip; 1000003: more
# than one trip of both kernels' full grids, and a multiple of neither
SIZES = [1, 63, 64, 65, 2049, 300007, 1000003]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["constant", "two_values", "random"])
def test_hand_made_maps(gpu, n, kind):
    rng = np.random.default_rng(n)
    if kind == "constant":
        dm = np.full(n, 0.375)
    elif kind == "two_values":
        dm = np.full(n, 0.125)
        dm[n // 2] = 3.5               # one pixel carries the maximum (the whole map when n = 1)
    else:
        dm = np.where(rng.random(n) < 0.25, 0.0, 1.0 / rng.uniform(0.01, 50.0, n))
    rc, got, r = _finish_on_device(gpu, dm)
    assert rc == 0, gpu.lib.ndt_hip_last_error()
    want, lo, hi = finish_on_host(dm)
    assert np.array_equal(got, want)
    assert r.view(np.uint64).tolist() == np.array([lo, hi]).view(np.uint64).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 65, 300007])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
def test_planted_nan_and_infinity_are_refused(gpu, n, bad):
    rng = np.random.default_rng(n)
    for at in sorted({0, n // 2, n - 1}):
        dm = 1.0 / rng.uniform(0.5, 50.0, n)
        dm[at] = bad
        rc, got, r = _finish_on_device(gpu, dm)
        assert rc == NDT_E_UNSUPPORTED
        assert "pixel %d)" % at in gpu.lib.ndt_hip_last_error().decode()
        assert (got == 0xA5).all()              # nothing written
        assert r.tolist() == [-7.0, -7.0]
    # two of them: the one named is the lowest
    if n > 2:
        dm = 1.0 / rng.uniform(0.5, 50.0, n)
        dm[n - 1] = dm[n // 2] = bad
        rc, got, _ = _finish_on_device(gpu, dm)
        assert rc == NDT_E_UNSUPPORTED and "pixel %d)" % (n // 2) in gpu.lib.ndt_hip_last_error().decode()
        assert (got == 0xA5).all()


@pytest.mark.gpu
def test_bad_arguments_are_refused(gpu):
    import torch
    dev = torch.zeros(16, dtype=torch.float64, device="cuda")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lib, d, o = gpu.lib, dev.data_ptr(), out.data_ptr()
    assert lib.ndt_hip_depth_rgba8_device(gpu.ctx, None, 16, C.c_void_p(o), None) == NDT_E_INVALID
    assert lib.ndt_hip_depth_rgba8_device(gpu.ctx, C.c_void_p(d), 16, None, None) == NDT_E_INVALID
    assert lib.ndt_hip_depth_rgba8_device(None, C.c_void_p(d), 16, C.c_void_p(o), None) == NDT_E_INVALID
    assert lib.ndt_hip_depth_rgba8_device(gpu.ctx, C.c_void_p(d), 0, C.c_void_p(o), None) == NDT_E_INVALID
    assert lib.ndt_hip_depth_rgba8_device(gpu.ctx, C.c_void_p(d + 4), 8, C.c_void_p(o), None) == NDT_E_INVALID
    assert lib.ndt_hip_depth_rgba8_device(gpu.ctx, C.c_void_p(d), 8, C.c_void_p(o + 2), None) == NDT_E_INVALID
    assert lib.ndt_hip_depth_rgba8_device(gpu.ctx, C.c_void_p(d), 16, C.c_void_p(o), None) == 0        # range_out is optional
    assert (out.cpu().numpy().reshape(16, 4) == np.array([0, 0, 0, 255], dtype=np.uint8)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["depth_c3_random4d", "aa_c3_random4d_depth", "st_zoo4d_sbs"])
def test_png_files_decode_to_the_same_bytes(gpu, name):
    g, _, rgba8, depth8, rng = _render_both(gpu, name)
    png, depth_png, rng2, _ = gpu.render_png_depth(g.width, g.height, g.depth, **CASES[name])
    assert np.array_equal(read_png(png), rgba8)
    assert np.array_equal(read_png(depth_png), depth8)
    assert rng2.view(np.uint64).tolist() == rng.view(np.uint64).tolist()
    assert [s.png_bytes for s in gpu.png_stats] == [len(png), len(depth_png)]      # (before render_png replaces the record)
    assert png == gpu.render_png(g.width, g.height, g.depth, **CASES[name])[0]
    # the image as a file, the map as its bytes
    png3, depth8_3, _, _ = gpu.render_png_depth(g.width, g.height, g.depth, depth_png=False, **CASES[name])
    assert png3 == png and np.array_equal(depth8_3, depth8)


@pytest.mark.gpu
def test_refusals_are_those_of_render_depth(gpu):
    g = golden("depth_c3_random4d")
    gpu.upload_scene(g.scene)
    # -z beside a stochastic -a (samples > 1 under recursive_aa): the code and the text of ndt_hip_render_depth
    with pytest.raises(nh.NdtHipError) as want:
        gpu.render(g.width, g.height, g.depth, aa=(20, 2), samples=3, depth_map=True)
    assert want.value.code == NDT_E_UNSUPPORTED
    with pytest.raises(nh.NdtHipError) as got:
        gpu.render_rgba8_depth(g.width, g.height, g.depth, aa=(20, 2), samples=3)
    assert got.value.code == want.value.code and str(got.value) == str(want.value)
    with pytest.raises(nh.NdtHipError) as got:
        gpu.render_png_depth(g.width, g.height, g.depth, aa=(20, 2), samples=3)
    assert got.value.code == want.value.code and str(got.value) == str(want.value)
    # room one byte short, for either file: NDT_E_NOMEM with the size needed, and nothing written to that buffer
    png, depth_png, _, _ = gpu.render_png_depth(g.width, g.height, g.depth)
    p = gpu.params(g.width, g.height, g.depth)
    for short_image in (True, False):
        cap, depth_cap = len(png) - (1 if short_image else 0), len(depth_png) - (0 if short_image else 1)
        a, b = np.full(cap + 64, 0xA5, dtype=np.uint8), np.full(depth_cap + 64, 0xA5, dtype=np.uint8)
        st = (nh.PngStats * 2)()
        rc = gpu.lib.ndt_hip_render_png_depth(gpu.ctx, C.byref(p), a.ctypes.data, cap, b.ctypes.data, depth_cap, None, C.byref(st), None, None)
        assert rc == NDT_E_NOMEM
        assert str(len(png) if short_image else len(depth_png)) in gpu.lib.ndt_hip_last_error().decode()
        assert (st[0].png_bytes, st[1].png_bytes) == ((len(png), 0) if short_image else (len(png), len(depth_png)))
        assert (b == 0xA5).all()
        assert (a == 0xA5).all() if short_image else a[:cap].tobytes() == png and (a[cap:] == 0xA5).all()
    # the map goes to exactly one place
    out = np.zeros(nh.png_bound(g.width, g.height), dtype=np.uint8)
    assert gpu.lib.ndt_hip_render_png_depth(gpu.ctx, C.byref(p), out.ctypes.data, out.size, None, 0, None, None, None, None) == NDT_E_INVALID
    assert gpu.lib.ndt_hip_render_png_depth(gpu.ctx, C.byref(p), out.ctypes.data, out.size, out.ctypes.data, out.size, out.ctypes.data,
                                            None, None, None) == NDT_E_INVALID


# ---------------------------------------------------------------- driver

def _run(cwd, *flags, scene="builtin:yaml"):
    assert os.path.exists(DRIVER), "ndt_amd/host/ndt_hip is not built"
    os.makedirs(str(cwd), exist_ok=True)
    return subprocess.run([DRIVER, "-s", scene, "-d", "4", "-f", "0", "-r", "96x54", "-l", "6"] + list(flags),
                          capture_output=True, text=True, cwd=str(cwd))


def test_driver_refuses_flag_combinations_before_anything_else(tmp_path):
    """(CPU) the three refused combinations end the run with a message, before a scene is loaded or a device asked for."""
    for flags, words in ((["--depth", "gpu"], ("--depth gpu", "-z")),
                         (["-z", "--depth", "gpu", "--raw", "fb.f64"], ("--depth gpu", "--raw")),
                         (["-z", "--depth", "gpu", "--png", "--depth-png"], ("--depth-png", "--deflate gpu")),
                         (["-z", "--png", "--deflate", "gpu", "--depth-png"], ("--depth-png", "--depth gpu")),
                         (["-z", "--depth", "card"], ("--depth", "host or gpu"))):
        r = _run(tmp_path, *flags)
        assert r.returncode != 0, flags
        for w in words:
            assert w in r.stderr, (flags, r.stderr)
    assert not list(tmp_path.rglob("*.p*"))


@pytest.fixture(scope="module")
def zoo(tmp_path_factory):
    """tests/scenes/parity_zoo.c compiled against this repository's host headers (it says #include "../scene.h")."""
    d = tmp_path_factory.mktemp("zoo")
    (d / "scenes").mkdir()
    for h in os.listdir(os.path.join(HOST, "include")):
        os.symlink(os.path.join(HOST, "include", h), d / h)
    shutil.copy(ZOO_SRC, d / "scenes" / "parity_zoo.c")
    so = str(d / "scenes" / "parity_zoo.so")
    r = subprocess.run(["gcc", "-O2", "-std=c99", "-D_GNU_SOURCE", "-fPIC", "-shared", "-o", so, str(d / "scenes" / "parity_zoo.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return so


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [[], ["--png"], ["--png", "--deflate", "gpu"]], ids=["ppm", "png", "png_deflate_gpu"])
def test_driver_writes_the_same_files(zoo, tmp_path, fmt):
    files = {}
    for where in ("host", "gpu"):
        r = _run(tmp_path / where, "-z", "--depth", where, *fmt, scene=zoo)
        assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
        image = list((tmp_path / where / "images").rglob("*.p*"))
        depth = list((tmp_path / where / "depth").glob("*.p*"))
        assert len(image) == 1 and len(depth) == 1 and depth[0].suffix == ".ppm"
        assert image[0].suffix == (".png" if fmt else ".ppm")
        files[where] = (image[0].name, image[0].read_bytes(), depth[0].name, depth[0].read_bytes())
        assert ("finished depth map [" in r.stdout) == (where == "gpu")
        if where == "gpu":
            assert " on GPU 0 in 2 launches" in r.stdout
    assert files["gpu"] == files["host"]
    assert read_ppm(files["gpu"][3]).max() == 255 and read_ppm(files["gpu"][3]).min() == 0


@pytest.mark.gpu
def test_driver_depth_png_decodes_to_the_ppm(zoo, tmp_path):
    r = _run(tmp_path / "ppm", "-z", "--depth", "host", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:]
    want = read_ppm(list((tmp_path / "ppm" / "depth").glob("*.ppm"))[0].read_bytes())
    r = _run(tmp_path / "png", "-z", "--depth", "gpu", "--png", "--deflate", "gpu", "--depth-png", "-g", "2", scene=zoo)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    found = list((tmp_path / "png" / "depth").glob("*"))
    assert len(found) == 1 and found[0].suffix == ".png"
    pixels = read_png(found[0].read_bytes())
    assert np.array_equal(pixels[..., :3], want) and (pixels[..., 3] == 255).all()
    assert "compressed depth PNG of %d bytes on GPU" % len(found[0].read_bytes()) in r.stdout
