"""Many-light scenes pinned by the compiled reference (tests/golden/make_golden_lights.py): YAML files of 140-150 lights --
point lattices, directionals, ambient entries at list positions 0, 64, 65 and the end -- the scene the reference built from
each (flattened), the framebuffer it rendered and its trace_kd counts.  The oracle, the host's YAML reader and the device path
must all arrive at the reference's answers for more lights than one 64-light window of the lighting kernels."""
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, GOLDEN
from ndt_amd import load_scene

YDIR = os.path.join(GOLDEN, "yaml")
HOST = os.path.join(ROOT, "ndt_amd", "host")
DRIVER = os.path.join(HOST, "ndt_hip")
CASES = ["yl_random4d_150", "yl_hypercube6d_140"]
TOL_SPEC = 1e-4
TOL_TIGHT = 1e-9


def _meta(name):
    with open(os.path.join(YDIR, name + ".json")) as f:
        return json.load(f)


def _scene(name):
    return load_scene(os.path.join(YDIR, name + ".ndtscene.gz"))


def _fb(name):
    return np.load(os.path.join(YDIR, name + ".npz"))["fb"]


@pytest.mark.parametrize("name", CASES)
def test_fixture_has_many_lights(name):
    fs = _scene(name)
    types = [l["type"] for l in fs.lights]
    assert len(types) == _meta(name)["lights"] > 128
    assert types[0] == types[64] == types[65] == types[-1] == 0        # ambient where windows of 64 start and end
    assert {1, 2} <= set(types)


@pytest.mark.parametrize("name", CASES)
def test_oracle_reproduces_the_reference(oracle, name):
    m = _meta(name)
    out, st = oracle.render(_scene(name), m["width"], m["height"], m["depth"])
    assert np.array_equal(out, _fb(name))
    assert st.rays_ref_equiv == m["rays_total"]


@pytest.fixture(scope="module")
def driver():
    subprocess.run(["make", "-C", os.path.join(ROOT, "ndt_amd", "csrc"), "-j", "8"], check=True, capture_output=True)
    subprocess.run(["make", "-C", HOST], check=True, capture_output=True)
    return DRIVER


@pytest.mark.parametrize("name", CASES)
def test_yaml_loads_to_the_scene_the_reference_builds(driver, tmp_path, name):
    """The host's YAML reader, flattener and driver take every light: the dump is the reference's, byte for byte."""
    m = _meta(name)
    y = str(tmp_path / (name + ".yaml"))
    with gzip.open(os.path.join(YDIR, name + ".yaml.gz"), "rb") as src, open(y, "wb") as dst:
        dst.write(src.read())
    out = str(tmp_path / "out.ndtscene")
    r = subprocess.run([DRIVER, "-s", "builtin:yaml", "-u", y, "-d", str(m["dims"]), "-f", "0:0", "--dump-scene", out],
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    with gzip.open(os.path.join(YDIR, name + ".ndtscene.gz"), "rt") as f:
        assert open(out).read() == f.read()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_renders_the_references_frame(oracle, name):
    """The device's frame against the reference's; rays_ref_equiv against the reference's trace_kd count, rays_shadow (rays
    traced, not weighted by the reference's re-tracing) against the oracle's."""
    from ndt_amd.hip import NdtHip
    m = _meta(name)
    fs = _scene(name)
    _, so = oracle.render(fs, m["width"], m["height"], m["depth"])
    gpu = NdtHip(0)
    try:
        gpu.upload_scene(fs)
        out, st = gpu.render(m["width"], m["height"], m["depth"])
    finally:
        gpu.close()
    diff = np.abs(out - _fb(name))
    assert diff.max() < TOL_SPEC, "max abs diff %g" % diff.max()
    assert (diff > TOL_TIGHT).sum() == 0, "max abs diff %g" % diff.max()
    assert st.rays_ref_equiv == m["rays_total"]
    assert st.rays_shadow == so.rays_shadow
    assert st.rays_primary == m["width"] * m["height"]
