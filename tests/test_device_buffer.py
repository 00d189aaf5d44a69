"""DeviceBuffer (ndt_amd/csrc/ndt_buffer.hpp), the one grow and free path of the context's device buffers, on its own: the
stand-alone program tests/device_buffer_main.cpp includes nothing but that header, is built here and run once.

Without a HIP device every hipMalloc fails, which is the one way to see what reserve() leaves behind then: an empty buffer and
NDT_E_NOMEM, also for a smaller request after it (a size left standing would let the next frame render into a null pointer).
With a device: reserve, reuse, growth, head room and release on a stream of the program's own, a few KB in all.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRONG_MACHINE = 77


def run_program(tmp_path, mode):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "device_buffer_main")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "ndt_amd", "csrc"), "-x", "hip",
                    os.path.join(ROOT, "tests", "device_buffer_main.cpp"), "-o", exe], check=True, timeout=60)
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=60)
    print(r.stdout + r.stderr)
    return r


def test_a_failed_allocation_leaves_an_empty_buffer(tmp_path):
    r = run_program(tmp_path, "nodevice")
    if r.returncode == WRONG_MACHINE:
        pytest.skip("a HIP device is present: its hipMalloc does not fail")
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_reserve_reuses_grows_and_releases_on_the_device(tmp_path):
    r = run_program(tmp_path, "device")
    assert r.returncode == 0, r.stderr
