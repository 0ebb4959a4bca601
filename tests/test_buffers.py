"""csrc/cmax_buffers.h on its own: tests/buffers_check.hip (its own main, its own cmax::set_error, no other file of the library) is
compiled with hipcc and run as a process.  Without a device every allocation fails and the program checks that the buffers say so every
time (CMAX_ENOMEM, null, capacity 0, nothing counted; release, the destructor and swap harmless); with one it reserves, regrows, swaps
and releases a few KB.  The program says which of the two it ran."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("buffers") / "buffers_check")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "buffers_check.hip"), "-o", exe],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"rc {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
    return p.stdout.strip().splitlines()[-1]


def test_buffers_fail_cleanly_without_a_device(check_output):
    if check_output == "device ok":
        pytest.skip("a device is present: test_buffers_on_a_device covers this machine")
    assert check_output == "no-device ok"


@pytest.mark.gpu
def test_buffers_on_a_device(check_output):
    assert check_output == "device ok"
