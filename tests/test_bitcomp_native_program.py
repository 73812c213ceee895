"""examples/bitcomp_native_example.cpp runs end to end: against the host emulation of the kernels (CPU-only) and, built
by examples/Makefile, on the card. The program verifies its own result (non-zero exit code on a mismatch)."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd, **kw):
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900, **kw)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}"
    return r.stdout


def check(out):
    assert "lossy round trip within the error bound" in out and "partial range" in out and "equal" in out
    ratio = float(out.split("ratio:")[1].split()[0])
    assert ratio > 1.5


def test_native_example_on_emulator(tmp_path):
    import conftest

    conftest.emu_library()
    exe = tmp_path / "bitcomp_native_emu"
    run(["g++", "-O1", "-std=c++17", "-Itests/emu", "-Iinclude", "-Iexamples", "examples/bitcomp_native_example.cpp",
         "-o", str(exe), "-Ltests/emu", "-lnvcomp_emu", f"-Wl,-rpath,{REPO}/tests/emu"])
    check(run([str(exe), "4"]))  # 4 MiB: the emulator runs a lane at a time


@pytest.mark.gpu
def test_native_example_on_gpu():
    run(["make", "-C", "examples", f"{REPO}/examples/bin/bitcomp_native_example"])
    check(run(["examples/bin/bitcomp_native_example"]))
