"""include/nvcomp/device/detail/wave_casc.hpp -- the wave primitives the device-side Cascaded core adds to the other four
detail headers -- lane by lane against the model of tests/wave_model.py, on the card and on the host emulation (`backend`),
where tests/emu/nvcomp/device/detail/wave_casc.hpp stands in for the header. Every function the header defines is run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import wave_model as model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "nvcomp", "device", "detail", "wave_casc.hpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

KERNELS = r"""
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <nvcomp/device/detail/wave_casc.hpp>
namespace w = nvcomp::device::detail::wave;

/* one wave per case: lane l of case c works on element 64 c + l */
__global__ void __launch_bounds__(64) k_align_bits(const uint32_t* hi, const uint32_t* lo, const uint32_t* shift, uint32_t* out)
{
  const uint32_t i = 64 * blockIdx.x + threadIdx.x;
  out[i] = w::align_bits(hi[i], lo[i], shift[i]);
}

__global__ void __launch_bounds__(64) k_scan_max(const uint32_t* v, uint32_t* out)
{
  const uint32_t i = 64 * blockIdx.x + threadIdx.x;
  out[i] = w::scan_max_inclusive(v[i]);
}

extern "C" int wcasc_align_bits(const uint32_t* hi, const uint32_t* lo, const uint32_t* shift, uint32_t* out, unsigned cases, hipStream_t s)
{
  hipLaunchKernelGGL(k_align_bits, dim3(cases), dim3(64), 0, s, hi, lo, shift, out);
  return (int)hipGetLastError();
}

extern "C" int wcasc_scan_max(const uint32_t* v, uint32_t* out, unsigned cases, hipStream_t s)
{
  hipLaunchKernelGGL(k_scan_max, dim3(cases), dim3(64), 0, s, v, out);
  return (int)hipGetLastError();
}
"""

_libs = {}


@pytest.fixture
def ops(backend, tmp_path_factory):
    if backend.name not in _libs:
        d = tmp_path_factory.mktemp(f"wcasc_{backend.name}")
        src, so = d / "wave_casc_kernels.hip", str(d / "wcasc.so")
        src.write_text(KERNELS)
        if backend.name == "emu":
            import conftest

            conftest.emu_library()
            cmd = ["g++", "-O1", "-std=c++17", "-x", "c++", "-shared", "-fPIC", "-Itests/emu", "-Iinclude", str(src), "-o", so,
                   "-Ltests/emu", "-lnvcomp_emu", f"-Wl,-rpath,{REPO}/tests/emu"]
        else:
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(REPO, "include"),
                   str(src), "-o", so]
        r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        lib = C.CDLL(so)
        vp = C.c_void_p
        lib.wcasc_align_bits.argtypes = [vp, vp, vp, vp, C.c_uint, vp]
        lib.wcasc_scan_max.argtypes = [vp, vp, C.c_uint, vp]
        _libs[backend.name] = lib
    return _libs[backend.name]


def run(backend, fn, *inputs):
    dev = backend.dev
    cases = inputs[0].shape[0]
    bufs = [dev.upload(np.ascontiguousarray(a, dtype=np.uint32).view(np.uint8)) for a in inputs]
    out = dev.upload(np.full(cases * 64, 0xDEADBEEF, dtype=np.uint32).view(np.uint8))
    assert fn(*[dev.ptr(b) for b in bufs], dev.ptr(out), cases, dev.stream()) == 0
    dev.synchronize()
    return dev.download(out).view(np.uint32).reshape(cases, 64)


def lane_values(rng, cases):
    """Rows of 64 lane values: random, all equal, ascending, descending, a single peak in every lane position's row, and the
    ends of the range."""
    rows = [rng.randint(0, 1 << 32, size=64, dtype=np.uint64) for _ in range(cases)]
    rows += [np.full(64, 7), np.arange(64), np.arange(64)[::-1], np.zeros(64), np.full(64, 0xFFFFFFFF)]
    for peak in (0, 15, 16, 31, 32, 47, 48, 63):  # the DPP ladder's row boundaries
        r = rng.randint(0, 1000, size=64)
        r[peak] = 0xFFFFFFF0
        rows.append(r)
    return np.asarray(rows, dtype=np.uint64).astype(np.uint32)


def test_scan_max_inclusive(backend, ops):
    v = lane_values(np.random.RandomState(1), 24)
    got = run(backend, ops.wcasc_scan_max, v)
    for row, g in zip(v, got):
        assert np.array_equal(g, np.asarray(model.scan_max_inclusive(row), dtype=np.uint32))
        assert np.array_equal(g, np.maximum.accumulate(row))


def test_align_bits(backend, ops):
    rng = np.random.RandomState(2)
    hi, lo = lane_values(rng, 24), lane_values(rng, 24)[::-1].copy()
    shift = np.tile(np.arange(64, dtype=np.uint32) % 32, (hi.shape[0], 1))  # every shift 0 ... 31, twice a row
    got = run(backend, ops.wcasc_align_bits, hi, lo, shift)
    want = (((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> shift.astype(np.uint64)).astype(np.uint32)
    assert np.array_equal(got, want)
    for h, l, s, g in zip(hi, lo, shift, got):
        assert np.array_equal(g, np.asarray(model.align_bits(h, l, s), dtype=np.uint32))


def test_every_function_of_the_header_is_tested():
    """The header's functions are exactly the ones the kernels above call, and the emulation's stand-in names them all."""
    text = open(HEADER).read()
    defined = set(re.findall(r"__device__ __forceinline__ \w+ (\w+)\(", text))
    assert defined == {"align_bits", "scan_max_inclusive"}
    shadow = open(os.path.join(REPO, "tests", "emu", "nvcomp", "device", "detail", "wave_casc.hpp")).read()
    for name in defined:
        assert f"w::{name}(" in KERNELS and f"using ::wave::{name};" in shadow and hasattr(model, name)
