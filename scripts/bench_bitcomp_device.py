#!/usr/bin/env python3
"""Device-side Bitcomp (include/nvcomp/device/bitcomp.hpp) fused into its consumer, against the two-kernel path.

Workload: 1 GiB in 64 KiB chunks of nvcomp_amd.datasets.float_columns (the data of the README's Bitcomp row, read as
int32), compressed once with nvcompBatchedBitcompCompressAsync {algorithm 0, int}. The consumer is
y[i] += a * (q[i] * delta) into an fp32 array.

  (a) fused       one user kernel decodes each chunk with decompress_to() and accumulates where the values are decoded;
  (b) two-kernel  nvcompBatchedBitcompDecompressAsync writes the int32 values to HBM, an elementwise kernel reads them;
  (c) plain       decompress() from a user kernel against the batched call alone: the cost of the header-only path.

--lib PATH takes the batched calls from another build of libnvcomp.so (the parent commit's, for an A/B in one process).
Each call is timed with HIP events around it; GB/s are uncompressed bytes over the median time. The paths alternate, in
--repeats rounds. (a) and (b) are checked to give the same y bit for bit, (c) the same bytes as the batched decoder.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SRC = os.path.join(REPO, "scripts", "bench_bitcomp_device.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CHUNK = 1 << 16


def build(out_dir):
    """Compile the kernels; return (library path, resource use per kernel)."""
    so = os.path.join(out_dir, "bench_bitcomp_device.so")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(REPO, "include"),
                        "-Rpass-analysis=kernel-resource-usage", SRC, "-o", so], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr[-3000:])
    res, cur = {}, None
    keys = {"VGPRs": "vgpr", "TotalSGPRs": "sgpr", "ScratchSize [bytes/lane]": "scratch", "LDS Size [bytes/block]": "lds",
            "Occupancy [waves/SIMD]": "occupancy"}
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\s*)(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = next((n for n in ("fused_decode_axpy", "axpy_from_ints", "plain_decompress") if n in m.group(2)), None)
            if cur:
                res[cur] = {}
        elif cur is not None:
            res[cur][keys[m.group(1)]] = int(m.group(2))
    return so, res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib", default=None, help="libnvcomp.so for the batched calls (default: this tree's)")
    args = ap.parse_args()

    import torch

    import nvcomp_amd
    from nvcomp_amd import datasets
    from nvcomp_amd._lib import BitcompOpts

    so, resources = build(tempfile.mkdtemp(prefix="bench_bitcomp_device_"))
    k = C.CDLL(so)
    vp, sz, f = C.c_void_p, C.c_size_t, C.c_float
    k.bench_fused.argtypes = [vp, vp, vp, sz, sz, f, f, vp, vp]
    k.bench_axpy.argtypes = [vp, vp, sz, f, f, C.c_uint, vp]
    k.bench_plain.argtypes = [vp, vp, vp, sz, sz, vp, vp]
    lib = nvcomp_amd.load_library(args.lib) if args.lib else nvcomp_amd.load_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    s = C.c_void_p(stream.cuda_stream)
    opts = BitcompOpts(0, 4)
    a, delta = 0.37, 1e-3

    total = int(args.gib * (1 << 30)) // CHUNK * CHUNK
    n = total // CHUNK
    unique = np.ascontiguousarray(datasets.float_columns(64 << 20, seed=11)).view(np.uint8).reshape(-1)
    data = torch.from_numpy(unique).to(dev).repeat(-(-total // unique.size))[:total].contiguous()
    in_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * CHUNK + data.data_ptr()
    sizes = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
    max_out = C.c_size_t(0)
    assert lib.nvcompBatchedBitcompCompressGetMaxOutputChunkSize(CHUNK, opts, C.byref(max_out)) == 0
    comp = torch.empty(n * max_out.value, dtype=torch.uint8, device=dev)
    comp_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * max_out.value + comp.data_ptr()
    comp_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    assert lib.nvcompBatchedBitcompCompressAsync(in_ptrs.data_ptr(), sizes.data_ptr(), CHUNK, n, None, 0, comp_ptrs.data_ptr(),
                                                 comp_sizes.data_ptr(), opts, s) == 0
    torch.cuda.synchronize()
    comp_total = int(comp_sizes.sum().item())

    inter = torch.empty(total, dtype=torch.uint8, device=dev)
    inter_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * CHUNK + inter.data_ptr()
    plain_out = torch.empty(total, dtype=torch.uint8, device=dev)
    actual = torch.zeros(n, dtype=torch.int64, device=dev)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=dev)
    st_fused = torch.full((n,), -1, dtype=torch.int32, device=dev)
    st_plain = torch.full((n,), -1, dtype=torch.int32, device=dev)
    y_two = torch.zeros(total // 4, dtype=torch.float32, device=dev)
    y_fused = torch.zeros(total // 4, dtype=torch.float32, device=dev)
    axpy_grid = 256 * 32 * 8

    def batched():
        assert lib.nvcompBatchedBitcompDecompressAsync(comp_ptrs.data_ptr(), comp_sizes.data_ptr(), sizes.data_ptr(),
                                                       actual.data_ptr(), n, None, 0, inter_ptrs.data_ptr(),
                                                       statuses.data_ptr(), s) == 0

    def two_kernel():
        batched()
        assert k.bench_axpy(inter.data_ptr(), y_two.data_ptr(), total // 4, a, delta, axpy_grid, s) == 0

    def fused():
        assert k.bench_fused(comp_ptrs.data_ptr(), comp_sizes.data_ptr(), y_fused.data_ptr(), CHUNK, n, a, delta,
                             st_fused.data_ptr(), s) == 0

    def plain():
        assert k.bench_plain(comp_ptrs.data_ptr(), comp_sizes.data_ptr(), plain_out.data_ptr(), CHUNK, n, st_plain.data_ptr(), s) == 0

    paths = {"two_kernel": two_kernel, "fused": fused, "batched": batched, "plain": plain}
    ms = {name: [] for name in paths}
    for _ in range(args.repeats):  # alternate the paths so that drift on the card hits all alike
        for name, fn in paths.items():
            for _ in range(args.warmup):
                fn()
            for _ in range(args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
    torch.cuda.synchronize()

    # both accumulators ran the same number of steps from zero: they must agree bit for bit
    ok = bool((statuses == 0).all().item() and (st_fused == 0).all().item() and (st_plain == 0).all().item())
    ok = ok and torch.equal(y_two.view(torch.int32), y_fused.view(torch.int32))
    ok = ok and torch.equal(plain_out, inter) and torch.equal(inter, data)

    def gbps(v):
        return round(total / (np.median(v) * 1e-3) / 1e9, 1)

    res = {"metric": "bitcomp_device_fused_decode_axpy", "unit": "GB/s (uncompressed bytes)", "bytes": total, "chunks": n,
           "chunk_bytes": CHUNK, "ratio": round(total / comp_total, 4), "steps": args.steps * args.repeats,
           "warmup": args.warmup, "batched_library": args.lib or "this tree",
           "expected_traffic_ratio": round((comp_total + 2 * total) / (comp_total + 4 * total), 3),
           **{f"{name}_gbps": gbps(v) for name, v in ms.items()},
           **{f"{name}_ms_min_median_max": [round(min(v), 4), round(float(np.median(v)), 4), round(max(v), 4)] for name, v in ms.items()},
           "fused_over_two_kernel": round(float(np.median(ms["two_kernel"]) / np.median(ms["fused"])), 3),
           "plain_over_batched": round(float(np.median(ms["batched"]) / np.median(ms["plain"])), 3),
           "kernel_resources": resources, "verified": ok}
    print(json.dumps(res))
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
