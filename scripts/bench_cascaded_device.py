#!/usr/bin/env python3
"""Device-side Cascaded (include/nvcomp/device/cascaded.hpp) fused into its consumer, against the batched calls.

Workload: 1 GiB in 64 KiB chunks, options {4096, int, 2, 1, 1}, of nvcomp_amd.datasets.float_columns read as int32 (the
data of the README's Cascaded row) and of nvcomp_amd.datasets.int32_column, compressed once with
nvcompBatchedCascadedCompressAsync. The consumer is a filter and a sum: per chunk, the sum of the values v with
lo <= v < hi.

  (a) fused       one user kernel decodes each chunk with decompress_to() and sums where the values are decoded;
  (b) two_kernel  nvcompBatchedCascadedDecompressAsync writes the int32 values to HBM, a reduction kernel reads them;
  (c) plain       decompress() from a user kernel into memory;
  (d) batched     the batched decode alone;
  (e) compress / batched_compress   compress() from a user kernel against nvcompBatchedCascadedCompressAsync.

--lib PATH takes the batched calls from another build of libnvcomp.so. Each call is timed with HIP events around it; GB/s
are uncompressed bytes over the median time. The paths alternate, in --repeats rounds. (a) and (b) must give the same
sums, (c) the same bytes as (d), (e) the same streams. Prints one JSON line per input."""
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
SRC = os.path.join(REPO, "scripts", "bench_cascaded_device.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CHUNK = 1 << 16
KERNELS = ("fused_filter_sum", "filter_sum_ints", "plain_decompress", "plain_compress")


def build(out_dir):
    """Compile the kernels; return (library path, resource use per kernel)."""
    so = os.path.join(out_dir, "bench_cascaded_device.so")
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
            cur = next((n for n in KERNELS if n in m.group(2)), None)
            if cur:
                res[cur] = {}
        elif cur is not None:
            res[cur][keys[m.group(1)]] = int(m.group(2))
    return so, res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lib", default=None, help="libnvcomp.so for the batched calls (default: this tree's)")
    args = ap.parse_args()

    import torch

    import nvcomp_amd
    from nvcomp_amd import datasets
    from nvcomp_amd._lib import CascadedOpts

    so, resources = build(tempfile.mkdtemp(prefix="bench_cascaded_device_"))
    k = C.CDLL(so)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
    k.bench_fused.argtypes = [vp, vp, sz, sz, i32, i32, vp, vp, vp]
    k.bench_reduce.argtypes = [vp, sz, sz, i32, i32, vp, vp]
    k.bench_plain.argtypes = [vp, vp, vp, sz, sz, vp, vp]
    k.bench_compress.argtypes = [vp, sz, sz, vp, vp, CascadedOpts, vp]
    lib = nvcomp_amd.load_library(args.lib) if args.lib else nvcomp_amd.load_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    s = C.c_void_p(stream.cuda_stream)
    opts = CascadedOpts(4096, 4, 2, 1, 1)
    total = int(args.gib * (1 << 30)) // CHUNK * CHUNK
    n = total // CHUNK
    all_ok = True

    for name, gen in (("float_columns", datasets.float_columns), ("int32_column", datasets.int32_column)):
        unique = np.ascontiguousarray(gen(64 << 20, 11)).view(np.uint8).reshape(-1)
        as_int = unique.view(np.int32)
        lo, hi = (int(v) for v in np.percentile(as_int[: 1 << 20], [25, 75]))  # about half of the values pass the filter
        data = torch.from_numpy(unique).to(dev).repeat(-(-total // unique.size))[:total].contiguous()
        in_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * CHUNK + data.data_ptr()
        sizes = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
        max_out, temp_c, temp_d = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        assert lib.nvcompBatchedCascadedCompressGetMaxOutputChunkSize(CHUNK, opts, C.byref(max_out)) == 0
        assert lib.nvcompBatchedCascadedCompressGetTempSize(n, CHUNK, opts, C.byref(temp_c)) == 0
        assert lib.nvcompBatchedCascadedDecompressGetTempSize(n, CHUNK, C.byref(temp_d)) == 0
        slot = (max_out.value + 7) // 8 * 8
        temp = torch.empty(max(temp_c.value, temp_d.value, 8), dtype=torch.uint8, device=dev)
        comp = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        comp_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * slot + comp.data_ptr()
        comp_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
        comp2 = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        comp2_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * slot + comp2.data_ptr()
        comp2_sizes = torch.zeros(n, dtype=torch.int64, device=dev)

        def batched_compress():
            assert lib.nvcompBatchedCascadedCompressAsync(in_ptrs.data_ptr(), sizes.data_ptr(), CHUNK, n, temp.data_ptr(), temp_c.value,
                                                          comp_ptrs.data_ptr(), comp_sizes.data_ptr(), opts, s) == 0

        def compress():
            assert k.bench_compress(data.data_ptr(), CHUNK, n, comp2_ptrs.data_ptr(), comp2_sizes.data_ptr(), opts, s) == 0

        batched_compress()
        torch.cuda.synchronize()
        comp_total = int(comp_sizes.sum().item())

        inter = torch.empty(total, dtype=torch.uint8, device=dev)
        inter_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * CHUNK + inter.data_ptr()
        plain_out = torch.empty(total, dtype=torch.uint8, device=dev)
        actual = torch.zeros(n, dtype=torch.int64, device=dev)
        statuses = torch.full((n,), -1, dtype=torch.int32, device=dev)
        st_fused = torch.full((n,), -1, dtype=torch.int32, device=dev)
        st_plain = torch.full((n,), -1, dtype=torch.int32, device=dev)
        sums_two = torch.zeros(n, dtype=torch.int64, device=dev)
        sums_fused = torch.zeros(n, dtype=torch.int64, device=dev)

        def batched():
            assert lib.nvcompBatchedCascadedDecompressAsync(comp_ptrs.data_ptr(), comp_sizes.data_ptr(), sizes.data_ptr(),
                                                            actual.data_ptr(), n, temp.data_ptr(), temp_d.value, inter_ptrs.data_ptr(),
                                                            statuses.data_ptr(), s) == 0

        def two_kernel():
            batched()
            assert k.bench_reduce(inter.data_ptr(), CHUNK, n, lo, hi, sums_two.data_ptr(), s) == 0

        def fused():
            assert k.bench_fused(comp_ptrs.data_ptr(), comp_sizes.data_ptr(), CHUNK, n, lo, hi, sums_fused.data_ptr(),
                                 st_fused.data_ptr(), s) == 0

        def plain():
            assert k.bench_plain(comp_ptrs.data_ptr(), comp_sizes.data_ptr(), plain_out.data_ptr(), CHUNK, n, st_plain.data_ptr(), s) == 0

        paths = {"two_kernel": two_kernel, "fused": fused, "batched": batched, "plain": plain, "batched_compress": batched_compress,
                 "compress": compress}
        ms = {p: [] for p in paths}
        for _ in range(args.repeats):  # alternate the paths so that drift on the card hits all alike
            for p, fn in paths.items():
                for _ in range(args.warmup):
                    fn()
                for _ in range(args.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    ms[p].append(e0.elapsed_time(e1))
        torch.cuda.synchronize()

        refused = int((st_fused != 0).sum().item()) + int((st_plain != 0).sum().item())
        ok = bool((statuses == 0).all().item()) and refused == 0
        ok = ok and torch.equal(sums_two, sums_fused) and bool((sums_fused != 0).any().item())
        ok = ok and torch.equal(plain_out, inter) and torch.equal(inter, data)
        ok = ok and torch.equal(comp_sizes, comp2_sizes)
        if ok:
            keep = (torch.arange(slot, device=dev)[None, :] < comp_sizes[:, None])
            ok = bool(((comp.view(n, slot) == comp2.view(n, slot)) | ~keep).all().item())
        all_ok = all_ok and ok

        def gbps(v):
            return round(total / (np.median(v) * 1e-3) / 1e9, 1)

        res = {"metric": "cascaded_device_fused_filter_sum", "input": name, "unit": "GB/s (uncompressed bytes)", "bytes": total,
               "chunks": n, "chunk_bytes": CHUNK, "opts": [4096, 4, 2, 1, 1], "ratio": round(total / comp_total, 4),
               "filter": [lo, hi], "steps": args.steps * args.repeats, "warmup": args.warmup, "batched_library": args.lib or "this tree",
               # HBM bytes a call must move: the fused path reads the streams and writes 8 bytes a chunk; the two-kernel path
               # also writes the column and reads it back
               "bytes_moved": {"fused": comp_total + 8 * n, "two_kernel": comp_total + 2 * total + 8 * n, "batched": comp_total + total},
               "fused_bound_over_two_kernel": round((comp_total + 2 * total + 8 * n) / (comp_total + 8 * n), 2),
               **{f"{p}_gbps": gbps(v) for p, v in ms.items()},
               **{f"{p}_ms_min_median_max": [round(min(v), 4), round(float(np.median(v)), 4), round(max(v), 4)] for p, v in ms.items()},
               "fused_over_two_kernel": round(float(np.median(ms["two_kernel"]) / np.median(ms["fused"])), 3),
               "fused_over_batched": round(float(np.median(ms["batched"]) / np.median(ms["fused"])), 3),
               "plain_over_batched": round(float(np.median(ms["batched"]) / np.median(ms["plain"])), 3),
               "compress_over_batched_compress": round(float(np.median(ms["batched_compress"]) / np.median(ms["compress"])), 3),
               "chunks_refused_for_lds": refused, "kernel_resources": resources, "verified": ok}
        print(json.dumps(res), flush=True)
        del data, comp, comp2, inter, plain_out
        torch.cuda.empty_cache()
    if not all_ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
