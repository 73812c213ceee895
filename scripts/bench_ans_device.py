#!/usr/bin/env python3
"""Device-side ANS (include/nvcomp/device/ans.hpp) fused into its consumer, against the two-kernel path, on the card.

Workload: 1 GiB in 64 KiB chunks (64 MiB of nvcomp_amd.datasets.silesia_style, 16 times over), compressed once with
nvcompBatchedANSCompressAsync. The consumer turns every decoded byte into an fp16 value through a 256-entry codebook.

  two-kernel  nvcompBatchedANSDecompressAsync writes the bytes to HBM, then a lookup kernel reads them back;
  fused       one user kernel decodes each chunk with decompress_to() and looks the bytes up where they are decoded.

Each call is timed with HIP events around it; GB/s are uncompressed bytes over the time. Both outputs are checked
against the codebook applied to the original bytes. Also reports the fused kernel's VGPR / SGPR / LDS / scratch use
(compiler remarks; scratch must be 0). Prints one JSON line."""
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
SRC = os.path.join(REPO, "scripts", "bench_ans_device.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CHUNK = 1 << 16


def build(out_dir):
    """Compile the kernels; return (library path, resource use of the fused kernel)."""
    so = os.path.join(out_dir, "bench_ans_device.so")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(REPO, "include"),
                        "-Rpass-analysis=kernel-resource-usage", SRC, "-o", so], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr[-3000:])
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:\s*)(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key == "Function Name":
            cur = val
            res[cur] = {}
        elif cur is not None:
            res[cur][{"VGPRs": "vgpr", "TotalSGPRs": "sgpr", "ScratchSize [bytes/lane]": "scratch",
                      "LDS Size [bytes/block]": "lds", "Occupancy [waves/SIMD]": "occupancy"}[key]] = int(val)
    fused = next(v for k, v in res.items() if "fused_decode_lookup" in k)
    return so, fused


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    import nvcomp_amd
    from nvcomp_amd import datasets
    from nvcomp_amd._lib import ANSOpts

    tmp = tempfile.mkdtemp(prefix="bench_ans_device_")
    so, resources = build(tmp)
    k = C.CDLL(so)
    vp, sz = C.c_void_p, C.c_size_t
    k.bench_fused.argtypes = [vp, vp, vp, vp, vp, sz, sz, vp, vp]
    k.bench_lookup.argtypes = [vp, vp, vp, sz, C.c_uint, vp]
    lib = nvcomp_amd.load_library()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    s = C.c_void_p(stream.cuda_stream)

    total = int(args.gib * (1 << 30)) // CHUNK * CHUNK
    n = total // CHUNK
    unique = datasets.silesia_style(64 << 20, seed=11)
    reps = -(-total // unique.size)
    data = torch.from_numpy(unique).to(dev).repeat(reps)[:total].contiguous()
    base = data.data_ptr()
    in_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * CHUNK + base
    sizes = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
    max_out = C.c_size_t(0)
    assert lib.nvcompBatchedANSCompressGetMaxOutputChunkSize(CHUNK, ANSOpts(0), C.byref(max_out)) == 0
    comp = torch.empty(n * max_out.value, dtype=torch.uint8, device=dev)
    comp_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * max_out.value + comp.data_ptr()
    comp_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    assert lib.nvcompBatchedANSCompressAsync(in_ptrs.data_ptr(), sizes.data_ptr(), CHUNK, n, None, 0, comp_ptrs.data_ptr(),
                                             comp_sizes.data_ptr(), ANSOpts(0), s) == 0
    torch.cuda.synchronize()
    comp_total = int(comp_sizes.sum().item())

    book = (torch.randn(256, generator=torch.Generator().manual_seed(3)) * 4).to(torch.float16)
    book_dev = book.to(dev)
    book_bits = book_dev.view(torch.int16)
    inter = torch.empty(total, dtype=torch.uint8, device=dev)
    inter_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * CHUNK + inter.data_ptr()
    actual = torch.zeros(n, dtype=torch.int64, device=dev)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=dev)
    out2 = torch.empty(total, dtype=torch.float16, device=dev)
    out1 = torch.empty(total, dtype=torch.float16, device=dev)
    fused_status = torch.full((n,), -1, dtype=torch.int32, device=dev)
    lookup_grid = 256 * 32 * 8

    def two_kernel():
        assert lib.nvcompBatchedANSDecompressAsync(comp_ptrs.data_ptr(), comp_sizes.data_ptr(), sizes.data_ptr(),
                                                   actual.data_ptr(), n, None, 0, inter_ptrs.data_ptr(), statuses.data_ptr(),
                                                   s) == 0
        assert k.bench_lookup(inter.data_ptr(), book_bits.data_ptr(), out2.data_ptr(), total, lookup_grid, s) == 0

    def fused():
        assert k.bench_fused(comp_ptrs.data_ptr(), comp_sizes.data_ptr(), sizes.data_ptr(), book_bits.data_ptr(),
                             out1.data_ptr(), CHUNK, n, fused_status.data_ptr(), s) == 0

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    # alternate the two paths so that drift on the card hits both alike
    ms_two, ms_fused = [], []
    for _ in range(2):
        ms_two += timed(two_kernel)
        ms_fused += timed(fused)
    torch.cuda.synchronize()

    ok = bool((statuses == 0).all().item() and (fused_status == 0).all().item() and (actual == CHUNK).all().item())
    piece = 64 << 20
    for o in range(0, total, piece):
        ref = book_dev[data[o: o + piece].long()]
        ok = ok and torch.equal(out1[o: o + piece], ref) and torch.equal(out2[o: o + piece], ref)

    def gbps(ms):
        return total / (np.median(ms) * 1e-3) / 1e9

    res = {
        "metric": "ans_device_fused_decode_lookup", "unit": "GB/s (uncompressed bytes)", "bytes": total, "chunks": n,
        "chunk_bytes": CHUNK, "ratio": round(total / comp_total, 4), "steps": args.steps * 2, "warmup": args.warmup,
        "two_kernel_gbps": round(gbps(ms_two), 1), "fused_gbps": round(gbps(ms_fused), 1),
        "two_kernel_ms_median": round(float(np.median(ms_two)), 4), "fused_ms_median": round(float(np.median(ms_fused)), 4),
        "two_kernel_ms_min_max": [round(min(ms_two), 4), round(max(ms_two), 4)],
        "fused_ms_min_max": [round(min(ms_fused), 4), round(max(ms_fused), 4)],
        "speedup": round(float(np.median(ms_two) / np.median(ms_fused)), 3),
        "fused_kernel_resources": resources, "verified": ok,
    }
    print(json.dumps(res))
    if not ok or resources.get("scratch", 1) != 0:
        sys.exit(1)


if __name__ == "__main__":
    main()
