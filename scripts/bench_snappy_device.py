#!/usr/bin/env python3
"""Device-side Snappy (include/nvcomp/device/snappy.hpp) against the batched calls, alone and fused into a consumer.

Workloads, each 16 384 chunks of 64 KiB (1 GiB): the mix (nvcomp_amd.datasets.silesia_style) and the int32 column
(nvcomp_amd.datasets.int32_column), compressed by libsnappy (the oracle's C restatement where libsnappy is not built). 64 MiB
are generated and compressed on the host; the compressed chunks are laid out 16 times over. The consumer is a 256-bin byte
histogram per chunk.

  (a) plain       decompress() global -> global in a user kernel, against nvcompBatchedSnappyDecompressAsync on the same
                  buffers;
  (b) fused       one user kernel decodes each chunk into 64 KiB of LDS and counts it there, against the two-kernel path:
                  the batched call writes the chunks to HBM, a histogram kernel reads them;
  (c) compress    compress() global -> global in a user kernel, against nvcompBatchedSnappyCompressAsync on the same chunks.

--lib PATH takes the batched calls from another build of libnvcomp.so. Each call is timed with HIP events around it; GB/s
are uncompressed bytes over the median time. The paths alternate, in --repeats rounds. plain is checked to give the batched
decoder's bytes (the original data), fused the two-kernel path's histograms, compress streams that the batched decoder
turns back into the data. Prints one JSON line per workload."""
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
SRC = os.path.join(REPO, "scripts", "bench_snappy_device.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CHUNK = 1 << 16
SLOT = (32 + CHUNK + CHUNK // 6 + 15) // 16 * 16
KERNELS = ("plain_decompress", "fused_histogram", "histogram_from_hbm", "plain_compress")


def build(out_dir):
    """Compile the kernels; return (library path, resource use per kernel)."""
    so = os.path.join(out_dir, "bench_snappy_device.so")
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


def compress_on_host(oracle, data):
    from concurrent.futures import ThreadPoolExecutor

    fn = oracle.ref_snappy_compress if oracle.have_ref() else oracle.snappy_compress
    chunks = [data[o: o + CHUNK] for o in range(0, data.size, CHUNK)]
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:  # the C code runs outside the interpreter lock
        return list(pool.map(fn, chunks))


def run(args, k, lib, resources, name, unique, compressor):
    import torch

    from oracle import oracle_py as oracle

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    s = C.c_void_p(stream.cuda_stream)
    n = args.chunks
    total = n * CHUNK
    comp = compress_on_host(oracle, unique)
    u = len(comp)
    offs = np.concatenate([[0], np.cumsum([(c.size + 15) // 16 * 16 for c in comp])]).astype(np.int64)
    slab = np.zeros(int(offs[-1]), dtype=np.uint8)
    for c, o in zip(comp, offs):
        slab[o: o + c.size] = c
    copies = -(-n // u)
    comp_dev = torch.from_numpy(slab).to(dev).repeat(copies).contiguous()
    idx = np.arange(n)
    ptrs = (idx // u) * int(offs[-1]) + offs[idx % u] + comp_dev.data_ptr()
    comp_ptrs = torch.from_numpy(ptrs.astype(np.int64)).to(dev)
    comp_sizes = torch.from_numpy(np.asarray([comp[i % u].size for i in range(n)], dtype=np.int64)).to(dev)
    comp_total = int(comp_sizes.sum().item())
    want = torch.from_numpy(unique).to(dev).repeat(copies)[:total].contiguous()

    caps = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
    inter = torch.empty(total, dtype=torch.uint8, device=dev)
    inter_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * CHUNK + inter.data_ptr()
    plain_out = torch.empty(total, dtype=torch.uint8, device=dev)
    actual = torch.zeros(n, dtype=torch.int64, device=dev)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=dev)
    st_fused = torch.full((n,), -1, dtype=torch.int32, device=dev)
    st_plain = torch.full((n,), -1, dtype=torch.int32, device=dev)
    h_two = torch.zeros(n * 256, dtype=torch.int32, device=dev)
    h_fused = torch.zeros(n * 256, dtype=torch.int32, device=dev)
    tb = C.c_size_t(0)
    assert lib.nvcompBatchedSnappyDecompressGetTempSize(n, CHUNK, C.byref(tb)) == 0
    temp = torch.empty(max(tb.value, 4), dtype=torch.uint8, device=dev)

    # the compressors: the original chunks in, one slot of the bound per chunk out
    raw_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * CHUNK + want.data_ptr()
    raw_sizes = torch.full((n,), CHUNK, dtype=torch.int64, device=dev)
    c_batched = torch.empty(n * SLOT, dtype=torch.uint8, device=dev)
    c_device = torch.empty(n * SLOT, dtype=torch.uint8, device=dev)
    c_batched_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * SLOT + c_batched.data_ptr()
    c_device_ptrs = torch.arange(n, dtype=torch.int64, device=dev) * SLOT + c_device.data_ptr()
    c_batched_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    c_device_sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    ctb = C.c_size_t(0)
    from nvcomp_amd._lib import SnappyOpts

    opts = SnappyOpts(0)
    assert lib.nvcompBatchedSnappyCompressGetTempSize(n, CHUNK, opts, C.byref(ctb)) == 0
    ctemp = torch.empty(max(ctb.value, 4), dtype=torch.uint8, device=dev)

    def batched(src=comp_ptrs, sizes=comp_sizes):
        rc = lib.nvcompBatchedSnappyDecompressAsync(src.data_ptr(), sizes.data_ptr(), caps.data_ptr(), actual.data_ptr(), n,
                                                    temp.data_ptr(), tb.value, inter_ptrs.data_ptr(), statuses.data_ptr(), s)
        if rc != 0:
            sys.exit(f"nvcompBatchedSnappyDecompressAsync returned {rc}")

    def two_kernel():
        batched()
        assert k.bench_histogram(inter.data_ptr(), CHUNK, n, h_two.data_ptr(), s) == 0

    def fused():
        assert k.bench_fused(comp_ptrs.data_ptr(), comp_sizes.data_ptr(), h_fused.data_ptr(), n, st_fused.data_ptr(), s) == 0

    def plain():
        assert k.bench_plain(comp_ptrs.data_ptr(), comp_sizes.data_ptr(), plain_out.data_ptr(), CHUNK, n, st_plain.data_ptr(), s) == 0

    def batched_compress():
        rc = lib.nvcompBatchedSnappyCompressAsync(raw_ptrs.data_ptr(), raw_sizes.data_ptr(), CHUNK, n, ctemp.data_ptr(), ctb.value,
                                                  c_batched_ptrs.data_ptr(), c_batched_sizes.data_ptr(), opts, s)
        if rc != 0:
            sys.exit(f"nvcompBatchedSnappyCompressAsync returned {rc}")

    def plain_compress():
        assert k.bench_compress(want.data_ptr(), CHUNK, n, c_device.data_ptr(), SLOT, c_device_sizes.data_ptr(), s) == 0

    paths = {"two_kernel": two_kernel, "fused": fused, "batched": batched, "plain": plain, "batched_compress": batched_compress,
             "plain_compress": plain_compress}
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

    ok = bool((statuses == 0).all().item() and (st_fused == 0).all().item() and (st_plain == 0).all().item())
    ok = ok and bool((actual == CHUNK).all().item())
    ok = ok and torch.equal(inter, want) and torch.equal(plain_out, want) and torch.equal(h_two, h_fused)
    ok = ok and int(h_fused.sum().item()) == total
    # the device compressor's streams, back through the batched decoder
    inter.zero_()
    batched(c_device_ptrs, c_device_sizes)
    torch.cuda.synchronize()
    ok = ok and bool((statuses == 0).all().item()) and torch.equal(inter, want)
    ok = ok and bool((c_device_sizes > 0).all().item() and (c_device_sizes <= 32 + CHUNK + CHUNK // 6).all().item())

    def gbps(v):
        return round(total / (np.median(v) * 1e-3) / 1e9, 1)

    res = {"metric": "snappy_device_" + name, "unit": "GB/s (uncompressed bytes)", "bytes": total, "chunks": n, "chunk_bytes": CHUNK,
           "compressor": compressor, "ratio": round(total / comp_total, 4),
           "ratio_batched_compress": round(total / int(c_batched_sizes.sum().item()), 4),
           "ratio_device_compress": round(total / int(c_device_sizes.sum().item()), 4),
           "steps": args.steps * args.repeats, "warmup": args.warmup, "batched_library": args.lib or "this tree",
           **{f"{p}_gbps": gbps(v) for p, v in ms.items()},
           **{f"{p}_ms_min_median_max": [round(min(v), 4), round(float(np.median(v)), 4), round(max(v), 4)] for p, v in ms.items()},
           "plain_over_batched": round(float(np.median(ms["batched"]) / np.median(ms["plain"])), 3),
           "fused_over_two_kernel": round(float(np.median(ms["two_kernel"]) / np.median(ms["fused"])), 3),
           "compress_over_batched": round(float(np.median(ms["batched_compress"]) / np.median(ms["plain_compress"])), 3),
           "kernel_resources": resources, "verified": ok}
    print(json.dumps(res), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chunks", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--unique-mib", type=int, default=64, help="MiB generated and compressed on the host, then repeated")
    ap.add_argument("--lib", default=None, help="libnvcomp.so for the batched calls (default: this tree's)")
    args = ap.parse_args()

    import torch  # noqa: F401  first: its HIP runtime must be the one resident when the two libraries are loaded

    import nvcomp_amd
    from nvcomp_amd import datasets
    from oracle import oracle_py as oracle

    oracle.build()
    compressor = "libsnappy" if oracle.have_ref() else "the oracle's C restatement of libsnappy"
    so, resources = build(tempfile.mkdtemp(prefix="bench_snappy_device_"))
    k = C.CDLL(so)
    vp, sz = C.c_void_p, C.c_size_t
    k.bench_plain.argtypes = [vp, vp, vp, sz, sz, vp, vp]
    k.bench_fused.argtypes = [vp, vp, vp, sz, vp, vp]
    k.bench_histogram.argtypes = [vp, sz, sz, vp, vp]
    k.bench_compress.argtypes = [vp, sz, sz, vp, sz, vp, vp]
    lib = nvcomp_amd.load_library(args.lib) if args.lib else nvcomp_amd.load_library()
    size = min(args.unique_mib << 20, args.chunks * CHUNK)
    ok = True
    for name, gen in (("mix", datasets.silesia_style), ("int32_column", datasets.int32_column)):
        unique = np.ascontiguousarray(gen(size, 11)).view(np.uint8).reshape(-1)[:size].copy()
        ok = run(args, k, lib, resources, name, unique, compressor) and ok
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
