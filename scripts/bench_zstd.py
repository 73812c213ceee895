#!/usr/bin/env python3
"""Batched Zstd decode throughput on the card: uncompressed GB/s of nvcompBatchedZstdDecompressAsync, timed with HIP
events around the call, for 64 KiB chunks written by CPU libzstd (nvcomp_amd/zstd_cpu.py) at levels 1 / 3 / 19.

Inputs: the dataset mix (nvcomp_amd.datasets.silesia_style, every CLASSES entry) and the int32, zeros and noise classes
on their own, at 16 384 and 65 536 chunks. The CPU compresses `--unique` distinct chunks per input (level 19 costs
seconds per MiB); a batch points its chunks at them round-robin, every chunk with its own output slot, so the card
decodes as many chunks as the batch names. HBM fraction as bench.py computes its roofline: (compressed + uncompressed +
44 B per chunk) / kernel time against 8 TB/s. Host baseline: libzstd's ZSTD_decompress on 16 threads over the unique
chunks. `--trace`: re-runs itself under rocprofv3 --kernel-trace --stats (a run of its own) for the kernel time, writing to
`--trace-dir`.
Prints one JSON line per (input, level, chunks) and exits non-zero when libzstd cannot be loaded."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBPS = 8000.0
CHUNK = 65536


def host_baseline(comps, sizes, threads=16, reps=3):
    from nvcomp_amd import zstd_cpu

    lib = zstd_cpu.load()
    outs = [np.empty(s, np.uint8) for s in sizes]
    srcs = [np.ascontiguousarray(c) for c in comps]

    def work(idx):
        for i in idx:
            lib.ZSTD_decompress(outs[i].ctypes.data, outs[i].size, srcs[i].ctypes.data, srcs[i].size)

    parts = [list(range(t, len(comps), threads)) for t in range(threads)]
    best = float("inf")
    with ThreadPoolExecutor(threads) as ex:
        for _ in range(reps):
            t0 = time.perf_counter()
            list(ex.map(work, parts))
            best = min(best, time.perf_counter() - t0)
    return sum(sizes) / best / 1e9


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chunks", type=int, nargs="+", default=[16384, 65536])
    ap.add_argument("--levels", type=int, nargs="+", default=[1, 3, 19])
    ap.add_argument("--inputs", nargs="+", default=["mix", "int32", "zeros", "noise"])
    ap.add_argument("--unique", type=int, default=512, help="distinct chunks compressed on the CPU per input and level")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace", action="store_true", help="re-run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--trace-dir", default=os.path.join(REPO, "build", "zstd_trace"),
                    help="where rocprofv3 writes its trace and statistics (default: build/zstd_trace, not tracked)")
    args = ap.parse_args()

    from nvcomp_amd import datasets, zstd_cpu

    if zstd_cpu.load() is None:
        print("bench_zstd: libzstd cannot be loaded; no measurement without the CPU producer", file=sys.stderr)
        sys.exit(2)
    if args.trace:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", os.path.abspath(args.trace_dir), "-o", "zstd", "--", sys.executable,
               os.path.abspath(__file__), "--chunks", str(args.chunks[0]), "--levels", "3", "--inputs", "mix",
               "--steps", "3", "--warmup", "1", "--unique", str(args.unique)]
        sys.exit(subprocess.call(cmd))

    import torch

    import nvcomp_amd
    from nvcomp_amd.batched import BatchedCodec

    lib = nvcomp_amd.load_library()
    dev = nvcomp_amd.TorchDevice("cuda:0")
    codec = BatchedCodec(lib, dev, "Zstd")
    stream = torch.cuda.current_stream()
    print(json.dumps({"libzstd": zstd_cpu.version(), "device": torch.cuda.get_device_name(0)}), flush=True)
    for name in args.inputs:
        if name == "mix":
            data = datasets.silesia_style(args.unique * CHUNK, seed=5)
        else:
            data = datasets.CLASSES[name](args.unique * CHUNK, 5)
        chunks = datasets.split_chunks(data)
        for level in args.levels:
            t0 = time.perf_counter()
            with ThreadPoolExecutor(16) as ex:
                comps = list(ex.map(lambda c: zstd_cpu.compress(c, level), chunks))
            t_comp = time.perf_counter() - t0
            cpu = host_baseline(comps, [c.size for c in chunks])
            # the unique compressed chunks once on the card
            offs = np.cumsum([0] + [c.size for c in comps])
            comp_slab = torch.from_numpy(np.concatenate(comps)).to("cuda:0")
            comp_ptrs_u = np.array([comp_slab.data_ptr() + int(o) for o in offs[:-1]], np.uint64)
            comp_sizes_u = np.array([c.size for c in comps], np.uint64)
            for n in args.chunks:
                idx = np.arange(n) % len(comps)
                raw_sizes = np.array([chunks[i].size for i in idx], np.uint64)
                out = torch.empty(n * CHUNK, dtype=torch.uint8, device="cuda:0")
                ptrs = torch.from_numpy(comp_ptrs_u[idx].view(np.int64)).to("cuda:0")
                csz = torch.from_numpy(comp_sizes_u[idx].view(np.int64)).to("cuda:0")
                osz = torch.from_numpy(raw_sizes.view(np.int64)).to("cuda:0")
                optrs = torch.from_numpy((np.arange(n, dtype=np.uint64) * CHUNK + out.data_ptr()).view(np.int64)).to("cuda:0")
                act = torch.zeros(n, dtype=torch.int64, device="cuda:0")
                st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
                tb = codec.decompress_temp_size(n, CHUNK)
                temp = torch.empty(tb, dtype=torch.uint8, device="cuda:0")
                fn = lib.nvcompBatchedZstdDecompressAsync

                def call():
                    rc = fn(ptrs.data_ptr(), csz.data_ptr(), osz.data_ptr(), act.data_ptr(), n, temp.data_ptr(), tb,
                            optrs.data_ptr(), st.data_ptr(), C.c_void_p(stream.cuda_stream))
                    assert rc == 0, rc

                for _ in range(args.warmup):
                    call()
                torch.cuda.synchronize()
                ok = bool((st == 0).all().item()) and bool((act.cpu().numpy().view(np.uint64) == raw_sizes).all())
                host_out = out.cpu().numpy()
                for k in range(0, n, max(1, n // 64)):  # a sample of the outputs, byte for byte
                    ok = ok and np.array_equal(host_out[k * CHUNK: k * CHUNK + chunks[idx[k]].size], chunks[idx[k]])
                times = []
                for _ in range(args.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call()
                    e1.record(stream)
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1))
                ms = float(np.median(times))
                raw = int(raw_sizes.sum())
                compb = int(comp_sizes_u[idx].sum())
                gbps = raw / ms / 1e6
                alg = compb + raw + 44 * n
                print(json.dumps({
                    "input": name, "level": level, "chunks": n, "chunk_bytes": CHUNK, "ratio": round(raw / compb, 3),
                    "GBps": round(gbps, 2), "ms": round(ms, 3), "verified": ok,
                    "hbm_frac": round(alg / ms / 1e6 / HBM_PEAK_GBPS, 4),
                    "libzstd_16t_GBps": round(cpu, 2), "vs_libzstd_16t": round(gbps / cpu, 2),
                    "unique_chunks": len(comps), "cpu_compress_s": round(t_comp, 1)}), flush=True)
                del out, temp
            del comp_slab
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
