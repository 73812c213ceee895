#!/usr/bin/env python3
"""Batched CRC-32 throughput on the card: input GB/s of nvcompBatchedCRC32Async (include/nvcomp/crc32.h), timed with HIP
events around the call, for four shapes:

  mix      65 536 x 64 KiB of the dataset mix (4 GiB: 64 MiB of nvcomp_amd.datasets.silesia_style, 64 times over);
  1x1GiB   one chunk of 1 GiB, random bytes;
  16x64MiB sixteen chunks of 64 MiB, random bytes;
  1Mx512B  1 048 576 chunks of 512 bytes, random bytes.

Every result is checked against Python's zlib.crc32, and that host computation is timed too (one thread, on the bytes
downloaded from the card; the mix on its 64 MiB of distinct bytes). HBM fraction: input bytes / time against 8 TB/s.
Prints one JSON line per shape; exits non-zero when a checksum differs."""
import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

HBM_PEAK_GBPS = 8000.0
SHAPES = ("mix", "1x1GiB", "16x64MiB", "1Mx512B")


def host_crcs(host, sizes, offsets):
    t0 = time.perf_counter()
    out = [zlib.crc32(host[o: o + s]) & 0xFFFFFFFF for o, s in zip(offsets, sizes)]
    return out, time.perf_counter() - t0


def make_shape(torch, name):
    """(device bytes, chunk sizes, chunk offsets, expected CRCs, host seconds, host bytes)"""
    if name == "mix":
        from nvcomp_amd import datasets

        unique = datasets.silesia_style(64 << 20, seed=11)
        n = unique.size // 65536
        exp, secs = host_crcs(memoryview(unique), [65536] * n, [65536 * i for i in range(n)])
        slab = torch.from_numpy(unique).cuda().repeat(64)
        return slab, [65536] * (64 * n), [65536 * i for i in range(64 * n)], exp * 64, secs, unique.size
    count, size = {"1x1GiB": (1, 1 << 30), "16x64MiB": (16, 64 << 20), "1Mx512B": (1 << 20, 512)}[name]
    g = torch.Generator(device="cuda").manual_seed(7)
    slab = torch.randint(0, 256, (count * size,), dtype=torch.uint8, device="cuda", generator=g)
    host = memoryview(slab.cpu().numpy())
    offsets = [i * size for i in range(count)]
    exp, secs = host_crcs(host, [size] * count, offsets)
    return slab, [size] * count, offsets, exp, secs, count * size


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=SHAPES)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    import nvcomp_amd

    lib = nvcomp_amd.load_library()
    stream = torch.cuda.current_stream()
    print(json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)
    ok = True
    for name in args.shapes:
        slab, sizes, offsets, expect, host_s, host_bytes = make_shape(torch, name)
        n = len(sizes)
        base = slab.data_ptr()
        ptrs = torch.tensor([base + o for o in offsets], dtype=torch.int64, device="cuda")
        szs = torch.tensor(sizes, dtype=torch.int64, device="cuda")
        out = torch.empty(n, dtype=torch.int32, device="cuda")

        def call():
            rc = lib.nvcompBatchedCRC32Async(ptrs.data_ptr(), szs.data_ptr(), n, out.data_ptr(), stream.cuda_stream)
            if rc != 0:
                raise RuntimeError(f"nvcompBatchedCRC32Async returned {rc}")

        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            times.append(a.elapsed_time(b) / 1e3)
        got = (out.cpu().numpy().view(np.uint32)).tolist()
        bad = sum(g != e for g, e in zip(got, expect))
        ok &= bad == 0
        total = sum(sizes)
        med = float(np.median(times))
        gbps = total / med / 1e9
        print(json.dumps({
            "shape": name, "chunks": n, "bytes": total, "median_ms": round(med * 1e3, 4),
            "best_ms": round(min(times) * 1e3, 4), "gbps": round(gbps, 1), "gbps_best": round(total / min(times) / 1e9, 1),
            "hbm_fraction": round(gbps / HBM_PEAK_GBPS, 3), "host_zlib_gbps": round(host_bytes / host_s / 1e9, 2),
            "wrong": bad}), flush=True)
        del slab, ptrs, szs, out
        torch.cuda.empty_cache()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
