#!/usr/bin/env python3
"""The compressor of the device-side LZ4 API (include/nvcomp/device/lz4.hpp) against the batched call, alone and fused
behind a producer.

Workloads, each 16 384 chunks of 64 KiB (1 GiB): the mix (nvcomp_amd.datasets.silesia_style) and the int32 column
(nvcomp_amd.datasets.int32_column). 64 MiB are generated on the host and laid out 16 times over. The producer is a byte
shuffle: the chunk's 4-byte elements transposed into four planes.

  (a) plain   compress() global -> global in a user kernel, against nvcompBatchedLZ4CompressAsync on the same buffers;
  (b) fused   one user kernel shuffles each chunk into 64 KiB of LDS and compresses it from there, against the two-kernel
              path: a shuffle kernel writes the planes to HBM, the batched call compresses them.

Every (workload, leg) pair runs in a process of its own under its own `timeout`, one after the other, chained with `&&`:
the first one that fails or runs out of time ends the run. Each call is timed with HIP events around it; GB/s are
uncompressed bytes over the median time. The two paths of a leg alternate, in --repeats rounds. Every path's blocks are
decoded again with nvcompBatchedLZ4DecompressAsync and compared with what went in. One JSON line per pair, printed and
written to --record (default profiles/lz4_device_compress_bench.jsonl)."""
import argparse
import ctypes as C
import json
import os
import re
import shlex
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SRC = os.path.join(REPO, "scripts", "bench_lz4_device_compress.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CHUNK = 1 << 16
KERNELS = ("plain_compress", "fused_shuffle", "shuffle_to_hbm")
WORKLOADS = {"mix": "silesia_style", "int32_column": "int32_column"}
LEGS = ("plain", "fused")


def build(out_dir):
    """Compile the kernels; return (library path, resource use per kernel)."""
    so = os.path.join(out_dir, "bench_lz4_device_compress.so")
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


def run_one(args, workload, leg):
    """One leg of one workload, in this process."""
    import torch  # first: its HIP runtime must be the one resident when the two libraries are loaded

    import nvcomp_amd
    from nvcomp_amd import datasets
    from nvcomp_amd._lib import OPTS

    k = C.CDLL(args.so)
    vp, sz = C.c_void_p, C.c_size_t
    k.bench_plain.argtypes = [vp, sz, vp, sz, vp, vp]
    k.bench_fused.argtypes = [vp, sz, vp, sz, vp, vp]
    k.bench_shuffle.argtypes = [vp, sz, vp, vp]
    k.bench_slot_bytes.restype = sz
    lib = nvcomp_amd.load_library()
    opts = OPTS["LZ4"](0)

    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream(dev)
    s = C.c_void_p(stream.cuda_stream)
    n = args.chunks
    total = n * CHUNK
    size = min(args.unique_mib << 20, total)
    unique = np.ascontiguousarray(getattr(datasets, WORKLOADS[workload])(size, 11)).view(np.uint8).reshape(-1)[:size].copy()
    data = torch.from_numpy(unique).to(dev).repeat(-(-total // size))[:total].contiguous()
    slot = int(k.bench_slot_bytes())
    mb = C.c_size_t(0)
    assert lib.nvcompBatchedLZ4CompressGetMaxOutputChunkSize(CHUNK, opts, C.byref(mb)) == 0 and mb.value == slot

    def i64(v):
        return torch.from_numpy(np.asarray(v, dtype=np.int64)).to(dev)

    idx = np.arange(n, dtype=np.int64)
    sizes = i64(np.full(n, CHUNK))
    comp = {p: torch.empty(n * slot, dtype=torch.uint8, device=dev) for p in ("ours", "batched")}
    comp_ptrs = {p: i64(idx * slot + t.data_ptr()) for p, t in comp.items()}
    comp_bytes = {p: torch.zeros(n, dtype=torch.int64, device=dev) for p in comp}
    shuffled = torch.empty(total, dtype=torch.uint8, device=dev) if leg == "fused" else None
    batched_in = i64(idx * CHUNK + (shuffled if leg == "fused" else data).data_ptr())
    tb = C.c_size_t(0)
    assert lib.nvcompBatchedLZ4CompressGetTempSize(n, CHUNK, opts, C.byref(tb)) == 0
    temp = torch.empty(max(tb.value, 4), dtype=torch.uint8, device=dev)

    def batched():
        rc = lib.nvcompBatchedLZ4CompressAsync(batched_in.data_ptr(), sizes.data_ptr(), CHUNK, n, temp.data_ptr(), tb.value,
                                               comp_ptrs["batched"].data_ptr(), comp_bytes["batched"].data_ptr(), opts, s)
        if rc != 0:
            sys.exit(f"nvcompBatchedLZ4CompressAsync returned {rc}")

    def two_kernel():
        assert k.bench_shuffle(data.data_ptr(), n, shuffled.data_ptr(), s) == 0
        batched()

    def plain():
        assert k.bench_plain(data.data_ptr(), n, comp["ours"].data_ptr(), slot, comp_bytes["ours"].data_ptr(), s) == 0

    def fused():
        assert k.bench_fused(data.data_ptr(), n, comp["ours"].data_ptr(), slot, comp_bytes["ours"].data_ptr(), s) == 0

    ours, theirs = (("plain", plain), ("batched", batched)) if leg == "plain" else (("fused", fused), ("two_kernel", two_kernel))
    paths = dict([theirs, ours])
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

    # the way back: both paths' blocks through the batched decoder
    want = shuffled if leg == "fused" else data
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    out_ptrs = i64(idx * CHUNK + out.data_ptr())
    actual = torch.zeros(n, dtype=torch.int64, device=dev)
    statuses = torch.full((n,), -1, dtype=torch.int32, device=dev)
    db = C.c_size_t(0)
    assert lib.nvcompBatchedLZ4DecompressGetTempSize(n, CHUNK, C.byref(db)) == 0
    dtemp = torch.empty(max(db.value, 4), dtype=torch.uint8, device=dev)
    ok = True
    totals = {}
    for p in comp:
        out.zero_()
        rc = lib.nvcompBatchedLZ4DecompressAsync(comp_ptrs[p].data_ptr(), comp_bytes[p].data_ptr(), sizes.data_ptr(), actual.data_ptr(),
                                                 n, dtemp.data_ptr(), db.value, out_ptrs.data_ptr(), statuses.data_ptr(), s)
        torch.cuda.synchronize()
        ok = ok and rc == 0 and bool((statuses == 0).all().item()) and bool((actual == CHUNK).all().item()) and torch.equal(out, want)
        ok = ok and bool(((comp_bytes[p] >= 1) & (comp_bytes[p] <= slot)).all().item())
        totals[p] = int(comp_bytes[p].sum().item())

    def gbps(v):
        return round(total / (np.median(v) * 1e-3) / 1e9, 2)

    res = {"metric": f"lz4_device_compress_{workload}_{leg}", "unit": "GB/s (uncompressed bytes)", "bytes": total, "chunks": n,
           "chunk_bytes": CHUNK, "input": "byte-shuffled 4-byte elements" if leg == "fused" else "as generated",
           "steps": args.steps * args.repeats, "warmup": args.warmup,
           **{f"{p}_gbps": gbps(v) for p, v in ms.items()},
           **{f"{p}_ms_min_median_max": [round(min(v), 4), round(float(np.median(v)), 4), round(max(v), 4)] for p, v in ms.items()},
           f"{ours[0]}_over_{theirs[0]}": round(float(np.median(ms[theirs[0]]) / np.median(ms[ours[0]])), 3),
           f"{ours[0]}_ratio": round(total / totals["ours"], 4), f"{theirs[0]}_ratio": round(total / totals["batched"], 4),
           "kernel_resources": json.loads(args.resources) if args.resources else None, "verified": ok}
    line = json.dumps(res)
    print(line, flush=True)
    if args.record:
        os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
        with open(args.record, "a") as f:
            f.write(line + "\n")
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--chunks", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--unique-mib", type=int, default=64, help="MiB generated on the host, then repeated")
    ap.add_argument("--record", default=os.path.join(REPO, "profiles", "lz4_device_compress_bench.jsonl"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds one (workload, leg) pair may take")
    ap.add_argument("--so", default=None, help="the kernels, already built (default: built into a temporary directory)")
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)  # WORKLOAD:LEG, in this process
    ap.add_argument("--resources", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()

    if args.one:
        workload, leg = args.one.split(":")
        sys.exit(0 if run_one(args, workload, leg) else 1)

    resources = json.loads(args.resources) if args.resources else None
    if args.so is None:
        args.so, resources = build(tempfile.mkdtemp(prefix="bench_lz4_device_compress_"))
    os.makedirs(os.path.dirname(os.path.abspath(args.record)), exist_ok=True)
    open(args.record, "w").close()  # the pairs append to it
    common = [sys.executable, os.path.abspath(__file__), "--so", args.so, "--chunks", str(args.chunks), "--steps", str(args.steps),
              "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--unique-mib", str(args.unique_mib), "--record", args.record]
    if resources:
        common += ["--resources", json.dumps(resources)]
    steps = [shlex.join(["timeout", "-k", "10", str(args.timeout), *common, "--one", f"{w}:{leg}"]) for w in WORKLOADS for leg in LEGS]
    sys.exit(subprocess.run(["bash", "-c", " && ".join(steps)]).returncode)


if __name__ == "__main__":
    main()
