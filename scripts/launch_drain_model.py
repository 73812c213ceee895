#!/usr/bin/env python3
"""CPU model of how a persistent LZ4 decode launch empties (common/lz_launch.hip.h, common/lz_order.hip.h): the launch
time of the headline mix for several orders in which the ticket counter hands out the chunks.

The chunks are liblz4 HC-12 streams of nvcomp_amd.datasets.silesia_style (a sample of --sample chunks, repeated to the
batch size as bench.py repeats its 1 024). A chunk costs 0.03 ms + 0.62 ms x sequences / 6 035 on a wave of a full card
(the text chunk's 0.62 ms is its own instruction stream). The launch's waves (28 per CU on 256 CUs)
take the first places statically and the others by ticket, in the order under test. While tickets remain the card is full
and every wave runs at the full-card rate; once they run out, the waves left run faster as the card empties, by the
measured curve of section 4 (4 / 8 / 16 / 28 waves per CU: 153 / 294 / 512 / 674 GB/s, i.e. 1.59 / 1.53 / 1.33 / 1.0
of the full card's rate per wave).

Orders: index order; true cost, descending; the size key of common/lz_order.hip.h (compressed size, 0 for chunks stored
nearly raw) sorted exactly, in 2 / 4 / 32 equal buckets and in the shipped eight buckets per octave; and the shipped
order, which sorts only the last places (one and two rounds of the resident waves) and leaves the bulk in index order.

WHAT THE MODEL LEAVES OUT, and the card shows: a wave's rate also depends on WHAT the other waves run. With the whole
launch by descending size the card runs text chunks alone, then run-like chunks alone (the supposed cause; only the
end-to-end time was measured), and the launch is 2.6 % slower than index order where the model says 4 % faster; with only
the last round sorted the bulk keeps the mix and the launch gains 1.7 %. The model speaks about the
tail and is blind to the bulk. Its sample is small: 128 chunks repeated make groups of hundreds of equal keys.

CPU only; needs the reference-side liblz4 shim (oracle/_ref). A plain run prints the table of DESIGN.md section 6.

usage: launch_drain_model.py [--sample 128] [--batches 8192,16384,65536]
"""
import argparse
import heapq
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

CHUNK = 1 << 16
CUS, WAVES_PER_CU = 256, 28
RATE = [(0.0, 1.59), (4.0, 1.59), (8.0, 1.53), (16.0, 1.33), (28.0, 1.0)]  # waves per CU -> a wave's rate


def rate(waves):
    per_cu = waves / CUS
    for (x0, y0), (x1, y1) in zip(RATE, RATE[1:]):
        if per_cu <= x1:
            return y0 + (y1 - y0) * (per_cu - x0) / (x1 - x0)
    return 1.0


def launch_ms(cost, order, waves=CUS * WAVES_PER_CU):
    """Chunks handed out in `order` to `waves` servers. All running waves progress at the same rate, so the hand-out is
    list scheduling in units of full-card time; the time after the last ticket is stretched by the rate of what is left."""
    jobs = cost[order]
    busy = [float(c) for c in jobs[:waves]]
    heapq.heapify(busy)
    for c in jobs[waves:]:
        heapq.heapreplace(busy, busy[0] + float(c))
    now = busy[0] if len(jobs) > waves else 0.0  # the last ticket is drawn when a wave first comes free after it
    real = now
    ends = sorted(busy)
    for k, end in enumerate(ends):
        if end > now:
            real += (end - now) / rate(len(ends) - k)
            now = end
    return real


def size_key(in_len, cap):
    return np.where(in_len * 10 >= cap * 9, 0, in_len)


def octave_bucket(key):
    """common/lz_order.hip.h: eight buckets per octave."""
    key = np.asarray(key, dtype=np.int64)
    e = np.floor(np.log2(np.maximum(key, 1))).astype(np.int64)
    return np.where(key < 8, key, (e - 2) * 8 + ((key >> np.maximum(e - 3, 0)) & 7))


def descending(key):
    return np.argsort(-np.asarray(key, dtype=np.float64), kind="stable")


def tail_only(bucket, n, tail):
    first = max(n - tail, 0)
    return np.concatenate([np.arange(first), first + descending(bucket[first:])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", type=int, default=128)
    ap.add_argument("--batches", default="8192,16384,65536")
    a = ap.parse_args()
    from nvcomp_amd import datasets
    from oracle import oracle_py as oracle
    from window_history_model import lz4_sequences

    oracle.build()
    if not oracle.have_ref():
        raise SystemExit("needs liblz4 (oracle/_ref): the streams are LZ4_compress_HC(12)'s")
    chunks = datasets.split_chunks(datasets.silesia_style(a.sample * CHUNK, 0), CHUNK)
    comp = [oracle.ref_lz4_compress(c, 12) for c in chunks]
    seqs = np.array([len(lz4_sequences(c)) for c in comp], dtype=np.float64)
    in_len = np.array([c.size for c in comp], dtype=np.int64)
    cost1 = 0.03 + 0.62 * seqs / 6035.0
    key1 = size_key(in_len, np.full(len(comp), CHUNK, dtype=np.int64))
    print(f"{len(comp)} chunks: {seqs.min():.0f} ... {seqs.max():.0f} sequences, cost {cost1.min():.3f} ... {cost1.max():.3f} ms, "
          f"{int((key1 == 0).sum())} stored nearly raw; correlation of size key and cost {np.corrcoef(key1, cost1)[0, 1]:.3f}")
    waves = CUS * WAVES_PER_CU
    print("| hand-out order | " + " | ".join(f"{int(n):,} chunks".replace(",", " ") for n in a.batches.split(",")) + " |")
    print("|---|" + "---|" * len(a.batches.split(",")))
    rows = {}
    for n in (int(x) for x in a.batches.split(",")):
        reps = -(-n // len(comp))
        cost, key = np.tile(cost1, reps)[:n], np.tile(key1, reps)[:n]
        full = cost.sum() / waves
        top = int(key.max()) + 1
        orders = [("index order", np.arange(n)), ("true cost, descending", descending(cost)), ("size key, sorted", descending(key))]
        orders += [(f"size key, {b} equal buckets", descending(key * b // top)) for b in (2, 4, 32)]
        orders += [("size key, eight buckets per octave", descending(octave_bucket(key)))]
        orders += [(f"... for the last {r} x {waves} places only (shipped: 1)", tail_only(octave_bucket(key), n, r * waves)) for r in (1, 2)]
        base = None
        for name, order in orders:
            ms = launch_ms(cost, order)
            base = ms if base is None else base
            rows.setdefault(name, []).append(f"{ms:.2f} ms, {100 * (ms / full - 1):+.1f} % of full, {100 * (ms / base - 1):+.1f} %")
    for name, cells in rows.items():
        print(f"| {name} | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
