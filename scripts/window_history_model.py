#!/usr/bin/env python3
"""CPU model of the output window's history (common/lz_window.hip.h, common/lz_out_window.hip.h): of the far matches
of the headline workload -- short matches whose source is flushed --, how many have their whole source in what the
window still holds, and what a slide that keeps more history buys and costs.

The model follows the one-wave LZ4 decoder's batching: sequences are taken 64 at a time (refilled when fewer than 24 are
in hand), a batch ends at 64 sequences or kBatchMax bytes, out_make_room slides only when the batch does not fit and
keeps min(keep target, what the batch leaves room for), the flushed mark is the batch's end rounded down to 16 bytes, a
sequence with a literal run or a match of 4 KiB goes past the window, which restarts behind it. Output buffers are taken
as 16-byte aligned. The run executor is not modelled: the inputs are the mix's five text-like classes (liblz4 HC-12
streams of nvcomp_amd.datasets, weighted by SILESIA_STYLE_MIX), which never reach it.

CPU only; a plain run prints the table of DESIGN.md 3.1.

usage: window_history_model.py [--chunks 16] [--keeps 32,64,128,256,512,768,1024,4096]
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCH_MAX, KEEP, OUT_WIN = 2048, 32, 2048 + 64 + 32  # common/lz_ring.hip.h
STREAM = 4096                                        # common/lz_stream.hip.h
MATCH_SHORT, REFILL_BELOW = 32, 24
TEXT_LIKE = ("text", "table", "float_csv", "float32", "lowcard")


def lz4_sequences(block):
    """(literal length, offset, match length) of every sequence of an LZ4 block; the last one has no match."""
    b, i, n, out = bytes(block), 0, len(block), []
    while i < n:
        token = b[i]
        i += 1
        lit = token >> 4
        if lit == 15:
            while True:
                lit += b[i]
                i += 1
                if b[i - 1] != 255:
                    break
        i += lit
        if i >= n:
            out.append((lit, 0, 0))
            break
        off = b[i] | (b[i + 1] << 8)
        i += 2
        mlen = (token & 15) + 4
        if mlen == 19:
            while True:
                mlen += b[i]
                i += 1
                if b[i - 1] != 255:
                    break
        out.append((lit, off, mlen))
    return out


def model_chunk(seqs, keep_target, st):
    op = wbase = valid_lo = flushed = 0
    at, count = 0, 0
    while at < len(seqs):
        if count < REFILL_BELOW:
            count = min(64, len(seqs) - at)
        lit, off, mlen = seqs[at]
        if lit >= STREAM or mlen >= STREAM or lit + mlen > BATCH_MAX:  # stream_sequence: the window restarts
            op += lit + mlen
            wbase, valid_lo, flushed = op & ~15, op, op
            at, count = at + 1, count - 1
            continue
        take = total = 0
        while take < count:
            l, _, m = seqs[at + take]
            if total + l + m > BATCH_MAX or l >= STREAM or m >= STREAM:
                break
            total += l + m
            take += 1
        st["batches"] += 1
        if op - wbase + total > OUT_WIN:  # out_make_room
            keep = min(keep_target, OUT_WIN - 30 - total)
            new_base = max(min(max(op - keep, 0), flushed), valid_lo) & ~15
            if new_base != wbase:
                st["slides"] += 1
                st["slide_bytes"] += op - new_base
                wbase, valid_lo = new_base, max(valid_lo, new_base)
        pos = op
        for l, o, m in seqs[at: at + take]:
            dst = pos + l
            pos = dst + m
            if not 4 <= m <= MATCH_SHORT:
                continue
            st["short"] += 1
            src = dst - o
            if src + m <= flushed:  # the parent fetched every one of these
                st["final"] += 1
                if src >= valid_lo and o >= 4:
                    st["held"] += 1
                    st["held_beyond_512"] += o > 512
        op += total
        flushed = max(flushed, op & ~15)
        at, count = at + take, count - take


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=16, help="64 KiB chunks per class")
    ap.add_argument("--keeps", default="32,64,128,256,512,768,1024,4096")
    a = ap.parse_args()
    from nvcomp_amd import datasets
    from oracle import oracle_py as oracle

    oracle.build()
    assert oracle.have_ref(), "needs liblz4 (the oracle's reference-side shim)"
    shares = dict(datasets.SILESIA_STYLE_MIX)
    per_class = {}
    for name in TEXT_LIKE:
        chunks = datasets.split_chunks(datasets.CLASSES[name](a.chunks * datasets.CHUNK, 0))
        per_class[name] = [lz4_sequences(oracle.ref_lz4_compress(c, 12)) for c in chunks]
    print("| slide keeps | far matches whose source the window holds | ... and offset > 512 B | slides per chunk "
          "| batches per chunk | bytes copied per slide |")
    print("|---|---|---|---|---|---|")
    for keep in [int(k) for k in a.keeps.split(",")]:
        keys = ("batches", "slides", "slide_bytes", "final", "held", "held_beyond_512")
        mix = dict.fromkeys(keys, 0.0)  # per chunk of the mix: a class weighs by its share of the chunks (the other classes add nothing)
        for name in TEXT_LIKE:
            st = dict.fromkeys(keys + ("short",), 0)
            for seqs in per_class[name]:
                model_chunk(seqs, keep, st)
            for k in keys:
                mix[k] += shares[name] * st[k] / len(per_class[name])
        print(f"| {'all that fits' if keep >= OUT_WIN else str(keep) + ' B'} | {100 * mix['held'] / mix['final']:.1f} % "
              f"| {100 * mix['held_beyond_512'] / mix['final']:.1f} % | {mix['slides']:.0f} | {mix['batches']:.0f} "
              f"| {mix['slide_bytes'] / max(mix['slides'], 1e-9):.0f} |")


if __name__ == "__main__":
    main()
