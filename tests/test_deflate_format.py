"""The DEFLATE / gzip decoder against streams zlib never writes.

tests/deflate_streams.py writes every stream here from an explicit description and expands that description itself; the
expansion is the reference. zlib checks the writer (test_writer_against_zlib) and is asked for its verdict on every
stream the decoder must refuse (test_refusals_against_zlib). The decoder runs on the emulator and on the card through
the `backend` fixture and BatchedCodec.decompress, whose output slots are followed by guard bytes that must survive.

The cases are built around the decoder's own numbers (deflate/deflate_decode.hip.h): the literal/length lookup of
kLutBits = 10 bits (and 9, the A/B the source names), the distance lookup of kDistLutBits = 8, the speculative window of
kScanWin = 512 bit positions, the stream ring's refill of 512 bytes, batches of 768 bytes and 64 records, literal runs
closed at 192 (between rounds) and 255 (the record's field), and the top jump table's bias of 64 bits (it holds
distances of 64 .. 318 bits).

Where this file departs from the obvious list of cases, and why:
  * HCLEN 4 sends lengths for the code-length symbols 16, 17, 18 and 0 only, so every length of the block is 0 and
    symbol 256 has no code: that header is a refusal case, and 5 (which adds the length 8) is the smallest valid one;
  * the batched entry points always decode with the checks on (api/deflate_api.hip: only the status WRITE depends on
    the caller's pointer), so a wrong ISIZE gives size 0 in the call without statuses too;
  * the gzip size query answers ISIZE for every chunk of at least 18 bytes with the magic number and CM 8, and 0
    otherwise (api/deflate_api.hip: gzip_size_kernel): it does not walk the header;
  * the emulator tier keeps every group, every kind of case and every refusal, and shrinks counts: one of the three
    extra-bit values per symbol and code width (group A), 1 000 literals of 15 bits for 3 000, 64 pairs of 48 bits for
    400, 300 tiny blocks for 3 000, every third remainder of the 258-byte matches and the last ten for all 258, 16
    random streams for 240. The emulator's time goes with table builds (4 ms a block) and with symbols that take the
    wave-uniform path (0.7 ms each), not with bytes; with the card's counts this file would take four times
    tests/test_zstd_format.py's time on the CPU, and it is to take no longer.

Where zlib and the decoder disagree on accepting a stream (also in DESIGN.md): ZLIB_REFUSES below. No stream of this
file is refused by the decoder and decoded by zlib (ZLIB_ACCEPTS is empty, and asserted to be).
"""
import ctypes as C
import os
import random
import re
import sys
import tempfile
import zlib
from collections import namedtuple

import numpy as np
import pytest

import deflate_streams as ds
from deflate_streams import DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, Stream, gzip_member, rnd_bytes
from nvcomp_amd import datasets
from nvcomp_amd._lib import NvcompStatus

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Decoded by the decoder, refused by zlib 1.2 / 1.3:
ZLIB_REFUSES = {
    # RFC 1951 3.2.2 defines a code by its lengths alone ("the Huffman codes used for each alphabet in the 'deflate'
    # format ... are defined by the sequence of bit lengths"); nothing asks that they fill the code space, and 3.2.7
    # itself describes a distance code with "one unused code". zlib accepts an incomplete code only there (one distance
    # code, or none). The decoder's rule: an incomplete code is fine until a bit pattern without a symbol is met.
    "c_incomplete_dist_two_symbols",
    "c_incomplete_litlen",
    # RFC 1952 2.3.1: CRC32 and the header's CRC16 are there for the reader to check; the decoder checks ISIZE only
    # (the library has nvcompBatchedCRC32Async for the callers who want the check).
    "h_crc32_wrong", "h_hcrc_wrong",
}
# Refused by the decoder, decoded by zlib:
ZLIB_ACCEPTS = set()

Case = namedtuple("Case", "name fmt comp out ok cap trace query")  # query: what the size query must answer


def case(name, s, fmt="Deflate", comp=None, cap=None, ok=None, query=None, out=None):
    """A chunk from a Stream (or, with comp / out given, from bytes). Valid unless the stream is marked invalid."""
    ok = (s.invalid is None) if ok is None else ok
    out = (bytes(s.out) if s is not None and s.out is not None else b"") if out is None else bytes(out)
    comp = s.bytes() if comp is None else bytes(comp)
    if cap is None:
        cap = max(len(out), 1) if ok else 4096
    if query is None:
        query = len(out) if ok else 0
    return Case(name, fmt, comp, out if ok else None, ok, cap, s.trace if s is not None else set(), query)


def code(assign, n=286, pool=None, max_bits=15):
    """Code lengths for an alphabet of n symbols: `assign` as told, completed with symbols of `pool` (every other symbol,
    from the top down, by default)."""
    lens = [0] * n
    for s, l in assign.items():
        lens[s] = l
    if pool is None:
        pool = [s for s in range(n - 1, -1, -1) if s not in assign]
    return ds.complete_lengths(lens, pool, max_bits)


def extras(bits, tier, turn):
    """The extra-bit values of a symbol: all zero, all one, random; the emulator tier takes one of them, in turn."""
    if bits == 0:
        return [("zero", 0)]
    kinds = [("zero", 0), ("ones", (1 << bits) - 1), ("rand", random.Random(turn * 16 + bits).randrange(1 << bits))]
    return kinds if tier == "gpu" else [kinds[turn % 3]]


def raw_match(length, distance):
    """A pair as a raw item, for streams marked invalid (the writer expands nothing there)."""
    ls, d = ds.length_symbol(length), ds.distance_symbol(distance)
    return ("pair", ls, length - LEN_BASE[ls - 257], d, distance - DIST_BASE[d])


# ---- group A: every length and distance symbol ----

FRONT = b"\x11\x22\x33\x44\x55\x66\x77\x88"  # eight distinct bytes in front of every length case
LL_WIDTHS = (9, 10, 11, 15)   # on both sides of the lookup (10) and of its A/B (9), and the longest
D_WIDTHS = (7, 8, 9, 15)      # on both sides of the distance lookup (8), and the longest


def _length_case(name, length, ls, width, dist=3):
    # nine literals and the end of block at 4 bits, the length symbol at `width`, fillers complete the code
    ll = code({**{b: 4 for b in FRONT}, 0x5A: 4, 256: 4, ls: width})
    s = Stream()
    s.dynamic([FRONT, (length, dist, ls), 0x5A], ll, code({ds.distance_symbol(dist): 1}, 30), final=True)
    assert s.out[-1] == 0x5A and len(s.out) == 9 + length
    return case(name, s)


def _distance_case(name, dist, dsym, width, length=4, seed=0):
    """Random history of dist - 1 bytes in a stored block, one literal, then the match: it starts at the stream's first
    byte, so one further back is refused and one nearer copies other bytes."""
    ll = code({0x41: 2, 0x5A: 2, 256: 2, ds.length_symbol(length): 2})
    s = Stream()
    s.stored(rnd_bytes(1000 + dist + seed, dist - 1))
    s.dynamic([0x41, (length, dist), 0x5A], ll, code({dsym: width}, 30), final=True)
    assert ds.distance_symbol(dist) == dsym
    return case(name, s)


def group_a(tier):
    out = []
    for wi, width in enumerate(LL_WIDTHS):
        for ls in range(257, 286):
            for tag, x in extras(LEN_EXTRA[ls - 257], tier, ls + wi):
                out.append(_length_case(f"a_len{ls}_{tag}_w{width}", LEN_BASE[ls - 257] + x, ls, width))
        out.append(_length_case(f"a_258_as_284+31_w{width}", 258, 284, width))
        out.append(_length_case(f"a_258_at_1_w{width}", 258, 285, width, dist=1))
    for wi, width in enumerate(D_WIDTHS):
        for d in range(30):
            for tag, x in extras(DIST_EXTRA[d], tier, d + wi):
                out.append(_distance_case(f"a_dist{d}_{tag}_w{width}", DIST_BASE[d] + x, d, width))
        out.append(_distance_case(f"a_3_at_32768_w{width}", 32768, 29, width, length=3))
        out.append(_distance_case(f"a_258_at_32768_w{width}", 32768, 29, width, length=258))
    return out


# ---- group B: symbol widths against the scan ----

def deep_literal_code():
    """Every literal at 15 bits: 256 at 1 bit, 257..262 at 2..7 bits, and 256 codes of 15 bits fill the last 1/128."""
    ll = {256: 1}
    ll.update({257 + i: 2 + i for i in range(6)})
    ll.update({b: 15 for b in range(256)})
    return code(ll)


def pairs48_codes():
    """Literals A / B at 1 / 2 bits, 256 at 3, fillers at 4..14, length symbols 281 and 282 (5 extra bits) at 15; distance
    symbols 28 and 29 (13 extra bits) at 15 behind a chain of 1..14: a pair takes 15 + 5 + 15 + 13 = 48 bits."""
    ll = {0x41: 1, 0x42: 2, 256: 3, 281: 15, 282: 15}
    ll.update({i: 3 + i for i in range(1, 12)})
    dd = {28: 15, 29: 15}
    dd.update({i: 1 + i for i in range(14)})
    return code(ll), code(dd, 30)


def pairs48(with_literals, n=400, seed=48):
    """The shortest lengths with 5 extra bits (131..194): a batch of 768 bytes holds four or five such matches, and what a
    round decoded beyond them it decodes again, so the emulator's time goes with the number of batches."""
    r = random.Random(seed)
    ll, dd = pairs48_codes()
    s = Stream()
    s.stored(rnd_bytes(seed, 32768))
    syms = []
    for _ in range(n):
        ls = 281 if r.random() < 0.9 else 282
        syms.append((LEN_BASE[ls - 257] + r.randrange(32), r.randrange(16385, 32769), ls))
        if with_literals and r.random() < 0.5:
            syms.append(r.choice((0x41, 0x42)))
    s.dynamic(syms, ll, dd, final=True)
    assert {"ll_max:15", "d_max:15"} <= s.trace
    return s, len(syms)


def one_bit_blocks(blocks=7, per_block=700):
    """Blocks of one literal and the end of block at 1 bit each: sixteen symbols take 16 bits, below the top table's bias."""
    s = Stream()
    for k in range(blocks):
        s.dynamic([0x30 + k] * per_block, {0x30 + k: 1, 256: 1}, [0], final=k == blocks - 1)
    return s, blocks * per_block


SAT_LEN = {0: 257, 1: 265, 2: 269, 3: 273, 4: 277, 5: 281}                  # extra bits -> a length symbol
SAT_DIST = {0: 0, 1: 4, 3: 8, 5: 12, 7: 16, 9: 20, 10: 22, 11: 24}          # extra bits -> a distance symbol


def saturating(total, periods=40, seed=0):
    """Pairs the lookups can tell (codes of 4 and 3 bits), sixteen of which take exactly `total` bits, whichever sixteen:
    fifteen of 20 bits and one of total - 300, over and over. 318 is the most a top-table entry holds."""
    r = random.Random(total + seed)
    ll = code({**{s: 4 for s in SAT_LEN.values()}, 0x58: 4, 256: 4})
    dd = code({s: 3 for s in SAT_DIST.values()}, 30)

    def pair(bits):
        le, de = r.choice([(a, b) for a in SAT_LEN for b in SAT_DIST if 7 + a + b == bits])
        ls, d = SAT_LEN[le], SAT_DIST[de]
        return (LEN_BASE[ls - 257] + r.randrange(1 << le), DIST_BASE[d] + r.randrange(1 << de), ls)

    s = Stream()
    s.stored(rnd_bytes(total, 8200))
    s.dynamic([pair(20) if k % 16 else pair(total - 300) for k in range(16 * periods)], ll, dd, final=True)
    return s


def long_code_at_rank(rank, width):
    """64 literals from the start of a block, all of 4 bits but the one at `rank`, which takes `width`."""
    short = list(range(0x61, 0x6F))
    ll = code({**{b: 4 for b in short}, 256: 5, 0x7A: width})
    r = random.Random(rank * 16 + width)
    syms = [r.choice(short) for _ in range(84)]
    syms[rank] = 0x7A
    s = Stream()
    s.dynamic(syms, ll, [0], final=True)
    return s


def group_b(tier):
    """The emulator's time goes with the symbols that take the wave-uniform path (0.7 ms each, and a round that runs into
    the batch's 768 bytes decodes its tail again): a third of the literals and a sixth of the pairs there."""
    out = []
    s = Stream()
    s.dynamic(rnd_bytes(15, 3000 if tier == "gpu" else 1000), deep_literal_code(), [0], final=True)
    assert "ll_max:15" in s.trace
    out.append(case("b_all_15_bit_literals", s))
    pairs = 400 if tier == "gpu" else 64
    out.append(case("b_pairs48", pairs48(False, pairs)[0]))
    out.append(case("b_pairs48_literals_between", pairs48(True, pairs)[0]))
    out.append(case("b_one_bit_codes", one_bit_blocks()[0]))
    for total in range(316, 322):
        out.append(case(f"b_sixteen_symbols_{total}_bits", saturating(total)))
    for width in (11, 15):
        for rank in range(64):
            out.append(case(f"b_long_code_w{width}_rank{rank}", long_code_at_rank(rank, width)))
    return out


# ---- group C: dynamic headers ----

LL_316 = [8] * 226 + [9] * 60          # 286 lengths, none 0: 226 / 256 + 60 / 512 = 1
D_316 = [5] * 28 + [4] * 2             # 30 lengths: 28 / 32 + 2 / 16 = 1
TEXT = b"a header is only as good as the block behind it; "


def maximal_header(s, final=True, plain=True):
    """HLIT 286, HDIST 30, every length sent by itself, and symbols from both ends of both alphabets."""
    s.dynamic([TEXT, (258, 1), 0xFF, 0x00, (3, 30), (4, 1), TEXT[:9]], LL_316, D_316, plain=plain, final=final)
    return s


def _repeat_case(sym, n):
    """One operation `sym` with count n at literal 100, between literals in use and the end-of-block code behind it."""
    ll = {0x61: 2, 0x62: 2, 256: 2}
    if sym == 16:
        ll.update({100 + k: 9 for k in range(n + 1)})
        at = 101
    else:
        at = 100
    lens = code(ll, pool=list(range(240, 256)) + list(range(257, 286)))
    assert sym == 16 or not any(lens[100: 100 + n])
    s = Stream()
    s.dynamic([b"abba", 240 if lens[240] else 0x61], lens, [0], forced={at: (sym, n)}, final=True)
    assert f"op{sym}:{n}" in s.trace
    return case(f"c_op{sym}_x{n}", s)


def group_c(tier):
    out = []
    s = Stream()
    s.dynamic([b"abcabc"], {0x61: 2, 0x62: 2, 0x63: 2, 256: 2}, [0], final=True)
    assert {"hlit:257", "hdist:1", "dist codes:0"} <= s.trace
    out.append(case("c_hlit257_hdist1_no_distance_code", s))
    s = Stream()
    s.stored(rnd_bytes(3, 24576))
    s.dynamic([0x41, (258, 24577), 0x42], code({0x41: 2, 0x42: 2, 256: 2, 285: 3}), code({29: 2, 0: 1}, 30), final=True)
    assert {"hlit:286", "hdist:30"} <= s.trace
    out.append(case("c_hlit286_hdist30", s))
    s = Stream()  # symbols 1..256 at 8 bits: the header needs the code-length symbols 16, 0 and 8 only
    s.dynamic([bytes(range(1, 256))], {k: 8 for k in range(1, 257)}, [0], cl_lens={16: 2, 17: 2, 0: 2, 8: 2}, final=True)
    assert "hclen:5" in s.trace
    out.append(case("c_hclen5", s))
    s = Stream()
    s.dynamic(rnd_bytes(19, 40), deep_literal_code(), [0], final=True)
    assert "hclen:19" in s.trace
    out.append(case("c_hclen19", s))
    s = Stream()  # 32 codes of 6 bits, 32 of 7, 32 of 8, 64 of 9; the code-length code is a chain down to 7 bits
    ll = {**{0x20 + k: 6 for k in range(32)}, **{0x40 + k: 7 for k in range(32)}, **{0x60 + k: 8 for k in range(32)},
          **{0x80 + k: 9 for k in range(63)}, 256: 9}
    s.dynamic([rnd_bytes(7, 200, range(0x20, 0xBF))], ll, [0], cl_lens={0: 1, 8: 2, 18: 3, 7: 4, 9: 5, 17: 6, 16: 7, 6: 7}, final=True)
    assert "cl_max:7" in s.trace and any(t.startswith("op16:") for t in s.trace)
    out.append(case("c_code_length_code_of_7_bits", s))
    for sym, counts in ((16, range(3, 7)), (17, range(3, 11)), (18, range(11, 139))):
        out += [_repeat_case(sym, n) for n in counts]
    # a 16 that repeats the last literal/length length into the distance lengths
    s = Stream()
    s.dynamic([0x61, (4, 1), (5, 2)], {0x61: 1, 256: 2, 258: 3, 259: 3}, {0: 3, 1: 3, 2: 2, 3: 1}, forced={259: (16, 3)}, final=True)
    assert "repeat crosses boundary:16" in s.trace
    out.append(case("c_16_crosses_into_distance_lengths", s))
    s = Stream()
    s.dynamic([b"aaaa", (4, 3), (5, 4)], {0x61: 1, 256: 2, 258: 3, 259: 3}, {2: 1, 3: 1}, hlit=262, forced={260: (17, 4)}, final=True)
    assert "repeat crosses boundary:17" in s.trace
    out.append(case("c_17_crosses_into_distance_lengths", s))
    for name, forced in (("c_18_crosses_into_distance_lengths", {260: (18, 30)}), ("c_greedy_crosses_into_distance_lengths", None)):
        s = Stream()
        s.dynamic([b"a" * 70, (4, 40), (5, 50)], {0x61: 1, 256: 2, 258: 3, 259: 3}, {10: 1, 11: 1}, hlit=280, forced=forced, final=True)
        assert "repeat crosses boundary:18" in s.trace
        out.append(case(name, s))
    s = Stream()
    s.dynamic([0x61, (10, 1), 0x62], {0x61: 2, 0x62: 2, 256: 2, 264: 2}, [1], final=True)
    assert "dist codes:1" in s.trace
    out.append(case("c_single_distance_code_of_1_bit", s))
    # the 316-length header (about 200 bytes) over the stream ring's refills at 512 and 1 024 bytes
    for pad in (300, 400, 480, 505, 506, 507, 810, 1000, 1018):
        s = Stream()
        s.stored(rnd_bytes(pad, pad))
        out.append(case(f"c_header_behind_{pad + 5}_bytes", maximal_header(s)))
    out.append(case("c_316_lengths_one_by_one", maximal_header(Stream())))
    out.append(case("c_316_lengths_greedy", maximal_header(Stream(), plain=False)))
    # the two kinds zlib refuses and the format allows
    s = Stream()
    s.dynamic([0x61, (3, 1), (3, 2), 0x61], {0x61: 2, 256: 2, 257: 1}, {0: 2, 1: 2}, final=True)
    assert "incomplete dist" in s.trace
    out.append(case("c_incomplete_dist_two_symbols", s))
    s = Stream()
    s.dynamic([b"aaa"], {0x61: 2, 256: 2}, [0], final=True)
    assert "incomplete litlen" in s.trace
    out.append(case("c_incomplete_litlen", s))
    return out


# ---- group D: block structure ----

TINY_LL = {0x61: 2, 0x62: 2, 256: 2, 257: 2}


def tiny_blocks(n=3000, seed=33):
    """n blocks of mixed kind; returns the stream and how many of its blocks hold a symbol other than the end of block."""
    r = random.Random(seed)
    s = Stream()
    with_symbols = 0
    for k in range(n):
        kind = r.randrange(5)
        final = k == n - 1
        if kind == 0:
            s.fixed([], final=final)
        elif kind == 1:
            s.fixed([(r.randrange(3, 40), r.randrange(1, min(len(s.out), 32768) + 1))] if s.out and r.random() < 0.5 else [r.randrange(256)], final=final)
            with_symbols += 1
        elif kind == 2:
            s.stored(b"", final=final, pad=r.randrange(128))
        elif kind == 3:
            s.stored(rnd_bytes(k, r.randrange(1, 20)), final=final, pad=r.randrange(128))
        else:
            syms = [r.choice((0x61, 0x62, (3, 1))) for _ in range(r.randrange(1, 6))]
            if not s.out:
                syms = [0x61] + syms
            s.dynamic(syms, TINY_LL, [1], final=final)
            with_symbols += 1
    return s, with_symbols


RUNS = (191, 192, 193, 254, 255, 256, 257, 700)


SHORT_LITS, LONG_LITS = bytes(range(0x61, 0x6D)), bytes(range(0x41, 0x51))


def _run_cases():
    """Literal runs around the two places a run is closed (192 between rounds, 255 in a record), by codes the lookup tells
    (the fixed code) and by codes it cannot, in front of everything a run can meet. The second kind has twelve literals of
    4 bits and sixteen of 15 (the wave-uniform path); a run takes the long ones around its 192nd and its 255th byte."""
    out = []
    deep = code({**{b: 4 for b in SHORT_LITS}, 256: 4, 257: 4, **{b: 15 for b in LONG_LITS}})
    for kind in ("fixed", "deep"):
        def block(s, syms, final):
            if kind == "fixed":
                s.fixed(syms, final=final)
            else:
                s.dynamic(syms, deep, {0: 1, 1: 1}, final=final)
        for n in RUNS:
            lits = rnd_bytes(n, n)
            if kind == "deep":
                lits = bytes((LONG_LITS if 184 <= i < 200 or 248 <= i < 264 else SHORT_LITS)[b % 12] for i, b in enumerate(lits))
            for behind in ("match", "block", "stored", "end"):
                s = Stream()
                if behind == "match":
                    block(s, [lits, (3, 2), 0x61], True)
                elif behind == "block":
                    block(s, [lits], False)
                    block(s, [b"deed", (3, 1)], True)
                elif behind == "stored":
                    block(s, [lits], False)
                    s.stored(b"stored bytes behind a run", final=True)
                else:
                    block(s, [lits], True)
                out.append(case(f"d_run{n}_{kind}_then_{behind}", s))
    return out


def group_d(tier):
    # the emulator spends 4 ms on a block's tables whatever the block holds: 300 blocks there
    out = [case("d_tiny_blocks", tiny_blocks(3000 if tier == "gpu" else 300)[0])]
    for k in range(8):
        # a fixed block of k literals of 9 bits: 3 + 9 k + 7 bits, then the stored block's header: phase (5 + k) mod 8
        for pad in (0, 0x7F):
            s = Stream()
            s.fixed([0x90 + k] * k)
            s.stored(b"", pad=pad)
            s.fixed([b"behind"], final=True)
            assert f"stored:phase{(5 + k) % 8}" in s.trace
            out.append(case(f"d_empty_stored_phase{(5 + k) % 8}_pad{pad}", s))
    s = Stream()
    s.fixed([b"xy"])
    s.stored(rnd_bytes(5, 300), pad=0b10101)
    s.fixed([(20, 150)], final=True)
    assert "stored:padding set" in s.trace
    out.append(case("d_stored_padding_set", s))
    s = Stream()
    s.stored(rnd_bytes(6, 65535)).stored(b"").stored(rnd_bytes(7, 65535))
    s.fixed([(258, 32768), (3, 1)], final=True)
    assert {"stored:0", "stored:65535"} <= s.trace
    out.append(case("d_stored_65535_0_65535_far_match", s))
    s = Stream()
    s.fixed([b"ten bytes!"])
    s.stored(rnd_bytes(8, 20), final=True)
    out.append(case("d_stored_behind_pending_run", s))
    out += _run_cases()
    for r in range(258) if tier == "gpu" else sorted(set(range(0, 258, 3)) | set(range(248, 258))):
        # 1 + r literals, then ten matches of 258 bytes at distance 1 + r: the batch's 768 bytes end inside a match at
        # every remainder, and the match that does not fit is carried
        s = Stream()
        s.fixed([rnd_bytes(r, 1 + r)] + [(258, 1 + r)] * 10 + [0x2E], final=True)
        out.append(case(f"d_258s_behind_{1 + r}_literals", s))
    for n in (63, 64, 65, 128, 129):
        r = random.Random(n)
        s = Stream()
        s.fixed([b"wxyz"] + [(3, r.randrange(1, 5)) for _ in range(n)] + [0x2E], final=True)
        out.append(case(f"d_{n}_records_of_3_bytes", s))
    s = Stream(tail_fill=1)
    s.fixed([b"the last byte's unused bits are ones"], final=True)
    assert s.bytes()[-1] != s.w.bytes()[-1]
    out.append(case("d_tail_bits_set", s))
    return out


# ---- group E: output capacity ----

def group_e(tier):
    out = []
    makers = {
        "literal": lambda s: s.fixed([rnd_bytes(1, 500), (40, 7), b"end"], final=True),
        "match": lambda s: s.fixed([rnd_bytes(2, 500), (258, 300)], final=True),
        "short_match": lambda s: s.fixed([b"ab", (3, 2)], final=True),
        "stored": lambda s: s.fixed([rnd_bytes(3, 100)]).stored(rnd_bytes(4, 900), final=True),
        "stored_1": lambda s: s.stored(b"x", final=True),
    }
    for name, make in makers.items():
        s = Stream()
        make(s)
        out.append(case(f"e_last_{name}_fits", s))
        out.append(case(f"e_last_{name}_one_short", s, ok=False, cap=len(s.out) - 1, query=len(s.out)))
    return out


# ---- group F: seeded random streams ----

def random_stream(r, limit, counts=(0, 1, 10, 100, 1000, 3000)):
    """1 to 5 blocks; each dynamic block has a random complete code over a random alphabet of 2..286 literal/length
    symbols and 1..30 distance symbols, built by random tree splitting (biased deep half the time)."""
    s = Stream()
    p_match = r.choice((0.0, 0.1, 0.5, 0.95))
    nblocks = r.randrange(1, 6)
    for k in range(nblocks):
        final = k == nblocks - 1
        room = limit - len(s.out)
        kind = r.randrange(8)
        if kind == 0 or room < 600:
            s.stored(rnd_bytes(r.random(), r.randrange(0, min(room, 3000) + 1)), final=final, pad=r.randrange(128))
            continue
        if kind == 1:
            ll_syms, d_syms = list(range(286)), list(range(30))
            ll_lens, d_lens = ds.FIXED_LL, ds.FIXED_D
        else:
            n_ll = r.choice((2, 3, 5, 20, 100, 286, r.randrange(2, 287)))
            n_d = r.choice((1, 2, 5, 30, r.randrange(1, 31)))
            ll_syms = sorted(r.sample([x for x in range(286) if x != 256], n_ll - 1) + [256])
            if not any(x < 256 for x in ll_syms):
                ll_syms[ll_syms.index(min(x for x in ll_syms if x != 256))] = r.randrange(256)  # something to start with
            d_syms = sorted(r.sample(range(30), n_d))
            ll_lens, d_lens = [0] * 286, [0] * 30
            deep = r.random() < 0.5
            for x, l in zip(ll_syms, ds.random_complete_lengths(r, len(ll_syms), deep=deep)):
                ll_lens[x] = l
            for x, l in zip(d_syms, ds.random_complete_lengths(r, n_d, deep=deep) if n_d > 1 else [1]):
                d_lens[x] = l
        lits = [x for x in ll_syms if x < 256]
        lens = [x for x in ll_syms if 257 <= x <= 285]
        syms, produced = [], len(s.out)
        for _ in range(r.choice(counts)):
            if room - (produced - len(s.out)) < 300:
                break
            far = [d for d in d_syms if DIST_BASE[d] <= produced]
            if lens and far and (r.random() < p_match or not lits):
                ls, d = r.choice(lens), r.choice(far)
                length = LEN_BASE[ls - 257] + r.randrange(1 << LEN_EXTRA[ls - 257])
                dist = min(DIST_BASE[d] + r.randrange(1 << DIST_EXTRA[d]), produced)
                syms.append((min(length, 258), dist, ls))
                produced += min(length, 258)
            elif lits:
                syms.append(r.choice(lits))
                produced += 1
            else:
                break
        if kind == 1:
            s.fixed(syms, final=final)
        else:
            s.dynamic(syms, ll_lens, d_lens, final=final, plain=r.random() < 0.1)
    return s


def group_f(tier):
    """16 streams of at most 6 KB and 300 symbols a block on the emulator (a deep code sends every symbol the slow way
    there), 240 of at most 12 KB and 3 000 symbols a block on the card."""
    r = random.Random(1951)
    if tier == "emu":
        return [case(f"f_random_emu_{i}", random_stream(r, 6000, (0, 1, 10, 60, 300))) for i in range(16)]
    return [case(f"f_random_{i}", random_stream(r, 12000)) for i in range(240)]


# ---- group G: refusals ----

def _bad(why):
    return Stream(invalid=why)


def group_g(tier):
    out = []

    def add(name, s, **kw):
        out.append(case("g_" + name, s, **kw))

    s = _bad("BTYPE 3")
    s.fixed([b"abc"])
    s.reserved()
    s.raw_bits(0, 29)
    add("btype3", s)
    add("btype3_first", _bad("BTYPE 3").reserved())
    add("len_nlen_disagree", _bad("LEN / NLEN").stored(b"hello", final=True, nlen=0xFFFB))
    add("stored_longer_than_stream", _bad("LEN past the end").stored(b"hel", final=True, length=5))
    ok_ll, ok_d = {0x61: 1, 256: 1}, [0]
    for field in (30, 31):
        add(f"hlit_field_{field}", _bad("HLIT").dynamic([b"aa"], ok_ll, ok_d, hlit=257 + field, final=True))
        add(f"hdist_field_{field}", _bad("HDIST").dynamic([b"aa"], ok_ll, ok_d, hdist=1 + field, final=True))
    add("code_length_code_oversubscribed", _bad("CL code").dynamic([b"aa"], ok_ll, ok_d, cl_lens={0: 1, 1: 1, 18: 1, 17: 2}, final=True))
    add("litlen_oversubscribed", _bad("LL code").dynamic([b"aa"], {0x61: 1, 0x62: 1, 256: 1}, ok_d, final=True))
    add("dist_oversubscribed", _bad("D code").dynamic([b"aa"], ok_ll, {0: 1, 1: 1, 2: 1}, final=True))
    seq = [0] * 97 + [1] + [0] * 158 + [1] + [0]  # ok_ll and ok_d as HLIT 257 + HDIST 1 lengths
    add("repeat_16_first", _bad("16 first").dynamic([b"aa"], ok_ll, ok_d, ops=[(16, 3)] + ds.greedy_ops(seq[3:]), final=True))
    tail0 = {0: 1, 1: 1}           # HDIST 4: two distance lengths of 0 at the end
    for sym, n in ((17, 3), (18, 11)):
        full = [0] * 97 + [1] + [0] * 158 + [1] + [1, 1, 0, 0]
        add(f"repeat_{sym}_past_the_lengths", _bad("repeat overruns").dynamic(
            [b"aa"], ok_ll, tail0, hdist=4, ops=ds.greedy_ops(full[:-2]) + [(sym, n)], final=True))
    full = [0] * 97 + [1] + [0] * 158 + [1] + [2, 2, 2, 2]
    add("repeat_16_past_the_lengths", _bad("repeat overruns").dynamic(
        [b"aa"], ok_ll, {0: 2, 1: 2, 2: 2, 3: 2}, ops=ds.greedy_ops(full[:-2]) + [(16, 3)], final=True))
    add("no_code_for_256", _bad("no 256").dynamic([b"abab"], {0x61: 1, 0x62: 1}, ok_d, end=False, final=True))
    # HCLEN 4: only 16, 17, 18 and 0 have codes, so every length is 0
    add("hclen4_all_lengths_0", _bad("no 256").dynamic([], {}, [0], hclen=4, cl_lens={18: 1, 0: 1}, ops=[(18, 138), (18, 120)], end=False, final=True))
    for sym in (286, 287):
        add(f"fixed_symbol_{sym}", _bad("286 / 287").fixed([b"abc", ("ll", sym), b"d"], final=True))
    for d in (30, 31):
        add(f"fixed_distance_symbol_{d}", _bad("30 / 31").fixed([b"abc", ("pair", 257, 0, d, 0), b"d"], final=True))
    # codes 00 and 01 are taken; 1x is no symbol
    add("litlen_pattern_without_symbol", _bad("hole").dynamic([b"aa", ("bits", 3, 2), b"a"], {0x61: 2, 256: 2}, ok_d, final=True))
    add("dist_pattern_without_symbol", _bad("hole").dynamic(
        [b"aa", ("ll", 257), ("bits", 3, 2), b"a"], {0x61: 2, 256: 2, 257: 1}, {0: 2, 1: 2}, final=True))
    add("code_length_pattern_without_symbol", _bad("hole").dynamic(
        [b"aa"], ok_ll, ok_d, cl_lens={0: 2, 1: 2, 18: 2}, ops=[(18, 97), ("bits", 3, 2), (1,), (18, 138)], final=True))
    add("length_without_distance_codes", _bad("no D code").dynamic(
        [b"aa", ("pair", 257, 0, None, 0), b"a"], {0x61: 2, 256: 2, 257: 1}, [0], final=True))
    add("distance_past_start_first_block", _bad("too far").fixed([b"abc", raw_match(3, 4)], final=True))
    s = _bad("too far")
    s.stored(b"0123456789").fixed([b"abc"])
    s.fixed([b"d", raw_match(5, 15)], final=True)
    add("distance_past_start_third_block", s)
    s = _bad("too far")
    s.stored(b"0123456789").fixed([b"abc"])
    s.dynamic([b"a", raw_match(3, 15)], {0x61: 2, 256: 2, 257: 1}, {7: 1}, final=True)
    add("distance_past_start_third_block_dynamic", s)
    # every valid header case, cut by one whole byte and to half its bytes
    for c in corpus("c", tier):
        if c.ok:
            for tag, n in (("less_1_byte", len(c.comp) - 1), ("half", len(c.comp) // 2)):
                out.append(Case(f"g_{c.name}_{tag}", "Deflate", c.comp[:n], None, False, c.cap, c.trace, 0))
    return out


# ---- group H: gzip members ----

def _gzip_query(comp):
    """What the gzip size query answers: ISIZE where the chunk has 18 bytes, the magic number and CM 8; else 0."""
    return int.from_bytes(comp[-4:], "little") if len(comp) >= 18 and comp[:3] == b"\x1f\x8b\x08" else 0


def group_h(tier):
    out = []
    s = Stream()
    s.fixed([b"a gzip member: ", rnd_bytes(52, 300), (30, 200)], final=True)
    raw, data = s.bytes(), bytes(s.out)

    def good(tag, **kw):
        comp = gzip_member(raw, data, **kw)
        out.append(case("h_" + tag, s, fmt="Gzip", comp=comp, query=_gzip_query(comp)))

    def bad(tag, comp):
        out.append(case("h_" + tag, s, fmt="Gzip", comp=comp, ok=False, cap=len(data) + 64, query=_gzip_query(comp)))

    extra, name, comment = rnd_bytes(1, 3000), rnd_bytes(2, 2000, range(1, 256)), rnd_bytes(3, 1500, range(1, 256))
    good("plain")
    good("ftext", flg=ds.FTEXT)
    good("fextra_3000", extra=extra)
    good("fextra_0", extra=b"")
    good("fname_2000", name=name)
    good("fname_empty", name=b"")
    good("fcomment_1500", comment=comment)
    good("fhcrc", hcrc=True)
    good("every_field", extra=extra, name=name, comment=comment, hcrc=True, mtime=0x12345678, xfl=2, os=3)
    good("crc32_wrong", crc=ds.crc32(data) ^ 1)
    good("hcrc_wrong", hcrc=True, hcrc_value=0x1234)
    full = gzip_member(raw, data, extra=extra, name=name, comment=comment, hcrc=True)
    at_name, at_comment, at_hcrc = 12 + 3000, 12 + 3000 + 2001, 12 + 3000 + 2001 + 1501
    bad("fextra_past_the_chunk", full[:11] + bytes(7))  # 18 bytes, XLEN 184
    bad("cut_in_fextra", full[:1500])
    bad("cut_in_fname", full[: at_name + 1000])
    bad("cut_in_fcomment", full[: at_comment + 700])
    bad("cut_in_fhcrc", full[: at_hcrc + 1])
    bad("cut_behind_header", full[: at_hcrc + 2])
    bad("cut_in_trailer", full[:-3])
    bad("fname_unterminated", gzip_member(b"", b"", flg=ds.FNAME)[:10] + b"n" * 600)
    short = gzip_member(raw[:1], b"", name=b"abcdef", hcrc=True)
    bad("cut_in_fhcrc_18_bytes", short[:18])
    for bit in (0x20, 0x40, 0x80):
        bad(f"flg_reserved_{bit:02x}", gzip_member(raw, data, flg=bit))
    bad("cm_7", gzip_member(raw, data, cm=7))
    bad("id2_wrong", b"\x1f\x8c" + gzip_member(raw, data)[2:])
    bad("17_bytes", gzip_member(raw, data)[:10] + bytes(7))
    bad("raw_stream_as_member", raw)
    bad("isize_one_more", gzip_member(raw, data, isize=len(data) + 1))
    bad("isize_one_less", gzip_member(raw, data, isize=len(data) - 1))
    return out


GROUPS = {"a": group_a, "b": group_b, "c": group_c, "d": group_d, "e": group_e, "f": group_f, "g": group_g, "h": group_h}
_corpus = {}


def corpus(g, tier):
    """Group g's cases for a tier ("emu": the thinned set; "gpu": everything), built once."""
    if (g, tier) not in _corpus:
        cases = GROUPS[g](tier)
        assert len({c.name for c in cases}) == len(cases)
        _corpus[g, tier] = cases
    return _corpus[g, tier]


def every_case():
    """Both tiers' cases, each name once."""
    seen, out = set(), []
    for g in GROUPS:
        for c in corpus(g, "gpu") + corpus(g, "emu"):
            if c.name not in seen:
                seen.add(c.name)
                out.append(c)
    return out


def arr(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def zlib_says(c):
    """The bytes zlib decodes a case to within the case's capacity, or None where it refuses (or needs more room)."""
    try:
        o = zlib.decompressobj(-15 if c.fmt == "Deflate" else 31)
        got = o.decompress(c.comp, c.cap + 1)
        if not o.eof or len(got) > c.cap:
            return None
        return got
    except zlib.error:
        return None


def decode_cases(backend, cases):
    """One batched call per format: valid cases give Success, the exact size and every byte; the others
    ErrorCannotDecompress and size 0. The size query answers what each case says. Then the call without statuses and the
    call without sizes on the three smallest valid cases (and the first forty refused ones: their sizes read 0 without statuses too)."""
    for fmt in ("Deflate", "Gzip"):
        part = [c for c in cases if c.fmt == fmt]
        if not part:
            continue
        codec = backend.codec(fmt)
        comps, caps = [arr(c.comp) for c in part], [c.cap for c in part]
        outs, actual, status = codec.decompress(comps, caps)
        for c, o, a, st in zip(part, outs, actual.tolist(), status.tolist()):
            if c.ok:
                assert st == NvcompStatus.Success, (c.name, st)
                assert a == len(c.out), (c.name, a, len(c.out))
                assert o[:a].tobytes() == c.out, (c.name, "differs at", next(i for i in range(a) if o[i] != c.out[i]))
            else:
                assert st == NvcompStatus.ErrorCannotDecompress, (c.name, st)
                assert a == 0, (c.name, a)
        sizes = codec.get_decompress_size(comps).tolist()
        assert sizes == [c.query for c in part], [(c.name, s, c.query) for c, s in zip(part, sizes) if s != c.query]
        some = sorted([c for c in part if c.ok], key=lambda c: len(c.comp) + len(c.out))[:3] + [c for c in part if not c.ok][:40]
        comps, caps = [arr(c.comp) for c in some], [c.cap for c in some]
        outs, actual, status = codec.decompress(comps, caps, checked=False)
        assert status is None
        for c, o, a in zip(some, outs, actual.tolist()):
            assert a == (len(c.out) if c.ok else 0), (c.name, a)
            assert not c.ok or o[:a].tobytes() == c.out, c.name
        outs, actual, status = codec.decompress(comps, caps, want_actual=False)
        assert actual is None
        for c, o, st in zip(some, outs, status.tolist()):
            assert st == (NvcompStatus.Success if c.ok else NvcompStatus.ErrorCannotDecompress), (c.name, st)
            assert not c.ok or o[: len(c.out)].tobytes() == c.out, c.name


# ---- the writer itself, and what zlib says to the refusals (CPU only) ----

def test_bit_writer():
    w = ds.BitWriter()
    w.put(1, 1), w.put(0b110, 3, True), w.align(0b1010)
    assert w.bytes() == bytes([0b10100111]) and w.bit_length() == 8
    w.raw(b"\x55"), w.put(0x1FF, 9)
    assert w.bytes() == b"\xa7\x55\xff\x01"
    assert ds.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4]) == {0: (2, 3), 1: (3, 3), 2: (4, 3), 3: (5, 3), 4: (6, 3), 5: (0, 2), 6: (14, 4), 7: (15, 4)}  # RFC 1951 3.2.2
    assert ds.crc32(b"123456789") == 0xCBF43926 and ds.crc32(b"") == 0


def test_writer_refuses_what_it_cannot_expand():
    with pytest.raises(ValueError, match="past the"):
        Stream().fixed([b"abc", (3, 4)])
    with pytest.raises(ValueError, match="has no code"):
        Stream().dynamic([0x62], {0x61: 1, 256: 1}, [0])
    with pytest.raises(ValueError, match="has no code"):
        Stream().dynamic([0x61, (3, 1)], {0x61: 1, 256: 2, 257: 2}, [0])
    with pytest.raises(ValueError, match="over-subscribed"):
        Stream().dynamic([0x61], {0x61: 1, 0x62: 1, 256: 1}, [0])
    with pytest.raises(ValueError, match="do not send"):
        Stream().dynamic([0x61], {0x61: 1, 256: 1}, [0], ops=[(18, 138)])
    with pytest.raises(ValueError, match="not one of symbol"):
        Stream().fixed([b"abc", (258, 1, 283)])
    with pytest.raises(ValueError, match="marked invalid"):
        Stream().fixed([("ll", 286)])
    with pytest.raises(ValueError, match="65 535"):
        Stream().stored(bytes(65536))


@pytest.mark.parametrize("g", sorted(GROUPS))
def test_writer_against_zlib(g):
    """Every valid stream of the corpus, both tiers, decodes with zlib to the writer's own expansion, except the named
    ones zlib refuses; and those it does refuse."""
    refused = set()
    for c in corpus(g, "gpu") + [c for c in corpus(g, "emu") if c.name not in {k.name for k in corpus(g, "gpu")}]:
        if c.ok:
            got = zlib_says(c)
            if got is None:
                refused.add(c.name)
            else:
                assert got == c.out, f"{c.name}: zlib and the writer's expansion differ"
    assert refused == {n for n in ZLIB_REFUSES if n.startswith(g + "_")}


def test_refusals_against_zlib():
    """zlib's verdict on every stream the decoder must refuse: it refuses them too, except ZLIB_ACCEPTS. (A case of group
    E is a valid stream in a slot one byte short: zlib_says gives zlib that much room and no more.)"""
    accepted = {c.name for c in every_case() if not c.ok and zlib_says(c) is not None}
    assert accepted == ZLIB_ACCEPTS, sorted(accepted ^ ZLIB_ACCEPTS)


def test_corpus_covers_the_format():
    """What the writer's traces say the corpus holds, the emulator tier's thinned set included."""
    for tier in ("emu", "gpu"):
        trace = set().union(*[c.trace for g in GROUPS for c in corpus(g, tier) if c.ok])
        want = {f"len_sym:{s}" for s in range(257, 286)} | {f"dist_sym:{d}" for d in range(30)}
        want |= {f"ll_max:{w}" for w in (1, 9, 10, 11, 15)} | {f"d_max:{w}" for w in (1, 7, 8, 9, 15)}
        want |= {f"op16:{n}" for n in range(3, 7)} | {f"op17:{n}" for n in range(3, 11)} | {f"op18:{n}" for n in range(11, 139)}
        want |= {f"repeat crosses boundary:{s}" for s in (16, 17, 18)} | {f"stored:phase{p}" for p in range(8)}
        want |= {"284+31", "kind:stored", "kind:fixed", "kind:dynamic", "hlit:257", "hlit:286", "hdist:1", "hdist:30", "hclen:5",
                 "hclen:19", "cl_max:7", "dist codes:0", "dist codes:1", "stored:0", "stored:65535", "stored:padding set",
                 "tail bits set", "incomplete litlen", "incomplete dist"}
        assert want <= trace, sorted(want - trace)
    for g in "gh":  # every refusal on both tiers
        assert {c.name for c in corpus(g, "emu")} == {c.name for c in corpus(g, "gpu")}


# ---- groups A-H on the decoder ----

@pytest.mark.parametrize("g", sorted(GROUPS))
def test_group(backend, g):
    cases = corpus(g, backend.name)
    if g == "f":
        print(len(cases), "random streams,", sum(len(c.out) for c in cases), "bytes")
    decode_cases(backend, cases)


def test_isize_is_checked_without_statuses(backend):
    """ISIZE off by one: size 0 with statuses and without (the checks do not depend on the caller's pointers)."""
    cases = [c for c in corpus("h", backend.name) if c.name.startswith("h_isize")]
    assert len(cases) == 2
    codec = backend.codec("Gzip")
    for kw in ({}, {"checked": False}):
        outs, actual, status = codec.decompress([arr(c.comp) for c in cases], [c.cap for c in cases], **kw)
        assert actual.tolist() == [0, 0]
        assert status is None or status.tolist() == [NvcompStatus.ErrorCannotDecompress] * 2


# ---- the cases reach the paths they are named for (emulator only: the counters compile out of the product) ----

def emu_stats():
    """The emulator's LZ_STAT counters (text on stderr: dumped into a file, read back)."""
    lib = C.CDLL(os.path.join(REPO, "tests", "emu", "libnvcomp_emu.so"))
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            lib.emu_stats_dump(0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"stat (\S+)\s+(\d+)", text)}


def counted(emu, s):
    """The counters one decode of the stream adds."""
    before = emu_stats()
    outs, actual, status = emu.codec("Deflate").decompress([arr(s.bytes())], [len(s.out)])
    assert status.tolist() == [NvcompStatus.Success] and outs[0].tobytes() == bytes(s.out)
    after = emu_stats()
    return {k: after.get(k, 0) - before.get(k, 0) for k in after}


def test_cases_reach_their_paths(emu):
    # literals of 15 bits: no lookup tells any of them, so each is walked wave-uniformly: one call each at least
    s = Stream()
    s.dynamic(rnd_bytes(15, 500), deep_literal_code(), [0], final=True)
    n = counted(emu, s)
    assert n["deflate_uniform_symbols"] >= 500, n
    # the same data by zlib: what an enumeration yields on a stream zlib writes
    data = datasets.CLASSES["text"](16384, 1).tobytes()
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    zs = z.compress(data) + z.flush()
    before = emu_stats()
    outs, actual, status = emu.codec("Deflate").decompress([arr(zs)], [len(data)])
    assert outs[0].tobytes() == data
    after = emu_stats()
    z_enum = after["deflate_enumerations"] - before.get("deflate_enumerations", 0)
    z_syms = after["deflate_round_symbols"] - before.get("deflate_round_symbols", 0)
    # 1-bit codes: sixteen symbols take 16 bits, the top table's entry (distance - 64) cannot hold that and reads 255, so
    # an enumeration ends at rank 15 at the latest
    s, syms = one_bit_blocks()
    n = counted(emu, s)
    assert n["deflate_enumerations"] * 16 >= syms, n
    assert n["deflate_enumerations"] * z_syms > z_enum * n["deflate_round_symbols"], (n, z_enum, z_syms)
    # 48-bit pairs of two 15-bit codes: every enumeration stops at its first symbol
    for with_literals in (False, True):
        pairs = 40
        s, syms = pairs48(with_literals, pairs)
        n = counted(emu, s)
        assert n["deflate_enumerations"] >= pairs and n["deflate_uniform_symbols"] >= pairs, n
        assert n["deflate_enumerations"] * z_syms > z_enum * n["deflate_round_symbols"], (n, z_enum, z_syms)
    # sixteen symbols of 319 bits and more: the top table's entry reads 255 and no enumeration gets past rank 15
    for total in (319, 321):
        n = counted(emu, saturating(total))
        assert n["deflate_enumerations"] * 16 >= 16 * 40, (total, n)
    # a block's tables are its own: one build at least for every block that holds a symbol
    s, with_symbols = tiny_blocks(100)
    n = counted(emu, s)
    assert n["deflate_builds"] >= with_symbols, (n, with_symbols)
