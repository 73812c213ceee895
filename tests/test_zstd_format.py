"""The Zstandard decoder against frames libzstd never writes.

tests/zstd_frames.py writes every frame here from an explicit description and expands that description itself; the
expansion is the reference. CPU libzstd, where it loads, checks the writer (test_writer_against_libzstd) and is asked
for its verdict on every frame the decoder must refuse (test_refusals_against_libzstd). The decoder runs on the
emulator and on the card through the `backend` fixture with the guard-byte layout of tests/test_zstd.py.

Where this file departs from a literal reading of the format's limits, and why:
  * four Huffman streams cannot hold 5 literals (three streams of (5 + 3) / 4 = 2 leave -1 for the fourth): that size
    is a refusal case; one stream cannot hold more than 1 023 (its header has 10 bits);
  * raw literals of 131 072 bytes do not fit a block of at most 128 KiB with their header: 131 060 leaves room for one sequence, and
    131 072 is a refusal case (Block_Size 131 076);
  * LL code 35 / ML code 52 with all extra bits set regenerate 131 074 bytes in one block, two more than
    Block_Maximum_Size; neither libzstd nor this decoder bounds a block's regenerated size other than by the output.

Where libzstd 1.4.8 and the decoder disagree on accepting a frame (also in DESIGN.md):
  * LIBZSTD_ACCEPTS below: frames the decoder refuses and libzstd decodes;
  * LIBZSTD_REFUSES below: frames the decoder decodes and libzstd 1.4.8 refuses.
"""
import random
from collections import namedtuple

import numpy as np
import pytest

import zstd_frames as zf
from nvcomp_amd import zstd_cpu
from nvcomp_amd._lib import NvcompStatus
from nvcomp_amd.batched import BatchedCodec
from test_zstd import _ncount, check_exact, needs_libzstd, run
from zstd_frames import REP1, REP2, REP3, Frame, huf_lit, raw_lit, rle_lit, treeless_lit

# Refused by the decoder, decoded by libzstd 1.4.8:
LIBZSTD_ACCEPTS = {
    # Repeated_Offset 3 with ll == 0 when rep0 is 1 gives offset 0, which RFC 8878 3.1.1.5 calls corrupt; libzstd
    # "corrects" it to 1. The decoder's rule: an offset of 0 is refused.
    "g4_rep0_minus_1_is_0",
    # Huffman codes of 12 bits: RFC 8878 4.2.1 allows 11; libzstd's decoder builds tables of up to 12. The decoder's
    # rule: the weights must complete a code of at most 11 bits.
    "g6_depth_12", "g8_huffman_depth_12",
    # Reserved bits of the sequences' mode byte set: "must be zero" (RFC 8878 3.1.1.3.2.1); libzstd 1.4.8 ignores them.
    "g8_mode_byte_reserved_1", "g8_mode_byte_reserved_2", "g8_mode_byte_reserved_3",
    # Bits left in the sequences' stream after the last sequence: libzstd 1.4.8 only checks that the stream did not run
    # out. The decoder's rule: every bit stream ends exactly at its padding bit.
    "g8_stream_with_1_bits_left", "g8_stream_with_8_bits_left", "g8_stream_with_9_bits_left",
    # A raw or RLE block of 131 073 bytes, one more than Block_Maximum_Size (RFC 8878 3.1.1.2.3): libzstd's one-shot
    # ZSTD_decompress bounds such a block by the input and the output only. The decoder's rule: Block_Size <= 128 KiB.
    "g7_block_size_131073", "g8_block_size_above_128k",
}
# Decoded by the decoder, refused by libzstd 1.4.8:
LIBZSTD_REFUSES = {
    # a compressed block of 2 bytes (1-byte literals header saying 0, Number_of_Sequences 0): valid by RFC 8878;
    # libzstd 1.4.8 wants at least 3 bytes in a compressed block
    "g7_compressed_empty_2_bytes",
}

Case = namedtuple("Case", "name comp out ok cap trace query")  # query: what the size query must answer, or None


def case(name, *parts, ok=True, cap=None, query=None):
    """A chunk of frames (Frame) and raw byte strings (skippable frames) in order."""
    frames = [p for p in parts if isinstance(p, Frame)]
    for f in frames:
        if f.fcs_bytes == 1 and len(f.out) > 255:  # left at the default: the smallest field that holds the content
            finish(f)
    comp = b"".join(p.bytes() if isinstance(p, Frame) else bytes(p) for p in parts)
    out = b"".join(bytes(f.out) for f in frames)
    trace = set().union(*[f.trace for f in frames]) if frames else set()
    return Case(name, comp, out, ok, max(len(out), 1) if cap is None else cap, trace, query)


def refuse(name, *parts, cap=4096, query=None):
    """A chunk the decoder must refuse. A frame left at the default header gets a window descriptor and no
    Frame_Content_Size, so that nothing but the rule the case names can refuse it: whatever a lenient decoder would
    produce fits `cap` and contradicts no header field. Only group 10's cases, which are about the field, carry one."""
    for f in parts:
        if isinstance(f, Frame) and f.single and f.fcs_bytes == 1 and f.fcs is None and f.header is None:
            f.single, f.window_log, f.fcs_bytes = False, 24, 0
    return case(name, *parts, ok=False, cap=cap, query=query)


def rnd_bytes(seed, n, alphabet=None):
    r = random.Random(seed)
    if alphabet is None:
        return bytes(r.getrandbits(8) for _ in range(n))
    return bytes(r.choice(alphabet) for _ in range(n))


def fcs_for(n):
    return 1 if n < 256 else 2 if n < 65792 else 4


def finish(f):
    """The frame with the smallest FCS field that holds its content."""
    f.fcs_bytes = fcs_for(len(f.out))
    return f


RLE3 = dict(ll=("rle",), of=("rle",), ml=("rle",))
LL_ALL = ("fse", [29] + [1] * 35, 6)       # tables that hold every code
ML_ALL = ("fse", [12] + [1] * 52, 6)
OF_ALL25 = ("fse", [8] + [1] * 24, 5)      # offset codes 0-24
OF_ALL32 = ("fse", [1] * 32, 5)            # offset codes 0-31


# ---- group 1: Number_of_Sequences ----

def group1(tier):
    counts = [127, 128, 0x7F00, 0x7F01] if tier == "emu" else [1, 127, 128, 129, 0x7EFF, 0x7F00, 0x7F01, 43690]
    out = []
    for n in counts:
        f = Frame()
        f.raw(b"\x5a")
        f.compressed(raw_lit(b""), [(0, 3, 1)] * n, last=True, **RLE3)
        out.append(case(f"g1_nseq_{n}", finish(f)))
    f = Frame()
    f.raw(b"\x5a")
    f.compressed(raw_lit(b""), [(0, 3, 1)] * 5, last=True, nseq_bytes=2, **RLE3)  # 5 in the 2-byte form
    out.append(case("g1_nseq_5_in_2_bytes", finish(f)))
    return out


# ---- group 2: every length code ----

def _extras(seed, bits):
    vals = [0, (1 << bits) - 1, random.Random(seed).randrange(1 << bits)]
    return list(zip(("zero", "ones", "rand"), vals))[: 3 if bits else 1]


FRONT = b"\x11\x22\x33\x44\x55\x66\x77\x88"  # eight distinct bytes in front of every group 2 block


def group2(tier):
    out = []
    for c in range(36):
        for tag, extra in _extras(c, zf.LL_BITS[c]):
            ll = zf.LL_BASE[c] + extra
            assert zf.ll_code(ll) == c
            # The literals are one byte value, so the match behind them says where the run ended: it reaches across the
            # run into the distinct bytes in front, and a run that is any k literals short or long moves what it copies.
            f = Frame()
            f.raw(FRONT)
            f.compressed(rle_lit(0x6C, ll), [(ll, 4, ll + 3)], last=True, **RLE3)
            assert bytes(f.out[-4:]) == FRONT[5:] + b"\x6c"[: min(ll, 1)] + FRONT[5:6][: 1 - min(ll, 1)]
            out.append(case(f"g2_ll{c}_{tag}_rle", finish(f)))
            f = Frame()
            f.raw(FRONT)
            f.compressed(rle_lit(0x6D, ll + 1), [(0, 3, 2), (ll, 4, ll + 6), (1, 3, 1)], ll=LL_ALL, ml=ML_ALL, of=OF_ALL25, last=True)
            out.append(case(f"g2_ll{c}_{tag}_fse", finish(f)))
    for c in range(53):
        for tag, extra in _extras(100 + c, zf.ML_BITS[c]):
            ml = zf.ML_BASE[c] + extra
            assert zf.ml_code(ml) == c
            f = Frame()
            f.raw(FRONT)
            f.compressed(raw_lit(b"q"), [(1, ml, 3)], last=True, **RLE3)
            out.append(case(f"g2_ml{c}_{tag}_rle", finish(f)))
            f = Frame()
            f.raw(FRONT)
            f.compressed(raw_lit(b"qr"), [(0, 3, 2), (1, ml, 3), (1, 3, 1)], ll=LL_ALL, ml=ML_ALL, of=OF_ALL25, last=True)
            out.append(case(f"g2_ml{c}_{tag}_fse", finish(f)))
    return out


# ---- group 3: offset codes ----

def _far_frame(off, of_spec, ml=8, check=True):
    """`off` bytes of output (64 random bytes in a raw block, then RLE blocks of 128 KiB), then one match that reaches
    back to the frame's first byte."""
    f = Frame()
    head = rnd_bytes(off, min(off, 64))
    f.raw(head)
    k = 1
    while len(f.out) < off:
        n = min(off - len(f.out), zf.BLOCK_MAX)
        f.rle(k & 255, n)
        k += 1
    f.compressed(raw_lit(b""), [(0, min(ml, (1 << 24) - off), off)], ll=("rle",), ml=("rle",), of=of_spec, last=True, check=check)
    return finish(f)


def group3(tier):
    out = []
    top = 20 if tier == "emu" else 24
    limit = (1 << 24) - 3  # code 24's smallest offset, 2^24 - 3, and a match of 3 fill the 16 MiB a chunk may hold
    for c in range(top + 1):
        lo, hi = max((1 << c) - 3, 1), min((2 << c) - 4, limit)
        for off in sorted({lo, hi}):
            if off < 1 or (off + 3).bit_length() - 1 != c:
                continue
            out.append(case(f"g3_of{c}_{off}_rle", _far_frame(off, ("rle",))))
            out.append(case(f"g3_of{c}_{off}_fse", _far_frame(off, OF_ALL25)))
    for code, c in ((REP1, 0), (REP2, 1), (REP3, 1)):  # codes 0 and 1 are the repeat codes: offset values 1, 2 and 3
        for name, spec in (("rle", ("rle",)), ("fse", OF_ALL25)):
            f = Frame()
            f.raw(rnd_bytes(c, 16))
            f.compressed(raw_lit(b"uv"), [(2, 8, code)], ll=("rle",), ml=("rle",), of=spec, last=True)
            out.append(case(f"g3_of{c}_{code}_{name}", f))
    for c in range(25, 32):
        for name, spec in (("rle", ("rle",)), ("fse", OF_ALL32)):
            f = Frame()
            f.raw(rnd_bytes(c, 64))
            f.compressed(raw_lit(b""), [(0, 8, (1 << c) - 3)], ll=("rle",), ml=("rle",), of=spec, last=True, check=False)
            out.append(refuse(f"g3_of{c}_{name}", f))
    return out


# ---- group 4: repeat offsets ----

def group4(tier):
    out = []
    setup = [(2, 5, 7), (1, 4, 11), (3, 6, 13)]              # rep = 13, 11, 7
    chain = [(1, 3, REP1), (1, 3, REP2), (1, 3, REP3), (1, 4, REP3), (1, 3, REP2)]
    for code in (REP1, REP2, REP3):
        for ll in (2, 0):
            f = Frame()
            f.raw(rnd_bytes(40 + ll, 32))
            f.compressed(raw_lit(rnd_bytes(41, 64)), setup + [(ll, 4, code)] + chain, last=True)
            out.append(case(f"g4_{code}_ll{ll}", finish(f)))
    f = Frame()  # ll == 0 three times in a row: rep1, rep2, rep0 - 1 chained
    f.raw(rnd_bytes(42, 32))
    f.compressed(raw_lit(rnd_bytes(43, 32)), setup + [(0, 3, REP1), (0, 3, REP2), (0, 3, REP3), (0, 3, REP3)] + chain, last=True)
    out.append(case("g4_ll0_chain", finish(f)))
    for between in ("raw", "rle", "both"):
        f = Frame()
        f.raw(rnd_bytes(44, 32))
        f.compressed(raw_lit(rnd_bytes(45, 16)), setup)
        if between in ("raw", "both"):
            f.raw(rnd_bytes(46, 21))
        if between in ("rle", "both"):
            f.rle(0x77, 19)
        f.compressed(raw_lit(rnd_bytes(47, 16)), [(1, 3, REP3), (0, 3, REP1), (2, 4, REP2)] + chain, last=True)
        out.append(case(f"g4_across_{between}", finish(f)))
    a, b = Frame(), Frame()
    a.raw(rnd_bytes(48, 32))
    a.compressed(raw_lit(rnd_bytes(49, 16)), setup + chain, last=True)
    b.raw(rnd_bytes(50, 16))
    b.compressed(raw_lit(rnd_bytes(51, 16)), [(1, 3, REP3), (1, 3, REP3), (1, 3, REP3)], last=True)  # 8, then 4, then 1
    out.append(case("g4_second_frame_starts_at_1_4_8", finish(a), finish(b)))
    # the initial offsets 1 / 4 / 8 used by a frame's first sequence: just enough bytes in front, and one too few
    for code, need in ((REP1, 1), (REP2, 4), (REP3, 8)):
        f = Frame()
        f.compressed(raw_lit(rnd_bytes(52, need + 2)), [(need, 5, code)], last=True)
        out.append(case(f"g4_initial_{code}_fits", finish(f)))
        f = Frame()
        f.compressed(raw_lit(rnd_bytes(53, need + 2)), [(need - 1, 5, code)] if need > 1 else [(0, 5, REP1)], last=True, check=False)
        out.append(refuse(f"g4_initial_{code}_before_frame", f))
    f = Frame(single=False, window_log=10)  # no Frame_Content_Size: nothing but the offset decides
    f.raw(rnd_bytes(54, 16))
    f.compressed(raw_lit(b"ab"), [(0, 3, REP3)], last=True, check=False)
    out.append(refuse("g4_rep0_minus_1_is_0", f))
    return out


# ---- group 5: FSE table descriptions ----

SEQS5 = [(0, 3, 1), (1, 4, 2), (2, 5, 5), (0, 3, 1), (1, 4, 2), (3, 3, 1), (0, 3, 1), (2, 7, 9), (0, 3, 1)]


def _g5(name, ok=True, seqs=SEQS5, **kw):
    f = Frame()
    f.raw(rnd_bytes(60, 16))
    f.compressed(raw_lit(rnd_bytes(61, 40)), seqs, last=True, check=ok, **kw)
    return case(name, finish(f)) if ok else refuse(name, f)


def group5(tier):
    out = [
        _g5("g5_log5", ll=("fse", None, 5), of=("fse", None, 5), ml=("fse", None, 5)),
        _g5("g5_log_max", ll=("fse", None, 9), of=("fse", None, 8), ml=("fse", None, 9)),
        _g5("g5_ll_log10", ok=False, ll=("fse", None, 10)),
        _g5("g5_of_log9", ok=False, of=("fse", None, 9)),
        _g5("g5_ml_log10", ok=False, ml=("fse", None, 10)),
        _g5("g5_less_than_one", ll=("fse", [-1, 28, -1, -1, -1], 5), of=("fse", [-1, -1, 28, -1, -1], 5),
            ml=("fse", [26, -1, -1, -1, -1, -1, -1], 5)),
        # zero runs of 1, 3, 4, 6 and 30 symbols between the codes in use
        _g5("g5_zero_runs", seqs=[(0, 3, 1), (0, 5, 1), (0, 9, 1), (0, 14, 1), (0, 21, 1), (0, zf.ML_BASE[49], 1), (0, 3, 1)],
            ml=("fse", [16, 0, 8] + [0] * 3 + [4] + [0] * 4 + [2] + [0] * 6 + [1] + [0] * 30 + [1], 5)),
        _g5("g5_last_symbols", ll=("fse", [29] + [1] * 35, 6), of=("fse", [1] * 32, 5), ml=("fse", [12] + [1] * 52, 6)),
        _g5("g5_ll_symbol_36", ok=False, ll=("fse", [28] + [1] * 36, 6)),
        _g5("g5_of_symbol_32", ok=False, of=("fse", [32] + [1] * 32, 6)),
        _g5("g5_ml_symbol_53", ok=False, ml=("fse", [11] + [1] * 53, 6)),
        # every symbol of the alphabet listed and the counts still short of the table size
        _g5("g5_ll_sum_short", ok=False, ll=("fse", [2] + [1] * 35, 6)),
        _g5("g5_of_sum_short", ok=False, of=("fse", [1] * 32, 6)),
        _g5("g5_ml_sum_short", ok=False, ml=("fse", [2] + [1] * 52, 6)),
    ]
    firsts = {"predefined": dict(), "rle": dict(RLE3), "fse": dict(ll=("fse", None, 6), of=("fse", None, 5), ml=("fse", None, 7))}
    for name, kw in firsts.items():
        f = Frame()
        f.raw(rnd_bytes(62, 16))
        seqs = [(1, 3, 1)] * 4 if name == "rle" else SEQS5
        f.compressed(raw_lit(rnd_bytes(63, 40)), seqs, **kw)
        f.compressed(raw_lit(rnd_bytes(64, 40)), list(reversed(seqs)), ll=("repeat",), of=("repeat",), ml=("repeat",))
        f.compressed(raw_lit(rnd_bytes(65, 40)), seqs, ll=("repeat",), of=("repeat",), ml=("repeat",), last=True)
        out.append(case(f"g5_repeat_after_{name}", finish(f)))
    for which in ("ll", "of", "ml"):
        out.append(_g5(f"g5_{which}_repeat_without_table", ok=False, **{which: ("repeat",)}))
    f = Frame()  # a block without sequences sets up no table either
    f.compressed(raw_lit(rnd_bytes(66, 20)), [])
    f.compressed(raw_lit(rnd_bytes(67, 40)), SEQS5, of=("repeat",), last=True, check=False)
    out.append(refuse("g5_repeat_after_block_without_sequences", f))
    return out


# ---- group 6: Huffman ----

TEXT = b"eeeeeeeettttaaaooiinn shrdlu,.\n"


def _huf_sizes(tier):
    return [4, 5, 6, 7, 8, 1023, 1024, 16383, 16384] + ([131072] if tier == "gpu" else [])


def group6(tier):
    out = []
    direct = {1: [1, 1], 2: [1, 1, 2], 3: [1, 1, 2, 3], 127: [1] * 128, 128: [1] * 128 + [8]}
    for listed, weights in direct.items():
        f = Frame()
        data = rnd_bytes(70 + listed, 150, [s for s, w in enumerate(weights) if w])
        f.compressed(huf_lit(data, streams=1, weights=weights), [(3, 4, 2)], last=True)
        out.append(case(f"g6_direct_{listed}", finish(f)))
    for last_symbol in (19, 20):  # 19 and 20 weights listed: the stream ends in the one state and in the other
        f = Frame()
        data = rnd_bytes(80, 300, list(range(last_symbol + 1)) * 2 + [0, 0, 0, 1, 1, 2] * 9) + bytes([last_symbol])
        f.compressed(huf_lit(data, streams=4, desc="fse"), [(3, 4, 2)], last=True)
        assert f"huf:fse:{last_symbol}" in f.trace
        out.append(case(f"g6_fse_weights_{last_symbol}", finish(f)))
    f = Frame()
    w11 = [1, 1] + list(range(2, 12))  # 1 + 1 + 2 + ... + 2^10 = 2^11: codes of 11 bits down to 1
    f.compressed(huf_lit(rnd_bytes(81, 400, range(12)), streams=4, weights=w11), [(3, 4, 2)], last=True)
    assert "huf:depth11" in f.trace
    out.append(case("g6_depth_11", finish(f)))
    f = Frame()
    f.compressed(huf_lit(rnd_bytes(82, 400, range(13)), streams=4, weights=w11[:-1] + [11, 12]), [(3, 4, 2)], last=True, check=False)
    assert "huf:depth12" in f.trace
    out.append(refuse("g6_depth_12", f))
    f = Frame()
    # Five codes of 3 bits (cells 0-4 of 8): the sum 5 leaves 3, no power of two. The literals use only those five, so a
    # decoder that built a table all the same would decode them: nothing but the rule refuses this frame.
    f.compressed(huf_lit(rnd_bytes(83, 40, range(5)), streams=1, weights=[1, 1, 1, 1, 1, 2]), [], last=True, check=False)
    out.append(refuse("g6_weights_complete_no_code", f))
    f = Frame()
    f.compressed(huf_lit(rnd_bytes(84, 500, [0, 0, 0, 0, 1, 1, 2, 9, 255, 255]), streams=4, desc="fse"), [(3, 4, 2)], last=True)
    assert "huf:fse:255" in f.trace
    out.append(case("g6_symbol_255_implied", finish(f)))
    for regen in _huf_sizes(tier):
        data = rnd_bytes(regen, regen, TEXT)
        data = data[:-4] + b"eetz"  # the four streams' last symbols are told apart
        for streams in (1, 4):
            if streams == 1 and regen > 1023:
                continue
            f = Frame()
            if streams == 4 and regen == 5:
                f.compressed(huf_lit(data, streams=4, counts=[2, 2, 1, 0]), [], last=True, check=False)
                out.append(refuse("g6_regen5_4streams", f))
                continue
            f.compressed(huf_lit(data, streams=streams), [(min(regen, 3), 3, 1)], last=True)
            out.append(case(f"g6_regen{regen}_{streams}streams", finish(f)))
    f = Frame()  # every Size_Format at a size the smallest holds
    for sf in (1, 2, 3):
        f.compressed(huf_lit(rnd_bytes(85 + sf, 200, TEXT), streams=4, sf=sf), [(3, 4, 2)], last=sf == 3)
    out.append(case("g6_size_formats_not_minimal", finish(f)))
    f = Frame()
    f.compressed(huf_lit(rnd_bytes(86, 300, TEXT), streams=4), [(3, 4, 2)])
    f.compressed(raw_lit(rnd_bytes(87, 50)), [(3, 4, 2)])
    f.compressed(rle_lit(0x21, 50), [(3, 4, 2)])
    f.compressed(treeless_lit(rnd_bytes(88, 300, TEXT), streams=4), [(3, 4, 2)])
    f.compressed(treeless_lit(rnd_bytes(89, 200, TEXT), streams=1), [(3, 4, 2)], last=True)
    out.append(case("g6_treeless_after_raw_and_rle", finish(f)))
    f = Frame()
    f.compressed(treeless_lit(rnd_bytes(90, 100, b"\x00\x01"), streams=1), [], last=True, check=False)
    out.append(refuse("g6_treeless_first", f))
    return out


# ---- group 7: literal headers and the block layer ----

def group7(tier):
    out = []
    for size in (0, 5, 31, 32, 4095, 4096, 131060, 131072):
        for hl in (1, 2, 3):
            if size >= 1 << (5, 12, 20)[hl - 1] or (size > 4096 and tier == "emu" and hl != 3):
                continue
            for kind in ("raw", "rle"):
                if (kind, size) == ("raw", 131072) or size == 0 and (kind == "rle" or hl == 1):
                    continue
                f = Frame()
                lit = raw_lit(rnd_bytes(size, size), hl) if kind == "raw" else rle_lit(0x3C, size, hl)
                f.compressed(lit, [(size // 2, 3, 1)] if size > 1 else [], last=True)
                out.append(case(f"g7_{kind}_lit_{size}_hl{hl}", finish(f)))
    f = Frame()
    f.compressed(raw_lit(bytes(131072), 3), [], last=True, check=False)
    out.append(refuse("g7_raw_lit_131072_block_size_131076", f, cap=131072))
    for kind in ("raw", "rle"):
        for size in (0, 1, 15, 16, 17, 1039, 131072):
            for align in range(16):
                f = Frame()
                f.raw(rnd_bytes(align, align))
                if kind == "raw":
                    f.raw(rnd_bytes(size + 1, size))
                else:
                    f.rle(0xB0 + align, size)
                seqs = []
                if size + align:
                    seqs.append((0, 4, 1))                           # from the block's last byte
                    start = max(align - 1, 0)                         # across the block's first byte
                    seqs.append((1, 3, size + align + 4 + 1 - start))
                f.compressed(raw_lit(b"xyz"), seqs, last=True)
                out.append(case(f"g7_{kind}_block_{size}_at_{align}", finish(f)))
    f = Frame()
    f.compressed(raw_lit(b"abc"), [])
    f.raw(b"", last=True)
    out.append(case("g7_empty_last_raw_block", finish(f)))
    f = Frame()
    f.block(0, 131073, bytes(131073), last=True)
    out.append(refuse("g7_block_size_131073", f, cap=131073))
    f = Frame()
    f.compressed(raw_lit(b"", hl=2), [], last=True)
    out.append(case("g7_compressed_empty_3_bytes", f))
    f = Frame()
    f.compressed(raw_lit(b""), [], last=True)
    out.append(case("g7_compressed_empty_2_bytes", f))
    f = Frame()
    f.raw(b"content")
    f.raw(b"", last=True)
    out.append(case("g7_skippable_alone", zf.skippable(b"nothing here", 3)))
    out.append(case("g7_skippable_in_front", zf.skippable(b"", 15), f))
    out.append(case("g7_skippable_behind", f, zf.skippable(b"x" * 300)))
    return out


# ---- group 8: deliberately invalid frames ----

def _g8_base(**kw):
    f = Frame()
    f.raw(rnd_bytes(95, 16))
    f.compressed(raw_lit(rnd_bytes(96, 40)), SEQS5, last=True, **kw)
    return f


def group8(tier):
    out = []
    f = Frame()
    f.raw(b"abc")
    f.block(3, 3, b"xyz", last=True)
    out.append(refuse("g8_reserved_block_type", f))
    for bit in (1, 2, 3):
        out.append(refuse(f"g8_mode_byte_reserved_{bit}", _g8_base(reserved=bit, check=False)))
    out.append(refuse("g8_accuracy_log_above_max", _g8_base(ml=("fse", None, 10), check=False)))
    out.append(refuse("g8_symbol_beyond_alphabet", _g8_base(ll=("fse", [28] + [1] * 36, 6), check=False)))
    out.append(refuse("g8_counts_short_of_table_size", _g8_base(of=("fse", [1] * 32, 6), check=False)))
    f = Frame()
    f.compressed(huf_lit(rnd_bytes(97, 40, range(3)), streams=4, weights=[1, 1, 1, 2, 2]), [], last=True, check=False)
    out.append(refuse("g8_huffman_weights_complete_no_code", f))
    f = Frame()
    f.compressed(huf_lit(rnd_bytes(98, 99, range(13)), streams=1, weights=[1, 1] + list(range(2, 13))), [], last=True, check=False)
    out.append(refuse("g8_huffman_depth_12", f))
    out.append(refuse("g8_stream_without_padding_bit", _g8_base(padding=False, check=False)))
    for extra in (1, 8, 9):
        out.append(refuse(f"g8_stream_with_{extra}_bits_left", _g8_base(leftover=extra, check=False)))
    f = Frame()
    f.raw(rnd_bytes(99, 16))
    f.compressed(raw_lit(b"abcd"), [(2, 3, 1), (3, 3, 1)], last=True, check=False)
    out.append(refuse("g8_sequences_overrun_literals", f))
    f = Frame()
    f.raw(rnd_bytes(99, 16))
    f.compressed(raw_lit(b"abcd"), [(2, 3, 19)], last=True, check=False)
    out.append(refuse("g8_offset_before_frame", f))
    a, b = Frame(), Frame()  # the bytes in front belong to another frame
    a.raw(rnd_bytes(99, 16), last=True)
    b.compressed(raw_lit(b"abcd"), [(2, 3, 3)], last=True, check=False)
    out.append(refuse("g8_offset_into_previous_frame", a, b))
    f = Frame()
    f.block(1, 131073, b"z", last=True)
    out.append(refuse("g8_block_size_above_128k", f, cap=131073))
    return out


# ---- group 9: the decoder's own cuts ----

def group9(tier):
    out = []
    big = (1023, 1024, 1025, 2047, 2048, 2049, 70000)
    for n in big:
        f = Frame()
        f.raw(rnd_bytes(n, 20))
        f.compressed(raw_lit(rnd_bytes(n + 1, n + 7)), [(n, 5, 3), (3, 4, 9)], last=True)
        out.append(case(f"g9_ll_{n}", finish(f)))
        for off in (3, 19):
            f = Frame()
            f.raw(rnd_bytes(n, 20))
            f.compressed(raw_lit(b"abcdefg"), [(2, n, off), (3, 4, 9)], last=True)
            out.append(case(f"g9_ml_{n}_off{off}", finish(f)))
    for n in (63, 64, 65, 127, 128, 129):
        r = random.Random(n)
        seqs = [(r.randrange(0, 3), r.randrange(3, 9), r.randrange(1, 20)) for _ in range(n)]
        f = Frame()
        f.raw(rnd_bytes(n, 20))
        f.compressed(raw_lit(rnd_bytes(n + 1, sum(s[0] for s in seqs) + 5)), seqs, last=True)
        out.append(case(f"g9_{n}_sequences", finish(f)))
        f = Frame()  # no literals at all: 64 records are exactly one batch
        f.raw(rnd_bytes(n, 20))
        f.compressed(raw_lit(b""), [(0, s[1], s[2]) for s in seqs], last=True)
        out.append(case(f"g9_{n}_sequences_no_literals", finish(f)))
    for off in (1, 2, 3, 7, 16, 17):
        for ll in (1000, 1020, 1023):
            f = Frame()
            f.raw(rnd_bytes(off, 20))
            f.compressed(raw_lit(rnd_bytes(off + ll, ll + 2)), [(ll, 200, off), (1, 3000, off), (1, 3, 1)], last=True)
            out.append(case(f"g9_overlap_off{off}_after_{ll}", finish(f)))
    for r16 in range(16):
        f = Frame()
        f.raw(rnd_bytes(r16, 20))
        seqs = [(1000 + r16, 3, 5), (40, 3, 2), (100, 4, 7), (900 + r16, 3, 11), (33, 5, 1)]
        f.compressed(raw_lit(rnd_bytes(200 + r16, sum(s[0] for s in seqs) + 30 + r16)), seqs, last=True)
        out.append(case(f"g9_ring_wrap_{r16}", finish(f)))
    return out


# ---- group 10: Frame_Content_Size ----

def _sized(n, width, fcs=None):
    f = Frame(single=width != 0, window_log=17 if width == 0 else None, fcs_bytes=width, fcs=fcs)
    if n:
        f.rle(0x42, n, last=True)
    else:
        f.raw(b"", last=True)
    return f


def group10(tier):
    out = []
    for n in (0, 255, 256, 65791, 65792):
        for width in (0, 1, 2, 4, 8):
            if width == 1 and n > 255 or width == 2 and not 256 <= n <= 65791:
                continue
            out.append(case(f"g10_fcs{width}_{n}", _sized(n, width), query=n if width else 0))
    for width in (4, 8):
        out.append(refuse(f"g10_fcs{width}_4g_minus_1", _sized(0, width, fcs=(1 << 32) - 1), query=(1 << 32) - 1))
    out.append(refuse("g10_fcs8_above_4g", _sized(0, 8, fcs=(1 << 32) + 5), query=(1 << 32) + 5))
    out.append(refuse("g10_fcs_above_capacity", _sized(300, 2), cap=299))
    out.append(refuse("g10_fcs_one_more_than_content", _sized(300, 2, fcs=301)))
    out.append(refuse("g10_fcs_one_less_than_content", _sized(300, 2, fcs=299)))
    out.append(refuse("g10_fcs_0_with_content", _sized(1, 1, fcs=0)))
    f = Frame(checksum=True)  # the content checksum (skipped by the decoder, verified by libzstd in the writer's test)
    f.raw(rnd_bytes(7, 70))
    f.compressed(raw_lit(b"abc"), [(1, 5, 9)], last=True)
    out.append(case("g10_checksum", f))
    return out


GROUPS = {1: group1, 2: group2, 3: group3, 4: group4, 5: group5, 6: group6, 7: group7, 8: group8, 9: group9, 10: group10}
_corpus = {}


def corpus(g, tier):
    """Group g's cases for a tier ("emu": the smaller set; "gpu": everything), built once."""
    if (g, tier) not in _corpus:
        cases = GROUPS[g](tier)
        assert len({c.name for c in cases}) == len(cases)
        _corpus[g, tier] = cases
    return _corpus[g, tier]


def arr(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def decode_cases(backend, cases):
    """Valid cases: exact bytes, sizes, Success. Refused ones: not Success and actual size 0. Cases of similar size
    share a call (the slab's stride is the largest capacity of the call)."""
    for lo, hi in ((0, 1 << 12), (1 << 12, 1 << 18), (1 << 18, 1 << 21), (1 << 21, 1 << 25)):
        part = [c for c in cases if lo <= c.cap < hi]
        good = [c for c in part if c.ok]
        bad = [c for c in part if not c.ok]
        if good:
            try:
                check_exact(backend, [arr(c.out) for c in good], [arr(c.comp) for c in good])
            except AssertionError:
                # say which: one at a time
                for c in good:
                    outs, actual, status = run(backend, [arr(c.comp)], [c.cap])
                    assert status[0] == NvcompStatus.Success, (c.name, status[0])
                    assert actual[0] == len(c.out), (c.name, actual[0], len(c.out))
                    assert outs[0][: len(c.out)].tobytes() == c.out, c.name
                raise
        if bad:
            outs, actual, status = run(backend, [arr(c.comp) for c in bad], [c.cap for c in bad])
            for c, s, a in zip(bad, status, actual):
                assert s != NvcompStatus.Success, c.name
                assert a == 0, c.name


def libzstd_says(c):
    """The bytes libzstd decodes a case to, or None where it refuses."""
    try:
        return zstd_cpu.decompress(arr(c.comp), c.cap).tobytes()
    except RuntimeError:
        return None


# ---- the writer itself, and what libzstd says to the refusals (CPU only) ----

@needs_libzstd
@pytest.mark.parametrize("g", sorted(GROUPS))
def test_writer_against_libzstd(g):
    """Every valid frame of the corpus, both tiers, decodes with libzstd to the writer's own expansion."""
    for c in corpus(g, "gpu") + [c for c in corpus(g, "emu") if c.name not in {k.name for k in corpus(g, "gpu")}]:
        if not c.ok:
            continue
        got = libzstd_says(c)
        if c.name in LIBZSTD_REFUSES and got is None:
            continue
        assert got is not None, f"{c.name}: libzstd refuses a frame the writer calls valid"
        assert got == c.out, f"{c.name}: libzstd and the writer's expansion differ"


@needs_libzstd
def test_refusals_against_libzstd():
    """libzstd's verdict on every frame the decoder must refuse: it refuses them too, except LIBZSTD_ACCEPTS."""
    accepted = set()
    for g in GROUPS:
        for c in corpus(g, "gpu"):
            if not c.ok and libzstd_says(c) is not None:
                accepted.add(c.name)
    print("libzstd", zstd_cpu.version(), "accepts:", sorted(accepted))
    assert accepted <= LIBZSTD_ACCEPTS, sorted(accepted - LIBZSTD_ACCEPTS)
    if zstd_cpu.version() == "1.4.8":
        assert accepted == LIBZSTD_ACCEPTS, sorted(LIBZSTD_ACCEPTS - accepted)


def test_xxh64():
    assert zf.xxh64(b"") == 0xEF46DB3751D8E999
    assert zf.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    assert zf.xxh64(b"Nobody inspects the spammish repetition") == 0xFBCEA83C8A378BF1


# ---- groups 1-10 on the decoder ----

@pytest.mark.parametrize("g", sorted(GROUPS))
def test_group(backend, g):
    decode_cases(backend, corpus(g, backend.name))


def test_get_decompress_size(backend):
    """Every FCS width through the size query, up to 2^32 - 1 in the 4- and 8-byte forms."""
    cases = [c for c in corpus(10, backend.name) if c.query is not None]
    sizes = BatchedCodec(backend.lib, backend.dev, "Zstd").get_decompress_size([arr(c.comp) for c in cases])
    want = [c.query for c in cases]
    assert sizes.tolist() == want, [(c.name, s, w) for c, s, w in zip(cases, sizes.tolist(), want) if s != w]
    assert {0, 255, 256, 65791, 65792, (1 << 32) - 1, (1 << 32) + 5} <= set(want)


# ---- what the corpus holds: walked from its headers ----

def walk_more(comp):
    """Feature names of a chunk beyond tests/test_zstd.py::walk: the rows of the table in this file's coverage test."""
    b = bytes(comp)
    seen, pos, frames = set(), 0, 0
    while pos < len(b):
        magic = int.from_bytes(b[pos: pos + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            seen.add("frame:skippable")
            pos += 8 + int.from_bytes(b[pos + 4: pos + 8], "little")
            continue
        assert magic == zf.MAGIC
        frames += 1
        fhd = b[pos + 4]
        fcs_flag, single, checksum = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1
        fcs_bytes = [single, 2, 4, 8][fcs_flag]
        seen.add(f"frame:fcs{fcs_bytes}" if fcs_bytes else "frame:fcs_absent")
        if checksum:
            seen.add("frame:checksum")
        pos += 5 + (0 if single else 1) + fcs_bytes
        while True:
            bh = int.from_bytes(b[pos: pos + 3], "little")
            last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
            pos += 3
            seen.add("block:" + ["raw", "rle", "compressed", "reserved"][btype])
            if btype == 2:
                p, end = pos, pos + bsize
                lt, sf = b[p] & 3, (b[p] >> 2) & 3
                seen.add("lit:" + ["raw", "rle", "compressed", "treeless"][lt])
                if lt <= 1:
                    hl = [1, 2, 1, 3][sf]
                    seen.add(f"lit:{['raw', 'rle'][lt]}:hl{hl}")
                    regen = b[p] >> 3 if hl == 1 else (int.from_bytes(b[p: p + hl], "little") >> 4)
                    p += hl + (regen if lt == 0 else 1)
                else:
                    seen.add("streams:%d" % (1 if sf == 0 else 4))
                    hl, w = [(3, 10), (3, 10), (4, 14), (5, 18)][sf]
                    seen.add(f"lit:huf:hl{hl}")
                    csize = (int.from_bytes(b[p: p + hl], "little") >> (4 + w)) & ((1 << w) - 1)
                    if lt == 2:
                        hb = b[p + hl]
                        seen.add(f"huf:direct:{hb - 127}" if hb >= 128 else "huf:fse")
                    p += hl + csize
                n0 = b[p]
                nseq = n0 if n0 < 128 else ((n0 - 128) << 8) + b[p + 1] if n0 < 255 else b[p + 1] + (b[p + 2] << 8) + 0x7F00
                width = 1 if n0 < 128 else 2 if n0 < 255 else 3
                seen.add(f"nseq:{width}")
                p += width
                if nseq:
                    modes = b[p]
                    p += 1
                    for name, shift in (("LL", 6), ("OF", 4), ("ML", 2)):
                        mode = (modes >> shift) & 3
                        seen.add(f"seq:{name}:" + ["predefined", "rle", "fse", "repeat"][mode])
                        if mode == 1:
                            seen.add(f"{name}:sym{b[p]}")
                            seen.add(f"{name}:rle:sym{b[p]}")
                            p += 1
                        elif mode == 2:
                            counts, used = _ncount(b, p, zf.MAX_LOG[name])
                            seen.add(f"{name}:log{(b[p] & 15) + 5}")
                            seen.update(f"{name}:sym{i}" for i, c in enumerate(counts) if c)
                            if -1 in counts:
                                seen.add("fse:less_than_one")
                            p += used
                pos = end
            else:
                pos += 1 if btype == 1 else bsize
            if last:
                break
        pos += 4 if checksum else 0
    if frames > 1:
        seen.add("frame:several")
    return seen


def test_corpus_covers_the_format():
    """Everything groups 1-10 generate holds what libzstd's own output does not: the 3-byte sequence count, direct
    Huffman weights up to 128, the 8-byte FCS, every literal header width, the top LL / ML / OF codes, and (from the
    writer's trace, for no header shows them) what the repeat offsets did."""
    seen, trace = set(), set()
    for g in GROUPS:
        for c in corpus(g, "gpu"):
            trace |= c.trace
            try:
                seen |= walk_more(c.comp)
            except (AssertionError, IndexError):
                assert not c.ok, c.name  # only a frame that is invalid on purpose may stop the walker
    want = {"block:raw", "block:rle", "block:compressed", "lit:raw", "lit:rle", "lit:compressed", "lit:treeless",
            "streams:1", "streams:4", "frame:fcs_absent", "frame:checksum", "frame:several", "frame:skippable"}
    want |= {f"seq:{t}:{m}" for t in ("LL", "OF", "ML") for m in ("predefined", "rle", "fse", "repeat")}
    want |= {"nseq:1", "nseq:2", "nseq:3", "frame:fcs1", "frame:fcs2", "frame:fcs4", "frame:fcs8"}
    want |= {f"huf:direct:{n}" for n in (1, 2, 3, 127, 128)} | {"huf:fse"}
    want |= {f"lit:{k}:hl{h}" for k in ("raw", "rle") for h in (1, 2, 3)} | {"lit:huf:hl3", "lit:huf:hl4", "lit:huf:hl5"}
    want |= {f"LL:sym{c}" for c in range(36)} | {f"ML:sym{c}" for c in range(53)} | {f"OF:sym{c}" for c in range(32)}
    want |= {"LL:log5", "LL:log9", "OF:log5", "OF:log8", "ML:log5", "ML:log9", "fse:less_than_one"}
    assert want <= seen, sorted(want - seen)
    want_trace = {f"rep:{k}:{z}" for k in (1, 2, 3) for z in ("ll", "ll0")}
    want_trace |= {"rep:zero", "rep:before_frame", "rep:across_raw", "rep:across_rle", "off:before_frame",
                   "huf:depth11", "huf:depth12", "huf:fse:255"}
    assert want_trace <= trace, sorted(want_trace - trace)
    # offset codes in RLE mode other than 0, and the ones no chunk can hold: from the walked headers
    want_rle = {f"OF:rle:sym{c}" for c in range(32)}
    assert want_rle <= seen, sorted(want_rle - seen)


# ---- group 11: structured fuzz ----

def random_frame(r, limit=4096):
    """A random valid description: blocks of every type, literals of every type, sequences with distances and repeat
    codes, every table mode that is possible at that point; at most `limit` bytes of output."""
    f = Frame()
    alphabet = [r.randrange(256) for _ in range(r.choice((2, 5, 20, 60)))]
    nblocks = r.randrange(1, 5)
    for k in range(nblocks):
        last = k == nblocks - 1
        room = limit - len(f.out)
        kind = r.randrange(6) if room > 200 else 0
        if kind == 0:
            f.raw(rnd_bytes(r.random(), r.randrange(0, min(room, 40) + 1)), last=last)
            continue
        if kind == 1:
            f.rle(r.randrange(256), r.randrange(0, min(room, 300) + 1), last=last)
            continue
        nlit = r.choice((0, 3, 30, 200, min(room // 2, 1100)))
        data = bytes(r.choice(alphabet) for _ in range(nlit))
        lk = r.randrange(4)
        if lk == 0 or nlit < 8 or len(set(data)) < 2:
            lit = raw_lit(data, r.choice([h for h in (1, 2, 3) if nlit < 1 << (5, 12, 20)[h - 1]]))
        elif lk == 1:
            lit = rle_lit(data[0], nlit, r.choice([h for h in (1, 2, 3) if nlit < 1 << (5, 12, 20)[h - 1]]))
            data = lit["data"]
        elif lk == 2 and f.huf is not None and set(data) <= set(f.huf.code):
            lit = treeless_lit(data, *r.choice(((1, 0), (4, 1), (4, 2), (4, 3)) if nlit < 1024 else ((4, 2), (4, 3))))
        else:
            streams, sf = r.choice(((1, 0), (4, 1), (4, 2), (4, 3)) if nlit < 1000 else ((4, 2), (4, 3)))
            desc = "direct" if max(data) <= 128 and r.random() < 0.5 else "fse"
            lit = huf_lit(data, streams, sf, desc=desc, depth=r.choice((11, 11, 8)))
            if streams == 4 and nlit == 5:
                lit = raw_lit(data)
        seqs, used, produced = [], 0, len(f.out)
        budget = room - nlit
        for _ in range(r.choice((0, 1, 2, 10, 70, 140))):
            ll = min(r.choice((0, 0, 1, 2, 5, 17, 40, 300)), nlit - used)
            ml = r.choice((3, 3, 4, 5, 8, 20, 35, 70, 300, 1100))
            if ml > budget:
                break
            here = produced + ll
            if here == 0:
                continue
            pick = r.random()
            reps = list(f.rep) if not seqs else reps
            if pick < 0.4:
                code = r.choice((REP1, REP2, REP3))
                idx = zf._REP[code] - 1 + (ll == 0)
                off = reps[idx] if idx < 3 else reps[0] - 1
                if off < 1 or off > here:
                    continue
                reps = [off] + [x for i, x in enumerate(reps) if i != min(idx, 2)] if idx else reps
                seqs.append((ll, ml, code))
            else:
                off = r.choice((1, 2, 3, 4, 7, 8, 16, 17, here, max(here - 1, 1), r.randrange(1, here + 1)))
                off = min(off, here)
                reps = [off, reps[0], reps[1]]
                seqs.append((ll, ml, off))
            used += ll
            produced = here + ml
            budget -= ml
        if not seqs and nlit == 0:
            lit = raw_lit(b"", r.choice((2, 3)))  # not the 2-byte block of LIBZSTD_REFUSES: libzstd checks this test too
        spec = {}
        for name, key, log in (("LL", "ll", r.choice((5, 6, 9))), ("OF", "of", r.choice((5, 8))), ("ML", "ml", r.choice((5, 7, 9)))):
            codes = {"LL": [zf.ll_code(s[0]) for s in seqs], "ML": [zf.ml_code(s[1]) for s in seqs],
                     "OF": [((zf._REP[s[2]] if s[2] in zf._REP else s[2] + 3).bit_length() - 1) for s in seqs]}[name]
            options = ["fse", "fse_low"]
            default = zf.DEFAULTS[name][0]
            if all(c < len(default) and default[c] for c in codes):
                options.append("predefined")
            if len(set(codes)) == 1:
                options.append("rle")
            prev = f.tables[name]
            if prev is not None and all(c in prev.sym for c in codes):
                options += ["repeat", "repeat"]
            o = r.choice(options)
            spec[key] = {"fse": ("fse", None, log), "fse_low": ("fse", None, log, -1), "predefined": ("predefined",),
                         "rle": ("rle",), "repeat": ("repeat",)}[o]
        f.compressed(lit, seqs, last=last, **spec)
    f.fcs_bytes = r.choice([w for w in (1, 2, 4, 8) if (w != 1 or len(f.out) < 256) and (w != 2 or len(f.out) >= 256)])
    return f


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_structured_fuzz(backend, seed):
    """Random valid descriptions in one call: 48 on the emulator, 600 on the card."""
    r = random.Random(seed)
    n = 48 if backend.name == "emu" else 600
    cases = []
    for i in range(n):
        parts = [random_frame(r) for _ in range(1 if r.random() < 0.8 else 2)]
        if r.random() < 0.1:
            parts.insert(r.randrange(len(parts) + 1), zf.skippable(rnd_bytes(i, r.randrange(20)), r.randrange(16)))
        cases.append(case(f"fuzz_{seed}_{i}", *parts))
    if zstd_cpu.load() is not None:
        for c in cases:
            assert libzstd_says(c) == c.out, c.name
    check_exact(backend, [arr(c.out) for c in cases], [arr(c.comp) for c in cases])


# ---- group 12: mutation fuzz ----

def mutants(n=200, seed=12):
    """(chunk, what was done, capacity): byte flips, truncations and one inserted byte in small valid frames of groups
    1-9. Those frames have Single_Segment set and no checksum."""
    r = random.Random(seed)
    pool = [c for g in range(1, 10) for c in corpus(g, "emu") if c.ok and len(c.comp) <= 600 and c.cap <= 8192
            and c.name not in LIBZSTD_REFUSES]
    out = []
    for i in range(n):
        c = pool[r.randrange(len(pool))]
        b = bytearray(c.comp)
        kind = r.randrange(3)
        at = r.randrange(4, len(b))  # behind the magic number
        if kind == 0:
            mask = 1 << r.randrange(8) if r.random() < 0.5 else r.randrange(1, 256)
            b[at] ^= mask
            what = f"{c.name}: byte {at} ^ 0x{mask:02x}"
        elif kind == 1:
            del b[at:]
            what = f"{c.name}: cut at {at}"
        else:
            v = r.randrange(256)
            b.insert(at, v)
            what = f"{c.name}: 0x{v:02x} inserted at {at}"
        out.append((bytes(b), what, c.cap + 64))
    return out


@needs_libzstd
def test_mutation_fuzz(backend):
    """About 200 damaged frames in one call: the call returns, the guard bytes survive (run() checks them), a refusal
    reports size 0, and what the decoder accepts libzstd accepts too, with the same bytes.

    The reverse is no failure; each chunk libzstd decodes and the decoder refuses is printed. With this seed there is
    none. Where one appears, expect a kind LIBZSTD_ACCEPTS names: a flip that shortens a table description by a byte,
    for instance, leaves bits in front of the sequences' stream that libzstd 1.4.8 does not look at."""
    ms = mutants()
    caps = [m[2] for m in ms]
    outs, actual, status = run(backend, [arr(m[0]) for m in ms], caps)
    stricter = []
    for (comp, what, cap), o, a, s in zip(ms, outs, actual, status):
        try:
            ref = zstd_cpu.decompress(arr(comp), cap).tobytes()
        except RuntimeError:
            ref = None
        if s == NvcompStatus.Success:
            assert ref is not None, f"{what}: decoded here, refused by libzstd"
            assert a == len(ref) and o[: len(ref)].tobytes() == ref, what
        else:
            assert a == 0, what
            if ref is not None:
                stricter.append(what)
    for what in stricter:
        print("libzstd decodes, the decoder refuses:", what)
    assert sum(s == NvcompStatus.Success for s in status) >= 5  # some mutations are harmless: both sides are exercised
