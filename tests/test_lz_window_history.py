"""Matches into the history the output window still holds (common/lz_window.hip.h: execute_window_batch;
common/lz_out_window.hip.h: out_make_room).

In the one-wave LZ4 decoder (the executor's HISTORY switch) a short match whose whole source lies in [valid_lo, flushed)
-- flushed, but still in the wave's LDS -- is copied in LDS like a near match; one whose source starts in front of
valid_lo is fetched from the output buffer, as every flushed source is in the other decoders. The two must agree to the
byte wherever the boundary is, and the boundary moves: the window slides only when a batch does not fit, the run
executor and a streamed sequence write straight to the output buffer and restart the window behind them. The tests do
not know where valid_lo or the flushed mark are, nor what a slide keeps: they sweep the source byte by byte across every
place they can be.

Expected bytes are the CPU decoder's (zlib's for DEFLATE), and before any kernel is judged they must equal a plain Python
expansion of the same sequences. Literal bytes are random, so a copy from a wrong place shows. Every chunk is decoded
with its exact size as capacity, through every decode path (`lz_path`), on the emulator and on the card.

What a batch is, for the builders below: at most 64 sequences and 2 048 bytes, in stream order. So behind 64 sequences
everything in front of them is flushed, whatever the batches were."""
import ctypes as C
import itertools
import os
import re
import sys
import tempfile
import zlib

import numpy as np
import pytest

import deflate_streams as ds
from nvcomp_amd._lib import NvcompStatus
from test_lz_window_masks import _expand, _lz4_block, _snappy_block, check

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (4, 5, 8, 15, 16, 17, 31, 32)
MAX_BLOCK = 8192
WINDOW = 2048 + 64 + 32  # the output window (common/lz_ring.hip.h); the builders only need "about 2 KiB"


class Plan:
    """Sequences (literal bytes, offset, match length) in the making, and the output position they have reached."""

    def __init__(self, seed):
        self.rng, self.seqs, self.pos = np.random.RandomState(seed), [], 0

    def add(self, lit, off, mlen):
        assert 1 <= off <= self.pos + len(lit) and off < 65536
        self.seqs.append((bytes(lit), int(off), int(mlen)))
        self.pos += len(lit) + mlen

    def copy_from(self, lit, src, mlen):
        """lit, then a match whose source starts at output position src"""
        self.add(lit, self.pos + len(lit) - src, mlen)

    def literals(self, n):
        """n random bytes, then four more of the last one (period 1: the whole wave copies such a match in LDS; it is
        neither fetched nor a lane's own copy)"""
        self.add(self.rng.bytes(n), 1, 4)

    def filler(self, n=64):
        """n sequences of five bytes that no counter of the lane-parallel matches sees"""
        for _ in range(n):
            self.literals(1)

    def align_to(self, residue, src):
        """a filler match (from src) that brings the output position to `residue` modulo 4"""
        need = (residue - self.pos) & 3
        if need:
            self.copy_from(b"", src, 4 + need)

    def done(self, tail=12):
        return self.seqs, self.rng.bytes(tail)


# ---- the cases ---------------------------------------------------------------------------------------------------

HEAD = 240  # random bytes at the chunk's start: the sources of the no-slide cases


def no_slide(seed, literals_in_front, pick):
    """Under 2 KiB: the window never slides and holds the chunk from its first byte. HEAD random bytes, 64 fillers (HEAD is
    flushed from here on), then every length at every destination residue modulo 4; pick(i, dst, mlen) -> source."""
    p = Plan(seed)
    p.literals(HEAD)
    p.filler()
    first = len(p.seqs)
    for i, (mlen, da) in enumerate(itertools.product(LENGTHS, range(4))):
        nlit = 1 + i % 3 if literals_in_front else 0
        p.align_to((da - nlit) & 3, 7 + 3 * i)
        assert (p.pos + nlit) & 3 == da
        p.copy_from(p.rng.bytes(nlit), pick(i, p.pos + nlit, mlen), mlen)
    assert p.pos + 12 < 2048
    return p.done(), first


def from_head(i, dst, mlen):
    """sources in the chunk's first bytes -- 0, 1, 2 and 3 among them -- all inside HEAD"""
    return (0, 1, 2, 3, 5, 16, 17, 63, 100, 129, 191, HEAD - mlen - 16)[i % 12]


def by_distance(i, dst, mlen):
    """distances from 4 (the same batch) to the chunk's start"""
    d = (4, 5, 7, 8, 12, 16, 17, 31, 32, 33, 48, 64, 100, 200, 333, dst)[i % 16]
    return dst - (d if d <= dst else dst)


PREFIX_RUNS = 3
PREFIX = PREFIX_RUNS * 604  # three sequences of 600 literals: most of a window, flushed by the time the sweep runs
SWEEP = 144


def across_slide(seed, fill, span_lo):
    """PREFIX bytes that fill the window, a sequence of `fill` literals that does not fit behind them -- its batch slides
    the window, and what the slide keeps depends on what that batch needs --, then SWEEP matches whose sources start at
    span_lo, span_lo + 1, ..."""
    p = Plan(seed)
    for _ in range(PREFIX_RUNS):
        p.literals(600)
    assert p.pos == PREFIX and PREFIX + fill + 4 > WINDOW
    p.literals(fill)
    for k in range(SWEEP):
        p.copy_from(p.rng.bytes(k % 5 == 0), span_lo + k, LENGTHS[(k + k // 8) % 8])
    return p.done()


def slide_chunks(seed):
    """(fill, span_lo) so that the sweeps cover, byte by byte: all of the prefix and the fill for a batch that needs little
    (a slide may keep nearly all of the window), the last 1 152 bytes in front of the slide for one that needs a KiB
    more, the last 288 for one that leaves room for 32 .. 210 bytes."""
    plan = [(340, lo) for lo in range(0, PREFIX + 344, SWEEP)]
    plan += [(1000, lo) for lo in range(PREFIX - 8 * SWEEP, PREFIX, SWEEP)]
    plan += [(1900, lo) for lo in range(PREFIX - 2 * SWEEP, PREFIX, SWEEP)]
    return [across_slide(seed + i, fill, lo) for i, (fill, lo) in enumerate(plan)], plan


def straddle_flushed(seed, r):
    """64 sequences (one batch: the flushed mark is now the 16-byte boundary at or below their end G, and r = 0 .. 15 moves
    G through every residue), 48 literals, then matches of 8 and 12 bytes whose source END sweeps from G - 28 to G + 28."""
    p = Plan(seed)
    p.literals(100 + r)
    p.filler(63)
    g = p.pos
    p.literals(48)
    for e in range(g - 28, g + 29):
        mlen = 8 + 4 * (e & 1)
        p.copy_from(b"", e - mlen, mlen)
    assert len(p.seqs) - 64 <= 64
    return p.done(), g


RUNS = 22


def behind_runs(seed):
    """22 runs of period 8 (8 literals, then 250 bytes of them again and again): the block shrinks more than 8 x, the
    decoders hand it to the loop that holds the run executor, and that writes the runs straight to the output buffer. The
    window restarts with the last 16 bytes. Then short matches from all over the runs (at the joints of two runs, where the
    bytes change) and, byte by byte, from the last 40 bytes."""
    p = Plan(seed)
    for _ in range(RUNS):
        p.add(p.rng.bytes(8), 8, 250)
    end = p.pos
    for k in range(40):
        p.copy_from(b"", end - 40 + k, LENGTHS[k % 4])
    for k in range(48):
        joint = 258 * (1 + (k * 5) % (RUNS - 1))
        p.copy_from(p.rng.bytes(k % 3 == 0), joint - 12 + k % 9, LENGTHS[k % 8])
    return p.done(), end


def behind_streamed(seed):
    """A literal run of 4 KiB is copied from the stream to the output buffer, and the window restarts empty behind it at E.
    40 literals, then matches whose source sweeps from E - 40 to E + 20, and matches from deep inside the run."""
    p = Plan(seed)
    p.literals(4096)
    end = p.pos
    p.literals(40)
    for k in range(60):
        p.copy_from(b"", end - 40 + k, LENGTHS[k % 8] if k < 40 else 4 + k % 5)
    for k in range(32):
        p.copy_from(p.rng.bytes(k % 2), 3 + 127 * k, LENGTHS[k % 8])
    return p.done(), end


def split_matches(seqs, most=64):
    """The same bytes with no match longer than `most` (Snappy's copies end at 64 bytes)."""
    out = []
    for lit, off, mlen in seqs:
        while mlen > most:
            out.append((lit, off, most))
            lit, mlen = b"", mlen - most
        out.append((lit, off, mlen))
    return out


FORMATS = ["LZ4", "Snappy"]
_cache = {}


def built(fmt, oracle, name, make):
    """(streams, expected outputs, what make() returned): built, and checked against the Python expansion, once."""
    if (fmt, name) not in _cache:
        made = make()
        if fmt == "LZ4":
            block, dec = _lz4_block, oracle.lz4_decompress
        else:  # libsnappy where the reference-side shim exists
            block, dec = _snappy_block, (oracle.ref_snappy_decompress if oracle.have_ref() else oracle.snappy_decompress)
        streams, want = [], []
        for seqs, tail in made["chunks"]:
            if fmt == "Snappy":
                seqs = split_matches(seqs)
            stream, plain = block(seqs, tail), _expand(seqs, tail)
            assert plain.size <= MAX_BLOCK and stream.size <= MAX_BLOCK, name
            rc, out = dec(stream, plain.size)
            assert rc == 0 and np.array_equal(out, plain), f"{fmt} {name}: the CPU decoder does not read the hand-built block as written"
            streams.append(stream)
            want.append(out)
        _cache[fmt, name] = (streams, want, made)
    return _cache[fmt, name]


def make_no_slide():
    chunks, firsts = [], []
    for seed, (lits, pick) in enumerate(itertools.product((False, True), (from_head, by_distance))):
        chunk, first = no_slide(40 + seed, lits, pick)
        chunks.append(chunk)
        firsts.append(first)
    return {"chunks": chunks, "firsts": firsts}


def sources(seqs):
    """(source start, length, destination) of every match"""
    pos, out = 0, []
    for lit, off, mlen in seqs:
        out.append((pos + len(lit) - off, mlen, pos + len(lit)))
        pos += len(lit) + mlen
    return out


# ---- bytes -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_no_slide(backend, lz_path, oracle, fmt):
    """Output under 2 KiB: lengths {4, 5, 8, 15, 16, 17, 31, 32} at every destination residue, with and without literals in
    front, sources in the chunk's first bytes (0, 1 and 2 among them) and at distances from 4 to the chunk's start."""
    streams, want, made = built(fmt, oracle, "no_slide", make_no_slide)
    assert all(w.size < 2048 for w in want)
    for (seqs, _), first in zip(made["chunks"], made["firsts"]):
        late = sources(seqs)[first:]
        assert {(m, d & 3) for _, m, d in late} >= set(itertools.product(LENGTHS, range(4)))
    head = [s for (seqs, _), first in zip(made["chunks"][::2], made["firsts"][::2]) for s, _, _ in sources(seqs)[first:]]
    assert {0, 1, 2, 3} <= set(head)
    far = sources(made["chunks"][1][0])[made["firsts"][1]:]
    assert 4 in {d - s for s, _, d in far} and 0 in {s for s, _, _ in far}
    assert not any(lit for lit, _, _ in made["chunks"][0][0][made["firsts"][0]:])
    assert any(lit for lit, _, _ in made["chunks"][2][0][made["firsts"][2]:])
    check(backend, fmt, streams, want, "matches into unslid history")


@pytest.mark.parametrize("fmt", FORMATS)
def test_across_slide(backend, lz_path, oracle, fmt):
    """A full window, a batch that forces the slide, then sources that sweep byte by byte over everything a slide may keep."""
    streams, want, made = built(fmt, oracle, "slide", lambda: dict(zip(("chunks", "plan"), slide_chunks(100))))
    swept = {}
    for (seqs, _), (fill, lo) in zip(made["chunks"], made["plan"]):
        got = [s for s, _, _ in sources(seqs)[PREFIX_RUNS + 1:]]
        assert got == list(range(lo, lo + SWEEP))
        swept.setdefault(fill, set()).update(got)
    assert swept[340] >= set(range(PREFIX + 344))                # whatever a slide keeps of a window of 2 144 bytes
    assert swept[1000] >= set(range(PREFIX - 1152, PREFIX))      # room for at most 2 144 - 30 - 1 004 bytes
    assert swept[1900] >= set(range(PREFIX - 288, PREFIX))       # room for at most 210; at least 32 stay
    check(backend, fmt, streams, want, "matches across a slide")


@pytest.mark.parametrize("fmt", FORMATS)
def test_straddling_flushed(backend, lz_path, oracle, fmt):
    """Sources that end below, at and above the flushed mark, for every residue modulo 16 of the batch's end."""
    streams, want, made = built(fmt, oracle, "flushed", lambda: dict(zip(
        ("chunks", "ends"), zip(*[straddle_flushed(200 + r, r) for r in range(16)]))))
    assert {g & 15 for g in made["ends"]} == set(range(16))
    for (seqs, _), g in zip(made["chunks"], made["ends"]):
        ends = {s + m for s, m, _ in sources(seqs)[65:]}
        assert ends == set(range(g - 28, g + 29))
    check(backend, fmt, streams, want, "sources across the flushed mark")


@pytest.mark.parametrize("fmt", FORMATS)
def test_behind_run_executor(backend, lz_path, oracle, fmt):
    """Short matches into what the run executor wrote straight to the output buffer: fetched, not read from a window that
    never held them."""
    streams, want, made = built(fmt, oracle, "runs", lambda: dict(zip(("chunks", "end"), zip(*[behind_runs(300)]))))
    assert want[0].size > 8 * streams[0].size, "the block shrinks more than 8 x: the loop with the run executor takes it"
    end = made["end"][0]
    late = [s for s, m, _ in sources(made["chunks"][0][0])[RUNS:]]
    assert set(range(end - 40, end)) <= set(late) and min(late) < 300
    check(backend, fmt, streams, want, "matches behind the run executor")


@pytest.mark.parametrize("fmt", FORMATS)
def test_behind_streamed_sequence(backend, lz_path, oracle, fmt):
    """The same behind a literal run of 4 KiB, which is streamed to the output buffer."""
    streams, want, made = built(fmt, oracle, "streamed", lambda: dict(zip(("chunks", "end"), zip(*[behind_streamed(400)]))))
    end = made["end"][0]
    assert len(made["chunks"][0][0][0][0]) >= 4096
    late = [s for s, m, _ in sources(made["chunks"][0][0])[2:]]
    assert set(range(end - 40, end + 20)) <= set(late) and min(late) < 16
    check(backend, fmt, streams, want, "matches behind a streamed sequence")


# ---- DEFLATE: matches of three bytes -------------------------------------------------------------------------------

def deflate_streams():
    """Fixed-code blocks of random literals and three-byte matches: one under 1 KiB whose sources sweep the chunk's first
    380 bytes, one of 5 KiB (the window slides many times) whose distances sweep from 4 to 700 and from 600 to 1 500."""
    out = []
    r = np.random.RandomState(7)
    s, syms, pos = ds.Stream(), [], 0
    syms.append(r.bytes(400))
    pos = 400
    for k in range(150):
        if k % 4 == 0:
            syms.append(r.bytes(1))
            pos += 1
        syms.append((3, pos - (k * 7) % 380 if k > 2 else pos - k))
        pos += 3
    out.append(s.fixed(syms, final=True))
    s, syms = ds.Stream(), [r.bytes(700)]
    pos = 700
    for d in itertools.chain(range(4, 700), range(600, 1500, 2)):
        if d % 5 == 0:
            syms.append(r.bytes(1))
            pos += 1
        syms.append((3, min(d, pos)))
        pos += 3
    out.append(s.fixed(syms, final=True))
    return out


def test_deflate_three_byte_matches(backend):
    """DEFLATE's three-byte matches (RING_LITERALS) into window history: sources at the chunk's positions 0, 1 and 2,
    distances from 4 on, across many slides."""
    made = deflate_streams()
    comp, want = [], []
    for s in made:
        data = s.bytes()
        assert len(data) <= MAX_BLOCK and len(s.out) <= MAX_BLOCK
        assert zlib.decompressobj(-15).decompress(data) == bytes(s.out), "zlib does not read the stream as written"
        comp.append(np.frombuffer(data, dtype=np.uint8))
        want.append(np.frombuffer(bytes(s.out), dtype=np.uint8))
    codec = backend.codec("Deflate")
    for mis in (0, 3):
        outs, actual, status = codec.decompress(comp, [w.size for w in want], base_misalign=mis)
        assert (status == NvcompStatus.Success).all() and actual.tolist() == [w.size for w in want]
        for o, w in zip(outs, want):
            assert np.array_equal(o, w), f"shift {mis}: differs from byte {int(np.flatnonzero(o != w)[0])} on"


# ---- the counters (emulator only) --------------------------------------------------------------------------------------

def chase_stats():
    """The LZ_STAT counters of the emulator build that forces one wave per chunk (text on stderr: dumped into a file, read
    back; as tests/test_deflate_format.py::emu_stats)."""
    lib = C.CDLL(os.path.join(REPO, "tests", "emu", "libnvcomp_emu_chase.so"))
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


def counted(fmt, stream, want):
    import conftest

    codec = conftest.Backend("emu", conftest.emu_path_library("chase"), conftest.HostDevice()).codec(fmt)
    before = chase_stats()
    outs, actual, status = codec.decompress([stream], [want.size])
    assert status.tolist() == [NvcompStatus.Success] and np.array_equal(outs[0], want)
    after = chase_stats()
    return {k: after[k] - before.get(k, 0) for k in after}


@pytest.mark.parametrize("fmt", FORMATS)
def test_history_is_read_from_the_window(oracle, fmt):
    """A block under 2 KiB in which every lane-parallel match has a flushed source the window still holds. LZ4: none is
    fetched, each is counted as a match into history. (A reclassification that silently does nothing passes every byte
    test above.) Snappy, whose decoder leaves the switch off: each is fetched but the ones from the chunk's first three
    bytes, which the whole wave copies. And the block of runs does reach the run executor."""
    streams, want, made = built(fmt, oracle, "no_slide", make_no_slide)
    seqs, first = made["chunks"][0][0], made["firsts"][0]
    late = sources(seqs)[first:]
    assert all(s + m <= HEAD for s, m, _ in late) and all(off == 1 for _, off, _ in seqs[:first])
    n = counted(fmt, streams[0], want[0])
    if fmt == "LZ4":
        assert n["match_far_lanes"] == 0 and n["match_hist_lanes"] == len(late), n
    else:
        assert n["match_hist_lanes"] == 0 and n["match_far_lanes"] == sum(s >= 3 for s, _, _ in late), n
    streams, want, made = built(fmt, oracle, "runs", lambda: dict(zip(("chunks", "end"), zip(*[behind_runs(300)]))))
    n = counted(fmt, streams[0], want[0])
    assert n["run_batches"] >= 1 and n["match_far_lanes"] >= 48, n
