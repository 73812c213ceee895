"""The lane paths of the window executor (common/lz_window.hip.h: execute_window_batch) on hand-built LZ4 and Snappy
streams: far matches (loaded from the output already written: none, one, all 64 lanes of a batch; every short length; a
source that ends at the flushed boundary; a source in the last 32 bytes of the capacity), literal runs of every size class
(0 .. 33 bytes; across the wrap of the 2 KiB input ring; behind what the ring holds), every input and output alignment,
and one corrupt stream per format. Everything is compared with the CPU oracle's decoders; every output slot is followed by
a guard pattern (BatchedCodec.decompress).

The emulator runs the chunks once through the build that sends every batch to the persistent one-wave-per-chunk kernel;
the card runs them as a batch of 4 097 chunks, the size from which the shipped library launches that kernel."""
import numpy as np
import pytest

from nvcomp_amd._lib import NvcompStatus

FAR_LENGTHS = [4, 5, 8, 9, 15, 16, 17, 31, 32, 33]  # 33: not a lane's match any more (the whole wave copies it)
LIT_LENGTHS = [0, 1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33]
PREFIX_SEQS = 64   # a batch is at most 64 sequences: the prefix below is the first batch, what follows reads it from HBM
PREFIX_BYTES = 12 * PREFIX_SEQS
GPU_BATCH = 4097
MAX_CHUNK = 3072


class Lz4Stream:
    """An LZ4 block written sequence by sequence, and what it decodes to."""

    def __init__(self):
        self.stream, self.out = bytearray(), bytearray()

    @staticmethod
    def _ext(n):
        b = bytearray()
        while n >= 255:
            b.append(255)
            n -= 255
        b.append(n)
        return b

    def seq(self, lit, off, mlen):
        assert mlen >= 4 and 1 <= off <= len(self.out) + len(lit)
        self.stream.append((min(len(lit), 15) << 4) | min(mlen - 4, 15))
        if len(lit) >= 15:
            self.stream += self._ext(len(lit) - 15)
        self.stream += lit
        self.stream += bytes([off & 255, off >> 8])
        if mlen - 4 >= 15:
            self.stream += self._ext(mlen - 4 - 15)
        self._emit(lit, off, mlen)

    def last(self, lit):
        assert len(lit) >= 5  # the format's end: the last five bytes are literals
        self.stream.append(min(len(lit), 15) << 4)
        if len(lit) >= 15:
            self.stream += self._ext(len(lit) - 15)
        self.stream += lit
        self.out += lit
        return np.frombuffer(bytes(self.stream), dtype=np.uint8), np.frombuffer(bytes(self.out), dtype=np.uint8)

    def _emit(self, lit, off, mlen):
        self.out += lit
        for _ in range(mlen):
            self.out.append(self.out[-off])


class SnappyStream(Lz4Stream):
    """The same sequences as Snappy elements: a literal element (if any) and one copy with a two-byte offset."""

    def _literal(self, lit):
        if not lit:
            return
        n = len(lit) - 1
        if n < 60:
            self.stream.append(n << 2)
        else:
            assert n < 256
            self.stream += bytes([60 << 2, n])
        self.stream += lit

    def seq(self, lit, off, mlen):
        assert 1 <= mlen <= 64 and 1 <= off <= len(self.out) + len(lit)
        self._literal(lit)
        self.stream += bytes([2 | ((mlen - 1) << 2), off & 255, off >> 8])
        self._emit(lit, off, mlen)

    def last(self, lit):
        self._literal(lit)
        self.out += lit
        n, pre = len(self.out), bytearray()
        while n >= 128:
            pre.append((n & 127) | 128)
            n >>= 7
        pre.append(n)
        return np.frombuffer(bytes(pre + self.stream), dtype=np.uint8), np.frombuffer(bytes(self.out), dtype=np.uint8)


def _prefix(cls, rng):
    """64 sequences of 8 fresh literals and a 4-byte copy of them: 768 bytes that no later byte repeats by chance."""
    b = cls()
    for _ in range(PREFIX_SEQS):
        b.seq(rng.bytes(8), 8, 4)
    return b


def far_batch_chunk(cls, rng, far_lanes, lengths, src_end=None):
    """The prefix, then 64 sequences of one literal and a match: lanes in `far_lanes` copy from the prefix (far: their
    source is in HBM only), the others from the bytes right behind them (near: the window holds the source).
    src_end: where the far sources END (default: spread over the prefix's first half)."""
    b = _prefix(cls, rng)
    if 0 not in far_lanes:
        b.seq(rng.bytes(7), 7, 4)  # (a near lane 0 needs bytes of its own batch behind it)
    for j in range(64):
        mlen = lengths[j % len(lengths)]
        lit = rng.bytes(1)
        pos = len(b.out) + 1
        if j in far_lanes:
            src = (src_end - mlen) if src_end is not None else 16 + 5 * j
            b.seq(lit, pos - src, mlen)
        else:
            b.seq(lit, 4 + j % 5, mlen)
    return b.last(rng.bytes(12))


def tail_source_chunk(cls, rng, src):
    """A match whose source is flushed but lies in the last 32 bytes of the (exact) capacity: the 16-byte loads of a far
    match would leave the buffer, so it must not be one (the copy paths inside the window take it)."""
    b = _prefix(cls, rng)
    b.seq(rng.bytes(1), PREFIX_BYTES + 1 - src, 8)
    out = b.last(rng.bytes(12))
    assert src > out[1].size - 32 and src + 8 <= PREFIX_BYTES
    return out


def literal_chunk(cls, rng, rotate):
    """Literal runs of every size class, each followed by a near match; `rotate` moves the classes over the lanes."""
    b = cls()
    b.seq(rng.bytes(9), 9, 4)
    for j in range(96):
        n = LIT_LENGTHS[(j + rotate) % len(LIT_LENGTHS)]
        b.seq(rng.bytes(n), 4 + j % 7, 4 + j % 3)
    return b.last(rng.bytes(5 + rotate))


def long_literal_stream_chunk(cls, rng, phase, run, lead=0):
    """A stream of more than 2 KiB that is literal runs of `run` bytes back to back: whatever the stream's alignment, one
    of the phases puts a run across the end of the 2 KiB input ring (inside its 16-byte mirror, and behind it).
    lead: that many short sequences first -- a whole batch that ends in the middle of the ring's first KiB, so that the
    batch behind it is parsed while the ring holds the stream's first 2 KiB only: the run that crosses that edge is not
    resident when its lane wants it (the whole wave copies it from the stream)."""
    b = cls()
    b.seq(rng.bytes(4 + phase), 4, 4)
    for _ in range(lead):
        b.seq(rng.bytes(12), 12, 4)
    while len(b.stream) < 2900 - phase and len(b.out) < MAX_CHUNK - 2 * (run + 4) - 16:
        b.seq(rng.bytes(run), run, 4)
    return b.last(rng.bytes(6))


def corrupt_chunk(cls, rng):
    """A match offset beyond the output produced so far, in the second batch of an otherwise valid stream."""
    b = _prefix(cls, rng)
    b.seq(rng.bytes(3), 5, 6)
    at = len(b.stream)
    b.seq(rng.bytes(2), 9, 5)
    stream, _ = b.last(rng.bytes(12))
    stream = stream.copy()
    head = stream.size - len(b.stream)  # Snappy: the preamble in front
    lit_header = 1  # both formats: one byte in front of the two literals (LZ4: the token; Snappy: the literal's tag)
    o = head + at + lit_header + 2 + (1 if cls is SnappyStream else 0)
    off = len(b.out) + 4096
    stream[o], stream[o + 1] = off & 255, off >> 8
    return stream


def build_cases(cls):
    rng = np.random.RandomState(20 if cls is Lz4Stream else 21)
    cases = []  # (name, stream, expected)
    add = lambda name, pair: cases.append((name, pair[0], pair[1]))
    add("far_none", far_batch_chunk(cls, rng, set(), FAR_LENGTHS))
    for lane in (0, 17, 63):
        add(f"far_one_{lane}", far_batch_chunk(cls, rng, {lane}, FAR_LENGTHS))
    add("far_all", far_batch_chunk(cls, rng, set(range(64)), FAR_LENGTHS))
    for mlen in FAR_LENGTHS:  # a batch whose far matches all have one length (8 dword steps, 4, 2)
        add(f"far_all_len{mlen}", far_batch_chunk(cls, rng, set(range(64)), [mlen]))
        add(f"far_half_len{mlen}", far_batch_chunk(cls, rng, set(range(0, 64, 2)), [mlen]))
    # a far source that ends exactly at the flushed boundary: the boundary is the last multiple of 16 (by address) in
    # front of the batch, so for every output alignment one of sixteen ends hits it; the ends behind it are not far
    for e in range(PREFIX_BYTES - 15, PREFIX_BYTES + 4):
        add(f"far_end_{e}", far_batch_chunk(cls, rng, {5, 40}, [4, 9, 17, 32], src_end=e))
    for src in range(PREFIX_BYTES + 1 + 8 + 12 - 31, PREFIX_BYTES - 8 + 1):
        add(f"far_tail_{src}", tail_source_chunk(cls, rng, src))
    for rotate in range(len(LIT_LENGTHS)):
        add(f"literals_{rotate}", literal_chunk(cls, rng, rotate))
    for phase in range(0, 36, 1):
        add(f"ring_wrap_{phase}", long_literal_stream_chunk(cls, rng, phase, 32 if phase % 3 else 17))
    for phase in range(0, 36, 3):
        add(f"ring_edge_{phase}", long_literal_stream_chunk(cls, rng, phase, 32 if phase % 2 else 24, lead=63))
    return cases


_cache = {}


def cases_for(fmt, oracle):
    """Streams, the CPU oracle's decode of them (computed once per format, shared by both backends) and the corrupt stream."""
    if fmt not in _cache:
        cls = Lz4Stream if fmt == "LZ4" else SnappyStream
        dec = oracle.lz4_decompress if fmt == "LZ4" else oracle.snappy_decompress
        cases = build_cases(cls)
        ref = []
        for name, stream, expected in cases:
            assert stream.size <= MAX_CHUNK and expected.size <= MAX_CHUNK, name
            rc, out = dec(stream, expected.size)
            assert rc == 0 and np.array_equal(out, expected), f"{fmt} {name}: the CPU oracle does not read the hand-built stream"
            ref.append(out)
        bad = corrupt_chunk(cls, np.random.RandomState(5))
        rc, _ = dec(bad, MAX_CHUNK)
        assert rc != 0, f"{fmt}: the CPU oracle accepts the corrupt stream"
        _cache[fmt] = ([c[0] for c in cases], [c[1] for c in cases], ref, bad)
    return _cache[fmt]


def window_backend(backend):
    """The persistent one-wave-per-chunk kernel: forced on the emulator, chosen by the batch size on the card."""
    if backend.name == "emu":
        from conftest import emu_path_library

        backend.lib = emu_path_library("chase")
    return backend


def residues(sizes):
    """Start offsets modulo 16 of chunks packed tight (nvcomp_amd.batched._layout with align = 1)."""
    return set((np.concatenate([[0], np.cumsum(sizes)[:-1]]) % 16).tolist())


@pytest.mark.parametrize("fmt", ["LZ4", "Snappy"])
def test_window_lane_paths(backend, oracle, fmt):
    names, streams, ref, bad = cases_for(fmt, oracle)
    b = window_backend(backend)
    n = GPU_BATCH if b.name == "gpu" else len(streams) + 1
    # the corrupt stream once, in the middle of the valid ones (which are repeated to fill the card's batch)
    order = [i % len(streams) for i in range(n - 1)]
    bad_at = len(streams) // 2
    comp = [streams[i] for i in order[:bad_at]] + [bad] + [streams[i] for i in order[bad_at:]]
    want = [ref[i] for i in order[:bad_at]] + [None] + [ref[i] for i in order[bad_at:]]
    caps = [w.size if w is not None else MAX_CHUNK for w in want]  # exact capacities: the last 32 bytes are the chunk's own
    # chunks and output slots (capacity + 32 guard bytes) are packed tight: every alignment of both occurs
    assert residues([c.size for c in comp]) == set(range(16)), "input alignments"
    assert residues([c + 32 for c in caps]) == set(range(16)), "output alignments"
    outs, actual, status = b.codec(fmt).decompress(comp, caps)  # asserts the guard pattern behind every slot
    for i, w in enumerate(want):
        if w is None:
            assert status[i] != NvcompStatus.Success and actual[i] == 0, f"{fmt}: the corrupt stream"
            continue
        name = names[order[i if i < bad_at else i - 1]]
        assert status[i] == NvcompStatus.Success, f"{fmt} chunk {i} ({name}): status {status[i]}"
        assert actual[i] == w.size, f"{fmt} chunk {i} ({name}): size"
        assert np.array_equal(outs[i], w), f"{fmt} chunk {i} ({name}): bytes"


@pytest.mark.parametrize("fmt", ["LZ4", "Snappy"])
def test_far_batch_at_every_input_alignment(backend, oracle, fmt):
    """The chunk whose second batch is 64 far matches of every length, one with a source at the flushed boundary and one of
    the literal chunks, with both slabs moved byte by byte (the emulator: all sixteen shifts; the card, whose batch in
    test_window_lane_paths already holds every alignment, three)."""
    names, streams, ref, _ = cases_for(fmt, oracle)
    b = window_backend(backend)
    pick = [names.index("far_all"), names.index("far_end_%d" % PREFIX_BYTES), names.index("literals_3")]
    reps = 1366 if b.name == "gpu" else 2  # the card: 4 098 chunks per call
    comp = [streams[i] for i in pick] * reps
    want = [ref[i] for i in pick] * reps
    codec = b.codec(fmt)
    for shift in ((0, 5, 11) if b.name == "gpu" else range(16)):
        outs, actual, status = codec.decompress(comp, [w.size for w in want], base_misalign=shift)
        assert (status == NvcompStatus.Success).all(), f"{fmt} shift {shift}"
        assert all(np.array_equal(o, w) for o, w in zip(outs, want)), f"{fmt} shift {shift}"
