"""The window executor's lane predicates and its destination-aligned far data (common/lz_window.hip.h:
execute_window_batch; common/lz_copy.hip.h: far_store_aligned, steps_for) on hand-built streams.

The executor takes every lane predicate of a batch from a scalar mask, and loads a far match -- one whose source only
the output buffer holds -- at `source - (destination & 3)`, so that the loaded dwords are the window's aligned dwords. What
can go wrong with that is a matter of a few bytes: the head and the tail of a match at some alignment, a length class that
picks the wrong number of copy steps, a source in the chunk's first three bytes (the load would start in front of the
buffer) or its last 32. So the blocks below are written sequence by sequence: every length at every alignment of source
and destination, with and without literals in front, at the chunk's edges, and the near-match rounds and literal runs of
every length class that the same masks steer.

Expected bytes are the CPU decoder's, and before any kernel is judged they must equal a plain Python expansion of the
same sequences: a wrong hand-built block fails as the block. Every chunk is decoded with its exact size as capacity
(BatchedCodec.decompress puts a guard pattern behind it), through every decode path (`lz_path`)."""
import itertools
import zlib

import numpy as np
import pytest

from nvcomp_amd._lib import NvcompStatus

PREFIX = 4096  # a literal run of this length is written straight to the output buffer: the window restarts behind it
MAX_CHUNK = 32768


# ---- the two formats, from one list of sequences (literal bytes, offset, match length) + the last literals -----------

def _lz4_block(seqs, tail, spans=None):
    """Hand-built LZ4 block: seqs = [(literal bytes, offset, match length >= 4)], tail = the final literal-only sequence.
    spans, if given, receives (first, last) stream offsets of every sequence's literals."""
    out = bytearray()

    def lens(n):
        b = bytearray()
        while n >= 255:
            b.append(255)
            n -= 255
        b.append(n)
        return b

    for lit, off, mlen in seqs:
        ll, ml = len(lit), mlen - 4
        out.append((min(ll, 15) << 4) | min(ml, 15))
        if ll >= 15:
            out += lens(ll - 15)
        if spans is not None:
            spans.append((len(out), len(out) + ll - 1))
        out += lit
        out += bytes([off & 255, off >> 8])
        if ml >= 15:
            out += lens(ml - 15)
    ll = len(tail)
    out.append(min(ll, 15) << 4)
    if ll >= 15:
        out += lens(ll - 15)
    out += tail
    return np.frombuffer(bytes(out), dtype=np.uint8)


def _snappy_block(seqs, tail, spans=None):
    """The same sequences as Snappy elements: a literal element (if any), then a copy -- with a one-byte offset where the
    format has one (4..11 bytes from less than 2 KiB back) for every other such copy, with a two-byte offset otherwise."""
    out, at = bytearray(), []

    def literal(lit):
        n = len(lit) - 1
        if n < 0:
            return
        if n < 60:
            out.append(n << 2)
        elif n < 256:
            out.extend([60 << 2, n])
        else:
            out.extend([61 << 2, n & 255, n >> 8])
        at.append((len(out), len(out) + n))
        out.extend(lit)

    for i, (lit, off, mlen) in enumerate(seqs):
        assert 1 <= mlen <= 64
        literal(lit)
        if 4 <= mlen <= 11 and off < 2048 and i % 2:
            out.extend([1 | ((mlen - 4) << 2) | ((off >> 8) << 5), off & 255])
        else:
            out.extend([2 | ((mlen - 1) << 2), off & 255, off >> 8])
    literal(tail)
    n, pre = sum(len(lit) + m for lit, _, m in seqs) + len(tail), bytearray()
    while n >= 128:
        pre.append((n & 127) | 128)
        n >>= 7
    pre.append(n)
    if spans is not None:
        spans += [(a + len(pre), b + len(pre)) for a, b in at]
    return np.frombuffer(bytes(pre + out), dtype=np.uint8)


def _expand(seqs, tail):
    """What the sequences mean, byte by byte."""
    out = bytearray()
    for lit, off, mlen in seqs:
        out += lit
        assert 1 <= off <= len(out)
        for _ in range(mlen):
            out.append(out[-off])
    out += tail
    return np.frombuffer(bytes(out), dtype=np.uint8)


class Plan:
    """Sequences in the making, and the output position they have reached."""

    def __init__(self, seed):
        self.rng, self.seqs, self.pos = np.random.RandomState(seed), [], 0

    def add(self, lit, off, mlen):
        assert 1 <= off <= self.pos + len(lit) and off < 65536
        self.seqs.append((bytes(lit), int(off), int(mlen)))
        self.pos += len(lit) + mlen

    def copy_from(self, lit, src, mlen):
        """lit, then a match whose source starts at output position src"""
        self.add(lit, self.pos + len(lit) - src, mlen)

    def prefix(self):
        """4 KiB of incompressible literals: flushed, and behind the window, for everything that follows"""
        self.add(self.rng.bytes(PREFIX), 8, 4)

    def align_to(self, residue, src):
        """a filler match (from src) that brings the output position to `residue` modulo 4"""
        need = (residue - self.pos) & 3
        if need:
            self.copy_from(b"", src, 4 + need)

    def done(self, tail=12):
        return self.seqs, self.rng.bytes(tail)


# ---- the cases ---------------------------------------------------------------------------------------------------

def far_matches(lengths, literals_in_front, seed):
    """Every length at every destination and source residue modulo 4, the sources spread over the prefix."""
    p = Plan(seed)
    p.prefix()
    for i, (mlen, da, sa) in enumerate(itertools.product(lengths, range(4), range(4))):
        nlit = i % 4 if literals_in_front else 0
        p.align_to((da - nlit) & 3, 64 + (i * 7) % 1000)
        assert (p.pos + nlit) & 3 == da
        p.copy_from(p.rng.bytes(nlit), 16 + 4 * ((i * 13) % 900) + sa, mlen)
    return p.done()


def far_chunk_edges(seed):
    """Sources at the chunk's positions 0, 1, 2 and 3: a load at source - (destination & 3) would start in front of the buffer."""
    p = Plan(seed)
    p.prefix()
    for i, (mlen, da, src) in enumerate(itertools.product((4, 5, 7, 8, 9, 16, 17, 31, 32), range(4), range(4))):
        nlit = i % 2
        p.align_to((da - nlit) & 3, 200 + i)
        p.copy_from(p.rng.bytes(nlit), src, mlen)
    return p.done()


def far_tight_capacity(seed, src_back, mlen, tail):
    """The prefix leaves the flushed mark exactly at its end, P. One literal, then a match whose source starts src_back
    bytes in front of P. With 12 last literals and a source 8 .. 10 bytes in front of P the source lies in the last 32
    bytes of the (exact) capacity; with src_back = mlen it ends exactly at the flushed mark, with mlen - 1 one byte behind it."""
    p = Plan(seed)
    p.prefix()
    mark = p.pos
    p.copy_from(p.rng.bytes(1), mark - src_back, mlen)
    for j in range(3 if tail > 12 else 0):  # a little company in the batch
        p.copy_from(p.rng.bytes(j), 100 + 5 * j, 6 + j)
    return p.done(tail)


def near_matches(seed):
    """Short offsets into what the same batch has just produced: chains of dependent matches. Three stretches of 192
    sequences -- whole batches of each kind: lengths 4..8 only (rounds of 2 steps), 9..16 only (4 steps), and 4..8 with
    one match of 17..32 in every twenty (a round takes 8 steps for the one lane that needs them)."""
    p = Plan(seed)
    r = p.rng
    p.add(r.bytes(48), 5, 4)
    for kind in range(3):
        for j in range(192):
            lo, hi = ((4, 8), (9, 16), (4, 8))[kind]
            mlen = int(r.randint(17, 33)) if kind == 2 and j % 20 == 7 else int(r.randint(lo, hi + 1))
            lit = r.bytes(int(r.randint(0, 2)))
            p.add(lit, int(r.randint(4, 41)), mlen)
    return p.done()


def chain_depths(seqs, horizon=32):
    """For every sequence: the length of the chain of matches it ends, counting only sources that one of the `horizon`
    sequences in front of it produced (a batch is 64 sequences at most: such chains lie inside one batch for most of them)."""
    producer, depth = [], []
    for k, (lit, off, mlen) in enumerate(seqs):
        producer += [-1] * len(lit)
        start = len(producer) - off
        src = set(producer[start: start + min(mlen, off)])
        depth.append(1 + max([depth[j] for j in src if j >= 0 and j >= k - horizon] + [0]))
        producer += [k] * mlen
    return depth


def literal_runs(seed):
    """Runs of 0 .. 33 bytes at every destination residue, in an order that mixes the classes (none, 1..3 bytes: byte by
    byte; 4..32: a lane's dword steps, 2, 4 or 8 of them; 33: the whole wave) within every batch."""
    p = Plan(seed)
    p.add(p.rng.bytes(9), 9, 4)
    items = list(itertools.product(range(34), range(4)))
    p.rng.shuffle(items)
    for i, (n, da) in enumerate(items):
        p.align_to(da, p.pos - 4 - i % 7)
        p.add(p.rng.bytes(n), 4 + i % 9, 4 + i % 3)
    return p.done()


def ring_wrap(seed, phase, run):
    """Literal runs of `run` bytes back to back, through the end of the 2 KiB input ring"""
    p = Plan(seed)
    p.add(p.rng.bytes(4 + phase), 4, 4)
    while p.pos < 3000:
        p.add(p.rng.bytes(run), run, 4)
    return p.done(6)


LZ4_LENGTHS = list(range(4, 33))
SNAPPY_LENGTHS = list(range(4, 33)) + [33, 40, 48, 63, 64]  # above 32 the whole wave copies the match


def build_cases(fmt):
    lengths = LZ4_LENGTHS if fmt == "LZ4" else SNAPPY_LENGTHS
    cases = {"far": [far_matches(lengths, False, 1)],
             "far_literals": [far_matches(lengths, True, 2)],
             "far_edges": [far_chunk_edges(3)],
             "far_tight": [far_tight_capacity(10 + b, b, 8, 12) for b in (8, 9, 10)]
                          + [far_tight_capacity(20 + m + d, m - d, m, 60) for m in (4, 9, 17, 32) for d in (0, 1)],
             "near": [near_matches(4)],
             "literals": [literal_runs(5)] + [ring_wrap(30 + ph, ph, run) for ph, run in ((0, 32), (7, 32), (13, 17), (22, 32), (31, 24))]}
    return cases


_cache = {}


def cases_for(fmt, oracle):
    """name -> (streams, expected outputs): built, and checked against the Python expansion, once per format."""
    if fmt not in _cache:
        block = _lz4_block if fmt == "LZ4" else _snappy_block
        if fmt == "LZ4":
            dec = oracle.lz4_decompress
        else:  # libsnappy where the reference-side shim exists
            dec = oracle.ref_snappy_decompress if oracle.have_ref() else oracle.snappy_decompress
        built = {}
        for name, chunks in build_cases(fmt).items():
            streams, want = [], []
            for seqs, tail in chunks:
                stream, plain = block(seqs, tail), _expand(seqs, tail)
                assert plain.size <= MAX_CHUNK and stream.size <= MAX_CHUNK, name
                rc, out = dec(stream, plain.size)
                assert rc == 0 and np.array_equal(out, plain), f"{fmt} {name}: the CPU decoder does not read the hand-built block as written"
                streams.append(stream)
                want.append(out)
            built[name] = (streams, want, chunks)
        _cache[fmt] = built
    return _cache[fmt]


def check(backend, fmt, streams, want, what):
    codec = backend.codec(fmt)
    for mis in (0, 3):
        outs, actual, status = codec.decompress(streams, [w.size for w in want], base_misalign=mis)
        assert (status == NvcompStatus.Success).all(), f"{fmt} {what}, shift {mis}: statuses {status}"
        assert actual.tolist() == [w.size for w in want], f"{fmt} {what}, shift {mis}: sizes"
        for i, (o, w) in enumerate(zip(outs, want)):
            if not np.array_equal(o, w):
                at = int(np.flatnonzero(o != w)[0])
                raise AssertionError(f"{fmt} {what}, shift {mis}: chunk {i} differs from byte {at} on "
                                     f"(got {o[at: at + 8].tolist()}, want {w[at: at + 8].tolist()})")


FORMATS = ["LZ4", "Snappy"]


@pytest.mark.parametrize("fmt", FORMATS)
def test_far_matches(backend, lz_path, oracle, fmt):
    """Every length 4..32 (Snappy: and copies up to 64 bytes) at every destination & 3 and source & 3, from the prefix."""
    streams, want, chunks = cases_for(fmt, oracle)["far"]
    assert all(not lit for lit, _, _ in chunks[0][0][1:]), "no literals in front of these matches"
    check(backend, fmt, streams, want, "far matches")


@pytest.mark.parametrize("fmt", FORMATS)
def test_far_matches_literals_in_front(backend, lz_path, oracle, fmt):
    """The same with 0..3 literals in front of each match (Snappy: literal and copy are one sequence)."""
    streams, want, chunks = cases_for(fmt, oracle)["far_literals"]
    assert {len(lit) for lit, _, _ in chunks[0][0][1:]} == {0, 1, 2, 3}
    check(backend, fmt, streams, want, "far matches behind literals")


@pytest.mark.parametrize("fmt", FORMATS)
def test_far_matches_chunk_edges(backend, lz_path, oracle, fmt):
    """Sources at the chunk's positions 0, 1, 2 and 3."""
    streams, want, chunks = cases_for(fmt, oracle)["far_edges"]
    pos, sources = 0, set()
    for lit, off, mlen in chunks[0][0]:
        sources.add(pos + len(lit) - off)
        pos += len(lit) + mlen
    assert {0, 1, 2, 3} <= sources
    check(backend, fmt, streams, want, "far matches from the chunk's first bytes")


@pytest.mark.parametrize("fmt", FORMATS)
def test_far_matches_tight_capacity(backend, lz_path, oracle, fmt):
    """Exact capacities: a source inside the buffer's last 32 bytes, one that ends exactly at the flushed mark, one that
    ends a byte behind it."""
    streams, want, chunks = cases_for(fmt, oracle)["far_tight"]
    mark = PREFIX + 4
    for (seqs, tail), w in zip(chunks[:3], want[:3]):
        src = mark + 1 - seqs[1][1]
        assert w.size - 32 < src and src + seqs[1][2] <= mark, "the source lies in the last 32 bytes and is flushed"
    ends = [mark + 1 - seqs[1][1] + seqs[1][2] - mark for seqs, _ in chunks[3:]]
    assert sorted(set(ends)) == [0, 1], "sources that end at the flushed mark, and one byte behind it"
    check(backend, fmt, streams, want, "far matches, tight capacity")


@pytest.mark.parametrize("fmt", FORMATS)
def test_near_matches(backend, lz_path, oracle, fmt):
    """Chains of dependent matches inside a batch, offsets 4..40, rounds of 2, 4 and 8 copy steps."""
    streams, want, chunks = cases_for(fmt, oracle)["near"]
    seqs = chunks[0][0]
    depth = chain_depths(seqs)
    for kind in range(3):  # chains four deep in each stretch, many times
        assert sum(d >= 4 for d in depth[1 + 192 * kind: 1 + 192 * (kind + 1)]) >= 10, kind
    assert {off for _, off, _ in seqs[1:]} == set(range(4, 41))
    assert all(m <= 8 for _, _, m in seqs[1:193]) and all(9 <= m <= 16 for _, _, m in seqs[193:385])
    late = [m for _, _, m in seqs[385:]]
    assert sum(m >= 17 for m in late) >= 8 and all(m <= 8 or m >= 17 for m in late)
    check(backend, fmt, streams, want, "near matches")


@pytest.mark.parametrize("fmt", FORMATS)
def test_literal_runs(backend, lz_path, oracle, fmt):
    """Runs of 0..33 bytes at every destination residue, the classes mixed within a batch; runs through the ring's wrap."""
    streams, want, chunks = cases_for(fmt, oracle)["literals"]
    seqs = chunks[0][0]
    pos, seen = 0, set()
    for lit, _, mlen in seqs:
        seen.add((len(lit), pos & 3))
        pos += len(lit) + mlen
    assert set(itertools.product(range(34), range(4))) <= seen
    for k in range(1, len(seqs) - 64, 64):  # every stretch of 64 sequences has runs of 1..3 and of 4..32 bytes
        sizes = {len(lit) for lit, _, _ in seqs[k: k + 64]}
        assert sizes & {1, 2, 3} and sizes & set(range(4, 33))
    # the ring's coordinates start at the stream's address modulo 16: whatever that is, a run of one of the chunks crosses 2 KiB
    block = _lz4_block if fmt == "LZ4" else _snappy_block
    crossed = set()
    for (wseqs, wtail), stream in zip(chunks[1:], streams[1:]):
        spans = []
        assert np.array_equal(block(wseqs, wtail, spans), stream)
        crossed |= {a for first, last in spans for a in range(16) if 4 <= last - first + 1 <= 32 and first < 2048 - a <= last}
    assert crossed == set(range(16))
    check(backend, fmt, streams, want, "literal runs")


# ---- DEFLATE: the same executor with matches of three bytes ----------------------------------------------------------

def inflate_matches(data):
    """(length, distance) of every match of a raw DEFLATE stream, and the bytes it decodes to: a plain Python inflater."""
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((data[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    def table(lengths):
        codes, code = {}, 0
        for n in range(1, 16):
            for sym, l in enumerate(lengths):
                if l == n:
                    codes[(n, code)] = sym
                    code += 1
            code <<= 1
        return codes

    def symbol(codes):
        code = 0
        for n in range(1, 16):
            code = (code << 1) | bits(1)
            if (n, code) in codes:
                return codes[(n, code)]
        raise ValueError("bad code")

    lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    lext = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dbase = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
    dext = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
    out, matches, final = bytearray(), [], 0
    while not final:
        final, btype = bits(1), bits(2)
        if btype == 0:
            pos = (pos + 7) & ~7
            n = bits(16)
            bits(16)
            out += bytes(data[pos >> 3: (pos >> 3) + n])
            pos += 8 * n
            continue
        if btype == 1:
            ll, dd = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 30)
        else:
            hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
            cl = [0] * 19
            for i in range(hclen):
                cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = bits(3)
            clt, lens = table(cl), []
            while len(lens) < hlit + hdist:
                s = symbol(clt)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + bits(2))
                else:
                    lens += [0] * (3 + bits(3) if s == 17 else 11 + bits(7))
            ll, dd = table(lens[:hlit]), table(lens[hlit:])
        while True:
            s = symbol(ll)
            if s < 256:
                out.append(s)
            elif s == 256:
                break
            else:
                length = lbase[s - 257] + bits(lext[s - 257])
                d = symbol(dd)
                dist = dbase[d] + bits(dext[d])
                matches.append((length, dist))
                for _ in range(length):
                    out.append(out[-dist])
    return matches, bytes(out)


def test_deflate_three_byte_far_matches(backend):
    """DEFLATE's matches of three bytes go through the same far store. Compressible text at level 9 is the stream the
    issue names; zlib's lazy matcher (levels 4-9) drops a three-byte match further back than 4 KiB (TOO_FAR, deflate.c),
    its fast matcher (levels 1-3) keeps it: the case holds both streams of the same text, and asserts by the Python
    inflater above that three-byte matches from beyond 4 KiB -- far behind the 2 KiB window -- are among them."""
    from nvcomp_amd import datasets

    text = datasets.text(MAX_CHUNK, 3).tobytes()
    comp, far3 = [], 0
    for level in (9, 1):
        o = zlib.compressobj(level, zlib.DEFLATED, -15)
        stream = o.compress(text) + o.flush()
        matches, plain = inflate_matches(stream)
        assert plain == text, "the Python inflater reads zlib's stream"
        far3 += sum(1 for length, dist in matches if length == 3 and dist > 4096)
        comp.append(np.frombuffer(stream, dtype=np.uint8))
    assert far3 >= 10, f"three-byte matches from beyond 4 KiB: {far3}"
    want = np.frombuffer(text, dtype=np.uint8)
    codec = backend.codec("Deflate")
    for mis in (0, 3):
        outs, actual, status = codec.decompress(comp, [want.size] * len(comp), base_misalign=mis)
        assert (status == NvcompStatus.Success).all() and actual.tolist() == [want.size] * len(comp)
        assert all(np.array_equal(o, want) for o in outs)
