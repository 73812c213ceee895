"""Cascaded and Bitcomp at every packed bit width and at both ends of the element range.

The kernels of both codecs pick their code path by the width of a packed stream (cascaded/cascaded.hip.h: pack_stream,
unpack_stream, stream_range and their special cases at 32 and 64 bits; bitcomp/bitcomp.hip.h: a row's width byte). The
other tests meet whatever widths their datasets happen to give, never a value with the top bit set, never a negative
value next to a positive one. Here the inputs are BUILT for a width and a place in the range, the expected `bits` and
`min` of every stream are computed in Python ints (tests/cascaded_stream.py reads and writes the container on its own),
and the coverage -- every width seen, packed, with the intended header -- is asserted. Everything the round-trip helpers
of test_cascaded.py / test_bitcomp.py assert is asserted here too (they are restated below only to hand the streams back).
"""
import struct

import numpy as np
import pytest

import cascaded_stream as cs
from nvcomp_amd._lib import NvcompStatus

WIDTH = cs.WIDTH
DT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
SUB = 4096


def is_signed(typ):
    return typ % 2 == 0


# ---- the round trips of test_cascaded.py / test_bitcomp.py, every assertion kept; they return the compressed chunks ----

def casc_roundtrip(backend, oracle, chunks, opts):
    sub, typ, r, d, bp = opts
    codec = backend.codec("Cascaded", opts)
    comp = codec.compress(chunks, in_align=8)
    for i, (cc, c) in enumerate(zip(comp, chunks)):
        ref = oracle.cascaded_compress(c, sub, typ, r, d, bp)
        assert cc.size == ref.size and np.array_equal(cc, ref), f"chunk {i}: compressed bytes differ from the CPU model"
        rc, out = oracle.cascaded_decompress(cc, c.size)
        assert rc == 0 and np.array_equal(out, c), f"chunk {i}: the CPU model does not invert the stream"
    outs, actual, status = codec.decompress(comp, [c.size for c in chunks], comp_align=8, out_align=8)
    assert (status == NvcompStatus.Success).all(), status
    assert actual.tolist() == [c.size for c in chunks]
    for i, (o, c) in enumerate(zip(outs, chunks)):
        assert np.array_equal(o, c), f"chunk {i}: the decoder does not invert the stream"
    sizes = codec.get_decompress_size(comp, comp_align=8)
    assert sizes.tolist() == [c.size for c in chunks]
    return comp


def bitcomp_roundtrip(backend, oracle, chunks, algo, typ):
    codec = backend.codec("Bitcomp", (algo, typ))
    comp = codec.compress(chunks, in_align=8)
    for i, (cc, c) in enumerate(zip(comp, chunks)):
        ref = oracle.bitcomp_compress(c, algo, WIDTH[typ])
        assert cc.size == ref.size and np.array_equal(cc, ref), f"chunk {i}: compressed bytes differ from the CPU model"
        rc, out = oracle.bitcomp_decompress(cc, c.size)
        assert rc == 0 and np.array_equal(out, c), f"chunk {i}: the CPU model does not invert the stream"
    outs, actual, status = codec.decompress(comp, [c.size for c in chunks], comp_align=8, out_align=8)
    assert (status == NvcompStatus.Success).all(), status
    assert actual.tolist() == [c.size for c in chunks]
    for i, (o, c) in enumerate(zip(outs, chunks)):
        assert np.array_equal(o, c), f"chunk {i}: the decoder does not invert the stream"
    sizes = codec.get_decompress_size(comp, comp_align=8)
    assert sizes.tolist() == [c.size for c in chunks]
    outs2, actual2, _ = codec.decompress(comp, [c.size for c in chunks], checked=False, comp_align=8, out_align=8)
    assert actual2.tolist() == [c.size for c in chunks]
    for i, (o, c) in enumerate(zip(outs2, chunks)):
        assert np.array_equal(o, c), f"chunk {i}: the status-less decoder does not invert the stream"
    return comp


# ---- inputs ----

def random_below(rng, n, b):
    """n uint64 uniform in [0, 2^b), 0 <= b <= 64."""
    if b == 0:
        return np.zeros(n, dtype=np.uint64)
    return np.frombuffer(rng.bytes(8 * n), dtype=np.uint64) >> np.uint64(64 - b)


def in_range(rng, n, w, base, b, lo_at, hi_at):
    """n elements of w bytes, uniform in [base, base + 2^b - 1] mod 2^(8 w), both endpoints planted."""
    off = random_below(rng, n, b).copy()
    off[lo_at] = 0
    off[hi_at] = (1 << b) - 1
    with np.errstate(over="ignore"):
        return (off + np.uint64(base % (1 << 64))).astype(DT[w])


def straddling_base(typ, b):
    """A range of 2^b values around zero (signed types) or around 2^(8 w - 1) (unsigned types); 0 at full width."""
    w = WIDTH[typ]
    if b >= 8 * w:
        return 0
    mid = 0 if is_signed(typ) else 1 << (8 * w - 1)
    return (mid - (1 << b) // 2) % (1 << (8 * w))


# ---- the expectation, in Python ints ----

def bits_and_min(vals, w, as_signed):
    """(bits, min) of a stream of w-byte values (ints in [0, 2^(8 w))) ranged in signed or unsigned order."""
    half, mod = 1 << (8 * w - 1), 1 << (8 * w)
    keys = [v - mod if as_signed and v >= half else v for v in vals]
    lo, hi = min(keys), max(keys)
    return (hi - lo).bit_length(), lo % mod


def model_sub_chunk(vals, typ, r, d):
    """The streams of one sub-chunk as doc/cascaded_overview.md describes the scheme: RLE and delta layers interleaved, the
    RLE values feeding the next layer, a layer that takes out fewer than one element in eight left out (all runs 1).
    Returns ([(bits, min, count) for runs[0 .. r-1] and the values], the values' list, the sub-chunk's packed size)."""
    w = WIDTH[typ]
    mod = 1 << (8 * w)
    c = list(vals)
    heads = []
    for l in range(max(r, d)):
        if l < r:
            starts = [i for i in range(len(c)) if i == 0 or c[i] != c[i - 1]]
            if len(starts) + (len(c) >> 3) > len(c):
                heads.append((0, 1, len(c)))
            else:
                runs = [e - s for s, e in zip(starts, starts[1:] + [len(c)])]
                heads.append(((max(runs) - min(runs)).bit_length(), min(runs), len(runs)))
                c = [c[s] for s in starts]
        if l < d:
            c = c[:1] + [(c[i] - c[i - 1]) % mod for i in range(1, len(c))]
    heads.append(bits_and_min(c, w, d > 0 or is_signed(typ)) + (len(c),))
    size = 4 + 4 * r + sum(12 + 4 * ((cnt * bits + 31) // 32) for bits, _, cnt in heads)
    return heads, c, size


def check_chunk(comp, chunk, opts):
    """Parse a compressed chunk on our own and hold every sub-chunk against the Python-int model: raw exactly when the
    cascade is not smaller than 4 + round_up_4(bytes); otherwise the counts, every stream's bits / min and the value
    stream's elements as modelled. Returns [(parsed sub-chunk, modelled headers)]."""
    sub_bytes, typ, r, d, _ = opts
    w = WIDTH[typ]
    subs = cs.parse(comp)
    assert len(subs) == (chunk.size + sub_bytes - 1) // sub_bytes
    out = []
    for s, sub in enumerate(subs):
        raw = chunk[s * sub_bytes: (s + 1) * sub_bytes].tobytes()
        heads, vals, size = model_sub_chunk(cs.elements(raw, w), typ, r, d)
        raw_size = 4 + (len(raw) + 3) // 4 * 4
        if size >= raw_size:
            assert sub.raw is not None, f"sub-chunk {s}: packed, but {size} >= {raw_size} bytes"
            assert sub.raw == raw
        else:
            assert sub.raw is None, f"sub-chunk {s}: raw, but the cascade takes {size} < {raw_size} bytes"
            assert sub.bytes == size
            assert [(st.bits, st.min, st.count) for st in sub.streams] == heads, f"sub-chunk {s}"
            assert sub.count == [cnt for _, _, cnt in heads[:-1]]
            assert cs.unpack(sub.values, w) == vals, f"sub-chunk {s}: value stream"
        out.append((sub, heads))
    return out


# ---- 1. Cascaded, every width, plain packing ----

def plain_bases(typ, b):
    w = WIDTH[typ]
    top = 1 << (8 * w)
    if is_signed(typ):  # INT_MIN; INT_MAX - (2^b - 1); around zero
        return [top // 2, (top // 2 - (1 << b)) % top, straddling_base(typ, b)]
    return [0, top - (1 << b), straddling_base(typ, b)]  # 0; up to UINT_MAX; around 2^(8 w - 1)


@pytest.mark.parametrize("typ", range(8))
def test_cascaded_every_width_plain(backend, oracle, typ):
    """One sub-chunk of 4096 / w elements per (width, base), uniform over exactly 2^b values with both ends planted away
    from the first and the last element; every b in 0 .. 8 w - 1 (8 w bits never shrink a sub-chunk without an RLE layer:
    test_cascaded_full_width). The stream must be packed with bits == b and min == the planted minimum: pack_stream's
    three shapes and its bits == 0 exit, stream_range's sign extension and key flip at both ends of the range, and on
    the way back every width of unpack_stream's two paths."""
    w = WIDTH[typ]
    n = SUB // w
    rng = np.random.RandomState(1000 + typ)
    opts = (SUB, typ, 0, 0, 1)
    cases = [(b, base) for b in range(8 * w) for base in plain_bases(typ, b)]
    chunks = [in_range(rng, n, w, base, b, 5, n - 7).view(np.uint8) for b, base in cases]
    comp = casc_roundtrip(backend, oracle, chunks, opts)
    seen = set()
    for (b, base), cc, c in zip(cases, comp, chunks):
        (sub, heads), = check_chunk(cc, c, opts)
        assert sub.raw is None, f"type {typ}, {b} bits at {base:#x}: not packed"
        assert (sub.values.bits, sub.values.min, sub.values.count) == (b, base, n), f"type {typ}, {b} bits at {base:#x}"
        seen.add(b)
    assert seen == set(range(8 * w))


# ---- 2. Cascaded, full width ----

@pytest.mark.parametrize("typ", range(8))
def test_cascaded_full_width(backend, oracle, typ):
    """bits == 8 w shrinks a sub-chunk only behind an RLE layer: full-range values, the type's two extremes first, every
    value eight times. The value stream is packed with 8 w bits -- the masks that would be a shift by the full width."""
    w = WIDTH[typ]
    n = SUB // w
    rng = np.random.RandomState(2000 + typ)
    vals = np.frombuffer(rng.bytes(n // 8 * w), dtype=DT[w]).copy()
    lo, hi = ((1 << (8 * w - 1)), (1 << (8 * w - 1)) - 1) if is_signed(typ) else (0, (1 << (8 * w)) - 1)
    vals[0], vals[1] = lo, hi
    chunk = np.repeat(vals, 8).view(np.uint8)
    opts = (SUB, typ, 1, 0, 1)
    comp, = casc_roundtrip(backend, oracle, [chunk], opts)
    (sub, heads), = check_chunk(comp, chunk, opts)
    assert sub.raw is None
    assert sub.values.bits == 8 * w and sub.values.min == lo
    assert sub.values.count == sub.count[0] <= n // 8


# ---- 3. Cascaded, element counts at the unpack's tile edges ----

TILE_COUNTS = [63, 64, 65, 255, 256, 257, 511, 512, 513]


@pytest.mark.parametrize("typ", range(8))
def test_cascaded_counts_at_tile_edges(backend, oracle, typ):
    """The unpack handles 8 (elements of up to 4 bytes, up to 32 bits) or 4 tiles of 64 elements a step and clamps the lanes
    beyond the count: counts on either side of a tile, of four and of eight tiles, and one element short of a sub-chunk,
    each as the short last sub-chunk behind a whole one, at the widths on either side of every path boundary (the widths
    an element of this type can have; 8 w bits included, which must go raw). Packed or raw is decided by the size rule
    (the cascade must be smaller than 4 + round_up_4(bytes)), computed here."""
    w = WIDTH[typ]
    n = SUB // w
    rng = np.random.RandomState(3000 + typ)
    widths = sorted({b for b in (1, 16, 17, 31, 32, 8 * w - 1) + ((33, 47, 63) if w == 8 else ()) if b <= 8 * w})
    opts = (SUB, typ, 0, 0, 1)
    cases = [(count, b) for count in TILE_COUNTS + [n - 1] for b in widths]
    chunks = []
    for count, b in cases:
        base = straddling_base(typ, b)
        whole = in_range(rng, n, w, base, min(b, 8 * w - 1), 9, n - 2)
        short = in_range(rng, count, w, base, b, count - 2, 1)
        chunks.append(np.concatenate([whole, short]).view(np.uint8))
    comp = casc_roundtrip(backend, oracle, chunks, opts)
    packed = {}
    for (count, b), cc, c in zip(cases, comp, chunks):
        (first, _), (last, heads) = check_chunk(cc, c, opts)[:2]  # (8-byte types: 513 elements are a whole sub-chunk and one)
        assert first.raw is None
        assert last.n_elems == min(count, n)
        count = min(count, n)
        if last.raw is None:
            assert heads[-1][0] == b and last.values.bits == b
            packed.setdefault(count, []).append(b)
        else:
            assert 16 + 4 * ((count * b + 31) // 32) >= 4 + (count * w + 3) // 4 * 4
    counts = {min(count, n) for count, _ in cases}
    assert all(packed.get(count) for count in counts), packed
    if w == 8:  # the three-word straddle (sh + bits > 64) at every count; by the size rule 63 bits shrink 255 elements, not 65
        assert all({33, 47} <= set(packed[count]) for count in counts), packed
        assert all(63 in packed[count] for count in counts if count >= 255), packed


# ---- 4. Cascaded, delta layers that wrap ----

def wrapping_inputs(typ, rng):
    """[(name, values as uint64 mod 2^(8 w), b or None)]: a whole sub-chunk and 100 elements of a second one."""
    w = WIDTH[typ]
    n = SUB // w + 100
    top = 1 << (8 * w)
    mask = np.uint64(top - 1)
    lo, hi = (top // 2, top // 2 - 1) if is_signed(typ) else (0, top - 1)
    i = np.arange(n, dtype=np.uint64)
    out = [("sawtooth", np.where(i % 2 == 0, np.uint64(lo), np.uint64(hi)), None),
           ("half", np.where(i % 2 == 0, np.uint64(0), np.uint64(top // 2)), None)]
    with np.errstate(over="ignore"):
        # up across the wrap point and down again: 0 / 2^(8 w) for everyone, 2^(8 w - 1) for the signed order
        tri = np.minimum(i, np.uint64(n - 1) - i) * np.uint64(3)
        out.append(("walk over 2^(8w)", (np.uint64((top - n // 2) % (1 << 64)) + tri) & mask, None))
        out.append(("walk over 2^(8w-1)", (np.uint64((top // 2 - n // 2) % (1 << 64)) + tri) & mask, None))
        for b in (1, 2, 4 * w, 8 * w - 1):
            # deltas uniform in [-2^(b-1), 2^(b-1) - 1], both ends planted. The delta layer keeps the first value in the
            # stream it ranges; the first value is 0, inside every such range, so it widens nothing.
            delta = random_below(rng, n, b) - np.uint64(1 << (b - 1))
            delta[0] = 0
            delta[7] = np.uint64(0) - np.uint64(1 << (b - 1))
            delta[n - 120] = (1 << (b - 1)) - 1
            out.append((f"deltas of {b} bits", np.cumsum(delta, dtype=np.uint64) & mask, b))
    return out


@pytest.mark.parametrize("r,d", [(0, 1), (0, 2), (1, 1)])
@pytest.mark.parametrize("typ", [0, 1, 4, 5, 6, 7])
def test_cascaded_wrapping_deltas(backend, oracle, typ, r, d):
    """Deltas that wrap the element range in both directions: differences are taken and summed mod 2^(8 w), then ranged as
    SIGNED whatever the type. Every sub-chunk's packed / raw verdict, stream headers and value stream are held against the
    Python-int model; with one delta layer a walk built from b-bit deltas packs into exactly b bits."""
    w = WIDTH[typ]
    rng = np.random.RandomState(4000 + 100 * typ + 10 * r + d)
    opts = (SUB, typ, r, d, 1)
    inputs = wrapping_inputs(typ, rng)
    chunks = [v.astype(DT[w]).view(np.uint8) for _, v, _ in inputs]
    comp = casc_roundtrip(backend, oracle, chunks, opts)
    for (name, _, b), cc, c in zip(inputs, comp, chunks):
        subs = check_chunk(cc, c, opts)
        if b is not None and (r, d) == (0, 1):
            first, _ = subs[0]
            assert first.raw is None and first.values.bits == b, f"type {typ}, {name}"
            assert first.values.min == (-(1 << (b - 1))) % (1 << (8 * w))
    # the sawtooth's deltas are +-(2^(8 w) - 1) = -+1: with the first value 0 of an unsigned type kept, [-1, 1] takes two bits
    # (a signed type's first value is its minimum: 8 w bits, raw -- the model above has said so)
    if (r, d) == (0, 1) and not is_signed(typ):
        first, _ = check_chunk(comp[0], chunks[0], opts)[0]
        assert first.raw is None and first.values.bits == 2


# ---- 5. Cascaded, streams from another writer ----

FOREIGN = {1: 3, 3: 11, 4: 13, 5: 29, 7: 7}  # type -> b0, the bits its value set needs


def foreign_streams(typ):
    """[(what, chunk bytes, the elements as Python ints)] -- all legal: 300 elements in sub-chunks of 256."""
    w = WIDTH[typ]
    b0 = FOREIGN[typ]
    top = 1 << (8 * w)
    rng = np.random.RandomState(5000 + typ)
    n, sub = 300, 256 * w
    off = [int(x) for x in random_below(rng, n, b0)]
    off[3], off[250], off[258], off[297] = 0, (1 << b0) - 1, (1 << b0) - 1, 0
    garbage = (0xA5C3F00F5A3C0FF1 << (8 * w)) % (1 << 64)  # nonzero bits above the element width only
    out = []
    wrapping = top - (1 << (b0 - 1)) - 1  # min + x crosses 2^(8 w) inside every sub-chunk
    for base in (wrapping, 5):
        vals = [(base + x) % top for x in off]
        for bits in range(b0, 65) if base == wrapping else (b0, 32, 64):
            out.append((f"bits {bits}, min {base:#x}", cs.write_plain(vals, typ, bits, base, sub), vals))
            if w < 8:
                out.append((f"bits {bits}, min {base:#x} with high bits",
                            cs.write_plain(vals, typ, bits, base | garbage, sub, high=(1 << 64) - 1), vals))
    for const in (top - 1, 1):
        vals = [const] * n
        out.append((f"bits 0, min {const:#x}", cs.write_plain(vals, typ, 0, const, sub), vals))
        if w < 8:
            out.append((f"bits 0, min {const:#x} with high bits", cs.write_plain(vals, typ, 0, const | garbage, sub), vals))
    return out


@pytest.mark.parametrize("typ", sorted(FOREIGN))
def test_cascaded_streams_from_another_writer(backend, oracle, typ):
    """The decoder is driven by the stream alone. Legal streams our compressor never writes: bits above the minimum up to
    64 (beyond the element width for the narrow types: the generic unpack path with a 1- to 4-byte element), a min with
    bits above the element width, x with bits above the element width, min + x wrapping the element range, bits == 0
    with a nonzero min. Library decoder == CPU model == the Python-int reader. A stream header that says 65 bits is refused
    by both, nothing is reported as written and the bytes behind the output stay as they were."""
    w = WIDTH[typ]
    streams = foreign_streams(typ)
    for what, stream, vals in streams:  # the reader inverts the writer (neither knows the library)
        assert [v for sub in cs.parse(stream) for v in cs.unpack(sub.values, w)] == vals, what
    # 65 bits: once a well-formed stream with all the words 65 bits an element take (nothing but the width is wrong with
    # it), once written into the header of the second sub-chunk of a good stream (the first one decodes)
    good, vals = streams[0][1], streams[0][2]
    h = cs.header(good)
    bad_first = cs.write_plain(vals, typ, 65, 0, 256 * w)
    bad_second = bytearray(good)
    struct.pack_into("<I", bad_second, h.payload + h.sub_end[0] + 4, 65)
    comp = [np.frombuffer(s, dtype=np.uint8) for _, s, _ in streams]
    n_good = len(comp)
    comp[1:1] = [np.frombuffer(bytes(bad_first), dtype=np.uint8)]  # among the good ones, not behind them
    comp.append(np.frombuffer(bytes(bad_second), dtype=np.uint8))
    bad_at = (1, len(comp) - 1)
    caps = [300 * w] * len(comp)
    codec = backend.codec("Cascaded", (256 * w, typ, 0, 0, 1))
    outs, actual, status = codec.decompress(comp, caps, comp_align=8, out_align=8)  # guard bytes checked inside
    sizes = codec.get_decompress_size(comp, comp_align=8)
    expected = iter(streams)
    for i, cc in enumerate(comp):
        rc, ref = oracle.cascaded_decompress(cc, caps[i])
        if i in bad_at:
            assert rc != 0, f"chunk {i}: the CPU model reads a 65-bit stream"
            assert status[i] != NvcompStatus.Success and actual[i] == 0, f"chunk {i}: the decoder reads a 65-bit stream"
            continue
        what, _, vals = next(expected)
        want = cs.to_bytes(vals, w)
        assert rc == 0 and ref.tobytes() == want, f"type {typ}, {what}: CPU model"
        assert status[i] == NvcompStatus.Success and actual[i] == len(want), f"type {typ}, {what}: status {status[i]}"
        assert outs[i].tobytes() == want, f"type {typ}, {what}: decoder"
        assert sizes[i] == len(want)
    assert len(comp) == n_good + 2


# ---- 6. Bitcomp, every row width ----

def bitcomp_row_widths(stream, s):
    """The width byte of every row of a Bitcomp stream, in order (docs/HISTORY.md section 2, "Bitcomp stream layout");
    a zero-block marker counts as its rows of width 0. The stream must be consumed exactly."""
    b = bytes(stream)
    assert b[:4] == b"BTC\x01" and 1 << b[5] == s and b[6:8] == b"\0\0"
    n_bytes = struct.unpack_from("<I", b, 8)[0]
    lane_elems = 4 // s if s < 4 else 1
    row_elems = 64 * lane_elems
    rows_left = (n_bytes // s + row_elems - 1) // row_elems
    pos = 12
    widths = []
    while rows_left:
        rows = min(32, rows_left)
        if b[pos] == 0xFF:
            assert b[pos: pos + 4] == b"\xff\0\0\0"
            widths += [0] * rows
            pos += 4
        else:
            block = list(b[pos: pos + rows])
            assert not any(b[pos + rows: pos + (rows + 3) // 4 * 4]), "padding of the width bytes"
            widths += block
            pos += (rows + 3) // 4 * 4 + (sum(block) * lane_elems + 31) // 32 * 256
        rows_left -= rows
    assert pos + n_bytes % s == len(b)
    return widths


@pytest.mark.parametrize("typ", [1, 3, 5, 7])
@pytest.mark.parametrize("algo", [0, 1])
def test_bitcomp_every_row_width(backend, oracle, algo, typ):
    """A row of every width 0 .. 8 S, in rising order (a full-width row followed by a zero row where the cycle restarts) and
    in a second chunk in falling order, over several blocks with a partial last block and a partial last row. Algorithm 1
    packs the elements, algorithm 0 the zigzag of the differences: the sequence is built backwards from zigzag values of
    the wanted bit length, the all-ones one (difference -2^(8 S - 1)) among them. The width bytes read out of the
    stream are the planned ones."""
    s = WIDTH[typ]
    full = 8 * s
    lane_elems = 4 // s if s < 4 else 1
    row_elems = 64 * lane_elems
    rng = np.random.RandomState(6000 + 10 * typ + algo)
    n_rows = max(2 * (full + 1) + 3, 70)
    rising = [i % (full + 1) for i in range(n_rows)]
    chunks, plans = [], []
    for plan in (rising, rising[::-1]):
        rows = []
        for i, r in enumerate(plan):
            v = random_below(rng, row_elems if i + 1 < n_rows else 37, r).copy()
            if r:
                v[3] |= np.uint64(1 << (r - 1))
            if r == full:
                v[5] = (1 << full) - 1
            rows.append(v)
        v = np.concatenate(rows)
        if algo == 0:  # v is the zigzag: difference = (v >> 1) ^ -(v & 1), elements = running sum mod 2^(8 S)
            with np.errstate(over="ignore"):
                diff = (v >> np.uint64(1)) ^ (np.uint64(0) - (v & np.uint64(1)))
                v = np.cumsum(diff, dtype=np.uint64)
        chunks.append(v.astype(DT[s]).view(np.uint8))
        plans.append(plan)
    if algo == 0:
        e = cs.elements(chunks[0].tobytes(), s)
        assert any((b - a) % (1 << full) == 1 << (full - 1) for a, b in zip(e, e[1:])), "no difference of -2^(8 S - 1)"
    assert n_rows > 64 and n_rows % 32 and chunks[0].size // s % row_elems
    comp = bitcomp_roundtrip(backend, oracle, chunks, algo, typ)
    for cc, plan in zip(comp, plans):
        widths = bitcomp_row_widths(cc, s)
        assert widths == plan
        assert set(widths) == set(range(full + 1))
    both = list(zip(plans[0], plans[0][1:])) + list(zip(plans[1], plans[1][1:]))
    assert (full, 0) in both and (0, full) in both
