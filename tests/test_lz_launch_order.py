"""The order in which a persistent LZ4 / Snappy decode launch hands out its chunks (common/lz_order.hip.h: by descending
compressed size, chunks stored nearly raw last). A launch with more chunks than resident waves and the temp buffer of
the size query runs the order pass and maps every place of the launch to order[place]; the outputs, sizes and statuses
are by chunk index and must not change. What is checked here is that the order is a permutation in every launch -- a
duplicate or a hole shows as a wrong or an untouched slot -- and that every gate falls back to the launch without it.

Chunks are tiny (a batch above every gate is a few MB) and compressed on the host. The emulator's one-CU card keeps
eight waves resident, so a dozen chunks already draw tickets there; the forced "chase" build sends every batch size to
the persistent kernel on it. On the card the library is the shipped one."""
import ctypes as C

import numpy as np
import pytest

from nvcomp_amd import datasets
from nvcomp_amd.batched import BatchedCodec, empty_batch, make_batch

OK, BAD = 0, 12  # nvcompSuccess, nvcompErrorCannotDecompress
PAIR_MAX_BATCH = 4096  # NVCOMP_LZ_PAIR_MAX_BATCH as shipped (tests/test_abi.py holds the header and bench.py to it)
TOO_LONG = 0xFFFFFFFF - 63  # the first in_len the decode loop rejects unread (lzl::Chunk::too_long)
FILL = 0xA5


def order_temp_bytes(n):
    """What the order of n chunks needs of the temp buffer: the ticket's 16 bytes, a word per chunk, and 192 counters for
    each workgroup of the pass (one per 1 024 chunks, 64 at the most). The size query asks for it from 7 169 chunks on (the
    waves of a whole MI355X: below, a launch has a place for every chunk) and for the ticket alone below; a launch uses
    whatever buffer holds it."""
    return 16 + 4 * n + 4 * 192 * min(64, max(1, -(-n // 1024)))


def library(backend):
    from conftest import emu_path_library

    return emu_path_library("chase") if backend.name == "emu" else backend.lib


def order_entry(lib, fmt="LZ4"):
    fn = getattr(lib, f"nvcompAmd{fmt}DecompressOrderAsync")
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                   C.c_void_p]
    return fn


def resident_places(backend, fmt="LZ4"):
    """Waves of a persistent launch of the format's decoder on this card, from the library."""
    places = C.c_size_t(0)
    assert order_entry(library(backend), fmt)(None, None, 0, 0, None, 0, None, C.byref(places), None) == 0
    assert places.value > 0
    return places.value


def batch_sizes(backend, fmt):
    """Below the resident places (static places, no ticket), just above them, and well above."""
    fit = resident_places(backend, fmt)
    if backend.name == "emu":
        return [fit - 3, fit + 4, 1100]  # the last: two workgroups of the order pass
    assert fit > PAIR_MAX_BATCH + 4
    return [PAIR_MAX_BATCH + 4, fit + 8, 20000]


_pool = {}


def pool(oracle, fmt, count):
    """`count` chunks of 256 ... 1 024 bytes of the mix and their streams, made once per format and shared."""
    if fmt not in _pool or len(_pool[fmt][0]) < count:
        total = max(count, 20000 if count > 100 else 40)
        sizes = 256 + (np.arange(total) * 389) % 769
        data = datasets.silesia_style(int(sizes.sum()), 17, chunk=4096)
        ends = np.cumsum(sizes)
        chunks = [data[int(e - s): int(e)] for s, e in zip(sizes, ends)]
        enc = oracle.lz4_compress if fmt == "LZ4" else oracle.snappy_compress
        _pool[fmt] = (chunks, [enc(c) for c in chunks])
    chunks, comp = _pool[fmt]
    return chunks[:count], comp[:count]


def decode(backend, fmt, comp, caps, checked, temp="query", in_lens=None):
    """One nvcompBatched<fmt>DecompressAsync over pre-filled outputs, sizes and statuses -> (slots, sizes, statuses or
    None). `temp`: "query" (a fresh buffer of the size the query asks for) or (buffer, bytes). `in_lens` replaces the
    compressed sizes the call is told."""
    d = backend.dev
    codec = BatchedCodec(library(backend), d, fmt)
    n = len(comp)
    cb = make_batch(d, comp, align=1)
    if in_lens is not None:
        cb.sizes = d.upload(np.asarray(in_lens, dtype=np.uint64).view(np.uint8))
    ob = empty_batch(d, [c + 8 for c in caps], fill=FILL)  # eight guard bytes behind every slot
    ob.sizes = d.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    actual = d.upload(np.full(n, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
    statuses = d.upload(np.full(n, -1, dtype=np.int32).view(np.uint8)) if checked else None
    if temp == "query":  # of a batch the query gives the order's room for: the emulator's card is full with eight chunks
        tb = codec.decompress_temp_size(max(n, 7169), max(caps + [1]))
        assert tb >= order_temp_bytes(n)
        temp = (d.empty(tb), tb)
    assert codec.decompress_async(cb, ob, actual, statuses, temp[0], temp[1]) == 0
    d.synchronize()
    host = d.download(ob.slab)
    slots = [host[int(o): int(o) + c + 8] for o, c in zip(ob.offsets, caps)]
    return (slots, d.download(actual).view(np.uint64)[:n],
            d.download(statuses).view(np.int32)[:n] if checked else None)


def check_all_decoded(result, chunks, what=""):
    slots, actual, statuses = result
    assert actual.tolist() == [c.size for c in chunks], what
    if statuses is not None:
        assert (statuses == OK).all(), what
    for i, (s, c) in enumerate(zip(slots, chunks)):
        assert np.array_equal(s[: c.size], c) and (s[c.size:] == FILL).all(), (what, i)


FORMATS = pytest.mark.parametrize("fmt", ["LZ4", "Snappy"])
CHECKED = pytest.mark.parametrize("checked", [True, False], ids=["statuses", "no statuses"])


@FORMATS
@CHECKED
def test_every_chunk_is_decoded_once(backend, oracle, fmt, checked):
    """Batch sizes on both sides of the gates: the two-wave threshold, the resident places, and far above."""
    for n in batch_sizes(backend, fmt):
        chunks, comp = pool(oracle, fmt, n)
        check_all_decoded(decode(backend, fmt, comp, [c.size for c in chunks], checked), chunks, n)


def literal_chunks(count, step):
    """Chunk i: the first 16 + i * step of one sequence of random non-zero bytes, then an eighth as many (+ 64) zeros --
    its stream is the literals and a few bytes, so the compressed sizes rise strictly with i, and every chunk shrinks by
    more than a tenth (it has a key)."""
    noise = np.random.RandomState(5).randint(1, 256, 16 + count * step).astype(np.uint8)
    return [np.concatenate([noise[: 16 + i * step], np.zeros((16 + i * step) // 8 + 64, np.uint8)]) for i in range(count)]


@FORMATS
@CHECKED
@pytest.mark.parametrize("shape", ["one size", "increasing", "decreasing"])
def test_sizes_that_stress_the_key(backend, oracle, fmt, checked, shape):
    """All chunks in one bucket; compressed sizes strictly increasing and strictly decreasing by index (the order is
    then the exact reverse of, or exactly, the index order, bucket by bucket)."""
    n = resident_places(backend, fmt) + 8
    enc = oracle.lz4_compress if fmt == "LZ4" else oracle.snappy_compress
    if shape == "one size":
        chunks, comp = pool(oracle, fmt, 1)
        chunks, comp = chunks * n, comp * n
    else:
        chunks = literal_chunks(n, 1)
        comp = [enc(c) for c in chunks]
        lens = np.array([c.size for c in comp])
        assert (np.diff(lens) > 0).all() and all(cc.size * 10 < c.size * 9 for cc, c in zip(comp, chunks))
        if shape == "decreasing":
            chunks, comp = chunks[::-1], comp[::-1]
    check_all_decoded(decode(backend, fmt, comp, [c.size for c in chunks], checked), chunks)


@FORMATS
@CHECKED
def test_cheap_and_rejected_chunks_among_the_rest(backend, oracle, fmt, checked):
    """Every seventh chunk is one of: empty, random bytes (its stream is longer than the capacity it is given: in_len >
    cap), nearly raw (shrinks by under a tenth), and, once, a chunk whose declared length is over the limit and which
    the loop rejects unread. The expectation is the CPU decoder's for every stream; the chunk over the limit fails
    with size 0 like any chunk that cannot be decoded."""
    n = resident_places(backend, fmt) + 8
    chunks, comp = (list(x) for x in pool(oracle, fmt, n))
    enc, dec = ((oracle.lz4_compress, oracle.lz4_decompress) if fmt == "LZ4" else (oracle.snappy_compress, oracle.snappy_decompress))
    rng = np.random.RandomState(9)
    for k, i in enumerate(range(3, n, 7)):
        kind = k % 3
        if kind == 0:
            chunks[i] = np.zeros(0, np.uint8)
        elif kind == 1:
            chunks[i] = rng.randint(0, 256, 300 + k % 50).astype(np.uint8)
        else:
            chunks[i] = np.concatenate([rng.randint(0, 256, 500).astype(np.uint8), np.zeros(24, np.uint8)])
        comp[i] = enc(chunks[i]) if chunks[i].size else np.zeros(0, np.uint8)
        if kind == 1:
            assert comp[i].size > chunks[i].size
        elif kind == 2:
            assert chunks[i].size * 9 <= comp[i].size * 10 and comp[i].size <= chunks[i].size
    caps = [c.size for c in chunks]
    in_lens = [c.size for c in comp]
    over = n // 2
    in_lens[over] = TOO_LONG
    want = []
    for i in range(n):
        rc, out = (1, None) if i == over else dec(comp[i], caps[i])
        want.append((OK, out) if rc == 0 else (BAD, np.zeros(0, np.uint8)))
    slots, actual, statuses = decode(backend, fmt, comp, caps, checked, in_lens=in_lens)
    assert actual.tolist() == [w[1].size for w in want]
    if checked:
        assert statuses.tolist() == [w[0] for w in want]
    for i, (s, (st, out)) in enumerate(zip(slots, want)):
        assert (s[caps[i]:] == FILL).all(), i
        if st == OK:
            assert np.array_equal(s[: out.size], out) and np.array_equal(out, chunks[i]), i


@FORMATS
@CHECKED
def test_one_temp_buffer_for_batches_of_different_sizes(backend, oracle, fmt, checked):
    """The ticket and the order are rebuilt by every call: a larger batch after a smaller one, then a smaller again."""
    small, _, large = batch_sizes(backend, fmt)
    mid = resident_places(backend, fmt) + 8
    d = backend.dev
    codec = BatchedCodec(library(backend), d, fmt)
    tb = codec.decompress_temp_size(max(large, 7169), 1024)
    temp = d.upload(np.full(tb, 0xFF, dtype=np.uint8))
    all_chunks, all_comp = pool(oracle, fmt, large)
    for n, first in ((mid, 0), (large, 0), (mid, large - mid), (small, 5)):
        chunks, comp = all_chunks[first: first + n], all_comp[first: first + n]
        check_all_decoded(decode(backend, fmt, comp, [c.size for c in chunks], checked, temp=(temp, tb)), chunks, (n, first))


@FORMATS
@CHECKED
def test_temp_buffers_that_cannot_hold_the_order(backend, oracle, fmt, checked):
    """Room for the ticket alone, one word short of the order, off by one to three bytes, none at all: the launches
    without the order, with the same results."""
    n = resident_places(backend, fmt) + 8
    chunks, comp = pool(oracle, fmt, n)
    caps = [c.size for c in chunks]
    d = backend.dev
    tb = order_temp_bytes(n)
    if n > 7168:
        assert BatchedCodec(library(backend), d, fmt).decompress_temp_size(n, max(caps)) == tb
    whole = d.upload(np.full(tb + 4, 0xFF, dtype=np.uint8))
    assert d.ptr(whole) % 4 == 0
    cases = [("ticket only", whole, 16), ("a word short", whole, tb - 4), ("null", None, 0)]
    cases += [(f"off by {k}", whole[k:], tb) for k in (1, 2, 3)]
    for what, temp, temp_bytes in cases:
        check_all_decoded(decode(backend, fmt, comp, caps, checked, temp=(temp, temp_bytes)), chunks, what)


def order_key(in_len, cap):
    """The documented key: the compressed size, 0 for a chunk stored nearly raw (in_len * 10 >= cap * 9, capacities
    clamped to 2^26 as everywhere)."""
    cap = min(cap, 1 << 26)
    return 0 if in_len * 10 >= cap * 9 else in_len


def size_arrays(shape, n):
    rng = np.random.RandomState(n)
    caps = np.full(n, 65536, dtype=np.uint64)
    if shape == "increasing":
        lens = 1 + np.arange(n, dtype=np.uint64) % 58000
    elif shape == "decreasing":
        lens = (1 + np.arange(n, dtype=np.uint64) % 58000)[::-1].copy()
    elif shape == "one size":
        lens = np.full(n, 30000, dtype=np.uint64)
    else:  # every kind of chunk and capacity
        lens = rng.randint(0, 70000, n).astype(np.uint64)
        caps = rng.choice(np.array([0, 1, 300, 65536, 1 << 20, 1 << 26, 1 << 40], dtype=np.uint64), n)
        lens[rng.randint(0, n, max(n // 50, 1))] = TOO_LONG
        lens[rng.randint(0, n, max(n // 50, 1))] = np.uint64(1 << 63)
    return lens, caps


@FORMATS
@pytest.mark.parametrize("shape", ["increasing", "decreasing", "one size", "mixed"])
def test_the_order_is_a_permutation_by_descending_key(backend, fmt, shape):
    """The order pass alone, on size arrays only (it reads no stream): batches of one workgroup of the pass, of several
    with a ragged last one, and of its full width. The ordered part is a permutation of its chunks, and along it the key
    never rises by more than a bucket is wide (an eighth of an octave: a later chunk's key is under 9/8 of every earlier one's, + 1)."""
    d = backend.dev
    fn = order_entry(library(backend), fmt)
    for n in ([1, 700, 2500] if backend.name == "emu" else [1, 1000, 1025, 7177, 70001]):
        lens, caps = size_arrays(shape, n)
        tb = order_temp_bytes(n)  # exactly: four bytes less are refused below
        temp = d.upload(np.full(tb, 0xFF, dtype=np.uint8))
        offset = C.c_size_t(0)
        dl, dc = d.upload(lens.view(np.uint8)), d.upload(caps.view(np.uint8))
        assert fn(d.ptr(dl), d.ptr(dc), 0, n, d.ptr(temp), tb - 4, C.byref(offset), None, d.stream()) != 0  # too small
        assert fn(d.ptr(dl), d.ptr(dc), n + 1, n, d.ptr(temp), tb, C.byref(offset), None, d.stream()) != 0
        for first in sorted({0, n // 3, n - 1, n}):  # the places in front of `first` keep their own chunks
            temp = d.upload(np.full(tb, 0xFF, dtype=np.uint8))
            assert fn(d.ptr(dl), d.ptr(dc), first, n, d.ptr(temp), tb, C.byref(offset), None, d.stream()) == 0
            d.synchronize()
            host = d.download(temp)
            assert host[:4].view(np.uint32)[0] == 0, "the pass clears the ticket"
            order = host[offset.value: offset.value + 4 * n].view(np.uint32)
            assert np.array_equal(order[:first], np.arange(first, dtype=np.uint32)), (shape, n, first)
            assert np.array_equal(np.sort(order[first:]), np.arange(first, n, dtype=np.uint32)), (shape, n, first)
            keys = np.array([order_key(int(lens[i]), int(caps[i])) for i in order[first:]], dtype=np.uint64)
            if keys.size > 1:
                lowest_before = np.minimum.accumulate(keys)
                assert (keys[1:] * 8 <= lowest_before[:-1] * 9 + 8).all(), (shape, n, first)
            if shape in ("increasing", "decreasing") and first == 0 and n > 1:
                assert keys[0] > keys[-1]


@pytest.mark.parametrize("fmt", ["LZ4", "Snappy"])
def test_temp_size_holds_the_order(backend, fmt):
    """Nothing for no batch, the ticket alone for batches a whole card has places for, above that the order's room as
    well. The compress query stays at the ticket."""
    codec = BatchedCodec(library(backend), backend.dev, fmt)
    assert codec.decompress_temp_size(0, 65536) == 0
    for n in (1, 5000, 7168):
        assert codec.decompress_temp_size(n, 65536) == 16
    for n in (7169, 20000, 65536, 1 << 20):
        assert codec.decompress_temp_size(n, 65536) == order_temp_bytes(n)
    assert codec.compress_temp_size(65536, 65536) == 16
