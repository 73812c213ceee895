"""The compressor of the device-side Snappy API (include/nvcomp/device/snappy.hpp): kernels of
tests/device_api/snappy_device_kernels.hip call compress(), on the host emulation and on the MI355X (`backend`) -- from
global memory to global memory, from LDS to global memory and from LDS into LDS. Every stream is held to the same things:
its size is 1 ... max_compressed_bytes(n); a strict element walk in Python finds the rules kept (the preamble equals n, no
copy-4, offsets 1 ... 65 535 and never in front of the chunk, no copy piece shorter than 4, literal lengths spelled
shortest); libsnappy / the oracle, the batched decoder and the device decoder each return the chunk. Every output slot is
max_compressed_bytes(n) long, prefilled, and followed by 32 guard bytes of 0xA5 that must survive."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from nvcomp_amd import datasets
from nvcomp_amd._lib import NvcompStatus
from nvcomp_amd.batched import DeviceBatch

import test_snappy_device as dec
from test_snappy_device import HIPCC, REPO, SRC, _need_hipcc, k, kernels  # noqa: F401  (k: the fixture)

GUARD = 32
PREFILL = 0x5A
MODES = ("gg", "lg", "ll")  # global -> global, LDS (staged by the wave) -> global, LDS -> LDS (copied out)
LEFTOVERS, ONES, ZEROS = 0, 1, 2  # what the scratch area holds at a call
OK = int(NvcompStatus.Success)
TOO_LARGE_FOR_LDS = (1 << 64) - 1
_held = set()


def bound(n):
    return 32 + n + n // 6


def rnd(rng, n):
    return rng.randint(0, 256, size=n).astype(np.uint8)


def as_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()


# ---- the format rules, walked in Python ----

def walk(stream, n):
    """The elements of a stream that must decode to n bytes: [("lit", length, position) | ("copy", length, offset,
    position)]. Asserts the rules compress() promises."""
    b = bytes(stream)
    total = shift = i = 0
    while True:
        assert i < len(b) and i < 5, "the preamble runs off the stream"
        x = b[i]
        i += 1
        total |= (x & 127) << shift
        shift += 7
        if not x & 128:
            break
    assert total == n, f"the preamble says {total}, the chunk has {n} bytes"
    assert i == len(dec.varint(n)), "the preamble is not the shortest varint"
    out, els = 0, []
    while i < len(b):
        tag = b[i]
        i += 1
        kind = tag & 3
        if kind == 0:
            m = tag >> 2
            if m >= 60:
                nb = m - 59
                assert i + nb <= len(b)
                m = int.from_bytes(b[i: i + nb], "little")
                i += nb
                assert m >= (60 if nb == 1 else 1 << (8 * (nb - 1))), f"a literal of {m + 1} bytes with {nb} length bytes"
            i += m + 1
            assert i <= len(b), "literals run off the stream"
            els.append(("lit", m + 1, out))
            out += m + 1
            continue
        assert kind != 3, "a copy-4 element"
        if kind == 1:
            ln, off = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | b[i]
            i += 1
        else:
            ln, off = 1 + (tag >> 2), b[i] | (b[i + 1] << 8)
            i += 2
            assert not (4 <= ln <= 11 and off < 2048), f"copy-2 for length {ln} at offset {off}: copy-1 is shorter"
        assert i <= len(b)
        assert 1 <= off <= 65535 and off <= out, f"offset {off} at position {out}"
        assert ln >= 4, f"a copy piece of {ln} bytes"
        els.append(("copy", ln, off, out))
        out += ln
    assert out == n, f"the stream decodes to {out} bytes, not {n}"
    return els


def matches(els):
    """Copy pieces joined back into matches: [(offset, length, position)]."""
    ms = []
    prev = None
    for e in els:
        if e[0] == "copy" and prev is not None and prev[0] == "copy" and ms[-1][0] == e[2]:
            ms[-1] = (ms[-1][0], ms[-1][1] + e[1], ms[-1][2])
        elif e[0] == "copy":
            ms.append((e[2], e[1], e[3]))
        prev = e
    return ms


# ---- running the kernels ----

def place(dev, chunks, aligns, pad=0, fill=None, prefill=None):
    """Chunks (or, with `fill`, empty slots of these sizes, themselves holding `prefill`) in one slab of `fill` (0xA5),
    chunk i at an address that is aligns[i] mod 16, `pad` bytes of room behind each. Returns the batch and the slab's
    bytes."""
    n = len(chunks)
    sizes = [c if fill is not None else c.size for c in chunks]
    offs, pos = [], 16
    for s, a in zip(sizes, aligns):
        pos = (pos + 15) // 16 * 16 + a
        offs.append(pos)
        pos += s + pad
    host = np.full(pos + 16, 0xA5 if fill is None else fill, dtype=np.uint8)
    for c, o in zip(chunks, offs):
        if fill is None:
            host[o: o + c.size] = c
        elif prefill is not None:
            host[o: o + c] = prefill
    slab = dev.upload(host)
    base = dev.ptr(slab)
    assert base % 16 == 0
    offs = np.asarray(offs, dtype=np.int64)
    ptrs = dev.upload((offs.astype(np.uint64) + np.uint64(base)).view(np.uint8)) if n else dev.upload(np.zeros(8, np.uint8))
    hs = np.asarray(sizes, dtype=np.uint64)
    return DeviceBatch(slab, ptrs, dev.upload(hs.view(np.uint8)) if n else dev.upload(np.zeros(8, np.uint8)), offs, hs, n), host


def per_chunk(v, n):
    return [v] * n if isinstance(v, int) else list(v)


def dev_compress(backend, k, chunks, mode="gg", block=None, in_align=0, out_align=0, fill=LEFTOVERS, grid=None,
                 chunks_per_wave=1):
    """compress() over a batch; returns the streams. gg: in_align / out_align place the chunks and the slots in global
    memory (an int or one per chunk); lg, ll: the global placement is 16-byte aligned and the ints place the chunk and
    (ll) the stream in LDS. Asserts 1 <= size <= bound, the guards behind every slot and around the scratch areas."""
    d = backend.dev
    n = len(chunks)
    sizes = [c.size for c in chunks]
    gg = mode == "gg"
    if block is None:
        block = 256 if gg or max(sizes + [0]) <= k.snpcmp_lds_in_bytes(256) else 64
    src, src_host = place(d, chunks, per_chunk(in_align, n) if gg else [0] * n)
    out, _ = place(d, [bound(s) for s in sizes], per_chunk(out_align, n) if gg else [0] * n, pad=GUARD, fill=0xA5, prefill=PREFILL)
    got = d.upload(np.full(n, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
    flags = d.upload(np.zeros(4, dtype=np.uint8))
    if grid is None:
        waves = -(-n // chunks_per_wave)
        grid = max(1, -(-waves // (block // 64)))
    p = d.ptr
    if gg:
        rc = k.snpcmp_global(p(src.ptrs), p(src.sizes), p(out.ptrs), p(got), n, block, grid, fill, p(flags), d.stream())
    else:
        rc = k.snpcmp_lds(p(src.ptrs), p(src.sizes), p(out.ptrs), p(got), n, 1 if mode == "ll" else 0, int(in_align),
                          int(out_align), block, grid, fill, p(flags), d.stream())
    assert rc == 0
    d.synchronize()
    assert d.download(flags).view(np.uint32)[0] == 0, "a guard around a scratch area or behind a stream in LDS changed"
    assert np.array_equal(d.download(src.slab), src_host), "the input was written to"
    host = d.download(out.slab)
    got = d.download(got).view(np.uint64)[:n]
    assert (got != TOO_LARGE_FOR_LDS).all(), "the test kernel's LDS cannot hold this chunk: a bug in this test"
    streams = []
    for o, s, g in zip(out.offsets, sizes, got):
        o, g = int(o), int(g)
        assert 1 <= g <= bound(s), f"size {g} for a chunk of {s} bytes"
        assert (host[o + bound(s): o + bound(s) + GUARD] == 0xA5).all(), "a write past the bound"
        assert (host[o - 16: o] == 0xA5).all(), "a write in front of the slot"
        streams.append(host[o: o + g].copy())
    return streams


def hold(backend, oracle, k, chunks, streams, device_modes=("gg",), emulated_decoders=True):
    """What each stream is held to. Returns the walks. emulated_decoders=False: on the emulator the oracle alone decodes."""
    sizes = [c.size for c in chunks]
    walks = [walk(s, c.size) for s, c in zip(streams, chunks)]
    for i, (s, c) in enumerate(zip(streams, chunks)):
        rc, back = oracle.snappy_decompress(s, c.size)
        assert rc == 0 and np.array_equal(back, c), f"the oracle, chunk {i}"
        if oracle.have_ref():
            rc, back = oracle.ref_snappy_decompress(s, c.size)
            assert rc == 0 and np.array_equal(back, c), f"libsnappy, chunk {i}"
    if backend.name == "emu" and not emulated_decoders:
        return walks
    # a (chunk, stream) pair that the decoders of this backend have already returned the chunk for is not decoded again: the
    # address modes and scratch contents mostly give the same stream
    keys = [(backend.name, device_modes, hashlib.sha1(c.tobytes()).digest(), hashlib.sha1(s.tobytes()).digest())
            for c, s in zip(chunks, streams)]
    fresh = [i for i, key in enumerate(keys) if key not in _held]
    chunks, streams, sizes = [chunks[i] for i in fresh], [streams[i] for i in fresh], [sizes[i] for i in fresh]
    if not fresh:
        return walks
    outs, actual, status = backend.codec("Snappy").decompress(streams, sizes)
    assert (status == OK).all() and actual.tolist() == sizes
    assert all(np.array_equal(o, c) for o, c in zip(outs, chunks)), "the batched decoder"
    for mode in device_modes:
        outs, actual, status = dec.dev_decompress(backend, k, streams, sizes, mode=mode, in_align=5, out_align=3)
        assert (status == OK).all() and actual.tolist() == sizes, "the device decoder refuses a stream"
        assert all(np.array_equal(o, c) for o, c in zip(outs, chunks)), "the device decoder"
    _held.update(keys[i] for i in fresh)
    return walks


def fits_lds(k, chunks):
    return max([c.size for c in chunks] + [0]) <= k.snpcmp_lds_in_bytes(64)


def through(backend, oracle, k, chunks, modes=None, **kw):
    """compress() through every address combination the chunks fit, each stream held to the rules."""
    if modes is None:
        modes = MODES if fits_lds(k, chunks) else ("gg",)
    walks = {}
    for mode in modes:
        walks[mode] = hold(backend, oracle, k, chunks, dev_compress(backend, k, chunks, mode=mode, **kw))
    return walks


# ---- 1. chunk sizes ----

def test_chunk_sizes(backend, oracle, k):
    step = int(k.snpcmp_step_bytes())
    assert step == 64 and k.snpcmp_shared_bytes() % 16 == 0 and k.snpcmp_shared_bytes() <= 12 * 1024
    sizes = sorted({0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 63, 64, 65, step - 1, step, step + 1, 4096, 65535, 65536, 65537})
    base = datasets.text(70000, 9)
    chunks = [base[:s].copy() for s in sizes]
    small = [c for c in chunks if c.size <= k.snpcmp_lds_in_bytes(256)]
    for block in (64, 256):
        through(backend, oracle, k, small, block=block)
    large = [c for c in chunks if c.size > k.snpcmp_lds_in_bytes(256)]
    through(backend, oracle, k, large, modes=("gg",), block=256)
    through(backend, oracle, k, [c for c in large if c.size <= k.snpcmp_lds_in_bytes(64)], modes=("lg", "ll"), block=64)
    walks = through(backend, oracle, k, [datasets.text(200000 if backend.name == "gpu" else 90000, 3)])
    assert max(m[0] for m in matches(walks["gg"][0])) <= 65535


def test_one_chunk_of_the_largest_size(backend, oracle, k):
    """1 << 24 bytes: zeros (one match of 1 << 24 - 1 bytes: 262 144 copy pieces written a piece a lane) and, on the card,
    text. On the emulator the walk and the oracle hold the stream: its emulated decoders take ten seconds over as many
    elements, and run this very stream shape on the card (test_snappy_device.py)."""
    n = int(k.snpdev_max_chunk_bytes())
    assert n == 1 << 24
    chunks = [np.zeros(n, np.uint8)] + ([datasets.text(n, 3)] if backend.name == "gpu" else [])
    streams = dev_compress(backend, k, chunks)
    walks = hold(backend, oracle, k, chunks, streams, emulated_decoders=False)
    assert matches(walks[0]) == [(1, n - 1, 1)]
    if len(walks) > 1:
        assert max(m[0] for m in matches(walks[1])) <= 65535


def test_an_empty_chunk_is_what_the_batched_compressor_writes(backend, k):
    (want,) = backend.codec("Snappy").compress([np.zeros(0, np.uint8)])
    for mode in MODES:
        (got,) = dev_compress(backend, k, [np.zeros(0, np.uint8)], mode=mode)
        assert got.tolist() == want.tolist() == [0]


def test_a_chunk_above_the_largest_size_is_refused_untouched(backend, k):
    d = backend.dev
    n = 1 << 24
    inb, outb = d.upload(np.full(64, 0xA5, np.uint8)), d.upload(np.full(64, 0xA5, np.uint8))
    size = d.upload(np.full(1, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
    flags = d.upload(np.zeros(4, dtype=np.uint8))
    assert k.snpcmp_too_large(d.ptr(inb) + 32, n + 1, d.ptr(outb) + 32, d.ptr(size), d.ptr(flags), d.stream()) == 0
    d.synchronize()
    assert d.download(size).view(np.uint64)[0] == 0
    assert d.download(flags).view(np.uint32)[0] == 0, "the scratch area was touched"
    assert (d.download(inb) == 0xA5).all() and (d.download(outb) == 0xA5).all()


@pytest.mark.parametrize("n", [0, 1, 5, 6, 65536, 1 << 24])
def test_max_compressed_bytes(backend, k, n):
    assert k.snpcmp_max_compressed_bytes(n) == backend.codec("Snappy").max_compressed_size(n) == bound(n)
    assert bound(65536) == 76490


# ---- 2. zeros, literal runs, match lengths, distances ----

def test_zeros(backend, oracle, k):
    """One literal byte, then one match to the chunk's last byte."""
    chunks = [np.zeros(n, np.uint8) for n in list(range(8, 41)) + [100000]]
    for mode, ws in through(backend, oracle, k, chunks[:-1]).items():
        for c, els in zip(chunks, ws):
            ms = matches(els)
            assert len(ms) == 1 and ms[0] == (1, c.size - 1, 1), f"{mode}: {c.size} zeros: {els}"
    (els,) = through(backend, oracle, k, chunks[-1:])["gg"]
    assert matches(els) == [(1, 99999, 1)]


def planted(rng, runs, lengths):
    """The source bytes and 70 random ones (a step of the compressor looks for candidates in front of itself), then for
    every (literal run, match length): that many random bytes and a copy of the chunk's first bytes. The byte behind a copy
    differs from the byte behind its source and behind every earlier copy, the byte in front of it from the byte in front
    of every earlier copy: neither end of a planted match can grow."""
    src = rnd(rng, max(lengths) + 1)
    out = [src, rnd(rng, 70)]
    firsts, lasts = set(), set()

    def fresh(taken, avoid):
        b = int(rng.randint(0, 256))
        while b in taken or b in avoid:
            b = (b + 1) & 255
        taken.add(b)
        return b

    for i, (ll, ml) in enumerate(zip(runs, lengths)):
        lit = rnd(rng, ll)
        assert ll >= 2
        if i:
            lit[0] = fresh(firsts, {int(src[m]) for m in lengths})
        lit[-1] = fresh(lasts, set())
        out += [lit, src[:ml]]
    tail = rnd(rng, 13)
    tail[0] = fresh(firsts, {int(src[m]) for m in lengths})
    out.append(tail)
    return np.concatenate(out)


def test_literal_run_boundaries(backend, oracle, k):
    rng = np.random.RandomState(11)
    runs = [59, 60, 61, 256, 257]
    chunks = [planted(rng, runs, [24] * 5), planted(rng, runs[::-1], [24] * 5)]
    chunks += [planted(rng, [ll, ll], [24, 24]) for ll in runs]
    for mode, ws in through(backend, oracle, k, chunks).items():
        for ll, els in zip(runs, ws[2:]):
            # (the run in front of the first copy also holds the chunk's head; a hash collision may move a match's start by a
            # byte, but not both runs')
            assert ll in [e[1] for e in els if e[0] == "lit"], (mode, ll, els)


def test_match_length_boundaries(backend, oracle, k):
    rng = np.random.RandomState(12)
    lengths = [4, 11, 12, 64, 65, 67, 68, 128, 1000]
    chunks = [planted(rng, [9] * 9, lengths), planted(rng, [70] * 9, lengths[::-1])]
    chunks += [planted(rng, [9, 9], [ml, ml]) for ml in lengths]
    for mode, ws in through(backend, oracle, k, chunks).items():
        for ml, els in zip(lengths, ws[2:]):
            got = [m[1] for m in matches(els)]
            assert got == [ml, ml], (mode, ml, got)


@pytest.mark.parametrize("dist", [2047, 2048])
def test_the_copy1_distance_boundary(backend, oracle, k, dist):
    rng = np.random.RandomState(dist)
    chunk = rnd(rng, 3000)
    chunk[dist + 100: dist + 108] = chunk[100: 108]
    els = through(backend, oracle, k, [chunk])["gg"][0]
    assert (dist, 8, dist + 100) in matches(els)  # (the walk has checked the spelling: copy-1 below 2 048, copy-2 from there)


@pytest.mark.parametrize("dist", [65535, 65536, 65537])
def test_distance_boundaries(backend, oracle, k, dist):
    """70 000 random bytes whose only repeat lies `dist` back; and the same with nothing but one run of zeros in between,
    so that the table still holds the first occurrence when the second comes: its two-byte entry then reads as distance
    65 535, 0 and 1."""
    rng = np.random.RandomState(dist)
    noise = rnd(rng, 70000)
    noise[69000: 69040] = noise[69000 - dist: 69040 - dist]
    held = np.zeros(70000, np.uint8)
    held[:48] = rng.randint(1, 256, size=48)
    held[dist: dist + 48] = held[:48]
    held[dist + 48:] = rnd(rng, 70000 - dist - 48)
    walks = through(backend, oracle, k, [noise, held], modes=("gg",))["gg"]
    if dist != 65535:
        assert not matches(walks[0]), "random bytes with one repeat beyond the reach: no match exists"
    far = [off for off, _, start in matches(walks[1]) if start >= dist]
    if dist == 65535:
        assert 65535 in far
    else:  # no match behind the run of zeros has its source in the chunk's first 48 bytes: those lie out of reach
        assert all(start - off >= 48 for off, _, start in matches(walks[1]) if start >= dist), matches(walks[1])[-5:]


def test_incompressible(backend, oracle, k):
    chunk = rnd(np.random.RandomState(13), 65536)
    for mode in MODES:
        (s,) = dev_compress(backend, k, [chunk], mode=mode)
        assert 65536 < s.size <= bound(65536)
        hold(backend, oracle, k, [chunk], [s])


# ---- 3. data classes, and the ratio against the batched compressor ----

def class_chunks(backend):
    n = 20000 if backend.name == "emu" else 65536
    return {name: as_bytes(datasets.CLASSES[name](n, 1))[:n] for name in sorted(datasets.CLASSES)}


@pytest.mark.parametrize("name", sorted(datasets.CLASSES))
def test_classes(backend, oracle, k, name):
    through(backend, oracle, k, [class_chunks(backend)[name]])


# The device compressor's total over one chunk of every class against the batched compressor's, measured on the emulator
# (20 000-byte chunks): the batched compressor wrote 123 356, 123 375 and 123 358 bytes in three runs -- a mean of 123 363
# and a spread of 19 bytes, 0.0154 %: its hash-slot races under the emulator's changing lane order. The device compressor
# wrote 123 269 bytes over a zeroed scratch area: an excess of -94 bytes (-0.076 %) against the batched mean, i.e. none. The
# bound is that excess, counted as 0, plus the spread, rounded up to the next hundredth of a per cent.
RATIO_EXCESS = 0.0002


def test_ratio_against_the_batched_compressor(backend, k):
    chunks = list(class_chunks(backend).values())
    runs = [sum(s.size for s in backend.codec("Snappy").compress(chunks)) for _ in range(3)]
    batched = sum(runs) / 3
    device = sum(s.size for s in dev_compress(backend, k, chunks, fill=ZEROS))
    print(f"batched {runs} device {device} excess {device / batched - 1:.4%} spread {(max(runs) - min(runs)) / batched:.4%}")
    assert device <= batched * (1 + RATIO_EXCESS)


# ---- 4. alignments, scratch contents, launch shapes ----

def test_alignments(backend, oracle, k):
    chunk = datasets.silesia_style(4 * 65536, 5)[65536: 65536 + 1500].copy()
    als = (0, 1, 3, 8, 15)
    pairs = [(a, b) for a in als for b in als]
    streams = dev_compress(backend, k, [chunk] * len(pairs), in_align=[a for a, _ in pairs], out_align=[b for _, b in pairs])
    hold(backend, oracle, k, [chunk] * len(pairs), streams, device_modes=dec.MODES)
    for ia, oa in ((0, 0), (5, 11), (15, 1)):
        for mode in ("lg", "ll"):
            hold(backend, oracle, k, [chunk] * 4, dev_compress(backend, k, [chunk] * 4, mode=mode, in_align=ia, out_align=oa))


@pytest.mark.parametrize("block", [64, 256])
def test_what_the_scratch_area_holds_does_not_matter(backend, oracle, k, block):
    """Every wave compresses four chunks one after the other: over zeros, over 0xFF, over its last chunk's leftovers."""
    gens = sorted(datasets.CLASSES)
    chunks = [as_bytes(datasets.CLASSES[gens[i % len(gens)]](3000 + 501 * (i % 7), i))[: 3000 + 501 * (i % 7)] for i in range(16)]
    sizes = {}
    for fill in (ZEROS, ONES, LEFTOVERS):
        for mode in MODES:
            streams = dev_compress(backend, k, chunks, mode=mode, block=block, fill=fill, chunks_per_wave=4)
            hold(backend, oracle, k, chunks, streams)
            sizes[fill, mode] = sum(s.size for s in streams)
    # garbage costs candidates that fail their check, never matches: the totals stay within a per cent of the clean ones
    for key, total in sizes.items():
        assert total <= sizes[ZEROS, key[1]] * 1.01, (key, total, sizes[ZEROS, key[1]])


def test_many_chunks_share_workgroups(backend, oracle, k):
    """256 chunks over 4 workgroups of 256 threads: every wave loops over 16 chunks beside waves on other chunks."""
    gens = sorted(datasets.CLASSES)
    chunks = [as_bytes(datasets.CLASSES[gens[i % len(gens)]](1500, i))[: 300 + 23 * (i % 16)] for i in range(256)]
    for mode in MODES:
        hold(backend, oracle, k, chunks, dev_compress(backend, k, chunks, mode=mode, block=256, grid=4))


# ---- 5. the last byte in front of an unmapped page (emulator only) ----

def test_nothing_is_touched_behind_the_chunk_or_the_bound(emu, oracle, tmp_path_factory):
    """Host memory: the chunk's last byte, then the last byte of the output bound, is the last byte in front of a
    PROT_NONE page, or lies one, two, three bytes in front of it. A read or write past the end is a segmentation fault.
    (Never on the card: there the guard bytes stand in.)"""
    from hlif_container import guarded_mapping

    k = kernels(emu, tmp_path_factory)
    base, span = guarded_mapping(2)
    text = datasets.text(3000, 4)
    ends_in_a_match = np.concatenate([text[:2000], text[100:1100]])  # the last match runs to the chunk's last byte
    for chunk in (text, ends_in_a_match, np.zeros(777, np.uint8)):
        sizes = np.array([chunk.size], dtype=np.uint64)
        for back in (0, 1, 2, 3):
            got, flags = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
            # the chunk against the page
            at = span - back - chunk.size
            C.memmove(base + at, chunk.ctypes.data, chunk.size)
            out = np.full(bound(chunk.size) + GUARD, 0xA5, dtype=np.uint8)
            ptrs, optrs = np.array([base + at], dtype=np.uint64), np.array([out.ctypes.data], dtype=np.uint64)
            assert k.snpcmp_global(ptrs.ctypes.data, sizes.ctypes.data, optrs.ctypes.data, got.ctypes.data, 1, 64, 1, ONES,
                                   flags.ctypes.data, None) == 0
            assert flags[0] == 0 and 1 <= got[0] <= bound(chunk.size) and (out[bound(chunk.size):] == 0xA5).all()
            walk(out[: int(got[0])], chunk.size)
            rc, again = oracle.snappy_decompress(out[: int(got[0])].copy(), chunk.size)
            assert rc == 0 and np.array_equal(again, chunk)
            # the output bound against the page
            src = chunk.copy()
            oat = span - back - bound(chunk.size)
            ptrs, optrs = np.array([src.ctypes.data], dtype=np.uint64), np.array([base + oat], dtype=np.uint64)
            assert k.snpcmp_global(ptrs.ctypes.data, sizes.ctypes.data, optrs.ctypes.data, got.ctypes.data, 1, 64, 1, ONES,
                                   flags.ctypes.data, None) == 0
            assert flags[0] == 0 and 1 <= got[0] <= bound(chunk.size)
            stream = np.ctypeslib.as_array((C.c_uint8 * int(got[0])).from_address(base + oat)).copy()
            rc, again = oracle.snappy_decompress(stream, chunk.size)
            assert rc == 0 and np.array_equal(again, chunk)
    # incompressible: the stream is the chunk and a few header bytes
    noise = rnd(np.random.RandomState(5), 3000)
    oat = span - bound(noise.size)
    sizes = np.array([noise.size], dtype=np.uint64)
    ptrs, optrs = np.array([noise.ctypes.data], dtype=np.uint64), np.array([base + oat], dtype=np.uint64)
    got, flags = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    assert k.snpcmp_global(ptrs.ctypes.data, sizes.ctypes.data, optrs.ctypes.data, got.ctypes.data, 1, 64, 1, ONES,
                           flags.ctypes.data, None) == 0
    assert flags[0] == 0 and noise.size < got[0] <= bound(noise.size)


# ---- 6. the header's promises ----

def test_kernels_that_call_the_api_use_no_private_scratch(tmp_path):
    """hipcc -Rpass-analysis=kernel-resource-usage over the test kernels: a scratch size of 0 for every kernel that calls
    decompress or compress."""
    _need_hipcc()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(REPO, "include"),
                        "--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", SRC, "-o", str(tmp_path / "k.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    usage = dict(re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", r.stderr, flags=re.S))
    callers = {name: int(v) for name, v in usage.items()
               if any(t in name for t in ("kd_global", "kd_lds", "k_mixed", "kc_global", "kc_lds", "kc_too_large"))}
    assert len(callers) == 8, usage  # kd_global, kd_lds<1>, kd_lds<4>, k_mixed, kc_global, kc_lds<1>, kc_lds<4>, kc_too_large
    assert all(v == 0 for v in callers.values()), callers
