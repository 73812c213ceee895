"""Device-side LZ4 API (include/nvcomp/device/lz4.hpp): kernels of tests/device_api/lz4_device_kernels.hip call it, on the
host emulation and on the MI355X (`backend`). The agreement rule: for every stream and capacity decompress() returns the
(status, byte count) pair nvcompBatchedLZ4DecompressAsync writes for the chunk, and where it succeeds the bytes liblz4
produces -- from global memory to global memory, into LDS, and from LDS into LDS. Every output slot is followed by 32
guard bytes of 0xA5 that must survive."""
import ctypes as C
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from nvcomp_amd import datasets
from nvcomp_amd._lib import NvcompStatus
from nvcomp_amd.batched import DeviceBatch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "device_api", "lz4_device_kernels.hip")
GOLDEN = os.path.join(REPO, "tests", "golden")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GUARD = 32
MODES = ("gg", "gl", "ll")  # global -> global, global -> LDS (copied out), LDS -> LDS (staged by the wave, copied out)
OK, BAD = int(NvcompStatus.Success), int(NvcompStatus.ErrorCannotDecompress)

_libs = {}


def kernels(backend, tmp_path_factory):
    """The test kernels built for the backend's tier (once per session)."""
    if backend.name not in _libs:
        d = tmp_path_factory.mktemp(f"lz4dev_{backend.name}")
        so = str(d / "lz4dev.so")
        if backend.name == "emu":
            import conftest

            conftest.emu_library()
            cmd = ["g++", "-O1", "-std=c++17", "-x", "c++", "-shared", "-fPIC", "-Itests/emu", "-Iinclude", SRC, "-o", so,
                   "-Ltests/emu", "-lnvcomp_emu", f"-Wl,-rpath,{REPO}/tests/emu"]
        else:
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(REPO, "include"), "-shared", "-fPIC",
                   SRC, "-o", so]
        r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        lib = C.CDLL(so)
        vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
        lib.lz4dev_global.argtypes = [vp, vp, vp, vp, vp, vp, sz, u, u, vp, vp]
        lib.lz4dev_lds.argtypes = [vp, vp, vp, vp, vp, vp, sz, u, u, u, u, u, vp, vp]
        lib.lz4dev_mixed.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, u, u, vp, vp]
        lib.lz4dev_sizes.argtypes = [vp, vp, vp, vp, sz, u, vp]
        for name in ("shared_bytes", "ring_bytes", "max_chunk_bytes"):
            getattr(lib, "lz4dev_" + name).restype = sz
        for name in ("lds_out_bytes", "lds_in_bytes"):
            getattr(lib, "lz4dev_" + name).restype = sz
            getattr(lib, "lz4dev_" + name).argtypes = [u]
        _libs[backend.name] = lib
    return _libs[backend.name]


@pytest.fixture
def k(backend, tmp_path_factory):
    return kernels(backend, tmp_path_factory)


# ---- block writer and expander (after _lz4_block / _lz4_expand of tests/test_lz4_decode.py) ----

def _len_bytes(n):
    b = bytearray()
    while n >= 255:
        b.append(255)
        n -= 255
    b.append(n)
    return b


class Block:
    """A hand-built LZ4 block. add() returns where the sequence's fields landed in the stream."""

    def __init__(self):
        self.stream = bytearray()
        self.out = bytearray()

    def add(self, lit, off, mlen, expand=True):
        lit = bytes(lit)
        pos = {"token": len(self.stream)}
        ll, ml = len(lit), mlen - 4
        self.stream.append((min(ll, 15) << 4) | min(ml, 15))
        pos["lit_ext"] = len(self.stream)
        if ll >= 15:
            self.stream += _len_bytes(ll - 15)
        pos["lit"] = len(self.stream)
        self.stream += lit
        pos["offset"] = len(self.stream)
        self.stream += bytes([off & 255, off >> 8])
        pos["match_ext"] = len(self.stream)
        if ml >= 15:
            self.stream += _len_bytes(ml - 15)
        pos["end"] = len(self.stream)
        if expand:
            self.out += lit
            for _ in range(mlen):
                self.out.append(self.out[-off])
        return pos

    def finish(self, tail):
        tail = bytes(tail)
        ll = len(tail)
        self.stream.append(min(ll, 15) << 4)
        if ll >= 15:
            self.stream += _len_bytes(ll - 15)
        self.stream += tail
        self.out += tail
        return np.frombuffer(bytes(self.stream), dtype=np.uint8).copy(), np.frombuffer(bytes(self.out), dtype=np.uint8).copy()


def block_of(seqs, tail):
    b = Block()
    for lit, off, mlen in seqs:
        b.add(lit, off, mlen)
    return b.finish(tail)


def rnd(rng, n):
    return rng.randint(0, 256, size=n).astype(np.uint8).tobytes()


# ---- running the kernels ----

def place(dev, chunks, aligns, pad=0, fill=None):
    """Chunks (or, with `fill`, empty slots of these sizes) in one slab, chunk i at an address that is aligns[i] mod 16,
    `pad` bytes of room behind each."""
    n = len(chunks)
    sizes = [c if fill is not None else c.size for c in chunks]
    offs, pos = [], 0
    for s, a in zip(sizes, aligns):
        pos = (pos + 15) // 16 * 16 + a
        offs.append(pos)
        pos += s + pad
    host = np.full(pos + 16, 0 if fill is None else fill, dtype=np.uint8)
    if fill is None:
        for c, o in zip(chunks, offs):
            host[o: o + c.size] = c
    slab = dev.upload(host)
    base = dev.ptr(slab)
    assert base % 16 == 0
    offs = np.asarray(offs, dtype=np.int64)
    ptrs = dev.upload((offs.astype(np.uint64) + np.uint64(base)).view(np.uint8)) if n else dev.upload(np.zeros(8, np.uint8))
    hs = np.asarray(sizes, dtype=np.uint64)
    return DeviceBatch(slab, ptrs, dev.upload(hs.view(np.uint8)) if n else dev.upload(np.zeros(8, np.uint8)), offs, hs, n)


def per_chunk(v, n):
    return [v] * n if isinstance(v, int) else list(v)


def block_for(k, mode, streams, caps):
    """Workgroups of 256 threads where a wave's share of the test kernel's LDS holds the chunk, of 64 otherwise."""
    if mode == "gg":
        return 256
    big = max(caps + [0]) > k.lz4dev_lds_out_bytes(256) or (mode == "ll" and max([s.size for s in streams] + [0]) > k.lz4dev_lds_in_bytes(256))
    return 64 if big else 256


def dev_decompress(backend, k, streams, caps, mode="gg", block=None, in_align=0, out_align=0, chunks_per_wave=1):
    """decompress() over a batch. gg: in_align / out_align place the chunks in global memory (an int or one per chunk);
    gl, ll: the global placement is 16-byte aligned and the ints place the stream (ll) and the output in LDS. Returns
    (whole output slots, actual sizes, statuses); the guards behind every slot and around the scratch areas are asserted."""
    d = backend.dev
    n = len(streams)
    caps = [int(c) for c in caps]
    if block is None:
        block = block_for(k, mode, streams, caps)
    gg = mode == "gg"
    src = place(d, streams, per_chunk(in_align, n) if gg else [0] * n)
    out = place(d, [c + GUARD for c in caps], per_chunk(out_align, n) if gg else [0] * n, fill=0xA5)
    capd = d.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    actual = d.upload(np.full(n, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
    status = d.upload(np.full(n, -1, dtype=np.int32).view(np.uint8))
    flags = d.upload(np.zeros(4, dtype=np.uint8))
    waves = -(-n // chunks_per_wave)
    grid = max(1, -(-waves // (block // 64)))
    p = d.ptr
    if gg:
        rc = k.lz4dev_global(p(src.ptrs), p(src.sizes), p(out.ptrs), p(capd), p(actual), p(status), n, block, grid, p(flags), d.stream())
    else:
        rc = k.lz4dev_lds(p(src.ptrs), p(src.sizes), p(out.ptrs), p(capd), p(actual), p(status), n, 1 if mode == "ll" else 0,
                          int(in_align), int(out_align), block, grid, p(flags), d.stream())
    assert rc == 0
    d.synchronize()
    assert d.download(flags).view(np.uint32)[0] == 0, "a guard around a scratch area or behind an output in LDS changed"
    host = d.download(out.slab)
    outs = []
    for o, c in zip(out.offsets, caps):
        o = int(o)
        outs.append(host[o: o + c].copy())
        assert (host[o + c: o + c + GUARD] == 0xA5).all(), "a write past the output capacity"
    st = d.download(status).view(np.int32)[:n].copy()
    assert (st != -2).all(), "the test kernel's LDS cannot hold this chunk: a bug in this test"
    return outs, d.download(actual).view(np.uint64)[:n].copy(), st


def dev_sizes(backend, k, streams, block=256):
    d = backend.dev
    n = len(streams)
    src = place(d, streams, [i % 16 for i in range(n)])
    sizes = d.upload(np.full(n, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
    status = d.upload(np.full(n, -1, dtype=np.int32).view(np.uint8))
    assert k.lz4dev_sizes(d.ptr(src.ptrs), d.ptr(src.sizes), d.ptr(sizes), d.ptr(status), n, block, d.stream()) == 0
    d.synchronize()
    return d.download(sizes).view(np.uint64)[:n].copy(), d.download(status).view(np.int32)[:n].copy()


def check_sizes(backend, k, streams):
    """decompressed_size() == nvcompBatchedLZ4GetDecompressSizeAsync, and its status says whether that is a refusal."""
    want = backend.codec("LZ4").get_decompress_size(streams)
    got, st = dev_sizes(backend, k, streams)
    assert got.tolist() == want.tolist()
    assert all(s == OK or g == 0 for s, g in zip(st, got)) and set(st.tolist()) <= {OK, BAD}


def agree(backend, k, streams, caps, expect=None, modes=MODES, sizes=True, **kw):
    """The agreement rule over a batch, through every address combination in `modes`. expect: the original bytes of
    chunks that must decode (None entries: whatever the batched decoder says). Returns the batched statuses."""
    caps = [int(c) for c in caps]
    b_outs, b_actual, b_status = backend.codec("LZ4").decompress(streams, caps)
    if expect is not None:
        for i, e in enumerate(expect):
            if e is not None:
                assert b_status[i] == OK and b_actual[i] == e.size and np.array_equal(b_outs[i][: e.size], e), f"batched decoder, chunk {i}"
    for mode in modes:
        outs, actual, status = dev_decompress(backend, k, streams, caps, mode=mode, **kw)
        assert status.tolist() == b_status.tolist(), (mode, np.flatnonzero(status != b_status)[:10])
        assert actual.tolist() == b_actual.tolist(), (mode, np.flatnonzero(actual != b_actual)[:10])
        for i, (o, bo) in enumerate(zip(outs, b_outs)):
            if status[i] == OK:
                n = int(actual[i])
                assert np.array_equal(o[:n], bo[:n]), f"{mode}: chunk {i} differs from the batched decoder's bytes"
                assert (o[n:] == 0xA5).all(), f"{mode}: chunk {i}: bytes behind the decoded size were written"
    if sizes:
        check_sizes(backend, k, streams)
    return b_status


def liblz4(oracle, chunks, hc=0):
    if oracle.have_ref():
        return [oracle.ref_lz4_compress(c, hc) for c in chunks]
    return [oracle.lz4_compress(c) for c in chunks]


def oracle_agrees(oracle, stream, want):
    """liblz4's decoder (LZ4_decompress_safe where installed, the port otherwise) on a hand-built block: pins the writer."""
    rc, ref = (oracle.ref_lz4_decompress if oracle.have_ref() else oracle.lz4_decompress)(stream, want.size)
    assert rc == 0 and np.array_equal(ref, want), "the block writer of this test is wrong"


# ---- 1. degenerate chunks ----

def test_degenerate_chunks(backend, oracle, k):
    rng = np.random.RandomState(1)
    streams, wants = [np.zeros(0, np.uint8), np.zeros(1, np.uint8)], [np.zeros(0, np.uint8), np.zeros(0, np.uint8)]
    for n in (1, 14, 15, 16, 269, 270, 271, 15 + 255 * 3):
        s, w = block_of([], rnd(rng, n))
        oracle_agrees(oracle, s, w)
        streams.append(s)
        wants.append(w)
    for caps in ([w.size for w in wants], [w.size + 5 for w in wants]):
        for block in (64, 256):
            st = agree(backend, k, streams, caps, expect=wants, block=block)
            assert (st == OK).all()


# ---- 2. lengths and offsets ----

MATCH_LENGTHS = (4, 18, 19, 20, 273, 274, 275, 4 + 15 + 3 * 255 + 7)  # the last: four length bytes
OFFSETS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 65535)


def test_match_lengths_and_offsets(backend, oracle, k):
    rng = np.random.RandomState(2)
    streams, wants = [], []
    for off in (37, 350):  # overlapping for most lengths / not for the short ones
        b = Block()
        b.add(rnd(rng, 400), 400, 4)
        for mlen in MATCH_LENGTHS:
            b.add(rnd(rng, 3), off, mlen)
        s, w = b.finish(rnd(rng, 13))
        streams.append(s)
        wants.append(w)
    for off in OFFSETS:
        if off >= 5:  # a match is 4 bytes at least: no length < offset below 5
            s, w = block_of([(rnd(rng, off + 5), off, off - 1 if off <= 65 else 300), (rnd(rng, 2), off, 4)], rnd(rng, 13))
            streams.append(s)
            wants.append(w)
        if off < 65535:
            s, w = block_of([(rnd(rng, off + 5), off, off + 7), (rnd(rng, 2), off, 2 * off + 70)], rnd(rng, 13))
            streams.append(s)
            wants.append(w)
    s, w = block_of([(rnd(rng, 10), 10, 25), (b"", 35, 35)], rnd(rng, 13))  # sources that start exactly at out[0]
    streams.append(s)
    wants.append(w)
    for s, w in zip(streams, wants):
        oracle_agrees(oracle, s, w)
    st = agree(backend, k, streams, [w.size for w in wants], expect=wants)
    assert (st == OK).all()
    # offset 65 535 overlapping: 128 KiB of output, more than a CU's LDS share holds -- global memory only
    s, w = block_of([(rnd(rng, 65535), 65535, 65535 + 9)], rnd(rng, 13))
    oracle_agrees(oracle, s, w)
    assert (agree(backend, k, [s], [w.size], expect=[w], modes=("gg",)) == OK).all()


# ---- 3. batch and ring boundaries ----

def small_sequences(rng, b, count):
    for _ in range(count):
        produced = len(b.out)
        lit = rnd(rng, rng.randint(0, 7) if produced else 5)
        produced += len(lit)
        b.add(lit, int(rng.randint(1, min(produced, 300) + 1)), int(rng.randint(4, 21)))


def test_sequence_counts_around_a_batch(backend, oracle, k):
    rng = np.random.RandomState(3)
    streams, wants = [], []
    for count in (63, 64, 65, 127, 128, 129):
        b = Block()
        small_sequences(rng, b, count)
        s, w = b.finish(rnd(rng, 13))
        streams.append(s)
        wants.append(w)
    # the chain: 1 literal + a match of 4 that starts 1 back of the previous sequence's last byte (offset 3, overlapping):
    # every match needs the one before it, a round resolves one lane
    b = Block()
    b.add(rnd(rng, 4), 2, 4)
    for _ in range(200):
        b.add(rnd(rng, 1), 3, 4)
    s, w = b.finish(rnd(rng, 13))
    streams.append(s)
    wants.append(w)
    for s, w in zip(streams, wants):
        oracle_agrees(oracle, s, w)
    for block in (64, 256):
        assert (agree(backend, k, streams, [w.size for w in wants], expect=wants, block=block) == OK).all()


def straddle_block(rng, target, field, shift):
    """A block in which `field` of one sequence lies across stream index `target` (a multiple of the staging ring's
    size): byte target - shift of the stream is the field's first. A literal run in front of it is sized to place it."""
    import copy

    prefix = Block()
    small_sequences(rng, prefix, 40)
    while len(prefix.stream) < target - 900:
        small_sequences(rng, prefix, 10)
    special = {"token": (rnd(rng, 3), 2, 6), "lit_ext": (rnd(rng, 15 + 2 * 255 + 9), 5, 8), "lit": (rnd(rng, 20), 9, 5),
               "lit_wave": (rnd(rng, 60), 9, 5), "offset": (rnd(rng, 2), 260, 9), "match_ext": (rnd(rng, 1), 7, 4 + 15 + 3 * 255 + 1),
               "match_ext_long": (rnd(rng, 1), 7, 4 + 15 + 9 * 255 + 1)}[field]
    key = {"lit_wave": "lit", "match_ext_long": "match_ext"}.get(field, field)
    filler = rnd(rng, 1200)
    for pad in range(20, 1200):
        b = copy.deepcopy(prefix)
        b.add(filler[:pad], 1, 4)
        if b.add(*special)[key] == target - shift:
            small_sequences(rng, b, 30)
            return b.finish(rnd(rng, 13))
    raise AssertionError("no padding places the field: a bug in this test")


def test_fields_across_the_end_of_the_staging_ring(backend, oracle, k):
    ring = int(k.lz4dev_ring_bytes())
    assert ring + 16 == k.lz4dev_shared_bytes() and ring % 16 == 0
    rng = np.random.RandomState(4)
    streams, wants = [], []
    for target in (ring, 2 * ring):
        for field, shifts in (("token", (0, 1)), ("lit_ext", (1, 2)), ("lit", (7,)), ("lit_wave", (33,)), ("offset", (1,)),
                              ("match_ext", (1, 2)), ("match_ext_long", (4,))):
            for shift in shifts:
                s, w = straddle_block(rng, target, field, shift)
                oracle_agrees(oracle, s, w)
                streams.append(s)
                wants.append(w)
    # stream index = ring position for a stream at a 16-byte aligned address (the default placement), global or LDS
    assert (agree(backend, k, streams, [w.size for w in wants], expect=wants) == OK).all()


# ---- 4. alignments ----

def test_every_alignment(backend, oracle, k):
    mix = datasets.silesia_style(4 * 65536, 5)
    chunk = mix[65536: 65536 + 1500].copy()
    for hc in (0, 12):
        (s,) = liblz4(oracle, [chunk], hc)
        pairs = [(a, b) for a in range(16) for b in range(16)]
        outs, actual, status = dev_decompress(backend, k, [s] * len(pairs), [chunk.size] * len(pairs), mode="gg",
                                              in_align=[a for a, _ in pairs], out_align=[b for _, b in pairs])
        assert (status == OK).all() and (actual == chunk.size).all()
        assert all(np.array_equal(o, chunk) for o in outs)
        for a in range(16):
            for mode, ia, oa in (("gl", 0, a), ("ll", a, 0), ("ll", a, (5 * a + 3) % 16)):
                outs, actual, status = dev_decompress(backend, k, [s] * 4, [chunk.size] * 4, mode=mode, in_align=ia, out_align=oa)
                assert (status == OK).all() and (actual == chunk.size).all() and all(np.array_equal(o, chunk) for o in outs), (mode, ia, oa)


# ---- 5. liblz4 streams ----

@pytest.mark.parametrize("name", ["text", "table", "float_csv", "float32", "int32", "lowcard", "zeros", "noise"])
def test_classes_small(backend, oracle, k, name):
    data = datasets.CLASSES[name](65536 + 777, 1)
    chunks = datasets.split_chunks(data)
    for hc in (0, 12):
        comp = liblz4(oracle, chunks, hc)
        assert (agree(backend, k, comp, [c.size for c in chunks], expect=chunks) == OK).all()


def test_ragged_sizes(backend, oracle, k):
    rng = np.random.RandomState(7)
    sizes = [1, 2, 3, 4, 5, 11, 12, 13, 14, 15, 16, 17, 31, 63, 64, 65, 255, 256, 257, 1000, 4095, 4097, 16384, 40001, 65535, 65536]
    base = datasets.text(70000, 9)
    chunks = [base[rng.randint(0, 2000):][:s].copy() for s in sizes]
    for hc in (0, 12):
        comp = liblz4(oracle, chunks, hc)
        assert (agree(backend, k, comp, sizes, expect=chunks) == OK).all()


MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))


@pytest.mark.parametrize("kind", ["lz4_default", "lz4_hc12"])
def test_golden_vectors(backend, k, kind):
    comp, recs = [], []
    for entry in MANIFEST["files"].values():
        for rec in entry["chunks"]:
            comp.append(np.fromfile(os.path.join(GOLDEN, rec["streams"][kind]["file"]), dtype=np.uint8))
            recs.append(rec)
    caps = [r["bytes"] for r in recs]
    for mode in MODES:
        outs, actual, status = dev_decompress(backend, k, comp, caps, mode=mode)
        assert (status == OK).all() and actual.tolist() == caps
        for o, r in zip(outs, recs):
            assert hashlib.sha256(o.tobytes()).hexdigest() == r["sha256"]
    check_sizes(backend, k, comp)


def test_one_chunk_of_the_largest_size(backend, oracle, k):
    """kMaxChunkBytes, global destination: text, so that every path of the decoder runs far into the chunk."""
    n = int(k.lz4dev_max_chunk_bytes())
    assert n == 1 << 24
    if backend.name == "emu":
        # the emulated wave decodes a megabyte of text in seconds, not sixteen: the text is the card's to run; here a run of
        # zeros of that size (one match with a length field of 65 793 bytes) stands in
        chunks = [np.zeros(n, np.uint8)]
    else:
        chunks = [datasets.text(n, 3), np.zeros(n, np.uint8)]
    comp = liblz4(oracle, chunks)
    assert (agree(backend, k, comp, [n] * len(chunks), expect=chunks, modes=("gg",)) == OK).all()


# ---- launch shapes ----

def test_mixed_workgroup(backend, oracle, k):
    """Three waves of every workgroup decode chunks of different kinds while the fourth does not call at all: the calls
    contain no workgroup barrier."""
    d = backend.dev
    count = 6 if backend.name == "emu" else 150
    grid = -(-count // 3)
    iters = 2000
    gens = sorted(datasets.CLASSES)
    chunks = [np.ascontiguousarray(datasets.CLASSES[gens[i % len(gens)]](3000 + 997 * (i % 5), i)).view(np.uint8).reshape(-1).copy()
              for i in range(count)]
    comp = liblz4(oracle, chunks)
    caps = [c.size for c in chunks]
    src = place(d, comp, [i % 16 for i in range(count)])
    out = place(d, [c + GUARD for c in caps], [(3 * i) % 16 for i in range(count)], fill=0xA5)
    capd = d.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    actual = d.upload(np.zeros(count, dtype=np.uint64).view(np.uint8))
    status = d.upload(np.full(count, -1, dtype=np.int32).view(np.uint8))
    side = d.upload(np.zeros(grid * 64, dtype=np.uint32).view(np.uint8))
    flags = d.upload(np.zeros(4, dtype=np.uint8))
    p = d.ptr
    assert k.lz4dev_mixed(p(src.ptrs), p(src.sizes), p(out.ptrs), p(capd), p(actual), p(status), count, p(side), iters, grid,
                          p(flags), d.stream()) == 0
    d.synchronize()
    assert d.download(flags).view(np.uint32)[0] == 0
    assert (d.download(status).view(np.int32)[:count] == OK).all()
    assert d.download(actual).view(np.uint64)[:count].tolist() == caps
    host = d.download(out.slab)
    for o, c in zip(out.offsets, chunks):
        assert np.array_equal(host[int(o): int(o) + c.size], c) and (host[int(o) + c.size: int(o) + c.size + GUARD] == 0xA5).all()
    x = np.arange(1, grid * 64 + 1, dtype=np.uint32)
    for _ in range(iters):
        x ^= x << np.uint32(13)
        x ^= x >> np.uint32(17)
        x ^= x << np.uint32(5)
    assert np.array_equal(d.download(side).view(np.uint32)[: x.size], x)


@pytest.mark.parametrize("block", [64, 256])
def test_a_wave_reuses_its_scratch_area(backend, oracle, k, block):
    """Every wave decodes two chunks one after the other, a refused one among them."""
    count = 16 if backend.name == "emu" else 300
    chunks = [datasets.table_rows(2000 + 501 * (i % 7), i) for i in range(count)]
    comp = liblz4(oracle, chunks)
    comp[3] = comp[3][:-2]
    expect = [None if i == 3 else c for i, c in enumerate(chunks)]
    for mode in MODES:
        st = agree(backend, k, comp, [c.size for c in chunks], expect=expect, modes=(mode,), block=block, chunks_per_wave=2,
                   sizes=False)
        assert st[3] == BAD and (np.delete(st, 3) == OK).all()


# ---- 6. refusals ----

def test_capacities(backend, oracle, k):
    chunk = datasets.text(5000, 2)
    (s,) = liblz4(oracle, [chunk])
    big, want = block_of([(b"abcdefgh", 8, 3000)], b"0123456789abc")  # the match that does not fit is the whole wave's
    lit, lwant = block_of([], bytes(range(200)) * 3)
    streams = [s, s, s, big, big, big, lit, lit, lit]
    caps = [5000, 4999, 0, want.size, want.size - 1, 0, lwant.size, lwant.size - 1, 0]
    st = agree(backend, k, streams, caps, expect=[chunk, None, None, want, None, None, lwant, None, None])
    assert st.tolist() == [OK, BAD, BAD] * 3


def forty_byte_block(rng):
    """Two sequences, a length byte of either kind, and twelve final literals (liblz4 wants the last match that far from
    the end)."""
    b = Block()
    b.add(rnd(rng, 4), 3, 7)
    b.add(rnd(rng, 15), 10, 19)
    s, w = b.finish(rnd(rng, 12))
    assert s.size == 40
    return s, w


def test_truncation_and_trailing_bytes(backend, oracle, k):
    rng = np.random.RandomState(8)
    s, w = forty_byte_block(rng)
    oracle_agrees(oracle, s, w)
    streams = [s] + [s[:n].copy() for n in range(1, 40)] + [np.concatenate([s, np.array(t, np.uint8)]) for t in ([0], [7], [0, 0], [1, 9])]
    st = agree(backend, k, streams, [w.size + 64] * len(streams), expect=[w] + [None] * (len(streams) - 1))
    assert st[0] == OK
    # a prefix that ends behind a sequence's literals is a block of its own (its last sequence: literals only); every
    # other prefix, and every block with bytes behind its final literal run, is refused
    assert (st[-4:] == BAD).all() and (st[1:40] == BAD).sum() >= 30


def wrapped_source_blocks(rng):
    """offset = position + 1 and friends: the match's source starts in front of out[0]."""
    out = []
    for data in ("constant", "random"):
        for pre, extra, mlen in ((40, 1, 4), (40, 1, 100), (40, 3, 50), (40, 100, 30), (40, 100, 300), (0, 1, 20), (0, 65535, 8),
                                 (3000, 40, 100), (3000, 3, 50), (3000, 100, 300)):
            b = Block()
            lit = bytes(pre) if data == "constant" else rnd(rng, pre)
            if pre > 100:  # behind a period-1 run, like the sequences of a run batch
                b.add(lit[:8], 1 if data == "constant" else 8, pre - 8)
                b.add(b"", len(b.out) + extra, mlen, expand=False)
            else:
                b.add(lit, pre + extra, mlen, expand=False)
            s, _ = b.finish(bytes(13) if data == "constant" else rnd(rng, 13))
            out.append(s)
    return out


def test_offsets_in_front_of_the_output(backend, oracle, k):
    rng = np.random.RandomState(9)
    streams = wrapped_source_blocks(rng)
    b = Block()
    at = b.add(rnd(rng, 20), 5, 6)["offset"]
    b.add(rnd(rng, 3), 1, 4)
    s, _ = b.finish(rnd(rng, 13))
    s[at] = 0  # the first sequence's offset: 5 -> 0
    streams.append(s)
    # a match length field that runs to the end of the input
    b = Block()
    b.add(rnd(rng, 5), 2, 4 + 15 + 255 * 3)
    s, _ = b.finish(b"")
    streams.append(s[:-2].copy())  # ... 255 255 255 | (the field's last byte and the final token are gone)
    streams.append(np.concatenate([s[:-2], np.full(300, 255, np.uint8)]))
    for s in streams:
        rc, _ = oracle.lz4_decompress(s, 70000)
        assert rc != 0, "liblz4 accepts the block: a bug in this test"
    st = agree(backend, k, streams, [70000 if s.size < 400 else 4000 for s in streams], modes=("gg",))
    assert (st == BAD).all()
    st = agree(backend, k, streams, [16000] * len(streams), modes=("gl", "ll"), sizes=False)
    assert (st == BAD).all()


# ---- 7. mutation fuzz ----

def test_single_byte_mutations(backend, oracle, k):
    """2 000 single-byte mutations over twenty blocks of 200-600 bytes: status, byte count and (on success) bytes equal
    the batched decoder's for every one of them."""
    rng = np.random.RandomState(1234)
    blocks = []
    gens = [g for g in sorted(datasets.CLASSES) if g not in ("zeros",)]
    for i in range(10):  # liblz4, default and HC: the shortest prefix of a class that compresses to 250 bytes or more
        raw = np.ascontiguousarray(datasets.CLASSES[gens[i % len(gens)]](65536, i)).view(np.uint8).reshape(-1)
        n = 300
        while liblz4(oracle, [raw[:n]], 12 if i % 2 else 0)[0].size < 250:
            n += 50
        (s,) = liblz4(oracle, [raw[:n]], 12 if i % 2 else 0)
        assert 200 <= s.size <= 600
        blocks.append((s, n))
    while len(blocks) < 20:
        b = Block()
        small_sequences(rng, b, int(rng.randint(40, 90)))
        if len(blocks) % 3 == 0:
            b.add(rnd(rng, 40), 17, 4 + 15 + 255 + 3)
        s, w = b.finish(rnd(rng, 13))
        if 200 <= s.size <= 600:
            blocks.append((s, w.size))
    streams, caps = [], []
    for i in range(2000):
        s, n = blocks[i % 20]
        m = s.copy()
        at = int(rng.randint(0, m.size))
        m[at] ^= np.uint8(rng.randint(1, 256))
        streams.append(m)
        caps.append(n + (0 if i % 4 else 40))
    for lo in range(0, 2000, 500):
        agree(backend, k, streams[lo: lo + 500], caps[lo: lo + 500], modes=("gg", "ll") if lo else MODES)


# ---- 9. the last byte in front of an unmapped page (emulator only) ----

def test_nothing_is_touched_behind_the_stream_or_the_capacity(emu, oracle, tmp_path_factory):
    """Host memory: the stream's last byte, then the output's, is the last byte in front of a PROT_NONE page, or lies one,
    two, three bytes in front of it. A read or write past the end is a segmentation fault. (Never on the card: there the
    guard bytes stand in.)"""
    from hlif_container import guarded_mapping

    k = kernels(emu, tmp_path_factory)
    chunk = datasets.text(3000, 4)
    (s,) = liblz4(oracle, [chunk])
    base, span = guarded_mapping(2)
    room = (C.c_uint8 * span).from_address(base)
    for back in (0, 1, 2, 3):
        # the stream against the page
        at = span - back - s.size
        C.memmove(base + at, s.ctypes.data, s.size)
        out = np.full(chunk.size + GUARD, 0xA5, dtype=np.uint8)
        ptrs = np.array([base + at], dtype=np.uint64)
        sizes = np.array([s.size], dtype=np.uint64)
        optrs = np.array([out.ctypes.data], dtype=np.uint64)
        caps = np.array([chunk.size], dtype=np.uint64)
        actual, status, flags = np.zeros(1, np.uint64), np.full(1, -1, np.int32), np.zeros(1, np.uint32)
        assert k.lz4dev_global(ptrs.ctypes.data, sizes.ctypes.data, optrs.ctypes.data, caps.ctypes.data, actual.ctypes.data,
                               status.ctypes.data, 1, 64, 1, flags.ctypes.data, None) == 0
        assert status[0] == OK and actual[0] == chunk.size and np.array_equal(out[: chunk.size], chunk) and flags[0] == 0
        got = np.zeros(1, np.uint64)
        assert k.lz4dev_sizes(ptrs.ctypes.data, sizes.ctypes.data, got.ctypes.data, status.ctypes.data, 1, 64, None) == 0
        assert got[0] == chunk.size
        # the output against the page, the capacity exact
        src = s.copy()
        ptrs = np.array([src.ctypes.data], dtype=np.uint64)
        oat = span - back - chunk.size
        C.memset(base + oat, 0xA5, chunk.size)
        optrs = np.array([base + oat], dtype=np.uint64)
        assert k.lz4dev_global(ptrs.ctypes.data, sizes.ctypes.data, optrs.ctypes.data, caps.ctypes.data, actual.ctypes.data,
                               status.ctypes.data, 1, 64, 1, flags.ctypes.data, None) == 0
        assert status[0] == OK and actual[0] == chunk.size and flags[0] == 0
        assert np.array_equal(np.frombuffer(room, dtype=np.uint8, count=chunk.size, offset=oat), chunk)


# ---- 10. the header's promises ----

def test_header_is_self_contained(tmp_path):
    if shutil.which(HIPCC) is None and not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")
    only = tmp_path / "only.hip"
    only.write_text("#include <nvcomp/device/lz4.hpp>\n")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(REPO, "include"),
                        "-c", str(only), "-o", str(tmp_path / "only.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_not_in_the_umbrella_headers():
    for umbrella in ("nvcomp.h", "nvcomp.hpp"):
        r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(REPO, "include"), "-I",
                            "/opt/rocm/include", "-M", "-x", "c++", os.path.join(REPO, "include", umbrella)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "nvcomp/device" not in r.stdout and "lz4_core" not in r.stdout


@pytest.mark.gpu
def test_example_on_gpu():
    exe = os.path.join(REPO, "examples", "bin", "lz4_device_example")
    r = subprocess.run(["make", "-C", "examples", exe], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "PASSED" in r.stdout
