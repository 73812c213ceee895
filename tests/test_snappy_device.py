"""Device-side Snappy API (include/nvcomp/device/snappy.hpp), the decoder: kernels of
tests/device_api/snappy_device_kernels.hip call it, on the host emulation and on the MI355X (`backend`). Every check is
three-way: for every stream and capacity decompress() returns the (status, byte count) pair
nvcompBatchedSnappyDecompressAsync writes for the chunk, and both agree with the C restatement of the format
(oracle.snappy_decompress; snappy::RawUncompress where the reference build is there) on whether the stream decodes and on
its bytes -- from global memory to global memory, into LDS, and from LDS into LDS. Every output slot is followed by 32 guard
bytes of 0xA5 that must survive, and nothing is written at or behind the decoded size."""
import copy
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
SRC = os.path.join(REPO, "tests", "device_api", "snappy_device_kernels.hip")
GOLDEN = os.path.join(REPO, "tests", "golden")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GUARD = 32
MODES = ("gg", "gl", "ll")  # global -> global, global -> LDS (copied out), LDS -> LDS (staged by the wave, copied out)
OK, BAD = int(NvcompStatus.Success), int(NvcompStatus.ErrorCannotDecompress)
LIT_SHORT = 32  # literal elements above this are copied by the whole wave (snappy_core.hpp: kLitShort)

_libs = {}


def kernels(backend, tmp_path_factory):
    """The test kernels built for the backend's tier (once per session; the compressor's tests use the same library)."""
    if backend.name not in _libs:
        d = tmp_path_factory.mktemp(f"snpdev_{backend.name}")
        so = str(d / "snpdev.so")
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
        lib.snpdev_global.argtypes = [vp, vp, vp, vp, vp, vp, sz, u, u, vp, vp]
        lib.snpdev_lds.argtypes = [vp, vp, vp, vp, vp, vp, sz, u, u, u, u, u, vp, vp]
        lib.snpdev_mixed.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, sz, vp, u, u, vp, vp]
        lib.snpdev_sizes.argtypes = [vp, vp, vp, vp, sz, u, vp]
        lib.snpcmp_global.argtypes = [vp, vp, vp, vp, sz, u, u, u, vp, vp]
        lib.snpcmp_lds.argtypes = [vp, vp, vp, vp, sz, u, u, u, u, u, u, vp, vp]
        lib.snpcmp_too_large.argtypes = [vp, sz, vp, vp, vp, vp]
        for name in ("snpdev_shared_bytes", "snpdev_ring_bytes", "snpdev_max_chunk_bytes", "snpcmp_shared_bytes", "snpcmp_step_bytes"):
            getattr(lib, name).restype = sz
        for name in ("snpdev_lds_out_bytes", "snpdev_lds_in_bytes", "snpcmp_lds_in_bytes"):
            getattr(lib, name).restype = sz
            getattr(lib, name).argtypes = [u]
        lib.snpcmp_max_compressed_bytes.restype = sz
        lib.snpcmp_max_compressed_bytes.argtypes = [sz]
        _libs[backend.name] = lib
    return _libs[backend.name]


@pytest.fixture
def k(backend, tmp_path_factory):
    return kernels(backend, tmp_path_factory)


# ---- stream writer and expander ----

def varint(n):
    out = bytearray()
    while n >= 128:
        out.append((n & 127) | 128)
        n >>= 7
    out.append(n)
    return bytes(out)


class Stream:
    """A hand-built Snappy stream. lit() / copy() return where the element's fields landed among the elements (finish()
    says how long the preamble in front of them is)."""

    def __init__(self):
        self.el = bytearray()
        self.out = bytearray()
        self.count = 0

    def lit(self, data, nb=None):
        """A literal element; nb: the number of length bytes (None: the shortest spelling)."""
        data = bytes(data)
        m = len(data) - 1
        assert m >= 0
        if nb is None:
            nb = 0 if m < 60 else 1 if m < 1 << 8 else 2 if m < 1 << 16 else 3 if m < 1 << 24 else 4
        pos = {"tag": len(self.el)}
        if nb == 0:
            assert m < 60
            self.el.append(m << 2)
        else:
            assert m < 1 << (8 * nb)
            self.el.append((59 + nb) << 2)
            self.el += m.to_bytes(nb, "little")
        pos["lit"] = len(self.el)
        self.el += data
        pos["end"] = len(self.el)
        self.out += data
        self.count += 1
        return pos

    def copy(self, kind, off, n, expand=True):
        pos = {"tag": len(self.el), "offset": len(self.el) + 1}
        if kind == 1:
            assert 4 <= n <= 11 and off < 2048
            self.el += bytes([1 | ((n - 4) << 2) | ((off >> 8) << 5), off & 255])
        else:
            assert 1 <= n <= 64 and kind in (2, 4)
            self.el.append((2 if kind == 2 else 3) | ((n - 1) << 2))
            self.el += off.to_bytes(kind, "little")
        pos["end"] = len(self.el)
        if expand:
            for _ in range(n):
                self.out.append(self.out[-off])
        self.count += 1
        return pos

    def finish(self, declared=None):
        pre = varint(len(self.out) if declared is None else declared)
        s = np.frombuffer(pre + bytes(self.el), dtype=np.uint8).copy()
        return s, np.frombuffer(bytes(self.out), dtype=np.uint8).copy()

    def pre(self):
        return len(varint(len(self.out)))


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
    big = max(caps + [0]) > k.snpdev_lds_out_bytes(256) or (mode == "ll" and max([s.size for s in streams] + [0]) > k.snpdev_lds_in_bytes(256))
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
        rc = k.snpdev_global(p(src.ptrs), p(src.sizes), p(out.ptrs), p(capd), p(actual), p(status), n, block, grid, p(flags), d.stream())
    else:
        rc = k.snpdev_lds(p(src.ptrs), p(src.sizes), p(out.ptrs), p(capd), p(actual), p(status), n, 1 if mode == "ll" else 0,
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
    assert k.snpdev_sizes(d.ptr(src.ptrs), d.ptr(src.sizes), d.ptr(sizes), d.ptr(status), n, block, d.stream()) == 0
    d.synchronize()
    return d.download(sizes).view(np.uint64)[:n].copy(), d.download(status).view(np.int32)[:n].copy()


def check_sizes(backend, k, streams):
    """decompressed_size() == nvcompBatchedSnappyGetDecompressSizeAsync; a refusal reports 0."""
    want = backend.codec("Snappy").get_decompress_size(streams)
    got, st = dev_sizes(backend, k, streams)
    assert got.tolist() == want.tolist()
    assert all(s == OK or g == 0 for s, g in zip(st, got)) and set(st.tolist()) <= {OK, BAD}


def agree(backend, oracle, k, streams, caps, expect=None, modes=MODES, sizes=True, **kw):
    """The three-way rule over a batch, through every address combination in `modes`: the device API against the batched
    decoder (status and size), both against the oracle (whether the stream decodes, and its bytes). expect: the original
    bytes of chunks that must decode. Returns the batched statuses."""
    caps = [int(c) for c in caps]
    b_outs, b_actual, b_status = backend.codec("Snappy").decompress(streams, caps)
    refs = []
    for i, (s, cap) in enumerate(zip(streams, caps)):
        rc, ref = oracle.snappy_decompress(s, cap)
        refs.append(ref if rc == 0 else None)
        if rc == 0:
            assert b_status[i] == OK and b_actual[i] == ref.size and np.array_equal(b_outs[i][: ref.size], ref), f"batched decoder, chunk {i}"
        else:
            assert b_status[i] == BAD and b_actual[i] == 0, f"batched decoder, chunk {i}"
        if expect is not None and expect[i] is not None:
            assert rc == 0 and np.array_equal(ref, expect[i]), f"chunk {i}: the stream writer of this test is wrong"
    for mode in modes:
        outs, actual, status = dev_decompress(backend, k, streams, caps, mode=mode, **kw)
        assert status.tolist() == b_status.tolist(), (mode, np.flatnonzero(status != b_status)[:10])
        assert actual.tolist() == b_actual.tolist(), (mode, np.flatnonzero(actual != b_actual)[:10])
        for i, o in enumerate(outs):
            if status[i] == OK:
                n = int(actual[i])
                assert np.array_equal(o[:n], refs[i]), f"{mode}: chunk {i} differs from the oracle's bytes"
                assert (o[n:] == 0xA5).all(), f"{mode}: chunk {i}: bytes behind the decoded size were written"
    if sizes:
        check_sizes(backend, k, streams)
    return b_status


def libsnappy(oracle, chunks):
    if oracle.have_ref():
        return [oracle.ref_snappy_compress(c) for c in chunks]
    return [oracle.snappy_compress(c) for c in chunks]


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8).copy()


# ---- 1. degenerate streams ----

def test_degenerate_streams(backend, oracle, k):
    rng = np.random.RandomState(1)
    streams = [np.zeros(0, np.uint8), u8(b"\x00"), u8(varint(5)), u8(varint(300)), u8(varint(1 << 20))]
    wants = [None, np.zeros(0, np.uint8), None, None, None]
    for n in (1, 2, 3):
        s = Stream()
        s.lit(rnd(rng, n))
        st, w = s.finish()
        streams.append(st)
        wants.append(w)
    for caps in ([0 if w is None else w.size for w in wants], [64] * len(wants)):
        for block in (64, 256):
            st = agree(backend, oracle, k, streams, caps, expect=wants, block=block)
            assert st.tolist() == [BAD, OK, BAD, BAD, BAD, OK, OK, OK]


# ---- 2. element kinds and field boundaries ----

LITERAL_LENGTHS = (1, 59, 60, 61, 256, 257, 65536, 65537)
OFFSETS = (1, 2, 3, 4, 7, 8, 15, 16, 17, 63, 64, 65, 255, 256, 2047, 2048, 65535)
COPY_LENGTHS = (1, 2, 3, 4, 63, 64)


def test_literal_lengths_and_spellings(backend, oracle, k):
    rng = np.random.RandomState(2)
    streams, wants = [], []
    for n in LITERAL_LENGTHS:
        for after in (False, True):  # alone, and between two copies
            s = Stream()
            if after:
                s.lit(rnd(rng, 9))
                s.copy(2, 5, 7)
            s.lit(rnd(rng, n))
            if after:
                s.copy(1, 3, 4)
                s.lit(rnd(rng, 2))
            st, w = s.finish()
            streams.append(st)
            wants.append(w)
    # non-canonical spellings: more length bytes than the value needs, a four-byte field that holds 5
    for n, nb in ((5, 4), (5, 1), (6, 2), (1, 3), (60, 4), (300, 3), (300, 4), (33, 1), (32, 2)):
        s = Stream()
        s.lit(rnd(rng, 3))
        s.lit(rnd(rng, n), nb=nb)
        s.copy(2, n, 11)
        s.lit(rnd(rng, n), nb=nb)
        st, w = s.finish()
        streams.append(st)
        wants.append(w)
    caps = [w.size for w in wants]
    small = [i for i, c in enumerate(caps) if c <= k.snpdev_lds_out_bytes(64) - 2000]
    pick = lambda xs, idx: [xs[i] for i in idx]  # noqa: E731
    assert (agree(backend, oracle, k, pick(streams, small), pick(caps, small), expect=pick(wants, small)) == OK).all()
    assert (agree(backend, oracle, k, streams, caps, expect=wants, modes=("gg",)) == OK).all()


def test_copy_kinds_lengths_and_offsets(backend, oracle, k):
    rng = np.random.RandomState(3)
    streams, wants = [], []
    for off in OFFSETS:
        s = Stream()
        s.lit(rnd(rng, off + 3))
        for kind in (2, 4):
            for n in COPY_LENGTHS:
                s.copy(kind, off, n)
                s.lit(rnd(rng, 1 + n % 3))
        if off < 2048:
            for n in (4, 11):
                s.copy(1, off, n)
                s.copy(1, off, n)  # a train of two
                s.lit(rnd(rng, 2))
        s.copy(2 if len(s.out) < 65536 else 4, len(s.out), 64)  # the source starts exactly at out[0]
        st, w = s.finish()
        streams.append(st)
        wants.append(w)
    assert (agree(backend, oracle, k, streams, [w.size for w in wants], expect=wants) == OK).all()


def test_copy4_offsets_above_64k(backend, oracle, k):
    """One chunk of about 72 KiB: copy-4 at offsets 65 535, 65 536 and 70 000, overlapping nothing and each other."""
    rng = np.random.RandomState(4)
    s = Stream()
    s.lit(rnd(rng, 70000))
    for off in (65535, 65536, 70000):
        for n in (1, 4, 64):
            s.copy(4, off, n)
        s.copy(4, off, 64)
        s.copy(4, off, 64)
        s.lit(rnd(rng, 3))
    s.copy(4, len(s.out), 64)
    s.lit(rnd(rng, 40))
    s.copy(2, 65535, 64)
    st, w = s.finish()
    assert 70000 < w.size <= 73 * 1024
    assert (agree(backend, oracle, k, [st], [w.size], expect=[w]) == OK).all()
    # the same offsets one byte too far: in front of out
    bad = Stream()
    bad.lit(rnd(rng, 69999))
    bad.copy(4, 70000, 5, expand=False)
    bst, _ = bad.finish(declared=70004)
    assert (agree(backend, oracle, k, [bst], [70004], modes=("gg",)) == BAD).all()


# ---- 3. copy trains and batching ----

def test_copy_trains(backend, oracle, k):
    """Trains of 2, 3, 64 and 65 copies of one offset at periods 1, 2, 3, 4, 8 after a literal of the period's length --
    chains of dependent copies -- in every copy kind and at lengths that keep and break the period's phase."""
    rng = np.random.RandomState(5)
    streams, wants = [], []
    for period in (1, 2, 3, 4, 8):
        for cars in (2, 3, 64, 65):
            for kind, n in ((2, 64), (2, 7), (1, 11), (4, 1), (2, 3)):
                if kind == 1 and cars > 3:
                    continue
                s = Stream()
                s.lit(rnd(rng, period))
                for _ in range(cars):
                    s.copy(kind, period, n)
                s.lit(rnd(rng, 5))
                s.copy(2, period + 5, 9)  # a train behind a train, another offset
                s.copy(2, period, 64)
                s.copy(2, period, 13)
                st, w = s.finish()
                streams.append(st)
                wants.append(w)
    for block in (64, 256):
        assert (agree(backend, oracle, k, streams, [w.size for w in wants], expect=wants, block=block) == OK).all()


def small_elements(rng, s, count):
    """`count` tokens as the decoder batches them: a copy, or a short literal with the copy behind it."""
    for _ in range(count):
        if not s.out or rng.randint(0, 3):
            s.lit(rnd(rng, rng.randint(1, 8)))
        produced = len(s.out)
        off = int(rng.randint(1, min(produced, 300) + 1))
        kind = (1, 2, 4)[rng.randint(0, 3)]
        s.copy(kind, off, int(rng.randint(4, 12)) if kind == 1 else int(rng.randint(1, 30)))


def test_element_counts_around_a_batch(backend, oracle, k):
    rng = np.random.RandomState(6)
    streams, wants = [], []
    for count in (63, 64, 65, 127, 128, 129):
        for copies_only in (False, True):
            s = Stream()
            if copies_only:  # one literal, then `count - 1` copies: every copy a token of its own
                s.lit(rnd(rng, 20))
                for i in range(count - 1):
                    s.copy(2, 1 + (7 * i) % 20, 1 + i % 9)
            else:
                small_elements(rng, s, count)
            st, w = s.finish()
            streams.append(st)
            wants.append(w)
    # the chain: every copy starts one byte behind the start of the copy before it (offset 3, overlapping): a round
    # resolves one lane
    s = Stream()
    s.lit(rnd(rng, 4))
    s.copy(2, 2, 4)
    for _ in range(200):
        s.lit(rnd(rng, 1))
        s.copy(2, 3, 4)
    st, w = s.finish()
    streams.append(st)
    wants.append(w)
    for block in (64, 256):
        assert (agree(backend, oracle, k, streams, [w.size for w in wants], expect=wants, block=block) == OK).all()


def test_long_literals_at_the_whole_wave_threshold(backend, oracle, k):
    rng = np.random.RandomState(7)
    streams, wants = [], []
    for n in (LIT_SHORT - 1, LIT_SHORT, LIT_SHORT + 1, 2 * LIT_SHORT, 1023, 1024, 1025, 5000):
        s = Stream()
        s.lit(rnd(rng, 6))
        for _ in range(3):
            s.copy(2, 4, 9)
            s.lit(rnd(rng, n))
            s.copy(1 if n < 2048 else 2, n, 4)
            s.copy(2, n + 2, 30)
        st, w = s.finish()
        streams.append(st)
        wants.append(w)
    assert (agree(backend, oracle, k, streams, [w.size for w in wants], expect=wants) == OK).all()


# ---- 4. the end of the staging ring ----

def straddle_stream(rng, target, field, shift):
    """A stream in which `field` of one element starts at stream index target - shift (target: a multiple of the staging
    ring's size). A literal in front of it is sized to place it."""
    prefix = Stream()
    small_elements(rng, prefix, 40)
    while len(prefix.el) < target - 900:
        small_elements(rng, prefix, 10)
    filler = rnd(rng, 1200)

    def special(s):
        if field == "lit_len1":
            return s.lit(rnd(rng, 200))["tag"] + 1
        if field == "lit_len2":
            return s.lit(rnd(rng, 700))["tag"] + 1
        if field == "lit_len3":
            return s.lit(rnd(rng, 70), nb=3)["tag"] + 1
        if field == "lit_len4":
            return s.lit(rnd(rng, 5), nb=4)["tag"] + 1
        if field == "lit":
            return s.lit(rnd(rng, 20))["lit"]
        if field == "copy1":
            return s.copy(1, 9, 5)["offset"]
        if field == "copy2":
            return s.copy(2, 300, 40)["offset"]
        if field == "copy4":
            return s.copy(4, 260, 33)["offset"]
        if field == "fused":  # the copy behind a short literal: its tag is the field
            s.lit(rnd(rng, 7))
            return s.copy(2, 11, 20)["tag"]
        raise AssertionError(field)

    state = rng.get_state()
    pad = 300
    for _ in range(8):  # the padding's own length field and the preamble move with it: a few corrections settle it
        rng.set_state(state)
        s = copy.deepcopy(prefix)
        s.lit(filler[:pad])
        s.copy(2, 1, 4)
        at = special(s)
        small_elements(rng, s, 30)
        miss = target - shift - (at + s.pre())
        if miss == 0:
            return s.finish()
        pad += miss
        assert 61 <= pad <= 1200
    raise AssertionError("no padding places the field: a bug in this test")


def test_fields_across_the_end_of_the_staging_ring(backend, oracle, k):
    """A tag is the ring's last byte (shift 1) with its length or offset bytes behind the end; the field split 1/2/3 ways
    (shifts 1, 2, 3 from the field's first byte = shift 0)."""
    ring = int(k.snpdev_ring_bytes())
    assert ring + 16 == k.snpdev_shared_bytes() and ring % 16 == 0
    rng = np.random.RandomState(8)
    streams, wants = [], []
    for target in (ring, 2 * ring):
        for field, shifts in (("lit_len1", (0, 1)), ("lit_len2", (0, 1)), ("lit_len3", (0, 1, 2)), ("lit_len4", (0, 1, 2, 3)),
                              ("lit", (0, 7)), ("copy1", (0, 1)), ("copy2", (0, 1)), ("copy4", (0, 1, 2, 3)), ("fused", (0, 1, 2))):
            for shift in shifts if target == ring else shifts[-1:]:  # (the ring's end comes round: one split there)
                st, w = straddle_stream(rng, target, field, shift)
                streams.append(st)
                wants.append(w)
    # stream index = ring position for a stream at a 16-byte aligned address (the default placement), global or LDS
    assert (agree(backend, oracle, k, streams, [w.size for w in wants], expect=wants) == OK).all()


# ---- 5. alignments ----

def test_alignments(backend, oracle, k):
    mix = datasets.silesia_style(4 * 65536, 5)
    chunk = mix[65536: 65536 + 1500].copy()
    (s,) = libsnappy(oracle, [chunk])
    als = (0, 1, 3, 8, 15)
    pairs = [(a, b) for a in als for b in als]
    outs, actual, status = dev_decompress(backend, k, [s] * len(pairs), [chunk.size] * len(pairs), mode="gg",
                                          in_align=[a for a, _ in pairs], out_align=[b for _, b in pairs])
    assert (status == OK).all() and (actual == chunk.size).all()
    assert all(np.array_equal(o, chunk) for o in outs)
    for a, b in pairs:
        for mode in ("gl", "ll"):
            if mode == "gl" and a:
                continue  # (the stream's place in global memory is the gg case)
            outs, actual, status = dev_decompress(backend, k, [s] * 4, [chunk.size] * 4, mode=mode, in_align=a, out_align=b)
            assert (status == OK).all() and (actual == chunk.size).all() and all(np.array_equal(o, chunk) for o in outs), (mode, a, b)


# ---- 6. data and launch shapes ----

@pytest.mark.parametrize("name", sorted(datasets.CLASSES))
def test_classes_small(backend, oracle, k, name):
    data = np.ascontiguousarray(datasets.CLASSES[name](16384 + 777, 1)).view(np.uint8).reshape(-1)
    chunks = datasets.split_chunks(data, 8192)
    comp = libsnappy(oracle, chunks) + backend.codec("Snappy").compress(chunks)
    chunks = chunks + chunks
    assert (agree(backend, oracle, k, comp, [c.size for c in chunks], expect=chunks) == OK).all()


def test_ragged_sizes(backend, oracle, k):
    rng = np.random.RandomState(9)
    sizes = [1, 2, 3, 4, 5, 11, 12, 13, 15, 16, 17, 31, 59, 60, 61, 63, 64, 65, 255, 256, 257, 1000, 4095, 4097, 16384, 40001, 65535, 65536]
    base = datasets.text(70000, 9)
    chunks = [base[rng.randint(0, 2000):][:s].copy() for s in sizes]
    comp = libsnappy(oracle, chunks)
    assert (agree(backend, oracle, k, comp, sizes, expect=chunks) == OK).all()


MANIFEST = json.load(open(os.path.join(GOLDEN, "manifest.json")))


def test_golden_vectors(backend, k):
    comp, recs = [], []
    for entry in MANIFEST["files"].values():
        for rec in entry["chunks"]:
            comp.append(np.fromfile(os.path.join(GOLDEN, rec["streams"]["snappy"]["file"]), dtype=np.uint8))
            recs.append(rec)
    caps = [r["bytes"] for r in recs]
    for mode in MODES:
        outs, actual, status = dev_decompress(backend, k, comp, caps, mode=mode)
        assert (status == OK).all() and actual.tolist() == caps
        for o, r in zip(outs, recs):
            assert hashlib.sha256(o.tobytes()).hexdigest() == r["sha256"]
    check_sizes(backend, k, comp)


def test_one_chunk_of_the_largest_size(backend, oracle, k):
    """kMaxChunkBytes, global destination: text on the card, so that every path of the decoder runs far into the chunk."""
    n = int(k.snpdev_max_chunk_bytes())
    assert n == 1 << 24
    if backend.name == "emu":
        # the emulated wave decodes a megabyte of text in seconds, not sixteen, and a run of zeros of that size is 262 144
        # copy elements: text and zeros are the card's to run; here one literal element with a three-byte length and
        # copy-4 elements that reach across most of it stand in
        rng = np.random.RandomState(12)
        s = Stream()
        s.lit(rnd(rng, n - 200))
        s.copy(4, n - 300, 64)
        s.copy(4, 1 << 23, 64)
        s.lit(rnd(rng, 72))
        st, w = s.finish()
        assert w.size == n
        comp, chunks = [st], [w]
    else:
        chunks = [datasets.text(n, 3), np.zeros(n, np.uint8)]
        comp = libsnappy(oracle, chunks)
    assert (agree(backend, oracle, k, comp, [n] * len(chunks), expect=chunks, modes=("gg",)) == OK).all()


def test_mixed_workgroup(backend, oracle, k):
    """Two waves of every workgroup decode chunks of different kinds, the third compresses one, the fourth does not call
    at all: the calls contain no workgroup barrier."""
    d = backend.dev
    grid = 3 if backend.name == "emu" else 75
    count, iters = 2 * grid, 2000
    gens = sorted(datasets.CLASSES)
    chunks = [np.ascontiguousarray(datasets.CLASSES[gens[i % len(gens)]](3000 + 997 * (i % 5), i)).view(np.uint8).reshape(-1).copy()
              for i in range(count)]
    comp = libsnappy(oracle, chunks)
    caps = [c.size for c in chunks]
    raws = chunks[:grid]
    bounds = [32 + r.size + r.size // 6 for r in raws]
    src = place(d, comp, [i % 16 for i in range(count)])
    out = place(d, [c + GUARD for c in caps], [(3 * i) % 16 for i in range(count)], fill=0xA5)
    raw = place(d, raws, [(5 * i) % 16 for i in range(grid)])
    cout = place(d, [b + GUARD for b in bounds], [(7 * i) % 16 for i in range(grid)], fill=0xA5)
    capd = d.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    actual = d.upload(np.zeros(count, dtype=np.uint64).view(np.uint8))
    status = d.upload(np.full(count, -1, dtype=np.int32).view(np.uint8))
    csizes = d.upload(np.zeros(grid, dtype=np.uint64).view(np.uint8))
    side = d.upload(np.zeros(grid * 64, dtype=np.uint32).view(np.uint8))
    flags = d.upload(np.zeros(4, dtype=np.uint8))
    p = d.ptr
    assert k.snpdev_mixed(p(src.ptrs), p(src.sizes), p(out.ptrs), p(capd), p(actual), p(status), count, p(raw.ptrs), p(raw.sizes),
                          p(cout.ptrs), p(csizes), grid, p(side), iters, grid, p(flags), d.stream()) == 0
    d.synchronize()
    assert d.download(flags).view(np.uint32)[0] == 0
    assert (d.download(status).view(np.int32)[:count] == OK).all()
    assert d.download(actual).view(np.uint64)[:count].tolist() == caps
    host = d.download(out.slab)
    for o, c in zip(out.offsets, chunks):
        assert np.array_equal(host[int(o): int(o) + c.size], c) and (host[int(o) + c.size: int(o) + c.size + GUARD] == 0xA5).all()
    host = d.download(cout.slab)
    got = d.download(csizes).view(np.uint64)[:grid]
    for o, r, b, g in zip(cout.offsets, raws, bounds, got):
        o, g = int(o), int(g)
        assert 1 <= g <= b and (host[o + b: o + b + GUARD] == 0xA5).all()
        rc, back = oracle.snappy_decompress(host[o: o + g].copy(), r.size)
        assert rc == 0 and np.array_equal(back, r)
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
    comp = libsnappy(oracle, chunks)
    comp[3] = comp[3][:-2]
    for mode in MODES:
        st = agree(backend, oracle, k, comp, [c.size for c in chunks], modes=(mode,), block=block, chunks_per_wave=2, sizes=False)
        assert st[3] == BAD and (np.delete(st, 3) == OK).all()


# ---- 7. refusals ----

def test_capacities(backend, oracle, k):
    chunk = datasets.text(5000, 2)
    (s,) = libsnappy(oracle, [chunk])
    lit = Stream()
    lit.lit(bytes(range(200)) * 3)
    ls, lw = lit.finish()
    streams = [s, s, s, s, ls, ls, ls, ls]
    caps = [5000, 4999, 0, 5100, lw.size, lw.size - 1, 0, lw.size + 7]
    st = agree(backend, oracle, k, streams, caps, expect=[chunk, None, None, chunk, lw, None, None, lw])
    assert st.tolist() == [OK, BAD, BAD, OK] * 2


def test_the_preamble_is_the_limit(backend, oracle, k):
    """The cases of tests/test_snappy.py::test_preamble_is_the_limit: the guard bytes at and behind the declared length
    stay intact although the capacity leaves room."""
    rng = np.random.RandomState(5)
    data = rng.randint(0, 256, size=6000).astype(np.uint8).tobytes()

    def lit(b):
        s = Stream()
        s.lit(b)
        return bytes(s.el)

    copy2 = lambda n, off: bytes([((n - 1) << 2) | 2]) + off.to_bytes(2, "little")  # noqa: E731
    cases = [
        (b"\x80", 64, None),
        (b"\x80\x80\x80\x80\x80\x00" + lit(data[:8]), 64, None),
        (b"\xff\xff\xff\xff\x1f" + lit(data[:8]), 64, None),
        (b"\xe4\x80\x80\x80\x10" + lit(data[:100]), 100, None),
        (varint(1200) + lit(data[:1000]) + 4 * copy2(50, 100), 1200, 1200),
        (varint(1300) + lit(data[:1000]) + 4 * copy2(50, 100), 1300, 1300),
        (varint(1000) + lit(data[:1000]) + 4 * copy2(50, 100), 2000, 1000),
        (varint(5000) + lit(data[:3000]) + lit(data[3000:5000]) + copy2(60, 7), 6000, 5000),
        (varint(5000) + lit(data[:4500]) + lit(data[4500:5500]), 6000, 5000),
        (varint(1000) + lit(data[:990]) + copy2(11, 100), 2000, 1000),  # a copy that overruns by one byte
        (varint(20) + lit(data[:10]) + lit(data[:11]), 64, 20),         # a short literal that does
        (varint(1 << 27) + lit(data[:10]), 1 << 28, 1 << 27),           # a declared length above 64 MiB
    ]
    streams = [u8(c[0]) for c in cases[:-1]]
    st = agree(backend, oracle, k, streams, [c[1] for c in cases[:-1]])
    assert st.tolist() == [BAD] * 4 + [OK] + [BAD] * 6
    for mode in MODES:
        outs, _, _ = dev_decompress(backend, k, streams, [c[1] for c in cases[:-1]], mode=mode)
        for i, (o, c) in enumerate(zip(outs, cases)):
            if st[i] == BAD:
                assert (o[c[2] or 0:] == 0xA5).all(), f"{mode}: case {i}: wrote at or behind the declared length"
    # a capacity above 64 MiB counts as 64 MiB: the declared 128 MiB do not fit, whatever the caller says (nothing is
    # written, so the slot need not be that large)
    d = backend.dev
    src = place(d, [u8(cases[-1][0])], [0])
    out = place(d, [64], [0], fill=0xA5)
    capd = d.upload(np.asarray([cases[-1][1]], dtype=np.uint64).view(np.uint8))
    actual = d.upload(np.full(1, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
    status = d.upload(np.full(1, -1, dtype=np.int32).view(np.uint8))
    flags = d.upload(np.zeros(4, dtype=np.uint8))
    p = d.ptr
    assert k.snpdev_global(p(src.ptrs), p(src.sizes), p(out.ptrs), p(capd), p(actual), p(status), 1, 64, 1, p(flags), d.stream()) == 0
    d.synchronize()
    assert d.download(status).view(np.int32)[0] == BAD and d.download(actual).view(np.uint64)[0] == 0
    assert (d.download(out.slab) == 0xA5).all()
    got, sst = dev_sizes(backend, k, [u8(cases[-1][0])])
    assert got[0] == 1 << 27 and sst[0] == OK
    check_sizes(backend, k, [u8(cases[-1][0])])


def test_very_large_in_bytes(backend, k):
    """A stream of 2^32 - 64 bytes or more is refused by decompress(), one of 2^32 - 8 or more gives 0 from
    decompressed_size(), as the batched calls do -- before a byte is read, so a buffer of a few bytes stands in. One byte
    below either limit the preamble is read (and here, by the size query alone, found good: 5)."""
    d = backend.dev
    src = place(d, [u8(varint(5) + b"\x10abcde")], [0])
    p = d.ptr
    lim_dec, lim_size = (1 << 32) - 64, (1 << 32) - 8
    for n in (lim_dec, lim_dec + 1, lim_size, 1 << 32, (1 << 40) + 7):
        sizes = d.upload(np.asarray([n], dtype=np.uint64).view(np.uint8))
        out = place(d, [64], [0], fill=0xA5)
        capd = d.upload(np.asarray([32], dtype=np.uint64).view(np.uint8))
        actual = d.upload(np.full(1, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
        status = d.upload(np.full(1, -1, dtype=np.int32).view(np.uint8))
        flags = d.upload(np.zeros(4, dtype=np.uint8))
        assert k.snpdev_global(p(src.ptrs), p(sizes), p(out.ptrs), p(capd), p(actual), p(status), 1, 64, 1, p(flags), d.stream()) == 0
        d.synchronize()
        assert d.download(status).view(np.int32)[0] == BAD and d.download(actual).view(np.uint64)[0] == 0, n
        assert (d.download(out.slab) == 0xA5).all() and d.download(flags).view(np.uint32)[0] == 0
    for n, want in ((lim_size - 1, 5), (lim_size, 0), (lim_size + 1, 0), (1 << 32, 0), ((1 << 40) + 7, 0)):
        sizes = d.upload(np.asarray([n], dtype=np.uint64).view(np.uint8))
        got = d.upload(np.full(1, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
        status = d.upload(np.full(1, -1, dtype=np.int32).view(np.uint8))
        assert k.snpdev_sizes(p(src.ptrs), p(sizes), p(got), p(status), 1, 64, d.stream()) == 0
        d.synchronize()
        assert d.download(got).view(np.uint64)[0] == want, n
        assert d.download(status).view(np.int32)[0] == (OK if want else BAD), n
        # the batched size query on the same arguments
        bgot = d.upload(np.full(1, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
        assert backend.lib.nvcompBatchedSnappyGetDecompressSizeAsync(p(src.ptrs), p(sizes), p(bgot), 1, d.stream()) == 0
        d.synchronize()
        assert d.download(bgot).view(np.uint64)[0] == want, n


def forty_byte_stream(rng):
    """Every element kind in 40 bytes."""
    s = Stream()
    s.lit(rnd(rng, 6))
    s.copy(1, 3, 7)
    s.lit(rnd(rng, 9))
    s.copy(2, 10, 19)
    s.copy(4, 12, 5)
    s.lit(rnd(rng, 2), nb=1)
    s.copy(2, 1, 4)
    s.lit(rnd(rng, 4))
    st, w = s.finish()
    assert st.size == 40, st.size
    return st, w


def test_truncation_and_trailing_bytes(backend, oracle, k):
    rng = np.random.RandomState(10)
    s, w = forty_byte_stream(rng)
    streams = [s] + [s[:n].copy() for n in range(0, 40)] + [np.concatenate([s, np.array(t, np.uint8)]) for t in ([0], [7], [0, 0], [1, 9], [0xf0])]
    st = agree(backend, oracle, k, streams, [w.size + 64] * len(streams), expect=[w] + [None] * (len(streams) - 1))
    assert st[0] == OK and (st[1:] == BAD).all()


def test_offsets_in_front_of_the_output(backend, oracle, k):
    rng = np.random.RandomState(11)
    streams, declared = [], []
    for pre in (1, 40, 3000):
        for kind in (2, 4):
            for off in (0, pre + 1, pre + 100, 65535):
                for n in (1, 4, 64):
                    s = Stream()
                    s.lit(rnd(rng, pre))
                    s.copy(kind, off, n, expand=False)
                    s.lit(rnd(rng, 5))
                    st, _ = s.finish(declared=pre + n + 5)
                    streams.append(st)
                    declared.append(pre + n + 5)
    for off in (0, 41):  # copy-1
        s = Stream()
        s.lit(rnd(rng, 40))
        s.copy(1, off, 8, expand=False)
        st, _ = s.finish(declared=48)
        streams.append(st)
        declared.append(48)
    s = Stream()  # far in front, behind a train
    s.lit(rnd(rng, 2))
    for _ in range(70):
        s.copy(2, 2, 64)
    s.copy(4, len(s.out) + 1, 64, expand=False)
    st, _ = s.finish(declared=len(s.out) + 64)
    streams.append(st)
    declared.append(len(s.out) + 64)
    st = agree(backend, oracle, k, streams, declared)
    assert (st == BAD).all()


@pytest.mark.parametrize("first", range(0, 40, 5))
def test_every_single_byte_mutation_of_a_small_stream(backend, oracle, k, first):
    """All 255 other values of every byte of a 40-byte stream of all element kinds, five positions (1 275 streams) a case:
    status, byte count and bytes agree three-way for every one of them, at the exact capacity and with room behind it, and
    the guards behind the capacity are intact."""
    s, w = forty_byte_stream(np.random.RandomState(1234))
    streams, caps = [], []
    for at in range(first, first + 5):
        for x in range(1, 256):
            m = s.copy()
            m[at] ^= np.uint8(x)
            streams.append(m)
            caps.append(w.size + (0 if x % 2 else 40))
    agree(backend, oracle, k, streams, caps)


def test_random_single_byte_mutations(backend, oracle, k):
    """600 random single-byte mutations over streams of libsnappy and of the batched compressor."""
    rng = np.random.RandomState(1234)
    blocks = []
    gens = [g for g in sorted(datasets.CLASSES) if g not in ("zeros",)]
    for i in range(12):
        raw = np.ascontiguousarray(datasets.CLASSES[gens[i % len(gens)]](65536, i)).view(np.uint8).reshape(-1)
        n = 300
        comp = (libsnappy(oracle, [raw[:n]]) if i % 2 else backend.codec("Snappy").compress([raw[:n].copy()]))[0]
        while comp.size < 250:
            n += 50
            comp = (libsnappy(oracle, [raw[:n]]) if i % 2 else backend.codec("Snappy").compress([raw[:n].copy()]))[0]
        blocks.append((comp, n))
    streams, caps = [], []
    for i in range(600):
        c, n = blocks[i % len(blocks)]
        m = c.copy()
        m[int(rng.randint(0, m.size))] ^= np.uint8(rng.randint(1, 256))
        streams.append(m)
        caps.append(n + (0 if i % 4 else 40))
    for lo in range(0, 600, 300):
        agree(backend, oracle, k, streams[lo: lo + 300], caps[lo: lo + 300], modes=("gg", "ll") if lo else MODES)


# ---- 8. the last byte in front of an unmapped page (emulator only) ----

def test_nothing_is_touched_behind_the_stream_or_the_capacity(emu, oracle, tmp_path_factory):
    """Host memory: the stream's last byte, then the output's, is the last byte in front of a PROT_NONE page, or lies one,
    two, three bytes in front of it. A read or write past the end is a segmentation fault. (Never on the card: there the
    guard bytes stand in.)"""
    from hlif_container import guarded_mapping

    k = kernels(emu, tmp_path_factory)
    chunk = datasets.text(3000, 4)
    (s,) = libsnappy(oracle, [chunk])
    t = Stream()  # ends in copies of 1 .. 3 bytes at offsets 1 .. 3, and in a long literal
    t.lit(chunk[:50])
    t.copy(2, 1, 1)
    t.copy(2, 3, 2)
    t.copy(2, 2, 3)
    t2 = copy.deepcopy(t)
    t2.lit(chunk[100:300])
    cases = [(s, chunk), t.finish(), t2.finish()]
    base, span = guarded_mapping(2)
    room = (C.c_uint8 * span).from_address(base)
    for s, want in cases:
        for back in (0, 1, 2, 3):
            # the stream against the page
            at = span - back - s.size
            C.memmove(base + at, s.ctypes.data, s.size)
            out = np.full(want.size + GUARD, 0xA5, dtype=np.uint8)
            ptrs = np.array([base + at], dtype=np.uint64)
            sizes = np.array([s.size], dtype=np.uint64)
            optrs = np.array([out.ctypes.data], dtype=np.uint64)
            caps = np.array([want.size], dtype=np.uint64)
            actual, status, flags = np.zeros(1, np.uint64), np.full(1, -1, np.int32), np.zeros(1, np.uint32)
            assert k.snpdev_global(ptrs.ctypes.data, sizes.ctypes.data, optrs.ctypes.data, caps.ctypes.data, actual.ctypes.data,
                                   status.ctypes.data, 1, 64, 1, flags.ctypes.data, None) == 0
            assert status[0] == OK and actual[0] == want.size and np.array_equal(out[: want.size], want) and flags[0] == 0
            assert (out[want.size:] == 0xA5).all()
            # the preamble alone against the page
            for cut in (1, 2):
                C.memmove(base + span - cut, s.ctypes.data, cut)
                ptrs1, sizes1, got = np.array([base + span - cut], dtype=np.uint64), np.array([cut], dtype=np.uint64), np.zeros(1, np.uint64)
                assert k.snpdev_sizes(ptrs1.ctypes.data, sizes1.ctypes.data, got.ctypes.data, status.ctypes.data, 1, 64, None) == 0
            # the output against the page, the capacity exact
            src = s.copy()
            ptrs = np.array([src.ctypes.data], dtype=np.uint64)
            oat = span - back - want.size
            C.memset(base + oat, 0xA5, want.size)
            optrs = np.array([base + oat], dtype=np.uint64)
            assert k.snpdev_global(ptrs.ctypes.data, sizes.ctypes.data, optrs.ctypes.data, caps.ctypes.data, actual.ctypes.data,
                                   status.ctypes.data, 1, 64, 1, flags.ctypes.data, None) == 0
            assert status[0] == OK and actual[0] == want.size and flags[0] == 0
            assert np.array_equal(np.frombuffer(room, dtype=np.uint8, count=want.size, offset=oat), want)


# ---- 9. the header's promises ----

def _need_hipcc():
    if shutil.which(HIPCC) is None and not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")


def test_header_is_self_contained(tmp_path):
    _need_hipcc()
    only = tmp_path / "only.hip"
    only.write_text("#include <nvcomp/device/snappy.hpp>\n")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(REPO, "include"),
                        "-c", str(only), "-o", str(tmp_path / "only.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_not_in_the_umbrella_headers():
    assert os.path.exists(os.path.join(REPO, "include", "nvcomp", "device", "snappy.hpp"))
    for umbrella in ("nvcomp.h", "nvcomp.hpp"):
        r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(REPO, "include"), "-I",
                            "/opt/rocm/include", "-M", "-x", "c++", os.path.join(REPO, "include", umbrella)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "nvcomp/device" not in r.stdout and "snappy_core" not in r.stdout


@pytest.mark.gpu
def test_example_on_gpu():
    exe = os.path.join(REPO, "examples", "bin", "snappy_device_example")
    r = subprocess.run(["make", "-C", "examples", exe], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "PASSED" in r.stdout
