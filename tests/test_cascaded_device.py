"""Device-side Cascaded API (include/nvcomp/device/cascaded.hpp): kernels of tests/device_api/cascaded_device_kernels.hip
call it, on the host emulation and on the MI355X (`backend`). Its streams must be the batched API's byte for byte, through
memory and through element sources; its decoders -- into memory and into element sinks -- must invert both compressors'
output and the CPU model's (oracle/cascaded_ref.c) at every place the decoder leaves a sub-chunk, keep to the LDS slice
they are given, and refuse what the batched decoder refuses. Everything is exact: bytes, sizes, statuses; every output
slot is followed by guard bytes that must survive."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import cascaded_stream as cs
from nvcomp_amd import datasets
from nvcomp_amd._lib import CascadedOpts, NvcompStatus
from nvcomp_amd.batched import make_batch, empty_batch, read_batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "device_api", "cascaded_device_kernels.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GUARD = 32
PARTS = 7  # tests/device_api/cascaded_device_kernels.hip: -DCDEV_PART=0 ... 6
WIDTH = [1, 1, 2, 2, 4, 4, 8, 8]
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
SCHEMES = [(0, 0, 1), (1, 0, 1), (0, 1, 1), (2, 2, 1), (3, 1, 1), (1, 2, 0), (2, 1, 0), (0, 0, 0)]  # test_scheme_combinations
LDS_LIMIT = 65536  # what a workgroup of these tests holds
NOT_SUPPORTED = 11


class Slices(C.Structure):
    _fields_ = [("lead", C.c_uint), ("pitch", C.c_uint), ("bytes", C.c_uint)]


_libs = {}


def compile_parts(d, extra):
    from concurrent.futures import ThreadPoolExecutor

    def one(p):
        obj = str(d / f"part{p}.o")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(REPO, "include"),
                            f"-DCDEV_PART={p}", *extra, "-c", SRC, "-o", obj], cwd=REPO, capture_output=True, text=True)
        (d / f"part{p}.log").write_text(r.stderr)
        assert r.returncode == 0, r.stderr[-3000:]
        return obj

    with ThreadPoolExecutor(PARTS) as pool:
        return list(pool.map(one, range(PARTS)))


def kernels(backend, tmp_path_factory):
    """The test kernels built for the backend's tier (once per session)."""
    if backend.name not in _libs:
        d = tmp_path_factory.mktemp(f"cdev_{backend.name}")
        so = str(d / "cdev.so")
        if backend.name == "emu":
            import conftest

            conftest.emu_library()
            cmd = ["g++", "-O1", "-std=c++17", "-x", "c++", "-shared", "-fPIC", "-Itests/emu", "-Iinclude", SRC, "-o", so,
                   "-Ltests/emu", "-lnvcomp_emu", f"-Wl,-rpath,{REPO}/tests/emu"]
            r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-3000:]
        else:
            objs = compile_parts(d, ["-fPIC"])
            r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", so], cwd=REPO,
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-3000:]
        lib = C.CDLL(so)
        vp, sz, u, O, S = C.c_void_p, C.c_size_t, C.c_uint, CascadedOpts, Slices
        lib.cdev_compress.argtypes = [vp, vp, vp, vp, sz, O, u, S, u, u, u, vp, vp]
        lib.cdev_decompress.argtypes = [vp, vp, vp, vp, vp, vp, sz, u, u, S, u, u, vp, vp, vp, vp]
        lib.cdev_mixed.argtypes = [vp, vp, vp, vp, vp, vp, sz, S, vp, u, u, vp]
        lib.cdev_lds.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, O, vp]
        lib.cdev_sizes.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp]
        for name in ("cdev_max_compressed_bytes", "cdev_compress_shared_bytes", "cdev_decompress_shared_bytes", "cdev_max_chunk_bytes"):
            getattr(lib, name).restype = sz
        lib.cdev_max_compressed_bytes.argtypes = [sz, O]
        lib.cdev_compress_shared_bytes.argtypes = [O]
        lib.cdev_decompress_shared_bytes.argtypes = [O]
        _libs[backend.name] = lib
    return _libs[backend.name]


@pytest.fixture
def k(backend, tmp_path_factory):
    return kernels(backend, tmp_path_factory)


class Dev:
    def __init__(self, backend):
        self.d = backend.dev

    def zeros(self, n, dtype):
        return self.d.upload(np.zeros(max(n, 1), dtype=dtype).view(np.uint8))

    def get(self, buf, n, dtype):
        return self.d.download(buf).view(dtype)[:n].copy()

    def p(self, buf):
        return self.d.ptr(buf) if buf is not None else None


def layout(slice_bytes, waves=4):
    """Slices that are parts of one larger array: 16 bytes in front, 16 bytes between them; as many waves (at most
    `waves`) as one workgroup's LDS holds."""
    pitch = (slice_bytes + 15) // 16 * 16 + 16
    waves = max(1, min(waves, 1 + (LDS_LIMIT - 16 - slice_bytes) // pitch))
    sl = Slices(16, pitch, slice_bytes)
    assert 16 + (waves - 1) * pitch + slice_bytes <= LDS_LIMIT
    return sl, 64 * waves, 16 + (waves - 1) * pitch + slice_bytes


def dev_compress(backend, k, chunks, opts, mode=0, slice_bytes=None):
    """compress() (mode 0) or compress_from() over a memory source (1). Every output slot is max_compressed_bytes long (or
    what the batched bound would be where the options are refused) and followed by guard bytes that must survive."""
    h = Dev(backend)
    n = len(chunks)
    o = CascadedOpts(*opts)
    if slice_bytes is None:
        slice_bytes = int(k.cdev_compress_shared_bytes(o)) or 4096
    sl, block, lds = layout(slice_bytes)
    src = make_batch(backend.dev, chunks, align=8)
    longest = max([c.size for c in chunks] + [1])
    max_out = int(k.cdev_max_compressed_bytes(longest, o)) or (longest + 4096)
    dst = empty_batch(backend.dev, [max_out + GUARD] * n, stride=(max_out + GUARD + 7) // 8 * 8, fill=0xA5)
    flags = h.zeros(1, np.uint32)
    waves = block // 64
    rc = k.cdev_compress(h.p(src.ptrs), h.p(src.sizes), h.p(dst.ptrs), h.p(dst.sizes), n, o, mode, sl, lds, block,
                         max(1, -(-n // waves)), h.p(flags), backend.dev.stream())
    assert rc == 0
    backend.dev.synchronize()
    sizes = h.get(dst.sizes, n, np.uint64)
    assert (sizes <= max_out).all()
    host = backend.dev.download(dst.slab)
    for off in dst.offsets:
        assert (host[int(off) + max_out: int(off) + max_out + GUARD] == 0xA5).all(), "the compressor wrote past its bound"
    assert int(h.get(flags, 1, np.uint32)[0]) == 0, "the source was asked for an element at or beyond n_elems"
    return read_batch(backend.dev, dst, sizes)


def dev_decompress(backend, k, comp, caps, mode=0, elem=4, slice_bytes=None, opts=(4096, 4, 2, 1, 1), waves=4, base_misalign=0,
                   out_align=16):
    """decompress() (mode 0) or decompress_to<elem bytes>() (1: a sink that stores and counts its calls per element; 2: a
    sink that adds the elements up). Output slots are filled with 0xA5 and followed by guard bytes that must survive.
    Returns (whole output slots, actual sizes, statuses, call counts per element or None, sums or None)."""
    h = Dev(backend)
    n = len(comp)
    if slice_bytes is None:
        slice_bytes = int(k.cdev_decompress_shared_bytes(CascadedOpts(*opts)))
    sl, block, _ = layout(slice_bytes, waves)
    src = make_batch(backend.dev, comp, align=8, base_misalign=base_misalign)
    out = empty_batch(backend.dev, [c + GUARD for c in caps], align=out_align, fill=0xA5)
    out.sizes = backend.dev.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    actual = h.zeros(n, np.uint64)
    status = backend.dev.upload(np.full(n, -1, dtype=np.int32).view(np.uint8))
    flags = h.zeros(1, np.uint32)
    cnt = empty_batch(backend.dev, [4 * (c // elem + 8) for c in caps], align=16, fill=0) if mode == 1 else None
    sums = h.zeros(n, np.uint64) if mode == 2 else None
    w = block // 64
    rc = k.cdev_decompress(h.p(src.ptrs), h.p(src.sizes), h.p(out.ptrs), h.p(out.sizes), h.p(actual), h.p(status), n, mode, elem,
                           sl, block, max(1, -(-n // w)), h.p(cnt.ptrs) if cnt else None, h.p(sums), h.p(flags),
                           backend.dev.stream())
    assert rc == 0
    backend.dev.synchronize()
    host = backend.dev.download(out.slab)
    outs = []
    for off, s in zip(out.offsets, caps):
        off = int(off)
        outs.append(host[off: off + s].copy())
        assert (host[off + s: off + s + GUARD] == 0xA5).all(), "a write past the output capacity"
    assert int(h.get(flags, 1, np.uint32)[0]) == 0, "the sink was handed an element beyond the capacity"
    counts = [c.view(np.uint32) for c in read_batch(backend.dev, cnt)] if cnt else None
    return outs, h.get(actual, n, np.uint64), h.get(status, n, np.int32), counts, (h.get(sums, n, np.uint64) if mode == 2 else None)


def check_decodes(backend, k, streams, chunks, elem, opts, modes=(0, 1, 2), **kw):
    """Through memory, through the storing and counting sink, through the summing sink."""
    caps = [c.size for c in chunks]
    for mode in modes:
        outs, actual, status, counts, sums = dev_decompress(backend, k, streams, caps, mode=mode, elem=elem, opts=opts, **kw)
        assert (status == NvcompStatus.Success).all(), (mode, status)
        assert actual.tolist() == caps
        if mode == 2:
            want = [int(c.view(UNSIGNED[elem]).astype(np.uint64).sum(dtype=np.uint64)) for c in chunks]
            assert sums.tolist() == want
            continue
        for i, (c, o) in enumerate(zip(chunks, outs)):
            assert np.array_equal(o, c), (mode, i)
        if mode == 1:
            for c, cnt in zip(chunks, counts):
                n_el = c.size // elem
                assert (cnt[:n_el] == 1).all(), "an element was handed to the sink other than once"
                assert (cnt[n_el:] == 0).all(), "the sink saw an element at or beyond n / sizeof(T)"


def mixed_chunk(w, n_bytes, seed):
    """Smooth values, runs, a constant stretch and noise in one chunk of n_bytes (whole elements)."""
    rng = np.random.RandomState(seed)
    dt = UNSIGNED[w]
    n = n_bytes // w
    q = max(1, n // 4)
    smooth = np.cumsum(rng.randint(0, 5, size=q)).astype(np.uint64).astype(dt)
    runs = np.repeat(rng.randint(0, 100, size=q // 3 + 1), 3)[:q].astype(dt)
    const = np.full(q, 7, dt)
    noise = np.frombuffer(rng.bytes(max(0, n - 3 * q) * w), dtype=dt)
    return np.concatenate([smooth, runs, const, noise])[:n].view(np.uint8).copy()


@pytest.mark.parametrize("typ", range(8))
def test_streams(backend, oracle, k, typ):
    """compress() == compress_from() == the batched compressor == the CPU model, byte for byte: every scheme of
    test_scheme_combinations at 4 096-byte sub-chunks and the default scheme at 256, 1 000, 4 096 and 16 384; chunks of 0
    bytes, of one element and one that ends in a partial sub-chunk. Options the batched compressor refuses for want of LDS
    give 0 here."""
    w = WIDTH[typ]
    combos = [(4096, typ, r, d, bp) for r, d, bp in SCHEMES] + [(sub, typ, 2, 1, 1) for sub in (256, 1000, 16384)]
    for opts in combos:
        sub = opts[0]
        chunks = [np.zeros(0, np.uint8), mixed_chunk(w, w, 1), mixed_chunk(w, 2 * sub + (sub // 2) // w * w + w, typ + sub)]
        made = dev_compress(backend, k, chunks, opts, mode=0)
        sourced = dev_compress(backend, k, chunks, opts, mode=1)
        try:
            batched = backend.codec("Cascaded", opts).compress(chunks, in_align=8)
        except RuntimeError as e:
            assert f"returned {NOT_SUPPORTED}" in str(e)
            assert all(m.size == 0 for m in made + sourced), f"{opts}: refused by the batched compressor, yet compressed"
            continue
        for i, c in enumerate(chunks):
            ref = oracle.cascaded_compress(c, *opts)
            assert np.array_equal(made[i], ref), f"{opts} chunk {i}: compress() and the CPU model differ"
            assert np.array_equal(sourced[i], ref), f"{opts} chunk {i}: compress_from() and the CPU model differ"
            assert np.array_equal(batched[i], ref), f"{opts} chunk {i}"
            assert len(cs.parse(made[i])) == -(-c.size // sub)
        check_decodes(backend, k, made, chunks, w, opts, modes=(0, 1))


def exit_shapes(w, rng):
    """The shapes of test_cascaded.py::test_short_run_expansion, and what reaches the other ways out of a sub-chunk."""
    dt = UNSIGNED[w]

    def column(run_lengths, n_runs):
        runs = rng.choice(run_lengths, size=n_runs)
        vals = (np.cumsum(rng.randint(1, 7, size=n_runs)) % (1 << (8 * w - 1) if w < 8 else 1 << 62)).astype(dt)
        vals[1:][vals[1:] == vals[:-1]] += 1
        return np.repeat(vals, runs).view(np.uint8)

    shapes = {
        "runs 1..2": column([1, 1, 1, 1, 1, 1, 1, 2], 3000),
        "runs 1..4": column([1, 1, 1, 1, 2, 3, 4], 3000),
        "max run 8": column([1, 1, 1, 5, 8], 2000),
        "max run 64": column([1, 2, 64], 400),
        "run of 65": column([1, 2, 65], 400),
        "min run 2": column([2, 3], 2000),
        "run of 300": column([1, 1, 1, 1, 1, 300], 500),
        "every value twice": np.repeat(column([1, 2], 1500).view(dt), 2).view(np.uint8),
        "distinct": column([1], 5000),
        "noise": np.frombuffer(rng.bytes(12288 + 8), dtype=np.uint8),
        "float columns": np.ascontiguousarray(datasets.float_columns(32768, w)).view(np.uint8).reshape(-1),
    }
    return {name: c[: min(c.size, 65536) // w * w].copy() for name, c in shapes.items()}


@pytest.mark.parametrize("w", [1, 2, 4, 8])
def test_every_decoder_exit(backend, oracle, k, w):
    """The five places where decompress_sub leaves a sub-chunk -- raw copy, layer 0's delta, direct expansion, pool + marks
    expansion, copy-out -- through memory and through the sink: the output equals the input, every element reaches the
    sink exactly once, a per-chunk sum equals numpy's."""
    typ = {1: 1, 2: 3, 4: 4, 8: 6}[w]
    shapes = exit_shapes(w, np.random.RandomState(100 + w))
    names, chunks = zip(*shapes.items())
    for r, d, bp in ((2, 1, 1), (1, 0, 1), (0, 1, 1), (0, 0, 1), (1, 1, 1)):
        opts = (4096, typ, r, d, bp)
        streams = [oracle.cascaded_compress(c, *opts) for c in chunks]
        parsed = {n: cs.parse(s) for n, s in zip(names, streams)}
        assert all(s.raw is not None for s in parsed["noise"]), "noise is stored raw"
        if r:
            for name, short in (("run of 65", False), ("run of 300", False), ("max run 64", True), ("max run 8", True)):
                subs = [s for s in parsed[name] if s.raw is None]
                assert subs
                is_short = [s.runs[0].bits <= 6 and 1 <= s.runs[0].min and s.runs[0].min + (1 << s.runs[0].bits) - 1 <= 64 for s in subs]
                assert all(is_short) if short else not all(is_short), name
        check_decodes(backend, k, streams, chunks, w, opts)


def test_other_producers(backend, oracle, k):
    """Streams of the batched compressor and of the CPU model decode through the header; the header's streams decode
    through nvcompBatchedCascadedDecompressAsync and the CPU model; tests/cascaded_stream.py parses them."""
    opts = (4096, 4, 2, 1, 1)
    chunks = [np.ascontiguousarray(datasets.int32_column(30000, 2)).view(np.uint8), datasets.float_columns(65536, 1),
              datasets.lowcard(20000, 3), datasets.noise(8192, 4), np.zeros(4, np.uint8)]
    chunks = [np.ascontiguousarray(c).view(np.uint8).reshape(-1)[: c.size // 4 * 4].copy() for c in chunks]
    codec = backend.codec("Cascaded", opts)
    for streams in (codec.compress(chunks, in_align=8), [oracle.cascaded_compress(c, *opts) for c in chunks]):
        check_decodes(backend, k, streams, chunks, 4, opts)
    made = dev_compress(backend, k, chunks, opts, mode=1)
    outs, actual, status = codec.decompress(made, [c.size for c in chunks], comp_align=8, out_align=8)
    assert (status == NvcompStatus.Success).all() and actual.tolist() == [c.size for c in chunks]
    for c, o, m in zip(chunks, outs, made):
        assert np.array_equal(o, c)
        rc, ref = oracle.cascaded_decompress(m, c.size)
        assert rc == 0 and np.array_equal(ref, c)
        h = cs.header(m)
        assert (h.type, h.num_rles, h.num_deltas, h.use_bp, h.n_bytes, h.sub_chunk_bytes) == (4, 2, 1, 1, c.size, 4096)
        cs.parse(m)
    # the header queries agree with the batched size query
    h = Dev(backend)
    n = len(made)
    src = make_batch(backend.dev, made, align=8)
    sizes, elems, types, shared = h.zeros(n, np.uint64), h.zeros(n, np.uint32), h.zeros(n, np.int32), h.zeros(n, np.uint64)
    assert k.cdev_sizes(h.p(src.ptrs), h.p(src.sizes), h.p(sizes), h.p(elems), h.p(types), h.p(shared), n, backend.dev.stream()) == 0
    backend.dev.synchronize()
    assert h.get(sizes, n, np.uint64).tolist() == codec.get_decompress_size(made, comp_align=8).tolist() == [c.size for c in chunks]
    assert (h.get(elems, n, np.uint32) == 4).all() and (h.get(types, n, np.int32) == 4).all()
    assert (h.get(shared, n, np.uint64) == k.cdev_decompress_shared_bytes(CascadedOpts(*opts))).all()


def test_queries(backend, k):
    """max_compressed_bytes is nvcompBatchedCascadedCompressGetMaxOutputChunkSize; refused options give 0 everywhere."""
    assert k.cdev_max_chunk_bytes() == 1 << 24
    for opts in ((4096, 4, 2, 1, 1), (256, 0, 0, 0, 0), (16384, 7, 7, 7, 1), (1000, 6, 1, 2, 1)):
        codec = backend.codec("Cascaded", opts)
        for n in (0, 1, 255, 4096, 65536, 65543, 1 << 24):
            assert k.cdev_max_compressed_bytes(n, CascadedOpts(*opts)) == codec.max_compressed_size(n)
        assert k.cdev_compress_shared_bytes(CascadedOpts(*opts)) % 16 == 0 and k.cdev_compress_shared_bytes(CascadedOpts(*opts)) >= opts[0]
        assert k.cdev_decompress_shared_bytes(CascadedOpts(*opts)) >= 2 * opts[0]
    assert k.cdev_max_compressed_bytes((1 << 24) + 1, CascadedOpts(4096, 4, 2, 1, 1)) == 0
    for bad in ((4096, 8, 2, 1, 1), (4096, 4, 8, 1, 1), (4096, 4, 2, 8, 1), (4096, 4, 2, 1, 2), (100, 4, 2, 1, 1), (4098, 4, 2, 1, 1),
                (32768, 4, 2, 1, 1), (4096, 0xff, 2, 1, 1)):
        o = CascadedOpts(*bad)
        assert k.cdev_max_compressed_bytes(65536, o) == k.cdev_compress_shared_bytes(o) == k.cdev_decompress_shared_bytes(o) == 0
        c = [np.arange(1024, dtype=np.uint32).view(np.uint8)]
        assert dev_compress(backend, k, c, bad, mode=0)[0].size == 0
    # not whole elements
    assert dev_compress(backend, k, [np.zeros(1001, np.uint8)], (4096, 4, 2, 1, 1))[0].size == 0


def sub_needs(stream, w):
    """What decompress_sub plans for every sub-chunk of a stream with ONE RLE layer (casc::decompress_sub): nothing for a
    raw one; one value buffer when the runs are short or the layer is the identity; else values, run pool and marks."""
    a16 = lambda v: (v + 15) // 16 * 16
    needs = []
    for s in cs.parse(stream):
        if s.raw is not None:
            needs.append(0)
            continue
        r = s.runs[0]
        ident = r.bits == 0 and r.min == 1 and r.count == s.n_elems
        short = r.bits <= 6 and 1 <= r.min and r.min + (1 << r.bits) - 1 <= 64
        if ident:
            needs.append(a16(s.n_elems * w))
        elif short:
            needs.append(a16(r.count * w))
        else:
            needs.append(a16(r.count * w) + a16(2 * r.count) + a16(2 * s.n_elems))
    return needs


def test_lds_contract(backend, oracle, k):
    """The slice is carved from the stream's actual counts: a pool + marks sub-chunk decodes in exactly what it needs and
    gives nvcompErrorNotSupported, size 0, one 16-byte step below -- the guards and, for decompress(), everything behind
    the last good sub-chunk untouched; compressible chunks decode far below the worst case; compress() with too small a
    slice returns 0."""
    opts = (4096, 4, 1, 0, 1)
    rng = np.random.RandomState(9)
    vals = np.cumsum(rng.randint(1, 7, size=3000)).astype(np.uint32)
    long_runs = np.repeat(vals, rng.choice([1, 1, 2, 300], size=3000))[4096: 4096 + 6 * 1024]  # six sub-chunks
    smooth = np.repeat(vals, rng.choice([1, 2, 3], size=3000))[: 6 * 1024]                    # short runs everywhere
    chunk = np.concatenate([smooth[:2048], long_runs[:3072], smooth[2048:3072]]).view(np.uint8)  # subs 0-1 short, 2-4 long, 5 short
    stream = oracle.cascaded_compress(chunk, *opts)
    needs = sub_needs(stream, 4)
    worst = int(k.cdev_decompress_shared_bytes(CascadedOpts(*opts)))
    need = max(needs)
    first_big = needs.index(need)
    assert need < worst and first_big >= 2 and max(needs[:first_big]) <= need - 16
    check_decodes(backend, k, [stream], [chunk], 4, opts, slice_bytes=need)
    for mode in (0, 1):
        outs, actual, status, counts, _ = dev_decompress(backend, k, [stream], [chunk.size], mode=mode, elem=4, slice_bytes=need - 16)
        assert status[0] == NvcompStatus.ErrorNotSupported and actual[0] == 0
        done = first_big * 4096
        assert (outs[0][done:] == 0xA5).all(), "written behind the sub-chunk that did not fit"
        assert np.array_equal(outs[0][:done], chunk[:done])
        if mode == 1:
            assert (counts[0][: done // 4] == 1).all() and (counts[0][done // 4:] == 0).all()
    # compressible data: far below the worst case of its options
    d_opts = (4096, 4, 2, 1, 1)
    easy = [np.ascontiguousarray(datasets.int32_column(65536, 3)).view(np.uint8), np.ascontiguousarray(datasets.float_columns(65536, 2)).view(np.uint8)]
    streams = [oracle.cascaded_compress(c, *d_opts) for c in easy]
    assert int(k.cdev_decompress_shared_bytes(CascadedOpts(*d_opts))) >= 2 * 5120
    check_decodes(backend, k, streams, easy, 4, d_opts, slice_bytes=5120)
    # the compressor: no sub-chunk fits, or the run pool does not
    for small in (0, 1024, 4096 + 48):
        for mode in (0, 1):
            assert dev_compress(backend, k, [chunk], d_opts, mode=mode, slice_bytes=small)[0].size == 0
    whole = dev_compress(backend, k, [chunk], d_opts, slice_bytes=int(k.cdev_compress_shared_bytes(CascadedOpts(*d_opts))))
    assert np.array_equal(whole[0], oracle.cascaded_compress(chunk, *d_opts))


def test_mixed_workgroup(backend, oracle, k):
    """A 256-thread workgroup: wave 0 calls decompress(), wave 3 decompress_to(), each with its own part of one LDS array;
    wave 1 has returned and wave 2 spins on arithmetic. No call contains a workgroup barrier."""
    h = Dev(backend)
    opts = (4096, 4, 2, 1, 1)
    count = 6 if backend.name == "emu" else 48
    chunks = [np.ascontiguousarray((datasets.float_columns if i % 2 else datasets.int32_column)(12288 + 4096 * (i % 3) + 8 * i, i)).view(np.uint8).reshape(-1)
              for i in range(count)]
    chunks = [c[: c.size // 4 * 4].copy() for c in chunks]
    comp = [oracle.cascaded_compress(c, *opts) for c in chunks]
    caps = [c.size for c in chunks]
    sl = Slices(48, 5120 + 32, 5120)  # the slices of compressible data: all four parts fit a 64 KiB workgroup with room to spare
    src = make_batch(backend.dev, comp, align=8)
    out = empty_batch(backend.dev, [c + GUARD for c in caps], align=16, fill=0xA5)
    out.sizes = backend.dev.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    actual = h.zeros(count, np.uint64)
    status = backend.dev.upload(np.full(count, -1, dtype=np.int32).view(np.uint8))
    grid, iters = count // 2, 2000
    side = h.zeros(grid * 64, np.uint32)
    assert k.cdev_mixed(h.p(src.ptrs), h.p(src.sizes), h.p(out.ptrs), h.p(out.sizes), h.p(actual), h.p(status), count, sl, h.p(side),
                        iters, grid, backend.dev.stream()) == 0
    backend.dev.synchronize()
    assert (h.get(status, count, np.int32) == 0).all() and h.get(actual, count, np.uint64).tolist() == caps
    host = backend.dev.download(out.slab)
    for o, c in zip(out.offsets, chunks):
        assert np.array_equal(host[int(o): int(o) + c.size], c) and (host[int(o) + c.size: int(o) + c.size + GUARD] == 0xA5).all()
    x = np.arange(1, grid * 64 + 1, dtype=np.uint32)
    for _ in range(iters):
        x ^= x << np.uint32(13)
        x ^= x >> np.uint32(17)
        x ^= x << np.uint32(5)
    assert np.array_equal(h.get(side, x.size, np.uint32), x)


def refusals(oracle):
    """(label, stream, capacity) -- deterministic damage to streams of 30 000 bytes of an int32 column, default options."""
    opts = (4096, 4, 2, 1, 1)
    c = np.ascontiguousarray(datasets.int32_column(30000, 2)).view(np.uint8)
    good = oracle.cascaded_compress(c, *opts)
    n = c.size
    out = [("good", good, n)]
    for cut in (0, 3, 4, 7, 8, 11, 12, 15, 16, 19, 20, 23, 20 + 4 * 8 - 1, 20 + 4 * 8, 20 + 4 * 8 + 3, good.size // 2, good.size - 1):
        out.append((f"cut at {cut}", good[:cut].copy(), n))

    def poke(label, at, fmt, value, cap=n):
        b = good.copy()
        b[at: at + struct.calcsize(fmt)] = np.frombuffer(struct.pack(fmt, value), dtype=np.uint8)
        out.append((label, b, cap))

    first = 20 + 4 * 8  # the first sub-chunk's payload: n_elems, count[0], count[1], then the run streams
    count0 = struct.unpack_from("<I", good.tobytes(), first + 4)[0]
    poke("magic", 0, "<B", good[0] ^ 0xFF)
    poke("type 8", 4, "<B", 8)
    poke("8 RLE layers", 5, "<B", 8)
    poke("8 delta layers", 6, "<B", 8)
    poke("sub-chunk bytes 0", 12, "<I", 0)
    poke("sub-chunk bytes odd", 12, "<I", 4098)
    poke("num_sub", 16, "<I", 7)
    poke("size field", 8, "<B", good[8] ^ 0x40)
    poke("table runs backwards", 20 + 4, "<I", 3)
    poke("table beyond the stream", 20 + 4 * 7, "<I", good.size)
    poke("n_elems", first, "<I", 1023)
    poke("counts grow", first + 8, "<I", count0 + 1)
    poke("count beyond n", first + 4, "<I", 1025)
    poke("bits 65", first + 12, "<I", 65)
    poke("bits of the values", first + 12 + 12 + 12, "<I", 65)
    out.append(("capacity one byte short", good, n - 1))
    out.append(("capacity four bytes short", good, n - 4))
    rng = np.random.RandomState(5)  # the mutations of test_cascaded.py::test_corrupt_and_misaligned
    b = good.copy()
    b[rng.randint(20, b.size)] ^= 0x10
    out.append(("a payload bit", b, n))
    return out, c


def test_refusals_match_batched(backend, oracle, k):
    """Chunk by chunk, status and size are the batched decoder's -- through memory and through the sink --, a misaligned
    `in` is nvcompErrorAlignment, a sink of another width nvcompErrorInvalidValue, and random damage returns inside its slot."""
    cases, chunk = refusals(oracle)
    labels, streams, caps = zip(*cases)
    codec = backend.codec("Cascaded", (4096, 4, 2, 1, 1))
    _, b_actual, b_status = codec.decompress(list(streams), list(caps), comp_align=8, out_align=8)
    assert b_status[0] == 0 and (b_status[1:18] != 0).all()
    for mode in (0, 1):
        outs, actual, status, counts, _ = dev_decompress(backend, k, list(streams), list(caps), mode=mode, elem=4)
        for i, label in enumerate(labels):
            assert status[i] == b_status[i] and actual[i] == b_actual[i], (mode, label, status[i], b_status[i])
            if b_status[i] == 0:
                rc, ref = oracle.cascaded_decompress(streams[i], caps[i])
                assert rc == 0 and np.array_equal(outs[i][: ref.size], ref)
        short = labels.index("capacity one byte short")
        assert (outs[short] == 0xA5).all(), "a refused capacity, yet something was written"
    n = 4
    _, _, b_status = codec.decompress([streams[0]] * n, [caps[0]] * n, comp_align=8, out_align=8, base_misalign=1)
    assert (b_status == NvcompStatus.ErrorAlignment).all()
    for mode in (0, 1):
        outs, actual, status, _, _ = dev_decompress(backend, k, [streams[0]] * n, [caps[0]] * n, mode=mode, base_misalign=1)
        assert (status == NvcompStatus.ErrorAlignment).all() and (actual == 0).all() and all((o == 0xA5).all() for o in outs)
    # an output that is not aligned to the element: the batched decoder's nvcompErrorAlignment
    outs, actual, status, _, _ = dev_decompress(backend, k, [streams[0]] * 2, [caps[0] + 2, caps[0]], mode=0, out_align=1)
    _, _, b_status = codec.decompress([streams[0]] * 2, [caps[0] + 2, caps[0]], comp_align=8, out_align=1)
    assert status.tolist() == b_status.tolist()
    for elem in (1, 2, 8):
        outs, actual, status, counts, _ = dev_decompress(backend, k, [streams[0]], [caps[0]], mode=1, elem=elem)
        assert status[0] == NvcompStatus.ErrorInvalidValue and actual[0] == 0
        assert (outs[0] == 0xA5).all() and (counts[0] == 0).all()
    rng = np.random.RandomState(11)
    flipped = []
    for _ in range(24 if backend.name == "emu" else 200):
        b = streams[0].copy()
        for at in rng.randint(0, b.size, size=rng.randint(1, 4)):
            b[at] ^= 1 << rng.randint(0, 8)
        flipped.append(b)
    _, b_actual, b_status = codec.decompress(flipped, [caps[0]] * len(flipped), comp_align=8, out_align=8)
    for mode in (0, 1):
        outs, actual, status, _, _ = dev_decompress(backend, k, flipped, [caps[0]] * len(flipped), mode=mode)  # (guards checked inside)
        assert status.tolist() == b_status.tolist() and actual.tolist() == b_actual.tolist()


def test_in_and_out_in_lds(backend, oracle, k):
    """A 16 KiB chunk decoded into LDS, consumed there, and another compressed from LDS: the global path's results."""
    h = Dev(backend)
    opts = (4096, 4, 2, 1, 1)
    raws = [datasets.int32_column(16384, 1), datasets.float_columns(16384, 2), datasets.noise(16384, 3), datasets.lowcard(10000, 4),
            np.zeros(0, np.uint8)]
    raws = [np.ascontiguousarray(c).view(np.uint8).reshape(-1)[: c.size // 4 * 4].copy() for c in raws]
    others = raws[1:] + raws[:1]
    streams = [oracle.cascaded_compress(c, *opts) for c in others]
    n = len(raws)
    src = make_batch(backend.dev, streams, align=8)
    rawb = make_batch(backend.dev, raws, align=8)
    dec = empty_batch(backend.dev, [16384 + GUARD] * n, stride=16384 + GUARD, fill=0xA5)
    max_out = int(k.cdev_max_compressed_bytes(16384, CascadedOpts(*opts)))
    comp = empty_batch(backend.dev, [max_out] * n, stride=(max_out + 7) // 8 * 8)
    actual, status, sums = h.zeros(n, np.uint64), h.zeros(n, np.int32), h.zeros(n, np.uint64)
    assert k.cdev_lds(h.p(src.ptrs), h.p(src.sizes), h.p(dec.ptrs), h.p(actual), h.p(status), h.p(sums), h.p(rawb.ptrs), h.p(rawb.sizes),
                      h.p(comp.ptrs), h.p(comp.sizes), n, CascadedOpts(*opts), backend.dev.stream()) == 0
    backend.dev.synchronize()
    assert (h.get(status, n, np.int32) == 0).all() and h.get(actual, n, np.uint64).tolist() == [c.size for c in others]
    assert h.get(sums, n, np.uint64).tolist() == [int(c.view(np.uint32).astype(np.uint64).sum(dtype=np.uint64)) for c in others]
    for c, o in zip(others, read_batch(backend.dev, dec, [16384 + GUARD] * n)):
        assert np.array_equal(o[: c.size], c) and (o[c.size:] == 0xA5).all()
    global_path = dev_compress(backend, k, raws, opts)
    for c, g, cc in zip(raws, global_path, read_batch(backend.dev, comp, h.get(comp.sizes, n, np.uint64))):
        assert np.array_equal(cc, g) and np.array_equal(cc, oracle.cascaded_compress(c, *opts))


def _hipcc_or_skip():
    if shutil.which(HIPCC) is None and not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")


def test_header_is_self_contained(tmp_path):
    """A translation unit that includes only nvcomp/device/cascaded.hpp cross-compiles for gfx950 with `-I include` alone
    and defines no device variable; neither umbrella header pulls it in."""
    _hipcc_or_skip()
    only = tmp_path / "only.hip"
    only.write_text("#include <nvcomp/device/cascaded.hpp>\n")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(REPO, "include"),
                        "--cuda-device-only", "-S", str(only), "-o", str(tmp_path / "only.s")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = (tmp_path / "only.s").read_text()
    objects = [line for line in asm.splitlines() if "@object" in line and line.lstrip().startswith(".type")]
    assert len(objects) <= 1, objects  # (the compilation unit's id, which every HIP translation unit carries)
    assert not any(line.lstrip().startswith(".amdhsa_kernel") for line in asm.splitlines())
    for umbrella in ("nvcomp.h", "nvcomp.hpp"):
        r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(REPO, "include"), "-I",
                            "/opt/rocm/include", "-M", "-x", "c++", os.path.join(REPO, "include", umbrella)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "nvcomp/device" not in r.stdout and "cascaded_core" not in r.stdout


HOST_PROGRAM = r"""
#include <nvcomp/device/cascaded.hpp>
#include <cstdio>
#include <cstring>
#include <vector>
namespace dev = nvcomp::device::cascaded;
static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } } while (0)
int main()
{
  const nvcompBatchedCascadedOpts_t ok = {4096, NVCOMP_TYPE_INT, 2, 1, 1};
  CHECK(dev::max_compressed_bytes(65536, ok) == 20 + 12 * 16 + 65536);
  CHECK(dev::max_compressed_bytes(0, ok) == 20);
  CHECK(dev::max_compressed_bytes(((size_t)1 << 24) + 1, ok) == 0);
  CHECK(dev::compress_shared_bytes(ok) == 64 + 4096 + 2048);
  CHECK(dev::decompress_shared_bytes(ok) == 128 + 8192 + 4096 + 2048);
  const nvcompBatchedCascadedOpts_t bad[] = {{4096, (nvcompType_t)8, 2, 1, 1}, {4096, NVCOMP_TYPE_BITS, 2, 1, 1}, {4096, NVCOMP_TYPE_INT, 8, 1, 1},
                                             {4096, NVCOMP_TYPE_INT, -1, 1, 1}, {4096, NVCOMP_TYPE_INT, 2, 8, 1}, {4096, NVCOMP_TYPE_INT, 2, 1, 2},
                                             {255, NVCOMP_TYPE_INT, 2, 1, 1}, {16388, NVCOMP_TYPE_INT, 2, 1, 1}, {4098, NVCOMP_TYPE_INT, 2, 1, 1},
                                             {(size_t)-1, NVCOMP_TYPE_LONGLONG, 7, 7, 1}};
  for (const auto& o : bad) {
    CHECK(dev::max_compressed_bytes(65536, o) == 0);
    CHECK(dev::compress_shared_bytes(o) == 0);
    CHECK(dev::decompress_shared_bytes(o) == 0);
  }
  /* a sound header of {4096, int, 2, 1, 1}, 30 000 bytes, then every truncation of it in a buffer of exactly that size
   * (the sanitizer sees a read past it) and every single damaged field */
  const uint32_t words[5] = {0x43534143u, 4u | (2u << 8) | (1u << 16) | (1u << 24), 30000u, 4096u, 8u};
  for (size_t len = 0; len <= 20; ++len) {
    std::vector<uint32_t> buf((len + 3) / 4 + 1);
    std::memcpy(buf.data(), words, len);
    const void* p = len ? (const void*)buf.data() : nullptr;
    const bool whole = len >= 20;
    CHECK(dev::decompressed_size(p, len) == (whole ? 30000u : 0u));
    CHECK(dev::stream_type(p, len) == (whole ? NVCOMP_TYPE_INT : NVCOMP_TYPE_BITS));
    CHECK(dev::stream_element_bytes(p, len) == (whole ? 4u : 0u));
    CHECK(dev::stream_shared_bytes(p, len) == (whole ? dev::decompress_shared_bytes(ok) : 0u));
  }
  CHECK(dev::decompressed_size(nullptr, 100) == 0 && dev::stream_shared_bytes(nullptr, 100) == 0);
  struct { int word; uint32_t value; } damage[] = {{0, 0x43534142u}, {1, 8u}, {1, 4u | (8u << 8)}, {1, 4u | (8u << 16)}, {3, 0u}, {3, 4098u},
                                                   {2, 30001u}, {3, 4u * 16388u}};
  for (const auto& d : damage) {
    uint32_t b[5];
    std::memcpy(b, words, 20);
    b[d.word] = d.value;
    CHECK(dev::stream_type(b, 20) == NVCOMP_TYPE_BITS);
    CHECK(dev::stream_element_bytes(b, 20) == 0 && dev::stream_shared_bytes(b, 20) == 0);
    CHECK(dev::decompressed_size(b, 20) == (d.word == 0 ? 0u : b[2]));
  }
  /* a misaligned stream reports no size, as the batched query does */
  alignas(8) unsigned char shifted[32];
  std::memcpy(shifted + 1, words, 20);
  CHECK(dev::decompressed_size(shifted + 1, 20) == 0);
  CHECK(dev::stream_type(shifted + 1, 20) == NVCOMP_TYPE_INT);
  for (int t = 0; t < 8; ++t) {
    uint32_t b[5];
    std::memcpy(b, words, 20);
    b[1] = (uint32_t)t | (7u << 8);
    b[2] = 0;
    b[3] = 16384;
    CHECK(dev::stream_type(b, 20) == (nvcompType_t)t && dev::stream_element_bytes(b, 20) == (1u << (t >> 1)));
    const nvcompBatchedCascadedOpts_t o = {16384, (nvcompType_t)t, 7, 0, 1};
    CHECK(dev::stream_shared_bytes(b, 20) == dev::decompress_shared_bytes(o));
  }
  std::printf(fails ? "FAILED\n" : "OK\n");
  return fails != 0;
}
"""


def test_host_queries_under_sanitizers(tmp_path):
    """The host-callable queries in a stand-alone program built with -fsanitize=address,undefined (CPU only): truncated
    and malformed headers, refused options."""
    src = tmp_path / "host_queries.cpp"
    src.write_text(HOST_PROGRAM)
    exe = tmp_path / "host_queries"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(REPO, "tests", "emu"), "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_example_on_gpu():
    exe = os.path.join(REPO, "examples", "bin", "cascaded_device_example")
    r = subprocess.run(["make", "-C", "examples", exe], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "OK" in r.stdout
