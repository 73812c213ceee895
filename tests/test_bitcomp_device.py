"""Device-side Bitcomp API (include/nvcomp/device/bitcomp.hpp): kernels of tests/device_api/bitcomp_device_kernels.hip
call it, on the host emulation and on the MI355X (`backend`). Its streams must be the batched API's byte for byte,
through memory and through element sources, and its decoders -- into memory and into element sinks -- must invert both
compressors' output and the CPU model's (oracle/bitcomp_ref.c), and refuse what the batched decoder refuses."""
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
from nvcomp_amd.batched import make_batch, empty_batch, read_batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "device_api", "bitcomp_device_kernels.hip")
GOLDEN = os.path.join(REPO, "tests", "golden")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MIB = 1 << 20
GUARD = 32

# nvcompType_t codes by element width: (signed, unsigned)
TYPES = {1: (0, 1), 2: (2, 3), 4: (4, 5), 8: (6, 7)}
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}

PARTS = 8  # tests/device_api/bitcomp_device_kernels.hip: -DBCDEV_PART=0 ... 7

_libs = {}


def compile_parts(d, extra):
    """hipcc over the slices of the kernel file, side by side (in one piece the device compiler takes minutes over the
    eighty instantiations of the codec). Returns the object files; the remarks of part p are in <d>/part<p>.log."""
    from concurrent.futures import ThreadPoolExecutor

    def one(p):
        obj = str(d / f"part{p}.o")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(REPO, "include"),
                            f"-DBCDEV_PART={p}", *extra, "-c", SRC, "-o", obj], cwd=REPO, capture_output=True, text=True)
        (d / f"part{p}.log").write_text(r.stderr)
        assert r.returncode == 0, r.stderr[-3000:]
        return obj

    with ThreadPoolExecutor(PARTS) as pool:
        return list(pool.map(one, range(PARTS)))


def kernels(backend, tmp_path_factory):
    """The test kernels built for the backend's tier (once per session)."""
    if backend.name not in _libs:
        d = tmp_path_factory.mktemp(f"bcdev_{backend.name}")
        so = str(d / "bcdev.so")
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
        vp, sz, u, i = C.c_void_p, C.c_size_t, C.c_uint, C.c_int
        lib.bcdev_compress.argtypes = [vp, vp, vp, vp, sz, i, i, u, u, u, vp, vp, vp]
        lib.bcdev_decompress.argtypes = [vp, vp, vp, vp, vp, vp, sz, u, u, u, u, vp, vp, vp]
        lib.bcdev_mixed.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, i, vp, u, u, u, vp]
        lib.bcdev_lds_compress.argtypes = [vp, vp, vp, vp, sz, i, i, u, vp]
        lib.bcdev_lds_decompress.argtypes = [vp, vp, vp, vp, vp, sz, u, vp]
        lib.bcdev_sizes.argtypes = [vp, vp, vp, vp, vp, sz, vp]
        lib.bcdev_quant.argtypes = [vp, vp, vp, sz, u, C.c_double, vp]
        lib.bcdev_quant_compress.argtypes = [vp, vp, vp, vp, sz, C.c_float, i, vp]
        lib.bcdev_fused_axpy.argtypes = [vp, vp, vp, vp, C.c_float, C.c_float, vp, sz, vp]
        lib.bcdev_max_compressed_bytes.argtypes = [sz, i]
        lib.bcdev_max_compressed_bytes.restype = sz
        lib.bcdev_max_chunk_bytes.restype = sz
        _libs[backend.name] = lib
    return _libs[backend.name]


@pytest.fixture
def k(backend, tmp_path_factory):
    return kernels(backend, tmp_path_factory)


class Dev:
    """Small helpers over backend.dev (numpy arrays on the emulator, torch tensors on the card)."""

    def __init__(self, backend):
        self.d = backend.dev

    def zeros(self, n, dtype):
        return self.d.upload(np.zeros(max(n, 1), dtype=dtype).view(np.uint8))

    def get(self, buf, n, dtype):
        return self.d.download(buf).view(dtype)[:n].copy()

    def p(self, buf):
        return self.d.ptr(buf) if buf is not None else None


def grid_for(count, block, chunks_per_wave=1):
    waves = -(-count // chunks_per_wave)
    return max(1, -(-waves // (block // 64)))


def dev_compress(backend, k, chunks, type_code, algo, mode=0, block=256, chunks_per_wave=1):
    """compress() (mode 0) or compress_from() over a memory source (1; 2: a source that counts its calls). Every output
    slot is max_compressed_bytes long and followed by guard bytes that must survive. Returns (streams, flags, counts):
    counts[c] holds, for mode 2, the number of calls the source saw per element (and eight more slots behind)."""
    h = Dev(backend)
    n = len(chunks)
    elem = [w for w, t in TYPES.items() if type_code in t][0]
    src = make_batch(backend.dev, chunks, align=8)
    max_out = int(k.bcdev_max_compressed_bytes(max([c.size for c in chunks] + [1]), type_code))
    dst = empty_batch(backend.dev, [max_out + GUARD] * n, stride=max_out + GUARD, fill=0xA5)
    flags = h.zeros(1, np.uint32)
    cnt = None
    if mode == 2:
        cnt = empty_batch(backend.dev, [4 * (c.size // elem + 8) for c in chunks], align=16, fill=0)
    rc = k.bcdev_compress(h.p(src.ptrs), h.p(src.sizes), h.p(dst.ptrs), h.p(dst.sizes), n, type_code, algo, mode, block,
                          grid_for(n, block, chunks_per_wave), h.p(cnt.ptrs) if cnt else None, h.p(flags),
                          backend.dev.stream())
    assert rc == 0
    backend.dev.synchronize()
    sizes = h.get(dst.sizes, n, np.uint64)
    assert (sizes <= max_out).all()
    host = backend.dev.download(dst.slab)
    for o in dst.offsets:
        assert (host[int(o) + max_out: int(o) + max_out + GUARD] == 0xA5).all(), "the compressor wrote past its bound"
    counts = [c.view(np.uint32) for c in read_batch(backend.dev, cnt)] if cnt else None
    return read_batch(backend.dev, dst, sizes), int(h.get(flags, 1, np.uint32)[0]), counts


def dev_decompress(backend, k, comp, caps, mode=0, elem=1, block=256, chunks_per_wave=1, comp_align=1):
    """decompress() (mode 0) or decompress_to<elem bytes>() (1: storing sink, tail behind the elements; 2: counting sink,
    tail to a side buffer; 3: storing sink, null tail_out). Output slots are filled with 0xA5 (counters: 0) and followed
    by guard bytes that must survive. Returns (whole output slots, actual sizes, statuses, flags, tails)."""
    h = Dev(backend)
    n = len(comp)
    slot = [4 * (c // elem) if mode == 2 else c for c in caps]
    src = make_batch(backend.dev, comp, align=comp_align)
    out = empty_batch(backend.dev, [s + GUARD for s in slot], align=16, fill=0 if mode == 2 else 0xA5)
    out.sizes = backend.dev.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    actual = h.zeros(n, np.uint64)
    status = backend.dev.upload(np.full(n, -1, dtype=np.int32).view(np.uint8))
    flags = h.zeros(1, np.uint32)
    tails = backend.dev.upload(np.full(16 * n + 16, 0xA5, dtype=np.uint8)) if mode == 2 else None
    rc = k.bcdev_decompress(h.p(src.ptrs), h.p(src.sizes), h.p(out.ptrs), h.p(out.sizes), h.p(actual), h.p(status), n, mode,
                            elem, block, grid_for(n, block, chunks_per_wave), h.p(tails), h.p(flags), backend.dev.stream())
    assert rc == 0
    backend.dev.synchronize()
    host = backend.dev.download(out.slab)
    outs = []
    for o, s in zip(out.offsets, slot):
        o = int(o)
        outs.append(host[o: o + s].copy())
        assert (host[o + s: o + s + GUARD] == (0 if mode == 2 else 0xA5)).all(), "a write past the output capacity"
    tail_host = backend.dev.download(tails).reshape(-1, 16)[:n] if mode == 2 else None
    return outs, h.get(actual, n, np.uint64), h.get(status, n, np.int32), int(h.get(flags, 1, np.uint32)[0]), tail_host


def shapes(elem, count, seed=0):
    """The fixed data shapes, `count` elements of `elem` bytes each, as bytes."""
    dt = UNSIGNED[elem]
    rng = np.random.RandomState(seed + 31 * elem + count)
    block = 2048 * max(1, 4 // elem)
    top = np.iinfo(dt).max
    alt = np.where(np.arange(count) % 2 == 0, 5, top - 4).astype(dt)  # +5, -5, +5, ...: the zigzag's two sides
    hole = rng.randint(1, 200, size=count).astype(dt)
    hole[block: 2 * block] = 0  # an all-zero block between two others (where the chunk is that long)
    out = {
        "zeros": np.zeros(count, dt),
        "constant": np.full(count, 77, dt),
        "ramp": np.arange(count).astype(dt),
        "noise": np.frombuffer(rng.bytes(count * elem), dtype=dt).copy(),
        "alternating": alt,
        "zero_block": hole,
    }
    return {name: v.view(np.uint8) for name, v in out.items()}


def edge_counts(elem):
    e = max(1, 4 // elem)
    return [0, 1] + [e * c for c in (63, 64, 65, 2047, 2048, 2049, 4097)] + [e * 64 - 1, e * 2048 + 1]


def corpus(backend, elem):
    """(name, chunk) of one element width: the shapes at every edge count, a ramp with every possible tail, the dataset
    classes at 3 * block + 7 elements and at 65 536 bytes, and one chunk of 1 MiB per class."""
    out = []
    for count in edge_counts(elem):
        for name, c in shapes(elem, count).items():
            out.append((f"{name}/{count}", c))
    ramp = shapes(elem, 2049 * max(1, 4 // elem) + 2)["ramp"]
    for t in range(1, elem):
        out.append((f"tail/{t}", ramp[: ramp.size - elem + t].copy()))
    out.append(("tail/short", ramp[: elem - 1].copy()))  # no element at all, only a tail
    for name, gen in sorted(datasets.CLASSES.items()):
        for n in ((3 * 2048 * max(1, 4 // elem) + 7) * elem, 65536):
            out.append((f"{name}/{n}B", np.ascontiguousarray(gen(n, 3)).view(np.uint8).reshape(-1)[:n].copy()))
        if backend.name == "gpu" or name in ("float_columns", "noise"):
            # the emulator's time goes to the edge sizes; the card runs every class at 1 MiB
            out.append((f"{name}/1MiB", np.ascontiguousarray(gen(MIB, 5)).view(np.uint8).reshape(-1)[:MIB].copy()))
    return out


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_byte_identity_and_cross_decode(backend, oracle, k, elem, algo):
    """compress() == compress_from(memory source) == batched compressor == CPU model, byte for byte; decompress(),
    decompress_to(storing sink) and the batched decoder each invert the streams; sizes and widths are reported as the
    batched API reports them. Signed and unsigned type codes write the same bytes."""
    names, chunks = zip(*corpus(backend, elem))
    signed, unsigned = TYPES[elem]
    codec = backend.codec("Bitcomp", (algo, unsigned))
    dev_comp, flags, _ = dev_compress(backend, k, chunks, unsigned, algo)
    assert flags == 0
    bat_comp = codec.compress(chunks)
    whole = [i for i, c in enumerate(chunks) if c.size % elem == 0]  # compress_from takes elements: no tail
    src_comp, flags, _ = dev_compress(backend, k, [chunks[i] for i in whole], unsigned, algo, mode=1)
    assert flags == 0
    for name, c, dc, bc in zip(names, chunks, dev_comp, bat_comp):
        assert np.array_equal(dc, bc), f"{name}: device and batched streams differ"
        assert np.array_equal(dc, oracle.bitcomp_compress(c, algo, elem)), f"{name}: the CPU model writes other bytes"
    for i, sc in zip(whole, src_comp):
        assert np.array_equal(sc, dev_comp[i]), f"{names[i]}: compress_from and compress streams differ"
    sub = [i for i, n in enumerate(names) if n.split("/")[1] in ("0", "1", str(2049 * max(1, 4 // elem))) or n.startswith("tail")]
    sgn_comp, flags, _ = dev_compress(backend, k, [chunks[i] for i in sub], signed, algo)
    assert flags == 0 and all(np.array_equal(s, dev_comp[i]) for i, s in zip(sub, sgn_comp))
    sgn_bat = backend.codec("Bitcomp", (algo, signed)).compress([chunks[i] for i in sub])
    assert all(np.array_equal(s, dev_comp[i]) for i, s in zip(sub, sgn_bat))

    caps = [c.size for c in chunks]
    for mode in (0, 1):
        outs, actual, status, flags, _ = dev_decompress(backend, k, dev_comp, caps, mode=mode, elem=elem)
        assert flags == 0 and (status == NvcompStatus.Success).all(), (mode, status)
        assert actual.tolist() == caps
        for name, c, o in zip(names, chunks, outs):
            assert np.array_equal(o, c), (mode, name)
    b_outs, b_actual, b_status = codec.decompress(dev_comp, caps)
    assert (b_status == NvcompStatus.Success).all() and b_actual.tolist() == caps
    assert all(np.array_equal(o, c) for o, c in zip(b_outs, chunks))
    h = Dev(backend)
    n = len(chunks)
    src = make_batch(backend.dev, dev_comp)
    sizes, elems, types = h.zeros(n, np.uint64), h.zeros(n, np.uint32), h.zeros(n, np.int32)
    assert k.bcdev_sizes(h.p(src.ptrs), h.p(src.sizes), h.p(sizes), h.p(elems), h.p(types), n, backend.dev.stream()) == 0
    backend.dev.synchronize()
    assert h.get(sizes, n, np.uint64).tolist() == codec.get_decompress_size(dev_comp).tolist() == caps
    assert (h.get(elems, n, np.uint32) == elem).all() and (h.get(types, n, np.int32) == unsigned).all()


OWN = [s for s in json.load(open(os.path.join(GOLDEN, "own_manifest.json")))["streams"] if s["format"] == "Bitcomp"]


@pytest.mark.parametrize("rec", OWN, ids=[s["file"] for s in OWN])
def test_golden_streams(backend, oracle, k, rec):
    """The committed Bitcomp streams: compress() and compress_from() reproduce them, both decoders invert them."""
    stream = np.fromfile(os.path.join(GOLDEN, rec["file"]), dtype=np.uint8)
    assert hashlib.sha256(stream.tobytes()).hexdigest() == rec["stream_sha256"]
    rc, chunk = oracle.lz4_decompress(np.fromfile(os.path.join(GOLDEN, rec["source"]), dtype=np.uint8), rec["bytes"])
    assert rc == 0 and hashlib.sha256(chunk.tobytes()).hexdigest() == rec["sha256"]
    algo, type_code = rec["opts"]
    elem = [w for w, t in TYPES.items() if type_code in t][0]
    for mode in (0, 1) if chunk.size % elem == 0 else (0,):
        (made,), flags, _ = dev_compress(backend, k, [chunk], type_code, algo, mode=mode)
        assert flags == 0 and np.array_equal(made, stream), f"mode {mode}: bytes differ from the committed golden stream"
    for mode in (0, 1):
        (out,), actual, status, flags, _ = dev_decompress(backend, k, [stream], [chunk.size], mode=mode, elem=elem)
        assert flags == 0 and status[0] == 0 and actual[0] == chunk.size and np.array_equal(out, chunk)


def test_decodes_oracle_streams_unaligned(backend, oracle, k):
    """The CPU model's streams, packed tight (any alignment of `in`), through decompress() and a storing sink."""
    chunks = [(datasets.float_columns(70000, 2), 4), (datasets.int32_column(4100, 1), 4), (np.arange(5000, dtype=np.uint8), 1),
              (np.zeros(5, np.uint8), 2), (datasets.noise(8200, 4), 8), (datasets.lowcard(8197, 3), 2)]
    for algo in (0, 1):
        for c, elem in chunks:
            c = np.ascontiguousarray(c).view(np.uint8).reshape(-1)
            comp = [oracle.bitcomp_compress(c, algo, elem)] * 3  # three copies: odd offsets in the slab
            for mode in (0, 1):
                outs, actual, status, flags, _ = dev_decompress(backend, k, comp, [c.size] * 3, mode=mode, elem=elem)
                assert flags == 0 and (status == 0).all() and actual.tolist() == [c.size] * 3
                assert all(np.array_equal(o, c) for o in outs)


def test_constants_and_refusals(backend, k):
    """kMaxChunkBytes and max_compressed_bytes are the batched API's; a type or algorithm it refuses gives 0 and writes
    nothing; on the card, so does a chunk of kMaxChunkBytes + 1."""
    assert k.bcdev_max_chunk_bytes() == 1 << 24
    for elem, (signed, unsigned) in TYPES.items():
        codec = backend.codec("Bitcomp", (0, unsigned))
        for n in (0, 1, 7, 2048, 65536, 65543, 1 << 24):
            assert k.bcdev_max_compressed_bytes(n, unsigned) == k.bcdev_max_compressed_bytes(n, signed) == codec.max_compressed_size(n)
    assert k.bcdev_max_compressed_bytes(100, 0xff) == 0 and k.bcdev_max_compressed_bytes(100, 8) == 0
    h = Dev(backend)
    c = np.arange(1000, dtype=np.uint32).view(np.uint8)
    for type_code, algo in ((0xff, 0), (8, 0), (5, 2), (5, -1)):
        src = make_batch(backend.dev, [c], align=8)
        dst = empty_batch(backend.dev, [8192], fill=0xA5)
        flags = h.zeros(1, np.uint32)
        assert k.bcdev_compress(h.p(src.ptrs), h.p(src.sizes), h.p(dst.ptrs), h.p(dst.sizes), 1, type_code, algo, 0, 64, 1,
                                None, h.p(flags), backend.dev.stream()) == 0
        backend.dev.synchronize()
        assert h.get(dst.sizes, 1, np.uint64)[0] == 0 and (backend.dev.download(dst.slab) == 0xA5).all()
    if backend.name == "gpu":
        big = np.full((1 << 24) + 1, 3, np.uint8)
        for mode in (0, 1):
            comp, flags, _ = dev_compress(backend, k, [big], 1, 0, mode=mode)
            assert flags == 0 and comp[0].size == 0


@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_sink_contract(backend, oracle, k, elem):
    """A counting sink sees every element exactly once and none at or beyond n / sizeof(T); tail_out receives exactly
    the tail bytes; a null tail_out is accepted; a stream of another width is nvcompErrorInvalidValue, no sink call."""
    e = max(1, 4 // elem)
    rng = np.random.RandomState(elem)
    sizes = [0, elem - 1, elem, elem * (64 * e - 1) + elem // 2, elem * (64 * e + 1), elem * (2048 * e - 1),
             elem * (2048 * e + 1) + elem - 1, elem * (3 * 2048 * e + 70 * e + 1) + elem - 1]
    chunks = [rng.randint(0, 256, n).astype(np.uint8) for n in sizes] + [shapes(elem, 2048 * e * 3 + 5)["zero_block"]]
    for algo in (0, 1):
        comp = [oracle.bitcomp_compress(c, algo, elem) for c in chunks]
        caps = [c.size + 3 * elem for c in chunks]  # room the sink must not be handed
        outs, actual, status, flags, tails = dev_decompress(backend, k, comp, caps, mode=2, elem=elem)
        assert flags == 0 and (status == 0).all() and actual.tolist() == [c.size for c in chunks]
        for c, o, t in zip(chunks, outs, tails):
            counts = o.view(np.uint32)
            n_el, n_tail = c.size // elem, c.size % elem
            assert (counts[:n_el] == 1).all(), "an element was handed to the sink other than once"
            assert (counts[n_el:] == 0).all(), "the sink saw an element at or beyond n / sizeof(T)"
            assert np.array_equal(t[:n_tail], c[c.size - n_tail:]) and (t[n_tail:] == 0xA5).all()
        for mode in (1, 3):
            outs, actual, status, flags, _ = dev_decompress(backend, k, comp, caps, mode=mode, elem=elem)
            assert flags == 0 and (status == 0).all()
            for c, o in zip(chunks, outs):
                kept = c.size if mode == 1 else c.size // elem * elem  # mode 3: tail_out is null, the tail is dropped
                assert np.array_equal(o[:kept], c[:kept]) and (o[kept:] == 0xA5).all()
        other = 2 if elem != 2 else 4
        outs, actual, status, flags, tails = dev_decompress(backend, k, comp, caps, mode=2, elem=other)
        assert flags == 0 and (status == NvcompStatus.ErrorInvalidValue).all() and (actual == 0).all()
        assert all((o == 0).all() for o in outs) and (tails == 0xA5).all()


@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_source_contract(backend, oracle, k, elem):
    """A counting source is called exactly once per element and never for an index >= n_elems, the partial last row and
    block included; what it yields is what is compressed."""
    e = max(1, 4 // elem)
    counts_el = [0, 1, 64 * e - 1, 64 * e + 1, 2048 * e - 1, 2048 * e, 2048 * e + 1, 3 * 2048 * e + 70 * e + 1]
    rng = np.random.RandomState(10 + elem)
    chunks = [rng.randint(0, 256, n * elem).astype(np.uint8) for n in counts_el]
    for algo in (0, 1):
        comp, flags, counts = dev_compress(backend, k, chunks, TYPES[elem][1], algo, mode=2)
        assert flags == 0, "the source was asked for an element at or beyond n_elems"
        for c, cc, cnt in zip(chunks, comp, counts):
            n_el = c.size // elem
            assert (cnt[:n_el] == 1).all() and (cnt[n_el:] == 0).all()
            assert np.array_equal(cc, oracle.bitcomp_compress(c, algo, elem))


def corruptions(stream, elem, n):
    """(label, bad stream) pairs, deterministic. `stream` codes n bytes of noise: more than one block, the first one
    whole and packed; the tail cases exist where n % elem != 0."""
    tail = n % elem
    assert stream[12] != 0xFF and n // elem > 2048 * max(1, 4 // elem) and (tail != 0 or elem == 1)
    out = []
    for label, at, value in (("magic", 0, stream[0] ^ 0x20), ("version", 3, 2), ("algo", 4, 2), ("width code", 5, 4),
                             ("reserved", 6, 1), ("reserved high", 7, 0x80), ("row width", 12, 8 * elem + 1),
                             ("width of the last row", 12 + 31, 8 * elem + 1)):
        b = stream.copy()
        b[at] = value
        out.append((label, b))
    out += [("empty", stream[:0]), ("eleven bytes", stream[:11]), ("header only", stream[:12]), ("in the widths", stream[:14]),
            ("in the payload", stream[: 12 + 32 + 1000]), ("payload one dword short", stream[: stream.size - tail - 4])]
    if tail:
        out.append(("in the tail", stream[:-1]))
    return out


@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_errors_match_batched(backend, oracle, k, elem):
    """Every corruption is rejected by the CPU model, and gives nvcompErrorCannotDecompress exactly where the batched
    decoder does -- through decompress() and through decompress_to(); a capacity one byte short is refused with nothing
    written and *decompressed_bytes == 0."""
    e = max(1, 4 // elem)
    n = elem * (2048 * e + 300 * e) + elem - 1
    rng = np.random.RandomState(20 + elem)
    cases, caps, short = [], [], []
    for algo in (0, 1):
        src = rng.randint(0, 256, n).astype(np.uint8)
        stream = oracle.bitcomp_compress(src, algo, elem)
        for label, b in corruptions(stream, elem, n):
            rc, _ = oracle.bitcomp_decompress(b, n)
            assert rc != 0, f"the CPU model accepts '{label}': a bug in this test"
            cases.append(b)
            caps.append(n)
        rc, _ = oracle.bitcomp_decompress(stream, n - 1)
        assert rc != 0
        short.append(len(cases))
        cases.append(stream)
        caps.append(n - 1)
    codec = backend.codec("Bitcomp", (0, TYPES[elem][1]))
    _, b_actual, b_status = codec.decompress(cases, caps)
    assert (b_status == NvcompStatus.ErrorCannotDecompress).all()
    for mode in (0, 1):
        outs, actual, status, flags, _ = dev_decompress(backend, k, cases, caps, mode=mode, elem=elem)
        assert flags == 0
        assert status.tolist() == b_status.tolist(), mode
        assert actual.tolist() == b_actual.tolist() and (actual == 0).all()
        for i in short:
            assert (outs[i] == 0xA5).all(), "a refused capacity, yet something was written"


@pytest.mark.parametrize("block", [64, 256, 1024])
@pytest.mark.parametrize("chunks_per_wave", [1, 3])
def test_launch_shapes(backend, oracle, k, block, chunks_per_wave):
    """Workgroups of 1, 4 and 16 waves; waves that loop over several chunks."""
    rng = np.random.RandomState(block + chunks_per_wave)
    count = 16 if backend.name == "emu" else 600
    elem, algo = (4, 0) if chunks_per_wave == 1 else (2, 1)
    gens = sorted(datasets.CLASSES)
    chunks = [np.ascontiguousarray(datasets.CLASSES[gens[i % len(gens)]](9000, i)).view(np.uint8).reshape(-1)
              [: int(rng.randint(0, 9000))].copy() for i in range(count)]
    for mode in (0, 1):
        use = chunks if mode == 0 else [c[: c.size // elem * elem] for c in chunks]
        comp, flags, _ = dev_compress(backend, k, use, TYPES[elem][1], algo, mode=mode, block=block,
                                      chunks_per_wave=chunks_per_wave)
        assert flags == 0
        for c, cc in zip(use, comp):
            assert np.array_equal(cc, oracle.bitcomp_compress(c, algo, elem))
    caps = [c.size for c in use]
    for mode in (0, 1):
        outs, actual, status, flags, _ = dev_decompress(backend, k, comp, caps, mode=mode, elem=elem, block=block,
                                                        chunks_per_wave=chunks_per_wave)
        assert flags == 0 and (status == 0).all() and actual.tolist() == caps
        assert all(np.array_equal(o, c) for o, c in zip(outs, use))


@pytest.mark.parametrize("block", [256, 1024])
def test_mixed_workgroup(backend, oracle, k, block):
    """In every workgroup odd waves compress while even waves decompress and the last wave only spins on arithmetic: the
    calls contain no workgroup barrier."""
    h = Dev(backend)
    pairs = (block // 64 - 1) // 2
    count = 2 * pairs if backend.name == "emu" else 70 * pairs
    grid = -(-count // pairs)
    iters = 2000
    raw = [np.ascontiguousarray(datasets.float_columns(3000 + 996 * (i % 7), i)).view(np.uint8) for i in range(count)]
    other = [np.ascontiguousarray(datasets.int32_column(2000 + 1000 * (i % 5), i)).view(np.uint8) for i in range(count)]
    comp_in = [oracle.bitcomp_compress(c, 0, 4) for c in other]
    caps = [c.size for c in other]
    src = make_batch(backend.dev, comp_in)
    out = empty_batch(backend.dev, [c + GUARD for c in caps], align=16, fill=0xA5)
    out.sizes = backend.dev.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    actual = h.zeros(count, np.uint64)
    status = backend.dev.upload(np.full(count, -1, dtype=np.int32).view(np.uint8))
    rawb = make_batch(backend.dev, raw, align=8)
    max_out = int(k.bcdev_max_compressed_bytes(max(c.size for c in raw), 5))
    dst = empty_batch(backend.dev, [max_out] * count, stride=max_out)
    side = h.zeros(grid * 64, np.uint32)
    assert k.bcdev_mixed(h.p(src.ptrs), h.p(src.sizes), h.p(out.ptrs), h.p(out.sizes), h.p(actual), h.p(status),
                         h.p(rawb.ptrs), h.p(rawb.sizes), h.p(dst.ptrs), h.p(dst.sizes), count, 0, h.p(side), iters, block,
                         grid, backend.dev.stream()) == 0
    backend.dev.synchronize()
    assert (h.get(status, count, np.int32) == 0).all() and h.get(actual, count, np.uint64).tolist() == caps
    host = backend.dev.download(out.slab)
    for o, c, cap in zip(out.offsets, other, caps):
        assert np.array_equal(host[int(o): int(o) + cap], c) and (host[int(o) + cap: int(o) + cap + GUARD] == 0xA5).all()
    for c, cc in zip(raw, read_batch(backend.dev, dst, h.get(dst.sizes, count, np.uint64))):
        assert np.array_equal(cc, oracle.bitcomp_compress(c, 0, 4))
    x = np.arange(1, grid * 64 + 1, dtype=np.uint32)  # lane t of the spinning waves starts at t + 1
    for _ in range(iters):
        x ^= x << np.uint32(13)
        x ^= x >> np.uint32(17)
        x ^= x << np.uint32(5)
    assert np.array_equal(h.get(side, x.size, np.uint32), x)


@pytest.mark.parametrize("misalign", [0, 3])
def test_in_and_out_in_lds(backend, oracle, k, misalign):
    """A chunk staged in LDS (at offsets 0 and 3 mod 4), wave_sync(), compressed to global memory; a stream decoded into
    LDS and copied out."""
    h = Dev(backend)
    for elem, algo in ((4, 0), (1, 0), (8, 1), (2, 0)):
        chunks = [datasets.float_columns(6144, 1), np.zeros(0, np.uint8), np.full(3000, 9, np.uint8), datasets.int32_column(2052, 2),
                  np.random.RandomState(1).randint(0, 256, 5001).astype(np.uint8), datasets.lowcard(777, 3)]
        chunks = [np.ascontiguousarray(c).view(np.uint8).reshape(-1)[:6144].copy() for c in chunks]
        n = len(chunks)
        ref = [oracle.bitcomp_compress(c, algo, elem) for c in chunks]
        src = make_batch(backend.dev, chunks)
        max_out = int(k.bcdev_max_compressed_bytes(6144, TYPES[elem][1]))
        comp = empty_batch(backend.dev, [max_out] * n, stride=max_out)
        assert k.bcdev_lds_compress(h.p(src.ptrs), h.p(src.sizes), h.p(comp.ptrs), h.p(comp.sizes), n, TYPES[elem][1], algo,
                                    misalign, backend.dev.stream()) == 0
        backend.dev.synchronize()
        for cc, r in zip(read_batch(backend.dev, comp, h.get(comp.sizes, n, np.uint64)), ref):
            assert np.array_equal(cc, r)
        streams = make_batch(backend.dev, ref)
        dec = empty_batch(backend.dev, [6144] * n, stride=6144)
        actual, status = h.zeros(n, np.uint64), h.zeros(n, np.int32)
        assert k.bcdev_lds_decompress(h.p(streams.ptrs), h.p(streams.sizes), h.p(dec.ptrs), h.p(actual), h.p(status), n,
                                      misalign, backend.dev.stream()) == 0
        backend.dev.synchronize()
        assert (h.get(status, n, np.int32) == 0).all() and h.get(actual, n, np.uint64).tolist() == [c.size for c in chunks]
        for c, o in zip(chunks, read_batch(backend.dev, dec, [c.size for c in chunks])):
            assert np.array_equal(o, c)


FP = {2: (np.float16, np.float32, np.int16), 4: (np.float32, np.float32, np.int32), 8: (np.float64, np.float64, np.int64)}
DELTAS = (1e-3, 0.25, 3.0)


def lossy_values(width, delta):
    """Normal values, values next to .5 quotients, +-inf, NaN, +-0, subnormals and saturating magnitudes."""
    ft, work, it = FP[width]
    rng = np.random.RandomState(width)
    fi = np.finfo(ft)
    normal = (rng.standard_normal(3000) * 50).astype(ft)
    halves = ((np.arange(-300, 300).astype(work) + work(0.5)) * work(delta)).astype(ft)
    near = np.concatenate([halves, np.nextafter(halves, ft(np.inf)), np.nextafter(halves, ft(-np.inf))])
    special = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, fi.tiny, -fi.tiny, fi.tiny / 4, -fi.tiny / 4, fi.max, -fi.max,
                        fi.max / 2, 1.0, -1.0], dtype=ft)
    info = np.iinfo(it)
    with np.errstate(all="ignore"):
        edge = (np.array([info.max, info.min], dtype=work) * work(delta)).astype(ft)
        big = np.concatenate([edge, np.nextafter(edge, ft(np.inf)), np.nextafter(edge, ft(-np.inf)), edge * ft(2)])
    return np.concatenate([normal, near, special, big]).astype(ft)


def model_quantize(x, delta, width):
    """np.rint(x / delta) in fp32 (fp16 widened exactly, fp32) or fp64, saturated to the signed integer, NaN -> 0."""
    ft, work, it = FP[width]
    info = np.iinfo(it)
    with np.errstate(all="ignore"):
        q = np.rint(x.astype(work) / work(delta))
        hi, lo = work(info.max), work(info.min)  # 2^31 - 1 and 2^63 - 1 round up to the power of two, as in the kernel
        mid = ~(np.isnan(q) | (q >= hi) | (q <= lo))
        out = np.zeros(x.size, dtype=it)
        out[q >= hi] = info.max
        out[q <= lo] = info.min
        out[mid] = q[mid].astype(it)
    return out


def model_dequantize(q, delta, width):
    ft, work, it = FP[width]
    with np.errstate(all="ignore"):
        return (q.astype(work) * work(delta)).astype(ft)


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("width", [2, 4, 8])
def test_lossy_helpers(backend, k, width, delta):
    """quantize / dequantize equal numpy's rint(x / delta), saturated, NaN -> 0, and q * delta, bit for bit."""
    h = Dev(backend)
    ft, work, it = FP[width]
    x = lossy_values(width, delta)
    xd = backend.dev.upload(x.view(np.uint8))
    qd, bd = h.zeros(x.size, it), h.zeros(x.size, ft)
    assert k.bcdev_quant(h.p(xd), h.p(qd), h.p(bd), x.size, width, delta, backend.dev.stream()) == 0
    backend.dev.synchronize()
    q = h.get(qd, x.size, it)
    want = model_quantize(x, delta, width)
    assert np.array_equal(q, want), np.flatnonzero(q != want)[:10]
    back = h.get(bd, x.size, UNSIGNED[width])
    assert np.array_equal(back, model_dequantize(want, delta, width).view(UNSIGNED[width]))


@pytest.mark.parametrize("algo", [0, 1])
def test_quantising_source(backend, k, algo):
    """compress_from with a quantising source == the batched compressor over the numpy-quantised integers."""
    h = Dev(backend)
    delta = 1e-3
    xs = [np.ascontiguousarray(datasets.float32_column(4 * n, n)).view(np.float32)[:n].copy() for n in (0, 1, 65, 2049, 4097, 16384)]
    xs.append(lossy_values(4, delta))
    want = backend.codec("Bitcomp", (algo, 4)).compress([model_quantize(x, delta, 4).view(np.uint8) for x in xs])
    n = len(xs)
    src = make_batch(backend.dev, [x.view(np.uint8) for x in xs], align=8)
    max_out = int(k.bcdev_max_compressed_bytes(max(x.size * 4 for x in xs), 4))
    dst = empty_batch(backend.dev, [max_out] * n, stride=max_out)
    assert k.bcdev_quant_compress(h.p(src.ptrs), h.p(src.sizes), h.p(dst.ptrs), h.p(dst.sizes), n, delta, algo,
                                  backend.dev.stream()) == 0
    backend.dev.synchronize()
    for w, got in zip(want, read_batch(backend.dev, dst, h.get(dst.sizes, n, np.uint64))):
        assert np.array_equal(got, w)


def test_fused_axpy(backend, oracle, k):
    """y += a * dequantize(q) through decompress_to == the two-step numpy computation, bit for bit (fp32, the order
    y + (a * (q * delta)), each step rounded)."""
    h = Dev(backend)
    a, delta = np.float32(0.37), np.float32(1e-3)
    rng = np.random.RandomState(6)
    counts = (16384, 4099, 2048, 100, 0, 16403)
    qs = [model_quantize(np.ascontiguousarray(datasets.float32_column(4 * n + 4, n)).view(np.float32)[:n], delta, 4) for n in counts]
    ys = [rng.standard_normal(n).astype(np.float32) for n in counts]
    comp = [oracle.bitcomp_compress(q.view(np.uint8), 0, 4) for q in qs]
    n = len(counts)
    src = make_batch(backend.dev, comp)
    yb = make_batch(backend.dev, [y.view(np.uint8) for y in ys], align=16)
    caps = backend.dev.upload(np.asarray([4 * c for c in counts], dtype=np.uint64).view(np.uint8))
    status = backend.dev.upload(np.full(n, -1, dtype=np.int32).view(np.uint8))
    assert k.bcdev_fused_axpy(h.p(src.ptrs), h.p(src.sizes), h.p(caps), h.p(yb.ptrs), a, delta, h.p(status), n,
                              backend.dev.stream()) == 0
    backend.dev.synchronize()
    assert (h.get(status, n, np.int32) == 0).all()
    for q, y, got in zip(qs, ys, read_batch(backend.dev, yb)):
        want = y + a * (q.astype(np.float32) * delta)
        assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _hipcc_or_skip():
    if shutil.which(HIPCC) is None and not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")


def test_header_is_self_contained(tmp_path):
    """A translation unit that includes only nvcomp/device/bitcomp.hpp, and the test kernels with every entry point,
    cross-compile for gfx950 with `-I include` alone; the kernels that only call the API have no LDS."""
    _hipcc_or_skip()
    only = tmp_path / "only.hip"
    only.write_text("#include <nvcomp/device/bitcomp.hpp>\n")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(REPO, "include"),
                        "--cuda-device-only", "-c", str(only), "-o", str(tmp_path / "only.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    compile_parts(tmp_path, ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"])
    remarks = "".join((tmp_path / f"part{p}.log").read_text() for p in range(PARTS))
    lds, name = {}, None
    for line in remarks.splitlines():
        if "Function Name:" in line:
            name = line.split("Function Name:")[1].split()[0]
        elif "LDS Size [bytes/block]:" in line:
            lds[name] = int(line.split("LDS Size [bytes/block]:")[1].split()[0])
    api_only = [n for n in lds if "k_lds_" not in n]
    assert len(api_only) == 15 and all(lds[n] == 0 for n in api_only), lds  # every width of the templates, and the rest
    staged = [n for n in lds if "k_lds_" in n]
    assert len(staged) == 2 and all(lds[n] == 4 * (6144 + 16) for n in staged), lds  # the test's own staging buffers only


def test_not_in_the_umbrella_headers(tmp_path):
    """nvcomp.h still compiles as C; neither nvcomp.h nor nvcomp.hpp pulls the device header in."""
    src = tmp_path / "t.c"
    src.write_text('#include "nvcomp.h"\nint main(void){return (int)nvcompSuccess;}\n')
    subprocess.run(["gcc", "-std=c99", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(REPO, "include"), "-I", "/opt/rocm/include",
                    "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
    for umbrella in ("nvcomp.h", "nvcomp.hpp"):
        r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(REPO, "include"), "-I",
                            "/opt/rocm/include", "-M", "-x", "c++", os.path.join(REPO, "include", umbrella)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "nvcomp/device" not in r.stdout and "bitcomp_core" not in r.stdout


@pytest.mark.gpu
def test_example_on_gpu():
    exe = os.path.join(REPO, "examples", "bin", "bitcomp_device_example")
    r = subprocess.run(["make", "-C", "examples", exe], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "OK" in r.stdout
