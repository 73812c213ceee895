"""Device-side ANS API (include/nvcomp/device/ans.hpp): kernels of tests/device_api/ans_device_kernels.hip call it, on
the host emulation and on the MI355X (`backend`). Its streams must be the batched API's byte for byte, and both
decoders must invert both compressors' output and the CPU model's (oracle/ans_ref.c)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from nvcomp_amd import datasets
from nvcomp_amd._lib import NvcompStatus
from nvcomp_amd.batched import make_batch, empty_batch, read_batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "device_api", "ans_device_kernels.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MIB = 1 << 20

_libs = {}


def kernels(backend, tmp_path_factory):
    """The test kernels built for the backend's tier (once per session)."""
    if backend.name not in _libs:
        d = tmp_path_factory.mktemp(f"ansdev_{backend.name}")
        so = str(d / "ansdev.so")
        if backend.name == "emu":
            import conftest

            conftest.emu_library()
            cmd = ["g++", "-O1", "-std=c++17", "-x", "c++", "-shared", "-fPIC", "-Itests/emu", "-Iinclude", SRC, "-o", so,
                   "-Ltests/emu", "-lnvcomp_emu", f"-Wl,-rpath,{REPO}/tests/emu"]
        else:
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Iinclude", SRC, "-o", so]
        r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        lib = C.CDLL(so)
        vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
        lib.ansdev_compress.argtypes = [vp, vp, vp, vp, sz, u, u, vp, vp]
        lib.ansdev_decompress.argtypes = [vp, vp, vp, vp, vp, vp, sz, u, u, u, vp, vp]
        lib.ansdev_mixed.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, u, u, u, vp, vp]
        lib.ansdev_lds_roundtrip.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz, u, vp, vp]
        lib.ansdev_sizes.argtypes = [vp, vp, vp, sz, vp]
        lib.ansdev_codebook.argtypes = [vp, vp, vp, vp, vp, u, vp, sz, vp]
        lib.ansdev_max_compressed_bytes.argtypes = [sz]
        lib.ansdev_max_compressed_bytes.restype = sz
        lib.ansdev_shared_bytes.argtypes = [C.c_int]
        lib.ansdev_shared_bytes.restype = sz
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
        return self.d.upload(np.zeros(n, dtype=dtype).view(np.uint8))

    def get(self, buf, n, dtype):
        return self.d.download(buf).view(dtype)[:n].copy()

    def p(self, buf):
        return self.d.ptr(buf) if buf is not None else None


def grid_for(count, block, chunks_per_wave=1):
    waves = -(-count // chunks_per_wave)
    return max(1, -(-waves // (block // 64)))


def dev_compress(backend, k, chunks, block=256, chunks_per_wave=1):
    """Device compress(): (compressed chunks, guard flags)."""
    h = Dev(backend)
    n = len(chunks)
    src = make_batch(backend.dev, chunks, align=8)
    max_out = int(k.ansdev_max_compressed_bytes(max([c.size for c in chunks] + [1])))
    dst = empty_batch(backend.dev, [max_out] * n, stride=max_out)
    flags = h.zeros(1, np.uint32)
    rc = k.ansdev_compress(h.p(src.ptrs), h.p(src.sizes), h.p(dst.ptrs), h.p(dst.sizes), n, block,
                           grid_for(n, block, chunks_per_wave), h.p(flags), backend.dev.stream())
    assert rc == 0
    backend.dev.synchronize()
    sizes = h.get(dst.sizes, n, np.uint64)
    return read_batch(backend.dev, dst, sizes), int(h.get(flags, 1, np.uint32)[0])


def dev_decompress(backend, k, comp, caps, mode=0, block=256, chunks_per_wave=1, comp_align=1, pad=32):
    """Device decompress() (mode 0) or decompress_to() (1: store sink, 2: counting sink). Output slots are followed by
    `pad` guard bytes that must survive. Returns (outputs, actual sizes, statuses, flags)."""
    h = Dev(backend)
    n = len(comp)
    unit = 4 if mode == 2 else 1
    src = make_batch(backend.dev, comp, align=comp_align)
    out = empty_batch(backend.dev, [c * unit + pad for c in caps], align=16, fill=0 if mode == 2 else 0xA5)
    out.sizes = backend.dev.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    actual = h.zeros(n, np.uint64)
    status = backend.dev.upload(np.full(n, -1, dtype=np.int32).view(np.uint8))
    flags = h.zeros(1, np.uint32)
    rc = k.ansdev_decompress(h.p(src.ptrs), h.p(src.sizes), h.p(out.ptrs), h.p(out.sizes), h.p(actual), h.p(status), n, mode,
                             block, grid_for(n, block, chunks_per_wave), h.p(flags), backend.dev.stream())
    assert rc == 0
    backend.dev.synchronize()
    host = backend.dev.download(out.slab)
    outs = []
    for o, c in zip(out.offsets, caps):
        o = int(o)
        outs.append(host[o: o + c * unit].copy())
        if mode != 2:
            assert (host[o + c: o + c + pad] == 0xA5).all(), "the decoder wrote past the output capacity"
        else:
            assert (host[o + 4 * c: o + 4 * c + pad] == 0).all(), "the sink was handed bytes past the capacity"
    return outs, h.get(actual, n, np.uint64), h.get(status, n, np.int32), int(h.get(flags, 1, np.uint32)[0])


def kinds(n, seed):
    """The data of the byte-identity test: fixed shapes and the dataset classes."""
    rng = np.random.RandomState(seed + n)
    out = {
        "zeros": np.zeros(n, np.uint8),
        "two_symbols": (rng.rand(n) < 0.3).astype(np.uint8) * 77,
        "all_256": np.resize(rng.permutation(256).astype(np.uint8), n),
        "skewed": np.minimum(rng.geometric(0.35, size=n), 255).astype(np.uint8),
        "random": rng.randint(0, 256, n).astype(np.uint8),
    }
    for name, gen in sorted(datasets.CLASSES.items()):
        out[name] = np.ascontiguousarray(gen(max(n, 64), seed)).view(np.uint8).reshape(-1)[:n].copy()
    return out


SIZES = [0, 1, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4099, 65536, 65613, MIB]


def corpus(backend):
    chunks, names = [], []
    for n in SIZES:
        for name, c in kinds(n, 3).items():
            if n == MIB and backend.name == "emu" and name not in ("skewed", "random", "text"):
                continue  # the emulator's time goes to the edge sizes; the card runs every class at 1 MiB
            assert c.size == n, (name, n)
            chunks.append(c)
            names.append(f"{name}/{n}")
    if backend.name == "gpu":
        big = np.minimum(np.random.RandomState(9).geometric(0.2, size=16 * MIB), 255).astype(np.uint8)
        chunks.append(big)
        names.append("skewed/16MiB")
    return chunks, names


def test_byte_identity_and_cross_decode(backend, oracle, k):
    """Device compress == batched compress == CPU model; device decompress inverts all of them and the batched decoder
    inverts the device streams; decompressed_size == GetDecompressSizeAsync."""
    chunks, names = corpus(backend)
    codec = backend.codec("ANS")
    dev_comp, flags = dev_compress(backend, k, chunks, block=256)
    assert flags == 0
    bat_comp = codec.compress(chunks)
    for name, c, dc, bc in zip(names, chunks, dev_comp, bat_comp):
        assert dc.size == bc.size and np.array_equal(dc, bc), f"{name}: device and batched streams differ"
        assert dc.size <= c.size + 12
        if c.size <= MIB:
            ref = oracle.ans_compress(c)
            assert np.array_equal(dc, ref), f"{name}: the CPU model writes other bytes"
    caps = [c.size for c in chunks]
    outs, actual, status, flags = dev_decompress(backend, k, dev_comp, caps)
    assert flags == 0 and (status == NvcompStatus.Success).all(), status
    assert actual.tolist() == caps
    for name, c, o in zip(names, chunks, outs):
        assert np.array_equal(o, c), name
    b_outs, b_actual, b_status = codec.decompress(dev_comp, caps)
    assert (b_status == NvcompStatus.Success).all() and b_actual.tolist() == caps
    assert all(np.array_equal(o, c) for o, c in zip(b_outs, chunks))
    h = Dev(backend)
    src = make_batch(backend.dev, dev_comp)
    sizes = h.zeros(len(chunks), np.uint64)
    assert k.ansdev_sizes(h.p(src.ptrs), h.p(src.sizes), h.p(sizes), len(chunks), backend.dev.stream()) == 0
    backend.dev.synchronize()
    assert h.get(sizes, len(chunks), np.uint64).tolist() == codec.get_decompress_size(dev_comp).tolist() == caps


def test_decodes_oracle_streams(backend, oracle, k):
    chunks = [datasets.text(70001, 2), datasets.lowcard(4099, 1), np.arange(2048, dtype=np.uint8), np.zeros(5, np.uint8)]
    comp = [oracle.ans_compress(c) for c in chunks]
    outs, actual, status, flags = dev_decompress(backend, k, comp, [c.size for c in chunks], comp_align=1)
    assert flags == 0 and (status == 0).all() and actual.tolist() == [c.size for c in chunks]
    assert all(np.array_equal(o, c) for o, c in zip(outs, chunks))


def test_oversized_chunk_returns_zero(backend, k):
    """n > nvcompANSCompressionMaxAllowedChunkSize: compress() returns 0 (the card runs the 16 MiB + 1 byte chunk)."""
    if backend.name == "emu":
        pytest.skip("a 16 MiB chunk takes minutes on the emulator; the card runs it")
    big = np.full(16 * MIB + 1, 3, np.uint8)
    comp, flags = dev_compress(backend, k, [big, np.full(1000, 4, np.uint8)])
    assert flags == 0 and comp[0].size == 0 and comp[1].size == 1012


def test_constants(backend, k):
    codec = backend.codec("ANS")
    for n in (0, 1, 7, 2048, 65536, 16 * MIB):
        assert k.ansdev_max_compressed_bytes(n) == codec.max_compressed_size(n)
    assert k.ansdev_shared_bytes(0) == 4096 and k.ansdev_shared_bytes(1) == 5120


@pytest.mark.parametrize("block", [64, 256, 1024])
@pytest.mark.parametrize("chunks_per_wave", [1, 3])
def test_launch_shapes(backend, oracle, k, block, chunks_per_wave):
    """Workgroups of 1, 4 and 16 waves; waves that loop over several chunks and reuse their LDS area."""
    rng = np.random.RandomState(block + chunks_per_wave)
    count = 20 if backend.name == "emu" else 600
    chunks = [datasets.CLASSES[sorted(datasets.CLASSES)[i % len(datasets.CLASSES)]](int(rng.randint(1, 9000)), i)
              .view(np.uint8)[: int(rng.randint(0, 9000))].copy() for i in range(count)]
    comp, flags = dev_compress(backend, k, chunks, block=block, chunks_per_wave=chunks_per_wave)
    assert flags == 0
    for c, cc in zip(chunks, comp):
        assert np.array_equal(cc, oracle.ans_compress(c))
    caps = [c.size for c in chunks]
    for mode in (0, 1):
        outs, actual, status, flags = dev_decompress(backend, k, comp, caps, mode=mode, block=block,
                                                     chunks_per_wave=chunks_per_wave)
        assert flags == 0 and (status == 0).all() and actual.tolist() == caps
        assert all(np.array_equal(o, c) for o, c in zip(outs, chunks))


@pytest.mark.parametrize("block", [256, 1024])
def test_mixed_workgroup(backend, oracle, k, block):
    """Half the waves of each workgroup decode while the others run unrelated code: no workgroup barrier in the calls."""
    h = Dev(backend)
    pairs_per_block = block // 128
    count = 6 if backend.name == "emu" else 512
    chunks = [datasets.text(3000 + 997 * i, i) for i in range(count)]
    comp = [oracle.ans_compress(c) for c in chunks]
    caps = [c.size for c in chunks]
    grid = -(-count // pairs_per_block)
    iters = 2000
    src = make_batch(backend.dev, comp)
    out = empty_batch(backend.dev, [c + 32 for c in caps], align=16, fill=0xA5)
    out.sizes = backend.dev.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    actual, flags = h.zeros(count, np.uint64), h.zeros(1, np.uint32)
    status = backend.dev.upload(np.full(count, -1, dtype=np.int32).view(np.uint8))
    side = h.zeros(grid * pairs_per_block * 64, np.uint32)
    assert k.ansdev_mixed(h.p(src.ptrs), h.p(src.sizes), h.p(out.ptrs), h.p(out.sizes), h.p(actual), h.p(status), count,
                          h.p(side), iters, block, grid, h.p(flags), backend.dev.stream()) == 0
    backend.dev.synchronize()
    assert int(h.get(flags, 1, np.uint32)[0]) == 0
    assert (h.get(status, count, np.int32) == 0).all() and h.get(actual, count, np.uint64).tolist() == caps
    host = backend.dev.download(out.slab)
    for o, c, cap in zip(out.offsets, chunks, caps):
        assert np.array_equal(host[int(o): int(o) + cap], c) and (host[int(o) + cap: int(o) + cap + 32] == 0xA5).all()
    x = np.arange(1, grid * pairs_per_block * 64 + 1, dtype=np.uint32)  # lane t of the unrelated waves starts at t + 1
    for _ in range(iters):
        x ^= x << np.uint32(13)
        x ^= x >> np.uint32(17)
        x ^= x << np.uint32(5)
    assert np.array_equal(h.get(side, x.size, np.uint32), x)


@pytest.mark.parametrize("misalign", [0, 3])
def test_in_and_out_in_lds(backend, k, misalign):
    """Chunks staged in LDS, compressed into LDS and decompressed from LDS into LDS."""
    h = Dev(backend)
    chunks = [datasets.text(6144, 1), np.zeros(0, np.uint8), np.full(3000, 9, np.uint8), datasets.float_csv(2049, 2),
              np.random.RandomState(1).randint(0, 256, 5000).astype(np.uint8), datasets.lowcard(777, 3)]
    chunks = [c.view(np.uint8)[:6144].copy() for c in chunks]
    n = len(chunks)
    codec = backend.codec("ANS")
    ref = codec.compress(chunks)
    src = make_batch(backend.dev, chunks)
    max_out = int(k.ansdev_max_compressed_bytes(6144))
    comp = empty_batch(backend.dev, [max_out] * n, stride=max_out)
    dec = empty_batch(backend.dev, [6144] * n, stride=6144)
    actual, status, flags = h.zeros(n, np.uint64), h.zeros(n, np.int32), h.zeros(1, np.uint32)
    assert k.ansdev_lds_roundtrip(h.p(src.ptrs), h.p(src.sizes), h.p(comp.ptrs), h.p(comp.sizes), h.p(dec.ptrs),
                                  h.p(actual), h.p(status), n, misalign, h.p(flags), backend.dev.stream()) == 0
    backend.dev.synchronize()
    assert int(h.get(flags, 1, np.uint32)[0]) == 0
    comp_out = read_batch(backend.dev, comp, h.get(comp.sizes, n, np.uint64))
    for c, cc, r in zip(chunks, comp_out, ref):
        assert np.array_equal(cc, r)
    assert (h.get(status, n, np.int32) == 0).all() and h.get(actual, n, np.uint64).tolist() == [c.size for c in chunks]
    for c, o in zip(chunks, read_batch(backend.dev, dec, [c.size for c in chunks])):
        assert np.array_equal(o, c)


def test_sink_contract(backend, oracle, k):
    """A counting sink sees every byte of [0, n) exactly once, at offsets % 4 == 0, stored chunks included."""
    sizes = [0, 1, 5, 255, 257, 513, 2047, 2049, 4099, 65613]
    rng = np.random.RandomState(4)
    chunks = [np.minimum(rng.geometric(0.3, size=n), 255).astype(np.uint8) for n in sizes]
    chunks += [rng.randint(0, 256, 4099).astype(np.uint8), rng.randint(0, 256, 3).astype(np.uint8)]  # stored
    comp = [oracle.ans_compress(c) for c in chunks]
    caps = [c.size for c in chunks]
    outs, actual, status, flags = dev_decompress(backend, k, comp, caps, mode=2)
    assert flags == 0 and (status == 0).all() and actual.tolist() == caps
    for c, o in zip(chunks, outs):
        assert (o.view(np.uint32) == 1).all(), "a byte was handed to the sink other than once"
    outs, actual, status, flags = dev_decompress(backend, k, comp, caps, mode=1)
    assert flags == 0 and (status == 0).all()
    assert all(np.array_equal(o, c) for o, c in zip(outs, chunks))


@pytest.mark.parametrize("elem_bytes", [2, 4])
def test_fused_codebook(backend, oracle, k, elem_bytes):
    """The fused consumer: decoded bytes looked up in a 256-entry fp16 / fp32 codebook, against numpy."""
    h = Dev(backend)
    rng = np.random.RandomState(elem_bytes)
    chunks = [np.minimum(rng.geometric(0.05, size=n), 255).astype(np.uint8) for n in (65536, 4099, 2048, 100, 0, 65613)]
    comp = [oracle.ans_compress(c) for c in chunks]
    dt = np.float16 if elem_bytes == 2 else np.float32
    book = (rng.standard_normal(256) * 3).astype(dt)
    n = len(chunks)
    src = make_batch(backend.dev, comp)
    caps = [c.size for c in chunks]
    out = empty_batch(backend.dev, [c * elem_bytes for c in caps], align=16)
    cb = backend.dev.upload(book.view(np.uint8))
    status = h.zeros(n, np.int32)
    capbuf = backend.dev.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    assert k.ansdev_codebook(h.p(src.ptrs), h.p(src.sizes), h.p(capbuf), h.p(out.ptrs), h.p(cb), elem_bytes, h.p(status), n,
                             backend.dev.stream()) == 0
    backend.dev.synchronize()
    assert (h.get(status, n, np.int32) == 0).all()
    for c, o in zip(chunks, read_batch(backend.dev, out)):
        assert np.array_equal(o.view(dt), book[c])


def corruptions(stream, rng):
    """(label, bad stream) pairs: truncations, a wrong magic, flipped bits in the frequency table, states and words."""
    out = [("empty", stream[:0]), ("header only", stream[:12]), ("half", stream[: stream.size // 2]),
           ("one short", stream[:-1])]
    b = stream.copy()
    b[0] ^= 0x20
    out.append(("magic", b))
    b = stream.copy()
    b[8] = 2
    out.append(("mode", b))
    for label, lo, hi in (("freq", 16, 528), ("state", 528, 1040), ("words", 1040, stream.size)):
        for _ in range(3):
            b = stream.copy()
            b[rng.randint(lo, hi)] ^= 1 << rng.randint(0, 8)
            out.append((label, b))
    return out


def test_errors_match_batched(backend, oracle, k):
    """Every corruption gives nvcompErrorCannotDecompress exactly where the batched decoder does, and so does a capacity
    one byte too small; guard bytes behind each output and around each wave's LDS area survive."""
    rng = np.random.RandomState(8)
    srcs = [datasets.text(20000, 5), datasets.lowcard(65536, 2)]
    cases, caps = [], []
    for s in srcs:
        stream = oracle.ans_compress(s)
        assert stream[8] == 1  # coded, so that every region exists
        for label, b in corruptions(stream, rng):
            cases.append(b)
            caps.append(s.size)
        cases.append(stream)
        caps.append(s.size - 1)
    stored = rng.randint(0, 256, 3000).astype(np.uint8)
    st_stream = oracle.ans_compress(stored)
    cases += [st_stream[:-1], st_stream]
    caps += [3000, 2999]
    codec = backend.codec("ANS")
    _, b_actual, b_status = codec.decompress(cases, caps)
    for mode in (0, 1):
        outs, actual, status, flags = dev_decompress(backend, k, cases, caps, mode=mode)
        assert flags == 0  # the guards around the LDS areas, and the sink only ever inside the capacity
        assert status.tolist() == b_status.tolist()
        assert actual.tolist() == b_actual.tolist()
        assert (status[-2:] == NvcompStatus.ErrorCannotDecompress).all()
        assert all(status[i] == NvcompStatus.ErrorCannotDecompress for i in range(len(cases)) if caps[i] == srcs[0].size - 1)


def test_header_is_self_contained(tmp_path):
    """Every entry point, in a kernel that sees nothing but `-I include`, cross-compiles for gfx950 and uses no scratch."""
    if shutil.which(HIPCC) is None and not os.path.exists(HIPCC):
        pytest.skip("hipcc is not installed")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(REPO, "include"),
                        "--cuda-device-only", "-c", SRC, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    scratch = [l for l in r.stderr.splitlines() if "ScratchSize" in l]
    assert len(scratch) >= 7 and all(l.split("ScratchSize [bytes/lane]:")[1].split()[0] == "0" for l in scratch), scratch


@pytest.mark.gpu
def test_example_on_gpu():
    r = subprocess.run(["make", "-C", "examples", os.path.join(REPO, "examples", "bin", "ans_device_example")], cwd=REPO,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(REPO, "examples", "bin", "ans_device_example")], cwd=REPO, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fused decode matches" in r.stdout
