"""The high-level managers (nvcomp_amd/csrc/hlif/manager.hip: LZ4Manager ... DeflateManager, create_manager) against an
independent model of their container (tests/hlif_container.py) and CPU codecs, on the host emulation and on the MI355X
(`backend`). tests/hlif/hlif_driver.cpp gives ctypes a way to the C++ classes. Bit-exact throughout: every comparison is
equality of bytes, sizes or status codes."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import hlif_container as hc
from nvcomp_amd import datasets
from nvcomp_amd._lib import OPTS, NvcompStatus

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "hlif", "hlif_driver.cpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

OK, INVALID_ARGUMENT, RUNTIME_ERROR = 0, 1, 2  # the driver's return codes
SUCCESS, INVALID_VALUE = int(NvcompStatus.Success), int(NvcompStatus.ErrorInvalidValue)
CANNOT, BAD_CRC = int(NvcompStatus.ErrorCannotDecompress), int(NvcompStatus.ErrorBadChecksum)
NO_NO, COMPUTE_NO, NO_IFPRESENT, COMPUTE_IFPRESENT, COMPUTE_VERIFY = range(5)  # nvcomp::ChecksumPolicy
POLICIES = [NO_NO, COMPUTE_NO, NO_IFPRESENT, COMPUTE_IFPRESENT, COMPUTE_VERIFY]
COMPUTES = {COMPUTE_NO, COMPUTE_IFPRESENT, COMPUTE_VERIFY}
VERIFIES = {NO_IFPRESENT, COMPUTE_IFPRESENT, COMPUTE_VERIFY}

FORMATS = ["LZ4", "Snappy", "Deflate", "Cascaded", "Bitcomp", "ANS"]
DEFAULT_OPTS = {"LZ4": (0,), "Snappy": (0,), "Deflate": (0,), "Cascaded": (4096, 4, 2, 1, 1), "Bitcomp": (0, 1), "ANS": (0,)}
# other valid options of the same format (Snappy and ANS have only one valid value)
OTHER_OPTS = {"LZ4": (2,), "Snappy": (0,), "Deflate": (1,), "Cascaded": (1024, 1, 0, 0, 0), "Bitcomp": (1, 5), "ANS": (0,)}
BAD_OPTS = {"LZ4": (8,), "Snappy": (1,), "Deflate": (3,), "Cascaded": (100, 4, 2, 1, 1), "Bitcomp": (2, 1), "ANS": (1,)}
GUARD = 64
# The LZ match finders let several lanes write one hash-table slot in one instruction. The card orders them the same way
# every time; the emulator's scheduler orders lanes pseudo-randomly ON PURPOSE (tests/emu/hip/hip_runtime.h), so there two
# calls of these compressors choose other matches ("the emulator's streams differ in a few offsets"). Their
# streams are compared byte for byte with the batched API's on the card; on the emulator after reseed() only.
RACY_ON_EMULATOR = {"LZ4", "Snappy", "Deflate"}


def reseed(backend, seed=1):
    """Emulator: restart the lane scheduler's pseudo-random order, so that the same sequence of launches behind two
    reseed() calls orders its lanes alike. The card needs nothing."""
    if backend.name == "emu":
        fn = getattr(backend.lib, "_ZN3emu8set_seedEm")  # emu::set_seed(uint64_t), tests/emu/emu.cpp
        fn.argtypes, fn.restype = [C.c_uint64], None
        fn(seed)

_libs = {}


def driver(backend, tmp_path_factory):
    """tests/hlif/hlif_driver.cpp built for the backend's tier (once per session)."""
    if backend.name not in _libs:
        d = tmp_path_factory.mktemp(f"hlif_{backend.name}")
        so = str(d / "hlif_driver.so")
        if backend.name == "emu":
            import conftest

            conftest.emu_library()
            cmd = ["g++", "-O1", "-std=c++17", "-x", "c++", "-shared", "-fPIC", "-Itests/emu", "-Iinclude", SRC, "-o", so,
                   "-Ltests/emu", "-lnvcomp_emu", f"-Wl,-rpath,{REPO}/tests/emu"]
        else:
            cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Iinclude", SRC, "-o", so,
                   "-Lnvcomp_amd/lib", "-lnvcomp", f"-Wl,-rpath,{REPO}/nvcomp_amd/lib"]
        r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        lib = C.CDLL(so)
        vp, sz, i, szp, vpp = C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p)
        lib.hlif_last_error.restype = C.c_char_p
        lib.hlif_open.argtypes = [i, sz, vp, sz, i, vp, i, vpp]
        lib.hlif_open_from_buffer.argtypes = [vp, i, vp, vpp]
        lib.hlif_close.argtypes = [vp]
        lib.hlif_configure_compression.argtypes = [vp, sz, vpp, szp, szp]
        lib.hlif_compress.argtypes = [vp, vp, vp, vp]
        lib.hlif_configure_decompression.argtypes = [vp, vp, vpp, szp, szp, szp]
        lib.hlif_configure_decompression_from_config.argtypes = [vp, vp, vpp, szp, szp, szp]
        lib.hlif_decompress.argtypes = [vp, vp, vp, vp]
        lib.hlif_compression_status.argtypes = [vp, C.POINTER(i)]
        lib.hlif_decompression_status.argtypes = [vp, C.POINTER(i)]
        lib.hlif_compression_status_address.argtypes = [vp]
        lib.hlif_compression_status_address.restype = vp
        lib.hlif_decompression_status_address.argtypes = [vp]
        lib.hlif_decompression_status_address.restype = vp
        lib.hlif_compressed_output_size.argtypes = [vp, vp, szp]
        lib.hlif_close_compression_config.argtypes = [vp]
        lib.hlif_close_decompression_config.argtypes = [vp]
        _libs[backend.name] = lib
    return _libs[backend.name]


class HlifError(Exception):
    def __init__(self, code, text):
        super().__init__(f"{code}: {text}")
        self.code = code


class Config:
    def __init__(self, lib, handle, compression, **fields):
        self.lib, self.handle, self.compression = lib, handle, compression
        self.__dict__.update(fields)

    def status(self):
        out = C.c_int(-1)
        fn = self.lib.hlif_compression_status if self.compression else self.lib.hlif_decompression_status
        assert fn(self.handle, C.byref(out)) == OK
        return out.value

    def status_address(self):
        fn = self.lib.hlif_compression_status_address if self.compression else self.lib.hlif_decompression_status_address
        return fn(self.handle)

    def close(self):
        fn = self.lib.hlif_close_compression_config if self.compression else self.lib.hlif_close_decompression_config
        assert fn(self.handle) == OK
        self.handle = None


class Manager:
    """One nvcomp manager behind the driver. Errors of the library come back as HlifError(code)."""

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle

    def _check(self, rc):
        if rc != OK:
            raise HlifError(rc, self.lib.hlif_last_error().decode())

    @classmethod
    def open(cls, lib, fmt, chunk, opts=None, policy=NO_NO, stream=None, defaults=False):
        raw = bytes(OPTS[fmt](*(DEFAULT_OPTS[fmt] if opts is None else opts)))
        out = C.c_void_p()
        rc = lib.hlif_open(hc.FORMAT_IDS[fmt], chunk, raw, len(raw), policy, stream, int(defaults), C.byref(out))
        if rc != OK:
            raise HlifError(rc, lib.hlif_last_error().decode())
        return cls(lib, out)

    @classmethod
    def from_buffer(cls, lib, comp_ptr, policy=NO_NO, stream=None):
        out = C.c_void_p()
        rc = lib.hlif_open_from_buffer(comp_ptr, policy, stream, C.byref(out))
        if rc != OK:
            raise HlifError(rc, lib.hlif_last_error().decode())
        return cls(lib, out)

    def configure_compression(self, nbytes):
        h, a, b = C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._check(self.lib.hlif_configure_compression(self.handle, nbytes, C.byref(h), C.byref(a), C.byref(b)))
        return Config(self.lib, h, True, max_compressed_buffer_size=a.value, num_chunks=b.value)

    def compress(self, src_ptr, dst_ptr, cfg):
        self._check(self.lib.hlif_compress(self.handle, src_ptr, dst_ptr, cfg.handle))

    def configure_decompression(self, comp_ptr):
        h, a, b, c = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self.lib.hlif_configure_decompression(self.handle, comp_ptr, C.byref(h), C.byref(a), C.byref(b), C.byref(c)))
        return Config(self.lib, h, False, decomp_data_size=a.value, num_chunks=b.value, chunk_size=c.value)

    def configure_decompression_from(self, comp_cfg):
        h, a, b, c = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self.lib.hlif_configure_decompression_from_config(self.handle, comp_cfg.handle, C.byref(h), C.byref(a),
                                                                      C.byref(b), C.byref(c)))
        return Config(self.lib, h, False, decomp_data_size=a.value, num_chunks=b.value, chunk_size=c.value)

    def decompress(self, dst_ptr, comp_ptr, cfg):
        self._check(self.lib.hlif_decompress(self.handle, dst_ptr, comp_ptr, cfg.handle))

    def compressed_output_size(self, comp_ptr):
        out = C.c_size_t()
        self._check(self.lib.hlif_compressed_output_size(self.handle, comp_ptr, C.byref(out)))
        return out.value

    def close(self):
        self._check(self.lib.hlif_close(self.handle))
        self.handle = None


class Buf:
    """`nbytes` device bytes at `offset` past a 256-byte boundary, GUARD bytes of `fill` on both sides (the test owns
    alignment and guard bytes)."""

    def __init__(self, backend, nbytes, offset=0, fill=0xA5, data=None):
        self.dev, self.nbytes, self.fill = backend.dev, int(nbytes), fill
        room = self.nbytes + 2 * GUARD + 512 + offset
        self.raw = self.dev.empty(room)
        lead = (-self.dev.ptr(self.raw)) % 256
        if lead < GUARD:
            lead += 256
        self.at = lead + offset
        self.ptr = self.dev.ptr(self.raw) + self.at
        image = np.full(room, fill, dtype=np.uint8)
        if data is not None:
            data = np.asarray(data).view(np.uint8).reshape(-1)
            image[self.at: self.at + data.size] = data
        self._put(0, image)

    def _put(self, at, host):
        if hasattr(self.dev, "torch"):
            self.raw[at: at + host.size].copy_(self.dev.torch.from_numpy(np.ascontiguousarray(host)))
        else:
            self.raw[at: at + host.size] = host

    def write(self, host, at=0):
        self._put(self.at + at, np.asarray(host).view(np.uint8).reshape(-1))

    def read(self, nbytes=None):
        n = self.nbytes if nbytes is None else int(nbytes)
        return self.dev.download(self.raw)[self.at: self.at + n].copy()

    def guards_intact(self, used=None):
        """Nothing in front of the buffer and nothing behind its first `used` bytes has changed."""
        used = self.nbytes if used is None else int(used)
        host = self.dev.download(self.raw)
        return bool((host[: self.at] == self.fill).all() and (host[self.at + used:] == self.fill).all())


@pytest.fixture
def drv(backend, tmp_path_factory):
    return driver(backend, tmp_path_factory)


def elem_width(fmt, opts):
    if fmt == "Cascaded":
        return 1 << (opts[1] >> 1)
    return 1


def compress(backend, drv, fmt, data, chunk, opts=None, policy=NO_NO, comp_offset=0, in_offset=0, fill=0xA5, mgr=None,
             seed=None):
    """One manager compress(): returns (container bytes, parsed container, max_compressed_buffer_size). Checks the status,
    the size bound, the guard bytes and the container's structure."""
    opts = DEFAULT_OPTS[fmt] if opts is None else opts
    own = mgr is None
    m = Manager.open(drv, fmt, chunk, opts, policy, backend.dev.stream()) if own else mgr
    data = np.asarray(data).view(np.uint8).reshape(-1)
    cfg = m.configure_compression(data.size)
    assert cfg.num_chunks == -(-data.size // chunk)
    src = Buf(backend, data.size, offset=in_offset, data=data)
    dst = Buf(backend, cfg.max_compressed_buffer_size, offset=comp_offset, fill=fill)
    if seed is not None:
        reseed(backend, seed)
    m.compress(src.ptr, dst.ptr, cfg)
    total = m.compressed_output_size(dst.ptr)  # synchronises
    backend.dev.synchronize()
    assert cfg.status() == SUCCESS
    assert total <= cfg.max_compressed_buffer_size
    assert dst.guards_intact(), "compress() wrote outside max_compressed_buffer_size"
    assert np.array_equal(src.read(), data) and src.guards_intact()
    container = dst.read(total)
    parsed = hc.parse(container, fmt, OPTS[fmt](*opts), policy in COMPUTES)
    assert parsed.uncompressed_size == data.size and parsed.chunk_size == chunk and parsed.compressed_size == total
    max_size = cfg.max_compressed_buffer_size
    cfg.close()
    if own:
        m.close()
    return container, parsed, max_size


def decompress(backend, drv, container, policy=NO_NO, mgr=None, comp_offset=0, out_offset=0, expect_bytes=None):
    """One manager decompress() of a container: returns (status, output bytes). The manager comes from create_manager
    unless one is given. The guard bytes around the output must survive, whatever the status."""
    container = np.asarray(container).view(np.uint8)
    comp = Buf(backend, container.size, offset=comp_offset, data=container)
    own = mgr is None
    m = Manager.from_buffer(drv, comp.ptr, policy, backend.dev.stream()) if own else mgr
    try:
        cfg = m.configure_decompression(comp.ptr)
        if expect_bytes is not None:
            assert cfg.decomp_data_size == expect_bytes
        out = Buf(backend, cfg.decomp_data_size, offset=out_offset, fill=0x3C)
        m.decompress(out.ptr, comp.ptr, cfg)
        backend.dev.synchronize()
        status = cfg.status()
        assert out.guards_intact(), "decompress() wrote outside decomp_data_size"
        assert np.array_equal(comp.read(), container), "decompress() changed the container"
        result = out.read()
        cfg.close()
    finally:
        if own:
            m.close()
    return status, result


def cpu_decode(oracle, fmt, payload, cap):
    """(decoded without error, bytes) by a decoder that is not this library's kernels."""
    payload = np.ascontiguousarray(payload)
    if fmt == "Deflate":
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress(payload.tobytes(), cap + 1)
        except zlib.error:
            return False, np.zeros(0, np.uint8)
        return d.eof and not d.unused_data, np.frombuffer(out, dtype=np.uint8)
    if fmt == "LZ4":
        fn = oracle.ref_lz4_decompress if oracle.have_ref() else oracle.lz4_decompress
    elif fmt == "Snappy":
        fn = oracle.ref_snappy_decompress if oracle.have_ref() else oracle.snappy_decompress
    else:
        fn = {"Cascaded": oracle.cascaded_decompress, "Bitcomp": oracle.bitcomp_decompress, "ANS": oracle.ans_decompress}[fmt]
    rc, out = fn(payload, cap)
    return rc == 0, out


def chunks_of(data, chunk):
    return [data[i: i + chunk] for i in range(0, data.size, chunk)]


def check_against_cpu(backend, oracle, fmt, opts, data, chunk, parsed, sums):
    """(a): the payloads are the batched API's, decode on the CPU to the input, and carry zlib's checksums."""
    pieces = chunks_of(data, chunk)
    assert len(pieces) == parsed.num_chunks
    if pieces and (backend.name == "gpu" or fmt not in RACY_ON_EMULATOR):
        direct = backend.codec(fmt, opts).compress(pieces, max_chunk=chunk)
        for i, (p, d) in enumerate(zip(parsed.payloads, direct)):
            assert int(parsed.comp_size[i]) == d.size and np.array_equal(p, d), f"chunk {i}: not the batched API's bytes"
    for i, (p, raw) in enumerate(zip(parsed.payloads, pieces)):
        ok, back = cpu_decode(oracle, fmt, p, raw.size)
        assert ok and np.array_equal(back, raw), f"chunk {i}: the CPU decoder does not give the input back"
        if sums:
            assert int(parsed.crc_uncomp[i]) == zlib.crc32(raw.tobytes()), f"crc_uncomp[{i}]"
            assert int(parsed.crc_comp[i]) == zlib.crc32(p.tobytes()), f"crc_comp[{i}]"


def sample(name, nbytes, seed=1):
    return np.ascontiguousarray(datasets.CLASSES[name](max(nbytes, 64), seed)).view(np.uint8).reshape(-1)[:nbytes].copy()


def mixed(nbytes, seed=0):
    """Text, numbers, runs and noise in turn: every chunk of a test compresses to another size."""
    if nbytes > 1 << 18:  # large buffers repeat a 256 KiB block: the generators are Python loops
        return np.resize(mixed(1 << 18, seed), nbytes)
    rng = np.random.RandomState(seed)
    parts, have = [np.zeros(0, np.uint8)], 0
    names = ["text", "int32", "noise", "zeros", "table", "lowcard", "float32"]
    while have < nbytes:
        n = int(rng.randint(40, 1500)) * 4
        parts.append(sample(names[len(parts) % len(names)], n, seed + len(parts)))
        have += n
    return np.concatenate(parts)[:nbytes].copy()


# ---------------------------------------------------------------------------------------------- (a) writer against the CPU

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", sorted(datasets.CLASSES))
def test_writer_against_cpu(backend, oracle, drv, fmt, name):
    chunk, nbytes = 4096, 5 * 4096 + 1028  # a ragged last chunk, a whole number of 4-byte elements for Cascaded
    data = sample(name, nbytes)
    opts = DEFAULT_OPTS[fmt]
    policy = COMPUTE_NO if sorted(datasets.CLASSES).index(name) % 2 else NO_NO
    container, parsed, _ = compress(backend, drv, fmt, data, chunk, opts, policy)
    check_against_cpu(backend, oracle, fmt, opts, data, chunk, parsed, policy in COMPUTES)
    status, out = decompress(backend, drv, container, NO_IFPRESENT, expect_bytes=nbytes)
    assert status == SUCCESS and np.array_equal(out, data)


@pytest.mark.parametrize("fmt", FORMATS)
def test_default_constructor_arguments(backend, drv, fmt):
    """M(chunk) alone: default options, stream 0, device 0, no checksums."""
    m = Manager.open(drv, fmt, 8192, defaults=True)
    data = mixed(20000, 3)
    container, parsed, _ = compress(backend, drv, fmt, data, 8192, mgr=m)
    assert parsed.flags == 0
    status, out = decompress(backend, drv, container, mgr=m)
    assert status == SUCCESS and np.array_equal(out, data)
    m.close()


# ------------------------------------------------------------------------------------- (b) reader against a foreign writer

def foreign_writers(oracle):
    """name -> (format, compress one chunk on the CPU). The liblz4 / libsnappy / libdeflate ones need the _ref shim."""
    w = {
        "zlib_raw_deflate": ("Deflate", lambda c: np.frombuffer(
            (lambda o: o.compress(c.tobytes()) + o.flush())(zlib.compressobj(6, zlib.DEFLATED, -15)), dtype=np.uint8)),
        "oracle_lz4": ("LZ4", oracle.lz4_compress),
        "oracle_snappy": ("Snappy", oracle.snappy_compress),
        "oracle_cascaded": ("Cascaded", oracle.cascaded_compress),
        "oracle_bitcomp": ("Bitcomp", oracle.bitcomp_compress),
        "oracle_ans": ("ANS", oracle.ans_compress),
    }
    if oracle.have_ref():
        w["liblz4"] = ("LZ4", oracle.ref_lz4_compress)
        w["liblz4_hc"] = ("LZ4", lambda c: oracle.ref_lz4_compress(c, hc_level=9))
        w["libsnappy"] = ("Snappy", oracle.ref_snappy_compress)
    return w


WRITERS = ["zlib_raw_deflate", "oracle_lz4", "oracle_snappy", "oracle_cascaded", "oracle_bitcomp", "oracle_ans", "liblz4",
           "liblz4_hc", "libsnappy"]


@pytest.mark.parametrize("writer", WRITERS)
@pytest.mark.parametrize("sums", [False, True])
def test_reader_against_foreign_writer(backend, oracle, drv, writer, sums):
    """Containers written by hlif_container.build around CPU-compressed chunks decode through create_manager and through
    a typed manager opened with ANOTHER chunk size and OTHER options: the header's options need not match the reader's."""
    writers = foreign_writers(oracle)
    if writer not in writers:
        pytest.skip("needs liblz4 / libsnappy (oracle.have_ref())")
    fmt, enc = writers[writer]
    chunk = 4096
    data = mixed(6 * chunk + 520, 5)
    pieces = chunks_of(data, chunk)
    comp = [np.asarray(enc(p)).view(np.uint8) for p in pieces]
    crcs = ([zlib.crc32(p.tobytes()) for p in pieces], [zlib.crc32(c.tobytes()) for c in comp]) if sums else None
    container = hc.build(fmt, chunk, OPTS[fmt](*DEFAULT_OPTS[fmt]), comp, data.size, crcs)
    hc.parse(container, fmt, OPTS[fmt](*DEFAULT_OPTS[fmt]), sums)
    policy = COMPUTE_VERIFY if sums else NO_IFPRESENT
    # (include/nvcomp/cascaded.h: uncompressed chunks are aligned to the element type)
    status, out = decompress(backend, drv, container, policy, expect_bytes=data.size, comp_offset=8,
                             out_offset=4 if fmt == "Cascaded" else 3)
    assert status == SUCCESS and np.array_equal(out, data)
    typed = Manager.open(drv, fmt, 1024, OTHER_OPTS[fmt], policy, backend.dev.stream())
    status, out = decompress(backend, drv, container, mgr=typed, expect_bytes=data.size)
    assert status == SUCCESS and np.array_equal(out, data)
    typed.close()


# --------------------------------------------------------------------------------------------------------------- (c) shapes

def roundtrip(backend, oracle, drv, fmt, data, chunk, opts=None, policy=COMPUTE_VERIFY, cpu=True, **where):
    opts = DEFAULT_OPTS[fmt] if opts is None else opts
    container, parsed, _ = compress(backend, drv, fmt, data, chunk, opts, policy, **where)
    if cpu:
        check_against_cpu(backend, oracle, fmt, opts, data, chunk, parsed, policy in COMPUTES)
    status, out = decompress(backend, drv, container, policy if policy != COMPUTE_VERIFY or parsed.flags else NO_NO,
                             expect_bytes=data.size, comp_offset=where.get("comp_offset", 0))
    assert status == SUCCESS and np.array_equal(out, data)
    return parsed


@pytest.mark.parametrize("fmt", FORMATS)
def test_buffer_sizes_around_a_chunk(backend, oracle, drv, fmt):
    chunk = 512
    for nbytes in (0, 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 1):
        if nbytes % elem_width(fmt, DEFAULT_OPTS[fmt]):
            opts = (4096, 1, 2, 1, 1)  # Cascaded on bytes: any size
        else:
            opts = DEFAULT_OPTS[fmt]
        parsed = roundtrip(backend, oracle, drv, fmt, mixed(nbytes, nbytes), chunk, opts)
        assert parsed.num_chunks == -(-nbytes // chunk)
        if nbytes == 0:
            assert parsed.compressed_size == 64 + 8 and hc.table_bytes(0) == 8


def test_empty_buffer_without_checksums(backend, oracle, drv):
    container, parsed, _ = compress(backend, drv, "LZ4", np.zeros(0, np.uint8), 65536, policy=NO_NO)
    assert container.size == 72 and parsed.num_chunks == 0
    status, out = decompress(backend, drv, container, NO_NO)
    assert status == SUCCESS and out.size == 0


@pytest.mark.parametrize("fmt", ["LZ4", "ANS"])
@pytest.mark.parametrize("chunk", [1, 512, 4096, 65536, 1 << 24])
def test_chunk_sizes(backend, oracle, drv, fmt, chunk):
    if chunk == 1 << 24 and backend.name == "emu":
        pytest.skip("a 16 MiB chunk takes minutes on the emulator; the card runs it")
    nbytes = {1: 37, 512: 512 * 3 + 5, 4096: 4096 * 2 + 77, 65536: 65536 + 4100, 1 << 24: 1 << 24}[chunk]
    data = mixed(nbytes, chunk % 1000)
    parsed = roundtrip(backend, oracle, drv, fmt, data, chunk, cpu=chunk < (1 << 24))
    assert parsed.num_chunks == -(-nbytes // chunk)


@pytest.mark.parametrize("fmt", FORMATS)
def test_chunk_size_limits(backend, drv, fmt):
    for bad in (0, (1 << 24) + 1):
        with pytest.raises(HlifError) as e:
            Manager.open(drv, fmt, bad)
        assert e.value.code == INVALID_ARGUMENT
    if fmt != "Deflate":  # nvcompDeflateCompressionMaxAllowedChunkSize is 64 KiB
        Manager.open(drv, fmt, 1 << 24).close()
    else:
        Manager.open(drv, fmt, 1 << 16).close()
        with pytest.raises(HlifError):
            Manager.open(drv, fmt, (1 << 16) + 1)


EMU_COUNTS = [1, 2, 255, 256, 257, 511, 512, 513, 1000]
GPU_COUNTS = [4095, 4096, 4097, 8193, 70000]
UNEVEN_COUNTS = [257, 511, 513, 1000]  # layout_kernel: per >= 2 and threads that own fewer chunks than `per`, or none


def count_case(backend, oracle, drv, fmt, count, chunk=64):
    nbytes = (count - 1) * chunk + 4  # a ragged last chunk
    opts = DEFAULT_OPTS[fmt]
    data = mixed(nbytes, count)
    # the CPU decode of every payload is Python-loop bound: sample it for the large counts, the structure, the batched
    # API's bytes and the round trip are checked for every chunk
    container, parsed, _ = compress(backend, drv, fmt, data, chunk, opts, COMPUTE_NO)
    assert parsed.num_chunks == count
    pieces = chunks_of(data, chunk)
    if backend.name == "gpu" or fmt not in RACY_ON_EMULATOR:
        direct = backend.codec(fmt, opts).compress(pieces, max_chunk=chunk)
        assert [int(s) for s in parsed.comp_size] == [d.size for d in direct]
        assert all(np.array_equal(p, d) for p, d in zip(parsed.payloads, direct))
    assert len(set(int(s) for s in parsed.comp_size)) > 1 or count < 3, "the chunks should not all have one size"
    step = max(1, count // 300)
    for i in list(range(0, count, step)) + [count - 1]:
        ok, back = cpu_decode(oracle, fmt, parsed.payloads[i], pieces[i].size)
        assert ok and np.array_equal(back, pieces[i])
        assert int(parsed.crc_uncomp[i]) == zlib.crc32(pieces[i].tobytes())
        assert int(parsed.crc_comp[i]) == zlib.crc32(parsed.payloads[i].tobytes())
    status, out = decompress(backend, drv, container, COMPUTE_VERIFY, expect_bytes=nbytes)
    assert status == SUCCESS and np.array_equal(out, data)


@pytest.mark.parametrize("fmt", ["LZ4", "Bitcomp"])
@pytest.mark.parametrize("count", EMU_COUNTS + GPU_COUNTS)
def test_chunk_counts(backend, oracle, drv, fmt, count):
    if count in GPU_COUNTS and backend.name == "emu":
        pytest.skip("thousands of chunks are the card's share; the emulator runs the counts up to 1 000")
    count_case(backend, oracle, drv, fmt, count)


@pytest.mark.parametrize("fmt", ["Snappy", "Deflate", "Cascaded", "ANS"])
@pytest.mark.parametrize("count", UNEVEN_COUNTS)
def test_uneven_layout_split_every_format(backend, oracle, drv, fmt, count):
    count_case(backend, oracle, drv, fmt, count)


GATHER_SIZES = [4088, 4095, 4096, 4097, 8191, 8192, 12289] + [4096 + t for t in range(1, 8)] + [40 + t for t in range(1, 8)]


@pytest.mark.parametrize("comp_offset", [0, 8, 24])
def test_compressed_sizes_around_the_gather_loop(backend, oracle, drv, comp_offset):
    """gather_kernel's 4 KiB vector loop and its 8-byte tail: compressed chunks of exactly k bytes. ANS stores a chunk of
    noise as 12 bytes of header + the bytes, so a chunk size of k - 12 gives k: checked by parse, not assumed. The
    container starts 0, 8 and 24 bytes past a 256-byte boundary, so the 16-byte accesses meet 8-byte aligned addresses."""
    for k in sorted(set(GATHER_SIZES)):
        chunk = k - 12
        data = sample("noise", 2 * chunk + 9, k)
        # dirty the staging buffer first, with a larger batch of ones
        m = Manager.open(drv, "ANS", chunk, policy=COMPUTE_NO, stream=backend.dev.stream())
        compress(backend, drv, "ANS", np.full(4 * chunk, 0xFF, np.uint8), chunk, policy=COMPUTE_NO, mgr=m)
        container, parsed, _ = compress(backend, drv, "ANS", data, chunk, policy=COMPUTE_NO, comp_offset=comp_offset,
                                        in_offset=1, mgr=m)
        m.close()
        assert [int(s) for s in parsed.comp_size] == [k, k, 9 + 12], k
        check_against_cpu(backend, oracle, "ANS", DEFAULT_OPTS["ANS"], data, chunk, parsed, True)
        status, out = decompress(backend, drv, container, COMPUTE_VERIFY, comp_offset=comp_offset, out_offset=5)
        assert status == SUCCESS and np.array_equal(out, data)


@pytest.mark.parametrize("fmt", FORMATS)
def test_odd_buffer_offsets(backend, oracle, drv, fmt):
    opts = (4096, 1, 2, 1, 1) if fmt == "Cascaded" else DEFAULT_OPTS[fmt]
    data = mixed(3 * 2048 + 333, 17)
    for in_offset, comp_offset in ((1, 8), (7, 24), (13, 0)):
        container, parsed, _ = compress(backend, drv, fmt, data, 2048, opts, COMPUTE_NO, comp_offset=comp_offset,
                                        in_offset=in_offset)
        check_against_cpu(backend, oracle, fmt, opts, data, 2048, parsed, True)
        status, out = decompress(backend, drv, container, COMPUTE_VERIFY, comp_offset=comp_offset, out_offset=in_offset + 2)
        assert status == SUCCESS and np.array_equal(out, data)


# ------------------------------------------------------------------------------- (d) the container is a function of its input

@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("policy", [NO_NO, COMPUTE_NO])
def test_container_is_a_function_of_its_input(backend, drv, fmt, policy):
    chunk = 2048
    data = mixed(5 * chunk + 300, 23)
    dirty = Manager.open(drv, fmt, chunk, policy=policy, stream=backend.dev.stream())
    compress(backend, drv, fmt, np.bitwise_not(mixed(9 * chunk, 29)), chunk, policy=policy, mgr=dirty)  # larger, other data
    first, parsed, _ = compress(backend, drv, fmt, data, chunk, policy=policy, fill=0xA5, mgr=dirty, seed=5)
    dirty.close()
    second, _, _ = compress(backend, drv, fmt, data, chunk, policy=policy, fill=0x5A, seed=5)
    assert any(int(s) % 8 for s in parsed.comp_size), "no chunk has padding: the test would not see it"
    assert all(not p.any() for p in parsed.padding)
    if policy == NO_NO:
        assert not parsed.crc_uncomp.any() and not parsed.crc_comp.any()
    assert first.size == second.size and np.array_equal(first, second)


# ------------------------------------------------------------------------------------------------------------- (e) policies

def policy_case(backend, drv, fmt, writer, reader):
    chunk = 1024
    data = mixed(4 * chunk + 100, 31)
    container, parsed, _ = compress(backend, drv, fmt, data, chunk, policy=writer)
    assert bool(parsed.flags & hc.FLAG_CHECKSUMS) == (writer in COMPUTES)
    if reader == COMPUTE_VERIFY and writer not in COMPUTES:
        # ComputeAndVerify demands checksums: configure_decompression(buffer) throws
        with pytest.raises(HlifError) as e:
            decompress(backend, drv, container, reader)
        assert e.value.code == RUNTIME_ERROR and "checksum" in str(e.value)
        return
    status, out = decompress(backend, drv, container, reader)
    assert status == SUCCESS and np.array_equal(out, data)
    # the same through a typed manager
    m = Manager.open(drv, fmt, chunk, policy=reader, stream=backend.dev.stream())
    status, out = decompress(backend, drv, container, mgr=m)
    assert status == SUCCESS and np.array_equal(out, data)
    m.close()


@pytest.mark.parametrize("writer", POLICIES)
@pytest.mark.parametrize("reader", POLICIES)
def test_policy_matrix_lz4(backend, drv, writer, reader):
    policy_case(backend, drv, "LZ4", writer, reader)


@pytest.mark.parametrize("fmt", [f for f in FORMATS if f != "LZ4"])
@pytest.mark.parametrize("policy", POLICIES)
def test_policy_diagonal(backend, drv, fmt, policy):
    policy_case(backend, drv, fmt, policy, policy)


def test_compute_and_verify_through_the_compression_config(backend, drv):
    """configure_decompression(CompressionConfig) never reads the header (it must not synchronise), so it cannot refuse
    a buffer without checksums the way configure_decompression(buffer) does. Pinned behaviour (nvcompManager.hpp says
    so): decompress() then verifies nothing and reports nvcompSuccess, it does not fail."""
    chunk = 1024
    data = mixed(3 * chunk, 37)
    writer = Manager.open(drv, "LZ4", chunk, policy=NO_NO, stream=backend.dev.stream())
    ccfg = writer.configure_compression(data.size)
    src = Buf(backend, data.size, data=data)
    comp = Buf(backend, ccfg.max_compressed_buffer_size)
    writer.compress(src.ptr, comp.ptr, ccfg)
    reader = Manager.open(drv, "LZ4", chunk, policy=COMPUTE_VERIFY, stream=backend.dev.stream())
    dcfg = reader.configure_decompression_from(ccfg)
    assert (dcfg.decomp_data_size, dcfg.num_chunks, dcfg.chunk_size) == (data.size, 3, chunk)
    out = Buf(backend, data.size, fill=0x3C)
    reader.decompress(out.ptr, comp.ptr, dcfg)
    backend.dev.synchronize()
    assert dcfg.status() == SUCCESS and np.array_equal(out.read(), data) and out.guards_intact()
    with pytest.raises(HlifError):
        reader.configure_decompression(comp.ptr)
    # with checksums present the same overload does verify
    writer2 = Manager.open(drv, "LZ4", chunk, policy=COMPUTE_NO, stream=backend.dev.stream())
    ccfg2 = writer2.configure_compression(data.size)
    writer2.compress(src.ptr, comp.ptr, ccfg2)
    total = writer2.compressed_output_size(comp.ptr)
    image = comp.read(total)
    t = hc.table_offsets(3)
    image[t.crc_uncomp + 4] ^= 1
    comp.write(image)
    dcfg2 = reader.configure_decompression_from(ccfg2)
    reader.decompress(out.ptr, comp.ptr, dcfg2)
    backend.dev.synchronize()
    assert dcfg2.status() == BAD_CRC and np.array_equal(out.read(), data)
    for c in (ccfg, dcfg, ccfg2, dcfg2):
        c.close()
    for m in (writer, reader, writer2):
        m.close()


# ---------------------------------------------------------------------------------------- (f) corruption with a defined verdict

FLIP_SEED = 21
STRICT = {"Cascaded", "Bitcomp", "ANS"}  # tests/test_fuzz_corrupt.py: the kernels agree with the CPU models on accept / reject


def flip_container(fmt):
    """A small container whose chunks a bit flip sometimes breaks and sometimes only changes: match-heavy and entropy
    coded chunks, and stored noise."""
    chunk = 512
    kinds = ["lowcard", "noise", "int32", "text" if fmt != "Bitcomp" else "int32"]
    parts = [sample(k, chunk, i) for i, k in enumerate(kinds)]
    return np.concatenate(parts), chunk


def flip_positions(parsed, per_chunk, seed=FLIP_SEED):
    rng = np.random.RandomState(seed)
    out = []
    for i in range(parsed.num_chunks):
        size = int(parsed.comp_size[i])
        for k in range(per_chunk):
            # every other position in the chunk's first 16 bytes: the codecs without redundancy in their payload (Cascaded,
            # Bitcomp, ANS) notice little else, and both verdicts have to be in the sample
            out.append((i, int(rng.randint(0, min(size, 16) if k % 2 else size)), int(rng.randint(0, 8))))
    return out


@pytest.mark.parametrize("fmt", FORMATS)
def test_payload_bit_flips(backend, oracle, drv, fmt):
    data, chunk = flip_container(fmt)
    opts = (4096, 1, 2, 1, 1) if fmt == "Cascaded" else DEFAULT_OPTS[fmt]
    container, parsed, _ = compress(backend, drv, fmt, data, chunk, opts, COMPUTE_NO, seed=3)
    pieces = chunks_of(data, chunk)
    verifying = Manager.open(drv, fmt, chunk, opts, COMPUTE_VERIFY, backend.dev.stream())
    plain = Manager.open(drv, fmt, chunk, opts, NO_NO, backend.dev.stream())
    positions = flip_positions(parsed, 10 if backend.name == "emu" else 25)
    decodes = undecided = 0
    for i, at, bit in positions:
        bad = container.copy()
        where = parsed.tables.data + int(parsed.comp_offset[i]) + at
        bad[where] ^= 1 << bit
        payload = bad[parsed.tables.data + int(parsed.comp_offset[i]):][: int(parsed.comp_size[i])]
        ok, back = cpu_decode(oracle, fmt, payload, pieces[i].size)
        right_length = ok and back.size == pieces[i].size
        decodes += right_length
        status, out = decompress(backend, drv, bad, mgr=verifying)
        assert status in (CANNOT, BAD_CRC), (i, at, bit, status)
        want = BAD_CRC if right_length else CANNOT  # a decode error outranks the checksum
        if status != want:
            assert fmt not in STRICT, (fmt, i, at, bit, status, want)
            undecided += 1
        status, out = decompress(backend, drv, bad, mgr=plain)  # its guard bytes are checked inside
        assert status in (SUCCESS, CANNOT)
        if fmt in STRICT:
            assert status == (SUCCESS if right_length else CANNOT), (fmt, i, at, bit, status)
        for j, piece in enumerate(pieces):
            if j != i:
                assert np.array_equal(out[j * chunk: (j + 1) * chunk], piece), "another chunk's output changed"
    total = len(positions)
    # the sample has to hold both classes, by the CPU decoders alone
    assert 10 * decodes >= total and 10 * (total - decodes) >= total, (fmt, decodes, total)
    assert 10 * undecided <= total, (fmt, undecided, total)
    verifying.close()
    plain.close()


def corrupted(container, edit):
    bad = container.copy()
    edit(bad)
    return bad


@pytest.mark.parametrize("fmt", FORMATS)
def test_table_corruption(backend, oracle, drv, fmt):
    """Flipped checksum slots, lowered sizes and swapped offsets: every access stays inside the container."""
    chunk = 1024
    opts = (4096, 1, 2, 1, 1) if fmt == "Cascaded" else DEFAULT_OPTS[fmt]
    data = np.concatenate([sample("noise", 2 * chunk, 3), mixed(2 * chunk + 40, 41)])  # chunks 0 and 1: equal lengths
    container, parsed, _ = compress(backend, drv, fmt, data, chunk, opts, COMPUTE_NO)
    n, t = parsed.num_chunks, parsed.tables
    assert int(parsed.comp_size[0]) == int(parsed.comp_size[1])
    verifying = Manager.open(drv, fmt, chunk, opts, NO_IFPRESENT, backend.dev.stream())
    plain = Manager.open(drv, fmt, chunk, opts, COMPUTE_NO, backend.dev.stream())
    for table in (t.crc_uncomp, t.crc_comp):
        for i in (0, n - 1):
            bad = corrupted(container, lambda b: b.__setitem__(table + 4 * i + 2, b[table + 4 * i + 2] ^ 0x10))
            status, out = decompress(backend, drv, bad, mgr=verifying)
            assert status == BAD_CRC and np.array_equal(out, data)
            status, out = decompress(backend, drv, bad, mgr=plain)
            assert status == SUCCESS and np.array_equal(out, data)
    for i in (0, n - 1):
        size = int(parsed.comp_size[i])
        for smaller in (size - 1, size // 2):
            bad = corrupted(container, lambda b: hc.put_u64(b, t.sizes + 8 * i, smaller))
            for m in (verifying, plain):
                status, out = decompress(backend, drv, bad, mgr=m)
                ok, back = cpu_decode(oracle, fmt, parsed.payloads[i][:smaller], min(chunk, data.size - i * chunk))
                assert not (ok and back.size == min(chunk, data.size - i * chunk)), "the CPU decoder accepts the cut chunk"
                assert status != SUCCESS, (fmt, i, smaller, status)
    # two offsets exchanged between chunks of equal length
    def swap(b):
        hc.put_u64(b, t.offsets, int(parsed.comp_offset[1]))
        hc.put_u64(b, t.offsets + 8, int(parsed.comp_offset[0]))
    bad = corrupted(container, swap)
    status, out = decompress(backend, drv, bad, mgr=verifying)
    assert status == BAD_CRC
    status, out = decompress(backend, drv, bad, mgr=plain)
    ok0, back0 = cpu_decode(oracle, fmt, parsed.payloads[1], chunk)  # what now stands in chunk 0's place
    ok1, back1 = cpu_decode(oracle, fmt, parsed.payloads[0], chunk)
    assert ok0 and ok1 and status == SUCCESS
    assert np.array_equal(out[:chunk], back0) and np.array_equal(out[chunk: 2 * chunk], back1)
    assert np.array_equal(out[:chunk], data[chunk: 2 * chunk]) and np.array_equal(out[chunk: 2 * chunk], data[:chunk])
    assert np.array_equal(out[2 * chunk:], data[2 * chunk:])
    verifying.close()
    plain.close()


def test_header_corruption(backend, drv):
    """Each of these throws from configure_decompression / create_manager: no kernel is launched, the output buffer is
    never handed over."""
    chunk = 1024
    data = mixed(4 * chunk + 8, 43)
    container, parsed, _ = compress(backend, drv, "LZ4", data, chunk, policy=COMPUTE_NO)
    lz4 = Manager.open(drv, "LZ4", chunk, stream=backend.dev.stream())
    snappy = Manager.open(drv, "Snappy", chunk, stream=backend.dev.stream())

    def u32(at, v):
        return lambda b: hc.put_u32(b, at, v)

    def u16(at, v):
        return lambda b: b.__setitem__(slice(at, at + 2), np.frombuffer(int(v).to_bytes(2, "little"), dtype=np.uint8))

    cases = {
        "magic": u32(hc.OFF_MAGIC, hc.MAGIC ^ 0x100),
        "version": u16(hc.OFF_VERSION, 2),
        "chunk_size 0": u32(hc.OFF_CHUNK, 0),
        "chunk_size 2^24+1": u32(hc.OFF_CHUNK, (1 << 24) + 1),
        "num_chunks + 1": u32(hc.OFF_COUNT, 6),
        "num_chunks - 1": u32(hc.OFF_COUNT, 4),
        "uncompressed_size grown": lambda b: hc.put_u64(b, hc.OFF_UNCOMP, data.size + chunk),
        "uncompressed_size shrunk": lambda b: hc.put_u64(b, hc.OFF_UNCOMP, data.size - chunk),
        "uncompressed_size 0": lambda b: hc.put_u64(b, hc.OFF_UNCOMP, 0),
    }
    for name, edit in cases.items():
        comp = Buf(backend, container.size, data=corrupted(container, edit))
        with pytest.raises(HlifError) as e:
            lz4.configure_decompression(comp.ptr)
        assert e.value.code == RUNTIME_ERROR, name
        if name in ("magic", "version"):
            with pytest.raises(HlifError) as e:
                Manager.from_buffer(drv, comp.ptr)
            assert e.value.code == RUNTIME_ERROR, name
    # the format id: an unknown one for create_manager and the typed manager, another format's for the typed manager
    for fid in (0, 7, 0xFFFF):
        comp = Buf(backend, container.size, data=corrupted(container, u16(hc.OFF_FORMAT, fid)))
        with pytest.raises(HlifError) as e:
            Manager.from_buffer(drv, comp.ptr)
        assert e.value.code == RUNTIME_ERROR and "format" in str(e.value)
        with pytest.raises(HlifError):
            lz4.configure_decompression(comp.ptr)
    comp = Buf(backend, container.size, data=container)
    with pytest.raises(HlifError) as e:
        snappy.configure_decompression(comp.ptr)
    assert e.value.code == RUNTIME_ERROR and "format" in str(e.value)
    cfg = lz4.configure_decompression(comp.ptr)  # the untouched container is still fine
    cfg.close()
    lz4.close()
    snappy.close()


# ------------------------------------------------------- (g) table entries that point outside the container: emulator only

@pytest.mark.parametrize("fmt", ["LZ4", "Snappy", "ANS", "Bitcomp", "Cascaded", "Deflate"])
@pytest.mark.parametrize("policy", [NO_NO, COMPUTE_VERIFY])
def test_table_entries_outside_the_container(emu, tmp_path_factory, fmt, policy):
    """Host memory only: the container's last byte is the last one in front of a PROT_NONE page, so a read through an
    unconfined table entry is a segfault of this process. Never run on the card."""
    drv = driver(emu, tmp_path_factory)
    chunk = 1024
    opts = (4096, 1, 2, 1, 1) if fmt == "Cascaded" else DEFAULT_OPTS[fmt]
    data = mixed(5 * chunk + 100, 47)
    container, parsed, _ = compress(emu, drv, fmt, data, chunk, opts, COMPUTE_NO)
    n, t = parsed.num_chunks, parsed.tables
    base, span = hc.guarded_mapping(-(-container.size // 4096) + 1)
    at = base + span - container.size
    assert at % 8 == 0
    m = Manager.open(drv, fmt, chunk, opts, policy, None)
    end = int(parsed.comp_offset[n])
    beyond = [end + 8, end + (1 << 20), (1 << 32) + 8, (1 << 63), (1 << 64) - 8]
    edits = []
    for v in beyond:
        edits.append((f"comp_size[{n - 1}] = {v:#x}", lambda b, v=v: hc.put_u64(b, t.sizes + 8 * (n - 1), v)))
        edits.append((f"comp_size[0] = {v:#x}", lambda b, v=v: hc.put_u64(b, t.sizes, v)))
        edits.append((f"comp_offset[2] = {v:#x}", lambda b, v=v: hc.put_u64(b, t.offsets + 16, v)))
        edits.append((f"comp_offset[N] = {v:#x}", lambda b, v=v: hc.put_u64(b, t.offsets + 8 * n, v)))
    # offset[N] too large AND a chunk that reaches into what it falsely declares
    edits.append(("comp_offset[N] and comp_size[N-1] past the end",
                  lambda b: (hc.put_u64(b, t.offsets + 8 * n, end + (1 << 20)), hc.put_u64(b, t.sizes + 8 * (n - 1), 1 << 19))))
    edits.append(("comp_size[1] = the whole data area", lambda b: hc.put_u64(b, t.sizes + 8, end)))
    for name, edit in edits:
        bad = corrupted(container, edit)
        C.memmove(at, bad.ctypes.data, bad.size)
        cfg = m.configure_decompression(at)
        out = Buf(emu, data.size, fill=0x3C)
        m.decompress(out.ptr, at, cfg)
        if name.startswith("comp_offset[N] = "):
            # the chunks themselves are where they were: a larger offset[N] alone harms nothing
            assert cfg.status() == SUCCESS and np.array_equal(out.read(), data), name
        else:
            assert cfg.status() != SUCCESS, name
        assert out.guards_intact(), name
        cfg.close()
    # a smaller offset[N] cuts the last chunks off
    bad = corrupted(container, lambda b: hc.put_u64(b, t.offsets + 8 * n, int(parsed.comp_offset[n - 1])))
    C.memmove(at, bad.ctypes.data, bad.size)
    cfg = m.configure_decompression(at)
    out = Buf(emu, data.size, fill=0x3C)
    m.decompress(out.ptr, at, cfg)
    assert cfg.status() == CANNOT and out.guards_intact()
    assert np.array_equal(out.read()[: (n - 1) * chunk], data[: (n - 1) * chunk])
    # and so does a smaller compressed_size in the header
    bad = corrupted(container, lambda b: hc.put_u64(b, hc.OFF_TOTAL, parsed.compressed_size - 8))
    C.memmove(at, bad.ctypes.data, bad.size)
    cfg2 = m.configure_decompression(at)
    m.decompress(out.ptr, at, cfg2)
    assert cfg2.status() == CANNOT and out.guards_intact()
    cfg.close()
    cfg2.close()
    m.close()


# -------------------------------------------------------------------------------------------------- (h) lifetimes and streams

def test_more_live_configurations_than_one_slab(backend, drv):
    """600 live compression configurations (the status words come in slabs of 512), each with its own status."""
    chunk = 256
    m = Manager.open(drv, "Cascaded", chunk, (4096, 1, 2, 1, 1), NO_NO, backend.dev.stream())
    data = mixed(chunk + 10, 53)
    src = Buf(backend, data.size, data=data)
    cfgs = [m.configure_compression(data.size) for _ in range(600)]
    assert len({c.status_address() for c in cfgs}) == 600
    comp = Buf(backend, cfgs[0].max_compressed_buffer_size)
    picked = [0, 1, 511, 512, 513, 599]
    for i in picked:
        m.compress(src.ptr, comp.ptr, cfgs[i])
    backend.dev.synchronize()
    assert all(c.status() == SUCCESS for c in cfgs)
    container = comp.read(m.compressed_output_size(comp.ptr))
    # decompression configurations: some report an error, the others must not see it
    bad = container.copy()
    bad[hc.table_offsets(2).data + 5] ^= 0xFF
    hc.put_u64(bad, hc.table_offsets(2).sizes, 3)
    good_buf, bad_buf = Buf(backend, container.size, data=container), Buf(backend, bad.size, data=bad)
    out = Buf(backend, data.size, fill=0x3C)
    dcfgs = [m.configure_decompression(good_buf.ptr) for _ in range(600)]
    assert len({c.status_address() for c in dcfgs} | {c.status_address() for c in cfgs}) == 1200
    for i in picked:
        m.decompress(out.ptr, bad_buf.ptr if i % 2 else good_buf.ptr, dcfgs[i])
    backend.dev.synchronize()
    for i, c in enumerate(dcfgs):
        assert c.status() == (CANNOT if i in picked and i % 2 else SUCCESS), i
    for c in cfgs + dcfgs:
        c.close()
    m.close()


def test_configuration_dropped_before_synchronisation(backend, drv):
    """A decompression configuration closed while its kernels may still be in flight: its status word is the LAST one to
    be handed out again, and the configurations made next have statuses of their own."""
    chunk = 4096
    data = mixed(40 * chunk, 59)
    container, parsed, _ = compress(backend, drv, "LZ4", data, chunk, policy=COMPUTE_NO)
    bad = container.copy()
    hc.put_u64(bad, parsed.tables.sizes + 8, 2)
    m = Manager.open(drv, "LZ4", chunk, policy=COMPUTE_VERIFY, stream=backend.dev.stream())
    good_buf, bad_buf = Buf(backend, container.size, data=container), Buf(backend, bad.size, data=bad)
    out1, out2 = Buf(backend, data.size, fill=0x3C), Buf(backend, data.size, fill=0x3C)
    dropped = m.configure_decompression(bad_buf.ptr)
    word = dropped.status_address()
    m.decompress(out1.ptr, bad_buf.ptr, dropped)
    dropped.close()  # no synchronisation in between
    fresh = [m.configure_decompression(good_buf.ptr) for _ in range(8)]
    assert word not in {c.status_address() for c in fresh}, "a word that was just given back was handed out first"
    for c in fresh:
        assert c.status() == SUCCESS
    m.decompress(out2.ptr, good_buf.ptr, fresh[0])
    m.decompress(out1.ptr, bad_buf.ptr, fresh[1])
    backend.dev.synchronize()
    assert fresh[0].status() == SUCCESS and np.array_equal(out2.read(), data)
    assert fresh[1].status() == CANNOT
    assert all(c.status() == SUCCESS for c in fresh[2:])
    assert out1.guards_intact() and out2.guards_intact()
    for c in fresh:
        c.close()
    m.close()


def test_scratch_regrowth_while_work_is_queued(backend, drv):
    """Ten buffers of different sizes and chunk counts, growing and shrinking, through one manager on one stream with
    no synchronisation in between; a verifying policy, so the side stream takes part. Everything is checked at the end."""
    chunk = 1024
    m = Manager.open(drv, "LZ4", chunk, policy=COMPUTE_VERIFY, stream=backend.dev.stream())
    sizes = [3 * chunk + 5, 40 * chunk, chunk - 1, 130 * chunk + 77, 2 * chunk, 300 * chunk + 1, 7, 64 * chunk, 301 * chunk, 9 * chunk]
    if backend.name == "gpu":
        sizes = [s * 16 for s in sizes]
    datas = [mixed(s, 61 + i) for i, s in enumerate(sizes)]
    srcs = [Buf(backend, d.size, data=d) for d in datas]
    ccfgs = [m.configure_compression(d.size) for d in datas]
    comps = [Buf(backend, c.max_compressed_buffer_size) for c in ccfgs]
    outs = [Buf(backend, d.size, fill=0x3C) for d in datas]
    dcfgs = []
    for s, c, cfg, o in zip(srcs, comps, ccfgs, outs):
        m.compress(s.ptr, c.ptr, cfg)
        d = m.configure_decompression_from(cfg)  # does not synchronise
        m.decompress(o.ptr, c.ptr, d)
        dcfgs.append(d)
    backend.dev.synchronize()
    for i, (d, c, cfg, dcfg, o) in enumerate(zip(datas, comps, ccfgs, dcfgs, outs)):
        assert cfg.status() == SUCCESS and dcfg.status() == SUCCESS, i
        assert np.array_equal(o.read(), d) and o.guards_intact() and c.guards_intact(), i
        hc.parse(c.read(m.compressed_output_size(c.ptr)), "LZ4", OPTS["LZ4"](0), True)
    for c in ccfgs + dcfgs:
        c.close()
    m.close()


def test_two_managers_on_two_streams(backend, drv):
    """Interleaved work of two managers on two streams (on the emulator streams are serial: a smoke run there)."""
    if backend.name == "gpu":
        torch = backend.dev.torch
        keep = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        streams = [s.cuda_stream for s in keep]
    else:
        streams = [None, None]
    chunk = 4096
    scale = 64 if backend.name == "gpu" else 1
    fmts = ["LZ4", "ANS"]
    ms = [Manager.open(drv, f, chunk, policy=COMPUTE_VERIFY, stream=s) for f, s in zip(fmts, streams)]
    datas = [[mixed((5 + 3 * r) * chunk * scale + 11 * k, 71 + 10 * k + r) for r in range(4)] for k in range(2)]
    work = []
    for r in range(4):
        for k in range(2):
            d = datas[k][r]
            src = Buf(backend, d.size, data=d)
            backend.dev.synchronize()  # the upload ran on the device's current stream
            cfg = ms[k].configure_compression(d.size)
            comp, out = Buf(backend, cfg.max_compressed_buffer_size), Buf(backend, d.size, fill=0x3C)
            backend.dev.synchronize()
            ms[k].compress(src.ptr, comp.ptr, cfg)
            dcfg = ms[k].configure_decompression_from(cfg)
            ms[k].decompress(out.ptr, comp.ptr, dcfg)
            work.append((k, d, src, comp, out, cfg, dcfg))
    backend.dev.synchronize()
    for k, d, src, comp, out, cfg, dcfg in work:
        assert cfg.status() == SUCCESS and dcfg.status() == SUCCESS
        assert np.array_equal(out.read(), d) and out.guards_intact() and comp.guards_intact()
        hc.parse(comp.read(ms[k].compressed_output_size(comp.ptr)), fmts[k], OPTS[fmts[k]](0), True)
        cfg.close()
        dcfg.close()
    for m in ms:
        m.close()


@pytest.mark.parametrize("dtype,width", [(1, 1), (2, 2), (3, 2), (4, 4), (5, 4), (6, 8), (7, 8)])
def test_cascaded_element_width(backend, oracle, drv, dtype, width):
    opts = (4096, dtype, 2, 1, 1)
    m = Manager.open(drv, "Cascaded", 4096, opts, stream=backend.dev.stream())
    for nbytes in (8 * 100, 8 * 100 + 1, 8 * 100 + 2, 8 * 100 + 4):
        if nbytes % width:
            with pytest.raises(HlifError) as e:
                m.configure_compression(nbytes)
            assert e.value.code == INVALID_ARGUMENT
        else:
            m.configure_compression(nbytes).close()
    m.close()
    if width > 1:
        odd = Manager.open(drv, "Cascaded", 4096 + width // 2, opts, stream=backend.dev.stream())
        with pytest.raises(HlifError) as e:
            odd.configure_compression(8 * 100)
        assert e.value.code == INVALID_ARGUMENT
        odd.close()
    else:
        roundtrip(backend, oracle, drv, "Cascaded", mixed(4097 + 333, 83), 4097, opts)
    data = sample("int32", 3 * 4096 + 8 * 11, dtype)
    roundtrip(backend, oracle, drv, "Cascaded", data, 4096, opts)


@pytest.mark.parametrize("fmt", FORMATS)
def test_invalid_format_options(backend, drv, fmt):
    with pytest.raises(HlifError) as e:
        Manager.open(drv, fmt, 4096, BAD_OPTS[fmt])
    assert e.value.code == RUNTIME_ERROR and "options" in str(e.value)
    Manager.open(drv, fmt, 4096, OTHER_OPTS[fmt]).close()
