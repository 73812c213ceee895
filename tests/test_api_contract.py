"""The argument contract of the batched C API and the behaviour of the per-chunk frame, one table row per format.

(a) What every entry point answers to NULL pointers, bad options, oversized chunks and empty batches, and in which
    order. The formats differ in places (Zstd's oversize status, the temp buffers Zstd and Cascaded require, Cascaded's
    ErrorNotSupported); the differences are recorded here as they are, not harmonised. No case of (a) launches a kernel:
    every call returns from its argument checks.
(b) What the frame around a codec's decode_chunk / encode_chunk does whatever the codec: the tail guard of a batch
    that does not fill its last workgroup, optional status and size arrays, the capacity clamp, the refusal of a chunk
    larger than the caller declared. Five chunks of 1-4 KiB: 5 is no multiple of any kernel's waves per workgroup.
    The codec files assert parts of this for their own format at other sizes: optional arrays in
    tests/test_deflate.py::test_unchecked_and_without_sizes and the round trips of tests/test_bitcomp.py, the capacity in
    tests/test_deflate.py::test_output_capacity_is_respected, the refusal (size 0, without the untouched slot) in
    tests/test_lz4_encode.py::test_oversized_chunk_is_refused_by_every_compressor. Here it is one rule, at one small
    shape, for all eight formats.
"""
import ctypes as C
import zlib
from collections import namedtuple

import numpy as np
import pytest

import zstd_frames as zf
from nvcomp_amd import _lib
from nvcomp_amd.batched import empty_batch, make_batch, read_batch

S = _lib.NvcompStatus
LIMIT = 1 << 24  # nvcomp<Format>CompressionMaxAllowedChunkSize of every format but Deflate

# fmt, good options, bad options, largest max_uncompressed_chunk_bytes, compress temp bytes of a batch of n,
# decompress temp bytes of a batch of n, max output chunk size of 65 536 bytes
Row = namedtuple("Row", "fmt opts bad limit ctemp dtemp bound")
COMPRESSORS = [
    Row("LZ4", (0,), (6,), LIMIT, lambda n: 16 if n else 0, lambda n: 16 if n else 0, 65809),  # data_type LONGLONG: refused
    Row("Snappy", (0,), (1,), LIMIT, lambda n: 16 if n else 0, lambda n: 16 if n else 0, 76490),
    Row("Cascaded", (4096, 4, 2, 1, 1), (4096, 4, 8, 1, 1), LIMIT, lambda n: 4 * n, lambda n: 4 * n,
        20 + 4 * 16 + 8 * 16 + 65536),
    Row("Bitcomp", (0, 1), (2, 1), LIMIT, lambda n: 0, lambda n: 0, None),
    Row("ANS", (0,), (1,), LIMIT, lambda n: 0, lambda n: 0, 65552),
    Row("Deflate", (0,), (3,), 1 << 16, lambda n: 0, lambda n: 0, None),
]
BY_FMT = {r.fmt: r for r in COMPRESSORS}
DECODERS = [r.fmt for r in COMPRESSORS] + ["Gzip", "Zstd"]
# DecompressAsync requires a temp buffer: NULL is ErrorInvalidValue
NEEDS_TEMP = ("Cascaded", "Zstd")
ZSTD_HEADER = 64  # zstd::kTempHeader
ZSTD_MAX_WAVES = 3072
ZSTD_BLOCK_MAX = 128 * 1024


def fn(backend, fmt, name):
    return getattr(backend.lib, f"nvcompBatched{fmt}{name}")


def opts_of(row, values):
    return _lib.OPTS[row.fmt](*values)


def zstd_slot(max_chunk):
    s = min(max_chunk, ZSTD_BLOCK_MAX)
    return (max(s, 16) + 15) & ~15


def dec_temp_bytes(fmt, n, max_chunk):
    if fmt == "Zstd":
        return ZSTD_HEADER + max(min(n, ZSTD_MAX_WAVES), 1) * zstd_slot(max_chunk)
    return 0 if fmt == "Gzip" else BY_FMT[fmt].dtemp(n)


@pytest.fixture
def some_ptr(backend):
    """A device address aligned to 64 bytes with 4 KiB of zeros behind it. The calls of (a) never get as far as reading it."""
    buf = backend.dev.upload(np.zeros(4096 + 64, dtype=np.uint8))
    yield (backend.dev.ptr(buf) + 63) & ~63
    del buf


# ---- (a) the host contract ----

@pytest.mark.parametrize("row", COMPRESSORS, ids=lambda r: r.fmt)
def test_compress_queries(backend, row):
    good, bad = opts_of(row, row.opts), opts_of(row, row.bad)
    out = C.c_size_t(0xABCD)
    temp, temp_ex, bound = (fn(backend, row.fmt, n) for n in ("CompressGetTempSize", "CompressGetTempSizeEx",
                                                            "CompressGetMaxOutputChunkSize"))
    # a NULL result pointer, whatever else is wrong
    for chunk in (65536, row.limit + 1):
        assert temp(7, chunk, good, None) == S.ErrorInvalidValue
        assert temp_ex(7, chunk, good, None, 1 << 30) == S.ErrorInvalidValue
        assert bound(chunk, good, None) == S.ErrorInvalidValue
    # bad options come before the chunk size
    for chunk in (65536, row.limit + 1):
        assert temp(7, chunk, bad, C.byref(out)) == S.ErrorInvalidValue
        assert temp_ex(7, chunk, bad, C.byref(out), 1 << 30) == S.ErrorInvalidValue
        assert bound(chunk, bad, C.byref(out)) == S.ErrorInvalidValue
    # limit + 1, and nothing written
    assert temp(7, row.limit + 1, good, C.byref(out)) == S.ErrorChunkSizeTooLarge
    assert temp_ex(7, row.limit + 1, good, C.byref(out), 1 << 30) == S.ErrorChunkSizeTooLarge
    assert bound(row.limit + 1, good, C.byref(out)) == S.ErrorChunkSizeTooLarge
    assert out.value == 0xABCD
    # exactly the limit; Ex answers what the plain query answers
    for n in (0, 1, 7, 5000):
        for chunk in (1, 65536 if row.limit >= 65536 else row.limit, row.limit):
            a, b = C.c_size_t(0xABCD), C.c_size_t(0xDCBA)
            assert temp(n, chunk, good, C.byref(a)) == S.Success
            assert temp_ex(n, chunk, good, C.byref(b), 12345) == S.Success
            assert a.value == b.value == row.ctemp(n)
    assert bound(row.limit, good, C.byref(out)) == S.Success and out.value >= row.limit
    assert bound(65536, good, C.byref(out)) == S.Success
    assert out.value == row.bound if row.bound is not None else out.value >= 65536


@pytest.mark.parametrize("fmt", DECODERS)
def test_decompress_temp_queries(backend, fmt):
    temp, temp_ex = fn(backend, fmt, "DecompressGetTempSize"), fn(backend, fmt, "DecompressGetTempSizeEx")
    assert temp(7, 65536, None) == S.ErrorInvalidValue
    assert temp_ex(7, 65536, None, 1 << 30) == S.ErrorInvalidValue
    out, out_ex = C.c_size_t(0xABCD), C.c_size_t(0xDCBA)
    # only Zstd looks at the chunk size, and answers ErrorInvalidValue where the compressors say ErrorChunkSizeTooLarge
    over = S.ErrorInvalidValue if fmt == "Zstd" else S.Success
    assert temp(7, LIMIT + 1, C.byref(out)) == over
    assert temp_ex(7, LIMIT + 1, C.byref(out_ex), 1 << 30) == over
    if fmt == "Zstd":
        assert (out.value, out_ex.value) == (0xABCD, 0xDCBA)
    for n in (0, 1, 7, 5000):
        for chunk in (1, 1000, 65536, LIMIT):
            assert temp(n, chunk, C.byref(out)) == S.Success and out.value == dec_temp_bytes(fmt, n, chunk)
            assert temp_ex(n, chunk, C.byref(out_ex), 1 << 30) == S.Success and out_ex.value == out.value
    if fmt == "Zstd":
        # Ex: no block regenerates more literals than the whole batch holds -- min(max_total, max_chunk) stands for the chunk
        assert temp_ex(7, 65536, C.byref(out_ex), 1000) == S.Success and out_ex.value == dec_temp_bytes(fmt, 7, 1000)
        assert temp_ex(7, LIMIT + 1, C.byref(out_ex), 1000) == S.Success and out_ex.value == dec_temp_bytes(fmt, 7, 1000)
        assert temp_ex(7, 1000, C.byref(out_ex), LIMIT + 1) == S.Success and out_ex.value == dec_temp_bytes(fmt, 7, 1000)


@pytest.mark.parametrize("row", COMPRESSORS, ids=lambda r: r.fmt)
def test_compress_async_arguments(backend, row, some_ptr):
    good, bad = opts_of(row, row.opts), opts_of(row, row.bad)
    call = fn(backend, row.fmt, "CompressAsync")
    p, stream = some_ptr, backend.dev.stream()
    # bad options first, then the chunk size, then the empty batch, then the pointers
    assert call(None, None, row.limit + 1, 0, None, 0, None, None, bad, stream) == S.ErrorInvalidValue
    assert call(p, p, 4096, 1, p, 4096, p, p, bad, stream) == S.ErrorInvalidValue
    assert call(None, None, row.limit + 1, 0, None, 0, None, None, good, stream) == S.ErrorChunkSizeTooLarge
    assert call(None, None, row.limit + 1, 1, None, 0, None, None, good, stream) == S.ErrorChunkSizeTooLarge
    assert call(None, None, row.limit, 0, None, 0, None, None, good, stream) == S.Success
    assert call(None, None, 4096, 0, None, 0, None, None, good, stream) == S.Success
    for null in range(4):
        in_ptrs, in_bytes, out_ptrs, out_bytes = (None if k == null else p for k in range(4))
        assert call(in_ptrs, in_bytes, 4096, 1, p, 4096, out_ptrs, out_bytes, good, stream) == S.ErrorInvalidValue, null


def test_cascaded_refuses_options_its_decoder_cannot_hold(backend):
    """Sub-chunks of 16 KiB of bytes with seven RLE layers need more LDS than the decoder's last pass has: valid
    options (the queries accept them), ErrorNotSupported from CompressAsync -- behind the empty batch and the pointers.
    The arrays are real ones of one chunk, so that a library that did launch would be caught by the assert, not by a fault."""
    opts = _lib.CascadedOpts(16384, 0, 7, 1, 1)
    out = C.c_size_t(0)
    assert backend.lib.nvcompBatchedCascadedCompressGetTempSize(1, 16384, opts, C.byref(out)) == S.Success
    assert backend.lib.nvcompBatchedCascadedCompressGetMaxOutputChunkSize(16384, opts, C.byref(out)) == S.Success
    d = backend.dev
    src = make_batch(d, [np.zeros(16384, dtype=np.uint8)], align=8)
    dst = empty_batch(d, [out.value], align=8)
    temp = d.empty(4096)
    call = backend.lib.nvcompBatchedCascadedCompressAsync
    a, b, c, e, t, stream = d.ptr(src.ptrs), d.ptr(src.sizes), d.ptr(dst.ptrs), d.ptr(dst.sizes), d.ptr(temp), d.stream()
    assert call(a, b, 16384, 1, t, 4096, c, e, opts, stream) == S.ErrorNotSupported
    assert call(a, b, 16384, 1, None, 0, c, e, opts, stream) == S.ErrorNotSupported
    assert call(None, None, 16384, 0, None, 0, None, None, opts, stream) == S.Success
    assert call(None, b, 16384, 1, t, 4096, c, e, opts, stream) == S.ErrorInvalidValue
    d.synchronize()


@pytest.mark.parametrize("fmt", DECODERS)
def test_decompress_async_arguments(backend, fmt, some_ptr):
    call = fn(backend, fmt, "DecompressAsync")
    p, stream = some_ptr, backend.dev.stream()
    assert call(None, None, None, None, 0, None, 0, None, None, stream) == S.Success
    for null in range(4):
        comp_ptrs, comp_bytes, out_caps, out_ptrs = (None if k == null else p for k in range(4))
        for actual, statuses in ((p, p), (None, None)):
            assert call(comp_ptrs, comp_bytes, out_caps, actual, 1, p, 4096, out_ptrs, statuses, stream) == S.ErrorInvalidValue, null
    if fmt in NEEDS_TEMP:
        assert call(p, p, p, p, 1, None, 4096, p, p, stream) == S.ErrorInvalidValue
    if fmt == "Cascaded":  # one word per chunk
        assert call(p, p, p, p, 2, p, 7, p, p, stream) == S.ErrorInvalidValue
    if fmt == "Zstd":  # aligned to 16 bytes, the header and one slot of 16 bytes
        assert call(p, p, p, p, 1, p + 8, 4096, p, p, stream) == S.ErrorInvalidValue
        assert call(p, p, p, p, 1, p, ZSTD_HEADER + 15, p, p, stream) == S.ErrorInvalidValue


@pytest.mark.parametrize("fmt", DECODERS)
def test_get_decompress_size_async_arguments(backend, fmt, some_ptr):
    call = fn(backend, fmt, "GetDecompressSizeAsync")
    p, stream = some_ptr, backend.dev.stream()
    assert call(None, None, None, 0, stream) == S.Success
    for null in range(3):
        a, b, c = (None if k == null else p for k in range(3))
        assert call(a, b, c, 1, stream) == S.ErrorInvalidValue, null


# ---- (b) the frame ----

SIZES = (1024, 4096, 2504, 3000, 1784)


def plain_chunks():
    r = np.random.RandomState(7)
    words = [b"alpha ", b"beta ", b"gamma ", b"delta ", b"0123456789", b"\x00\x00\x00\x00"]
    out = []
    for n in SIZES:
        text = b"".join(words[k] for k in r.randint(0, len(words), n // 4))[: n - 64]
        out.append(np.frombuffer(text + r.bytes(n - len(text)), dtype=np.uint8).copy())
    return out


def zstd_frame(data):
    f = zf.Frame(fcs_bytes=2)
    f.raw(data[: len(data) // 3])
    f.raw(data[len(data) // 3:], last=True)
    return np.frombuffer(f.bytes(), dtype=np.uint8).copy()


_batches = {}


def compressed_batch(backend, fmt):
    """(chunks, their streams), made once per backend and format."""
    key = (backend.name, fmt)
    if key not in _batches:
        chunks = plain_chunks()
        if fmt == "Gzip":
            comp = []
            for c in chunks:
                o = zlib.compressobj(6, zlib.DEFLATED, 15 | 16)
                comp.append(np.frombuffer(o.compress(c.tobytes()) + o.flush(), dtype=np.uint8).copy())
        elif fmt == "Zstd":
            comp = [zstd_frame(c.tobytes()) for c in chunks]
        else:
            comp = backend.codec(fmt).compress(chunks)
        _batches[key] = (chunks, comp)
    return _batches[key]


@pytest.mark.parametrize("fmt", DECODERS)
def test_status_and_size_arrays_are_optional(backend, fmt):
    chunks, comp = compressed_batch(backend, fmt)
    codec = backend.codec(fmt)
    caps = [c.size for c in chunks]
    outs, actual, status = codec.decompress(comp, caps, comp_align=8, out_align=8)
    assert (status == S.Success).all() and actual.tolist() == caps
    assert all(np.array_equal(o, c) for o, c in zip(outs, chunks))
    outs2, actual2, status2 = codec.decompress(comp, caps, checked=False, comp_align=8, out_align=8)
    assert status2 is None and actual2.tolist() == caps
    assert all(np.array_equal(o, c) for o, c in zip(outs2, chunks))
    outs3, actual3, status3 = codec.decompress(comp, caps, want_actual=False, comp_align=8, out_align=8)
    assert actual3 is None and (status3 == S.Success).all()
    assert all(np.array_equal(o, c) for o, c in zip(outs3, chunks))
    sizes = codec.get_decompress_size(comp, comp_align=8)
    assert sizes.tolist() == caps


@pytest.mark.parametrize("fmt", DECODERS)
def test_capacity_one_byte_short(backend, fmt):
    """The chunk fails alone: status, size 0, nothing behind its slot (BatchedCodec.decompress checks the guard bytes
    behind every slot, which for the short slot start at the chunk's last byte), neighbours intact."""
    chunks, comp = compressed_batch(backend, fmt)
    codec = backend.codec(fmt)
    caps = [c.size for c in chunks]
    caps[2] -= 1
    for checked, want_actual in ((True, True), (False, True), (True, False)):
        outs, actual, status = codec.decompress(comp, caps, checked=checked, want_actual=want_actual, comp_align=8, out_align=8)
        if checked:
            assert status.tolist() == [S.Success, S.Success, S.ErrorCannotDecompress, S.Success, S.Success]
        if want_actual:
            assert actual.tolist() == [caps[0], caps[1], 0, caps[3], caps[4]]
        for k in (0, 1, 3, 4):
            assert np.array_equal(outs[k], chunks[k]), k


@pytest.mark.parametrize("row", COMPRESSORS, ids=lambda r: r.fmt)
def test_chunk_larger_than_declared_is_not_compressed(backend, row):
    chunks = plain_chunks()
    codec = backend.codec(row.fmt)
    d = backend.dev
    declared = 3000  # chunk 1 (4 096 bytes) is larger; chunk 3 is exactly this
    n = len(chunks)
    src = make_batch(d, chunks, align=8)
    max_out = codec.max_compressed_size(declared)
    stride = (max_out + 7) & ~7
    dst = empty_batch(d, [stride] * n, stride=stride, fill=0xA5)
    dst.sizes = d.upload(np.full(n, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
    tb = codec.compress_temp_size(n, declared)
    temp = d.empty(tb) if tb else None
    assert codec.compress_async(src, dst, declared, temp, tb) == S.Success
    d.synchronize()
    sizes = d.download(dst.sizes).view(np.uint64)[:n]
    assert sizes[1] == 0 and (sizes <= max_out).all() and all(sizes[k] > 0 for k in (0, 2, 3, 4))
    slots = read_batch(d, dst, [stride] * n)
    assert (slots[1] == 0xA5).all(), "the refused chunk's output slot was written"
    keep = (0, 2, 3, 4)
    outs, actual, status = codec.decompress([slots[k][: int(sizes[k])] for k in keep], [chunks[k].size for k in keep],
                                            comp_align=8, out_align=8)
    assert (status == S.Success).all() and actual.tolist() == [chunks[k].size for k in keep]
    assert all(np.array_equal(o, chunks[k]) for o, k in zip(outs, keep))
