"""The LZ4 / Snappy launches with every kind of temp buffer. One helper (common/api_batch.hip.h: launch_persistent) decides
between persistent waves drawing tickets from the caller's temp buffer and one place per chunk, statically: a buffer that
is NULL, misaligned or too small for the counter must give the same bytes as the one the size query asks for."""
import numpy as np
import pytest

from nvcomp_amd import datasets
from nvcomp_amd.batched import BatchedCodec, empty_batch, make_batch, read_batch


def small_chunks(count):
    """`count` chunks of 160 ... 384 bytes of the mix."""
    sizes = 160 + (np.arange(count) * 37) % 225
    data = datasets.silesia_style(int(sizes.sum()), 11, chunk=4096)
    ends = np.cumsum(sizes)
    return [data[int(e - s): int(e)] for s, e in zip(sizes, ends)]


def temp_arguments(dev, temp_bytes):
    """(a) what the query asks for, (b) NULL, (c) the same buffer from its third byte on, (d) two bytes."""
    assert temp_bytes >= 8
    whole = dev.empty(temp_bytes)
    assert dev.ptr(whole) % 4 == 0
    return [("query", whole, temp_bytes), ("null", None, 0), ("misaligned", whole[2:], temp_bytes - 2), ("two bytes", dev.empty(2), 2)]


def path_library(backend, path):
    from conftest import emu_path_library, gpu_path_library

    if path == "team" and backend.name == "emu":
        return backend.lib  # the shipped thresholds: 257 ... 512 chunks run the persistent eight-wave teams
    return (emu_path_library if backend.name == "emu" else gpu_path_library)(path)


@pytest.mark.parametrize("path", ["chase", "team"])
@pytest.mark.parametrize("fmt", ["LZ4", "Snappy"])
def test_decompress_with_any_temp_buffer(backend, oracle, fmt, path):
    """Batches just past what stays resident, so that the buffer of the query really hands out tickets."""
    count = {("emu", "chase"): 12, ("emu", "team"): 300, ("gpu", "chase"): 8200, ("gpu", "team"): 600}[backend.name, path]
    chunks = small_chunks(count)
    enc = oracle.lz4_compress if fmt == "LZ4" else oracle.snappy_compress
    d = backend.dev
    codec = BatchedCodec(path_library(backend, path), d, fmt)
    cb = make_batch(d, [enc(c) for c in chunks], align=1)
    caps = [c.size for c in chunks]
    for name, temp, temp_bytes in temp_arguments(d, codec.decompress_temp_size(count, max(caps))):
        ob = empty_batch(d, caps, fill=0xA5)
        actual = d.upload(np.full(count, 0xDEADBEEF, dtype=np.uint64).view(np.uint8))
        statuses = d.upload(np.full(count, -1, dtype=np.int32).view(np.uint8))
        rc = codec.decompress_async(cb, ob, actual, statuses, temp, temp_bytes)
        d.synchronize()
        assert rc == 0, name
        assert (d.download(statuses).view(np.int32)[:count] == 0).all(), name
        assert d.download(actual).view(np.uint64)[:count].tolist() == caps, name
        # the slots are packed: the slab is the chunks one after another, so every path gives the same bytes
        assert np.array_equal(d.download(ob.slab)[: sum(caps)], np.concatenate(chunks)), name


@pytest.mark.parametrize("fmt,data_type", [("LZ4", 0), ("LZ4", 2), ("LZ4", 4), ("Snappy", None)])
def test_compress_with_any_temp_buffer(backend, oracle, fmt, data_type):
    """LZ4 as CHAR (the wide compressor), SHORT and INT (the strided ones), and Snappy. Every output decodes to the input
    with the CPU oracle; on the card the four temp arguments also give the same compressed bytes. The emulator cannot show
    the latter: it runs the lanes of a wave in a fresh pseudo-random order at every step (tests/emu/emu.cpp), which lane's
    position a hash-table slot keeps follows that order, and two calls with the SAME temp buffer already differ there (in
    10 of 24 chunks when this test was written)."""
    count = 12 if backend.name == "emu" else 8200
    chunks = small_chunks(count)
    dec = oracle.lz4_decompress if fmt == "LZ4" else oracle.snappy_decompress
    d = backend.dev
    codec = backend.codec(fmt, None if data_type is None else (data_type,))
    src = make_batch(d, chunks, align=8)
    max_chunk = max(c.size for c in chunks)
    max_out = codec.max_compressed_size(max_chunk)
    first = None
    for name, temp, temp_bytes in temp_arguments(d, codec.compress_temp_size(count, max_chunk)):
        dst = empty_batch(d, [max_out] * count, stride=max_out)
        rc = codec.compress_async(src, dst, max_chunk, temp, temp_bytes)
        d.synchronize()
        assert rc == 0, name
        sizes = d.download(dst.sizes).view(np.uint64)[:count]
        assert (sizes > 0).all() and (sizes <= max_out).all(), name
        comp = read_batch(d, dst, sizes)
        if first is None or backend.name == "emu":
            for cc, c in zip(comp, chunks):
                rc, out = dec(cc, c.size)
                assert rc == 0 and np.array_equal(out, c), name
        if first is None:
            first = comp
        elif backend.name == "gpu":
            assert all(np.array_equal(x, y) for x, y in zip(comp, first)), name
