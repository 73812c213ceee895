"""Batched standard CRC-32 (include/nvcomp/crc32.h) against Python's zlib.crc32. Every test without a `gpu` mark runs on
the emulator (-m "not gpu") and on the MI355X (-m gpu) through the `backend` fixture; the large shapes run on the card
only. Exact: every checksum, every guard word."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

from nvcomp_amd import datasets
from nvcomp_amd._lib import NvcompStatus
from nvcomp_amd.batched import crc32, make_batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "nvcomp", "crc32.h")

TILE = 2048               # bytes one wave walks per step (hlif/crc32.hip.h: 64 lanes x 32 bytes)
MIN_SEGMENT = 64 << 10    # api/crc32_api.hip: a split segment is at least this long
EMU_WAVES = 8             # the emulator's card: one CU keeping two workgroups of four waves resident
GUARD = 16
GARBAGE = 0xDEADBEEF


def want(buf):
    return zlib.crc32(np.ascontiguousarray(buf).tobytes()) & 0xFFFFFFFF


def waves_per_chunk(resident, num_chunks):
    return max(1, -(-resident // num_chunks))


def segments(n, t):
    """[lo, hi) of every non-empty segment of a chunk of n bytes with t waves (api/crc32_api.hip)."""
    s = max(-(-(-(-n // t)) // TILE) * TILE, MIN_SEGMENT)
    return [(lo, min(lo + s, n)) for lo in range(0, n, s)]


def call(backend, ptrs, sizes):
    """nvcompBatchedCRC32Async over raw device pointers. The output holds len(ptrs) words prefilled with garbage and
    GUARD guard words behind them. Returns (status, the output words, the guard words)."""
    dev = backend.dev
    n = len(ptrs)
    out = dev.upload(np.full(n + GUARD, GARBAGE, dtype=np.uint32).view(np.uint8))
    p = dev.upload(np.asarray(ptrs, dtype=np.uint64).view(np.uint8))
    z = dev.upload(np.asarray(sizes, dtype=np.uint64).view(np.uint8))
    rc = backend.lib.nvcompBatchedCRC32Async(dev.ptr(p), dev.ptr(z), n, dev.ptr(out), dev.stream())
    dev.synchronize()
    host = dev.download(out, 4 * (n + GUARD)).view(np.uint32)
    return rc, host[:n].copy(), host[n:].copy()


def check(backend, chunks, base_misalign=0):
    """CRC every chunk of a packed slab through the raw call; results and guards exact."""
    dev = backend.dev
    batch = make_batch(dev, chunks, base_misalign=base_misalign)
    base = dev.ptr(batch.slab)
    ptrs = [base + int(o) for o in batch.offsets]
    rc, got, guard = call(backend, ptrs, [c.size for c in chunks])
    assert rc == NvcompStatus.Success
    assert (guard == GARBAGE).all(), "the call wrote past num_chunks outputs"
    expect = [want(c) for c in chunks]
    bad = [i for i, (g, w) in enumerate(zip(got.tolist(), expect)) if g != w]
    assert not bad, f"{len(bad)} wrong checksums, first: chunk {bad[0]} of {chunks[bad[0]].size} bytes"


def rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# known answers


def test_check_value(backend):
    assert crc32(backend.lib, backend.dev, [np.frombuffer(b"123456789", np.uint8)]).tolist() == [0xCBF43926]


def test_empty(backend):
    assert crc32(backend.lib, backend.dev, [np.zeros(0, np.uint8)]).tolist() == [0]


def test_every_single_byte(backend):
    chunks = [np.array([b], np.uint8) for b in range(256)]
    assert crc32(backend.lib, backend.dev, chunks).tolist() == [want(c) for c in chunks]


# ---------------------------------------------------------------------------------------------------------------------
# sizes and alignments


def test_every_size_to_300(backend):
    data = rand(300, 1)
    check(backend, [data[:n] for n in range(301)])


BOUNDARY_SIZES = (2047, 2048, 2049, 4095, 4096, 4097, 65535, 65536, 65537, 131071, 131072, 131073, 3 * 65536 + 1000,
                  8 * 65536 - 1, 8 * 65536 + 1, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1000003)


@pytest.mark.parametrize("n", BOUNDARY_SIZES)
def test_tile_and_segment_boundaries_alone(backend, n):
    """Batch of one: the widest split."""
    check(backend, [rand(n, n)])


def test_tile_and_segment_boundaries_batched(backend):
    check(backend, [rand(n, n + 1) for n in BOUNDARY_SIZES])


@pytest.mark.parametrize("offset", range(16))
def test_pointer_offsets(backend, offset):
    """Chunks that start at every offset 0..15 into a slab, sizes across the tile and segment edges."""
    check(backend, [rand(n, offset) for n in (1, 5, 33, 2049, 70001)], base_misalign=offset)
    check(backend, [rand(70001 + offset, offset)], base_misalign=offset)


# ---------------------------------------------------------------------------------------------------------------------
# batch shapes


@pytest.mark.parametrize("count", [1, 2, 3])
def test_small_batches(backend, count):
    check(backend, [rand(200000 + 7919 * i, 10 + i) for i in range(count)])


def test_batch_of_1000(backend):
    sizes = np.random.default_rng(5).integers(0, 5000, 1000)
    check(backend, [rand(int(n), i) for i, n in enumerate(sizes)])


def test_mixed_batch(backend):
    check(backend, [rand(0, 0), rand(1, 1), rand(65536, 2), rand(1 << 20, 3)])


def test_same_pointer_twice(backend):
    dev = backend.dev
    data = rand(150001, 7)
    buf = dev.upload(data)
    p = dev.ptr(buf)
    rc, got, guard = call(backend, [p, p, p + 1], [data.size, data.size, data.size - 1])
    assert rc == NvcompStatus.Success and (guard == GARBAGE).all()
    assert got.tolist() == [want(data)] * 2 + [want(data[1:])]


@pytest.mark.parametrize("count", [1, 3, 64])
def test_empty_chunk_with_null_pointer(backend, count):
    dev = backend.dev
    data = rand(100000, 8)
    buf = dev.upload(data)
    ptrs = [0] * count
    sizes = [0] * count
    ptrs[-1], sizes[-1] = dev.ptr(buf), data.size
    rc, got, guard = call(backend, ptrs, sizes)
    assert rc == NvcompStatus.Success and (guard == GARBAGE).all()
    assert got.tolist() == [0] * (count - 1) + [want(data)]


# ---------------------------------------------------------------------------------------------------------------------
# the split path


LOG_SCRIPT = """
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {repo!r} + '/tests')
import numpy as np
import conftest
from nvcomp_amd.batched import crc32
if sys.argv[1] == 'emu':
    lib, dev = conftest.emu_library(), conftest.HostDevice()
else:
    import nvcomp_amd
    lib, dev = nvcomp_amd.load_library(), nvcomp_amd.TorchDevice('cuda:0')
for count in (1, 2, 3, 5, 8, 9, 1000):
    crc32(lib, dev, [np.zeros(1, np.uint8)] * count)
"""


def launch_shapes(name, tmp_path):
    """waves_per_chunk the library logs (NVCOMP_LOG_LEVEL=4) for batches of 1, 2, 3, 5, 8, 9 and 1 000 chunks."""
    log = tmp_path / "crc.log"
    env = dict(os.environ, NVCOMP_LOG_LEVEL="4", NVCOMP_LOG_FILE=str(log))
    subprocess.run([sys.executable, "-c", LOG_SCRIPT.format(repo=REPO), name], check=True, env=env, timeout=600)
    text = log.read_text()
    counts = [int(c) for c in re.findall(r"nvcompBatchedCRC32Async\(num_chunks=(\d+),", text)]
    shapes = [int(t) for t in re.findall(r"nvcompBatchedCRC32Async: waves_per_chunk=(\d+) ", text)]
    assert counts == [1, 2, 3, 5, 8, 9, 1000] and len(shapes) == len(counts), text
    return dict(zip(counts, shapes))


def test_split_is_taken(backend, tmp_path):
    """The batch size alone sets the waves per chunk: ceil(resident waves / chunks). A batch of one gets every resident
    wave; the emulator's card keeps EMU_WAVES resident."""
    shapes = launch_shapes(backend.name, tmp_path)
    resident = shapes[1]
    assert resident > 1
    if backend.name == "emu":
        assert resident == EMU_WAVES
    for count, t in shapes.items():
        assert t == waves_per_chunk(resident, count), (count, t)


@pytest.mark.parametrize("n, used", [(3 * 65536 + 1000, 4), (1000003, 8), (8 * 65536 + 1, 8)])
def test_split_segments(backend, n, used):
    """A batch of one on the emulator's card: T = 8 waves, the last segment ends inside a tile, and (3 x 64 KiB + 1 000
    bytes, under the segment floor of 64 KiB per wave) four waves have nothing to do."""
    t = waves_per_chunk(EMU_WAVES, 1)
    segs = segments(n, t)
    assert t == 8 and len(segs) == used
    assert (segs[-1][1] - segs[-1][0]) % TILE != 0
    check(backend, [rand(n, 99)])


def test_split_three_chunks_mixed(backend):
    """T = 3 on the emulator: one chunk split in three, one empty, one split in two."""
    sizes = [3 * 70001, 0, 65536 + 3]
    assert [len(segments(n, 3)) for n in sizes] == [3, 0, 2]
    check(backend, [rand(n, i) for i, n in enumerate(sizes)])


# ---------------------------------------------------------------------------------------------------------------------
# output buffer and arguments


@pytest.mark.parametrize("count", [1, 2, 9, 300])
def test_output_garbage_and_guards(backend, count):
    """Outputs prefilled with garbage (the split path zeroes and XORs, the one-wave path stores) and guard words behind."""
    check(backend, [rand(1000 + 37 * i if count > 2 else 150000 + i, i) for i in range(count)])


def test_argument_checks(backend):
    dev = backend.dev
    data = rand(1000, 3)
    buf = dev.upload(data)
    ptrs = dev.upload(np.array([dev.ptr(buf)], np.uint64).view(np.uint8))
    sizes = dev.upload(np.array([data.size], np.uint64).view(np.uint8))
    out = dev.upload(np.full(4, GARBAGE, np.uint32).view(np.uint8))
    f = backend.lib.nvcompBatchedCRC32Async
    P, Z, O, S = dev.ptr(ptrs), dev.ptr(sizes), dev.ptr(out), dev.stream()
    for args in ((None, Z, 1, O, S), (P, None, 1, O, S), (P, Z, 1, None, S), (None, None, 1, None, S)):
        assert f(*args) == NvcompStatus.ErrorInvalidValue
    dev.synchronize()
    assert (dev.download(out, 16).view(np.uint32) == GARBAGE).all(), "a rejected call launched something"
    assert f(None, None, 0, None, S) == NvcompStatus.Success
    assert f(P, Z, 0, O, S) == NvcompStatus.Success
    dev.synchronize()
    assert (dev.download(out, 16).view(np.uint32) == GARBAGE).all(), "num_chunks == 0 launched something"
    assert f(P, Z, 1, O, S) == NvcompStatus.Success
    dev.synchronize()
    assert dev.download(out, 16).view(np.uint32).tolist() == [want(data)] + [GARBAGE] * 3


def test_abi(backend):
    """Every function crc32.h declares is exported, and the header is in the umbrella."""
    declared = re.findall(r"nvcompStatus_t\s+(nvcomp\w+)\s*\(", open(HEADER).read())
    assert declared == ["nvcompBatchedCRC32Async"]
    for name in declared:
        assert hasattr(backend.lib, name), name
    assert '#include "nvcomp/crc32.h"' in open(os.path.join(REPO, "include", "nvcomp.h")).read()


# ---------------------------------------------------------------------------------------------------------------------
# the card only: the shapes the split exists for


def device_crc_of(gpu, tensor, sizes, offsets):
    """CRC of chunks [offsets[i], offsets[i] + sizes[i]) of a device tensor."""
    dev = gpu.dev
    base = dev.ptr(tensor)
    ptrs = [base + int(o) for o in offsets]
    rc, got, guard = call(gpu, ptrs, sizes)
    assert rc == NvcompStatus.Success and (guard == GARBAGE).all()
    return got


@pytest.mark.gpu
def test_headline_mix_65536_chunks(gpu):
    """65 536 x 64 KiB of the dataset mix (4 GiB on the card: 64 MiB of datasets.silesia_style, 64 times)."""
    torch = gpu.dev.torch
    unique = datasets.silesia_style(64 << 20, seed=11)
    per = [want(c) for c in datasets.split_chunks(unique)]
    dev_unique = gpu.dev.upload(unique)
    slab = dev_unique.repeat(64)
    n = 65536
    got = device_crc_of(gpu, slab, [65536] * n, np.arange(n, dtype=np.int64) * 65536)
    assert got.tolist() == per * 64
    del slab
    torch.cuda.empty_cache()


def random_device_bytes(torch, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


def host_crc_by_slices(t, n, slice_bytes=256 << 20):
    c = 0
    for lo in range(0, n, slice_bytes):
        c = zlib.crc32(t[lo: min(lo + slice_bytes, n)].cpu().numpy().tobytes(), c)
    return c & 0xFFFFFFFF


@pytest.mark.gpu
def test_one_1gib_chunk(gpu):
    torch = gpu.dev.torch
    n = 1 << 30
    t = random_device_bytes(torch, n, 21)
    assert device_crc_of(gpu, t, [n], [0]).tolist() == [host_crc_by_slices(t, n)]
    del t
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_one_chunk_past_4gib(gpu):
    """4 GiB + 12 345 bytes: past 2^31 and 2^32, split over the card (batch of one) and walked by one wave (a batch of
    65 536 whose other chunks are empty, so every chunk gets one wave: 1 GiB pieces chained, hlif/crc32.hip.h)."""
    torch = gpu.dev.torch
    n = (4 << 30) + 12345
    t = random_device_bytes(torch, n, 31)
    expect = host_crc_by_slices(t, n)
    assert device_crc_of(gpu, t, [n], [0]).tolist() == [expect]
    count = 65536
    dev = gpu.dev
    ptrs = [0] * count
    sizes = [0] * count
    ptrs[count // 2], sizes[count // 2] = dev.ptr(t), n
    rc, got, guard = call(gpu, ptrs, sizes)
    assert rc == NvcompStatus.Success and (guard == GARBAGE).all()
    assert int(got[count // 2]) == expect and not got[: count // 2].any() and not got[count // 2 + 1:].any()
    del t
    torch.cuda.empty_cache()
