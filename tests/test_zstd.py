"""Zstandard batched decoder (include/nvcomp/zstd.h) against CPU libzstd, the producer of the chunks Parquet / ORC /
Arrow readers hand to nvCOMP. Every test runs on the emulator (-m "not gpu") and on the MI355X (-m gpu) through the
`backend` fixture. Exact: every byte, every size, every status."""
import ctypes as C
import gzip
import hashlib
import json
import os
import re

import numpy as np
import pytest

from nvcomp_amd import datasets, zstd_cpu
from nvcomp_amd._lib import NvcompStatus, ZSTD_ENTRY_POINTS
from nvcomp_amd.batched import BatchedCodec, empty_batch, make_batch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
HEADER = os.path.join(REPO, "include", "nvcomp", "zstd.h")

needs_libzstd = pytest.mark.skipif(zstd_cpu.load() is None, reason="libzstd cannot be loaded")

LEVELS = (-5, 1, 3, 19)
CHUNK_SIZES = (1, 1000, 65536, 65536 + 4321)
GUARD = 64


def original(recipe):
    """The bytes a fixture recipe names (scripts/make_golden_zstd.py writes the recipes)."""
    kind = recipe["source"]
    if kind == "gz":
        raw = gzip.open(os.path.join(GOLDEN, recipe["file"])).read()
        return np.frombuffer(raw[recipe["offset"]: recipe["offset"] + recipe["size"]], dtype=np.uint8).copy()
    if kind == "dataset":
        return datasets.CLASSES[recipe["class"]](recipe["size"], recipe["seed"])
    if kind == "far":
        unit = np.zeros(recipe["period"], dtype=np.uint8)
        unit[: recipe["noise"]] = datasets.noise(recipe["noise"], recipe["seed"])
        return np.resize(unit, recipe["size"])
    if kind == "concat":
        return np.concatenate([original(r) for r in recipe["parts"]] or [np.zeros(0, np.uint8)])
    if kind == "hex":
        return np.frombuffer(bytes.fromhex(recipe["hex"]), dtype=np.uint8).copy()
    raise ValueError(kind)


def fixtures():
    manifest = json.load(open(os.path.join(GOLDEN, "zstd_manifest.json")))
    out = []
    for e in manifest["frames"]:
        data = original(e["recipe"])
        assert hashlib.sha256(data.tobytes()).hexdigest() == e["sha256"], e["file"]
        comp = np.fromfile(os.path.join(GOLDEN, e["file"]), dtype=np.uint8)
        out.append((e, data, comp))
    return out


def run(backend, comps, caps, actual=True, statuses=True, temp_chunks=None):
    """Decode with the `stride` layout: every output slot is followed by GUARD bytes of 0xA5 that must survive.
    Returns (outputs, actual sizes or None, statuses or None)."""
    dev = backend.dev
    codec = BatchedCodec(backend.lib, dev, "Zstd")
    n = len(comps)
    caps = [int(c) for c in caps]
    stride = max(caps + [0]) + GUARD
    comp = make_batch(dev, [np.asarray(c, dtype=np.uint8) for c in comps])
    out = empty_batch(dev, [stride] * n, stride=stride, fill=0xA5)
    out.sizes = dev.upload(np.asarray(caps, dtype=np.uint64).view(np.uint8))
    act = dev.upload(np.full(n, 0xDEADBEEF, dtype=np.uint64).view(np.uint8)) if actual else None
    st = dev.upload(np.full(n, -1, dtype=np.int32).view(np.uint8)) if statuses else None
    tb = codec.decompress_temp_size(temp_chunks or n, max(caps + [1]))
    temp = dev.empty(tb)
    rc = codec.decompress_async(comp, out, act, st, temp, tb)
    assert rc == NvcompStatus.Success
    dev.synchronize()
    host = dev.download(out.slab)
    outs = []
    for i, c in enumerate(caps):
        o = int(out.offsets[i])
        outs.append(host[o: o + c].copy())
        assert (host[o + c: o + stride] == 0xA5).all(), f"chunk {i}: decoder wrote past its output capacity"
    a = dev.download(act).view(np.uint64)[:n].copy() if actual else None
    s = dev.download(st).view(np.int32)[:n].copy() if statuses else None
    return outs, a, s


def check_exact(backend, chunks, comps, caps=None):
    caps = [max(c.size, 1) for c in chunks] if caps is None else caps
    outs, actual, status = run(backend, comps, caps)
    assert status.tolist() == [NvcompStatus.Success] * len(chunks), status
    assert actual.tolist() == [c.size for c in chunks]
    for i, (o, c) in enumerate(zip(outs, chunks)):
        assert np.array_equal(o[: c.size], c), f"chunk {i} differs"


# ---- a host-side frame walker: headers only, no entropy data ----

def _ncount(b, at, max_log):
    """RFC 8878 4.1.1: the normalized counts of an FSE table description; returns (counts, bytes)."""
    bits = int.from_bytes(bytes(b[at: at + 80]), "little")
    log = (bits & 15) + 5
    assert log <= max_log
    pos, remaining, threshold, nb, counts, prev0 = 4, (1 << log) + 1, 1 << log, log + 1, [], False
    while remaining > 1:
        if prev0:
            while (bits >> pos) & 0xFFFF == 0xFFFF:
                counts += [0] * 24
                pos += 16
            while (bits >> pos) & 3 == 3:
                counts += [0] * 3
                pos += 2
            counts += [0] * ((bits >> pos) & 3)
            pos += 2
        mx = (2 * threshold - 1) - remaining
        v = bits >> pos
        if v & (threshold - 1) < mx:
            count = v & (threshold - 1)
            pos += nb - 1
        else:
            count = v & (2 * threshold - 1)
            if count >= threshold:
                count -= mx
            pos += nb
        count -= 1
        remaining -= abs(count)
        counts.append(count)
        prev0 = count == 0
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    return counts, (pos + 7) // 8


def walk(comp):
    """What a chunk's headers say: a set of feature names and the largest offset code any table can produce."""
    b = bytes(comp)
    seen, max_of = set(), 0
    pos, frames = 0, 0
    while pos < len(b):
        magic = int.from_bytes(b[pos: pos + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            seen.add("frame:skippable")
            pos += 8 + int.from_bytes(b[pos + 4: pos + 8], "little")
            continue
        assert magic == 0xFD2FB528
        frames += 1
        fhd = b[pos + 4]
        fcs_flag, single, checksum, did = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
        fcs_bytes = [single, 2, 4, 8][fcs_flag]
        seen.add("frame:fcs_absent" if fcs_bytes == 0 else "frame:fcs")
        if checksum:
            seen.add("frame:checksum")
        if did:
            seen.add("frame:dict_id")
        pos += 5 + (0 if single else 1) + [0, 1, 2, 4][did] + fcs_bytes
        while True:
            bh = int.from_bytes(b[pos: pos + 3], "little")
            last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
            pos += 3
            seen.add("block:" + ["raw", "rle", "compressed"][btype])
            if btype == 2:
                p, end = pos, pos + bsize
                lt, sf = b[p] & 3, (b[p] >> 2) & 3
                seen.add("lit:" + ["raw", "rle", "compressed", "treeless"][lt])
                if lt <= 1:
                    hl = [1, 2, 1, 3][sf]
                    regen = b[p] >> 3 if hl == 1 else (int.from_bytes(b[p: p + hl], "little") >> 4)
                    p += hl + (regen if lt == 0 else 1)
                else:
                    seen.add("streams:%d" % (1 if sf == 0 else 4))
                    hl, w = [(3, 10), (3, 10), (4, 14), (5, 18)][sf]
                    csize = (int.from_bytes(b[p: p + hl], "little") >> (4 + w)) & ((1 << w) - 1)
                    p += hl + csize
                n0 = b[p]
                nseq = n0 if n0 < 128 else ((n0 - 128) << 8) + b[p + 1] if n0 < 255 else b[p + 1] + (b[p + 2] << 8) + 0x7F00
                p += 1 if n0 < 128 else 2 if n0 < 255 else 3
                if nseq:
                    modes = b[p]
                    p += 1
                    for name, shift, max_log in (("LL", 6, 9), ("OF", 4, 8), ("ML", 2, 9)):
                        mode = (modes >> shift) & 3
                        seen.add(f"seq:{name}:" + ["predefined", "rle", "fse", "repeat"][mode])
                        if mode == 1:
                            if name == "OF":
                                max_of = max(max_of, b[p])
                            p += 1
                        elif mode == 2:
                            counts, used = _ncount(b, p, max_log)
                            if name == "OF":
                                max_of = max(max_of, max(i for i, c in enumerate(counts) if c != 0))
                            p += used
                        elif mode == 0 and name == "OF":
                            max_of = max(max_of, 28)  # the predefined table can code any offset up to 2^28
                pos = end
            else:
                pos += 1 if btype == 1 else bsize
            if last:
                break
        pos += 4 if checksum else 0
    if frames > 1:
        seen.add("frame:several")
    return seen, max_of


def test_golden_fixtures_cover_the_format():
    """The committed frames hold every block, literal, stream and table shape the decoder has a path for."""
    seen, max_of = set(), 0
    for e, data, comp in fixtures():
        s, m = walk(comp)
        seen |= s
        if "frame:dict_id" not in s:
            max_of = max(max_of, m)
    want = {"block:raw", "block:rle", "block:compressed", "lit:raw", "lit:rle", "lit:compressed", "lit:treeless",
            "streams:1", "streams:4", "frame:fcs_absent", "frame:checksum", "frame:several", "frame:skippable"}
    want |= {f"seq:{t}:{m}" for t in ("LL", "OF", "ML") for m in ("predefined", "rle", "fse", "repeat")}
    assert want <= seen, sorted(want - seen)
    # an offset code of 17 or more: an offset above 65 535 (the far_wl* frames, FSE-described)
    far = [walk(c)[1] for e, d, c in fixtures() if e["file"].startswith("zstd_far")]
    assert max(far) >= 17, far


def test_golden_frames(backend):
    items = fixtures()
    comps = [c for e, d, c in items]
    caps = [max(d.size, 1) for e, d, c in items]
    outs, actual, status = run(backend, comps, caps)
    for (e, data, comp), o, a, s in zip(items, outs, actual, status):
        if e.get("dict_id"):
            assert s == NvcompStatus.ErrorNotSupported, e["file"]
            assert a == 0
            continue
        assert s == NvcompStatus.Success, (e["file"], s)
        assert a == data.size, e["file"]
        assert np.array_equal(o[: data.size], data), e["file"]


CLASS_NAMES = sorted(datasets.CLASSES)


@needs_libzstd
@pytest.mark.parametrize("level", LEVELS)
def test_against_libzstd(backend, level):
    """Every dataset class x chunk sizes 1 / 1 000 / 65 536 / 65 536 + 4 321 at this level, in one batch."""
    chunks = []
    for k, name in enumerate(CLASS_NAMES):
        for size in CHUNK_SIZES:
            chunks.append(datasets.CLASSES[name](size, 100 + k))
    comps = [zstd_cpu.compress(c, level) for c in chunks]
    for c, cc in zip(chunks, comps):
        assert np.array_equal(zstd_cpu.decompress(cc, c.size), c)
    check_exact(backend, chunks, comps)


@needs_libzstd
def test_streamed_and_concatenated(backend):
    """Multi-block frames (flushes: repeat modes, treeless literals) and concatenations of frames."""
    chunks, comps = [], []
    for k, (name, flush, level) in enumerate((("text", 1024, 3), ("table", 4096, 19), ("float_csv", 700, 1),
                                              ("lowcard", 8192, -5), ("int32", 3000, 9))):
        c = datasets.CLASSES[name](50000, 200 + k)
        chunks.append(c)
        comps.append(zstd_cpu.compress_streamed(c, level, flush, checksum=k % 2 == 0))
    a, b = datasets.text(30000, 300), datasets.table_rows(20000, 301)
    chunks.append(np.concatenate([a, b, a]))
    comps.append(np.concatenate([zstd_cpu.compress(a, 3), zstd_cpu.compress(b, 1, content_size=False),
                                 zstd_cpu.skippable_frame(b"x" * 100), zstd_cpu.compress(a, 19, checksum=True)]))
    check_exact(backend, chunks, comps)


def _mixed_batch(n, seed):
    rng = np.random.RandomState(seed)
    chunks = []
    for i in range(n):
        kind = i % 5
        size = 0 if kind == 0 else int(rng.randint(1, 3000))
        name = CLASS_NAMES[int(rng.randint(len(CLASS_NAMES)))]
        chunks.append(datasets.CLASSES[name](size, seed + i) if size else np.zeros(0, np.uint8))
    return chunks


@needs_libzstd
@pytest.mark.parametrize("n", [1, 7, 513])
def test_batch_shapes(backend, n):
    """Batches past the launch's resident waves (two on the emulator): the persistent loop's ticket tail is reached;
    0-byte frames mixed in."""
    chunks = _mixed_batch(n, n)
    comps = [zstd_cpu.compress(c, 1 + (i % 3)) for i, c in enumerate(chunks)]
    check_exact(backend, chunks, comps)


@pytest.mark.gpu
@needs_libzstd
def test_batch_of_4100(gpu):
    """More chunks than the card keeps waves resident (3 072): the ticket tail on the card."""
    chunks = _mixed_batch(4100, 4100)
    comps = [zstd_cpu.compress(c, 1 + (i % 3)) for i, c in enumerate(chunks)]
    check_exact(gpu, chunks, comps)


@needs_libzstd
def test_large_chunks(backend):
    """1 MiB chunks on the emulator; 16 MiB chunks with windowLog 24 and repeats megabytes back on the GPU."""
    if backend.name == "gpu":
        size, period, wl = 16 << 20, 3 << 20, 24
        n = 2
    else:
        size, period, wl = 1 << 20, 300 << 10, 20
        n = 1
    chunks = []
    for k in range(n):
        unit = np.zeros(period, dtype=np.uint8)
        unit[: 40000] = datasets.noise(40000, 400 + k)
        unit[period // 2: period // 2 + 30000] = datasets.text(30000, 401 + k)
        chunks.append(np.resize(unit, size))
    comps = [zstd_cpu.compress(c, 3, window_log=wl) for c in chunks]
    check_exact(backend, chunks, comps)


@needs_libzstd
def test_get_decompress_size(backend):
    a, b = datasets.text(5000, 1), datasets.table_rows(300, 2)
    comps = [zstd_cpu.compress(a, 3), zstd_cpu.compress(a, 3, content_size=False),
             np.concatenate([zstd_cpu.compress(a, 3), zstd_cpu.skippable_frame(b"abc"), zstd_cpu.compress(b, 1)]),
             np.concatenate([zstd_cpu.compress(a, 3), zstd_cpu.compress(b, 1, content_size=False)]),
             np.frombuffer(gzip.compress(a.tobytes()), dtype=np.uint8), np.zeros(3, np.uint8),
             zstd_cpu.compress(np.zeros(0, np.uint8), 3), zstd_cpu.compress(datasets.zeros(300, 0), 3)]
    sizes = BatchedCodec(backend.lib, backend.dev, "Zstd").get_decompress_size(comps)
    assert sizes.tolist() == [5000, 0, 5300, 0, 0, 0, 0, 300]


@needs_libzstd
def test_null_outputs(backend):
    chunks = [datasets.text(2000, 5), datasets.zeros(100, 0)]
    comps = [zstd_cpu.compress(c, 3) for c in chunks]
    outs, a, s = run(backend, comps, [c.size for c in chunks], actual=False, statuses=False)
    assert a is None and s is None
    assert all(np.array_equal(o, c) for o, c in zip(outs, chunks))


def test_host_queries_and_invalid_arguments(backend):
    lib = backend.lib
    out = C.c_size_t(0)
    assert lib.nvcompBatchedZstdDecompressGetTempSize(10, 65536, C.byref(out)) == NvcompStatus.Success
    assert out.value == 64 + 10 * 65536
    assert lib.nvcompBatchedZstdDecompressGetTempSize(100000, 65536, C.byref(out)) == NvcompStatus.Success
    big = out.value
    assert big == 64 + 3072 * 65536 and big < 4096 * 65536  # scales with the resident waves, not the batch
    assert lib.nvcompBatchedZstdDecompressGetTempSize(5, 1 << 24, C.byref(out)) == NvcompStatus.Success
    assert out.value == 64 + 5 * (128 << 10)
    assert lib.nvcompBatchedZstdDecompressGetTempSizeEx(5, 1 << 20, C.byref(out), 1000) == NvcompStatus.Success
    assert out.value == 64 + 5 * 1008
    assert lib.nvcompBatchedZstdDecompressGetTempSize(5, 1000, None) == NvcompStatus.ErrorInvalidValue
    assert lib.nvcompBatchedZstdDecompressGetTempSize(5, (1 << 24) + 1, C.byref(out)) == NvcompStatus.ErrorInvalidValue
    dummy = backend.dev.upload(np.zeros(64, np.uint8))
    p = backend.dev.ptr(dummy)
    args = [p, p, p, None, 1, p, 4096, p, None, backend.dev.stream()]
    for i in (0, 1, 2, 5, 7):
        bad = list(args)
        bad[i] = None
        assert lib.nvcompBatchedZstdDecompressAsync(*bad) == NvcompStatus.ErrorInvalidValue, i
    small = list(args)
    small[6] = 16
    assert lib.nvcompBatchedZstdDecompressAsync(*small) == NvcompStatus.ErrorInvalidValue
    assert lib.nvcompBatchedZstdGetDecompressSizeAsync(None, p, p, 1, None) == NvcompStatus.ErrorInvalidValue
    assert lib.nvcompBatchedZstdDecompressAsync(None, None, None, None, 0, None, 0, None, None, None) == NvcompStatus.Success


def _flip(b, i, mask=0xFF):
    b = bytearray(b)
    b[i] ^= mask
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _set(b, i, v):
    b = bytearray(b)
    b[i] = v
    return np.frombuffer(bytes(b), dtype=np.uint8)


def _frame_parts(comp):
    """(frame header length, list of (block start, block header value)) of a single-frame chunk."""
    b = bytes(comp)
    fhd = b[4]
    single, did, fcs_flag = (fhd >> 5) & 1, fhd & 3, fhd >> 6
    pos = 5 + (0 if single else 1) + [0, 1, 2, 4][did] + [single, 2, 4, 8][fcs_flag]
    hdr, blocks = pos, []
    while True:
        bh = int.from_bytes(b[pos: pos + 3], "little")
        blocks.append((pos, bh))
        pos += 3 + (1 if (bh >> 1) & 3 == 1 else bh >> 3)
        if bh & 1:
            return hdr, blocks, pos


def _with_prefix(data, prefix, level=3):
    """A frame compressed against a prefix (ZSTD_CCtx_refPrefix): its offsets reach in front of the frame."""
    lib = zstd_cpu.load()
    lib.ZSTD_CCtx_refPrefix.restype, lib.ZSTD_CCtx_refPrefix.argtypes = C.c_size_t, [C.c_void_p, C.c_void_p, C.c_size_t]
    cctx = zstd_cpu._cctx(lib, level, False, True, None)
    src = np.ascontiguousarray(data)
    pre = np.ascontiguousarray(prefix)
    dst = np.empty(lib.ZSTD_compressBound(src.size), np.uint8)
    try:
        zstd_cpu._check(lib, lib.ZSTD_CCtx_refPrefix(cctx, pre.ctypes.data, pre.size), "refPrefix")
        n = zstd_cpu._check(lib, lib.ZSTD_compress2(cctx, dst.ctypes.data, dst.size, src.ctypes.data, src.size), "compress2")
    finally:
        lib.ZSTD_freeCCtx(cctx)
    return dst[:n].copy()


@needs_libzstd
def test_corrupt_input(backend):
    """Every malformed chunk gets a non-Success status, every call returns, no byte behind an output slot changes."""
    data = datasets.table_rows(20000, 9)
    good = zstd_cpu.compress(data, 3, checksum=True)
    hdr, blocks, end = _frame_parts(good)
    assert any((bh >> 1) & 3 == 2 for _, bh in blocks)
    cstart, cbh = next((p, bh) for p, bh in blocks if (bh >> 1) & 3 == 2)
    lit = cstart + 3
    bad = {
        "empty": np.zeros(0, np.uint8),
        "bad_magic": _flip(good, 0, 0x01),
        "reserved_bit": _flip(good, 4, 0x08),
        "block_type_3": _set(good, cstart, good[cstart] | 0x06),
        "block_too_long": _set(_set(good, cstart + 2, 0xFF), cstart + 1, 0xFF),
        "huffman_header": _set(good, lit + 3 if (good[lit] & 3) == 2 else lit, 0x7F),
        "stream_padding": _set(good, cstart + 3 + (cbh >> 3) - 1, 0),
        "seq_modes_reserved": None,
        "trailing_garbage": np.concatenate([good, np.frombuffer(b"\x01\x02", np.uint8)]),
        "no_checksum": good[:-4],
        "offset_before_frame": _with_prefix(data[:5000], data[5000:]),
    }
    # the sequences' mode byte: walk the literals section of the first compressed block
    b = bytes(good)
    lt, sf = b[lit] & 3, (b[lit] >> 2) & 3
    if lt >= 2:
        hl, w = [(3, 10), (3, 10), (4, 14), (5, 18)][sf]
        p = lit + hl + ((int.from_bytes(b[lit: lit + hl], "little") >> (4 + w)) & ((1 << w) - 1))
    else:
        hl = [1, 2, 1, 3][sf]
        p = lit + hl + ((b[lit] >> 3 if hl == 1 else int.from_bytes(b[lit: lit + hl], "little") >> 4) if lt == 0 else 1)
    p += 1 if b[p] < 128 else 2 if b[p] < 255 else 3
    bad["seq_modes_reserved"] = _set(good, p, b[p] | 1)
    # truncations at every header boundary and inside every section
    for cut in sorted({4, 5, hdr - 1, hdr, hdr + 2, lit, lit + 2, p, p + 1, end - 1, end + 2, good.size - 1}):
        bad[f"cut_{cut}"] = good[:cut]
    names = list(bad)
    comps = [bad[k] for k in names]
    caps = [data.size] * len(comps)
    names.append("capacity_one_short")
    comps.append(good)
    caps.append(data.size - 1)
    names.append("capacity_one_short_no_fcs")
    comps.append(zstd_cpu.compress(data, 3, content_size=False))
    caps.append(data.size - 1)
    outs, actual, status = run(backend, comps, caps)
    for k, s, a in zip(names, status, actual):
        assert s != NvcompStatus.Success, k
        assert a == 0, k
    # random flips anywhere: whatever the status, the call returns and stays inside its slots
    rng = np.random.RandomState(5)
    flips = [_flip(good, int(rng.randint(good.size)), int(rng.randint(1, 256))) for _ in range(24)]
    run(backend, flips, [data.size] * len(flips))


def test_abi(backend):
    """Every function zstd.h declares is exported; no Zstd compressor is."""
    declared = re.findall(r"nvcompStatus_t\s+(nvcompBatchedZstd\w+)\s*\(", open(HEADER).read())
    assert sorted(declared) == sorted("nvcompBatchedZstd" + n for n in ZSTD_ENTRY_POINTS)
    for name in declared:
        assert hasattr(backend.lib, name), name
    for name in ("CompressGetTempSize", "CompressGetMaxOutputChunkSize", "CompressAsync", "CompressGetTempSizeEx"):
        assert not hasattr(backend.lib, "nvcompBatchedZstd" + name), name
    assert "nvcompBatchedZstdOpts_t" not in open(HEADER).read()


@pytest.mark.gpu
@needs_libzstd
def test_headline_mix_level3(gpu):
    """16 384 chunks of 64 KiB of the dataset mix, libzstd level 3, decode bit-exact."""
    data = datasets.silesia_style(16384 * 65536, seed=3)
    chunks = datasets.split_chunks(data)
    comps = [zstd_cpu.compress(c, 3) for c in chunks]
    codec = BatchedCodec(gpu.lib, gpu.dev, "Zstd")
    outs, actual, status = codec.decompress(comps, [c.size for c in chunks])
    assert (status == NvcompStatus.Success).all()
    assert actual.tolist() == [c.size for c in chunks]
    assert all(np.array_equal(o, c) for o, c in zip(outs, chunks))
