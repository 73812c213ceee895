"""Every codec at bench-sized batches on the card, every byte checked.

tests/test_headline_parity.py does this for the LZ4 and Snappy decoders; the other GPU tests run batches sized for the
emulator. Here Cascaded, Bitcomp, ANS and DEFLATE run in both directions, gzip decodes, and LZ4 and Snappy compress, over
four batch shapes (SHAPES below): the bench shape, a batch of more than 2^16 chunks and 2^32 bytes in one slab, 262 144
small ragged chunks (empty ones among them), and 24 chunks of the largest size the header allows. A batch is a small
unique set replicated on the device (tests/scale_batch.py); the CPU reference runs over the unique set only and every
replica is compared on the device.

References (never the code under test):
  * decode: the streams come from the CPU models (oracle.*_compress) / zlib level 9 (wbits -15 and 31); expected are the
    bytes the CPU decoder writes for the same stream, which must equal the originals before the card is touched;
    statuses all Success, sizes exact; then once more with statuses and sizes NULL.
  * compress, own formats (Cascaded, Bitcomp, ANS): sizes and bytes of every chunk of every replica equal the CPU model's.
  * compress, LZ4 / Snappy / DEFLATE (algo 0, 1, 2): EVERY replica is downloaded and decoded on the CPU (liblz4 /
    libsnappy where the shim is built, the oracle's decoders otherwise; zlib), every chunk must equal its original and
    every size stay within GetMaxOutputChunkSize. Replicas are NOT required to be byte-identical, for a reason the code
    shows: the match finders insert a window's positions into the per-wave hash table with ONE LDS store of all lanes
    (common/lz_match.hip.h: insert_lanes, common/lz_match_wide.hip.h: probe_step), lanes whose words share a slot store to
    the same address, and which lane's value stays is not defined by the ISA. Every outcome is a valid candidate (it is
    verified before use), so two runs over the same chunk may choose different matches and both streams are right. The
    emulator runs the lanes in a seeded random order and does show this: the same chunk at the same addresses compresses
    to different bytes from call to call -- which is also what looked like a dependence on placement there.
    Placement: the match finders address the input by position inside the chunk only (the LDS image holds byte p at
    p & 1023, the table holds positions mod 65 536); no address bit enters. All replicas are still laid out so that
    chunk i has the same address modulo 4 096 in every replica (scale_batch.PLACEMENT), for inputs and outputs alike.
  * Zstd is left out: tests/test_zstd.py::test_headline_mix_level3 already decodes 16 384 chunks of 64 KiB and compares
    every output byte with the originals.

Every temp buffer is filled with 0xFF before the first call and reused by the following calls as they left it; the
outputs are zeroed in between. In the bench and the ragged shape every output slot is followed by a 64-byte guard.

The host half of every case (data, CPU streams, "the CPU decoder restores the originals") also runs in the CPU tier.

Wall time: NOT MEASURED YET, neither `pytest tests -m gpu` without this file nor this file alone on the same MI355X box;
the replica counts are the ones the shapes are defined with, nothing has been reduced. (The CPU tier's share of this
file, the checker's tests and the 44 host halves, takes 46 s on 8 cores.) Whoever measures them writes both here; if
this file more than doubles the GPU tier, the replicas of "bench" and "ragged" go down, never the shapes or codecs.
"""
import zlib
from collections import OrderedDict
from dataclasses import dataclass
from functools import lru_cache
from typing import List, Optional, Tuple

import numpy as np
import pytest

import scale_batch as sb
from nvcomp_amd import datasets

CHUNK = 1 << 16
UNIQUE_BYTES = 64 << 20
LARGE = 1 << 24  # nvcomp{Cascaded,Bitcomp,ANS,LZ4,Snappy}CompressionMaxAllowedChunkSize
DEFLATE_LARGE = 1 << 16  # nvcompDeflateCompressionMaxAllowedChunkSize (the decoder has no limit: it takes LARGE)


@dataclass(frozen=True)
class Shape:
    unique: str    # which unique set: "64k" (1 024 x 64 KiB), "ragged" (4 096 x 0 .. 8 192 bytes), "large" (3 x the maximum)
    replicas: int
    guard: int


SHAPES = {
    "bench": Shape("64k", 16, sb.GUARD),      # 16 384 x 64 KiB, 1 GiB
    "past4g": Shape("64k", 68, 0),            # 69 632 x 64 KiB, 4.25 GiB in one slab
    "ragged": Shape("ragged", 64, sb.GUARD),  # 262 144 chunks of 0 .. 8 192 bytes
    "large": Shape("large", 8, 0),            # 24 chunks of the largest allowed size
}
RAGGED_UNIQUE, RAGGED_TOP = 4096, 8192


@dataclass(frozen=True)
class Variant:
    opts: Optional[tuple]       # the format options of the call
    sources: Tuple[str, ...]    # datasets, taken in turn 64 KiB block by block
    elem: int = 1               # element size: chunk sizes are whole elements
    align: int = 1              # alignment of chunk pointers on both sides

    @property
    def name(self) -> str:
        return f"{self.opts} on {'+'.join(self.sources)}"


INT, UCHAR, UINT, LONGLONG, ULONGLONG = 4, 1, 5, 6, 7
VARIANTS = {
    "Cascaded": [Variant((4096, INT, 2, 1, 1), ("silesia_style", "float_columns", "int32"), 4, 8),
                 Variant((16384, LONGLONG, 2, 1, 1), ("mortgage_col0_like", "silesia_style", "float_columns"), 8, 8)],
    # both algorithms; the 8-byte element types run the kernels that are bound to 6 workgroups per CU
    "Bitcomp": [Variant((0, UCHAR), ("silesia_style",), 1, 8),
                Variant((0, UINT), ("int32", "float_columns"), 4, 8),
                Variant((1, UINT), ("float_columns", "int32"), 4, 8),
                Variant((0, ULONGLONG), ("mortgage_col0_like",), 8, 8),
                Variant((1, ULONGLONG), ("mortgage_col0_like", "float_columns"), 8, 8)],
    "ANS": [Variant((0,), ("silesia_style",))],
    "Deflate": [Variant((0,), ("silesia_style",))],
    "Gzip": [Variant(None, ("silesia_style",))],
    "LZ4": [Variant((0,), ("silesia_style",))],
    "Snappy": [Variant((0,), ("silesia_style",))],
}
# DEFLATE compresses with each of its three settings
DEFLATE_COMPRESS = [Variant((a,), ("silesia_style",)) for a in (0, 1, 2)]

CASES = ([(c, "decode") for c in ("Cascaded", "Bitcomp", "ANS", "Deflate", "Gzip")]
         + [(c, "compress") for c in ("Cascaded", "Bitcomp", "ANS", "Deflate", "LZ4", "Snappy")])
PARAMS = [(c, d, s) for c, d in CASES for s in SHAPES]
IDS = [f"{c}-{d}-{s}" for c, d, s in PARAMS]


# ------------------------------------------------------------------------------------------------ data

@lru_cache(maxsize=None)
def _dataset(name: str) -> np.ndarray:
    gen = getattr(datasets, name) if hasattr(datasets, name) else datasets.CLASSES[name]
    data = gen(UNIQUE_BYTES, 0)
    data.setflags(write=False)
    return data


@lru_cache(maxsize=None)
def _stream(sources: Tuple[str, ...]) -> np.ndarray:
    """UNIQUE_BYTES taken from the sources in turn, 64 KiB block j from sources[j % len]."""
    if len(sources) == 1:
        return _dataset(sources[0])
    out = np.empty(UNIQUE_BYTES, dtype=np.uint8)
    for j in range(UNIQUE_BYTES // CHUNK):
        out[j * CHUNK: (j + 1) * CHUNK] = _dataset(sources[j % len(sources)])[j * CHUNK: (j + 1) * CHUNK]
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def _runs(width: int, kind: int, size: int) -> np.ndarray:
    """The runs_of kinds of tests/test_cascaded.py::test_later_passes_over_many_chunks, `size` bytes each: a run per
    element or two overflows the pools of Cascaded's first pass (the chunk is flagged for the later passes), long runs
    do not; kind 3 is noise."""
    rng = np.random.RandomState(770 + 10 * width + kind)
    lengths = {4: ([1, 1, 2], [40, 300], [1]), 8: ([1, 1, 1, 2], [300, 500], [1])}[width]
    if kind == 3:
        return datasets.noise(size, 1)
    dt = {4: np.uint32, 8: np.uint64}[width]
    k = size // width
    m = k // min(lengths[kind]) + 1  # values enough to fill k elements whatever lengths are drawn
    vals = np.cumsum(rng.randint(1, 9, size=m)).astype(np.uint64).astype(dt)
    return np.repeat(vals, rng.choice(lengths[kind], size=m))[:k].view(np.uint8)


def _flagged(i: int, n: int) -> bool:
    """Cascaded: which chunks of a unique set of n are of the runs_of kinds -- every third chunk in its first third, one
    in seven in the second, all in the last."""
    if i < n // 3:
        return i % 3 == 0
    if i < 2 * (n // 3):
        return i % 7 == 0
    return True


def large_size(codec: str, direction: str) -> int:
    return DEFLATE_LARGE if codec == "Deflate" and direction == "compress" else LARGE


def unique_chunks(codec: str, var: Variant, unique: str, large: int = LARGE) -> List[np.ndarray]:
    if unique == "64k":
        sizes = np.full(UNIQUE_BYTES // CHUNK, CHUNK, dtype=np.int64)
    elif unique == "ragged":
        sizes = sb.ragged_sizes(RAGGED_UNIQUE, RAGGED_TOP, var.elem, seed=5)
    else:
        sizes = np.full(3, large, dtype=np.int64)
    chunks = sb.cut(_stream(var.sources), sizes, var.elem)
    if codec == "Cascaded":
        top = int(sizes.max())
        for i in range(len(chunks)):
            if _flagged(i, len(chunks)):
                chunks[i] = _runs(var.elem, i % 4, top)[: chunks[i].size]
    return chunks


# ------------------------------------------------------------------------------------------------ the host half

def _deflate(wbits: int):
    def run(c: np.ndarray) -> np.ndarray:
        o = zlib.compressobj(9, zlib.DEFLATED, wbits)
        return np.frombuffer(o.compress(c.tobytes()) + o.flush(), dtype=np.uint8)
    return run


def _inflate(wbits: int):
    def run(c: np.ndarray) -> np.ndarray:
        return np.frombuffer(zlib.decompress(c.tobytes(), wbits), dtype=np.uint8)
    return run


def _first_difference(what: str, replica: int, got: List[np.ndarray], want: List[np.ndarray]) -> None:
    """Host-side comparison of decoded chunks with the originals; names the first difference."""
    for i, (g, w) in enumerate(zip(got, want)):
        if g.size != w.size:
            raise sb.Mismatch(what, "size", replica, i, None, f"decodes to {g.size} bytes, the original has {w.size}")
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise sb.Mismatch(what, "byte", replica, i, at, f"decodes to 0x{int(g[at]):02x}, the original holds 0x{int(w[at]):02x}")


def cpu_streams(oracle, codec: str, var: Variant, chunks: List[np.ndarray]) -> List[np.ndarray]:
    """The CPU producer of `codec` over the chunks, and the proof that its CPU decoder restores them."""
    if codec == "Cascaded":
        comp = sb.pool_map(lambda c: oracle.cascaded_compress(c, *var.opts), chunks)
        dec = oracle.CASCADED_DEC
    elif codec == "Bitcomp":
        comp = sb.pool_map(lambda c: oracle.bitcomp_compress(c, var.opts[0], var.elem), chunks)
        dec = oracle.BITCOMP_DEC
    elif codec == "ANS":
        comp = sb.pool_map(oracle.ans_compress, chunks)
        dec = oracle.ANS_DEC
    else:
        wbits = -15 if codec == "Deflate" else 31
        comp = sb.pool_map(_deflate(wbits), chunks)
        ref = sb.pool_map(_inflate(wbits), comp)
        _first_difference(f"{codec} {var.name}: the CPU decoder does not restore the originals (the producer is broken)", 0, ref, chunks)
        return comp
    _, ref, errs = oracle.batch_run(dec, comp, [c.size for c in chunks], threads=sb.pool_threads())
    assert errs == 0, f"{codec} {var.name}: the CPU decoder rejects {errs} of the CPU model's streams (the producer is broken)"
    _first_difference(f"{codec} {var.name}: the CPU decoder does not restore the originals (the producer is broken)", 0, ref, chunks)
    return comp


_host_cache: "OrderedDict[tuple, list]" = OrderedDict()


def host_half(oracle, codec: str, direction: str, shape: str) -> List[tuple]:
    """[(variant, chunks, streams or None)] of a case: everything that needs no card. `streams` are the CPU producer's
    (decode: the input; compress of the own formats: the expected output); the CPU decoder's output for them has been
    compared with the originals, so the expected decode output IS the list of chunks."""
    lz = direction == "compress" and codec in ("LZ4", "Snappy", "Deflate")
    key = (codec, lz, SHAPES[shape].unique, large_size(codec, direction))
    if key in _host_cache:
        _host_cache.move_to_end(key)
        return _host_cache[key]
    out = []
    for var in (DEFLATE_COMPRESS if lz and codec == "Deflate" else VARIANTS[codec]):
        chunks = unique_chunks(codec, var, SHAPES[shape].unique, large_size(codec, direction))
        assert all(c.size % var.elem == 0 for c in chunks)
        if SHAPES[shape].unique == "ragged":
            assert any(c.size == 0 for c in chunks) and max(c.size for c in chunks) == RAGGED_TOP
        out.append((var, chunks, None if lz else cpu_streams(oracle, codec, var, chunks)))
    _host_cache[key] = out
    while len(_host_cache) > 4:
        _host_cache.popitem(last=False)
    return out


@pytest.mark.parametrize("codec,direction,shape", PARAMS, ids=IDS)
def test_reference_restores_the_originals(oracle, codec, direction, shape):
    """The host half of every hardware case (the case with no replicas): the unique set is what the issue asks for and
    the CPU reference alone restores it."""
    for var, chunks, streams in host_half(oracle, codec, direction, shape):
        want = {"64k": UNIQUE_BYTES // CHUNK, "ragged": RAGGED_UNIQUE, "large": 3}[SHAPES[shape].unique]
        assert len(chunks) == want
        assert streams is None or (len(streams) == want and all(s.size > 0 for s in streams))
    if codec == "Cascaded":
        n = len(chunks)
        flags = [_flagged(i, n) for i in range(n)]
        assert 0 < sum(flags) < n or n == 3


# ------------------------------------------------------------------------------------------------ the card

def _device_batch(dev, slots: sb.Slots, slab, sizes: np.ndarray, replicas: int):
    from nvcomp_amd.batched import DeviceBatch

    ptrs = slots.pointers(dev.ptr(slab), replicas)
    tiled = np.tile(np.asarray(sizes, dtype=np.uint64), replicas)
    return DeviceBatch(slab, dev.upload(ptrs.view(np.uint8)), dev.upload(tiled.view(np.uint8)), None, tiled, len(tiled))


def _temp(dev, nbytes: int):
    """The caller's temp buffer as a caller may leave it: every byte 0xFF."""
    if not nbytes:
        return None
    t = dev.empty(nbytes)
    t.fill_(0xFF)
    return t


def _reset(slab, template, replicas: int) -> None:
    slab.view(replicas, template.numel()).copy_(template[None, :].expand(replicas, template.numel()))


def run_decode(gpu, codec_name: str, var: Variant, chunks, streams, shape: Shape, what: str) -> None:
    import torch
    from nvcomp_amd.batched import BatchedCodec

    dev, R, n_u = gpu.dev, shape.replicas, len(chunks)
    n = R * n_u
    in_slots = sb.pack_slots([s.size for s in streams], align=var.align)
    out_slots = sb.pack_slots([c.size for c in chunks], align=var.align, guard=shape.guard)
    in_slab = dev.upload(in_slots.image(streams)).repeat(R)
    template = dev.upload(out_slots.image())
    out_slab = template.repeat(R)
    exp = sb.expect(out_slots, chunks)
    image, mask, sizes = dev.upload(exp.image), dev.upload(exp.mask), torch.from_numpy(exp.sizes).to(out_slab.device)
    cb = _device_batch(dev, in_slots, in_slab, [s.size for s in streams], R)
    ob = _device_batch(dev, out_slots, out_slab, exp.sizes, R)
    codec = BatchedCodec(gpu.lib, dev, codec_name, var.opts)
    tb = codec.decompress_temp_size(n, max(int(exp.sizes.max()), 1))
    temp = _temp(dev, tb)
    # two checked calls on the same temp buffer (ticket counters, flag words), then one with statuses and sizes NULL
    for call, checked in (("first call", True), ("second call", True), ("call without statuses and sizes", False)):
        w = f"{what}, {call}"
        _reset(out_slab, template, R)
        actual = dev.upload(np.full(n, 0xDEADBEEF, dtype=np.uint64).view(np.uint8)) if checked else None
        statuses = dev.upload(np.full(n, -1, dtype=np.int32).view(np.uint8)) if checked else None
        assert codec.decompress_async(cb, ob, actual, statuses, temp, tb) == 0, w
        dev.synchronize()
        if checked:
            sb.check_statuses(statuses.view(torch.int32)[:n], R, n_u, w)
            sb.check_sizes(actual.view(torch.int64)[:n], sizes, R, w)
        sb.check_bytes(out_slab, image, mask, out_slots, R, w)
        if shape.guard:
            sb.check_guards(out_slab, out_slots, R, w)


def _cpu_decode(oracle, codec_name: str, streams, caps):
    if codec_name == "Deflate":
        return sb.pool_map(_inflate(-15), streams)
    use_ref = oracle.have_ref()
    dec = oracle.LZ4_DEC if codec_name == "LZ4" else oracle.SNAPPY_DEC
    _, outs, errs = oracle.batch_run(dec, streams, caps, threads=sb.pool_threads(), use_ref=use_ref)
    assert errs == 0, f"the CPU decoder rejects {errs} streams"
    return outs


def run_compress(gpu, oracle, codec_name: str, var: Variant, chunks, streams, shape: Shape, what: str) -> None:
    import torch
    from nvcomp_amd.batched import BatchedCodec

    dev, R, n_u = gpu.dev, shape.replicas, len(chunks)
    n = R * n_u
    codec = BatchedCodec(gpu.lib, dev, codec_name, var.opts)
    raw_sizes = np.array([c.size for c in chunks], dtype=np.int64)
    max_chunk = max(int(raw_sizes.max()), 1)
    max_out = codec.max_compressed_size(max_chunk)
    in_slots = sb.pack_slots(raw_sizes, align=var.align)
    out_slots = sb.pack_slots([max_out] * n_u, align=var.align, guard=shape.guard)
    in_slab = dev.upload(in_slots.image(chunks)).repeat(R)
    template = dev.upload(out_slots.image())
    out_slab = template.repeat(R)
    src = _device_batch(dev, in_slots, in_slab, raw_sizes, R)
    dst = _device_batch(dev, out_slots, out_slab, out_slots.cap, R)
    caps = dst.sizes.clone()
    if streams is not None:
        assert all(s.size <= max_out for s in streams), f"{what}: the CPU model's stream exceeds GetMaxOutputChunkSize"
        exp = sb.expect(out_slots, streams)
        image, mask, sizes = dev.upload(exp.image), dev.upload(exp.mask), torch.from_numpy(exp.sizes).to(out_slab.device)
    tb = codec.compress_temp_size(n, max_chunk)
    temp = _temp(dev, tb)
    for call in ("first call", "second call"):
        w = f"{what}, {call}"
        _reset(out_slab, template, R)
        dst.sizes.copy_(caps)
        assert codec.compress_async(src, dst, max_chunk, temp, tb) == 0, w
        dev.synchronize()
        got = dst.sizes.view(torch.int64)[:n]
        if shape.guard:
            sb.check_guards(out_slab, out_slots, R, w)
        if streams is not None:  # own format: the CPU model's bytes
            sb.check_sizes(got, sizes, R, w)
            sb.check_bytes(out_slab, image, mask, out_slots, R, w)
            continue
        # LZ4 / Snappy / DEFLATE: every replica through the CPU decoder (see the module docstring)
        host_sizes = got.cpu().numpy().reshape(R, n_u)
        over = np.argwhere((host_sizes > max_out) | ((host_sizes == 0) & (raw_sizes[None, :] > 0)))
        if len(over):
            r, c = (int(v) for v in over[0])
            raise sb.Mismatch(w, "size", r, c, None, f"reported {host_sizes[r, c]}, GetMaxOutputChunkSize is {max_out}")
        for r in range(R):
            host = out_slab[r * out_slots.stride: (r + 1) * out_slots.stride].cpu().numpy()
            comp = [host[int(o): int(o) + int(s)] for o, s in zip(out_slots.off, host_sizes[r])]
            _first_difference(f"{w}: the CPU decoder on the card's streams", r, _cpu_decode(oracle, codec_name, comp, raw_sizes), chunks)


@pytest.mark.gpu
@pytest.mark.parametrize("codec,direction,shape", PARAMS, ids=IDS)
def test_scale_parity(gpu, oracle, codec, direction, shape):
    for var, chunks, streams in host_half(oracle, codec, direction, shape):
        what = f"{codec} {direction} {shape} [{var.name}]"
        if direction == "decode":
            run_decode(gpu, codec, var, chunks, streams, SHAPES[shape], what)
        else:
            run_compress(gpu, oracle, codec, var, chunks, streams, SHAPES[shape], what)
        gpu.dev.torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the checker, checked

def _synthetic(replicas=5, n_u=7, guard=sb.GUARD):
    """A correct batch of replicas on the host: slots of uneven capacity, outputs shorter than their slots."""
    import torch

    rng = np.random.RandomState(3)
    caps = rng.randint(40, 400, size=n_u)
    outs = [rng.randint(0, 256, size=int(c) - 9).astype(np.uint8) for c in caps]
    slots = sb.pack_slots(caps, align=8, guard=guard)
    exp = sb.expect(slots, outs)
    slab = torch.from_numpy(slots.image(outs)).repeat(replicas)
    reported = torch.from_numpy(np.tile(exp.sizes, replicas))
    return slots, exp, slab, reported, outs


def _check_all(slots, exp, slab, reported, replicas):
    import torch

    sb.check_statuses(torch.zeros(replicas * slots.count, dtype=torch.int32), replicas, slots.count, "synthetic")
    sb.check_sizes(reported, torch.from_numpy(exp.sizes), replicas, "synthetic")
    sb.check_bytes(slab, torch.from_numpy(exp.image), torch.from_numpy(exp.mask), slots, replicas, "synthetic")
    sb.check_guards(slab, slots, replicas, "synthetic")


def test_checker_passes_a_correct_batch():
    slots, exp, slab, reported, _ = _synthetic()
    _check_all(slots, exp, slab, reported, 5)
    # bytes of a slot behind the expected output are the compressor's to leave as it likes
    slab[int(slots.off[2]) + int(exp.sizes[2])] ^= 0xFF
    _check_all(slots, exp, slab, reported, 5)


def test_checker_names_a_flipped_last_byte():
    slots, exp, slab, reported, outs = _synthetic()
    r, c = 4, slots.count - 1
    slab[r * slots.stride + int(slots.off[c]) + outs[c].size - 1] ^= 0x01
    with pytest.raises(sb.Mismatch) as e:
        _check_all(slots, exp, slab, reported, 5)
    assert (e.value.kind, e.value.replica, e.value.chunk, e.value.offset) == ("byte", r, c, outs[c].size - 1)
    assert f"replica {r}, chunk {c}, byte offset {outs[c].size - 1}" in str(e.value)


def test_checker_names_a_wrong_size():
    slots, exp, slab, reported, _ = _synthetic()
    r, c = 3, 2
    reported[r * slots.count + c] += 1
    with pytest.raises(sb.Mismatch) as e:
        _check_all(slots, exp, slab, reported, 5)
    assert (e.value.kind, e.value.replica, e.value.chunk) == ("size", r, c)
    assert f"replica {r}, chunk {c}" in str(e.value)


def test_checker_names_a_touched_guard_byte():
    slots, exp, slab, reported, _ = _synthetic()
    r, c, k = 4, slots.count - 1, sb.GUARD - 1
    slab[r * slots.stride + int(slots.off[c]) + int(slots.cap[c]) + k] = 0
    with pytest.raises(sb.Mismatch) as e:
        _check_all(slots, exp, slab, reported, 5)
    assert (e.value.kind, e.value.replica, e.value.chunk, e.value.offset) == ("guard", r, c, k)


def test_checker_names_a_failed_status():
    import torch

    st = torch.zeros(5 * 7, dtype=torch.int32)
    st[2 * 7 + 6] = 12
    with pytest.raises(sb.Mismatch) as e:
        sb.check_statuses(st, 5, 7, "synthetic")
    assert (e.value.kind, e.value.replica, e.value.chunk) == ("status", 2, 6)


def test_checker_refuses_to_compare_nothing():
    import torch

    slots, exp, slab, reported, _ = _synthetic()
    with pytest.raises(AssertionError):
        sb.check_bytes(slab, torch.from_numpy(exp.image), torch.zeros(slots.stride, dtype=torch.uint8), slots, 5, "synthetic")
    with pytest.raises(AssertionError):
        sb.check_sizes(reported[:0], torch.from_numpy(exp.sizes), 0, "synthetic")


def test_host_comparison_names_chunk_and_offset():
    a = [np.arange(10, dtype=np.uint8), np.arange(20, dtype=np.uint8)]
    b = [a[0].copy(), a[1].copy()]
    b[1][19] ^= 1
    with pytest.raises(sb.Mismatch) as e:
        _first_difference("synthetic", 6, b, a)
    assert (e.value.kind, e.value.replica, e.value.chunk, e.value.offset) == ("byte", 6, 1, 19)
