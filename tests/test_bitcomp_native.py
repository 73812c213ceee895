"""The native Bitcomp API (include/nvcomp/native/bitcomp.h): plans over one buffer of any length, lossless and lossy
(error-bounded) compression, partial decompression, self-describing buffers. The behavioural tests run on the emulator
and on the MI355X through the same C ABI; the lossy results are compared bit for bit with a numpy model of the
quantisation the header defines."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import nvcomp_amd
from nvcomp_amd import _lib, datasets
from nvcomp_amd import bitcomp_native as bn
from nvcomp_amd.bitcomp_native import Algorithm, DataType, Mode, Plan, Result

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = bn.SEGMENT_BYTES
GUARD = 64  # bytes of 0xA5 in front of and behind every output; a multiple of 8 keeps the alignment

INT_TYPES = [DataType.UNSIGNED_8BIT, DataType.SIGNED_8BIT, DataType.UNSIGNED_16BIT, DataType.SIGNED_16BIT,
             DataType.UNSIGNED_32BIT, DataType.SIGNED_32BIT, DataType.UNSIGNED_64BIT, DataType.SIGNED_64BIT]
FP_TYPES = [DataType.FP16_DATA, DataType.FP32_DATA, DataType.FP64_DATA]
FP_NUMPY = {DataType.FP16_DATA: np.float16, DataType.FP32_DATA: np.float32, DataType.FP64_DATA: np.float64}
DATA_CLASSES = {"float_columns": datasets.float_columns, "int32_column": datasets.int32_column, "zeros": datasets.zeros,
                "noise": datasets.noise}


def guarded(dev, nbytes):
    """A device buffer of GUARD + nbytes + GUARD bytes of 0xA5; returns (buffer, address of the middle part)."""
    buf = dev.upload(np.full(nbytes + 2 * GUARD, 0xA5, dtype=np.uint8))
    return buf, dev.ptr(buf) + GUARD


def read_guarded(dev, buf, nbytes, what=""):
    dev.synchronize()
    host = dev.download(buf, nbytes + 2 * GUARD)
    assert (host[:GUARD] == 0xA5).all(), f"{what}: bytes in front of the output were written"
    assert (host[GUARD + nbytes:] == 0xA5).all(), f"{what}: bytes behind the output were written"
    return host[GUARD: GUARD + nbytes].copy()


def compress(backend, plan, data, delta=None):
    """Compress `data` (host bytes) into a guarded buffer of bitcompMaxBuflen bytes: (device buffer, its address, host copy
    of the compressed bytes, compressed size). Checks that the reported size is the last byte written."""
    dev = backend.dev
    cap = plan.max_buflen()
    src = dev.upload(data) if data.size else dev.empty(8)
    comp, comp_ptr = guarded(dev, cap)
    if delta is None:
        plan.compress_into(dev.ptr(src), comp_ptr)
    else:
        plan.compress_lossy_into(dev.ptr(src), comp_ptr, delta)
    host = read_guarded(dev, comp, cap, "compress")
    size = bn.compressed_size(backend.lib, comp_ptr)
    assert 32 <= size <= cap == bn.max_buflen(backend.lib, data.size)
    written = np.flatnonzero(host != 0xA5)
    assert written.size and written[-1] < size, "the compressor wrote behind the size it reports"
    # the last byte of a stream is a payload or width byte and may by chance equal the fill; it cannot lie further back
    # than one dword row of the last block
    assert size - 1 - written[-1] < 260
    plan.keepalive = (src, comp)  # callers that keep only the address: the buffers live as long as the plan object
    return comp, comp_ptr, host[:size].copy(), size


def uncompress(backend, plan, comp_ptr, nbytes):
    out, out_ptr = guarded(backend.dev, nbytes)
    plan.uncompress_into(comp_ptr, out_ptr)
    return read_guarded(backend.dev, out, nbytes, "uncompress")


def sizes_for(elem):
    """0, one element, 1 000 elements, a segment minus / plus one element, 3 segments + 5 elements, 16 MiB + 4 bytes (for the
    8-byte types + 8: a plan holds whole elements)."""
    return [0, elem, 1000 * elem, SEG - elem, SEG + elem, 3 * SEG + 5 * elem, (16 << 20) + max(4, elem)]


# ---- 1. lossless round trip ----

@pytest.mark.parametrize("algo", [Algorithm.DEFAULT, Algorithm.SPARSE])
@pytest.mark.parametrize("dtype", INT_TYPES + FP_TYPES, ids=lambda t: t.name)
def test_lossless_roundtrip_exact(backend, dtype, algo):
    elem = bn.ELEM_BYTES[dtype]
    biggest = sizes_for(elem)[-1]
    sources = {name: gen(biggest, 3) for name, gen in DATA_CLASSES.items()}
    for n in sizes_for(elem):
        with Plan(n, dtype, Mode.LOSSLESS, algo, backend.dev, backend.lib) as plan:
            for name, src in sources.items():
                if n == biggest and name != "float_columns" and backend.name == "emu" and dtype not in (
                        DataType.UNSIGNED_32BIT, DataType.FP64_DATA, DataType.UNSIGNED_8BIT):
                    # the emulator runs a lane at a time: every class at 16 MiB for one type of each loop shape (1-, 4- and
                    # 8-byte elements; 2-byte elements share the 1-byte code), one class for the others; the card runs all
                    continue
                data = np.ascontiguousarray(src[:n]).view(np.uint8)
                _, comp_ptr, _, size = compress(backend, plan, data)
                assert size <= bn.max_buflen(backend.lib, n), f"{name}, {n} bytes: {size} exceeds the bound"
                out = uncompress(backend, plan, comp_ptr, n)
                assert np.array_equal(out, data), f"{name}, {n} bytes"
                assert bn.uncompressed_size(backend.lib, comp_ptr) == n


def test_compression_ratio_of_the_classes(backend):
    """zeros collapse, the columns compress, noise stays below the bound"""
    n = 4 * SEG
    sizes = {}
    for name, gen in DATA_CLASSES.items():
        with Plan(n, DataType.UNSIGNED_32BIT, device=backend.dev, lib=backend.lib) as plan:
            sizes[name] = compress(backend, plan, gen(n, 1))[3]
    assert sizes["zeros"] < 400 and sizes["int32_column"] < n / 2 and sizes["float_columns"] < n
    assert n < sizes["noise"] <= bn.max_buflen(backend.lib, n)


# ---- 2. lossy: bit-exact against numpy ----

def int_dtype(dtype, signed):
    bits = 8 * bn.ELEM_BYTES[dtype]
    return np.dtype(f"{'int' if signed else 'uint'}{bits}")


def model_q(x, delta, dtype, signed):
    """q = rint(x / delta) in fp32 (fp16, fp32 data; fp16 widened exactly) or fp64, saturated to the integer of the
    element's width, NaN -> 0. Returns (q as that integer type, mask of the elements that did not saturate)."""
    work = np.float64 if dtype == DataType.FP64_DATA else np.float32
    it = int_dtype(dtype, signed)
    info = np.iinfo(it)
    with np.errstate(all="ignore"):
        q = np.rint(x.astype(work) / work(delta))
    lo_f = work(info.min)                       # exact: 0 or -2^(w-1)
    hi_f = work(info.max)                       # 32767 / 65535 exact; 2^31 - 1 and above round up to the power of two
    nan = np.isnan(q)
    high = ~nan & (q >= hi_f)
    low = ~nan & (q <= lo_f)
    inside = ~(nan | high | low)
    out = np.zeros(x.shape, dtype=it)
    out[high] = info.max
    out[low] = info.min
    out[inside] = q[inside].astype(it)
    return out, inside


def model_decode(q, delta, dtype):
    work = np.float64 if dtype == DataType.FP64_DATA else np.float32
    with np.errstate(all="ignore"):
        return (q.astype(work) * work(delta)).astype(FP_NUMPY[dtype])


def lossy_inputs(dtype, delta, signed, n=3 * SEG // 8 + 37):
    """Random values around the integer range's scale, plus every special case the header speaks of."""
    ft = FP_NUMPY[dtype]
    work = np.float64 if dtype == DataType.FP64_DATA else np.float32
    rng = np.random.RandomState(int(delta * 1000) % 1000 + 8 * bn.ELEM_BYTES[dtype] + signed)
    fmax = float(np.finfo(ft).max)
    with np.errstate(all="ignore"):
        x = (rng.standard_normal(n) * min(1000 * delta, fmax / 8)).astype(ft)
        x[::7] = (rng.standard_normal(x[::7].size) * min(delta, fmax / 8)).astype(ft)
        k = rng.randint(-3000, 3000, size=256)
        halves = ((k + 0.5) * work(delta)).astype(ft)                   # quotients exactly on .5 (where representable)
        tiny = np.finfo(ft).tiny
        sub = np.array([tiny / 2, -tiny / 4, np.finfo(ft).smallest_subnormal], dtype=ft)
        info = np.iinfo(int_dtype(dtype, signed))
        sat = np.array([min(float(info.max) * delta * s, fmax) for s in (0.999, 1.0, 1.001, 2.0, 1e6)]
                       + [max(float(info.min) * delta * s, -fmax) for s in (0.999, 1.0, 1.001, 2.0)]
                       + [fmax, -fmax], dtype=np.float64).astype(ft)
        special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -delta, -0.4 * delta, 0.5 * delta, 1.5 * delta,
                            2.5 * delta, -0.5 * delta], dtype=np.float64).astype(ft)
    x[: halves.size] = halves
    tail = np.concatenate([sub, sat, special])
    x[-tail.size:] = tail
    return x


@pytest.mark.parametrize("delta", [2.0 ** -10, 1e-3, 0.37, 1000.0])
@pytest.mark.parametrize("mode", [Mode.LOSSY_FP_TO_SIGNED, Mode.LOSSY_FP_TO_UNSIGNED], ids=lambda m: m.name)
@pytest.mark.parametrize("dtype", FP_TYPES, ids=lambda t: t.name)
def test_lossy_matches_the_numpy_model_bit_for_bit(backend, dtype, mode, delta):
    signed = mode == Mode.LOSSY_FP_TO_SIGNED
    ft = FP_NUMPY[dtype]
    work = np.float64 if dtype == DataType.FP64_DATA else np.float32
    delta = float(work(delta))  # what the C call receives: a float for fp16 / fp32 data
    x = lossy_inputs(dtype, delta, signed)
    q, inside = model_q(x, delta, dtype, signed)
    want = model_decode(q, delta, dtype)
    for algo in (Algorithm.DEFAULT, Algorithm.SPARSE):
        with Plan(x.nbytes, dtype, mode, algo, backend.dev, backend.lib) as plan:
            _, comp_ptr, _, size = compress(backend, plan, x.view(np.uint8), delta)
            got = uncompress(backend, plan, comp_ptr, x.nbytes).view(ft)
        bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[x.itemsize]
        bad = np.flatnonzero(got.view(bits) != want.view(bits))
        assert bad.size == 0, (f"{bad.size} elements differ from the model, first: x={x[bad[0]]!r} got={got[bad[0]]!r} "
                               f"want={want[bad[0]]!r} q={q[bad[0]]}")
    # the property the header promises, on the finite elements that did not saturate
    ok = inside & np.isfinite(x) & np.isfinite(want)
    xe, we = x[ok].astype(np.longdouble), want[ok].astype(np.longdouble)
    ulp = np.spacing(np.abs(want[ok])).astype(np.longdouble)
    assert ok.sum() > x.size // 4  # (FP_TO_UNSIGNED: the negative half of the inputs saturates at 0)
    assert (np.abs(xe - we) <= np.longdouble(delta) / 2 + ulp).all()


# ---- 3. lossy pays ----

def test_lossy_streams_are_smaller_on_the_float_columns(backend):
    files = sorted(glob.glob(os.path.join(REPO, "tests", "golden", "ExampleFloatData_col*_float.bin")))
    assert len(files) == 3
    for f in files:
        x = np.fromfile(f, dtype=np.float32)
        with Plan(x.nbytes, DataType.FP32_DATA, device=backend.dev, lib=backend.lib) as plan:
            lossless = compress(backend, plan, x.view(np.uint8))[3]
        with Plan(x.nbytes, DataType.FP32_DATA, Mode.LOSSY_FP_TO_SIGNED, device=backend.dev, lib=backend.lib) as plan:
            fine = compress(backend, plan, x.view(np.uint8), 1e-3)[3]
            coarse = compress(backend, plan, x.view(np.uint8), 1e-1)[3]
        print(f"{os.path.basename(f)}: lossless {lossless}, delta 1e-3 {fine}, delta 1e-1 {coarse} bytes")
        assert coarse < fine < lossless


# ---- 4. partial uncompress ----

def emu_segments_decoded(backend):
    """The emulator's count of segments the decode kernel took up (LZ_STAT in api/bitcomp_native_api.hip; compiled out of
    the product). The emulator reports its counters as text on stderr: dumped into a file, read back."""
    import sys
    import tempfile

    lib = C.CDLL(os.path.join(REPO, "tests", "emu", "libnvcomp_emu.so"))
    sys.stderr.flush()
    with tempfile.TemporaryFile() as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            lib.emu_stats_dump(0)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read()
    m = re.search(rb"stat bitcomp_native_segments_decoded\s+(\d+)", text)
    return int(m.group(1)) if m else 0


@pytest.mark.parametrize("lossy", [False, True], ids=["lossless", "lossy"])
def test_partial_uncompress(backend, lossy):
    elem = 4
    n = 5 * SEG + 5 * elem
    rng = np.random.RandomState(5)
    if lossy:
        data = (rng.standard_normal(n // 4) * 50).astype(np.float32).view(np.uint8)
        plan = Plan(n, DataType.FP32_DATA, Mode.LOSSY_FP_TO_SIGNED, Algorithm.DEFAULT, backend.dev, backend.lib)
    else:
        data = datasets.int32_column(n, 2)
        plan = Plan(n, DataType.SIGNED_32BIT, Mode.LOSSLESS, Algorithm.DEFAULT, backend.dev, backend.lib)
    with plan:
        _, comp_ptr, _, _ = compress(backend, plan, data, 0.01 if lossy else None)
        full = uncompress(backend, plan, comp_ptr, n)
        ranges = [(0, 0), (0, n), (n - elem, elem), (SEG + 400, 1000), (2 * SEG - 8, 16), (SEG, SEG), (n, 0)]
        for _ in range(20):
            start = int(rng.randint(0, n // elem)) * elem
            length = int(rng.randint(0, (n - start) // elem + 1)) * elem
            ranges.append((start, min(length, int(rng.choice([length, 4096, 3 * SEG])))))
        for start, length in ranges:
            out, out_ptr = guarded(backend.dev, length)
            before = emu_segments_decoded(backend) if backend.name == "emu" else 0
            plan.partial_uncompress_into(comp_ptr, out_ptr, start, length)
            got = read_guarded(backend.dev, out, length, f"range ({start}, {length})")
            assert np.array_equal(got, full[start: start + length]), (start, length)
            if backend.name == "emu":
                overlapping = 0 if length == 0 else (start + length - 1) // SEG - start // SEG + 1
                assert emu_segments_decoded(backend) - before == overlapping, (start, length)


# ---- 5. self-description ----

@pytest.mark.parametrize("dtype,mode,algo,delta", [
    (DataType.SIGNED_16BIT, Mode.LOSSLESS, Algorithm.SPARSE, None),
    (DataType.UNSIGNED_64BIT, Mode.LOSSLESS, Algorithm.DEFAULT, None),
    (DataType.FP32_DATA, Mode.LOSSLESS, Algorithm.DEFAULT, None),
    (DataType.FP16_DATA, Mode.LOSSY_FP_TO_SIGNED, Algorithm.DEFAULT, 0.25),
    (DataType.FP32_DATA, Mode.LOSSY_FP_TO_UNSIGNED, Algorithm.SPARSE, 1e-3),
    (DataType.FP64_DATA, Mode.LOSSY_FP_TO_SIGNED, Algorithm.DEFAULT, 1e-6)])
def test_compressed_buffer_describes_itself(backend, dtype, mode, algo, delta):
    dev, lib = backend.dev, backend.lib
    n = 2 * SEG + 24
    rng = np.random.RandomState(9)
    if dtype in FP_NUMPY:
        data = np.abs(rng.standard_normal(n // bn.ELEM_BYTES[dtype]) * 30).astype(FP_NUMPY[dtype]).view(np.uint8)
    else:
        data = datasets.int32_column(n, 4)
    with Plan(n, dtype, mode, algo, dev, lib) as plan:
        comp, comp_ptr, host, size = compress(backend, plan, data, delta)
        want = uncompress(backend, plan, comp_ptr, n)
    host_copy = np.ascontiguousarray(host)  # the same bytes in host memory
    for ptr in (comp_ptr, host_copy.ctypes.data):
        assert bn.compressed_info(lib, ptr, size) == (dtype, mode, algo)
        assert bn.compressed_info(lib, ptr, 32) == (dtype, mode, algo)
        assert bn.uncompressed_size(lib, ptr) == n and bn.compressed_size(lib, ptr) == size
        with Plan.from_compressed(ptr, dev, lib) as reader:
            assert reader.n_bytes == n
            assert np.array_equal(uncompress(backend, reader, comp_ptr, n), want)
            with pytest.raises(bn.BitcompError) as e:  # a plan made from compressed data decompresses
                reader.compress_into(comp_ptr, comp_ptr) if delta is None else reader.compress_lossy_into(comp_ptr, comp_ptr, delta)
            assert e.value.rc == Result.INVALID_PARAMETER
    answer = dev.upload(np.full(1, 0xDEADBEEF, dtype=np.uint64))
    assert lib.bitcompGetCompressedSizeAsync(comp_ptr, dev.ptr(answer), dev.stream()) == 0
    dev.synchronize()
    assert int(dev.download(answer, 8).view(np.uint64)[0]) == size
    if delta is None:
        assert np.array_equal(want, data)


# ---- 6. errors ----

@pytest.fixture(scope="module")
def cpu_lib():
    """the built library, loaded plainly: the host-only entry points need no GPU"""
    if not os.path.exists(nvcomp_amd.LIB_PATH):
        nvcomp_amd.build_library()
    return _lib.declare(C.CDLL(nvcomp_amd.LIB_PATH))


def test_host_only_calls_work_without_gpu(cpu_lib):
    lib = cpu_lib
    slot = 65808  # 12 + 8 x (32 + 8192) + 4, rounded to 16: the largest chunk stream of 64 KiB (1-, 2- and 4-byte elements)
    assert lib.bitcompMaxBuflen(0) == 32 + 8
    assert lib.bitcompMaxBuflen(1) == 32 + 16 + slot
    assert lib.bitcompMaxBuflen(SEG) == 32 + 16 + slot
    assert lib.bitcompMaxBuflen(SEG + 1) == 32 + 24 + 2 * slot
    assert lib.bitcompMaxBuflen(5 << 32) == 32 + 8 * ((5 << 16) + 1) + (5 << 16) * slot  # above 4 GiB
    h = C.c_void_p(None)
    assert lib.bitcompCreatePlan(C.byref(h), 1001, DataType.UNSIGNED_32BIT, 0, 0) == Result.INVALID_INPUT_LENGTH
    assert lib.bitcompCreatePlan(C.byref(h), 1000, 11, 0, 0) == Result.INVALID_PARAMETER
    assert lib.bitcompCreatePlan(C.byref(h), 1000, DataType.FP32_DATA, 3, 0) == Result.INVALID_PARAMETER
    assert lib.bitcompCreatePlan(C.byref(h), 1000, DataType.FP32_DATA, 0, 2) == Result.INVALID_PARAMETER
    assert lib.bitcompCreatePlan(C.byref(h), 1000, DataType.SIGNED_32BIT, Mode.LOSSY_FP_TO_SIGNED, 0) == Result.INVALID_PARAMETER
    assert lib.bitcompCreatePlan(None, 1000, DataType.SIGNED_32BIT, 0, 0) == Result.INVALID_PARAMETER
    assert h.value is None
    assert lib.bitcompDestroyPlan(None) == Result.INVALID_PARAMETER
    # a header in host memory is read without a device; a short or foreign one is refused
    junk = np.zeros(64, dtype=np.uint8)
    out = C.c_size_t(0)
    assert lib.bitcompGetCompressedSize(junk.ctypes.data, C.byref(out)) == Result.INVALID_COMPRESSED_DATA
    assert lib.bitcompCreatePlanFromCompressedData(C.byref(h), junk.ctypes.data) == Result.INVALID_COMPRESSED_DATA


def rc_of(call, *args):
    try:
        call(*args)
    except bn.BitcompError as e:
        return e.rc
    return Result.SUCCESS


def test_argument_errors(backend):
    dev, lib = backend.dev, backend.lib
    n = 4096
    buf = dev.upload(np.zeros(n + 64, dtype=np.uint8))
    comp = dev.empty(bn.max_buflen(lib, n) + 64)
    p, c = dev.ptr(buf), dev.ptr(comp)
    assert p % 8 == 0 and c % 8 == 0
    with Plan(n, DataType.FP32_DATA, Mode.LOSSLESS, 0, dev, lib) as lossless, \
            Plan(n, DataType.FP32_DATA, Mode.LOSSY_FP_TO_SIGNED, 0, dev, lib) as lossy:
        assert rc_of(lossless.compress_lossy_into, p, c, 0.5) == Result.INVALID_PARAMETER
        assert rc_of(lossy.compress_into, p, c) == Result.INVALID_PARAMETER
        for fn in (lib.bitcompCompressLossy_fp16, lib.bitcompCompressLossy_fp64):  # the wrong width
            assert fn(lossy.handle, p, c, 0.5) == Result.INVALID_PARAMETER
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert rc_of(lossy.compress_lossy_into, p, c, bad) == Result.INVALID_PARAMETER
        assert rc_of(lossless.compress_into, p + 2, c) == Result.INVALID_ALIGNMENT
        assert rc_of(lossless.compress_into, p, c + 4) == Result.INVALID_ALIGNMENT
        assert rc_of(lossless.compress_into, p, c) == Result.SUCCESS
        dev.synchronize()
        assert rc_of(lossless.uncompress_into, c + 4, p) == Result.INVALID_ALIGNMENT
        assert rc_of(lossless.uncompress_into, c, p + 1) == Result.INVALID_ALIGNMENT
        assert rc_of(lossless.partial_uncompress_into, c, p, 2, 8) == Result.INVALID_INPUT_LENGTH
        assert rc_of(lossless.partial_uncompress_into, c, p, 8, 6) == Result.INVALID_INPUT_LENGTH
        assert rc_of(lossless.partial_uncompress_into, c, p, n - 8, 16) == Result.INVALID_PARAMETER
        assert rc_of(lossless.partial_uncompress_into, c, p, n + 4, 0) == Result.INVALID_PARAMETER
        assert rc_of(lossless.compress_into, 0, c) == Result.INVALID_PARAMETER
        assert rc_of(lossless.uncompress_into, c, 0) == Result.INVALID_PARAMETER
        # truncation is seen by the query that is told how many bytes there are
        t, m, a = C.c_int(), C.c_int(), C.c_int()
        for short in (0, 1, 31):
            assert lib.bitcompGetCompressedInfo(c, short, C.byref(t), C.byref(m), C.byref(a)) == Result.INVALID_COMPRESSED_DATA
        assert lib.bitcompGetCompressedInfo(c, 32, C.byref(t), C.byref(m), C.byref(a)) == Result.SUCCESS
    with pytest.raises(bn.BitcompError):
        Plan(n + 2, DataType.FP32_DATA, device=dev, lib=lib)
    dev.synchronize()


@pytest.mark.parametrize("lossy", [False, True], ids=["lossless", "lossy"])
def test_bit_flipped_buffers_stay_inside_their_bounds(backend, lossy):
    """32 seeded single-bit flips each in the header, the offset table and the payload. The buffer handed to the decoder is
    always an allocation of bitcompMaxBuflen(n_bytes) bytes, the bound the library reads within."""
    dev, lib = backend.dev, backend.lib
    n = 3 * SEG + 20
    rng = np.random.RandomState(17)
    if lossy:
        data = (rng.standard_normal(n // 4) * 20).astype(np.float32).view(np.uint8)
        plan = Plan(n, DataType.FP32_DATA, Mode.LOSSY_FP_TO_SIGNED, 0, dev, lib)
    else:
        data = datasets.float_columns(n, 6)
        plan = Plan(n, DataType.UNSIGNED_32BIT, Mode.LOSSLESS, 0, dev, lib)
    cap = bn.max_buflen(lib, n)
    with plan:
        _, _, good, size = compress(backend, plan, data, 0.05 if lossy else None)
        table_end = 32 + 8 * 5
        regions = {"header": (0, 32), "table": (32, table_end), "payload": (table_end, size)}
        for region, (lo, hi) in regions.items():
            for _ in range(32):
                bad = np.full(cap, 0x5A, dtype=np.uint8)
                bad[:size] = good
                at, bit = int(rng.randint(lo, hi)), int(rng.randint(0, 8))
                bad[at] ^= 1 << bit
                comp = dev.upload(bad)
                ptr = dev.ptr(comp)
                out = C.c_size_t(0)
                rc = lib.bitcompGetCompressedSize(ptr, C.byref(out))
                rc_host = lib.bitcompGetCompressedSize(bad.ctypes.data, C.byref(out))
                assert rc == rc_host and rc in (Result.SUCCESS, Result.INVALID_COMPRESSED_DATA), (region, at, bit, rc)
                if at < 4 or (at == 7) or (region == "header" and 8 <= at < 16):
                    # magic, segment size, n_bytes (any change leaves the bound the size was checked against)
                    assert rc == Result.INVALID_COMPRESSED_DATA or (8 <= at < 16 and rc == Result.SUCCESS), (at, bit)
                if at < 4:
                    h = C.c_void_p(None)
                    assert lib.bitcompCreatePlanFromCompressedData(C.byref(h), ptr) == Result.INVALID_COMPRESSED_DATA
                if region != "header":
                    assert rc == Result.SUCCESS
                got = uncompress(backend, plan, ptr, n)  # returns; the guards around the output are checked inside
                assert got.size == n


# ---- 7. the hot calls only enqueue ----

@pytest.mark.gpu
def test_compress_and_uncompress_inside_a_graph(gpu):
    import torch

    dev, lib = gpu.dev, gpu.lib
    n = 8 * SEG + 40
    x = (np.random.RandomState(3).standard_normal(n // 4) * 10).astype(np.float32)
    delta = float(np.float32(1e-2))
    q, _ = model_q(x, delta, DataType.FP32_DATA, True)
    want = model_decode(q, delta, DataType.FP32_DATA)
    src = dev.upload(x.view(np.uint8))
    comp = dev.empty(bn.max_buflen(lib, n))
    out = dev.upload(np.full(n, 0xA5, dtype=np.uint8))
    side = torch.cuda.Stream()
    with Plan(n, DataType.FP32_DATA, Mode.LOSSY_FP_TO_SIGNED, 0, dev, lib) as plan:
        plan.set_stream(side.cuda_stream)
        plan.compress_lossy_into(dev.ptr(src), dev.ptr(comp), delta)  # warm: code objects loaded outside the capture
        plan.uncompress_into(dev.ptr(comp), dev.ptr(out))
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                plan.compress_lossy_into(dev.ptr(src), dev.ptr(comp), delta)
                plan.uncompress_into(dev.ptr(comp), dev.ptr(out))
        for round_ in range(2):
            comp.fill_(0)
            out.fill_(0xA5)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            got = dev.download(out, n).view(np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"replay {round_}"
        del graph


# ---- 8. ABI ----

def declared():
    text = open(os.path.join(REPO, "include", "nvcomp", "native", "bitcomp.h")).read()
    text = text.split('extern "C" {')[1].split("#ifdef __cplusplus")[0]
    return sorted(set(re.findall(r"^(?:bitcompResult_t|size_t)\s+(bitcomp\w+)\s*\(", text, flags=re.M)))


def test_every_declared_function_is_exported(cpu_lib):
    names = declared()
    assert names == sorted(bn.FUNCTIONS) and len(names) == 16
    assert not [n for n in names if not hasattr(cpu_lib, n)]
    emu = os.path.join(REPO, "tests", "emu", "libnvcomp_emu.so")
    if os.path.exists(emu):
        lib = C.CDLL(emu)
        assert not [n for n in names if not hasattr(lib, n)]


def test_native_header_compiles_as_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "nvcomp/native/bitcomp.h"\n'
                   "int main(void){bitcompHandle_t h = 0; bitcompMode_t m = BITCOMP_LOSSY_FP_TO_SIGNED;\n"
                   " return (int)bitcompMaxBuflen(0) + (int)m + (h != 0);}\n")
    subprocess.run(["gcc", "-std=c99", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(REPO, "include"), "-I", "/opt/rocm/include",
                    "-c", str(src), "-o", str(tmp_path / "t.o")], check=True)
