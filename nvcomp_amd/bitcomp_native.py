"""Host-side plumbing for the native Bitcomp API (include/nvcomp/native/bitcomp.h): a plan object over the C calls, used by
the tests and scripts/bench_bitcomp_native.py. No codec logic here: every method is one call into the library."""
from __future__ import annotations

import ctypes as C
import enum


class Result(enum.IntEnum):
    SUCCESS = 0
    INVALID_PARAMETER = -1
    INVALID_COMPRESSED_DATA = -2
    INVALID_ALIGNMENT = -3
    INVALID_INPUT_LENGTH = -4
    CUDA_KERNEL_LAUNCH_ERROR = -5
    CUDA_API_ERROR = -6
    UNKNOWN_ERROR = -7


class DataType(enum.IntEnum):
    UNSIGNED_8BIT = 0
    SIGNED_8BIT = 1
    UNSIGNED_16BIT = 2
    SIGNED_16BIT = 3
    UNSIGNED_32BIT = 4
    SIGNED_32BIT = 5
    UNSIGNED_64BIT = 6
    SIGNED_64BIT = 7
    FP16_DATA = 8
    FP32_DATA = 9
    FP64_DATA = 10


class Mode(enum.IntEnum):
    LOSSLESS = 0
    LOSSY_FP_TO_SIGNED = 1
    LOSSY_FP_TO_UNSIGNED = 2


class Algorithm(enum.IntEnum):
    DEFAULT = 0
    SPARSE = 1


ELEM_BYTES = {0: 1, 1: 1, 2: 2, 3: 2, 4: 4, 5: 4, 6: 8, 7: 8, 8: 2, 9: 4, 10: 8}
SEGMENT_BYTES = 65536
HEADER_BYTES = 32

FUNCTIONS = (
    "bitcompCreatePlan", "bitcompCreatePlanFromCompressedData", "bitcompDestroyPlan", "bitcompSetStream",
    "bitcompCompressLossless", "bitcompCompressLossy_fp16", "bitcompCompressLossy_fp32", "bitcompCompressLossy_fp64",
    "bitcompUncompress", "bitcompPartialUncompress", "bitcompMaxBuflen", "bitcompGetCompressedSize",
    "bitcompGetCompressedSizeAsync", "bitcompGetUncompressedSize", "bitcompGetUncompressedSizeFromHandle",
    "bitcompGetCompressedInfo",
)


class BitcompError(RuntimeError):
    def __init__(self, call: str, rc: int) -> None:
        self.rc = Result(rc) if rc in Result._value2member_map_ else rc
        super().__init__(f"{call} returned {self.rc!r}")


def _check(call: str, rc: int) -> None:
    if rc != 0:
        raise BitcompError(call, rc)


def max_buflen(lib, n_bytes: int) -> int:
    return int(lib.bitcompMaxBuflen(n_bytes))


def compressed_size(lib, ptr: int) -> int:
    """Synchronous; `ptr` is a device or host address of a compressed buffer whose writer has finished."""
    out = C.c_size_t(0)
    _check("bitcompGetCompressedSize", lib.bitcompGetCompressedSize(ptr, C.byref(out)))
    return out.value


def uncompressed_size(lib, ptr: int) -> int:
    out = C.c_size_t(0)
    _check("bitcompGetUncompressedSize", lib.bitcompGetUncompressedSize(ptr, C.byref(out)))
    return out.value


def compressed_info(lib, ptr: int, max_bytes: int):
    """(DataType, Mode, Algorithm) of a compressed buffer, reading at most max_bytes of it."""
    t, m, a = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    _check("bitcompGetCompressedInfo", lib.bitcompGetCompressedInfo(ptr, max_bytes, C.byref(t), C.byref(m), C.byref(a)))
    return DataType(t.value), Mode(m.value), Algorithm(a.value)


class Plan:
    """bitcompCreatePlan + the calls on the handle. `device` is the buffer provider the batched wrapper uses
    (nvcomp_amd.TorchDevice, or the tests' host stand-in): .empty(nbytes), .ptr(buf), .stream().
    Pointers are plain integers; the `*_into` methods take them, the others allocate their output."""

    def __init__(self, n_bytes: int, dtype: int, mode: int = Mode.LOSSLESS, algo: int = Algorithm.DEFAULT, device=None,
                 lib=None, from_compressed: int | None = None) -> None:
        if lib is None:
            from . import load_library

            lib = load_library()
        self.lib, self.dev = lib, device
        self.handle = C.c_void_p(None)
        if from_compressed is not None:
            _check("bitcompCreatePlanFromCompressedData",
                   lib.bitcompCreatePlanFromCompressedData(C.byref(self.handle), from_compressed))
            n = C.c_size_t(0)
            _check("bitcompGetUncompressedSizeFromHandle", lib.bitcompGetUncompressedSizeFromHandle(self.handle, C.byref(n)))
            self.n_bytes, self.dtype, self.mode, self.algo = n.value, None, None, None
        else:
            _check("bitcompCreatePlan", lib.bitcompCreatePlan(C.byref(self.handle), n_bytes, int(dtype), int(mode), int(algo)))
            self.n_bytes, self.dtype, self.mode, self.algo = int(n_bytes), DataType(dtype), Mode(mode), Algorithm(algo)
        stream = device.stream() if device is not None else None
        if stream:
            self.set_stream(stream)

    @classmethod
    def from_compressed(cls, ptr: int, device=None, lib=None) -> "Plan":
        return cls(0, 0, device=device, lib=lib, from_compressed=ptr)

    def set_stream(self, stream: int | None) -> None:
        _check("bitcompSetStream", self.lib.bitcompSetStream(self.handle, stream))

    def destroy(self) -> None:
        if self.handle:
            _check("bitcompDestroyPlan", self.lib.bitcompDestroyPlan(self.handle))
            self.handle = C.c_void_p(None)

    def __enter__(self) -> "Plan":
        return self

    def __exit__(self, *exc) -> None:
        self.destroy()

    def max_buflen(self) -> int:
        return max_buflen(self.lib, self.n_bytes)

    # ---- on raw pointers: one library call each, nothing else ----
    def compress_into(self, in_ptr: int, out_ptr: int) -> None:
        _check("bitcompCompressLossless", self.lib.bitcompCompressLossless(self.handle, in_ptr, out_ptr))

    def compress_lossy_into(self, in_ptr: int, out_ptr: int, delta: float) -> None:
        name = {DataType.FP16_DATA: "fp16", DataType.FP32_DATA: "fp32", DataType.FP64_DATA: "fp64"}.get(self.dtype)
        if name is None:
            raise BitcompError("bitcompCompressLossy", Result.INVALID_PARAMETER)
        fn = getattr(self.lib, "bitcompCompressLossy_" + name)
        _check(fn.__name__, fn(self.handle, in_ptr, out_ptr, delta))

    def uncompress_into(self, in_ptr: int, out_ptr: int) -> None:
        _check("bitcompUncompress", self.lib.bitcompUncompress(self.handle, in_ptr, out_ptr))

    def partial_uncompress_into(self, in_ptr: int, out_ptr: int, start: int, length: int) -> None:
        _check("bitcompPartialUncompress", self.lib.bitcompPartialUncompress(self.handle, in_ptr, out_ptr, start, length))

    # ---- on device buffers of `device` ----
    def compress(self, data):
        out = self.dev.empty(self.max_buflen())
        self.compress_into(self.dev.ptr(data), self.dev.ptr(out))
        return out

    def compress_lossy(self, data, delta: float):
        out = self.dev.empty(self.max_buflen())
        self.compress_lossy_into(self.dev.ptr(data), self.dev.ptr(out), delta)
        return out

    def uncompress(self, comp):
        out = self.dev.empty(self.n_bytes)
        self.uncompress_into(self.dev.ptr(comp), self.dev.ptr(out))
        return out

    def partial_uncompress(self, comp, start: int, length: int):
        out = self.dev.empty(length)
        self.partial_uncompress_into(self.dev.ptr(comp), self.dev.ptr(out), start, length)
        return out

    def compressed_size(self, comp) -> int:
        self.dev.synchronize()
        return compressed_size(self.lib, self.dev.ptr(comp))
