"""CPU libzstd through ctypes: the producer of Zstd chunks and the checker of the HIP decoder (tests, fixtures,
scripts/bench_zstd.py). Test and measurement infrastructure only; the library's Zstd path is HIP and has no CPU
fall-back. ``load()`` returns None where no libzstd can be loaded."""
import ctypes as C
import ctypes.util
import os
import sys
from typing import Optional

import numpy as np

ZSTD_c_compressionLevel = 100
ZSTD_c_windowLog = 101
ZSTD_c_contentSizeFlag = 200
ZSTD_c_checksumFlag = 201
ZSTD_c_nbWorkers = 400
ZSTD_e_continue, ZSTD_e_flush, ZSTD_e_end = 0, 1, 2


class _InBuffer(C.Structure):
    _fields_ = [("src", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


class _OutBuffer(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


_lib = None
_tried = False


def load() -> Optional[C.CDLL]:
    """libzstd (1.4 or later), or None."""
    global _lib, _tried
    if _tried:
        return _lib
    _tried = True
    names = ["libzstd.so.1", ctypes.util.find_library("zstd"), os.path.join(sys.prefix, "lib", "libzstd.so.1")]
    for name in names:
        if not name:
            continue
        try:
            lib = C.CDLL(name)
        except OSError:
            continue
        sz, vp = C.c_size_t, C.c_void_p
        lib.ZSTD_versionString.restype = C.c_char_p
        lib.ZSTD_compressBound.restype, lib.ZSTD_compressBound.argtypes = sz, [sz]
        lib.ZSTD_isError.restype, lib.ZSTD_isError.argtypes = C.c_uint, [sz]
        lib.ZSTD_getErrorName.restype, lib.ZSTD_getErrorName.argtypes = C.c_char_p, [sz]
        lib.ZSTD_createCCtx.restype = vp
        lib.ZSTD_freeCCtx.argtypes = [vp]
        lib.ZSTD_CCtx_setParameter.restype, lib.ZSTD_CCtx_setParameter.argtypes = sz, [vp, C.c_int, C.c_int]
        lib.ZSTD_compress2.restype, lib.ZSTD_compress2.argtypes = sz, [vp, vp, sz, vp, sz]
        lib.ZSTD_compressStream2.restype = sz
        lib.ZSTD_compressStream2.argtypes = [vp, C.POINTER(_OutBuffer), C.POINTER(_InBuffer), C.c_int]
        lib.ZSTD_decompress.restype, lib.ZSTD_decompress.argtypes = sz, [vp, sz, vp, sz]
        _lib = lib
        break
    return _lib


def version() -> str:
    lib = load()
    return lib.ZSTD_versionString().decode() if lib else "absent"


def _check(lib, r: int, what: str) -> int:
    if lib.ZSTD_isError(r):
        raise RuntimeError(f"{what}: {lib.ZSTD_getErrorName(r).decode()}")
    return r


def _cctx(lib, level: int, checksum: bool, content_size: bool, window_log: Optional[int], workers: int = 0):
    cctx = lib.ZSTD_createCCtx()
    _check(lib, lib.ZSTD_CCtx_setParameter(cctx, ZSTD_c_compressionLevel, level), "level")
    _check(lib, lib.ZSTD_CCtx_setParameter(cctx, ZSTD_c_checksumFlag, int(checksum)), "checksumFlag")
    _check(lib, lib.ZSTD_CCtx_setParameter(cctx, ZSTD_c_contentSizeFlag, int(content_size)), "contentSizeFlag")
    if window_log is not None:
        _check(lib, lib.ZSTD_CCtx_setParameter(cctx, ZSTD_c_windowLog, window_log), "windowLog")
    if workers:
        _check(lib, lib.ZSTD_CCtx_setParameter(cctx, ZSTD_c_nbWorkers, workers), "nbWorkers")
    return cctx


def compress(data, level: int = 3, checksum: bool = False, content_size: bool = True,
             window_log: Optional[int] = None) -> np.ndarray:
    """One frame, ZSTD_compress2."""
    lib = load()
    src = np.ascontiguousarray(np.asarray(data).view(np.uint8).reshape(-1))
    cap = lib.ZSTD_compressBound(src.size)
    dst = np.empty(cap, dtype=np.uint8)
    cctx = _cctx(lib, level, checksum, content_size, window_log)
    try:
        n = _check(lib, lib.ZSTD_compress2(cctx, dst.ctypes.data, cap, src.ctypes.data, src.size), "ZSTD_compress2")
    finally:
        lib.ZSTD_freeCCtx(cctx)
    return dst[:n].copy()


def compress_streamed(data, level: int = 3, flush_every: int = 4096, checksum: bool = False,
                      window_log: Optional[int] = None) -> np.ndarray:
    """One frame written by ZSTD_compressStream2 with a ZSTD_e_flush every `flush_every` bytes: many blocks, whose
    sequence tables and Huffman trees the encoder reuses (repeat modes, treeless literals). No content size."""
    lib = load()
    src = np.ascontiguousarray(np.asarray(data).view(np.uint8).reshape(-1))
    cctx = _cctx(lib, level, checksum, True, window_log)
    out = bytearray()
    buf = np.empty(lib.ZSTD_compressBound(max(flush_every, 1)) + (1 << 17), dtype=np.uint8)
    try:
        pos = 0
        while True:
            piece = src[pos: pos + flush_every]
            last = pos + piece.size >= src.size
            inb = _InBuffer(piece.ctypes.data if piece.size else None, piece.size, 0)
            mode = ZSTD_e_end if last else ZSTD_e_flush
            while True:
                outb = _OutBuffer(buf.ctypes.data, buf.size, 0)
                rem = _check(lib, lib.ZSTD_compressStream2(cctx, C.byref(outb), C.byref(inb), mode), "compressStream2")
                out += buf[: outb.pos].tobytes()
                if rem == 0 and inb.pos == inb.size:
                    break
            pos += piece.size
            if last:
                break
    finally:
        lib.ZSTD_freeCCtx(cctx)
    return np.frombuffer(bytes(out), dtype=np.uint8)


def decompress(comp, capacity: int) -> np.ndarray:
    lib = load()
    src = np.ascontiguousarray(np.asarray(comp).view(np.uint8).reshape(-1))
    dst = np.empty(max(capacity, 1), dtype=np.uint8)
    n = _check(lib, lib.ZSTD_decompress(dst.ctypes.data, dst.size, src.ctypes.data, src.size), "ZSTD_decompress")
    return dst[:n].copy()


def skippable_frame(payload: bytes, nibble: int = 0) -> np.ndarray:
    """A skippable frame (RFC 8878 3.1.2): magic 0x184D2A5?, 4-byte size, payload."""
    head = (0x184D2A50 | (nibble & 15)).to_bytes(4, "little") + len(payload).to_bytes(4, "little")
    return np.frombuffer(head + payload, dtype=np.uint8)


def with_dictionary_id(frame: np.ndarray, dict_id: int = 0x1234ABCD) -> np.ndarray:
    """The same frame with a 4-byte Dictionary_ID inserted into its header (Dict_ID_flag = 3). libzstd writes no ID for
    raw-content dictionaries, so the header is edited by hand; the frame's content does not depend on it."""
    b = bytes(frame)
    fhd = b[4]
    assert fhd & 3 == 0, "frame already carries a Dictionary_ID"
    skip = 0 if fhd & 0x20 else 1  # the window descriptor sits between the descriptor and the ID
    head = b[:4] + bytes([fhd | 3]) + b[5: 5 + skip] + dict_id.to_bytes(4, "little")
    return np.frombuffer(head + b[5 + skip:], dtype=np.uint8)
