"""An independent model of the HLIF container (helper module of tests/test_hlif_managers.py; numpy + struct only).

Written from the layout documented in docs/HISTORY.md ("HLIF container (ours)") and at the top of
nvcomp_amd/csrc/hlif/manager.hip; nothing here calls the library. All fields little endian:

    [0, 64)  u32 magic 'NVAM' | u16 version = 1 | u16 format id | u64 uncompressed size | u32 chunk size |
             u32 chunk count N | 24 bytes of format options | u32 flags (bit 0: checksums) | u32 reserved = 0 |
             u64 total container size
    then     u64 comp_size[N] | u64 comp_offset[N + 1] | u32 crc_uncomp[N] | u32 crc_comp[N]
    then     the data area: chunk i at comp_offset[i], every chunk on an 8-byte boundary, zero padding behind it.
"""
import ctypes as C
import mmap
import struct
from types import SimpleNamespace

import numpy as np

MAGIC = 0x4D41564E  # 'NVAM'
HEADER = struct.Struct("<IHHQII24sIIQ")
assert HEADER.size == 64
FLAG_CHECKSUMS = 1
FORMAT_IDS = {"LZ4": 1, "Snappy": 2, "Cascaded": 3, "Bitcomp": 4, "ANS": 5, "Deflate": 6}
MAX_CHUNK = 1 << 24
# byte offsets of the header fields, for the corruption tests
OFF_MAGIC, OFF_VERSION, OFF_FORMAT, OFF_UNCOMP, OFF_CHUNK, OFF_COUNT, OFF_OPTS, OFF_FLAGS, OFF_TOTAL = 0, 4, 6, 8, 16, 20, 24, 48, 56


def round8(v):
    return (int(v) + 7) & ~7


def table_bytes(n):
    return round8(8 * n + 8 * (n + 1) + 4 * n + 4 * n)


def table_offsets(n):
    """Byte offsets, inside the container, of comp_size[], comp_offset[], crc_uncomp[], crc_comp[] and the data area."""
    sizes = 64
    offsets = sizes + 8 * n
    crc_u = offsets + 8 * (n + 1)
    crc_c = crc_u + 4 * n
    return SimpleNamespace(sizes=sizes, offsets=offsets, crc_uncomp=crc_u, crc_comp=crc_c, data=64 + table_bytes(n))


def opts_bytes(opts):
    """The 24 options bytes of the header: the format's options structure, zero filled."""
    raw = bytes(opts) if not isinstance(opts, (bytes, bytearray)) else bytes(opts)
    assert len(raw) <= 24
    return raw + bytes(24 - len(raw))


def parse(container, fmt=None, opts=None, checksums=None, zero_padding=True):
    """Take a container apart and assert every structural invariant. `fmt`, `opts` (the options the writer was opened
    with) and `checksums` (whether the writer's policy computes them) are compared when given."""
    buf = np.ascontiguousarray(container).view(np.uint8).reshape(-1)
    assert buf.size >= 64 + 8, "shorter than a header and the tables of an empty buffer"
    magic, version, fid, uncomp, chunk, n, raw_opts, flags, reserved, total = HEADER.unpack(buf[:64].tobytes())
    assert magic == MAGIC and version == 1
    assert fid in FORMAT_IDS.values()
    if fmt is not None:
        assert fid == FORMAT_IDS[fmt]
    assert 0 < chunk <= MAX_CHUNK
    assert n == -(-uncomp // chunk), "num_chunks == ceil(size / chunk)"
    assert reserved == 0 and flags & ~FLAG_CHECKSUMS == 0
    if opts is not None:
        assert raw_opts == opts_bytes(opts), "the options bytes are the writer's"
    if checksums is not None:
        assert bool(flags & FLAG_CHECKSUMS) == bool(checksums), "the flags are the writer's policy"
    t = table_offsets(n)
    assert buf.size >= t.data
    sizes = buf[t.sizes: t.sizes + 8 * n].view(np.uint64).copy()
    offsets = buf[t.offsets: t.offsets + 8 * (n + 1)].view(np.uint64).copy()
    crc_u = buf[t.crc_uncomp: t.crc_uncomp + 4 * n].view(np.uint32).copy()
    crc_c = buf[t.crc_comp: t.crc_comp + 4 * n].view(np.uint32).copy()
    assert int(offsets[0]) == 0
    for i in range(n):
        assert int(offsets[i + 1]) == int(offsets[i]) + round8(sizes[i]), f"offset[{i + 1}]"
    assert total == t.data + int(offsets[n]), "compressed_size == 64 + table_bytes(N) + offset[N]"
    assert buf.size >= total
    payloads, padding = [], []
    for i in range(n):
        lo = t.data + int(offsets[i])
        assert lo % 8 == 0
        payloads.append(buf[lo: lo + int(sizes[i])].copy())
        padding.append(buf[lo + int(sizes[i]): lo + round8(sizes[i])].copy())
    if zero_padding:
        assert all(not p.any() for p in padding), "the padding behind every chunk is zero"
    if not flags & FLAG_CHECKSUMS:
        assert not crc_u.any() and not crc_c.any(), "unused checksum slots are zero"
    return SimpleNamespace(format=fid, uncompressed_size=uncomp, chunk_size=chunk, num_chunks=n, opts=raw_opts, flags=flags,
                           compressed_size=total, comp_size=sizes, comp_offset=offsets, crc_uncomp=crc_u, crc_comp=crc_c,
                           payloads=payloads, padding=padding, tables=t)


def build(fmt, chunk_size, opts, chunks_compressed, uncompressed_size, crcs=None):
    """Write a container around chunks compressed elsewhere. `crcs` = (crc_uncomp[], crc_comp[]) or None."""
    n = len(chunks_compressed)
    assert n == -(-uncompressed_size // chunk_size)
    t = table_offsets(n)
    sizes = np.array([c.size for c in chunks_compressed], dtype=np.uint64)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    for i in range(n):
        offsets[i + 1] = int(offsets[i]) + round8(sizes[i])
    total = t.data + int(offsets[n])
    out = np.zeros(total, dtype=np.uint8)
    out[:64] = np.frombuffer(HEADER.pack(MAGIC, 1, FORMAT_IDS[fmt], uncompressed_size, chunk_size, n, opts_bytes(opts),
                                         FLAG_CHECKSUMS if crcs is not None else 0, 0, total), dtype=np.uint8)
    out[t.sizes: t.sizes + 8 * n] = sizes.view(np.uint8)
    out[t.offsets: t.offsets + 8 * (n + 1)] = offsets.view(np.uint8)
    if crcs is not None:
        out[t.crc_uncomp: t.crc_uncomp + 4 * n] = np.asarray(crcs[0], dtype=np.uint32).view(np.uint8)
        out[t.crc_comp: t.crc_comp + 4 * n] = np.asarray(crcs[1], dtype=np.uint32).view(np.uint8)
    for i, c in enumerate(chunks_compressed):
        lo = t.data + int(offsets[i])
        out[lo: lo + c.size] = np.asarray(c).view(np.uint8)
    return out


def put_u64(container, at, value):
    container[at: at + 8] = np.frombuffer(struct.pack("<Q", value & (2 ** 64 - 1)), dtype=np.uint8)


def put_u32(container, at, value):
    container[at: at + 4] = np.frombuffer(struct.pack("<I", value & (2 ** 32 - 1)), dtype=np.uint8)


def guarded_mapping(span_pages):
    """`span_pages` readable and writable pages followed by one PROT_NONE page (host memory, for the emulator, where the
    kernels are host code and a read past the end is a segfault). Returns (base address, span in bytes): the last
    usable byte is base + span - 1."""
    libc = C.CDLL(None, use_errno=True)
    libc.mmap.restype = C.c_void_p
    libc.mmap.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_long]
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    page = mmap.PAGESIZE
    span = span_pages * page
    base = libc.mmap(None, span + page, mmap.PROT_READ | mmap.PROT_WRITE, mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS, -1, 0)
    assert base not in (None, C.c_void_p(-1).value)
    assert libc.mprotect(base + span, page, 0) == 0  # PROT_NONE
    return base, span
