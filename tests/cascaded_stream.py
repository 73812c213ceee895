"""An independent reader and writer of the Cascaded container (helper module of tests/test_numeric_widths.py).

Written from the layout documented in docs/HISTORY.md section 2 ("Cascaded stream layout"); Python ints and numpy only,
nothing here calls the library or the CPU model. All fields little endian, everything 4-byte aligned:

    chunk  : u32 'CASC' | u8 type, num_RLEs, num_deltas, use_bp | u32 uncompressed bytes | u32 sub-chunk bytes
             | u32 num_sub | u32 sub_end[num_sub] (payload bytes up to the end of each sub-chunk) | payloads
    payload: u32 n_elems (or 0xffffffff + the raw bytes, padded to 4)
             u32 count[l] per RLE layer | streams runs[0 .. R-1], values
    stream : u32 bits | u64 min | ceil(count * bits / 32) x u32, element i = bits [i * bits, (i + 1) * bits) of the words
             read as one little-endian number; the value is (x + min) mod 2^(8 w).

A packed stream is handled as ONE Python integer: no word indices, no shifts by 32 - sh, no third word -- the arithmetic the
kernels and oracle/cascaded_ref.c share is not restated here.
"""
import struct
from types import SimpleNamespace

MAGIC = 0x43534143  # 'CASC'
RAW_MARKER = 0xFFFFFFFF
WIDTH = [1, 1, 2, 2, 4, 4, 8, 8]
HEADER_BYTES = 20


def _u32(b, pos):
    return struct.unpack_from("<I", b, pos)[0]


def header(chunk_bytes):
    b = bytes(chunk_bytes)
    magic, typ, num_rles, num_deltas, use_bp, n_bytes, sub, num_sub = struct.unpack_from("<IBBBBIII", b, 0)
    assert magic == MAGIC, hex(magic)
    assert typ < 8 and sub and sub % WIDTH[typ] == 0 and n_bytes % WIDTH[typ] == 0
    assert num_sub == (n_bytes + sub - 1) // sub
    sub_end = [_u32(b, HEADER_BYTES + 4 * i) for i in range(num_sub)]
    return SimpleNamespace(type=typ, width=WIDTH[typ], num_rles=num_rles, num_deltas=num_deltas, use_bp=use_bp, n_bytes=n_bytes,
                           sub_chunk_bytes=sub, num_sub=num_sub, sub_end=sub_end, payload=HEADER_BYTES + 4 * num_sub)


def _stream(b, pos, end, count):
    assert pos + 12 <= end, "stream header beyond the sub-chunk"
    bits = _u32(b, pos)
    minimum = struct.unpack_from("<Q", b, pos + 4)[0]
    n_words = (count * bits + 31) // 32
    assert pos + 12 + 4 * n_words <= end, "packed words beyond the sub-chunk"
    words = list(struct.unpack_from(f"<{n_words}I", b, pos + 12))
    return SimpleNamespace(bits=bits, min=minimum, count=count, words=words), pos + 12 + 4 * n_words


def parse(chunk_bytes):
    """One entry per sub-chunk: .raw is the raw bytes or None; a packed one has .n_elems, .count[l], .runs[l], .values
    (streams with .bits, .min, .count, .words) and .streams = runs + [values]. The chunk must be consumed exactly."""
    b = bytes(chunk_bytes)
    h = header(b)
    subs = []
    begin = 0
    for s, end in enumerate(h.sub_end):
        assert begin + 4 <= end and h.payload + end <= len(b), (s, begin, end, len(b))
        n_bytes = min(h.sub_chunk_bytes, h.n_bytes - s * h.sub_chunk_bytes)
        pos, lim = h.payload + begin, h.payload + end
        first = _u32(b, pos)
        if first == RAW_MARKER:
            assert end - begin == 4 + (n_bytes + 3) // 4 * 4, "raw sub-chunk: marker + bytes padded to 4"
            subs.append(SimpleNamespace(raw=b[pos + 4: pos + 4 + n_bytes], n_elems=n_bytes // h.width, bytes=end - begin))
        else:
            assert first == n_bytes // h.width, (s, first, n_bytes)
            count = [_u32(b, pos + 4 + 4 * l) for l in range(h.num_rles)]
            pos += 4 + 4 * h.num_rles
            runs = []
            for l in range(h.num_rles):
                st, pos = _stream(b, pos, lim, count[l])
                runs.append(st)
            values, pos = _stream(b, pos, lim, count[-1] if count else first)
            assert pos == lim, "sub-chunk longer than its streams"
            subs.append(SimpleNamespace(raw=None, n_elems=first, count=count, runs=runs, values=values, streams=runs + [values],
                                        bytes=end - begin))
        begin = end
    assert h.payload + begin == len(b), "bytes behind the last sub-chunk"
    return subs


def unpack(stream, w):
    """The values of a stream as Python ints: (x + min) mod 2^(8 w)."""
    big = 0
    for k, word in enumerate(stream.words):
        big |= word << (32 * k)
    mask = (1 << stream.bits) - 1
    mod = 1 << (8 * w)
    return [(((big >> (i * stream.bits)) & mask) + stream.min) % mod for i in range(stream.count)]


def elements(raw, w):
    """The w-byte little-endian elements of a byte string as Python ints."""
    raw = bytes(raw)
    return [int.from_bytes(raw[i: i + w], "little") for i in range(0, len(raw), w)]


def to_bytes(values, w):
    return b"".join((v % (1 << (8 * w))).to_bytes(w, "little") for v in values)


def write_plain(values, typ, bits, minimum, sub_chunk_bytes, high=0):
    """A chunk with num_RLEs = num_deltas = 0, use_bp = 1 whose every sub-chunk is packed and whose value streams have
    exactly the given `bits` and `minimum` (a u64; it may carry bits above the element width). `values` are the elements
    as Python ints. `bits` need not be minimal but must hold every (v - minimum) mod 2^(8 w); where it exceeds the
    element width, `high` is OR-ed into the bits of every x above the element width (the decoder must drop them)."""
    w = WIDTH[typ]
    mod = 1 << (8 * w)
    assert 0 <= minimum < (1 << 64) and sub_chunk_bytes % w == 0 and sub_chunk_bytes
    per = sub_chunk_bytes // w
    n_bytes = len(values) * w
    num_sub = (n_bytes + sub_chunk_bytes - 1) // sub_chunk_bytes
    payload = b""
    table = []
    for s in range(num_sub):
        vals = values[s * per: (s + 1) * per]
        big = 0
        for i, v in enumerate(vals):
            x = (v - minimum) % mod
            assert bits >= 8 * w or x < (1 << bits), (v, minimum, bits)
            x = (x | ((high << (8 * w)) if bits > 8 * w else 0)) & ((1 << bits) - 1)
            big |= x << (i * bits)
        n_words = (len(vals) * bits + 31) // 32
        payload += struct.pack("<IIQ", len(vals), bits, minimum) + big.to_bytes(4 * n_words, "little")
        table.append(len(payload))
    head = struct.pack("<IBBBBIII", MAGIC, typ, 0, 0, 1, n_bytes, sub_chunk_bytes, num_sub)
    return head + struct.pack(f"<{num_sub}I", *table) + payload
