"""A DEFLATE / gzip stream writer for tests, written from RFC 1951 and RFC 1952. Pure Python, no zlib.

The writer never chooses what matters: the caller says what goes on the wire (block kinds, the padding bits of a stored
block, every code length of a dynamic block, HLIT / HDIST / HCLEN, the code-length code and the run-length operations
that send the lengths, each symbol and, where it matters, which length symbol carries a length), and the writer says
what those bits mean: `Stream.out` is the plain expansion of the description, matches copied byte by byte. That
expansion is the reference of tests/test_deflate_format.py; test_writer_against_zlib there checks it against zlib.

    s = Stream()
    s.stored(b"abc", pad=0b101)
    s.dynamic([0x61, (258, 1, 284), 0x62], ll_lens={0x61: 1, 0x62: 2, 256: 3, 284: 3}, d_lens=[1], final=True)
    s.bytes(), s.out, s.trace

A symbol is a literal (an int below 256) or a pair (length, distance[, length symbol]); bytes stand for their literals.
The writer refuses what it cannot expand (a distance past the history, a symbol without a code, lengths sent by
operations that do not give them). `Stream(invalid="why")` is the exception: it is written as told, takes the raw items
("ll", symbol), ("pair", length symbol, extra value, distance symbol or None, extra value) and ("bits", value, n)
besides, ("bits", value, n) among the run-length operations too, and has no expansion (`out` is None).
"""
import random

# ---- the alphabets (RFC 1951 3.2.5) ----
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]        # symbols 257..285
DIST_EXTRA = [0] * 4 + [k for k in range(1, 14) for _ in (0, 1)]                   # symbols 0..29
LEN_BASE, DIST_BASE = [], []
_v = 3
for _k in LEN_EXTRA[:-1]:
    LEN_BASE.append(_v)
    _v += 1 << _k
LEN_BASE.append(258)
_v = 1
for _k in DIST_EXTRA:
    DIST_BASE.append(_v)
    _v += 1 << _k
assert LEN_BASE[284 - 257] == 227 and DIST_BASE[29] == 24577 and _v == 32769 and len(LEN_BASE) == 29 and len(DIST_BASE) == 30
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def length_symbol(length):
    """The symbol a compressor would use: the last one whose base is not above the length (258 is symbol 285)."""
    return 257 + max(i for i in range(29) if LEN_BASE[i] <= length)


def distance_symbol(distance):
    return max(i for i in range(30) if DIST_BASE[i] <= distance)


# ---- bits ----

class BitWriter:
    """LSB-first bit packing of RFC 1951; Huffman codes go in most significant bit first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, n, msb_first=False):
        value &= (1 << n) - 1
        if msb_first and n > 1:
            value = int(format(value, "0%db" % n)[::-1], 2)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self, fill=0):
        """To the next byte boundary; the padding bits are the low bits of `fill`, first bit first."""
        if self.n:
            self.put(fill, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def bit_length(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


# ---- canonical codes (RFC 1951 3.2.2) ----

def kraft(lengths, max_bits=15):
    """The code space the lengths take, in units of 2^-max_bits: 2^max_bits is a complete code."""
    return sum(1 << (max_bits - l) for l in lengths if l)


def canonical_codes(lengths, check=True):
    """{symbol: (code, length)} for the non-zero lengths; the code's first bit on the wire is its most significant."""
    lengths = list(lengths)
    top = max(lengths + [0])
    if check and kraft(lengths, max(top, 1)) > 1 << max(top, 1):
        raise ValueError("over-subscribed code lengths")
    count = [0] * (top + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, first = 0, [0] * (top + 2)
    for bits in range(1, top + 1):
        code = (code + count[bits - 1]) << 1
        first[bits] = code
    out = {}
    for sym, l in enumerate(lengths):
        if l:
            out[sym] = (first[l] & ((1 << l) - 1), l)
            first[l] += 1
    return out


def complete_lengths(lengths, pool, max_bits=15):
    """The lengths with unused symbols of `pool` (in that order) given lengths so that the code is complete. zlib
    refuses incomplete literal/length codes, so most test codes are completed this way. The filler lengths are the
    binary digits of what is left, longest first."""
    lengths = list(lengths)
    left = (1 << max_bits) - kraft(lengths, max_bits)
    if left < 0:
        raise ValueError("over-subscribed code lengths")
    want = [max_bits - b for b in range(max_bits + 1) if (left >> b) & 1]
    free = [s for s in pool if s < len(lengths) and lengths[s] == 0]
    if len(want) > len(free):
        raise ValueError("not enough unused symbols to complete the code")
    for s, l in zip(free, want):
        lengths[s] = l
    assert kraft(lengths, max_bits) == 1 << max_bits
    return lengths


def random_complete_lengths(r, n, max_bits=15, deep=False):
    """n code lengths of a complete code by random tree splitting (n >= 2); `deep` prefers splitting the deepest leaf."""
    leaves = [1, 1]
    while len(leaves) < n:
        can = [i for i, d in enumerate(leaves) if d < max_bits]
        i = max(can, key=lambda j: leaves[j]) if deep and r.random() < 0.7 else r.choice(can)
        leaves[i] += 1
        leaves.append(leaves[i])
    r.shuffle(leaves)
    return leaves


# ---- the run-length operations of a dynamic header (RFC 1951 3.2.7) ----

def expand_ops(ops):
    """The lengths a list of operations (symbol[, repeat]) sends; ValueError for a 16 in front of everything."""
    out = []
    for op in ops:
        sym = op[0]
        if sym < 16:
            out.append(sym)
        elif sym == 16:
            if not out:
                raise ValueError("16 with no previous length")
            out += [out[-1]] * op[1]
        else:
            out += [0] * op[1]
    return out


def greedy_ops(seq, forced=None, plain=False):
    """Operations for the lengths `seq`, longest repeat first; the caller hands HLIT + HDIST lengths as one sequence, so a
    repeat may run from the literal/length lengths into the distance lengths. forced = {index: (symbol, repeat)} puts
    that operation at that index; plain sends every other length one by one."""
    forced = forced or {}
    ops, i = [], 0
    while i < len(seq):
        if i in forced:
            op = forced[i]
            ops.append(op)
            i += op[1] if op[0] >= 16 else 1
            continue
        stop = min([j for j in forced if j > i] + [len(seq)])
        run = 1
        while i + run < stop and seq[i + run] == seq[i]:
            run += 1
        if plain:
            ops.append((seq[i],))
            i += 1
        elif seq[i] == 0 and run >= 3:
            n = min(run, 138)
            ops.append((18 if n >= 11 else 17, n))
            i += n
        elif seq[i] and i and seq[i - 1] == seq[i] and run >= 3:
            n = min(run, 6)
            ops.append((16, n))
            i += n
        else:
            ops.append((seq[i],))
            i += 1
    return ops


_RANGE = {16: (3, 2), 17: (3, 3), 18: (11, 7)}  # first repeat count, bits of the count


class Stream:
    """One raw DEFLATE stream, block by block."""

    def __init__(self, invalid=None, tail_fill=0):
        self.w = BitWriter()
        self.out = None if invalid else bytearray()
        self.invalid = invalid
        self.tail_fill = tail_fill  # what the unused bits of the last byte hold
        self.trace = set()
        self.blocks = 0
        if tail_fill:
            self.trace.add("tail bits set")

    # -- expansion --
    def _literal(self, b):
        if self.out is not None:
            self.out.append(b)

    def _match(self, length, distance):
        if self.out is None:
            return
        if not 3 <= length <= 258 or not 1 <= distance <= 32768:
            raise ValueError("no such match: %d, %d" % (length, distance))
        if distance > len(self.out):
            raise ValueError("distance %d past the %d bytes of history" % (distance, len(self.out)))
        if distance >= length:
            at = len(self.out) - distance
            self.out += self.out[at: at + length]
        else:
            for _ in range(length):
                self.out.append(self.out[-distance])

    def _head(self, final, btype):
        self.w.put(1 if final else 0, 1)
        self.w.put(btype, 2)
        self.blocks += 1
        self.trace.add("kind:" + ("stored", "fixed", "dynamic", "reserved")[btype])

    def reserved(self, final=True):
        """The header of a block of type 3 (invalid streams)."""
        self._invalid_only()
        self._head(final, 3)
        return self

    def raw_bits(self, value, n):
        """Bits as they are (invalid streams, and padding in front of a block)."""
        self.w.put(value, n)

    # -- blocks --
    def stored(self, data, final=False, pad=0, length=None, nlen=None):
        """A stored block; `pad`: the bits between the header and LEN; length / nlen: other field values (invalid)."""
        data = bytes(data)
        if self.invalid is None and (len(data) > 65535 or length is not None or nlen is not None):
            raise ValueError("a stored block holds at most 65 535 bytes and says so truthfully")
        self._head(final, 0)
        if self.w.n and pad:
            self.trace.add("stored:padding set")
        self.trace.add("stored:phase%d" % self.w.n)
        self.w.align(pad)
        n = len(data) if length is None else length
        self.w.put(n, 16)
        self.w.put(n ^ 0xFFFF if nlen is None else nlen, 16)
        self.w.raw(data)
        self.trace.add("stored:%d" % len(data) if len(data) in (0, 65535) else "stored:some")
        if self.out is not None:
            self.out += data
        return self

    def fixed(self, symbols, final=False, end=True):
        self._head(final, 1)
        self._symbols(symbols, canonical_codes(FIXED_LL), canonical_codes(FIXED_D), end)
        return self

    def dynamic(self, symbols, ll_lens, d_lens, final=False, hlit=None, hdist=None, hclen=None, cl_lens=None, ops=None,
                forced=None, plain=False, end=True):
        """ll_lens / d_lens: lists or {symbol: length}. hlit / hdist / hclen: the COUNTS (257.., 1.., 4..), smallest that
        fits by default; in an invalid stream any count the field can hold. ops: the run-length operations, or the greedy
        encoder's (with `forced` / `plain`, see greedy_ops)."""
        ll = _as_list(ll_lens, 288)
        dd = _as_list(d_lens, 32)
        loose = self.invalid is not None
        if hlit is None:
            hlit = max(257, max([i + 1 for i, l in enumerate(ll) if l] + [0]))
        if hdist is None:
            hdist = max(1, max([i + 1 for i, l in enumerate(dd) if l] + [0]))
        if not loose:
            if not (257 <= hlit <= 286 and 1 <= hdist <= 30) or any(ll[hlit:]) or any(dd[hdist:]):
                raise ValueError("HLIT / HDIST do not hold the lengths")
            if kraft(ll) > 1 << 15 or kraft(dd) > 1 << 15:
                raise ValueError("over-subscribed code lengths")
        seq = ll[:hlit] + dd[:hdist]
        if ops is None:
            ops = greedy_ops(seq, forced, plain)
        ops = [tuple(op) if isinstance(op, (tuple, list)) else (op,) for op in ops]
        if not loose and expand_ops(ops) != seq:
            raise ValueError("the operations do not send the code lengths")
        used = sorted({op[0] for op in ops if op[0] != "bits"})
        if cl_lens is None:
            # the code-length code nobody asked for: equal lengths, completed (zlib wants this code complete)
            k = max(1, (len(used) - 1).bit_length())
            short = (1 << k) - len(used)  # this many codes of k - 1 bits and the rest of k bits fill the code space
            cl = [0] * 19
            for i, s in enumerate(used):
                cl[s] = k - 1 if i < short and len(used) > 1 else k
            cl = complete_lengths(cl, [s for s in CL_ORDER if s not in used], 7)
        else:
            cl = _as_list(cl_lens, 19)
        if hclen is None:
            hclen = max(4, max([i + 1 for i, s in enumerate(CL_ORDER) if cl[s]] + [0]))
        if not loose:
            if not 4 <= hclen <= 19 or any(cl[s] for s in CL_ORDER[hclen:]) or max(cl) > 7 or kraft(cl, 7) > 1 << 7:
                raise ValueError("HCLEN or the code-length code is not valid")
        cl_code = canonical_codes(cl, check=not loose)
        self._head(final, 2)
        w = self.w
        w.put(hlit - 257, 5), w.put(hdist - 1, 5), w.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.put(cl[s], 3)
        at = 0
        for op in ops:
            if op[0] == "bits":
                self._invalid_only()
                w.put(op[1], op[2])
                continue
            if op[0] not in cl_code:
                raise ValueError("code-length symbol %d has no code" % op[0])
            w.put(*cl_code[op[0]], msb_first=True)
            if op[0] >= 16:
                first, bits = _RANGE[op[0]]
                if not 0 <= op[1] - first < 1 << bits:
                    raise ValueError("no such repeat count: %r" % (op,))
                w.put(op[1] - first, bits)
                self.trace.add("op%d:%d" % op)
                if at < hlit < at + op[1]:
                    self.trace.add("repeat crosses boundary")
                    self.trace.add("repeat crosses boundary:%d" % op[0])
                at += op[1]
            else:
                at += 1
        self.trace |= {"hlit:%d" % hlit, "hdist:%d" % hdist, "hclen:%d" % hclen, "cl_max:%d" % max(cl)}
        if sum(1 for l in dd if l) <= 1:
            self.trace.add("dist codes:%d" % sum(1 for l in dd if l))
        for name, lens in (("litlen", ll), ("dist", dd)):
            if 0 < kraft(lens) < 1 << 15 and not (name == "dist" and sum(1 for l in lens if l) == 1):
                self.trace.add("incomplete " + name)
        self._symbols(symbols, canonical_codes(ll, check=not loose), canonical_codes(dd, check=not loose), end)
        return self

    def _symbols(self, symbols, ll_code, d_code, end):
        w = self.w
        ll_max = d_max = 0

        def send(code, sym, what):
            if sym not in code:
                raise ValueError("%s symbol %d has no code" % (what, sym))
            w.put(*code[sym], msb_first=True)
            return code[sym][1]

        for item in _flatten(symbols):
            if isinstance(item, int):
                ll_max = max(ll_max, send(ll_code, item, "literal"))
                self._literal(item)
            elif item[0] == "bits":
                self._invalid_only()
                w.put(item[1], item[2])
            elif item[0] == "ll":
                self._invalid_only()
                ll_max = max(ll_max, send(ll_code, item[1], "literal/length"))
            elif item[0] == "pair":
                self._invalid_only()
                _, ls, lx, ds, dx = item
                ll_max = max(ll_max, send(ll_code, ls, "length"))
                w.put(lx, LEN_EXTRA[ls - 257] if 257 <= ls <= 285 else 0)
                if ds is not None:  # None: a block without distance codes
                    d_max = max(d_max, send(d_code, ds, "distance"))
                    w.put(dx, DIST_EXTRA[ds] if ds < 30 else 0)
            else:
                length, distance = item[0], item[1]
                ls = item[2] if len(item) > 2 else length_symbol(length)
                lx = length - LEN_BASE[ls - 257]
                if not 0 <= lx < 1 << LEN_EXTRA[ls - 257] and not (ls == 285 and lx == 0):
                    raise ValueError("length %d is not one of symbol %d" % (length, ls))
                if (length, ls) == (258, 284):
                    self.trace.add("284+31")
                ds = distance_symbol(distance)
                self._match(length, distance)
                ll_max = max(ll_max, send(ll_code, ls, "length"))
                w.put(lx, LEN_EXTRA[ls - 257])
                d_max = max(d_max, send(d_code, ds, "distance"))
                w.put(distance - DIST_BASE[ds], DIST_EXTRA[ds])
                self.trace |= {"len_sym:%d" % ls, "dist_sym:%d" % ds}
        if end:
            ll_max = max(ll_max, send(ll_code, 256, "end of block"))
        elif self.invalid is None:
            raise ValueError("a block ends with symbol 256")
        self.trace |= {"ll_max:%d" % ll_max, "d_max:%d" % d_max}

    def _invalid_only(self):
        if self.invalid is None:
            raise ValueError("raw items belong to streams marked invalid")

    def bytes(self):
        w = self.w
        if w.n and self.tail_fill:
            return bytes(w.out) + bytes([w.acc | (0xFF << w.n) & 0xFF])
        return w.bytes()


def _as_list(lens, n):
    if isinstance(lens, dict):
        out = [0] * n
        for s, l in lens.items():
            out[s] = l
        return out
    return list(lens) + [0] * (n - len(lens))


def _flatten(symbols):
    for item in symbols:
        if isinstance(item, (bytes, bytearray)):
            yield from item
        else:
            yield item


# ---- gzip (RFC 1952) ----

_CRC = []
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ (0xEDB88320 if _c & 1 else 0)
    _CRC.append(_c)


def crc32(data):
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


FTEXT, FHCRC, FEXTRA, FNAME, FCOMMENT = 1, 2, 4, 8, 16


def gzip_member(deflate, out, extra=None, name=None, comment=None, hcrc=False, flg=None, cm=8, mtime=0, xfl=0, os=255,
                crc=None, isize=None, hcrc_value=None):
    """A member around a raw stream. extra: the bytes of the extra field (XLEN is written for them); name / comment: bytes
    without the terminator (one is added); FLG says what is there unless `flg` says otherwise; crc / isize / hcrc_value:
    other values than the true ones."""
    f = (FEXTRA if extra is not None else 0) | (FNAME if name is not None else 0) | (FCOMMENT if comment is not None else 0) | (FHCRC if hcrc else 0)
    head = bytes([0x1F, 0x8B, cm, f if flg is None else flg]) + mtime.to_bytes(4, "little") + bytes([xfl, os])
    if extra is not None:
        head += len(extra).to_bytes(2, "little") + bytes(extra)
    if name is not None:
        head += bytes(name) + b"\0"
    if comment is not None:
        head += bytes(comment) + b"\0"
    if hcrc:
        head += ((crc32(head) & 0xFFFF) if hcrc_value is None else hcrc_value).to_bytes(2, "little")
    out = bytes(out)
    tail = (crc32(out) if crc is None else crc).to_bytes(4, "little") + ((len(out) & 0xFFFFFFFF) if isize is None else isize).to_bytes(4, "little")
    return head + bytes(deflate) + tail


def rnd_bytes(seed, n, alphabet=None):
    r = random.Random(seed)
    if alphabet is None:
        return r.randbytes(n)
    alphabet = list(alphabet)
    return bytes(r.choice(alphabet) for _ in range(n))
