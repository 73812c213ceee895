"""A Zstandard frame writer for tests, written from RFC 8878. Pure Python, no libzstd.

The writer never chooses: the caller says what goes on the wire (frame header fields, block types and sizes, the
literals section's type, header width, stream count and Huffman weights, the sequences and the mode and table of each of
LL / OF / ML), and the writer says what those bytes mean: `Frame.out` is the plain expansion of the description
(literals, then the match byte by byte, the repeat-offset rules of RFC 8878 3.1.1.5 applied here). That expansion is the
reference of tests/test_zstd_format.py; tests/test_zstd_format.py::test_writer_against_libzstd checks it against CPU
libzstd where one can be loaded.

    f = Frame(fcs_bytes=1)
    f.raw(b"abc")
    f.compressed(lit=raw_lit(b"xy"), seqs=[(2, 4, 3), (0, 3, REP1)], ml=("fse", None, 5), last=True)
    f.bytes(), f.out

`check=False` on a call lets a description through that no decoder may accept (the invalid frames of the tests).
"""

MAGIC = 0xFD2FB528
BLOCK_MAX = 128 * 1024

# ---- code tables (RFC 8878 3.1.1.3.2.1.1): the extra bits per code; the baselines follow from them ----
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def _bases(first, bits):
    out = []
    for b in bits:
        out.append(first)
        first += 1 << b
    return out


LL_BASE = _bases(0, LL_BITS)
ML_BASE = _bases(3, ML_BITS)
assert LL_BASE[35] == 65536 and ML_BASE[52] == 65539 and LL_BASE[25] == 64 and ML_BASE[43] == 131

# predefined distributions (RFC 8878 3.1.1.3.2.2) and their accuracy logs
LL_DEFAULT = [4, 3] + [2] * 11 + [1] * 3 + [2] * 9 + [3, 2] + [1] * 5 + [-1] * 4
ML_DEFAULT = [1, 4, 3] + [2] * 6 + [1] * 37 + [-1] * 7
OF_DEFAULT = [1] * 6 + [2] * 3 + [1] * 15 + [-1] * 5
DEFAULTS = {"LL": (LL_DEFAULT, 6), "OF": (OF_DEFAULT, 5), "ML": (ML_DEFAULT, 6)}
MAX_LOG = {"LL": 9, "OF": 8, "ML": 9}
MAX_SYM = {"LL": 35, "OF": 31, "ML": 52}
assert len(LL_DEFAULT) == 36 and len(ML_DEFAULT) == 53 and len(OF_DEFAULT) == 29
assert all(sum(abs(c) for c in d) == 1 << lg for d, lg in DEFAULTS.values())

REP1, REP2, REP3 = "rep1", "rep2", "rep3"  # Repeated_Offset codes in a sequence's offset field
_REP = {REP1: 1, REP2: 2, REP3: 3}


def ll_code(v):
    return max(c for c in range(36) if LL_BASE[c] <= v)


def ml_code(v):
    return max(c for c in range(53) if ML_BASE[c] <= v)


# ---- bits ----

class BitsForward:
    """Little-endian bit packing, read forwards (FSE table descriptions)."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def add(self, v, nbits):
        assert 0 <= v < (1 << nbits) or nbits == 0 and v == 0, (v, nbits)
        self.acc |= v << self.n
        self.n += nbits

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def backward_stream(reads, padding=True, leftover=0):
    """The bytes of a stream read backwards (RFC 8878 4.1): `reads` is the list of (value, bits) in the order the decoder
    reads them, so it is written last to first, then the padding bit. `leftover` zero bits are put in front of
    everything (bits no decoder reads: an invalid stream); `padding=False` leaves a zero last byte."""
    w = BitsForward()
    w.add(0, leftover)
    for v, nbits in reversed(reads):
        w.add(v, nbits)
    if padding:
        w.add(1, 1)
        return w.bytes()
    return w.bytes() + b"\0"


# ---- FSE ----

class Fse:
    """The decoding table of normalized counts (RFC 8878 4.1.1), and what an encoder needs of it."""

    def __init__(self, norm, log):
        size = 1 << log
        assert sum(abs(c) for c in norm) == size, "counts do not sum to the table size"
        sym, high, nxt = [0] * size, size - 1, []
        for s, c in enumerate(norm):
            if c == -1:
                sym[high] = s
                high -= 1
                nxt.append(1)
            else:
                nxt.append(c)
        step, pos = (size >> 1) + (size >> 3) + 3, 0
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                sym[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
        assert pos == 0
        self.log, self.sym, self.nb, self.base = log, sym, [], []
        for u in range(size):
            x = nxt[sym[u]]
            nxt[sym[u]] += 1
            nb = log - (x.bit_length() - 1)
            self.nb.append(nb)
            self.base.append((x << nb) - size)
        self._into = {}

    @classmethod
    def rle(cls, symbol):
        t = cls.__new__(cls)
        t.log, t.sym, t.nb, t.base, t._into = 0, [symbol], [0], [0], {}
        return t

    def first_state(self, s):
        """The state of symbol s that reads the most bits (its lowest state): where an encoder starts."""
        return self.sym.index(s)

    def state_into(self, s, nxt):
        """The state that emits s and whose next-state range holds `nxt`."""
        m = self._into.get(s)
        if m is None:
            m = [None] * len(self.sym)
            for u, su in enumerate(self.sym):
                if su == s:
                    for v in range(self.base[u], self.base[u] + (1 << self.nb[u])):
                        m[v] = u
            self._into[s] = m
        return m[nxt]

    def chain(self, symbols):
        """States u_0 .. u_n-1 that emit `symbols` in decoding order."""
        states = [0] * len(symbols)
        for k in range(len(symbols) - 1, -1, -1):
            s = symbols[k]
            assert s in self.sym, f"symbol {s} has no state in the table"
            states[k] = self.first_state(s) if k == len(symbols) - 1 else self.state_into(s, states[k + 1])
        return states


def ncount(norm, log, max_log=None):
    """An FSE table description (RFC 8878 4.1.1) of `norm` (trailing zeros dropped). With max_log=None nothing is
    checked: a log out of range or counts that stop short of the table size are written as they are."""
    norm = list(norm)
    while norm and norm[-1] == 0:
        norm.pop()
    if max_log is not None:
        assert 5 <= log <= max_log and sum(abs(c) for c in norm) == 1 << log
    w = BitsForward()
    w.add(log - 5, 4)
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    s = 0
    while s < len(norm) and remaining > 1:
        c = norm[s]
        s += 1
        val, mx = c + 1, 2 * threshold - 1 - remaining
        if val < mx:
            w.add(val, nb - 1)
        else:
            w.add(val + mx if val >= threshold else val, nb)
        remaining -= abs(c)
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
        if c == 0:
            zeros = 0
            while s < len(norm) and norm[s] == 0:
                zeros += 1
                s += 1
            for _ in range(zeros // 3):
                w.add(3, 2)
            w.add(zeros % 3, 2)
    return w.bytes()


def normalize(hist, log, low=1):
    """Normalized counts of a histogram that sum to 1 << log: every present symbol gets at least 1 (`low=-1`: the
    less-than-one marker for those that round to nothing), the most frequent takes the remainder."""
    size, total = 1 << log, sum(hist)
    norm = []
    for h in hist:
        c = h * size // total if h else 0
        norm.append(c if c >= 1 or h == 0 else low)
    top = max(range(len(hist)), key=lambda i: hist[i])
    norm[top] += size - sum(abs(c) for c in norm)
    assert norm[top] >= 1, "too many symbols for this accuracy log"
    return norm


# ---- Huffman ----

def huffman_weights(hist, depth=11):
    """Weights (0: absent) of a complete prefix code of at most `depth` bits for the symbols present in `hist`."""
    import heapq

    freq = {s: h for s, h in enumerate(hist) if h}
    assert len(freq) >= 2, "a Huffman table needs two symbols"
    while True:
        heap = [(f, s, (s,)) for s, f in freq.items()]
        heapq.heapify(heap)
        length = dict.fromkeys(freq, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                length[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        mx = max(length.values())
        if mx <= depth:
            break
        freq = {s: f // 2 + 1 for s, f in freq.items()}
    return [mx + 1 - length[s] if s in length else 0 for s in range(max(freq) + 1)]


class Huffman:
    """Prefix codes from weights (RFC 8878 4.2.1.3); weights[-1] is the symbol the description leaves out.
    `strict=False` takes weights that complete no code (invalid on purpose): the codes are handed out in the same
    order, so those of the smallest weight are still what a decoder that skipped the check would read."""

    def __init__(self, weights, strict=True):
        self.weights = list(weights)
        total = sum(1 << (w - 1) for w in weights if w)
        self.max_bits = (total - 1).bit_length()
        assert total == 1 << self.max_bits or not strict, "the weights complete no code"
        self.code, nxt = {}, 0
        for w in range(1, self.max_bits + 1):
            for s, ws in enumerate(weights):
                if ws == w:
                    self.code[s] = (nxt >> (w - 1), self.max_bits + 1 - w)
                    nxt += 1 << (w - 1)

    def stream(self, data):
        return backward_stream([self.code[x] for x in data])


def weights_direct(listed):
    assert 1 <= len(listed) <= 128
    out = bytearray([127 + len(listed)])
    for i in range(0, len(listed), 2):
        out.append(listed[i] << 4 | (listed[i + 1] if i + 1 < len(listed) else 0))
    return bytes(out)


def weights_fse(listed, log=6, norm=None):
    """FSE-compressed weights (RFC 8878 4.2.1.2): two interleaved states; the last two weights are the states the
    decoder is left in when the stream runs out."""
    n = len(listed)
    assert n >= 2
    if norm is None:
        hist = [0] * (max(listed) + 1)
        for x in listed:
            hist[x] += 1
        norm = normalize(hist, log)
    t = Fse(norm, log)
    even, odd = t.chain(listed[0::2]), t.chain(listed[1::2])
    reads = [(even[0], log), (odd[0], log)]
    for i in range(n - 2):
        states = even if i % 2 == 0 else odd
        u, v = states[i // 2], states[i // 2 + 1]
        reads.append((v - t.base[u], t.nb[u]))
    body = ncount(norm, log, 6) + backward_stream(reads)
    assert len(body) < 128, "FSE-compressed weights must fit 127 bytes"
    return bytes([len(body)]) + body


# ---- literals sections ----

def raw_lit(data, hl=None):
    return {"kind": "raw", "data": bytes(data), "hl": hl}


def rle_lit(byte, regen, hl=None):
    return {"kind": "rle", "data": bytes([byte]) * regen, "byte": byte, "hl": hl}


def huf_lit(data, streams=4, sf=None, weights=None, desc="direct", depth=11, counts=None):
    """Huffman literals. `weights`: one per symbol up to and including the last present one (None: from the
    histogram, at most `depth` bits); `desc`: "direct" or "fse"; `sf`: Size_Format (None: the smallest that fits);
    `counts`: symbols per stream, where a description other than the format's own split is wanted (invalid)."""
    return {"kind": "huf", "data": bytes(data), "streams": streams, "sf": sf, "weights": weights, "desc": desc,
            "depth": depth, "counts": counts}


def treeless_lit(data, streams=4, sf=None):
    return {"kind": "treeless", "data": bytes(data), "streams": streams, "sf": sf, "counts": None}


def xxh64(data, seed=0):
    """XXH64 (the content checksum is its low 4 bytes)."""
    p1, p2, p3, p4, p5 = (11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579,
                          2870177450012600261)
    m = (1 << 64) - 1

    def rotl(x, r):
        return ((x << r) | (x >> (64 - r))) & m

    def rnd(acc, v):
        return rotl((acc + v * p2) & m, 31) * p1 & m

    def le(at, nbytes):
        return int.from_bytes(data[at: at + nbytes], "little")

    n, p = len(data), 0
    if n >= 32:
        v = [(seed + p1 + p2) & m, (seed + p2) & m, seed, (seed - p1) & m]
        while p + 32 <= n:
            v = [rnd(v[i], le(p + 8 * i, 8)) for i in range(4)]
            p += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & m
        for x in v:
            h = ((h ^ rnd(0, x)) * p1 + p4) & m
    else:
        h = (seed + p5) & m
    h = (h + n) & m
    while p + 8 <= n:
        h = (rotl(h ^ rnd(0, le(p, 8)), 27) * p1 + p4) & m
        p += 8
    if p + 4 <= n:
        h = (rotl(h ^ (le(p, 4) * p1 & m), 23) * p2 + p3) & m
        p += 4
    while p < n:
        h = rotl(h ^ (data[p] * p5 & m), 11) * p1 & m
        p += 1
    h = (h ^ (h >> 33)) * p2 & m
    h = (h ^ (h >> 29)) * p3 & m
    return h ^ (h >> 32)


def skippable(payload=b"", nibble=0):
    return (0x184D2A50 | nibble).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + bytes(payload)


def _copy_match(out, off, ml):
    """out[-off] byte by byte, ml times (a match may overlap what it writes: then it repeats its last `off` bytes)."""
    if off >= ml:
        start = len(out) - off
        out += out[start: start + ml]
    else:
        unit = bytes(out[len(out) - off:])
        out += (unit * (ml // off + 1))[:ml]


class Frame:
    """One frame. Header fields are the constructor's; blocks are appended with raw() / rle() / compressed() / block().
    `out` is the frame's expansion, `trace` what the sequences did that no header shows."""

    def __init__(self, single=True, window_log=None, fcs_bytes=None, fcs=None, checksum=False, header=None):
        """fcs_bytes 0 / 1 / 2 / 4 / 8 (None: 1 with Single_Segment, else 0); 1 needs Single_Segment, 0 forbids it.
        `fcs`: the value to write where it shall differ from the content. `header`: raw header bytes instead."""
        if fcs_bytes is None:
            fcs_bytes = 1 if single else 0
        assert fcs_bytes in (0, 1, 2, 4, 8) and (fcs_bytes != 1 or single) and (fcs_bytes != 0 or not single)
        assert single or window_log is not None
        self.single, self.window_log, self.fcs_bytes, self.fcs, self.checksum = single, window_log, fcs_bytes, fcs, checksum
        self.header = header
        self.body = bytearray()
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.tables = {"LL": None, "OF": None, "ML": None}
        self.huf = None
        self.trace = set()
        self.between, self.seen_compressed = set(), False

    # -- the frame --
    def bytes(self):
        if self.header is not None:
            head = bytes(self.header)
        else:
            flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[self.fcs_bytes]
            head = MAGIC.to_bytes(4, "little") + bytes([flag << 6 | int(self.single) << 5 | int(self.checksum) << 2])
            if not self.single:
                head += bytes([(self.window_log - 10) << 3])
            fcs = len(self.out) if self.fcs is None else self.fcs
            if self.fcs_bytes:
                head += (fcs - 256 if self.fcs_bytes == 2 else fcs).to_bytes(self.fcs_bytes, "little")
        tail = (xxh64(bytes(self.out)) & 0xFFFFFFFF).to_bytes(4, "little") if self.checksum else b""
        return head + bytes(self.body) + tail

    # -- blocks --
    def block(self, btype, size, payload, last=False):
        """A block header (Block_Size as given) and whatever bytes follow it."""
        self.body += (size << 3 | btype << 1 | int(last)).to_bytes(3, "little") + bytes(payload)

    def raw(self, data, last=False):
        self.block(0, len(data), data, last)
        self.out += data
        if self.seen_compressed:
            self.between.add("raw")

    def rle(self, byte, size, last=False):
        self.block(1, size, bytes([byte]), last)
        self.out += bytes([byte]) * size
        if self.seen_compressed:
            self.between.add("rle")

    def compressed(self, lit, seqs=(), ll=("predefined",), of=("predefined",), ml=("predefined",), last=False,
                   nseq_bytes=None, reserved=0, padding=True, leftover=0, check=True):
        """A compressed block. `seqs`: (ll, ml, offset) with offset a distance or one of REP1 / REP2 / REP3; literals
        the sequences leave over follow the last one. Each of ll / of / ml is ("predefined",), ("rle",) or
        ("rle", symbol), ("fse", counts, log), ("fse", None, log) or ("fse", None, log, -1) to normalize the block's
        histogram (-1: rare symbols become less-than-one entries), or ("repeat",). `nseq_bytes`: the width of
        Number_of_Sequences (None: the smallest); `reserved`: the mode byte's low bits; `padding` / `leftover`: see
        backward_stream()."""
        payload = self._literals(lit, check) + self._sequences(lit["data"], list(seqs), ll, of, ml, nseq_bytes, reserved,
                                                               padding, leftover, check)
        assert not check or len(payload) <= BLOCK_MAX
        self.block(2, len(payload), payload, last)

    # -- literals --
    def _literals(self, lit, check):
        kind, data = lit["kind"], lit["data"]
        regen = len(data)
        if kind in ("raw", "rle"):
            hl = lit["hl"] or (1 if regen < 32 else 2 if regen < 4096 else 3)
            assert regen < (1 << (5, 12, 20)[hl - 1])
            t = 0 if kind == "raw" else 1
            if hl == 1:
                head = bytes([regen << 3 | t])
            else:
                head = (regen << 4 | (1 if hl == 2 else 3) << 2 | t).to_bytes(hl, "little")
            self.trace.add(f"lit:{kind}:hl{hl}")
            return head + (data if kind == "raw" else bytes([lit["byte"]]))
        streams = lit["streams"]
        tree = b""
        if kind == "huf":
            weights = lit["weights"]
            if weights is None:
                hist = [0] * 256
                for x in data:
                    hist[x] += 1
                weights = huffman_weights(hist, lit["depth"])
            listed = list(weights[:-1])
            tree = weights_direct(listed) if lit["desc"] == "direct" else weights_fse(listed)
            self.huf = Huffman(weights, strict=check)
            self.trace.add(f"huf:{lit['desc']}:{len(listed)}")
            self.trace.add(f"huf:depth{self.huf.max_bits}")
        else:
            assert self.huf is not None or not check, "treeless literals need an earlier Huffman table"
        huf = self.huf
        if huf is None:  # treeless without a table, invalid on purpose: any table will do for the bytes that follow
            huf = Huffman([1, 1])
            data = bytes(x & 1 for x in data)
        if streams == 1:
            body = huf.stream(data)
        else:
            seg = (regen + 3) // 4
            counts = lit["counts"] or [seg, seg, seg, regen - 3 * seg]
            assert sum(counts) == regen and min(counts) >= 0, "this many literals cannot be split into four streams"
            parts, at = [], 0
            for c in counts:
                parts.append(huf.stream(data[at: at + c]))
                at += c
            body = b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
        csize = len(tree) + len(body)
        sf = lit["sf"]
        if sf is None:
            sf = 0 if streams == 1 else 1 if max(regen, csize) < 1024 else 2 if max(regen, csize) < 16384 else 3
        assert (sf == 0) == (streams == 1)
        bits = (10, 10, 14, 18)[sf]
        assert regen < (1 << bits) and csize < (1 << bits), "sizes do not fit this Size_Format"
        t = 2 if kind == "huf" else 3
        head = (t | sf << 2 | regen << 4 | csize << (4 + bits)).to_bytes((3, 3, 4, 5)[sf], "little")
        self.trace.add(f"lit:{kind}:sf{sf}")
        return head + tree + body

    # -- sequences --
    def _table(self, name, spec, codes, check):
        """(table, description bytes, mode) of one of LL / OF / ML for this block's codes."""
        kind = spec[0]
        if kind == "predefined":
            t, desc, mode = Fse(*DEFAULTS[name]), b"", 0
        elif kind == "rle":
            sym = spec[1] if len(spec) > 1 else codes[0]
            t, desc, mode = Fse.rle(sym), bytes([sym]), 1
        elif kind == "fse":
            norm, log = spec[1], spec[2]
            if norm is None:
                hist = [0] * (max(codes) + 1)
                for c in codes:
                    hist[c] += 1
                norm = normalize(hist, log, spec[3] if len(spec) > 3 else 1)
            desc, mode = ncount(norm, log, MAX_LOG[name] if check else None), 2
            assert not check or len(norm) <= MAX_SYM[name] + 1
            try:
                t = Fse(norm, log)
            except AssertionError:
                if check:
                    raise
                t = Fse(normalize([1 if c else 0 for c in norm], log), log)  # invalid on purpose: some table for the bits
        else:
            assert kind == "repeat"
            t, desc, mode = self.tables[name], b"", 3
            if t is None:
                assert not check, "repeat mode needs an earlier table"
                return Fse(*DEFAULTS[name]), b"", 3
        self.tables[name] = t
        return t, desc, mode

    def _sequences(self, literals, seqs, ll, of, ml, nseq_bytes, reserved, padding, leftover, check):
        n = len(seqs)
        width = nseq_bytes or (1 if n < 128 else 2 if n < 0x7F00 else 3)
        if width == 1:
            assert n < 128
            head = bytes([n])
        elif width == 2:
            assert n < 0x7F00
            head = bytes([128 + (n >> 8), n & 255])
        else:
            assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
            head = b"\xff" + (n - 0x7F00).to_bytes(2, "little")
        self.trace.add(f"nseq:{width}")
        at = 0
        fields = []
        for s_ll, s_ml, s_off in seqs:
            self.out += literals[at: at + s_ll]
            at += s_ll
            assert not check or at <= len(literals), "the sequences overrun the literals"
            if s_off in _REP:
                ofv = _REP[s_off]
                idx = ofv - 1 + (1 if s_ll == 0 else 0)
                self.trace.add(f"rep:{ofv}:{'ll0' if s_ll == 0 else 'll'}")
                off = self.rep[idx] if idx < 3 else self.rep[0] - 1
                if idx == 1:
                    self.rep = [off, self.rep[0], self.rep[2]]
                elif idx >= 2:
                    self.rep = [off, self.rep[0], self.rep[1]]
                for b in self.between:
                    self.trace.add(f"rep:across_{b}")
                if off == 0:
                    self.trace.add("rep:zero")
                elif off > len(self.out):
                    self.trace.add("rep:before_frame")
            else:
                off, ofv = s_off, s_off + 3
                self.rep = [off, self.rep[0], self.rep[1]]
            if off > len(self.out) or off == 0:
                assert not check, "an offset before the frame"
                self.trace.add("off:before_frame")
                off = 0
            if off:
                _copy_match(self.out, off, s_ml)
            fields.append((ll_code(s_ll), s_ll, ofv.bit_length() - 1, ofv, ml_code(s_ml), s_ml))
        self.out += literals[at:]
        self.between = set()
        self.seen_compressed = True
        if n == 0:
            return head
        lt, ldesc, lmode = self._table("LL", ll, [f[0] for f in fields], check)
        ot, odesc, omode = self._table("OF", of, [f[2] for f in fields], check)
        mt, mdesc, mmode = self._table("ML", ml, [f[4] for f in fields], check)
        ls, os_, ms = lt.chain([f[0] for f in fields]), ot.chain([f[2] for f in fields]), mt.chain([f[4] for f in fields])
        reads = [(ls[0], lt.log), (os_[0], ot.log), (ms[0], mt.log)]
        for k, (lc, lv, oc, ov, mc, mv) in enumerate(fields):
            reads.append((ov - (1 << oc), oc))
            reads.append((mv - ML_BASE[mc], ML_BITS[mc]))
            reads.append((lv - LL_BASE[lc], LL_BITS[lc]))
            if k + 1 < n:
                reads.append((ls[k + 1] - lt.base[ls[k]], lt.nb[ls[k]]))
                reads.append((ms[k + 1] - mt.base[ms[k]], mt.nb[ms[k]]))
                reads.append((os_[k + 1] - ot.base[os_[k]], ot.nb[os_[k]]))
        modes = lmode << 6 | omode << 4 | mmode << 2 | reserved
        return head + bytes([modes]) + ldesc + odesc + mdesc + backward_stream(reads, padding, leftover)
