"""A lane model of the wave64 primitives of nvcomp_amd/csrc/common/wave.h, in plain numpy and Python.

Every primitive is a function over arrays of 64 lane values plus wave-uniform arguments, written from the documented
meaning (the comment above the primitive in common/wave.h), serially over the lanes, sums taken in uint64 and
truncated. Each function checks its preconditions first and raises ContractError: tests/test_wave_primitives.py calls the
model before any launch, so an input that would make a kernel loop forever or read outside the wave reaches neither the
card nor the emulator.
"""
import numpy as np

N = 64
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


class ContractError(ValueError):
    """An input outside a primitive's documented domain."""


def _need(ok, what):
    if not ok:
        raise ContractError(what)


def _lanes(v):
    """64 lane values as Python ints in 0 .. 2^32 - 1."""
    v = [int(x) for x in np.asarray(v).reshape(-1)]
    _need(len(v) == N, "a lane vector has 64 entries")
    _need(all(0 <= x <= M32 for x in v), "lane values are 32-bit")
    return v


def _u32(v):
    return np.array([x & M32 for x in v], dtype=np.uint32)


def _lane_index(lane):
    lane = int(lane)
    _need(0 <= lane < N, f"lane index {lane} is not in 0..63")
    return lane


def _mask(m):
    m = int(m)
    _need(0 <= m <= M64, "a wave mask has 64 bits")
    return m


# ---- lane ids, masks ----------------------------------------------------------------------------------------------

def lane_id():
    return np.arange(N, dtype=np.uint32)


fresh_lane_id = lane_id


def lane_in(mask):
    mask = _mask(mask)
    return _u32([(mask >> i) & 1 for i in range(N)])


def ballot(pred):
    pred = np.asarray(pred).reshape(-1)
    _need(pred.size == N, "a lane vector has 64 entries")
    return sum(1 << i for i in range(N) if pred[i])


def prefix_popc(mask):
    mask = _mask(mask)
    out, below = [], 0
    for i in range(N):
        out.append(below)
        below += (mask >> i) & 1
    return _u32(out)


def popc64(mask):
    return bin(_mask(mask)).count("1")


def ctz64(mask):
    mask = _mask(mask)
    _need(mask != 0, "ctz64 of an empty mask")
    i = 0
    while not (mask >> i) & 1:
        i += 1
    return i


# ---- broadcasts and lane writes -----------------------------------------------------------------------------------

def read_lane(v, lane):
    return _lanes(v)[_lane_index(lane)]


def uniform(v):
    v = _lanes(v)
    _need(all(x == v[0] for x in v), "uniform() of a value that differs between lanes")
    return v[0]


def uniform64(lo, hi):
    return (uniform(hi) << 32) | uniform(lo)


def write_lane(vec, val, lane):
    vec = _lanes(vec)
    val = int(val)
    _need(0 <= val <= M32, "the written value is 32-bit")
    vec[_lane_index(lane)] = val
    return _u32(vec)


write_lane_scalar = write_lane


# ---- the serial walks ---------------------------------------------------------------------------------------------

def chain_walk(step, limit, r, k, rec):
    """repeat { rec[k++] = r; r += step[r]; } while (r < limit). Returns (r, k, rec)."""
    step, rec = _lanes(step), _lanes(rec)
    limit, r, k = int(limit), int(r), int(k)
    _need(0 <= r < limit <= N, f"chain_walk needs r < limit <= 64 (r = {r}, limit = {limit})")
    _need(0 <= k < N, f"chain_walk needs k < 64 (k = {k})")
    while True:
        _need(k < N, "chain_walk needs k + iterations <= 64")
        _need(step[r] >= 1, f"chain_walk: the step of lane {r} is 0, the walk would not end")
        rec[k] = r
        k += 1
        r += step[r]
        _need(r <= M32, "chain_walk: the position wrapped")
        if r >= limit:
            break
    return r, k, _u32(rec)


def select_walk(candidates, length, start):
    """From lane `start`: take the lowest candidate f at or above the current lane, go on at f + length[f]. Returns
    (taken, end)."""
    candidates, length, start = _mask(candidates), _lanes(length), int(start)
    _need(0 <= start < N, f"select_walk needs start < 64 (start = {start})")
    _need(candidates >> start != 0, "select_walk needs a candidate at or above start")
    taken, pos = 0, start
    while pos < N and candidates >> pos:
        while not (candidates >> pos) & 1:
            pos += 1
        _need(1 <= length[pos] <= 63, f"select_walk: the length of taken lane {pos} is {length[pos]}, not in 1..63")
        taken |= 1 << pos
        pos += length[pos]
    return taken, pos


# ---- moves --------------------------------------------------------------------------------------------------------

def shuffle(v, src_lane):
    """Lane i receives v of lane src_lane[i]; the index is taken modulo 64."""
    v, src = _lanes(v), _lanes(src_lane)
    return _u32([v[src[i] & 63] for i in range(N)])


def permute_to(v, dst_lane):
    v, dst = _lanes(v), _lanes(dst_lane)
    _need(sorted(dst) == list(range(N)), "permute_to: the destinations are not a permutation of 0..63")
    out = [0] * N
    for i in range(N):
        out[dst[i]] = v[i]
    return _u32(out)


def prev_lane(v):
    v = _lanes(v)
    return _u32([0] + v[:-1])


def next_lane(v):
    v = _lanes(v)
    return _u32(v[1:] + [0])


# ---- scans and reductions -----------------------------------------------------------------------------------------

def scan_add_inclusive(v):
    out, s = [], 0
    for x in _lanes(v):
        s += x
        out.append(s)
    return _u32(out)


def reduce_add(v):
    return sum(_lanes(v)) & M32


def umax(a, b):
    return _u32([max(x, y) for x, y in zip(_lanes(a), _lanes(b))])


def scan_max_inclusive(v):
    out, m = [], 0
    for x in _lanes(v):
        m = max(m, x)
        out.append(m)
    return _u32(out)


def reduce_max(v):
    return max(_lanes(v))


def scan_last_writer(val, mask):
    """Lane k: per bit, the value bit of the highest lane j <= k whose mask has the bit (0 where none has), and the OR of
    the masks of lanes 0..k. Returns (val, mask)."""
    val, mask = _lanes(val), _lanes(mask)
    out_v, out_m = [], []
    for k in range(N):
        v = m = 0
        for bit in range(32):
            for j in range(k, -1, -1):
                if (mask[j] >> bit) & 1:
                    v |= ((val[j] >> bit) & 1) << bit
                    m |= 1 << bit
                    break
        out_v.append(v)
        out_m.append(m)
    return _u32(out_v), _u32(out_m)


# ---- LDS read-modify-write ----------------------------------------------------------------------------------------

def _lds_rmw(words, index, value, fn):
    words, index, value = _lanes(words), _lanes(index), _lanes(value)
    _need(all(i < N for i in index), "an LDS word index is outside the 64 words")
    for i in range(N):
        words[index[i]] = fn(words[index[i]], value[i]) & M32
    return _u32(words)


def lds_or(words, index, bits):
    return _lds_rmw(words, index, bits, lambda w, v: w | v)


def lds_add(words, index, v):
    return _lds_rmw(words, index, v, lambda w, x: w + x)


def lds_sub(words, index, v):
    return _lds_rmw(words, index, v, lambda w, x: w - x)


# ---- per-lane arithmetic ------------------------------------------------------------------------------------------

def _per_lane(fn, *operands):
    ops = [_lanes(o) for o in operands]
    return _u32([fn(*xs) for xs in zip(*ops)])


def _mul24(a, b):
    _need(a < (1 << 24) and b < (1 << 24), "mul24: an operand is not below 2^24")
    return (a * b) & M32


def _align_bits(hi, lo, shift):
    _need(shift <= 31, f"align_bits: the shift {shift} is not in 0..31")
    return (((hi << 32) | lo) >> shift) & M32


def _align_bytes(hi, lo, shift):
    return (((hi << 32) | lo) >> (8 * (shift & 3))) & M32  # only the low two bits of the shift count


def _pk_add_sat255(a, b):
    lo = min(((a & 0xFFFF) + (b & 0xFFFF)) & 0xFFFF, 255)
    hi = min(((a >> 16) + (b >> 16)) & 0xFFFF, 255)
    return lo | (hi << 16)


def _bit_reverse(v):
    return sum(((v >> i) & 1) << (31 - i) for i in range(32))


def _perm_bytes(hi, lo, sel):
    src = (hi << 32) | lo
    out = 0
    for i in range(4):
        s = (sel >> (8 * i)) & 0xFF
        _need(s <= 7 or s >= 12, f"perm_bytes: the selector byte {s} is in 8..11")
        byte = (src >> (8 * s)) & 0xFF if s <= 7 else 0 if s == 12 else 0xFF
        out |= byte << (8 * i)
    return out


def mul24(a, b):
    return _per_lane(_mul24, a, b)


def align_bits(hi, lo, shift):
    return _per_lane(_align_bits, hi, lo, shift)


def align_bytes(hi, lo, shift):
    return _per_lane(_align_bytes, hi, lo, shift)


def pk_add_sat255(a, b):
    return _per_lane(_pk_add_sat255, a, b)


def bit_reverse(v):
    return _per_lane(_bit_reverse, v)


def perm_bytes(hi, lo, sel):
    return _per_lane(_perm_bytes, hi, lo, sel)
