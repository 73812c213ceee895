/*
 * nvcomp/device/detail/lz4_core.hpp -- the wave-level LZ4 block decoder behind nvcomp/device/lz4.hpp (gfx950, CDNA4).
 *
 * Implementation detail; not an interface of its own. One full, converged wave64 decodes one block. It is the compact
 * version of the batched decoder's idea, written for a caller's kernel: no persistent loop, no output
 * window, no run executor.
 *
 *   staging   the stream goes through a ring of kRingBytes in the wave's scratch area, filled by aligned 16-byte loads
 *             (64 lanes x 16 bytes a step). Virtual position = byte index + (address of the stream & 15), so that ring
 *             blocks are the stream's aligned 16-byte blocks. Only blocks that lie wholly inside the stream are loaded
 *             whole; the first and the last block are read byte by byte: NOTHING outside [in, in + in_bytes) is read.
 *             16 mirror bytes behind the ring let an unaligned dword read run over its end.
 *   chase     wave-uniform: the token chain is walked over a 256-byte register window (lane l holds an aligned dword of
 *             the ring; a byte is one v_readlane), up to 64 sequences a batch. Every field is bounds-tested here, so a
 *             malformed stream is refused before anything of the batch is copied.
 *   parse     lane k reads the fields of sequence k from the ring.
 *   scan      a DPP prefix sum gives every lane its output position; capacity and offsets are tested by lane arithmetic.
 *   literals  runs of up to kLitShort bytes by their own lane out of the ring, longer ones by the whole wave from the
 *             stream, 16 bytes a lane.
 *   matches   in rounds: a lane copies once every byte of its source lies below the oldest pending match (or it is that
 *             match). offset < 4 replicates a pattern held in registers, offset >= 4 copies dwords front to back; matches
 *             above kMatchShort bytes are copied by the whole wave, the pattern doubling as it grows. A wave-scope fence
 *             (wave::sync) separates a round's stores from the next round's loads.
 *   big       a sequence with 270 literals or more, or a match of 2 059 bytes or more (a second / a ninth length byte),
 *             is a batch of its own: its length bytes are summed 64 at a time, its copies are the whole wave's.
 *
 * `out` and the stream are reached with accesses of at most 4 bytes at any alignment, or 16 bytes at 16-byte aligned
 * addresses: both may be LDS.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

/* angle brackets: the host emulation of the test suite puts its own versions of these first on the include path */
#include <nvcomp/device/detail/wave.hpp>
#include <nvcomp/device/detail/wave_ext.hpp>
#include <nvcomp/device/detail/wave_lz.hpp>

namespace nvcomp {
namespace device {
namespace detail {
namespace lz4 {

namespace wv = ::nvcomp::device::detail::wave;

enum : uint32_t {
  kErrNone = 0,
  kErrInput = 1,  /* stream truncated / malformed */
  kErrOutput = 2, /* output does not fit */
  kErrOffset = 4  /* match offset 0 or in front of the output */
};

constexpr uint32_t kRingBytes = 2048;
constexpr uint32_t kRingMask = kRingBytes - 1;
constexpr uint32_t kMirrorBytes = 16;
constexpr uint32_t kDecodeLds = kRingBytes + kMirrorBytes;
constexpr uint32_t kMaxOutCap = 1u << 26; /* the batched decoder's: a larger capacity counts as this */

constexpr uint32_t kLitShort = 32;   /* literal runs up to here are copied by their own lane */
constexpr uint32_t kMatchShort = 64; /* matches up to here likewise */
constexpr uint32_t kMatchExtMax = 8; /* length bytes of a match the lane parser follows (matches to 2 058 bytes) */
/* what a sequence of a batch spans at most in the stream: token, one length byte, 269 literals, offset, 8 length bytes */
constexpr uint32_t kSpan = 288;
static_assert(kSpan >= 1 + 1 + 269 + 2 + kMatchExtMax + 1 && kSpan + 16 <= kRingBytes, "a batch's first sequence is resident");
constexpr uint32_t kLenMax = 0x7fffff00u; /* length fields saturate here: far above any capacity */

/* ---- accessors: at most 4 bytes at any alignment ---- */

__device__ __forceinline__ uint32_t ld_u32(const uint8_t* p)
{
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

__device__ __forceinline__ void st_u32(uint8_t* p, uint32_t v)
{
  __builtin_memcpy(p, &v, 4);
}

/* Store the low `rem` bytes (rem >= 1; 4 or more stores all four) of v at p. */
__device__ __forceinline__ void st_upto4(uint8_t* p, uint32_t v, uint32_t rem)
{
  if (rem >= 4) {
    st_u32(p, v);
  } else {
    if (rem & 2) {
      const uint16_t h = (uint16_t)v;
      __builtin_memcpy(p, &h, 2);
      if (rem & 1) {
        p[2] = (uint8_t)(v >> 16);
      }
    } else {
      p[0] = (uint8_t)v;
    }
  }
}

struct alignas(16) Block16
{
  uint32_t w[4];
};

__device__ __forceinline__ Block16 ld_block_aligned(const uint8_t* p)
{
  Block16 v;
  __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), 16);
  return v;
}

__device__ __forceinline__ void st_block_aligned(uint8_t* p, const Block16& v)
{
  __builtin_memcpy(__builtin_assume_aligned(p, 16), &v, 16);
}

/* 16 bytes a lane through dword accesses: any alignment, global or LDS. */
__device__ __forceinline__ void copy16(uint8_t* d, const uint8_t* s)
{
  const uint32_t a = ld_u32(s), b = ld_u32(s + 4), c = ld_u32(s + 8), e = ld_u32(s + 12);
  st_u32(d, a);
  st_u32(d + 4, b);
  st_u32(d + 8, c);
  st_u32(d + 12, e);
}

/* ---- the stream as the decoder reads it ---- */

/* Through the staging ring. Resident: virtual positions [lo, hi), multiples of 16, hi - lo <= kRingBytes. */
struct RingSrc
{
  const uint8_t* base; /* the stream's address rounded down to 16 bytes */
  uint8_t* ring;
  uint32_t vbeg, vend; /* virtual positions of the stream's first byte and of its end */
  uint32_t lo, hi;

  __device__ __forceinline__ void init(const uint8_t* in, uint32_t in_len, uint8_t* shared)
  {
    const uint32_t a = (uint32_t)((uintptr_t)in & 15u);
    base = in - a;
    ring = shared;
    vbeg = a;
    vend = a + in_len;
    lo = 0;
    hi = 0;
  }

  /* Make [from & ~15, that + kRingBytes) resident, as far as the stream goes. `from` never moves backwards. Uniform. */
  __device__ __forceinline__ void ensure(uint32_t from)
  {
    lo = from & ~15u;
    if (hi < lo) {
      hi = lo;
    }
    const uint32_t vend16 = (vend + 15u) & ~15u;
    const uint32_t end = vend16 - lo < kRingBytes ? vend16 : lo + kRingBytes;
    if (hi >= end) {
      return;
    }
    wv::sync(); /* the lanes' reads of the blocks that go */
    const uint32_t blocks = (end - hi) >> 4;
    for (uint32_t i = (uint32_t)wv::lane_id(); i < blocks; i += 64) {
      const uint32_t b = hi + 16u * i;
      Block16 v;
      if (b >= vbeg && vend - b >= 16u) {
        v = ld_block_aligned(base + b);
      } else { /* the stream's first or last block: its own bytes only */
        v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
        for (uint32_t j = 0; j < 16; ++j) {
          const uint32_t p = b + j;
          if (p >= vbeg && p < vend) {
            v.w[j >> 2] |= (uint32_t)base[p] << (8 * (j & 3u));
          }
        }
      }
      const uint32_t slot = b & kRingMask;
      st_block_aligned(ring + slot, v);
      if (slot == 0) {
        st_block_aligned(ring + kRingBytes, v);
      }
    }
    hi = end;
    wv::sync();
  }

  /* the end of what may be looked at: ~0 when the rest of the stream is resident */
  __device__ __forceinline__ uint32_t limit() const { return hi >= vend ? ~0u : hi; }
  __device__ __forceinline__ uint32_t u8(uint32_t p) const { return ring[p & kRingMask]; }
  __device__ __forceinline__ uint32_t u32(uint32_t p) const { return ld_u32(ring + (p & kRingMask)); } /* (the mirror) */
  __device__ __forceinline__ uint32_t window_dword(uint32_t v) const
  {
    uint32_t x;
    __builtin_memcpy(&x, __builtin_assume_aligned(ring + (v & kRingMask), 4), 4);
    return x;
  }
};

/* Straight from memory (decompressed_size has no scratch area): virtual position = byte index + (address & 3). */
struct MemSrc
{
  const uint8_t* base;
  uint32_t vbeg, vend;

  __device__ __forceinline__ void init(const uint8_t* in, uint32_t in_len, uint8_t*)
  {
    const uint32_t a = (uint32_t)((uintptr_t)in & 3u);
    base = in - a;
    vbeg = a;
    vend = a + in_len;
  }
  __device__ __forceinline__ void ensure(uint32_t) {}
  __device__ __forceinline__ uint32_t limit() const { return ~0u; }
  __device__ __forceinline__ uint32_t u8(uint32_t p) const { return base[p]; }
  __device__ __forceinline__ uint32_t u32(uint32_t p) const { return ld_u32(base + p); }
  __device__ __forceinline__ uint32_t window_dword(uint32_t v) const
  {
    uint32_t x = 0;
    if (v >= vbeg && v < vend && vend - v >= 4u) {
      __builtin_memcpy(&x, __builtin_assume_aligned(base + v, 4), 4);
    } else {
      for (uint32_t j = 0; j < 4; ++j) {
        if (v + j >= vbeg && v + j < vend) {
          x |= (uint32_t)base[v + j] << (8 * j);
        }
      }
    }
    return x;
  }
};

/* ---- the token chase ---- */

/* For each of the 4 token candidates in a dword: distance to the next token if neither nibble needs length bytes
 * (token + literals + offset), else 0. */
__device__ __forceinline__ uint32_t fast_deltas(uint32_t cw)
{
  const uint32_t hi = (cw >> 4) & 0x0f0f0f0fu;
  const uint32_t lo = cw & 0x0f0f0f0fu;
  const uint32_t ext = (((hi + 0x01010101u) | (lo + 0x01010101u)) >> 4) & 0x01010101u;
  return (hi + 0x03030303u) & ~(ext * 0xffu);
}

/* 256 bytes of the stream in registers: lane l holds the aligned dword at virtual position wb + 4 l. */
struct Window
{
  uint32_t wb;
  uint32_t cw;
  uint32_t dv; /* fast_deltas(cw) */
};

template <class Src>
__device__ __forceinline__ void window_load(Window& w, const Src& src, uint32_t q)
{
  w.wb = q & ~3u;
  w.cw = src.window_dword(w.wb + 4u * (uint32_t)wv::lane_id());
  w.dv = fast_deltas(w.cw);
}

/* Byte at virtual position q (uniform). */
template <class Src>
__device__ __forceinline__ uint32_t window_byte(Window& w, const Src& src, uint32_t q)
{
  if (q - w.wb >= 256u) {
    window_load(w, src, q);
  }
  const uint32_t r = q - w.wb;
  return (wv::read_lane(w.cw, r >> 2) >> ((r & 3u) * 8u)) & 0xffu;
}

struct Batch
{
  uint32_t count; /* sequences recorded in lanes [0, count) of seqpos */
  bool ends;      /* the last of them is the block's last: literals only */
  bool big;       /* the sequence at q is not for a lane: a batch of its own */
};

/* Record the virtual positions of the next (up to 64) sequences from q on and test every field of them against the end
 * of the stream. The window is resident from q on (RingSrc::ensure(q) came first). Uniform. */
template <class Src>
__device__ __forceinline__ Batch chase(const Src& src, Window& w, uint32_t& q, uint32_t& seqpos, uint32_t& err)
{
  const uint32_t vend = src.vend;
  const uint32_t lim = src.limit();
  Batch b = {0u, false, false};
  window_load(w, src, q);
  while (b.count < 64u && q < vend) {
    if (lim != ~0u && lim - q < kSpan) { /* (lim = ~0: the rest is resident) */
      break;
    }
    if (q - w.wb >= 256u) {
      window_load(w, src, q);
    }
    const uint32_t r = q - w.wb;
    const uint32_t d = (wv::read_lane(w.dv, r >> 2) >> ((r & 3u) * 8u)) & 0xffu;
    uint32_t next;
    if (d != 0 && d < vend - q) {
      next = q + d; /* no length bytes, and a token follows the match */
    } else {
      const uint32_t t = window_byte(w, src, q);
      uint32_t pos = q + 1;
      uint32_t lit = t >> 4;
      if (lit == 15) {
        if (pos >= vend) {
          err |= kErrInput;
          return b;
        }
        const uint32_t e = window_byte(w, src, pos++);
        if (e == 255) {
          b.big = true;
          break;
        }
        lit += e;
      }
      if (lit > vend - pos) {
        err |= kErrInput;
        return b;
      }
      pos += lit;
      if (pos == vend) {
        b.ends = true; /* the last sequence: literals only */
      } else {
        if (vend - pos < 2) {
          err |= kErrInput;
          return b;
        }
        pos += 2;
        if ((t & 15u) == 15u) {
          uint32_t n = 0;
          for (;;) {
            if (pos >= vend) {
              err |= kErrInput;
              return b;
            }
            const uint32_t e = window_byte(w, src, pos++);
            if (e != 255) {
              break;
            }
            if (++n == kMatchExtMax) {
              b.big = true;
              break;
            }
          }
          if (b.big) {
            break;
          }
        }
        if (pos >= vend) { /* a token must follow every match */
          err |= kErrInput;
          return b;
        }
      }
      next = pos;
    }
    seqpos = wv::write_lane(seqpos, q, b.count);
    ++b.count;
    q = next;
  }
  return b;
}

/* The rest of a length field from virtual position pos on, 64 bytes a step (a byte a lane, one ballot for the first that
 * is not 255). Adds them to `sum`, saturating; returns the position behind the field, or vend + 1 when the stream ends
 * first. Uniform. */
template <class Src>
__device__ __forceinline__ uint32_t scan_length_bytes(Src& src, uint32_t pos, uint32_t& sum)
{
  const uint32_t lane = (uint32_t)wv::lane_id();
  const uint32_t vend = src.vend;
  for (;;) {
    if (pos >= vend) {
      return vend + 1;
    }
    src.ensure(pos);
    const bool inside = lane < vend - pos;
    const uint32_t b = inside ? src.u8(pos + lane) : 0u;
    const uint64_t stop = wv::ballot(b != 255u || !inside);
    if (stop) {
      const uint32_t n = wv::ctz64(stop);
      if (n >= vend - pos) {
        return vend + 1;
      }
      const uint32_t add = 255u * n + wv::read_lane(b, n);
      sum = sum + add < kLenMax ? sum + add : kLenMax;
      return pos + n + 1;
    }
    sum = sum + 255u * 64u < kLenMax ? sum + 255u * 64u : kLenMax;
    pos += 64;
  }
}

/* ---- the whole wave's copies ---- */

/* dst[0, len) = src[0, len), not overlapping; 16 bytes a lane, the last len % 16 a byte a lane. */
__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t len)
{
  const uint32_t lane = (uint32_t)wv::lane_id();
  const uint32_t body = len & ~15u;
  if ((((uintptr_t)dst | (uintptr_t)src) & 15u) == 0) {
    for (uint32_t i = lane * 16u; i < body; i += 1024u) {
      st_block_aligned(dst + i, ld_block_aligned(src + i));
    }
  } else {
    for (uint32_t i = lane * 16u; i < body; i += 1024u) {
      copy16(dst + i, src + i);
    }
  }
  if (lane < len - body) {
    dst[body + lane] = src[body + lane];
  }
}

/* d[i] = d[i - off], i in [0, len), byte-serial semantics (off < len replicates a pattern). The effective offset E stays
 * a multiple of off and doubles as the pattern grows, so that a step never reads a byte the same step writes. */
__device__ __forceinline__ void wave_match_copy(uint8_t* d, uint32_t off, uint32_t len)
{
  const uint32_t lane = (uint32_t)wv::lane_id();
  uint32_t done = 0;
  uint32_t E = off;
  while (done < len) {
    while (E < 1024u && 2u * E <= done + off) {
      E *= 2u;
    }
    const uint32_t rem = len - done;
    if (E >= 1024u && rem >= 1024u) {
      uint8_t* t = d + done + lane * 16u;
      copy16(t, t - E);
      done += 1024u;
    } else if (E >= 256u && rem >= 256u) {
      uint8_t* t = d + done + lane * 4u;
      st_u32(t, ld_u32(t - E));
      done += 256u;
    } else {
      uint32_t n = E < 64u ? E : 64u;
      n = n < rem ? n : rem;
      if (lane < n) {
        uint8_t* t = d + done + lane;
        *t = *(t - E);
      }
      done += n;
    }
    wv::sync();
  }
}

/* ---- one batch ---- */

struct Seq
{
  uint32_t lit_src; /* virtual position of the first literal */
  uint32_t lit_len;
  uint32_t match_off;
  uint32_t match_len; /* 0: the block's last sequence */
};

/* Lane k < count reads the fields of the sequence at p. The chase has tested them: nothing can be wrong here. */
template <class Src>
__device__ __forceinline__ void parse(const Src& src, uint32_t p, bool active, bool last, Seq& s)
{
  s.lit_src = 0;
  s.lit_len = 0;
  s.match_off = 0;
  s.match_len = 0;
  if (!active) {
    return;
  }
  const uint32_t t = src.u8(p);
  uint32_t pos = p + 1;
  uint32_t lit = t >> 4;
  if (lit == 15) {
    lit += src.u8(pos++);
  }
  s.lit_src = pos;
  s.lit_len = lit;
  pos += lit;
  if (last) {
    return;
  }
  s.match_off = src.u8(pos) | (src.u8(pos + 1) << 8);
  pos += 2;
  uint32_t m = t & 15u;
  if (m == 15) {
    uint32_t e;
    do {
      e = src.u8(pos++);
      m += e;
    } while (e == 255);
  }
  s.match_len = m + 4;
}

/* Execute the batch's sequences; lane k owns sequence k. `op`: output bytes in front of the batch. Returns the batch's
 * output size; sets err and copies nothing when the output does not fit or an offset is 0 or reaches in front of out. */
template <bool SIZE_ONLY, class Src>
__device__ __forceinline__ uint32_t execute_batch(
    const Src& src, const uint8_t* in, uint8_t* out, uint32_t out_cap, uint32_t op, const Seq& s, uint32_t& err)
{
  const uint32_t lane = (uint32_t)wv::lane_id();
  const uint32_t lit_len = s.lit_len;
  const uint32_t match_len = s.match_len;
  const uint32_t off = s.match_off;
  const uint32_t len = lit_len + match_len; /* at most 269 + 2 059 */
  const uint32_t incl = wv::scan_add_inclusive(len);
  const uint32_t total = wv::read_lane(incl, 63);
  if (SIZE_ONLY) {
    if (total > kMaxOutCap - op) {
      err |= kErrOutput;
      return 0;
    }
    return total;
  }
  const uint32_t lit_dst = op + incl - len; /* op <= out_cap <= 2^26: no wrap */
  const uint32_t match_dst = lit_dst + lit_len;
  {
    const bool bad_out = op + incl > out_cap;
    const bool bad_off = match_len != 0 && (off == 0 || off > match_dst);
    const uint64_t any_out = wv::ballot(bad_out);
    const uint64_t any_off = wv::ballot(bad_off);
    if (any_out | any_off) {
      err |= (any_out ? kErrOutput : 0u) | (any_off ? kErrOffset : 0u);
      return 0;
    }
  }

  /* ---- literals ---- */
  {
    const bool lit_lane = lit_len != 0 && lit_len <= kLitShort;
    const uint32_t max_lit = wv::reduce_max(lit_lane ? lit_len : 0u);
    uint8_t* dst = out + lit_dst;
    for (uint32_t i = 0; i < max_lit; i += 4) {
      if (lit_lane && i < lit_len) {
        st_upto4(dst + i, src.u32(s.lit_src + i), lit_len - i);
      }
    }
    for (uint64_t pending = wv::ballot(lit_len > kLitShort); pending; pending &= pending - 1) {
      const uint32_t j = wv::ctz64(pending);
      const uint32_t jsrc = wv::read_lane(s.lit_src, j);
      const uint32_t jlen = wv::read_lane(lit_len, j);
      const uint32_t jdst = wv::read_lane(lit_dst, j);
      wave_copy(out + jdst, in + (jsrc - src.vbeg), jlen);
    }
  }
  wv::sync();

  /* ---- matches, in rounds ---- */
  {
    const uint32_t match_src = match_dst - off; /* off <= match_dst: no wrap */
    const bool short_match = match_len != 0 && match_len <= kMatchShort;
    uint64_t pending = wv::ballot(match_len != 0);
    const uint64_t short_mask = wv::ballot(short_match);
    while (pending) {
      const uint32_t f = wv::ctz64(pending);
      const uint32_t hw = wv::read_lane(match_dst, f); /* every byte below hw is final */
      if (!((short_mask >> f) & 1)) {
        const uint32_t foff = wv::read_lane(off, f);
        const uint32_t flen = wv::read_lane(match_len, f);
        wave_match_copy(out + hw, foff, flen);
        pending &= pending - 1;
        continue;
      }
      const bool ready = short_match && ((pending >> lane) & 1) && (lane == f || match_src + match_len <= hw);
      const uint32_t max_len = wv::reduce_max(ready ? match_len : 0u);
      const uint8_t* from = out + match_src;
      uint8_t* dst = out + match_dst;
      /* offset 1, 2, 3: the pattern in a register, eight bytes of it; a dword of the copy is the pattern from phase
       * i % off on (i = 0, 4, 8 ...: the phase moves for offset 3 only) */
      uint64_t pattern = 0;
      uint32_t phase = 0;
      if (ready && off < 4) {
        const uint32_t p = ld_u32(from); /* from + 4 <= dst + 3 < dst + match_len */
        pattern = off == 1   ? (uint64_t)(p & 0xffu) * 0x0101010101010101ull
                  : off == 2 ? (uint64_t)(p & 0xffffu) * 0x0001000100010001ull
                             : (uint64_t)(p & 0xffffffu) * 0x0001000001000001ull;
      }
      for (uint32_t i = 0; i < max_len; i += 4) {
        if (ready && i < match_len) {
          const uint32_t v = off >= 4 ? ld_u32(from + i) : (uint32_t)(pattern >> (8 * phase));
          st_upto4(dst + i, v, match_len - i);
          if (off == 3) {
            phase = phase == 2 ? 0 : phase + 1;
          }
        }
      }
      wv::sync();
      pending &= ~wv::ballot(ready);
    }
  }
  return total;
}

/* The sequence at q whose lengths are not for a lane, by the whole wave. Returns false with err set when it is
 * malformed or does not fit. Uniform. */
template <bool SIZE_ONLY, class Src>
__device__ __forceinline__ bool big_sequence(
    Src& src, const uint8_t* in, uint8_t* out, uint32_t out_cap, uint32_t& q, uint32_t& op, uint32_t& err)
{
  const uint32_t vend = src.vend;
  const uint32_t cap = SIZE_ONLY ? kMaxOutCap : out_cap;
  src.ensure(q);
  const uint32_t t = wv::uniform(src.u8(q));
  uint32_t pos = q + 1;
  uint32_t lit = t >> 4;
  if (lit == 15) {
    pos = scan_length_bytes(src, pos, lit);
    if (pos > vend) {
      err |= kErrInput;
      return false;
    }
  }
  if (lit > vend - pos) {
    err |= kErrInput;
    return false;
  }
  if (lit > cap - op) {
    err |= kErrOutput;
    return false;
  }
  if (!SIZE_ONLY && lit != 0) {
    wave_copy(out + op, in + (pos - src.vbeg), lit);
    wv::sync();
  }
  op += lit;
  pos += lit;
  if (pos != vend) {
    if (vend - pos < 2) {
      err |= kErrInput;
      return false;
    }
    src.ensure(pos);
    const uint32_t off = wv::uniform(src.u8(pos) | (src.u8(pos + 1) << 8));
    pos += 2;
    uint32_t mlen = t & 15u;
    if (mlen == 15) {
      pos = scan_length_bytes(src, pos, mlen);
      if (pos > vend) {
        err |= kErrInput;
        return false;
      }
    }
    if (pos >= vend) { /* a token must follow every match */
      err |= kErrInput;
      return false;
    }
    mlen += 4;
    if (!SIZE_ONLY && (off == 0 || off > op)) {
      err |= kErrOffset;
      return false;
    }
    if (mlen > cap - op) {
      err |= kErrOutput;
      return false;
    }
    if (!SIZE_ONLY) {
      wave_match_copy(out + op, off, mlen);
    }
    op += mlen;
  }
  q = pos;
  return true;
}

/* Decode one block with the calling wave (SIZE_ONLY: add up what it decodes to, copy nothing, test no offset and no
 * capacity but kMaxOutCap). Returns the bytes produced; err != 0: refused, the return value is 0. */
template <bool SIZE_ONLY, class Src>
__device__ __forceinline__ uint32_t decode_block(
    const uint8_t* in, uint32_t in_len, uint8_t* out, uint32_t out_cap, uint8_t* shared, uint32_t& err)
{
  err = kErrNone;
  if (in_len == 0) {
    return 0; /* an empty block decodes to nothing */
  }
  const uint32_t lane = (uint32_t)wv::lane_id();
  Src src;
  src.init(in, in_len, shared);
  Window w;
  uint32_t q = src.vbeg;
  uint32_t op = 0;
  while (q < src.vend) {
    src.ensure(q);
    uint32_t seqpos = 0;
    const Batch b = chase(src, w, q, seqpos, err);
    if (err) {
      return 0;
    }
    if (b.count != 0) {
      Seq s;
      parse(src, seqpos, lane < b.count, b.ends && lane + 1 == b.count, s);
      op += execute_batch<SIZE_ONLY>(src, in, out, out_cap, op, s, err);
    } else if (b.big) {
      big_sequence<SIZE_ONLY>(src, in, out, out_cap, q, op, err);
    } else {
      err |= kErrInput; /* (not reached: a batch's first sequence is always resident) */
    }
    if (err) {
      return 0;
    }
  }
  return op;
}

} // namespace lz4
} // namespace detail
} // namespace device
} // namespace nvcomp
