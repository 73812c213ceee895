/*
 * nvcomp/device/detail/lz4_encode_core.hpp -- the wave-level LZ4 block compressor behind nvcomp/device/lz4.hpp (gfx950,
 * CDNA4).
 *
 * Implementation detail; not an interface of its own. One full, converged wave64 compresses one chunk. It is the compact
 * version of the batched compressor's idea, written for a caller's kernel: a STEP covers 64 positions,
 * lane l at position ip + l, and a step begins where the last match ended.
 *
 *   probe     the word at the position, its hash, the table entry (position mod 65 536, two bytes) -> candidate; then the
 *             step's positions go into the table. A position also looks 1, 2, 4 and 8 bytes back (runs, typed columns):
 *             such a repeat wins over the table's candidate.
 *   verify    every candidate is compared by its bytes, its distance is 1 ... 65 535 and it lies at or behind the chunk's
 *             start: the table is NEVER cleared. What an earlier chunk, or anything else, left in the scratch area is a
 *             candidate that fails here; so is a position that aliases beyond 64 KiB (distance 65 536 reads as 0).
 *   measure   every hit by its own lane, a dword at a time, up to kCap bytes, and up to four bytes backwards.
 *   select    the scalar walk over the hit mask, greedy with one step of lazy evaluation; a match that reached kCap is
 *             measured to its end by the whole wave, 256 bytes a round.
 *   emit      the selected matches are compacted into lanes through a queue in the scratch area; sizes and output
 *             positions come from one DPP scan; a lane writes its own sequence (literal runs to 64 bytes, one length
 *             byte a field), the few others are written by the whole wave.
 *
 * Where the input lies decides how it is read (DirectSrc / StagedSrc): in LDS, every byte is read where it lies; in
 * global memory, the positions around the step come out of an image of kImageBytes in the scratch area, restaged every
 * 28 steps or so, and only candidates in front of the image, long literal runs and long matches go to memory.
 *
 * The chunk is read with accesses of at most 4 bytes that lie wholly inside it, `out` is written with accesses of at most
 * 4 bytes that lie wholly inside the written block: both may be LDS, at any alignment.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

/* angle brackets: the host emulation of the test suite puts its own versions of these first on the include path */
#include <nvcomp/device/detail/wave.hpp>
#include <nvcomp/device/detail/wave_ext.hpp>
#include <nvcomp/device/detail/wave_lz.hpp>
#include <nvcomp/device/detail/wave_lzc.hpp>

#include "nvcomp/device/detail/lz4_core.hpp" /* ld_u32, st_u32 */

namespace nvcomp {
namespace device {
namespace detail {
namespace lz4enc {

namespace wv = ::nvcomp::device::detail::wave;
using ::nvcomp::device::detail::lz4::ld_u32;
using ::nvcomp::device::detail::lz4::st_u32;

constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kMfLimit = 12;     /* the last match starts this far before the end */
constexpr uint32_t kLastLiterals = 5; /* and the last five bytes are literals */

constexpr uint32_t kStep = 64;          /* positions per step: one per lane */
constexpr uint32_t kHashBits = 12;
constexpr uint32_t kTableBytes = 2u << kHashBits; /* 4 096 entries of two bytes */
constexpr uint32_t kQueueBytes = 8 * 64;          /* the selected matches of a step: two dwords each */
constexpr uint32_t kImageBytes = 2048;
constexpr uint32_t kEncodeLds = kTableBytes + kQueueBytes + kImageBytes;
constexpr uint32_t kCap = 32;       /* per-lane match measurement; longer matches: the whole wave */
constexpr uint32_t kLaneLiterals = 64; /* a lane writes literal runs up to here itself */
constexpr uint32_t kBehind = kLaneLiterals + 8; /* what a step reads in front of its first position: those runs, 8 back */
constexpr uint32_t kAhead = kStep + kCap + 4;   /* and from it on */
static_assert(kBehind + kAhead + kStep <= kImageBytes, "an image serves more than one step");

__device__ __forceinline__ uint32_t hash(uint32_t v)
{
  return (v * 2654435761u) >> (32 - kHashBits);
}

/* ---- the chunk as the match finder reads it ---- */

/* The chunk lies in LDS: everything is read where it lies. */
struct DirectSrc
{
  const uint8_t* src;

  __device__ __forceinline__ void init(const uint8_t* in, uint32_t, uint8_t*) { src = in; }
  __device__ __forceinline__ void ensure(uint32_t) {}
  __device__ __forceinline__ uint32_t u8(uint32_t p) const { return src[p]; }
  __device__ __forceinline__ uint32_t u32(uint32_t p) const { return ld_u32(src + p); }
  __device__ __forceinline__ uint32_t cand_u32(uint32_t p) const { return ld_u32(src + p); }
};

/* The chunk lies in global memory: positions [lo, hi) are resident in the image. u8 / u32: resident positions only (what
 * a step reads around itself); cand_u32: any position below a resident one. */
struct StagedSrc
{
  const uint8_t* src;
  uint8_t* img;
  uint32_t n, lo, hi;

  __device__ __forceinline__ void init(const uint8_t* in, uint32_t n_, uint8_t* image)
  {
    src = in;
    img = image;
    n = n_;
    lo = 0;
    hi = 0;
  }

  /* [ip - kBehind, ip + kAhead) resident, as far as the chunk goes. Uniform. */
  __device__ __forceinline__ void ensure(uint32_t ip)
  {
    const uint32_t need_lo = ip > kBehind ? ip - kBehind : 0u;
    const uint32_t need_hi = n - ip > kAhead ? ip + kAhead : n;
    if (need_lo >= lo && need_hi <= hi) {
      return;
    }
    wv::sync(); /* the lanes' reads of what goes */
    lo = need_lo;
    hi = n - lo > kImageBytes ? lo + kImageBytes : n;
    const uint32_t len = hi - lo;
    for (uint32_t o = 4u * (uint32_t)wv::lane_id(); o < len; o += 256u) {
      if (o + 4u <= len) {
        st_u32(img + o, ld_u32(src + lo + o));
      } else { /* the chunk's last one to three bytes */
        for (uint32_t j = o; j < len; ++j) {
          img[j] = src[lo + j];
        }
      }
    }
    wv::sync();
  }

  __device__ __forceinline__ uint32_t u8(uint32_t p) const { return img[p - lo]; }
  __device__ __forceinline__ uint32_t u32(uint32_t p) const { return ld_u32(img + (p - lo)); }
  __device__ __forceinline__ uint32_t cand_u32(uint32_t p) const { return ld_u32(p >= lo ? img + (p - lo) : src + p); }
};

/* ---- whole-wave pieces ---- */

/* Length-extension bytes for value v (15 already subtracted): v / 255 + 1 bytes, all 255 but the last, v % 255. */
__device__ __forceinline__ uint32_t put_extension(uint8_t* dst, uint32_t v)
{
  const uint32_t count = v / 255u + 1u;
  for (uint32_t i = (uint32_t)wv::lane_id(); i < count; i += 64u) {
    dst[i] = i + 1u < count ? (uint8_t)255 : (uint8_t)(v % 255u);
  }
  return count;
}

/* One sequence written by the whole wave; match_len == 0: the final, literals-only one. Returns its size. */
__device__ __forceinline__ uint32_t emit_wave(uint8_t* dst, const uint8_t* lit, uint32_t lit_len, uint32_t offset, uint32_t match_len)
{
  const uint32_t lane = (uint32_t)wv::lane_id();
  const uint32_t ml = match_len ? match_len - kMinMatch : 0u;
  uint32_t pos = 1;
  if (lane == 0) {
    dst[0] = (uint8_t)(((lit_len < 15u ? lit_len : 15u) << 4) | (ml < 15u ? ml : 15u));
  }
  if (lit_len >= 15u) {
    pos += put_extension(dst + pos, lit_len - 15u);
  }
  for (uint32_t o = 4u * lane; o < lit_len; o += 256u) {
    if (o + 4u <= lit_len) {
      st_u32(dst + pos + o, ld_u32(lit + o));
    } else {
      for (uint32_t j = o; j < lit_len; ++j) {
        dst[pos + j] = lit[j];
      }
    }
  }
  pos += lit_len;
  if (match_len) {
    if (lane == 0) {
      dst[pos] = (uint8_t)(offset & 255u);
      dst[pos + 1] = (uint8_t)(offset >> 8);
    }
    pos += 2;
    if (ml >= 15u) {
      pos += put_extension(dst + pos, ml - 15u);
    }
  }
  return pos;
}

/* The match at p with its source at c (c < p), `have` bytes of it known: its length, at most end - p. 256 bytes a round. */
__device__ __forceinline__ uint32_t extend_wave(const uint8_t* src, uint32_t p, uint32_t c, uint32_t have, uint32_t end)
{
  const uint32_t lane = (uint32_t)wv::lane_id();
  for (;;) {
    const uint32_t q = p + have + 4u * lane;
    uint32_t same = 0;
    if (q + 4u <= end) {
      const uint32_t x = ld_u32(src + q) ^ ld_u32(src + (q - (p - c)));
      same = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
    } else {
      for (uint32_t j = q; j < end && src[j] == src[j - (p - c)]; ++j) {
        ++same;
      }
    }
    const uint64_t stop = wv::ballot(same < 4u);
    if (stop) {
      const uint32_t f = wv::ctz64(stop);
      return have + 4u * f + wv::read_lane(same, f);
    }
    have += 256u;
  }
}

/* ---- the compressor ---- */

/* Compresses in[0, n), n <= 16 MiB, into one LZ4 block at dst (at most n + n / 255 + 16 bytes); `scratch`: kEncodeLds
 * bytes, 16-byte aligned, whatever they hold. Returns the block's size, on every lane. */
template <class Src>
__device__ __forceinline__ uint32_t encode_block(const uint8_t* in, uint32_t n, uint8_t* dst, uint8_t* scratch)
{
  const uint32_t lane = (uint32_t)wv::lane_id();
  uint16_t* table = (uint16_t*)scratch;
  uint32_t* queue = (uint32_t*)(scratch + kTableBytes);
  uint32_t op = 0;
  uint32_t anchor = 0;
  if (n > kMfLimit) {
    Src s;
    s.init(in, n, scratch + kTableBytes + kQueueBytes);
    const uint32_t last_start = n - kMfLimit;
    const uint32_t match_end = n - kLastLiterals;
    uint32_t ip = 0;
    while (ip <= last_start) {
      s.ensure(ip);
      /* ---- probe ---- */
      const uint32_t pos = ip + lane;
      const bool valid = pos <= last_start;
      uint32_t w = 0, near = 0;
      if (valid) {
        w = s.u32(pos);
        near = pos >= 8u && s.u32(pos - 8u) == w ? 8u : 0u;
        near = pos >= 4u && s.u32(pos - 4u) == w ? 4u : near;
        near = pos >= 2u && s.u32(pos - 2u) == w ? 2u : near;
        near = pos >= 1u && s.u32(pos - 1u) == w ? 1u : near;
      }
      const uint32_t slot = hash(w);
      const uint32_t entry = table[slot];
      wv::sync(); /* every lane has looked before any lane's position goes in */
      if (valid) {
        table[slot] = (uint16_t)pos;
      }
      wv::sync();
      /* ---- verify: distance 1 ... 65 535 (0: the position's own low bits, 65 536 back or garbage), not in front of
       * the chunk, and the same word ---- */
      const uint32_t back = near ? near : (pos - entry) & 0xffffu;
      const uint32_t cand = pos - back;
      bool ok = valid && back != 0 && back <= pos;
      if (ok && near == 0) {
        ok = s.cand_u32(cand) == w;
      }
      /* ---- measure ---- */
      uint32_t len = 0;
      uint32_t grow = 0; /* the bytes in front of the position that stand in front of the candidate as well: at most 4 */
      if (ok) {
        if (cand >= 4u) {
          const uint32_t x = s.u32(pos - 4u) ^ s.cand_u32(cand - 4u);
          grow = x ? (uint32_t)__builtin_clz(x) >> 3 : 4u;
        }
        len = kMinMatch;
        while (len < kCap && pos + len < match_end) { /* (the dword ends inside the chunk: match_end + 4 <= n) */
          const uint32_t x = s.u32(pos + len) ^ s.cand_u32(cand + len);
          if (x) {
            len += (uint32_t)__builtin_ctz(x) >> 3;
            break;
          }
          len += 4u;
        }
        const uint32_t room = match_end - pos;
        len = len < room ? len : room;
      }
      /* ---- select: a match shorter than the one that starts at the next position is passed over ---- */
      uint32_t ahead = wv::shuffle(len, (lane + 1u) & 63u);
      ahead = lane == 63u ? 0u : ahead;
      const uint64_t eff = wv::ballot(len != 0 && !(len < kCap && ahead > len));
      uint64_t sel = 0;
      uint32_t cur = 0; /* position in the step behind the last selected match */
      for (uint64_t rest = eff; rest != 0;) {
        const uint32_t f = wv::ctz64(rest);
        uint32_t flen = wv::read_lane(len, f);
        if (flen >= kCap && ip + f + flen < match_end) {
          flen = extend_wave(in, ip + f, wv::read_lane(cand, f), flen, match_end);
          len = wv::write_lane(len, flen, f);
        }
        sel |= 1ull << f;
        cur = f + flen;
        rest = cur < 64u ? eff & (~0ull << cur) : 0ull;
      }
      if (sel != 0) {
        /* ---- emit: the selected matches, compacted into lanes ---- */
        const uint32_t n_sel = wv::popc64(sel);
        if ((sel >> lane) & 1ull) {
          const uint32_t at = wv::prefix_popc(sel);
          queue[2u * at] = lane | (grow << 6) | (back << 9);
          queue[2u * at + 1u] = len;
        }
        wv::sync();
        const bool mine = lane < n_sel;
        const uint32_t s0 = mine ? queue[2u * lane] : 0u;
        uint32_t my_len = mine ? queue[2u * lane + 1u] : 0u;
        const uint32_t mpos = ip + (s0 & 63u);
        const uint32_t offset = s0 >> 9;
        /* a lane's literal run starts where the match of the lane below ends (the first one's: at the anchor) */
        uint32_t prev_end = wv::prev_lane(mpos + my_len);
        prev_end = lane == 0 ? anchor : prev_end;
        uint32_t lit_len = mine ? mpos - prev_end : 0u;
        {
          /* a match found a few positions late (a table entry overwritten, a longer match one position on) takes the
           * bytes in front of it back, never into the match before */
          const uint32_t g = (s0 >> 6) & 7u;
          const uint32_t b = g < lit_len ? g : lit_len;
          lit_len -= b;
          my_len += b;
        }
        const uint32_t ml = my_len - kMinMatch;
        const uint32_t size = mine ? 1u + (lit_len >= 15u ? (lit_len - 15u) / 255u + 1u : 0u) + lit_len + 2u +
                                         (ml >= 15u ? (ml - 15u) / 255u + 1u : 0u)
                                   : 0u;
        const uint32_t incl = wv::scan_add_inclusive(size);
        const uint32_t total = wv::read_lane(incl, 63);
        const bool small = mine && lit_len <= kLaneLiterals && ml < 15u + 255u;
        uint64_t big = wv::ballot(mine && !small);
        if (small) {
          uint8_t* d = dst + op + (incl - size);
          *d++ = (uint8_t)(((lit_len < 15u ? lit_len : 15u) << 4) | (ml < 15u ? ml : 15u));
          if (lit_len >= 15u) {
            *d++ = (uint8_t)(lit_len - 15u);
          }
          uint32_t i = 0;
          for (; i + 4u <= lit_len; i += 4u) {
            st_u32(d + i, s.u32(prev_end + i));
          }
          for (; i < lit_len; ++i) {
            d[i] = (uint8_t)s.u8(prev_end + i);
          }
          d += lit_len;
          d[0] = (uint8_t)(offset & 255u);
          d[1] = (uint8_t)(offset >> 8);
          if (ml >= 15u) {
            d[2] = (uint8_t)(ml - 15u);
          }
        }
        /* the few sequences a single lane cannot write (a long literal run after steps without a match, a long match) */
        while (big) {
          const uint32_t j = wv::ctz64(big);
          big &= big - 1;
          emit_wave(dst + op + wv::read_lane(incl - size, j), in + wv::read_lane(prev_end, j), wv::read_lane(lit_len, j),
                    wv::read_lane(offset, j), wv::read_lane(my_len, j));
        }
        op += total;
        anchor = ip + cur;
      }
      ip += cur > kStep ? cur : kStep;
    }
  }
  op += emit_wave(dst + op, in + anchor, n - anchor, 0, 0);
  wv::sync(); /* the block is the caller's to read, across lanes; the scratch area is free */
  return op;
}

} // namespace lz4enc
} // namespace detail
} // namespace device
} // namespace nvcomp
