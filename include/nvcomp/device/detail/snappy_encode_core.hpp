/*
 * nvcomp/device/detail/snappy_encode_core.hpp -- the wave-level Snappy raw-format compressor behind
 * nvcomp/device/snappy.hpp (gfx950, CDNA4).
 *
 * Implementation detail; not an interface of its own. One full, converged wave64 compresses one chunk. The match finder is
 * the step of lz4_encode_core.hpp -- probe, verify, measure, select over 64 positions, lane l at position ip + l, the hash
 * table never cleared, the chunk read through DirectSrc (LDS) or StagedSrc (global memory) -- without LZ4's end-of-block
 * rules: a match may start four bytes before the chunk's end and run to its last byte. What is new is the emitter:
 *
 *   preamble  the chunk's size as a varint32.
 *   literal   tag with the length - 1 (up to 60 bytes), or tag 60 .. 63 and the length - 1 in one to four bytes: always the
 *             shortest field.
 *   copy      copy-1 (two bytes) for a length of 4 .. 11 at an offset below 2 048, copy-2 (three bytes) otherwise; never
 *             copy-4: offsets are 1 .. 65 535. A match above 64 bytes is cut into pieces of 64 while 68 or more remain, one
 *             of 60 if more than 64 remain, and the rest: no piece is shorter than 4.
 *   emit      the selected matches are compacted into lanes through a queue in the scratch area; sizes and output
 *             positions come from one DPP scan; a lane writes its own literal element (to 64 bytes) and its copy pieces
 *             (matches to kLaneMatch bytes), the few others are written by the whole wave, a piece a lane.
 *
 * The chunk is read with accesses of at most 4 bytes that lie wholly inside it, `out` is written with accesses of at most
 * 4 bytes that lie wholly inside the written block: both may be LDS, at any alignment.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nvcomp/device/detail/lz4_encode_core.hpp" /* DirectSrc, StagedSrc, hash, extend_wave, the table's geometry */

namespace nvcomp {
namespace device {
namespace detail {
namespace snappyenc {

namespace wv = ::nvcomp::device::detail::wave;
namespace lze = ::nvcomp::device::detail::lz4enc;
using ::nvcomp::device::detail::lz4::ld_u32;
using ::nvcomp::device::detail::lz4::st_u32;
using lze::DirectSrc;
using lze::StagedSrc;

constexpr uint32_t kMinMatch = 4;
constexpr uint32_t kStep = lze::kStep;
constexpr uint32_t kTableBytes = lze::kTableBytes;
constexpr uint32_t kQueueBytes = lze::kQueueBytes;
constexpr uint32_t kEncodeLds = lze::kEncodeLds;
constexpr uint32_t kCap = lze::kCap;
constexpr uint32_t kLaneLiterals = lze::kLaneLiterals;
constexpr uint32_t kLaneMatch = 64 * 4; /* a lane writes up to four or five copy pieces itself */
constexpr uint32_t kMinProbed = 8;      /* shorter chunks are literals only, as the batched compressor's */
static_assert(lze::kAhead >= kStep + kCap + 4 && lze::kBehind >= kLaneLiterals + 8, "what a step reads is resident");

/* A byte of a candidate: any position below a resident one. */
__device__ __forceinline__ uint32_t cand_u8(const DirectSrc& s, uint32_t p)
{
  return s.src[p];
}
__device__ __forceinline__ uint32_t cand_u8(const StagedSrc& s, uint32_t p)
{
  return p >= s.lo ? s.img[p - s.lo] : s.src[p];
}

/* ---- sizes ---- */

__device__ __forceinline__ uint32_t literal_header(uint32_t len) /* len >= 1 */
{
  const uint32_t m = len - 1u;
  return 1u + (m < 60u ? 0u : m < (1u << 8) ? 1u : m < (1u << 16) ? 2u : m < (1u << 24) ? 3u : 4u);
}

__device__ __forceinline__ uint32_t piece_size(uint32_t offset, uint32_t len)
{
  return len >= 4u && len < 12u && offset < 2048u ? 2u : 3u;
}

__device__ __forceinline__ uint32_t copy_size(uint32_t offset, uint32_t len)
{
  uint32_t sz = 0;
  if (len >= 68u) {
    const uint32_t full = (len - 68u) / 64u + 1u;
    sz = 3u * full;
    len -= 64u * full;
  }
  if (len > 64u) {
    sz += 3u;
    len -= 60u;
  }
  return sz + piece_size(offset, len);
}

/* ---- one lane's pieces ---- */

__device__ __forceinline__ uint32_t put_literal_header(uint8_t* d, uint32_t len) /* len >= 1; returns its size */
{
  const uint32_t m = len - 1u;
  if (m < 60u) {
    d[0] = (uint8_t)(m << 2);
    return 1;
  }
  const uint32_t nb = m < (1u << 8) ? 1u : m < (1u << 16) ? 2u : m < (1u << 24) ? 3u : 4u;
  d[0] = (uint8_t)((59u + nb) << 2);
  for (uint32_t i = 0; i < nb; ++i) {
    d[1u + i] = (uint8_t)(m >> (8u * i));
  }
  return 1u + nb;
}

__device__ __forceinline__ uint32_t put_piece(uint8_t* d, uint32_t offset, uint32_t len) /* len 1 .. 64 */
{
  if (len >= 4u && len < 12u && offset < 2048u) {
    d[0] = (uint8_t)(1u | ((len - 4u) << 2) | ((offset >> 8) << 5));
    d[1] = (uint8_t)(offset & 255u);
    return 2;
  }
  d[0] = (uint8_t)(2u | ((len - 1u) << 2));
  d[1] = (uint8_t)(offset & 255u);
  d[2] = (uint8_t)(offset >> 8);
  return 3;
}

/* ---- whole-wave pieces ---- */

/* A literal element of any length by the whole wave (len == 0: nothing). Returns its size. */
__device__ __forceinline__ uint32_t emit_literal_wave(uint8_t* dst, const uint8_t* lit, uint32_t len)
{
  if (len == 0) {
    return 0;
  }
  const uint32_t lane = (uint32_t)wv::lane_id();
  const uint32_t hdr = literal_header(len);
  if (lane == 0) {
    put_literal_header(dst, len);
  }
  for (uint32_t o = 4u * lane; o < len; o += 256u) {
    if (o + 4u <= len) {
      st_u32(dst + hdr + o, ld_u32(lit + o));
    } else {
      for (uint32_t j = o; j < len; ++j) {
        dst[hdr + j] = lit[j];
      }
    }
  }
  return hdr + len;
}

/* A match of any length as copy elements, a piece a lane. Returns their size. */
__device__ __forceinline__ uint32_t emit_copy_wave(uint8_t* dst, uint32_t offset, uint32_t len)
{
  const uint32_t lane = (uint32_t)wv::lane_id();
  uint32_t pos = 0;
  if (len >= 68u) {
    const uint32_t full = (len - 68u) / 64u + 1u;
    for (uint32_t i = lane; i < full; i += 64u) {
      put_piece(dst + 3u * i, offset, 64u);
    }
    pos = 3u * full;
    len -= 64u * full;
  }
  if (len > 64u) {
    if (lane == 0) {
      put_piece(dst + pos, offset, 60u);
    }
    pos += 3u;
    len -= 60u;
  }
  if (lane == 0) {
    put_piece(dst + pos, offset, len);
  }
  return pos + piece_size(offset, len);
}

/* ---- the compressor ---- */

/* Compresses in[0, n), n <= 16 MiB, into one Snappy raw-format stream at dst (at most 32 + n + n / 6 bytes); `scratch`:
 * kEncodeLds bytes, 16-byte aligned, whatever they hold. Returns the stream's size, on every lane. */
template <class Src>
__device__ __forceinline__ uint32_t encode_block(const uint8_t* in, uint32_t n, uint8_t* dst, uint8_t* scratch)
{
  const uint32_t lane = (uint32_t)wv::lane_id();
  uint16_t* table = (uint16_t*)scratch;
  uint32_t* queue = (uint32_t*)(scratch + kTableBytes);
  uint32_t op = 0;
  { /* the preamble */
    uint32_t v = n;
    do {
      if (lane == 0) {
        dst[op] = (uint8_t)((v & 127u) | (v >= 128u ? 128u : 0u));
      }
      v >>= 7;
      ++op;
    } while (v);
  }
  uint32_t anchor = 0;
  if (n >= kMinProbed) {
    Src s;
    s.init(in, n, scratch + kTableBytes + kQueueBytes);
    const uint32_t last_start = n - kMinMatch;
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
      const uint32_t slot = lze::hash(w);
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
        bool open = true;
        while (len < kCap && pos + len + 4u <= n) { /* dwords that end inside the chunk */
          const uint32_t x = s.u32(pos + len) ^ s.cand_u32(cand + len);
          if (x) {
            len += (uint32_t)__builtin_ctz(x) >> 3;
            open = false;
            break;
          }
          len += 4u;
        }
        if (open) { /* the chunk's last one to three bytes */
          while (len < kCap && pos + len < n && s.u8(pos + len) == cand_u8(s, cand + len)) {
            ++len;
          }
        }
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
        if (flen >= kCap && ip + f + flen < n) {
          flen = lze::extend_wave(in, ip + f, wv::read_lane(cand, f), flen, n);
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
        const uint32_t size = mine ? (lit_len ? literal_header(lit_len) + lit_len : 0u) + copy_size(offset, my_len) : 0u;
        const uint32_t incl = wv::scan_add_inclusive(size);
        const uint32_t total = wv::read_lane(incl, 63);
        const bool small = mine && lit_len <= kLaneLiterals && my_len <= kLaneMatch;
        uint64_t big = wv::ballot(mine && !small);
        if (small) {
          uint8_t* d = dst + op + (incl - size);
          if (lit_len) {
            d += put_literal_header(d, lit_len);
            uint32_t i = 0;
            for (; i + 4u <= lit_len; i += 4u) {
              st_u32(d + i, s.u32(prev_end + i));
            }
            for (; i < lit_len; ++i) {
              d[i] = (uint8_t)s.u8(prev_end + i);
            }
            d += lit_len;
          }
          uint32_t rest = my_len;
          while (rest >= 68u) {
            d += put_piece(d, offset, 64u);
            rest -= 64u;
          }
          if (rest > 64u) {
            d += put_piece(d, offset, 60u);
            rest -= 60u;
          }
          put_piece(d, offset, rest);
        }
        /* the few sequences a single lane cannot write (a long literal run after steps without a match, a long match) */
        while (big) {
          const uint32_t j = wv::ctz64(big);
          big &= big - 1;
          uint8_t* d = dst + op + wv::read_lane(incl - size, j);
          const uint32_t jlit = wv::read_lane(lit_len, j);
          d += emit_literal_wave(d, in + wv::read_lane(prev_end, j), jlit);
          emit_copy_wave(d, wv::read_lane(offset, j), wv::read_lane(my_len, j));
        }
        op += total;
        anchor = ip + cur;
      }
      ip += cur > kStep ? cur : kStep;
    }
  }
  op += emit_literal_wave(dst + op, in + anchor, n - anchor);
  wv::sync(); /* the stream is the caller's to read, across lanes; the scratch area is free */
  return op;
}

} // namespace snappyenc
} // namespace detail
} // namespace device
} // namespace nvcomp
