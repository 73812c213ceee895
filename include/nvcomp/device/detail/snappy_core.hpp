/*
 * nvcomp/device/detail/snappy_core.hpp -- the wave-level Snappy raw-format decoder behind nvcomp/device/snappy.hpp (gfx950,
 * CDNA4).
 *
 * Implementation detail; not an interface of its own. One full, converged wave64 decodes one stream. The compact version
 * of the batched decoder's idea, written for a caller's kernel: no persistent loop, no output window, no
 * run executor. The format-independent parts are those of lz4_core.hpp, used where they stand: the staging ring
 * (RingSrc), the 256-byte register window of the chase, the accessors and the whole wave's copies.
 *
 *   preamble  the varint32 declared length, out of the ring. It is the output limit: elements must produce exactly that
 *             many bytes, whatever the capacity is.
 *   chase     wave-uniform: the element chain is walked over the register window, up to 64 TOKENS a batch. A token is a
 *             copy element, or a literal element together with the copy element behind it (literal elements of at most
 *             kLitShort bytes, as the batched decoder fuses them: otherwise trains of copies would halve the batch), or a
 *             literal element alone. Every field is tested against the end of the stream and every length against the
 *             declared length HERE, so that a malformed or overrunning stream is refused before anything of the batch is
 *             copied -- nothing is ever written at or behind the declared length.
 *   parse     lane k reads the fields of token k from the ring.
 *   trains    a copy that continues the copy before it (same offset, no literal between) is the same match going on --
 *             how the format spells a long match, a run, a typed column. The head of a train takes the whole length, the
 *             followers become empty: chains of dependent 64-byte copies become one long match.
 *   scan      a DPP prefix sum gives every lane its output position; offsets are tested by lane arithmetic.
 *   literals  elements of up to kLitShort bytes by their own lane out of the ring, longer ones by the whole wave from the
 *             stream, 16 bytes a lane.
 *   matches   in rounds, as in lz4_core.hpp: a lane copies once every byte of its source lies below the oldest pending
 *             match (or it is that match). offset < 4 replicates a pattern held in a register (its bytes are read one by
 *             one: a copy may be 1 byte long), offset >= 4 copies dwords front to back; merged trains above kMatchShort
 *             bytes are copied by the whole wave, the pattern doubling as it grows.
 *
 * `out` and the stream are reached with accesses of at most 4 bytes at any alignment, or 16 bytes at 16-byte aligned
 * addresses: both may be LDS.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nvcomp/device/detail/lz4_core.hpp" /* RingSrc, Window, ld_u32 / st_upto4, wave_copy, wave_match_copy */

namespace nvcomp {
namespace device {
namespace detail {
namespace snappy {

namespace wv = ::nvcomp::device::detail::wave;
namespace lzc = ::nvcomp::device::detail::lz4;

using lzc::kErrInput;
using lzc::kErrNone;
using lzc::kErrOffset;
using lzc::kErrOutput;
using lzc::RingSrc;

constexpr uint32_t kRingBytes = lzc::kRingBytes;
constexpr uint32_t kDecodeLds = lzc::kDecodeLds;
constexpr uint32_t kMaxOutCap = lzc::kMaxOutCap; /* the batched decoder's: a larger capacity counts as this */

constexpr uint32_t kLitShort = 32;   /* literal elements up to here are copied by their own lane, and take the copy behind them */
constexpr uint32_t kMatchShort = 64; /* a copy element; only merged trains are longer */
/* what the ring must hold of a token: tag, four length bytes, kLitShort literals, the copy's tag and four offset bytes */
constexpr uint32_t kSpan = 48;
static_assert(kSpan >= 1 + 4 + kLitShort + 1 + 4 && kSpan + 16 <= kRingBytes, "a batch's first token is resident");

/* The varint32 preamble straight from memory, by every lane alike: false when the stream ends inside it or it does not fit
 * 32 bits (a fifth byte above 15 or with its continuation bit). What nvcompBatchedSnappyGetDecompressSizeAsync accepts. */
__device__ __forceinline__ bool preamble(const uint8_t* in, uint32_t in_len, uint32_t& total)
{
  total = 0;
  for (uint32_t i = 0; i < 5 && i < in_len; ++i) {
    const uint32_t b = wv::uniform(in[i]);
    total |= (b & 127u) << (7 * i);
    if (!(b & 128u)) {
      return !(i == 4 && b > 15u);
    }
  }
  return false;
}

/* ---- the element chase ---- */

/* Record the virtual positions of the next (up to 64) tokens from q on; test every field of them against the end of the
 * stream and every length against what the declared length leaves (op: produced so far, advanced). The ring is resident
 * from q on (RingSrc::ensure(q) came first). Uniform. */
__device__ __forceinline__ uint32_t chase(
    const RingSrc& src, lzc::Window& w, uint32_t& q, uint32_t& op, uint32_t limit, uint32_t& seqpos, uint32_t& err)
{
  const uint32_t vend = src.vend;
  const uint32_t lim = src.limit();
  uint32_t count = 0;
  lzc::window_load(w, src, q);
  while (count < 64u && q < vend) {
    if (lim != ~0u && q + kSpan > lim) { /* (lim = ~0: the rest is resident) */
      break;
    }
    uint32_t t = lzc::window_byte(w, src, q);
    uint32_t kind = t & 3u;
    uint32_t pos = q + 1;
    bool copy = true;
    if (kind == 0) {
      uint32_t len = t >> 2; /* length - 1 */
      if (len >= 60u) {
        const uint32_t nb = len - 59u;
        if (vend - pos < nb) {
          err |= kErrInput;
          return 0;
        }
        len = 0;
        for (uint32_t i = 0; i < nb; ++i) {
          len |= lzc::window_byte(w, src, pos + i) << (8u * i);
        }
        pos += nb;
      }
      if (len >= vend - pos) {
        err |= kErrInput;
        return 0;
      }
      len += 1;
      if (len > limit - op) {
        err |= kErrOutput;
        return 0;
      }
      op += len;
      pos += len;
      copy = false;
      if (len <= kLitShort && pos < vend) {
        t = lzc::window_byte(w, src, pos);
        kind = t & 3u;
        if (kind != 0) {
          copy = true;
          ++pos;
        }
      }
    }
    if (copy) {
      const uint32_t need = kind == 3u ? 4u : kind;
      if (vend - pos < need) {
        err |= kErrInput;
        return 0;
      }
      pos += need;
      const uint32_t mlen = kind == 1u ? 4u + ((t >> 2) & 7u) : 1u + (t >> 2);
      if (mlen > limit - op) {
        err |= kErrOutput;
        return 0;
      }
      op += mlen;
    }
    seqpos = wv::write_lane(seqpos, q, count);
    ++count;
    q = pos;
  }
  return count;
}

/* ---- one batch ---- */

struct Seq
{
  uint32_t lit_src; /* virtual position of the first literal */
  uint32_t lit_len;
  uint32_t match_off;
  uint32_t match_len; /* 0: a literal element alone */
};

/* Lane k < count reads the fields of the token at p, by the chase's rule. The chase has tested them against the stream's
 * end: nothing can be wrong here but an offset. */
__device__ __forceinline__ void parse(const RingSrc& src, uint32_t p, bool active, Seq& s)
{
  s.lit_src = 0;
  s.lit_len = 0;
  s.match_off = 0;
  s.match_len = 0;
  if (!active) {
    return;
  }
  uint32_t t = src.u8(p);
  uint32_t kind = t & 3u;
  uint32_t pos = p + 1;
  if (kind == 0) {
    uint32_t len = t >> 2;
    if (len >= 60u) {
      const uint32_t nb = len - 59u;
      const uint32_t f = src.u32(pos);
      len = nb == 4u ? f : f & ((1u << (8u * nb)) - 1u);
      pos += nb;
    }
    len += 1;
    s.lit_src = pos;
    s.lit_len = len;
    pos += len;
    if (len > kLitShort || pos >= src.vend) {
      return;
    }
    t = src.u8(pos);
    kind = t & 3u;
    if (kind == 0) {
      return;
    }
    ++pos;
  }
  const uint32_t f = src.u32(pos); /* (the ring: bytes behind the field are read and dropped) */
  s.match_len = kind == 1u ? 4u + ((t >> 2) & 7u) : 1u + (t >> 2);
  s.match_off = kind == 1u ? ((t >> 5) << 8) | (f & 0xffu) : kind == 2u ? f & 0xffffu : f;
}

/* A copy that continues the copy before it (same offset, nothing in between) is the same match going on. The first lane
 * of a train takes the whole length, the others become empty tokens. */
__device__ __forceinline__ void merge_trains(Seq& s)
{
  const uint32_t lane = (uint32_t)wv::lane_id();
  /* lanes behind the batch hold empty tokens, lane 0's neighbour reads as one */
  const uint32_t prev_off = wv::prev_lane(s.match_off);
  const uint32_t prev_len = wv::prev_lane(s.match_len);
  const bool cont = s.lit_len == 0 && s.match_len != 0 && prev_len != 0 && prev_off == s.match_off;
  const uint64_t train = wv::ballot(cont);
  if (train) {
    const uint32_t incl = wv::scan_add_inclusive(s.match_len);
    const uint64_t above = lane < 63u ? train >> (lane + 1u) : 0ull;
    const uint32_t followers = wv::ctz64(~above); /* continuing lanes right behind this one */
    const uint32_t end_incl = wv::shuffle(incl, (lane + followers) & 63u);
    if (cont) {
      s.match_len = 0;
      s.match_off = 0;
    } else if (followers) {
      s.match_len += end_incl - incl;
    }
  }
}

/* Execute the batch's tokens; lane k owns token k. `op`: output bytes in front of the batch; the chase has made sure that
 * the batch ends at or in front of the declared length. Sets err and copies nothing when an offset is 0 or reaches in
 * front of out. */
__device__ __forceinline__ void execute_batch(
    const RingSrc& src, const uint8_t* in, uint8_t* out, uint32_t op, Seq& s, uint32_t& err)
{
  using lzc::ld_u32;
  using lzc::st_upto4;
  const uint32_t lane = (uint32_t)wv::lane_id();
  const uint32_t lit_len = s.lit_len;
  const uint32_t len0 = lit_len + s.match_len; /* the sum over the batch is at most the declared length: no wrap */
  const uint32_t incl = wv::scan_add_inclusive(len0);
  const uint32_t lit_dst = op + incl - len0;
  const uint32_t match_dst = lit_dst + lit_len;
  if (wv::ballot(s.match_len != 0 && (s.match_off == 0 || s.match_off > match_dst))) {
    err |= kErrOffset;
    return;
  }
  merge_trains(s); /* (a train's head passed the offset test: so do its followers) */
  const uint32_t match_len = s.match_len;
  const uint32_t off = s.match_off;

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
      lzc::wave_copy(out + jdst, in + (jsrc - src.vbeg), jlen);
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
        lzc::wave_match_copy(out + hw, foff, flen);
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
        uint32_t p = from[0];
        if (off > 1) {
          p |= (uint32_t)from[1] << 8;
        }
        if (off > 2) {
          p |= (uint32_t)from[2] << 16;
        }
        pattern = off == 1   ? (uint64_t)p * 0x0101010101010101ull
                  : off == 2 ? (uint64_t)p * 0x0001000100010001ull
                             : (uint64_t)p * 0x0001000001000001ull;
      }
      for (uint32_t i = 0; i < max_len; i += 4) {
        if (ready && i < match_len) {
          /* off >= 4: the dword ends at or in front of dst + i, and in front of the copy's end */
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
}

/* Decode one stream with the calling wave. Returns the bytes produced; err != 0: refused, the return value is 0.
 * out_cap <= kMaxOutCap, in_len <= 2^32 - 65. */
__device__ __forceinline__ uint32_t decode_block(
    const uint8_t* in, uint32_t in_len, uint8_t* out, uint32_t out_cap, uint8_t* shared, uint32_t& err)
{
  err = kErrNone;
  if (in_len == 0) {
    err = kErrInput; /* no preamble */
    return 0;
  }
  const uint32_t lane = (uint32_t)wv::lane_id();
  RingSrc src;
  src.init(in, in_len, shared);
  src.ensure(src.vbeg);
  uint32_t q = src.vbeg;
  uint32_t total = 0;
  {
    bool ok = false;
    for (uint32_t shift = 0; shift <= 28u && q < src.vend; shift += 7u) {
      const uint32_t b = wv::uniform(src.u8(q));
      ++q;
      total |= (b & 127u) << shift;
      if (!(b & 128u)) {
        ok = !(shift == 28u && b > 15u);
        break;
      }
    }
    if (!ok) {
      err = kErrInput;
      return 0;
    }
  }
  if (total > out_cap) {
    err = kErrOutput;
    return 0;
  }
  lzc::Window w;
  uint32_t op = 0;
  while (q < src.vend) {
    src.ensure(q);
    uint32_t seqpos = 0;
    const uint32_t before = op;
    const uint32_t count = chase(src, w, q, op, total, seqpos, err);
    if (err) {
      return 0;
    }
    if (count == 0) {
      err |= kErrInput; /* (not reached: a batch's first token is always resident) */
      return 0;
    }
    Seq s;
    parse(src, seqpos, lane < count, s);
    execute_batch(src, in, out, before, s, err);
    if (err) {
      return 0;
    }
  }
  if (op != total) { /* the elements end short of the declared length */
    err = kErrInput;
    return 0;
  }
  return op;
}

} // namespace snappy
} // namespace detail
} // namespace device
} // namespace nvcomp
