/*
 * lz4/lz4_size.hip.h -- what an LZ4 block decodes to, for nvcompBatchedLZ4GetDecompressSizeAsync: an LZ4 block does not
 * say, so one wavefront walks the chunk's token chain and sums the lengths. Nothing is written.
 *   1. chase - the wave walks the token chain with wave-uniform (scalar) arithmetic over a 256-byte register window and
 *              records the start of up to 64 sequences;
 *   2. parse - lane k decodes the fields of sequence k and checks them against the end of the chunk;
 *   3. sum   - the batch's lengths are added up across the wave.
 * The decoders proper are in lz4_decode_window.hip.h.
 *
 * Block format (public LZ4 specification; checked against liblz4 in tests):
 *   token: hi nibble = literal length, lo nibble = match length - 4; a nibble
 *   of 15 is extended by following bytes (each added, 255 continues); literals;
 *   2-byte little-endian offset; match-length extension. The last sequence is
 *   literals only and ends exactly at the end of the chunk.
 */
#pragma once

#include "common/lz_common.hip.h"

namespace lz4 {

/* ---- 256-byte register window over the compressed stream ------------------
 * Lane l holds the aligned dword at "virtual position" wb + 4l, where virtual
 * position = byte index in the chunk + (chunk address & 3). A wave-uniform byte
 * is fetched with one v_readlane and scalar shifts: no memory round trip on the
 * token chain. */
struct InWindow
{
  const uint8_t* base; /* chunk pointer rounded down to 4 bytes (uniform) */
  uint32_t vbeg;       /* virtual position of the first chunk byte: chunk & 3 */
  uint32_t vend;       /* vbeg + chunk length */
  uint32_t wb;         /* virtual position of lane 0's dword (multiple of 4) */
  uint32_t cw;         /* this lane's dword */
};

__device__ __forceinline__ void window_init(InWindow& w, const uint8_t* in, uint32_t in_len)
{
  const uint32_t a = (uint32_t)((uintptr_t)in & 3u);
  w.base = in - a;
  w.vbeg = a;
  w.vend = a + in_len;
  w.wb = 0;
  w.cw = 0;
}

/* (Re)load the window so that it starts at the dword containing virtual
 * position q. Bytes outside the chunk read as zero and are never fetched. */
__device__ __forceinline__ void window_load(InWindow& w, uint32_t q)
{
  w.wb = q & ~3u;
  const uint32_t v = w.wb + 4u * (uint32_t)wave::lane_id();
  uint32_t x = 0;
  if (v >= w.vbeg && v + 4 <= w.vend) {
    x = *(const uint32_t*)(w.base + v);
  } else if (v + 4 > w.vbeg && v < w.vend) {
    for (uint32_t j = 0; j < 4; ++j) {
      if (v + j >= w.vbeg && v + j < w.vend) {
        x |= (uint32_t)w.base[v + j] << (8 * j);
      }
    }
  }
  w.cw = x;
}

__device__ __forceinline__ bool window_has(const InWindow& w, uint32_t q)
{
  return q - w.wb < 256u;
}

/* Byte at virtual position q (uniform; must be inside the window). */
__device__ __forceinline__ uint32_t window_byte(const InWindow& w, uint32_t q)
{
  const uint32_t r = q - w.wb;
  return (wave::read_lane(w.cw, r >> 2) >> ((r & 3u) * 8u)) & 0xffu;
}

/* ---- the token chase ------------------------------------------------------ */

/* For each of the 4 token candidates in a dword: distance to the next token if
 * neither nibble needs extension bytes (1 token + L literals + 2 offset), else 0. */
__device__ __forceinline__ uint32_t fast_deltas(uint32_t cw)
{
  const uint32_t hi = (cw >> 4) & 0x0f0f0f0fu;
  const uint32_t lo = cw & 0x0f0f0f0fu;
  const uint32_t ext = (((hi + 0x01010101u) | (lo + 0x01010101u)) >> 4) & 0x01010101u;
  return (hi + 0x03030303u) & ~(ext * 0xffu);
}

struct Chase
{
  InWindow w;
  uint32_t dv; /* fast_deltas of the window */
  uint32_t q;  /* virtual position of the next token (uniform) */
};

__device__ __forceinline__ void chase_reload(Chase& c, uint32_t q)
{
  window_load(c.w, q);
  c.dv = fast_deltas(c.w.cw);
}

__device__ __forceinline__ void chase_init(Chase& c, const uint8_t* in, uint32_t in_len)
{
  window_init(c.w, in, in_len);
  c.q = c.w.vbeg;
  chase_reload(c, c.q);
}

/* Next token position for a token whose lengths use extension bytes (uniform,
 * scalar walk over the register window). Any value >= vend ends the chase;
 * the lane-parallel parse decides whether that is the legal end of the block. */
__device__ __forceinline__ uint32_t chase_slow_next(Chase& c)
{
  const uint32_t vend = c.w.vend;
  const uint32_t t = window_byte(c.w, c.q);
  uint32_t pos = c.q + 1;
  uint32_t lit = t >> 4;
  if (lit == 15) {
    for (;;) {
      if (pos >= vend) {
        return vend + 1;
      }
      if (!window_has(c.w, pos)) {
        chase_reload(c, pos);
      }
      const uint32_t b = window_byte(c.w, pos);
      ++pos;
      lit += b;
      if (b != 255) {
        break;
      }
    }
  }
  if (lit >= vend - pos) { /* literals reach (or pass) the end: last sequence or overrun */
    return vend + 1;
  }
  pos += lit + 2;
  if ((t & 15u) == 15u) {
    for (;;) {
      if (pos >= vend) {
        return vend + 1;
      }
      if (!window_has(c.w, pos)) {
        chase_reload(c, pos);
      }
      const uint32_t b = window_byte(c.w, pos);
      ++pos;
      if (b != 255) {
        break;
      }
    }
  }
  return pos;
}

/* Record the virtual start positions of the next (up to 64) sequences:
 * lane k of seqpos <- start of sequence k. Returns the count. */
__device__ __forceinline__ uint32_t chase(Chase& c, uint32_t& seqpos)
{
  uint32_t k = 0;
  while (k < 64u && c.q < c.w.vend) {
    if (!window_has(c.w, c.q)) {
      chase_reload(c, c.q);
    }
    const uint32_t r = c.q - c.w.wb;
    const uint32_t d = (wave::read_lane(c.dv, r >> 2) >> ((r & 3u) * 8u)) & 0xffu;
    seqpos = wave::write_lane(seqpos, c.q, k);
    ++k;
    c.q = d ? c.q + d : chase_slow_next(c);
  }
  return k;
}

/* ---- one sequence --------------------------------------------------------- */

/* Lane-parallel field decode of the sequence whose token is at in[p]; the walker reads the two lengths. `bad`: the
 * sequence does not fit the chunk, or no token follows its match. */
__device__ __forceinline__ void parse(
    const uint8_t* __restrict__ in, uint32_t in_len, uint32_t p, bool active, lz::Seq& s, bool& bad)
{
  s.lit_src = 0;
  s.lit_len = 0;
  s.match_off = 0;
  s.match_len = 0;
  bad = false;
  if (!active) {
    return;
  }
  const uint32_t t = in[p];
  uint32_t pos = p + 1;
  uint32_t lit = t >> 4;
  if (lit == 15) {
    uint32_t b;
    do {
      if (pos >= in_len) {
        bad = true;
        return;
      }
      b = in[pos++];
      lit += b;
    } while (b == 255);
  }
  if (lit > in_len - pos) {
    bad = true;
    return;
  }
  s.lit_src = pos;
  s.lit_len = lit;
  pos += lit;
  if (pos == in_len) {
    return; /* last sequence: literals only */
  }
  if (in_len - pos < 2) {
    bad = true;
    return;
  }
  s.match_off = (uint32_t)in[pos] | ((uint32_t)in[pos + 1] << 8);
  pos += 2;
  uint32_t mlen = t & 15u;
  if (mlen == 15) {
    uint32_t b;
    do {
      if (pos >= in_len) {
        bad = true;
        return;
      }
      b = in[pos++];
      mlen += b;
    } while (b == 255);
  }
  if (mlen > 0x40000000u) {
    bad = true;
    return;
  }
  if (pos >= in_len) { /* a token must follow every match */
    bad = true;
    return;
  }
  s.match_len = mlen + 4;
}

/* What the chunk decodes to, by the calling wave; 0 and an error bit for a block that is malformed or too large. */
__device__ __forceinline__ uint32_t decoded_size(const uint8_t* __restrict__ in, uint32_t in_len, uint32_t& err)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  uint32_t op = 0;
  err = lz::kErrNone;
  if (in_len == 0) {
    return 0;
  }
  Chase c;
  chase_init(c, in, in_len);
  while (c.q < c.w.vend) {
    uint32_t seqpos = 0;
    const uint32_t count = chase(c, seqpos);
    lz::Seq s;
    bool bad;
    parse(in, in_len, seqpos - c.w.vbeg, lane < count, s, bad);
    if (wave::ballot(bad)) {
      err |= lz::kErrInput;
      return 0;
    }
    /* a hostile stream may claim lengths whose 32-bit sum wraps to a small bogus size: the batch is summed in two
     * 16-bit halves (64 x 65535 fits) and the total checked against the largest chunk any decoder here accepts */
    const uint32_t len = s.lit_len + s.match_len;
    const uint64_t batch = (uint64_t)wave::reduce_add(len & 0xffffu) + ((uint64_t)wave::reduce_add(len >> 16) << 16);
    if (batch + op > (1u << 26)) {
      err |= lz::kErrOutput;
      return 0;
    }
    op += (uint32_t)batch;
  }
  return op;
}

} // namespace lz4
