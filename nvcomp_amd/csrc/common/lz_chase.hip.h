/*
 * common/lz_chase.hip.h -- the token chase by pointer doubling: where the next 64 sequences of a stream start.
 */
#pragma once

#include "common/lz_ring.hip.h"

namespace lzw {

/* ---- token chase by pointer doubling ------------------------------------------
 *
 * The format-specific part is a functor `delta(r, p)`: the distance from a (speculative)
 * token at virtual position p to the token after it, or kUnknown when that cannot be
 * told from the resident bytes. For a window of 256 positions the wave builds, in LDS,
 * byte tables J_i[p] = distance from p to the 2^i-th token after p (255 = leaves the
 * window / unknown), i = 0..5, by five doubling rounds J_i[p] = J_{i-1}[p] + J_{i-1}[p +
 * J_{i-1}[p]]. Lane n then finds the n-th token after any start position by following the
 * set bits of n through the tables: 64 token positions for 6 dependent LDS reads, instead of
 * 64 dependent scalar steps. The tables do not depend on the start, so a window is built
 * once however many batches it feeds. */

/* Delta stored for a position whose next token cannot be derived in the parallel
 * pass (chunk sizes are < 2^28, so position + kUnknown never looks like a position). */
constexpr uint32_t kUnknown = 1u << 28;
constexpr uint32_t kNxUnknown = 0xffffu;     /* the same in the 16-bit form the chase keeps (real deltas are < 2^15) */

struct Chase
{
  uint32_t wb;    /* virtual position of window slot 0 */
  uint32_t nx01, nx23; /* lane l: the deltas of positions wb + 4 l + {0, 1} and {2, 3}, 16 bits each (kNxUnknown = unknown) */
  uint32_t q;     /* virtual position of the next token */
  uint8_t* tab;   /* LDS, kChaseLds bytes */
};

__device__ __forceinline__ void chase_init(Chase& c, uint32_t q, uint8_t* lds)
{
  c.q = q;
  c.nx01 = 0;
  c.nx23 = 0;
  c.wb = q - kChaseWin; /* forces a build */
  c.tab = lds;
}

/* Lane l of a build owns the 4 consecutive window positions 4 l .. 4 l + 3: their token
 * bytes come from two dword reads of the ring and their table entries are written as one dword.
 * A window is "interior" when every byte a delta may look at is resident and before the end of
 * the chunk; the format's `fast` delta then needs no bounds tests at all. */
template <class R, class Delta>
__device__ __forceinline__ void chase_build(Chase& c, const R& r, Delta delta, uint32_t positions = kChaseWin)
{
  /* `positions` (<= kChaseWin, uniform): only the first that many window positions count as inside the window -- the
   * workgroup-per-chunk decoder (common/lz_team.hip.h) cuts its windows where 64 lanes are sure to hold every token */
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  c.wb = c.q;
  const uint32_t room = r.vend - c.wb; /* c.q < vend */
  const uint32_t limit = room < positions ? room : positions;
  const uint32_t reach = c.wb + kChaseWin + Delta::kReach;
  const bool interior = c.wb >= r.lo && reach <= r.hi && reach <= r.vend;
  const uint32_t base = c.wb + 4 * lane;
  uint32_t nx[4];
  if (interior) {
    /* 8 stream bytes from `base` on, from three aligned dwords (a misaligned ds_read_b32 costs 16x) */
    const uint32_t a0 = base & ~3u;
    const uint32_t d0 = *(const uint32_t*)(r.ring + (a0 & R::kMask));
    const uint32_t d1 = *(const uint32_t*)(r.ring + ((a0 + 4) & R::kMask));
    const uint32_t d2 = *(const uint32_t*)(r.ring + ((a0 + 8) & R::kMask));
    const uint32_t w0 = wave::align_bytes(d1, d0, base & 3u);
    const uint32_t w1 = wave::align_bytes(d2, d1, base & 3u);
    const uint64_t w = ((uint64_t)w1 << 32) | w0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      nx[k] = delta.fast(r, base + k, w >> (8 * k));
    }
    /* what the straight-line form gave up on gets the general one (a branch for the wave: rare on text, every window
     * of a sorted column, whose matches take a second length byte) */
    if (Delta::kSecondChance && wave::ballot((nx[0] | nx[1] | nx[2] | nx[3]) >= kUnknown)) {
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        if (nx[k] >= kUnknown) {
          nx[k] = delta.second(r, base + k, w >> (8 * k));
        }
      }
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      nx[k] = delta(r, base + k);
    }
  }
  uint32_t a[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    a[k] = 4 * lane + k + nx[k] < limit ? nx[k] : 255u; /* the successor must be a token inside the window */
    nx[k] = nx[k] >= kNxUnknown ? kNxUnknown : nx[k];
  }
  /* kept for the token through which the chain leaves the window (chase_tokens): two registers, not four */
  c.nx01 = nx[0] | (nx[1] << 16);
  c.nx23 = nx[2] | (nx[3] << 16);
  /* the four distances of a lane travel as two dwords of two 16-bit lanes (positions 0|1 and 2|3): a doubling round
   * is two packed adds + two packed saturations instead of four of each, and one byte permute packs the table word */
  uint32_t a01 = a[0] | (a[1] << 16), a23 = a[2] | (a[3] << 16);
  *(uint32_t*)(c.tab + 4 * lane) = wave::perm_bytes(a23, a01, 0x06040200u);
  wave::sync();
#pragma unroll
  for (uint32_t i = 1; i < kChaseLevels; ++i) {
    const uint8_t* prev = c.tab + (i - 1) * kChaseWin + 4 * lane;
    /* a == 255 reads past its table (into the next one, still inside kChaseLds): the sum saturates anyway */
    const uint32_t g0 = prev[0 + (a01 & 0xffffu)], g1 = prev[1 + (a01 >> 16)];
    const uint32_t g2 = prev[2 + (a23 & 0xffffu)], g3 = prev[3 + (a23 >> 16)];
    a01 = wave::pk_add_sat255(a01, g0 | (g1 << 16)); /* valid sums are <= 254: position + sum < 256 */
    a23 = wave::pk_add_sat255(a23, g2 | (g3 << 16));
    *(uint32_t*)(c.tab + i * kChaseWin + 4 * lane) = wave::perm_bytes(a23, a01, 0x06040200u);
    wave::sync();
  }
}

/* Append token positions to seqpos lanes [k, 64); returns the new count. `slow(r, p)`
 * gives the successor of the token at p when its delta is kUnknown.
 * (A window's ~54 tokens and a batch's 64 never line up: every batch enumerates 2.2 times. Round 6 kept what an
 * enumeration found and the batch had no room for in a register and handed it to the next batch with a shuffle -- 36 vector
 * instructions fewer per batch, and slower: mix 648 -> 646 GB/s, Snappy 481 -> 473, text 596 -> 558 (gpurun r6n); one more
 * live register and two more branches in this loop cost more than the table walk they save. Not kept.) */
template <class R, class Delta, class Slow>
__device__ __forceinline__ uint32_t chase_tokens(
    Chase& c, const R& r, uint32_t& seqpos, uint32_t k, Delta delta, Slow slow)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  while (k < 64 && c.q < r.vend) {
    if (c.q - c.wb >= kChaseWin) {
      if (k >= kChaseEnough) {
        break; /* a batch of what one window held is cheaper than a second build + enumeration for a few more tokens */
      }
      chase_build(c, r, delta);
      LZW_T(1);
    }
    /* Lane k + n: the n-th token from c.q, if it lies in this window. Pure lane arithmetic, no predicate logic (the
     * scalar unit is as busy as the vector unit in this kernel: every && of two lane conditions is a scalar
     * instruction): a lane follows the levels named by the bits of n; a level it does not take adds 0; 255 (the
     * successor leaves the window) poisons the lane through `worst`; the position wraps inside the table. */
    const uint32_t idx = (lane - k) & 63u;
    const uint32_t pos0 = c.q - c.wb;
    /* ranks 32 and up start at the 32nd token: two steps of the 16-token table from the start position (every lane
     * reads the same two bytes); the jump tables themselves stop at 16, one doubling round less per window */
    const uint32_t top = (kChaseLevels - 1) * kChaseWin;
    const uint32_t t1 = c.tab[top + pos0];
    const uint32_t t2 = c.tab[top + ((pos0 + t1) & (kChaseWin - 1))];
    const bool upper = (idx & 32u) != 0;
    uint32_t pos = upper ? (pos0 + t1 + t2) & (kChaseWin - 1) : pos0;
    uint32_t worst = upper ? (t1 > t2 ? t1 : t2) : 0u;
#pragma unroll
    for (uint32_t i = 0; i < kChaseLevels; ++i) {
      const uint32_t a = c.tab[i * kChaseWin + pos];
      const uint32_t adv = a & (uint32_t)(-(int32_t)((idx >> i) & 1u));
      worst = adv > worst ? adv : worst;
      pos = (pos + adv) & (kChaseWin - 1);
    }
    /* every n appears in exactly one lane, and the valid n are a prefix: their number is the ballot's population */
    const uint32_t count = wave::popc64(wave::ballot(worst != 255u));
    const uint32_t room = 64 - k;
    const uint32_t take = count < room ? count : room;
    if (idx < take) {
      seqpos = c.wb + pos;
    }
    if (take < count) {
      c.q = c.wb + wave::read_lane(pos, (k + take) & 63u);
    } else {
      /* the window's chain is used up: leave through the last token's own delta */
      const uint32_t last = wave::read_lane(pos, (k + count - 1) & 63u);
      const uint32_t pair = wave::read_lane((last & 2u) ? c.nx23 : c.nx01, last >> 2);
      const uint32_t d = (last & 1u) ? pair >> 16 : pair & 0xffffu;
      c.q = d == kNxUnknown ? slow(r, c.wb + last) : c.wb + last + d;
    }
    k += take;
    LZW_T(2);
  }
  return k;
}

} // namespace lzw
