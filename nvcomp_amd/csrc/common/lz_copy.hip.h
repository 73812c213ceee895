/*
 * common/lz_copy.hip.h -- the copy primitives of the LZ decoders: clamped dword copies in LDS, the aligned
 * store of far-match data, overlapping (periodic) match copies.
 */
#pragma once

#include "common/lz_ring.hip.h"

namespace lzw {

/* ---- LDS copies ------------------------------------------------------------ */

__device__ __forceinline__ uint32_t ld32(const uint8_t* p)
{
  return lz::ld_u32(p);
}

/* Number of 4-byte steps (2, 4 or 8) that cover the longest participating run:
 * two ballots instead of a wave-wide max reduction.
 * A ballot of ONE compare is the compare itself (v_cmp writes the mask). A ballot of `a && b` is not: the compiler forms
 * the mask on the scalar side (s_and_b64), turns it into a 0 / 1 register (v_cndmask) and compares that with 0 (v_cmp_ne)
 * -- two vector instructions for a mask the scalar unit already held. So the masks of this file are ballots of single
 * compares, joined with & | ~ on the scalar unit; `participants` is such a mask. */
__device__ __forceinline__ uint32_t steps_for(uint64_t participants, uint32_t len)
{
  if (wave::ballot(len > 16) & participants) {
    return 8;
  }
  return (wave::ballot(len > 8) & participants) ? 4u : 2u;
}
__device__ __forceinline__ uint32_t steps_for(bool participates, uint32_t len)
{
  return steps_for(wave::ballot(participates), len);
}
/* The same from the length classes of a batch, balloted once where the batch is prepared (gt16 = ballot(len > 16),
 * gt8 = ballot(len > 8)): scalar only. A loop that asks once per round -- the near-match rounds -- otherwise pays the
 * two compares every round, or, with the compares hoisted as lane booleans, a v_cndmask and a v_cmp for each to get the
 * mask back. */
__device__ __forceinline__ uint32_t steps_for(uint64_t participants, uint64_t gt16, uint64_t gt8)
{
  if (gt16 & participants) {
    return 8;
  }
  return (gt8 & participants) ? 4u : 2u;
}

/* Note on alignment: a ds_read_b32 / ds_write_b32 with any misaligned lane serialises the wave instruction
 * on gfx950 (64 cycles instead of 4, scripts/microbench/lds_unaligned.hip). A variant of the copies below
 * that reads aligned dwords, realigns with v_alignbyte_b32 and writes aligned dwords + head/tail bytes
 * halved the LDS busy time but added 48 % VALU instructions and was 13 % slower (profiles/
 * r01_exec_ablation.json): the decoder is bound by instruction issue, not by the LDS pipe, so the
 * misaligned dword moves stay. The token chase, which reads the ring with uniform phase, uses aligned reads. */

/* Per-lane copy of len (4..32) bytes in `steps` dword moves whose offsets are
 * clamped to len-4: the last moves simply repeat the final dword, so there is no
 * tail handling and no per-step predication. Byte-serial semantics hold for
 * overlapping LDS ranges as long as the distance is >= 4. */
template <uint32_t STEPS>
__device__ __forceinline__ void copy_dwords_clamped(uint8_t* dst, const uint8_t* src, uint32_t len)
{
  const uint32_t last = len - 4;
#pragma unroll
  for (uint32_t i = 0; i < STEPS; ++i) {
    const uint32_t o = 4 * i < last ? 4 * i : last;
    lz::st_u32(dst + o, lz::ld_u32(src + o));
  }
}

/* The same for ranges that do not overlap (a literal run: ring -> window): every load is issued before the first store, so
 * the run costs one LDS round trip, and the dwords live in an array of this instantiation alone. (One array filled and
 * stored under `if (i < steps)` for a run-time `steps` travelled through the arms of that ladder: 5 v_mov_b32 and 8
 * v_mov_b64 per batch.) */
template <uint32_t STEPS>
__device__ __forceinline__ void copy_dwords_clamped_disjoint(uint8_t* dst, const uint8_t* src, uint32_t len)
{
  const uint32_t last = len - 4;
  uint32_t data[STEPS];
#pragma unroll
  for (uint32_t i = 0; i < STEPS; ++i) {
    const uint32_t o = 4 * i < last ? 4 * i : last;
    data[i] = lz::ld_u32(src + o);
  }
#pragma unroll
  for (uint32_t i = 0; i < STEPS; ++i) {
    const uint32_t o = 4 * i < last ? 4 * i : last;
    lz::st_u32(dst + o, data[i]);
  }
}

/* Far-match data (registers) into the window with aligned accesses only. The destination sits a = 0..3 bytes into the
 * aligned `frame`, and the data was LOADED at source - a (execute_window_batch): d[j] is frame dword j as it
 * stands, no realignment (loaded at the source's own address every dword took a v_alignbyte_b32: nine a batch). The match
 * is frame bytes [a, end), end = a + len, len = kMin .. 4 * STEPS, at most 4 * STEPS + 3: dwords 0 .. STEPS - 1 can be whole
 * ones, the bytes behind the last whole dword come from l4, the match's last 4 bytes.
 *   head  a != 0: frame bytes [a, 4) -- all of them the match's, a match being 3 bytes at least -- as a byte (a odd) and
 *         a 16-bit store at byte 2 (a = 1, 2): two stores at most, where byte by byte it was three;
 *   whole dwords; dword 0 only when a = 0 (THREE: and the match has a fourth byte);
 *   tail  end & 3 bytes: a 16-bit store (2, 3) and a byte (1, 3), out of l4's top bytes.
 * Called by the far lanes only. */
template <uint32_t STEPS, bool THREE>
__device__ __forceinline__ void far_store_aligned(uint8_t* frame, uint32_t a, const uint32_t (&d)[8], uint32_t l4, uint32_t len)
{
  const uint32_t end = a + len;
  if (a & 1u) {
    frame[a] = (uint8_t)wave::align_bytes(0u, d[0], a); /* d[0] >> 8 a */
  }
  if ((a + 1u) & 2u) {
    *(uint16_t*)(frame + 2) = (uint16_t)(d[0] >> 16);
  }
  if (a == 0 && (!THREE || len > 3)) {
    *(uint32_t*)frame = d[0];
  }
#pragma unroll
  for (uint32_t j = 1; j < STEPS; ++j) {
    if (4 * j + 4 <= end) {
      *(uint32_t*)(frame + 4 * j) = d[j];
    }
  }
  /* the last tc bytes of the match are the top tc bytes of l4 */
  const uint32_t tc = end & 3u;
  uint8_t* tp = frame + (end & ~3u);
  if (tc & 2u) {
    *(uint16_t*)tp = (uint16_t)wave::align_bytes(0u, l4, 0u - end); /* l4 >> 16 (tc = 2), l4 >> 8 (tc = 3): shift = -end & 3 */
  }
  if (tc & 1u) {
    tp[tc & 2u] = (uint8_t)(l4 >> 24);
  }
}

/* x / off == umulhi(x, kMagic.v[off]) for x < 2^16 and 2 <= off < 256 (the runs' periods): a table instead of the 32-bit
 * division 0xffffffff / off + 1, which was ~40 instructions per long match. */
struct MagicTable
{
  uint32_t v[256];
  constexpr MagicTable() : v()
  {
    for (uint32_t i = 2; i < 256; ++i) {
      v[i] = 0xffffffffu / i + 1;
    }
  }
};
__constant__ static const MagicTable kMagic = MagicTable();

/* Periodic fill: d[i] = d[i - off] for i in [0, len) with off < 256, i.e. the `off` bytes before d repeated. The
 * pattern is read ONCE -- lane l keeps its bytes 4l .. 4l+3 -- and every output dword is assembled from four
 * cross-lane fetches (ds_bpermute) at byte index (position mod off); the dwords go out with ALIGNED stores, 256 bytes
 * per step, a few head / tail bytes around them. No step reads what an earlier step wrote: no round trips through
 * LDS, and when off divides 256 (1, 2, 4, 8, ... : runs and typed columns) the dword of a lane never changes, a step is
 * one store. The pattern-doubling copy this replaces for short periods moved 4 .. 64 bytes per dependent round trip. */
__device__ __forceinline__ void lds_periodic_fill(uint8_t* d, uint32_t off, uint32_t len)
{
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  /* the pattern, a dword per lane: ONE (misaligned) read by the off / 4 lanes that hold a piece of it -- a misaligned
   * LDS access costs per active lane, and the periods of runs are short; the last lane's dword may reach past d - 1:
   * bytes at or behind `off` are never selected */
  uint32_t pat = 0;
  if (4 * lane < off) {
    pat = ld32(d - off + 4 * lane);
  }
  const uint32_t head = (4u - ((uint32_t)(uintptr_t)d & 3u)) & 3u; /* bytes up to the first aligned dword */
  const uint32_t h = head < len ? head : len;
  const uint32_t magic = kMagic.v[off]; /* x / off == umulhi(x, magic) for x < 2^16 (off 1: x mod 1 = 0 below, magic unused) */
  if (lane < h) {
    const uint32_t sidx = off == 1 ? 0u : lane - __umulhi(lane, magic) * off;
    d[lane] = (uint8_t)(wave::shuffle(pat, sidx >> 2) >> (8 * (sidx & 3u)));
  } else if (h != 0) {
    (void)wave::shuffle(pat, 0); /* the cross-lane fetch is executed by the whole wave */
  }
  const uint32_t body = (len - h) >> 2; /* aligned dwords */
  const uint32_t step = off == 1 ? 0u : 256u - __umulhi(256u, magic) * off; /* 256 mod off: how far the phase moves per 256-byte step */
  uint32_t r = h + 4 * lane;
  r = off == 1 ? 0u : r - __umulhi(r, magic) * off;
  uint32_t word = 0;
  bool fresh = true;
  for (uint32_t base = 0; base < body; base += 64) {
    if (fresh) {
      uint32_t sidx = r;
      word = 0;
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t b = (wave::shuffle(pat, sidx >> 2) >> (8 * (sidx & 3u))) & 0xffu;
        word |= b << (8 * k);
        sidx = sidx + 1 == off ? 0 : sidx + 1;
      }
      fresh = step != 0;
      r += step;
      r = r >= off ? r - off : r;
    }
    if (base + lane < body) {
      *(uint32_t*)(d + h + 4 * (base + lane)) = word;
    }
  }
  const uint32_t tail_at = h + 4 * body;
  const uint32_t tail = len - tail_at; /* 0 .. 3 */
  {
    const uint32_t i = tail_at + lane;
    const uint32_t sidx = off == 1 ? 0u : i - __umulhi(i, magic) * off;
    const uint32_t b = wave::shuffle(pat, (lane < tail ? sidx : 0u) >> 2) >> (8 * (sidx & 3u));
    if (lane < tail) {
      d[i] = (uint8_t)b;
    }
  }
  wave::sync();
}

/* The same for the periods of runs and typed columns -- off in {1, 2, 4, 8, 16}, len >= 32: every ALIGNED 16-byte
 * block of the run holds the same 16 bytes. The first 32 bytes are written byte by byte (32 lanes, index & (off - 1)),
 * the aligned block inside them is read back by all lanes at once (one address: a broadcast), and the run is a
 * sequence of ds_write_b128 -- 1 KiB per instruction, no cross-lane fetches, no division. A sorted-key column compressed
 * by liblz4 (the reference's published shape) is almost only such matches: 400 bytes at offset 8. */
__device__ __forceinline__ void lds_pow2_fill(uint8_t* d, uint32_t off, uint32_t len)
{
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  if (lane < 32) {
    d[lane] = d[(int32_t)(lane & (off - 1)) - (int32_t)off];
  }
  wave::sync();
  uint8_t* a = d + ((16u - ((uint32_t)(uintptr_t)d & 15u)) & 15u); /* first aligned block: inside d[0, 32) */
  const wave::u32x4 q = *(const wave::u32x4*)a;
  const uint32_t nblk = (uint32_t)(d + len - a) >> 4; /* whole blocks from a on */
  for (uint32_t b = lane; b < nblk; b += 64) {
    *(wave::u32x4*)(a + 16 * b) = q;
  }
  uint8_t* t = a + 16 * nblk;
  if (t + lane < d + len) { /* the last partial block: its bytes are the block's first ones */
    t[lane] = a[lane];
  }
  wave::sync();
}

/* Match copy inside the window with byte-serial semantics: d[i] = d[i - off].
 * Periods below 256 are a periodic fill; longer ones move 256 bytes per step (a step never reads what it writes). */
__device__ __forceinline__ void lds_match_copy(uint8_t* d, uint32_t off, uint32_t len)
{
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  if (off <= 16 && (off & (off - 1)) == 0 && len >= 32) {
    lds_pow2_fill(d, off, len);
    return;
  }
  if (off < 256) {
    lds_periodic_fill(d, off, len);
    return;
  }
  uint32_t done = 0;
  while (done < len) {
    const uint32_t rem = len - done;
    if (rem >= 256) {
      uint8_t* t = d + done + lane * 4;
      lz::st_u32(t, ld32(t - off));
      done += 256;
    } else {
      for (uint32_t i = lane; i < rem; i += 64) {
        uint8_t* t = d + done + i;
        *t = *(t - off);
      }
      done = len;
    }
    wave::sync();
  }
}

/* dst (LDS) <- src (HBM), non-overlapping, whole wave, any alignment. */
__device__ __forceinline__ void copy_to_lds(uint8_t* dst, const uint8_t* src, uint32_t len)
{
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  uint32_t base = 0;
  for (; base + 256 <= len; base += 256) {
    lz::st_u32(dst + base + lane * 4, wave::gload_u32(src + base + lane * 4));
  }
  for (uint32_t i = base + lane; i < len; i += 64) {
    dst[i] = (uint8_t)wave::gload_u8(src + i);
  }
}

} // namespace lzw
