/*
 * common/lz_ring.hip.h -- the geometry of a wave's LDS (common/lz_window.hip.h), the phase clock of the
 * profiling builds and the input ring: the compressed stream, loaded from HBM in blocks ahead of its readers.
 */
#pragma once

#include "common/lz_common.hip.h"

namespace lzw {

/* Tunables (overridable with -D for the A/B builds of scripts/build_variants.sh). */
/* The output window holds ONE BATCH: the bytes a batch produces (at most kBatchMax) plus the tail of the previous one
 * that still waits for its 16-byte block to fill up -- and 32 bytes of history, no more. Measured on MI355X (profiles/archive/r03_ab_*.jsonl): 84 % of
 * the matches of the headline workload reach further back than any window that fits the LDS budget (61 % further than
 * 4 KiB), so history only turned a twentieth of the far matches into near ones, and paid for it with 1 KiB of LDS per
 * wave and a slide of 768 bytes every other batch: without it +1.6 % (LZ4 mix), +2.4 % (Snappy), +7 % (text, 1 GiB
 * batches). Rounds 1-2 kept 768 bytes of a 2 KiB window (profiles/archive/r01_window_variants.json). A batch may produce up to
 * 2 KiB: 5 712 B of LDS per wave still fit seven waves per SIMD (163 840 / 28), 64 sequences of text never get there,
 * and data with long matches pays the per-batch costs half as often (sorted-key column 749 -> 887 GB/s, int32 column
 * 684 -> 778, profiles/archive/r03_ab_h.jsonl). */
#ifndef NVCOMP_LZW_BATCHMAX
#define NVCOMP_LZW_BATCHMAX 2048
#endif
#ifndef NVCOMP_LZW_KEEP
#define NVCOMP_LZW_KEEP 32 /* the last 32 bytes stay: what the shortest offsets reach (Snappy's one-byte-offset copies, the
                             * patterns of runs that go on across a batch boundary): Snappy mix +3 %, LZ4 mix +1 % */
#endif
#ifndef NVCOMP_LZW_OUTWIN
#define NVCOMP_LZW_OUTWIN (NVCOMP_LZW_BATCHMAX + 64 + NVCOMP_LZW_KEEP)
#endif
#ifndef NVCOMP_LZW_INRING
#define NVCOMP_LZW_INRING 2048
#endif
/* (Round 4 measured the far-match loads non-temporal -- inline-asm loads waited for by hand --: 663 -> 412 GB/s,
 * docs/HISTORY.md 4; the path is gone.) */
#ifndef NVCOMP_LZW_FLUSH_ALIGN
#define NVCOMP_LZW_FLUSH_ALIGN 16 /* a batch's flush ends on this address boundary (16 | 32 | 64 | 128); the rest waits in the window */
#endif
#ifndef NVCOMP_LZW_WAVES_PER_SIMD
#define NVCOMP_LZW_WAVES_PER_SIMD 7
#endif

constexpr uint32_t kOutWin = NVCOMP_LZW_OUTWIN;     /* bytes of output window per wave */
constexpr uint32_t kBatchMax = NVCOMP_LZW_BATCHMAX; /* most output bytes one batch may produce */
constexpr uint32_t kKeep = NVCOMP_LZW_KEEP;         /* history kept when the window slides */
constexpr uint32_t kInRing = NVCOMP_LZW_INRING;     /* bytes of compressed-stream ring per wave */
constexpr uint32_t kInBlock = kInRing / 2; /* ring refill granule: 16 bytes per lane, 64 lanes (1 KiB) or 32 (deflate's 512-byte blocks) */
static_assert(kInBlock == 1024 || kInBlock == 512, "in_load_block: one 16-byte load by the first kInBlock / 16 lanes");
constexpr uint32_t kFlushAlign = NVCOMP_LZW_FLUSH_ALIGN;
constexpr uint32_t kOutLds = kOutWin + 32;
constexpr uint32_t kInLds = kInRing + 16; /* first 16 bytes mirrored after the end */
/* The initial value of a register that is written under a condition and read only where that condition held (the far
 * matches' data: loaded by far lanes, stored by far lanes). On the device: whatever the register holds -- an empty asm
 * statement "defines" it, no instruction is issued; a literal 0 was a v_mov per register and batch (and the compiler turns
 * __builtin_nondeterministic_value into the same zeros). The host build of the emulator (tests/emu) keeps zeros: its
 * sanitizer runs want defined values. */
#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t unset_u32()
{
  uint32_t v;
  asm volatile("" : "=v"(v)); /* volatile: every use is a register of its own, not copies of one */
  return v;
}
#define LZW_UNSET_U32 lzw::unset_u32()
#else
#define LZW_UNSET_U32 0u
#endif
#ifndef NVCOMP_LZW_CHASE_ENOUGH
#define NVCOMP_LZW_CHASE_ENOUGH 64 /* tokens in hand from which the chase does not open another window (A/B: 40, 48) */
#endif
constexpr uint32_t kChaseEnough = NVCOMP_LZW_CHASE_ENOUGH;
constexpr uint32_t kChaseWin = 256;                 /* stream positions one chase window covers */
constexpr uint32_t kChaseLevels = 5;                /* jump tables for 1, 2, 4, 8, 16 tokens ahead; 32 = two steps of the
                                                     * last one from the start position (chase_tokens): no sixth round */
constexpr uint32_t kChaseLds = kChaseLevels * kChaseWin;
constexpr uint32_t kLdsPerWave = kOutLds + kInLds + kChaseLds;

constexpr uint32_t kLitShort = 32;   /* lane-parallel literal runs: up to 8 dwords */
constexpr uint32_t kMatchShort = 32; /* lane-parallel matches:      up to 8 dwords */

/* ---- phase clock (profiling builds only: -DNVCOMP_LZW_PROF) ------------------ */
#ifdef NVCOMP_LZW_PROF
constexpr uint32_t kProfSlots = 20;
__device__ unsigned long long g_prof[kProfSlots];
__device__ __forceinline__ unsigned long long* prof_slots()
{
  __shared__ unsigned long long slots[16][kProfSlots + 1];
  return slots[threadIdx.x >> 6];
}
__device__ __forceinline__ void prof_begin()
{
  if (wave::lane_id() == 0) {
    unsigned long long* p = prof_slots();
    for (uint32_t i = 0; i < kProfSlots; ++i) {
      p[i] = 0;
    }
    p[kProfSlots] = __builtin_readcyclecounter();
  }
}
__device__ __forceinline__ void prof_mark(uint32_t slot)
{
  if (wave::lane_id() == 0) {
    unsigned long long* p = prof_slots();
    const unsigned long long t = __builtin_readcyclecounter();
    p[slot] += t - p[kProfSlots];
    p[kProfSlots] = t;
  }
}
__device__ __forceinline__ void prof_end()
{
  if (wave::lane_id() == 0) {
    unsigned long long* p = prof_slots();
    for (uint32_t i = 0; i < kProfSlots; ++i) {
      atomicAdd(&g_prof[i], p[i]);
    }
  }
}
#define LZW_T(slot) lzw::prof_mark(slot)
#else
#define LZW_T(slot) ((void)0)
#endif

/* ---- compressed-stream ring ------------------------------------------------ */

struct InRing
{
  static constexpr uint32_t kMask = kInRing - 1; /* ring index of virtual position v = v & kMask */
  const uint8_t* base; /* chunk pointer rounded down to 16 bytes (uniform) */
  uint8_t* ring;       /* LDS, kInLds bytes, 16-byte aligned */
  uint32_t vbeg;       /* virtual position of the first chunk byte: chunk & 15 */
  uint32_t vend;       /* vbeg + chunk length */
  uint32_t lo, hi;     /* resident virtual range [lo, hi): multiples of kInBlock */
};

__device__ __forceinline__ void in_init(InRing& r, const uint8_t* in, uint32_t in_len, uint8_t* lds)
{
  const uint32_t a = (uint32_t)((uintptr_t)in & 15u);
  r.base = in - a;
  r.ring = lds;
  r.vbeg = a;
  r.vend = a + in_len;
  r.lo = 0;
  r.hi = 0;
}

/* Load the block of kInBlock bytes starting at virtual position vb (multiple of kInBlock)
 * into the ring. Bytes outside the chunk are never fetched (read as zero). */
__device__ __forceinline__ void in_load_block(InRing& r, uint32_t vb)
{
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  if (kInBlock < 1024 && 16u * lane >= kInBlock) {
    return;
  }
  const uint32_t v = vb + 16u * lane;
  wave::u32x4 x = {0, 0, 0, 0};
  if (v >= r.vbeg && v + 16 <= r.vend) {
    x = wave::gload_u32x4_aligned(r.base + v);
  } else if (v + 16 > r.vbeg && v < r.vend) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
      if (v + j >= r.vbeg && v + j < r.vend) {
        w[j >> 2] |= wave::gload_u8(r.base + v + j) << (8 * (j & 3));
      }
    }
    x.x = w[0];
    x.y = w[1];
    x.z = w[2];
    x.w = w[3];
  }
  const uint32_t idx = v & (kInRing - 1);
  *(wave::u32x4*)(r.ring + idx) = x;
  if (idx == 0) {
    *(wave::u32x4*)(r.ring + kInRing) = x; /* mirror: 4-byte reads may run past the end */
  }
}

/* Make [q, want_hi) resident as far as the ring allows, keeping everything from
 * q's block on. q must be >= the oldest position still needed. */
__device__ __forceinline__ void in_ensure(InRing& r, uint32_t q, uint32_t want_hi)
{
  const uint32_t qb = q & ~(kInBlock - 1);
  if (qb >= r.hi || qb < r.lo) { /* nothing useful resident: restart at q's block */
    r.lo = qb;
    r.hi = qb;
  } else {
    r.lo = qb;
  }
  bool loaded = false;
  while (r.hi < want_hi && r.hi < r.vend && r.hi - r.lo < kInRing) {
    in_load_block(r, r.hi);
    r.hi += kInBlock;
    loaded = true;
  }
  if (loaded) {
    wave::sync();
  }
}

/* Byte at virtual position v (per lane): LDS when resident, HBM otherwise. The stream type R is lzw::InRing (a wave's
 * ring over the chunk) or lzt::Stream (common/lz_team.hip.h: the whole chunk staged in LDS, kMask = all ones). */
template <class R>
__device__ __forceinline__ uint32_t in_byte(const R& r, uint32_t v)
{
  if (v >= r.lo && v < r.hi) {
    return r.ring[v & R::kMask];
  }
  return wave::gload_u8(r.base + v);
}

/* Same for a wave-uniform position; the result is uniform. */
template <class R>
__device__ __forceinline__ uint32_t in_byte_uniform(const R& r, uint32_t v)
{
  return wave::uniform(in_byte(r, v));
}

/* The 8 stream bytes at virtual position p -- those of them that are resident, the others are whatever the ring
 * holds there: three aligned dword reads (a misaligned ds_read_b32 is served lane by lane) and a funnel shift. */
template <class R>
__device__ __forceinline__ uint64_t ring_bytes8(const R& r, uint32_t p)
{
  const uint32_t m = R::kMask;
  const uint32_t a0 = p & ~3u;
  const uint32_t d0 = *(const uint32_t*)(r.ring + (a0 & m));
  const uint32_t d1 = *(const uint32_t*)(r.ring + ((a0 + 4) & m));
  const uint32_t d2 = *(const uint32_t*)(r.ring + ((a0 + 8) & m));
  const uint32_t lo = wave::align_bytes(d1, d0, p & 3u);
  const uint32_t hi = wave::align_bytes(d2, d1, p & 3u);
  return ((uint64_t)hi << 32) | lo;
}

} // namespace lzw
