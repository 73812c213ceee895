/*
 * common/lz_common.hip.h -- what every LZ-family decoder and encoder here shares (LZ4, Snappy, DEFLATE, Zstd):
 *   - the error bits a chunk's decode ends with;
 *   - unaligned accessors (gfx950 global and LDS accesses may be unaligned);
 *   - wave_copy, the wave-cooperative copy of bytes that do not overlap (the encoders write literal runs with it);
 *   - Seq, one parsed sequence as a lane holds it between a format's parser and the executors (common/lz_window.hip.h).
 * How a chunk is decoded is described where it is done (common/lz_window.hip.h); docs/HISTORY.md 3.1 has the generations.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common/wave.h"

namespace lz {

enum : uint32_t {
  kErrNone = 0,
  kErrInput = 1,  /* compressed stream truncated / malformed */
  kErrOutput = 2, /* output buffer too small */
  kErrOffset = 4  /* match offset 0 or beyond the produced output */
};

/* ---- unaligned accessors (gfx950 global/LDS accesses may be unaligned) ---- */

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

struct __attribute__((packed)) Bytes16
{
  uint32_t w[4];
};

__device__ __forceinline__ void copy16(uint8_t* d, const uint8_t* s)
{
  Bytes16 t;
  __builtin_memcpy(&t, s, 16);
  __builtin_memcpy(d, &t, 16);
}

/* ---- wave-cooperative copy ------------------------------------------------ */

/* dst[0,len) = src[0,len), non-overlapping, any alignment. */
__device__ __forceinline__ void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t len)
{
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  uint32_t base = 0;
  for (; base + 1024 <= len; base += 1024) {
    copy16(dst + base + lane * 16, src + base + lane * 16);
  }
  for (; base + 256 <= len; base += 256) {
    st_u32(dst + base + lane * 4, ld_u32(src + base + lane * 4));
  }
  for (uint32_t i = base + lane; i < len; i += 64) {
    dst[i] = src[i];
  }
}

/* ---- per-lane sequence record --------------------------------------------- */

struct Seq
{
  uint32_t lit_src;   /* byte index of the first literal in the compressed chunk */
  uint32_t lit_len;
  uint32_t match_off; /* distance back from the match destination */
  uint32_t match_len; /* 0: no match (LZ4 last sequence / Snappy literal element) */
  /* Filled by no parser and read by no executor. They stay because without them seven of the decode kernels come out of
   * the compiler with other text (profiles/lz_first_generation_retired.md). */
  uint32_t lit_lo = 0;
  uint32_t lit_hi = 0;
};

} // namespace lz
