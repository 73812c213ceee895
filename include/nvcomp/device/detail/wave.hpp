/*
 * nvcomp/device/detail/wave.hpp -- the wave64 cross-lane primitives the device-side codecs use (gfx950, CDNA4).
 *
 * Implementation detail of nvcomp/device/ans.hpp; not an interface of its own. These are the same operations as the
 * library's internal wave header, reduced to what the ANS core needs, in their own namespace so that both can be
 * included into one translation unit. Every function assumes a full, converged wave of 64 lanes and is called from
 * wave-uniform control flow.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nvcomp {
namespace device {
namespace detail {
namespace wave {

/* The lane's index in its wave, computed where it is asked for (two VALU instructions, nothing held live across loops). */
__device__ __forceinline__ int fresh_lane_id()
{
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

/* 64-bit mask of lanes whose predicate is true. */
__device__ __forceinline__ uint64_t ballot(bool pred)
{
  return __builtin_amdgcn_ballot_w64(pred);
}

/* Value of lane `lane` (wave-uniform index) broadcast to the scalar unit. */
__device__ __forceinline__ uint32_t read_lane(uint32_t v, uint32_t lane)
{
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane);
}

/* Tell the compiler a value is wave-uniform (it moves to an SGPR). */
__device__ __forceinline__ uint32_t uniform(uint32_t v)
{
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

/* Inclusive prefix sum across the wave: 4 row_shr steps inside each row of 16 lanes, then row_bcast:15 / row_bcast:31
 * to carry across rows (DPP, no LDS). */
__device__ __forceinline__ uint32_t scan_add_inclusive(uint32_t v)
{
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); /* row_shr:1 */
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); /* row_shr:2 */
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); /* row_shr:4 */
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); /* row_shr:8 */
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); /* row_bcast:15 */
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); /* row_bcast:31 */
  return v;
}

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b)
{
  return a > b ? a : b;
}

/* Wave-wide unsigned maximum, returned as a uniform value (same DPP ladder; lane 63 ends up holding it). */
__device__ __forceinline__ uint32_t reduce_max(uint32_t v)
{
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
  v = umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
  return read_lane(v, 63);
}

__device__ __forceinline__ uint32_t reduce_add(uint32_t v)
{
  return read_lane(scan_add_inclusive(v), 63);
}

/* Order this wave's earlier memory writes (LDS or global) before its later reads, across lanes. A wave's LDS and
 * vector-memory operations are served in issue order, so what has to be stopped is the compiler moving a load above a
 * store it believes cannot alias: fences at wavefront scope and a wave barrier. No workgroup barrier. */
__device__ __forceinline__ void sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t popc64(uint64_t m)
{
  return (uint32_t)__builtin_popcountll(m);
}

/* a * b for operands below 2^24 (v_mul_u32_u24: full rate, unlike the 32-bit v_mul_lo_u32). */
__device__ __forceinline__ uint32_t mul24(uint32_t a, uint32_t b)
{
  uint32_t r;
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

/* Number of set bits of m below the calling lane (v_mbcnt_lo/hi). */
__device__ __forceinline__ uint32_t prefix_popc(uint64_t m)
{
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

} // namespace wave
} // namespace detail
} // namespace device
} // namespace nvcomp
