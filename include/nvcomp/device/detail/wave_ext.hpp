/*
 * nvcomp/device/detail/wave_ext.hpp -- the wave64 primitives the Bitcomp core needs beyond nvcomp/device/detail/wave.hpp
 * (gfx950, CDNA4).
 *
 * Implementation detail of nvcomp/device/bitcomp.hpp; not an interface of its own. The same operations as the
 * library's internal wave header, in the device API's namespace so that both can be included into one translation
 * unit. The cross-lane ones assume a full, converged wave of 64 lanes and are called from wave-uniform control flow.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nvcomp {
namespace device {
namespace detail {
namespace wave {

__device__ __forceinline__ int lane_id()
{
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

/* Per-lane gather: lane i receives v of lane src_lane(i) (ds_bpermute_b32: the LDS crossbar, no LDS memory). */
__device__ __forceinline__ uint32_t shuffle(uint32_t v, uint32_t src_lane)
{
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), (int)v);
}

/* v of the lane below (lane 0: 0): one DPP move across the whole wave (wave_shr:1). */
__device__ __forceinline__ uint32_t prev_lane(uint32_t v)
{
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, true);
}

/* "This value is used here": a register that a load is still filling is waited for at this point, not at its real use
 * further down (the compiler places s_waitcnt in front of the first use). */
__device__ __forceinline__ void touch(uint32_t& v)
{
  asm volatile("" : "+v"(v));
}

/* Nothing is scheduled across this point: unrolled bodies stay one after the other instead of being interleaved (and
 * their temporaries live all at once). */
__device__ __forceinline__ void sched_fence()
{
  __builtin_amdgcn_sched_barrier(0);
}

} // namespace wave
} // namespace detail
} // namespace device
} // namespace nvcomp
