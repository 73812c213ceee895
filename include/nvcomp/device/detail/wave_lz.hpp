/*
 * nvcomp/device/detail/wave_lz.hpp -- the wave64 primitives the LZ4 core needs beyond nvcomp/device/detail/wave.hpp and
 * wave_ext.hpp (gfx950, CDNA4).
 *
 * Implementation detail of nvcomp/device/lz4.hpp; not an interface of its own. Called from wave-uniform control flow by a
 * full, converged wave of 64 lanes.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nvcomp {
namespace device {
namespace detail {
namespace wave {

/* `vec` with lane `lane` (wave-uniform index) replaced by the wave-uniform `val`: a compare and a select. */
__device__ __forceinline__ uint32_t write_lane(uint32_t vec, uint32_t val, uint32_t lane)
{
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == lane ? val : vec;
}

/* Index of the lowest set bit of a mask that is not 0. */
__device__ __forceinline__ uint32_t ctz64(uint64_t m)
{
  return (uint32_t)__builtin_ctzll(m);
}

} // namespace wave
} // namespace detail
} // namespace device
} // namespace nvcomp
