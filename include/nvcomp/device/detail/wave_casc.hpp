/*
 * nvcomp/device/detail/wave_casc.hpp -- the wave64 primitives the Cascaded core needs beyond
 * nvcomp/device/detail/wave.hpp, wave_ext.hpp and wave_lz.hpp (gfx950, CDNA4).
 *
 * Implementation detail of nvcomp/device/cascaded.hpp; not an interface of its own. The same operations as the
 * library's internal wave header, in the device API's namespace so that both can be included into one translation
 * unit. The cross-lane one assumes a full, converged wave of 64 lanes and is called from wave-uniform control flow.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nvcomp {
namespace device {
namespace detail {
namespace wave {

/* (hi:lo) >> shift, low 32 bits, shift = 0 ... 31 (v_alignbit_b32). */
__device__ __forceinline__ uint32_t align_bits(uint32_t hi, uint32_t lo, uint32_t shift)
{
  return __builtin_amdgcn_alignbit(hi, lo, shift);
}

/* Inclusive running unsigned maximum across the wave: the DPP ladder of scan_add_inclusive (4 row_shr steps inside each
 * row of 16 lanes, then row_bcast:15 / row_bcast:31), no LDS. */
__device__ __forceinline__ uint32_t scan_max_inclusive(uint32_t v)
{
#define NVCOMP_WAVE_CASC_MAX_STEP(ctrl, rows)                                                     \
  {                                                                                                \
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rows, 0xf, false); \
    v = v > o ? v : o;                                                                             \
  }
  NVCOMP_WAVE_CASC_MAX_STEP(0x111, 0xf) /* row_shr:1 */
  NVCOMP_WAVE_CASC_MAX_STEP(0x112, 0xf) /* row_shr:2 */
  NVCOMP_WAVE_CASC_MAX_STEP(0x114, 0xf) /* row_shr:4 */
  NVCOMP_WAVE_CASC_MAX_STEP(0x118, 0xf) /* row_shr:8 */
  NVCOMP_WAVE_CASC_MAX_STEP(0x142, 0xa) /* row_bcast:15 */
  NVCOMP_WAVE_CASC_MAX_STEP(0x143, 0xc) /* row_bcast:31 */
#undef NVCOMP_WAVE_CASC_MAX_STEP
  return v;
}

} // namespace wave
} // namespace detail
} // namespace device
} // namespace nvcomp
