/*
 * cascaded/cascaded.hip.h -- the batched Cascaded kernels' view of the codec core.
 *
 * The wave-level codec -- the sub-chunk coder and decoder and the per-chunk loops around them -- lives in the public detail
 * header nvcomp/device/detail/cascaded_core.hpp, where the device-side API (nvcomp/device/cascaded.hpp) runs the same code
 * in a caller's kernel. This header names that core `casc` for the library's sources and puts the library's own
 * instruments behind the core's hooks: the phase clock of the profiling builds (-DNVCOMP_CASC_PROF) and the path counters
 * of the host emulation (LZ_STAT). Stream layout: see cascaded_core.hpp and DESIGN.md.
 */
#pragma once

#include "common/wave.h"

/* ---- phase clock (profiling builds only: -DNVCOMP_CASC_PROF) ---- */
#ifdef NVCOMP_CASC_PROF
namespace casc_prof {
constexpr uint32_t kProfSlots = 12;
__device__ unsigned long long g_prof[kProfSlots * 64]; /* 64 copies of every slot: the atomics of 8 000 waves on one word would be the profile */
struct ProfClock
{
  unsigned long long last;
  __device__ __forceinline__ void begin() { last = __builtin_readcyclecounter(); }
  __device__ __forceinline__ void mark(uint32_t slot)
  {
    const unsigned long long t = __builtin_readcyclecounter();
    if (wave::lane_id() == 0) {
      atomicAdd(&g_prof[slot * 64 + (blockIdx.x & 63u)], t - last);
    }
    last = __builtin_readcyclecounter();
  }
};
} // namespace casc_prof
#define NVCOMP_CASC_PHASE_BEGIN casc_prof::ProfClock prof_clock; prof_clock.begin()
#define NVCOMP_CASC_PHASE(slot) prof_clock.mark(slot)
#endif

#define NVCOMP_CASC_STAT(name, n) LZ_STAT(name, n)

#include <nvcomp/device/detail/cascaded_core.hpp>

namespace casc = nvcomp::device::detail::cascaded;
