/*
 * common/api_launch.h -- the host-side lines every file under api/ puts around its kernel launches.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "nvcomp/shared_types.h"

constexpr unsigned kWavesPerBlock = 4; /* 256-thread workgroups, one chunk per wave */

/* hipGetLastError() is sticky per host thread: an unrelated earlier runtime call
 * of the application (e.g. a failed pointer-attribute query) must not be
 * reported as this launch's failure, so the slate is cleared before launching. */
static inline void clear_stale_error()
{
  (void)hipGetLastError();
}

static inline nvcompStatus_t launch_status()
{
  return hipGetLastError() == hipSuccess ? nvcompSuccess : nvcompErrorCudaError;
}

static inline unsigned grid_for(size_t batch_size)
{
  return (unsigned)((batch_size + kWavesPerBlock - 1) / kWavesPerBlock);
}

/* Profiling builds only: read (and clear) the per-phase cycle sums a decoder or compressor keeps in a __device__ array of
 * SLOTS x PER counters (PER > 1: one counter per lane, summed here). Returns the number of slots, -1 on failure. */
template <int SLOTS, int PER = 1, class Symbol>
static inline int prof_read_and_clear(const Symbol& symbol, unsigned long long* host_slots, int n)
{
  static_assert(sizeof(Symbol) == sizeof(unsigned long long) * SLOTS * PER, "the counters as the kernels declare them");
  unsigned long long v[SLOTS * PER] = {};
  if (hipMemcpyFromSymbol(v, HIP_SYMBOL(symbol), sizeof(v)) != hipSuccess) {
    return -1;
  }
  for (int i = 0; i < n && i < SLOTS; ++i) {
    host_slots[i] = 0;
    for (int k = 0; k < PER; ++k) {
      host_slots[i] += v[i * PER + k];
    }
  }
  const unsigned long long z[SLOTS * PER] = {};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(symbol), z, sizeof(z));
  return SLOTS;
}
