/*
 * nvcomp/device/detail/wave_lzc.hpp -- what the LZ4 compressor core needs beyond nvcomp/device/detail/wave.hpp,
 * wave_ext.hpp and wave_lz.hpp (gfx950, CDNA4).
 *
 * Implementation detail of nvcomp/device/lz4.hpp; not an interface of its own.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nvcomp {
namespace device {
namespace detail {
namespace wave {

/* Whether a generic address points into LDS (a compare with the aperture's base). */
__device__ __forceinline__ bool is_lds(const void* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_is_shared(p);
#else
  (void)p;
  return false; /* (the host pass only parses device code) */
#endif
}

} // namespace wave
} // namespace detail
} // namespace device
} // namespace nvcomp
