/*
 * tests/emu/nvcomp/device/detail/wave_lzc.hpp -- TEST INFRASTRUCTURE ONLY.
 * CPU stand-in for include/nvcomp/device/detail/wave_lzc.hpp, so that kernels that call the compressor of
 * nvcomp/device/lz4.hpp run on the host emulation. -Itests/emu comes first on the emulator's include path and the core
 * includes this header with angle brackets, so this file is the one found.
 *
 * The emulation has one piece of memory that stands for LDS, the running workgroup's dynamic area
 * (emu::dynamic_lds(), 160 KiB); `__shared__` arrays are ordinary statics there. A test kernel that wants the
 * compressor's LDS path on the emulator keeps its chunk in that area.
 */
#pragma once

#include "common/wave.h"

namespace nvcomp {
namespace device {
namespace detail {
namespace wave {

inline bool is_lds(const void* p)
{
  const uint8_t* lds = emu::dynamic_lds();
  return (const uint8_t*)p >= lds && (const uint8_t*)p < lds + 160 * 1024;
}

} // namespace wave
} // namespace detail
} // namespace device
} // namespace nvcomp
