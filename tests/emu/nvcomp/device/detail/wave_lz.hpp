/*
 * tests/emu/nvcomp/device/detail/wave_lz.hpp -- TEST INFRASTRUCTURE ONLY.
 * CPU stand-in for include/nvcomp/device/detail/wave_lz.hpp: the device LZ4 core's additional wave primitives, taken
 * from the emulated set (tests/emu/common/wave.h), so that kernels that call nvcomp/device/lz4.hpp run on the host
 * emulation. -Itests/emu comes first on the emulator's include path and the core includes this header with angle
 * brackets, so this file is the one found.
 */
#pragma once

#include "common/wave.h"

namespace nvcomp {
namespace device {
namespace detail {
namespace wave {

using ::wave::ctz64;
using ::wave::write_lane;

} // namespace wave
} // namespace detail
} // namespace device
} // namespace nvcomp
