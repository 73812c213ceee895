/*
 * tests/emu/nvcomp/device/detail/wave_casc.hpp -- TEST INFRASTRUCTURE ONLY.
 * CPU stand-in for include/nvcomp/device/detail/wave_casc.hpp: the device Cascaded core's additional wave primitives,
 * taken from the emulated set (tests/emu/common/wave.h), so that the Cascaded kernels in libnvcomp_emu.so and kernels
 * that call nvcomp/device/cascaded.hpp run on the host emulation. -Itests/emu comes first on the emulator's include path
 * and the core includes this header with angle brackets, so this file is the one found.
 */
#pragma once

#include "common/wave.h"

namespace nvcomp {
namespace device {
namespace detail {
namespace wave {

using ::wave::align_bits;
using ::wave::scan_max_inclusive;

} // namespace wave
} // namespace detail
} // namespace device
} // namespace nvcomp
