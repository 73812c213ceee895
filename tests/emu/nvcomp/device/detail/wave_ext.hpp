/*
 * tests/emu/nvcomp/device/detail/wave_ext.hpp -- TEST INFRASTRUCTURE ONLY.
 * CPU stand-in for include/nvcomp/device/detail/wave_ext.hpp: the device Bitcomp core's additional wave primitives,
 * taken from the emulated set (tests/emu/common/wave.h), so that the Bitcomp kernels in libnvcomp_emu.so and kernels
 * that call nvcomp/device/bitcomp.hpp run on the host emulation. -Itests/emu comes first on the emulator's include path
 * and the core includes this header with angle brackets, so this file is the one found.
 */
#pragma once

#include "common/wave.h"

namespace nvcomp {
namespace device {
namespace detail {
namespace wave {

using ::wave::lane_id;
using ::wave::prev_lane;
using ::wave::sched_fence;
using ::wave::shuffle;
using ::wave::touch;

} // namespace wave
} // namespace detail
} // namespace device
} // namespace nvcomp
