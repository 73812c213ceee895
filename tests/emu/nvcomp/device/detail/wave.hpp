/*
 * tests/emu/nvcomp/device/detail/wave.hpp -- TEST INFRASTRUCTURE ONLY.
 * CPU stand-in for include/nvcomp/device/detail/wave.hpp: the device ANS core's wave primitives, taken from the
 * emulated set (tests/emu/common/wave.h), so that the batched ANS kernels in libnvcomp_emu.so and kernels that call
 * nvcomp/device/ans.hpp run on the host emulation. -Itests/emu comes first on the emulator's include path and the core
 * includes this header with angle brackets, so this file is the one found.
 */
#pragma once

#include "common/wave.h"

namespace nvcomp {
namespace device {
namespace detail {
namespace wave {

using ::wave::ballot;
using ::wave::fresh_lane_id;
using ::wave::mul24;
using ::wave::popc64;
using ::wave::prefix_popc;
using ::wave::read_lane;
using ::wave::reduce_add;
using ::wave::reduce_max;
using ::wave::scan_add_inclusive;
using ::wave::sync;
using ::wave::umax;
using ::wave::uniform;

} // namespace wave
} // namespace detail
} // namespace device
} // namespace nvcomp
