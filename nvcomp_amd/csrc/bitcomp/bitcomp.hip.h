/*
 * bitcomp/bitcomp.hip.h -- the batched and native Bitcomp kernels' view of the codec core.
 *
 * The wave-level encoder and decoder live in the public detail header nvcomp/device/detail/bitcomp_core.hpp, where the
 * device-side API (nvcomp/device/bitcomp.hpp) runs the same code in a caller's kernel. This header names that core
 * `bitcomp` for the library's sources. Stream layout: see bitcomp_core.hpp and DESIGN.md.
 */
#pragma once

#include <nvcomp/device/detail/bitcomp_core.hpp>

#include "common/wave.h"

namespace bitcomp = nvcomp::device::detail::bitcomp;
