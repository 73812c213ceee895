/*
 * ans/ans.hip.h -- the batched ANS kernels' view of the codec core.
 *
 * The wave-level encoder and decoder live in the public detail header nvcomp/device/detail/ans_core.hpp, where the
 * device-side API (nvcomp/device/ans.hpp) runs the same code in a caller's kernel. This header names that core `ans`
 * for the library's sources. Stream layout and LDS budget: see ans_core.hpp and DESIGN.md "ANS stream layout".
 */
#pragma once

#include <nvcomp/device/detail/ans_core.hpp>

#include "common/wave.h"

namespace ans = nvcomp::device::detail::ans;
