/*
 * bitcomp/quantize.hip.h -- the load-side and store-side transforms of the native Bitcomp API (include/nvcomp/native/
 * bitcomp.h, api/bitcomp_native_api.hip): error-bounded quantisation of fp16 / fp32 / fp64 elements, fused into the pack
 * and unpack loops of bitcomp/bitcomp.hip.h through its `X` parameter.
 *
 *   compress:    q  = rint(x / delta)   round-half-to-even, the division correctly rounded, in fp32 for fp16 and fp32
 *                                       elements (fp16 widened exactly first) and in fp64 for fp64 elements;
 *                q -> integer of the element's width, signed or unsigned, SATURATING at the type's limits, NaN -> 0
 *   decompress:  x' = (fp)q * delta     in the same precision, narrowed round-to-nearest-even for fp16
 *
 * numpy's `np.rint(x / delta)` in the same precision is the model (tests/test_bitcomp_native.py checks bit for bit), which
 * is why the division is `__fdiv_rn` / `__ddiv_rn` and nothing faster: an approximate reciprocal is off by an ulp on
 * quotients that lie next to .5, and the integer differs.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <nvcomp/device/detail/bitcomp_quantize.hpp>

#include "bitcomp/bitcomp.hip.h"

/* The numeric helpers (bits_as, half_to_float / float_to_half, div_rn, quantize*, dequantize*) live in the public
 * detail header above, which the device-side API shares; the transforms below stay the native API's own. */
namespace nvcomp {
namespace device {
namespace detail {
namespace bitcomp {

/* The element transform of a lossy plan. One type serves the three widths: `in` / `out` are picked by the width of T. */
template <bool SIGNED>
struct Quantize
{
  static constexpr bool kIdentity = false;
  double delta;

  template <class T>
  __device__ __forceinline__ T in(T bits) const
  {
    if (sizeof(T) == 2) {
      return (T)quantize16<SIGNED>((uint16_t)bits, (float)delta);
    }
    if (sizeof(T) == 4) {
      return (T)quantize32<SIGNED>(bits_as<float>((uint32_t)bits), (float)delta);
    }
    if (sizeof(T) == 8) {
      return (T)quantize64<SIGNED>(bits_as<double>((uint64_t)bits), delta);
    }
    return bits; /* (no one-byte floating-point type: never instantiated by the API) */
  }

  template <class T>
  __device__ __forceinline__ T out(T q) const
  {
    if (sizeof(T) == 2) {
      return (T)dequantize16<SIGNED>((uint16_t)q, (float)delta);
    }
    if (sizeof(T) == 4) {
      return (T)dequantize32<SIGNED>((uint32_t)q, (float)delta);
    }
    if (sizeof(T) == 8) {
      return (T)dequantize64<SIGNED>((uint64_t)q, delta);
    }
    return q;
  }

  __device__ __forceinline__ bool keep(uint32_t) const
  {
    return true;
  }
};

/* A store-side transform that also keeps only the elements [lo, hi) of the chunk: partial decompression. */
template <class Q>
struct Range
{
  static constexpr bool kIdentity = false;
  Q q;
  uint32_t lo, hi;

  template <class T>
  __device__ __forceinline__ T in(T v) const
  {
    return q.template in<T>(v);
  }
  template <class T>
  __device__ __forceinline__ T out(T v) const
  {
    return q.template out<T>(v);
  }
  __device__ __forceinline__ bool keep(uint32_t i) const
  {
    return i >= lo && i < hi;
  }
};

} // namespace bitcomp
} // namespace detail
} // namespace device
} // namespace nvcomp
