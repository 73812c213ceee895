/*
 * nvcomp/device/detail/bitcomp_quantize.hpp -- the element arithmetic of Bitcomp's lossy modes: error-bounded
 * quantisation of fp16 / fp32 / fp64 values to integers of the same width, and back.
 *
 * The one implementation: the native API's kernels (nvcomp_amd/csrc/bitcomp/quantize.hip.h fuses these into the pack and
 * unpack loops) and the device-side API (nvcomp/device/bitcomp.hpp: quantize / dequantize, for use inside a caller's
 * sources and sinks) both run the functions below. Implementation detail: not an interface of its own.
 *
 *   quantise:    q  = rint(x / delta)   round-half-to-even, the division correctly rounded, in fp32 for fp16 and fp32
 *                                       elements (fp16 widened exactly first) and in fp64 for fp64 elements;
 *                q -> integer of the element's width, signed or unsigned, SATURATING at the type's limits, NaN -> 0
 *   dequantise:  x' = (fp)q * delta     in the same precision, narrowed round-to-nearest-even for fp16
 *
 * numpy's `np.rint(x / delta)` in the same precision is the model, which is why the division is `__fdiv_rn` /
 * `__ddiv_rn` and nothing faster: an approximate reciprocal is off by an ulp on quotients that lie next to .5, and the
 * integer differs.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace nvcomp {
namespace device {
namespace detail {
namespace bitcomp {

template <class To, class From>
__host__ __device__ __forceinline__ To bits_as(From v)
{
  static_assert(sizeof(To) == sizeof(From), "same width");
  To r;
  __builtin_memcpy(&r, &v, sizeof(To));
  return r;
}

/* IEEE binary16 <-> binary32 on bit patterns: exact widening, round-to-nearest-even narrowing (overflow to infinity,
 * subnormal results included). The card has instructions for both; the host build of the tests has not everywhere. */
__host__ __device__ __forceinline__ float half_to_float(uint16_t h)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return (float)bits_as<_Float16>(h);
#else
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  const uint32_t exp = (h >> 10) & 31u;
  const uint32_t man = h & 0x3ffu;
  if (exp == 0) {
    const float v = (float)man * 5.9604644775390625e-8f; /* man * 2^-24: exact */
    return bits_as<float>(bits_as<uint32_t>(v) | sign);
  }
  if (exp == 31) {
    return bits_as<float>(sign | 0x7f800000u | (man << 13));
  }
  return bits_as<float>(sign | ((exp + 112u) << 23) | (man << 13));
#endif
}

__host__ __device__ __forceinline__ uint16_t float_to_half(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return bits_as<uint16_t>((_Float16)f);
#else
  uint32_t x = bits_as<uint32_t>(f);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7fffffffu;
  if (x >= 0x7f800000u) { /* infinity, NaN (kept a NaN) */
    return (uint16_t)(sign | 0x7c00u | (x > 0x7f800000u ? 0x200u | ((x >> 13) & 0x3ffu) : 0u));
  }
  if (x >= 0x477ff000u) { /* 65520 and above round to infinity */
    return (uint16_t)(sign | 0x7c00u);
  }
  if (x < 0x38800000u) { /* below 2^-14: a subnormal half; the addition rounds to its 2^-24 grid, to nearest even */
    const float r = bits_as<float>(x) + 0.5f;
    return (uint16_t)(sign | (bits_as<uint32_t>(r) - 0x3f000000u));
  }
  const uint32_t odd = (x >> 13) & 1u;
  x += 0xc8000000u + 0xfffu + odd; /* rebias the exponent by -112, round half to even */
  return (uint16_t)(sign | (x >> 13));
#endif
}

/* The correctly rounded quotient. On the card the intrinsic that promises it; the tests' host build of this file has
 * no such intrinsic and needs none: the host's `/` is IEEE division, round to nearest even. */
__device__ __forceinline__ float div_rn(float a, float b)
{
#if defined(__HIPCC__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}

__device__ __forceinline__ double div_rn(double a, double b)
{
#if defined(__HIPCC__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}

/* The rounded product, never contracted with an addition behind it: a caller's sink that accumulates `y + q * delta`
 * gets the two roundings the definition states, whatever -ffp-contract says (hipcc's default fuses across statements,
 * and through __fmul_rn, which is a plain product there). */
__device__ __forceinline__ float mul_rn(float a, float b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a * b;
}

__device__ __forceinline__ double mul_rn(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a * b;
}

/* rint(x / delta) as an integer, saturated: everything at or above `hi` becomes hi_bits, at or below `lo` lo_bits */
template <bool SIGNED>
__device__ __forceinline__ uint32_t quantize32(float x, float delta, float lo, float hi, uint32_t lo_bits, uint32_t hi_bits)
{
  const float q = rintf(div_rn(x, delta));
  if (q != q) {
    return 0u;
  }
  if (q >= hi) {
    return hi_bits;
  }
  if (q <= lo) {
    return lo_bits;
  }
  return SIGNED ? (uint32_t)(int32_t)q : (uint32_t)q;
}

template <bool SIGNED>
__device__ __forceinline__ uint64_t quantize64(double x, double delta)
{
  const double q = rint(div_rn(x, delta));
  if (q != q) {
    return 0u;
  }
  if (SIGNED) {
    if (q >= 9223372036854775808.0) {
      return 0x7fffffffffffffffull;
    }
    if (q <= -9223372036854775808.0) {
      return 0x8000000000000000ull;
    }
    return (uint64_t)(int64_t)q;
  }
  if (q >= 18446744073709551616.0) {
    return 0xffffffffffffffffull;
  }
  if (q <= 0.0) {
    return 0u;
  }
  return (uint64_t)q;
}

/* (fp)q * delta on bit patterns: the three widths, q read as a signed or an unsigned integer */
template <bool SIGNED>
__device__ __forceinline__ uint16_t dequantize16(uint16_t q, float delta)
{
  const float v = SIGNED ? (float)(int16_t)q : (float)q;
  return float_to_half(mul_rn(v, delta));
}

template <bool SIGNED>
__device__ __forceinline__ uint32_t dequantize32(uint32_t q, float delta)
{
  const float v = SIGNED ? (float)(int32_t)q : (float)q;
  return bits_as<uint32_t>(mul_rn(v, delta));
}

template <bool SIGNED>
__device__ __forceinline__ uint64_t dequantize64(uint64_t q, double delta)
{
  const double v = SIGNED ? (double)(int64_t)q : (double)q;
  return bits_as<uint64_t>(mul_rn(v, delta));
}

/* the fp16 quantiser: the element widened exactly, the fp32 arithmetic, saturated to 16 bits */
template <bool SIGNED>
__device__ __forceinline__ uint16_t quantize16(uint16_t half_bits, float delta)
{
  return SIGNED ? (uint16_t)quantize32<true>(half_to_float(half_bits), delta, -32768.0f, 32767.0f, 0x8000u, 0x7fffu)
                : (uint16_t)quantize32<false>(half_to_float(half_bits), delta, 0.0f, 65535.0f, 0u, 0xffffu);
}

/* the fp32 quantiser at its own width */
template <bool SIGNED>
__device__ __forceinline__ uint32_t quantize32(float x, float delta)
{
  return SIGNED ? quantize32<true>(x, delta, -2147483648.0f, 2147483648.0f, 0x80000000u, 0x7fffffffu)
                : quantize32<false>(x, delta, 0.0f, 4294967296.0f, 0u, 0xffffffffu);
}

} // namespace bitcomp
} // namespace detail
} // namespace device
} // namespace nvcomp
