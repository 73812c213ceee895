/*
 * nvcomp/device/bitcomp.hpp -- device-side Bitcomp: a caller's own HIP kernel compresses or decompresses a chunk
 * itself, and may produce or consume the elements in registers instead of memory.
 *
 * The shape follows nvcomp/device/ans.hpp and is this library's own (the reference tree has no such header).
 * Header-only, gfx950: a HIP translation unit compiled with `hipcc --offload-arch=gfx950 -I include` uses it with no
 * other include directory and without linking libnvcomp.so. It is not included from nvcomp.h or nvcomp.hpp, which plain
 * C and C++ compilers read.
 *
 * The stream is the one nvcompBatchedBitcompCompressAsync writes (nvcomp/bitcomp.h): both run the same wave-level code
 * (nvcomp/device/detail/bitcomp_core.hpp), so a chunk compressed here is decoded by the batched API and the other way
 * round, and both compressors write the same bytes.
 *
 * NO SHARED MEMORY IS USED AND NO `shared` ARGUMENT EXISTS -- unlike the ANS device API. The codec keeps a block's
 * values in registers and a lane owns its elements from load to store, so a caller's kernel keeps all of its LDS.
 *
 * Rules for compress, compress_from, decompress and decompress_to:
 *   - One full wave: all 64 lanes of a wavefront call it together, converged, with the same arguments. Partial waves
 *     are not supported.
 *   - The calls synchronise at wave scope only and contain NO workgroup barrier (__syncthreads): the other waves of the
 *     workgroup may be on other chunks or doing unrelated work, and need not call at all.
 *   - `in` and `out` may be global or LDS addresses, at any alignment. A wave that has just written `in` itself (a
 *     chunk staged in LDS, lane by lane) calls wave_sync() first.
 *   - Results are returned on every lane, and *decompressed_bytes is written by every lane.
 *   - Sources and sinks are called in DIVERGENT control flow by the lane that owns the element: they must not use
 *     cross-lane operations or barriers.
 *
 * Launch shape: the batched kernels run one wave per chunk in workgroups of four waves, compiled for eight workgroups
 * per CU (six for 8-byte elements): __launch_bounds__(256, 8). A kernel built on this header does best with the same:
 * one chunk per wave, 256 threads, and sinks / sources light enough to stay within 64 vector registers. The codec hides
 * memory latency with waves, not with work inside a wave, so fewer waves per SIMD cost throughput directly. Measured at
 * that shape, decompress() in a user kernel runs at the batched call's speed. compress() and
 * decompress() pick the element width at run time and so carry all eight variants of the codec; a kernel that knows its
 * type calls compress_from<T> / decompress_to<T> and carries two.
 *
 * The lossy helpers (quantize / dequantize) promise a correctly rounded fp32 division. hipcc's default provides it; a
 * translation unit compiled with -fno-hip-fp32-correctly-rounded-divide-sqrt or -ffast-math loses the bit-exactness.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nvcomp/shared_types.h"
#include "nvcomp/device/detail/bitcomp_core.hpp"
#include "nvcomp/device/detail/bitcomp_quantize.hpp"

namespace nvcomp {
namespace device {
namespace bitcomp {

namespace core = ::nvcomp::device::detail::bitcomp;

/* The largest chunk compress() accepts: nvcompBitcompCompressionMaxAllowedChunkSize (nvcomp/bitcomp.h). */
constexpr size_t kMaxChunkBytes = (size_t)1 << 24;

/* Bytes of an element of `type`; 0 for a code that is not a Bitcomp type (the batched API refuses those). */
__host__ __device__ inline uint32_t element_bytes(nvcompType_t type)
{
  switch ((int)type) {
  case NVCOMP_TYPE_CHAR:
  case NVCOMP_TYPE_UCHAR: return 1;
  case NVCOMP_TYPE_SHORT:
  case NVCOMP_TYPE_USHORT: return 2;
  case NVCOMP_TYPE_INT:
  case NVCOMP_TYPE_UINT: return 4;
  case NVCOMP_TYPE_LONGLONG:
  case NVCOMP_TYPE_ULONGLONG: return 8;
  default: return 0;
  }
}

/* Output bound of compress() and compress_from(): equals nvcompBatchedBitcompCompressGetMaxOutputChunkSize(n, {*, type}).
 * 0 for a type the batched API refuses. */
__host__ __device__ inline size_t max_compressed_bytes(size_t n, nvcompType_t type)
{
  const uint32_t s = element_bytes(type);
  return s == 0 ? 0 : (core::max_compressed_bytes(n, s) + 7) & ~(size_t)7;
}

/* Orders the calling wave's earlier writes (LDS or global) before its later reads by other lanes of the same wave:
 * wavefront-scope fences around a wave barrier. No workgroup barrier. */
__device__ inline void wave_sync()
{
  ::nvcomp::device::detail::wave::sync();
}

namespace impl {

__device__ __forceinline__ size_t uniform_size(size_t v)
{
  using ::nvcomp::device::detail::wave::uniform;
  return ((size_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v);
}

template <uint32_t S>
struct UnsignedOf;
template <>
struct UnsignedOf<1>
{
  using type = uint8_t;
};
template <>
struct UnsignedOf<2>
{
  using type = uint16_t;
};
template <>
struct UnsignedOf<4>
{
  using type = uint32_t;
};
template <>
struct UnsignedOf<8>
{
  using type = uint64_t;
};

/* sink(i, T) behind the core's sink(i, unsigned integer of T's width) */
template <class T, class U, class Sink>
struct TypedSink
{
  Sink& sink;
  __device__ __forceinline__ void operator()(uint32_t i, U bits) const
  {
    T v;
    __builtin_memcpy(&v, &bits, sizeof(T));
    sink(i, v);
  }
};

/* The batched decoder's rules around the core (api/bitcomp_api.hip, bitcomp_decompress_kernel), restated:
 *   - an input of 2^32 - 64 bytes or more is refused (nvcompErrorCannotDecompress);
 *   - a capacity above 64 MiB counts as 64 MiB, so a stream that declares more than that is refused;
 *   - the stream is fully validated (the CHECKED decoder) whatever the caller does with the status. */
constexpr size_t kMaxOutCap = (size_t)1 << 26;

__device__ __forceinline__ nvcompStatus_t finish(uint32_t err, uint32_t produced, size_t* decompressed_bytes)
{
  if (decompressed_bytes != nullptr) {
    *decompressed_bytes = err ? 0 : produced;
  }
  return err ? nvcompErrorCannotDecompress : nvcompSuccess;
}

} // namespace impl

/* Compresses in[0, n) into out[0, max_compressed_bytes(n, type)). Returns the compressed size, or 0 -- and writes
 * nothing -- for n > kMaxChunkBytes or a type / algorithm (0: delta + bit-packing, 1: bit-packing only) the batched API
 * refuses. The bytes equal what nvcompBatchedBitcompCompressAsync writes for the chunk with the same
 * {algorithm_type, data_type}; n need not be a multiple of the element size (the rest travels raw). */
__device__ inline size_t compress(const void* in, size_t n, void* out, nvcompType_t type, int algorithm)
{
  n = impl::uniform_size(n);
  const uint32_t s = element_bytes(type);
  if (n > kMaxChunkBytes || s == 0 || (algorithm != 0 && algorithm != 1)) {
    return 0;
  }
  const uint8_t* src = (const uint8_t*)in;
  uint8_t* dst = (uint8_t*)out;
  const uint32_t len = (uint32_t)n;
  switch (s * 2 + (uint32_t)algorithm) {
  case 2: return core::encode_chunk<uint8_t, true>(src, len, dst);
  case 3: return core::encode_chunk<uint8_t, false>(src, len, dst);
  case 4: return core::encode_chunk<uint16_t, true>(src, len, dst);
  case 5: return core::encode_chunk<uint16_t, false>(src, len, dst);
  case 8: return core::encode_chunk<uint32_t, true>(src, len, dst);
  case 9: return core::encode_chunk<uint32_t, false>(src, len, dst);
  case 16: return core::encode_chunk<uint64_t, true>(src, len, dst);
  default: return core::encode_chunk<uint64_t, false>(src, len, dst);
  }
}

/* The fused producer: compresses the n_elems elements that `src` yields, without their ever being in memory.
 * `T src(uint32_t i)` returns element i (T: any type of 1, 2, 4 or 8 bytes; its bit pattern is what is compressed). It
 * is called exactly once for every i of [0, n_elems) and for no other, by the lane that owns the element, in divergent
 * control flow and in no particular order: no cross-lane operations, no barriers inside. The stream is byte for byte
 * that of compress() over the same values; out[0, max_compressed_bytes(n_elems * sizeof(T), type of that width)).
 * Returns the compressed size, or 0 -- writing nothing and calling nothing -- for n_elems * sizeof(T) > kMaxChunkBytes
 * or an algorithm other than 0 or 1. */
template <class T, class Source>
__device__ inline size_t compress_from(size_t n_elems, void* out, int algorithm, Source&& src)
{
  using U = typename impl::UnsignedOf<sizeof(T)>::type;
  n_elems = impl::uniform_size(n_elems);
  if (n_elems > kMaxChunkBytes / sizeof(T) || (algorithm != 0 && algorithm != 1)) {
    return 0;
  }
  const uint32_t len = (uint32_t)(n_elems * sizeof(T));
  const core::FromSource<U, Source> from{src};
  if (algorithm == 0) {
    return core::encode_chunk<U, true>(nullptr, len, (uint8_t*)out, core::AsIs(), from);
  }
  return core::encode_chunk<U, false>(nullptr, len, (uint8_t*)out, core::AsIs(), from);
}

/* Decompresses in[0, in_bytes) into out[0, capacity). Returns nvcompSuccess, or nvcompErrorCannotDecompress exactly
 * where nvcompBatchedBitcompDecompressAsync reports it: a corrupt or truncated stream, or one that declares more than
 * `capacity` bytes. Sets *decompressed_bytes (may be null) to the decoded size, 0 on error. Writes nothing outside
 * out[0, capacity). The batched decoder's size rules hold: an input of 2^32 - 64 bytes or more is refused, and a
 * capacity above 64 MiB counts as 64 MiB. */
__device__ inline nvcompStatus_t decompress(
    const void* in, size_t in_bytes, void* out, size_t capacity, size_t* decompressed_bytes)
{
  in_bytes = impl::uniform_size(in_bytes);
  capacity = impl::uniform_size(capacity);
  if (capacity > impl::kMaxOutCap) {
    capacity = impl::kMaxOutCap;
  }
  uint32_t err = core::kErrNone;
  uint32_t produced = 0;
  if (in_bytes > 0xffffffffull - 64) {
    err = core::kErrInput;
  } else {
    produced = core::decode_chunk<true>((const uint8_t*)in, (uint32_t)in_bytes, (uint8_t*)out, (uint32_t)capacity, err);
  }
  return impl::finish(err, produced, decompressed_bytes);
}

/* The fused consumer: the decoded elements are handed to `sink` instead of memory. `sink(uint32_t i, T v)` is called
 * exactly once for every element i of [0, n / sizeof(T)) (n: the stream's decoded size) and for no other, by the lane
 * that decoded it, in divergent control flow: no cross-lane operations, no barriers inside. Rows arrive in no particular
 * order; for 1- and 2-byte T a lane's 4 / sizeof(T) elements of a row (consecutive indices) arrive as consecutive
 * calls. The n % sizeof(T) trailing raw bytes (at most 7) are written to tail_out[0, n % sizeof(T)), or dropped if
 * tail_out is null. `capacity_bytes` bounds n as `capacity` does in decompress(), with the same size rules.
 * Returns nvcompErrorInvalidValue, without calling the sink, for a sound header whose element width is not sizeof(T)
 * (ask stream_element_bytes() first); otherwise as decompress(). What the sink saw is meaningful only if the call
 * returns nvcompSuccess: a corrupt stream is detected block by block, as in the batched decoder. */
template <class T, class Sink>
__device__ inline nvcompStatus_t decompress_to(
    const void* in, size_t in_bytes, size_t capacity_bytes, size_t* decompressed_bytes, void* tail_out, Sink&& sink)
{
  using U = typename impl::UnsignedOf<sizeof(T)>::type;
  in_bytes = impl::uniform_size(in_bytes);
  capacity_bytes = impl::uniform_size(capacity_bytes);
  if (capacity_bytes > impl::kMaxOutCap) {
    capacity_bytes = impl::kMaxOutCap;
  }
  uint32_t err = core::kErrNone;
  uint32_t produced = 0;
  if (in_bytes > 0xffffffffull - 64) {
    err = core::kErrInput;
  } else {
    const uint8_t* src = (const uint8_t*)in;
    const core::Header h = core::read_header(src, (uint32_t)in_bytes);
    if (!h.ok) {
      err = core::kErrInput;
    } else if ((1u << h.log2_size) != sizeof(T)) {
      if (decompressed_bytes != nullptr) {
        *decompressed_bytes = 0;
      }
      return nvcompErrorInvalidValue;
    } else if (h.n > capacity_bytes) {
      err = core::kErrOutput;
    } else {
      const impl::TypedSink<T, U, Sink> typed{sink};
      const core::ToSink<const impl::TypedSink<T, U, Sink>> to{typed};
      if (h.algo == 0) {
        produced = core::decode_body<U, true, true>(src, (uint32_t)in_bytes, (uint8_t*)tail_out, h.n, err, core::AsIs(), to);
      } else {
        produced = core::decode_body<U, false, true>(src, (uint32_t)in_bytes, (uint8_t*)tail_out, h.n, err, core::AsIs(), to);
      }
    }
  }
  return impl::finish(err, produced, decompressed_bytes);
}

/* The uncompressed size a stream declares, as nvcompBatchedBitcompGetDecompressSizeAsync reports it: 0 unless
 * in_bytes >= 12 and the stream starts with the Bitcomp magic. Any thread may call it; it is no wave operation. */
__host__ __device__ inline size_t decompressed_size(const void* in, size_t in_bytes)
{
  if (in_bytes < core::kHeaderBytes) {
    return 0;
  }
  uint32_t magic, n;
  __builtin_memcpy(&magic, in, 4);
  __builtin_memcpy(&n, (const uint8_t*)in + 8, 4);
  return magic == core::kMagic ? n : 0;
}

/* The element width (1, 2, 4 or 8 bytes) a stream was compressed with -- the sizeof(T) decompress_to() wants -- or 0 if
 * the header is not one the decoder accepts. Any thread may call it. */
__host__ __device__ inline uint32_t stream_element_bytes(const void* in, size_t in_bytes)
{
  if (in_bytes < core::kHeaderBytes) {
    return 0;
  }
  uint32_t magic, kind;
  __builtin_memcpy(&magic, in, 4);
  __builtin_memcpy(&kind, (const uint8_t*)in + 4, 4);
  const bool ok = magic == core::kMagic && (kind & 0xffu) <= 1 && ((kind >> 8) & 0xffu) <= 3 && (kind >> 16) == 0;
  return ok ? 1u << ((kind >> 8) & 0xffu) : 0u;
}

/* The same as an unsigned nvcompType_t (UCHAR, USHORT, UINT, ULONGLONG); NVCOMP_TYPE_BITS for a header that is not
 * accepted. The stream does not record signedness: it does not change a byte. */
__host__ __device__ inline nvcompType_t stream_type(const void* in, size_t in_bytes)
{
  switch (stream_element_bytes(in, in_bytes)) {
  case 1: return NVCOMP_TYPE_UCHAR;
  case 2: return NVCOMP_TYPE_USHORT;
  case 4: return NVCOMP_TYPE_UINT;
  case 8: return NVCOMP_TYPE_ULONGLONG;
  default: return NVCOMP_TYPE_BITS;
  }
}

/* ---- the lossy modes' element arithmetic, for use inside sources and sinks ----
 * Exactly the native API's (nvcomp/native/bitcomp.h, signed integers): q = rint(x / delta), round-half-to-even of the
 * correctly rounded quotient, saturated at the integer's limits, NaN -> 0; x' = (fp)q * delta. fp32 and fp16 compute in
 * fp32 (fp16 widened exactly, narrowed round-to-nearest-even; its delta is a float, as the native API's plan holds it),
 * fp64 in fp64. numpy's np.rint(x / delta) in that precision is the model, bit for bit. */
__device__ inline int32_t quantize(float x, float delta)
{
  return (int32_t)core::quantize32<true>(x, delta);
}

__device__ inline int64_t quantize(double x, double delta)
{
  return (int64_t)core::quantize64<true>(x, delta);
}

__device__ inline float dequantize(int32_t q, float delta)
{
  return core::bits_as<float>(core::dequantize32<true>((uint32_t)q, delta));
}

__device__ inline double dequantize(int64_t q, double delta)
{
  return core::bits_as<double>(core::dequantize64<true>((uint64_t)q, delta));
}

/* fp16 as its bit pattern */
__device__ inline int16_t quantize_half_bits(uint16_t x_bits, float delta)
{
  return (int16_t)core::quantize16<true>(x_bits, delta);
}

__device__ inline uint16_t dequantize_half_bits(int16_t q, float delta)
{
  return core::dequantize16<true>((uint16_t)q, delta);
}

#if defined(__clang__)
/* fp16 as _Float16 */
__device__ inline int16_t quantize(_Float16 x, float delta)
{
  return quantize_half_bits(core::bits_as<uint16_t>(x), delta);
}

__device__ inline _Float16 dequantize(int16_t q, float delta)
{
  return core::bits_as<_Float16>(dequantize_half_bits(q, delta));
}
#endif

} // namespace bitcomp
} // namespace device
} // namespace nvcomp
