/*
 * nvcomp/device/ans.hpp -- device-side ANS: a caller's own HIP kernel compresses or decompresses a chunk itself.
 *
 * nvCOMP 3.0 introduced a device-side API limited to the ANS format; its header is not part of the reference tree, so
 * the shape below is this library's own (like nvcomp/amd_ext.h). Header-only, gfx950: a HIP translation unit compiled
 * with `hipcc --offload-arch=gfx950 -I include` uses it with no other include directory and without linking
 * libnvcomp.so. It is not included from nvcomp.h or nvcomp.hpp, which plain C and C++ compilers read.
 *
 * The stream is the one nvcompBatchedANSCompressAsync writes (nvcomp/ans.h): both run the same wave-level code
 * (nvcomp/device/detail/ans_core.hpp), so a chunk compressed here is decoded by the batched API and the other way
 * round, and both compressors write the same bytes.
 *
 * Rules for compress, decompress and decompress_to:
 *   - One full wave: all 64 lanes of a wavefront call it together, converged, with the same arguments. Partial waves
 *     are not supported.
 *   - The calls synchronise at wave scope only and contain NO workgroup barrier (__syncthreads): the other waves of the
 *     workgroup may be on other chunks or doing unrelated work, and need not call at all.
 *   - `shared` is this wave's own scratch area of kCompressSharedBytes / kDecompressSharedBytes bytes, 16-byte
 *     aligned, normally in LDS (__shared__). Waves of one workgroup need disjoint areas; a wave may reuse its area as
 *     soon as the call has returned. Nothing is written outside it.
 *   - `in` and `out` may be global or LDS addresses. A wave that has just written `in` itself (a chunk staged in LDS,
 *     lane by lane) calls wave_sync() first.
 *   - Results are returned on every lane, and *decompressed_bytes is written by every lane.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nvcomp/shared_types.h"
#include "nvcomp/device/detail/ans_core.hpp"

namespace nvcomp {
namespace device {
namespace ans {

namespace core = ::nvcomp::device::detail::ans;

/* LDS one wave needs (16-byte aligned): 4 KiB of histograms / symbol table to compress; a 4 KiB decode table and a
 * 1 KiB stream ring to decompress. */
constexpr size_t kCompressSharedBytes = core::kEncodeLds;
constexpr size_t kDecompressSharedBytes = core::kDecodeLds;
static_assert(kCompressSharedBytes % 16 == 0 && kDecompressSharedBytes % 16 == 0, "per-wave areas keep 16-byte alignment");

/* The largest chunk compress() accepts: nvcompANSCompressionMaxAllowedChunkSize (nvcomp/ans.h). */
constexpr size_t kMaxChunkBytes = (size_t)1 << 24;

/* Output bound of compress(): equals nvcompBatchedANSCompressGetMaxOutputChunkSize(n). */
__host__ __device__ constexpr size_t max_compressed_bytes(size_t n)
{
  return core::max_compressed_bytes(n);
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

/* The batched decoder's rules around the core (api/ans_api.hip, ans_decompress_kernel): an input of 2^32 - 64 bytes or
 * more is refused, a capacity above 64 MiB counts as 64 MiB. */
template <class Out>
__device__ __forceinline__ nvcompStatus_t decode(
    const void* in, size_t in_bytes, size_t capacity, size_t* decompressed_bytes, void* shared, Out& out)
{
  in_bytes = uniform_size(in_bytes);
  capacity = uniform_size(capacity);
  if (capacity > core::kMaxOutCap) {
    capacity = core::kMaxOutCap;
  }
  uint32_t err = core::kErrNone;
  uint32_t produced = 0;
  if (in_bytes > 0xffffffffull - 64) {
    err = core::kErrInput;
  } else {
    produced = core::decode_chunk((const uint8_t*)in, (uint32_t)in_bytes, out, (uint32_t)capacity, (uint8_t*)shared, err);
  }
  if (decompressed_bytes != nullptr) {
    *decompressed_bytes = err ? 0 : produced;
  }
  return err ? nvcompErrorCannotDecompress : nvcompSuccess;
}

} // namespace impl

/* Compresses in[0, n) into out[0, max_compressed_bytes(n)). Returns the compressed size, or 0 for n > kMaxChunkBytes
 * (nothing is written then). The bytes equal what nvcompBatchedANSCompressAsync writes for the chunk.
 * `shared`: kCompressSharedBytes. */
__device__ inline size_t compress(const void* in, size_t n, void* out, void* shared)
{
  n = impl::uniform_size(n);
  if (n > kMaxChunkBytes) {
    return 0;
  }
  return core::encode_chunk((const uint8_t*)in, (uint32_t)n, (uint8_t*)out, (uint8_t*)shared);
}

/* Decompresses in[0, in_bytes) into out[0, capacity). Returns nvcompSuccess, or nvcompErrorCannotDecompress exactly
 * where the batched decoder reports it (a corrupt or truncated stream, or more than `capacity` bytes). Sets
 * *decompressed_bytes (may be null) to the decoded size, 0 on error. Writes nothing outside out[0, capacity) and
 * shared[0, kDecompressSharedBytes). */
__device__ inline nvcompStatus_t decompress(
    const void* in, size_t in_bytes, void* out, size_t capacity, size_t* decompressed_bytes, void* shared)
{
  core::MemoryOut o{(uint8_t*)out};
  return impl::decode(in, in_bytes, capacity, decompressed_bytes, shared, o);
}

/* The same, with the decoded bytes handed to `sink` instead of memory: the point where a caller's kernel consumes them
 * in place. sink(uint32_t offset, uint32_t word, uint32_t nbytes) is called with offset % 4 == 0 and nbytes in 1 ... 4;
 * `word` holds bytes offset ... offset + nbytes - 1 of the chunk, little-endian, and zeros above them. The calls cover
 * every byte of [0, n) exactly once, stored chunks included, in no particular order. They are made by the lanes that
 * hold bytes, in divergent control flow: the sink must not use cross-lane operations or barriers. What the sink saw is
 * meaningful only if the call returns nvcompSuccess: a corrupt stream is detected late, as in the batched decoder.
 * `capacity` bounds n as in decompress(). */
template <class Sink>
__device__ inline nvcompStatus_t decompress_to(
    const void* in, size_t in_bytes, size_t capacity, size_t* decompressed_bytes, void* shared, Sink&& sink)
{
  core::SinkOut<Sink> o{sink, {0u, 0u}};
  return impl::decode(in, in_bytes, capacity, decompressed_bytes, shared, o);
}

/* The uncompressed size a stream declares, as nvcompBatchedANSGetDecompressSizeAsync reports it: 0 unless
 * in_bytes >= 12 and the stream starts with the ANS magic. Any thread may call it; it is no wave operation. */
__host__ __device__ inline size_t decompressed_size(const void* in, size_t in_bytes)
{
  if (in_bytes < core::kHeaderBytes) {
    return 0;
  }
  uint32_t magic, n;
  __builtin_memcpy(&magic, in, 4);
  __builtin_memcpy(&n, (const uint8_t*)in + 4, 4);
  return magic == core::kMagic ? n : 0;
}

} // namespace ans
} // namespace device
} // namespace nvcomp
