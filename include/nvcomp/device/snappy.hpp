/*
 * nvcomp/device/snappy.hpp -- device-side Snappy: a caller's own HIP kernel compresses or decompresses a chunk itself.
 *
 * The Snappy member of the device-side family (nvcomp/device/ans.hpp, bitcomp.hpp, lz4.hpp); the reference tree has no such
 * header, so the shape below is this library's own, and it is the shape of nvcomp/device/lz4.hpp. Header-only, gfx950: a
 * HIP translation unit compiled with `hipcc --offload-arch=gfx950 -I include` uses it with no other include directory and
 * without linking libnvcomp.so. It is not included from nvcomp.h or nvcomp.hpp, which plain C and C++ compilers read.
 *
 * The stream is the Snappy raw format of nvcomp/snappy.h: a varint32 that declares the uncompressed length, then tagged
 * elements (literals, copies with one-, two- and four-byte offsets) -- what snappy::RawCompress and
 * nvcompBatchedSnappyCompressAsync write for a chunk. The decoder (nvcomp/device/detail/snappy_core.hpp) and the
 * compressor (nvcomp/device/detail/snappy_encode_core.hpp) are code of their own, not the batched kernels': those are
 * tuned to their persistent launch and stay as they are.
 *
 * Rules for compress, decompress and decompressed_size:
 *   - One full wave: all 64 lanes of a wavefront call it together, converged, with the same arguments. Partial waves
 *     are not supported.
 *   - The calls synchronise at wave scope only and contain NO workgroup barrier (__syncthreads): the other waves of the
 *     workgroup may be on other chunks or doing unrelated work, and need not call at all.
 *   - `shared` is this wave's own scratch area of kDecompressSharedBytes (kCompressSharedBytes) bytes, 16-byte
 *     aligned, normally in LDS (__shared__). It may hold anything on entry. Waves of one workgroup need disjoint areas; a
 *     wave may reuse its area as soon as the call has returned, and need not clear it. Nothing is written outside it and
 *     out[0, out_capacity) (the compressor: out[0, max_compressed_bytes(in_bytes))).
 *   - `in` and `out` may each be a global or an LDS address, at any alignment. A wave that has just written `in` itself
 *     (a chunk staged in LDS, lane by lane) calls wave_sync() first; so does a wave that goes on to read `out` across
 *     lanes.
 *   - Results are returned on every lane, and *decompressed_bytes is written by every lane.
 *
 * `out` in LDS is the point of decompress: every copy is then resolved in LDS and the page never goes to HBM; the caller's
 * kernel consumes it in place (a Parquet / ORC / Avro page decoded and scanned by one kernel).
 *
 * The decoder is always the checked one; there is no variant that trusts the stream. It decodes all four element kinds,
 * whatever the producing compressor chose: literals with 0 to 4 length bytes (also non-canonical spellings, a four-byte
 * field that holds 5), copy-1, copy-2, copy-4 (offsets above 65 535 in chunks above 64 KiB). It reads nothing outside
 * [in, in + in_bytes) -- strictly: blocks of 16 aligned bytes are loaded only where they lie wholly inside the stream, its
 * first and last bytes are read one by one -- and writes nothing outside out[0, out_capacity) and its scratch area.
 *
 * Agreement with the batched API: for every stream and capacity, decompress returns the status and the byte count that
 * nvcompBatchedSnappyDecompressAsync writes to device_statuses[i] and device_actual_uncompressed_bytes[i] for the chunk
 * (nvcompErrorCannotDecompress and 0 for every refusal), and on success the bytes snappy::RawUncompress produces:
 *   - the DECLARED LENGTH is the output limit, not the capacity: a declared length above the capacity is refused before
 *     anything is written; elements that end short of the declared length, or overrun it, are refused, and on an overrun
 *     nothing is written at or behind the declared length (a refused stream may have written a part of its output in front
 *     of it);
 *   - a stream of 0 bytes, a preamble that the stream ends in, one longer than five bytes or above 2^32 - 1 is refused;
 *     bytes behind the last element are elements: there is no trailing garbage that is skipped;
 *   - a field that runs off the stream, an offset of 0 and one that reaches in front of `out` are refused;
 *   - a capacity above 64 MiB counts as 64 MiB (so a declared length above 64 MiB is refused); a stream of 2^32 - 64
 *     bytes or more is refused.
 *
 * compress is the mirror image: `in` in LDS is the point. With `in` in LDS every byte the match finder looks at is an LDS
 * read; with `in` in global memory the positions around the current step are staged in the scratch area. It reads nothing
 * outside in[0, in_bytes) -- strictly, with accesses of at most four bytes that lie wholly inside -- and writes nothing
 * outside out[0, max_compressed_bytes(in_bytes)) and its scratch area. It does not depend on what the scratch area holds on
 * entry: its hash table is never cleared, every candidate is verified by its bytes and its distance (1 ... 65 535, also in
 * chunks above 64 KiB: copy-4 is never written). After another chunk, or over garbage, the stream may differ from the one
 * a zeroed area gives; it is always a valid one, accepted by snappy::RawUncompress, nvcompBatchedSnappyDecompressAsync and
 * decompress above. Literals carry the shortest length field; a match is copy-1 where its length is 4 .. 11 and its
 * offset below 2 048, copy-2 otherwise; a match above 64 bytes is cut so that no piece is shorter than 4. Its bytes are not
 * the batched compressor's; its ratio and its speed against that one: DESIGN.md 3.11.
 *
 * This is the untyped codec: nvcompBatchedSnappyOpts_t has no data type, and neither has the device API.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nvcomp/shared_types.h"
#include "nvcomp/device/detail/snappy_core.hpp"
#include "nvcomp/device/detail/snappy_encode_core.hpp"

namespace nvcomp {
namespace device {
namespace snappy {

namespace core = ::nvcomp::device::detail::snappy;

/* LDS one wave needs to decompress (16-byte aligned): the 2 KiB input staging ring and its 16 mirror bytes, 2 064 bytes.
 * The batch itself lives in registers. */
constexpr size_t kDecompressSharedBytes = core::kDecodeLds;
static_assert(kDecompressSharedBytes % 16 == 0, "per-wave areas keep 16-byte alignment");

/* LDS one wave needs to compress (16-byte aligned): the hash table of 4 096 two-byte positions, 8 192 bytes, the queue of
 * a step's selected matches, 512, and the image of the input around the current step, 2 048 (unused when `in` is LDS):
 * 10 752 bytes. */
constexpr size_t kCompressSharedBytes = ::nvcomp::device::detail::snappyenc::kEncodeLds;
static_assert(kCompressSharedBytes % 16 == 0 && kCompressSharedBytes <= 12 * 1024, "per-wave areas keep 16-byte alignment");

/* The positions one step of the compressor covers (tests place chunk sizes around it). */
constexpr size_t kCompressStepBytes = ::nvcomp::device::detail::snappyenc::kStep;

/* The size of the staging ring inside the scratch area (tests place fields across its end). */
constexpr size_t kStagingRingBytes = core::kRingBytes;

/* The largest chunk the batched compressor accepts: nvcompSnappyCompressionMaxAllowedChunkSize (nvcomp/snappy.h). */
constexpr size_t kMaxChunkBytes = (size_t)1 << 24;

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
  return ((size_t)uniform((uint32_t)((uint64_t)v >> 32)) << 32) | uniform((uint32_t)v);
}

} // namespace impl

/* Decompresses the Snappy stream in[0, in_bytes) into out[0, out_capacity). Returns nvcompSuccess, or
 * nvcompErrorCannotDecompress exactly where the batched decoder reports it. Sets *decompressed_bytes (may be null) to
 * the decoded size -- the declared length --, 0 on error. `shared`: kDecompressSharedBytes. */
__device__ inline nvcompStatus_t decompress(
    const void* in, size_t in_bytes, void* out, size_t out_capacity, size_t* decompressed_bytes, void* shared)
{
  in_bytes = impl::uniform_size(in_bytes);
  out_capacity = impl::uniform_size(out_capacity);
  const uint8_t* src = (const uint8_t*)impl::uniform_size((size_t)in);
  uint8_t* dst = (uint8_t*)impl::uniform_size((size_t)out);
  uint8_t* lds = (uint8_t*)impl::uniform_size((size_t)shared);
  if (out_capacity > core::kMaxOutCap) {
    out_capacity = core::kMaxOutCap;
  }
  uint32_t err = core::kErrNone;
  uint32_t produced = 0;
  if (in_bytes > 0xffffffffull - 64) {
    err = core::kErrInput;
  } else {
    produced = core::decode_block(src, (uint32_t)in_bytes, dst, (uint32_t)out_capacity, lds, err);
  }
  if (decompressed_bytes != nullptr) {
    *decompressed_bytes = err ? 0 : produced;
  }
  return err ? nvcompErrorCannotDecompress : nvcompSuccess;
}

/* The preamble alone: the length the stream declares, as nvcompBatchedSnappyGetDecompressSizeAsync reports it for the
 * chunk -- 0 (and nvcompErrorCannotDecompress) for a malformed preamble, or a stream of 2^32 - 8 bytes or more; the
 * elements are not looked at, and a declared length above 64 MiB is reported as it stands. A wave operation
 * like decompress, without a scratch area: at most five bytes are read where they lie. */
__device__ inline nvcompStatus_t decompressed_size(const void* in, size_t in_bytes, size_t* decompressed_bytes)
{
  in_bytes = impl::uniform_size(in_bytes);
  const uint8_t* src = (const uint8_t*)impl::uniform_size((size_t)in);
  uint32_t total = 0;
  /* (the batched size query gives 0 for a stream of 2^32 - 8 bytes or more) */
  const bool ok = in_bytes <= 0xffffffffull - 8 && core::preamble(src, in_bytes > 5 ? 5u : (uint32_t)in_bytes, total);
  if (decompressed_bytes != nullptr) {
    *decompressed_bytes = ok ? total : 0;
  }
  return ok ? nvcompSuccess : nvcompErrorCannotDecompress;
}

/* The largest stream compress writes for a chunk of n bytes: nvcompBatchedSnappyCompressGetMaxOutputChunkSize(n). */
__host__ __device__ constexpr size_t max_compressed_bytes(size_t n)
{
  return 32 + n + n / 6;
}

/* Compresses in[0, in_bytes) into one Snappy stream at out[0, max_compressed_bytes(in_bytes)) and returns its size, on
 * every lane; an empty chunk gives the one-byte stream (a preamble of 0) the batched compressor writes.
 * in_bytes > kMaxChunkBytes: returns 0 and touches neither in, out nor shared. `shared`: kCompressSharedBytes, whatever
 * they hold. (Always inlined: as a called function it would keep its callee-saved registers in private scratch memory.) */
__device__ __forceinline__ size_t compress(const void* in, size_t in_bytes, void* out, void* shared)
{
  namespace enc = ::nvcomp::device::detail::snappyenc;
  in_bytes = impl::uniform_size(in_bytes);
  const uint8_t* src = (const uint8_t*)impl::uniform_size((size_t)in);
  uint8_t* dst = (uint8_t*)impl::uniform_size((size_t)out);
  uint8_t* lds = (uint8_t*)impl::uniform_size((size_t)shared);
  if (in_bytes > kMaxChunkBytes) {
    return 0;
  }
  if (::nvcomp::device::detail::wave::is_lds(src)) {
    return enc::encode_block<enc::DirectSrc>(src, (uint32_t)in_bytes, dst, lds);
  }
  return enc::encode_block<enc::StagedSrc>(src, (uint32_t)in_bytes, dst, lds);
}

} // namespace snappy
} // namespace device
} // namespace nvcomp
