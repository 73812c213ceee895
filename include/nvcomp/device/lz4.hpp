/*
 * nvcomp/device/lz4.hpp -- device-side LZ4: a caller's own HIP kernel compresses or decompresses a chunk itself.
 *
 * The LZ4 half of the reference's device-side extension (nvcomp/device/ans.hpp is the other); its header is not part of
 * the reference tree, so the shape below is this library's own. Header-only, gfx950: a HIP translation unit compiled with
 * `hipcc --offload-arch=gfx950 -I include` uses it with no other include directory and without linking libnvcomp.so. It
 * is not included from nvcomp.h or nvcomp.hpp, which plain C and C++ compilers read.
 *
 * The stream is one LZ4 block, the format of nvcomp/lz4.h: what nvcompBatchedLZ4CompressAsync and liblz4's
 * LZ4_compress_default / LZ4_compress_HC write for a chunk. The decoder (nvcomp/device/detail/lz4_core.hpp) and the
 * compressor (nvcomp/device/detail/lz4_encode_core.hpp) are code of their own, not the batched kernels': those are tuned
 * to their persistent launch and stay as they are.
 *
 * Rules for compress, decompress and decompressed_size:
 *   - One full wave: all 64 lanes of a wavefront call it together, converged, with the same arguments. Partial waves
 *     are not supported.
 *   - The calls synchronise at wave scope only and contain NO workgroup barrier (__syncthreads): the other waves of the
 *     workgroup may be on other chunks or doing unrelated work, and need not call at all.
 *   - `shared` is this wave's own scratch area of kDecompressSharedBytes (kCompressSharedBytes) bytes, 16-byte
 *     aligned, normally in LDS (__shared__). Waves of one workgroup need disjoint areas; a wave may reuse its area as soon
 *     as the call has returned, and need not clear it. Nothing is written outside it and out[0, out_capacity) (the
 *     compressor: out[0, max_compressed_bytes(in_bytes))).
 *   - `in` and `out` may each be a global or an LDS address, at any alignment. A wave that has just written `in` itself
 *     (a chunk staged in LDS, lane by lane) calls wave_sync() first; so does a wave that goes on to read `out` across
 *     lanes.
 *   - Results are returned on every lane, and *decompressed_bytes is written by every lane.
 *
 * `out` in LDS is the point: every match is then resolved in LDS and the chunk never goes to HBM; the caller's kernel
 * consumes it in place. A chunk of 64 KiB in LDS allows two such workgroups per CU on this part (160 KiB of LDS per CU:
 * 2 x (64 KiB + the waves' scratch areas)).
 *
 * The decoder is always the checked one; there is no variant that trusts the stream. It reads nothing outside
 * [in, in + in_bytes) -- strictly: blocks of 16 aligned bytes are loaded only where they lie wholly inside the stream, its
 * first and last bytes are read one by one -- and writes nothing outside out[0, out_capacity) and its scratch area. A
 * match that reaches in front of `out`, an offset of 0, a truncated stream, bytes behind the final literal run and an
 * output that does not fit are refused. A refused stream may have written a part of its output (inside the capacity).
 *
 * Agreement with the batched API: for every stream and capacity, decompress returns the status and the byte count that
 * nvcompBatchedLZ4DecompressAsync writes to device_statuses[i] and device_actual_uncompressed_bytes[i] for the chunk
 * (nvcompErrorCannotDecompress and 0 for every refusal), and on success the bytes LZ4_decompress_safe produces.
 * Where the batched decoder and liblz4 differ, this decoder follows the batched one:
 *   - a block of 0 bytes decodes to 0 bytes (liblz4: an error);
 *   - liblz4's end-of-block restrictions for encoders (the last five bytes are literals, the last match starts twelve
 *     bytes before the end) are not enforced: a block whose final sequence is literals only, of any length including 0,
 *     and whose matches are each followed by a token, is decoded;
 *   - a capacity above 64 MiB counts as 64 MiB; a stream of 2^32 - 64 bytes or more is refused.
 *
 * compress is the mirror image: `in` in LDS is the point. A kernel that produces or transforms a chunk on the CU -- a byte
 * shuffle in front of LZ4, a quantiser, a page that is about to be parked -- compresses it where it lies, and only the
 * block goes to HBM. With `in` in LDS every byte the match finder looks at is an LDS read; with `in` in global memory the
 * positions around the current step are staged in the scratch area. It reads nothing outside in[0, in_bytes) --
 * strictly, with accesses of at most four bytes that lie wholly inside -- and writes nothing outside
 * out[0, max_compressed_bytes(in_bytes)) and its scratch area. It does not depend on what the scratch area holds on entry:
 * its hash table is never cleared, every candidate is verified by its bytes and its distance (1 ... 65 535, also in
 * chunks above 64 KiB). After another chunk, or over garbage, the block may differ from the one a zeroed area gives; it is
 * always a valid one. The block obeys liblz4's end-of-block rules (the last five bytes are literals, the last match starts
 * at least twelve bytes before the end, chunks below 13 bytes are literals only) and is accepted by LZ4_decompress_safe,
 * nvcompBatchedLZ4DecompressAsync and decompress above. Its bytes are not the batched compressor's, whose own are not
 * deterministic either (benign hash-slot races); its ratio is the batched compressor's to a fraction of a per cent, its
 * speed is not.
 *
 * This is the untyped compressor: the data_type option of nvcompBatchedLZ4Opts_t is not part of the device API.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nvcomp/shared_types.h"
#include "nvcomp/device/detail/lz4_core.hpp"
#include "nvcomp/device/detail/lz4_encode_core.hpp"

namespace nvcomp {
namespace device {
namespace lz4 {

namespace core = ::nvcomp::device::detail::lz4;

/* LDS one wave needs to decompress (16-byte aligned): the 2 KiB input staging ring and its 16 mirror bytes, 2 064 bytes.
 * The batch itself lives in registers. Four waves of a __launch_bounds__(256) workgroup take 8 256 bytes: 19 such
 * workgroups fit a CU's 160 KiB, more than the 8 (32 waves per CU, 8 per SIMD) that registers allow at best -- the
 * decoder is never LDS-limited by its own scratch. */
constexpr size_t kDecompressSharedBytes = core::kDecodeLds;
static_assert(kDecompressSharedBytes % 16 == 0, "per-wave areas keep 16-byte alignment");

/* LDS one wave needs to compress (16-byte aligned): the hash table of 4 096 two-byte positions, 8 192 bytes, the queue of
 * a step's selected matches, 512, and the image of the input around the current step, 2 048 (unused when `in` is LDS):
 * 10 752 bytes. A workgroup that keeps a 64 KiB chunk in LDS and compresses it with one wave takes 76 288 bytes: two such
 * workgroups fit a CU's 160 KiB. Four waves that each compress their own quarter of it take 108 544: one workgroup per
 * CU. Without a chunk in LDS, four compressing waves take 43 008 bytes: three workgroups, 12 waves per CU. */
constexpr size_t kCompressSharedBytes = ::nvcomp::device::detail::lz4enc::kEncodeLds;
static_assert(kCompressSharedBytes % 16 == 0 && kCompressSharedBytes <= 12 * 1024, "per-wave areas keep 16-byte alignment");

/* The positions one step of the compressor covers (tests place chunk sizes around it). */
constexpr size_t kCompressStepBytes = ::nvcomp::device::detail::lz4enc::kStep;

/* The size of the staging ring inside the scratch area (tests place fields across its end). */
constexpr size_t kStagingRingBytes = core::kRingBytes;

/* The largest chunk the batched compressor accepts: nvcompLZ4CompressionMaxAllowedChunkSize (nvcomp/lz4.h). */
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

/* Decompresses the LZ4 block in[0, in_bytes) into out[0, out_capacity). Returns nvcompSuccess, or
 * nvcompErrorCannotDecompress exactly where the batched decoder reports it. Sets *decompressed_bytes (may be null) to
 * the decoded size, 0 on error. `shared`: kDecompressSharedBytes. */
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
    produced = core::decode_block<false, core::RingSrc>(src, (uint32_t)in_bytes, dst, (uint32_t)out_capacity, lds, err);
  }
  if (decompressed_bytes != nullptr) {
    *decompressed_bytes = err ? 0 : produced;
  }
  return err ? nvcompErrorCannotDecompress : nvcompSuccess;
}

/* The parse without the copies: what the block decodes to, as nvcompBatchedLZ4GetDecompressSizeAsync reports it for the
 * chunk -- 0 (and nvcompErrorCannotDecompress) for a malformed block or one of more than 64 MiB; offsets are not
 * tested. A wave operation like decompress, without a scratch area: the stream is read where it lies. */
__device__ inline nvcompStatus_t decompressed_size(const void* in, size_t in_bytes, size_t* decompressed_bytes)
{
  in_bytes = impl::uniform_size(in_bytes);
  const uint8_t* src = (const uint8_t*)impl::uniform_size((size_t)in);
  uint32_t err = core::kErrNone;
  uint32_t produced = 0;
  if (in_bytes > 0xffffffffull - 64) {
    err = core::kErrInput;
  } else {
    produced = core::decode_block<true, core::MemSrc>(src, (uint32_t)in_bytes, nullptr, 0, nullptr, err);
  }
  if (decompressed_bytes != nullptr) {
    *decompressed_bytes = err ? 0 : produced;
  }
  return err ? nvcompErrorCannotDecompress : nvcompSuccess;
}

/* The largest block compress writes for a chunk of n bytes: nvcompBatchedLZ4CompressGetMaxOutputChunkSize(n). */
__host__ __device__ constexpr size_t max_compressed_bytes(size_t n)
{
  return n + n / 255 + 16;
}

/* Compresses in[0, in_bytes) into one LZ4 block at out[0, max_compressed_bytes(in_bytes)) and returns its size, on every
 * lane; an empty chunk gives the one-byte block the batched compressor writes. in_bytes > kMaxChunkBytes: returns 0 and
 * touches neither in, out nor shared. `shared`: kCompressSharedBytes, whatever they hold. (Always inlined: as a called
 * function it would keep its callee-saved registers in private scratch memory.) */
__device__ __forceinline__ size_t compress(const void* in, size_t in_bytes, void* out, void* shared)
{
  namespace enc = ::nvcomp::device::detail::lz4enc;
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

} // namespace lz4
} // namespace device
} // namespace nvcomp
