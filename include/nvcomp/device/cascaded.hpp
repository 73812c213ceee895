/*
 * nvcomp/device/cascaded.hpp -- device-side Cascaded (RLE + delta + bit-packing): a caller's own HIP kernel compresses
 * or decompresses a chunk itself, and may produce or consume the elements in registers instead of memory.
 *
 * The shape follows nvcomp/device/bitcomp.hpp and is this library's own (the reference tree has no such header).
 * Header-only, gfx950: a HIP translation unit compiled with `hipcc --offload-arch=gfx950 -I include` uses it with no
 * other include directory and without linking libnvcomp.so. It is not included from nvcomp.h or nvcomp.hpp, which plain
 * C and C++ compilers read.
 *
 * The stream is the one nvcompBatchedCascadedCompressAsync writes (nvcomp/cascaded.h): both run the same wave-level code
 * (nvcomp/device/detail/cascaded_core.hpp), so a chunk compressed here is decoded by the batched API and the
 * CascadedManager and the other way round, and both compressors write the same bytes.
 *
 * SHARED MEMORY: the codec keeps a sub-chunk's intermediate streams in LDS. Every wave that calls passes its own slice
 * `shared` (16-byte aligned, any part of a __shared__ array) of `shared_bytes` bytes; nothing else in LDS is touched and
 * the slice holds nothing between calls. compress_shared_bytes(opts) / decompress_shared_bytes(opts) are the worst cases:
 * with that much a call never fails for lack of LDS. The decoder carves its slice from the stream's actual counts, so
 * compressible data decodes in far less (smooth int32 / float columns at the default options: under 5 KiB where the worst
 * case is 14 KiB); a sub-chunk that does not fit is reported, never overrun.
 *
 * Rules for compress, compress_from, decompress and decompress_to:
 *   - One full wave: all 64 lanes of a wavefront call it together, converged, with the same arguments. Partial waves
 *     are not supported.
 *   - The calls synchronise at wave scope only and contain NO workgroup barrier (__syncthreads): the other waves of the
 *     workgroup may be on other chunks or doing unrelated work, and need not call at all.
 *   - `in` and `out` may be global or LDS addresses. A stream is 4-byte aligned, decoded elements are aligned to their
 *     width (what the batched API asks for). A wave that has just written `in` itself (a chunk staged in LDS, lane by
 *     lane) calls wave_sync() first.
 *   - Results are returned on every lane, and *decompressed_bytes is written by every lane.
 *   - Sources and sinks are called in DIVERGENT control flow by the lane that stages or holds the element: they must not
 *     use cross-lane operations or barriers.
 *
 * Launch shape: the batched decoder's first pass runs one wave per chunk in workgroups of four waves with 5 KiB of LDS a
 * wave, compiled for eight workgroups per CU: __launch_bounds__(256, 8). A kernel built on this header does best near
 * that: the codec hides its chains of dependent LDS accesses with waves, not with work inside a wave. DESIGN.md 3.12 has
 * the measurements.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "nvcomp/shared_types.h"
#include "nvcomp/cascaded.h"
#include "nvcomp/device/detail/cascaded_core.hpp"

namespace nvcomp {
namespace device {
namespace cascaded {

namespace core = ::nvcomp::device::detail::cascaded;

/* The largest chunk compress() accepts: nvcompCascadedCompressionMaxAllowedChunkSize (nvcomp/cascaded.h). */
constexpr size_t kMaxChunkBytes = (size_t)1 << 24;

/* The LDS a workgroup of the batched API may hold: options whose DECODER could need more than this for a sub-chunk are
 * refused by nvcompBatchedCascadedCompressAsync (nvcompErrorNotSupported), and by compress() here, so that every stream
 * either compressor writes can be decoded by the batched decoder. */
constexpr uint32_t kBatchedLdsLimit = 64 * 1024;

/* Bytes of an element of `type`; 0 for a code that is not a Cascaded type. */
__host__ __device__ inline uint32_t element_bytes(nvcompType_t type)
{
  return (int)type >= (int)NVCOMP_TYPE_CHAR && (int)type <= (int)NVCOMP_TYPE_ULONGLONG ? 1u << ((unsigned)type >> 1) : 0u;
}

/* The options the batched API accepts (api/cascaded_api.hip: opts_ok). */
__host__ __device__ inline bool opts_valid(const nvcompBatchedCascadedOpts_t& o)
{
  const uint32_t w = element_bytes(o.type);
  return w != 0 && o.num_RLEs >= 0 && o.num_RLEs <= 7 && o.num_deltas >= 0 && o.num_deltas <= 7 && (o.use_bp == 0 || o.use_bp == 1)
         && o.chunk_size >= 256 && o.chunk_size <= 16384 && o.chunk_size % w == 0;
}

/* Output bound of compress() and compress_from(): what nvcompBatchedCascadedCompressGetMaxOutputChunkSize(n, opts) returns;
 * 0 where that call fails (options it refuses, n > kMaxChunkBytes). */
__host__ __device__ inline size_t max_compressed_bytes(size_t n, const nvcompBatchedCascadedOpts_t& opts)
{
  if (!opts_valid(opts) || n > kMaxChunkBytes) {
    return 0;
  }
  /* worst case: every sub-chunk stored raw (4-byte marker + bytes padded to 4) */
  const size_t num_sub = (n + opts.chunk_size - 1) / opts.chunk_size;
  return core::kHeaderBytes + 4 * num_sub + 8 * num_sub + ((n + 3) & ~(size_t)3);
}

/* LDS per calling wave with which compress() / compress_from() never fail for lack of it (a multiple of 16); 0 for options
 * the batched API refuses. */
__host__ __device__ inline size_t compress_shared_bytes(const nvcompBatchedCascadedOpts_t& opts)
{
  if (!opts_valid(opts)) {
    return 0;
  }
  return (core::compress_lds_per_wave((uint32_t)opts.chunk_size, element_bytes(opts.type), (uint32_t)opts.num_RLEs) + 15u) & ~15u;
}

/* ... with which decompress() / decompress_to() never report nvcompErrorNotSupported for a stream of these options. */
__host__ __device__ inline size_t decompress_shared_bytes(const nvcompBatchedCascadedOpts_t& opts)
{
  if (!opts_valid(opts)) {
    return 0;
  }
  return core::decompress_lds_per_wave((uint32_t)opts.chunk_size, element_bytes(opts.type), (uint32_t)opts.num_RLEs);
}

namespace impl {

struct Header
{
  bool ok;
  uint32_t type, num_rles, num_deltas, n_bytes, sub_bytes;
};

/* The header fields if the stream starts like a Cascaded chunk the decoder may accept. No alignment is asked for: the
 * words are copied out. */
__host__ __device__ inline Header read_header(const void* in, size_t in_bytes)
{
  Header h = {false, 0, 0, 0, 0, 0};
  if (in == nullptr || in_bytes < core::kHeaderBytes) {
    return h;
  }
  uint32_t word[4];
  __builtin_memcpy(word, in, 16);
  h.type = word[1] & 0xffu;
  h.num_rles = (word[1] >> 8) & 0xffu;
  h.num_deltas = (word[1] >> 16) & 0xffu;
  h.n_bytes = word[2];
  h.sub_bytes = word[3];
  if (word[0] != core::kMagic || h.type > 7 || h.num_rles > 7 || h.num_deltas > 7) {
    return h;
  }
  const uint32_t w = 1u << (h.type >> 1);
  h.ok = h.sub_bytes != 0 && h.sub_bytes % w == 0 && h.n_bytes % w == 0 && h.sub_bytes / w <= core::kMaxElems;
  return h;
}

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

/* T source(i) as the core's unsigned integer of T's width */
template <class T, class U, class Source>
struct TypedSource
{
  Source& source;
  __device__ __forceinline__ U operator()(uint32_t i) const
  {
    const T v = source(i);
    U bits;
    __builtin_memcpy(&bits, &v, sizeof(T));
    return bits;
  }
};

/* What every compress call checks before the core runs; the core's parameters if it may. */
__device__ __forceinline__ bool compress_params(const nvcompBatchedCascadedOpts_t& opts, size_t n_bytes, const void* shared,
                                                size_t shared_bytes, core::Params& p)
{
  if (!opts_valid(opts) || n_bytes > kMaxChunkBytes) {
    return false;
  }
  const uint32_t w = element_bytes(opts.type);
  if (n_bytes % w != 0 || ((uintptr_t)shared & 15u) != 0) {
    return false;
  }
  p.sub_bytes = (uint32_t)opts.chunk_size;
  p.type = (uint32_t)opts.type;
  p.num_rles = (uint32_t)opts.num_RLEs;
  p.num_deltas = (uint32_t)opts.num_deltas;
  p.use_bp = (uint32_t)opts.use_bp;
  p.max_bytes = (uint32_t)n_bytes;
  /* what the decoder may need: the batched compressor's rule (nvcompErrorNotSupported there) */
  return core::decompress_lds_per_wave(p.sub_bytes, w, p.num_rles) + 64 <= kBatchedLdsLimit;
}

__device__ __forceinline__ uint32_t budget_of(size_t shared_bytes)
{
  return shared_bytes > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)shared_bytes & ~15u;
}

__device__ __forceinline__ nvcompStatus_t finish(const core::DecodedChunk done, size_t* decompressed_bytes)
{
  const uint32_t err = done.err, produced = done.produced;
  const bool deferred = done.deferred;
  const bool good = err == core::kOk && !deferred;
  if (decompressed_bytes != nullptr) {
    *decompressed_bytes = good ? produced : 0;
  }
  if (err & core::kErrWidth) {
    return nvcompErrorInvalidValue;
  }
  if (err & core::kErrAlign) {
    return nvcompErrorAlignment;
  }
  if (err != core::kOk) {
    return nvcompErrorCannotDecompress;
  }
  return deferred ? nvcompErrorNotSupported : nvcompSuccess;
}

} // namespace impl

/* Orders the calling wave's earlier writes (LDS or global) before its later reads by other lanes of the same wave:
 * wavefront-scope fences around a wave barrier. No workgroup barrier. */
__device__ inline void wave_sync()
{
  ::nvcomp::device::detail::wave::sync();
}

/* Compresses in[0, n_bytes) into out[0, max_compressed_bytes(n_bytes, opts)) and returns the stream's size. The bytes equal
 * what nvcompBatchedCascadedCompressAsync writes for the chunk with the same options. Returns 0 -- nothing final has been
 * written then -- for options the batched API refuses (with nvcompErrorInvalidValue, or with nvcompErrorNotSupported:
 * more RLE layers x elements than the batched decoder's LDS holds), an n_bytes that is no whole number of elements or lies
 * above kMaxChunkBytes, a `shared` that is not 16-byte aligned, or a shared_bytes too small for a sub-chunk's streams
 * (never with compress_shared_bytes(opts)). `in`: aligned to the element width; `out`: 4-byte aligned. */
__device__ inline size_t compress(
    const void* in, size_t n_bytes, void* out, const nvcompBatchedCascadedOpts_t& opts, void* shared, size_t shared_bytes)
{
  n_bytes = impl::uniform_size(n_bytes);
  shared_bytes = impl::uniform_size(shared_bytes);
  core::Params p;
  if (!impl::compress_params(opts, n_bytes, shared, shared_bytes, p)) {
    return 0;
  }
  const uint32_t lane = (uint32_t)::nvcomp::device::detail::wave::lane_id();
  const core::CompressedChunk done = core::compress_chunk((const uint8_t*)in, (uint32_t)n_bytes, (uint8_t*)out, p, (uint8_t*)shared,
                                                          impl::budget_of(shared_bytes), lane);
  return done.deferred ? 0 : core::kHeaderBytes + 4 * (size_t)done.num_sub + done.pay;
}

/* The fused producer: compresses the n_elems elements that `src` yields, without their ever being in memory.
 * `T src(uint32_t i)` returns element i (T: any type of 1, 2, 4 or 8 bytes; its bit pattern is what is compressed); it is
 * asked on the lane that stages the element, in divergent control flow. The source must be PURE: it may be asked more than
 * once for the same i (a sub-chunk that turns out incompressible is read again for its raw copy), and is never asked for an
 * i >= n_elems. sizeof(T) must equal the width of opts.type; otherwise, and wherever compress() would, the call returns 0.
 * The stream is byte for byte that of compress() over the same values. */
template <class T, class Source>
__device__ inline size_t compress_from(
    size_t n_elems, void* out, const nvcompBatchedCascadedOpts_t& opts, void* shared, size_t shared_bytes, Source&& src)
{
  using U = typename impl::UnsignedOf<sizeof(T)>::type;
  n_elems = impl::uniform_size(n_elems);
  shared_bytes = impl::uniform_size(shared_bytes);
  core::Params p;
  if (element_bytes(opts.type) != sizeof(T) || n_elems > kMaxChunkBytes / sizeof(T)
      || !impl::compress_params(opts, n_elems * sizeof(T), shared, shared_bytes, p)) {
    return 0;
  }
  const impl::TypedSource<T, U, Source> typed{src};
  const core::FromSource<U, const impl::TypedSource<T, U, Source>> from{typed};
  const uint32_t lane = (uint32_t)::nvcomp::device::detail::wave::lane_id();
  const core::CompressedChunk done = core::compress_chunk(nullptr, (uint32_t)(n_elems * sizeof(T)), (uint8_t*)out, p, (uint8_t*)shared,
                                                          impl::budget_of(shared_bytes), lane, from);
  return done.deferred ? 0 : core::kHeaderBytes + 4 * (size_t)done.num_sub + done.pay;
}

/* Decompresses in[0, in_bytes) into out[0, capacity). Always checked. Returns the status nvcompBatchedCascadedDecompressAsync
 * reports for the chunk -- nvcompSuccess, nvcompErrorCannotDecompress (corrupt, truncated, or more than `capacity` bytes),
 * nvcompErrorAlignment (`in` not 4-byte aligned, `out` not aligned to the element width) -- and sets *decompressed_bytes
 * (may be null) to the decoded size, 0 unless the status is nvcompSuccess. One status is this call's own: a sub-chunk whose
 * streams do not fit shared_bytes gives nvcompErrorNotSupported (never with decompress_shared_bytes(opts) or
 * stream_shared_bytes(in, in_bytes)); the sub-chunks in front of it have been written, nothing behind them. A `shared`
 * that is not 16-byte aligned is nvcompErrorInvalidValue. Writes nothing outside out[0, capacity). */
__device__ inline nvcompStatus_t decompress(const void* in, size_t in_bytes, void* out, size_t capacity, size_t* decompressed_bytes,
                                            void* shared, size_t shared_bytes)
{
  in_bytes = impl::uniform_size(in_bytes);
  capacity = impl::uniform_size(capacity);
  shared_bytes = impl::uniform_size(shared_bytes);
  if (((uintptr_t)shared & 15u) != 0) { /* a slice that is not 16-byte aligned */
    return impl::finish(core::DecodedChunk{core::kErrWidth, 0, false}, decompressed_bytes);
  }
  const uint32_t lane = (uint32_t)::nvcomp::device::detail::wave::fresh_lane_id();
  return impl::finish(core::decode_chunk((const uint8_t*)in, in_bytes, (uint8_t*)out, capacity, 0u, 1u, lane, (uint8_t*)shared,
                                         impl::budget_of(shared_bytes), true),
                      decompressed_bytes);
}

/* The fused consumer: the decoded elements are handed to `sink` instead of memory; the decoder itself stores nothing
 * outside `shared`. `sink(uint32_t i, T v)` receives element i of the chunk exactly once, on some lane, in divergent control
 * flow and in no particular order: no cross-lane operations, no barriers inside. No element is passed twice and none at or
 * beyond n / sizeof(T) (n: the stream's decoded size). `capacity_bytes` bounds n as `capacity` does in decompress(). Returns
 * nvcompErrorInvalidValue, without calling the sink, for a sound header whose element width is not sizeof(T) (ask
 * stream_element_bytes() first); otherwise as decompress(). What the sink saw counts only if the call returns
 * nvcompSuccess: a corrupt stream, or a slice too small, is detected sub-chunk by sub-chunk. */
template <class T, class Sink>
__device__ inline nvcompStatus_t decompress_to(const void* in, size_t in_bytes, size_t capacity_bytes, size_t* decompressed_bytes,
                                               void* shared, size_t shared_bytes, Sink&& sink)
{
  using U = typename impl::UnsignedOf<sizeof(T)>::type;
  in_bytes = impl::uniform_size(in_bytes);
  capacity_bytes = impl::uniform_size(capacity_bytes);
  shared_bytes = impl::uniform_size(shared_bytes);
  if (((uintptr_t)shared & 15u) != 0) {
    return impl::finish(core::DecodedChunk{core::kErrWidth, 0, false}, decompressed_bytes);
  }
  const impl::TypedSink<T, U, Sink> typed{sink};
  const core::ToSink<U, const impl::TypedSink<T, U, Sink>> to{typed};
  const uint32_t lane = (uint32_t)::nvcomp::device::detail::wave::fresh_lane_id();
  return impl::finish(core::decode_chunk((const uint8_t*)in, in_bytes, nullptr, capacity_bytes, 0u, 1u, lane, (uint8_t*)shared,
                                         impl::budget_of(shared_bytes), true, to),
                      decompressed_bytes);
}

/* The uncompressed size a stream declares, as nvcompBatchedCascadedGetDecompressSizeAsync reports it: 0 unless
 * in_bytes >= 20, `in` is 4-byte aligned and the stream starts with the Cascaded magic. Any thread may call it; it is no
 * wave operation. */
__host__ __device__ inline size_t decompressed_size(const void* in, size_t in_bytes)
{
  if (in == nullptr || in_bytes < core::kHeaderBytes || ((uintptr_t)in & 3u) != 0) {
    return 0;
  }
  uint32_t magic, n;
  __builtin_memcpy(&magic, in, 4);
  __builtin_memcpy(&n, (const uint8_t*)in + 8, 4);
  return magic == core::kMagic ? n : 0;
}

/* The element type a stream was compressed with; NVCOMP_TYPE_BITS if the header is not one the decoder accepts. */
__host__ __device__ inline nvcompType_t stream_type(const void* in, size_t in_bytes)
{
  const impl::Header h = impl::read_header(in, in_bytes);
  return h.ok ? (nvcompType_t)h.type : NVCOMP_TYPE_BITS;
}

/* The element width (1, 2, 4 or 8 bytes) of the stream -- the sizeof(T) decompress_to() wants -- or 0. */
__host__ __device__ inline uint32_t stream_element_bytes(const void* in, size_t in_bytes)
{
  const impl::Header h = impl::read_header(in, in_bytes);
  return h.ok ? 1u << (h.type >> 1) : 0u;
}

/* The LDS with which THIS stream never gives nvcompErrorNotSupported: the worst case of its own options, read from its
 * header. 0 if the data is not a Cascaded chunk. */
__host__ __device__ inline size_t stream_shared_bytes(const void* in, size_t in_bytes)
{
  const impl::Header h = impl::read_header(in, in_bytes);
  return h.ok ? core::decompress_lds_per_wave(h.sub_bytes, 1u << (h.type >> 1), h.num_rles) : 0;
}

} // namespace cascaded
} // namespace device
} // namespace nvcomp
