/*
 * api/lz4_api.hip -- C ABI of the batched LZ4 codec (include/nvcomp/lz4.h) and
 * the kernels it launches. Host side does argument checks and one launch per
 * *Async call on the caller's stream; nothing here allocates or synchronises.
 * What LZ4 shares with Snappy (kernel bodies, dispatch) is common/lz_api.hip.h, what with every format common/api_batch.hip.h.
 */
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "nvcomp/amd_ext.h"
#include "nvcomp/lz4.h"

#include "common/lz_api.hip.h"
#include "lz4/lz4_decode_window.hip.h"
#include "lz4/lz4_encode.hip.h"
#include "lz4/lz4_size.hip.h"

namespace {

using lzl::kDecWaves;
using lzl::kEncWaves;
using lzl::kWideWaves;

#ifndef NVCOMP_LZ4_RUNS_RATIO
#define NVCOMP_LZ4_RUNS_RATIO 8
#endif
constexpr size_t kRunsRatio = NVCOMP_LZ4_RUNS_RATIO;

/* LZ4 as common/lz_api.hip.h sees it. */
struct Lz4
{
  using FrontEnd = lz4w::FrontEnd;
  static constexpr bool kPairRuns = false; /* the runs of a typed column go to alone() */
  static constexpr bool kEmptyIsError = false;
  /* a chunk that shrank 8 x or more (by the caller's capacity: an LZ4 block does not say what it decodes to) takes the
   * instance of the loop that tries the run executor; everything else the one without it (lz4w::decode_chunk) */
  static __device__ __forceinline__ bool runs(size_t in_len, size_t cap) { return NVCOMP_LZW_RUNS && in_len * kRunsRatio <= cap; }
  template <bool CHECKED>
  static __device__ __forceinline__ uint32_t alone(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, uint8_t* lds, uint32_t& err)
  {
    return lz4w::decode_chunk<CHECKED, true>(in, n, out, cap, lds, err);
  }
};

template <bool CHECKED>
__global__ void __launch_bounds__(64 * kDecWaves, NVCOMP_LZW_WAVES_PER_SIMD) lz4_decompress_window_kernel(const lzl::Tickets launch)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kDecWaves][lzw::kLdsPerWave];
  const uint32_t w = wave::uniform(threadIdx.x >> 6);
  lzl::decode_window_loop<CHECKED>(launch, w, [&](const lzl::Chunk& c, uint32_t& err) -> uint32_t {
    if (Lz4::runs(c.in_len, c.cap)) {
      return lz4w::decode_chunk<CHECKED, true>(c.in, (uint32_t)c.in_len, c.out, (uint32_t)c.cap, lds[w], err);
    }
    return lz4w::decode_chunk<CHECKED, false>(c.in, (uint32_t)c.in_len, c.out, (uint32_t)c.cap, lds[w], err);
  });
}

template <bool CHECKED>
__global__ void __launch_bounds__(128, 7) lz4_decompress_pair_kernel(const lzl::Batch b)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[lzw::pair::kLdsPerChunk];
  lzl::decode_pair<CHECKED, Lz4>(b, lds);
}

template <bool CHECKED, uint32_t WAVES>
__global__ void __launch_bounds__(64 * WAVES, 4) lz4_decompress_team_kernel(const lzl::Tickets launch)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[lzt::Geo<WAVES>::kLds];
  lzl::decode_team_loop<CHECKED, WAVES, Lz4>(launch, lds);
}

__global__ void __launch_bounds__(64 * kWavesPerBlock) lz4_decompress_size_kernel(
    const void* const* __restrict__ comp_ptrs,
    const size_t* __restrict__ comp_bytes,
    size_t* uncompressed_bytes,
    size_t batch_size)
{
  lzl::decompress_size(comp_ptrs, comp_bytes, uncompressed_bytes, batch_size, [](const uint8_t* in, uint32_t in_len) -> uint32_t {
    uint32_t err = lz::kErrNone;
    const uint32_t produced = lz4::decoded_size(in, in_len, err);
    return err ? 0 : produced;
  });
}

/* STRIDE: the element size the caller declared (nvcompBatchedLZ4Opts_t.data_type): matches are searched at element
 * boundaries only, a step covers 64 elements (common/lz_match.hip.h). */
template <uint32_t STRIDE>
__global__ void __launch_bounds__(64 * kEncWaves, NVCOMP_LZM_WAVES_PER_SIMD) lz4_compress_kernel(const lzl::CompressLaunch launch)
{
  __shared__ uint16_t tables[kEncWaves][lzm::kTableU16];
  __shared__ __attribute__((aligned(8))) uint8_t images[kEncWaves][lzm::kImageBytes];
  const uint32_t w = wave::uniform(threadIdx.x >> 6);
  lzl::compress_loop<kEncWaves>(launch, w, [&](const uint8_t* src, uint32_t n, uint8_t* dst) -> uint32_t {
    return lz4::encode_chunk<STRIDE>(src, n, dst, tables[w], images[w]);
  });
}

/* Untyped data: 256-position steps (common/lz_match_wide.hip.h); a wave's LDS is lzm::wide::kLdsPerWave bytes. */
__global__ void __launch_bounds__(64 * kWideWaves, NVCOMP_LZMW_WAVES_PER_SIMD) lz4_compress_wide_kernel(const lzl::CompressLaunch launch)
{
  __shared__ uint16_t tables[kWideWaves][lzm::wide::kEntries];
  __shared__ __attribute__((aligned(16))) uint8_t images[kWideWaves][lzm::wide::kImage];
  __shared__ __attribute__((aligned(16))) uint8_t scratch[kWideWaves][lzm::wide::kScratch];
  const uint32_t w = wave::uniform(threadIdx.x >> 6);
  lzl::compress_loop<kWideWaves>(launch, w, [&](const uint8_t* src, uint32_t n, uint8_t* dst) -> uint32_t {
    return lz4::encode_chunk_wide(src, n, dst, tables[w], images[w], scratch[w]);
  });
}

/* worst case of the block format: one length byte per 255 literals + token + slack (== LZ4_compressBound) */
size_t lz4_bound(size_t n)
{
  return n + n / 255 + 16;
}

nvcompStatus_t lz4_opts_status(nvcompBatchedLZ4Opts_t opts, size_t max_chunk_bytes)
{
  const nvcompType_t t = opts.data_type;
  return lzl::compress_opts_status((t >= NVCOMP_TYPE_CHAR && t <= NVCOMP_TYPE_UINT) || t == NVCOMP_TYPE_BITS, max_chunk_bytes,
                                   nvcompLZ4CompressionMaxAllowedChunkSize);
}

} // namespace

extern "C" {

nvcompStatus_t nvcompBatchedLZ4DecompressGetTempSize(
    size_t num_chunks, size_t /*max_uncompressed_chunk_bytes*/, size_t* temp_bytes)
{
  /* the ticket counter of the persistent waves / workgroups (common/lz_launch.hip.h) and the order they hand out in */
  return lzl::temp_size(num_chunks, temp_bytes, lzl::order_query_bytes(num_chunks));
}

NVCOMP_API_DECOMPRESS_TEMP_SIZE_EX(LZ4)

nvcompStatus_t nvcompBatchedLZ4DecompressAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes,
    size_t* device_actual_uncompressed_bytes,
    size_t batch_size,
    void* const device_temp_ptr,
    size_t temp_bytes,
    void* const* device_uncompressed_ptrs,
    nvcompStatus_t* device_statuses,
    hipStream_t stream)
{
  return lzl::decompress_async<lz4_decompress_team_kernel<true, 16>, lz4_decompress_team_kernel<true, 8>,
                               lz4_decompress_pair_kernel<true>, lz4_decompress_window_kernel<true>>(
      "LZ4", device_compressed_ptrs, device_compressed_bytes, device_uncompressed_bytes,
      device_actual_uncompressed_bytes, batch_size, device_temp_ptr, temp_bytes, device_uncompressed_ptrs, device_statuses, stream);
}

nvcompStatus_t nvcompAmdLZ4DecompressOrderAsync(
    const size_t* device_compressed_bytes, const size_t* device_uncompressed_bytes, size_t first_ordered, size_t batch_size,
    void* device_temp_ptr, size_t temp_bytes, size_t* order_offset, size_t* resident_places, hipStream_t stream)
{
  return lzl::order_inspect_async<lz4_decompress_window_kernel<true>>(
      device_compressed_bytes, device_uncompressed_bytes, first_ordered, batch_size, device_temp_ptr, temp_bytes, order_offset,
      resident_places, stream);
}

nvcompStatus_t nvcompBatchedLZ4GetDecompressSizeAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes,
    size_t batch_size,
    hipStream_t stream)
{
  return lzl::decompress_size_async<lz4_decompress_size_kernel>(device_compressed_ptrs, device_compressed_bytes,
                                                                device_uncompressed_bytes, batch_size, stream);
}

nvcompStatus_t nvcompBatchedLZ4CompressGetTempSize(
    size_t batch_size, size_t max_uncompressed_chunk_bytes, nvcompBatchedLZ4Opts_t format_opts, size_t* temp_bytes)
{
  return lzl::compress_query(temp_bytes, lz4_opts_status(format_opts, max_uncompressed_chunk_bytes),
                             [&] { return batch_size == 0 ? 0 : lzl::kTicketBytes; });
}

NVCOMP_API_COMPRESS_TEMP_SIZE_EX(LZ4, nvcompBatchedLZ4Opts_t)

nvcompStatus_t nvcompBatchedLZ4CompressGetMaxOutputChunkSize(
    size_t max_uncompressed_chunk_bytes, nvcompBatchedLZ4Opts_t format_opts, size_t* max_compressed_bytes)
{
  return lzl::compress_query(max_compressed_bytes, lz4_opts_status(format_opts, max_uncompressed_chunk_bytes),
                             [&] { return lz4_bound(max_uncompressed_chunk_bytes); });
}

nvcompStatus_t nvcompBatchedLZ4CompressAsync(
    const void* const* device_uncompressed_ptrs,
    const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    void* const* device_compressed_ptrs,
    size_t* device_compressed_bytes,
    nvcompBatchedLZ4Opts_t format_opts,
    hipStream_t stream)
{
  const lzl::CompressCall call = {"LZ4", lz4_opts_status(format_opts, max_uncompressed_chunk_bytes), device_uncompressed_ptrs,
                                  device_uncompressed_bytes, max_uncompressed_chunk_bytes, batch_size, device_temp_ptr, temp_bytes,
                                  device_compressed_ptrs, device_compressed_bytes, stream};
  switch (format_opts.data_type) {
  case NVCOMP_TYPE_SHORT:
  case NVCOMP_TYPE_USHORT: return lzl::compress_async<lz4_compress_kernel<2>, kEncWaves>(call);
  case NVCOMP_TYPE_INT:
  case NVCOMP_TYPE_UINT: return lzl::compress_async<lz4_compress_kernel<4>, kEncWaves>(call);
  default:
    return lzl::compress_async<lz4_compress_wide_kernel, kWideWaves>(call);
  }
}

} // extern "C"

#ifdef NVCOMP_LZM_PROF
/* Profiling builds only: read (and clear) the per-phase cycle sums of the LZ4 compressor. */
extern "C" int nvcompAmdCompProfRead(unsigned long long* host_slots, int n)
{
  return prof_read_and_clear<lzm::kProfSlots>(lzm::g_prof, host_slots, n);
}
#endif

#ifdef NVCOMP_LZW_PROF
/* Profiling builds only: read (and clear) the per-phase cycle sums of the window decoder. */
extern "C" int nvcompAmdProfRead(unsigned long long* host_slots, int n)
{
  return prof_read_and_clear<lzw::kProfSlots>(lzw::g_prof, host_slots, n);
}
#endif
