/*
 * api/snappy_api.hip -- C ABI of the batched Snappy codec (include/nvcomp/snappy.h) and
 * the kernels it launches. Host side does argument checks and one launch per
 * *Async call on the caller's stream; nothing here allocates or synchronises.
 * What Snappy shares with LZ4 (kernel bodies, dispatch) is common/lz_api.hip.h, what with every format common/api_batch.hip.h.
 */
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "nvcomp/snappy.h"

#include "nvcomp/amd_ext.h"

#include "common/lz_api.hip.h"
#include "snappy/snappy_decode_window.hip.h"
#include "snappy/snappy_encode.hip.h"
#include "snappy/snappy_preamble.hip.h"

namespace {

using lzl::kDecWaves;
using lzl::kEncWaves;
using lzl::kWideWaves;

#ifndef NVCOMP_SNAPPY_RUNS_RATIO
#define NVCOMP_SNAPPY_RUNS_RATIO 8
#endif
constexpr size_t kRunsRatio = NVCOMP_SNAPPY_RUNS_RATIO;

/* Snappy as common/lz_api.hip.h sees it. */
struct Snappy
{
  using FrontEnd = snappyw::FrontEnd;
  static constexpr bool kPairRuns = false; /* the runs of a typed column go to alone() */
  static constexpr bool kEmptyIsError = true; /* an empty stream has no preamble: malformed */
  /* a chunk that shrank 8 x or more takes the instance of the loop that tries the run executor (snappyw::decode_chunk) */
  static __device__ __forceinline__ bool runs(size_t in_len, size_t cap)
  {
    return NVCOMP_LZW_RUNS && in_len * kRunsRatio <= cap;
  }
  template <bool CHECKED>
  static __device__ __forceinline__ uint32_t alone(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, uint8_t* lds, uint32_t& err)
  {
    return snappyw::decode_chunk<CHECKED, true>(in, n, out, cap, lds, err);
  }
};

template <bool CHECKED>
__global__ void __launch_bounds__(64 * kDecWaves, NVCOMP_LZW_WAVES_PER_SIMD) snappy_decompress_window_kernel(const lzl::Tickets launch)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kDecWaves][lzw::kLdsPerWave];
  const uint32_t w = wave::uniform(threadIdx.x >> 6);
  lzl::decode_window_loop<CHECKED>(launch, w, [&](const lzl::Chunk& c, uint32_t& err) -> uint32_t {
    if (Snappy::runs(c.in_len, c.cap)) {
      return snappyw::decode_chunk<CHECKED, true>(c.in, (uint32_t)c.in_len, c.out, (uint32_t)c.cap, lds[w], err);
    }
    return snappyw::decode_chunk<CHECKED, false>(c.in, (uint32_t)c.in_len, c.out, (uint32_t)c.cap, lds[w], err);
  });
}

template <bool CHECKED, uint32_t WAVES>
__global__ void __launch_bounds__(64 * WAVES, 4) snappy_decompress_team_kernel(const lzl::Tickets launch)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[lzt::Geo<WAVES>::kLds];
  lzl::decode_team_loop<CHECKED, WAVES, Snappy>(launch, lds);
}

template <bool CHECKED>
__global__ void __launch_bounds__(128, 7) snappy_decompress_pair_kernel(const lzl::Batch b)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[lzw::pair::kLdsPerChunk];
  lzl::decode_pair<CHECKED, Snappy>(b, lds);
}

__global__ void __launch_bounds__(64 * kWavesPerBlock) snappy_decompress_size_kernel(
    const void* const* __restrict__ comp_ptrs,
    const size_t* __restrict__ comp_bytes,
    size_t* uncompressed_bytes,
    size_t batch_size)
{
  lzl::decompress_size(comp_ptrs, comp_bytes, uncompressed_bytes, batch_size, [](const uint8_t* in, uint32_t in_len) -> uint32_t {
    bool ok;
    return snappy::decoded_size(in, in_len, ok); /* preamble only */
  });
}

/* The one-window compressor (common/lz_match.hip.h). No call launches it since untyped data -- all of Snappy's -- takes the
 * wide steps below (its A/B switch is retired: DESIGN.md, "retired switches"). It is still compiled: without it in the
 * module the compiler writes one condition of snappy_compress_wide_kernel differently (profiles/lz_switches_retired.md). */
__global__ void __launch_bounds__(64 * kEncWaves, NVCOMP_LZM_WAVES_PER_SIMD) snappy_compress_kernel(const lzl::CompressLaunch launch)
{
  __shared__ uint16_t tables[kEncWaves][lzm::kTableU16];
  __shared__ __attribute__((aligned(8))) uint8_t images[kEncWaves][lzm::kImageBytes];
  const uint32_t w = wave::uniform(threadIdx.x >> 6);
  lzl::compress_loop<kEncWaves>(launch, w, [&](const uint8_t* src, uint32_t n, uint8_t* dst) -> uint32_t {
    return snappy::encode_chunk(src, n, dst, tables[w], images[w]);
  });
}

/* Untyped data: 256-position steps (common/lz_match_wide.hip.h); a wave's LDS is lzm::wide::kLdsPerWave bytes. */
__global__ void __launch_bounds__(64 * kWideWaves, NVCOMP_LZMW_WAVES_PER_SIMD) snappy_compress_wide_kernel(const lzl::CompressLaunch launch)
{
  __shared__ uint16_t tables[kWideWaves][lzm::wide::kEntries];
  __shared__ __attribute__((aligned(16))) uint8_t images[kWideWaves][lzm::wide::kImage];
  __shared__ __attribute__((aligned(16))) uint8_t scratch[kWideWaves][lzm::wide::kScratch];
  const uint32_t w = wave::uniform(threadIdx.x >> 6);
  lzl::compress_loop<kWideWaves>(launch, w, [&](const uint8_t* src, uint32_t n, uint8_t* dst) -> uint32_t {
    return snappy::encode_chunk_wide(src, n, dst, tables[w], images[w], scratch[w]);
  });
}

nvcompStatus_t snappy_opts_status(nvcompBatchedSnappyOpts_t opts, size_t max_chunk_bytes)
{
  return lzl::compress_opts_status(opts.reserved == 0, max_chunk_bytes, nvcompSnappyCompressionMaxAllowedChunkSize);
}

} // namespace

extern "C" {

nvcompStatus_t nvcompBatchedSnappyDecompressGetTempSize(
    size_t num_chunks, size_t /*max_uncompressed_chunk_bytes*/, size_t* temp_bytes)
{
  /* the ticket counter of the persistent waves / workgroups (common/lz_launch.hip.h) and the order they hand out in; the
   * decoder itself keeps all state in registers and LDS */
  return lzl::temp_size(num_chunks, temp_bytes, lzl::order_query_bytes(num_chunks));
}

NVCOMP_API_DECOMPRESS_TEMP_SIZE_EX(Snappy)

nvcompStatus_t nvcompBatchedSnappyDecompressAsync(
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
  return lzl::decompress_async<snappy_decompress_team_kernel<true, 16>, snappy_decompress_team_kernel<true, 8>,
                               snappy_decompress_pair_kernel<true>, snappy_decompress_window_kernel<true>>(
      "Snappy", device_compressed_ptrs, device_compressed_bytes, device_uncompressed_bytes,
      device_actual_uncompressed_bytes, batch_size, device_temp_ptr, temp_bytes, device_uncompressed_ptrs, device_statuses, stream);
}

nvcompStatus_t nvcompAmdSnappyDecompressOrderAsync(
    const size_t* device_compressed_bytes, const size_t* device_uncompressed_bytes, size_t first_ordered, size_t batch_size,
    void* device_temp_ptr, size_t temp_bytes, size_t* order_offset, size_t* resident_places, hipStream_t stream)
{
  return lzl::order_inspect_async<snappy_decompress_window_kernel<true>>(
      device_compressed_bytes, device_uncompressed_bytes, first_ordered, batch_size, device_temp_ptr, temp_bytes, order_offset,
      resident_places, stream);
}

nvcompStatus_t nvcompBatchedSnappyGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes,
    size_t batch_size,
    hipStream_t stream)
{
  return lzl::decompress_size_async<snappy_decompress_size_kernel>(device_compressed_ptrs, device_compressed_bytes,
                                                                   device_uncompressed_bytes, batch_size, stream);
}

nvcompStatus_t nvcompBatchedSnappyCompressGetTempSize(
    size_t batch_size, size_t max_uncompressed_chunk_bytes, nvcompBatchedSnappyOpts_t format_opts, size_t* temp_bytes)
{
  return lzl::compress_query(temp_bytes, snappy_opts_status(format_opts, max_uncompressed_chunk_bytes),
                             [&] { return batch_size == 0 ? 0 : lzl::kTicketBytes; });
}

NVCOMP_API_COMPRESS_TEMP_SIZE_EX(Snappy, nvcompBatchedSnappyOpts_t)

nvcompStatus_t nvcompBatchedSnappyCompressGetMaxOutputChunkSize(
    size_t max_uncompressed_chunk_bytes, nvcompBatchedSnappyOpts_t format_opts, size_t* max_compressed_bytes)
{
  /* the raw format's classic bound: preamble + literal headers */
  return lzl::compress_query(max_compressed_bytes, snappy_opts_status(format_opts, max_uncompressed_chunk_bytes),
                             [&] { return 32 + max_uncompressed_chunk_bytes + max_uncompressed_chunk_bytes / 6; });
}

nvcompStatus_t nvcompBatchedSnappyCompressAsync(
    const void* const* device_uncompressed_ptrs,
    const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    void* const* device_compressed_ptrs,
    size_t* device_compressed_bytes,
    nvcompBatchedSnappyOpts_t format_opts,
    hipStream_t stream)
{
  const lzl::CompressCall call = {"Snappy", snappy_opts_status(format_opts, max_uncompressed_chunk_bytes), device_uncompressed_ptrs,
                                  device_uncompressed_bytes, max_uncompressed_chunk_bytes, batch_size, device_temp_ptr, temp_bytes,
                                  device_compressed_ptrs, device_compressed_bytes, stream};
  return lzl::compress_async<snappy_compress_wide_kernel, kWideWaves>(call);
}

} // extern "C"

#ifdef NVCOMP_LZW_PROF
/* Profiling builds only: read (and clear) the per-phase cycle sums of the Snappy window decoder. */
extern "C" int nvcompAmdProfReadSnappy(unsigned long long* host_slots, int n)
{
  return prof_read_and_clear<lzw::kProfSlots>(lzw::g_prof, host_slots, n);
}
#endif
