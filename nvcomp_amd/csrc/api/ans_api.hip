/*
 * api/ans_api.hip -- C ABI of the batched ANS codec (include/nvcomp/ans.h) and the kernels
 * it launches: one wavefront per chunk, one launch per *Async call on the caller's stream;
 * nothing here allocates or synchronises. The compress and size-query frames and the argument
 * checks are common/api_batch.hip.h; the decode kernel spells its frame out, because the compiler
 * writes it differently otherwise (profiles/api_frame_shared.md).
 */
#include <hip/hip_runtime.h>

#include "nvcomp/ans.h"

#include "common/api_batch.hip.h"
#include "common/log.h"

#include "ans/ans.hip.h"

namespace {

__global__ void __launch_bounds__(64 * kWavesPerBlock) ans_compress_kernel(
    const void* const* __restrict__ in_ptrs,
    const size_t* __restrict__ in_bytes,
    size_t max_chunk_bytes,
    size_t batch_size,
    void* const* __restrict__ out_ptrs,
    size_t* out_bytes)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][ans::kEncodeLds];
  const uint32_t w = wave::uniform(threadIdx.x >> 6);
  lzl::compress_static<kWavesPerBlock>(in_ptrs, in_bytes, max_chunk_bytes, batch_size, out_ptrs, out_bytes,
                                       [&](const uint8_t* src, uint32_t n, uint8_t* dst) -> uint32_t {
                                         return ans::encode_chunk(src, n, dst, lds[w]);
                                       });
}

__global__ void __launch_bounds__(64 * kWavesPerBlock) ans_decompress_kernel(
    const void* const* __restrict__ comp_ptrs,
    const size_t* __restrict__ comp_bytes,
    const size_t* out_caps,
    size_t* actual_bytes,
    size_t batch_size,
    void* const* __restrict__ out_ptrs,
    nvcompStatus_t* statuses)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWavesPerBlock][ans::kDecodeLds];
  const uint32_t w = wave::uniform(threadIdx.x >> 6);
  const size_t chunk = (size_t)blockIdx.x * kWavesPerBlock + w;
  if (chunk >= batch_size) {
    return;
  }
  const uint8_t* in = wave::uniform_ptr((const uint8_t*)comp_ptrs[chunk]);
  uint8_t* out = wave::uniform_ptr((uint8_t*)out_ptrs[chunk]);
  const size_t in_len64 = wave::uniform64(comp_bytes[chunk]);
  size_t cap64 = wave::uniform64(out_caps[chunk]);
  if (cap64 > ans::kMaxOutCap) {
    cap64 = ans::kMaxOutCap;
  }
  uint32_t err = ans::kErrNone;
  uint32_t produced = 0;
  if (in_len64 > 0xffffffffull - 64) {
    err = ans::kErrInput;
  } else {
    ans::MemoryOut o{out};
    produced = ans::decode_chunk(in, (uint32_t)in_len64, o, (uint32_t)cap64, lds[w], err);
  }
  if (wave::lane_id() == 0) {
    if (actual_bytes != nullptr) {
      actual_bytes[chunk] = err ? 0 : produced;
    }
    if (statuses != nullptr) {
      statuses[chunk] = err ? nvcompErrorCannotDecompress : nvcompSuccess;
    }
  }
}

__global__ void __launch_bounds__(256) ans_decompress_size_kernel(
    const void* const* __restrict__ comp_ptrs, const size_t* __restrict__ comp_bytes, size_t* out_bytes, size_t batch_size)
{
  lzl::size_by_lane(comp_ptrs, comp_bytes, out_bytes, batch_size, [](const uint8_t* in, size_t in_len) -> size_t {
    return in_len >= ans::kHeaderBytes && ans::load_as<uint32_t>(in) == ans::kMagic ? ans::load_as<uint32_t>(in + 4) : 0;
  });
}

nvcompStatus_t opts_status(nvcompBatchedANSOpts_t o, size_t max_chunk_bytes)
{
  return lzl::compress_opts_status(o.type == nvcomp_rANS, max_chunk_bytes, nvcompANSCompressionMaxAllowedChunkSize);
}

} // namespace

extern "C" {

nvcompStatus_t nvcompBatchedANSCompressGetTempSize(
    size_t /*batch_size*/, size_t max_uncompressed_chunk_bytes, nvcompBatchedANSOpts_t format_opts, size_t* temp_bytes)
{
  /* histogram and symbol table live in LDS */
  return lzl::compress_query(temp_bytes, opts_status(format_opts, max_uncompressed_chunk_bytes), [] { return 0; });
}

nvcompStatus_t nvcompBatchedANSCompressGetMaxOutputChunkSize(
    size_t max_uncompressed_chunk_bytes, nvcompBatchedANSOpts_t format_opts, size_t* max_compressed_bytes)
{
  return lzl::compress_query(max_compressed_bytes, opts_status(format_opts, max_uncompressed_chunk_bytes),
                             [&] { return ans::max_compressed_bytes(max_uncompressed_chunk_bytes); });
}

nvcompStatus_t nvcompBatchedANSCompressAsync(
    const void* const* device_uncompressed_ptrs,
    const size_t* device_uncompressed_bytes,
    size_t max_uncompressed_chunk_bytes,
    size_t batch_size,
    void* /*device_temp_ptr*/,
    size_t /*temp_bytes*/,
    void* const* device_compressed_ptrs,
    size_t* device_compressed_bytes,
    nvcompBatchedANSOpts_t format_opts,
    hipStream_t stream)
{
  nvlog::call(3, "nvcompBatchedANSCompressAsync(batch_size=%zu, max_uncompressed_chunk_bytes=%zu, stream=%p)", batch_size,
              max_uncompressed_chunk_bytes, (void*)stream);
  const nvcompStatus_t st = opts_status(format_opts, max_uncompressed_chunk_bytes);
  if (st != nvcompSuccess) {
    return st;
  }
  return lzl::checked_launch(
      batch_size, lzl::all_set(device_uncompressed_ptrs, device_uncompressed_bytes, device_compressed_ptrs, device_compressed_bytes), [&] {
        hipLaunchKernelGGL(ans_compress_kernel, dim3(grid_for(batch_size)), dim3(64 * kWavesPerBlock), 0, stream,
                           device_uncompressed_ptrs, device_uncompressed_bytes, max_uncompressed_chunk_bytes, batch_size,
                           device_compressed_ptrs, device_compressed_bytes);
      });
}

nvcompStatus_t nvcompBatchedANSDecompressGetTempSize(
    size_t /*num_chunks*/, size_t /*max_uncompressed_chunk_bytes*/, size_t* temp_bytes)
{
  return lzl::no_temp(temp_bytes); /* the decode table lives in LDS */
}

nvcompStatus_t nvcompBatchedANSDecompressAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes,
    size_t* device_actual_uncompressed_bytes,
    size_t batch_size,
    void* const /*device_temp_ptr*/,
    size_t /*temp_bytes*/,
    void* const* device_uncompressed_ptrs,
    nvcompStatus_t* device_statuses,
    hipStream_t stream)
{
  nvlog::call(3, "nvcompBatchedANSDecompressAsync(batch_size=%zu, statuses=%s, actual_sizes=%s, stream=%p)", batch_size,
              device_statuses ? "yes" : "null", device_actual_uncompressed_bytes ? "yes" : "null", (void*)stream);
  return lzl::checked_launch(
      batch_size, lzl::all_set(device_compressed_ptrs, device_compressed_bytes, device_uncompressed_bytes, device_uncompressed_ptrs), [&] {
        hipLaunchKernelGGL(ans_decompress_kernel, dim3(grid_for(batch_size)), dim3(64 * kWavesPerBlock), 0, stream,
                           device_compressed_ptrs, device_compressed_bytes, device_uncompressed_bytes,
                           device_actual_uncompressed_bytes, batch_size, device_uncompressed_ptrs, device_statuses);
      });
}

nvcompStatus_t nvcompBatchedANSGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes,
    size_t batch_size,
    hipStream_t stream)
{
  return lzl::size_by_lane_async<ans_decompress_size_kernel>(device_compressed_ptrs, device_compressed_bytes,
                                                             device_uncompressed_bytes, batch_size, stream);
}

NVCOMP_API_COMPRESS_TEMP_SIZE_EX(ANS, nvcompBatchedANSOpts_t)
NVCOMP_API_DECOMPRESS_TEMP_SIZE_EX(ANS)

} // extern "C"
