/*
 * api/zstd_api.hip -- C ABI of the batched Zstandard decoder (include/nvcomp/zstd.h) and the kernels it launches. Host
 * side does argument checks, one 4-byte memset of the ticket counter and one launch per *Async call on the caller's
 * stream; nothing here allocates or synchronises. The batch, the ticket and the argument checks are common/api_batch.hip.h;
 * the kernels spell their frames out, because the compiler writes them differently otherwise (profiles/api_frame_shared.md).
 */
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include "nvcomp/zstd.h"

#include "common/api_batch.hip.h"
#include "common/log.h"

#include "zstd/zstd_decode.hip.h"

namespace {

/* One wave per workgroup (chunks of a mixed batch take very different times: api/deflate_api.hip), persistent: a wave
 * that finishes a chunk draws the next one from the ticket counter (common/api_batch.hip.h). zstd::kLdsPerWave =
 * 9.1 KiB would allow 17 waves per CU; the registers (130 VGPRs, no scratch) allow 3 per SIMD = 12 per CU. */
constexpr unsigned kDecWavesPerSimd = 3;
constexpr size_t kMaxSlot = zstd::kBlockMax;

struct ZstdLaunch : lzl::Tickets /* first_dynamic = waves of the launch */
{
  uint8_t* slots; /* slot_bytes per wave of the launch */
  size_t slot_bytes;
};

/* The bounds and offset checks always run (Zstd chunks come from outside); only the status WRITE depends on `statuses`. */
__global__ void __launch_bounds__(64, kDecWavesPerSimd) zstd_decompress_kernel(const ZstdLaunch launch)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[zstd::kLdsPerWave];
  const size_t wave_id = blockIdx.x;
  size_t chunk = wave_id;
  for (;;) {
    const auto* a = wave::kernel_args(launch);
    if (chunk >= a->b.batch_size) {
      break;
    }
    const uint8_t* in = wave::uniform_ptr((const uint8_t*)a->b.comp_ptrs[chunk]);
    uint8_t* out = wave::uniform_ptr((uint8_t*)a->b.out_ptrs[chunk]);
    const size_t in_len64 = wave::uniform64(a->b.comp_bytes[chunk]);
    size_t cap64 = wave::uniform64(a->b.out_caps[chunk]);
    if (cap64 > lzl::kMaxOutCap) {
      cap64 = lzl::kMaxOutCap;
    }
    uint8_t* slot = wave::uniform_ptr(a->slots + wave_id * a->slot_bytes);
    const uint32_t slot_cap = (uint32_t)a->slot_bytes;
    uint32_t err = lz::kErrNone;
    uint32_t produced = 0;
    if (in_len64 > (1u << 28)) {
      err = lz::kErrInput;
    } else {
      produced = zstd::decode_chunk(in, (uint32_t)in_len64, out, (uint32_t)cap64, lds, slot, slot_cap, err);
    }
    a = wave::kernel_args(launch);
    if (wave::lane_id() == 0) {
      if (a->b.actual_bytes != nullptr) {
        a->b.actual_bytes[chunk] = err ? 0 : produced;
      }
      if (a->b.statuses != nullptr) {
        a->b.statuses[chunk] = err == 0 ? nvcompSuccess : (err & zstd::kUnsupported) ? nvcompErrorNotSupported : nvcompErrorCannotDecompress;
      }
    }
    uint32_t* ticket = a->ticket;
    if (ticket == nullptr) {
      break;
    }
    chunk = lzl::next_chunk(ticket, a->first_dynamic);
  }
}

/* Size query: one lane per chunk walks the frame and block headers (no entropy data). */
__global__ void __launch_bounds__(256) zstd_size_kernel(
    const void* const* __restrict__ comp_ptrs, const size_t* __restrict__ comp_bytes, size_t* uncompressed_bytes, size_t batch_size)
{
  const size_t chunk = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (chunk >= batch_size) {
    return;
  }
  const size_t n = comp_bytes[chunk];
  uncompressed_bytes[chunk] = n > (1u << 28) ? 0 : zstd::content_size((const uint8_t*)comp_ptrs[chunk], (uint32_t)n);
}

size_t slot_for(size_t max_chunk)
{
  const size_t s = max_chunk < kMaxSlot ? max_chunk : kMaxSlot;
  return ((s > 16 ? s : 16) + 15) & ~(size_t)15;
}

} // namespace

extern "C" {

nvcompStatus_t nvcompBatchedZstdDecompressGetTempSize(size_t num_chunks, size_t max_uncompressed_chunk_bytes, size_t* temp_bytes)
{
  nvlog::call(3, "nvcompBatchedZstdDecompressGetTempSize(num_chunks=%zu, max_uncompressed_chunk_bytes=%zu)", num_chunks,
              max_uncompressed_chunk_bytes);
  if (temp_bytes == nullptr || max_uncompressed_chunk_bytes > nvcompZstdCompressionMaxAllowedChunkSize) {
    return nvcompErrorInvalidValue;
  }
  const size_t waves = num_chunks < zstd::kMaxWaves ? num_chunks : zstd::kMaxWaves;
  *temp_bytes = zstd::kTempHeader + (waves ? waves : 1) * slot_for(max_uncompressed_chunk_bytes);
  return nvcompSuccess;
}

nvcompStatus_t nvcompBatchedZstdDecompressGetTempSizeEx(
    size_t num_chunks, size_t max_uncompressed_chunk_bytes, size_t* temp_bytes, size_t max_total_uncompressed_bytes)
{
  nvlog::call(3, "nvcompBatchedZstdDecompressGetTempSizeEx(num_chunks=%zu, max_uncompressed_chunk_bytes=%zu, max_total=%zu)",
              num_chunks, max_uncompressed_chunk_bytes, max_total_uncompressed_bytes);
  /* no block regenerates more literals than the whole batch holds */
  const size_t m = max_total_uncompressed_bytes < max_uncompressed_chunk_bytes ? max_total_uncompressed_bytes : max_uncompressed_chunk_bytes;
  return nvcompBatchedZstdDecompressGetTempSize(num_chunks, m, temp_bytes);
}

nvcompStatus_t nvcompBatchedZstdDecompressAsync(
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
  nvlog::call(3, "nvcompBatchedZstdDecompressAsync(batch_size=%zu, temp_bytes=%zu, statuses=%s, actual_sizes=%s, stream=%p)",
              batch_size, temp_bytes, device_statuses ? "yes" : "null", device_actual_uncompressed_bytes ? "yes" : "null",
              (void*)stream);
  const bool arrays_ok = lzl::all_set(device_compressed_ptrs, device_compressed_bytes, device_uncompressed_bytes, device_uncompressed_ptrs,
                                      device_temp_ptr)
                         && ((uintptr_t)device_temp_ptr & 15u) == 0 && temp_bytes >= zstd::kTempHeader + 16;
  return lzl::checked_launch(batch_size, arrays_ok, [&]() -> nvcompStatus_t {
    /* as many waves as stay resident (at most kMaxWaves, at most one per chunk), each with its literal slot */
    static lzl::ResidentCache resident; /* per device ordinal */
    size_t waves = resident.get(zstd_decompress_kernel, 64, 0);
    if (waves == 0 || waves > zstd::kMaxWaves) {
      waves = zstd::kMaxWaves;
    }
    if (waves > batch_size) {
      waves = batch_size;
    }
    size_t slot = ((temp_bytes - zstd::kTempHeader) / waves) & ~(size_t)15;
    if (slot > kMaxSlot) {
      slot = kMaxSlot;
    }
    if (slot < 16) { /* a buffer sized for fewer chunks than the launch has waves: fewer waves */
      slot = 16;
      waves = (temp_bytes - zstd::kTempHeader) / slot;
    }
    uint32_t* ticket = nullptr;
    if (waves < batch_size) {
      if (hipMemsetAsync(device_temp_ptr, 0, sizeof(uint32_t), stream) != hipSuccess) {
        return nvcompErrorCudaError;
      }
      ticket = (uint32_t*)device_temp_ptr;
    }
    const lzl::Batch b = {device_compressed_ptrs, device_compressed_bytes, device_uncompressed_bytes,
                          device_actual_uncompressed_bytes, batch_size, device_uncompressed_ptrs, (int*)device_statuses};
    const ZstdLaunch launch = {{b, ticket, waves}, (uint8_t*)device_temp_ptr + zstd::kTempHeader, slot};
    hipLaunchKernelGGL(zstd_decompress_kernel, dim3((unsigned)waves), dim3(64), 0, stream, launch);
    return nvcompSuccess;
  });
}

nvcompStatus_t nvcompBatchedZstdGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes,
    size_t batch_size,
    hipStream_t stream)
{
  nvlog::call(3, "nvcompBatchedZstdGetDecompressSizeAsync(batch_size=%zu, stream=%p)", batch_size, (void*)stream);
  return lzl::size_by_lane_async<zstd_size_kernel>(device_compressed_ptrs, device_compressed_bytes, device_uncompressed_bytes,
                                                   batch_size, stream);
}

} // extern "C"
