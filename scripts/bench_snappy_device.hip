/*
 * scripts/bench_snappy_device.hip -- kernels of scripts/bench_snappy_device.py: the device-side Snappy API
 * (include/nvcomp/device/snappy.hpp) against the batched calls. Built with hipcc --offload-arch=gfx950 -I include alone.
 *
 *   plain_decompress    decompress() per wave, global -> global: the header-only path itself, against the batched call
 *   fused_histogram     one wave per workgroup: decompress() into 64 KiB of LDS, a 256-bin histogram counted from there
 *   histogram_from_hbm  the second kernel of the two-kernel path: reads the chunk the batched decoder wrote to HBM
 *   plain_compress      compress() per wave, global -> global, against the batched compressor
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <nvcomp/device/snappy.hpp>

namespace snpdev = nvcomp::device::snappy;

namespace {

constexpr unsigned kWaves = 4; /* the batched kernels' launch shape: four waves a workgroup, one chunk each */
constexpr size_t kChunk = 1 << 16;

/* bins[] += the bytes of words[0, n / 4) (n % 4 == 0), by one wave */
__device__ inline void count_words(const uint32_t* words, size_t n, uint32_t* bins, unsigned lane)
{
  for (size_t i = lane; i < n / 4; i += 64) {
    const uint32_t w = words[i];
    atomicAdd(&bins[w & 255u], 1u);
    atomicAdd(&bins[(w >> 8) & 255u], 1u);
    atomicAdd(&bins[(w >> 16) & 255u], 1u);
    atomicAdd(&bins[w >> 24], 1u);
  }
}

__global__ void __launch_bounds__(64 * kWaves) plain_decompress(const void* const* comp, const size_t* comp_bytes, uint8_t* out,
                                                                size_t chunk_bytes, size_t num_chunks, int* status)
{
  __shared__ __attribute__((aligned(16))) uint8_t scratch[kWaves][snpdev::kDecompressSharedBytes];
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  const nvcompStatus_t st = snpdev::decompress(comp[c], comp_bytes[c], out + c * chunk_bytes, chunk_bytes, nullptr, scratch[w]);
  if (threadIdx.x % 64 == 0) {
    status[c] = (int)st;
  }
}

__global__ void __launch_bounds__(64) fused_histogram(const void* const* comp, const size_t* comp_bytes, uint32_t* histograms,
                                                      int* status)
{
  __shared__ __attribute__((aligned(16))) uint8_t chunk[kChunk];
  __shared__ __attribute__((aligned(16))) uint8_t scratch[snpdev::kDecompressSharedBytes];
  __shared__ uint32_t bins[256];
  const unsigned lane = threadIdx.x;
  const size_t c = blockIdx.x;
  for (unsigned i = lane; i < 256; i += 64) {
    bins[i] = 0;
  }
  size_t n = 0;
  const nvcompStatus_t st = snpdev::decompress(comp[c], comp_bytes[c], chunk, kChunk, &n, scratch);
  snpdev::wave_sync();
  count_words((const uint32_t*)chunk, st == nvcompSuccess ? n : 0, bins, lane);
  snpdev::wave_sync();
  for (unsigned i = lane; i < 256; i += 64) {
    histograms[c * 256 + i] = bins[i];
  }
  if (lane == 0) {
    status[c] = (int)st;
  }
}

__global__ void __launch_bounds__(64 * kWaves) histogram_from_hbm(const uint8_t* data, size_t chunk_bytes, size_t num_chunks,
                                                                  uint32_t* histograms)
{
  __shared__ uint32_t bins[kWaves][256];
  const unsigned lane = threadIdx.x % 64;
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  for (unsigned i = lane; i < 256; i += 64) {
    bins[w][i] = 0;
  }
  snpdev::wave_sync();
  count_words((const uint32_t*)(data + c * chunk_bytes), chunk_bytes, bins[w], lane);
  snpdev::wave_sync();
  for (unsigned i = lane; i < 256; i += 64) {
    histograms[c * 256 + i] = bins[w][i];
  }
}

__global__ void __launch_bounds__(64 * kWaves) plain_compress(const uint8_t* data, size_t chunk_bytes, size_t num_chunks,
                                                              uint8_t* out, size_t slot_bytes, size_t* sizes)
{
  __shared__ __attribute__((aligned(16))) uint8_t scratch[kWaves][snpdev::kCompressSharedBytes];
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  const size_t got = snpdev::compress(data + c * chunk_bytes, chunk_bytes, out + c * slot_bytes, scratch[w]);
  if (threadIdx.x % 64 == 0) {
    sizes[c] = got;
  }
}

} // namespace

extern "C" {

int bench_plain(const void* const* comp, const size_t* comp_bytes, uint8_t* out, size_t chunk_bytes, size_t num_chunks,
                int* status, hipStream_t stream)
{
  hipLaunchKernelGGL(plain_decompress, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, comp,
                     comp_bytes, out, chunk_bytes, num_chunks, status);
  return (int)hipGetLastError();
}

int bench_fused(const void* const* comp, const size_t* comp_bytes, uint32_t* histograms, size_t num_chunks, int* status,
                hipStream_t stream)
{
  hipLaunchKernelGGL(fused_histogram, dim3((unsigned)num_chunks), dim3(64), 0, stream, comp, comp_bytes, histograms, status);
  return (int)hipGetLastError();
}

int bench_histogram(const uint8_t* data, size_t chunk_bytes, size_t num_chunks, uint32_t* histograms, hipStream_t stream)
{
  hipLaunchKernelGGL(histogram_from_hbm, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, data,
                     chunk_bytes, num_chunks, histograms);
  return (int)hipGetLastError();
}

int bench_compress(const uint8_t* data, size_t chunk_bytes, size_t num_chunks, uint8_t* out, size_t slot_bytes, size_t* sizes,
                   hipStream_t stream)
{
  if (slot_bytes < snpdev::max_compressed_bytes(chunk_bytes)) {
    return -1;
  }
  hipLaunchKernelGGL(plain_compress, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, data,
                     chunk_bytes, num_chunks, out, slot_bytes, sizes);
  return (int)hipGetLastError();
}

} // extern "C"
