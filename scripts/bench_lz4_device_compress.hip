/*
 * scripts/bench_lz4_device_compress.hip -- kernels of scripts/bench_lz4_device_compress.py: the compressor of the
 * device-side LZ4 API (include/nvcomp/device/lz4.hpp) against the batched call. Built with hipcc --offload-arch=gfx950
 * -I include alone.
 *
 *   plain_compress   compress() per wave, global -> global: the header-only path itself, against the batched call
 *   fused_shuffle    one wave per workgroup: the chunk's 4-byte elements byte-transposed into planes in 64 KiB of LDS,
 *                    compress() from there; only the block goes to HBM
 *   shuffle_to_hbm   the first kernel of the two-kernel path: the same planes written to HBM, for the batched call
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <nvcomp/device/lz4.hpp>

namespace lz4dev = nvcomp::device::lz4;

namespace {

constexpr unsigned kWaves = 4; /* the batched kernels' launch shape: four waves a workgroup, one chunk each */
constexpr size_t kChunk = 1 << 16;

/* planes[b * elems + i] = byte b of words[i], by one wave */
__device__ inline void shuffle_chunk(const uint32_t* words, uint8_t* planes, unsigned lane)
{
  constexpr size_t elems = kChunk / 4;
  for (size_t i = lane; i < elems; i += 64) {
    const uint32_t w = words[i];
    planes[i] = (uint8_t)w;
    planes[elems + i] = (uint8_t)(w >> 8);
    planes[2 * elems + i] = (uint8_t)(w >> 16);
    planes[3 * elems + i] = (uint8_t)(w >> 24);
  }
}

__global__ void __launch_bounds__(64 * kWaves) plain_compress(const uint8_t* data, size_t num_chunks, uint8_t* comp, size_t slot_bytes,
                                                              size_t* comp_bytes)
{
  __shared__ __attribute__((aligned(16))) uint8_t scratch[kWaves][lz4dev::kCompressSharedBytes];
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  const size_t size = lz4dev::compress(data + c * kChunk, kChunk, comp + c * slot_bytes, scratch[w]);
  if (threadIdx.x % 64 == 0) {
    comp_bytes[c] = size;
  }
}

__global__ void __launch_bounds__(64) fused_shuffle(const uint8_t* data, uint8_t* comp, size_t slot_bytes, size_t* comp_bytes)
{
  __shared__ __attribute__((aligned(16))) uint8_t planes[kChunk];
  __shared__ __attribute__((aligned(16))) uint8_t scratch[lz4dev::kCompressSharedBytes];
  const unsigned lane = threadIdx.x;
  const size_t c = blockIdx.x;
  shuffle_chunk((const uint32_t*)(data + c * kChunk), planes, lane);
  lz4dev::wave_sync();
  const size_t size = lz4dev::compress(planes, kChunk, comp + c * slot_bytes, scratch);
  if (lane == 0) {
    comp_bytes[c] = size;
  }
}

__global__ void __launch_bounds__(64 * kWaves) shuffle_to_hbm(const uint8_t* data, size_t num_chunks, uint8_t* shuffled)
{
  const unsigned lane = threadIdx.x % 64;
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  shuffle_chunk((const uint32_t*)(data + c * kChunk), shuffled + c * kChunk, lane);
}

} // namespace

extern "C" {

int bench_plain(const uint8_t* data, size_t num_chunks, uint8_t* comp, size_t slot_bytes, size_t* comp_bytes, hipStream_t stream)
{
  hipLaunchKernelGGL(plain_compress, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, data,
                     num_chunks, comp, slot_bytes, comp_bytes);
  return (int)hipGetLastError();
}

int bench_fused(const uint8_t* data, size_t num_chunks, uint8_t* comp, size_t slot_bytes, size_t* comp_bytes, hipStream_t stream)
{
  hipLaunchKernelGGL(fused_shuffle, dim3((unsigned)num_chunks), dim3(64), 0, stream, data, comp, slot_bytes, comp_bytes);
  return (int)hipGetLastError();
}

int bench_shuffle(const uint8_t* data, size_t num_chunks, uint8_t* shuffled, hipStream_t stream)
{
  hipLaunchKernelGGL(shuffle_to_hbm, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, data,
                     num_chunks, shuffled);
  return (int)hipGetLastError();
}

size_t bench_slot_bytes(void)
{
  return lz4dev::max_compressed_bytes(kChunk);
}

} // extern "C"
