/*
 * scripts/bench_bitcomp_device.hip -- kernels of scripts/bench_bitcomp_device.py: the device-side Bitcomp API
 * (include/nvcomp/device/bitcomp.hpp) against the batched call. Built with hipcc --offload-arch=gfx950 -I include alone.
 *
 *   fused_decode_axpy   one wave per chunk: decompress_to<int32_t> with a sink y[i] += a * (q * delta)
 *   axpy_from_ints      the second kernel of the two-kernel path: reads the int32 buffer the batched decoder wrote
 *   plain_decompress    decompress() per wave into memory: the header-only path itself, against the batched call
 *
 * The arithmetic order is y + (a * (q * delta)), each step rounded once, in both paths.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <nvcomp/device/bitcomp.hpp>

namespace bc = nvcomp::device::bitcomp;

namespace {

constexpr unsigned kWaves = 4; /* the batched kernels' launch shape: four waves a workgroup, one chunk each */

__device__ inline float add_product(float y, float a, float t)
{
#pragma clang fp contract(off)
  const float p = a * t;
  return y + p;
}

__global__ void __launch_bounds__(64 * kWaves, 8) fused_decode_axpy(const void* const* comp, const size_t* comp_bytes,
                                                                    float* y, size_t chunk_bytes, size_t num_chunks, float a,
                                                                    float delta, int* status)
{
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  float* ys = y + c * (chunk_bytes / 4);
  const nvcompStatus_t st = bc::decompress_to<int32_t>(comp[c], comp_bytes[c], chunk_bytes, nullptr, nullptr, [&](uint32_t i, int32_t q) {
    ys[i] = add_product(ys[i], a, bc::dequantize(q, delta));
  });
  if (threadIdx.x % 64 == 0) {
    status[c] = (int)st;
  }
}

__global__ void __launch_bounds__(256) axpy_from_ints(const int32_t* q, float* y, size_t n, float a, float delta)
{
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    y[i] = add_product(y[i], a, bc::dequantize(q[i], delta));
  }
}

__global__ void __launch_bounds__(64 * kWaves, 8) plain_decompress(const void* const* comp, const size_t* comp_bytes,
                                                                   uint8_t* out, size_t chunk_bytes, size_t num_chunks,
                                                                   int* status)
{
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  const nvcompStatus_t st = bc::decompress(comp[c], comp_bytes[c], out + c * chunk_bytes, chunk_bytes, nullptr);
  if (threadIdx.x % 64 == 0) {
    status[c] = (int)st;
  }
}

} // namespace

extern "C" {

int bench_fused(const void* const* comp, const size_t* comp_bytes, float* y, size_t chunk_bytes, size_t num_chunks, float a,
                float delta, int* status, hipStream_t stream)
{
  hipLaunchKernelGGL(fused_decode_axpy, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, comp,
                     comp_bytes, y, chunk_bytes, num_chunks, a, delta, status);
  return (int)hipGetLastError();
}

int bench_axpy(const int32_t* q, float* y, size_t n, float a, float delta, unsigned grid, hipStream_t stream)
{
  hipLaunchKernelGGL(axpy_from_ints, dim3(grid), dim3(256), 0, stream, q, y, n, a, delta);
  return (int)hipGetLastError();
}

int bench_plain(const void* const* comp, const size_t* comp_bytes, uint8_t* out, size_t chunk_bytes, size_t num_chunks,
                int* status, hipStream_t stream)
{
  hipLaunchKernelGGL(plain_decompress, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream, comp,
                     comp_bytes, out, chunk_bytes, num_chunks, status);
  return (int)hipGetLastError();
}

} // extern "C"
