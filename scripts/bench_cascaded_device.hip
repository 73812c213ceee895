/*
 * scripts/bench_cascaded_device.hip -- kernels of scripts/bench_cascaded_device.py: the device-side Cascaded API
 * (include/nvcomp/device/cascaded.hpp) against the batched calls. Built with hipcc --offload-arch=gfx950 -I include alone.
 *
 *   fused_filter_sum    one wave per chunk: decompress_to<int32_t> with a sink that adds up the values in [lo, hi)
 *   filter_sum_ints     the second kernel of the two-kernel path: one wave per chunk reads the int32 buffer the batched
 *                       decoder wrote and computes the same sum
 *   plain_decompress    decompress() per wave into memory: the header-only path itself, against the batched call
 *   plain_compress      compress() per wave, against nvcompBatchedCascadedCompressAsync
 *
 * The decoders get the LDS slice of the batched decoder's first pass (5 KiB a wave, eight workgroups a CU), the compressor
 * that of the batched compressor's first pass (6 400 bytes, six workgroups): a user kernel has no later pass to hand a
 * chunk to, so a chunk that does not fit is reported (the script checks that none is).
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <nvcomp/device/cascaded.hpp>

namespace casc = nvcomp::device::cascaded;

namespace {

constexpr unsigned kWaves = 4; /* the batched kernels' launch shape: four waves a workgroup, one chunk each */
constexpr unsigned kDecSlice = 5 * 1024;
constexpr unsigned kCompSlice = 6400;

__device__ inline long long wave_sum(long long v)
{
  for (int off = 32; off >= 1; off >>= 1) {
    v += __shfl_xor(v, off);
  }
  return v;
}

__global__ void __launch_bounds__(64 * kWaves, 8) fused_filter_sum(const void* const* comp, const size_t* comp_bytes,
                                                                   size_t chunk_bytes, size_t num_chunks, int32_t lo, int32_t hi,
                                                                   long long* sums, int* status)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWaves][kDecSlice];
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  long long sum = 0;
  const nvcompStatus_t st = casc::decompress_to<int32_t>(comp[c], comp_bytes[c], chunk_bytes, nullptr, lds[w], kDecSlice,
                                                         [&](uint32_t, int32_t v) { sum += (v >= lo && v < hi) ? v : 0; });
  sum = wave_sum(sum);
  if (threadIdx.x % 64 == 0) {
    sums[c] = sum;
    status[c] = (int)st;
  }
}

__global__ void __launch_bounds__(64 * kWaves, 8) filter_sum_ints(const int32_t* values, size_t chunk_bytes, size_t num_chunks,
                                                                  int32_t lo, int32_t hi, long long* sums)
{
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  const int4* v = (const int4*)(values + c * (chunk_bytes / 4));
  long long sum = 0;
  for (size_t i = threadIdx.x % 64; i < chunk_bytes / 16; i += 64) {
    const int4 q = v[i];
    sum += (q.x >= lo && q.x < hi) ? q.x : 0;
    sum += (q.y >= lo && q.y < hi) ? q.y : 0;
    sum += (q.z >= lo && q.z < hi) ? q.z : 0;
    sum += (q.w >= lo && q.w < hi) ? q.w : 0;
  }
  sum = wave_sum(sum);
  if (threadIdx.x % 64 == 0) {
    sums[c] = sum;
  }
}

__global__ void __launch_bounds__(64 * kWaves, 8) plain_decompress(const void* const* comp, const size_t* comp_bytes, uint8_t* out,
                                                                   size_t chunk_bytes, size_t num_chunks, int* status)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWaves][kDecSlice];
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  const nvcompStatus_t st = casc::decompress(comp[c], comp_bytes[c], out + c * chunk_bytes, chunk_bytes, nullptr, lds[w], kDecSlice);
  if (threadIdx.x % 64 == 0) {
    status[c] = (int)st;
  }
}

__global__ void __launch_bounds__(64 * kWaves, 6) plain_compress(const uint8_t* in, size_t chunk_bytes, size_t num_chunks,
                                                                 void* const* out, size_t* out_bytes,
                                                                 nvcompBatchedCascadedOpts_t opts)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWaves][kCompSlice];
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t c = (size_t)blockIdx.x * kWaves + w;
  if (c >= num_chunks) {
    return;
  }
  const size_t n = casc::compress(in + c * chunk_bytes, chunk_bytes, out[c], opts, lds[w], kCompSlice);
  if (threadIdx.x % 64 == 0) {
    out_bytes[c] = n;
  }
}

unsigned grid_for(size_t num_chunks)
{
  return (unsigned)((num_chunks + kWaves - 1) / kWaves);
}

} // namespace

extern "C" {

int bench_fused(const void* const* comp, const size_t* comp_bytes, size_t chunk_bytes, size_t num_chunks, int32_t lo, int32_t hi,
                long long* sums, int* status, hipStream_t stream)
{
  hipLaunchKernelGGL(fused_filter_sum, dim3(grid_for(num_chunks)), dim3(64 * kWaves), 0, stream, comp, comp_bytes, chunk_bytes,
                     num_chunks, lo, hi, sums, status);
  return (int)hipGetLastError();
}

int bench_reduce(const int32_t* values, size_t chunk_bytes, size_t num_chunks, int32_t lo, int32_t hi, long long* sums,
                 hipStream_t stream)
{
  hipLaunchKernelGGL(filter_sum_ints, dim3(grid_for(num_chunks)), dim3(64 * kWaves), 0, stream, values, chunk_bytes, num_chunks, lo,
                     hi, sums);
  return (int)hipGetLastError();
}

int bench_plain(const void* const* comp, const size_t* comp_bytes, uint8_t* out, size_t chunk_bytes, size_t num_chunks, int* status,
                hipStream_t stream)
{
  hipLaunchKernelGGL(plain_decompress, dim3(grid_for(num_chunks)), dim3(64 * kWaves), 0, stream, comp, comp_bytes, out, chunk_bytes,
                     num_chunks, status);
  return (int)hipGetLastError();
}

int bench_compress(const uint8_t* in, size_t chunk_bytes, size_t num_chunks, void* const* out, size_t* out_bytes,
                   nvcompBatchedCascadedOpts_t opts, hipStream_t stream)
{
  hipLaunchKernelGGL(plain_compress, dim3(grid_for(num_chunks)), dim3(64 * kWaves), 0, stream, in, chunk_bytes, num_chunks, out,
                     out_bytes, opts);
  return (int)hipGetLastError();
}

} // extern "C"
