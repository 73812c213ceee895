/*
 * scripts/bench_ans_device.hip -- kernels of scripts/bench_ans_device.py: an ANS decode fused into its consumer through
 * the device-side API (nvcomp/device/ans.hpp), and the consumer alone for the two-kernel path (batched decode to HBM,
 * then this kernel). The consumer is a 256-entry codebook lookup that writes fp16 values (as their bit patterns).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <nvcomp/device/ans.hpp>

namespace {

constexpr unsigned kWaves = 4;

typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(64 * kWaves) fused_decode_lookup(const void* const* comp, const size_t* comp_bytes,
                                                                   const size_t* caps, const uint16_t* codebook,
                                                                   uint16_t* out, size_t chunk_bytes, size_t num_chunks,
                                                                   int* status)
{
  __shared__ __attribute__((aligned(16))) uint8_t scratch[kWaves][nvcomp::device::ans::kDecompressSharedBytes];
  __shared__ uint16_t book[256];
  for (unsigned i = threadIdx.x; i < 256; i += blockDim.x) {
    book[i] = codebook[i];
  }
  __syncthreads();
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t chunk = (size_t)blockIdx.x * kWaves + w;
  if (chunk >= num_chunks) {
    return;
  }
  uint16_t* dst = out + chunk * chunk_bytes;
  const nvcompStatus_t st = nvcomp::device::ans::decompress_to(
      comp[chunk], comp_bytes[chunk], caps[chunk], nullptr, scratch[w], [&](uint32_t off, uint32_t word, uint32_t nb) {
        if (nb == 4) {
          const u16x4 v = {book[word & 255u], book[(word >> 8) & 255u], book[(word >> 16) & 255u], book[word >> 24]};
          *(u16x4*)(dst + off) = v;
        } else {
          for (uint32_t k = 0; k < nb; ++k) {
            dst[off + k] = book[(word >> (8 * k)) & 255u];
          }
        }
      });
  if (threadIdx.x % 64 == 0) {
    status[chunk] = (int)st;
  }
}

/* the consumer of the two-kernel path: 4 bytes a thread, grid-stride */
__global__ void __launch_bounds__(256) lookup(const uint32_t* codes, const uint16_t* codebook, uint16_t* out, size_t words)
{
  __shared__ uint16_t book[256];
  book[threadIdx.x] = codebook[threadIdx.x];
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) {
    const uint32_t word = codes[i];
    const u16x4 v = {book[word & 255u], book[(word >> 8) & 255u], book[(word >> 16) & 255u], book[word >> 24]};
    *(u16x4*)(out + 4 * i) = v;
  }
}

} // namespace

extern "C" {

int bench_fused(const void* const* comp, const size_t* comp_bytes, const size_t* caps, const uint16_t* codebook, uint16_t* out,
                size_t chunk_bytes, size_t num_chunks, int* status, hipStream_t stream)
{
  hipLaunchKernelGGL(fused_decode_lookup, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0,
                     stream, comp, comp_bytes, caps, codebook, out, chunk_bytes, num_chunks, status);
  return (int)hipGetLastError();
}

int bench_lookup(const void* codes, const uint16_t* codebook, uint16_t* out, size_t bytes, unsigned grid, hipStream_t stream)
{
  hipLaunchKernelGGL(lookup, dim3(grid), dim3(256), 0, stream, (const uint32_t*)codes, codebook, out, bytes / 4);
  return (int)hipGetLastError();
}

} // extern "C"
