/*
 * examples/ans_device_example.cpp -- the device-side ANS API (nvcomp/device/ans.hpp) in a caller's own kernel.
 *
 * 8 MiB of 8-bit codes (a quantised signal) are compressed in 64 KiB chunks with the batched API
 * (nvcompBatchedANSCompressAsync). A user kernel then decodes each chunk with nvcomp::device::ans::decompress_to and
 * consumes the bytes where they are decoded: a 256-entry codebook lookup that writes fp32 values. The decoded bytes
 * never go to memory. Exits non-zero on any mismatch with the host's lookup of the original codes.
 */
#include <cmath>
#include <random>

#include "nvcomp/ans.h"
#include "nvcomp/device/ans.hpp"
#include "util.hpp"

namespace {

constexpr unsigned kWaves = 4; /* waves per workgroup, one chunk each */

/* One wave per chunk: codes -> book[code], four values (16 bytes) per sink call. */
__global__ void __launch_bounds__(64 * kWaves) decode_lookup(const void* const* comp, const size_t* comp_bytes,
                                                             const size_t* n_bytes, const float* codebook, float* out,
                                                             size_t chunk_bytes, size_t num_chunks, int* errors)
{
  /* each wave needs its own kDecompressSharedBytes of LDS; the calls contain no workgroup barrier */
  __shared__ __attribute__((aligned(16))) uint8_t scratch[kWaves][nvcomp::device::ans::kDecompressSharedBytes];
  __shared__ float book[256];
  for (unsigned i = threadIdx.x; i < 256; i += blockDim.x) {
    book[i] = codebook[i];
  }
  __syncthreads(); /* the kernel's own barrier, before the waves part */
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t chunk = (size_t)blockIdx.x * kWaves + w;
  if (chunk >= num_chunks) {
    return; /* a whole wave leaves: the API needs all 64 lanes of a wave, not of a workgroup */
  }
  float* dst = out + chunk * chunk_bytes;
  size_t n = 0;
  const nvcompStatus_t st = nvcomp::device::ans::decompress_to(
      comp[chunk], comp_bytes[chunk], n_bytes[chunk], &n, scratch[w], [&](uint32_t off, uint32_t word, uint32_t nb) {
        if (nb == 4) {
          const float4 v = {book[word & 255u], book[(word >> 8) & 255u], book[(word >> 16) & 255u], book[word >> 24]};
          *(float4*)(dst + off) = v;
        } else {
          for (uint32_t k = 0; k < nb; ++k) {
            dst[off + k] = book[(word >> (8 * k)) & 255u];
          }
        }
      });
  if (threadIdx.x % 64 == 0 && (st != nvcompSuccess || n != n_bytes[chunk])) {
    atomicAdd(errors, 1);
  }
}

} // namespace

int main()
{
  try {
    const size_t total = (8u << 20) + 12345, chunk = 1 << 16;
    const size_t num_chunks = (total + chunk - 1) / chunk;
    std::vector<uint8_t> codes(total);
    std::mt19937 gen(7);
    std::normal_distribution<float> noise(0.f, 12.f);
    for (size_t i = 0; i < total; ++i) { /* a slow sine plus noise, quantised to 8 bits */
      const float v = 128.f + 90.f * std::sin(i * 1e-4f) + noise(gen);
      codes[i] = (uint8_t)std::fmin(255.f, std::fmax(0.f, v));
    }
    std::vector<float> book(256);
    for (int i = 0; i < 256; ++i) {
      book[i] = (i - 127.5f) / 64.f;
    }

    uint8_t* d_codes;
    HIP_CHECK(hipMalloc((void**)&d_codes, total));
    HIP_CHECK(hipMemcpy(d_codes, codes.data(), total, hipMemcpyHostToDevice));
    size_t max_out = 0;
    if (nvcompBatchedANSCompressGetMaxOutputChunkSize(chunk, nvcompBatchedANSDefaultOpts, &max_out) != nvcompSuccess) {
      throw std::runtime_error("GetMaxOutputChunkSize failed");
    }
    uint8_t* d_comp;
    HIP_CHECK(hipMalloc((void**)&d_comp, num_chunks * max_out));
    std::vector<void*> h_in(num_chunks), h_comp(num_chunks);
    std::vector<size_t> h_n(num_chunks);
    for (size_t i = 0; i < num_chunks; ++i) {
      h_in[i] = d_codes + i * chunk;
      h_comp[i] = d_comp + i * max_out;
      h_n[i] = std::min(chunk, total - i * chunk);
    }
    void **d_in, **d_comp_ptrs;
    size_t *d_n, *d_comp_bytes;
    HIP_CHECK(hipMalloc((void**)&d_in, num_chunks * sizeof(void*)));
    HIP_CHECK(hipMalloc((void**)&d_comp_ptrs, num_chunks * sizeof(void*)));
    HIP_CHECK(hipMalloc((void**)&d_n, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_comp_bytes, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMemcpy(d_in, h_in.data(), num_chunks * sizeof(void*), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_comp_ptrs, h_comp.data(), num_chunks * sizeof(void*), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_n, h_n.data(), num_chunks * sizeof(size_t), hipMemcpyHostToDevice));
    if (nvcompBatchedANSCompressAsync((const void* const*)d_in, d_n, chunk, num_chunks, nullptr, 0, d_comp_ptrs, d_comp_bytes,
                                      nvcompBatchedANSDefaultOpts, 0) != nvcompSuccess) {
      throw std::runtime_error("nvcompBatchedANSCompressAsync failed");
    }
    std::vector<size_t> h_comp_bytes(num_chunks);
    HIP_CHECK(hipMemcpy(h_comp_bytes.data(), d_comp_bytes, num_chunks * sizeof(size_t), hipMemcpyDeviceToHost));
    size_t comp_total = 0;
    for (size_t b : h_comp_bytes) {
      comp_total += b;
    }

    float *d_book, *d_out;
    int* d_errors;
    HIP_CHECK(hipMalloc((void**)&d_book, 256 * sizeof(float)));
    HIP_CHECK(hipMalloc((void**)&d_out, total * sizeof(float)));
    HIP_CHECK(hipMalloc((void**)&d_errors, sizeof(int)));
    HIP_CHECK(hipMemcpy(d_book, book.data(), 256 * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(d_out, 0xff, total * sizeof(float)));
    HIP_CHECK(hipMemset(d_errors, 0, sizeof(int)));
    hipLaunchKernelGGL(decode_lookup, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, 0,
                       (const void* const*)d_comp_ptrs, d_comp_bytes, d_n, d_book, d_out, chunk, num_chunks, d_errors);
    HIP_CHECK(hipGetLastError());
    int errors = 0;
    HIP_CHECK(hipMemcpy(&errors, d_errors, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<float> out(total);
    HIP_CHECK(hipMemcpy(out.data(), d_out, total * sizeof(float), hipMemcpyDeviceToHost));
    size_t bad = 0;
    for (size_t i = 0; i < total; ++i) {
      bad += out[i] != book[codes[i]];
    }
    printf("%zu chunks, %zu bytes of codes -> %zu compressed (ratio %.3f); %d chunks reported errors, %zu values differ\n",
           num_chunks, total, comp_total, (double)total / comp_total, errors, bad);
    for (void* p : {(void*)d_codes, (void*)d_comp, (void*)d_in, (void*)d_comp_ptrs, (void*)d_n, (void*)d_comp_bytes,
                    (void*)d_book, (void*)d_out, (void*)d_errors}) {
      HIP_CHECK(hipFree(p));
    }
    if (errors != 0 || bad != 0) {
      printf("FAILED\n");
      return 1;
    }
    printf("fused decode matches the host's codebook lookup\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
