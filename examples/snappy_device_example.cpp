/*
 * examples/snappy_device_example.cpp -- the device-side Snappy API (nvcomp/device/snappy.hpp) in a caller's own kernels:
 * a page is decoded into LDS and consumed there, and a page produced in LDS is compressed where it lies.
 *
 * 16 MiB of synthetic records are compressed in pages of 64 KiB with nvcompBatchedSnappyCompressAsync. Then
 *   1. ONE kernel, one wave per page, decodes its page with decompress() into a 64 KiB buffer in LDS (every copy is
 *      resolved in LDS) and counts the page's bytes into a 256-bin histogram, reading the buffer where it lies. Only the
 *      1 KiB histogram leaves the CU. The host counts the same histograms from the original bytes and compares.
 *   2. ONE kernel, one wave per page, stages its page in LDS, upper-cases its letters there (the "producer"), and
 *      compresses the result with compress() out of LDS: only the Snappy stream goes to HBM. The streams are decoded
 *      with nvcompBatchedSnappyDecompressAsync and compared with the upper-cased pages.
 * Exits non-zero on any mismatch.
 */
#include <cstring>
#include <vector>

#include "nvcomp/device/snappy.hpp"
#include "nvcomp/snappy.h"
#include "util.hpp"

namespace {

namespace snpdev = nvcomp::device::snappy;

constexpr size_t kChunk = 1 << 16;

__device__ __host__ inline uint8_t upper(uint8_t b)
{
  return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b;
}

__global__ void __launch_bounds__(64) decode_into_lds_and_count(const void* const* comp, const size_t* comp_bytes,
                                                                const size_t* chunk_bytes, uint32_t* histograms, int* errors)
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
  snpdev::wave_sync(); /* the lanes now read what other lanes decoded (and the zeroed bins) */
  if (st != nvcompSuccess || n != chunk_bytes[c]) {
    if (lane == 0) {
      atomicAdd(errors, 1);
    }
    return;
  }
  const uint32_t* words = (const uint32_t*)chunk;
  for (size_t i = lane; i < n / 4; i += 64) {
    const uint32_t w = words[i];
    atomicAdd(&bins[w & 255u], 1u);
    atomicAdd(&bins[(w >> 8) & 255u], 1u);
    atomicAdd(&bins[(w >> 16) & 255u], 1u);
    atomicAdd(&bins[w >> 24], 1u);
  }
  for (size_t i = (n & ~(size_t)3) + lane; i < n; i += 64) {
    atomicAdd(&bins[chunk[i]], 1u);
  }
  snpdev::wave_sync();
  for (unsigned i = lane; i < 256; i += 64) {
    histograms[c * 256 + i] = bins[i];
  }
}

__global__ void __launch_bounds__(64) produce_in_lds_and_compress(const void* const* raw, const size_t* raw_bytes,
                                                                  void* const* comp, size_t* comp_bytes)
{
  __shared__ __attribute__((aligned(16))) uint8_t chunk[kChunk];
  __shared__ __attribute__((aligned(16))) uint8_t scratch[snpdev::kCompressSharedBytes];
  const unsigned lane = threadIdx.x;
  const size_t c = blockIdx.x;
  const size_t n = raw_bytes[c];
  const uint8_t* src = (const uint8_t*)raw[c];
  for (size_t i = lane; i < n; i += 64) {
    chunk[i] = upper(src[i]);
  }
  snpdev::wave_sync(); /* the chunk was written lane by lane */
  const size_t got = snpdev::compress(chunk, n, comp[c], scratch);
  if (lane == 0) {
    comp_bytes[c] = got;
  }
}

#define NVCOMP_OK(expr)                                                    \
  do {                                                                     \
    const nvcompStatus_t st_ = (expr);                                     \
    if (st_ != nvcompSuccess) {                                            \
      throw std::runtime_error(std::string(#expr) + " failed with " + std::to_string((int)st_)); \
    }                                                                      \
  } while (0)

} // namespace

int main()
{
  try {
    const size_t total = (16u << 20) + 12345; /* the last page is a short one */
    const size_t num_chunks = (total + kChunk - 1) / kChunk;
    std::vector<uint8_t> data(total);
    uint32_t x = 12345;
    for (size_t i = 0; i < total; ++i) { /* records of a few repeating fields and a noisy one */
      x = x * 1664525u + 1013904223u;
      const size_t col = i % 48;
      data[i] = col < 20 ? (uint8_t)("2024-01-01,station-"[col]) : col < 40 ? (uint8_t)('0' + (i / 48 + col) % 7) : (uint8_t)(x >> 24);
    }

    std::vector<const void*> in_ptrs(num_chunks);
    std::vector<void*> comp_ptrs(num_chunks), back_ptrs(num_chunks);
    std::vector<size_t> in_bytes(num_chunks);
    size_t max_out = 0, temp_bytes = 0, dec_temp_bytes = 0;
    NVCOMP_OK(nvcompBatchedSnappyCompressGetMaxOutputChunkSize(kChunk, nvcompBatchedSnappyDefaultOpts, &max_out));
    NVCOMP_OK(nvcompBatchedSnappyCompressGetTempSize(num_chunks, kChunk, nvcompBatchedSnappyDefaultOpts, &temp_bytes));
    NVCOMP_OK(nvcompBatchedSnappyDecompressGetTempSize(num_chunks, kChunk, &dec_temp_bytes));
    if (max_out != snpdev::max_compressed_bytes(kChunk)) {
      throw std::runtime_error("max_compressed_bytes disagrees with the batched bound");
    }
    uint8_t *d_data, *d_comp, *d_back;
    void *d_temp, *d_dec_temp, **d_in_ptrs, **d_comp_ptrs, **d_back_ptrs;
    size_t *d_in_bytes, *d_comp_bytes, *d_actual;
    nvcompStatus_t* d_status;
    uint32_t* d_hist;
    int* d_errors;
    HIP_CHECK(hipMalloc((void**)&d_data, total));
    HIP_CHECK(hipMalloc((void**)&d_back, total));
    HIP_CHECK(hipMalloc((void**)&d_comp, num_chunks * max_out));
    HIP_CHECK(hipMalloc(&d_temp, temp_bytes ? temp_bytes : 1));
    HIP_CHECK(hipMalloc(&d_dec_temp, dec_temp_bytes ? dec_temp_bytes : 1));
    HIP_CHECK(hipMalloc((void**)&d_in_ptrs, num_chunks * sizeof(void*)));
    HIP_CHECK(hipMalloc((void**)&d_comp_ptrs, num_chunks * sizeof(void*)));
    HIP_CHECK(hipMalloc((void**)&d_back_ptrs, num_chunks * sizeof(void*)));
    HIP_CHECK(hipMalloc((void**)&d_in_bytes, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_comp_bytes, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_actual, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_status, num_chunks * sizeof(nvcompStatus_t)));
    HIP_CHECK(hipMalloc((void**)&d_hist, num_chunks * 256 * sizeof(uint32_t)));
    HIP_CHECK(hipMalloc((void**)&d_errors, sizeof(int)));
    for (size_t c = 0; c < num_chunks; ++c) {
      in_ptrs[c] = d_data + c * kChunk;
      back_ptrs[c] = d_back + c * kChunk;
      comp_ptrs[c] = d_comp + c * max_out;
      in_bytes[c] = total - c * kChunk < kChunk ? total - c * kChunk : kChunk;
    }
    HIP_CHECK(hipMemcpy(d_data, data.data(), total, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_in_ptrs, in_ptrs.data(), num_chunks * sizeof(void*), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_comp_ptrs, comp_ptrs.data(), num_chunks * sizeof(void*), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_back_ptrs, back_ptrs.data(), num_chunks * sizeof(void*), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_in_bytes, in_bytes.data(), num_chunks * sizeof(size_t), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(d_errors, 0, sizeof(int)));
    HIP_CHECK(hipMemset(d_hist, 0xff, num_chunks * 256 * sizeof(uint32_t)));

    /* 1. batched compressor -> decode into LDS, fused with the histogram */
    NVCOMP_OK(nvcompBatchedSnappyCompressAsync((const void* const*)d_in_ptrs, d_in_bytes, kChunk, num_chunks, d_temp, temp_bytes,
                                               (void* const*)d_comp_ptrs, d_comp_bytes, nvcompBatchedSnappyDefaultOpts, 0));
    hipLaunchKernelGGL(decode_into_lds_and_count, dim3((unsigned)num_chunks), dim3(64), 0, 0, (const void* const*)d_comp_ptrs,
                       d_comp_bytes, d_in_bytes, d_hist, d_errors);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());

    int errors = 0;
    std::vector<uint32_t> hist(num_chunks * 256);
    std::vector<size_t> comp_bytes(num_chunks);
    HIP_CHECK(hipMemcpy(&errors, d_errors, sizeof(int), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hist.data(), d_hist, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(comp_bytes.data(), d_comp_bytes, num_chunks * sizeof(size_t), hipMemcpyDeviceToHost));
    size_t comp_total = 0, bad = 0;
    for (size_t c = 0; c < num_chunks; ++c) {
      comp_total += comp_bytes[c];
      uint32_t want[256] = {0};
      for (size_t i = 0; i < in_bytes[c]; ++i) {
        ++want[data[c * kChunk + i]];
      }
      bad += std::memcmp(want, &hist[c * 256], sizeof(want)) != 0;
    }
    printf("decode into LDS: %zu pages, %zu bytes <- %zu compressed (ratio %.3f); %d pages reported errors, %zu histograms differ\n",
           num_chunks, total, comp_total, (double)total / comp_total, errors, bad);

    /* 2. produce in LDS, compress from LDS -> batched decoder */
    HIP_CHECK(hipMemset(d_comp, 0, num_chunks * max_out));
    hipLaunchKernelGGL(produce_in_lds_and_compress, dim3((unsigned)num_chunks), dim3(64), 0, 0, (const void* const*)d_in_ptrs,
                       d_in_bytes, (void* const*)d_comp_ptrs, d_comp_bytes);
    HIP_CHECK(hipGetLastError());
    NVCOMP_OK(nvcompBatchedSnappyDecompressAsync((const void* const*)d_comp_ptrs, d_comp_bytes, d_in_bytes, d_actual, num_chunks,
                                                 d_dec_temp, dec_temp_bytes, (void* const*)d_back_ptrs, d_status, 0));
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<uint8_t> back(total);
    std::vector<size_t> actual(num_chunks);
    std::vector<nvcompStatus_t> status(num_chunks);
    HIP_CHECK(hipMemcpy(back.data(), d_back, total, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(actual.data(), d_actual, num_chunks * sizeof(size_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(status.data(), d_status, num_chunks * sizeof(nvcompStatus_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(comp_bytes.data(), d_comp_bytes, num_chunks * sizeof(size_t), hipMemcpyDeviceToHost));
    size_t dev_total = 0, refused = 0, differ = 0;
    for (size_t c = 0; c < num_chunks; ++c) {
      dev_total += comp_bytes[c];
      refused += status[c] != nvcompSuccess || actual[c] != in_bytes[c] || comp_bytes[c] == 0 || comp_bytes[c] > max_out;
    }
    for (size_t i = 0; i < total; ++i) {
      differ += back[i] != upper(data[i]);
    }
    printf("compress from LDS: %zu bytes -> %zu compressed (ratio %.3f); %zu streams refused, %zu bytes differ\n", total, dev_total,
           (double)total / dev_total, refused, differ);

    for (void* p : {(void*)d_data, (void*)d_back, (void*)d_comp, d_temp, d_dec_temp, (void*)d_in_ptrs, (void*)d_comp_ptrs,
                    (void*)d_back_ptrs, (void*)d_in_bytes, (void*)d_comp_bytes, (void*)d_actual, (void*)d_status, (void*)d_hist,
                    (void*)d_errors}) {
      HIP_CHECK(hipFree(p));
    }
    if (errors != 0 || bad != 0 || refused != 0 || differ != 0) {
      printf("FAILED\n");
      return 1;
    }
    printf("PASSED\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
