/*
 * examples/lz4_device_compress_example.cpp -- the compressor of the device-side LZ4 API (nvcomp/device/lz4.hpp) in a
 * caller's own kernel: a chunk is transformed in LDS and compressed from there, only the LZ4 block goes to HBM.
 *
 * 16 MiB of 4-byte counters are cut into chunks of 64 KiB. ONE kernel, one wave per chunk,
 *   1. byte-transposes its chunk into four planes in LDS (plane b holds byte b of every element: the byte shuffle that
 *      columnar formats put in front of LZ4; the high bytes of neighbouring counters are equal and become runs);
 *   2. compresses the planes with compress(), reading them where they lie, into the chunk's slot in global memory.
 * 64 KiB + the wave's scratch area: two such workgroups per CU. The transposed chunk never exists in HBM.
 *
 * The host decodes every block twice -- with liblz4's LZ4_decompress_safe and with nvcompBatchedLZ4DecompressAsync --,
 * undoes the transpose and compares with the original; exits non-zero on any mismatch.
 */
#include <cstring>
#include <vector>

#include <lz4.h>

#include "nvcomp/device/lz4.hpp"
#include "nvcomp/lz4.h"
#include "util.hpp"

namespace {

namespace lz4dev = nvcomp::device::lz4;

constexpr size_t kChunk = 1 << 16;

__global__ void __launch_bounds__(64) shuffle_in_lds_and_compress(const uint8_t* data, const size_t* chunk_bytes, uint8_t* comp,
                                                                  size_t slot_bytes, size_t* comp_bytes)
{
  __shared__ __attribute__((aligned(16))) uint8_t planes[kChunk];
  __shared__ __attribute__((aligned(16))) uint8_t scratch[lz4dev::kCompressSharedBytes];
  const unsigned lane = threadIdx.x;
  const size_t c = blockIdx.x;
  const size_t n = chunk_bytes[c]; /* a multiple of 4 */
  const size_t elems = n / 4;
  const uint32_t* words = (const uint32_t*)(data + c * kChunk);
  for (size_t i = lane; i < elems; i += 64) {
    const uint32_t w = words[i];
    planes[i] = (uint8_t)w;
    planes[elems + i] = (uint8_t)(w >> 8);
    planes[2 * elems + i] = (uint8_t)(w >> 16);
    planes[3 * elems + i] = (uint8_t)(w >> 24);
  }
  lz4dev::wave_sync(); /* the compressor reads what other lanes wrote */
  const size_t size = lz4dev::compress(planes, n, comp + c * slot_bytes, scratch);
  if (lane == 0) {
    comp_bytes[c] = size;
  }
}

#define NVCOMP_OK(expr)                                                    \
  do {                                                                     \
    const nvcompStatus_t st_ = (expr);                                     \
    if (st_ != nvcompSuccess) {                                            \
      throw std::runtime_error(std::string(#expr) + " failed with " + std::to_string((int)st_)); \
    }                                                                      \
  } while (0)

/* planes -> elements; true where they are the original bytes */
bool unshuffled_equals(const uint8_t* planes, const uint8_t* want, size_t n)
{
  const size_t elems = n / 4;
  for (size_t i = 0; i < elems; ++i) {
    for (size_t b = 0; b < 4; ++b) {
      if (planes[b * elems + i] != want[4 * i + b]) {
        return false;
      }
    }
  }
  return true;
}

} // namespace

int main()
{
  try {
    const size_t total = (16u << 20) + 12344; /* the last chunk is a short one */
    const size_t num_chunks = (total + kChunk - 1) / kChunk;
    std::vector<uint8_t> data(total);
    uint32_t x = 12345, counter = 1000000;
    for (size_t i = 0; i < total / 4; ++i) { /* counters that grow by a small, noisy step */
      x = x * 1664525u + 1013904223u;
      counter += 1 + (x >> 29);
      std::memcpy(&data[4 * i], &counter, 4);
    }

    const size_t slot = lz4dev::max_compressed_bytes(kChunk);
    size_t api_bound = 0, temp_bytes = 0;
    NVCOMP_OK(nvcompBatchedLZ4CompressGetMaxOutputChunkSize(kChunk, nvcompBatchedLZ4DefaultOpts, &api_bound));
    if (api_bound != slot) {
      throw std::runtime_error("max_compressed_bytes differs from the batched API's bound");
    }
    NVCOMP_OK(nvcompBatchedLZ4DecompressGetTempSize(num_chunks, kChunk, &temp_bytes));
    std::vector<size_t> in_bytes(num_chunks);
    std::vector<const void*> comp_ptrs(num_chunks);
    std::vector<void*> out_ptrs(num_chunks);
    uint8_t *d_data, *d_comp, *d_out;
    void *d_temp, **d_comp_ptrs, **d_out_ptrs;
    size_t *d_in_bytes, *d_comp_bytes, *d_actual;
    nvcompStatus_t* d_status;
    HIP_CHECK(hipMalloc((void**)&d_data, num_chunks * kChunk));
    HIP_CHECK(hipMalloc((void**)&d_comp, num_chunks * slot));
    HIP_CHECK(hipMalloc((void**)&d_out, num_chunks * kChunk));
    HIP_CHECK(hipMalloc(&d_temp, temp_bytes ? temp_bytes : 1));
    HIP_CHECK(hipMalloc((void**)&d_comp_ptrs, num_chunks * sizeof(void*)));
    HIP_CHECK(hipMalloc((void**)&d_out_ptrs, num_chunks * sizeof(void*)));
    HIP_CHECK(hipMalloc((void**)&d_in_bytes, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_comp_bytes, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_actual, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_status, num_chunks * sizeof(nvcompStatus_t)));
    for (size_t c = 0; c < num_chunks; ++c) {
      in_bytes[c] = total - c * kChunk < kChunk ? total - c * kChunk : kChunk;
      comp_ptrs[c] = d_comp + c * slot;
      out_ptrs[c] = d_out + c * kChunk;
    }
    HIP_CHECK(hipMemcpy(d_data, data.data(), total, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_in_bytes, in_bytes.data(), num_chunks * sizeof(size_t), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_comp_ptrs, comp_ptrs.data(), num_chunks * sizeof(void*), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_out_ptrs, out_ptrs.data(), num_chunks * sizeof(void*), hipMemcpyHostToDevice));

    hipLaunchKernelGGL(shuffle_in_lds_and_compress, dim3((unsigned)num_chunks), dim3(64), 0, 0, d_data, d_in_bytes, d_comp, slot,
                       d_comp_bytes);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());

    /* the way back on the GPU: the batched decoder */
    NVCOMP_OK(nvcompBatchedLZ4DecompressAsync((const void* const*)d_comp_ptrs, d_comp_bytes, d_in_bytes, d_actual, num_chunks,
                                              d_temp, temp_bytes, (void* const*)d_out_ptrs, d_status, 0));
    HIP_CHECK(hipDeviceSynchronize());

    std::vector<size_t> comp_bytes(num_chunks), actual(num_chunks);
    std::vector<nvcompStatus_t> status(num_chunks);
    std::vector<uint8_t> comp(num_chunks * slot), out(num_chunks * kChunk), planes(kChunk);
    HIP_CHECK(hipMemcpy(comp_bytes.data(), d_comp_bytes, num_chunks * sizeof(size_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(actual.data(), d_actual, num_chunks * sizeof(size_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(status.data(), d_status, num_chunks * sizeof(nvcompStatus_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(comp.data(), d_comp, comp.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(out.data(), d_out, out.size(), hipMemcpyDeviceToHost));
    size_t comp_total = 0, bad_size = 0, bad_cpu = 0, bad_gpu = 0;
    for (size_t c = 0; c < num_chunks; ++c) {
      const size_t n = in_bytes[c];
      comp_total += comp_bytes[c];
      if (comp_bytes[c] == 0 || comp_bytes[c] > lz4dev::max_compressed_bytes(n)) {
        ++bad_size;
        continue;
      }
      /* the way back on the CPU: liblz4 */
      const int got = LZ4_decompress_safe((const char*)&comp[c * slot], (char*)planes.data(), (int)comp_bytes[c], (int)n);
      bad_cpu += got != (int)n || !unshuffled_equals(planes.data(), &data[c * kChunk], n);
      bad_gpu += status[c] != nvcompSuccess || actual[c] != n || !unshuffled_equals(&out[c * kChunk], &data[c * kChunk], n);
    }
    printf("%zu chunks, %zu bytes -> %zu compressed (ratio %.3f); %zu sizes out of range, %zu blocks liblz4 decodes to other "
           "bytes, %zu the batched decoder\n",
           num_chunks, total, comp_total, (double)total / comp_total, bad_size, bad_cpu, bad_gpu);
    for (void* p : {(void*)d_data, (void*)d_comp, (void*)d_out, d_temp, (void*)d_comp_ptrs, (void*)d_out_ptrs, (void*)d_in_bytes,
                    (void*)d_comp_bytes, (void*)d_actual, (void*)d_status}) {
      HIP_CHECK(hipFree(p));
    }
    if (bad_size != 0 || bad_cpu != 0 || bad_gpu != 0) {
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
