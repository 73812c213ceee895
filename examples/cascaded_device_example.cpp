/*
 * examples/cascaded_device_example.cpp -- the device-side Cascaded API (nvcomp/device/cascaded.hpp) in a caller's own
 * kernel: a filter and a sum over a compressed int32 column, with no decoded buffer.
 *
 * A column of 4 Mi int32 values is compressed by the batched API (nvcompBatchedCascadedCompressAsync, 64 KiB chunks, the
 * default options). ONE kernel then decodes each chunk with decompress_to, one wave per chunk: the sink keeps the values
 * with lo <= v < hi and adds them up per lane; a wave reduction leaves one sum and one count per chunk. The decoded column
 * is never written to memory. The program checks the result three ways: against the batched decode of the same streams,
 * against the input column, and the statuses; it exits non-zero on any mismatch.
 */
#include <cstring>
#include <vector>

#include "nvcomp/cascaded.h"
#include "nvcomp/device/cascaded.hpp"
#include "util.hpp"

namespace {

namespace casc = nvcomp::device::cascaded;

#define NVCOMP_CHECK(expr)                                                                                  \
  do {                                                                                                      \
    const nvcompStatus_t st_ = (expr);                                                                      \
    if (st_ != nvcompSuccess) {                                                                             \
      throw std::runtime_error(std::string("nvcomp status ") + std::to_string((int)st_) + " from " + #expr); \
    }                                                                                                       \
  } while (0)

constexpr unsigned kWaves = 4;         /* waves per workgroup, one chunk each */
/* LDS per wave: decompress_shared_bytes() of the default options, with which no stream of theirs is refused for want of
 * LDS (main() checks). A column known to be smooth decodes in the 5 KiB of the batched decoder's first pass, at four
 * times the waves per CU. */
constexpr unsigned kSliceBytes = 14464;

__global__ void __launch_bounds__(64 * kWaves, 2) filter_sum(const void* const* comp, const size_t* comp_bytes, size_t chunk_bytes,
                                                             int32_t lo, int32_t hi, long long* sums, unsigned* counts, int* status,
                                                             size_t num_chunks)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kWaves][kSliceBytes];
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t chunk = (size_t)blockIdx.x * kWaves + w;
  if (chunk >= num_chunks) {
    return; /* a whole wave leaves: the API needs all 64 lanes of a wave, not of a workgroup */
  }
  long long sum = 0;
  unsigned kept = 0;
  /* the fused consumer: the sink sees every element once, on the lane that holds it */
  const nvcompStatus_t st = casc::decompress_to<int32_t>(comp[chunk], comp_bytes[chunk], chunk_bytes, nullptr, lds[w], kSliceBytes,
                                                         [&](uint32_t, int32_t v) {
                                                           if (v >= lo && v < hi) {
                                                             sum += v;
                                                             ++kept;
                                                           }
                                                         });
  for (int off = 32; off >= 1; off >>= 1) { /* the caller's own wave reduction, outside the sink */
    sum += __shfl_xor(sum, off);
    kept += __shfl_xor(kept, off);
  }
  if (threadIdx.x % 64 == 0) {
    sums[chunk] = sum;
    counts[chunk] = kept;
    status[chunk] = (int)st;
  }
}

} // namespace

int main()
{
  try {
    const size_t total = (4u << 20) + 1234, chunk_bytes = 65536, chunk_elems = chunk_bytes / 4;
    const size_t num_chunks = (total + chunk_elems - 1) / chunk_elems;
    const int32_t lo = 1000, hi = 250000;
    /* an analytics column: a slowly rising key with plateaus and a little jitter */
    std::vector<int32_t> column(total);
    uint32_t rng = 12345;
    int32_t level = 0;
    for (size_t i = 0; i < total; ++i) {
      rng = rng * 1664525u + 1013904223u;
      if ((rng >> 28) == 0) {
        level += (int32_t)((rng >> 8) & 63);
      }
      column[i] = level + (int32_t)((rng >> 16) & 3);
    }
    const nvcompBatchedCascadedOpts_t opts = nvcompBatchedCascadedDefaultOpts;
    if (casc::decompress_shared_bytes(opts) > kSliceBytes) {
      throw std::runtime_error("kSliceBytes is below the worst case of the options");
    }
    size_t max_out = 0, comp_temp = 0, dec_temp = 0;
    NVCOMP_CHECK(nvcompBatchedCascadedCompressGetMaxOutputChunkSize(chunk_bytes, opts, &max_out));
    NVCOMP_CHECK(nvcompBatchedCascadedCompressGetTempSize(num_chunks, chunk_bytes, opts, &comp_temp));
    NVCOMP_CHECK(nvcompBatchedCascadedDecompressGetTempSize(num_chunks, chunk_bytes, &dec_temp));
    max_out = (max_out + 7) & ~(size_t)7;

    int32_t *d_column, *d_decoded;
    uint8_t *d_comp, *d_temp;
    void **d_in_ptrs, **d_comp_ptrs, **d_out_ptrs;
    size_t *d_in_bytes, *d_comp_bytes, *d_actual;
    long long* d_sums;
    unsigned* d_counts;
    int* d_status;
    nvcompStatus_t* d_batched_status;
    HIP_CHECK(hipMalloc((void**)&d_column, total * 4));
    HIP_CHECK(hipMalloc((void**)&d_decoded, total * 4));
    HIP_CHECK(hipMalloc((void**)&d_comp, num_chunks * max_out));
    HIP_CHECK(hipMalloc((void**)&d_temp, (comp_temp > dec_temp ? comp_temp : dec_temp) + 8));
    HIP_CHECK(hipMalloc((void**)&d_in_ptrs, num_chunks * sizeof(void*)));
    HIP_CHECK(hipMalloc((void**)&d_comp_ptrs, num_chunks * sizeof(void*)));
    HIP_CHECK(hipMalloc((void**)&d_out_ptrs, num_chunks * sizeof(void*)));
    HIP_CHECK(hipMalloc((void**)&d_in_bytes, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_comp_bytes, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_actual, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_sums, num_chunks * sizeof(long long)));
    HIP_CHECK(hipMalloc((void**)&d_counts, num_chunks * sizeof(unsigned)));
    HIP_CHECK(hipMalloc((void**)&d_status, num_chunks * sizeof(int)));
    HIP_CHECK(hipMalloc((void**)&d_batched_status, num_chunks * sizeof(nvcompStatus_t)));
    std::vector<void*> in_ptrs(num_chunks), comp_ptrs(num_chunks), out_ptrs(num_chunks);
    std::vector<size_t> in_bytes(num_chunks);
    for (size_t c = 0; c < num_chunks; ++c) {
      in_ptrs[c] = d_column + c * chunk_elems;
      out_ptrs[c] = d_decoded + c * chunk_elems;
      comp_ptrs[c] = d_comp + c * max_out;
      in_bytes[c] = 4 * (total - c * chunk_elems < chunk_elems ? total - c * chunk_elems : chunk_elems);
    }
    HIP_CHECK(hipMemcpy(d_column, column.data(), total * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_in_ptrs, in_ptrs.data(), num_chunks * sizeof(void*), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_comp_ptrs, comp_ptrs.data(), num_chunks * sizeof(void*), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_out_ptrs, out_ptrs.data(), num_chunks * sizeof(void*), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_in_bytes, in_bytes.data(), num_chunks * sizeof(size_t), hipMemcpyHostToDevice));
    NVCOMP_CHECK(nvcompBatchedCascadedCompressAsync(d_in_ptrs, d_in_bytes, chunk_bytes, num_chunks, d_temp, comp_temp, d_comp_ptrs,
                                                    d_comp_bytes, opts, 0));

    /* the fused filter + sum: no decoded buffer */
    hipLaunchKernelGGL(filter_sum, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, 0, d_comp_ptrs,
                       d_comp_bytes, chunk_bytes, lo, hi, d_sums, d_counts, d_status, num_chunks);
    HIP_CHECK(hipGetLastError());
    /* the check: the batched decode of the same streams, filtered and summed on the host */
    NVCOMP_CHECK(nvcompBatchedCascadedDecompressAsync(d_comp_ptrs, d_comp_bytes, d_in_bytes, d_actual, num_chunks, d_temp, dec_temp,
                                                      d_out_ptrs, d_batched_status, 0));
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<long long> sums(num_chunks);
    std::vector<unsigned> counts(num_chunks);
    std::vector<int> status(num_chunks);
    std::vector<nvcompStatus_t> batched_status(num_chunks);
    std::vector<size_t> comp_bytes(num_chunks);
    std::vector<int32_t> decoded(total);
    HIP_CHECK(hipMemcpy(sums.data(), d_sums, num_chunks * sizeof(long long), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(counts.data(), d_counts, num_chunks * sizeof(unsigned), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(status.data(), d_status, num_chunks * sizeof(int), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(batched_status.data(), d_batched_status, num_chunks * sizeof(nvcompStatus_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(comp_bytes.data(), d_comp_bytes, num_chunks * sizeof(size_t), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(decoded.data(), d_decoded, total * 4, hipMemcpyDeviceToHost));
    size_t bad_status = 0, bad_chunks = 0, comp_total = 0;
    long long grand = 0, host_grand = 0;
    unsigned long long kept = 0;
    for (size_t c = 0; c < num_chunks; ++c) {
      bad_status += status[c] != (int)nvcompSuccess || batched_status[c] != nvcompSuccess;
      long long from_batched = 0, from_input = 0;
      unsigned n_batched = 0;
      for (size_t i = c * chunk_elems; i < c * chunk_elems + in_bytes[c] / 4; ++i) {
        if (decoded[i] >= lo && decoded[i] < hi) {
          from_batched += decoded[i];
          ++n_batched;
        }
        if (column[i] >= lo && column[i] < hi) {
          from_input += column[i];
        }
      }
      bad_chunks += sums[c] != from_batched || sums[c] != from_input || counts[c] != n_batched;
      grand += sums[c];
      host_grand += from_input;
      kept += counts[c];
      comp_total += comp_bytes[c];
    }
    const bool same_column = std::memcmp(decoded.data(), column.data(), total * 4) == 0;
    printf("%zu chunks, %zu bytes of int32 -> %zu compressed (ratio %.2f); %llu values in [%d, %d), sum %lld (host: %lld); "
           "%zu chunks with a status, %zu chunks differ, batched decode %s the input\n",
           num_chunks, total * 4, comp_total, (double)(total * 4) / comp_total, kept, lo, hi, grand, host_grand, bad_status, bad_chunks,
           same_column ? "equals" : "DIFFERS FROM");
    for (void* p : {(void*)d_column, (void*)d_decoded, (void*)d_comp, (void*)d_temp, (void*)d_in_ptrs, (void*)d_comp_ptrs, (void*)d_out_ptrs,
                    (void*)d_in_bytes, (void*)d_comp_bytes, (void*)d_actual, (void*)d_sums, (void*)d_counts, (void*)d_status,
                    (void*)d_batched_status}) {
      HIP_CHECK(hipFree(p));
    }
    if (bad_status != 0 || bad_chunks != 0 || !same_column || grand != host_grand || kept == 0) {
      printf("FAILED\n");
      return 1;
    }
    printf("OK\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
