/*
 * examples/bitcomp_native_example.cpp -- the native Bitcomp API (nvcomp/native/bitcomp.h): a lossy, error-bounded
 * round trip of a synthetic fp32 field (a smooth wave plus noise; 64 MiB, or argv[1] MiB), then a partial decompression of one
 * mebibyte out of its middle. Prints the sizes, the ratio and the largest absolute error against delta / 2.
 * Exit code 0 = the error bound holds and the partial range equals the full decode.
 */
#include <cmath>
#include <cstring>
#include <random>

#include "nvcomp/native/bitcomp.h"
#include "util.hpp"

#define BITCOMP_CHECK(expr)                                                                       \
  do {                                                                                            \
    const bitcompResult_t rc_ = (expr);                                                           \
    if (rc_ != BITCOMP_SUCCESS) {                                                                 \
      throw std::runtime_error(std::string(#expr) + " returned " + std::to_string((int)rc_));    \
    }                                                                                             \
  } while (0)

int main(int argc, char** argv)
{
  try {
    const size_t mib = argc > 1 ? (size_t)std::atoi(argv[1]) : 64; /* size of the field; at least 4 */
    const size_t count = (mib < 4 ? 4 : mib) << 18;
    const size_t n_bytes = count * sizeof(float);
    const float delta = 1e-3f;
    std::vector<float> field(count);
    std::mt19937 rng(42);
    std::normal_distribution<float> noise(0.0f, 0.02f);
    for (size_t i = 0; i < count; ++i) {
      field[i] = 300.0f + 25.0f * std::sin((float)i * 1e-4f) + noise(rng);
    }

    hipStream_t stream;
    HIP_CHECK(hipStreamCreate(&stream));
    float *d_in = nullptr, *d_out = nullptr, *d_part = nullptr;
    void* d_comp = nullptr;
    const size_t part_start = n_bytes / 2 + 4, part_bytes = (size_t)1 << 20;
    HIP_CHECK(hipMalloc((void**)&d_in, n_bytes));
    HIP_CHECK(hipMalloc((void**)&d_out, n_bytes));
    HIP_CHECK(hipMalloc((void**)&d_part, part_bytes));
    HIP_CHECK(hipMalloc(&d_comp, bitcompMaxBuflen(n_bytes)));
    HIP_CHECK(hipMemcpy(d_in, field.data(), n_bytes, hipMemcpyHostToDevice));

    bitcompHandle_t plan;
    BITCOMP_CHECK(bitcompCreatePlan(&plan, n_bytes, BITCOMP_FP32_DATA, BITCOMP_LOSSY_FP_TO_SIGNED, BITCOMP_DEFAULT_ALGO));
    BITCOMP_CHECK(bitcompSetStream(plan, stream));
    BITCOMP_CHECK(bitcompCompressLossy_fp32(plan, d_in, d_comp, delta));
    HIP_CHECK(hipStreamSynchronize(stream));
    size_t comp_bytes = 0;
    BITCOMP_CHECK(bitcompGetCompressedSize(d_comp, &comp_bytes));

    /* the reader knows nothing but the buffer */
    bitcompHandle_t reader;
    BITCOMP_CHECK(bitcompCreatePlanFromCompressedData(&reader, d_comp));
    BITCOMP_CHECK(bitcompSetStream(reader, stream));
    BITCOMP_CHECK(bitcompUncompress(reader, d_comp, d_out));
    BITCOMP_CHECK(bitcompPartialUncompress(reader, d_comp, d_part, part_start, part_bytes));
    HIP_CHECK(hipStreamSynchronize(stream));

    std::vector<float> back(count), part(part_bytes / sizeof(float));
    HIP_CHECK(hipMemcpy(back.data(), d_out, n_bytes, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(part.data(), d_part, part_bytes, hipMemcpyDeviceToHost));
    double worst = 0.0;
    for (size_t i = 0; i < count; ++i) {
      worst = std::max(worst, std::fabs((double)field[i] - (double)back[i]));
    }
    const bool part_ok = std::memcmp(part.data(), back.data() + part_start / sizeof(float), part_bytes) == 0;
    /* delta / 2 plus one rounding of q * delta at the field's magnitude (ulp of 512 in fp32 = 2^-14) */
    const double bound = (double)delta / 2 + 6.103515625e-05;
    std::printf("uncompressed (B): %zu\n", n_bytes);
    std::printf("compressed (B): %zu, ratio: %.3f\n", comp_bytes, (double)n_bytes / (double)comp_bytes);
    std::printf("max abs error: %.6g (delta / 2 = %.6g)\n", worst, (double)delta / 2);
    std::printf("partial range of %zu bytes at %zu: %s\n", part_bytes, part_start, part_ok ? "equal" : "DIFFERENT");

    BITCOMP_CHECK(bitcompDestroyPlan(reader));
    BITCOMP_CHECK(bitcompDestroyPlan(plan));
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipFree(d_part);
    (void)hipFree(d_comp);
    (void)hipStreamDestroy(stream);
    if (!(worst <= bound) || !part_ok || comp_bytes >= n_bytes) {
      std::printf("FAILED\n");
      return 1;
    }
    std::printf("lossy round trip within the error bound\n");
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
}
