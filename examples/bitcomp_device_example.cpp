/*
 * examples/bitcomp_device_example.cpp -- the device-side Bitcomp API (nvcomp/device/bitcomp.hpp) in a caller's own
 * kernel, both ways, with the elements in registers.
 *
 * 4 Mi fp32 samples of a smooth signal are handled in chunks of 16 Ki values, one wave per chunk. ONE kernel
 *   1. quantises its chunk to int32 (q = rint(x / delta)) inside the source of compress_from: the integers are never in
 *      memory, only the compressed stream is written;
 *   2. decodes that stream with decompress_to, whose sink dequantises and accumulates: y[i] += a * (q * delta).
 * No LDS is used: the API needs none. The host repeats the arithmetic with plain loops and compares bit for bit; exits
 * non-zero on any mismatch.
 */
#include <cmath>
#include <cstring>
#include <vector>

#include "nvcomp/device/bitcomp.hpp"
#include "util.hpp"

namespace {

namespace bc = nvcomp::device::bitcomp;

constexpr unsigned kWaves = 4; /* waves per workgroup, one chunk each */

/* y + (a * t), the product and the sum each rounded once: what the host's check computes (hipcc would otherwise fuse) */
__device__ inline float add_product(float y, float a, float t)
{
#pragma clang fp contract(off)
  const float p = a * t;
  return y + p;
}

__global__ void __launch_bounds__(64 * kWaves, 8) quantise_compress_decode_accumulate(
    const float* x, float* y, size_t total, size_t chunk_elems, uint8_t* comp, size_t slot_bytes, size_t* comp_bytes,
    float delta, float a, size_t num_chunks, int* errors)
{
  const unsigned w = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const size_t chunk = (size_t)blockIdx.x * kWaves + w;
  if (chunk >= num_chunks) {
    return; /* a whole wave leaves: the API needs all 64 lanes of a wave, not of a workgroup */
  }
  const size_t first = chunk * chunk_elems;
  const size_t n = total - first < chunk_elems ? total - first : chunk_elems;
  const float* xs = x + first;
  float* ys = y + first;
  uint8_t* stream = comp + chunk * slot_bytes;
  /* the fused producer: the source is asked once per element, by the lane that owns it */
  const size_t c = bc::compress_from<int32_t>(n, stream, 0, [&](uint32_t i) { return bc::quantize(xs[i], delta); });
  bc::wave_sync(); /* this wave wrote the stream lane by lane and now reads it */
  /* the fused consumer: y[i] + (a * (q * delta)), each step rounded once */
  size_t got = 0;
  const nvcompStatus_t st = bc::decompress_to<int32_t>(stream, c, n * sizeof(int32_t), &got, nullptr, [&](uint32_t i, int32_t q) {
    ys[i] = add_product(ys[i], a, bc::dequantize(q, delta));
  });
  if (threadIdx.x % 64 == 0) {
    comp_bytes[chunk] = c;
    if (c == 0 || st != nvcompSuccess || got != n * sizeof(int32_t)) {
      atomicAdd(errors, 1);
    }
  }
}

} // namespace

int main()
{
  try {
    const size_t total = (4u << 20) + 321, chunk_elems = 1 << 14;
    const size_t num_chunks = (total + chunk_elems - 1) / chunk_elems;
    const float delta = 1e-3f, a = 0.37f;
    std::vector<float> x(total), y0(total);
    for (size_t i = 0; i < total; ++i) {
      x[i] = 3.f * std::sin(i * 2e-4f) + 0.25f * std::sin(i * 3.1e-2f);
      y0[i] = 1.f + 1e-6f * (float)(i % 1000);
    }
    const size_t slot = bc::max_compressed_bytes(chunk_elems * sizeof(int32_t), NVCOMP_TYPE_INT);

    float *d_x, *d_y;
    uint8_t* d_comp;
    size_t* d_comp_bytes;
    int* d_errors;
    HIP_CHECK(hipMalloc((void**)&d_x, total * sizeof(float)));
    HIP_CHECK(hipMalloc((void**)&d_y, total * sizeof(float)));
    HIP_CHECK(hipMalloc((void**)&d_comp, num_chunks * slot));
    HIP_CHECK(hipMalloc((void**)&d_comp_bytes, num_chunks * sizeof(size_t)));
    HIP_CHECK(hipMalloc((void**)&d_errors, sizeof(int)));
    HIP_CHECK(hipMemcpy(d_x, x.data(), total * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(d_y, y0.data(), total * sizeof(float), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(d_errors, 0, sizeof(int)));
    hipLaunchKernelGGL(quantise_compress_decode_accumulate, dim3((unsigned)((num_chunks + kWaves - 1) / kWaves)),
                       dim3(64 * kWaves), 0, 0, d_x, d_y, total, chunk_elems, d_comp, slot, d_comp_bytes, delta, a, num_chunks,
                       d_errors);
    HIP_CHECK(hipGetLastError());
    int errors = 0;
    HIP_CHECK(hipMemcpy(&errors, d_errors, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<float> y(total);
    std::vector<size_t> comp_bytes(num_chunks);
    HIP_CHECK(hipMemcpy(y.data(), d_y, total * sizeof(float), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(comp_bytes.data(), d_comp_bytes, num_chunks * sizeof(size_t), hipMemcpyDeviceToHost));
    size_t comp_total = 0;
    for (size_t b : comp_bytes) {
      comp_total += b;
    }
    size_t bad = 0;
    for (size_t i = 0; i < total; ++i) {
      const volatile float quotient = x[i] / delta; /* (volatile: every step rounded to fp32, nothing fused) */
      const volatile float back = (float)(int32_t)std::nearbyint(quotient) * delta;
      const volatile float scaled = a * back;
      const float want = y0[i] + scaled;
      bad += std::memcmp(&want, &y[i], sizeof(float)) != 0;
    }
    printf("%zu chunks, %zu bytes of fp32 -> %zu compressed at delta %g (ratio %.3f); %d chunks reported errors, %zu values differ\n",
           num_chunks, total * sizeof(float), comp_total, (double)delta, (double)(total * sizeof(float)) / comp_total, errors, bad);
    for (void* p : {(void*)d_x, (void*)d_y, (void*)d_comp, (void*)d_comp_bytes, (void*)d_errors}) {
      HIP_CHECK(hipFree(p));
    }
    if (errors != 0 || bad != 0) {
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
