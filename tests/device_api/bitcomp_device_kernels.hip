/*
 * tests/device_api/bitcomp_device_kernels.hip -- TEST ONLY: kernels that call the device-side Bitcomp API
 * (include/nvcomp/device/bitcomp.hpp), behind extern "C" launchers that tests/test_bitcomp_device.py drives through
 * ctypes. One source for both tiers: the MI355X (hipcc --offload-arch=gfx950 -shared -fPIC -I include) and the host
 * emulation (g++ -x c++ -Itests/emu -Iinclude ... -lnvcomp_emu).
 *
 * Launch shapes: 64, 256 or 1 024 threads; with fewer waves than chunks a wave loops over several chunks. Apart from the
 * two k_lds_* kernels, which stage chunks themselves, no kernel here declares LDS and all are launched with a dynamic
 * LDS size of 0: the API needs none.
 *
 * The file instantiates the codec some eighty times (every width and algorithm, through memory, sources and sinks), which
 * takes the device compiler minutes in one piece. -DBCDEV_PART=0 ... 7 compiles one slice each; the test builds the
 * slices side by side and links them. Without the macro everything is compiled at once.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <nvcomp/device/bitcomp.hpp>

namespace dev = nvcomp::device::bitcomp;

#ifdef BCDEV_PART
#define BCDEV_HAS(part) (BCDEV_PART == (part))
#else
#define BCDEV_HAS(part) 1
#endif

/* launchers of the other slices, called by the dispatching ones */
extern "C" {
int bcdev_compress_from_narrow(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                               int algo, unsigned elem, unsigned block, unsigned grid, uint32_t* const* counts,
                               uint32_t* flags, hipStream_t stream);
int bcdev_compress_from_wide(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                             int algo, unsigned elem, unsigned block, unsigned grid, uint32_t* const* counts, uint32_t* flags,
                             hipStream_t stream);
int bcdev_decompress_to_narrow(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps,
                               size_t* actual, int* status, size_t count, unsigned mode, unsigned elem, unsigned block,
                               unsigned grid, uint8_t* tails, uint32_t* flags, hipStream_t stream);
int bcdev_decompress_to_wide(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps,
                             size_t* actual, int* status, size_t count, unsigned mode, unsigned elem, unsigned block,
                             unsigned grid, uint8_t* tails, uint32_t* flags, hipStream_t stream);
}

#if defined(__HIP_DEVICE_COMPILE__)
#define WAVE_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define WAVE_UNIFORM(x) (x)
#endif

namespace {

constexpr size_t kLdsChunk = 6144; /* the largest chunk the LDS kernels stage */

enum : uint32_t { kSinkOutOfRange = 1, kSourceOutOfRange = 2, kBadValue = 4 };

/* y + (a * t): the product and the sum each rounded once, never contracted into a fused multiply-add */
__device__ inline float add_product(float y, float a, float t)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float p = a * t;
  return y + p;
}

template <class U>
__device__ inline U load_as(const void* p, size_t i)
{
  U v;
  __builtin_memcpy(&v, (const uint8_t*)p + i * sizeof(U), sizeof(U));
  return v;
}

template <class U>
__device__ inline void store_as(void* p, size_t i, U v)
{
  __builtin_memcpy((uint8_t*)p + i * sizeof(U), &v, sizeof(U));
}

#if BCDEV_HAS(0)
/* compress() of every chunk, type and algorithm picked at run time */
__global__ void __launch_bounds__(1024) k_compress(const void* const* in, const size_t* in_bytes, void* const* out,
                                                   size_t* out_bytes, size_t count, int type, int algo)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    const size_t r = dev::compress(in[c], in_bytes[c], out[c], (nvcompType_t)type, algo);
    if (lane == 0) {
      out_bytes[c] = r;
    }
  }
}

#endif

#if BCDEV_HAS(1) || BCDEV_HAS(2)
/* compress_from<U>() over the elements of in[0, n) through a memory source, which counts its calls in counts[c][i]
 * where `counts` is given and flags a call for an element that does not exist */
template <class U>
__global__ void __launch_bounds__(1024) k_compress_from(const void* const* in, const size_t* in_bytes, void* const* out,
                                                        size_t* out_bytes, size_t count, int algo, uint32_t* const* counts,
                                                        uint32_t* flags)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    const void* src = in[c];
    const size_t n_elems = in_bytes[c] / sizeof(U);
    uint32_t* cnt = counts != nullptr ? counts[c] : nullptr;
    const size_t r = dev::compress_from<U>(n_elems, out[c], algo, [&](uint32_t i) {
      if (i >= n_elems) {
        atomicOr(flags, (uint32_t)kSourceOutOfRange);
        return (U)0;
      }
      if (cnt != nullptr) {
        atomicAdd(&cnt[i], 1u);
      }
      return load_as<U>(src, i);
    });
    if (lane == 0) {
      out_bytes[c] = r;
    }
  }
}

#endif

#if BCDEV_HAS(3)
/* decompress() of every chunk into out */
__global__ void __launch_bounds__(1024) k_decompress(const void* const* in, const size_t* in_bytes, void* const* out,
                                                     const size_t* caps, size_t* actual, int* status, size_t count)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    size_t got = 0xDEADBEEF;
    const nvcompStatus_t st = dev::decompress(in[c], in_bytes[c], out[c], caps[c], &got);
    if (lane == 0) {
      actual[c] = got;
      status[c] = (int)st;
    }
  }
}

#endif

#if BCDEV_HAS(4) || BCDEV_HAS(5)
/* decompress_to<U>(): mode 1 stores the elements into out (and the tail bytes behind them), mode 2 counts every call in
 * out (one uint32 per element of the capacity) and sends the tail to tails[16 c], mode 3 stores and drops the tail
 * (tail_out null). A call for an element beyond the capacity is flagged, not carried out. */
template <class U>
__global__ void __launch_bounds__(1024) k_decompress_to(const void* const* in, const size_t* in_bytes, void* const* out,
                                                        const size_t* caps, size_t* actual, int* status, size_t count,
                                                        uint32_t mode, uint8_t* tails, uint32_t* flags)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    uint8_t* o = (uint8_t*)out[c];
    const size_t cap = caps[c];
    const size_t cap_elems = cap / sizeof(U);
    const size_t n = dev::decompressed_size(in[c], in_bytes[c]);
    uint8_t* tail_out = nullptr;
    if (mode == 1 && n <= cap) {
      tail_out = o + n / sizeof(U) * sizeof(U);
    } else if (mode == 2) {
      tail_out = tails + 16 * c;
    }
    const bool counting = mode == 2;
    size_t got = 0xDEADBEEF;
    const nvcompStatus_t st = dev::decompress_to<U>(in[c], in_bytes[c], cap, &got, tail_out, [&](uint32_t i, U v) {
      if (i >= cap_elems) {
        atomicOr(flags, (uint32_t)kSinkOutOfRange);
      } else if (counting) {
        atomicAdd((uint32_t*)o + i, 1u);
      } else {
        store_as<U>(o, i, v);
      }
    });
    if (lane == 0) {
      actual[c] = got;
      status[c] = (int)st;
    }
  }
}

#endif

#if BCDEV_HAS(6)
/* A mixed workgroup, no barrier anywhere: of every pair of waves the even one decompresses item j (decompress() into
 * dec_out, uint32 elements through a storing sink) while the odd one compresses item j (compress_from over raw); the workgroup's last wave only spins
 * on arithmetic: a xorshift chain of `iters` steps per lane into side[]. */
__global__ void __launch_bounds__(1024) k_mixed(const void* const* comp_in, const size_t* comp_in_bytes, void* const* dec_out,
                                                const size_t* caps, size_t* actual, int* status, const void* const* raw,
                                                const size_t* raw_bytes, void* const* comp_out, size_t* comp_out_bytes,
                                                size_t count, int algo, uint32_t* side, uint32_t iters)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  if (w == waves - 1) {
    const size_t t = (size_t)blockIdx.x * 64 + lane;
    uint32_t x = (uint32_t)t + 1;
    for (uint32_t i = 0; i < iters; ++i) {
      x ^= x << 13;
      x ^= x >> 17;
      x ^= x << 5;
    }
    side[t] = x;
    return;
  }
  const size_t pairs = (waves - 1) / 2;
  const size_t j = (size_t)blockIdx.x * pairs + (w >> 1);
  if ((w >> 1) >= pairs || j >= count) {
    return;
  }
  if (w & 1) {
    const uint32_t* vals = (const uint32_t*)raw[j];
    const size_t r = dev::compress_from<uint32_t>(raw_bytes[j] / 4, comp_out[j], algo, [&](uint32_t i) { return vals[i]; });
    if (lane == 0) {
      comp_out_bytes[j] = r;
    }
  } else {
    size_t got = 0xDEADBEEF;
    uint32_t* o = (uint32_t*)dec_out[j];
    const size_t cap_elems = caps[j] / 4;
    const nvcompStatus_t st = dev::decompress_to<uint32_t>(comp_in[j], comp_in_bytes[j], caps[j], &got, nullptr, [&](uint32_t i, uint32_t v) {
      if (i < cap_elems) {
        o[i] = v;
      }
    });
    if (lane == 0) {
      actual[j] = got;
      status[j] = (int)st;
    }
  }
}

#endif

#if BCDEV_HAS(7)
/* Four waves, one chunk (at most kLdsChunk bytes) each: the chunk is staged at byte `misalign` of an LDS buffer,
 * wave_sync(), compressed from there into global memory. */
__global__ void __launch_bounds__(256) k_lds_compress(const void* const* in, const size_t* in_bytes, void* const* out,
                                                      size_t* out_bytes, size_t count, int type, int algo, uint32_t misalign)
{
  __shared__ __attribute__((aligned(16))) uint8_t raw[4][kLdsChunk + 16];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const size_t c = (size_t)blockIdx.x * 4 + w;
  if (c >= count) {
    return;
  }
  const size_t n = in_bytes[c] < kLdsChunk ? in_bytes[c] : kLdsChunk;
  uint8_t* r = raw[w] + misalign;
  const uint8_t* src = (const uint8_t*)in[c];
  for (size_t i = lane; i < n; i += 64) {
    r[i] = src[i];
  }
  dev::wave_sync();
  const size_t zn = dev::compress(r, n, out[c], (nvcompType_t)type, algo);
  if (lane == 0) {
    out_bytes[c] = zn;
  }
}

#endif

#if BCDEV_HAS(6)
/* The other way: decompressed from global memory into LDS (at byte `misalign`), wave_sync(), copied out. */
__global__ void __launch_bounds__(256) k_lds_decompress(const void* const* in, const size_t* in_bytes, void* const* out,
                                                        size_t* actual, int* status, size_t count, uint32_t misalign)
{
  __shared__ __attribute__((aligned(16))) uint8_t raw[4][kLdsChunk + 16];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const size_t c = (size_t)blockIdx.x * 4 + w;
  if (c >= count) {
    return;
  }
  uint8_t* r = raw[w] + misalign;
  size_t got = 0xDEADBEEF;
  const nvcompStatus_t st = dev::decompress(in[c], in_bytes[c], r, kLdsChunk, &got);
  dev::wave_sync();
  uint8_t* o = (uint8_t*)out[c];
  for (size_t i = lane; i < got && i < kLdsChunk; i += 64) {
    o[i] = r[i];
  }
  if (lane == 0) {
    actual[c] = got;
    status[c] = (int)st;
  }
}

#endif

#if BCDEV_HAS(0)
/* decompressed_size() and stream_element_bytes() / stream_type(), one thread per chunk */
__global__ void __launch_bounds__(256) k_sizes(const void* const* in, const size_t* in_bytes, size_t* sizes, uint32_t* elems,
                                               int* types, size_t count)
{
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < count) {
    sizes[c] = dev::decompressed_size(in[c], in_bytes[c]);
    elems[c] = dev::stream_element_bytes(in[c], in_bytes[c]);
    types[c] = (int)dev::stream_type(in[c], in_bytes[c]);
  }
}

/* quantize / dequantize, one thread per element: width 2 (fp16 as bits), 4 or 8 */
__global__ void __launch_bounds__(256) k_quant(const void* x, void* q, void* back, size_t n, uint32_t width, double delta)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) {
    return;
  }
  if (width == 2) {
    const int16_t v = dev::quantize_half_bits(((const uint16_t*)x)[i], (float)delta);
    ((int16_t*)q)[i] = v;
    ((uint16_t*)back)[i] = dev::dequantize_half_bits(v, (float)delta);
  } else if (width == 4) {
    const int32_t v = dev::quantize(((const float*)x)[i], (float)delta);
    ((int32_t*)q)[i] = v;
    ((float*)back)[i] = dev::dequantize(v, (float)delta);
  } else {
    const int64_t v = dev::quantize(((const double*)x)[i], delta);
    ((int64_t*)q)[i] = v;
    ((double*)back)[i] = dev::dequantize(v, delta);
  }
}

/* The fused producer: fp32 values quantised inside the source of compress_from<int32_t> */
__global__ void __launch_bounds__(256) k_quant_compress(const void* const* in, const size_t* in_bytes, void* const* out,
                                                        size_t* out_bytes, size_t count, float delta, int algo)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const size_t c = (size_t)blockIdx.x * 4 + w;
  if (c >= count) {
    return;
  }
  const float* x = (const float*)in[c];
  const size_t r = dev::compress_from<int32_t>(in_bytes[c] / 4, out[c], algo, [&](uint32_t i) { return dev::quantize(x[i], delta); });
  if (lane == 0) {
    out_bytes[c] = r;
  }
}

/* The fused consumer: y[i] = y[i] + (a * (q * delta)). Three roundings in that order -- the product q * delta
 * (dequantize), its product with a, the sum with y[i] -- and no fused multiply-add. */
__global__ void __launch_bounds__(256) k_fused_axpy(const void* const* in, const size_t* in_bytes, const size_t* caps,
                                                    void* const* y, float a, float delta, int* status, size_t count)
{
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const size_t c = (size_t)blockIdx.x * 4 + w;
  if (c >= count) {
    return;
  }
  float* yy = (float*)y[c];
  const nvcompStatus_t st = dev::decompress_to<int32_t>(in[c], in_bytes[c], caps[c], nullptr, nullptr, [&](uint32_t i, int32_t q) {
    yy[i] = add_product(yy[i], a, dev::dequantize(q, delta));
  });
  if (lane == 0) {
    status[c] = (int)st;
  }
}

#endif

int last_error()
{
  return (int)hipGetLastError();
}

} // namespace

extern "C" {

#if BCDEV_HAS(0)
int bcdev_compress(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count, int type,
                   int algo, unsigned mode, unsigned block, unsigned grid, uint32_t* const* counts, uint32_t* flags,
                   hipStream_t stream)
{
  if (mode == 0) {
    hipLaunchKernelGGL(k_compress, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, out_bytes, count, type, algo);
    return last_error();
  }
  const unsigned elem = dev::element_bytes((nvcompType_t)type);
  return (elem < 4 ? bcdev_compress_from_narrow : bcdev_compress_from_wide)(in, in_bytes, out, out_bytes, count, algo, elem, block,
                                                                           grid, mode == 2 ? counts : nullptr, flags, stream);
}

#endif

#if BCDEV_HAS(1)
int bcdev_compress_from_narrow(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                               int algo, unsigned elem, unsigned block, unsigned grid, uint32_t* const* counts,
                               uint32_t* flags, hipStream_t stream)
{
  if (elem == 1) {
    hipLaunchKernelGGL(k_compress_from<uint8_t>, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, out_bytes, count, algo,
                       counts, flags);
  } else {
    hipLaunchKernelGGL(k_compress_from<uint16_t>, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, out_bytes, count, algo,
                       counts, flags);
  }
  return last_error();
}
#endif

#if BCDEV_HAS(2)
int bcdev_compress_from_wide(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                             int algo, unsigned elem, unsigned block, unsigned grid, uint32_t* const* counts, uint32_t* flags,
                             hipStream_t stream)
{
  if (elem == 4) {
    hipLaunchKernelGGL(k_compress_from<uint32_t>, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, out_bytes, count, algo,
                       counts, flags);
  } else {
    hipLaunchKernelGGL(k_compress_from<uint64_t>, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, out_bytes, count, algo,
                       counts, flags);
  }
  return last_error();
}
#endif

#if BCDEV_HAS(3)
int bcdev_decompress(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                     int* status, size_t count, unsigned mode, unsigned elem, unsigned block, unsigned grid, uint8_t* tails,
                     uint32_t* flags, hipStream_t stream)
{
  if (mode == 0) {
    hipLaunchKernelGGL(k_decompress, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, caps, actual, status, count);
    return last_error();
  }
  return (elem < 4 ? bcdev_decompress_to_narrow : bcdev_decompress_to_wide)(in, in_bytes, out, caps, actual, status, count, mode,
                                                                           elem, block, grid, tails, flags, stream);
}
#endif

#if BCDEV_HAS(4)
int bcdev_decompress_to_narrow(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps,
                               size_t* actual, int* status, size_t count, unsigned mode, unsigned elem, unsigned block,
                               unsigned grid, uint8_t* tails, uint32_t* flags, hipStream_t stream)
{
  if (elem == 1) {
    hipLaunchKernelGGL(k_decompress_to<uint8_t>, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, caps, actual, status,
                       count, (uint32_t)mode, tails, flags);
  } else {
    hipLaunchKernelGGL(k_decompress_to<uint16_t>, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, caps, actual, status,
                       count, (uint32_t)mode, tails, flags);
  }
  return last_error();
}
#endif

#if BCDEV_HAS(5)
int bcdev_decompress_to_wide(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps,
                             size_t* actual, int* status, size_t count, unsigned mode, unsigned elem, unsigned block,
                             unsigned grid, uint8_t* tails, uint32_t* flags, hipStream_t stream)
{
  if (elem == 4) {
    hipLaunchKernelGGL(k_decompress_to<uint32_t>, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, caps, actual, status,
                       count, (uint32_t)mode, tails, flags);
  } else {
    hipLaunchKernelGGL(k_decompress_to<uint64_t>, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, caps, actual, status,
                       count, (uint32_t)mode, tails, flags);
  }
  return last_error();
}
#endif

#if BCDEV_HAS(6)
int bcdev_mixed(const void* const* comp_in, const size_t* comp_in_bytes, void* const* dec_out, const size_t* caps,
                size_t* actual, int* status, const void* const* raw, const size_t* raw_bytes, void* const* comp_out,
                size_t* comp_out_bytes, size_t count, int algo, uint32_t* side, unsigned iters, unsigned block,
                unsigned grid, hipStream_t stream)
{
  hipLaunchKernelGGL(k_mixed, dim3(grid), dim3(block), 0, stream, comp_in, comp_in_bytes, dec_out, caps, actual, status, raw,
                     raw_bytes, comp_out, comp_out_bytes, count, algo, side, (uint32_t)iters);
  return last_error();
}
#endif

#if BCDEV_HAS(7)
int bcdev_lds_compress(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                       int type, int algo, unsigned misalign, hipStream_t stream)
{
  hipLaunchKernelGGL(k_lds_compress, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, in, in_bytes, out, out_bytes,
                     count, type, algo, (uint32_t)misalign);
  return last_error();
}

#endif

#if BCDEV_HAS(6)
int bcdev_lds_decompress(const void* const* in, const size_t* in_bytes, void* const* out, size_t* actual, int* status,
                         size_t count, unsigned misalign, hipStream_t stream)
{
  hipLaunchKernelGGL(k_lds_decompress, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, in, in_bytes, out, actual,
                     status, count, (uint32_t)misalign);
  return last_error();
}

#endif

#if BCDEV_HAS(0)
int bcdev_sizes(const void* const* in, const size_t* in_bytes, size_t* sizes, uint32_t* elems, int* types, size_t count,
                hipStream_t stream)
{
  hipLaunchKernelGGL(k_sizes, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, in, in_bytes, sizes, elems, types,
                     count);
  return last_error();
}

int bcdev_quant(const void* x, void* q, void* back, size_t n, unsigned width, double delta, hipStream_t stream)
{
  hipLaunchKernelGGL(k_quant, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, q, back, n, (uint32_t)width, delta);
  return last_error();
}

int bcdev_quant_compress(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                         float delta, int algo, hipStream_t stream)
{
  hipLaunchKernelGGL(k_quant_compress, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, in, in_bytes, out, out_bytes,
                     count, delta, algo);
  return last_error();
}

int bcdev_fused_axpy(const void* const* in, const size_t* in_bytes, const size_t* caps, void* const* y, float a, float delta,
                     int* status, size_t count, hipStream_t stream)
{
  hipLaunchKernelGGL(k_fused_axpy, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, in, in_bytes, caps, y, a, delta,
                     status, count);
  return last_error();
}

size_t bcdev_max_compressed_bytes(size_t n, int type)
{
  return dev::max_compressed_bytes(n, (nvcompType_t)type);
}

size_t bcdev_max_chunk_bytes()
{
  return dev::kMaxChunkBytes;
}
#endif

} // extern "C"
