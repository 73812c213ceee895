/*
 * tests/device_api/cascaded_device_kernels.hip -- TEST ONLY: kernels that call the device-side Cascaded API
 * (include/nvcomp/device/cascaded.hpp), behind extern "C" launchers that tests/test_cascaded_device.py drives through
 * ctypes. One source for both tiers: the MI355X (hipcc --offload-arch=gfx950 -shared -fPIC -I include) and the host
 * emulation (g++ -x c++ -Itests/emu -Iinclude ... -lnvcomp_emu).
 *
 * LDS: every kernel takes the workgroup's dynamically sized segment and gives wave w the slice
 * [lead + w * pitch, lead + w * pitch + slice_bytes): the test chooses slice sizes (worst case, one step short, far below)
 * and pitches / leads that are multiples of 16 only, so a slice is "any 16-byte aligned part of a larger array".
 *
 * -DCDEV_PART=0 ... 6 compiles one slice of the file each (the instantiations of the codec take the device compiler a
 * while in one piece); the test builds the slices side by side and links them. Without the macro everything is compiled.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <nvcomp/device/cascaded.hpp>

namespace dev = nvcomp::device::cascaded;

#ifdef CDEV_PART
#define CDEV_HAS(part) (CDEV_PART == (part))
#else
#define CDEV_HAS(part) 1
#endif

#if defined(__HIPCC__)
#define WAVE_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#define CDEV_LDS(name) extern __shared__ __attribute__((aligned(16))) uint8_t name[]
#else
#define WAVE_UNIFORM(x) (x)
#define CDEV_LDS(name) uint8_t* name = emu::dynamic_lds()
#endif

/* where a wave's slice lies in the workgroup's LDS */
struct CdevSlices
{
  uint32_t lead, pitch, bytes;
};

/* launchers of the other parts, called by the dispatching ones */
extern "C" {
int cdev_compress_from_narrow(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                              nvcompBatchedCascadedOpts_t opts, CdevSlices sl, unsigned block, unsigned grid, uint32_t* flags,
                              hipStream_t stream);
int cdev_compress_from_wide(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                            nvcompBatchedCascadedOpts_t opts, CdevSlices sl, unsigned block, unsigned grid, uint32_t* flags,
                            hipStream_t stream);
int cdev_decompress_to_narrow(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                              int* status, size_t count, unsigned mode, unsigned elem, CdevSlices sl, unsigned block, unsigned grid,
                              uint32_t* const* counts, unsigned long long* sums, uint32_t* flags, hipStream_t stream);
int cdev_decompress_to_wide(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                            int* status, size_t count, unsigned mode, unsigned elem, CdevSlices sl, unsigned block, unsigned grid,
                            uint32_t* const* counts, unsigned long long* sums, uint32_t* flags, hipStream_t stream);
}

namespace {

constexpr uint32_t kLdsChunk = 16384; /* the chunk the LDS kernel stages */
constexpr uint32_t kLdsSlice = 16384; /* ... and its codec slice: above both worst cases of {4096, 4-byte, 2 RLEs} */

enum : uint32_t { kSinkOutOfRange = 1, kSourceOutOfRange = 2 };

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

__device__ inline uint8_t* slice_of(uint8_t* lds, const CdevSlices& sl, uint32_t w)
{
  return lds + sl.lead + (size_t)w * sl.pitch;
}

#if CDEV_HAS(0)
/* compress() of every chunk */
__global__ void __launch_bounds__(256) k_compress(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes,
                                                  size_t count, nvcompBatchedCascadedOpts_t opts, CdevSlices sl)
{
  CDEV_LDS(lds);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    const size_t r = dev::compress(in[c], in_bytes[c], out[c], opts, slice_of(lds, sl, w), sl.bytes);
    if (lane == 0) {
      out_bytes[c] = r;
    }
  }
}
#endif

#if CDEV_HAS(1) || CDEV_HAS(2)
/* compress_from<U>() over the elements of in[0, n) through a memory source, which flags a call for an element that does
 * not exist */
template <class U>
__global__ void __launch_bounds__(256) k_compress_from(const void* const* in, const size_t* in_bytes, void* const* out,
                                                       size_t* out_bytes, size_t count, nvcompBatchedCascadedOpts_t opts,
                                                       CdevSlices sl, uint32_t* flags)
{
  CDEV_LDS(lds);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    const void* src = in[c];
    const size_t n_elems = in_bytes[c] / sizeof(U);
    const size_t r = dev::compress_from<U>(n_elems, out[c], opts, slice_of(lds, sl, w), sl.bytes, [&](uint32_t i) {
      if (i >= n_elems) {
        atomicOr(flags, (uint32_t)kSourceOutOfRange);
        return (U)0;
      }
      return load_as<U>(src, i);
    });
    if (lane == 0) {
      out_bytes[c] = r;
    }
  }
}
#endif

#if CDEV_HAS(3)
/* decompress() of every chunk into out */
__global__ void __launch_bounds__(256) k_decompress(const void* const* in, const size_t* in_bytes, void* const* out,
                                                    const size_t* caps, size_t* actual, int* status, size_t count, CdevSlices sl)
{
  CDEV_LDS(lds);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    size_t got = 0xDEADBEEF;
    const nvcompStatus_t st = dev::decompress(in[c], in_bytes[c], out[c], caps[c], &got, slice_of(lds, sl, w), sl.bytes);
    if (lane == 0) {
      actual[c] = got;
      status[c] = (int)st;
    }
  }
}
#endif

#if CDEV_HAS(4) || CDEV_HAS(5)
/* decompress_to<U>(): mode 1 stores element i into out[c] and counts the call in counts[c][i]; mode 2 adds the elements
 * up, a partial sum per lane, into sums[c] (unsigned 64-bit, wrapping). A call for an element beyond the capacity is
 * flagged, not carried out. */
template <class U>
__global__ void __launch_bounds__(256) k_decompress_to(const void* const* in, const size_t* in_bytes, void* const* out,
                                                       const size_t* caps, size_t* actual, int* status, size_t count, uint32_t mode,
                                                       CdevSlices sl, uint32_t* const* counts, unsigned long long* sums,
                                                       uint32_t* flags)
{
  CDEV_LDS(lds);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    const size_t cap_elems = caps[c] / sizeof(U);
    size_t got = 0xDEADBEEF;
    nvcompStatus_t st;
    if (mode == 1) {
      uint8_t* o = (uint8_t*)out[c];
      uint32_t* cnt = counts[c];
      st = dev::decompress_to<U>(in[c], in_bytes[c], caps[c], &got, slice_of(lds, sl, w), sl.bytes, [&](uint32_t i, U v) {
        if (i >= cap_elems) {
          atomicOr(flags, (uint32_t)kSinkOutOfRange);
        } else {
          atomicAdd(&cnt[i], 1u);
          store_as<U>(o, i, v);
        }
      });
    } else {
      unsigned long long part = 0;
      st = dev::decompress_to<U>(in[c], in_bytes[c], caps[c], &got, slice_of(lds, sl, w), sl.bytes, [&](uint32_t i, U v) {
        if (i >= cap_elems) {
          atomicOr(flags, (uint32_t)kSinkOutOfRange);
        } else {
          part += (unsigned long long)v;
        }
      });
      atomicAdd(&sums[c], part);
    }
    if (lane == 0) {
      actual[c] = got;
      status[c] = (int)st;
    }
  }
}
#endif

#if CDEV_HAS(6)
/* A workgroup of four waves, no barrier anywhere: wave 0 decodes chunk 2 b (decompress()), wave 1 has returned, wave 2
 * only spins on arithmetic (a xorshift chain of `iters` steps per lane into side[]), wave 3 decodes chunk 2 b + 1 through
 * a storing sink. The two slices are parts of one array: [lead, lead + bytes) and [lead + 3 pitch, ...). */
__global__ void __launch_bounds__(256) k_mixed(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps,
                                               size_t* actual, int* status, size_t count, CdevSlices sl, uint32_t* side,
                                               uint32_t iters)
{
  CDEV_LDS(lds);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  if (w == 1) {
    return;
  }
  if (w == 2) {
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
  const size_t j = 2 * (size_t)blockIdx.x + (w == 3 ? 1 : 0);
  if (j >= count) {
    return;
  }
  size_t got = 0xDEADBEEF;
  nvcompStatus_t st;
  if (w == 0) {
    st = dev::decompress(in[j], in_bytes[j], out[j], caps[j], &got, slice_of(lds, sl, w), sl.bytes);
  } else {
    uint32_t* o = (uint32_t*)out[j];
    const size_t cap_elems = caps[j] / 4;
    st = dev::decompress_to<uint32_t>(in[j], in_bytes[j], caps[j], &got, slice_of(lds, sl, w), sl.bytes, [&](uint32_t i, uint32_t v) {
      if (i < cap_elems) {
        o[i] = v;
      }
    });
  }
  if (lane == 0) {
    actual[j] = got;
    status[j] = (int)st;
  }
}

/* One wave per workgroup, everything in LDS: the stream in[c] is decoded into an LDS buffer, consumed there (its uint32
 * elements summed into sums[c], the bytes copied to dec_out[c]); then raw[c] is staged in the same buffer and compressed
 * from LDS into comp_out[c]. Chunks of at most kLdsChunk bytes. */
__global__ void __launch_bounds__(64) k_lds(const void* const* in, const size_t* in_bytes, void* const* dec_out, size_t* actual,
                                            int* status, unsigned long long* sums, const void* const* raw, const size_t* raw_bytes,
                                            void* const* comp_out, size_t* comp_out_bytes, size_t count,
                                            nvcompBatchedCascadedOpts_t opts)
{
  CDEV_LDS(lds);
  uint8_t* chunk = lds;
  uint8_t* slice = lds + kLdsChunk;
  const uint32_t lane = threadIdx.x & 63;
  const size_t c = blockIdx.x;
  if (c >= count) {
    return;
  }
  size_t got = 0xDEADBEEF;
  const nvcompStatus_t st = dev::decompress(in[c], in_bytes[c], chunk, kLdsChunk, &got, slice, kLdsSlice);
  dev::wave_sync();
  unsigned long long part = 0;
  uint8_t* o = (uint8_t*)dec_out[c];
  for (size_t i = lane; i < got / 4 && i < kLdsChunk / 4; i += 64) {
    const uint32_t v = ((const uint32_t*)chunk)[i];
    part += v;
    ((uint32_t*)o)[i] = v;
  }
  atomicAdd(&sums[c], part);
  if (lane == 0) {
    actual[c] = got;
    status[c] = (int)st;
  }
  dev::wave_sync();
  const size_t n = raw_bytes[c] < kLdsChunk ? raw_bytes[c] : kLdsChunk;
  const uint8_t* src = (const uint8_t*)raw[c];
  for (size_t i = lane; i < n; i += 64) {
    chunk[i] = src[i];
  }
  dev::wave_sync();
  const size_t zn = dev::compress(chunk, n, comp_out[c], opts, slice, kLdsSlice);
  if (lane == 0) {
    comp_out_bytes[c] = zn;
  }
}
#endif

#if CDEV_HAS(0)
/* the header queries, one thread per chunk */
__global__ void __launch_bounds__(256) k_sizes(const void* const* in, const size_t* in_bytes, size_t* sizes, uint32_t* elems,
                                               int* types, size_t* shared, size_t count)
{
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < count) {
    sizes[c] = dev::decompressed_size(in[c], in_bytes[c]);
    elems[c] = dev::stream_element_bytes(in[c], in_bytes[c]);
    types[c] = (int)dev::stream_type(in[c], in_bytes[c]);
    shared[c] = dev::stream_shared_bytes(in[c], in_bytes[c]);
  }
}
#endif

int last_error()
{
  return (int)hipGetLastError();
}

} // namespace

extern "C" {

#if CDEV_HAS(0)
int cdev_compress(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                  nvcompBatchedCascadedOpts_t opts, unsigned mode, CdevSlices sl, unsigned lds_bytes, unsigned block, unsigned grid,
                  uint32_t* flags, hipStream_t stream)
{
  (void)lds_bytes; /* (the host emulation's launch macro has no LDS size) */
  if (mode == 0) {
    hipLaunchKernelGGL(k_compress, dim3(grid), dim3(block), lds_bytes, stream, in, in_bytes, out, out_bytes, count, opts, sl);
    return last_error();
  }
  const unsigned elem = dev::element_bytes(opts.type);
  return (elem < 4 ? cdev_compress_from_narrow : cdev_compress_from_wide)(in, in_bytes, out, out_bytes, count, opts, sl, block, grid,
                                                                         flags, stream);
}

int cdev_sizes(const void* const* in, const size_t* in_bytes, size_t* sizes, uint32_t* elems, int* types, size_t* shared,
               size_t count, hipStream_t stream)
{
  hipLaunchKernelGGL(k_sizes, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, in, in_bytes, sizes, elems, types, shared,
                     count);
  return last_error();
}

size_t cdev_max_compressed_bytes(size_t n, nvcompBatchedCascadedOpts_t opts)
{
  return dev::max_compressed_bytes(n, opts);
}

size_t cdev_compress_shared_bytes(nvcompBatchedCascadedOpts_t opts)
{
  return dev::compress_shared_bytes(opts);
}

size_t cdev_decompress_shared_bytes(nvcompBatchedCascadedOpts_t opts)
{
  return dev::decompress_shared_bytes(opts);
}

size_t cdev_max_chunk_bytes()
{
  return dev::kMaxChunkBytes;
}
#endif

/* (compress_from is launched with the slices' extent as its LDS size) */
#if CDEV_HAS(1)
int cdev_compress_from_narrow(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                              nvcompBatchedCascadedOpts_t opts, CdevSlices sl, unsigned block, unsigned grid, uint32_t* flags,
                              hipStream_t stream)
{
  const unsigned lds_bytes = sl.lead + (block / 64 - 1) * sl.pitch + sl.bytes;
  (void)lds_bytes;
  if (dev::element_bytes(opts.type) == 1) {
    hipLaunchKernelGGL(k_compress_from<uint8_t>, dim3(grid), dim3(block), lds_bytes, stream, in, in_bytes, out, out_bytes, count, opts,
                       sl, flags);
  } else {
    hipLaunchKernelGGL(k_compress_from<uint16_t>, dim3(grid), dim3(block), lds_bytes, stream, in, in_bytes, out, out_bytes, count, opts,
                       sl, flags);
  }
  return last_error();
}
#endif

#if CDEV_HAS(2)
int cdev_compress_from_wide(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                            nvcompBatchedCascadedOpts_t opts, CdevSlices sl, unsigned block, unsigned grid, uint32_t* flags,
                            hipStream_t stream)
{
  const unsigned lds_bytes = sl.lead + (block / 64 - 1) * sl.pitch + sl.bytes;
  (void)lds_bytes;
  if (dev::element_bytes(opts.type) == 4) {
    hipLaunchKernelGGL(k_compress_from<uint32_t>, dim3(grid), dim3(block), lds_bytes, stream, in, in_bytes, out, out_bytes, count, opts,
                       sl, flags);
  } else {
    hipLaunchKernelGGL(k_compress_from<uint64_t>, dim3(grid), dim3(block), lds_bytes, stream, in, in_bytes, out, out_bytes, count, opts,
                       sl, flags);
  }
  return last_error();
}
#endif

#if CDEV_HAS(3)
int cdev_decompress(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual, int* status,
                    size_t count, unsigned mode, unsigned elem, CdevSlices sl, unsigned block, unsigned grid, uint32_t* const* counts,
                    unsigned long long* sums, uint32_t* flags, hipStream_t stream)
{
  if (mode == 0) {
    const unsigned lds_bytes = sl.lead + (block / 64 - 1) * sl.pitch + sl.bytes;
    (void)lds_bytes;
    hipLaunchKernelGGL(k_decompress, dim3(grid), dim3(block), lds_bytes, stream, in, in_bytes, out, caps, actual, status, count, sl);
    return last_error();
  }
  return (elem < 4 ? cdev_decompress_to_narrow : cdev_decompress_to_wide)(in, in_bytes, out, caps, actual, status, count, mode, elem, sl,
                                                                         block, grid, counts, sums, flags, stream);
}
#endif

#if CDEV_HAS(4)
int cdev_decompress_to_narrow(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                              int* status, size_t count, unsigned mode, unsigned elem, CdevSlices sl, unsigned block, unsigned grid,
                              uint32_t* const* counts, unsigned long long* sums, uint32_t* flags, hipStream_t stream)
{
  const unsigned lds_bytes = sl.lead + (block / 64 - 1) * sl.pitch + sl.bytes;
  (void)lds_bytes;
  if (elem == 1) {
    hipLaunchKernelGGL(k_decompress_to<uint8_t>, dim3(grid), dim3(block), lds_bytes, stream, in, in_bytes, out, caps, actual, status,
                       count, (uint32_t)mode, sl, counts, sums, flags);
  } else {
    hipLaunchKernelGGL(k_decompress_to<uint16_t>, dim3(grid), dim3(block), lds_bytes, stream, in, in_bytes, out, caps, actual, status,
                       count, (uint32_t)mode, sl, counts, sums, flags);
  }
  return last_error();
}
#endif

#if CDEV_HAS(5)
int cdev_decompress_to_wide(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                            int* status, size_t count, unsigned mode, unsigned elem, CdevSlices sl, unsigned block, unsigned grid,
                            uint32_t* const* counts, unsigned long long* sums, uint32_t* flags, hipStream_t stream)
{
  const unsigned lds_bytes = sl.lead + (block / 64 - 1) * sl.pitch + sl.bytes;
  (void)lds_bytes;
  if (elem == 4) {
    hipLaunchKernelGGL(k_decompress_to<uint32_t>, dim3(grid), dim3(block), lds_bytes, stream, in, in_bytes, out, caps, actual, status,
                       count, (uint32_t)mode, sl, counts, sums, flags);
  } else {
    hipLaunchKernelGGL(k_decompress_to<uint64_t>, dim3(grid), dim3(block), lds_bytes, stream, in, in_bytes, out, caps, actual, status,
                       count, (uint32_t)mode, sl, counts, sums, flags);
  }
  return last_error();
}
#endif

#if CDEV_HAS(6)
int cdev_mixed(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual, int* status,
               size_t count, CdevSlices sl, uint32_t* side, unsigned iters, unsigned grid, hipStream_t stream)
{
  const unsigned lds_bytes = sl.lead + 3 * sl.pitch + sl.bytes;
  (void)lds_bytes;
  hipLaunchKernelGGL(k_mixed, dim3(grid), dim3(256), lds_bytes, stream, in, in_bytes, out, caps, actual, status, count, sl, side,
                     (uint32_t)iters);
  return last_error();
}

int cdev_lds(const void* const* in, const size_t* in_bytes, void* const* dec_out, size_t* actual, int* status,
             unsigned long long* sums, const void* const* raw, const size_t* raw_bytes, void* const* comp_out, size_t* comp_out_bytes,
             size_t count, nvcompBatchedCascadedOpts_t opts, hipStream_t stream)
{
  hipLaunchKernelGGL(k_lds, dim3((unsigned)count), dim3(64), kLdsChunk + kLdsSlice, stream, in, in_bytes, dec_out, actual, status, sums,
                     raw, raw_bytes, comp_out, comp_out_bytes, count, opts);
  return last_error();
}
#endif

} // extern "C"
