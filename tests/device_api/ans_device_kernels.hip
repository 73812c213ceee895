/*
 * tests/device_api/ans_device_kernels.hip -- TEST ONLY: kernels that call the device-side ANS API
 * (include/nvcomp/device/ans.hpp), behind extern "C" launchers that tests/test_ans_device.py drives through ctypes.
 * One source for both tiers: the MI355X (hipcc --offload-arch=gfx950 -shared -fPIC -I include) and the host emulation
 * (g++ -x c++ -Itests/emu -Iinclude ... -lnvcomp_emu).
 *
 * Every wave's `shared` area in LDS sits between 16 guard bytes on either side; a kernel that finds a guard changed
 * sets kBadGuard in *flags. Launch shapes: 64, 256 or 1 024 threads; with fewer waves than chunks a wave loops over
 * several chunks and reuses its area.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <nvcomp/device/ans.hpp>

namespace dev = nvcomp::device::ans;

#if defined(__HIP_DEVICE_COMPILE__)
#define WAVE_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define WAVE_UNIFORM(x) (x)
#endif

namespace {

constexpr unsigned kMaxWaves = 16; /* 1 024-thread workgroups */
constexpr unsigned kGuardBytes = 16;
constexpr size_t kCompSlot = dev::kCompressSharedBytes + 2 * kGuardBytes;
constexpr size_t kDecSlot = dev::kDecompressSharedBytes + 2 * kGuardBytes;
constexpr size_t kLdsChunk = 6144; /* the largest chunk the LDS kernel stages */
constexpr size_t kLdsComp = dev::max_compressed_bytes(kLdsChunk);

enum : uint32_t { kBadGuard = 1, kBadSinkCall = 2, kSinkOutOfRange = 4 };

__device__ inline uint32_t guard_word(uint32_t i)
{
  return (0x9E3779B9u * (i + 1)) ^ 0xA5C3E1F7u;
}

/* lanes 0-3: the 16 bytes in front of the area, lanes 4-7: the 16 behind it */
__device__ inline uint32_t* guard_at(uint8_t* slot, size_t area, uint32_t lane)
{
  return (uint32_t*)(lane < 4 ? slot : slot + kGuardBytes + area) + (lane & 3);
}

__device__ inline void set_guards(uint8_t* slot, size_t area, uint32_t lane)
{
  if (lane < 8) {
    *guard_at(slot, area, lane) = guard_word(lane);
  }
}

__device__ inline void check_guards(uint8_t* slot, size_t area, uint32_t lane, uint32_t* flags)
{
  if (lane < 8 && *guard_at(slot, area, lane) != guard_word(lane)) {
    atomicOr(flags, (uint32_t)kBadGuard);
  }
}

__global__ void __launch_bounds__(1024) k_compress(const void* const* in, const size_t* in_bytes, void* const* out,
                                                   size_t* out_bytes, size_t count, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kMaxWaves][kCompSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  uint8_t* slot = lds[w];
  set_guards(slot, dev::kCompressSharedBytes, lane);
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    const size_t r = dev::compress(in[c], in_bytes[c], out[c], slot + kGuardBytes);
    if (lane == 0) {
      out_bytes[c] = r;
    }
    check_guards(slot, dev::kCompressSharedBytes, lane, flags);
  }
}

/* mode 0: decompress() into out; 1: decompress_to() with a sink that stores the bytes into out; 2: decompress_to()
 * with a sink that counts every byte it is handed (out holds one uint32 counter per byte of the capacity) */
__global__ void __launch_bounds__(1024) k_decompress(const void* const* in, const size_t* in_bytes, void* const* out,
                                                     const size_t* caps, size_t* actual, int* status, size_t count,
                                                     uint32_t mode, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kMaxWaves][kDecSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  uint8_t* slot = lds[w];
  set_guards(slot, dev::kDecompressSharedBytes, lane);
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    uint8_t* o = (uint8_t*)out[c];
    const size_t cap = caps[c];
    size_t got = 0xDEADBEEF;
    nvcompStatus_t st;
    if (mode == 0) {
      st = dev::decompress(in[c], in_bytes[c], o, cap, &got, slot + kGuardBytes);
    } else if (mode == 1) {
      st = dev::decompress_to(in[c], in_bytes[c], cap, &got, slot + kGuardBytes, [&](uint32_t off, uint32_t v, uint32_t nb) {
        if (off % 4 != 0 || nb < 1 || nb > 4 || (nb < 4 && (v >> (8 * nb)) != 0)) {
          atomicOr(flags, (uint32_t)kBadSinkCall);
        }
        for (uint32_t k = 0; k < nb && k < 4; ++k) {
          if (off + k < cap) {
            o[off + k] = (uint8_t)(v >> (8 * k));
          } else {
            atomicOr(flags, (uint32_t)kSinkOutOfRange);
          }
        }
      });
    } else {
      uint32_t* counts = (uint32_t*)o;
      st = dev::decompress_to(in[c], in_bytes[c], cap, &got, slot + kGuardBytes, [&](uint32_t off, uint32_t v, uint32_t nb) {
        if (off % 4 != 0 || nb < 1 || nb > 4) {
          atomicOr(flags, (uint32_t)kBadSinkCall);
        }
        for (uint32_t k = 0; k < nb && k < 4; ++k) {
          if (off + k < cap) {
            atomicAdd(&counts[off + k], 1u);
          } else {
            atomicOr(flags, (uint32_t)kSinkOutOfRange);
          }
        }
        (void)v;
      });
    }
    if (lane == 0) {
      actual[c] = got;
      status[c] = (int)st;
    }
    check_guards(slot, dev::kDecompressSharedBytes, lane, flags);
  }
}

/* Even waves decode one chunk each (decompress() into out); odd waves meanwhile run unrelated code: a xorshift chain of
 * `iters` steps per lane into side[]. */
__global__ void __launch_bounds__(1024) k_mixed(const void* const* in, const size_t* in_bytes, void* const* out,
                                                const size_t* caps, size_t* actual, int* status, size_t count,
                                                uint32_t* side, uint32_t iters, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kMaxWaves / 2][kDecSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const size_t pairs = blockDim.x >> 7;
  const size_t job = (size_t)blockIdx.x * pairs + (w >> 1);
  if (w & 1) {
    uint32_t x = (uint32_t)(job * 64 + lane) + 1;
    for (uint32_t i = 0; i < iters; ++i) {
      x ^= x << 13;
      x ^= x >> 17;
      x ^= x << 5;
    }
    side[job * 64 + lane] = x;
    return;
  }
  if (job >= count) {
    return;
  }
  uint8_t* slot = lds[w >> 1];
  set_guards(slot, dev::kDecompressSharedBytes, lane);
  size_t got = 0xDEADBEEF;
  const nvcompStatus_t st = dev::decompress(in[job], in_bytes[job], out[job], caps[job], &got, slot + kGuardBytes);
  if (lane == 0) {
    actual[job] = got;
    status[job] = (int)st;
  }
  check_guards(slot, dev::kDecompressSharedBytes, lane, flags);
}

/* Four waves, one chunk (at most kLdsChunk bytes) each, everything in LDS: the chunk is staged at byte `misalign` of an
 * LDS buffer, compressed into another LDS buffer (at `misalign` too), which is copied out to comp_out; then decompressed
 * from there back into the first buffer and copied out to dec_out. */
__global__ void __launch_bounds__(256) k_lds_roundtrip(const void* const* in, const size_t* in_bytes, void* const* comp_out,
                                                       size_t* comp_bytes, void* const* dec_out, size_t* actual, int* status,
                                                       size_t count, uint32_t misalign, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t raw[4][kLdsChunk + 16];
  __shared__ __attribute__((aligned(16))) uint8_t comp[4][kLdsComp + 16];
  __shared__ __attribute__((aligned(16))) uint8_t lds[4][kDecSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const size_t c = (size_t)blockIdx.x * 4 + w;
  if (c >= count) {
    return;
  }
  uint8_t* slot = lds[w];
  set_guards(slot, dev::kDecompressSharedBytes, lane);
  const size_t n = in_bytes[c] < kLdsChunk ? in_bytes[c] : kLdsChunk;
  uint8_t* r = raw[w] + misalign;
  uint8_t* z = comp[w] + misalign;
  const uint8_t* src = (const uint8_t*)in[c];
  for (size_t i = lane; i < n; i += 64) {
    r[i] = src[i];
  }
  dev::wave_sync();
  const size_t zn = dev::compress(r, n, z, slot + kGuardBytes);
  check_guards(slot, dev::kDecompressSharedBytes, lane, flags);
  dev::wave_sync();
  uint8_t* zo = (uint8_t*)comp_out[c];
  for (size_t i = lane; i < zn; i += 64) {
    zo[i] = z[i];
  }
  for (size_t i = lane; i < n; i += 64) {
    r[i] = 0;
  }
  if (lane == 0) {
    comp_bytes[c] = zn;
  }
  dev::wave_sync();
  size_t got = 0xDEADBEEF;
  const nvcompStatus_t st = dev::decompress(z, zn, r, kLdsChunk, &got, slot + kGuardBytes);
  check_guards(slot, dev::kDecompressSharedBytes, lane, flags);
  dev::wave_sync();
  uint8_t* dout = (uint8_t*)dec_out[c];
  for (size_t i = lane; i < got && i < n; i += 64) {
    dout[i] = r[i];
  }
  if (lane == 0) {
    actual[c] = got;
    status[c] = (int)st;
  }
}

/* decompressed_size(), one thread per chunk */
__global__ void __launch_bounds__(256) k_sizes(const void* const* in, const size_t* in_bytes, size_t* sizes, size_t count)
{
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < count) {
    sizes[c] = dev::decompressed_size(in[c], in_bytes[c]);
  }
}

/* The fused consumer: each decoded byte b becomes book[b] (a 256-entry codebook of T: fp16 or fp32 bit patterns) */
template <class T>
__global__ void __launch_bounds__(256) k_codebook(const void* const* in, const size_t* in_bytes, const size_t* caps,
                                                  void* const* out, const T* codebook, int* status, size_t count)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[4][dev::kDecompressSharedBytes];
  __shared__ T book[256];
  for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) {
    book[i] = codebook[i];
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const size_t c = (size_t)blockIdx.x * 4 + w;
  if (c >= count) {
    return;
  }
  T* o = (T*)out[c];
  const nvcompStatus_t st = dev::decompress_to(in[c], in_bytes[c], caps[c], nullptr, lds[w], [&](uint32_t off, uint32_t v, uint32_t nb) {
    for (uint32_t k = 0; k < nb; ++k) {
      o[off + k] = book[(v >> (8 * k)) & 255u];
    }
  });
  if (lane == 0) {
    status[c] = (int)st;
  }
}

int last_error()
{
  return (int)hipGetLastError();
}

} // namespace

extern "C" {

int ansdev_compress(const void* const* in, const size_t* in_bytes, void* const* out, size_t* out_bytes, size_t count,
                    unsigned block, unsigned grid, uint32_t* flags, hipStream_t stream)
{
  hipLaunchKernelGGL(k_compress, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, out_bytes, count, flags);
  return last_error();
}

int ansdev_decompress(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                      int* status, size_t count, unsigned mode, unsigned block, unsigned grid, uint32_t* flags,
                      hipStream_t stream)
{
  hipLaunchKernelGGL(k_decompress, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, caps, actual, status, count,
                     (uint32_t)mode, flags);
  return last_error();
}

int ansdev_mixed(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                 int* status, size_t count, uint32_t* side, unsigned iters, unsigned block, unsigned grid, uint32_t* flags,
                 hipStream_t stream)
{
  hipLaunchKernelGGL(k_mixed, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, caps, actual, status, count, side,
                     (uint32_t)iters, flags);
  return last_error();
}

int ansdev_lds_roundtrip(const void* const* in, const size_t* in_bytes, void* const* comp_out, size_t* comp_bytes,
                         void* const* dec_out, size_t* actual, int* status, size_t count, unsigned misalign, uint32_t* flags,
                         hipStream_t stream)
{
  hipLaunchKernelGGL(k_lds_roundtrip, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, in, in_bytes, comp_out,
                     comp_bytes, dec_out, actual, status, count, (uint32_t)misalign, flags);
  return last_error();
}

int ansdev_sizes(const void* const* in, const size_t* in_bytes, size_t* sizes, size_t count, hipStream_t stream)
{
  hipLaunchKernelGGL(k_sizes, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, in, in_bytes, sizes, count);
  return last_error();
}

int ansdev_codebook(const void* const* in, const size_t* in_bytes, const size_t* caps, void* const* out, const void* codebook,
                    unsigned elem_bytes, int* status, size_t count, hipStream_t stream)
{
  const dim3 grid((unsigned)((count + 3) / 4));
  if (elem_bytes == 2) {
    hipLaunchKernelGGL(k_codebook<uint16_t>, grid, dim3(256), 0, stream, in, in_bytes, caps, out, (const uint16_t*)codebook,
                       status, count);
  } else {
    hipLaunchKernelGGL(k_codebook<uint32_t>, grid, dim3(256), 0, stream, in, in_bytes, caps, out, (const uint32_t*)codebook,
                       status, count);
  }
  return last_error();
}

size_t ansdev_max_compressed_bytes(size_t n)
{
  return dev::max_compressed_bytes(n);
}

size_t ansdev_shared_bytes(int decompress)
{
  return decompress ? dev::kDecompressSharedBytes : dev::kCompressSharedBytes;
}

} // extern "C"
