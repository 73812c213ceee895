/*
 * tests/device_api/lz4_device_kernels.hip -- TEST ONLY: kernels that call the device-side LZ4 API
 * (include/nvcomp/device/lz4.hpp), behind extern "C" launchers that tests/test_lz4_device.py drives through ctypes.
 * One source for both tiers: the MI355X (hipcc --offload-arch=gfx950 -shared -fPIC -I include) and the host emulation
 * (g++ -x c++ -Itests/emu -Iinclude ... -lnvcomp_emu).
 *
 * Every wave's `shared` area in LDS sits between 16 guard bytes on either side; a kernel that finds a guard changed
 * sets kBadGuard in *flags. An output in LDS is followed by 16 guard bytes of 0xA5 (kBadLdsGuard). Launch shapes: 64 or
 * 256 threads; with fewer waves than chunks a wave loops over several chunks and reuses its area.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <nvcomp/device/lz4.hpp>

namespace dev = nvcomp::device::lz4;

#if defined(__HIP_DEVICE_COMPILE__)
#define WAVE_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define WAVE_UNIFORM(x) (x)
#endif

namespace {

constexpr unsigned kGuardBytes = 16;
constexpr size_t kDecSlot = dev::kDecompressSharedBytes + 2 * kGuardBytes;
constexpr size_t kLdsOut = 65536 + 1024; /* the output bytes a workgroup keeps in LDS, shared out among its waves */
constexpr size_t kLdsIn = 65536 + 1024;  /* the same for staged input: more than the bound of a 64 KiB chunk */

enum : uint32_t { kBadGuard = 1, kBadLdsGuard = 2 };
enum : int { kTooLargeForLds = -2 };

__device__ inline uint32_t guard_word(uint32_t i)
{
  return (0x9E3779B9u * (i + 1)) ^ 0xA5C3E1F7u;
}

/* lanes 0-3: the 16 bytes in front of the area, lanes 4-7: the 16 behind it */
__device__ inline uint32_t* guard_at(uint8_t* slot, uint32_t lane)
{
  return (uint32_t*)(lane < 4 ? slot : slot + kGuardBytes + dev::kDecompressSharedBytes) + (lane & 3);
}

__device__ inline void set_guards(uint8_t* slot, uint32_t lane)
{
  if (lane < 8) {
    *guard_at(slot, lane) = guard_word(lane);
  }
}

__device__ inline void check_guards(uint8_t* slot, uint32_t lane, uint32_t* flags)
{
  if (lane < 8 && *guard_at(slot, lane) != guard_word(lane)) {
    atomicOr(flags, (uint32_t)kBadGuard);
  }
}

/* global -> global; a wave takes chunks w, w + (waves in the grid), ... and reuses its area */
__global__ void __launch_bounds__(256) k_global(const void* const* in, const size_t* in_bytes, void* const* out,
                                                const size_t* caps, size_t* actual, int* status, size_t count, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[4][kDecSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  uint8_t* slot = lds[w];
  set_guards(slot, lane);
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    size_t got = 0xDEADBEEF;
    const nvcompStatus_t st = dev::decompress(in[c], in_bytes[c], out[c], caps[c], &got, slot + kGuardBytes);
    if (lane == 0) {
      actual[c] = got;
      status[c] = (int)st;
    }
    check_guards(slot, lane, flags);
  }
}

/* The output in LDS (at byte out_align of the wave's buffer), then copied out, all `cap` bytes of it. stage_in: the
 * stream is first staged in LDS by the wave itself (at byte in_align), wave_sync(), and decoded from there. */
template <unsigned WAVES>
__global__ void __launch_bounds__(64 * WAVES) k_lds(const void* const* in, const size_t* in_bytes, void* const* out,
                                                    const size_t* caps, size_t* actual, int* status, size_t count,
                                                    uint32_t stage_in, uint32_t in_align, uint32_t out_align, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t obuf[WAVES][kLdsOut / WAVES + 48];
  __shared__ __attribute__((aligned(16))) uint8_t ibuf[WAVES][kLdsIn / WAVES + 16];
  __shared__ __attribute__((aligned(16))) uint8_t lds[WAVES][kDecSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  uint8_t* slot = lds[w];
  set_guards(slot, lane);
  for (size_t c = (size_t)blockIdx.x * WAVES + w; c < count; c += (size_t)gridDim.x * WAVES) {
    const size_t cap = caps[c];
    const size_t n = in_bytes[c];
    if (cap > kLdsOut / WAVES || (stage_in && n > kLdsIn / WAVES)) {
      if (lane == 0) {
        actual[c] = 0;
        status[c] = kTooLargeForLds;
      }
      continue;
    }
    uint8_t* o = obuf[w] + out_align;
    for (size_t i = lane; i < cap + 16; i += 64) {
      o[i] = 0xA5;
    }
    const uint8_t* src = (const uint8_t*)in[c];
    if (stage_in) {
      uint8_t* s = ibuf[w] + in_align;
      for (size_t i = lane; i < n; i += 64) {
        s[i] = src[i];
      }
      src = s;
    }
    dev::wave_sync();
    size_t got = 0xDEADBEEF;
    const nvcompStatus_t st = dev::decompress(src, n, o, cap, &got, slot + kGuardBytes);
    dev::wave_sync();
    if (lane < 16 && o[cap + lane] != 0xA5) {
      atomicOr(flags, (uint32_t)kBadLdsGuard);
    }
    uint8_t* d = (uint8_t*)out[c];
    for (size_t i = lane; i < cap; i += 64) {
      d[i] = o[i];
    }
    if (lane == 0) {
      actual[c] = got;
      status[c] = (int)st;
    }
    check_guards(slot, lane, flags);
    dev::wave_sync(); /* the copy out before the next chunk's fill */
  }
}

/* Waves 0, 1, 2 of every workgroup decode a chunk each (global -> global); wave 3 does not call at all: a xorshift chain
 * of `iters` steps per lane into side[]. */
__global__ void __launch_bounds__(256) k_mixed(const void* const* in, const size_t* in_bytes, void* const* out,
                                               const size_t* caps, size_t* actual, int* status, size_t count, uint32_t* side,
                                               uint32_t iters, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[3][kDecSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  if (w == 3) {
    uint32_t x = (uint32_t)(blockIdx.x * 64 + lane) + 1;
    for (uint32_t i = 0; i < iters; ++i) {
      x ^= x << 13;
      x ^= x >> 17;
      x ^= x << 5;
    }
    side[blockIdx.x * 64 + lane] = x;
    return;
  }
  const size_t job = (size_t)blockIdx.x * 3 + w;
  if (job >= count) {
    return;
  }
  uint8_t* slot = lds[w];
  set_guards(slot, lane);
  size_t got = 0xDEADBEEF;
  const nvcompStatus_t st = dev::decompress(in[job], in_bytes[job], out[job], caps[job], &got, slot + kGuardBytes);
  if (lane == 0) {
    actual[job] = got;
    status[job] = (int)st;
  }
  check_guards(slot, lane, flags);
}

/* decompressed_size(), one wave per chunk */
__global__ void __launch_bounds__(256) k_sizes(const void* const* in, const size_t* in_bytes, size_t* sizes, int* status,
                                               size_t count)
{
  const uint32_t lane = threadIdx.x & 63;
  const size_t c = (size_t)blockIdx.x * (blockDim.x >> 6) + WAVE_UNIFORM(threadIdx.x >> 6);
  if (c >= count) {
    return;
  }
  size_t got = 0xDEADBEEF;
  const nvcompStatus_t st = dev::decompressed_size(in[c], in_bytes[c], &got);
  if (lane == 0) {
    sizes[c] = got;
    status[c] = (int)st;
  }
}

int last_error()
{
  return (int)hipGetLastError();
}

} // namespace

extern "C" {

int lz4dev_global(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                  int* status, size_t count, unsigned block, unsigned grid, uint32_t* flags, hipStream_t stream)
{
  if (block != 64 && block != 256) {
    return -1;
  }
  hipLaunchKernelGGL(k_global, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, caps, actual, status, count, flags);
  return last_error();
}

int lz4dev_lds(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
               int* status, size_t count, unsigned stage_in, unsigned in_align, unsigned out_align, unsigned block,
               unsigned grid, uint32_t* flags, hipStream_t stream)
{
  if (in_align > 15 || out_align > 15) {
    return -1;
  }
  if (block == 64) {
    hipLaunchKernelGGL(k_lds<1>, dim3(grid), dim3(64), 0, stream, in, in_bytes, out, caps, actual, status, count,
                       (uint32_t)stage_in, (uint32_t)in_align, (uint32_t)out_align, flags);
  } else if (block == 256) {
    hipLaunchKernelGGL(k_lds<4>, dim3(grid), dim3(256), 0, stream, in, in_bytes, out, caps, actual, status, count,
                       (uint32_t)stage_in, (uint32_t)in_align, (uint32_t)out_align, flags);
  } else {
    return -1;
  }
  return last_error();
}

int lz4dev_mixed(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                 int* status, size_t count, uint32_t* side, unsigned iters, unsigned grid, uint32_t* flags, hipStream_t stream)
{
  hipLaunchKernelGGL(k_mixed, dim3(grid), dim3(256), 0, stream, in, in_bytes, out, caps, actual, status, count, side,
                     (uint32_t)iters, flags);
  return last_error();
}

int lz4dev_sizes(const void* const* in, const size_t* in_bytes, size_t* sizes, int* status, size_t count, unsigned block,
                 hipStream_t stream)
{
  const unsigned waves = block / 64;
  hipLaunchKernelGGL(k_sizes, dim3((unsigned)((count + waves - 1) / waves)), dim3(block), 0, stream, in, in_bytes, sizes,
                     status, count);
  return last_error();
}

size_t lz4dev_shared_bytes(void)
{
  return dev::kDecompressSharedBytes;
}

size_t lz4dev_ring_bytes(void)
{
  return dev::kStagingRingBytes;
}

size_t lz4dev_max_chunk_bytes(void)
{
  return dev::kMaxChunkBytes;
}

/* what one wave of a workgroup of `block` threads can keep in LDS: output bytes / staged input bytes */
size_t lz4dev_lds_out_bytes(unsigned block)
{
  return kLdsOut / (block / 64);
}

size_t lz4dev_lds_in_bytes(unsigned block)
{
  return kLdsIn / (block / 64);
}

} // extern "C"
