/*
 * tests/device_api/lz4_device_compress_kernels.hip -- TEST ONLY: kernels that call the compressor of the device-side LZ4
 * API (include/nvcomp/device/lz4.hpp), behind extern "C" launchers that tests/test_lz4_device_compress.py drives through
 * ctypes. One source for both tiers: the MI355X (hipcc --offload-arch=gfx950 -shared -fPIC -I include) and the host
 * emulation (g++ -x c++ -Itests/emu -Iinclude ... -lnvcomp_emu).
 *
 * Every wave's `shared` area sits between 16 guard bytes on either side; a kernel that finds a guard changed sets
 * kBadGuard in *flags. An output in LDS is followed by 16 guard bytes of 0xA5 (kBadLdsGuard). Launch shapes: 64 or 256
 * threads; with fewer waves than chunks a wave loops over several chunks and reuses its area. `fill` says what the area
 * holds at a call: kLeftovers (what the wave's last chunk left there; the first chunk of a wave: whatever the launch
 * before left), kOnes (0xFF, written by the wave in front of every call) or kZeros.
 *
 * On the emulator `__shared__` arrays are ordinary statics and the running workgroup's dynamic area is what counts as LDS:
 * k_lds keeps its buffers there, so that the compressor's LDS path runs on both tiers.
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
constexpr size_t kEncSlot = dev::kCompressSharedBytes + 2 * kGuardBytes;

enum : uint32_t { kBadGuard = 1, kBadLdsGuard = 2 };
enum : uint32_t { kLeftovers = 0, kOnes = 1, kZeros = 2 };
constexpr size_t kTooLargeForLds = ~(size_t)0;

/* what one wave of a workgroup of WAVES waves keeps in LDS: a staged chunk, and a block with its guard */
template <unsigned WAVES>
struct Lds
{
  static constexpr size_t kIn = WAVES == 1 ? 65536 + 16 : 8192; /* chunk bytes */
  static constexpr size_t kInBuf = kIn + 16;                     /* + an alignment of up to 15 */
  static constexpr size_t kOutBuf = (dev::max_compressed_bytes(kIn) + 15 + 16 + 15) / 16 * 16;
  static constexpr size_t kTotal = WAVES * (kInBuf + kOutBuf + kEncSlot);
};
static_assert(Lds<1>::kTotal <= 160 * 1024 && Lds<4>::kTotal <= 160 * 1024, "a CU's LDS");

__device__ inline uint32_t guard_word(uint32_t i)
{
  return (0x9E3779B9u * (i + 1)) ^ 0xA5C3E1F7u;
}

/* lanes 0-3: the 16 bytes in front of the area, lanes 4-7: the 16 behind it */
__device__ inline uint32_t* guard_at(uint8_t* slot, uint32_t lane)
{
  return (uint32_t*)(lane < 4 ? slot : slot + kGuardBytes + dev::kCompressSharedBytes) + (lane & 3);
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

__device__ inline void fill_area(uint8_t* area, uint32_t lane, uint32_t fill)
{
  if (fill != kLeftovers) {
    const uint32_t v = fill == kOnes ? 0xFFFFFFFFu : 0u;
    for (size_t i = lane; i < dev::kCompressSharedBytes / 4; i += 64) {
      ((uint32_t*)area)[i] = v;
    }
  }
  dev::wave_sync();
}

/* global -> global; a wave takes chunks w, w + (waves in the grid), ... and reuses its area */
__global__ void __launch_bounds__(256) k_global(const void* const* in, const size_t* in_bytes, void* const* out, size_t* sizes,
                                                size_t count, uint32_t fill, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[4][kEncSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  uint8_t* slot = lds[w];
  set_guards(slot, lane);
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    fill_area(slot + kGuardBytes, lane, fill);
    const size_t got = dev::compress(in[c], in_bytes[c], out[c], slot + kGuardBytes);
    if (lane == 0) {
      sizes[c] = got;
    }
    check_guards(slot, lane, flags);
  }
}

/* The chunk staged in LDS by the wave itself (at byte in_align of its buffer), wave_sync(), compressed from there: into
 * global memory, or (out_lds) into LDS at byte out_align of the wave's buffer and then copied out, the whole bound. */
template <unsigned WAVES>
__global__ void __launch_bounds__(64 * WAVES) k_lds(const void* const* in, const size_t* in_bytes, void* const* out, size_t* sizes,
                                                    size_t count, uint32_t out_lds, uint32_t in_align, uint32_t out_align,
                                                    uint32_t fill, uint32_t* flags)
{
  using L = Lds<WAVES>;
#if defined(__HIPCC__)
  __shared__ __attribute__((aligned(16))) uint8_t lds_all[L::kTotal];
  uint8_t* base = lds_all;
#else
  uint8_t* base = emu::dynamic_lds();
#endif
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  uint8_t* ibuf = base + w * L::kInBuf;
  uint8_t* obuf = base + WAVES * L::kInBuf + w * L::kOutBuf;
  uint8_t* slot = base + WAVES * (L::kInBuf + L::kOutBuf) + w * kEncSlot;
  set_guards(slot, lane);
  for (size_t c = (size_t)blockIdx.x * WAVES + w; c < count; c += (size_t)gridDim.x * WAVES) {
    const size_t n = in_bytes[c];
    if (n > L::kIn) {
      if (lane == 0) {
        sizes[c] = kTooLargeForLds;
      }
      continue;
    }
    const size_t bound = dev::max_compressed_bytes(n);
    const uint8_t* src = (const uint8_t*)in[c];
    uint8_t* s = ibuf + in_align;
    for (size_t i = lane; i < n; i += 64) {
      s[i] = src[i];
    }
    uint8_t* o = out_lds ? obuf + out_align : (uint8_t*)out[c];
    if (out_lds) {
      for (size_t i = lane; i < bound + 16; i += 64) {
        o[i] = 0xA5;
      }
    }
    fill_area(slot + kGuardBytes, lane, fill); /* (ends in a wave_sync) */
    const size_t got = dev::compress(s, n, o, slot + kGuardBytes);
    dev::wave_sync();
    if (out_lds) {
      if (lane < 16 && o[bound + lane] != 0xA5) {
        atomicOr(flags, (uint32_t)kBadLdsGuard);
      }
      uint8_t* d = (uint8_t*)out[c];
      for (size_t i = lane; i < bound; i += 64) {
        d[i] = o[i];
      }
    }
    if (lane == 0) {
      sizes[c] = got;
    }
    check_guards(slot, lane, flags);
    dev::wave_sync(); /* the copy out before the next chunk's fill */
  }
}

/* One call with in_bytes above kMaxChunkBytes: the scratch area holds a pattern that must survive. */
__global__ void __launch_bounds__(64) k_too_large(const void* in, size_t in_bytes, void* out, size_t* size, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kEncSlot];
  const uint32_t lane = threadIdx.x & 63;
  set_guards(lds, lane);
  uint32_t* area = (uint32_t*)(lds + kGuardBytes);
  for (uint32_t i = lane; i < dev::kCompressSharedBytes / 4; i += 64) {
    area[i] = guard_word(i);
  }
  dev::wave_sync();
  const size_t got = dev::compress(in, in_bytes, out, area);
  dev::wave_sync();
  for (uint32_t i = lane; i < dev::kCompressSharedBytes / 4; i += 64) {
    if (area[i] != guard_word(i)) {
      atomicOr(flags, (uint32_t)kBadGuard);
    }
  }
  if (lane == 0) {
    *size = got;
  }
  check_guards(lds, lane, flags);
}

/* The way back through the device decoder, global -> global, one wave per chunk. */
__global__ void __launch_bounds__(256) k_decompress(const void* const* in, const size_t* in_bytes, void* const* out,
                                                    const size_t* caps, size_t* actual, int* status, size_t count)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[4][dev::kDecompressSharedBytes];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const size_t c = (size_t)blockIdx.x * 4 + w;
  if (c >= count) {
    return;
  }
  size_t got = 0xDEADBEEF;
  const nvcompStatus_t st = dev::decompress(in[c], in_bytes[c], out[c], caps[c], &got, lds[w]);
  if (lane == 0) {
    actual[c] = got;
    status[c] = (int)st;
  }
}

int last_error()
{
  return (int)hipGetLastError();
}

} // namespace

extern "C" {

int lz4cmp_global(const void* const* in, const size_t* in_bytes, void* const* out, size_t* sizes, size_t count, unsigned block,
                  unsigned grid, unsigned fill, uint32_t* flags, hipStream_t stream)
{
  if ((block != 64 && block != 256) || fill > kZeros) {
    return -1;
  }
  hipLaunchKernelGGL(k_global, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, sizes, count, (uint32_t)fill, flags);
  return last_error();
}

int lz4cmp_lds(const void* const* in, const size_t* in_bytes, void* const* out, size_t* sizes, size_t count, unsigned out_lds,
               unsigned in_align, unsigned out_align, unsigned block, unsigned grid, unsigned fill, uint32_t* flags,
               hipStream_t stream)
{
  if (in_align > 15 || out_align > 15 || fill > kZeros) {
    return -1;
  }
  if (block == 64) {
    hipLaunchKernelGGL(k_lds<1>, dim3(grid), dim3(64), 0, stream, in, in_bytes, out, sizes, count, (uint32_t)out_lds,
                       (uint32_t)in_align, (uint32_t)out_align, (uint32_t)fill, flags);
  } else if (block == 256) {
    hipLaunchKernelGGL(k_lds<4>, dim3(grid), dim3(256), 0, stream, in, in_bytes, out, sizes, count, (uint32_t)out_lds,
                       (uint32_t)in_align, (uint32_t)out_align, (uint32_t)fill, flags);
  } else {
    return -1;
  }
  return last_error();
}

int lz4cmp_too_large(const void* in, size_t in_bytes, void* out, size_t* size, uint32_t* flags, hipStream_t stream)
{
  hipLaunchKernelGGL(k_too_large, dim3(1), dim3(64), 0, stream, in, in_bytes, out, size, flags);
  return last_error();
}

int lz4cmp_decompress(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                      int* status, size_t count, hipStream_t stream)
{
  hipLaunchKernelGGL(k_decompress, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream, in, in_bytes, out, caps, actual,
                     status, count);
  return last_error();
}

size_t lz4cmp_shared_bytes(void)
{
  return dev::kCompressSharedBytes;
}

size_t lz4cmp_step_bytes(void)
{
  return dev::kCompressStepBytes;
}

size_t lz4cmp_max_chunk_bytes(void)
{
  return dev::kMaxChunkBytes;
}

size_t lz4cmp_max_compressed_bytes(size_t n)
{
  return dev::max_compressed_bytes(n);
}

/* the chunk one wave of a workgroup of `block` threads can stage in LDS */
size_t lz4cmp_lds_in_bytes(unsigned block)
{
  return block == 64 ? Lds<1>::kIn : Lds<4>::kIn;
}

} // extern "C"
