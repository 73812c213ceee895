/*
 * tests/device_api/snappy_device_kernels.hip -- TEST ONLY: kernels that call the device-side Snappy API
 * (include/nvcomp/device/snappy.hpp), behind extern "C" launchers that tests/test_snappy_device.py (snpdev_*) and
 * tests/test_snappy_device_compress.py (snpcmp_*) drive through ctypes. One source for both tiers: the MI355X
 * (hipcc --offload-arch=gfx950 -shared -fPIC -I include) and the host emulation (g++ -x c++ -Itests/emu -Iinclude ...
 * -lnvcomp_emu).
 *
 * Every wave's `shared` area sits between 16 guard bytes on either side; a kernel that finds a guard changed sets
 * kBadGuard in *flags. An output in LDS is followed by 16 guard bytes of 0xA5 (kBadLdsGuard). Launch shapes: 64 or 256
 * threads; with fewer waves than chunks a wave loops over several chunks and reuses its area. The compressor's `fill`
 * says what the area holds at a call: kLeftovers (what the wave's last chunk left there; the first chunk of a wave:
 * whatever the launch before left), kOnes (0xFF, written by the wave in front of every call) or kZeros.
 *
 * On the emulator `__shared__` arrays are ordinary statics and the running workgroup's dynamic area is what counts as LDS:
 * kc_lds keeps its buffers there, so that the compressor's LDS path runs on both tiers.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <nvcomp/device/snappy.hpp>

namespace dev = nvcomp::device::snappy;

#if defined(__HIP_DEVICE_COMPILE__)
#define WAVE_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define WAVE_UNIFORM(x) (x)
#endif

namespace {

constexpr unsigned kGuardBytes = 16;
constexpr size_t kDecSlot = dev::kDecompressSharedBytes + 2 * kGuardBytes;
constexpr size_t kEncSlot = dev::kCompressSharedBytes + 2 * kGuardBytes;
constexpr size_t kLdsOut = 74 * 1024; /* the output bytes a workgroup keeps in LDS, shared out among its waves */
constexpr size_t kLdsIn = 74 * 1024;  /* the same for staged input */

enum : uint32_t { kBadGuard = 1, kBadLdsGuard = 2 };
enum : uint32_t { kLeftovers = 0, kOnes = 1, kZeros = 2 };
enum : int { kTooLargeForLds = -2 };
constexpr size_t kSizeTooLargeForLds = ~(size_t)0;

/* what one wave of a workgroup of WAVES waves keeps in LDS to compress: a staged chunk, and a stream with its guard */
template <unsigned WAVES>
struct EncLds
{
  static constexpr size_t kIn = WAVES == 1 ? 65536 + 16 : 8192; /* chunk bytes */
  static constexpr size_t kInBuf = kIn + 16;                     /* + an alignment of up to 15 */
  static constexpr size_t kOutBuf = (dev::max_compressed_bytes(kIn) + 15 + 16 + 15) / 16 * 16;
  static constexpr size_t kTotal = WAVES * (kInBuf + kOutBuf + kEncSlot);
};
static_assert(EncLds<1>::kTotal <= 160 * 1024 && EncLds<4>::kTotal <= 160 * 1024, "a CU's LDS");
static_assert(kLdsOut + kLdsIn + 4 * (48 + 16 + kDecSlot) <= 160 * 1024, "a CU's LDS");

__device__ inline uint32_t guard_word(uint32_t i)
{
  return (0x9E3779B9u * (i + 1)) ^ 0xA5C3E1F7u;
}

/* lanes 0-3: the 16 bytes in front of an area of `area` bytes, lanes 4-7: the 16 behind it */
__device__ inline uint32_t* guard_at(uint8_t* slot, uint32_t lane, size_t area)
{
  return (uint32_t*)(lane < 4 ? slot : slot + kGuardBytes + area) + (lane & 3);
}

__device__ inline void set_guards(uint8_t* slot, uint32_t lane, size_t area)
{
  if (lane < 8) {
    *guard_at(slot, lane, area) = guard_word(lane);
  }
}

__device__ inline void check_guards(uint8_t* slot, uint32_t lane, size_t area, uint32_t* flags)
{
  if (lane < 8 && *guard_at(slot, lane, area) != guard_word(lane)) {
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

/* ---- the decoder ---- */

/* global -> global; a wave takes chunks w, w + (waves in the grid), ... and reuses its area */
__global__ void __launch_bounds__(256) kd_global(const void* const* in, const size_t* in_bytes, void* const* out,
                                                 const size_t* caps, size_t* actual, int* status, size_t count, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[4][kDecSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  uint8_t* slot = lds[w];
  set_guards(slot, lane, dev::kDecompressSharedBytes);
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    size_t got = 0xDEADBEEF;
    const nvcompStatus_t st = dev::decompress(in[c], in_bytes[c], out[c], caps[c], &got, slot + kGuardBytes);
    if (lane == 0) {
      actual[c] = got;
      status[c] = (int)st;
    }
    check_guards(slot, lane, dev::kDecompressSharedBytes, flags);
  }
}

/* The output in LDS (at byte out_align of the wave's buffer), then copied out, all `cap` bytes of it. stage_in: the
 * stream is first staged in LDS by the wave itself (at byte in_align), wave_sync(), and decoded from there. */
template <unsigned WAVES>
__global__ void __launch_bounds__(64 * WAVES) kd_lds(const void* const* in, const size_t* in_bytes, void* const* out,
                                                     const size_t* caps, size_t* actual, int* status, size_t count,
                                                     uint32_t stage_in, uint32_t in_align, uint32_t out_align, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t obuf[WAVES][kLdsOut / WAVES + 48];
  __shared__ __attribute__((aligned(16))) uint8_t ibuf[WAVES][kLdsIn / WAVES + 16];
  __shared__ __attribute__((aligned(16))) uint8_t lds[WAVES][kDecSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  uint8_t* slot = lds[w];
  set_guards(slot, lane, dev::kDecompressSharedBytes);
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
    check_guards(slot, lane, dev::kDecompressSharedBytes, flags);
    dev::wave_sync(); /* the copy out before the next chunk's fill */
  }
}

/* Waves 0 and 1 of every workgroup decode a chunk each, wave 2 compresses one (all global -> global); wave 3 does not
 * call at all: a xorshift chain of `iters` steps per lane into side[]. */
__global__ void __launch_bounds__(256) k_mixed(const void* const* in, const size_t* in_bytes, void* const* out,
                                               const size_t* caps, size_t* actual, int* status, size_t count,
                                               const void* const* raw, const size_t* raw_bytes, void* const* comp,
                                               size_t* comp_sizes, size_t raw_count, uint32_t* side, uint32_t iters,
                                               uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t dec[2][kDecSlot];
  __shared__ __attribute__((aligned(16))) uint8_t enc[kEncSlot];
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
  if (w == 2) {
    const size_t job = blockIdx.x;
    if (job >= raw_count) {
      return;
    }
    set_guards(enc, lane, dev::kCompressSharedBytes);
    const size_t got = dev::compress(raw[job], raw_bytes[job], comp[job], enc + kGuardBytes);
    if (lane == 0) {
      comp_sizes[job] = got;
    }
    check_guards(enc, lane, dev::kCompressSharedBytes, flags);
    return;
  }
  const size_t job = (size_t)blockIdx.x * 2 + w;
  if (job >= count) {
    return;
  }
  uint8_t* slot = dec[w];
  set_guards(slot, lane, dev::kDecompressSharedBytes);
  size_t got = 0xDEADBEEF;
  const nvcompStatus_t st = dev::decompress(in[job], in_bytes[job], out[job], caps[job], &got, slot + kGuardBytes);
  if (lane == 0) {
    actual[job] = got;
    status[job] = (int)st;
  }
  check_guards(slot, lane, dev::kDecompressSharedBytes, flags);
}

/* decompressed_size(), one wave per chunk */
__global__ void __launch_bounds__(256) kd_sizes(const void* const* in, const size_t* in_bytes, size_t* sizes, int* status,
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

/* ---- the compressor ---- */

/* global -> global; a wave takes chunks w, w + (waves in the grid), ... and reuses its area */
__global__ void __launch_bounds__(256) kc_global(const void* const* in, const size_t* in_bytes, void* const* out, size_t* sizes,
                                                 size_t count, uint32_t fill, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[4][kEncSlot];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t w = WAVE_UNIFORM(threadIdx.x >> 6);
  const uint32_t waves = blockDim.x >> 6;
  uint8_t* slot = lds[w];
  set_guards(slot, lane, dev::kCompressSharedBytes);
  for (size_t c = (size_t)blockIdx.x * waves + w; c < count; c += (size_t)gridDim.x * waves) {
    fill_area(slot + kGuardBytes, lane, fill);
    const size_t got = dev::compress(in[c], in_bytes[c], out[c], slot + kGuardBytes);
    if (lane == 0) {
      sizes[c] = got;
    }
    check_guards(slot, lane, dev::kCompressSharedBytes, flags);
  }
}

/* The chunk staged in LDS by the wave itself (at byte in_align of its buffer), wave_sync(), compressed from there: into
 * global memory, or (out_lds) into LDS at byte out_align of the wave's buffer and then copied out, the whole bound. */
template <unsigned WAVES>
__global__ void __launch_bounds__(64 * WAVES) kc_lds(const void* const* in, const size_t* in_bytes, void* const* out, size_t* sizes,
                                                     size_t count, uint32_t out_lds, uint32_t in_align, uint32_t out_align,
                                                     uint32_t fill, uint32_t* flags)
{
  using L = EncLds<WAVES>;
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
  set_guards(slot, lane, dev::kCompressSharedBytes);
  for (size_t c = (size_t)blockIdx.x * WAVES + w; c < count; c += (size_t)gridDim.x * WAVES) {
    const size_t n = in_bytes[c];
    if (n > L::kIn) {
      if (lane == 0) {
        sizes[c] = kSizeTooLargeForLds;
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
    check_guards(slot, lane, dev::kCompressSharedBytes, flags);
    dev::wave_sync(); /* the copy out before the next chunk's fill */
  }
}

/* One call with in_bytes above kMaxChunkBytes: the scratch area holds a pattern that must survive. */
__global__ void __launch_bounds__(64) kc_too_large(const void* in, size_t in_bytes, void* out, size_t* size, uint32_t* flags)
{
  __shared__ __attribute__((aligned(16))) uint8_t lds[kEncSlot];
  const uint32_t lane = threadIdx.x & 63;
  set_guards(lds, lane, dev::kCompressSharedBytes);
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
  check_guards(lds, lane, dev::kCompressSharedBytes, flags);
}

int last_error()
{
  return (int)hipGetLastError();
}

} // namespace

extern "C" {

int snpdev_global(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                  int* status, size_t count, unsigned block, unsigned grid, uint32_t* flags, hipStream_t stream)
{
  if (block != 64 && block != 256) {
    return -1;
  }
  hipLaunchKernelGGL(kd_global, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, caps, actual, status, count, flags);
  return last_error();
}

int snpdev_lds(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
               int* status, size_t count, unsigned stage_in, unsigned in_align, unsigned out_align, unsigned block,
               unsigned grid, uint32_t* flags, hipStream_t stream)
{
  if (in_align > 15 || out_align > 15) {
    return -1;
  }
  if (block == 64) {
    hipLaunchKernelGGL(kd_lds<1>, dim3(grid), dim3(64), 0, stream, in, in_bytes, out, caps, actual, status, count,
                       (uint32_t)stage_in, (uint32_t)in_align, (uint32_t)out_align, flags);
  } else if (block == 256) {
    hipLaunchKernelGGL(kd_lds<4>, dim3(grid), dim3(256), 0, stream, in, in_bytes, out, caps, actual, status, count,
                       (uint32_t)stage_in, (uint32_t)in_align, (uint32_t)out_align, flags);
  } else {
    return -1;
  }
  return last_error();
}

int snpdev_mixed(const void* const* in, const size_t* in_bytes, void* const* out, const size_t* caps, size_t* actual,
                 int* status, size_t count, const void* const* raw, const size_t* raw_bytes, void* const* comp,
                 size_t* comp_sizes, size_t raw_count, uint32_t* side, unsigned iters, unsigned grid, uint32_t* flags,
                 hipStream_t stream)
{
  hipLaunchKernelGGL(k_mixed, dim3(grid), dim3(256), 0, stream, in, in_bytes, out, caps, actual, status, count, raw,
                     raw_bytes, comp, comp_sizes, raw_count, side, (uint32_t)iters, flags);
  return last_error();
}

int snpdev_sizes(const void* const* in, const size_t* in_bytes, size_t* sizes, int* status, size_t count, unsigned block,
                 hipStream_t stream)
{
  const unsigned waves = block / 64;
  hipLaunchKernelGGL(kd_sizes, dim3((unsigned)((count + waves - 1) / waves)), dim3(block), 0, stream, in, in_bytes, sizes,
                     status, count);
  return last_error();
}

size_t snpdev_shared_bytes(void)
{
  return dev::kDecompressSharedBytes;
}

size_t snpdev_ring_bytes(void)
{
  return dev::kStagingRingBytes;
}

size_t snpdev_max_chunk_bytes(void)
{
  return dev::kMaxChunkBytes;
}

/* what one wave of a workgroup of `block` threads can keep in LDS: output bytes / staged input bytes */
size_t snpdev_lds_out_bytes(unsigned block)
{
  return kLdsOut / (block / 64);
}

size_t snpdev_lds_in_bytes(unsigned block)
{
  return kLdsIn / (block / 64);
}

int snpcmp_global(const void* const* in, const size_t* in_bytes, void* const* out, size_t* sizes, size_t count, unsigned block,
                  unsigned grid, unsigned fill, uint32_t* flags, hipStream_t stream)
{
  if ((block != 64 && block != 256) || fill > kZeros) {
    return -1;
  }
  hipLaunchKernelGGL(kc_global, dim3(grid), dim3(block), 0, stream, in, in_bytes, out, sizes, count, (uint32_t)fill, flags);
  return last_error();
}

int snpcmp_lds(const void* const* in, const size_t* in_bytes, void* const* out, size_t* sizes, size_t count, unsigned out_lds,
               unsigned in_align, unsigned out_align, unsigned block, unsigned grid, unsigned fill, uint32_t* flags,
               hipStream_t stream)
{
  if (in_align > 15 || out_align > 15 || fill > kZeros) {
    return -1;
  }
  if (block == 64) {
    hipLaunchKernelGGL(kc_lds<1>, dim3(grid), dim3(64), 0, stream, in, in_bytes, out, sizes, count, (uint32_t)out_lds,
                       (uint32_t)in_align, (uint32_t)out_align, (uint32_t)fill, flags);
  } else if (block == 256) {
    hipLaunchKernelGGL(kc_lds<4>, dim3(grid), dim3(256), 0, stream, in, in_bytes, out, sizes, count, (uint32_t)out_lds,
                       (uint32_t)in_align, (uint32_t)out_align, (uint32_t)fill, flags);
  } else {
    return -1;
  }
  return last_error();
}

int snpcmp_too_large(const void* in, size_t in_bytes, void* out, size_t* size, uint32_t* flags, hipStream_t stream)
{
  hipLaunchKernelGGL(kc_too_large, dim3(1), dim3(64), 0, stream, in, in_bytes, out, size, flags);
  return last_error();
}

size_t snpcmp_shared_bytes(void)
{
  return dev::kCompressSharedBytes;
}

size_t snpcmp_step_bytes(void)
{
  return dev::kCompressStepBytes;
}

size_t snpcmp_max_compressed_bytes(size_t n)
{
  return dev::max_compressed_bytes(n);
}

/* the chunk one wave of a workgroup of `block` threads can stage in LDS to compress */
size_t snpcmp_lds_in_bytes(unsigned block)
{
  return block == 64 ? EncLds<1>::kIn : EncLds<4>::kIn;
}

} // extern "C"
