/*
 * tests/wave/wave_ops_kernels.hip -- TEST INFRASTRUCTURE ONLY.
 *
 * One kernel per family of wave64 primitives, behind extern "C" launchers that tests/test_wave_primitives.py drives
 * through ctypes and compares, lane by lane, with the lane model of tests/wave_model.py. The file is compiled four times:
 * for gfx950 (hipcc) and for the host emulation (g++ -Itests/emu), each once against the library's header
 * (common/wave.h, namespace wave) and once, with -DWAVE_OPS_DEVICE_HEADERS, against the device API's copies
 * (nvcomp/device/detail/wave*.hpp, namespace nvcomp::device::detail::wave). The second build holds only what those
 * headers define.
 *
 * One wave (a block of 64 lanes) per case, blockIdx.x the case. A case's input row is kInWords words: four operands
 * of 64 lanes (a, b, c, d), then eight wave-uniform words u[0..7]. Its output row is eight results of 64 lanes. Every
 * primitive is called from wave-uniform control flow with all 64 lanes active; the branches below are on uniform words.
 * The inputs are checked by the model before a launch: nothing here guards a primitive's preconditions.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#if defined(WAVE_OPS_DEVICE_HEADERS)
#include <nvcomp/device/detail/wave.hpp>
#include <nvcomp/device/detail/wave_ext.hpp>
#include <nvcomp/device/detail/wave_lz.hpp>
#include <nvcomp/device/detail/wave_lzc.hpp>
namespace W = nvcomp::device::detail::wave;
#define WAVE_OPS_LIBRARY 0
#else
#include "common/lz_common.hip.h"
#include "common/wave.h"
namespace W = wave;
#define WAVE_OPS_LIBRARY 1
#endif

namespace {

constexpr uint32_t kInWords = 4 * 64 + 8;
constexpr uint32_t kOutWords = 8 * 64;

struct Case
{
  const uint32_t* in;
  uint32_t* out;
  uint32_t lane;
  uint32_t a, b, c, d;

  __device__ uint32_t u(uint32_t i) const { return W::uniform(in[256 + i]); }
  __device__ void put(uint32_t row, uint32_t v) const { out[row * 64 + lane] = v; }
};

__device__ __forceinline__ Case open_case(const uint32_t* in, uint32_t* out)
{
  Case k;
  k.in = in + (size_t)blockIdx.x * kInWords;
  k.out = out + (size_t)blockIdx.x * kOutWords;
  k.lane = threadIdx.x & 63;
  k.a = k.in[k.lane];
  k.b = k.in[64 + k.lane];
  k.c = k.in[128 + k.lane];
  k.d = k.in[192 + k.lane];
  return k;
}

/* scans and reductions of a; umax(a, b). touch() and sched_fence() have no value of their own: the results behind them
 * must still be right. */
__global__ void __launch_bounds__(64) k_scan(const uint32_t* in, uint32_t* out)
{
  const Case k = open_case(in, out);
  uint32_t v = k.a;
  W::touch(v);
  k.put(0, W::scan_add_inclusive(v));
  W::sched_fence();
  k.put(1, W::reduce_add(v));
  k.put(2, W::reduce_max(v));
  k.put(3, W::umax(v, k.b));
#if WAVE_OPS_LIBRARY
  k.put(4, W::scan_max_inclusive(v));
  uint32_t val = k.c, mask = k.d;
  W::scan_last_writer(val, mask);
  k.put(5, val);
  k.put(6, mask);
#endif
}

/* moves: shuffle(a, b), prev_lane(a), next_lane(a), permute_to(a, c) */
__global__ void __launch_bounds__(64) k_move(const uint32_t* in, uint32_t* out)
{
  const Case k = open_case(in, out);
  k.put(0, W::shuffle(k.a, k.b));
  k.put(1, W::prev_lane(k.a));
#if WAVE_OPS_LIBRARY
  k.put(2, W::next_lane(k.a));
  k.put(3, W::permute_to(k.a, k.c));
#endif
}

/* read_lane(a, u0); write_lane(a, u1, u2); write_lane_scalar twice in a row (u1 -> lane u2, then u3 -> lane u4);
 * uniform(b) of a b that is the same in every lane; uniform64(d:c) likewise; a load through uniform_ptr. */
__global__ void __launch_bounds__(64) k_lane(const uint32_t* in, uint32_t* out)
{
  const Case k = open_case(in, out);
  k.put(0, W::read_lane(k.a, k.u(0)));
  k.put(1, W::write_lane(k.a, k.u(1), k.u(2)));
  k.put(2, W::uniform(k.b));
#if WAVE_OPS_LIBRARY
  uint32_t v = W::write_lane_scalar(k.a, k.u(1), k.u(2));
  v = W::write_lane_scalar(v, k.u(3), k.u(4));
  k.put(3, v);
  const uint64_t q = W::uniform64(((uint64_t)k.d << 32) | k.c);
  k.put(4, (uint32_t)q);
  k.put(5, (uint32_t)(q >> 32));
  const uint32_t* p = W::uniform_ptr(k.in);
  k.put(6, p[k.lane] + p[256 + 5]); /* a[lane] + u5 */
#endif
}

/* the 64-bit mask u1:u0: ballot of (a != 0), prefix_popc, popc64, ctz64 (of a mask that is not 0), lane_in */
__global__ void __launch_bounds__(64) k_mask(const uint32_t* in, uint32_t* out)
{
  const Case k = open_case(in, out);
  const uint64_t m = ((uint64_t)k.u(1) << 32) | k.u(0);
  const uint64_t b = W::ballot(k.a != 0);
  k.put(0, (uint32_t)b);
  k.put(1, (uint32_t)(b >> 32));
  k.put(2, W::prefix_popc(m));
  k.put(3, W::popc64(m));
  k.put(4, m != 0 ? W::ctz64(m) : 0xffffffffu);
#if WAVE_OPS_LIBRARY
  k.put(5, W::lane_in(m) ? 1u : 0u);
#endif
}

/* per-lane arithmetic, the operation chosen by u0 */
__global__ void __launch_bounds__(64) k_arith(const uint32_t* in, uint32_t* out)
{
  const Case k = open_case(in, out);
  const uint32_t op = k.u(0);
  uint32_t r = 0;
  if (op == 0) {
    r = W::mul24(k.a, k.b);
  }
#if WAVE_OPS_LIBRARY
  else if (op == 1) {
    r = W::align_bits(k.a, k.b, k.c);
  } else if (op == 2) {
    r = W::align_bytes(k.a, k.b, k.c);
  } else if (op == 3) {
    r = W::pk_add_sat255(k.a, k.b);
  } else if (op == 4) {
    r = W::bit_reverse(k.a);
  } else if (op == 5) {
    r = W::perm_bytes(k.a, k.b, k.c);
  }
#endif
  k.put(0, r);
}

/* lane_id() and fresh_lane_id() in both waves of a block of 128; sync() between a store and a cross-lane load of it.
 * Library build: wave 0 hands 64 words to wave 1 behind a flag, once with the release / acquire pair and nap(), once with
 * the relaxed pair between sync() calls and nap_short(). The polls are bounded: a consumer that never sees the flag
 * writes kGaveUp and goes on. */
constexpr uint32_t kGaveUp = 0xdead0000u;
constexpr uint32_t kPollLimit = 1u << 20;

__global__ void __launch_bounds__(128) k_two_waves(const uint32_t* in, uint32_t* out)
{
  const Case k = open_case(in, out);
  __shared__ uint32_t data[3][64];
  __shared__ uint32_t flag[2];
  const uint32_t w = W::uniform(threadIdx.x >> 6);
  if (threadIdx.x < 2) {
    flag[threadIdx.x] = 0;
  }
  __syncthreads();
  k.put(w ? 2 : 0, (uint32_t)W::lane_id());
  k.put(w ? 3 : 1, (uint32_t)W::fresh_lane_id());
  if (w == 0) {
    data[2][k.lane] = k.c;
    W::sync();
    k.put(4, data[2][63 - k.lane]);
  }
#if WAVE_OPS_LIBRARY
  if (w == 0) {
    data[0][k.lane] = k.a;
    W::sync();
    if (k.lane == 0) {
      W::lds_store_release(&flag[0], 1u);
    }
    data[1][k.lane] = k.b;
    W::sync();
    if (k.lane == 0) {
      W::lds_store_relaxed(&flag[1], 1u);
    }
    W::sync();
  } else {
    uint32_t seen = 0;
    for (uint32_t i = 0; i < kPollLimit && !seen; ++i) {
      seen = W::read_lane(W::lds_load_acquire(&flag[0]), 0);
      if (!seen) {
        W::nap();
      }
    }
    k.put(5, seen ? data[0][63 - k.lane] : kGaveUp);
    seen = 0;
    for (uint32_t i = 0; i < kPollLimit && !seen; ++i) {
      W::sync();
      seen = W::read_lane(W::lds_load_relaxed(&flag[1]), 0);
      W::sync();
      if (!seen) {
        W::nap_short();
      }
    }
    k.put(6, seen ? data[1][63 - k.lane] : kGaveUp);
  }
#endif
}

#if WAVE_OPS_LIBRARY

/* chain_walk(step = a, limit = u0, r = u1, k = u2, rec = b) */
__global__ void __launch_bounds__(64) k_chain_walk(const uint32_t* in, uint32_t* out)
{
  const Case k = open_case(in, out);
  uint32_t r = k.u(1), n = k.u(2), rec = k.b;
  W::chain_walk(k.a, k.u(0), r, n, rec);
  k.put(0, rec);
  k.put(1, r);
  k.put(2, n);
}

/* select_walk(candidates = u1:u0, len = a, start = u2) */
__global__ void __launch_bounds__(64) k_select_walk(const uint32_t* in, uint32_t* out)
{
  const Case k = open_case(in, out);
  const uint64_t cand = ((uint64_t)k.u(1) << 32) | k.u(0);
  uint64_t taken;
  uint32_t end;
  W::select_walk(cand, k.a, k.u(2), taken, end);
  k.put(0, (uint32_t)taken);
  k.put(1, (uint32_t)(taken >> 32));
  k.put(2, end);
}

/* LDS words start as c; every lane applies b to word a (< 64) with the operation u0 */
__global__ void __launch_bounds__(64) k_lds_atomic(const uint32_t* in, uint32_t* out)
{
  const Case k = open_case(in, out);
  __shared__ uint32_t words[64];
  words[k.lane] = k.c;
  W::sync();
  const uint32_t op = k.u(0);
  if (op == 0) {
    W::lds_or(&words[k.a], k.b);
  } else if (op == 1) {
    W::lds_add(&words[k.a], k.b);
  } else {
    W::lds_sub(&words[k.a], k.b);
  }
  W::sync_wave();
  k.put(0, words[k.lane]);
}

/* kernel_args: a kernel whose only parameter is a struct; every field read through the returned pointer */
struct ArgBlock
{
  uint8_t f8;
  uint16_t f16;
  uint32_t f32;
  uint64_t f64;
  uint32_t* out;
};

__global__ void __launch_bounds__(64) k_kernel_args(ArgBlock args)
{
  const auto* p = W::kernel_args(args);
  uint32_t* out = p->out;
  const uint32_t lane = threadIdx.x & 63;
  out[0 * 64 + lane] = p->f8;
  out[1 * 64 + lane] = p->f16;
  out[2 * 64 + lane] = p->f32;
  out[3 * 64 + lane] = (uint32_t)p->f64;
  out[4 * 64 + lane] = (uint32_t)(p->f64 >> 32);
}

/* The unaligned accessors, the operation chosen by u0 at byte offset u1. Loads: lane l reads at src + 16 * l + u1.
 * Stores: lane l writes (a, b, c, d) at its own slot of kSlot bytes, kGuard bytes in. */
constexpr uint32_t kSlot = 64, kGuard = 16;

__global__ void __launch_bounds__(64) k_access(const uint32_t* in, uint32_t* out, const uint8_t* src, uint8_t* dst)
{
  const Case k = open_case(in, out);
  const uint32_t op = k.u(0), off = k.u(1);
  const uint8_t* s = src + 16 * k.lane + off;
  uint8_t* d = dst + ((size_t)blockIdx.x * 64 + k.lane) * kSlot + kGuard + off;
  W::u32x4 q;
  q.x = k.a, q.y = k.b, q.z = k.c, q.w = k.d;
  if (op == 0) {
    k.put(0, W::gload_u8(s));
  } else if (op == 1) {
    k.put(0, W::gload_u16((const uint16_t*)s));
  } else if (op == 2) {
    k.put(0, W::gload_u32(s));
  } else if (op == 3) {
    const uint64_t v = W::gload_u64(s);
    k.put(0, (uint32_t)v);
    k.put(1, (uint32_t)(v >> 32));
  } else if (op == 4) {
    const W::u32x3 v = W::gload_u32x3(s);
    k.put(0, v.x);
    k.put(1, v.y);
    k.put(2, v.z);
  } else if (op == 5 || op == 6) {
    const W::u32x4 v = op == 5 ? W::gload_u32x4(s) : W::gload_u32x4_aligned(s);
    k.put(0, v.x);
    k.put(1, v.y);
    k.put(2, v.z);
    k.put(3, v.w);
  } else if (op == 7) {
    W::gstore_u8(d, k.a);
  } else if (op == 8) {
    W::gstore_u32(d, k.a);
  } else if (op == 9) {
    W::gstore_u32x4(d, q);
  } else if (op == 10) {
    W::gstore_u32x4_aligned(d, q);
  } else if (op == 11) {
    W::gstore_u32x4_aligned_nt(d, q);
  }
}

/* common/lz_common.hip.h. u0 = 0: wave_copy of u1 bytes. u0 = 1: lane l moves 4 bytes with ld_u32 / st_u32 from s + 4 l
 * to d + 8 l. u0 = 2: lane l moves 16 bytes with copy16 from s + 16 l to d + 32 l. s = src + u2, d = this case's region
 * of dst (kRegion bytes) + kGuard + u3. */
constexpr uint32_t kRegion = 2112;

__global__ void __launch_bounds__(64) k_lz_copy(const uint32_t* in, uint32_t* out, const uint8_t* src, uint8_t* dst)
{
  const Case k = open_case(in, out);
  const uint32_t op = k.u(0), len = k.u(1);
  const uint8_t* s = src + k.u(2);
  uint8_t* d = dst + (size_t)blockIdx.x * kRegion + kGuard + k.u(3);
  if (op == 0) {
    lz::wave_copy(d, s, len);
  } else if (op == 1) {
    lz::st_u32(d + 8 * k.lane, lz::ld_u32(s + 4 * k.lane));
  } else {
    lz::copy16(d + 32 * k.lane, s + 16 * k.lane);
  }
}

#else /* device headers */

/* is_lds: a pointer into the block's dynamic LDS area, and one into global memory */
__global__ void __launch_bounds__(64) k_is_lds(const uint32_t* in, uint32_t* out)
{
  const Case k = open_case(in, out);
#if defined(__HIPCC__)
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
#else
  uint8_t* lds = emu::dynamic_lds();
#endif
  k.put(0, W::is_lds(lds + 4 * k.lane) ? 1u : 0u);
  k.put(1, W::is_lds(k.in + k.lane) ? 1u : 0u);
  k.put(2, W::is_lds(k.out) ? 1u : 0u);
}

#endif

int launched()
{
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

} // namespace

extern "C" {

#define WAVE_OPS_LAUNCHER(name, kernel, threads)                                                   \
  int name(const uint32_t* in, uint32_t* out, unsigned n_cases, hipStream_t stream)              \
  {                                                                                                \
    (void)hipGetLastError();                                                                       \
    hipLaunchKernelGGL(kernel, dim3(n_cases), dim3(threads), 0, stream, in, out);                  \
    return launched();                                                                             \
  }

WAVE_OPS_LAUNCHER(waveops_scan, k_scan, 64)
WAVE_OPS_LAUNCHER(waveops_move, k_move, 64)
WAVE_OPS_LAUNCHER(waveops_lane, k_lane, 64)
WAVE_OPS_LAUNCHER(waveops_mask, k_mask, 64)
WAVE_OPS_LAUNCHER(waveops_arith, k_arith, 64)
WAVE_OPS_LAUNCHER(waveops_two_waves, k_two_waves, 128)

#if WAVE_OPS_LIBRARY
WAVE_OPS_LAUNCHER(waveops_chain_walk, k_chain_walk, 64)
WAVE_OPS_LAUNCHER(waveops_select_walk, k_select_walk, 64)
WAVE_OPS_LAUNCHER(waveops_lds_atomic, k_lds_atomic, 64)

int waveops_kernel_args(unsigned f8, unsigned f16, uint32_t f32, uint64_t f64, uint32_t* out, hipStream_t stream)
{
  ArgBlock args;
  args.f8 = (uint8_t)f8, args.f16 = (uint16_t)f16, args.f32 = f32, args.f64 = f64, args.out = out;
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_kernel_args, dim3(1), dim3(64), 0, stream, args);
  return launched();
}

int waveops_access(const uint32_t* in, uint32_t* out, const uint8_t* src, uint8_t* dst, unsigned n_cases, hipStream_t stream)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_access, dim3(n_cases), dim3(64), 0, stream, in, out, src, dst);
  return launched();
}

int waveops_lz_copy(const uint32_t* in, uint32_t* out, const uint8_t* src, uint8_t* dst, unsigned n_cases, hipStream_t stream)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_lz_copy, dim3(n_cases), dim3(64), 0, stream, in, out, src, dst);
  return launched();
}
#else
int waveops_is_lds(const uint32_t* in, uint32_t* out, unsigned n_cases, hipStream_t stream)
{
  (void)hipGetLastError();
  hipLaunchKernelGGL(k_is_lds, dim3(n_cases), dim3(64), 256, stream, in, out);
  return launched();
}
#endif

} // extern "C"
