/*
 * api/crc32_api.hip -- C ABI of the batched standard CRC-32 (include/nvcomp/crc32.h) and the kernel it launches. Host
 * side does the argument checks, at most one memset of the outputs and one launch on the caller's stream; nothing here
 * allocates or synchronises.
 *
 * The host knows the batch size, not the chunk sizes, so the work is split by batch size alone: every chunk gets
 * T = ceil(W / num_chunks) waves (at least 1, at most W), where W is the waves the card keeps resident. Wave j of a chunk
 * of n bytes takes the segment [j S, min((j + 1) S, n)) with S = max(round_up(ceil(n / T), kTile), kMinSegment); waves
 * whose segment is empty return at once.
 *   - T = 1: the wave walks the whole chunk (hlif/crc32.hip.h) and stores the finished CRC, as the managers' crc_kernel.
 *   - T > 1: each wave takes the raw remainder of its segment (from 0xffffffff for segment 0, from 0 for the others),
 *     multiplies it by x^(8 * bytes after the segment) mod P and XORs it into the output, which a memset zeroed in front
 *     of the launch; the wave of segment 0 also XORs in the final complement. The remainder is linear in the message,
 *     so the XOR of the parts is the chunk's CRC whatever order the waves finish in.
 */
#include <hip/hip_runtime.h>

#include "nvcomp/crc32.h"

#include "common/api_batch.hip.h"
#include "common/log.h"
#include "common/wave.h"

#include "hlif/crc32.hip.h"

namespace {

constexpr unsigned kWavesPerGroup = 4;            /* as crc_kernel: the 8 KiB of tables serve four waves */
constexpr uint32_t kTile = 64 * crc32w::kSegDefault;
constexpr uint64_t kMinSegment = 64u << 10;       /* a segment streams at least this many bytes */
constexpr size_t kDefaultWaves = 256 * 32;        /* W when the runtime cannot tell: 256 CUs x 32 waves */
constexpr size_t kMaxGroups = 1u << 16;           /* larger batches loop over their waves */

/* XOR v into *p. On the card this is one hardware atomic: the waves of a chunk finish at about the same time, and a
 * compare-and-swap loop on one word is quadratic in them (measured: one 1 GiB chunk, 8 192 waves, 11 GB/s). The CPU
 * emulation of the runtime has no atomicXor and runs one wave at a time, so there a compare-and-swap loop does it. */
__device__ __forceinline__ void atomic_xor(uint32_t* p, uint32_t v)
{
#if defined(__HIPCC__)
  atomicXor(p, v);
#else
  uint32_t old = 0;
  for (;;) {
    const uint32_t seen = atomicCAS(p, old, old ^ v);
    if (seen == old) {
      return;
    }
    old = seen;
  }
#endif
}

__global__ void __launch_bounds__(64 * kWavesPerGroup) crc32_kernel(
    const void* const* __restrict__ ptrs, const size_t* __restrict__ sizes, size_t num_chunks, uint32_t* out,
    uint32_t waves_per_chunk)
{
  __shared__ uint32_t tables[crc32w::kLdsDwords];
  crc32w::load_tables(tables);
  __syncthreads();
  const size_t total = num_chunks * waves_per_chunk;
  const size_t stride = (size_t)gridDim.x * kWavesPerGroup;
  for (size_t g = (size_t)blockIdx.x * kWavesPerGroup + wave::uniform(threadIdx.x >> 6); g < total; g += stride) {
    if (waves_per_chunk == 1) {
      const uint8_t* p = wave::uniform_ptr((const uint8_t*)ptrs[g]);
      const uint64_t n = wave::uniform64(sizes[g]);
      const uint32_t c = crc32w::wave_crc32_raw_long(p, n, 0xffffffffu, tables) ^ 0xffffffffu;
      if (wave::lane_id() == 0) {
        out[g] = c;
      }
      continue;
    }
    const size_t i = g / waves_per_chunk;
    const uint32_t j = (uint32_t)(g - i * waves_per_chunk);
    const uint64_t n = wave::uniform64(sizes[i]);
    /* S = max(round_up(ceil(n / T), kTile), kMinSegment); n / T < 2^63, so nothing overflows */
    uint64_t seg = n / waves_per_chunk + (n % waves_per_chunk != 0);
    seg = (seg + kTile - 1) / kTile * kTile;
    seg = seg > kMinSegment ? seg : kMinSegment;
    const uint64_t segments = n / seg + (n % seg != 0);
    if (j >= segments) {
      continue; /* (n = 0: the memset already holds the CRC of nothing, 0) */
    }
    const uint64_t lo = (uint64_t)j * seg;
    const uint64_t len = n - lo < seg ? n - lo : seg;
    const uint8_t* p = wave::uniform_ptr((const uint8_t*)ptrs[i]);
    uint32_t r = crc32w::wave_crc32_raw_long(p + lo, len, j == 0 ? 0xffffffffu : 0u, tables);
    r = crc32w::append_zeros(r, n - lo - len);
    if (j == 0) {
      r ^= 0xffffffffu;
    }
    if (wave::lane_id() == 0) {
      atomic_xor(&out[i], r);
    }
  }
}

} // namespace

extern "C" {

nvcompStatus_t nvcompBatchedCRC32Async(
    const void* const* device_uncompressed_chunk_ptrs,
    const size_t* device_uncompressed_chunk_bytes,
    size_t num_chunks,
    uint32_t* device_crc32_ptr,
    hipStream_t stream)
{
  nvlog::call(3, "nvcompBatchedCRC32Async(num_chunks=%zu, stream=%p)", num_chunks, (void*)stream);
  if (num_chunks == 0) {
    return nvcompSuccess;
  }
  if (device_uncompressed_chunk_ptrs == nullptr || device_uncompressed_chunk_bytes == nullptr || device_crc32_ptr == nullptr) {
    return nvcompErrorInvalidValue;
  }
  clear_stale_error();
  static lzl::ResidentCache resident; /* per device ordinal */
  size_t waves = (size_t)resident.get(crc32_kernel, 64 * kWavesPerGroup, 0) * kWavesPerGroup;
  if (waves == 0) {
    waves = kDefaultWaves;
  }
  const size_t per_chunk = num_chunks < waves ? (waves + num_chunks - 1) / num_chunks : 1;
  if (per_chunk > 1 && hipMemsetAsync(device_crc32_ptr, 0, num_chunks * sizeof(uint32_t), stream) != hipSuccess) {
    return nvcompErrorCudaError;
  }
  const size_t total = num_chunks * per_chunk;
  size_t groups = (total + kWavesPerGroup - 1) / kWavesPerGroup;
  groups = groups < kMaxGroups ? groups : kMaxGroups;
  nvlog::call(4, "nvcompBatchedCRC32Async: waves_per_chunk=%zu workgroups=%zu", per_chunk, groups);
  hipLaunchKernelGGL(crc32_kernel, dim3((unsigned)groups), dim3(64 * kWavesPerGroup), 0, stream,
                     device_uncompressed_chunk_ptrs, device_uncompressed_chunk_bytes, num_chunks, device_crc32_ptr,
                     (uint32_t)per_chunk);
  return launch_status();
}

} // extern "C"
