/*
 * common/api_batch.hip.h -- what the files under api/ have in common whatever their format: the frame of a kernel around
 * the codec's decode_chunk / encode_chunk (which chunk, its four wave-uniform arguments, the clamps, the size and status
 * lane 0 writes), the persistent launch, and the argument checks of the entry points.
 *
 * The __global__ functions stay in their files, under their own names and with their __shared__ arrays; each calls a
 * frame here with its codec's call as a lambda. A frame is taken up by a kernel only where the compiler then writes
 * the kernel's code as before, instruction for instruction (scripts/lz_window_isa.py --diff; profiles/api_frame_shared.md
 * lists the kernels that keep their own lines for that reason).
 *
 * The namespace is the LZ launch layer's, where most of this came from (common/lz_launch.hip.h, common/lz_api.hip.h):
 * kernel symbols carry it in their parameter types, and profiles and bench.py name kernels.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "common/api_launch.h"
#include "common/wave.h"

namespace lzl {

constexpr uint32_t kMaxOutCap = 1u << 26; /* no chunk decodes to more: capacities are clamped to it */
constexpr size_t kTicketBytes = 16; /* what the temp-size queries ask for: one u32 counter, padded */

/* The caller's arrays of one nvcompBatched<Fmt>DecompressAsync call. */
struct Batch
{
  const void* const* comp_ptrs;
  const size_t* comp_bytes;
  const size_t* out_caps;
  size_t* actual_bytes;
  size_t batch_size;
  void* const* out_ptrs;
  int* statuses; /* nvcompStatus_t* */
};

/* The head of a persistent kernel's single parameter: the batch, the ticket counter (NULL: one chunk per wave, statically),
 * the first place handed out by ticket (= waves of the launch) and, for the kernels that read it, the chunk of every
 * place (common/lz_order.hip.h; NULL: place i is chunk i). Read through wave::kernel_args where needed. */
struct Tickets
{
  Batch b;
  uint32_t* ticket;
  size_t first_dynamic;
  const uint32_t* order;
};

/* The wave's next chunk: `first_dynamic` + a ticket (lane 0 draws it, the wave shares it). */
__device__ __forceinline__ size_t next_chunk(uint32_t* ticket, size_t first_dynamic)
{
  uint32_t t = 0;
  if (wave::lane_id() == 0) {
    t = atomicAdd(ticket, 1u);
  }
  return first_dynamic + wave::uniform(wave::read_lane(t, 0));
}

/* One chunk of a decompress call as the wave (or workgroup) that decodes it reads it, wave-uniform. */
struct Chunk
{
  const uint8_t* in;
  uint8_t* out;
  size_t in_len;
  size_t cap; /* at most kMaxOutCap */
  __device__ __forceinline__ bool too_long() const { return in_len > 0xffffffffull - 64; }
};

template <class BatchPtr>
__device__ __forceinline__ Chunk fetch_chunk(BatchPtr b, size_t chunk)
{
  Chunk c;
  c.in = wave::uniform_ptr((const uint8_t*)b->comp_ptrs[chunk]);
  c.out = wave::uniform_ptr((uint8_t*)b->out_ptrs[chunk]);
  c.in_len = wave::uniform64(b->comp_bytes[chunk]);
  c.cap = wave::uniform64(b->out_caps[chunk]);
  if (c.cap > kMaxOutCap) {
    c.cap = kMaxOutCap;
  }
  return c;
}

/* The chunk's size and status, by one lane (the caller picks it). */
template <bool CHECKED, class BatchPtr>
__device__ __forceinline__ void report(BatchPtr b, size_t chunk, uint32_t produced, uint32_t err)
{
  size_t* actual_bytes = b->actual_bytes;
  if (actual_bytes != nullptr) {
    actual_bytes[chunk] = err ? 0 : produced;
  }
  if (CHECKED && b->statuses != nullptr) {
    b->statuses[chunk] = err ? nvcompErrorCannotDecompress : nvcompSuccess;
  }
}

/* Size queries, one wave per chunk: size_of(in, in_len) -> what the stream says it decodes to (0: malformed). */
template <class SizeOf>
__device__ __forceinline__ void decompress_size(
    const void* const* __restrict__ comp_ptrs, const size_t* __restrict__ comp_bytes, size_t* uncompressed_bytes,
    size_t batch_size, SizeOf size_of)
{
  const size_t chunk = (size_t)blockIdx.x * kWavesPerBlock + wave::uniform(threadIdx.x >> 6);
  if (chunk >= batch_size) {
    return;
  }
  const uint8_t* in = wave::uniform_ptr((const uint8_t*)comp_ptrs[chunk]);
  const size_t in_len64 = wave::uniform64(comp_bytes[chunk]);
  uint32_t produced = 0;
  if (in_len64 <= 0xffffffffull - 8) {
    produced = size_of(in, (uint32_t)in_len64);
  }
  if (wave::lane_id() == 0) {
    uncompressed_bytes[chunk] = produced;
  }
}

/* ... and one LANE per chunk, in workgroups of 256, for formats whose header says it: size_of(in, in_len) -> bytes. */
template <class SizeOf>
__device__ __forceinline__ void size_by_lane(
    const void* const* __restrict__ comp_ptrs, const size_t* __restrict__ comp_bytes, size_t* uncompressed_bytes,
    size_t batch_size, SizeOf size_of)
{
  const size_t chunk = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (chunk >= batch_size) {
    return;
  }
  uncompressed_bytes[chunk] = size_of((const uint8_t*)comp_ptrs[chunk], comp_bytes[chunk]);
}

/* The compressors that take the caller's arrays as they come: workgroups of WAVES, one chunk per wave.
 * encode(src, n, dst) -> bytes written. */
template <unsigned WAVES, class Encode>
__device__ __forceinline__ void compress_static(
    const void* const* __restrict__ in_ptrs, const size_t* __restrict__ in_bytes, size_t max_chunk_bytes, size_t batch_size,
    void* const* __restrict__ out_ptrs, size_t* out_bytes, Encode encode)
{
  const size_t chunk = (size_t)blockIdx.x * WAVES + wave::uniform(threadIdx.x >> 6);
  if (chunk >= batch_size) {
    return;
  }
  const uint8_t* src = wave::uniform_ptr((const uint8_t*)in_ptrs[chunk]);
  uint8_t* dst = wave::uniform_ptr((uint8_t*)out_ptrs[chunk]);
  const size_t n64 = wave::uniform64(in_bytes[chunk]);
  /* a chunk larger than the caller declared would overrun the output slot sized from GetMaxOutputChunkSize: it is
   * not compressed, its size reads 0 */
  const uint32_t produced = n64 > max_chunk_bytes ? 0u : encode(src, (uint32_t)n64, dst);
  if (wave::lane_id() == 0) {
    out_bytes[chunk] = produced;
  }
}

/* ---- host side ---- */

/* Workgroups of `kernel` (block threads, static LDS) the current device keeps resident at once, at most `max_per_cu`
 * per CU (0: no cap); 0 when the runtime cannot tell (the launch is then static). */
template <class Kernel>
inline unsigned resident_workgroups(Kernel kernel, unsigned block_threads, int max_per_cu, int* device = nullptr)
{
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess
      || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess
      || hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)block_threads, 0) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  if (device != nullptr) {
    *device = dev;
  }
  if (max_per_cu > 0 && per_cu > max_per_cu) {
    per_cu = max_per_cu;
  }
  return cus > 0 && per_cu > 0 ? (unsigned)cus * (unsigned)per_cu : 0u;
}

/* The same, remembered PER DEVICE ORDINAL (one instance per kernel, a function-local static of the caller): a process
 * that drives several cards from one thread (benchmarks/benchmark_allgather.cpp: hipSetDevice in a loop) gets each
 * card's own geometry, and the two runtime queries are made once per kernel and card. Lock-free; two threads racing on
 * the first call both ask and store the same answer. */
struct ResidentCache
{
  static constexpr int kDevices = 64;
  std::atomic<unsigned> known[kDevices] = {}; /* answer + 1; 0 = not asked yet */
  template <class Kernel>
  unsigned get(Kernel kernel, unsigned block_threads, int max_per_cu)
  {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    if (dev < 0 || dev >= kDevices) {
      return resident_workgroups(kernel, block_threads, max_per_cu);
    }
    const unsigned seen = known[dev].load(std::memory_order_relaxed);
    if (seen != 0) {
      return seen - 1;
    }
    const unsigned fit = resident_workgroups(kernel, block_threads, max_per_cu);
    known[dev].store(fit + 1, std::memory_order_relaxed);
    return fit;
  }
};

/* ... of Kernel, whoever asks. */
template <auto Kernel>
static inline unsigned resident_fit(unsigned block_threads, int max_per_cu)
{
  static ResidentCache resident; /* per kernel; inside, per device ordinal */
  return resident.get(Kernel, block_threads, max_per_cu);
}

/* Launch Kernel over a batch, `places` chunks per workgroup at a time. Persistent when the caller's temp buffer
 * can hold the ticket counter: as many workgroups as stay resident (at most `max_per_cu` per CU; 0: no cap), the rest of
 * the batch by ticket. Otherwise one place per chunk, statically. make_args(ticket, first_dynamic) -> the kernel's parameter. */
template <auto Kernel, class MakeArgs>
static inline void launch_persistent(
    hipStream_t stream, void* temp, size_t temp_bytes, size_t batch_size, unsigned places, unsigned block_threads,
    int max_per_cu, MakeArgs make_args)
{
  unsigned groups = (unsigned)((batch_size + places - 1) / places);
  uint32_t* ticket = nullptr;
  if (temp != nullptr && temp_bytes >= sizeof(uint32_t) && ((uintptr_t)temp & 3u) == 0) {
    const unsigned fit = resident_fit<Kernel>(block_threads, max_per_cu);
    if (fit != 0 && fit < groups && hipMemsetAsync(temp, 0, sizeof(uint32_t), stream) == hipSuccess) {
      ticket = (uint32_t*)temp;
      groups = fit;
    }
  }
  const auto args = make_args(ticket, (size_t)groups * places);
  hipLaunchKernelGGL(Kernel, dim3(groups), dim3(block_threads), 0, stream, args);
}

/* Whether the caller passed every array the call needs. */
template <class... T>
static inline bool all_set(const T*... arrays)
{
  return (... && (arrays != nullptr));
}

/* What every *Async entry point does behind its own checks of options and sizes: an empty batch is a success whatever
 * the pointers, a missing array an error; otherwise launch() puts the kernels on the stream. launch() may return a
 * status of its own; anything but success is returned in place of the launch's. */
template <class Launch>
static inline nvcompStatus_t checked_launch(size_t batch_size, bool arrays_ok, Launch launch)
{
  if (batch_size == 0) {
    return nvcompSuccess;
  }
  if (!arrays_ok) {
    return nvcompErrorInvalidValue;
  }
  clear_stale_error();
  if constexpr (std::is_void_v<decltype(launch())>) {
    launch();
  } else {
    const nvcompStatus_t refused = launch();
    if (refused != nvcompSuccess) {
      return refused;
    }
  }
  return launch_status();
}

/* nvcompBatched<format>GetDecompressSizeAsync with the format's size kernel, in workgroups of `block_threads` that
 * take `places` chunks each. */
template <auto Kernel>
static inline nvcompStatus_t decompress_size_async(
    const void* const* comp_ptrs, const size_t* comp_bytes, size_t* uncompressed_bytes, size_t batch_size, hipStream_t stream,
    unsigned places = kWavesPerBlock, unsigned block_threads = 64 * kWavesPerBlock)
{
  return checked_launch(batch_size, all_set(comp_ptrs, comp_bytes, uncompressed_bytes), [&] {
    hipLaunchKernelGGL(Kernel, dim3((unsigned)((batch_size + places - 1) / places)), dim3(block_threads), 0, stream, comp_ptrs,
                       comp_bytes, uncompressed_bytes, batch_size);
  });
}

/* ... with a size_by_lane kernel. */
template <auto Kernel>
static inline nvcompStatus_t size_by_lane_async(
    const void* const* comp_ptrs, const size_t* comp_bytes, size_t* uncompressed_bytes, size_t batch_size, hipStream_t stream)
{
  return decompress_size_async<Kernel>(comp_ptrs, comp_bytes, uncompressed_bytes, batch_size, stream, 256, 256);
}

/* What the three compress entry points check first: `opts_ok` is the format's verdict on its options. */
static inline nvcompStatus_t compress_opts_status(bool opts_ok, size_t max_chunk_bytes, size_t limit)
{
  if (!opts_ok) {
    return nvcompErrorInvalidValue;
  }
  return max_chunk_bytes > limit ? nvcompErrorChunkSizeTooLarge : nvcompSuccess;
}

/* nvcompBatched<format>CompressGetTempSize / GetMaxOutputChunkSize: the result pointer, then `opts_status`
 * (compress_opts_status), and only then value() -> *result. */
template <class Value>
static inline nvcompStatus_t compress_query(size_t* result, nvcompStatus_t opts_status, Value value)
{
  const nvcompStatus_t st = result == nullptr ? nvcompErrorInvalidValue : opts_status;
  if (st == nvcompSuccess) {
    *result = value();
  }
  return st;
}

/* nvcompBatched<format>DecompressGetTempSize: `bytes` for a batch, nothing for none. */
static inline nvcompStatus_t temp_size(size_t num_chunks, size_t* temp_bytes, size_t bytes = kTicketBytes)
{
  if (temp_bytes == nullptr) {
    return nvcompErrorInvalidValue;
  }
  *temp_bytes = num_chunks == 0 ? 0 : bytes;
  return nvcompSuccess;
}

/* ... of a codec that keeps all its state in registers and LDS. */
static inline nvcompStatus_t no_temp(size_t* temp_bytes)
{
  return temp_size(0, temp_bytes);
}

} // namespace lzl

/* The *GetTempSizeEx queries of a format whose scratch does not depend on the batch's total size: the plain query's answer.
 * Inside extern "C". */
#define NVCOMP_API_COMPRESS_TEMP_SIZE_EX(Format, Opts)                                                                       \
  nvcompStatus_t nvcompBatched##Format##CompressGetTempSizeEx(size_t batch_size, size_t max_uncompressed_chunk_bytes,      \
                                                              Opts format_opts, size_t* temp_bytes,                         \
                                                              const size_t /*max_total_uncompressed_bytes*/)                \
  {                                                                                                                         \
    return nvcompBatched##Format##CompressGetTempSize(batch_size, max_uncompressed_chunk_bytes, format_opts, temp_bytes);  \
  }
#define NVCOMP_API_DECOMPRESS_TEMP_SIZE_EX(Format)                                                                           \
  nvcompStatus_t nvcompBatched##Format##DecompressGetTempSizeEx(size_t num_chunks, size_t max_uncompressed_chunk_bytes,    \
                                                                size_t* temp_bytes, size_t /*max_total_uncompressed_bytes*/) \
  {                                                                                                                         \
    return nvcompBatched##Format##DecompressGetTempSize(num_chunks, max_uncompressed_chunk_bytes, temp_bytes);             \
  }
