/*
 * common/lz_api.hip.h -- what api/lz4_api.hip and api/snappy_api.hip have in common: the bodies of their kernels around
 * the format's decode / encode call, the persistent-or-static launch, the dispatch by batch size (common/lz_launch.hip.h)
 * and the argument checks of the entry points.
 *
 * The __global__ functions stay in the two files, under their own names and with their __shared__ arrays; each declares
 * its LDS and calls a body here. A FORMAT is a struct of static functions (Lz4, Snappy in the two files):
 *   using FrontEnd                      what the team (common/lz_team.hip.h) and the two waves (common/lz_pair.hip.h) decode with
 *   kEmptyIsError                       whether a stream of 0 bytes is malformed (Snappy: no preamble) or decodes to nothing (LZ4)
 *   runs(in_len, cap)                   whether the chunk shrank enough to try the run executor
 *   alone<CHECKED>(in, n, out, cap, lds, err)           the one-wave loop that holds the run executor
 *   kPairRuns                           whether the two-wave kernel's consumer tries the run executor (not as a team's fallback)
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common/api_launch.h"
#include "common/log.h"
#include "common/lz_launch.hip.h"
#include "common/lz_window.hip.h"
#include "common/lz_pair.hip.h"
#include "common/lz_team.hip.h"

#ifndef NVCOMP_LZ_DEC_WAVES_PER_BLOCK
#define NVCOMP_LZ_DEC_WAVES_PER_BLOCK 4
#endif
#ifndef NVCOMP_LZM_WAVES_PER_BLOCK
#define NVCOMP_LZM_WAVES_PER_BLOCK 4
#endif
/* Untyped data takes the 256-position steps of common/lz_match_wide.hip.h; typed data (2- and 4-byte elements) the
 * one-window compressor of common/lz_match.hip.h. */
#ifndef NVCOMP_LZMW_WAVES_PER_BLOCK
#define NVCOMP_LZMW_WAVES_PER_BLOCK 1
#endif
#ifndef NVCOMP_LZMW_WAVES_PER_SIMD
#define NVCOMP_LZMW_WAVES_PER_SIMD 4 /* what the wave's LDS allows (15-16 waves per CU): a budget of 128 registers */
#endif

namespace lzl {

constexpr unsigned kDecWaves = NVCOMP_LZ_DEC_WAVES_PER_BLOCK;
constexpr unsigned kEncWaves = NVCOMP_LZM_WAVES_PER_BLOCK; /* the compressors' workgroup size */
constexpr unsigned kWideWaves = NVCOMP_LZMW_WAVES_PER_BLOCK;

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

/* One wave (`w` of its workgroup) per chunk at a time; with a ticket counter the waves are persistent (common/lz_launch.hip.h).
 * decode(chunk, launch arguments, err) -> bytes produced, for chunks that are not too long. */
template <bool CHECKED, class Decode>
__device__ __forceinline__ void decode_window_loop(const Launch& launch, uint32_t w, Decode decode)
{
  size_t place = (size_t)blockIdx.x * kDecWaves + w; /* the wave's place in the launch = its first chunk */
#ifdef NVCOMP_LZW_PROF
  lzw::prof_begin();
#endif
  for (;;) {
    /* the arguments are read where they are used, not held in scalar registers across the decode (wave::kernel_args) */
    const auto* a = wave::kernel_args(launch);
    if (place >= a->b.batch_size) {
      break;
    }
    const size_t chunk = place;
    const Chunk c = fetch_chunk(&a->b, chunk);
    uint32_t err = lz::kErrNone;
    uint32_t produced = 0;
    if (c.too_long()) {
      err = lz::kErrInput;
    } else {
      produced = decode(c, a, err);
    }
    if (wave::lane_id() == 0) {
      report<CHECKED>(&a->b, chunk, produced, err);
    }
    a = wave::kernel_args(launch);
    uint32_t* ticket = a->ticket;
    if (ticket == nullptr) {
      break;
    }
    place = next_chunk(ticket, a->first_dynamic);
  }
#ifdef NVCOMP_LZW_PROF
  lzw::prof_end();
#endif
}

/* Small batches: two waves per chunk, a producer (chase + parse) and a consumer (execute), common/lz_pair.hip.h. `lds`: the workgroup's
 * lzw::pair::kLdsPerChunk bytes. */
template <bool CHECKED, class Format>
__device__ __forceinline__ void decode_pair(const Batch& b, uint8_t* lds)
{
  const uint32_t w = wave::uniform(threadIdx.x >> 6);
  const size_t chunk = blockIdx.x;
  if (chunk >= b.batch_size) {
    return;
  }
  lzw::pair::reset_control(lds);
  __syncthreads();
  const Chunk c = fetch_chunk(&b, chunk);
  const bool work = !c.too_long() && c.in_len != 0;
  /* A chunk that shrank 8 x or more is decoded by the second wave ALONE, with the one-wave loop that holds the run
   * executor (Format::alone; the first wave leaves): sorted keys and typed columns are 4-5 x faster there than through
   * producer and consumer (4 096 chunks of the sorted-key column: 840 GB/s here, 5 120 chunks in the persistent kernel:
   * 3 850). That loop's registers cost this kernel its eighth wave per SIMD (common/lz_launch.hip.h: the mix does not mind). */
  static_assert(lzw::kLdsPerWave <= lzw::pair::kLdsPerChunk, "the lone wave's LDS is the pair's");
  const bool solo = work && Format::runs(c.in_len, c.cap);
  if (w == 0) {
    if (work && !solo) {
      lzw::pair::produce<typename Format::FrontEnd, CHECKED>(c.in, (uint32_t)c.in_len, lds);
    }
    return;
  }
  uint32_t err = c.too_long() || (Format::kEmptyIsError && c.in_len == 0) ? lz::kErrInput : lz::kErrNone;
  uint32_t produced = 0;
  if (solo) {
    produced = Format::template alone<CHECKED>(c.in, (uint32_t)c.in_len, c.out, (uint32_t)c.cap, lds, err);
  } else if (work) {
    produced = lzw::pair::consume<typename Format::FrontEnd, CHECKED, Format::kPairRuns>(c.in, (uint32_t)c.in_len, c.out, (uint32_t)c.cap, lds, err);
  }
  if (wave::lane_id() == 0) {
    report<CHECKED>(&b, chunk, produced, err);
  }
}

/* A workgroup per chunk (common/lz_team.hip.h): batches that cannot fill the card with one wave per chunk. Persistent
 * workgroups when the caller's temp buffer holds a ticket counter, one workgroup per chunk otherwise. `lds`: the
 * workgroup's lzt::Geo<WAVES>::kLds bytes. */
template <bool CHECKED, uint32_t WAVES, class Format>
__device__ __forceinline__ void decode_team_loop(const Launch& launch, uint8_t* lds)
{
  size_t chunk = blockIdx.x;
#ifdef NVCOMP_LZW_PROF
  lzw::prof_begin();
#endif
  for (;;) {
    const auto* a = wave::kernel_args(launch);
    if (chunk >= a->b.batch_size) {
      break;
    }
    const Chunk c = fetch_chunk(&a->b, chunk);
    uint32_t err = lz::kErrNone;
    uint32_t produced = 0;
    if (c.too_long()) {
      err = lz::kErrInput;
    } else {
      produced = lzt::decode_chunk<typename Format::FrontEnd, WAVES>(
          c.in, (uint32_t)c.in_len, c.out, (uint32_t)c.cap, lds, err,
          [](uint32_t role, const uint8_t* i, uint32_t n, uint8_t* o, uint32_t cap, uint8_t* scratch, uint32_t& e) -> uint32_t {
            /* the team's fallback is the two-wave kernel: chunks that shrank 8 x (here: mostly the 16 x ones of the team's
             * own test) are runs -- one wave with the loop that holds the run executor */
            const bool solo = Format::runs(n, cap);
            if (role == 0) {
              if (!solo) {
                lzw::pair::produce<typename Format::FrontEnd, true>(i, n, scratch);
              }
              return 0u;
            }
            if (solo) {
              return Format::template alone<true>(i, n, o, cap, scratch, e);
            }
            return lzw::pair::consume<typename Format::FrontEnd, true, false>(i, n, o, cap, scratch, e);
          });
    }
    a = wave::kernel_args(launch);
    if (threadIdx.x == 0) {
      report<CHECKED>(&a->b, chunk, produced, err);
    }
    uint32_t* ticket = a->ticket;
    if (ticket == nullptr) {
      break;
    }
    uint32_t* slot = (uint32_t*)(lds + lzt::Geo<WAVES>::kLds - 4 * lzt::kCtlWords) + lzt::kCtlTicket;
    if (threadIdx.x == 0) {
      *slot = atomicAdd(ticket, 1u);
    }
    __syncthreads();
    chunk = a->first_dynamic + wave::uniform(*slot);
    __syncthreads();
  }
#ifdef NVCOMP_LZW_PROF
  lzw::prof_end();
#endif
}

/* One wave per chunk: size_of(in, in_len) -> what the stream says it decodes to (0: malformed). */
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

/* The compressors: wave `w` of workgroups of WAVES; persistent waves, as in the decoders (common/lz_launch.hip.h): chunks of
 * a batch compress at very different speeds. encode(src, n, dst) -> bytes written. */
template <unsigned WAVES, class Encode>
__device__ __forceinline__ void compress_loop(const CompressLaunch& launch, uint32_t w, Encode encode)
{
  size_t chunk = (size_t)blockIdx.x * WAVES + w;
  for (;;) {
    const auto* a = wave::kernel_args(launch);
    if (chunk >= a->batch_size) {
      break;
    }
    const uint8_t* src = wave::uniform_ptr((const uint8_t*)a->in_ptrs[chunk]);
    uint8_t* dst = wave::uniform_ptr((uint8_t*)a->out_ptrs[chunk]);
    const size_t n64 = wave::uniform64(a->in_bytes[chunk]);
    /* a chunk larger than the caller declared would overrun the output slot sized from GetMaxOutputChunkSize: it is
     * not compressed, its size reads 0 */
    const uint32_t produced = n64 > a->max_chunk_bytes ? 0u : encode(src, (uint32_t)n64, dst);
    a = wave::kernel_args(launch);
    if (wave::lane_id() == 0) {
      a->out_bytes[chunk] = produced;
    }
    uint32_t* ticket = a->ticket;
    if (ticket == nullptr) {
      break;
    }
    chunk = next_chunk(ticket, a->first_dynamic);
  }
}

/* ---- host side ---- */

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
    static ResidentCache resident; /* per kernel; inside, per device ordinal */
    const unsigned fit = resident.get(Kernel, block_threads, max_per_cu);
    if (fit != 0 && fit < groups && hipMemsetAsync(temp, 0, sizeof(uint32_t), stream) == hipSuccess) {
      ticket = (uint32_t*)temp;
      groups = fit;
    }
  }
  const auto args = make_args(ticket, (size_t)groups * places);
  hipLaunchKernelGGL(Kernel, dim3(groups), dim3(block_threads), 0, stream, args);
}

static inline nvcompStatus_t temp_size(size_t num_chunks, size_t* temp_bytes, size_t bytes = kTicketBytes)
{
  if (temp_bytes == nullptr) {
    return nvcompErrorInvalidValue;
  }
  *temp_bytes = num_chunks == 0 ? 0 : bytes;
  return nvcompSuccess;
}

/* nvcompBatched<format>DecompressAsync with the format's four kernels: which one runs is decided by the batch size alone.
 * with_index: the one-wave-per-chunk launch gets the token-index slices of the temp buffer when it has room for them. */
template <auto Team16, auto Team8, auto Pair, auto Window>
static inline nvcompStatus_t decompress_async(
    const char* format, bool with_index, const void* const* comp_ptrs, const size_t* comp_bytes, const size_t* out_caps,
    size_t* actual_bytes, size_t batch_size, void* temp, size_t temp_bytes, void* const* out_ptrs, nvcompStatus_t* statuses,
    hipStream_t stream)
{
  nvlog::call(3, "nvcompBatched%sDecompressAsync(batch_size=%zu, statuses=%s, actual_sizes=%s, temp_bytes=%zu, stream=%p)", format,
              batch_size, statuses ? "yes" : "null", actual_bytes ? "yes" : "null", temp_bytes, (void*)stream);
  if (batch_size == 0) {
    return nvcompSuccess;
  }
  if (comp_ptrs == nullptr || comp_bytes == nullptr || out_caps == nullptr || out_ptrs == nullptr) {
    return nvcompErrorInvalidValue;
  }
  clear_stale_error();
  /* Bounds are checked whether or not the caller asked for statuses (round 4): the kernels without the checks were no
   * faster (655-668 against 675 GB/s on the headline batch over three evidence runs: the checks are a handful of
   * wave-uniform tests per batch), and a corrupt stream decoded with statuses == NULL could write past its output slot.
   * A NULL status array only means that nobody is told: a failed chunk still reads 0 in actual_bytes. */
  const Batch b = {comp_ptrs, comp_bytes, out_caps, actual_bytes, batch_size, out_ptrs, (int*)statuses};
  if (batch_size <= kTeam16MaxBatch) {
    /* at most one chunk per CU: sixteen waves a chunk (one team holds a whole CU's LDS budget for two) */
    const Launch one_each = {b, nullptr, batch_size, nullptr};
    hipLaunchKernelGGL(Team16, dim3((unsigned)batch_size), dim3(1024), 0, stream, one_each);
  } else if (batch_size <= kTeamMaxBatch) {
    /* small batches cannot fill the card with one wave per chunk: a workgroup per chunk (common/lz_team.hip.h) */
    launch_persistent<Team8>(stream, temp, temp_bytes, batch_size, 1, 512, 0,
                             [&](uint32_t* ticket, size_t first_dynamic) { return Launch{b, ticket, first_dynamic, nullptr}; });
  } else if (batch_size <= kPairMaxBatch) {
    /* (round 2's path for small batches: two waves per chunk, producer / consumer) */
    hipLaunchKernelGGL(Pair, dim3((unsigned)batch_size), dim3(128), 0, stream, b);
  } else {
    launch_persistent<Window>(stream, temp, temp_bytes, batch_size, kDecWaves, 64 * kDecWaves, NVCOMP_LZ_MAX_WG_PER_CU,
                              [&](uint32_t* ticket, size_t waves) {
                                return Launch{b, ticket, waves, with_index ? index_base(temp, temp_bytes, waves) : nullptr};
                              });
  }
  return launch_status();
}

/* nvcompBatched<format>GetDecompressSizeAsync with the format's size kernel. */
template <auto Kernel>
static inline nvcompStatus_t decompress_size_async(
    const void* const* comp_ptrs, const size_t* comp_bytes, size_t* uncompressed_bytes, size_t batch_size, hipStream_t stream)
{
  if (batch_size == 0) {
    return nvcompSuccess;
  }
  if (comp_ptrs == nullptr || comp_bytes == nullptr || uncompressed_bytes == nullptr) {
    return nvcompErrorInvalidValue;
  }
  clear_stale_error();
  hipLaunchKernelGGL(Kernel, dim3(grid_for(batch_size)), dim3(64 * kWavesPerBlock), 0, stream, comp_ptrs, comp_bytes,
                     uncompressed_bytes, batch_size);
  return launch_status();
}

/* What the three compress entry points check first: `opts_ok` is the format's verdict on its options. */
static inline nvcompStatus_t compress_opts_status(bool opts_ok, size_t max_chunk_bytes, size_t limit)
{
  if (!opts_ok) {
    return nvcompErrorInvalidValue;
  }
  return max_chunk_bytes > limit ? nvcompErrorChunkSizeTooLarge : nvcompSuccess;
}

/* The arguments of nvcompBatched<format>CompressAsync, behind the format's name and compress_opts_status(). */
struct CompressCall
{
  const char* format;
  nvcompStatus_t opts_status;
  const void* const* in_ptrs;
  const size_t* in_bytes;
  size_t max_chunk_bytes;
  size_t batch_size;
  void* temp;
  size_t temp_bytes;
  void* const* out_ptrs;
  size_t* out_bytes;
  hipStream_t stream;
};

/* ... with the compressor the format chose: Kernel, in workgroups of WAVES. The per-chunk hash tables live in LDS; the temp
 * buffer is the persistent waves' ticket counter. */
template <auto Kernel, unsigned WAVES>
static inline nvcompStatus_t compress_async(const CompressCall& c)
{
  nvlog::call(3, "nvcompBatched%sCompressAsync(batch_size=%zu, max_uncompressed_chunk_bytes=%zu, stream=%p)", c.format, c.batch_size,
              c.max_chunk_bytes, (void*)c.stream);
  if (c.opts_status != nvcompSuccess) {
    return c.opts_status;
  }
  if (c.batch_size == 0) {
    return nvcompSuccess;
  }
  if (c.in_ptrs == nullptr || c.in_bytes == nullptr || c.out_ptrs == nullptr || c.out_bytes == nullptr) {
    return nvcompErrorInvalidValue;
  }
  clear_stale_error();
  launch_persistent<Kernel>(c.stream, c.temp, c.temp_bytes, c.batch_size, WAVES, 64 * WAVES, 0,
                            [&](uint32_t* ticket, size_t first_dynamic) {
                              return CompressLaunch{c.in_ptrs, c.in_bytes, c.max_chunk_bytes, c.batch_size,
                                                    c.out_ptrs, c.out_bytes, ticket, first_dynamic};
                            });
  return launch_status();
}

} // namespace lzl
