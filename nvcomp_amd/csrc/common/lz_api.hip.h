/*
 * common/lz_api.hip.h -- what api/lz4_api.hip and api/snappy_api.hip have in common beyond what every format has
 * (common/api_batch.hip.h: the chunk frame, the persistent launch, the argument checks): the bodies of their window, pair,
 * team and compress kernels around the format's decode / encode call, and the dispatch by batch size (common/lz_launch.hip.h).
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

#include "common/log.h"
#include "common/lz_launch.hip.h"
#include "common/lz_order.hip.h"
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
/* the size query's threshold is the waves of a whole MI355X (256 CUs) at the launch's cap: change them together */
static_assert(NVCOMP_LZ_MAX_WG_PER_CU == 0 || kOrderMinQueryBatch == 256u * NVCOMP_LZ_MAX_WG_PER_CU * kDecWaves,
              "common/lz_order.hip.h: kOrderMinQueryBatch is the resident waves of the one-wave decoders");

/* One wave (`w` of its workgroup) per chunk at a time; with a ticket counter the waves are persistent (common/lz_launch.hip.h).
 * A place of the launch (the wave's own first, then one per ticket) is chunk order[place] where the launch has an order
 * (common/lz_order.hip.h: long chunks first), the chunk of that index otherwise.
 * decode(chunk, err) -> bytes produced, for chunks that are not too long. */
template <bool CHECKED, class Decode>
__device__ __forceinline__ void decode_window_loop(const Tickets& launch, uint32_t w, Decode decode)
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
    const uint32_t* order = a->order;
    const size_t chunk = order != nullptr ? (size_t)wave::uniform(order[place]) : place;
    const Chunk c = fetch_chunk(&a->b, chunk);
    uint32_t err = lz::kErrNone;
    uint32_t produced = 0;
    if (c.too_long()) {
      err = lz::kErrInput;
    } else {
      produced = decode(c, err);
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
__device__ __forceinline__ void decode_team_loop(const Tickets& launch, uint8_t* lds)
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

/* nvcompBatched<format>DecompressAsync with the format's four kernels: which one runs is decided by the batch size alone. */
template <auto Team16, auto Team8, auto Pair, auto Window>
static inline nvcompStatus_t decompress_async(
    const char* format, const void* const* comp_ptrs, const size_t* comp_bytes, const size_t* out_caps,
    size_t* actual_bytes, size_t batch_size, void* temp, size_t temp_bytes, void* const* out_ptrs, nvcompStatus_t* statuses,
    hipStream_t stream)
{
  nvlog::call(3, "nvcompBatched%sDecompressAsync(batch_size=%zu, statuses=%s, actual_sizes=%s, temp_bytes=%zu, stream=%p)", format,
              batch_size, statuses ? "yes" : "null", actual_bytes ? "yes" : "null", temp_bytes, (void*)stream);
  /* Bounds are checked whether or not the caller asked for statuses (round 4): the kernels without the checks were no
   * faster (655-668 against 675 GB/s on the headline batch over three evidence runs: the checks are a handful of
   * wave-uniform tests per batch), and a corrupt stream decoded with statuses == NULL could write past its output slot.
   * A NULL status array only means that nobody is told: a failed chunk still reads 0 in actual_bytes. */
  const Batch b = {comp_ptrs, comp_bytes, out_caps, actual_bytes, batch_size, out_ptrs, (int*)statuses};
  return checked_launch(batch_size, all_set(comp_ptrs, comp_bytes, out_caps, out_ptrs), [&] {
    if (batch_size <= kTeam16MaxBatch) {
      /* at most one chunk per CU: sixteen waves a chunk (one team holds a whole CU's LDS budget for two) */
      const Tickets one_each = {b, nullptr, batch_size, nullptr};
      hipLaunchKernelGGL(Team16, dim3((unsigned)batch_size), dim3(1024), 0, stream, one_each);
    } else if (batch_size <= kTeamMaxBatch) {
      /* small batches cannot fill the card with one wave per chunk: a workgroup per chunk (common/lz_team.hip.h) */
      launch_persistent<Team8>(stream, temp, temp_bytes, batch_size, 1, 512, 0,
                               [&](uint32_t* ticket, size_t first_dynamic) { return Tickets{b, ticket, first_dynamic, nullptr}; });
    } else if (batch_size <= kPairMaxBatch) {
      /* (round 2's path for small batches: two waves per chunk, producer / consumer) */
      hipLaunchKernelGGL(Pair, dim3((unsigned)batch_size), dim3(128), 0, stream, b);
    } else {
      /* persistent waves; with more chunks than waves and the temp buffer of the size query, long chunks first */
      launch_persistent_ordered<Window>(
          stream, temp, temp_bytes, b, kDecWaves, 64 * kDecWaves, NVCOMP_LZ_MAX_WG_PER_CU,
          [&](uint32_t* ticket, size_t waves, const uint32_t* order) { return Tickets{b, ticket, waves, order}; });
    }
  });
}

/* nvcompAmd<format>DecompressOrderAsync (include/nvcomp/amd_ext.h), for tests and scripts: what a persistent decode launch
 * of the format's Window kernel holds on this card (`resident_places`: waves, = chunks in flight; 0 when the runtime cannot
 * tell) and, for a batch and a temp buffer, the order pass alone (common/lz_order.hip.h) with the places in front of
 * `first_ordered` left to their own chunks: `order_offset` is where in the temp buffer the batch_size chunk indices
 * (uint32) then stand. nvcompErrorInvalidValue when the temp buffer cannot hold them or first_ordered > batch_size.
 * Either result pointer may be NULL. */
template <auto Window>
static inline nvcompStatus_t order_inspect_async(
    const size_t* comp_bytes, const size_t* out_caps, size_t first_ordered, size_t batch_size, void* temp, size_t temp_bytes,
    size_t* order_offset, size_t* resident_places, hipStream_t stream)
{
  if (resident_places != nullptr) {
    *resident_places = (size_t)resident_fit<Window>(64 * kDecWaves, NVCOMP_LZ_MAX_WG_PER_CU) * kDecWaves;
  }
  if (order_offset == nullptr) {
    return nvcompSuccess;
  }
  return checked_launch(batch_size, all_set(comp_bytes, out_caps), [&]() -> nvcompStatus_t {
    if (first_ordered > batch_size || !order_fits(temp, temp_bytes, batch_size)) {
      return nvcompErrorInvalidValue;
    }
    const uint32_t* order = order_async(stream, temp, comp_bytes, out_caps, first_ordered, batch_size);
    if (order == nullptr) {
      return nvcompErrorCudaError;
    }
    *order_offset = (size_t)((const uint8_t*)order - (const uint8_t*)temp);
    return nvcompSuccess;
  });
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
  return checked_launch(c.batch_size, all_set(c.in_ptrs, c.in_bytes, c.out_ptrs, c.out_bytes), [&] {
    launch_persistent<Kernel>(c.stream, c.temp, c.temp_bytes, c.batch_size, WAVES, 64 * WAVES, 0,
                              [&](uint32_t* ticket, size_t first_dynamic) {
                                return CompressLaunch{c.in_ptrs, c.in_bytes, c.max_chunk_bytes, c.batch_size,
                                                      c.out_ptrs, c.out_bytes, ticket, first_dynamic};
                              });
  });
}

} // namespace lzl
