/*
 * common/lz_launch.hip.h -- how the batched LZ decoders (LZ4, Snappy) put a batch on the card.
 *
 * PERSISTENT WAVES. One wavefront decodes one chunk at a time, but a launch has only as many workgroups as the
 * card keeps resident; a wave that finishes its chunk takes the next one from a ticket counter in the caller's temp
 * buffer. Chunks of one batch take very different times (the mix: 5x), and with one chunk per wave and four waves per
 * workgroup a workgroup's LDS and wave slots stay allocated until its SLOWEST chunk ends; one-wave workgroups fix that
 * and pay four times as many workgroup launches instead (measured in round 2: +2 % on the mix, -7 % on uniformly fast
 * chunks). Persistent waves have neither cost. The counter is cleared by a 4-byte hipMemsetAsync on the caller's
 * stream in front of the kernel; without a temp buffer (a caller that passes NULL) the launch falls back to one
 * wave per chunk, statically.
 *
 * THE LAST PLACES BY SIZE. When the counter runs out every wave still holds a chunk, and the card empties over the
 * decode time of the slowest of them. The one-wave decoders therefore run the order pass of common/lz_order.hip.h in
 * place of that memset (two small launches that read only the call's two size arrays, clear the ticket and write
 * order[] behind it in the temp buffer): the last places of the launch, as many as it has resident waves, get the last
 * chunks of the batch by descending compressed size, chunks stored nearly raw at the very end; every place in front of
 * them keeps the chunk of its own index, so the bulk of the launch runs on the batch's own mix (the whole launch by
 * descending size is 2.6 % SLOWER than index order: DESIGN.md section 6). It runs when the launch has more chunks than
 * resident waves and the temp buffer holds the order (nvcompBatched<Fmt>DecompressGetTempSize asks for it from 7 169 chunks on); with a
 * smaller buffer the launch is the ticket's alone, with none the static one. The team and pair kernels and the
 * compressors hand out in index order.
 *
 * PATH BY BATCH SIZE. Batches of at most kTeamMaxBatch chunks cannot fill the card with one wave per chunk and run a
 * WORKGROUP of eight waves per chunk (common/lz_team.hip.h); kPairMaxBatch is the same for round 2's two waves per chunk
 * (producer / consumer, common/lz_pair.hip.h), which the team supersedes where both apply. The thresholds are
 * compile-time constants: the library has no run-time tuning state (tests force each path with an A/B build of this
 * file's macros).
 *
 * This file holds the thresholds and the compressors' parameter struct (the decoders' is lzl::Tickets). What a
 * launch needs whatever the format (the batch, the ticket, the residency query, the persistent launch itself) is
 * common/api_batch.hip.h; the kernel bodies LZ4 and Snappy share and the dispatch by batch size are common/lz_api.hip.h.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common/api_batch.hip.h"

#ifndef NVCOMP_LZ_PAIR_MAX_BATCH
#define NVCOMP_LZ_PAIR_MAX_BATCH 4096 /* two waves per chunk up to here: 319 against 310 GB/s at 4 096 chunks since the pair kernels lost their scratch
                                        * (round 4, profiles/r04_final_nsweep.jsonl; 3 072 before); 412 against 454 at 8 192. Round 6: the kernels hold
                                        * the one-wave loop with the run executor for the chunks that shrank 8 x (lzl::decode_pair: `solo`), whose
                                        * registers cost them the eighth wave per SIMD -- 7 168 resident waves for 8 192 at 4 096 chunks -- and the
                                        * mix at 4 096 chunks is FASTER so: 328 against 317 GB/s (and 301 in the persistent kernel; gpurun r6ak) */
#endif
#ifndef NVCOMP_LZ_TEAM_MAX_BATCH
#define NVCOMP_LZ_TEAM_MAX_BATCH 512 /* a WORKGROUP per chunk up to this many chunks (common/lz_team.hip.h): 263 us per chunk against 467 (two waves) and 677 (one); from 1 024 chunks on two waves per chunk keep more chunks in flight (profiles/r04_team.jsonl) */
#endif
#ifndef NVCOMP_LZ_TEAM16_MAX_BATCH
#define NVCOMP_LZ_TEAM16_MAX_BATCH 256 /* ... of which batches of at most one chunk per CU get teams of sixteen waves */
#endif
#ifndef NVCOMP_LZ_MAX_WG_PER_CU
#define NVCOMP_LZ_MAX_WG_PER_CU 7 /* cap on the persistent workgroups (of four waves) per CU; 0 = as many as stay resident.
                                   * Measured on MI355X (profiles/archive/r03_ab_g.jsonl): the decoders fit 8 waves/SIMD since they stopped
                                   * spilling, and run SLOWER there than at 7 (LZ4 mix 632 vs 644 GB/s, sorted-key column 686 vs
                                   * 750): 28 waves per CU already keep the vector, scalar and LDS pipes two thirds busy, four more
                                   * only add contention for L1 / L2 and the LDS pipe; 6 is worse again (607). */
#endif

namespace lzl {

constexpr size_t kPairMaxBatch = (size_t)(NVCOMP_LZ_PAIR_MAX_BATCH);
constexpr size_t kTeamMaxBatch = (size_t)(NVCOMP_LZ_TEAM_MAX_BATCH);
constexpr size_t kTeam16MaxBatch = (size_t)(NVCOMP_LZ_TEAM16_MAX_BATCH) < kTeamMaxBatch ? (size_t)(NVCOMP_LZ_TEAM16_MAX_BATCH) : kTeamMaxBatch;
/* The compressors' single parameter: the caller's arrays of one nvcompBatched<Fmt>CompressAsync call. */
struct CompressLaunch
{
  const void* const* in_ptrs;
  const size_t* in_bytes;
  size_t max_chunk_bytes;
  size_t batch_size;
  void* const* out_ptrs;
  size_t* out_bytes;
  uint32_t* ticket;
  size_t first_dynamic;
};

} // namespace lzl
