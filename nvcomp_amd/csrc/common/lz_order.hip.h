/*
 * common/lz_order.hip.h -- the order in which a persistent LZ decode launch hands out its chunks: long chunks first.
 *
 * A persistent launch (common/lz_launch.hip.h) ends when its slowest late chunk ends: once the ticket counter runs out,
 * every wave still holds a chunk it drew at some moment, and the card empties over the decode time of the longest of
 * them. Handed out in index order, the last chunks of a shuffled batch are a random draw of it, text chunks of up to
 * 1 ms among them. Handed out by descending cost, the last ones are the cheap ones.
 *
 * ONLY THE TAIL IS ORDERED. The whole batch by descending size is slower than index order (LZ4 mix, 65 536 chunks:
 * 712 against 731 GB/s). The supposed cause, from the end-to-end times alone: the card then runs text chunks alone for
 * the first half of the launch and run-like chunks alone at the end, and the launch loses what a mix of chunks that load
 * different units gains. So the places in front
 * of the last kOrderTailPercent % of the resident waves keep their own chunks, and only the chunks behind them are
 * sorted: one round of the card is long enough for the longest chunk to start before the counter runs out (745 GB/s;
 * two rounds 742, three 737, four 736: DESIGN.md section 6).
 *
 * THE KEY reads the two size arrays of the call and nothing else, never a compressed stream (round 5's pre-pass of
 * this name parsed the first tokens of every stream with two kernels, 0.1 ms in front of every launch, and lost on
 * every batch under 16 384 chunks for it): the chunk's compressed size, which tracks its number of sequences, or 0
 * where the chunk is stored nearly raw (in_len * 10 >= cap * 9: one literal run, tens of microseconds; this also
 * covers in_len > cap and the lengths the decode loop rejects). It is quantised to kOrderBuckets buckets, eight per
 * octave (a bucket is 6-12 % wide wherever the key lies, so the scale needs no pass that finds the largest key).
 *
 * THE PASS is a counting sort in two small launches on the caller's stream, in place of the 4-byte memset that clears
 * the ticket: order_count_kernel writes one histogram per workgroup (no global atomics, so nothing needs clearing
 * first) and clears the ticket; order_scatter_kernel sums the histograms to each workgroup's first slot per bucket
 * (descending buckets; inside a bucket workgroup after workgroup, inside a workgroup as the LDS atomics fall) and
 * writes order[]. The temp buffer holds, behind the ticket's kTicketBytes, order[batch_size] and the histograms.
 *
 * The decode loop maps its place to order[place] (lzl::decode_window_loop); everything downstream uses the chunk index.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common/api_batch.hip.h"
#include "common/wave.h"

#ifndef NVCOMP_LZ_ORDER_TAIL_PERCENT
#define NVCOMP_LZ_ORDER_TAIL_PERCENT 100 /* the places that are handed out by size: the last so many, in percent of the resident waves */
#endif
#ifndef NVCOMP_LZ_ORDER_MIN_BATCH_PERCENT
#define NVCOMP_LZ_ORDER_MIN_BATCH_PERCENT 100 /* no order for a batch of no more chunks than this, in percent of the resident waves */
#endif

namespace lzl {

constexpr unsigned kOrderTailPercent = NVCOMP_LZ_ORDER_TAIL_PERCENT;
constexpr unsigned kOrderMinBatchPercent = NVCOMP_LZ_ORDER_MIN_BATCH_PERCENT;
static_assert(kOrderTailPercent > 0 && kOrderMinBatchPercent >= 100, "the whole batch by size is slower than index order; a launch that fits has nothing to order");
constexpr unsigned kOrderBuckets = 192;      /* keys below 2^26 at eight buckets per octave: (25 - 2) * 8 + 7 is the last */
constexpr unsigned kOrderThreads = 256;
constexpr unsigned kOrderMaxGroups = 64;     /* workgroups of the two kernels: each takes one contiguous part of the batch */
constexpr unsigned kOrderMinPerGroup = 1024; /* ... of at least this many chunks, while there are that many */
static_assert(kOrderBuckets % 64 == 0 && kOrderBuckets <= kOrderThreads, "one wave scans the buckets, one thread sums each");

/* Workgroups of the order pass for a batch, and what the pass needs of the temp buffer (the ticket included). */
static inline unsigned order_groups(size_t batch_size)
{
  const size_t groups = (batch_size + kOrderMinPerGroup - 1) / kOrderMinPerGroup;
  return groups < 1 ? 1u : groups > kOrderMaxGroups ? kOrderMaxGroups : (unsigned)groups;
}

static inline size_t order_temp_bytes(size_t batch_size)
{
  return kTicketBytes + sizeof(uint32_t) * (batch_size + (size_t)kOrderBuckets * order_groups(batch_size));
}

/* What nvcompBatched<Fmt>DecompressGetTempSize asks for: the ticket alone up to the waves a whole MI355X keeps resident
 * (a launch of no more chunks has a place for every chunk and nothing to order), the order's room above. The query is a
 * pure function of its arguments; the launch itself looks at the card and at the buffer it is given. */
constexpr size_t kOrderMinQueryBatch = 7168;
static inline size_t order_query_bytes(size_t num_chunks)
{
  return num_chunks > kOrderMinQueryBatch ? order_temp_bytes(num_chunks) : kTicketBytes;
}

/* The bucket of a chunk: 0 = cheap, kOrderBuckets - 1 = the longest streams. */
__host__ __device__ __forceinline__ uint32_t order_bucket(size_t in_len, size_t cap)
{
  if (cap > kMaxOutCap) {
    cap = kMaxOutCap;
  }
  if (in_len >= cap || in_len * 10 >= cap * 9) { /* in_len < cap <= 2^26 where the products are formed */
    return 0;
  }
  const uint32_t key = (uint32_t)in_len;
  if (key < 8) {
    return key;
  }
  const uint32_t e = 31u - (uint32_t)__builtin_clz(key); /* 3 ... 25 */
  return (e - 2) * 8 + ((key >> (e - 3)) & 7u);
}

/* The workgroup's part of the chunks [first, n): `per_group` of them, the last workgroups fewer or none. */
__device__ __forceinline__ void order_part(uint32_t first, uint32_t n, uint32_t per_group, uint32_t& begin, uint32_t& end)
{
  const uint64_t b = first + (uint64_t)blockIdx.x * per_group;
  begin = b < n ? (uint32_t)b : n;
  end = n - begin < per_group ? n : begin + per_group;
}

/* f(chunk, bucket) for the chunks [begin, end), a workgroup's threads side by side; four chunks' sizes are in flight per
 * thread (a workgroup's part is read in one or two round trips to memory, not one per 256 chunks). */
template <class F>
__device__ __forceinline__ void order_for_each(
    const size_t* __restrict__ comp_bytes, const size_t* __restrict__ out_caps, uint32_t begin, uint32_t end, F f)
{
  constexpr uint32_t kInFlight = 4;
  for (uint32_t base = begin; base < end; base += kInFlight * kOrderThreads) {
    size_t in_len[kInFlight], cap[kInFlight];
#pragma unroll
    for (uint32_t k = 0; k < kInFlight; ++k) {
      const uint32_t i = base + k * kOrderThreads + threadIdx.x;
      const uint32_t safe = i < end ? i : end - 1;
      in_len[k] = comp_bytes[safe];
      cap[k] = out_caps[safe];
    }
#pragma unroll
    for (uint32_t k = 0; k < kInFlight; ++k) {
      const uint32_t i = base + k * kOrderThreads + threadIdx.x;
      if (i < end) {
        f(i, order_bucket(in_len[k], cap[k]));
      }
    }
  }
}

/* hist[group][bucket]: how many chunks of the workgroup's part of [first, n) fall into each bucket. Clears the ticket,
 * and writes the places in front of `first`, which keep their own chunks. */
template <unsigned BUCKETS>
__global__ void __launch_bounds__(kOrderThreads) order_count_kernel(
    const size_t* __restrict__ comp_bytes, const size_t* __restrict__ out_caps, uint32_t first, uint32_t n, uint32_t per_group,
    uint32_t* __restrict__ ticket, uint32_t* __restrict__ hist, uint32_t* __restrict__ order)
{
  __shared__ uint32_t counts[BUCKETS];
  for (uint32_t b = threadIdx.x; b < BUCKETS; b += kOrderThreads) {
    counts[b] = 0;
  }
  __syncthreads();
  uint32_t begin, end;
  order_part(first, n, per_group, begin, end);
  order_for_each(comp_bytes, out_caps, begin, end, [&](uint32_t, uint32_t bucket) { atomicAdd(&counts[bucket], 1u); });
  for (uint32_t i = blockIdx.x * kOrderThreads + threadIdx.x; i < first; i += gridDim.x * kOrderThreads) {
    order[i] = i;
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < BUCKETS; b += kOrderThreads) {
    hist[blockIdx.x * BUCKETS + b] = counts[b];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *ticket = 0;
  }
}

/* order[first, n): the chunks [first, n) by descending bucket. */
template <unsigned BUCKETS>
__global__ void __launch_bounds__(kOrderThreads) order_scatter_kernel(
    const size_t* __restrict__ comp_bytes, const size_t* __restrict__ out_caps, uint32_t first, uint32_t n, uint32_t per_group,
    const uint32_t* __restrict__ hist, uint32_t* __restrict__ order)
{
  __shared__ uint32_t total[BUCKETS];  /* chunks of all workgroups in the bucket */
  __shared__ uint32_t cursor[BUCKETS]; /* where this workgroup's next chunk of the bucket goes */
  const uint32_t groups = gridDim.x;
  if (threadIdx.x < BUCKETS) {
    uint32_t all = 0, before = 0;
    for (uint32_t g0 = 0; g0 < groups; g0 += 16) {
#pragma unroll
      for (uint32_t g = g0; g < g0 + 16; ++g) { /* sixteen loads in flight; those past the last histogram read it again */
        const uint32_t c = hist[(g < groups ? g : groups - 1) * BUCKETS + threadIdx.x];
        all += g < groups ? c : 0u;
        before += g < blockIdx.x ? c : 0u; /* blockIdx.x < groups */
      }
    }
    total[threadIdx.x] = all;
    cursor[threadIdx.x] = first + before;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    /* the first wave adds what the higher buckets hold: lane l takes the BUCKETS / 64 next lower ones, from the top */
    constexpr uint32_t kPerLane = BUCKETS / 64;
    const uint32_t top = BUCKETS - 1 - threadIdx.x * kPerLane;
    uint32_t mine = 0;
    for (uint32_t k = 0; k < kPerLane; ++k) {
      mine += total[top - k];
    }
    uint32_t above = wave::scan_add_inclusive(mine) - mine;
    for (uint32_t k = 0; k < kPerLane; ++k) {
      cursor[top - k] += above;
      above += total[top - k];
    }
  }
  __syncthreads();
  uint32_t begin, end;
  order_part(first, n, per_group, begin, end);
  order_for_each(comp_bytes, out_caps, begin, end, [&](uint32_t i, uint32_t bucket) { order[atomicAdd(&cursor[bucket], 1u)] = i; });
}

/* ---- host side ---- */

/* Whether `temp` can hold the ticket and the order of `batch_size` chunks. */
static inline bool order_fits(const void* temp, size_t temp_bytes, size_t batch_size)
{
  return temp != nullptr && ((uintptr_t)temp & 3u) == 0 && batch_size < (1ull << 31) && temp_bytes >= order_temp_bytes(batch_size);
}

/* The two launches: the places in front of `first` keep their own chunks, the places from there on get the chunks
 * [first, batch_size) by descending key. The ticket is temp's first word, the order is returned; NULL when a launch was
 * refused (the ticket and the order are then not to be trusted: the caller clears the ticket itself). */
static inline const uint32_t* order_async(
    hipStream_t stream, void* temp, const size_t* comp_bytes, const size_t* out_caps, size_t first, size_t batch_size)
{
  const unsigned groups = order_groups(batch_size - first);
  const uint32_t per_group = (uint32_t)((batch_size - first + groups - 1) / groups);
  uint32_t* ticket = (uint32_t*)temp;
  uint32_t* order = (uint32_t*)((uint8_t*)temp + kTicketBytes);
  uint32_t* hist = order + batch_size;
  hipLaunchKernelGGL(order_count_kernel<kOrderBuckets>, dim3(groups), dim3(kOrderThreads), 0, stream, comp_bytes, out_caps,
                     (uint32_t)first, (uint32_t)batch_size, per_group, ticket, hist, order);
  hipLaunchKernelGGL(order_scatter_kernel<kOrderBuckets>, dim3(groups), dim3(kOrderThreads), 0, stream, comp_bytes, out_caps,
                     (uint32_t)first, (uint32_t)batch_size, per_group, (const uint32_t*)hist, order);
  return hipGetLastError() == hipSuccess ? order : nullptr;
}

/* launch_persistent for the decoders that hand out by order: where the launch has more chunks than resident places and
 * the temp buffer holds the order, the order pass runs in place of the ticket's memset; otherwise the launch is
 * launch_persistent's (the ticket alone with a smaller buffer, static places with none), with a null order.
 * make_args(ticket, first_dynamic, order) -> the kernel's parameter. */
template <auto Kernel, class MakeArgs>
static inline void launch_persistent_ordered(
    hipStream_t stream, void* temp, size_t temp_bytes, const Batch& b, unsigned places, unsigned block_threads, int max_per_cu,
    MakeArgs make_args)
{
  if (order_fits(temp, temp_bytes, b.batch_size)) {
    const unsigned groups = (unsigned)((b.batch_size + places - 1) / places);
    const unsigned fit = resident_fit<Kernel>(block_threads, max_per_cu);
    if (fit != 0 && fit < groups && b.batch_size > (size_t)fit * places * kOrderMinBatchPercent / 100) {
      const size_t tail = (size_t)fit * places * kOrderTailPercent / 100;
      const size_t first = tail >= b.batch_size ? 0 : b.batch_size - tail;
      const uint32_t* order = order_async(stream, temp, b.comp_bytes, b.out_caps, first, b.batch_size);
      if (order != nullptr) {
        const auto args = make_args((uint32_t*)temp, (size_t)fit * places, order);
        hipLaunchKernelGGL(Kernel, dim3(fit), dim3(block_threads), 0, stream, args);
        return;
      }
    }
  }
  launch_persistent<Kernel>(stream, temp, temp_bytes, b.batch_size, places, block_threads, max_per_cu,
                            [&](uint32_t* ticket, size_t first_dynamic) { return make_args(ticket, first_dynamic, nullptr); });
}

} // namespace lzl
