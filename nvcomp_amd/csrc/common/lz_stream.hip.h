/*
 * common/lz_stream.hip.h -- long literal runs and long matches, copied straight to HBM behind the window's back.
 */
#pragma once

#include "common/lz_out_window.hip.h"
#include "common/lz_copy.hip.h"

namespace lzw {

/* ---- long runs: straight to HBM ----------------------------------------------------------------------------------
 *
 * A sequence with a long literal run or a long match does not go through the window: the window's bytes are flushed,
 * the sequence is written to the output buffer directly with 16-byte lane accesses (1 KiB per wave instruction), and the
 * window restarts behind it (it holds no history). Data of this kind is what CAN approach the HBM roofline
 * (incompressible chunks are one literal run, runs and sorted columns are a few long matches), and through the window
 * it paid an LDS round trip, a per-batch cut at kBatchMax bytes and, for matches, a dependent load -> store chain per
 * step. The reference's only published number is of this shape (doc/Benchmarks.md:88-95).
 */
#ifndef NVCOMP_LZW_STREAM_LIT
#define NVCOMP_LZW_STREAM_LIT 4096 /* literal runs from this length on are streamed */
#endif
#ifndef NVCOMP_LZW_STREAM_MATCH
#define NVCOMP_LZW_STREAM_MATCH 4096 /* matches from this length on are streamed */
#endif
constexpr uint32_t kStreamLit = NVCOMP_LZW_STREAM_LIT;
constexpr uint32_t kStreamMatch = NVCOMP_LZW_STREAM_MATCH;

/* dst[0, n) = src[0, n): different buffers or src at least 8 KiB in front of dst; any alignment. The stores are 16-byte
 * aligned and non-temporal, four loads of 1 KiB are in flight before the first store (one load -> store round trip per KiB
 * made a 64 KiB literal run latency-bound at 2 TB/s of copy traffic), and the next four are issued BEFORE the stores of
 * the four in hand. scripts/probes/copy_bench.hip (16 384 runs of 64 KiB, the decoders' launch shape): load-then-store
 * 2 380 GB/s -- the very rate the decoder had on incompressible chunks --, with the loads ahead 2 500, with non-temporal
 * stores as well 2 615; hipMemcpyAsync device-to-device 2 499. */
__device__ __forceinline__ void stream_copy(uint8_t* dst, const uint8_t* src, uint32_t n)
{
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  const uint32_t head = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
  const uint32_t h = head < n ? head : n;
  if (lane < h) {
    wave::gstore_u8(dst + lane, wave::gload_u8(src + lane));
  }
  const uint32_t body_end = h + ((n - h) & ~15u); /* the 16-byte blocks end here */
  uint32_t base = h;
  if (base + 4096 <= body_end) {
    uint32_t at = base + 16 * lane;
    wave::u32x4 a = wave::gload_u32x4(src + at), b = wave::gload_u32x4(src + at + 1024);
    wave::u32x4 c = wave::gload_u32x4(src + at + 2048), d = wave::gload_u32x4(src + at + 3072);
    for (base += 4096; base + 4096 <= body_end; base += 4096) {
      const uint32_t nx = base + 16 * lane;
      const wave::u32x4 a2 = wave::gload_u32x4(src + nx), b2 = wave::gload_u32x4(src + nx + 1024);
      const wave::u32x4 c2 = wave::gload_u32x4(src + nx + 2048), d2 = wave::gload_u32x4(src + nx + 3072);
      wave::gstore_u32x4_aligned_nt(dst + at, a);
      wave::gstore_u32x4_aligned_nt(dst + at + 1024, b);
      wave::gstore_u32x4_aligned_nt(dst + at + 2048, c);
      wave::gstore_u32x4_aligned_nt(dst + at + 3072, d);
      a = a2, b = b2, c = c2, d = d2;
      at = nx;
    }
    wave::gstore_u32x4_aligned_nt(dst + at, a);
    wave::gstore_u32x4_aligned_nt(dst + at + 1024, b);
    wave::gstore_u32x4_aligned_nt(dst + at + 2048, c);
    wave::gstore_u32x4_aligned_nt(dst + at + 3072, d);
  }
  for (; base < body_end; base += 1024) {
    const uint32_t at = base + 16 * lane;
    if (at < body_end) {
      wave::gstore_u32x4_aligned(dst + at, wave::gload_u32x4(src + at));
    }
  }
  const uint32_t tail = body_end + lane;
  if (tail < n) {
    wave::gstore_u8(dst + tail, wave::gload_u8(src + tail));
  }
}

/* d[i] = d[i - off] for i in [0, len), off < 256, the off bytes in front of d already in HBM: the pattern is read once
 * (a dword per lane) and every 16-byte store is assembled in registers from cross-lane fetches at (position mod off);
 * when off divides 1 KiB (1, 2, 4, 8, ...: runs, typed columns) a lane's 16 bytes never change and the run is a sequence
 * of plain stores -- no load at all behind the first. */
__device__ __forceinline__ void stream_periodic(uint8_t* d, uint32_t off, uint32_t len)
{
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  uint32_t pat = 0;
  if (4 * lane < off) {
    pat = wave::gload_u32(d - off + 4 * lane); /* bytes at or behind `off` are never selected */
  }
  const uint32_t magic = kMagic.v[off]; /* x / off == umulhi(x, magic) for x < 2^16 */
  const uint32_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
  const uint32_t h = head < len ? head : len;
  {
    const uint32_t sidx = off == 1 ? 0u : lane - __umulhi(lane, magic) * off; /* lane < 64 <= 2^16 */
    const uint32_t b = wave::shuffle(pat, (lane < h ? sidx : 0u) >> 2) >> (8 * (sidx & 3u));
    if (lane < h) {
      wave::gstore_u8(d + lane, b);
    }
  }
  const uint32_t blocks = (len - h) >> 4; /* aligned 16-byte blocks */
  const uint32_t step = off == 1 ? 0u : 1024u - __umulhi(1024u, magic) * off; /* 1024 mod off: the phase shift per KiB */
  uint32_t r = h + 16 * lane;
  r = off == 1 ? 0u : r - __umulhi(r, magic) * off;
  wave::u32x4 q = {0, 0, 0, 0};
  bool fresh = true;
  for (uint32_t base = 0; base < blocks; base += 64) {
    if (fresh) {
      uint32_t sidx = r;
      uint32_t w[4];
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        uint32_t word = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t b = (wave::shuffle(pat, sidx >> 2) >> (8 * (sidx & 3u))) & 0xffu;
          word |= b << (8 * j);
          sidx = sidx + 1 == off ? 0 : sidx + 1;
        }
        w[k] = word;
      }
      q.x = w[0], q.y = w[1], q.z = w[2], q.w = w[3];
      fresh = step != 0;
      r += step;
      r = r >= off ? r - off : r;
    }
    if (base + lane < blocks) {
      wave::gstore_u32x4_aligned(d + h + 16 * (base + lane), q);
    }
  }
  const uint32_t tail_at = h + 16 * blocks;
  {
    const uint32_t i = tail_at + lane;
    const uint32_t x = i % off; /* once per run: i may be as large as the chunk */
    const uint32_t b = wave::shuffle(pat, (i < len ? x : 0u) >> 2) >> (8 * (x & 3u));
    if (i < len) {
      wave::gstore_u8(d + i, b);
    }
  }
}

/* d[i] = d[i - off], i in [0, len), byte-serial semantics, everything in front of d already in HBM (one wave's vector
 * memory operations are served in issue order: a later load sees an earlier store of the same wave). */
__device__ __forceinline__ void stream_match(uint8_t* d, uint32_t off, uint32_t len)
{
  if (off < 256) {
    stream_periodic(d, off, len);
    return;
  }
  /* The effective offset E stays a multiple of off and doubles as the run grows (E <= done + off: the source never
   * starts in front of d - off), so a step of up to E bytes reads nothing the same step writes: 4 KiB with four loads
   * in flight once E allows it, 1 KiB or 256 bytes before, single bytes for what is left. */
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  uint32_t done = 0;
  uint32_t E = off;
  while (done < len) {
    while (E < 4096 && 2 * E <= done + off) {
      E *= 2;
    }
    const uint32_t rem = len - done;
    if (E >= 4096 && rem >= 4096) {
      uint8_t* t = d + done + 16 * lane;
      const wave::u32x4 a = wave::gload_u32x4(t - E), b = wave::gload_u32x4(t - E + 1024);
      const wave::u32x4 c = wave::gload_u32x4(t - E + 2048), e = wave::gload_u32x4(t - E + 3072);
      wave::gstore_u32x4(t, a);
      wave::gstore_u32x4(t + 1024, b);
      wave::gstore_u32x4(t + 2048, c);
      wave::gstore_u32x4(t + 3072, e);
      done += 4096;
    } else if (E >= 1024 && rem >= 1024) {
      uint8_t* t = d + done + 16 * lane;
      wave::gstore_u32x4(t, wave::gload_u32x4(t - E));
      done += 1024;
    } else if (rem >= 256) { /* E >= off >= 256 */
      uint8_t* t = d + done + 4 * lane;
      wave::gstore_u32(t, wave::gload_u32(t - E));
      done += 256;
    } else {
      for (uint32_t i = lane; i < rem; i += 64) { /* rem < 256 <= E: no byte of this step reads another */
        uint8_t* t = d + done + i;
        wave::gstore_u8(t, wave::gload_u8(t - E));
      }
      done = len;
    }
    wave::sync();
  }
}

/* A sequence that is streamed instead of executed in the window (execute_window_batch reported `big` for the first
 * sequence in hand): literals [lsrc, lsrc + llen) of the stream, then the match (moff, mlen). Validates like the batch
 * executor; returns false on error. The window is flushed first and restarts empty behind the sequence. */
template <bool CHECKED>
__device__ __forceinline__ bool stream_sequence(
    const InRing& ir, OutWindow& ow, uint32_t out_cap, uint32_t& op, uint32_t lsrc, uint32_t llen, uint32_t moff, uint32_t mlen,
    uint32_t& err)
{
  /* tested whether or not the caller asked for statuses (once per streamed sequence: nothing): an unchecked decode of a
   * corrupt stream must not turn a claimed length of megabytes into an HBM-to-HBM copy past the output slot */
  {
    const uint64_t end = (uint64_t)op + llen + mlen;
    if (end > out_cap || (mlen != 0 && (moff == 0 || moff > op + llen))) {
      err |= end > out_cap ? lz::kErrOutput : lz::kErrOffset;
      return false;
    }
  }
  out_flush_all(ow, op); /* the copies below read what the window still held back */
  wave::sync();
  if (llen) {
    stream_copy(ow.out + op, ir.base + lsrc, llen);
    wave::sync();
  }
  if (mlen) {
    stream_match(ow.out + op + llen, moff, mlen);
  }
  op += llen + mlen;
  restart_window(ow, op);
  return true;
}

/* (Round 6 measured a path of its own for "a few literals, then a long match of period 1 .. 16" -- the sequences of sorted
 * key columns --: the whole wave executed such a sequence alone, sources in LDS, the run's aligned block stored straight to HBM,
 * no batch around it. ~150 instructions a sequence against the ~100 the batch executor spends on it amortised: sorted-key
 * column (HC) 2 166 -> 1 720 GB/s, int32 column 1 476 -> 1 262, gpurun r6l. Gone; what these chunks need is several runs in
 * flight at once, not a shorter path for one.) */
/* A match copied by the whole wave into the window at output position hw (everything below hw is final): its source
 * may start in front of what the window holds -- those bytes are in HBM (flushed before the window let go of them). */
__device__ __forceinline__ void coop_match(OutWindow& ow, uint32_t hw, uint32_t foff, uint32_t flen)
{
  const uint32_t fsrc = hw - foff;
  if (fsrc >= ow.valid_lo) {
    lds_match_copy(out_at(ow, hw), foff, flen);
  } else {
    const uint32_t n_hbm = fsrc + flen <= ow.valid_lo ? flen : ow.valid_lo - fsrc;
    copy_to_lds(out_at(ow, hw), ow.out + fsrc, n_hbm);
    wave::sync();
    if (n_hbm < flen) {
      lds_match_copy(out_at(ow, hw + n_hbm), foff, flen - n_hbm);
    }
  }
}

} // namespace lzw
