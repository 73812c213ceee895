/*
 * common/lz_run_batch.hip.h -- the run executor: batches of "a few literals, then a match of period 1 .. 16"
 * (sorted keys, typed columns), sixty sequences at a time straight to the output.
 */
#pragma once

#include "common/lz_out_window.hip.h"
#include "common/lz_copy.hip.h"
#include "common/lz_stream.hip.h"

namespace lzw {

/* ---- runs: sequences that are "a few literals, then a match of period 1, 2, 4, 8 or 16" ---------------------------------
 *
 * Sorted key columns, typed columns, runs -- the reference's only published LZ4 number is of this shape
 * (doc/Benchmarks.md:88-95) -- decode to a few hundred such sequences a chunk, 200-400 bytes each. The batch executor
 * below takes five of them per batch (2 KiB of window) and copies every match with the whole wave, one after the other:
 * ~65 vector and ~80 scalar instructions a sequence, 0.28 of the memory roofline with neither the memory system nor the
 * vector units busy. Here up to 64 of them are executed at once and never pass through the window:
 *
 *   pattern   With a period that divides 16, every ALIGNED 16-byte block of a run holds the same 16 bytes Q (byte i = the
 *             byte of every output address congruent to i). Q of sequence k is Q of sequence k - 1 with the literals of k
 *             written over it at their address residues: a "last writer" scan across the lanes
 *             (wave::scan_last_writer), seeded with the 16 bytes in front of the batch from the window.
 *   joints    The blocks that are not all run -- the end of run k - 1, the literals of k, the head of run k: at most two
 *             blocks a sequence with up to 16 literals -- are assembled in a 32-byte slot per lane (the window's LDS, which
 *             nothing else needs meanwhile) and stored by their lane.
 *   bodies    The whole blocks of a run are stores of Q, 1 KiB per instruction, a short scalar loop per run.
 *
 * Sequences without literals behind a match of the same period continue its run (liblz4's fast compressor cuts a run in
 * two, Snappy's copies end at 64 bytes): they are merged into it. The window restarts behind the batch with the last 16
 * bytes as its history. Returns the number of sequences executed; 0 = not this kind of batch, nothing touched: the
 * caller goes on with execute_window_batch (which also reports what is wrong with a corrupt stream).
 */
#ifndef NVCOMP_LZW_RUNS
#define NVCOMP_LZW_RUNS 1 /* A/B: 0 = every batch through execute_window_batch (rounds 1-5) */
#endif
#ifndef NVCOMP_LZW_RUN_MIN
#define NVCOMP_LZW_RUN_MIN 4 /* fewer leading sequences of the shape (and fewer than 256 bytes): not worth the fixed cost of this path */
#endif
constexpr uint32_t kRunMin = NVCOMP_LZW_RUN_MIN;
#ifndef NVCOMP_LZW_RUN_MIN_BYTES
#define NVCOMP_LZW_RUN_MIN_BYTES 2048 /* a batch of runs smaller than this (a batch of the window): not worth it -- the path's
                                        * fixed cost is ~450 instructions, the window's batch of 2 KiB costs ~1 000 all in (measured:
                                        * Snappy's int32 column, whose 64 elements a refill are ~9 runs or 2-4 KB, lost 10 % here) */
#endif
constexpr uint32_t kRunMinBytes = NVCOMP_LZW_RUN_MIN_BYTES;

/* When the decoders try execute_run_batch (the loops that hold it: lz4w::decode_chunk<., ., true>). A batch of the window
 * that was cut by its size with fewer than 24 sequences -- long sequences -- turns the attempts on for the batches behind
 * it. An attempt that finds the first sequences not of the shape at all (liblz4's fast compressor on the sorted-key column:
 * every other sequence is a 6-byte match far back) spaces the next ones out, 2, 4, 8, 16 batches of the window between them;
 * an attempt declined for a short run among the first sequences or a small batch does not (the int32 column: one run in
 * twenty is shorter than 16 bytes; 1 500 GB/s with those counted, 1 830 without: gpurun r6v, r6w). */
/* (Every batch tried, without a gate: default-compressed sorted keys 1 542 against 1 591-1 607 GB/s, Snappy of the same
 * 1 297 against 1 403-1 423: profiles/r06_ab_runs.jsonl, "gate variants", g0.) */
/* One uniform word (as a struct of three the compiler kept it in scratch memory): bit 0 = the last batch of the window took
 * few, long sequences (set at the start: the loops that hold the path get the chunks that shrank 8 x, their first batch is
 * tried); bits 4-6 = attempts in a row that found other shapes; bits 8-15 = batches of the window to let pass before the
 * next attempt. */
typedef uint32_t RunGate;
constexpr RunGate kRunGateInit = 1u;
__device__ __forceinline__ bool run_gate_open(RunGate g)
{
  return NVCOMP_LZW_RUNS && (g & 0xff01u) == 1u;
}
__device__ __forceinline__ RunGate run_gate_tried(RunGate g, uint32_t take, bool misfit)
{
  if (take) {
    return g & ~0x70u;
  }
  if (!misfit) {
    return g;
  }
  const uint32_t m = (g >> 4) & 7u, m1 = m < 4 ? m + 1 : 4u;
  return (g & 1u) | (m1 << 4) | ((1u << m1) << 8);
}
__device__ __forceinline__ RunGate run_gate_window_took(RunGate g, uint32_t take, uint32_t count)
{
  const uint32_t skip = g >> 8;
  return (g & 0x70u) | (take < 24u && take < count ? 1u : 0u) | ((skip ? skip - 1u : 0u) << 8);
}

constexpr uint32_t kRunMax = 60; /* sequences a batch: 32 bytes of joint a lane + the table of the sweep = the window's LDS */
constexpr bool kRunFits = kRunMax * 32 + 64 * 4 <= kOutLds; /* its slots and table live in the window's LDS (the callers assert it) */

/* mask of the low n bytes of a dword, n clamped to 0 .. 4 */
__device__ __forceinline__ uint32_t low_bytes_mask(int32_t n)
{
  const uint32_t c = n < 0 ? 0u : n > 4 ? 4u : (uint32_t)n;
  return c == 4 ? ~0u : (1u << (8u * c)) - 1u;
}

/* x as a ring of 16 bytes, rotated so that byte j moves to byte (j + sft) & 15 */
__device__ __forceinline__ void rotate16(uint32_t (&x)[4], uint32_t sft)
{
  const uint32_t bs = sft & 3u, ws = sft >> 2;
  uint32_t t[4];
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d) {
    t[d] = bs ? wave::align_bytes(x[d], x[(d + 3) & 3], 4u - bs) : x[d];
  }
#pragma unroll
  for (uint32_t d = 0; d < 4; ++d) {
    x[d] = ws == 0 ? t[d] : ws == 1 ? t[(d + 3) & 3] : ws == 2 ? t[(d + 2) & 3] : t[(d + 1) & 3];
  }
}

/* the last `off` bytes of the 16-byte value x (off = 1, 2, 4, 8, 16: uniform), repeated over all 16 */
__device__ __forceinline__ void repeat_tail16(uint32_t (&x)[4], uint32_t off)
{
  if (off == 8) {
    x[0] = x[2], x[1] = x[3];
  } else if (off <= 4) {
    uint32_t v = x[3];
    if (off == 2) {
      v = (v & 0xffff0000u) | (v >> 16);
    } else if (off == 1) {
      v >>= 24;
      v |= v << 8;
      v |= v << 16;
    }
    x[0] = v, x[1] = v, x[2] = v, x[3] = v;
  }
}

template <bool CHECKED>
__device__ __forceinline__ uint32_t execute_run_batch(
    const InRing& ir, OutWindow& ow, uint32_t out_cap, uint32_t& op, uint32_t n, const lz::Seq& s, bool& misfit)
{
  misfit = true; /* declined because the first sequences are not of this shape at all (RunGate spaces the attempts out) */
  /* uniform tests on the first sequence and the window: what a batch of any other kind of data pays for this path */
  uint32_t off = wave::read_lane(s.match_off, 0);
  if ((off - 1u >= 16u || (off & (off - 1u)) != 0) && n > 1) {
    /* the second sequence's instead: Snappy's literals are an element of their own in front of the copy; liblz4's fast
     * compressor starts a run of equal keys with a short match from far back (below: speculated) */
    off = wave::read_lane(s.match_off, 1);
  }
  if (off - 1u >= 16u || (off & (off - 1u)) != 0) {
    LZ_STAT("run_decl_period", 1);
    return 0;
  }
  /* the joints are whole aligned blocks: everything in front of the window's tail block must be in HBM (not so at the
   * start of a chunk whose buffer is not 16-byte aligned: the first batch goes through the window) */
  if (((ow.flushed + ow.align) & 15u) != 0 || op - ow.flushed >= 16u) {
    LZ_STAT("run_decl_window", 1);
    return 0;
  }
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  /* the leading sequences of this shape: the period of the first one, at most 16 literals (resident in the ring); a
   * sequence may be literals only (Snappy's literal elements; the run is then what follows it) or nothing at all (the
   * followers of a merged copy train) */
  /* ... and a match whose distance is a MULTIPLE of the period is taken for what it mostly is on such data -- the same
   * bytes the run would have produced there (equal keys: the new key's unchanged bytes copied from an earlier key) -- and
   * checked against the patterns further down */
  const bool weak = lane < n && (s.match_len == 0 || ((s.match_off & (off - 1u)) == 0 && s.match_off != 0 && s.match_len < kStreamMatch))
                    && (s.lit_len == 0 || (s.lit_len <= 16u && s.lit_src - ir.lo + s.lit_len <= ir.hi - ir.lo));
  const uint64_t not_weak = ~wave::ballot(weak) | (1ull << kRunMax);
  const uint32_t r0 = wave::ctz64(not_weak);
  if (r0 < kRunMin) {
    LZ_STAT("run_decl_lead", 1);
    return 0;
  }
  misfit = false; /* what declines from here on is this batch's bad luck: a short run among the first, a small batch */
  const bool in0 = lane < r0;
  const uint32_t len = in0 ? s.lit_len + s.match_len : 0u;
  const uint32_t incl = wave::scan_add_inclusive(len);
  /* a sequence without literals goes on with the run in front of it: heads are the others; a head's run ends where the
   * next head's literals start */
  const bool head = in0 && (lane == 0 || s.lit_len != 0);
  uint64_t heads = wave::ballot(head);
  const uint64_t hx = heads | (1ull << r0);
  const uint64_t above = lane < 63 ? hx >> (lane + 1) : 0ull;
  const uint32_t next_head = above ? lane + 1 + wave::ctz64(above) : r0;
  const uint32_t L = op + incl - len;      /* where the sequence's literals go */
  const uint32_t M = L + s.lit_len;        /* where its match starts */
  uint32_t E = 0; /* where the sequence's (merged) run ends */
  /* How many of the r1 leading sequences a batch can be: its last run must be 16 bytes long -- the window restarts with its
   * pattern as the last 16 bytes of the output. (Runs in between may be of any length: the joints of sequences that meet in
   * one block share it, below. The first versions ended a batch at a run shorter than 16 bytes, then at one without a block
   * boundary in it: int32 column 1 750-1 810, then 2 370-2 570 GB/s.) */
  auto settle = [&](uint32_t r1) -> uint32_t {
    const uint32_t nh = next_head < r1 ? next_head : r1;
    E = op + wave::shuffle(incl, (nh - 1u) & 63u);
    uint32_t r = r1;
    for (uint32_t i = 0; i < 4 && r >= kRunMin; ++i) {
      const uint32_t last_head = 63u - (uint32_t)__builtin_clzll(heads & ((1ull << r) - 1ull)); /* lane 0 is a head */
      if (wave::read_lane(E - M, last_head) >= 16u) {
        return r;
      }
      r = last_head;
    }
    return 0;
  };
  uint32_t R = settle(r0);
  if (R < kRunMin) {
    LZ_STAT("run_decl_short", 1);
    return 0;
  }
  heads &= (1ull << R) - 1ull;
  uint32_t total = wave::read_lane(incl, R - 1);
  {
    /* the batch's end is the only output test; the first match must have its period in front of it (every other one
     * starts behind it), in the window if the literals do not cover it */
    const uint32_t m0 = op + wave::read_lane(s.lit_len, 0);
    if (op + total > out_cap || m0 < off || (m0 - op < off && m0 - off < ow.valid_lo)) {
      LZ_STAT("run_decl_first", 1);
    return 0;
    }
    /* short runs and small batches are as well off in the window */
    if (total < 64u * wave::popc64(heads) || total < kRunMinBytes) {
      LZ_STAT("run_decl_small", 1);
    return 0;
    }
  }
  LZW_T(4);
  LZ_STAT("run_batches", 1);
  LZ_STAT("run_seqs", R);
  LZ_STAT("run_heads", wave::popc64(heads));
  LZ_STAT("run_bytes", total);

  /* the 16 bytes in front of the batch by address residue: the window's tail block up to op, the block before behind it */
  uint32_t qi[4];
  {
    const uint32_t cop = op + ow.align; /* "coordinates": position + align, congruent to the address modulo 16; window index = coordinate - wbase */
    const uint32_t fl = cop & ~15u, t = cop & 15u;
    const wave::u32x4 w1 = *(const wave::u32x4*)(ow.win + (fl - ow.wbase));
    wave::u32x4 w0 = {0, 0, 0, 0};
    if (fl - ow.wbase >= 16u) {
      w0 = *(const wave::u32x4*)(ow.win + (fl - 16u - ow.wbase));
    }
    const uint32_t a1[4] = {w1.x, w1.y, w1.z, w1.w}, a0[4] = {w0.x, w0.y, w0.z, w0.w};
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      const uint32_t m = low_bytes_mask((int32_t)t - (int32_t)(4 * d));
      qi[d] = (a1[d] & m) | (a0[d] & ~m);
    }
  }
  /* a lane's contribution: its last 16 literal bytes (those it has: the others masked out), their last `off` repeated,
   * rotated to the address residues of the bytes in front of its match */
  uint32_t q[4], qm[4];
  {
    const uint32_t e = s.lit_src + s.lit_len;
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      q[d] = ld32(ir.ring + ((e - 16u + 4u * d) & (kInRing - 1)));
      qm[d] = ~low_bytes_mask(16 - (int32_t)(4 * d) - (int32_t)s.lit_len);
    }
    repeat_tail16(q, off);
    repeat_tail16(qm, off);
    const uint32_t sft = (M + ow.align) & 15u;
    rotate16(q, sft);
    rotate16(qm, sft);
    if (lane == 0) {
      /* the first sequence inherits from the output in front of the batch: its last `off` bytes, repeated like a run */
      uint32_t h[4] = {qi[0], qi[1], qi[2], qi[3]};
      const uint32_t t = (op + ow.align) & 15u;
      rotate16(h, (16u - t) & 15u); /* byte j = position op - 16 + j */
      repeat_tail16(h, off);
      rotate16(h, t);
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) {
        q[d] = (q[d] & qm[d]) | (h[d] & ~qm[d]);
        qm[d] = ~0u;
      }
    }
#pragma unroll
    for (uint32_t d = 0; d < 4; ++d) {
      wave::scan_last_writer(q[d], qm[d]);
    }
  }
  /* ---- the speculated matches (distance a multiple of the period, not the period): each one's source bytes must be what
   * the run's pattern gives at its destination. The source lies in a run of this batch (then its bytes are that run's
   * pattern: compare the two patterns at the residues the match covers) or, up to 16 bytes, in the output in front of the
   * batch (one 16-byte load). A match that fails, or whose source is anywhere else, ends the batch in front of it: every
   * pattern below it is right whatever comes behind (the scan runs upwards), and nothing has been written yet. ---- */
  {
    const bool spec = lane < R && s.match_len != 0 && s.match_off != off;
    if (wave::ballot(spec)) {
      const uint32_t sp = M - s.match_off; /* wraps for an offset beyond the output: fails every test below */
      const uint32_t m = s.match_len;
      const uint32_t sft = (M + ow.align) & 15u;
      /* (a) in this batch: the sequence t whose output holds sp (the L are ascending; lanes behind the batch hold its end) */
      uint32_t t = 0;
#pragma unroll
      for (uint32_t step = 32; step != 0; step >>= 1) {
        const uint32_t c = t + step;
        t = wave::shuffle(L, c) <= sp ? c : t;
      }
      const uint32_t mt = wave::shuffle(M, t), et = wave::shuffle(E, t);
      bool ok = spec && sp >= op && sp + off >= mt && sp + m <= et;
      {
        uint32_t cover[4];
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
          cover[d] = low_bytes_mask((int32_t)m - (int32_t)(4 * d)); /* the first min(m, 16) bytes ... */
        }
        rotate16(cover, sft); /* ... at the residues of the match's destination */
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
          diff |= (wave::shuffle(q[d], t) ^ q[d]) & cover[d];
        }
        ok = ok && diff == 0;
      }
      /* (b) in HBM in front of the batch, 16 bytes at most, the load inside the chunk's buffer */
      const bool hbm = spec && !ok && m <= 16u && sp <= ow.flushed && m <= ow.flushed - sp && out_cap >= 16u && sp <= out_cap - 16u;
      if (wave::ballot(hbm)) {
        uint32_t want[4] = {q[0], q[1], q[2], q[3]};
        rotate16(want, (16u - sft) & 15u); /* byte i = the pattern's byte at the destination's position M + i */
        wave::u32x4 got = {0, 0, 0, 0};
        if (hbm) {
          got = wave::gload_u32x4(ow.out + sp);
        }
        const uint32_t g[4] = {got.x, got.y, got.z, got.w};
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
          diff |= (g[d] ^ want[d]) & low_bytes_mask((int32_t)m - (int32_t)(4 * d));
        }
        ok = ok || (hbm && diff == 0);
      }
      const uint64_t failed = wave::ballot(spec && !ok);
      LZ_STAT("run_spec", wave::popc64(wave::ballot(spec)));
      LZ_STAT("run_spec_failed", wave::popc64(failed));
      if (failed) {
        /* the batch ends in front of the first one; its last run may have become short, the batch small */
        R = settle(wave::ctz64(failed));
        if (R < kRunMin) {
          misfit = true;
          LZ_STAT("run_decl_spec", 1);
          return 0;
        }
        heads &= (1ull << R) - 1ull;
        total = wave::read_lane(incl, R - 1);
        if (total < 64u * wave::popc64(heads) || total < kRunMinBytes) {
          misfit = true;
          LZ_STAT("run_decl_spec", 1);
          return 0;
        }
      }
    }
  }
  LZW_T(16); /* runs: the patterns */
  /* ---- joints: the blocks that are not all one run, assembled on a canvas in LDS (the window's, which nothing else needs
   * meanwhile). A head's joint are the blocks from its first literal to the first whole block of its run, two at most;
   * when its run is too short to reach the next block boundary the next head's joint starts in the same block, and the
   * two (or more) share that block of the canvas. Every byte of the canvas has one writer -- the head whose literals or
   * whose run it belongs to (a run's bytes: its pattern, masked) -- so the writes are ORs into a zeroed canvas and plain
   * stores of the literals. ---- */
  uint8_t* const gbase = ow.out - ow.align; /* coordinate 0 */
  const bool jlane = wave::lane_in(heads);
  {
    const uint32_t cl = L + ow.align, cm = M + ow.align; /* coordinates of the literals and of the run */
    const uint32_t a = cl & 15u;                         /* where the literals start in the joint's first block */
    const uint32_t b0 = cl >> 4, b1 = (cm + 15u) >> 4;   /* the joint's blocks [b0, b1) */
    const uint32_t nj = jlane ? b1 - b0 : 0u;
    /* a head whose first block is the last block of the joint below shares it (the b1 are ascending: the running maximum is
     * the nearest one below) */
    const uint32_t below_b1 = wave::prev_lane(wave::scan_max_inclusive(nj ? b1 : 0u));
    const uint32_t shared = nj != 0 && below_b1 == b0 + 1u ? 1u : 0u;
    /* The common batch (the sorted-key column: every run hundreds of bytes) has no shared block and no run that ends inside
     * its own joint: every head then owns the two blocks at 2 x its lane, writes them whole -- the pattern below up to its
     * literals, its own pattern behind -- and its literals over them: a sixth of the instructions of the general case. */
    const bool plain = wave::ballot(jlane && (shared != 0 || ((E + ow.align) >> 4) < b1)) == 0;
    const uint32_t cv = plain ? 2u * lane : wave::scan_add_inclusive(nj - shared) - nj; /* the joint's first block on the canvas */
    uint32_t* const canvas = (uint32_t*)ow.win;
    wave::sync(); /* the window's blocks have been read */
    if (plain) {
      wave::u32x4 w0, w1;
      uint32_t x[4];
#pragma unroll
      for (uint32_t d = 0; d < 4; ++d) {
        const uint32_t below = wave::prev_lane(q[d]);
        const uint32_t m = low_bytes_mask((int32_t)a - (int32_t)(4 * d));
        x[d] = ((lane == 0 ? qi[d] : below) & m) | (q[d] & ~m);
      }
      w0.x = x[0], w0.y = x[1], w0.z = x[2], w0.w = x[3];
      w1.x = q[0], w1.y = q[1], w1.z = q[2], w1.w = q[3];
      if (lane < kRunMax) {
        *(wave::u32x4*)(ow.win + 32u * lane) = w0;
        *(wave::u32x4*)(ow.win + 32u * lane + 16) = w1;
      }
    } else {
      const wave::u32x4 zero = {0, 0, 0, 0};
      if (lane < kRunMax) {
        *(wave::u32x4*)(ow.win + 32u * lane) = zero;
        *(wave::u32x4*)(ow.win + 32u * lane + 16) = zero;
      }
    }
    wave::sync();
    const uint32_t next_cv = plain ? 0u : wave::shuffle(cv, next_head & 63u); /* where the next head's joint starts */
    if (jlane && !plain) {
      /* my run's bytes inside my own joint: from the run's start to the joint's end or the run's, whichever is first */
      const uint32_t run_lo = a + s.lit_len;          /* relative to my first block: 0 .. 31 */
      const uint32_t run_hi = E + ow.align - 16u * b0; /* where my run ends, relative to my first block */
      const uint32_t hi = run_hi < 16u * nj ? run_hi : 16u * nj;
#pragma unroll
      for (uint32_t d = 0; d < 8; ++d) {
        const uint32_t m = low_bytes_mask((int32_t)hi - (int32_t)(4 * d)) & ~low_bytes_mask((int32_t)run_lo - (int32_t)(4 * d));
        if (m != 0 && 4 * d < 16u * nj) {
          wave::lds_or(canvas + 4u * cv + d, q[d & 3] & m);
        }
      }
      /* ... and in front of the next head's literals, when those start in a block of their own */
      const uint32_t ce = E + ow.align;
      if (next_head < R && (ce >> 4) >= b1 && (ce & 15u) != 0) {
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
          const uint32_t m = low_bytes_mask((int32_t)(ce & 15u) - (int32_t)(4 * d));
          if (m != 0) {
            wave::lds_or(canvas + 4u * next_cv + d, q[d] & m);
          }
        }
      }
      /* the first joint's first block starts with the output in front of the batch (the window's tail block) */
      if (lane == 0 && nj != 0) {
#pragma unroll
        for (uint32_t d = 0; d < 4; ++d) {
          const uint32_t m = low_bytes_mask((int32_t)a - (int32_t)(4 * d));
          if (m != 0) {
            wave::lds_or(canvas + 4u * cv + d, qi[d] & m);
          }
        }
      }
    }
    if (jlane) {
      /* the literals */
      uint8_t* at = ow.win + 16u * cv + a;
      if (s.lit_len >= 4) {
        const uint32_t last = s.lit_len - 4;
        uint32_t data[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
          const uint32_t o = 4 * i < last ? 4 * i : last;
          data[i] = ld32(ir.ring + ((s.lit_src + o) & (kInRing - 1)));
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
          const uint32_t o = 4 * i < last ? 4 * i : last;
          lz::st_u32(at + o, data[i]);
        }
      } else if (s.lit_len != 0) {
        at[0] = ir.ring[s.lit_src & (kInRing - 1)];
        if (s.lit_len > 1) {
          at[1] = ir.ring[(s.lit_src + 1) & (kInRing - 1)];
        }
        if (s.lit_len > 2) {
          at[2] = ir.ring[(s.lit_src + 2) & (kInRing - 1)];
        }
      }
    }
    /* the table of the sweep: one word a head, in address order -- its first block's number in the batch (14 bits), how many
     * of its blocks are joint blocks (2), where they are on the canvas (7), its lane (6: whose pattern the blocks behind
     * the joint hold); unused entries compare above every block. Heads that start in one block have equal block numbers:
     * the search below takes the last of them, whose canvas block is the shared one and whose run goes on behind it. */
    uint32_t* tab = (uint32_t*)(ow.win + 32u * kRunMax);
    tab[lane] = ~0u;
    wave::sync();
    if (jlane) {
      const uint32_t blk = b0 - ((op + ow.align) >> 4);
      tab[wave::prefix_popc(heads)] = (blk << 15) | (nj << 13) | (cv << 6) | lane;
    }
    wave::sync();
  }
  LZW_T(17); /* runs: the joints */
  /* ---- the sweep: every whole block of the batch, in address order, 1 KiB a store instruction. A lane finds the head its
   * block belongs to (binary search of the table) and takes the block from the canvas or that head's pattern from its
   * lane. (Stores run by run -- a run's ~25 blocks an instruction, the joints scattered -- left the memory pipe the bound:
   * 2 550 GB/s on the sorted-key column, two thirds of the time in that loop: gpurun r6q, r6r.) ---- */
  {
    const uint32_t* tab = (const uint32_t*)(ow.win + 32u * kRunMax);
    const uint32_t c0 = (op + ow.align) & ~15u;
    const uint32_t nblk = (((op + total + ow.align) & ~15u) - c0) >> 4;
    for (uint32_t base = 0; base < nblk; base += 64) {
      const uint32_t bi = base + lane;
      uint32_t lo = 0;
#pragma unroll
      for (uint32_t step = 32; step != 0; step >>= 1) {
        const uint32_t c = lo + step;
        lo = (tab[c] >> 15) <= bi ? c : lo;
      }
      const uint32_t key = tab[lo];
      const uint32_t k = key & 63u, jb = bi - (key >> 15);
      const bool joint = jb < ((key >> 13) & 3u);
      wave::u32x4 x;
      x.x = wave::shuffle(q[0], k), x.y = wave::shuffle(q[1], k), x.z = wave::shuffle(q[2], k), x.w = wave::shuffle(q[3], k);
      if (joint) {
        x = *(const wave::u32x4*)(ow.win + 16u * (((key >> 6) & 127u) + jb));
      }
      if (bi < nblk) {
        wave::gstore_u32x4_aligned(gbase + c0 + 16u * bi, x); /* (non-temporal: 3 440 against 3 600-3 700 GB/s) */
      }
    }
  }
  LZW_T(18); /* runs: the bodies */
  /* ---- the window restarts behind the batch: the last run's pattern is its history, its last partial block the tail
   * that waits for the next flush ---- */
  {
    wave::u32x4 ql;
    ql.x = wave::read_lane(q[0], R - 1), ql.y = wave::read_lane(q[1], R - 1);
    ql.z = wave::read_lane(q[2], R - 1), ql.w = wave::read_lane(q[3], R - 1);
    wave::sync();
    op += total;
    const uint32_t nbase = (op - 16u) & ~15u;
    const uint32_t fl = (op + ow.align) & ~15u;
    const uint32_t i0 = fl - 16u - nbase; /* 0 or 16 */
    if (lane == 0) {
      *(wave::u32x4*)(ow.win + i0) = ql;
      *(wave::u32x4*)(ow.win + i0 + 16) = ql;
    }
    wave::sync(); /* and later far reads of this wave see the stores above */
    ow.wbase = nbase;
    ow.valid_lo = op - 16u;
    ow.flushed = fl - ow.align;
  }
  LZW_T(19); /* runs: the window restart */
  return R;
}

} // namespace lzw
