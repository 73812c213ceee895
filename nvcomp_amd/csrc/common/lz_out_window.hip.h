/*
 * common/lz_out_window.hip.h -- the output window: a linear LDS window over the most recent output, flushed to HBM
 * in aligned 16-byte blocks (common/lz_window.hip.h).
 */
#pragma once

#include "common/lz_ring.hip.h"

namespace lzw {

/* ---- output window --------------------------------------------------------- */

struct OutWindow
{
  uint8_t* win;      /* LDS, kOutLds bytes, 16-byte aligned */
  uint8_t* out;      /* chunk output pointer in HBM (uniform) */
  uint32_t align;    /* out & 15: window index = position - wbase + align */
  uint32_t falign;   /* out & (kFlushAlign - 1): position + falign is address-congruent modulo kFlushAlign */
  uint32_t wbase;    /* output position of window index `align` (multiple of 16) */
  uint32_t valid_lo; /* positions >= valid_lo (and < op) are present in the window */
  uint32_t flushed;  /* positions < flushed are in HBM; valid_lo <= flushed <= op, op - flushed < 16 between batches */
};

__device__ __forceinline__ void out_init(OutWindow& w, uint8_t* out, uint8_t* lds)
{
  w.win = lds;
  w.out = out;
  w.align = (uint32_t)((uintptr_t)out & 15u);
  w.falign = (uint32_t)((uintptr_t)out & (kFlushAlign - 1));
  w.wbase = 0;
  w.valid_lo = 0;
  w.flushed = 0;
}

__device__ __forceinline__ uint8_t* out_at(const OutWindow& w, uint32_t pos)
{
  return w.win + (pos - w.wbase + w.align);
}

/* Slide the window so that the batch's `need` bytes (at most kBatchMax) fit after position op. (Until round 6 it made room for
 * kBatchMax whatever the batch produced, i.e. slid in front of every batch: a batch of text is ~700 bytes, the slide two
 * syncs and a copy: profiles/r06_ab_runs.jsonl, "roomk".) What stays behind without a slide -- up to 1.4 KiB of flushed
 * output -- is history: execute_window_batch copies a short match whose whole source lies in [valid_lo, flushed) in LDS
 * instead of fetching it (a twelfth of the mix's far matches: scripts/window_history_model.py). */
__device__ __forceinline__ void out_make_room(OutWindow& w, uint32_t op, uint32_t need)
{
  if (op - w.wbase + w.align + need <= kOutWin) {
    return;
  }
  /* history kept: kKeep bytes. (As much as the coming batch leaves room for, up to 64 .. 1 024 bytes or all of it, with the
   * matches into it copied in LDS: more slides and longer ones cost more than the requests they save, LZ4 mix 726 GB/s
   * with 32 bytes, 721 with 512, 709 with 1 024, 692 with all that fits: profiles/ab_window_history.jsonl. The round-6
   * measurement of the same, r6ax, could not see history at all: every flushed source was fetched then.) */
  uint32_t keep_from = op > kKeep ? op - kKeep : 0;
  if (keep_from > w.flushed) {
    keep_from = w.flushed; /* the tail that waits for its 16-byte block to fill up always stays (kKeep < 16: no history at all) */
  }
  if (keep_from < w.valid_lo) {
    keep_from = w.valid_lo;
  }
  /* wbase stays a multiple of 16 so that window index and HBM address agree mod 16 */
  const uint32_t new_base = keep_from & ~15u;
  const uint32_t shift = new_base - w.wbase; /* multiple of 16 */
  if (shift == 0) {
    return;
  }
  const uint32_t len = op - new_base + w.align; /* window bytes still needed, from index 0 */
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  for (uint32_t base = 0; base < len; base += 1024) {
    const uint32_t i = base + lane * 16;
    wave::u32x4 t = {0, 0, 0, 0};
    if (i < len) {
      t = *(const wave::u32x4*)(w.win + shift + i);
    }
    wave::sync(); /* every lane has read before any lane overwrites */
    if (i < len) {
      *(wave::u32x4*)(w.win + i) = t;
    }
    wave::sync();
  }
  w.wbase = new_base;
  if (w.valid_lo < new_base) {
    w.valid_lo = new_base;
  }
}

/* Flush window bytes of output positions [from, to) to HBM: byte stores up to
 * the first 16-byte boundary, aligned 16-byte lane stores, byte stores for the tail. */
__device__ __forceinline__ void out_flush_range(const OutWindow& w, uint32_t from, uint32_t to)
{
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  const uint32_t a_from = from + w.align; /* absolute-address-congruent coordinates */
  const uint32_t a_to = to + w.align;
  uint32_t body_lo = (a_from + 15u) & ~15u;
  uint32_t body_hi = a_to & ~15u;
  if (body_lo > body_hi) { /* everything inside one 16-byte block */
    body_lo = a_to;
    body_hi = a_to;
  }
  uint8_t* gout = w.out - w.align;            /* so that gout + a == out + pos */
  const uint8_t* lwin = w.win - w.wbase;      /* so that lwin + a == win + (pos - wbase + align) */
  if (lane < body_lo - a_from) {
    wave::gstore_u8(gout + a_from + lane, lwin[a_from + lane]);
  }
  for (uint32_t a = body_lo + lane * 16; a < body_hi; a += 1024) {
    wave::gstore_u32x4_aligned(gout + a, *(const wave::u32x4*)(lwin + a));
  }
  if (lane < a_to - body_hi) {
    wave::gstore_u8(gout + body_hi + lane, lwin[body_hi + lane]);
  }
}

/* Per-batch flush: only whole 16-byte blocks go out; the last op % 16 bytes wait in the window for the
 * next batch (sub-dword global stores cost a memory request each). After the first flush `flushed` sits on
 * a 16-byte boundary of the output address, so a batch issues aligned 16-byte stores only. */
__device__ __forceinline__ void out_flush(OutWindow& w, uint32_t op_end)
{
  /* address-congruent coordinate of the end of the last whole block (of kFlushAlign bytes: a multiple of 16) */
  const uint32_t f_to = (op_end + w.falign) & ~(kFlushAlign - 1);
  if (f_to > w.flushed + w.falign) {
    out_flush_range(w, w.flushed, f_to - w.falign);
    w.flushed = f_to - w.falign;
  }
}

/* After a sequence was streamed HBM -> HBM behind the window's back (the callers' `big` path): restart the window at op. */
__device__ __forceinline__ void restart_window(OutWindow& w, uint32_t op)
{
  w.wbase = op & ~15u;
  w.valid_lo = op;
  w.flushed = op;
}

/* Everything up to op_end, tail bytes included (end of the chunk, or before HBM-to-HBM copies). */
__device__ __forceinline__ void out_flush_all(OutWindow& w, uint32_t op_end)
{
  if (op_end > w.flushed) {
    out_flush_range(w, w.flushed, op_end);
    w.flushed = op_end;
  }
}

} // namespace lzw
