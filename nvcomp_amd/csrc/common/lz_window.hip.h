/*
 * common/lz_window.hip.h -- LDS-staged, sequence-parallel LZ77 batch executor
 * shared by the LZ4 and Snappy decoders (one wavefront per chunk).
 *
 * Measured on MI355X (profiles/archive/r01_v1_direct_pmc.json): decoding straight to
 * HBM leaves a wave waiting on memory 62 % of its cycles -- every literal/match
 * step is a dependent global load->store round trip -- and reads 10x the
 * algorithmic bytes (partial-line writes and far match sources miss the L2).
 * So everything a sequence can depend on is kept in the CU's LDS:
 *
 *   input ring   (kInRing bytes)  the compressed stream, loaded from HBM in
 *                1 KiB blocks of 16-byte lane loads, ahead of the token chase;
 *   output window (kOutWin bytes) a linear window over the most recent output.
 *                Literals and matches are assembled here; a match whose source
 *                is still inside the window never touches HBM. After every
 *                batch the new bytes are flushed to HBM with 16-byte aligned,
 *                fully coalesced stores, and when the window fills up its last
 *                kKeep bytes slide to the front.
 *
 * Only matches that reach further back than the window ("far") read HBM, all of
 * a batch's far reads being issued together before the LDS work starts.
 *
 * This file is the batch executor, execute_window_batch. Its parts are headers of their own: lz_ring.hip.h (the
 * geometry, the phase clock, the input ring), lz_out_window.hip.h, lz_copy.hip.h and lz_stream.hip.h, included here;
 * lz_chase.hip.h (the token chase) and lz_run_batch.hip.h (the run executor), included by the decoders that use them.
 */
#pragma once

#include "common/lz_ring.hip.h"
#include "common/lz_out_window.hip.h"
#include "common/lz_copy.hip.h"
#include "common/lz_stream.hip.h"

namespace lzw {

/* The first `take` of `count` sequences in hand are done: the others move down to lane 0, and the lanes behind them
 * become EMPTY sequences again (execute_window_batch relies on that instead of masking by the count). */
__device__ __forceinline__ void drop_front(lz::Seq& s, uint32_t take, uint32_t count)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  const uint32_t from = (lane + take) & 63u;
  const bool keep = lane < count - take;
  const uint32_t a = wave::shuffle(s.lit_src, from), b = wave::shuffle(s.lit_len, from);
  const uint32_t c = wave::shuffle(s.match_off, from), d = wave::shuffle(s.match_len, from);
  s.lit_src = keep ? a : 0u;
  s.lit_len = keep ? b : 0u;
  s.match_off = keep ? c : 0u;
  s.match_len = keep ? d : 0u;
}

/*
 * Execute the first sequences of a parsed batch inside the window. Lane k owns
 * sequence k (k < n, n >= 1); lanes >= n hold EMPTY sequences (lit_len = match_len = 0:
 * the callers keep it so), lit positions are virtual positions in the input ring's
 * coordinate system. Consumes as many leading sequences as fit kBatchMax output
 * bytes (at least one unless the first one alone is larger: then `big` is set
 * and nothing is consumed). Returns the number of sequences consumed and adds
 * the bytes produced to op.
 *
 * Written for the scalar unit as much as for the vector unit (they are equally busy in this kernel): every
 * && / || of two lane conditions is a scalar instruction on 64-bit masks, so ranges are tested with one unsigned
 * compare ((x - lo) <= hi - lo), conditions that grow with the lane are tested once for the wave, and nothing is
 * masked that the callers' invariant already zeroes.
 */

/* A batch's whole blocks are written to HBM at its end. (Round 6 tried writing them only when the window has to slide --
 * every third or fourth batch of text, 2 KiB at a time; nothing needs them earlier: LZ4 mix 683 -> 686 GB/s, Snappy mix
 * 501 -> 484, float32 column 412 -> 400. DESIGN.md, "retired switches".) */
/* HISTORY: a short match whose whole source the window still holds is copied in LDS, not fetched (below). */
template <bool CHECKED, bool RING_LITERALS = false, bool HISTORY = false>
__device__ __forceinline__ uint32_t execute_window_batch(
    InRing& ir, OutWindow& ow, uint32_t out_cap, uint32_t& op, uint32_t n, const lz::Seq& s, uint32_t& err, bool& big)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  const uint32_t len = s.lit_len + s.match_len;
  const uint32_t incl = wave::scan_add_inclusive(len);
  big = false;

  /* leading sequences whose cumulative output fits one batch (a length is < 2^31: the first sum above kBatchMax has
   * not wrapped, whatever the sums behind it do) */
  /* ... and a sequence with a long literal run or a long match is not for the window at all (stream_sequence) */
  const uint64_t over = wave::ballot(incl > kBatchMax)
                        | (RING_LITERALS ? 0ull : wave::ballot(s.lit_len >= kStreamLit) | wave::ballot(s.match_len >= kStreamMatch));
  uint32_t take = over ? wave::ctz64(over) : 64u;
  take = take < n ? take : n;
  if (take == 0) {
    big = true;
    return 0;
  }
  /* The batch's lanes as a MASK, and every predicate of the batch below as a mask too: a ballot of one compare of the
   * sequence's own fields (the compare itself writes the mask), cut to the batch on the scalar unit. A lane takes its
   * predicate from the mask (wave::lane_in: the mask is the exec mask of the branch). Balloted from lengths that were
   * zeroed outside the batch first -- `mine ? len : 0` -- every one of these was an && of two lane conditions, which
   * the compiler joins on the scalar unit and then turns into a lane boolean and back (common/lz_copy.hip.h, steps_for). */
  const uint64_t mine_mask = take < 64 ? (1ull << take) - 1 : ~0ull;
  const uint32_t total = wave::read_lane(incl, take - 1);
  const uint32_t lit_dst = op + incl - len;
  const uint32_t match_dst = lit_dst + s.lit_len;
  /* (used by lanes of the batch only) */
  const uint32_t my_lit = s.lit_len;
  const uint32_t my_match = s.match_len;
  const uint64_t match_mask = wave::ballot(s.match_len != 0) & mine_mask;
  /* the length classes, once per batch: what steps_for asks of the far store, of the literal copy and of every near round */
  const uint64_t match_gt16 = wave::ballot(s.match_len > 16), match_gt8 = wave::ballot(s.match_len > 8);

  if (CHECKED) {
    /* the sums grow with the lane: the batch's end is the only output test (op <= out_cap <= 2^26, total <= kBatchMax);
     * offset 0 wraps to the largest value, so one compare covers "0 or beyond the produced output" */
    const bool bad_out = op + total > out_cap;
    const uint64_t any_off = match_mask & wave::ballot(s.match_off - 1 >= match_dst);
    if (bad_out || any_off) {
      err |= (bad_out ? lz::kErrOutput : 0u) | (any_off ? lz::kErrOffset : 0u);
      return 0;
    }
  }

  LZ_STAT("batches", 1);
  LZ_STAT("seqs", take);
  LZ_STAT("bytes", total);
  LZW_T(4);
  out_make_room(ow, op, total);
  LZW_T(5);

  /* ---- far matches: sources the window no longer holds, read from HBM ---- */
  const uint32_t match_src = match_dst - s.match_off;
  /* DEFLATE (RING_LITERALS) has matches of THREE bytes -- a sixth of all matches of a zlib stream, and as whole-wave
   * copies, one after the other, they were 18 % of that decoder's time (phase clock, profiles/archive/r03_deflate_phases.json) */
  constexpr uint32_t kMinShort = RING_LITERALS ? 3 : 4;
  /* the data comes with one or two 16-byte loads that start up to 3 bytes IN FRONT of the source -- at source - (the
   * destination's address & 3), so that the dwords arrive as the window's aligned dwords: far_store_aligned -- and must
   * stay inside the chunk's buffer: 3 <= match_src <= out_cap - 32 in one unsigned compare. (A source in the first 3
   * or the last 32 bytes of the buffer, or a wrapped one of a corrupt unchecked stream, takes the cooperative path below.) */
  const uint64_t short_mask = wave::ballot(s.match_len - kMinShort <= kMatchShort - kMinShort) & mine_mask; /* kMinShort .. kMatchShort */
  /* near: a short match with a period of 4 or more whose source STARTS in what the window holds, [valid_lo, op): copied
   * in LDS by its own lane, in the rounds below */
  const uint64_t near_mask = short_mask & wave::ballot(match_src >= ow.valid_lo) & wave::ballot(s.match_off >= 4);
  /* A source that is flushed to its end is final, and in the output buffer. With HISTORY, where the window holds all of it
   * as well -- the 32 bytes a slide kept and whatever the batches since have added, up to 1.4 KiB (out_make_room) -- the
   * match is a near one that is ready in the first round, and costs no memory request: only the others are far. (A source
   * that straddles valid_lo starts in front of it: far.) That is a twelfth of the LZ4 mix's far matches and a fifth of
   * the Snappy mix's (scripts/window_history_model.py, scripts/emu_match_rounds.py), and it pays only where the card's
   * gather rate is what bounds the launch -- the one-wave LZ4 kernel on 65 536 chunks of the mix, 714 -> 728 GB/s: for a
   * wave that waits for its other far loads anyway, the copy in LDS is work on top. Snappy mix 547 -> 520 GB/s, 4 096 chunks
   * of the LZ4 mix (two waves a chunk) 388 -> 373, the same with these matches copied beside the far store instead of
   * in the rounds: profiles/ab_window_history.jsonl. So the decoders say which they are. */
  const uint64_t final_mask = short_mask & wave::ballot(match_src + s.match_len <= ow.flushed);
  const uint64_t hist_mask = HISTORY ? final_mask & near_mask : 0ull;
  const uint64_t far_mask = out_cap >= 35 ? final_mask & ~hist_mask & wave::ballot(match_src - 3u <= out_cap - 35u) : 0ull;
  const bool far_lane = wave::lane_in(far_mask);
  /* where the destination sits in its aligned dword: the window is 16-byte aligned and wbase a multiple of 16 (out_at) */
  const uint32_t far_a = (match_dst + ow.align) & 3u;
  /* (no zero fill: far_store_aligned is called by the far lanes only, and of a match of up to 16 bytes it stores nothing
   * that comes from far_data[4..7]) */
  uint32_t far_l4 = LZW_UNSET_U32;
  uint32_t far_data[8] = {LZW_UNSET_U32, LZW_UNSET_U32, LZW_UNSET_U32, LZW_UNSET_U32,
                          LZW_UNSET_U32, LZW_UNSET_U32, LZW_UNSET_U32, LZW_UNSET_U32};
  const uint32_t far_steps = steps_for(far_mask, match_gt16, match_gt8);
  if (far_lane) {
    /* (folded onto the chunk's first KiB -- L2-resident lines -- the kernel gains 4-8 %: profiles/r06_far_ablate.jsonl;
     * DESIGN.md, "retired switches") */
    const uint32_t src_at = match_src - far_a;
    /* every address is the chunk's (uniform) base plus a 32-bit lane offset: the loads take the scalar-base form, no
     * 64-bit address is built per lane (3 <= match_src, match_src + my_match <= flushed <= out_cap < 2^31: the sums do
     * not wrap) */
    const uint8_t* src = ow.out + src_at;
    /* A scattered load costs the CU's address unit a slot per lane whatever its width (profiles/archive/r02_decode_phases.json:
     * issuing 3-9 dword loads per batch was 11 % of the wave's time): 16 bytes per load, two loads at most, plus the
     * match's last dword. */
    const wave::u32x4 f0 = wave::gload_u32x4(src);
    far_data[0] = f0.x, far_data[1] = f0.y, far_data[2] = f0.z, far_data[3] = f0.w;
    if (my_match > 16) {
      const wave::u32x4 f1 = wave::gload_u32x4(ow.out + (src_at + 16u));
      far_data[4] = f1.x, far_data[5] = f1.y, far_data[6] = f1.z, far_data[7] = f1.w;
    }
    /* the match's last four bytes; of a three-byte match: the byte in front of it (match_src >= 3), then its three.
     * (Taken out of the first load where the match ends within it -- a select among its dwords and a shift, seven vector
     * instructions in place of this load for those lanes -- the mix LOSES 1.7 %: profiles/ab_window_masks.jsonl, ABDE.) */
    far_l4 = wave::gload_u32(ow.out + (match_src + my_match - 4u));
  }

  LZW_T(11); /* far classification + load issue */
  /* ---- literals ---- */
  {
    uint8_t* dst = out_at(ow, lit_dst);
    /* a run of 1 .. kLitShort bytes that the ring holds is copied by its own lane (a position in front of the resident
     * range wraps to a huge value: one compare) */
    const uint64_t own_mask = wave::ballot(s.lit_len - 1 < kLitShort) & wave::ballot(s.lit_src - ir.lo + s.lit_len <= ir.hi - ir.lo) & mine_mask;
    const uint64_t word_mask = wave::ballot(s.lit_len >= 4);
    const bool lit_lane = wave::lane_in(own_mask & word_mask);
    /* the ring wraps at kInRing; its 16-byte mirror covers a dword that starts before the end. A run that ends inside
     * the mirror is read from ONE base address (clamped offsets added, as everywhere); only when some lane's run goes on
     * behind the mirror -- one run in a hundred -- the wave takes the loop that wraps every step's address by itself. */
    const uint32_t lit_steps = steps_for(own_mask & word_mask, wave::ballot(s.lit_len > 16), wave::ballot(s.lit_len > 8));
    const uint32_t lit_at = s.lit_src & (kInRing - 1);
    const uint64_t lit_wraps = wave::ballot(lit_at + s.lit_len > kInRing + 16) & own_mask & word_mask;
    if (lit_wraps == 0) {
      if (lit_lane) {
        const uint8_t* src = ir.ring + lit_at;
        if (lit_steps == 2) {
          copy_dwords_clamped_disjoint<2>(dst, src, my_lit);
        } else if (lit_steps == 4) {
          copy_dwords_clamped_disjoint<4>(dst, src, my_lit);
        } else {
          copy_dwords_clamped_disjoint<8>(dst, src, my_lit);
        }
      }
    } else if (lit_lane) {
      const uint32_t last = my_lit - 4;
#pragma unroll 1
      for (uint32_t i = 0; i < lit_steps; ++i) {
        const uint32_t o = 4 * i < last ? 4 * i : last;
        lz::st_u32(dst + o, ld32(ir.ring + ((s.lit_src + o) & (kInRing - 1))));
      }
    }
    LZW_T(6); /* literal runs of 4..32 bytes */
    /* 1..3 bytes: byte-wise (as ONE misaligned dword store, whose excess bytes the match behind it would overwrite, they
     * measured 5 % slower on the headline: a misaligned LDS store costs a cycle or two per ACTIVE lane, and 30 % of the
     * sequences have such a run, 10 % one of four bytes or more) */
    if (own_mask & ~word_mask) {
      if (wave::lane_in(own_mask & ~word_mask)) {
        dst[0] = ir.ring[s.lit_src & (kInRing - 1)];
        if (my_lit > 1) {
          dst[1] = ir.ring[(s.lit_src + 1) & (kInRing - 1)];
        }
        if (my_lit > 2) {
          dst[2] = ir.ring[(s.lit_src + 2) & (kInRing - 1)];
        }
      }
    }
    LZW_T(12); /* literal runs of 1..3 bytes */
    uint64_t pending = wave::ballot(s.lit_len != 0) & mine_mask & ~own_mask;
    LZ_STAT("lit_lanes", wave::popc64(own_mask));
    LZ_STAT("lit_coop", wave::popc64(pending));
    while (pending) {
      const uint32_t j = wave::ctz64(pending);
      pending &= pending - 1;
      const uint32_t jsrc = wave::read_lane(s.lit_src, j);
      const uint32_t jlen = wave::read_lane(my_lit, j);
      const uint32_t jdst = wave::read_lane(lit_dst, j);
      if (!RING_LITERALS) {
        copy_to_lds(out_at(ow, jdst), ir.base + jsrc, jlen);
      } else {
        /* a ring without a stream behind it (deflate/deflate_decode.hip.h: the literals were decoded, not copied out
         * of the chunk): the run is resident by construction */
        uint8_t* d = out_at(ow, jdst);
        for (uint32_t i = lane; i < jlen; i += 64) {
          d[i] = ir.ring[(jsrc + i) & (kInRing - 1)];
        }
      }
    }
  }

  LZW_T(13); /* long literal runs, whole wave */
  /* ---- far match data into the window ---- */
  if (far_lane) {
    uint8_t* frame = out_at(ow, match_dst - far_a);
    if (far_steps == 2) {
      far_store_aligned<2, RING_LITERALS>(frame, far_a, far_data, far_l4, my_match);
    } else if (far_steps == 4) {
      far_store_aligned<4, RING_LITERALS>(frame, far_a, far_data, far_l4, my_match);
    } else {
      far_store_aligned<8, RING_LITERALS>(frame, far_a, far_data, far_l4, my_match);
    }
  }
  wave::sync();
  LZW_T(7);

  /* ---- remaining matches, oldest first: multi-round resolution in LDS ---- */
  {
    uint64_t pending = match_mask & ~far_mask;
    const uint32_t match_end = match_src + s.match_len; /* where a lane's source ends */
    LZ_STAT("match_far_lanes", wave::popc64(far_mask));
    LZ_STAT("match_near_lanes", wave::popc64(near_mask));
    LZ_STAT("match_hist_lanes", wave::popc64(hist_mask));
    LZ_STAT("match_coop", wave::popc64(pending & ~near_mask));
    LZ_STAT("match_coop_below_4", wave::popc64(match_mask & wave::ballot(my_match < 4)));
    LZ_STAT("match_coop_long", wave::popc64(match_mask & wave::ballot(my_match > kMatchShort)));
    LZ_STAT("match_coop_short_period",
            wave::popc64(short_mask & wave::ballot(match_src >= ow.valid_lo) & wave::ballot(s.match_off < 4)));
    while (pending) {
      const uint32_t f = wave::ctz64(pending);
      const uint32_t hw = wave::read_lane(match_dst, f); /* every byte below hw is final */
      if (!((near_mask >> f) & 1)) {
        /* the oldest pending match is long, has a period < 4, or reaches behind the window */
        const uint32_t foff = wave::read_lane(s.match_off, f);
        const uint32_t flen = wave::read_lane(my_match, f);
        coop_match(ow, hw, foff, flen);
        pending &= ~(1ull << f);
        LZW_T(14); /* matches copied by the whole wave */
        continue;
      }
      /* ready: a pending near lane whose source is final -- and the oldest one, whatever its source (it overlaps only
       * itself) */
      const uint64_t ready_mask = near_mask & pending & (wave::ballot(match_end <= hw) | (1ull << f));
      const uint32_t steps = steps_for(ready_mask, match_gt16, match_gt8);
      LZ_STAT("mrr_rounds", 1);
      LZ_STAT("mrr_iters", steps);
      if (wave::lane_in(ready_mask)) {
        const uint8_t* src = out_at(ow, match_src);
        uint8_t* dst = out_at(ow, match_dst);
        if (RING_LITERALS && my_match < 4) { /* three bytes, offset >= 4 */
          const uint8_t b0 = src[0], b1 = src[1], b2 = src[2];
          dst[0] = b0, dst[1] = b1, dst[2] = b2;
        } else if (steps == 2) {
          copy_dwords_clamped<2>(dst, src, my_match);
        } else if (steps == 4) {
          copy_dwords_clamped<4>(dst, src, my_match);
        } else {
          copy_dwords_clamped<8>(dst, src, my_match);
        }
      }
      wave::sync();
      pending &= ~ready_mask;
    }
  }

  LZW_T(8);
  out_flush(ow, op + total);
  LZW_T(9);
  wave::sync(); /* later far reads of this wave must see the flushed bytes */
  op += total;
  return take;
}

} // namespace lzw
