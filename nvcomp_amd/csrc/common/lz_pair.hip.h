/*
 * common/lz_pair.hip.h -- two waves per chunk (small batches), for LZ4 and Snappy alike.
 *
 * One wave per chunk leaves the card under-filled below ~7 000 chunks, and a 64 KiB chunk takes a wave ~0.75 ms
 * however idle the CU is: the wave's own dependent chain -- chase, parse, far loads, copy rounds, flush -- is what
 * takes the time (profiles/archive/r02_decode_phases.json). For small batches the chain is cut in two: wave 0 of a 128-thread
 * workgroup (the PRODUCER) runs the token chase and the parse and hands batches of parsed sequences to wave 1 (the
 * CONSUMER), which executes them; the two overlap, a chunk takes about as long as its slower half. Hand-over is a
 * two-slot queue in LDS with one flag word per slot (wave::lds_store_release / lds_load_acquire). The producer never
 * depends on anything the consumer does except a free slot; each wave keeps its own ring over the compressed stream
 * (the consumer's serves the literal copies), so nothing else is shared. Same bytes as the formats' decode_chunk.
 *
 * The format is a FrontEnd (lz4w::FrontEnd, snappyw::FrontEnd: the one common/lz_team.hip.h decodes with). Of it the two
 * waves use Delta, Slow and parse_batch() as the team does, and what the formats differ in here:
 *   open(ir, q, total)              the start of the stream: q = the first token; false = malformed. Snappy makes the first
 *                                   ring block resident and reads its preamble (total = what the elements must produce)
 *   kDeclaresLength                 whether open() gives a total. Then, under CHECKED, the chunk may produce exactly that
 *                                   (not the caller's capacity, which must hold it), and the tokens must end exactly at the
 *                                   end of the stream: the producer sees the one, the consumer the other
 *   ensure_literals(ir, s, count)   the stream bytes that the literal copies of the sequences in hand read, made resident
 *                                   (for speed: a literal run that is not resident is copied from HBM, lane after lane)
 *   streamed_take(s, count)         how many sequences a streamed one takes out of the hand (Snappy: the empty followers
 *                                   of its copy train with it, which would cost a round of their own)
 */
#pragma once

#include "common/lz_window.hip.h"
#include "common/lz_chase.hip.h"
#include "common/lz_run_batch.hip.h"

namespace lzw {
namespace pair {

constexpr uint32_t kSlotBytes = 16 + 4 * 64 * 4; /* n, flags, pad | lit_src[64] | lit_len[64] | match_off[64] | match_len[64] */
constexpr uint32_t kFlagLast = 1, kFlagBad = 2;
constexpr uint32_t kCtrlBytes = 16; /* state[2], abort, pad */
/* window | consumer ring | producer ring | chase tables | two slots | control */
constexpr uint32_t kLdsPerChunk = lzw::kOutLds + 2 * lzw::kInLds + lzw::kChaseLds + 2 * kSlotBytes + kCtrlBytes;

struct Shared
{
  uint8_t* slots;  /* two of kSlotBytes each: slot(k) -- not an array of two pointers: indexed by a run-time k, that array
                    * lived in scratch memory (40 bytes per lane, a scratch load per hand-over) */
  uint32_t* state; /* [2]: 0 = empty, 1 = full */
  uint32_t* abort; /* the consumer gave up: the producer stops waiting */
  __device__ __forceinline__ uint8_t* slot(uint32_t k) const { return slots + k * kSlotBytes; }
};

__device__ __forceinline__ Shared shared_at(uint8_t* lds)
{
  uint8_t* q = lds + lzw::kOutLds + 2 * lzw::kInLds + lzw::kChaseLds;
  Shared sh;
  sh.slots = q;
  sh.state = (uint32_t*)(q + 2 * kSlotBytes);
  sh.abort = sh.state + 2;
  return sh;
}

/* Both slots empty, no abort: by the first four threads of the workgroup, in front of a barrier. `lds`: the chunk's
 * kLdsPerChunk bytes. */
__device__ __forceinline__ void reset_control(uint8_t* lds)
{
  if (threadIdx.x < 4) {
    ((uint32_t*)(lds + kLdsPerChunk - kCtrlBytes))[threadIdx.x] = 0;
  }
}

/* lane 0's view of a flag word, the same for the whole wave */
__device__ __forceinline__ uint32_t poll(const uint32_t* p)
{
  return wave::read_lane(wave::lds_load_acquire(p), 0);
}

/* A batch of `count` sequences, one per lane, into slot k (which the producer found empty) ... */
__device__ __forceinline__ void slot_write(const Shared& sh, uint32_t k, const lz::Seq& s, uint32_t count, uint32_t flags)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  uint32_t* f = (uint32_t*)(sh.slot(k) + 16);
  f[lane] = s.lit_src;
  f[64 + lane] = s.lit_len;
  f[128 + lane] = s.match_off;
  f[192 + lane] = s.match_len;
  if (lane == 0) {
    ((uint32_t*)sh.slot(k))[0] = count;
    ((uint32_t*)sh.slot(k))[1] = flags;
  }
}

/* ... and out of it (which the consumer found full) */
__device__ __forceinline__ void slot_read(const Shared& sh, uint32_t k, lz::Seq& s, uint32_t& count, uint32_t& flags)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  const uint32_t* f = (const uint32_t*)(sh.slot(k) + 16);
  s.lit_src = f[lane];
  s.lit_len = f[64 + lane];
  s.match_off = f[128 + lane];
  s.match_len = f[192 + lane];
  count = wave::read_lane(((const uint32_t*)sh.slot(k))[0], 0);
  flags = wave::read_lane(((const uint32_t*)sh.slot(k))[1], 0);
}

/* The consumer gives the chunk up: the producer stops waiting for a free slot. */
__device__ __forceinline__ void raise_abort(const Shared& sh)
{
  if (wave::lane_id() == 0) {
    wave::lds_store_release(sh.abort, 1u);
  }
}

template <class FrontEnd, bool CHECKED>
__device__ __forceinline__ void produce(const uint8_t* __restrict__ in, uint32_t in_len, uint8_t* lds)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  const Shared sh = shared_at(lds);
  lzw::InRing ir;
  lzw::in_init(ir, in, in_len, lds + lzw::kOutLds + lzw::kInLds);
  uint32_t q, total;
  const bool opened = FrontEnd::open(ir, q, total); /* false: one slot that says so (the consumer reads the same and left) */
  lzw::Chase c;
  lzw::chase_init(c, q, lds + lzw::kOutLds + 2 * lzw::kInLds);
  uint32_t k = 0;
  for (;;) {
    const bool last = !opened || c.q >= ir.vend;
    uint32_t count = 0;
    lz::Seq s;
    s.lit_src = 0, s.lit_len = 0, s.match_off = 0, s.match_len = 0;
    /* the tokens must end exactly at the end (belt and braces: the parser flags a token that passes the end first, so no
     * stream gets here with c.q behind vend; the test mirrors the one-wave loops and the team's finish_ok) */
    bool bad = !opened || (last && CHECKED && FrontEnd::kDeclaresLength && c.q != ir.vend);
    if (!last) {
      lzw::in_ensure(ir, c.q, (c.q & ~(lzw::kInBlock - 1)) + 3 * lzw::kInBlock);
      uint32_t seqpos = 0;
      count = lzw::chase_tokens(c, ir, seqpos, 0, typename FrontEnd::Delta(), typename FrontEnd::Slow());
      FrontEnd::parse_batch(ir, seqpos, 0, count, s, bad);
    }
    const uint32_t flags = (last ? kFlagLast : 0u) | (wave::ballot(bad) ? kFlagBad : 0u);
    while (poll(sh.state + k) != 0) {
      if (poll(sh.abort) != 0) {
        return;
      }
      wave::nap();
    }
    slot_write(sh, k, s, count, flags);
    wave::sync();
    if (lane == 0) {
      wave::lds_store_release(sh.state + k, 1u);
    }
    if (flags) {
      return; /* the end of the chunk, or a malformed token: nothing follows */
    }
    k ^= 1;
  }
}

/* RUNS: the rounds try the run executor first (Format::kPairRuns; false in both formats: their chunks of runs go to Format::alone). */
template <class FrontEnd, bool CHECKED, bool RUNS>
__device__ __forceinline__ uint32_t consume(
    const uint8_t* __restrict__ in, uint32_t in_len, uint8_t* out, uint32_t out_cap, uint8_t* lds, uint32_t& err)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  const Shared sh = shared_at(lds);
  lzw::InRing ir;
  lzw::OutWindow ow;
  lzw::in_init(ir, in, in_len, lds + lzw::kOutLds);
  lzw::out_init(ow, out, lds);
  uint32_t q, total;
  const bool opened = FrontEnd::open(ir, q, total);
  if (!opened || (CHECKED && FrontEnd::kDeclaresLength && total > out_cap)) {
    err = opened ? lz::kErrOutput : lz::kErrInput;
    raise_abort(sh);
    return 0;
  }
  const uint32_t limit = CHECKED && FrontEnd::kDeclaresLength ? total : out_cap;
  uint32_t op = 0;
  uint32_t count = 0;
  uint32_t k = 0;
  lzw::RunGate gate = lzw::kRunGateInit;
  lz::Seq s;
  s.lit_src = 0, s.lit_len = 0, s.match_off = 0, s.match_len = 0;
  for (;;) {
    if (count == 0) {
      while (poll(sh.state + k) != 1) {
        wave::nap();
      }
      uint32_t n, flags;
      slot_read(sh, k, s, n, flags);
      wave::sync();
      if (lane == 0) {
        wave::lds_store_release(sh.state + k, 0u);
      }
      k ^= 1;
      if (flags & kFlagBad) {
        err |= lz::kErrInput;
        return 0;
      }
      if (flags & kFlagLast) {
        break;
      }
      count = n;
      if (count == 0) {
        continue;
      }
    }
    FrontEnd::ensure_literals(ir, s, count); /* the literal copies read this wave's own ring */
    bool big = false;
    uint32_t take = 0;
    if (RUNS && lzw::run_gate_open(gate)) {
      bool misfit;
      take = lzw::execute_run_batch<CHECKED>(ir, ow, limit, op, count, s, misfit);
      gate = wave::uniform(lzw::run_gate_tried(gate, take, misfit));
    }
    if (take == 0) {
      take = lzw::execute_window_batch<CHECKED>(ir, ow, limit, op, count, s, err, big);
      if (RUNS) {
        gate = wave::uniform(lzw::run_gate_window_took(gate, take, count));
      }
    }
    if (CHECKED && err) {
      raise_abort(sh);
      return 0;
    }
    if (big) {
      /* the first sequence in hand has a long literal run or a long match, or is larger than a batch: straight to HBM */
      if (!lzw::stream_sequence<CHECKED>(ir, ow, limit, op, wave::read_lane(s.lit_src, 0), wave::read_lane(s.lit_len, 0),
                                         wave::read_lane(s.match_off, 0), wave::read_lane(s.match_len, 0), err)) {
        raise_abort(sh);
        return 0;
      }
      take = FrontEnd::streamed_take(s, count);
    }
    if (take < count) {
      lzw::drop_front(s, take, count);
    }
    count -= take;
  }
  if (CHECKED && FrontEnd::kDeclaresLength && op != total) {
    err |= lz::kErrInput;
    return 0;
  }
  lzw::out_flush_all(ow, op);
  return op;
}

} // namespace pair
} // namespace lzw
