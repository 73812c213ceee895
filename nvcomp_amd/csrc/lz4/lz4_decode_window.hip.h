/*
 * lz4/lz4_decode_window.hip.h -- the LZ4 block decoder, on the LDS-staged executor
 * (common/lz_window.hip.h): what nvcompBatchedLZ4DecompressAsync runs, one wave per
 * chunk here, two waves or a workgroup per chunk through common/lz_pair.hip.h and
 * common/lz_team.hip.h with this file's front end. decode_chunk() returns the bytes
 * produced, 0 with an error bit for a chunk it rejects. (The block format: lz4_size.hip.h.)
 *
 * Token chase: the next 256 stream positions are examined in parallel -- lane l
 * of register j assumes a token starts at position wb + 64 j + l and computes
 * the distance to the token after it (reading the at most two length-extension
 * bytes it needs from the input ring). The real chain is then followed with one
 * v_readlane per sequence. Tokens with a literal run of 525 bytes or more or a match of
 * 1 549 or more (a third / a seventh length-extension byte) take a scalar slow path.
 */
#pragma once

#include "common/lz_window.hip.h"
#include "common/lz_chase.hip.h"
#include "common/lz_run_batch.hip.h"

namespace lz4w {

using lzw::kUnknown;
using lzw::ring_bytes8;

/* A length field behind a nibble of 15, its bytes in `f` from bit 0 on (six of them, zeros above): how many of them are
 * 255 (0 .. 6; 6 = the field goes on behind what f holds) */
__device__ __forceinline__ uint32_t leading_255(uint64_t f)
{
  return (uint32_t)__builtin_ctzll(~f) >> 3; /* bits 48-63 of ~f are set */
}

/* Distance from a (speculative) token at virtual position p to the next token, with every bound tested: the windows at
 * the edges of the chunk and of the resident stream, and the positions of an interior window whose lengths the
 * straight-line DeltaFn::fast() gave up on. Up to two extension bytes of the literal length (runs to 524 bytes) and SIX
 * of the match length (to 1 548 bytes): a sorted key column compressed by liblz4 -- the reference's published shape --
 * is all matches of 170 .. 680 bytes, and with one extension byte every one of its tokens left the chase through the
 * scalar slow path, one enumeration per token (profiles/archive/r03_pmc_mortgage.json: 155 scalar instructions per sequence).
 * Longer fields -> kUnknown -> chase_slow_next(). */
template <class R>
__device__ __forceinline__ uint32_t token_delta(const R& r, uint32_t p)
{
  const uint8_t* ring = r.ring;
  const uint32_t m = R::kMask;
  const uint32_t t = ring[p & m];
  const uint32_t e1 = ring[(p + 1) & m];
  const uint32_t e1b = ring[(p + 2) & m];
  const uint32_t lit_code = t >> 4;
  const bool lit_ext = lit_code == 15;
  const bool lit_ext2 = lit_ext && e1 == 255;
  const uint32_t lit = lit_code + (lit_ext ? e1 : 0u) + (lit_ext2 ? e1b : 0u);
  const uint32_t lit_end = p + 1 + (lit_ext ? 1u : 0u) + (lit_ext2 ? 1u : 0u) + lit;
  const bool ends = lit_end >= r.vend; /* literals reach the end of the chunk: the chase stops here */
  const uint32_t mpos = lit_end + 2;   /* where a match-length extension byte would sit */
  const bool m_ext = (t & 15u) == 15u;
  const uint32_t n255 = leading_255(ring_bytes8(r, mpos) & 0xffffffffffffull);
  const uint32_t mfield = m_ext ? n255 + 1 : 0u; /* bytes of the match length field: trusted below only when resident */
  const uint32_t delta = ends ? lit_end - p : mpos + mfield - p;
  const bool unknown = p < r.lo || p + 3 > r.hi || p >= r.vend || (lit_ext2 && e1b == 255)
                       || (!ends && m_ext && (n255 >= 6 || mpos + n255 >= r.hi));
  return unknown ? kUnknown : delta;
}


/* The rest of a length field whose bytes so far were all 255, from virtual position pos on: 64 bytes per step (a byte
 * per lane, one ballot for the first byte that is not 255). Adds the bytes to `sum` (saturating: a corrupt stream may claim
 * anything) and returns the position behind the field, or vend + 1 when the chunk ends first. Whole wave, uniform
 * arguments. A chunk that is ONE literal run or ONE match -- incompressible data, zeros -- spells its length in 257 such
 * bytes, and walking them one dependent LDS read at a time (twice: once for the chase, once for the parser) took a third
 * of such a chunk's time. */
template <class R>
__device__ __forceinline__ uint32_t scan_length_bytes(const R& r, uint32_t pos, uint32_t& sum)
{
  const uint32_t lane = (uint32_t)wave::fresh_lane_id();
  for (;;) {
    const uint32_t p = pos + lane;
    const bool inside = p < r.vend;
    const uint32_t b = inside ? lzw::in_byte(r, p) : 0u;
    const uint64_t stop = wave::ballot(b != 255u || !inside);
    if (stop) {
      const uint32_t n = wave::ctz64(stop);
      if (pos + n >= r.vend) {
        return r.vend + 1;
      }
      const uint32_t add = 255u * n + wave::read_lane(b, n);
      sum = sum + add < 0x7fffff00u ? sum + add : 0x7fffff00u;
      return pos + n + 1;
    }
    sum = sum + 255u * 64u < 0x7fffff00u ? sum + 255u * 64u : 0x7fffff00u;
    pos += 64;
  }
}

/* Scalar walk over one token with multi-byte length extensions. */
template <class R>
__device__ __forceinline__ uint32_t chase_slow_next(const R& r, uint32_t q)
{
  const uint32_t vend = r.vend;
  const uint32_t t = lzw::in_byte_uniform(r, q);
  uint32_t pos = q + 1;
  uint32_t lit = t >> 4;
  if (lit == 15) {
    pos = scan_length_bytes(r, pos, lit);
    if (pos > vend) {
      return vend + 1;
    }
  }
  if (lit >= vend - pos) {
    return vend + 1;
  }
  pos += lit + 2;
  if ((t & 15u) == 15u) {
    uint32_t ignored = 0;
    pos = scan_length_bytes(r, pos, ignored);
    if (pos > vend) {
      return vend + 1;
    }
  }
  return pos;
}


struct DeltaFn
{
  /* a delta looks at most this far past its position: token, 2 length bytes, 15 + 254 literals, offset, 8 bytes of length */
  static constexpr uint32_t kReach = 288;
  template <class R>
  __device__ __forceinline__ uint32_t operator()(const R& r, uint32_t p) const { return token_delta(r, p); }
  /* interior window: `w` = the stream bytes from p on (token in bits 0-7, the byte behind it in 8-15) */
  template <class R>
  __device__ __forceinline__ uint32_t fast(const R& r, uint32_t p, uint64_t w) const
  {
    /* straight-line on purpose (no ||, no early exit): the byte a match-length extension would use is read whatever
     * the token says, so that the four positions of a lane compile to one instruction stream without exec-mask
     * juggling -- the scalar unit is as busy as the vector unit in this kernel */
    const uint32_t t = (uint32_t)w & 0xffu;
    const uint32_t e1 = (uint32_t)(w >> 8) & 0xffu;
    const uint32_t lit_code = t >> 4;
    const uint32_t lit_ext = lit_code == 15 ? 1u : 0u;
    const uint32_t d0 = 3 + lit_code + (lit_ext ? e1 + 1u : 0u); /* to the byte a match-length extension would use */
    const uint32_t m_ext = (t & 15u) == 15u ? 1u : 0u;
    const uint32_t e2 = r.ring[(p + d0) & R::kMask];
    const uint32_t unknown = (lit_ext & (e1 == 255 ? 1u : 0u)) | (m_ext & (e2 == 255 ? 1u : 0u));
    return unknown ? kUnknown : d0 + m_ext;
  }
  /* the positions fast() gave up on, once more (lzw::chase_build, under a branch of the wave): a match length with two
   * to six extension bytes -- 274 .. 1 548 bytes, every sequence of a sorted key column -- is resolved here; everything
   * longer stays with the scalar walk */
  static constexpr bool kSecondChance = true;
  template <class R>
  __device__ __forceinline__ uint32_t second(const R& r, uint32_t p, uint64_t w) const
  {
    const uint32_t t = (uint32_t)w & 0xffu;
    const uint32_t e1 = (uint32_t)(w >> 8) & 0xffu;
    const uint32_t lit_code = t >> 4;
    const bool lit_ext = lit_code == 15;
    const uint32_t d0 = 3 + lit_code + (lit_ext ? e1 + 1u : 0u);
    const uint32_t n255 = leading_255(ring_bytes8(r, p + d0) & 0xffffffffffffull);
    const bool ok = !(lit_ext && e1 == 255) && (t & 15u) == 15u && n255 < 6;
    return ok ? d0 + n255 + 1 : kUnknown;
  }
};
struct SlowFn
{
  template <class R>
  __device__ __forceinline__ uint32_t operator()(const R& r, uint32_t p) const { return chase_slow_next(r, p); }
};

/* Lane-parallel field decode of the sequence whose token is at virtual position p (the general parser: any length, any
 * residency, the chunk's last sequence). A lane reads the first byte of a length field itself; a field that goes on
 * behind a 255 is finished by the whole wave, one such lane after the other (scan_length_bytes). */
template <class R>
__device__ __forceinline__ void parse(const R& r, uint32_t p, bool active, lz::Seq& s, bool& bad)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  const uint32_t vend = r.vend;
  s.lit_src = 0;
  s.lit_len = 0;
  s.match_off = 0;
  s.match_len = 0;
  bad = false;
  uint32_t t = 0, pos = 0, lit = 0;
  bool more = false;
  if (active) {
    t = lzw::in_byte(r, p);
    pos = p + 1;
    lit = t >> 4;
    if (lit == 15) {
      if (pos >= vend) {
        bad = true;
      } else {
        const uint32_t b = lzw::in_byte(r, pos++);
        lit += b;
        more = b == 255;
      }
    }
  }
  for (uint64_t m = wave::ballot(more); m; m &= m - 1) {
    const uint32_t j = wave::ctz64(m);
    uint32_t sum = 0;
    const uint32_t np = scan_length_bytes(r, wave::read_lane(pos, j), sum);
    if (lane == j) {
      bad = np > vend;
      pos = np;
      lit += sum;
    }
  }
  bool has_match = false;
  uint32_t mlen = 0;
  more = false;
  if (active && !bad) {
    if (lit > vend - pos) {
      bad = true;
    } else {
      s.lit_src = pos;
      s.lit_len = lit;
      pos += lit;
      if (pos != vend) { /* pos == vend: the last sequence, literals only */
        if (vend - pos < 2) {
          bad = true;
        } else {
          s.match_off = lzw::in_byte(r, pos) | (lzw::in_byte(r, pos + 1) << 8);
          pos += 2;
          has_match = true;
          mlen = t & 15u;
          if (mlen == 15) {
            if (pos >= vend) {
              bad = true;
            } else {
              const uint32_t b = lzw::in_byte(r, pos++);
              mlen += b;
              more = b == 255;
            }
          }
        }
      }
    }
  }
  for (uint64_t m = wave::ballot(more); m; m &= m - 1) {
    const uint32_t j = wave::ctz64(m);
    uint32_t sum = 0;
    const uint32_t np = scan_length_bytes(r, wave::read_lane(pos, j), sum);
    if (lane == j) {
      bad = np > vend;
      pos = np;
      mlen += sum;
    }
  }
  if (has_match && !bad) {
    if (mlen > 0x40000000u || pos >= vend) { /* a token must follow every match */
      bad = true;
    } else {
      s.match_len = mlen + 4;
    }
  }
  if (bad) {
    s.lit_src = 0;
    s.lit_len = 0;
    s.match_off = 0;
    s.match_len = 0;
  }
}

/* The parser of a batch, lanes [from, to) (to >= from). A lane whose fields are resident and inside the chunk -- the
 * position of its offset tells: everything it looks at lies within 8 bytes of it -- runs straight-line code: one
 * extension byte of the literal length, up to six of the match length (to 1 548 bytes; 255 * (the number of leading 255s)
 * + the byte behind them). The other lanes -- the last sequences of a chunk, a literal run of 270 bytes or more, a
 * longer match -- go through parse() together afterwards. (Until the middle of round 3 ONE such lane sent the whole
 * batch to parse(), which finishes a field with a second extension byte one lane after the other: every batch of a
 * sorted key column -- matches of 170 .. 680 bytes -- and the last 40 sequences of every such chunk.) */
/* Returns the lanes whose sequence is malformed, as a mask: the persistent loop asks "any?" on the scalar unit. */
template <class R>
__device__ __forceinline__ uint64_t parse_batch_mask(const R& r, uint32_t p, uint32_t from, uint32_t to, lz::Seq& s)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  const uint32_t lim = r.hi < r.vend ? r.hi : r.vend;
  const uint64_t w = ring_bytes8(r, p); /* a lane outside [from, to) reads somewhere inside the ring: harmless */
  const uint32_t t = (uint32_t)w & 0xffu;
  const uint32_t e1 = (uint32_t)(w >> 8) & 0xffu;
  const uint32_t code = t >> 4;
  const bool lit_ext = code == 15;
  const uint32_t lit = code + (lit_ext ? e1 : 0u);
  const uint32_t lit_src = p + 1 + (lit_ext ? 1u : 0u);
  const uint32_t q = lit_src + lit; /* the offset */
  const uint64_t x = ring_bytes8(r, q);
  const uint32_t mcode = t & 15u;
  const uint64_t f = x >> 16; /* the match length field, if there is one */
  const uint32_t n255 = leading_255(f);
  const uint32_t mext = 255u * n255 + ((uint32_t)(f >> (8 * n255)) & 0xffu);
  /* not for this path: a second extension byte of the literal length (code 15 followed by 255 = bits 4-15 of w all
   * set), a seventh of the match length, fields that are not resident or reach the end of the chunk (q + 8 < vend also
   * says that a token follows the match) */
  const bool lit2 = ((uint32_t)w & 0xfff0u) == 0xfff0u;
  /* (masks of single compares joined on the scalar unit, the lane's predicate taken from the mask: common/lz_copy.hip.h,
   * steps_for; common/lz_window.hip.h) */
  const uint64_t active = wave::ballot(lane - from < to - from);
  const uint64_t other = wave::ballot(lit2) | wave::ballot(n255 >= 6) | wave::ballot(p < r.lo) | wave::ballot(q + 8 >= lim);
  const bool mine = wave::lane_in(active & ~other);
  s.lit_src = mine ? lit_src : 0;
  s.lit_len = mine ? lit : 0;
  s.match_off = mine ? ((uint32_t)x & 0xffffu) : 0;
  s.match_len = mine ? mcode + 4 + (mcode == 15 ? mext : 0u) : 0;
  const uint64_t rest = active & other;
  uint64_t bad_mask = 0;
  if (rest) {
    lz::Seq g;
    bool gbad;
    parse(r, p, wave::lane_in(rest), g, gbad);
    if (wave::lane_in(rest)) {
      s = g;
    }
    bad_mask = wave::ballot(gbad) & rest;
  }
  return bad_mask;
}
template <class R>
__device__ __forceinline__ void parse_batch(const R& r, uint32_t p, uint32_t from, uint32_t to, lz::Seq& s, bool& bad)
{
  bad = wave::lane_in(parse_batch_mask(r, p, from, to, s));
}

/* What the workgroup-per-chunk decoder (common/lz_team.hip.h) and the two-wave decoder (common/lz_pair.hip.h) need to know
 * of the format. */
struct FrontEnd
{
  static constexpr uint32_t kPositions = 192; /* a sequence is at least 3 bytes (token + offset): 64 tokens at most */
  static constexpr bool kEmptyIsError = false; /* an empty block decodes to nothing */
  static constexpr uint32_t kFewLongMatchesRatio = 16; /* common/lz_team.hip.h: such chunks go to the two-wave decoder */
  using Delta = DeltaFn;
  using Slow = SlowFn;
  /* an LZ4 block does not say what it decodes to: the caller's capacity decides (pass tight capacities for the team path) */
  static constexpr bool kDeclaresLength = false;
  static __device__ __forceinline__ uint32_t declared_length(const uint8_t*, uint32_t) { return ~0u; }
  template <class R>
  static __device__ __forceinline__ bool begin(const R& r, uint32_t out_cap, uint32_t& q, uint32_t& limit, uint32_t&)
  {
    q = r.vbeg;
    limit = out_cap;
    return true;
  }
  static __device__ __forceinline__ bool finish_ok(uint32_t, uint32_t, uint32_t, uint32_t) { return true; }
  template <class R>
  static __device__ __forceinline__ void parse_batch(const R& r, uint32_t p, uint32_t from, uint32_t to, lz::Seq& s, bool& bad)
  {
    lz4w::parse_batch(r, p, from, to, s, bad);
  }
  /* the two waves: the tokens start with the block */
  static __device__ __forceinline__ bool open(lzw::InRing& ir, uint32_t& q, uint32_t& total)
  {
    q = ir.vbeg;
    total = 0;
    return true;
  }
  /* every sequence has a position, in stream order: from the first one's literals to the last one's */
  static __device__ __forceinline__ void ensure_literals(lzw::InRing& ir, const lz::Seq& s, uint32_t count)
  {
    const uint32_t oldest = wave::read_lane(s.lit_src, 0);
    const uint32_t newest = wave::read_lane(s.lit_src, count - 1);
    lzw::in_ensure(ir, oldest, (newest & ~(lzw::kInBlock - 1)) + 2 * lzw::kInBlock);
  }
  static __device__ __forceinline__ uint32_t streamed_take(const lz::Seq&, uint32_t) { return 1; }
};

/* Decode one chunk with the calling wave; `lds` is this wave's kLdsPerWave bytes. */
/* RUNS: the loop tries lzw::execute_run_batch (sorted keys, typed columns). Its mere presence in the loop costs every
 * other kind of data 1.5-2 % (block placement and register allocation of the batch executor around it: gpurun r6u, r6v --
 * the same with the attempts gated off at run time), so the kernels instantiate the loop twice and pick per chunk by what
 * the stream shrank to (decode_one: runs only pay from 8 x on). */
template <bool CHECKED, bool RUNS = false>
__device__ __forceinline__ uint32_t decode_chunk(
    const uint8_t* __restrict__ in, uint32_t in_len, uint8_t* out, uint32_t out_cap, uint8_t* lds, uint32_t& err)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  err = lz::kErrNone;
  if (in_len == 0) {
    return 0;
  }
  LZW_T(9);
  lzw::InRing ir;
  lzw::OutWindow ow;
  lzw::in_init(ir, in, in_len, lds + lzw::kOutLds);
  lzw::out_init(ow, out, lds);
  lzw::Chase c;
  lzw::chase_init(c, ir.vbeg, lds + lzw::kOutLds + lzw::kInLds);
  uint32_t op = 0;
  uint32_t seqpos = 0;
  uint32_t count = 0; /* sequences recorded in seqpos lanes [0, count) and not yet executed */
  /* A batch ends at 1 KiB of output, so on data with long matches (runs, sorted key columns: 200-400 bytes per
   * sequence) a round executes only a handful of the 64 sequences a chase delivers: chasing again for the rest every
   * round was 5 000 cycles per SEQUENCE on the reference's own published shape (profiles/archive/r02_mortgage_like.json).
   * The chase runs only when fewer than kRefillBelow token positions are left; on text a round takes all 64 and
   * every round refills, as before. The parsed FIELDS stay in registers across rounds too (four more live registers);
   * parsing the positions in hand again every round (two LDS round trips) measured 498 against 500 GB/s on the headline
   * batch (noise) and 442 against 545 on the mortgage-like column. */
  constexpr uint32_t kRefillBelow = 24;
  lzw::RunGate gate = lzw::kRunGateInit;
  lz::Seq s;
  s.lit_src = 0;
  s.lit_len = 0;
  s.match_off = 0;
  s.match_len = 0;
  for (;;) {
    const bool more = c.q < ir.vend; /* the chase has stream left */
    if (count == 0 && !more) {
      break;
    }
    const uint32_t before = count; /* lanes [before, count) are parsed this round */
    const bool refill = count < kRefillBelow && more;
    /* (`more` computed once, and chase and parse under a test of `refill` each, on purpose: with c.q compared where it is
     * used the compiler rotates the loop, with one block it lays the kernels out anew, and both were measured --
     * two waves per chunk lose 2-3 % at 4 096 chunks: profiles/lz_token_index_retired.md) */
    if (refill) {
      /* keep the stream resident from the oldest unexecuted token to well past the chase */
      const uint32_t oldest = count ? wave::read_lane(seqpos, 0) : c.q;
      LZW_T(10);
      lzw::in_ensure(ir, oldest, (c.q & ~(lzw::kInBlock - 1)) + 3 * lzw::kInBlock);
      LZW_T(0);
      count = lzw::chase_tokens(c, ir, seqpos, count, DeltaFn(), SlowFn());
    }
    if (refill) {
      lz::Seq fresh;
      const uint64_t bad = parse_batch_mask(ir, seqpos, before, count, fresh);
      LZW_T(3);
      if (lane >= before) {
        s = fresh;
      }
      if (bad) {
        err |= lz::kErrInput;
        return 0;
      }
    }
    bool big = false;
    /* runs (sorted keys, typed columns) are executed 60 at a time, straight to the output: lzw::execute_run_batch */
    static_assert(!NVCOMP_LZW_RUNS || lzw::kRunFits, "the run executor needs 2 176 bytes of window LDS");
    uint32_t take = 0;
    if (RUNS && lzw::run_gate_open(gate)) {
      bool misfit;
      take = lzw::execute_run_batch<CHECKED>(ir, ow, out_cap, op, count, s, misfit);
      gate = wave::uniform(lzw::run_gate_tried(gate, take, misfit));
    }
    if (take == 0) {
      take = lzw::execute_window_batch<CHECKED, false, true>(ir, ow, out_cap, op, count, s, err, big); /* HISTORY: one wave a chunk is what runs at the card's gather rate */
      if (CHECKED && err) {
        return 0;
      }
      if (RUNS) {
        gate = wave::uniform(lzw::run_gate_window_took(gate, take, count));
      }
    }
    if (big) {
      /* the first sequence in hand has a long literal run or a long match, or is larger than a batch: straight to HBM */
      if (!lzw::stream_sequence<CHECKED>(ir, ow, out_cap, op, wave::read_lane(s.lit_src, 0), wave::read_lane(s.lit_len, 0),
                                         wave::read_lane(s.match_off, 0), wave::read_lane(s.match_len, 0), err)) {
        return 0;
      }
      take = 1;
    }
    /* drop the executed sequences, keep the rest for the next round */
    if (take < count) {
      const uint32_t from = (lane + take) & 63u;
      seqpos = wave::shuffle(seqpos, from);
      lzw::drop_front(s, take, count);
    }
    count -= take;
  }
  lzw::out_flush_all(ow, op);
  return op;
}

} // namespace lz4w
