/*
 * zstd/zstd_decode.hip.h -- batched Zstandard (RFC 8878) decoder for gfx950.
 *
 * Replaces the device side of nvcompBatchedZstdDecompressAsync. The chunks are written by CPU libzstd (Parquet / ORC /
 * Arrow pages, .zst files); the wire format is the public one and libzstd is the oracle in tests/.
 *
 * One wavefront per chunk, in the DEFLATE decoder's shape (deflate/deflate_decode.hip.h):
 *   frame / block layer   wave-uniform: frame header (FCS widths 0/1/2/4/8, the 2-byte form + 256), skippable frames,
 *                         3-byte block headers. A raw block is a wave-wide 16-byte copy HBM -> HBM, an RLE block a
 *                         fill; both go around the executor's window (flushed in front, restarted behind).
 *   literals              raw / RLE / Huffman / treeless (the Huffman table persists across the blocks of a frame).
 *                         They are regenerated into the wave's slot of the temp buffer (one block's literals, at most
 *                         128 KiB): raw and RLE by the whole wave, Huffman streams one lane per stream (1 or 4 lanes),
 *                         each read backwards from its padding bit through an 11-bit lookup table in LDS.
 *   sequences             wave-uniform FSE decode of the three interleaved states (LL, OF, ML) with the repeat offsets
 *                         of the frame; each sequence {literal run, match length, offset} becomes one or more records
 *                         (split so that a batch produces at most lzw::kBatchMax bytes).
 *   back end              64 records at a time are executed by the LZ window executor (common/lz_window.hip.h) with
 *                         RING_LITERALS: a batch's literals are copied from the slot into a 1 KiB literal ring in LDS
 *                         first, exactly as DEFLATE's front end fills its ring. Far matches (up to 16 MiB back) are
 *                         read from the chunk's output in HBM.
 *
 * LDS per wave (kLdsPerWave = 9.1 KiB): executor window 1 152 B | literal ring 1 040 B | Huffman
 * lookup 2^11 x u16 = 4 KiB | FSE tables LL 2^9, ML 2^9, OF 2^8 x u16 = 2.5 KiB | 512 B of table-construction scratch.
 * An FSE cell is 16 bits: symbol (6) | x (10), where x is the cell's "next state" in [count, 2 count); its bit count is
 * accuracy_log - highbit(x) and its baseline (x << bits) - table size, so no baseline is stored. RLE mode is a table of
 * accuracy 0 with one cell (x = 1: no bits, baseline 0).
 *
 * Validation: every read is bounded by the chunk, every write by the output capacity (the executor's checks plus the
 * raw / RLE paths' own); normalized counts must sum to 1 << accuracy_log (accuracy <= 9 for LL / ML, 8 for OF, 6 for
 * Huffman weights), Huffman weights must complete a code of at most 11 bits, every bit stream must end exactly at its
 * padding bit, and an offset may not reach in front of its frame. Every loop is bounded by the input or a table size.
 * A frame with a Dictionary_ID is refused with kUnsupported; the content checksum is skipped, not verified.
 */
#pragma once

#ifndef NVCOMP_LZW_BATCHMAX
#define NVCOMP_LZW_BATCHMAX 1024
#endif
#ifndef NVCOMP_LZW_INRING
#define NVCOMP_LZW_INRING 1024
#endif
#include "common/lz_window.hip.h"

namespace zstd {

static_assert(lzw::kBatchMax <= lzw::kInRing, "a batch's literals fit the literal ring");

constexpr uint32_t kMagic = 0xFD2FB528u;
constexpr uint32_t kBlockMax = 128u * 1024u;  /* Block_Maximum_Size: also the most literals a block regenerates */
constexpr uint32_t kHufMaxBits = 11;
constexpr uint32_t kLLMaxLog = 9, kMLMaxLog = 9, kOFMaxLog = 8;
constexpr uint32_t kLLMaxSym = 35, kMLMaxSym = 52, kOFMaxSym = 31;

/* error bits besides lz::kErr* */
constexpr uint32_t kUnsupported = 8;

/* ---- LDS of one wave ---- */
constexpr uint32_t kOffWin = 0;
constexpr uint32_t kOffRing = kOffWin + lzw::kOutLds;
constexpr uint32_t kOffHuf = kOffRing + lzw::kInLds;           /* u16[1 << 11]: symbol | bits << 8 */
constexpr uint32_t kOffLL = kOffHuf + (2u << kHufMaxBits);     /* u16[1 << 9] */
constexpr uint32_t kOffML = kOffLL + (2u << kLLMaxLog);        /* u16[1 << 9] */
constexpr uint32_t kOffOF = kOffML + (2u << kMLMaxLog);        /* u16[1 << 8] */
constexpr uint32_t kOffTmp = kOffOF + (2u << kOFMaxLog);       /* 512 B: weights u8[256] | norm i16[64] | next u16[64] */
constexpr uint32_t kLdsPerWave = kOffTmp + 512;
static_assert(kOffHuf % 16 == 0 && kLdsPerWave % 16 == 0, "16-byte alignment");

/* ---- temp buffer: a ticket counter, then one literal slot per wave of the launch ---- */
constexpr size_t kTempHeader = 64;
constexpr size_t kMaxWaves = 3072; /* what the temp-size queries assume at most (MI355X: 256 CUs x 12) */

/* Literals_Length / Match_Length codes: baseline | extra bits << 24 */
__constant__ static const uint32_t kLLCode[36] = {
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,
    16 | 1u << 24, 18 | 1u << 24, 20 | 1u << 24, 22 | 1u << 24, 24 | 2u << 24, 28 | 2u << 24, 32 | 3u << 24,
    40 | 3u << 24, 48 | 4u << 24, 64 | 6u << 24, 128 | 7u << 24, 256 | 8u << 24, 512 | 9u << 24, 1024 | 10u << 24,
    2048 | 11u << 24, 4096 | 12u << 24, 8192 | 13u << 24, 16384 | 14u << 24, 32768 | 15u << 24, 65536 | 16u << 24};
__constant__ static const uint32_t kMLCode[53] = {
    3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
    33, 34, 35 | 1u << 24, 37 | 1u << 24, 39 | 1u << 24, 41 | 1u << 24, 43 | 2u << 24, 47 | 2u << 24, 51 | 3u << 24,
    59 | 3u << 24, 67 | 4u << 24, 83 | 4u << 24, 99 | 5u << 24, 131 | 7u << 24, 259 | 8u << 24, 515 | 9u << 24,
    1027 | 10u << 24, 2051 | 11u << 24, 4099 | 12u << 24, 8195 | 13u << 24, 16387 | 14u << 24, 32771 | 15u << 24,
    65539 | 16u << 24};
/* predefined distributions (RFC 8878 3.1.1.3.2.2) */
__constant__ static const int8_t kLLDefault[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                                                   2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
__constant__ static const int8_t kMLDefault[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                                   1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                                   1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
__constant__ static const int8_t kOFDefault[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1,
                                                   1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};

__device__ __forceinline__ uint32_t highbit(uint32_t v) /* v > 0 */
{
  return 31u - (uint32_t)__builtin_clz(v);
}

/* ---- the chunk's bytes: every read bounded by its length ---- */
struct Src
{
  const uint8_t* p;
  uint32_t n;
  __device__ __forceinline__ uint32_t u8(uint32_t i) const { return i < n ? wave::gload_u8(p + i) : 0u; }
  /* little-endian, bytes at or beyond n read as zero */
  __device__ __forceinline__ uint32_t le(uint32_t i, uint32_t bytes) const
  {
    uint32_t v = 0;
    for (uint32_t k = 0; k < bytes; ++k) {
      v |= u8(i + k) << (8 * k);
    }
    return v;
  }
  __device__ __forceinline__ uint64_t le64(uint32_t i) const
  {
    if (i + 8 <= n) {
      return wave::gload_u64(p + i);
    }
    return (uint64_t)le(i, 4) | ((uint64_t)le(i + 4, 4) << 32);
  }
};

/* ---- backward bit reader (RFC 8878 4.1: streams are read from their end, the last byte holds a padding bit) ----
 * Container semantics of libzstd's BIT_DStream: `used` bits of the 64-bit container have been consumed from the top;
 * bits in front of the stream's first byte read as zero. */
enum : uint32_t { kUnfinished = 0, kEndOfBuffer = 1, kCompleted = 2, kOverflow = 3 };

struct BitR
{
  const uint8_t* start; /* first byte of the stream (inside the chunk) */
  uint32_t ptr;         /* byte offset of the container's first byte */
  uint32_t used;
  uint64_t c;

  /* false: empty stream or no padding bit */
  __device__ __forceinline__ bool init(const uint8_t* s, uint32_t size)
  {
    start = s;
    if (size == 0) {
      return false;
    }
    const uint32_t last = wave::gload_u8(s + size - 1);
    if (last == 0) {
      return false;
    }
    if (size >= 8) {
      ptr = size - 8;
      c = wave::gload_u64(s + ptr);
      used = 8 - highbit(last);
    } else {
      ptr = 0;
      c = 0;
      for (uint32_t k = 0; k < size; ++k) {
        c |= (uint64_t)wave::gload_u8(s + k) << (8 * k);
      }
      used = 8 - highbit(last) + 8 * (8 - size);
    }
    return true;
  }
  __device__ __forceinline__ uint32_t peek(uint32_t n) const /* 1 <= n <= 32 */
  {
    return used >= 64 ? 0u : (uint32_t)((c << used) >> (64 - n));
  }
  __device__ __forceinline__ uint32_t read(uint32_t n) /* 0 <= n <= 32 */
  {
    const uint32_t v = n == 0 ? 0u : peek(n);
    used += n;
    return v;
  }
  __device__ __forceinline__ uint32_t reload()
  {
    if (used > 64) {
      return kOverflow;
    }
    if (ptr >= 8) {
      ptr -= used >> 3;
      used &= 7;
      c = wave::gload_u64(start + ptr);
      return kUnfinished;
    }
    if (ptr == 0) {
      return used < 64 ? kEndOfBuffer : kCompleted;
    }
    uint32_t nb = used >> 3;
    uint32_t st = kUnfinished;
    if (nb > ptr) {
      nb = ptr;
      st = kEndOfBuffer;
    }
    ptr -= nb;
    used -= 8 * nb;
    c = wave::gload_u64(start + ptr);
    return st;
  }
  __device__ __forceinline__ bool finished() const { return ptr == 0 && used == 64; }
};

/* the same, made wave-uniform after a load (the sequence decoder's reader) */
__device__ __forceinline__ void uniform_reload(BitR& b, uint32_t& st)
{
  st = b.reload();
  b.c = wave::uniform64(b.c);
}

/* ---- FSE table description (RFC 8878 4.1.1): normalized counts into norm[], returns bytes consumed or 0 ---- */
__device__ __forceinline__ uint32_t read_ncount(
    const Src& src, uint32_t at, uint32_t end, int16_t* norm, uint32_t max_sym, uint32_t max_log, uint32_t& log, uint32_t& nsym)
{
  if (at >= end) {
    return 0;
  }
  /* a forward bit position over [at, end) */
  uint32_t bp = 0;
  const uint32_t avail = 8 * (end - at);
  auto bits32 = [&](uint32_t q) -> uint32_t {
    const uint64_t w = src.le64(at + (q >> 3)); /* bytes beyond the chunk read as zero; the position is checked below */
    return (uint32_t)(w >> (q & 7u));
  };
  log = (src.u8(at) & 15u) + 5;
  if (log > max_log) {
    return 0;
  }
  bp = 4;
  int32_t remaining = (1 << log) + 1;
  int32_t threshold = 1 << log;
  uint32_t nb = log + 1;
  uint32_t sym = 0;
  bool prev0 = false;
  while (remaining > 1 && sym <= max_sym) {
    if (bp > avail) {
      return 0;
    }
    if (prev0) {
      uint32_t n0 = sym;
      while ((bits32(bp) & 0xFFFFu) == 0xFFFFu) {
        n0 += 24;
        bp += 16;
        if (bp > avail || n0 > max_sym + 1) {
          return 0;
        }
      }
      while ((bits32(bp) & 3u) == 3u) {
        n0 += 3;
        bp += 2;
        if (bp > avail || n0 > max_sym + 1) {
          return 0;
        }
      }
      n0 += bits32(bp) & 3u;
      bp += 2;
      if (n0 > max_sym + 1 || bp > avail) {
        return 0;
      }
      while (sym < n0) {
        norm[sym++] = 0;
      }
      if (sym > max_sym) {
        break;
      }
    }
    const int32_t mx = (2 * threshold - 1) - remaining;
    const uint32_t v = bits32(bp);
    int32_t count;
    if ((int32_t)(v & (uint32_t)(threshold - 1)) < mx) {
      count = (int32_t)(v & (uint32_t)(threshold - 1));
      bp += nb - 1;
    } else {
      count = (int32_t)(v & (uint32_t)(2 * threshold - 1));
      if (count >= threshold) {
        count -= mx;
      }
      bp += nb;
    }
    count -= 1;
    remaining -= count < 0 ? -count : count;
    norm[sym++] = (int16_t)count;
    prev0 = count == 0;
    if (remaining < 1) {
      return 0;
    }
    while (remaining < threshold) {
      nb -= 1;
      threshold >>= 1;
    }
  }
  if (remaining != 1 || bp > avail || sym == 0) {
    return 0;
  }
  nsym = sym;
  return (bp + 7) >> 3;
}

/* Spread normalized counts into a decoding table (RFC 8878 4.1.1): cell = x << 6 | symbol. The spread is serial by
 * nature (a cell's place depends on every cell before it); lane 0 builds the table, the wave waits for it. `next` is
 * scratch of nsym u16. */
__device__ __forceinline__ void build_fse(uint16_t* table, const int16_t* norm, uint16_t* next, uint32_t nsym, uint32_t log)
{
  if (wave::lane_id() == 0) {
    const uint32_t size = 1u << log;
    uint32_t high = size - 1;
    for (uint32_t s = 0; s < nsym; ++s) {
      const int32_t c = norm[s];
      if (c == -1) {
        table[high] = (uint16_t)s;
        high -= 1;
        next[s] = 1;
      } else {
        next[s] = (uint16_t)c;
      }
    }
    const uint32_t step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; ++s) {
      const int32_t c = norm[s];
      for (int32_t i = 0; i < c; ++i) {
        table[pos] = (uint16_t)s;
        do { /* step is odd: the walk visits every cell; high + 1 of them take the positive counts */
          pos = (pos + step) & mask;
        } while (pos > high);
      }
    }
    for (uint32_t u = 0; u < size; ++u) {
      const uint32_t s = table[u] & 63u;
      const uint32_t x = next[s];
      next[s] = (uint16_t)(x + 1);
      table[u] = (uint16_t)((x << 6) | s);
    }
  }
  wave::sync();
}

__device__ __forceinline__ void build_rle(uint16_t* table, uint32_t sym)
{
  table[0] = (uint16_t)((1u << 6) | sym);
  wave::sync();
}

/* An FSE state: the cell it points at, read wave-uniformly */
struct State
{
  uint32_t s;   /* state value (index into the table) */
  uint32_t log;
  const uint16_t* table;
  __device__ __forceinline__ uint32_t cell() const { return wave::uniform(table[s]); }
};

/* next state of a cell: baseline + bits read */
__device__ __forceinline__ void fse_update(State& st, uint32_t cell, BitR& b)
{
  const uint32_t x = cell >> 6;
  const uint32_t nb = st.log - highbit(x);
  st.s = ((x << nb) - (1u << st.log)) + b.read(nb);
}

/* ---- Huffman ---- */

/* Huffman tree description (RFC 8878 4.2.1) at [at, end): builds the lookup table; returns bytes consumed or 0. */
__device__ __forceinline__ uint32_t read_huffman(const Src& src, uint32_t at, uint32_t end, uint8_t* lds, uint32_t& max_bits)
{
  uint8_t* weights = lds + kOffTmp;
  int16_t* norm = (int16_t*)(lds + kOffTmp + 256);
  uint16_t* next = (uint16_t*)(lds + kOffTmp + 384);
  uint16_t* lut = (uint16_t*)(lds + kOffHuf);
  const uint32_t lane = (uint32_t)wave::lane_id();
  if (at >= end) {
    return 0;
  }
  const uint32_t hb = src.u8(at);
  uint32_t nw = 0, used = 0;
  if (hb >= 128) {
    /* direct: 4 bits per weight */
    nw = hb - 127;
    used = 1 + (nw + 1) / 2;
    if (at + used > end) {
      return 0;
    }
    for (uint32_t k = lane; k < nw; k += 64) {
      const uint32_t byte = src.u8(at + 1 + k / 2);
      weights[k] = (uint8_t)(k & 1u ? byte & 15u : byte >> 4);
    }
    wave::sync();
  } else {
    /* FSE-compressed weights: a table of accuracy <= 6, two interleaved states over a backward stream */
    const uint32_t csize = hb;
    used = 1 + csize;
    if (csize == 0 || at + used > end) {
      return 0;
    }
    uint32_t log = 0, nsym = 0;
    const uint32_t hdr = read_ncount(src, at + 1, at + 1 + csize, norm, 12, 6, log, nsym);
    wave::sync();
    if (hdr == 0 || hdr >= csize) {
      return 0;
    }
    /* the weights' FSE table: 64 cells at the end of the lookup table's space, which is rebuilt behind it */
    uint16_t* table = (uint16_t*)(lds + kOffHuf + 4096 - 128);
    build_fse(table, norm, next, nsym, log);
    BitR b;
    if (!b.init(src.p + at + 1 + hdr, csize - hdr)) {
      return 0;
    }
    b.c = wave::uniform64(b.c);
    State s1 = {b.read(log), log, table};
    State s2 = {b.read(log), log, table};
    uint32_t st = b.reload();
    b.c = wave::uniform64(b.c);
    if (st == kOverflow) {
      return 0;
    }
    for (;;) {
      if (nw > 253) {
        return 0;
      }
      uint32_t c1 = s1.cell();
      weights[nw++] = (uint8_t)(c1 & 63u);
      fse_update(s1, c1, b);
      uniform_reload(b, st);
      if (st == kOverflow) {
        weights[nw++] = (uint8_t)(s2.cell() & 63u);
        break;
      }
      const uint32_t c2 = s2.cell();
      weights[nw++] = (uint8_t)(c2 & 63u);
      fse_update(s2, c2, b);
      uniform_reload(b, st);
      if (st == kOverflow) {
        weights[nw++] = (uint8_t)(s1.cell() & 63u);
        break;
      }
    }
    wave::sync();
  }
  if (nw == 0 || nw > 255) {
    return 0;
  }
  /* the weights must complete a code: the implied last weight fills the sum up to the next power of two */
  uint32_t total = 0;
  for (uint32_t k = lane; k < nw; k += 64) {
    const uint32_t w = weights[k];
    total += w > kHufMaxBits + 1 ? 1u << 20 : w ? 1u << (w - 1) : 0u;
  }
  total = wave::reduce_add(total);
  if (total == 0 || total >= (1u << kHufMaxBits)) {
    return 0;
  }
  const uint32_t mb = highbit(total) + 1;
  const uint32_t rest = (1u << mb) - total;
  if ((rest & (rest - 1)) != 0) {
    return 0;
  }
  const uint32_t last_w = highbit(rest) + 1;
  weights[nw] = (uint8_t)last_w;
  const uint32_t nsym = nw + 1;
  wave::sync();
  /* rank starts: weight w's codes take (count_w << (w - 1)) cells, weights in ascending order */
  uint32_t* rank = (uint32_t*)(lds + kOffTmp + 256); /* u32[16], over the norm / next scratch (done with) */
  {
    uint32_t cnt = 0;
    if (lane >= 1 && lane <= mb) {
      for (uint32_t k = 0; k < nsym; ++k) {
        cnt += weights[k] == lane ? 1u : 0u;
      }
    }
    const uint32_t cells = lane >= 1 && lane <= mb ? cnt << (lane - 1) : 0u;
    const uint32_t incl = wave::scan_add_inclusive(cells);
    wave::sync();
    if (lane < 16) {
      rank[lane] = incl - cells;
    }
    wave::sync();
  }
  for (uint32_t k = 0; k < nsym; ++k) {
    const uint32_t w = wave::uniform(weights[k]);
    if (w == 0) {
      continue;
    }
    const uint32_t len = 1u << (w - 1);
    const uint32_t first = wave::uniform(rank[w]);
    const uint16_t e = (uint16_t)(k | ((mb + 1 - w) << 8));
    for (uint32_t i = lane; i < len; i += 64) {
      lut[first + i] = e;
    }
    wave::sync();
    rank[w] = first + len;
    wave::sync();
  }
  max_bits = mb;
  return used;
}

/* Decode `count` literals of one Huffman stream [s, s + size) to dst (per lane; lanes that do not take part pass
 * size 0). Returns false on a malformed stream. */
__device__ __forceinline__ bool huf_stream(const uint16_t* lut, uint32_t mb, const uint8_t* s, uint32_t size, uint8_t* dst, uint32_t count)
{
  BitR b;
  if (!b.init(s, size)) {
    return false;
  }
  uint32_t acc = 0, k = 0;
  while (k < count) {
    if (b.reload() == kOverflow) {
      return false;
    }
    /* four symbols of at most 11 bits fit the 57 bits a reload leaves (fewer near the stream's start: zeros) */
    const uint32_t burst = count - k < 4 ? count - k : 4u;
    for (uint32_t j = 0; j < burst; ++j) {
      const uint32_t e = lut[b.peek(mb)];
      b.used += e >> 8;
      acc |= (e & 255u) << (8 * (k & 3u));
      k += 1;
      if ((k & 3u) == 0) {
        wave::gstore_u32(dst + k - 4, acc);
        acc = 0;
      }
    }
  }
  for (uint32_t j = 0; j < (k & 3u); ++j) {
    wave::gstore_u8(dst + (k & ~3u) + j, acc >> (8 * j));
  }
  b.reload();
  return b.finished();
}

/* ---- sequence records and the batch executor ---- */
struct Batch
{
  lzw::InRing ring; /* the literal ring in the executor's clothes */
  lz::Seq s;        /* record k in lane k */
  uint32_t n;       /* records in hand */
  uint32_t bytes;   /* output bytes they produce */
  uint32_t lit_lo;  /* first literal (slot position) of the batch */
  uint32_t lp;      /* next literal to hand out */
};

__device__ __forceinline__ void batch_clear(Batch& bt)
{
  bt.s.lit_src = 0, bt.s.lit_len = 0, bt.s.match_off = 0, bt.s.match_len = 0;
  bt.n = 0;
  bt.bytes = 0;
  bt.lit_lo = bt.lp;
}

/* Execute the records in hand: their literals slot -> ring, then the window executor. */
__device__ __forceinline__ bool flush(Batch& bt, const uint8_t* slot, lzw::OutWindow& ow, uint32_t cap, uint32_t& op, uint32_t& err)
{
  if (bt.n == 0) {
    return true;
  }
  const uint32_t lane = (uint32_t)wave::lane_id();
  for (uint32_t v = bt.lit_lo + lane; v < bt.lp; v += 64) {
    const uint8_t x = (uint8_t)wave::gload_u8(slot + v);
    const uint32_t at = v & (lzw::kInRing - 1);
    bt.ring.ring[at] = x;
    if (at < 16) {
      bt.ring.ring[lzw::kInRing + at] = x; /* the mirror the executor's dword reads rely on */
    }
  }
  bt.ring.lo = bt.lit_lo;
  bt.ring.hi = bt.lp;
  wave::sync();
  bool big = false;
  const uint32_t took = lzw::execute_window_batch<true, true>(bt.ring, ow, cap, op, bt.n, bt.s, err, big);
  if (err) {
    return false;
  }
  if (took != bt.n || big) { /* cannot happen: a batch is cut at lzw::kBatchMax bytes */
    err |= lz::kErrInput;
    return false;
  }
  wave::sync();
  batch_clear(bt);
  return true;
}

/* One sequence (wave-uniform): ll literals from the slot, then ml bytes from `off` back; split into records so that a
 * batch never produces more than kBatchMax bytes. */
__device__ __forceinline__ bool emit(
    Batch& bt, uint32_t ll, uint32_t ml, uint32_t off, const uint8_t* slot, lzw::OutWindow& ow, uint32_t cap, uint32_t& op, uint32_t& err)
{
  while (ll != 0 || ml != 0) {
    const uint32_t room = lzw::kBatchMax - bt.bytes;
    if (bt.n == 64 || room == 0) {
      if (!flush(bt, slot, ow, cap, op, err)) {
        return false;
      }
      continue;
    }
    const uint32_t l = ll < room ? ll : room;
    const uint32_t m = l == ll ? (ml < room - l ? ml : room - l) : 0u;
    bt.s.lit_src = wave::write_lane(bt.s.lit_src, bt.lp, bt.n);
    bt.s.lit_len = wave::write_lane(bt.s.lit_len, l, bt.n);
    bt.s.match_off = wave::write_lane(bt.s.match_off, m ? off : 0u, bt.n);
    bt.s.match_len = wave::write_lane(bt.s.match_len, m, bt.n);
    bt.n += 1;
    bt.bytes += l + m;
    bt.lp += l;
    ll -= l;
    ml -= m;
  }
  return true;
}

/* ---- what persists across the blocks of a frame ---- */
struct FrameState
{
  uint32_t rep0, rep1, rep2;
  uint32_t huf_bits; /* 0: no Huffman table yet */
  uint32_t ll_log, ml_log, of_log;
  bool ll_ok, ml_ok, of_ok; /* a table exists for the repeat mode */
};

/* Symbol compression mode of one of LL / OF / ML: sets up its table; returns the bytes of description consumed, or
 * ~0u on error. */
__device__ __forceinline__ uint32_t setup_table(
    const Src& src, uint32_t at, uint32_t end, uint32_t mode, uint8_t* lds, uint16_t* table, const int8_t* def, uint32_t def_n,
    uint32_t def_log, uint32_t max_sym, uint32_t max_log, uint32_t& log, bool& ok)
{
  int16_t* norm = (int16_t*)(lds + kOffTmp + 256);
  uint16_t* next = (uint16_t*)(lds + kOffTmp + 384);
  const uint32_t lane = (uint32_t)wave::lane_id();
  if (mode == 0) { /* predefined */
    if (lane < def_n) {
      norm[lane] = def[lane];
    }
    wave::sync();
    build_fse(table, norm, next, def_n, def_log);
    log = def_log;
    ok = true;
    return 0;
  }
  if (mode == 1) { /* RLE */
    if (at >= end) {
      return ~0u;
    }
    const uint32_t sym = wave::uniform(src.u8(at));
    if (sym > max_sym) {
      return ~0u;
    }
    build_rle(table, sym);
    log = 0;
    ok = true;
    return 1;
  }
  if (mode == 2) { /* FSE-compressed */
    uint32_t nsym = 0, lg = 0;
    const uint32_t used = read_ncount(src, at, end, norm, max_sym, max_log, lg, nsym);
    wave::sync();
    if (used == 0) {
      return ~0u;
    }
    build_fse(table, norm, next, nsym, lg);
    log = lg;
    ok = true;
    return used;
  }
  return ok ? 0u : ~0u; /* repeat: the previous block's table */
}

/*
 * Decode one chunk: one or more frames (skippable ones included) into out[0, cap). `slot` is the wave's literal slot
 * of slot_cap bytes. Returns the bytes produced; err != 0 on failure (kUnsupported: a frame needs a dictionary).
 */
__device__ __forceinline__ uint32_t decode_chunk(
    const uint8_t* __restrict__ in, uint32_t in_len, uint8_t* out, uint32_t cap, uint8_t* lds, uint8_t* slot, uint32_t slot_cap,
    uint32_t& err)
{
  const uint32_t lane = (uint32_t)wave::lane_id();
  err = lz::kErrNone;
  const Src src = {in, in_len};
  lzw::OutWindow ow;
  lzw::out_init(ow, out, lds + kOffWin);
  Batch bt;
  bt.ring.base = nullptr;
  bt.ring.ring = lds + kOffRing;
  bt.ring.vbeg = 0, bt.ring.vend = ~0u, bt.ring.lo = 0, bt.ring.hi = 0;
  bt.lp = 0;
  batch_clear(bt);
  uint16_t* const ll_t = (uint16_t*)(lds + kOffLL);
  uint16_t* const ml_t = (uint16_t*)(lds + kOffML);
  uint16_t* const of_t = (uint16_t*)(lds + kOffOF);
  const uint16_t* const lut = (const uint16_t*)(lds + kOffHuf);

  uint32_t op = 0;
  uint32_t pos = 0;
  if (in_len == 0) {
    err = lz::kErrInput;
    return 0;
  }
  while (pos < in_len) {
    if (in_len - pos < 4) {
      err |= lz::kErrInput;
      return 0;
    }
    const uint32_t magic = wave::uniform(src.le(pos, 4));
    if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) { /* skippable frame */
      if (in_len - pos < 8) {
        err |= lz::kErrInput;
        return 0;
      }
      const uint32_t fsize = wave::uniform(src.le(pos + 4, 4));
      if (fsize > in_len - pos - 8) {
        err |= lz::kErrInput;
        return 0;
      }
      pos += 8 + fsize;
      continue;
    }
    if (magic != kMagic) {
      err |= lz::kErrInput;
      return 0;
    }
    /* ---- frame header ---- */
    pos += 4;
    const uint32_t fhd = wave::uniform(src.u8(pos));
    const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, checksum = (fhd >> 2) & 1u, did_flag = fhd & 3u;
    if (pos >= in_len || (fhd & 8u) != 0) { /* reserved bit */
      err |= lz::kErrInput;
      return 0;
    }
    pos += 1;
    if (!single) {
      const uint32_t wd = wave::uniform(src.u8(pos));
      if ((wd >> 3) + 10 > 41) { /* window log beyond 41 */
        err |= lz::kErrInput;
        return 0;
      }
      pos += 1;
    }
    const uint32_t did_bytes = did_flag == 3 ? 4u : did_flag;
    const uint32_t did = wave::uniform(src.le(pos, did_bytes));
    pos += did_bytes;
    const uint32_t fcs_bytes = fcs_flag == 0 ? single : fcs_flag == 1 ? 2u : fcs_flag == 2 ? 4u : 8u;
    uint64_t fcs = 0;
    if (fcs_bytes == 8) {
      fcs = (uint64_t)wave::uniform(src.le(pos, 4)) | ((uint64_t)wave::uniform(src.le(pos + 4, 4)) << 32);
    } else if (fcs_bytes) {
      fcs = wave::uniform(src.le(pos, fcs_bytes)) + (fcs_bytes == 2 ? 256u : 0u);
    }
    pos += fcs_bytes;
    if (pos > in_len) {
      err |= lz::kErrInput;
      return 0;
    }
    if (did != 0) {
      err |= kUnsupported;
      return 0;
    }
    if (fcs_bytes && fcs > (uint64_t)(cap - op)) {
      err |= lz::kErrOutput;
      return 0;
    }
    const uint32_t frame_start = op;
    FrameState fs;
    fs.rep0 = 1, fs.rep1 = 4, fs.rep2 = 8;
    fs.huf_bits = 0;
    fs.ll_log = fs.ml_log = fs.of_log = 0;
    fs.ll_ok = fs.ml_ok = fs.of_ok = false;
    /* ---- blocks ---- */
    for (;;) {
      if (in_len - pos < 3) {
        err |= lz::kErrInput;
        return 0;
      }
      const uint32_t bh = wave::uniform(src.le(pos, 3));
      pos += 3;
      const uint32_t last = bh & 1u, type = (bh >> 1) & 3u, bsize = bh >> 3;
      if (type == 3 || bsize > kBlockMax) {
        err |= lz::kErrInput;
        return 0;
      }
      if (type == 0 || type == 1) {
        const uint32_t need = type == 0 ? bsize : 1u; /* an RLE block carries its byte even when it repeats it 0 times */
        if (need > in_len - pos) {
          err |= lz::kErrInput;
          return 0;
        }
        if (bsize > cap - op) {
          err |= lz::kErrOutput;
          return 0;
        }
        if (bsize) {
          lzw::out_flush_all(ow, op);
          wave::sync();
          if (type == 0) {
            lzw::stream_copy(out + op, in + pos, bsize);
          } else {
            const uint32_t byte = wave::uniform(src.u8(pos));
            const uint32_t word = byte * 0x01010101u;
            uint8_t* d = out + op;
            const uint32_t head = (16u - (uint32_t)((uintptr_t)d & 15u)) & 15u;
            const uint32_t h = head < bsize ? head : bsize;
            if (lane < h) {
              wave::gstore_u8(d + lane, byte);
            }
            const uint32_t body_end = h + ((bsize - h) & ~15u);
            const wave::u32x4 q = {word, word, word, word};
            for (uint32_t at = h + 16 * lane; at < body_end; at += 1024) {
              wave::gstore_u32x4_aligned(d + at, q);
            }
            if (body_end + lane < bsize) {
              wave::gstore_u8(d + body_end + lane, byte);
            }
          }
          wave::sync();
          op += bsize;
          lzw::restart_window(ow, op);
        }
        pos += need;
      } else {
        /* ---- compressed block ---- */
        if (bsize > in_len - pos || bsize == 0) {
          err |= lz::kErrInput;
          return 0;
        }
        const uint32_t bend = pos + bsize;
        uint32_t p = pos;
        /* literals section header */
        const uint32_t h0 = wave::uniform(src.u8(p));
        const uint32_t lt = h0 & 3u, sf = (h0 >> 2) & 3u;
        uint32_t regen = 0, csize = 0, hl = 0, streams = 1;
        if (lt <= 1) {
          if ((sf & 1u) == 0) {
            hl = 1, regen = h0 >> 3;
          } else if (sf == 1) {
            hl = 2, regen = (h0 >> 4) + (wave::uniform(src.u8(p + 1)) << 4);
          } else {
            hl = 3, regen = (h0 >> 4) + (wave::uniform(src.le(p + 1, 2)) << 4);
          }
        } else {
          streams = sf == 0 ? 1u : 4u;
          hl = sf <= 1 ? 3u : sf == 2 ? 4u : 5u;
          const uint64_t v = (uint64_t)wave::uniform(src.le(p, 4)) | ((uint64_t)wave::uniform(src.u8(p + 4)) << 32);
          const uint32_t bits = sf <= 1 ? 10u : sf == 2 ? 14u : 18u;
          regen = (uint32_t)(v >> 4) & ((1u << bits) - 1u);
          csize = (uint32_t)(v >> (4 + bits)) & ((1u << bits) - 1u);
        }
        if (hl > bend - p || regen > kBlockMax || regen > slot_cap) {
          err |= lz::kErrInput;
          return 0;
        }
        p += hl;
        if (lt == 0) { /* raw */
          if (regen > bend - p) {
            err |= lz::kErrInput;
            return 0;
          }
          lzw::stream_copy(slot, in + p, regen);
          p += regen;
        } else if (lt == 1) { /* RLE */
          if (p >= bend) {
            err |= lz::kErrInput;
            return 0;
          }
          const uint32_t byte = wave::uniform(src.u8(p));
          for (uint32_t k = lane; k < regen; k += 64) {
            wave::gstore_u8(slot + k, byte);
          }
          p += 1;
        } else { /* Huffman-compressed or treeless */
          if (csize > bend - p || regen == 0 || (streams == 4 && regen < 4)) {
            err |= lz::kErrInput;
            return 0;
          }
          const uint32_t lend = p + csize;
          uint32_t q = p;
          if (lt == 2) {
            uint32_t mb = 0;
            const uint32_t used = read_huffman(src, q, lend, lds, mb);
            if (used == 0) {
              err |= lz::kErrInput;
              return 0;
            }
            fs.huf_bits = mb;
            q += used;
          } else if (fs.huf_bits == 0) {
            err |= lz::kErrInput;
            return 0;
          }
          /* stream bounds: one stream, or a 6-byte jump table of the first three sizes */
          uint32_t s_at[4] = {q, 0, 0, 0}, s_len[4] = {lend - q, 0, 0, 0}, s_cnt[4] = {regen, 0, 0, 0};
          if (streams == 4) {
            if (lend - q < 6) {
              err |= lz::kErrInput;
              return 0;
            }
            const uint32_t a = wave::uniform(src.le(q, 2)), b2 = wave::uniform(src.le(q + 2, 2)), c2 = wave::uniform(src.le(q + 4, 2));
            const uint32_t total = lend - q - 6;
            if ((uint64_t)a + b2 + c2 > total) {
              err |= lz::kErrInput;
              return 0;
            }
            const uint32_t seg = (regen + 3) / 4;
            if (3 * seg > regen) {
              err |= lz::kErrInput;
              return 0;
            }
            s_at[0] = q + 6, s_len[0] = a;
            s_at[1] = s_at[0] + a, s_len[1] = b2;
            s_at[2] = s_at[1] + b2, s_len[2] = c2;
            s_at[3] = s_at[2] + c2, s_len[3] = total - a - b2 - c2;
            s_cnt[0] = s_cnt[1] = s_cnt[2] = seg;
            s_cnt[3] = regen - 3 * seg;
          }
          /* lane k decodes stream k (the selects keep the arrays in registers) */
          const uint32_t my_at = lane == 0 ? s_at[0] : lane == 1 ? s_at[1] : lane == 2 ? s_at[2] : s_at[3];
          const uint32_t my_len = lane == 0 ? s_len[0] : lane == 1 ? s_len[1] : lane == 2 ? s_len[2] : s_len[3];
          const uint32_t my_cnt = lane == 0 ? s_cnt[0] : lane == 1 ? s_cnt[1] : lane == 2 ? s_cnt[2] : s_cnt[3];
          const uint32_t my_dst = lane == 0 ? 0u : lane * s_cnt[0];
          bool ok = true;
          if (lane < streams) {
            ok = huf_stream(lut, fs.huf_bits, in + my_at, my_len, slot + my_dst, my_cnt);
          }
          if (wave::ballot(!ok)) {
            err |= lz::kErrInput;
            return 0;
          }
          p = lend;
        }
        wave::sync(); /* the slot's literals are visible to every lane */
        /* ---- sequences section ---- */
        if (p >= bend) {
          err |= lz::kErrInput;
          return 0;
        }
        const uint32_t b0 = wave::uniform(src.u8(p));
        uint32_t nseq = 0;
        if (b0 < 128) {
          nseq = b0, p += 1;
        } else if (b0 < 255) {
          nseq = ((b0 - 128) << 8) + wave::uniform(src.u8(p + 1)), p += 2;
        } else {
          nseq = wave::uniform(src.le(p + 1, 2)) + 0x7F00u, p += 3;
        }
        if (p > bend) {
          err |= lz::kErrInput;
          return 0;
        }
        bt.lp = 0;
        batch_clear(bt);
        uint32_t pos_in_frame = op - frame_start; /* output position of the next sequence, frame-relative */
        if (nseq != 0) {
          if (p >= bend) {
            err |= lz::kErrInput;
            return 0;
          }
          const uint32_t modes = wave::uniform(src.u8(p));
          p += 1;
          if (modes & 3u) {
            err |= lz::kErrInput;
            return 0;
          }
          uint32_t u = setup_table(src, p, bend, modes >> 6, lds, ll_t, kLLDefault, 36, 6, kLLMaxSym, kLLMaxLog, fs.ll_log, fs.ll_ok);
          if (u == ~0u) {
            err |= lz::kErrInput;
            return 0;
          }
          p += u;
          u = setup_table(src, p, bend, (modes >> 4) & 3u, lds, of_t, kOFDefault, 29, 5, kOFMaxSym, kOFMaxLog, fs.of_log, fs.of_ok);
          if (u == ~0u) {
            err |= lz::kErrInput;
            return 0;
          }
          p += u;
          u = setup_table(src, p, bend, (modes >> 2) & 3u, lds, ml_t, kMLDefault, 53, 6, kMLMaxSym, kMLMaxLog, fs.ml_log, fs.ml_ok);
          if (u == ~0u || p + u >= bend) {
            err |= lz::kErrInput;
            return 0;
          }
          p += u;
          wave::sync();
          BitR b;
          if (!b.init(in + p, bend - p)) {
            err |= lz::kErrInput;
            return 0;
          }
          b.c = wave::uniform64(b.c);
          State sl = {0, fs.ll_log, ll_t}, so = {0, fs.of_log, of_t}, sm = {0, fs.ml_log, ml_t};
          sl.s = b.read(sl.log);
          so.s = b.read(so.log);
          sm.s = b.read(sm.log);
          uint32_t st = 0;
          uniform_reload(b, st);
          for (uint32_t k = 0; k < nseq; ++k) {
            if (st == kOverflow) {
              err |= lz::kErrInput;
              return 0;
            }
            const uint32_t cl = sl.cell(), co = so.cell(), cm = sm.cell();
            const uint32_t llc = cl & 63u, ofc = co & 63u, mlc = cm & 63u;
            /* offset, then match length, then literal length */
            const uint32_t ofv = (1u << ofc) + b.read(ofc); /* ofc <= 31: read() takes up to 32 bits */
            uniform_reload(b, st);
            const uint32_t mle = kMLCode[mlc];
            const uint32_t ml = (mle & 0xFFFFFFu) + b.read(mle >> 24);
            const uint32_t lle = kLLCode[llc];
            const uint32_t ll = (lle & 0xFFFFFFu) + b.read(lle >> 24);
            uniform_reload(b, st);
            uint32_t off;
            if (ofv > 3) {
              off = ofv - 3;
              fs.rep2 = fs.rep1, fs.rep1 = fs.rep0, fs.rep0 = off;
            } else {
              const uint32_t idx = ofv - 1 + (ll == 0 ? 1u : 0u);
              if (idx == 0) {
                off = fs.rep0;
              } else if (idx == 1) {
                off = fs.rep1;
                fs.rep1 = fs.rep0, fs.rep0 = off;
              } else if (idx == 2) {
                off = fs.rep2;
                fs.rep2 = fs.rep1, fs.rep1 = fs.rep0, fs.rep0 = off;
              } else {
                off = fs.rep0 - 1;
                fs.rep2 = fs.rep1, fs.rep1 = fs.rep0, fs.rep0 = off;
              }
            }
            /* the literals must exist, the match must stay inside the frame's output */
            if (ll > regen - bt.lp || off == 0 || (uint64_t)off > (uint64_t)pos_in_frame + ll
                || (uint64_t)ll + ml > (uint64_t)(cap - op - bt.bytes)) {
              err |= off == 0 || (uint64_t)off > (uint64_t)pos_in_frame + ll ? lz::kErrOffset : lz::kErrInput;
              return 0;
            }
            pos_in_frame += ll + ml;
            if (k + 1 < nseq) { /* states: LL, ML, OF */
              fse_update(sl, cl, b);
              fse_update(sm, cm, b);
              fse_update(so, co, b);
              uniform_reload(b, st);
            }
            if (!emit(bt, ll, ml, off, slot, ow, cap, op, err)) {
              return 0;
            }
          }
          if (st != kCompleted || !b.finished()) {
            err |= lz::kErrInput;
            return 0;
          }
        } else if (p != bend) {
          err |= lz::kErrInput;
          return 0;
        }
        /* the literals behind the last sequence */
        if (regen - bt.lp > cap - op - bt.bytes) {
          err |= lz::kErrOutput;
          return 0;
        }
        if (!emit(bt, regen - bt.lp, 0, 0, slot, ow, cap, op, err) || !flush(bt, slot, ow, cap, op, err)) {
          return 0;
        }
        pos = bend;
      }
      if (last) {
        break;
      }
    }
    if (checksum) {
      if (in_len - pos < 4) {
        err |= lz::kErrInput;
        return 0;
      }
      pos += 4; /* XXH64 content checksum: consumed, not verified */
    }
    if (fcs_bytes && (uint64_t)(op - frame_start) != fcs) {
      err |= lz::kErrInput;
      return 0;
    }
  }
  lzw::out_flush_all(ow, op);
  return op;
}

/* Sum of the frames' Frame_Content_Size; 0 when a frame has none or the chunk is not Zstd. One lane per chunk. */
__device__ __forceinline__ uint64_t content_size(const uint8_t* in, uint32_t in_len)
{
  const Src src = {in, in_len};
  uint64_t sum = 0;
  uint32_t pos = 0;
  if (in_len == 0) {
    return 0;
  }
  while (pos < in_len) {
    if (in_len - pos < 4) {
      return 0;
    }
    const uint32_t magic = src.le(pos, 4);
    if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {
      if (in_len - pos < 8 || src.le(pos + 4, 4) > in_len - pos - 8) {
        return 0;
      }
      pos += 8 + src.le(pos + 4, 4);
      continue;
    }
    if (magic != kMagic) {
      return 0;
    }
    pos += 4;
    const uint32_t fhd = src.u8(pos);
    const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, checksum = (fhd >> 2) & 1u, did_flag = fhd & 3u;
    if ((fhd & 8u) != 0) {
      return 0;
    }
    pos += 1 + (single ? 0u : 1u) + (did_flag == 3 ? 4u : did_flag);
    const uint32_t fcs_bytes = fcs_flag == 0 ? single : fcs_flag == 1 ? 2u : fcs_flag == 2 ? 4u : 8u;
    if (fcs_bytes == 0) {
      return 0;
    }
    if (fcs_bytes == 8) {
      sum += (uint64_t)src.le(pos, 4) | ((uint64_t)src.le(pos + 4, 4) << 32);
    } else {
      sum += src.le(pos, fcs_bytes) + (fcs_bytes == 2 ? 256u : 0u);
    }
    pos += fcs_bytes;
    if (pos > in_len) {
      return 0;
    }
    for (;;) { /* skip the blocks: each header moves on by at least three bytes */
      if (in_len - pos < 3) {
        return 0;
      }
      const uint32_t bh = src.le(pos, 3);
      const uint32_t type = (bh >> 1) & 3u, bsize = bh >> 3;
      const uint32_t need = type == 1 ? 1u : bsize;
      if (type == 3 || need > in_len - pos - 3) {
        return 0;
      }
      pos += 3 + need;
      if (bh & 1u) {
        break;
      }
    }
    if (checksum) {
      if (in_len - pos < 4) {
        return 0;
      }
      pos += 4;
    }
  }
  return sum;
}

} // namespace zstd
