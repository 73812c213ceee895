/*
 * snappy/snappy_preamble.hip.h -- the varint32 preamble of a Snappy raw-format stream: the uncompressed length, which is
 * all nvcompBatchedSnappyGetDecompressSizeAsync reads, and what the decoders check their output against. The elements
 * behind it are decoded in snappy_decode_window.hip.h.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snappy {

/* The varint32 preamble (uncompressed length) straight from memory, by every lane alike. False: malformed -- the stream
 * ends inside it, or it does not fit 32 bits (a fifth byte above 15, or with its continuation bit set). Accepts exactly
 * what snappyw::read_preamble() (through the stream ring) accepts. */
__device__ __forceinline__ bool preamble(const uint8_t* __restrict__ in, uint32_t in_len, uint32_t& total)
{
  total = 0;
  for (uint32_t i = 0; i < 5 && i < in_len; ++i) {
    const uint32_t b = in[i];
    total |= (b & 127u) << (7 * i);
    if (!(b & 128u)) {
      return !(i == 4 && b > 15u);
    }
  }
  return false;
}

/* Uncompressed length from the preamble; 0 if malformed. */
__device__ __forceinline__ uint32_t decoded_size(const uint8_t* __restrict__ in, uint32_t in_len, bool& ok)
{
  uint32_t total;
  ok = preamble(in, in_len, total);
  return ok ? total : 0;
}

} // namespace snappy
