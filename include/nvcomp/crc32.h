/*
 * nvcomp/crc32.h -- batched standard CRC-32, low-level C API, MI355X build.
 *
 * nvCOMP 3.0.x's nvcompBatchedCRC32Async (the reference's CHANGELOG.md, 2.5.0: "Added Standard CRC32 support and its
 * LLAPI"). For every chunk it computes the standard CRC-32 (IEEE 802.3: reflected polynomial 0xEDB88320, initial value
 * and final XOR 0xffffffff), equal to zlib's crc32(0, p, n) and boost::crc_32_type.
 *
 *   - Sizes: any size_t below SIZE_MAX; chunks of 2 GiB, 4 GiB and more are fine. A chunk of size 0 gives 0, and its
 *     pointer may then be NULL (it is not read).
 *   - Alignment: none required.
 *   - Arguments: with num_chunks > 0, a NULL pointer array, size array or output gives nvcompErrorInvalidValue and
 *     nothing is launched; num_chunks == 0 gives nvcompSuccess and nothing is launched.
 *   - Stream: one kernel on `stream` (and, when the batch has fewer chunks than the card has resident waves, a memset of
 *     device_crc32_ptr in front of it). No temp buffer, no allocation, no host synchronisation.
 *
 * device_uncompressed_chunk_ptrs, device_uncompressed_chunk_bytes (num_chunks each) and device_crc32_ptr (num_chunks
 * uint32_t) must be dereferenceable by the GPU that owns `stream`.
 */
#ifndef NVCOMP_CRC32_H
#define NVCOMP_CRC32_H

#include "shared_types.h"
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

static const size_t nvcompCRC32RequiredAlignment = 1;

nvcompStatus_t nvcompBatchedCRC32Async(
    const void* const* device_uncompressed_chunk_ptrs,
    const size_t* device_uncompressed_chunk_bytes,
    size_t num_chunks,
    uint32_t* device_crc32_ptr,
    hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NVCOMP_CRC32_H */
