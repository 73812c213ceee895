/*
 * nvcomp/amd_ext.h -- MI355X-build extensions. Nothing here exists in the reference's
 * interface and no reference-side caller needs it. The library has no run-time
 * tuning state: which kernel a batch takes depends on the arguments of the call alone.
 */
#ifndef NVCOMP_AMD_EXT_H
#define NVCOMP_AMD_EXT_H

#include <stddef.h>

#include <hip/hip_runtime_api.h>

#include "nvcomp/shared_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Pack the chunks of a batch (e.g. what nvcompBatched<Fmt>CompressAsync left in its worst-case-sized slots) into one
 * contiguous buffer, in batch order and without gaps: device_offsets[i] = sum of device_chunk_bytes[0..i),
 * device_offsets[batch_size] = the packed size; chunk i is copied to device_packed + device_offsets[i]. Everything
 * happens on `stream`: a device-side prefix sum, then one wavefront per chunk. A chunk that would end behind
 * `packed_capacity` is left out (size the buffer as batch_size x the compressor's declared bound). This is the step
 * between "compress" and "send" of the reference's all-gather benchmark (benchmarks/benchmark_allgather.cpp:322-361
 * moves the whole slots instead); bench.py --allgather is built on it. */
nvcompStatus_t nvcompAmdBatchedPackAsync(
    const void* const* device_chunk_ptrs,
    const size_t* device_chunk_bytes,
    size_t batch_size,
    void* device_packed,
    size_t packed_capacity,
    size_t* device_offsets,
    hipStream_t stream);

/* Inspection entries for tests and scripts, not needed by any caller of the batched API. `resident_places` receives the
 * number of chunks a persistent one-wave LZ4 / Snappy decode launch keeps in flight on the current device (0 when the
 * runtime cannot tell). Where `order_offset` is not NULL, the pass that orders such a launch's last places by compressed
 * size runs alone on `stream`, over the two size arrays of a decompress call, with the places in front of `first_ordered`
 * left to their own chunks: *order_offset is then the offset in `device_temp_ptr` of batch_size chunk indices (uint32),
 * and the first word of the buffer, the launch's ticket, is cleared. nvcompErrorInvalidValue when the buffer is NULL, not
 * 4-byte aligned or too small (16 + 4 x batch_size + 768 bytes for every 1 024 chunks, 64 times at the most), or
 * first_ordered > batch_size. Either result pointer may be NULL. */
nvcompStatus_t nvcompAmdLZ4DecompressOrderAsync(
    const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes,
    size_t first_ordered,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    size_t* order_offset,
    size_t* resident_places,
    hipStream_t stream);
nvcompStatus_t nvcompAmdSnappyDecompressOrderAsync(
    const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes,
    size_t first_ordered,
    size_t batch_size,
    void* device_temp_ptr,
    size_t temp_bytes,
    size_t* order_offset,
    size_t* resident_places,
    hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NVCOMP_AMD_EXT_H */
