/*
 * nvcomp/zstd.h -- batched Zstandard (RFC 8878) decompression, low-level C API, MI355X build.
 *
 * The nvCOMP 3.0.x decompression entry points of nvcompBatchedZstd*. Chunks are written by CPU libzstd (Parquet, ORC
 * and Arrow IPC pages, .zst files) and read back here. Decompression only: this library exports no Zstd compressor.
 *
 * What a chunk may hold:
 *   - one or more frames, concatenated; skippable frames (magic 0x184D2A50 .. 0x184D2A5F) are skipped;
 *   - raw, RLE and compressed blocks; raw, RLE, Huffman-compressed and treeless literals, 1 or 4 streams; every
 *     sequence table mode (predefined, RLE, FSE-compressed, repeat); offsets back to the start of the frame.
 * Statuses:
 *   - a frame whose header carries a (non-zero) Dictionary_ID: nvcompErrorNotSupported for that chunk;
 *   - every other problem (truncation, a malformed table or stream, an offset in front of the frame, an output
 *     capacity too small, a Frame_Content_Size that disagrees with the content): nvcompErrorCannotDecompress;
 *   - the content checksum is consumed but not verified.
 * device_actual_uncompressed_bytes and device_statuses may be NULL, as for every other codec here.
 *
 * Temp buffer (required): a 64-byte ticket counter, then one literal slot per wave of the launch, where a wave
 * regenerates one block's literals:
 *   temp_bytes = 64 + min(num_chunks, 3072) * slot,  slot = round_up_16(min(128 KiB, max_uncompressed_chunk_bytes))
 * (GetTempSizeEx also caps slot at max_total_uncompressed_bytes). The launch keeps at most 3072 waves resident, so the
 * buffer scales with the card, not with the batch.
 */
#ifndef NVCOMP_ZSTD_H
#define NVCOMP_ZSTD_H

#include "shared_types.h"
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* reference call site: benchmarks/benchmark_zstd_chunked.cu:54 validates chunk sizes against it */
static const size_t nvcompZstdCompressionMaxAllowedChunkSize = 1 << 24;

static const size_t nvcompZstdRequiredAlignment = 1;

nvcompStatus_t nvcompBatchedZstdDecompressGetTempSize(
    size_t num_chunks,
    size_t max_uncompressed_chunk_bytes,
    size_t* temp_bytes);

nvcompStatus_t nvcompBatchedZstdDecompressGetTempSizeEx(
    size_t num_chunks,
    size_t max_uncompressed_chunk_bytes,
    size_t* temp_bytes,
    size_t max_total_uncompressed_bytes);

nvcompStatus_t nvcompBatchedZstdDecompressAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    const size_t* device_uncompressed_bytes,
    size_t* device_actual_uncompressed_bytes,
    size_t batch_size,
    void* const device_temp_ptr,
    size_t temp_bytes,
    void* const* device_uncompressed_ptrs,
    nvcompStatus_t* device_statuses,
    hipStream_t stream);

/* The sum of the chunk's frames' Frame_Content_Size fields; 0 when a frame has no such field or the chunk is not
 * Zstd. */
nvcompStatus_t nvcompBatchedZstdGetDecompressSizeAsync(
    const void* const* device_compressed_ptrs,
    const size_t* device_compressed_bytes,
    size_t* device_uncompressed_bytes,
    size_t batch_size,
    hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NVCOMP_ZSTD_H */
