/*
 * nvcomp/native/bitcomp.h -- the native Bitcomp API: plans over ONE buffer of any length, lossless and lossy
 * (error-bounded) compression of numerical data, partial decompression. MI355X build.
 *
 * nvCOMP 2.5.0 "added independent bitcomp.h header to access full feature set of bitcomp compressor" (the reference's
 * CHANGELOG.md); this is that header's plan / handle family. The batched nvcompBatchedBitcomp* calls of nvcomp/bitcomp.h
 * take chunks the caller has cut and are lossless only; this API takes the whole buffer, cuts it itself, and can
 * quantise fp16 / fp32 / fp64 data by a caller-given `delta` in front of the integer coder.
 *
 *   bitcompHandle_t plan;
 *   bitcompCreatePlan(&plan, n_bytes, BITCOMP_FP32_DATA, BITCOMP_LOSSY_FP_TO_SIGNED, BITCOMP_DEFAULT_ALGO);
 *   bitcompSetStream(plan, stream);
 *   hipMalloc(&comp, bitcompMaxBuflen(n_bytes));
 *   bitcompCompressLossy_fp32(plan, device_input, comp, 1e-3f);     // enqueues kernels, returns at once
 *   bitcompUncompress(plan, comp, device_output);                   // |x - x'| <= delta / 2
 *   hipStreamSynchronize(stream); bitcompGetCompressedSize(comp, &bytes);
 *   bitcompDestroyPlan(plan);
 *
 * Plans.
 *   - A plan is for exactly n_bytes of one data type: any size_t, 0 and sizes above 4 GiB included; n_bytes must be a
 *     multiple of the element size (BITCOMP_INVALID_INPUT_LENGTH). Signed and unsigned integer types of one width are
 *     coded alike; the floating-point types on a LOSSLESS plan are coded as the unsigned integer of their width.
 *   - The LOSSY modes need a floating-point data type (BITCOMP_INVALID_PARAMETER otherwise).
 *   - bitcompCreatePlan allocates device memory on the current device (scratch for the compressor: about n_bytes) and
 *     queries it; it is the only call that does. With valid arguments and no usable device it returns
 *     BITCOMP_CUDA_API_ERROR; argument errors are reported without touching a device.
 *   - bitcompCreatePlanFromCompressedData reads type, mode, algorithm and size from a compressed buffer (device or host
 *     pointer). Such a plan is for decompression: it owns no scratch, and the compress calls return
 *     BITCOMP_INVALID_PARAMETER on it.
 *   - All state is in the handle; the library keeps none of its own. A handle is used by one thread at a time.
 *
 * Compress / uncompress / partial uncompress ONLY ENQUEUE KERNELS on the plan's stream (bitcompSetStream; default: the
 * null stream): no allocation, no host synchronisation, legal inside a stream capture. Device pointers must be aligned
 * to the element size and the compressed buffer to 8 bytes (BITCOMP_INVALID_ALIGNMENT). bitcompCompressLossless on a
 * lossy plan, bitcompCompressLossy_* on a lossless plan or on a plan of another width, and a delta that is not a finite
 * number above 0 are BITCOMP_INVALID_PARAMETER.
 *
 * Lossy compression, exactly. For element x and the call's delta:
 *     q  = rint(x / delta)       round-half-to-even; the division is correctly rounded; computed in fp32 for fp16 and
 *                                fp32 data (fp16 is widened exactly first), in fp64 for fp64 data
 *     q -> the integer of the element's width, signed (BITCOMP_LOSSY_FP_TO_SIGNED) or unsigned (..._TO_UNSIGNED),
 *          SATURATING at the type's limits; NaN becomes 0; negative values under FP_TO_UNSIGNED become 0
 *     x' = (fp)q * delta         on decompression, same precision, narrowed round-to-nearest-even for fp16
 *   so |x - x'| <= delta / 2 (plus one rounding of the product) for every finite x with x / delta inside the integer
 *   range; saturated and non-finite inputs are not restored. The integers go through the lossless coder:
 *   BITCOMP_DEFAULT_ALGO = differences between neighbours + bit packing (algorithm_type 0 of nvcomp/bitcomp.h),
 *   BITCOMP_SPARSE_ALGO = bit packing only (algorithm_type 1). delta is stored in the compressed buffer.
 *
 * The compressed buffer is self-describing and never larger than bitcompMaxBuflen(n_bytes):
 *     32-byte header (magic, type, mode, algorithm, n_bytes, compressed size, delta)
 *     | u64 offset[segments + 1] | the segments' streams, contiguous        (a segment = 64 KiB of input)
 *   The segments decode independently: bitcompUncompress runs them in parallel and bitcompPartialUncompress touches
 *   only those that overlap [start_bytes, start_bytes + length_bytes) (both multiples of the element size, else
 *   BITCOMP_INVALID_INPUT_LENGTH; a range that ends behind n_bytes is BITCOMP_INVALID_PARAMETER); `output` receives
 *   the range's first element at offset 0.
 *
 * Malformed compressed data never makes the library write outside [output, output + n_bytes) nor read outside
 * [input, input + min(the compressed size its header states, bitcompMaxBuflen(n_bytes))). The calls have no compressed-
 * size argument, so a buffer shorter than its own header states cannot be detected. The kernels have no status channel:
 * a buffer whose header does not match the plan is not decoded at all, a corrupt segment decodes to unspecified bytes
 * inside its part of the output. The queries below return BITCOMP_INVALID_COMPRESSED_DATA for a bad header.
 *
 * Queries. `data` may be a device or a host pointer (bitcompGetCompressedSizeAsync: device). The synchronous ones copy
 * the 32-byte header with a blocking copy: the caller has synchronised the stream that wrote the buffer.
 *
 * Differences from the published header: `cudaStream_t` is `hipStream_t`; bitcompCompressLossy_fp16 takes the data as
 * `const void*` (IEEE binary16 bit patterns) and delta as `float`, so that this header compiles as C without a half type
 * (C++ callers compiled by hipcc get an overload on `__half`); the batched-plan family (bitcompCreateBatchedPlan,
 * bitcompBatch*) and the bitcompHost* CPU functions are not provided.
 */
#ifndef NVCOMP_NATIVE_BITCOMP_H
#define NVCOMP_NATIVE_BITCOMP_H

#include <stddef.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bitcompContext* bitcompHandle_t;

typedef enum bitcompResult_t
{
  BITCOMP_SUCCESS = 0,
  BITCOMP_INVALID_PARAMETER = -1,
  BITCOMP_INVALID_COMPRESSED_DATA = -2,
  BITCOMP_INVALID_ALIGNMENT = -3,
  BITCOMP_INVALID_INPUT_LENGTH = -4,
  BITCOMP_CUDA_KERNEL_LAUNCH_ERROR = -5,
  BITCOMP_CUDA_API_ERROR = -6,
  BITCOMP_UNKNOWN_ERROR = -7
} bitcompResult_t;

typedef enum bitcompDataType_t
{
  BITCOMP_UNSIGNED_8BIT = 0,
  BITCOMP_SIGNED_8BIT,
  BITCOMP_UNSIGNED_16BIT,
  BITCOMP_SIGNED_16BIT,
  BITCOMP_UNSIGNED_32BIT,
  BITCOMP_SIGNED_32BIT,
  BITCOMP_UNSIGNED_64BIT,
  BITCOMP_SIGNED_64BIT,
  BITCOMP_FP16_DATA,
  BITCOMP_FP32_DATA,
  BITCOMP_FP64_DATA
} bitcompDataType_t;

typedef enum bitcompMode_t
{
  BITCOMP_LOSSLESS = 0,
  BITCOMP_LOSSY_FP_TO_SIGNED = 1,
  BITCOMP_LOSSY_FP_TO_UNSIGNED = 2
} bitcompMode_t;

typedef enum bitcompAlgorithm_t
{
  BITCOMP_DEFAULT_ALGO = 0,
  BITCOMP_SPARSE_ALGO = 1
} bitcompAlgorithm_t;

/* ---- plans ---- */
bitcompResult_t bitcompCreatePlan(
    bitcompHandle_t* handle, size_t n_bytes, bitcompDataType_t data_type, bitcompMode_t mode, bitcompAlgorithm_t algo);
bitcompResult_t bitcompCreatePlanFromCompressedData(bitcompHandle_t* handle, const void* data);
bitcompResult_t bitcompDestroyPlan(bitcompHandle_t handle);
bitcompResult_t bitcompSetStream(bitcompHandle_t handle, hipStream_t stream);

/* ---- the hot calls: kernels on the plan's stream, nothing else ---- */
bitcompResult_t bitcompCompressLossless(const bitcompHandle_t handle, const void* input, void* output);
bitcompResult_t bitcompCompressLossy_fp16(const bitcompHandle_t handle, const void* input, void* output, float delta);
bitcompResult_t bitcompCompressLossy_fp32(const bitcompHandle_t handle, const float* input, void* output, float delta);
bitcompResult_t bitcompCompressLossy_fp64(const bitcompHandle_t handle, const double* input, void* output, double delta);
bitcompResult_t bitcompUncompress(const bitcompHandle_t handle, const void* input, void* output);
bitcompResult_t bitcompPartialUncompress(
    const bitcompHandle_t handle, const void* input, void* output, size_t start_bytes, size_t length_bytes);

/* ---- sizes and descriptions ---- */
/* the largest compressed size of n_bytes of any type and mode; host only, needs no device */
size_t bitcompMaxBuflen(size_t n_bytes);
bitcompResult_t bitcompGetCompressedSize(const void* data, size_t* bytes);
/* *device_bytes is written on `stream` (0 for a bad header) */
bitcompResult_t bitcompGetCompressedSizeAsync(const void* data, size_t* device_bytes, hipStream_t stream);
bitcompResult_t bitcompGetUncompressedSize(const void* data, size_t* bytes);
bitcompResult_t bitcompGetUncompressedSizeFromHandle(const bitcompHandle_t handle, size_t* bytes);
/* reads at most max_bytes of `data` (fewer than the 32 bytes of the header: BITCOMP_INVALID_COMPRESSED_DATA) */
bitcompResult_t bitcompGetCompressedInfo(
    const void* data, size_t max_bytes, bitcompDataType_t* data_type, bitcompMode_t* mode, bitcompAlgorithm_t* algo);

#ifdef __cplusplus
}

#if defined(__HIPCC__)
#include <hip/hip_fp16.h>
/* the published signature, for C++ callers that hold `__half` data */
inline bitcompResult_t bitcompCompressLossy_fp16(const bitcompHandle_t handle, const __half* input, void* output, __half delta)
{
  return bitcompCompressLossy_fp16(handle, (const void*)input, output, __half2float(delta));
}
#endif
#endif

#endif /* NVCOMP_NATIVE_BITCOMP_H */
