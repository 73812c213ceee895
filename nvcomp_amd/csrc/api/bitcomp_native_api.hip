/*
 * api/bitcomp_native_api.hip -- C ABI of the native Bitcomp API (include/nvcomp/native/bitcomp.h) and the kernels it
 * launches. A plan covers one buffer of any length; the buffer is cut into segments of 64 KiB, one wavefront codes a
 * segment with the batched codec's loops (bitcomp/bitcomp.hip.h), and the lossy modes quantise inside those loops
 * (bitcomp/quantize.hip.h). Plan creation allocates and asks the device; the compress / uncompress calls only enqueue.
 *
 * Compressed buffer (every field little-endian, the buffer 8-byte aligned):
 *
 *      0  u32  magic 'B' 'C' 'N' 0x01
 *      4  u8   data type | u8 mode | u8 algorithm | u8 log2(segment bytes) = 16
 *      8  u64  n_bytes
 *     16  u64  compressed bytes (the whole buffer, this header included)
 *     24  f64  delta (0 for lossless)
 *     32  u64  offset[segments + 1]   offset[i] = where segment i starts behind the table, offset[segments] = their sum
 *     32 + 8 (segments + 1)           the segments' chunk streams (bitcomp/bitcomp.hip.h: `chunk`), contiguous
 *
 * Compress is three steps on the plan's stream, none of which waits for the host:
 *   1. native_compress_kernel: a resident grid, one wave per segment, into worst-case slots of the plan's scratch;
 *      sizes[segment] = bytes produced;
 *   2. nvcompAmdBatchedPackAsync (api/pack_api.hip): prefix sum of the sizes straight into the buffer's offset table,
 *      then one wave per segment copies slot -> its place;
 *   3. native_header_kernel: the 32-byte header, whose compressed size needs the sum.
 * Uncompress and partial uncompress are one launch: a resident grid, one wave per segment that overlaps the range, every
 * offset taken from the buffer bounded before it is used.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <string.h>

#include <new>
#include <vector>

#include "nvcomp/amd_ext.h"
#include "nvcomp/native/bitcomp.h"

#include "common/log.h"
#include "common/api_batch.hip.h"

#include "bitcomp/quantize.hip.h"

namespace {

constexpr uint32_t kSegLog2 = 16;
constexpr size_t kSeg = (size_t)1 << kSegLog2; /* 64 KiB: the batched path's chunk, where its kernels were tuned */
constexpr uint32_t kMagic = 0x014e4342u;       /* 'B' 'C' 'N' 1 */
constexpr size_t kHeaderBytes = 32;
constexpr unsigned kDefaultGroups = 256 * 8;   /* when the runtime cannot tell what stays resident */

__host__ __device__ inline size_t segments_of(size_t n_bytes)
{
  return n_bytes / kSeg + (n_bytes % kSeg != 0);
}

/* a segment's slot in the scratch = the largest chunk stream of 64 KiB of any element size, 16-byte aligned */
__host__ __device__ inline size_t slot_bytes()
{
  size_t m = 0;
  for (uint32_t s = 1; s <= 8; s *= 2) {
    const size_t b = bitcomp::max_compressed_bytes(kSeg, s);
    m = b > m ? b : m;
  }
  return (m + 15) & ~(size_t)15;
}

__host__ __device__ inline size_t payload_start(size_t segments)
{
  return kHeaderBytes + 8 * (segments + 1);
}

__host__ __device__ inline size_t max_buflen(size_t n_bytes)
{
  const size_t segments = segments_of(n_bytes);
  return payload_start(segments) + segments * slot_bytes();
}

__host__ __device__ inline uint32_t kind_word(uint32_t dtype, uint32_t mode, uint32_t algo)
{
  return dtype | (mode << 8) | (algo << 16) | (kSegLog2 << 24);
}

__host__ __device__ inline uint32_t elem_bytes(uint32_t dtype)
{
  return dtype <= BITCOMP_SIGNED_8BIT ? 1u : dtype <= BITCOMP_SIGNED_16BIT ? 2u : dtype <= BITCOMP_SIGNED_32BIT ? 4u
       : dtype <= BITCOMP_SIGNED_64BIT ? 8u : dtype == BITCOMP_FP16_DATA ? 2u : dtype == BITCOMP_FP32_DATA ? 4u : 8u;
}

struct StreamHeader
{
  uint32_t magic;
  uint32_t kind;
  uint64_t n_bytes;
  uint64_t comp_bytes;
  double delta;
};
static_assert(sizeof(StreamHeader) == kHeaderBytes, "header layout");

/* Is this a header a compressor here can have written? Everything later code divides by or sizes from is checked. */
__host__ __device__ inline bool header_ok(const StreamHeader& h)
{
  const uint32_t dtype = h.kind & 0xffu, mode = (h.kind >> 8) & 0xffu, algo = (h.kind >> 16) & 0xffu;
  if (h.magic != kMagic || (h.kind >> 24) != kSegLog2 || dtype > BITCOMP_FP64_DATA || mode > BITCOMP_LOSSY_FP_TO_UNSIGNED
      || algo > BITCOMP_SPARSE_ALGO) {
    return false;
  }
  if (h.n_bytes % elem_bytes(dtype) != 0 || h.n_bytes > ((uint64_t)1 << 62)) {
    return false;
  }
  if (mode == BITCOMP_LOSSLESS ? h.delta != 0.0 : !(dtype >= BITCOMP_FP16_DATA && h.delta > 0.0 && h.delta < INFINITY)) {
    return false;
  }
  return h.comp_bytes >= payload_start(segments_of(h.n_bytes)) && h.comp_bytes <= max_buflen(h.n_bytes);
}

__device__ __forceinline__ uint64_t load_u64(const uint8_t* p)
{
  return bitcomp::load_elem<uint64_t>(p);
}

__device__ __forceinline__ void set_delta(bitcomp::AsIs&, double) {}
template <bool SIGNED>
__device__ __forceinline__ void set_delta(bitcomp::Quantize<SIGNED>& q, double delta)
{
  q.delta = delta;
}

/* ---- kernels ------------------------------------------------------------------- */

/* Workgroups a CU the register allocation aims at. The batched compressor's figures (api/bitcomp_api.hip: 8, and 6 for
 * 8-byte elements) leave these kernels -- a loop over segments around the same body, 64-bit addressing, and for the lossy
 * ones a division per element inlined 32 times -- 6 to 43 spilled registers; a step down each and none spills. */
template <class T, class Q>
constexpr unsigned compress_groups_per_cu()
{
  return sizeof(T) == 8 ? (Q::kIdentity ? 5 : 4) : (sizeof(T) == 2 && !Q::kIdentity ? 5 : 8);
}

template <class T, bool DELTA, class Q>
__global__ void __launch_bounds__(64 * kWavesPerBlock, (compress_groups_per_cu<T, Q>())) native_compress_kernel(
    const uint8_t* __restrict__ in, size_t n_bytes, size_t segments, uint8_t* __restrict__ slots, size_t slot,
    size_t* __restrict__ sizes, double delta)
{
  Q q;
  set_delta(q, delta);
  const size_t stride = (size_t)gridDim.x * kWavesPerBlock;
  for (size_t s = (size_t)blockIdx.x * kWavesPerBlock + wave::uniform(threadIdx.x >> 6); s < segments; s += stride) {
    const size_t at = s * kSeg;
    const uint32_t n = (uint32_t)(n_bytes - at < kSeg ? n_bytes - at : kSeg);
    const uint32_t produced = bitcomp::encode_chunk<T, DELTA, Q>(in + at, n, slots + s * slot, q);
    if (wave::lane_id() == 0) {
      sizes[s] = produced;
    }
  }
}

__global__ void __launch_bounds__(64) native_header_kernel(uint8_t* out, StreamHeader h, size_t segments)
{
  if (threadIdx.x == 0) {
    h.comp_bytes = payload_start(segments) + load_u64(out + kHeaderBytes + 8 * segments);
    bitcomp::store_elem<StreamHeader>(out, h);
  }
}

/* What a plan knows of the buffer it decodes; the header must say the same, or nothing is decoded. */
struct Expect
{
  size_t n_bytes;
  uint32_t kind;
};

/* Segments [first, first + count) of the buffer; only the bytes [start, start + length) of the data are stored, at
 * out + (their position - start). The whole buffer: first = 0, count = all, start = 0, length = n_bytes. */
template <class T, bool DELTA, class Q>
__global__ void __launch_bounds__(64 * kWavesPerBlock) native_decompress_kernel(
    const uint8_t* __restrict__ comp, uint8_t* __restrict__ out, Expect want, size_t first, size_t count, size_t start,
    size_t length)
{
  StreamHeader h;
  h.magic = wave::uniform(bitcomp::load_u32(comp));
  h.kind = wave::uniform(bitcomp::load_u32(comp + 4));
  h.n_bytes = wave::uniform64(load_u64(comp + 8));
  h.comp_bytes = wave::uniform64(load_u64(comp + 16));
  h.delta = bitcomp::bits_as<double>(wave::uniform64(load_u64(comp + 24)));
  if (!header_ok(h) || h.kind != want.kind || h.n_bytes != want.n_bytes) {
    return;
  }
  const size_t segments = segments_of(want.n_bytes);
  const size_t base = payload_start(segments);
  const size_t limit = h.comp_bytes - base; /* header_ok: base <= comp_bytes <= max_buflen(n_bytes) */
  const size_t slot = slot_bytes();
  bitcomp::Range<Q> x;
  set_delta(x.q, h.delta);
  const size_t stride = (size_t)gridDim.x * kWavesPerBlock;
  for (size_t k = (size_t)blockIdx.x * kWavesPerBlock + wave::uniform(threadIdx.x >> 6); k < count; k += stride) {
    const size_t s = first + k;
    const uint64_t lo = wave::uniform64(load_u64(comp + kHeaderBytes + 8 * s));
    const uint64_t hi = wave::uniform64(load_u64(comp + kHeaderBytes + 8 * s + 8));
    if (lo > hi || hi > limit || hi - lo > slot) {
      continue; /* a segment that claims bytes outside the buffer is not read */
    }
    const size_t at = s * kSeg;
    const uint32_t n = (uint32_t)(want.n_bytes - at < kSeg ? want.n_bytes - at : kSeg);
    const size_t from = start > at ? start - at : 0;
    const size_t to = start + length < at + n ? (start + length > at ? start + length - at : 0) : n;
    x.lo = (uint32_t)(from / sizeof(T));
    x.hi = (uint32_t)(to / sizeof(T));
    LZ_STAT("bitcomp_native_segments_decoded", 1);
    /* (element i of the segment goes to out + at - start + i sizeof(T): behind `out` for every element that is kept) */
    uint8_t* dst = (uint8_t*)((uintptr_t)out + (uintptr_t)at - (uintptr_t)start);
    uint32_t err = bitcomp::kErrNone;
    bitcomp::decode_body<T, DELTA, true, bitcomp::Range<Q>>(comp + base + lo, (uint32_t)(hi - lo), dst, n, err, x);
  }
}

__global__ void __launch_bounds__(64) native_size_kernel(const uint8_t* comp, size_t* bytes)
{
  if (threadIdx.x == 0) {
    const StreamHeader h = bitcomp::load_elem<StreamHeader>(comp);
    *bytes = header_ok(h) ? (size_t)h.comp_bytes : 0;
  }
}

/* ---- which kernels a plan launches ---------------------------------------------- */

struct Ops
{
  void (*compress)(unsigned grid, hipStream_t, const uint8_t*, size_t, size_t, uint8_t*, size_t, size_t*, double);
  void (*decompress)(unsigned grid, hipStream_t, const uint8_t*, uint8_t*, Expect, size_t, size_t, size_t, size_t);
  unsigned (*resident_compress)();
  unsigned (*resident_decompress)();
};

template <class T, bool DELTA, class Q>
void launch_compress(unsigned grid, hipStream_t stream, const uint8_t* in, size_t n_bytes, size_t segments, uint8_t* slots,
                     size_t slot, size_t* sizes, double delta)
{
  hipLaunchKernelGGL((native_compress_kernel<T, DELTA, Q>), dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, in, n_bytes,
                     segments, slots, slot, sizes, delta);
}

template <class T, bool DELTA, class Q>
void launch_decompress(unsigned grid, hipStream_t stream, const uint8_t* comp, uint8_t* out, Expect want, size_t first,
                       size_t count, size_t start, size_t length)
{
  hipLaunchKernelGGL((native_decompress_kernel<T, DELTA, Q>), dim3(grid), dim3(64 * kWavesPerBlock), 0, stream, comp, out,
                     want, first, count, start, length);
}

template <class T, bool DELTA, class Q>
unsigned resident_compress()
{
  return lzl::resident_workgroups(native_compress_kernel<T, DELTA, Q>, 64 * kWavesPerBlock, 0);
}

template <class T, bool DELTA, class Q>
unsigned resident_decompress()
{
  return lzl::resident_workgroups(native_decompress_kernel<T, DELTA, Q>, 64 * kWavesPerBlock, 0);
}

template <class T, class Q>
Ops ops_of(bool delta)
{
  if (delta) {
    return Ops{launch_compress<T, true, Q>, launch_decompress<T, true, Q>, resident_compress<T, true, Q>,
               resident_decompress<T, true, Q>};
  }
  return Ops{launch_compress<T, false, Q>, launch_decompress<T, false, Q>, resident_compress<T, false, Q>,
             resident_decompress<T, false, Q>};
}

template <class Q>
Ops ops_fp(uint32_t elem, bool delta)
{
  return elem == 2 ? ops_of<uint16_t, Q>(delta) : elem == 4 ? ops_of<uint32_t, Q>(delta) : ops_of<uint64_t, Q>(delta);
}

Ops ops_for(uint32_t elem, int mode, bool delta)
{
  if (mode == BITCOMP_LOSSY_FP_TO_SIGNED) {
    return ops_fp<bitcomp::Quantize<true>>(elem, delta);
  }
  if (mode == BITCOMP_LOSSY_FP_TO_UNSIGNED) {
    return ops_fp<bitcomp::Quantize<false>>(elem, delta);
  }
  return elem == 1 ? ops_of<uint8_t, bitcomp::AsIs>(delta) : ops_fp<bitcomp::AsIs>(elem, delta);
}

/* launch_status() (common/api_launch.h) in this API's result type */
bitcompResult_t native_launch_status()
{
  return hipGetLastError() == hipSuccess ? BITCOMP_SUCCESS : BITCOMP_CUDA_KERNEL_LAUNCH_ERROR;
}

bool aligned(const void* p, size_t a)
{
  return ((uintptr_t)p & (a - 1)) == 0;
}

/* The first `n` bytes of a compressed buffer, wherever it lives. A pointer the runtime does not know is host memory. */
bool fetch(const void* data, void* to, size_t n)
{
#if defined(__HIPCC__)
  hipPointerAttribute_t attr;
  const bool on_device = hipPointerGetAttributes(&attr, data) == hipSuccess
                         && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged);
  (void)hipGetLastError();
  if (on_device) {
    return hipMemcpy(to, data, n, hipMemcpyDeviceToHost) == hipSuccess;
  }
#endif
  /* (the tests' host build of this file runs the kernels on the CPU: every pointer is host memory there) */
  memcpy(to, data, n);
  return true;
}

bitcompResult_t read_header(const void* data, size_t max_bytes, StreamHeader* h)
{
  if (data == nullptr) {
    return BITCOMP_INVALID_PARAMETER;
  }
  if (max_bytes < kHeaderBytes) {
    return BITCOMP_INVALID_COMPRESSED_DATA;
  }
  if (!fetch(data, h, kHeaderBytes)) {
    return BITCOMP_CUDA_API_ERROR;
  }
  return header_ok(*h) ? BITCOMP_SUCCESS : BITCOMP_INVALID_COMPRESSED_DATA;
}

} // namespace

struct bitcompContext
{
  size_t n_bytes = 0;
  size_t segments = 0;
  uint32_t dtype = 0, mode = 0, algo = 0, elem = 1;
  hipStream_t stream = nullptr;
  Ops ops{};
  unsigned grid_compress = 1, grid_decompress = 1;
  /* compressor scratch, one allocation: slots | sizes | slot pointers. NULL: a plan for decompression, or of 0 bytes */
  uint8_t* scratch = nullptr;
  uint8_t* slots = nullptr;
  size_t* sizes = nullptr;
  void** slot_ptrs = nullptr;
};

namespace {

unsigned grid_of(unsigned resident, size_t segments)
{
  const size_t groups = (segments + kWavesPerBlock - 1) / kWavesPerBlock;
  const size_t fit = resident != 0 ? resident : kDefaultGroups;
  const size_t g = groups < fit ? groups : fit;
  return (unsigned)(g != 0 ? g : 1);
}

bitcompResult_t make_plan(bitcompHandle_t* handle, size_t n_bytes, int dtype, int mode, int algo, bool for_compression)
{
  if (handle == nullptr || dtype < BITCOMP_UNSIGNED_8BIT || dtype > BITCOMP_FP64_DATA || mode < BITCOMP_LOSSLESS
      || mode > BITCOMP_LOSSY_FP_TO_UNSIGNED || algo < BITCOMP_DEFAULT_ALGO || algo > BITCOMP_SPARSE_ALGO
      || (mode != BITCOMP_LOSSLESS && dtype < BITCOMP_FP16_DATA)) {
    return BITCOMP_INVALID_PARAMETER;
  }
  const uint32_t elem = elem_bytes((uint32_t)dtype);
  if (n_bytes % elem != 0) {
    return BITCOMP_INVALID_INPUT_LENGTH;
  }
  bitcompContext* c = new (std::nothrow) bitcompContext;
  if (c == nullptr) {
    return BITCOMP_UNKNOWN_ERROR;
  }
  c->n_bytes = n_bytes;
  c->segments = segments_of(n_bytes);
  c->dtype = (uint32_t)dtype;
  c->mode = (uint32_t)mode;
  c->algo = (uint32_t)algo;
  c->elem = elem;
  c->ops = ops_for(elem, mode, algo == BITCOMP_DEFAULT_ALGO);
  if (c->segments != 0) {
    clear_stale_error();
    if (for_compression) {
      const size_t slot = slot_bytes();
      const size_t slots_bytes = c->segments * slot;
      if (hipMalloc((void**)&c->scratch, slots_bytes + 16 * c->segments) != hipSuccess) {
        (void)hipGetLastError();
        delete c;
        return BITCOMP_CUDA_API_ERROR;
      }
      c->slots = c->scratch;
      c->sizes = (size_t*)(c->scratch + slots_bytes);
      c->slot_ptrs = (void**)(c->scratch + slots_bytes + 8 * c->segments);
      std::vector<void*> ptrs(c->segments);
      for (size_t s = 0; s < c->segments; ++s) {
        ptrs[s] = c->slots + s * slot;
      }
      if (hipMemcpy(c->slot_ptrs, ptrs.data(), 8 * c->segments, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(c->scratch);
        delete c;
        return BITCOMP_CUDA_API_ERROR;
      }
      c->grid_compress = grid_of(c->ops.resident_compress(), c->segments);
    }
    c->grid_decompress = grid_of(c->ops.resident_decompress(), c->segments);
  }
  *handle = c;
  return BITCOMP_SUCCESS;
}

bitcompResult_t compress(bitcompHandle_t h, const void* input, void* output, bool lossy, uint32_t dtype, double delta)
{
  if (h == nullptr || output == nullptr || (input == nullptr && h->n_bytes != 0)) {
    return BITCOMP_INVALID_PARAMETER;
  }
  if (lossy ? (h->mode == BITCOMP_LOSSLESS || h->dtype != dtype || !(delta > 0.0 && delta < INFINITY))
            : h->mode != BITCOMP_LOSSLESS) {
    return BITCOMP_INVALID_PARAMETER;
  }
  if (h->segments != 0 && h->scratch == nullptr) {
    return BITCOMP_INVALID_PARAMETER; /* a plan made from compressed data decompresses */
  }
  if (!aligned(input, h->elem) || !aligned(output, 8)) {
    return BITCOMP_INVALID_ALIGNMENT;
  }
  nvlog::call(3, "bitcompCompress(n_bytes=%zu, type=%u, mode=%u, algo=%u, delta=%g, stream=%p)", h->n_bytes, h->dtype, h->mode,
              h->algo, delta, (void*)h->stream);
  clear_stale_error();
  uint8_t* out = (uint8_t*)output;
  const size_t slot = slot_bytes();
  if (h->segments != 0) {
    h->ops.compress(h->grid_compress, h->stream, (const uint8_t*)input, h->n_bytes, h->segments, h->slots, slot, h->sizes,
                    delta);
  }
  if (nvcompAmdBatchedPackAsync(h->slot_ptrs, h->sizes, h->segments, out + payload_start(h->segments), h->segments * slot,
                                (size_t*)(out + kHeaderBytes), h->stream) != nvcompSuccess) {
    return BITCOMP_CUDA_KERNEL_LAUNCH_ERROR;
  }
  StreamHeader head;
  head.magic = kMagic;
  head.kind = kind_word(h->dtype, h->mode, h->algo);
  head.n_bytes = h->n_bytes;
  head.comp_bytes = 0;
  head.delta = lossy ? delta : 0.0;
  hipLaunchKernelGGL(native_header_kernel, dim3(1), dim3(64), 0, h->stream, out, head, h->segments);
  return native_launch_status();
}

} // namespace

extern "C" {

size_t bitcompMaxBuflen(size_t n_bytes)
{
  return max_buflen(n_bytes);
}

bitcompResult_t bitcompCreatePlan(
    bitcompHandle_t* handle, size_t n_bytes, bitcompDataType_t data_type, bitcompMode_t mode, bitcompAlgorithm_t algo)
{
  nvlog::call(3, "bitcompCreatePlan(n_bytes=%zu, type=%d, mode=%d, algo=%d)", n_bytes, (int)data_type, (int)mode, (int)algo);
  return make_plan(handle, n_bytes, (int)data_type, (int)mode, (int)algo, true);
}

bitcompResult_t bitcompCreatePlanFromCompressedData(bitcompHandle_t* handle, const void* data)
{
  if (handle == nullptr) {
    return BITCOMP_INVALID_PARAMETER;
  }
  StreamHeader h;
  const bitcompResult_t rc = read_header(data, kHeaderBytes, &h);
  if (rc != BITCOMP_SUCCESS) {
    return rc;
  }
  return make_plan(handle, (size_t)h.n_bytes, (int)(h.kind & 0xffu), (int)((h.kind >> 8) & 0xffu), (int)((h.kind >> 16) & 0xffu),
                   false);
}

bitcompResult_t bitcompDestroyPlan(bitcompHandle_t handle)
{
  if (handle == nullptr) {
    return BITCOMP_INVALID_PARAMETER;
  }
  bitcompResult_t rc = BITCOMP_SUCCESS;
  if (handle->scratch != nullptr && hipFree(handle->scratch) != hipSuccess) {
    (void)hipGetLastError();
    rc = BITCOMP_CUDA_API_ERROR;
  }
  delete handle;
  return rc;
}

bitcompResult_t bitcompSetStream(bitcompHandle_t handle, hipStream_t stream)
{
  if (handle == nullptr) {
    return BITCOMP_INVALID_PARAMETER;
  }
  handle->stream = stream;
  return BITCOMP_SUCCESS;
}

bitcompResult_t bitcompCompressLossless(const bitcompHandle_t handle, const void* input, void* output)
{
  return compress(handle, input, output, false, 0, 0.0);
}

bitcompResult_t bitcompCompressLossy_fp16(const bitcompHandle_t handle, const void* input, void* output, float delta)
{
  return compress(handle, input, output, true, BITCOMP_FP16_DATA, (double)delta);
}

bitcompResult_t bitcompCompressLossy_fp32(const bitcompHandle_t handle, const float* input, void* output, float delta)
{
  return compress(handle, input, output, true, BITCOMP_FP32_DATA, (double)delta);
}

bitcompResult_t bitcompCompressLossy_fp64(const bitcompHandle_t handle, const double* input, void* output, double delta)
{
  return compress(handle, input, output, true, BITCOMP_FP64_DATA, delta);
}

bitcompResult_t bitcompPartialUncompress(
    const bitcompHandle_t handle, const void* input, void* output, size_t start_bytes, size_t length_bytes)
{
  if (handle == nullptr || input == nullptr || (output == nullptr && length_bytes != 0)) {
    return BITCOMP_INVALID_PARAMETER;
  }
  if (start_bytes % handle->elem != 0 || length_bytes % handle->elem != 0) {
    return BITCOMP_INVALID_INPUT_LENGTH;
  }
  if (start_bytes > handle->n_bytes || length_bytes > handle->n_bytes - start_bytes) {
    return BITCOMP_INVALID_PARAMETER;
  }
  if (!aligned(input, 8) || !aligned(output, handle->elem)) {
    return BITCOMP_INVALID_ALIGNMENT;
  }
  nvlog::call(3, "bitcompPartialUncompress(n_bytes=%zu, start=%zu, length=%zu, stream=%p)", handle->n_bytes, start_bytes,
              length_bytes, (void*)handle->stream);
  if (length_bytes == 0) {
    return BITCOMP_SUCCESS;
  }
  const size_t first = start_bytes / kSeg;
  const size_t count = (start_bytes + length_bytes - 1) / kSeg - first + 1;
  clear_stale_error();
  Expect want;
  want.n_bytes = handle->n_bytes;
  want.kind = kind_word(handle->dtype, handle->mode, handle->algo);
  const unsigned groups = (unsigned)((count + kWavesPerBlock - 1) / kWavesPerBlock < handle->grid_decompress
                                         ? (count + kWavesPerBlock - 1) / kWavesPerBlock
                                         : handle->grid_decompress);
  handle->ops.decompress(groups, handle->stream, (const uint8_t*)input, (uint8_t*)output, want, first, count, start_bytes,
                         length_bytes);
  return native_launch_status();
}

bitcompResult_t bitcompUncompress(const bitcompHandle_t handle, const void* input, void* output)
{
  if (handle == nullptr) {
    return BITCOMP_INVALID_PARAMETER;
  }
  return bitcompPartialUncompress(handle, input, output, 0, handle->n_bytes);
}

bitcompResult_t bitcompGetCompressedSize(const void* data, size_t* bytes)
{
  StreamHeader h;
  if (bytes == nullptr) {
    return BITCOMP_INVALID_PARAMETER;
  }
  const bitcompResult_t rc = read_header(data, kHeaderBytes, &h);
  if (rc == BITCOMP_SUCCESS) {
    *bytes = (size_t)h.comp_bytes;
  }
  return rc;
}

bitcompResult_t bitcompGetCompressedSizeAsync(const void* data, size_t* device_bytes, hipStream_t stream)
{
  if (data == nullptr || device_bytes == nullptr) {
    return BITCOMP_INVALID_PARAMETER;
  }
  if (!aligned(data, 8)) {
    return BITCOMP_INVALID_ALIGNMENT;
  }
  clear_stale_error();
  hipLaunchKernelGGL(native_size_kernel, dim3(1), dim3(64), 0, stream, (const uint8_t*)data, device_bytes);
  return native_launch_status();
}

bitcompResult_t bitcompGetUncompressedSize(const void* data, size_t* bytes)
{
  StreamHeader h;
  if (bytes == nullptr) {
    return BITCOMP_INVALID_PARAMETER;
  }
  const bitcompResult_t rc = read_header(data, kHeaderBytes, &h);
  if (rc == BITCOMP_SUCCESS) {
    *bytes = (size_t)h.n_bytes;
  }
  return rc;
}

bitcompResult_t bitcompGetUncompressedSizeFromHandle(const bitcompHandle_t handle, size_t* bytes)
{
  if (handle == nullptr || bytes == nullptr) {
    return BITCOMP_INVALID_PARAMETER;
  }
  *bytes = handle->n_bytes;
  return BITCOMP_SUCCESS;
}

bitcompResult_t bitcompGetCompressedInfo(
    const void* data, size_t max_bytes, bitcompDataType_t* data_type, bitcompMode_t* mode, bitcompAlgorithm_t* algo)
{
  StreamHeader h;
  if (data_type == nullptr || mode == nullptr || algo == nullptr) {
    return BITCOMP_INVALID_PARAMETER;
  }
  const bitcompResult_t rc = read_header(data, max_bytes, &h);
  if (rc == BITCOMP_SUCCESS) {
    *data_type = (bitcompDataType_t)(h.kind & 0xffu);
    *mode = (bitcompMode_t)((h.kind >> 8) & 0xffu);
    *algo = (bitcompAlgorithm_t)((h.kind >> 16) & 0xffu);
  }
  return rc;
}

} // extern "C"
