/* tests/hlif/hlif_driver.cpp -- TEST CODE ONLY: extern "C" entry points over the high-level C++ interface, so that
 * tests/test_hlif_managers.py can drive the managers through ctypes. Public headers only, the typed managers (their
 * constructors and default arguments are compiled and run), no codec or container logic. Every entry point catches:
 * 0 = success, 1 = std::invalid_argument, 2 = std::runtime_error, 3 = anything else; hlif_last_error() has the text. */
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "nvcomp.hpp"
#include "nvcomp/ans.hpp"
#include "nvcomp/bitcomp.hpp"
#include "nvcomp/cascaded.hpp"
#include "nvcomp/deflate.hpp"
#include "nvcomp/lz4.hpp"
#include "nvcomp/nvcompManagerFactory.hpp"
#include "nvcomp/snappy.hpp"

using namespace nvcomp;

namespace {

thread_local std::string g_error;

template <typename F>
int guarded(F&& f)
{
  try {
    f();
    g_error.clear();
    return 0;
  } catch (const std::invalid_argument& e) {
    g_error = e.what();
    return 1;
  } catch (const std::runtime_error& e) {
    g_error = e.what();
    return 2;
  } catch (const std::exception& e) {
    g_error = e.what();
    return 3;
  } catch (...) {
    g_error = "unknown exception";
    return 3;
  }
}

struct Manager
{
  std::shared_ptr<nvcompManagerBase> m;
};

/* defaults: every default argument of the typed constructor */
template <typename M, typename O>
std::shared_ptr<nvcompManagerBase> open_typed(
    size_t chunk, const void* opts, size_t opts_bytes, hipStream_t stream, int device, ChecksumPolicy policy, bool defaults)
{
  if (defaults) {
    return std::make_shared<M>(chunk);
  }
  if (opts_bytes != sizeof(O)) {
    throw std::invalid_argument("driver: options bytes do not have the size of the format's options");
  }
  O o;
  memcpy(&o, opts, sizeof(o));
  return std::make_shared<M>(chunk, o, stream, device, policy);
}

} // namespace

extern "C" {

const char* hlif_last_error()
{
  return g_error.c_str();
}

/* format: BatchedManager::Format. defaults != 0: M(chunk) alone (default options, stream 0, device 0, no checksums). */
int hlif_open(int format, size_t chunk, const void* opts, size_t opts_bytes, int policy, void* stream, int defaults, void** out)
{
  return guarded([&] {
    hipStream_t s = (hipStream_t)stream;
    const ChecksumPolicy p = (ChecksumPolicy)policy;
    const bool d = defaults != 0;
    std::shared_ptr<nvcompManagerBase> m;
    switch (format) {
    case BatchedManager::kLZ4: m = open_typed<LZ4Manager, nvcompBatchedLZ4Opts_t>(chunk, opts, opts_bytes, s, 0, p, d); break;
    case BatchedManager::kSnappy: m = open_typed<SnappyManager, nvcompBatchedSnappyOpts_t>(chunk, opts, opts_bytes, s, 0, p, d); break;
    case BatchedManager::kCascaded: m = open_typed<CascadedManager, nvcompBatchedCascadedOpts_t>(chunk, opts, opts_bytes, s, 0, p, d); break;
    case BatchedManager::kBitcomp: m = open_typed<BitcompManager, nvcompBatchedBitcompFormatOpts>(chunk, opts, opts_bytes, s, 0, p, d); break;
    case BatchedManager::kANS: m = open_typed<ANSManager, nvcompBatchedANSOpts_t>(chunk, opts, opts_bytes, s, 0, p, d); break;
    case BatchedManager::kDeflate: m = open_typed<DeflateManager, nvcompBatchedDeflateOpts_t>(chunk, opts, opts_bytes, s, 0, p, d); break;
    default: throw std::invalid_argument("driver: unknown format");
    }
    *out = new Manager{m};
  });
}

int hlif_open_from_buffer(const void* comp_buffer, int policy, void* stream, void** out)
{
  return guarded([&] {
    *out = new Manager{create_manager((const uint8_t*)comp_buffer, (hipStream_t)stream, 0, (ChecksumPolicy)policy)};
  });
}

int hlif_close(void* manager)
{
  return guarded([&] { delete (Manager*)manager; });
}

int hlif_configure_compression(void* manager, size_t bytes, void** config, size_t* max_compressed, size_t* num_chunks)
{
  return guarded([&] {
    auto* c = new CompressionConfig(((Manager*)manager)->m->configure_compression(bytes));
    *config = c;
    *max_compressed = c->max_compressed_buffer_size;
    *num_chunks = c->num_chunks;
  });
}

int hlif_compress(void* manager, const void* decomp, void* comp, void* config)
{
  return guarded([&] { ((Manager*)manager)->m->compress((const uint8_t*)decomp, (uint8_t*)comp, *(CompressionConfig*)config); });
}

int hlif_configure_decompression(void* manager, const void* comp, void** config, size_t* decomp_bytes, size_t* num_chunks,
                                 size_t* chunk_size)
{
  return guarded([&] {
    auto* d = new DecompressionConfig(((Manager*)manager)->m->configure_decompression((const uint8_t*)comp));
    *config = d;
    *decomp_bytes = d->decomp_data_size;
    *num_chunks = d->num_chunks;
    *chunk_size = d->chunk_size;
  });
}

int hlif_configure_decompression_from_config(void* manager, void* comp_config, void** config, size_t* decomp_bytes,
                                             size_t* num_chunks, size_t* chunk_size)
{
  return guarded([&] {
    auto* d = new DecompressionConfig(((Manager*)manager)->m->configure_decompression(*(CompressionConfig*)comp_config));
    *config = d;
    *decomp_bytes = d->decomp_data_size;
    *num_chunks = d->num_chunks;
    *chunk_size = d->chunk_size;
  });
}

int hlif_decompress(void* manager, void* decomp, const void* comp, void* config)
{
  return guarded([&] { ((Manager*)manager)->m->decompress((uint8_t*)decomp, (const uint8_t*)comp, *(DecompressionConfig*)config); });
}

int hlif_compression_status(void* config, int* status)
{
  return guarded([&] { *status = (int)*((CompressionConfig*)config)->get_status(); });
}

int hlif_decompression_status(void* config, int* status)
{
  return guarded([&] { *status = (int)*((DecompressionConfig*)config)->get_status(); });
}

/* the address of the status word: lifetimes tests look at which words are handed out */
const void* hlif_compression_status_address(void* config)
{
  return ((CompressionConfig*)config)->get_status();
}

const void* hlif_decompression_status_address(void* config)
{
  return ((DecompressionConfig*)config)->get_status();
}

int hlif_compressed_output_size(void* manager, void* comp, size_t* bytes)
{
  return guarded([&] { *bytes = ((Manager*)manager)->m->get_compressed_output_size((uint8_t*)comp); });
}

int hlif_close_compression_config(void* config)
{
  return guarded([&] { delete (CompressionConfig*)config; });
}

int hlif_close_decompression_config(void* config)
{
  return guarded([&] { delete (DecompressionConfig*)config; });
}

} /* extern "C" */
