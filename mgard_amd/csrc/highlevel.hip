// High-level path of libmgard_hip.so: whole-array compress / decompress (SURVEY.md section 8b
// "high-level", 8f ranks 2-4) on top of the low-level C ABI of capi.hip:
//   domain decomposition + double-buffered subdomain pipeline
//     (reference DomainDecomposer.hpp:72-470, 649-845; GPUPipelines.hpp:69-207, 330-520),
//   Huffman [+ Zstd] lossless stage (huffman.hpp; Lossless.hpp:70-118, Zstd.hpp:69-128),
//   self-describing container (format.hpp; Metadata.cpp:249-462).
// Host code is C++; everything exported is extern "C" (include/mgard_hip_compress.h).
#include "../../include/mgard_hip_compress.h"
#include "../../include/mgard_hip_level_layers.h"

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cmath>
#include <memory>
#include <mutex>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <stdexcept>
#include <string>
#include <condition_variable>
#include <thread>
#include <vector>

#include "format.hpp"
#include "huffman.hpp"
#include "huffman_record.hpp"
#include "env.hpp"
#include "hierarchy.hpp"
#include "compare_plan.hpp"
#include "domain_plan.hpp"
#include "size_plan.hpp"
#include "target_plan.hpp"
#include "mask_plan.hpp"
#include "pwrel_plan.hpp"
#include "roi_plan.hpp"

extern "C" void mgh_set_last_error_(const char *msg);  // capi.hip
// (capi.hip: mgh_mask_fill / mgh_mask_restore with the value given as the bits of the data type)
extern "C" int mgh_mask_fill_bits_(int D, int dtype, const uint64_t *shape, const void *data, const uint64_t *words,
                                   uint64_t c_bits, void *out, void *stream);
extern "C" int mgh_mask_restore_bits_(int D, int dtype, const uint64_t *shape, const uint64_t *words, uint64_t value_bits,
                                      void *data, void *stream);
// (capi.hip: the reduction of mgh_compare on two device arrays given by element strides, asynchronous)
extern "C" size_t mgh_compare_scratch_bytes_(void);
extern "C" void mgh_compare_release_(void);
extern "C" int mgh_compare_device_(int D, int dtype, const uint64_t *shape, const void *d_a, const uint64_t *stride_a,
                                   const void *d_b, const uint64_t *stride_b, void *d_scratch, void *stream);
// (capi.hip: the packed mask of a level grid, a coarsened grid or a window gathered out of the array's)
extern "C" int mgh_mask_sample_(int D, const uint64_t *shape, const uint64_t *words, const uint64_t *out_shape,
                                const uint32_t *const *d_idx, uint64_t *out_words, uint64_t *d_count, void *stream);
// (capi.hip: ... with a packed mask seen through element strides and the bit of the first element)
extern "C" int mgh_compare_masked_device_(int D, int dtype, const uint64_t *shape, const void *d_a, const uint64_t *stride_a,
                                          const void *d_b, const uint64_t *stride_b, const uint64_t *d_words,
                                          const uint64_t *stride_m, uint64_t bit0, void *d_scratch, void *stream);

namespace {
constexpr int kOutlierOverflow = -1000;  // internal: more outliers than the buffers hold
constexpr int kLadderMaxTols = 64;       // mgh_compress_ladder: tolerances per call

// Kernel attributes such as the dynamic-LDS limit belong to the function on the current device and
// are set once per device ordinal: `if (hl_attr_pending(once)) { set ...; hl_attr_done(once); }`.
// The bit is set AFTER the attributes exist, so a second host thread on the same device can never
// launch before them (two threads setting them twice is harmless).
inline uint64_t hl_device_bit() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return (uint64_t)1 << (dev & 63);
}
inline bool hl_attr_pending(const std::atomic<uint64_t> &done) {
  return !(done.load(std::memory_order_acquire) & hl_device_bit());
}
inline void hl_attr_done(std::atomic<uint64_t> &done) {
  done.fetch_or(hl_device_bit(), std::memory_order_release);
}
// compute units of the current device (cached per device ordinal)
inline int hl_num_cu() {
  static std::atomic<int> cache[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  int v = cache[dev & 63].load(std::memory_order_relaxed);
  if (v <= 0) {
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
    cache[dev & 63].store(v, std::memory_order_relaxed);
  }
  return v;
}


using namespace mgh;

// MGH_DEBUG_SYNC=1: name the stages on stderr and synchronise (developer aid, see capi.hip)
inline void hl_debug(const char *what) {
  static const bool on = env_get("MGH_DEBUG_SYNC", 0) != 0;
  static const bool timing = env_get("MGH_HL_TIMING", 0) != 0;  // + microseconds since the last mark
  if (on || timing) {
    (void)hipDeviceSynchronize();
    static auto last = std::chrono::steady_clock::now();
    const auto now = std::chrono::steady_clock::now();
    if (timing)
      std::fprintf(stderr, "[mgh-hl] %8.1f us  %s\n",
                   std::chrono::duration<double, std::micro>(now - last).count(), what);
    else
      std::fprintf(stderr, "[mgh-hl] %s\n", what);
    std::fflush(stderr);
    last = std::chrono::steady_clock::now();
  }
}

int hl_fail(int code, const std::string &msg) {
  mgh_set_last_error_(msg.c_str());
  return code;
}

#define HL_HIP(expr)                                                                       \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return hl_fail(_e == hipErrorOutOfMemory ? MGH_ERR_OUT_OF_MEMORY : MGH_ERR_DEVICE,   \
                     std::string(#expr) + ": " + hipGetErrorString(_e));                   \
  } while (0)
#define HL_TRY(expr)                       \
  do {                                     \
    int _rc = (expr);                      \
    if (_rc != MGH_SUCCESS) return _rc;    \
  } while (0)

// The body of an extern "C" entry: no exception leaves the library, it becomes the entry's status.
template <typename Body> int hl_guarded(Body &&body) {
  try {
    return body();
  } catch (const std::exception &e) {
    return hl_fail(MGH_ERR_DEVICE, e.what());
  }
}

// the dynamic-LDS limit of some kernels, once per device (hl_attr_pending)
template <typename... K> int hl_lds_limit(std::atomic<uint64_t> &once, int bytes, K... kernels) {
  if (!hl_attr_pending(once)) return MGH_SUCCESS;
  for (const void *k : {reinterpret_cast<const void *>(kernels)...})
    HL_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  hl_attr_done(once);
  return MGH_SUCCESS;
}

// MemoryManager::IsDevicePointer
bool is_device_pointer(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice;
}

// device memory OF DEVICE `dev`: the zero-copy paths (encoder writing into the caller's record,
// decoders reading the code units in place) let KERNELS touch the caller's buffer, which works
// only on the device the kernels run on; memory of another GPU goes through hipMemcpyAsync
bool is_device_pointer_on(const void *p, int dev) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeDevice && a.device == dev;
}

bool is_registered_host(const void *p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// grow-only device buffer
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  int ensure(size_t bytes) {
    if (bytes <= cap) return MGH_SUCCESS;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    HL_HIP(hipMalloc(&p, bytes));
    cap = bytes;
    return MGH_SUCCESS;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// grow-only pinned host buffer: the small host<->device transfers of the lossless stage (histogram,
// code table, record head, counts) go through it -- out of pageable memory every one of them is a
// staged, host-synchronous copy of 15-25 us (rocprofv3 timeline of mgh_compress: ten of them in a row)
struct PinBuf {
  void *p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return MGH_SUCCESS;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    HL_HIP(hipHostMalloc(&p, bytes, hipHostMallocDefault));
    cap = bytes;
    return MGH_SUCCESS;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// ---- Zstd through the system library (libzstd.so.1), resolved at first use -----------------
struct ZstdApi {
  void *lib = nullptr;
  size_t (*compressBound)(size_t) = nullptr;
  size_t (*compress)(void *, size_t, const void *, size_t, int) = nullptr;
  size_t (*decompress)(void *, size_t, const void *, size_t) = nullptr;
  unsigned (*isError)(size_t) = nullptr;
  bool tried = false;
  bool load() {
    if (tried) return lib != nullptr;
    tried = true;
    for (const char *name : {"libzstd.so.1", "libzstd.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) return false;
    compressBound = (size_t(*)(size_t))dlsym(lib, "ZSTD_compressBound");
    compress = (size_t(*)(void *, size_t, const void *, size_t, int))dlsym(lib, "ZSTD_compress");
    decompress = (size_t(*)(void *, size_t, const void *, size_t))dlsym(lib, "ZSTD_decompress");
    isError = (unsigned (*)(size_t))dlsym(lib, "ZSTD_isError");
    if (!compressBound || !compress || !decompress || !isError) {
      dlclose(lib);
      lib = nullptr;
    }
    return lib != nullptr;
  }
};
ZstdApi g_zstd;

} // namespace

// ---- lossless context ----------------------------------------------------------------------
struct mgh_lossless_ctx {
  int dev = 0;
  DevBuf freq, code, bits, entry, total, units, tables, oidx, oval, state, dtable, sync;
  bool use_sync = false;   // the record of the last compress call carries synchronisation points
  uint64_t prepared_n = 0, prepared_dict = 0, prepared_chunk = 0;  // lossless_prepare() ran for a record of this size
  size_t n_chunks = 0;
  bool overflow = false;  // the code stream did not fit into cap_units: treat as incompressible
  huff::Codebook codebook;
  std::vector<uint8_t> host;   // serialized payload (when assembled on the host)
  std::vector<uint8_t> host2;  // zstd scratch
  // the record of the last compress call in pieces: everything before the code units sits in
  // `head`, the units and the outlier lists are still on the device
  std::vector<uint8_t> head;   // (decompression: host copy of the leading part of a record)
  // compression: [8 bytes: the record's size prefix, filled by the caller][head of the record:
  // lay.ddata bytes][histogram][code table][counts] in ONE pinned allocation
  PinBuf pin;
  PinBuf dpin;                         // decompression: pinned copy of the decode table (source of its upload)
  PinBuf tagpin;                       // decompression: word a kernel clears when a device-resident record's sync tag is wrong
  bool tag_pending = false;            // ... to be looked at once the stream has been synchronised (lossless_tag_check)
  uint8_t *chead = nullptr;            // = pin.p + 8
  unsigned long long *pcounts = nullptr;  // [0..2] encoder state, [3] outlier count read back, [4] n_outliers to write
  PayloadLayout lay;
  uint64_t n_units = 0, n_outliers = 0;
  uint64_t outliers_needed = 0;  // set when lossless_compress returns kOutlierOverflow
  const uint64_t *d_oidx = nullptr;
  const int64_t *d_oval = nullptr;
  bool on_host = false;  // Huffman_Zstd: the whole record is in `host`
  // the encoder wrote the code units straight into the caller's record (lossless_compress:
  // `direct`): record_write() does not move them again
  bool units_in_place = false;
  std::vector<uint32_t> h_dtable;  // decompression: two-level decode table (source of an asynchronous upload)
  // A reader that comes back to ONE record (mgh_progressive). 1: the next lossless_decompress() parses
  // the head, inflates a Zstd frame, uploads the decode tables, the whole chunk table and the outlier
  // lists, and keeps them (-> 2); 2: all that is in place -- a call moves only the code units and
  // synchronisation entries of the chunks it decodes.
  int keep = 0;
  size_t record_size() const { return overflow ? ~(size_t)0 : (on_host ? host.size() : lay.total); }
};

namespace {

using ChunkFn = std::function<int(size_t, size_t, hipEvent_t)>;
int copy_any(void *dst, const void *src, size_t bytes, hipStream_t st, const ChunkFn *on_chunk = nullptr);  // (below)

// Host copy of the first bytes of the device-resident stream a decompression call is reading:
// header, record size and the leading part of the first record come out of ONE device-to-host
// copy instead of four synchronous ones (tens of microseconds each). Valid only inside
// mgh_decompress (HostPrefix guard).
struct HostPrefixState {
  const uint8_t *base = nullptr;
  std::vector<uint8_t> bytes;
};
inline HostPrefixState &host_prefix() {
  static thread_local HostPrefixState s;
  return s;
}
int aux_read(void *dst, const void *src, size_t bytes);  // (below, with the cache)
struct HostPrefix {
  HostPrefix(const void *dev, size_t size) {
    HostPrefixState &s = host_prefix();
    s.base = nullptr;
    const size_t want = std::min<size_t>(size, 320 * 1024);
    s.bytes.resize(want);
    // (through the cache's pinned buffer and its own stream once a cache exists: a hipMemcpy into
    // pageable memory is staged by the runtime, ~20 us more per call)
    if (aux_read(s.bytes.data(), dev, want) == MGH_SUCCESS)
      s.base = (const uint8_t *)dev;
  }
  ~HostPrefix() { host_prefix().base = nullptr; }
};
hipStream_t cache_copy_stream(int dev);                   // (below: the calling thread's copy stream on that device, or nullptr)
// device -> host copy that is served from the prefix where it can be
inline int dev_to_host(void *dst, const void *src, size_t bytes) {
  const HostPrefixState &s = host_prefix();
  const uint8_t *p = (const uint8_t *)src;
  if (s.base && p >= s.base && bytes <= s.bytes.size() && (size_t)(p - s.base) <= s.bytes.size() - bytes) {
    std::memcpy(dst, s.bytes.data() + (p - s.base), bytes);
    return MGH_SUCCESS;
  }
  return aux_read(dst, src, bytes);
}

// The small pieces of a device-resident record -- its head out of the context's pinned buffer (which
// the device reads directly), the outlier count, the two outlier lists, the synchronisation points
// -- in ONE launch instead of five asynchronous copies of ~7 us of host time each, which all sit
// between the encoder's result and the caller's return. Any byte alignment on either side.
struct RecordPieces {
  const uint8_t *src[5];
  uint8_t *dst[5];
  size_t bytes[5];
  int n;
  // decompression of a device-resident record: the 8 bytes that must be the tag of the
  // synchronisation-point section (any alignment); *tag_ok (pinned host memory) = 0 if they are not
  const uint8_t *tag_src;
  unsigned long long tag_want;
  unsigned *tag_ok;
  void add(const void *from, void *to, size_t nbytes) {
    if (!nbytes) return;
    src[n] = (const uint8_t *)from;
    dst[n] = (uint8_t *)to;
    bytes[n] = nbytes;
    n++;
  }
  size_t total() const {
    size_t t = 0;
    for (int i = 0; i < n; i++) t += bytes[i];
    return t;
  }
};
__global__ void __launch_bounds__(256) k_record_pieces(RecordPieces P) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  if (P.tag_src && t == 0) {
    unsigned long long tag;
    __builtin_memcpy(&tag, P.tag_src, 8);
    if (tag != P.tag_want) *P.tag_ok = 0;
  }
  for (int i = 0; i < P.n; i++) {
    const uint8_t *sp = P.src[i];
    uint8_t *dp = P.dst[i];
    const size_t words = P.bytes[i] / 8;
    for (size_t w = t; w < words; w += stride) {
      unsigned long long v;
      __builtin_memcpy(&v, sp + 8 * w, 8);
      __builtin_memcpy(dp + 8 * w, &v, 8);
    }
    for (size_t b = words * 8 + t; b < P.bytes[i]; b += stride) dp[b] = sp[b];
  }
}

int launch_record_pieces(const RecordPieces &P, hipStream_t st) {
  const unsigned blocks = (unsigned)std::min<size_t>(std::max<size_t>(P.total() / (256 * 64), 1), 512);
  k_record_pieces<<<blocks, 256, 0, st>>>(P);
  HL_HIP(hipGetLastError());
  return MGH_SUCCESS;
}

// Copy the record of the last lossless_compress() to dst (host or device memory, record_size()
// bytes). Asynchronous on st where the memory kinds allow it.
int record_write(mgh_lossless_ctx *c, void *dst, hipStream_t st, const uint64_t *size_prefix = nullptr) {
  // size_prefix: the 8 bytes in front of dst get *size_prefix -- for a device-resident record they
  // travel with the head of the record in ONE copy out of the pinned buffer
  char *d = (char *)dst;
  if (c->on_host) {
    if (size_prefix) {
      // (through the context's pinned buffer: the caller's variable may be gone before the queued copy runs)
      std::memcpy(c->chead - 8, size_prefix, 8);
      HL_HIP(hipMemcpyAsync(d - 8, c->chead - 8, 8, hipMemcpyDefault, st));
    }
    HL_HIP(hipMemcpyAsync(d, c->host.data(), c->host.size(), hipMemcpyDefault, st));
    return MGH_SUCCESS;
  }
  const PayloadLayout &L = c->lay;
  void *dev_head = nullptr;
  if (is_device_pointer_on(dst, c->dev) &&
      hipHostGetDevicePointer(&dev_head, c->chead - 8, 0) == hipSuccess && dev_head) {
    if (size_prefix) std::memcpy(c->chead - 8, size_prefix, 8);
    if (c->n_units && !c->units_in_place)
      HL_TRY(copy_any(d + L.ddata, c->units.p, c->n_units * 8, st));
    RecordPieces P{};
    const uint8_t *dh = (const uint8_t *)dev_head;
    if (size_prefix) P.add(dh, d - 8, 8 + L.ddata);
    else P.add(dh + 8, d, L.ddata);
    // (the count out of the pinned buffer too: &c->pcounts[4] lies behind the head in the same allocation)
    P.add(dh + ((const uint8_t *)&c->pcounts[4] - (c->chead - 8)), d + L.outlier_count, 8);
    P.add(c->d_oidx, d + L.outlier_idx, c->n_outliers * 8);
    P.add(c->d_oval, d + L.outliers, c->n_outliers * 8);
    if (c->use_sync) P.add(c->sync.p, d + L.sync_tag, PayloadLayout::sync_bytes(c->n_chunks));
    return launch_record_pieces(P, st);
  }
  (void)hipGetLastError();
  if (size_prefix) {
    std::memcpy(c->chead - 8, size_prefix, 8);
    HL_HIP(hipMemcpyAsync(d - 8, c->chead - 8, 8 + L.ddata, hipMemcpyDefault, st));
  } else {
    HL_HIP(hipMemcpyAsync(d, c->chead, L.ddata, hipMemcpyDefault, st));
  }
  if (c->n_units && !c->units_in_place)
    HL_TRY(copy_any(d + L.ddata, c->units.p, c->n_units * 8, st));
  // (the count travels from pinned memory that outlives the asynchronous copy)
  HL_HIP(hipMemcpyAsync(d + L.outlier_count, &c->pcounts[4], 8, hipMemcpyDefault, st));
  if (c->n_outliers) {
    HL_HIP(hipMemcpyAsync(d + L.outlier_idx, c->d_oidx, c->n_outliers * 8, hipMemcpyDefault, st));
    HL_HIP(hipMemcpyAsync(d + L.outliers, c->d_oval, c->n_outliers * 8, hipMemcpyDefault, st));
  }
  if (c->use_sync)  // (tag + entries as the encoder left them: one piece)
    HL_TRY(copy_any(d + L.sync_tag, c->sync.p, PayloadLayout::sync_bytes(c->n_chunks), st));
  return MGH_SUCCESS;
}

// ocount: number of outliers, or (d_ocount != nullptr) read from the device together with the
// results of the encoder (one host synchronisation less) and checked against ocap.
// cap_units: upper bound for the code stream the caller is interested in (0: worst case).
// The stage runs in two halves so that the subdomain pipeline can queue the first half of
// subdomain k+1 (behind its decomposition, on its own stream) before it waits for subdomain k:
//   lossless_begin():  histogram kernel + its copy to the host, queued on st, no synchronisation;
//   lossless_finish(): waits for the histogram, builds the code on the host, encodes, reads the
//                      counts back (second synchronisation) and lays out the head of the record.
// lossless_compress() = both, for the stand-alone entry point.
struct LosslessJob {
  const int64_t *d_q = nullptr;
  uint64_t n = 0, dict = 0, chunk = 0;
  int lossless = MGH_LOSSLESS_HUFFMAN, zstd_level = 3;
  const uint64_t *d_oidx = nullptr;
  const int64_t *d_oval = nullptr;
  uint64_t ocount = 0;
  const uint64_t *d_ocount = nullptr;
  uint64_t ocap = ~(uint64_t)0, cap_units = 0;
  bool sym16 = false;
  bool bins_filled = false;  // the quantizer counted the symbols into the context's bins (mgh_quantize_symbols)
};

// Zeroing of the stage's device state (histogram bins, the encoder's chunk states, optionally a
// counter of the caller) in ONE launch. Queued by the subdomain pipeline in FRONT of the
// subdomain's decomposition, where the device is waiting for the host's launches anyway; three
// memsets between quantizer and encoder were ~15 us of every record's critical path.
__global__ void __launch_bounds__(256) k_zero_words(unsigned long long *a, size_t na, unsigned long long *b,
                                                    size_t nb, unsigned long long *c1) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
  for (size_t i = t; i < na; i += stride) a[i] = 0;
  for (size_t i = t; i < nb; i += stride) b[i] = 0;
  if (c1 && t == 0) *c1 = 0;
}
int lossless_prepare(mgh_lossless_ctx *c, uint64_t n, uint64_t dict, uint64_t chunk, hipStream_t st,
                     unsigned long long *also_zero = nullptr) {
  c->prepared_n = 0;
  if (n == 0 || dict == 0 || dict > 16384 || chunk == 0 || chunk > (1u << 30)) return MGH_SUCCESS;  // (lossless_begin reports it)
  const size_t nchunk = (n - 1) / chunk + 1;
  HL_TRY(c->freq.ensure((dict * 4 + 7) / 8 * 8));
  HL_TRY(c->state.ensure((3 + nchunk) * 8));
  const size_t words = (dict * 4 + 7) / 8 + 3 + nchunk;
  k_zero_words<<<(unsigned)std::min<size_t>((words + 255) / 256, 256), 256, 0, st>>>(
      (unsigned long long *)c->freq.p, (dict * 4 + 7) / 8, (unsigned long long *)c->state.p, 3 + nchunk, also_zero);
  HL_HIP(hipGetLastError());
  c->prepared_n = n;
  c->prepared_dict = dict;
  c->prepared_chunk = chunk;
  return MGH_SUCCESS;
}

int lossless_begin(mgh_lossless_ctx *c, const LosslessJob &J, hipStream_t st) {
  const int64_t *d_q = J.d_q;
  const uint64_t n = J.n, dict = J.dict, chunk = J.chunk;
  const int lossless = J.lossless;
  const bool sym16 = J.sym16;
  // sym16: d_q points to uint16_t symbols (mgh_decompose_quantize_sym16) -- only with the
  // single-pass encoder (lossless_sym16_ok)
  if (lossless != MGH_LOSSLESS_HUFFMAN && lossless != MGH_LOSSLESS_HUFFMAN_ZSTD)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless: only Huffman and Huffman_Zstd are supported");
  if (n == 0 || dict == 0 || dict > 16384 || chunk == 0 || chunk > (1u << 30))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless: n, dict_size (<= 16384) or chunk_size");
  if (lossless == MGH_LOSSLESS_HUFFMAN_ZSTD && !g_zstd.load())
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless: libzstd.so.1 not found");
  const size_t nchunk = (n - 1) / chunk + 1;
  const bool prepared = c->prepared_n == n && c->prepared_dict == dict && c->prepared_chunk == chunk;
  c->prepared_n = 0;  // (good for one record)
  HL_TRY(c->freq.ensure((dict * 4 + 7) / 8 * 8));
  HL_TRY(c->code.ensure(dict * 8));
  HL_TRY(c->bits.ensure(nchunk * 8));
  HL_TRY(c->entry.ensure(nchunk * 8));
  HL_TRY(c->total.ensure(8));
  hl_debug("lossless_compress: begin");
  // the frequency counts are 32-bit (a subdomain of 2^32 symbols is 32 GB of int64: the domain
  // decomposer never produces one, but the stand-alone entry point could be handed one)
  if (n >= ((uint64_t)1 << 32))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless stage: more than 2^32 - 1 symbols in one record");
  // (bins_filled: lossless_prepare zeroed the bins in front of the quantizer that filled them)
  if (J.bins_filled && !prepared) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless: filled bins without lossless_prepare");
  if (!prepared) HL_HIP(hipMemsetAsync(c->freq.p, 0, dict * 4, st));
  const unsigned hblocks =
      (unsigned)std::min<size_t>((n + huff::kHistThreads - 1) / huff::kHistThreads, 2 * (size_t)hl_num_cu());
  if (J.bins_filled)
    hl_debug("lossless_compress: bins filled by the quantizer");
  else if (sym16)
    huff::k_histogram<uint16_t><<<hblocks, huff::kHistThreads, dict * 4, st>>>((const uint16_t *)d_q, n, (int)dict,
                                                                               (unsigned *)c->freq.p);
  else
    huff::k_histogram<int64_t><<<hblocks, huff::kHistThreads, dict * 4, st>>>(d_q, n, (int)dict,
                                                                              (unsigned *)c->freq.p);
  HL_HIP(hipGetLastError());
  // (the encoder's chunk states are cleared here, behind the histogram kernel, so that nothing but
  // the code table stands between the code construction on the host and the encoder's launch)
  HL_TRY(c->state.ensure((3 + nchunk) * 8));
  if (!prepared) HL_HIP(hipMemsetAsync(c->state.p, 0, (3 + nchunk) * 8, st));
  hl_debug("lossless_compress: histogram kernel done");
  // pinned staging of this call (see PinBuf)
  PayloadLayout &L = c->lay;
  L.compute(nchunk, dict, 0, 0);  // (the offsets before the code units do not depend on the counts)
  const size_t o_head = 8, o_freq = (o_head + L.ddata + 15) / 16 * 16, o_code = o_freq + dict * 4,
               o_cnt = o_code + dict * 8;
  HL_TRY(c->pin.ensure(o_cnt + 64));
  uint8_t *const pinp = (uint8_t *)c->pin.p;
  c->chead = pinp + o_head;
  c->pcounts = (unsigned long long *)(pinp + o_cnt);
  unsigned *freq = (unsigned *)(pinp + o_freq);
  HL_HIP(hipMemcpyAsync(freq, c->freq.p, dict * 4, hipMemcpyDeviceToHost, st));
  return MGH_SUCCESS;
}

int lossless_finish(mgh_lossless_ctx *c, const LosslessJob &J, hipStream_t st, uint8_t *direct = nullptr,
                    size_t direct_cap = 0) {
  const int64_t *d_q = J.d_q;
  const uint64_t n = J.n, dict = J.dict, chunk = J.chunk, ocap = J.ocap, cap_units = J.cap_units;
  const int lossless = J.lossless, zstd_level = J.zstd_level;
  const uint64_t *d_oidx = J.d_oidx, *d_ocount = J.d_ocount;
  const int64_t *d_oval = J.d_oval;
  uint64_t ocount = J.ocount;
  const bool sym16 = J.sym16;
  // direct (memory of this device, 8-byte aligned, direct_cap bytes): where record_write() will be
  // asked to put this record. The single-pass encoder then writes the code units there itself --
  // the offset of the units inside a record does not depend on the counts -- instead of into a
  // buffer of the context from which record_write() copies them (512^3 f32: 150 MB moved twice).
  c->units_in_place = false;
  const size_t nchunk = (n - 1) / chunk + 1;
  PayloadLayout &L = c->lay;
  const size_t o_head = 8, o_freq = (o_head + L.ddata + 15) / 16 * 16, o_code = o_freq + dict * 4;
  uint8_t *const pinp = (uint8_t *)c->pin.p;
  unsigned *freq = (unsigned *)(pinp + o_freq);
  HL_HIP(hipStreamSynchronize(st));
  hl_debug("lossless_compress: histogram on the host");
  huff::Codebook &cb = c->codebook;
  try {
    huff::build_codebook(freq, (int)dict, cb);
  } catch (const std::exception &e) {
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, e.what());
  }
  hl_debug("lossless_compress: histogram + codebook done");
  // code table for the kernels: 32-bit entries when every code fits 27 bits (it practically
  // always does: half the LDS of the encoder, two workgroups per CU), else 64-bit entries
  // (codes longer than 27 bits -- the rarest symbols of a large subdomain -- become escape entries
  // into a list of 64-bit entries behind the table)
  size_t nlong = 0;
  if (cb.max_len > huff::kShortCodeBits)
    for (uint64_t k = 0; k < dict; k++) nlong += (cb.code[k] >> huff::kMaxCodeBits) > (uint64_t)huff::kShortCodeBits;
  const size_t o_long = (dict * 4 + 7) / 8 * 8;  // offset of the escape list behind the 32-bit table
  const bool short_codes = o_long + nlong * 8 <= dict * 8;  // (table + list fit the buffers sized for 64-bit entries)
  if (!short_codes) nlong = 0;
  if (short_codes) {
    uint32_t *c32 = (uint32_t *)(pinp + o_code);
    uint64_t *lg = (uint64_t *)(pinp + o_code + o_long);
    size_t j = 0;
    for (uint64_t k = 0; k < dict; k++) {
      const uint64_t len = cb.code[k] >> huff::kMaxCodeBits;
      if (len <= (uint64_t)huff::kShortCodeBits) {
        c32[k] = (uint32_t)(len << huff::kShortCodeBits) |
                 (uint32_t)(cb.code[k] & (((uint64_t)1 << huff::kShortCodeBits) - 1));
      } else {
        c32[k] = (huff::kEscapeLen << huff::kShortCodeBits) | (uint32_t)j;
        lg[j++] = cb.code[k];
      }
    }
    HL_HIP(hipMemcpyAsync(c->code.p, c32, o_long + nlong * 8, hipMemcpyHostToDevice, st));
  } else {
    std::memcpy(pinp + o_code, cb.code.data(), dict * 8);
    HL_HIP(hipMemcpyAsync(c->code.p, pinp + o_code, dict * 8, hipMemcpyHostToDevice, st));
  }
  // Synchronisation points for the decoder behind the record (PayloadLayout): when, is
  // record_has_sync (size_plan.hpp, which prices a record from its histogram). MGH_HUFF_SYNC=0: never.
  c->n_chunks = nchunk;
  c->use_sync = record_has_sync(lossless, dict, chunk, cb.total_bits, n, env_get("MGH_HUFF_SYNC", 1));
  if (c->use_sync) HL_TRY(c->sync.ensure(PayloadLayout::sync_bytes(nchunk)));
  const size_t sync_bytes = c->use_sync ? PayloadLayout::sync_bytes(nchunk) : 0;
  // ---- serialize (Huffman.hpp:163-239): the small leading part on the host, the code units
  // and the outlier lists stay where they are until record_write() ----
  uint8_t *const out = c->chead;
  std::memset(out, 0, L.ddata);
  auto fetch_meta = [&]() -> int {  // bits_per_chunk[] and word_entry[] into the head
    HL_HIP(hipMemcpyAsync(out + L.huffmeta, c->bits.p, nchunk * 8, hipMemcpyDeviceToHost, st));
    HL_HIP(hipMemcpyAsync(out + L.huffmeta + nchunk * 8, c->entry.p, nchunk * 8,
                          hipMemcpyDeviceToHost, st));
    if (d_ocount) HL_HIP(hipMemcpyAsync(&c->pcounts[3], d_ocount, 8, hipMemcpyDeviceToHost, st));
    return MGH_SUCCESS;
  };
  unsigned long long units = 0;
  const size_t enc_lds = huff::encode_chain_lds(dict, short_codes ? 4 : 8, chunk);
  if (lossless_sym16_ok(dict, chunk) && chunk <= (1u << 24)) {
    // one pass: bit counts, unit offsets (decoupled look-back) and packing in the same kernel.
    // The stream is written into a buffer of cap_units; more than that means "not compressible".
    const unsigned long long worst = n + nchunk;  // a code is shorter than a unit
    unsigned long long cap = cap_units ? std::min<unsigned long long>(cap_units, worst) : worst;
    unsigned long long *units_dst = nullptr;
    // (the record may start at any byte: the encoder stores its units unaligned where it has to)
    if (direct && lossless == MGH_LOSSLESS_HUFFMAN && direct_cap > L.ddata + 64 + sync_bytes &&
        is_device_pointer_on(direct, c->dev)) {
      // (what does not fit behind the units -- outlier lists -- is the caller's capacity check)
      cap = std::min<unsigned long long>(cap, (direct_cap - L.ddata - 8 - sync_bytes) / 8);
      units_dst = (unsigned long long *)(direct + L.ddata);
      c->units_in_place = true;
    } else {
      HL_TRY(c->units.ensure(std::max<size_t>(cap, 1) * 8 + 8));
      units_dst = (unsigned long long *)c->units.p;
    }
    static std::atomic<uint64_t> once{0};
    HL_TRY(hl_lds_limit(once, 144 * 1024, huff::k_encode_chain<int64_t, uint64_t>, huff::k_encode_chain<uint16_t, uint64_t>,
                        huff::k_encode_chain<int64_t, uint32_t>, huff::k_encode_chain<uint16_t, uint32_t>));
    auto enc = [&](auto sym_tag, auto code_tag) {
      using SYM = decltype(sym_tag);
      using CODE = decltype(code_tag);
      huff::k_encode_chain<SYM, CODE><<<(unsigned)nchunk, huff::kEncThreads, enc_lds, st>>>(
          (const SYM *)d_q, n, (int)chunk, (int)dict, nchunk, (const CODE *)c->code.p,
          (unsigned long long *)c->state.p, (unsigned long long *)c->bits.p,
          (unsigned long long *)c->entry.p, units_dst, cap, (int)nlong,
          c->use_sync ? (unsigned *)c->sync.p + 2 : nullptr, PayloadLayout::kSyncTag);
    };
    if (sym16 && short_codes) enc(uint16_t(), uint32_t());
    else if (sym16) enc(uint16_t(), uint64_t());
    else if (short_codes) enc(int64_t(), uint32_t());
    else enc(int64_t(), uint64_t());
    HL_HIP(hipGetLastError());
    unsigned long long *st3 = c->pcounts;
    HL_HIP(hipMemcpyAsync(st3, c->state.p, 24, hipMemcpyDeviceToHost, st));
    HL_TRY(fetch_meta());
    HL_HIP(hipStreamSynchronize(st));
    if ((st3[2] & 2) && c->units_in_place) {
      // a chunk needed the path that packs with atomics, which an unaligned destination cannot
      // take (k_encode_chain): once more into the context's own (aligned) buffer
      c->units_in_place = false;
      cap = cap_units ? std::min<unsigned long long>(cap_units, worst) : worst;
      HL_TRY(c->units.ensure(std::max<size_t>(cap, 1) * 8 + 8));
      units_dst = (unsigned long long *)c->units.p;
      HL_HIP(hipMemsetAsync(c->state.p, 0, (3 + nchunk) * 8, st));
      if (sym16 && short_codes) enc(uint16_t(), uint32_t());
      else if (sym16) enc(uint16_t(), uint64_t());
      else if (short_codes) enc(int64_t(), uint32_t());
      else enc(int64_t(), uint64_t());
      HL_HIP(hipGetLastError());
      HL_HIP(hipMemcpyAsync(st3, c->state.p, 24, hipMemcpyDeviceToHost, st));
      HL_TRY(fetch_meta());
      HL_HIP(hipStreamSynchronize(st));
    }
    if (d_ocount) ocount = c->pcounts[3];
    units = st3[1];
    c->overflow = (st3[2] & 1) != 0;
  } else {
    if (sym16) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless: 16-bit symbols need the single-pass encoder");
    c->use_sync = false;
    if (short_codes)  // (these kernels read 64-bit entries)
      HL_HIP(hipMemcpyAsync(c->code.p, cb.code.data(), dict * 8, hipMemcpyHostToDevice, st));
    huff::k_chunk_bits<<<(unsigned)nchunk, 256, 0, st>>>(d_q, n, (int)chunk, (const uint64_t *)c->code.p,
                                                         (unsigned long long *)c->bits.p);
    huff::k_unit_offsets<<<1, 1024, 0, st>>>((const unsigned long long *)c->bits.p, nchunk,
                                             (unsigned long long *)c->entry.p,
                                             (unsigned long long *)c->total.p);
    HL_HIP(hipGetLastError());
    HL_HIP(hipMemcpyAsync(&c->pcounts[1], c->total.p, 8, hipMemcpyDeviceToHost, st));
    HL_TRY(fetch_meta());
    HL_HIP(hipStreamSynchronize(st));
    units = c->pcounts[1];
    if (d_ocount) ocount = c->pcounts[3];
    HL_TRY(c->units.ensure(std::max<size_t>(units, 1) * 8 + 8));
    HL_HIP(hipMemsetAsync(c->units.p, 0, units * 8, st));
    huff::k_encode<<<(unsigned)nchunk, 256, 0, st>>>(d_q, n, (int)chunk, (const uint64_t *)c->code.p,
                                                     (const unsigned long long *)c->entry.p,
                                                     (unsigned long long *)c->units.p);
    HL_HIP(hipGetLastError());
    c->overflow = false;
  }
  hl_debug("lossless_compress: encode launched");
  if (ocount > ocap) {
    // the caller re-runs the quantizer with buffers of this size (the reference re-allocates and
    // re-launches the same way: LinearQuantization.hpp:621-676)
    c->outliers_needed = ocount;
    return kOutlierOverflow;
  }
  c->on_host = false;
  if (c->overflow) return MGH_SUCCESS;  // record_size() says "larger than anything"
  L.compute(nchunk, dict, units, ocount, c->use_sync);
  auto put64 = [&](size_t off, uint64_t v) { std::memcpy(out + off, &v, 8); };
  auto put32 = [&](size_t off, int32_t v) { std::memcpy(out + off, &v, 4); };
  put64(L.primary_count, n);
  put32(8, (int32_t)dict);
  put32(12, (int32_t)chunk);
  put64(16, 2 * nchunk);
  put64(L.decodebook_size, 8 * (2 * 64) + 8 * dict);
  std::memcpy(out + L.decodebook, cb.first.data(), 8 * 64);
  std::memcpy(out + L.decodebook + 8 * 64, cb.entry.data(), 8 * 64);
  std::memcpy(out + L.decodebook + 8 * 128, cb.keys.data(), 8 * dict);
  put64(L.ddata_size, units);
  c->n_units = units;
  c->n_outliers = ocount;
  c->pcounts[4] = ocount;
  c->d_oidx = d_oidx;
  c->d_oval = d_oval;
  if (lossless == MGH_LOSSLESS_HUFFMAN_ZSTD) {
    // [size_t input_count][zstd frame] (Zstd.hpp:69-90): needs the whole record on the host
    std::vector<uint8_t> &full = c->host2;
    full.resize(L.total);
    HL_TRY(record_write(c, full.data(), st));
    HL_HIP(hipStreamSynchronize(st));
    const size_t bound = g_zstd.compressBound(full.size());
    c->host.resize(bound + 8);
    const size_t got = g_zstd.compress(c->host.data() + 8, bound, full.data(), full.size(), zstd_level);
    if (g_zstd.isError(got)) return hl_fail(MGH_ERR_DEVICE, "ZSTD_compress failed");
    const uint64_t in_size = full.size();
    std::memcpy(c->host.data(), &in_size, 8);
    c->host.resize(got + 8);
    c->on_host = true;
  }
  return MGH_SUCCESS;
}

int lossless_compress(mgh_lossless_ctx *c, const int64_t *d_q, uint64_t n, uint64_t dict,
                      uint64_t chunk, int lossless, int zstd_level, const uint64_t *d_oidx,
                      const int64_t *d_oval, uint64_t ocount, hipStream_t st,
                      const uint64_t *d_ocount = nullptr, uint64_t ocap = ~(uint64_t)0,
                      uint64_t cap_units = 0, bool sym16 = false, uint8_t *direct = nullptr,
                      size_t direct_cap = 0) {
  LosslessJob J;
  J.d_q = d_q; J.n = n; J.dict = dict; J.chunk = chunk; J.lossless = lossless; J.zstd_level = zstd_level;
  J.d_oidx = d_oidx; J.d_oval = d_oval; J.ocount = ocount; J.d_ocount = d_ocount; J.ocap = ocap;
  J.cap_units = cap_units; J.sym16 = sym16;
  HL_TRY(lossless_begin(c, J, st));
  return lossless_finish(c, J, st, direct, direct_cap);
}

// After a synchronisation of the stream lossless_decompress() ran on: was the tag of the
// synchronisation-point section of a device-resident record what it has to be?
int lossless_tag_check(mgh_lossless_ctx *c) {
  if (!c->tag_pending) return MGH_SUCCESS;
  c->tag_pending = false;
  if (*reinterpret_cast<volatile unsigned *>(c->tagpin.p) == 0)
    return hl_fail(MGH_ERR_FORMAT, "Huffman record: outlier lists");
  return MGH_SUCCESS;
}

// What the lossless stage of the last mgh_decompress* call of this thread did (mgh_last_decompress_stats).
inline mgh_decompress_stats &decompress_stats() {
  static thread_local mgh_decompress_stats s{};
  return s;
}

// The MGH_HUFF_* switches of the decoders (the two cross-check decoders are chosen once per process).
inline DecodeSwitches decode_switches() {
  static const bool serial = env_get("MGH_HUFF_SERIAL_DECODE", 0) != 0, par = env_get("MGH_HUFF_PAR_DECODE", 0) != 0;
  return DecodeSwitches{serial, par, env_get("MGH_HUFF_SYNC_DECODE", 1) != 0, env_get("MGH_HUFF_PAIR", 1), env_get("MGH_HUFF_TB", DecodeSwitches::kNotSet)};
}

// The Huffman record inside a Huffman_Zstd record, inflated into the context (a kept context holds it already).
int lossless_inflate(mgh_lossless_ctx *c, const uint8_t *payload, uint64_t size, bool on_dev) {
  if (c->keep == 2) return MGH_SUCCESS;
  if (!g_zstd.load()) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless: libzstd.so.1 not found");
  if (size < 8) return hl_fail(MGH_ERR_FORMAT, "zstd record truncated");
  const uint8_t *src = payload;
  if (on_dev) {
    c->host.resize(size);
    HL_HIP(hipMemcpy(c->host.data(), payload, size, hipMemcpyDeviceToHost));
    src = c->host.data();
  }
  uint64_t raw = 0;
  std::memcpy(&raw, src, 8);
  if (raw > ((uint64_t)1 << 40)) return hl_fail(MGH_ERR_FORMAT, "zstd record: implausible size");
  c->host2.resize(raw);
  const size_t got = g_zstd.decompress(c->host2.data(), raw, src + 8, size - 8);
  if (g_zstd.isError(got) || got != raw) return hl_fail(MGH_ERR_FORMAT, "ZSTD_decompress failed");
  return MGH_SUCCESS;
}

// Chunk table, decodebook and outlier lists of a parsed record into the context's device buffers
// (a kept context has them). here: the record lies in memory of the context's device.
int record_upload(mgh_lossless_ctx *c, const uint8_t *p, bool on_dev, bool here, const RecordPlan &R, hipStream_t st) {
  const PayloadLayout &L = R.L;
  const size_t nchunk = R.nchunk, ocount = R.ocount;
  const bool kept = c->keep == 2;
  mgh_decompress_stats &stats = decompress_stats();
  HL_TRY(c->bits.ensure(nchunk * 8));
  HL_TRY(c->entry.ensure(nchunk * 8));
  HL_TRY(c->tables.ensure(R.dbsize));
  HL_TRY(c->oidx.ensure(std::max<size_t>(ocount, 1) * 8));
  HL_TRY(c->oval.ensure(std::max<size_t>(ocount, 1) * 8));
  // (a record on this device: chunk table, decodebook and outlier lists in ONE launch -- five
  // queued copies of ~5 us each stood in front of every decoder launch)
  if (here) {
    RecordPieces P{};
    if (!kept) {
      P.add(p + L.huffmeta + R.tb0 * 8, c->bits.p, R.tb_cnt * 8);
      P.add(p + L.huffmeta + (nchunk + R.tb0) * 8, c->entry.p, R.tb_cnt * 8);
      P.add(p + L.decodebook, c->tables.p, R.dbsize);
      P.add(p + R.o_oidx, c->oidx.p, ocount * 8);
      P.add(p + R.o_oval, c->oval.p, ocount * 8);
    }
    if (R.has_sync && !kept) {
      // The section was recognised by the record's size alone (no host copy of its tag): the kernel
      // looks at the tag and clears a pinned word if it is not one; whoever synchronises the stream
      // next turns that into MGH_ERR_FORMAT (lossless_tag_check) -- a damaged record must not decode
      // quietly with arbitrary synchronisation points.
      HL_TRY(c->tagpin.ensure(64));
      void *dev_word = nullptr;
      if (hipHostGetDevicePointer(&dev_word, c->tagpin.p, 0) == hipSuccess && dev_word) {
        *reinterpret_cast<volatile unsigned *>(c->tagpin.p) = 1;
        P.tag_src = p + R.o_sync - 8;
        P.tag_want = PayloadLayout::kSyncTag;
        P.tag_ok = (unsigned *)dev_word;
        c->tag_pending = true;
      } else {
        (void)hipGetLastError();
      }
    }
    stats.record_bytes_moved += P.total();
    if (!kept) HL_TRY(launch_record_pieces(P, st));
  } else if (!kept) {
    // (a record in device memory: these go device-to-device from the record itself, not back up
    // from the pageable host copy)
    const uint8_t *meta_src = on_dev ? p : c->head.data();
    HL_HIP(hipMemcpyAsync(c->bits.p, meta_src + L.huffmeta + R.tb0 * 8, R.tb_cnt * 8, hipMemcpyDefault, st));
    HL_HIP(hipMemcpyAsync(c->entry.p, meta_src + L.huffmeta + (nchunk + R.tb0) * 8, R.tb_cnt * 8, hipMemcpyDefault, st));
    HL_HIP(hipMemcpyAsync(c->tables.p, meta_src + L.decodebook, R.dbsize, hipMemcpyDefault, st));
    stats.record_bytes_moved += 2 * R.tb_cnt * 8 + R.dbsize;
  }
  if (ocount && !here && !kept) {
    stats.record_bytes_moved += 16 * ocount;
    HL_HIP(hipMemcpyAsync(c->oidx.p, p + R.o_oidx, ocount * 8, hipMemcpyDefault, st));
    HL_HIP(hipMemcpyAsync(c->oval.p, p + R.o_oval, ocount * 8, hipMemcpyDefault, st));
  }
  return MGH_SUCCESS;
}

// `payload` may be host or device memory: only the small leading part of the record is brought
// to the host, the code units and outlier lists go device-to-device (or host-to-device). What the
// record says is read by huffman_record.hpp (record_fixed, record_plan), which decoder takes it by
// its decode_plan; this function fetches, uploads and launches.
// sym16: decode to uint16_t symbols at d_q (the ring decoder only; *sym16 is cleared when another
// decoder had to be used and d_q holds int64 values). require16: d_q holds 16-bit elements and nothing
// else -- a record the ring decoder does not take is refused (sym16_refusal) before anything is queued.
// range (DecodeRange): a prefix or a range writes d_q[0 .. ) from the first integer of its first chunk
// to the end of its last and nothing behind it, and of a record that has to be copied only what those
// chunks need is moved; the decoders run on the chunk-table entries, synchronisation entries and code
// units of the range alone. n_prefix == 0: a context with keep == 1 only (the reader's open).
int lossless_decompress(mgh_lossless_ctx *c, const uint8_t *payload, uint64_t size, int lossless,
                        int64_t *d_q, uint64_t n, uint64_t *ocount_out, hipStream_t st,
                        bool *sym16 = nullptr, bool sync_end = true, const DecodeRange &range = DecodeRange(),
                        bool require16 = false) {
  if (range.n_prefix == 0 && c->keep != 1) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless_decompress: empty prefix");
  if (range.n_prefix != 0 && range.first >= std::min<uint64_t>(range.n_prefix, n))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless_decompress: empty range");
  const bool kept = c->keep == 2;  // head, tables, lists (and the inflated frame) are those of this record already
  const uint8_t *p = payload;
  uint64_t psize = size;
  bool on_dev = is_device_pointer(payload);
  if (lossless == MGH_LOSSLESS_HUFFMAN_ZSTD) {
    HL_TRY(lossless_inflate(c, payload, size, on_dev));
    p = c->host2.data();
    psize = c->host2.size();
    on_dev = false;
  } else if (lossless != MGH_LOSSLESS_HUFFMAN) {
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless: only Huffman and Huffman_Zstd are supported");
  }
  std::vector<uint8_t> &head = c->head;
  auto fetch = [&](size_t upto) -> int {  // make head a host copy of bytes [0, upto) of the record
    if (head.size() >= upto) return MGH_SUCCESS;
    const size_t have = head.size();
    head.resize(upto);
    if (on_dev) HL_TRY(dev_to_host(head.data() + have, p + have, upto - have));
    else std::memcpy(head.data() + have, p + have, upto - have);
    return MGH_SUCCESS;
  };
  if (!kept) head.clear();
  // (a record in device memory: one copy that covers the whole leading part for the default
  // parameters instead of one per field -- every synchronous copy costs tens of microseconds)
  if (psize >= 24) HL_TRY(fetch(std::min<size_t>(psize, on_dev ? 24 + 16 * ((n - 1) / 20480 + 1) + 16 + 8 * 128 + 8 * 8192 + 16 : 24)));
  const DecodeSwitches sw = decode_switches();
  RecordPlan R;
  if (const char *bad = record_fixed(head.data(), head.size(), psize, n, range, c->keep != 0, R))
    return hl_fail(MGH_ERR_FORMAT, bad);
  HL_TRY(fetch(R.L.ddata));
  if (const char *bad = record_plan(head.data(), head.size(), on_dev ? nullptr : p, psize, sw, R))
    return hl_fail(MGH_ERR_FORMAT, bad);
  const DecodePlan D = decode_plan(R, n, sw);
  if (require16)
    if (const char *bad = sym16_refusal(D)) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad);
  const PayloadLayout &L = R.L;
  const size_t nchunk = R.nchunk, ndec = R.ndec, cf = R.cf, ocount = R.ocount;
  const size_t n_out = ndec ? R.n_dec - cf * (size_t)R.chunk : 0;  // integers the call writes
  const size_t units_b = (R.units_need - R.units_lo) * 8;           // bytes of the code units it reads
  hl_debug("lossless_decompress: record head parsed");
  mgh_decompress_stats &stats = decompress_stats();
  stats.chunks_total += nchunk;
  stats.chunks_decoded += ndec - std::min(cf, ndec);
  stats.symbols_decoded += n_out;
  stats.record_bytes += size;
  const bool here = on_dev && is_device_pointer_on(p, c->dev);
  HL_TRY(record_upload(c, p, on_dev, here, R, st));
  const bool ring = D.kind == DecodeKind::ring;
  // A device-resident record is decoded where it is (512^3: 150 MB not copied) -- by the ring
  // decoder wherever its code units start (load_unit), by the others when they start 8-byte
  // aligned. The decoders peek one unit past the stream; in the record that is the outlier count
  // -- the peeked bits lie beyond the last code of the last chunk and never reach a symbol (every
  // chunk stops at its bit count).
  // (only memory of the device the decoder runs on: a record on another GPU is copied over)
  const bool units_in_place = here && R.units && (ring || ((uintptr_t)(p + L.ddata) & 7) == 0);
  const unsigned long long *d_units = (const unsigned long long *)(p + L.ddata);
  bool units_follow = false;
  if (!units_in_place) {
    // (not for units decoded in place: 8 N bytes a lane would hold for nothing. The entries of the
    // chunk table count from the start of the stream: the pointer is moved down by what is left out)
    HL_TRY(c->units.ensure(units_b + 8));
    d_units = (const unsigned long long *)c->units.p - R.units_lo;
    // A large record in HOST memory is decoded while it arrives (below: the ring decoder's launches
    // follow the pieces of the copy, which runs on the cache's copy stream); everything else is
    // copied here, in stream order. (A record in pageable memory travels through the pinned ring.)
    units_follow = !on_dev && ring && units_b >= ((size_t)32 << 20) && cache_copy_stream(c->dev) &&
                   env_get("MGH_HL_DECODE_FOLLOWS", 1) != 0;
    if (units_b && !units_follow) HL_TRY(copy_any(c->units.p, p + L.ddata + R.units_lo * 8, units_b, st));
    HL_HIP(hipMemsetAsync((char *)c->units.p + units_b, 0, 8, st));  // (the decoder peeks one unit ahead)
    stats.record_bytes_moved += units_b;
  }
  hl_debug("lossless_decompress: uploads done");
  static std::atomic<uint64_t> once{0}, once_ring{0}, once_pair{0}, once_par{0};
  HL_TRY(hl_lds_limit(once, 156 * 1024, huff::k_decode));
  hl_debug("lossless_decompress: uploads done (units, tables, outliers)");
  const unsigned long long *tab = (const unsigned long long *)c->tables.p;
  if (ring) {
    // two-level table from the decodebook (host, microseconds); 16 waves per workgroup when the
    // table leaves room
    const uint64_t *book = reinterpret_cast<const uint64_t *>(head.data() + L.decodebook);
    const size_t lds_cap = huff::kRingLdsCap;
    static_assert(huff::kRingWaveLds == huff::kRingUnits * 64 * 8 + 64 * huff::kStageStride * 2, "decode_ring_lds per wave");
    // (kept in the context: the upload below is asynchronous and must not outlive its source)
    std::vector<uint32_t> &dt = c->h_dtable;
    if (!kept) {
      dt = huff::build_decode_table(book, book + 64, book + 128, R.dict, D.rtb,
                                    (lds_cap - huff::kRingMinWaves * huff::kRingWaveLds) / 4 - (D.pair ? ((size_t)1 << D.rtb) : 0));
      if (D.pair) dt = huff::make_pair_table(dt, D.rtb);
      HL_TRY(c->dtable.ensure(dt.size() * 4));
      // (out of pinned memory: a copy from pageable memory is staged synchronously, ~15 us)
      HL_TRY(c->dpin.ensure(dt.size() * 4));
      std::memcpy(c->dpin.p, dt.data(), dt.size() * 4);
      HL_HIP(hipMemcpyAsync(c->dtable.p, c->dpin.p, dt.size() * 4, hipMemcpyHostToDevice, st));
    }
    const int waves = huff::decode_ring_lds(dt.size(), 16) <= lds_cap ? 16 : huff::kRingMinWaves;
    if (huff::decode_ring_lds(dt.size(), waves) > lds_cap)  // (decode_plan and build_decode_table keep the table inside)
      return hl_fail(MGH_ERR_DEVICE, "lossless_decompress: decode table larger than the ring decoder's LDS");
    HL_TRY(hl_lds_limit(once_ring, 156 * 1024, huff::k_decode_ring<int64_t>, huff::k_decode_ring<uint16_t>));
    if (D.pair) HL_TRY(hl_lds_limit(once_pair, 156 * 1024, huff::k_decode_sync<int64_t>, huff::k_decode_sync<uint16_t>));
    // synchronisation points of the encoder, if the record has them: read where they lie in a
    // record on this device (any alignment), else from a copy
    const size_t sync_per = 4 * (size_t)huff::kSyncLanes;
    const uint8_t *d_sync = nullptr;
    size_t sync0 = 0;  // chunk d_sync starts at
    if (D.sync && here) {
      d_sync = p + R.o_sync;
    } else if (D.sync) {
      if (on_dev) {  // (a record on another device: its tag has not been looked at yet)
        uint64_t tag = 0;
        HL_TRY(aux_read(&tag, p + R.o_sync - 8, 8));
        if (tag != PayloadLayout::kSyncTag) return hl_fail(MGH_ERR_FORMAT, "Huffman record: outlier lists");
      }
      // (the entries of the chunks decoded)
      const size_t sync_need = sync_per * (ndec - std::min(cf, ndec));
      HL_TRY(c->sync.ensure(std::max<size_t>(sync_need, sync_per)));
      if (sync_need) HL_HIP(hipMemcpyAsync(c->sync.p, p + R.o_sync + sync_per * cf, sync_need, hipMemcpyDefault, st));
      stats.record_bytes_moved += sync_need;
      d_sync = (const uint8_t *)c->sync.p;
      sync0 = cf;
    }
    const size_t lds_b = huff::decode_ring_lds(dt.size(), waves);
    // chunks [c0, c1): the kernels index everything by chunk, so a range is the same launch with
    // the per-chunk arrays, the output and the symbol count moved up by c0 chunks
    auto launch_range = [&](size_t c0, size_t c1, auto *q) -> int {
      if (c1 <= c0) return MGH_SUCCESS;
      using OUT = std::remove_pointer_t<decltype(q)>;
      const auto kernel = D.pair ? huff::k_decode_sync<OUT> : huff::k_decode_ring<OUT>;
      const size_t cnt = c1 - c0;
      kernel<<<(unsigned)((cnt + waves - 1) / waves), 64 * waves, lds_b, st>>>(
          d_units, (const unsigned long long *)c->bits.p + (c0 - R.tb0), (const unsigned long long *)c->entry.p + (c0 - R.tb0),
          cnt, R.chunk, R.n_dec - c0 * (size_t)R.chunk, R.dict, D.rtb, (const unsigned *)c->dtable.p, (unsigned)dt.size(),
          tab, tab + 64, tab + 128, q + (c0 - cf) * (size_t)R.chunk,
          d_sync ? reinterpret_cast<const unsigned *>(d_sync + (c0 - sync0) * sync_per) : nullptr);
      HL_HIP(hipGetLastError());
      return MGH_SUCCESS;
    };
    auto launch = [&](size_t c0, size_t c1) -> int {
      return sym16 && *sym16 ? launch_range(c0, c1, (uint16_t *)d_q) : launch_range(c0, c1, d_q);
    };
    if (units_follow) {
      // the record's code units on the copy stream, piece by piece; behind every piece the chunks
      // whose units have landed (chunks_landed) are decoded on st
      const uint64_t *h_bits = reinterpret_cast<const uint64_t *>(head.data() + L.huffmeta);
      size_t c_done = cf;
      const ChunkFn on_piece = [&](size_t off, size_t nb, hipEvent_t landed) -> int {
        const size_t c_hi = chunks_landed(R, h_bits, h_bits + nchunk, c_done, R.units_lo + (off + nb) / 8, off + nb >= units_b);
        if (c_hi > c_done) {
          HL_HIP(hipStreamWaitEvent(st, landed, 0));
          HL_TRY(launch(c_done, c_hi));
          c_done = c_hi;
        }
        return MGH_SUCCESS;
      };
      // (the copy stream must not run ahead of what st has queued in front: the small uploads above
      // are independent of the units; the units buffer itself is free -- the caller drained st)
      HL_TRY(copy_any(c->units.p, p + L.ddata + R.units_lo * 8, units_b, cache_copy_stream(c->dev), &on_piece));
      if (c_done < ndec) return hl_fail(MGH_ERR_DEVICE, "lossless_decompress: chunks left behind the last piece");
    } else {
      HL_TRY(launch(cf, ndec));
    }
  } else if (D.kind != DecodeKind::none) {
    if (sym16) *sym16 = false;
    // parallel inside the chunks, one wave per chunk (k_decode_par), or one lane per chunk (k_decode)
    const bool par = D.kind == DecodeKind::par;
    if (par) HL_TRY(hl_lds_limit(once_par, 156 * 1024, huff::k_decode_par));
    const auto kernel = par ? huff::k_decode_par : huff::k_decode;
    const unsigned per_group = par ? huff::kParWaves : 64, threads = par ? 64 * huff::kParWaves : 64;
    kernel<<<(unsigned)((ndec - cf + per_group - 1) / per_group), threads, D.lds, st>>>(
        d_units, (const unsigned long long *)c->bits.p + (cf - R.tb0), (const unsigned long long *)c->entry.p + (cf - R.tb0),
        ndec - cf, R.chunk, n_out, R.dict, D.tb, tab, tab + 64, tab + 128, d_q);
  }
  HL_HIP(hipGetLastError());
  hl_debug("lossless_decompress: decode launched");
  // the host payload may go away when we return (the subdomain pipeline keeps it, and the context's
  // host-side sources, alive until the lane has drained: sync_end = false)
  *ocount_out = ocount;
  if (c->keep == 1) c->keep = 2;
  if (sync_end) {
    HL_HIP(hipStreamSynchronize(st));
    return lossless_tag_check(c);
  }
  return MGH_SUCCESS;
}

// ---- domain decomposition: its host logic is domain_plan.hpp -------------------------------------
// a refusal of domain_plan.hpp as a status of this file
inline int hl_plan(const Refusal &r) { return r.msg ? hl_fail(r.code, r.msg) : MGH_SUCCESS; }

int make_decomposer(Decomposer &dd, int D, const uint64_t *shape, size_t elem, const mgh_config &cfg) {
  size_t free_b = 0, total_b = 0;
  HL_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t avail = std::min<size_t>(free_b, cfg.max_memory_footprint);
  return hl_plan(split_domain(dd, D, shape, elem, avail, cfg.domain_decomposition, cfg.block_size,
                              cfg.domain_decomposition_dim, cfg.domain_decomposition_sizes,
                              cfg.num_domain_decomposition_sizes, cfg.estimate_outlier_ratio, cfg.huff_dict_size,
                              cfg.huff_block_size));
}

// ---- host side of the host <-> device transfers ----------------------------------------------
// Numbers of the box the design follows (tools/micro/host_link.hip, 512 MB): pinned DMA 57.6 GB/s
// either way in one piece, 56.7 in 64 MB pieces, 55.2 in 16 MB pieces; memcpy pageable <-> pinned
// 32 GB/s on one thread, 85 on 4, 120 on 8; a ring of four pinned 16-32 MB slots filled by 4
// persistent threads while the DMA drains them: 52-53 GB/s; first touch of 512 MB of fresh 4 KB
// pages 72 ms on one thread (40 ms inside hipMemcpy), 3 ms with transparent huge pages and 8 threads;
// hipHostRegister of 512 MB 16 ms.
//
// Copy pool: a few persistent threads of the calling thread (released with its cache). A job is
// a function over part numbers; whoever waits for a job works on it too, so a job always
// completes even when the workers are busy with an earlier one. (Round 5 spawned 7 std::threads
// per 32 MB chunk.)
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
}
// CPUs next to the current device (local_cpulist of its PCI function), empty when sysfs does not say.
// The boxes seen have two sockets and the GPU hangs on one of them: copy threads on the other
// socket write the pinned slots across the socket link (512^3 f32 host to host, pageable, whole
// process on the GPU's node 14.9 / 14.4 ms, on the other node 15.7 / 16.5 ms: tools/exp_numa.sh).
inline std::vector<int> device_local_cpus() {
  std::vector<int> cpus;
  int dev = 0;
  char bus[64] = {0};
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetPCIBusId(bus, sizeof bus, dev) != hipSuccess) {
    (void)hipGetLastError();
    return cpus;
  }
  for (char *q = bus; *q; q++) *q = (char)std::tolower((unsigned char)*q);
  const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/local_cpulist";
  std::FILE *f = std::fopen(path.c_str(), "r");
  if (!f) return cpus;
  char line[4096] = {0};
  if (std::fgets(line, sizeof line, f)) {
    for (char *tok = std::strtok(line, ",\n"); tok; tok = std::strtok(nullptr, ",\n")) {
      int a = 0, b = 0;
      if (std::sscanf(tok, "%d-%d", &a, &b) == 2) {
        for (int c = a; c <= b && c < CPU_SETSIZE; c++) cpus.push_back(c);
      } else if (std::sscanf(tok, "%d", &a) == 1 && a < CPU_SETSIZE) {
        cpus.push_back(a);
      }
    }
  }
  std::fclose(f);
  return cpus;
}

struct HostPool {
  static constexpr int kMaxWorkers = 31;
  std::vector<int> near_cpus;  // where the workers run (MGH_HL_COPY_AFFINITY=0: wherever the scheduler puts them)
  int kWorkers = (int)env_get("MGH_HL_COPY_THREADS", 5) - 1;  // copy threads beside the calling one
  struct Job {
    std::function<void(int)> fn;
    int nparts = 0;
    std::atomic<int> next{0}, done{0};
  };
  std::thread th[kMaxWorkers];
  bool started = false;
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<uint64_t> gen{0};
  std::shared_ptr<Job> cur;  // (guarded by mu)
  bool stop = false;

  static void work(Job &j) {
    for (;;) {
      const int p = j.next.fetch_add(1, std::memory_order_relaxed);
      if (p >= j.nparts) break;
      j.fn(p);
      j.done.fetch_add(1, std::memory_order_release);
    }
  }
  void worker() {
    if (!near_cpus.empty()) {
      cpu_set_t set;
      CPU_ZERO(&set);
      for (int c : near_cpus) CPU_SET(c, &set);
      (void)pthread_setaffinity_np(pthread_self(), sizeof set, &set);  // (refused by a cpuset: stay where we are)
    }
    uint64_t seen = 0;
    for (;;) {
      std::shared_ptr<Job> j;
      // a chunked transfer posts a job every few hundred microseconds: poll that long before sleeping
      for (int spin = 0; spin < 4000 && gen.load(std::memory_order_acquire) == seen; spin++) cpu_relax();
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || gen.load(std::memory_order_acquire) != seen; });
        if (stop) return;
        seen = gen.load(std::memory_order_acquire);
        j = cur;
      }
      if (j) work(*j);
    }
  }
  std::shared_ptr<Job> post(std::function<void(int)> fn, int nparts) {
    auto j = std::make_shared<Job>();
    j->fn = std::move(fn);
    j->nparts = nparts;
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!started) {
        if (env_get("MGH_HL_COPY_AFFINITY", 1) != 0) near_cpus = device_local_cpus();
        for (int k = 0; k < kWorkers; k++) th[k] = std::thread([this] { worker(); });
        started = true;
      }
      cur = j;
      gen.fetch_add(1, std::memory_order_release);
    }
    cv.notify_all();
    return j;
  }
  static void wait(Job &j) {
    work(j);
    while (j.done.load(std::memory_order_acquire) < j.nparts) cpu_relax();
  }
  void run(std::function<void(int)> fn, int nparts) {
    auto j = post(std::move(fn), nparts);
    wait(*j);
  }
  // dst <- src on the pool (both host memory)
  void copy(void *dst, const void *src, size_t bytes) {
    if (bytes < ((size_t)1 << 20)) {
      std::memcpy(dst, src, bytes);
      return;
    }
    // one part per thread: smaller parts taken as the threads get to them measured slower (profiles/NOTES.md)
    const int kParts = (int)std::max<size_t>(1, std::min<size_t>(kWorkers + 1, bytes >> 18));
    const size_t part = (bytes / kParts + 4095) / 4096 * 4096;
    run([=](int t) {
      const size_t lo = std::min(bytes, (size_t)t * part), hi = std::min(bytes, (size_t)(t + 1) * part);
      if (hi > lo) std::memcpy((char *)dst + lo, (const char *)src + lo, hi - lo);
    }, kParts);
  }
  void shutdown() {
    {
      std::lock_guard<std::mutex> lk(mu);
      if (!started) return;
      stop = true;
    }
    cv.notify_all();
    for (int k = 0; k < kWorkers; k++) th[k].join();
    started = false;
    stop = false;
    cur.reset();
  }
};
thread_local HostPool *g_pool_ptr = nullptr;
// The pool's worker threads end with the thread that owns them (a thread_local destructor: joining
// std::threads makes no HIP call, unlike the release of the cache and the pinned rings, which stays
// with mgh_release_cache) -- a caller thread that exits without releasing leaves memory behind, not
// threads.
struct HostPoolGuard {
  ~HostPoolGuard() {
    if (g_pool_ptr) {
      g_pool_ptr->shutdown();
      delete g_pool_ptr;
      g_pool_ptr = nullptr;
    }
  }
};
inline HostPool &host_pool() {
  static thread_local HostPoolGuard guard;
  (void)guard;
  if (!g_pool_ptr) g_pool_ptr = new HostPool();
  return *g_pool_ptr;
}

// Ring of pinned slots between PAGEABLE host memory and the device: the pool fills (drains) slot
// c % kSlots while the DMA engine works on the slots before it. (The reference registers the
// caller's buffers instead -- auto_pin_host_buffers -- at 16 ms per 512 MB on this box, and see
// mgh_config_default.) One ring per direction and thread, released with the cache.
struct PinnedRing {
  static constexpr int kSlots = 4;
  size_t kChunk = (size_t)env_get("MGH_HL_RING_MB", 16) << 20;
  void *buf[kSlots] = {};
  hipEvent_t ev[kSlots] = {};
  int dev = -1;  // device the events belong to
  int ensure(bool buffers) {
    int cur = 0;
    HL_HIP(hipGetDevice(&cur));
    if (cur != dev) {  // events recorded into another device's stream fail: recreate them
      release();
      dev = cur;
    }
    for (int i = 0; i < kSlots; i++) {
      if (buffers && !buf[i]) HL_HIP(hipHostMalloc(&buf[i], kChunk, hipHostMallocDefault));
      if (!ev[i]) HL_HIP(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    }
    return MGH_SUCCESS;
  }
  void release() {
    for (int i = 0; i < kSlots; i++) {
      if (buf[i]) (void)hipHostFree(buf[i]);
      if (ev[i]) (void)hipEventDestroy(ev[i]);
      buf[i] = nullptr;
      ev[i] = nullptr;
    }
  }
};
// One ring per direction: the host->device prefetch of subdomain id+1 and the device->host copy of
// record id run on different streams of the same thread and must not share slots.
thread_local PinnedRing *g_ring_ptr[2] = {nullptr, nullptr};
inline PinnedRing &ring(int dir) {
  if (!g_ring_ptr[dir]) g_ring_ptr[dir] = new PinnedRing();
  return *g_ring_ptr[dir];
}
void release_host_transfer_state() {
  for (auto *&r : g_ring_ptr)
    if (r) {
      r->release();
      delete r;
      r = nullptr;
    }
  if (g_pool_ptr) {
    g_pool_ptr->shutdown();
    delete g_pool_ptr;
    g_pool_ptr = nullptr;
  }
}

// Called for every piece of a host -> device transfer once its copy has been QUEUED on the
// transfer's stream: [off, off + nb) of the destination is complete when `landed` fires (the event
// is recorded again for a later piece: wait for it -- hipStreamWaitEvent -- before returning).

// dst (device) <- src (pageable host). The source is consumed when the call returns; the device
// side is complete in stream order.
int staged_h2d(void *dst, const void *src, size_t bytes, hipStream_t st, const ChunkFn *on_chunk) {
  PinnedRing &b = ring(0);
  HL_TRY(b.ensure(true));
  HostPool &pool = host_pool();
  size_t off = 0;
  for (int c = 0; off < bytes; c++) {
    const int i = c % PinnedRing::kSlots;
    const size_t nb = std::min(b.kChunk, bytes - off);
    HL_HIP(hipEventSynchronize(b.ev[i]));  // the previous transfer out of this slot is done
    pool.copy(b.buf[i], (const char *)src + off, nb);
    HL_HIP(hipMemcpyAsync((char *)dst + off, b.buf[i], nb, hipMemcpyHostToDevice, st));
    HL_HIP(hipEventRecord(b.ev[i], st));
    if (on_chunk) HL_TRY((*on_chunk)(off, nb, b.ev[i]));
    off += nb;
  }
  return MGH_SUCCESS;
}

// dst (pageable host) <- src (device), after everything queued on st. Complete on return.
int staged_d2h(void *dst, const void *src, size_t bytes, hipStream_t st) {
  PinnedRing &b = ring(1);
  HL_TRY(b.ensure(true));
  HostPool &pool = host_pool();
  constexpr int K = PinnedRing::kSlots;
  size_t off = 0, done = 0;
  size_t len[K] = {};
  int c = 0;
  for (; off < bytes; c++) {
    const int i = c % K;
    HL_HIP(hipEventSynchronize(b.ev[i]));  // (c < K: a transfer of an earlier call may still use the slot)
    if (c >= K) {  // drain the slot we are about to reuse
      pool.copy((char *)dst + done, b.buf[i], len[i]);
      done += len[i];
    }
    len[i] = std::min(b.kChunk, bytes - off);
    HL_HIP(hipMemcpyAsync(b.buf[i], (const char *)src + off, len[i], hipMemcpyDeviceToHost, st));
    HL_HIP(hipEventRecord(b.ev[i], st));
    off += len[i];
  }
  for (int k = std::max(0, c - K); k < c; k++) {
    const int i = k % K;
    HL_HIP(hipEventSynchronize(b.ev[i]));
    pool.copy((char *)dst + done, b.buf[i], len[i]);
    done += len[i];
  }
  return MGH_SUCCESS;
}

// contiguous copy between any two of device / pinned host / pageable host memory
int copy_any(void *dst, const void *src, size_t bytes, hipStream_t st, const ChunkFn *on_chunk) {
  constexpr size_t kStagedMin = (size_t)8 << 20;
  const bool dd = is_device_pointer(dst), sd = is_device_pointer(src);
  if (bytes >= kStagedMin) {
    if (dd && !sd && !is_registered_host(src)) return staged_h2d(dst, src, bytes, st, on_chunk);
    if (sd && !dd && !is_registered_host(dst)) return staged_d2h(dst, src, bytes, st);
  }
  if (on_chunk && dd && !sd) {
    // pinned source, a consumer per piece: 64 MB pieces (56.7 GB/s against 57.6 in one piece) for the
    // big transfers, 16 MB (55.2 GB/s) where a consumer that is slower than the link follows the
    // pieces (a record of a few hundred MB and its decoder)
    const size_t kPiece = bytes >= ((size_t)256 << 20) ? (size_t)64 << 20 : (size_t)16 << 20;
    PinnedRing &b = ring(0);
    HL_TRY(b.ensure(false));
    size_t off = 0;
    for (int c = 0; off < bytes; c++) {
      const size_t nb = std::min(kPiece, bytes - off);
      hipEvent_t ev = b.ev[c % PinnedRing::kSlots];
      HL_HIP(hipMemcpyAsync((char *)dst + off, (const char *)src + off, nb, hipMemcpyHostToDevice, st));
      HL_HIP(hipEventRecord(ev, st));
      HL_TRY((*on_chunk)(off, nb, ev));
      off += nb;
    }
    return MGH_SUCCESS;
  }
  HL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, st));
  return MGH_SUCCESS;
}

// Host memory the library hands to the caller (released with free()): 2 MB aligned and advised for
// transparent huge pages -- the first touch of 512 MB costs 3 ms that way instead of 40-70 ms of
// 4 KB faults inside the device -> host copy. `touch`: fault the pages in now, on a few short-lived
// threads the caller joins before it writes (mgh_decompress: while the device decodes).
void *host_alloc_large(size_t bytes) {
  constexpr size_t kHuge = (size_t)2 << 20;
  if (bytes < 4 * kHuge) return std::malloc(bytes);
  void *p = nullptr;
  if (posix_memalign(&p, kHuge, bytes) != 0) return nullptr;
  (void)madvise(p, bytes, MADV_HUGEPAGE);
  return p;
}
struct Pretouch {
  std::vector<std::thread> th;
  void start(void *p, size_t bytes) {
    constexpr int kThreads = 8;
    if (bytes < ((size_t)64 << 20)) return;
    const size_t part = (bytes / kThreads + 4095) / 4096 * 4096;
    for (int t = 0; t < kThreads; t++) {
      const size_t lo = std::min(bytes, (size_t)t * part), hi = std::min(bytes, (size_t)(t + 1) * part);
      if (hi > lo)
        th.emplace_back([=] {
          for (size_t o = lo; o < hi; o += 4096) ((volatile char *)p)[o] = 0;
        });
    }
  }
  void join() {
    for (auto &t : th) t.join();
    th.clear();
  }
  ~Pretouch() { join(); }
};

// The output of a call that allocates it unless the caller brought it (prealloc): in the memory space of
// the call's input (`dev`), device memory or host_alloc_large. A failed call goes out through fail(rc),
// which frees and clears only what alloc() made.
struct OutSlot {
  void **slot;
  bool dev, prealloc;
  int alloc(size_t bytes) const {
    if (prealloc) return MGH_SUCCESS;
    if (dev) HL_HIP(hipMalloc(slot, bytes));
    else if (!(*slot = host_alloc_large(bytes))) return hl_fail(MGH_ERR_OUT_OF_MEMORY, "malloc");
    return MGH_SUCCESS;
  }
  int fail(int rc) const {
    if (rc != MGH_SUCCESS && !prealloc) {
      if (dev) (void)hipFree(*slot); else std::free(*slot);
      *slot = nullptr;
    }
    return rc;
  }
};

// A box of an array <-> a dense buffer, both in memory of the current device: one launch whatever
// the dimension (the reference copies subdomains with its own N-D kernels too:
// DomainDecomposer.hpp:649-845). One wave per row of the box; W = 4- or 8-byte words.
struct BoxCopy {
  uint32_t ext[MGH_MAX_DIM];      // extents of the box, leading 1s
  uint64_t fstride[MGH_MAX_DIM];  // element strides of the full array for those dims
  uint64_t rows;                  // product of all extents but the last
};
template <typename W>
__global__ void __launch_bounds__(256)
k_copy_box(W *__restrict__ dense, W *__restrict__ full, BoxCopy B, int to_dense) {
  const int lane = threadIdx.x & 63;
  for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < B.rows; row += (uint64_t)gridDim.x * 4) {
    uint64_t r = row, fo = 0;
#pragma unroll
    for (int d = MGH_MAX_DIM - 2; d >= 0; d--) {
      const uint64_t q = r / B.ext[d];
      fo += (r - q * B.ext[d]) * B.fstride[d];
      r = q;
    }
    W *f = full + fo;
    W *s = dense + row * B.ext[MGH_MAX_DIM - 1];
    if (to_dense)
      for (uint32_t k = lane; k < B.ext[MGH_MAX_DIM - 1]; k += 64) s[k] = f[k];
    else
      for (uint32_t k = lane; k < B.ext[MGH_MAX_DIM - 1]; k += 64) f[k] = s[k];
  }
}

// copy_subdomain (DomainDecomposer.hpp:649-845): dense subdomain buffer <-> its box inside the
// full array (host or device). Device to device on one GPU: ONE kernel launch. Otherwise as few
// strided copies as the box allows -- one hipMemcpy3DAsync per 3-D sub-box (round 5; a 2-D copy per
// r-plane was 129 calls of ~5 us for a 129^3 block, more than the block's compression).
// copy_box is the general form: a dense buffer of extents `ext` <-> the box at offset `off` of a
// dense array of shape `shape` (a subdomain in the full array; a level array of a subdomain in the
// stitched array of mgh_decompress_coarsened).
int copy_box(const std::vector<uint64_t> &ext, const std::vector<uint64_t> &off, const std::vector<uint64_t> &shape,
             size_t elem, void *sub, const void *full_c, void *full_m, bool to_sub, hipStream_t st) {
  hl_debug(to_sub ? "copy_subdomain: to subdomain" : "copy_subdomain: to original");
  const int D = (int)shape.size();
  if ((int)ext.size() != D || (int)off.size() != D || D < 1 || D > MGH_MAX_DIM)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "copy_box: dimension");
  for (int d = 0; d < D; d++)
    if (ext[d] == 0 || off[d] > shape[d] || ext[d] > shape[d] - off[d])
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, "copy_box: the box leaves the array");
  {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const void *full_any = to_sub ? full_c : (const void *)full_m;
    if ((elem == 4 || elem == 8) && is_device_pointer_on(full_any, dev) && is_device_pointer_on(sub, dev)) {
      BoxCopy B{};
      uint64_t fs = 1, first = 0;
      std::vector<uint64_t> fstr(D);
      for (int d = D - 1; d >= 0; d--) {
        fstr[d] = fs;
        fs *= shape[d];
      }
      B.rows = 1;
      for (int k = 0; k < MGH_MAX_DIM; k++) {
        const int d = k - (MGH_MAX_DIM - D);
        B.ext[k] = d >= 0 ? (uint32_t)ext[d] : 1u;
        B.fstride[k] = d >= 0 ? fstr[d] : 0;
        if (d >= 0) first += off[d] * fstr[d];
        if (k < MGH_MAX_DIM - 1) B.rows *= B.ext[k];
      }
      const unsigned grid = (unsigned)std::min<uint64_t>((B.rows + 3) / 4, 256 * 32);
      char *fp = (char *)const_cast<void *>(full_any) + first * elem;
      if (elem == 4)
        k_copy_box<uint32_t><<<grid, 256, 0, st>>>((uint32_t *)sub, (uint32_t *)fp, B, to_sub ? 1 : 0);
      else
        k_copy_box<uint64_t><<<grid, 256, 0, st>>>((uint64_t *)sub, (uint64_t *)fp, B, to_sub ? 1 : 0);
      HL_HIP(hipGetLastError());
      return MGH_SUCCESS;
    }
  }
  // merge trailing dimensions the box spans completely
  int k = D - 1;
  while (k > 0 && ext[k] == shape[k]) k--;
  // width = ext[k] * prod(shape[k+1:]) contiguous elements; rows along dim k-1
  size_t inner = 1;
  for (int d = k + 1; d < D; d++) inner *= shape[d];
  const size_t width = ext[k] * inner * elem;        // bytes per contiguous run
  const size_t full_pitch = shape[k] * inner * elem;  // distance between runs (dim k-1)
  const size_t rows = k >= 1 ? ext[k - 1] : 1;
  // outer dims 0 .. k-2
  std::vector<uint64_t> idx(std::max(k - 1, 0), 0);
  std::vector<size_t> fstride(D);  // element strides of the full array
  {
    size_t s = 1;
    for (int d = D - 1; d >= 0; d--) {
      fstride[d] = s;
      s *= shape[d];
    }
  }
  if (k == 0) {  // one contiguous run
    const size_t fo = off[0] * fstride[0];
    if (to_sub) return copy_any(sub, (const char *)full_c + fo * elem, width, st);
    return copy_any((char *)full_m + fo * elem, sub, width, st);
  }
  size_t sub_off = 0;
  // slabs of dim k-2 travel in one 3-D copy each (depth = ext[k-2]; the full array's slice pitch is
  // a whole number of its rows); the loop runs over the dims in front of it
  const bool use3d = k >= 2;
  const size_t depth = use3d ? ext[k - 2] : 1;
  const size_t sub_block = rows * width * depth;
  const int outer = use3d ? k - 2 : k - 1;  // dims 0 .. outer-1 are looped over
  for (;;) {
    size_t fo = off[k] * fstride[k];
    if (k >= 1) fo += off[k - 1] * fstride[k - 1];
    if (use3d) fo += off[k - 2] * fstride[k - 2];
    for (int d = 0; d < outer; d++) fo += (off[d] + idx[d]) * fstride[d];
    char *sp = (char *)sub + sub_off;
    char *fp = (char *)const_cast<void *>(to_sub ? full_c : (const void *)full_m) + fo * elem;
    if (use3d) {
      hipMemcpy3DParms pr{};
      // (pitched pointers: pitch in bytes, then the allocation's width in bytes and height in rows)
      const hipPitchedPtr dense = make_hipPitchedPtr(sp, width, width, rows);
      const hipPitchedPtr whole = make_hipPitchedPtr(fp, full_pitch, full_pitch, shape[k - 1]);
      pr.srcPtr = to_sub ? whole : dense;
      pr.dstPtr = to_sub ? dense : whole;
      pr.extent = make_hipExtent(width, rows, depth);
      pr.kind = hipMemcpyDefault;
      HL_HIP(hipMemcpy3DAsync(&pr, st));
    } else if (to_sub) {
      HL_HIP(hipMemcpy2DAsync(sp, width, fp, full_pitch, width, rows, hipMemcpyDefault, st));
    } else {
      HL_HIP(hipMemcpy2DAsync(fp, full_pitch, sp, width, width, rows, hipMemcpyDefault, st));
    }
    sub_off += sub_block;
    int d = outer - 1;
    while (d >= 0) {
      if (++idx[d] < ext[d]) break;
      idx[d] = 0;
      d--;
    }
    if (d < 0) break;
  }
  return MGH_SUCCESS;
}

int copy_subdomain(const Decomposer &dd, uint64_t id, size_t elem, void *sub, const void *full_c,
                   void *full_m, bool to_sub, hipStream_t st) {
  return copy_box(dd.subdomain_shape(id), dd.subdomain_offset(id), dd.shape, elem, sub, full_c, full_m, to_sub, st);
}

// ---- per-thread cache: hierarchies, device buffers, lossless context
// (CompressorCache, CompressionLowLevel/CompressorCache.hpp:139-142) -------------------------
// One compute lane of the subdomain pipeline: a stream with everything a subdomain needs between
// its decomposition and its record (quantized symbols, outlier lists, lossless context, pinned
// scratch). Two lanes: while subdomain k is in histogram -> code construction (host) -> encoder
// -> record on one lane, subdomain k+1 is decomposed and quantized on the other
// (GPUPipelines.hpp:88-207 runs 2 buffers x 3 queues the same way).
struct Lane {
  hipStream_t st = nullptr;
  DevBuf q, q2, ocount, oidx, oval;  // q2: level-linearised copy (config.reorder == 1)
  DevBuf q3;                         // writing from coefficients kept in q: the linearised copy of the integers in q2
  DevBuf sub;                        // decompression: the dense subdomain when the output is not written in place
  DevBuf lvl;                        // full-grid preview: the dense array of the subdomain's level, before it is prolonged
  DevBuf cmp, orig;                  // mgh_verify: scratch of the reduction; the box of a host-resident original
  PinBuf pin;                        // [0, 8) size prefix of a raw record, [16, 24) norm read-back
  mgh_lossless_ctx *ll = nullptr;
  uint64_t ocap = 0;                 // elements oidx / oval hold
  void release() {
    q.release();
    q2.release();
    q3.release();
    ocount.release();
    oidx.release();
    oval.release();
    sub.release();
    lvl.release();
    cmp.release();
    orig.release();
    pin.release();
    if (ll) mgh_lossless_destroy(ll);
    ll = nullptr;
    ocap = 0;
    if (st) (void)hipStreamDestroy(st);
    st = nullptr;
  }
};
constexpr int kLanes = 2;
constexpr int kInBufs = 3;  // subdomain k in its record phase, k+1 being decomposed, k+2 arriving

struct HlCache {
  std::map<std::vector<uint64_t>, mgh_hierarchy *> hier;  // key: lane, dtype, normalize, max_level, shape...
  DevBuf in[kInBufs];
  hipEvent_t in_ready[kInBufs] = {nullptr, nullptr, nullptr};  // the copy into in[b] has landed
  hipEvent_t in_free[kInBufs] = {nullptr, nullptr, nullptr};   // the last reader of in[b] is done (norm phase)
  PinBuf hpin;  // pinned staging of mgh_compress: [64, ...) the header
  Lane lane[kLanes];
  hipStream_t copy_st = nullptr;  // prefetch of the next subdomains (compression), strided write-back (decompression)
  hipStream_t aux_st = nullptr;   // small device -> host reads that must not wait for the lanes
  PinBuf aux_pin;
  DevBuf vres;  // mgh_verify: one mgh_error_stats per subdomain, read back once at the end
  // mgh_compress_masked / mgh_decompress_masked: the filled (or decoded) array; the packed mask with the scan's
  // statistics behind it; the mask's bytes as symbols of the lossless stage
  DevBuf mfill, mwords, msym;
  // the masked readers at reduced resolution: the index lists of the sample, and the sampled packed mask
  DevBuf midx, msamp;
  int dev = -1;
  // device bytes the cache holds now (they are reused, so they count as available to the next call)
  size_t held_bytes() const {
    size_t b = 0;
    for (auto &kv : hier) b += mgh_device_bytes(kv.second);
    for (auto &x : in) b += x.cap;
    b += vres.cap + mfill.cap + mwords.cap + msym.cap + midx.cap + msamp.cap;
    for (auto &l : lane) {
      b += l.q.cap + l.q2.cap + l.q3.cap + l.oidx.cap + l.oval.cap + l.sub.cap + l.orig.cap + l.cmp.cap;
      if (l.ll) b += l.ll->units.cap + l.ll->oidx.cap + l.ll->oval.cap;
    }
    return b;
  }
  void release() {
    for (auto &kv : hier) mgh_hierarchy_destroy(kv.second);
    hier.clear();
    for (auto &b : in) b.release();
    for (auto *arr : {in_ready, in_free})
      for (int b = 0; b < kInBufs; b++) {
        if (arr[b]) (void)hipEventDestroy(arr[b]);
        arr[b] = nullptr;
      }
    hpin.release();
    aux_pin.release();
    vres.release();
    mfill.release();
    mwords.release();
    msym.release();
    midx.release();
    msamp.release();
    for (auto &l : lane) l.release();
    for (hipStream_t *s : {&copy_st, &aux_st}) {
      if (*s) (void)hipStreamDestroy(*s);
      *s = nullptr;
    }
    dev = -1;
  }
};
// Deliberately never destroyed automatically: a thread_local destructor would run HIP calls at
// thread / process exit, possibly after the HIP runtime has started to tear itself down. The
// resources are returned by mgh_release_cache() (like mgard_x::release_cache); a thread that
// exits without calling it leaves them to process teardown.
thread_local HlCache *g_cache_ptr = nullptr;
inline HlCache &hl_cache() {
  if (!g_cache_ptr) g_cache_ptr = new HlCache();
  return *g_cache_ptr;
}
#define g_cache (hl_cache())

hipStream_t cache_copy_stream(int dev) { return g_cache_ptr && g_cache_ptr->dev == dev ? g_cache_ptr->copy_st : nullptr; }

// Small synchronous device -> host read (record sizes, record heads). On the cache's own stream
// and through its pinned buffer: hipMemcpy() would run on the NULL stream and with it wait for
// everything the lanes have queued. Stand-alone calls that never prepared a cache use hipMemcpy.
int aux_read(void *dst, const void *src, size_t bytes) {
  HlCache *c = g_cache_ptr;
  if (!c || !c->aux_st || !c->aux_pin.p) {
    HL_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return MGH_SUCCESS;
  }
  for (size_t off = 0; off < bytes; off += c->aux_pin.cap) {
    const size_t nb = std::min(c->aux_pin.cap, bytes - off);
    HL_HIP(hipMemcpyAsync(c->aux_pin.p, (const char *)src + off, nb, hipMemcpyDeviceToHost, c->aux_st));
    HL_HIP(hipStreamSynchronize(c->aux_st));
    std::memcpy((char *)dst + off, c->aux_pin.p, nb);
  }
  return MGH_SUCCESS;
}

int cache_prepare(int dev) {
  if (g_cache.dev != dev) {
    g_cache.release();
    HL_HIP(hipSetDevice(dev));
    // Default (blocking) flags like the reference's queues (DeviceAdapterHip.h:514): the pipeline
    // streams are ordered against the NULL stream, so a device-resident input that an earlier
    // kernel / copy on the NULL stream (torch's default stream) is still producing is complete
    // before the first pipeline stage reads it, and work the caller queues on the NULL stream
    // afterwards waits for the pipeline. Inputs produced on OTHER non-blocking streams must be
    // synchronised by the caller (include/mgard_hip_compress.h).
    // The two lanes must sit on DIFFERENT hardware queues, or the pipeline is a sequence again. The
    // runtime multiplexes all streams of one priority over a few hardware queues (GPU_MAX_HW_QUEUES,
    // 4 by default) by use count: in a process that already holds many streams -- torch keeps a pool
    // of 32 -- two freshly created ones can share a queue (seen in bench.py: both lanes on one queue,
    // 64 x 512^3 decompression 97 instead of 86 ms). Queues are pooled PER PRIORITY, so the lanes get
    // different priorities (they swap roles with every subdomain, neither is favoured for long), and
    // the copy / small-read streams the third level, away from both.
    int prio_least = 0, prio_greatest = 0;
    HL_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    const bool three = prio_least > 0 && prio_greatest < 0;
    for (int l = 0; l < kLanes; l++) {
      HL_HIP(hipStreamCreateWithPriority(&g_cache.lane[l].st, hipStreamDefault, l == 0 ? 0 : prio_greatest));
      HL_TRY(mgh_lossless_create(&g_cache.lane[l].ll, dev));
    }
    HL_HIP(hipStreamCreateWithPriority(&g_cache.copy_st, hipStreamDefault, three ? prio_least : 0));
    HL_HIP(hipStreamCreateWithPriority(&g_cache.aux_st, hipStreamDefault, three ? prio_least : 0));
    for (auto &e : g_cache.in_ready) HL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto &e : g_cache.in_free) HL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HL_TRY(g_cache.aux_pin.ensure(512 * 1024));
    g_cache.dev = dev;
  }
  return MGH_SUCCESS;
}

// Hierarchy of a subdomain (DomainDecomposer::subdomain_hierarchy, :265-301). Uniform ones
// are cached by shape (at most 4 alive); non-uniform ones are built per subdomain.
constexpr size_t kHierCacheMax = 8 * kLanes;  // (a Block decomposition of a 3-D array has up to 8 subdomain shapes)
// start of a high-level call (nothing in flight): make room when the cache is full
int trim_hierarchy_cache() {
  if (g_cache.hier.size() < kHierCacheMax) return MGH_SUCCESS;
  for (auto &kv : g_cache.hier) mgh_hierarchy_destroy(kv.second);
  g_cache.hier.clear();
  return MGH_SUCCESS;
}

// A hierarchy owns the workspace of the subdomain that runs on it, so the two lanes of the
// pipeline keep separate ones (`lane` is part of the key). cached = false: one of the caller's own,
// always owned (the progressive reader keeps the state of its level loop in it between the calls).
int get_hierarchy(mgh_hierarchy **out, bool *owned, int dtype, const std::vector<uint64_t> &shape,
                  const std::vector<std::vector<double>> *coords, const std::vector<uint64_t> &off,
                  const mgh_config &cfg, int lane = 0, bool cached = true) {
  const int D = (int)shape.size();
  if (!coords) {
    std::vector<uint64_t> key = {(uint64_t)lane, (uint64_t)dtype, (uint64_t)cfg.normalize_coordinates,
                                 cfg.max_larget_level};
    key.insert(key.end(), shape.begin(), shape.end());
    auto it = cached ? g_cache.hier.find(key) : g_cache.hier.end();
    if (it != g_cache.hier.end()) {
      *out = it->second;
      *owned = false;
      return MGH_SUCCESS;
    }
    mgh_hierarchy *h = nullptr;
    HL_TRY(mgh_hierarchy_create(&h, D, shape.data(), dtype, nullptr, cfg.normalize_coordinates,
                                cfg.max_larget_level, cfg.dev_id));
    *out = h;
    // A full cache is emptied between calls only (trim_hierarchy_cache): inside a call a cached
    // hierarchy may be at work on the other lane. A shape that does not fit any more is built for
    // its subdomain alone.
    *owned = !cached || g_cache.hier.size() >= kHierCacheMax;
    if (!*owned) g_cache.hier[key] = h;
    return MGH_SUCCESS;
  }
  // slice of the coordinate arrays, converted to the data type
  std::vector<std::vector<float>> cf(D);
  std::vector<std::vector<double>> cd(D);
  const void *ptrs[MGH_MAX_DIM];
  for (int d = 0; d < D; d++) {
    const double *src = (*coords)[d].data() + off[d];
    if (dtype == MGH_FLOAT) {
      cf[d].assign(src, src + shape[d]);
      ptrs[d] = cf[d].data();
    } else {
      cd[d].assign(src, src + shape[d]);
      ptrs[d] = cd[d].data();
    }
  }
  HL_TRY(mgh_hierarchy_create(out, D, shape.data(), dtype, ptrs, cfg.normalize_coordinates,
                              cfg.max_larget_level, cfg.dev_id));
  *owned = true;
  return MGH_SUCCESS;
}

int header_from(const Decomposer &dd, int dtype, int ebtype, double tol, double s, double norm,
                const std::vector<std::vector<double>> *coords, const mgh_config &cfg, fmt::Header &h) {
  h = fmt::Header();
  h.is_double = dtype == MGH_DOUBLE;
  h.shape = dd.shape;
  h.uniform = coords == nullptr;
  if (coords) h.coords = *coords;
  h.rel = ebtype == MGH_REL;
  h.tol = tol;
  h.s = s;
  h.norm = norm;
  if (dd.decomposed) {
    h.dd_method = dd.method == MGH_DD_MAXDIM ? fmt::DD_MAX_DIMENSION
                  : dd.method == MGH_DD_BLOCK ? fmt::DD_BLOCK : fmt::DD_VARIABLE;
  } else {
    h.dd_method = fmt::DD_NOOP;
  }
  h.dd_dim = dd.dim;
  h.dd_size = dd.size;
  h.hierarchy = fmt::HIER_MULTIDIM;
  h.l_target = 0;  // never filled by the reference (Metadata.hpp:78-113)
  h.reorder = cfg.reorder != 0;
  h.compressor = cfg.lossless == MGH_LOSSLESS_HUFFMAN ? fmt::COMP_X_HUFFMAN : fmt::COMP_X_HUFFMAN_ZSTD;
  h.huff_dict_size = cfg.huff_dict_size;
  h.huff_block_size = cfg.huff_block_size;
  h.backend = fmt::DEV_X_HIP;
  return MGH_SUCCESS;
}

// ---- what the two entries into the writer share (compress_impl from the caller's data, -------------
// ---- CoefficientSession::write from coefficients already on the device) ---------------------------
// What the last writing call of this thread did (mgh_last_compress_stats).
inline mgh_compress_stats &compress_stats() {
  thread_local mgh_compress_stats s{};
  return s;
}

// Where the records of a writing call go: its output and how much of it is used.
struct RecordSink {
  void *out = nullptr;
  size_t cap = 0, byte_offset = 0;
  bool out_dev = false;
};

// The output of a writing call into `sink`: the caller's buffer of *size bytes, or one the call allocates
// for an array of n elements stored raw (CompressionHighLevel.hpp:147-162).
int writer_output(const OutSlot &o, size_t n, size_t elem, const size_t *size, RecordSink &sink) {
  sink.cap = o.prealloc ? *size : n * elem + (size_t)1e6;
  HL_TRY(o.alloc(sink.cap));
  sink.out = *o.slot, sink.out_dev = is_device_pointer(*o.slot);
  return MGH_SUCCESS;
}

// The lane's outlier lists for ocap pairs, their counter and the lane's pinned words.
int ensure_lane_lists(Lane &L, uint64_t ocap) {
  HL_TRY(L.ocount.ensure(8));
  HL_TRY(L.oidx.ensure(ocap * 8));
  HL_TRY(L.oval.ensure(ocap * 8));
  L.ocap = std::max(L.ocap, ocap);  // (grow-only buffers: an earlier call may have left more)
  HL_TRY(L.pin.ensure(64));
  return MGH_SUCCESS;
}

// The header of a writing call and the size of its metadata, behind which the sink's records start. The
// size is known up front: the header does not depend on the payloads, except for the norm of a
// non-decomposed REL run, whose encoding has a fixed length (a non-zero double).
int header_step(const Decomposer &dd, int dtype, int ebtype, double tol, double s, double norm,
                const std::vector<std::vector<double>> *coords, const mgh_config &cfg, RecordSink &sink,
                fmt::Header &hdr, size_t &meta_size) {
  header_from(dd, dtype, ebtype, tol, s, norm, coords, cfg, hdr);
  meta_size = fmt::serialize_metadata(hdr).size();
  if (meta_size > sink.cap) return hl_fail(MGH_ERR_OUTPUT_TOO_LARGE, "output buffer too small for the header");
  sink.byte_offset = meta_size;
  // (sized once, here: an asynchronous copy out of it must never meet a re-allocation)
  return g_cache.hpin.ensure(64 + meta_size);
}

// The lossless stage's job for one subdomain of n elements: the integers q_enc, the lane's outlier lists.
LosslessJob subdomain_job(const Lane &L, const mgh_config &cfg, const int64_t *q_enc, uint64_t n, size_t elem,
                          bool sym16, bool bins_filled) {
  LosslessJob lj;
  lj.d_q = q_enc;
  lj.n = n;
  lj.dict = cfg.huff_dict_size;
  lj.chunk = cfg.huff_block_size;
  lj.lossless = cfg.lossless;
  lj.zstd_level = cfg.zstd_compress_level;
  lj.d_oidx = (const uint64_t *)L.oidx.p;
  lj.d_oval = (const int64_t *)L.oval.p;
  lj.ocount = 0;  // (read back together with the encoder's results)
  lj.d_ocount = (const uint64_t *)L.ocount.p;
  lj.ocap = L.ocap;
  lj.cap_units = n * elem / 8 + 1;
  lj.sym16 = sym16;
  lj.bins_filled = bins_filled;
  return lj;
}

// Whether a host array under this bound has its norm reduced while it arrives (stream_in_with_norm), given
// that the fused path, which takes the streamed norm, runs on its hierarchy (mgh_sym16_supported).
// MGH_HL_STREAM_NORM=0: norm after arrival (cross-check).
bool norm_streams_in(bool in_dev, int ebtype) {
  return !in_dev && ebtype == MGH_REL && env_get("MGH_HL_STREAM_NORM", 1) != 0;
}

// One subdomain arriving from the host under a REL bound: into dst on the copy stream, in_ready[0] behind
// it, its norm reduced piece by piece on the lane's stream lst while the following pieces are still on
// the link (the norm pass is a pure reduction). For s != inf the norm is a sum over these pieces, so both
// entries into the writer come through here: their headers hold the same bits.
int stream_in_with_norm(mgh_hierarchy *h, void *dst, const void *src, size_t bytes, size_t elem, double s,
                        hipStream_t lst) {
  HL_TRY(mgh_norm_stream_begin(h, lst));
  const size_t warm = (size_t)192 << 20;  // (what the level pass may still find cached)
  const ChunkFn on_piece = [=](size_t off, size_t nb, hipEvent_t landed) -> int {
    HL_HIP(hipStreamWaitEvent(lst, landed, 0));
    return mgh_norm_stream_add(h, (const char *)dst + off, nb / elem, s, off + nb + warm < bytes ? 1 : 0, lst);
  };
  HL_TRY(copy_any(dst, src, bytes, g_cache.copy_st, &on_piece));
  if (hipEventRecord(g_cache.in_ready[0], g_cache.copy_st) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipEventRecord");
  return MGH_SUCCESS;
}

// The second half of a subdomain's lossless stage (lossless_begin is queued on the lane), with the retry
// of an outlier overflow: estimate_outlier_ratio was too optimistic, so the lane's lists grow to what the
// subdomain needs and `again()` quantizes it once more and queues lossless_begin for the job `lj` then
// describes (LinearQuantization.hpp:621-676 re-launches the same way).
template <typename Again>
int encode_record(Lane &L, const LosslessJob &lj, const RecordSink &S, Again &&again) {
  int frc = MGH_SUCCESS;
  for (int attempt = 0; attempt < 2; attempt++) {
    const bool direct_ok = S.out_dev && S.cap - S.byte_offset > 8;
    frc = lossless_finish(L.ll, lj, L.st, direct_ok ? (uint8_t *)S.out + S.byte_offset + 8 : nullptr,
                          direct_ok ? S.cap - S.byte_offset - 8 : 0);
    if (frc != kOutlierOverflow) break;
    if (attempt == 1) return hl_fail(MGH_ERR_DEVICE, "outlier lists overflowed twice");
    const uint64_t need = L.ll->outliers_needed;
    HL_TRY(L.oidx.ensure(need * 8));
    HL_TRY(L.oval.ensure(need * 8));
    L.ocap = need;
    compress_stats().outlier_retries++;
    HL_TRY(again());
  }
  return frc;
}

// The record encode_record left in the lane's context -- or the dense subdomain `dense_in` itself where
// the record is not smaller (a RAW record) -- behind its size prefix at the sink's offset. `last_hdr`
// (the container's last record): the metadata, of meta_size bytes, travels on the record's stream, in
// front of the synchronisation that record needs anyway; it comes out of g_cache.hpin, which the
// caller has sized. Ends with the lane synchronised. no_raw_layer >= 0 (mgh_compress_layers: a residual
// layer's "data" is no array a reader could take in its place): a record the RAW rule would store raw
// ends the call instead, with nothing written.
int write_record(Lane &L, uint64_t n, size_t elem, const void *dense_in, RecordSink &S, const fmt::Header *last_hdr,
                 size_t meta_size, int no_raw_layer = -1, const char *who = "compress_layers: ") {
  hipStream_t st = L.st;
  uint64_t csize = L.ll->record_size();
  const bool raw = (double)(n * elem) / (double)csize < 1.0;  // GPUPipelines.hpp:136-155
  if (raw && no_raw_layer >= 0)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + "layer " + std::to_string(no_raw_layer) + " would be stored raw");
  if (raw) csize = n * elem;
  if (csize > S.cap - S.byte_offset || S.cap - S.byte_offset - csize < 8)
    return hl_fail(MGH_ERR_OUTPUT_TOO_LARGE, "Output too large");
  char *dst = (char *)S.out + S.byte_offset;
  const bool prefix_with_record = S.out_dev && !raw;  // (one copy: size prefix + head of the record)
  if (S.out_dev && raw) {
    std::memcpy(L.pin.p, &csize, 8);
    HL_HIP(hipMemcpyAsync(dst, L.pin.p, 8, hipMemcpyHostToDevice, st));
  } else if (!S.out_dev) {
    std::memcpy(dst, &csize, 8);
  }
  dst += 8;
  if (raw) {
    // the dense subdomain itself (the decomposition does not modify its input, so the buffer still
    // holds it)
    HL_TRY(copy_any(dst, dense_in, csize, st));
  } else {
    const uint64_t cs64 = csize;
    HL_TRY(record_write(L.ll, dst, st, prefix_with_record ? &cs64 : nullptr));
  }
  if (last_hdr) {
    const std::vector<uint8_t> meta = fmt::serialize_metadata(*last_hdr);
    if (meta.size() != meta_size) return hl_fail(MGH_ERR_FORMAT, "metadata size changed");
    if (S.out_dev) {
      // (out of pinned memory: the copy is queued, not staged synchronously)
      std::memcpy((char *)g_cache.hpin.p + 64, meta.data(), meta.size());
      HL_HIP(hipMemcpyAsync(S.out, (char *)g_cache.hpin.p + 64, meta.size(), hipMemcpyHostToDevice, st));
    } else {
      std::memcpy(S.out, meta.data(), meta.size());
    }
  }
  if (hipStreamSynchronize(st) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "writing the subdomain record");
  hl_debug("compress: record written");
  compress_stats().records++;
  compress_stats().raw_records += raw ? 1 : 0;
  S.byte_offset += 8 + csize;
  return MGH_SUCCESS;
}

template <typename T>
int compress_impl(int D, int dtype, const uint64_t *shape, double tol_d, double s_d, int ebtype,
                  const void *original, void **compressed, size_t *compressed_size,
                  const void *const *coords_in, const mgh_config &cfg, bool prealloc) {
  compress_stats() = mgh_compress_stats{};
  HL_TRY(cache_prepare(cfg.dev_id));
  HL_TRY(trim_hierarchy_cache());
  const T tol = (T)tol_d, s = (T)s_d;
  size_t total = 1;
  for (int d = 0; d < D; d++) total *= shape[d];
  const size_t elem = sizeof(T);
  const bool in_dev = is_device_pointer(original);
  Decomposer dd;
  HL_TRY(make_decomposer(dd, D, shape, elem, cfg));
  std::vector<std::vector<double>> coords;
  if (coords_in) {
    coords.resize(D);
    for (int d = 0; d < D; d++) {
      const T *c = static_cast<const T *>(coords_in[d]);
      coords[d].assign(c, c + shape[d]);
    }
  }
  const std::vector<std::vector<double>> *cptr = coords_in ? &coords : nullptr;
  // output buffer, same memory space as the input
  const OutSlot slot{compressed, in_dev, prealloc};
  RecordSink sink;
  HL_TRY(writer_output(slot, total, elem, compressed_size, sink));
  // pin the host buffers for asynchronous transfers (auto_pin_host_buffers,
  // CompressionHighLevel.hpp:164-189: input and output)
  bool pinned_here = false, out_pinned_here = false;
  if (!in_dev && cfg.auto_pin_host_buffers && !is_registered_host(original)) {
    if (hipHostRegister(const_cast<void *>(original), total * elem, hipHostRegisterDefault) == hipSuccess)
      pinned_here = true;
    else
      (void)hipGetLastError();
  }
  if (!sink.out_dev && cfg.auto_pin_host_buffers && !is_registered_host(*compressed)) {
    if (hipHostRegister(*compressed, sink.cap, hipHostRegisterDefault) == hipSuccess)
      out_pinned_here = true;
    else
      (void)hipGetLastError();
  }
  // MGH_HL_PIPELINE=0: every subdomain runs start to end before the next one is queued (cross-check;
  // same container byte for byte up to the order of the outlier lists)
  const bool pipelined = env_get("MGH_HL_PIPELINE", 1) != 0;
  int nlanes = dd.num > 1 && pipelined ? kLanes : 1;
  auto drain = [&] {  // nothing of this call may be in flight when it returns
    for (int l = 0; l < kLanes; l++) (void)hipStreamSynchronize(g_cache.lane[l].st);
    (void)hipStreamSynchronize(g_cache.copy_st);
  };
  std::vector<mgh_hierarchy *> owned_alive;  // per-subdomain hierarchies (non-uniform grids) not yet destroyed
  auto cleanup = [&](int rc) {
    if (rc != MGH_SUCCESS) drain();
    for (mgh_hierarchy *h : owned_alive) mgh_hierarchy_destroy(h);
    owned_alive.clear();
    if (pinned_here) (void)hipHostUnregister(const_cast<void *>(original));
    if (out_pinned_here) (void)hipHostUnregister(*compressed);
    return slot.fail(rc);
  };
  const uint64_t max_elems = dd.max_subdomain_elems();
  const uint64_t ocap = std::max<uint64_t>(1, (uint64_t)(cfg.estimate_outlier_ratio * (double)max_elems));
  // device-resident input whose subdomains are contiguous slabs: compress them where they are
  const bool zero_copy = in_dev && dd.all_contiguous();
  int nbufs = zero_copy ? 0 : (int)std::min<uint64_t>(dd.num, nlanes > 1 ? kInBufs : 2);
  // The subdomain sizes follow the REFERENCE's footprint estimate (make_decomposer). What this
  // implementation keeps resident is different -- less per subdomain, but the two-lane pipeline
  // holds up to three inputs and two sets of everything else: where that set does not fit what is
  // free (plus what the cache already holds), the schedule falls back to one lane and two inputs
  // instead of failing in an allocation half way through.
  if (nlanes > 1) {
    size_t free_b = 0, total_b = 0;
    HL_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t avail = std::min<size_t>(free_b + g_cache.held_bytes(), cfg.max_memory_footprint);
    if (own_resident_bytes(D, max_elems, elem, cfg.reorder != 0, ocap, nlanes, nbufs) > avail) {
      nlanes = 1;
      nbufs = zero_copy ? 0 : (int)std::min<uint64_t>(dd.num, 2);
    }
  }
  auto sub_in = [&](uint64_t id) -> const void * {
    return zero_copy ? (const void *)((const char *)original + dd.linear_offset(id) * elem)
                     : (const void *)g_cache.in[id % nbufs].p;
  };
  // subdomain id into its input buffer on the copy stream; in_ready[buffer] fires when it has landed
  auto fetch_sub = [&](uint64_t id) -> int {
    if (zero_copy) return MGH_SUCCESS;
    const int b = (int)(id % nbufs);
    HL_TRY(copy_subdomain(dd, id, elem, g_cache.in[b].p, original, nullptr, true, g_cache.copy_st));
    HL_HIP(hipEventRecord(g_cache.in_ready[b], g_cache.copy_st));
    return MGH_SUCCESS;
  };
  int rc;
  auto ensure_all = [&]() -> int {
    for (int b = 0; b < nbufs; b++) HL_TRY(g_cache.in[b].ensure(max_elems * elem));
    for (int l = 0; l < nlanes; l++) {
      Lane &L = g_cache.lane[l];
      HL_TRY(L.q.ensure(max_elems * 8));
      if (cfg.reorder) HL_TRY(L.q2.ensure(max_elems * 8));
      HL_TRY(ensure_lane_lists(L, ocap));
    }
    return MGH_SUCCESS;
  };
  if ((rc = ensure_all()) != MGH_SUCCESS) return cleanup(rc);

  // norm of the whole domain when it is decomposed (calc_norm_decomposed_w_prefetch)
  T norm = 1;
  T local_tol = tol;
  int local_eb = ebtype;
  if (dd.decomposed) {
    if (ebtype == MGH_REL) {
      // every subdomain's norm is left on the device (one slot each) and all of them come back in
      // one copy: no host round trip between the reductions
      hipStream_t st = g_cache.lane[0].st;
      DevBuf &slots = g_cache.lane[0].q;  // (free until the pipeline starts)
      if ((rc = g_cache.aux_pin.ensure(std::max<size_t>(512 * 1024, dd.num * sizeof(T)))) != MGH_SUCCESS)
        return cleanup(rc);
      if ((rc = slots.ensure(dd.num * sizeof(T))) != MGH_SUCCESS) return cleanup(rc);
      for (uint64_t id = 0; id < dd.num; id++) {
        if (!zero_copy) {
          // (the buffers in turn: the copy of id waits for the reduction that read id - nbufs)
          if (id >= (uint64_t)nbufs && hipStreamWaitEvent(g_cache.copy_st, g_cache.in_free[id % nbufs], 0) != hipSuccess)
            return cleanup(hl_fail(MGH_ERR_DEVICE, "hipStreamWaitEvent"));
          if ((rc = fetch_sub(id)) != MGH_SUCCESS) return cleanup(rc);
          if (hipStreamWaitEvent(st, g_cache.in_ready[id % nbufs], 0) != hipSuccess)
            return cleanup(hl_fail(MGH_ERR_DEVICE, "hipStreamWaitEvent"));
        }
        mgh_hierarchy *h = nullptr;
        bool owned = false;
        const auto sshape = dd.subdomain_shape(id);
        if ((rc = get_hierarchy(&h, &owned, dtype, sshape, nullptr, dd.subdomain_offset(id), cfg, 0)) != MGH_SUCCESS)
          return cleanup(rc);
        if (owned) owned_alive.push_back(h);
        rc = mgh_norm_device(h, sub_in(id), s_d, (char *)slots.p + id * sizeof(T), st);
        if (rc != MGH_SUCCESS) return cleanup(rc);
        if (!zero_copy && hipEventRecord(g_cache.in_free[id % nbufs], st) != hipSuccess)
          return cleanup(hl_fail(MGH_ERR_DEVICE, "hipEventRecord"));
      }
      if (hipMemcpyAsync(g_cache.aux_pin.p, slots.p, dd.num * sizeof(T), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        return cleanup(hl_fail(MGH_ERR_DEVICE, "norms of the subdomains"));
      for (mgh_hierarchy *h : owned_alive) mgh_hierarchy_destroy(h);
      owned_alive.clear();
      NormAccumulator na{s == std::numeric_limits<T>::infinity(), cfg.normalize_coordinates != 0};
      for (uint64_t id = 0; id < dd.num; id++) {
        uint64_t cnt = 1;
        for (uint64_t e : dd.subdomain_shape(id)) cnt *= e;
        na.add((double)((const T *)g_cache.aux_pin.p)[id], cnt);
      }
      norm = (T)na.result(total);
    }
    local_tol = local_abs_tol<T>(ebtype, norm, tol, s, dd.num);
    local_eb = MGH_ABS;  // CompressionHighLevel.hpp:135-138
  }

  // (the norm of a non-decomposed REL run is the pipeline's to compute: any non-zero double stands in)
  fmt::Header hdr;
  size_t meta_size;
  if ((rc = header_step(dd, dtype, ebtype, tol_d, s_d, ebtype == MGH_REL ? (dd.decomposed ? (double)norm : 1.0) : 0.0,
                        cptr, cfg, sink, hdr, meta_size)) != MGH_SUCCESS)
    return cleanup(rc);

  // ---- subdomain pipeline (compress_pipeline_gpu, GPUPipelines.hpp:69-207) ----
  // issue(k): decomposition + quantizer + histogram of subdomain k queued on lane k % nlanes, no
  // host synchronisation; finish(k): code construction, encoder, record -- the host waits for lane
  // k % nlanes only. With two lanes issue(k + 1) is queued BEFORE finish(k), so the device has the
  // next subdomain's level passes and solves to run while this one's histogram travels to the
  // host and its encoder runs; the input of k + 2 arrives on the copy stream meanwhile.
  struct SubJob {
    uint64_t id = 0, n = 0;
    int lane = 0;
    mgh_hierarchy *h = nullptr;
    bool owned = false, sym16 = false, norm_deferred = false;
    double norm_out = 0;
    LosslessJob lj;
  };
  // (pre_h: the hierarchy of a subdomain whose norm was reduced while it arrived, see below)
  mgh_hierarchy *pre_h = nullptr;
  bool pre_owned = false;
  auto issue = [&](SubJob &J, uint64_t id) -> int {
    J = SubJob();
    J.id = id;
    J.lane = (int)(id % nlanes);
    Lane &L = g_cache.lane[J.lane];
    hipStream_t st = L.st;
    const auto sshape = dd.subdomain_shape(id);
    J.n = 1;
    for (uint64_t e : sshape) J.n *= e;
    if (!zero_copy) HL_HIP(hipStreamWaitEvent(st, g_cache.in_ready[id % nbufs], 0));
    if (pre_h) {
      J.h = pre_h;
      J.owned = pre_owned;
      pre_h = nullptr;
    } else {
      HL_TRY(get_hierarchy(&J.h, &J.owned, dtype, sshape, cptr, dd.subdomain_offset(id), cfg, J.lane));
      if (J.owned) owned_alive.push_back(J.h);
    }
    hl_debug("compress: subdomain ready");
    // (outlier counter of the lane + the lossless stage's bins and chunk states: one launch, here)
    if (cfg.reorder || cfg.lossless == MGH_LOSSLESS_HUFFMAN_ZSTD) {
      HL_HIP(hipMemsetAsync(L.ocount.p, 0, 8, st));
    } else {
      HL_TRY(lossless_prepare(L.ll, J.n, cfg.huff_dict_size, cfg.huff_block_size, st, (unsigned long long *)L.ocount.p));
      if (!L.ll->prepared_n) HL_HIP(hipMemsetAsync(L.ocount.p, 0, 8, st));
    }
    J.norm_out = (double)norm;
    // 16-bit symbols straight from the quantizer where the fused kernels run (a quarter of the
    // bytes written by the quantizer and read twice by the lossless stage); int64 otherwise
    if (!cfg.reorder && lossless_sym16_ok(cfg.huff_dict_size, cfg.huff_block_size)) {
      const int r16 = mgh_decompose_quantize_sym16(
          J.h, sub_in(id), local_eb, (double)local_tol, s_d, local_eb == MGH_REL ? 0.0 : (double)norm,
          nullptr /* the norm stays on the device: see below */, cfg.huff_dict_size, (uint16_t *)L.q.p,
          (uint64_t *)L.ocount.p, (uint64_t *)L.oidx.p, (int64_t *)L.oval.p, L.ocap, st);
      if (r16 == MGH_SUCCESS) J.sym16 = true;
      else if (r16 != MGH_ERR_UNSUPPORTED_DIMENSION) return r16;
    }
    if (!J.sym16)
      HL_TRY(mgh_decompose_quantize(J.h, sub_in(id), local_eb, (double)local_tol, s_d,
                                    local_eb == MGH_REL ? 0.0 : (double)norm,
                                    local_eb == MGH_REL ? &J.norm_out : nullptr, cfg.huff_dict_size, 1,
                                    (int64_t *)L.q.p, (uint64_t *)L.ocount.p, (uint64_t *)L.oidx.p,
                                    (int64_t *)L.oval.p, L.ocap, nullptr, st));
    hl_debug("compress: decompose + quantize done");
    compress_stats().decompositions++;
    compress_stats().quantize_passes++;
    compress_stats().histogram_launches++;
    // REL on the fused device path (the 16-bit symbol call: the norm never left the device): it
    // is fetched behind the quantizer into pinned memory and read when the lossless stage has
    // synchronised anyway -- a read-back inside the call above would stall the queue in front of
    // the histogram kernel. Every other path hands the norm back itself (norm_out).
    if (local_eb == MGH_REL && J.sym16) {
      J.norm_deferred = true;
      HL_HIP(hipMemcpyAsync((char *)L.pin.p + 16, mgh_norm_device_ptr(J.h), sizeof(T), hipMemcpyDeviceToHost, st));
    }
    const int64_t *q_enc = (const int64_t *)L.q.p;
    if (cfg.reorder) {
      // config.reorder == 1: the lossless stage sees the integers level by level, outlier
      // indices are positions in that array (LinearQuantization.hpp:226-232, 588-605)
      HL_TRY(mgh_level_linearize(J.h, (const int64_t *)L.q.p, (int64_t *)L.q2.p, 0, (uint64_t *)L.oidx.p,
                                 (const uint64_t *)L.ocount.p, 0, L.ocap, st));
      q_enc = (const int64_t *)L.q2.p;
    }
    J.lj = subdomain_job(L, cfg, q_enc, J.n, elem, J.sym16, /*bins_filled=*/false);
    return lossless_begin(L.ll, J.lj, st);
  };
  auto finish = [&](SubJob &J) -> int {
    Lane &L = g_cache.lane[J.lane];
    const uint64_t id = J.id, n = J.n;
    HL_TRY(encode_record(L, J.lj, sink, [&]() -> int {
      mgh_hierarchy *h = J.h;
      SubJob again;
      // (the hierarchy of the first attempt serves the second; issue() looks it up again)
      if (J.owned) {
        owned_alive.erase(std::remove(owned_alive.begin(), owned_alive.end(), h), owned_alive.end());
        mgh_hierarchy_destroy(h);
      }
      HL_TRY(issue(again, id));
      J = again;
      return MGH_SUCCESS;
    }));
    if (J.norm_deferred) {  // (lossless_finish has synchronised the lane)
      T nv;
      std::memcpy(&nv, (const char *)L.pin.p + 16, sizeof(T));
      norm = nv;
    } else if (local_eb == MGH_REL) {
      norm = (T)J.norm_out;
    }
    hl_debug("compress: lossless stage done");
    // the last record takes the header along, with the norm the pipeline computed for a non-decomposed REL run
    const bool last = id + 1 == dd.num;
    if (last) header_from(dd, dtype, ebtype, tol_d, s_d, ebtype == MGH_REL ? (double)norm : 0.0, cptr, cfg, hdr);
    HL_TRY(write_record(L, n, elem, sub_in(id), sink, last ? &hdr : nullptr, meta_size));
    if (J.owned) {
      owned_alive.erase(std::remove(owned_alive.begin(), owned_alive.end(), J.h), owned_alive.end());
      mgh_hierarchy_destroy(J.h);
    }
    return MGH_SUCCESS;
  };

  // Inputs: P = nbufs - 1 subdomains are fetched ahead of the one whose record is being written.
  // At the start of iteration id the buffer of subdomain id + P is the one subdomain id - 1 used,
  // and finish(id - 1) ended with a synchronisation of its lane.
  const uint64_t P = nbufs > 0 ? (uint64_t)(nbufs - 1) : 0;
  // One subdomain arriving from the host under a REL bound: its norm is reduced while it arrives
  // (stream_in_with_norm), so the decomposition starts when the last piece has landed instead of a whole
  // norm pass later; issue() waits for in_ready[0] and the fused call takes the norm from the hierarchy.
  bool first_fetched = false;
  if (dd.num == 1 && norm_streams_in(in_dev, ebtype)) {
    if ((rc = get_hierarchy(&pre_h, &pre_owned, dtype, dd.subdomain_shape(0), cptr, dd.subdomain_offset(0), cfg, 0)) !=
        MGH_SUCCESS)
      return cleanup(rc);
    if (pre_owned) owned_alive.push_back(pre_h);
    if (mgh_sym16_supported(pre_h)) {  // (= the fused path will run, which takes the streamed norm)
      if ((rc = stream_in_with_norm(pre_h, g_cache.in[0].p, original, total * elem, elem, s_d, g_cache.lane[0].st)) !=
          MGH_SUCCESS)
        return cleanup(rc);
      first_fetched = true;
    }
  }
  for (uint64_t id = first_fetched ? 1 : 0; id < std::max<uint64_t>(P, 1) && id < dd.num; id++)
    if ((rc = fetch_sub(id)) != MGH_SUCCESS) return cleanup(rc);
  SubJob jobs[kLanes];
  if ((rc = issue(jobs[0], 0)) != MGH_SUCCESS) return cleanup(rc);
  for (uint64_t id = 0; id < dd.num; id++) {
    if (P > 0 && id + P < dd.num && (rc = fetch_sub(id + P)) != MGH_SUCCESS) return cleanup(rc);
    if (nlanes > 1 && id + 1 < dd.num && (rc = issue(jobs[(id + 1) % nlanes], id + 1)) != MGH_SUCCESS)
      return cleanup(rc);
    if ((rc = finish(jobs[id % nlanes])) != MGH_SUCCESS) return cleanup(rc);
    if (nlanes == 1 && id + 1 < dd.num && (rc = issue(jobs[0], id + 1)) != MGH_SUCCESS) return cleanup(rc);
  }
  *compressed_size = sink.byte_offset;
  return cleanup(MGH_SUCCESS);
}

int decomposer_from_header(const fmt::Header &hd, const mgh_config &cfg, Decomposer &dd) {
  return hl_plan(mgh::decomposer_from_header(hd, cfg.domain_decomposition_sizes, cfg.num_domain_decomposition_sizes, dd));
}

// first bytes of a (host or device) stream on the host
int fetch_host(const void *data, size_t size, size_t want, std::vector<uint8_t> &out) {
  want = std::min(want, size);
  out.resize(want);
  if (is_device_pointer(data)) HL_TRY(dev_to_host(out.data(), data, want));
  else std::memcpy(out.data(), data, want);
  return MGH_SUCCESS;
}

int read_header(const void *data, size_t size, fmt::Header &hd, size_t &meta_size) {
  std::vector<uint8_t> pre;
  HL_TRY(fetch_host(data, size, fmt::kPreambleSize, pre));
  if (pre.size() < fmt::kPreambleSize) return hl_fail(MGH_ERR_FORMAT, "stream shorter than the preamble");
  uint64_t hs = 0;
  for (int i = 0; i < 8; i++) hs |= (uint64_t)pre[5 + i] << (8 * i);
  if (hs > size - fmt::kPreambleSize) return hl_fail(MGH_ERR_FORMAT, "header: truncated");
  std::vector<uint8_t> all;
  HL_TRY(fetch_host(data, size, fmt::kPreambleSize + hs, all));
  try {
    meta_size = fmt::parse_metadata(all.data(), all.size(), hd);
  } catch (const std::exception &e) {
    return hl_fail(MGH_ERR_FORMAT, e.what());
  }
  return MGH_SUCCESS;
}

// Level shapes of the array a container holds, from its header and the caller's configuration alone
// (max_larget_level is not recorded: INTEGRATION.md). level < 0: only l_target.
int header_level_shape(const fmt::Header &hd, const mgh_config &cfg, int level, int *l_target_out,
                       std::vector<uint64_t> *shape_out) {
  if (hd.shape.empty() || hd.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "header: dimension");
  if (hd.dd_method != fmt::DD_NOOP)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT,
                   "reconstruction at a coarser level: the container is domain-decomposed (every subdomain has its "
                   "own hierarchy and l_target); only containers with one subdomain are supported");
  for (uint64_t e : hd.shape)
    if (e < 3) return hl_fail(MGH_ERR_FORMAT, "header: extent below 3");
  const int L = mgh::hierarchy_l_target(hd.shape.size(), hd.shape.data(), cfg.max_larget_level);
  if (l_target_out) *l_target_out = L;
  if (level < 0 && !shape_out) return MGH_SUCCESS;
  if (level < 0 || level > L) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "level outside 0 .. l_target");
  if (shape_out) {
    shape_out->assign(hd.shape.begin(), hd.shape.end());
    for (uint64_t &e : *shape_out)
      for (int k = 0; k < L - level; k++) e = e / 2 + 1;
  }
  return MGH_SUCCESS;
}

// ---- what the decoders (mgh_decompress*, mgh_progressive_*) share ------------------------------------
// One subdomain record inside a container.
struct RecordView {
  int lossless = MGH_LOSSLESS_HUFFMAN;  // the header's compressor as a lossless mode
  const uint8_t *rec = nullptr;         // the record, behind its 8-byte size prefix (borrowed from the container)
  uint64_t csize = 0;
  bool raw = false;                     // it holds the data itself (the lossless stage did not pay)
};
// ... its part from the header: refuses the containers no decoder here reads
int record_view_header(const fmt::Header &hd, RecordView &rv) {
  if (hd.compressor == fmt::COMP_X_HUFFMAN) rv.lossless = MGH_LOSSLESS_HUFFMAN;
  else if (hd.compressor == fmt::COMP_X_HUFFMAN_ZSTD) rv.lossless = MGH_LOSSLESS_HUFFMAN_ZSTD;
  else return hl_fail(MGH_ERR_FORMAT, "this lossless compressor is not supported");
  if (hd.hierarchy != fmt::HIER_MULTIDIM) return hl_fail(MGH_ERR_FORMAT, "only the multi-dimensional decomposition is supported");
  return MGH_SUCCESS;
}
// ... and the record whose size prefix is at byte `at` of the container; data_bytes: the subdomain as data
int record_view_at(const void *container, size_t size, size_t at, uint64_t data_bytes, RecordView &rv) {
  if (size - at < 8) return hl_fail(MGH_ERR_FORMAT, "subdomain record truncated");
  std::vector<uint8_t> sz;
  HL_TRY(fetch_host((const char *)container + at, 8, 8, sz));
  std::memcpy(&rv.csize, sz.data(), 8);
  if (rv.csize > size - at - 8) return hl_fail(MGH_ERR_FORMAT, "subdomain record truncated");
  rv.rec = (const uint8_t *)container + at + 8;
  rv.raw = !((double)data_bytes / (double)rv.csize > 1.0);  // GPUPipelines.hpp:414-417
  if (rv.raw && rv.csize != data_bytes) return hl_fail(MGH_ERR_FORMAT, "raw subdomain record has the wrong size");
  return MGH_SUCCESS;
}

// Where the `num` records of a (host or device) container lie behind its header of meta_size bytes: the
// offset of every size prefix and the length of its frame, prefix included.
int record_table(const void *container, size_t size, size_t meta_size, uint64_t num, std::vector<size_t> &off,
                 std::vector<size_t> &len) {
  off.assign(num, 0);
  len.assign(num, 0);
  size_t at = meta_size;
  std::vector<uint8_t> sz;
  for (uint64_t id = 0; id < num; id++) {
    if (const char *bad = frame_prefix(size, at)) return hl_fail(MGH_ERR_FORMAT, bad);
    uint64_t cs = 0;
    HL_TRY(fetch_host((const char *)container + at, 8, 8, sz));
    std::memcpy(&cs, sz.data(), 8);
    off[id] = at;
    if (const char *bad = frame_next(size, at, cs, &at)) return hl_fail(MGH_ERR_FORMAT, bad);
    len[id] = at - off[id];
  }
  return MGH_SUCCESS;
}

// The coordinates a decoder builds its hierarchies from (get_hierarchy converts them to the data
// type); nullptr: a uniform grid.
// The reference rebuilds the coordinates of a non-uniform grid through `(float)` when it
// decompresses, for double data as well (CompressionHighLevel.hpp:455-462). Mirrored on request
// only: with it an f64 non-uniform stream reconstructs exactly like stock MGARD-X does, without
// it the coordinates the compressor used are taken at full precision.
const std::vector<std::vector<double>> *decoder_coords(const fmt::Header &hd, const mgh_config &cfg,
                                                       std::vector<std::vector<double>> &mirrored) {
  if (hd.uniform) return nullptr;
  if (!cfg.mirror_reference_coord_cast) return &hd.coords;
  mirrored = hd.coords;
  for (auto &c : mirrored)
    for (double &x : c) x = (double)(float)x;
  return &mirrored;
}

// The quantization a record was made with (the header's, per subdomain), in the data type's precision.
struct RecordQuant {
  int eb;
  double tol, s, norm;
  uint64_t dict;
  bool reorder;
};

// A record that holds the data itself, below l_target: a coarser level is what a Huffman record of
// this subdomain would have given -- the integers of the header's bound, made here (no dictionary:
// prep_huffman = 0) into q, through `data`.
int raw_record_integers(mgh_hierarchy *h, const RecordView &rv, const RecordQuant &qp, DevBuf &data, DevBuf &q,
                        uint64_t n, hipStream_t st) {
  HL_TRY(q.ensure(n * 8));
  HL_TRY(data.ensure(rv.csize));
  HL_TRY(copy_any(data.p, rv.rec, rv.csize, st));
  return mgh_decompose_quantize(h, data.p, qp.eb, qp.tol, qp.s, qp.norm, nullptr, qp.dict, 0, (int64_t *)q.p, nullptr,
                                nullptr, nullptr, 0, nullptr, st);
}

// A Huffman record of n integers to the dense subdomain at `dst`, queued on st: the whole array
// (level < 0), the dense array of `level`, or -- linear_head -- that array from the first n_head
// integers of a reorder = 1 record alone (q holds q_cap).
int reconstruct_record(mgh_hierarchy *h, mgh_lossless_ctx *ll, DevBuf &q, DevBuf &q2, const RecordQuant &qp,
                       const RecordView &rv, uint64_t n, int level, bool linear_head, uint64_t n_head, uint64_t q_cap,
                       void *dst, hipStream_t st) {
  uint64_t ocount = 0;
  // 16-bit symbols between decoder and dequantizer (a quarter of the bytes the decoder writes and
  // the two passes over the finest level read). The symbol width is chosen PER LEVEL inside
  // mgh_dequantize_recompose_sym16: the finest level reads the symbols, the levels below --
  // where the out-of-dictionary values live -- an int64 copy of the coarse corner box.
  // Subdomains below 2^25 elements keep int64: the box copy and the outlier table are three more
  // launches in a latency-bound chain (256^3: 0.86 ms with int64, 0.89 ms with symbols; 512^3: 2.16
  // vs 2.03 ms). MGH_SYM16_DECODE=0 / 1: never / always (cross-checks).
  static const long sym16_env = env_get("MGH_SYM16_DECODE", -1);
  const bool sym16_decode = sym16_env < 0 ? n >= ((uint64_t)1 << 25) : sym16_env != 0;
  bool sym16 = sym16_decode && !qp.reorder && mgh_sym16_supported(h) && qp.dict <= 65536;
  int64_t *src = (int64_t *)q.p;
  if (linear_head) {
    if (level >= mgh_l_target(h)) return hl_fail(MGH_ERR_FORMAT, "header: the hierarchy of the subdomain is not the header's");
    HL_TRY(lossless_decompress(ll, rv.rec, rv.csize, rv.lossless, src, n, &ocount, st, nullptr, /*sync_end=*/false,
                               DecodeRange{/*n_prefix=*/n_head, q_cap}));
    return mgh_dequantize_recompose_linear_to_level(h, src, qp.eb, qp.tol, qp.s, qp.norm, qp.dict, 1,
                                                    (const uint64_t *)ll->oidx.p, (const int64_t *)ll->oval.p, ocount,
                                                    level, dst, st);
  }
  HL_TRY(lossless_decompress(ll, rv.rec, rv.csize, rv.lossless, src, n, &ocount, st, &sym16, /*sync_end=*/false));
  const uint64_t *oidx = (const uint64_t *)ll->oidx.p;
  const int64_t *oval = (const int64_t *)ll->oval.p;
  if (sym16 && level >= 0)
    return mgh_dequantize_recompose_sym16_to_level(h, (const uint16_t *)q.p, qp.eb, qp.tol, qp.s, qp.norm, qp.dict, oidx,
                                                   oval, ocount, level, dst, st);
  if (sym16)
    return mgh_dequantize_recompose_sym16(h, (const uint16_t *)q.p, qp.eb, qp.tol, qp.s, qp.norm, qp.dict, oidx, oval,
                                          ocount, dst, st);
  if (qp.reorder) {
    // level-linearised integers: outliers back at their linearised positions, the
    // permutation undone, then the ordinary path with nothing left to restore
    HL_TRY(mgh_outlier_restore(src, n, oidx, oval, ocount, st));
    HL_TRY(mgh_level_linearize(h, src, (int64_t *)q2.p, 1, nullptr, nullptr, 0, 0, st));
    src = (int64_t *)q2.p;
    oidx = nullptr;
    oval = nullptr;
    ocount = 0;
  }
  if (level >= 0)
    return mgh_dequantize_recompose_to_level(h, src, qp.eb, qp.tol, qp.s, qp.norm, qp.dict, 1, oidx, oval, ocount, level,
                                             dst, st);
  return mgh_dequantize_recompose(h, src, qp.eb, qp.tol, qp.s, qp.norm, qp.dict, 1, oidx, oval, ocount, dst, st);
}

// What one subdomain becomes in the output: the level it is reconstructed at (-1: the whole
// subdomain) and the box its dense array fills in the output array.
struct SubdomainPlan {
  int level = -1;
  std::vector<uint64_t> ext, off;
  uint64_t n = 0, n_out = 0;  // elements of the subdomain and of its box
  bool linear_head = false;   // the level is made from the head of a reorder = 1 record alone
  // full-grid preview: the level's dense array (n_level elements) is prolonged inside the subdomain's
  // own hierarchy (mgh_prolong) to the whole subdomain, which is what fills the box
  bool prolong = false;
  uint64_t n_level = 0;
  // windowed preview: the subdomain does not meet the window and is not opened; else `wlo` is where
  // the window's part begins inside the subdomain (ext / off: that part and its place in the window)
  bool skip = false;
  std::vector<uint64_t> wlo;
};

// The box [lo, lo + ext) of the array a windowed preview writes (mgh_decompress_preview_window).
struct Window {
  std::vector<uint64_t> lo, ext;
};

// mgh_verify: the array every reconstructed subdomain is compared with instead of being written out,
// and the statistics of the whole array when the call is through.
struct VerifyJob {
  const void *original = nullptr;
  // mgh_verify_masked: the packed mask of the whole array on the device; a set position takes part in nothing
  const uint64_t *d_words = nullptr;
  mgh_error_stats stats{};
  bool rel = false;  // the bound of the header
  double tol = 0, s = 0, norm = 0;
};

// level >= 0: mgh_decompress_level -- the output is the dense array of that level of the hierarchy.
// halvings > 0: mgh_decompress_coarsened -- every subdomain at its level l_target_i - halvings, stitched.
// ... and preview: mgh_decompress_preview -- every subdomain at that level, prolonged to its full shape and
// placed where mgh_decompress places it; nothing is interpolated across subdomain borders.
// ... and win: mgh_decompress_preview_window -- the output is the window alone; only the subdomains that
// meet it are opened, each reconstructed as for the preview and its part of the window written by
// mgh_prolong_window of its own hierarchy (halvings = 0: the box copy of its finest level).
// vfy: mgh_verify -- there is no output (prealloc, *out == NULL): where finish() would copy the dense
// subdomain into its box of the output, it is compared with that box of vfy->original instead.
template <typename T>
int decompress_impl(const fmt::Header &hd, size_t meta_size, const void *compressed, size_t csize_total,
                    void **out, const mgh_config &cfg_in, bool prealloc, int level = -1, int halvings = -1,
                    bool preview = false, const Window *win = nullptr, VerifyJob *vfy = nullptr) {
  mgh_config cfg = cfg_in;
  const int dtype = hd.is_double ? MGH_DOUBLE : MGH_FLOAT;
  const size_t elem = sizeof(T);
  std::vector<uint64_t> dshape = hd.shape;  // of the output array
  int l_target = 0;
  // (refuses a decomposed container and a level outside the hierarchy)
  if (level >= 0) HL_TRY(header_level_shape(hd, cfg, level, &l_target, &dshape));
  Decomposer dd;
  HL_TRY(decomposer_from_header(hd, cfg, dd));
  if (const char *bad = check_extents(dd)) return hl_fail(MGH_ERR_FORMAT, bad);
  std::vector<SubdomainPlan> plan(dd.num);
  if (level >= 0) {
    plan[0].level = level;
    plan[0].ext = dshape;
    plan[0].off.assign(dshape.size(), 0);
    plan[0].linear_head = hd.reorder && level < l_target;
  } else if (halvings >= 0) {  // (refuses more halvings than the shallowest subdomain has levels)
    StitchedLayout sl;
    HL_TRY(hl_plan(stitched_layout(dd, cfg.max_larget_level, halvings, sl)));
    if (halvings > 0) {
      if (!preview) dshape = sl.shape;
      for (uint64_t id = 0; id < dd.num; id++) {
        const auto sid = dd.dim_subdomain_id(id), sshape = dd.subdomain_shape(id);
        SubdomainPlan &P = plan[id];
        P.level = mgh::hierarchy_l_target(sshape.size(), sshape.data(), cfg.max_larget_level) - halvings;
        P.n_level = 1;
        for (int d = 0; d < dd.D; d++) P.n_level *= sl.ext[d][sid[d]];
        if (preview) {
          P.prolong = true;
          P.ext = sshape;
          P.off = dd.subdomain_offset(id);
        } else {
          for (int d = 0; d < dd.D; d++) {
            P.ext.push_back(sl.ext[d][sid[d]]);
            P.off.push_back(sl.off[d][sid[d]]);
          }
        }
        P.linear_head = hd.reorder != 0;  // (level < l_target)
      }
    }
  }
  std::vector<uint64_t> order;  // the subdomains the call opens, ascending
  if (win) {
    dshape = win->ext;
    for (uint64_t id = 0; id < dd.num; id++) {
      SubdomainPlan &P = plan[id];
      const auto soff = dd.subdomain_offset(id), sshape = dd.subdomain_shape(id);
      std::vector<uint64_t> wext(dd.D), woff(dd.D);
      P.wlo.resize(dd.D);
      for (int d = 0; d < dd.D && !P.skip; d++) {
        const uint64_t a = std::max(win->lo[d], soff[d]), b = std::min(win->lo[d] + win->ext[d], soff[d] + sshape[d]);
        P.skip = a >= b;
        if (P.skip) break;
        P.wlo[d] = a - soff[d];
        wext[d] = b - a;
        woff[d] = a - win->lo[d];
      }
      if (P.skip) continue;
      if (!P.prolong) {  // (halvings = 0: the finest level, whole, is what the window is cut from)
        P.prolong = true;
        P.n_level = 1;
        for (uint64_t e : sshape) P.n_level *= e;
      }
      P.ext = wext;
      P.off = woff;
    }
  }
  for (uint64_t id = 0; id < dd.num; id++)
    if (!plan[id].skip) order.push_back(id);
  if (order.empty()) return hl_fail(MGH_ERR_FORMAT, "header: no subdomain under the window");
  size_t total = 1;
  for (uint64_t e : dshape) total *= e;
  uint64_t sub_elems = 0, q_elems = 0, q2_elems = 0;  // what a lane's buffers hold: the maxima over the subdomains
  uint64_t lvl_elems = 0;
  bool all_slabs = true;  // every box spans every dimension but the slowest: a contiguous run of the output
  const uint64_t hblock = std::max<uint64_t>(hd.huff_block_size, 1);
  for (uint64_t id = 0; id < dd.num; id++) {
    SubdomainPlan &P = plan[id];
    if (P.skip) continue;
    if (P.level < 0 && !win) {
      P.ext = dd.subdomain_shape(id);
      P.off = dd.subdomain_offset(id);
    }
    P.n = P.n_out = 1;
    for (uint64_t e : dd.subdomain_shape(id)) P.n *= e;
    for (uint64_t e : P.ext) P.n_out *= e;
    for (int d = 1; d < dd.D; d++) all_slabs = all_slabs && P.ext[d] == dshape[d];
    sub_elems = std::max(sub_elems, P.n_out);
    if (!P.prolong) P.n_level = P.n_out;  // (the box IS the level's array)
    else lvl_elems = std::max(lvl_elems, P.n_level);
    // A level below l_target of a level-linearised (reorder = 1) record: its first n_level integers are
    // the box of the level -- only the chunks that hold them are decoded, and the level is made from
    // that head; nothing on the way is sized by the subdomain.
    q_elems = std::max(q_elems, P.linear_head ? std::min<uint64_t>(P.n, ((P.n_level - 1) / hblock + 1) * hblock) : P.n);
    if (hd.reorder && !P.linear_head) q2_elems = std::max(q2_elems, P.n);
  }
  HL_TRY(cache_prepare(cfg.dev_id));
  HL_TRY(trim_hierarchy_cache());
  RecordView rv_hd;
  HL_TRY(record_view_header(hd, rv_hd));
  const bool in_dev = is_device_pointer(compressed);
  Pretouch pretouch;  // (joined before the first byte of the output is written, and on every way out)
  const OutSlot slot{out, in_dev, prealloc};
  HL_TRY(slot.alloc(total * elem));
  // fresh host pages: faulted in beside the decoder instead of inside the device -> host copy
  if (!prealloc && !in_dev) pretouch.start(*out, total * elem);
  // auto_pin_host_buffers (CompressionHighLevel.hpp:470-497): stream and output registered for the call
  bool in_pinned_here = false, out_pinned_here = false;
  if (cfg.auto_pin_host_buffers) {
    if (!in_dev && !is_registered_host(compressed)) {
      if (hipHostRegister(const_cast<void *>(compressed), csize_total, hipHostRegisterDefault) == hipSuccess) in_pinned_here = true;
      else (void)hipGetLastError();
    }
    if (!vfy && !is_device_pointer(*out) && !is_registered_host(*out)) {
      pretouch.join();
      if (hipHostRegister(*out, total * elem, hipHostRegisterDefault) == hipSuccess) out_pinned_here = true;
      else (void)hipGetLastError();
    }
  }
  const bool pipelined = env_get("MGH_HL_PIPELINE", 1) != 0;
  const int nlanes = order.size() > 1 && pipelined ? kLanes : 1;
  mgh_hierarchy *owned_h[kLanes] = {nullptr, nullptr};  // per-subdomain hierarchy (non-uniform grid) of the lane's last job
  auto cleanup = [&](int rc) {
    for (int l = 0; l < kLanes; l++) {
      if (rc != MGH_SUCCESS || owned_h[l]) (void)hipStreamSynchronize(g_cache.lane[l].st);
      if (owned_h[l]) mgh_hierarchy_destroy(owned_h[l]);
      owned_h[l] = nullptr;
    }
    pretouch.join();
    if (in_pinned_here) (void)hipHostUnregister(const_cast<void *>(compressed));
    if (out_pinned_here) (void)hipHostUnregister(*out);
    return slot.fail(rc);
  };
  const uint64_t max_elems = dd.max_subdomain_elems();
  int rc;
  // device-resident output whose subdomains are contiguous slabs: reconstruct them in place
  const bool zero_copy = !win && !vfy && is_device_pointer(*out) && all_slabs;
  // windowed preview into device memory: the window kernel writes the box of the output itself
  const bool direct = win && is_device_pointer(*out);
  const bool vfy_in_place = vfy && is_device_pointer_on(vfy->original, cfg.dev_id);  // (the original is read where it lies)
  uint64_t slab_inner = 1;  // elements of one plane of the slowest dimension of the output
  for (size_t d = 1; d < dshape.size(); d++) slab_inner *= dshape[d];
  auto ensure_all = [&]() -> int {
    for (int l = 0; l < nlanes; l++) {
      Lane &L = g_cache.lane[l];
      if (!zero_copy && !direct) HL_TRY(L.sub.ensure(sub_elems * elem));
      if (lvl_elems) HL_TRY(L.lvl.ensure(lvl_elems * elem));
      HL_TRY(L.q.ensure(q_elems * 8));
      if (q2_elems) HL_TRY(L.q2.ensure(q2_elems * 8));
      if (vfy) HL_TRY(L.cmp.ensure(mgh_compare_scratch_bytes_()));
      if (vfy && !vfy_in_place) HL_TRY(L.orig.ensure(sub_elems * elem));
    }
    if (vfy) HL_TRY(g_cache.vres.ensure(order.size() * sizeof(mgh_error_stats)));
    return MGH_SUCCESS;
  };
  if ((rc = ensure_all()) != MGH_SUCCESS) return cleanup(rc);
  const T tol = (T)hd.tol, s = (T)hd.s, norm = (T)hd.norm;
  T local_tol = tol;
  int local_eb = hd.rel ? MGH_REL : MGH_ABS;
  if (dd.decomposed) {  // CompressionHighLevel.hpp:513-522
    local_tol = local_abs_tol<T>(local_eb, norm, tol, s, dd.num);
    local_eb = MGH_ABS;
  }
  const RecordQuant qp{local_eb, (double)local_tol, (double)s, (double)norm, hd.huff_dict_size, hd.reorder};
  std::vector<std::vector<double>> mirrored;
  const std::vector<std::vector<double>> *cptr = decoder_coords(hd, cfg, mirrored);
  // ---- subdomain pipeline (decompress_pipeline_gpu, GPUPipelines.hpp:330-520) ----
  // issue(k): everything of subdomain k up to the reconstructed dense subdomain, queued on lane
  // k % nlanes without a host synchronisation (the decoder of k + 1 runs beside the recomposition
  // of k); finish(k): the dense subdomain into its box of the output when it was not reconstructed
  // in place (for a pageable host output that copy occupies the host).
  size_t byte_offset = meta_size;
  uint64_t next_id = 0;  // the subdomain whose record begins at byte_offset
  auto issue = [&](uint64_t k) -> int {
    const uint64_t id = order[k];
    const int lane = (int)(k % nlanes);
    Lane &L = g_cache.lane[lane];
    hipStream_t st = L.st;
    for (; next_id < id; next_id++) {  // (records the window does not meet: their size prefix is all that is read)
      RecordView skipped = rv_hd;
      uint64_t sn = 1;
      for (uint64_t e : dd.subdomain_shape(next_id)) sn *= e;
      HL_TRY(record_view_at(compressed, csize_total, byte_offset, sn * elem, skipped));
      byte_offset += 8 + skipped.csize;
    }
    next_id = id + 1;
    // what the lane's previous subdomain read from the host (decode tables, record head) and its
    // hierarchy are free again once the lane has drained
    HL_HIP(hipStreamSynchronize(st));
    HL_TRY(lossless_tag_check(L.ll));
    if (owned_h[lane]) mgh_hierarchy_destroy(owned_h[lane]);
    owned_h[lane] = nullptr;
    if (in_dev && csize_total - byte_offset >= 8) {
      // ONE device -> host read per subdomain: the size prefix and what the lossless stage will want
      // of the record's head (chunk table for the largest subdomain, decodebook) -- every further
      // read of this subdomain is served from it (dev_to_host). A read is a queued copy plus a
      // synchronisation, ~25 us: three per subdomain were more than the decoder of a 65^3 block.
      HostPrefixState &hp = host_prefix();
      const uint8_t *at = (const uint8_t *)compressed + byte_offset;
      const bool covered = hp.base && at >= hp.base && (size_t)(at - hp.base) + 8 <= hp.bytes.size();
      if (!covered) {
        const size_t want = std::min<size_t>(csize_total - byte_offset,
                                             8 + 24 + 16 * ((max_elems - 1) / std::max<uint64_t>(hd.huff_block_size, 1) + 1) +
                                                 16 + 8 * 128 + 8 * (size_t)hd.huff_dict_size + 16);
        hp.base = nullptr;
        hp.bytes.resize(want);
        HL_TRY(aux_read(hp.bytes.data(), at, want));
        hp.base = at;
      }
    }
    const auto sshape = dd.subdomain_shape(id);
    const SubdomainPlan &P = plan[id];
    const uint64_t n = P.n;
    const int level = P.level;
    RecordView rv = rv_hd;
    HL_TRY(record_view_at(compressed, csize_total, byte_offset, n * elem, rv));
    byte_offset += 8 + rv.csize;
    void *sub = zero_copy ? (void *)((char *)*out + P.off[0] * slab_inner * elem) : L.sub.p;
    decompress_stats().subdomains++;
    if (rv.raw) {
      decompress_stats().record_bytes += rv.csize;
      if (level < 0 && !win) return copy_any(sub, rv.rec, rv.csize, st);
    }
    mgh_hierarchy *h = nullptr;
    bool owned = false;
    HL_TRY(get_hierarchy(&h, &owned, dtype, sshape, cptr, dd.subdomain_offset(id), cfg, lane));
    if (owned) owned_h[lane] = h;
    if (level >= 0 && level > mgh_l_target(h)) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "level outside 0 .. l_target");
    if (halvings > 0 && level != mgh_l_target(h) - halvings)
      return hl_fail(MGH_ERR_FORMAT, "header: the hierarchy of the subdomain is not the header's");
    // (full-grid preview: the level into the lane's own buffer, then prolonged to the dense subdomain)
    void *made = P.prolong ? L.lvl.p : sub;
    if (rv.raw && win && level < 0) {  // (the data, whole: the window is cut from it below)
      HL_TRY(copy_any(made, rv.rec, rv.csize, st));
    } else if (rv.raw) {  // (the finest level is the data)
      if (level == mgh_l_target(h)) return copy_any(sub, rv.rec, rv.csize, st);
      // (q: the head of a reorder = 1 record is all the lane holds otherwise)
      HL_TRY(raw_record_integers(h, rv, qp, L.q2, L.q, n, st));
      HL_TRY(mgh_dequantize_recompose_to_level(h, (int64_t *)L.q.p, qp.eb, qp.tol, qp.s, qp.norm, qp.dict, 0, nullptr,
                                               nullptr, 0, level, made, st));
    } else {
      HL_TRY(reconstruct_record(h, L.ll, L.q, L.q2, qp, rv, n, level, P.linear_head, P.n_level, q_elems, made, st));
    }
    if (!P.prolong) return MGH_SUCCESS;
    if (!win) return mgh_prolong(h, level, made, sub, st);
    // the subdomain's part of the window: into its box of a device-resident output through that
    // array's strides, else dense into the lane's buffer (finish copies it out)
    uint64_t str[MGH_MAX_DIM];
    const std::vector<uint64_t> &into = direct ? dshape : P.ext;
    uint64_t run = 1, at = 0;
    for (int d = dd.D - 1; d >= 0; d--) {
      str[d] = run;
      run *= into[d];
      if (direct) at += P.off[d] * str[d];
    }
    return mgh_prolong_window_strided(h, level < 0 ? mgh_l_target(h) : level, made, P.wlo.data(), P.ext.data(),
                                      direct ? (void *)((char *)*out + at * elem) : L.sub.p, str, st);
  };
  auto finish = [&](uint64_t k) -> int {
    if (zero_copy || direct) return MGH_SUCCESS;
    pretouch.join();
    Lane &L = g_cache.lane[k % nlanes];
    if (vfy) {
      const SubdomainPlan &P = plan[order[k]];
      const void *a = L.orig.p;
      // the box through its offset and the strides of the array: the original where it lies, and the mask
      uint64_t astr[MGH_MAX_DIM], run = 1, at = 0;
      for (int d = dd.D - 1; d >= 0; d--) {
        astr[d] = run;
        at += P.off[d] * run;
        run *= dshape[d];
      }
      if (vfy_in_place) a = (const char *)vfy->original + at * elem;
      else HL_TRY(copy_box(P.ext, P.off, dshape, elem, L.orig.p, vfy->original, nullptr, true, L.st));
      if (vfy->d_words)
        HL_TRY(mgh_compare_masked_device_(dd.D, dtype, P.ext.data(), a, vfy_in_place ? astr : nullptr, L.sub.p, nullptr,
                                          vfy->d_words, astr, at, L.cmp.p, L.st));
      else
        HL_TRY(mgh_compare_device_(dd.D, dtype, P.ext.data(), a, vfy_in_place ? astr : nullptr, L.sub.p, nullptr, L.cmp.p,
                                   L.st));
      HL_HIP(hipMemcpyAsync((char *)g_cache.vres.p + k * sizeof(mgh_error_stats), L.cmp.p, sizeof(mgh_error_stats),
                            hipMemcpyDeviceToDevice, L.st));
      return MGH_SUCCESS;
    }
    return copy_box(plan[order[k]].ext, plan[order[k]].off, dshape, elem, L.sub.p, nullptr, *out, false, L.st);
  };
  if ((rc = issue(0)) != MGH_SUCCESS) return cleanup(rc);
  for (uint64_t k = 0; k < order.size(); k++) {
    if (nlanes > 1 && k + 1 < order.size() && (rc = issue(k + 1)) != MGH_SUCCESS) return cleanup(rc);
    if ((rc = finish(k)) != MGH_SUCCESS) return cleanup(rc);
    if (nlanes == 1 && k + 1 < order.size() && (rc = issue(k + 1)) != MGH_SUCCESS) return cleanup(rc);
  }
  for (int l = 0; l < nlanes; l++) {
    if (hipStreamSynchronize(g_cache.lane[l].st) != hipSuccess) return cleanup(hl_fail(MGH_ERR_DEVICE, "sync"));
    if ((rc = lossless_tag_check(g_cache.lane[l].ll)) != MGH_SUCCESS) return cleanup(rc);
  }
  if (vfy) {
    // the subdomains' results, in subdomain order; a box's argmax becomes the index in the whole array
    std::vector<mgh_error_stats> parts(order.size());
    if (hipMemcpy(parts.data(), g_cache.vres.p, parts.size() * sizeof(mgh_error_stats), hipMemcpyDeviceToHost) != hipSuccess)
      return cleanup(hl_fail(MGH_ERR_DEVICE, "mgh_verify: reading the results back"));
    vfy->stats = mgh_error_stats{};
    for (uint64_t k = 0; k < order.size(); k++) {
      const SubdomainPlan &P = plan[order[k]];
      mgh_error_stats part = parts[k];
      uint64_t rest = part.argmax, run = 1, at = 0;
      for (int d = dd.D - 1; d >= 0; d--) {
        at += (P.off[d] + rest % P.ext[d]) * run;
        rest /= P.ext[d];
        run *= dshape[d];
      }
      part.argmax = mgh::compare_finite(part) ? at : 0;
      mgh::merge(vfy->stats, part, 0);
    }
  }
  return cleanup(MGH_SUCCESS);
}

int check_config(const mgh_config *cfg) {
  if (!cfg) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "config is NULL (use mgh_config_default)");
  if (cfg->lossless != MGH_LOSSLESS_HUFFMAN && cfg->lossless != MGH_LOSSLESS_HUFFMAN_ZSTD)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless: only Huffman and Huffman_Zstd are supported");
  if (cfg->huff_dict_size < 2 || cfg->huff_dict_size > 16384 || cfg->huff_block_size == 0)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "huff_dict_size (2..16384) / huff_block_size");
  if (cfg->reorder != 0 && cfg->reorder != 1) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "reorder must be 0 or 1");
  int ndev = mgh_device_count();
  if (ndev <= 0) return hl_fail(MGH_ERR_NO_DEVICE, "no HIP device");
  if (cfg->dev_id < 0 || cfg->dev_id >= ndev) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "dev_id");
  return MGH_SUCCESS;
}

// What every entry that takes an array checks, in this order. `given`: the caller's pre-allocated output.
int size_call_args(int D, int dtype, const uint64_t *shape, int ebtype, const void *original, const mgh_config *config,
                   void *const *given = nullptr) {
  if (!shape || !original) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (D < 1 || D > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "D must be 1..5");
  if (dtype != MGH_FLOAT && dtype != MGH_DOUBLE) return hl_fail(MGH_ERR_UNSUPPORTED_DTYPE, "dtype");
  if (ebtype != MGH_REL && ebtype != MGH_ABS) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "error_bound_type");
  if (given && !*given) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  const std::string bad = env_validate();  // MGH_* developer switches: a typo is an error
  if (!bad.empty()) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad);
  HL_TRY(check_config(config));
  if (hipSetDevice(config->dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return MGH_SUCCESS;
}

// The K tolerances and K output slots of mgh_compress_ladder / _layers (`who` starts the refusals).
int tolerance_list_args(const char *who, int ntol, const double *tols, void *const *slots, bool prealloc,
                        bool strictly_decreasing) {
  const std::string w(who);
  if (ntol < 1 || ntol > kLadderMaxTols) return hl_fail(MGH_ERR_INVALID_ARGUMENT, w + "ntol must be in 1..64");
  for (int k = 0; k < ntol; k++) {
    if (!(tols[k] > 0) || !std::isfinite(tols[k]))
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, w + "every tolerance must be positive and finite");
    if (strictly_decreasing && k > 0 && !(tols[k] < tols[k - 1]))
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, w + "the tolerances must be strictly decreasing");
    if (prealloc && !slots[k]) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  }
  return MGH_SUCCESS;
}

// The session below keeps one array's coefficients: a configuration that decomposes the domain is refused.
int one_subdomain_only(const char *who, const Decomposer &dd) {
  if (dd.decomposed || dd.num != 1)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT,
                   std::string(who) + "the configuration decomposes the domain (containers of one subdomain only)");
  return MGH_SUCCESS;
}

// ---- sizes from histograms: mgh_estimate_sizes, mgh_compress_budget (size_plan.hpp) ---------------
// ---- errors from round trips: mgh_achieved_errors, mgh_compress_target (target_plan.hpp) ----------
// ---- containers from them: mgh_compress_ladder, mgh_compress_layers, the last step of budget and target
// The session of one array: decomposed once (begin), its coefficients kept on the device (lane 0's
// integer buffer, free between calls) while tolerances are priced against them (price), their
// reconstructions compared with the input (achieved), and containers written from them (write).
struct CoefficientSession {
  int D = 0, dtype = 0, ebtype = 0;
  std::vector<uint64_t> shape_v;
  const void *d_in = nullptr;  // the input on the device: the caller's array, or its upload
  bool in_dev = false;         // the caller's array is device memory (so is every output the call allocates)
  double s = 0, norm = 1;
  uint64_t n = 0;
  size_t elem = 0;
  mgh_config cfg{};
  Decomposer dd;
  std::vector<std::vector<double>> coords;
  const std::vector<std::vector<double>> *cptr = nullptr;
  mgh_hierarchy *h = nullptr;
  bool owned = false;
  std::vector<uint32_t> freq;
  std::vector<uint64_t> outl;
  huff::Codebook cb;
  bool res_in_q3 = false;  // write(layer): the coefficients the next layer reads are in lane 0's q3, not its q
  ~CoefficientSession() {
    if (h && owned) mgh_hierarchy_destroy(h);
  }

  int fail_drained(int rc) {
    (void)hipStreamSynchronize(g_cache.lane[0].st);
    (void)hipStreamSynchronize(g_cache.copy_st);
    return rc;
  }

  // an output of this array's calls: in the input's memory space
  OutSlot out_slot(void **slot, bool prealloc) const { return OutSlot{slot, in_dev, prealloc}; }

  // Upload (host input), norm of a REL bound with the reduction compress_impl uses, decomposition. `who`
  // starts the refusals ("size estimates: "). huffman_only: the call prices -- a size is a function of the
  // histogram under Huffman alone; an achieved error does not depend on the lossless stage at all, and
  // a written container takes either.
  int begin(const char *who, bool huffman_only, int D_, int dtype_, const uint64_t *shape, double s_, int ebtype_,
            const void *original, const void *const *coords_in, const mgh_config &cfg_) {
    D = D_, dtype = dtype_, ebtype = ebtype_, s = s_, cfg = cfg_;
    elem = dtype == MGH_FLOAT ? 4 : 8;
    shape_v.assign(shape, shape + D);
    if (huffman_only && cfg.lossless != MGH_LOSSLESS_HUFFMAN)
      return hl_fail(MGH_ERR_INVALID_ARGUMENT,
                     std::string(who) + "lossless must be Huffman (a Zstd frame's size is no function of the histogram)");
    HL_TRY(cache_prepare(cfg.dev_id));
    HL_TRY(trim_hierarchy_cache());
    HL_TRY(make_decomposer(dd, D, shape, elem, cfg));
    HL_TRY(one_subdomain_only(who, dd));
    n = 1;
    for (int d = 0; d < D; d++) n *= shape[d];
    if (coords_in) {
      coords.resize(D);
      for (int d = 0; d < D; d++) {
        if (dtype == MGH_FLOAT) coords[d].assign((const float *)coords_in[d], (const float *)coords_in[d] + shape[d]);
        else coords[d].assign((const double *)coords_in[d], (const double *)coords_in[d] + shape[d]);
      }
      cptr = &coords;
    }
    HL_TRY(get_hierarchy(&h, &owned, dtype, dd.subdomain_shape(0), cptr, dd.subdomain_offset(0), cfg, 0));
    Lane &L = g_cache.lane[0];
    hipStream_t st = L.st;
    const size_t bytes = n * elem;
    d_in = original;
    in_dev = is_device_pointer(original);
    bool have_norm = ebtype != MGH_REL;
    if (!in_dev) {
      HL_TRY(g_cache.in[0].ensure(bytes));
      d_in = g_cache.in[0].p;
      int rc;
      // (where compress_impl reduces the norm of such an input while it arrives, so does this)
      const bool streamed = norm_streams_in(in_dev, ebtype) && mgh_sym16_supported(h);
      if (streamed) rc = stream_in_with_norm(h, g_cache.in[0].p, original, bytes, elem, s, st);
      else if ((rc = copy_any(g_cache.in[0].p, original, bytes, g_cache.copy_st)) == MGH_SUCCESS &&
               hipEventRecord(g_cache.in_ready[0], g_cache.copy_st) != hipSuccess)
        rc = hl_fail(MGH_ERR_DEVICE, "hipEventRecord");
      if (rc != MGH_SUCCESS) return fail_drained(rc);
      if (hipStreamWaitEvent(st, g_cache.in_ready[0], 0) != hipSuccess)
        return fail_drained(hl_fail(MGH_ERR_DEVICE, "hipEventRecord"));
      if (streamed && (rc = mgh_norm_stream_end(h, s, &norm, st)) != MGH_SUCCESS) return fail_drained(rc);
      have_norm = have_norm || streamed;
    }
    int rc;
    if (!have_norm && (rc = mgh_norm(h, d_in, s, &norm, st)) != MGH_SUCCESS) return fail_drained(rc);
    if ((rc = L.q.ensure(std::max<size_t>(bytes, n * 8))) != MGH_SUCCESS) return fail_drained(rc);
    if ((rc = mgh_decompose(h, d_in, L.q.p, st)) != MGH_SUCCESS) return fail_drained(rc);
    return MGH_SUCCESS;
  }

  // The second entry into the writer: the container mgh_compress(tol) writes for this array, from the
  // coefficients begin() left in lane 0's buffer (they survive the call: the next tolerance reads them
  // again). What compress_impl does for its one subdomain behind the decomposition, in its order:
  // output, lists, header size, quantizer, lossless_begin, then encode_record / write_record, which
  // both entries call. The quantizing step:
  //   - reorder == 0 and the single-pass encoder (lossless_sym16_ok): mgh_quantize_symbols into the
  //     lane's second buffer, with the histogram into the context's bins where kFusedSymbolHistogram
  //     says so (DESIGN.md section 8 has the measurement);
  //   - else mgh_quantize to int64 there and, for reorder == 1, mgh_level_linearize into a third buffer.
  // Host buffers are not registered here (auto_pin_host_buffers: begin() has moved the input already).
  // layer >= 0 (mgh_compress_layers, which has refused everything but the first route): the quantizing step
  // is mgh_quantize_symbols_residual, which leaves what this layer did not take of the coefficients in the
  // OTHER of two buffers (lane 0's q and q3). encode_record may run the step again (outlier overflow), and
  // that pass must read what the first read, so the two swap roles only when the record is written. A
  // record the RAW rule would store raw ends the call (write_record).
  // layer >= 0 with cfg.reorder (mgh_compress_level_layers, which sets it whatever the caller's says): the
  // quantizing step is mgh_quantize_residual_linear -- the level-linearised integers straight into the
  // lane's second buffer, the list's indices linearised, the residual in array order with the same
  // ping-pong.
  static constexpr bool kFusedSymbolHistogram = true;
  int write(double tol, void **compressed, size_t *compressed_size, bool prealloc, int layer = -1) {
    Lane &L = g_cache.lane[0];
    hipStream_t st = L.st;
    const OutSlot slot = out_slot(compressed, prealloc);
    RecordSink sink;
    HL_TRY(writer_output(slot, n, elem, compressed_size, sink));
    auto cleanup = [&](int rc) {
      if (rc != MGH_SUCCESS) fail_drained(rc);
      return slot.fail(rc);
    };
    const uint64_t dict = cfg.huff_dict_size, chunk = cfg.huff_block_size;
    const bool sym16 = !cfg.reorder && lossless_sym16_ok(dict, chunk) && !qsym_refusal(n, dict);
    const uint64_t ocap = std::max<uint64_t>(1, (uint64_t)(cfg.estimate_outlier_ratio * (double)n));
    int rc;
    if ((rc = L.q2.ensure(sym16 ? n * 2 : n * 8)) != MGH_SUCCESS) return cleanup(rc);
    if (cfg.reorder && layer < 0 && (rc = L.q3.ensure(n * 8)) != MGH_SUCCESS) return cleanup(rc);
    if (layer >= 0 && (rc = L.q3.ensure(n * elem)) != MGH_SUCCESS) return cleanup(rc);
    const void *const coef = layer >= 0 && res_in_q3 ? L.q3.p : L.q.p;
    void *const residual = layer < 0 ? nullptr : res_in_q3 ? L.q.p : L.q3.p;
    if ((rc = ensure_lane_lists(L, ocap)) != MGH_SUCCESS) return cleanup(rc);
    fmt::Header hdr;
    size_t meta_size;
    if ((rc = header_step(dd, dtype, ebtype, tol, s, ebtype == MGH_REL ? norm : 0.0, cptr, cfg, sink, hdr, meta_size)) !=
        MGH_SUCCESS)
      return cleanup(rc);

    LosslessJob lj;
    auto quantize = [&]() -> int {
      // (outlier counter of the lane + the lossless stage's bins and chunk states: one launch)
      HL_TRY(lossless_prepare(L.ll, n, dict, chunk, st, (unsigned long long *)L.ocount.p));
      if (!L.ll->prepared_n) HL_HIP(hipMemsetAsync(L.ocount.p, 0, 8, st));
      const bool fused_bins = sym16 && kFusedSymbolHistogram && L.ll->prepared_n != 0;
      const int64_t *q_enc = (const int64_t *)L.q2.p;
      if (layer >= 0 && cfg.reorder) {
        HL_TRY(mgh_quantize_residual_linear(h, coef, ebtype, tol, s, norm, dict, (int64_t *)L.q2.p, (uint64_t *)L.ocount.p,
                                            (uint64_t *)L.oidx.p, (int64_t *)L.oval.p, L.ocap, residual, st));
      } else if (layer >= 0) {
        HL_TRY(mgh_quantize_symbols_residual(h, coef, ebtype, tol, s, norm, dict, (uint16_t *)L.q2.p,
                                             fused_bins ? (uint32_t *)L.ll->freq.p : nullptr, (uint64_t *)L.ocount.p,
                                             (uint64_t *)L.oidx.p, (int64_t *)L.oval.p, L.ocap, residual, st));
      } else if (sym16) {
        HL_TRY(mgh_quantize_symbols(h, L.q.p, ebtype, tol, s, norm, dict, (uint16_t *)L.q2.p,
                                    fused_bins ? (uint32_t *)L.ll->freq.p : nullptr, (uint64_t *)L.ocount.p,
                                    (uint64_t *)L.oidx.p, (int64_t *)L.oval.p, L.ocap, st));
      } else {
        HL_TRY(mgh_quantize(h, L.q.p, ebtype, tol, s, norm, dict, 1, (int64_t *)L.q2.p, (uint64_t *)L.ocount.p,
                            (uint64_t *)L.oidx.p, (int64_t *)L.oval.p, L.ocap, st));
        if (cfg.reorder) {
          // config.reorder == 1: the lossless stage sees the integers level by level, outlier
          // indices are positions in that array (as in compress_impl)
          HL_TRY(mgh_level_linearize(h, (const int64_t *)L.q2.p, (int64_t *)L.q3.p, 0, (uint64_t *)L.oidx.p,
                                     (const uint64_t *)L.ocount.p, 0, L.ocap, st));
          q_enc = (const int64_t *)L.q3.p;
        }
      }
      compress_stats().quantize_passes++;
      if (!fused_bins) compress_stats().histogram_launches++;
      lj = subdomain_job(L, cfg, q_enc, n, elem, sym16, fused_bins);
      return lossless_begin(L.ll, lj, st);
    };
    if ((rc = quantize()) != MGH_SUCCESS) return cleanup(rc);
    if ((rc = encode_record(L, lj, sink, quantize)) != MGH_SUCCESS) return cleanup(rc);
    if ((rc = write_record(L, n, elem, d_in, sink, &hdr, meta_size, layer,
                           cfg.reorder ? "compress_level_layers: " : "compress_layers: ")) != MGH_SUCCESS)
      return cleanup(rc);
    if (layer >= 0) res_in_q3 = !res_in_q3;
    *compressed_size = sink.byte_offset;
    return MGH_SUCCESS;
  }

  // Per tolerance: the coefficients as the decoder will see them into the lane's second buffer
  // (mgh_quantize_roundtrip), recomposed there in place, compared with the input on the device by the
  // kernel of mgh_compare -- the launch mgh_verify makes for a container of one subdomain (dense `a`
  // read in place, dense `b`), so the sums add up in the same order.
  int achieved(int ntol, const double *tols, mgh_error_stats *out) {
    Lane &L = g_cache.lane[0];
    hipStream_t st = L.st;
    int rc;
    if ((rc = L.q2.ensure(n * elem)) != MGH_SUCCESS) return fail_drained(rc);
    if ((rc = L.cmp.ensure(mgh_compare_scratch_bytes_())) != MGH_SUCCESS) return fail_drained(rc);
    for (int k = 0; k < ntol; k++) {
      if ((rc = mgh_quantize_roundtrip(h, L.q.p, ebtype, tols[k], s, norm, L.q2.p, st)) != MGH_SUCCESS) return fail_drained(rc);
      if ((rc = mgh_recompose(h, L.q2.p, L.q2.p, st)) != MGH_SUCCESS) return fail_drained(rc);
      if ((rc = mgh_compare_device_(D, dtype, shape_v.data(), d_in, nullptr, L.q2.p, nullptr, L.cmp.p, st)) != MGH_SUCCESS)
        return fail_drained(rc);
      // (pageable destination: the copy has landed when the call returns, and L.cmp is free for the next)
      if (hipMemcpyAsync(&out[k], L.cmp.p, sizeof(mgh_error_stats), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess)
        return fail_drained(hl_fail(MGH_ERR_DEVICE, "achieved errors: reading the statistics back"));
    }
    return MGH_SUCCESS;
  }

  // one histogram pass per launch group, the codes on the host, the brackets
  int price(int ntol, const double *tols, mgh_size_estimate *out) {
    Lane &L = g_cache.lane[0];
    hipStream_t st = L.st;
    const uint64_t dict = cfg.huff_dict_size, chunk = cfg.huff_block_size;
    const size_t fbytes = (size_t)ntol * dict * 4, o_outl = (fbytes + 7) / 8 * 8;
    HL_TRY(L.q2.ensure(o_outl + (size_t)ntol * 8));
    uint32_t *d_freq = (uint32_t *)L.q2.p;
    uint64_t *d_outl = (uint64_t *)((char *)L.q2.p + o_outl);
    int rc = mgh_quantize_histograms(h, L.q.p, ebtype, ntol, tols, s, norm, dict, d_freq, d_outl, st);
    if (rc != MGH_SUCCESS) return fail_drained(rc);
    freq.resize((size_t)ntol * dict);
    outl.resize(ntol);
    if (hipMemcpyAsync(freq.data(), d_freq, fbytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(outl.data(), d_outl, (size_t)ntol * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return fail_drained(hl_fail(MGH_ERR_DEVICE, "size estimates: reading the histograms back"));
    const long sync_env = env_get("MGH_HUFF_SYNC", 1);
    for (int k = 0; k < ntol; k++) {
      try {
        huff::build_codebook(freq.data() + (size_t)k * dict, (int)dict, cb);
      } catch (const std::exception &e) {
        return hl_fail(MGH_ERR_INVALID_ARGUMENT, e.what());
      }
      const bool with_sync = record_has_sync(cfg.lossless, dict, chunk, cb.total_bits, n, sync_env);
      const ByteBracket rb = record_bytes_bracket(n, dict, chunk, cb.total_bits, outl[k], with_sync);
      fmt::Header hdr;
      header_from(dd, dtype, ebtype, tols[k], s, ebtype == MGH_REL ? norm : 0.0, cptr, cfg, hdr);
      const ContainerBracket c = container_bytes_bracket(fmt::serialize_metadata(hdr).size(), n, elem, rb);
      out[k] = mgh_size_estimate{tols[k], c.min, c.max, outl[k], cb.total_bits, c.raw};
    }
    return MGH_SUCCESS;
  }
};

} // namespace

extern "C" {

void mgh_config_default(mgh_config *c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->dev_id = 0;
  c->domain_decomposition = MGH_DD_MAXDIM;
  c->domain_decomposition_dim = 0;
  c->block_size = 256;
  c->estimate_outlier_ratio = 1.0;
  c->huff_dict_size = 8192;
  c->huff_block_size = 1024 * 20;
  c->lossless = MGH_LOSSLESS_HUFFMAN;
  c->zstd_compress_level = 3;
  c->normalize_coordinates = 1;
  c->max_larget_level = std::numeric_limits<uint64_t>::max();
  c->max_memory_footprint = std::numeric_limits<uint64_t>::max();
  c->reorder = 0;
  c->mirror_reference_coord_cast = 0;
  // The reference defaults to true. Here it is opt-in: on ROCm 7.0 registering and unregistering
  // caller memory (hipHostRegister / hipHostUnregister) was observed to leave the runtime
  // treating later allocations at the same addresses as pinned -- a copy into such a buffer
  // then dies with a GPU memory fault (1 in 3 runs of the test suite). Without registration
  // pageable buffers travel through the library's own ring of pinned slots (staged_h2d / _d2h):
  // 512^3 f32 host to host 15.2 / 16.9 ms against 13.7 / 13.7 ms with registered buffers (round 6,
  // bench.py end_to_end_host) -- and registering costs 16 ms per 512 MB the first time.
  c->auto_pin_host_buffers = 0;
}

int mgh_compress(int D, int dtype, const uint64_t *shape, double tol, double s, int ebtype,
                 const void *original_data, void **compressed_data, size_t *compressed_size,
                 const void *const *coords, const mgh_config *config, int output_pre_allocated) {
  if (!compressed_data || !compressed_size) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  HL_TRY(size_call_args(D, dtype, shape, ebtype, original_data, config, output_pre_allocated ? compressed_data : nullptr));
  return hl_guarded([&]() -> int {
    if (dtype == MGH_FLOAT)
      return compress_impl<float>(D, dtype, shape, tol, s, ebtype, original_data, compressed_data,
                                  compressed_size, coords, *config, output_pre_allocated != 0);
    return compress_impl<double>(D, dtype, shape, tol, s, ebtype, original_data, compressed_data,
                                 compressed_size, coords, *config, output_pre_allocated != 0);
  });
}

int mgh_estimate_sizes(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, double s, int ebtype,
                       const void *original_data, const void *const *coords, const mgh_config *config,
                       mgh_size_estimate *out) {
  if (!tols || !out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (ntol < 1 || ntol > kQhistMaxTols) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "ntol must be in 1..64");
  HL_TRY(size_call_args(D, dtype, shape, ebtype, original_data, config));
  return hl_guarded([&]() -> int {
    CoefficientSession E;
    HL_TRY(E.begin("size estimates: ", true, D, dtype, shape, s, ebtype, original_data, coords, *config));
    return E.price(ntol, tols, out);
  });
}

int mgh_compress_budget(int D, int dtype, const uint64_t *shape, size_t max_bytes, double tol_min, double tol_max,
                        int rounds, double s, int ebtype, const void *original_data, void **compressed_data,
                        size_t *compressed_size, const void *const *coords, const mgh_config *config,
                        int output_pre_allocated, double *tol_used, mgh_size_estimate *estimate_used) {
  if (!compressed_data || !compressed_size || !tol_used) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*compressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  if (!(tol_min > 0) || !(tol_min <= tol_max) || !std::isfinite(tol_max) || rounds < 1 || rounds > 8)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "compress_budget: 0 < tol_min <= tol_max (finite), rounds in 1..8");
  HL_TRY(size_call_args(D, dtype, shape, ebtype, original_data, config));
  mgh_size_estimate used{};
  return hl_guarded([&]() -> int {
    CoefficientSession E;
    compress_stats() = mgh_compress_stats{};
    HL_TRY(E.begin("size estimates: ", true, D, dtype, shape, s, ebtype, original_data, coords, *config));
    compress_stats().decompositions++;
    int rc = MGH_SUCCESS;
    std::vector<mgh_size_estimate> seen;  // every candidate priced, in order
    auto fits3 = [&](const double m[3], bool ok[3]) {
      mgh_size_estimate e[3];
      if (rc == MGH_SUCCESS) rc = E.price(3, m, e);
      for (int k = 0; k < 3; k++) {
        ok[k] = rc == MGH_SUCCESS && e[k].bytes_max <= max_bytes;
        if (rc == MGH_SUCCESS) seen.push_back(e[k]);
      }
    };
    auto fits1 = [&](double tol) {
      mgh_size_estimate e;
      if (rc == MGH_SUCCESS) rc = E.price(1, &tol, &e);
      if (rc != MGH_SUCCESS) return false;
      seen.push_back(e);
      return e.bytes_max <= max_bytes;
    };
    const SearchResult r = budget_search(tol_min, tol_max, rounds, fits1, fits3);
    HL_TRY(rc);
    if (r.end == SearchEnd::bad_argument) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "compress_budget: tolerances or rounds");
    if (r.end == SearchEnd::nothing_fits)
      return hl_fail(MGH_ERR_OUTPUT_TOO_LARGE, "compress_budget: the container of tol_max is larger than max_bytes");
    *tol_used = r.tol;
    for (const mgh_size_estimate &e : seen)
      if (e.tol == r.tol) used = e;
    if (estimate_used) *estimate_used = used;
    // the container of tol_used from the coefficients the candidates were priced on (CoefficientSession::write)
    void *const given = *compressed_data;
    HL_TRY(E.write(*tol_used, compressed_data, compressed_size, output_pre_allocated != 0));
    if (*compressed_size > max_bytes) {  // (the bracket is an invariant of the record's layout: never expected)
      E.out_slot(compressed_data, output_pre_allocated != 0).fail(MGH_ERR_FORMAT);
      if (!output_pre_allocated) *compressed_data = given;  // (not NULL: what the caller passed in)
      return hl_fail(MGH_ERR_FORMAT, "compress_budget: the container left the estimate's bracket");
    }
    return MGH_SUCCESS;
  });
}

int mgh_achieved_errors(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, double s, int ebtype,
                        const void *original_data, const void *const *coords, const mgh_config *config,
                        mgh_error_stats *out) {
  if (!tols || !out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (ntol < 1 || ntol > kTargetMaxTols) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "achieved_errors: ntol must be in 1..64");
  HL_TRY(size_call_args(D, dtype, shape, ebtype, original_data, config));
  return hl_guarded([&]() -> int {
    CoefficientSession E;
    HL_TRY(E.begin("achieved errors: ", false, D, dtype, shape, s, ebtype, original_data, coords, *config));
    return E.achieved(ntol, tols, out);
  });
}

int mgh_compress_target(int D, int dtype, const uint64_t *shape, int metric, double target, double tol_min,
                        double tol_max, int rounds, double s, int ebtype, const void *original_data,
                        void **compressed_data, size_t *compressed_size, const void *const *coords,
                        const mgh_config *config, int output_pre_allocated, double *tol_used, mgh_error_stats *stats_used,
                        int *candidates) {
  if (!compressed_data || !compressed_size || !tol_used) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*compressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  if (!target_metric_valid(metric) || std::isnan(target))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "compress_target: metric in 0..2 (max_abs, rmse, psnr), target not NaN");
  if (!(tol_min > 0) || !(tol_min <= tol_max) || !std::isfinite(tol_max) || rounds < 1 || rounds > kTargetMaxRounds)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "compress_target: 0 < tol_min <= tol_max (finite), rounds in 1..16");
  HL_TRY(size_call_args(D, dtype, shape, ebtype, original_data, config));
  mgh_error_stats used{};
  int evaluated = 0;
  return hl_guarded([&]() -> int {
    CoefficientSession E;
    compress_stats() = mgh_compress_stats{};
    HL_TRY(E.begin("achieved errors: ", false, D, dtype, shape, s, ebtype, original_data, coords, *config));
    compress_stats().decompositions++;
    int rc = MGH_SUCCESS;
    std::vector<std::pair<double, mgh_error_stats>> seen;  // every candidate evaluated, in order
    auto meets = [&](double tol) {
      mgh_error_stats e{};
      if (rc == MGH_SUCCESS) rc = E.achieved(1, &tol, &e);
      if (rc != MGH_SUCCESS) return false;
      seen.emplace_back(tol, e);
      return target_meets(e, (TargetMetric)metric, target);
    };
    const TargetResult r = target_search(tol_min, tol_max, rounds, meets);
    HL_TRY(rc);
    if (r.end == TargetEnd::bad_argument) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "compress_target: tolerances or rounds");
    if (r.end == TargetEnd::nothing_meets)
      return hl_fail(MGH_ERR_TARGET_NOT_MET, "compress_target: not even tol_min meets the target");
    *tol_used = r.tol;
    evaluated = r.candidates;
    for (const auto &c : seen)
      if (c.first == r.tol) used = c.second;
    if (stats_used) *stats_used = used;
    if (candidates) *candidates = evaluated;
    // the container of tol_used from the coefficients the candidates share (CoefficientSession::write)
    return E.write(*tol_used, compressed_data, compressed_size, output_pre_allocated != 0);
  });
}

int mgh_compress_ladder(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, double s, int ebtype,
                        const void *original_data, void **compressed_data, size_t *compressed_size,
                        const void *const *coords, const mgh_config *config, int output_pre_allocated) {
  if (!tols || !compressed_data || !compressed_size) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  HL_TRY(tolerance_list_args("compress_ladder: ", ntol, tols, compressed_data, output_pre_allocated != 0, false));
  HL_TRY(size_call_args(D, dtype, shape, ebtype, original_data, config));
  if (!output_pre_allocated)
    for (int k = 0; k < ntol; k++) compressed_data[k] = nullptr;
  return hl_guarded([&]() -> int {
    CoefficientSession E;
    compress_stats() = mgh_compress_stats{};
    HL_TRY(E.begin("compress_ladder: ", false, D, dtype, shape, s, ebtype, original_data, coords, *config));
    compress_stats().decompositions++;
    // (a failure at tolerance k leaves containers 0 .. k-1 the caller's; write() has freed its own)
    for (int k = 0; k < ntol; k++)
      HL_TRY(E.write(tols[k], &compressed_data[k], &compressed_size[k], output_pre_allocated != 0));
    return MGH_SUCCESS;
  });
}

int mgh_compress_layers(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, double s, int ebtype,
                        const void *original_data, void **compressed_data, size_t *compressed_size,
                        const void *const *coords, const mgh_config *config, int output_pre_allocated) {
  if (!tols || !compressed_data || !compressed_size) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  HL_TRY(tolerance_list_args("compress_layers: ", ntol, tols, compressed_data, output_pre_allocated != 0, true));
  HL_TRY(size_call_args(D, dtype, shape, ebtype, original_data, config));
  {
    // what the layer writer does not take, before anything is allocated
    uint64_t n = 1;
    for (int d = 0; d < D; d++) n *= shape[d];
    Decomposer dd;
    HL_TRY(make_decomposer(dd, D, shape, dtype == MGH_FLOAT ? 4 : 8, *config));
    HL_TRY(one_subdomain_only("compress_layers: ", dd));
    if (config->reorder)
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, "compress_layers: reorder = 1 is not supported (the layers are reorder = 0 records)");
    if (!lossless_sym16_ok(config->huff_dict_size, config->huff_block_size))
      return hl_fail(MGH_ERR_INVALID_ARGUMENT,
                     "compress_layers: huff_dict_size / huff_block_size outside what the single-pass encoder takes");
    if (const char *bad = qsym_refusal(n, config->huff_dict_size))
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string("compress_layers: ") + bad);
  }
  if (!output_pre_allocated)
    for (int k = 0; k < ntol; k++) compressed_data[k] = nullptr;
  return hl_guarded([&]() -> int {
    CoefficientSession E;
    compress_stats() = mgh_compress_stats{};
    HL_TRY(E.begin("compress_layers: ", false, D, dtype, shape, s, ebtype, original_data, coords, *config));
    compress_stats().decompositions++;
    // (a failure at layer k leaves containers 0 .. k-1 the caller's; write() has freed its own)
    for (int k = 0; k < ntol; k++)
      HL_TRY(E.write(tols[k], &compressed_data[k], &compressed_size[k], output_pre_allocated != 0, k));
    return MGH_SUCCESS;
  });
}

int mgh_compress_level_layers(int D, int dtype, const uint64_t *shape, int ntol, const double *tols, double s, int ebtype,
                              const void *original_data, void **compressed_data, size_t *compressed_size,
                              const void *const *coords, const mgh_config *config, int output_pre_allocated) {
  if (!tols || !compressed_data || !compressed_size) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  HL_TRY(tolerance_list_args("compress_level_layers: ", ntol, tols, compressed_data, output_pre_allocated != 0, true));
  HL_TRY(size_call_args(D, dtype, shape, ebtype, original_data, config));
  mgh_config cfg = *config;
  cfg.reorder = 1;  // (the records are level-linearised whatever the caller's configuration says)
  {
    // what the layer writer does not take, before anything is allocated
    uint64_t n = 1;
    for (int d = 0; d < D; d++) n *= shape[d];
    Decomposer dd;
    HL_TRY(make_decomposer(dd, D, shape, dtype == MGH_FLOAT ? 4 : 8, cfg));
    HL_TRY(one_subdomain_only("compress_level_layers: ", dd));
    if (const char *bad = qsym_refusal(n, cfg.huff_dict_size))
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string("compress_level_layers: ") + bad);
  }
  if (!output_pre_allocated)
    for (int k = 0; k < ntol; k++) compressed_data[k] = nullptr;
  return hl_guarded([&]() -> int {
    CoefficientSession E;
    compress_stats() = mgh_compress_stats{};
    HL_TRY(E.begin("compress_level_layers: ", false, D, dtype, shape, s, ebtype, original_data, coords, cfg));
    compress_stats().decompositions++;
    // (a failure at layer k leaves containers 0 .. k-1 the caller's; write() has freed its own)
    for (int k = 0; k < ntol; k++)
      HL_TRY(E.write(tols[k], &compressed_data[k], &compressed_size[k], output_pre_allocated != 0, k));
    return MGH_SUCCESS;
  });
}

int mgh_last_compress_stats(mgh_compress_stats *out) {
  if (!out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = compress_stats();
  return MGH_SUCCESS;
}

int mgh_histogram_sym16(const uint16_t *d_symbols, uint64_t n, uint64_t dict_size, uint32_t *d_freq, void *stream) {
  if (!d_symbols || !d_freq) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (n == 0 || n >= ((uint64_t)1 << 32) || dict_size < 2 || dict_size > 16384)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "histogram_sym16: 1 .. 2^32 - 1 symbols, dict_size in 2..16384");
  const unsigned hblocks =
      (unsigned)std::min<size_t>((n + huff::kHistThreads - 1) / huff::kHistThreads, 2 * (size_t)hl_num_cu());
  huff::k_histogram<uint16_t><<<hblocks, huff::kHistThreads, dict_size * 4, (hipStream_t)stream>>>(
      d_symbols, n, (int)dict_size, (unsigned *)d_freq);
  HL_HIP(hipGetLastError());
  return MGH_SUCCESS;
}

static int decompress_entry(const void *compressed_data, size_t compressed_size, void **decompressed_data,
                            const mgh_config *config, int output_pre_allocated, size_t expect_bytes, int expect_dtype,
                            int level = -1, int halvings = -1, bool preview = false, const uint64_t *win_lo = nullptr,
                            const uint64_t *win_ext = nullptr, VerifyJob *vfy = nullptr);

int mgh_decompress_preview(const void *compressed_data, size_t compressed_size, int halvings, void **decompressed_data,
                           const mgh_config *config, int output_pre_allocated) {
  if (halvings < 0)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "halvings outside 0 .. the smallest l_target of the subdomains");
  return decompress_entry(compressed_data, compressed_size, decompressed_data, config, output_pre_allocated, 0, -1, -1,
                          halvings, true);
}

int mgh_decompress_preview_window(const void *compressed_data, size_t compressed_size, int halvings, const uint64_t *lo,
                                  const uint64_t *ext, void **decompressed_data, const mgh_config *config,
                                  int output_pre_allocated) {
  if (!lo || !ext) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (halvings < 0)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "halvings outside 0 .. the smallest l_target of the subdomains");
  return decompress_entry(compressed_data, compressed_size, decompressed_data, config, output_pre_allocated, 0, -1, -1,
                          halvings, true, lo, ext);
}

int mgh_decompress_coarsened(const void *compressed_data, size_t compressed_size, int halvings, void **decompressed_data,
                             const mgh_config *config, int output_pre_allocated) {
  if (halvings < 0)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "halvings outside 0 .. the smallest l_target of the subdomains");
  return decompress_entry(compressed_data, compressed_size, decompressed_data, config, output_pre_allocated, 0, -1, -1,
                          halvings);
}

int mgh_decompress_level(const void *compressed_data, size_t compressed_size, int level, void **decompressed_data,
                         const mgh_config *config, int output_pre_allocated) {
  if (level < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "level outside 0 .. l_target");
  return decompress_entry(compressed_data, compressed_size, decompressed_data, config, output_pre_allocated, 0, -1, level);
}

int mgh_decompress(const void *compressed_data, size_t compressed_size, void **decompressed_data,
                   const mgh_config *config, int output_pre_allocated) {
  return decompress_entry(compressed_data, compressed_size, decompressed_data, config, output_pre_allocated, 0, -1);
}

int mgh_decompress_into(const void *compressed_data, size_t compressed_size, void *out, size_t out_bytes,
                        int out_dtype, const mgh_config *config) {
  if (!out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (out_dtype != MGH_FLOAT && out_dtype != MGH_DOUBLE) return hl_fail(MGH_ERR_UNSUPPORTED_DTYPE, "dtype");
  void *dst = out;
  return decompress_entry(compressed_data, compressed_size, &dst, config, 1, out_bytes, out_dtype);
}

// expect_dtype >= 0: the caller's buffer holds expect_bytes bytes of that type -- checked against the
// header the call reads anyway, before anything is written (mgh_decompress_into)
// vfy: mgh_verify -- the buffer is the ORIGINAL (vfy->original) and there is no output; the bound of
// the header is left in vfy for the caller to evaluate
static int decompress_entry(const void *compressed_data, size_t compressed_size, void **decompressed_data,
                            const mgh_config *config, int output_pre_allocated, size_t expect_bytes, int expect_dtype,
                            int level, int halvings, bool preview, const uint64_t *win_lo, const uint64_t *win_ext,
                            VerifyJob *vfy) {
  const char *who = vfy ? "mgh_verify" : "mgh_decompress_into";
  decompress_stats() = mgh_decompress_stats{};
  if (!compressed_data || !decompressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (!vfy && output_pre_allocated && !*decompressed_data)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  {
    const std::string bad = env_validate();
    if (!bad.empty()) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad);
  }
  mgh_config def;
  if (!config) {
    mgh_config_default(&def);
    config = &def;
  }
  int ndev = mgh_device_count();
  if (ndev <= 0) return hl_fail(MGH_ERR_NO_DEVICE, "no HIP device");
  if (hipSetDevice(config->dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  std::unique_ptr<HostPrefix> prefix;
  if (is_device_pointer(compressed_data)) prefix.reset(new HostPrefix(compressed_data, compressed_size));
  fmt::Header hd;
  size_t meta_size = 0;
  HL_TRY(read_header(compressed_data, compressed_size, hd, meta_size));
  if (hd.shape.empty() || hd.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "header: dimension");
  if (!hd.quantized) return hl_fail(MGH_ERR_FORMAT, "not a compressed (quantized) stream");
  if (expect_dtype >= 0) {
    size_t need = hd.is_double ? 8 : 4;
    for (uint64_t e : hd.shape) need *= e;
    if ((expect_dtype == MGH_DOUBLE) != hd.is_double)
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + ": the stream holds the other data type");
    if (expect_bytes != need)
      return hl_fail(MGH_ERR_INVALID_ARGUMENT,
                     std::string(who) + ": the buffer does not have the size of the array in the stream");
  }
  if (vfy) {
    vfy->rel = hd.rel;
    vfy->tol = hd.tol;
    vfy->s = hd.s;
    vfy->norm = hd.norm;
  }
  Window window;
  if (win_lo) {
    window.lo.assign(win_lo, win_lo + hd.shape.size());
    window.ext.assign(win_ext, win_ext + hd.shape.size());
    for (size_t d = 0; d < hd.shape.size(); d++)
      if (window.ext[d] == 0 || window.lo[d] > hd.shape[d] || window.ext[d] > hd.shape[d] - window.lo[d])
        return hl_fail(MGH_ERR_INVALID_ARGUMENT, "the window leaves the array");
  }
  const Window *win = win_lo ? &window : nullptr;
  return hl_guarded([&]() -> int {
    if (hd.is_double)
      return decompress_impl<double>(hd, meta_size, compressed_data, compressed_size, decompressed_data,
                                     *config, output_pre_allocated != 0, level, halvings, preview, win, vfy);
    return decompress_impl<float>(hd, meta_size, compressed_data, compressed_size, decompressed_data,
                                  *config, output_pre_allocated != 0, level, halvings, preview, win, vfy);
  });
}


int mgh_verify(const void *compressed_data, size_t compressed_size, const void *original, size_t original_bytes,
               int original_dtype, int halvings, const mgh_config *config, mgh_verify_result *out) {
  if (!original || !out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (original_dtype != MGH_FLOAT && original_dtype != MGH_DOUBLE) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_verify: dtype");
  if (halvings < 0)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "halvings outside 0 .. the smallest l_target of the subdomains");
  VerifyJob job;
  job.original = original;
  void *none = nullptr;  // (there is no output: pre-allocated, and never looked at)
  // (halvings = 0 goes the way of mgh_decompress_preview(0), which is mgh_decompress)
  const int rc = decompress_entry(compressed_data, compressed_size, &none, config, 1, original_bytes, original_dtype, -1,
                                  halvings, true, nullptr, nullptr, &job);
  if (rc != MGH_SUCCESS) return rc;
  const bool normalize = config ? config->normalize_coordinates != 0 : true;
  mgh_verify_result r{};
  r.stats = job.stats;
  r.bound = job.rel ? job.tol * job.norm : job.tol;
  r.bound_kind = std::isinf(job.s) ? 0 : job.s == 0 ? 1 : -1;
  r.achieved = r.bound_kind == 0 ? r.stats.max_abs_err
               : r.bound_kind == 1 ? mgh::l2_error(r.stats, normalize) : 0.0;
  if (halvings > 0 || r.bound_kind < 0) r.within = -1;  // (a preview carries no bound)
  else r.within = r.stats.nonfinite == 0 && r.achieved <= r.bound ? 1 : 0;
  *out = r;
  return MGH_SUCCESS;
}

}  // extern "C"

// ---- one process, several devices ------------------------------------------------------------
// The domain is cut into slabs along the slowest dimension (recorded in the header as a
// MaxDim decomposition of dimension 0, so any MGARD-X reader finds the subdomains where it
// expects them); slab id runs on device dev_ids[id % num_dev], every device on its own host
// thread with its own streams and caches. Subdomains are independent (own hierarchy, no halo:
// DomainDecomposer.hpp:260-303); the only coupling is the error budget of a REL bound: the slab
// norms are combined on the host (ErrorToleranceCalculator.hpp:69-89) and every slab then runs
// with the ABS bound calc_local_abs_tol (:134-155) -- exactly what mgh_compress does for a
// decomposed domain, so the container is the one mgh_compress would write with this decomposition
// (up to the order of the outlier lists) and mgh_decompress / mgh_decompress_multi both read it.
// Payloads are framed `[u64 size][payload]` in id order (GPUPipelines.hpp:189-193).
namespace {

struct MultiErr {
  std::mutex m;
  int rc = MGH_SUCCESS;
  std::string msg;
  void set(int code) {
    std::lock_guard<std::mutex> g(m);
    if (rc == MGH_SUCCESS) {
      rc = code;
      msg = mgh_last_error();
    }
  }
};

void worker_thread_teardown();

template <typename T>
int compress_multi_impl(int ndev, const int *devs, int D, int dtype, const uint64_t *shape,
                        double tol_d, double s_d, int ebtype, const void *original,
                        void **compressed, size_t *compressed_size, const void *const *coords_in,
                        const mgh_config &cfg0, bool prealloc) {
  const size_t elem = sizeof(T);
  const Decomposer dd = Decomposer::slabs_of_dim0(std::vector<uint64_t>(shape, shape + D), multi_slab_size(shape[0], ndev));
  if (!dd.decomposed) {  // nothing to share out
    mgh_config c = cfg0;
    c.dev_id = devs[0];
    return mgh_compress(D, dtype, shape, tol_d, s_d, ebtype, original, compressed, compressed_size,
                        coords_in, &c, prealloc);
  }
  size_t total = 1, inner = 1;
  for (int d = 0; d < D; d++) total *= shape[d];
  for (int d = 1; d < D; d++) inner *= shape[d];
  const T tol = (T)tol_d, s = (T)s_d;
  std::vector<std::vector<double>> coords;
  if (coords_in) {
    coords.resize(D);
    for (int d = 0; d < D; d++) {
      const T *c = static_cast<const T *>(coords_in[d]);
      coords[d].assign(c, c + shape[d]);
    }
  }
  // Device-resident input (GPUPipelines.hpp:69-207 takes device pointers): the volume lives on ONE
  // device; a slab that runs elsewhere travels there ONCE, device to device (hipMemcpyPeerAsync:
  // xGMI), into a buffer of the worker that serves both the norm and the compression; slabs of
  // the source device are compressed where they are. The container is assembled in device
  // memory of the source device (same memory space as the input, like mgh_compress).
  const bool in_dev = is_device_pointer(original);
  int src_dev = -1;
  if (in_dev) {
    hipPointerAttribute_t a;
    HL_HIP(hipPointerGetAttributes(&a, original));
    src_dev = a.device;
  }
  const uint64_t num = dd.num;
  const int nthr = (int)std::min<uint64_t>(num, (uint64_t)ndev);
  auto slab_ptr = [&](uint64_t id) { return (const char *)original + dd.linear_offset(id) * elem; };
  auto slab_coords = [&](uint64_t id, std::vector<const void *> &out) {
    out.assign(D, nullptr);
    if (!coords_in) return (const void *const *)nullptr;
    for (int d = 0; d < D; d++)
      out[d] = (const void *)(static_cast<const T *>(coords_in[d]) + (d == 0 ? dd.subdomain_offset(id)[0] : 0));
    return (const void *const *)out.data();
  };
  MultiErr err;
  // One worker thread per device for the whole call: (REL) norms of its slabs -> rendezvous, where
  // the last worker to arrive combines them on the host (ErrorToleranceCalculator.hpp:69-89) ->
  // every slab as a stand-alone ABS compression (calc_local_abs_tol).
  std::vector<double> ln(num, 0.0);
  std::vector<void *> part(num, nullptr);
  std::vector<size_t> part_size(num, 0);
  std::mutex rv_m;
  std::condition_variable rv_cv;
  int rv_arrived = 0;
  T norm = 1, local_tol = 0;
  auto rendezvous = [&] {
    std::unique_lock<std::mutex> lk(rv_m);
    if (++rv_arrived == nthr) {
      if (ebtype == MGH_REL && err.rc == MGH_SUCCESS) {
        NormAccumulator na{s == std::numeric_limits<T>::infinity(), cfg0.normalize_coordinates != 0};
        for (uint64_t id = 0; id < num; id++) na.add(ln[id], inner * dd.subdomain_shape(id)[0]);
        norm = (T)na.result(total);
      }
      local_tol = local_abs_tol<T>(ebtype, norm, tol, s, num);
      rv_cv.notify_all();
    } else {
      rv_cv.wait(lk, [&] { return rv_arrived == nthr; });
    }
  };
  {
    std::vector<std::thread> th;
    for (int k = 0; k < nthr; k++)
      th.emplace_back([&, k] {
        bool arrived = false;
        try {
          mgh_config c = cfg0;
          c.dev_id = devs[k];
          c.domain_decomposition = MGH_DD_MAXDIM;  // (a slab that does not fit is split further)
          bool ok = hipSetDevice(c.dev_id) == hipSuccess && cache_prepare(c.dev_id) == MGH_SUCCESS;
          if (!ok) err.set(hl_fail(MGH_ERR_DEVICE, "device of a worker thread"));
          // slabs of this worker; a device-resident slab of another device is brought over once
          // and kept when it is the worker's only one (the usual case: one slab per device)
          std::vector<uint64_t> mine;
          for (uint64_t id = k; id < num; id += nthr) mine.push_back(id);
          // the worker's copies of its remote slabs: every one travels ONCE and serves both the
          // norm and the compression; if they do not all fit the device, the oldest ones are
          // dropped and fetched again when their turn comes
          std::vector<std::pair<uint64_t, std::unique_ptr<DevBuf>>> peers;
          struct PeerGuard {  // (released on every way out of the worker, exceptions included)
            std::vector<std::pair<uint64_t, std::unique_ptr<DevBuf>>> &v;
            ~PeerGuard() {
              for (auto &kv : v) kv.second->release();
              v.clear();
            }
          } peer_guard{peers};
          auto local_ptr = [&](uint64_t id, const void **out) -> int {
            // where this worker reads slab id from: host memory, the source device itself, or a peer copy
            // (MGH_MULTI_FORCE_PEER=1: take the peer copy also when the slab is already on the
            // worker's device -- the one-GPU test of that path)
            static const bool force_peer = env_get("MGH_MULTI_FORCE_PEER", 0) != 0;
            if (!in_dev || (c.dev_id == src_dev && !force_peer)) {
              *out = slab_ptr(id);
              return MGH_SUCCESS;
            }
            for (auto &kv : peers)
              if (kv.first == id) {
                *out = kv.second->p;
                return MGH_SUCCESS;
              }
            const size_t bytes = inner * dd.subdomain_shape(id)[0] * elem;
            std::unique_ptr<DevBuf> nb(new DevBuf());
            while (nb->ensure(bytes) != MGH_SUCCESS) {
              if (peers.empty()) return hl_fail(MGH_ERR_OUT_OF_MEMORY, "peer copy of a slab");
              peers.front().second->release();
              peers.erase(peers.begin());
            }
            HL_HIP(hipMemcpyPeerAsync(nb->p, c.dev_id, slab_ptr(id), src_dev, bytes, g_cache.lane[0].st));
            HL_HIP(hipStreamSynchronize(g_cache.lane[0].st));
            *out = nb->p;
            peers.emplace_back(id, std::move(nb));
            return MGH_SUCCESS;
          };
          if (ok && ebtype == MGH_REL) {
            for (uint64_t id : mine) {
              if (err.rc != MGH_SUCCESS) break;
              const auto sshape = dd.subdomain_shape(id);
              uint64_t cnt = 1;
              for (uint64_t e : sshape) cnt *= e;
              mgh_hierarchy *h = nullptr;
              bool owned = false;
              int rc = get_hierarchy(&h, &owned, dtype, sshape, nullptr, dd.subdomain_offset(id), c);
              const void *src = nullptr;
              if (rc == MGH_SUCCESS && in_dev) rc = local_ptr(id, &src);
              if (rc == MGH_SUCCESS && !in_dev) {
                rc = g_cache.in[0].ensure(cnt * elem);
                if (rc == MGH_SUCCESS) rc = copy_any(g_cache.in[0].p, slab_ptr(id), cnt * elem, g_cache.lane[0].st);
                src = g_cache.in[0].p;
              }
              if (rc == MGH_SUCCESS) rc = mgh_norm(h, src, s_d, &ln[id], g_cache.lane[0].st);
              if (owned) mgh_hierarchy_destroy(h);
              if (rc != MGH_SUCCESS) err.set(rc);
            }
          }
          rendezvous();
          arrived = true;
          if (ok && err.rc == MGH_SUCCESS) {
            for (uint64_t id : mine) {
              if (err.rc != MGH_SUCCESS) break;
              const auto sshape = dd.subdomain_shape(id);
              std::vector<const void *> cs;
              const void *const *cp = slab_coords(id, cs);
              const void *src = nullptr;
              int rc = local_ptr(id, &src);
              size_t sz = 0;
              if (rc == MGH_SUCCESS)
                rc = mgh_compress(D, dtype, sshape.data(), (double)local_tol, s_d, MGH_ABS, src, &part[id], &sz,
                                  cp, &c, 0);
              part_size[id] = sz;
              for (size_t k = 0; k < peers.size(); k++)  // (this slab's copy has served its purpose)
                if (peers[k].first == id) {
                  peers[k].second->release();
                  peers.erase(peers.begin() + k);
                  break;
                }
              if (rc != MGH_SUCCESS) err.set(rc);
            }
          }
          worker_thread_teardown();
        } catch (const std::exception &e) {
          // (an exception must not leave a worker thread: std::terminate)
          err.set(hl_fail(MGH_ERR_OUT_OF_MEMORY, std::string("worker thread: ") + e.what()));
          if (!arrived) rendezvous();  // the others must not wait for this thread for ever
        }
      });
    for (auto &t : th) t.join();
  }
  // (parts are host memory for a host input, device memory of their worker's device otherwise)
  auto free_parts = [&] {
    for (void *p : part) {
      if (!p) continue;
      if (in_dev) (void)hipFree(p); else std::free(p);
    }
  };
  if (err.rc != MGH_SUCCESS) {
    free_parts();
    mgh_set_last_error_(err.msg.c_str());
    return err.rc;
  }
  // ---- assembly: one header, the records in id order -------------------------------------------
  fmt::Header hdr;
  header_from(dd, dtype, ebtype, tol_d, s_d, ebtype == MGH_REL ? (double)norm : 0.0,
              coords_in ? &coords : nullptr, cfg0, hdr);
  const std::vector<uint8_t> meta = fmt::serialize_metadata(hdr);
  std::vector<size_t> body_off(num), body_len(num);
  size_t need = meta.size();
  for (uint64_t id = 0; id < num; id++) {
    fmt::Header sh;
    size_t ms = 0;
    int rc = read_header(part[id], part_size[id], sh, ms);
    if (rc == MGH_SUCCESS && sh.dd_method != fmt::DD_NOOP)
      rc = hl_fail(MGH_ERR_OUT_OF_MEMORY, "a slab does not fit its device in one piece: use more, smaller slabs");
    if (rc != MGH_SUCCESS) {
      free_parts();
      return rc;
    }
    body_off[id] = ms;
    body_len[id] = part_size[id] - ms;
    need += body_len[id];
  }
  if (in_dev && hipSetDevice(src_dev) != hipSuccess) {
    free_parts();
    return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  }
  if (!prealloc) {
    const bool ok = in_dev ? hipMalloc(compressed, need) == hipSuccess : (*compressed = std::malloc(need)) != nullptr;
    if (!ok) {
      free_parts();
      return hl_fail(MGH_ERR_OUT_OF_MEMORY, in_dev ? "hipMalloc" : "malloc");
    }
  } else if (*compressed_size < need) {
    free_parts();
    return hl_fail(MGH_ERR_OUTPUT_TOO_LARGE, "output buffer too small");
  }
  char *o = (char *)*compressed;
  const bool any_dev = in_dev || is_device_pointer(o);
  bool copied = true;
  auto put = [&](size_t at, const void *src, size_t len) {
    if (!any_dev) std::memcpy(o + at, src, len);
    else copied = copied && hipMemcpy(o + at, src, len, hipMemcpyDefault) == hipSuccess;
  };
  put(0, meta.data(), meta.size());
  size_t at = meta.size();
  for (uint64_t id = 0; id < num; id++) {
    put(at, (const char *)part[id] + body_off[id], body_len[id]);
    at += body_len[id];
  }
  free_parts();
  if (!copied) return OutSlot{compressed, in_dev, prealloc}.fail(hl_fail(MGH_ERR_DEVICE, "assembling the container"));
  *compressed_size = at;
  return MGH_SUCCESS;
}

template <typename T>
int decompress_multi_impl(int ndev, const int *devs, const fmt::Header &hd, size_t meta_size,
                          const void *compressed, size_t compressed_size, void **out,
                          const mgh_config &cfg0, bool prealloc) {
  const size_t elem = sizeof(T);
  Decomposer dd;
  HL_TRY(decomposer_from_header(hd, cfg0, dd));
  size_t total = 1;
  for (uint64_t e : hd.shape) total *= e;
  if (!prealloc && !(*out = std::malloc(total * elem))) return hl_fail(MGH_ERR_OUT_OF_MEMORY, "malloc");
  auto bail = [&](int rc) {
    if (!prealloc) {
      std::free(*out);
      *out = nullptr;
    }
    return rc;
  };
  // record offsets (the sizes are in the stream)
  const uint64_t num = dd.num;
  std::vector<size_t> off, len;
  if (const int rc = record_table(compressed, compressed_size, meta_size, num, off, len)) return bail(rc);
  const T norm = (T)hd.norm, tol = (T)hd.tol, s = (T)hd.s;
  const T local_tol = local_abs_tol<T>(hd.rel ? MGH_REL : MGH_ABS, norm, tol, s, num);
  const int nthr = (int)std::min<uint64_t>(num, (uint64_t)ndev);
  MultiErr err;
  std::vector<std::thread> th;
  for (int k = 0; k < nthr; k++)
    th.emplace_back([&, k] {
        try {
      mgh_config c = cfg0;
      c.dev_id = devs[k];
      for (uint64_t id = k; id < num && err.rc == MGH_SUCCESS; id += nthr) {
        // the record as a container of its own: header of the slab (ABS bound) + the record
        const std::vector<uint8_t> meta = fmt::serialize_metadata(slab_header(hd, dd, id, (double)local_tol));
        std::vector<uint8_t> mini(meta.size() + len[id]);
        std::memcpy(mini.data(), meta.data(), meta.size());
        std::memcpy(mini.data() + meta.size(), (const char *)compressed + off[id], len[id]);
        void *dst = (char *)*out + dd.linear_offset(id) * elem;
        const int rc = mgh_decompress(mini.data(), mini.size(), &dst, &c, 1);
        if (rc != MGH_SUCCESS) err.set(rc);
      }
      worker_thread_teardown();
      } catch (const std::exception &e) {
          // (an exception must not leave a worker thread: std::terminate)
          err.set(hl_fail(MGH_ERR_OUT_OF_MEMORY, std::string("worker thread: ") + e.what()));
        }
      });
  for (auto &t : th) t.join();
  if (err.rc != MGH_SUCCESS) {
    mgh_set_last_error_(err.msg.c_str());
    return bail(err.rc);
  }
  return MGH_SUCCESS;
}

// End of a worker thread of the multi-device calls: release the device state AND delete the
// per-thread objects themselves (they are deliberately not destroyed by thread_local destructors --
// HIP calls at process exit -- so a thread that ends has to do it, or every call leaks them).
void worker_thread_teardown() {
  mgh_release_cache();
  delete g_cache_ptr;
  g_cache_ptr = nullptr;
}

int check_devs(int num_dev, const int *dev_ids) {
  if (num_dev < 1 || !dev_ids) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "device list");
  const int have = mgh_device_count();
  if (have <= 0) return hl_fail(MGH_ERR_NO_DEVICE, "no HIP device");
  for (int k = 0; k < num_dev; k++)
    if (dev_ids[k] < 0 || dev_ids[k] >= have) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "device id out of range");
  return MGH_SUCCESS;
}

}  // namespace

extern "C" {

int mgh_compress_multi(int num_dev, const int *dev_ids, int D, int dtype, const uint64_t *shape,
                       double tol, double s, int ebtype, const void *original_data,
                       void **compressed_data, size_t *compressed_size, const void *const *coords,
                       const mgh_config *config, int output_pre_allocated) {
  if (!shape || !original_data || !compressed_data || !compressed_size)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (D < 1 || D > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "D must be 1..5");
  if (dtype != MGH_FLOAT && dtype != MGH_DOUBLE) return hl_fail(MGH_ERR_UNSUPPORTED_DTYPE, "dtype");
  if (ebtype != MGH_REL && ebtype != MGH_ABS) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "error_bound_type");
  if (output_pre_allocated && !*compressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  HL_TRY(check_devs(num_dev, dev_ids));
  HL_TRY(check_config(config));
  // host input -> host container; device-resident input (on any one device) -> container in device
  // memory of that device. A pre-allocated output must be of the same kind.
  if (output_pre_allocated && is_device_pointer(original_data) != is_device_pointer(*compressed_data))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compress_multi: input and pre-allocated output must both be host or both be device memory");
  return hl_guarded([&]() -> int {
    if (dtype == MGH_FLOAT)
      return compress_multi_impl<float>(num_dev, dev_ids, D, dtype, shape, tol, s, ebtype, original_data,
                                        compressed_data, compressed_size, coords, *config,
                                        output_pre_allocated != 0);
    return compress_multi_impl<double>(num_dev, dev_ids, D, dtype, shape, tol, s, ebtype, original_data,
                                       compressed_data, compressed_size, coords, *config,
                                       output_pre_allocated != 0);
  });
}

int mgh_decompress_multi(int num_dev, const int *dev_ids, const void *compressed_data,
                         size_t compressed_size, void **decompressed_data, const mgh_config *config,
                         int output_pre_allocated) {
  if (!compressed_data || !decompressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*decompressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  HL_TRY(check_devs(num_dev, dev_ids));
  mgh_config def;
  if (!config) {
    mgh_config_default(&def);
    config = &def;
  }
  if (is_device_pointer(compressed_data) || (output_pre_allocated && is_device_pointer(*decompressed_data)))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_decompress_multi: host buffers only");
  fmt::Header hd;
  size_t meta_size = 0;
  HL_TRY(read_header(compressed_data, compressed_size, hd, meta_size));
  if (hd.shape.empty() || hd.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "header: dimension");
  if (!hd.quantized) return hl_fail(MGH_ERR_FORMAT, "not a compressed (quantized) stream");
  // slabs of the slowest dimension only; anything else goes through the single-device path
  const bool slabs = hd.dd_method == fmt::DD_MAX_DIMENSION && hd.dd_dim == 0;
  if (!slabs) {
    mgh_config c = *config;
    c.dev_id = dev_ids[0];
    return mgh_decompress(compressed_data, compressed_size, decompressed_data, &c, output_pre_allocated);
  }
  return hl_guarded([&]() -> int {
    if (hd.is_double)
      return decompress_multi_impl<double>(num_dev, dev_ids, hd, meta_size, compressed_data, compressed_size,
                                           decompressed_data, *config, output_pre_allocated != 0);
    return decompress_multi_impl<float>(num_dev, dev_ids, hd, meta_size, compressed_data, compressed_size,
                                        decompressed_data, *config, output_pre_allocated != 0);
  });
}

}  // extern "C"

// ---- one rank per GPU: RCCL ---------------------------------------------------------------------
// The reference's multi-GPU pattern is one MPI rank per GPU, every rank compressing its own block
// (examples/mgard-x/CompressXgcData/TestXGCAbsoluteError.cpp:36-252). Here the ranks' slabs of the
// slowest dimension form ONE domain: the norm a REL bound refers to is reduced over the ranks
// (ncclAllReduce: MAX for s = inf, SUM of squares otherwise -- ErrorToleranceCalculator.hpp:69-131),
// every rank compresses its slab with the ABS bound of calc_local_abs_tol (:134-155), the record
// sizes travel by ncclAllGather and the records by ncclSend / ncclRecv to the root, which writes the
// container mgh_compress would write for this decomposition (GPUPipelines.hpp:189-193). RCCL is
// resolved at first use (dlsym of an RCCL the application already carries, else librccl.so.1), so
// single-GPU users do not link it; the communicator is the caller's.
namespace {
struct RcclApi {
  void *lib = nullptr;
  bool ready = false;
  // (ncclResult_t, ncclDataType_t, ncclRedOp_t are ints; ncclComm_t is a pointer: rccl.h:448-470)
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  int (*Broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  static constexpr int kUint8 = 1, kUint64 = 5, kFloat64 = 8, kSum = 0, kMax = 2;
  bool bind(void *from) {
    auto sym = [&](const char *n) { return dlsym(from, n); };
    AllReduce = reinterpret_cast<decltype(AllReduce)>(sym("ncclAllReduce"));
    AllGather = reinterpret_cast<decltype(AllGather)>(sym("ncclAllGather"));
    Broadcast = reinterpret_cast<decltype(Broadcast)>(sym("ncclBroadcast"));
    Send = reinterpret_cast<decltype(Send)>(sym("ncclSend"));
    Recv = reinterpret_cast<decltype(Recv)>(sym("ncclRecv"));
    GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
    GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
    ready = AllReduce && AllGather && Broadcast && Send && Recv && GroupStart && GroupEnd && GetErrorString;
    return ready;
  }
  bool load(const char *path) {
    static std::mutex m;
    std::lock_guard<std::mutex> lk(m);
    if (path) {  // the library the caller's communicator comes from
      void *l = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
      if (!l) return false;
      lib = l;
      return bind(l);
    }
    if (ready) return true;
    if (bind(RTLD_DEFAULT)) return true;  // the application links RCCL itself
    for (const char *n : {"librccl.so.1", "librccl.so"}) {
      lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (lib && bind(lib)) return true;
    }
    return false;
  }
};
RcclApi g_rccl;

#define HL_NCCL(expr)                                                                            \
  do {                                                                                           \
    const int _r = (expr);                                                                       \
    if (_r != 0) return hl_fail(MGH_ERR_DEVICE, std::string(#expr) + ": " + g_rccl.GetErrorString(_r)); \
  } while (0)

template <typename T>
int compress_dist_impl(void *comm, int rank, int nranks, int root, int D, int dtype, const uint64_t *lshape,
                       double tol_d, double s_d, int ebtype, const void *d_local, void **compressed,
                       size_t *compressed_size, const void *const *coords_in, const mgh_config &cfg, bool prealloc) {
  HL_TRY(cache_prepare(cfg.dev_id));
  hipStream_t st = g_cache.lane[0].st;
  const T tol = (T)tol_d, s = (T)s_d;
  // ---- every rank learns every slab's shape (and that they agree on everything else) ----
  constexpr int kMeta = 8;
  DevBuf dmeta;
  struct Rel { DevBuf &b; ~Rel() { b.release(); } } rel_meta{dmeta};
  HL_TRY(dmeta.ensure((size_t)(nranks + 1) * kMeta * 8));
  uint64_t mine[kMeta] = {(uint64_t)D, (uint64_t)dtype, 0, 0, 0, 0, 0, coords_in ? 1u : 0u};
  for (int d = 0; d < D; d++) mine[2 + d] = lshape[d];
  uint64_t *d_mine = (uint64_t *)dmeta.p, *d_all = d_mine + kMeta;
  HL_HIP(hipMemcpyAsync(d_mine, mine, sizeof mine, hipMemcpyHostToDevice, st));
  HL_NCCL(g_rccl.AllGather(d_mine, d_all, kMeta, RcclApi::kUint64, comm, st));
  std::vector<uint64_t> all((size_t)nranks * kMeta);
  HL_HIP(hipMemcpyAsync(all.data(), d_all, all.size() * 8, hipMemcpyDeviceToHost, st));
  HL_HIP(hipStreamSynchronize(st));
  std::vector<uint64_t> n0(nranks);
  for (int r = 0; r < nranks; r++) {
    const uint64_t *m = &all[(size_t)r * kMeta];
    bool same = m[0] == mine[0] && m[1] == mine[1] && m[7] == mine[7];
    for (int d = 1; d < D; d++) same = same && m[2 + d] == mine[2 + d];
    if (!same) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compress_dist: the ranks disagree on dimension, type or the extents of dimensions 1..");
    n0[r] = m[2];
  }
  if (nranks == 1)  // (nothing to share out: the plain call, like mgh_compress_multi on one slab)
    return mgh_compress(D, dtype, lshape, tol_d, s_d, ebtype, d_local, compressed, compressed_size, coords_in, &cfg,
                        prealloc);
  uint64_t slab = 0;
  if (const char *bad = dist_slab_size(n0, &slab)) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad);
  std::vector<uint64_t> gshape(lshape, lshape + D);  // of the whole domain
  gshape[0] = 0;
  for (uint64_t e : n0) gshape[0] += e;
  // (one slab per rank, nranks >= 2 of them: dist_slab_size saw to it)
  const Decomposer dd = Decomposer::slabs_of_dim0(gshape, slab);
  size_t total = 1, cnt = 1;
  for (int d = 0; d < D; d++) {
    total *= dd.shape[d];
    cnt *= lshape[d];
  }
  // ---- the norm of the whole domain ----
  T norm = 1;
  DevBuf dscal;
  Rel rel_scal{dscal};
  HL_TRY(dscal.ensure(64));
  if (ebtype == MGH_REL) {
    mgh_hierarchy *h = nullptr;
    bool owned = false;
    std::vector<uint64_t> sshape(lshape, lshape + D), off(D, 0);
    HL_TRY(get_hierarchy(&h, &owned, dtype, sshape, nullptr, off, cfg, 0));
    double ln = 0;
    const int rc = mgh_norm(h, d_local, s_d, &ln, st);
    if (owned) mgh_hierarchy_destroy(h);
    HL_TRY(rc);
    NormAccumulator na{s == std::numeric_limits<T>::infinity(), cfg.normalize_coordinates != 0};
    na.add(ln, cnt);  // this rank's contribution; the ranks' are reduced the way add() combines them
    HL_HIP(hipMemcpyAsync(dscal.p, &na.acc, 8, hipMemcpyHostToDevice, st));
    HL_NCCL(g_rccl.AllReduce(dscal.p, (char *)dscal.p + 8, 1, RcclApi::kFloat64, na.inf ? RcclApi::kMax : RcclApi::kSum, comm, st));
    HL_HIP(hipMemcpyAsync(&na.acc, (char *)dscal.p + 8, 8, hipMemcpyDeviceToHost, st));
    HL_HIP(hipStreamSynchronize(st));
    norm = (T)na.result(total);
  }
  const T local_tol = local_abs_tol<T>(ebtype, norm, tol, s, (uint64_t)nranks);
  // ---- this rank's slab as a stand-alone ABS compression; its body is the record ----
  void *part = nullptr;
  size_t part_size = 0;
  mgh_config c = cfg;
  c.domain_decomposition = MGH_DD_MAXDIM;
  HL_TRY(mgh_compress(D, dtype, lshape, (double)local_tol, s_d, MGH_ABS, d_local, &part, &part_size, coords_in, &c, 0));
  struct FreePart { void *p; ~FreePart() { if (p) (void)hipFree(p); } } free_part{part};
  fmt::Header sh;
  size_t ms = 0;
  HL_TRY(read_header(part, part_size, sh, ms));
  if (sh.dd_method != fmt::DD_NOOP) return hl_fail(MGH_ERR_OUT_OF_MEMORY, "mgh_compress_dist: the slab does not fit its device in one piece");
  uint64_t body = part_size - ms;
  HL_HIP(hipMemcpyAsync(d_mine, &body, 8, hipMemcpyHostToDevice, st));
  HL_NCCL(g_rccl.AllGather(d_mine, d_all, 1, RcclApi::kUint64, comm, st));
  std::vector<uint64_t> len(nranks);
  HL_HIP(hipMemcpyAsync(len.data(), d_all, (size_t)nranks * 8, hipMemcpyDeviceToHost, st));
  // coordinates of dimension 0: every rank's slab of them to the root (padded to the slab size)
  std::vector<double> c0;
  if (coords_in) {
    DevBuf dc;
    Rel rel_c{dc};
    HL_TRY(dc.ensure((size_t)(nranks + 1) * slab * 8));
    std::vector<double> my(slab, 0.0);
    for (uint64_t i = 0; i < lshape[0]; i++) my[i] = (double)static_cast<const T *>(coords_in[0])[i];
    HL_HIP(hipMemcpyAsync(dc.p, my.data(), slab * 8, hipMemcpyHostToDevice, st));
    HL_NCCL(g_rccl.AllGather(dc.p, (char *)dc.p + slab * 8, slab, RcclApi::kFloat64, comm, st));
    std::vector<double> allc((size_t)nranks * slab);
    HL_HIP(hipMemcpyAsync(allc.data(), (char *)dc.p + slab * 8, allc.size() * 8, hipMemcpyDeviceToHost, st));
    HL_HIP(hipStreamSynchronize(st));
    for (int r = 0; r < nranks; r++) c0.insert(c0.end(), allc.begin() + (size_t)r * slab, allc.begin() + (size_t)r * slab + n0[r]);
  }
  HL_HIP(hipStreamSynchronize(st));
  if (rank != root) {
    HL_NCCL(g_rccl.Send((const char *)part + ms, body, RcclApi::kUint8, root, comm, st));
    HL_HIP(hipStreamSynchronize(st));
    *compressed_size = 0;
    return MGH_SUCCESS;
  }
  // ---- root: header of the whole domain, then the records in rank order ----
  std::vector<std::vector<double>> coords;
  if (coords_in) {
    coords.resize(D);
    coords[0] = c0;
    for (int d = 1; d < D; d++) {
      const T *cd = static_cast<const T *>(coords_in[d]);
      coords[d].assign(cd, cd + lshape[d]);
    }
  }
  fmt::Header hdr;
  header_from(dd, dtype, ebtype, tol_d, s_d, ebtype == MGH_REL ? (double)norm : 0.0, coords_in ? &coords : nullptr, cfg, hdr);
  const std::vector<uint8_t> meta = fmt::serialize_metadata(hdr);
  size_t need = meta.size();
  for (uint64_t l : len) need += l;
  if (!prealloc) HL_HIP(hipMalloc(compressed, need));
  else if (*compressed_size < need) return hl_fail(MGH_ERR_OUTPUT_TOO_LARGE, "output buffer too small");
  else if (!is_device_pointer(*compressed)) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compress_dist: the container is assembled in device memory");
  char *o = (char *)*compressed;
  auto bail = [&](int rc) {
    if (!prealloc) {
      (void)hipFree(*compressed);
      *compressed = nullptr;
    }
    return rc;
  };
  HL_TRY(g_cache.hpin.ensure(64 + meta.size()));
  std::memcpy((char *)g_cache.hpin.p + 64, meta.data(), meta.size());
  if (hipMemcpyAsync(o, (char *)g_cache.hpin.p + 64, meta.size(), hipMemcpyHostToDevice, st) != hipSuccess)
    return bail(hl_fail(MGH_ERR_DEVICE, "header"));
  size_t at = meta.size();
  int nrc = g_rccl.GroupStart();
  for (int r = 0; r < nranks && nrc == 0; r++) {
    if (r != root) nrc = g_rccl.Recv(o + at, len[r], RcclApi::kUint8, r, comm, st);
    at += len[r];
  }
  if (nrc == 0) nrc = g_rccl.GroupEnd(); else (void)g_rccl.GroupEnd();
  if (nrc != 0) return bail(hl_fail(MGH_ERR_DEVICE, std::string("ncclRecv: ") + g_rccl.GetErrorString(nrc)));
  size_t mine_at = meta.size();
  for (int r = 0; r < root; r++) mine_at += len[r];
  if (hipMemcpyAsync(o + mine_at, (const char *)part + ms, body, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return bail(hl_fail(MGH_ERR_DEVICE, "assembling the container"));
  *compressed_size = at;
  return MGH_SUCCESS;
}

template <typename T>
int decompress_dist_impl(void *comm, int rank, int nranks, int root, fmt::Header &hd, const void *compressed,
                         size_t compressed_size, size_t meta_size, void *d_local_out, const mgh_config &cfg) {
  hipStream_t st = g_cache.lane[0].st;
  Decomposer dd;
  HL_TRY(decomposer_from_header(hd, cfg, dd));
  if (!(hd.dd_method == fmt::DD_MAX_DIMENSION && hd.dd_dim == 0 && dd.num == (uint64_t)nranks))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_decompress_dist: the container is not one slab of dimension 0 per rank");
  // record table from the root
  DevBuf dtab;
  struct Rel { DevBuf &b; ~Rel() { b.release(); } } rel_tab{dtab};
  HL_TRY(dtab.ensure((size_t)nranks * 16));
  std::vector<uint64_t> tab((size_t)nranks * 2, 0);  // offset (of the size prefix), length (prefix included)
  if (rank == root) {
    std::vector<size_t> off, len;
    HL_TRY(record_table(compressed, compressed_size, meta_size, (uint64_t)nranks, off, len));
    for (int r = 0; r < nranks; r++) {
      tab[2 * r] = off[r];
      tab[2 * r + 1] = len[r];
    }
    HL_HIP(hipMemcpyAsync(dtab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
  }
  HL_NCCL(g_rccl.Broadcast(dtab.p, dtab.p, tab.size(), RcclApi::kUint64, root, comm, st));
  HL_HIP(hipMemcpyAsync(tab.data(), dtab.p, tab.size() * 8, hipMemcpyDeviceToHost, st));
  HL_HIP(hipStreamSynchronize(st));
  // this rank's record behind the header of its slab: a container of its own (decompress_multi_impl)
  const T norm = (T)hd.norm, tol = (T)hd.tol, s = (T)hd.s;
  const T local_tol = local_abs_tol<T>(hd.rel ? MGH_REL : MGH_ABS, norm, tol, s, (uint64_t)nranks);
  const std::vector<uint8_t> meta = fmt::serialize_metadata(slab_header(hd, dd, (uint64_t)rank, (double)local_tol));
  const size_t mylen = tab[2 * rank + 1];
  DevBuf mini;
  Rel rel_mini{mini};
  HL_TRY(mini.ensure(meta.size() + mylen));
  HL_TRY(g_cache.hpin.ensure(64 + meta.size()));
  std::memcpy((char *)g_cache.hpin.p + 64, meta.data(), meta.size());
  HL_HIP(hipMemcpyAsync(mini.p, (char *)g_cache.hpin.p + 64, meta.size(), hipMemcpyHostToDevice, st));
  if (rank == root) {
    HL_NCCL(g_rccl.GroupStart());
    int nrc = 0;
    for (int r = 0; r < nranks && nrc == 0; r++)
      if (r != root) nrc = g_rccl.Send((const char *)compressed + tab[2 * r], tab[2 * r + 1], RcclApi::kUint8, r, comm, st);
    const int erc = g_rccl.GroupEnd();
    if (nrc != 0 || erc != 0) return hl_fail(MGH_ERR_DEVICE, std::string("ncclSend: ") + g_rccl.GetErrorString(nrc ? nrc : erc));
    HL_HIP(hipMemcpyAsync((char *)mini.p + meta.size(), (const char *)compressed + tab[2 * rank], mylen, hipMemcpyDeviceToDevice, st));
  } else {
    HL_NCCL(g_rccl.Recv((char *)mini.p + meta.size(), mylen, RcclApi::kUint8, root, comm, st));
  }
  HL_HIP(hipStreamSynchronize(st));
  void *dst = d_local_out;
  return mgh_decompress(mini.p, meta.size() + mylen, &dst, &cfg, 1);
}
}  // namespace

extern "C" {

int mgh_dist_use_library(const char *path) {
  if (!path) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (!g_rccl.load(path)) return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string("mgh_dist_use_library: no RCCL in ") + path);
  return MGH_SUCCESS;
}

int mgh_compress_dist(void *nccl_comm, int rank, int nranks, int root, int D, int dtype, const uint64_t *local_shape,
                      double tol, double s, int ebtype, const void *d_local_data, void **compressed_data,
                      size_t *compressed_size, const void *const *coords, const mgh_config *config,
                      int output_pre_allocated) {
  if (!nccl_comm || !local_shape || !d_local_data || !compressed_size) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (nranks < 1 || rank < 0 || rank >= nranks || root < 0 || root >= nranks) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "rank / nranks / root");
  if (rank == root && (!compressed_data || (output_pre_allocated && !*compressed_data)))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "the root needs an output");
  if (D < 1 || D > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "D must be 1..5");
  if (dtype != MGH_FLOAT && dtype != MGH_DOUBLE) return hl_fail(MGH_ERR_UNSUPPORTED_DTYPE, "dtype");
  if (ebtype != MGH_REL && ebtype != MGH_ABS) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "error_bound_type");
  HL_TRY(check_config(config));
  if (hipSetDevice(config->dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  if (!is_device_pointer_on(d_local_data, config->dev_id))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_compress_dist: the slab must be resident on config->dev_id");
  if (!g_rccl.load(nullptr)) return hl_fail(MGH_ERR_NO_DEVICE, "mgh_compress_dist: no RCCL (librccl.so.1) found");
  size_t dummy = 0;
  void *none = nullptr;
  return hl_guarded([&]() -> int {
    if (dtype == MGH_FLOAT)
      return compress_dist_impl<float>(nccl_comm, rank, nranks, root, D, dtype, local_shape, tol, s, ebtype, d_local_data,
                                       rank == root ? compressed_data : &none, rank == root ? compressed_size : &dummy,
                                       coords, *config, rank == root && output_pre_allocated != 0);
    return compress_dist_impl<double>(nccl_comm, rank, nranks, root, D, dtype, local_shape, tol, s, ebtype, d_local_data,
                                      rank == root ? compressed_data : &none, rank == root ? compressed_size : &dummy,
                                      coords, *config, rank == root && output_pre_allocated != 0);
  });
}

int mgh_decompress_dist(void *nccl_comm, int rank, int nranks, int root, const void *compressed_data,
                        size_t compressed_size, void *d_local_out, const mgh_config *config) {
  if (!nccl_comm || !d_local_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (nranks < 1 || rank < 0 || rank >= nranks || root < 0 || root >= nranks) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "rank / nranks / root");
  if (rank == root && !compressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "the root needs the container");
  mgh_config def;
  if (!config) {
    mgh_config_default(&def);
    config = &def;
  }
  if (hipSetDevice(config->dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  if (!g_rccl.load(nullptr)) return hl_fail(MGH_ERR_NO_DEVICE, "mgh_decompress_dist: no RCCL (librccl.so.1) found");
  HL_TRY(cache_prepare(config->dev_id));
  hipStream_t st = g_cache.lane[0].st;
  return hl_guarded([&]() -> int {
    // the header travels first: its length, then its bytes
    if (nranks > 1 && rank == root && !is_device_pointer_on(compressed_data, config->dev_id))
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_decompress_dist: the container must be resident on the root's device");
    fmt::Header hd;
    size_t meta_size = 0;
    std::vector<uint8_t> hbytes;
    if (rank == root) {
      std::unique_ptr<HostPrefix> prefix;
      if (is_device_pointer(compressed_data)) prefix.reset(new HostPrefix(compressed_data, compressed_size));
      HL_TRY(read_header(compressed_data, compressed_size, hd, meta_size));
      HL_TRY(fetch_host(compressed_data, compressed_size, meta_size, hbytes));
    }
    DevBuf dh;
    struct Rel { DevBuf &b; ~Rel() { b.release(); } } rel{dh};
    HL_TRY(dh.ensure(8));
    uint64_t ms64 = meta_size;
    HL_HIP(hipMemcpyAsync(dh.p, &ms64, 8, hipMemcpyHostToDevice, st));
    HL_NCCL(g_rccl.Broadcast(dh.p, dh.p, 1, RcclApi::kUint64, root, nccl_comm, st));
    HL_HIP(hipMemcpyAsync(&ms64, dh.p, 8, hipMemcpyDeviceToHost, st));
    HL_HIP(hipStreamSynchronize(st));
    if (ms64 == 0 || ms64 > ((uint64_t)1 << 32)) return hl_fail(MGH_ERR_FORMAT, "header size");
    HL_TRY(dh.ensure(ms64));
    hbytes.resize(ms64);
    if (rank == root) HL_HIP(hipMemcpyAsync(dh.p, hbytes.data(), ms64, hipMemcpyHostToDevice, st));
    HL_NCCL(g_rccl.Broadcast(dh.p, dh.p, ms64, RcclApi::kUint8, root, nccl_comm, st));
    HL_HIP(hipMemcpyAsync(hbytes.data(), dh.p, ms64, hipMemcpyDeviceToHost, st));
    HL_HIP(hipStreamSynchronize(st));
    if (rank != root) {
      try {
        meta_size = fmt::parse_metadata(hbytes.data(), hbytes.size(), hd);
      } catch (const std::exception &e) {
        return hl_fail(MGH_ERR_FORMAT, e.what());
      }
    }
    if (nranks == 1) {  // (nothing to hand out: the plain call)
      void *dst = d_local_out;
      return mgh_decompress(compressed_data, compressed_size, &dst, config, 1);
    }
    if (hd.is_double)
      return decompress_dist_impl<double>(nccl_comm, rank, nranks, root, hd, compressed_data, compressed_size, meta_size,
                                          d_local_out, *config);
    return decompress_dist_impl<float>(nccl_comm, rank, nranks, root, hd, compressed_data, compressed_size, meta_size,
                                       d_local_out, *config);
  });
}

}  // extern "C"

extern "C" {

int mgh_infer_shape(const void *data, size_t size, int *D_out, uint64_t *shape_out) {
  if (!data || !D_out || !shape_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  fmt::Header hd;
  size_t ms = 0;
  HL_TRY(read_header(data, size, hd, ms));
  if (hd.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "header: dimension");
  *D_out = (int)hd.shape.size();
  for (size_t d = 0; d < hd.shape.size(); d++) shape_out[d] = hd.shape[d];
  return MGH_SUCCESS;
}

namespace {
int infer_level(const void *data, size_t size, const mgh_config *config, int level, int *L_out,
                std::vector<uint64_t> *shape_out, std::vector<uint64_t> *full_out) {
  if (!data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  mgh_config def;
  if (!config) {
    mgh_config_default(&def);
    config = &def;
  }
  fmt::Header hd;
  size_t ms = 0;
  HL_TRY(read_header(data, size, hd, ms));
  if (full_out) full_out->assign(hd.shape.begin(), hd.shape.end());
  return header_level_shape(hd, *config, level, L_out, shape_out);
}
} // namespace

int mgh_infer_level_shape(const void *data, size_t size, const mgh_config *config, int level, int *D_out,
                          uint64_t *shape_out, int *l_target_out) {
  std::vector<uint64_t> shp;
  int L = 0;
  HL_TRY(infer_level(data, size, config, level, &L, level < 0 ? nullptr : &shp, nullptr));
  if (l_target_out) *l_target_out = L;
  if (level >= 0) {
    if (D_out) *D_out = (int)shp.size();
    if (shape_out) std::copy(shp.begin(), shp.end(), shape_out);
  }
  return MGH_SUCCESS;
}

int mgh_infer_level_nodes(const void *data, size_t size, const mgh_config *config, int level, int dim,
                          uint64_t *h_idx_out, uint64_t cap) {
  std::vector<uint64_t> full;
  int L = 0;
  HL_TRY(infer_level(data, size, config, -1, &L, nullptr, &full));
  if (level < 0) return L;
  if (level > L) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "level outside 0 .. l_target");
  if (dim < 0 || dim >= (int)full.size() || !h_idx_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "dim / NULL argument");
  std::vector<uint64_t> idx;
  mgh::level_nodes(full[dim], L - level, idx);
  if (idx.size() > cap) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_infer_level_nodes: capacity too small");
  std::copy(idx.begin(), idx.end(), h_idx_out);
  return (int)idx.size();
}

namespace {
int infer_coarsened(const void *data, size_t size, const mgh_config *config, int halvings, int nodes_of_dim,
                    StitchedLayout &sl) {
  if (!data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  mgh_config def;
  if (!config) {
    mgh_config_default(&def);
    config = &def;
  }
  fmt::Header hd;
  size_t ms = 0;
  HL_TRY(read_header(data, size, hd, ms));
  if (hd.shape.empty() || hd.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "header: dimension");
  Decomposer dd;
  HL_TRY(decomposer_from_header(hd, *config, dd));
  if (halvings >= 0 && nodes_of_dim != -1 && (nodes_of_dim < 0 || nodes_of_dim >= dd.D))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "dim / NULL argument");
  return hl_plan(stitched_layout(dd, config->max_larget_level, halvings, sl, nodes_of_dim));
}
} // namespace

int mgh_infer_coarsened_shape(const void *data, size_t size, const mgh_config *config, int halvings, int *D_out,
                              uint64_t *shape_out, int *max_halvings_out) {
  StitchedLayout sl;
  HL_TRY(infer_coarsened(data, size, config, halvings, -1, sl));
  if (max_halvings_out) *max_halvings_out = sl.K;
  if (halvings >= 0) {
    if (D_out) *D_out = (int)sl.shape.size();
    if (shape_out) std::copy(sl.shape.begin(), sl.shape.end(), shape_out);
  }
  return MGH_SUCCESS;
}

int mgh_infer_coarsened_nodes(const void *data, size_t size, const mgh_config *config, int halvings, int dim,
                              uint64_t *h_idx_out, uint64_t cap) {
  StitchedLayout sl;
  if (halvings < 0) {
    HL_TRY(infer_coarsened(data, size, config, -1, -1, sl));
    return sl.K;
  }
  if (dim < 0 || !h_idx_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "dim / NULL argument");
  HL_TRY(infer_coarsened(data, size, config, halvings, dim, sl));
  const std::vector<uint64_t> &idx = sl.nodes[dim];
  if (idx.size() > cap) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_infer_coarsened_nodes: capacity too small");
  std::copy(idx.begin(), idx.end(), h_idx_out);
  return (int)idx.size();
}

int mgh_infer_data_type(const void *data, size_t size, int *dtype_out) {
  if (!data || !dtype_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  fmt::Header hd;
  size_t ms = 0;
  HL_TRY(read_header(data, size, hd, ms));
  *dtype_out = hd.is_double ? MGH_DOUBLE : MGH_FLOAT;
  return MGH_SUCCESS;
}

// pin_memory / check_memory_pinned / unpin_memory (compress_x.hpp:166-178; HIP backend:
// MemoryManager<HIP>::HostRegister / CheckHostRegister / HostUnregister, DeviceAdapterHip.h)
int mgh_pin_memory(void *ptr, size_t num_bytes) {
  if (!ptr || !num_bytes) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (is_registered_host(ptr)) return MGH_SUCCESS;  // already pinned
  HL_HIP(hipHostRegister(ptr, num_bytes, hipHostRegisterPortable));
  return MGH_SUCCESS;
}

int mgh_check_memory_pinned(const void *ptr) { return ptr && is_registered_host(ptr) ? 1 : 0; }

int mgh_unpin_memory(void *ptr) {
  if (!ptr) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  HL_HIP(hipHostUnregister(ptr));
  return MGH_SUCCESS;
}

void mgh_free_device(void *p) {
  if (p) (void)hipFree(p);
}

void mgh_release_cache(void) {
  if (g_cache_ptr) g_cache_ptr->release();
  release_host_transfer_state();  // pinned rings, copy threads
  mgh_compare_release_();         // idle scratch buffers of mgh_compare (process-wide)
}

int mgh_memcpy(void *dst, const void *src, size_t bytes) {
  if (!dst || !src) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  HL_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
  return MGH_SUCCESS;
}

int64_t mgh_metadata_serialize(const mgh_header_info *in, uint8_t *out, uint64_t capacity) {
  if (!in || in->D < 1 || in->D > MGH_MAX_DIM) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "header info");
  fmt::Header h;
  for (int i = 0; i < 3; i++) h.version[i] = in->version[i];
  h.is_double = in->dtype == MGH_DOUBLE;
  h.shape.assign(in->shape, in->shape + in->D);
  h.uniform = in->uniform != 0;
  if (!h.uniform)
    for (int d = 0; d < in->D; d++) {
      if (!in->coords[d]) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "coords");
      h.coords.emplace_back(in->coords[d], in->coords[d] + in->shape[d]);
    }
  h.rel = in->error_bound_type == MGH_REL;
  h.tol = in->tol;
  h.s = in->s;
  h.norm = in->norm;
  h.dd_method = !in->domain_decomposed ? fmt::DD_NOOP
                : in->dd_method == MGH_DD_MAXDIM ? fmt::DD_MAX_DIMENSION
                : in->dd_method == MGH_DD_BLOCK ? fmt::DD_BLOCK : fmt::DD_VARIABLE;
  h.dd_dim = in->dd_dim;
  h.dd_size = in->dd_size;
  h.l_target = in->l_target;
  h.reorder = in->reorder != 0;
  h.compressor = in->lossless == MGH_LOSSLESS_HUFFMAN ? fmt::COMP_X_HUFFMAN
                 : in->lossless == MGH_LOSSLESS_HUFFMAN_LZ4 ? fmt::COMP_X_HUFFMAN_LZ4
                 : in->lossless == MGH_LOSSLESS_HUFFMAN_ZSTD ? fmt::COMP_X_HUFFMAN_ZSTD
                 : fmt::COMP_CPU_HUFFMAN_ZSTD;
  h.huff_dict_size = in->lossless == MGH_LOSSLESS_CPU ? 0 : in->huff_dict_size;
  h.huff_block_size = in->lossless == MGH_LOSSLESS_CPU ? 0 : in->huff_block_size;
  const std::vector<uint8_t> b = fmt::serialize_metadata(h);
  if (out) {
    if (capacity < b.size()) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "capacity");
    std::memcpy(out, b.data(), b.size());
  }
  return (int64_t)b.size();
}

int mgh_metadata_parse(const uint8_t *data, uint64_t size, mgh_header_info *out, double *cstore,
                       uint64_t ccap, uint64_t *metadata_size_out) {
  if (!data || !out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  fmt::Header h;
  size_t ms = 0;
  try {
    ms = fmt::parse_metadata(data, size, h);
  } catch (const std::exception &e) {
    return hl_fail(MGH_ERR_FORMAT, e.what());
  }
  if (h.shape.empty() || h.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "header: dimension");
  std::memset(out, 0, sizeof(*out));
  for (int i = 0; i < 3; i++) out->version[i] = h.version[i];
  out->dtype = h.is_double ? MGH_DOUBLE : MGH_FLOAT;
  out->D = (int)h.shape.size();
  for (int d = 0; d < out->D; d++) out->shape[d] = h.shape[d];
  out->uniform = h.uniform ? 1 : 0;
  if (!h.uniform) {
    uint64_t need = 0;
    for (uint64_t n : h.shape) need += n;
    if (!cstore || ccap < need) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "coords_storage too small");
    uint64_t off = 0;
    for (int d = 0; d < out->D; d++) {
      std::memcpy(cstore + off, h.coords[d].data(), h.coords[d].size() * 8);
      out->coords[d] = cstore + off;
      off += h.shape[d];
    }
  }
  out->error_bound_type = h.rel ? MGH_REL : MGH_ABS;
  out->tol = h.tol;
  out->s = h.s;
  out->norm = h.norm;
  out->domain_decomposed = h.dd_method != fmt::DD_NOOP;
  out->dd_method = h.dd_method == fmt::DD_BLOCK ? MGH_DD_BLOCK
                   : h.dd_method == fmt::DD_VARIABLE ? MGH_DD_VARIABLE : MGH_DD_MAXDIM;
  out->dd_dim = h.dd_dim;
  out->dd_size = h.dd_size;
  out->l_target = h.l_target;
  out->reorder = h.reorder ? 1 : 0;
  out->lossless = h.compressor == fmt::COMP_X_HUFFMAN ? MGH_LOSSLESS_HUFFMAN
                  : h.compressor == fmt::COMP_X_HUFFMAN_LZ4 ? MGH_LOSSLESS_HUFFMAN_LZ4
                  : h.compressor == fmt::COMP_X_HUFFMAN_ZSTD ? MGH_LOSSLESS_HUFFMAN_ZSTD : MGH_LOSSLESS_CPU;
  out->huff_dict_size = h.huff_dict_size;
  out->huff_block_size = h.huff_block_size;
  if (metadata_size_out) *metadata_size_out = ms;
  return MGH_SUCCESS;
}

int mgh_huffman_codebook(const uint32_t *freq, uint64_t dict_size, uint64_t *code_out,
                         uint64_t *first_out, uint64_t *entry_out, uint64_t *keys_out) {
  if (!freq || !dict_size || !code_out || !first_out || !entry_out || !keys_out)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  try {
    const huff::Codebook cb = huff::build_codebook(std::vector<unsigned>(freq, freq + dict_size));
    std::memcpy(code_out, cb.code.data(), dict_size * 8);
    std::memcpy(first_out, cb.first.data(), 64 * 8);
    std::memcpy(entry_out, cb.entry.data(), 64 * 8);
    std::memcpy(keys_out, cb.keys.data(), dict_size * 8);
  } catch (const std::exception &e) {
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, e.what());
  }
  return MGH_SUCCESS;
}

int mgh_lossless_create(mgh_lossless_ctx **out, int dev_id) {
  if (!out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = new mgh_lossless_ctx();
  (*out)->dev = dev_id;
  return MGH_SUCCESS;
}

void mgh_lossless_destroy(mgh_lossless_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->dev);
  for (DevBuf *b : {&c->freq, &c->code, &c->bits, &c->entry, &c->total, &c->units, &c->tables, &c->oidx, &c->oval, &c->state, &c->dtable,
                    &c->sync})
    b->release();
  c->pin.release();
  c->dpin.release();
  c->tagpin.release();
  delete c;
}

// mgh_lossless_compress[_sym16]: d_q holds int64 values, or (sym16) uint16_t symbols
static int lossless_compress_to_host(mgh_lossless_ctx *ctx, const void *d_q, bool sym16, uint64_t n, uint64_t dict,
                                     uint64_t chunk, int lossless, int zstd_level, const uint64_t *d_oidx,
                                     const int64_t *d_oval, uint64_t ocount, const uint8_t **payload_out,
                                     uint64_t *size_out, void *stream) {
  if (!ctx || !d_q || !payload_out || !size_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (sym16 && !lossless_sym16_ok(dict, chunk))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless: 16-bit symbols need the single-pass encoder");
  if (hipSetDevice(ctx->dev) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  HL_TRY(hl_guarded([&] {
    return lossless_compress(ctx, (const int64_t *)d_q, n, dict, chunk, lossless, zstd_level, d_oidx, d_oval, ocount,
                             (hipStream_t)stream, nullptr, ~(uint64_t)0, 0, sym16);
  }));
  if (!ctx->on_host) {
    ctx->host.resize(ctx->lay.total);
    HL_TRY(record_write(ctx, ctx->host.data(), (hipStream_t)stream));
    HL_HIP(hipStreamSynchronize((hipStream_t)stream));
  }
  *payload_out = ctx->host.data();
  *size_out = ctx->host.size();
  return MGH_SUCCESS;
}

int mgh_lossless_compress(mgh_lossless_ctx *ctx, const int64_t *d_q, uint64_t n, uint64_t dict,
                          uint64_t chunk, int lossless, int zstd_level, const uint64_t *d_oidx,
                          const int64_t *d_oval, uint64_t ocount, const uint8_t **payload_out,
                          uint64_t *size_out, void *stream) {
  return lossless_compress_to_host(ctx, d_q, false, n, dict, chunk, lossless, zstd_level, d_oidx, d_oval, ocount,
                                   payload_out, size_out, stream);
}

int mgh_lossless_compress_sym16(mgh_lossless_ctx *ctx, const uint16_t *d_symbols, uint64_t n, uint64_t dict,
                                uint64_t chunk, int lossless, int zstd_level, const uint64_t *d_oidx,
                                const int64_t *d_oval, uint64_t ocount, const uint8_t **payload_out,
                                uint64_t *size_out, void *stream) {
  return lossless_compress_to_host(ctx, d_symbols, true, n, dict, chunk, lossless, zstd_level, d_oidx, d_oval, ocount,
                                   payload_out, size_out, stream);
}

// mgh_lossless_compress_device[_sym16]
static int lossless_compress_to_device(mgh_lossless_ctx *ctx, const void *d_q, bool sym16, uint64_t n, uint64_t dict,
                                       uint64_t chunk, const uint64_t *d_oidx, const int64_t *d_oval,
                                       uint64_t ocount, void *d_record_out, uint64_t capacity, uint64_t *size_out,
                                       void *stream) {
  if (!ctx || !d_q || !d_record_out || !size_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (sym16 && !lossless_sym16_ok(dict, chunk))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "lossless: 16-bit symbols need the single-pass encoder");
  if (hipSetDevice(ctx->dev) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  if (!is_device_pointer(d_record_out)) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "d_record_out must be device memory");
  HL_TRY(hl_guarded([&] {
    return lossless_compress(ctx, (const int64_t *)d_q, n, dict, chunk, MGH_LOSSLESS_HUFFMAN, 0, d_oidx, d_oval, ocount,
                             (hipStream_t)stream, nullptr, ~(uint64_t)0, 0, sym16, (uint8_t *)d_record_out,
                             (size_t)capacity);
  }));
  if (ctx->overflow || ctx->record_size() > capacity)
    return hl_fail(MGH_ERR_OUTPUT_TOO_LARGE, "record does not fit the buffer");
  HL_TRY(record_write(ctx, d_record_out, (hipStream_t)stream));
  HL_HIP(hipStreamSynchronize((hipStream_t)stream));
  *size_out = ctx->record_size();
  return MGH_SUCCESS;
}

int mgh_lossless_compress_device(mgh_lossless_ctx *ctx, const int64_t *d_q, uint64_t n, uint64_t dict,
                                 uint64_t chunk, const uint64_t *d_oidx, const int64_t *d_oval,
                                 uint64_t ocount, void *d_record_out, uint64_t capacity, uint64_t *size_out,
                                 void *stream) {
  return lossless_compress_to_device(ctx, d_q, false, n, dict, chunk, d_oidx, d_oval, ocount, d_record_out, capacity,
                                     size_out, stream);
}

int mgh_lossless_compress_device_sym16(mgh_lossless_ctx *ctx, const uint16_t *d_symbols, uint64_t n, uint64_t dict,
                                       uint64_t chunk, const uint64_t *d_oidx, const int64_t *d_oval,
                                       uint64_t ocount, void *d_record_out, uint64_t capacity, uint64_t *size_out,
                                       void *stream) {
  return lossless_compress_to_device(ctx, d_symbols, true, n, dict, chunk, d_oidx, d_oval, ocount, d_record_out,
                                     capacity, size_out, stream);
}

int mgh_lossless_decompress(mgh_lossless_ctx *ctx, const uint8_t *payload, uint64_t size, int lossless,
                            int64_t *d_q, uint64_t n, const uint64_t **oidx_out,
                            const int64_t **oval_out, uint64_t *ocount_out, void *stream) {
  if (!ctx || !payload || !d_q || !ocount_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (hipSetDevice(ctx->dev) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  HL_TRY(hl_guarded([&] { return lossless_decompress(ctx, payload, size, lossless, d_q, n, ocount_out, (hipStream_t)stream); }));
  if (oidx_out) *oidx_out = (const uint64_t *)ctx->oidx.p;
  if (oval_out) *oval_out = (const int64_t *)ctx->oval.p;
  return MGH_SUCCESS;
}

int mgh_lossless_decompress_prefix(mgh_lossless_ctx *ctx, const uint8_t *payload, uint64_t size, int lossless,
                                   int64_t *d_q, uint64_t n, uint64_t n_prefix, const uint64_t **oidx_out,
                                   const int64_t **oval_out, uint64_t *ocount_out, void *stream) {
  if (!ctx || !payload || !d_q || !ocount_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (n_prefix == 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_lossless_decompress_prefix: n_prefix is 0");
  if (hipSetDevice(ctx->dev) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  HL_TRY(hl_guarded([&] {
    return lossless_decompress(ctx, payload, size, lossless, d_q, n, ocount_out, (hipStream_t)stream, nullptr, true,
                               DecodeRange{n_prefix});
  }));
  if (oidx_out) *oidx_out = (const uint64_t *)ctx->oidx.p;
  if (oval_out) *oval_out = (const int64_t *)ctx->oval.p;
  return MGH_SUCCESS;
}

int mgh_lossless_decompress_range(mgh_lossless_ctx *ctx, const uint8_t *payload, uint64_t size, int lossless,
                                  int64_t *d_q, uint64_t n, uint64_t first, uint64_t count, const uint64_t **oidx_out,
                                  const int64_t **oval_out, uint64_t *ocount_out, void *stream) {
  if (!ctx || !payload || !d_q || !ocount_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (count == 0 || first >= n || count > n - first)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_lossless_decompress_range: first / count outside the record");
  if (hipSetDevice(ctx->dev) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  HL_TRY(hl_guarded([&] {
    return lossless_decompress(ctx, payload, size, lossless, d_q, n, ocount_out, (hipStream_t)stream, nullptr, true,
                               DecodeRange{first + count, ~(uint64_t)0, first});
  }));
  if (oidx_out) *oidx_out = (const uint64_t *)ctx->oidx.p;
  if (oval_out) *oval_out = (const int64_t *)ctx->oval.p;
  return MGH_SUCCESS;
}

int mgh_lossless_decompress_sym16(mgh_lossless_ctx *ctx, const uint8_t *payload, uint64_t size, int lossless,
                                  uint16_t *d_symbols, uint64_t n, uint64_t first, uint64_t count,
                                  const uint64_t **oidx_out, const int64_t **oval_out, uint64_t *ocount_out,
                                  void *stream) {
  if (!ctx || !payload || !d_symbols || !ocount_out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (count == 0 || first >= n || count > n - first)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_lossless_decompress_sym16: first / count outside the record");
  if (hipSetDevice(ctx->dev) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  const DecodeRange range = first == 0 && count == n ? DecodeRange() : DecodeRange{first + count, ~(uint64_t)0, first};
  HL_TRY(hl_guarded([&] {
    bool sym16 = true;
    return lossless_decompress(ctx, payload, size, lossless, (int64_t *)d_symbols, n, ocount_out, (hipStream_t)stream,
                               &sym16, true, range, /*require16=*/true);
  }));
  if (oidx_out) *oidx_out = (const uint64_t *)ctx->oidx.p;
  if (oval_out) *oval_out = (const int64_t *)ctx->oval.p;
  return MGH_SUCCESS;
}

int mgh_infer_level_range(const void *data, size_t size, const mgh_config *config, int level, uint64_t *first_elem,
                          uint64_t *num_elems, uint64_t *first_chunk, uint64_t *num_chunks) {
  if (!data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  mgh_config def;
  if (!config) {
    mgh_config_default(&def);
    config = &def;
  }
  fmt::Header hd;
  size_t ms = 0;
  HL_TRY(read_header(data, size, hd, ms));
  std::vector<uint64_t> shp;
  HL_TRY(header_level_shape(hd, *config, level, nullptr, &shp));
  uint64_t hi = 1, lo = 0;
  for (uint64_t e : shp) hi *= e;
  if (level > 0) {
    HL_TRY(header_level_shape(hd, *config, level - 1, nullptr, &shp));
    lo = 1;
    for (uint64_t e : shp) lo *= e;
  }
  const uint64_t block = std::max<uint64_t>(hd.huff_block_size, 1);
  if (first_elem) *first_elem = lo;
  if (num_elems) *num_elems = hi - lo;
  if (first_chunk) *first_chunk = lo / block;
  if (num_chunks) *num_chunks = (hi - 1) / block - lo / block + 1;
  return MGH_SUCCESS;
}

}  // extern "C"

// ---- progressive reader: a reduced-resolution reconstruction refined level by level -----------------
// State between the calls: the dense nodal array of the current level (what the next level step
// reads), the integers decoded but not used yet (the tail of the boundary chunk), and a lossless
// context that keeps the record's head, decode tables, chunk table and outlier lists on the device.
struct mgh_progressive {
  fmt::Header hd;
  mgh_config cfg;
  RecordView rv;  // the record inside the caller's container (borrowed)
  RecordQuant qp{};
  bool in_dev = false;
  int dtype = MGH_FLOAT;
  size_t elem = 4;
  uint64_t n = 0, block = 1, nchunk = 0, ocount = 0;
  int L = 0, level = -1;
  std::vector<uint64_t> N;  // N[l] = prod(level_shape(l))
  mgh_hierarchy *h = nullptr;
  mgh_lossless_ctx *ll = nullptr;
  hipStream_t st = nullptr;
  DevBuf q[2];             // q[qi]: integers [q_first, dec_end) of the level-linearised array
  int qi = 0;
  uint64_t q_first = 0, dec_end = 0;
  DevBuf state[2];         // state[si]: the dense array of `level`
  int si = 0;
  DevBuf lin;              // a raw record: all its level-linearised integers (made at open)
  DevBuf full;             // mgh_progressive_preview into host memory: the full-grid array on its way out
  DevBuf win;              // mgh_progressive_preview_window into host memory: the window on its way out
};

namespace {
void progressive_free(mgh_progressive *p) {
  if (!p) return;
  (void)hipSetDevice(p->cfg.dev_id);
  if (p->st) (void)hipStreamSynchronize(p->st);
  for (DevBuf *b : {&p->q[0], &p->q[1], &p->state[0], &p->state[1], &p->lin, &p->full, &p->win}) b->release();
  if (p->h) mgh_hierarchy_destroy(p->h);
  if (p->ll) mgh_lossless_destroy(p->ll);
  if (p->st) (void)hipStreamDestroy(p->st);
  delete p;
}

int progressive_open(mgh_progressive *p, const void *data, size_t size) {
  std::unique_ptr<HostPrefix> prefix;
  p->in_dev = is_device_pointer(data);
  if (p->in_dev) prefix.reset(new HostPrefix(data, size));
  size_t meta_size = 0;
  fmt::Header &hd = p->hd;
  HL_TRY(read_header(data, size, hd, meta_size));
  if (hd.shape.empty() || hd.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "header: dimension");
  if (!hd.quantized) return hl_fail(MGH_ERR_FORMAT, "not a compressed (quantized) stream");
  HL_TRY(header_level_shape(hd, p->cfg, -1, &p->L, nullptr));  // (refuses a decomposed container)
  HL_TRY(record_view_header(hd, p->rv));
  if (!hd.reorder)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT,
                   "mgh_progressive_open: a reorder = 1 (level-linearised) container is needed: the levels of a "
                   "reorder = 0 record are spread over every Huffman chunk");
  p->dtype = hd.is_double ? MGH_DOUBLE : MGH_FLOAT;
  p->elem = hd.is_double ? 8 : 4;
  auto in_type = [&](double v) { return hd.is_double ? v : (double)(float)v; };
  p->qp = RecordQuant{hd.rel ? MGH_REL : MGH_ABS, in_type(hd.tol), in_type(hd.s), in_type(hd.norm), hd.huff_dict_size, true};
  p->block = std::max<uint64_t>(hd.huff_block_size, 1);
  p->N.resize(p->L + 1);
  for (int l = 0; l <= p->L; l++) {
    std::vector<uint64_t> shp;
    HL_TRY(header_level_shape(hd, p->cfg, l, nullptr, &shp));
    p->N[l] = 1;
    for (uint64_t e : shp) p->N[l] *= e;
  }
  p->n = p->N[p->L];
  HL_TRY(record_view_at(data, size, meta_size, p->n * p->elem, p->rv));  // the one record
  // hierarchy of the array (its own: it holds the state of the level loop between the calls)
  std::vector<std::vector<double>> mirrored;
  bool owned = true;
  HL_TRY(get_hierarchy(&p->h, &owned, p->dtype, hd.shape, decoder_coords(hd, p->cfg, mirrored),
                       std::vector<uint64_t>(hd.shape.size(), 0), p->cfg, 0, /*cached=*/false));
  if (mgh_l_target(p->h) != p->L) return hl_fail(MGH_ERR_FORMAT, "header: the hierarchy of the subdomain is not the header's");
  HL_HIP(hipStreamCreate(&p->st));
  if (p->rv.raw) {
    // the integers a Huffman record of this array would have held, level-linearised: the route of
    // mgh_decompress_level, once
    if (p->L == 0) return MGH_SUCCESS;
    DevBuf data_in, qfull;
    int rc = p->lin.ensure(p->n * 8);
    if (rc == MGH_SUCCESS) rc = raw_record_integers(p->h, p->rv, p->qp, data_in, qfull, p->n, p->st);
    if (rc == MGH_SUCCESS)
      rc = mgh_level_linearize(p->h, (const int64_t *)qfull.p, (int64_t *)p->lin.p, 0, nullptr, nullptr, 0, 0, p->st);
    (void)hipStreamSynchronize(p->st);
    data_in.release();
    qfull.release();
    return rc;
  }
  // head parsed and validated, decode tables, chunk table and outlier lists uploaded, a Zstd frame
  // inflated -- once
  HL_TRY(mgh_lossless_create(&p->ll, p->cfg.dev_id));
  p->ll->keep = 1;
  decompress_stats() = mgh_decompress_stats{};
  HL_TRY(lossless_decompress(p->ll, p->rv.rec, p->rv.csize, p->rv.lossless, nullptr, p->n, &p->ocount, p->st, nullptr,
                             /*sync_end=*/true, DecodeRange{/*n_prefix=*/0}));
  p->nchunk = decompress_stats().chunks_total;
  return MGH_SUCCESS;
}

int progressive_refine(mgh_progressive *p, int to, void **out, bool prealloc) {
  const fmt::Header &hd = p->hd;
  mgh_decompress_stats &stats = decompress_stats();
  stats = mgh_decompress_stats{};
  stats.subdomains = 1;
  const int from = p->level;
  hipStream_t st = p->st;
  const uint64_t dict = hd.huff_dict_size;
  const size_t out_bytes = p->N[to] * p->elem;
  int at = p->si;
  const bool raw_full = p->rv.raw && to == p->L;  // (a raw record IS the finest level)
  if (raw_full) stats.record_bytes = p->rv.csize;
  if (!raw_full) {
    const int64_t *base = nullptr;  // integer `first` of the array
    uint64_t first = 0;
    const uint64_t *oidx = nullptr;
    const int64_t *oval = nullptr;
    if (p->rv.raw) {
      stats.record_bytes = p->rv.csize;
      base = (const int64_t *)p->lin.p;
    } else {
      // the integers [N_from, N_to): what is left of the boundary chunk, and the chunks not decoded yet
      const uint64_t lo = from < 0 ? 0 : p->N[from];
      const uint64_t carry = p->dec_end > lo ? p->dec_end - lo : 0;
      const uint64_t new_end = std::max(p->dec_end, std::min(p->n, ((p->N[to] - 1) / p->block + 1) * p->block));
      DevBuf &qn = p->q[p->qi ^ 1];
      HL_TRY(qn.ensure(std::max<uint64_t>(carry + (new_end - p->dec_end), 1) * 8));
      if (carry)
        HL_HIP(hipMemcpyAsync(qn.p, (const int64_t *)p->q[p->qi].p + (lo - p->q_first), carry * 8, hipMemcpyDeviceToDevice, st));
      if (new_end > p->dec_end) {
        HL_TRY(lossless_decompress(p->ll, p->rv.rec, p->rv.csize, p->rv.lossless, (int64_t *)qn.p + carry, p->n, &p->ocount, st,
                                   nullptr, /*sync_end=*/false,
                                   DecodeRange{/*n_prefix=*/new_end, /*q_cap=*/new_end - p->dec_end, /*first=*/p->dec_end}));
      } else {  // (everything this refine reads was decoded with the boundary chunk of an earlier one)
        stats.chunks_total = p->nchunk;
        stats.record_bytes = p->rv.csize;
      }
      p->qi ^= 1;
      p->q_first = lo;
      p->dec_end = new_end;
      base = (const int64_t *)qn.p;
      first = lo;
      oidx = (const uint64_t *)p->ll->oidx.p;
      oval = (const int64_t *)p->ll->oval.p;
    }
    const int prep = p->rv.raw ? 0 : 1;
    const uint64_t ocount = p->rv.raw ? 0 : p->ocount;
    int l = from;
    if (from < 0) {
      HL_TRY(p->state[at].ensure(out_bytes));
      HL_TRY(mgh_dequantize_recompose_linear_to_level(p->h, (int64_t *)base, p->qp.eb, p->qp.tol, p->qp.s, p->qp.norm, dict, prep, oidx,
                                                      oval, ocount, to, p->state[at].p, st));
      l = to;
    }
    for (l = l + 1; l <= to; l++) {
      HL_TRY(p->state[at ^ 1].ensure(p->N[l] * p->elem));
      HL_TRY(mgh_refine_level(p->h, p->state[at].p, (int64_t *)base + (p->N[l - 1] - first), p->qp.eb, p->qp.tol, p->qp.s, p->qp.norm,
                              dict, prep, oidx, oval, ocount, l, p->state[at ^ 1].p, st));
      at ^= 1;
    }
  }
  // the array of to_level out, in the container's memory space
  const OutSlot slot{out, p->in_dev, prealloc};
  HL_TRY(slot.alloc(out_bytes));
  int rc = raw_full ? copy_any(*out, p->rv.rec, out_bytes, st) : copy_any(*out, p->state[at].p, out_bytes, st);
  if (rc == MGH_SUCCESS && hipStreamSynchronize(st) != hipSuccess) rc = hl_fail(MGH_ERR_DEVICE, "sync");
  if (rc == MGH_SUCCESS && p->ll) rc = lossless_tag_check(p->ll);
  if (rc == MGH_SUCCESS) {
    p->si = at;
    p->level = to;
  }
  return slot.fail(rc);
}

// The current level prolonged to the full grid; reads the state, changes none of it (the level
// buffers of the hierarchy it passes through are scratch between the calls).
int progressive_preview(mgh_progressive *p, void **out, bool prealloc) {
  hipStream_t st = p->st;
  const size_t out_bytes = p->n * p->elem;
  const bool raw_full = p->rv.raw && p->level == p->L;  // (a raw record IS the finest level: no state)
  const OutSlot slot{out, p->in_dev, prealloc};
  HL_TRY(slot.alloc(out_bytes));
  int rc = MGH_SUCCESS;
  if (raw_full) {
    rc = copy_any(*out, p->rv.rec, out_bytes, st);
  } else if (is_device_pointer(*out)) {
    rc = mgh_prolong(p->h, p->level, p->state[p->si].p, *out, st);
  } else {
    rc = p->full.ensure(out_bytes);
    if (rc == MGH_SUCCESS) rc = mgh_prolong(p->h, p->level, p->state[p->si].p, p->full.p, st);
    if (rc == MGH_SUCCESS) rc = copy_any(*out, p->full.p, out_bytes, st);
  }
  if (rc == MGH_SUCCESS && hipStreamSynchronize(st) != hipSuccess) rc = hl_fail(MGH_ERR_DEVICE, "sync");
  return slot.fail(rc);
}

// ... a window of it (mgh_prolong_window): the same reading of the state, window-sized work on the
// fused 3-D route.
int progressive_preview_window(mgh_progressive *p, const uint64_t *lo, const uint64_t *ext, void **out, bool prealloc) {
  hipStream_t st = p->st;
  size_t out_bytes = p->elem;
  for (size_t d = 0; d < p->hd.shape.size(); d++) {
    if (ext[d] == 0 || lo[d] > p->hd.shape[d] || ext[d] > p->hd.shape[d] - lo[d])
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, "the window leaves the array");
    out_bytes *= ext[d];
  }
  const bool raw_full = p->rv.raw && p->level == p->L;  // (a raw record IS the finest level: no state)
  const OutSlot slot{out, p->in_dev, prealloc};
  HL_TRY(slot.alloc(out_bytes));
  int rc = MGH_SUCCESS;
  const void *lvl = p->state[p->si].p;
  if (raw_full && is_device_pointer(p->rv.rec)) {
    lvl = p->rv.rec;
  } else if (raw_full) {
    rc = p->full.ensure(p->n * p->elem);
    if (rc == MGH_SUCCESS) rc = copy_any(p->full.p, p->rv.rec, p->n * p->elem, st);
    lvl = p->full.p;
  }
  const bool out_dev = is_device_pointer(*out);
  if (rc == MGH_SUCCESS && !out_dev) rc = p->win.ensure(out_bytes);
  if (rc == MGH_SUCCESS) rc = mgh_prolong_window(p->h, p->level, lvl, lo, ext, out_dev ? *out : p->win.p, st);
  if (rc == MGH_SUCCESS && !out_dev) rc = copy_any(*out, p->win.p, out_bytes, st);
  if (rc == MGH_SUCCESS && hipStreamSynchronize(st) != hipSuccess) rc = hl_fail(MGH_ERR_DEVICE, "sync");
  return slot.fail(rc);
}
}  // namespace

extern "C" {

int mgh_progressive_open(mgh_progressive **out, const void *compressed_data, size_t compressed_size,
                         const mgh_config *config) {
  if (!out || !compressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = nullptr;
  {
    const std::string bad = env_validate();
    if (!bad.empty()) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad);
  }
  mgh_config def;
  if (!config) {
    mgh_config_default(&def);
    config = &def;
  }
  if (mgh_device_count() <= 0) return hl_fail(MGH_ERR_NO_DEVICE, "no HIP device");
  if (hipSetDevice(config->dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  mgh_progressive *p = new mgh_progressive();
  p->cfg = *config;
  const int rc = hl_guarded([&] { return progressive_open(p, compressed_data, compressed_size); });
  if (rc != MGH_SUCCESS) {
    progressive_free(p);
    return rc;
  }
  *out = p;
  return MGH_SUCCESS;
}

int mgh_progressive_level(const mgh_progressive *p) { return p ? p->level : -1; }

int mgh_progressive_refine(mgh_progressive *p, int to_level, void **data, int output_pre_allocated) {
  if (!p || !data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  if (to_level < 0 || to_level > p->L) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "level outside 0 .. l_target");
  if (to_level <= p->level)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_progressive_refine: to_level must be above the current level");
  if (hipSetDevice(p->cfg.dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return hl_guarded([&] { return progressive_refine(p, to_level, data, output_pre_allocated != 0); });
}

int mgh_progressive_preview(mgh_progressive *p, void **data, int output_pre_allocated) {
  if (!p || !data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  if (p->level < 0)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_progressive_preview: nothing refined yet (call mgh_progressive_refine first)");
  if (hipSetDevice(p->cfg.dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return hl_guarded([&] { return progressive_preview(p, data, output_pre_allocated != 0); });
}

int mgh_progressive_preview_window(mgh_progressive *p, const uint64_t *lo, const uint64_t *ext, void **data,
                                   int output_pre_allocated) {
  if (!p || !data || !lo || !ext) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  if (p->level < 0)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT,
                   "mgh_progressive_preview_window: nothing refined yet (call mgh_progressive_refine first)");
  if (hipSetDevice(p->cfg.dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return hl_guarded([&] { return progressive_preview_window(p, lo, ext, data, output_pre_allocated != 0); });
}

void mgh_progressive_close(mgh_progressive *p) { progressive_free(p); }

int mgh_last_decompress_stats(mgh_decompress_stats *out) {
  if (!out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = decompress_stats();
  return MGH_SUCCESS;
}

} // extern "C"

// ---- precision layers, the reader: containers of mgh_compress_layers added up in the coefficients ------
// State between the calls: the accumulator -- the coefficients of the array as the layers added so far
// give them -- on the device, and the header of layer 0, which every later layer has to agree with. A
// layer costs a decode and one stream over the accumulator (mgh_dequantize_add); the recomposition runs
// when the data is asked for, on a copy (mgh_recompose is not in place here: the accumulator stays).
struct mgh_layers {
  fmt::Header hd;  // of layer 0
  mgh_config cfg;
  bool in_dev = false;
  int dtype = MGH_FLOAT;
  size_t elem = 4;
  uint64_t n = 0;
  int count = 0;
  double tol = 0;  // of the last layer added
  mgh_hierarchy *h = nullptr;
  mgh_lossless_ctx *ll = nullptr;
  hipStream_t st = nullptr;
  DevBuf acc;  // n elements: the coefficients
  DevBuf q;    // n int64: the integers of the layer being added
  DevBuf out;  // n elements: the recomposed array on its way to host memory
};

namespace {
void layers_free(mgh_layers *p) {
  if (!p) return;
  (void)hipSetDevice(p->cfg.dev_id);
  if (p->st) (void)hipStreamSynchronize(p->st);
  for (DevBuf *b : {&p->acc, &p->q, &p->out}) b->release();
  if (p->h) mgh_hierarchy_destroy(p->h);
  if (p->ll) mgh_lossless_destroy(p->ll);
  if (p->st) (void)hipStreamDestroy(p->st);
  delete p;
}

// What a later layer must share with layer 0 to be a layer of the same array.
const char *layers_mismatch(const fmt::Header &a, const fmt::Header &b) {
  if (a.shape != b.shape) return "the shape";
  if (a.is_double != b.is_double) return "the data type";
  if (a.uniform != b.uniform || (!a.uniform && a.coords != b.coords)) return "the coordinates";
  if (a.rel != b.rel) return "the error bound type";
  if (!(a.s == b.s)) return "s";
  if (!(a.norm == b.norm)) return "the norm";
  if (a.dd_method != b.dd_method || a.hierarchy != b.hierarchy) return "the decomposition";
  return nullptr;
}

// One container into the accumulator: layer 0 (p->count == 0) opens it, every other one is added. Every
// refusal comes before the accumulator is touched.
int layers_add(mgh_layers *p, const void *data, size_t size) {
  const bool first = p->count == 0;
  const char *who = first ? "mgh_layers_open" : "mgh_layers_add";
  std::unique_ptr<HostPrefix> prefix;
  const bool in_dev = is_device_pointer(data);
  if (in_dev) prefix.reset(new HostPrefix(data, size));
  size_t meta_size = 0;
  fmt::Header hd;
  HL_TRY(read_header(data, size, hd, meta_size));
  if (hd.shape.empty() || hd.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "header: dimension");
  if (!hd.quantized) return hl_fail(MGH_ERR_FORMAT, "not a compressed (quantized) stream");
  RecordView rv;
  HL_TRY(record_view_header(hd, rv));
  if (hd.dd_method != fmt::DD_NOOP)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + ": the container is domain-decomposed (layers have one subdomain)");
  if (hd.reorder) return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + ": a reorder = 1 container is no layer");
  for (uint64_t e : hd.shape)
    if (e < 3) return hl_fail(MGH_ERR_FORMAT, "header: extent below 3");
  if (!first) {
    if (const char *what = layers_mismatch(p->hd, hd))
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + ": " + what + " is not layer 0's");
    if (!(hd.tol < p->tol))
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + ": the tolerance is not below the last layer's");
  }
  uint64_t n = 1;
  for (uint64_t e : hd.shape) n *= e;
  const size_t elem = hd.is_double ? 8 : 4;
  HL_TRY(record_view_at(data, size, meta_size, n * elem, rv));
  if (rv.raw) return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + ": the record is stored raw (no layer is)");
  if (first) {
    p->hd = hd;
    p->in_dev = in_dev;
    p->dtype = hd.is_double ? MGH_DOUBLE : MGH_FLOAT;
    p->elem = elem;
    p->n = n;
    std::vector<std::vector<double>> mirrored;
    bool owned = true;
    HL_TRY(get_hierarchy(&p->h, &owned, p->dtype, hd.shape, decoder_coords(hd, p->cfg, mirrored),
                         std::vector<uint64_t>(hd.shape.size(), 0), p->cfg, 0, /*cached=*/false));
    HL_HIP(hipStreamCreate(&p->st));
    HL_TRY(mgh_lossless_create(&p->ll, p->cfg.dev_id));
    HL_TRY(p->acc.ensure(n * elem));
    HL_TRY(p->q.ensure(n * 8));
    decompress_stats() = mgh_decompress_stats{};
  }
  auto in_type = [&](double v) { return hd.is_double ? v : (double)(float)v; };
  uint64_t ocount = 0;
  int rc = lossless_decompress(p->ll, rv.rec, rv.csize, rv.lossless, (int64_t *)p->q.p, n, &ocount, p->st);
  if (rc != MGH_SUCCESS) {
    (void)hipStreamSynchronize(p->st);
    return rc;
  }
  rc = mgh_dequantize_add(p->h, (int64_t *)p->q.p, hd.rel ? MGH_REL : MGH_ABS, in_type(hd.tol), in_type(hd.s),
                          in_type(hd.norm), hd.huff_dict_size, 1, (const uint64_t *)p->ll->oidx.p,
                          (const int64_t *)p->ll->oval.p, ocount, first ? 1 : 0, p->acc.p, p->st);
  if (hipStreamSynchronize(p->st) != hipSuccess && rc == MGH_SUCCESS) rc = hl_fail(MGH_ERR_DEVICE, "sync");
  HL_TRY(rc);
  p->count++;
  p->tol = hd.tol;
  return MGH_SUCCESS;
}

// mgh_recompose of the accumulator into an array in the containers' memory space (or the caller's buffer).
// level >= 0 (mgh_layers_data_level): mgh_recompose_to_level, the dense array of that level -- the whole
// accumulator is there either way, the call reads its corner box.
int layers_data(mgh_layers *p, void **out, bool prealloc, int level = -1) {
  hipStream_t st = p->st;
  size_t out_bytes = p->n * p->elem;
  if (level >= 0) {
    uint64_t shp[MGH_MAX_DIM];
    HL_TRY(mgh_level_shape(p->h, level, shp));
    out_bytes = p->elem;
    for (size_t d = 0; d < p->hd.shape.size(); d++) out_bytes *= shp[d];
  }
  auto recompose = [&](void *dst) {
    return level >= 0 ? mgh_recompose_to_level(p->h, p->acc.p, level, dst, st) : mgh_recompose(p->h, p->acc.p, dst, st);
  };
  const OutSlot slot{out, p->in_dev, prealloc};
  HL_TRY(slot.alloc(out_bytes));
  int rc = MGH_SUCCESS;
  if (is_device_pointer(*out)) {
    rc = recompose(*out);
  } else {
    rc = p->out.ensure(out_bytes);
    if (rc == MGH_SUCCESS) rc = recompose(p->out.p);
    if (rc == MGH_SUCCESS) rc = copy_any(*out, p->out.p, out_bytes, st);
  }
  if (hipStreamSynchronize(st) != hipSuccess && rc == MGH_SUCCESS) rc = hl_fail(MGH_ERR_DEVICE, "sync");
  return slot.fail(rc);
}
}  // namespace

extern "C" {

int mgh_layers_open(mgh_layers **out, const void *compressed_data, size_t compressed_size, const mgh_config *config) {
  if (!out || !compressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = nullptr;
  {
    const std::string bad = env_validate();
    if (!bad.empty()) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad);
  }
  mgh_config def;
  if (!config) {
    mgh_config_default(&def);
    config = &def;
  }
  if (mgh_device_count() <= 0) return hl_fail(MGH_ERR_NO_DEVICE, "no HIP device");
  if (hipSetDevice(config->dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  mgh_layers *p = new mgh_layers();
  p->cfg = *config;
  const int rc = hl_guarded([&] { return layers_add(p, compressed_data, compressed_size); });
  if (rc != MGH_SUCCESS) {
    layers_free(p);
    return rc;
  }
  *out = p;
  return MGH_SUCCESS;
}

int mgh_layers_add(mgh_layers *p, const void *compressed_data, size_t compressed_size) {
  if (!p || !compressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (hipSetDevice(p->cfg.dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return hl_guarded([&] { return layers_add(p, compressed_data, compressed_size); });
}

int mgh_layers_count(const mgh_layers *p) { return p ? p->count : -1; }

double mgh_layers_tolerance(const mgh_layers *p) { return p ? p->tol : 0.0; }

int mgh_layers_data(mgh_layers *p, void **data, int output_pre_allocated) {
  if (!p || !data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  if (hipSetDevice(p->cfg.dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return hl_guarded([&] { return layers_data(p, data, output_pre_allocated != 0); });
}

void mgh_layers_close(mgh_layers *p) { layers_free(p); }

int mgh_decompress_layers(int nlayers, const void *const *compressed_data, const size_t *compressed_size,
                          const mgh_config *config, void **decompressed_data, int output_pre_allocated) {
  if (!compressed_data || !compressed_size || !decompressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (nlayers < 1 || nlayers > kLadderMaxTols) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "decompress_layers: nlayers must be in 1..64");
  for (int k = 0; k < nlayers; k++)
    if (!compressed_data[k]) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*decompressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  mgh_layers *p = nullptr;
  int rc = mgh_layers_open(&p, compressed_data[0], compressed_size[0], config);
  for (int k = 1; k < nlayers && rc == MGH_SUCCESS; k++) rc = mgh_layers_add(p, compressed_data[k], compressed_size[k]);
  if (rc == MGH_SUCCESS) rc = mgh_layers_data(p, decompressed_data, output_pre_allocated);
  mgh_layers_close(p);
  return rc;
}

int mgh_layers_data_level(mgh_layers *p, int level, void **data, int output_pre_allocated) {
  if (!p || !data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  if (level < 0 || level > mgh_l_target(p->h))
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_layers_data_level: level outside 0 .. l_target");
  if (hipSetDevice(p->cfg.dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return hl_guarded([&] { return layers_data(p, data, output_pre_allocated != 0, level); });
}

} // extern "C"

// ---- precision layers in level order: containers of mgh_compress_level_layers read by resolution AND by
// tolerance. State between the calls: the accumulator in LEVEL-LINEARISED order (n elements), the header of
// layer 0, and per layer its header and the level up to which it has been added (depth, non-increasing in
// the layer's number: on every level the accumulator is the sum of a leading run of layers). A call decodes
// the chunks that hold its window [N_from, N_level) of one record -- a prefix, or a range from the chunk
// that holds N_from -- and streams that window into the accumulator (mgh_dequantize_add_linear); the decode
// buffer grows to the largest window decoded. mgh_level_layers_data recomposes the head [0, N_level) of the
// accumulator on a copy (mgh_recompose_linear_to_level).
struct mgh_level_layers {
  struct Layer {
    fmt::Header hd;
    int depth;
  };
  fmt::Header hd;  // of layer 0
  mgh_config cfg;
  bool in_dev = false;
  int dtype = MGH_FLOAT;
  size_t elem = 4;
  uint64_t n = 0;
  int L = 0;
  std::vector<uint64_t> N;  // N[l] = prod(level_shape(l))
  std::vector<Layer> layers;
  mgh_hierarchy *h = nullptr;
  mgh_lossless_ctx *ll = nullptr;
  hipStream_t st = nullptr;
  DevBuf acc;  // n elements: the coefficients, level-linearised
  DevBuf q;    // the integers of the chunks of the window being added
  DevBuf out;  // a level's array on its way to host memory
};

namespace {
void level_layers_free(mgh_level_layers *p) {
  if (!p) return;
  (void)hipSetDevice(p->cfg.dev_id);
  if (p->st) (void)hipStreamSynchronize(p->st);
  for (DevBuf *b : {&p->acc, &p->q, &p->out}) b->release();
  if (p->h) mgh_hierarchy_destroy(p->h);
  if (p->ll) mgh_lossless_destroy(p->ll);
  if (p->st) (void)hipStreamDestroy(p->st);
  delete p;
}

// One window of one container into the accumulator. k == count: layer 0 opens the handle (count == 0),
// every other one is added; k < count: layer k goes deeper. Every refusal comes before the accumulator is
// touched.
int level_layers_take(mgh_level_layers *p, int k, const void *data, size_t size, int level) {
  const int count = (int)p->layers.size();
  const bool first = count == 0, extend = k < count;
  const std::string who = first ? "mgh_level_layers_open: " : extend ? "mgh_level_layers_extend: " : "mgh_level_layers_add: ";
  std::unique_ptr<HostPrefix> prefix;
  const bool in_dev = is_device_pointer(data);
  if (in_dev) prefix.reset(new HostPrefix(data, size));
  size_t meta_size = 0;
  fmt::Header hd;
  HL_TRY(read_header(data, size, hd, meta_size));
  if (hd.shape.empty() || hd.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_UNSUPPORTED_DIMENSION, "header: dimension");
  if (!hd.quantized) return hl_fail(MGH_ERR_FORMAT, "not a compressed (quantized) stream");
  RecordView rv;
  HL_TRY(record_view_header(hd, rv));
  if (hd.dd_method != fmt::DD_NOOP)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, who + "the container is domain-decomposed (layers have one subdomain)");
  if (!hd.reorder)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, who + "a reorder = 0 container is no level-ordered layer (mgh_layers_* reads those)");
  for (uint64_t e : hd.shape)
    if (e < 3) return hl_fail(MGH_ERR_FORMAT, "header: extent below 3");
  if (!first) {
    if (const char *what = layers_mismatch(p->hd, hd)) return hl_fail(MGH_ERR_INVALID_ARGUMENT, who + what + " is not layer 0's");
    if (!extend && !(hd.tol < p->layers.back().hd.tol))
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, who + "the tolerance is not below the last layer's");
    if (extend) {
      const fmt::Header &was = p->layers[k].hd;
      if (!(hd.tol == was.tol) || hd.huff_dict_size != was.huff_dict_size || hd.huff_block_size != was.huff_block_size)
        return hl_fail(MGH_ERR_INVALID_ARGUMENT, who + "the container is not the one recorded for layer " + std::to_string(k) +
                                                     " (tolerance, dictionary or chunk size)");
    }
  }
  int L = p->L;
  std::vector<uint64_t> N = p->N;
  if (first) {
    HL_TRY(header_level_shape(hd, p->cfg, -1, &L, nullptr));
    N.resize(L + 1);
    for (int l = 0; l <= L; l++) {
      std::vector<uint64_t> shp;
      HL_TRY(header_level_shape(hd, p->cfg, l, nullptr, &shp));
      N[l] = 1;
      for (uint64_t e : shp) N[l] *= e;
    }
  }
  // the level: layer 0 anywhere, a new layer no deeper than the one before it, a layer going deeper no
  // deeper than the one before it either -- a finer layer alone on a level would be a residual of nothing
  const int lo_level = extend ? p->layers[k].depth + 1 : 0;
  const int hi_level = k > 0 ? p->layers[k - 1].depth : L;
  if (level < lo_level || level > hi_level)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, who + "level " + std::to_string(level) + " outside " + std::to_string(lo_level) +
                                                 " .. " + std::to_string(hi_level) + " for layer " + std::to_string(k));
  const uint64_t n = N[L];
  const size_t elem = hd.is_double ? 8 : 4;
  HL_TRY(record_view_at(data, size, meta_size, n * elem, rv));
  if (rv.raw) return hl_fail(MGH_ERR_INVALID_ARGUMENT, who + "the record is stored raw (no layer is)");
  if (first) {
    p->hd = hd;
    p->in_dev = in_dev;
    p->dtype = hd.is_double ? MGH_DOUBLE : MGH_FLOAT;
    p->elem = elem;
    p->n = n;
    p->L = L;
    p->N = N;
    std::vector<std::vector<double>> mirrored;
    bool owned = true;
    HL_TRY(get_hierarchy(&p->h, &owned, p->dtype, hd.shape, decoder_coords(hd, p->cfg, mirrored),
                         std::vector<uint64_t>(hd.shape.size(), 0), p->cfg, 0, /*cached=*/false));
    if (mgh_l_target(p->h) != L) return hl_fail(MGH_ERR_FORMAT, "header: the hierarchy of the subdomain is not the header's");
    HL_HIP(hipStreamCreate(&p->st));
    HL_TRY(mgh_lossless_create(&p->ll, p->cfg.dev_id));
    HL_TRY(p->acc.ensure(n * elem));
  }
  // the window [lo, hi) of the level-linearised array, and the chunks that hold it
  const uint64_t block = std::max<uint64_t>(hd.huff_block_size, 1);
  const uint64_t lo = extend ? N[p->layers[k].depth] : 0, hi = N[level];
  const uint64_t dec_first = lo / block * block, dec_end = std::min(n, ((hi - 1) / block + 1) * block);
  HL_TRY(p->q.ensure((dec_end - dec_first) * 8));
  mgh_decompress_stats &stats = decompress_stats();
  stats = mgh_decompress_stats{};
  stats.subdomains = 1;
  auto in_type = [&](double v) { return hd.is_double ? v : (double)(float)v; };
  uint64_t ocount = 0;
  int rc = lossless_decompress(p->ll, rv.rec, rv.csize, rv.lossless, (int64_t *)p->q.p, n, &ocount, p->st, nullptr,
                               /*sync_end=*/false, DecodeRange{/*n_prefix=*/hi, /*q_cap=*/dec_end - dec_first, /*first=*/lo});
  if (rc == MGH_SUCCESS)
    rc = mgh_dequantize_add_linear(p->h, (int64_t *)p->q.p + (lo - dec_first), lo, hi - lo, hd.rel ? MGH_REL : MGH_ABS,
                                   in_type(hd.tol), in_type(hd.s), in_type(hd.norm), hd.huff_dict_size, 1,
                                   (const uint64_t *)p->ll->oidx.p, (const int64_t *)p->ll->oval.p, ocount, k == 0 ? 1 : 0,
                                   p->acc.p, p->st);
  if (hipStreamSynchronize(p->st) != hipSuccess && rc == MGH_SUCCESS) rc = hl_fail(MGH_ERR_DEVICE, "sync");
  if (rc == MGH_SUCCESS) rc = lossless_tag_check(p->ll);
  HL_TRY(rc);
  if (extend) p->layers[k].depth = level;
  else p->layers.push_back({hd, level});
  return MGH_SUCCESS;
}

// mgh_recompose_linear_to_level of the accumulator's head into an array in the containers' memory space
// (or the caller's buffer); the accumulator stays.
int level_layers_data(mgh_level_layers *p, int level, void **out, bool prealloc) {
  hipStream_t st = p->st;
  const size_t out_bytes = p->N[level] * p->elem;
  const OutSlot slot{out, p->in_dev, prealloc};
  HL_TRY(slot.alloc(out_bytes));
  int rc = MGH_SUCCESS;
  if (is_device_pointer(*out)) {
    rc = mgh_recompose_linear_to_level(p->h, p->acc.p, level, *out, st);
  } else {
    rc = p->out.ensure(out_bytes);
    if (rc == MGH_SUCCESS) rc = mgh_recompose_linear_to_level(p->h, p->acc.p, level, p->out.p, st);
    if (rc == MGH_SUCCESS) rc = copy_any(*out, p->out.p, out_bytes, st);
  }
  if (hipStreamSynchronize(st) != hipSuccess && rc == MGH_SUCCESS) rc = hl_fail(MGH_ERR_DEVICE, "sync");
  return slot.fail(rc);
}
}  // namespace

extern "C" {

int mgh_level_layers_open(mgh_level_layers **out, const void *compressed_data, size_t compressed_size,
                          const mgh_config *config, int level) {
  if (!out || !compressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  *out = nullptr;
  {
    const std::string bad = env_validate();
    if (!bad.empty()) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad);
  }
  mgh_config def;
  if (!config) {
    mgh_config_default(&def);
    config = &def;
  }
  if (mgh_device_count() <= 0) return hl_fail(MGH_ERR_NO_DEVICE, "no HIP device");
  if (hipSetDevice(config->dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  mgh_level_layers *p = new mgh_level_layers();
  p->cfg = *config;
  const int rc = hl_guarded([&] { return level_layers_take(p, 0, compressed_data, compressed_size, level); });
  if (rc != MGH_SUCCESS) {
    level_layers_free(p);
    return rc;
  }
  *out = p;
  return MGH_SUCCESS;
}

int mgh_level_layers_add(mgh_level_layers *p, const void *compressed_data, size_t compressed_size, int level) {
  if (!p || !compressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (p->layers.size() >= (size_t)kLadderMaxTols) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_level_layers_add: 64 layers at most");
  if (hipSetDevice(p->cfg.dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return hl_guarded([&] { return level_layers_take(p, (int)p->layers.size(), compressed_data, compressed_size, level); });
}

int mgh_level_layers_extend(mgh_level_layers *p, int k, const void *compressed_data, size_t compressed_size, int level) {
  if (!p || !compressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (k < 0 || k >= (int)p->layers.size())
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_level_layers_extend: no layer " + std::to_string(k));
  if (hipSetDevice(p->cfg.dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return hl_guarded([&] { return level_layers_take(p, k, compressed_data, compressed_size, level); });
}

int mgh_level_layers_count(const mgh_level_layers *p) { return p ? (int)p->layers.size() : -1; }

int mgh_level_layers_depth(const mgh_level_layers *p, int k) {
  return p && k >= 0 && k < (int)p->layers.size() ? p->layers[k].depth : -1;
}

double mgh_level_layers_tolerance(const mgh_level_layers *p, int k) {
  return p && k >= 0 && k < (int)p->layers.size() ? p->layers[k].hd.tol : 0.0;
}

int mgh_level_layers_data(mgh_level_layers *p, int level, void **data, int output_pre_allocated) {
  if (!p || !data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  if (level < 0 || level > p->layers[0].depth)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_level_layers_data: level " + std::to_string(level) + " outside 0 .. " +
                                                 std::to_string(p->layers[0].depth) + " (the depth of layer 0)");
  if (hipSetDevice(p->cfg.dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return hl_guarded([&] { return level_layers_data(p, level, data, output_pre_allocated != 0); });
}

void mgh_level_layers_close(mgh_level_layers *p) { level_layers_free(p); }

int mgh_decompress_level_layers(int nlayers, const void *const *compressed_data, const size_t *compressed_size, int level,
                                const mgh_config *config, void **decompressed_data, int output_pre_allocated) {
  if (!compressed_data || !compressed_size || !decompressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (nlayers < 1 || nlayers > kLadderMaxTols)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "decompress_level_layers: nlayers must be in 1..64");
  for (int k = 0; k < nlayers; k++)
    if (!compressed_data[k]) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*decompressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  mgh_level_layers *p = nullptr;
  int rc = mgh_level_layers_open(&p, compressed_data[0], compressed_size[0], config, level);
  for (int k = 1; k < nlayers && rc == MGH_SUCCESS; k++) rc = mgh_level_layers_add(p, compressed_data[k], compressed_size[k], level);
  if (rc == MGH_SUCCESS) rc = mgh_level_layers_data(p, level, decompressed_data, output_pre_allocated);
  mgh_level_layers_close(p);
  return rc;
}

} // extern "C"

// ---- arrays with missing values: mgh_compress_masked and its readers (mask_plan.hpp) ----------------------
namespace {

// the mask's bytes <-> symbols of the lossless stage (dictionary 256), and the mask as one byte per element
__global__ void __launch_bounds__(256) k_mask_widen(const uint8_t *__restrict__ bytes, size_t nb, uint16_t *__restrict__ sym) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (size_t)gridDim.x * 256) sym[i] = bytes[i];
}
template <typename SYM>
__global__ void __launch_bounds__(256) k_mask_narrow(const SYM *__restrict__ sym, size_t nb, uint8_t *__restrict__ bytes) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nb; i += (size_t)gridDim.x * 256) bytes[i] = (uint8_t)sym[i];
}
__global__ void __launch_bounds__(256)
k_mask_expand(const unsigned long long *__restrict__ words, size_t n, uint8_t *__restrict__ mask) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    mask[i] = (uint8_t)((words[i >> 6] >> (i & 63)) & 1);
}
inline unsigned mask_grid(size_t items) { return (unsigned)std::min<size_t>((items + 255) / 256, 2048); }

int masked_shape_elems(const char *who, int D, const uint64_t *shape, uint64_t *n_out) {
  uint64_t n = 1;
  for (int d = 0; d < D; d++) {
    if (shape[d] == 0 || shape[d] > 0xffffffffull || n * shape[d] > 0xffffffffull)
      return hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string(who) + ": 1 .. 2^32 - 1 elements");
    n *= shape[d];
  }
  *n_out = n;
  return MGH_SUCCESS;
}

// The record of a packed bitmap of n bits, n_set of them set (the mask; the flag bits of the pointwise-relative
// writer): one record of the lossless stage where that is smaller than the packed words (mask_record_kind).
int bitmap_record(const char *who, const uint64_t *d_words, uint64_t n, uint64_t n_set, const mgh_config &cfg, hipStream_t st,
                  uint32_t &kind, std::vector<uint8_t> &rec) {
  HlCache &C = g_cache;
  const uint64_t nw = mask_words(n), nb = mask_packed_bytes(n);
  const std::string w(who);
  mgh_lossless_ctx *ll = C.lane[0].ll;
  uint64_t coded = 0;
  rec.clear();
  if (n_set && mask_record_codable(cfg.huff_block_size)) {
    HL_TRY(C.msym.ensure(nb * 2));
    k_mask_widen<<<mask_grid(nb), 256, 0, st>>>((const uint8_t *)d_words, nb, (uint16_t *)C.msym.p);
    if (hipGetLastError() != hipSuccess) return hl_fail(MGH_ERR_DEVICE, w + ": k_mask_widen");
    // (a code stream of the packed words' size or more is of no interest: cap_units)
    HL_TRY(lossless_compress(ll, (const int64_t *)C.msym.p, nb, kMaskDict, cfg.huff_block_size, cfg.lossless,
                             cfg.zstd_compress_level, nullptr, nullptr, 0, st, nullptr, ~(uint64_t)0, nw + 1, /*sym16=*/true));
    if (!ll->overflow) coded = ll->record_size();
  }
  kind = mask_record_kind(n, n_set, coded);
  if (kind == kMaskCoded) {
    if (ll->on_host) {
      rec = ll->host;
    } else {
      rec.resize(coded);
      HL_TRY(record_write(ll, rec.data(), st));
      if (hipStreamSynchronize(st) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, w + ": reading the mask record back");
    }
  } else if (kind == kMaskPacked) {
    rec.resize(nb);
    if (hipMemcpyAsync(rec.data(), d_words, nb, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return hl_fail(MGH_ERR_DEVICE, w + ": reading the packed mask back");
  }
  return MGH_SUCCESS;
}

// The record and the footer of a packed bitmap (the mask; the flag bits of the pointwise-relative writer) behind the
// first `at` bytes of an output of `cap` bytes: bitmap_record -> the capacity -> the footer behind the record -> the
// two into the output. footer(kind, the record's bytes, its CRC32, dst) serialises `footer_bytes` bytes; too_small
// is the refusal's text behind `who`. *end: the bytes of the output in use.
template <typename Footer>
int write_trailer(const char *who, const char *too_small, void *out, size_t at, size_t cap, const uint64_t *d_words, uint64_t n,
                  uint64_t n_set, const mgh_config &cfg, hipStream_t st, size_t footer_bytes, Footer footer, size_t *end) {
  uint32_t kind = kMaskNone;
  std::vector<uint8_t> rec;
  HL_TRY(bitmap_record(who, d_words, n, n_set, cfg, st, kind, rec));
  const size_t record = rec.size();
  if (at + record + footer_bytes > cap) return hl_fail(MGH_ERR_OUTPUT_TOO_LARGE, std::string(who) + too_small);
  rec.resize(record + footer_bytes);
  footer(kind, record, fmt::crc32(rec.data(), record), rec.data() + record);
  if (is_device_pointer(out)) {
    if (hipMemcpyAsync((char *)out + at, rec.data(), rec.size(), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return hl_fail(MGH_ERR_DEVICE, std::string(who) + ": writing mask record and footer");
  } else {
    std::memcpy((char *)out + at, rec.data(), rec.size());
  }
  *end = at + rec.size();
  return MGH_SUCCESS;
}

// What the classifying pass of a writer left on the device: the array (`src`, device memory), its packed mask and
// the statistics of the valid elements. in_dev: the caller's array is device memory.
struct MaskedScan {
  const void *src = nullptr;
  bool in_dev = false;
  uint64_t n = 0, n_masked = 0;
  double vmin = 0, vmax = 0;
  uint64_t *d_words = nullptr;
};

// The head of a writer, in front of its classifying pass: element count -> the caller's own argument check
// (bad_arg: its refusal, or nullptr) -> footprint (the array on the device and a copy beside a device-resident one;
// too_large: the refusal's text) -> the cache -> the mask words with the pass's statistics behind them -> a host
// array uploaded into C.mfill. S.src is the array on the device; S.n_masked, S.vmin and S.vmax are the caller's to
// fill from *d_stats once its pass has run.
template <typename Stats>
int scan_head(const char *who, const char *bad_arg, const char *too_large, int D, int dtype, const uint64_t *shape,
              const void *original, const mgh_config &cfg, MaskedScan &S, Stats **d_stats) {
  HL_TRY(masked_shape_elems(who, D, shape, &S.n));
  if (bad_arg) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad_arg);
  const size_t bytes = (size_t)S.n * (dtype == MGH_DOUBLE ? 8 : 4);
  S.in_dev = is_device_pointer(original);
  if ((S.in_dev ? 2 : 1) * (uint64_t)bytes > cfg.max_memory_footprint) return hl_fail(MGH_ERR_INVALID_ARGUMENT, too_large);
  HL_TRY(cache_prepare(cfg.dev_id));
  HlCache &C = g_cache;
  const uint64_t nb = mask_packed_bytes(S.n);
  HL_TRY(C.mwords.ensure(nb + sizeof(Stats)));
  S.d_words = (uint64_t *)C.mwords.p;
  *d_stats = (Stats *)((char *)C.mwords.p + nb);
  S.src = original;
  if (!S.in_dev) {
    HL_TRY(C.mfill.ensure(bytes));
    HL_TRY(copy_any(C.mfill.p, original, bytes, C.lane[0].st));
    S.src = C.mfill.p;
  }
  return MGH_SUCCESS;
}

// The masked writer behind its scan, shared by mgh_compress_masked and mgh_compress_pwrel: fill -> the output ->
// mgh_compress of the filled array -> mask record -> footer. *csize: the bytes written (on entry the capacity of a
// pre-allocated output). behind_min / behind_max: bytes the caller appends behind the masked buffer, at least and at
// most (0, 0 for mgh_compress_masked): the first is kept free in a pre-allocated output, the second is added to an
// allocated one. A failure has gone through slot.fail.
int masked_write(const char *who, int D, int dtype, const uint64_t *shape, double tol, double s, int ebtype, const MaskedScan &S,
                 double restore_value, const OutSlot &slot, size_t *csize, const void *const *coords, const mgh_config &cfg,
                 size_t behind_min, size_t behind_max) {
  const bool is_double = dtype == MGH_DOUBLE;
  const size_t elem = is_double ? 8 : 4;
  const uint64_t n = S.n, nb = mask_packed_bytes(n);
  const std::string w(who);
  HlCache &C = g_cache;
  hipStream_t st = C.lane[0].st;
  const void *filled = S.src;  // (nothing masked: the array as it is, a device-resident one where it lies)
  if (S.n_masked) {
    HL_TRY(C.mfill.ensure(n * elem));
    const uint64_t c_bits = mask_value_bits(is_double, mask_fill_constant(S.vmin, S.vmax));
    HL_TRY(mgh_mask_fill_bits_(D, dtype, shape, S.src, S.d_words, c_bits, C.mfill.p, st));
    HL_HIP(hipStreamSynchronize(st));
    filled = C.mfill.p;
  }
  // the output: mgh_compress's own capacity, and room for the packed mask and the footer behind it
  size_t cap = 0, ccap = 0;
  if (slot.prealloc) {
    cap = *csize;
    if (cap <= kMaskFooterBytes + behind_min) return hl_fail(MGH_ERR_OUTPUT_TOO_LARGE, w + ": the output cannot hold the footer");
    ccap = cap - kMaskFooterBytes - behind_min;
  } else {
    ccap = n * elem + (size_t)1e6;
    cap = ccap + nb + kMaskFooterBytes + behind_max;
    HL_TRY(slot.alloc(cap));
  }
  void *out = *slot.slot;
  size_t container = ccap;
  int rc = mgh_compress(D, dtype, shape, tol, s, ebtype, filled, &out, &container, coords, &cfg, 1);
  if (rc != MGH_SUCCESS) return slot.fail(rc);
  // the mask record: one record of the lossless stage where that is smaller than the packed words
  MaskFooter f;
  f.container = container;
  f.n_masked = S.n_masked;
  f.restore_bits = mask_value_bits(is_double, restore_value);
  return slot.fail(write_trailer(who, ": the output cannot hold container, mask record and footer", out, container,
                                 cap - behind_min, S.d_words, n, S.n_masked, cfg, st, kMaskFooterBytes,
                                 [&](uint32_t kind, size_t record, uint32_t crc, uint8_t *dst) {
                                   f.kind = kind;
                                   f.record = record;
                                   f.crc = crc;
                                   mask_footer_serialize(f, dst);
                                 },
                                 csize));
}

int compress_masked_impl(int D, int dtype, const uint64_t *shape, double tol, double s, int ebtype, const void *original,
                         const mgh_mask_spec &spec, void **compressed, size_t *csize, const void *const *coords,
                         const mgh_config &cfg, bool prealloc) {
  const char *bad_arg = nullptr;
  if (spec.flags == 0 || (spec.flags & ~(MGH_MASK_NONFINITE | MGH_MASK_VALUE)))
    bad_arg = "compress_masked: flags must be MGH_MASK_NONFINITE, MGH_MASK_VALUE or both";
  else if ((spec.flags & MGH_MASK_VALUE) && std::isnan(spec.fill_value))
    bad_arg = "compress_masked: a NaN fill_value (MGH_MASK_NONFINITE masks NaN)";
  MaskedScan S;
  mgh_mask_stats *d_stats = nullptr;
  // the array on the device, and for a device-resident one its filled copy beside it
  HL_TRY(scan_head("compress_masked", bad_arg,
                   "compress_masked: the array and its filled copy do not fit max_memory_footprint (masked arrays are "
                   "not streamed in parts)",
                   D, dtype, shape, original, cfg, S, &d_stats));
  hipStream_t st = g_cache.lane[0].st;
  HL_TRY(mgh_mask_scan(D, dtype, shape, S.src, spec.flags, spec.fill_value, S.d_words, d_stats, st));
  mgh_mask_stats hs{};
  HL_HIP(hipMemcpyAsync(&hs, d_stats, sizeof(hs), hipMemcpyDeviceToHost, st));
  HL_HIP(hipStreamSynchronize(st));
  S.n_masked = hs.n_masked;
  S.vmin = hs.vmin;
  S.vmax = hs.vmax;
  return masked_write("compress_masked", D, dtype, shape, tol, s, ebtype, S, spec.restore_value, OutSlot{compressed, S.in_dev, prealloc},
                      csize, coords, cfg, 0, 0);
}

// A masked buffer opened: the footer, the header of the container in front of it, and the record on the host.
struct MaskedView {
  MaskFooter f;
  fmt::Header hd;
  uint64_t n = 0;
  int dtype = MGH_FLOAT, lossless = MGH_LOSSLESS_HUFFMAN;
  std::vector<uint8_t> rec;
};

// Bytes [at, at + len) of a buffer in device memory (in_dev) or on the host, on the host.
int host_piece(void *dst, const void *buf, bool in_dev, size_t at, size_t len) {
  const uint8_t *p = (const uint8_t *)buf + at;
  if (len && in_dev) return aux_read(dst, p, len);
  if (len) std::memcpy(dst, p, len);
  return MGH_SUCCESS;
}

// The rule of every reader that needs its footer: open(buf, size, v) < 0 is a status, 0 (no footer's magic) is
// MGH_ERR_FORMAT with the reader's own text.
template <typename Open, typename View>
int open_or_refuse(Open open, const void *buf, size_t size, View &v, const std::string &no_footer) {
  const int opened = open(buf, size, v);
  return opened < 0 ? opened : opened == 0 ? hl_fail(MGH_ERR_FORMAT, no_footer) : MGH_SUCCESS;
}

// 1: a masked buffer that passed every check; 0: no footer's magic; negative: a status.
int masked_open(const void *buf, size_t size, MaskedView &v) {
  if (size < kMaskFooterBytes) return 0;
  const bool in_dev = is_device_pointer(buf);
  uint8_t tail[kMaskFooterBytes];
  HL_TRY(host_piece(tail, buf, in_dev, size - kMaskFooterBytes, kMaskFooterBytes));
  if (!mask_footer_present(tail, size)) return 0;
  if (const char *bad = mask_footer_parse(tail, size, v.f)) return hl_fail(MGH_ERR_FORMAT, bad);
  size_t meta = 0;
  HL_TRY(read_header(buf, (size_t)v.f.container, v.hd, meta));
  if (v.hd.shape.empty() || v.hd.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_FORMAT, "header: dimension");
  v.n = 1;
  for (uint64_t e : v.hd.shape) {
    if (e == 0 || e > 0xffffffffull || v.n * e > 0xffffffffull) return hl_fail(MGH_ERR_FORMAT, "mask footer: an array of 2^32 elements or more");
    v.n *= e;
  }
  v.dtype = v.hd.is_double ? MGH_DOUBLE : MGH_FLOAT;
  v.lossless = v.hd.compressor == fmt::COMP_X_HUFFMAN_ZSTD ? MGH_LOSSLESS_HUFFMAN_ZSTD : MGH_LOSSLESS_HUFFMAN;
  if (const char *bad = mask_footer_check_n(v.f, v.n, v.hd.is_double)) return hl_fail(MGH_ERR_FORMAT, bad);
  v.rec.resize((size_t)v.f.record);
  HL_TRY(host_piece(v.rec.data(), buf, in_dev, (size_t)v.f.container, (size_t)v.f.record));
  if (const char *bad = mask_record_check_crc(v.f, v.rec.data())) return hl_fail(MGH_ERR_FORMAT, bad);
  return 1;
}

// The packed bitmap of n bits that a record of `kind` holds (bitmap_record), into the device buffer `dst` of at least
// 8 ceil(n / 64) bytes, queued on `st`.
int bitmap_words(uint32_t kind, const std::vector<uint8_t> &rec, uint64_t n, int lossless, void *dst, hipStream_t st) {
  HlCache &C = g_cache;
  const uint64_t nb = mask_packed_bytes(n);
  if (kind == kMaskNone) {
    HL_HIP(hipMemsetAsync(dst, 0, nb, st));
  } else if (kind == kMaskPacked) {
    HL_HIP(hipMemcpyAsync(dst, rec.data(), nb, hipMemcpyHostToDevice, st));
    HL_HIP(hipStreamSynchronize(st));  // (the record's host copy belongs to the caller)
  } else {
    HL_TRY(C.msym.ensure(nb * 8));
    const mgh_decompress_stats kept = decompress_stats();  // (the statistics are the container's, not the mask's)
    bool sym16 = true;
    uint64_t ocount = 0;
    const int rc = lossless_decompress(C.lane[0].ll, rec.data(), rec.size(), lossless, (int64_t *)C.msym.p, nb, &ocount,
                                       st, &sym16);
    decompress_stats() = kept;
    HL_TRY(rc);
    if (ocount) return hl_fail(MGH_ERR_FORMAT, "mask record: outliers in a record of bytes");
    if (sym16) k_mask_narrow<uint16_t><<<mask_grid(nb), 256, 0, st>>>((const uint16_t *)C.msym.p, nb, (uint8_t *)dst);
    else k_mask_narrow<int64_t><<<mask_grid(nb), 256, 0, st>>>((const int64_t *)C.msym.p, nb, (uint8_t *)dst);
    HL_HIP(hipGetLastError());
  }
  return MGH_SUCCESS;
}

// The packed mask of an opened buffer in the cache's device buffer, queued on `st`.
int masked_words(const MaskedView &v, hipStream_t st, uint64_t **d_words_out) {
  HlCache &C = g_cache;
  HL_TRY(C.mwords.ensure(mask_packed_bytes(v.n) + sizeof(mgh_mask_stats)));
  *d_words_out = (uint64_t *)C.mwords.p;
  return bitmap_words(v.f.kind, v.rec, v.n, v.lossless, C.mwords.p, st);
}

int masked_config(const mgh_config *config, mgh_config &cfg) {
  if (config) cfg = *config;
  else mgh_config_default(&cfg);
  int ndev = mgh_device_count();
  if (ndev <= 0) return hl_fail(MGH_ERR_NO_DEVICE, "no HIP device");
  if (cfg.dev_id < 0 || cfg.dev_id >= ndev) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "dev_id");
  if (hipSetDevice(cfg.dev_id) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, "hipSetDevice");
  return MGH_SUCCESS;
}

// A reader whose last pass runs on the device, around the plain reader of the container part. It owns the output
// (allocated in the memory space of `buf` unless pre-allocated), the device buffer a host output is reconstructed in
// (C.mfill), the copy out and the final synchronise; every failure behind the allocation goes through slot.fail.
// decode(&dst): the plain reader with the pre-allocated device destination; post(d_data, st): the device passes
// over its result, queued on `st`.
template <typename Decode, typename Post>
int staged_read(const char *who, const void *buf, size_t bytes, const mgh_config &cfg, void **out, bool prealloc, Decode decode,
                Post post) {
  const bool in_dev = is_device_pointer(buf);
  const bool out_dev = prealloc ? is_device_pointer(*out) : in_dev;
  HL_TRY(cache_prepare(cfg.dev_id));
  HlCache &C = g_cache;
  hipStream_t st = C.lane[0].st;
  const OutSlot slot{out, in_dev, prealloc};
  HL_TRY(slot.alloc(bytes));
  void *d_data = *out;
  int rc = MGH_SUCCESS;
  if (!out_dev) {
    if ((rc = C.mfill.ensure(bytes)) != MGH_SUCCESS) return slot.fail(rc);
    d_data = C.mfill.p;
  }
  void *dst = d_data;
  if ((rc = decode(&dst)) != MGH_SUCCESS) return slot.fail(rc);
  if ((rc = post(d_data, st)) != MGH_SUCCESS) return slot.fail(rc);
  if (!out_dev && (rc = copy_any(*out, d_data, bytes, st)) != MGH_SUCCESS) return slot.fail(rc);
  if (hipStreamSynchronize(st) != hipSuccess) return slot.fail(hl_fail(MGH_ERR_DEVICE, std::string(who) + ": hipStreamSynchronize"));
  return MGH_SUCCESS;
}

// n bits of packed words on the device as one byte each in `mask` (host or device memory), complete on return.
int mask_bytes_out(const uint64_t *d_words, size_t n, uint8_t *mask, hipStream_t st) {
  HlCache &C = g_cache;
  const bool out_dev = is_device_pointer(mask);
  uint8_t *d_mask = mask;
  if (!out_dev) {  // (the symbols have been narrowed into the words: their buffer is free)
    HL_TRY(C.msym.ensure(n));
    d_mask = (uint8_t *)C.msym.p;
  }
  k_mask_expand<<<mask_grid(n), 256, 0, st>>>((const unsigned long long *)d_words, n, d_mask);
  HL_HIP(hipGetLastError());
  if (!out_dev) HL_TRY(copy_any(mask, d_mask, n, st));
  HL_HIP(hipStreamSynchronize(st));
  return MGH_SUCCESS;
}

// ---- masked buffers in the full, reduced-resolution, preview and verify readers ------------------------------
// THE RULE: a node of a level or coarsened array is masked when the element of the full array at that node's
// index is masked (sampling: masked neighbours do not count); a position of a preview or of a window is masked
// when that position of the full array is. Masked positions hold restore_value's bits; every other position
// holds, bit for bit, what the same reader writes for the container part alone -- near masked regions that
// value carries the influence of the fill.
enum class ReadKind { full, level, coarsened, preview, window };  // mgh_decompress, _level, _coarsened, _preview(_window)
struct MaskedRead {
  ReadKind kind = ReadKind::full;
  int level = -1, halvings = -1;
  const uint64_t *lo = nullptr, *ext = nullptr;  // the window
  const char *who = "masked reader";             // ... in the messages, and the refusal of a buffer without the footer
  const char *no_footer = "masked reader: no mask footer (a plain container has the plain reader)";
};

// The shape of what the reader returns and, per dimension, the index in the full array of each of its positions
// (sampled = false: the output is the full array and no list is made).
int masked_read_lists(const MaskedView &v, const mgh_config &cfg, const MaskedRead &R, std::vector<uint64_t> &oshape,
                      std::vector<std::vector<uint32_t>> &lists, bool &sampled) {
  const int D = (int)v.hd.shape.size();
  lists.assign(D, {});
  sampled = R.kind != ReadKind::full && R.kind != ReadKind::preview;
  std::vector<uint64_t> idx;
  if (!sampled) {  // (nothing asked of the header but its shape: a decomposed container is as good as any)
    oshape = v.hd.shape;
  } else if (R.kind == ReadKind::level) {  // (refuses a decomposed container, as mgh_decompress_level does)
    int L = 0;
    HL_TRY(header_level_shape(v.hd, cfg, R.level, &L, &oshape));
    for (int d = 0; d < D; d++) {
      mgh::level_nodes(v.hd.shape[d], L - R.level, idx);
      lists[d].assign(idx.begin(), idx.end());
    }
  } else if (R.kind == ReadKind::window) {
    oshape.assign(R.ext, R.ext + D);
    for (int d = 0; d < D; d++) {
      if (R.ext[d] == 0 || R.lo[d] > v.hd.shape[d] || R.ext[d] > v.hd.shape[d] - R.lo[d])
        return hl_fail(MGH_ERR_INVALID_ARGUMENT, "the window leaves the array");
      for (uint64_t i = 0; i < R.ext[d]; i++) lists[d].push_back((uint32_t)(R.lo[d] + i));
    }
  } else {  // the code that answers mgh_infer_coarsened_nodes
    Decomposer dd;
    HL_TRY(decomposer_from_header(v.hd, cfg, dd));
    for (int d = 0; d < D; d++) {
      StitchedLayout sl;
      HL_TRY(hl_plan(stitched_layout(dd, cfg.max_larget_level, R.halvings, sl, d)));
      lists[d].assign(sl.nodes[d].begin(), sl.nodes[d].end());
      oshape = sl.shape;
    }
  }
  for (int d = 0; d < D && sampled; d++)
    if (lists[d].size() != oshape[d]) return hl_fail(MGH_ERR_FORMAT, "masked reader: node list and shape disagree");
  return MGH_SUCCESS;
}

// The node lists in the cache's index buffer, complete on the device on return; d_idx[d]: the list of dimension d.
int upload_lists(const std::vector<std::vector<uint32_t>> &lists, hipStream_t st, const uint32_t **d_idx) {
  HlCache &C = g_cache;
  std::vector<uint32_t> all;
  size_t at[MGH_MAX_DIM];
  for (size_t d = 0; d < lists.size(); d++) {
    at[d] = all.size();
    all.insert(all.end(), lists[d].begin(), lists[d].end());
  }
  HL_TRY(C.midx.ensure(all.size() * sizeof(uint32_t)));
  HL_HIP(hipMemcpyAsync(C.midx.p, all.data(), all.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HL_HIP(hipStreamSynchronize(st));  // (the lists' host copy ends with this call)
  for (size_t d = 0; d < lists.size(); d++) d_idx[d] = (const uint32_t *)C.midx.p + at[d];
  return MGH_SUCCESS;
}

// The mask of the reader's output, packed, in the cache (queued on `st`): the full mask, or its sample through
// the lists, which are uploaded into the cache's index buffer.
int masked_read_words(const MaskedView &v, const std::vector<uint64_t> &oshape, const std::vector<std::vector<uint32_t>> &lists,
                      bool sampled, hipStream_t st, uint64_t **d_words_out) {
  HlCache &C = g_cache;
  uint64_t *d_full = nullptr;
  HL_TRY(masked_words(v, st, &d_full));
  *d_words_out = d_full;
  if (!sampled) return MGH_SUCCESS;
  const int D = (int)oshape.size();
  uint64_t n_out = 1;
  for (int d = 0; d < D; d++) n_out *= oshape[d];
  HL_TRY(C.msamp.ensure(mask_packed_bytes(n_out)));
  const uint32_t *d_idx[MGH_MAX_DIM];
  HL_TRY(upload_lists(lists, st, d_idx));
  HL_TRY(mgh_mask_sample_(D, v.hd.shape.data(), d_full, oshape.data(), d_idx, (uint64_t *)C.msamp.p, nullptr, st));
  *d_words_out = (uint64_t *)C.msamp.p;
  return MGH_SUCCESS;
}

// The plain reader of the view R on the container part, into the pre-allocated device destination *dst.
int plain_read(const MaskedRead &R, const void *buf, size_t csize, const mgh_config &cfg, void **dst) {
  switch (R.kind) {
  case ReadKind::full: return mgh_decompress(buf, csize, dst, &cfg, 1);
  case ReadKind::level: return mgh_decompress_level(buf, csize, R.level, dst, &cfg, 1);
  case ReadKind::coarsened: return mgh_decompress_coarsened(buf, csize, R.halvings, dst, &cfg, 1);
  case ReadKind::preview: return mgh_decompress_preview(buf, csize, R.halvings, dst, &cfg, 1);
  default: return mgh_decompress_preview_window(buf, csize, R.halvings, R.lo, R.ext, dst, &cfg, 1);
  }
}

// masked_open -> the plain reader on the first C bytes into a device buffer -> the mask -> its sample -> restore
int masked_read_impl(const void *buf, size_t size, const mgh_config &cfg, const MaskedRead &R, void **out, bool prealloc) {
  MaskedView v;
  HL_TRY(open_or_refuse(masked_open, buf, size, v, R.no_footer));
  std::vector<uint64_t> oshape;
  std::vector<std::vector<uint32_t>> lists;
  bool sampled = false;
  HL_TRY(masked_read_lists(v, cfg, R, oshape, lists, sampled));
  size_t bytes = v.hd.is_double ? 8 : 4;
  for (uint64_t e : oshape) bytes *= (size_t)e;
  const size_t csize = (size_t)v.f.container;
  return staged_read(
      R.who, buf, bytes, cfg, out, prealloc, [&](void **dst) { return plain_read(R, buf, csize, cfg, dst); },
      [&](void *d_data, hipStream_t st) -> int {
        if (v.f.kind == kMaskNone) return MGH_SUCCESS;
        uint64_t *d_words = nullptr;
        HL_TRY(masked_read_words(v, oshape, lists, sampled, st, &d_words));
        return mgh_mask_restore_bits_((int)oshape.size(), v.dtype, oshape.data(), d_words, v.f.restore_bits, d_data, st);
      });
}

// ... and the sampled mask alone, one byte per output element
int masked_read_mask_impl(const void *buf, size_t size, const mgh_config &cfg, const MaskedRead &R, uint8_t *mask) {
  MaskedView v;
  HL_TRY(open_or_refuse(masked_open, buf, size, v, R.no_footer));
  std::vector<uint64_t> oshape;
  std::vector<std::vector<uint32_t>> lists;
  bool sampled = false;
  HL_TRY(masked_read_lists(v, cfg, R, oshape, lists, sampled));
  size_t n_out = 1;
  for (uint64_t e : oshape) n_out *= (size_t)e;
  HL_TRY(cache_prepare(cfg.dev_id));
  hipStream_t st = g_cache.lane[0].st;
  uint64_t *d_words = nullptr;
  HL_TRY(masked_read_words(v, oshape, lists, sampled, st, &d_words));
  return mask_bytes_out(d_words, n_out, mask, st);
}

int masked_read_entry(const void *buf, size_t size, const mgh_config *config, const MaskedRead &R, void **out, int prealloc) {
  if (!buf || !out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (prealloc && !*out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  mgh_config cfg;
  HL_TRY(masked_config(config, cfg));
  return hl_guarded([&] { return masked_read_impl(buf, size, cfg, R, out, prealloc != 0); });
}

int masked_read_mask_entry(const void *buf, size_t size, const mgh_config *config, const MaskedRead &R, uint8_t *mask) {
  if (!buf || !mask) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  mgh_config cfg;
  HL_TRY(masked_config(config, cfg));
  return hl_guarded([&] { return masked_read_mask_impl(buf, size, cfg, R, mask); });
}

const char *const kBadHalvings = "halvings outside 0 .. the smallest l_target of the subdomains";

} // namespace

extern "C" {

int mgh_compress_masked(int D, int dtype, const uint64_t *shape, double tol, double s, int ebtype, const void *original_data,
                        const mgh_mask_spec *spec, void **compressed_data, size_t *compressed_size,
                        const void *const *coords, const mgh_config *config, int output_pre_allocated) {
  if (!compressed_data || !compressed_size || !spec) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  HL_TRY(size_call_args(D, dtype, shape, ebtype, original_data, config, output_pre_allocated ? compressed_data : nullptr));
  return hl_guarded([&]() -> int {
    return compress_masked_impl(D, dtype, shape, tol, s, ebtype, original_data, *spec, compressed_data, compressed_size,
                                coords, *config, output_pre_allocated != 0);
  });
}

int mgh_masked_info(const void *compressed_data, size_t compressed_size, struct mgh_masked_info *info) {
  if (!compressed_data || !info) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  return hl_guarded([&]() -> int {
    MaskedView v;
    const int opened = masked_open(compressed_data, compressed_size, v);
    if (opened <= 0) return opened;
    info->container_size = v.f.container;
    info->record_size = v.f.record;
    info->n_masked = v.f.n_masked;
    info->kind = (int)v.f.kind;
    info->restore_value = mask_bits_value(v.hd.is_double, v.f.restore_bits);
    return 1;
  });
}

int mgh_decompress_masked(const void *compressed_data, size_t compressed_size, const mgh_config *config,
                          void **decompressed_data, int output_pre_allocated) {
  MaskedRead R;  // (the full array)
  R.who = "decompress_masked";
  R.no_footer = "decompress_masked: no mask footer (a plain container has mgh_decompress)";
  return masked_read_entry(compressed_data, compressed_size, config, R, decompressed_data, output_pre_allocated);
}

int mgh_decompress_mask(const void *compressed_data, size_t compressed_size, const mgh_config *config, uint8_t *mask) {
  MaskedRead R;  // (the full array)
  R.no_footer = "decompress_mask: no mask footer";
  return masked_read_mask_entry(compressed_data, compressed_size, config, R, mask);
}

int mgh_decompress_masked_level(const void *compressed_data, size_t compressed_size, int level, void **decompressed_data,
                                const mgh_config *config, int output_pre_allocated) {
  if (level < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "level outside 0 .. l_target");
  MaskedRead R;
  R.kind = ReadKind::level;
  R.level = level;
  return masked_read_entry(compressed_data, compressed_size, config, R, decompressed_data, output_pre_allocated);
}

int mgh_decompress_masked_coarsened(const void *compressed_data, size_t compressed_size, int halvings, void **decompressed_data,
                                    const mgh_config *config, int output_pre_allocated) {
  if (halvings < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, kBadHalvings);
  MaskedRead R;
  R.kind = ReadKind::coarsened;
  R.halvings = halvings;
  return masked_read_entry(compressed_data, compressed_size, config, R, decompressed_data, output_pre_allocated);
}

int mgh_decompress_masked_preview(const void *compressed_data, size_t compressed_size, int halvings, void **decompressed_data,
                                  const mgh_config *config, int output_pre_allocated) {
  if (halvings < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, kBadHalvings);
  MaskedRead R;
  R.kind = ReadKind::preview;
  R.halvings = halvings;
  return masked_read_entry(compressed_data, compressed_size, config, R, decompressed_data, output_pre_allocated);
}

int mgh_decompress_masked_preview_window(const void *compressed_data, size_t compressed_size, int halvings, const uint64_t *lo,
                                         const uint64_t *ext, void **decompressed_data, const mgh_config *config,
                                         int output_pre_allocated) {
  if (!lo || !ext) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (halvings < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, kBadHalvings);
  MaskedRead R;
  R.kind = ReadKind::window;
  R.halvings = halvings;
  R.lo = lo;
  R.ext = ext;
  return masked_read_entry(compressed_data, compressed_size, config, R, decompressed_data, output_pre_allocated);
}

int mgh_decompress_mask_level(const void *compressed_data, size_t compressed_size, int level, const mgh_config *config,
                              uint8_t *mask) {
  if (level < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "level outside 0 .. l_target");
  MaskedRead R;
  R.kind = ReadKind::level;
  R.level = level;
  return masked_read_mask_entry(compressed_data, compressed_size, config, R, mask);
}

int mgh_decompress_mask_coarsened(const void *compressed_data, size_t compressed_size, int halvings, const mgh_config *config,
                                  uint8_t *mask) {
  if (halvings < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, kBadHalvings);
  MaskedRead R;
  R.kind = ReadKind::coarsened;
  R.halvings = halvings;
  return masked_read_mask_entry(compressed_data, compressed_size, config, R, mask);
}

int mgh_decompress_mask_window(const void *compressed_data, size_t compressed_size, const uint64_t *lo, const uint64_t *ext,
                               const mgh_config *config, uint8_t *mask) {
  if (!lo || !ext) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  MaskedRead R;
  R.kind = ReadKind::window;
  R.lo = lo;
  R.ext = ext;
  return masked_read_mask_entry(compressed_data, compressed_size, config, R, mask);
}

int mgh_verify_masked(const void *compressed_data, size_t compressed_size, const void *original, size_t original_bytes,
                      int original_dtype, int halvings, const mgh_config *config, mgh_verify_result *out,
                      uint64_t *n_masked_out) {
  if (!compressed_data || !original || !out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (original_dtype != MGH_FLOAT && original_dtype != MGH_DOUBLE)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_verify_masked: dtype");
  if (halvings < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, kBadHalvings);
  mgh_config cfg;
  HL_TRY(masked_config(config, cfg));
  VerifyJob job;
  job.original = original;
  uint64_t n_total = 0;
  HL_TRY(hl_guarded([&]() -> int {
    MaskedView v;
    HL_TRY(open_or_refuse(masked_open, compressed_data, compressed_size, v,
                          "mgh_verify_masked: no mask footer (a plain container has the plain reader)"));
    n_total = v.n;
    compressed_size = (size_t)v.f.container;
    // the packed mask, whole and complete on the device before the subdomains' lanes read it
    HL_TRY(cache_prepare(cfg.dev_id));
    uint64_t *d_words = nullptr;
    HL_TRY(masked_words(v, g_cache.lane[0].st, &d_words));
    HL_HIP(hipStreamSynchronize(g_cache.lane[0].st));
    job.d_words = d_words;
    return MGH_SUCCESS;
  }));
  void *none = nullptr;  // (there is no output: pre-allocated, and never looked at)
  HL_TRY(decompress_entry(compressed_data, compressed_size, &none, &cfg, 1, original_bytes, original_dtype, -1, halvings, true,
                          nullptr, nullptr, &job));
  mgh_verify_result r{};
  r.stats = job.stats;
  r.bound = job.rel ? job.tol * job.norm : job.tol;
  r.bound_kind = std::isinf(job.s) ? 0 : job.s == 0 ? 1 : -1;
  // s = 0: the writer bounds the sum over ALL elements of the filled array, of which the valid positions are a
  // part -- the divisor is the array's element count, masked ones included
  r.achieved = r.bound_kind == 0   ? r.stats.max_abs_err
               : r.bound_kind == 1 ? (cfg.normalize_coordinates ? std::sqrt(r.stats.sum_sq_err / (double)n_total)
                                                                : std::sqrt(r.stats.sum_sq_err))
                                   : 0.0;
  if (halvings > 0 || r.bound_kind < 0) r.within = -1;  // (a preview carries no bound)
  else r.within = r.stats.nonfinite == 0 && r.achieved <= r.bound ? 1 : 0;
  *out = r;
  if (n_masked_out) *n_masked_out = n_total - r.stats.n;
  return MGH_SUCCESS;
}

} // extern "C"

// ---- pointwise relative error bound: mgh_compress_pwrel and its readers (pwrel_plan.hpp) -------------------
// (capi.hip: the three streaming passes of kernels_pwrel.hpp)
extern "C" int mgh_pwrel_forward_(int D, int dtype, const uint64_t *shape, const void *data, double abs_floor, void *y_out,
                                  uint64_t *mask_words, uint64_t *flag_words, mgh_pwrel_stats *stats, void *stream);
extern "C" int mgh_pwrel_inverse_(int D, int dtype, const uint64_t *shape, const uint64_t *mask_words,
                                  const uint64_t *flag_words, void *data_inout, void *stream);
extern "C" int mgh_pwrel_inverse_sampled_(int D, int dtype, const uint64_t *shape, const uint64_t *mask_words,
                                          const uint64_t *flag_words, const uint64_t *out_shape, const uint32_t *const *d_idx,
                                          void *data_inout, void *stream);
extern "C" int mgh_compare_pwrel_(int D, int dtype, const uint64_t *shape, const void *original, const void *reconstructed,
                                  double abs_floor, mgh_pwrel_compare *out, void *stream);

namespace {

// forward (the array is read once: it stands in for the masked writer's scan) -> statistics -> delta -> the masked
// writer's tail on y (ABS, s = inf, delta; restore_value 0) -> flag record -> footer
int compress_pwrel_impl(int D, int dtype, const uint64_t *shape, double eps, double abs_floor, const void *original,
                        void **compressed, size_t *csize, const void *const *coords, const mgh_config &cfg, bool prealloc) {
  const bool is_double = dtype == MGH_DOUBLE;
  double delta = 0;
  const char *bad_arg = pwrel_abs_tolerance(is_double, eps, -1.0, &delta);
  if (!bad_arg && (!(abs_floor >= 0.0) || std::isinf(abs_floor))) bad_arg = "compress_pwrel: abs_floor must be finite and >= 0";
  MaskedScan S;
  mgh_pwrel_stats *d_stats = nullptr;
  // the array on the device (a host array is uploaded once and transformed in place), and for a device-resident one,
  // which is not modified, y beside it
  HL_TRY(scan_head("compress_pwrel", bad_arg,
                   "compress_pwrel: the array and its transformed copy do not fit max_memory_footprint (such arrays are "
                   "not streamed in parts)",
                   D, dtype, shape, original, cfg, S, &d_stats));
  HlCache &C = g_cache;
  hipStream_t st = C.lane[0].st;
  const uint64_t n = S.n, nb = mask_packed_bytes(n);
  HL_TRY(C.msamp.ensure(nb));
  HL_TRY(C.mfill.ensure(n * (is_double ? 8 : 4)));
  uint64_t *d_flags = (uint64_t *)C.msamp.p;
  const void *x = S.src;
  S.src = C.mfill.p;
  HL_TRY(mgh_pwrel_forward_(D, dtype, shape, x, abs_floor, C.mfill.p, S.d_words, d_flags, d_stats, st));
  mgh_pwrel_stats hs{};
  HL_HIP(hipMemcpyAsync(&hs, d_stats, sizeof(hs), hipMemcpyDeviceToHost, st));
  HL_HIP(hipStreamSynchronize(st));
  S.n_masked = hs.n_masked;
  S.vmin = hs.ymin;
  S.vmax = hs.ymax;
  const double ybound = hs.n_masked >= n ? -1.0 : std::fmax(std::fabs(hs.ymin), std::fabs(hs.ymax));
  if (const char *bad = pwrel_abs_tolerance(is_double, eps, ybound, &delta)) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad);
  const OutSlot slot{compressed, S.in_dev, prealloc};
  // the flag record, like the mask record, and the footer found from the end: at most the packed flag words and the
  // footer, which an allocated output has behind whatever the masked buffer took
  const size_t behind_max = nb + kPwrelFooterBytes, given = prealloc ? *csize : 0;
  size_t masked = given;
  HL_TRY(masked_write("compress_pwrel", D, dtype, shape, delta, std::numeric_limits<double>::infinity(), MGH_ABS, S, 0.0, slot,
                      &masked, coords, cfg, kPwrelFooterBytes, behind_max));
  PwrelFooter f;
  f.masked = masked;
  f.n_flag = hs.n_flag;
  f.eps = eps;
  f.abs_floor = abs_floor;
  return slot.fail(write_trailer("compress_pwrel", ": the output cannot hold masked buffer, flag record and footer", *compressed,
                                 masked, prealloc ? given : masked + behind_max, d_flags, n, hs.n_flag, cfg, st, kPwrelFooterBytes,
                                 [&](uint32_t kind, size_t record, uint32_t crc, uint8_t *dst) {
                                   f.kind = kind;
                                   f.record = record;
                                   f.crc = crc;
                                   pwrel_footer_serialize(f, dst);
                                 },
                                 csize));
}

// A pointwise-relative buffer opened: its footer, the masked buffer in front of it, and the flag record on the host.
struct PwrelView {
  PwrelFooter f;
  MaskedView m;
  std::vector<uint8_t> rec;
};

// 1: such a buffer that passed every check; 0: no footer's magic; negative: a status.
int pwrel_open(const void *buf, size_t size, PwrelView &v) {
  if (size < kPwrelFooterBytes) return 0;
  const bool in_dev = is_device_pointer(buf);
  uint8_t tail[kPwrelFooterBytes];
  HL_TRY(host_piece(tail, buf, in_dev, size - kPwrelFooterBytes, kPwrelFooterBytes));
  if (!pwrel_footer_present(tail, size)) return 0;
  if (const char *bad = pwrel_footer_parse(tail, size, v.f)) return hl_fail(MGH_ERR_FORMAT, bad);
  HL_TRY(open_or_refuse(masked_open, buf, (size_t)v.f.masked, v.m,
                        "pwrel footer: the bytes in front of the flag record are no masked buffer"));
  if (v.m.f.restore_bits != 0) return hl_fail(MGH_ERR_FORMAT, "pwrel footer: the masked buffer's restore value is not +0.0");
  if (const char *bad = pwrel_footer_check_n(v.f, v.m.n)) return hl_fail(MGH_ERR_FORMAT, bad);
  v.rec.resize((size_t)v.f.record);
  HL_TRY(host_piece(v.rec.data(), buf, in_dev, (size_t)v.f.masked, (size_t)v.f.record));
  if (const char *bad = pwrel_record_check_crc(v.f, v.rec.data())) return hl_fail(MGH_ERR_FORMAT, bad);
  return 1;
}

const char *const kNoPwrelFooter =
    ": no pointwise-relative footer (a plain container has mgh_decompress, a masked buffer mgh_decompress_masked)";

// THE RULE of the views: a node of a level or coarsened array takes its class and sign from the
// element of the full array it stands on (sampling, as for masks), a position of a preview or of a window from that
// position of the full array; the value is k_pwrel_inverse's of the y' the same plain reader writes for the
// container part alone. Such an output carries no error bound.
// footer -> the plain reader of the view on the container part -> mask words and flag words of the FULL array ->
// k_pwrel_inverse (the full array, a preview) or k_pwrel_inverse_sampled through the view's node lists
int pwrel_read_impl(const void *buf, size_t size, const mgh_config &cfg, const MaskedRead &R, void **out, bool prealloc) {
  PwrelView v;
  HL_TRY(open_or_refuse(pwrel_open, buf, size, v, std::string(R.who) + kNoPwrelFooter));
  std::vector<uint64_t> oshape;
  std::vector<std::vector<uint32_t>> lists;
  bool sampled = false;
  HL_TRY(masked_read_lists(v.m, cfg, R, oshape, lists, sampled));
  size_t bytes = v.m.hd.is_double ? 8 : 4;
  for (uint64_t e : oshape) bytes *= (size_t)e;
  const uint64_t n = v.m.n;
  const int D = (int)v.m.hd.shape.size();
  return staged_read(
      R.who, buf, bytes, cfg, out, prealloc, [&](void **dst) { return plain_read(R, buf, (size_t)v.m.f.container, cfg, dst); },
      [&](void *d_data, hipStream_t st) -> int {
        HlCache &C = g_cache;
        uint64_t *d_words = nullptr;
        HL_TRY(masked_words(v.m, st, &d_words));
        // (the two records share the symbol buffer and the lossless context of the lane: one after the other)
        if (hipStreamSynchronize(st) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, std::string(R.who) + ": hipStreamSynchronize");
        HL_TRY(C.msamp.ensure(mask_packed_bytes(n)));
        HL_TRY(bitmap_words(v.f.kind, v.rec, n, v.m.lossless, C.msamp.p, st));
        const uint64_t *d_flags = (const uint64_t *)C.msamp.p;
        if (!sampled) return mgh_pwrel_inverse_(D, v.m.dtype, v.m.hd.shape.data(), d_words, d_flags, d_data, st);
        const uint32_t *d_idx[MGH_MAX_DIM];
        HL_TRY(upload_lists(lists, st, d_idx));
        return mgh_pwrel_inverse_sampled_(D, v.m.dtype, v.m.hd.shape.data(), d_words, d_flags, oshape.data(), d_idx, d_data, st);
      });
}

int pwrel_read_entry(const void *buf, size_t size, const mgh_config *config, const MaskedRead &R, void **out, int prealloc) {
  if (!buf || !out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (prealloc && !*out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  mgh_config cfg;
  HL_TRY(masked_config(config, cfg));
  return hl_guarded([&] { return pwrel_read_impl(buf, size, cfg, R, out, prealloc != 0); });
}

struct DeviceTemp {
  void *p = nullptr;
  ~DeviceTemp() {
    if (p) (void)hipFree(p);
  }
};

// decode the whole array into a device buffer, then one pass of k_compare_pwrel against the original
int verify_pwrel_impl(const void *buf, size_t size, const void *original, size_t original_bytes, int original_dtype,
                      const mgh_config &cfg, mgh_pwrel_compare *out, int *within) {
  PwrelView v;
  HL_TRY(open_or_refuse(pwrel_open, buf, size, v, std::string("mgh_verify_pwrel") + kNoPwrelFooter));
  const uint64_t n = v.m.n;
  const size_t bytes = (size_t)n * (v.m.hd.is_double ? 8 : 4);
  if (original_dtype != v.m.dtype) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_verify_pwrel: the original's dtype is not the buffer's");
  if (original_bytes != bytes) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_verify_pwrel: original_bytes is not the array's size");
  HL_TRY(cache_prepare(cfg.dev_id));
  DeviceTemp recon, staged;
  HL_HIP(hipMalloc(&recon.p, bytes));
  void *dst = recon.p;
  MaskedRead full;  // (the full array)
  full.who = "mgh_verify_pwrel";
  HL_TRY(pwrel_read_impl(buf, size, cfg, full, &dst, true));
  hipStream_t st = g_cache.lane[0].st;
  const void *d_orig = original;
  if (!is_device_pointer(original)) {
    HL_HIP(hipMalloc(&staged.p, bytes));
    HL_TRY(copy_any(staged.p, original, bytes, st));
    d_orig = staged.p;
  }
  mgh_pwrel_compare r{};
  HL_TRY(mgh_compare_pwrel_((int)v.m.hd.shape.size(), v.m.dtype, v.m.hd.shape.data(), d_orig, recon.p, v.f.abs_floor, &r, st));
  *out = r;
  if (within)
    *within = r.max_rel_err <= v.f.eps && r.n_class_mismatch == 0 && r.n_sign_mismatch == 0 &&
                      r.max_zeroed_abs < pwrel_floor_eff(v.m.hd.is_double, v.f.abs_floor)
                  ? 1
                  : 0;
  return MGH_SUCCESS;
}

} // namespace

extern "C" {

int mgh_compress_pwrel(int D, int dtype, const uint64_t *shape, double eps, double abs_floor, const void *original_data,
                       void **compressed_data, size_t *compressed_size, const void *const *coords, const mgh_config *config,
                       int output_pre_allocated) {
  if (!compressed_data || !compressed_size) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  HL_TRY(size_call_args(D, dtype, shape, MGH_ABS, original_data, config, output_pre_allocated ? compressed_data : nullptr));
  return hl_guarded([&]() -> int {
    return compress_pwrel_impl(D, dtype, shape, eps, abs_floor, original_data, compressed_data, compressed_size, coords, *config,
                               output_pre_allocated != 0);
  });
}

int mgh_pwrel_info(const void *compressed_data, size_t compressed_size, struct mgh_pwrel_info *info) {
  if (!compressed_data || !info) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  return hl_guarded([&]() -> int {
    PwrelView v;
    const int opened = pwrel_open(compressed_data, compressed_size, v);
    if (opened <= 0) return opened;
    info->eps = v.f.eps;
    info->abs_floor = v.f.abs_floor;
    info->delta = v.m.hd.tol;
    info->n_masked = v.m.f.n_masked;
    info->n_flag = v.f.n_flag;
    info->container_size = v.m.f.container;
    info->masked_size = v.f.masked;
    info->mask_record_size = v.m.f.record;
    info->flag_record_size = v.f.record;
    info->mask_kind = (int)v.m.f.kind;
    info->flag_kind = (int)v.f.kind;
    return 1;
  });
}

int mgh_decompress_pwrel(const void *compressed_data, size_t compressed_size, const mgh_config *config,
                         void **decompressed_data, int output_pre_allocated) {
  MaskedRead R;  // (the full array)
  R.who = "decompress_pwrel";
  return pwrel_read_entry(compressed_data, compressed_size, config, R, decompressed_data, output_pre_allocated);
}

int mgh_decompress_pwrel_level(const void *compressed_data, size_t compressed_size, int level, void **decompressed_data,
                               const mgh_config *config, int output_pre_allocated) {
  if (level < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "level outside 0 .. l_target");
  MaskedRead R;
  R.kind = ReadKind::level;
  R.level = level;
  R.who = "decompress_pwrel_level";
  return pwrel_read_entry(compressed_data, compressed_size, config, R, decompressed_data, output_pre_allocated);
}

int mgh_decompress_pwrel_coarsened(const void *compressed_data, size_t compressed_size, int halvings, void **decompressed_data,
                                   const mgh_config *config, int output_pre_allocated) {
  if (halvings < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, kBadHalvings);
  MaskedRead R;
  R.kind = ReadKind::coarsened;
  R.halvings = halvings;
  R.who = "decompress_pwrel_coarsened";
  return pwrel_read_entry(compressed_data, compressed_size, config, R, decompressed_data, output_pre_allocated);
}

int mgh_decompress_pwrel_preview(const void *compressed_data, size_t compressed_size, int halvings, void **decompressed_data,
                                 const mgh_config *config, int output_pre_allocated) {
  if (halvings < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, kBadHalvings);
  MaskedRead R;
  R.kind = ReadKind::preview;
  R.halvings = halvings;
  R.who = "decompress_pwrel_preview";
  return pwrel_read_entry(compressed_data, compressed_size, config, R, decompressed_data, output_pre_allocated);
}

int mgh_decompress_pwrel_preview_window(const void *compressed_data, size_t compressed_size, int halvings, const uint64_t *lo,
                                        const uint64_t *ext, void **decompressed_data, const mgh_config *config,
                                        int output_pre_allocated) {
  if (!lo || !ext) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (halvings < 0) return hl_fail(MGH_ERR_INVALID_ARGUMENT, kBadHalvings);
  MaskedRead R;
  R.kind = ReadKind::window;
  R.halvings = halvings;
  R.lo = lo;
  R.ext = ext;
  R.who = "decompress_pwrel_preview_window";
  return pwrel_read_entry(compressed_data, compressed_size, config, R, decompressed_data, output_pre_allocated);
}

int mgh_verify_pwrel(const void *compressed_data, size_t compressed_size, const void *original, size_t original_bytes,
                     int original_dtype, const mgh_config *config, mgh_pwrel_compare *out, int *within) {
  if (!compressed_data || !original || !out) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (original_dtype != MGH_FLOAT && original_dtype != MGH_DOUBLE)
    return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_verify_pwrel: dtype");
  mgh_config cfg;
  HL_TRY(masked_config(config, cfg));
  return hl_guarded([&] {
    return verify_pwrel_impl(compressed_data, compressed_size, original, original_bytes, original_dtype, cfg, out, within);
  });
}

} // extern "C"

// ---- region of interest: mgh_compress_roi and its readers (roi_plan.hpp) ------------------------------------
// (capi.hip: the two streaming passes of kernels_roi.hpp)
extern "C" size_t mgh_box_scratch_bytes_(void);
extern "C" int mgh_box_residual_(int D, int dtype, const uint64_t *shape, const uint64_t *lo, const uint64_t *ext, const void *x,
                                 const void *b, void *r_out, void *d_scratch, void *stream);
extern "C" int mgh_box_add_(int D, int dtype, const uint64_t *shape, const uint64_t *lo, const uint64_t *ext, const void *r,
                            void *data_inout, void *stream);

namespace {

struct RoiBoxStats {  // (kernels_roi.hpp: BoxStats)
  double max_abs_r, max_abs_x;
  uint64_t n_nonfinite, pad;
};

// the absolute bound a tolerance of the container `hd` stands for: mgh_verify's rule
inline double roi_abs_factor(const fmt::Header &hd) { return hd.rel ? hd.norm : 1.0; }

// C0 = mgh_compress(x, tol) into the output -> its header (the norm of a REL bound) -> b = mgh_decompress(C0) on
// the device -> per box: residual and statistics in one pass -> tolres -> mgh_compress of the residual -> the
// records, the table and the footer behind C0
int compress_roi_impl(int D, int dtype, const uint64_t *shape, double tol, double s, int ebtype, const void *original,
                      std::vector<RoiBox> &B, void **compressed, size_t *csize, const void *const *coords, const mgh_config &cfg,
                      bool prealloc) {
  const bool is_double = dtype == MGH_DOUBLE;
  const size_t elem = is_double ? 8 : 4;
  const int nbox = (int)B.size();
  uint64_t n = 1, box_max = 0, box_sum = 0;
  for (int d = 0; d < D; d++) n *= shape[d];
  for (const RoiBox &b : B) {
    box_max = std::max(box_max, roi_box_elems(b));
    box_sum += roi_box_elems(b);
  }
  const size_t bytes = (size_t)n * elem;
  if (const char *bad = roi_check_footprint(bytes, cfg.max_memory_footprint)) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad);
  const bool in_dev = is_device_pointer(original);
  HL_TRY(cache_prepare(cfg.dev_id));
  HlCache &C = g_cache;
  hipStream_t st = C.lane[0].st;
  // the output: mgh_compress's own capacity for C0 and for every residual, the table and the footer
  const size_t trailer = (size_t)nbox * kRoiEntryBytes + kRoiFooterBytes, slack = (size_t)1e6;
  const OutSlot slot{compressed, in_dev, prealloc};
  size_t cap = 0;
  if (prealloc) {
    cap = *csize;
    if (cap <= trailer) return hl_fail(MGH_ERR_OUTPUT_TOO_LARGE, "compress_roi: the output cannot hold the box table and the footer");
  } else {
    cap = bytes + slack + box_sum * elem + (size_t)nbox * slack + trailer;
    HL_TRY(slot.alloc(cap));
  }
  void *out = *slot.slot;
  size_t container = prealloc ? cap - trailer : bytes + slack;
  int rc = mgh_compress(D, dtype, shape, tol, s, ebtype, original, &out, &container, coords, &cfg, 1);
  if (rc != MGH_SUCCESS) return slot.fail(rc);
  fmt::Header hd;
  size_t meta = 0;
  if ((rc = read_header(out, container, hd, meta)) != MGH_SUCCESS) return slot.fail(rc);
  const double factor = roi_abs_factor(hd);
  // x on the device (a host array is uploaded once), b beside it, the residual of one box and the statistics
  const void *x = original;
  if (!in_dev) {
    if ((rc = C.mfill.ensure(bytes)) != MGH_SUCCESS) return slot.fail(rc);
    if ((rc = copy_any(C.mfill.p, original, bytes, st)) != MGH_SUCCESS) return slot.fail(rc);
    x = C.mfill.p;
  }
  if ((rc = C.msamp.ensure(bytes)) != MGH_SUCCESS || (rc = C.msym.ensure((size_t)box_max * elem)) != MGH_SUCCESS ||
      (rc = C.mwords.ensure(mgh_box_scratch_bytes_())) != MGH_SUCCESS)
    return slot.fail(rc);
  void *b = C.msamp.p;
  if ((rc = mgh_decompress(out, container, &b, &cfg, 1)) != MGH_SUCCESS) return slot.fail(rc);
  // the residual: the caller's configuration (lossless stage, dictionary, chunk) without its domain decomposition --
  // a box is a small array of its own, cut only where the footprint asks (the default)
  mgh_config rcfg = cfg;
  rcfg.domain_decomposition = MGH_DD_MAXDIM;
  rcfg.domain_decomposition_dim = 0;
  rcfg.domain_decomposition_sizes = nullptr;
  rcfg.num_domain_decomposition_sizes = 0;
  std::vector<uint8_t> tail;
  uint64_t at = container;
  for (int i = 0; i < nbox; i++) {
    RoiBox &bx = B[i];
    const uint64_t *lo = bx.lo + (kRoiMaxDim - D), *ext = bx.ext + (kRoiMaxDim - D);
    if ((rc = mgh_box_residual_(D, dtype, shape, lo, ext, x, b, C.msym.p, C.mwords.p, st)) != MGH_SUCCESS) return slot.fail(rc);
    RoiBoxStats hs{};
    if (hipMemcpyAsync(&hs, C.mwords.p, sizeof(hs), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return slot.fail(hl_fail(MGH_ERR_DEVICE, "compress_roi: reading the box statistics back"));
    if (hs.n_nonfinite)
      return slot.fail(hl_fail(MGH_ERR_INVALID_ARGUMENT,
                               "compress_roi: a box holds a non-finite value (masked arrays with boxes are not built)"));
    if (const char *bad = roi_tolres(is_double, bx.tol * factor, hs.max_abs_r, hs.max_abs_x, &bx.tolres))
      return slot.fail(hl_fail(MGH_ERR_INVALID_ARGUMENT, std::string("compress_") + bad));
    bx.offset = at;
    bx.size = 0;
    bx.crc = fmt::crc32(nullptr, 0);
    if (hs.max_abs_r == 0) continue;  // the base is exact in the box: nothing is stored
    void *rec = nullptr;  // (device memory: the residual's own space)
    size_t rsize = 0;
    rc = mgh_compress(D, dtype, ext, bx.tolres, std::numeric_limits<double>::infinity(), MGH_ABS, C.msym.p, &rec, &rsize, nullptr,
                      &rcfg, 0);
    if (rc != MGH_SUCCESS) return slot.fail(rc);
    const size_t had = tail.size();
    tail.resize(had + rsize);
    rc = dev_to_host(tail.data() + had, rec, rsize);
    (void)hipFree(rec);
    if (rc != MGH_SUCCESS) return slot.fail(rc);
    bx.size = rsize;
    bx.crc = fmt::crc32(tail.data() + had, rsize);
    at += rsize;
  }
  const std::vector<uint8_t> tf = roi_trailer_serialize(container, B);
  tail.insert(tail.end(), tf.begin(), tf.end());
  if (container + tail.size() > cap)
    return slot.fail(hl_fail(MGH_ERR_OUTPUT_TOO_LARGE, "compress_roi: the output cannot hold container, box records, table and footer"));
  if (is_device_pointer(out)) {
    if (hipMemcpyAsync((char *)out + container, tail.data(), tail.size(), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return slot.fail(hl_fail(MGH_ERR_DEVICE, "compress_roi: writing box records, table and footer"));
  } else {
    std::memcpy((char *)out + container, tail.data(), tail.size());
  }
  *csize = container + tail.size();
  return MGH_SUCCESS;
}

// A buffer with boxes opened: the footer, the table, and the header of the container in front of them.
struct RoiView {
  RoiFooter f;
  std::vector<RoiBox> boxes;
  fmt::Header hd;
  uint64_t n = 0;
  int dtype = MGH_FLOAT;
  std::vector<std::vector<uint8_t>> recs;  // the records on the host, where their CRC-32 is checked
};

// 1: such a buffer that passed every check; 0: no footer's magic; negative: a status.
int roi_open(const void *buf, size_t size, RoiView &v) {
  if (size < kRoiFooterBytes) return 0;
  const bool in_dev = is_device_pointer(buf);
  uint8_t tail[kRoiFooterBytes];
  HL_TRY(host_piece(tail, buf, in_dev, size - kRoiFooterBytes, kRoiFooterBytes));
  if (!roi_footer_present(tail, size)) return 0;
  if (const char *bad = roi_footer_parse(tail, size, v.f)) return hl_fail(MGH_ERR_FORMAT, bad);
  std::vector<uint8_t> table((size_t)v.f.table_bytes);
  HL_TRY(host_piece(table.data(), buf, in_dev, size - kRoiFooterBytes - table.size(), table.size()));
  if (const char *bad = roi_table_parse(v.f, table.data(), size, v.boxes)) return hl_fail(MGH_ERR_FORMAT, bad);
  size_t meta = 0;
  HL_TRY(read_header(buf, (size_t)v.f.container, v.hd, meta));
  if (v.hd.shape.empty() || v.hd.shape.size() > MGH_MAX_DIM) return hl_fail(MGH_ERR_FORMAT, "header: dimension");
  v.n = 1;
  for (uint64_t e : v.hd.shape) {
    if (e == 0 || e > 0xffffffffull || v.n * e > 0xffffffffull) return hl_fail(MGH_ERR_FORMAT, "roi footer: an array of 2^32 elements or more");
    v.n *= e;
  }
  v.dtype = v.hd.is_double ? MGH_DOUBLE : MGH_FLOAT;
  if (const char *bad = roi_table_check_shape(v.boxes, (int)v.hd.shape.size(), v.hd.shape.data())) return hl_fail(MGH_ERR_FORMAT, bad);
  v.recs.resize(v.boxes.size());
  for (size_t i = 0; i < v.boxes.size(); i++) {
    const RoiBox &b = v.boxes[i];
    v.recs[i].resize((size_t)b.size);
    HL_TRY(host_piece(v.recs[i].data(), buf, in_dev, (size_t)b.offset, (size_t)b.size));
    if (const char *bad = roi_record_check_crc(b, v.recs[i].data())) return hl_fail(MGH_ERR_FORMAT, bad);
  }
  return 1;
}

const char *const kNoRoiFooter =
    ": no box footer (a plain container has mgh_decompress, a masked buffer mgh_decompress_masked, a pointwise-relative "
    "one mgh_decompress_pwrel)";

// An opened buffer: the plain reader on the first C bytes -> per box with a record: its plain reader into the lane
// buffer, k_box_add into the box
int roi_read_view(const char *who, const RoiView &v, const void *buf, const mgh_config &cfg, void **out, bool prealloc) {
  const int D = (int)v.hd.shape.size();
  const size_t elem = v.hd.is_double ? 8 : 4, bytes = (size_t)v.n * elem;
  return staged_read(
      who, buf, bytes, cfg, out, prealloc, [&](void **dst) { return mgh_decompress(buf, (size_t)v.f.container, dst, &cfg, 1); },
      [&](void *d_data, hipStream_t st) -> int {
        HlCache &C = g_cache;
        for (size_t i = 0; i < v.boxes.size(); i++) {
          const RoiBox &b = v.boxes[i];
          if (b.size == 0) continue;
          const uint64_t *lo = b.lo + (kRoiMaxDim - D), *ext = b.ext + (kRoiMaxDim - D);
          // (the lane buffer is read by the previous box's pass: one after the other)
          if (hipStreamSynchronize(st) != hipSuccess) return hl_fail(MGH_ERR_DEVICE, std::string(who) + ": hipStreamSynchronize");
          HL_TRY(C.msym.ensure((size_t)roi_box_elems(b) * elem));
          // (the record's checked host copy: a record starts wherever the one before it ended, and the plain reader
          // of a device buffer reads code units in place)
          const void *rec = v.recs[i].data();
          fmt::Header rh;
          size_t meta = 0;
          HL_TRY(read_header(rec, (size_t)b.size, rh, meta));
          if (rh.is_double != v.hd.is_double || rh.shape.size() != (size_t)D || !std::equal(rh.shape.begin(), rh.shape.end(), ext))
            return hl_fail(MGH_ERR_FORMAT, "roi record: the container does not hold the box's residual");
          void *lane = C.msym.p;
          HL_TRY(mgh_decompress(rec, (size_t)b.size, &lane, &cfg, 1));
          HL_TRY(mgh_box_add_(D, v.dtype, v.hd.shape.data(), lo, ext, C.msym.p, d_data, st));
        }
        return MGH_SUCCESS;
      });
}

int roi_read_impl(const char *who, const void *buf, size_t size, const mgh_config &cfg, void **out, bool prealloc) {
  RoiView v;
  HL_TRY(open_or_refuse(roi_open, buf, size, v, std::string(who) + kNoRoiFooter));
  return roi_read_view(who, v, buf, cfg, out, prealloc);
}

// decode the whole array into a device buffer, then mgh_compare's reduction over the array and over every box
int verify_roi_impl(const void *buf, size_t size, const void *original, size_t original_bytes, int original_dtype,
                    const mgh_config &cfg, mgh_verify_result *whole, mgh_verify_result *per_box) {
  RoiView v;
  HL_TRY(open_or_refuse(roi_open, buf, size, v, std::string("mgh_verify_roi") + kNoRoiFooter));
  const int D = (int)v.hd.shape.size();
  const size_t elem = v.hd.is_double ? 8 : 4, bytes = (size_t)v.n * elem;
  if (original_dtype != v.dtype) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_verify_roi: the original's dtype is not the buffer's");
  if (original_bytes != bytes) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_verify_roi: original_bytes is not the array's size");
  HL_TRY(cache_prepare(cfg.dev_id));
  DeviceTemp recon, staged, scratch;
  HL_HIP(hipMalloc(&recon.p, bytes));
  HL_HIP(hipMalloc(&scratch.p, mgh_compare_scratch_bytes_()));
  void *dst = recon.p;
  HL_TRY(roi_read_view("mgh_verify_roi", v, buf, cfg, &dst, true));  // (the view opened above: the records are read once)
  hipStream_t st = g_cache.lane[0].st;
  const void *d_orig = original;
  if (!is_device_pointer(original)) {
    HL_HIP(hipMalloc(&staged.p, bytes));
    HL_TRY(copy_any(staged.p, original, bytes, st));
    d_orig = staged.p;
  }
  uint64_t str[MGH_MAX_DIM], run = 1;
  for (int d = D - 1; d >= 0; d--) {
    str[d] = run;
    run *= v.hd.shape[d];
  }
  const double factor = roi_abs_factor(v.hd);
  auto compare = [&](const uint64_t *ext, uint64_t at, bool strided, double bound, mgh_verify_result *res) -> int {
    HL_TRY(mgh_compare_device_(D, v.dtype, ext, (const char *)d_orig + at * elem, strided ? str : nullptr,
                               (const char *)recon.p + at * elem, strided ? str : nullptr, scratch.p, st));
    mgh_verify_result r{};
    HL_HIP(hipMemcpyAsync(&r.stats, scratch.p, sizeof(r.stats), hipMemcpyDeviceToHost, st));
    HL_HIP(hipStreamSynchronize(st));
    r.bound_kind = 0;
    r.bound = bound;
    r.achieved = r.stats.max_abs_err;
    r.within = r.stats.nonfinite == 0 && r.achieved <= r.bound ? 1 : 0;
    *res = r;
    return MGH_SUCCESS;
  };
  HL_TRY(compare(v.hd.shape.data(), 0, false, v.hd.tol * factor, whole));
  for (size_t i = 0; per_box && i < v.boxes.size(); i++) {
    const RoiBox &b = v.boxes[i];
    uint64_t at = 0;
    for (int d = 0; d < D; d++) at += b.lo[kRoiMaxDim - D + d] * str[d];
    HL_TRY(compare(b.ext + (kRoiMaxDim - D), at, true, b.tol * factor, per_box + i));
  }
  return MGH_SUCCESS;
}

} // namespace

extern "C" {

int mgh_compress_roi(int D, int dtype, const uint64_t *shape, double tol, double s, int ebtype, const void *original_data,
                     int nbox, const mgh_roi_box *boxes, void **compressed_data, size_t *compressed_size,
                     const void *const *coords, const mgh_config *config, int output_pre_allocated) {
  if (!compressed_data || !compressed_size || !boxes || !shape || !original_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  // the rules of the boxes (roi_plan.hpp) come before anything that needs a device
  std::vector<RoiBox> B;
  for (int i = 0; i < nbox && i < kRoiMaxBoxes && D >= 1 && D <= MGH_MAX_DIM; i++)
    B.push_back(roi_box(D, boxes[i].lo, boxes[i].ext, boxes[i].tol));
  if (const char *bad = roi_check_boxes(D, shape, tol, s, nbox, B.data())) return hl_fail(MGH_ERR_INVALID_ARGUMENT, bad);
  HL_TRY(size_call_args(D, dtype, shape, ebtype, original_data, config, output_pre_allocated ? compressed_data : nullptr));
  return hl_guarded([&]() -> int {
    return compress_roi_impl(D, dtype, shape, tol, s, ebtype, original_data, B, compressed_data, compressed_size, coords,
                             *config, output_pre_allocated != 0);
  });
}

int mgh_decompress_roi(const void *compressed_data, size_t compressed_size, void **decompressed_data, const mgh_config *config,
                       int output_pre_allocated) {
  if (!compressed_data || !decompressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (output_pre_allocated && !*decompressed_data) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "pre-allocated output is NULL");
  mgh_config cfg;
  HL_TRY(masked_config(config, cfg));
  return hl_guarded([&] {
    return roi_read_impl("decompress_roi", compressed_data, compressed_size, cfg, decompressed_data, output_pre_allocated != 0);
  });
}

int mgh_roi_info(const void *compressed_data, size_t compressed_size, struct mgh_roi_info *info) {
  if (!compressed_data || !info) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  return hl_guarded([&]() -> int {
    RoiView v;
    const int opened = roi_open(compressed_data, compressed_size, v);
    if (opened <= 0) return opened;
    const int D = (int)v.hd.shape.size();
    std::memset(info, 0, sizeof(*info));
    info->container_size = v.f.container;
    info->nbox = (int)v.boxes.size();
    info->D = D;
    for (size_t i = 0; i < v.boxes.size(); i++) {
      for (int d = 0; d < D; d++) {
        info->box[i].lo[d] = v.boxes[i].lo[kRoiMaxDim - D + d];
        info->box[i].ext[d] = v.boxes[i].ext[kRoiMaxDim - D + d];
      }
      info->box[i].tol = v.boxes[i].tol;
      info->box[i].tolres = v.boxes[i].tolres;
      info->box[i].record_size = v.boxes[i].size;
    }
    return 1;
  });
}

int mgh_verify_roi(const void *compressed_data, size_t compressed_size, const void *original, size_t original_bytes,
                   int original_dtype, const mgh_config *config, mgh_verify_result *whole, mgh_verify_result *per_box) {
  if (!compressed_data || !original || !whole) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "NULL argument");
  if (original_dtype != MGH_FLOAT && original_dtype != MGH_DOUBLE) return hl_fail(MGH_ERR_INVALID_ARGUMENT, "mgh_verify_roi: dtype");
  mgh_config cfg;
  HL_TRY(masked_config(config, cfg));
  return hl_guarded([&] {
    return verify_roi_impl(compressed_data, compressed_size, original, original_bytes, original_dtype, cfg, whole, per_box);
  });
}

} // extern "C"
