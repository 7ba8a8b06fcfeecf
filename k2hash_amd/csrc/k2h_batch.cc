// k2hash_amd -- batch C-ABI (include/k2hash_amd.h section 2) over the HIP kernels.
//
// Device-pointer entry points validate arguments and launch on the caller's stream.
// Host-pointer entry points stage through pinned buffers and pipeline
// host-copy -> H2D -> kernel -> D2H over two streams in chunks, so a caller that holds
// keys in host memory (the k2hash process itself) gets the PCIe-bound rate without
// managing device memory.  HIP is touched only inside these calls (lazy init), never at
// library load, so libk2hash can dlopen this library as its plugin safely.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/k2hash_amd.h"
#include "k2h_fnv_device.h"
#include "k2h_kernels.h"

namespace {

thread_local char g_err[256];


int fail(int code, const char* what, hipError_t e = hipSuccess) {
  if (e != hipSuccess)
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(g_err, sizeof g_err, "%s", what);
  return code;
}

uint64_t seed_for(uint32_t flags) {
  return (flags & K2H_AMD_FLAG_STD_FNV) ? k2h::kSeedStd : k2h::kSeedBuiltin;
}

// A launcher's K2H_AMD_EINVAL: the `bytes` it counted for `what` do not fit the caller's out_cap.
int exceeds_cap(const char* who, const char* what, uint64_t bytes, uint64_t cap) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: the %llu bytes of the %s exceed out_cap %llu", who, (unsigned long long)bytes, what,
           (unsigned long long)cap);
  return fail(K2H_AMD_EINVAL, msg);
}

// The whole answer of a call over nothing: its one offset, 0, written on the stream.
int clear_word(uint64_t* word, void* stream, const char* what) {
  const hipError_t e = hipMemsetAsync(word, 0, 8, (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, what, e);
}

// ---------------------------------------------------------------------------
// Device gate (include/k2hash_amd.h: K2H_AMD_ENODEV = "no usable gfx950 device").  The
// library carries gfx950 code objects only, so every entry point that launches checks the
// device's architecture once (cached per device) and returns ENODEV before any launch on a
// device without a gfx950 ISA.  K2H_AMD_TEST_ARCH, read once per process, replaces the name
// the runtime reports: a test hook that lets a gfx950 box exercise the refusal.
// ---------------------------------------------------------------------------
constexpr int kMaxDevices = 64;
std::atomic<int8_t> g_arch_ok[kMaxDevices];  // 0 unknown, 1 gfx950, -1 other

int gate_device(int device) {
  if (device < 0 || device >= kMaxDevices) return fail(K2H_AMD_EINVAL, "device index out of range");
  int8_t s = g_arch_ok[device].load(std::memory_order_relaxed);
  if (s == 0) {
    static const char* forced = getenv("K2H_AMD_TEST_ARCH");
    char name[256] = {0};
    if (forced) {
      snprintf(name, sizeof name, "%s", forced);
    } else {
      hipDeviceProp_t p;
      hipError_t e = hipGetDeviceProperties(&p, device);
      if (e != hipSuccess) return fail(K2H_AMD_ENODEV, "hipGetDeviceProperties", e);
      snprintf(name, sizeof name, "%s", p.gcnArchName);
    }
    // gcnArchName is "gfx950" or "gfx950:sramecc+:xnack-": the processor name before ':'
    s = (strncmp(name, "gfx950", 6) == 0 && (name[6] == 0 || name[6] == ':')) ? 1 : -1;
    g_arch_ok[device].store(s, std::memory_order_relaxed);
  }
  if (s < 0) return fail(K2H_AMD_ENODEV, "device is not gfx950 (this library holds gfx950 code only)");
  return K2H_AMD_OK;
}

// The caller's current device (device-pointer entry points launch there).
int gate_current() {
  int d = -1;
  hipError_t e = hipGetDevice(&d);
  if (e != hipSuccess) return fail(K2H_AMD_ENODEV, "no HIP device", e);
  return gate_device(d);
}

#define K2H_GATE()                          \
  do {                                      \
    if (int gate_rc_ = gate_current())      \
      return gate_rc_;                      \
  } while (0)

// ---------------------------------------------------------------------------
// Parallel host copies for the staging pipeline.  One core's memcpy into pinned memory
// runs at ~16 GB/s on the MI355X hosts, a third of PCIe (57 GB/s measured,
// tools/host_rate.py), so staging copies are split over a small worker pool.  The pool
// is created on the first host-path call (never at library load) and re-created in a
// forked child, whose copy of the pool has no threads.
// ---------------------------------------------------------------------------
class CopyPool {
 public:
  void copy(void* dst, const void* src, size_t len) {
    if (len < (4u << 20) || nthreads() <= 1) {
      memcpy(dst, src, len);
      return;
    }
    std::unique_lock<std::mutex> lk(mu_);
    ensure();
    dst_ = (uint8_t*)dst;
    src_ = (const uint8_t*)src;
    len_ = len;
    piece_ = std::max<size_t>(1u << 20, (len + 4 * (nworkers_ + 1) - 1) / (4 * (nworkers_ + 1)));
    piece_ = (piece_ + 4095) & ~(size_t)4095;
    next_.store(0);
    busy_ = nworkers_;
    ++gen_;
    cv_.notify_all();
    lk.unlock();
    run();  // the caller copies too
    lk.lock();
    done_cv_.wait(lk, [&] { return busy_ == 0; });
  }

 private:
  static int nthreads() {
    static int n = [] {
      const char* e = getenv("K2H_AMD_COPY_THREADS");
      int v = e ? atoi(e) : (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency() / 2));
      return v < 1 ? 1 : v;
    }();
    return n;
  }
  void ensure() {
    if (pid_ == getpid() && nworkers_) return;
    // (re)start: in a forked child the parent's workers do not exist.  Workers are
    // detached and the pool is never destroyed (see pool()), so process exit neither
    // joins nor terminates them.
    nworkers_ = 0;
    pid_ = getpid();
    gen_ = 0;
    for (int i = 0; i < nthreads() - 1; ++i, ++nworkers_)
      std::thread([this] {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
          cv_.wait(lk, [&] { return gen_ != seen; });
          seen = gen_;
          lk.unlock();
          run();
          lk.lock();
          if (--busy_ == 0) done_cv_.notify_all();
        }
      }).detach();
  }
  void run() {
    for (;;) {
      size_t off = next_.fetch_add(piece_);
      if (off >= len_) return;
      memcpy(dst_ + off, src_ + off, std::min(piece_, len_ - off));
    }
  }
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  size_t nworkers_ = 0;
  pid_t pid_ = 0;
  uint64_t gen_ = 0;
  size_t busy_ = 0;
  uint8_t* dst_ = nullptr;
  const uint8_t* src_ = nullptr;
  size_t len_ = 0, piece_ = 0;
  std::atomic<size_t> next_{0};
};

CopyPool& pool() {
  static CopyPool* p = new CopyPool;  // never destroyed: detached workers may outlive statics
  return *p;
}

// ---------------------------------------------------------------------------
// Host-path pipeline: per device, two slots used alternately, one stream each.
//  - in:  the caller's keys are copied into the slot's pinned staging buffer by the copy
//         pool (8+ threads: ~119 GB/s, tools/host_probe.hip) while the previous chunk's
//         H2D DMA runs, then DMA'd at the PCIe rate (57.5 GB/s).  Handing the runtime the
//         caller's pageable buffer instead makes it pin the whole allocation on every call
//         (~40 ms per 512 MiB, rocprofv3 --sys-trace of tools/host_trace.py).
//  - out: fixed-length keys: the kernel stores the hashes straight into the slot's pinned
//         output buffer over PCIe (a wave writes whole lines), so no D2H copy queues behind
//         the next chunk's H2D on the DMA engine; CSR keys (hashes stored in length-sorted
//         order, partial lines) come back with a D2H copy.  The pool then copies them to
//         the caller when the slot is reused or the call ends.
// ---------------------------------------------------------------------------
struct Slot {
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;
  uint8_t* h_in = nullptr;   // pinned input bytes
  uint64_t* h_off = nullptr; // pinned offsets (CSR)
  uint64_t* h_out = nullptr; // pinned h1 (+h2) results
  uint64_t* h_out_dev = nullptr; // the same buffer as a device pointer (kernel stores)
  uint8_t* d_in = nullptr;
  uint64_t* d_off = nullptr;
  uint64_t* d_out = nullptr;
  uint64_t cap_in = 0, cap_keys = 0;
  bool busy = false;
  // pending result copy-out
  uint64_t first = 0, count = 0;
  bool want_h2 = false;
};

struct HostCtx {
  std::mutex mu;
  Slot slot[2];
};

HostCtx g_ctx[64];

int slot_reserve(Slot& s, uint64_t bytes, uint64_t keys) {
  hipError_t e;
  if (!s.stream) {
    if ((e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking)) != hipSuccess)
      return fail(K2H_AMD_EHIP, "hipStreamCreate", e);
    if ((e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess)
      return fail(K2H_AMD_EHIP, "hipEventCreate", e);
  }
  if (bytes > s.cap_in) {
    if (s.h_in) (void)hipHostFree(s.h_in);
    if (s.d_in) (void)hipFree(s.d_in);
    s.h_in = nullptr;
    s.d_in = nullptr;
    s.cap_in = 0;
    if (hipHostMalloc((void**)&s.h_in, bytes, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void**)&s.d_in, bytes) != hipSuccess)
      return fail(K2H_AMD_ENOMEM, "staging allocation (bytes)");
    s.cap_in = bytes;
  }
  if (keys > s.cap_keys) {
    if (s.h_off) (void)hipHostFree(s.h_off);
    if (s.h_out) (void)hipHostFree(s.h_out);
    if (s.d_off) (void)hipFree(s.d_off);
    if (s.d_out) (void)hipFree(s.d_out);
    s.h_off = nullptr;
    s.h_out = nullptr;
    s.h_out_dev = nullptr;
    s.d_off = nullptr;
    s.d_out = nullptr;
    s.cap_keys = 0;
    if (hipHostMalloc((void**)&s.h_off, (keys + 1) * 8, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&s.h_out, keys * 16, hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void**)&s.d_off, (keys + 1) * 8) != hipSuccess || hipMalloc((void**)&s.d_out, keys * 16) != hipSuccess)
      return fail(K2H_AMD_ENOMEM, "staging allocation (keys)");
    if (hipHostGetDevicePointer((void**)&s.h_out_dev, s.h_out, 0) != hipSuccess) s.h_out_dev = nullptr;
    s.cap_keys = keys;
  }
  return K2H_AMD_OK;
}

// Wait for a slot's previous chunk and copy its results out of pinned memory.
int slot_drain(Slot& s, uint64_t* h1, uint64_t* h2) {
  if (!s.busy) return K2H_AMD_OK;
  hipError_t e = hipEventSynchronize(s.done);
  s.busy = false;
  if (e != hipSuccess) return fail(K2H_AMD_EHIP, "chunk completion", e);
  pool().copy(h1 + s.first, s.h_out, s.count * 8);
  if (s.want_h2 && h2) pool().copy(h2 + s.first, s.h_out + s.count, s.count * 8);
  return K2H_AMD_OK;
}

// Forget a slot's pending chunk without copying it anywhere: waits for the device work that
// still writes into the slot's buffers.  Every host call starts by discarding both slots,
// and every error return discards them too, so a chunk left behind by a failed call can
// never be drained into a later caller's output.
void slot_discard(Slot& s) {
  if (s.busy && s.done) (void)hipEventSynchronize(s.done);
  s.busy = false;
}

struct SlotsGuard {  // discards both slots on entry and on every return path
  HostCtx& c;
  explicit SlotsGuard(HostCtx& ctx) : c(ctx) {
    slot_discard(c.slot[0]);
    slot_discard(c.slot[1]);
  }
  ~SlotsGuard() {
    slot_discard(c.slot[0]);
    slot_discard(c.slot[1]);
  }
};

constexpr uint64_t kChunkBytes = 64ull << 20;  // 64 MiB of key bytes per pipeline chunk
constexpr uint64_t kChunkKeysMax = 4ull << 20;

// Makes `device` current for the duration of a host-pointer call and restores the caller's
// current device on every return path (a torch process must not see its current
// device change under it).
class DeviceGuard {
 public:
  int enter(int device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) return fail(K2H_AMD_ENODEV, "no HIP device", e);
    if (device < 0 || device >= count || device >= 64) return fail(K2H_AMD_EINVAL, "device index out of range");
    if (int rc = gate_device(device)) return rc;
    if ((e = hipGetDevice(&prev_)) != hipSuccess) return fail(K2H_AMD_EHIP, "hipGetDevice", e);
    if (prev_ != device && (e = hipSetDevice(device)) != hipSuccess) return fail(K2H_AMD_EHIP, "hipSetDevice", e);
    set_ = prev_ != device;
    return K2H_AMD_OK;
  }
  ~DeviceGuard() {
    if (set_) (void)hipSetDevice(prev_);
  }

 private:
  int prev_ = -1;
  bool set_ = false;
};

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int k2h_amd_hash_fixed(const void* keys, uint64_t key_len, uint64_t n,
                                                              uint64_t* h1, uint64_t* h2, uint32_t flags,
                                                              void* stream) {
  if (n == 0) return K2H_AMD_OK;
  if (!h1) return fail(K2H_AMD_EINVAL, "h1 is NULL");
  if (key_len && n > UINT64_MAX / key_len) return fail(K2H_AMD_EINVAL, "n * key_len overflows");
  K2H_GATE();
  hipError_t e = k2h::launch_fixed(keys, key_len, n, seed_for(flags), h1, h2, (hipStream_t)stream);
  if (e != hipSuccess) return fail(K2H_AMD_EHIP, "launch_fixed", e);
  return K2H_AMD_OK;
}

__attribute__((visibility("default"))) int k2h_amd_hash_csr(const void* bytes, const uint64_t* offsets, uint64_t n,
                                                            uint64_t* h1, uint64_t* h2, uint32_t flags,
                                                            void* stream) {
  if (n == 0) return K2H_AMD_OK;
  if (!h1 || !offsets) return fail(K2H_AMD_EINVAL, "h1/offsets is NULL");
  K2H_GATE();
  hipError_t e = k2h::launch_csr(bytes, offsets, n, seed_for(flags), h1, h2, (hipStream_t)stream);
  if (e != hipSuccess) return fail(K2H_AMD_EHIP, "launch_csr", e);
  return K2H_AMD_OK;
}

}  // extern "C"

namespace {
int bucket_params(uint64_t cur_mask, uint64_t collision_mask, uint64_t* kindex, uint64_t* ckindex,
                  k2h::BucketParams& bp) {
  int bits = 0;
  for (uint64_t m = cur_mask; m; m >>= 1) ++bits;  // GetMaskBitCount, lib/k2hshm.cc:85-90
  if (kindex && bits > k2h::kKindexPosShift)
    return fail(K2H_AMD_EINVAL, "cur_mask wider than 58 bits cannot be packed into kindex");
  int cbits = 0;
  for (uint64_t m = collision_mask; m; m >>= 1) ++cbits;
  bp.cur_mask = cur_mask;
  bp.collision_mask = collision_mask;
  bp.cshift = (uint32_t)cbits;
  bp.kindex = kindex;
  bp.ckindex = ckindex;
  return K2H_AMD_OK;
}
}  // namespace

extern "C" {

__attribute__((visibility("default"))) int k2h_amd_bucket_index(const uint64_t* h1, uint64_t n, uint64_t cur_mask,
                                                                uint64_t collision_mask, uint64_t* kindex,
                                                                uint64_t* ckindex, void* stream) {
  if (n == 0 || (!kindex && !ckindex)) return K2H_AMD_OK;
  if (!h1) return fail(K2H_AMD_EINVAL, "h1 is NULL");
  k2h::BucketParams bp;
  int rc = bucket_params(cur_mask, collision_mask, kindex, ckindex, bp);
  if (rc) return rc;
  K2H_GATE();
  hipError_t e = k2h::launch_bucket_index(h1, n, bp, (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_bucket_index", e);
}

__attribute__((visibility("default"))) int k2h_amd_hash_fixed_index(const void* keys, uint64_t key_len, uint64_t n,
                                                                    uint64_t* h1, uint64_t* h2, uint32_t flags,
                                                                    uint64_t cur_mask, uint64_t collision_mask,
                                                                    uint64_t* kindex, uint64_t* ckindex,
                                                                    void* stream) {
  if (n == 0) return K2H_AMD_OK;
  if (!h1) return fail(K2H_AMD_EINVAL, "h1 is NULL");
  if (key_len && n > UINT64_MAX / key_len) return fail(K2H_AMD_EINVAL, "n * key_len overflows");
  k2h::BucketParams bp;
  int rc = bucket_params(cur_mask, collision_mask, kindex, ckindex, bp);
  if (rc) return rc;
  K2H_GATE();
  hipError_t e =
      k2h::launch_fixed(keys, key_len, n, seed_for(flags), h1, h2, (hipStream_t)stream, &bp);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_fixed (index)", e);
}

__attribute__((visibility("default"))) int k2h_amd_hash_csr_index(const void* bytes, const uint64_t* offsets,
                                                                  uint64_t n, uint64_t* h1, uint64_t* h2,
                                                                  uint32_t flags, uint64_t cur_mask,
                                                                  uint64_t collision_mask, uint64_t* kindex,
                                                                  uint64_t* ckindex, void* stream) {
  if (n == 0) return K2H_AMD_OK;
  if (!h1 || !offsets) return fail(K2H_AMD_EINVAL, "h1/offsets is NULL");
  k2h::BucketParams bp;
  int rc = bucket_params(cur_mask, collision_mask, kindex, ckindex, bp);
  if (rc) return rc;
  K2H_GATE();
  hipError_t e = k2h::launch_csr(bytes, offsets, n, seed_for(flags), h1, h2, (hipStream_t)stream, &bp);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_csr (index)", e);
}

// Table forms with a NULL bitmap (every entry assigned) run the stateless epilogue; what
// that epilogue cannot express is filled here: found = 1 (0 when cur_mask is 0), and for
// cur_mask 0 kindex = K2H_AMD_KINDEX_NONE -- GetKIndex returns NULL then
// (lib/k2hshm.cc:882-907), the same as the bitmap form -- so the epilogue
// does not write kindex in that case.
static int null_bitmap_fill(const k2h_amd_table* table, uint64_t n, uint64_t* kindex, uint8_t* found,
                            k2h::BucketParams& bp, void* stream) {
  if (table->assigned) return K2H_AMD_OK;
  if (found) {
    hipError_t e = hipMemsetAsync(found, table->cur_mask ? 1 : 0, n, (hipStream_t)stream);
    if (e != hipSuccess) return fail(K2H_AMD_EHIP, "found fill", e);
  }
  if (kindex && table->cur_mask == 0) {
    hipError_t e = hipMemsetAsync(kindex, 0xFF, n * sizeof(uint64_t), (hipStream_t)stream);
    if (e != hipSuccess) return fail(K2H_AMD_EHIP, "kindex fill", e);
    bp.kindex = nullptr;
  }
  return K2H_AMD_OK;
}

__attribute__((visibility("default"))) int k2h_amd_bucket_index_table(const uint64_t* h1, uint64_t n,
                                                                      const k2h_amd_table* table, uint64_t* kindex,
                                                                      uint64_t* ckindex, uint8_t* found, void* stream) {
  if (!table) return fail(K2H_AMD_EINVAL, "table is NULL");
  if (n == 0 || (!kindex && !ckindex && !found)) return K2H_AMD_OK;
  if (!h1) return fail(K2H_AMD_EINVAL, "h1 is NULL");
  k2h::BucketParams bp;
  int rc = bucket_params(table->cur_mask, table->collision_mask, kindex, ckindex, bp);
  if (rc) return rc;
  bp.assigned = table->assigned;
  bp.found = table->assigned ? found : nullptr;
  K2H_GATE();
  if ((rc = null_bitmap_fill(table, n, kindex, found, bp, stream))) return rc;
  hipError_t e = k2h::launch_bucket_index(h1, n, bp, (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_bucket_index (table)", e);
}

__attribute__((visibility("default"))) int k2h_amd_hash_fixed_index_table(
    const void* keys, uint64_t key_len, uint64_t n, uint64_t* h1, uint64_t* h2, uint32_t flags,
    const k2h_amd_table* table, uint64_t* kindex, uint64_t* ckindex, uint8_t* found, void* stream) {
  if (!table) return fail(K2H_AMD_EINVAL, "table is NULL");
  if (n == 0) return K2H_AMD_OK;
  if (!h1) return fail(K2H_AMD_EINVAL, "h1 is NULL");
  if (key_len && n > UINT64_MAX / key_len) return fail(K2H_AMD_EINVAL, "n * key_len overflows");
  k2h::BucketParams bp;
  int rc = bucket_params(table->cur_mask, table->collision_mask, kindex, ckindex, bp);
  if (rc) return rc;
  bp.assigned = table->assigned;
  bp.found = table->assigned ? found : nullptr;
  K2H_GATE();
  if ((rc = null_bitmap_fill(table, n, kindex, found, bp, stream))) return rc;
  hipError_t e = k2h::launch_fixed(keys, key_len, n, seed_for(flags), h1, h2, (hipStream_t)stream, &bp);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_fixed (table index)", e);
}

__attribute__((visibility("default"))) int k2h_amd_hash_csr_index_table(
    const void* bytes, const uint64_t* offsets, uint64_t n, uint64_t* h1, uint64_t* h2, uint32_t flags,
    const k2h_amd_table* table, uint64_t* kindex, uint64_t* ckindex, uint8_t* found, void* stream) {
  if (!table) return fail(K2H_AMD_EINVAL, "table is NULL");
  if (n == 0) return K2H_AMD_OK;
  if (!h1 || !offsets) return fail(K2H_AMD_EINVAL, "h1/offsets is NULL");
  k2h::BucketParams bp;
  int rc = bucket_params(table->cur_mask, table->collision_mask, kindex, ckindex, bp);
  if (rc) return rc;
  bp.assigned = table->assigned;
  bp.found = table->assigned ? found : nullptr;
  K2H_GATE();
  if ((rc = null_bitmap_fill(table, n, kindex, found, bp, stream))) return rc;
  hipError_t e = k2h::launch_csr(bytes, offsets, n, seed_for(flags), h1, h2, (hipStream_t)stream, &bp);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_csr (table index)", e);
}

__attribute__((visibility("default"))) int k2h_amd_hash_fixed_host(const void* keys, uint64_t key_len, uint64_t n,
                                                                   uint64_t* h1, uint64_t* h2, uint32_t flags,
                                                                   int device) {
  if (n == 0) return K2H_AMD_OK;
  if (!h1) return fail(K2H_AMD_EINVAL, "h1 is NULL");
  if (key_len && n > UINT64_MAX / key_len) return fail(K2H_AMD_EINVAL, "n * key_len overflows");
  if (!keys || key_len == 0) {
    memset(h1, 0, n * 8);
    if (h2) memset(h2, 0, n * 8);
    return K2H_AMD_OK;
  }
  DeviceGuard dg;
  int rc = dg.enter(device);
  if (rc) return rc;
  HostCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lk(c.mu);
  SlotsGuard sg(c);
  uint64_t per = kChunkBytes / key_len;
  if (per == 0) per = 1;
  if (per > kChunkKeysMax) per = kChunkKeysMax;
  const uint8_t* src = (const uint8_t*)keys;
  int k = 0;
  for (uint64_t first = 0; first < n; first += per, k ^= 1) {
    uint64_t cnt = n - first < per ? n - first : per;
    Slot& s = c.slot[k];
    if ((rc = slot_drain(s, h1, h2))) return rc;
    if ((rc = slot_reserve(s, per * key_len, per))) return rc;
    pool().copy(s.h_in, src + first * key_len, cnt * key_len);
    hipError_t e = hipMemcpyAsync(s.d_in, s.h_in, cnt * key_len, hipMemcpyHostToDevice, s.stream);
    uint64_t* out = s.h_out_dev ? s.h_out_dev : s.d_out;  // kernel stores over PCIe when mapped
    if (e == hipSuccess)
      e = k2h::launch_fixed(s.d_in, key_len, cnt, seed_for(flags), out, h2 ? out + cnt : nullptr, s.stream);
    if (e == hipSuccess && !s.h_out_dev)
      e = hipMemcpyAsync(s.h_out, s.d_out, cnt * (h2 ? 16 : 8), hipMemcpyDeviceToHost, s.stream);
    if (e == hipSuccess) e = hipEventRecord(s.done, s.stream);
    if (e != hipSuccess) return fail(K2H_AMD_EHIP, "fixed host chunk", e);
    s.busy = true;
    s.first = first;
    s.count = cnt;
    s.want_h2 = h2 != nullptr;
  }
  for (int j = 0; j < 2; ++j)
    if ((rc = slot_drain(c.slot[j], h1, h2))) return rc;
  return K2H_AMD_OK;
}

__attribute__((visibility("default"))) int k2h_amd_hash_csr_host(const void* bytes, const uint64_t* offsets,
                                                                 uint64_t n, uint64_t* h1, uint64_t* h2,
                                                                 uint32_t flags, int device) {
  if (n == 0) return K2H_AMD_OK;
  if (!h1 || !offsets) return fail(K2H_AMD_EINVAL, "h1/offsets is NULL");
  if (!bytes) {
    memset(h1, 0, n * 8);
    if (h2) memset(h2, 0, n * 8);
    return K2H_AMD_OK;
  }
  DeviceGuard dg;
  int rc = dg.enter(device);
  if (rc) return rc;
  HostCtx& c = g_ctx[device];
  std::lock_guard<std::mutex> lk(c.mu);
  SlotsGuard sg(c);
  const uint8_t* src = (const uint8_t*)bytes;
  int k = 0;
  uint64_t first = 0;
  while (first < n) {
    // the longest run of keys from `first` within the byte budget and the key cap (>= 1
    // key), found by a linear walk that checks every offset pair on the way: a decrease
    // ends the call with EINVAL before any of this chunk's work is queued (the GPU still
    // works on the previous chunk meanwhile), and no search runs over unchecked offsets
    // (ADVICE r2).  Byte counts are differences of checked, non-decreasing offsets, so
    // nothing wraps.
    const uint64_t cap = n - first < kChunkKeysMax ? n : first + kChunkKeysMax;
    if (offsets[first + 1] < offsets[first]) return fail(K2H_AMD_EINVAL, "offsets not non-decreasing");
    uint64_t last = first + 1;
    while (last < cap) {
      const uint64_t a = offsets[last], b = offsets[last + 1];
      if (b < a) return fail(K2H_AMD_EINVAL, "offsets not non-decreasing");
      if (b - offsets[first] > kChunkBytes) break;
      ++last;
    }
    uint64_t cnt = last - first;
    uint64_t nb = offsets[last] - offsets[first];
    Slot& s = c.slot[k];
    if ((rc = slot_drain(s, h1, h2))) return rc;
    if ((rc = slot_reserve(s, nb > kChunkBytes ? nb : kChunkBytes, kChunkKeysMax))) return rc;
    // the kernel takes the caller's offsets as they are, relative to a byte base placed
    // offsets[first] bytes before the chunk (no rebasing pass on the CPU)
    pool().copy(s.h_in, src + offsets[first], nb);
    pool().copy(s.h_off, offsets + first, (cnt + 1) * 8);
    hipError_t e = nb ? hipMemcpyAsync(s.d_in, s.h_in, nb, hipMemcpyHostToDevice, s.stream) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(s.d_off, s.h_off, (cnt + 1) * 8, hipMemcpyHostToDevice, s.stream);
    if (e == hipSuccess)
      e = k2h::launch_csr((const uint8_t*)s.d_in - offsets[first], s.d_off, cnt, seed_for(flags), s.d_out,
                          h2 ? s.d_out + cnt : nullptr, s.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(s.h_out, s.d_out, cnt * (h2 ? 16 : 8), hipMemcpyDeviceToHost, s.stream);
    if (e == hipSuccess) e = hipEventRecord(s.done, s.stream);
    if (e != hipSuccess) return fail(K2H_AMD_EHIP, "csr host chunk", e);
    s.busy = true;
    s.first = first;
    s.count = cnt;
    s.want_h2 = h2 != nullptr;
    first = last;
    k ^= 1;
  }
  for (int j = 0; j < 2; ++j)
    if ((rc = slot_drain(c.slot[j], h1, h2))) return rc;
  return K2H_AMD_OK;
}

__attribute__((visibility("default"))) int k2h_amd_hash_ranges(const void* base, const uint64_t* starts,
                                                               const uint64_t* lens, uint64_t n, uint64_t* h1,
                                                               uint64_t* h2, uint32_t flags, void* stream) {
  if (n == 0) return K2H_AMD_OK;
  if (!h1 || !starts || !lens || !base) return fail(K2H_AMD_EINVAL, "NULL base/starts/lens/h1");
  K2H_GATE();
  hipError_t e = k2h::launch_ranges(base, starts, lens, n, seed_for(flags), (flags & K2H_AMD_FLAG_CSTR) != 0, h1, h2,
                                    (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_ranges", e);
}

// k2himport inputs in device memory (include/k2hash_amd.h section 5)
__attribute__((visibility("default"))) int k2h_amd_import_scan_device(const void* file, uint64_t size, int format,
                                                                      k2h_amd_import_rec* recs, uint64_t cap,
                                                                      uint64_t* count, void* stream) {
  if (!count || (size && !file) || (format != K2H_AMD_IMPORT_TSV && format != K2H_AMD_IMPORT_MDBM))
    return fail(K2H_AMD_EINVAL, "import_scan_device: NULL count/file or bad format");
  if (size) K2H_GATE();  // an empty file has no records and needs no device
  hipError_t e = hipSuccess;
  int rc = k2h::launch_import_scan(file, size, format, recs, cap, count, (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EHIP) return fail(rc, "launch_import_scan", e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "import_scan_device: not a mdbm file, or more records than cap");
}

__attribute__((visibility("default"))) int k2h_amd_import_scan_prehash_device(
    const void* file, uint64_t size, int format, k2h_amd_import_rec* recs, uint64_t cap, uint64_t* count, uint64_t* h1,
    uint64_t* h2, uint32_t flags, void* stream) {
  if (!count || (size && !file) || (format != K2H_AMD_IMPORT_TSV && format != K2H_AMD_IMPORT_MDBM))
    return fail(K2H_AMD_EINVAL, "import_scan_prehash_device: NULL count/file or bad format");
  if (recs && cap && !h1) return fail(K2H_AMD_EINVAL, "import_scan_prehash_device: NULL h1");
  if (size) K2H_GATE();  // an empty file has no records and needs no device
  hipError_t e = hipSuccess;
  int rc = k2h::launch_import_scan(file, size, format, recs, cap, count, (hipStream_t)stream, &e, h1, h2,
                                   seed_for(flags));
  if (rc == K2H_AMD_EHIP) return fail(rc, "launch_import_scan", e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "import_scan_prehash_device: not a mdbm file, or more records than cap");
}

__attribute__((visibility("default"))) int k2h_amd_import_prehash(const void* file, uint64_t size,
                                                                  const k2h_amd_import_rec* recs, uint64_t n, uint64_t* h1, uint64_t* h2,
                                                                  uint32_t flags, void* stream) {
  if (n == 0) return K2H_AMD_OK;
  if (!file || !recs || !h1) return fail(K2H_AMD_EINVAL, "import_prehash: NULL file/recs/h1");
  K2H_GATE();
  hipError_t e = k2h::launch_import_prehash(file, size, recs, n, seed_for(flags), h1, h2, (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_import_prehash", e);
}

// k2hash archives in device memory (include/k2hash_amd.h section 5)
__attribute__((visibility("default"))) int k2h_amd_archive_scan_device(const void* file, uint64_t size,
                                                                       k2h_amd_archive_rec* recs, uint64_t cap,
                                                                       uint64_t* count, void* stream) {
  if (!count || (size && !file)) return fail(K2H_AMD_EINVAL, "archive_scan_device: NULL count/file");
  if (size >= 104) K2H_GATE();  // a file without a whole header has no records and needs no device
  hipError_t e = hipSuccess;
  int rc = k2h::launch_archive_scan(file, size, recs, cap, count, (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EHIP || rc == K2H_AMD_ENOMEM) return fail(rc, "launch_archive_scan", e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "archive_scan_device: more records than cap, or too many candidates");
}

__attribute__((visibility("default"))) int k2h_amd_archive_prehash(const void* file, uint64_t size,
                                                                   const k2h_amd_archive_rec* recs, uint64_t n,
                                                                   uint64_t* h1, uint64_t* h2, uint64_t* new_h1,
                                                                   uint64_t* new_h2, uint32_t flags, void* stream) {
  if (flags & K2H_AMD_FLAG_CSTR) return fail(K2H_AMD_EINVAL, "archive_prehash: archive keys are hashed as stored");
  if (n == 0) return K2H_AMD_OK;
  if (!recs || !h1 || (size && !file)) return fail(K2H_AMD_EINVAL, "archive_prehash: NULL file/recs/h1");
  K2H_GATE();
  k2h::ArchiveHashOut out;
  out.h1 = h1, out.h2 = h2, out.new_h1 = new_h1, out.new_h2 = new_h2;
  hipError_t e = k2h::launch_archive_prehash(file, size, recs, n, seed_for(flags), out, (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_archive_prehash", e);
}

__attribute__((visibility("default"))) int k2h_amd_archive_scan_prehash_device(
    const void* file, uint64_t size, k2h_amd_archive_rec* recs, uint64_t cap, uint64_t* count, uint64_t* h1,
    uint64_t* h2, uint64_t* new_h1, uint64_t* new_h2, uint32_t flags, void* stream) {
  if (flags & K2H_AMD_FLAG_CSTR)
    return fail(K2H_AMD_EINVAL, "archive_scan_prehash_device: archive keys are hashed as stored");
  if (!count || (size && !file)) return fail(K2H_AMD_EINVAL, "archive_scan_prehash_device: NULL count/file");
  if (recs && cap && !h1) return fail(K2H_AMD_EINVAL, "archive_scan_prehash_device: NULL h1");
  if (size >= 104) K2H_GATE();
  k2h::ArchiveHashOut out;
  out.h1 = h1, out.h2 = h2, out.new_h1 = new_h1, out.new_h2 = new_h2;
  hipError_t e = hipSuccess;
  int rc = k2h::launch_archive_scan(file, size, recs, cap, count, (hipStream_t)stream, &e,
                                    (recs && cap) ? &out : nullptr, seed_for(flags));
  if (rc == K2H_AMD_EHIP || rc == K2H_AMD_ENOMEM) return fail(rc, "launch_archive_scan", e);
  return rc == K2H_AMD_OK ? rc
                          : fail(rc, "archive_scan_prehash_device: more records than cap, or too many candidates");
}

// Section 5b: a transaction archive folded by Load's rule.  Judged on the host before any
// device is touched.
__attribute__((visibility("default"))) int k2h_amd_archive_fold(const void* file, uint64_t size,
                                                                const k2h_amd_archive_rec* recs, uint64_t n,
                                                                const uint64_t* h1, uint8_t* keep, uint64_t* by,
                                                                uint64_t* dropped, void* stream) {
  if (dropped) *dropped = 0;
  if (n == 0) return K2H_AMD_OK;
  if (!keep) return fail(K2H_AMD_EINVAL, "archive_fold: NULL keep");
  if (!file) return fail(K2H_AMD_EINVAL, "archive_fold: NULL file");
  if (!recs) return fail(K2H_AMD_EINVAL, "archive_fold: NULL recs");
  if (n > 0xFFFFFFFEull)
    return fail(K2H_AMD_EINVAL, "archive_fold: more than 2^32 - 2 records (indices are sorted as 32-bit values)");
  K2H_GATE();
  hipError_t e = hipSuccess;
  int rc = k2h::launch_archive_fold(file, size, recs, n, h1, seed_for(0), keep, by, dropped, (hipStream_t)stream, &e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_archive_fold", e);
}

// Section 5c: a log applied to a held blob stream.  Judged on the host like the one above.
__attribute__((visibility("default"))) int k2h_amd_archive_apply(
    const void* held, uint64_t held_size, const uint64_t* held_off, uint64_t na, const uint8_t* held_keep,
    const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n, const uint8_t* consider,
    const uint64_t* h1, const uint64_t* h2, uint32_t flags, void* out, uint64_t out_cap, uint64_t* out_off,
    uint64_t* origin, uint8_t* touched, uint64_t* counts, uint64_t* stop, void* stream) {
  if (!counts) return fail(K2H_AMD_EINVAL, "archive_apply: NULL counts");
  if (!stop) return fail(K2H_AMD_EINVAL, "archive_apply: NULL stop");
  for (int k = 0; k < 7; ++k) counts[k] = 0;
  *stop = n;
  if (na && !held) return fail(K2H_AMD_EINVAL, "archive_apply: NULL held");
  if (na && !held_off) return fail(K2H_AMD_EINVAL, "archive_apply: NULL held_off");
  if (n && !file) return fail(K2H_AMD_EINVAL, "archive_apply: NULL file");
  if (n && !recs) return fail(K2H_AMD_EINVAL, "archive_apply: NULL recs");
  if (out && !out_off) return fail(K2H_AMD_EINVAL, "archive_apply: out given without out_off");
  if (!h1 != !h2) return fail(K2H_AMD_EINVAL, "archive_apply: h1 and h2 are given together or not at all");
  if (flags & ~K2H_AMD_FLAG_STD_FNV) return fail(K2H_AMD_EINVAL, "archive_apply: unknown flags");
  if (flags && h1) return fail(K2H_AMD_EINVAL, "archive_apply: flags choose the hash only when h1 and h2 are NULL");
  if (na > 0xFFFFFFFEull || n > 0xFFFFFFFEull - na)
    return fail(K2H_AMD_EINVAL, "archive_apply: more than 2^32 - 2 blobs and records (indices are sorted as 32-bit values)");
  if (na + n == 0 && !out_off) return K2H_AMD_OK;
  K2H_GATE();
  hipError_t e = hipSuccess;
  if (na + n == 0) return clear_word(out_off, stream, "archive_apply: hipMemsetAsync");  // nothing held, no log
  int rc = k2h::launch_archive_apply(held, held_size, held_off, na, held_keep, file, size, recs, n, consider, h1, h2,
                                     seed_for(flags), out, out_cap, out_off, origin, touched, counts, stop,
                                     (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EINVAL) return exceeds_cap("archive_apply", "emitted blobs", counts[1], out_cap);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_archive_apply", e);
}

// Section 5d: the barrier record at b executed on the held arena.  Judged on the host like the two above.
__attribute__((visibility("default"))) int k2h_amd_archive_barrier(
    void* held, uint64_t held_size, uint64_t held_cap, uint64_t* held_off, uint64_t na, uint8_t* held_keep,
    const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n, uint64_t b, const uint8_t* consider,
    const uint64_t* h1, const uint64_t* h2, const uint64_t* new_h1, const uint64_t* new_h2, uint32_t flags,
    uint64_t* result, void* stream) {
  if (!result) return fail(K2H_AMD_EINVAL, "archive_barrier: NULL result");
  for (int k = 0; k < 8; ++k) result[k] = 0;
  result[0] = K2H_AMD_BARRIER_NOT_A_BARRIER;
  result[5] = ~0ull;
  if (!held_keep) return fail(K2H_AMD_EINVAL, "archive_barrier: NULL held_keep");
  if (na && !held) return fail(K2H_AMD_EINVAL, "archive_barrier: NULL held");
  if (na && !held_off) return fail(K2H_AMD_EINVAL, "archive_barrier: NULL held_off");
  if (!file) return fail(K2H_AMD_EINVAL, "archive_barrier: NULL file");
  if (!recs) return fail(K2H_AMD_EINVAL, "archive_barrier: NULL recs");
  if (b >= n) return fail(K2H_AMD_EINVAL, "archive_barrier: b is not below n");
  if (held_cap < held_size) return fail(K2H_AMD_EINVAL, "archive_barrier: held_cap is below held_size");
  const int given = !!h1 + !!h2 + !!new_h1 + !!new_h2;
  if (given != 0 && given != 4)
    return fail(K2H_AMD_EINVAL, "archive_barrier: h1, h2, new_h1 and new_h2 are given together or not at all");
  if (flags & ~(K2H_AMD_FLAG_STD_FNV | K2H_AMD_BARRIER_COUNT_ONLY)) return fail(K2H_AMD_EINVAL, "archive_barrier: unknown flags");
  if ((flags & K2H_AMD_FLAG_STD_FNV) && given)
    return fail(K2H_AMD_EINVAL, "archive_barrier: K2H_AMD_FLAG_STD_FNV chooses the hash only when the hashes are NULL");
  if (na > 0xFFFFFFFEull)
    return fail(K2H_AMD_EINVAL, "archive_barrier: more than 2^32 - 2 blobs (indices are kept as 32-bit values)");
  const bool count_only = (flags & K2H_AMD_BARRIER_COUNT_ONLY) != 0;
  if (!count_only && (!held || !held_off))
    return fail(K2H_AMD_EINVAL, "archive_barrier: NULL held or held_off without K2H_AMD_BARRIER_COUNT_ONLY");
  K2H_GATE();
  hipError_t e = hipSuccess;
  int rc = k2h::launch_archive_barrier(held, held_size, held_cap, held_off, na, held_keep, file, size, recs, n, b,
                                       consider, h1, h2, new_h1, new_h2, seed_for(flags), count_only, result,
                                       (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EINVAL) return exceeds_cap("archive_barrier", "appended blob", result[2], held_cap - held_size);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_archive_barrier", e);
}

// ---------------------------------------------------------------------------
// RALLEDATA producer (include/k2hash_amd.h section 4)
// ---------------------------------------------------------------------------
__attribute__((visibility("default"))) uint64_t k2h_amd_ralledata_size(uint64_t n, uint64_t key_bytes,
                                                                       uint64_t val_bytes, uint64_t skey_bytes,
                                                                       uint64_t attr_bytes) {
  return 80ull * n + key_bytes + val_bytes + skey_bytes + attr_bytes;
}

__attribute__((visibility("default"))) int k2h_amd_build_ralledata(
    const void* keys, const uint64_t* key_off, const void* vals, const uint64_t* val_off, const void* skeys,
    const uint64_t* skey_off, const void* attrs, const uint64_t* attr_off, uint64_t n, void* out, uint64_t* blob_off,
    uint32_t flags, void* stream) {
  if (!key_off) return fail(K2H_AMD_EINVAL, "key_off is NULL");
  if (n && !out) return fail(K2H_AMD_EINVAL, "out is NULL");
  if ((val_off && !vals) || (skey_off && !skeys) || (attr_off && !attrs))
    return fail(K2H_AMD_EINVAL, "segment offsets without segment bytes");
  K2H_GATE();
  k2h::RalleInputs in;
  in.keys = (const uint8_t*)keys;
  in.koff = key_off;
  in.vals = (const uint8_t*)vals;
  in.voff = val_off;
  in.skeys = (const uint8_t*)skeys;
  in.soff = skey_off;
  in.attrs = (const uint8_t*)attrs;
  in.aoff = attr_off;
  hipError_t e = k2h::launch_ralledata(in, n, seed_for(flags), (uint8_t*)out, blob_off, (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_ralledata", e);
}

// Host form: stage each segment's byte range and offsets on `device`, build there, copy
// the blobs (and offsets) back.  One shot, not pipelined.
__attribute__((visibility("default"))) int k2h_amd_build_ralledata_host(
    const void* keys, const uint64_t* key_off, const void* vals, const uint64_t* val_off, const void* skeys,
    const uint64_t* skey_off, const void* attrs, const uint64_t* attr_off, uint64_t n, void* out, uint64_t* blob_off,
    uint32_t flags, int device) {
  if (!key_off) return fail(K2H_AMD_EINVAL, "key_off is NULL");
  if (n == 0) {
    if (blob_off) blob_off[0] = 0;
    return K2H_AMD_OK;
  }
  if (!out) return fail(K2H_AMD_EINVAL, "out is NULL");
  const void* src[4] = {keys, vals, skeys, attrs};
  const uint64_t* off[4] = {key_off, val_off, skey_off, attr_off};
  uint64_t total = 80ull * n;
  for (int s = 0; s < 4; ++s) {
    if (!off[s]) continue;
    if (!src[s] && off[s][n] != off[s][0]) return fail(K2H_AMD_EINVAL, "segment offsets without segment bytes");
    for (uint64_t i = 0; i < n; ++i)
      if (off[s][i + 1] < off[s][i]) return fail(K2H_AMD_EINVAL, "offsets not non-decreasing");
    total += off[s][n] - off[s][0];
  }
  DeviceGuard dg;
  int rc = dg.enter(device);
  if (rc) return rc;
  hipStream_t st;
  hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  if (e != hipSuccess) return fail(K2H_AMD_EHIP, "hipStreamCreate", e);
  void* dbuf[4] = {nullptr, nullptr, nullptr, nullptr};
  uint64_t* doff[4] = {nullptr, nullptr, nullptr, nullptr};
  uint8_t* dout = nullptr;
  uint64_t* dblob = nullptr;
  k2h::RalleInputs in;
  const uint8_t** bp[4] = {&in.keys, &in.vals, &in.skeys, &in.attrs};
  const uint64_t** op[4] = {&in.koff, &in.voff, &in.soff, &in.aoff};
  for (int s = 0; s < 4 && e == hipSuccess; ++s) {
    if (!off[s]) continue;
    uint64_t lo = off[s][0], len = off[s][n] - lo;
    e = hipMallocAsync((void**)&doff[s], (n + 1) * 8, st);
    if (e == hipSuccess) e = hipMemcpyAsync(doff[s], off[s], (n + 1) * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMallocAsync(&dbuf[s], len ? len : 1, st);
    if (e == hipSuccess && len) e = hipMemcpyAsync(dbuf[s], (const uint8_t*)src[s] + lo, len, hipMemcpyHostToDevice, st);
    *bp[s] = (const uint8_t*)dbuf[s] - lo;  // kernel indexes with the caller's raw offsets
    *op[s] = doff[s];
  }
  if (e == hipSuccess) e = hipMallocAsync((void**)&dout, total, st);
  if (e == hipSuccess && blob_off) e = hipMallocAsync((void**)&dblob, (n + 1) * 8, st);
  if (e == hipSuccess) e = k2h::launch_ralledata(in, n, seed_for(flags), dout, dblob, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, total, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && blob_off) e = hipMemcpyAsync(blob_off, dblob, (n + 1) * 8, hipMemcpyDeviceToHost, st);
  for (int s = 0; s < 4; ++s) {
    if (dbuf[s]) (void)hipFreeAsync(dbuf[s], st);
    if (doff[s]) (void)hipFreeAsync(doff[s], st);
  }
  if (dout) (void)hipFreeAsync(dout, st);
  if (dblob) (void)hipFreeAsync(dblob, st);
  hipError_t f = hipStreamSynchronize(st);
  (void)hipStreamDestroy(st);
  if (e == hipSuccess) e = f;
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "build_ralledata_host", e);
}

// ---------------------------------------------------------------------------
// RALLEDATA consumer side (include/k2hash_amd.h section 4b).  Arguments are judged before
// the device gate, so a bad call fails the same way with or without a GPU.
// ---------------------------------------------------------------------------
__attribute__((visibility("default"))) int k2h_amd_ralledata_check(const void* blobs, uint64_t size,
                                                                   const uint64_t* blob_off, uint64_t n,
                                                                   const k2h_amd_hash_range* range, uint32_t flags,
                                                                   uint8_t* status, uint8_t* route, uint64_t* h1,
                                                                   uint64_t* h2, void* stream) {
  if (flags & K2H_AMD_FLAG_CSTR) return fail(K2H_AMD_EINVAL, "ralledata_check: blob keys are hashed as stored");
  if (n == 0) return K2H_AMD_OK;
  if (!blobs || !blob_off || !status) return fail(K2H_AMD_EINVAL, "ralledata_check: NULL blobs/blob_off/status");
  if ((range != nullptr) != (route != nullptr))
    return fail(K2H_AMD_EINVAL, "ralledata_check: range and route go together");
  k2h::RalleRoute rr;
  if (range) {
    if (range->target_max_hash == 0) return fail(K2H_AMD_EINVAL, "ralledata_check: target_max_hash is 0");
    // lib/k2hshmdirect.cc:118-119; the sums wrap in 64 bits
    const uint64_t add = range->target_hash_range > 0 ? (uint64_t)range->target_hash_range - 1 : 0;
    rr.t = range->target_hash;
    rr.t_max = range->target_max_hash;
    rr.t_end = (range->target_hash + add) % range->target_max_hash;
    rr.old_on = range->old_hash != ~0ull;
    if (rr.old_on) {
      if (range->old_max_hash == 0) return fail(K2H_AMD_EINVAL, "ralledata_check: old_max_hash is 0");
      rr.o = range->old_hash;
      rr.o_max = range->old_max_hash;
      rr.o_end = (range->old_hash + add) % range->old_max_hash;
    }
  }
  K2H_GATE();
  hipError_t e = k2h::launch_ralledata_check(blobs, size, blob_off, n, seed_for(flags), rr, status, route, h1, h2,
                                             (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_ralledata_check", e);
}

__attribute__((visibility("default"))) int k2h_amd_ralledata_select(const void* blobs, uint64_t size,
                                                                    const uint64_t* blob_off, uint64_t n,
                                                                    const uint8_t* keep, void* out, uint64_t out_cap,
                                                                    uint64_t* out_off, uint64_t* index, uint64_t* kept,
                                                                    uint64_t* kept_bytes, void* stream) {
  if (!kept || !kept_bytes) return fail(K2H_AMD_EINVAL, "ralledata_select: NULL kept/kept_bytes");
  *kept = *kept_bytes = 0;
  if (n == 0) return K2H_AMD_OK;
  if (!blobs || !blob_off || !keep || (out && !out_off))
    return fail(K2H_AMD_EINVAL, "ralledata_select: NULL blobs/blob_off/keep/out_off");
  K2H_GATE();
  hipError_t e = hipSuccess;
  int rc = k2h::launch_ralledata_select(blobs, size, blob_off, n, keep, out, out_cap, out_off, index, kept, kept_bytes,
                                        (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EHIP || rc == K2H_AMD_ENOMEM) return fail(rc, "launch_ralledata_select", e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "ralledata_select: the kept blobs exceed out_cap, or too many blobs");
}

// Section 4b': the superseded duplicates of a stream.  Judged on the host like the two above.
__attribute__((visibility("default"))) int k2h_amd_ralledata_dedup(const void* blobs, uint64_t size,
                                                                   const uint64_t* blob_off, uint64_t n,
                                                                   const uint8_t* consider, uint8_t* keep,
                                                                   uint64_t* by, uint64_t* dropped, void* stream) {
  if (dropped) *dropped = 0;
  if (n == 0) return K2H_AMD_OK;
  if (!keep) return fail(K2H_AMD_EINVAL, "ralledata_dedup: NULL keep");
  if (!blobs) return fail(K2H_AMD_EINVAL, "ralledata_dedup: NULL blobs");
  if (!blob_off) return fail(K2H_AMD_EINVAL, "ralledata_dedup: NULL blob_off");
  if (n > 0xFFFFFFFEull)
    return fail(K2H_AMD_EINVAL, "ralledata_dedup: more than 2^32 - 2 blobs (indices are sorted as 32-bit values)");
  K2H_GATE();
  hipError_t e = hipSuccess;
  int rc = k2h::launch_ralledata_dedup(blobs, size, blob_off, n, consider, keep, by, dropped, (hipStream_t)stream, &e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_ralledata_dedup", e);
}

// Section 4b'''': the times in the blobs' attrs.  Judged on the host like the ones above.
__attribute__((visibility("default"))) int k2h_amd_ralledata_times(
    const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n, const uint8_t* consider,
    const k2h_amd_time_window* window, const uint8_t* route, uint8_t* tflags, int64_t* mtime, int64_t* expire,
    uint8_t* keep, void* stream) {
  if (!tflags && !mtime && !expire && !keep)
    return fail(K2H_AMD_EINVAL, "ralledata_times: tflags, mtime, expire and keep are all NULL");
  if (route && !window) return fail(K2H_AMD_EINVAL, "ralledata_times: route given without window");
  if (window && (window->flags & ~(K2H_AMD_WIN_START | K2H_AMD_WIN_END | K2H_AMD_WIN_EXPIRE)))
    return fail(K2H_AMD_EINVAL, "ralledata_times: unknown window flag bits");
  if (n == 0) return K2H_AMD_OK;
  if (!blobs) return fail(K2H_AMD_EINVAL, "ralledata_times: NULL blobs");
  if (!blob_off) return fail(K2H_AMD_EINVAL, "ralledata_times: NULL blob_off");
  K2H_GATE();
  hipError_t e = k2h::launch_ralledata_times(blobs, size, blob_off, n, consider, window, route, tflags, mtime, expire,
                                             keep, (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_ralledata_times", e);
}

// And the dedup under the mtime rule.
__attribute__((visibility("default"))) int k2h_amd_ralledata_dedup_mtime(
    const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n, const uint8_t* consider, uint8_t* keep,
    uint64_t* by, uint64_t* dropped, const k2h_amd_timespec* pts, void* stream) {
  if (dropped) *dropped = 0;
  if (n == 0) return K2H_AMD_OK;
  if (!keep) return fail(K2H_AMD_EINVAL, "ralledata_dedup_mtime: NULL keep");
  if (!blobs) return fail(K2H_AMD_EINVAL, "ralledata_dedup_mtime: NULL blobs");
  if (!blob_off) return fail(K2H_AMD_EINVAL, "ralledata_dedup_mtime: NULL blob_off");
  if (!pts) return fail(K2H_AMD_EINVAL, "ralledata_dedup_mtime: NULL pts");
  if (n > 0xFFFFFFFEull)
    return fail(K2H_AMD_EINVAL,
                "ralledata_dedup_mtime: more than 2^32 - 2 blobs (indices are sorted as 32-bit values)");
  K2H_GATE();
  hipError_t e = hipSuccess;
  int rc = k2h::launch_ralledata_dedup_mtime(blobs, size, blob_off, n, consider, pts, keep, by, dropped,
                                             (hipStream_t)stream, &e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_ralledata_dedup_mtime", e);
}

// Section 4b''''': two streams joined by identity.  Judged on the host like the ones above.
__attribute__((visibility("default"))) int k2h_amd_ralledata_diff(
    const void* a_blobs, uint64_t a_size, const uint64_t* a_off, uint64_t na, const uint8_t* a_consider,
    const void* b_blobs, uint64_t b_size, const uint64_t* b_off, uint64_t nb, const uint8_t* b_consider,
    const k2h_amd_diff_times* times, uint8_t* rel, uint64_t* match, uint8_t* seen, uint64_t* counts, void* stream) {
  if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
  if (na && !rel) return fail(K2H_AMD_EINVAL, "ralledata_diff: NULL rel");
  if (na && !a_blobs) return fail(K2H_AMD_EINVAL, "ralledata_diff: NULL a_blobs");
  if (na && !a_off) return fail(K2H_AMD_EINVAL, "ralledata_diff: NULL a_off");
  if (nb && !b_blobs) return fail(K2H_AMD_EINVAL, "ralledata_diff: NULL b_blobs");
  if (nb && !b_off) return fail(K2H_AMD_EINVAL, "ralledata_diff: NULL b_off");
  if (na > 0xFFFFFFFEull || nb > 0xFFFFFFFEull || na + nb > 0xFFFFFFFEull)
    return fail(K2H_AMD_EINVAL,
                "ralledata_diff: more than 2^32 - 2 blobs in the two streams (indices are sorted as 32-bit values)");
  if (na == 0 && !(seen && nb)) return K2H_AMD_OK;
  K2H_GATE();
  hipError_t e = hipSuccess;
  if (na == 0) {  // nothing arrives: no held blob is mentioned
    e = hipMemsetAsync(seen, 0, nb, (hipStream_t)stream);
    return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "ralledata_diff: hipMemsetAsync", e);
  }
  int rc = k2h::launch_ralledata_diff(a_blobs, a_size, a_off, na, a_consider, b_blobs, b_size, b_off, nb, b_consider,
                                      times, rel, match, seen, counts, (hipStream_t)stream, &e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_ralledata_diff", e);
}

// Section 4b'''''': subkeys as edges, and the subtree closure.  Judged on the host like the ones above.
__attribute__((visibility("default"))) int k2h_amd_ralledata_subkeys(
    const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n, const uint8_t* consider, uint32_t flags,
    uint8_t* sk_flags, uint64_t* edge_off, uint64_t* rep, uint64_t* child, uint64_t cap, uint64_t* counts,
    void* stream) {
  if (!counts) return fail(K2H_AMD_EINVAL, "ralledata_subkeys: NULL counts");
  for (int k = 0; k < 5; ++k) counts[k] = 0;
  if (flags & K2H_AMD_FLAG_CSTR)
    return fail(K2H_AMD_EINVAL, "ralledata_subkeys: subkey names are hashed as stored");
  if (flags & ~(uint32_t)K2H_AMD_FLAG_STD_FNV) return fail(K2H_AMD_EINVAL, "ralledata_subkeys: unknown flag bits");
  if (n && !sk_flags) return fail(K2H_AMD_EINVAL, "ralledata_subkeys: NULL sk_flags");
  if (n && !edge_off) return fail(K2H_AMD_EINVAL, "ralledata_subkeys: NULL edge_off");
  if (n && !blobs) return fail(K2H_AMD_EINVAL, "ralledata_subkeys: NULL blobs");
  if (n && !blob_off) return fail(K2H_AMD_EINVAL, "ralledata_subkeys: NULL blob_off");
  if (n > 0xFFFFFFFEull)
    return fail(K2H_AMD_EINVAL,
                "ralledata_subkeys: more than 2^32 - 2 blobs and edges (indices are sorted as 32-bit values)");
  if (n == 0 && !edge_off) return K2H_AMD_OK;
  K2H_GATE();
  hipError_t e = hipSuccess;
  if (n == 0) return clear_word(edge_off, stream, "ralledata_subkeys: hipMemsetAsync");  // no blob, no edge
  int why = 0;
  int rc = k2h::launch_ralledata_subkeys(blobs, size, blob_off, n, consider, seed_for(flags), sk_flags, edge_off, rep,
                                         child, cap, counts, &why, (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EINVAL) {
    char msg[160];
    if (why == 1)
      snprintf(msg, sizeof msg, "ralledata_subkeys: cap %llu is less than the E = %llu edges of the stream",
               (unsigned long long)cap, (unsigned long long)counts[3]);
    else
      snprintf(msg, sizeof msg,
               "ralledata_subkeys: more than 2^32 - 2 blobs and edges (n + E with E = %llu; indices are sorted as "
               "32-bit values)",
               (unsigned long long)counts[3]);
    return fail(rc, msg);
  }
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_ralledata_subkeys", e);
}

__attribute__((visibility("default"))) int k2h_amd_ralledata_reach(const uint64_t* edge_off, const uint64_t* child,
                                                                   const uint64_t* rep, uint64_t n,
                                                                   const uint8_t* roots, uint64_t max_levels,
                                                                   uint8_t* reach, uint64_t* counts, void* stream) {
  if (!counts) return fail(K2H_AMD_EINVAL, "ralledata_reach: NULL counts");
  counts[0] = counts[1] = 0;
  counts[2] = 1;  // nothing to traverse: converged
  if (n == 0) return K2H_AMD_OK;
  if (!reach) return fail(K2H_AMD_EINVAL, "ralledata_reach: NULL reach");
  if (!edge_off) return fail(K2H_AMD_EINVAL, "ralledata_reach: NULL edge_off");
  if (!child) return fail(K2H_AMD_EINVAL, "ralledata_reach: NULL child");
  if (!rep) return fail(K2H_AMD_EINVAL, "ralledata_reach: NULL rep");
  if (!roots) return fail(K2H_AMD_EINVAL, "ralledata_reach: NULL roots");
  if (n > 0xFFFFFFFEull)
    return fail(K2H_AMD_EINVAL, "ralledata_reach: more than 2^32 - 2 blobs (a frontier holds 32-bit indices)");
  K2H_GATE();
  hipError_t e = hipSuccess;
  int rc = k2h::launch_ralledata_reach(edge_off, child, rep, n, roots, max_levels, reach, counts, (hipStream_t)stream,
                                       &e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_ralledata_reach", e);
}

// Section 4b''''''': subkey names unlinked from a stream.  Judged on the host like the ones above.
__attribute__((visibility("default"))) int k2h_amd_ralledata_unlink(
    const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n, const uint8_t* keep,
    const uint8_t* sk_flags, const uint64_t* edge_off, const uint8_t* drop, void* out, uint64_t out_cap,
    uint64_t* out_off, uint64_t* index, uint8_t* changed, uint64_t* counts, void* stream) {
  if (!counts) return fail(K2H_AMD_EINVAL, "ralledata_unlink: NULL counts");
  for (int k = 0; k < 7; ++k) counts[k] = 0;
  if (n && !blobs) return fail(K2H_AMD_EINVAL, "ralledata_unlink: NULL blobs");
  if (n && !blob_off) return fail(K2H_AMD_EINVAL, "ralledata_unlink: NULL blob_off");
  if (n && !sk_flags) return fail(K2H_AMD_EINVAL, "ralledata_unlink: NULL sk_flags");
  if (n && !edge_off) return fail(K2H_AMD_EINVAL, "ralledata_unlink: NULL edge_off");
  if (out && !out_off) return fail(K2H_AMD_EINVAL, "ralledata_unlink: out given without out_off");
  if (n > 0xFFFFFFFEull) return fail(K2H_AMD_EINVAL, "ralledata_unlink: more than 2^32 - 2 blobs (ranks are 32-bit values)");
  if (n == 0 && !out_off) return K2H_AMD_OK;
  K2H_GATE();
  hipError_t e = hipSuccess;
  if (n == 0) return clear_word(out_off, stream, "ralledata_unlink: hipMemsetAsync");  // no blob
  int rc = k2h::launch_ralledata_unlink(blobs, size, blob_off, n, keep, sk_flags, edge_off, drop, out, out_cap, out_off,
                                        index, changed, counts, (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EINVAL) return exceeds_cap("ralledata_unlink", "emitted blobs", counts[1], out_cap);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_ralledata_unlink", e);
}

__attribute__((visibility("default"))) int k2h_amd_subkeys_drop_mask(const uint64_t* child, uint64_t edges,
                                                                     const uint8_t* gone, uint64_t n, int dangling,
                                                                     uint8_t* drop, void* stream) {
  if (edges == 0) return K2H_AMD_OK;
  if (!child) return fail(K2H_AMD_EINVAL, "subkeys_drop_mask: NULL child");
  if (!drop) return fail(K2H_AMD_EINVAL, "subkeys_drop_mask: NULL drop");
  K2H_GATE();
  hipError_t e = k2h::launch_subkeys_drop_mask(child, edges, gone, n, dangling, drop, (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "launch_subkeys_drop_mask", e);
}

// Section 4b'': the stream split into parts.  Judged on the host like the three above.
__attribute__((visibility("default"))) int k2h_amd_ralledata_partition(
    const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n, const k2h_amd_part_rule* rule,
    const uint32_t* part_ids, const uint8_t* consider, void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* index,
    uint32_t* part_out, uint64_t* part_first, uint64_t* part_byte, void* stream) {
  if (!rule) return fail(K2H_AMD_EINVAL, "ralledata_partition: NULL rule");
  if (rule->kind != K2H_AMD_PART_IDS && rule->kind != K2H_AMD_PART_OWNER && rule->kind != K2H_AMD_PART_MASK)
    return fail(K2H_AMD_EINVAL, "ralledata_partition: unknown rule kind");
  if (rule->parts == 0 || rule->parts > K2H_AMD_PART_MAX)
    return fail(K2H_AMD_EINVAL, "ralledata_partition: parts must be 1 .. K2H_AMD_PART_MAX (256)");
  if (!part_first) return fail(K2H_AMD_EINVAL, "ralledata_partition: NULL part_first");
  if (!part_byte) return fail(K2H_AMD_EINVAL, "ralledata_partition: NULL part_byte");
  if (rule->kind == K2H_AMD_PART_IDS && !part_ids)
    return fail(K2H_AMD_EINVAL, "ralledata_partition: K2H_AMD_PART_IDS needs part_ids");
  if (rule->kind != K2H_AMD_PART_IDS && part_ids)
    return fail(K2H_AMD_EINVAL, "ralledata_partition: part_ids given with a hash rule");
  if (rule->kind == K2H_AMD_PART_OWNER) {
    if (rule->max_hash == 0) return fail(K2H_AMD_EINVAL, "ralledata_partition: OWNER max_hash is 0");
    if (rule->span == 0) return fail(K2H_AMD_EINVAL, "ralledata_partition: OWNER span is 0");
    if ((rule->max_hash - 1) / rule->span + 1 != (uint64_t)rule->parts)
      return fail(K2H_AMD_EINVAL, "ralledata_partition: OWNER parts is not ceil(max_hash / span)");
  }
  for (uint32_t p = 0; p <= rule->parts; ++p) part_first[p] = part_byte[p] = 0;
  if (n == 0) return K2H_AMD_OK;
  if (!blobs) return fail(K2H_AMD_EINVAL, "ralledata_partition: NULL blobs");
  if (!blob_off) return fail(K2H_AMD_EINVAL, "ralledata_partition: NULL blob_off");
  if (out && !out_off) return fail(K2H_AMD_EINVAL, "ralledata_partition: out given without out_off");
  K2H_GATE();
  hipError_t e = hipSuccess;
  int rc = k2h::launch_ralledata_partition(blobs, size, blob_off, n, *rule, part_ids, consider, out, out_cap, out_off,
                                           index, part_out, part_first, part_byte, (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EHIP || rc == K2H_AMD_ENOMEM) return fail(rc, "launch_ralledata_partition", e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "ralledata_partition: the kept blobs exceed out_cap, or too many blobs");
}

// ---------------------------------------------------------------------------
// RALLEDATA blobs from range records (include/k2hash_amd.h section 4c).  Arguments are judged
// before the device gate, so a bad call fails the same way with or without a GPU.
// ---------------------------------------------------------------------------
namespace {

// What both forms check on the host; returns > 0 when the call is already answered.
int recs_ralledata_args(const char* who, const void* file, uint64_t size, const void* recs, uint64_t n,
                        uint64_t* blob_off, uint64_t* total, uint32_t flags, void* stream, int* rc) {
  static thread_local char msg[96];
  auto bad = [&](const char* what) {
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    *rc = fail(K2H_AMD_EINVAL, msg);
    return 1;
  };
  if (flags & K2H_AMD_FLAG_CSTR) return bad("the terminators are fixed by the form, not by K2H_AMD_FLAG_CSTR");
  if (!total) return bad("NULL total");
  *total = 0;
  if (n == 0) {
    *rc = K2H_AMD_OK;
    if (blob_off) {
      if ((*rc = gate_current())) return 1;
      *rc = clear_word(blob_off, stream, who);
    }
    return 1;
  }
  if (!blob_off || !recs || (size && !file)) return bad("NULL file/recs/blob_off");
  // a blob is at most 80 + 2 + 2 size (import) or 80 + 4 size (archive) bytes
  if (size > (~0ull - 82) / 4 || n > ~0ull / (82 + 4 * size)) return bad("n blobs of this file overflow 64 bits");
  return 0;
}

}  // namespace

__attribute__((visibility("default"))) int k2h_amd_import_ralledata(const void* file, uint64_t size,
                                                                    const k2h_amd_import_rec* recs, uint64_t n,
                                                                    void* out, uint64_t out_cap, uint64_t* blob_off,
                                                                    uint64_t* total, uint32_t flags, void* stream) {
  int rc = K2H_AMD_OK;
  if (recs_ralledata_args("import_ralledata", file, size, recs, n, blob_off, total, flags, stream, &rc)) return rc;
  K2H_GATE();
  hipError_t e = hipSuccess;
  rc = k2h::launch_import_ralledata(file, size, recs, n, seed_for(flags), out, out_cap, blob_off, total,
                                    (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EHIP) return fail(rc, "launch_import_ralledata", e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "import_ralledata: the blobs exceed out_cap, or too many records");
}

__attribute__((visibility("default"))) int k2h_amd_archive_ralledata(const void* file, uint64_t size,
                                                                     const k2h_amd_archive_rec* recs, uint64_t n,
                                                                     void* out, uint64_t out_cap, uint64_t* blob_off,
                                                                     uint64_t* total, uint32_t flags, void* stream) {
  int rc = K2H_AMD_OK;
  if (recs_ralledata_args("archive_ralledata", file, size, recs, n, blob_off, total, flags, stream, &rc)) return rc;
  K2H_GATE();
  hipError_t e = hipSuccess;
  rc = k2h::launch_archive_ralledata(file, size, recs, n, seed_for(flags), out, out_cap, blob_off, total,
                                     (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EHIP) return fail(rc, "launch_archive_ralledata", e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "archive_ralledata: the blobs exceed out_cap, or too many records");
}

// ---------------------------------------------------------------------------
// A blob stream written as a k2hash archive (include/k2hash_amd.h section 4d).  Arguments are
// judged before the device gate, so a bad call fails the same way with or without a GPU.
// ---------------------------------------------------------------------------
__attribute__((visibility("default"))) int k2h_amd_ralledata_archive(const void* blobs, uint64_t size,
                                                                     const uint64_t* blob_off, uint64_t n,
                                                                     const uint8_t* keep, void* out, uint64_t out_cap,
                                                                     uint64_t* rec_off, uint64_t* records,
                                                                     uint64_t* total, void* stream) {
  if (!total) return fail(K2H_AMD_EINVAL, "ralledata_archive: NULL total");
  *total = 0;
  if (records) *records = 0;
  if (n == 0) {
    if (!rec_off) return K2H_AMD_OK;
    K2H_GATE();
    return clear_word(rec_off, stream, "ralledata_archive");
  }
  if (!rec_off) return fail(K2H_AMD_EINVAL, "ralledata_archive: NULL rec_off");
  if (!blobs) return fail(K2H_AMD_EINVAL, "ralledata_archive: NULL blobs");
  if (!blob_off) return fail(K2H_AMD_EINVAL, "ralledata_archive: NULL blob_off");
  // a record is at most 104 + 4 size bytes (each of a blob's four segments lies inside it)
  if (size > (~0ull - K2H_AMD_SCOM_HEADER) / 4 || n > ~0ull / (K2H_AMD_SCOM_HEADER + 4 * size))
    return fail(K2H_AMD_EINVAL, "ralledata_archive: n records of this stream overflow 64 bits");
  K2H_GATE();
  hipError_t e = hipSuccess;
  int rc = k2h::launch_ralledata_archive(blobs, size, blob_off, n, keep, out, out_cap, rec_off, records, total,
                                         (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EHIP) return fail(rc, "launch_ralledata_archive", e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "ralledata_archive: the records exceed out_cap, or too many blobs");
}

// Section 4d': the log that turns the held stream into the new one.  Judged on the host before
// any device is touched.
__attribute__((visibility("default"))) int k2h_amd_ralledata_delta(
    const void* a_blobs, uint64_t a_size, const uint64_t* a_off, uint64_t na, const uint8_t* rel, const void* b_blobs,
    uint64_t b_size, const uint64_t* b_off, uint64_t nb, const uint8_t* b_consider, const uint8_t* seen, void* out,
    uint64_t out_cap, uint64_t* slot_off, uint8_t* made, uint64_t* counts, void* stream) {
  if (!counts) return fail(K2H_AMD_EINVAL, "ralledata_delta: NULL counts");
  for (int k = 0; k < 8; ++k) counts[k] = 0;
  if (na && !rel) return fail(K2H_AMD_EINVAL, "ralledata_delta: NULL rel");
  if (na && !a_blobs) return fail(K2H_AMD_EINVAL, "ralledata_delta: NULL a_blobs");
  if (na && !a_off) return fail(K2H_AMD_EINVAL, "ralledata_delta: NULL a_off");
  if (nb && seen && !b_blobs) return fail(K2H_AMD_EINVAL, "ralledata_delta: seen given with NULL b_blobs");
  if (nb && seen && !b_off) return fail(K2H_AMD_EINVAL, "ralledata_delta: seen given with NULL b_off");
  if (out && !slot_off && (na || nb)) return fail(K2H_AMD_EINVAL, "ralledata_delta: out given without slot_off");
  if (na > 0xFFFFFFFEull || nb > 0xFFFFFFFEull - na)
    return fail(K2H_AMD_EINVAL,
                "ralledata_delta: more than 2^32 - 2 slots (neither the ranks of the emitting slots nor a launch grid "
                "would fit)");
  if (na + nb == 0 && !slot_off) return K2H_AMD_OK;
  K2H_GATE();
  hipError_t e = hipSuccess;
  if (na + nb == 0) return clear_word(slot_off, stream, "ralledata_delta: hipMemsetAsync");  // no slot
  int rc = k2h::launch_ralledata_delta(a_blobs, a_size, a_off, na, rel, b_blobs, b_size, b_off, nb, b_consider, seen, out,
                                       out_cap, slot_off, made, counts, (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EINVAL) return exceeds_cap("ralledata_delta", "records", counts[1], out_cap);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_ralledata_delta", e);
}

// Section 4e: keys looked up in a held stream.  Judged on the host like the ones above.
__attribute__((visibility("default"))) uint64_t k2h_amd_ralledata_index_size(uint64_t n) {
  return k2h::ralledata_index_bytes(n);
}

__attribute__((visibility("default"))) int k2h_amd_ralledata_index(const void* blobs, uint64_t size,
                                                                   const uint64_t* blob_off, uint64_t n,
                                                                   const uint8_t* consider, void* index,
                                                                   uint64_t index_cap, uint64_t* participants,
                                                                   void* stream) {
  if (participants) *participants = 0;
  if (n && !blobs) return fail(K2H_AMD_EINVAL, "ralledata_index: NULL blobs");
  if (n && !blob_off) return fail(K2H_AMD_EINVAL, "ralledata_index: NULL blob_off");
  if (!index) return fail(K2H_AMD_EINVAL, "ralledata_index: NULL index");
  if (n > 0xFFFFFFFEull)
    return fail(K2H_AMD_EINVAL, "ralledata_index: more than 2^32 - 2 blobs (indices are sorted as 32-bit values)");
  if (index_cap < k2h::ralledata_index_bytes(n)) {
    char msg[160];
    snprintf(msg, sizeof msg, "ralledata_index: index_cap %llu is below k2h_amd_ralledata_index_size(n) = %llu",
             (unsigned long long)index_cap, (unsigned long long)k2h::ralledata_index_bytes(n));
    return fail(K2H_AMD_EINVAL, msg);
  }
  if ((uintptr_t)index & 255u) return fail(K2H_AMD_EINVAL, "ralledata_index: index is not 256-byte aligned");
  K2H_GATE();
  hipError_t e = hipSuccess;
  int rc = k2h::launch_ralledata_index(blobs, size, blob_off, n, consider, index, participants, (hipStream_t)stream, &e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_ralledata_index", e);
}

__attribute__((visibility("default"))) int k2h_amd_ralledata_find(
    const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n, const void* index, const void* keys,
    uint64_t key_bytes, const uint64_t* key_off, uint64_t m, const uint64_t* h1, const uint64_t* h2, uint32_t flags,
    const k2h_amd_timespec* now, uint64_t* match, uint8_t* status, uint8_t* hit, uint64_t* counts, void* stream) {
  if (counts) counts[0] = counts[1] = counts[2] = 0;
  if (m && !status) return fail(K2H_AMD_EINVAL, "ralledata_find: NULL status");
  if (key_bytes && !keys) return fail(K2H_AMD_EINVAL, "ralledata_find: NULL keys");
  if (m && !key_off) return fail(K2H_AMD_EINVAL, "ralledata_find: NULL key_off");
  if (!index) return fail(K2H_AMD_EINVAL, "ralledata_find: NULL index");
  if (n && !blobs) return fail(K2H_AMD_EINVAL, "ralledata_find: NULL blobs");
  if (n && !blob_off) return fail(K2H_AMD_EINVAL, "ralledata_find: NULL blob_off");
  if (!h1 != !h2) return fail(K2H_AMD_EINVAL, "ralledata_find: h1 and h2 go together, both given or both NULL");
  if (flags & ~(K2H_AMD_FLAG_STD_FNV | K2H_AMD_FLAG_CSTR)) return fail(K2H_AMD_EINVAL, "ralledata_find: unknown flags");
  if ((flags & K2H_AMD_FLAG_STD_FNV) && h1)
    return fail(K2H_AMD_EINVAL, "ralledata_find: K2H_AMD_FLAG_STD_FNV is legal only when h1 and h2 are NULL");
  if (n > 0xFFFFFFFEull)
    return fail(K2H_AMD_EINVAL, "ralledata_find: more than 2^32 - 2 blobs (indices are sorted as 32-bit values)");
  if (m == 0 && !(hit && n)) return K2H_AMD_OK;
  K2H_GATE();
  hipError_t e = hipSuccess;
  if (m == 0) {  // no query: no blob is a match
    e = hipMemsetAsync(hit, 0, n, (hipStream_t)stream);
    return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "ralledata_find: hipMemsetAsync", e);
  }
  int rc = k2h::launch_ralledata_find(blobs, size, blob_off, n, index, keys, key_bytes, key_off, m, h1, h2,
                                      seed_for(flags), (flags & K2H_AMD_FLAG_CSTR) != 0, now, match, status, hit, counts,
                                      (hipStream_t)stream, &e);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_ralledata_find", e);
}

__attribute__((visibility("default"))) int k2h_amd_ralledata_fetch(const void* blobs, uint64_t size,
                                                                   const uint64_t* blob_off, uint64_t n,
                                                                   const uint64_t* which, uint64_t m,
                                                                   const uint8_t* take, uint32_t segment, void* out,
                                                                   uint64_t out_cap, uint64_t* out_off, uint8_t* bad,
                                                                   uint64_t* total, void* stream) {
  if (!total) return fail(K2H_AMD_EINVAL, "ralledata_fetch: NULL total");
  *total = 0;
  if (m && !which) return fail(K2H_AMD_EINVAL, "ralledata_fetch: NULL which");
  if (m && n && !blobs) return fail(K2H_AMD_EINVAL, "ralledata_fetch: NULL blobs");
  if (m && n && !blob_off) return fail(K2H_AMD_EINVAL, "ralledata_fetch: NULL blob_off");
  if (segment > K2H_AMD_SEG_ATTRS) return fail(K2H_AMD_EINVAL, "ralledata_fetch: unknown segment");
  if (out && !out_off) return fail(K2H_AMD_EINVAL, "ralledata_fetch: out given without out_off");
  if (m == 0 && !out_off) return K2H_AMD_OK;
  K2H_GATE();
  hipError_t e = hipSuccess;
  if (m == 0) return clear_word(out_off, stream, "ralledata_fetch: hipMemsetAsync");  // no slot
  int rc = k2h::launch_ralledata_fetch(blobs, size, blob_off, n, which, m, take, segment, out, out_cap, out_off, bad,
                                       total, (hipStream_t)stream, &e);
  if (rc == K2H_AMD_EINVAL) return exceeds_cap("ralledata_fetch", "segments", *total, out_cap);
  return rc == K2H_AMD_OK ? rc : fail(rc, "launch_ralledata_fetch", e);
}

__attribute__((visibility("default"))) const char* k2h_amd_version(void) {
  return "k2hash_amd 0.1 (FNV-1A BUILTIN, gfx950 HIP batch kernels)";
}

__attribute__((visibility("default"))) const char* k2h_amd_strerror(int code) {
  static const char* names[] = {"ok", "invalid argument", "HIP runtime error", "out of memory", "no device"};
  if (code == 0) return names[0];
  if (g_err[0]) return g_err;
  if (code < 0 && code >= -4) return names[-code];
  return "unknown error";
}


__attribute__((visibility("default"))) int k2h_amd_synth_bytes(void* out, uint64_t nbytes, uint64_t seed,
                                                               uint64_t byte_off, void* stream) {
  if (nbytes && !out) return fail(K2H_AMD_EINVAL, "out is NULL");
  K2H_GATE();
  hipError_t e = k2h::launch_synth_bytes((uint8_t*)out, nbytes, seed, byte_off, (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "synth_bytes", e);
}

__attribute__((visibility("default"))) int k2h_amd_synth_lengths(uint32_t* lens, uint64_t n, uint64_t seed,
                                                                 uint64_t first_key, uint32_t min_len,
                                                                 uint32_t max_len, void* stream) {
  if (n && !lens) return fail(K2H_AMD_EINVAL, "lens is NULL");
  if (max_len < min_len) return fail(K2H_AMD_EINVAL, "max_len < min_len");
  K2H_GATE();
  hipError_t e = k2h::launch_synth_lengths(lens, n, seed, first_key, min_len, max_len, (hipStream_t)stream);
  return e == hipSuccess ? K2H_AMD_OK : fail(K2H_AMD_EHIP, "synth_lengths", e);
}

}  // extern "C"
