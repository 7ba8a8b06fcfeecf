// k2hash_amd -- the one way a device launcher keeps its temporaries ("Scratch
// policy"): one grow-only device buffer per launcher family and device, held across calls under
// a per-device lock and cut into columns by a Carver (k2h_layout.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <mutex>

#include "../../include/k2hash_amd.h"
#include "k2h_layout.h"

namespace k2h {

// The first HIP error of a launcher's calls: tr(call) for each, tr.e at the end.
struct FirstError {
  hipError_t e = hipSuccess;
  void operator()(hipError_t x) {
    if (e == hipSuccess) e = x;
  }
  bool ok() const { return e == hipSuccess; }
};

// The scanners free a buffer above this at the end of the call that needed it: per-call pool
// allocations of the temporaries' size cost ~0.15 ms per hipFreeAsync on MI355X (rocprofv3
// --runtime-trace, profiles/r03f_import_api_stats.csv), more than the scan itself, so the
// buffer is held across calls -- but a file of several GB does not pin its peak for the life of
// the process.
constexpr size_t kScratchKeep = (size_t)512 << 20;  // > the temporaries of a 1.2 GB TSV file (~20 % of its size)

struct DeviceScratch {
  std::mutex mu;
  void* p = nullptr;
  size_t bytes = 0;
  hipEvent_t done = nullptr;  // stays null for a launcher that synchronises before it unlocks

  // Under mu: at least `total` bytes at p.  Returns a K2H_AMD_* code (the HIP error in *herr).
  int grow(size_t total, hipError_t* herr) {
    hipError_t e = hipSuccess;
    if (bytes < total) {
      if (p) e = hipFree(p);  // waits for the device: no earlier call's kernel still uses it
      p = nullptr;
      bytes = 0;
      const hipError_t a = e == hipSuccess ? hipMalloc(&p, total) : e;
      if (a == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        p = nullptr;
        *herr = a;
        return K2H_AMD_ENOMEM;
      }
      if (e == hipSuccess) e = a;
      if (e == hipSuccess) bytes = total;
    }
    *herr = e;
    return e == hipSuccess ? K2H_AMD_OK : K2H_AMD_EHIP;
  }

  // For a launcher whose kernels still use the buffer after it has returned: grow, and `stream`
  // behind the last call's event.  Such a launcher ends with mark_done.
  int reserve(size_t total, hipStream_t stream, hipError_t* herr) {
    *herr = done ? hipSuccess : hipEventCreateWithFlags(&done, hipEventDisableTiming);
    if (*herr != hipSuccess) return K2H_AMD_EHIP;
    if (const int rc = grow(total, herr)) return rc;
    *herr = hipStreamWaitEvent(stream, done, 0);  // never recorded: no wait
    return *herr == hipSuccess ? K2H_AMD_OK : K2H_AMD_EHIP;
  }
  hipError_t mark_done(hipStream_t stream) { return hipEventRecord(done, stream); }

  // For a launcher that has synchronised its stream: no kernel still reads the buffer.
  void release_above(size_t keep) {
    if (bytes <= keep) return;
    (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// A launcher family's instances, one per device.
template <class S = DeviceScratch>
class PerDevice {
 public:
  // The current device's instance; null with the error in tr (hipGetDevice's, or
  // hipErrorInvalidDevice), also when tr held an error before.
  S* current(FirstError& tr) {
    int dev = 0;
    tr(hipGetDevice(&dev));
    if (tr.ok() && (dev < 0 || dev >= kDevices)) tr.e = hipErrorInvalidDevice;
    return tr.ok() ? &at_[dev] : nullptr;
  }

 private:
  static constexpr int kDevices = 64;
  S at_[kDevices];
};

}  // namespace k2h
