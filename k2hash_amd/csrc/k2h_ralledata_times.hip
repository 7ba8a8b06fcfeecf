// k2hash_amd -- RALLEDATA consumer side: the mtime and expire of every blob of a stream in
// device memory, and the time-window selection of K2HShm::GetElementListToBinary
// (include/k2hash_amd.h section 4b''''; lib/k2hshmdirect.cc:137-197).
//
// One lane per blob: span, header and classify (k2h_ralle_header.h, the participants of
// _dedup), then, for a participant with attrs, the serial walk of k2h_ralle_attrs.h.  The
// walk is a chain of dependent 16-byte loads, one per attrs entry.  The kernel holds a header's
// ten fields and the walk's few words (34 VGPRs), so every wave slot of a SIMD would be usable;
// it is launched with kWalkLdsBytes of LDS it never touches, which leaves two waves per SIMD
// resident, because it measures a third faster that way (k2h_ralle_attrs.h).
//
// No byte outside [0, size) is read: the header of a good span is inside it, classify keeps
// the attrs segment inside the blob, and every load of the walk lies inside the segment.
// Nothing of a non-participant beyond its header is read, and no header of a bad span.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k2h_kernels.h"
#include "k2h_ralle_attrs.h"
#include "k2h_ralle_header.h"

namespace k2h {
namespace {

constexpr int kTimesBlock = 256;  // blobs per block, one per thread

__global__ __launch_bounds__(kTimesBlock) void ralledata_times_kernel(
    const uint8_t* __restrict__ blobs, uint64_t size, const uint64_t* __restrict__ off, uint64_t n,
    const uint8_t* __restrict__ consider, k2h_amd_time_window win, bool have_win, const uint8_t* __restrict__ route,
    uint8_t* __restrict__ tflags, int64_t* __restrict__ mtime, int64_t* __restrict__ expire,
    uint8_t* __restrict__ keep) {
  const uint64_t i = (uint64_t)blockIdx.x * kTimesBlock + threadIdx.x;
  if (i >= n) return;
  bool part = false;
  AttrTimes t = {0, 0, 0, 0, 0};
  uint32_t attrs_bit = 0;
  if (!consider || consider[i]) {
    const uint64_t b = off[i], e = off[i + 1];
    if (e >= b && e <= size && e - b >= (uint64_t)kHdr) {
      uint64_t f[10];
      load_fields(blobs + b, f);
      if (classify(f, e - b) == K2H_AMD_RALLE_OK) {
        part = true;
        if (f[5]) {
          attrs_bit = K2H_AMD_TIMES_ATTRS;
          t = walk_attrs(blobs + b + f[9], f[5]);
        }
      }
    }
  }
  if (tflags) tflags[i] = (uint8_t)(t.flags | attrs_bit);
  if (mtime) {
    mtime[2 * i] = t.msec;
    mtime[2 * i + 1] = t.mnsec;
  }
  if (expire) {
    expire[2 * i] = t.esec;
    expire[2 * i + 1] = t.ensec;
  }
  if (keep) {
    bool k = part;
    if (part && have_win) {
      // lib/k2hshmdirect.cc:146-151, then :155-189
      if ((win.flags & K2H_AMD_WIN_EXPIRE) && (t.flags & kAttrExpire) &&
          time_less(t.esec, t.ensec, win.now.sec, win.now.nsec)) {
        k = false;
      } else if (t.flags & kAttrMtime) {
        const bool need_start = !route || (route[i] & K2H_AMD_ROUTE_OLD);
        if (need_start && (win.flags & K2H_AMD_WIN_START) &&
            time_less(t.msec, t.mnsec, win.start.sec, win.start.nsec))
          k = false;
        else if ((win.flags & K2H_AMD_WIN_END) && time_less(win.end.sec, win.end.nsec, t.msec, t.mnsec))
          k = false;
      }
    }
    keep[i] = k ? 1 : 0;
  }
}

}  // namespace

// Asynchronous on the stream.  n >= 1; window may be NULL.
hipError_t launch_ralledata_times(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                                  const uint8_t* consider, const k2h_amd_time_window* window, const uint8_t* route,
                                  uint8_t* tflags, int64_t* mtime, int64_t* expire, uint8_t* keep,
                                  hipStream_t stream) {
  const uint64_t grid = (n + kTimesBlock - 1) / kTimesBlock;
  if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
  k2h_amd_time_window win = {};
  if (window) win = *window;
  ralledata_times_kernel<<<(unsigned)grid, kTimesBlock, kWalkLdsBytes, stream>>>((const uint8_t*)blobs, size, blob_off, n,
                                                                    consider, win, window != nullptr, route, tflags,
                                                                    mtime, expire, keep);
  return hipGetLastError();
}

}  // namespace k2h
