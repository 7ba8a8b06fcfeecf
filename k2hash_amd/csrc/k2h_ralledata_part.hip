// k2hash_amd -- RALLEDATA consumer side: a stable P-way partition of a blob stream in device
// memory (include/k2hash_amd.h section 4b''), the P-way sibling of the select kernels
// (k2h_ralledata_check.hip).
//
// Blob i = blobs[off[i], off[i+1]).  A blob that takes part gets a part 0 <= p < parts, from
// the caller's ids, from its stored hash's owner ((hash % max_hash) / span, the selection of
// K2HShm::GetElementListToBinary, lib/k2hshmdirect.cc:118-131, cut into consecutive ranges) or
// from its collision slot ((hash & mask) % parts; hash & collision_mask is the CKINDEX slot,
// lib/k2hshm.cc:1093); the output holds part 0's blobs in stream order, then part 1's, ...
//
//   count   per tile of kPartBlobs blobs: every blob's part (the one pass that reads headers,
//           8 bytes each) into the call's id array, and the tile's (count, bytes) per part from
//           an LDS histogram, written part-major: entry p * ntiles + t
//   scan    one exclusive sum over the parts * ntiles + 1 entries of each of the two arrays, in
//           place: entry p * ntiles + t becomes where tile t's blobs of part p begin (as a rank
//           and as a byte offset), entry p * ntiles where part p begins
//   bounds  those parts + 1 entries of each array, gathered for one copy to the host
//   copy    per tile: a stable block sort of (id, index in tile) gives each blob its rank among
//           the tile's blobs of its part, a block sum in that order the bytes before it; then
//           the blobs are moved, 16 lanes to a blob
//
// Every address is byte-aligned.  No byte outside a participant's span is read, nothing of a
// blob that does not take part, and of a participant's header only its first 8 bytes, once.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <mutex>

#include "k2h_fnv_device.h"
#include "k2h_kernels.h"
#include "k2h_scratch.h"

namespace k2h {
namespace {

constexpr int kPartBlobs = 1024;   // blobs per 256-thread block, four per thread
constexpr int kPartThreads = 256;
constexpr int kPartPer = kPartBlobs / kPartThreads;
constexpr int kPartLanes = 16;     // lanes that move one blob: up to 256 bytes a trip
constexpr int kPartLong = 4096;    // a blob of at least this many bytes is moved by the whole block
constexpr uint16_t kNoPart = K2H_AMD_PART_MAX;  // the id of a blob left out
static_assert(K2H_AMD_PART_MAX == 256 && kPartThreads >= K2H_AMD_PART_MAX, "one thread per part");
static_assert(kPartLanes >= 16 && kPartThreads % kPartLanes == 0, "a lane per head / tail byte");

typedef uint64_t u64_ua __attribute__((aligned(1)));

// ------------------------------------------------------------------------------- count
// The histogram takes LDS atomics: 1024 adds a tile on as few as `parts` addresses, a few
// thousand cycles next to the tile's 1024 scattered header reads.
__global__ __launch_bounds__(kPartThreads) void ralledata_part_count_kernel(
    const uint8_t* __restrict__ blobs, uint64_t size, const uint64_t* __restrict__ off, uint64_t n,
    k2h_amd_part_rule rule, const uint32_t* __restrict__ part_ids, const uint8_t* __restrict__ consider,
    uint64_t ntiles, uint16_t* __restrict__ ids, uint32_t* __restrict__ part_out, uint64_t* __restrict__ hist_count,
    uint64_t* __restrict__ hist_bytes) {
  __shared__ unsigned long long cnt[K2H_AMD_PART_MAX], bytes[K2H_AMD_PART_MAX];
  const uint32_t tid = threadIdx.x;
  if (tid < rule.parts) cnt[tid] = bytes[tid] = 0;
  __syncthreads();
  const uint64_t r0 = (uint64_t)blockIdx.x * kPartBlobs;
#pragma unroll
  for (int k = 0; k < kPartPer; ++k) {
    const uint64_t i = r0 + (uint32_t)k * kPartThreads + tid;
    if (i >= n) break;
    uint32_t part = kNoPart;
    uint64_t len = 0;
    if (!consider || consider[i]) {
      const uint64_t s = off[i], e = off[i + 1];
      if (e >= s && e <= size) {
        len = e - s;
        if (rule.kind == K2H_AMD_PART_IDS) {
          const uint32_t v = part_ids[i];
          if (v < rule.parts) part = v;
        } else if (len >= (uint64_t)K2H_AMD_RALLEDATA_HEADER) {
          const uint64_t h = *reinterpret_cast<const u64_ua*>(blobs + s);
          part = rule.kind == K2H_AMD_PART_OWNER ? (uint32_t)((h % rule.max_hash) / rule.span)
                                                 : (uint32_t)((h & rule.mask) % rule.parts);
        }
      }
    }
    ids[i] = (uint16_t)part;
    if (part_out) part_out[i] = part == kNoPart ? K2H_AMD_PART_NONE : part;
    if (part != kNoPart) {
      atomicAdd(&cnt[part], 1ull);
      atomicAdd(&bytes[part], (unsigned long long)len);
    }
  }
  __syncthreads();
  if (tid < rule.parts) {
    hist_count[(uint64_t)tid * ntiles + blockIdx.x] = cnt[tid];
    hist_bytes[(uint64_t)tid * ntiles + blockIdx.x] = bytes[tid];
  }
}

// bounds[p] = where part p begins as a rank, bounds[parts + 1 + p] as a byte offset (p <= parts)
__global__ __launch_bounds__(kPartThreads) void ralledata_part_bounds_kernel(const uint64_t* __restrict__ scan_count,
                                                                            const uint64_t* __restrict__ scan_bytes,
                                                                            uint64_t ntiles, uint32_t parts,
                                                                            uint64_t* __restrict__ bounds) {
  for (uint32_t p = threadIdx.x; p <= parts; p += kPartThreads) {
    bounds[p] = scan_count[(uint64_t)p * ntiles];
    bounds[parts + 1 + p] = scan_bytes[(uint64_t)p * ntiles];
  }
}

// -------------------------------------------------------------------------------- copy
// Blob [s, s + L) of the stream to [d, d + L) of out by `lanes` lanes (this one is `lane`): the
// 16-byte pieces ALIGNED IN OUT that lie wholly inside the blob are one unaligned load and one
// aligned store each; the up to 15 bytes before the first such piece and behind the last one
// share their piece with a neighbour in out -- usually a blob of another tile, so the piece is
// never read or written as a whole -- and are stored byte by byte.
__device__ __forceinline__ void move_blob(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, uint64_t L,
                                          uint32_t lane, uint32_t lanes) {
  typedef uint32_t u32x4_al __attribute__((ext_vector_type(4)));
  const uint64_t to_piece = (uint64_t)(-(uintptr_t)d & 15u);
  const uint64_t head = to_piece < L ? to_piece : L;
  const uint64_t np = (L - head) >> 4, tail = head + 16 * np;
  const uint8_t* sb = s + head;
  uint8_t* db = d + head;
  uint64_t q = lane;
  for (; q + 3ull * lanes < np; q += 4ull * lanes) {  // long blobs: four loads in flight
    u32x4_ua w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = *reinterpret_cast<const u32x4_ua*>(sb + 16 * (q + (uint64_t)u * lanes));
#pragma unroll
    for (int u = 0; u < 4; ++u)
      *reinterpret_cast<u32x4_al*>(db + 16 * (q + (uint64_t)u * lanes)) = u32x4_al{w[u].x, w[u].y, w[u].z, w[u].w};
  }
  for (; q < np; q += lanes) {
    const u32x4_ua w = *reinterpret_cast<const u32x4_ua*>(sb + 16 * q);
    *reinterpret_cast<u32x4_al*>(db + 16 * q) = u32x4_al{w.x, w.y, w.z, w.w};
  }
  if (lane < head) d[lane] = s[lane];
  if (lane < 16 && tail + lane < L) d[tail + lane] = s[tail + lane];
}

// A block takes the tile's kPartBlobs blobs, thread t blobs 4 t .. 4 t + 3 of the tile.  Ids and
// spans are the count kernel's (no header is read here).  Sorted stably by id, the blobs of one
// part are consecutive and in stream order: a blob's rank in its part's run of the tile is its
// sorted position less the run's first, the bytes before it the block sum up to it less the sum
// at the run's first; the scanned histogram entry of (part, this tile) is added to both.  The
// sort takes id_bits bits: ids 0 .. parts, the last one a blob left out.  Block-relative
// positions are 16- and 32-bit; byte sums, sources and destinations are 64-bit.
// 25 KiB of LDS: six blocks per CU.  (A form with 38 KiB, four blocks per CU, took the same time,
// and so did one that kept four blobs per group in flight: DESIGN.md 5.4d.)
__global__ __launch_bounds__(kPartThreads) void ralledata_part_copy_kernel(
    const uint8_t* __restrict__ blobs, const uint64_t* __restrict__ off, uint64_t n, const uint16_t* __restrict__ ids,
    const uint64_t* __restrict__ scan_count, const uint64_t* __restrict__ scan_bytes, uint64_t ntiles, uint32_t parts,
    int id_bits, uint8_t* __restrict__ out, uint64_t* __restrict__ out_off, uint64_t* __restrict__ index) {
  typedef hipcub::BlockRadixSort<uint16_t, kPartThreads, kPartPer, uint16_t> Sort;
  typedef hipcub::BlockScan<uint64_t, kPartThreads> Scan;
  __shared__ union {
    typename Sort::TempStorage sort;
    typename Scan::TempStorage scan;
  } tmp;
  constexpr uint64_t kLeftOut = ~0ull;
  __shared__ uint64_t span[kPartBlobs + 1];  // by index in the tile: the tile's offsets as given,
  __shared__ uint64_t dst[kPartBlobs];       // the blob's first byte in out, kLeftOut when it is left out
  // of (part, this tile): the scanned rank / byte offset, less the run's first sorted position /
  // the block sum there once the run's first blob has subtracted them (mod 2^64)
  __shared__ uint64_t base_rank[K2H_AMD_PART_MAX], base_byte[K2H_AMD_PART_MAX];
  __shared__ uint16_t last_id[kPartThreads];
  __shared__ uint32_t is_long[kPartBlobs / 32];  // bit j: blob j is moved by the whole block
  const uint32_t tid = threadIdx.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * kPartBlobs;
  const uint32_t nr = (uint32_t)(n - r0 < (uint64_t)kPartBlobs ? n - r0 : (uint64_t)kPartBlobs);
  if (tid < parts) {
    base_rank[tid] = scan_count[(uint64_t)tid * ntiles + blockIdx.x];
    base_byte[tid] = scan_bytes[(uint64_t)tid * ntiles + blockIdx.x];
  }
  if (tid < kPartBlobs / 32) is_long[tid] = 0;
  if (blockIdx.x == 0 && tid == 0) out_off[scan_count[(uint64_t)parts * ntiles]] = scan_bytes[(uint64_t)parts * ntiles];
  for (uint32_t j = tid; j <= nr; j += kPartThreads) span[j] = off[r0 + j];
  uint16_t key[kPartPer], val[kPartPer];
#pragma unroll
  for (int k = 0; k < kPartPer; ++k) {
    const uint32_t j = kPartPer * tid + k;
    key[k] = (uint16_t)parts;
    val[k] = (uint16_t)j;
    if (j < nr) {
      const uint16_t id = ids[r0 + j];
      if (id != kNoPart) key[k] = id;
    }
    dst[j] = kLeftOut;
  }
  Sort(tmp.sort).Sort(key, val, 0, id_bits);  // blocked: thread t holds sorted positions 4 t .. 4 t + 3
  last_id[tid] = key[kPartPer - 1];
  __syncthreads();  // span / dst / last_id written, the sort's storage free
  uint64_t L[kPartPer], x[kPartPer];
#pragma unroll
  for (int k = 0; k < kPartPer; ++k)  // a participant's span is good (the count kernel judged it)
    L[k] = key[k] < parts ? span[val[k] + 1] - span[val[k]] : 0;
  Scan(tmp.scan).ExclusiveSum(L, x);
  uint16_t before = tid ? last_id[tid - 1] : (uint16_t)parts;
#pragma unroll
  for (int k = 0; k < kPartPer; ++k) {
    if (key[k] < parts && (key[k] != before || (tid == 0 && k == 0))) {  // its run's first: one per part
      base_rank[key[k]] -= kPartPer * tid + k;
      base_byte[key[k]] -= x[k];
    }
    before = key[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPartPer; ++k) {
    const uint32_t p = key[k];
    if (p >= parts) continue;
    const uint64_t rank = base_rank[p] + (kPartPer * tid + k);
    const uint64_t d = base_byte[p] + x[k];
    dst[val[k]] = d;
    out_off[rank] = d;
    if (index) index[rank] = r0 + val[k];
    if (L[k] >= (uint64_t)kPartLong) atomicOr(&is_long[val[k] >> 5], 1u << (val[k] & 31u));
  }
  __syncthreads();
  // in the tile's order, so that the lanes of a wave read neighbouring blobs of the stream
  const uint32_t g = tid / kPartLanes, lane = tid % kPartLanes;
  for (uint32_t j = g; j < nr; j += kPartThreads / kPartLanes) {
    const uint64_t d = dst[j], B = span[j + 1] - span[j];
    if (d == kLeftOut || B >= (uint64_t)kPartLong) continue;
    move_blob(blobs + span[j], out + d, B, lane, kPartLanes);
  }
  for (uint32_t w = 0; w < kPartBlobs / 32; ++w) {
    for (uint32_t bits = is_long[w]; bits; bits &= bits - 1) {
      const uint32_t j = 32 * w + (uint32_t)__ffs((int)bits) - 1;
      move_blob(blobs + span[j], out + dst[j], span[j + 1] - span[j], tid, kPartThreads);
    }
  }
}

// The call's temporaries (k2h_scratch.h): the two histograms, the bounds, a part id per blob and
// the scan's own storage.  The copy kernel still reads the buffer after the call has returned.
PerDevice<> g_part;

struct PartCols {
  uint64_t *hc, *hb, *bounds;
  uint16_t* ids;
  void* tmp;
  size_t total;
};

}  // namespace

// Returns K2H_AMD_* codes (the HIP error, if any, in *herr); synchronises the stream once.
// n >= 1; the rule has been judged by the caller.
int launch_ralledata_partition(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                               const k2h_amd_part_rule& rule, const uint32_t* part_ids, const uint8_t* consider,
                               void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* index, uint32_t* part_out,
                               uint64_t* part_first, uint64_t* part_byte, hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  const uint32_t parts = rule.parts;
  const uint64_t nt = (n + kPartBlobs - 1) / kPartBlobs;
  if (nt > 0x7FFFFFFFull / parts) return K2H_AMD_EINVAL;
  const uint64_t m = nt * parts;  // histogram entries; entry m of a scan is the total
  FirstError tr;
  DeviceScratch* const sc = g_part.current(tr);
  size_t tmp_bytes = 0;
  tr(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, m + 1, stream));
  if (!tr.ok()) {
    *herr = tr.e;
    return K2H_AMD_EHIP;
  }
  auto layout = [&](void* base) {
    Carver c(base);
    PartCols k;
    k.hc = c.take<uint64_t>(m + 1);
    k.hb = c.take<uint64_t>(m + 1);
    k.bounds = c.take<uint64_t>(2 * (parts + 1));
    k.ids = c.take<uint16_t>(n);
    k.tmp = c.bytes(tmp_bytes);
    k.total = c.total();
    return k;
  };
  std::lock_guard<std::mutex> lk(sc->mu);
  if (const int rc = sc->reserve(layout(nullptr).total, stream, herr)) return rc;
  const PartCols k = layout(sc->p);
  // entry m of the histograms is 0, so entry m of the exclusive scans is the total
  tr(hipMemsetAsync(k.hc + m, 0, 8, stream));
  tr(hipMemsetAsync(k.hb + m, 0, 8, stream));
  if (tr.ok()) {
    ralledata_part_count_kernel<<<(unsigned)nt, kPartThreads, 0, stream>>>(
        (const uint8_t*)blobs, size, blob_off, n, rule, part_ids, consider, nt, k.ids, part_out, k.hc, k.hb);
    tr(hipGetLastError());
  }
  if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(k.tmp, tmp_bytes, k.hc, k.hc, m + 1, stream));
  if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(k.tmp, tmp_bytes, k.hb, k.hb, m + 1, stream));
  if (tr.ok()) {
    ralledata_part_bounds_kernel<<<1, kPartThreads, 0, stream>>>(k.hc, k.hb, nt, parts, k.bounds);
    tr(hipGetLastError());
  }
  uint64_t host[2 * (K2H_AMD_PART_MAX + 1)];
  if (tr.ok()) tr(hipMemcpyAsync(host, k.bounds, 2 * (parts + 1) * 8, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(hipStreamSynchronize(stream));
  int rc = K2H_AMD_OK;
  if (tr.ok()) {
    for (uint32_t p = 0; p <= parts; ++p) {
      part_first[p] = host[p];
      part_byte[p] = host[parts + 1 + p];
    }
    if (out && part_byte[parts] > out_cap) {
      rc = K2H_AMD_EINVAL;
    } else if (out) {
      int id_bits = 1;  // the sort's keys are 0 .. parts
      while ((1u << id_bits) <= parts) ++id_bits;
      ralledata_part_copy_kernel<<<(unsigned)nt, kPartThreads, 0, stream>>>(
          (const uint8_t*)blobs, blob_off, n, k.ids, k.hc, k.hb, nt, parts, id_bits, (uint8_t*)out, out_off, index);
      tr(hipGetLastError());
      if (tr.ok()) tr(sc->mark_done(stream));
    }
  }
  *herr = tr.e;
  return !tr.ok() ? K2H_AMD_EHIP : rc;
}

}  // namespace k2h
