// k2hash_amd -- RALLEDATA consumer side: check, route and compact a blob stream in device
// memory (include/k2hash_amd.h section 4, second part).
//
// K2HShm::SetElementByBinArray (lib/k2hshmdirect.cc:343-478) TRUSTS the hash / subhash
// fields of the blob it is given, so a receiver of a blob stream (replication or merge via
// k2h_get_elements_by_hash, another producer, a table built with the other seed) has to
// re-derive them before it feeds k2h_set_element_by_binary.  ralledata_check_kernel does that
// for a whole stream -- header sanity in the order SetElementByBinArray tests it (:351, :355,
// :361-364), the key re-hashed, and optionally the circular hash-range test of
// K2HShm::GetElementListToBinary (lib/k2hshmdirect.cc:118-131, old range :119, :165-176) --
// and the select kernels pack the blobs a caller keeps back to back.
//
// Blob i = blobs[off[i], off[i+1]), the layout k2h_amd_build_ralledata writes
// (k2h_ralledata.hip).  Every address is byte-aligned.  No byte outside [0, size) is read
// except within the aligned 16 bytes that hold a valid byte (the staged form's hull loads,
// as the producer's), and nothing of a blob whose span is bad.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <mutex>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_ralle_header.h"
#include "k2h_scratch.h"

namespace k2h {
namespace {

// Workgroup barrier over LDS only (the block's waves share only LDS here; __syncthreads()
// also waits for every outstanding vector-memory operation).
__device__ __forceinline__ void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

constexpr int kCheckBlobs = 64;     // blobs per 256-thread block (the producer's tile)
constexpr int kCheckStage = 18432;  // staged hull bytes (BASELINE-like: ~15.6 KB, sd ~0.6 KB; 8 blocks per CU)

struct CheckOut {
  uint8_t* status;
  uint8_t* route;  // null: no range given
  uint64_t* h1;    // may be null
  uint64_t* h2;    // may be null
};

// lib/k2hshmdirect.cc:122-131 (and :165-176 over the old range), restated verbatim: m is
// the hash modulo the range's max, lo the range's start, end its (already reduced) end.
__device__ __forceinline__ bool in_hash_range(uint64_t m, uint64_t lo, uint64_t end) {
  bool in = true;
  if (lo <= end) {
    if (m < lo || end < m) in = false;
  } else {
    if (end < m && m < lo) in = false;
  }
  return in;
}

// st: the header's status; r1 / r2: the recomputed hashes when st is OK.
__device__ __forceinline__ void emit(const CheckOut& o, const RalleRoute& rp, uint64_t i, uint32_t st, uint64_t hash,
                                     uint64_t sub, uint64_t r1, uint64_t r2) {
  if (st == K2H_AMD_RALLE_OK) {
    if (hash != r1) st = K2H_AMD_RALLE_BAD_HASH;
    else if (sub != r2) st = K2H_AMD_RALLE_BAD_SUBHASH;
  } else {
    r1 = r2 = 0;
  }
  o.status[i] = (uint8_t)st;
  if (o.route) {
    uint32_t r = 0;
    if (st == K2H_AMD_RALLE_OK) {
      r = in_hash_range(hash % rp.t_max, rp.t, rp.t_end) ? 1u : 0u;
      if (rp.old_on && in_hash_range(hash % rp.o_max, rp.o, rp.o_end)) r |= 2u;
    }
    o.route[i] = (uint8_t)r;
  }
  if (o.h1) o.h1[i] = r1;
  if (o.h2) o.h2[i] = r2;
}

// A block takes kCheckBlobs consecutive blobs.  Staged form: the tile's blobs are one
// contiguous span of the stream; its aligned hull is read once, all lanes on consecutive
// aligned 16-byte pieces, into LDS, and wave 0 takes headers and keys from there, one lane per
// blob (end-aligned chunks, the second hash from the snapshot before the last byte).  A tile
// that holds a blob with a bad span, or whose hull exceeds the stage (large values), takes
// the direct form: one lane per blob, the header and the key alone read from HBM.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void ralledata_check_kernel(
    const uint8_t* __restrict__ blobs, uint64_t size, const uint64_t* __restrict__ off, uint64_t n, CheckOut out,
    RalleRoute rp, SpadTable spad_tab) {
  typedef uint32_t u32x4_al __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) uint8_t img[kCheckStage];
  __shared__ uint64_t spad[16];
  static_assert(kCheckStage % 16 == 0 && kCheckStage + 8 * 16 <= 20 * 1024, "8 blocks per CU");
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint64_t r0 = (uint64_t)blockIdx.x * kCheckBlobs;
  const uint32_t nr = (uint32_t)(n - r0 < (uint64_t)kCheckBlobs ? n - r0 : (uint64_t)kCheckBlobs);
  // every wave reads the tile's offsets (wave 0 keeps them: lane = blob) and judges the spans
  // itself, so the form is known block-wide without a barrier
  uint64_t b = 0, e = 0;
  bool span_ok = true;
  if (lane < nr) {
    b = off[r0 + lane];
    e = off[r0 + lane + 1];
    span_ok = e >= b && e <= size && e - b >= (uint64_t)kHdr;
  }
  const uint64_t first = off[r0], last = off[r0 + nr];
  const uint64_t a0 = (uint64_t)(uintptr_t)(blobs + first);
  const uint64_t lo = a0 & ~15ull, hi = ((uint64_t)(uintptr_t)(blobs + last) + 15) & ~15ull;
  // all spans good: first <= ... <= last <= size, so the hull is the tile's blobs
  const bool staged = __all(span_ok) && hi - lo <= (uint64_t)kCheckStage;
  if (tid < 16) spad[tid] = spad_tab.v[tid];
  if (!staged) {  // block-uniform
    __syncthreads();
    if (tid >= nr) return;
    uint32_t st = K2H_AMD_RALLE_BAD_SPAN;
    uint64_t f[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, r1 = 0, r2 = 0;
    if (span_ok) {
      const uint8_t* p = blobs + b;
      load_fields(p, f);
      st = classify(f, e - b);
      if (st == K2H_AMD_RALLE_OK) {
        const uint64_t kl = f[2], k = (kl + 15) >> 4;
        end_aligned_walk_ptr<true, true>(k, (uint32_t)(16 * k - kl), p + f[6] + kl - 16 * k, blobs, spad, r1, r2);
        if (kl == 1) r2 = r1;  // lib/k2hashfunc.cc:83
      }
    }
    emit(out, rp, r0 + tid, st, f[0], f[1], r1, r2);
    return;
  }
  // the hull: piece q -> img[16 q]; global (not flat) non-temporal loads, as the producer's
  constexpr int PPT = (kCheckStage / 16 + 255) / 256;
  const uint32_t np = (uint32_t)((hi - lo) >> 4);
  u32x4_al v[PPT];
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    const uint32_t q = tid + 256u * u;
    if (q < np)
      v[u] = __builtin_nontemporal_load(
          reinterpret_cast<const __attribute__((address_space(1))) u32x4_al*>((uintptr_t)(lo + 16ull * q)));
  }
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    const uint32_t q = tid + 256u * u;
    if (q < np) *reinterpret_cast<u32x4_al*>(img + 16 * q) = v[u];
  }
  lds_sync();
  if (tid >= nr) return;
  // wave 0, lane = blob: everything block-relative fits 32 bits
  const uint32_t at = (uint32_t)(a0 & 15u) + (uint32_t)(b - first);
  uint64_t f[10], r1 = 0, r2 = 0;
  load_fields(img + at, f);
  const uint32_t st = classify(f, e - b);
  if (st == K2H_AMD_RALLE_OK) {
    // (the key lies at or above byte 80 of its blob: chunk 0 never starts below the image)
    const uint32_t kl = (uint32_t)f[2], k = (kl + 15) >> 4, p = 16 * k - kl;
    const uint8_t* cp = img + at + (uint32_t)f[6] + kl - 16 * k;
    end_aligned_walk<true, false>(
        k, p, mask_lead(ld16(cp), p), spad, [=](uint32_t q) { return ld16(cp + 16 * q); }, r1, r2);
    if (kl == 1) r2 = r1;  // lib/k2hashfunc.cc:83
  }
  emit(out, rp, r0 + tid, st, f[0], f[1], r1, r2);
}

// ------------------------------------------------------------------------------ select
constexpr int kSelBlobs = 256;         // blobs per 256-thread block, one per thread
constexpr int kSelTabPieces = 4096;    // a tile whose kept bytes span up to this many 16-byte pieces looks
                                       // its pieces' blobs up in a table (64 KiB: BASELINE-like tiles do)
static_assert(kSelBlobs <= 256, "a blob's index in its tile is a table byte");

// Blob i as select sees it: kept when keep[i] != 0 and its span is valid (non-decreasing,
// ends at or before size); b = its start, the return value its length.
__device__ __forceinline__ uint64_t kept_span(const uint8_t* keep, const uint64_t* off, uint64_t size, uint64_t n,
                                              uint64_t i, uint64_t& b, uint32_t& kept) {
  b = 0;
  kept = 0;
  if (i >= n || !keep[i]) return 0;
  const uint64_t s = off[i], e = off[i + 1];
  if (e < s || e > size) return 0;
  b = s;
  kept = 1;
  return e - s;
}

// per tile: the kept blobs' bytes and their count
__global__ __launch_bounds__(256) void ralledata_select_sum_kernel(const uint64_t* __restrict__ off, uint64_t size,
                                                                   uint64_t n, const uint8_t* __restrict__ keep,
                                                                   uint64_t* __restrict__ tile_bytes,
                                                                   uint64_t* __restrict__ tile_count) {
  typedef hipcub::BlockReduce<uint64_t, kSelBlobs> Reduce;
  __shared__ typename Reduce::TempStorage ta, tb;
  uint64_t b;
  uint32_t kept;
  const uint64_t len = kept_span(keep, off, size, n, (uint64_t)blockIdx.x * kSelBlobs + threadIdx.x, b, kept);
  const uint64_t bytes = Reduce(ta).Sum(len), count = Reduce(tb).Sum((uint64_t)kept);
  if (threadIdx.x == 0) {
    tile_bytes[blockIdx.x] = bytes;
    tile_count[blockIdx.x] = count;
  }
}

// The tile's kept blobs land back to back at out + tile_bytes[tile] (the scanned sums).  The
// block writes that destination span as 16-byte pieces aligned in `out`, consecutive lanes
// on consecutive pieces: a piece whose 16 source bytes are contiguous in the stream (inside
// one blob, or across kept neighbours, which touch in the source as they do in the
// destination) is one unaligned load and one aligned store; a piece across a dropped blob is
// gathered byte by byte into registers and stored once; the two pieces the span shares with
// the neighbouring tiles are stored byte by byte, this tile's bytes only.  The blob that
// holds a piece's first byte comes from a byte table each kept blob fills for its own pieces
// (one LDS read per piece); a tile whose span outgrows the table (large values) searches the
// tile's prefix sums instead (eight dependent reads).
__global__ __launch_bounds__(256) void ralledata_select_copy_kernel(
    const uint8_t* __restrict__ blobs, uint64_t size, const uint64_t* __restrict__ off, uint64_t n,
    const uint8_t* __restrict__ keep, const uint64_t* __restrict__ tile_bytes, const uint64_t* __restrict__ tile_count,
    uint64_t ntiles, uint8_t* __restrict__ out, uint64_t* __restrict__ out_off, uint64_t* __restrict__ index) {
  typedef uint32_t u32x4_al __attribute__((ext_vector_type(4)));
  typedef hipcub::BlockScan<uint64_t, kSelBlobs> Scan;
  __shared__ typename Scan::TempStorage ta, tb;
  __shared__ uint64_t pre[kSelBlobs + 1];  // kept bytes of the tile's blobs before blob j
  __shared__ uint64_t delta[kSelBlobs];    // blob j: span byte x sits at blobs[x + delta[j]]
  __shared__ uint8_t tab[kSelTabPieces];   // the blob holding the first of this tile's bytes in piece p
  const uint32_t tid = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * kSelBlobs + tid;
  uint64_t b, x, B, rank, cnt;
  uint32_t kept;
  const uint64_t len = kept_span(keep, off, size, n, i, b, kept);
  Scan(ta).ExclusiveSum(len, x, B);
  Scan(tb).ExclusiveSum((uint64_t)kept, rank, cnt);
  const uint64_t D0 = tile_bytes[blockIdx.x], C0 = tile_count[blockIdx.x];
  pre[tid] = x;
  delta[tid] = b - x;
  if (tid == 0) pre[kSelBlobs] = B;
  if (kept) {
    out_off[C0 + rank] = D0 + x;
    if (index) index[C0 + rank] = i;
  }
  if (blockIdx.x == 0 && tid == 0) out_off[tile_count[ntiles]] = tile_bytes[ntiles];
  uint8_t* const dst = out + D0;
  const uint32_t a = (uint32_t)((uintptr_t)dst & 15u);
  const uint64_t npieces = (a + B + 15) >> 4;
  const bool tabled = npieces <= (uint64_t)kSelTabPieces;  // block-uniform
  if (tabled && len) {
    // piece p's first byte of this tile is span byte max(16 p - a, 0): blob tid holds it for
    // p from ceil((x + a) / 16) (from 0 when the span starts with this blob) to its last byte's piece
    const uint32_t last = (uint32_t)((x + len - 1 + a) >> 4);
    for (uint32_t p = x ? (uint32_t)((x + a + 15) >> 4) : 0u; p <= last; ++p) tab[p] = (uint8_t)tid;
  }
  __syncthreads();
  if (!B) return;
  for (uint64_t p = tid; p < npieces; p += kSelBlobs) {
    // the piece holds span bytes [x0, x0 + 16), this tile's part of it [xl, xh)
    const int64_t x0 = (int64_t)(16 * p) - (int64_t)a;
    const uint64_t xl = x0 < 0 ? 0 : (uint64_t)x0, xh = (uint64_t)(x0 + 16) < B ? (uint64_t)(x0 + 16) : B;
    uint32_t j = 0;  // the blob holding byte xl: the last j with pre[j] <= xl
    if (tabled) {
      j = tab[p];
    } else {
#pragma unroll
      for (uint32_t step = kSelBlobs / 2; step; step >>= 1)
        if (pre[j + step] <= xl) j += step;
    }
    const bool whole = xh - xl == 16;
    bool contiguous = whole;
    if (whole && pre[j + 1] < xh) {  // past blob j: every blob up to the one holding xh - 1
      for (uint32_t m = j; pre[m + 1] < xh;) {
        ++m;
        if (pre[m + 1] > pre[m] && delta[m] != delta[j]) contiguous = false;
      }
    }
    if (contiguous) {
      const u32x4_ua w = *reinterpret_cast<const u32x4_ua*>(blobs + xl + delta[j]);
      *reinterpret_cast<u32x4_al*>(dst + x0) = u32x4_al{w.x, w.y, w.z, w.w};
      continue;
    }
    // Eight places at a time: first every place's source address (an LDS walk), then eight byte
    // loads with nothing between them, all in flight before the first is used (a loop over
    // the bytes waited for each load in turn).  A place outside [xl, xh) reads the nearest
    // byte inside it; those bytes are never stored.
    uint32_t w[4];
    uint32_t m = j;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint8_t* src[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int64_t y = x0 + 8 * h + k;
        const uint64_t yc = y < (int64_t)xl ? xl : y >= (int64_t)xh ? xh - 1 : (uint64_t)y;
        while (pre[m + 1] <= yc) ++m;
        src[k] = blobs + yc + delta[m];
      }
      uint32_t bt[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) bt[k] = *src[k];
      w[2 * h] = bt[0] | bt[1] << 8 | bt[2] << 16 | bt[3] << 24;
      w[2 * h + 1] = bt[4] | bt[5] << 8 | bt[6] << 16 | bt[7] << 24;
    }
    if (whole) {
      *reinterpret_cast<u32x4_al*>(dst + x0) = u32x4_al{w[0], w[1], w[2], w[3]};
    } else {
      for (uint64_t y = xl; y < xh; ++y) {
        const uint32_t k = (uint32_t)((int64_t)y - x0);
        dst[y] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
      }
    }
  }
}

// The select's temporaries (k2h_scratch.h): per tile of kSelBlobs blobs its kept bytes and
// count, their scans, and the scan's own storage -- 32 bytes per 256 blobs.  The copy kernel
// still reads the buffer after the call has returned.
PerDevice<> g_sel;

struct SelCols {
  uint64_t *tb, *tc, *sb, *scn;
  void* tmp;
  size_t total;
};

}  // namespace

hipError_t launch_ralledata_check(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                                  uint64_t seed, const RalleRoute& route, uint8_t* status, uint8_t* route_out,
                                  uint64_t* h1, uint64_t* h2, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint64_t grid = (n + kCheckBlobs - 1) / kCheckBlobs;
  if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
  ralledata_check_kernel<<<(unsigned)grid, 256, 0, stream>>>((const uint8_t*)blobs, size, blob_off, n,
                                                            CheckOut{status, route_out, h1, h2}, route,
                                                            make_spad(seed));
  return hipGetLastError();
}

// Returns K2H_AMD_* codes (the HIP error, if any, in *herr); synchronises the stream once.
int launch_ralledata_select(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                            const uint8_t* keep, void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* index,
                            uint64_t* kept, uint64_t* kept_bytes, hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  *kept = *kept_bytes = 0;
  if (n == 0) return K2H_AMD_OK;
  const uint64_t nt = (n + kSelBlobs - 1) / kSelBlobs;
  if (nt > 0x7FFFFFFFull) return K2H_AMD_EINVAL;
  FirstError tr;
  DeviceScratch* const sc = g_sel.current(tr);
  size_t tmp_bytes = 0;
  tr(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, nt + 1, stream));
  if (!tr.ok()) {
    *herr = tr.e;
    return K2H_AMD_EHIP;
  }
  auto layout = [&](void* base) {
    Carver c(base);
    SelCols k;
    k.tb = c.take<uint64_t>(nt + 1);
    k.tc = c.take<uint64_t>(nt + 1);
    k.sb = c.take<uint64_t>(nt + 1);
    k.scn = c.take<uint64_t>(nt + 1);
    k.tmp = c.bytes(tmp_bytes);
    k.total = c.total();
    return k;
  };
  std::lock_guard<std::mutex> lk(sc->mu);
  if (const int rc = sc->reserve(layout(nullptr).total, stream, herr)) return rc;
  const SelCols k = layout(sc->p);
  // entry nt of the sums is 0, so entry nt of the exclusive scans is the total
  tr(hipMemsetAsync(k.tb + nt, 0, 8, stream));
  tr(hipMemsetAsync(k.tc + nt, 0, 8, stream));
  if (tr.ok()) {
    ralledata_select_sum_kernel<<<(unsigned)nt, kSelBlobs, 0, stream>>>(blob_off, size, n, keep, k.tb, k.tc);
    tr(hipGetLastError());
  }
  if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(k.tmp, tmp_bytes, k.tb, k.sb, nt + 1, stream));
  if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(k.tmp, tmp_bytes, k.tc, k.scn, nt + 1, stream));
  uint64_t tot[2] = {0, 0};
  if (tr.ok()) tr(hipMemcpyAsync(&tot[0], k.sb + nt, 8, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(hipMemcpyAsync(&tot[1], k.scn + nt, 8, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(hipStreamSynchronize(stream));
  int rc = K2H_AMD_OK;
  if (tr.ok()) {
    *kept_bytes = tot[0];
    *kept = tot[1];
    if (out && tot[0] > out_cap) {
      rc = K2H_AMD_EINVAL;
    } else if (out) {
      ralledata_select_copy_kernel<<<(unsigned)nt, kSelBlobs, 0, stream>>>((const uint8_t*)blobs, size, blob_off, n,
                                                                          keep, k.sb, k.scn, nt, (uint8_t*)out, out_off,
                                                                          index);
      tr(hipGetLastError());
      if (tr.ok()) tr(sc->mark_done(stream));
    }
  }
  *herr = tr.e;
  return !tr.ok() ? K2H_AMD_EHIP : rc;
}

}  // namespace k2h
