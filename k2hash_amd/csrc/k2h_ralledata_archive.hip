// k2hash_amd -- a RALLEDATA blob stream written as a k2hash archive (include/k2hash_amd.h
// section 4d): one SCOM_SET_ALL record per blob, the bytes K2HCommandArchive::SetAll produces
// (lib/k2hcommand.cc:69-135, scom_init at lib/k2hcommand.h:99-113) and K2HArchive::Load replays.
//
// Record sizes differ per blob and a blob may yield no record, so the record offsets are a
// scan, as in k2h_ralledata_recs.hip: a sizing kernel judges each blob (keep byte, span, the
// header tests of k2h_ralle_header.h -- the participants of _dedup) and writes its record size
// (104 + its four lengths, or 0) into rec_off, an exclusive sum turns the sizes into offsets in
// place, and the build kernel places the records by them.  The build kernel judges nothing
// again: a blob takes part exactly when its record has bytes.
//
// Build kernel = the scheme of ralledata_recs_kernel: a 256-thread block takes kArcBlobs
// consecutive blobs, whose records are one contiguous output span.  The blobs of a stream lie
// back to back, so the block stages ONE run of the stream -- the aligned 16-byte hull from its
// first participant's first byte to its last participant's last, headers and payload alike,
// less the pieces that belong wholly to blobs that take no part -- into LDS, reads the blobs'
// headers THERE (the build reads every stream byte once, and the block's choice of form needs
// only the two offset arrays), builds the 104-byte record headers beside them, and writes the
// span as aligned 16-byte non-temporal pieces from a five-segment table per record:
//   header, key, value, subkeys, attrs
// 32 blobs, not the 64 records of that kernel: the blobs' own 80-byte headers ride along in the
// run and the record header is 24 bytes longer, so at 8 blocks per CU the pool holds 32 blobs of
// up to 447 bytes on average where it would hold 64 of 143.
//
// Staged or direct (block-uniform).  The block is STAGED when
//   - its participants lie in stream order without overlap (each starts at or after the end of
//     the one before it) and the first one's start .. the last one's end is at most kArcHullMax:
//     judged from blob_off alone, before anything of the stream is read; and
//   - inside every participant the segments of length > 0 lie in record order without overlap:
//     judged from the staged headers.
// Every other block is DIRECT: 8 lanes per blob straight from HBM (one large value, permuted or
// overlapping segments, offsets that step backwards).  Both forms write the same bytes.
//
// Memory.  A blob's header is read only when its span is good and its keep byte set, its
// segments are addressed only when its header passes classify(), and every segment of a
// participant lies inside its blob, so inside [0, size).  The staged form loads the aligned
// 16-byte pieces that hold a byte of a participant, and no other piece of the run; the direct
// form and the edges of a span touch exact bytes only.  The hash and subhash fields are not
// loaded by the sizing kernel or the direct form.  All absolute offsets are 64-bit; only
// block-relative ones are 32-bit.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_layout.h"
#include "k2h_ralle_header.h"
#include "k2h_ralle_pieces.h"

namespace k2h {
namespace {

constexpr int kScom = K2H_AMD_SCOM_HEADER;  // sizeof(SCOM), packed
constexpr int kArcBlobs = 32;               // blobs per 256-thread block
constexpr int kArcPool = 14336;             // staged stream bytes (the aligned hull)
constexpr int kArcHullMax = kArcPool - 32;  // first start .. last end; + 2 x 15 bytes of alignment fits the pool
constexpr int kArcHdr = 16;                 // LDS offset of the record headers (a window may begin 15 bytes below)
constexpr int kArcSlot = 112;               // LDS bytes per record header: 104, kept 16-byte aligned
constexpr int kArcImg = kArcHdr + kArcSlot * kArcBlobs + kArcPool + 16;
constexpr int kArcSpanMax = kScom * kArcBlobs + kArcHullMax;  // headers, stream bytes
constexpr int kArcPieces = kArcSpanMax / 16 + 2;

// szCommand of a SET_ALL record: "\nK2H_SET_ALL" and four 0x00 bytes (lib/k2hcommand.h:36-45).
constexpr uint64_t kCmd0 = 0x5445535F48324B0Aull;  // "\nK2H_SET"
constexpr uint64_t kCmd1 = 0x000000004C4C415Full;  // "_ALL\0\0\0\0"

typedef uint32_t u32x2_ua __attribute__((ext_vector_type(2), aligned(1)));

// The thirteen 64-bit words of the record header, two at a time: chunk c = words 2c, 2c + 1
// (chunk 6 has one).  szCommand; type 0; the four lengths and exdata_length 0; key_pos 104 and
// the running positions; exdata_pos 104 (scom_init's value, which Put leaves for SET_ALL).
template <class T>
__device__ __forceinline__ void scom_chunk(int c, T k, T v, T s, T a, T& w0, T& w1) {
  switch (c) {
    case 1: w0 = 0, w1 = k; break;
    case 2: w0 = v, w1 = s; break;
    case 3: w0 = a, w1 = 0; break;
    case 4: w0 = kScom, w1 = kScom + k; break;
    case 5: w0 = kScom + k + v, w1 = kScom + k + v + s; break;
    default: w0 = kScom, w1 = 0; break;  // 6
  }
}

// The header's lengths and positions (fields 2 .. 9); the hash fields stay unread, as 0.
__device__ __forceinline__ void load_lens_pos(const uint8_t* p, uint64_t (&f)[10]) {
  f[0] = f[1] = 0;
#pragma unroll
  for (int c = 1; c < 5; ++c) {
    const uint4 v = ld16(p + 16 * c);
    f[2 * c] = pack2(v.x, v.y);
    f[2 * c + 1] = pack2(v.z, v.w);
  }
}

// rec_off[i] = the record size of blob i, 0 for a blob that yields none; entry n is 0 (entry n
// of the exclusive sum is the total).  Counts the records into word 0 of the counter lines
// (k2h_layout.h).
__global__ __launch_bounds__(256) void scom_archive_size_kernel(const uint8_t* __restrict__ blobs, uint64_t size,
                                                                const uint64_t* __restrict__ off, uint64_t n,
                                                                const uint8_t* __restrict__ keep,
                                                                uint64_t* __restrict__ sizes,
                                                                unsigned long long* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint64_t v = 0;
  if (i < n && (!keep || keep[i])) {
    const uint64_t b = off[i], e = off[i + 1];
    if (e >= b && e <= size && e - b >= (uint64_t)kHdr) {
      uint64_t f[10];
      load_lens_pos(blobs + b, f);
      if (classify(f, e - b) == K2H_AMD_RALLE_OK) v = kScom + f[2] + f[3] + f[4] + f[5];
    }
  }
  if (i <= n) sizes[i] = v;
  // one atomic per wave, neighbouring waves on different lines (as the dedup resolve kernel)
  const unsigned long long m = __ballot(v != 0);
  if ((threadIdx.x & 63u) == 0 && m) {
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    atomicAdd(counters + 8 * (wave % kCounterLines), (unsigned long long)__popcll(m));
  }
}

// Direct form: one blob by a group of G lanes, straight to HBM.
template <int G>
__device__ __forceinline__ void direct_record(const uint8_t* __restrict__ blobs, const uint64_t* __restrict__ blob_off,
                                              uint8_t* __restrict__ out, const uint64_t* __restrict__ rec_off,
                                              uint64_t i, uint32_t q) {
  const uint64_t at = rec_off[i];
  if (rec_off[i + 1] == at) return;  // yields no record: nothing of the blob is read
  const uint8_t* b = blobs + blob_off[i];
  uint64_t f[10];
  load_lens_pos(b, f);
  uint8_t* r = out + at;
  if (q < 7) {
    uint64_t w0 = kCmd0, w1 = kCmd1;
    if (q) scom_chunk<uint64_t>((int)q, f[2], f[3], f[4], f[5], w0, w1);
    if (q < 6)
      *reinterpret_cast<u32x4_ua*>(r + 16 * q) = u32x4_ua{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
    else
      *reinterpret_cast<u32x2_ua*>(r + 96) = u32x2_ua{(uint32_t)w0, (uint32_t)(w0 >> 32)};
  }
  uint64_t to = kScom;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const uint64_t len = f[2 + s];
    if (len) group_copy<G>(r + to, b + f[6 + s], len, q);  // the pos of a length-0 segment is ignored
    to += len;
  }
}

__device__ __forceinline__ uint64_t lane64(uint64_t v, uint32_t lane) {
  return pack2((uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane),
               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane));
}

// 8 blocks per CU: under 20 KiB of LDS, at most 64 VGPRs.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void scom_archive_build_kernel(
    const uint8_t* __restrict__ blobs, const uint64_t* __restrict__ blob_off, uint64_t n, uint8_t* __restrict__ out,
    const uint64_t* __restrict__ rec_off) {
  constexpr int NS = 5, NF = 4;
  constexpr int R = kArcBlobs, NSEG = NS * R;
  typedef uint32_t u32x4_al __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) uint8_t img[kArcImg];
  __shared__ uint32_t seg[NSEG + 1];       // segment g: seg_pack(adj, end)
  __shared__ uint8_t tab[kArcPieces + 1];  // the segment holding piece p's first byte (+ a dump slot)
  __shared__ u32x4_al qmask[17];
  __shared__ uint32_t unordered;  // a participant's segments are not in record order
  static_assert(kArcImg + 4 * (NSEG + 1) + kArcPieces + 1 + 16 * 17 + 4 <= 20 * 1024, "8 blocks per CU");
  static_assert(kArcSpanMax < 32768 && kArcSpanMax % 16 == 0, "seg_pack: adj and end in 16 bits");
  static_assert(NSEG < 256, "tab: a segment index in a byte");
  static_assert(8 * R == 256, "direct form: 8 lanes per blob, one pass");
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint64_t r0 = (uint64_t)blockIdx.x * R;
  const uint32_t nr = (uint32_t)(n - r0 < (uint64_t)R ? n - r0 : (uint64_t)R);
  const uint64_t o_first = rec_off[r0];
  const uint64_t span = rec_off[r0 + nr] - o_first;
  if (span == 0) return;  // no blob of the block yields a record

  // Every wave reads the block's offsets (lane l: blob r0 + l) and derives the same block-uniform
  // facts from them with wave operations: no barrier, and no byte of the stream, before the
  // staged loads.
  uint64_t mine = 0, b = 0, e = 0;
  bool keep = false;
  if (lane < nr) {
    mine = rec_off[r0 + lane];
    keep = rec_off[r0 + lane + 1] != mine;
    b = blob_off[r0 + lane];
    e = blob_off[r0 + lane + 1];
  }
  // the last end among the participants before this one (an inclusive max scan, shifted by one)
  uint64_t inc = keep ? e : 0;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t t = __shfl_up(inc, d);
    if (lane >= d && t > inc) inc = t;
  }
  uint64_t prev = __shfl_up(inc, 1u);
  if (lane == 0) prev = 0;
  const uint64_t kept = __ballot(keep);
  const bool ordered = __ballot(keep && b < prev) == 0;
  const uint64_t hull_b = lane64(b, (uint32_t)__ffsll((unsigned long long)kept) - 1u);
  const uint64_t hull_e = lane64(inc, 63u);
  const uint32_t nk = (uint32_t)__popcll(kept), rank = (uint32_t)__popcll(kept & ((1ull << lane) - 1ull));

  if (!ordered || hull_e - hull_b > (uint64_t)kArcHullMax) {  // block-uniform: the direct form
    if (tid / 8 < nr) direct_record<8>(blobs, blob_off, out, rec_off, r0 + tid / 8, tid % 8);
    return;
  }

  // the staged run: stream bytes [hull_b, hull_e), its aligned hull, stream byte f at img[area + f - hull_b]
  const uint64_t a_b = (uint64_t)(uintptr_t)(blobs + hull_b), a_lo = a_b & ~15ull;
  const uint32_t hull_n = (uint32_t)((((uint64_t)(uintptr_t)(blobs + hull_e) + 15) & ~15ull) - a_lo) >> 4;
  const int32_t area = kArcHdr + kArcSlot * R + (int32_t)(a_b - a_lo);
  // 1a. the staged pieces: up to PPT aligned non-temporal loads per thread.  Between the first
  // and the last participant may lie blobs that take no part (a keep mask, a refused header):
  // nothing of those is read beyond the 16-byte pieces they share with a participant.  The
  // block-uniform test for such a hole is free; only a block that has one looks each piece up
  // among the participants' spans (every wave holds them, lane l: blob r0 + l).
  constexpr int PPT = (kArcPool / 16 + 255) / 256;
  const uint32_t first = (uint32_t)__ffsll((unsigned long long)kept) - 1u;
  const bool holes = ((kept >> first) & ((kept >> first) + 1)) != 0;
  bool need[PPT];
#pragma unroll
  for (int u = 0; u < PPT; ++u) need[u] = !holes;
  if (holes) {
    const uint64_t a_blobs = (uint64_t)(uintptr_t)blobs;
    for (uint32_t j = first; j < nr; ++j) {
      if (!((kept >> j) & 1)) continue;
      const uint64_t pb = a_blobs + lane64(b, j), pe = a_blobs + lane64(e, j);
#pragma unroll
      for (int u = 0; u < PPT; ++u) {
        const uint64_t pa = a_lo + 16ull * (tid + 256 * u);
        need[u] = need[u] || (pa < pe && pa + 16 > pb);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    const uint32_t q = tid + 256 * u;
    if (q < hull_n && need[u]) {
      // a global (not flat) load, so that the LDS reads after the barrier do not wait for it
      const u32x4_al v = __builtin_nontemporal_load(
          reinterpret_cast<const __attribute__((address_space(1))) u32x4_al*>((uintptr_t)(a_lo + 16ull * q)));
      *reinterpret_cast<u32x4_al*>(img + kArcHdr + kArcSlot * R + 16 * q) = v;
    }
  }
  const uint64_t a_out = (uint64_t)(uintptr_t)(out + o_first);
  const int32_t d0 = (int32_t)(a_out & 15u);
  if (tid >= 64 && tid < 64 + 17) {  // qmask[l] = bytes [l, 16) of a piece
    const int l = (int)tid - 64;
    u32x4_al m;
    m.x = (uint32_t)(~0ull << (8 * min(max(l - 0, 0), 4)));
    m.y = (uint32_t)(~0ull << (8 * min(max(l - 4, 0), 4)));
    m.z = (uint32_t)(~0ull << (8 * min(max(l - 8, 0), 4)));
    m.w = (uint32_t)(~0ull << (8 * min(max(l - 12, 0), 4)));
    qmask[l] = m;
  }
  lds_sync();  // the block's waves share only LDS
  // 1b. wave 0, one lane per blob, from the blob's staged header: whether its segments lie in
  // order, the record header and the segment table at the blob's rank among the participants.
  // (A participant passed classify(): every length and position is below its blob's length.)
  if (tid < 64) {
    bool ok = true;
    if (keep) {
      const int32_t at = area + (int32_t)(uint32_t)(b - hull_b);  // the blob's first byte in the image
      const u32x4_ua l0 = *reinterpret_cast<const u32x4_ua*>(img + at + 16), l1 = *reinterpret_cast<const u32x4_ua*>(img + at + 32);
      const u32x4_ua p0 = *reinterpret_cast<const u32x4_ua*>(img + at + 48), p1 = *reinterpret_cast<const u32x4_ua*>(img + at + 64);
      const uint32_t len[NF] = {l0.x, l0.z, l1.x, l1.z}, pos[NF] = {p0.x, p0.z, p1.x, p1.z};
      uint8_t* h = img + kArcHdr + kArcSlot * rank;
      *reinterpret_cast<u32x4_al*>(h) = u32x4_al{(uint32_t)kCmd0, (uint32_t)(kCmd0 >> 32), (uint32_t)kCmd1, 0};
#pragma unroll
      for (int c = 1; c < 7; ++c) {
        uint32_t w0, w1;
        scom_chunk<uint32_t>(c, len[0], len[1], len[2], len[3], w0, w1);
        *reinterpret_cast<u32x4_al*>(h + 16 * c) = u32x4_al{w0, 0, w1, 0};  // (chunk 6: the slot's last 8 bytes are spare)
      }
      int32_t start = (int32_t)(uint32_t)(mine - o_first);
      seg[NS * rank] = seg_pack(kArcHdr + kArcSlot * (int32_t)rank - start, start + kScom);
      start += kScom;
      uint32_t hi = 0;
#pragma unroll
      for (int s = 0; s < NF; ++s) {
        // the pos of a length-0 segment is ignored: it supplies no byte, any place in the image will do
        const int32_t from = len[s] ? at + (int32_t)pos[s] : kArcHdr;
        if (len[s]) {
          ok = ok && pos[s] >= hi;
          hi = pos[s] + len[s];
        }
        seg[NS * rank + 1 + s] = seg_pack(from - start, start + (int32_t)len[s]);
        start += (int32_t)len[s];
      }
      if (rank + 1 == nk) seg[NS * nk] = seg_pack(kArcHdr, start);  // read (never used) as the last segment's successor
    }
    const bool any_bad = __ballot(!ok) != 0;
    if (tid == 0) unordered = any_bad ? 1u : 0u;
  }
  lds_sync();
  if (unordered) {  // block-uniform: permuted or overlapping segments inside a blob
    if (tid / 8 < nr) direct_record<8>(blobs, blob_off, out, rec_off, r0 + tid / 8, tid % 8);
    return;
  }
  // 1c. the piece table: which segment holds each piece's first byte
  for (uint32_t g = tid; g < NS * nk; g += 256) {
    const int32_t end = seg_unpack(seg[g]).y, beg = g ? seg_unpack(seg[g - 1]).y : 0;
    const int32_t last = (end - 1 + d0) >> 4;
    for (int32_t p = g ? (beg + d0 + 15) >> 4 : 0; p <= last; p += 4) {
#pragma unroll
      for (int32_t u = 0; u < 4; ++u) tab[p + u <= last ? p + u : kArcPieces] = (uint8_t)g;
    }
  }
  lds_sync();
  // 2. aligned output pieces: the window of each segment in the piece, aligned with the
  // piece, merged forward (segment k supplies bytes [its start, 16) over what came before)
  const int32_t sp = (int32_t)span;
  const uint32_t np = (uint32_t)((d0 + sp + 15) >> 4);
  uint8_t* const base = out + (o_first - (uint64_t)d0);
  auto piece = [&](uint32_t p, uint32_t g, int2 s0, int2 s1, const u32x4_ua& w0, const u32x4_ua& w1) {
    const int32_t x = 16 * (int32_t)p - d0, end = min(x + 16, sp);
    u32x4_al acc = {w0.x, w0.y, w0.z, w0.w};
    int32_t pos = s0.y;
    auto merge = [&](const u32x4_ua& w) {  // bytes [pos - x, 16) from w
      const u32x4_al q = qmask[pos - x];
      acc.x = (w.x & q.x) | (acc.x & ~q.x);
      acc.y = (w.y & q.y) | (acc.y & ~q.y);
      acc.z = (w.z & q.z) | (acc.z & ~q.z);
      acc.w = (w.w & q.w) | (acc.w & ~q.w);
    };
    if (pos < end) {
      if (s1.y > pos) {
        merge(w1);
        pos = s1.y;
      }
      ++g;
      while (pos < end) {
        const int2 sn = seg_unpack(seg[++g]);
        if (sn.y > pos) {
          merge(*reinterpret_cast<const u32x4_ua*>(img + sn.x + x));
          pos = sn.y;
        }
      }
    }
    return acc;
  };
  // A piece's next segment is read before it is known to reach into the piece (the read is
  // then discarded), and its window can fall outside the image: clamp the index into it.
  auto window = [&](int2 sg, uint32_t p) {
    const int32_t at = min(max(sg.x + 16 * (int32_t)p - d0, 0), kArcImg - 16);
    return *reinterpret_cast<const u32x4_ua*>(img + at);
  };
  auto build = [&](uint32_t p) {
    const uint32_t g = tab[p];
    const int2 s0 = seg_unpack(seg[g]), s1 = seg_unpack(seg[g + 1]);  // the piece's segment and the next
    return piece(p, g, s0, s1, window(s0, p), window(s1, p));
  };
  // pieces wholly inside the span: one aligned store each; the (at most two) pieces shared
  // with the neighbouring blocks: this block's bytes only, by two lanes of waves 2 and 3
  const uint32_t pf = d0 ? 1u : 0u, pl = ((d0 + sp) & 15) ? np - 1u : np;
  for (uint32_t p = pf + tid; p < pl; p += 256) __builtin_nontemporal_store(build(p), reinterpret_cast<u32x4_al*>(base + 16ull * p));
  const uint32_t pe = tid == 128 && pf ? 0u : tid == 192 && pl < np && (pl > 0 || !pf) ? np - 1u : ~0u;
  if (pe != ~0u) {
    const u32x4_al acc = build(pe);
    const int32_t x = 16 * (int32_t)pe - d0;
    const uint32_t wv[4] = {acc.x, acc.y, acc.z, acc.w};
    for (int k = max(0, -x); k < 16 && x + k < sp; ++k) base[16ull * pe + k] = (uint8_t)(wv[k >> 2] >> (8 * (k & 3)));
  }
}

}  // namespace

// Returns a K2H_AMD_* code (the HIP error, if any, in *herr) and synchronises the stream once
// to return *total and *records.  n >= 1.
int launch_ralledata_archive(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                             const uint8_t* keep, void* out, uint64_t out_cap, uint64_t* rec_off, uint64_t* records,
                             uint64_t* total, hipStream_t stream, hipError_t* herr) {
  const uint64_t grid_s = n / 256 + 1, grid_b = (n + kArcBlobs - 1) / kArcBlobs;
  if (grid_b > 0x7FFFFFFFull) return K2H_AMD_EINVAL;
  hipError_t e = hipSuccess;
  auto tr = [&](hipError_t x) {
    if (e == hipSuccess) e = x;
  };
  size_t scan_bytes = 0;
  uint8_t* tmp = nullptr;
  tr(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, rec_off, rec_off, n + 1, stream));
  const size_t counters_at = align256(scan_bytes ? scan_bytes : 1);
  if (e == hipSuccess) tr(hipMallocAsync((void**)&tmp, counters_at + kCounterBytes, stream));
  unsigned long long* counters = (unsigned long long*)(tmp + counters_at);
  if (e == hipSuccess) tr(hipMemsetAsync(counters, 0, kCounterBytes, stream));
  if (e == hipSuccess) {
    scom_archive_size_kernel<<<(unsigned)grid_s, 256, 0, stream>>>((const uint8_t*)blobs, size, blob_off, n, keep,
                                                                  rec_off, counters);
    tr(hipGetLastError());
  }
  if (e == hipSuccess) tr(hipcub::DeviceScan::ExclusiveSum(tmp, scan_bytes, rec_off, rec_off, n + 1, stream));
  uint64_t tot = 0;
  unsigned long long counts[kCounterBytes / 8];
  if (e == hipSuccess) tr(hipMemcpyAsync(&tot, rec_off + n, 8, hipMemcpyDeviceToHost, stream));
  if (e == hipSuccess) tr(hipMemcpyAsync(counts, counters, kCounterBytes, hipMemcpyDeviceToHost, stream));
  if (tmp) tr(hipFreeAsync(tmp, stream));
  if (e == hipSuccess) tr(hipStreamSynchronize(stream));
  int rc = K2H_AMD_OK;
  if (e == hipSuccess) {
    *total = tot;
    if (records) *records = counter_sum(counts, 0);
    if (out && tot > out_cap) {
      rc = K2H_AMD_EINVAL;
    } else if (out && tot) {
      scom_archive_build_kernel<<<(unsigned)grid_b, 256, 0, stream>>>((const uint8_t*)blobs, blob_off, n,
                                                                     (uint8_t*)out, rec_off);
      tr(hipGetLastError());
    }
  }
  *herr = e;
  return e != hipSuccess ? K2H_AMD_EHIP : rc;
}

}  // namespace k2h
