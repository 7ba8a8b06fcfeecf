// k2hash_amd -- RALLEDATA blobs straight from range records (include/k2hash_amd.h section 4c).
//
// The device scans (k2h_import_dev.hip, k2h_archive_dev.hip) report each record of a file in
// HBM as offsets and lengths into that file; this producer turns those records into the packed
// direct-set blobs of section 4 without a CSR copy in between.  Blob sizes differ per record
// and a record may yield no blob, so the blob offsets are a scan: a sizing kernel writes each
// record's blob size (80 + its segment lengths, or 0) into blob_off, an exclusive sum turns
// them into offsets in place, and the build kernel places the blobs by them.
//
// Build kernel = the scheme of ralledata_gather_kernel (k2h_ralledata.hip): a 256-thread block
// takes 64 consecutive records, whose blobs are one contiguous output span.  The records of a
// scanned file lie nearly back to back in it (TSV: key TAB value NL ...; archive: header,
// segments ...), so the block stages ONE run of the file -- the aligned 16-byte hull of its
// records' bytes -- into LDS, builds the headers there, hashes the keys from the staged bytes
// in wave 0 while waves 1-3 build the piece table, and writes the span as aligned 16-byte
// non-temporal pieces.  Five segments per record, the table shape of the CSR kernel:
//   import:  header, key, NUL, value, NUL   (the NULs are 1-byte segments whose source is a
//                                            zero byte of the LDS image: written, not copied)
//   archive: header, key, value, subkeys, attrs
// The kernel is written once and takes the record format as a reader type.
//
// Staged or direct (block-uniform).  Walk the block's kept records in order and, in each, its
// file segments of length > 0 in blob order.  The block is STAGED when every such segment
// starts at or after the end of the one before it (file order, no overlap) and the distance
// from the first one's start to the last one's end is at most kRecHullMax (the aligned hull
// then fits the pool at any alignment of the file); a block without any such segment is
// staged with an empty hull.  Every other block is DIRECT: 8 lanes per record straight from
// HBM (one large value, a stretch of an archive dominated by records that yield no blob,
// caller-permuted or overlapping records, mdbm's key line at EOF whose value is the previous
// record's).  Both forms write the same bytes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_ralle_pieces.h"

namespace k2h {
namespace {

constexpr int kRecRecs = 64;                // records per 256-thread block
constexpr int kRecPool = 12288;             // staged file bytes (the aligned hull)
constexpr int kRecHullMax = kRecPool - 32;  // first start .. last end; + 2 x 15 bytes of alignment fits the pool
constexpr int kRecHdr = 16;                 // LDS offset of the headers; the 16 bytes below are zero
constexpr int kRecZero = 15;                // the zero byte every NUL segment reads
constexpr int kRecImg = kRecHdr + 80 * kRecRecs + kRecPool + 16;
constexpr int kRecSpanMax = 80 * kRecRecs + kRecHullMax + 2 * kRecRecs;  // headers, file bytes, NULs
constexpr int kRecPieces = kRecSpanMax / 16 + 2;

__device__ __forceinline__ bool inside(uint64_t off, uint64_t len, uint64_t size) { return off <= size && len <= size - off; }

// The record readers: NF file segments per record in blob order; read() returns whether the
// record yields a blob and, only then, its segments (nothing of a skipped record is used).
struct ImportReader {  // key + NUL, value + NUL: the strings K2HShm::Set(const char*, const char*) stores
  typedef k2h_amd_import_rec Rec;
  static constexpr int NF = 2;
  static constexpr bool kNul = true;
  static __device__ __forceinline__ bool read(const Rec* recs, uint64_t i, uint64_t size, uint64_t (&off)[NF],
                                              uint64_t (&len)[NF]) {
    const Rec r = recs[i];
    off[0] = r.key_off, len[0] = r.key_len, off[1] = r.val_off, len[1] = r.val_len;
    return inside(r.key_off, r.key_len, size) && inside(r.val_off, r.val_len, size);
  }
};
struct ArchiveReader {  // a whole element as stored: SCOM_SET_ALL (type 0) with a key
  typedef k2h_amd_archive_rec Rec;
  static constexpr int NF = 4;
  static constexpr bool kNul = false;
  static __device__ __forceinline__ bool read(const Rec* recs, uint64_t i, uint64_t size, uint64_t (&off)[NF],
                                              uint64_t (&len)[NF]) {
    const Rec& r = recs[i];
    if (r.status != 0 || r.type != 0 || r.key_len == 0) return false;
    off[0] = r.key_off, len[0] = r.key_len, off[1] = r.val_off, len[1] = r.val_len;
    off[2] = r.skey_off, len[2] = r.skey_len, off[3] = r.attrs_off, len[3] = r.attrs_len;
    return inside(off[0], len[0], size) && inside(off[1], len[1], size) && inside(off[2], len[2], size) &&
           inside(off[3], len[3], size);
  }
};

// The four length fields of the header, and what the terminators add to a blob.
template <class Rd, class T>
__device__ __forceinline__ void field_lens(const T (&len)[Rd::NF], T (&f)[4]) {
  if constexpr (Rd::kNul) f[0] = len[0] + 1, f[1] = len[1] + 1, f[2] = 0, f[3] = 0;
  else f[0] = len[0], f[1] = len[1], f[2] = len[2], f[3] = len[3];
}

template <class Rd>
__global__ __launch_bounds__(256) void ralledata_recs_size_kernel(const typename Rd::Rec* __restrict__ recs,
                                                                  uint64_t size, uint64_t n,
                                                                  uint64_t* __restrict__ sizes) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  uint64_t v = 0, off[Rd::NF], len[Rd::NF];
  if (i < n && Rd::read(recs, i, size, off, len)) {
    uint64_t f[4];
    field_lens<Rd>(len, f);
    v = 80 + f[0] + f[1] + f[2] + f[3];
  }
  sizes[i] = v;  // entry n is 0: entry n of the exclusive sum is the total
}

// Finish a key hash: as stored (archive), or of key + NUL from the hash `raw` of the key
// alone -- one more FNV step with byte 0 is a multiply by the prime, so h1 = raw * P and
// h2 = raw; the empty key is the 1-byte string "\0" with h2 = h1 (lib/k2hashfunc.cc:83).
template <bool NUL>
__device__ __forceinline__ void finish_hash(bool empty, bool one, uint64_t seed, uint64_t& r1, uint64_t& r2) {
  if constexpr (NUL) {
    const uint64_t raw = empty ? seed : r1;
    r1 = raw * kPrime;
    r2 = empty ? r1 : raw;
  } else {
    if (one) r2 = r1;         // lib/k2hashfunc.cc:83
    if (empty) r1 = r2 = 0;   // lib/k2hashfunc.cc:66-68, 80-82
  }
}

// Key hash from the staged bytes (staged_key_hash of k2h_ralledata.hip): end-aligned chunks;
// an empty key is passed to the walk as k = 0, whose one chunk at `end` is don't-care bytes
// inside the image and whose result finish_hash drops.
template <bool NUL>
__device__ __forceinline__ void staged_hash(const uint8_t* end, uint32_t len, const uint64_t* spad, uint64_t& r1,
                                            uint64_t& r2) {
  const uint32_t k = (len + 15) >> 4;
  const uint8_t* cp = end - 16 * k;
  const uint32_t p = 16 * k - len;
  r2 = 0;
  end_aligned_walk<!NUL, false>(
      k, p, mask_lead(ld16(cp), p), spad, [=](uint32_t q) { return ld16(cp + 16 * q); }, r1, r2);
  finish_hash<NUL>(!len, len == 1, spad[0], r1, r2);
}

// The same straight from the file (direct form); bytes below the file are never read.
template <bool NUL>
__device__ __forceinline__ void file_hash(const uint8_t* file, uint64_t b, uint64_t len, const uint64_t* spad,
                                          uint64_t& r1, uint64_t& r2) {
  r1 = r2 = 0;
  if (len) {
    const uint64_t k = (len + 15) >> 4;
    end_aligned_walk_ptr<!NUL, false>(k, (uint32_t)(16 * k - len), file + b + len - 16 * k, file, spad, r1, r2);
  }
  finish_hash<NUL>(!len, len == 1, spad[0], r1, r2);
}

// Direct form: one record by a group of G lanes, straight to HBM; lane 0 hashes the key.
template <class Rd, int G>
__device__ __forceinline__ void direct_record(const uint8_t* __restrict__ file, uint64_t size,
                                              const typename Rd::Rec* __restrict__ recs, uint8_t* __restrict__ out,
                                              const uint64_t* __restrict__ blob_off, uint64_t i, uint32_t q,
                                              const uint64_t* spad) {
  uint64_t off[Rd::NF], len[Rd::NF], f[4];
  if (!Rd::read(recs, i, size, off, len)) return;
  field_lens<Rd>(len, f);
  uint8_t* b = out + blob_off[i];
  if (q < 5) {
    uint64_t f0, f1;
    switch (q) {
      case 0: file_hash<Rd::kNul>(file, off[0], len[0], spad, f0, f1); break;
      case 1: f0 = f[0]; f1 = f[1]; break;
      case 2: f0 = f[2]; f1 = f[3]; break;
      case 3: f0 = 80; f1 = 80 + f[0]; break;
      default: f0 = 80 + f[0] + f[1]; f1 = 80 + f[0] + f[1] + f[2]; break;
    }
    *reinterpret_cast<u32x4_ua*>(b + 16 * q) = u32x4_ua{(uint32_t)f0, (uint32_t)(f0 >> 32), (uint32_t)f1, (uint32_t)(f1 >> 32)};
  }
  uint64_t at = 80;
#pragma unroll
  for (int s = 0; s < Rd::NF; ++s) {
    if (len[s]) group_copy<G>(b + at, file + off[s], len[s], q);
    at += len[s];
    if constexpr (Rd::kNul) {
      if (q == 5u + s) b[at] = 0;  // the terminator: written, never copied
      at += 1;
    }
  }
}

__device__ __forceinline__ uint64_t read_lane64(uint64_t v, uint32_t lane) {
  return pack2((uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)lane),
               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)lane));
}

// 8 blocks per CU, as the CSR gather kernel: under 20 KiB of LDS, at most 64 VGPRs.
template <class Rd>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void ralledata_recs_kernel(
    const uint8_t* __restrict__ file, uint64_t size, const typename Rd::Rec* __restrict__ recs, uint64_t n,
    uint8_t* __restrict__ out, const uint64_t* __restrict__ blob_off, SpadTable spad_tab) {
  constexpr int NS = 5, NF = Rd::NF;
  constexpr int R = kRecRecs, NSEG = NS * R;
  typedef uint32_t u32x4_al __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) uint8_t img[kRecImg];
  __shared__ uint32_t seg[NSEG + 1];  // segment g: seg_pack(adj, end)
  constexpr int NRUN = (kRecPieces + 63) / 64;
  __shared__ uint8_t tab[kRecPieces + 1];  // low byte of the segment holding piece p's first byte (+ a dump slot)
  __shared__ uint16_t tbase[NRUN + 1];     // segment holding piece 64 j's first byte (+ a dump slot)
  __shared__ u32x4_al qmask[17];
  __shared__ uint64_t spad[16];
  static_assert(kRecImg + 4 * (NSEG + 1) + kRecPieces + 1 + 2 * (NRUN + 1) + 16 * 17 + 8 * 16 <= 20 * 1024,
                "8 blocks per CU");
  static_assert(kRecSpanMax < 32768, "seg_pack: adj and end in 16 bits");
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint64_t r0 = (uint64_t)blockIdx.x * R;
  const uint32_t nr = (uint32_t)(n - r0 < (uint64_t)R ? n - r0 : (uint64_t)R);
  const uint64_t o_first = blob_off[r0];
  const uint64_t span = blob_off[r0 + nr] - o_first;
  if (span == 0) return;  // no record of the block yields a blob

  // Every wave reads the block's 64 records (lane l: record r0 + l) and derives the same
  // block-uniform facts from them with wave operations: no barrier before the staged loads.
  uint64_t off[NF], len[NF];
  const bool keep = lane < nr && Rd::read(recs, r0 + lane, size, off, len);
  // the record's own run: its first start, its last end, in order and not overlapping
  uint64_t lo = ~0ull, hi = 0;
  bool ok = true;
#pragma unroll
  for (int s = 0; s < NF; ++s) {
    if (!keep) off[s] = len[s] = 0;
    if (len[s]) {
      ok = ok && off[s] >= hi;
      lo = lo == ~0ull ? off[s] : lo;
      hi = off[s] + len[s] > hi ? off[s] + len[s] : hi;
    }
  }
  // the last end among the records before this one (an inclusive max scan, shifted by one)
  uint64_t inc = hi;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint64_t t = __shfl_up(inc, d);
    if (lane >= d && t > inc) inc = t;
  }
  uint64_t prev = __shfl_up(inc, 1u);
  if (lane == 0) prev = 0;
  ok = ok && (lo == ~0ull || lo >= prev);
  const uint64_t with_bytes = __ballot(lo != ~0ull), kept = __ballot(keep);
  const bool ordered = __ballot(!ok) == 0;
  const uint64_t hull_b = with_bytes ? read_lane64(lo, (uint32_t)__ffsll((unsigned long long)with_bytes) - 1u) : 0;
  const uint64_t hull_e = with_bytes ? read_lane64(inc, 63u) : 0;
  const uint32_t nk = (uint32_t)__popcll(kept), rank = (uint32_t)__popcll(kept & ((1ull << lane) - 1ull));

  if (!ordered || hull_e - hull_b > (uint64_t)kRecHullMax) {  // block-uniform: the direct form
    if (tid < 16) spad[tid] = spad_tab.v[tid];
    __syncthreads();
    for (uint32_t rec = tid / 8; rec < nr; rec += 32) direct_record<Rd, 8>(file, size, recs, out, blob_off, r0 + rec, tid % 8, spad);
    return;
  }

  // the staged run: file bytes [hull_b, hull_e), its aligned hull, file byte f at img[area + f - hull_b]
  const uint64_t a_b = (uint64_t)(uintptr_t)(file + hull_b), a_lo = a_b & ~15ull;
  const uint32_t hull_n = with_bytes ? (uint32_t)((((uint64_t)(uintptr_t)(file + hull_e) + 15) & ~15ull) - a_lo) >> 4 : 0u;
  const int32_t area = kRecHdr + 80 * R + (int32_t)(a_b - a_lo);
  // 1a. the staged pieces: up to PPT aligned non-temporal loads per thread of waves 1-3
  constexpr uint32_t SW = 64, NST = 256 - SW;
  constexpr int PPT = (kRecPool / 16 + NST - 1) / NST;
  u32x4_al v[PPT];
  uint32_t dst[PPT];
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    const uint32_t q = tid - SW + NST * u;
    dst[u] = 0xffffffffu;
    if (tid >= SW && q < hull_n) {
      // a global (not flat) load, so that the LDS reads after the barrier do not wait for it
      v[u] = __builtin_nontemporal_load(
          reinterpret_cast<const __attribute__((address_space(1))) u32x4_al*>((uintptr_t)(a_lo + 16ull * q)));
      dst[u] = kRecHdr + 80 * R + 16 * q;
    }
  }
  // 1b. wave 0, one lane per record: header and segment table, at the record's rank among the
  // kept ones (a skipped record has no segments, so a 64-piece run still meets < 256 of them)
  const uint64_t a_out = (uint64_t)(uintptr_t)(out + o_first);
  const int32_t d0 = (int32_t)(a_out & 15u);
  if (tid < 17) {  // qmask[l] = bytes [l, 16) of a piece
    u32x4_al m;
    m.x = (uint32_t)(~0ull << (8 * min(max((int)tid - 0, 0), 4)));
    m.y = (uint32_t)(~0ull << (8 * min(max((int)tid - 4, 0), 4)));
    m.z = (uint32_t)(~0ull << (8 * min(max((int)tid - 8, 0), 4)));
    m.w = (uint32_t)(~0ull << (8 * min(max((int)tid - 12, 0), 4)));
    qmask[tid] = m;
  }
  if (tid < 16) spad[tid] = spad_tab.v[tid];
  if (tid == 32) *reinterpret_cast<u32x4_al*>(img) = u32x4_al{0, 0, 0, 0};  // holds the zero byte
  uint32_t rel[NF], l32[NF];
#pragma unroll
  for (int s = 0; s < NF; ++s) {
    l32[s] = (uint32_t)len[s];
    rel[s] = len[s] ? (uint32_t)(off[s] - hull_b) : 0u;
  }
  if (tid < 64 && keep) {
    uint32_t fl[4];
    field_lens<Rd>(l32, fl);
    const int32_t B = (int32_t)(uint32_t)(blob_off[r0 + tid] - o_first);
    const uint32_t f[20] = {0, 0, 0, 0, fl[0], 0, fl[1], 0, fl[2], 0,  // hashes: filled in by wave 0 below
                            fl[3], 0, 80, 0, 80 + fl[0], 0, 80 + fl[0] + fl[1], 0, 80 + fl[0] + fl[1] + fl[2], 0};
#pragma unroll
    for (int c = 0; c < 5; ++c)
      *reinterpret_cast<u32x4_al*>(img + kRecHdr + 80 * rank + 16 * c) = u32x4_al{f[4 * c], f[4 * c + 1], f[4 * c + 2], f[4 * c + 3]};
    int32_t start = B;
#pragma unroll
    for (int c = 0; c < NS; ++c) {
      // segment c of the record: the header, a file segment, or (import) a terminator
      int32_t L, from;
      if (c == 0) {
        L = 80, from = kRecHdr + 80 * (int32_t)rank;
      } else if (Rd::kNul && c % 2 == 0) {
        L = 1, from = kRecZero;
      } else {
        const int s = Rd::kNul ? (c - 1) / 2 : c - 1;
        L = (int32_t)l32[s], from = area + (int32_t)rel[s];
      }
      seg[NS * rank + c] = seg_pack(from - start, start + L);
      start += L;
    }
    if (rank + 1 == nk) seg[NS * nk] = seg_pack(kRecHdr, start);  // read (never used) as the last segment's successor
  }
#pragma unroll
  for (int u = 0; u < PPT; ++u)
    if (dst[u] != 0xffffffffu) *reinterpret_cast<u32x4_al*>(img + dst[u]) = v[u];
  lds_sync();  // the block's waves share only LDS
  // 1c'. the piece table, by waves 1-3 while wave 0 hashes (as in ralledata_gather_kernel)
  if (tid >= 64)
    for (uint32_t g = tid - 64; g < NS * nk; g += 192) {
      const int32_t end = seg_unpack(seg[g]).y, beg = g ? seg_unpack(seg[g - 1]).y : 0;
      const int32_t last = (end - 1 + d0) >> 4;
      for (int32_t p = g ? (beg + d0 + 15) >> 4 : 0; p <= last; p += 4) {
#pragma unroll
        for (int32_t u = 0; u < 4; ++u) tab[p + u <= last ? p + u : kRecPieces] = (uint8_t)g;
        const int32_t r = (p + 63) & ~63;  // the run start among pieces p .. p + 3, if any
        tbase[r <= min(p + 3, last) ? r >> 6 : NRUN] = (uint16_t)g;
      }
    }
  // 1c. wave 0 hashes the kept records' keys from the image into the headers (an empty key
  // has no place in the staged run: its don't-care chunk is read at the pool's start)
  if (tid < 64 && keep) {
    uint64_t h1, h2;
    staged_hash<Rd::kNul>(img + (l32[0] ? area + (int32_t)(rel[0] + l32[0]) : kRecHdr + 80 * R), l32[0], spad, h1, h2);
    *reinterpret_cast<u32x4_al*>(img + kRecHdr + 80 * rank) =
        u32x4_al{(uint32_t)h1, (uint32_t)(h1 >> 32), (uint32_t)h2, (uint32_t)(h2 >> 32)};
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
    const int32_t at = min(max(sg.x + 16 * (int32_t)p - d0, 0), kRecImg - 16);
    return *reinterpret_cast<const u32x4_ua*>(img + at);
  };
  auto build = [&](uint32_t p) {
    const uint32_t gb = tbase[p >> 6];
    const uint32_t g = gb + ((tab[p] - gb) & 0xffu);
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

template <class Rd>
int build_from_recs(const void* file, uint64_t size, const void* recs, uint64_t n, uint64_t seed, void* out,
                    uint64_t out_cap, uint64_t* blob_off, uint64_t* total, hipStream_t stream, hipError_t* herr) {
  typedef typename Rd::Rec Rec;
  const uint64_t grid_s = n / 256 + 1, grid_b = (n + kRecRecs - 1) / kRecRecs;
  if (grid_b > 0x7FFFFFFFull) return K2H_AMD_EINVAL;
  hipError_t e = hipSuccess;
  auto tr = [&](hipError_t x) {
    if (e == hipSuccess) e = x;
  };
  size_t tmp_bytes = 0;
  void* tmp = nullptr;
  tr(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, blob_off, blob_off, n + 1, stream));
  if (e == hipSuccess) tr(hipMallocAsync(&tmp, tmp_bytes ? tmp_bytes : 1, stream));
  if (e == hipSuccess) {
    ralledata_recs_size_kernel<Rd><<<(unsigned)grid_s, 256, 0, stream>>>((const Rec*)recs, size, n, blob_off);
    tr(hipGetLastError());
  }
  if (e == hipSuccess) tr(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, blob_off, blob_off, n + 1, stream));
  if (tmp) tr(hipFreeAsync(tmp, stream));
  uint64_t tot = 0;
  if (e == hipSuccess) tr(hipMemcpyAsync(&tot, blob_off + n, 8, hipMemcpyDeviceToHost, stream));
  if (e == hipSuccess) tr(hipStreamSynchronize(stream));
  int rc = K2H_AMD_OK;
  if (e == hipSuccess) {
    *total = tot;
    if (out && tot > out_cap) {
      rc = K2H_AMD_EINVAL;
    } else if (out && tot) {
      ralledata_recs_kernel<Rd><<<(unsigned)grid_b, 256, 0, stream>>>((const uint8_t*)file, size, (const Rec*)recs, n,
                                                                      (uint8_t*)out, blob_off, make_spad(seed));
      tr(hipGetLastError());
    }
  }
  *herr = e;
  return e != hipSuccess ? K2H_AMD_EHIP : rc;
}

}  // namespace

int launch_import_ralledata(const void* file, uint64_t size, const k2h_amd_import_rec* recs, uint64_t n, uint64_t seed,
                            void* out, uint64_t out_cap, uint64_t* blob_off, uint64_t* total, hipStream_t stream,
                            hipError_t* herr) {
  return build_from_recs<ImportReader>(file, size, recs, n, seed, out, out_cap, blob_off, total, stream, herr);
}

int launch_archive_ralledata(const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n,
                             uint64_t seed, void* out, uint64_t out_cap, uint64_t* blob_off, uint64_t* total,
                             hipStream_t stream, hipError_t* herr) {
  return build_from_recs<ArchiveReader>(file, size, recs, n, seed, out, out_cap, blob_off, total, stream, herr);
}

}  // namespace k2h
