// k2hash_amd -- k2hash archive scan and prehash on the GPU.
//
// The same records as the host scanner (k2h_archive.cc, restating K2HArchive::Load,
// lib/k2harchive.cc:279-383) for a file that already sits in HBM, without a host pass.
// The SCOM record stream (lib/k2hcommand.h:64-79) has no index and no alignment: record
// i + 1 starts 104 + the five lengths of record i later, so the host scan is a pointer
// chase.  The handle is szCommand, which the reference's writer always starts with
// SCOM_COMSTR_PREFIX "\nK2H_" (lib/k2hcommand.h:36-45, lib/k2hcommand.cc:116-186):
//   detect   every offset whose five bytes are the prefix (a "candidate"), in file order:
//            a count pass, a scan of the per-wave counts, a write pass;
//   link     one lane per candidate: the candidate index of
//            the header that follows its record (binary search), END or MISS;
//   resolve  which candidates lie on the chain from offset 0: reach / jump doubling, every
//            hop is at least 104 bytes so ceil(log2(size / 104 + 1)) rounds, known up front;
//   emit     ranks of the reached candidates (exclusive scan), one record each; the keys
//            hashed by the same lane when the caller asked for the prehash.
// A prefix inside a value is a candidate too (a decoy): nothing reaches it, so it costs
// work and no record.  Where the chain arrives at an offset that holds no prefix (MISS),
// the scan ends there with one K2H_AMD_ARCHIVE_NO_MAGIC record (include/k2hash_amd.h).
//
// Every length and position in a header is untrusted: every read of the file goes through
// FileView, whose accessors check the range against the file size in overflow-safe form.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <mutex>

#include "../../include/k2hash_amd.h"
#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_scratch.h"

namespace k2h {
namespace {

constexpr uint64_t kScom = 104;  // sizeof(SCOM), packed (lib/k2hcommand.h:64-79)
// "\nK2H_" as the low five bytes of a little-endian load
constexpr uint64_t kMagic5 = 0x5F48324B0Aull;

constexpr uint32_t kThreads = 256;
// detect: a wave reads kDetQ pieces of 16 bytes per lane, 64 lanes side by side: 4 KiB
constexpr uint32_t kDetQ = 4;
constexpr uint32_t kDetWave = 64u * 16u * kDetQ;
constexpr uint32_t kDetWavesPerBlock = kThreads / 64u;

// next[] values that are no candidate index
constexpr uint32_t kEnd = 0xFFFFFFFFu;   // the scan stops after this record
constexpr uint32_t kMiss = 0xFFFFFFFEu;  // a header fits at the next offset, but it is no candidate
constexpr uint64_t kMaxCand = 0xFFFFFFFEull;  // candidate indices are 32-bit: more is K2H_AMD_EINVAL

typedef uint64_t u64_ua __attribute__((aligned(1)));
typedef uint32_t u32_ua __attribute__((aligned(1)));

// The only way to the file's bytes.  has(off, len): [off, off + len) lies inside the file,
// written so that no sum can wrap.  A load whose range does not lie inside reads the bytes
// that do and zeroes for the rest, never memory outside [f, f + size).
struct FileView {
  const uint8_t* f;
  uint64_t size;
  __device__ bool has(uint64_t off, uint64_t len) const { return off <= size && len <= size - off; }
  __device__ uint32_t byte(uint64_t off) const { return off < size ? f[off] : 0u; }
  __device__ uint32_t ld4(uint64_t off) const {
    if (has(off, 4)) return *reinterpret_cast<const u32_ua*>(f + off);
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4; ++j)
      if (off <= size && j < size - off) v |= (uint32_t)f[off + j] << (8 * j);
    return v;
  }
  __device__ uint64_t ld8(uint64_t off) const {
    if (has(off, 8)) return *reinterpret_cast<const u64_ua*>(f + off);
    uint64_t v = 0;
    for (uint32_t j = 0; j < 8; ++j)
      if (off <= size && j < size - off) v |= (uint64_t)f[off + j] << (8 * j);
    return v;
  }
  __device__ uint4 ld16(uint64_t off) const {
    if (has(off, 16)) {
      const u32x4_ua v = *reinterpret_cast<const u32x4_ua*>(f + off);
      return make_uint4(v.x, v.y, v.z, v.w);
    }
    return make_uint4(ld4(off), ld4(off + 4 < off ? size : off + 4), ld4(off + 8 < off ? size : off + 8),
                      ld4(off + 12 < off ? size : off + 12));
  }
};

// ---------------------------------------------------------------------------
// Detect.
// ---------------------------------------------------------------------------
// bit 7 of every byte of w that equals c (exact: no borrow between bytes)
__device__ inline uint32_t eq_bytes(uint32_t w, uint32_t c4) {
  const uint32_t t = w ^ c4;
  return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}

// Candidates that start in the 16 bytes v (the four bytes after them in halo): bit k set for
// a prefix at byte k.  A newline followed by 'K' is found for all 16 positions at once; the
// few such places are then compared in full.
__device__ inline uint32_t piece_mask(uint4 v, uint32_t halo) {
  const uint32_t w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w, w4 = halo;
  const uint32_t k0 = eq_bytes(w0, 0x4B4B4B4Bu), k1 = eq_bytes(w1, 0x4B4B4B4Bu), k2 = eq_bytes(w2, 0x4B4B4B4Bu),
                 k3 = eq_bytes(w3, 0x4B4B4B4Bu), k4 = eq_bytes(w4, 0x4B4B4B4Bu);
  // a newline at byte b of word j whose next byte is 'K'
  const uint32_t c0 = eq_bytes(w0, 0x0A0A0A0Au) & __builtin_amdgcn_alignbit(k1, k0, 8);
  const uint32_t c1 = eq_bytes(w1, 0x0A0A0A0Au) & __builtin_amdgcn_alignbit(k2, k1, 8);
  const uint32_t c2 = eq_bytes(w2, 0x0A0A0A0Au) & __builtin_amdgcn_alignbit(k3, k2, 8);
  const uint32_t c3 = eq_bytes(w3, 0x0A0A0A0Au) & __builtin_amdgcn_alignbit(k4, k3, 8);
  // byte b of word j at bit 8 b + j
  uint32_t c = (c0 >> 7) | (c1 >> 6) | (c2 >> 5) | (c3 >> 4);
  uint32_t m = 0;
  while (c) {
    const uint32_t t = (uint32_t)__builtin_ctz(c);
    c &= c - 1;
    const uint32_t j = t & 7u, b = t >> 3;
    const uint32_t lo = j == 0 ? w0 : j == 1 ? w1 : j == 2 ? w2 : w3;
    const uint32_t hi = j == 0 ? w1 : j == 1 ? w2 : j == 2 ? w3 : w4;
    const uint64_t x = (pack2(lo, hi) >> (8 * b)) & 0xFFFFFFFFFFull;
    m |= x == kMagic5 ? 1u << (4 * j + b) : 0u;
  }
  return m;
}

__device__ inline uint32_t lanes_below(uint64_t b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// One wave's 4 KiB: the candidate mask of each lane's kDetQ pieces.  Piece q of lane l is
// at wbase + 16 (64 q + l): each load instruction reads 1 KiB side by side.  Bytes past the
// file read as zero (no candidate: a prefix has no zero byte), so a candidate at p always has
// p + 5 <= size.  The four bytes after a piece are the next lane's first word; lane 63 takes
// them from lane 0's next piece, or -- for the wave's last piece -- from the file.
__device__ inline void wave_masks(const FileView& fv, uint64_t wbase, uint32_t (&m)[kDetQ]) {
  const uint32_t l = threadIdx.x & 63u;
  uint4 v[kDetQ];
#pragma unroll
  for (uint32_t q = 0; q < kDetQ; ++q) v[q] = fv.ld16(wbase + 16ull * (64u * q + l));
  const uint32_t tail = fv.ld4(wbase + kDetWave);  // (the same address in every lane)
#pragma unroll
  for (uint32_t q = 0; q < kDetQ; ++q) {
    const uint32_t nxt = (uint32_t)__shfl_down((int)v[q].x, 1, 64);
    const uint32_t first =
        q + 1 < kDetQ ? (uint32_t)__builtin_amdgcn_readfirstlane((int)v[(q + 1) % kDetQ].x) : tail;  // (lane 0's)
    m[q] = piece_mask(v[q], l == 63u ? first : nxt);
  }
}

// Pass 1: candidates per wave.
__global__ __launch_bounds__(kThreads) void arc_count_kernel(FileView fv, uint64_t nwave, uint64_t* __restrict__ wcnt) {
  const uint64_t gw = (uint64_t)blockIdx.x * kDetWavesPerBlock + (threadIdx.x >> 6);
  if (gw >= nwave) return;  // (the whole wave)
  uint32_t m[kDetQ];
  wave_masks(fv, gw * kDetWave, m);
  uint32_t c = 0;
#pragma unroll
  for (uint32_t q = 0; q < kDetQ; ++q) c += (uint32_t)__builtin_popcount(m[q]);
  // at most 4 candidates per piece (they lie 5 bytes apart or more): c <= 16
  uint32_t tot = 0;
#pragma unroll
  for (uint32_t b = 0; b < 5; ++b) tot += (uint32_t)__builtin_popcountll(__ballot((c >> b) & 1u)) << b;
  if ((threadIdx.x & 63u) == 0) wcnt[gw] = tot;
}

// Where the host loop goes after the record whose header is at off: the offset of the next
// header, or kNoNext when the loop ends there (k2h_archive.cc:41-67: no whole header at off,
// the five lengths overflow, total > size - off, or no whole header fits at off + total).
constexpr uint64_t kNoNext = ~0ull;
__device__ inline uint64_t next_offset(const FileView& fv, uint64_t off) {
  if (fv.size < kScom || off > fv.size - kScom) return kNoNext;
  uint64_t total = kScom;
  bool overflow = false;
  // the five lengths, bytes [24, 64) of the header, in three loads (a lane's loads lie a
  // record apart from its neighbours': each one costs the wave 64 lines, whatever its width)
  const uint64_t l0 = fv.ld8(off + 24);
  const uint4 a = fv.ld16(off + 32), b = fv.ld16(off + 48);
  const uint64_t len[5] = {l0, pack2(a.x, a.y), pack2(a.z, a.w), pack2(b.x, b.y), pack2(b.z, b.w)};
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    if (total + len[j] < total) overflow = true;
    total += len[j];
  }
  if (overflow || total > fv.size - off) return kNoNext;
  const uint64_t t = off + total;  // <= size
  return t <= fv.size - kScom ? t : kNoNext;
}

// Pass 2: the same masks again, each candidate's offset written at its rank, and with it the
// offset its record leads to (the header's lengths are read here, where the detect pass has
// just brought their lines in; round 7: the link kernel read them again, 318 us of a 2.7 ms
// call).  woff is the exclusive scan of the wave counts (woff[nwave]: the total).  With more
// candidates than ccap nothing is written (the host retries with room for all).
__global__ __launch_bounds__(kThreads) void arc_write_kernel(FileView fv, uint64_t nwave,
                                                              const uint64_t* __restrict__ woff, uint64_t ccap,
                                                              uint64_t* __restrict__ cand,
                                                              uint64_t* __restrict__ nxtoff, uint64_t* host_flags) {
  const uint64_t gw = (uint64_t)blockIdx.x * kDetWavesPerBlock + (threadIdx.x >> 6);
  const uint64_t total = woff[nwave];
  if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(host_flags + 1, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (gw >= nwave || total > ccap) return;
  uint32_t m[kDetQ];
  const uint64_t wbase = gw * kDetWave;
  wave_masks(fv, wbase, m);
  uint64_t at = woff[gw];
  const uint32_t l = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t q = 0; q < kDetQ; ++q) {
    const uint32_t c = (uint32_t)__builtin_popcount(m[q]);
    if (__ballot(c != 0) == 0) continue;  // (wave-uniform)
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (uint32_t b = 0; b < 3; ++b) {  // c <= 4
      const uint64_t bb = __ballot((c >> b) & 1u);
      pre += lanes_below(bb) << b;
      tot += (uint32_t)__builtin_popcountll(bb) << b;
    }
    uint64_t r = at + pre;
    uint32_t mm = m[q];
    const uint64_t o = wbase + 16ull * (64u * q + l);
    while (mm) {
      const uint32_t k = (uint32_t)__builtin_ctz(mm);
      mm &= mm - 1;
      if (r < ccap) {
        cand[r] = o + k;
        nxtoff[r] = next_offset(fv, o + k);
      }
      ++r;
    }
    at += tot;
  }
}

// ---------------------------------------------------------------------------
// Headers.
// ---------------------------------------------------------------------------
// The record whose header is at off (a whole header fits: off <= size - 104), exactly as
// k2h_amd_archive_scan reports it (k2h_archive.cc:41-67): offsets in wrapping 64-bit
// arithmetic, TRUNCATED for a non-empty segment that does not lie in the file, BAD_TYPE
// before TRUNCATED.  total = 104 + the five lengths; stop: the sum overflowed, or the next
// header would start beyond the file.
struct Header {
  k2h_amd_archive_rec r;
  uint64_t total;
  bool stop;
};
__device__ inline Header read_header(const FileView& fv, uint64_t off) {
  Header h;
  const uint64_t size = fv.size;
  uint64_t len[5], pos[5];
  // bytes [16, 104) of the header in six loads, not eleven (see next_offset)
  const uint4 a = fv.ld16(off + 16), b = fv.ld16(off + 32), c = fv.ld16(off + 48), d = fv.ld16(off + 64),
              e = fv.ld16(off + 80);
  h.r.type = (int64_t)pack2(a.x, a.y);
  len[0] = pack2(a.z, a.w), len[1] = pack2(b.x, b.y), len[2] = pack2(b.z, b.w);
  len[3] = pack2(c.x, c.y), len[4] = pack2(c.z, c.w);
  pos[0] = pack2(d.x, d.y), pos[1] = pack2(d.z, d.w), pos[2] = pack2(e.x, e.y), pos[3] = pack2(e.z, e.w);
  pos[4] = fv.ld8(off + 96);
  h.r.offset = off;
  int32_t status = (h.r.type < 0 || h.r.type > 6) ? K2H_AMD_ARCHIVE_BAD_TYPE : 0;
  uint64_t total = kScom;
  bool overflow = false;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    if (len[j] > size || pos[j] > size || off + pos[j] + len[j] > size) {
      if (len[j] && !status) status = K2H_AMD_ARCHIVE_TRUNCATED;
    }
    if (total + len[j] < total) overflow = true;
    total += len[j];
  }
  h.r.key_off = off + pos[0], h.r.key_len = len[0];
  h.r.val_off = off + pos[1], h.r.val_len = len[1];
  h.r.skey_off = off + pos[2], h.r.skey_len = len[2];
  h.r.attrs_off = off + pos[3], h.r.attrs_len = len[3];
  h.r.exdata_off = off + pos[4], h.r.exdata_len = len[4];
  h.r.status = status;
  h.r.reserved = 0;
  h.total = total;
  h.stop = overflow || total > size - off;
  return h;
}

// ---------------------------------------------------------------------------
// Link and resolve.
// ---------------------------------------------------------------------------
// next[i]: the candidate whose header follows candidate i's record, kEnd when the host loop
// ends after record i, kMiss when a header fits at the next offset but no prefix starts
// there.  Candidates are sorted, and the next offset lies after this one: the search is over
// (i, n).  Lane 0 also seeds the chain: candidate 0 is reached when it is at offset 0.
__global__ __launch_bounds__(kThreads) void arc_link_kernel(const uint64_t* __restrict__ woff, uint64_t nwave,
                                                             uint64_t ccap, const uint64_t* __restrict__ cand,
                                                             const uint64_t* __restrict__ nxtoff,
                                                             uint32_t* __restrict__ next, uint32_t* reach) {
  const uint64_t n = woff[nwave];
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n > ccap || i >= n) return;
  if (i == 0 && cand[0] == 0) reach[0] = 1u;
  const uint64_t t = nxtoff[i];
  uint32_t nx = kEnd;
  if (t != kNoNext) {
    nx = kMiss;
    if (i + 1 < n && cand[i + 1] == t) {  // no decoy in between: the usual case
      nx = (uint32_t)(i + 1);
    } else {
      uint64_t lo = i + 1, hi = n;  // first index in [lo, hi) with cand >= t
      while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (cand[mid] < t) lo = mid + 1;
        else hi = mid;
      }
      if (lo < n && cand[lo] == t) nx = (uint32_t)lo;
    }
  }
  next[i] = nx;
}

// One doubling round: a reached candidate reaches the one its jump points at, and every
// jump becomes the jump of its target (jin -> jout: the rounds ping-pong).  After round r
// the candidates within 2^r hops of candidate 0 are reached.  reach is written while other
// lanes read it: a lane that sees this round's mark only marks a candidate of the same chain.
__global__ __launch_bounds__(kThreads) void arc_jump_kernel(const uint64_t* __restrict__ woff, uint64_t nwave,
                                                             uint64_t ccap, const uint32_t* __restrict__ jin,
                                                             uint32_t* __restrict__ jout, uint32_t* reach) {
  const uint64_t n = woff[nwave];
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n > ccap || i >= n) return;
  const uint32_t j = jin[i];
  uint32_t out = j;
  if (j < kMiss && j < n) {
    if (reach[i]) reach[j] = 1u;
    out = jin[j];
  }
  jout[i] = out;
}

// ---------------------------------------------------------------------------
// Hash.
// ---------------------------------------------------------------------------
// h1 / h2 of the bytes [off, off + len) hashed as stored (k2h_hash / k2h_second_hash,
// lib/k2hashfunc.cc:62-90): an empty key gives 0, the second hash covers all but the last
// byte of a key longer than one byte.  A range that does not lie in the file gives 0 -- the
// check hash_cstr_checked makes for the import scanner -- and every load below goes through
// FileView again.  The key is read as ceil(len / 16) chunks that end at its last byte; the
// first starts p bytes early with those bytes zeroed and the state at seed * P^-p.
__device__ inline void hash_raw_checked(const FileView& fv, uint64_t off, uint64_t len, const SpadTable& sp,
                                        uint64_t& h1, uint64_t& h2) {
  h1 = h2 = 0;
  if (!fv.has(off, len) || len == 0) return;
  const uint64_t k = (len + 15) / 16;
  const uint32_t p = (uint32_t)(16 * k - len);
  // (a key that starts within 15 bytes of the file's start has nothing before it to read)
  const uint4 c0 =
      off >= p ? fv.ld16(off - p) : chunk0_from_bytes(p, [fv, off](uint32_t i) { return fv.byte(off + i); });
  const uint64_t at = off - p;  // (wraps when off < p; chunks q >= 1 start at at + 16 q >= off)
  end_aligned_walk(k, p, mask_lead_sel(c0, p), sp.v, [fv, at](uint64_t q) { return fv.ld16(at + 16 * q); }, h1, h2);
  if (len == 1) h2 = h1;  // lib/k2hashfunc.cc:83
}

struct HashOut {
  uint64_t *h1, *h2, *new_h1, *new_h2;
};

// A record's hashes: its key's, and for SCOM_RENAME (type 6) its new key's (exdata); zeros
// for a record whose status is not 0.
__device__ inline void hash_record(const FileView& fv, const k2h_amd_archive_rec& r, const SpadTable& sp,
                                   const HashOut& out, uint64_t i) {
  uint64_t a = 0, b = 0, c = 0, d = 0;
  if (r.status == 0) {
    hash_raw_checked(fv, r.key_off, r.key_len, sp, a, b);
    if ((out.new_h1 || out.new_h2) && r.type == 6) hash_raw_checked(fv, r.exdata_off, r.exdata_len, sp, c, d);
  }
  out.h1[i] = a;
  if (out.h2) out.h2[i] = b;
  if (out.new_h1) out.new_h1[i] = c;
  if (out.new_h2) out.new_h2[i] = d;
}

__global__ __launch_bounds__(kThreads) void arc_hash_kernel(FileView fv, const k2h_amd_archive_rec* __restrict__ recs,
                                                             uint64_t n, SpadTable sp, HashOut out) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  hash_record(fv, recs[i], sp, out, i);
}

// ---------------------------------------------------------------------------
// Emit.
// ---------------------------------------------------------------------------
// Reached candidate i's record goes to rank[i] (the exclusive scan of reach), within cap.
// The reached lanes of a wave hold consecutive ranks, so the wave's records are one
// contiguous run of the output: they are staged in LDS and written as consecutive 8-byte
// words (round 7: each lane storing its own 104 bytes at a 104-byte stride made the emit
// kernel 1.0 ms of a 2.7 ms call).  The one reached candidate whose next is no candidate is
// the chain's last: it knows the record count, and for kMiss appends the NO_MAGIC record of
// the header its record runs into.  A file whose offset 0 holds no prefix is that one record
// alone.
constexpr uint32_t kRecWords = sizeof(k2h_amd_archive_rec) / 8;
static_assert(kRecWords * 8 == sizeof(k2h_amd_archive_rec) && kRecWords == 13, "a record is 13 words");
template <bool HASH>
__global__ __launch_bounds__(kThreads) void arc_emit_kernel(FileView fv, const uint64_t* __restrict__ woff,
                                                             uint64_t nwave, uint64_t ccap,
                                                             const uint64_t* __restrict__ cand,
                                                             const uint32_t* __restrict__ next,
                                                             const uint32_t* __restrict__ reach,
                                                             const uint32_t* __restrict__ rank,
                                                             k2h_amd_archive_rec* __restrict__ recs, uint64_t cap,
                                                             SpadTable sp, HashOut out, uint64_t* host_flags) {
  __shared__ uint64_t s_rec[kThreads / 64][64 * kRecWords];
  const uint64_t n = woff[nwave];
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n > ccap) return;  // (every thread)
  // the rare records outside the staged run: one lane, its own stores
  auto put = [&](uint64_t at, const k2h_amd_archive_rec& r) {
    if (!recs || at >= cap) return;
    recs[at] = r;
    if constexpr (HASH) hash_record(fv, r, sp, out, at);
  };
  const bool nostart = n == 0 || cand[0] != 0;
  if (i == 0 && nostart) {  // (size >= 104: the caller checked)
    Header h = read_header(fv, 0);
    h.r.status = K2H_AMD_ARCHIVE_NO_MAGIC;
    put(0, h.r);
    __hip_atomic_store(host_flags, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const bool live = !nostart && i < n && reach[i] != 0;
  const uint64_t at = live ? rank[i] : 0;
  // the wave's run: reached lanes in lane order hold ranks first, first + 1, ...
  const uint64_t lanes = __ballot(live);
  const uint32_t slot = lanes_below(lanes), cnt = (uint32_t)__builtin_popcountll(lanes);
  uint64_t* stage = s_rec[threadIdx.x >> 6];
  if (live) {
    const uint64_t off = cand[i];
    const Header h = read_header(fv, off);  // (a reached candidate holds a whole header)
    if (recs) *reinterpret_cast<k2h_amd_archive_rec*>(stage + slot * kRecWords) = h.r;
    if constexpr (HASH)
      if (recs && at < cap) hash_record(fv, h.r, sp, out, at);
    const uint32_t nx = next[i];
    if (nx >= kMiss) {
      uint64_t count = at + 1;
      if (nx == kMiss) {
        Header m = read_header(fv, off + h.total);
        m.r.status = K2H_AMD_ARCHIVE_NO_MAGIC;
        put(count, m.r);
        ++count;
      }
      __hip_atomic_store(host_flags, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  __syncthreads();  // (every thread of the block arrives: no return above but the uniform one)
  if (!recs || cnt == 0) return;
  // the run's first rank: that of the wave's first reached lane
  const uint32_t lane0 = (uint32_t)__builtin_ctzll(lanes);
  const uint64_t first = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(at >> 32), (int)lane0, 64) << 32) |
                         (uint32_t)__shfl((int)(uint32_t)at, (int)lane0, 64);
  uint64_t* dst = reinterpret_cast<uint64_t*>(recs) + first * kRecWords;
  const uint32_t words = cnt * kRecWords;
  for (uint32_t w = threadIdx.x & 63u; w < words; w += 64u)
    if (first + w / kRecWords < cap) dst[w] = stage[w];
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// The scan's temporaries (k2h_scratch.h), as the import scanner keeps them: freed at the end of
// a call that needed more than kScratchKeep, and neither an event nor a wait, since the call
// synchronises its stream before it unlocks.  Per candidate: its offset and its record's next
// offset (16 B), next and the two jump arrays (12 B), reach and rank (8 B); per 4 KiB wave of
// the file 16 B of counts.  The record count comes back through mapped pinned host memory.
struct ArcState {
  DeviceScratch buf;
  uint64_t* hflags = nullptr;    // mapped pinned host memory: [0] record count, [1] candidates
  uint64_t* hflags_d = nullptr;  // ... and its device address
};
PerDevice<ArcState> g_arc;

struct ArcCols {
  uint64_t *wcnt, *woff;
  void* tmp;
  uint64_t *cand, *nxtoff;
  uint32_t *next, *ja, *jb, *reach, *rank;
  size_t total;
};

}  // namespace

// Returns K2H_AMD_* codes (the HIP error, if any, in *herr); synchronises the stream.
int launch_archive_scan(const void* file, uint64_t size, k2h_amd_archive_rec* recs, uint64_t cap, uint64_t* count,
                        hipStream_t stream, hipError_t* herr, const ArchiveHashOut* hash, uint64_t seed) {
  *herr = hipSuccess;
  *count = 0;
  if (size < kScom) return K2H_AMD_OK;  // no whole header: no records, no device work
  const FileView fv{(const uint8_t*)file, size};
  const uint64_t nwave = (size + kDetWave - 1) / kDetWave;
  const uint64_t nblk = (nwave + kDetWavesPerBlock - 1) / kDetWavesPerBlock;
  if (nblk > 0x7FFFFFFFull) return K2H_AMD_EINVAL;
  FirstError tr;
  ArcState* const scp = g_arc.current(tr);
  if (!tr.ok()) {
    *herr = tr.e;
    return K2H_AMD_EHIP;
  }
  // the chain has at most size / 104 records; 2^rounds hops cover it
  uint32_t rounds = 0;
  while ((size / kScom) >> rounds) ++rounds;
  ArcState& sc = *scp;
  std::lock_guard<std::mutex> lk(sc.buf.mu);
  if (!sc.hflags) {
    void* hp = nullptr;
    tr(hipHostMalloc(&hp, 64, hipHostMallocMapped));
    void* dp = nullptr;
    if (tr.ok()) tr(hipHostGetDevicePointer(&dp, hp, 0));
    if (tr.ok()) {
      sc.hflags = (uint64_t*)hp;
      sc.hflags_d = (uint64_t*)dp;
    } else if (hp) {
      (void)hipHostFree(hp);
    }
  }
  const SpadTable sp = make_spad(seed);
  HashOut ho{nullptr, nullptr, nullptr, nullptr};
  if (hash) ho = HashOut{hash->h1, hash->h2, hash->new_h1, hash->new_h2};
  // A file without decoys has one candidate per record, at most size / 104: room for that
  // many first; a file with more reports its count and is scanned again with room for all.
  uint64_t ccap = size / kScom + 1;
  uint64_t nrec = 0;
  int rc = K2H_AMD_OK;
  for (int attempt = 0; attempt < 2 && tr.ok(); ++attempt) {
    size_t tmp1 = 0, tmp2 = 0;
    tr(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp1, (uint64_t*)nullptr, (uint64_t*)nullptr, nwave + 1, stream));
    tr(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp2, (uint32_t*)nullptr, (uint32_t*)nullptr, ccap + 1, stream));
    if (!tr.ok()) break;
    auto layout = [&](void* base) {
      Carver c(base);
      ArcCols k;
      k.wcnt = c.take<uint64_t>(nwave + 1);
      k.woff = c.take<uint64_t>(nwave + 1);
      k.tmp = c.bytes(tmp1 > tmp2 ? tmp1 : tmp2);
      k.cand = c.take<uint64_t>(ccap);
      k.nxtoff = c.take<uint64_t>(ccap);
      k.next = c.take<uint32_t>(ccap);
      k.ja = c.take<uint32_t>(ccap);
      k.jb = c.take<uint32_t>(ccap);
      k.reach = c.take<uint32_t>(ccap + 1);
      k.rank = c.take<uint32_t>(ccap + 1);
      k.total = c.total();
      return k;
    };
    hipError_t ge = hipSuccess;
    if (sc.buf.grow(layout(nullptr).total, &ge) == K2H_AMD_ENOMEM) {
      rc = K2H_AMD_ENOMEM;
      break;
    }
    tr(ge);
    if (!tr.ok()) break;
    sc.hflags[0] = 0;  // the previous call on this device has synchronised (the lock)
    sc.hflags[1] = 0;
    const ArcCols k = layout(sc.buf.p);
    uint32_t* jbuf[2] = {k.ja, k.jb};
    const unsigned gc = blocks_for(ccap);
    tr(hipMemsetAsync(k.wcnt + nwave, 0, 8, stream));
    tr(hipMemsetAsync(k.reach, 0, (ccap + 1) * 4, stream));
    if (tr.ok()) {
      arc_count_kernel<<<(unsigned)nblk, kThreads, 0, stream>>>(fv, nwave, k.wcnt);
      tr(hipGetLastError());
    }
    if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(k.tmp, tmp1, k.wcnt, k.woff, nwave + 1, stream));
    if (tr.ok()) {
      arc_write_kernel<<<(unsigned)nblk, kThreads, 0, stream>>>(fv, nwave, k.woff, ccap, k.cand, k.nxtoff, sc.hflags_d);
      tr(hipGetLastError());
    }
    if (tr.ok()) {
      arc_link_kernel<<<gc, kThreads, 0, stream>>>(k.woff, nwave, ccap, k.cand, k.nxtoff, k.next, k.reach);
      tr(hipGetLastError());
    }
    const uint32_t* jin = k.next;
    for (uint32_t r = 0; r < rounds && tr.ok(); ++r) {
      arc_jump_kernel<<<gc, kThreads, 0, stream>>>(k.woff, nwave, ccap, jin, jbuf[r & 1], k.reach);
      tr(hipGetLastError());
      jin = jbuf[r & 1];
    }
    if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(k.tmp, tmp2, k.reach, k.rank, ccap + 1, stream));
    if (tr.ok()) {
      if (hash)
        arc_emit_kernel<true><<<gc, kThreads, 0, stream>>>(fv, k.woff, nwave, ccap, k.cand, k.next, k.reach, k.rank,
                                                           recs, cap, sp, ho, sc.hflags_d);
      else
        arc_emit_kernel<false><<<gc, kThreads, 0, stream>>>(fv, k.woff, nwave, ccap, k.cand, k.next, k.reach, k.rank,
                                                            recs, cap, sp, ho, sc.hflags_d);
      tr(hipGetLastError());
    }
    tr(hipStreamSynchronize(stream));
    if (!tr.ok()) break;
    const uint64_t ncand = __atomic_load_n(&sc.hflags[1], __ATOMIC_ACQUIRE);
    if (ncand <= ccap) {
      nrec = __atomic_load_n(&sc.hflags[0], __ATOMIC_ACQUIRE);
      break;
    }
    if (ncand > kMaxCand || attempt == 1) {  // candidate indices are 32-bit
      rc = K2H_AMD_EINVAL;
      break;
    }
    ccap = ncand;
  }
  sc.buf.release_above(kScratchKeep);
  *herr = tr.e;
  if (!tr.ok()) return tr.e == hipErrorOutOfMemory ? K2H_AMD_ENOMEM : K2H_AMD_EHIP;
  if (rc != K2H_AMD_OK) return rc;
  *count = nrec;
  return (recs && nrec > cap) ? K2H_AMD_EINVAL : K2H_AMD_OK;
}

hipError_t launch_archive_prehash(const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n,
                                  uint64_t seed, const ArchiveHashOut& hash, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const HashOut ho{hash.h1, hash.h2, hash.new_h1, hash.new_h2};
  arc_hash_kernel<<<blocks_for(n), kThreads, 0, stream>>>(FileView{(const uint8_t*)file, size}, recs, n,
                                                         make_spad(seed), ho);
  return hipGetLastError();
}

}  // namespace k2h
