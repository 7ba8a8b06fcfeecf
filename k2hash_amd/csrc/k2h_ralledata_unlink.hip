// k2hash_amd -- RALLEDATA consumer side: subkey names unlinked from a blob stream in device
// memory (include/k2hash_amd.h section 4b'''''''): the first half of K2HShm::Remove(key, subkey)
// (lib/k2hshm.cc:2567-2667 -- K2HSubKeys::erase, Serialize, the subkeys page replaced), applied to
// the blobs before they are fed.  The stream is packed as k2h_amd_ralledata_select packs it,
// except that a blob one of whose edges is dropped has its list serialized again without the
// dropped names and is written in GetElementToBinary's layout (lib/k2hshmdirect.cc:59-89).
//
// The scheme of k2h_ralledata_archive.hip: output sizes differ per blob, so the placement is a
// scan.  All on the caller's stream:
//   size     one lane per blob: keep byte and span (select's test).  With a drop mask, every
//            emitted blob with PART and without BAD in sk_flags has its header judged by
//            classify() and its segment walked by the strict rule (k2h_ralle_subkeys.h), the
//            drop byte of every edge read on the way; nothing the caller passed about it is
//            trusted: a header that is no participant's, a BAD walk, an edge count other than
//            edge_off[i + 1] - edge_off[i] or an edge range outside [0, E] leave the blob as it
//            is (a mismatch).  Leaves the blob's output size, a kept flag and its
//            K2H_AMD_UNLINK_* byte; the seven counts go into counter lines.  This is the count
//            pass of k2h_ralledata_subkeys.hip over again and starts from its launch shape
//            (kWalkLdsBytes, two waves per SIMD); without a drop mask nothing of the stream is
//            read and the kernel runs at full occupancy.
//   scan     PlaceRank (k2h_sort_stage.h): the sizes into places, the kept flags into ranks.  The counts
//            come back to the host (the one synchronisation).
//   copy     the select copy kernel's scheme over the places (k2h_ralle_copy.h): a tile of
//            256 blobs writes its destination span as aligned 16-byte pieces, one unaligned
//            load each where the source is contiguous.  A rewritten blob supplies no byte here: a piece wholly
//            inside one is skipped, a piece it shares with its neighbours is stored with
//            filler in the rewritten blob's places.
//   rewrite  launched only when a blob is rewritten, after the copy on the same stream, so its
//            bytes land over the filler: 8 lanes per blob, straight from HBM (group_copy of
//            k2h_ralle_pieces.h, the direct form of the archive builder).  The header is built
//            in registers; key and value are copied from wherever their positions put them; the
//            eight lanes walk the list together and copy every maximal run of consecutive kept
//            entries (length words and names lie contiguous in the source) as one range; the
//            count word is synthesised; the attrs follow.  The same bytes result wherever the
//            segments lay in the input: permuted, overlapping, with gaps, of any size.
//
// Why two build kernels.  The list walk is a chain of dependent loads with a drop byte per
// entry; inside the copy kernel it would hold a tile's 256 lanes for the longest list of the
// tile and add its registers to every tile's, rewritten blob or not.  Rewritten blobs are the
// rare case (one Remove touches one parent), so they get a pass of their own and the copy keeps
// the select kernel's shape and cost; with no drop set the call runs no rewrite kernel at all.
//
// Reads.  No byte of `blobs` outside [0, size): the copy loads exact source bytes of emitted
// blobs; the walk's loads lie wholly inside the segment, which classify keeps inside the blob;
// group_copy touches exact bytes.  drop is read only at e in [edge_off[i], edge_off[i + 1]) of a
// blob whose range lies inside [0, edge_off[n]].  Nothing of a blob that is not emitted is
// read; of an emitted blob without PART, or with BAD, in sk_flags nothing is interpreted.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_ralle_header.h"
#include "k2h_ralle_ident.h"
#include "k2h_ralle_copy.h"
#include "k2h_ralle_pieces.h"
#include "k2h_ralle_subkeys.h"

namespace k2h {
namespace {

constexpr int kUlBlobs = 256;        // size / copy: blobs per 256-thread block, one per thread
constexpr int kUlGroup = 8;          // rewrite: lanes per blob
constexpr int kUlTabPieces = 4096;   // copy: as kSelTabPieces of the select copy

typedef uint32_t u32x2_ua __attribute__((ext_vector_type(2), aligned(1)));

struct UlIn {
  const uint8_t* blobs;
  uint64_t size;
  const uint64_t* off;
  const uint8_t* keep;
  const uint8_t* sk_flags;
  const uint64_t* edge_off;
  const uint8_t* drop;
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d; d >>= 1) v += __shfl_down((unsigned long long)v, d);
  return v;  // in lane 0
}

// One add per wave and word, neighbouring waves on different lines.
__device__ __forceinline__ void ul_count(unsigned long long* counter, int word, uint64_t v) {
  const uint64_t s = wave_sum(v);
  if ((threadIdx.x & 63u) == 0 && s) {
    const uint32_t wave = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    atomicAdd(counter + 8 * (wave % kCounterLines) + word, (unsigned long long)s);
  }
}

// sizes[i] = blob i's bytes in the output (0: not emitted), kept[i] = 1 for an emitted blob,
// chg[i] (and changed[i], when given) its K2H_AMD_UNLINK_* bits; entry n of sizes and kept is 0.
__global__ __launch_bounds__(kUlBlobs) void unlink_size_kernel(UlIn s, uint64_t n, uint64_t* __restrict__ sizes,
                                                               uint32_t* __restrict__ kept, uint8_t* __restrict__ chg,
                                                               uint8_t* __restrict__ changed,
                                                               unsigned long long* __restrict__ counter) {
  const uint64_t i = (uint64_t)blockIdx.x * kUlBlobs + threadIdx.x;
  uint64_t v = 0, dropped = 0;
  uint32_t k = 0, ch = 0;
  bool mismatch = false;
  if (i < n && (!s.keep || s.keep[i])) {
    const uint64_t b = s.off[i], e = s.off[i + 1];
    if (e >= b && e <= s.size) {
      k = 1;
      v = e - b;
      const uint32_t fl = s.drop ? s.sk_flags[i] : 0u;
      if ((fl & K2H_AMD_SKEY_PART) && !(fl & K2H_AMD_SKEY_BAD)) {
        const uint64_t e0 = s.edge_off[i], e1 = s.edge_off[i + 1], cnt = e1 - e0;
        uint64_t f[10], edges = 0, names = 0, bytes = 0, dr = 0;
        bool ok = e0 <= e1 && e1 <= s.edge_off[n] && v >= (uint64_t)kHdr;
        if (ok) {
          load_fields(s.blobs + b, f);
          ok = classify(f, v) == K2H_AMD_RALLE_OK;
        }
        if (ok && f[4]) {
          const uint8_t* const drop = s.drop + e0;
          ok = walk_subkeys(s.blobs + b + f[8], f[4], edges, [&](uint64_t x, uint64_t, uint64_t len) {
            if (x < cnt && drop[x]) {
              ++dr;
            } else {
              ++names;
              bytes += 8 + len;
            }
          });
        }
        if (!ok || edges != cnt) {
          mismatch = true;
        } else if (dr) {
          v = (uint64_t)kHdr + f[2] + f[3] + (names ? 8 + bytes : 0) + f[5];
          ch = K2H_AMD_UNLINK_REWRITTEN;
          if (!names) ch |= K2H_AMD_UNLINK_EMPTIED;
          if (!names && !f[3] && !f[5]) ch |= K2H_AMD_UNLINK_KEY_ONLY;
          dropped = dr;
        }
      }
    }
  }
  if (i <= n) {
    sizes[i] = v;
    kept[i] = k;
  }
  if (i < n) {
    chg[i] = (uint8_t)ch;
    if (changed) changed[i] = (uint8_t)ch;
  }
  ul_count(counter, 0, k);
  ul_count(counter, 1, v);
  ul_count(counter, 2, ch ? 1 : 0);
  ul_count(counter, 3, dropped);
  ul_count(counter, 4, (ch & K2H_AMD_UNLINK_EMPTIED) ? 1 : 0);
  ul_count(counter, 5, (ch & K2H_AMD_UNLINK_KEY_ONLY) ? 1 : 0);
  ul_count(counter, 6, mismatch ? 1 : 0);
}

// One rewritten blob by a group of kUlGroup lanes, in GetElementToBinary's layout.  The size
// kernel judged the blob (header, walk, edge count); nothing is judged again.
// 8 waves per SIMD: at most 64 VGPRs, no scratch.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void unlink_rewrite_kernel(
    UlIn s, uint64_t n, const uint64_t* __restrict__ place, const uint8_t* __restrict__ chg, uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * (256 / kUlGroup) + threadIdx.x / kUlGroup;
  const uint32_t q = threadIdx.x % kUlGroup;
  if (i >= n || !(chg[i] & K2H_AMD_UNLINK_REWRITTEN)) return;
  const uint8_t* const b = s.blobs + s.off[i];
  uint64_t f[10];
  load_fields(b, f);
  const uint64_t at = place[i];
  const uint64_t sk = place[i + 1] - at - (uint64_t)kHdr - f[2] - f[3] - f[5];  // the new list's length
  uint8_t* const r = out + at;
  if (q < 5) {
    uint64_t w0, w1;
    switch (q) {
      case 0: w0 = f[0], w1 = f[1]; break;
      case 1: w0 = f[2], w1 = f[3]; break;
      case 2: w0 = sk, w1 = f[5]; break;
      case 3: w0 = kHdr, w1 = kHdr + f[2]; break;
      default: w0 = kHdr + f[2] + f[3], w1 = kHdr + f[2] + f[3] + sk; break;
    }
    *reinterpret_cast<u32x4_ua*>(r + 16 * q) = u32x4_ua{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
  }
  uint8_t* to = r + kHdr;
  if (f[2]) group_copy<kUlGroup>(to, b + f[6], f[2], q);  // the pos of a length-0 segment is ignored
  to += f[2];
  if (f[3]) group_copy<kUlGroup>(to, b + f[7], f[3], q);
  to += f[3];
  if (f[5]) group_copy<kUlGroup>(to + sk, b + f[9], f[5], q);
  if (!sk) return;
  // the group's lanes walk the list together; a run = consecutive kept entries, S[run_at, + run_len)
  const uint8_t* const S = b + f[8];
  const uint64_t e0 = s.edge_off[i], cnt = s.edge_off[i + 1] - e0;
  const uint8_t* const drop = s.drop + e0;
  uint64_t run_at = 0, run_len = 0, names = 0, edges;
  uint8_t* w = to + 8;
  walk_subkeys(S, f[4], edges, [&](uint64_t x, uint64_t pos, uint64_t len) {
    if (x < cnt && drop[x]) return;
    ++names;
    if (run_at + run_len == pos - 8) {  // (never for an empty run: pos >= 16)
      run_len += 8 + len;
      return;
    }
    if (run_len) group_copy<kUlGroup>(w, S + run_at, run_len, q);
    w += run_len;
    run_at = pos - 8;
    run_len = 8 + len;
  });
  if (run_len) group_copy<kUlGroup>(w, S + run_at, run_len, q);
  if (q == 0) *reinterpret_cast<u32x2_ua*>(to) = u32x2_ua{(uint32_t)names, (uint32_t)(names >> 32)};
}

__global__ __launch_bounds__(256) void subkeys_drop_mask_kernel(const uint64_t* __restrict__ child, uint64_t edges,
                                                                const uint8_t* __restrict__ gone, uint64_t n,
                                                                uint32_t dangling, uint8_t* __restrict__ drop) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= edges) return;
  const uint64_t c = child[e];
  drop[e] = c == ~0ull ? (uint8_t)dangling : (uint8_t)(gone && c < n && gone[c] != 0);
}

// The call's temporaries (k2h_scratch.h) and the pinned lines the counts land in (seven words in
// each).
struct UlScratch : DeviceScratch {
  void* pinned = nullptr;
};
PerDevice<UlScratch> g_ul;

struct UlCols {
  uint64_t* place;
  uint32_t* rank;
  uint8_t* chg;
  unsigned long long* counter;
  void* tmp;
  size_t total;
};

}  // namespace

// Returns a K2H_AMD_* code (the HIP error, if any, in *herr).  1 <= n <= 2^32 - 2.  Synchronises
// the stream once to return counts.  K2H_AMD_EINVAL: out != NULL and counts[1] > out_cap
// (counts, and changed when given, are filled; out, out_off and index are not written).
int launch_ralledata_unlink(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                            const uint8_t* keep, const uint8_t* sk_flags, const uint64_t* edge_off,
                            const uint8_t* drop, void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* index,
                            uint8_t* changed, uint64_t* counts, hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  FirstError tr;
  auto done = [&](int rc) {
    *herr = tr.e;
    return !tr.ok() ? K2H_AMD_EHIP : rc;
  };
  UlScratch* const scp = g_ul.current(tr);
  PlaceRank<> pr;
  pr.measure(tr, n, stream);
  if (!tr.ok()) return done(K2H_AMD_OK);
  UlScratch& sc = *scp;
  std::lock_guard<std::mutex> lk(sc.mu);
  if (!sc.pinned) tr(hipHostMalloc(&sc.pinned, kCounterBytes, hipHostMallocDefault));
  if (!tr.ok()) return done(K2H_AMD_OK);
  unsigned long long* const host = (unsigned long long*)sc.pinned;
  auto layout = [&](void* base) {
    Carver c(base);
    UlCols k;
    k.place = c.take<uint64_t>(n + 1);
    k.rank = c.take<uint32_t>(n + 1);
    k.chg = c.take<uint8_t>(n);
    k.counter = (unsigned long long*)c.bytes(kCounterBytes);
    k.tmp = c.bytes(pr.tmp_bytes());
    k.total = c.total();
    return k;
  };
  if (const int rc = sc.reserve(layout(nullptr).total, stream, herr)) return rc;
  const UlCols k = layout(sc.p);
  const UlIn s{(const uint8_t*)blobs, size, blob_off, keep, sk_flags, edge_off, drop};

  tr(hipMemsetAsync(k.counter, 0, kCounterBytes, stream));
  if (tr.ok()) {
    unlink_size_kernel<<<(unsigned)(n / kUlBlobs + 1), kUlBlobs, drop ? kWalkLdsBytes : 0, stream>>>(
        s, n, k.place, k.rank, k.chg, changed, k.counter);
    tr(hipGetLastError());
  }
  pr.scan(tr, k.tmp, k.place, k.rank, stream);
  if (tr.ok()) tr(hipMemcpyAsync(host, k.counter, kCounterBytes, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(sc.mark_done(stream));
  if (tr.ok()) tr(hipStreamSynchronize(stream));
  if (!tr.ok()) return done(K2H_AMD_OK);
  for (int w = 0; w < 7; ++w) counts[w] = counter_sum(host, w);
  if (!out) return done(K2H_AMD_OK);
  if (counts[1] > out_cap) return done(K2H_AMD_EINVAL);
  ralle_place_copy_kernel<true, kUlBlobs, kUlTabPieces>
      <<<(unsigned)((n + kUlBlobs - 1) / kUlBlobs), kUlBlobs, 0, stream>>>(
      s.blobs, blob_off, n, k.place, k.rank, k.chg, (uint8_t*)out, out_off, index);
  tr(hipGetLastError());
  if (tr.ok() && counts[2]) {
    const uint64_t per = 256 / kUlGroup;
    unlink_rewrite_kernel<<<(unsigned)((n + per - 1) / per), 256, 0, stream>>>(s, n, k.place, k.chg, (uint8_t*)out);
    tr(hipGetLastError());
  }
  if (tr.ok()) tr(sc.mark_done(stream));
  return done(K2H_AMD_OK);
}

hipError_t launch_subkeys_drop_mask(const uint64_t* child, uint64_t edges, const uint8_t* gone, uint64_t n,
                                    int dangling, uint8_t* drop, hipStream_t stream) {
  if (edges == 0) return hipSuccess;
  const uint64_t grid = (edges + 255) / 256;
  if (grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
  subkeys_drop_mask_kernel<<<(unsigned)grid, 256, 0, stream>>>(child, edges, gone, n, dangling ? 1u : 0u, drop);
  return hipGetLastError();
}

}  // namespace k2h
