// k2hash_amd -- internal launch interface between the C-ABI (k2h_batch.cc) and the
// HIP kernels.  Not part of the public ABI (see include/k2hash_amd.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/k2hash_amd.h"

namespace k2h {

// Bucket-index epilogue: where a hash lands in a k2hash table with
// masks (cur_mask, collision_mask) -- the stateless part of K2HShm::GetKIndexPos
// (lib/k2hshm.cc:810-833, with MakeMask / GetMaskBitCount at :78-90) and the collision
// slot `hash & collision_mask` (lib/k2hshm.cc:1093).
//   shifted       = hash >> bitlen(collision_mask)   (shift count taken mod 64, as the
//                                                     x86-64 shr the reference compiles to)
//   KIPtrArrayPos = bitlen(shifted & cur_mask)        (the reference's bitmask loop)
//   KIArrayPos    = shifted & MakeMask(KIPtrArrayPos - 1)   (MakeMask(0) = 0)
// kindex[i] packs KIPtrArrayPos << 58 | KIArrayPos (bitlen(cur_mask) <= 58 checked by the
// ABI); ckindex[i] = hash & collision_mask.  Either output may be null.
// Table state (assigned != null): K2HShm::GetKIndex(hash, false) (lib/k2hshm.cc:882-907)
// -- cur_mask walked down (>>= 1) until the K_INDEX at the masked shifted hash is
// assigned; `assigned` has one bit per K_INDEX entry, entry (p, a) at bit p ? 2^(p-1)+a : 0,
// which is exactly the masked shifted hash v = (hash >> cshift) & m (p = bitlen(v),
// a = v without its top bit).  No assigned entry: the mask-1 probe (what the loop leaves);
// cur_mask 0: kindex = all ones (NULL).  found[i] = 1 when an assigned entry was reached.
struct BucketParams {
  uint64_t cur_mask = 0;
  uint64_t collision_mask = 0;
  uint32_t cshift = 0;
  uint64_t* kindex = nullptr;
  uint64_t* ckindex = nullptr;
  const uint32_t* assigned = nullptr;
  uint8_t* found = nullptr;
};
constexpr int kKindexPosShift = 58;

#ifdef __HIPCC__
// NT: nontemporal stores, for kernels whose lanes write consecutive i (a wave fills
// whole lines); kernels that write in a permuted order (CSR tiles, length-sorted) use
// plain stores so that L2 merges the partial lines before they reach HBM.
template <bool NT = true>
__device__ __forceinline__ void bucket_emit(const BucketParams& bp, uint64_t i, uint64_t h) {
  if (bp.assigned) {  // table state: GetKIndex's walk over the assigned K_INDEX entries
    const uint64_t shifted = h >> (bp.cshift & 63u);
    uint64_t tmp = 0;
    bool hit = false;
    for (uint64_t m = bp.cur_mask; m; m >>= 1) {
      tmp = shifted & m;
      if ((bp.assigned[tmp >> 5] >> (tmp & 31u)) & 1u) {
        hit = true;
        break;
      }
    }
    if (bp.kindex) {
      const uint64_t pos = tmp ? 64u - (uint64_t)__clzll((long long)tmp) : 0u;
      const uint64_t arr = pos ? tmp & ((1ull << (pos - 1)) - 1ull) : 0u;
      const uint64_t v = bp.cur_mask ? (pos << kKindexPosShift) | arr : ~0ull;
      if constexpr (NT) __builtin_nontemporal_store(v, bp.kindex + i);
      else bp.kindex[i] = v;
    }
    if (bp.found) bp.found[i] = hit;
  } else if (bp.kindex) {
    uint64_t shifted = h >> (bp.cshift & 63u);
    uint64_t tmp = shifted & bp.cur_mask;
    uint64_t pos = tmp ? 64u - (uint64_t)__clzll((long long)tmp) : 0u;
    uint64_t arr = pos ? shifted & ((1ull << (pos - 1)) - 1ull) : 0u;
    uint64_t v = (pos << kKindexPosShift) | arr;
    if constexpr (NT) __builtin_nontemporal_store(v, bp.kindex + i);
    else bp.kindex[i] = v;
  }
  if (bp.ckindex) {
    if constexpr (NT) __builtin_nontemporal_store(h & bp.collision_mask, bp.ckindex + i);
    else bp.ckindex[i] = h & bp.collision_mask;
  }
}
#endif

// The launch ladder: the runtime pair (second hash wanted, index epilogue wanted) as the
// kernels' two template booleans.  f is a generic lambda taking two std::bool_constant values.
template <class F>
inline void with_h2_epi(bool h2, bool epi, F&& f) {
  if (epi) {
    if (h2) f(std::true_type{}, std::true_type{});
    else f(std::false_type{}, std::true_type{});
  } else {
    if (h2) f(std::true_type{}, std::false_type{});
    else f(std::false_type{}, std::false_type{});
  }
}

// Standalone epilogue over hashes already in device memory.
hipError_t launch_bucket_index(const uint64_t* h1, uint64_t n, const BucketParams& bp, hipStream_t stream);

// RALLEDATA producer inputs (k2h_ralledata.hip): four CSR streams; a null offsets
// array = that segment is empty for every record.
struct RalleInputs {
  const uint8_t* keys = nullptr;
  const uint64_t* koff = nullptr;
  const uint8_t* vals = nullptr;
  const uint64_t* voff = nullptr;
  const uint8_t* skeys = nullptr;
  const uint64_t* soff = nullptr;
  const uint8_t* attrs = nullptr;
  const uint64_t* aoff = nullptr;
};
hipError_t launch_ralledata(const RalleInputs& in, uint64_t n, uint64_t seed, uint8_t* out, uint64_t* blob_off,
                            hipStream_t stream);

// RALLEDATA consumer side (k2h_ralledata_check.hip).  RalleRoute is k2h_amd_hash_range with
// the two range ends already reduced (lib/k2hshmdirect.cc:118-119): t / o the target / old
// range's start, *_end its end, *_max its modulus; old_on = 0 when old_hash is ~0.
struct RalleRoute {
  uint64_t t = 0, t_end = 0, t_max = 1;
  uint64_t o = 0, o_end = 0, o_max = 1;
  uint32_t old_on = 0;
};
hipError_t launch_ralledata_check(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                                  uint64_t seed, const RalleRoute& route, uint8_t* status, uint8_t* route_out,
                                  uint64_t* h1, uint64_t* h2, hipStream_t stream);
// Returns a K2H_AMD_* code (the HIP error in *herr) and synchronises the stream once.
int launch_ralledata_select(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                            const uint8_t* keep, void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* index,
                            uint64_t* kept, uint64_t* kept_bytes, hipStream_t stream, hipError_t* herr);

// Superseded duplicates of a blob stream (k2h_ralledata_dedup.hip).  Returns a K2H_AMD_* code
// (the HIP error in *herr); synchronises the stream once when dropped != NULL.  1 <= n <= 2^32 - 2.
int launch_ralledata_dedup(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                           const uint8_t* consider, uint8_t* keep, uint64_t* by, uint64_t* dropped, hipStream_t stream,
                           hipError_t* herr);
// The same under the mtime rule; pts is a host pointer, read before the call returns.
int launch_ralledata_dedup_mtime(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                                 const uint8_t* consider, const k2h_amd_timespec* pts, uint8_t* keep, uint64_t* by,
                                 uint64_t* dropped, hipStream_t stream, hipError_t* herr);

// Two streams joined by identity (k2h_ralledata_diff.hip): A the incoming stream, B the held one.
// Returns a K2H_AMD_* code (the HIP error in *herr); synchronises the stream once when
// counts != NULL.  na >= 1, na + nb <= 2^32 - 2; times is a host pointer, read before the return.
int launch_ralledata_diff(const void* a_blobs, uint64_t a_size, const uint64_t* a_off, uint64_t na,
                          const uint8_t* a_consider, const void* b_blobs, uint64_t b_size, const uint64_t* b_off,
                          uint64_t nb, const uint8_t* b_consider, const k2h_amd_diff_times* times, uint8_t* rel,
                          uint64_t* match, uint8_t* seen, uint64_t* counts, hipStream_t stream, hipError_t* herr);

// The subkeys of a stream as edges between its blobs, and what root blobs reach over them
// (k2h_ralledata_subkeys.hip).  Both return a K2H_AMD_* code (the HIP error in *herr);
// 1 <= n <= 2^32 - 2.  _subkeys synchronises the stream once after its count pass and, when
// child != NULL, once more at the end; K2H_AMD_EINVAL with *why = 1: cap < E, 2: n + E >
// 2^32 - 2 (counts and edge_off are filled, child is not written).  _reach synchronises once for
// the start set, once per level run and once at the end.
int launch_ralledata_subkeys(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                             const uint8_t* consider, uint64_t seed, uint8_t* sk_flags, uint64_t* edge_off,
                             uint64_t* rep, uint64_t* child, uint64_t cap, uint64_t* counts, int* why,
                             hipStream_t stream, hipError_t* herr);
int launch_ralledata_reach(const uint64_t* edge_off, const uint64_t* child, const uint64_t* rep, uint64_t n,
                           const uint8_t* roots, uint64_t max_levels, uint8_t* reach, uint64_t* counts,
                           hipStream_t stream, hipError_t* herr);

// Subkey names unlinked from a stream (k2h_ralledata_unlink.hip).  _unlink returns a K2H_AMD_*
// code (the HIP error in *herr), 1 <= n <= 2^32 - 2, and synchronises the stream once;
// K2H_AMD_EINVAL: out != NULL and counts[1] > out_cap (counts and changed are filled).
// _drop_mask is asynchronous on the stream.
int launch_ralledata_unlink(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                            const uint8_t* keep, const uint8_t* sk_flags, const uint64_t* edge_off,
                            const uint8_t* drop, void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* index,
                            uint8_t* changed, uint64_t* counts, hipStream_t stream, hipError_t* herr);
hipError_t launch_subkeys_drop_mask(const uint64_t* child, uint64_t edges, const uint8_t* gone, uint64_t n,
                                    int dangling, uint8_t* drop, hipStream_t stream);

// The mtime and expire of every blob's attrs and the time-window selection
// (k2h_ralledata_times.hip).  Asynchronous on the stream; n >= 1, window may be NULL.
hipError_t launch_ralledata_times(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                                  const uint8_t* consider, const k2h_amd_time_window* window, const uint8_t* route,
                                  uint8_t* tflags, int64_t* mtime, int64_t* expire, uint8_t* keep,
                                  hipStream_t stream);

// A stream split into parts (k2h_ralledata_part.hip).  Returns a K2H_AMD_* code (the HIP error
// in *herr) and synchronises the stream once.  n >= 1 and a rule the ABI has judged.
int launch_ralledata_partition(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                               const k2h_amd_part_rule& rule, const uint32_t* part_ids, const uint8_t* consider,
                               void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* index, uint32_t* part_out,
                               uint64_t* part_first, uint64_t* part_byte, hipStream_t stream, hipError_t* herr);

// RALLEDATA blobs from range records (k2h_ralledata_recs.hip): the records of a scanned
// import file (key + NUL, value + NUL) or archive (SCOM_SET_ALL records as stored) become
// blobs packed in record order, a record that yields none taking 0 bytes; blob_off (n + 1,
// required) by a sizing kernel and an exclusive sum.  Both return a K2H_AMD_* code (the HIP
// error in *herr) and synchronise the stream once to return *total; out == NULL: sizes only;
// *total > out_cap: K2H_AMD_EINVAL with nothing written to out.  n >= 1.
int launch_import_ralledata(const void* file, uint64_t size, const k2h_amd_import_rec* recs, uint64_t n, uint64_t seed,
                            void* out, uint64_t out_cap, uint64_t* blob_off, uint64_t* total, hipStream_t stream,
                            hipError_t* herr);
int launch_archive_ralledata(const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n,
                             uint64_t seed, void* out, uint64_t out_cap, uint64_t* blob_off, uint64_t* total,
                             hipStream_t stream, hipError_t* herr);

// A blob stream as a k2hash archive (k2h_ralledata_archive.hip): one SCOM_SET_ALL record per
// participating blob, packed in blob order; rec_off (n + 1, required) by a sizing kernel and an
// exclusive sum.  Returns a K2H_AMD_* code (the HIP error in *herr) and synchronises the stream
// once to return *total and *records (may be NULL); out == NULL: sizes only; *total > out_cap:
// K2H_AMD_EINVAL with nothing written to out.  n >= 1.
int launch_ralledata_archive(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                             const uint8_t* keep, void* out, uint64_t out_cap, uint64_t* rec_off, uint64_t* records,
                             uint64_t* total, hipStream_t stream, hipError_t* herr);

// The log that turns the held stream B into the new stream A (k2h_ralledata_delta.hip), from the
// rel and seen of launch_ralledata_diff over the two.  Returns a K2H_AMD_* code (the HIP error in
// *herr) and synchronises the stream once to return counts.  1 <= na + nb <= 2^32 - 2;
// slot_off given with out.  K2H_AMD_EINVAL: out != NULL and counts[1] > out_cap (counts, slot_off
// and made are filled).
int launch_ralledata_delta(const void* a_blobs, uint64_t a_size, const uint64_t* a_off, uint64_t na, const uint8_t* rel,
                           const void* b_blobs, uint64_t b_size, const uint64_t* b_off, uint64_t nb,
                           const uint8_t* b_consider, const uint8_t* seen, void* out, uint64_t out_cap, uint64_t* slot_off,
                           uint8_t* made, uint64_t* counts, hipStream_t stream, hipError_t* herr);

// Keys looked up in a held stream (k2h_ralledata_find.hip).  All three return a K2H_AMD_* code (the
// HIP error in *herr); n <= 2^32 - 2.  ralledata_index_bytes is host arithmetic alone.  _index
// (index: at least ralledata_index_bytes(n), 256-byte aligned) synchronises the stream once when
// participants != NULL, _find (m >= 1; h1 and h2 both given or both NULL, then hashed with `seed`;
// now a host pointer, read before the return) once when counts != NULL, _fetch (m >= 1) always
// once, to return *total; out == NULL: sizes only; *total > out_cap: K2H_AMD_EINVAL with nothing
// written to out.
uint64_t ralledata_index_bytes(uint64_t n);
int launch_ralledata_index(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                           const uint8_t* consider, void* index, uint64_t* participants, hipStream_t stream,
                           hipError_t* herr);
int launch_ralledata_find(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n, const void* index,
                          const void* keys, uint64_t key_bytes, const uint64_t* key_off, uint64_t m,
                          const uint64_t* h1, const uint64_t* h2, uint64_t seed, bool cstr,
                          const k2h_amd_timespec* now, uint64_t* match, uint8_t* status, uint8_t* hit,
                          uint64_t* counts, hipStream_t stream, hipError_t* herr);
int launch_ralledata_fetch(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                           const uint64_t* which, uint64_t m, const uint8_t* take, uint32_t segment, void* out,
                           uint64_t out_cap, uint64_t* out_off, uint8_t* bad, uint64_t* total, hipStream_t stream,
                           hipError_t* herr);

// Keys at arbitrary (start, length) ranges (k2h_ranges.hip); cstr: hash key + NUL.
hipError_t launch_ranges(const void* base, const uint64_t* starts, const uint64_t* lens, uint64_t n, uint64_t seed,
                         bool cstr, uint64_t* h1, uint64_t* h2, hipStream_t stream);

// k2himport inputs already in device memory (k2h_import_dev.hip).  launch_import_scan
// returns a K2H_AMD_* code (the HIP error in *herr) and synchronises the stream.
// h1 != NULL: each written record's key is also hashed (key + NUL) by the same kernel.
int launch_import_scan(const void* file, uint64_t size, int format, k2h_amd_import_rec* recs, uint64_t cap,
                       uint64_t* count, hipStream_t stream, hipError_t* herr, uint64_t* h1 = nullptr,
                       uint64_t* h2 = nullptr, uint64_t seed = 0);
hipError_t launch_import_prehash(const void* file, uint64_t size, const k2h_amd_import_rec* recs, uint64_t n,
                                 uint64_t seed, uint64_t* h1, uint64_t* h2, hipStream_t stream);

// k2hash archives already in device memory (k2h_archive_dev.hip).  launch_archive_scan
// returns a K2H_AMD_* code (the HIP error in *herr) and synchronises the stream.
// hash != NULL: each written record's key (and, where new_h1 / new_h2 are given, the new key
// of each SCOM_RENAME record) is also hashed as stored, by the kernel that writes the record.
struct ArchiveHashOut {
  uint64_t* h1 = nullptr;  // required; the others may be null
  uint64_t* h2 = nullptr;
  uint64_t* new_h1 = nullptr;
  uint64_t* new_h2 = nullptr;
};
int launch_archive_scan(const void* file, uint64_t size, k2h_amd_archive_rec* recs, uint64_t cap, uint64_t* count,
                        hipStream_t stream, hipError_t* herr, const ArchiveHashOut* hash = nullptr, uint64_t seed = 0);
hipError_t launch_archive_prehash(const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n,
                                  uint64_t seed, const ArchiveHashOut& hash, hipStream_t stream);

// Log compaction by Load's rule (k2h_archive_fold.hip).  Returns a K2H_AMD_* code (the HIP
// error in *herr).  h1 == NULL: the keys are hashed with `seed` by launch_archive_prehash.
// Synchronises the stream once after the link stage, once per cover round, and once more when
// dropped != NULL.  1 <= n <= 2^32 - 2.
int launch_archive_fold(const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n,
                        const uint64_t* h1, uint64_t seed, uint8_t* keep, uint64_t* by, uint64_t* dropped,
                        hipStream_t stream, hipError_t* herr);

// A log applied to a held blob stream (k2h_archive_apply.hip).  Returns a K2H_AMD_* code (the HIP
// error in *herr) and synchronises the stream once.  1 <= na + n <= 2^32 - 2; h1 and h2 both
// given or both NULL (then hashed with `seed`).  K2H_AMD_EINVAL: out != NULL and counts[1] >
// out_cap (counts, stop and touched are filled).
int launch_archive_apply(const void* held, uint64_t held_size, const uint64_t* held_off, uint64_t na,
                         const uint8_t* held_keep, const void* file, uint64_t size, const k2h_amd_archive_rec* recs,
                         uint64_t n, const uint8_t* consider, const uint64_t* h1, const uint64_t* h2, uint64_t seed,
                         void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* origin, uint8_t* touched,
                         uint64_t* counts, uint64_t* stop, hipStream_t stream, hipError_t* herr);

// A barrier record executed on a held arena in place (k2h_archive_barrier.hip).  Returns a
// K2H_AMD_* code (the HIP error in *herr) and synchronises the stream once, to return result.
// na <= 2^32 - 2, b < n, held_cap >= held_size; the four hash arrays all given or all NULL (then
// record b's are hashed with `seed`).  K2H_AMD_EINVAL: an executed outcome whose result[2] exceeds
// held_cap - held_size (result is filled, nothing on the device is written).
int launch_archive_barrier(void* held, uint64_t held_size, uint64_t held_cap, uint64_t* held_off, uint64_t na,
                           uint8_t* held_keep, const void* file, uint64_t size, const k2h_amd_archive_rec* recs,
                           uint64_t n, uint64_t b, const uint8_t* consider, const uint64_t* h1, const uint64_t* h2,
                           const uint64_t* new_h1, const uint64_t* new_h2, uint64_t seed, bool count_only,
                           uint64_t* result, hipStream_t stream, hipError_t* herr);

// S_p = seed * P^-p (p = 0..15): start states for end-aligned chunking (k2h_csr.hip).
struct SpadTable {
  uint64_t v[16];
};
SpadTable make_spad(uint64_t seed);

// CSR tile kernel (k2h_csr.hip): 512-key LDS-staged tiles hashed two keys per lane; a
// tile whose bytes exceed the stage is hashed by the same block with the line ring.
hipError_t launch_csr_tile(const void* bytes, const uint64_t* offsets, uint64_t n, uint64_t seed, uint64_t* h1,
                           uint64_t* h2, hipStream_t stream, const BucketParams* bp = nullptr);
// Long fixed-length keys (> 32 B): the line-DMA kernel for multiples of 128 B at a
// 128-aligned base, else the cooperative line ring (>= 128 B) or direct loads (< 128 B).
bool fixed_lines_ok(const void* keys, uint64_t key_len);
hipError_t launch_fixed_long(const void* keys, uint64_t key_len, uint64_t n, uint64_t seed, uint64_t* h1,
                             uint64_t* h2, hipStream_t stream, const BucketParams* bp = nullptr);

hipError_t launch_fixed(const void* keys, uint64_t key_len, uint64_t n, uint64_t seed, uint64_t* h1, uint64_t* h2,
                        hipStream_t stream, const BucketParams* bp = nullptr);
hipError_t launch_csr(const void* bytes, const uint64_t* offsets, uint64_t n, uint64_t seed, uint64_t* h1,
                      uint64_t* h2, hipStream_t stream, const BucketParams* bp = nullptr);

// Synthetic inputs (bench/test harness; same spec as oracle/fnv_oracle.c generators).
hipError_t launch_synth_bytes(uint8_t* out, uint64_t nbytes, uint64_t seed, uint64_t byte_off, hipStream_t stream);
hipError_t launch_synth_lengths(uint32_t* lens, uint64_t n, uint64_t seed, uint64_t first_key, uint32_t min_len,
                                uint32_t max_len, hipStream_t stream);

}  // namespace k2h
