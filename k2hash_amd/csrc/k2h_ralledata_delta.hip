// k2hash_amd -- the transaction log that turns a held RALLEDATA stream into a new one
// (include/k2hash_amd.h section 4d': k2h_amd_ralledata_delta), the inverse of
// k2h_amd_archive_apply.  A is the new stream, B the held one; rel and seen are what
// k2h_amd_ralledata_diff said of the pair.  A blob i is slot i, B blob j slot na + j, and every
// slot yields 0 to 3 records in the bytes K2HCommandArchive::Put writes
// (lib/k2hcommand.cc:69-135, scom_init at lib/k2hcommand.h:99-113):
//   A, PART without FOUND   one SET_ALL with the blob's key, value, subkeys and attrs
//   A, PART and FOUND       one REPLACE_VAL / REPLACE_SKEY / REPLACE_ATTRS per differ bit, in that
//                           order, each with the key and the blob's bytes of the field (empty data
//                           clears the field, as Load does)
//   B, seen == 0            one DEL_KEY with the key, where b_consider lets the blob take part
//
// All on the caller's stream:
//   size     one lane per slot.  The slot's bits say which records it asks for; a slot that asks
//            for one is judged again -- span, header and classify (k2h_ralle_header.h) -- since
//            memory safety does not rest on rel or seen.  It leaves the slot's bytes, its emit
//            flag and its made byte, and counts the records per type and the refused slots by
//            per-wave ballots into the counter lines (k2h_layout.h).
//   place    PlaceRank (k2h_sort_stage.h) over the slots, bytes into slot_off and emit flags into ranks;
//            the counts come back to the host (the one synchronisation of the call).
//   compact  the emitting slots into a list, each at its rank.
//   build    over the list only: 8 lanes per emitting slot, 32 slots per block.  The record
//            headers come from registers, the key and the carried field go through group_copy
//            (k2h_ralle_pieces.h); a field of kDeltaLong bytes or more is moved by the slot's
//            whole wave.  A slot writes its up to three records in turn, header and key each time.
// In a replication delta a few percent of the blobs change: the size pass reads one byte of
// most slots and the build pass never sees them.
//
// Reads.  Nothing of a slot that asks for no record, nothing of a blob whose span is bad, nothing
// beyond the header of a blob that classify() refuses; with seen == NULL nothing of B.  The
// header is read in 16-byte loads at the blob's own alignment, inside the blob; the copies load
// exact source bytes, and every segment of a blob that passed lies inside it.  Nothing outside
// out[0, total), slot_off[0 .. na + nb] and made[0, na + nb) is written.  All absolute offsets
// are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_layout.h"
#include "k2h_ralle_header.h"
#include "k2h_ralle_ident.h"
#include "k2h_ralle_pieces.h"
#include "k2h_scratch.h"

// A build can launch the build kernel over every slot instead of over the compacted list: the
// comparison of DESIGN.md 5.4l.  0 is what is built.
#ifndef K2H_DELTA_ALL_SLOTS
#define K2H_DELTA_ALL_SLOTS 0
#endif

namespace k2h {
namespace {

constexpr bool kDeltaAllSlots = K2H_DELTA_ALL_SLOTS != 0;
constexpr int kScom = K2H_AMD_SCOM_HEADER;  // sizeof(SCOM), packed
constexpr int kDeltaBlock = 256;            // size, compact: slots per block, one per thread
constexpr int kDeltaGroup = 8;              // build: lanes per emitting slot
constexpr int kDeltaSlots = 256 / kDeltaGroup;
constexpr uint64_t kDeltaLong = 4096;  // build: a field of at least this many bytes is moved by the whole wave

constexpr uint32_t kSet = K2H_AMD_DELTA_SET_ALL, kVal = K2H_AMD_DELTA_REPLACE_VAL, kSkey = K2H_AMD_DELTA_REPLACE_SKEY,
                   kAttrs = K2H_AMD_DELTA_REPLACE_ATTRS, kDel = K2H_AMD_DELTA_DEL_KEY;
static_assert(kVal == kSet << 1 && kSkey == kSet << 2 && kAttrs == kSet << 3, "field f of a FOUND slot is bit kVal << f");
static_assert(K2H_AMD_DIFF_SKEY == K2H_AMD_DIFF_VAL << 1 && K2H_AMD_DIFF_ATTRS == K2H_AMD_DIFF_VAL << 2,
              "the differ bits in field order");

typedef uint32_t u32x2_ua __attribute__((ext_vector_type(2), aligned(1)));

// Bytes [8 w, 8 w + 8) of szCommand: the name, NUL-padded to 16 (lib/k2hcommand.h:36-45).
template <int N>
constexpr uint64_t cmd_word(const char (&s)[N], int w) {
  static_assert(N - 1 <= 16, "szCommand has 16 bytes");
  uint64_t v = 0;
  for (int b = 0; b < 8; ++b)
    if (8 * w + b < N - 1) v |= (uint64_t)(uint8_t)s[8 * w + b] << (8 * b);
  return v;
}
constexpr uint64_t kCmdSet0 = cmd_word("\nK2H_SET_ALL", 0), kCmdSet1 = cmd_word("\nK2H_SET_ALL", 1);
constexpr uint64_t kCmdRep0 = cmd_word("\nK2H_REP_VAL", 0);  // "\nK2H_REP" begins the three REPLACE names
constexpr uint64_t kCmdVal1 = cmd_word("\nK2H_REP_VAL", 1), kCmdSkey1 = cmd_word("\nK2H_REP_SKEY", 1),
                   kCmdAttrs1 = cmd_word("\nK2H_REP_ATTRS", 1);
constexpr uint64_t kCmdDel0 = cmd_word("\nK2H_DEL_KEY", 0), kCmdDel1 = cmd_word("\nK2H_DEL_KEY", 1);
static_assert(kCmdSet0 == 0x5445535F48324B0Aull && kCmdSet1 == 0x000000004C4C415Full, "as k2h_ralledata_archive.hip has them");
static_assert(cmd_word("\nK2H_REP_SKEY", 0) == kCmdRep0 && cmd_word("\nK2H_REP_ATTRS", 0) == kCmdRep0, "one first word");

struct DeltaIn {
  const uint8_t* a;
  uint64_t a_size;
  const uint64_t* a_off;
  uint64_t na;
  const uint8_t* rel;
  const uint8_t* b;
  uint64_t b_size;
  const uint64_t* b_off;
  uint64_t nb;
  const uint8_t* b_consider;
  const uint8_t* seen;
};

// The header's lengths and positions (fields 2 .. 9); the hash fields stay unread, as 0: a
// record stores no hash.
__device__ __forceinline__ void load_lens_pos(const uint8_t* p, uint64_t (&f)[10]) {
  f[0] = f[1] = 0;
#pragma unroll
  for (int c = 1; c < 5; ++c) {
    const uint4 v = ld16(p + 16 * c);
    f[2 * c] = pack2(v.x, v.y);
    f[2 * c + 1] = pack2(v.z, v.w);
  }
}

__device__ __forceinline__ void delta_count(unsigned long long* counter, int word, bool v) {
  const unsigned long long m = __ballot(v);
  if ((threadIdx.x & 63u) == 0 && m) {
    const uint32_t wave = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    atomicAdd(counter + 8 * (wave % kCounterLines) + word, (unsigned long long)__popcll(m));
  }
}

// Slot g of the na + nb: sizes[g] = the bytes of its records, flags[g] = 1 when it has some,
// mine[g] (and made[g], where the caller wants it) = a K2H_AMD_DELTA_* bit per record; entry
// na + nb of sizes and flags is 0, so entry na + nb of their exclusive sums is the total.
// Counts {SET_ALL, REPLACE_VAL, REPLACE_SKEY, REPLACE_ATTRS, DEL_KEY, refused} into words 0 .. 5.
__global__ __launch_bounds__(kDeltaBlock) void delta_size_kernel(DeltaIn s, uint64_t* __restrict__ sizes,
                                                                 uint32_t* __restrict__ flags, uint8_t* __restrict__ mine,
                                                                 uint8_t* __restrict__ made,
                                                                 unsigned long long* __restrict__ counter) {
  const uint64_t g = (uint64_t)blockIdx.x * kDeltaBlock + threadIdx.x;
  const uint64_t N = s.na + s.nb;
  uint32_t want = 0;  // the records the slot's bits ask for
  const uint8_t* base = nullptr;
  uint64_t size = 0, b = 0, e = 0;
  if (g < s.na) {
    const uint32_t r = s.rel[g];
    if (r & K2H_AMD_DIFF_PART)
      want = (r & K2H_AMD_DIFF_FOUND) ? ((r / K2H_AMD_DIFF_VAL) & 7u) * kVal : kSet;
    if (want) base = s.a, size = s.a_size, b = s.a_off[g], e = s.a_off[g + 1];
  } else if (g < N && s.seen) {
    const uint64_t j = g - s.na;
    if (s.seen[j] == 0 && (!s.b_consider || s.b_consider[j])) {
      want = kDel;
      base = s.b, size = s.b_size, b = s.b_off[j], e = s.b_off[j + 1];
    }
  }
  uint64_t v = 0;
  uint32_t m = 0;
  if (want && e >= b && e <= size && e - b >= (uint64_t)kHdr) {
    uint64_t f[10];
    load_lens_pos(base + b, f);
    if (classify(f, e - b) == K2H_AMD_RALLE_OK) {
      m = want;
      const uint64_t head = (uint64_t)kScom + f[2];  // every record repeats the header and the key
      if (m & (kSet | kDel)) {
        v = head + (m & kSet ? f[3] + f[4] + f[5] : 0);
      } else {
#pragma unroll
        for (int x = 0; x < 3; ++x)
          if (m & (kVal << x)) v += head + f[3 + x];
      }
    }
  }
  if (g <= N) {
    sizes[g] = v;
    flags[g] = m ? 1u : 0u;
  }
  if (g < N) {
    mine[g] = (uint8_t)m;
    if (made) made[g] = (uint8_t)m;
  }
  delta_count(counter, 0, m & kSet);
  delta_count(counter, 1, m & kVal);
  delta_count(counter, 2, m & kSkey);
  delta_count(counter, 3, m & kAttrs);
  delta_count(counter, 4, m & kDel);
  delta_count(counter, 5, want && !m);
}

// list[rank[g]] = g for every slot that emits.
__global__ __launch_bounds__(kDeltaBlock) void delta_compact_kernel(const uint32_t* __restrict__ rank, uint64_t N,
                                                                    uint32_t* __restrict__ list) {
  const uint64_t g = (uint64_t)blockIdx.x * kDeltaBlock + threadIdx.x;
  if (g >= N) return;
  const uint32_t r = rank[g];
  if (rank[g + 1] != r) list[r] = (uint32_t)g;
}

// Chunk c (words 2c, 2c + 1; chunk 6 has one) of the header of a record of `type` whose carried
// lengths are v, s and a -- 0 for what the type does not carry, which then keeps scom_init's
// position, 104, as exdata does.
__device__ __forceinline__ void delta_chunk(uint32_t c, uint32_t bit, uint64_t k, uint64_t v, uint64_t s, uint64_t a,
                                            uint64_t& w0, uint64_t& w1) {
  const bool all = bit == kSet;
  switch (c) {
    case 0:
      w0 = bit == kSet ? kCmdSet0 : bit == kDel ? kCmdDel0 : kCmdRep0;
      w1 = bit == kSet ? kCmdSet1 : bit == kVal ? kCmdVal1 : bit == kSkey ? kCmdSkey1 : bit == kAttrs ? kCmdAttrs1 : kCmdDel1;
      break;
    case 1:  // SCOM_SET_ALL 0, _REPLACE_VAL 1, _REPLACE_SKEY 2, _DEL_KEY 3, _REPLACE_ATTRS 5 (lib/k2hcommand.h:47-56)
      w0 = bit == kSet ? 0 : bit == kVal ? 1 : bit == kSkey ? 2 : bit == kDel ? 3 : 5;
      w1 = k;
      break;
    case 2: w0 = v, w1 = s; break;
    case 3: w0 = a, w1 = 0; break;
    case 4: w0 = kScom, w1 = all || bit == kVal ? kScom + k : kScom; break;
    case 5:
      w0 = all || bit == kSkey ? kScom + k + v : kScom;
      w1 = all || bit == kAttrs ? kScom + k + v + s : kScom;
      break;
    default: w0 = kScom, w1 = 0; break;  // 6
  }
}

// The records of the emitting slots, one slot per group of kDeltaGroup lanes.  A slot goes
// through three steps, one per field of {value, subkeys, attrs}: a record begins at step 0 for
// SET_ALL and DEL_KEY and at step f for the REPLACE of field f, and field f is copied at step f
// when the record at hand carries it.  The steps are the wave's, so that a long field can be
// left to all 64 lanes.  8 waves per SIMD: at most 64 VGPRs, no scratch.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void delta_build_kernel(
    DeltaIn s, const uint32_t* __restrict__ list, uint64_t emitting, const uint8_t* __restrict__ mine,
    const uint64_t* __restrict__ place, uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kDeltaSlots + threadIdx.x / kDeltaGroup;
  const uint32_t q = threadIdx.x % kDeltaGroup, lane = threadIdx.x & 63u;
  uint64_t f[10] = {};
  const uint8_t* blob = nullptr;
  uint8_t* to = nullptr;
  uint32_t m = 0;
  if (i < emitting) {
    const uint64_t g = kDeltaAllSlots ? i : list[i];
    m = mine[g];
    if (!kDeltaAllSlots || m) {
      blob = g < s.na ? s.a + s.a_off[g] : s.b + s.b_off[g - s.na];
      load_lens_pos(blob, f);  // the size pass judged it: every segment lies inside the blob
      to = out + place[g];
    }
  }
#pragma unroll
  for (int x = 0; x < 3; ++x) {
    const uint32_t bit = x == 0 && (m & (kSet | kDel)) ? m : m & (kVal << x);  // the record that begins here
    if (bit) {
      const bool all = bit == kSet;
      if (q < 7) {
        uint64_t w0, w1;
        delta_chunk(q, bit, f[2], all || bit == kVal ? f[3] : 0, all || bit == kSkey ? f[4] : 0,
                    all || bit == kAttrs ? f[5] : 0, w0, w1);
        if (q < 6)
          *reinterpret_cast<u32x4_ua*>(to + 16 * q) =
              u32x4_ua{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
        else
          *reinterpret_cast<u32x2_ua*>(to + 96) = u32x2_ua{(uint32_t)w0, (uint32_t)(w0 >> 32)};
      }
      group_copy<kDeltaGroup>(to + kScom, blob + f[6], f[2], q);
      to += (uint64_t)kScom + f[2];
    }
    // field x: of the SET_ALL at hand, or of the REPLACE that has just begun; the pos of a length-0 segment is ignored
    const uint64_t len = m & (kSet | (kVal << x)) ? f[3 + x] : 0;
    const uint8_t* const src = blob + f[7 + x];
    const bool wide = len >= kDeltaLong;
    if (len && !wide) group_copy<kDeltaGroup>(to, src, len, q);
    for (unsigned long long todo = __ballot(wide && q == 0); todo; todo &= todo - 1) {
      const int from = __ffsll((long long)todo) - 1;
      uint8_t* const d = (uint8_t*)ralle_shfl_u64((uint64_t)to, from);
      const uint8_t* const c = (const uint8_t*)ralle_shfl_u64((uint64_t)src, from);
      group_copy<64>(d, c, ralle_shfl_u64(len, from), lane);
    }
    to += len;
  }
}

// The call's temporaries (k2h_scratch.h) and the pinned words the results land in.  With
// N = na + nb: a made byte, a rank and a list entry per slot (9 N bytes), a place per slot (8 N)
// when the caller gives no slot_off, the counters and the library's own storage.
struct DeltaScratch : DeviceScratch {
  void* pinned = nullptr;
};
PerDevice<DeltaScratch> g_delta;

constexpr size_t kDeltaPinned = kCounterBytes + 16;  // the counter lines, the bytes, the emitting slots

struct DeltaCols {
  uint64_t* place;
  uint32_t* rank;
  uint32_t* list;
  uint8_t* mine;
  unsigned long long* counter;
  void* tmp;
  size_t total;
};

}  // namespace

// Returns a K2H_AMD_* code (the HIP error, if any, in *herr).  1 <= na + nb <= 2^32 - 2.
// Synchronises the stream once, to return counts.  K2H_AMD_EINVAL: out != NULL and counts[1] >
// out_cap (counts, slot_off and made are filled; out is not written).
int launch_ralledata_delta(const void* a_blobs, uint64_t a_size, const uint64_t* a_off, uint64_t na, const uint8_t* rel,
                           const void* b_blobs, uint64_t b_size, const uint64_t* b_off, uint64_t nb,
                           const uint8_t* b_consider, const uint8_t* seen, void* out, uint64_t out_cap, uint64_t* slot_off,
                           uint8_t* made, uint64_t* counts, hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  FirstError tr;
  auto done = [&](int rc) {
    *herr = tr.e;
    return !tr.ok() ? K2H_AMD_EHIP : rc;
  };
  const uint64_t N = na + nb;
  DeltaScratch* const scp = g_delta.current(tr);
  PlaceRank<> pr;
  pr.measure(tr, N, stream);
  if (!tr.ok()) return done(K2H_AMD_OK);
  DeltaScratch& sc = *scp;
  std::lock_guard<std::mutex> lk(sc.mu);
  if (!sc.pinned) tr(hipHostMalloc(&sc.pinned, kDeltaPinned, hipHostMallocDefault));
  if (!tr.ok()) return done(K2H_AMD_OK);
  unsigned long long* const host = (unsigned long long*)sc.pinned;
  auto layout = [&](void* base) {
    Carver c(base);
    DeltaCols k;
    k.place = c.take<uint64_t>(slot_off ? 0 : N + 1);
    k.rank = c.take<uint32_t>(N + 1);
    k.list = c.take<uint32_t>(N);
    k.mine = c.take<uint8_t>(N);
    k.counter = (unsigned long long*)c.bytes(kCounterBytes);
    k.tmp = c.bytes(pr.tmp_bytes());
    k.total = c.total();
    return k;
  };
  if (const int rc = sc.reserve(layout(nullptr).total, stream, herr)) return rc;
  const DeltaCols k = layout(sc.p);
  uint64_t* const place = slot_off ? slot_off : k.place;
  const DeltaIn s{(const uint8_t*)a_blobs, a_size, a_off, na, rel, (const uint8_t*)b_blobs, b_size, b_off, nb, b_consider,
                  seen};

  tr(hipMemsetAsync(k.counter, 0, kCounterBytes, stream));
  if (tr.ok()) {
    delta_size_kernel<<<(unsigned)(N / kDeltaBlock + 1), kDeltaBlock, 0, stream>>>(s, place, k.rank, k.mine, made,
                                                                                   k.counter);
    tr(hipGetLastError());
  }
  pr.scan(tr, k.tmp, place, k.rank, stream);
  unsigned long long* const tail = host + kCounterBytes / 8;  // bytes | emitting slots
  if (tr.ok()) tr(hipMemcpyAsync(host, k.counter, kCounterBytes, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(hipMemcpyAsync(tail, place + N, 8, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(hipMemcpyAsync(tail + 1, k.rank + N, 4, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(sc.mark_done(stream));
  if (tr.ok()) tr(hipStreamSynchronize(stream));
  if (!tr.ok()) return done(K2H_AMD_OK);
  const uint64_t emitting = (uint32_t)tail[1];
  counts[0] = 0;
  counts[1] = tail[0];
  for (int w = 0; w < 5; ++w) counts[0] += counts[2 + w] = counter_sum(host, w);
  counts[7] = counter_sum(host, 5);
  if (!out) return done(K2H_AMD_OK);
  if (counts[1] > out_cap) return done(K2H_AMD_EINVAL);
  if (emitting) {
    const uint64_t groups = kDeltaAllSlots ? N : emitting;
    if (!kDeltaAllSlots) {
      delta_compact_kernel<<<(unsigned)((N + kDeltaBlock - 1) / kDeltaBlock), kDeltaBlock, 0, stream>>>(k.rank, N, k.list);
      tr(hipGetLastError());
    }
    if (tr.ok()) {
      delta_build_kernel<<<(unsigned)((groups + kDeltaSlots - 1) / kDeltaSlots), 256, 0, stream>>>(
          s, k.list, groups, k.mine, place, (uint8_t*)out);
      tr(hipGetLastError());
    }
    if (tr.ok()) tr(sc.mark_done(stream));
  }
  return done(K2H_AMD_OK);
}

}  // namespace k2h
