/*
 * k2hash_amd -- MI355X-native key-hash path for yahoojapan/k2hash.
 *
 * C ABI of the two shared libraries built from k2hash_amd/csrc/:
 *
 *   libk2hfnv_plugin.so   the DROP-IN hash plugin.  Exports exactly the three
 *                         symbols k2hash's plugin loader resolves (section 1).
 *                         Pure C++, no HIP dependency, safe to dlopen from any
 *                         process/thread and across fork.
 *   libk2hash_amd.so      the same three symbols plus the batch ABI (section 2)
 *                         backed by hand-written CDNA4 HIP kernels.  Also a valid
 *                         plugin; HIP is initialised lazily by the first batch call.
 *
 * All hashes are bit-identical to the reference's default build
 * (lib/k2hashfunc.cc, "FNV-1A BUILTIN"), or, with K2H_AMD_FLAG_STD_FNV, to its
 * USE_STD_FNV_HASH_FUNCTION build ("STD::FNV BUILTIN").
 */
#ifndef K2HASH_AMD_H
#define K2HASH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* lib/k2hash.h:37 */
typedef uint64_t k2h_hash_t;

/* ---------------------------------------------------------------------------
 * 1. Drop-in plugin ABI.
 *
 * Replaces the weak builtins declared at lib/k2hashfunc.h:62-74 and defined at
 * lib/k2hashfunc.cc:62-96.  K2HashDynLib::Load (lib/k2hashfunc.cc:132-161,
 * reached from k2h_load_hash_library, lib/k2hash.cc:106-117, and from the tools'
 * -ext options, e.g. tests/k2hlinetool.cc:4995-5008) dlopen()s the plugin with
 * RTLD_LAZY and dlsym()s these three names, all-or-nothing
 * (lib/k2hashfunc.cc:149-156).  The same symbols also override the builtins at
 * link time or through LD_PRELOAD (lib/k2hcommon.h:41-45, docs/k2hash.1:50-55).
 *
 * Semantics (identical to the reference):
 *   - ptr == NULL or length == 0 -> 0            (lib/k2hashfunc.cc:66-68, 80-82)
 *   - k2h_hash: FNV-1a-64 over `length` bytes, each byte read as signed char
 *     and sign-extended before the XOR               (lib/k2hashfunc.cc:49-59)
 *   - k2h_second_hash: same over length-1 bytes when length > 1
 *                                                     (lib/k2hashfunc.cc:83-85)
 *   - k2h_hash_version: "FNV-1A BUILTIN" -- the reference's own string, because
 *     the hashes are identical and the string is stamped into / checked against
 *     every k2hash file header (lib/k2hshminit.cc:405, 641-646).  < 32 bytes
 *     (lib/k2hash.h:69).
 * Reentrant, lock-free, allocation-free, never throws or logs; no GPU work.
 * ------------------------------------------------------------------------- */
k2h_hash_t k2h_hash(const void* ptr, size_t length);        /* lib/k2hashfunc.h:65 */
k2h_hash_t k2h_second_hash(const void* ptr, size_t length); /* lib/k2hashfunc.h:68 */
const char* k2h_hash_version(void);                         /* lib/k2hashfunc.h:72 */

/* ---------------------------------------------------------------------------
 * 2. Batch ABI (new surface; libk2hash_amd.so only).
 *
 * The reference has no batch entry point: every call site hashes one key
 * synchronously (lib/k2hshm.cc:1230-1231, 2184-2185, ...).  Bulk callers
 * (bulk loads, archive import, RALLEDATA producers, benches) use these.
 *
 * Return value: K2H_AMD_OK (0) or a negative K2H_AMD_E* code;
 * k2h_amd_strerror() describes the last failure on the calling thread.
 * Per-key results follow the plugin semantics above; a key of length 0 hashes
 * to 0 (h1 and h2), and so does every key when the byte buffer is NULL.
 * h2 may be NULL (second hash not wanted).  `stream` is a hipStream_t
 * (NULL = the null stream).  Every device operation of a device-pointer call --
 * kernels, memsets, copies -- is issued to `stream` and to no other, so inputs
 * need only be ready on it; the call is asynchronous on it unless its section
 * says how often it synchronises `stream`.  Host structs passed by pointer are
 * read before the call returns.  (The Python wrappers order their own torch ops
 * on `stream` as well; stream=None there is the current torch stream.)
 * ------------------------------------------------------------------------- */
#define K2H_AMD_OK 0
#define K2H_AMD_EINVAL (-1)   /* bad argument (NULL output, overflow, ...) */
#define K2H_AMD_EHIP (-2)     /* HIP runtime error (see k2h_amd_strerror) */
#define K2H_AMD_ENOMEM (-3)   /* device / pinned host allocation failed */
#define K2H_AMD_ENODEV (-4)   /* no usable gfx950 device */

#define K2H_AMD_FLAG_STD_FNV 0x1u /* USE_STD_FNV_HASH_FUNCTION build: seed 2166136261
                                      (lib/k2hashfunc.cc:35-37, 69-70, 86-87) */

/* Fixed-length keys in device memory: key i = keys[i*key_len, (i+1)*key_len). */
int k2h_amd_hash_fixed(const void* keys, uint64_t key_len, uint64_t n, uint64_t* h1, uint64_t* h2, uint32_t flags,
                       void* stream);

/* CSR keys in device memory: key i = bytes[offsets[i], offsets[i+1]), offsets has n+1
 * non-decreasing entries (byte offsets relative to `bytes`). */
int k2h_amd_hash_csr(const void* bytes, const uint64_t* offsets, uint64_t n, uint64_t* h1, uint64_t* h2,
                     uint32_t flags, void* stream);

/* Host-memory forms: same layouts, host pointers in and out.  The library stages
 * through pinned buffers and overlaps H2D / kernel / D2H in chunks on `device`.
 * Synchronous: returns when h1/h2 are filled.  The CSR form checks its offsets chunk
 * by chunk as it streams them; offsets that decrease return K2H_AMD_EINVAL, and the
 * contents of h1/h2 are then unspecified (earlier chunks may have been written). */
int k2h_amd_hash_fixed_host(const void* keys, uint64_t key_len, uint64_t n, uint64_t* h1, uint64_t* h2,
                            uint32_t flags, int device);
int k2h_amd_hash_csr_host(const void* bytes, const uint64_t* offsets, uint64_t n, uint64_t* h1, uint64_t* h2,
                          uint32_t flags, int device);

/* ---------------------------------------------------------------------------
 * 3. Bucket-index epilogue (where each key lands in a k2hash table).
 *
 * For table masks (cur_mask, collision_mask) -- K2HSHM header fields, e.g. the
 * defaults 0xFF / 0xF of K2HShm::DEFAULT_MASK_BITCOUNT / DEFAULT_COLLISION_MASK_BITCOUNT
 * (lib/k2hshm.h:132-133) -- computes per hash h the stateless part of
 * K2HShm::GetKIndexPos (lib/k2hshm.cc:810-833, MakeMask / GetMaskBitCount at :78-90)
 * and the collision slot of K2HShm::GetCKIndex (lib/k2hshm.cc:1093):
 *   shifted       = h >> GetMaskBitCount(collision_mask)   (count taken mod 64)
 *   KIPtrArrayPos = GetMaskBitCount(shifted & cur_mask)
 *   KIArrayPos    = shifted & MakeMask(KIPtrArrayPos ? KIPtrArrayPos - 1 : 0)
 *   kindex[i]     = KIPtrArrayPos << 58 | KIArrayPos     (K2H_AMD_KINDEX_* below)
 *   ckindex[i]    = h & collision_mask
 * i.e. &key_index_area[KIPtrArrayPos][KIArrayPos] (CVT_ABS_PKINDEX, lib/k2hshm.cc:50)
 * and &ckey_list[ckindex].  The table-state part of GetKIndex (walking cur_mask down
 * past unassigned K_INDEX entries, lib/k2hshm.cc:882-907) is the *_table forms below.
 * kindex and ckindex may each be NULL; cur_mask must fit 58 bits when kindex is wanted.
 * The fused forms hash and index in one pass (the index costs no extra key read).
 * ------------------------------------------------------------------------- */
#define K2H_AMD_KINDEX_POS(v) ((uint64_t)(v) >> 58)                     /* KIPtrArrayPos */
#define K2H_AMD_KINDEX_ARR(v) ((uint64_t)(v) & ((1ull << 58) - 1ull))  /* KIArrayPos */

int k2h_amd_bucket_index(const uint64_t* h1, uint64_t n, uint64_t cur_mask, uint64_t collision_mask,
                         uint64_t* kindex, uint64_t* ckindex, void* stream);
int k2h_amd_hash_fixed_index(const void* keys, uint64_t key_len, uint64_t n, uint64_t* h1, uint64_t* h2,
                             uint32_t flags, uint64_t cur_mask, uint64_t collision_mask, uint64_t* kindex,
                             uint64_t* ckindex, void* stream);
int k2h_amd_hash_csr_index(const void* bytes, const uint64_t* offsets, uint64_t n, uint64_t* h1, uint64_t* h2,
                           uint32_t flags, uint64_t cur_mask, uint64_t collision_mask, uint64_t* kindex,
                           uint64_t* ckindex, void* stream);

/* Table-state forms: the K_INDEX that K2HShm::GetKIndex(hash, isMergeCurmask = false)
 * returns (lib/k2hshm.cc:862-907) for a snapshot of the table's assigned flags: cur_mask
 * walked down (cur_mask >>= 1 while > 0) until the entry GetKIndexPos gives for that mask
 * has assign == KINDEX_ASSIGNED (lib/k2hstructure.h:40-41).  Without the side effect of
 * the isMergeCurmask = true form (ArrangeToUpperKIndex): the caller rearranges.
 *   table->assigned: device bitmap, one bit per K_INDEX entry of the mapped table, LSB
 *     first in 32-bit words: entry KIArrayPos of key_index_area[KIPtrArrayPos] at bit
 *     KIPtrArrayPos ? 2^(KIPtrArrayPos-1) + KIArrayPos : 0  (cur_mask + 1 bits).  NULL:
 *     every entry assigned (= the stateless forms above).
 *   kindex[i]: the entry reached, packed as above; when no probed entry is assigned, the
 *     last probe's (mask 1), as the reference's loop leaves it; K2H_AMD_KINDEX_NONE when
 *     cur_mask is 0 (the reference returns NULL).
 *   found[i] (may be NULL): 1 when an assigned entry was reached, else 0. */
#define K2H_AMD_KINDEX_NONE (~0ull)
typedef struct k2h_amd_table {
  uint64_t cur_mask;         /* K2HSHM cur_mask */
  uint64_t collision_mask;   /* K2HSHM collision_mask */
  const uint32_t* assigned;  /* device bitmap of assigned K_INDEX entries, or NULL */
} k2h_amd_table;

int k2h_amd_bucket_index_table(const uint64_t* h1, uint64_t n, const k2h_amd_table* table, uint64_t* kindex,
                               uint64_t* ckindex, uint8_t* found, void* stream);
int k2h_amd_hash_fixed_index_table(const void* keys, uint64_t key_len, uint64_t n, uint64_t* h1, uint64_t* h2,
                                   uint32_t flags, const k2h_amd_table* table, uint64_t* kindex, uint64_t* ckindex,
                                   uint8_t* found, void* stream);
int k2h_amd_hash_csr_index_table(const void* bytes, const uint64_t* offsets, uint64_t n, uint64_t* h1,
                                 uint64_t* h2, uint32_t flags, const k2h_amd_table* table, uint64_t* kindex,
                                 uint64_t* ckindex, uint8_t* found, void* stream);

/* ---------------------------------------------------------------------------
 * 4. RALLEDATA producer (bulk direct-set input with precomputed hashes).
 *
 * k2h_set_element_by_binary (lib/k2hash.cc:1562-1581) -> K2HShm::SetElementByBinArray
 * (lib/k2hshmdirect.cc:343-478) inserts an element from a packed RALLEDATA blob
 * (lib/k2hshmdirect.h:36-47) and TRUSTS its hash / subhash fields: a bulk loader that
 * builds blobs here never runs the scalar hash per key.  Blob i (layout of
 * K2HShm::GetElementToBinary, lib/k2hshmdirect.cc:59-88):
 *   u64 hash = k2h_hash(key), subhash = k2h_second_hash(key),
 *   u64 key_length, val_length, skey_length, attrs_length,
 *   u64 key_pos = 80, val_pos, skey_pos, attrs_pos   (offsets from the blob top)
 *   then key | value | subkeys | attrs bytes.
 * Records are four CSR streams (bytes + n+1 offsets, offsets relative to the bytes
 * pointer); a NULL offsets array means that segment is empty for every record.  Blobs
 * are packed back to back in `out` (k2h_amd_ralledata_size bytes): blob i starts at
 * 80*i + the bytes of all earlier records, written to blob_off[i] (n+1 entries,
 * optional).  A K2HBIN for blob i is {out + blob_off[i], blob_off[i+1] - blob_off[i]}.
 * ------------------------------------------------------------------------- */
#define K2H_AMD_RALLEDATA_HEADER 80 /* sizeof(RALLEDATA), packed */

uint64_t k2h_amd_ralledata_size(uint64_t n, uint64_t key_bytes, uint64_t val_bytes, uint64_t skey_bytes,
                                uint64_t attr_bytes);
int k2h_amd_build_ralledata(const void* keys, const uint64_t* key_off, const void* vals, const uint64_t* val_off,
                            const void* skeys, const uint64_t* skey_off, const void* attrs, const uint64_t* attr_off,
                            uint64_t n, void* out, uint64_t* blob_off, uint32_t flags, void* stream);
int k2h_amd_build_ralledata_host(const void* keys, const uint64_t* key_off, const void* vals,
                                 const uint64_t* val_off, const void* skeys, const uint64_t* skey_off,
                                 const void* attrs, const uint64_t* attr_off, uint64_t n, void* out,
                                 uint64_t* blob_off, uint32_t flags, int device);

/* 4b. The consumer side: check, route and compact a blob stream before it is fed to
 * k2h_set_element_by_binary (which trusts the hash fields: a wrong one plants an element
 * no Get reaches).  Device pointers only; there is no host-pointer form.
 *
 * The stream: blob i = blobs[blob_off[i], blob_off[i+1]), blob_off has n+1 entries
 * relative to `blobs`, `size` is the number of readable bytes at `blobs` -- what
 * k2h_amd_build_ralledata writes, or a K2HBIN array laid end to end (trailing slack
 * inside a blob is allowed).
 *
 * k2h_amd_ralledata_check (async on `stream`): status[i] is the first that applies of
 *   BAD_SPAN     blob_off[i+1] < blob_off[i], or blob_off[i+1] > size, or length < 80
 *   EMPTY        all four lengths are 0                        (lib/k2hshmdirect.cc:351)
 *   NO_KEY       key_length == 0                               (lib/k2hshmdirect.cc:355)
 *   BAD_RANGE    for a segment of length > 0: pos < 80 (pos is a signed off_t), or
 *                pos + len overflows or passes the blob's end; the pos of a length-0
 *                segment is ignored, as lib/k2hshmdirect.cc:362-364 ignores it
 *   BAD_HASH     hash field != k2h_hash(key) under `flags` (K2H_AMD_FLAG_STD_FNV is
 *                honoured; K2H_AMD_FLAG_CSTR returns K2H_AMD_EINVAL)
 *   BAD_SUBHASH  subhash field != k2h_second_hash(key)
 * else OK.  Segment order and overlap are not checked (SetElementByBinArray honours any
 * positions).  No byte outside [0, size) is read except within the aligned 16 bytes that
 * hold a valid byte, and nothing of a BAD_SPAN blob.  h1[i] / h2[i] (each may be NULL):
 * the recomputed hashes for status OK, BAD_HASH and BAD_SUBHASH, else 0.
 *
 * With `range` (route must then be given; both NULL otherwise) route[i] is 0 unless
 * status[i] is OK, else
 *   bit 0: the stored hash is in the target range as K2HShm::GetElementListToBinary
 *          selects (lib/k2hshmdirect.cc:118-131):
 *            end = (target_hash + (target_hash_range > 0 ? target_hash_range - 1 : 0))
 *                  % target_max_hash            (the sum wraps in 64 bits)
 *            m = hash % target_max_hash
 *            in  = target_hash <= end ? !(m < target_hash || end < m)
 *                                     : !(end < m && m < target_hash)
 *          restated verbatim, target_hash >= target_max_hash included;
 *   bit 1: the hash is in the old range, the condition under which
 *          lib/k2hshmdirect.cc:165-176 leaves need_check_start true: the same
 *          arithmetic over old_hash / old_max_hash (and the same target_hash_range);
 *          0 when old_hash == ~0 (lib/k2hshmdirect.cc:119; no modulo is taken then).
 * target_max_hash == 0, or old_max_hash == 0 with old_hash != ~0: K2H_AMD_EINVAL.
 * Parity with GetElementListToBinary is a restatement: libk2hash itself is not built by
 * this project's tests (it needs libfullock).
 *
 * k2h_amd_ralledata_select copies every blob with keep[i] != 0 and a valid span (non-
 * decreasing, ending at or before size) back to back, in order, into `out`; out_off
 * (room for n+1) receives kept+1 offsets relative to `out`, starting at 0; index (room
 * for n; may be NULL) the kept blobs' original indices.  It synchronises `stream` once
 * to return *kept and *kept_bytes (host).  out == NULL: count only.  kept_bytes >
 * out_cap: K2H_AMD_EINVAL with both counts set and nothing written.
 *
 * Both: n == 0 returns K2H_AMD_OK with no device work. */
#define K2H_AMD_RALLE_OK 0
#define K2H_AMD_RALLE_BAD_SPAN 1
#define K2H_AMD_RALLE_EMPTY 2
#define K2H_AMD_RALLE_NO_KEY 3
#define K2H_AMD_RALLE_BAD_RANGE 4
#define K2H_AMD_RALLE_BAD_HASH 5
#define K2H_AMD_RALLE_BAD_SUBHASH 6
#define K2H_AMD_ROUTE_TARGET 0x1u /* route bit 0 */
#define K2H_AMD_ROUTE_OLD 0x2u    /* route bit 1 */

typedef struct k2h_amd_hash_range {
  uint64_t target_hash, target_max_hash;
  int64_t target_hash_range;
  uint64_t old_hash, old_max_hash; /* old_hash == ~0: no old range */
} k2h_amd_hash_range;

int k2h_amd_ralledata_check(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                            const k2h_amd_hash_range* range, uint32_t flags, uint8_t* status, uint8_t* route,
                            uint64_t* h1, uint64_t* h2, void* stream);
int k2h_amd_ralledata_select(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                             const uint8_t* keep, void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* index,
                             uint64_t* kept, uint64_t* kept_bytes, void* stream);

/* 4b'. Superseded duplicates: the blobs of a stream that k2h_set_element_by_binary need not
 * be fed, because a later blob of the same stream undoes them.  Device pointers only (the
 * stream arguments mean what they mean for k2h_amd_ralledata_check).
 *
 * Identity.  K2HShm::SetElementByBinArray finds the element a blob addresses from the
 * blob's STORED hash (GetCKIndex, lib/k2hshmdirect.cc:373), its stored hash and subhash
 * (GetElementList, :377) and its key bytes (GetElement, :378).  Two blobs address the same
 * element exactly when stored hash, stored subhash, key_length and the key bytes are equal.
 * The hash fields are trusted, not recomputed, as SetElementByBinArray trusts them.
 *
 * Rule.  Blob i is superseded when some later blob has i's identity -- call the nearest j --
 * and both i and j have attrs_length == 0.  Feeding the stream without i then leaves the
 * table that feeding it with i leaves, whatever the table held before: an absent element,
 * one without an attrs page (K2HShm::GetAttrs gives NULL, lib/k2hshm.cc:2059-2073) or an
 * expired one is overwritten by i, and i, having no attrs, is overwritten by j
 * unconditionally; before a live element with an mtime both i and j return early
 * (lib/k2hshmdirect.cc:402-405 when it is newer than pts, :421-427 because neither has an
 * mtime of its own).  A key-only blob (removes, inserts nothing, :438) takes the same
 * paths.  A blob with attrs is never dropped and never causes a drop: whether it wins
 * depends on the mtime and expiry inside its serialized K2HAttrs.
 *
 * Participants.  Blob i takes part when consider is NULL or consider[i] != 0, its span is
 * good (not BAD_SPAN) and its header passes the header tests of k2h_amd_ralledata_check
 * (not EMPTY, NO_KEY or BAD_RANGE).  All blobs of one identity get the same status and
 * route from _check, so the two compose as consider[i] = (status[i] == OK && route bit).
 *
 *   keep[i]  (n entries, required) 0 for a non-participant and for a superseded
 *            participant, 1 for every other participant
 *   by[i]    (n entries, may be NULL) the nearest later participant of i's identity, whether
 *            or not it supersedes i; ~0 when there is none, and for a non-participant
 *   *dropped (host, may be NULL) the number of superseded blobs
 *
 * dropped == NULL: asynchronous on `stream`; else `stream` is synchronised once.  n == 0:
 * K2H_AMD_OK, *dropped = 0, no device work.  K2H_AMD_EINVAL, judged on the host before any
 * device is touched, each with its own message: keep, blobs or blob_off NULL with n > 0;
 * n > 2^32 - 2 (indices are sorted as 32-bit values).
 *
 * No byte outside [0, size) is read except within the aligned 16 bytes that hold a valid
 * byte; nothing of a non-participant beyond its header, and no header of a blob whose
 * span is bad.  Temporary device memory: about 56 bytes per blob plus the sort's own, kept
 * per device between calls.  Cost: a gather pass over the headers, one library radix sort of
 * (stored hash, index) pairs on the hash's low bits, and a resolve pass that reads only the
 * keys of blobs whose stored hash occurs more than once; r DISTINCT keys under one stored
 * hash cost O(r^2) key compares (a crafted stream, or one whose hash fields _check would
 * have refused), and r stored hashes that agree in all their low bits O(r^2) walk steps. */
int k2h_amd_ralledata_dedup(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                            const uint8_t* consider, uint8_t* keep, uint64_t* by, uint64_t* dropped, void* stream);

/* 4b''. A stream split into parts: the P-way sibling of k2h_amd_ralledata_select, a stable
 * partition of variable-length blobs.  One call takes a stream and produces the same blobs
 * grouped by part, in stream order within each part -- one buffer slice per owner node, or
 * per lock domain of a loader -- where P calls of _select would read the stream's offsets
 * and masks P times and synchronise P times.
 *
 * Device pointers: blobs, blob_off, part_ids, consider, out, out_off, index, part_out.  Host
 * pointers: rule, part_first, part_byte; the last two have rule->parts + 1 entries each.
 *
 * Which blobs take part.  Blob i takes part when all of these hold:
 *   - consider is NULL or consider[i] != 0;
 *   - its span is valid as _select judges it: non-decreasing, ending at or before size;
 *   - K2H_AMD_PART_IDS: part_ids[i] < parts, and its part is part_ids[i].  A blob of 0 bytes
 *     with a valid span takes part, as in _select;
 *   - K2H_AMD_PART_OWNER / _MASK: the span is at least 80 bytes.  The stored hash is the
 *     blob's first 8 bytes; it is trusted, not recomputed, as SetElementByBinArray and _dedup
 *     trust it (compose with _check through consider[i] = (status[i] == OK)).  Nothing of a
 *     blob beyond those 8 bytes is read to decide its part, and nothing at all of a blob whose
 *     span is bad or short.
 *
 * Outputs.
 *   out        the participants of part 0 in stream order, then those of part 1, and so on,
 *              back to back
 *   out_off    (room for n + 1) kept + 1 offsets relative to out, starting at 0
 *   index      (room for n; may be NULL) the original indices, in output order
 *   part_out   (n entries; may be NULL) each blob's part, or K2H_AMD_PART_NONE if left out
 *   part_first[p]  the rank in out_off at which part p starts; part_first[parts] = kept
 *   part_byte[p]   the byte offset in out at which part p starts; part_byte[parts] = kept_bytes
 * Part p is blobs [part_first[p], part_first[p+1]) of the output; an empty part has equal
 * neighbours.  Because the partition is stable, all blobs of one identity (4b') land in one
 * part in their original order: _dedup before or after the partition gives the same result.
 *
 * Flow, as _select: the counts first, one synchronisation of `stream` that returns part_first
 * and part_byte, then the copy, asynchronous on `stream`.  out == NULL: counts only (and
 * part_out if given).  kept_bytes > out_cap: K2H_AMD_EINVAL with both host arrays set and
 * nothing written to out, out_off or index.  n == 0: K2H_AMD_OK, both host arrays zeroed, no
 * device work.
 *
 * K2H_AMD_EINVAL, judged on the host before any device is touched, each with its own message:
 * rule, part_first or part_byte NULL; an unknown kind; parts 0 or above K2H_AMD_PART_MAX; IDS
 * without part_ids, or part_ids given with another kind; OWNER with max_hash == 0, span == 0 or
 * parts != ceil(max_hash / span); blobs or blob_off NULL with n > 0; out given without out_off.
 *
 * OWNER.  part = (stored hash % max_hash) / span.  For every part p with p*span + span <=
 * max_hash, the members are exactly the blobs whose route bit 0 is set by
 * k2h_amd_ralledata_check with {target_hash = p*span, target_max_hash = max_hash,
 * target_hash_range = span}.  The last, short part (when span does not divide max_hash) takes
 * m = hash % max_hash in [p*span, max_hash); the reference's range would wrap there.  Parity
 * with GetElementListToBinary is the same restatement as for _check.
 *
 * MASK.  part = (stored hash & mask) % parts.  With mask = collision_mask and parts <=
 * collision_mask + 1, blobs in different parts have different hash & collision_mask
 * (lib/k2hshm.cc:1093), so different CKINDEX entries -- the lock SetElementByBinArray takes
 * (lib/k2hshmdirect.cc:369-373) -- in any table state.  A wider mask (cur_mask bits included)
 * separates K_INDEX entries only when every K_INDEX at cur_mask is assigned; see the _table
 * forms of section 3.  Whether feeding the parts from several threads actually speeds up
 * libk2hash is NOT measured here: the library is not built by this project, and page
 * allocation has locks of its own.
 *
 * Temporary device memory, kept per device between calls: per tile of 1024 blobs 16 * parts
 * bytes (the tile's count and bytes per part, scanned in place), plus 2 bytes per blob for
 * its part, plus the scan's own.  8 Mi blobs at 256 parts: 33.5 MB + 16.8 MB. */
#define K2H_AMD_PART_MAX 256
#define K2H_AMD_PART_NONE 0xFFFFFFFFu /* part_out[i] of a blob left out */
#define K2H_AMD_PART_IDS 0            /* part[i] given by the caller */
#define K2H_AMD_PART_OWNER 1          /* (stored hash % max_hash) / span */
#define K2H_AMD_PART_MASK 2           /* (stored hash & mask) % parts */

typedef struct k2h_amd_part_rule {
  uint32_t kind, parts;    /* 1 <= parts <= K2H_AMD_PART_MAX */
  uint64_t max_hash, span; /* OWNER: both > 0, parts == ceil(max_hash / span) */
  uint64_t mask;           /* MASK */
} k2h_amd_part_rule;

int k2h_amd_ralledata_partition(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                                const k2h_amd_part_rule* rule, const uint32_t* part_ids, const uint8_t* consider,
                                void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* index, uint32_t* part_out,
                                uint64_t* part_first, uint64_t* part_byte, void* stream);

/* 4b''''. The times inside a blob's attrs: the mtime window of GetElementListToBinary, and a
 * dedup that works on streams whose blobs carry the builtin mtime.  Both rest on one device
 * walk of the serialized K2HAttrs (k2hash_amd/csrc/k2h_ralle_attrs.h).
 *
 * Parsing, K2HAttrs::Serialize(const unsigned char*, size_t), lib/k2hattrs.cc:121-166.  A is
 * the attrs segment, AL its length.  AL < 8: no entries.  Else count = the u64 at 0, pos = 8,
 * rest = AL - 8, and up to count times: rest < 16 stops; kl, vl = the u64s at pos, pos + 8; an
 * entry that does not fit in rest stops (the entries accepted before stay); the key is
 * A[pos + 16, + kl) and the value the vl bytes behind it; kl == 0 is consumed but not kept
 * (insert refuses it); a key equal to an earlier one replaces it (:356-363); pos += 16 + kl +
 * vl.  One departure: the reference forms 16 + kl + vl in size_t, and where that sum wraps it
 * reads out of bounds; here kl > rest - 16 || vl > rest - 16 - kl is tested without forming
 * the sum, and the walk stops.
 *
 * Times, K2hAttrBuiltin::GetTime, lib/k2hattrbuiltin.cc:864-883.  A time is present exactly
 * when the last accepted entry with its key has vl == 16; the key is "mtime\0" (kl 6) or
 * "expire\0" (kl 7), the NUL included as find(const char*) includes it; the value is a struct
 * timespec, int64 tv_sec then int64 tv_nsec.  Times compare signed, sec first, nsec as stored.
 * A later entry of the same key with vl != 16 hides an earlier good one.  Expired at `now`
 * (IsExpire, :830-862; the reference reads the clock, here the caller passes it): expire is
 * present and expire < now.
 *
 * k2h_amd_ralledata_times (async on `stream`; device pointers except `window`, a host pointer
 * that may be NULL and is read before the call returns).
 *
 * Participants, as _dedup: consider is NULL or consider[i] != 0, the span is good and the
 * header is not EMPTY, NO_KEY or BAD_RANGE.  A non-participant gets tflags 0, zero times and
 * keep 0, and nothing of it beyond its header is read.
 *
 *   tflags[i]  K2H_AMD_TIMES_MTIME / _EXPIRE: that time is present; _CUT: the walk stopped
 *              before count entries were read, or AL is 1 to 7; _ATTRS: attrs_length != 0
 *   mtime, expire  (2 n int64 each) sec, nsec of blob i at [2 i], [2 i + 1]; an absent time
 *              is 0, 0
 *   keep[i]    for a participant, lib/k2hshmdirect.cc:137-197 in its order: 0 if WIN_EXPIRE is
 *              set and the blob is expired at window->now; otherwise, if the blob has an mtime,
 *              0 if need_start(i) and WIN_START is set and mtime < start, otherwise 0 if
 *              WIN_END is set and end < mtime, otherwise 1; a blob without mtime is 1
 *              (:155-157).  need_start(i) = (route[i] & K2H_AMD_ROUTE_OLD) != 0, the bit
 *              k2h_amd_ralledata_check computes; route == NULL: true for every blob.
 *              window == NULL: keep[i] = participant.  Route bit 0 is not looked at: the
 *              caller ANDs it in.
 * Each of the four may be NULL, but not all.  K2H_AMD_EINVAL, judged on the host before any
 * device is touched, each with its own message: all four outputs NULL; route given without
 * window; unknown window flag bits; blobs or blob_off NULL with n > 0.  n == 0: K2H_AMD_OK, no
 * device work.
 *
 * No byte outside [0, size) is read except within the aligned 16 bytes that hold a valid
 * byte; every load of the walk lies inside the attrs segment, at any alignment.  One lane
 * walks one segment, a chain of one dependent 16-byte load per entry.  Dropping blobs because
 * they are themselves expired is not done anywhere: an expired blob still overwrites and
 * hides an older element; _times reports the fact and the policy is the caller's.
 *
 * k2h_amd_ralledata_dedup_mtime: the arguments of k2h_amd_ralledata_dedup plus pts, a required
 * host pointer (read before the call returns): the pts the caller will pass to
 * k2h_set_element_by_binary for every blob of the stream.  Identity, participants, by, dropped
 * and the async / sync rule are those of _dedup.  Blob i is superseded by the nearest later
 * participant j of its identity when
 *   (a) i has no mtime (no attrs, or attrs in which GetMTime fails), or
 *   (b) i and j both have an mtime, m_i < m_j and m_i < pts (both strict; they mirror the <=
 *       refusals at lib/k2hshmdirect.cc:402 and :416).
 * Otherwise i is kept: i with an mtime before a j without one is kept, and an expired i gets
 * no special treatment.  Against a prior element E, i either is refused exactly when j would
 * be, or is accepted and then overwritten by j.  (a), E without mtime, without attrs or
 * expired: j overwrites i because i has no mtime (:395-400); (a), E live with an mtime: both
 * are refused (:421-427); (b), i accepted: j is accepted because pts > m_i and m_j > m_i; (b),
 * i refused (pts <= m_E, or m_i <= m_E against a live E): the stream without i meets the same
 * E.  Three assumptions: one pts for the whole feed; the blobs are fed in stream order; an
 * element that is expired stays expired.  Every blob _dedup drops is dropped here too, and on
 * a stream without attrs the two results are equal.  Temporary device memory: that of _dedup
 * plus 16 bytes per blob.  K2H_AMD_EINVAL as _dedup, and for pts NULL (with n > 0).
 *
 * Parity: the parse is pinned by tests/golden/ralle_attrs.json, written by the reference's own
 * K2HAttrs (tests/golden/gen_ralle_attrs.cc); GetTime, IsExpire, the window and the replay that
 * shows the drop rule sound are restatements -- libk2hash itself is not built by this
 * project's tests. */
typedef struct k2h_amd_timespec {
  int64_t sec, nsec;
} k2h_amd_timespec;
#define K2H_AMD_WIN_START 0x1u
#define K2H_AMD_WIN_END 0x2u
#define K2H_AMD_WIN_EXPIRE 0x4u
typedef struct k2h_amd_time_window {
  uint32_t flags, reserved;
  k2h_amd_timespec start, end, now;
} k2h_amd_time_window;
#define K2H_AMD_TIMES_MTIME 0x1u
#define K2H_AMD_TIMES_EXPIRE 0x2u
#define K2H_AMD_TIMES_CUT 0x4u
#define K2H_AMD_TIMES_ATTRS 0x8u /* attrs_length != 0 */

int k2h_amd_ralledata_times(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                            const uint8_t* consider, const k2h_amd_time_window* window, const uint8_t* route,
                            uint8_t* tflags, int64_t* mtime, int64_t* expire, uint8_t* keep, void* stream);
int k2h_amd_ralledata_dedup_mtime(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                                  const uint8_t* consider, uint8_t* keep, uint64_t* by, uint64_t* dropped,
                                  const k2h_amd_timespec* pts, void* stream);

/* 4b'''''. Two streams joined by identity: what an incoming stream changes.  The calls above
 * judge a stream against itself; a receiver's question compares two.  A is the incoming stream
 * (the output of k2h_get_elements_by_hash on a peer), B the held stream: a dump of what the
 * local table holds for the identities in question.  For every blob of A that the table
 * already holds, K2HShm::SetElementByBinArray (lib/k2hshmdirect.cc:343-478) takes the CKINDEX
 * write lock, finds the element and parses its attrs, and then returns early (:402-405,
 * :416-419, :421-427) or frees an element only to allocate the same bytes again.  This call
 * says which blobs of A are worth that.  Device pointers except `times` and `counts`.
 *
 * Participants, in both streams, by the rule of _dedup: consider is NULL or consider[i] != 0,
 * the span is good and the header is not EMPTY, NO_KEY or BAD_RANGE.  Identity is that of
 * section 4b': stored hash, stored subhash, key_length, key bytes; the hash fields are trusted,
 * not recomputed (compose with _check through the consider arrays).
 *
 *   match[i] (na entries, may be NULL) the index in B of the LAST participant of B with i's
 *            identity; ~0 when there is none, and for a non-participant of A.  A dump holds one
 *            blob per identity; of a B that holds several the last one is taken.
 *   rel[i]   (na entries, required) 0 for a non-participant; else K2H_AMD_DIFF_PART, and
 *            _DATA  when any of i's value, subkeys and attrs lengths is non-zero (:438);
 *            _FOUND when match[i] != ~0; with it one of _VAL, _SKEY, _ATTRS per segment that
 *                   differs from the matched blob's.  Two segments are equal when their lengths
 *                   are equal and, where the length is non-zero, their bytes are; the pos of a
 *                   length-0 segment is ignored, and unequal lengths set the bit without a
 *                   payload byte being read;
 *            _REPEAT when another participant of A stores i's 64-bit hash: an over-approximation
 *                   of "another blob of A has i's identity" that needs no key read;
 *            _APPLY only when `times` is given.  Not FOUND: set (the path falls through at
 *                   :377-378).  FOUND: :380-431 with the matched blob's attrs as the existing
 *                   element's, in this order: set if the matched blob has attrs_length == 0 (no
 *                   attrs page, GetAttrs NULL); set if it is expired at times->now; set if it
 *                   has no mtime; clear if pts <= m_b (:402); set if i has an mtime and
 *                   m_b < m_i; clear otherwise (:416, :426).  Times are read and compared as in
 *                   section 4b''''.
 *   seen[j]  (nb entries, may be NULL) 1 when some participant of A has match == j, else 0; all
 *            nb entries are written.  The blobs of B with seen 0 are the held elements A does
 *            not mention.  This call only reports them; k2h_amd_ralledata_delta (section 4d')
 *            turns them into DEL_KEY records.
 *   counts   (host, 4 entries, may be NULL) participants of A, FOUND, FOUND with no differ bit,
 *            APPLY.  counts != NULL: `stream` is synchronised once; else the call is
 *            asynchronous.
 *
 * What the bits are for.  Let change(i) = FOUND ? (VAL | SKEY | ATTRS) != 0 : DATA, and
 * feed(i) = PART && (REPEAT || (APPLY && change(i))).  Feeding only the blobs with feed leaves
 * the table that feeding all of A leaves, provided B holds the table's element for every
 * identity of A that the table has, and no other; one pts is used for the whole feed; now is
 * the clock at feed time; and an expired element stays expired.  A blob without APPLY returns
 * early; one with APPLY and no change frees an element (or finds none) and stores the same
 * bytes (or none).  A REPEAT blob is always fed: its verdict against B goes stale as soon as an
 * earlier blob of its key is applied -- an applied blob that is itself expired lets any later
 * blob overwrite it.  tests/test_ralledata_diff.py replays this on the CPU against a
 * transliteration of SetElementByBinArray; libk2hash itself is not built by this project, so
 * parity with it is a restatement, as in the sections above.
 *
 * K2H_AMD_EINVAL, judged on the host before any device is touched, each with its own message:
 * rel NULL with na > 0; a stream's blobs or offsets NULL with its n > 0; na + nb > 2^32 - 2
 * (indices of both streams are sorted as 32-bit values of one space).  na == 0: K2H_AMD_OK,
 * counts zeroed, seen (if given) zeroed by one memset on `stream`.  nb == 0 is an ordinary call
 * in which nothing is found.
 *
 * No byte outside [0, size) of either stream is read except within the aligned 16 bytes that
 * hold a valid byte; nothing of a blob whose span is bad or whose consider byte is 0, nothing
 * of a non-participant beyond its header, and no payload byte of a pair whose segment lengths
 * differ.  All absolute offsets are 64-bit.
 *
 * Cost: a gather pass over both streams' headers (with times also over the attrs of the blobs
 * that have some), one library radix sort of na + nb (stored hash, index) pairs on the hash's
 * low bits, one max-scan, a resolve pass that reads the keys of the blobs whose stored hash
 * occurs in both streams, and a compare pass that reads the equal-length segments of every
 * matched pair from both streams.  r copies of one key in A, matched or not, cost O(1) steps
 * each; r DISTINCT identities that agree in all sorted bits, in A or in B, cost O(r) steps per
 * blob of A among them -- the crafted-stream case of section 4b'.  Temporary device memory, kept
 * per device between calls: 57 bytes per blob of na + nb (the 56 of _dedup and a participant
 * byte; the scan column and the compare's work items reuse the sort's input columns) plus the
 * sort's own, and 16 bytes per blob more with times. */
#define K2H_AMD_DIFF_PART 0x01u   /* A blob i takes part */
#define K2H_AMD_DIFF_FOUND 0x02u  /* a held blob of i's identity exists */
#define K2H_AMD_DIFF_VAL 0x04u    /* FOUND, and the value segments differ */
#define K2H_AMD_DIFF_SKEY 0x08u   /* FOUND, and the subkeys segments differ */
#define K2H_AMD_DIFF_ATTRS 0x10u  /* FOUND, and the attrs segments differ */
#define K2H_AMD_DIFF_DATA 0x20u   /* i has a value, subkeys or attrs (lib/k2hshmdirect.cc:438) */
#define K2H_AMD_DIFF_REPEAT 0x40u /* another participant of A stores i's hash */
#define K2H_AMD_DIFF_APPLY 0x80u  /* with times: SetElementByBinArray would not return early */

typedef struct k2h_amd_diff_times {
  k2h_amd_timespec pts, now;
} k2h_amd_diff_times;

int k2h_amd_ralledata_diff(const void* a_blobs, uint64_t a_size, const uint64_t* a_off, uint64_t na,
                           const uint8_t* a_consider, const void* b_blobs, uint64_t b_size, const uint64_t* b_off,
                           uint64_t nb, const uint8_t* b_consider, const k2h_amd_diff_times* times, uint8_t* rel,
                           uint64_t* match, uint8_t* seen, uint64_t* counts, void* stream);

/* 4b''''''. Subkeys followed through a stream: edges and subtree closure.  Every call above
 * treats a blob's subkeys segment as opaque bytes, yet subkeys are what make a k2hash table a
 * tree: K2HShm::Remove(key, true) removes a key with everything below it.  These two calls read
 * the segment: _subkeys turns every name in it into an edge to the blob the table would find
 * under that name, _reach follows the edges from a set of roots.  Device pointers except
 * `counts`.
 *
 * The segment, K2HSubKeys::Serialize(const unsigned char*, size_t), lib/k2hsubkeys.cc:113-156,
 * with S the segment and L = skeys_length: a u64 count, then count entries of u64 length +
 * length bytes.  A zero-length entry is refused by insert (:302-305) and skipped, parsing goes
 * on; when a length field or a name does not fit, Serialize returns false and
 * K2HPage::GetSubKeys throws the whole list away (lib/k2hpage.cc:274-299): a rejected segment
 * means no subkeys, not the entries read so far.  Bytes after the last entry are ignored;
 * count == 0 is an accepted empty list.  One departure, the counterpart of the one section
 * 4b'''' makes for the attrs sum that wraps: the reference starts rest_length at the whole L although its read
 * position is already past the count, so on a malformed segment it accepts an entry that runs
 * up to 8 bytes past the segment's end, and it reads the count out of bounds when L is 1 to 7.
 * The rule here is the strict one, which never reads outside the segment: L == 0 is no list;
 * L < 8 is BAD; else pos = 8 and count times: BAD if L - pos < 8; len = the u64 at pos,
 * pos += 8; BAD if L - pos < len; an edge when len > 0; pos += len.  Every segment the
 * reference's own writer produces is judged the same by both rules; they differ only where the
 * reference reads out of bounds.
 *
 * The rule restated, K2HShm::Remove(key, true): lib/k2hshm.cc:2544-2560, RemoveEx :2735-2864,
 * RemoveSubkeys :2866-2898.  It hashes the name with K2H_HASH_FUNC / K2H_2ND_HASH_FUNC, finds
 * the element by hash, subhash and key bytes, takes its subkey list through
 * GetSubKeys(pElement, pSubKeys) -- the form that makes no expiry or history check -- removes
 * the element, and does the same for every name in the list, re-entrantly; a name that is not
 * found is skipped, and a cycle ends because the element is already gone.  The history
 * attribute (IsMarkHistory), which renames instead of removing, is out of scope.
 *
 * Proviso.  "The table the stream leaves" is taken as: the LAST participant of an identity
 * wins.  That holds for a feed without the mtime attribute or with non-decreasing times; a
 * caller with mtime-bearing blobs passes as `consider` the keep of k2h_amd_ralledata_dedup_mtime
 * first.  Expiry is deliberately not applied, as Remove does not apply it; a caller who wants
 * it composes k2h_amd_ralledata_times.  A participant with a key and nothing else counts as its
 * key's last copy like any other, although feeding it leaves no element (lib/k2hshmdirect.cc:438):
 * it has no list, and a name that addresses it is not dangling.
 *
 * k2h_amd_ralledata_subkeys.  Participants, as _dedup: consider is NULL or consider[i] != 0,
 * the span is good and the header is not EMPTY, NO_KEY or BAD_RANGE.  An edge carries the
 * name's COMPUTED hashes -- k2h_hash and k2h_second_hash over the raw name bytes, no NUL added
 * (the name carries whatever NUL it was stored with), seed by K2H_AMD_FLAG_STD_FNV -- its length
 * and its bytes; a blob its STORED hash, stored subhash, key_length and key bytes (the identity
 * of section 4b').  They are joined as the table would look the name up: a blob whose stored
 * hashes are wrong is not found by name.
 *
 *   sk_flags[i] (n, required) 0 for a non-participant; else K2H_AMD_SKEY_PART, _HAS when
 *               skeys_length != 0, _BAD when the strict walk rejected the segment (then no edges)
 *   edge_off    (n + 1, required) edge_off[0] = 0; blob i's edges are [edge_off[i],
 *               edge_off[i+1]), one per entry with len > 0 in segment order; E = edge_off[n]
 *   rep[i]      (n, may be NULL) the LAST participant of i's own identity: i itself for the last
 *               copy of a key; ~0 for a non-participant.  Written only when child != NULL.
 *   child[e]    (cap entries; NULL: count only) the LAST participant whose identity edge e's name
 *               addresses; ~0 when there is none: a dangling name
 *   counts      (host, 5 entries, required) participants, blobs with >= 1 edge, BAD segments,
 *               E, dangling edges (0 when child is NULL)
 *
 * `stream` is synchronised once after the count pass (E sizes everything behind it) and, when
 * child != NULL, once more at the end: once with child NULL, twice otherwise.  No form of the
 * call is asynchronous.
 *
 * K2H_AMD_EINVAL, judged on the host before any device is touched, each with its own message:
 * counts NULL; K2H_AMD_FLAG_CSTR; unknown flag bits; sk_flags, edge_off, blobs or blob_off NULL
 * with n > 0; n > 2^32 - 2.  After the count pass, with counts and edge_off filled and nothing
 * written to child or rep: child != NULL and cap < E (the message names E); n + E > 2^32 - 2
 * (blobs and edges are sorted as 32-bit indices of one space, as in _diff).  n == 0:
 * K2H_AMD_OK, counts zeroed, edge_off[0] = 0 by one memset on `stream` (when edge_off is given).
 *
 * No byte outside [0, size) is read except within the aligned 16 bytes that hold a valid byte;
 * every load of the walk lies inside the subkeys segment, at any alignment; nothing of a
 * non-participant beyond its header, and nothing outside a blob's own subkeys segment is ever
 * interpreted.  All absolute offsets are 64-bit.
 *
 * Cost: a count pass over the headers and the segments (one lane walks one segment: one
 * dependent 8-byte load per entry, so a very long list holds its wave for its length); with
 * child a second such pass that leaves the names' places, a pass that hashes every name, one
 * library radix sort of n + E (hash, index) pairs on the hash's low bits, two max-scans and a
 * resolve pass that reads the keys and names whose hashes meet.  r copies of one key cost O(1)
 * steps per entry; r DISTINCT identities that agree in all sorted bits cost O(r) steps per
 * entry among them -- the crafted-stream case of section 4b'.  Temporary device memory, kept
 * per device between calls and shared with _reach: 60 bytes per blob and edge of n + E, a byte
 * and the tile counts per blob, plus the sort's own; count only: 8 bytes per blob.
 *
 * k2h_amd_ralledata_reach.  edge_off, child and rep are the outputs of _subkeys over the same
 * n (trusted as such; a child or rep entry >= n is taken as ~0); roots is a byte per blob.
 * Start set: {rep[i] : roots[i] != 0, rep[i] != ~0} -- a root that is an earlier copy of a key
 * stands for the key's last copy, a root that is a non-participant for nothing.  A
 * level-synchronous frontier traversal follows child from there.  Only blobs that are their own
 * rep are followed: earlier copies of a key are not in the table, and their lists do not exist.
 * A blob is visited once; total work is O(n + E).
 *
 *   reach[i]  (n, required) rep[i] != ~0 and rep[i] was visited: every copy of a reached key is
 *             marked, so keep = ~reach cannot resurrect a removed key from an earlier duplicate
 *   counts    (host, 3 entries, required) blobs with reach 1; levels run; converged (1 or 0)
 *   max_levels  0: no limit.  Else at most that many levels are run; when the frontier is not
 *             empty then, converged is 0 and reach marks a subset of the closure.
 *
 * A level is one kernel over the current frontier and one 8-byte read-back of the next
 * frontier's size through pinned host memory.  `stream` is synchronised once for the start
 * set, once per level run and once at the end: levels + 2 times.  A chain-shaped stream (every
 * blob naming the next) costs one level per link: the crafted case, which max_levels bounds.
 * K2H_AMD_EINVAL, judged on the host before any device is touched, each with its own message:
 * counts NULL; with n > 0: reach, edge_off, child, rep or roots NULL; n > 2^32 - 2.  n == 0:
 * K2H_AMD_OK, counts = 0, 0, 1, no device work.  Temporary device memory: a bit and 8 bytes per
 * blob.
 *
 * Parity: the parse is pinned by tests/golden/ralle_subkeys.json, written by the reference's
 * own K2HSubKeys (tests/golden/gen_ralle_subkeys.cc); Remove is a restatement
 * (tests/ralle_subkeys_model.py) -- libk2hash itself is not built by this project's tests. */
#define K2H_AMD_SKEY_PART 0x1u   /* participant */
#define K2H_AMD_SKEY_HAS  0x2u   /* skeys_length != 0 */
#define K2H_AMD_SKEY_BAD  0x4u   /* HAS, and the strict walk rejected the segment: no edges */

int k2h_amd_ralledata_subkeys(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                              const uint8_t* consider, uint32_t flags,
                              uint8_t* sk_flags,      /* n, required */
                              uint64_t* edge_off,     /* n+1, required */
                              uint64_t* rep,          /* n, may be NULL */
                              uint64_t* child,        /* cap entries; NULL: count only */
                              uint64_t cap,
                              uint64_t* counts,       /* host, required: participants, blobs with >= 1 edge,
                                                         BAD segments, edges E, dangling edges (0 when child NULL) */
                              void* stream);

int k2h_amd_ralledata_reach(const uint64_t* edge_off, const uint64_t* child, const uint64_t* rep, uint64_t n,
                            const uint8_t* roots, uint64_t max_levels,
                            uint8_t* reach,           /* n, required */
                            uint64_t* counts,         /* host, required: blobs reached, levels run, converged (0/1) */
                            void* stream);

/* 4b'''''''. Subkey names unlinked from a stream: the first call that rewrites blobs.  Every
 * call above keeps or drops whole blobs.  The reference's removal of a subkey,
 * K2HShm::Remove(key, subkey) with RemoveEx(pElement, bySubKey, ...) (lib/k2hshm.cc:2567-2667),
 * has two halves: it erases the name from the parent's list (K2HSubKeys::erase), serializes the
 * list again and replaces the subkeys page; only then does it remove the child with everything
 * below it.  _reach and _select are the second half; this call is the first, fused with
 * _select's keep mask, so "remove these subtrees and unlink them" is one pass over the stream.
 *
 * blobs, blob_off, keep, sk_flags, edge_off, drop, out, out_off, index and changed are device
 * pointers; counts is a host pointer.  sk_flags and edge_off are what _subkeys wrote for the same
 * stream; drop has E = edge_off[n] bytes, drop[e] != 0 leaves the entry of edge e out (NULL:
 * nothing is dropped, and the call is _select).  k2h_amd_subkeys_drop_mask makes such a mask
 * from _subkeys' child and a per-blob mask such as _reach's.
 *
 * Which blobs are emitted: exactly _select's rule.  Blob i is emitted when keep is NULL or
 * keep[i] != 0 and its span is valid (non-decreasing, ending at or before size).  Emitted
 * blobs lie back to back, in order, in out; out_off (n + 1 entries of room) receives the
 * emitted blobs' offsets plus one, starting at 0; index (may be NULL) their original indices.
 *
 * Which emitted blobs are rewritten: those with K2H_AMD_SKEY_PART and without K2H_AMD_SKEY_BAD
 * in sk_flags[i] and drop[e] != 0 for at least one e in [edge_off[i], edge_off[i+1]).  Every
 * other emitted blob is copied byte for byte, slack included; with no drop set anywhere the
 * output bytes, out_off and index equal _select's.
 *
 * The rewritten form.  The new list holds the entries of non-zero length whose edge is not
 * dropped, in segment order, as K2HSubKeys::Serialize(unsigned char**, size_t&) writes a list
 * (lib/k2hsubkeys.cc:58-111): a u64 count, then per name a u64 length and the bytes.
 * Zero-length entries are left out (K2HSubKeys::insert refuses them), bytes after the last
 * counted entry are left out, the count word is the number of entries written, and a list
 * with no entry left is no segment at all: skey_length = 0.  The blob is written in
 * GetElementToBinary's layout (lib/k2hshmdirect.cc:59-89): hash and subhash as stored; key,
 * value and attrs bytes as stored, from wherever their positions put them; key_pos = 80 and the
 * running sums, written for zero-length segments too; length exactly 80 plus the four lengths.
 * The same bytes result wherever the segments lay in the input (permuted, overlapping, with
 * gaps).  A blob left with a key and nothing else (K2H_AMD_UNLINK_KEY_ONLY) leaves no element
 * when fed (SetElementByBinArray, lib/k2hshmdirect.cc:438), where Remove(key, subkey) on the
 * table leaves an element with a key and no value.
 *
 * The call trusts nothing it can check.  With a drop mask, every emitted blob with PART and
 * without BAD in sk_flags has its header judged again by the header tests of section 4b and its
 * segment walked again by the strict rule of section 4b''''''.  It is copied unchanged and counted
 * in counts[6] when its header is no participant's, when its walk is BAD, when its walk does
 * not yield exactly edge_off[i+1] - edge_off[i] edges, or when that range is decreasing or ends
 * behind E -- whether or not a drop byte is set for it.  (A blob without PART, or with BAD, in
 * sk_flags is copied and not looked into; with drop NULL no blob is.)  Memory rule, as in
 * _subkeys: no byte of blobs outside [0, size) is read, except within the aligned 16 bytes
 * that hold a valid byte; nothing outside a blob's own segments is interpreted; all absolute
 * offsets are 64-bit.
 *
 * One departure from the reference.  For a list that is not strictly ascending the reference's
 * parse (K2HSubKeys::Serialize(const unsigned char*, size_t) through insert) would sort and
 * deduplicate; its own writer never produces such a list.  Here the order is kept and every
 * entry is judged by its own drop byte.  Detecting such lists is out of scope.
 *
 *   counts   (host, 7 entries, required) blobs emitted; bytes emitted; blobs rewritten; entries
 *            dropped; lists emptied; blobs left key-only; mismatches
 *   changed  (n, may be NULL) K2H_AMD_UNLINK_* per INPUT blob, 0 for every blob not rewritten
 *
 * Cost: a sizing pass (offsets, keep and flag bytes; with a drop mask the count pass of _subkeys
 * over again: every participant's header and one walk of its list), two scans of n + 1 entries,
 * a copy pass of the select copy's shape
 * and, only when a blob is rewritten, a pass of 8 lanes per rewritten blob that walks its list
 * once more and copies every run of consecutive kept entries as one range.  `stream` is
 * synchronised once, to return counts.  out == NULL: count only -- counts and, if given, changed
 * are filled.  counts[1] > out_cap: K2H_AMD_EINVAL with counts set and nothing written to out.
 * K2H_AMD_EINVAL, judged on the host before any device is touched, each with its own message:
 * counts NULL; with n > 0: blobs, blob_off, sk_flags or edge_off NULL; out != NULL with out_off
 * NULL; n > 2^32 - 2.  n == 0: K2H_AMD_OK, counts zeroed, out_off[0] = 0 when out_off is given,
 * no other device work.  Temporary device memory, kept per device between calls: 13 bytes per
 * blob (an 8-byte place, a 4-byte rank, a flag byte) plus the scans' own.
 *
 * k2h_amd_subkeys_drop_mask.  One kernel, asynchronous on `stream`:
 *   drop[e] = child[e] == ~0 ? dangling != 0 : gone != NULL && child[e] < n && gone[child[e]] != 0
 * child has `edges` entries (as _subkeys wrote it), gone n bytes (may be NULL), drop `edges`
 * bytes.  edges == 0 does no work.
 *
 * Parity: the rewritten list is pinned by tests/golden/ralle_unlink.json, written by the
 * reference's own K2HSubKeys::erase and Serialize (tests/golden/gen_ralle_unlink.cc);
 * Remove(key, subkey) is a restatement (tests/ralle_unlink_model.py). */
#define K2H_AMD_UNLINK_REWRITTEN 0x1u  /* the blob's list was re-serialized              */
#define K2H_AMD_UNLINK_EMPTIED   0x2u  /* ... and no name was left: skey_length is now 0 */
#define K2H_AMD_UNLINK_KEY_ONLY  0x4u  /* ... and the blob now has a key and nothing else */

int k2h_amd_ralledata_unlink(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                             const uint8_t* keep,      /* n, or NULL: every blob */
                             const uint8_t* sk_flags,  /* n,     as _subkeys wrote it */
                             const uint64_t* edge_off, /* n + 1, as _subkeys wrote it */
                             const uint8_t* drop,      /* E = edge_off[n] bytes: != 0 leaves edge e's entry out */
                             void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* index,
                             uint8_t* changed,         /* n, may be NULL: K2H_AMD_UNLINK_* per INPUT blob, 0 otherwise */
                             uint64_t* counts,         /* host, 7 entries, required */
                             void* stream);

int k2h_amd_subkeys_drop_mask(const uint64_t* child, uint64_t edges, const uint8_t* gone, uint64_t n,
                              int dangling, uint8_t* drop, void* stream);

/* 4c. Blobs straight from scanned records: the middle of a bulk load whose file is already
 * in device memory.  The device scans of section 5 (k2h_amd_import_scan_device,
 * k2h_amd_archive_scan_device and their _scan_prehash_device forms) report every record as
 * offsets and lengths into the file; these two calls turn such records into the blobs of
 * section 4 without a CSR copy of the payload in between.  (The record types are declared
 * in section 5.)
 *
 * file, recs, out and blob_off are device pointers; blob_off has n+1 entries and is
 * required; total is a host pointer and is required.  Blobs are packed back to back in
 * record order: blob i = out[blob_off[i], blob_off[i+1]), blob_off[0] = 0, *total =
 * blob_off[n].  A record that yields no blob contributes 0 bytes (blob_off[i+1] ==
 * blob_off[i]); there is no separate index array.  That is exactly a stream
 * k2h_amd_ralledata_check / _select accept (a 0-byte blob is BAD_SPAN there).
 *
 * k2h_amd_import_ralledata: every record yields a blob that holds the two C strings
 * K2HShm::Set(const char*, const char*) stores and hashes (lib/k2hshm.cc:2081-2083):
 *   key    = file[key_off, key_off+key_len) followed by one 0x00 byte, key_length = key_len+1
 *   value  = file[val_off, val_off+val_len) followed by one 0x00 byte, val_length = val_len+1
 *   skey_length = attrs_length = 0
 *   key_pos = 80, val_pos = 80 + key_length, skey_pos = attrs_pos = val_pos + val_length
 *   hash / subhash = k2h_hash / k2h_second_hash of key + NUL (the values of
 *   k2h_amd_import_prehash); an empty key gives the 1-byte key "\0" with subhash == hash.
 * The 0x00 bytes are written, never copied (the file byte after a key is a TAB or a
 * newline).  A record is skipped (0 bytes) when its key range or its value range is not
 * inside [0, size): off <= size && len <= size - off per range (recs are the caller's).
 *
 * k2h_amd_archive_ralledata: a record yields a blob only when status == 0, type == 0
 * (SCOM_SET_ALL, the one record type that is a whole element, lib/k2harchive.cc:328-329),
 * key_len > 0 (lib/k2hshmdirect.cc:355) and its key, value, subkeys and attrs ranges are
 * each inside the file (the same test).  The four segments are copied as stored and hashed
 * as stored; exdata is ignored.  Every other record gives 0 bytes.  A blob with a key and
 * nothing else inserts nothing (lib/k2hshmdirect.cc:438); it is still emitted, with a
 * faithful layout.
 *
 * K2H_AMD_FLAG_STD_FNV is honoured; K2H_AMD_FLAG_CSTR returns K2H_AMD_EINVAL (the import
 * form is always key + NUL, the archive form always as stored).
 *
 * Flow: a sizing kernel and an exclusive sum fill blob_off, `stream` is synchronised once
 * to return *total, then the blobs are built asynchronously on `stream`.  out == NULL:
 * sizes only.  *total > out_cap: K2H_AMD_EINVAL with *total and blob_off set and nothing
 * written to out.  n == 0: K2H_AMD_OK, *total = 0, blob_off[0] = 0 if blob_off is given,
 * no other device work.  n so large that n * (82 + 4 * size) overflows 64 bits, a NULL
 * total, or a NULL blob_off with n > 0: K2H_AMD_EINVAL, judged on the host.
 *
 * No byte outside [0, size) of the file is read except within the aligned 16 bytes that
 * hold a valid byte, nothing of a skipped record's ranges is read, and nothing outside
 * out[0, *total) and blob_off[0..n] is written.
 *
 * Parity: the layout is pinned by the fixture of oracle/gen_ralledata.cc and the hashes by
 * the reference build of lib/k2hashfunc.cc.  That these blobs equal what
 * K2HShm::GetElementToBinary would emit after Set / ReplaceAll of the same records is a
 * restatement: libk2hash itself is not built by this project's tests. */
struct k2h_amd_import_rec;  /* section 5 */
struct k2h_amd_archive_rec; /* section 5 */
int k2h_amd_import_ralledata(const void* file, uint64_t size, const struct k2h_amd_import_rec* recs, uint64_t n,
                             void* out, uint64_t out_cap, uint64_t* blob_off, uint64_t* total, uint32_t flags,
                             void* stream);
int k2h_amd_archive_ralledata(const void* file, uint64_t size, const struct k2h_amd_archive_rec* recs, uint64_t n,
                              void* out, uint64_t out_cap, uint64_t* blob_off, uint64_t* total, uint32_t flags,
                              void* stream);

/* 4d. A stream written as a k2hash archive: the portable exit of a blob stream.  Blobs fit
 * only a table with the hash function and seed that produced their hash fields; an archive
 * stores no hashes (K2HArchive::Load, lib/k2harchive.cc:279-383, re-hashes every key through
 * ReplaceAll), so k2h_load_archive and the load command of k2hlinetool replay it into any
 * table.  K2HArchive::Save (lib/k2harchive.cc:86-257) writes one SCOM_SET_ALL record per
 * element; this call writes the same record for every participating blob, on the device.
 *
 * blobs, blob_off, keep, out and rec_off are device pointers (the stream arguments mean what
 * they mean for k2h_amd_ralledata_check); records and total are host pointers.  keep and
 * records may be NULL; total is required.
 *
 * Participants, the rule of _dedup.  Blob i yields a record when keep is NULL or keep[i] != 0,
 * its span is good (not BAD_SPAN) and its header passes the header tests of
 * k2h_amd_ralledata_check (not EMPTY, NO_KEY or BAD_RANGE).  The hash and subhash fields are
 * neither read for a decision nor verified: the archive does not store them.  A blob with a
 * key and nothing else takes part (K2HCommandArchive::Put accepts it, lib/k2hcommand.cc:71).
 *
 * The record is what K2HCommandArchive::SetAll produces for the blob's four segments
 * (lib/k2hcommand.cc:69-135, scom_init at lib/k2hcommand.h:99-113), a packed 104-byte SCOM
 * header (the layout of section 5) and the data:
 *   szCommand      "\nK2H_SET_ALL" followed by four 0x00 bytes
 *   type           0 (SCOM_SET_ALL)
 *   key_length, val_length, skey_length, attr_length   the blob's four lengths
 *   exdata_length  0
 *   key_pos = 104, val_pos = 104 + key_length, skey_pos = val_pos + val_length,
 *   attrs_pos = skey_pos + skey_length
 *   exdata_pos     104 (scom_init sets it and Put leaves it for SET_ALL)
 *   then the key, value, subkeys and attrs bytes, in that order and back to back.
 * The segment bytes are read from the blob at its *_pos fields, wherever they point inside
 * the blob: order, overlap and slack in the blob are not assumptions, and the pos of a
 * length-0 segment is ignored.  One SET_ALL record is written however large the value is:
 * Save splits a value above 10 MiB into SCOM_OW_VAL records, but Load has no such limit.
 *
 * Output and flow, the convention of section 4c.  Records are packed back to back in blob
 * order: the record of blob i is out[rec_off[i], rec_off[i+1]), and a blob that yields none
 * has 0 bytes there.  rec_off has n+1 entries and is required for n > 0; rec_off[0] = 0,
 * *total = rec_off[n], *records = the number of blobs that yielded a record.  out[0, *total)
 * is a file K2HArchive::Load and k2h_amd_archive_scan walk from offset 0.  A sizing kernel
 * and an exclusive sum fill rec_off, `stream` is synchronised once to return the counts, then
 * the records are built asynchronously on `stream`.  out == NULL: sizes and counts only.
 * *total > out_cap: K2H_AMD_EINVAL with *total, *records and rec_off set and nothing written
 * to out.  n == 0: K2H_AMD_OK, *total = 0, *records = 0, rec_off[0] = 0 if rec_off is given,
 * no other device work.
 *
 * K2H_AMD_EINVAL, judged on the host before any device is touched, each with its own
 * message: total NULL; rec_off, blobs or blob_off NULL with n > 0; n so large that
 * n * (104 + 4 * size) overflows 64 bits.
 *
 * No byte outside [0, size) of the stream is read except within the aligned 16 bytes that
 * hold a valid byte.  Nothing of a blob whose span is bad or whose keep byte is 0 is read,
 * and nothing beyond the header of any other blob that yields no record -- except, for both,
 * within the aligned 16 bytes they share with a participant.  Nothing outside out[0, *total)
 * and rec_off[0..n] is written;
 * bytes that share an aligned 16-byte piece with the first or last output byte keep their
 * value.  All absolute offsets are 64-bit.
 *
 * Parity: the record layout is pinned by the SET_ALL records the reference's own
 * K2HCommandArchive wrote into the archive fixture of oracle/gen_archive.cc.  That
 * K2HArchive::Load accepts the output is a restatement: libk2hash itself is not built by
 * this project's tests. */
#define K2H_AMD_SCOM_HEADER 104 /* sizeof(SCOM), packed (lib/k2hcommand.h:69-82) */
int k2h_amd_ralledata_archive(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                              const uint8_t* keep, void* out, uint64_t out_cap, uint64_t* rec_off,
                              uint64_t* records, uint64_t* total, void* stream);

/* 4d'. From two dumps to a log: the transaction log that turns a held stream into a new one.
 * The calls of section 5 read a K2HTransaction log in every useful way; this one writes it.  A is
 * the new stream (today's dump), B the held one (yesterday's); rel (na entries) and seen (nb
 * entries) are the outputs of k2h_amd_ralledata_diff over the same two streams and consider
 * masks, called without `times`.  The records are what K2HArchive::Load replays onto
 * yesterday's table to get today's, and what k2h_amd_archive_apply (section 5c) replays onto
 * yesterday's stream: the call is the inverse of that one.  All pointers are device pointers,
 * except counts.
 *
 * Slots.  A blob i is slot i, B blob j is slot na + j.  Every slot yields 0 to 3 records, back
 * to back in out[slot_off[s], slot_off[s+1]); slot_off has na + nb + 1 entries, slot_off[0] = 0.
 *   A slot without K2H_AMD_DIFF_PART   nothing.
 *   A slot with PART, without FOUND    one SET_ALL with the blob's key and its value, subkeys and
 *                                      attrs, as section 4d writes it; a key-only blob gives a
 *                                      key-only SET_ALL.
 *   A slot with PART and FOUND         one record per differ bit, in the order _VAL, _SKEY,
 *                                      _ATTRS: REPLACE_VAL(key, value), REPLACE_SKEY(key, subkeys),
 *                                      REPLACE_ATTRS(key, attrs), each with the A blob's current
 *                                      bytes of that field, which may be empty: Load clears the
 *                                      field then, which a SET_ALL cannot (K2HShm::ReplaceAll
 *                                      writes subkeys and attrs only when the record's own are
 *                                      non-empty, lib/k2hshm.cc:2948-2950).  No differ bit: nothing.
 *   B slot j                           one DEL_KEY(key) when seen[j] == 0 and b_consider is NULL
 *                                      or b_consider[j] != 0.
 * seen == NULL means no deletions: nothing of B is read, and b_blobs / b_off may be NULL.
 * _REPEAT, _APPLY and _DATA are ignored.
 *
 * The rule is right when each stream has one participant per identity, as a dump has: two
 * new-key copies in A would give two SET_ALLs of which the second cannot clear what the first
 * set, and an earlier copy in B has seen == 0 and would delete a key A still has.  A caller whose
 * streams may repeat an identity reduces each to the last copy first and passes that as the
 * consider masks of the diff and as b_consider here (INTEGRATION.md 2c''').
 *
 * Record bytes: exactly what K2HCommandArchive::Put writes for the type (lib/k2hcommand.cc:69-135,
 * scom_init at lib/k2hcommand.h:99-113).  The header is packed and 104 bytes long: szCommand
 * "\nK2H_SET_ALL", "\nK2H_REP_VAL", "\nK2H_REP_SKEY", "\nK2H_REP_ATTRS" or "\nK2H_DEL_KEY",
 * NUL-padded to 16; the type; the five lengths, 0 for what the type does not carry; key_pos = 104,
 * the carried segment's position right behind the key (SET_ALL: the three behind each other), and
 * 104 for every position the type does not carry, exdata_pos included.  The key and the carried
 * bytes follow.
 *
 * Memory safety does not rest on rel or seen.  The writer judges every blob it is about to read
 * again: its span lies inside [0, size) and has at least 80 bytes, and its header passes the
 * header tests of k2h_amd_ralledata_check (not EMPTY, NO_KEY or BAD_RANGE).  A slot whose bits
 * ask for a record but whose blob fails that test yields nothing and is counted as refused.
 * Segments are read at their *_pos wherever they lie inside the blob; the pos of a length-0
 * segment is ignored.
 *
 *   made[s]  (na + nb entries, may be NULL) a bit per record the slot yielded, K2H_AMD_DELTA_*.
 *   counts   (host, 8 entries, required) records, bytes, then the records per type -- SET_ALL,
 *            REPLACE_VAL, REPLACE_SKEY, REPLACE_ATTRS, DEL_KEY -- and the refused slots.
 *
 * Flow, the convention of section 4d: a sizing pass and two exclusive sums, `stream` is
 * synchronised once to return counts, then the records are built asynchronously on `stream`.
 * out == NULL: sizes, made and counts only (slot_off may then be NULL too).  counts[1] >
 * out_cap: K2H_AMD_EINVAL with counts, slot_off and made set and nothing written to out.
 * na + nb == 0: K2H_AMD_OK, counts zeroed, slot_off[0] = 0 if slot_off is given.
 *
 * K2H_AMD_EINVAL, judged on the host before any device is touched, each with its own message:
 * counts NULL; rel NULL with na > 0; A's blobs or offsets NULL with na > 0; B's blobs or offsets
 * NULL with nb > 0 and seen given; slot_off NULL with out given and na + nb > 0; na + nb >
 * 2^32 - 2 (the emitting slots are ranked in 32 bits, and no launch grid would fit).
 *
 * No byte outside [0, size) of either stream is read except within the aligned 16 bytes that
 * hold a valid byte; nothing of a slot that asks for no record, nothing of a blob whose span is
 * bad, and nothing beyond the header of any other blob that is refused.  Nothing outside
 * out[0, counts[1]), slot_off[0 .. na + nb] and made[0, na + nb) is written; bytes that share an
 * aligned 16-byte piece with the first or last output byte keep their value.  All absolute
 * offsets are 64-bit.
 *
 * Cost: one byte per slot for the slots that ask for nothing, a 64-byte header read for the
 * others, two scans over na + nb entries, and a build pass over the emitting slots alone, 8 lanes
 * each.  Temporary device memory, kept per device between calls: 9 bytes per slot (17 without
 * slot_off) plus the scans' own.
 *
 * Parity: the record layout is pinned by the records of all these types that the reference's own
 * K2HCommandArchive wrote into the archive fixture of oracle/gen_archive.cc.  That
 * K2HArchive::Load, replaying the output onto the held table, leaves the new one is shown against
 * a transliteration of Load (tests/test_ralledata_delta.py); libk2hash itself is not built by this
 * project's tests, so parity with it is a restatement.  It holds for tables without builtin attrs
 * and without history, the preconditions of section 5c. */
#define K2H_AMD_DELTA_SET_ALL 0x01u
#define K2H_AMD_DELTA_REPLACE_VAL 0x02u
#define K2H_AMD_DELTA_REPLACE_SKEY 0x04u
#define K2H_AMD_DELTA_REPLACE_ATTRS 0x08u
#define K2H_AMD_DELTA_DEL_KEY 0x10u
int k2h_amd_ralledata_delta(const void* a_blobs, uint64_t a_size, const uint64_t* a_off, uint64_t na,
                            const uint8_t* rel, const void* b_blobs, uint64_t b_size, const uint64_t* b_off,
                            uint64_t nb, const uint8_t* b_consider, const uint8_t* seen, void* out, uint64_t out_cap,
                            uint64_t* slot_off, uint8_t* made, uint64_t* counts, void* stream);

/* 4e. Keys looked up in a held stream: index, find and fetch.  Every call above feeds, routes,
 * rewrites or compares a stream; these three answer what it holds for a key.  Together they are
 * K2HShm::Get(const unsigned char*, size_t, unsigned char**, bool checkattr, ...)
 * (lib/k2hshm.cc:1857-1938) for a batch of keys, answered from a stream in device memory with
 * no table: the element is reached as GetElement reaches it and as SetElementByBinArray does
 * (lib/k2hshmdirect.cc:373-378) -- K2H_HASH_FUNC / K2H_2ND_HASH_FUNC of the key, then hash,
 * subhash, key length, key bytes, the identity of section 4b'.  The held side is sorted once, by
 * _index, and probed many times, by _find; _fetch is the inverse of k2h_amd_build_ralledata for
 * one segment.  All pointers are device pointers unless marked host; every call runs on `stream`.
 *
 * k2h_amd_ralledata_index.  Participants, as in section 4b': consider NULL or consider[i] != 0,
 * a span inside [0, size) of at least 80 bytes, a header that is not EMPTY, NO_KEY or BAD_RANGE.
 * The index is opaque, caller-owned device memory of k2h_amd_ralledata_index_size(n) bytes (host
 * arithmetic only; about 44 bytes per blob: the hashes sorted on their low bits, the blob of each
 * sorted position, a 32-byte record per blob, and a 256-byte header that is written last) at a
 * 256-byte aligned address.  It is library output and is trusted by _find, as a stream's stored
 * hashes are trusted by section 4b'; it is valid for exactly the (blobs, size, blob_off, n) bytes
 * it was built from.  *participants (host, may be NULL) receives their number: given, `stream` is
 * synchronised once to return it; NULL, nothing waits for the device.  n == 0 is valid and gives
 * an index in which nothing is found.
 *   K2H_AMD_EINVAL, judged on the host before any device is touched, each with its own message:
 *   blobs or blob_off NULL with n > 0; index NULL; index_cap below the size function's value;
 *   index not 256-byte aligned; n > 2^32 - 2 (indices are sorted as 32-bit values).
 *   Cost: dedup's gather, compact and sort, and no resolve.  Temporary device memory, kept per
 *   device between calls: 13 bytes per blob, the tile counts and the sort's own.
 *
 * k2h_amd_ralledata_find.  The m queries are a CSR column: query i = keys[key_off[i],
 * key_off[i+1]), m + 1 offsets.  Query i takes part when key_off[i] <= key_off[i+1] <= key_bytes
 * and it has at least one byte; with K2H_AMD_FLAG_CSTR a query of any length takes part and
 * stands for its bytes plus one NUL that the buffer does not hold, as Get(const char*) passes
 * strlen + 1 (every blob of the import route stores such keys).  Its hashes are h1[i] / h2[i] or,
 * with both NULL, what k2h_amd_hash_csr gives for it under `flags`; K2H_AMD_FLAG_STD_FNV is legal
 * only then, _CSTR either way.  Its lookup length L is its length, plus 1 with _CSTR.  Each query
 * is judged alone: the offsets need not be monotone from query to query.
 *   The match is the LAST participant of the stream (the choice of section 4b''''''s match) with
 * stored hash == h1, stored subhash == h2, key_length == L and the query's key bytes -- with
 * _CSTR the query's bytes and a final byte of 0.  A blob whose stored hashes are not those of its
 * key is never matched, as Get would never find it.
 *   match[i]   (m, may be NULL) the blob index, or ~0.
 *   status[i]  (m, required) K2H_AMD_FIND_* bits: _PART the query takes part; _FOUND a blob
 *              matched; _ATTRS the matched blob has attrs_length != 0; _EXPIRED only when `now`
 *              (host, may be NULL, read before the call returns) is given: the matched blob's attrs
 *              give an expire earlier than *now, the IsExpire rule of section 4b'''' -- only the
 *              attrs of matched blobs are walked.  Get(..., checkattr = true) returns a value
 *              exactly for _FOUND without _EXPIRED, up to the history marker and value
 *              decryption, which are not judged: _ATTRS lets a caller route such keys to the CPU.
 *              _BAD_INDEX: the index header's magic, n or size disagree with the arguments; then
 *              every query gets exactly this byte, match is ~0, hit stays 0 and nothing behind
 *              the header is read.
 *   hit[j]     (n, may be NULL) all n entries are written: 0 by one memset on `stream`, then 1 for
 *              every blob that is some query's match.  On a stream with one blob per identity (a
 *              dump, or the survivors of section 4b') keep = !hit followed by
 *              k2h_amd_ralledata_select is a batch Remove(key).  With several copies of an
 *              identity only the last copy is marked.
 *   counts     (host, 3 entries, may be NULL) the queries that take part, found, expired.  Given,
 *              `stream` is synchronised once to return them; NULL, nothing waits for the device.
 *   m == 0: K2H_AMD_OK, counts zeroed, hit zeroed by its memset, no kernel.  n == 0: an ordinary
 *   call in which nothing is found.
 *   K2H_AMD_EINVAL (host side, each with its own message): status NULL with m > 0; keys NULL with
 *   key_bytes > 0; key_off NULL with m > 0; index NULL; blobs or blob_off NULL with n > 0; exactly
 *   one of h1 / h2 NULL; unknown flag bits; _STD_FNV with the hashes given; n > 2^32 - 2.
 *   Memory rule: no byte outside [0, key_bytes) of keys or [0, size) of the stream is read, except
 *   within the aligned 16 bytes that hold a valid byte; nothing of a query that takes no part;
 *   all absolute offsets are 64-bit.
 *   Cost: one lane per query; about ceil(log2 P) dependent loads (P the participants) and the
 *   walk back through the run of the query's sorted hash bits -- one entry, now and then two.  r
 *   distinct identities that share the sorted bits cost O(r) per lane: the crafted-stream case of
 *   section 4b'.  Hashes not passed are computed one lane per query first.  Temporary device
 *   memory, kept per device between calls: 4 KiB of counters, and 16 bytes per query when the
 *   hashes are computed.
 *
 * k2h_amd_ralledata_fetch.  Slot i yields the chosen segment (K2H_AMD_SEG_*) of blob which[i], in
 * slot order, packed back to back: out[out_off[i], out_off[i+1]), out_off has m + 1 entries and
 * starts at 0.  take (m, or NULL: every slot).  A slot yields 0 bytes when take[i] == 0 or
 * which[i] == ~0, and 0 bytes with bad[i] = 1 (bad: m, may be NULL) when which[i] >= n, the
 * blob's span is bad or shorter than 80 bytes, or the segment's [pos, pos + length) is not inside
 * [0, blob length) -- tested without forming a sum that can wrap; the pos of a length-0 segment
 * is ignored.  No other header test is made: a blob's segments may be permuted, gapped or
 * overlapping, as section 5c accepts.  Repeated indices are legal: the blob is copied twice.
 *   out == NULL: count only; *total (host, required), and out_off and bad if given, are filled.
 *   *total > out_cap: K2H_AMD_EINVAL with total set and nothing written to out.  `stream` is
 *   synchronised exactly once per call, to return total, then the bytes are copied asynchronously
 *   on `stream`; with m == 0 nothing waits for the device.
 *   K2H_AMD_EINVAL (host side, each with its own message): total NULL; which NULL with m > 0;
 *   blobs or blob_off NULL with n > 0 and m > 0; an unknown segment; out given without out_off.
 *   Memory rule: that of _find for the stream; only the segments' own bytes are read, and nothing
 *   of out at or beyond *total is written.
 *   Cost: a 16-byte header read per slot, one scan over m + 1 entries, and a copy pass: 16 lanes
 *   per slot in 16-byte pieces, a slot of 4 KiB or more by a whole block.  Temporary device
 *   memory, kept per device between calls: 16 bytes per slot plus the scan's own.
 *
 * Parity: libk2hash is not built by this project's tests, so parity with Get is a restatement
 * against the Python model of tests/ralle_find_model.py, whose lookup is shown to agree with
 * "feed the blobs in order, the last one wins". */
#define K2H_AMD_FIND_PART 0x01u
#define K2H_AMD_FIND_FOUND 0x02u
#define K2H_AMD_FIND_ATTRS 0x04u
#define K2H_AMD_FIND_EXPIRED 0x08u
#define K2H_AMD_FIND_BAD_INDEX 0x80u
#define K2H_AMD_SEG_KEY 0u
#define K2H_AMD_SEG_VAL 1u
#define K2H_AMD_SEG_SKEY 2u
#define K2H_AMD_SEG_ATTRS 3u
uint64_t k2h_amd_ralledata_index_size(uint64_t n);
int k2h_amd_ralledata_index(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                            const uint8_t* consider, void* index, uint64_t index_cap, uint64_t* participants,
                            void* stream);
int k2h_amd_ralledata_find(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n, const void* index,
                           const void* keys, uint64_t key_bytes, const uint64_t* key_off, uint64_t m,
                           const uint64_t* h1, const uint64_t* h2, uint32_t flags, const k2h_amd_timespec* now,
                           uint64_t* match, uint8_t* status, uint8_t* hit, uint64_t* counts, void* stream);
int k2h_amd_ralledata_fetch(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                            const uint64_t* which, uint64_t m, const uint8_t* take, uint32_t segment, void* out,
                            uint64_t out_cap, uint64_t* out_off, uint8_t* bad, uint64_t* total, void* stream);

/* ---------------------------------------------------------------------------
 * 5. Bulk key streams: keys anywhere in a buffer, and k2hash archives.
 *
 * k2h_amd_hash_ranges hashes key i = base[starts[i], starts[i] + lens[i]) (device
 * pointers).  With K2H_AMD_FLAG_CSTR each key is hashed as the C string that
 * K2HShm::Set(const char*, ...) stores (lib/k2hshm.cc:2081-2083): the range plus a
 * terminating NUL (strlen + 1 bytes) -- the form k2himport's TSV / mdbm loaders use
 * (tests/k2himport.cc:81-112).  The call synchronises `stream` once (to size the
 * staging buffer the keys are packed into).
 *
 * k2h_amd_archive_scan walks a k2hash archive (K2HArchive::Save / Load,
 * lib/k2harchive.cc:82-383; record = packed 104-byte SCOM header + data,
 * lib/k2hcommand.h:64-79: char szCommand[16]; int64 type; uint64 key / val / skey / attr /
 * exdata length; int64 key / val / skey / attrs / exdata position from the record's start;
 * the next record starts 104 + the five lengths later) as Load does and reports each record; recs may be NULL to
 * count only.  k2h_amd_archive_prehash_host then hashes every record's key on the GPU
 * (and, if new_h1/new_h2 are given, the new key of each SCOM_RENAME record), so a
 * loader can have all hashes before applying record one.  Host pointers.
 * ------------------------------------------------------------------------- */
#define K2H_AMD_FLAG_CSTR 0x2u /* hash each key as key + NUL (K2HShm::Set(const char*)) */

int k2h_amd_hash_ranges(const void* base, const uint64_t* starts, const uint64_t* lens, uint64_t n, uint64_t* h1,
                        uint64_t* h2, uint32_t flags, void* stream);

#define K2H_AMD_ARCHIVE_BAD_TYPE 1  /* type outside SCOM_TYPE_MIN..MAX (Load: skip / fail) */
#define K2H_AMD_ARCHIVE_TRUNCATED 2 /* a data segment runs past the end of the file */
typedef struct k2h_amd_archive_rec {
  int64_t type;    /* SCOM_SET_ALL .. SCOM_RENAME (lib/k2hcommand.h:47-55) */
  uint64_t offset; /* record start in the file */
  uint64_t key_off, key_len, val_off, val_len, skey_off, skey_len, attrs_off, attrs_len, exdata_off, exdata_len;
  /* absolute offsets in the file */
  int32_t status;  /* 0, K2H_AMD_ARCHIVE_BAD_TYPE or K2H_AMD_ARCHIVE_TRUNCATED (device scan: or NO_MAGIC) */
  int32_t reserved;
} k2h_amd_archive_rec;

int k2h_amd_archive_scan(const void* file, uint64_t size, k2h_amd_archive_rec* recs, uint64_t cap,
                         uint64_t* count);
int k2h_amd_archive_prehash_host(const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t count,
                                 uint64_t* h1, uint64_t* h2, uint64_t* new_h1, uint64_t* new_h2, uint32_t flags,
                                 int device);

/* The same scan and prehash for an archive already in device memory (file, recs, h1 ...:
 * device pointers; count: host), with no host pass (k2hash_amd/csrc/k2h_archive_dev.hip).
 *
 * k2h_amd_archive_scan_device returns the records k2h_amd_archive_scan returns for the
 * same bytes -- field for field, in file order, same count / cap convention (recs may be
 * NULL to count only; more records than cap: K2H_AMD_EINVAL with *count set and nothing
 * written past cap) -- and synchronises `stream`.  size < 104: *count = 0, no device work.
 * It finds the record starts by the string every record's szCommand begins with,
 * SCOM_COMSTR_PREFIX "\nK2H_" (lib/k2hcommand.h:36-45; K2HCommandArchive always writes it,
 * lib/k2hcommand.cc:116-186), and resolves which of those places lie on the chain of
 * records from offset 0; the same bytes inside a value are on no chain and change nothing.
 * The one difference from the host scan: where the chain arrives at an offset at which a
 * whole header fits but whose first five bytes are not that string, that record is
 * reported with its fields filled in as usual and status K2H_AMD_ARCHIVE_NO_MAGIC (before
 * BAD_TYPE and TRUNCATED), it is the last record and is counted, and the call returns
 * K2H_AMD_OK.  (Load does not look at szCommand, so the host scan walks on; the reference's
 * writer never produces such a file.)  A file whose offset 0 holds no prefix gives that one
 * record.  K2H_AMD_EINVAL also for a file with 2^32 - 2 or more such places.
 *
 * k2h_amd_archive_prehash (async on `stream`) hashes every record's key as stored, read
 * straight from the device-resident file, one lane per record: h1 = k2h_hash, h2 =
 * k2h_second_hash (an empty key: 0); new_h1 / new_h2 the same of the exdata segment for
 * SCOM_RENAME records (type 6), 0 for every other record.  h2, new_h1 and new_h2 may each
 * be NULL.  A record with status != 0 gets zeros, and so does one whose key range is not
 * inside [0, size) (recs are the caller's: off <= size && len <= size - off is checked
 * again and nothing outside the file is read).  K2H_AMD_FLAG_STD_FNV selects the std-FNV
 * seed; K2H_AMD_FLAG_CSTR returns K2H_AMD_EINVAL (archive keys are hashed as stored).
 *
 * k2h_amd_archive_scan_prehash_device does both in one call, the hashes from the kernel
 * that writes the records; h1 (required with recs), h2, new_h1, new_h2 need room for cap
 * entries; count / cap / errors as k2h_amd_archive_scan_device. */
#define K2H_AMD_ARCHIVE_NO_MAGIC 3 /* device scan only: no "\nK2H_" where the chain arrives */

int k2h_amd_archive_scan_device(const void* file, uint64_t size, k2h_amd_archive_rec* recs, uint64_t cap,
                                uint64_t* count, void* stream);
int k2h_amd_archive_prehash(const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n,
                            uint64_t* h1, uint64_t* h2, uint64_t* new_h1, uint64_t* new_h2, uint32_t flags,
                            void* stream);
int k2h_amd_archive_scan_prehash_device(const void* file, uint64_t size, k2h_amd_archive_rec* recs, uint64_t cap,
                                        uint64_t* count, uint64_t* h1, uint64_t* h2, uint64_t* new_h1,
                                        uint64_t* new_h2, uint32_t flags, void* stream);

/* 5b. A transaction archive folded to the records that still matter: log compaction by the
 * rule of K2HArchive::Load, for a log already in device memory.  K2HTransaction writes such a
 * log from a live table: Set emits SET_ALL (lib/k2hshm.cc:2314), Remove DEL_KEY (:2711),
 * ReplaceValue / ReplaceSubkeys / AddSubkey / ReplaceAttrs emit REPLACE_VAL / REPLACE_SKEY /
 * REPLACE_ATTRS (:3099-3123), direct access OW_VAL, Rename RENAME.  The blob route
 * (k2h_amd_archive_ralledata + k2h_amd_ralledata_dedup) is for Save outputs only: it turns
 * nothing but SET_ALL into blobs, so a key set and then removed comes back, and its whole-blob
 * rule is SetElementByBinArray's, not Load's.  Device pointers only (file, recs, h1, keep, by);
 * dropped is a host pointer.
 *
 * The rule.  Per key a table element is (exists, V, S, A).  Load's switch
 * (lib/k2harchive.cc:328-363) goes through K2HShm::ReplaceAll (lib/k2hshm.cc:2948-2950),
 * K2HShm::Replace (:2973-3036), ReplacePage (:3168-3225) and Remove(key, false) (:2544-2560,
 * RemoveEx :2789-2820).  Each record type writes a set of fields W:
 *   SET_ALL         V always (an empty value clears it), S if skey_length > 0, A if
 *                   attr_length > 0
 *   REPLACE_VAL / REPLACE_SKEY / REPLACE_ATTRS
 *                   {V} / {S} / {A} (empty data clears the field; a missing key is created with
 *                   only that field)
 *   DEL_KEY         {V, S, A} (the element is freed; removing an absent key succeeds, :2817-2819)
 *   OW_VAL, RENAME  barriers: always kept, nothing folds across them
 *
 * Participants.  Record i takes part when status == 0, type is in 0..6, key_len >= 1 and the
 * key range is inside [0, size) (off <= size && len <= size - off, checked again on the device:
 * recs are the caller's).  Every other record gets keep 0: these are the records Load with
 * isErrSkip skips.
 * Identity.  Two participants address the same element when key_len and the key bytes are equal.
 * Segment.  seg(i) = the number of participants of type RENAME before i in record order.
 * Rename touches two keys and possibly more, so it is a barrier for every key.
 * Chain.  The chain of i is the later participants of i's identity in record order, cut before
 * the first one that is OW_VAL or RENAME or whose seg differs from seg(i).
 * Drop.  A participant i of type SET_ALL, REPLACE_* or DEL_KEY is dropped exactly when W(i) is a
 * subset of the union of W(j) over its chain.  A dropped i is not the last writer of any of its
 * fields and, W(i) being non-empty, not the last record of its key: at the chain record where
 * the cover completes the element is the same with and without i, and no barrier lies between.
 * So the kept records, replayed in order, leave the table that the whole log leaves, from any
 * prior table.  [SET_ALL(k, v1, skeys = S), SET_ALL(k, v2, skeys = "")] keeps both records
 * (Load gives (v2, S)); [SET_ALL, DEL_KEY] keeps only the delete.
 *
 * Preconditions.  The table has no builtin attributes and no history switched on (otherwise
 * Set on a missing key adds attrs of its own and Remove renames for history).  The subkeys and
 * attrs segments are ones K2HSubKeys / K2HAttrs::Serialize accept, as the library's writer
 * produces them.  Parity with Load is a restatement: libk2hash itself is not built by this
 * project's tests (it needs libfullock).  Merging a key's surviving records into one SET_ALL
 * is not done (here: section 5c does it, k2h_amd_archive_apply with an empty held stream).
 *
 *   h1       (n entries, may be NULL) k2h_hash of each key, as k2h_amd_archive_prehash gives it.
 *            Only a grouping key: identity is always decided on key length and key bytes, and
 *            values that are equal for different keys only cost time.  Records of equal keys
 *            must carry equal values (any function of the key bytes will do, all zeros included);
 *            records of one key under different values are not brought together.  NULL: the
 *            call computes it (default seed) by the prehash path.
 *   keep[i]  (n entries, required) 0 for a non-participant and for a dropped participant, else 1
 *   by[i]    (n entries, may be NULL) the nearest later participant of i's identity, barrier or
 *            not, in any seg; ~0 when there is none, and for a non-participant
 *   *dropped (host, may be NULL) the number of dropped participants
 *
 * n == 0: K2H_AMD_OK, *dropped = 0, no device work.  K2H_AMD_EINVAL, judged on the host before
 * any device is touched, each with its own message: keep, file or recs NULL with n > 0;
 * n > 2^32 - 2 (indices are sorted as 32-bit values).
 *
 * Stages (k2hash_amd/csrc/k2h_archive_fold.hip): a gather pass over the records, one library
 * radix sort of (h1, index) pairs on the hash's low bits, a link pass that walks to the nearest
 * later record of the same key (it reads only keys whose hash occurs more than once), and a
 * cover by pointer doubling over the chains, so that a key with a million records costs about
 * 20 rounds over 8 bytes per record and not a million dependent loads in one lane.  The host
 * reads one word after the link pass and after every cover round to learn whether a record is
 * still undecided: the call synchronises `stream` once, plus once per round -- about
 * log2 of the longest run of one key's records that ends in a record left uncovered: six on the
 * measured 8 Mi-record log with a quarter rewrites, 20 for a key with a million records, at most
 * 32 -- plus once when dropped != NULL.  It is never fully asynchronous.  r DISTINCT keys
 * under one h1 cost O(r^2) key compares (wrong h1 values only).
 *
 * No byte outside [0, size) is read except within the aligned 16 bytes that hold a valid byte;
 * nothing of a record is read but its key, and nothing of a non-participant.  Temporary device
 * memory: about 72 bytes per record plus the sort's own, kept per device between calls. */
int k2h_amd_archive_fold(const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n,
                         const uint64_t* h1, uint8_t* keep, uint64_t* by, uint64_t* dropped, void* stream);

/* 5c. A transaction log applied to a held RALLEDATA stream: replication on the device.  A peer
 * holds yesterday's elements as a blob stream (section 4) and receives the log; the call gives
 * the stream that holds the new state.  It is also the merge section 5b leaves undone -- with an
 * empty held stream (na = 0) the output is one blob per surviving key, so a log with REPLACE_*
 * and DEL_KEY records becomes a snapshot, which k2h_amd_archive_ralledata (SET_ALL only) cannot
 * give.  All pointers are device pointers except counts and stop.
 *
 * Stop.  *stop is the index of the first record with consider[i] != 0, status == 0 and type
 * OW_VAL or RENAME; n when there is none.  Such a record with a bad status or consider[i] == 0
 * does not count.  Only the prefix [0, stop) is the log for everything below: records at or
 * behind stop are not applied and leave no trace.  OW_VAL and RENAME are not executed on the
 * device by this call; k2h_amd_archive_barrier (section 5d) executes that one record on this
 * call's output, and the caller calls again with the rest of the log and that stream.
 *
 * Participants.  Record i takes part by the rule of 5b (status 0, type 0..6, key_len >= 1, key
 * range inside [0, size), checked on the device) and also needs consider[i] != 0 and i < stop.
 * Held blob j takes part by the rule of 4b''''' (a span inside [0, held_size) of at least 80
 * bytes; header not EMPTY, NO_KEY or BAD_RANGE) and also needs held_keep[j] != 0.  A held blob
 * with held_keep[j] == 0 or a bad span is not emitted at all; one with a good span that is kept
 * but takes no part is copied through unchanged.
 *
 * Identity is (hash, subhash, key length, key bytes).  A blob uses its stored fields, trusted
 * as in _dedup and _diff; a record uses h1[i] and h2[i].  With h1 == h2 == NULL the call
 * computes both by the prehash path (k2h_amd_archive_prehash; flags: K2H_AMD_FLAG_STD_FNV or 0,
 * and 0 when the hashes are given).  Unlike 5b's h1 these values are no mere grouping key: they
 * end up in the output headers and must be those of the table's hash function.  A held blob
 * whose stored hashes are not those of its key is never matched, as Load would never find it.
 *
 * The rule.  Per identity the prior element is the (V, S, A) of the LAST held participant of
 * that identity; earlier held copies of an identity, touched by a record or not, are left out
 * of the output and counted as superseded.  The final element is what Load's switch
 * (lib/k2harchive.cc:328-341) leaves after the identity's participant records in log order,
 * under the preconditions of 5b.  In last-writer terms: walk the identity's records from the
 * last one backwards.  A DEL_KEY ends the walk with every field still open empty, and with the
 * element absent when no later record wrote.  SET_ALL supplies V always, S and A only when its
 * own are non-empty; REPLACE_* supplies its one field, empty data clears it.  Fields still open
 * at the start come from the prior element.  An identity with an applied record whose last one
 * is no DEL_KEY exists, even with all three fields empty.  A record's data segment whose range
 * is not inside [0, size) is taken as empty.
 *
 * Output.  Two parts, back to back; out_off has counts[0] + 1 entries and starts at 0.
 *   part 1  in held order: every kept, good-span held blob that takes no part, and the deciding
 *           blob of every identity that no applied record touches; byte for byte, slack
 *           included.  It equals k2h_amd_ralledata_select of the held stream under
 *           keep[j] = (touched[j] == 0).
 *   part 2  one blob per touched identity whose final element exists, in the order of the
 *           identities' last applied records, each in GetElementToBinary's layout
 *           (lib/k2hshmdirect.cc:59-89): the identity's hash and subhash; key_pos = 80 and the
 *           running sums, written for zero-length segments too; length exactly 80 plus the four
 *           lengths.  Segment bytes are read from wherever their source puts them: a record's
 *           file ranges, or a held blob's permuted, gapped or overlapping segments.  Part 2 on
 *           its own is the incremental dump.  A part-2 blob with a key and nothing else leaves
 *           no element when fed (SetElementByBinArray, lib/k2hshmdirect.cc:438), where Load
 *           leaves an element with a key and no value (as in 4b''''''').
 *
 *   origin[k]   (counts[0] entries, may be NULL) j for a part-1 blob; na + i for a part-2 blob,
 *               i the identity's last applied record
 *   touched[j]  (na entries, may be NULL) 0: emitted unchanged; K2H_AMD_APPLY_TOUCHED: the
 *               deciding blob of an identity with applied records -- whatever is left of it is
 *               in part 2; K2H_AMD_APPLY_SUPERSEDED: an earlier copy; K2H_AMD_APPLY_LEFT_OUT:
 *               not kept, or a bad span
 *   counts      (host, 7 entries, required) blobs emitted; bytes emitted; part-1 blobs; held
 *               blobs touched; held blobs superseded; touched identities left absent; records
 *               applied
 *   stop        (host, required)
 *
 * `stream` is synchronised exactly once per call, to return counts and stop (never when
 * na == 0 and n == 0).  out == NULL: count only -- counts, stop and, if given, touched are filled.
 * counts[1] > out_cap: K2H_AMD_EINVAL with counts, stop and touched set and nothing written to
 * out, out_off or origin.  K2H_AMD_EINVAL, judged on the host before any device is touched, each
 * with its own message: counts or stop NULL; held or held_off NULL with na > 0; file or recs
 * NULL with n > 0; out given without out_off; exactly one of h1 / h2 NULL; flags other than
 * K2H_AMD_FLAG_STD_FNV, or any flag with the hashes given; na + n > 2^32 - 2.
 * na == 0 && n == 0: K2H_AMD_OK, counts and stop zeroed, out_off[0] = 0 when out_off is given.
 * n == 0, or stop == 0: the call is _select of the held stream without its superseded copies.
 *
 * A consider mask from k2h_amd_archive_fold is valid only if the fold saw exactly the records
 * [0, stop): it drops a record because of LATER records of its key, which may lie behind the
 * stop.  Without a mask the result is the same -- the fold never drops a key's last record, so
 * the anchors do not move -- but a key with r applied records then costs a backward walk of up
 * to r steps in one lane (the walk ends as soon as V, S and A are covered, so a long run of
 * SET_ALLs is cheap and a head REPLACE_SKEY before a long run of REPLACE_VALs is not).  r
 * DISTINCT identities that share the sorted hash bits cost O(r) steps per lane (wrong or
 * crafted hashes only, the case 4b'''' documents).
 *
 * Memory rule as in 5b and 4b''''': no byte outside [0, held_size) of the held stream or
 * [0, size) of the file is read, except within the aligned 16 bytes that hold a valid byte;
 * all absolute offsets are 64-bit.  Temporary device memory, kept per device between calls:
 * about 69 bytes per held blob and record, 16 more per record and 16 more when the call hashes
 * the keys, plus the sort's own. */
#define K2H_AMD_APPLY_TOUCHED 1u
#define K2H_AMD_APPLY_SUPERSEDED 2u
#define K2H_AMD_APPLY_LEFT_OUT 3u

int k2h_amd_archive_apply(const void* held, uint64_t held_size, const uint64_t* held_off, uint64_t na,
                          const uint8_t* held_keep, /* na, or NULL: every blob; _select's meaning */
                          const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n,
                          const uint8_t* consider,  /* n, or NULL: every record */
                          const uint64_t* h1, const uint64_t* h2, /* n each, both or neither */
                          uint32_t flags,           /* K2H_AMD_FLAG_STD_FNV, only when h1 / h2 are NULL */
                          void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* origin,
                          uint8_t* touched,         /* na, may be NULL */
                          uint64_t* counts,         /* host, 7 entries, required */
                          uint64_t* stop,           /* host, required */
                          void* stream);

/* 5d. The barrier record a k2h_amd_archive_apply stopped at, executed on the held stream in
 * place: OW_VAL (K2HArchive::Save writes one per 10 MiB chunk of a large value, K2HDAccess::Write
 * logs one per write) and RENAME (K2HShm::Rename, and every overwrite of a table with history).
 * All pointers are device pointers except result.
 *
 * The held stream is an arena.  Blob j is held[held_off[j], held_off[j + 1]) as in 5c; held_size
 * bytes are in use and held_off[na] == held_size; the allocation has held_cap >= held_size
 * bytes, held_off room for na + 2 entries and held_keep for na + 1.  An executed call clears
 * held_keep[j] of EVERY participant copy of the addressed identity, appends at most one blob at
 * held[held_size ...), writes held_off[na + 1] and sets held_keep[na] = 1.  Nothing else of the
 * arena is written and no copy of the stream is made: the next k2h_amd_archive_apply takes
 * na + 1 blobs with this held_keep and compacts the dead copies away, as it does for any
 * held_keep[j] == 0.  Several barrier calls may follow each other on one arena.
 *
 * Matching.  Identity and participation of held blobs are those of 5c (a good span, a header that
 * is not EMPTY, NO_KEY or BAD_RANGE, held_keep[j] != 0; stored hash, subhash, key length, then key
 * bytes); the deciding blob is the LAST participant of the identity.  Record b's old key is
 * looked up under h1[b] / h2[b], a RENAME's new key (its exdata range) under new_h1[b] /
 * new_h2[b].  The four arrays have n entries each and are given together or not at all; without
 * them the call hashes what it needs (K2H_AMD_FLAG_STD_FNV chooses the seed).  The values end up
 * in the appended header, as in 5c.
 *
 * Record b must have status == 0, consider[b] != 0 (consider NULL: every record), type OW_VAL or
 * RENAME, key_len >= 1 and its key range inside [0, size): otherwise NOT_A_BARRIER.
 *
 * result[0], the outcome.  Anything but EXECUTED changes nothing on the device.
 *   K2H_AMD_BARRIER_EXECUTED
 *   K2H_AMD_BARRIER_NOT_FOUND      RENAME: no participant has the old identity (Load fails the
 *                                  record, lib/k2hshm.cc:3389-3392)
 *   K2H_AMD_BARRIER_NEW_EXISTS     RENAME: a participant holds the new identity and the new key's
 *                                  bytes are not the old key's.  Refused: Rename does not look for
 *                                  a live element under the new key, InsertElement
 *                                  (lib/k2hshm.cc:1279-1316) appends the renamed one behind it and
 *                                  GetElement (:1196-1212) goes on finding the older one, so the
 *                                  table holds two elements under one key -- a state no stream can
 *                                  express, because in a stream the last copy wins.
 *   K2H_AMD_BARRIER_BAD_RECORD     RENAME: exdata_len == 0 (:3366) or its range outside the file.
 *                                  OW_VAL: exdata_len not in 1..8, offset < 0
 *                                  (lib/k2hdaccess.cc:266), val_len == 0 (:394), or the val or
 *                                  exdata range outside the file.  Known differences: for
 *                                  val_len == 0 the reference has created the key and stretched
 *                                  the value before it fails, this call has no side effect; an
 *                                  exdata of more than 8 bytes overflows OWVAL_EXDATA
 *                                  (lib/k2hcommand.h:90-93) on the reference's stack.
 *   K2H_AMD_BARRIER_NOT_A_BARRIER
 * For NOT_FOUND before NEW_EXISTS: Rename fails on the missing old key first.
 *
 * RENAME (lib/k2harchive.cc:361-362, lib/k2hshm.cc:3364-3502), executed: the appended blob has the
 * new key, new_h1[b] / new_h2[b], and the value and subkeys of the deciding old blob; its attrs
 * are the record's when attrs_len > 0 and the range is inside the file, otherwise the old blob's
 * (:3427-3436).  A new key with the same bytes as the old one is executed like any other.
 *
 * OW_VAL (lib/k2harchive.cc:343-360, lib/k2hdaccess.cc:168-455), executed: the offset is the
 * exdata's 1..8 bytes over a zeroed off_t, little-endian.  After b the call absorbs the records
 * b + 1, b + 2, ... while each is a considered, status-0 OW_VAL with the same key length and key
 * bytes that is no BAD_RECORD, up to K2H_AMD_BARRIER_MAX_RUN records in all; the first record
 * that fails a test ends the run and is left alone.  The value is what the run's writes leave
 * when executed in log order: its length is the maximum of the old length and every
 * offset + val_len, and where writes overlap the later one wins.  A byte that neither a write nor
 * the old value covers is written as ZERO and the call is flagged K2H_AMD_BARRIER_GAP: the
 * reference stretches the value without initialising it (lib/k2hdaccess.cc:260-262, :336-351,
 * lib/k2hpagemem.cc:471-475), so those bytes are undefined there and zero is this library's
 * choice.  Subkeys and attrs are the deciding blob's.  A key that is not held is created
 * (K2HDAccess::Open, Set(key, NULL, 0)): no old value, no subkeys, no attrs, flagged
 * K2H_AMD_BARRIER_CREATED -- under 5b's precondition of a table without builtin attributes.
 *
 * The appended blob is in GetElementToBinary's layout as 5c's part 2 is: 80 bytes plus the four
 * segment lengths, the running positions written for empty segments too.  Segment bytes are
 * read from wherever the deciding blob puts them, permuted, gapped or overlapping.
 *
 *   result  (host, 8 entries, required) [0] the outcome; [1] records executed -- the caller
 *           continues at b + result[1]; [2] bytes appended; [3] K2H_AMD_BARRIER_CREATED |
 *           K2H_AMD_BARRIER_GAP; [4] held copies cleared; [5] the deciding blob's index, or
 *           UINT64_MAX; [6] the final value length; [7] reserved, 0.  Any outcome but EXECUTED:
 *           [1..4], [6] and [7] are 0 and [5] is UINT64_MAX.
 *
 * With K2H_AMD_BARRIER_COUNT_ONLY nothing on the device is written and result is complete.
 * Without it, result[2] > held_cap - held_size returns K2H_AMD_EINVAL with result set and nothing
 * written, held_keep included.  `stream` is synchronised exactly once per call, to return result.
 * K2H_AMD_EINVAL, judged on the host before any device is touched, each with its own message:
 * result NULL; held_keep NULL; held or held_off NULL with na > 0 (or without COUNT_ONLY); file or
 * recs NULL; b >= n; held_cap < held_size; the four hash arrays neither all given nor all NULL;
 * unknown flags; K2H_AMD_FLAG_STD_FNV with the hashes given; na > 2^32 - 2.
 *
 * Memory rule as in 5c; all absolute offsets are 64-bit.  Temporary device memory, kept per
 * device between calls: 4 bytes per held blob and about 8 KiB. */
#define K2H_AMD_BARRIER_EXECUTED 0u
#define K2H_AMD_BARRIER_NOT_FOUND 1u
#define K2H_AMD_BARRIER_NEW_EXISTS 2u
#define K2H_AMD_BARRIER_BAD_RECORD 3u
#define K2H_AMD_BARRIER_NOT_A_BARRIER 4u
#define K2H_AMD_BARRIER_CREATED 1u
#define K2H_AMD_BARRIER_GAP 2u
#define K2H_AMD_BARRIER_COUNT_ONLY 0x100u
#define K2H_AMD_BARRIER_MAX_RUN 256

int k2h_amd_archive_barrier(void* held, uint64_t held_size, uint64_t held_cap, uint64_t* held_off, uint64_t na,
                            uint8_t* held_keep,            /* na + 1, in/out, required */
                            const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n,
                            uint64_t b,                    /* the record to execute, b < n */
                            const uint8_t* consider,       /* n, or NULL: every record */
                            const uint64_t* h1, const uint64_t* h2, const uint64_t* new_h1, const uint64_t* new_h2,
                            uint32_t flags,                /* K2H_AMD_FLAG_STD_FNV | K2H_AMD_BARRIER_COUNT_ONLY */
                            uint64_t* result,              /* host, 8 entries, required */
                            void* stream);

/* k2himport inputs (tests/k2himport.cc:74-117): k2h_amd_import_scan splits a TSV
 * (key TAB value NEWLINE) or mdbm_export file (five header lines ending "HEADER=END",
 * then key line / value line) into records exactly as the tool's std::getline loops
 * do, and reports each key and value as the C string K2HShm::Set(const char*, const
 * char*) stores (lib/k2hshm.cc:2081-2083): *_len = strlen, i.e. cut at a NUL byte.
 * recs may be NULL to count only; a bad mdbm header returns K2H_AMD_EINVAL (the tool
 * exits).  Faithful to getline: an mdbm key line ending at EOF reports the previous
 * record's value range (the string a failed getline leaves untouched).  k2h_amd_import_prehash_host hashes every key as key + NUL on the GPU (the
 * bytes Set hashes).  Host pointers. */
#define K2H_AMD_IMPORT_TSV 0
#define K2H_AMD_IMPORT_MDBM 1
typedef struct k2h_amd_import_rec {
  uint64_t key_off, key_len; /* absolute offset in the file, strlen of the key */
  uint64_t val_off, val_len; /* likewise for the value */
} k2h_amd_import_rec;

int k2h_amd_import_scan(const void* file, uint64_t size, int format, k2h_amd_import_rec* recs, uint64_t cap,
                        uint64_t* count);
int k2h_amd_import_prehash_host(const void* file, uint64_t size, const k2h_amd_import_rec* recs, uint64_t count,
                                uint64_t* h1, uint64_t* h2, uint32_t flags, int device);

/* The same scan for a file already in device memory (file, recs: device pointers;
 * count: host), with no host pass: record ends are the newlines of the lines that hold
 * a TAB (TSV) or every second line after the header (mdbm), found by parallel passes
 * (k2hash_amd/csrc/k2h_import_dev.hip).  Same records, same errors as
 * k2h_amd_import_scan; synchronises `stream`.  k2h_amd_import_prehash hashes every
 * record's key as key + NUL straight from the device-resident file, one lane per
 * record (async on `stream`); a record whose key range is not inside [0, size) gets
 * h1 = h2 = 0 and nothing outside the file is read. */
int k2h_amd_import_scan_device(const void* file, uint64_t size, int format, k2h_amd_import_rec* recs, uint64_t cap,
                               uint64_t* count, void* stream);
int k2h_amd_import_prehash(const void* file, uint64_t size, const k2h_amd_import_rec* recs, uint64_t n, uint64_t* h1,
                           uint64_t* h2, uint32_t flags, void* stream);
/* Both in one call: the records and, from the same kernel, h1 / h2 (h2 may be NULL) of
 * every record's key + NUL -- the prehash without a second pass over the records.  h1
 * and h2 need room for cap entries; count / cap / errors as k2h_amd_import_scan_device. */
int k2h_amd_import_scan_prehash_device(const void* file, uint64_t size, int format, k2h_amd_import_rec* recs,
                                       uint64_t cap, uint64_t* count, uint64_t* h1, uint64_t* h2, uint32_t flags,
                                       void* stream);

/* Identity / diagnostics. */
const char* k2h_amd_version(void);     /* library + kernel identity, e.g. "k2hash_amd 0.1 gfx950" */
const char* k2h_amd_strerror(int code); /* message for `code`, with the last HIP error if any */

/* Synthetic-workload generator used by bench.py and the tests (not the hash
 * path): writes bytes [byte_off, byte_off+nbytes) of the splitmix64 word stream
 * with `seed`, and CSR lengths min_len + mix(seed, first_key+i) % (max_len-min_len+1).
 * Same spec as oracle/fnv_oracle.c. */
int k2h_amd_synth_bytes(void* out, uint64_t nbytes, uint64_t seed, uint64_t byte_off, void* stream);
int k2h_amd_synth_lengths(uint32_t* lens, uint64_t n, uint64_t seed, uint64_t first_key, uint32_t min_len,
                          uint32_t max_len, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* K2HASH_AMD_H */
