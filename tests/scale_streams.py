"""Helper for tests/test_scale_streams.py, tests/test_sort_regimes.py and tests/test_find_regimes.py
(not a test module, not a conftest): streams of a million blobs or records, built with numpy, and
what the sort-based calls must answer on them, derived from the columns the generator wrote; for
k2h_amd_ralledata_find also the queries (find_queries) and their answer (find_expect).

The per-blob builders (dm.blobs_of, sm.blobs_with_lists, archive_fold_model.scom_record) give one
template per kind of blob or record; the template is tiled and the key bytes, the value, the names
and the stored hashes are overwritten in place.  Offsets are a cumulative sum with 0-15 slack bytes
behind every blob.  The hashes are the oracle's (hash_fixed over the key array).

The expectation never runs a per-blob loop and never looks at the bytes: identities are grouped with
one stable np.lexsort over the columns (stored hash, stored subhash, key length, key words), so a
group's members stand in stream order; "nearest later copy" is the next member, "last held copy" the
group's maximum, a child the last participant whose stored hashes are the name's true ones.
tests/test_scale_streams.py holds every expectation against the transliterated model of its call
(dm.dedup_model, fm.diff_model, sm.edges_model and sm.reach_model, archive_fold_model.fold_model) at
sizes on both sides of the library sort's one-block limit; the same code path, only n differs.

sort_regimes() reads the two limits of the library sort from the rocPRIM headers of the ROCm that
builds the library.
"""
import os
import re
import types

import numpy as np

import archive_fold_model as af
import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_diff_model as fm
import ralle_subkeys_model as sm
from ralle_check_model import ROOT

NONE = np.uint64(rm.M64)
M32 = np.uint64(0xFFFFFFFF)
KLEN = (11, 21)          # the two key lengths; 21 bytes are two 16-byte compare chunks
KW = 24                  # bytes of a key column row: three words, zero behind the key
FILL = bytes((7 * j + 3) & 0xFF for j in range(KW))
VLEN = 4
ATTRS = b"\x01attrs"     # the attrs segment of a blob that has one; its first byte is overwritten
SLACK = 0xC7             # the slack bytes between blobs
LIST_SIZES = (0, 1, 2, 8)
ONE_BLOCK = 1024         # pairs the library sort gives to one block,
MERGE_SORT_LIMIT = 1 << 20   # and to its merge sort: restated, held against the headers by sort_regimes()
N_LARGE = MERGE_SORT_LIMIT + 5003    # just above the limit, no multiple of 256
N_SMALL = (700, 3000)    # the sizes of the cross-check against the models: one block, merge sort


# ----------------------------------------------------------------------------- the sort's regimes
def sort_bits(n):
    """sort_bits_for of k2h_ralle_ident.h and k2h_archive_fold.hip, restated."""
    bits = (max(n - 1, 0).bit_length() + 8 + 7) // 8 * 8
    return min(max(bits, 16), 64)


def rocm_root():
    """The ROCm root as k2hash_amd/csrc/Makefile takes it: two levels above HIPCC."""
    mk = (ROOT / "k2hash_amd" / "csrc" / "Makefile").read_text()
    m = re.search(r"^HIPCC\s*\?=\s*(\S+)", mk, re.M)
    assert m, "HIPCC ?= not found in the Makefile"
    hipcc = os.environ.get("HIPCC", m.group(1))
    return os.path.dirname(os.path.dirname(hipcc))


def sort_regimes():
    """(one-block size, merge_sort_limit) of rocprim::radix_sort for a default config, parsed
    from the headers; None when they are not there."""
    inc = os.path.join(rocm_root(), "include", "rocprim", "device")
    try:
        cfg = open(os.path.join(inc, "device_radix_sort_config.hpp")).read()
        src = open(os.path.join(inc, "device_radix_sort.hpp")).read()
    except OSError:
        return None
    m = re.search(r"size_t\s+MergeSortLimit\s*=\s*(\d+)\s*\*\s*(\d+)\s*>\s*struct\s+radix_sort_config", cfg)
    assert m, "radix_sort_config's MergeSortLimit default not found"
    limit = int(m.group(1)) * int(m.group(2))
    b = re.search(r"default_block_sort_config\s*=\s*kernel_config<\s*rocprim::min\((\d+)u,[^>]*?block_size\),\s*"
                  r"rocprim::min\((\d+)u,[^>]*?items_per_thread\)>", src)
    assert b, "the one-block sort's default config not found"
    assert re.search(r"size\s*\)?\s*<=\s*merge_sort_limit", src), "the merge sort's size test not found"
    return int(b.group(1)) * int(b.group(2)), limit


# --------------------------------------------------------------------------- grouping by columns
def group_sorted(cols):
    """(order, new): a stable sort of the rows by the columns (first column most significant), and
    new[k] = sorted row k begins a group of equal rows.  Stable: a group's rows keep their order."""
    order = np.lexsort(cols[::-1])
    new = np.zeros(order.size, bool)
    if order.size:
        new[0] = True
    for col in cols:
        s = col[order]
        new[1:] |= s[1:] != s[:-1]
    return order, new


def join_last(tcols, tidx, qcols):
    """Per query row the largest tidx among the table rows with equal columns, -1 without one."""
    T = tidx.size
    if qcols[0].size == 0:
        return np.zeros(0, np.int64)
    order, new = group_sorted([np.concatenate([t, q]) for t, q in zip(tcols, qcols)])
    starts = np.flatnonzero(new)
    val = np.where(order < T, np.append(tidx, -1)[np.minimum(order, T)], -1).astype(np.int64)
    best = np.maximum.reduceat(val, starts)
    out = np.empty(order.size, np.int64)
    out[order] = best[np.cumsum(new) - 1]
    return out[T:]


def next_in_group(cols, idx, n, later="nearest"):
    """by (uint64 n): for the rows idx (ascending blob indices) the nearest later row of the same
    columns, NONE without one.  later="any": the LAST row of the group instead, which differs for
    every group of three or more -- what an unstable sort could leave."""
    by = np.full(n, NONE, np.uint64)
    if idx.size < 2:
        return by
    order, new = group_sorted(cols)
    s = idx[order]
    if later == "nearest":
        same = ~new[1:]
        by[s[:-1][same]] = s[1:][same]
    else:
        starts = np.flatnonzero(new)
        ends = np.append(starts[1:], s.size) - 1
        last = ends[np.cumsum(new) - 1]
        k = np.flatnonzero(last != np.arange(s.size))
        by[s[k]] = s[last[k]]
    return by


def ident_cols(c, idx, hashes=True):
    kw = c.key.view("<u8")
    cols = [c.klen[idx], kw[idx, 0], kw[idx, 1], kw[idx, 2]]
    return ([c.hash[idx], c.sub[idx]] if hashes else []) + cols


# -------------------------------------------------------------------------------- key columns
def fresh_keys(ids, long_):
    """Key rows (len(ids) x KW) whose first 8 bytes are the id, FILL behind, cut to the length."""
    key = np.empty((ids.size, KW), np.uint8)
    key[:] = np.frombuffer(FILL, np.uint8)
    key[:, :8] = np.ascontiguousarray(ids, "<u8").view(np.uint8).reshape(-1, 8)
    key[~long_, KLEN[0]:] = 0
    key[long_, KLEN[1]:] = 0
    return key


def true_hashes(oracle, key, klen):
    h, s = np.zeros(klen.size, np.uint64), np.zeros(klen.size, np.uint64)
    for L in KLEN:
        idx = np.flatnonzero(klen == L)
        if idx.size:
            h[idx], s[idx] = oracle.hash_fixed(np.ascontiguousarray(key[idx, :L]), L)
    return h, s


def _roles(n, rng, sizes):
    """Disjoint index sets of the given sizes at random places, and the rest (sorted)."""
    perm = rng.permutation(n)
    out, at = {}, 0
    for name, k in sizes.items():
        out[name] = perm[at:at + k]
        at += k
    assert at < n // 2
    out["orig"] = np.sort(perm[at:])
    return out


def ralle_columns(oracle, n, seed):
    """The columns of a RALLEDATA stream of n blobs, with everything the scale tests ask for."""
    rng = np.random.default_rng(seed)
    m = max(n // 700, 4)
    r = _roles(n, rng, dict(rep=n // 5, hot=max(n // 350, 6), xor=2 * m, same=2 * m, subflip=m, ones=2 * m, exact=3))
    orig = r["orig"]
    long_ = rng.random(n) < 0.5
    base = fresh_keys(np.arange(n), long_)
    src = np.arange(n)
    src[r["rep"]] = rng.choice(orig, r["rep"].size)
    src[r["hot"]] = orig[0]
    for name in ("xor", "same"):                     # the second half repeats the first half's identity
        src[r[name][:m]] = rng.choice(orig, m)
        src[r[name][m:]] = src[r[name][:m]]
    src[r["subflip"]] = rng.choice(orig, m)
    src[r["ones"][m:]] = r["ones"][:m]
    src[r["exact"][1]] = r["exact"][0]
    c = types.SimpleNamespace(n=n, roles=r, src=src)
    c.key, c.klen = base[src], np.where(long_[src], KLEN[1], KLEN[0]).astype(np.int64)
    same = r["same"]                                 # another key of the same length: one byte of it changed,
    for half in (same[:m], same[m:]):                # the first (even) or the last (odd)
        c.key[half[0::2], 0] ^= 0x80
        c.key[half[1::2], c.klen[half[1::2]] - 1] ^= 0x01
    c.h_true, c.s_true = true_hashes(oracle, c.key, c.klen)
    c.hash, c.sub = c.h_true.copy(), c.s_true.copy()
    flip = np.uint64(1) << (np.uint64(32) + (np.arange(m, dtype=np.uint64) % np.uint64(32)))
    c.hash[r["xor"]] ^= np.concatenate([flip, flip])
    c.hash[same], c.sub[same] = c.h_true[src[same]], c.s_true[src[same]]
    c.sub[r["subflip"]] ^= np.uint64(1)
    c.hash[r["ones"]] |= M32
    c.hash[r["exact"]] = NONE
    # the value names the blob; half of the repeats are exact copies of their source, attrs included
    vsrc = np.arange(n)
    reps = np.concatenate([r["rep"], r["hot"]])
    exact = reps[rng.random(reps.size) < 0.5]
    vsrc[exact] = src[exact]
    c.val = np.ascontiguousarray(vsrc.astype("<u4")).view(np.uint8).reshape(n, VLEN)
    c.att = (rng.random(n) < 0.15)[vsrc]
    c.ab = rng.integers(0, 4, n).astype(np.uint8)[vsrc]
    # non-participants: not considered, no key, a key range past the blob
    out = np.concatenate([rng.choice(n, max(n // 100, 9), replace=False), r["rep"][:3], r["hot"][:3]])
    c.bad = np.zeros(n, np.uint8)
    c.consider = np.ones(n, np.uint8)
    c.consider[out[0::3]] = 0
    c.bad[out[1::3]] = 1
    c.bad[out[2::3]] = 2
    c.gap = rng.integers(0, 16, n)
    c.lsize = np.zeros(n, np.int64)
    return c


def participants(c, consider=True):
    p = c.bad == 0
    return p & (c.consider != 0) if consider else p


# ------------------------------------------------------------------------------ the blob bytes
def _put_words(rows, idx, at, words):
    rows[idx, at:at + 8] = np.ascontiguousarray(words, "<u8").view(np.uint8).reshape(-1, 8)


def build_ralle(oracle, c, lo=0, hi=None):
    """(bytes uint8, offsets int64) of blobs lo..hi of the columns; c.names (E_all x KW), when there,
    holds the names of every blob's list in blob order, c.lsize their number and c.ncls their class."""
    hi = c.n if hi is None else hi
    n = hi - lo
    g = np.arange(lo, hi)
    has_lists = hasattr(c, "names")
    width = rm.HEADER + KLEN[1] + VLEN + (8 + 8 * (8 + KLEN[1]) if has_lists else len(ATTRS)) + 15
    rows = np.full((n, width), SLACK, np.uint8)
    size = np.zeros(n, np.int64)
    cls = (c.klen[g] == KLEN[1]).astype(np.int64)
    if has_lists:
        kind = cls * 8 + np.searchsorted(LIST_SIZES, c.lsize[g]) * 2 + c.ncls[g]
        first = np.concatenate([[0], np.cumsum(c.lsize)])[g]
    else:
        kind = cls * 2 + c.att[g]
    for k in np.unique(kind):
        idx = np.flatnonzero(kind == k)
        L = KLEN[k // 8 if has_lists else k // 2]
        if has_lists:
            ls, Ln = LIST_SIZES[(k % 8) // 2], KLEN[k % 2]
            t = sm.blobs_with_lists(oracle, [FILL[:L]], [sm.serialize([FILL[:Ln]] * ls) if ls else b""],
                                    [bytes(VLEN)])[0]
        else:
            t = dm.blobs_of(oracle, [FILL[:L]], [bytes(VLEN)], None, [ATTRS if k % 2 else b""])[0]
        kpos, vpos, spos, apos = (rm.get(t, 0, f) for f in (rm.F_KPOS, rm.F_VPOS, rm.F_SPOS, rm.F_APOS))
        rows[idx, :len(t)] = np.frombuffer(bytes(t), np.uint8)
        size[idx] = len(t)
        rows[idx, kpos:kpos + L] = c.key[g[idx], :L]
        rows[idx, vpos:vpos + VLEN] = c.val[g[idx]]
        if has_lists:
            for j in range(ls):
                at = spos + 8 + j * (8 + Ln) + 8
                rows[idx, at:at + Ln] = c.names[first[idx] + j, :Ln]
        elif k % 2:
            rows[idx, apos] = c.ab[g[idx]]
    _put_words(rows, slice(None), rm.F_HASH, c.hash[g])
    _put_words(rows, slice(None), rm.F_SUBHASH, c.sub[g])
    length = size + c.gap[g]
    nokey = np.flatnonzero(c.bad[g] == 1)
    _put_words(rows, nokey, rm.F_KLEN, np.zeros(nokey.size, np.uint64))
    past = np.flatnonzero(c.bad[g] == 2)             # the key's last byte is the first byte behind the blob
    _put_words(rows, past, rm.F_KPOS, (length[past] - c.klen[g[past]] + 1).astype(np.uint64))
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(length)
    return rows[np.arange(width)[None, :] < length[:, None]], off


def blob_by_builder(oracle, c, i):
    """Blob i as the per-blob builders make it (participants only): for the byte comparison."""
    key, val = bytes(c.key[i, :c.klen[i]]), bytes(c.val[i])
    if hasattr(c, "names"):
        e0 = int(c.lsize[:i].sum())
        names = [bytes(c.names[e, :KLEN[c.ncls[i]]]) for e in range(e0, e0 + int(c.lsize[i]))]
        b = sm.blobs_with_lists(oracle, [key], [sm.serialize(names) if names else b""], [val])[0]
    else:
        b = dm.blobs_of(oracle, [key], [val], None, [bytes([c.ab[i]]) + ATTRS[1:] if c.att[i] else b""])[0]
    return bytes(dm.set_hash(b, int(c.hash[i]), int(c.sub[i])))


# -------------------------------------------------------------------------------------- dedup
def dedup_stream(oracle, n, seed):
    """(buf, off, consider, columns) of the dedup stream."""
    c = ralle_columns(oracle, n, seed)
    buf, off = build_ralle(oracle, c)
    return buf, off, c.consider, c


def dedup_expect(c, part, later="nearest"):
    """(keep, by, dropped) of the plain rule over the participants `part` (bool n)."""
    idx = np.flatnonzero(part)
    by = next_in_group(ident_cols(c, idx), idx, c.n, later)
    keep = part.astype(np.uint8)
    p = np.flatnonzero(by != NONE)
    drop = p[~c.att[p] & ~c.att[by[p].astype(np.int64)]]
    keep[drop] = 0
    return keep, by, int(drop.size)


def ralle_holds(c, part):
    """What the stream holds, counted from the columns: the claims of the issue, by name."""
    idx = np.flatnonzero(part)
    cols = ident_cols(c, idx)
    order, new = group_sorted(cols)
    gid = np.empty(idx.size, np.int64)
    gid[order] = np.cumsum(new) - 1                  # identity number per participant
    sizes = np.bincount(gid)
    by = next_in_group(cols, idx, c.n)
    has = np.flatnonzero(by != NONE)

    def split_groups(coarse):
        """Groups of equal `coarse` columns that hold more than one identity."""
        o, nw = group_sorted(coarse)
        cg = np.cumsum(nw) - 1
        g = gid[o]
        differs = np.zeros(cg[-1] + 1, bool)
        differs[cg[1:][(~nw[1:]) & (g[1:] != g[:-1])]] = True
        return int(differs.sum())
    lo = c.hash[idx] & M32
    uh = np.unique(c.h_true)
    notpart = np.flatnonzero(~part)
    live = np.zeros((1,), bool)
    if notpart.size:                                 # non-participants whose identity a participant has
        live = join_last(cols, idx, ident_cols(c, notpart)) >= 0
    z = idx[c.hash[idx] == NONE]
    return dict(
        short_keys=int((c.klen[idx] == KLEN[0]).sum()), long_keys=int((c.klen[idx] == KLEN[1]).sum()),
        repeats=int(has.size), median_distance=int(np.median(by[has].astype(np.int64) - has)) if has.size else 0,
        three_or_more=int((sizes >= 3).sum()), hot=int(sizes.max()),
        high_bits_only=split_groups([lo] + cols[1:]), same_hashes_other_key=split_groups(cols[:3]),
        other_subhash=split_groups([cols[0]] + cols[2:]),
        natural_low32=int(uh.size - np.unique(uh & M32).size),
        low32_ones=int((lo == M32).sum()), exactly_ones=int(z.size),
        exactly_ones_repeat=int((by[z] != NONE).sum()),
        not_considered=int((c.consider == 0).sum()), no_key=int((c.bad == 1).sum()), key_past=int((c.bad == 2).sum()),
        non_participants_with_a_live_identity=int(live.sum()), non_participants=int(notpart.size),
        attrs=int(c.att[idx].sum()))


# --------------------------------------------------------------------------------------- find
Q_PICK, Q_ROLE, Q_FRESH, Q_NEAR, Q_EMPTY = range(5)     # why a query is there
FIND_ROLES = ("hot", "xor", "same", "subflip", "ones", "exact")
FIND_PART, FIND_FOUND, FIND_ATTRS, FIND_EXPIRED = 0x01, 0x02, 0x04, 0x08   # include/k2hash_amd.h section 4e, restated
M_LARGE = (1 << 18) + 77     # queries over the N_LARGE stream: no multiple of 256, 4,098 waves
FIND_SEEDS = (1, 5)          # the N_LARGE find tests' columns (the dedup stream's) and queries


def find_queries(oracle, c, m, seed):
    """m queries over the columns c, in an order unrelated to the stream: q.key (m x KW key rows),
    q.klen, the CSR q.bytes and q.key_off (uint64 m + 1), and two hash pairs per query, q.stored
    (the picked blob's stored hash and subhash) and q.true (true_hashes of the query's bytes).
    q.kind says why a query is there and q.pick which blob it was taken from (-1: none):

    * Q_PICK: a blob picked uniformly, participant or not;
    * Q_ROLE: every blob of the roles hot, xor, same, subflip, ones and exact;
    * Q_FRESH: a key no blob has, stored == true;
    * Q_NEAR: a picked participant's stored hashes over its key with one byte changed, byte 0 (chunk 0
      of the compare, under its lead mask) for the first half, the last byte for the second -- by bits
      the role `same` does not use, so that no blob has the changed key;
    * Q_EMPTY: key_off[i] == key_off[i + 1], which takes no part."""
    rng = np.random.default_rng([seed, 11])
    n = c.n
    roles = np.concatenate([c.roles[name] for name in FIND_ROLES])
    n_empty, n_fresh, n_near = min(100, m // 8), m // 32, m // 32 // 2 * 2
    n_pick = m - roles.size - n_empty - n_fresh - n_near
    assert n_pick > m // 2, "m is too small for the roles"
    pick = np.concatenate([rng.integers(0, n, n_pick), roles])
    idx = np.flatnonzero(participants(c, False))
    near = idx[rng.integers(0, idx.size, n_near)]
    fresh_long = rng.random(n_fresh) < 0.5
    fresh = fresh_keys(n + np.arange(n_fresh), fresh_long)
    near_key = c.key[near].copy()
    half = n_near // 2
    near_key[:half, 0] ^= 0x40
    near_key[np.arange(half, n_near), c.klen[near[half:]] - 1] ^= 0x02
    q = types.SimpleNamespace(m=m)
    q.key = np.concatenate([c.key[pick], fresh, near_key, np.zeros((n_empty, KW), np.uint8)])
    q.klen = np.concatenate([c.klen[pick], np.where(fresh_long, KLEN[1], KLEN[0]), c.klen[near], np.zeros(n_empty, np.int64)])
    q.kind = np.repeat([Q_PICK, Q_ROLE, Q_FRESH, Q_NEAR, Q_EMPTY], [n_pick, roles.size, n_fresh, n_near, n_empty])
    q.pick = np.concatenate([pick, np.full(n_fresh, -1), near, np.full(n_empty, -1)])
    order = rng.permutation(m)
    q.key, q.klen, q.kind, q.pick = q.key[order], q.klen[order], q.kind[order], q.pick[order]
    full = np.flatnonzero(q.klen > 0)
    h, s = np.zeros(m, np.uint64), np.zeros(m, np.uint64)
    h[full], s[full] = true_hashes(oracle, q.key[full], q.klen[full])
    q.true = (h, s)
    from_blob = q.pick >= 0
    q.stored = (np.where(from_blob, c.hash[q.pick], h), np.where(from_blob, c.sub[q.pick], s))
    q.key_off = np.zeros(m + 1, np.uint64)
    q.key_off[1:] = np.cumsum(q.klen)
    q.bytes = q.key[np.arange(KW)[None, :] < q.klen[:, None]]
    return q


def find_expect(c, part, q, hashes, now=None, later="last"):
    """(match uint64 m, status uint8 m, hit uint8 n, counts [part, found, expired]) of the queries q
    under the hash pair `hashes` (q.stored or q.true) against the participants `part`: the LAST
    participant with the query's hash, subhash, key length and key bytes.  later="first": the
    EARLIEST copy instead -- what an unstable sort, or a walk in the wrong direction, could leave.

    EXPIRED is ralle_times_model.is_expire over the attrs segments the generator can write, one per
    value of c.ab.  None of them parses to an expire entry (six bytes: shorter than the count), so no
    match expires and counts[2] == 0 with `now` given; expiry itself is pinned by the planted stream
    of tests/test_ralledata_find.py, not at scale."""
    import ralle_times_model as tm
    idx = np.flatnonzero(part)
    full = np.flatnonzero(q.klen > 0)
    kw = np.ascontiguousarray(q.key[full]).view("<u8")
    qcols = [hashes[0][full], hashes[1][full], q.klen[full], kw[:, 0], kw[:, 1], kw[:, 2]]
    j = join_last(ident_cols(c, idx), idx if later == "last" else c.n - idx, qcols)
    found = j >= 0
    if later != "last":
        j = np.where(found, c.n - j, j)
    match, status, hit = np.full(q.m, NONE, np.uint64), np.zeros(q.m, np.uint8), np.zeros(c.n, np.uint8)
    status[full] = FIND_PART
    at, j = full[found], j[found]
    match[at] = j.astype(np.uint64)
    hit[j] = 1
    expires = np.array([now is not None and tm.is_expire(bytes([ab]) + ATTRS[1:], now) for ab in range(4)])
    status[at] |= (FIND_FOUND | FIND_ATTRS * c.att[j] | FIND_EXPIRED * (c.att[j] & expires[c.ab[j]])).astype(np.uint8)
    return match, status, hit, [int(full.size), int(at.size), int((status & FIND_EXPIRED != 0).sum())]


def shared_sorted_bits(c, part, bits):
    """Neighbours in the stable order of the participants by their stored hash's low `bits` bits that
    share those bits under different hashes: the entries the backward walk steps over by hash alone."""
    h = c.hash[np.flatnonzero(part)]
    mask = np.uint64((1 << bits) - 1)
    s = h[np.argsort(h & mask, kind="stable")]
    return int((((s[1:] ^ s[:-1]) & mask == 0) & (s[1:] != s[:-1])).sum())


# --------------------------------------------------------------------------------------- diff
def diff_streams(oracle, n, seed):
    """((a_buf, a_off), (b_buf, b_off), a_consider, b_consider, columns): one column set of n blobs,
    the first nb of them the held stream B, the rest the incoming stream A."""
    c = ralle_columns(oracle, n, seed)
    c.nb = n // 2 - 3
    return (build_ralle(oracle, c, c.nb, n), build_ralle(oracle, c, 0, c.nb), c.consider[c.nb:], c.consider[:c.nb], c)


def diff_expect(c, part, later="last"):
    """(rel, match, seen, counts) without times.  later="any": the FIRST held copy instead of the
    last, the perturbation."""
    nb, na = c.nb, c.n - c.nb
    b, a = np.flatnonzero(part[:nb]), nb + np.flatnonzero(part[nb:])
    j = join_last(ident_cols(c, b), b if later == "last" else nb - b, ident_cols(c, a))
    found = j >= 0
    if later != "last":
        j = np.where(found, nb - j, j)
    rel, match, seen = np.zeros(na, np.uint8), np.full(na, NONE, np.uint64), np.zeros(nb, np.uint8)
    rel[a - nb] = fm.PART | fm.DATA                  # every blob has a value
    _u, inv, cnt = np.unique(c.hash[a], return_inverse=True, return_counts=True)
    rel[(a - nb)[cnt[inv] > 1]] |= fm.REPEAT
    i, j = a[found], j[found]
    match[i - nb] = j.astype(np.uint64)
    seen[j] = 1
    vdiff = (c.val[i] != c.val[j]).any(axis=1)
    adiff = (c.att[i] != c.att[j]) | (c.att[i] & (c.ab[i] != c.ab[j]))
    rel[i - nb] |= (fm.FOUND | fm.VAL * vdiff | fm.ATTRS * adiff).astype(np.uint8)
    return rel, match, seen, [int(a.size), int(i.size), int((~vdiff & ~adiff).sum()), 0]


# ------------------------------------------------------------------------------------ subkeys
def subkeys_stream(oracle, total, seed):
    """(buf, off, consider, columns) with n + E == total: a third of the pairs are blobs.  Lists of
    0, 1, 2 and 8 names, all names of a list of one length; a name is the key of a random blob --
    blobs that store a wrong hash five times as often -- or, one in 30, of no blob."""
    n = total * 10 // 32
    c = ralle_columns(oracle, n, seed)
    rng = np.random.default_rng([seed, 1])
    part = participants(c)
    p = rng.permutation(np.flatnonzero(part))
    k = p.size // 5
    c.lsize[p[:k]], c.lsize[p[k:2 * k]] = 8, 2
    ones = total - n - 10 * k                        # the lists of one name make up the rest
    assert 0 < ones < p.size - 2 * k
    c.lsize[p[2 * k:2 * k + ones]] = 1
    c.lsize[~part] = 1                               # a list that is never read
    c.ncls = rng.integers(0, 2, n)
    owner = np.repeat(np.arange(n), c.lsize)
    E = owner.size
    wrong = np.concatenate([c.roles[x] for x in ("xor", "same", "subflip", "ones")])
    tgt = np.zeros(E, np.int64)
    for cl in (0, 1):
        pool = np.flatnonzero(c.klen == KLEN[cl])
        pool = np.concatenate([pool] + [wrong[c.klen[wrong] == KLEN[cl]]] * 5)
        e = np.flatnonzero(c.ncls[owner] == cl)
        tgt[e] = pool[rng.integers(0, pool.size, e.size)]
    c.names = c.key[tgt]
    c.dangling = rng.random(E) < 1 / 30
    d = np.flatnonzero(c.dangling)
    c.names[d] = fresh_keys(n + d, c.ncls[owner[d]] == 1)
    c.owner, c.nklen = owner, np.where(c.ncls[owner] == 1, KLEN[1], KLEN[0]).astype(np.int64)
    buf, off = build_ralle(oracle, c)
    return buf, off, c.consider, c


def subkeys_expect(oracle, c, part):
    """An Edges of the model's shape: flags, edge_off, child, rep, counts."""
    m = sm.Edges()
    idx = np.flatnonzero(part)
    m.flags = np.where(part, sm.PART | np.where(c.lsize > 0, sm.HAS, 0), 0).astype(np.uint8)
    per = np.where(part, c.lsize, 0)
    m.edge_off = np.zeros(c.n + 1, np.uint64)
    m.edge_off[1:] = np.cumsum(per)
    cols = ident_cols(c, idx)
    m.rep = np.full(c.n, NONE, np.uint64)
    m.rep[idx] = join_last(cols, idx, cols).astype(np.uint64)
    e = np.flatnonzero(part[c.owner])                # the edges that are read, in blob order
    names, nklen = c.names[e], c.nklen[e]
    h, s = true_hashes(oracle, names, nklen)
    kw = np.ascontiguousarray(names).view("<u8")
    m.child = join_last(cols, idx, [h, s, nklen, kw[:, 0], kw[:, 1], kw[:, 2]]).astype(np.uint64)  # -1: NONE
    m.counts = [int(idx.size), int((per > 0).sum()), 0, int(e.size), int((m.child == NONE).sum())]
    return m


def reach_expect(m, roots_mask, max_levels=0):
    """(reach, [reached, levels, done]): the traversal of k2h_amd_ralledata_reach level by level."""
    n = m.rep.size
    eo, child = m.edge_off.astype(np.int64), m.child
    seen = np.zeros(n, bool)
    f = m.rep[np.flatnonzero(roots_mask)]
    f = np.unique(f[f != NONE]).astype(np.int64)
    seen[f] = True
    levels, widest = 0, f.size
    while f.size and (not max_levels or levels < max_levels):
        cnt = eo[f + 1] - eo[f]
        e = np.repeat(eo[f] - (np.cumsum(cnt) - cnt), cnt) + np.arange(int(cnt.sum()))
        ch = child[e]
        ch = ch[ch != NONE].astype(np.int64)
        f = np.unique(ch[~seen[ch]])
        seen[f] = True
        levels += 1
        widest = max(widest, f.size)
    ok = m.rep != NONE
    reach = np.zeros(n, np.uint8)
    reach[ok] = seen[m.rep[ok].astype(np.int64)]
    m.widest = widest
    return reach, [int(reach.sum()), levels, 0 if f.size else 1]


# --------------------------------------------------------------------------------------- fold
SET_V, SET_VS, SET_VA, SET_VSA, REP_V, REP_S, REP_A, DEL, OW, REN = range(10)   # the record kinds
KIND_TYPE = np.array([af.SET_ALL] * 4 + [af.REPLACE_VAL, af.REPLACE_SKEY, af.REPLACE_ATTRS, af.DEL_KEY, af.OW_VAL,
                      af.RENAME])
KIND_W = np.array([af.V, af.V | af.S, af.V | af.A, af.V | af.S | af.A, af.V, af.S, af.A, af.V | af.S | af.A, 0, 0])
F_SKEY, F_ATTRS, F_EX = b"skey-6", b"attr5", b"exdata-8"


def _kind_record(kind, key, val):
    s = F_SKEY if kind in (SET_VS, SET_VSA, REP_S) else b""
    a = F_ATTRS if kind in (SET_VA, SET_VSA, REP_A, REN) else b""
    v = val if kind in (SET_V, SET_VS, SET_VA, SET_VSA, REP_V, OW) else b""
    return af.scom_record(int(KIND_TYPE[kind]), key, v, s, a, F_EX if kind in (OW, REN) else b"")


def fold_log(oracle, n, seed):
    """(data uint8, recs REC_DTYPE, h1 as the caller may pass it, columns)."""
    from k2hash_amd import archive
    rng = np.random.default_rng(seed)
    m = max(n // 700, 4)
    r = _roles(n, rng, dict(rep=n // 5, hot=n // 7, xor=m, same=m, ones=m, exact=1))
    orig = r["orig"]
    # the hot key's records lie between the RENAMEs of the log's first and last twentieth: one seg
    lo, hi = n // 20, n - n // 20
    inside = (r["hot"] >= lo) & (r["hot"] < hi)
    r["rep"], r["hot"] = np.concatenate([r["rep"], r["hot"][~inside]]), np.sort(r["hot"][inside])
    r["ren"] = np.concatenate([rng.integers(0, lo, 3), rng.integers(hi, n, 3)])
    long_ = rng.random(n) < 0.5
    base = fresh_keys(np.arange(n), long_)
    src = np.arange(n)
    src[r["rep"]] = rng.choice(np.concatenate([orig, r["xor"], r["same"], r["ones"], r["exact"]]), r["rep"].size)
    src[r["rep"][:4]] = r["exact"][0]
    src[r["hot"]] = r["hot"][0]
    src[r["ren"]] = r["ren"]
    c = types.SimpleNamespace(n=n, roles=r, src=src)
    c.key, c.klen = base[src], np.where(long_[src], KLEN[1], KLEN[0]).astype(np.int64)
    c.h_true, _s = true_hashes(oracle, c.key, c.klen)
    # h1 as a caller may pass it: any function of the key bytes.  Keys that share another key's sorted bits
    # and differ above, that share another key's whole value, whose low 32 bits are ones, and ~0
    hb = c.h_true.copy()
    t = rng.choice(orig, m)
    hb[r["xor"]] = c.h_true[t] ^ (np.uint64(1) << (np.uint64(32) + (np.arange(m, dtype=np.uint64) % np.uint64(32))))
    hb[r["same"]] = c.h_true[rng.choice(orig, m)]
    hb[r["ones"]] |= M32
    hb[r["exact"]] = NONE
    c.h1 = hb[src]
    # kinds: first records SET_ALL of every shape, repeats anything, the hot key one SET_ALL(v, s, a) and
    # REPLACE_VALs behind it
    c.kind = rng.choice([SET_V, SET_VS, SET_VA, SET_VSA], n, p=[.5, .2, .15, .15])
    rep = r["rep"]
    c.kind[rep] = rng.choice(np.arange(9), rep.size, p=[.2, .1, .1, .05, .2, .1, .1, .1, .05])
    c.kind[r["hot"]] = REP_V
    c.kind[r["hot"][0]] = SET_VSA
    c.kind[r["ren"]] = REN
    c.val = np.ascontiguousarray(np.arange(n).astype("<u4")).view(np.uint8).reshape(n, VLEN)
    out = rng.choice(np.setdiff1d(np.arange(n), r["hot"][:1]), max(n // 100, 8), replace=False)
    c.bad = np.zeros(n, np.uint8)                    # 1: status, 2: type 7, 3: no key, 4: key past the file
    for k in range(4):
        c.bad[out[k::4]] = k + 1
    c.gap = rng.integers(0, 16, n)
    width = af.SCOM + KLEN[1] + VLEN + len(F_SKEY) + len(F_ATTRS) + len(F_EX) + 15
    rows = np.full((n, width), SLACK, np.uint8)
    size = np.zeros(n, np.int64)
    recs = np.zeros(n, archive.REC_DTYPE)
    kk = c.kind * 2 + (c.klen == KLEN[1])
    for k in np.unique(kk):
        idx = np.flatnonzero(kk == k)
        L = KLEN[k % 2]
        t = _kind_record(k // 2, FILL[:L], bytes(VLEN))
        head = np.frombuffer(t[24:af.SCOM], "<u8")   # five lengths, five positions
        rows[idx, :len(t)] = np.frombuffer(t, np.uint8)
        size[idx] = len(t)
        rows[idx, af.SCOM:af.SCOM + L] = c.key[idx, :L]
        if head[1]:
            rows[idx, int(head[6]):int(head[6]) + VLEN] = c.val[idx]
        for j, name in enumerate(("key", "val", "skey", "attrs", "exdata")):
            recs[name + "_len"][idx], recs[name + "_off"][idx] = head[j], head[5 + j]
    length = size + c.gap
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(length)
    recs["type"], recs["offset"] = KIND_TYPE[c.kind], off[:-1]
    for name in ("key", "val", "skey", "attrs", "exdata"):
        recs[name + "_off"] += off[:-1].astype(np.uint64)
    recs["status"][c.bad == 1] = 1
    recs["type"][c.bad == 2] = 7
    recs["key_len"][c.bad == 3] = 0
    recs["key_off"][c.bad == 4] = off[-1] - 3        # the key's last bytes lie behind the file
    c.off = off
    return rows[np.arange(width)[None, :] < length[:, None]], recs, c.h1, c


def fold_expect(c, later="nearest"):
    """(keep, by, dropped) of the fold: per key (length and bytes) the records in log order; a run is
    a stretch of one key's records in one seg without a barrier; a record is dropped when every
    field it writes is written again later in its run."""
    part = c.bad == 0
    idx = np.flatnonzero(part)
    ren = part & (c.kind == REN)
    seg = np.cumsum(ren) - ren
    cols = ident_cols(c, idx, hashes=False)
    by = next_in_group(cols, idx, c.n, later)
    order, new = group_sorted(cols)
    s = idx[order]
    barrier = KIND_W[c.kind[s]] == 0
    newrun = new.copy()
    newrun[1:] |= (seg[s][1:] != seg[s][:-1]) | barrier[1:] | barrier[:-1]
    starts, run = np.flatnonzero(newrun), np.cumsum(newrun) - 1
    w, pos = KIND_W[c.kind[s]], np.arange(s.size)
    uncovered = np.zeros(s.size, bool)
    for bit in (af.V, af.S, af.A):
        last = np.maximum.reduceat(np.where(w & bit, pos, -1), starts)
        uncovered |= ((w & bit) != 0) & (last[run] <= pos)
    keep = np.zeros(c.n, np.uint8)
    keep[s] = barrier | uncovered
    return keep, by, int(idx.size - keep.sum())


def fold_holds(c):
    part = c.bad == 0
    idx = np.flatnonzero(part)
    cols = ident_cols(c, idx, hashes=False)
    order, new = group_sorted(cols)
    sizes = np.diff(np.append(np.flatnonzero(new), idx.size))
    hot = c.roles["hot"]
    ren = part & (c.kind == REN)
    seg = np.cumsum(ren) - ren
    uh = np.unique(c.h1[idx])                        # h1 is a function of the key: keys minus values share one
    return dict(kinds=np.bincount(c.kind[idx], minlength=10).tolist(),
                repeated_kinds=np.bincount(c.kind[np.flatnonzero(c.src != np.arange(c.n))], minlength=10).tolist(),
                hot=int(sizes.max()), hot_in_one_seg=int(np.unique(seg[hot[part[hot]]]).size == 1), segs=int(seg.max()) + 1,
                three_or_more=int((sizes >= 3).sum()), long_keys=int((c.klen[idx] == KLEN[1]).sum()),
                short_keys=int((c.klen[idx] == KLEN[0]).sum()), bad=np.bincount(c.bad, minlength=5).tolist(),
                keys_sharing_h1=int(new.sum() - uh.size), low32_shared=int(uh.size - np.unique(uh & M32).size),
                low32_ones=int(((c.h1[idx] & M32) == M32).sum()), exactly_ones=int((c.h1[idx] == NONE).sum()))
