"""k2h_amd_archive_apply above the library sort's merge-sort limit: na + n = scale_streams.N_LARGE
blobs and records.  The per-blob model (archive_apply_model.apply_model) cannot run at that size,
so the expectation comes from the columns the test wrote: one stable np.lexsort groups the entries
by identity, a group's members stand in index order, and "last held copy", "last record", "last
DEL_KEY" and "last writer of a field" are maxima over a group.  A CPU test holds that expectation
against apply_model at scale_streams.N_SMALL (one block, merge sort): the same code, only N differs.

The stream and the file are laid down with numpy: fixed field widths, two key lengths, the bytes
of every field a function of the entry that wrote it.  The file has no record headers; the call
reads nothing of a record but the ranges in recs.
"""
import types

import numpy as np
import pytest

import archive_apply_model as am
import archive_fold_model as fm
import ralle_check_model as rm
import scale_streams as ss

from k2hash_amd import archive

LEN = (4, 12, 6)             # the bytes of a value, a subkeys and an attrs field that is not empty
STRIDE, LEAD = 48, 7         # a record's row in the file: key (KW), V, S, A; the first row's offset
AT = (ss.KW, ss.KW + LEN[0], ss.KW + LEN[0] + LEN[1])
M32 = np.uint64(0xFFFFFFFF)


def content(f, g):
    """Field f as entry g (shared index space) writes it: (len(g), LEN[f]) bytes."""
    w = (g.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(f + 1)) | np.uint64(1)
    two = np.stack([w, ~w], 1).astype("<u8").view(np.uint8).reshape(-1, 16)
    return two[:, :LEN[f]]


def columns(oracle, N, seed):
    rng = np.random.default_rng([9090, seed])
    c = types.SimpleNamespace(N=N, na=N * 2 // 5)
    c.n = n = N - c.na
    na = c.na
    P = na + n // 4                                       # the identities: held ones, and some only the log knows
    long_ = rng.random(P) < 0.5
    c.key, c.klen = ss.fresh_keys(np.arange(P), long_), np.where(long_, ss.KLEN[1], ss.KLEN[0]).astype(np.int64)
    c.hash, c.sub = ss.true_hashes(oracle, c.key, c.klen)
    c.hash[rng.choice(P, min(40, P // 8), replace=False)] |= M32    # these share the sorted bits with each other
    # the held stream
    c.hid = rng.permutation(P)[:na]
    dup = rng.choice(na, max(na // 20, 3), replace=False)
    c.hid[dup] = c.hid[rng.integers(0, na, dup.size)]     # earlier or later copies of another blob's identity
    c.hkeep = (rng.random(na) < 0.97).astype(np.uint8)
    c.hbad = rng.random(na) < 0.01                        # NO_KEY: kept, copied through, never matched
    c.hf = rng.integers(0, 8, na)                         # which of V, S, A the blob has
    c.gap = rng.integers(0, 16, na)
    # the log
    c.rid = rng.integers(0, P, n)
    hot = rng.choice(n, max(n // 50, 4), replace=False)
    c.rid[hot] = c.hid[rng.integers(0, 5, hot.size)]      # five keys with many records
    c.type = rng.choice([0, 1, 2, 3, 5], n, p=[0.4, 0.25, 0.1, 0.1, 0.15]).astype(np.int64)
    c.rf = rng.integers(0, 4, n)                          # SET_ALL: subkeys (1) and attrs (2) non-empty
    c.remp = rng.random(n) < 0.1                          # the record's main field is empty
    c.cons = (rng.random(n) < 0.95).astype(np.uint8)
    c.status = np.where(rng.random(n) < 0.01, 2, 0).astype(np.int64)
    c.stop = n - min(777, n // 3)
    c.type[c.stop] = fm.OW_VAL
    c.cons[c.stop], c.status[c.stop] = 1, 0
    t, full = c.type, ~c.remp
    c.rlen = np.stack([np.where(((t == 0) | (t == 1)) & full, LEN[0], 0),
                       np.where(((t == 0) & (c.rf & 1 != 0)) | ((t == 2) & full), LEN[1], 0),
                       np.where(((t == 0) & (c.rf & 2 != 0)) | ((t == 5) & full), LEN[2], 0)], 1)
    c.w = np.stack([(t == 0) | (t == 1), ((t == 0) & (c.rlen[:, 1] > 0)) | (t == 2),
                    ((t == 0) & (c.rlen[:, 2] > 0)) | (t == 5)], 1)
    c.hlen = np.stack([np.where(c.hf >> f & 1, LEN[f], 0) for f in range(3)], 1)
    return c


def _place(rows, at, data, on):
    r = np.flatnonzero(on)
    rows[r[:, None], at[r, None] + np.arange(data.shape[1])[None, :]] = data[r]


def _blobs(hash_, sub, key, klen, lens, srcs, gap=None, nokey=None):
    """Blobs in GetElementToBinary's layout as (bytes, offsets): field f of blob k is
    content(f, srcs[k, f]) when lens[k, f] != 0."""
    m = klen.size
    gap = np.zeros(m, np.int64) if gap is None else gap
    size = rm.HEADER + klen + lens.sum(1)
    rows = np.full((m, rm.HEADER + ss.KW + sum(LEN) + 15), ss.SLACK, np.uint8)
    pos = np.stack([np.full(m, rm.HEADER), rm.HEADER + klen, rm.HEADER + klen + lens[:, 0],
                    rm.HEADER + klen + lens[:, 0] + lens[:, 1]], 1)
    head = np.concatenate([np.stack([hash_, sub], 1).astype(np.uint64), np.stack([klen], 1).astype(np.uint64),
                           lens.astype(np.uint64), pos.astype(np.uint64)], 1)
    if nokey is not None:
        head[nokey, 2] = 0
    rows[:, :rm.HEADER] = head.astype("<u8").view(np.uint8).reshape(m, rm.HEADER)
    for L in ss.KLEN:
        idx = np.flatnonzero(klen == L)
        rows[idx, rm.HEADER:rm.HEADER + L] = key[idx, :L]
    for f in range(3):
        _place(rows, pos[:, 1 + f], content(f, srcs[:, f]), lens[:, f] > 0)
    length = size + gap
    off = np.zeros(m + 1, np.int64)
    off[1:] = np.cumsum(length)
    return rows[np.arange(rows.shape[1])[None, :] < length[:, None]], off


def build(c):
    """(held bytes, held offsets, file bytes, host records, h1, h2)."""
    na, n = c.na, c.n
    own = np.repeat(np.arange(na)[:, None], 3, 1)
    held, off = _blobs(c.hash[c.hid], c.sub[c.hid], c.key[c.hid], c.klen[c.hid], c.hlen, own, c.gap, np.flatnonzero(c.hbad))
    rows = np.full((n, STRIDE), 0x7E, np.uint8)
    rows[:, :ss.KW] = c.key[c.rid]
    g = na + np.arange(n)
    for f in range(3):
        rows[:, AT[f]:AT[f] + LEN[f]] = content(f, g)
    file = np.concatenate([np.full(LEAD, 0x7E, np.uint8), rows.reshape(-1)])
    recs = np.zeros(n, archive.REC_DTYPE)
    base = LEAD + STRIDE * np.arange(n, dtype=np.uint64)
    recs["type"], recs["status"], recs["offset"] = c.type, c.status, base
    recs["key_off"], recs["key_len"] = base, c.klen[c.rid]
    for f, name in enumerate(("val", "skey", "attrs")):
        recs[name + "_off"], recs[name + "_len"] = base + np.uint64(AT[f]), c.rlen[:, f]
    return held, off, file, recs, c.hash[c.rid], c.sub[c.rid]


def expect(c):
    """What the call must answer, from the columns alone."""
    na, n, N = c.na, c.n, c.N
    part = np.concatenate([(c.hkeep != 0) & ~c.hbad, (np.arange(n) < c.stop) & (c.cons != 0) & (c.status == 0)])
    ident = np.concatenate([c.hid, c.rid])
    g = np.flatnonzero(part)                                   # ascending: a group's members stay in index order
    order, new = ss.group_sorted([ident[g]])
    s = g[order]
    starts = np.flatnonzero(new)
    grp = np.cumsum(new) - 1                                   # sorted row -> group
    rec = s >= na
    typ = np.where(rec, np.append(c.type, 0)[np.maximum(s - na, 0)], -1)
    gmax = lambda on: np.maximum.reduceat(np.where(on, s, -1), starts)  # noqa: E731
    last_held, anchor, last_del = gmax(~rec), gmax(rec), gmax(rec & (typ == fm.DEL_KEY))
    wrote = [gmax(rec & (typ != fm.DEL_KEY) & np.append(c.w[:, f], False)[np.where(rec, s - na, n)]) for f in range(3)]
    # the held side
    touched = np.where(c.hkeep != 0, 0, am.LEFT_OUT).astype(np.uint8)
    h = ~rec
    touched[s[h]] = np.where(s[h] != last_held[grp[h]], am.SUPERSEDED, np.where(anchor[grp[h]] >= 0, am.TOUCHED, 0))
    # part 2: the groups with a record whose last one is no DEL_KEY, in the order of those records
    atype = np.where(anchor >= 0, c.type[np.maximum(anchor - na, 0)], -1)
    live = np.flatnonzero((anchor >= 0) & (atype != fm.DEL_KEY))
    live = live[np.argsort(anchor[live], kind="stable")]
    srcs = np.stack([np.where(wrote[f] > last_del, wrote[f], np.where(last_del >= 0, -1, last_held))[live]
                     for f in range(3)], 1)
    lens = np.stack([np.where(srcs[:, f] < 0, 0, np.where(srcs[:, f] < na, np.append(c.hlen[:, f], 0)[np.minimum(srcs[:, f], na)],
                                                        np.append(c.rlen[:, f], 0)[np.clip(srcs[:, f] - na, 0, n)]))
                     for f in range(3)], 1)
    pid = c.rid[anchor[live] - na]
    p2, p2off = _blobs(c.hash[pid], c.sub[pid], c.key[pid], c.klen[pid], lens, np.maximum(srcs, 0))
    counts_tail = [int((touched == am.TOUCHED).sum()), int((touched == am.SUPERSEDED).sum()),
                   int(((anchor >= 0) & (atype == fm.DEL_KEY)).sum()), int(part[na:].sum())]
    return types.SimpleNamespace(touched=touched, p2=p2, p2off=p2off, origin2=anchor[live], tail=counts_tail, stop=c.stop)


def whole(c, e, held, off):
    """The expectation as the model gives it: out, out_off, origin, counts."""
    keep = np.flatnonzero(e.touched == 0)
    data, soff, index = rm.select_model(held, off, e.touched == 0)
    out = np.concatenate([data, e.p2])
    ooff = np.concatenate([soff.astype(np.int64), soff[-1].astype(np.int64) + e.p2off[1:]])
    origin = np.concatenate([index.astype(np.int64), e.origin2])
    assert (index == keep).all()
    return out, ooff, origin, [len(origin), out.size, len(index)] + e.tail


# ------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("N", ss.N_SMALL)
def test_expectation_against_the_model(oracle, N):
    c = columns(oracle, N, N)
    held, off, file, recs, h1, h2 = build(c)
    e = expect(c)
    out, ooff, origin, counts = whole(c, e, held, off)
    m = am.apply_model(held.tobytes(), off, c.hkeep, fm.recs_of(file.tobytes(), recs), c.cons, h1, h2)
    assert m.stop == e.stop and m.counts == counts
    assert (m.touched == e.touched).all() and (m.out_off.view(np.int64) == ooff).all()
    assert (m.origin.view(np.int64) == origin).all() and m.out == out.tobytes()
    # every role is there: superseded copies, absent keys, fields from held blobs and from records, shared sorted bits
    assert min(counts[3:]) > 0 and m.stepped["bits"] > 0 and counts[2] > 0 and counts[0] > counts[2]


# ------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_above_the_merge_sort_limit(cuda, oracle):
    N = ss.N_LARGE
    assert N > ss.MERGE_SORT_LIMIT and N % 256
    c = columns(oracle, N, 1)
    held, off, file, recs, h1, h2 = build(c)
    e = expect(c)
    out, ooff, origin, counts = whole(c, e, held, off)
    got = am.run_apply(cuda, held.tobytes(), off, recs, file.tobytes(), keep=c.hkeep, consider=c.cons, h1=h1, h2=h2)
    rc, gout, gooff, gorigin, gtouched, gcounts, gstop = got
    assert rc == 0 and gstop == e.stop and gcounts == counts
    assert (gtouched == e.touched).all() and (gooff.view(np.int64) == ooff).all() and (gorigin.view(np.int64) == origin).all()
    assert gout == out.tobytes()
