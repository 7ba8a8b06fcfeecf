"""Helper for tests/test_ralledata_find.py (not a test module, not a conftest).

A plain-Python restatement of the three calls of include/k2hash_amd.h section 4e over
(bytes, offsets):

* participants: ralle_check_model.header_status, as ralle_dedup_model uses it;
* find_model: for every query a scan of the stream for the LAST participant with the query's
  identity -- hash, subhash, lookup length, bytes; expiry from ralle_times_model.is_expire;
* last_wins: the same answer by another road, "feed the blobs in order into a dict, the last one
  wins", which is what a table fed by SetElementByBinArray holds for a stream without attrs;
* fetch_model: slicing.

Device runners for the three entry points, with sentinel-filled outputs between canaries.
"""
import struct

import numpy as np

import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_times_model as tm
from ralle_check_model import M64

PART, FOUND, ATTRS, EXPIRED, BAD_INDEX = 0x01, 0x02, 0x04, 0x08, 0x80
NONE = M64
SEGS = ("key", "value", "subkeys", "attrs")


# ------------------------------------------------------------------------------- the model
def participants(buf, off, size=None, consider=None):
    """[(index, fields)] of the stream's participants, in stream order."""
    raw = bytes(buf)
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    out = []
    for i in range(len(off) - 1):
        if consider is not None and not consider[i]:
            continue
        st, f = rm.header_status(raw, off[i], off[i + 1], size)
        if st == rm.OK:
            out.append((i, f))
    return out


def query_span(key_off, i, key_bytes, cstr):
    b, e = int(key_off[i]), int(key_off[i + 1])
    return (b, e) if b <= e <= key_bytes and (cstr or e > b) else None


def find_model(buf, off, keys, key_off, h1, h2, cstr=False, now=None, size=None, consider=None):
    """(match uint64 m, status uint8 m, hit uint8 n, counts [part, found, expired])."""
    raw, kraw = bytes(buf), bytes(keys)
    off = [int(x) for x in off]
    n, m = len(off) - 1, len(key_off) - 1
    parts = participants(raw, off, size, consider)
    match, status, hit = np.full(m, NONE, np.uint64), np.zeros(m, np.uint8), np.zeros(n, np.uint8)
    counts = [0, 0, 0]
    for q in range(m):
        span = query_span(key_off, q, len(kraw), cstr)
        if span is None:
            continue
        want = kraw[span[0]:span[1]] + (b"\0" if cstr else b"")
        st, got = PART, None
        for i, f in parts:                                  # a scan: the last one that agrees stays
            if f[0] == int(h1[q]) and f[1] == int(h2[q]) and f[2] == len(want) and \
                    raw[off[i] + f[6]:off[i] + f[6] + f[2]] == want:
                got = (i, f)
        if got is not None:
            i, f = got
            st |= FOUND
            match[q], hit[i] = i, 1
            if f[5]:
                st |= ATTRS
                if now is not None and tm.is_expire(raw[off[i] + f[9]:off[i] + f[9] + f[5]], now):
                    st |= EXPIRED
        status[q] = st
        for w, bit in enumerate((PART, FOUND, EXPIRED)):
            counts[w] += bool(st & bit)
    return match, status, hit, counts


def last_wins(buf, off, size=None, consider=None):
    """{(hash, subhash, key bytes): blob index}: the participants fed in order, the last one wins."""
    raw = bytes(buf)
    table = {}
    for i, f in participants(raw, off, size, consider):
        table[dm.identity(raw, int(off[i]), f)] = i
    return table


def fetch_model(buf, off, which, segment, take=None, size=None):
    """(bytes, out_off uint64 m + 1, bad uint8 m)."""
    raw = bytes(buf)
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    n, s = len(off) - 1, SEGS.index(segment)
    parts, ooff, bad = [], [0], np.zeros(len(which), np.uint8)
    for i, w in enumerate(which):
        w, piece = int(w) & M64, b""
        if (take is None or take[i]) and w != NONE:
            ok = False
            if w < n:
                b, e = off[w], off[w + 1]
                if b <= e <= size and e - b >= rm.HEADER:
                    f = struct.unpack_from("<10Q", raw, b)
                    ln, pos = f[2 + s], f[6 + s]
                    if ln == 0:
                        ok = True
                    elif pos <= e - b and ln <= e - b - pos:
                        ok, piece = True, raw[b + pos:b + pos + ln]
            bad[i] = not ok
        parts.append(piece)
        ooff.append(ooff[-1] + len(piece))
    return b"".join(parts), np.array(ooff, np.uint64), bad


# ---------------------------------------------------------------------------- queries
def csr(keys, lead=b""):
    """Keys laid end to end after `lead`: (bytes, offsets uint64)."""
    off = np.zeros(len(keys) + 1, np.uint64)
    off[0] = len(lead)
    if keys:
        off[1:] = len(lead) + np.cumsum([len(k) for k in keys])
    return bytes(lead) + b"".join(keys), off


def hashes_of(oracle, keys, variant=0, cstr=False):
    """The oracle's (h1, h2) of each key, with its NUL when cstr."""
    if not keys:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    data, koff = csr([k + (b"\0" if cstr else b"") for k in keys])
    r1, r2 = oracle.hash_csr(np.frombuffer(data, np.uint8), koff, variant)
    return np.asarray(r1, np.uint64), np.asarray(r2, np.uint64)


# ----------------------------------------------------------------------- device runners
GUARD = 64


def _guarded(torch, cuda, count, dtype, fill):
    """A sentinel-filled device tensor of `count` entries between two guards: (whole, view)."""
    g = GUARD // np.dtype(dtype).itemsize
    whole = torch.from_numpy(np.full(count + 2 * g, fill, dtype)).to(cuda)
    return whole, whole[g:g + count], g


def _guards_intact(whole, g, count, fill, what):
    h = whole.cpu().numpy()
    assert (h[:g] == fill).all() and (h[g + count:] == fill).all(), f"{what}: written outside its entries"


def _i64(a):
    return np.asarray(a, np.uint64).astype(np.int64)


def run_index(cuda, t, size, off, consider=None, count=True):
    """k2h_amd_ralledata_index over the placed stream t: (index tensor, participants)."""
    import ctypes

    import torch

    from k2hash_amd import _native
    lib = _native.batch_lib()
    n = len(off) - 1
    doff = torch.from_numpy(_i64(off)).to(cuda)
    dcon = torch.from_numpy(np.asarray(consider, np.uint8)).to(cuda) if consider is not None else None
    need = int(lib.k2h_amd_ralledata_index_size(n))
    whole = torch.full((need + 512,), 0xC3, dtype=torch.uint8, device=cuda)
    at = (-whole.data_ptr()) % 256
    index = whole[at:at + need]
    parts = ctypes.c_uint64(77)
    p = lambda x: ctypes.c_void_p(x.data_ptr() or 1) if x is not None else None  # noqa: E731
    _native.check(lib.k2h_amd_ralledata_index(p(t), size, p(doff), n, p(dcon), p(index), need,
                                              ctypes.byref(parts) if count else None, None))
    torch.cuda.synchronize()
    tail = whole[at + need:].cpu().numpy()
    assert (tail == 0xC3).all() and (whole[:at].cpu().numpy() == 0xC3).all(), "index: written outside its bytes"
    return index, (int(parts.value) if count else None), doff


def run_find(cuda, t, size, doff, n, index, kt, key_bytes, key_off, h1=None, h2=None, flags=0, now=None, count=True,
             want_hit=True, want_match=True):
    """k2h_amd_ralledata_find into sentinel-filled, guarded outputs: (match, status, hit, counts)."""
    import ctypes

    import torch

    from k2hash_amd import _native
    lib = _native.batch_lib()
    m = len(key_off) - 1
    dko = torch.from_numpy(_i64(key_off)).to(cuda)
    d1 = torch.from_numpy(_i64(h1)).to(cuda) if h1 is not None else None
    d2 = torch.from_numpy(_i64(h2)).to(cuda) if h2 is not None else None
    mw, mv, mg = _guarded(torch, cuda, m, np.int64, 0x5A5A5A5A5A5A5A5A)
    sw, sv, sg = _guarded(torch, cuda, m, np.uint8, 0x5A)
    hw, hv, hg = _guarded(torch, cuda, n, np.uint8, 0x5A)
    counts = (ctypes.c_uint64 * 3)(7, 7, 7)
    ts = _native.Timespec(*now) if now is not None else None
    p = lambda x: ctypes.c_void_p(x.data_ptr() or 1) if x is not None else None  # noqa: E731
    _native.check(lib.k2h_amd_ralledata_find(
        p(t), size, p(doff), n, p(index), p(kt), key_bytes, p(dko), m, p(d1), p(d2), flags,
        ctypes.byref(ts) if ts is not None else None, p(mv) if want_match else None, p(sv), p(hv) if want_hit else None,
        ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64)) if count else None, None))
    torch.cuda.synchronize()
    _guards_intact(mw, mg, m, 0x5A5A5A5A5A5A5A5A, "match")
    _guards_intact(sw, sg, m, 0x5A, "status")
    _guards_intact(hw, hg, n, 0x5A, "hit")
    return (mv.cpu().numpy().view(np.uint64), sv.cpu().numpy(), hv.cpu().numpy(), list(counts) if count else None)


def assert_found(got, want, what, want_hit=True, want_match=True):
    names = [("status", 1)] + ([("match", 0)] if want_match else []) + ([("hit", 2)] if want_hit else [])
    for name, k in names:
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, f"{what}: {name} differs at {int(bad[0])}: got {got[k][bad[0]]}, want {want[k][bad[0]]}"
    if got[3] is not None:
        assert got[3] == want[3], f"{what}: counts {got[3]}, want {want[3]}"


def find_against_model(cuda, oracle, buf, off, keys, what, lead=b"", hashes="oracle", variant=0, cstr=False, now=None,
                       consider=None, shift=0, key_shift=0, tail_pad=tm.PAD):
    """index + find over the stream and the list of query keys against find_model.  hashes:
    "oracle" (passed as the caller's), None (computed inside the call) or an (h1, h2) pair."""
    data, koff = csr(keys, lead)
    h1, h2 = hashes_of(oracle, keys, variant, cstr) if hashes in ("oracle", None) else hashes
    want = find_model(buf, off, data, koff, h1, h2, cstr=cstr, now=now, consider=consider)
    t = tm.place(cuda, buf, shift, tail_pad=tail_pad)
    kt = tm.place(cuda, data, key_shift, tail_pad=tail_pad)
    index, parts, doff = run_index(cuda, t, len(buf), off, consider)
    assert parts == len(participants(buf, off, consider=consider)), what
    given = (None, None) if hashes is None else (h1, h2)
    flags = (variant if hashes is None else 0) | (2 if cstr else 0)
    got = run_find(cuda, t, len(buf), doff, len(off) - 1, index, kt, len(data), koff, given[0], given[1], flags, now)
    assert_found(got, want, what)
    return got, want


def run_fetch(cuda, t, size, doff, n, which, segment, take=None, cap=None):
    """The count call and the fill of k2h_amd_ralledata_fetch: (bytes, out_off, bad, total)."""
    import ctypes

    import torch

    from k2hash_amd import _native
    lib = _native.batch_lib()
    m = len(which)
    dw = torch.from_numpy(_i64(which)).to(cuda)
    dt = torch.from_numpy(np.asarray(take, np.uint8)).to(cuda) if take is not None else None
    ow, ov, og = _guarded(torch, cuda, m + 1, np.int64, 0x5A5A5A5A5A5A5A5A)
    bw, bv, bg = _guarded(torch, cuda, m, np.uint8, 0x5A)
    total = ctypes.c_uint64(77)
    p = lambda x: ctypes.c_void_p(x.data_ptr() or 1) if x is not None else None  # noqa: E731
    seg = SEGS.index(segment)
    _native.check(lib.k2h_amd_ralledata_fetch(p(t), size, p(doff), n, p(dw), m, p(dt), seg, None, 0, p(ov), p(bv),
                                              ctypes.byref(total), None))
    torch.cuda.synchronize()
    counted = (int(total.value), ov.cpu().numpy().copy(), bv.cpu().numpy().copy())
    tot = counted[0] if cap is None else cap
    dw_, dv, dg = _guarded(torch, cuda, tot, np.uint8, 0x5A)
    ov.fill_(0x5A5A5A5A5A5A5A5A)
    bv.fill_(0x5A)
    total.value = 77
    rc = lib.k2h_amd_ralledata_fetch(p(t), size, p(doff), n, p(dw), m, p(dt), seg, p(dv), tot, p(ov), p(bv),
                                     ctypes.byref(total), None)
    torch.cuda.synchronize()
    _guards_intact(dw_, dg, tot, 0x5A, "out")
    _guards_intact(ow, og, m + 1, 0x5A5A5A5A5A5A5A5A, "out_off")
    _guards_intact(bw, bg, m, 0x5A, "bad")
    assert (int(total.value), ) == counted[:1]
    assert (ov.cpu().numpy() == counted[1]).all() and (bv.cpu().numpy() == counted[2]).all()
    return rc, dv.cpu().numpy().tobytes(), ov.cpu().numpy().view(np.uint64), bv.cpu().numpy(), int(total.value)


def fetch_against_model(cuda, buf, off, which, segment, what, take=None, shift=0, tail_pad=tm.PAD):
    import torch
    want = fetch_model(buf, off, which, segment, take)
    t = tm.place(cuda, buf, shift, tail_pad=tail_pad)
    doff = torch.from_numpy(_i64(off)).to(cuda)
    rc, data, ooff, bad, total = run_fetch(cuda, t, len(buf), doff, len(off) - 1, which, segment, take)
    assert rc == 0, what
    assert total == len(want[0]) and (ooff == want[1]).all(), f"{what}: out_off or total differ"
    assert (bad == want[2]).all(), f"{what}: bad differs"
    assert data == want[0], f"{what}: bytes differ"
    return want
