"""Helper for tests/test_archive_apply*.py and test_apply_stream.py (not a test module, not a
conftest): the model of k2h_amd_archive_apply (include/k2hash_amd.h section 5c).

* apply_model: the rule as one sequential last-writer pass -- per identity the records walked
  from the last one backwards, every field of {V, S, A} taken from the entry that wrote it last.
  It is NOT written on top of archive_fold_model.replay: the tests hold the two against each
  other.
* table_of: what a blob stream says about the table, in the form of replay's dict, for that
  comparison; prior_held: a held stream of such a dict.
* build_log / bare_log: file bytes and host records from a list of Rec.
* run_apply: the C call into sentinel-filled, guarded outputs.

Nothing here calls the code under test except run_apply at the end, which only launches it.
"""
import ctypes
import struct
from typing import NamedTuple

import numpy as np

import archive_fold_model as fm
import ralle_check_model as rm
from archive_fold_model import DEL_KEY, OW_VAL, RENAME, REPLACE_ATTRS, REPLACE_SKEY, REPLACE_VAL, SET_ALL, Rec
from ralle_unlink_model import layout

TOUCHED, SUPERSEDED, LEFT_OUT = 1, 2, 3
HEADER = rm.HEADER
FIELD = {REPLACE_VAL: 0, REPLACE_SKEY: 1, REPLACE_ATTRS: 2}


class Model(NamedTuple):
    out: bytes
    out_off: np.ndarray   # uint64, emitted + 1
    origin: np.ndarray    # uint64, emitted
    touched: np.ndarray   # uint8, na
    counts: list          # 7
    stop: int
    stepped: dict         # per class, the identities an anchor's walk steps over: they share its sorted bits only
                          # ("bits"), its h1 ("h1"), h1 and h2 ("h1h2"), or everything but the key bytes ("klen")


def stop_of(recs, consider=None):
    for i, r in enumerate(recs):
        if (consider is None or consider[i]) and r.status == 0 and r.type in (OW_VAL, RENAME):
            return i
    return len(recs)


def supplies(r):
    """{field: bytes} a record writes -- 0: V, 1: S, 2: A -- or None for a DEL_KEY."""
    if r.type == DEL_KEY:
        return None
    if r.type == SET_ALL:      # the value always, subkeys and attrs only when its own are non-empty
        w = {0: r.val}
        if r.skey:
            w[1] = r.skey
        if r.attrs:
            w[2] = r.attrs
        return w
    f = FIELD[r.type]
    return {f: (r.val, r.skey, r.attrs)[f]}


def final_element(chain, prior, supplies=supplies):
    """(exists, V, S, A) of one identity after its applied records `chain` (in log order, not
    empty); prior: the (V, S, A) bytes of the deciding held blob, or None."""
    got, exists, deleted = {}, False, False
    for r in reversed(chain):                   # from the last record backwards
        w = supplies(r)
        if w is None:                           # DEL_KEY: every field still open is empty
            deleted = True
            break
        exists = True
        for f, data in w.items():
            got.setdefault(f, data)
        if len(got) == 3:
            break
    if not exists:
        return False, b"", b"", b""
    if not deleted and prior is not None:       # the fields still open come from the prior element
        for f in range(3):
            got.setdefault(f, prior[f])
    return (True,) + tuple(got.get(f, b"") for f in range(3))


def apply_model(held, off, keep, recs, consider, h1, h2, size=None):
    """held: the stream's bytes, off its na + 1 offsets, keep a mask or None; recs: a list of Rec
    (archive_fold_model: key None when the range is not inside the file, segments already empty
    when theirs are not); consider a mask or None; h1 / h2: the records' hashes."""
    raw = bytes(held)
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    na, n = len(off) - 1, len(recs)
    stop = stop_of(recs, consider)
    touched = np.zeros(na, np.uint8)

    # the held side: what is emitted at all, who takes part, the last participant per identity
    spans, last, fields = {}, {}, {}
    superseded = 0
    for j in range(na):
        b, e = off[j], off[j + 1]
        st, f = rm.header_status(raw, b, e, size)
        if (keep is not None and not keep[j]) or st == rm.BAD_SPAN:
            touched[j] = LEFT_OUT
            continue
        spans[j] = raw[b:e]
        if st != rm.OK:
            continue
        ident = (f[0], f[1], raw[b + f[6]:b + f[6] + f[2]])
        if ident in last:
            touched[last[ident]] = SUPERSEDED
            del spans[last[ident]]
            superseded += 1
        last[ident] = j
        fields[j] = tuple(raw[b + f[6 + s]:b + f[6 + s] + f[2 + s]] if f[2 + s] else b"" for s in (1, 2, 3))

    # the log side: the applied records per identity, in log order
    chains, order, applied = {}, {}, 0
    for i in range(stop):
        r = recs[i]
        if (consider is not None and not consider[i]) or not fm.participant(r):
            continue
        applied += 1
        ident = (int(h1[i]), int(h2[i]), bytes(r.key))
        chains.setdefault(ident, []).append(i)
        order[ident] = i

    # what an anchor's walks have to step over: identities that share its sorted hash bits
    mask = (1 << fm.sort_bits(na + n)) - 1
    runs = {}
    for ident in set(last) | set(chains):
        runs.setdefault(ident[0] & mask, []).append(ident)
    stepped = {"bits": 0, "h1": 0, "h1h2": 0, "klen": 0}
    for ident in chains:
        for other in runs[ident[0] & mask]:
            if other == ident:
                continue
            if other[0] != ident[0]:
                stepped["bits"] += 1
            elif other[1] != ident[1]:
                stepped["h1"] += 1
            elif len(other[2]) != len(ident[2]):
                stepped["h1h2"] += 1
            else:
                stepped["klen"] += 1

    part2, absent, n_touched = [], 0, 0
    for ident, anchor in sorted(order.items(), key=lambda kv: kv[1]):
        j = last.get(ident)
        if j is not None:
            touched[j] = TOUCHED
            del spans[j]
            n_touched += 1
        exists, v, s, a = final_element([recs[i] for i in chains[ident]], fields.get(j))
        if not exists:
            absent += 1
            continue
        part2.append((na + anchor, layout((ident[0], ident[1]), ident[2], v, s, a)))

    blobs = [(j, spans[j]) for j in sorted(spans)] + part2
    ooff = [0]
    for _g, b in blobs:
        ooff.append(ooff[-1] + len(b))
    out = b"".join(b for _g, b in blobs)
    counts = [len(blobs), len(out), len(spans), n_touched, superseded, absent, applied]
    return Model(out, np.array(ooff, np.uint64), np.array([g for g, _b in blobs], np.uint64), touched, counts, stop,
                 stepped)


# ----------------------------------------------------------------- tables, for the comparisons
def table_of(out, out_off):
    """{key: (V, S, A)} (None for an empty field) a blob stream leaves when every blob, key-only
    ones included, stands for its element: later blobs of a key replace earlier ones."""
    raw = bytes(out)
    t = {}
    for k in range(len(out_off) - 1):
        b, e = int(out_off[k]), int(out_off[k + 1])
        st, f = rm.header_status(raw, b, e, len(raw))
        if st != rm.OK:
            continue
        seg = [raw[b + f[6 + s]:b + f[6 + s] + f[2 + s]] if f[2 + s] else b"" for s in range(4)]
        t[seg[0]] = tuple(x or None for x in seg[1:])
    return t


def prior_held(oracle, prior, variant=0):
    """A held stream of replay's prior table {key: (V, S, A)}: (bytes, offsets), blobs in key order."""
    keys = sorted(prior)
    if not keys:
        return b"", [0]
    hs = hashes_of(oracle, keys, variant)
    blobs = [layout(hs[k], k, *(x or b"" for x in prior[k])) for k in keys]
    buf, off = rm.join(blobs)
    return bytes(buf), off


def hashes_of(oracle, keys, variant=0):
    """{key: (h1, h2)} by the oracle."""
    keys = sorted(set(keys))
    if not keys:
        return {}
    koff = np.zeros(len(keys) + 1, np.uint64)
    koff[1:] = np.cumsum([len(k) for k in keys])
    a, b = oracle.hash_csr(np.frombuffer(b"".join(keys), np.uint8), koff, variant)
    return {k: (int(x), int(y)) for k, x, y in zip(keys, a, b)}


def rec_hashes(oracle, recs, variant=0):
    """(h1, h2) uint64 arrays of a list of Rec: the key's hashes, 0 for a record without a key."""
    hs = hashes_of(oracle, [r.key for r in recs if r.key], variant)
    h1 = np.array([hs[r.key][0] if r.key else 0 for r in recs], np.uint64)
    h2 = np.array([hs[r.key][1] if r.key else 0 for r in recs], np.uint64)
    return h1, h2


# ------------------------------------------------------------------------------ the inputs
def build_log(recs, lead=0):
    """(file bytes, host records in archive.REC_DTYPE) of a list of Rec, as K2HCommandArchive::Put
    writes them, behind `lead` filler bytes; the status of each Rec is carried over."""
    from k2hash_amd import archive
    parts, at = [bytes([0x7E]) * lead], lead
    out = np.zeros(len(recs), archive.REC_DTYPE)
    for i, r in enumerate(recs):
        b = fm.record_bytes(r if 0 <= r.type <= 6 else r._replace(type=SET_ALL))   # (a bad type keeps SET_ALL's layout)
        lens = struct.unpack_from("<5Q", b, 24)
        pos = struct.unpack_from("<5q", b, 64)
        out[i]["type"], out[i]["offset"], out[i]["status"] = r.type, at, r.status
        for name, ln, p in zip(("key", "val", "skey", "attrs", "exdata"), lens, pos):
            out[i][name + "_off"], out[i][name + "_len"] = at + p, ln
        parts.append(b)
        at += len(b)
    return b"".join(parts), out


def bare_log(recs, keys_at=None):
    """A log without record headers: every segment of every Rec laid down once, in order.  The
    call reads nothing of a record but the ranges in recs, so this is as good a file and lets a
    key start at file offset 0 (keys_at: the first key's offset)."""
    from k2hash_amd import archive
    buf = bytearray(bytes([0x7E]) * (keys_at or 0))
    out = np.zeros(len(recs), archive.REC_DTYPE)
    for i, r in enumerate(recs):
        out[i]["type"], out[i]["status"] = r.type, r.status
        for name, data in (("key", r.key), ("val", r.val), ("skey", r.skey), ("attrs", r.attrs), ("exdata", r.exdata)):
            out[i][name + "_off"], out[i][name + "_len"] = len(buf), len(data)
            buf += data
    return bytes(buf), out


# ------------------------------------------------------------------------------ device side
def to_dev(cuda, buf, shift):
    """buf in a guarded allocation, `shift` bytes past a 16-byte boundary: (whole, view)."""
    import torch

    import big_offsets as bo
    w, t = bo.guarded(torch, cuda, max(len(buf), 1), shift=shift, fill=0xA5)
    if len(buf):
        t[:len(buf)] = torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(cuda)
    return w, t


def run_apply(cuda, held, off, recs, file, keep=None, consider=None, h1=None, h2=None, flags=0, cap=None,
              count_only=False, want_origin=True, want_touched=True, hshift=5, fshift=11, oshift=3, held_size=None,
              file_size=None):
    """k2h_amd_archive_apply: a count-only call, then (unless count_only) the fill into an out of
    exactly `cap` bytes (default: the counted bytes) that lies `oshift` bytes off alignment between
    guards.  held / file: bytes (placed at odd shifts between canaries) or device tensors; recs:
    host records (archive.REC_DTYPE).  Returns (rc, out bytes, out_off, origin, touched, counts,
    stop); origin / touched None when NULL was passed."""
    import torch

    import big_offsets as bo
    from k2hash_amd import _native, archive
    na, n = len(off) - 1, len(recs)
    hw = fw = None
    if not torch.is_tensor(held):
        held_size = len(held) if held_size is None else held_size
        hw, held = to_dev(cuda, held, hshift)
    if not torch.is_tensor(file):
        file_size = len(file) if file_size is None else file_size
        fw, file = to_dev(cuda, file, fshift)
    d_off = torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)
    words = np.ascontiguousarray(recs).view(np.int64).reshape(-1, archive.REC_WORDS)
    d_recs = torch.from_numpy(words.copy()).to(cuda) if n else None
    u8 = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.uint8).copy()).to(cuda)  # noqa: E731
    u64 = lambda a: None if a is None else torch.from_numpy(  # noqa: E731
        np.ascontiguousarray(a, np.uint64).view(np.int64).copy()).to(cuda)
    d_keep, d_cons, d_h1, d_h2 = u8(keep), u8(consider), u64(h1), u64(h2)
    tw, touched = bo.guarded(torch, cuda, max(na, 1), fill=0xEE)
    counts = (ctypes.c_uint64 * 7)(*[0xDEAD] * 7)
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    stop = ctypes.c_uint64(0xDEAD)
    lib = _native.batch_lib()
    p = lambda x, k=1: None if x is None or not k else ctypes.c_void_p(x.data_ptr() or 1)  # noqa: E731

    def call(o, k, oo, og):
        return lib.k2h_amd_archive_apply(p(held, na), held_size, p(d_off, na), na, p(d_keep, na), p(file, n), file_size,
                                         p(d_recs, n), n, p(d_cons, n), p(d_h1, n), p(d_h2, n), flags, o, k, oo, og,
                                         p(touched) if want_touched else None, cp, ctypes.byref(stop), bo._stream())

    def guards():
        if na:
            assert bo.guards_intact(torch, tw, touched[:na], 0xEE), "bytes outside touched written"
        else:
            assert bool((tw == 0xEE).all()), "touched written although na = 0"
        if hw is not None:
            assert bo.guards_intact(torch, hw, held, 0xA5), "the held stream's guards changed"
        if fw is not None:
            assert bo.guards_intact(torch, fw, file, 0xA5), "the file's guards changed"
    rc = call(None, 0, None, None)
    torch.cuda.synchronize()
    guards()
    first, stop1 = [int(c) for c in counts], int(stop.value)
    tch = touched[:na].cpu().numpy()
    if count_only or rc != 0:
        return rc, None, None, None, tch if want_touched else None, first, stop1
    k = first[1] if cap is None else cap
    ow, out = bo.guarded(torch, cuda, k, shift=oshift)
    fo, ooff = bo.sentinel_words(torch, cuda, na + n + 1)
    fg, origin = bo.sentinel_words(torch, cuda, max(na + n, 1))
    rc = call(p(out), k, p(ooff), p(origin) if want_origin else None)
    torch.cuda.synchronize()
    guards()
    assert bo.guards_intact(torch, ow, out), "bytes outside out written"
    got = [int(c) for c in counts]
    tch2 = touched[:na].cpu().numpy()
    if rc != 0:
        assert bool((out == bo.OUT_FILL).all()), "out written although the call failed"
        assert (fo.cpu().numpy().view(np.uint64) == np.uint64(bo.SENTINEL)).all(), "out_off written although the call failed"
        return rc, None, None, None, tch2 if want_touched else None, got, int(stop.value)
    assert got == first and int(stop.value) == stop1, f"the fill counts {got}, the count-only call {first}"
    assert np.array_equal(tch, tch2), "touched differs between the count-only call and the fill"
    if not want_touched:
        assert (tch2 == 0xEE).all(), "touched written although NULL was passed"
    e = got[0]
    a = fo.cpu().numpy().view(np.uint64)
    assert (a[e + 1:] == np.uint64(bo.SENTINEL)).all(), "out_off written past entry emitted"
    b = fg.cpu().numpy().view(np.uint64)
    assert (b[e if want_origin else 0:] == np.uint64(bo.SENTINEL)).all(), "origin written past entry emitted - 1"
    return (rc, out.cpu().numpy().tobytes(), a[:e + 1], b[:e] if want_origin else None, tch2 if want_touched else None,
            got, stop1)


def assert_applied(got, m, what):
    rc, out, ooff, origin, touched, counts, stop = got
    assert rc == 0, (what, rc)
    assert stop == m.stop, f"{what}: stop {stop}, want {m.stop}"
    assert counts == m.counts, f"{what}: counts {counts}, want {m.counts}"
    for name, g, w in (("out_off", ooff, m.out_off), ("origin", origin, m.origin), ("touched", touched, m.touched)):
        if g is None:
            continue
        assert len(g) == len(w), f"{what}: {name} has {len(g)} entries, want {len(w)}"
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert bad.size == 0, f"{what}: {name} differs at {int(bad[0])}: got {int(g[bad[0]])}, want {int(w[bad[0]])}"
    if out is not None and out != m.out:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(m.out, np.uint8)
        at = int(np.nonzero(a != b)[0][0]) if len(a) == len(b) else min(len(a), len(b))
        blob = int(np.searchsorted(m.out_off, at, side="right")) - 1
        raise AssertionError(f"{what}: out differs at byte {at} (output blob {blob}, origin {int(m.origin[blob])}, "
                             f"{at - int(m.out_off[blob])} bytes into it)")
