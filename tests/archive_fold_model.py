"""Helper for tests/test_archive_fold.py (not a test module, not a conftest): the model of
k2h_amd_archive_fold (include/k2hash_amd.h section 5b).

* scom_record: a struct.pack restatement of what K2HCommandArchive::Put writes for each of the
  seven record types (lib/k2hcommand.cc:69-201, scom_init at lib/k2hcommand.h:99-113); the test
  pins it to the 64 records the reference wrote into tests/golden/archive.k2har.
* writes / fold_model: the rule, as one sequential reverse pass with a dict per identity.
* replay: a transliteration of K2HArchive::Load with isErrSkip (lib/k2harchive.cc:296-376) over
  a dict key -> (V, S, A).  OW_VAL and RENAME are opaque readers, so that any dependence the
  barriers fail to protect shows up as a difference between two replays.

Nothing here calls the code under test except run_fold at the end, which only launches it.
"""
import ctypes
import struct
from typing import NamedTuple, Optional

import numpy as np

SET_ALL, REPLACE_VAL, REPLACE_SKEY, DEL_KEY, OW_VAL, REPLACE_ATTRS, RENAME = range(7)
SCOM = 104
NONE = (1 << 64) - 1
V, S, A = 1, 2, 4
COMMANDS = {SET_ALL: b"\nK2H_SET_ALL", REPLACE_VAL: b"\nK2H_REP_VAL", REPLACE_SKEY: b"\nK2H_REP_SKEY",
            DEL_KEY: b"\nK2H_DEL_KEY", OW_VAL: b"\nK2H_OW_VAL", REPLACE_ATTRS: b"\nK2H_REP_ATTRS",
            RENAME: b"\nK2H_REN_KEY"}   # lib/k2hcommand.h:36-45


class Rec(NamedTuple):
    """One record as the fold sees it.  key None: the key range is not inside the file."""
    type: int
    key: Optional[bytes]
    val: bytes = b""
    skey: bytes = b""
    attrs: bytes = b""
    exdata: bytes = b""
    status: int = 0


def scom_record(type, key, val=b"", skey=b"", attrs=b"", exdata=b""):
    """The bytes K2HCommandArchive::Put produces: only the segments the type carries are stored
    (lib/k2hcommand.cc:76-98), each right behind the one before it, and the positions of the
    others stay where scom_init put them, at 104."""
    carried = {SET_ALL: (val, skey, attrs, b""), REPLACE_VAL: (val, b"", b"", b""), REPLACE_SKEY: (b"", skey, b"", b""),
               REPLACE_ATTRS: (b"", b"", attrs, b""), DEL_KEY: (b"", b"", b"", b""), OW_VAL: (val, b"", b"", exdata),
               RENAME: (b"", b"", attrs, exdata)}[type]
    lens = [len(key)] + [len(x) for x in carried]
    pos, at = [SCOM], SCOM + len(key)
    for x, stored in zip(carried, _STORED[type]):
        pos.append(at if stored else SCOM)
        at += len(x)
    head = COMMANDS[type].ljust(16, b"\0") + struct.pack("<q", type) + struct.pack("<5Q", *lens) + \
        struct.pack("<5q", *pos)
    assert len(head) == SCOM
    return head + key + b"".join(carried)


# which of (val, skey, attrs, exdata) Put gives a position of its own, per type
_STORED = {SET_ALL: (1, 1, 1, 0), REPLACE_VAL: (1, 0, 0, 0), REPLACE_SKEY: (0, 1, 0, 0), REPLACE_ATTRS: (0, 0, 1, 0),
           DEL_KEY: (0, 0, 0, 0), OW_VAL: (1, 0, 0, 1), RENAME: (0, 0, 1, 1)}


def record_bytes(r: Rec):
    return scom_record(r.type, r.key, r.val, r.skey, r.attrs, r.exdata)


def participant(r: Rec):
    return r.status == 0 and 0 <= r.type <= 6 and r.key is not None and len(r.key) >= 1


def barrier(r: Rec):
    return r.type in (OW_VAL, RENAME)


def writes(r: Rec):
    """W: the fields of the element the record writes (barriers: none)."""
    if r.type == SET_ALL:      # ReplaceAll: the value always, subkeys and attrs only when non-empty (lib/k2hshm.cc:2948-2950)
        return V | (S if r.skey else 0) | (A if r.attrs else 0)
    return {REPLACE_VAL: V, REPLACE_SKEY: S, REPLACE_ATTRS: A, DEL_KEY: V | S | A}.get(r.type, 0)


def fold_model(recs):
    """(keep, by, dropped) of a list of Rec: one pass from the last record to the first.  Per
    identity the pass holds the nearest later participant and the cover of the chain that starts
    there: (seg, union of W), emptied by a barrier and useless under another seg."""
    n = len(recs)
    seg, s = [0] * n, 0
    for i, r in enumerate(recs):
        seg[i] = s
        s += participant(r) and r.type == RENAME
    keep, by, dropped = np.zeros(n, np.uint8), np.full(n, NONE, np.uint64), 0
    later, cover = {}, {}
    for i in range(n - 1, -1, -1):
        r = recs[i]
        if not participant(r):
            continue
        k = r.key
        if k in later:
            by[i] = later[k]
        later[k] = i
        cs, cu = cover.get(k, (seg[i], 0))
        if cs != seg[i]:
            cu = 0
        if barrier(r):
            keep[i] = 1
            cover[k] = (seg[i], 0)
            continue
        w = writes(r)
        if w & ~cu:
            keep[i] = 1
        else:
            dropped += 1
        cover[k] = (seg[i], cu | w)
    return keep, by, dropped


def sort_bits(n):
    """sort_bits_for of k2h_archive_fold.hip, restated: the low hash bits the (h1, index) pairs of
    n records are sorted by -- 8 more than n - 1 has, in whole bytes, at least 16."""
    bits = (max(n - 1, 0).bit_length() + 8 + 7) // 8 * 8
    return min(max(bits, 16), 64)


RENAMED = ("renamed-table",)   # the one key of a table frozen by a RENAME (no bytes key equals a tuple)


def replay(recs, prior):
    """The table K2HArchive::Load (isErrSkip) leaves: dict key -> (V, S, A), a field None when
    absent or empty.  prior: the table before."""
    t = dict(prior)
    for r in recs:
        if not (0 <= r.type <= 6) or r.status != 0:          # lib/k2harchive.cc:298-301, :310-318
            continue
        if not r.key:                                        # ReplaceAll / Replace / Remove refuse an empty key: skipped, :366-369
            continue
        v, s, a = t.get(r.key, (None, None, None))
        if r.type == SET_ALL:                                # :329 -> ReplaceAll, lib/k2hshm.cc:2948-2950
            t[r.key] = (r.val or None, r.skey or s, r.attrs or a)
        elif r.type == REPLACE_VAL:                          # :332 -> Replace, lib/k2hshm.cc:2973-3036, ReplacePage :3168-3225
            t[r.key] = (r.val or None, s, a)
        elif r.type == REPLACE_SKEY:                         # :335
            t[r.key] = (v, r.skey or None, a)
        elif r.type == REPLACE_ATTRS:                        # :338
            t[r.key] = (v, s, r.attrs or None)
        elif r.type == DEL_KEY:                              # :341 -> Remove(key, false), lib/k2hshm.cc:2544-2560, :2789-2820
            t.pop(r.key, None)
        elif r.type == OW_VAL:                               # :343-360: reads and rewrites the value in place
            if not r.exdata:
                continue                                     # :344-345
            t[r.key] = (("ow", r.key in t, v, s, a, r.val, r.exdata), s, a)
        else:                                                # :362 Rename: two keys and whatever hangs on them
            t = {RENAMED: (tuple(sorted(t.items(), key=repr)), r.key, r.exdata, r.attrs)}
    return t


def recs_of(data, recs):
    """The Rec list of host-scan records (archive.REC_DTYPE) over the file bytes `data`; a
    segment whose range is not inside the file reads as None (key) or empty."""
    size = len(data)

    def seg(off, ln):
        off, ln = int(off), int(ln)
        return bytes(data[off:off + ln]) if off <= size and ln <= size - off else None
    out = []
    for r in recs:
        out.append(Rec(int(r["type"]), seg(r["key_off"], r["key_len"]), seg(r["val_off"], r["val_len"]) or b"",
                       seg(r["skey_off"], r["skey_len"]) or b"", seg(r["attrs_off"], r["attrs_len"]) or b"",
                       seg(r["exdata_off"], r["exdata_len"]) or b"", int(r["status"])))
    return out


# ---- the alphabet of the exhaustive tests: one key, values that name their position
def letter(name, key, at):
    """Record `name` of the alphabet on `key`; `at` makes its data unlike every other record's."""
    v, s, a = b"v%d" % at, b"s%d" % at, b"a%d" % at
    return {
        "set-v": Rec(SET_ALL, key, v), "set-vs": Rec(SET_ALL, key, v, s), "set-va": Rec(SET_ALL, key, v, b"", a),
        "set-vsa": Rec(SET_ALL, key, v, s, a), "rep-v": Rec(REPLACE_VAL, key, v), "rep-s": Rec(REPLACE_SKEY, key, b"", s),
        "rep-a": Rec(REPLACE_ATTRS, key, b"", b"", a), "del": Rec(DEL_KEY, key),
        "ow": Rec(OW_VAL, key, v, b"", b"", struct.pack("<q", at)),
        "rep-v0": Rec(REPLACE_VAL, key), "rep-s0": Rec(REPLACE_SKEY, key), "rep-a0": Rec(REPLACE_ATTRS, key),
    }[name]


NINE = ("set-v", "set-vs", "set-va", "set-vsa", "rep-v", "rep-s", "rep-a", "del", "ow")
TWELVE = NINE + ("rep-v0", "rep-s0", "rep-a0")


def priors(key):
    """Four states of the key before the log: absent, V only, S only, V + S + A."""
    return {"absent": {}, "v": {key: (b"pv", None, None)}, "s": {key: (None, b"ps", None)},
            "vsa": {key: (b"pv", b"ps", b"pa")}}


# ================================================================================ device side
def run_fold(cuda, data, recs, h1=None, shift=0):
    """k2h_amd_archive_fold over the file bytes `data` (in a guarded allocation, `shift` bytes
    past a 16-byte boundary) and host records (archive.REC_DTYPE), into sentinel-filled outputs:
    (keep, by, dropped) on the host.  h1: None, or a uint64 array passed as the caller's."""
    import torch

    import big_offsets as bo
    fw, file = bo.guarded(torch, cuda, max(len(data), 1), shift=shift, fill=0xA5)
    if len(data):
        file[:len(data)] = torch.from_numpy(np.frombuffer(bytes(data), np.uint8).copy()).to(cuda)
    return run_fold_on(cuda, file, len(data), recs, h1, whole=fw)


def run_fold_on(cuda, file, size, recs, h1=None, whole=None):
    import torch

    import big_offsets as bo
    from k2hash_amd import _native, archive
    n = len(recs)
    words = np.ascontiguousarray(recs).view(np.int64).reshape(-1, archive.REC_WORDS)
    d_recs = torch.from_numpy(words.copy()).to(cuda) if n else torch.zeros((1, archive.REC_WORDS), dtype=torch.int64,
                                                                         device=cuda)
    kw, keep = bo.guarded(torch, cuda, max(n, 1), fill=0xEE)
    full, by = bo.sentinel_words(torch, cuda, n)
    d_h1 = None if h1 is None else torch.from_numpy(np.ascontiguousarray(h1, np.uint64).view(np.int64).copy()).to(cuda)
    dropped = ctypes.c_uint64(0xDEAD)
    _native.check(_native.batch_lib().k2h_amd_archive_fold(
        bo._p(file), size, bo._p(d_recs), n, None if d_h1 is None else bo._p(d_h1), bo._p(keep), bo._p(by),
        ctypes.byref(dropped), bo._stream()))
    torch.cuda.synchronize()
    assert bo.guards_intact(torch, kw, keep[:n], 0xEE) if n else bool((kw == 0xEE).all()), "bytes outside keep written"
    if whole is not None:
        assert bo.guards_intact(torch, whole, file, 0xA5), "the file's guards changed"
    return keep[:n].cpu().numpy(), bo.words_back(torch, full, n, "by"), int(dropped.value)


def assert_same(got, want, what):
    for name, g, w in zip(("keep", "by"), got[:2], want[:2]):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {name} differs at record {int(bad[0])}: got {g[bad[0]]}, want {w[bad[0]]}"
    assert got[2] == want[2], f"{what}: dropped {got[2]}, want {want[2]}"
