"""Helper for tests/test_ralledata_unlink*.py and test_unlink_stream.py (not a test module, not a
conftest).

* rewritten_list / unlink_model: what k2h_amd_ralledata_unlink writes, as a sequential pass over
  the stream's bytes (include/k2hash_amd.h section 4b''''''').
* UnlinkTable: K2HShm::Remove(key, subkey) with RemoveEx(pElement, bySubKey, ...)
  (lib/k2hshm.cc:2567-2667) transliterated on top of the Table of ralle_subkeys_model.py, whose
  remove is the second half (RemoveEx(bySubKey, ..., true, ...) and RemoveSubkeys).  The table is
  filled by SetElementByBinArray's rule (ralle_dedup_model.set_element_by_bin_array) and keeps
  value and attrs beside the subkeys segment.  libk2hash itself is not built here.
* fixture: tests/golden/ralle_unlink.json, written by the reference's own K2HSubKeys.
* run_unlink: the C call into sentinel-filled, guarded outputs.
"""
import json
import struct

import numpy as np

import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_subkeys_model as sm
from ralle_check_model import HEADER, ROOT

REWRITTEN, EMPTIED, KEY_ONLY = 1, 2, 4
FIXTURE = ROOT / "tests" / "golden" / "ralle_unlink.json"


def fixture():
    """(lists {label: bytes}, cases with "erase" as a list of bytes and "out" as bytes)."""
    d = json.loads(FIXTURE.read_text())
    lists = {k: bytes.fromhex(v) for k, v in d["lists"].items()}
    for c in d["cases"]:
        c["erase"] = [bytes.fromhex(x) for x in c["erase"]]
        c["out"] = bytes.fromhex(c["out"])
    assert d["count"] == len(d["cases"])
    return lists, d["cases"]


# ------------------------------------------------------------------------------- the model
def rewritten_list(seg, dropped):
    """The new segment of an accepted list: the entries of non-zero length whose edge index is
    not in `dropped`, in segment order, under a count of their own; b"" when none is left.
    Returns (bytes, entries dropped)."""
    w = sm.walk(seg)
    assert w is not None
    names = [bytes(seg[p:p + ln]) for k, (p, ln) in enumerate(w) if k not in dropped]
    return (sm.serialize(names) if names else b""), len(w) - len(names)


def layout(f, key, val, seg, attrs):
    """GetElementToBinary's blob (lib/k2hshmdirect.cc:59-89): positions are 80 and the running
    sums, written for zero-length segments too."""
    kp = HEADER
    vp = kp + len(key)
    sp = vp + len(val)
    ap = sp + len(seg)
    return struct.pack("<10Q", f[0], f[1], len(key), len(val), len(seg), len(attrs), kp, vp, sp, ap) + key + val + seg + attrs


class Unlink:
    """unlink_model's answer: out (bytes), out_off uint64 emitted + 1, index uint64 emitted,
    changed uint8 n, counts [7]."""


def unlink_model(buf, off, flags, edge_off, drop, keep=None, size=None):
    raw = bytes(buf)
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    n = len(off) - 1
    eo = [int(x) for x in edge_off]
    m = Unlink()
    m.changed = np.zeros(n, np.uint8)
    parts, ooff, index = [], [0], []
    rewritten = dropped = emptied = key_only = mismatch = 0
    for i in range(n):
        b, e = off[i], off[i + 1]
        if (keep is not None and not keep[i]) or not b <= e <= size:
            continue
        blob = raw[b:e]
        if drop is not None and int(flags[i]) & sm.PART and not int(flags[i]) & sm.BAD:
            e0, e1 = eo[i], eo[i + 1]
            ok = e0 <= e1 <= eo[n]
            if ok:
                st, f = rm.header_status(raw, b, e, size)
                ok = st == rm.OK
            if ok:
                seg = raw[b + f[8]:b + f[8] + f[4]] if f[4] else b""
                w = sm.walk(seg)
                ok = w is not None and len(w) == e1 - e0
            if not ok:
                mismatch += 1
            elif any(drop[e0:e1]):
                new, d = rewritten_list(seg, {k for k in range(e1 - e0) if drop[e0 + k]})
                key, val, attrs = (raw[b + f[6 + s]:b + f[6 + s] + f[2 + s]] if f[2 + s] else b"" for s in (0, 1, 3))
                blob = layout(f, key, val, new, attrs)
                ch = REWRITTEN | (0 if new else EMPTIED) | (0 if new or val or attrs else KEY_ONLY)
                m.changed[i] = ch
                rewritten += 1
                dropped += d
                emptied += not new
                key_only += bool(ch & KEY_ONLY)
        parts.append(blob)
        ooff.append(ooff[-1] + len(blob))
        index.append(i)
    m.out = b"".join(parts)
    m.out_off, m.index = np.array(ooff, np.uint64), np.array(index, np.uint64)
    m.counts = [len(index), len(m.out), rewritten, dropped, int(emptied), key_only, mismatch]
    return m


# ---------------------------------------------------------------- the reference's removal
def subkeys_object(seg):
    """What K2HPage::GetSubKeys makes of a subkeys page: None without one or for a rejected
    segment, else the names as K2HSubKeys holds them -- sorted by memcmp then length, without
    duplicates (insert, SUBKEY::compare)."""
    if not seg:
        return None
    w = sm.walk(seg)
    if w is None:
        return None
    return sorted(set(bytes(seg[p:p + ln]) for p, ln in w))


class UnlinkTable(sm.Table):
    """elements: {(hash, subhash, key): subkeys segment bytes} as in Table; rest: the same keys to
    (value, attrs), each bytes or None.  Fed by SetElementByBinArray's rule: a blob with a key and
    nothing else leaves no element (lib/k2hshmdirect.cc:438)."""

    def __init__(self, oracle, buf, off, size=None, consider=None, variant=0):
        full = {}
        raw = bytes(buf)
        for i, _ident, _seg, _at in sm.participants(buf, off, size, consider):
            dm.set_element_by_bin_array(full, raw[int(off[i]):int(off[i + 1])], (0, 0))
        self.elements = {k: (v[1] or b"") for k, v in full.items()}
        self.rest = {k: (v[0], v[2]) for k, v in full.items()}
        self.oracle, self.variant = oracle, variant
        self._hashes = {}

    def remove_subkey(self, key, name, removed):
        """K2HShm::Remove(key, subkey): :2581-2597 the element by the key's hashes and bytes
        (not found: done); RemoveEx :2618 its list (no page, or a rejected one: done); :2626
        erase (the name is not in it: done); :2635-2643 the list serialized again and the page
        replaced; :2657-2663 the child removed with everything below it."""
        key, name = bytes(key), bytes(name)
        ident = self._hash(key) + (key,)
        if ident not in self.elements:
            return
        names = subkeys_object(self.elements[ident])
        if names is None or name not in names:
            return
        names.remove(name)
        self.elements[ident] = sm.serialize(names) if names else b""
        self.remove(name, removed)

    def full(self):
        """{identity: (value, subkeys, attrs)} with None for an absent page, as
        ralle_dedup_model.replay gives it."""
        return {k: (self.rest[k][0], self.elements[k] or None, self.rest[k][1]) for k in self.elements}


def fed(buf, off):
    """The table a stream leaves: every blob through SetElementByBinArray, in order."""
    raw = bytes(buf)
    return dm.replay([raw[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)], {}, (0, 0))


# ------------------------------------------------------------------------------ device side
def run_unlink(cuda, t, size, off, flags, edge_off, drop, keep=None, cap=None, count_only=False, want_changed=True,
               want_index=True, shift=3):
    """k2h_amd_ralledata_unlink: a count-only call, then (unless count_only) the fill into an out
    of exactly `cap` bytes (default: the counted bytes) that lies `shift` bytes off alignment
    between guards.  Returns (rc, out bytes, out_off, index, changed, counts), index and changed
    None when NULL was passed for them; inputs are host arrays except t, the stream's tensor.
    drop None passes NULL."""
    import ctypes

    import torch

    import big_offsets as bo
    from k2hash_amd import _native
    n = len(off) - 1
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt, copy=False)).to(cuda)  # noqa: E731
    d_off = torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)
    d_fl = dev(np.asarray(flags, np.uint8), np.uint8)
    d_eo = dev(np.asarray(edge_off, np.uint64).view(np.int64), np.int64)
    d_drop = None if drop is None else dev(np.asarray(drop, np.uint8), np.uint8)
    d_keep = None if keep is None else dev(np.asarray(keep, np.uint8), np.uint8)
    cw, changed = bo.guarded(torch, cuda, n, fill=0xEE)
    counts = (ctypes.c_uint64 * 7)(*[0xDEAD] * 7)
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    lib = _native.batch_lib()
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr() or 1)  # noqa: E731

    def call(o, k, oo, ix):
        return lib.k2h_amd_ralledata_unlink(p(t), size, p(d_off), n, p(d_keep), p(d_fl), p(d_eo), p(d_drop), o, k, oo, ix,
                                            p(changed) if want_changed else None, cp, bo._stream())
    rc = call(None, 0, None, None)
    torch.cuda.synchronize()
    assert bo.guards_intact(torch, cw, changed, 0xEE), "bytes outside changed written"
    first = [int(c) for c in counts]
    ch = changed.cpu().numpy()
    if count_only or rc != 0:
        return rc, None, None, None, ch, first
    k = first[1] if cap is None else cap
    ow, out = bo.guarded(torch, cuda, k, shift=shift)
    fo, ooff = bo.sentinel_words(torch, cuda, n + 1)
    fi, index = bo.sentinel_words(torch, cuda, max(n, 1))
    rc = call(p(out), k, p(ooff), p(index) if want_index else None)
    torch.cuda.synchronize()
    assert bo.guards_intact(torch, ow, out), "bytes outside out written"
    assert bo.guards_intact(torch, cw, changed, 0xEE), "bytes outside changed written"
    got = [int(c) for c in counts]
    if rc != 0:
        assert bool((out == bo.OUT_FILL).all()), "out written although the call failed"
        return rc, out.cpu().numpy().tobytes(), fo.cpu().numpy().view(np.uint64), None, changed.cpu().numpy(), got
    assert got == first, f"the fill counts {got}, the count-only call {first}"
    assert np.array_equal(changed.cpu().numpy(), ch), "changed differs between the count-only call and the fill"
    e = got[0]
    a = fo.cpu().numpy().view(np.uint64)
    assert (a[e + 1:] == np.uint64(bo.SENTINEL)).all(), "out_off written past entry emitted"
    b = fi.cpu().numpy().view(np.uint64)
    assert (b[e if want_index else 0:] == np.uint64(bo.SENTINEL)).all(), "index written past entry emitted - 1"
    if not want_changed:
        assert (ch == 0xEE).all(), "changed written although NULL was passed"
    return rc, out.cpu().numpy().tobytes(), a[:e + 1], b[:e] if want_index else None, ch if want_changed else None, got


def assert_unlinked(got, m, what):
    rc, out, ooff, index, changed, counts = got
    assert rc == 0, (what, rc)
    assert counts == m.counts, f"{what}: counts {counts}, want {m.counts}"
    for name, g, w in (("out_off", ooff, m.out_off), ("index", index, m.index), ("changed", changed, m.changed)):
        if g is None:
            continue
        assert len(g) == len(w), f"{what}: {name} has {len(g)} entries, want {len(w)}"
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert bad.size == 0, f"{what}: {name} differs at {int(bad[0])}: got {int(g[bad[0]])}, want {int(w[bad[0]])}"
    if out != m.out:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(m.out, np.uint8)
        at = int(np.nonzero(a != b)[0][0]) if len(a) == len(b) else min(len(a), len(b))
        blob = int(np.searchsorted(m.out_off, at, side="right")) - 1
        raise AssertionError(f"{what}: out differs at byte {at} (output blob {blob}, input blob {int(m.index[blob])}, "
                             f"{at - int(m.out_off[blob])} bytes into it)")
