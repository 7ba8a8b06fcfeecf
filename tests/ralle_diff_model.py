"""Helper for tests/test_ralledata_diff.py, tests/test_ralledata_diff_held.py and
tests/test_ralledata_diff_4gib.py (not a test module, not a conftest).

* diff_model: what k2h_amd_ralledata_diff reports (include/k2hash_amd.h section 4b'''''), as a
  sequential pass: a dict from identity -- stored hash, stored subhash, key bytes -- to the last
  participant of B, then one look-up per participant of A.  APPLY is lib/k2hshmdirect.cc:380-431
  restated over the matched blob's attrs with ralle_times_model's get_time and is_expire.
* feed_of / feed_blobs: the mask the header defines from rel, and the replay's two policies.
* The compare kernel's threshold and the resolve kernel's block width, read from the source.
* run_diff: the C call into sentinel-filled outputs.
* assert_diff / explain: the comparison, and what a failure says about a differing blob of A: its
  attrs kind, the held blobs of its stored hash, and both answers' bits by name.
"""
import re

import numpy as np

import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_times_model as tm
from ralle_check_model import M64, ROOT

_SRC = (ROOT / "k2hash_amd" / "csrc" / "k2h_ralledata_diff.hip").read_text()


def _const(name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", _SRC)
    assert m, name
    return int(m.group(1))


WAVE_BYTES = _const("kDiffWaveBytes")        # a pair with more bytes to compare goes to its whole wave
RESOLVE_BLOCK = _const("kDiffResolveBlock")  # sorted positions per block of the resolve kernel
WAVE_STEP = 64 * 16                          # bytes of each side a wave compares per step
NONE = M64
PART, FOUND, VAL, SKEY, ATTRS, DATA, REPEAT, APPLY = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80


def _segments(raw, b, f):
    """(value, subkeys, attrs) of the blob at b: bytes, b"" for a length-0 segment."""
    return tuple(raw[b + f[7 + s]:b + f[7 + s] + f[3 + s]] if f[3 + s] else b"" for s in range(3))


def _participants(buf, off, size, consider):
    raw = bytes(buf)
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    for i in range(len(off) - 1):
        if consider is not None and not consider[i]:
            continue
        st, f = rm.header_status(raw, off[i], off[i + 1], size)
        if st == rm.OK:
            yield i, dm.identity(raw, off[i], f), _segments(raw, off[i], f)


def would_apply(a_attrs, b_attrs, pts, now):
    """lib/k2hshmdirect.cc:380-431 with b_attrs the existing element's: True when the call goes
    on to write."""
    if not b_attrs:                                   # no attrs page: GetAttrs NULL
        return True
    if tm.is_expire(b_attrs, now):                    # :390
        return True
    mb = tm.get_time(b_attrs, tm.MTIME)
    if mb is None:                                    # :395
        return True
    if not tm._less(mb, pts):                         # :402, pts <= m_b
        return False
    mi = tm.get_time(a_attrs, tm.MTIME) if a_attrs else None
    return mi is not None and tm._less(mb, mi)        # :416, :426


def diff_model(a_buf, a_off, b_buf, b_off, a_consider=None, b_consider=None, times=None, a_size=None, b_size=None):
    """(rel uint8 na, match uint64 na, seen uint8 nb, counts [4]); times: (pts, now) or None."""
    na, nb = len(a_off) - 1, len(b_off) - 1
    held = {}
    for j, ident, segs in _participants(b_buf, b_off, b_size, b_consider):
        held[ident] = (j, segs)                       # the last one stays
    rel, match, seen = np.zeros(na, np.uint8), np.full(na, NONE, np.uint64), np.zeros(nb, np.uint8)
    parts = list(_participants(a_buf, a_off, a_size, a_consider))
    hashes = {}
    for _i, ident, _s in parts:
        hashes[ident[0]] = hashes.get(ident[0], 0) + 1
    counts = [0, 0, 0, 0]
    for i, ident, segs in parts:
        r = PART | (DATA if any(segs) else 0) | (REPEAT if hashes[ident[0]] > 1 else 0)
        apply = True
        if ident in held:
            j, hsegs = held[ident]
            match[i], seen[j] = j, 1
            r |= FOUND
            for s, bit in enumerate((VAL, SKEY, ATTRS)):
                if segs[s] != hsegs[s]:
                    r |= bit
            if times is not None:
                apply = would_apply(segs[2], hsegs[2], *times)
        if times is not None and apply:
            r |= APPLY
        rel[i] = r
        counts[0] += 1
        counts[1] += bool(r & FOUND)
        counts[2] += bool(r & FOUND) and not r & (VAL | SKEY | ATTRS)
        counts[3] += bool(r & APPLY)
    return rel, match, seen, counts


def feed_of(rel, repeat_always=True):
    """The header's feed mask; repeat_always=False is the control policy that applies the
    per-blob verdict to REPEAT blobs as well."""
    rel = np.asarray(rel, np.uint8)
    change = np.where(rel & FOUND, (rel & (VAL | SKEY | ATTRS)) != 0, (rel & DATA) != 0)
    verdict = ((rel & APPLY) != 0) & change
    rep = (rel & REPEAT) != 0 if repeat_always else False
    return ((rel & PART) != 0) & (rep | verdict)


def table_blobs(oracle, table):
    """A dump of `table` ({(hash, subhash, key): (value, subkeys, attrs)}) as blobs: B."""
    if not table:
        return []
    idents = list(table)
    blobs = dm.blobs_of(oracle, [k for _h, _s, k in idents], [table[t][0] or b"" for t in idents],
                        [table[t][1] or b"" for t in idents], [table[t][2] or b"" for t in idents])
    for b, (h, s, _k) in zip(blobs, idents):
        dm.set_hash(b, h, s)
    return blobs


# ------------------------------------------------------------------------------ device side
def run_diff(cuda, ta, a_size, a_off, tb, b_size, b_off, a_consider=None, b_consider=None, times=None,
             want=(True, True, True)):
    """k2h_amd_ralledata_diff into sentinel-filled outputs: (rel, match, seen, counts) on the
    host, shaped as diff_model's.  want: match, seen, counts (False: NULL is passed)."""
    import ctypes

    import torch

    import big_offsets as bo
    from k2hash_amd import _native
    na, nb = len(a_off) - 1, len(b_off) - 1
    off = lambda o: torch.tensor([int(x) for x in o], dtype=torch.int64, device=cuda)  # noqa: E731
    da, db = off(a_off), off(b_off)
    rw, rel = bo.guarded(torch, cuda, na, fill=0xEE)
    sw, seen = bo.guarded(torch, cuda, nb, fill=0xEE)
    full, match = bo.sentinel_words(torch, cuda, na)
    dev = lambda c: None if c is None else torch.from_numpy(np.asarray(c, np.uint8)).to(cuda)  # noqa: E731
    ca, cb = dev(a_consider), dev(b_consider)
    counts = (ctypes.c_uint64 * 4)(0xDEAD, 0xDEAD, 0xDEAD, 0xDEAD)
    ts = None
    if times is not None:
        ts = _native.DiffTimes(_native.Timespec(*times[0]), _native.Timespec(*times[1]))
    ptr = lambda t: None if t is None else bo._p(t)  # noqa: E731
    _native.check(_native.batch_lib().k2h_amd_ralledata_diff(
        bo._p(ta), a_size, bo._p(da), na, ptr(ca), bo._p(tb) if nb else None, b_size, bo._p(db) if nb else None, nb,
        ptr(cb), None if ts is None else ctypes.byref(ts), bo._p(rel), bo._p(match) if want[0] else None,
        bo._p(seen) if want[1] and nb else None, ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64)) if want[2] else None,
        bo._stream()))
    torch.cuda.synchronize()
    assert bo.guards_intact(torch, rw, rel, 0xEE) and bo.guards_intact(torch, sw, seen, 0xEE), "bytes outside written"
    return (rel.cpu().numpy(), bo.words_back(torch, full, na, "match") if want[0] else None,
            seen.cpu().numpy() if want[1] and nb else None, [int(c) for c in counts] if want[2] else None)


BIT_NAMES = ((PART, "PART"), (FOUND, "FOUND"), (VAL, "VAL"), (SKEY, "SKEY"), (ATTRS, "ATTRS"), (DATA, "DATA"),
             (REPEAT, "REPEAT"), (APPLY, "APPLY"))


def bits_by_name(r):
    return "|".join(name for bit, name in BIT_NAMES if int(r) & bit) or "0"


def _kind_names():
    names = {bytes(v): k for k, v in tm.ATTRS_KINDS.items()}
    for k, table in tm.prior_states(None).items():
        for _v, _s, attrs in table.values():
            names.setdefault(bytes(attrs or b""), k)
    return names


def attrs_kind(attrs):
    """The name of the attrs bytes among tm.ATTRS_KINDS and the tm.prior_states attrs, else "other"."""
    return _kind_names().get(bytes(attrs), "other")


def explain(i, a, b, a_consider=None, b_consider=None, got=None, want=None):
    """Blob i of A for a failure message: its attrs kind and key length, every participant of B
    that shares its stored hash, in order, with what of the identity it shares and its attrs
    kind, and the model's and the device's rel and match (got, want: (rel, match, ...), match may
    be None)."""
    (a_buf, a_off), (b_buf, b_off) = a, b
    mine = [(ident, segs) for k, ident, segs in _participants(a_buf, a_off, None, a_consider) if k == i]
    if not mine:
        line = f"A[{i}]: takes no part"
    else:
        ident, segs = mine[0]
        held = [f"B[{j}] sub {'=' if d[1] == ident[1] else '!'} key {'=' if d[2] == ident[2] else '!'} "
                f"{attrs_kind(s[2])}" for j, d, s in _participants(b_buf, b_off, None, b_consider) if d[0] == ident[0]]
        line = (f"A[{i}] {attrs_kind(segs[2])}, key of {len(ident[2])} bytes, hash {ident[0]:#x} held by: "
                + ("; ".join(held) or "none"))
    for name, res in (("model", want), ("device", got)):
        if res is not None:
            m = "-" if res[1] is None else "none" if int(res[1][i]) == NONE else int(res[1][i])
            line += f"\n    {name}: {bits_by_name(res[0][i])}, match {m}"
    return line


def assert_diff(got, want, what, streams=None, consider=(None, None), shown=4):
    """streams: (a, b), each (buf, off); with them a failure describes the first `shown`
    differing blobs of A through explain()."""
    for name, g, w in zip(("rel", "match", "seen"), got[:3], want[:3]):
        if g is None:
            continue
        bad = np.nonzero(g != w)[0]
        if bad.size == 0:
            continue
        told = ""
        if streams is not None:
            if name == "seen":   # the blobs of A that the model or the device matched to these blobs of B
                hit = set(int(j) for j in bad[:shown])
                pick = [i for i in range(len(want[0])) if int(want[1][i]) in hit
                        or (got[1] is not None and int(got[1][i]) in hit)][:shown]
            else:
                pick = [int(i) for i in bad[:shown]]
            told = "".join("\n  " + explain(i, *streams, *consider, got=got, want=want) for i in pick)
        assert False, (f"{what}: {name} differs at {int(bad[0])}: got {int(g[bad[0]]):#x}, "
                       f"want {int(w[bad[0]]):#x} ({bad.size} in all){told}")
    if got[3] is not None:
        assert got[3] == want[3], f"{what}: counts {got[3]}, want {want[3]}"


def against_model(cuda, a, b, what, shifts=(3, 11), a_consider=None, b_consider=None, times=None, tail_pad=tm.PAD,
                  want=(True, True, True)):
    """a, b: (buf, off).  The device call on the two streams placed at the two shifts, against
    the model; returns the model's answer."""
    (a_buf, a_off), (b_buf, b_off) = a, b
    model = diff_model(a_buf, a_off, b_buf, b_off, a_consider, b_consider, times)
    ta = tm.place(cuda, a_buf, shifts[0], tail_pad=tail_pad)
    tb = tm.place(cuda, b_buf, shifts[1], canary=0x5A, tail_pad=tail_pad)
    got = run_diff(cuda, ta, len(a_buf), a_off, tb, len(b_buf), b_off, a_consider, b_consider, times, want)
    assert_diff(got, model, what, (a, b), (a_consider, b_consider))
    return model
