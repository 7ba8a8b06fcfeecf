"""Helper for tests/test_ralledata_delta.py, tests/test_ralledata_delta_4gib.py and
tests/test_delta_stream.py (not a test module, not a conftest): the model of
k2h_amd_ralledata_delta (include/k2hash_amd.h section 4d').

* delta_model: the rule as one sequential pass over the slots, built on ralle_check_model's
  header judgement and archive_fold_model.scom_record, which states the record bytes (and is
  pinned to the reference's own records by tests/test_archive_fold.py).
* table_of: the table a stream stands for, in replay's terms.
* last_copies: the reduction delta_log does before the diff, in numpy.
* The state grid and the random tables of the tests.
* run_delta / assert_delta: the C call into sentinel-filled, guarded outputs, and the comparison.

Nothing here calls the code under test except run_delta, which only launches it.
"""
import ctypes
import itertools

import numpy as np

import archive_fold_model as fm
import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_diff_model as df
from ralle_unlink_model import layout

SET_ALL, REPLACE_VAL, REPLACE_SKEY, REPLACE_ATTRS, DEL_KEY = 1, 2, 4, 8, 16     # the made bits
TYPE_OF = {SET_ALL: fm.SET_ALL, REPLACE_VAL: fm.REPLACE_VAL, REPLACE_SKEY: fm.REPLACE_SKEY,
           REPLACE_ATTRS: fm.REPLACE_ATTRS, DEL_KEY: fm.DEL_KEY}
BITS = (SET_ALL, REPLACE_VAL, REPLACE_SKEY, REPLACE_ATTRS, DEL_KEY)


def _segs(raw, b, f):
    """(key, value, subkeys, attrs) of the blob at b; the pos of a length-0 segment is ignored."""
    return tuple(raw[b + f[6 + s]:b + f[6 + s] + f[2 + s]] if f[2 + s] else b"" for s in range(4))


def asks(r):
    """The records an A slot's rel bits ask for, as made bits."""
    if not r & df.PART:
        return 0
    if not r & df.FOUND:
        return SET_ALL
    return (REPLACE_VAL if r & df.VAL else 0) | (REPLACE_SKEY if r & df.SKEY else 0) | (REPLACE_ATTRS if r & df.ATTRS else 0)


def records_of(want, segs):
    """The records of a slot that yields `want`, in order."""
    key, v, s, a = segs
    out = []
    if want & SET_ALL:
        out.append(fm.scom_record(fm.SET_ALL, key, v, s, a))
    if want & REPLACE_VAL:
        out.append(fm.scom_record(fm.REPLACE_VAL, key, val=v))
    if want & REPLACE_SKEY:
        out.append(fm.scom_record(fm.REPLACE_SKEY, key, skey=s))
    if want & REPLACE_ATTRS:
        out.append(fm.scom_record(fm.REPLACE_ATTRS, key, attrs=a))
    if want & DEL_KEY:
        out.append(fm.scom_record(fm.DEL_KEY, key))
    return out


def delta_model(a, a_off, rel, b, b_off, b_consider, seen, a_size=None, b_size=None, wrong_rule=False):
    """(bytes, slot_off uint64 na + nb + 1, made uint8 na + nb, counts [8]) of the call.
    seen None: no deletions, nothing of B is looked at.  wrong_rule: the control of the tests,
    one SET_ALL per changed blob."""
    raw_a = bytes(a)
    a_off = [int(x) for x in a_off]
    na = len(a_off) - 1
    nb = 0 if b_off is None else len(b_off) - 1
    slots = []
    for i in range(na):
        want = asks(int(rel[i]))
        if wrong_rule and want:
            want = SET_ALL
        slots.append((want, raw_a, a_off[i], a_off[i + 1], len(raw_a) if a_size is None else a_size))
    if nb:
        raw_b = bytes(b) if seen is not None else b""
        b_off = [int(x) for x in b_off]
        for j in range(nb):
            want = DEL_KEY if seen is not None and not seen[j] and (b_consider is None or b_consider[j]) else 0
            slots.append((want, raw_b, b_off[j], b_off[j + 1], len(raw_b) if b_size is None else b_size))
    parts, slot_off, made = [], [0], np.zeros(na + nb, np.uint8)
    counts = [0] * 8
    for g, (want, raw, lo, hi, size) in enumerate(slots):
        recs = []
        if want:
            st, f = rm.header_status(raw, lo, hi, size)
            if st == rm.OK:
                recs = records_of(want, _segs(raw, lo, f))
                made[g] = want
                for k, bit in enumerate(BITS):
                    counts[2 + k] += bool(want & bit)
            else:
                counts[7] += 1
        parts += recs
        slot_off.append(slot_off[-1] + sum(len(r) for r in recs))
    counts[0], counts[1] = sum(counts[2:7]), slot_off[-1]
    return b"".join(parts), np.array(slot_off, np.uint64), made, counts


def table_of(stream, off, consider=None):
    """The table a stream stands for: {key: (V, S, A)}, per identity the last participant
    winning, an empty field None as archive_fold_model.replay has it.  The tests' blobs store
    their keys' own hashes, so an identity is its key; two identities with one key would be two
    elements no key -> element table can hold, and raise."""
    raw = bytes(stream)
    t = {}
    for _i, ident, segs in df._participants(raw, off, None, consider):
        t[ident] = tuple(x or None for x in segs)
    keys = [ident[2] for ident in t]
    assert len(set(keys)) == len(keys), "two identities share a key"
    return {ident[2]: v for ident, v in t.items()}


def last_copies(stream, off, consider=None):
    """The mask delta_log reduces a stream to: 1 for the last considered participant of every
    identity and for every considered blob that is no participant, 0 for earlier copies and for
    the blobs consider leaves out."""
    n = len(off) - 1
    keep = np.ones(n, np.uint8) if consider is None else (np.asarray(consider) != 0).astype(np.uint8)
    last = {}
    for i, ident, _s in df._participants(bytes(stream), off, None, consider):
        if ident in last:
            keep[last[ident]] = 0
        last[ident] = i
    return keep


def log_recs(log):
    """The Rec list of a log's bytes, by the host scan."""
    from k2hash_amd import archive
    return fm.recs_of(log, archive.scan(log))


# --------------------------------------------------------------------------------- the inputs
def own_key(idx):
    """A key of its own per cell, lengths 1..100."""
    ln, k = 1 + idx % 100, idx // 100
    return (bytes([0x41 + k]) + bytes((7 * j + 3 * idx + 1) & 0xFF for j in range(ln)))[:ln]


PAIRS = ("00", "0x", "x0", "xx", "xy", "xz")   # (held, new) of one field: empty, x; x -> another of its length, of another length


def _field(state, name, idx):
    x = b"%s-%03d" % (name, idx)
    y = bytes(reversed(x))
    z = x + b"+longer" if idx % 2 else x[:3]
    return {"00": (b"", b""), "0x": (b"", x), "x0": (x, b""), "xx": (x, x), "xy": (x, y), "xz": (x, z)}[state]


def grid(hashes_of):
    """The 232 cells: (cells, held elements, new elements).  cells[c] = (key, kind, records the
    delta owes it); the elements are {key: (V, S, A)} with b"" for an empty field, in cell order.
    hashes_of: keys -> {key: (h1, h2)}."""
    cells, held, new = [], {}, {}
    idx = 0
    for states in itertools.product(PAIRS, repeat=3):
        key = own_key(idx)
        h, n = zip(*(_field(st, nm, idx) for st, nm in zip(states, (b"val", b"sub", b"att"))))
        held[key], new[key] = h, n
        cells.append((key, "both", sum(a != b for a, b in zip(h, n))))
        idx += 1
    for side, name in ((held, "held-only"), (new, "new-only")):
        for mask in range(8):
            key = own_key(idx)
            side[key] = tuple(b"%s-%03d" % (nm, idx) if mask >> k & 1 else b"" for k, nm in enumerate((b"val", b"sub", b"att")))
            cells.append((key, name, 1))
            idx += 1
    assert len(cells) == 232 and len({c[0] for c in cells}) == 232
    assert sorted({len(c[0]) for c in cells}) == list(range(1, 101))
    hs = hashes_of([c[0] for c in cells])
    return cells, held, new, hs


def stream_from(elements, hs, order=None):
    """(bytes, offsets) of {key: (V, S, A)} as GetElementToBinary's blobs, in dict (or `order`) order."""
    keys = list(elements) if order is None else order
    return rm.join([layout(hs[k], k, *elements[k]) for k in keys])


def as_table(elements):
    return {k: tuple(x or None for x in v) for k, v in elements.items()}


def random_pair(seed, hs_of):
    """Two streams with duplicates and non-participants and a consider mask each:
    ((a, a_off, a_consider), (b, b_off, b_consider))."""
    rng = np.random.default_rng([9100, seed])
    keys = [b"rk-%d-" % k + b"k" * (k % 7) for k in range(12)]
    hs = hs_of(keys)

    def field(name):
        u = rng.random()
        return b"" if u < 0.35 else b"%s%d" % (name, rng.integers(0, 3)) * int(rng.integers(1, 4))

    def stream():
        blobs = []
        for _ in range(int(rng.integers(0, 25))):
            k = keys[int(rng.integers(0, 12))]
            blob = bytearray(layout(hs[k], k, field(b"v"), field(b"s"), field(b"a")))
            u = rng.random()
            if u < 0.05:
                rm.put(blob, 0, rm.F_KLEN, 0)                 # NO_KEY, or EMPTY
            elif u < 0.08:
                rm.put(blob, 0, rm.F_KPOS, len(blob))         # BAD_RANGE
            elif u < 0.10:
                blob = blob[:70]                              # a short span
            blobs.append(blob)
        buf, off = rm.join(blobs, lead=b"\x99" * int(rng.integers(0, 5)))
        cons = (rng.random(len(blobs)) < 0.85).astype(np.uint8) if rng.random() < 0.5 else None
        return buf, off, cons
    return stream(), stream()


# ------------------------------------------------------------------------------ device side
def run_delta(cuda, a, a_off, rel, b, b_off, b_consider, seen, cap=None, count_only=False, want_made=True, ashift=5,
              bshift=11, oshift=3, a_size=None, b_size=None, pass_b=True):
    """k2h_amd_ralledata_delta: a count-only call, then (unless count_only) the fill into an out
    of exactly `cap` bytes (default: the counted bytes) that lies `oshift` bytes off alignment
    between guards.  a / b: bytes (placed at odd shifts between canaries) or device tensors.
    pass_b=False: NULL for B's blobs and offsets.  Returns (rc, out bytes, slot_off, made,
    counts); made None when NULL was passed."""
    import torch

    import big_offsets as bo
    from archive_apply_model import to_dev
    from k2hash_amd import _native
    na = len(a_off) - 1
    nb = 0 if b_off is None else len(b_off) - 1
    N = na + nb
    aw = bw = None
    if not torch.is_tensor(a):
        a_size = len(a) if a_size is None else a_size
        aw, a = to_dev(cuda, a, ashift)
    if b is None:
        b, b_size = a[:0], 0
    elif not torch.is_tensor(b):
        b_size = len(b) if b_size is None else b_size
        bw, b = to_dev(cuda, b, bshift)
    i64 = lambda o: None if o is None else torch.tensor([int(x) for x in o], dtype=torch.int64, device=cuda)  # noqa: E731
    u8 = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.uint8).copy()).to(cuda)  # noqa: E731
    d_aoff, d_boff, d_rel, d_cons, d_seen = i64(a_off), i64(b_off), u8(rel), u8(b_consider), u8(seen)
    mw, made = bo.guarded(torch, cuda, max(N, 1), fill=0xEE)
    counts = (ctypes.c_uint64 * 8)(*[0xDEAD] * 8)
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    lib = _native.batch_lib()
    p = lambda x, k=1: None if x is None or not k else ctypes.c_void_p(x.data_ptr() or 1)  # noqa: E731

    def call(o, k, so):
        return lib.k2h_amd_ralledata_delta(p(a, na), a_size, p(d_aoff, na), na, p(d_rel, na), p(b, nb and pass_b), b_size,
                                           p(d_boff, nb and pass_b), nb, p(d_cons, nb), p(d_seen, nb), o, k, so,
                                           p(made) if want_made else None, cp, bo._stream())

    def guards():
        if N:
            assert bo.guards_intact(torch, mw, made[:N], 0xEE), "bytes outside made written"
        else:
            assert bool((mw == 0xEE).all()), "made written although there is no slot"
        if aw is not None:
            assert bo.guards_intact(torch, aw, a, 0xA5), "stream A's guards changed"
        if bw is not None:
            assert bo.guards_intact(torch, bw, b, 0xA5), "stream B's guards changed"
    rc = call(None, 0, None)
    torch.cuda.synchronize()
    guards()
    first = [int(c) for c in counts]
    md = made[:N].cpu().numpy()
    if not want_made:
        assert (md == 0xEE).all(), "made written although NULL was passed"
    if count_only or rc != 0:
        return rc, None, None, md if want_made else None, first
    k = first[1] if cap is None else cap
    ow, out = bo.guarded(torch, cuda, k, shift=oshift)
    fo, soff = bo.sentinel_words(torch, cuda, N + 1)
    rc = call(p(out), k, p(soff))
    torch.cuda.synchronize()
    guards()
    assert bo.guards_intact(torch, ow, out), "bytes outside out written"
    got = [int(c) for c in counts]
    assert got == first, f"the fill counts {got}, the count-only call {first}"
    assert np.array_equal(md, made[:N].cpu().numpy()), "made differs between the count-only call and the fill"
    so = bo.words_back(torch, fo, N + 1, "slot_off")
    if rc != 0:
        assert bool((out == bo.OUT_FILL).all()), "out written although the call failed"
    return rc, out.cpu().numpy().tobytes(), so, md if want_made else None, got


def assert_delta(got, want, what):
    rc, out, so, made, counts = got
    w_out, w_so, w_made, w_counts = want
    assert rc == 0, (what, rc)
    assert counts == w_counts, f"{what}: counts {counts}, want {w_counts}"
    for name, g, w in (("slot_off", so, w_so), ("made", made, w_made)):
        if g is None:
            continue
        assert len(g) == len(w), f"{what}: {name} has {len(g)} entries, want {len(w)}"
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert bad.size == 0, f"{what}: {name} differs at {int(bad[0])}: got {int(g[bad[0]])}, want {int(w[bad[0]])}"
    if out is not None and out != w_out:
        x, y = np.frombuffer(out, np.uint8), np.frombuffer(w_out, np.uint8)
        at = int(np.nonzero(x != y)[0][0]) if len(x) == len(y) else min(len(x), len(y))
        slot = int(np.searchsorted(w_so, at, side="right")) - 1
        raise AssertionError(f"{what}: out differs at byte {at} (slot {slot}, made {int(w_made[slot])}, "
                             f"{at - int(w_so[slot])} bytes into its records)")


def against_model(cuda, a, b, what, a_consider=None, b_consider=None, rel=None, seen="model", **kw):
    """a, b: (buf, off) (b None: no held stream).  rel and seen from ralle_diff_model (or as
    given; seen None: no deletions), the call against delta_model.  Returns (got, model)."""
    (a_buf, a_off), (b_buf, b_off) = a, b if b is not None else (b"", [0])
    d = df.diff_model(a_buf, a_off, b_buf, b_off, a_consider, b_consider)
    rel = d[0] if rel is None else rel
    seen = d[2] if isinstance(seen, str) else seen
    if b is None:
        b_buf, b_off = None, None
    m = delta_model(a_buf, a_off, rel, b_buf, b_off, b_consider, seen)
    got = run_delta(cuda, a_buf, a_off, rel, b_buf, b_off, b_consider, seen, **kw)
    if got[1] is not None or kw.get("count_only"):
        assert_delta(got, m, what)
    return got, m
