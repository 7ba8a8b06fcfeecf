"""Helper for tests/test_ralledata_subkeys.py, test_ralledata_subkeys_4gib.py and
test_subkeys_stream.py (not a test module, not a conftest).

* walk: the strict walk of a subkeys segment (include/k2hash_amd.h section 4b'''''').
* edges_model: what k2h_amd_ralledata_subkeys reports, as a sequential pass: a dict from identity
  -- stored hash, stored subhash, key bytes -- to the last participant, then one look-up per name
  under the name's hashes as the oracle computes them.
* Table / remove: K2HShm::Remove(key, true) with RemoveEx and RemoveSubkeys
  (lib/k2hshm.cc:2544-2560, :2735-2864, :2866-2898) transliterated over a dict keyed by (hash,
  subhash, key) that is filled by feeding the participants in order.  libk2hash itself is not
  built here.
* reach_model: what k2h_amd_ralledata_reach reports: the closure by remove, and the levels of
  the level-synchronous traversal for max_levels.
* Stream builders, and run_subkeys / run_reach: the C calls into sentinel-filled outputs.
"""
import json
import struct

import numpy as np

import ralle_check_model as rm
import ralle_dedup_model as dm
from ralle_check_model import M64, ROOT

NONE = M64
PART, HAS, BAD = 1, 2, 4
FIXTURE = ROOT / "tests" / "golden" / "ralle_subkeys.json"


# --------------------------------------------------------------------------------- the walk
def walk(seg):
    """None for a BAD segment, else the list of (pos, len) of its edges, in segment order (the
    names of non-zero length, duplicates kept).  b"" is no list: []."""
    L = len(seg)
    if L == 0:
        return []
    if L < 8:
        return None
    count = struct.unpack_from("<Q", seg, 0)[0]
    pos, out = 8, []
    while count:
        if L - pos < 8:
            return None
        ln = struct.unpack_from("<Q", seg, pos)[0]
        pos += 8
        if L - pos < ln:
            return None
        if ln:
            out.append((pos, ln))
        pos += ln
        count -= 1
    return out


def names_of(seg):
    """The names the table would follow: [] for a BAD segment."""
    w = walk(seg)
    return [] if w is None else [bytes(seg[p:p + n]) for p, n in w]


def serialize(names, count=None, trail=b""):
    """count, then (length, bytes) per name, in the order given; then `trail`."""
    out = struct.pack("<Q", (len(names) if count is None else count) & M64)
    for nm in names:
        out += struct.pack("<Q", len(nm)) + bytes(nm)
    return out + trail


def fixture():
    """The cases of tests/golden/ralle_subkeys.json with their segment as bytes in "seg"."""
    d = json.loads(FIXTURE.read_text())
    whole = {c["name"]: bytes.fromhex(c["subkeys"]) for c in d["cases"] if "subkeys" in c}
    for c in d["cases"]:
        c["seg"] = whole[c["name"]] if "subkeys" in c else whole[c["cut_of"]][:c["cut"]]
    return d


def strictly_bad_segments():
    """Segments the fixture cannot hold, because the reference would read out of bounds on them:
    L < 8, a length field cut short, and names that end up to 8 bytes behind the segment."""
    a, b = b"first-name", b"\x00second\xff"
    whole = serialize([a, b])
    out = [whole[:cut] for cut in (1, 4, 7)]
    out += [whole[:8 + 3], whole[:8 + 8 + len(a) + 5], whole[:8 + 8 + len(a)]]       # length fields cut short, or absent
    out += [whole[:len(whole) - k] for k in (1, 5, 8)]                                # the last name 1, 5, 8 bytes short
    return out


# ------------------------------------------------------------------------------- the model
def hashes_of(oracle, names, variant=0):
    """{name: (h1, h2)} by the oracle."""
    names = sorted(set(bytes(x) for x in names))
    if not names:
        return {}
    off = np.zeros(len(names) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in names])
    h1, h2 = oracle.hash_csr(np.frombuffer(b"".join(names), np.uint8), off, variant)
    return {nm: (int(a), int(b)) for nm, a, b in zip(names, h1, h2)}


def participants(buf, off, size=None, consider=None):
    """(i, identity, subkeys segment bytes, absolute offset of the segment) per participant."""
    raw = bytes(buf)
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    for i in range(len(off) - 1):
        if consider is not None and not consider[i]:
            continue
        st, f = rm.header_status(raw, off[i], off[i + 1], size)
        if st == rm.OK:
            seg = raw[off[i] + f[8]:off[i] + f[8] + f[4]] if f[4] else b""
            yield i, dm.identity(raw, off[i], f), seg, off[i] + f[8]


class Edges:
    """edges_model's answer: flags uint8 n, edge_off uint64 n + 1, child uint64 E, rep uint64 n,
    counts [5], names (the E names as bytes), where (their absolute (pos, len))."""


def edges_model(oracle, buf, off, size=None, consider=None, variant=0):
    n = len(off) - 1
    m = Edges()
    m.flags, m.rep = np.zeros(n, np.uint8), np.full(n, NONE, np.uint64)
    per = [0] * n
    m.names, m.where, m.owner = [], [], []
    last, ident_of = {}, {}
    parts = list(participants(buf, off, size, consider))
    for i, ident, seg, at in parts:
        last[ident] = i
        ident_of[i] = ident
        m.flags[i] = PART | (HAS if seg else 0)
        w = walk(seg)
        if w is None:
            m.flags[i] |= BAD
            continue
        per[i] = len(w)
        for p, ln in w:
            m.names.append(seg[p:p + ln])
            m.where.append((at + p, ln))
            m.owner.append(i)
    for i, ident in ident_of.items():
        m.rep[i] = last[ident]
    m.edge_off = np.zeros(n + 1, np.uint64)
    m.edge_off[1:] = np.cumsum(per)
    hs = hashes_of(oracle, m.names, variant)
    m.child = np.array([last.get(hs[nm] + (nm,), NONE) for nm in m.names], np.uint64).reshape(-1)
    m.counts = [len(parts), sum(1 for x in per if x), int(((m.flags & BAD) != 0).sum()), len(m.names),
                int((m.child == np.uint64(NONE)).sum())]
    m.ident_of, m.last, m.hashes = ident_of, last, hs
    return m


# ---------------------------------------------------------------- the reference's removal
class Table:
    """{(hash, subhash, key): subkeys segment bytes}, filled by feeding the participants in
    stream order: a later blob of an identity replaces the element (lib/k2hshmdirect.cc:446-473)."""

    def __init__(self, oracle, buf, off, size=None, consider=None, variant=0):
        self.elements = {}
        for _i, ident, seg, _at in participants(buf, off, size, consider):
            self.elements[ident] = seg
        self.oracle, self.variant = oracle, variant
        self._hashes = {}

    def _hash(self, key):
        if key not in self._hashes:
            self._hashes[key] = (self.oracle.k2h_hash(key, self.variant), self.oracle.k2h_second_hash(key, self.variant))
        return self._hashes[key]

    def remove(self, key, removed):
        """K2HShm::Remove(key, true): the element found by the name's hashes and bytes, its list
        by GetSubKeys(pElement, pSubKeys) (no expiry or history check; a rejected segment is no
        list), the element removed, then the same for every name of the list.  A name that is
        not found is skipped; a cycle ends because the element is already gone."""
        todo = [bytes(key)]                       # the re-entrant calls, as a stack
        while todo:
            k = todo.pop()
            ident = self._hash(k) + (k,)
            seg = self.elements.get(ident)
            if seg is None:
                continue
            del self.elements[ident]
            removed.add(ident)
            todo.extend(reversed(names_of(seg)))


def removed_by(oracle, buf, off, root_blobs, size=None, consider=None, variant=0):
    """(reach uint8 n, the table after the removes): Remove(key of blob r, true) for every root
    blob r that takes part, reach[i] = blob i is a copy of a key that was removed."""
    t = Table(oracle, buf, off, size, consider, variant)
    raw, removed = bytes(buf), set()
    ident_of = {i: ident for i, ident, _s, _a in participants(buf, off, size, consider)}
    for r in root_blobs:
        if r in ident_of:
            assert t._hash(ident_of[r][2]) == ident_of[r][:2], "a root blob's stored hashes are its key's"
            t.remove(ident_of[r][2], removed)
    reach = np.zeros(len(off) - 1, np.uint8)
    for i, ident in ident_of.items():
        reach[i] = ident in removed
    del raw
    return reach, t.elements


def reach_model(m, root_blobs, max_levels=0):
    """(reach uint8 n, [reached, levels, converged]) of the level-synchronous traversal over
    edges_model's answer m."""
    n = len(m.rep)
    seen = set()
    frontier = []
    for r in root_blobs:
        c = int(m.rep[r])
        if c != NONE and c not in seen:
            seen.add(c)
            frontier.append(c)
    levels = 0
    while frontier and (not max_levels or levels < max_levels):
        nxt = []
        for b in frontier:
            for e in range(int(m.edge_off[b]), int(m.edge_off[b + 1])):
                c = int(m.child[e])
                if c != NONE and c not in seen:
                    seen.add(c)
                    nxt.append(c)
        frontier = nxt
        levels += 1
    reach = np.array([1 if int(m.rep[i]) != NONE and int(m.rep[i]) in seen else 0 for i in range(n)], np.uint8)
    return reach, [int(reach.sum()), levels, 0 if frontier else 1]


# ------------------------------------------------------------------------- stream builders
def blobs_with_lists(oracle, keys, lists, vals=None, variant=0):
    """One bytearray per record: key, a value (every blob has one) and the subkeys segment
    lists[i] (bytes as given; b"" for none)."""
    vals = [b"v%d" % i for i in range(len(keys))] if vals is None else vals
    return rm.split(*rm.stream_of(oracle, (list(keys), list(vals), [bytes(x) for x in lists], None), variant))


# ------------------------------------------------------------------------------ device side
def run_subkeys(cuda, t, size, off, consider=None, std_fnv=False, want_rep=True, count_only=False, cap=None):
    """k2h_amd_ralledata_subkeys, count then fill, into sentinel-filled outputs: (rc, flags,
    edge_off, child, rep, counts) on the host; cap: the child entries offered (default E)."""
    import ctypes

    import torch

    import big_offsets as bo
    from k2hash_amd import _native
    n = len(off) - 1
    d_off = torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)
    fw, flags = bo.guarded(torch, cuda, n, fill=0xEE)
    fe, eoff = bo.sentinel_words(torch, cuda, n + 1)
    fr, rep = bo.sentinel_words(torch, cuda, n)
    cons = None if consider is None else torch.from_numpy(np.asarray(consider, np.uint8)).to(cuda)
    counts = (ctypes.c_uint64 * 5)(*[0xDEAD] * 5)
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    lib = _native.batch_lib()

    def call(r, c, k):
        return lib.k2h_amd_ralledata_subkeys(bo._p(t), size, bo._p(d_off), n, None if cons is None else bo._p(cons),
                                             _native.K2H_AMD_FLAG_STD_FNV if std_fnv else 0, bo._p(flags), bo._p(eoff),
                                             r, c, k, cp, bo._stream())
    rc = call(None, None, 0)
    torch.cuda.synchronize()
    assert rc == 0, rc
    E = int(counts[3])
    child = None
    if not count_only:
        k = E if cap is None else cap
        fc, ch = bo.sentinel_words(torch, cuda, max(k, 1))
        rc = call(bo._p(rep) if want_rep else None, bo._p(ch), k)
        torch.cuda.synchronize()
        child = bo.words_back(torch, fc, max(k, 1), "child")[:min(k, E)] if rc == 0 else fc.cpu().numpy().view(np.uint64)
    assert bo.guards_intact(torch, fw, flags, 0xEE), "bytes outside sk_flags written"
    return (rc, flags.cpu().numpy(), bo.words_back(torch, fe, n + 1, "edge_off"), child,
            bo.words_back(torch, fr, n, "rep") if want_rep and not count_only and rc == 0 else fr.cpu().numpy().view(np.uint64),
            [int(c) for c in counts])


def run_reach(cuda, m, roots_mask, max_levels=0):
    """k2h_amd_ralledata_reach over a model's (or a run's) edge_off, child, rep: (reach, counts)."""
    import ctypes

    import torch

    import big_offsets as bo
    from k2hash_amd import _native
    n = len(m.rep)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(cuda)  # noqa: E731
    eo, ch, rp = dev(m.edge_off), dev(np.asarray(m.child, np.uint64)), dev(m.rep)
    roots = torch.from_numpy(np.asarray(roots_mask, np.uint8)).to(cuda)
    rw, reach = bo.guarded(torch, cuda, n, fill=0xEE)
    counts = (ctypes.c_uint64 * 3)(0xDEAD, 0xDEAD, 0xDEAD)
    p = lambda t: ctypes.c_void_p(t.data_ptr() or 1)  # noqa: E731
    _native.check(_native.batch_lib().k2h_amd_ralledata_reach(
        p(eo), p(ch), p(rp), n, p(roots), max_levels, p(reach), ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64)),
        bo._stream()))
    torch.cuda.synchronize()
    assert bo.guards_intact(torch, rw, reach, 0xEE), "bytes outside reach written"
    return reach.cpu().numpy(), [int(c) for c in counts]


def assert_edges(got, m, what, want_rep=True):
    rc, flags, eoff, child, rep, counts = got
    assert rc == 0, (what, rc)
    for name, g, w in (("sk_flags", flags, m.flags), ("edge_off", eoff, m.edge_off), ("child", child, m.child)) + \
            ((("rep", rep, m.rep),) if want_rep else ()):
        assert len(g) == len(w), f"{what}: {name} has {len(g)} entries, want {len(w)}"
        bad = np.nonzero(np.asarray(g) != np.asarray(w))[0]
        assert bad.size == 0, (f"{what}: {name} differs at {int(bad[0])}: got {int(g[bad[0]]):#x}, "
                               f"want {int(w[bad[0]]):#x} ({bad.size} in all)")
    assert counts == m.counts, f"{what}: counts {counts}, want {m.counts}"
