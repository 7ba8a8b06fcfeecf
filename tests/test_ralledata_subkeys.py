"""k2h_amd_ralledata_subkeys and k2h_amd_ralledata_reach (include/k2hash_amd.h section
4b''''''), and k2hash_amd/subkeys.py on top of them.

The parse is pinned to the reference's own K2HSubKeys by tests/golden/ralle_subkeys.json
(gen_ralle_subkeys.cc); the edges, the representatives and the closure are compared with
ralle_subkeys_model.py, whose removal is a transliteration of K2HShm::Remove(key, true).
Expected values come only from that model and the oracle hash, never from a device call.
"""
import ctypes
import inspect

import numpy as np
import pytest

import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_subkeys_model as sm
import ralle_times_model as tm
from ralle_subkeys_model import BAD, HAS, NONE, PART

from k2hash_amd import _native, subkeys


def sort_bits_for(n):
    """k2h_ralle_ident.h, restated."""
    bits = (n - 1).bit_length() if n > 1 else 0
    bits = (bits + 8 + 7) // 8 * 8
    return min(max(bits, 16), 64)


# ===================================================================================== CPU
@pytest.fixture(scope="module")
def golden():
    return sm.fixture()


def test_model_walk_on_reference_fixture(golden):
    """The strict walk gives the reference's verdict and name set on every case the reference
    could be handed (it sorts and dedups, so the names compare as a set)."""
    assert golden["judged"] == len(golden["cases"]) >= 300 and golden["skipped"] > 0
    accepted = 0
    for c in golden["cases"]:
        w = sm.walk(c["seg"])
        assert len(c["seg"]) >= 8
        assert (w is not None) == c["accepted"], c["name"]
        if c["accepted"]:
            accepted += 1
            assert set(sm.names_of(c["seg"])) == {bytes.fromhex(x) for x in c["names"]}, c["name"]
        else:
            assert c["names"] == []
    names = {c["name"] for c in golden["cases"]}
    for must in ("written-1", "written-2", "written-3", "written-70", "count-larger", "count-smaller", "count-zero",
                 "count-zero-trailing", "zero-length-between", "duplicate-name", "count-huge"):
        assert must in names, must
    assert accepted >= 10 and sum(1 for n in names if "-cut-" in n) >= 300
    by = {c["name"]: c for c in golden["cases"]}
    assert len(by["written-70"]["names"]) == 70 and len(by["zero-length-between"]["names"]) == 2
    assert len(by["duplicate-name"]["names"]) == 2 and len(sm.names_of(by["duplicate-name"]["seg"])) == 3
    assert all(sm.walk(s) is None for s in sm.strictly_bad_segments())


def test_public_names_and_header_constants():
    import k2hash_amd
    for name in ("subkey_edges", "reach_subkeys", "subtree_ralledata", "SubkeyEdges", "Reach"):
        assert hasattr(k2hash_amd, name) and name in k2hash_amd.__all__, name
    assert (subkeys.SKEY_PART, subkeys.SKEY_HAS, subkeys.SKEY_BAD) == (PART, HAS, BAD)
    assert subkeys.NO_BLOB == NONE
    header = (rm.ROOT / "include" / "k2hash_amd.h").read_text()
    for define in ("#define K2H_AMD_SKEY_PART 0x1u   /* participant */",
                   "#define K2H_AMD_SKEY_HAS  0x2u   /* skeys_length != 0 */",
                   "#define K2H_AMD_SKEY_BAD  0x4u   /* HAS, and the strict walk rejected the segment: no edges */"):
        assert define in header, define
    assert len(_native.SIGNATURES["k2h_amd_ralledata_subkeys"][1]) == 13
    assert len(_native.SIGNATURES["k2h_amd_ralledata_reach"][1]) == 9
    for fn in (subkeys.subkey_edges, subkeys.reach_subkeys, subkeys.subtree_ralledata):
        assert inspect.signature(fn).parameters["stream"].default is None
    assert list(inspect.signature(subkeys.subkey_edges).parameters) == [
        "blobs", "blob_off", "consider", "std_fnv", "want_rep", "count_only", "stream"]
    assert subkeys.SubkeyCounts._fields == ("participants", "with_edges", "bad", "edges", "dangling")
    for phrase in ("once with child NULL, twice otherwise", "levels + 2 times", "the LAST participant of an identity"):
        assert phrase in " ".join(header.split()).replace(" * ", " "), phrase


def test_argument_validation(oracle):
    """Judged on the host before any device is touched: the same answers with and without a
    GPU, each with its own message."""
    lib = _native.batch_lib()
    buf, off = rm.stream_of(oracle, rm.records(oracle, 4, seed=3))
    a, aoff = np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64)
    n = aoff.size - 1
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    flags, eoff = np.full(n, 0xEE, np.uint8), np.full(n + 1, 0xEE, np.uint64)
    counts = (ctypes.c_uint64 * 5)()
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    msg = lambda: bytes(lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL))  # noqa: E731

    def args(**kw):
        d = dict(blobs=p(a), off=p(aoff), n=n, fl=0, flags=p(flags), eoff=p(eoff), counts=cp)
        d.update(kw)
        return (d["blobs"], a.size, d["off"], d["n"], None, d["fl"], d["flags"], d["eoff"], None, None, 0, d["counts"],
                None)
    for i in range(5):
        counts[i] = 7
    assert lib.k2h_amd_ralledata_subkeys(*args(n=0, blobs=None, off=None, flags=None, eoff=None)) == _native.K2H_AMD_OK
    assert list(counts) == [0] * 5
    texts = set()
    for kw, text in ((dict(counts=None), b"NULL counts"), (dict(fl=_native.K2H_AMD_FLAG_CSTR), b"hashed as stored"),
                     (dict(fl=4), b"unknown flag bits"), (dict(flags=None), b"NULL sk_flags"),
                     (dict(eoff=None), b"NULL edge_off"), (dict(blobs=None), b"NULL blobs"),
                     (dict(off=None), b"NULL blob_off"), (dict(n=(1 << 32) - 1), b"2^32 - 2")):
        for i in range(5):
            counts[i] = 7
        assert lib.k2h_amd_ralledata_subkeys(*args(**kw)) == _native.K2H_AMD_EINVAL, kw
        assert text in msg() and msg().startswith(b"ralledata_subkeys: "), (kw, msg())
        if "counts" not in kw:
            assert list(counts) == [0] * 5
        texts.add(msg())
    assert len(texts) == 8
    assert (flags == 0xEE).all() and (eoff == 0xEE).all()

    rcounts = (ctypes.c_uint64 * 3)(7, 7, 7)
    rp = ctypes.cast(rcounts, ctypes.POINTER(ctypes.c_uint64))
    rep, child, roots, reach = np.zeros(n, np.uint64), np.zeros(1, np.uint64), np.zeros(n, np.uint8), np.full(n, 0xEE, np.uint8)

    def rargs(**kw):
        d = dict(eoff=p(eoff), child=p(child), rep=p(rep), n=n, roots=p(roots), reach=p(reach), counts=rp)
        d.update(kw)
        return d["eoff"], d["child"], d["rep"], d["n"], d["roots"], 0, d["reach"], d["counts"], None
    assert lib.k2h_amd_ralledata_reach(None, None, None, 0, None, 0, None, rp, None) == _native.K2H_AMD_OK
    assert list(rcounts) == [0, 0, 1]
    texts = set()
    for kw, text in ((dict(counts=None), b"NULL counts"), (dict(reach=None), b"NULL reach"),
                     (dict(eoff=None), b"NULL edge_off"), (dict(child=None), b"NULL child"), (dict(rep=None), b"NULL rep"),
                     (dict(roots=None), b"NULL roots"), (dict(n=1 << 33), b"2^32 - 2")):
        assert lib.k2h_amd_ralledata_reach(*rargs(**kw)) == _native.K2H_AMD_EINVAL, kw
        assert text in msg() and msg().startswith(b"ralledata_reach: "), (kw, msg())
        texts.add(msg())
    assert len(texts) == 7 and (reach == 0xEE).all()


# ------------------------------------------------------------------------ the test streams
def fixture_stream(oracle, golden):
    """Every fixture segment, and the strictly BAD ones the fixture cannot hold, as the subkeys
    of a blob of its own, directly followed -- as the blob's attrs segment -- by bytes that would
    be accepted if the walk read across the boundary: the rest of the list the segment was cut
    from, else one more well-formed entry.  Then one blob per distinct name, so that every name
    the walk emits addresses exactly one blob.  Returns (blobs, number of segment blobs)."""
    whole = {c["name"]: c["seg"] for c in golden["cases"] if "cut_of" not in c}
    extra = sm.serialize([b"across"])[8:]
    segs, tails = [], []
    for c in golden["cases"]:
        segs.append(c["seg"])
        tails.append(whole[c["cut_of"]][c["cut"]:] if "cut_of" in c else extra)
    bad = sm.strictly_bad_segments()
    full = sm.serialize([b"first-name", b"\x00second\xff"])
    segs += bad
    tails += [full[len(s):] for s in bad]
    names = sorted({nm for s in whole.values() for nm in sm.names_of(s)} | {b"first-name", b"\x00second\xff", b"across"})
    keys = [b"holder-%04d" % i for i in range(len(segs))] + names
    vals = [b"v"] * len(keys)
    blobs = rm.split(*rm.stream_of(oracle, (keys, vals, segs + [b""] * len(names), tails + [b""] * len(names))))
    for b, s in zip(blobs, segs):      # the continuation really is what follows the segment
        f = [rm.get(b, 0, 8 * k) for k in range(10)]
        assert f[4] == len(s) and f[9] == f[8] + f[4]
    return blobs, len(segs)


def forest(oracle, variant=0, seed=7):
    """About 2000 blobs: lists of 0, 1, 2, 63, 64, 65 and 300 names, name lengths 1..40 and one
    of 4 KiB, dangling names, a name whose target stores a wrong hash, a key that occurs three
    times with different lists, blobs of each non-participating kind, and later blobs whose stored
    hash shares every sorted bit with a named target's.  Returns (blobs, consider)."""
    rng = np.random.default_rng(seed)
    n_keys = 1900
    keys = []
    seen = set()
    while len(keys) < n_keys:
        k = bytes(rng.integers(0, 256, int(rng.integers(1, 41)), dtype=np.uint8))
        if k not in seen:
            seen.add(k)
            keys.append(k)
    big = bytes(rng.integers(0, 256, 4096, dtype=np.uint8))
    keys.append(big)
    pick = lambda k: [keys[int(j)] for j in rng.integers(0, len(keys), k)]  # noqa: E731
    lists = []
    for i in range(len(keys)):
        k = int(rng.choice([0, 0, 0, 1, 2, 2, 3, 5]))
        names = pick(k)
        if names and rng.random() < 0.15:
            names[0] = b"dangling-%d" % i
        lists.append(sm.serialize(names) if k or rng.random() < 0.1 else b"")
    for at, k in ((10, 63), (11, 64), (12, 65), (13, 300)):
        lists[at] = sm.serialize(pick(k - 1) + [big] if k == 65 else pick(k))
    lists[14] = sm.serialize([big, b"dangling-big" + big])
    lists[15] = sm.serialize(pick(4), count=9)                      # BAD: count larger than the entries
    lists[16] = sm.serialize(pick(2))[:-3]                          # BAD: the last name cut
    lists[17] = b"\x01\x00\x00"                                     # BAD: L < 8
    lists[18] = sm.serialize([keys[20], b"", keys[21], keys[20]])   # a zero-length entry, a duplicate
    order = list(range(len(keys)))
    # a key three times with different lists: the copies at three places of the stream
    triple = 30
    rec_keys = [keys[i] for i in order] + [keys[triple], keys[triple]]
    rec_lists = list(lists) + [sm.serialize([keys[40], keys[41]]), sm.serialize([keys[42]])]
    lists[19] = sm.serialize([keys[triple], keys[31]])              # names the tripled key and a wrong-hash target
    rec_lists[19] = lists[19]
    blobs = sm.blobs_with_lists(oracle, rec_keys, rec_lists, variant=variant)
    # keys[31]'s blob stores a wrong hash: not found by name
    dm.set_hash(blobs[31], rm.get(blobs[31], 0, rm.F_HASH) ^ (1 << 50))
    # behind every blob: blobs of other keys whose stored hash agrees with a named target's in the low 40 bits
    # (every sorted bit), with its subhash, with both and the key's length, and the target's own key under its
    # hash and another subhash -- the resolve steps over them
    shadows = []
    for t in range(100, 112):
        h, s = rm.get(blobs[t], 0, rm.F_HASH), rm.get(blobs[t], 0, rm.F_SUBHASH)
        other = bytes((x + 1) & 0xff for x in keys[t])
        for j, (key, hh, ss) in enumerate(((b"shadow-a-%d" % t, h ^ (1 << 44), None), (b"shadow-b-%d" % t, h, None),
                                           (other, h, s), (keys[t], h, s ^ 1))):
            b = sm.blobs_with_lists(oracle, [key], [sm.serialize([keys[t]]) if j == 0 else b""], variant=variant)[0]
            shadows.append(dm.set_hash(b, hh, ss))
    lists_named = [sm.serialize([keys[t] for t in range(100, 112)])]
    blobs += shadows + sm.blobs_with_lists(oracle, [b"names-the-shadowed"], lists_named, variant=variant)
    # non-participants of each kind
    junk = sm.blobs_with_lists(oracle, [b"empty", b"no-key", b"bad-range", b"left-out"],
                               [sm.serialize([keys[1]])] * 4, variant=variant)
    for f in (rm.F_KLEN, rm.F_VLEN, rm.F_SLEN, rm.F_ALEN):
        rm.put(junk[0], 0, f, 0)
    rm.put(junk[1], 0, rm.F_KLEN, 0)
    rm.put(junk[2], 0, 8 * 8, len(junk[2]))          # the subkeys' pos: the segment runs past the blob
    blobs = blobs[:700] + junk[:2] + blobs[700:] + junk[2:] + [bytearray(b"\x01" * 40)]   # ... and a bad span
    consider = np.ones(len(blobs), np.uint8)
    consider[len(blobs) - 2] = 0                     # "left-out"
    consider[rng.integers(0, len(blobs), 25)] = 0
    return dm.at_odd_offsets(blobs, seed=seed), consider


def shapes(oracle):
    """The reach test's stream: (blobs, consider, {name: blob index})."""
    recs, at = [], {}

    def add(key, names=None, seg=None, tag=None):
        at[tag or key] = len(recs)
        recs.append((key, seg if seg is not None else (sm.serialize(names) if names is not None else b"")))
    add(b"loop", [b"loop"])
    add(b"two-a", [b"two-b"])
    add(b"two-b", [b"two-a"])
    add(b"dia", [b"dia-l", b"dia-r"])
    add(b"dia-l", [b"dia-end"])
    add(b"dia-r", [b"dia-end", b"nobody"])
    add(b"dia-end")
    for k in range(71):
        add(b"chain-%02d" % k, [b"chain-%02d" % (k + 1)] if k < 70 else None)
    add(b"relaid", [b"old-child"], tag="relaid-first")
    add(b"old-child", [b"old-grandchild"])
    add(b"old-grandchild")
    add(b"new-child")
    add(b"outsider", [b"chain-69"])
    add(b"left-out", [b"dia"])
    add(b"path-a", [b"path-b"])
    add(b"path-b", seg=sm.serialize([b"path-c"])[:-2])        # a BAD list in the middle of a path
    add(b"path-c")
    add(b"wide", [b"leaf-%03d" % k for k in range(300)] + [b"dia-l"])
    for k in range(300):
        add(b"leaf-%03d" % k, [b"chain-60"] if k == 299 else None)
    add(b"relaid", [b"new-child"], tag="relaid-last")
    rng = np.random.default_rng(5)
    for k in range(200):
        add(b"fill-%03d" % k, [b"fill-%03d" % int(j) for j in rng.integers(0, 200, int(rng.integers(0, 4)))])
    blobs = sm.blobs_with_lists(oracle, [k for k, _s in recs], [s for _k, s in recs])
    consider = np.ones(len(blobs), np.uint8)
    consider[at[b"left-out"]] = 0
    return dm.at_odd_offsets(blobs, seed=3), consider, at


ROOT_SETS = (("loop",), ("two-a",), ("dia",), ("chain-00",), ("relaid-first",), ("relaid-last",), ("left-out",),
             ("dia", "dia-l", "outsider"), ("path-a",), ("wide",), ("wide", "chain-00", "loop", "fill-007"), ())


def _roots(at, names):
    return [at[x.encode() if x.encode() in at else x] for x in names]


def test_reach_model_is_the_transliterated_remove(oracle):
    """The traversal the device call is compared with marks exactly what Remove(key, true)
    removes, on every root set of the GPU test; the shapes are what they claim to be."""
    blobs, consider, at = shapes(oracle)
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off, consider=consider)
    assert m.flags[at[b"path-b"]] == PART | HAS | BAD and m.counts[4] >= 1
    depth = {}
    for names in ROOT_SETS:
        roots = _roots(at, names)
        want, _table = sm.removed_by(oracle, buf, off, roots, consider=consider)
        got, counts = sm.reach_model(m, roots)
        assert (got == want).all(), names
        assert counts[2] == 1 and counts[0] == int(want.sum())
        depth[names] = counts[1]
    assert depth[("chain-00",)] == 71 and depth[()] == 0 and depth[("left-out",)] == 0 and depth[("loop",)] == 1
    r, _t = sm.removed_by(oracle, buf, off, [at["relaid-first"]], consider=consider)
    assert r[at["relaid-first"]] and r[at["relaid-last"]] and r[at[b"new-child"]] and not r[at[b"old-child"]]
    r, _t = sm.removed_by(oracle, buf, off, [at[b"path-a"]], consider=consider)
    assert r[at[b"path-b"]] and not r[at[b"path-c"]]
    sub, c = sm.reach_model(m, [at[b"chain-00"]], max_levels=5)
    full, _c = sm.reach_model(m, [at[b"chain-00"]])
    assert c[1:] == [5, 0] and sub.sum() == 6 and ((sub <= full).all())


def test_forest_runs_the_step_over_path(oracle):
    """On the model side: distinct identities that share all sorted low bits exist where the
    resolve has to step over them -- later in the stream than the blob a name addresses."""
    blobs, consider = forest(oracle)
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off, consider=consider)
    mask = (1 << sort_bits_for(len(off) - 1 + m.counts[3])) - 1
    by_low = {}
    for i, ident in m.ident_of.items():
        by_low.setdefault(ident[0] & mask, []).append((i, ident))
    stepped = 0
    for e, nm in enumerate(m.names):
        c = int(m.child[e])
        if c != NONE:
            stepped += any(i > c and ident != m.ident_of[c] for i, ident in by_low[m.hashes[nm][0] & mask])
    assert stepped >= 5
    subs = {}                 # a named target's hash and key under two subhashes, the key of more than one chunk
    for _i, (h, s, key) in m.ident_of.items():
        subs.setdefault((h, key), set()).add(s)
    named = {nm for e, nm in enumerate(m.names) if int(m.child[e]) != NONE}
    assert any(len(v) > 1 and len(key) > 16 and key in named for (_h, key), v in subs.items())
    assert m.counts[2] >= 3 and m.counts[4] >= 20
    per = np.diff(m.edge_off.astype(np.int64))
    assert {0, 1, 2, 63, 64, 65, 300} <= set(int(x) for x in per)
    assert max(ln for _p, ln in m.where) >= 4096 and min(ln for _p, ln in m.where) == 1


# ===================================================================================== GPU
def _run(cuda, oracle, blobs, what, consider=None, variant=0, shift=5, **kw):
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off, consider=consider, variant=variant)
    t = tm.place(cuda, buf, shift)
    got = sm.run_subkeys(cuda, t, len(buf), off, consider, std_fnv=bool(variant), **kw)
    return m, got, buf, off


@pytest.mark.gpu
def test_fixture_segments_as_blobs(cuda, oracle, golden):
    blobs, nseg = fixture_stream(oracle, golden)
    m, got, _buf, _off = _run(cuda, oracle, blobs, "fixture")
    sm.assert_edges(got, m, "fixture segments")
    flags = got[1]
    for i, c in enumerate(golden["cases"]):
        assert bool(flags[i] & BAD) == (not c["accepted"]), c["name"]
    nbad = len(sm.strictly_bad_segments())
    assert (flags[len(golden["cases"]):nseg] == PART | HAS | BAD).all() and nseg - len(golden["cases"]) == nbad
    per = np.diff(got[2].astype(np.int64))
    assert (per[len(golden["cases"]):nseg] == 0).all()
    assert m.counts[4] == 0 and m.counts[3] > 70          # every emitted name found its one blob


@pytest.mark.gpu
@pytest.mark.parametrize("variant", (0, 1))
def test_edge_parity_on_a_forest(cuda, oracle, variant):
    blobs, consider = forest(oracle, variant)
    m, got, _buf, _off = _run(cuda, oracle, blobs, "forest", consider=consider, variant=variant, shift=3 + 8 * variant)
    sm.assert_edges(got, m, f"forest, variant {variant}")
    assert 1900 <= len(blobs) <= 4000


@pytest.mark.gpu
def test_edges_without_consider_and_without_rep(cuda, oracle):
    blobs, _consider = forest(oracle, seed=9)
    m, got, _buf, _off = _run(cuda, oracle, blobs[:600], "forest head", want_rep=False, shift=0)
    sm.assert_edges(got, m, "forest head, no consider, no rep", want_rep=False)
    assert (got[4] == np.uint64(0x5A5AA5A55A5AA5A5)).all()          # rep NULL: nothing of it was written


@pytest.mark.gpu
def test_reach_parity_with_remove(cuda, oracle):
    blobs, consider, at = shapes(oracle)
    m, got, buf, off = _run(cuda, oracle, blobs, "shapes", consider=consider)
    sm.assert_edges(got, m, "shapes")
    n = len(off) - 1
    for names in ROOT_SETS:
        roots = _roots(at, names)
        mask = np.zeros(n, np.uint8)
        mask[roots] = 1
        want, _table = sm.removed_by(oracle, buf, off, roots, consider=consider)
        reach, counts = sm.run_reach(cuda, m, mask)
        assert (reach == want).all(), (names, np.nonzero(reach != want)[0][:5])
        assert counts == sm.reach_model(m, roots)[1], names
    chain = np.zeros(n, np.uint8)
    chain[at[b"chain-00"]] = 1
    for limit in (1, 5, 70):
        reach, counts = sm.run_reach(cuda, m, chain, max_levels=limit)
        want, wc = sm.reach_model(m, [at[b"chain-00"]], max_levels=limit)
        assert (reach == want).all() and counts == wc and counts[1:] == [limit, 0], limit
    reach, counts = sm.run_reach(cuda, m, chain, max_levels=71)
    assert counts == [71, 71, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("remove", (False, True))
def test_subtree_ralledata(cuda, oracle, remove):
    import torch
    blobs, consider, at = shapes(oracle)
    buf, off = rm.join(blobs)
    roots = _roots(at, ("wide", "relaid-first", "path-a"))
    reach, table = sm.removed_by(oracle, buf, off, roots, consider=consider)
    t = tm.place(cuda, buf, 7)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    d_cons = torch.from_numpy(consider).to(cuda)
    d_roots = torch.tensor(roots, dtype=torch.int64, device=cuda)
    sel = subkeys.subtree_ralledata(t, d_off, d_roots, remove=remove, consider=d_cons)
    keep = (consider != 0) & (reach == 0) if remove else reach
    data, ooff, index = rm.select_model(np.frombuffer(bytes(buf), np.uint8), off, keep)
    assert sel.kept == len(index) and sel.kept_bytes == data.size
    assert (sel.blobs.cpu().numpy() == data).all() and (sel.index.cpu().numpy().view(np.uint64) == index).all()
    assert (sel.blob_off.cpu().numpy().view(np.uint64) == ooff).all()
    if remove:      # the kept stream, fed to the table, is the table after the removes
        kept = sm.Table(oracle, data.tobytes(), [int(x) for x in ooff]).elements
        assert kept == table and len(kept) < len(sm.Table(oracle, buf, off, consider=consider).elements)
    # the mask form of roots gives the same
    mask = torch.zeros(len(off) - 1, dtype=torch.bool, device=cuda)
    mask[d_roots] = True
    again = subkeys.subtree_ralledata(t, d_off, mask, remove=remove, consider=d_cons)
    assert torch.equal(again.blobs, sel.blobs) and torch.equal(again.index, sel.index)


@pytest.mark.gpu
def test_count_only_cap_and_empty_streams(cuda, oracle):
    import torch
    blobs, consider, _at = shapes(oracle)
    m, got, buf, off = _run(cuda, oracle, blobs, "shapes", consider=consider, count_only=True)
    assert got[0] == 0 and (got[1] == m.flags).all() and (got[2] == m.edge_off).all()
    assert got[5] == m.counts[:4] + [0] and got[3] is None
    # cap < E: EINVAL that names E, counts and edge_off filled, nothing written to child or rep
    E = m.counts[3]
    rc, flags, eoff, child, rep, counts = sm.run_subkeys(cuda, tm.place(cuda, buf, 1), len(buf), off, consider, cap=E - 1)
    assert rc == _native.K2H_AMD_EINVAL
    text = bytes(_native.batch_lib().k2h_amd_strerror(rc))
    assert text.startswith(b"ralledata_subkeys: ") and (b"E = %d" % E) in text, text
    assert (eoff == m.edge_off).all() and counts == m.counts[:4] + [0]
    assert (child == np.uint64(0x5A5AA5A55A5AA5A5)).all() and (rep == np.uint64(0x5A5AA5A55A5AA5A5)).all()
    # the wrapper: counts as a named tuple, count_only, n == 0, and a stream without subkeys
    t = tm.place(cuda, buf, 2)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    d_cons = torch.from_numpy(consider).to(cuda)
    only = subkeys.subkey_edges(t, d_off, consider=d_cons, count_only=True)
    assert only.child is None and only.rep is None and tuple(only.counts) == tuple(m.counts[:4] + [0])
    full = subkeys.subkey_edges(t, d_off, consider=d_cons)
    assert tuple(full.counts) == tuple(m.counts) and full.counts.edges == E and full.counts.dangling == m.counts[4]
    assert (full.child.cpu().numpy().view(np.uint64) == m.child).all()
    assert (full.rep.cpu().numpy().view(np.uint64) == m.rep).all()
    none = subkeys.subkey_edges(t[:0], d_off[:1] * 0)
    assert tuple(none.counts) == (0, 0, 0, 0, 0) and none.edge_off.cpu().tolist() == [0] and none.child.numel() == 0
    r = subkeys.reach_subkeys(none, torch.zeros(0, dtype=torch.uint8, device=cuda))
    assert (r.reached, r.levels, r.converged) == (0, 0, True)
    plain = dm.at_odd_offsets(dm.blobs_of(oracle, [b"k%d" % i for i in range(300)], [b"v"] * 300), seed=1)
    pbuf, poff = rm.join(plain)
    e = subkeys.subkey_edges(tm.place(cuda, pbuf, 4), torch.tensor(poff, dtype=torch.int64, device=cuda))
    assert tuple(e.counts) == (300, 0, 0, 0, 0) and e.child.numel() == 0 and (e.edge_off == 0).all()
    assert (e.rep.cpu().numpy() == np.arange(300)).all() and (e.flags == PART).all()
    r = subkeys.reach_subkeys(e, torch.tensor([5, 17], dtype=torch.int64, device=cuda))
    assert (r.reached, r.levels, r.converged) == (2, 1, True) and r.mask.cpu().numpy().nonzero()[0].tolist() == [5, 17]
