"""k2h_amd_ralledata_unlink and k2h_amd_subkeys_drop_mask (include/k2hash_amd.h section
4b'''''''), and drop_mask / unlink_subkeys / prune_ralledata of k2hash_amd/subkeys.py.

The rewritten list is pinned to the reference's own K2HSubKeys::erase + Serialize by
tests/golden/ralle_unlink.json (gen_ralle_unlink.cc); everything else is compared with
ralle_unlink_model.py: a sequential model of the call, and a transliteration of
K2HShm::Remove(key, subkey).  Expected values come only from the model and the fixture, never
from a device call.
"""
import ctypes
import inspect
import struct

import numpy as np
import pytest

import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_subkeys_model as sm
import ralle_times_model as tm
import ralle_unlink_model as um
from ralle_subkeys_model import BAD, HAS, NONE, PART
from ralle_unlink_model import EMPTIED, KEY_ONLY, REWRITTEN

from k2hash_amd import _native, subkeys


# ------------------------------------------------------------------------ the test streams
def raw_blob(oracle, key, val=b"", seg=b"", attrs=b"", order=(0, 1, 2, 3), gap=0):
    """A blob whose segments (0 key, 1 value, 2 subkeys, 3 attrs) lie in `order`, each behind
    `gap` filler bytes; a zero-length segment gets the position it would have."""
    parts, pos, body = [key, val, seg, attrs], [0] * 4, b""
    for s in order:
        body += b"\xcc" * gap
        pos[s] = rm.HEADER + len(body)
        body += parts[s]
    return bytearray(struct.pack("<10Q", oracle.k2h_hash(key, 0), oracle.k2h_second_hash(key, 0),
                                 *[len(x) for x in parts], *pos) + body)


def overlapping_blob(oracle, key, seg):
    """Key, then the list; the value is the key without its first byte, the attrs are the list's
    last five bytes: the four lengths add up to more than the blob holds."""
    return bytearray(struct.pack("<10Q", oracle.k2h_hash(key, 0), oracle.k2h_second_hash(key, 0), len(key), len(key) - 1,
                                 len(seg), 5, rm.HEADER, rm.HEADER + 1, rm.HEADER + len(key),
                                 rm.HEADER + len(key) + len(seg) - 5) + key + seg)


def name_of(i, salt=0):
    """Name i: 1 + (7 i + salt) % 40 bytes that differ from name to name."""
    ln = 1 + (7 * i + salt) % 40
    return bytes([i & 0xff, 0x80 | (i >> 8 & 0x7f)] + [33 + (i * 13 + j * 5 + salt) % 90 for j in range(2, ln)])[:ln]


def shapes(oracle):
    """The shapes where the kernel can go wrong: (blobs, {tag: blob index}, {blob index: the edge
    numbers within the blob to drop}, keep)."""
    blobs, at, spec = [], {}, {}

    def add(tag, blob, drops=()):
        at[tag] = len(blobs)
        blobs.append(blob)
        if drops:
            spec[at[tag]] = set(drops)
    a, b, c = b"name-a", b"\x00name-b\xff", b"c"
    add("one-emptied", raw_blob(oracle, b"one", b"value", sm.serialize([a])), [0])
    for k, tag in enumerate(("first", "middle", "last")):
        add("three-" + tag, raw_blob(oracle, b"three-" + tag.encode(), b"v", sm.serialize([a, b, c]), b"attrs"), [k])
    seventy = [name_of(i, 1) for i in range(70)]
    add("seventy", raw_blob(oracle, b"seventy", b"v" * 33, sm.serialize(seventy)), range(0, 70, 2))
    rng = np.random.default_rng(11)
    long = [name_of(i, 5) for i in range(3000)]
    add("long", raw_blob(oracle, b"long-list", b"v", sm.serialize(long), b"behind the long list"),
        [k for k in range(3000) if k % 3 == 0 or 1000 <= k < 1100 or rng.random() < 0.1])
    forty = [bytes(65 + (3 * i + j) % 50 for j in range(i + 1)) for i in range(40)]
    assert [len(x) for x in forty] == list(range(1, 41))
    for al in range(16):     # the key's length moves the list to every alignment
        add("align-%d" % al, raw_blob(oracle, b"k" * (al + 1), b"vv", sm.serialize(forty), b"at"),
            [k for k in range(40) if (k * 7 + al) % 3 == 0])
    add("zero-and-trail", raw_blob(oracle, b"zero-and-trail", b"v", sm.serialize([a, b"", b, c], trail=b"trailing!")), [1])
    add("count-smaller", raw_blob(oracle, b"count-smaller", b"v", sm.serialize([a, b, c], count=2), b"x"), [0])
    add("duplicates", raw_blob(oracle, b"duplicates", b"v", sm.serialize([a, b, a])), [0])
    add("permuted", raw_blob(oracle, b"permuted", b"the value", sm.serialize([a, b, c]), b"the attrs", order=(3, 2, 1, 0), gap=3),
        [1])
    add("gaps", raw_blob(oracle, b"gaps", b"", sm.serialize(seventy[:9]), b"", order=(2, 0, 1, 3), gap=17), [0, 8])
    add("overlapping", overlapping_blob(oracle, b"overlapping-key" + b"y" * 40, sm.serialize([a, b, c])), [2])
    add("overlapping-emptied", overlapping_blob(oracle, b"overlapping-key-2", sm.serialize([a])), [0])
    big = oracle.gen_bytes(64 << 10, byte_off=77).tobytes()
    add("big-value", raw_blob(oracle, b"big-value", big, sm.serialize([a, b, c]), b"after 64 KiB"), [1])
    add("big-value-last", raw_blob(oracle, b"big-value-2", big, sm.serialize([c, b]), order=(0, 2, 1, 3)), [0])
    add("key-only", raw_blob(oracle, b"key-and-list", b"", sm.serialize([a, b])), [0, 1])
    add("attrs-only-emptied", raw_blob(oracle, b"attrs-beside", b"", sm.serialize([a]), b"attrs"), [0])
    add("attrs-only", raw_blob(oracle, b"attrs-beside-2", b"", sm.serialize([a, b]), b"attrs"), [1])
    no_key = raw_blob(oracle, b"no-key", b"v", sm.serialize([a]))
    rm.put(no_key, 0, rm.F_KLEN, 0)
    add("non-participant", no_key)
    add("bad-segment", raw_blob(oracle, b"bad-segment", b"v", sm.serialize([a, b])[:-2], b"attrs"))
    add("untouched", raw_blob(oracle, b"untouched", b"v", sm.serialize([a, b, c], trail=b"kept as it is")))
    add("no-list", raw_blob(oracle, b"no-list", b"v"))
    add("earlier-copy", raw_blob(oracle, b"twice", b"old", sm.serialize([a, b])), [1])
    add("later-copy", raw_blob(oracle, b"twice", b"new", sm.serialize([b, c])))
    add("left-out", raw_blob(oracle, b"left-out", b"v", sm.serialize([a, b])), [0])
    add("short", bytearray(b"\x01" * 40))
    for k in range(300):     # more than one tile, and plain neighbours for the rewritten blobs
        drops = [0] if k % 50 == 7 else []
        add("fill-%d" % k, raw_blob(oracle, b"fill-%03d" % k, b"v%d" % k, sm.serialize([name_of(k, 2), a]) if k % 5 == 2 else b""),
            drops)
    order = list(range(len(blobs)))
    rng.shuffle(order)       # the shapes among the fill, not in front of it
    back = {old: new for new, old in enumerate(order)}
    blobs = [blobs[i] for i in order]
    at = {k: back[v] for k, v in at.items()}
    spec = {back[k]: v for k, v in spec.items()}
    keep = np.ones(len(blobs), np.uint8)
    keep[at["left-out"]] = 0
    return dm.at_odd_offsets(blobs, seed=4), at, spec, keep


def drop_of(m, spec):
    drop = np.zeros(m.counts[3], np.uint8)
    for i, ks in spec.items():
        e0, e1 = int(m.edge_off[i]), int(m.edge_off[i + 1])
        for k in ks:
            assert k < e1 - e0, (i, k, e1 - e0)
            drop[e0 + k] = 1
    return drop


def forest(oracle, seed=7, n_keys=2000):
    """About 2000 blobs with lists of 0..5 names over the stream's keys, some dangling, some
    blobs without a value, a few BAD lists and non-participants."""
    rng = np.random.default_rng(seed)
    keys = [b"key-%04d-" % i + bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8)) for i in range(n_keys)]
    lists = []
    for i in range(n_keys):
        k = int(rng.choice([0, 0, 1, 2, 3, 5]))
        names = [keys[int(j)] for j in rng.integers(0, n_keys, k)]
        if names and rng.random() < 0.2:
            names[int(rng.integers(0, len(names)))] = b"dangling-%d" % i
        lists.append(sm.serialize(names) if names else b"")
    lists[5] = sm.serialize([keys[1], keys[2]])[:-1]
    lists[6] = sm.serialize([keys[1]], count=4)
    blobs = sm.blobs_with_lists(oracle, keys, lists)
    for i in range(40, n_keys, 97):
        blobs[i] = raw_blob(oracle, keys[i], b"", lists[i], b"a" * (i % 2))
    rm.put(blobs[9], 0, rm.F_KLEN, 0)
    return dm.at_odd_offsets(blobs, seed=seed), keys


# ===================================================================================== CPU
@pytest.fixture(scope="module")
def golden():
    return um.fixture()


def _dropped_edges(seg, erase):
    """The edges of a written list (strictly ascending: one edge per name) whose name is erased."""
    names = sm.names_of(seg)
    return {k for k, nm in enumerate(names) if nm in erase}


def test_model_list_on_reference_fixture(golden):
    """The model's rewritten list is what the reference's own erase + Serialize leaves."""
    lists, cases = golden
    assert len(cases) >= 40 and set(lists) == {"written-1", "written-2", "written-3", "written-70"}
    emptied = unchanged = 0
    for c in cases:
        seg = lists[c["list"]]
        names = sm.names_of(seg)
        assert names == sorted(set(names)) and all(names)      # as the reference writes it
        dropped = _dropped_edges(seg, set(c["erase"]))
        assert len(dropped) == c["erased"], c["name"]
        new, d = um.rewritten_list(seg, dropped)
        assert new == c["out"] and d == c["erased"], c["name"]
        emptied += not c["out"]
        unchanged += c["out"] == seg
    assert emptied >= 4 and unchanged >= 8
    kinds = {c["name"].split("-erase-")[1].rstrip("0123456789-") for c in cases}
    assert {"first", "middle", "last", "every-other", "all", "none", "absent"} <= kinds


def test_model_without_drops_is_the_input(oracle):
    blobs, at, spec, keep = shapes(oracle)
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off)
    for drop in (None, np.zeros(m.counts[3], np.uint8)):
        for kp in (None, keep):
            u = um.unlink_model(buf, off, m.flags, m.edge_off, drop, keep=kp)
            data, ooff, index = rm.select_model(np.frombuffer(bytes(buf), np.uint8), off, np.ones(len(blobs)) if kp is None else kp)
            assert u.out == data.tobytes() and (u.out_off == ooff).all() and (u.index == index).all()
            assert u.counts == [len(index), data.size, 0, 0, 0, 0, 0] and not u.changed.any()
            for j, i in enumerate(u.index):
                assert u.out[int(u.out_off[j]):int(u.out_off[j + 1])] == bytes(buf[off[int(i)]:off[int(i) + 1]])


def test_model_on_the_shapes(oracle):
    """The shapes are what they claim to be, on the model side."""
    blobs, at, spec, keep = shapes(oracle)
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off)
    u = um.unlink_model(buf, off, m.flags, m.edge_off, drop_of(m, spec), keep=keep)
    ch = {k: int(u.changed[i]) for k, i in at.items()}
    assert ch["one-emptied"] == REWRITTEN | EMPTIED and ch["key-only"] == REWRITTEN | EMPTIED | KEY_ONLY
    assert ch["attrs-only-emptied"] == REWRITTEN | EMPTIED and ch["attrs-only"] == REWRITTEN
    assert ch["overlapping-emptied"] == REWRITTEN | EMPTIED and ch["earlier-copy"] == REWRITTEN and ch["later-copy"] == 0
    for tag in ("non-participant", "bad-segment", "untouched", "no-list", "left-out", "short"):
        assert ch[tag] == 0, tag
    assert m.flags[at["bad-segment"]] == PART | HAS | BAD and m.flags[at["non-participant"]] == 0
    pos = {int(i): j for j, i in enumerate(u.index)}

    def out_blob(tag):
        j = pos[at[tag]]
        return u.out[int(u.out_off[j]):int(u.out_off[j + 1])]
    f = struct.unpack_from("<10Q", out_blob("overlapping"))
    assert len(out_blob("overlapping")) == 80 + sum(f[2:6]) > len(blobs[at["overlapping"]])   # it grows
    assert sm.names_of(out_blob("zero-and-trail")[f_seg(out_blob("zero-and-trail"))]) == [b"name-a", b"c"]
    assert sm.names_of(out_blob("count-smaller")[f_seg(out_blob("count-smaller"))]) == [b"\x00name-b\xff"]
    assert sm.names_of(out_blob("duplicates")[f_seg(out_blob("duplicates"))]) == [b"\x00name-b\xff", b"name-a"]
    assert len(sm.names_of(out_blob("long")[f_seg(out_blob("long"))])) == 3000 - len(spec[at["long"]]) > 1500
    assert out_blob("bad-segment") == bytes(blobs[at["bad-segment"]]) and at["left-out"] not in pos
    assert u.counts[2] == len(spec) - 1 and u.counts[4] == 4 and u.counts[5] == 1 and u.counts[6] == 0
    assert u.counts[3] == sum(len(v) for k, v in spec.items() if k != at["left-out"])
    assert len(blobs) > 256


def f_seg(blob):
    f = struct.unpack_from("<10Q", blob)
    return slice(f[8], f[8] + f[4])


def test_public_names_and_header_constants():
    import k2hash_amd
    for name in ("drop_mask", "unlink_subkeys", "prune_ralledata", "Unlinked"):
        assert hasattr(k2hash_amd, name) and name in k2hash_amd.__all__, name
    assert (subkeys.UNLINK_REWRITTEN, subkeys.UNLINK_EMPTIED, subkeys.UNLINK_KEY_ONLY) == (REWRITTEN, EMPTIED, KEY_ONLY)
    header = (rm.ROOT / "include" / "k2hash_amd.h").read_text()
    for define in ("#define K2H_AMD_UNLINK_REWRITTEN 0x1u", "#define K2H_AMD_UNLINK_EMPTIED   0x2u",
                   "#define K2H_AMD_UNLINK_KEY_ONLY  0x4u"):
        assert define in header, define
    assert len(_native.SIGNATURES["k2h_amd_ralledata_unlink"][1]) == 15
    assert len(_native.SIGNATURES["k2h_amd_subkeys_drop_mask"][1]) == 7
    for fn in (subkeys.drop_mask, subkeys.unlink_subkeys, subkeys.prune_ralledata):
        assert inspect.signature(fn).parameters["stream"].default is None
    assert list(inspect.signature(subkeys.unlink_subkeys).parameters) == [
        "blobs", "blob_off", "edges", "drop", "keep", "out", "count_only", "stream"]
    assert list(inspect.signature(subkeys.prune_ralledata).parameters) == [
        "blobs", "blob_off", "roots", "dangling", "consider", "std_fnv", "out", "stream"]
    assert subkeys.Unlinked._fields == ("blobs", "blob_off", "index", "changed", "counts")
    assert len(subkeys.UnlinkCounts._fields) == 7
    doc = " ".join(subkeys.prune_ralledata.__doc__.split())
    for phrase in ("only from the one parent Remove(parent, name) is called on", "RemoveSubkeys skips names it does not find",
                   "a cleanup policy on top of the reference's rule, not a restatement of it"):
        assert phrase in doc, phrase
    text = " ".join(header.split()).replace(" * ", " ")
    for phrase in ("Detecting such lists is out of scope", "13 bytes per blob", "synchronised once, to return counts"):
        assert phrase in text, phrase


def test_argument_validation(oracle):
    """Judged on the host before any device is touched: the same answers with and without a
    GPU, each with its own message."""
    lib = _native.batch_lib()
    n = 4
    a, aoff = np.zeros(400, np.uint8), np.arange(n + 1, dtype=np.uint64) * 100
    flags, eoff, out, ooff = np.zeros(n, np.uint8), np.zeros(n + 1, np.uint64), np.full(400, 0xEE, np.uint8), np.zeros(n + 1, np.uint64)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    counts = (ctypes.c_uint64 * 7)()
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    msg = lambda: bytes(lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL))  # noqa: E731

    def args(**kw):
        d = dict(blobs=p(a), off=p(aoff), n=n, flags=p(flags), eoff=p(eoff), out=p(out), ooff=p(ooff), counts=cp)
        d.update(kw)
        return (d["blobs"], a.size, d["off"], d["n"], None, d["flags"], d["eoff"], None, d["out"], out.size, d["ooff"], None,
                None, d["counts"], None)
    for i in range(7):
        counts[i] = 7
    assert lib.k2h_amd_ralledata_unlink(*args(n=0, blobs=None, off=None, flags=None, eoff=None, out=None, ooff=None)) == 0
    assert list(counts) == [0] * 7
    texts = set()
    for kw, text in ((dict(counts=None), b"NULL counts"), (dict(blobs=None), b"NULL blobs"), (dict(off=None), b"NULL blob_off"),
                     (dict(flags=None), b"NULL sk_flags"), (dict(eoff=None), b"NULL edge_off"),
                     (dict(ooff=None), b"out given without out_off"), (dict(n=(1 << 32) - 1), b"2^32 - 2")):
        for i in range(7):
            counts[i] = 7
        assert lib.k2h_amd_ralledata_unlink(*args(**kw)) == _native.K2H_AMD_EINVAL, kw
        assert text in msg() and msg().startswith(b"ralledata_unlink: "), (kw, msg())
        if "counts" not in kw:
            assert list(counts) == [0] * 7
        texts.add(msg())
    assert len(texts) == 7 and (out == 0xEE).all()
    child, drop = np.zeros(3, np.uint64), np.full(3, 0xEE, np.uint8)
    assert lib.k2h_amd_subkeys_drop_mask(None, 0, None, 0, 1, None, None) == 0
    for kw, text in (((None, 3, None, 0, 0, p(drop), None), b"NULL child"), ((p(child), 3, None, 0, 0, None, None), b"NULL drop")):
        assert lib.k2h_amd_subkeys_drop_mask(*kw) == _native.K2H_AMD_EINVAL
        assert text in msg() and msg().startswith(b"subkeys_drop_mask: ")
    assert (drop == 0xEE).all()


def test_remove_subkey_model(oracle):
    """The transliterated Remove(key, subkey) on a small table: the name leaves the one parent's
    list, the child goes with everything below it, and the calls that do nothing do nothing."""
    ser = sm.serialize
    recs = [(b"p", b"pv", ser([b"c1", b"c2", b"nobody"])), (b"q", b"qv", ser([b"c1"])), (b"c1", b"v", ser([b"g"])),
            (b"c2", b"v", b""), (b"g", b"v", b""), (b"solo", b"", ser([b"c2"])), (b"bad", b"v", ser([b"g"])[:-1])]
    buf, off = rm.join([raw_blob(oracle, k, v, s) for k, v, s in recs])
    ident = lambda k: (oracle.k2h_hash(k, 0), oracle.k2h_second_hash(k, 0), k)  # noqa: E731
    t = um.UnlinkTable(oracle, buf, off)
    assert t.full() == um.fed(buf, off) and len(t.elements) == 7
    before = dict(t.elements)
    for key, name in ((b"absent", b"c1"), (b"p", b"not-in-list"), (b"c2", b"g"), (b"bad", b"g")):
        t.remove_subkey(key, name, set())
        assert t.elements == before, (key, name)
    removed = set()
    t.remove_subkey(b"p", b"c1", removed)
    assert removed == {ident(b"c1"), ident(b"g")} and t.elements[ident(b"p")] == ser([b"c2", b"nobody"])
    assert t.elements[ident(b"q")] == ser([b"c1"])              # another parent keeps the name: now dangling
    t.remove_subkey(b"p", b"nobody", removed)
    assert t.elements[ident(b"p")] == ser([b"c2"]) and len(removed) == 2
    t.remove_subkey(b"solo", b"c2", removed)
    assert t.full()[ident(b"solo")] == (None, None, None) and ident(b"c2") in removed


# ===================================================================================== GPU
def _run(cuda, oracle, blobs, spec, what, keep=None, shift=5, tail_pad=tm.PAD, **kw):
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off)
    drop = spec if spec is None or isinstance(spec, np.ndarray) else drop_of(m, spec)
    want = um.unlink_model(buf, off, m.flags, m.edge_off, drop, keep=keep)
    got = um.run_unlink(cuda, tm.place(cuda, buf, shift, tail_pad=tail_pad), len(buf), off, m.flags, m.edge_off, drop, keep=keep,
                        **kw)
    um.assert_unlinked(got, want, what)
    return m, want, got


@pytest.mark.gpu
def test_fixture_lists_in_blobs(cuda, oracle, golden):
    """Every fixture case as a blob at an odd offset: the device's list is the reference's
    bytes, and the header is GetElementToBinary's arithmetic."""
    lists, cases = golden
    blobs, spec = [], {}
    for i, c in enumerate(cases):
        seg = lists[c["list"]]
        blobs.append(raw_blob(oracle, b"holder-%03d" % i + b"x" * (i % 16), b"v" * (i % 7), seg, b"a" * (i % 3)))
        spec[i] = _dropped_edges(seg, set(c["erase"]))
    blobs = dm.at_odd_offsets(blobs, seed=2)
    _m, want, got = _run(cuda, oracle, blobs, {i: s for i, s in spec.items() if s}, "fixture")
    out, ooff = got[1], got[2]
    assert len(ooff) == len(cases) + 1
    for i, c in enumerate(cases):
        blob = out[int(ooff[i]):int(ooff[i + 1])]
        if not spec[i]:
            assert blob == bytes(blobs[i]) and got[4][i] == 0, c["name"]
            continue
        f = struct.unpack_from("<10Q", blob)
        src = struct.unpack_from("<10Q", blobs[i])
        assert f[:4] == src[:4] and f[5] == src[5] and f[4] == len(c["out"]), c["name"]
        assert f[6:] == (80, 80 + f[2], 80 + f[2] + f[3], 80 + f[2] + f[3] + f[4]) and len(blob) == 80 + sum(f[2:6]), c["name"]
        assert blob[f[8]:f[8] + f[4]] == c["out"], c["name"]
        assert blob[80:f[8]] == bytes(blobs[i][80:src[8]]) and blob[f[9]:] == bytes(blobs[i][src[9]:src[9] + src[5]]), c["name"]
        assert got[4][i] == REWRITTEN | (0 if c["out"] else EMPTIED) | (0 if c["out"] or f[3] or f[5] else KEY_ONLY), c["name"]


@pytest.mark.gpu
@pytest.mark.parametrize("with_keep", (False, True))
def test_random_forest(cuda, oracle, with_keep):
    blobs, _keys = forest(oracle)
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off)
    rng = np.random.default_rng(3)
    drop = (rng.random(m.counts[3]) < 0.3).astype(np.uint8) * rng.integers(1, 256, m.counts[3]).astype(np.uint8)
    keep = (rng.random(len(blobs)) < 0.7).astype(np.uint8) if with_keep else None
    _m, want, _got = _run(cuda, oracle, blobs, drop, f"forest, keep {with_keep}", keep=keep, shift=9 if with_keep else 0)
    assert want.counts[2] > 300 and want.counts[4] > 30 and want.counts[6] == 0 and 1900 <= len(blobs) <= 2100


@pytest.mark.gpu
def test_the_shapes(cuda, oracle):
    blobs, _at, spec, keep = shapes(oracle)
    _run(cuda, oracle, blobs, spec, "shapes", keep=keep, shift=13)
    _run(cuda, oracle, blobs, spec, "shapes, index NULL", keep=keep, shift=0, want_index=False, want_changed=False)


@pytest.mark.gpu
def test_no_drop_equals_select(cuda, oracle):
    import torch
    blobs, _at, _spec, keep = shapes(oracle)
    buf, off = rm.join(blobs)
    t = tm.place(cuda, buf, 6)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    d_keep = torch.from_numpy(keep).to(cuda)
    edges = subkeys.subkey_edges(t, d_off)
    sel = subkeys.select_ralledata(t, d_off, d_keep)
    data, ooff, index = rm.select_model(np.frombuffer(bytes(buf), np.uint8), off, keep)
    assert (sel.blobs.cpu().numpy() == data).all()
    for drop in (None, torch.zeros(edges.counts.edges, dtype=torch.uint8, device=cuda)):
        u = subkeys.unlink_subkeys(t, d_off, edges, drop, keep=d_keep)
        assert torch.equal(u.blobs, sel.blobs) and torch.equal(u.blob_off, sel.blob_off) and torch.equal(u.index, sel.index)
        assert tuple(u.counts) == (sel.kept, sel.kept_bytes, 0, 0, 0, 0, 0) and not bool(u.changed.any())
    _run(cuda, oracle, blobs, None, "drop NULL", keep=keep)


@pytest.mark.gpu
def test_mismatching_edge_off(cuda, oracle):
    """edge_off from another consider: the blobs whose edge counts disagree come out unchanged
    and are counted; the stream ends with its allocation."""
    blobs, at, spec, keep = shapes(oracle)
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off)
    consider = np.ones(len(blobs), np.uint8)
    consider[[at["seventy"], at["three-first"], at["align-3"]]] = 0
    other = sm.edges_model(oracle, buf, off, consider=consider)      # the three blobs' edges are missing
    drop = np.ones(other.counts[3], np.uint8)
    want = um.unlink_model(buf, off, m.flags, other.edge_off, drop, keep=keep)
    assert want.counts[6] >= 3 and want.counts[2] >= 20
    for tag in ("seventy", "three-first", "align-3"):
        assert want.changed[at[tag]] == 0
    t = tm.place(cuda, buf, 1, tail_pad=0)
    got = um.run_unlink(cuda, t, len(buf), off, m.flags, other.edge_off, drop, keep=keep)
    um.assert_unlinked(got, want, "mismatch")
    # flags that claim a participant where the header is none, a walk that is BAD, an edge range outside [0, E]
    flags = m.flags.copy()
    flags[at["non-participant"]] = PART | HAS
    flags[at["bad-segment"]] = PART | HAS
    flags[at["short"]] = PART | HAS
    eo = m.edge_off.copy()
    eo[at["bad-segment"] + 1:] += 1           # one edge for the BAD segment
    eo[at["non-participant"] + 1:] += 1
    eo[at["short"] + 1:] += 1
    drop = np.ones(int(eo[-1]), np.uint8)
    want = um.unlink_model(buf, off, flags, eo, drop, keep=keep)
    assert want.counts[6] >= 3
    um.assert_unlinked(um.run_unlink(cuda, t, len(buf), off, flags, eo, drop, keep=keep), want, "lying flags")
    eo = m.edge_off.copy()
    eo[at["three-last"]] += 1 << 40
    want = um.unlink_model(buf, off, m.flags, eo, np.ones(m.counts[3], np.uint8), keep=keep)
    assert want.counts[6] >= 1
    um.assert_unlinked(um.run_unlink(cuda, t, len(buf), off, m.flags, eo, np.ones(m.counts[3], np.uint8), keep=keep), want,
                       "edge range outside E")


def replay_stream(oracle, seed=5, n_keys=400):
    """Unique keys with strictly ascending lists (what the reference writes), some parents
    without a value, some dangling names."""
    rng = np.random.default_rng(seed)
    keys = [b"k%03d" % i for i in range(n_keys)]
    blobs = []
    for i in range(n_keys):
        k = 1 if i % 20 == 1 else int(rng.choice([0, 0, 1, 2, 4]))
        names = {keys[int(j)] for j in rng.integers(0, n_keys, k)}
        if names and i % 20 != 1 and rng.random() < 0.2:
            names.add(b"nobody-%d" % i)
        seg = sm.serialize(sorted(names)) if names else b""
        blobs.append(raw_blob(oracle, keys[i], b"" if i % 4 == 1 else b"v%d" % i, seg, b"at" if i % 9 == 0 else b""))
    return dm.at_odd_offsets(blobs, seed=seed), keys


def choose_edges(m, rng, want=40):
    """Edge sets D such that no parent in D lies in the closure of D's children; the only edges of
    some parents that have nothing but a key and a list are tried first."""
    E, D = m.counts[3], []
    lone = [int(m.edge_off[i]) for i in range(1, len(m.rep), 20) if int(m.edge_off[i + 1]) - int(m.edge_off[i]) == 1]
    for e in lone[:12] + list(rng.permutation(E)):
        if int(e) in D:
            continue
        cand = D + [int(e)]
        children = [int(m.child[x]) for x in cand if int(m.child[x]) != NONE]
        reach, _c = sm.reach_model(m, children)
        if not any(reach[m.owner[x]] for x in cand):
            D = cand
        if len(D) >= want:
            break
    return D


def replay_case(oracle, seed):
    """(buf, off, m, D, the table after Remove(parent, name) for every edge of D, the identities
    left with a key and nothing else)."""
    blobs, keys = replay_stream(oracle, seed)
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off)
    D = choose_edges(m, np.random.default_rng(seed))
    table = um.UnlinkTable(oracle, buf, off)
    removed = set()
    for e in D:
        table.remove_subkey(keys[m.owner[e]], m.names[e], removed)
    want = table.full()
    bare = {k for k, v in want.items() if v == (None, None, None)}
    return buf, off, m, D, want, bare, removed


@pytest.mark.parametrize("seed", (5, 6))
def test_replay_edge_sets(oracle, seed):
    """On the model side: D holds dangling names, parents that end with a key and nothing else,
    parents that keep other names, and children with subtrees of their own."""
    buf, off, m, D, want, bare, removed = replay_case(oracle, seed)
    assert len(D) >= 20 and any(int(m.child[e]) == NONE for e in D)
    assert len(bare) >= 2 and len(removed) > len({int(m.child[e]) for e in D} - {NONE})
    assert any(v[1] is not None for k, v in want.items() if k in {m.ident_of[m.owner[e]] for e in D})
    assert not removed & set(want)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", (5, 6))
def test_remove_parent_name_replay(cuda, oracle, seed):
    import torch
    buf, off, m, D, want, bare, removed = replay_case(oracle, seed)
    # the device: drop is D, roots are D's children, keep = ~reach
    t = tm.place(cuda, buf, 3)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    edges = subkeys.subkey_edges(t, d_off)
    drop = torch.zeros(edges.counts.edges, dtype=torch.uint8, device=cuda)
    drop[torch.tensor(D, dtype=torch.int64, device=cuda)] = 1
    roots = torch.tensor(sorted({int(m.child[e]) for e in D if int(m.child[e]) != NONE}), dtype=torch.int64, device=cuda)
    reach = subkeys.reach_subkeys(edges, roots).mask
    u = subkeys.unlink_subkeys(t, d_off, edges, drop, keep=(reach == 0))
    got = um.fed(u.blobs.cpu().numpy().tobytes(), u.blob_off.cpu().tolist())
    assert got == {k: v for k, v in want.items() if k not in bare}
    changed = u.changed.cpu().numpy()
    key_only = {m.ident_of[i] for i in np.nonzero(changed & KEY_ONLY)[0]}
    assert key_only == bare and u.counts.key_only == len(bare)
    assert u.counts.dropped == len(D) and u.counts.mismatches == 0


@pytest.mark.gpu
def test_prune_ralledata(cuda, oracle):
    import torch
    blobs, keys = forest(oracle, seed=8)
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off)
    assert m.counts[4] > 50 and m.counts[2] >= 2
    t = tm.place(cuda, buf, 11)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    roots = torch.tensor([20, 21, 300, 1500], dtype=torch.int64, device=cuda)
    for rts, dangling in ((None, True), (roots, True), (roots, False)):
        u = subkeys.prune_ralledata(t, d_off, rts, dangling=dangling)
        reach = np.zeros(len(blobs), np.uint8) if rts is None else sm.reach_model(m, rts.cpu().tolist())[0]
        drop = np.array([(c == NONE and dangling) or (c != NONE and reach[int(c)]) for c in m.child], np.uint8)
        want = um.unlink_model(buf, off, m.flags, m.edge_off, drop, keep=(reach == 0))
        assert tuple(u.counts) == tuple(want.counts) and u.blobs.cpu().numpy().tobytes() == want.out
        assert (u.changed.cpu().numpy() == want.changed).all()
        again = subkeys.subkey_edges(u.blobs, u.blob_off)
        m2 = sm.edges_model(oracle, want.out, [int(x) for x in want.out_off])
        assert tuple(again.counts) == tuple(m2.counts)
        if dangling:
            assert again.counts.dangling == 0
        else:
            assert again.counts.dangling == int(((m.child == np.uint64(NONE)) & (reach[np.array(m.owner)] == 0)).sum()) > 0
        was = m.flags[u.index.cpu().numpy()]
        now = again.flags.cpu().numpy()
        assert not ((now & BAD) & ~(was & BAD)).any() and again.counts.bad == int(((was & BAD) != 0).sum())
        if rts is not None:
            assert u.counts.emitted == len(blobs) - int(reach.sum()) < len(blobs)


@pytest.mark.gpu
def test_count_only_cap_and_empty_streams(cuda, oracle):
    import torch
    blobs, _at, spec, keep = shapes(oracle)
    buf, off = rm.join(blobs)
    m = sm.edges_model(oracle, buf, off)
    drop = drop_of(m, spec)
    want = um.unlink_model(buf, off, m.flags, m.edge_off, drop, keep=keep)
    t = tm.place(cuda, buf, 2)
    rc, out, _oo, _ix, changed, counts = um.run_unlink(cuda, t, len(buf), off, m.flags, m.edge_off, drop, keep=keep, count_only=True)
    assert rc == 0 and out is None and counts == want.counts and (changed == want.changed).all()
    # out_cap one byte short: EINVAL that names both figures, counts set, nothing written
    rc, out, ooff, _ix, changed, counts = um.run_unlink(cuda, t, len(buf), off, m.flags, m.edge_off, drop, keep=keep,
                                                        cap=want.counts[1] - 1)
    assert rc == _native.K2H_AMD_EINVAL and counts == want.counts and (changed == want.changed).all()
    text = bytes(_native.batch_lib().k2h_amd_strerror(rc))
    assert text.startswith(b"ralledata_unlink: ") and (b"%d" % want.counts[1]) in text and (b"%d" % (want.counts[1] - 1)) in text
    assert (ooff == np.uint64(0x5A5AA5A55A5AA5A5)).all()
    # the wrapper: count_only, a caller's out, one too small, n == 0, E == 0
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    edges = subkeys.subkey_edges(t, d_off)
    d_drop, d_keep = torch.from_numpy(drop).to(cuda), torch.from_numpy(keep).to(cuda)
    only = subkeys.unlink_subkeys(t, d_off, edges, d_drop, keep=d_keep, count_only=True)
    assert only.blobs is None and only.blob_off is None and only.index is None and tuple(only.counts) == tuple(want.counts)
    assert (only.changed.cpu().numpy() == want.changed).all()
    mine = torch.full((want.counts[1] + 32,), 0xC3, dtype=torch.uint8, device=cuda)
    u = subkeys.unlink_subkeys(t, d_off, edges, d_drop.view(torch.bool), keep=d_keep.view(torch.bool), out=mine)
    assert u.blobs.data_ptr() == mine.data_ptr() and u.blobs.cpu().numpy().tobytes() == want.out and bool((mine[want.counts[1]:] == 0xC3).all())
    with pytest.raises(_native.NativeError, match="exceed out_cap"):
        subkeys.unlink_subkeys(t, d_off, edges, d_drop, keep=d_keep, out=mine[:want.counts[1] - 1])
    with pytest.raises(ValueError, match="drop needs E entries"):
        subkeys.unlink_subkeys(t, d_off, edges, d_drop[:-1], keep=d_keep)
    none = subkeys.subkey_edges(t[:0], d_off[:1] * 0)
    z = subkeys.unlink_subkeys(t[:0], d_off[:1] * 0, none, subkeys.drop_mask(none, dangling=True))
    assert tuple(z.counts) == (0,) * 7 and z.blob_off.cpu().tolist() == [0] and z.blobs.numel() == 0 and z.changed.numel() == 0
    plain = dm.at_odd_offsets(dm.blobs_of(oracle, [b"k%d" % i for i in range(300)], [b"v"] * 300), seed=1)
    pbuf, poff = rm.join(plain)
    pt, po = tm.place(cuda, pbuf, 4), torch.tensor(poff, dtype=torch.int64, device=cuda)
    e = subkeys.subkey_edges(pt, po)
    assert e.counts.edges == 0
    u = subkeys.unlink_subkeys(pt, po, e, subkeys.drop_mask(e, gone=torch.ones(300, dtype=torch.uint8, device=cuda), dangling=True))
    assert u.blobs.cpu().numpy().tobytes() == bytes(pbuf) and tuple(u.counts) == (300, len(pbuf), 0, 0, 0, 0, 0)
    p = subkeys.prune_ralledata(pt, po, torch.tensor([3], dtype=torch.int64, device=cuda), dangling=True)
    assert p.counts.emitted == 299 and p.counts.rewritten == 0


@pytest.mark.gpu
def test_drop_mask(cuda):
    import torch

    import big_offsets as bo
    n, E = 1000, 5000
    rng = np.random.default_rng(2)
    child = rng.integers(0, n, E).astype(np.uint64)
    child[rng.random(E) < 0.2] = np.uint64(NONE)
    child[17] = n                     # out of range: no blob
    child[18] = (1 << 63) + 5
    gone = (rng.random(n) < 0.3).astype(np.uint8) * 7
    d_child = torch.from_numpy(child.view(np.int64)).to(cuda)
    d_gone = torch.from_numpy(gone).to(cuda)
    lib = _native.batch_lib()
    inside = np.where(child < n, child, 0).astype(np.int64)
    for g, dangling in ((d_gone, 0), (d_gone, 1), (None, 1), (None, 0), (d_gone, 5)):
        whole, drop = bo.guarded(torch, cuda, E, shift=1, fill=0xEE)
        rc = lib.k2h_amd_subkeys_drop_mask(bo._p(d_child), E, None if g is None else bo._p(g), n, dangling, bo._p(drop), bo._stream())
        torch.cuda.synchronize()
        assert rc == 0 and bo.guards_intact(torch, whole, drop, 0xEE)
        want = np.where(child == np.uint64(NONE), 1 if dangling else 0,
                        0 if g is None else ((child < n) & (gone[inside] != 0)).astype(np.uint8))
        assert (drop.cpu().numpy() == want).all(), dangling
    edges = subkeys.SubkeyEdges(torch.zeros(n, dtype=torch.uint8, device=cuda), torch.zeros(n + 1, dtype=torch.int64, device=cuda),
                                d_child, None, subkeys.SubkeyCounts(0, 0, 0, E, 0))
    got = subkeys.drop_mask(edges, gone=d_gone, dangling=True)
    assert got.dtype == torch.uint8 and got.numel() == E
    assert (got.cpu().numpy() == np.where(child == np.uint64(NONE), 1, (child < n) & (gone[inside] != 0))).all()
    with pytest.raises(ValueError, match="gone needs n entries"):
        subkeys.drop_mask(edges, gone=d_gone[:-1])
