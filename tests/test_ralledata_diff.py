"""Two RALLEDATA streams joined by identity (include/k2hash_amd.h section 4b''''':
k2h_amd_ralledata_diff; k2h_ralledata_diff.hip) against the model of ralle_diff_model.py, entry
for entry: rel, match, seen and the four counts.

The model is sequential: a dict from identity to the last participant of B, one look-up per
participant of A.  That the feed mask the header builds from rel is safe -- the table after the
fed blobs equals the table after all of A -- is shown on the CPU against the transliteration of
K2HShm::SetElementByBinArray in ralle_dedup_model.py, over real serialized attrs
(ralle_times_model.real_attrs); libk2hash itself is not built here, so parity with it is a
restatement.  Expected values never come from the device code, and every device output is
sentinel-filled first.
"""
import ctypes
import json
import struct

import numpy as np
import pytest

from conftest import GOLDEN

import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_diff_model as fm
import ralle_times_model as tm
from ralle_diff_model import APPLY, ATTRS, DATA, FOUND, NONE, PART, REPEAT, SKEY, VAL

from k2hash_amd import _native, ralledata

NOW = tm.NOW


@pytest.fixture(scope="module")
def golden():
    recs = json.loads((GOLDEN / "ralledata.json").read_text())["records"]
    return [bytearray(bytes.fromhex(r["blob"])) for r in recs]


# ---------------------------------------------------------------------------- blob builders
def fields(blob):
    return struct.unpack_from("<10Q", blob, 0)


def segments(blob):
    f = fields(blob)
    return [bytes(blob[f[6 + s]:f[6 + s] + f[2 + s]]) if f[2 + s] else b"" for s in range(4)]


def layout(hash_, sub, segs, order=(0, 1, 2, 3), slack=0, filler=0x11):
    """A blob of the four segments (key, value, subkeys, attrs) laid down in `order` with
    `slack` filler bytes before each and behind the last: positions are free, and
    SetElementByBinArray honours any.  A length-0 segment gets pos 0."""
    body, pos = bytearray(), [0, 0, 0, 0]
    for s in order:
        body += bytes([filler]) * slack
        if segs[s]:
            pos[s] = rm.HEADER + len(body)
            body += segs[s]
    body += bytes([filler]) * slack
    return bytearray(struct.pack("<10Q", hash_, sub, *(len(x) for x in segs), *pos)) + body


def relaid(blob, segs=None, **kw):
    """The blob's element, optionally with other segments, in another layout."""
    f = fields(blob)
    return layout(f[0], f[1], segs if segs is not None else segments(blob), **kw)


def with_segment(blob, s, data):
    segs = segments(blob)
    segs[s] = bytes(data)
    return relaid(blob, segs)


# ------------------------------------------------------------------------------------- CPU
def _mutated_fixture(golden):
    """A: the 48 reference blobs with chosen ones mutated; returns A and {index: bits}."""
    a = [bytearray(b) for b in golden]
    want = {}
    has = lambda i, s: fields(golden[i])[2 + s] != 0  # noqa: E731
    v = [i for i in range(48) if has(i, 1)]
    sk = [i for i in range(48) if has(i, 2)]
    at = [i for i in range(48) if has(i, 3)]
    assert len(v) > 4 and sk and at

    def flip(i, s, where):
        segs = segments(a[i])
        d = bytearray(segs[s])
        d[where] ^= 0x40
        a[i] = with_segment(a[i], s, d)
    flip(v[0], 1, 0)
    want[v[0]] = VAL
    flip(v[1], 1, -1)
    want[v[1]] = VAL
    flip(sk[0], 2, -1)
    want[sk[0]] = want.get(sk[0], 0) | SKEY
    flip(at[0], 3, 0)
    want[at[0]] = want.get(at[0], 0) | ATTRS
    a[v[2]] = with_segment(a[v[2]], 1, segments(a[v[2]])[1] + b"!")          # a value of another length
    want[v[2]] = want.get(v[2], 0) | VAL
    a[v[3]] = with_segment(a[v[3]], 1, b"")                                  # the value gone
    want[v[3]] = want.get(v[3], 0) | VAL
    new = relaid(a[v[4]], [segments(a[v[4]])[0] + b"-new"] + segments(a[v[4]])[1:])   # a new key under the old hash
    a.append(new)
    return a, want


def test_model_on_reference_fixture(golden):
    assert len(golden) == 48
    b = rm.join(golden)
    rel, match, seen, counts = fm.diff_model(*b, *b)
    base = np.array([PART | FOUND | (DATA if any(fields(g)[3:6]) else 0) for g in golden], np.uint8)
    assert (rel == base).all() and (match == np.arange(48)).all() and seen.all() and counts == [48, 48, 48, 0]
    a, want = _mutated_fixture(golden)
    rel, match, seen, counts = fm.diff_model(*rm.join(a), *b)
    # the new key stores an old blob's hash: not FOUND, and both blobs of that hash are REPEAT
    v4 = [i for i in range(48) if fields(a[i])[0] == fields(a[48])[0]]
    assert len(v4) == 1 and rel[48] == PART | DATA | REPEAT and match[48] == NONE
    for i in range(48):
        bits = int(base[i]) | want.get(i, 0) | (REPEAT if i == v4[0] else 0)
        if not any(fields(a[i])[3:6]):
            bits &= ~DATA
        assert rel[i] == bits, (i, hex(rel[i]), hex(bits))
        assert match[i] == i
    assert seen.all() and counts == [49, 48, 48 - len(want), 0]
    # with times every blob without a held one is APPLY, and a blob of A alone takes part
    rel, match, seen, counts = fm.diff_model(*rm.join(a[48:]), *b, times=((2000, 0), NOW))
    assert rel.tolist() == [PART | DATA | APPLY] and seen.sum() == 0 and counts == [1, 0, 0, 1]


def _ident(oracle, key):
    b = dm.blobs_of(oracle, [key], [b"x"])[0]
    return (rm.get(b, 0, rm.F_HASH), rm.get(b, 0, rm.F_SUBHASH), key)


def _feed_tables(oracle, a_blobs, table, pts, repeat_always=True):
    """(table after all of A, table after the fed blobs) from `table`, B being its dump."""
    b_blobs = fm.table_blobs(oracle, table)
    rel = fm.diff_model(*rm.join(a_blobs), *rm.join(b_blobs), times=(pts, NOW))[0]
    feed = fm.feed_of(rel, repeat_always)
    return dm.replay(a_blobs, table, pts), dm.replay([x for x, k in zip(a_blobs, feed) if k], table, pts), feed


def _single_key_cases(oracle):
    """(A's one blob, the table) for every attrs kind of A x with and without a value x the
    value equal to the held one or not, against every kind of held element."""
    ident = _ident(oracle, b"k")
    for bkind, table in tm.prior_states(ident).items():
        for akind, attrs in tm.ATTRS_KINDS.items():
            for val in (b"", b"prior-value", b"another"):
                yield (akind, bkind, val), dm.blobs_of(oracle, [b"k"], [val], None, [attrs])[0], table


def test_fed_blobs_replay_to_the_same_table_single_key(oracle):
    n = skipped = 0
    with tm.real_attrs(NOW):
        for what, blob, table in _single_key_cases(oracle):
            for pts in tm.PTS:
                whole, fed, feed = _feed_tables(oracle, [blob], table, pts)
                assert fed == whole, (what, pts)
                n += 1
                skipped += not feed[0]
    assert n == 12 * 10 * 3 * 5 and 200 < skipped < n


def test_apply_is_the_transliteration_going_on_to_write(oracle):
    """For every (A kind, B kind, pts): APPLY == set_element_by_bin_array got past :431, seen
    as `the element object was replaced or removed` on a table whose element differs from A's."""
    ident = _ident(oracle, b"k")
    n = applied = 0
    with tm.real_attrs(NOW):
        for bkind, table in tm.prior_states(ident).items():
            for akind, attrs in tm.ATTRS_KINDS.items():
                blob = dm.blobs_of(oracle, [b"k"], [b"a-value-no-prior-has"], None, [attrs])[0]
                for pts in tm.PTS:
                    rel = fm.diff_model(*rm.join([blob]), *rm.join(fm.table_blobs(oracle, table)), times=(pts, NOW))[0]
                    wrote = dm.replay([blob], table, pts) != table      # the new element differs from every prior
                    assert bool(rel[0] & APPLY) == wrote, (akind, bkind, pts)
                    assert bool(rel[0] & FOUND) == (bkind != "absent")
                    n += 1
                    applied += wrote
    assert n == 600 and 100 < applied < 500


def _random_feed(oracle, seed, n=10):
    rng = np.random.default_rng(seed)
    kinds = list(tm.ATTRS_KINDS)
    keys = [b"key-%d" % int(k) for k in rng.integers(0, 3, n)]
    vals = [b"" if rng.random() < 0.15 else b"v%d" % int(rng.integers(0, 3)) for _ in range(n)]
    attrs = [tm.ATTRS_KINDS[kinds[int(rng.integers(0, len(kinds)))]] for _ in range(n)]
    table = {}
    for k in range(3):
        states = tm.prior_states(_ident(oracle, b"key-%d" % k))
        table.update(states[list(states)[int(rng.integers(0, len(states)))]])
    return dm.blobs_of(oracle, keys, vals, None, attrs), table, tm.PTS[int(rng.integers(0, len(tm.PTS)))]


CONTROL_SEED = 67  # a stream for which the per-blob verdict applied to REPEAT blobs leaves another table


def test_fed_blobs_replay_to_the_same_table_with_repeats(oracle):
    """Random streams over 3 keys with repeats; and the control: the policy that applies the
    per-blob verdict to REPEAT blobs too leaves another table for some of these streams."""
    control_differs, seeds, skipped = 0, [], 0
    with tm.real_attrs(NOW):
        for seed in range(200):
            a, table, pts = _random_feed(oracle, seed)
            whole, fed, feed = _feed_tables(oracle, a, table, pts)
            assert fed == whole, seed
            skipped += len(a) - int(feed.sum())
            _w, control, _f = _feed_tables(oracle, a, table, pts, repeat_always=False)
            if control != whole:
                control_differs += 1
                seeds.append(seed)
        # an A whose first blob is applied and is itself expired: the second is refused against
        # B's live element, yet overwrites the expired one the first left
        ident = _ident(oracle, b"k")
        table = tm.prior_states(ident)["m900"]
        a = dm.blobs_of(oracle, [b"k", b"k"], [b"v1", b"v2"], None,
                        [tm.ATTRS_KINDS["m950-expired"], tm.ATTRS_KINDS["none"]])
        whole, fed, _f = _feed_tables(oracle, a, table, (2000, 0))
        _w, control, _f = _feed_tables(oracle, a, table, (2000, 0), repeat_always=False)
        assert fed == whole and control != whole and whole[ident] == (b"v2", None, None)
    assert control_differs > 0 and CONTROL_SEED in seeds, seeds[:10]
    assert skipped > 0


def _host_stream(oracle, seed):
    buf, off = rm.stream_of(oracle, rm.records(oracle, 4, seed=seed))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64)


def test_diff_argument_validation(oracle):
    """Judged on the host before any device is touched: the same answers with and without a
    GPU, each with its own message."""
    lib = _native.batch_lib()
    (a, aoff), (b, boff) = _host_stream(oracle, 1), _host_stream(oracle, 2)
    na, nb = aoff.size - 1, boff.size - 1
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    rel = np.full(na, 0xEE, np.uint8)
    counts = (ctypes.c_uint64 * 4)(7, 7, 7, 7)
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    diff = lib.k2h_amd_ralledata_diff
    msg = lambda: bytes(lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL))  # noqa: E731

    def args(**kw):
        d = dict(a=p(a), a_size=a.size, a_off=p(aoff), na=na, b=p(b), b_size=b.size, b_off=p(boff), nb=nb, rel=p(rel))
        d.update(kw)
        return (d["a"], d["a_size"], d["a_off"], d["na"], None, d["b"], d["b_size"], d["b_off"], d["nb"], None, None,
                d["rel"], None, None, cp, None)
    # nothing arrives: OK, counts zeroed, whatever B is
    assert diff(*args(a=None, a_off=None, na=0, rel=None)) == _native.K2H_AMD_OK
    assert list(counts) == [0, 0, 0, 0]
    assert diff(None, 0, None, 0, None, None, 0, None, 0, None, None, None, None, None, None, None) == _native.K2H_AMD_OK
    texts = set()
    for kw, text in ((dict(rel=None), b"NULL rel"), (dict(a=None), b"NULL a_blobs"), (dict(a_off=None), b"NULL a_off"),
                     (dict(b=None), b"NULL b_blobs"), (dict(b_off=None), b"NULL b_off"),
                     (dict(nb=(1 << 32) - 1 - na), b"2^32 - 2"), (dict(na=1 << 40), b"2^32 - 2"),
                     (dict(na=(1 << 64) - 1, nb=2), b"2^32 - 2"), (dict(na=0, a=None, a_off=None, b=None), b"NULL b_blobs")):
        for i in range(4):
            counts[i] = 7
        assert diff(*args(**kw)) == _native.K2H_AMD_EINVAL, kw
        assert text in msg() and msg().startswith(b"ralledata_diff: "), (kw, msg())
        assert list(counts) == [0, 0, 0, 0]
        texts.add(msg())
    assert len(texts) == 6
    assert (rel == 0xEE).all()


def test_diff_public_names():
    import inspect

    import k2hash_amd
    assert hasattr(k2hash_amd, "diff_ralledata") and "diff_ralledata" in k2hash_amd.__all__
    assert len(_native.SIGNATURES["k2h_amd_ralledata_diff"][1]) == 16
    assert ralledata.NO_MATCH == NONE
    assert (ralledata.DIFF_PART, ralledata.DIFF_FOUND, ralledata.DIFF_VAL, ralledata.DIFF_SKEY, ralledata.DIFF_ATTRS,
            ralledata.DIFF_DATA, ralledata.DIFF_REPEAT, ralledata.DIFF_APPLY) == (PART, FOUND, VAL, SKEY, ATTRS, DATA,
                                                                                  REPEAT, APPLY)
    header = (rm.ROOT / "include" / "k2hash_amd.h").read_text()
    for name, bit in (("PART", PART), ("FOUND", FOUND), ("VAL", VAL), ("SKEY", SKEY), ("ATTRS", ATTRS),
                      ("DATA", DATA), ("REPEAT", REPEAT), ("APPLY", APPLY)):
        assert f"#define K2H_AMD_DIFF_{name} 0x{bit:02x}u" in header
    sig = inspect.signature(ralledata.diff_ralledata).parameters
    assert list(sig)[:4] == ["a_blobs", "a_off", "b_blobs", "b_off"] and sig["count"].default is True
    assert ralledata.Diff._fields == ("rel", "match", "seen", "participants", "found", "same", "apply", "feed")
    assert fm.RESOLVE_BLOCK % 64 == 0 and 64 < fm.RESOLVE_BLOCK < 300 and fm.WAVE_BYTES > 65


# ---- the streams of the GPU tests, and (CPU) that each is what its test claims
SEG_LENS = sorted({0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, fm.WAVE_BYTES - 1, fm.WAVE_BYTES, fm.WAVE_BYTES + 1,
                   2 * fm.WAVE_STEP + 5})


def differing_places(L):
    """The first byte, the last byte, and each side of the first and last 16-byte chunk boundary,
    for chunks counted from the segment's start and for chunks that end at its last byte."""
    edges = {16, (L - 1) // 16 * 16, L - 16, L - (L - 1) // 16 * 16}
    places = {0, L - 1} | {e + d for e in edges for d in (-1, 0)}
    return sorted(x for x in places if 0 <= x < L)


def _segment_pairs(oracle):
    """(A blob, B blob, the bits expected beyond PART | FOUND | DATA) for every segment, length
    and place; both blobs rebuilt so that their segments sit at unrelated positions with slack,
    the filler around every segment different in A and in B."""
    rng = np.random.default_rng(77)
    cases = []
    for s in (1, 2, 3):
        for L in SEG_LENS:
            for at in [None] + differing_places(L):
                cases.append((s, L, at, False))
    for s in (1, 2, 3):                  # and with the other two segments present and equal
        for L in (17, fm.WAVE_BYTES - 20, fm.WAVE_BYTES + 1):
            for at in (None, 0, L - 1):
                cases.append((s, L, at, True))
    base = dm.blobs_of(oracle, [b"segment-pair-%04d" % c for c in range(len(cases))], [b"x"] * len(cases))
    a, b, bits = [], [], []
    for c, (s, L, at, others) in enumerate(cases):
        segs = [segments(base[c])[0], b"", b"", b""]
        for o in (1, 2, 3):
            if o == s:
                segs[o] = bytes(rng.integers(0, 256, L, dtype=np.uint8))
            elif others:
                segs[o] = bytes(rng.integers(0, 256, 9 + 4 * o, dtype=np.uint8))
        f = fields(base[c])
        b.append(layout(f[0], f[1], segs, order=(0, 1, 2, 3), slack=1 + c % 5, filler=0x11))
        if at is not None:
            d = bytearray(segs[s])
            d[at] ^= 1 << (c % 8)
            segs[s] = bytes(d)
        a.append(layout(f[0], f[1], segs, order=(3, 1, 0, 2), slack=8 + (c // 5) % 7, filler=0xEE))
        bits.append(0 if at is None else (VAL, SKEY, ATTRS)[s - 1])
    return a, b, bits


def test_segment_pairs_are_what_they_claim(oracle):
    a, b, bits = _segment_pairs(oracle)
    rel, match, seen, counts = fm.diff_model(*rm.join(a), *rm.join(b))
    assert (match == np.arange(len(a))).all() and seen.all()
    for i in range(len(a)):
        data = DATA if any(fields(a[i])[3:6]) else 0
        assert rel[i] == PART | FOUND | data | bits[i], i
        fa, fb = fields(a[i]), fields(b[i])
        for s in (1, 2, 3):              # the neighbours of every segment differ between the two blobs
            if fa[2 + s]:
                assert a[i][fa[6 + s] - 1] != b[i][fb[6 + s] - 1] or fa[6 + s] == 80
                assert a[i][fa[6 + s] + fa[2 + s]] != b[i][fb[6 + s] + fb[2 + s]]
                assert fa[6 + s] != fb[6 + s]
    assert counts[2] == bits.count(0) and 0 < counts[2] < len(a)
    assert {fields(x)[3] for x in a} >= set(SEG_LENS)


def _identity_streams(oracle):
    """(A blobs, B blobs): the identity cases of the GPU test, all in one pair of streams."""
    a, b = [], []
    mk = lambda key, val, n=1: dm.blobs_of(oracle, [key] * n, [val + b"%d" % i for i in range(n)])  # noqa: E731
    # same stored hash, different key (same length, another last byte; and another length)
    x, y, z = mk(b"collide-A", b"v")[0], mk(b"collide-B", b"v")[0], mk(b"collide-A-longer", b"v")[0]
    for blob in (y, z):
        dm.set_hash(blob, rm.get(x, 0, rm.F_HASH), rm.get(x, 0, rm.F_SUBHASH))
    a += [x]
    b += [y, z]
    # same hash and key, different subhash
    x, y = mk(b"sub-key", b"v")[0], mk(b"sub-key", b"v")[0]
    dm.set_hash(y, sub=rm.get(y, 0, rm.F_SUBHASH) ^ 1)
    a += [x]
    b += [y]
    # different hashes that agree in all sorted low bits: in A, in B and in both
    for k, (in_a, in_b) in enumerate(((True, False), (False, True), (True, True))):
        x, y = mk(b"low-bits-%d" % k, b"same")[0], mk(b"low-bits-%d" % k, b"same")[0]
        h = rm.get(x, 0, rm.F_HASH)
        hi = [dm.set_hash(bytearray(x), h ^ (1 << 63)), dm.set_hash(bytearray(x), h ^ (1 << 50))]
        a += [x] + (hi if in_a else [])
        b += (hi[::-1] if in_b else []) + [y]
    # B with three blobs of one identity: the last is matched
    a += mk(b"thrice", b"v2")
    b += mk(b"thrice", b"v", 3)
    # plain matches and misses around them
    a += mk(b"only-in-A", b"v") + mk(b"in-both", b"v")
    b += mk(b"in-both", b"v") + mk(b"only-in-B", b"v")
    return a, b


def _plant(blobs, rng_seed):
    """The blobs with one non-participant of each kind planted among them, each a copy of a
    participant (so it shares a stored hash and key); returns blobs, consider."""
    out = [bytearray(x) for x in blobs]
    src = bytearray(out[len(out) // 2])
    bad_span = src[:79]
    empty = bytearray(src)
    for f in (rm.F_KLEN, rm.F_VLEN, rm.F_SLEN, rm.F_ALEN):
        rm.put(empty, 0, f, 0)
    no_key = bytearray(src)
    rm.put(no_key, 0, rm.F_KLEN, 0)
    bad_range = bytearray(src)
    rm.put(bad_range, 0, rm.F_KPOS, 79)
    planted = [bad_span, empty, no_key, bad_range, bytearray(src)]     # the last: consider 0
    order = np.random.default_rng(rng_seed).permutation(len(out) + len(planted))
    both = out + planted
    consider = np.ones(len(both), np.uint8)
    consider[len(both) - 1] = 0
    return [both[i] for i in order], consider[order]


def test_identity_streams_model(oracle):
    a, b = _identity_streams(oracle)
    rel, match, seen, counts = fm.diff_model(*rm.join(a), *rm.join(b))
    assert rel[0] == PART | DATA and rel[1] == PART | DATA            # hash collides, key or subhash differs
    thrice = [j for j, x in enumerate(b) if segments(x)[0] == b"thrice"]
    at = [i for i, x in enumerate(a) if segments(x)[0] == b"thrice"][0]
    assert match[at] == thrice[2] and seen[thrice].tolist() == [0, 0, 1] and rel[at] & VAL
    assert counts[0] == len(a) and 0 < counts[1] < len(a)
    pa, ca = _plant(a, 1)
    rel, match, _seen, counts = fm.diff_model(*rm.join(pa), *rm.join(b), a_consider=ca)
    assert counts[0] == len(a) and (rel == 0).sum() == 5 and (match[rel == 0] == NONE).all()


def _run_stream(oracle, r):
    """A with r copies of one key (values differ) among other keys, B holding the key or not."""
    a = dm.blobs_of(oracle, [b"others-%d" % i for i in range(5)] + [b"the-run-key"] * r,
                    [b"v%d" % i for i in range(5 + r)])
    order = np.random.default_rng(r).permutation(len(a))
    return [a[i] for i in order]


# ------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_reference_fixture(cuda, golden):
    b = rm.join(golden)
    fm.against_model(cuda, b, b, "fixture against itself")
    a, _want = _mutated_fixture(golden)
    rel, _m, _s, counts = fm.against_model(cuda, rm.join(a), b, "mutated fixture", shifts=(0, 5))
    assert counts[2] < counts[1] == 48
    fm.against_model(cuda, rm.join(a), b, "mutated fixture, times", times=((2000, 0), NOW), shifts=(8, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("shifts", [(0, 7), (1, 0), (2, 9), (3, 3), (4, 13), (5, 10), (6, 15), (8, 11), (12, 14)])
def test_segment_compare(cuda, oracle, shifts):
    """Shifts 0 .. 15 between the two streams across the cases; (6, 15) and (1, 0) end with the
    tensor."""
    a, b, bits = _segment_pairs(oracle)
    tail = 0 if shifts in ((6, 15), (1, 0)) else tm.PAD
    rel, _match, _seen, counts = fm.against_model(cuda, rm.join(a), rm.join(b), f"segments at {shifts}", shifts=shifts,
                                                  tail_pad=tail)
    assert counts[2] == bits.count(0)
    # and with the roles swapped: B's layout incoming, A's held
    fm.against_model(cuda, rm.join(b), rm.join(a), f"segments at {shifts}, swapped", shifts=shifts, tail_pad=tail)


def test_segment_compare_shifts_cover_all():
    sh = [(0, 7), (1, 0), (2, 9), (3, 3), (4, 13), (5, 10), (6, 15), (8, 11), (12, 14)]
    assert {x for pair in sh for x in pair} == set(range(16))


@pytest.mark.gpu
def test_identity(cuda, oracle):
    a, b = _identity_streams(oracle)
    fm.against_model(cuda, rm.join(a), rm.join(b), "identity")
    fm.against_model(cuda, rm.join(dm.at_odd_offsets(a, 1)), rm.join(dm.at_odd_offsets(b, 2)), "identity, odd offsets",
                     shifts=(9, 2), tail_pad=0)
    pa, ca = _plant(a, 1)
    pb, cb = _plant(b, 2)
    model = fm.against_model(cuda, rm.join(pa), rm.join(pb), "non-participants in both", a_consider=ca, b_consider=cb,
                             shifts=(5, 6))
    assert (model[0] == 0).sum() == 5
    # outputs that may be NULL are
    fm.against_model(cuda, rm.join(pa), rm.join(pb), "NULL match, seen, counts", a_consider=ca, b_consider=cb,
                     want=(False, False, False))


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 2, 300])
def test_repeat_runs(cuda, oracle, r):
    a = _run_stream(oracle, r)
    held = dm.blobs_of(oracle, [b"unrelated", b"the-run-key", b"others-3"], [b"v", b"held", b"v3"])
    for what, b in (("held", held), ("not held", held[:1])):
        rel, match, seen, counts = fm.against_model(cuda, rm.join(a), rm.join(b), f"run of {r}, {what}",
                                                    times=((2000, 0), NOW))
        assert ((rel & REPEAT) != 0).sum() == (r if r > 1 else 0)
        assert counts[1] == (r + 1 if what == "held" else 0)


@pytest.mark.gpu
def test_hot_key(cuda, oracle):
    """65,536 copies of one key in A against a B that holds it, and against one that does not."""
    two = dm.blobs_of(oracle, [b"hot-key"] * 2 + [b"cold"], [b"held-value", b"other-value", b"c"])
    a = rm.join([two[i & 1] for i in range(65536)] + [two[2]])
    for what, b in (("held", [two[2], two[0]]), ("not held", [two[2]])):
        rel, match, seen, counts = fm.against_model(cuda, a, rm.join(b), f"hot key, {what}")
        assert counts[0] == 65537 and counts[1] == (65537 if what == "held" else 1)
        assert counts[2] == (32769 if what == "held" else 1)


@pytest.mark.gpu
def test_sizes(cuda, oracle):
    pool = dm.blobs_of(oracle, [b"size-key-%03d" % i for i in range(300)], [b"v%d" % (i % 7) for i in range(300)])
    changed = [with_segment(x, 1, b"changed") if i % 3 == 0 else x for i, x in enumerate(pool)]
    for na in (1, 255, 256, 257):
        for nb in (0, 1, 255, 256, 257):
            a, b = rm.join(changed[40:40 + na]), rm.join(pool[:nb])
            _rel, _match, _seen, counts = fm.against_model(cuda, a, b, f"na {na}, nb {nb}", shifts=(na % 16, nb % 16))
            assert counts[1] == max(0, min(40 + na, nb) - 40)


def _times_streams(oracle):
    """Every pair of an A attrs kind and a held element's kind, on distinct keys."""
    a_keys, a_vals, a_attrs, table = [], [], [], {}
    for c, (akind, bkind) in enumerate((x, y) for x in tm.ATTRS_KINDS for y in tm.prior_states(None)):
        key = b"times-%04d" % c
        a_keys.append(key)
        a_vals.append(b"" if c % 7 == 3 else b"prior-value" if c % 3 == 0 else b"new-value")
        a_attrs.append(tm.ATTRS_KINDS[akind])
        table.update(tm.prior_states(_ident(oracle, key))[bkind])
    return dm.blobs_of(oracle, a_keys, a_vals, None, a_attrs), fm.table_blobs(oracle, table)


def test_times_streams_cover_the_table(oracle):
    a, b = _times_streams(oracle)
    assert len(a) == 120 and len(b) == 110
    seen_apply = set()
    for pts in tm.PTS:
        rel = fm.diff_model(*rm.join(a), *rm.join(b), times=(pts, NOW))[0]
        seen_apply |= {(bool(r & FOUND), bool(r & APPLY)) for r in rel}
    assert seen_apply == {(False, True), (True, True), (True, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("pts", tm.PTS)
def test_times(cuda, oracle, pts):
    a, b = _times_streams(oracle)
    fm.against_model(cuda, rm.join(dm.at_odd_offsets(a, 4)), rm.join(dm.at_odd_offsets(b, 5)), f"times, pts {pts}",
                     times=(pts, NOW), shifts=(7, 2))


@pytest.mark.gpu
def test_wrapper_feed_replays_to_the_same_table(cuda, oracle):
    """diff_ralledata(...).feed -> select_ralledata -> the kept blobs, copied back and replayed
    on the host, leave the table that all of A leaves."""
    import torch
    a, b = _times_streams(oracle)
    extra, _t, _p = _random_feed(oracle, CONTROL_SEED, n=12)       # repeats of three more keys, none of them held
    a = a + extra
    pts = (1000, 500)
    table = {}
    for blob in b:
        f, s = fields(blob), segments(blob)
        table[(f[0], f[1], s[0])] = tuple(x if x else None for x in s[1:])
    (a_buf, a_off), (b_buf, b_off) = rm.join(a), rm.join(b)
    dev = lambda buf: torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(cuda)  # noqa: E731
    offs = lambda o: torch.tensor(o, dtype=torch.int64, device=cuda)  # noqa: E731
    ta, tb, da, db = dev(a_buf), dev(b_buf), offs(a_off), offs(b_off)
    d = ralledata.diff_ralledata(ta, da, tb, db, pts=pts, now=NOW, want_match=True, want_seen=True)
    rel, match, seen, counts = fm.diff_model(a_buf, a_off, b_buf, b_off, times=(pts, NOW))
    assert (d.rel.cpu().numpy() == rel).all() and (d.match.cpu().numpy().view(np.uint64) == match).all()
    assert (d.seen.cpu().numpy() == seen).all() and [d.participants, d.found, d.same, d.apply] == counts
    feed = d.feed.cpu().numpy()
    assert (feed == fm.feed_of(rel)).all() and 0 < feed.sum() < len(a)
    sel = ralledata.select_ralledata(ta, da, d.feed)
    torch.cuda.synchronize()
    out, ooff = sel.blobs.cpu().numpy().tobytes(), sel.blob_off.cpu().numpy()
    kept = [out[int(ooff[i]):int(ooff[i + 1])] for i in range(sel.kept)]
    assert sel.kept == int(feed.sum())
    with tm.real_attrs(NOW):
        assert dm.replay(kept, table, pts) == dm.replay(a, table, pts)
    # without times: no feed, no APPLY; asynchronous without counts
    plain = ralledata.diff_ralledata(ta, da, tb, db, count=False)
    torch.cuda.synchronize()
    assert plain.feed is None and plain.match is None and plain.seen is None and plain.found is None
    assert (plain.rel.cpu().numpy() == rel & ~np.uint8(APPLY)).all()
    with pytest.raises(ValueError):
        ralledata.diff_ralledata(ta, da, tb, db, pts=pts)
