"""Which held blob decides APPLY (k2h_amd_ralledata_diff with times; k2h_ralledata_diff.hip's
resolve walk) where B holds more than one blob that the walk meets for an incoming blob.

APPLY (lib/k2hshmdirect.cc:380-431) is the one output that depends on the side record and the
mtime of the held entry the resolve lane ends up with, not only on that entry's index.  The
streams here are deterministic and every key is planted for one reason:

* held: every (earlier kind, last kind, incoming kind), the two copies of a key apart in B;
* stepover: a later blob of B that shares the true match's stored hash (or only its sorted low
  bits) without sharing its identity, carrying a kind whose verdict differs; and on the A side a
  neighbour of the incoming blob's stored hash with another mtime;
* broken: the would-be last copy takes no part (masked, bad span, no key, key range outside,
  wrong stored hash), so the earlier copy decides; the same breakages on the A side;
* sizes: test_ralledata_diff.test_sizes' grid with times and every kind of attrs, larger calls
  before smaller ones.

Keys run from 9 to 60 bytes in every stream, one to four 16-byte chunks of same_key: a build
that lost the matched blob's side record for keys of more than one chunk passed every
deterministic test while all their keys were short.

The CPU tests state why a device test on these streams cannot pass for the wrong reason: the
model's choice is the rule, and the blob the walk must not choose would have given another
answer.  Expected values come from ralle_diff_model.diff_model and would_apply only.
"""
import itertools

import numpy as np
import pytest

import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_diff_model as fm
import ralle_times_model as tm
from ralle_diff_model import APPLY, DATA, FOUND, NONE, PART, REPEAT

NOW = tm.NOW
INC = tm.ATTRS_KINDS                                                       # 10 incoming kinds
HELD = {k: (list(t.values())[0][2] or b"") for k, t in tm.prior_states(None).items() if k != "absent"}   # 11 held kinds
PTS_TWO = ((950, 0), (2000, 0))
BREAKS = ("masked", "bad-span", "no-key", "bad-range", "wrong-hash")
_CACHE = {}


def verdict(g, h, pts):
    return fm.would_apply(INC[g], HELD[h], pts, NOW)


def differing(pts_list=tm.PTS):
    """{(x, y): [(g, pts), ...]}: the ordered pairs of held kinds whose verdicts differ, and where."""
    out = {}
    for x, y in itertools.permutations(HELD, 2):
        where = [(g, pts) for g in INC for pts in pts_list if verdict(g, x, pts) != verdict(g, y, pts)]
        if where:
            out[(x, y)] = where
    return out


def best_incoming(where):
    """The incoming kind that tells the pair apart at the most pts (the first such)."""
    return max(INC, key=lambda g: sum(1 for gg, _p in where if gg == g))


def key_of(prefix, c):
    """Keys of 1 to 4 16-byte chunks (same_key compares the first chunk apart from the rest), the
    length running against the kinds' cycles of 10 and 11."""
    return prefix + b"-%04d" % c + b"k" * (c % 41)


def chunks(blob):
    return (rm.get(blob, 0, rm.F_KLEN) + 15) // 16


def attrs_of(blob):
    f = np.frombuffer(bytes(blob[:rm.HEADER]), "<u8")
    return bytes(blob[int(f[9]):int(f[9]) + int(f[5])]) if f[5] else b""


def cached(oracle, build):
    if build.__name__ not in _CACHE:
        _CACHE[build.__name__] = build(oracle)
    return _CACHE[build.__name__]


def broken(blob, how):
    """A copy of `blob` that takes no part, or (wrong-hash) takes part under another identity."""
    x = bytearray(blob)
    if how == "bad-span":
        return x[:79]
    if how == "no-key":
        rm.put(x, 0, rm.F_KLEN, 0)
    elif how == "bad-range":
        rm.put(x, 0, rm.F_KPOS, 79)
    elif how == "wrong-hash":
        rm.put(x, 0, rm.F_HASH, rm.get(x, 0, rm.F_HASH) ^ 0x10)
    return x                                                               # masked: by its consider byte


# ------------------------------------------------------------- 1. earlier copy and last copy
def _held_streams(oracle):
    """(A blobs, B blobs, info): key c has the kinds info[c] = (earlier, last, incoming, slot of
    the earlier copy in B, slot of the last).  Key c's copies sit in slots 2c and
    2((c + 7) mod n) + 1, the lower slot the earlier copy's: never neighbours."""
    combos = list(itertools.product(HELD, HELD, INC))
    n = len(combos)
    keys = [key_of(b"held", c) for c in range(n)]
    a_vals = [b"" if c % 7 == 3 else (b"prior-value", b"earlier-value", b"new-value")[c % 3] for c in range(n)]
    b_keys, b_vals, b_attrs, info = [None] * 2 * n, [None] * 2 * n, [None] * 2 * n, []
    for c, (e, l, g) in enumerate(combos):
        se, sl = sorted((2 * c, 2 * ((c + 7) % n) + 1))
        b_keys[se], b_vals[se], b_attrs[se] = keys[c], b"earlier-value", HELD[e]
        b_keys[sl], b_vals[sl], b_attrs[sl] = keys[c], b"prior-value", HELD[l]
        info.append((e, l, g, se, sl))
    a = dm.blobs_of(oracle, keys, a_vals, None, [INC[g] for _e, _l, g in combos])
    return a, dm.blobs_of(oracle, b_keys, b_vals, None, b_attrs), info


def test_held_model_choice_is_the_rule(oracle):
    """diff_model over B gives the rel it gives over B without the earlier copies, the same match
    after index remapping, and both are would_apply(incoming, last) on the blobs' own attrs."""
    a, b, info = cached(oracle, _held_streams)
    assert len(a) == 1210 and len(b) == 2420 and all(abs(se - sl) > 1 and se < sl for *_k, se, sl in info)
    kept = np.array(sorted(sl for *_k, sl in info))
    ja, jb, jl = rm.join(a), rm.join(b), rm.join([b[j] for j in kept])
    for pts in tm.PTS:
        rel, match, seen, _c = fm.diff_model(*ja, *jb, times=(pts, NOW))
        rel_l, match_l, seen_l, _c = fm.diff_model(*ja, *jl, times=(pts, NOW))
        assert (rel == rel_l).all() and seen_l.all() and (match == kept[match_l.astype(np.int64)]).all()
        for c, (_e, _l, _g, se, sl) in enumerate(info):
            assert match[c] == sl and seen[sl] == 1 and seen[se] == 0
            assert bool(rel[c] & APPLY) == fm.would_apply(attrs_of(a[c]), attrs_of(b[sl]), pts, NOW), (c, pts)
            assert attrs_of(a[c]) == INC[_g] and attrs_of(b[sl]) == HELD[_l] and attrs_of(b[se]) == HELD[_e]


def test_held_earlier_copy_would_answer_otherwise(oracle):
    """The keys whose earlier copy gives another verdict than their last copy, counted on the
    stream's own blobs: 2,904 of the 6,050 (key, pts) cases,
        pts (800, 0): 600, (950, 0): 600, (950, 1): 576, (1000, 500): 564, (2000, 0): 564
    of 1,210 keys each, and 86 of the 121 ordered kind pairs for some incoming kind and pts.
    Every ordered pair that the kinds' table says can differ is present in the stream, and no pts
    has fewer than a quarter of its keys in this class."""
    a, b, info = cached(oracle, _held_streams)
    per_pts, pairs = {}, set()
    for pts in tm.PTS:
        n, lengths = 0, set()
        for c, (e, l, _g, se, sl) in enumerate(info):
            if fm.would_apply(attrs_of(a[c]), attrs_of(b[se]), pts, NOW) != \
                    fm.would_apply(attrs_of(a[c]), attrs_of(b[sl]), pts, NOW):
                n += 1
                pairs.add((e, l))
                lengths.add(chunks(a[c]))
        per_pts[pts] = n
        assert lengths == {1, 2, 3, 4}, pts                                # keys of every number of chunks among them
    assert pairs == set(differing()) and len(pairs) == 86
    assert sum(per_pts.values()) == 2904 and all(4 * n >= len(info) for n in per_pts.values()), per_pts
    assert per_pts == {(800, 0): 600, (950, 0): 600, (950, 1): 576, (1000, 500): 564, (2000, 0): 564}


@pytest.mark.gpu
@pytest.mark.parametrize("pts", tm.PTS)
def test_held_last_copy_decides(cuda, oracle, pts):
    a, b, _info = cached(oracle, _held_streams)
    fm.against_model(cuda, rm.join(dm.at_odd_offsets(a, 6)), rm.join(dm.at_odd_offsets(b, 7)),
                     f"earlier and last copy, pts {pts}", times=(pts, NOW), shifts=(5, 12))


# ------------------------------------------------------------------ 2. the step-over path
VARIANTS = ("other-subhash", "other-key", "other-key-length", "other-high-bit")


def _stepover_streams(oracle):
    """(A blobs, B blobs, info): for every ordered pair of held kinds (x, y) that some incoming
    kind g tells apart, and every variant, B holds the true match X (kind x) and LATER a blob of
    kind y that shares X's stored hash -- for the last variant only its sorted low bits -- but not
    its identity.  A holds the incoming blob (kind g) and next to it, before or behind, a blob of
    its key and hash under another subhash with kind g2.  info[c] = (x, y, g, g2, index of the
    incoming blob in A, of its neighbour, slot of X in B, slot of the later blob)."""
    cases = [(x, y, best_incoming(where), v) for (x, y), where in differing().items() for v in range(len(VARIANTS))]
    n = len(cases)
    keys = [key_of(b"step", c) for c in range(n)]
    xs = dm.blobs_of(oracle, keys, [b"prior-value"] * n, None, [HELD[x] for x, _y, _g, _v in cases])
    other = [k[:-1] + b"~" if v == 1 else k + b"-longer" if v == 2 else k for k, (_x, _y, _g, v) in zip(keys, cases)]
    later = dm.blobs_of(oracle, other, [b"stepped-value" if c % 2 else b"prior-value" for c in range(n)], None,
                        [HELD[y] for _x, y, _g, _v in cases])
    for c, (_x, _y, _g, v) in enumerate(cases):
        h, s = rm.get(xs[c], 0, rm.F_HASH), rm.get(xs[c], 0, rm.F_SUBHASH)
        dm.set_hash(later[c], h ^ (1 << 63) if v == 3 else h, s ^ 1 if v == 0 else s)
    slot = [n + (c + 37) % n for c in range(n)]                            # every later blob behind every X
    b = xs + [later[(k - 37) % n] for k in range(n)]
    a_keys, a_attrs, g2s = [], [], []
    for c, (x, _y, g, _v) in enumerate(cases):
        tells = [k for k in INC if any(verdict(k, x, p) != verdict(g, x, p) for p in tm.PTS)]
        g2 = tells[c % len(tells)] if tells else [k for k in INC if k != g][c % 9]
        g2s.append(g2)
        a_keys += [keys[c]] * 2
        a_attrs += [INC[g2], INC[g]] if c % 2 else [INC[g], INC[g2]]
    a = dm.blobs_of(oracle, a_keys, [b"prior-value" if i % 3 else b"new-value" for i in range(2 * n)], None, a_attrs)
    info = []
    for c, (x, y, g, _v) in enumerate(cases):
        own, nb = (2 * c + 1, 2 * c) if c % 2 else (2 * c, 2 * c + 1)
        dm.set_hash(a[nb], sub=rm.get(a[nb], 0, rm.F_SUBHASH) ^ 2)
        info.append((x, y, g, g2s[c], own, nb, c, slot[c]))
    return a, b, info


def test_stepover_substituted_attrs_answer_otherwise(oracle):
    """For EVERY planted case: the model matches X and reports would_apply(incoming, X), and at
    some pts that is not what the later blob's attrs would give.  On the A side the incoming
    blob's APPLY is its own although its neighbour shares its hash (REPEAT on both); wherever two
    incoming kinds can differ against X at all, the planted neighbour's kind does."""
    a, b, info = cached(oracle, _stepover_streams)
    assert len(info) == 4 * 86 and all(sx < sy for *_k, sx, sy in info)
    ja, jb = rm.join(a), rm.join(b)
    told = [False] * len(info)
    for pts in tm.PTS:
        rel, match, seen, _c = fm.diff_model(*ja, *jb, times=(pts, NOW))
        for c, (x, y, g, g2, own, nb, sx, sy) in enumerate(info):
            assert match[own] == sx and seen[sx] == 1 and seen[sy] == 0 and match[nb] == NONE
            assert attrs_of(a[own]) == INC[g] and attrs_of(b[sx]) == HELD[x] and attrs_of(b[sy]) == HELD[y]
            assert bool(rel[own] & APPLY) == verdict(g, x, pts)
            assert rel[own] & REPEAT and rel[nb] == PART | DATA | REPEAT | APPLY
            told[c] |= verdict(g, x, pts) != fm.would_apply(attrs_of(a[own]), attrs_of(b[sy]), pts, NOW)
    assert all(told)
    for v in range(len(VARIANTS)):
        assert {chunks(a[i[4]]) for i in info[v::4]} == {1, 2, 3, 4}, VARIANTS[v]
    for x in HELD:
        can = any(verdict(g, x, p) != verdict(k, x, p) for g in INC for k in INC for p in tm.PTS)
        mine = [i for i in info if i[0] == x]
        does = [any(verdict(i[2], x, p) != verdict(i[3], x, p) for p in tm.PTS) for i in mine]
        assert mine and all(does) == can and any(does) == can, x


@pytest.mark.gpu
@pytest.mark.parametrize("pts", tm.PTS)
def test_stepover_match_keeps_its_own_attrs(cuda, oracle, pts):
    a, b, _info = cached(oracle, _stepover_streams)
    fm.against_model(cuda, rm.join(dm.at_odd_offsets(a, 8)), rm.join(dm.at_odd_offsets(b, 9)),
                     f"later blobs of the match's hash, pts {pts}", times=(pts, NOW), shifts=(13, 6))


# ------------------------------------------- 3. non-participants as the would-be last copy
def _broken_streams(oracle):
    """(A blobs, a_consider, B blobs, b_consider, info, dead).  Key c of info: B holds the earlier
    copy (kind x) and behind it the would-be last copy (kind y) broken as info[c][3] says; A
    holds the incoming blob of kind g, which tells x from y at one of PTS_TWO.  dead: keys that B
    holds (one blob, every held kind) and A names only through a broken blob: (how, index in A,
    slot in B)."""
    cases = [(x, y, best_incoming(where), how) for (x, y), where in differing(PTS_TWO).items() for how in BREAKS]
    n = len(cases)
    keys = [key_of(b"broken", c) for c in range(n)]
    dead_cases = [(h, how) for h in HELD for how in BREAKS]
    dead_keys = [key_of(b"dead", c) for c in range(len(dead_cases))]
    a = dm.blobs_of(oracle, keys + dead_keys, [b"new-value" if c % 2 else b"prior-value" for c in range(n)] +
                    [b"prior-value"] * len(dead_cases), None,
                    [INC[g] for _x, _y, g, _h in cases] + [INC["m1000.500"]] * len(dead_cases))
    a = a[:n] + [broken(a[n + c], how) for c, (_h, how) in enumerate(dead_cases)]
    a_consider = np.array([1] * n + [how != "masked" for _h, how in dead_cases], np.uint8)
    first = dm.blobs_of(oracle, keys + dead_keys, [b"prior-value"] * (n + len(dead_cases)), None,
                        [HELD[x] for x, _y, _g, _h in cases] + [HELD[h] for h, _how in dead_cases])
    last = dm.blobs_of(oracle, keys, [b"prior-value"] * n, None, [HELD[y] for _x, y, _g, _h in cases])
    m = len(first)
    b = first + [broken(last[(k - 11) % n], cases[(k - 11) % n][3]) for k in range(n)]
    b_consider = np.array([1] * m + [cases[(k - 11) % n][3] != "masked" for k in range(n)], np.uint8)
    info = [(x, y, g, how, c, m + (c + 11) % n) for c, (x, y, g, how) in enumerate(cases)]
    dead = [(how, n + c, n + c) for c, (_h, how) in enumerate(dead_cases)]
    return a, a_consider, b, b_consider, info, dead


def test_broken_last_copy_leaves_the_earlier_to_decide(oracle):
    a, ca, b, cb, info, dead = cached(oracle, _broken_streams)
    assert {i[3] for i in info} == set(BREAKS) and len(info) == 5 * len(differing(PTS_TWO)) == 5 * 86
    ja, jb = rm.join(a), rm.join(b)
    told = [False] * len(info)
    for pts in PTS_TWO:
        rel, match, seen, _c = fm.diff_model(*ja, *jb, ca, cb, times=(pts, NOW))
        whole = fm.diff_model(*ja, *jb, times=(pts, NOW))                  # without the masks
        for c, (x, y, g, how, i, sl) in enumerate(info):
            assert match[i] == c and seen[c] == 1 and seen[sl] == 0 and rel[i] & FOUND
            assert bool(rel[i] & APPLY) == verdict(g, x, pts)
            told[c] |= verdict(g, x, pts) != verdict(g, y, pts)
            if how == "masked":                                            # only the mask keeps it out
                assert whole[1][i] == sl and bool(whole[0][i] & APPLY) == verdict(g, y, pts)
            elif how != "bad-span":
                assert attrs_of(b[sl]) == HELD[y]
        for how, i, j in dead:
            if how == "wrong-hash":
                assert rel[i] == PART | DATA | APPLY
            else:
                assert rel[i] == 0
            assert match[i] == NONE and seen[j] == 0
            if how == "masked":
                assert whole[1][i] == j and whole[2][j] == 1
    assert all(told)
    for how in BREAKS:
        assert {chunks(a[i[4]]) for i in info if i[3] == how} == {1, 2, 3, 4}, how


@pytest.mark.gpu
@pytest.mark.parametrize("pts", PTS_TWO)
def test_broken_last_copy(cuda, oracle, pts):
    a, ca, b, cb, _info, _dead = cached(oracle, _broken_streams)
    ja, jb = rm.join(dm.at_odd_offsets(a, 10)), rm.join(dm.at_odd_offsets(b, 11))
    model = fm.against_model(cuda, ja, jb, f"broken last copies, pts {pts}", a_consider=ca, b_consider=cb,
                             times=(pts, NOW), shifts=(9, 4))
    assert (model[0] == 0).sum() == 4 * len(HELD)
    if pts == PTS_TWO[0]:
        fm.against_model(cuda, ja, jb, "broken last copies, NULL match, seen, counts", a_consider=ca, b_consider=cb,
                         times=(pts, NOW), shifts=(2, 15), want=(False, False, False))


# ----------------------------------------------------------------- 4. sizes, with times
SIZES = sorted(itertools.product((1, 255, 256, 257), (0, 1, 255, 256, 257)), key=lambda s: -(s[0] + s[1]))


def _size_pools(oracle):
    keys = [key_of(b"size-key", i) for i in range(300)]
    held, inc = list(HELD.values()), list(INC.values())
    pool = dm.blobs_of(oracle, keys, [b"v%d" % (i % 7) for i in range(300)], None, [held[i % 11] for i in range(300)])
    incoming = dm.blobs_of(oracle, keys, [b"changed" if i % 3 == 0 else b"v%d" % (i % 7) for i in range(300)], None,
                           [inc[i % 10] for i in range(300)])
    return incoming, pool


def test_sizes_with_times_model(oracle):
    """Every later call is smaller than some earlier one, and across the grid the model shows
    matched blobs with and without APPLY and unmatched ones."""
    incoming, pool = cached(oracle, _size_pools)
    assert len(SIZES) == 20 and all(sum(SIZES[k]) <= sum(SIZES[k - 1]) for k in range(1, 20))
    assert sum(SIZES[0]) > max(sum(s) for s in SIZES[1:])
    combos = set()
    for k, (na, nb) in enumerate(SIZES):
        rel = fm.diff_model(*rm.join(incoming[40:40 + na]), *rm.join(pool[:nb]), times=(tm.PTS[k % 5], NOW))[0]
        combos |= {(na, nb, bool(r & FOUND), bool(r & APPLY)) for r in rel}
    assert {c[2:] for c in combos} == {(False, True), (True, True), (True, False)}
    edges = {(na, nb) for na in (255, 256, 257) for nb in (255, 256, 257)}
    assert {c[:2] for c in combos if c[2] and not c[3]} >= edges
    assert {chunks(x) for x in incoming[40:295]} == {1, 2, 3, 4} == {chunks(x) for x in pool[:255]}


@pytest.mark.gpu
def test_sizes_with_times(cuda, oracle):
    """The mtime column is the last of the call's grow-only scratch and the work items alias the
    key column: a smaller call after a larger one runs over the larger one's leftovers."""
    incoming, pool = cached(oracle, _size_pools)
    for k, (na, nb) in enumerate(SIZES):
        pts = tm.PTS[k % 5]
        _rel, _match, _seen, counts = fm.against_model(cuda, rm.join(incoming[40:40 + na]), rm.join(pool[:nb]),
                                                       f"na {na}, nb {nb}, pts {pts}", times=(pts, NOW),
                                                       shifts=(1 + na % 15, 1 + nb % 15))
        assert counts[1] == max(0, min(40 + na, nb) - 40)
