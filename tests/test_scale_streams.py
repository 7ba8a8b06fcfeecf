"""The streams of tests/scale_streams.py on the CPU: that the expectation each generator derives
from its columns is the pinned model's answer (at sizes where the per-blob models are quick, on both
sides of the library sort's one-block size; the same code path as at a million), that the tiled
blobs and records are the per-blob builders' bytes, that the streams hold what the GPU tests of
tests/test_sort_regimes.py and tests/test_find_regimes.py need them to hold at the size those tests
use (the queries of the find tests among them: find_expect against ralle_find_model), that this size is where
the library sort changes its algorithm, and that an expectation built on "any later copy" in place
of "the nearest" is another one, so those tests would notice an unstable sort.
"""
import numpy as np
import pytest

import archive_fold_model as af
import ralle_dedup_model as dm
import ralle_diff_model as fm
import ralle_find_model as ffm
import ralle_subkeys_model as sm
import ralle_times_model as tm
import scale_streams as ss
from scale_streams import M32, N_LARGE, N_SMALL, NONE


def first_difference(got, want, names, what):
    for name, g, w in zip(names, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has shape {g.shape}, want {w.shape}"
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, (f"{what}: {name} differs at {int(bad[0])}: constructed {g[bad[0]]}, model {w[bad[0]]} "
                               f"({bad.size} in all)")


# ------------------------------------------------------------------------- the regime claim
def test_large_and_small_sizes_fall_in_the_three_regimes():
    """The library sort's two limits as the installed rocPRIM headers give them: N_LARGE pairs take
    the Onesweep passes over 32 bits, the cross-check sizes the one-block sort and the merge sort."""
    regimes = ss.sort_regimes()
    if regimes is None:
        pytest.skip("no rocPRIM headers under " + ss.rocm_root())
    one_block, limit = regimes
    assert (one_block, limit) == (ss.ONE_BLOCK, ss.MERGE_SORT_LIMIT)
    assert limit < N_LARGE <= limit + limit // 100 and N_LARGE % 256
    assert ss.sort_bits(N_LARGE) == 32 and ss.sort_bits(limit) == 32 and af.sort_bits(N_LARGE) == 32
    assert N_SMALL[0] <= one_block < N_SMALL[1] <= limit
    # the pairs of the large tests are n, na + nb, n + E and n: N_LARGE each, the subkeys stream's from a
    # third as many blobs
    assert N_LARGE * 10 // 32 < limit // 2
    assert [ss.sort_bits(x) for x in (1, 257, 65537, 1 << 24, (1 << 24) + 1)] == [16, 24, 32, 32, 40]


# --------------------------------------------------------------- the expectation is the model's
@pytest.mark.parametrize("n", N_SMALL)
def test_dedup_expectation_is_the_model(oracle, n):
    buf, off, consider, c = ss.dedup_stream(oracle, n, seed=n)
    for cons in (consider, None):
        want = dm.dedup_model(buf, off, consider=cons)
        got = ss.dedup_expect(c, ss.participants(c, cons is not None))
        first_difference(got[:2], want[:2], ("keep", "by"), f"dedup {n}")
        assert got[2] == want[2] > n // 12
    # the attr-less part, as the mtime rule's test takes it
    cons = consider & ~c.att
    want = dm.dedup_model(buf, off, consider=cons)
    got = ss.dedup_expect(c, ss.participants(c) & ~c.att)
    first_difference(got[:2], want[:2], ("keep", "by"), f"dedup {n}, no attrs")
    assert got[2] == want[2] == int((want[1] != NONE).sum())


@pytest.mark.parametrize("n", N_SMALL)
def test_diff_expectation_is_the_model(oracle, n):
    a, b, ca, cb, c = ss.diff_streams(oracle, n, seed=n + 1)
    want = fm.diff_model(*a, *b, ca, cb)
    got = ss.diff_expect(c, ss.participants(c))
    first_difference(got[:3], want[:3], ("rel", "match", "seen"), f"diff {n}")
    assert got[3] == want[3] and want[3][1] > want[3][2] > 0


@pytest.mark.parametrize("n", N_SMALL)
def test_subkeys_and_reach_expectation_is_the_model(oracle, n):
    buf, off, consider, c = ss.subkeys_stream(oracle, n, seed=n + 2)
    assert c.n + int(c.lsize[ss.participants(c)].sum()) == n
    want = sm.edges_model(oracle, buf, off, consider=consider)
    got = ss.subkeys_expect(oracle, c, ss.participants(c))
    first_difference((got.flags, got.edge_off, got.child, got.rep), (want.flags, want.edge_off, want.child, want.rep),
                     ("sk_flags", "edge_off", "child", "rep"), f"subkeys {n}")
    assert got.counts == want.counts and want.counts[4] > 0
    roots = np.random.default_rng(n).random(c.n) < 0.02
    for max_levels in (0, 2):
        r_want = sm.reach_model(want, np.flatnonzero(roots).tolist(), max_levels)
        r_got = ss.reach_expect(got, roots, max_levels)
        first_difference(r_got[:1], r_want[:1], ("reach",), f"reach {n}")
        assert r_got[1] == r_want[1]
    assert r_want[1][0] > roots.sum()


@pytest.mark.parametrize("n", N_SMALL)
def test_fold_expectation_is_the_model(oracle, n):
    """fold_model itself over the N_LARGE log takes 11 s on the CPU this was written on (8.2 s for
    recs_of's Rec list, 2.7 s for the pass), so it is not part of the suite at that size; run there
    once by hand it gave the constructed keep, by and dropped."""
    data, recs, h1, c = ss.fold_log(oracle, n, seed=n + 3)
    want = af.fold_model(af.recs_of(bytes(data), recs))
    got = ss.fold_expect(c)
    first_difference(got[:2], want[:2], ("keep", "by"), f"fold {n}")
    assert got[2] == want[2] > n // 12


@pytest.mark.parametrize("n", N_SMALL)
def test_find_expectation_is_the_model(oracle, n):
    """Under the stored and under the true hashes, with and without consider, with `now` given."""
    buf, off, consider, c = ss.dedup_stream(oracle, n, seed=n)
    m = min(2 * n, 1500)                             # the model is a scan per query
    q = ss.find_queries(oracle, c, m, seed=n + 4)
    assert set(np.unique(q.kind)) == set(range(5)) and len(q.bytes) == q.key_off[-1]
    for name, hashes in (("stored", q.stored), ("true", q.true)):
        for cons in (consider, None):
            want = ffm.find_model(buf, off, q.bytes, q.key_off, hashes[0], hashes[1], now=tm.NOW, consider=cons)
            got = ss.find_expect(c, ss.participants(c, cons is not None), q, hashes, now=tm.NOW)
            first_difference(got[:3], want[:3], ("match", "status", "hit"), f"find {n}, {name} hashes")
            assert got[3] == want[3] and want[3][0] == m - (q.kind == ss.Q_EMPTY).sum() and want[3][1] > m // 2
    assert (ss.FIND_PART, ss.FIND_FOUND, ss.FIND_ATTRS, ss.FIND_EXPIRED) == (ffm.PART, ffm.FOUND, ffm.ATTRS, ffm.EXPIRED)


# ------------------------------------------------------- the tiled bytes are the builders' bytes
def test_tiled_blobs_are_the_builders_blobs(oracle):
    for maker in (ss.dedup_stream, ss.subkeys_stream):
        buf, off, _consider, c = maker(oracle, N_SMALL[1], seed=5)
        kinds = set()
        for i in np.flatnonzero(c.bad == 0)[:200]:
            want = ss.blob_by_builder(oracle, c, int(i))
            assert bytes(buf[off[i]:off[i] + len(want)]) == want, (maker.__name__, int(i))
            assert off[i + 1] - off[i] == len(want) + c.gap[i]
            assert (buf[off[i] + len(want):off[i + 1]] == ss.SLACK).all()
            kinds.add((int(c.klen[i]), bool(c.att[i]), int(c.lsize[i])))
        assert len(kinds) >= (4 if maker is ss.dedup_stream else 8)
        assert {(int(o) + 80) % 16 for o in off[:-1]} == set(range(16))


def test_tiled_records_are_the_builders_records(oracle):
    data, recs, _h1, c = ss.fold_log(oracle, N_SMALL[1], seed=6)
    model = af.recs_of(bytes(data), recs)
    seen = set()
    for i in np.flatnonzero(c.bad == 0)[:300]:
        want = ss._kind_record(int(c.kind[i]), bytes(c.key[i, :c.klen[i]]), bytes(c.val[i]))
        o = int(recs["offset"][i])
        assert bytes(data[o:o + len(want)]) == want and o == c.off[i], int(i)
        r = model[i]
        assert af.record_bytes(r) == want and r.type == ss.KIND_TYPE[c.kind[i]], int(i)
        seen.add(int(c.kind[i]))
    assert seen == set(range(10)) - {ss.REN} or seen == set(range(10))
    assert {int(o) % 16 for o in recs["key_off"]} == set(range(16))


# ------------------------------------------------------------ the streams are what they claim
@pytest.fixture(scope="module")
def large_columns(oracle):
    return ss.ralle_columns(oracle, N_LARGE, seed=1)


def test_large_ralle_stream_is_what_it_claims(large_columns):
    """The columns of the dedup stream at the size of the GPU tests (the diff streams are the same
    generator's under another seed, cut in two)."""
    c, n = large_columns, N_LARGE
    h = ss.ralle_holds(c, ss.participants(c))
    assert h["short_keys"] > n // 3 and h["long_keys"] > n // 3
    assert n // 6 < h["repeats"] < n // 4 and h["median_distance"] > 200_000
    assert h["three_or_more"] > 10_000 and 2_000 < h["hot"] < 5_000
    assert h["high_bits_only"] >= 1_000 and h["same_hashes_other_key"] >= 1_000 and h["other_subhash"] >= 1_000
    assert h["natural_low32"] >= 1 and 1_000 < h["low32_ones"] and h["exactly_ones"] >= 2
    assert h["exactly_ones_repeat"] >= 1
    assert n // 120 < h["non_participants"] < n // 80
    assert min(h["not_considered"], h["no_key"], h["key_past"]) > n // 400
    assert h["non_participants_with_a_live_identity"] > n // 2000
    assert n // 10 < h["attrs"] < n // 5
    # compacted positions differ from blob indices from the first non-participant on
    assert np.flatnonzero(~ss.participants(c))[0] < 1000


def test_large_diff_streams_are_what_they_claim(oracle):
    c = ss.ralle_columns(oracle, N_LARGE, seed=2)
    c.nb = N_LARGE // 2 - 3
    part = ss.participants(c)
    rel, match, seen, counts = ss.diff_expect(c, part)
    na = N_LARGE - c.nb
    assert abs(na - c.nb) < 10 and na + c.nb == N_LARGE
    found = (rel & fm.FOUND) != 0
    assert counts[0] > na * 98 // 100 and 50_000 < counts[1] < counts[0] // 2       # incoming only, and found
    assert counts[2] > 10_000 and ((rel & fm.VAL) != 0).sum() > 10_000 and ((rel & fm.ATTRS) != 0).sum() > 1_000
    assert 0 < seen.sum() < part[:c.nb].sum() - 100_000                              # held only
    assert ((rel & fm.REPEAT) != 0).sum() > 10_000
    assert (part[c.nb:] == 0).sum() > 1_000 and (part[:c.nb] == 0).sum() > 1_000
    # held identities that repeat, and the last copy decides: the first copy is another blob for thousands
    first = ss.diff_expect(c, part, later="any")
    assert (first[1] != match).sum() > 5_000 and (first[1][~found] == NONE).all()
    assert (first[0] != rel).sum() > 1_000


def test_large_subkeys_stream_is_what_it_claims(oracle):
    buf, off, consider, c = ss.subkeys_stream(oracle, N_LARGE, seed=3)
    part = ss.participants(c)
    m = ss.subkeys_expect(oracle, c, part)
    assert c.n < ss.MERGE_SORT_LIMIT // 2 and c.n + m.counts[3] == N_LARGE
    assert all(((c.lsize == k) & part).sum() > c.n // 10 for k in ss.LIST_SIZES)
    assert m.counts[4] > m.counts[3] // 40                                           # dangling, by both causes
    child_of = np.full(c.owner.size, NONE, np.uint64)
    child_of[part[c.owner]] = m.child
    assert ((child_of == NONE) & ~c.dangling & part[c.owner]).sum() > 1_000          # the target stores a wrong hash
    assert (child_of[c.dangling] == NONE).all()
    # a key three times over with different lists: groups of one identity whose list sizes differ
    idx = np.flatnonzero(part)
    order, new = ss.group_sorted(ss.ident_cols(c, idx))
    gid = np.cumsum(new) - 1
    sizes = np.bincount(gid)
    ls = c.lsize[idx[order]]
    lo, hi = np.minimum.reduceat(ls, np.flatnonzero(new)), np.maximum.reduceat(ls, np.flatnonzero(new))
    assert ((sizes >= 3) & (lo != hi)).sum() > 1_000
    roots = np.random.default_rng(4).random(c.n) < 1000 / c.n
    reach, counts = ss.reach_expect(m, roots)
    assert 900 < roots.sum() < 1100 and counts[0] > c.n // 3 and counts[1] > 8 and counts[2] == 1
    assert m.widest > 10_000                                                         # blobs of one level
    assert len(buf) < 140 << 20


def test_large_fold_log_is_what_it_claims(oracle):
    data, recs, h1, c = ss.fold_log(oracle, N_LARGE, seed=4)
    h = ss.fold_holds(c)
    assert all(k > 1_000 for k in h["kinds"][:9]) and 3 <= h["kinds"][ss.REN] <= 6 and h["segs"] >= 4
    assert all(k > 5_000 for k in h["repeated_kinds"][:9])
    assert h["hot"] > 1 << 17 and h["hot_in_one_seg"] == 1
    assert h["three_or_more"] > 10_000 and h["long_keys"] > N_LARGE // 3 and h["short_keys"] > N_LARGE // 3
    assert all(k > N_LARGE // 500 for k in h["bad"][1:])
    assert h["keys_sharing_h1"] > 1_000 and h["low32_shared"] > 1_000 and h["low32_ones"] > 1_000
    assert h["exactly_ones"] >= 2
    keep, by, dropped = ss.fold_expect(c)
    hot = c.roles["hot"][c.bad[c.roles["hot"]] == 0]
    assert keep[hot[0]] == 1 and keep[hot[-1]] == 1 and not keep[hot[1:-1]].any()    # the head waits for the chain's end
    assert dropped > N_LARGE // 5 and len(data) < 160 << 20 and h1.dtype == np.uint64
    assert (h1[c.bad == 0] != c.h_true[c.bad == 0]).sum() > 3_000


def test_large_find_queries_are_what_they_claim(oracle, large_columns):
    """What tests/test_find_regimes.py needs of its queries over the dedup stream, counted on the
    expectation (the figure behind each bound is what this seed gives)."""
    c, m = large_columns, ss.M_LARGE
    assert ss.FIND_SEEDS[0] == 1                                                     # large_columns is that stream
    q = ss.find_queries(oracle, c, m, seed=ss.FIND_SEEDS[1])
    part = ss.participants(c)
    match, status, hit, counts = ss.find_expect(c, part, q, q.stored)
    found, from_blob = (status & ss.FIND_FOUND) != 0, q.pick >= 0
    assert set((q.key_off[:-1] % np.uint64(16)).tolist()) == set(range(16))          # every CSR start
    assert m % 256 and m > 4096 and -(-m // 64) > 64 * 64                            # the counter lines wrap
    assert counts == [m - 100, int(found.sum()), 0] and counts[1] > m * 9 // 10      # 244,238
    first = ss.find_expect(c, part, q, q.stored, later="first")
    assert (first[0] != match).sum() > 10_000 and (first[0][~found] == NONE).all()   # 100,552
    assert not ((first[1] ^ status) & (0xFF ^ ss.FIND_ATTRS)).any() and (first[2] != hit).sum() > 10_000
    later = found & from_blob
    assert (match[later].astype(np.int64) > q.pick[later]).sum() > 10_000            # 55,127
    assert (found & ((q.stored[0] & M32) == M32)).sum() >= 500                       # 3,662
    assert (found & (q.stored[0] == NONE)).sum() >= 2                                # 5
    true = ss.find_expect(c, part, q, q.true)
    assert (found & ((true[1] & ss.FIND_FOUND) == 0)).sum() >= 1_000                 # 6,682
    assert ((true[1][q.kind == ss.Q_FRESH] & ss.FIND_FOUND) == 0).all() and true[3][1] > m * 8 // 10
    out = (q.kind == ss.Q_PICK) & ~part[np.maximum(q.pick, 0)]
    assert (out & found).sum() >= 500 and (out & ~found).sum() >= 500                # 890 and 1,478
    near = q.kind == ss.Q_NEAR
    assert near.sum() > 8_000 and not found[near].any()
    assert ((status & ss.FIND_ATTRS) != 0).sum() >= 10_000                           # 35,975
    # without consider the masked blobs take part: another expectation
    assert (ss.find_expect(c, ss.participants(c, False), q, q.stored)[0] != match).sum() > 100


def test_runs_of_sorted_bits_hold_other_hashes(oracle):
    """Neighbours of the sorted column that share their sorted bits under different full hashes, the
    entries find's backward walk steps over by `hq != h`: 399 at 65,536 blobs (24 sorted bits), 14 at
    256 (16 bits)."""
    for n, bits, least in ((65536, 24, 100), (256, 16, 1)):
        c = ss.ralle_columns(oracle, n, seed=n)
        assert ss.sort_bits(n) == bits and ss.shared_sorted_bits(c, ss.participants(c), bits) >= least


# ----------------------------------------------------------------- an unstable sort would show
def test_any_later_copy_is_another_expectation(oracle, large_columns):
    """"The nearest later copy" swapped for "any later copy" (the last one): against the model at the
    small size, and against the constructed expectation at the large one, in thousands of entries
    of by and -- where attrs make the two copies differ -- of keep."""
    buf, off, consider, c = ss.dedup_stream(oracle, N_SMALL[1], seed=N_SMALL[1])
    want = dm.dedup_model(buf, off, consider=consider)
    wrong = ss.dedup_expect(c, ss.participants(c), later="any")
    assert (wrong[1] != want[1]).sum() > 5
    part = ss.participants(large_columns)
    right, wrong = ss.dedup_expect(large_columns, part), ss.dedup_expect(large_columns, part, later="any")
    assert (right[1] != wrong[1]).sum() > 10_000 and (right[0] != wrong[0]).sum() > 100
    data, recs, h1, f = ss.fold_log(oracle, N_SMALL[1], seed=N_SMALL[1] + 3)
    assert (ss.fold_expect(f, later="any")[1] != af.fold_model(af.recs_of(bytes(data), recs))[1]).sum() > 5
