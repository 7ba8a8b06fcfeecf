"""k2h_amd_ralledata_index, _find and _fetch where the library sort changes its algorithm and where
the index sorts on more bits: the dedup stream of tests/scale_streams.py at N_LARGE blobs (Onesweep
passes, 32 sorted bits) under M_LARGE queries -- 4,098 waves, so the counter lines wrap -- and at
sizes on both sides of the one-block limit, inside the merge sort, and on both sides of the steps
from 16 to 24 and from 24 to 32 sorted bits.  Every output element is held against the expectation
scale_streams.find_expect derives from the columns, which tests/test_scale_streams.py holds against
ralle_find_model.find_model at small sizes and whose inputs it counts at this one.  Nothing is
sampled, nothing is timed, every comparison is exact.  Outputs are sentinel-filled and guarded by
the runners of ralle_find_model.py; stream and keys stand at non-zero shifts from a 16-byte boundary.
"""
import numpy as np
import pytest

import ralle_find_model as fm
import ralle_times_model as tm
import scale_streams as ss
from scale_streams import M_LARGE, N_LARGE, NONE

pytestmark = pytest.mark.gpu
NOW = tm.NOW
SIZES = (1024, 1025, 3000, 65536, 65537, 256, 257)


def _free():
    import torch
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def large(cuda, oracle):
    """The dedup stream and its queries on the device, shared by the find and the fetch tests."""
    buf, off, consider, c = ss.dedup_stream(oracle, N_LARGE, seed=ss.FIND_SEEDS[0])
    q = ss.find_queries(oracle, c, M_LARGE, seed=ss.FIND_SEEDS[1])
    s = dict(t=tm.place(cuda, buf, 5), kt=tm.place(cuda, q.bytes, 11), size=len(buf), off=off, consider=consider, c=c, q=q)
    yield s
    s.clear()
    _free()


def _find_both_ways(cuda, s, considered, now, what):
    """Index over consider or None, then find with the stored hashes passed and with none passed."""
    c, q = s["c"], s["q"]
    part = ss.participants(c, considered)
    index, parts, doff = fm.run_index(cuda, s["t"], s["size"], s["off"], s["consider"] if considered else None)
    assert parts == int(part.sum()), what
    for name, hashes, given in (("stored hashes passed", q.stored, q.stored), ("hashes computed", q.true, (None, None))):
        want = ss.find_expect(c, part, q, hashes, now=now)
        got = fm.run_find(cuda, s["t"], s["size"], doff, c.n, index, s["kt"], len(q.bytes), q.key_off, given[0], given[1], 0, now)
        fm.assert_found(got, want, f"{what}, {name}")
        assert want[3][1] > q.m // 2 and want[3][2] == 0
    del index, doff


@pytest.mark.parametrize("now", [None, NOW])
@pytest.mark.parametrize("considered", [True, False])
def test_find_large(cuda, large, considered, now):
    _find_both_ways(cuda, large, considered, now, f"find of {M_LARGE} keys in {N_LARGE} blobs, consider {considered}, now {now}")
    _free()


@pytest.mark.parametrize("n", SIZES)
def test_find_sizes(cuda, oracle, n):
    """One block and the merge sort (1024 | 1025), 16 | 24 sorted bits (256 | 257), 24 | 32 (65,536 |
    65,537), and 3,000: the size at which the expectation is held against the model."""
    buf, off, consider, c = ss.dedup_stream(oracle, n, seed=n)
    q = ss.find_queries(oracle, c, min(2 * n, 20_000), seed=n + 4)
    s = dict(t=tm.place(cuda, buf, 9), kt=tm.place(cuda, q.bytes, 3), size=len(buf), off=off, consider=consider, c=c, q=q)
    _find_both_ways(cuda, s, True, NOW, f"find of {q.m} keys in {n} blobs")


def _gather(rows, lens):
    """The rows' first lens[i] bytes, end to end."""
    return rows[np.arange(rows.shape[1])[None, :] < lens[:, None]]


@pytest.mark.parametrize("segment", ["value", "key"])
def test_fetch_large(cuda, large, segment):
    """which = the expected match of the stored-hash find, ~0 entries included: 2^18 + 77 slots, 16,400
    copy blocks.  Whole, and with take cutting every third slot."""
    import torch
    c, q = large["c"], large["q"]
    which = ss.find_expect(c, ss.participants(c), q, q.stored)[0]
    assert (which == NONE).sum() > 10_000
    doff = torch.from_numpy(np.asarray(large["off"], np.int64)).to(cuda)
    for take in (None, (np.arange(q.m) % 3 != 0).astype(np.uint8)):
        use = (which != NONE) if take is None else (which != NONE) & (take != 0)
        j = which[use].astype(np.int64)
        lens = np.zeros(q.m, np.int64)
        lens[use] = ss.VLEN if segment == "value" else c.klen[j]
        want = _gather(c.val[j], lens[use]) if segment == "value" else _gather(c.key[j], lens[use])
        want_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        rc, data, ooff, bad, total = fm.run_fetch(cuda, large["t"], large["size"], doff, c.n, which, segment, take)
        what = f"fetch of {segment}, take {take is not None}"
        assert rc == 0 and total == want.size == int(want_off[-1]), what
        assert (ooff == want_off).all(), f"{what}: out_off differs"
        assert not bad.any(), f"{what}: bad set"
        diff = np.flatnonzero(np.frombuffer(data, np.uint8) != want)
        assert diff.size == 0, f"{what}: {diff.size} bytes differ, first at {int(diff[0])}"
    del doff
    _free()
