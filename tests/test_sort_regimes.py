"""The sort-based stream calls where the library sort runs its Onesweep passes: N_LARGE pairs, just
above rocPRIM's merge_sort_limit, sorted on 32 bits (tests/test_scale_streams.py pins both against
the installed headers).  k2h_amd_ralledata_dedup and _dedup_mtime, k2h_amd_ralledata_diff,
k2h_amd_ralledata_subkeys with k2h_amd_ralledata_reach over its edges, and k2h_amd_archive_fold,
every output element against the expectation tests/scale_streams.py derives from the columns it
wrote -- which tests/test_scale_streams.py holds against the transliterated models at small sizes.
Nothing is sampled, nothing is timed, every comparison is exact.  Outputs are sentinel-filled and
guarded by the existing runners; the streams stand at a non-zero shift from a 16-byte boundary.
"""
import numpy as np
import pytest

import archive_fold_model as af
import big_offsets as bo
import ralle_diff_model as fm
import ralle_subkeys_model as sm
import ralle_times_model as tm
import scale_streams as ss
from scale_streams import N_LARGE

pytestmark = pytest.mark.gpu


def _free():
    import torch
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def dedup(cuda, oracle):
    """The dedup stream on the device, shared by the plain and the mtime rule's tests."""
    buf, off, consider, c = ss.dedup_stream(oracle, N_LARGE, seed=1)
    s = dict(t=tm.place(cuda, buf, 5), size=len(buf), off=off, consider=consider, c=c)
    yield s
    s.clear()
    _free()


@pytest.mark.parametrize("considered", [True, False])
def test_dedup(cuda, dedup, considered):
    c = dedup["c"]
    want = ss.dedup_expect(c, ss.participants(c, considered))
    got = tm.run_dedup_mtime(cuda, dedup["t"], dedup["size"], dedup["off"], None,
                             dedup["consider"] if considered else None, plain=True)
    tm.assert_dedup(got, want, f"dedup of {N_LARGE} blobs, consider {considered}")
    assert want[2] > N_LARGE // 8


def test_dedup_mtime_is_the_plain_rule_without_attrs(cuda, dedup):
    """The blobs without attrs of the same stream, chosen by consider: no mtime anywhere, so the mtime
    rule is the plain rule."""
    c = dedup["c"]
    consider = dedup["consider"] & ~c.att
    want = ss.dedup_expect(c, ss.participants(c) & ~c.att)
    got = tm.run_dedup_mtime(cuda, dedup["t"], dedup["size"], dedup["off"], (0, 0), consider)
    tm.assert_dedup(got, want, f"mtime rule, {N_LARGE} blobs, none with attrs")
    assert want[2] == int((want[1] != ss.NONE).sum()) > N_LARGE // 8


def test_diff(cuda, oracle):
    a, b, ca, cb, c = ss.diff_streams(oracle, N_LARGE, seed=2)
    assert (len(a[1]) - 1) + (len(b[1]) - 1) == N_LARGE
    want = ss.diff_expect(c, ss.participants(c))
    ta, tb = tm.place(cuda, a[0], 3), tm.place(cuda, b[0], 11, canary=0x5A)
    got = fm.run_diff(cuda, ta, len(a[0]), a[1], tb, len(b[0]), b[1], ca, cb)
    del ta, tb
    _free()
    fm.assert_diff(got, want, f"diff of {len(a[1]) - 1} incoming against {len(b[1]) - 1} held blobs")
    assert want[3][1] > 50_000


def test_subkeys_and_reach(cuda, oracle):
    buf, off, consider, c = ss.subkeys_stream(oracle, N_LARGE, seed=3)
    want = ss.subkeys_expect(oracle, c, ss.participants(c))
    assert c.n + want.counts[3] == N_LARGE
    t = tm.place(cuda, buf, 7)
    got = sm.run_subkeys(cuda, t, len(buf), off, consider)
    del t
    _free()
    sm.assert_edges(got, want, f"subkeys of {c.n} blobs with {want.counts[3]} names")
    roots = np.random.default_rng(4).random(c.n) < 1000 / c.n
    r_want, counts = ss.reach_expect(want, roots)
    reach, r_counts = sm.run_reach(cuda, want, roots.astype(np.uint8))
    _free()
    bad = np.nonzero(reach != r_want)[0]
    assert bad.size == 0, f"reach differs at blob {int(bad[0])}: got {reach[bad[0]]}, want {r_want[bad[0]]}"
    assert r_counts == counts and counts[0] > c.n // 3 and counts[1] > 8, (r_counts, counts)


def test_fold(cuda, oracle):
    """Once with the caller's h1 -- a function of the key that is not its hash for thousands of keys --
    and once with h1 computed by the call."""
    import torch
    data, recs, h1, c = ss.fold_log(oracle, N_LARGE, seed=4)
    want = ss.fold_expect(c)
    whole, file = bo.guarded(torch, cuda, len(data), shift=9, fill=0xA5)
    file[:] = torch.from_numpy(data).to(cuda)
    for name, h in (("h1 passed", h1), ("h1 computed", None)):
        got = af.run_fold_on(cuda, file, len(data), recs, h, whole=whole)
        af.assert_same(got, want, f"fold of {N_LARGE} records, {name}")
    del file, whole
    _free()
    assert want[2] > N_LARGE // 5
