"""Superseded duplicates under the mtime rule (include/k2hash_amd.h section 4b'''':
k2h_amd_ralledata_dedup_mtime; k2h_ralledata_dedup.hip) against dedup_mtime_model of
ralle_times_model.py, entry for entry: keep, by and dropped.

That the rule is safe -- the table after the kept blobs equals the table after all of them, from
every prior state of the key -- is shown on the CPU against ralle_dedup_model's transliteration of
K2HShm::SetElementByBinArray (lib/k2hshmdirect.cc:377-473) run over real serialized attrs;
libk2hash itself is not built here, so parity with it is a restatement.  Expected values never
come from the device code, and every device output is sentinel-filled first.
"""
import ctypes

import numpy as np
import pytest

from conftest import GOLDEN

import ralle_archive_model as am
import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_times_model as tm
from ralle_times_model import MTIME, NONE, timeval

from k2hash_amd import _native, archive, ralledata


# ------------------------------------------------------------------------------------- CPU
def _ident(oracle):
    b = dm.blobs_of(oracle, [b"k"], [b"x"])[0]
    return rm.get(b, 0, rm.F_HASH), rm.get(b, 0, rm.F_SUBHASH), b"k"


@pytest.mark.parametrize("what", ["pairs", "chains"])
def test_kept_blobs_replay_to_the_same_table(oracle, what):
    """Every pair (each blob with and without a value) and every chain of three of the ten attrs
    kinds, under every pts and from each of the 12 prior states: feeding the blobs the model
    keeps leaves the table that feeding all of them leaves.  No case is left out.  The
    control: the plain rule's mirror image (keep the first of a pair) fails somewhere."""
    cases = tm.pair_cases() if what == "pairs" else tm.chain_cases()
    blobs, spans = tm.case_blobs(oracle, cases, distinct_keys=False)
    priors = tm.prior_states(_ident(oracle))
    assert len(priors) == 12 and len(tm.ATTRS_KINDS) == 10
    assert len(cases) == (400 if what == "pairs" else 1000)
    checked = dropped_total = control_differs = 0
    with tm.real_attrs(tm.NOW):
        for (lo, hi) in spans:
            stream = blobs[lo:hi]
            buf, off = rm.join(stream)
            for pts in tm.PTS:
                keep, _by, dropped = tm.dedup_mtime_model(buf, off, pts)
                kept = [b for b, k in zip(stream, keep) if k]
                assert len(kept) == len(stream) - dropped
                dropped_total += dropped
                for name, prior in priors.items():
                    whole = dm.replay(stream, prior, pts)
                    assert dm.replay(kept, prior, pts) == whole, (lo, pts, name)
                    control_differs += dm.replay(stream[:1], prior, pts) != whole
                    checked += 1
    assert checked == len(cases) * len(tm.PTS) * 12
    assert dropped_total > len(cases) and control_differs > 0


def test_replay_reads_real_attrs(oracle):
    """The swapped hooks: GetMTime and IsExpire of serialized attrs, on the branches that use them."""
    ident = _ident(oracle)
    st = tm.prior_states(ident)
    blob = lambda kind: dm.blobs_of(oracle, [b"k"], [b"new"], None, [tm.ATTRS_KINDS[kind]])[0]  # noqa: E731
    new = lambda kind: {ident: (b"new", None, tm.ATTRS_KINDS[kind] or None)}  # noqa: E731
    pts = (2000, 0)
    with tm.real_attrs(tm.NOW):
        assert dm.replay([blob("m950.1")], st["m950"], pts) == new("m950.1")
        assert dm.replay([blob("m950")], st["m950"], pts) == st["m950"]                     # :416 is <=
        assert dm.replay([blob("m950")], st["m950"], (950, 0)) == st["m950"]                # :402 is <=
        assert dm.replay([blob("m900")], st["m1000.500-expired"], pts) == new("m900")       # :390
        assert dm.replay([blob("m900")], st["m950-live"], pts) == st["m950-live"]
        assert dm.replay([blob("none")], st["mtime-vl8"], pts) == new("none")               # :395: GetMTime fails
        assert dm.replay([blob("mtime-vl8")], st["m900"], pts) == st["m900"]                # :427
        assert dm.replay([blob("none")], st["m3000"], pts) == st["m3000"]                   # :402
    assert dm.attrs_mtime(dm.encode_attrs((5, 6))) == (5, 6)                                # the hooks are back


def test_model_rule_by_rule(oracle):
    def run(kinds, pts):
        blobs = dm.blobs_of(oracle, [b"k"] * len(kinds), [b"v"] * len(kinds), None, [tm.ATTRS_KINDS[k] for k in kinds])
        return tm.dedup_mtime_model(*rm.join(blobs), pts)[0].tolist()
    big = (5000, 0)
    assert run(["none", "none"], big) == [0, 1]                     # (a), the plain rule's case
    assert run(["uniqid-only", "m900"], big) == [0, 1]              # (a): attrs, but GetMTime fails
    assert run(["mtime-vl8", "none"], big) == [0, 1]
    assert run(["m900", "none"], big) == [1, 1]                     # i with an mtime before a j without one
    assert run(["m900", "m950"], big) == [0, 1]                     # (b)
    assert run(["m950", "m950"], big) == [1, 1]                     # m_i < m_j is strict
    assert run(["m950", "m950.1"], big) == [0, 1]
    assert run(["m950", "m950.1"], (950, 0)) == [1, 1]              # m_i < pts is strict: pts == m_i
    assert run(["m950", "m950.1"], (950, 1)) == [0, 1]
    assert run(["m950.1", "m950"], big) == [1, 1]
    assert run(["m950-expired", "m1000.500"], big) == [0, 1]        # an expired i: no special treatment
    assert run(["expired-only", "m900"], big) == [0, 1]
    assert run(["m900", "m950", "m900"], big) == [0, 1, 1]


def _host_stream(oracle):
    buf, off = rm.stream_of(oracle, rm.records(oracle, 4, seed=1))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64)


def test_dedup_mtime_argument_validation(oracle):
    """Judged on the host before any device is touched, each with its own message."""
    lib = _native.batch_lib()
    buf, off = _host_stream(oracle)
    n = off.size - 1
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    keep, by = np.full(n, 0xEE, np.uint8), np.zeros(n, np.uint64)
    dropped = ctypes.c_uint64(7)
    ts = _native.Timespec(1, 2)
    pts = ctypes.byref(ts)
    dedup = lib.k2h_amd_ralledata_dedup_mtime
    msg = lambda: bytes(lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL))  # noqa: E731
    assert dedup(None, 0, None, 0, None, None, None, ctypes.byref(dropped), None, None) == _native.K2H_AMD_OK
    assert dropped.value == 0
    texts = set()
    for args, text in (
            ((p(buf), buf.size, p(off), n, None, None, p(by), None, pts, None), b"NULL keep"),
            ((None, buf.size, p(off), n, None, p(keep), None, None, pts, None), b"NULL blobs"),
            ((p(buf), buf.size, None, n, None, p(keep), None, None, pts, None), b"NULL blob_off"),
            ((p(buf), buf.size, p(off), n, None, p(keep), None, None, None, None), b"NULL pts"),
            ((p(buf), buf.size, p(off), (1 << 32) - 1, None, p(keep), None, None, pts, None), b"2^32 - 2")):
        assert dedup(*args) == _native.K2H_AMD_EINVAL
        assert text in msg()
        texts.add(msg())
    assert len(texts) == 5 and all(b"ralledata_dedup_mtime: " in t for t in texts)
    assert (keep == 0xEE).all()


# ---- the streams of the GPU tests, and (CPU) that each is what its test claims
def _enumeration_stream(oracle):
    """Every pair and every chain as one stream, a distinct key per case."""
    cases = tm.pair_cases() + tm.chain_cases()
    blobs, spans = tm.case_blobs(oracle, cases, distinct_keys=True)
    return rm.join(dm.at_odd_offsets(blobs, seed=2)), spans


def test_enumeration_stream_is_the_cases_side_by_side(oracle):
    (buf, off), spans = _enumeration_stream(oracle)
    assert len(off) - 1 == 400 * 2 + 1000 * 3
    for pts in tm.PTS[1:3]:
        keep, by, dropped = tm.dedup_mtime_model(buf, off, pts)
        for lo, hi in spans[::37]:
            alone = tm.dedup_mtime_model(*rm.join([buf[off[i]:off[i + 1]] for i in range(lo, hi)]), pts)
            assert keep[lo:hi].tolist() == alone[0].tolist()
    assert {(off[i] + rm.get(buf, off[i], rm.F_APOS)) % 16 for i in range(len(off) - 1)
            if rm.get(buf, off[i], rm.F_ALEN)} == set(range(16))


def _edge_stream(oracle, W):
    """ralle_dedup_model's edge layout with mtimes: runs of three equal identities at sorted
    positions 62-64 (a wave edge) and W-2..W (a block edge), mtimes rising then falling, every
    other position a key of its own; stored hashes are small integers, so the order is known."""
    npos = 2 * W + 70
    group = list(range(npos))
    for lo in (62, W - 2):
        group[lo + 1] = group[lo + 2] = lo
    keys = [b"edge-key-%05d" % g for g in group]
    order = np.random.default_rng(11).permutation(npos)
    mt = {62: 900, 63: 950, 64: 920, W - 2: 950, W - 1: 900, W: 990}
    attrs = [tm.written_attrs([(MTIME, timeval(mt.get(int(p), 800), 0))]) for p in order]
    blobs = dm.blobs_of(oracle, [keys[p] for p in order], [b"v%d" % i for i in range(npos)], None, attrs)
    for b, p in zip(blobs, order):
        dm.set_hash(b, group[p])
    return rm.join(blobs), [group[p] for p in order]


def test_edge_stream_puts_the_runs_on_the_edges(oracle):
    W = dm.RESOLVE_BLOCK
    (buf, off), hashes = _edge_stream(oracle, W)
    srt = sorted(range(len(hashes)), key=lambda i: (hashes[i], i))
    for lo in (62, W - 2):
        assert [hashes[srt[p]] for p in range(lo - 1, lo + 4)] == [lo - 1, lo, lo, lo, lo + 3]
    keep, by, dropped = tm.dedup_mtime_model(buf, off, (5000, 0))
    assert 1 <= dropped <= 4 and (by != NONE).sum() == 4
    assert dm.dedup_model(buf, off)[2] == 0          # every blob has attrs: the plain rule drops nothing


def _mixed_stream(oracle, seed, n=3000, p_attrs=0.6):
    rng = np.random.default_rng(900 + seed)
    kinds = list(tm.ATTRS_KINDS.values())
    pool = [bytes(rng.integers(0, 256, int(rng.integers(1, 50)), dtype=np.uint8)) for _ in range(n // 6)]
    keys = [pool[int(k)] for k in rng.integers(0, len(pool), n)]
    vals = [b"" if rng.random() < 0.1 else b"v%d" % i for i in range(n)]
    attrs = []
    for _ in range(n):
        u = rng.random()
        if u >= p_attrs:
            attrs.append(b"")
        elif u < p_attrs / 2:
            attrs.append(kinds[int(rng.integers(0, len(kinds)))])
        else:
            attrs.append(tm.written_attrs([(MTIME, timeval(int(rng.integers(940, 960)), int(rng.integers(0, 3))))]))
    blobs = dm.blobs_of(oracle, keys, vals, None, attrs)
    for i in rng.integers(0, n, 30):             # a few hash collisions between different keys
        dm.set_hash(blobs[int(i)], 77, 99)
    consider = (rng.random(n) < 0.9).astype(np.uint8)
    return rm.join(dm.at_odd_offsets(blobs, seed)), consider


def test_mixed_stream_model_is_a_superset_of_the_plain_rule(oracle):
    (buf, off), consider = _mixed_stream(oracle, 0, n=900)
    plain = dm.dedup_model(buf, off, consider=consider)
    mt = tm.dedup_mtime_model(buf, off, (950, 1), consider=consider)
    assert (plain[1] == mt[1]).all()
    assert not ((plain[0] == 0) & (mt[0] == 1)).any() and plain[2] < mt[2]


# ------------------------------------------------------------------------------------- GPU
def against_model(cuda, buf, off, pts, what, shift=0, consider=None, tail_pad=tm.PAD):
    want = tm.dedup_mtime_model(buf, off, pts, consider=consider)
    got = tm.run_dedup_mtime(cuda, tm.place(cuda, buf, shift, tail_pad=tail_pad), len(buf), off, pts, consider)
    tm.assert_dedup(got, want, what)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("pts", tm.PTS)
def test_pairs_and_chains(cuda, oracle, pts):
    """pts below every mtime, equal to m_i (950.0 and 950.1 both occur as m_i), and above."""
    (buf, off), _spans = _enumeration_stream(oracle)
    keep, by, dropped = against_model(cuda, buf, off, pts, f"enumeration, pts {pts}", shift=pts[1] % 16)
    # rule (a) alone: 4 of the 10 kinds give no mtime, so 4 * 2 * 10 * 2 pairs and 2 * 4 * 100 chain
    # blobs; pts = (800, 0) is below every mtime, so rule (b) adds nothing there and something above
    assert dropped == 960 if pts == (800, 0) else dropped > 960


@pytest.mark.gpu
def test_runs_across_wave_and_block_edges(cuda, oracle):
    (buf, off), _hashes = _edge_stream(oracle, dm.RESOLVE_BLOCK)
    for pts in ((5000, 0), (950, 0)):
        against_model(cuda, buf, off, pts, f"edges, pts {pts}")


@pytest.mark.gpu
def test_equal_to_the_plain_rule_without_attrs(cuda, oracle):
    (buf, off), consider = _mixed_stream(oracle, 1, p_attrs=0.0)
    t = tm.place(cuda, buf, 3)
    want = dm.dedup_model(buf, off, consider=consider)
    tm.assert_dedup(tm.run_dedup_mtime(cuda, t, len(buf), off, (0, 0), consider), want, "mtime rule, no attrs")
    tm.assert_dedup(tm.run_dedup_mtime(cuda, t, len(buf), off, None, consider, plain=True), want, "plain rule")
    assert want[2] > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_mixed_stream_superset_and_same_by(cuda, oracle, seed):
    """consider masks, attrs of every kind: the model; every blob the plain rule drops is dropped;
    by is the plain rule's by."""
    (buf, off), consider = _mixed_stream(oracle, seed)
    t = tm.place(cuda, buf, seed + 1)
    for cons in (consider, None):
        for pts in ((950, 1), (5000, 0)):
            want = tm.dedup_mtime_model(buf, off, pts, consider=cons)
            got = tm.run_dedup_mtime(cuda, t, len(buf), off, pts, cons)
            tm.assert_dedup(got, want, f"mixed {seed}, pts {pts}")
            plain = tm.run_dedup_mtime(cuda, t, len(buf), off, None, cons, plain=True)
            tm.assert_dedup(plain, dm.dedup_model(buf, off, consider=cons), "plain rule on the same stream")
            assert (got[1] == plain[1]).all()
            assert not ((plain[0] == 0) & (got[0] == 1)).any() and plain[2] < got[2]


@pytest.mark.gpu
def test_wrapper_with_and_without_pts(cuda, oracle):
    """dedup_ralledata: pts selects the mtime rule; without it the call made is today's."""
    import torch
    (buf, off), consider = _mixed_stream(oracle, 2, n=1200)
    t = tm.place(cuda, buf)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    cons = torch.from_numpy(consider).to(cuda)
    calls = []
    real = _native.batch_lib()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def call(*a):
                calls.append((name, len(a)))
                return fn(*a)
            return call
    saved = _native.batch_lib
    _native.batch_lib = lambda: Spy()
    try:
        keep, by, dropped = ralledata.dedup_ralledata(t, d_off, consider=cons, want_by=True)
        assert calls == [("k2h_amd_ralledata_dedup", 9)]
        del calls[:]
        keep2, by2, dropped2 = ralledata.dedup_ralledata(t, d_off, consider=cons, want_by=True, pts=(950, 1))
        assert calls == [("k2h_amd_ralledata_dedup_mtime", 10)]
        del calls[:]
        ralledata.route_ralledata(t, d_off, rm.Range(0, 2).ctypes(), dedup=True)
        assert [c[0] for c in calls] == ["k2h_amd_ralledata_check", "k2h_amd_ralledata_dedup"] + \
            ["k2h_amd_ralledata_select"] * 2
    finally:
        _native.batch_lib = saved
    torch.cuda.synchronize()
    tm.assert_dedup((keep.cpu().numpy(), by.cpu().numpy().view(np.uint64), dropped),
                    dm.dedup_model(buf, off, consider=consider), "wrapper, plain")
    tm.assert_dedup((keep2.cpu().numpy(), by2.cpu().numpy().view(np.uint64), dropped2),
                    tm.dedup_mtime_model(buf, off, (950, 1), consider=consider), "wrapper, pts")
    keep3, _by, none = ralledata.dedup_ralledata(t, d_off, consider=cons, count=False, pts=(950, 1))
    torch.cuda.synchronize()
    assert none is None and torch.equal(keep3, keep2)


@pytest.mark.gpu
def test_route_with_window_dedup_and_pts(cuda, oracle):
    """route_ralledata(window=..., dedup=True, pts=...) end to end against the composed models:
    check, then the window under the check's route, then the mtime rule among what is left."""
    import torch
    rng = np.random.default_rng(41)
    n = 600
    keys = [b"route-key-%d" % int(k) for k in rng.integers(0, 90, n)]
    attrs = [b"" if rng.random() < 0.2 else
             tm.written_attrs([(MTIME, timeval(int(rng.integers(900, 1100)), 0))] +
                              ([(tm.EXPIRE, timeval(int(rng.integers(1400, 1600)), 0))] if rng.random() < 0.3 else []))
             for _ in range(n)]
    blobs = dm.blobs_of(oracle, keys, [b"v%d" % i for i in range(n)], None, attrs)
    dm.set_hash(blobs[17], rm.get(blobs[17], 0, rm.F_HASH) ^ 4)      # BAD_HASH
    buf, off = rm.join(blobs)
    r = rm.Range(0, 2, 1, 1, 3)
    status, route, _h1, _h2 = rm.expected(oracle, buf, off, rng=r)
    routed = ((status == rm.OK) & ((route & 1) != 0)).astype(np.uint8)
    win, pts = tm.Window((950, 0), (1050, 0), (1500, 0)), (1000, 0)
    timed = routed & tm.times_model(buf, off, consider=routed, window=win, route=route)[3]
    final = timed & tm.dedup_mtime_model(buf, off, pts, consider=timed)[0]
    plain = timed & dm.dedup_model(buf, off, consider=timed)[0]
    assert 0 < final.sum() < plain.sum() <= timed.sum() < routed.sum() < n
    assert (route & 2).any() and not (route & 2).all()
    t = tm.place(cuda, buf)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    w = ralledata.TimeWindow(win.start, win.end, win.now)
    for kw, keep in (({"window": w, "dedup": True, "pts": pts}, final), ({"window": w, "dedup": True}, plain),
                     ({"window": w}, timed), ({}, routed)):
        data, ooff, index = rm.select_model(buf, off, keep)
        sel, res = ralledata.route_ralledata(t, d_off, r.ctypes(), **kw)
        torch.cuda.synchronize()
        assert (res.status.cpu().numpy() == status).all()
        assert sel.kept == int(keep.sum()) and sel.kept_bytes == data.size, sorted(kw)
        assert (sel.blobs.cpu().numpy() == data).all()
        assert (sel.index.cpu().numpy().view(np.uint64) == index).all()


@pytest.mark.gpu
def test_archive_to_compacted_archive(cuda):
    """scan -> blobs -> dedup under the mtime rule -> archive, on the archive fixture laid down
    twice: the second copy of every SET_ALL record supersedes the first only where the first has
    no mtime, and the written archive holds the kept blobs' records."""
    import torch
    raw = (GOLDEN / "archive.k2har").read_bytes()
    file = torch.from_numpy(np.frombuffer(raw + raw, np.uint8).copy()).to(cuda)
    recs = archive.scan_device(file)
    blobs, boff = ralledata.archive_to_ralledata(file, recs)
    pts = (1 << 40, 0)
    keep, by, dropped = ralledata.dedup_ralledata(blobs, boff, want_by=True, pts=pts)
    torch.cuda.synchronize()
    hbuf, hoff = blobs.cpu().numpy().tobytes(), boff.cpu().numpy()
    want = tm.dedup_mtime_model(hbuf, hoff, pts)
    tm.assert_dedup((keep.cpu().numpy(), by.cpu().numpy().view(np.uint64), dropped), want, "archive twice")
    assert dropped > 0
    out = ralledata.ralledata_to_archive(blobs, boff, keep=keep)
    torch.cuda.synchronize()
    data, _rec_off, records, _segs = am.model(hbuf, hoff, keep=want[0])
    assert out.records == records == int(want[0].sum()) and out.total == len(data)
    assert out.bytes.cpu().numpy().tobytes() == bytes(data)
