"""The RALLEDATA consumer side (include/k2hash_amd.h section 4b: k2h_amd_ralledata_check,
k2h_amd_ralledata_select; k2h_ralledata_check.hip) against the model of ralle_check_model.py,
blob for blob.

The model restates the status precedence and, line by line, the hash-range test of
K2HShm::GetElementListToBinary (lib/k2hshmdirect.cc:118-131, 165-176); libk2hash itself is
not built here (it needs libfullock), so parity with it is a restatement.  The blobs are the
oracle's (oracle_build_ralledata, pinned byte for byte to the reference-built fixture
tests/golden/ralledata.json by tests/test_ralledata.py) and the hashes the oracle's.
"""
import ctypes
import json

import numpy as np
import pytest

from conftest import GOLDEN

import ralle_check_model as rm
from ralle_check_model import M64, Range

from k2hash_amd import _native, ralledata


@pytest.fixture(scope="module")
def golden():
    recs = json.loads((GOLDEN / "ralledata.json").read_text())["records"]
    b = bytes.fromhex
    return [[b(r[f]) for r in recs] for f in ("key", "val", "skey", "attrs")], [b(r["blob"]) for r in recs]


# The parameter sets of the range test: the issue's pinned cases, an old range, and sets whose
# moduli are not powers of two.
RANGES = {
    "t6-max8-range4": Range(6, 8, 4),
    "range0": Range(3, 8, 0),
    "range-negative": Range(3, 8, -5),
    "t9-max8-range1": Range(9, 8, 1),
    "old-none": Range(1, 3, 1, M64, 0),
    "old-range": Range(1, 3, 1, 2, 5),
    "old-wraps": Range(0, 7, 3, 6, 7),
    "sum-crosses-2-64": Range(M64 - 1, 1000, 4),
    "max-2-64-minus-1": Range(5, M64, 1 << 62, 1 << 63, M64 - 2),
}


# ------------------------------------------------------------------------------------- CPU
def test_model_marks_reference_fixture_ok(oracle, golden):
    segs, blobs = golden
    buf, off = rm.join(blobs)
    assert len(blobs) == 48
    status, _route, h1, h2 = rm.expected(oracle, buf, off)
    assert not status.any()
    assert [int(x) for x in h1] == [rm.get(b, 0, rm.F_HASH) for b in blobs]
    assert [int(x) for x in h2] == [rm.get(b, 0, rm.F_SUBHASH) for b in blobs]
    # the oracle's producer gives the same stream (what every other test here builds on)
    obuf, ooff = rm.stream_of(oracle, segs)
    assert bytes(obuf) == bytes(buf) and ooff == off


def _accepted(r, hashes=range(64)):
    return {h % r.target_max_hash for h in hashes if rm.is_target(h, r)}


def test_range_model_pinned_cases():
    assert _accepted(Range(6, 8, 4)) == {6, 7, 0, 1}
    assert _accepted(Range(3, 8, 1)) == {3}
    assert _accepted(Range(3, 8, 0)) == {3} and _accepted(Range(3, 8, -7)) == {3}  # as range 1
    # target_hash >= target_max_hash: end = 1 < 9, so everything but 1 < m < 9 passes
    assert _accepted(Range(9, 8, 1)) == {0, 1}
    assert all(rm.route_of(h, Range(1, 3, 1, M64, 0)) & 2 == 0 for h in range(50))  # no old range, no modulo
    assert {h % 5 for h in range(50) if rm.route_of(h, Range(1, 3, 1, 2, 5)) & 2} == {2}
    # target_hash + range - 1 crosses 2^64: (2^64 - 2) + 3 wraps to 1, so end = 1 % 1000 = 1 < target_hash
    r = Range(M64 - 1, 1000, 4)
    assert _accepted(r, range(3000)) == {0, 1}
    assert not rm.is_target(M64, r) and M64 % 1000 > 1
    assert rm.is_target(2001, r) and not rm.is_target(2002, r)


def _host_stream(oracle):
    buf, off = rm.stream_of(oracle, rm.records(oracle, 4, seed=1))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64)


def test_check_argument_validation(oracle):
    """Judged before any device is touched: the same answers with and without a GPU."""
    lib = _native.batch_lib()
    buf, off = _host_stream(oracle)
    n = off.size - 1
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    status, route = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    rng = Range(0, 2).ctypes()
    check = lib.k2h_amd_ralledata_check
    assert check(None, 0, None, 0, None, 0, None, None, None, None, None) == _native.K2H_AMD_OK
    assert check(p(buf), buf.size, p(off), n, None, 0, None, None, None, None, None) == _native.K2H_AMD_EINVAL
    assert check(p(buf), buf.size, p(off), n, ctypes.byref(Range(0, 0).ctypes()), 0, p(status), p(route), None, None,
                 None) == _native.K2H_AMD_EINVAL
    assert check(p(buf), buf.size, p(off), n, ctypes.byref(Range(0, 2, 1, 1, 0).ctypes()), 0, p(status), p(route), None,
                 None, None) == _native.K2H_AMD_EINVAL  # old_max_hash == 0 with an old range
    assert check(p(buf), buf.size, p(off), n, None, _native.K2H_AMD_FLAG_CSTR, p(status), None, None, None,
                 None) == _native.K2H_AMD_EINVAL
    assert check(p(buf), buf.size, p(off), n, None, 0, p(status), p(route), None, None, None) == _native.K2H_AMD_EINVAL
    assert check(p(buf), buf.size, p(off), n, ctypes.byref(rng), 0, p(status), None, None, None,
                 None) == _native.K2H_AMD_EINVAL
    assert b"range and route" in lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL)


def test_select_argument_validation(oracle):
    lib = _native.batch_lib()
    buf, off = _host_stream(oracle)
    n = off.size - 1
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    keep = np.ones(n, np.uint8)
    kept, kb = ctypes.c_uint64(7), ctypes.c_uint64(7)
    sel = lib.k2h_amd_ralledata_select
    assert sel(None, 0, None, 0, None, None, 0, None, None, ctypes.byref(kept), ctypes.byref(kb), None) == 0
    assert kept.value == 0 and kb.value == 0
    assert sel(p(buf), buf.size, p(off), n, None, None, 0, None, None, ctypes.byref(kept), ctypes.byref(kb),
               None) == _native.K2H_AMD_EINVAL  # keep
    assert sel(p(buf), buf.size, p(off), n, p(keep), None, 0, None, None, None, ctypes.byref(kb),
               None) == _native.K2H_AMD_EINVAL  # kept
    assert sel(p(buf), buf.size, p(off), n, p(keep), p(buf), buf.size, None, None, ctypes.byref(kept), ctypes.byref(kb),
               None) == _native.K2H_AMD_EINVAL  # out without out_off


def test_public_names():
    import k2hash_amd
    for name in ("check_ralledata", "select_ralledata", "route_ralledata", "HashRange"):
        assert hasattr(k2hash_amd, name) and name in k2hash_amd.__all__
    assert (ralledata.OK, ralledata.BAD_SPAN, ralledata.EMPTY, ralledata.NO_KEY, ralledata.BAD_RANGE,
            ralledata.BAD_HASH, ralledata.BAD_SUBHASH) == tuple(range(7))
    assert ctypes.sizeof(ralledata.HashRange) == 40


def test_stage_boundary_streams_reach_both_forms(oracle):
    """The stage-boundary streams of the GPU test below put tiles on both sides of kCheckStage
    (read from the kernel source), at both base alignments."""
    buf, off = _boundary_stream(oracle)
    f0, f8 = rm.tile_forms(0, off, len(buf)), rm.tile_forms(8, off, len(buf))
    # tile t holds STAGE + 16 (t % 5 - 2) bytes: aligned, the hull is the tile; at base 8 it is 16 more
    assert f0 == ["staged" if t % 5 <= 2 else "direct" for t in range(len(f0))]
    assert f8 == ["staged" if t % 5 <= 1 else "direct" for t in range(len(f8))]


# ------------------------------------------------------------------------------------- GPU
PAD = 64  # canary bytes on either side of a placed buffer (keeps its 16-byte alignment)


def place(cuda, buf, shift=0, canary=0xA5):
    """buf on the device, starting `shift` bytes past a 16-byte boundary, canary bytes around."""
    import torch
    whole = np.full(PAD + shift + len(buf) + PAD, canary, np.uint8)
    whole[PAD + shift:PAD + shift + len(buf)] = np.frombuffer(bytes(buf), np.uint8)
    t = torch.from_numpy(whole).to(cuda)
    assert t.data_ptr() % 16 == 0
    return t[PAD + shift:PAD + shift + len(buf)]


def run_check(cuda, buf, off, shift=0, rng=None, std_fnv=False, size=None):
    import torch
    t = place(cuda, buf, shift)
    if size is not None:
        t = t[:size]
    o = torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)
    res = ralledata.check_ralledata(t, o, rng.ctypes() if rng is not None else None, std_fnv=std_fnv,
                                    want_hashes=True)
    torch.cuda.synchronize()
    u64 = lambda x: x.cpu().numpy().view(np.uint64)  # noqa: E731
    return res.status.cpu().numpy(), None if res.route is None else res.route.cpu().numpy(), u64(res.h1), u64(res.h2)


def assert_same(got, want, what):
    for name, g, w in zip(("status", "route", "h1", "h2"), got, want):
        if w is None:
            assert g is None, (what, name)
            continue
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {name} differs at blob {int(bad[0])}: got {g[bad[0]]}, want {w[bad[0]]}"


def check_against_model(cuda, oracle, buf, off, what, shift=0, rng=None, variant=0, size=None):
    want = rm.expected(oracle, buf if size is None else buf[:size], off, size, variant, rng)
    got = run_check(cuda, buf, off, shift, rng, std_fnv=bool(variant), size=size)
    assert_same(got, want, what)
    return want


@pytest.mark.gpu
def test_reference_fixture(cuda, oracle, golden):
    segs, blobs = golden
    buf, off = rm.join(blobs)
    status, _r, h1, h2 = run_check(cuda, buf, off)
    assert not status.any()
    assert [int(x) for x in h1] == [rm.get(b, 0, rm.F_HASH) for b in blobs]
    assert [int(x) for x in h2] == [rm.get(b, 0, rm.F_SUBHASH) for b in blobs]
    # the same stream under the other seed: every hash field is wrong
    status, _r, g1, g2 = run_check(cuda, buf, off, std_fnv=True)
    assert (status == rm.BAD_HASH).all()
    r1, r2 = zip(*[(oracle.k2h_hash(k, 1), oracle.k2h_second_hash(k, 1)) for k in segs[0]])
    assert [int(x) for x in g1] == list(r1) and [int(x) for x in g2] == list(r2)
    # and a stream built with that seed is all OK under it
    vbuf, voff = rm.stream_of(oracle, segs, variant=1)
    status, _r, g1, _g2 = run_check(cuda, vbuf, voff, std_fnv=True)
    assert not status.any() and [int(x) for x in g1] == list(r1)


@pytest.mark.gpu
def test_one_corruption_per_status(cuda, oracle):
    """One corruption per blob, spread over a 200-blob stream; tiles 0 and 1 stay in the staged
    form, the span corruptions (which send their tile to the direct form) sit in tiles 2 and 3."""
    buf, off = rm.stream_of(oracle, rm.records(oracle, 200, klen=(2, 65), vlen=(1, 201), seed=3, p_empty=0))
    blobs = rm.split(buf, off)
    want = {}

    def plant(i, status, fn):
        fn(blobs[i])
        want[i] = status
    L = lambda b: len(b)  # noqa: E731
    plant(5, rm.BAD_HASH, lambda b: rm.put(b, 0, rm.F_HASH, rm.get(b, 0, rm.F_HASH) ^ (1 << 17)))
    plant(13, rm.BAD_SUBHASH, lambda b: rm.put(b, 0, rm.F_SUBHASH, rm.get(b, 0, rm.F_SUBHASH) ^ (1 << 63)))
    plant(21, rm.NO_KEY, lambda b: rm.put(b, 0, rm.F_KLEN, 0))
    plant(29, rm.EMPTY, lambda b: [rm.put(b, 0, f, 0) for f in (rm.F_KLEN, rm.F_VLEN, rm.F_SLEN, rm.F_ALEN)])
    plant(37, rm.BAD_RANGE, lambda b: rm.put(b, 0, rm.F_KPOS, 79))
    plant(45, rm.BAD_RANGE, lambda b: rm.put(b, 0, rm.F_KPOS, -1))
    plant(53, rm.BAD_RANGE, lambda b: rm.put(b, 0, rm.F_VPOS, L(b) + 1 - rm.get(b, 0, rm.F_VLEN)))
    plant(61, rm.BAD_RANGE, lambda b: rm.put(b, 0, rm.F_VLEN, 1 << 63))
    plant(69, rm.BAD_RANGE, lambda b: rm.put(b, 0, rm.F_SLEN, M64))  # pos + len wraps in 64 bits
    # precedence: a bad range together with a bad hash
    plant(77, rm.BAD_RANGE, lambda b: (rm.put(b, 0, rm.F_HASH, 1), rm.put(b, 0, rm.F_KPOS, 79)))
    plant(85, rm.BAD_HASH, lambda b: (rm.put(b, 0, rm.F_HASH, 1), rm.put(b, 0, rm.F_SUBHASH, 1)))
    # still OK: trailing slack, the value before the key, garbage positions on empty segments
    plant(93, rm.OK, lambda b: b.extend(b"\xee" * 23))
    blobs[101] = rm.value_before_key(blobs[101])
    want[101] = rm.OK
    plant(109, rm.OK, lambda b: (rm.put(b, 0, rm.F_SPOS, M64), rm.put(b, 0, rm.F_APOS, 3)))
    plant(64, rm.BAD_HASH, lambda b: rm.put(b, 0, rm.F_HASH, 0))   # a tile's first blob
    plant(127, rm.NO_KEY, lambda b: rm.put(b, 0, rm.F_KLEN, 0))    # and the last of one
    blobs.insert(150, bytearray(b"\x01" * 79))  # a 79-byte blob
    want = {(i if i < 150 else i + 1): s for i, s in want.items()}
    want[150] = rm.BAD_SPAN
    buf, off = rm.join(blobs)
    off[170] = off[171] + 5  # decreasing: blob 170 has a bad span, blob 169 gains trailing slack
    want[170] = rm.BAD_SPAN
    n = len(off) - 1
    size = len(buf)
    off[n] = size + 1  # the last blob runs past the stream
    want[n - 1] = rm.BAD_SPAN
    status, _r, h1, h2 = check_against_model(cuda, oracle, buf, off, "corruptions", size=size)
    for i in range(n):
        assert status[i] == want.get(i, rm.OK), (i, status[i])
    assert all(h1[i] == 0 and h2[i] == 0 for i, s in want.items() if 1 <= s <= 4)
    assert all(h1[i] != 0 for i, s in want.items() if s >= 5)
    forms = rm.tile_forms(0, off, size)
    assert forms == ["staged", "staged", "direct", "direct"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_small_counts(cuda, oracle, n):
    buf, off = rm.stream_of(oracle, rm.records(oracle, n, slen=(0, 16), seed=n))
    want = check_against_model(cuda, oracle, buf, off, n)
    assert not want[0].any()


@pytest.mark.gpu
def test_every_key_length(cuda, oracle):
    keys, vals, _s, _a = rm.records(oracle, 71 * 3, seed=9)
    keys = [(k * 72)[:1 + i % 71] for i, k in enumerate(keys)]
    buf, off = rm.stream_of(oracle, (keys, vals, None, None))
    status, _r, h1, h2 = check_against_model(cuda, oracle, buf, off, "key lengths")
    assert not status.any()
    assert all(h1[i] == h2[i] for i in range(0, len(keys), 71))  # one-byte keys: lib/k2hashfunc.cc:83


@pytest.mark.gpu
def test_large_blobs_among_small(cuda, oracle):
    """A 5000-byte key and a 5000-byte value in every 97th blob: direct-form tiles next to
    staged ones, with a wrong hash planted in some of the large blobs."""
    n = 1000
    keys, vals, _s, _a = rm.records(oracle, n, seed=11)
    big = oracle.gen_bytes(10000, byte_off=999).tobytes()
    for i in range(96, n, 97):
        keys[i], vals[i] = big[i:i + 5000], big[5000 - i:10000 - i]
    buf, off = rm.stream_of(oracle, (keys, vals, None, None))
    for i in range(96, n, 3 * 97):
        rm.put(buf, off[i], rm.F_SUBHASH, 5)
    forms = rm.tile_forms(0, off, len(buf))
    assert "staged" in forms and "direct" in forms
    status, _r, _h1, _h2 = check_against_model(cuda, oracle, buf, off, "large blobs")
    assert sorted(np.nonzero(status)[0]) == list(range(96, n, 3 * 97))


@pytest.mark.gpu
def test_base_shift_and_first_offset(cuda, oracle):
    """The stream at every alignment 0-15, and streams whose first offset is not 0."""
    buf, off = rm.stream_of(oracle, rm.records(oracle, 300, alen=(0, 24), seed=13))
    rm.put(buf, off[77], rm.F_HASH, 77)
    want = rm.expected(oracle, buf, off)
    for shift in range(16):
        assert_same(run_check(cuda, buf, off, shift), want, f"shift {shift}")
    blobs = rm.split(buf, off)
    for lead in (1, 37, 4099):
        lbuf, loff = rm.join(blobs, lead=b"\xc3" * lead)
        assert loff[0] == lead
        assert_same(run_check(cuda, lbuf, loff, shift=lead % 7), want, f"lead {lead}")


def _boundary_stream(oracle):
    """Tiles of TILE blobs whose bytes are STAGE + 16 (t % 5 - 2), 20 of them, so the tiles'
    hulls sit at the stage size - 32 .. + 32 (+ 16 when the base is not aligned)."""
    keys, vals = [], []
    data = oracle.gen_bytes(1 << 18, byte_off=21).tobytes()
    pos = 0
    for t in range(20):
        target = rm.STAGE + 16 * (t % 5 - 2) - rm.HEADER * rm.TILE  # key + value bytes of the tile
        per = target // rm.TILE
        for j in range(rm.TILE):
            kl = 8 + (j * 7 + t) % 24
            vl = per - kl + (1 if j < target - per * rm.TILE else 0)
            keys.append(data[pos:pos + kl])
            vals.append(data[pos + kl:pos + kl + vl])
            pos = (pos + kl + vl) % (len(data) - 1024)
    return rm.stream_of(oracle, (keys, vals, None, None))


@pytest.mark.gpu
def test_stage_boundary(cuda, oracle):
    buf, off = _boundary_stream(oracle)
    for t in range(0, 20, 3):
        rm.put(buf, off[rm.TILE * t + t], rm.F_HASH, t)
    want = rm.expected(oracle, buf, off)
    assert int((want[0] != 0).sum()) == 7
    for shift in (0, 8, 15):
        assert_same(run_check(cuda, buf, off, shift), want, f"boundary, shift {shift}")


@pytest.fixture(scope="module")
def routed_stream(oracle):
    buf, off = rm.stream_of(oracle, rm.records(oracle, 3000, seed=17))
    for i in range(10, 3000, 41):
        rm.put(buf, off[i], (rm.F_HASH, rm.F_SUBHASH, rm.F_KLEN, rm.F_KPOS)[i % 4], 1 << 40)
    return buf, off


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RANGES))
def test_route(cuda, oracle, routed_stream, name):
    buf, off = routed_stream
    status, route, _h1, _h2 = check_against_model(cuda, oracle, buf, off, name, rng=RANGES[name])
    assert (status != 0).sum() > 50 and not route[status != 0].any()
    assert route.any()


# ----------------------------------------------------------------------------- select
def run_select(cuda, buf, off, keep, cap=None, out=True, shift=0, out_shift=0, want_index=True):
    """k2h_amd_ralledata_select through ctypes; `out` between canary bytes.  Returns (rc, kept,
    kept_bytes, the out buffer with its canaries, out_off, index)."""
    import torch
    t = place(cuda, buf, shift)
    n = len(off) - 1
    o = torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)
    k = torch.from_numpy(np.asarray(keep, np.uint8)).to(cuda)
    cap = len(buf) if cap is None else cap
    whole = torch.full((PAD + out_shift + cap + PAD,), 0x5C, dtype=torch.uint8, device=cuda)
    ooff = torch.full((n + 1,), -1, dtype=torch.int64, device=cuda)
    idx = torch.full((n,), -1, dtype=torch.int64, device=cuda)
    kept, kb = ctypes.c_uint64(M64), ctypes.c_uint64(M64)
    rc = _native.batch_lib().k2h_amd_ralledata_select(
        ctypes.c_void_p(t.data_ptr()), len(buf), ctypes.c_void_p(o.data_ptr()), n, ctypes.c_void_p(k.data_ptr()),
        ctypes.c_void_p(whole.data_ptr() + PAD + out_shift) if out else None, cap, ctypes.c_void_p(ooff.data_ptr()),
        ctypes.c_void_p(idx.data_ptr()) if want_index else None, ctypes.byref(kept), ctypes.byref(kb),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, kept.value, kb.value, whole.cpu().numpy(), ooff.cpu().numpy().view(np.uint64), \
        idx.cpu().numpy().view(np.uint64)


def assert_selected(res, model, cap, out_shift=0, what=""):
    rc, kept, kb, whole, ooff, idx = res
    data, moff, mindex = model
    assert rc == 0, what
    assert (kept, kb) == (mindex.size, data.size), what
    lo = PAD + out_shift
    assert np.array_equal(whole[lo:lo + kb], data), what
    assert (whole[:lo] == 0x5C).all() and (whole[lo + kb:] == 0x5C).all(), f"{what}: bytes outside the kept span"
    assert np.array_equal(ooff[:kept + 1], moff) and (ooff[kept + 1:] == M64).all(), what
    assert np.array_equal(idx[:kept], mindex) and (idx[kept:] == M64).all(), what


@pytest.fixture(scope="module")
def select_stream(oracle):
    buf, off = rm.stream_of(oracle, rm.records(oracle, 2 * rm.SEL_TILE + 77, alen=(0, 24), seed=19))
    return rm.join(rm.split(buf, off), lead=b"\x11" * 29)  # a non-zero first offset


@pytest.mark.gpu
def test_select_all_and_none(cuda, select_stream):
    buf, off = select_stream
    n = len(off) - 1
    res = run_select(cuda, buf, off, np.ones(n, np.uint8), shift=3, out_shift=5)
    assert_selected(res, rm.select_model(buf, off, np.ones(n)), len(buf), 5, "keep all")
    assert np.array_equal(res[3][PAD + 5:PAD + 5 + res[2]], np.frombuffer(bytes(buf), np.uint8)[off[0]:off[n]])
    assert np.array_equal(res[4], np.array(off, np.uint64) - np.uint64(off[0]))
    res = run_select(cuda, buf, off, np.zeros(n, np.uint8))
    assert_selected(res, rm.select_model(buf, off, np.zeros(n)), len(buf), 0, "keep none")
    assert res[1] == 0 and res[2] == 0 and res[4][0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("out_shift", [0, 1, 9])
def test_select_random_half(cuda, select_stream, out_shift):
    buf, off = select_stream
    n = len(off) - 1
    keep = (np.random.default_rng(out_shift).random(n) < 0.5).astype(np.uint8) * 255
    model = rm.select_model(buf, off, keep)
    assert 0 < model[2].size < n
    assert_selected(run_select(cuda, buf, off, keep, shift=out_shift, out_shift=out_shift), model, len(buf),
                    out_shift, "p = 0.5")
    # without index
    res = run_select(cuda, buf, off, keep, want_index=False)
    assert res[0] == 0 and (res[5] == M64).all() and np.array_equal(res[4][:res[1] + 1], model[1])


@pytest.mark.gpu
def test_select_capacity_and_count_only(cuda, select_stream):
    buf, off = select_stream
    n = len(off) - 1
    keep = (np.arange(n) % 3 != 0).astype(np.uint8)
    data, moff, mindex = rm.select_model(buf, off, keep)
    rc, kept, kb, whole, ooff, idx = run_select(cuda, buf, off, keep, cap=data.size - 1)
    assert rc == _native.K2H_AMD_EINVAL and (kept, kb) == (mindex.size, data.size)
    assert (whole == 0x5C).all() and (ooff == M64).all() and (idx == M64).all()
    assert_selected(run_select(cuda, buf, off, keep, cap=data.size), (data, moff, mindex), data.size, 0, "exact cap")
    rc, kept, kb, whole, ooff, idx = run_select(cuda, buf, off, keep, out=False)
    assert rc == 0 and (kept, kb) == (mindex.size, data.size)
    assert (whole == 0x5C).all() and (ooff == M64).all() and (idx == M64).all()


@pytest.mark.gpu
def test_select_drops_invalid_spans_and_keeps_tiny_blobs(cuda, oracle):
    """Kept blobs with a decreasing or overrunning span are dropped; select does not look inside
    a blob, so blobs of 0-15 bytes (pieces that span several blobs) are copied like any other."""
    buf, off = rm.stream_of(oracle, rm.records(oracle, 400, vlen=(0, 40), seed=23))
    blobs = rm.split(buf, off)
    rng = np.random.default_rng(5)
    for i in range(100, 300):
        blobs[i] = bytearray(rng.integers(0, 256, int(rng.integers(0, 16)), dtype=np.uint8).tobytes())
    buf, off = rm.join(blobs)
    n = len(off) - 1
    off[50] = off[51] + 3       # blob 50 decreasing (49 longer)
    off[n] = len(buf) + 1       # the last one past the stream
    for keep in (np.ones(n, np.uint8), (rng.random(n) < 0.6).astype(np.uint8)):
        keep[50] = keep[n - 1] = 1
        model = rm.select_model(buf, off, keep)
        assert 50 not in model[2] and n - 1 not in model[2]
        assert_selected(run_select(cuda, buf, off, keep, cap=2 * len(buf), out_shift=7), model, 2 * len(buf), 7,
                        "invalid spans")


@pytest.mark.gpu
def test_select_tiles_beyond_the_piece_table(cuda, oracle):
    """Tiles whose kept bytes outgrow the copy kernel's piece table (kSelTabPieces, read from the
    source) search the tile's prefix sums instead; here they sit next to tiles that fit, and
    one tile's kept bytes are the table's size +- one piece."""
    n = 4 * rm.SEL_TILE
    keys, vals, _s, _a = rm.records(oracle, n, seed=37)
    big = oracle.gen_bytes(6000, byte_off=41).tobytes()
    for i in range(rm.SEL_TILE, 2 * rm.SEL_TILE, 7):
        vals[i] = big[i % 900:i % 900 + 5000]
    buf, off = rm.stream_of(oracle, (keys, vals, None, None))
    spans = [off[t + rm.SEL_TILE] - off[t] for t in range(0, n, rm.SEL_TILE)]
    assert spans[1] > 16 * rm.SEL_TAB > max(spans[0], spans[2], spans[3])
    rng = np.random.default_rng(3)
    for keep in (np.ones(n, np.uint8), (rng.random(n) < 0.5).astype(np.uint8)):
        assert_selected(run_select(cuda, buf, off, keep, out_shift=11), rm.select_model(buf, off, keep), len(buf),
                        11, "large tile")
    # tile 2 padded with trailing slack to 16 * SEL_TAB - 16, + 0 and + 16 kept bytes
    blobs = rm.split(buf, off)
    for extra in (-16, 0, 16):
        padded = list(blobs)
        last = 3 * rm.SEL_TILE - 1
        padded[last] = blobs[last] + b"\x00" * (16 * rm.SEL_TAB + extra - spans[2])
        pbuf, poff = rm.join(padded)
        keep = np.ones(n, np.uint8)
        for out_shift in (0, 5):
            assert_selected(run_select(cuda, pbuf, poff, keep, out_shift=out_shift),
                            rm.select_model(pbuf, poff, keep), len(pbuf), out_shift, f"table edge {extra}")


@pytest.mark.gpu
def test_python_select_and_route_round_trip(cuda, oracle):
    """build_ralledata on the device (n = 20011, keys + values) -> check: all OK; route with
    target_max_hash = 3 over the three targets partitions the stream exactly."""
    import torch
    n = 20011
    keys, vals, _s, _a = rm.records(oracle, n, seed=29)
    dev = lambda parts: (torch.from_numpy(np.frombuffer(b"".join(parts), np.uint8).copy()).to(cuda),  # noqa: E731
                         torch.from_numpy(np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64))
                         .to(cuda))
    blobs, boff = ralledata.build_ralledata(*dev(keys), *dev(vals))
    res = ralledata.check_ralledata(blobs, boff, want_hashes=True)
    torch.cuda.synchronize()
    assert not res.status.any().item()
    koff = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64)
    r1, r2 = oracle.hash_csr(np.frombuffer(b"".join(keys), np.uint8), koff)
    assert np.array_equal(res.h1.cpu().numpy().view(np.uint64), r1)
    assert np.array_equal(res.h2.cpu().numpy().view(np.uint64), r2)
    host, hoff = blobs.cpu().numpy(), boff.cpu().numpy()
    seen = []
    for target in range(3):
        sel, chk = ralledata.route_ralledata(blobs, boff, ralledata.make_hash_range(target, 3))
        torch.cuda.synchronize()
        keep = (r1 % np.uint64(3)) == np.uint64(target)
        data, moff, mindex = rm.select_model(host, hoff, keep)
        assert (sel.kept, sel.kept_bytes) == (mindex.size, data.size)
        assert np.array_equal(sel.blobs.cpu().numpy(), data)
        assert np.array_equal(sel.blob_off.cpu().numpy().view(np.uint64), moff)
        assert np.array_equal(sel.index.cpu().numpy().view(np.uint64), mindex)
        assert np.array_equal(chk.route.cpu().numpy() & 1, keep.astype(np.uint8))
        seen.append(mindex)
    assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(n, dtype=np.uint64))
    cnt = ralledata.select_ralledata(blobs, boff, torch.ones(n, dtype=torch.bool, device=cuda), count_only=True)
    assert (cnt.kept, cnt.kept_bytes, cnt.blobs) == (n, int(hoff[-1]), None)


CORRUPTIONS = ("hash", "subhash", "klen0", "empty", "kpos", "vlen", "spos-garbage", "slack", "span-short",
               "span-decreasing")


@pytest.mark.gpu
def test_fuzz(cuda, oracle):
    """30 seeded batches: n < 1500, random segment sets and length ranges, random alignment and
    first offset, about 10 % of the blobs corrupted (span corruptions rarely: each sends its
    whole tile to the direct form); status, route and hashes against the model."""
    rng = np.random.default_rng(77)
    for it in range(30):
        n = int(rng.integers(1, 1500))
        segs = dict(klen=(1, int(rng.integers(2, 90))), vlen=(0, int(rng.integers(1, 400))),
                    slen=(0, int(rng.integers(1, 40))) if rng.integers(0, 2) else None,
                    alen=(0, int(rng.integers(1, 40))) if rng.integers(0, 2) else None)
        variant = int(rng.integers(0, 2))
        buf, off = rm.stream_of(oracle, rm.records(oracle, n, seed=1000 + it, **segs), variant=variant)
        blobs = rm.split(buf, off)
        decreasing = []
        for i in np.nonzero(rng.random(n) < 0.1)[0]:
            b = blobs[i]
            kind = CORRUPTIONS[int(rng.integers(0, 8 if rng.random() < 0.97 else len(CORRUPTIONS)))]
            if kind == "hash":
                rm.put(b, 0, rm.F_HASH, rm.get(b, 0, rm.F_HASH) ^ (1 << int(rng.integers(0, 64))))
            elif kind == "subhash":
                rm.put(b, 0, rm.F_SUBHASH, rm.get(b, 0, rm.F_SUBHASH) + 1)
            elif kind == "klen0":
                rm.put(b, 0, rm.F_KLEN, 0)
            elif kind == "empty":
                for f in (rm.F_KLEN, rm.F_VLEN, rm.F_SLEN, rm.F_ALEN):
                    rm.put(b, 0, f, 0)
            elif kind == "kpos":
                rm.put(b, 0, rm.F_KPOS, int(rng.choice([0, 79, -1, len(b), 1 << 62, 81])))
            elif kind == "vlen":
                rm.put(b, 0, rm.F_VLEN, int(rng.choice([len(b), 1 << 63, M64, rm.get(b, 0, rm.F_VLEN) + 1])))
            elif kind == "spos-garbage":
                rm.put(b, 0, rm.F_SPOS, int(rng.integers(0, 1 << 62)))  # ignored when skey_length is 0
            elif kind == "slack":
                b.extend(b"\x77" * int(rng.integers(1, 40)))
            elif kind == "span-short":
                del b[int(rng.integers(0, 80)):]
            elif i > 0:
                decreasing.append(int(i))
        buf, off = rm.join(blobs, lead=b"\x99" * int(rng.integers(0, 50)))
        size = len(buf)
        for i in decreasing:
            if i + 1 < n:
                off[i] = min(off[i + 1] + int(rng.integers(1, 9)), size)
        if it % 7 == 3:
            off[n] = size + int(rng.integers(1, 1000))
        r = list(RANGES.values())[it % len(RANGES)] if it % 3 else Range(int(rng.integers(0, 1 << 62)),
                                                                        int(rng.integers(1, 1 << 63)),
                                                                        int(rng.integers(-5, 1 << 62)),
                                                                        int(rng.integers(0, 1 << 62)),
                                                                        int(rng.integers(1, 1 << 63)))
        check_against_model(cuda, oracle, buf, off, f"batch {it} (n = {n})", shift=int(rng.integers(0, 16)), rng=r,
                            variant=variant, size=size)
