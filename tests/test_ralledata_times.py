"""The times inside a blob's attrs (include/k2hash_amd.h section 4b'''': k2h_amd_ralledata_times;
k2h_ralle_attrs.h, k2h_ralledata_times.hip) against the model of ralle_times_model.py, entry for
entry: tflags, mtime, expire and keep.

The model's parse is pinned by tests/golden/ralle_attrs.json, which the reference's own
K2HAttrs::Serialize and find wrote (tests/golden/gen_ralle_attrs.cc); GetTime, IsExpire and the
window test on top of it are restatements of a few lines each.  Blobs are the oracle's, header
fields mutated with struct.pack_into.  Expected values never come from the device code, and every
device output is sentinel-filled first.
"""
import ctypes
import inspect
import json
import struct

import numpy as np
import pytest

from conftest import GOLDEN

import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_times_model as tm
from ralle_times_model import EXPIRE, MTIME, T_ATTRS, T_CUT, T_EXPIRE, T_MTIME, timeval

from k2hash_amd import _native, ralledata


@pytest.fixture(scope="module")
def cases():
    return json.loads((GOLDEN / "ralle_attrs.json").read_text())["cases"]


# ------------------------------------------------------------------------------------- CPU
def test_model_against_the_reference_parser(cases):
    """Every case: the entries accepted, and found / vallength / value of both keys."""
    assert 300 < len(cases) < 400
    names = {c["name"] for c in cases}
    for must in ("written-mtime", "written-expire", "written-both", "written-all-four", "count-larger",
                 "count-smaller", "dup-mtime-last-vl8", "mtime-without-nul", "mtimeX", "kl0-first", "al-0", "al-7",
                 "al-8-count-0"):
        assert must in names
    for c in cases:
        a = bytes.fromhex(c["attrs"])
        got, _cut = tm.parse_attrs(a)
        assert len(got) == c["accepted"], c["name"]
        for key, name in ((MTIME, "mtime"), (EXPIRE, "expire")):
            w = c[name]
            assert (key in got) == w["found"], c["name"]
            if w["found"]:
                assert len(got[key]) == w["vallength"] and got[key].hex() == w["value"], c["name"]
            t = tm.get_time(a, key)
            assert (t is not None) == (w["found"] and w["vallength"] == 16), c["name"]
            if t is not None:
                assert struct.pack("<qq", *t).hex() == w["value"], c["name"]


def test_every_cut_of_the_written_attrs_is_in_the_fixture(cases):
    by_name = {c["name"]: c for c in cases}
    for which in ("mtime", "expire", "both", "all-four"):
        whole = by_name[f"written-{which}"]["attrs"]
        for cut in range(len(whole) // 2):
            assert by_name[f"written-{which}-cut-{cut}"]["attrs"] == whole[:2 * cut]
    assert tm.written_attrs([(MTIME, timeval(1700000000, 123456789)), (EXPIRE, timeval(1700000600, 5))]).hex() == \
        by_name["written-both"]["attrs"]                  # the model writes what the reference writes


def test_cut_flag_of_the_model():
    both = tm.written_attrs([(MTIME, timeval(5, 6)), (EXPIRE, timeval(7, 8))])
    assert tm.parse_attrs(both) == ({MTIME: timeval(5, 6), EXPIRE: timeval(7, 8)}, False)
    assert tm.parse_attrs(both[:-1])[1] and tm.parse_attrs(both[:8])[1] and tm.parse_attrs(both[:7])[1]
    assert tm.parse_attrs(b"") == ({}, False)
    assert tm.parse_attrs(both + b"\0" * 9)[1] is False
    assert tm.parse_attrs(tm.serialize_attrs([(MTIME, timeval(5, 6))], count=2))[1]
    assert tm.parse_attrs(tm.serialize_attrs([(MTIME, timeval(5, 6)), (EXPIRE, b"")], count=1)) == \
        ({MTIME: timeval(5, 6)}, False)


def _host_stream(oracle):
    buf, off = rm.stream_of(oracle, rm.records(oracle, 4, seed=1))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64)


def test_times_argument_validation(oracle):
    """Judged on the host before any device is touched: the same answers with and without a
    GPU, each with its own message."""
    lib = _native.batch_lib()
    buf, off = _host_stream(oracle)
    n = off.size - 1
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    flags, keep = np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
    times = lib.k2h_amd_ralledata_times
    msg = lambda: bytes(lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL))  # noqa: E731
    win = tm.Window(start=(1, 2)).ctypes()
    assert win.flags == 1 and (win.start.sec, win.start.nsec) == (1, 2)
    w = ctypes.byref(win)
    assert times(None, 0, None, 0, None, None, None, p(flags), None, None, None, None) == _native.K2H_AMD_OK
    assert times(None, 0, None, 0, None, w, None, None, None, None, p(keep), None) == _native.K2H_AMD_OK
    texts = set()
    for args, text in (
            ((p(buf), buf.size, p(off), n, None, w, None, None, None, None, None, None), b"all NULL"),
            ((p(buf), buf.size, p(off), n, None, None, p(keep), None, None, None, p(keep), None), b"without window"),
            ((None, buf.size, p(off), n, None, None, None, p(flags), None, None, None, None), b"NULL blobs"),
            ((p(buf), buf.size, None, n, None, None, None, None, None, None, p(keep), None), b"NULL blob_off")):
        assert times(*args) == _native.K2H_AMD_EINVAL
        assert text in msg()
        texts.add(msg())
    win.flags = 8
    assert times(p(buf), buf.size, p(off), n, None, w, None, p(flags), None, None, None, None) == _native.K2H_AMD_EINVAL
    assert b"unknown window flag" in msg()
    texts.add(msg())
    assert len(texts) == 5 and all(b"ralledata_times: " in t for t in texts)
    assert (flags == 0xEE).all() and (keep == 0xEE).all()


def test_times_public_names():
    import k2hash_amd
    for name in ("blob_times", "TimeWindow", "Times"):
        assert hasattr(k2hash_amd, name) and name in k2hash_amd.__all__
    header = (rm.ROOT / "include" / "k2hash_amd.h").read_text()
    for name in ("k2h_amd_ralledata_times", "k2h_amd_ralledata_dedup_mtime", "k2h_amd_timespec",
                 "k2h_amd_time_window", "K2H_AMD_WIN_START", "K2H_AMD_WIN_END", "K2H_AMD_WIN_EXPIRE",
                 "K2H_AMD_TIMES_MTIME", "K2H_AMD_TIMES_EXPIRE", "K2H_AMD_TIMES_CUT", "K2H_AMD_TIMES_ATTRS"):
        assert name in header, name
    lib = _native.batch_lib()
    assert lib.k2h_amd_ralledata_times and lib.k2h_amd_ralledata_dedup_mtime
    assert len(_native.SIGNATURES["k2h_amd_ralledata_times"][1]) == 12
    assert len(_native.SIGNATURES["k2h_amd_ralledata_dedup_mtime"][1]) == 10
    assert ctypes.sizeof(_native.Timespec) == 16 and ctypes.sizeof(_native.TimeWindowStruct) == 56
    assert (ralledata.TIMES_MTIME, ralledata.TIMES_EXPIRE, ralledata.TIMES_CUT, ralledata.TIMES_ATTRS) == \
        (T_MTIME, T_EXPIRE, T_CUT, T_ATTRS)
    w = ralledata.TimeWindow(end=(3, 4), now=(-5, 6)).ctypes()
    assert w.flags == 6 and (w.end.sec, w.end.nsec, w.now.sec, w.now.nsec) == (3, 4, -5, 6)
    for fn, names in ((ralledata.dedup_ralledata, ("pts",)), (ralledata.route_ralledata, ("window", "pts")),
                      (ralledata.blob_times, ("consider", "window", "route", "stream"))):
        for nm in names:
            assert inspect.signature(fn).parameters[nm].default is None


# ---- the streams of the GPU tests, and (CPU) that each is what its test claims
def _case_blob(oracle, attrs, key=b"key", val=b"value"):
    return dm.blobs_of(oracle, [key], [val], None, [attrs])[0]


def _aligned_stream(oracle, cases):
    """Every case 16 times, with keys of 1 to 16 bytes and slack behind each blob that brings the
    next blob to a 16-byte boundary: each case's attrs segment starts at every alignment."""
    keys, vals, attrs = [], [], []
    for c in cases:
        for kl in range(1, 17):
            keys.append(b"K" * kl)
            vals.append(b"val")
            attrs.append(bytes.fromhex(c["attrs"]))
    blobs = [bytearray(b) + bytes(-len(b) % 16) for b in dm.blobs_of(oracle, keys, vals, None, attrs)]
    return rm.join(blobs)


def test_aligned_stream_covers_every_alignment(oracle, cases):
    buf, off = _aligned_stream(oracle, cases[:3] + cases[-3:])
    for c in range(6):
        if not rm.get(buf, off[16 * c], rm.F_ALEN):
            continue
        at = {(off[16 * c + r] + rm.get(buf, off[16 * c + r], rm.F_APOS)) % 16 for r in range(16)}
        assert at == set(range(16))


def _attrs_before_key(blob):
    """The same element with its attrs placed before its key and value."""
    f = struct.unpack_from("<10Q", blob, 0)
    seg = lambda s: bytes(blob[f[6 + s]:f[6 + s] + f[2 + s]])  # noqa: E731
    key, val, attrs = seg(0), seg(1), seg(3)
    out = bytearray(blob[:80]) + attrs + key + val
    rm.put(out, 0, rm.F_APOS, 80)
    rm.put(out, 0, rm.F_KPOS, 80 + len(attrs))
    rm.put(out, 0, rm.F_VPOS, 80 + len(attrs) + len(key))
    return out


def _crafted():
    """Entries whose lengths would make 16 + kl + vl wrap; behind each a good mtime entry that a
    walk which went on (to pos + the wrapped sum) would find."""
    good = struct.pack("<QQ", 6, 16) + MTIME + timeval(77, 88)
    out = {}
    # kl = 2^64 - 8: 16 + kl + 16 wraps to 24
    out["kl-huge"] = struct.pack("<QQQ", 2, (1 << 64) - 8, 16) + bytes(8) + good + good
    # kl = 6, vl = 2^64 - 6: 16 + kl + vl wraps to 16
    out["vl-huge"] = struct.pack("<QQQ", 2, 6, (1 << 64) - 6) + good + good
    # kl + vl alone wraps
    out["both-huge"] = struct.pack("<QQQ", 3, 1 << 63, 1 << 63) + good + good
    return out


def test_crafted_lengths_model():
    for name, a in _crafted().items():
        assert tm.parse_attrs(a) == ({}, True), name


def _planted_stream(oracle, cases, n, seed):
    """n blobs with fixture attrs; every fifth is a non-participant of some kind."""
    rng = np.random.default_rng(seed)
    pick = [cases[int(i)] for i in rng.integers(0, len(cases), n)]
    blobs = dm.blobs_of(oracle, [b"key-%d" % i for i in range(n)], [b"v" * int(rng.integers(0, 9)) for _ in range(n)],
                        None, [bytes.fromhex(c["attrs"]) for c in pick])
    consider = np.ones(n, np.uint8)
    for i in range(0, n, 5):
        kind = (i // 5) % 5
        if kind == 0:
            blobs[i] = blobs[i][:79]
        elif kind == 1:
            for f in (rm.F_KLEN, rm.F_VLEN, rm.F_ALEN):
                rm.put(blobs[i], 0, f, 0)
        elif kind == 2:
            rm.put(blobs[i], 0, rm.F_KLEN, 0)
        elif kind == 3:
            rm.put(blobs[i], 0, rm.F_APOS if rm.get(blobs[i], 0, rm.F_ALEN) else rm.F_KPOS, 79)
        else:
            consider[i] = 0
    return rm.join(dm.at_odd_offsets(blobs, seed)), consider


def test_planted_stream_model(oracle, cases):
    (buf, off), consider = _planted_stream(oracle, cases, 65, 1)
    flags, mtime, expire, keep = tm.times_model(buf, off, consider=consider)
    assert not keep[::5].any() and not flags[::5].any() and not mtime[::5].any() and keep.sum() == 65 - 13
    assert (flags & T_MTIME).any() and (flags & T_CUT).any() and (flags & T_EXPIRE).any()


def _fuzz_attrs(rng):
    keys = (MTIME, EXPIRE, b"mtime", b"expire", b"mtimeX\0", b"expirE\0", b"uniqid\0", b"", b"\0" * 6,
            bytes(rng.integers(0, 256, int(rng.integers(1, 30)), dtype=np.uint8)))
    n = int(rng.integers(0, 7))
    entries = []
    for _ in range(n):
        k = keys[int(rng.integers(0, len(keys)))]
        if k in (MTIME, EXPIRE):
            vl = (16, 16, 16, 16, 8, 0, 17)[int(rng.integers(0, 7))]
        else:
            vl = int(rng.integers(0, 40))
        entries.append((k, bytes(rng.integers(0, 256, vl, dtype=np.uint8))))
    u = rng.random()
    a = tm.serialize_attrs(entries, count=None if u < 0.7 else int(rng.integers(0, 9)) if u < 0.95 else (1 << 64) - 1)
    v = rng.random()
    if v < 0.2:
        a = a[:int(rng.integers(0, len(a) + 1))]
    elif v < 0.3:
        a += bytes(rng.integers(0, 256, int(rng.integers(1, 20)), dtype=np.uint8))
    elif v < 0.35 and len(a) > 24:
        a = bytearray(a)
        struct.pack_into("<Q", a, 8 * int(rng.integers(1, 3)), int(rng.integers(0, 1 << 63)) * 2 + 1)
        a = bytes(a)
    return a


def _fuzz_stream(oracle, seed, n=2000):
    rng = np.random.default_rng(700 + seed)
    keys = [bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8)) for _ in range(n)]
    vals = [bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8)) for _ in range(n)]
    attrs = [_fuzz_attrs(rng) for _ in range(n)]
    consider = (rng.random(n) < 0.9).astype(np.uint8)
    route = rng.integers(0, 4, n).astype(np.uint8)
    return rm.join(dm.at_odd_offsets(dm.blobs_of(oracle, keys, vals, None, attrs), seed)), consider, route


def test_fuzz_stream_reaches_every_flag(oracle):
    (buf, off), consider, _route = _fuzz_stream(oracle, 0, n=600)
    flags = tm.times_model(buf, off, consider=consider)[0]
    seen = {int(f) for f in flags}
    assert {0, T_ATTRS, T_ATTRS | T_MTIME, T_ATTRS | T_EXPIRE, T_ATTRS | T_CUT} <= seen
    assert any(f & T_CUT and f & (T_MTIME | T_EXPIRE) for f in seen)


START, END, NOWT = (1000, 500), (2000, 700), (1500, 250)
_MTIMES = (None, (999, 999), (1000, 499), (1000, 500), (1000, 501), (1001, 0), (1999, 800), (2000, 699), (2000, 700),
           (2000, 701), (2001, 0), (-5, 3), (1000, -1))
_EXPIRES = (None, (1499, 999), (1500, 249), (1500, 250), (1500, 251), (1501, 0), (-1, 0))
NEG_START, NEG_END, NEG_NOW = (-10, 5), (-3, -2), (-4, 0)
_NEG_MTIMES = ((-11, 9), (-10, 4), (-10, 5), (-10, 6), (-3, -3), (-3, -2), (-3, -1), (-2, 0), (0, 0))
_NEG_EXPIRES = (None, (-5, 9), (-4, -1), (-4, 0), (-4, 1), (-3, 0))


def _window_stream(oracle, mtimes, expires):
    attrs = []
    for m in mtimes:
        for e in expires:
            entries = ([(MTIME, timeval(*m))] if m else []) + ([(EXPIRE, timeval(*e))] if e else [])
            attrs.append(tm.written_attrs(entries) if entries else b"")
    n = len(attrs)
    return rm.join(dm.blobs_of(oracle, [b"w%03d" % i for i in range(n)], [b"v"] * n, None, attrs))


def _windows(start, end, now):
    return [tm.Window(start if b & 1 else None, end if b & 2 else None, now if b & 4 else None) for b in range(8)]


def _routes(n):
    mixed = np.random.default_rng(3).integers(0, 4, n).astype(np.uint8)
    return {"null": None, "zeros": np.zeros(n, np.uint8), "old": np.full(n, 2, np.uint8), "mixed": mixed}


def test_window_model_pins_each_strict_compare(oracle):
    """On each side of start, end and now, in sec and in nsec: the model's keep changes exactly
    where the reference's compares say."""
    buf, off = _window_stream(oracle, _MTIMES, _EXPIRES)
    ne = len(_EXPIRES)
    keep = {b: tm.times_model(buf, off, window=w)[3].reshape(len(_MTIMES), ne)
            for b, w in enumerate(_windows(START, END, NOWT))}
    col = {m: i for i, m in enumerate(_MTIMES)}
    assert keep[0].all()
    assert keep[1][:, 0].tolist() == [m is None or not m < START for m in _MTIMES]
    assert not keep[1][col[(1000, 499)], 0] and keep[1][col[(1000, 500)], 0] and not keep[1][col[(999, 999)], 0]
    assert keep[2][:, 0].tolist() == [m is None or not END < m for m in _MTIMES]
    assert keep[2][col[(2000, 700)], 0] and not keep[2][col[(2000, 701)], 0] and not keep[2][col[(2001, 0)], 0]
    assert keep[4][0].tolist() == [e is None or not e < NOWT for e in _EXPIRES]
    assert keep[4][0].tolist() == [1, 0, 0, 1, 1, 1, 0]
    # a blob outside the old range is not held to start
    zeros = tm.times_model(buf, off, window=_windows(START, END, NOWT)[1], route=np.zeros(len(off) - 1, np.uint8))[3]
    assert zeros.all()


# ------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_every_fixture_case_alone_at_the_buffers_end(cuda, oracle, cases):
    """n = 1; the attrs segment is the blob's last and the tensor ends with it (size exact)."""
    for c in cases:
        a = bytes.fromhex(c["attrs"])
        blob = _case_blob(oracle, a)
        if a:
            assert rm.get(blob, 0, rm.F_APOS) + len(a) == len(blob)
        flags, mtime, _e, _k = tm.times_against_model(cuda, blob, [0, len(blob)], c["name"], shift=len(a) % 16,
                                                      tail_pad=0)
        assert bool(flags[0] & T_MTIME) == (c["mtime"]["found"] and c["mtime"]["vallength"] == 16), c["name"]
        if flags[0] & T_MTIME:
            assert struct.pack("<qq", *mtime[0]).hex() == c["mtime"]["value"]


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 5])
def test_every_fixture_case_at_every_alignment(cuda, oracle, cases, shift):
    buf, off = _aligned_stream(oracle, cases)
    tm.times_against_model(cuda, buf, off, f"aligned, shift {shift}", shift=shift, tail_pad=0)


@pytest.mark.gpu
def test_attrs_before_the_key(cuda, oracle, cases):
    blobs = [_attrs_before_key(_case_blob(oracle, bytes.fromhex(c["attrs"]), key=b"k" * (1 + i % 16)))
             for i, c in enumerate(cases) if c["attrs"]]
    buf, off = rm.join(blobs)
    flags = tm.times_against_model(cuda, buf, off, "attrs first", shift=3)[0]
    assert (flags & T_MTIME).any() and (flags & T_CUT).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_crafted()))
def test_crafted_lengths_are_cut(cuda, oracle, name):
    blob = _case_blob(oracle, _crafted()[name])
    flags, mtime, expire, keep = tm.times_against_model(cuda, blob, [0, len(blob)], name, shift=9, tail_pad=0)
    assert flags[0] == T_ATTRS | T_CUT and not mtime.any() and keep[0] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_participants_and_others(cuda, oracle, cases, n):
    (buf, off), consider = _planted_stream(oracle, cases, n, n)
    tm.times_against_model(cuda, buf, off, f"planted {n}", shift=n % 16, consider=consider,
                           window=tm.Window(START, END, NOWT))
    tm.times_against_model(cuda, buf, off, f"planted {n}, all considered", shift=n % 16)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fuzz(cuda, oracle, seed):
    (buf, off), consider, route = _fuzz_stream(oracle, seed)
    flags = tm.times_against_model(cuda, buf, off, f"fuzz {seed}", shift=seed, consider=consider,
                                   window=tm.Window((100, 0), (1 << 62, 0), (0, 0)), route=route)[0]
    assert (flags & T_CUT).sum() > 100 and (flags & T_MTIME).sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["positive", "negative"])
def test_window_flags_and_routes(cuda, oracle, which):
    """Every flag combination under every kind of route, on times equal to start, end and now
    and one step to either side in sec and in nsec."""
    if which == "positive":
        (buf, off), wins = _window_stream(oracle, _MTIMES, _EXPIRES), _windows(START, END, NOWT)
    else:
        (buf, off), wins = _window_stream(oracle, _NEG_MTIMES, _NEG_EXPIRES), _windows(NEG_START, NEG_END, NEG_NOW)
    t = tm.place(cuda, buf, 7)
    kept = set()
    for b, w in enumerate(wins):
        for rname, route in _routes(len(off) - 1).items():
            if b == 0 and route is not None:
                w = tm.Window()           # no flags, but a window: route is allowed
            want = tm.times_model(buf, off, window=w, route=route)
            got = tm.run_times(cuda, t, len(buf), off, None, w, route)
            tm.assert_times(got, want, f"{which} flags {b} route {rname}")
            kept.add(int(want[3].sum()))
    assert len(kept) > 8
    want = tm.times_model(buf, off)
    tm.assert_times(tm.run_times(cuda, t, len(buf), off), want, "no window")
    assert want[3].all()


@pytest.mark.gpu
def test_only_the_outputs_asked_for(cuda, oracle, cases):
    """Each output alone: the three NULL ones are not touched."""
    import torch
    import big_offsets as bo
    (buf, off), consider = _planted_stream(oracle, cases, 70, 4)
    want = tm.times_model(buf, off, window=tm.Window(START, END, NOWT))
    t = tm.place(cuda, buf)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    win = tm.Window(START, END, NOWT).ctypes()
    n = len(off) - 1
    for k in range(4):
        byte_out = lambda: torch.full((n,), 0xEE, dtype=torch.uint8, device=cuda)  # noqa: E731
        word_out = lambda: torch.full((2 * n,), 7, dtype=torch.int64, device=cuda)  # noqa: E731
        outs = [byte_out(), word_out(), word_out(), byte_out()]
        ptrs = [bo._p(o) if i == k else None for i, o in enumerate(outs)]
        _native.check(_native.batch_lib().k2h_amd_ralledata_times(bo._p(t), len(buf), bo._p(d_off), n, None,
                                                                 ctypes.byref(win), None, *ptrs, bo._stream()))
        torch.cuda.synchronize()
        assert (outs[k].cpu().numpy().reshape(want[k].shape) == want[k]).all()


@pytest.mark.gpu
def test_blob_times_wrapper(cuda, oracle, cases):
    import torch
    (buf, off), consider = _planted_stream(oracle, cases, 130, 9)
    t = tm.place(cuda, buf, 2)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    route = np.random.default_rng(5).integers(0, 4, 130).astype(np.uint8)
    for kw, mkw in (({}, {}),
                    ({"consider": torch.from_numpy(consider).to(cuda)}, {"consider": consider}),
                    ({"window": ralledata.TimeWindow(START, END, NOWT), "route": torch.from_numpy(route).to(cuda)},
                     {"window": tm.Window(START, END, NOWT), "route": route})):
        res = ralledata.blob_times(t, d_off, **kw)
        torch.cuda.synchronize()
        got = (res.flags.cpu().numpy(), res.mtime.cpu().numpy(), res.expire.cpu().numpy(), res.keep.cpu().numpy())
        tm.assert_times(got, tm.times_model(buf, off, **mkw), f"wrapper {sorted(kw)}")
    with pytest.raises(ValueError):
        ralledata.blob_times(t, d_off, route=torch.from_numpy(route).to(cuda))
