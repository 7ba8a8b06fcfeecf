"""k2h_amd_hash_ranges (k2h_ranges.hip: gather -> CSR kernels -> cstr_fixup_kernel), every key of
every case against the oracle, over {CSTR} x {STD_FNV} x {h2 asked for or not}.

second=False with cstr=True runs the fixup with h2 == NULL; the all-empty call runs over the
16-byte dummy buffer (total == 0) and, with CSTR, must give seed * P of the *chosen* seed (the
oracle's hash of b"\\0").  The base buffer starts 0, 1 or 15 bytes into its allocation between
canary bytes that differ between two runs.  Outputs are sentinel-filled before the call.
"""
import ctypes

import numpy as np
import pytest

import csr_scenarios as cs

from k2hash_amd import _native, archive

SIZE = 50021  # bytes of the base buffer (odd: its last byte is at no aligned place)


def _staged():
    rng = np.random.default_rng(31)
    lens = rng.integers(0, 121, 3000)
    lens[::13] = 0
    return rng.integers(0, SIZE - 120, 3000), lens


def _oversize():
    rng = np.random.default_rng(32)
    return rng.integers(0, SIZE - 400, 600), rng.integers(150, 401, 600)


def _all_empty():
    return np.random.default_rng(33).integers(0, SIZE + 1, 1000), np.zeros(1000, np.int64)


def _overlap():
    """Identical ranges, nested ones, and chains that overlap their neighbour by all but one byte."""
    s = [100] * 40 + list(range(200, 260)) + [300 + i for i in range(50)] + [1000] * 3
    n = [77] * 40 + [90] * 60 + [100 - 2 * i for i in range(50)] + [400, 400, 150]
    return np.array(s), np.array(n)


def _edges():
    """Ranges that start at byte 0 and less than 16 bytes into the buffer with every pad
    p = 0..15 (lengths 1..32), ranges that end at the buffer's last byte, and the whole buffer."""
    s, n = [], []
    for start in range(16):
        for length in range(0, 33):
            s.append(start)
            n.append(length)
    for length in list(range(0, 41)) + [150, 4096]:
        s.append(SIZE - length)
        n.append(length)
    s.append(0)
    n.append(SIZE)
    return np.array(s), np.array(n)


CASES = {"staged": _staged, "oversize": _oversize, "all-empty": _all_empty, "overlap": _overlap, "edges": _edges}


def test_cases_reach_what_they_are_for():
    s, n = _staged()
    assert n.max() == 120 and (n == 0).any() and all(t["staged"] for t in cs.tile_model(n, 0, 0))
    s, n = _oversize()
    assert n.size == 600 and 150 <= n.min() and n.max() <= 400 and not cs.tile_model(n, 0, 0)[0]["staged"]
    s, n = _all_empty()
    assert n.size == 1000 and not n.any()
    s, n = _overlap()
    assert len(set(zip(s.tolist(), n.tolist()))) < s.size  # identical ranges
    assert ((s[1:] < (s + n)[:-1]) & (s[1:] > s[:-1])).any()  # overlapping neighbours
    s, n = _edges()
    near = s < 16
    assert {(int(a), int(-b % 16)) for a, b in zip(s[near], n[near]) if b} == {(a, p) for a in range(16) for p in range(16)}
    assert ((s == 0) & (n > 0)).any() and ((s + n == SIZE) & (n > 0)).sum() > 16
    for f in CASES.values():
        s, n = f()
        assert (s >= 0).all() and (s + n <= SIZE).all()


def hash_ranges(cuda, base, starts, lens, second, cstr, std):
    """archive.hash_ranges into sentinel-filled outputs; host uint64 arrays by name."""
    import torch

    from k2hash_amd.batch import _dev_ptr, _stream_handle
    n = starts.size
    d_s, d_n = torch.from_numpy(starts.astype(np.int64)).to(cuda), torch.from_numpy(lens.astype(np.int64)).to(cuda)
    full, o = cs.sentinel_outs(torch, cuda, n, ("h1", "h2") if second else ("h1",))
    flags = (archive.FLAG_CSTR if cstr else 0) | (archive.FLAG_STD_FNV if std else 0)
    _native.check(_native.batch_lib().k2h_amd_hash_ranges(
        ctypes.c_void_p(base.data_ptr()), _dev_ptr(d_s), _dev_ptr(d_n), n, _dev_ptr(o["h1"]),
        _dev_ptr(o["h2"]) if second else None, flags, _stream_handle()))
    return cs.collect(torch, full, n)


@pytest.mark.gpu
@pytest.mark.parametrize("second", [False, True], ids=["h1", "h1h2"])
@pytest.mark.parametrize("std", [False, True], ids=["builtin", "std"])
@pytest.mark.parametrize("cstr", [False, True], ids=["raw", "cstr"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_hash_ranges(cuda, oracle, case, cstr, std, second):
    starts, lens = CASES[case]()
    payload = oracle.gen_bytes(SIZE, byte_off=77)
    nul = np.zeros(1, np.uint8)
    parts = [payload[s:s + n] for s, n in zip(starts.tolist(), lens.tolist())]
    if cstr:
        parts = [np.concatenate([p, nul]) for p in parts]
    off = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    r1, r2 = oracle.hash_csr(np.concatenate(parts + [nul]), off, variant=int(std))
    if case == "all-empty":  # 0 without CSTR; with it what the oracle gives for b"\0" under this seed
        one = (oracle.k2h_hash(b"\0", int(std)), oracle.k2h_second_hash(b"\0", int(std))) if cstr else (0, 0)
        assert one[0] == one[1] and (r1 == one[0]).all() and (r2 == one[1]).all()
        assert not cstr or one[0] != oracle.k2h_hash(b"\0", 1 - int(std))
    want = {"h1": r1, "h2": r2} if second else {"h1": r1}
    for shift, canary in zip((0, 1, 15, 0), cs.CANARIES * 2):
        base = cs.place(cuda, payload, shift, canary)
        got = hash_ranges(cuda, base, starts, lens, second, cstr, std)
        cs.assert_equal(got, want, (case, cstr, std, second, shift, hex(canary)))
