"""The `stream` argument of k2hash_amd/find.py's wrappers: the two scenarios of
test_apply_stream.py -- late inputs, busy current stream -- with stream_harness.py as it is and
test_subkeys_stream.py's helpers.

index_stream and find_keys synchronise `stream` only to read their counts back; fetch_segments
and get_values once per library call for the total.  The index is opaque, so index_stream is
judged by its participants and, in the find_keys case, by what is found through it.  Expected
values come from ralle_find_model.py, never from a device call.
"""
import inspect

import numpy as np
import pytest

import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_find_model as fm
import stream_harness as sh
from stream_harness import independent_streams, stall, stalled
from test_subkeys_stream import SEED_BUSY, SEED_LATE, _back, _compare, _same, _to_dev, _warm

from k2hash_amd import find

N, M, KLEN, VLEN = 300, 240, 12, 24
NOW = (1500, 0)


def _build(oracle, seed):
    """A stream, a consider mask, queries and slots whose shapes do not depend on the seed: the
    keys, the values, which keys are asked for and which slots are empty or out of range do."""
    rng = np.random.default_rng([7710, seed])
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    keys = [b"%03d-" % i + rb(KLEN - 4) for i in range(N)]
    keys[N - 1] = keys[3]                                              # a later copy
    buf, off = rm.join(dm.blobs_of(oracle, keys, [rb(VLEN) for _ in range(N)], None, None), lead=b"\x66" * 5)
    consider = (rng.random(N) < 0.9).astype(np.uint8)
    asked = [keys[int(i)] if rng.random() < 0.6 else b"no--" + rb(KLEN - 4) for i in rng.integers(0, N, M)]
    data, koff = fm.csr(asked)
    h1, h2 = fm.hashes_of(oracle, asked)
    which = rng.integers(0, N, M).astype(np.int64)
    which[rng.random(M) < 0.1] = -1
    which[rng.random(M) < 0.05] = N + 2
    return dict(blobs=np.frombuffer(bytes(buf), np.uint8).copy(), blob_off=np.array(off, np.int64), consider=consider,
                keys=np.frombuffer(data, np.uint8).copy(), key_off=koff.astype(np.int64), h1=h1.view(np.int64).copy(),
                h2=h2.view(np.int64).copy(), which=which)


def _found(d):
    return fm.find_model(d["blobs"].tobytes(), d["blob_off"], d["keys"].tobytes(), d["key_off"], d["h1"].view(np.uint64),
                         d["h2"].view(np.uint64), now=NOW, consider=d["consider"])


def _expect_index(o, d):
    return dict(participants=len(fm.participants(d["blobs"].tobytes(), d["blob_off"], consider=d["consider"])))


def _expect_find(o, d):
    match, status, hit, counts = _found(d)
    return dict(match=match.view(np.int64), status=status, hit=hit, counts=tuple(counts))


def _expect_fetch(o, d):
    out, ooff, bad = fm.fetch_model(d["blobs"].tobytes(), d["blob_off"], d["which"], "value")
    return dict(out=np.frombuffer(out, np.uint8), out_off=ooff.view(np.int64), bad=bad)


def _expect_get(o, d):
    match, status, _hit, _counts = _found(d)
    take = [(int(x) & (fm.FOUND | fm.EXPIRED)) == fm.FOUND for x in status]
    out, ooff, _bad = fm.fetch_model(d["blobs"].tobytes(), d["blob_off"], match, "value", take)
    return dict(values=np.frombuffer(out, np.uint8), value_off=ooff.view(np.int64), status=status)


def _run_index(d, s):
    return dict(participants=find.index_stream(d["blobs"], d["blob_off"], consider=d["consider"], stream=s).participants)


def _run_find(d, s):
    ix = find.index_stream(d["blobs"], d["blob_off"], consider=d["consider"], count=False, stream=s)
    f = find.find_keys(d["blobs"], d["blob_off"], ix, d["keys"], d["key_off"], now=NOW, want_hit=True, stream=s)
    return dict(match=f.match, status=f.status, hit=f.hit, counts=tuple(f.counts))


def _run_fetch(d, s):
    out, out_off, bad = find.fetch_segments(d["blobs"], d["blob_off"], d["which"], "value", want_bad=True, stream=s)
    return dict(out=out, out_off=out_off, bad=bad)


def _run_get(d, s):
    ix = find.index_stream(d["blobs"], d["blob_off"], consider=d["consider"], count=False, stream=s)
    values, value_off, status = find.get_values(d["blobs"], d["blob_off"], ix, d["keys"], d["key_off"], now=NOW, h1=d["h1"],
                                                h2=d["h2"], stream=s)
    return dict(values=values, value_off=value_off, status=status)


# name -> (expected outputs, the call)
CASES = {"index_stream": (_expect_index, _run_index), "find_keys": (_expect_find, _run_find),
         "fetch_segments": (_expect_fetch, _run_fetch), "get_values": (_expect_get, _run_get)}
NAMES = list(CASES)


# ------------------------------------------------------------------------------------- CPU
def test_every_wrapper_of_the_module_has_a_case():
    found = {name for name, fn in inspect.getmembers(find, inspect.isfunction)
             if fn.__module__ == find.__name__ and not name.startswith("_") and "stream" in inspect.signature(fn).parameters}
    assert found == set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_decoy_has_the_shapes_and_another_answer(oracle, name):
    expect, _run = CASES[name]
    real, decoy = _build(oracle, SEED_LATE), _build(oracle, -SEED_LATE % 97)
    for k, v in real.items():
        assert decoy[k].shape == v.shape and decoy[k].dtype == v.dtype, k
    want, other = expect(oracle, real), expect(oracle, decoy)
    assert set(want) == set(other)
    for k in want:
        assert not _same(other[k], want[k]), f"{name}: the decoy's {k} equals the real one"


# ------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_late_inputs(cuda, oracle, name):
    """The inputs arrive on `stream` behind a stall, over a decoy; another, idle stream is
    current.  Whatever the call issues off `stream` runs at once, on the decoy."""
    import torch
    expect, run = CASES[name]
    c, s = independent_streams(cuda)
    real, decoy = _build(oracle, SEED_LATE), _build(oracle, -SEED_LATE % 97)
    want = expect(oracle, real)
    _warm(torch, run, _to_dev(torch, cuda, decoy), c, s)
    dev, staged = _to_dev(torch, cuda, decoy), _to_dev(torch, cuda, real)
    torch.cuda.synchronize()
    ev = stall(s)
    with torch.cuda.stream(s):
        for k, v in staged.items():
            dev[k].copy_(v)
    assert stalled(ev), "the stall was over before the call was made"
    out = {}
    with torch.cuda.stream(c):
        ms = sh.host_ms(lambda: out.update(run(dev, s)))
    print(f"{name}: host {ms:.3f} ms (synchronises)")
    _compare(name, _back(torch, out, s), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_busy_current_stream(cuda, oracle, name):
    """The current stream is stalled, the call names another: the results reach the host
    through `stream` while the current one is still stalled, so the call neither waited for the
    current stream nor left work on it."""
    import torch
    expect, run = CASES[name]
    c, s = independent_streams(cuda)
    real, decoy = _build(oracle, SEED_BUSY), _build(oracle, -SEED_BUSY % 97)
    want = expect(oracle, real)
    _warm(torch, run, _to_dev(torch, cuda, decoy), c, s)
    dev = _to_dev(torch, cuda, real)
    with torch.cuda.stream(c):          # what the current stream's pool hands out next holds 0x5A, not an earlier answer
        junk = [torch.full((512,), 0x5A, dtype=torch.uint8, device=cuda) for _ in range(64)]
        junk.append(torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=cuda))
    torch.cuda.synchronize()
    del junk
    with torch.cuda.stream(c):
        ev = stall(c)
        out = {}
        ms = sh.host_ms(lambda: out.update(run(dev, s)))
    got = _back(torch, out, s)
    still = stalled(ev)
    print(f"{name}: host {ms:.3f} ms")
    assert still, f"{name}: the current stream's stall was over when the results arrived (call: {ms:.2f} ms on the host)"
    _compare(name, got, want)
    del out
