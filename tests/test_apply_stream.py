"""The `stream` argument of apply_records and apply_log (k2hash_amd/apply.py): the two scenarios
of test_unlink_stream.py -- late inputs, busy current stream -- with stream_harness.py as it is
and test_subkeys_stream.py's helpers.

Both calls synchronise `stream` to read their counts back (apply_records once for the count call
and once for the fill; apply_log also for the scan, to find the stop and in the fold).  Expected
values come from archive_apply_model.py, never from a device call.
"""
import inspect

import numpy as np
import pytest

import archive_apply_model as am
import archive_fold_model as fm
import ralle_check_model as rm
import stream_harness as sh
from archive_fold_model import Rec
from ralle_unlink_model import layout
from stream_harness import independent_streams, stall, stalled
from test_subkeys_stream import SEED_BUSY, SEED_LATE, _back, _compare, _named, _same, _to_dev, _warm

from k2hash_amd import apply, archive

NH, NK, NR, BARRIER = 300, 360, 500, 450     # held blobs, keys, records, the OW_VAL's index
KLEN, VLEN = 12, 24


def _build(oracle, seed):
    """A held stream and a log whose shapes do not depend on the seed: keys, data and which key
    a record addresses do."""
    rng = np.random.default_rng([4411, seed])
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    keys = [b"%03d-" % i + rb(KLEN - 4) for i in range(NK)]
    hs = am.hashes_of(oracle, keys)
    held, off = rm.join([layout(hs[k], k, rb(VLEN), b"", rb(5)) for k in keys[:NH]], lead=b"\x66" * 3)
    log = []
    for i in range(NR):
        k = keys[int(rng.integers(0, NK))]
        t = (fm.SET_ALL, fm.REPLACE_VAL, fm.DEL_KEY, fm.REPLACE_SKEY, fm.REPLACE_ATTRS)[i % 5]
        log.append(Rec(fm.OW_VAL, k, rb(VLEN), b"", b"", rb(8)) if i == BARRIER else
                   Rec(t, k, rb(VLEN) if t <= 1 else b"", rb(VLEN) if t == fm.REPLACE_SKEY else b"",
                       rb(VLEN) if t == fm.REPLACE_ATTRS else b""))
    file, recs = am.build_log(log)
    h1, h2 = am.rec_hashes(oracle, log)
    return dict(held=np.frombuffer(bytes(held), np.uint8).copy(), held_off=np.array(off, np.int64),
                file=np.frombuffer(file, np.uint8).copy(),
                recs=np.ascontiguousarray(recs).view(np.int64).reshape(-1, archive.REC_WORDS).copy(),
                h1=h1.view(np.int64).copy(), h2=h2.view(np.int64).copy())


def _expect(oracle, d, fold):
    recs = np.ascontiguousarray(d["recs"]).view(archive.REC_DTYPE).reshape(-1)
    log = fm.recs_of(d["file"].tobytes(), recs)
    consider = None
    if fold:
        consider = np.ones(NR, np.uint8)
        consider[:BARRIER] = fm.fold_model(log[:BARRIER])[0]
    m = am.apply_model(d["held"].tobytes(), d["held_off"], None, log, consider, d["h1"].view(np.uint64),
                       d["h2"].view(np.uint64))
    assert m.stop == BARRIER
    return dict(blobs=np.frombuffer(m.out, np.uint8), blob_off=m.out_off.view(np.int64), origin=m.origin.view(np.int64),
                touched=m.touched, counts=tuple(m.counts), stop=m.stop, first_changed=m.counts[2])


# name -> (expected outputs, the call)
CASES = {
    "apply_records": (lambda o, d: _expect(o, d, False),
                      lambda d, s: _named(apply.apply_records(d["held"], d["held_off"], d["file"], d["recs"], d["h1"], d["h2"],
                                                              stream=s))),
    "apply_log": (lambda o, d: _expect(o, d, True),
                  lambda d, s: _named(apply.apply_log(d["held"], d["held_off"], d["file"], stream=s))),
}
NAMES = list(CASES)


# ------------------------------------------------------------------------------------- CPU
def test_every_wrapper_of_the_module_has_a_case():
    found = {name for name, fn in inspect.getmembers(apply, inspect.isfunction)
             if fn.__module__ == apply.__name__ and not name.startswith("_") and "stream" in inspect.signature(fn).parameters}
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
        if k != "stop":
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
