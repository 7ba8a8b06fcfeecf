"""The `stream` argument of delta_records and delta_log (k2hash_amd/delta.py): the two scenarios
of test_apply_stream.py -- late inputs, busy current stream -- with stream_harness.py as it is and
test_subkeys_stream.py's helpers.

Both calls synchronise `stream` to read their counts back (delta_records once for the count call
and once for the fill; delta_log also in the two count-only applies of its reduction).  Expected
values come from ralle_delta_model.py, never from a device call.
"""
import inspect

import numpy as np
import pytest

import archive_apply_model as am
import ralle_check_model as rm
import ralle_delta_model as dl
import ralle_diff_model as df
import stream_harness as sh
from ralle_unlink_model import layout
from stream_harness import independent_streams, stall, stalled
from test_subkeys_stream import SEED_BUSY, SEED_LATE, _back, _compare, _named, _same, _to_dev, _warm

from k2hash_amd import delta

NK, NH, N0, DUP = 360, 300, 40, 30     # keys; held blobs: keys [0, NH); new blobs: keys [N0, NK), then DUP second copies
KLEN, VLEN = 12, 24


def _build(oracle, seed):
    """A held and a new stream whose shapes do not depend on the seed: keys, data and which
    fields of which key changed do.  rel and seen are ralle_diff_model's over the two as they
    are (delta_records takes them as inputs; delta_log makes its own over the reduced streams)."""
    rng = np.random.default_rng([5511, seed])
    rb = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()  # noqa: E731
    keys = [b"%03d-" % i + rb(KLEN - 4) for i in range(NK)]
    hs = am.hashes_of(oracle, keys)
    was = {k: (rb(VLEN), rb(7), rb(5)) for k in keys[:NH]}
    change = lambda k: tuple(rb(len(x)) if rng.random() < 0.25 else x for x in was[k]) if k in was else (rb(VLEN), rb(7), rb(5))  # noqa: E731
    held, held_off = rm.join([layout(hs[k], k, *was[k]) for k in keys[:NH]], lead=b"\x66" * 3)
    order = keys[N0:] + [keys[int(i)] for i in rng.choice(np.arange(N0, NK), DUP, replace=False)]
    new, new_off = rm.join([layout(hs[k], k, *change(k)) for k in order], lead=b"\x33" * 7)
    d = df.diff_model(new, new_off, held, held_off)
    return dict(new=np.frombuffer(bytes(new), np.uint8).copy(), new_off=np.array(new_off, np.int64),
                held=np.frombuffer(bytes(held), np.uint8).copy(), held_off=np.array(held_off, np.int64),
                rel=d[0].copy(), seen=d[2].copy())


def _expect(d, reduced):
    new, held = (d["new"].tobytes(), d["new_off"]), (d["held"].tobytes(), d["held_off"])
    if reduced:
        ca, cb = dl.last_copies(*new), dl.last_copies(*held)
        x = df.diff_model(new[0], new[1], held[0], held[1], ca, cb)
        rel, seen = x[0], x[2]
    else:
        rel, seen, cb = d["rel"], d["seen"], None
    log, slot_off, made, counts = dl.delta_model(new[0], new[1], rel, held[0], held[1], cb, seen)
    return dict(log=np.frombuffer(log, np.uint8), slot_off=slot_off.view(np.int64), made=made, counts=tuple(counts))


# name -> (expected outputs, the call)
CASES = {
    "delta_records": (lambda o, d: _expect(d, False),
                      lambda d, s: _named(delta.delta_records(d["new"], d["new_off"], d["rel"], d["held"], d["held_off"],
                                                              d["seen"], want_made=True, stream=s))),
    "delta_log": (lambda o, d: _expect(d, True),
                  lambda d, s: _named(delta.delta_log(d["new"], d["new_off"], d["held"], d["held_off"], stream=s,
                                                      want_made=True))),
}
NAMES = list(CASES)


# ------------------------------------------------------------------------------------- CPU
def test_every_wrapper_of_the_module_has_a_case():
    found = {name for name, fn in inspect.getmembers(delta, inspect.isfunction)
             if fn.__module__ == delta.__name__ and not name.startswith("_") and "stream" in inspect.signature(fn).parameters}
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
    # the reduction matters here: the second copies change what delta_log answers
    assert not _same(_expect(real, True)["log"], _expect(real, False)["log"])


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
