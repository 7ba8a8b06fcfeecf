"""The `stream` argument of drop_mask, unlink_subkeys and prune_ralledata (k2hash_amd/unlink.py,
exported by subkeys.py too): the two scenarios of test_subkeys_stream.py -- late inputs, busy
current stream -- with stream_harness.py as it is and that module's stream builder and helpers.

drop_mask only enqueues work; unlink_subkeys synchronises `stream` to read its counts back
(once for the count call, once for the fill); prune_ralledata is subkey_edges, reach_subkeys and
those two.  Expected values come from ralle_unlink_model.py, never from a device call.
"""
import inspect

import numpy as np
import pytest

import ralle_subkeys_model as sm
import ralle_unlink_model as um
import stream_harness as sh
from stream_harness import independent_streams, stall, stalled
from test_subkeys_stream import N, SEED_BUSY, SEED_LATE, _back, _build, _compare, _named, _same, _to_dev, _warm

from k2hash_amd import subkeys, unlink


def _inputs(oracle, d):
    """The built stream with the model's edges (of the whole stream: E = 2 N whatever the seed),
    a drop mask, a gone mask and a keep mask that depend on the seed."""
    m = sm.edges_model(oracle, d["blobs"].tobytes(), d["blob_off"])
    assert m.counts[3] == 2 * N
    rng = np.random.default_rng([991, int(d["roots"].sum())])
    return dict(d, flags=m.flags, edge_off=m.edge_off.view(np.int64), child=m.child.view(np.int64),
                drop=(rng.random(2 * N) < 0.3).astype(np.uint8), gone=(rng.random(N) < 0.3).astype(np.uint8),
                keep=(rng.random(N) < 0.8).astype(np.uint8))


def _unlinked(u):
    return dict(blobs=np.frombuffer(u.out, np.uint8), blob_off=u.out_off.view(np.int64), index=u.index.view(np.int64),
                changed=u.changed, counts=tuple(u.counts))


def _expect_mask(oracle, d):
    child = d["child"].view(np.uint64)
    found = child != np.uint64(sm.NONE)
    return dict(drop=np.where(found, d["gone"][np.where(found, child, 0).astype(np.int64)] != 0, True).astype(np.uint8))


def _expect_unlink(oracle, d):
    return _unlinked(um.unlink_model(d["blobs"].tobytes(), d["blob_off"], d["flags"], d["edge_off"].view(np.uint64), d["drop"],
                                     keep=d["keep"]))


def _expect_prune(oracle, d):
    m = sm.edges_model(oracle, d["blobs"].tobytes(), d["blob_off"], consider=d["consider"])
    reach, _counts = sm.reach_model(m, d["roots"])
    drop = np.array([c == np.uint64(sm.NONE) or reach[int(c)] != 0 for c in m.child], np.uint8)
    return _unlinked(um.unlink_model(d["blobs"].tobytes(), d["blob_off"], m.flags, m.edge_off, drop,
                                     keep=(d["consider"] != 0) & (reach == 0)))


def _edges_of(d):
    return subkeys.SubkeyEdges(d["flags"], d["edge_off"], d["child"], None, subkeys.SubkeyCounts(0, 0, 0, 2 * N, 0))


# name -> (inputs from the built stream, expected outputs, the call)
CASES = {
    "drop_mask": (_inputs, _expect_mask,
                  lambda d, s: dict(drop=unlink.drop_mask(_edges_of(d), gone=d["gone"], dangling=True, stream=s))),
    "unlink_subkeys": (_inputs, _expect_unlink,
                       lambda d, s: _named(unlink.unlink_subkeys(d["blobs"], d["blob_off"], _edges_of(d), d["drop"],
                                                                 keep=d["keep"], stream=s))),
    "prune_ralledata": (lambda o, d: d, _expect_prune,
                        lambda d, s: _named(unlink.prune_ralledata(d["blobs"], d["blob_off"], d["roots"], dangling=True,
                                                                   consider=d["consider"], stream=s))),
}
NAMES = list(CASES)


# ------------------------------------------------------------------------------------- CPU
def test_every_wrapper_of_the_module_has_a_case():
    found = {name for name, fn in inspect.getmembers(unlink, inspect.isfunction)
             if fn.__module__ == unlink.__name__ and not name.startswith("_") and "stream" in inspect.signature(fn).parameters}
    assert found == set(NAMES)
    for name in NAMES:
        assert getattr(subkeys, name) is getattr(unlink, name)


@pytest.mark.parametrize("name", NAMES)
def test_decoy_has_the_shapes_and_another_answer(oracle, name):
    inputs, expect, _run = CASES[name]
    real, decoy = inputs(oracle, _build(oracle, SEED_LATE)), inputs(oracle, _build(oracle, -SEED_LATE % 97))
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
    inputs, expect, run = CASES[name]
    c, s = independent_streams(cuda)
    real, decoy = inputs(oracle, _build(oracle, SEED_LATE)), inputs(oracle, _build(oracle, -SEED_LATE % 97))
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
    print(f"{name}: host {ms:.3f} ms")
    _compare(name, _back(torch, out, s), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_busy_current_stream(cuda, oracle, name):
    """The current stream is stalled, the call names another: the results reach the host
    through `stream` while the current one is still stalled, so the call neither waited for the
    current stream nor left work on it."""
    import torch
    inputs, expect, run = CASES[name]
    c, s = independent_streams(cuda)
    real, decoy = inputs(oracle, _build(oracle, SEED_BUSY)), inputs(oracle, _build(oracle, -SEED_BUSY % 97))
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
