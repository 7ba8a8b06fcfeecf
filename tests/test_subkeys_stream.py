"""The `stream` argument of k2hash_amd/subkeys.py (batch.py's module docstring): stream=None is
the current torch stream; otherwise every device operation of the call, the wrapper's own torch
ops included, is ordered on `stream` and none on the current stream.  The two scenarios of
test_stream_contract.py, with stream_harness.py as it is:

  late inputs    `s` is stalled and the real inputs arrive on it behind the stall, over a decoy;
                 work issued anywhere but `s` reads the decoy and computes its answer
  busy current   `c` is stalled; work issued to `c`, or a read-back on it, is not done when the
                 results have reached the host through `s`

No form of these wrappers is asynchronous, per the header: subkey_edges synchronises `stream`
because it reads E back (once for the count call, twice for the fill call), reach_subkeys once per
level and twice more, subtree_ralledata is both and select_ralledata.  Expected values come from
ralle_subkeys_model.py, never from a device call.
"""
import numpy as np
import pytest

import ralle_check_model as rm
import ralle_subkeys_model as sm
import stream_harness as sh
from stream_harness import independent_streams, stall, stalled

from k2hash_amd import subkeys

N = 600
SEED_LATE, SEED_BUSY = 11, 12


def _build(oracle, seed):
    """A stream whose sizes do not depend on the seed: N blobs with keys of one length and
    lists of exactly two names of that length; which names, which blobs are considered and which
    are roots does."""
    rng = np.random.default_rng([990, seed])
    keys = [b"node-%04d" % i for i in range(N)]
    lists = [sm.serialize([keys[int(a)], keys[int(b)] if b < N else b"none-%04d" % (b - N)])
             for a, b in zip(rng.integers(0, N, N), rng.integers(0, N + 60, N))]
    buf, off = rm.join(sm.blobs_with_lists(oracle, keys, lists, vals=[b"v"] * N))
    consider = (rng.random(N) < 0.9).astype(np.uint8)
    roots = np.sort(rng.choice(N, 5, replace=False)).astype(np.int64)
    mask = np.zeros(N, np.uint8)
    mask[roots] = 1
    return dict(blobs=np.frombuffer(bytes(buf), np.uint8).copy(), blob_off=np.array(off, np.int64), consider=consider,
                roots=roots, roots_mask=mask)


def _with_edges(oracle, d, consider=None):
    """The inputs of reach_subkeys: the model's edges of the stream, as arrays (of the whole
    stream, so that their sizes do not depend on the seed either)."""
    m = sm.edges_model(oracle, d["blobs"].tobytes(), d["blob_off"], consider=consider)
    return dict(d, edge_off=m.edge_off.view(np.int64), child=m.child.view(np.int64), rep=m.rep.view(np.int64)), m


def _expect_edges(oracle, d, count_only=False):
    m = sm.edges_model(oracle, d["blobs"].tobytes(), d["blob_off"], consider=d["consider"])
    out = dict(flags=m.flags, edge_off=m.edge_off.view(np.int64), counts=tuple(m.counts[:4] + [0] if count_only else m.counts))
    if not count_only:
        out.update(child=m.child.view(np.int64), rep=m.rep.view(np.int64))
    return out


def _expect_reach(oracle, d, consider=None):
    _d, m = _with_edges(oracle, d, consider)
    reach, counts = sm.reach_model(m, d["roots"])
    want, _t = sm.removed_by(oracle, d["blobs"].tobytes(), d["blob_off"], [int(r) for r in d["roots"]], consider=consider)
    assert (reach == want).all()
    return dict(mask=reach, reached=counts[0], levels=counts[1], converged=bool(counts[2]))


def _expect_subtree(oracle, d, remove):
    reach = _expect_reach(oracle, d, d["consider"])["mask"]
    keep = (d["consider"] != 0) & (reach == 0) if remove else reach
    data, ooff, index = rm.select_model(d["blobs"], d["blob_off"], keep)
    return dict(blobs=data, blob_off=ooff.view(np.int64), index=index.view(np.int64), kept=len(index), kept_bytes=data.size)


def _edges_of(d):
    return subkeys.SubkeyEdges(None, d["edge_off"], d["child"], d["rep"], None)


def _named(res):
    return {k: v for k, v in res._asdict().items() if v is not None}


# name -> (inputs from the built stream, expected outputs, the call)
CASES = {
    "subkey_edges": (lambda o, d: d, _expect_edges,
                     lambda d, s: _named(subkeys.subkey_edges(d["blobs"], d["blob_off"], consider=d["consider"], stream=s))),
    "subkey_edges[count_only]": (lambda o, d: d, lambda o, d: _expect_edges(o, d, True),
                                 lambda d, s: _named(subkeys.subkey_edges(d["blobs"], d["blob_off"], consider=d["consider"],
                                                                          count_only=True, stream=s))),
    "reach_subkeys[mask]": (lambda o, d: _with_edges(o, d)[0], _expect_reach,
                            lambda d, s: _named(subkeys.reach_subkeys(_edges_of(d), d["roots_mask"], stream=s))),
    "reach_subkeys[index]": (lambda o, d: _with_edges(o, d)[0], _expect_reach,
                             lambda d, s: _named(subkeys.reach_subkeys(_edges_of(d), d["roots"], stream=s))),
    "subtree_ralledata": (lambda o, d: d, lambda o, d: _expect_subtree(o, d, False),
                          lambda d, s: _named(subkeys.subtree_ralledata(d["blobs"], d["blob_off"], d["roots"],
                                                                        consider=d["consider"], stream=s))),
    "subtree_ralledata[remove]": (lambda o, d: d, lambda o, d: _expect_subtree(o, d, True),
                                  lambda d, s: _named(subkeys.subtree_ralledata(d["blobs"], d["blob_off"], d["roots"],
                                                                                remove=True, consider=d["consider"],
                                                                                stream=s))),
}
NAMES = list(CASES)


def _same(a, b):
    if isinstance(b, np.ndarray):
        a = np.asarray(a)
        return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and (a.view(b.dtype) == b).all()
    return tuple(a) == tuple(b) if isinstance(b, tuple) else a == b


# ------------------------------------------------------------------------------------- CPU
def test_every_wrapper_of_the_module_has_a_case():
    import inspect
    found = {name for name, fn in inspect.getmembers(subkeys, inspect.isfunction)
             if fn.__module__ == subkeys.__name__ and not name.startswith("_") and "stream" in inspect.signature(fn).parameters}
    assert found == {"subkey_edges", "reach_subkeys", "subtree_ralledata"} == {n.split("[")[0] for n in NAMES}


def test_no_form_is_asynchronous_per_the_header():
    header = " ".join((rm.ROOT / "include" / "k2hash_amd.h").read_text().split()).replace(" * ", " ")
    for phrase in ("once with child NULL, twice otherwise. No form of the call is asynchronous.",
                   "`stream` is synchronised once for the start set, once per level run and once at the end: levels + 2 times"):
        assert phrase in header, phrase


@pytest.mark.parametrize("name", NAMES)
def test_decoy_has_the_shapes_and_another_answer(oracle, name):
    inputs, expect, _run = CASES[name]
    real, decoy = inputs(oracle, _build(oracle, SEED_LATE)), inputs(oracle, _build(oracle, -SEED_LATE % 97))
    for k, v in real.items():
        assert decoy[k].shape == v.shape and decoy[k].dtype == v.dtype, k
    want, other = expect(oracle, real), expect(oracle, decoy)
    assert set(want) == set(other)
    for k in want:
        if k not in ("converged", "edge_off"):       # every list has two names whatever the seed
            assert not _same(other[k], want[k]), f"{name}: the decoy's {k} equals the real one"


# ------------------------------------------------------------------------------------- GPU
def _to_dev(torch, cuda, arrays):
    return {k: torch.from_numpy(v).to(cuda) for k, v in arrays.items()}


def _back(torch, out, s):
    """The outputs on the host, read through `s`."""
    with torch.cuda.stream(s):
        got = {k: v.cpu() if torch.is_tensor(v) else v for k, v in out.items()}
    s.synchronize()
    return {k: v.numpy() if torch.is_tensor(v) else v for k, v in got.items()}


def _compare(name, got, want):
    assert set(got) == set(want), (name, sorted(got), sorted(want))
    for k in want:
        assert _same(got[k], want[k]), f"{name}: {k} differs from the model"


def _warm(torch, run, dev, c, s):
    """One call on the default stream and one as the tests make it: the launchers' scratch is
    grown and both streams' allocator pools hold blocks of these sizes before anything is stalled."""
    keep = [run(dev, None)]
    torch.cuda.synchronize()
    with torch.cuda.stream(c):
        keep.append(run(dev, s))
    torch.cuda.synchronize()


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
    print(f"{name}: host {ms:.3f} ms (synchronises)")
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
