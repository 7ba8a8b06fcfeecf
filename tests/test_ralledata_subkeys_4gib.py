"""k2h_amd_ralledata_subkeys and _reach with the stream's offsets across 2^32 (the first-offset
technique of big_offsets.py): a few hundred blobs that start just below byte 2^32 of a LINE +
SLACK buffer of which only the tail is written, parents and children on both sides of the line,
one list and one name running through it.  Expected values come from ralle_subkeys_model.py
over the stream's own bytes at offsets from 0.
"""
import numpy as np
import pytest

import big_offsets as bo
import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_subkeys_model as sm

N = 400
LINE_BLOB = 150          # its subkeys segment holds the line


@pytest.fixture(scope="module")
def big(cuda):
    """A LINE + 256 KiB buffer of which only the last 512 KiB are written; freed, and given
    back to the device, when the module ends.  Skips when the device has no room for it."""
    import torch
    free, _total = torch.cuda.mem_get_info(cuda)
    if free < bo.BIG + (256 << 20):
        pytest.skip("the device has less free memory than the 4 GiB buffer needs")
    t = bo.big_buffer(cuda)
    yield t
    del t
    torch.cuda.empty_cache()


def _stream(oracle):
    """(bytes, absolute offsets, roots): every blob names two others, one before and one behind
    it in the stream, so edges cross the line both ways; blob LINE_BLOB has a list of 40 names,
    inside which the line falls."""
    rng = np.random.default_rng(32)
    keys = [b"line-key-%03d-" % i + bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8))
            for i in range(N)]
    lists = []
    for i in range(N):
        names = [keys[int(rng.integers(0, max(i, 1)))], keys[int(rng.integers(i, N))]] if i % 3 else []
        if i % 7 == 0:
            names.append(b"nobody-%d" % i)
        lists.append(sm.serialize(names) if names else b"")
    lists[LINE_BLOB] = sm.serialize([keys[int(j)] for j in rng.integers(0, N, 40)])
    keys.append(keys[20])                                   # a later copy, above the line, of a key below it
    lists.append(sm.serialize([keys[390], keys[5]]))
    blobs = dm.at_odd_offsets(sm.blobs_with_lists(oracle, keys, lists), seed=4)
    buf, off = rm.join(blobs)
    spos = rm.get(blobs[LINE_BLOB], 0, rm.F_SPOS)
    first = bo.LINE - off[LINE_BLOB] - spos - 301           # the line falls 301 bytes into the list
    return bytes(buf), [first + x for x in off], [3, 20, LINE_BLOB, 399]


def test_line_runs_through_a_list(oracle):
    buf, off, roots = _stream(oracle)
    assert bo.image([(off[0], buf)]).size == bo.TAIL
    rel0 = [x - off[0] for x in off]
    m = sm.edges_model(oracle, buf, rel0)
    e0, e1 = int(m.edge_off[LINE_BLOB]), int(m.edge_off[LINE_BLOB + 1])
    assert e1 - e0 == 40
    where = [(off[0] + p, ln) for p, ln in m.where[e0:e1]]
    assert where[0][0] < bo.LINE < where[-1][0]             # names of the list on both sides of the line
    below = [i for i in range(len(rel0) - 1) if off[i + 1] <= bo.LINE]
    above = [i for i in range(len(rel0) - 1) if off[i] >= bo.LINE]
    assert len(below) > 100 and len(above) > 100
    up = sum(1 for e, c in enumerate(m.child) if int(c) != sm.NONE and m.owner[e] in below and int(c) in above)
    down = sum(1 for e, c in enumerate(m.child) if int(c) != sm.NONE and m.owner[e] in above and int(c) in below)
    assert up > 20 and down > 20 and m.counts[4] > 20
    assert int(m.rep[20]) == N and int(m.rep[N]) == N
    reach, counts = sm.reach_model(m, roots)
    assert 10 < counts[0] < N and counts[2] == 1


@pytest.mark.gpu
def test_offsets_across_4gib(cuda, oracle, big):
    buf, off, roots = _stream(oracle)
    bo.load_tail(big, bo.image([(off[0], buf)]))
    rel0 = [x - off[0] for x in off]
    m = sm.edges_model(oracle, buf, rel0)
    got = sm.run_subkeys(cuda, big, bo.BIG, off)
    sm.assert_edges(got, m, "offsets across 2^32")
    mask = np.zeros(len(off) - 1, np.uint8)
    mask[roots] = 1
    want, _table = sm.removed_by(oracle, buf, rel0, roots)
    reach, counts = sm.run_reach(cuda, m, mask)
    assert (reach == want).all() and counts == sm.reach_model(m, roots)[1]
