"""k2h_amd_ralledata_unlink with the stream's offsets across 2^32 (the first-offset technique of
big_offsets.py): a few hundred blobs that start just below byte 2^32 of a LINE + SLACK buffer of
which only the tail is written; the line falls inside a list that is rewritten.  Expected values
come from ralle_unlink_model.py over the stream's own bytes at offsets from 0.
"""
import numpy as np
import pytest

import big_offsets as bo
import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_subkeys_model as sm
import ralle_unlink_model as um

N = 300
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
    """(bytes, absolute offsets, drop, keep): lists of 0..3 names, blob LINE_BLOB with 40 names
    inside which the line falls and of which every other one is dropped; drops on both sides."""
    rng = np.random.default_rng(33)
    keys = [b"line-key-%03d-" % i + bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8)) for i in range(N)]
    lists = [sm.serialize([keys[int(j)] for j in rng.integers(0, N, i % 4)]) if i % 4 else b"" for i in range(N)]
    lists[LINE_BLOB] = sm.serialize([keys[int(j)] for j in rng.integers(0, N, 40)])
    blobs = dm.at_odd_offsets(sm.blobs_with_lists(oracle, keys, lists), seed=4)
    buf, off = rm.join(blobs)
    spos = rm.get(blobs[LINE_BLOB], 0, rm.F_SPOS)
    first = bo.LINE - off[LINE_BLOB] - spos - 301           # the line falls 301 bytes into the list
    m = sm.edges_model(oracle, bytes(buf), off)
    drop = (rng.random(m.counts[3]) < 0.4).astype(np.uint8)
    e0 = int(m.edge_off[LINE_BLOB])
    drop[e0:e0 + 40] = np.arange(40) % 2
    keep = (rng.random(N) < 0.9).astype(np.uint8)
    keep[LINE_BLOB] = 1
    return bytes(buf), [first + x for x in off], m, drop, keep


def test_line_runs_through_a_rewritten_list(oracle):
    buf, off, m, drop, keep = _stream(oracle)
    assert bo.image([(off[0], buf)]).size == bo.TAIL
    e0, e1 = int(m.edge_off[LINE_BLOB]), int(m.edge_off[LINE_BLOB + 1])
    assert e1 - e0 == 40
    where = [off[0] + p for p, _ln in m.where[e0:e1]]
    assert where[0] < bo.LINE < where[-1]                   # names of the list on both sides of the line
    want = um.unlink_model(buf, [x - off[0] for x in off], m.flags, m.edge_off, drop, keep=keep)
    assert want.changed[LINE_BLOB] == um.REWRITTEN and want.counts[2] > 50 and want.counts[6] == 0
    rewritten = np.nonzero(want.changed)[0]
    assert (np.array(off)[rewritten + 1] <= bo.LINE).sum() > 20 and (np.array(off)[rewritten] >= bo.LINE).sum() > 20


@pytest.mark.gpu
def test_offsets_across_4gib(cuda, oracle, big):
    buf, off, m, drop, keep = _stream(oracle)
    bo.load_tail(big, bo.image([(off[0], buf)]))
    want = um.unlink_model(buf, [x - off[0] for x in off], m.flags, m.edge_off, drop, keep=keep)
    um.assert_unlinked(um.run_unlink(cuda, big, bo.BIG, off, m.flags, m.edge_off, drop, keep=keep), want, "offsets across 2^32")
    want = um.unlink_model(buf, [x - off[0] for x in off], m.flags, m.edge_off, None)
    um.assert_unlinked(um.run_unlink(cuda, big, bo.BIG, off, m.flags, m.edge_off, None), want, "offsets across 2^32, no drop")
