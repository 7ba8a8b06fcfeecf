"""k2h_amd_ralledata_diff with one stream's offsets across 2^32 (the technique of
big_offsets.py): the big stream as A with a matched pair's value segment running through the
line and B small, then the roles swapped on the same fixture.  Expected values come from
ralle_diff_model.py over the streams' own bytes at offsets from 0.
"""
import numpy as np
import pytest

import big_offsets as bo
import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_diff_model as fm
import ralle_times_model as tm

LINE_BLOB = 80
LONG = 3000          # bytes of the value that runs through the line: more than two wave steps


@pytest.fixture(scope="module")
def big(cuda):
    """A LINE + 256 KiB buffer of which only the last 512 KiB are written; freed, and given
    back to the device, when the module ends."""
    import torch
    t = bo.big_buffer(cuda)
    yield t
    del t
    torch.cuda.empty_cache()


def _streams(oracle):
    """(big stream's bytes, its absolute offsets, small stream's blobs)."""
    rng = np.random.default_rng(64)
    keys = [b"line-key-%02d" % int(k) for k in rng.integers(0, 40, 160)]
    vals = [bytes(rng.integers(0, 256, int(rng.integers(0, 120)), dtype=np.uint8)) for _ in range(160)]
    long_val = bytes(rng.integers(0, 256, LONG, dtype=np.uint8))
    keys[LINE_BLOB] = keys[LINE_BLOB + 2] = b"the-long-one"
    vals[LINE_BLOB] = long_val
    vals[LINE_BLOB + 2] = long_val[:-1] + bytes([long_val[-1] ^ 1])
    blobs = dm.at_odd_offsets(dm.blobs_of(oracle, keys, vals), seed=8)
    buf, off = rm.join(blobs)
    vpos = rm.get(blobs[LINE_BLOB], 0, rm.F_VPOS)
    first = bo.LINE - off[LINE_BLOB] - vpos - 1111          # the line falls 1111 bytes into the long value
    held_keys = [b"line-key-%02d" % k for k in range(0, 40, 2)] + [b"the-long-one", b"held-only"]
    last = {k: v for k, v in zip(keys, vals)}
    held_vals = [long_val if k == b"the-long-one" else last.get(k, b"x") if i % 3 else b"stale" for i, k in
                 enumerate(held_keys)]
    small = dm.at_odd_offsets(dm.blobs_of(oracle, held_keys, held_vals), seed=9)
    return bytes(buf), [first + x for x in off], small


def test_line_runs_through_a_matched_value(oracle):
    buf, off, small = _streams(oracle)
    assert bo.image([(off[0], buf)]).size == bo.TAIL
    vpos = rm.get(buf, off[LINE_BLOB] - off[0], rm.F_VPOS)
    assert bo.holds_line(off[LINE_BLOB] + vpos + 1024, off[LINE_BLOB] + vpos + LONG - 1024)
    assert off[LINE_BLOB + 2] > bo.LINE and off[LINE_BLOB - 1] < bo.LINE
    rel0 = [x - off[0] for x in off]
    rel, match, seen, counts = fm.diff_model(buf, rel0, *rm.join(small))
    assert rel[LINE_BLOB] == fm.PART | fm.FOUND | fm.DATA | fm.REPEAT
    assert rel[LINE_BLOB + 2] == fm.PART | fm.FOUND | fm.DATA | fm.REPEAT | fm.VAL
    assert 0 < counts[2] < counts[1] < counts[0] == 160 and seen[-1] == 0 and seen[-2] == 1
    rel, match, seen, counts = fm.diff_model(*rm.join(small), buf, rel0)
    at = len(small) - 2
    assert match[at] == LINE_BLOB + 2 and rel[at] & fm.VAL and seen[LINE_BLOB] == 0 and seen[LINE_BLOB + 2] == 1


@pytest.mark.gpu
def test_offsets_across_4gib(cuda, oracle, big):
    buf, off, small = _streams(oracle)
    bo.load_tail(big, bo.image([(off[0], buf)]))
    rel0 = [x - off[0] for x in off]
    s_buf, s_off = rm.join(small)
    ts = tm.place(cuda, s_buf, 5)
    want = fm.diff_model(buf, rel0, s_buf, s_off)
    fm.assert_diff(fm.run_diff(cuda, big, bo.BIG, off, ts, len(s_buf), s_off), want, "A across 2^32")
    want = fm.diff_model(s_buf, s_off, buf, rel0)
    fm.assert_diff(fm.run_diff(cuda, ts, len(s_buf), s_off, big, bo.BIG, off), want, "B across 2^32")
