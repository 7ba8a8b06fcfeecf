"""k2h_amd_ralledata_times and k2h_amd_ralledata_dedup_mtime on a stream whose attrs segments lie
across byte offset 2^32: the first-offset technique of big_offsets.py (a LINE + 256 KiB buffer of
which only the last 512 KiB are written, blob_off absolute)."""
import numpy as np
import pytest

import big_offsets as bo
import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_times_model as tm
from ralle_times_model import EXPIRE, MTIME, timeval

LINE_BLOB = 80


def _line_stream(oracle):
    """160 blobs over 40 keys, every one with mtime, expire and uniqid attrs; the attrs segment of
    blob 80 starts 21 bytes below the line, so the line runs through its first entry's two lengths
    and every later entry is above it."""
    rng = np.random.default_rng(32)
    n = 160
    keys = [b"line-key-%02d" % int(k) for k in rng.integers(0, 40, n)]
    vals = [bytes(rng.integers(0, 256, int(rng.integers(0, 120)), dtype=np.uint8)) for _ in range(n)]
    attrs = [tm.written_attrs([(MTIME, timeval(int(rng.integers(900, 1100)), i)),
                               (EXPIRE, timeval(int(rng.integers(1400, 1600)), i)), (b"uniqid\0", b"u%03d\0" % i)])
             for i in range(n)]
    buf, off = rm.join(dm.at_odd_offsets(dm.blobs_of(oracle, keys, vals, None, attrs), seed=8))
    first = bo.LINE - off[LINE_BLOB] - rm.get(buf, off[LINE_BLOB], rm.F_APOS) - 21
    return bytes(buf), [first + x for x in off]


WINDOW = tm.Window((950, 0), (1050, 0), (1500, 0))
PTS = (1000, 0)


def test_line_stream_has_attrs_across_the_line(oracle):
    buf, off = _line_stream(oracle)
    assert bo.image([(off[0], buf)]).size == bo.TAIL
    rel = [x - off[0] for x in off]
    a0 = off[LINE_BLOB] + rm.get(buf, rel[LINE_BLOB], rm.F_APOS)
    assert bo.holds_line(a0, a0 + rm.get(buf, rel[LINE_BLOB], rm.F_ALEN)) and a0 + 21 == bo.LINE
    flags, mtime, expire, keep = tm.times_model(buf, rel, window=WINDOW)
    assert (flags == 11).all() and 0 < keep[:LINE_BLOB].sum() < LINE_BLOB and 0 < keep[LINE_BLOB:].sum() < 80
    dkeep, by, dropped = tm.dedup_mtime_model(buf, rel, PTS)
    pairs = [(i, int(by[i])) for i in range(160) if by[i] != tm.NONE]
    assert any(i < LINE_BLOB < j for i, j in pairs) and 10 < dropped < len(pairs)


@pytest.fixture(scope="module")
def big(cuda):
    import torch
    t = bo.big_buffer(cuda)
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_attrs_across_4gib(cuda, oracle, big):
    buf, off = _line_stream(oracle)
    bo.load_tail(big, bo.image([(off[0], buf)]))
    rel = [x - off[0] for x in off]
    tm.assert_times(tm.run_times(cuda, big, bo.BIG, off, window=WINDOW), tm.times_model(buf, rel, window=WINDOW),
                    "times across 2^32")
    want = tm.dedup_mtime_model(buf, rel, PTS)
    tm.assert_dedup(tm.run_dedup_mtime(cuda, big, bo.BIG, off, PTS), want, "dedup_mtime across 2^32")
