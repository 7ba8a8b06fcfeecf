"""k2h_amd_archive_fold on a log that lies across byte offset 2^32: the first-offset technique of
big_offsets.py (a LINE + 256 KiB buffer of which only the last 512 KiB are written, the records'
offsets absolute).  The line runs through a key that has a later duplicate, so the link stage
compares keys on both sides of it and across it."""
import numpy as np
import pytest

import archive_fold_model as fm
import big_offsets as bo

from k2hash_amd import archive

LINE_REC = 100


def _line_log():
    """200 records over 40 keys; returns (log, file bytes, records with absolute offsets, the
    file's absolute start).  Record 100's key holds the line."""
    rng = np.random.default_rng(32)
    keys = [b"line-key-%02d-" % k + bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8))
            for k in range(40)]
    log = [fm.letter(fm.NINE[int(rng.integers(0, 9))], keys[int(rng.integers(0, 40))], i) for i in range(200)]
    data = b"".join(fm.record_bytes(r) for r in log)
    recs = archive.scan(data)
    r = recs[LINE_REC]
    start = bo.LINE - (int(r["key_off"]) + int(r["key_len"]) // 2)
    return log, data, bo.shift_archive(recs, start), start


def test_line_log_has_a_duplicated_key_on_the_line():
    log, data, recs, start = _line_log()
    assert recs.size == 200 and bo.image([(start, data)]).size == bo.TAIL
    r = recs[LINE_REC]
    assert bo.holds_line(int(r["key_off"]), int(r["key_off"]) + int(r["key_len"]))
    keep, by, dropped = fm.fold_model(log)
    assert by[LINE_REC] != fm.NONE and any(int(b) == LINE_REC for b in by)
    pairs = [(i, int(by[i])) for i in range(200) if by[i] != fm.NONE]
    assert any(j < LINE_REC for i, j in pairs) and any(i > LINE_REC for i, j in pairs)
    assert 60 < dropped < len(pairs)


@pytest.fixture(scope="module")
def big(cuda):
    import torch
    t = bo.big_buffer(cuda)
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_fold_across_4gib(cuda, big):
    log, data, recs, start = _line_log()
    bo.load_tail(big, bo.image([(start, data)]))
    want = fm.fold_model(log)
    fm.assert_same(fm.run_fold_on(cuda, big, bo.BIG, recs), want, "across 2^32, h1 computed")
    fm.assert_same(fm.run_fold_on(cuda, big, bo.BIG, recs, h1=np.zeros(200, np.uint64)), want, "across 2^32, h1 = 0")
