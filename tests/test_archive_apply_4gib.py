"""k2h_amd_archive_apply across byte offset 2^32 (big_offsets.py): one LINE + SLACK buffer of
which only the tail is written serves as the held stream AND as the file.  Eight ballast blobs
with EMPTY headers fill it up to 4 KiB below the line and are copied through, so that part 1 ends
37 bytes below the line of the output; behind them a held blob X lies across the line with its
key on both sides of it; the log's first record addresses X by a key range that IS X's key, so a
record key crosses the line too; and the first part-2 blob, X rewritten, is written across the line
of the output with fields read from both sides of the line of the input.  Expected values come
from archive_apply_model.py over the tail's own bytes.
"""
import ctypes

import numpy as np
import pytest

import archive_apply_model as am
import archive_fold_model as fm
import big_offsets as bo
import ralle_archive_model as ra
import ralle_check_model as rm
from archive_fold_model import Rec
from big_offsets import BIG, LINE
from ralle_unlink_model import layout

NB = 8                       # ballast blobs
E = LINE - 4096              # where they end
S = E // NB
SHORT = 37                   # part 1 ends this many bytes below the line of the output
KX = b"the-key-of-the-blob-across-the-line"


@pytest.fixture(scope="module")
def big(cuda):
    """A LINE + 256 KiB buffer of which only the last 512 KiB are written; freed, and given
    back to the device, when the module ends.  Skips when the device has no room for it and an
    output of its size."""
    import torch
    free, _total = torch.cuda.mem_get_info(cuda)
    if free < 2 * bo.BIG + (512 << 20):
        pytest.skip("the device has less free memory than the two 4 GiB buffers need")
    t = bo.big_buffer(cuda)
    yield t
    del t
    torch.cuda.empty_cache()


def scenario(oracle):
    """(tail pieces, absolute held offsets, host records with absolute offsets, h1, h2, the model
    over the small stream, KX's absolute offset)."""
    keys = [KX, b"another-touched-key", b"an-untouched-key", b"filler", b"a-key-only-the-log-knows"]
    hs = am.hashes_of(oracle, keys)
    rng = ra._rng(77)
    # X: its key begins 11 bytes below the line; subkeys before the key, attrs behind the value
    x = ra.forge(KX, ra.rbytes(rng, 300), ra.rbytes(rng, 40), ra.rbytes(rng, 25), order=(2, 0, 1, 3), gaps=(3, 5, 0, 2),
                 slack=6, hashes=hs[KX])
    y = layout(hs[keys[1]], keys[1], b"y-value", b"", b"y-attrs")
    kpos = rm.get(x, 0, rm.F_KPOS)
    # X's key begins at LINE - 11: the filler's span takes `lead` slack bytes in to bring it there;
    # z is as long as it takes for part 1 (ballast, filler, z) to end at LINE - SHORT
    z = layout(hs[keys[2]], keys[2], ra.rbytes(rng, 11 + kpos - SHORT - 80 - len(keys[2])), b"", b"")
    filler = layout(hs[keys[3]], keys[3], ra.rbytes(rng, 3000), b"", b"")
    lead = 4096 - 11 - kpos - len(filler)
    assert lead >= 0
    small = bytes(filler) + bytes([0x5C]) * lead + bytes(x) + bytes(y) + bytes(z)
    rel = [0, len(filler) + lead, len(filler) + lead + len(x), len(filler) + lead + len(x) + len(y), len(small)]
    held_off = [k * S for k in range(NB)] + [E + r for r in rel]
    log = [Rec(fm.REPLACE_VAL, KX, ra.rbytes(rng, 5000)), Rec(fm.REPLACE_SKEY, keys[1], b"", b"new-subkeys"),
           Rec(fm.SET_ALL, keys[4], ra.rbytes(rng, 100), b"", b"attrs")]
    file, recs = am.build_log(log)
    f0 = E + len(small) + 13
    recs = bo.shift_archive(recs, f0)
    kx_at = held_off[NB + 1] + kpos
    recs[0]["key_off"] = kx_at                      # the record's key is the held blob's, across the line
    h1, h2 = am.rec_hashes(oracle, log)
    m = am.apply_model(small, rel, None, log, None, h1, h2)
    return [(E, small), (f0, file)], held_off, recs, h1, h2, m, kx_at


# ------------------------------------------------------------------------------------- CPU
def test_scenario_crosses_the_line_three_times(oracle):
    pieces, off, recs, h1, h2, m, kx_at = scenario(oracle)
    assert bo.image(pieces).size == bo.TAIL and NB * S == E
    assert bo.holds_line(off[NB + 1], off[NB + 2])                          # a held blob
    assert bo.holds_line(kx_at, kx_at + len(KX)) and int(recs[0]["key_off"]) == kx_at   # its key, which is a record's
    assert m.counts == [5, len(m.out), 2, 2, 0, 0, 3] and m.touched.tolist() == [0, 1, 1, 0]
    p1 = E + int(m.out_off[2])
    assert p1 == LINE - SHORT and bo.holds_line(p1, E + int(m.out_off[3]))  # the first part-2 blob, in the output
    assert m.origin.tolist() == [0, 3, 4, 5, 6]


# ------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_apply_across_4gib(cuda, oracle, big):
    import torch

    from k2hash_amd import _native, archive
    pieces, off, recs, h1, h2, m, _kx = scenario(oracle)
    bo.load_tail(big, bo.image(pieces))
    for k in range(NB):                             # the ballast blobs' headers: EMPTY, copied through
        big[k * S:k * S + rm.HEADER] = 0
    na, n = len(off) - 1, len(recs)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    d_recs = torch.from_numpy(np.ascontiguousarray(recs).view(np.int64).reshape(-1, archive.REC_WORDS).copy()).to(cuda)
    d_h1 = torch.from_numpy(h1.view(np.int64).copy()).to(cuda)
    d_h2 = torch.from_numpy(h2.view(np.int64).copy()).to(cuda)
    tw, touched = bo.guarded(torch, cuda, na, fill=0xEE)
    counts = (ctypes.c_uint64 * 7)(*[0xDEAD] * 7)
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    stop = ctypes.c_uint64(0xDEAD)
    lib = _native.batch_lib()

    def call(o, cap, oo, og):
        return lib.k2h_amd_archive_apply(bo._p(big), BIG, bo._p(d_off), na, None, bo._p(big), BIG, bo._p(d_recs), n, None,
                                         bo._p(d_h1), bo._p(d_h2), 0, o, cap, oo, og, bo._p(touched), cp,
                                         ctypes.byref(stop), bo._stream())
    want_counts = [NB + m.counts[0], E + m.counts[1], NB + m.counts[2]] + m.counts[3:]
    _native.check(call(None, 0, None, None))
    assert [int(c) for c in counts] == want_counts and stop.value == n
    whole, out = bo.guarded(torch, cuda, want_counts[1], shift=7)
    fo, ooff = bo.sentinel_words(torch, cuda, na + n + 1)
    fg, origin = bo.sentinel_words(torch, cuda, na + n)
    try:
        _native.check(call(bo._p(out), out.numel(), bo._p(ooff), bo._p(origin)))
        torch.cuda.synchronize()
        assert [int(c) for c in counts] == want_counts
        assert bo.guards_intact(torch, whole, out), "bytes outside out written"
        assert bo.guards_intact(torch, tw, touched, 0xEE), "bytes outside touched written"
        assert touched.cpu().numpy().tolist() == [0] * NB + m.touched.tolist()
        e = want_counts[0]
        a = fo.cpu().numpy().view(np.uint64)
        assert a[:e + 1].tolist() == [k * S for k in range(NB)] + [E + int(x) for x in m.out_off]
        assert (a[e + 1:] == np.uint64(bo.SENTINEL)).all(), "out_off written past entry emitted"
        b = fg.cpu().numpy().view(np.uint64)
        assert b[:e].tolist() == list(range(NB)) + [NB + int(x) for x in m.origin]
        assert (b[e:] == np.uint64(bo.SENTINEL)).all(), "origin written past entry emitted - 1"
        assert bo.rows_equal(torch, out[:E].view(-1, 4096), big[:E].view(-1, 4096), rows=1 << 16), "the ballast"
        got = out[E:].cpu().numpy().tobytes()
        assert got == m.out, "the blobs around the line"
    finally:
        del whole, out
