"""k2h_amd_ralledata_archive with byte offset 2^32 inside the stream it reads (the first-offset
technique of big_offsets.py: its row 5 streams, reused unchanged) and inside the archive it writes
(the ballast technique): block-relative quantities of the build kernel are 16- and 32-bit, every
absolute source and destination 64-bit.  Expected bytes come from ralle_archive_model.model."""
import ctypes
import struct

import numpy as np
import pytest

import big_offsets as bo
import ralle_archive_model as m
import ralle_check_model as rm
from big_offsets import BIG, LINE, TAIL, TAIL0

B = m.B


def input_scenario(oracle, kind):
    """bo.check_stream(kind): 192 blobs whose blob 96 holds the line, refused headers planted
    behind it.  Returns (tail image, absolute offsets, the model over the image, line block)."""
    data, off, planted = bo.check_stream(oracle, kind)
    tail = bo.image([(int(off[0]), data)])
    rel = [int(x) - TAIL0 for x in off]
    want = m.model(tail.tobytes(), rel, TAIL)
    return tail, off, want, planted, bo.CHECK_LINE_BLOB // B


class ArchiveBallast:
    """NB ballast blobs (an 8-byte key and one value; NB a multiple of the block, so the tail
    starts a block) whose records end 2048 bytes below the line, then the tail: block A (ordinary
    blobs, staged, its records hold the line), block B (one 20 KiB value: direct, every record
    above the line), block C (ordinary, staged, above the line)."""
    NB = 8192 - 64
    REC = (LINE - 2048) // NB            # 528416: a ballast blob's record
    STRIDE = REC - m.SCOM + rm.HEADER    # and the blob itself
    KEY = 8
    VAL = STRIDE - rm.HEADER - KEY

    def __init__(self, oracle):
        assert self.NB % B == 0 and self.NB * self.REC == LINE - 2048
        rng = m._rng(40)
        ks, vs, ss, as_ = m.records(rng, 3 * B, p_extra=0.3)
        vs[B + B // 2] = m.rbytes(rng, 20 * 1024)
        self.tail, tail_off = rm.join(m.blobs_of(oracle, ks, vs, ss, as_))
        self.ballast_in = self.NB * self.STRIDE
        self.ballast_out = self.NB * self.REC
        self.off = [i * self.STRIDE for i in range(self.NB)] + [self.ballast_in + x for x in tail_off]
        self.n = self.NB + 3 * B
        self.size = self.off[-1]
        self.want = m.model(self.tail, tail_off)
        self.forms = m.forms(self.want[3], tail_off)
        self.blob_head = struct.pack("<10Q", 0, 0, self.KEY, self.VAL, 0, 0, rm.HEADER, rm.HEADER + self.KEY,
                                     self.STRIDE, self.STRIDE)
        self.rec_head = m.scom_set_all(bytes(self.KEY), bytes(self.VAL))[:m.SCOM]
        self.total = self.ballast_out + int(self.want[1][-1])


# ------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("kind", ["staged", "direct"])
def test_input_scenario_holds_the_line_in_a_block_of_that_form(oracle, kind):
    tail, off, want, planted, blk = input_scenario(oracle, kind)
    assert bo.holds_line(int(off[bo.CHECK_LINE_BLOB]), int(off[bo.CHECK_LINE_BLOB + 1]))
    forms = m.forms(want[3], [int(x) - TAIL0 for x in off])
    assert forms[blk] == kind, forms
    segs = want[3]
    # the refused headers lie behind the line, in its block; the wrong hash fields change nothing
    for i, st in planted.items():
        assert (segs[i] is None) == (st in (rm.BAD_SPAN, rm.EMPTY, rm.NO_KEY, rm.BAD_RANGE)), (i, st)
        assert i // B == blk
    assert want[2] == len(segs) - sum(s is None for s in segs) and want[2] >= len(segs) - 5


def test_output_scenario_crosses_the_line_in_a_staged_block(oracle):
    b = ArchiveBallast(oracle)
    assert b.forms == ["staged", "direct", "staged"]
    rec_off = b.want[1].astype(np.int64) + b.ballast_out
    assert bo.holds_line(int(rec_off[0]), int(rec_off[B])) and rec_off[B] > LINE
    assert any(bo.holds_line(int(rec_off[i]), int(rec_off[i + 1])) for i in range(B))   # inside a record
    assert len(b.blob_head) == rm.HEADER and rm.header_status(b.blob_head + bytes(8), 0, b.STRIDE, b.STRIDE)[0] == rm.OK
    assert b.size < LINE < b.total


# ------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def device_memory(cuda):
    """What these tests free stays with torch's caching allocator until the module ends."""
    import torch
    yield
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big(cuda, device_memory):
    t = bo.big_buffer(cuda)
    yield t
    del t


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["staged", "direct"])
def test_archive_input_crosses_the_line(cuda, oracle, big, kind):
    """The stream lies across 2^32 of the big buffer."""
    tail, off, want, _planted, _blk = input_scenario(oracle, kind)
    bo.load_tail(big, tail)
    res = m.run(cuda, big, BIG, off, oshift=9)
    m.check(("input", kind), res, want)


@pytest.mark.gpu
def test_archive_output_crosses_the_line(cuda, oracle, device_memory):
    """rec_off passes 2^32 inside block A of the tail; blocks B and C lie wholly above it."""
    import torch

    from k2hash_amd import _native, batch
    b = ArchiveBallast(oracle)
    inp = batch.synth_bytes(b.size, cuda, byte_off=4343)
    head = torch.from_numpy(np.frombuffer(b.blob_head, np.uint8).copy()).to(cuda)
    inp[:b.ballast_in].view(b.NB, b.STRIDE)[:, :rm.HEADER] = head
    inp[b.ballast_in:] = torch.from_numpy(np.frombuffer(bytes(b.tail), np.uint8).copy()).to(cuda)
    d_off = torch.tensor(b.off, dtype=torch.int64, device=cuda)
    whole, out = bo.guarded(torch, cuda, b.total, shift=7)
    full, rec_off = bo.sentinel_words(torch, cuda, b.n + 1)
    total, recs = ctypes.c_uint64(0), ctypes.c_uint64(0)
    try:
        _native.check(_native.batch_lib().k2h_amd_ralledata_archive(
            bo._p(inp), b.size, bo._p(d_off), b.n, None, bo._p(out), out.numel(), bo._p(rec_off), ctypes.byref(recs),
            ctypes.byref(total), bo._stream()))
        torch.cuda.synchronize()
        assert (total.value, recs.value) == (b.total, b.n)
        got_off = bo.words_back(torch, full, b.n + 1, "rec_off")
        assert np.array_equal(got_off[:b.NB], np.arange(b.NB, dtype=np.uint64) * np.uint64(b.REC))
        assert np.array_equal(got_off[b.NB:], b.want[1] + np.uint64(b.ballast_out))
        assert bo.guards_intact(torch, whole, out), "bytes outside out written"
        rows = out[:b.ballast_out].view(b.NB, b.REC)
        want_head = torch.from_numpy(np.frombuffer(b.rec_head, np.uint8).copy()).to(cuda)
        assert bool((rows[:, :m.SCOM] == want_head).all()), "ballast record headers"
        assert bo.rows_equal(torch, rows[:, m.SCOM:], inp[:b.ballast_in].view(b.NB, b.STRIDE)[:, rm.HEADER:])
        got = out[b.ballast_out:].cpu().numpy()
        bad = np.flatnonzero(got != b.want[0])
        assert bad.size == 0, f"{bad.size} tail bytes differ, first at {int(bad[0])}"
    finally:
        del whole, out, inp
