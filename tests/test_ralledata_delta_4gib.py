"""k2h_amd_ralledata_delta with byte offset 2^32 inside both streams it reads (the first-offset
technique of big_offsets.py: the two streams are base pointers GAP apart into the one big buffer,
so that each stream's own offset 2^32 lies in its written part) and inside the log it writes (the
ballast technique): the build kernel keeps every absolute source and destination in 64 bits.
Expected bytes come from ralle_delta_model.delta_model."""
import ctypes
import struct

import numpy as np
import pytest

import archive_apply_model as am
import archive_fold_model as fm
import big_offsets as bo
import ralle_archive_model as ra
import ralle_check_model as rm
import ralle_delta_model as dl
import ralle_diff_model as df
from big_offsets import BIG, GAP, LINE, TAIL0
from ralle_unlink_model import layout

N_A, N_B, LINE_BLOB = 12, 13, 5
KINDS = ("group", "wave")


def input_scenario(oracle, kind):
    """A: 12 blobs, every other one changed against B or new, blob 5 -- all three fields differ --
    holding A's offset 2^32 inside its value ("wave": a value of 6,000 bytes, which the slot's wave
    moves).  B: the held blobs of nine of A's keys and 4 keys A does not have, blob 5 -- not seen --
    holding B's offset 2^32 inside its key.  Returns (image, A's absolute offsets, B's offsets
    relative to its base pointer big + GAP, (A bytes, offsets from 0), (B bytes, offsets from 0))."""
    rng = ra._rng(60, kind == "wave")
    ka = [b"new-%02d-" % i + ra.rbytes(rng, 5 + 3 * i) for i in range(N_A)]
    kb = [b"gone-%02d-" % j + ra.rbytes(rng, 50) for j in range(4)]
    hs = am.hashes_of(oracle, ka + kb)
    f = lambda n: ra.rbytes(rng, n)  # noqa: E731
    new = {k: (f(6000 if kind == "wave" and i == LINE_BLOB else 40 + i), f(i % 4 * 9), f(i % 3 * 7)) for i, k in enumerate(ka)}
    held = {}
    for i, k in enumerate(ka):
        if i % 2 == 0:
            held[k] = new[k]                                        # unchanged
        elif i % 4 == 1:
            held[k] = (f(33), f(8), f(8))                           # every field differs (blob 5 among them)
    order_b = list(held)[:LINE_BLOB] + [kb[0]] + list(held)[LINE_BLOB:] + kb[1:]
    held.update({k: (f(20), b"", f(3)) for k in kb})
    a, b = dl.stream_from(new, hs), dl.stream_from(held, hs, order_b)
    assert len(a[1]) - 1 == N_A and len(b[1]) - 1 == N_B
    a_first = LINE - a[1][LINE_BLOB] - rm.HEADER - len(ka[LINE_BLOB]) - 17      # the line 17 bytes into the value
    b_first = LINE - b[1][LINE_BLOB] - rm.HEADER - 9                            # and 9 bytes into the key
    img = bo.image([(a_first, a[0]), (GAP + b_first, b[0])])
    return img, [a_first + x for x in a[1]], [b_first + x for x in b[1]], a, b


def model_of(a, b):
    d = df.diff_model(a[0], a[1], b[0], b[1])
    return dl.delta_model(a[0], a[1], d[0], b[0], b[1], None, d[2]), d


class DeltaBallast:
    """NB ballast blobs of A (an 8-byte key and one value), all new keys, whose SET_ALL records end
    2048 bytes below the line; then the tail: 40 A blobs with every kind of slot and 30 B blobs of
    which a third is not seen.  The line falls inside the tail's first records."""
    NB = 8192 - 64
    REC = (LINE - 2048) // NB
    STRIDE = REC - fm.SCOM + rm.HEADER
    KEY = 8
    VAL = STRIDE - rm.HEADER - KEY

    def __init__(self, oracle):
        assert self.NB * self.REC == LINE - 2048
        rng = ra._rng(61)
        ks, vs, ss, as_ = ra.records(rng, 40, vlen=(60, 200), p_extra=0.5)
        ks = [b"t%02d" % i + k for i, k in enumerate(ks)]
        kb = [b"h%02d" % j + ra.rbytes(rng, 20) for j in range(10)]
        hs = am.hashes_of(oracle, ks + kb)
        new = {k: (v, s, a_) for k, v, s, a_ in zip(ks, vs, ss, as_)}
        held = {k: (new[k][0] + b"!" * (i % 2), new[k][1] + b"+" * (i % 5 == 0), b"" if i % 3 else b"was")
                for i, k in enumerate(ks[:20])}
        held.update({k: (b"v", b"", b"") for k in kb})
        self.a, self.b = dl.stream_from(new, hs), dl.stream_from(held, hs)
        (self.log, self.slot_off, self.made, self.counts), d = model_of(self.a, self.b)
        self.rel = np.concatenate([np.full(self.NB, df.PART | df.DATA, np.uint8), d[0]])
        self.seen = d[2]
        self.ballast_in, self.ballast_out = self.NB * self.STRIDE, self.NB * self.REC
        self.a_off = [i * self.STRIDE for i in range(self.NB)] + [self.ballast_in + x for x in self.a[1]]
        self.na, self.nb = self.NB + 40, 30
        self.a_size = self.a_off[-1]
        self.blob_head = struct.pack("<10Q", 0, 0, self.KEY, self.VAL, 0, 0, rm.HEADER, rm.HEADER + self.KEY,
                                     self.STRIDE, self.STRIDE)
        self.rec_head = fm.scom_record(fm.SET_ALL, bytes(self.KEY), bytes(self.VAL))[:fm.SCOM]
        self.total = self.ballast_out + len(self.log)


# ------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("kind", KINDS)
def test_input_scenario_holds_the_line_in_both_streams(oracle, kind):
    img, a_off, b_off, a, b = input_scenario(oracle, kind)
    assert bo.holds_line(a_off[LINE_BLOB], a_off[LINE_BLOB + 1]) and bo.holds_line(b_off[LINE_BLOB], b_off[LINE_BLOB + 1])
    (log, slot_off, made, counts), d = model_of(a, b)
    assert made[LINE_BLOB] == 14 and made[N_A + LINE_BLOB] == dl.DEL_KEY        # both line blobs are read for records
    fa = struct.unpack_from("<10Q", a[0], a[1][LINE_BLOB])
    assert a_off[LINE_BLOB] + fa[7] < LINE < a_off[LINE_BLOB] + fa[7] + fa[3]   # inside the value the delta carries
    assert (fa[3] >= 4096) == (kind == "wave")
    fb = struct.unpack_from("<10Q", b[0], b[1][LINE_BLOB])
    assert b_off[LINE_BLOB] + fb[6] < LINE < b_off[LINE_BLOB] + fb[6] + fb[2]   # inside the key of the DEL_KEY
    assert counts[2:7] == [3, 3, 3, 3, 4] and counts[7] == 0
    assert GAP + b_off[-1] <= BIG and a_off[0] >= TAIL0 and a_off[-1] < GAP + b_off[0]


def test_output_scenario_crosses_the_line_in_a_record(oracle):
    s = DeltaBallast(oracle)
    off = s.slot_off.astype(np.int64) + s.ballast_out
    assert off[0] < LINE < off[-1] and s.a_size < LINE < s.total
    assert any(bo.holds_line(int(off[i]), int(off[i + 1])) for i in range(len(off) - 1))    # inside a slot's records
    assert len(s.blob_head) == rm.HEADER and rm.header_status(s.blob_head + bytes(8), 0, s.STRIDE, s.STRIDE)[0] == rm.OK
    assert all(c > 0 for c in s.counts[2:7]) and s.counts[7] == 0


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
@pytest.mark.parametrize("kind", KINDS)
def test_delta_inputs_cross_the_line(cuda, oracle, big, kind):
    """Both streams lie across their own offset 2^32 of the big buffer."""
    img, a_off, b_off, a, b = input_scenario(oracle, kind)
    bo.load_tail(big, img)
    want, d = model_of(a, b)
    got = dl.run_delta(cuda, big, a_off, d[0], big[GAP:], b_off, None, d[2], a_size=BIG, b_size=BIG - GAP, oshift=9)
    dl.assert_delta(got, want, ("inputs", kind))


@pytest.mark.gpu
def test_delta_output_crosses_the_line(cuda, oracle, device_memory):
    """slot_off passes 2^32 inside the tail's first records; the B slots lie wholly above it."""
    import torch

    from k2hash_amd import _native, batch
    s = DeltaBallast(oracle)
    inp = batch.synth_bytes(s.a_size, cuda, byte_off=4747)
    head = torch.from_numpy(np.frombuffer(s.blob_head, np.uint8).copy()).to(cuda)
    inp[:s.ballast_in].view(s.NB, s.STRIDE)[:, :rm.HEADER] = head
    inp[s.ballast_in:] = torch.from_numpy(np.frombuffer(bytes(s.a[0]), np.uint8).copy()).to(cuda)
    u8 = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.uint8).copy()).to(cuda)  # noqa: E731
    d_b, d_rel, d_seen = u8(np.frombuffer(bytes(s.b[0]), np.uint8)), u8(s.rel), u8(s.seen)
    d_aoff = torch.tensor(s.a_off, dtype=torch.int64, device=cuda)
    d_boff = torch.tensor(s.b[1], dtype=torch.int64, device=cuda)
    whole, out = bo.guarded(torch, cuda, s.total, shift=7)
    full, slot_off = bo.sentinel_words(torch, cuda, s.na + s.nb + 1)
    counts = (ctypes.c_uint64 * 8)()
    try:
        _native.check(_native.batch_lib().k2h_amd_ralledata_delta(
            bo._p(inp), s.a_size, bo._p(d_aoff), s.na, bo._p(d_rel), bo._p(d_b), d_b.numel(), bo._p(d_boff), s.nb, None,
            bo._p(d_seen), bo._p(out), out.numel(), bo._p(slot_off), None, ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64)),
            bo._stream()))
        torch.cuda.synchronize()
        want_counts = list(s.counts)
        want_counts[0] += s.NB
        want_counts[1] += s.ballast_out
        want_counts[2] += s.NB
        assert list(counts) == want_counts
        got_off = bo.words_back(torch, full, s.na + s.nb + 1, "slot_off")
        assert np.array_equal(got_off[:s.NB], np.arange(s.NB, dtype=np.uint64) * np.uint64(s.REC))
        assert np.array_equal(got_off[s.NB:], s.slot_off + np.uint64(s.ballast_out))
        assert bo.guards_intact(torch, whole, out), "bytes outside out written"
        rows = out[:s.ballast_out].view(s.NB, s.REC)
        want_head = torch.from_numpy(np.frombuffer(s.rec_head, np.uint8).copy()).to(cuda)
        assert bool((rows[:, :fm.SCOM] == want_head).all()), "ballast record headers"
        assert bo.rows_equal(torch, rows[:, fm.SCOM:], inp[:s.ballast_in].view(s.NB, s.STRIDE)[:, rm.HEADER:])
        got = out[s.ballast_out:].cpu().numpy()
        bad = np.flatnonzero(got != np.frombuffer(s.log, np.uint8))
        assert bad.size == 0, f"{bad.size} tail bytes differ, first at {int(bad[0])}"
    finally:
        del whole, out, inp
