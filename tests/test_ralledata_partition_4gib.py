"""k2h_amd_ralledata_partition with byte offset 2^32 inside the stream it reads and inside the
output it writes (the scenarios of big_offsets.py rows 6 and 7, reused unchanged): block-relative
quantities of the copy kernel are 16- and 32-bit, every absolute source and destination 64-bit.
Expected values come from ralle_part_model.partition_model."""
import numpy as np
import pytest

import big_offsets as bo
import ralle_part_model as pm
from big_offsets import BIG, LINE, TAIL, TAIL0


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, f"{bad.size} of {want.size} differ, first at {int(bad[0])}: "
                           f"{int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}")


def input_ids(kind):
    """Ids of the 300 blobs of bo.select_input(kind): 0, 1, 2 and, for a quarter, a value >= 3."""
    rng = np.random.default_rng([4096, kind == "searched"])
    return rng.choice(np.array([0, 1, 2, 3, pm.NONE], np.uint32), bo.SEL_N, p=[0.25, 0.25, 0.25, 0.125, 0.125])


def ballast_ids(b):
    """Ballast blobs to part 0; tail blobs to part 0, part 1 or (id 2 of 2 parts) left out."""
    rng = np.random.default_rng(4097)
    ids = np.zeros(b.n, np.uint32)
    ids[b.NB:] = rng.integers(0, 3, bo.SEL_N)
    return ids


# ------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("kind", ["tabled", "searched"])
def test_input_scenario_puts_every_part_on_both_sides(kind):
    data, off, _keep = bo.select_input(kind)
    ids = input_ids(kind)
    assert bo.holds_line(int(off[bo.SEL_LINE_BLOB]), int(off[bo.SEL_LINE_BLOB + 1]))
    for p in (0, 1, 2):
        mine = np.flatnonzero(ids == p)
        assert (off[mine + 1] <= LINE).any() and (off[mine] >= LINE).any()
    assert (ids >= 3).sum() > 30


def test_output_scenario_crosses_the_line_inside_part_0():
    b = bo.SelectBallast()
    ids = ballast_ids(b)
    lens = (b.off[1:] - b.off[:-1])
    part0 = int(lens[ids == 0].sum())
    assert b.ballast_bytes < LINE < part0 and b.ballast_bytes % 16 == 0
    assert (ids[b.NB:] == 1).sum() > 50 and (ids[b.NB:] == 2).sum() > 50
    assert b.n > 8 * pm.TILE and b.NB % pm.TILE != 0        # the line's tile holds ballast and tail blobs


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
def test_partition_output_crosses_the_line(cuda, device_memory):
    """Part 0 = every ballast blob and a third of the tail: it passes output offset 2^32 inside
    the tail; part 1 lies wholly above it."""
    import torch

    from k2hash_amd import batch
    b = bo.SelectBallast()
    ids = ballast_ids(b)
    tail = np.frombuffer(bytes(b.tail), np.uint8)
    tbytes, tooff, tindex, tpart, tfirst, tbyte = pm.partition_model(
        tail, b.off[b.NB:] - b.ballast_bytes, tail.size, pm.ids_rule(2), ids[b.NB:])
    total = b.ballast_bytes + tbytes.size
    inp = batch.synth_bytes(b.size, cuda, byte_off=4242)
    inp[b.ballast_bytes:] = torch.from_numpy(tail.copy()).to(cuda)
    whole, out = bo.guarded(torch, cuda, total)
    try:
        got = pm.run_partition(cuda, inp, b.size, b.off, pm.ids_rule(2), ids, None, out)
        assert got["first"] == [0, b.NB + tfirst[1], b.NB + tfirst[2]]
        assert got["byte"] == [0, b.ballast_bytes + tbyte[1], total] and got["byte"][1] > LINE
        same(got["part_out"][:b.NB], np.zeros(b.NB, np.uint32), "part_out of the ballast")
        same(got["part_out"][b.NB:], tpart, "part_out of the tail")
        same(got["out_off"][:b.NB], b.off[:b.NB].astype(np.uint64), "out_off of the ballast")
        same(got["out_off"][b.NB:], tooff + np.uint64(b.ballast_bytes), "out_off of the tail")
        same(got["index"][:b.NB], np.arange(b.NB, dtype=np.uint64), "index of the ballast")
        same(got["index"][b.NB:], tindex + np.uint64(b.NB), "index of the tail")
        assert bo.guards_intact(torch, whole, out), "bytes outside out written"
        assert bo.rows_equal(torch, out[:b.ballast_bytes].view(b.NB, b.STRIDE),
                             inp[:b.ballast_bytes].view(b.NB, b.STRIDE))
        same(out[b.ballast_bytes:].cpu().numpy(), tbytes, "tail bytes")
    finally:
        del whole, out, inp


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tabled", "searched"])
def test_partition_input_crosses_the_line(cuda, big, kind):
    """The stream lies across 2^32 of the big buffer; ids from {0, 1, 2, >= parts}."""
    import torch
    data, off, _keep = bo.select_input(kind)
    ids = input_ids(kind)
    tail = bo.image([(int(off[0]), data)])
    bo.load_tail(big, tail)
    want = pm.partition_model(tail, off - TAIL0, TAIL, pm.ids_rule(3), ids)
    whole, out = bo.guarded(torch, cuda, want[0].size, shift=9)
    got = pm.run_partition(cuda, big, BIG, off, pm.ids_rule(3), ids, None, out)
    assert got["first"] == want[4] and got["byte"] == want[5]
    same(got["part_out"], want[3], (kind, "part_out"))
    same(got["out_off"], want[1], (kind, "out_off"))
    same(got["index"], want[2], (kind, "index"))
    same(out.cpu().numpy(), want[0], (kind, "bytes"))
    assert bo.guards_intact(torch, whole, out), kind
