"""The RALLEDATA producers, the check / select kernels and the archive device paths with byte offset
2^32 inside the tiles they work on (k2h_ralledata.hip, k2h_ralledata_recs.hip,
k2h_ralledata_check.hip, k2h_archive_dev.hip): these kernels keep block-relative quantities in 32
bits and absolute offsets in 64, and only an offset whose high half is non-zero shows a cast on
the wrong side of that split.

Scenarios and form models: big_offsets.py.  Inputs cross the line in one LINE + 256 KiB buffer of
which only the last 512 KiB are written (the technique of
test_csr_tiles.py::test_tile_straddles_byte_offset_2_pow_32); outputs cross it behind about 8000
ballast records of half a MiB each, whose blobs are compared on the device (a strided
torch.equal) while the tail is compared byte for byte on the host.

Expected values never come from the device code: oracle.build_ralledata (pinned by
tests/golden/ralledata.json), ralle_recs_model, ralle_check_model, the host archive scan with its
offsets moved, and the oracle's hashes.  Every output is sentinel- or canary-filled first.

The CPU tests prove, per scenario, which tile holds the line, that it takes the form its row
claims, and that it has offsets on both sides of the line.
"""
import ctypes

import numpy as np
import pytest

import big_offsets as bo
import csr_scenarios as cs
import ralle_check_model as rm
import ralle_recs_model as rr
from big_offsets import BIG, GAP, LINE, TAIL, TAIL0

from k2hash_amd import _native, archive


# =========================================================================================== CPU
def both_sides(values):
    v = np.asarray(values, np.int64)
    return bool((v < LINE).any()) and bool((v > LINE).any())


def test_gather_model_constants_are_the_kernel_s():
    ok, got = bo.constants_match_source()
    assert ok, got
    assert rm.SEL_TILE == 256 and rm.TILE == 64 and rr.R == 64
    assert TAIL0 < LINE < BIG and BIG - TAIL == TAIL0 and 4 * GAP == bo.SLACK


@pytest.mark.parametrize("kind", ["staged", "group"])
def test_csr_inputs_reach_their_form(kind):
    """Row 1: each stream's own offset LINE lies inside tile 1, which takes the form claimed, in
    the KV launch and in the four-stream launch."""
    parts, offs = bo.csr_inputs(kind)
    assert bo.csr_image(parts, offs).size == TAIL      # every stream inside the written part, none overlapping
    for streams in (offs[:2] + [None, None], offs):
        tiles = bo.gather_tiles(streams)
        assert [t["form"] for t in tiles] == ["staged", kind, "staged"]
        t = tiles[1]
        assert (t["hull"] > bo.kGatherPool) == (kind == "group")
        for o in streams:
            if o is not None:
                assert bo.holds_line(int(o[t["r0"]]), int(o[t["r0"] + t["nr"]]))
                assert both_sides(o[t["r0"] + 1:t["r0"] + t["nr"]])   # records' own offsets on either side
    if kind == "group":   # the 5000-byte values are copied from beyond the line
        assert all(offs[1][i] > LINE and offs[1][i + 1] - offs[1][i] == 5000 for i in (100, 110, 120))


def test_build_ballast_reaches_the_line():
    """Row 2: the staged tile whose blob span holds the line, the group tile above it, and the
    staged tile whose first blob offset gets an addend above 2^32 from the value stream alone."""
    b = bo.BuildBallast()
    forms = [t["form"] for t in b.tiles]
    assert set(forms[:b.tile_a]) == {"group"} and forms[b.tile_a:] == ["staged", "group", "staged"]
    assert b.V // 128 < 4200                       # trips of an 8-lane group over one ballast value
    a, g, c = (b.tiles[t] for t in (b.tile_a, b.tile_b, b.tile_c))
    span = b.blob_off[a["r0"]:a["r0"] + a["nr"] + 1]
    assert int(span[0]) == b.ballast_bytes == LINE - 2048 and bo.holds_line(int(span[0]), int(span[-1]))
    assert both_sides(span[1:-1])                  # blob_off entries either side of the line
    assert b.blob_off[g["r0"]] > LINE
    big = b.voff[g["r0"] + 1:g["r0"] + g["nr"] + 1] - b.voff[g["r0"]:g["r0"] + g["nr"]]
    assert sorted(big.tolist())[-6:] == [5000] * 3 + [300 << 10] * 3
    # tile C is staged and o_first's addend b - f of the value stream no longer fits 32 bits
    assert int(b.voff[c["r0"]]) - int(b.voff[0]) > LINE and int(b.koff[c["r0"]]) - int(b.koff[0]) < LINE
    assert b.total > LINE + (900 << 10)


@pytest.mark.parametrize("form", ["staged", "direct"])
@pytest.mark.parametrize("kind", ["import", "archive"])
def test_recs_inputs_reach_their_form(kind, form):
    """Row 3: block 1's file hull holds the line and takes the form claimed."""
    s = bo.RecsInput(kind, form)
    assert s.image().size == TAIL
    blk, lo, hi = bo.line_block(s.segs)
    assert blk == 1 and s.forms[1] == form and TAIL0 <= lo and hi <= BIG
    starts = [o for seg in s.segs[rr.R:2 * rr.R] if seg is not None for o, n in seg if n]
    assert both_sides(starts)
    assert all((a is None) == (b is None) for a, b in zip(s.segs, s.local_segs))


def test_import_ballast_reaches_the_line():
    """Row 4: block A staged with its blobs across the line, block B direct above it."""
    b = bo.ImportBallast()
    assert all(s is not None for s in b.segs)
    assert set(b.forms[:b.block_a]) == {"direct"} and b.forms[b.block_a:] == ["staged", "direct", "staged"]
    a0 = b.block_a * rr.R
    span = b.blob_off[a0:a0 + rr.R + 1]
    assert int(span[0]) == b.ballast_bytes == LINE - 2048 and bo.holds_line(int(span[0]), int(span[-1]))
    assert both_sides(span[1:-1])
    assert b.blob_off[a0 + rr.R] > LINE and b.total == b.blob_off[-1] > LINE
    assert b.VL // 128 < 4200 and b.size < LINE   # the file itself stays below the line: row 3 has the inputs


@pytest.mark.parametrize("kind", ["staged", "direct"])
def test_check_streams_reach_their_form(oracle, kind):
    """Row 5: tile 1 holds the line, takes the form claimed, and carries every planted status
    behind the line."""
    buf, off, planted = bo.check_stream(oracle, kind)
    assert bo.image([(off[0], buf)]).size == TAIL
    forms = rm.tile_forms(0, off, BIG)
    assert forms[1] == kind and bo.holds_line(off[64], off[128]) and both_sides(off[65:128])
    assert all(64 <= i < 128 and off[i] > LINE for i in planted)
    assert set(planted.values()) == set(range(2, 7)) | ({rm.BAD_SPAN} if kind == "direct" else set())
    status = rm.expected(oracle, host_bytes(buf), [x - off[0] for x in off], None, 0, bo.CHECK_RANGE)[0]
    assert all(status[i] == s for i, s in planted.items())
    assert (status[64:128] == rm.OK).sum() > 50


@pytest.mark.parametrize("kind", ["tabled", "searched"])
def test_select_inputs_reach_their_form(kind):
    """Row 6: tile 0 holds the line and looks its pieces up the way claimed; behind the line the
    kernel's delta (source offset minus place in the tile's kept bytes) needs more than 32 bits."""
    data, off, keep = bo.select_input(kind)
    assert bo.image([(int(off[0]), data)]).size == TAIL
    t = bo.select_tiles(off, keep, BIG)[0]
    assert t["form"] == kind and bo.holds_line(int(off[0]), int(off[256])) and both_sides(off[1:256])
    delta = [int(off[j]) - t["x"][j] for j in range(256) if keep[j]]
    assert sum(d >> 32 == 1 for d in delta) > 50 and sum(d >> 32 == 0 for d in delta) > 5
    assert 100 < keep.sum() < 200


def test_select_ballast_reaches_the_line():
    """Row 7: the first tail tile's destination span holds the line; out_off on either side."""
    b = bo.SelectBallast()
    tiles = bo.select_tiles(b.off, b.keep, b.size)
    assert {t["form"] for t in tiles[:b.line_tile]} == {"searched"}
    t = tiles[b.line_tile]
    assert t["form"] == "tabled" and t["dst0"] == b.ballast_bytes == LINE - 4096
    assert bo.holds_line(t["dst0"], t["dst0"] + t["bytes"])
    assert both_sides(b.out_off.astype(np.int64)) and b.kept_bytes > LINE
    assert b.index.size == b.out_off.size - 1 and b.NB < b.index.size < b.n


@pytest.mark.parametrize("case", bo.SCAN_CASES)
def test_scan_files_reach_the_line(case):
    """Row 8: where tail record 100 lies against the line, per case; and the hand-built head
    record and the shifted tail against the host scan of the same layout with a short value."""
    s = bo.ScanFile(case)
    r = s.line_rec()
    o, ko, kl = int(r["offset"]), int(r["key_off"]), int(r["key_len"])
    if case == "header":
        assert o + 24 < LINE < o + 64
    elif case.startswith("prefix-"):
        assert o == LINE - int(case[-1])
    elif case == "record-at-line":
        assert o == LINE
    else:
        assert ko < LINE < ko + kl
    assert s.size <= BIG and s.want.size == 1 + bo.SCAN_TAIL_N and s.size // 104 * 36 > 512 << 20  # past kScratchKeep
    assert int(s.want[0]["val_len"]) == s.val_len > LINE - (64 << 10)
    short = bo.set_all_header(s.command, len(bo.HEAD_KEY), 1000) + bo.HEAD_KEY + bytes(1000) + s.tail
    host = archive.scan(short)
    want = np.concatenate([bo.set_all_rec(len(bo.HEAD_KEY), 1000),
                           bo.shift_archive(s.tail_recs, 104 + len(bo.HEAD_KEY) + 1000)])
    assert host.size == want.size and all((host[n] == want[n]).all() for n in archive.REC_DTYPE.names)
    if case == "decoys":
        assert s.tail.count(bo.MAGIC) >= bo.SCAN_TAIL_N + 2 * 50
        decoy = [int(x["offset"]) for x in s.want[1:][1::4]]
        assert both_sides(decoy)    # records whose next offset is searched for, targets above 2^32


def test_hash_ranges_reach_the_line():
    """Row 9 and the off < p arm."""
    s, n = bo.line_ranges()
    for L in bo.RANGE_LENS:
        assert (LINE - L, L) in set(zip(s.tolist(), n.tolist())) and (LINE, L) in set(zip(s.tolist(), n.tolist()))
        assert L == 1 or any(a < LINE < a + b - 1 for a, b in zip(s.tolist(), n.tolist()) if b == L)
    assert {int(x) for x in cs.pads(np.array(bo.RANGE_LENS))} >= {0, 15}
    assert TAIL0 <= s.min() and (s + n).max() <= BIG
    s, n = bo.near_start_ranges()
    p = cs.pads(n)
    assert {(int(a), int(b)) for a, b in zip(s, p)} == {(a, b) for a in range(16) for b in range(16)}
    assert (s < p).sum() > 100 and (s == p).sum() >= 16 and (s > p).sum() > 100 and (s + n).max() <= 64


# =========================================================================================== GPU
@pytest.fixture(scope="module")
def device_memory(cuda):
    """Every test here that allocates gigabytes asks for this: what the tests free stays with
    torch's caching allocator, so that the next test reuses it (a fresh 4.3 GB allocation can cost
    more than the test itself), and goes back to the device once, when the module ends."""
    import torch
    yield
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big(cuda, device_memory):
    """The LINE + 256 KiB buffer every first-offset test shares; freed when the module ends."""
    t = bo.big_buffer(cuda)
    yield t
    del t


@pytest.fixture(scope="module")
def zeros(cuda, device_memory):
    """LINE + 256 KiB of zero bytes: the archive file of row 8 (each run writes its head and tail
    and zeroes them again)."""
    import torch
    t = torch.zeros(BIG, dtype=torch.uint8, device=cuda)
    yield t
    del t


def host_bytes(data):
    return np.frombuffer(bytes(data), np.uint8)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, f"{bad.size} of {want.size} differ, first at {int(bad[0])}: "
                           f"{int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}")


# The ballast tests (rows 2, 4 and 7) come first: each holds two allocations of about 4.3 GB (input
# and output; the comparison goes row block by row block) and drops them before it returns; the
# two module-scoped buffers above are only created by the tests behind them, out of the same
# cached memory.  So never more than three such buffers exist at once.
@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 5])
def test_build_ralledata_output_crosses_the_line(cuda, oracle, device_memory, shift):
    """Row 2: the blobs pass output offset 2^32 inside a staged tile; a group tile and a staged
    tile follow above it.  `out` starts on a 128-byte boundary (shift 0) and 5 bytes behind one."""
    import torch

    from k2hash_amd import batch
    b = bo.BuildBallast()
    tail_v = b"".join(b.tail_vals)
    nv = b.NB * b.V
    vals = batch.synth_bytes(nv + len(tail_v), cuda, byte_off=12345)
    vals[nv:] = torch.from_numpy(host_bytes(tail_v).copy()).to(cuda)
    keys = torch.from_numpy(np.concatenate([b.ballast_keys.reshape(-1), host_bytes(b"".join(b.tail_keys))])).to(cuda)
    whole, out = bo.guarded(torch, cuda, b.total, shift)
    try:
        boff = bo.run_build(cuda, [keys, vals, None, None], [b.koff, b.voff, None, None], b.n, out, b.total)
        ref, rboff = oracle.build_ralledata(b.tail_keys, b.tail_vals)
        same(boff, b.blob_off.astype(np.uint64), "blob_off")
        same(boff[b.NB:], rboff + np.uint64(b.ballast_bytes), "blob_off of the tail")
        assert int(boff[-1]) == b.total > LINE
        assert bo.guards_intact(torch, whole, out), "bytes outside out written"
        # the ballast: values on the device, headers and keys on the host
        assert bo.rows_equal(torch, out[80 + bo.BAL_KEY:].as_strided((b.NB, b.V), (b.BLOB, 1)),
                             vals[:nv].view(b.NB, b.V))
        head = out.as_strided((b.NB, 80 + bo.BAL_KEY), (b.BLOB, 1)).cpu().numpy()
        h1, h2 = oracle.hash_fixed(b.ballast_keys, bo.BAL_KEY)
        want = np.zeros((b.NB, 10), np.uint64)
        want[:, 0], want[:, 1] = h1, h2
        want[:, 2], want[:, 3] = bo.BAL_KEY, b.V
        want[:, 6], want[:, 7], want[:, 8], want[:, 9] = 80, 80 + bo.BAL_KEY, b.BLOB, b.BLOB
        same(np.ascontiguousarray(head[:, :80]).view(np.uint64), want, "ballast headers")
        same(head[:, 80:], b.ballast_keys, "ballast keys")
        same(out[b.ballast_bytes:].cpu().numpy(), ref, "tail blobs")
    finally:
        del whole, out, vals


@pytest.mark.gpu
def test_import_ralledata_output_crosses_the_line(cuda, oracle, device_memory):
    """Row 4: hand-built ballast records, then a small TSV's records: *total and blob_off[n] above
    2^32, a staged block across the line, a direct and a staged block above it."""
    import torch

    from k2hash_amd import batch
    b = bo.ImportBallast()
    n = b.recs.shape[0]
    file = batch.synth_bytes(b.size, cuda, byte_off=777)
    file[b.tail_at:] = torch.from_numpy(host_bytes(b.tail_data).copy()).to(cuda)
    recs = torch.from_numpy(np.ascontiguousarray(b.recs).view(np.int64)).to(cuda)
    whole, out = bo.guarded(torch, cuda, b.total)
    try:
        full, boff = bo.sentinel_words(torch, cuda, n + 1)
        total = ctypes.c_uint64(0)
        _native.check(_native.batch_lib().k2h_amd_import_ralledata(
            bo._p(file), b.size, bo._p(recs), n, bo._p(out), out.numel(), bo._p(boff), ctypes.byref(total), 0,
            bo._stream()))
        torch.cuda.synchronize()
        assert total.value == b.total > LINE
        got_off = bo.words_back(torch, full, n + 1, "blob_off")
        same(got_off, b.blob_off.astype(np.uint64), "blob_off")
        assert bo.guards_intact(torch, whole, out), "bytes outside out written"
        # the ballast: values on the device; headers, keys and the two terminators on the host
        kv = 80 + bo.BAL_KEY + 1
        assert bo.rows_equal(torch, out[kv:].as_strided((b.NB, b.VL), (b.BLOB, 1)),
                             file[bo.BAL_KEY + 1:].as_strided((b.NB, b.VL), (b.STRIDE, 1)))
        head = out.as_strided((b.NB, kv), (b.BLOB, 1)).cpu().numpy()
        keys = np.zeros((b.NB, bo.BAL_KEY + 1), np.uint8)
        keys[:, :bo.BAL_KEY] = file.as_strided((b.NB, bo.BAL_KEY), (b.STRIDE, 1)).cpu().numpy()
        h1, h2 = oracle.hash_fixed(keys, bo.BAL_KEY + 1)   # key + NUL, as K2HShm::Set(const char*) hashes it
        want = np.zeros((b.NB, 10), np.uint64)
        want[:, 0], want[:, 1] = h1, h2
        want[:, 2], want[:, 3] = bo.BAL_KEY + 1, b.VL + 1
        want[:, 6], want[:, 7], want[:, 8], want[:, 9] = 80, kv, b.BLOB, b.BLOB
        same(np.ascontiguousarray(head[:, :80]).view(np.uint64), want, "ballast headers")
        same(head[:, 80:], keys, "ballast keys + NUL")
        assert not out[b.BLOB - 1:].as_strided((b.NB,), (b.BLOB,)).any(), "a ballast value's terminator"
        # the tail: the TSV's own records against the model, behind the ballast
        local = [rr.import_segments(r, len(b.tail_data)) for r in b.tail_local]
        blobs, off = rr.expected(oracle, b.tail_data, local, True)
        same(got_off[b.NB:], off + np.uint64(b.ballast_bytes), "blob_off of the tail")
        same(out[b.ballast_bytes:].cpu().numpy(), blobs, "tail blobs")
    finally:
        del whole, out, file


@pytest.mark.gpu
def test_ralledata_select_output_crosses_the_line(cuda, device_memory):
    """Row 7: every ballast blob kept and a random half of the tail: out_off on both sides of
    2^32, kept_bytes above it, the tile whose destination span holds it."""
    import torch

    from k2hash_amd import batch
    b = bo.SelectBallast()
    inp = batch.synth_bytes(b.size, cuda, byte_off=4242)
    inp[b.ballast_bytes:] = torch.from_numpy(host_bytes(b.tail).copy()).to(cuda)
    whole, out = bo.guarded(torch, cuda, b.kept_bytes)
    try:
        kept, kb, ooff, index = bo.run_select(cuda, inp, b.size, b.off, b.keep, out, b.kept_bytes)
        assert (kept, kb) == (b.index.size, b.kept_bytes) and kb > LINE
        same(ooff, b.out_off, "out_off")
        same(index, b.index, "index")
        assert bo.guards_intact(torch, whole, out), "bytes outside out written"
        assert bo.rows_equal(torch, out[:b.ballast_bytes].view(b.NB, b.STRIDE),
                             inp[:b.ballast_bytes].view(b.NB, b.STRIDE))
        wbytes, wooff, windex = rm.select_model(host_bytes(b.tail), b.off[b.NB:] - b.ballast_bytes, b.keep[b.NB:])
        same(ooff[b.NB:], wooff + np.uint64(b.ballast_bytes), "out_off of the tail")
        same(out[b.ballast_bytes:].cpu().numpy(), wbytes, "tail bytes")
    finally:
        del whole, out, inp


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["staged", "group"])
def test_build_ralledata_inputs_cross_the_line(cuda, oracle, big, kind):
    """Row 1: k2h_amd_build_ralledata, KV launch and four-stream launch, every stream's offsets
    beginning just below 2^32 of its own base pointer."""
    import torch
    parts, offs = bo.csr_inputs(kind)
    ptrs = [big[s * GAP:] for s in range(4)]
    for canary in cs.CANARIES:
        bo.load_tail(big, bo.csr_image(parts, offs, canary))
        for streams in (2, 4):
            use = [parts[s] if s < streams else None for s in range(4)]
            ref, rboff = oracle.build_ralledata(*use)
            whole, out = bo.guarded(torch, cuda, ref.size, shift=3)
            boff = bo.run_build(cuda, ptrs, [offs[s] if s < streams else None for s in range(4)], bo.CSR_N, out,
                                ref.size)
            what = (kind, streams, hex(canary))
            same(boff, rboff, what + ("blob_off",))
            same(out.cpu().numpy(), ref, what + ("blobs",))
            assert bo.guards_intact(torch, whole, out), what


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["staged", "direct"])
@pytest.mark.parametrize("kind", ["import", "archive"])
def test_recs_to_ralledata_inputs_cross_the_line(cuda, oracle, big, kind, form):
    """Row 3: k2h_amd_import_ralledata / k2h_amd_archive_ralledata over caller-supplied records
    whose block 1 has the line inside its file hull."""
    s = bo.RecsInput(kind, form)
    blobs, off = rr.expected(oracle, s.data, s.local_segs, kind == "import")
    for canary in cs.CANARIES:
        bo.load_tail(big, s.image(canary))
        res = rr.run(cuda, kind, big, s.words, oshift=5)
        rr.check_stream((kind, form, hex(canary)), res, blobs, off)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["staged", "direct"])
def test_ralledata_check_crosses_the_line(cuda, oracle, big, kind):
    """Row 5: k2h_amd_ralledata_check with blob_off[0] just below 2^32: status, route, h1 and h2
    of every blob, one blob per non-OK status behind the line."""
    buf, off, planted = bo.check_stream(oracle, kind)
    tail = bo.image([(off[0], buf)])
    bo.load_tail(big, tail)
    want = rm.expected(oracle, tail, [x - TAIL0 for x in off], TAIL, 0, bo.CHECK_RANGE)
    got = bo.run_check(cuda, big, BIG, off, bo.CHECK_RANGE)
    for name, g, w in zip(("status", "route", "h1", "h2"), got, want):
        same(g, w, (kind, name))
    assert all(got[0][i] == s for i, s in planted.items())
    behind = [i for i in range(len(off) - 1) if off[i] > LINE]
    assert len(set(want[1][behind].tolist())) >= 3 and (want[2][behind] != 0).sum() > 50   # routes and hashes there


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tabled", "searched"])
def test_ralledata_select_input_crosses_the_line(cuda, big, kind):
    """Row 6: k2h_amd_ralledata_select reading a random half of blobs that lie across 2^32."""
    import torch
    data, off, keep = bo.select_input(kind)
    tail = bo.image([(int(off[0]), data)])
    bo.load_tail(big, tail)
    wbytes, wooff, windex = rm.select_model(tail, off - TAIL0, keep, TAIL)
    whole, out = bo.guarded(torch, cuda, wbytes.size)
    kept, kb, ooff, index = bo.run_select(cuda, big, BIG, off, keep, out, wbytes.size)
    assert (kept, kb) == (windex.size, wbytes.size)
    same(ooff, wooff, (kind, "out_off"))
    same(index, windex, (kind, "index"))
    same(out.cpu().numpy(), wbytes, (kind, "bytes"))
    assert bo.guards_intact(torch, whole, out), kind


def key_hashes(oracle, data, recs, base=0, nul=False):
    """The oracle's h1 / h2 of every record's key (REC_DTYPE rows; data starts at offset base)."""
    h1, h2 = np.zeros(recs.size, np.uint64), np.zeros(recs.size, np.uint64)
    for i, r in enumerate(recs):
        k = bytes(data[int(r["key_off"]) - base:int(r["key_off"]) - base + int(r["key_len"])]) + (b"\0" if nul else b"")
        assert len(k) == int(r["key_len"]) + nul
        if k:
            h1[i], h2[i] = oracle.k2h_hash(k), oracle.k2h_second_hash(k)
    return h1, h2


@pytest.mark.gpu
@pytest.mark.parametrize("case", bo.SCAN_CASES)
def test_archive_scan_crosses_the_line(cuda, oracle, zeros, case):
    """Row 8: k2h_amd_archive_scan_prehash_device over a real chained file above 4 GiB -- one
    record with a value of zero bytes, then 200 records around the line; afterwards a small scan
    (the scratch, grown past its keep size, was freed and is grown again)."""
    import torch
    s = bo.ScanFile(case)
    head = torch.from_numpy(host_bytes(s.head).copy()).to(cuda)
    tail = torch.from_numpy(host_bytes(s.tail).copy()).to(cuda)
    zeros[:head.numel()] = head
    zeros[s.tail_at:s.size] = tail
    try:
        n, recs, h1, h2 = bo.run_scan_prehash(cuda, zeros, s.size, s.want.size)
    finally:
        zeros[:head.numel()] = 0
        zeros[s.tail_at:s.size] = 0
        torch.cuda.synchronize()
    assert n == 1 + bo.SCAN_TAIL_N
    for name in archive.REC_DTYPE.names:
        same(recs[name], s.want[name], (case, name))
    w1, w2 = key_hashes(oracle, s.tail, s.tail_recs)
    same(h1[1:], w1, (case, "h1"))
    same(h2[1:], w2, (case, "h2"))
    assert (int(h1[0]), int(h2[0])) == (oracle.k2h_hash(bo.HEAD_KEY), oracle.k2h_second_hash(bo.HEAD_KEY))
    small, a, b = archive.scan_prehash_device(tail)
    got = archive.recs_to_numpy(small)
    assert got.size == s.tail_recs.size
    for name in archive.REC_DTYPE.names:
        same(got[name], s.tail_recs[name], (case, "small scan", name))
    same(a.cpu().numpy().view(np.uint64), w1, (case, "small scan h1"))
    same(b.cpu().numpy().view(np.uint64), w2, (case, "small scan h2"))


def hash_call(cuda, n, call):
    """call(h1 pointer, h2 pointer) into sentinel-filled outputs: (h1, h2) on the host."""
    import torch
    f1, h1 = bo.sentinel_words(torch, cuda, n)
    f2, h2 = bo.sentinel_words(torch, cuda, n)
    _native.check(call(bo._p(h1), bo._p(h2)))
    torch.cuda.synchronize()
    return bo.words_back(torch, f1, n, "h1"), bo.words_back(torch, f2, n, "h2")


def archive_rows(torch, cuda, starts, lens):
    rows = np.zeros(starts.size, archive.REC_DTYPE)
    rows["key_off"], rows["key_len"] = starts, lens
    return rows, torch.from_numpy(rows.view(np.int64).reshape(-1, archive.REC_WORDS).copy()).to(cuda)


def oracle_of(oracle, keys, variant):
    return (np.array([oracle.k2h_hash(k, variant) for k in keys], np.uint64),
            np.array([oracle.k2h_second_hash(k, variant) for k in keys], np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("std", [False, True], ids=["builtin", "std"])
def test_prehash_and_ranges_cross_the_line(cuda, oracle, big, std):
    """Row 9: k2h_amd_archive_prehash, k2h_amd_import_prehash and k2h_amd_hash_ranges over keys
    that end just below 2^32, begin on it and hold it."""
    import torch
    lib = _native.batch_lib()
    starts, lens = bo.line_ranges()
    n = starts.size
    tail = np.frombuffer(bo._bytes(bo._rng(9), TAIL, lo=1), np.uint8).copy()
    bo.load_tail(big, tail)
    keys = [tail[s - TAIL0:s - TAIL0 + ln].tobytes() for s, ln in zip(starts.tolist(), lens.tolist())]
    raw, cstr = oracle_of(oracle, keys, int(std)), oracle_of(oracle, [k + b"\0" for k in keys], int(std))
    flags = _native.K2H_AMD_FLAG_STD_FNV if std else 0
    _rows, d_rows = archive_rows(torch, cuda, starts, lens)
    got = hash_call(cuda, n, lambda a, b: lib.k2h_amd_archive_prehash(bo._p(big), BIG, bo._p(d_rows), n, a, b, None,
                                                                      None, flags, bo._stream()))
    same(got[0], raw[0], "archive h1"), same(got[1], raw[1], "archive h2")
    irecs = np.stack([starts, lens, starts + lens, np.zeros(n, np.int64)], 1)
    d_irecs = torch.from_numpy(np.ascontiguousarray(irecs)).to(cuda)
    got = hash_call(cuda, n, lambda a, b: lib.k2h_amd_import_prehash(bo._p(big), BIG, bo._p(d_irecs), n, a, b, flags,
                                                                     bo._stream()))
    same(got[0], cstr[0], "import h1"), same(got[1], cstr[1], "import h2")
    d_s, d_n = torch.from_numpy(starts).to(cuda), torch.from_numpy(lens).to(cuda)
    for want, f in ((raw, flags), (cstr, flags | _native.K2H_AMD_FLAG_CSTR)):
        got = hash_call(cuda, n, lambda a, b: lib.k2h_amd_hash_ranges(bo._p(big), bo._p(d_s), bo._p(d_n), n, a, b, f,
                                                                      bo._stream()))
        same(got[0], want[0], ("ranges h1", f)), same(got[1], want[1], ("ranges h2", f))


@pytest.mark.gpu
@pytest.mark.parametrize("std", [False, True], ids=["builtin", "std"])
def test_archive_prehash_keys_at_the_file_s_start(cuda, oracle, std):
    """k2h_amd_archive_prehash over caller-supplied records with key_off 0..15 x key lengths 1..32
    on a 64-byte file: a key that starts fewer than p bytes into the file has nothing in front of
    it to read (hash_raw_checked's chunk0_from_bytes arm)."""
    import torch
    lib = _native.batch_lib()
    starts, lens = bo.near_start_ranges()
    n = starts.size
    payload = oracle.gen_bytes(64, byte_off=99)
    keys = [payload[s:s + ln].tobytes() for s, ln in zip(starts.tolist(), lens.tolist())]
    want = oracle_of(oracle, keys, int(std))
    _rows, d_rows = archive_rows(torch, cuda, starts, lens)
    flags = _native.K2H_AMD_FLAG_STD_FNV if std else 0
    for shift, canary in zip((0, 5), cs.CANARIES):
        file = cs.place(cuda, payload, shift, canary)
        got = hash_call(cuda, n, lambda a, b: lib.k2h_amd_archive_prehash(bo._p(file), 64, bo._p(d_rows), n, a, b,
                                                                          None, None, flags, bo._stream()))
        same(got[0], want[0], ("h1", shift)), same(got[1], want[1], ("h2", shift))
