"""A RALLEDATA stream split into parts (include/k2hash_amd.h section 4b'':
k2h_amd_ralledata_partition; k2h_ralledata_part.hip) against the model of ralle_part_model.py:
bytes, out_off, index, part_out, part_first and part_byte.

The model is one sequential pass; on the CPU it is held against what the library already
offers for the same split (ralle_check_model.select_model once per part) and its OWNER rule
against the transliterated range test of K2HShm::GetElementListToBinary
(ralle_check_model.is_target).  Expected values never come from the device code, and every
device output is sentinel-filled or guard-filled first.
"""
import ctypes
import json

import numpy as np
import pytest

from conftest import GOLDEN

import big_offsets as bo
import ralle_check_model as rm
import ralle_part_model as pm

from k2hash_amd import _native, ralledata

T = pm.TILE
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def golden():
    recs = json.loads((GOLDEN / "ralledata.json").read_text())["records"]
    return [bytearray(bytes.fromhex(r["blob"])) for r in recs]


def _rng(*salt):
    return np.random.default_rng([7700 + int(x) for x in salt])


def raw_blobs(rng, lens):
    """Blobs of arbitrary bytes (the first 8 are the stored hash a hash rule reads)."""
    return [bytearray(rng.integers(0, 256, int(x), dtype=np.uint8).tobytes()) for x in lens]


def draw_ids(rng, n, parts, p_out=0.15):
    """Ids from [0, parts) and, with probability p_out, values at or above parts."""
    ids = rng.integers(0, parts, n).astype(np.uint32)
    bad = rng.random(n) < p_out
    ids[bad] = rng.choice(np.array([parts, parts + 1, 0x7FFFFFFF, pm.NONE], np.uint32), int(bad.sum()))
    return ids


GOLDEN_RULES = {"ids": pm.ids_rule(3), "owner": pm.owner_rule(5, 2), "mask": pm.mask_rule(0xF, 16)}


# ------------------------------------------------------------------------------------- CPU
def test_model_is_one_select_per_part(golden):
    """partition_model = the concatenation over p of select_model(keep = part == p)."""
    rng = _rng(1)
    streams = [(rm.join(golden, lead=b"lead!"), GOLDEN_RULES["mask"], None),
               (rm.join(golden), GOLDEN_RULES["owner"], None),
               (rm.join(raw_blobs(rng, rng.integers(0, 30, 500))), pm.ids_rule(5), draw_ids(rng, 500, 5))]
    for (buf, off), rule, ids in streams:
        n = len(off) - 1
        consider = (rng.random(n) < 0.8).astype(np.uint8)
        data, ooff, index, part, first, byte = pm.partition_model(buf, off, len(buf), rule, ids, consider)
        assert 0 < (part == pm.NONE).sum() < n
        datas, offs, idxs = [], [np.zeros(1, np.uint64)], []
        for p in range(rule.parts):
            d, o, ix = rm.select_model(np.frombuffer(bytes(buf), np.uint8), off, part == p)
            assert first[p] == sum(x.size for x in idxs) and byte[p] == sum(x.size for x in datas)
            datas.append(d)
            offs.append(o[1:] + np.uint64(byte[p]))
            idxs.append(ix)
        assert (data == np.concatenate(datas)).all() and (ooff == np.concatenate(offs)).all()
        assert (index == np.concatenate(idxs)).all()
        assert first[-1] == index.size and byte[-1] == data.size


@pytest.mark.parametrize("span", [1, 2])
@pytest.mark.parametrize("max_hash", [3, 5, 7, 256])
def test_owner_parts_are_the_reference_ranges(golden, max_hash, span):
    """Every non-wrapping part holds exactly the hashes is_target accepts for
    Range(p * span, max_hash, span); the short last part takes m in [p * span, max_hash)."""
    rng = _rng(2)
    hashes = [rm.get(b, 0, rm.F_HASH) for b in golden]
    hashes += [int(x) for x in rng.integers(0, 1 << 64, 6000, dtype=np.uint64)]
    hashes += [M64 - k for k in range(16)]
    rule = pm.owner_rule(max_hash, span)
    assert rule.parts == -(-max_hash // span)
    part = [pm.hash_part(h, rule) for h in hashes]
    short = 0
    for p in range(rule.parts):
        members = {h for h, q in zip(hashes, part) if q == p}
        assert members, (max_hash, span, p)
        if p * span + span <= max_hash:
            assert members == {h for h in hashes if rm.is_target(h, rm.Range(p * span, max_hash, span))}
        else:
            short += 1
            assert members == {h for h in hashes if p * span <= h % max_hash < max_hash}
    assert short == (1 if max_hash % span else 0)
    assert (max_hash, span) != (5, 2) or (rule.parts == 3 and short == 1)


def _host_stream(oracle):
    buf, off = rm.stream_of(oracle, rm.records(oracle, 4, seed=1))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64)


def test_partition_argument_validation(oracle):
    """Judged on the host before any device is touched: the same answers with and without a
    GPU, each case with its own message."""
    lib = _native.batch_lib()
    buf, off = _host_stream(oracle)
    n = off.size - 1
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    ids = np.zeros(n, np.uint32)
    out, ooff = np.full(buf.size, 0xEE, np.uint8), np.full(n + 1, 0xEE, np.uint64)
    first, byte = (ctypes.c_uint64 * 257)(), (ctypes.c_uint64 * 257)()
    part = lib.k2h_amd_ralledata_partition
    msg = lambda: bytes(lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL))  # noqa: E731
    R = _native.PartRule
    ok_ids, ok_mask = R(pm.IDS, 3, 0, 0, 0), R(pm.MASK, 4, 0, 0, 3)

    def call(rule=ok_mask, blobs=p(buf), boff=p(off), nn=n, pids=None, o=None, oo=None, f=first, b=byte):
        return part(blobs, buf.size, boff, nn, ctypes.byref(rule) if rule is not None else None, pids, None, o,
                    buf.size if o is not None else 0, oo, None, None, f, b, None)
    cases = {
        "NULL rule": dict(rule=None),
        "NULL part_first": dict(f=None),
        "NULL part_byte": dict(b=None),
        "unknown rule kind": dict(rule=R(3, 4, 0, 0, 0)),
        "parts must be": dict(rule=R(pm.MASK, 0, 0, 0, 3)),
        "needs part_ids": dict(rule=ok_ids),
        "part_ids given": dict(pids=p(ids)),
        "max_hash is 0": dict(rule=R(pm.OWNER, 1, 0, 1, 0)),
        "span is 0": dict(rule=R(pm.OWNER, 1, 4, 0, 0)),
        "ceil(max_hash / span)": dict(rule=R(pm.OWNER, 2, 5, 2, 0)),
        "NULL blobs": dict(blobs=None),
        "NULL blob_off": dict(boff=None),
        "out given without out_off": dict(o=p(out)),
    }
    texts = set()
    for needle, kw in cases.items():
        assert call(**kw) == _native.K2H_AMD_EINVAL, needle
        assert needle.encode() in msg() and msg().startswith(b"ralledata_partition: "), (needle, msg())
        texts.add(msg())
    assert len(texts) == len(cases)
    assert call(rule=R(pm.MASK, 257, 0, 0, 3)) == _native.K2H_AMD_EINVAL and b"parts must be" in msg()
    assert call(rule=R(pm.OWNER, 4, 5, 2, 0)) == _native.K2H_AMD_EINVAL and b"ceil" in msg()
    assert (out == 0xEE).all() and (ooff == 0xEE).all()
    # n == 0: answered without a device, both host arrays zeroed; the rule is still judged
    for rule, pids in ((ok_mask, None), (ok_ids, p(ids)), (R(pm.OWNER, 3, 5, 2, 0), None)):
        for k in range(257):
            first[k] = byte[k] = 7
        assert call(rule=rule, blobs=None, boff=None, nn=0, pids=pids) == _native.K2H_AMD_OK
        assert list(first)[:rule.parts + 1] == [0] * (rule.parts + 1) == list(byte)[:rule.parts + 1]
        assert first[rule.parts + 1] == 7 and byte[rule.parts + 1] == 7
    assert call(rule=None, blobs=None, boff=None, nn=0) == _native.K2H_AMD_EINVAL


def test_partition_public_names():
    import inspect

    import k2hash_amd
    assert hasattr(k2hash_amd, "partition_ralledata") and "partition_ralledata" in k2hash_amd.__all__
    assert len(_native.SIGNATURES["k2h_amd_ralledata_partition"][1]) == 15
    assert ralledata.Partitioned._fields == ("blobs", "blob_off", "index", "part_of", "part_first", "part_byte",
                                             "kept", "kept_bytes")
    sig = inspect.signature(ralledata.partition_ralledata).parameters
    assert [k for k, v in sig.items() if v.kind is v.KEYWORD_ONLY] == [
        "ids", "owner", "mask", "consider", "out", "count_only", "want_index", "want_parts", "stream"]
    assert (ralledata.PART_MAX, ralledata.PART_NONE) == (pm.PART_MAX, pm.NONE) == (
        _native.K2H_AMD_PART_MAX, _native.K2H_AMD_PART_NONE)
    assert (_native.K2H_AMD_PART_IDS, _native.K2H_AMD_PART_OWNER, _native.K2H_AMD_PART_MASK) == (
        pm.IDS, pm.OWNER, pm.MASK)
    assert ctypes.sizeof(_native.PartRule) == 32
    assert T % 256 == 0 and 80 < pm.LONG     # a header-sized blob never takes the whole block


# ------------------------------------------------------------------------------------- GPU
PAD = 64


def place(cuda, buf, shift=0, canary=0xA5):
    """buf on the device, starting `shift` bytes past a 16-byte boundary, canary bytes around it."""
    import torch
    whole = np.full(PAD + shift + len(buf) + PAD, canary, np.uint8)
    whole[PAD + shift:PAD + shift + len(buf)] = np.frombuffer(bytes(buf), np.uint8)
    t = torch.from_numpy(whole).to(cuda)
    assert t.data_ptr() % 16 == 0
    return t[PAD + shift:PAD + shift + len(buf)]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, f"{bad.size} of {want.size} differ, first at {int(bad[0])}: "
                           f"{int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}")


def same_tables(got, want, what):
    data, ooff, index, part, first, byte = want
    assert got["first"] == first, (what, "part_first", got["first"], first)
    assert got["byte"] == byte, (what, "part_byte", got["byte"], byte)
    same(got["part_out"], part, (what, "part_out"))
    same(got["out_off"], ooff, (what, "out_off"))
    same(got["index"], index, (what, "index"))


def against_model(cuda, buf, off, rule, what, ids=None, consider=None, size=None, shift=0, out_shift=0):
    """The call over the stream placed `shift` bytes past a 16-byte boundary, into an `out` of
    exactly the expected bytes `out_shift` bytes past one; everything compared with the model."""
    import torch
    size = len(buf) if size is None else size
    want = pm.partition_model(buf, off, size, rule, ids, consider)
    whole, out = bo.guarded(torch, cuda, want[0].size, shift=out_shift)
    got = pm.run_partition(cuda, place(cuda, buf, shift), size, off, rule, ids, consider, out)
    same_tables(got, want, what)
    same(out.cpu().numpy(), want[0], (what, "bytes"))
    assert bo.guards_intact(torch, whole, out), (what, "bytes outside out written")
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(GOLDEN_RULES))
def test_reference_fixture(cuda, golden, kind):
    buf, off = rm.join(golden)
    rule = GOLDEN_RULES[kind]
    ids = np.array([i % 4 for i in range(48)], np.uint32) if kind == "ids" else None   # id 3: left out
    data, ooff, index, part, first, byte = against_model(cuda, buf, off, rule, kind, ids=ids, shift=3, out_shift=5)
    assert first[-1] == (36 if kind == "ids" else 48)
    assert sum(first[p + 1] > first[p] for p in range(rule.parts)) >= 3


SHAPES = ["n1-kept", "n1-out", "T-1", "T", "T+1", "2T+1", "parts1", "parts256", "all-last", "all-out"]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_smallest_shapes(cuda, shape):
    import torch
    rng = _rng(3, SHAPES.index(shape))
    n = {"n1-kept": 1, "n1-out": 1, "T-1": T - 1, "T": T, "2T+1": 2 * T + 1}.get(shape, T + 1)
    if shape == "parts256":
        rule, ids = pm.mask_rule(0xFF, 256), None
        buf, off = rm.join(raw_blobs(rng, rng.integers(80, 121, n)))
    else:
        parts = 1 if shape == "parts1" else 4
        rule = pm.ids_rule(parts)
        ids = {"n1-out": np.full(n, parts, np.uint32), "all-out": np.full(n, pm.NONE, np.uint32),
               "all-last": np.full(n, parts - 1, np.uint32)}.get(shape)
        if ids is None:
            ids = draw_ids(rng, n, parts, p_out=0.0 if shape == "n1-kept" else 0.15)
        buf, off = rm.join(raw_blobs(rng, rng.integers(0, 41 if n > 1 else 1, n) + (7 if n == 1 else 0)))
    if shape in ("n1-out", "all-out"):
        # kept = 0: out_off[0] = 0 and nothing of an out that has room is touched
        whole, out = bo.guarded(torch, cuda, 64)
        got = pm.run_partition(cuda, place(cuda, buf), len(buf), off, rule, ids, None, out)
        same_tables(got, pm.partition_model(buf, off, len(buf), rule, ids), shape)
        assert got["first"] == [0] * (rule.parts + 1) == got["byte"] and got["out_off"].tolist() == [0]
        assert bool((whole == bo.OUT_FILL).all())
        return
    data, ooff, index, part, first, byte = against_model(cuda, buf, off, rule, shape, ids=ids, out_shift=1)
    if shape == "parts256":
        assert sum(first[p + 1] == first[p] for p in range(256)) >= 1 and first[-1] == n
    if shape == "all-last":
        assert first == [0] * (rule.parts) + [n]


@pytest.mark.gpu
@pytest.mark.parametrize("out_shift", [0, 9])
def test_tiny_blobs_share_destination_pieces(cuda, out_shift):
    """0-5 byte blobs: several of them, of different tiles and on either side of a part
    boundary, lie in one 16-byte piece of out."""
    rng = _rng(4)
    n = 3 * T + 7
    buf, off = rm.join(raw_blobs(rng, rng.integers(0, 6, n)), lead=b"abc")
    ids = draw_ids(rng, n, 3, p_out=0.1)
    data, ooff, index, part, first, byte = against_model(cuda, buf, off, pm.ids_rule(3), "tiny", ids=ids, shift=3,
                                                         out_shift=out_shift)
    for p in (1, 2):        # the piece that holds the part boundary holds blobs of both parts
        assert byte[p] % 16 and first[p] - 2 >= first[p - 1] and first[p] + 2 <= first[p + 1]
    tiles_of_piece = {}
    for r, i in enumerate(index):
        tiles_of_piece.setdefault((int(ooff[r]) + out_shift) // 16, set()).add(int(i) // T)
    assert max(len(v) for v in tiles_of_piece.values()) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("out_shift", [0, 9])
def test_mixed_lengths(cuda, out_shift):
    """Header-sized to 280-byte blobs with three of 5000 bytes and two of 300 KiB (the whole
    block moves those), a misaligned source, 16 parts by MASK."""
    rng = _rng(5)
    n = T + 300
    lens = rng.integers(80, 281, n)
    lens[[10, T - 1, T + 17]] = 5000
    lens[[500, T + 200]] = 300 << 10
    assert (lens >= pm.LONG).sum() == 5
    buf, off = rm.join(raw_blobs(rng, lens), lead=b"five!")
    data, ooff, index, part, first, byte = against_model(cuda, buf, off, pm.mask_rule(0xF, 16), "mixed", shift=0,
                                                         out_shift=out_shift)
    assert all(first[p + 1] > first[p] for p in range(16)) and off[0] % 16 == 5


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ids", "mask", "owner"])
def test_left_out_blobs(cuda, kind):
    """A decreasing span, an end past size, a 79-byte blob under a hash rule, consider[i] = 0
    and part_ids[i] >= parts: all K2H_AMD_PART_NONE, their neighbours placed correctly."""
    rng = _rng(6)
    n = 200
    lens = rng.integers(80, 200, n)
    lens[50] = 79
    buf, off = rm.join(raw_blobs(rng, lens))
    off[120] = off[119] - 30          # blob 119 decreases; blob 120 starts inside blob 118
    size = off[-1] - 10               # the last blob ends past size
    consider = np.ones(n, np.uint8)
    consider[[7, 8, 150]] = 0
    rule = {"ids": pm.ids_rule(5), "mask": pm.mask_rule(0x7, 8), "owner": pm.owner_rule(5, 2)}[kind]
    ids = None
    if kind == "ids":
        ids = draw_ids(rng, n, 5, p_out=0.0)
        ids[[30, 31]] = [5, pm.NONE]
    data, ooff, index, part, first, byte = against_model(cuda, buf, off, rule, kind, ids=ids, consider=consider,
                                                         size=size, shift=7, out_shift=3)
    out = [7, 8, 150, 119, n - 1] + ([30, 31] if kind == "ids" else [50])
    assert all(part[i] == pm.NONE for i in out) and (part == pm.NONE).sum() == len(out)
    assert part[120] != pm.NONE and part[118] != pm.NONE and (part[50] != pm.NONE) == (kind == "ids")


@pytest.mark.gpu
def test_count_only_and_out_too_small(cuda):
    import torch
    rng = _rng(7)
    n = T + 50
    buf, off = rm.join(raw_blobs(rng, rng.integers(80, 140, n)))
    rule = pm.mask_rule(0x3, 4)
    want = pm.partition_model(buf, off, len(buf), rule)
    t = place(cuda, buf)
    got = pm.run_partition(cuda, t, len(buf), off, rule, out=None)
    assert got["first"] == want[4] and got["byte"] == want[5]
    same(got["part_out"], want[3], "count only: part_out")
    got = pm.run_partition(cuda, t, len(buf), off, rule, out=None, want_parts=False)
    assert got["first"] == want[4] and got["byte"] == want[5]
    # one byte short: EINVAL, both host arrays set, out / out_off / index keep their fill
    whole, out = bo.guarded(torch, cuda, want[0].size)
    got = pm.run_partition(cuda, t, len(buf), off, rule, out=out, out_cap=want[0].size - 1,
                           expect=_native.K2H_AMD_EINVAL)
    assert got["first"] == want[4] and got["byte"] == want[5]
    assert b"out_cap" in _native.batch_lib().k2h_amd_strerror(_native.K2H_AMD_EINVAL)
    assert bool((whole == bo.OUT_FILL).all())
    # the wrapper: two-call sizing, and an out that is too small raises
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    res = ralledata.partition_ralledata(t, d_off, 4, mask=0x3, want_parts=True)
    torch.cuda.synchronize()
    assert (res.kept, res.kept_bytes, res.part_first, res.part_byte) == (want[4][-1], want[5][-1], want[4], want[5])
    same(res.blobs.cpu().numpy(), want[0], "wrapper bytes")
    same(res.blob_off.cpu().numpy().view(np.uint64), want[1], "wrapper out_off")
    same(res.index.cpu().numpy().view(np.uint64), want[2], "wrapper index")
    same(res.part_of.cpu().numpy().view(np.uint32), want[3], "wrapper part_of")
    cnt = ralledata.partition_ralledata(t, d_off, 4, mask=0x3, count_only=True)
    assert cnt.blobs is None and cnt.part_of is None and cnt.part_byte == want[5] and cnt.kept == want[4][-1]
    with pytest.raises(_native.NativeError, match="out_cap"):
        ralledata.partition_ralledata(t, d_off, 4, mask=0x3, out=out[:-1])
    with pytest.raises(ValueError, match="exactly one"):
        ralledata.partition_ralledata(t, d_off, 4, mask=0x3, owner=(4, 1))


def _parts_as_blobs(res):
    """Per part, the list of its blobs' bytes (a Partitioned or Selected on the device)."""
    data, ooff = res.blobs.cpu().numpy().tobytes(), res.blob_off.cpu().numpy()
    return [data[int(ooff[r]):int(ooff[r + 1])] for r in range(len(ooff) - 1)]


@pytest.mark.gpu
def test_stability_and_dedup_commute(cuda, golden):
    """The 48 reference blobs twice, shuffled: dedup then partition(MASK) equals, part for part,
    partition(MASK) then dedup of each part -- every identity's blobs stay together, in order."""
    import torch
    order = np.random.default_rng(48).permutation(96)
    buf, off = rm.join([(golden + golden)[i] for i in order])
    t, d_off = place(cuda, buf, 3), torch.tensor(off, dtype=torch.int64, device=cuda)
    keep, _by, dropped = ralledata.dedup_ralledata(t, d_off)
    assert 0 < dropped < 48
    a = ralledata.partition_ralledata(t, d_off, 16, mask=0xF, consider=keep)
    b = ralledata.partition_ralledata(t, d_off, 16, mask=0xF)
    torch.cuda.synchronize()
    assert a.kept == 96 - dropped and b.kept == 96
    a_blobs = _parts_as_blobs(a)
    nonempty = 0
    for p in range(16):
        want = a_blobs[a.part_first[p]:a.part_first[p + 1]]
        lo, hi = b.part_first[p], b.part_first[p + 1]
        if lo == hi:
            assert not want
            continue
        nonempty += 1
        sub = b.blobs[b.part_byte[p]:b.part_byte[p + 1]]
        sub_off = (b.blob_off[lo:hi + 1] - b.part_byte[p]).contiguous()
        k2, _by, _d = ralledata.dedup_ralledata(sub, sub_off)
        sel = ralledata.select_ralledata(sub, sub_off, k2)
        torch.cuda.synchronize()
        assert _parts_as_blobs(sel) == want, p
        assert all(rm.get(x, 0, rm.F_HASH) & 0xF == p for x in want)
    assert nonempty >= 8


@pytest.mark.gpu
def test_tsv_to_lock_partitions(cuda):
    """import_file_to_ralledata, check_ralledata, partition_ralledata(mask): every blob of part p
    parses to a stored hash with hash & 0xF == p, and the parts hold exactly the OK blobs."""
    import torch
    tsv = (GOLDEN / "import" / "random.tsv").read_bytes()
    file = torch.from_numpy(np.frombuffer(tsv, np.uint8).copy()).to(cuda)
    blobs, boff = ralledata.import_file_to_ralledata(file, "tsv")
    res = ralledata.check_ralledata(blobs, boff)
    ok = res.status == ralledata.OK
    part = ralledata.partition_ralledata(blobs, boff, 16, mask=0xF, consider=ok, want_parts=True)
    torch.cuda.synchronize()
    src, soff, okh = blobs.cpu().numpy().tobytes(), boff.cpu().numpy(), ok.cpu().numpy()
    want = sorted(src[int(soff[i]):int(soff[i + 1])] for i in range(len(okh)) if okh[i])
    got = _parts_as_blobs(part)
    assert part.kept == len(want) > 100 and sorted(got) == want
    for p in range(16):
        for b in got[part.part_first[p]:part.part_first[p + 1]]:
            assert ralledata.parse_blob(b).hash & 0xF == p
    assert sum(part.part_first[p + 1] > part.part_first[p] for p in range(16)) == 16
    of = part.part_of.cpu().numpy()
    assert ((of >= 0) == okh).all()


@pytest.mark.gpu
def test_scratch_is_reused_across_calls(cuda):
    """Two calls back to back on one stream, the first call's copy kernel still queued or running
    when the second is made: a large n at 256 parts, then a small n at 3 parts whose tables land
    where the first call's copy reads its own."""
    import torch
    rng = _rng(9)
    big_n = 4 * T + 5
    buf1, off1 = rm.join(raw_blobs(rng, rng.integers(80, 200, big_n)))
    buf2, off2 = rm.join(raw_blobs(rng, rng.integers(0, 50, 10)))
    ids2 = np.array([2, 0, 1, 3, 2, 2, 0, 1, 1, 0], np.uint32)
    w1 = pm.partition_model(buf1, off1, len(buf1), pm.mask_rule(0xFF, 256))
    w2 = pm.partition_model(buf2, off2, len(buf2), pm.ids_rule(3), ids2)
    t1, o1 = place(cuda, buf1), torch.tensor(off1, dtype=torch.int64, device=cuda)
    t2, o2 = place(cuda, buf2), torch.tensor(off2, dtype=torch.int64, device=cuda)
    d_ids2 = torch.from_numpy(ids2.view(np.int32)).to(cuda)
    out1 = torch.full((w1[0].size,), 0xC3, dtype=torch.uint8, device=cuda)
    out2 = torch.full((w2[0].size,), 0xC3, dtype=torch.uint8, device=cuda)
    r1 = ralledata.partition_ralledata(t1, o1, 256, mask=0xFF, out=out1)
    r2 = ralledata.partition_ralledata(t2, o2, 3, ids=d_ids2, out=out2)
    torch.cuda.synchronize()
    for r, w, what in ((r1, w1, "first"), (r2, w2, "second")):
        assert (r.part_first, r.part_byte) == (w[4], w[5]), what
        same(r.blobs.cpu().numpy(), w[0], (what, "bytes"))
        same(r.blob_off.cpu().numpy().view(np.uint64), w[1], (what, "out_off"))
        same(r.index.cpu().numpy().view(np.uint64), w[2], (what, "index"))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fuzz(cuda, seed):
    rng = _rng(10, seed)
    n = 5 * T + 3
    kind = int(rng.integers(0, 3))
    lens = rng.integers(0, 401, n)
    buf, off = rm.join(raw_blobs(rng, lens), lead=bytes(int(rng.integers(0, 16))))
    consider = (rng.random(n) < 0.85).astype(np.uint8)
    ids = None
    if kind == pm.IDS:
        rule = pm.ids_rule(int(rng.integers(2, 40)))
        ids = draw_ids(rng, n, rule.parts)
    elif kind == pm.OWNER:
        rule = pm.owner_rule(int(rng.integers(2, 100)), int(rng.integers(1, 4)))
    else:
        rule = pm.mask_rule(int(rng.integers(1, 1 << 12)), int(rng.integers(2, 257)))
    data, ooff, index, part, first, byte = against_model(cuda, buf, off, rule, f"fuzz {seed} kind {kind}", ids=ids,
                                                         consider=consider, shift=seed, out_shift=5 * seed)
    assert n // 2 < first[-1] < n
