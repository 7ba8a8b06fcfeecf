"""Superseded duplicates of a RALLEDATA stream (include/k2hash_amd.h section 4b':
k2h_amd_ralledata_dedup; k2h_ralledata_dedup.hip) against the model of ralle_dedup_model.py,
entry for entry: keep, by and dropped.

The model is a sequential pass with a dict from identity to the last index seen.  That its
rule is safe -- the table after the kept blobs equals the table after all of them, from every
prior state of a key -- is shown on the CPU against a transliteration of
K2HShm::SetElementByBinArray (lib/k2hshmdirect.cc:377-473); libk2hash itself is not built here,
so parity with it is a restatement.  Blobs are the oracle's (oracle_build_ralledata, pinned to
the reference-built fixture tests/golden/ralledata.json by tests/test_ralledata.py), header
fields mutated with struct.pack_into.  Expected values never come from the device code, and
every device output is sentinel-filled first.
"""
import ctypes
import json

import numpy as np
import pytest

from conftest import GOLDEN

import big_offsets as bo
import ralle_check_model as rm
import ralle_dedup_model as dm
from ralle_dedup_model import NONE

from k2hash_amd import _native, ralledata


@pytest.fixture(scope="module")
def golden():
    recs = json.loads((GOLDEN / "ralledata.json").read_text())["records"]
    return [bytearray(bytes.fromhex(r["blob"])) for r in recs]


# ------------------------------------------------------------------------------------- CPU
def test_model_on_reference_fixture(golden):
    """The 48 reference blobs hold 48 different keys; laid down twice, each first copy without
    attrs is superseded by its second copy and each with attrs stays."""
    assert len(golden) == 48
    buf, off = rm.join(golden)
    keep, by, dropped = dm.dedup_model(buf, off)
    assert keep.all() and (by == NONE).all() and dropped == 0
    buf, off = rm.join(golden + golden)
    keep, by, dropped = dm.dedup_model(buf, off)
    has_attrs = np.array([rm.get(b, 0, rm.F_ALEN) != 0 for b in golden])
    assert 0 < has_attrs.sum() < 48
    assert (keep[:48] == has_attrs).all() and keep[48:].all() and dropped == 48 - has_attrs.sum()
    assert (by[:48] == np.arange(48, 96)).all() and (by[48:] == NONE).all()


PTS = (1000, 500)
OLDER, NEWER = (900, 0), (1000, 500)   # an mtime older than pts; one pts does not pass (:402 is <=)


def _prior_states(ident):
    """The states a key's element can be in before the stream arrives."""
    val = b"prior-value"
    return {
        "absent": {},
        "no-attrs": {ident: (val, None, None)},
        "mtime-older": {ident: (val, None, dm.encode_attrs(OLDER))},
        "mtime-newer": {ident: (val, None, dm.encode_attrs(NEWER))},
        "expired": {ident: (val, None, dm.encode_attrs(NEWER, expired=True))},
        "attrs-without-mtime": {ident: (val, None, dm.encode_attrs(None))},
    }


def _random_stream(oracle, seed, n=24, nkeys=3):
    rng = np.random.default_rng(seed)
    keys = [b"key-%d" % int(k) for k in rng.integers(0, nkeys, n)]
    vals = [b"" if rng.random() < 0.15 else b"v%d" % i for i in range(n)]
    attrs = []
    for i in range(n):
        u = rng.random()
        if u < 0.6:
            attrs.append(b"")
        elif u < 0.7:
            attrs.append(dm.encode_attrs(None, salt=i))
        elif u < 0.8:
            attrs.append(dm.encode_attrs((950, i), expired=True, salt=i))
        else:
            attrs.append(dm.encode_attrs((int(rng.integers(850, 1100)), i), salt=i))
    return dm.blobs_of(oracle, keys, vals, None, attrs)


def test_kept_blobs_replay_to_the_same_table(oracle):
    """Whole stream against the model's kept blobs, from every prior state of key-0; and the
    control: keeping each identity's FIRST attrs-free blob instead leaves another table for
    some stream, so the replay can tell streams apart."""
    k0 = dm.blobs_of(oracle, [b"key-0"], [b"x"])[0]
    ident0 = (rm.get(k0, 0, rm.F_HASH), rm.get(k0, 0, rm.F_SUBHASH), b"key-0")
    control_differs = total_dropped = 0
    for seed in range(40):
        blobs = _random_stream(oracle, seed)
        keep, _by, dropped = dm.dedup_model(*rm.join(blobs))
        kept = [b for b, k in zip(blobs, keep) if k]
        assert len(kept) == len(blobs) - dropped
        total_dropped += dropped
        # the control's filter: the model over the reversed stream, so the first of a pair survives
        rkeep = dm.dedup_model(*rm.join(blobs[::-1]))[0][::-1]
        control = [b for b, k in zip(blobs, rkeep) if k]
        for name, prior in _prior_states(ident0).items():
            whole = dm.replay(blobs, prior, PTS)
            assert dm.replay(kept, prior, PTS) == whole, (seed, name)
            control_differs += dm.replay(control, prior, PTS) != whole
    assert total_dropped > 100
    assert control_differs > 0


def test_replay_follows_the_reference_branches(oracle):
    """The transliteration's own branches, one by one, on a single key."""
    def blob(val, attrs=b""):
        return dm.blobs_of(oracle, [b"k"], [val], None, [attrs])[0]
    plain = blob(b"v1")
    ident = (rm.get(plain, 0, rm.F_HASH), rm.get(plain, 0, rm.F_SUBHASH), b"k")
    st = _prior_states(ident)
    assert dm.replay([plain], st["absent"], PTS) == {ident: (b"v1", None, None)}
    assert dm.replay([plain], st["no-attrs"], PTS) == {ident: (b"v1", None, None)}
    assert dm.replay([plain], st["expired"], PTS) == {ident: (b"v1", None, None)}
    assert dm.replay([plain], st["attrs-without-mtime"], PTS) == {ident: (b"v1", None, None)}
    assert dm.replay([plain], st["mtime-newer"], PTS) == st["mtime-newer"]           # :402-405
    assert dm.replay([plain], st["mtime-older"], PTS) == st["mtime-older"]           # :421-427
    a_new, a_old = dm.encode_attrs((950, 0)), dm.encode_attrs((900, 0))
    assert dm.replay([blob(b"v2", a_new)], st["mtime-older"], PTS) == {ident: (b"v2", None, a_new)}
    assert dm.replay([blob(b"v2", a_old)], st["mtime-older"], PTS) == st["mtime-older"]   # :416-419, <=
    assert dm.replay([blob(b"")], st["no-attrs"], PTS) == {}                         # key only: :438, :446
    empty = bytearray(plain)
    for f in (rm.F_KLEN, rm.F_VLEN):
        rm.put(empty, 0, f, 0)
    assert not dm.set_element_by_bin_array({}, empty, PTS)                           # :351


def _host_stream(oracle):
    buf, off = rm.stream_of(oracle, rm.records(oracle, 4, seed=1))
    return np.frombuffer(bytes(buf), np.uint8).copy(), np.array(off, np.uint64)


def test_dedup_argument_validation(oracle):
    """Judged on the host before any device is touched: the same answers with and without a
    GPU, each with its own message."""
    lib = _native.batch_lib()
    buf, off = _host_stream(oracle)
    n = off.size - 1
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    keep, by = np.full(n, 0xEE, np.uint8), np.zeros(n, np.uint64)
    dropped = ctypes.c_uint64(7)
    dedup = lib.k2h_amd_ralledata_dedup
    msg = lambda: lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL)  # noqa: E731
    assert dedup(None, 0, None, 0, None, None, None, ctypes.byref(dropped), None) == _native.K2H_AMD_OK
    assert dropped.value == 0
    assert dedup(None, 0, None, 0, None, None, None, None, None) == _native.K2H_AMD_OK
    dropped.value = 7
    assert dedup(p(buf), buf.size, p(off), n, None, None, p(by), ctypes.byref(dropped),
                 None) == _native.K2H_AMD_EINVAL
    assert b"NULL keep" in msg()
    assert dedup(None, buf.size, p(off), n, None, p(keep), None, None, None) == _native.K2H_AMD_EINVAL
    assert b"NULL blobs" in msg()
    assert dedup(p(buf), buf.size, None, n, None, p(keep), None, None, None) == _native.K2H_AMD_EINVAL
    assert b"NULL blob_off" in msg()
    assert dedup(p(buf), buf.size, p(off), (1 << 32) - 1, None, p(keep), None, None, None) == _native.K2H_AMD_EINVAL
    assert b"2^32 - 2" in msg() and b"32-bit" in msg()
    assert (keep == 0xEE).all()
    texts = set()
    for args in ((p(buf), buf.size, p(off), n, None, None, None, None, None),
                 (None, buf.size, p(off), n, None, p(keep), None, None, None),
                 (p(buf), buf.size, None, n, None, p(keep), None, None, None),
                 (p(buf), buf.size, p(off), 1 << 40, None, p(keep), None, None, None)):
        assert dedup(*args) == _native.K2H_AMD_EINVAL
        texts.add(bytes(msg()))
    assert len(texts) == 4 and all(t.startswith(b"ralledata_dedup: ") for t in texts)


def test_dedup_public_names():
    import k2hash_amd
    assert hasattr(k2hash_amd, "dedup_ralledata") and "dedup_ralledata" in k2hash_amd.__all__
    assert len(_native.SIGNATURES["k2h_amd_ralledata_dedup"][1]) == 9
    assert ralledata.NO_LATER == NONE
    import inspect
    assert inspect.signature(ralledata.route_ralledata).parameters["dedup"].default is False
    assert dm.RESOLVE_BLOCK % dm.WAVE == 0 and dm.RESOLVE_BLOCK > 64   # the edge stream's two runs are two places


# ---- the streams of the GPU tests, and (CPU) that each is what its test claims
def _pair_hash(blobs, h=0x1234, sub=0x5678):
    return [dm.set_hash(b, h, sub) for b in blobs]


KEY_LENS = (1, 15, 16, 17, 33, 255, 4096)


def _differing_keys(L):
    """A base key of L bytes and its variants that differ in one byte only: the first, the
    last, byte 15 and byte 16 from the end (where the key has them)."""
    base = bytes((7 * i + 3) & 0xFF for i in range(L))
    places = sorted({0, L - 1} | {L - d for d in (15, 16) if L - d >= 0})
    out = [base]
    for at in places:
        k = bytearray(base)
        k[at] ^= 0x80
        out.append(bytes(k))
    return out


def _differing_stream(oracle):
    """Every key of _differing_keys twice, all under ONE stored hash and subhash (so equal
    lengths always reach the byte compare), with 0-15 slack bytes in each blob."""
    keys = [k for L in KEY_LENS for k in _differing_keys(L)]
    order = np.random.default_rng(5).permutation(2 * len(keys))
    keys = [(keys + keys)[i] for i in order]
    blobs = _pair_hash(dm.blobs_of(oracle, keys, [b"v%d" % i for i in range(len(keys))]))
    return rm.join(dm.at_odd_offsets(blobs, seed=3))


def test_differing_stream_covers_every_alignment(oracle):
    buf, off = _differing_stream(oracle)
    keep, by, dropped = dm.dedup_model(buf, off)
    n = len(off) - 1
    assert dropped == n // 2 and keep.sum() == n // 2       # every key twice, no two keys equal
    assert {(o + 80) % 16 for o in off[:-1]} == set(range(16))
    assert len({rm.get(buf, o, rm.F_HASH) for o in off[:-1]}) == 1


def _edge_stream(oracle, W):
    """Stored hashes are small integers, so the sorted order is known: a run of three equal
    identities at sorted positions 62-64 (a wave edge) and at W-2..W (a block edge), every
    other position a key of its own; laid down in a shuffled stream order."""
    npos = 2 * W + 70
    group = list(range(npos))
    for lo in (62, W - 2):
        group[lo + 1] = group[lo + 2] = lo
    keys = [b"edge-key-%05d" % g for g in group]
    order = np.random.default_rng(11).permutation(npos)
    blobs = dm.blobs_of(oracle, [keys[p] for p in order], [b"v%d" % i for i in range(npos)])
    for b, p in zip(blobs, order):
        dm.set_hash(b, group[p])
    return rm.join(blobs), [group[p] for p in order]


def test_edge_stream_puts_the_runs_on_the_edges(oracle):
    W = dm.RESOLVE_BLOCK
    (buf, off), hashes = _edge_stream(oracle, W)
    srt = sorted(range(len(hashes)), key=lambda i: (hashes[i], i))   # the stable sort's order
    for lo in (62, W - 2):
        assert [hashes[srt[p]] for p in range(lo - 1, lo + 4)] == [lo - 1, lo, lo, lo, lo + 3]
    assert 62 // dm.WAVE != 64 // dm.WAVE and (W - 2) // W != W // W
    keep, by, dropped = dm.dedup_model(buf, off)
    assert dropped == 4 and keep.sum() == len(hashes) - 4


ATTRS_CASES = {"OOAO": "..A.", "AA": "AA", "OAOO": ".A..", "OO-last-key-only": ".k"}


def _attrs_stream(oracle, pattern):
    n = len(pattern)
    vals = [b"" if c == "k" else b"val-%d" % i for i, c in enumerate(pattern)]
    attrs = [dm.encode_attrs((900 + i, 0)) if c == "A" else b"" for i, c in enumerate(pattern)]
    return rm.join(dm.blobs_of(oracle, [b"the-key"] * n, vals, None, attrs))


ATTRS_KEEP = {"OOAO": [0, 1, 1, 1], "AA": [1, 1], "OAOO": [1, 1, 0, 1], "OO-last-key-only": [0, 1]}


def test_attrs_cases_model(oracle):
    for case, pattern in ATTRS_CASES.items():
        keep, by, dropped = dm.dedup_model(*_attrs_stream(oracle, pattern))
        assert keep.tolist() == ATTRS_KEEP[case] and dropped == ATTRS_KEEP[case].count(0), case
        assert by.tolist() == list(range(1, len(pattern))) + [NONE], case


def _planted_stream(oracle):
    """Eight copies of one blob, a ninth identity, and among them one non-participant of each
    kind whose first bytes are the copies' (so it shares their stored hash): returns the
    stream, consider, and {index: what was planted}."""
    blobs = dm.blobs_of(oracle, [b"dup-key"] * 14 + [b"other"], [b"v%02d" % i for i in range(15)])
    planted = {}

    def plant(i, what, fn):
        blobs[i] = fn(blobs[i])
        planted[i] = what
    plant(2, "BAD_SPAN", lambda b: b[:79])
    plant(4, "EMPTY", lambda b: [rm.put(b, 0, f, 0) for f in (rm.F_KLEN, rm.F_VLEN)] and b)
    plant(6, "NO_KEY", lambda b: rm.put(b, 0, rm.F_KLEN, 0) or b)
    plant(8, "BAD_RANGE", lambda b: rm.put(b, 0, rm.F_KPOS, 79) or b)
    plant(10, "ZERO", lambda b: bytearray())
    planted[12] = "NOT_CONSIDERED"
    planted[13] = "NOT_CONSIDERED"          # the last copy: it must supersede nothing
    consider = np.ones(15, np.uint8)
    consider[[12, 13]] = 0
    return rm.join(blobs), consider, planted


def test_planted_stream_model(oracle):
    (buf, off), consider, planted = _planted_stream(oracle)
    keep, by, dropped = dm.dedup_model(buf, off, consider=consider)
    live = [i for i in range(14) if i not in planted]
    assert live == [0, 1, 3, 5, 7, 9, 11]
    assert [int(keep[i]) for i in live] == [0] * 6 + [1] and keep[14] == 1 and dropped == 6
    assert all(keep[i] == 0 and by[i] == NONE for i in planted)
    assert [int(by[i]) for i in live[:-1]] == live[1:] and by[11] == NONE


# ------------------------------------------------------------------------------------- GPU
PAD = 64


def place(cuda, buf, shift=0, canary=0xA5, tail_pad=PAD):
    """buf on the device, starting `shift` bytes past a 16-byte boundary, canary bytes around
    it (tail_pad = 0: the tensor ends with buf's last byte)."""
    import torch
    whole = np.full(PAD + shift + len(buf) + tail_pad, canary, np.uint8)
    whole[PAD + shift:PAD + shift + len(buf)] = np.frombuffer(bytes(buf), np.uint8)
    t = torch.from_numpy(whole).to(cuda)
    assert t.data_ptr() % 16 == 0
    return t[PAD + shift:PAD + shift + len(buf)]


def run_dedup(cuda, t, size, off, consider=None):
    """k2h_amd_ralledata_dedup into sentinel-filled outputs: (keep, by, dropped) on the host."""
    import torch
    n = len(off) - 1
    d_off = torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)
    kw, keep = bo.guarded(torch, cuda, n, fill=0xEE)
    full, by = bo.sentinel_words(torch, cuda, n)
    cons = None if consider is None else torch.from_numpy(np.asarray(consider, np.uint8)).to(cuda)
    dropped = ctypes.c_uint64(0xDEAD)
    _native.check(_native.batch_lib().k2h_amd_ralledata_dedup(
        bo._p(t), size, bo._p(d_off), n, None if cons is None else bo._p(cons), bo._p(keep), bo._p(by),
        ctypes.byref(dropped), bo._stream()))
    torch.cuda.synchronize()
    assert bo.guards_intact(torch, kw, keep, 0xEE), "bytes outside keep written"
    return keep.cpu().numpy(), bo.words_back(torch, full, n, "by"), int(dropped.value)


def assert_same(got, want, what):
    for name, g, w in zip(("keep", "by"), got[:2], want[:2]):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {name} differs at blob {int(bad[0])}: got {g[bad[0]]}, want {w[bad[0]]}"
    assert got[2] == want[2], f"{what}: dropped {got[2]}, want {want[2]}"


def against_model(cuda, buf, off, what, shift=0, consider=None, tail_pad=PAD):
    want = dm.dedup_model(buf, off, consider=consider)
    got = run_dedup(cuda, place(cuda, buf, shift, tail_pad=tail_pad), len(buf), off, consider)
    assert_same(got, want, what)
    return want


@pytest.mark.gpu
def test_reference_fixture(cuda, golden):
    buf, off = rm.join(golden)
    keep, by, dropped = against_model(cuda, buf, off, "fixture")
    assert keep.all() and dropped == 0
    keep, by, dropped = against_model(cuda, *rm.join(golden + golden), "fixture twice")
    assert dropped == sum(rm.get(b, 0, rm.F_ALEN) == 0 for b in golden)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["n1", "same-key", "subhash-differs", "key-is-prefix"])
def test_smallest_shapes(cuda, oracle, case):
    if case == "n1":
        blobs = dm.blobs_of(oracle, [b"only"], [b"v"])
    elif case == "same-key":
        blobs = dm.blobs_of(oracle, [b"same", b"same"], [b"v1", b"v2"])
    elif case == "subhash-differs":
        blobs = dm.blobs_of(oracle, [b"same", b"same"], [b"v1", b"v2"])
        dm.set_hash(blobs[1], sub=rm.get(blobs[1], 0, rm.F_SUBHASH) ^ 1)
    else:
        blobs = _pair_hash(dm.blobs_of(oracle, [b"prefix-of-the-other", b"prefix-of-the-other-key"], [b"v1", b"v2"]))
    keep, by, dropped = against_model(cuda, *rm.join(blobs), case, shift=3)
    assert dropped == (1 if case == "same-key" else 0)


@pytest.mark.gpu
def test_hashes_that_differ_in_high_bits_only(cuda, oracle):
    """The pairs are sorted by the hash's low bits, so blobs whose stored hashes differ in a
    high bit alone are neighbours: same key, subhash and low bits, and still two identities."""
    blobs = dm.blobs_of(oracle, [b"one-key"] * 6, [b"v%d" % i for i in range(6)])
    h = rm.get(blobs[0], 0, rm.F_HASH)
    for i, flip in enumerate((0, 1 << 63, 1 << 40, 0, 1 << 63, 1 << 40)):
        dm.set_hash(blobs[i], h ^ flip)
    keep, by, dropped = against_model(cuda, *rm.join(blobs), "high bits")
    assert keep.tolist() == [0, 0, 0, 1, 1, 1] and by.tolist()[:3] == [3, 4, 5] and dropped == 3


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 9])
def test_where_keys_differ(cuda, oracle, shift):
    buf, off = _differing_stream(oracle)
    against_model(cuda, buf, off, f"differing keys, shift {shift}", shift=shift)


@pytest.mark.gpu
def test_runs_across_wave_and_block_edges(cuda, oracle):
    (buf, off), _hashes = _edge_stream(oracle, dm.RESOLVE_BLOCK)
    keep, by, dropped = against_model(cuda, buf, off, "edges")
    assert dropped == 4


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(ATTRS_CASES))
def test_attrs_rule(cuda, oracle, case):
    buf, off = _attrs_stream(oracle, ATTRS_CASES[case])
    keep, by, dropped = against_model(cuda, buf, off, case)
    assert keep.tolist() == ATTRS_KEEP[case] and by.tolist() == list(range(1, len(keep))) + [NONE]


@pytest.mark.gpu
def test_non_participants_share_the_stored_hash(cuda, oracle):
    (buf, off), consider, planted = _planted_stream(oracle)
    keep, by, dropped = against_model(cuda, buf, off, "planted", shift=5, consider=consider)
    assert dropped == 6 and all(keep[i] == 0 for i in planted)
    # the same stream with everything considered: the copies at 12 and 13 now count
    keep, by, dropped = against_model(cuda, buf, off, "planted, all considered", shift=5)
    assert dropped == 8 and keep[13] == 1


@pytest.mark.gpu
def test_last_key_ends_with_the_buffer(cuda, oracle):
    """The key segment is the last thing in each blob, and the tensor ends with the stream."""
    blobs = [rm.value_before_key(b)
             for b in dm.blobs_of(oracle, [b"k" * 37, b"other-key", b"k" * 37], [b"v1", b"v2", b"v3"])]
    buf, off = rm.join(blobs)
    assert rm.get(blobs[-1], 0, rm.F_KPOS) + rm.get(blobs[-1], 0, rm.F_KLEN) == len(blobs[-1])
    for shift in (0, 7):
        keep, by, dropped = against_model(cuda, buf, off, "key at the end", shift=shift, tail_pad=0)
        assert keep.tolist() == [0, 1, 1] and by[0] == 2


@pytest.mark.gpu
def test_long_runs(cuda, oracle):
    blobs = dm.blobs_of(oracle, [b"one-key-many-times"] * 3000, [b"v%d" % i for i in range(3000)])
    keep, by, dropped = against_model(cuda, *rm.join(blobs), "3000 copies")
    assert dropped == 2999 and keep[-1] == 1
    # 300 different keys of one length under one stored hash and subhash: every lane walks to the run's end
    blobs = _pair_hash(dm.blobs_of(oracle, [b"distinct-%04d" % i for i in range(300)], [b"v"] * 300))
    keep, by, dropped = against_model(cuda, *rm.join(blobs), "300 keys, one hash")
    assert dropped == 0 and keep.all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fuzz(cuda, oracle, seed):
    rng = np.random.default_rng(100 + seed)
    pool = [bytes(rng.integers(0, 256, int(rng.integers(1, 70)), dtype=np.uint8)) for _ in range(600)]
    keys = [pool[int(k)] for k in rng.integers(0, 600, 5000)]
    vals = [bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8)) for _ in range(5000)]
    attrs = [dm.encode_attrs((int(rng.integers(0, 9)), 0)) if rng.random() < 0.3 else b"" for _ in range(5000)]
    blobs = dm.blobs_of(oracle, keys, vals, None, attrs)
    for i in rng.integers(0, 5000, 40):          # a few hash collisions between different keys
        dm.set_hash(blobs[int(i)], 77, 99)
    for i in rng.integers(0, 5000, 250):         # and copies of a key that differ in the hash's top bit alone
        dm.set_hash(blobs[int(i)], rm.get(blobs[int(i)], 0, rm.F_HASH) ^ (1 << 63))
    consider = (rng.random(5000) < 0.9).astype(np.uint8)
    keep, by, dropped = against_model(cuda, *rm.join(dm.at_odd_offsets(blobs, seed)), f"fuzz {seed}",
                                      shift=seed, consider=consider)
    assert 1000 < dropped < 4400


@pytest.mark.gpu
def test_tsv_to_deduplicated_blobs(cuda):
    """import_file_to_ralledata, dedup_ralledata, select_ralledata: the blobs that are left
    give the dict a loop over the lines gives, last value winning."""
    import torch
    rng = np.random.default_rng(9)
    lines = [(b"key%03d" % int(rng.integers(0, 150)), b"value-%d" % i) for i in range(1000)]
    want = {}
    for k, v in lines:
        want[k] = v
    tsv = b"".join(k + b"\t" + v + b"\n" for k, v in lines)
    file = torch.from_numpy(np.frombuffer(tsv, np.uint8).copy()).to(cuda)
    blobs, boff = ralledata.import_file_to_ralledata(file, "tsv")
    keep, by, dropped = ralledata.dedup_ralledata(blobs, boff, want_by=True)
    sel = ralledata.select_ralledata(blobs, boff, keep)
    torch.cuda.synchronize()
    assert sel.kept == len(want) and dropped == len(lines) - len(want)
    out, ooff = sel.blobs.cpu().numpy().tobytes(), sel.blob_off.cpu().numpy()
    got = {}
    for i in range(sel.kept):
        b = ralledata.parse_blob(out[int(ooff[i]):int(ooff[i + 1])])
        assert b.key not in got
        got[b.key] = b.val
    assert got == {k + b"\0": v + b"\0" for k, v in want.items()}
    model = dm.dedup_model(blobs.cpu().numpy().tobytes(), boff.cpu().numpy())
    assert_same((keep.cpu().numpy(), by.cpu().numpy().view(np.uint64), dropped), model, "tsv")
    # asynchronous form: no count, the same mask
    keep2, by2, none = ralledata.dedup_ralledata(blobs, boff, count=False)
    torch.cuda.synchronize()
    assert by2 is None and none is None and torch.equal(keep2, keep)


@pytest.mark.gpu
def test_route_ralledata_with_dedup(cuda, oracle):
    import torch
    rng = np.random.default_rng(21)
    keys = [b"route-key-%d" % int(k) for k in rng.integers(0, 60, 400)]
    blobs = dm.blobs_of(oracle, keys, [b"v%d" % i for i in range(400)])
    dm.set_hash(blobs[17], rm.get(blobs[17], 0, rm.F_HASH) ^ 4)      # BAD_HASH: neither kept nor superseding
    buf, off = rm.join(blobs)
    r = rm.Range(0, 2)
    status, route, _h1, _h2 = rm.expected(oracle, buf, off, rng=r)
    routed = ((status == rm.OK) & ((route & 1) != 0)).astype(np.uint8)
    t = place(cuda, buf)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    for dedup in (False, True):
        keep = routed & dm.dedup_model(buf, off, consider=routed)[0] if dedup else routed
        data, ooff, index = rm.select_model(buf, off, keep)
        sel, res = ralledata.route_ralledata(t, d_off, r.ctypes(), dedup=dedup)
        torch.cuda.synchronize()
        assert (res.status.cpu().numpy() == status).all()
        assert sel.kept == int(keep.sum()) and sel.kept_bytes == data.size
        assert (sel.blobs.cpu().numpy() == data).all()
        assert (sel.blob_off.cpu().numpy().view(np.uint64) == ooff).all()
        assert (sel.index.cpu().numpy().view(np.uint64) == index).all()
    assert 0 < keep.sum() < routed.sum()
    plain, _res = ralledata.route_ralledata(t, d_off, r.ctypes())      # the default is dedup=False
    assert plain.kept == int(routed.sum())


# ---- offsets across 2^32
@pytest.fixture(scope="module")
def big(cuda):
    """A LINE + 256 KiB buffer of which only the last 512 KiB are written; freed, and given
    back to the device, when the module ends."""
    import torch
    t = bo.big_buffer(cuda)
    yield t
    del t
    torch.cuda.empty_cache()


def _line_stream(oracle):
    """160 blobs over 40 keys whose blob 80 holds byte offset 2^32: absolute offsets."""
    rng = np.random.default_rng(32)
    keys = [b"line-key-%02d" % int(k) for k in rng.integers(0, 40, 160)]
    vals = [bytes(rng.integers(0, 256, int(rng.integers(0, 120)), dtype=np.uint8)) for _ in range(160)]
    buf, off = rm.join(dm.at_odd_offsets(dm.blobs_of(oracle, keys, vals), seed=8))
    first = bo.LINE - off[80] - 5
    return bytes(buf), [first + x for x in off]


def test_line_stream_has_duplicates_on_both_sides(oracle):
    buf, off = _line_stream(oracle)
    assert bo.image([(off[0], buf)]).size == bo.TAIL and bo.holds_line(off[80], off[81])
    keep, by, dropped = dm.dedup_model(buf, [x - off[0] for x in off])
    pairs = [(i, int(by[i])) for i in range(160) if by[i] != NONE]
    assert any(j < 80 for i, j in pairs) and any(i > 80 for i, j in pairs) and any(i < 80 < j for i, j in pairs)
    assert dropped == len(pairs) > 100


@pytest.mark.gpu
def test_offsets_across_4gib(cuda, oracle, big):
    buf, off = _line_stream(oracle)
    bo.load_tail(big, bo.image([(off[0], buf)]))
    want = dm.dedup_model(buf, [x - off[0] for x in off])
    assert_same(run_dedup(cuda, big, bo.BIG, off), want, "across 2^32")
