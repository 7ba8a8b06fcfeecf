"""A transaction log applied to a held RALLEDATA stream (include/k2hash_amd.h section 5c:
k2h_amd_archive_apply; k2h_archive_apply.hip) against the model of archive_apply_model.py, entry
for entry and byte for byte: out, out_off, origin, touched, counts and stop.

The model is a sequential last-writer pass.  That its rule is Load's is shown on the CPU against
the reviewed transliteration of Load with prior tables (archive_fold_model.replay), on which the
model is not built; libk2hash itself is not built here, so parity with it is a restatement.
Expected values never come from a device call, every device output is sentinel-filled and guarded
first, and both inputs stand at odd shifts from a 16-byte boundary between canaries.
"""
import ctypes
import itertools

import numpy as np
import pytest

from conftest import GOLDEN

import archive_apply_model as am
import archive_fold_model as fm
import ralle_archive_model as ra
import ralle_check_model as rm
from archive_apply_model import LEFT_OUT, SUPERSEDED, TOUCHED
from archive_fold_model import Rec
from ralle_unlink_model import layout

from k2hash_amd import _native, archive

KEY = b"the-key"
ELEVEN = tuple(x for x in fm.TWELVE if x != "ow")
EIGHT = tuple(x for x in fm.NINE if x != "ow")


def _fields(t, key):
    return tuple(x or b"" for x in t[key]) if key in t else None


# ------------------------------------------------------------------------------------- CPU
def test_rule_exhaustive_against_replay():
    """Every sequence of length 1..5 over the eleven barrier-free letters on one key, from the
    four prior states of that key: the last-writer rule leaves what Load leaves."""
    pri = fm.priors(KEY)
    letters = {(name, at): fm.letter(name, KEY, at) for name in ELEVEN for at in range(5)}
    seqs = absent = 0
    for length in range(1, 6):
        for names in itertools.product(ELEVEN, repeat=length):
            chain = [letters[(nm, at)] for at, nm in enumerate(names)]
            seqs += 1
            for pname, prior in pri.items():
                exists, v, s, a = am.final_element(chain, _fields(prior, KEY))
                want = fm.replay(chain, prior)
                assert (exists, (v or None, s or None, a or None) if exists else None) == \
                    (KEY in want, want.get(KEY)), (names, pname)
                absent += not exists
    assert seqs == sum(11 ** k for k in range(1, 6)) and absent > seqs // 4


def test_a_wrong_rule_is_told_apart():
    """The control: SET_ALL always writing S and A differs from Load on a two-letter log."""
    def wrong(r):
        return {0: r.val, 1: r.skey, 2: r.attrs} if r.type == fm.SET_ALL else am.supplies(r)
    chain = [fm.letter("set-vsa", KEY, 0), fm.letter("set-v", KEY, 1)]
    want = fm.replay(chain, {})[KEY]
    assert am.final_element(chain, None)[1:] == tuple(x or b"" for x in want) == (b"v1", b"s0", b"a0")
    assert am.final_element(chain, None, supplies=wrong)[1:] == (b"v1", b"", b"")


def _random_log(seed, n=40, nkeys=5, barriers=True):
    rng = np.random.default_rng([77, seed])
    keys = [b"key-%d" % k * (1 + k) for k in range(nkeys)]
    out = []
    for i in range(n):
        u = rng.random()
        key = keys[int(rng.integers(0, nkeys))]
        if u < 0.03:
            out.append(Rec(fm.SET_ALL, key, b"bad%d" % i, status=int(rng.integers(1, 4))))
        elif u < 0.05:
            out.append(Rec(7, key, b"bad%d" % i))
        elif u < 0.07:
            out.append(Rec(fm.SET_ALL, b"", b"nokey%d" % i))
        elif u < 0.08 and barriers:
            out.append(fm.letter("ow", key, i) if rng.random() < 0.5 else Rec(fm.RENAME, key, b"", b"", b"", b"new"))
        else:
            out.append(fm.letter(ELEVEN[int(rng.integers(0, 11))], key, i))
    prior = {k: fm.priors(k)[("absent", "v", "s", "vsa")[int(rng.integers(0, 4))]].get(k) for k in keys}
    return out, keys, {k: v for k, v in prior.items() if v is not None}, rng


def _model_of(oracle, prior, recs, consider=None):
    held, off = am.prior_held(oracle, prior)
    h1, h2 = am.rec_hashes(oracle, recs)
    return am.apply_model(held, off, None, recs, consider, h1, h2)


def test_model_random_logs_against_replay(oracle):
    """1,000 multi-key logs with skipped records, barriers and consider masks, over random prior
    tables given as a held stream: the model's output, fed into a dict, is the table Load
    leaves after the prefix before the stop."""
    stops = masked = 0
    for seed in range(1000):
        recs, keys, prior, rng = _random_log(seed)
        consider = (rng.random(len(recs)) < 0.9).astype(np.uint8) if seed % 2 else None
        m = _model_of(oracle, prior, recs, consider)
        stops += m.stop < len(recs)
        masked += consider is not None
        seen = [r for i, r in enumerate(recs[:m.stop]) if consider is None or consider[i]]
        assert am.table_of(m.out, m.out_off) == fm.replay(seen, prior), seed
        assert m.counts[0] == len(m.out_off) - 1 == len(m.origin) and m.counts[1] == len(m.out)
        assert m.counts[6] == sum(fm.participant(r) for r in seen)
    assert stops > 300 and masked == 500


def _blobs(m):
    return sorted(m.out[int(a):int(b)] for a, b in zip(m.out_off[:-1], m.out_off[1:]))


def test_split_log_applied_twice_equals_once(oracle):
    """The log cut at every point: the second half applied to the first call's output leaves the
    blobs that one call leaves."""
    for seed in range(12):
        recs, keys, prior, _rng = _random_log(seed, n=30, barriers=False)
        once = _model_of(oracle, prior, recs)
        held, off = am.prior_held(oracle, prior)
        for cut in range(len(recs) + 1):
            a, b = recs[:cut], recs[cut:]
            first = am.apply_model(held, off, None, a, None, *am.rec_hashes(oracle, a))
            second = am.apply_model(first.out, first.out_off, None, b, None, *am.rec_hashes(oracle, b))
            assert _blobs(second) == _blobs(once), (seed, cut)


def test_folds_keep_as_consider_changes_nothing(oracle):
    """consider = the fold's keep of the prefix [0, stop) gives the bytes consider = None gives."""
    dropped = 0
    for seed in range(200):
        recs, keys, prior, _rng = _random_log(seed)
        plain = _model_of(oracle, prior, recs)
        keep = np.ones(len(recs), np.uint8)
        keep[:plain.stop] = fm.fold_model(recs[:plain.stop])[0]
        dropped += int(sum(fm.participant(r) for r in recs[:plain.stop]) - keep[:plain.stop].sum())
        masked = _model_of(oracle, prior, recs, keep)
        assert masked.stop == plain.stop
        assert (masked.out, masked.out_off.tolist(), masked.origin.tolist(), masked.touched.tolist()) == \
            (plain.out, plain.out_off.tolist(), plain.origin.tolist(), plain.touched.tolist()), seed
        assert masked.counts[:6] == plain.counts[:6]
    assert dropped > 500


def test_stop_rules():
    ow, ren, put = fm.letter("ow", KEY, 1), Rec(fm.RENAME, KEY, b"", b"", b"", b"new"), fm.letter("set-v", KEY, 0)
    assert am.stop_of([put, put, put]) == 3 and am.stop_of([]) == 0
    assert am.stop_of([ow, put]) == 0 and am.stop_of([put, ren, ow]) == 1 and am.stop_of([put, put, ow]) == 2
    assert am.stop_of([put, ow._replace(status=2), ren]) == 2          # a bad status is no barrier
    assert am.stop_of([put, ow, ren], consider=[1, 0, 1]) == 2           # nor is a record not considered
    assert am.stop_of([put, ow._replace(key=b""), put]) == 1            # the key plays no part in it
    m = am.apply_model(b"", [0], None, [put, ow, fm.letter("del", KEY, 2)], None, [1, 1, 1], [2, 2, 2])
    assert m.stop == 1 and m.counts == [1, 80 + len(KEY) + 2, 0, 0, 0, 0, 1] and m.origin.tolist() == [0]


def test_every_einval_without_a_device():
    """Judged on the host before any device is touched: the same answers with and without a
    GPU, each with its own message."""
    lib = _native.batch_lib()
    na, n = 2, 3
    held, hoff = np.zeros(200, np.uint8), np.arange(na + 1, dtype=np.uint64) * 100
    file, recs = np.zeros(400, np.uint8), np.zeros(n, archive.REC_DTYPE)
    h, out, ooff = np.zeros(n, np.uint64), np.full(400, 0xEE, np.uint8), np.zeros(na + n + 1, np.uint64)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    counts = (ctypes.c_uint64 * 7)()
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    stop = ctypes.c_uint64(0)
    msg = lambda: bytes(lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL))  # noqa: E731

    def args(**kw):
        d = dict(held=p(held), hoff=p(hoff), na=na, file=p(file), recs=p(recs), n=n, h1=p(h), h2=p(h), flags=0, out=p(out),
                 ooff=p(ooff), counts=cp, stop=ctypes.byref(stop))
        d.update(kw)
        return (d["held"], held.size, d["hoff"], d["na"], None, d["file"], file.size, d["recs"], d["n"], None, d["h1"],
                d["h2"], d["flags"], d["out"], out.size, d["ooff"], None, None, d["counts"], d["stop"], None)
    for i in range(7):
        counts[i] = 7
    stop.value = 7
    nothing = dict(held=None, hoff=None, na=0, file=None, recs=None, n=0, h1=None, h2=None, out=None, ooff=None)
    assert lib.k2h_amd_archive_apply(*args(**nothing)) == 0
    assert list(counts) == [0] * 7 and stop.value == 0
    texts = set()
    cases = ((dict(counts=None), b"NULL counts"), (dict(stop=None), b"NULL stop"), (dict(held=None), b"NULL held"),
             (dict(hoff=None), b"NULL held_off"), (dict(file=None), b"NULL file"), (dict(recs=None), b"NULL recs"),
             (dict(ooff=None), b"out given without out_off"), (dict(h1=None), b"together"), (dict(h2=None), b"together"),
             (dict(flags=2), b"unknown flags"), (dict(flags=1), b"only when h1 and h2 are NULL"),
             (dict(na=(1 << 32) - 4), b"2^32 - 2"), (dict(n=(1 << 32) - 3), b"2^32 - 2"),
             (dict(na=(1 << 64) - 1, n=2), b"2^32 - 2"))
    for kw, text in cases:
        for i in range(7):
            counts[i] = 7
        assert lib.k2h_amd_archive_apply(*args(**kw)) == _native.K2H_AMD_EINVAL, kw
        assert text in msg() and msg().startswith(b"archive_apply: "), (kw, msg())
        if "counts" not in kw and "stop" not in kw:
            assert list(counts) == [0] * 7
        texts.add(msg())
    assert len(texts) == 11 and (out == 0xEE).all()
    # held NULL with na = 0 and the log's pointers NULL with n = 0 are no errors: only the pairing is judged
    assert lib.k2h_amd_archive_apply(*args(held=None, hoff=None, na=0, file=None, recs=None, n=0, h1=None)) == \
        _native.K2H_AMD_EINVAL and b"together" in msg()


def test_exports():
    import k2hash_amd
    from k2hash_amd import apply
    for name in ("apply_log", "apply_records", "Applied"):
        assert name in k2hash_amd.__all__ and getattr(k2hash_amd, name) is getattr(apply, name)
    assert apply.Applied._fields == ("blobs", "blob_off", "origin", "touched", "counts", "stop", "first_changed")
    assert (apply.APPLY_TOUCHED, apply.APPLY_SUPERSEDED, apply.APPLY_LEFT_OUT) == (TOUCHED, SUPERSEDED, LEFT_OUT)


def test_kernels_keep_the_register_budget(tmp_path):
    """Every kernel of k2h_archive_apply.hip: at most 64 VGPRs, no scratch, no spills."""
    import subprocess
    from pathlib import Path

    import test_archive_device as tad
    if not Path(tad.HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "k2h_archive_apply.s"
    subprocess.run([tad.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    f"-I{tad.ROOT / 'include'}", str(tad.CSRC / "k2h_archive_apply.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    kernels = {k: v for k, v in tad._kernel_meta(out.read_text()).items() if "apply_" in k or "ralle_place_copy" in k}
    for name in ("apply_gather_kernel", "apply_count_kernel", "apply_plan_kernel", "ralle_place_copy_kernel", "apply_build_kernel"):
        assert any(name in k for k in kernels), (name, sorted(kernels))
    for sym, f in kernels.items():
        assert f.get("vgpr_count", 999) <= 64, (sym, f.get("vgpr_count"))
        assert f.get("private_segment_fixed_size", 0) == 0, sym
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, sym


# ------------------------------------------------------------------------------------- GPU
def against_model(cuda, oracle, held, off, log, what, keep=None, consider=None, hashes="oracle", bare=None, variant=0,
                  **kw):
    """The call over (held, off) and the list of Rec `log` against the model.  hashes: "oracle"
    (the keys' own, passed as the caller's), None (computed inside the call; the model still
    uses the oracle's) or an (h1, h2) pair."""
    file, recs = am.build_log(log) if bare is None else am.bare_log(log, bare)
    seen = fm.recs_of(file, recs)
    h1, h2 = am.rec_hashes(oracle, log, variant) if hashes in ("oracle", None) else hashes
    m = am.apply_model(held, off, keep, seen, consider, h1, h2)
    given = (None, None) if hashes is None else (h1, h2)
    got = am.run_apply(cuda, held, off, recs, file, keep=keep, consider=consider, h1=given[0], h2=given[1],
                       flags=variant if hashes is None else 0, **kw)
    am.assert_applied(got, m, what)
    return got, m


def _held_of(oracle, table):
    return am.prior_held(oracle, table)


@pytest.mark.gpu
def test_boundary_sizes(cuda, oracle):
    # na = n = 0: no device work but out_off[0] = 0
    got = am.run_apply(cuda, b"", [0], np.zeros(0, archive.REC_DTYPE), b"")
    assert got[0] == 0 and got[1] == b"" and got[2].tolist() == [0] and got[5] == [0] * 7 and got[6] == 0
    # n = 0: the call is select (no identity repeats in this stream)
    blobs = ra.blobs_of(oracle, *ra.records(ra._rng(1), 600, klen=(4, 41), p_extra=0.3))
    held, off = rm.join(blobs, lead=b"\x55" * 3)
    keep = (np.random.default_rng(5).random(600) < 0.7).astype(np.uint8)
    for k in (None, keep):
        (rc, out, ooff, origin, touched, counts, stop), m = against_model(cuda, oracle, held, off, [], "n = 0", keep=k)
        data, soff, index = rm.select_model(np.frombuffer(bytes(held), np.uint8), off, np.ones(600) if k is None else k)
        assert out == data.tobytes() and (ooff == soff).all() and (origin == index).all() and stop == 0
        assert counts == [len(index), data.size, len(index), 0, 0, 0, 0]
    # na = 0 over the golden archive: 64 records of all seven types, the first barrier ends it
    f = (GOLDEN / "archive.k2har").read_bytes()
    recs = archive.scan(f)
    log = fm.recs_of(f, recs)
    h1, h2 = am.rec_hashes(oracle, log)
    m = am.apply_model(b"", [0], None, log, None, h1, h2)
    assert 0 < m.stop < 64 and m.counts[0] > 0
    am.assert_applied(am.run_apply(cuda, b"", [0], recs, f, h1=h1, h2=h2), m, "golden, caller hashes")
    am.assert_applied(am.run_apply(cuda, b"", [0], recs, f), m, "golden, hashed inside")
    # ... and with the barriers not considered: the whole file
    cons = np.array([r.type not in (fm.OW_VAL, fm.RENAME) for r in log], np.uint8)
    m = am.apply_model(b"", [0], None, log, cons, h1, h2)
    assert m.stop == 64
    am.assert_applied(am.run_apply(cuda, b"", [0], recs, f, consider=cons), m, "golden, barriers masked")


def _own_key(idx):
    """A key of its own per identity, lengths 1..100."""
    ln, k = 1 + idx % 100, idx // 100
    return (k.to_bytes(2, "little") + bytes((7 * j + idx) & 0xFF for j in range(ln)))[:ln]


@pytest.fixture(scope="module")
def exhaustive(oracle):
    """All 4,680 sequences of length 1..4 over the eight letters, each on a key of its own from
    each of the four priors: the held table, the log one key after the other, and the same
    records dealt round-robin."""
    seqs = [names for length in range(1, 5) for names in itertools.product(EIGHT, repeat=length)]
    assert len(seqs) == 4680
    table, chains = {}, []
    for idx, (names, pname) in enumerate(itertools.product(seqs, ("absent", "v", "s", "vsa"))):
        key = _own_key(idx)
        p = fm.priors(key)[pname]
        table.update(p)
        chains.append([fm.letter(nm, key, at) for at, nm in enumerate(names)])
    assert len(chains) == 18720 and len({c[0].key for c in chains}) == 18720
    flat = [r for c in chains for r in c]
    dealt = [c[at] for at in range(4) for c in chains if len(c) > at]
    assert len(flat) == len(dealt) == 72224
    return _held_of(oracle, table), flat, dealt


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["one-key-after-the-other", "round-robin"])
def test_rule_exhaustive(cuda, oracle, exhaustive, order):
    (held, off), flat, dealt = exhaustive
    log = flat if order == "one-key-after-the-other" else dealt
    got, m = against_model(cuda, oracle, held, off, log, order)
    assert m.counts[3] == 14040 and m.counts[5] > 1000 and m.counts[6] == 72224
    # the table the output leaves is Load's
    assert am.table_of(m.out, m.out_off) == fm.replay(log, am.table_of(held, off))


@pytest.mark.gpu
def test_identity_and_keys(cuda, oracle):
    base = bytes(range(40, 80))
    keys = [base, b"\x00" + base[1:], base[:-1] + b"\x00", base[:17], base[:16], base[:1], base + b"x"]
    table = {k: (b"held-" + k[:3], None, b"attr") for k in keys[::2]}
    held, off = _held_of(oracle, table)
    log = [fm.letter(("rep-v", "rep-s", "set-vs", "rep-a")[i % 4], k, i) for i, k in enumerate(keys + keys[::-1])]
    against_model(cuda, oracle, held, off, log, "first / last byte, prefixes")
    # record keys at file offsets 0..15, the file itself at every shift
    for at in range(16):
        against_model(cuda, oracle, held, off, log, f"keys from file offset {at}", bare=at, fshift=(5 * at + 1) % 16)


def _twins(hashes, log):
    """(h1, h2) arrays for `log` from {key: (h1, h2)}."""
    return (np.array([hashes[r.key][0] for r in log], np.uint64), np.array([hashes[r.key][1] for r in log], np.uint64))


@pytest.mark.gpu
def test_caller_hashes_that_collide(cuda, oracle):
    """Two identities that agree in the sorted bits only, in h1 only, in h1 and h2 only, and in
    everything but the key length or the key bytes: the walks step over the other one."""
    a = (0x1234, 9)
    same_len, other_len = (b"key-aaaa", b"key-bbbb", b"key-cccc"), (b"key-aaaa", b"key-a", b"key")
    for what, cls, keys, others in (("sorted bits only", "bits", same_len, ((0x1_0000_1234, 9), (0x2_0000_1234, 9))),
                                    ("h1 only", "h1", same_len, ((0x1234, 10), (0x1234, 11))),
                                    ("all but the key length", "h1h2", other_len, (a, a)),
                                    ("all but the key bytes", "klen", same_len, (a, a))):
        ka, kb, kc = keys
        hashes = {ka: a, kb: others[0], kc: others[1]}
        blobs = [layout(hashes[k], k, b"held-" + k, b"", b"A") for k in (ka, kb, kc, ka)]
        held, off = rm.join(blobs)
        log = [fm.letter(nm, k, i) for i, (nm, k) in enumerate(
            (("rep-s", ka), ("rep-s", kb), ("rep-s", kc), ("rep-v", kb), ("rep-v", kc), ("rep-v", ka), ("rep-a", kb),
             ("rep-a", kc)))]
        assert fm.sort_bits(len(blobs) + len(log)) == 16
        got, m = against_model(cuda, oracle, held, off, log, what, hashes=_twins(hashes, log))
        assert m.stepped[cls] == 6 and sum(m.stepped.values()) == 6 and m.counts[3:5] == [3, 1], (what, m.stepped)
    ka = same_len[0]
    # a held blob with a wrong stored hash next to a SET_ALL of its key: two blobs come out
    hs = am.hashes_of(oracle, [ka])[ka]
    held, off = rm.join([layout((hs[0] ^ 1 << 40, hs[1]), ka, b"stale", b"", b"")])
    got, m = against_model(cuda, oracle, held, off, [fm.letter("set-v", ka, 0)], "a wrong stored hash")
    assert m.counts[:4] == [2, len(m.out), 1, 0]


def _mutants(oracle):
    """Held blobs that are no participants or are left out, each next to a record of its key
    and alone: (blobs, keep, log)."""
    keys = [b"mutant-%d" % i * 2 for i in range(12)]
    hs = am.hashes_of(oracle, keys)
    blobs = [bytearray(layout(hs[k], k, b"value-of-" + k, b"", b"AT")) for k in keys]
    keep = np.ones(12, np.uint8)
    for i in (0, 1):                                  # EMPTY
        for f in (rm.F_KLEN, rm.F_VLEN, rm.F_ALEN):
            rm.put(blobs[i], 0, f, 0)
    for i in (2, 3):                                  # NO_KEY
        rm.put(blobs[i], 0, rm.F_KLEN, 0)
    for i in (4, 5):                                  # BAD_RANGE
        rm.put(blobs[i], 0, rm.F_VPOS, len(blobs[i]) - 3)
    for i in (6, 7):
        keep[i] = 0
    for i in (8, 9):                                  # a span of fewer than 80 bytes
        blobs[i] = blobs[i][:79]
    log = [fm.letter("rep-s", keys[i], i) for i in range(0, 12, 2)]
    return blobs, keep, log


@pytest.mark.gpu
def test_held_stream(cuda, oracle):
    # a key three times: the last copy decides, the others are superseded -- touched by a record or not
    ka, kb = b"three-times", b"also-three-times-but-untouched"
    hs = am.hashes_of(oracle, [ka, kb])
    blobs = [layout(hs[k], k, b"copy-%d" % c, b"S%d" % c if c != 1 else b"", b"A%d" % c) for c in range(3) for k in (ka, kb)]
    held, off = rm.join(blobs, lead=b"\x11" * 7)
    got, m = against_model(cuda, oracle, held, off, [fm.letter("rep-v", ka, 0)], "a key three times")
    assert m.touched.tolist() == [2, 2, 2, 2, 1, 0] and m.counts == [2, len(m.out), 1, 1, 4, 0, 1]
    assert am.table_of(m.out, m.out_off)[ka] == (b"v0", b"S2", b"A2")
    # non-participants and left-out blobs, next to a matching record and alone
    blobs, keep, log = _mutants(oracle)
    held, off = rm.join(blobs)
    got, m = against_model(cuda, oracle, held, off, log, "non-participants", keep=keep)
    assert m.touched.tolist() == [0] * 6 + [3] * 4 + [1, 0] and m.counts[3] == 1 and m.counts[0] == 6 + 1 + 6
    # bad spans: an end behind the stream, a decreasing pair
    bad = [0, 100, 90, len(held) + 1, len(held)]
    got, m = against_model(cuda, oracle, held, bad, log, "bad spans")
    assert m.touched.tolist() == [0, 3, 3, 3]
    # permuted, gapped and overlapping segments with slack as field sources
    k1, k2, k3 = b"forged-one", b"forged-two-with-a-longer-key", b"f3"
    hs = am.hashes_of(oracle, [k1, k2, k3])
    f1 = ra.forge(k1, b"value-one" * 5, b"subkeys-1", b"attrs-1", order=(3, 1, 0, 2), gaps=(5, 0, 9, 1), slack=13, hashes=hs[k1])
    f2 = ra.forge(k2, b"v2", b"s" * 33, b"a" * 17, order=(2, 3, 1, 0), gaps=(0, 3, 0, 7), slack=1, hashes=hs[k2])
    f3 = ra.forge(k3, b"0123456789abcdefXYZ", hashes=hs[k3], slack=4)
    rm.put(f3, 0, rm.F_SLEN, 7), rm.put(f3, 0, rm.F_SPOS, 80 + len(k3) + 3)     # the subkeys lie inside the value
    rm.put(f3, 0, rm.F_ALEN, 5), rm.put(f3, 0, rm.F_APOS, 80 + len(k3) - 1)     # the attrs across key and value
    held, off = rm.join([f1, f2, f3], lead=b"\x22")
    for nm in ("rep-v", "rep-s", "rep-a", "rep-a0"):
        log = [fm.letter(nm, k, i) for i, k in enumerate((k1, k2, k3))]
        got, m = against_model(cuda, oracle, held, off, log, f"forged sources, {nm}", oshift=9)
        assert m.counts[:4] == [3, len(m.out), 0, 3]
    assert am.table_of(m.out, m.out_off)[k3] == (b"0123456789abcdefXYZ", b"3456789", None)


@pytest.mark.gpu
def test_segment_shapes(cuda, oracle):
    sizes = (0, 1, 15, 16, 17, 4096, 65536)
    rng = ra._rng(33)
    keys = [b"shape-%02d" % i + b"k" * i for i in range(4 * len(sizes))]
    hs = am.hashes_of(oracle, keys)
    held_blobs, log = [], []
    for i, sz in enumerate(sizes):
        data = [ra.rbytes(rng, sz) for _ in range(4)]
        ka, kb, kc, kd = keys[4 * i:4 * i + 4]
        held_blobs += [layout(hs[ka], ka, data[0], b"hs", b""), layout(hs[kb], kb, b"hv", data[1], data[0])]
        log += [fm.letter("rep-a", ka, i), fm.letter("rep-v", kb, i),                    # fields from a held blob
                Rec(fm.SET_ALL, kc, data[2], b"", data[3]), Rec(fm.REPLACE_SKEY, kd, b"", data[3]),  # from a record
                Rec(fm.REPLACE_VAL, kd, data[2])]
    held, off = rm.join(held_blobs, lead=b"\x33" * 9)
    for oshift in range(16):           # all 16 output alignments
        got, m = against_model(cuda, oracle, held, off, log, f"segment sizes, out at {oshift}", oshift=oshift,
                               hshift=(oshift * 7 + 3) % 16, fshift=(oshift * 3 + 1) % 16)
    assert m.counts[2] == 0 and m.counts[0] == 4 * len(sizes) and m.counts[1] > 4 * 65536
    # key-only results, from a record alone and from a held blob emptied field by field
    ka, kb = keys[0], keys[1]
    held, off = rm.join([layout(hs[kb], kb, b"v", b"", b"a")])
    log = [fm.letter("rep-v0", ka, 0), fm.letter("del", kb, 1), fm.letter("rep-a0", kb, 2), fm.letter("rep-v0", kb, 3),
           fm.letter("rep-a0", kb, 4)]
    got, m = against_model(cuda, oracle, held, off, log, "key-only")
    assert m.out == layout(hs[ka], ka, b"", b"", b"") + layout(hs[kb], kb, b"", b"", b"")


@pytest.mark.gpu
def test_parts_empty_and_large(cuda, oracle):
    """Part 2 empty, part 1 empty, and more than one tile of 256 in each."""
    ks, vs, ss, as_ = ra.records(ra._rng(9), 700, p_extra=0.4)
    ks = [b"%04d" % i + k for i, k in enumerate(ks)]
    hs = am.hashes_of(oracle, ks)
    blobs = [layout(hs[k], k, v, s, a) for k, v, s, a in zip(ks, vs, ss, as_)]
    held, off = rm.join(blobs, lead=b"\x44" * 5)
    # part 2 empty: records of keys the stream does not hold, all deleted in the end; and no record
    log = [fm.letter(nm, b"stranger-%d" % i, i) for i in range(300) for nm in ("set-vsa", "del")]
    got, m = against_model(cuda, oracle, held, off, log, "part 2 empty")
    assert m.counts == [700, len(held) - 5, 700, 0, 0, 300, 600]
    # part 1 empty: every held key rewritten or deleted
    log = [fm.letter(("rep-v", "del", "set-vs", "rep-a0")[i % 4], k, i) for i, k in enumerate(ks)]
    got, m = against_model(cuda, oracle, held, off, log, "part 1 empty")
    assert m.counts[:6] == [525, len(m.out), 0, 700, 0, 175]
    # both parts, several tiles each, in an order that is neither's
    order = np.random.default_rng(3).permutation(700)[:400]
    log = [fm.letter(("rep-s", "rep-v", "set-va")[i % 3], ks[int(j)], i) for i, j in enumerate(order)]
    got, m = against_model(cuda, oracle, held, off, log, "both parts")
    assert m.counts[:4] == [700, len(m.out), 300, 400]


@pytest.mark.gpu
def test_stop(cuda, oracle):
    keys = [b"stop-key-%d" % i for i in range(6)]
    held, off = _held_of(oracle, {k: (b"held", b"hs", None) for k in keys[:3]})
    plain = [fm.letter(("rep-v", "set-vs", "del", "rep-a")[i % 4], keys[i % 6], i) for i in range(24)]
    for barrier in (fm.letter("ow", keys[1], 99), Rec(fm.RENAME, keys[2], b"", b"", b"", b"new-name")):
        for at in (0, 11, 23):
            log = plain[:at] + [barrier] + plain[at + 1:]
            got, m = against_model(cuda, oracle, held, off, log, f"type {barrier.type} at {at}")
            assert m.stop == at == got[6]
            # records behind the stop leave no trace: the same answer without them
            cut = am.apply_model(held, off, None, log[:at], None, *am.rec_hashes(oracle, log[:at]))
            assert (cut.out, cut.touched.tolist(), cut.counts) == (m.out, m.touched.tolist(), m.counts)
            # with a bad status, or not considered: no stop
            bad = log[:at] + [barrier._replace(status=2)] + log[at + 1:]
            got, m = against_model(cuda, oracle, held, off, bad, "a barrier with a bad status")
            assert m.stop == 24
            cons = np.ones(24, np.uint8)
            cons[at] = 0
            got, m = against_model(cuda, oracle, held, off, log, "a barrier not considered", consider=cons)
            assert m.stop == 24


@pytest.mark.gpu
def test_chains(cuda, oracle):
    """A REPLACE_SKEY before 65,536 REPLACE_VALs of one key, with and without the fold's keep; and
    the two-record logs of the header."""
    hot, other = b"the-hot-key", b"a-bystander"
    held, off = _held_of(oracle, {hot: (b"old", b"old-s", b"old-a"), other: (b"b", None, None)})
    log = [Rec(fm.REPLACE_SKEY, hot, b"", b"new-subkeys")] + [Rec(fm.REPLACE_VAL, hot, b"v%d" % i) for i in range(65536)]
    got, m = against_model(cuda, oracle, held, off, log, "the long chain")
    assert am.table_of(m.out, m.out_off)[hot] == (b"v65535", b"new-subkeys", b"old-a") and m.counts[6] == 65537
    keep = fm.fold_model(log)[0]
    assert keep.sum() == 2
    got2, m2 = against_model(cuda, oracle, held, off, log, "the long chain, folded", consider=keep)
    assert got2[1] == got[1] and m2.counts[6] == 2
    for names in (("set-vsa", "del"), ("del", "rep-a")):
        log = [fm.letter(nm, hot, at) for at, nm in enumerate(names)]
        against_model(cuda, oracle, held, off, log, str(names))


@pytest.mark.gpu
def test_call_shapes(cuda, oracle):
    ks, vs, ss, as_ = ra.records(ra._rng(21), 300, klen=(4, 41), p_extra=0.5)
    hs = am.hashes_of(oracle, ks)
    held, off = rm.join([layout(hs[k], k, v, s, a) for k, v, s, a in zip(ks[:200], vs, ss, as_)])
    log = [fm.letter(fm.TWELVE[(5 * i) % 12] if fm.TWELVE[(5 * i) % 12] != "ow" else "del", ks[(7 * i) % 300], i)
           for i in range(500)]
    got, m = against_model(cuda, oracle, held, off, log, "count only", count_only=True)
    assert got[1] is None and got[5] == m.counts
    # out_cap one byte short: EINVAL that names both figures, counts set, nothing written
    file, recs = am.build_log(log)
    h1, h2 = am.rec_hashes(oracle, log)
    rc, out, _o, _g, touched, counts, stop = am.run_apply(cuda, held, off, recs, file, h1=h1, h2=h2, cap=m.counts[1] - 1)
    assert rc == _native.K2H_AMD_EINVAL and counts == m.counts and (touched == m.touched).all() and stop == m.stop
    text = bytes(_native.batch_lib().k2h_amd_strerror(rc))
    assert b"%d" % m.counts[1] in text and b"%d" % (m.counts[1] - 1) in text
    against_model(cuda, oracle, held, off, log, "origin and touched NULL", want_origin=False, want_touched=False)
    # the hashes computed inside the call, under both seeds: the headers carry the table's hashes
    for variant in (0, 1):
        hv = am.hashes_of(oracle, ks, variant)
        held_v, off_v = rm.join([layout(hv[k], k, v, s, a) for k, v, s, a in zip(ks[:200], vs, ss, as_)])
        got, mv = against_model(cuda, oracle, held_v, off_v, log, f"hashed inside, variant {variant}", hashes=None,
                                variant=variant)
        assert mv.counts == m.counts
    assert mv.out != m.out


@pytest.mark.gpu
def test_end_to_end(cuda, oracle):
    """apply_log over a composed held stream and log: its output fed to the dict table is what
    Load leaves; its part 2 through ralledata_to_archive, replayed from the empty table, gives
    the touched keys of that table."""
    import torch

    from k2hash_amd import apply, ralledata
    recs, keys, prior, _rng = _random_log(4242, n=400, nkeys=40, barriers=False)
    recs = [r for r in recs if r.status == 0 and r.type <= 6]   # (the device scan judges status and type itself)
    barrier_at = 333
    recs[barrier_at] = fm.letter("ow", keys[0], 1)
    held, off = _held_of(oracle, prior)
    file, _r = am.build_log(recs)
    d_held = torch.from_numpy(np.frombuffer(held, np.uint8).copy()).to(cuda)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    d_file = torch.from_numpy(np.frombuffer(file, np.uint8).copy()).to(cuda)
    want = fm.replay(recs[:barrier_at], prior)
    for fold in (True, False):
        a = apply.apply_log(d_held, d_off, d_file, fold=fold)
        assert a.stop == barrier_at and a.first_changed == a.counts.unchanged
        out, ooff = a.blobs.cpu().numpy().tobytes(), a.blob_off.cpu().numpy()
        assert am.table_of(out, ooff) == want, fold
        m = am.apply_model(held, off, None, recs[:barrier_at], None, *am.rec_hashes(oracle, recs[:barrier_at]))
        assert out == m.out and (a.origin.cpu().numpy() == m.origin.view(np.int64)).all()
        assert (a.touched.cpu().numpy() == m.touched).all() and tuple(a.counts)[:6] == tuple(m.counts[:6])
    # part 2 as an archive, replayed from the empty table
    lo = int(ooff[a.first_changed])
    p2 = ralledata.ralledata_to_archive(a.blobs[lo:], a.blob_off[a.first_changed:] - lo)
    arc = p2.bytes.cpu().numpy().tobytes()
    back = fm.replay(fm.recs_of(arc, archive.scan(arc)), {})
    touched_keys = {r.key for r in recs[:barrier_at] if fm.participant(r)}
    assert back == {k: v for k, v in want.items() if k in touched_keys}
    # log -> snapshot with an empty held stream
    a0 = apply.apply_log(None, None, d_file)
    assert am.table_of(a0.blobs.cpu().numpy().tobytes(), a0.blob_off.cpu().numpy()) == fm.replay(recs[:barrier_at], {})
    assert a0.first_changed == 0 and a0.touched.numel() == 0
