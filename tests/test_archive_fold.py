"""A transaction archive folded by K2HArchive::Load's rule (include/k2hash_amd.h section 5b:
k2h_amd_archive_fold; k2h_archive_fold.hip) against the model of archive_fold_model.py, entry
for entry: keep, by and dropped.

The model is a sequential reverse pass with a dict per key.  That its rule is sound -- the table
after the kept records equals the table after all of them, from every prior state -- is shown on
the CPU against a transliteration of Load (archive_fold_model.replay) in which OW_VAL and RENAME
read everything they could depend on; libk2hash itself is not built here, so parity with it is a
restatement.  Records are packed by scom_record, pinned to the reference-written
tests/golden/archive.k2har.  Expected values never come from the device code, every device
output is sentinel-filled first, and the file sits in a guarded allocation.
"""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

from conftest import GOLDEN

import archive_fold_model as fm
import big_offsets as bo
from archive_fold_model import NONE, Rec

from k2hash_amd import _native, archive, hashfunc

KEY = b"the-key"


def golden_recs():
    f = (GOLDEN / "archive.k2har").read_bytes()
    recs = archive.scan(f)   # the host scan, pinned to archive.json by test_archive.py
    return f, recs, fm.recs_of(f, recs)


# ------------------------------------------------------------------------------------- CPU
def test_packer_reproduces_the_reference_records():
    """scom_record gives all 64 records of the golden file byte for byte, from their own segments."""
    f, recs, model = golden_recs()
    assert recs.size == 64 and {int(t) for t in recs["type"]} == set(range(7)) and not recs["status"].any()
    ends = [int(o) for o in recs["offset"][1:]] + [len(f)]
    for r, m, e in zip(recs, model, ends):
        assert fm.record_bytes(m) == f[int(r["offset"]):e], int(r["offset"])
    assert b"".join(fm.record_bytes(m) for m in model) == f


def test_golden_file_folds_to_itself():
    _f, _recs, model = golden_recs()
    assert len({m.key for m in model}) == 64
    keep, by, dropped = fm.fold_model(model)
    assert keep.all() and (by == NONE).all() and dropped == 0


def _sound(recs, prior_tables, what):
    keep, _by, dropped = fm.fold_model(recs)
    kept = [r for r, k in zip(recs, keep) if k]
    assert len(kept) == sum(fm.participant(r) for r in recs) - dropped, what
    if dropped:   # (nothing dropped: the two replays run over the same records)
        for name, prior in prior_tables.items():
            assert fm.replay(kept, prior) == fm.replay(recs, prior), (what, name)
    return dropped


def test_soundness_exhaustive():
    """Every sequence of length 1..5 over the twelve letters (the nine, and each REPLACE_* with
    empty data) on one key, from four prior states of that key."""
    pri = fm.priors(KEY)
    letters = {(name, at): fm.letter(name, KEY, at) for name in fm.TWELVE for at in range(5)}
    seqs = folded = 0
    for length in range(1, 6):
        for names in itertools.product(fm.TWELVE, repeat=length):
            seqs += 1
            folded += _sound([letters[(nm, at)] for at, nm in enumerate(names)], pri, names) > 0
    assert seqs == sum(12 ** k for k in range(1, 6)) and folded > seqs // 2


def _random_log(seed, n=40, nkeys=4):
    rng = np.random.default_rng(seed)
    keys = [b"key-%d" % k for k in range(nkeys)]
    out = []
    for i in range(n):
        u = rng.random()
        key = keys[int(rng.integers(0, nkeys))]
        if u < 0.04:
            out.append(Rec(fm.RENAME, key, b"", b"", b"ra%d" % i if rng.random() < 0.5 else b"",
                           keys[int(rng.integers(0, nkeys))]))
        elif u < 0.07:
            out.append(Rec(fm.SET_ALL, key, b"bad%d" % i, status=int(rng.integers(1, 4))))
        elif u < 0.09:
            out.append(Rec(7, key, b"bad%d" % i))
        elif u < 0.11:
            out.append(Rec(fm.SET_ALL, b"", b"nokey%d" % i))
        else:
            out.append(fm.letter(fm.TWELVE[int(rng.integers(0, 12))], key, i))
    return out, keys


def test_soundness_random():
    """1,000 logs of 40 records over 4 keys with RENAMEs and non-participants mixed in."""
    total = renames = 0
    for seed in range(1000):
        recs, keys = _random_log(seed)
        pri = {name: {k: fm.priors(k)[name][k] for k in keys} if name != "absent" else {}
               for name in ("absent", "v", "s", "vsa")}
        total += _sound(recs, pri, seed)
        renames += sum(r.type == fm.RENAME for r in recs)
    assert total > 5000 and renames > 500


def test_replay_tells_an_unsound_fold_apart():
    """The control: dropping the record before every barrier, or folding across a RENAME, leaves
    another table, so the replay can tell."""
    pri = fm.priors(KEY)
    a = [fm.letter("set-vsa", KEY, 0), fm.letter("ow", KEY, 1), fm.letter("rep-s", KEY, 2)]
    assert fm.replay(a[1:], pri["absent"]) != fm.replay(a, pri["absent"])
    other = b"other"
    b = [fm.letter("set-v", KEY, 0), Rec(fm.RENAME, other, b"", b"", b"", b"new"), fm.letter("set-v", KEY, 2)]
    assert fm.replay(b[1:], {}) != fm.replay(b, {})
    assert fm.fold_model(a)[0].all() and fm.fold_model(b)[0].all()


def test_fold_is_idempotent():
    for seed in range(200):
        recs, _keys = _random_log(seed)
        keep = fm.fold_model(recs)[0]
        kept = [r for r, k in zip(recs, keep) if k]
        again = fm.fold_model(kept)
        assert again[0].all() and again[2] == 0, seed


def test_motivating_cases():
    s_then_empty = [Rec(fm.SET_ALL, KEY, b"v1", b"S"), Rec(fm.SET_ALL, KEY, b"v2", b"")]
    keep, by, dropped = fm.fold_model(s_then_empty)
    assert keep.tolist() == [1, 1] and by.tolist() == [1, NONE] and dropped == 0
    assert fm.replay(s_then_empty, {}) == {KEY: (b"v2", b"S", None)}          # Load's rule, not the whole-blob one
    keep, by, dropped = fm.fold_model([Rec(fm.SET_ALL, KEY, b"v", b"s", b"a"), Rec(fm.DEL_KEY, KEY)])
    assert keep.tolist() == [0, 1] and dropped == 1
    keep, by, dropped = fm.fold_model([Rec(fm.DEL_KEY, KEY), Rec(fm.SET_ALL, KEY, b"v", b"s", b"a")])
    assert keep.tolist() == [0, 1] and dropped == 1
    # a delete before a set that leaves a field alone stays: the set would inherit the old subkeys
    keep, by, dropped = fm.fold_model([Rec(fm.DEL_KEY, KEY), Rec(fm.SET_ALL, KEY, b"v")])
    assert keep.tolist() == [1, 1] and dropped == 0


def test_fold_argument_validation():
    """Judged on the host before any device is touched: the same answers with and without a
    GPU, each with its own message."""
    lib = _native.batch_lib()
    f, recs, _model = golden_recs()
    buf = np.frombuffer(f, np.uint8).copy()
    n = recs.size
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    keep, by = np.full(n, 0xEE, np.uint8), np.zeros(n, np.uint64)
    dropped = ctypes.c_uint64(7)
    fold = lib.k2h_amd_archive_fold
    msg = lambda: lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL)  # noqa: E731
    assert fold(None, 0, None, 0, None, None, None, ctypes.byref(dropped), None) == _native.K2H_AMD_OK
    assert dropped.value == 0
    assert fold(None, 0, None, 0, None, None, None, None, None) == _native.K2H_AMD_OK
    texts = set()
    for args, text in (((p(buf), buf.size, p(recs), n, None, None, p(by), ctypes.byref(dropped), None), b"NULL keep"),
                       ((None, buf.size, p(recs), n, None, p(keep), None, None, None), b"NULL file"),
                       ((p(buf), buf.size, None, n, None, p(keep), None, None, None), b"NULL recs"),
                       ((p(buf), buf.size, p(recs), (1 << 32) - 1, None, p(keep), None, None, None), b"2^32 - 2"),
                       ((p(buf), buf.size, p(recs), 1 << 40, None, p(keep), None, None, None), b"32-bit")):
        assert fold(*args) == _native.K2H_AMD_EINVAL
        assert text in msg() and msg().startswith(b"archive_fold: ")
        texts.add(bytes(msg()))
    assert len(texts) == 4 and (keep == 0xEE).all()


def test_fold_public_names():
    import k2hash_amd
    for name in ("fold_device", "compact_device"):
        assert hasattr(k2hash_amd, name) and name in k2hash_amd.__all__
    assert len(_native.SIGNATURES["k2h_amd_archive_fold"][1]) == 9
    sig = inspect.signature(archive.fold_device).parameters
    assert [sig[k].default for k in ("recs", "h1", "want_by", "count", "stream")] == [None, None, False, True, None]
    assert inspect.signature(archive.compact_device).parameters["stream"].default is None
    assert archive.Folded._fields == ("keep", "by", "dropped", "recs")
    assert archive.Compacted._fields == ("bytes", "index", "kept", "kept_bytes", "records")
    assert archive.NO_LATER == NONE


# ---- the logs of the GPU tests, and (CPU) that each is what its test claims
KEY_LENS = (1, 15, 16, 17, 31, 32, 33, 100)


def _own_key(s, short):
    """A key for sequence s, unlike every other sequence's: the lengths cycle through KEY_LENS;
    there are only 256 keys of one byte, so once those are used up that turn takes two bytes.
    The bytes that tell two keys apart are the first ones for even s and the last ones for odd
    s, the rest is the same for all keys of a length."""
    L = KEY_LENS[s % len(KEY_LENS)]
    if L == 1:
        c = short[0]
        short[0] += 1
        return bytes([c]) if c < 256 else (c - 256).to_bytes(2, "little")
    fill = bytes((7 * i + 3) & 0xFF for i in range(L - 4))
    tag = s.to_bytes(4, "little")
    return fill + tag if s & 1 else tag + fill


def _exhaustive_sequences():
    """Every sequence of length 1..4 over the nine letters, each on a key of its own."""
    seqs, short = [], [0]
    for length in range(1, 5):
        for names in itertools.product(fm.NINE, repeat=length):
            key = _own_key(len(seqs), short)
            seqs.append([fm.letter(nm, key, at) for at, nm in enumerate(names)])
    return seqs


@pytest.fixture(scope="module")
def exhaustive():
    seqs = _exhaustive_sequences()
    flat = [r for s in seqs for r in s]
    inter = [s[j] for j in range(4) for s in seqs if j < len(s)]
    return seqs, flat, inter


def test_exhaustive_logs_are_what_they_claim(exhaustive):
    seqs, flat, inter = exhaustive
    assert len(seqs) == 9 + 81 + 729 + 6561 and len(flat) == len(inter) == 28602
    assert len({s[0].key for s in seqs}) == len(seqs)
    assert {len(s[0].key) for s in seqs} == set(KEY_LENS) | {2}
    # one sequence's records are neighbours in the one log and thousands of records apart in the other
    at = [i for i, r in enumerate(inter) if r.key == seqs[-1][0].key]
    assert len(at) == 4 and min(b - a for a, b in zip(at, at[1:])) > 4096
    for log in (flat, inter):
        keep, by, dropped = fm.fold_model(log)
        assert 5000 < dropped < len(log) - len(seqs)
    # the per-sequence answer does not depend on the interleaving
    want = np.concatenate([fm.fold_model(s)[0] for s in seqs])
    assert (fm.fold_model(flat)[0] == want).all()


COLLIDE_KEYS = [b"same-length-key-A", b"Bame-length-key-A", b"same-length-key-B", b"prefix", b"prefix-and-more",
                b"k", b"a-key-of-exactly-32-bytes-long-xx", b"b-key-of-exactly-32-bytes-long-xx"]


def _collision_log(extra=()):
    """300 records of 8 keys: pairs of equal length that differ only in the first or only in the
    last byte, and a key that is a prefix of another; plus `extra` keys, each written twice."""
    rng = np.random.default_rng(17)
    keys = list(COLLIDE_KEYS)
    log = [fm.letter(fm.TWELVE[int(rng.integers(0, 12))], keys[int(rng.integers(0, 8))], i) for i in range(300)]
    for j, k in enumerate(extra):
        log.insert(50 + 60 * j, fm.letter("set-v", k, 1000 + j))
        log.append(fm.letter("set-v", k, 2000 + j))
    return log


TWIN_BITS = fm.sort_bits(304)   # the bits a log of 304 records is sorted by


def _low_bit_twins(bits=TWIN_BITS):
    """Two keys whose default hashes agree in the low `bits` bits and differ above them."""
    seen = {}
    for i in range(1 << 20):
        k = b"twin-%d" % i
        h = hashfunc.k2h_hash(k)
        low = h & ((1 << bits) - 1)
        if low in seen and seen[low][1] != h:
            return seen[low][0], k
        seen[low] = (k, h)
    raise AssertionError("no twins found")


def test_collision_logs_are_what_they_claim():
    log = _collision_log()
    assert len(log) == 300 and len({r.key for r in log}) == 8
    assert COLLIDE_KEYS[0][1:] == COLLIDE_KEYS[1][1:] and COLLIDE_KEYS[0][:-1] == COLLIDE_KEYS[2][:-1]
    assert COLLIDE_KEYS[4].startswith(COLLIDE_KEYS[3])
    a, b = _low_bit_twins()
    ha, hb = hashfunc.k2h_hash(a), hashfunc.k2h_hash(b)
    assert TWIN_BITS == 24 and ha != hb and (ha ^ hb) & ((1 << TWIN_BITS) - 1) == 0
    keep, by, dropped = fm.fold_model(_collision_log((a, b)))
    assert len(_collision_log((a, b))) == 304
    assert 100 < dropped < 300 and keep.sum() + dropped == 304


HOT = b"the-hot-key"


def _hot_log(barrier):
    """One SET_ALL(v, s, a), then 65,536 REPLACE_VALs of one key, scattered among 10,000 records
    of other keys; barrier: one OW_VAL of the hot key in the middle."""
    rng = np.random.default_rng(23)
    n_hot, n_other = 65536, 10000
    slots = np.zeros(n_hot + n_other, bool)
    slots[rng.choice(n_hot + n_other, n_other, replace=False)] = True
    log, h = [fm.letter("set-vsa", HOT, 0)], 0
    for i, other in enumerate(slots):
        if other:
            log.append(fm.letter(fm.NINE[i % 8], b"other-%04d" % int(rng.integers(0, 3000)), i))
        else:
            h += 1
            if barrier and h == n_hot // 2:
                log.append(fm.letter("ow", HOT, i))
            log.append(Rec(fm.REPLACE_VAL, HOT, b"h%d" % h))
    return log


@pytest.fixture(scope="module")
def hot_logs():
    return {b: _hot_log(b) for b in (False, True)}


def test_hot_logs_are_what_they_claim(hot_logs):
    for barrier, log in hot_logs.items():
        keep = fm.fold_model(log)[0]
        hot = [i for i, r in enumerate(log) if r.key == HOT]
        kept = [i for i in hot if keep[i]]
        assert len(hot) == 65537 + barrier
        if not barrier:
            assert kept == [0, hot[-1]]
        else:
            ow = next(i for i in hot if log[i].type == fm.OW_VAL)
            before = max(i for i in hot if i < ow)
            assert kept == [0, before, ow, hot[-1]] and log[before].type == fm.REPLACE_VAL


def _rename_log():
    """2,000 records over 50 keys with three RENAMEs."""
    rng = np.random.default_rng(29)
    keys = [b"rename-key-%02d" % k for k in range(50)]
    log = [fm.letter(fm.TWELVE[int(rng.integers(0, 12))], keys[int(rng.integers(0, 50))], i) for i in range(2000)]
    for at in (400, 1000, 1600):
        log[at] = Rec(fm.RENAME, keys[at % 50], b"", b"", b"ren-attrs", b"renamed-%d" % at)
    return log


def test_rename_log_is_what_it_claims():
    log = _rename_log()
    keep, by, dropped = fm.fold_model(log)
    ren = [i for i, r in enumerate(log) if r.type == fm.RENAME]
    assert ren == [400, 1000, 1600] and all(keep[i] for i in ren) and 700 < dropped < 1900
    # every segment keeps, per key, at least the last record of that key in the segment
    for lo, hi in zip([0] + [r + 1 for r in ren], ren + [len(log)]):
        last = {}
        for i in range(lo, hi):
            last[log[i].key] = i
        assert all(keep[i] for i in last.values())
    # the RENAME's own key: the record of that key before it is kept, although a later one covers it
    for r in ren:
        prev = max(i for i in range(r) if log[i].key == log[r].key)
        assert keep[prev] and by[prev] == r and by[r] != NONE


def _host_file(log):
    data = b"".join(fm.record_bytes(r) for r in log)
    recs = archive.scan(data)
    assert recs.size == len(log) and not recs["status"].any()
    return data, recs


def _hostile():
    """A log of 120 good records with non-participants and hostile records planted among them:
    (data, recs, model records, {index: what})."""
    rng = np.random.default_rng(31)
    keys = [b"hostile-key-%d" % k for k in range(6)]
    log = [fm.letter(fm.NINE[int(rng.integers(0, 8))], keys[int(rng.integers(0, 6))], i) for i in range(120)]
    data, recs = _host_file(log)
    recs = recs.copy()
    planted = {}

    def plant(i, what, **fields):
        for k, v in fields.items():
            recs[i][k] = v
        planted[i] = what
    plant(10, "BAD_TYPE", status=archive.STATUS_BAD_TYPE)
    plant(20, "TRUNCATED", status=archive.STATUS_TRUNCATED)
    plant(30, "NO_MAGIC", status=archive.STATUS_NO_MAGIC)
    plant(40, "NO_KEY", key_len=0)
    plant(50, "TYPE_7", type=7)
    plant(60, "TYPE_NEGATIVE", type=-1)
    plant(70, "KEY_BEYOND_SIZE", key_off=len(data) + 1)
    plant(80, "KEY_WRAPS", key_off=(1 << 64) - 8, key_len=16)
    plant(90, "KEY_RUNS_OUT", key_len=len(data))
    plant(119, "LAST_NOT_OK", status=archive.STATUS_TRUNCATED)
    return data, recs, fm.recs_of(data, recs), planted


def test_hostile_log_is_what_it_claims():
    data, recs, model, planted = _hostile()
    assert all(not fm.participant(model[i]) for i in planted)
    assert sum(fm.participant(m) for m in model) == 120 - len(planted)
    keep, by, dropped = fm.fold_model(model)
    assert all(keep[i] == 0 and by[i] == NONE for i in planted) and dropped > 50
    assert not any(int(b) in planted for b in by if b != NONE)


def _near_start():
    """Hand-made records whose keys lie at file offsets 0..15 with lengths 1..32 (the shapes of
    big_offsets.near_start_ranges) over a file of period 7, so that many ranges hold equal keys:
    (data, recs, model records)."""
    starts, lens = bo.near_start_ranges()
    data = bytes((i % 7) + 65 for i in range(64))
    recs = np.zeros(starts.size, archive.REC_DTYPE)
    recs["key_off"], recs["key_len"] = starts, lens
    recs["type"] = np.arange(starts.size) % 4          # SET_ALL, REPLACE_VAL, REPLACE_SKEY, DEL_KEY
    for name in ("val_off", "skey_off", "attrs_off", "exdata_off"):
        recs[name] = 64
    return data, recs, fm.recs_of(data, recs)


def test_near_start_log_is_what_it_claims():
    data, recs, model = _near_start()
    assert len(model) == 512 and all(fm.participant(m) for m in model)
    keep, by, dropped = fm.fold_model(model)
    assert 50 < dropped < 450 and 50 < len({m.key for m in model}) < 400


# ------------------------------------------------------------------------------------- GPU
def against_model(cuda, log, what, h1=None, shift=0):
    data, recs = _host_file(log)
    want = fm.fold_model(log)
    fm.assert_same(fm.run_fold(cuda, data, recs, h1=h1, shift=shift), want, what)
    return want


@pytest.mark.gpu
def test_smallest_shapes(cuda):
    got = fm.run_fold(cuda, b"", np.zeros(0, archive.REC_DTYPE))
    assert got[0].size == 0 and got[1].size == 0 and got[2] == 0
    keep, by, dropped = against_model(cuda, [fm.letter("set-vsa", KEY, 0)], "n = 1", shift=3)
    assert keep.tolist() == [1] and dropped == 0
    keep, by, dropped = against_model(cuda, [fm.letter("ow", KEY, 0)], "n = 1, a barrier")
    assert keep.tolist() == [1]
    keep, by, dropped = against_model(cuda, [Rec(fm.SET_ALL, KEY, b"v1", b"S"), Rec(fm.SET_ALL, KEY, b"v2")], "S, empty")
    assert keep.tolist() == [1, 1] and by.tolist() == [1, NONE]
    keep, by, dropped = against_model(cuda, [fm.letter("set-vsa", KEY, 0), Rec(fm.DEL_KEY, KEY)], "set, delete")
    assert keep.tolist() == [0, 1] and dropped == 1
    keep, by, dropped = against_model(cuda, [Rec(fm.DEL_KEY, KEY), fm.letter("set-vsa", KEY, 1)], "delete, set")
    assert keep.tolist() == [0, 1] and dropped == 1


@pytest.mark.gpu
def test_golden_file(cuda):
    f, recs, model = golden_recs()
    want = fm.fold_model(model)
    for shift in (0, 5):
        fm.assert_same(fm.run_fold(cuda, f, recs, shift=shift), want, f"golden, shift {shift}")
    assert want[0].all() and want[2] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["one-key-per-sequence", "interleaved"])
def test_exhaustive(cuda, exhaustive, order):
    _seqs, flat, inter = exhaustive
    against_model(cuda, flat if order == "one-key-per-sequence" else inter, order, shift=1)


@pytest.mark.gpu
def test_forced_collisions(cuda):
    """Every h1 is 0: one run of 300 entries, and only the key compare tells the 8 keys apart."""
    log = _collision_log()
    against_model(cuda, log, "h1 all zeros", h1=np.zeros(len(log), np.uint64), shift=7)


@pytest.mark.gpu
def test_natural_low_bit_collision(cuda):
    """h1 computed by the call; two keys agree in the 24 sorted bits of their hashes only."""
    against_model(cuda, _collision_log(_low_bit_twins()), "low-bit twins")


@pytest.mark.gpu
@pytest.mark.parametrize("barrier", [False, True], ids=["plain", "ow-in-the-middle"])
def test_hot_key(cuda, hot_logs, barrier):
    log = hot_logs[barrier]
    keep, by, dropped = against_model(cuda, log, "hot key")
    kept_hot = [i for i, r in enumerate(log) if r.key == HOT and keep[i]]
    assert len(kept_hot) == (4 if barrier else 2)


@pytest.mark.gpu
def test_rename(cuda):
    against_model(cuda, _rename_log(), "three renames")


@pytest.mark.gpu
def test_non_participants_and_hostile_records(cuda):
    data, recs, model, planted = _hostile()
    want = fm.fold_model(model)
    for shift in (0, 11):
        got = fm.run_fold(cuda, data, recs, shift=shift)
        fm.assert_same(got, want, f"hostile, shift {shift}")
        assert all(got[0][i] == 0 for i in planted)
    # the same records with the caller's (wrong) hashes
    fm.assert_same(fm.run_fold(cuda, data, recs, h1=np.full(len(recs), 5, np.uint64)), want, "hostile, h1 = 5")


@pytest.mark.gpu
def test_keys_near_the_start_of_the_file(cuda):
    data, recs, model = _near_start()
    want = fm.fold_model(model)
    for h1 in (None, np.zeros(len(recs), np.uint64)):
        fm.assert_same(fm.run_fold(cuda, data, recs, h1=h1), want, "keys at offsets 0..15")


@pytest.mark.gpu
def test_compact_device_end_to_end(cuda, exhaustive):
    import torch
    _seqs, _flat, inter = exhaustive
    data, recs = _host_file(inter)
    keep, _by, dropped = fm.fold_model(inter)
    fw, file = bo.guarded(torch, cuda, len(data), shift=2, fill=0xA5)
    file[:] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(cuda)
    c = archive.compact_device(file)
    torch.cuda.synchronize()
    out = c.bytes.cpu().numpy().tobytes()
    kept = [r for r, k in zip(inter, keep) if k]
    assert c.records == len(inter) and c.kept == len(kept) == len(inter) - dropped and c.kept_bytes == len(out)
    assert (c.index.cpu().numpy() == np.flatnonzero(keep)).all()
    assert out == b"".join(fm.record_bytes(r) for r in kept)
    orecs = archive.scan(out)                         # the host scan walks the output as an archive
    assert orecs.size == len(kept) and not orecs["status"].any() and fm.recs_of(out, orecs) == kept
    f2 = archive.fold_device(c.bytes.clone(), want_by=False)
    assert f2.dropped == 0 and bool(f2.keep.all()) and f2.by is None
    # the same fold through the wrapper, with its own scan and hashes
    f1 = archive.fold_device(file, want_by=True)
    fm.assert_same((f1.keep.cpu().numpy(), f1.by.cpu().numpy().view(np.uint64), f1.dropped), (keep, _by, dropped),
                   "fold_device")
    f3 = archive.fold_device(file, count=False)
    torch.cuda.synchronize()
    assert f3.dropped is None and torch.equal(f3.keep, f1.keep)
    assert bo.guards_intact(torch, fw, file, 0xA5)
    keys = {r.key for r in inter}
    for name in ("absent", "v", "s", "vsa"):
        prior = {} if name == "absent" else {k: fm.priors(k)[name][k] for k in keys}
        assert fm.replay(fm.recs_of(out, orecs), prior) == fm.replay(inter, prior), name
