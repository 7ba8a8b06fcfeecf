"""The model of k2h_amd_archive_barrier (archive_barrier_model.py; include/k2hash_amd.h section 5d)
held against itself and against archive_fold_model.replay on the CPU, and the call's host-side
argument checks, which touch no device.  libk2hash itself is not built here: execute is a reviewed
transliteration of Load's two barrier arms, as replay is of the other five.
"""
import ctypes
import itertools
import struct

import numpy as np

import archive_apply_model as am
import archive_barrier_model as bm
import archive_fold_model as fm
import ralle_check_model as rm
from archive_barrier_model import BAD_RECORD, CREATED, EXECUTED, GAP, NEW_EXISTS, NOT_A_BARRIER, NOT_FOUND
from archive_fold_model import OW_VAL, RENAME, Rec
from ralle_unlink_model import layout

from k2hash_amd import _native, archive

KEY = b"the-key"
ELEVEN = tuple(x for x in fm.TWELVE if x != "ow")


def ow(key, off, data, exlen=8):
    return Rec(OW_VAL, key, data, b"", b"", struct.pack("<q", off)[:exlen])


def ren(key, new, attrs=b""):
    return Rec(RENAME, key, b"", b"", attrs, new)


def test_replay_all_is_replay_without_barriers():
    """Every sequence of length 1..4 over the eleven barrier-free letters and a fixed sample of
    3,000 of length 5, from the four prior states of the key."""
    pri = fm.priors(KEY)
    letters = {(nm, at): fm.letter(nm, KEY, at) for nm in ELEVEN for at in range(5)}
    rng = np.random.default_rng(5150)
    seqs = [s for k in range(1, 5) for s in itertools.product(ELEVEN, repeat=k)]
    seqs += [tuple(ELEVEN[int(x)] for x in rng.integers(0, 11, 5)) for _ in range(3000)]
    assert len(seqs) == 11 + 121 + 1331 + 14641 + 3000
    for names in seqs:
        chain = [letters[(nm, at)] for at, nm in enumerate(names)]
        for pname, prior in pri.items():
            assert bm.replay_all(chain, prior) == (fm.replay(chain, prior), len(chain), EXECUTED), (names, pname)


def test_the_save_pattern():
    """K2HArchive::Save for a large value: SET_ALL with an empty value, then OW_VAL chunks at
    ascending offsets (lib/k2harchive.cc:137-150, :194-245).  It leaves the table of SET_ALL(X)."""
    for chunk in (1, 7, 16):
        for n in range(51):
            x = bytes((3 * i + n) & 0xFF for i in range(n))
            log = [Rec(fm.SET_ALL, KEY, b"", b"subkeys", b"attrs")]
            log += [ow(KEY, at, x[at:at + chunk]) for at in range(0, n, chunk)]
            want = fm.replay([Rec(fm.SET_ALL, KEY, x, b"subkeys", b"attrs")], {})
            for prior in ({}, {KEY: (b"an older and longer value" * 3, None, b"old")}):
                if prior and n < 75:
                    continue   # (SET_ALL's empty value clears the old one: checked on the empty prior)
                assert bm.replay_all(log, prior) == (want, len(log), EXECUTED), (chunk, n)
            t, at, outcome = bm.replay_all(log, {KEY: (b"older", b"s0", None)})
            assert t == want and outcome == EXECUTED


def _arena(oracle, table):
    held, off = am.prior_held(oracle, table)
    return held, [int(x) for x in off]


def _hashes(oracle, log, variant=0):
    h1, h2 = am.rec_hashes(oracle, log, variant)
    new = [Rec(0, r.exdata if r.type == RENAME and r.status == 0 else b"") for r in log]
    n1, n2 = am.rec_hashes(oracle, new, variant)
    return h1, h2, n1, n2


def _table(m):
    """The table an arena leaves: the kept blobs, a later blob of a key replacing an earlier one."""
    keep = m.held_keep
    off = [int(x) for x in m.held_off]
    blobs = [m.arena[off[j]:off[j + 1]] for j in range(len(off) - 1) if keep[j]]
    return am.table_of(*rm.join(blobs)) if blobs else {}


def test_a_run_at_once_is_the_records_one_by_one(oracle):
    """Overlapping, out of order and with gaps; every split point of a five-record run; and the
    sequential execute over the dict table says the same."""
    runs = {
        "overlapping": [(0, b"AAAAAAAA"), (4, b"BBBBBBBB"), (2, b"CC"), (6, b"DDDDDDDDDD"), (0, b"E")],
        "out of order": [(20, b"tail"), (10, b"middle"), (0, b"head"), (16, b"XXXX"), (4, b"YYYYYY")],
        "gaps": [(5, b"a"), (30, b"bcd"), (12, b"efgh"), (40, b"i"), (29, b"j")],
        "hidden": [(3, b"xyz"), (0, b"0123456789"), (3, b"x"), (9, b"9876"), (2, b"--")],
    }
    for what, writes in runs.items():
        for pname, prior in fm.priors(KEY).items():
            held, off = _arena(oracle, prior)
            log = [ow(KEY, o, d) for o, d in writes]
            file, recs = am.build_log(log)
            hs = _hashes(oracle, log)
            once = bm.barrier_model(held, off, None, file, recs, 0, None, hs)
            assert once.result[:2] == [EXECUTED, 5] and once.result[4] == (0 if pname == "absent" else 1)
            want = dict(prior)
            flags, each = 0, []
            for r in log:
                outcome, f = bm.execute(want, r)
                assert outcome == EXECUTED
                flags |= f
                each.append(f & GAP)
            # GAP is the call's: a byte of the final value under neither the old value nor a write of
            # the run.  A record's own stretch that a later record of the run fills is none, so the
            # run can have none where its records, one by one, have some -- never the other way round.
            seen = bytearray(len(want[KEY][0]))
            seen[:len((prior.get(KEY) or (None,))[0] or b"")] = b"\1" * len((prior.get(KEY) or (None,))[0] or b"")
            for o, d in writes:
                seen[o:o + len(d)] = b"\1" * len(d)
            gap = GAP if 0 in seen else 0
            assert _table(once) == want and once.result[3] == (flags & CREATED) | gap, (what, pname)
            assert gap <= flags & GAP and (what != "gaps" or gap) and (what != "hidden" or pname != "absent" or (not gap and flags & GAP))
            assert once.result[6] == len(want[KEY][0])
            for cut in range(1, 5):
                cons = np.ones(5, np.uint8)
                cons[cut] = 0                                   # ends the first run at the cut
                a = bm.barrier_model(held, off, None, file, recs, 0, cons, hs)
                assert a.result[1] == cut
                b = bm.barrier_model(a.arena, a.held_off, a.held_keep, file, recs, cut, None, hs)
                assert b.result[1] == 5 - cut and b.result[3] & CREATED == 0
                assert _table(b) == want, (what, pname, cut)
                assert gap <= (a.result[3] | b.result[3]) & GAP <= flags & GAP
            m = bm.barrier_model(held, off, None, file, recs, 0, np.array([1, 0, 1, 0, 1]), hs)
            assert m.result[3] & GAP == each[0]
            for i in range(1, 5):                               # one call per record: the record's own flag
                assert m.result[1] == 1
                m = bm.barrier_model(m.arena, m.held_off, m.held_keep, file, recs, i,
                                     np.eye(5, dtype=np.uint8)[i], hs)
                assert m.result[3] == each[i], (what, pname, i)
            assert _table(m) == want, (what, pname)


def test_rename_there_and_back():
    for pname, prior in fm.priors(KEY).items():
        t = dict(prior)
        first = bm.execute(t, ren(KEY, b"another-key"))
        if pname == "absent":
            assert first == (NOT_FOUND, 0) and t == prior
            continue
        assert first == (EXECUTED, 0) and KEY not in t and t[b"another-key"] == prior[KEY]
        assert bm.execute(t, ren(b"another-key", KEY)) == (EXECUTED, 0) and t == prior
        assert bm.execute(t, ren(KEY, KEY)) == (EXECUTED, 0) and t == prior       # onto itself


def test_rename_with_attrs_replaces_the_attrs_only():
    for pname, prior in fm.priors(KEY).items():
        if pname == "absent":
            continue
        t = dict(prior)
        assert bm.execute(t, ren(KEY, b"n", b"new-attrs")) == (EXECUTED, 0)
        assert t == {b"n": prior[KEY][:2] + (b"new-attrs",)}


def test_a_wrong_rename_rule_is_told_apart():
    """The control: a RENAME that always takes the record's attrs, even when it has none."""
    wrong = lambda rec, old: rec  # noqa: E731
    prior = fm.priors(KEY)["vsa"]
    right_t, wrong_t = dict(prior), dict(prior)
    bm.execute(right_t, ren(KEY, b"n"))
    bm.execute(wrong_t, ren(KEY, b"n"), rename_attrs=wrong)
    assert right_t[b"n"] == (b"pv", b"ps", b"pa") and wrong_t[b"n"] == (b"pv", b"ps", None)
    bm.execute(wrong_t, ren(b"n", b"m", b"x"), rename_attrs=wrong)
    bm.execute(right_t, ren(b"n", b"m", b"x"))
    assert right_t == wrong_t                                   # (with attrs the two rules agree)


def test_every_outcome(oracle):
    prior = {KEY: (b"value", b"sk", b"at"), b"other": (b"o", None, None)}
    cases = [(ren(KEY, b"new"), EXECUTED, 0), (ren(b"stranger", b"new"), NOT_FOUND, 0), (ren(KEY, b"other"), NEW_EXISTS, 0),
             (ren(b"stranger", b"other"), NOT_FOUND, 0), (ren(KEY, b""), BAD_RECORD, 0),
             (ow(KEY, 2, b"xx"), EXECUTED, 0), (ow(KEY, 5, b"xx"), EXECUTED, 0), (ow(KEY, 6, b"xx"), EXECUTED, GAP),
             (ow(b"stranger", 0, b"xx"), EXECUTED, CREATED), (ow(b"stranger", 1, b"xx"), EXECUTED, CREATED | GAP),
             (ow(KEY, 0, b""), BAD_RECORD, 0), (ow(KEY, -1, b"xx"), BAD_RECORD, 0), (ow(KEY, 0, b"xx", exlen=0), BAD_RECORD, 0),
             (Rec(OW_VAL, KEY, b"xx", b"", b"", b"\0" * 9), BAD_RECORD, 0), (ow(KEY, 3, b"xx", exlen=1), EXECUTED, 0),
             (ow(KEY, 0x0102, b"xx", exlen=4), EXECUTED, GAP), (ow(b"", 0, b"xx"), NOT_A_BARRIER, 0),
             (ow(KEY, 0, b"xx")._replace(status=2), NOT_A_BARRIER, 0), (fm.letter("set-v", KEY, 0), NOT_A_BARRIER, 0)]
    seen = set()
    held, off = _arena(oracle, prior)
    for r, outcome, flags in cases:
        t = dict(prior)
        assert bm.execute(t, r) == (outcome, flags), r
        assert (t == prior) == (outcome != EXECUTED or r == ow(KEY, 0, b""))
        file, recs = am.build_log([r])
        m = bm.barrier_model(held, off, None, file, recs, 0, None, _hashes(oracle, [r]))
        assert m.result[0] == outcome and m.result[3] == flags, r
        if outcome == EXECUTED:
            assert _table(m) == t and m.result[1] == 1 and m.result[2] == len(m.arena) - len(held)
        else:
            assert m.arena == held and m.result[1:] == [0, 0, 0, 0, bm.NONE, 0, 0]
        seen.add(outcome)
    assert seen == {EXECUTED, NOT_FOUND, NEW_EXISTS, BAD_RECORD, NOT_A_BARRIER}
    # err_skip passes over NOT_FOUND and BAD_RECORD, never over NEW_EXISTS
    log = [ren(b"stranger", b"x"), ow(KEY, 0, b""), ren(KEY, b"other"), fm.letter("del", KEY, 3)]
    assert bm.replay_all(log, prior)[1:] == (0, NOT_FOUND)
    assert bm.replay_all(log, prior, err_skip=True) == (prior, 2, NEW_EXISTS)
    assert bm.replay_all(log[:2] + log[3:], prior, err_skip=True) == ({b"other": (b"o", None, None)}, 3, EXECUTED)


def test_the_last_copy_decides_and_every_copy_is_cleared(oracle):
    hs = am.hashes_of(oracle, [KEY, b"n"])
    blobs = [layout(hs[KEY], KEY, b"copy-%d" % c, b"S%d" % c, b"") for c in range(3)]
    held, off = rm.join(blobs)
    log = [ren(KEY, b"n")]
    file, recs = am.build_log(log)
    m = bm.barrier_model(held, off, [1, 1, 1], file, recs, 0, None, _hashes(oracle, log))
    assert m.result == [EXECUTED, 1, 80 + 1 + 6 + 2, 0, 3, 2, 6, 0] and m.held_keep.tolist() == [0, 0, 0, 1]
    assert _table(m) == {b"n": (b"copy-2", b"S2", None)}
    m = bm.barrier_model(held, off, [1, 1, 0], file, recs, 0, None, _hashes(oracle, log))
    assert m.result[4:6] == [2, 1] and m.held_keep.tolist() == [0, 0, 0, 1]
    m = bm.barrier_model(held, off, [0, 0, 0], file, recs, 0, None, _hashes(oracle, log))
    assert m.result[0] == NOT_FOUND


def test_every_einval_without_a_device():
    """Judged on the host before any device is touched, each with its own message."""
    lib = _native.batch_lib()
    na, n = 2, 3
    held, hoff, keep = np.full(400, 0xEE, np.uint8), np.arange(na + 2, dtype=np.uint64) * 100, np.ones(na + 1, np.uint8)
    file, recs, h = np.zeros(400, np.uint8), np.zeros(n, archive.REC_DTYPE), np.zeros(n, np.uint64)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    result = (ctypes.c_uint64 * 8)()
    rp = ctypes.cast(result, ctypes.POINTER(ctypes.c_uint64))
    msg = lambda: bytes(lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL))  # noqa: E731

    def args(**kw):
        d = dict(held=p(held), size=200, cap=400, hoff=p(hoff), na=na, keep=p(keep), file=p(file), recs=p(recs), n=n, b=1,
                 h1=p(h), h2=p(h), n1=p(h), n2=p(h), flags=0, result=rp)
        d.update(kw)
        return (d["held"], d["size"], d["cap"], d["hoff"], d["na"], d["keep"], d["file"], file.size, d["recs"], d["n"], d["b"],
                None, d["h1"], d["h2"], d["n1"], d["n2"], d["flags"], d["result"], None)
    cases = ((dict(result=None), b"NULL result"), (dict(keep=None), b"NULL held_keep"), (dict(held=None), b"NULL held"),
             (dict(hoff=None), b"NULL held_off"), (dict(file=None), b"NULL file"), (dict(recs=None), b"NULL recs"),
             (dict(b=3), b"b is not below n"), (dict(b=(1 << 64) - 1), b"b is not below n"), (dict(n=0, b=0), b"b is not below n"),
             (dict(cap=199), b"held_cap is below held_size"), (dict(h1=None), b"together"), (dict(n2=None), b"together"),
             (dict(h2=None, n1=None), b"together"), (dict(flags=2), b"unknown flags"), (dict(flags=0x200), b"unknown flags"),
             (dict(flags=1), b"only when the hashes are NULL"), (dict(flags=0x101), b"only when the hashes are NULL"),
             (dict(na=(1 << 32) - 1), b"2^32 - 2"),
             (dict(na=0, held=None, hoff=None), b"without K2H_AMD_BARRIER_COUNT_ONLY"))
    texts = set()
    for kw, text in cases:
        for i in range(8):
            result[i] = 7
        assert lib.k2h_amd_archive_barrier(*args(**kw)) == _native.K2H_AMD_EINVAL, kw
        assert text in msg() and msg().startswith(b"archive_barrier: "), (kw, msg())
        if "result" not in kw:
            assert list(result) == [bm.NOT_A_BARRIER, 0, 0, 0, 0, bm.NONE, 0, 0]
        texts.add(msg())
    assert len(texts) == 13 and (held == 0xEE).all() and (keep == 1).all()


def test_exports_and_constants():
    import k2hash_amd
    from k2hash_amd import barrier
    for name in ("execute_barrier", "replay_log", "Executed", "Replayed"):
        assert name in k2hash_amd.__all__ and getattr(k2hash_amd, name) is getattr(barrier, name)
    assert barrier.Replayed._fields == ("blobs", "blob_off", "segments", "barriers", "stopped_at", "outcome")
    assert barrier.Executed._fields[:6] == ("outcome", "executed", "flags", "appended", "na", "used")
    assert (barrier.BARRIER_EXECUTED, barrier.BARRIER_NOT_FOUND, barrier.BARRIER_NEW_EXISTS, barrier.BARRIER_BAD_RECORD,
            barrier.BARRIER_NOT_A_BARRIER) == (EXECUTED, NOT_FOUND, NEW_EXISTS, BAD_RECORD, NOT_A_BARRIER)
    assert (barrier.BARRIER_CREATED, barrier.BARRIER_GAP, barrier.BARRIER_MAX_RUN) == (CREATED, GAP, bm.MAX_RUN)
    assert _native.K2H_AMD_BARRIER_COUNT_ONLY == bm.COUNT_ONLY
    header = (rm.ROOT / "include" / "k2hash_amd.h").read_text()
    for name in ("EXECUTED", "NOT_FOUND", "NEW_EXISTS", "BAD_RECORD", "NOT_A_BARRIER", "CREATED", "GAP", "COUNT_ONLY", "MAX_RUN"):
        value = getattr(_native, "K2H_AMD_BARRIER_" + name)
        assert f"#define K2H_AMD_BARRIER_{name} {value:#x}u" in header or f"#define K2H_AMD_BARRIER_{name} {value}" in header
