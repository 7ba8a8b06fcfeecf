"""OW_VAL and RENAME executed on a held arena (include/k2hash_amd.h section 5d:
k2h_amd_archive_barrier; k2h_archive_barrier.hip) against the model of archive_barrier_model.py,
byte for byte: the appended blob, held_off, held_keep and the eight result words; and
barrier.replay_log against the sequential replay of the whole log.

Expected values never come from a device call.  The arena is sentinel-filled behind its used
bytes and lies at an odd shift between canaries, held_off and held_keep are sentinel-filled behind
their entries, and the file stands at an odd shift between canaries of its own.
"""
import struct

import numpy as np
import pytest

from conftest import GOLDEN

import archive_apply_model as am
import archive_barrier_model as bm
import archive_fold_model as fm
import ralle_archive_model as ra
import ralle_check_model as rm
from archive_barrier_model import BAD_RECORD, CREATED, EXECUTED, GAP, NEW_EXISTS, NOT_A_BARRIER, NOT_FOUND
from archive_fold_model import OW_VAL, RENAME, Rec
from ralle_unlink_model import layout
from test_archive_barrier_model import _hashes, _table, ow, ren

from k2hash_amd import _native, archive


def test_kernels_keep_the_register_budget(tmp_path):
    """Every kernel of k2h_archive_barrier.hip: at most 64 VGPRs, no scratch, no spills."""
    import subprocess
    from pathlib import Path

    import test_archive_device as tad
    if not Path(tad.HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "k2h_archive_barrier.s"
    subprocess.run([tad.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    f"-I{tad.ROOT / 'include'}", str(tad.CSRC / "k2h_archive_barrier.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    kernels = {k: v for k, v in tad._kernel_meta(out.read_text()).items() if "barrier_" in k}
    for name in ("barrier_judge_kernel", "barrier_locate_kernel", "barrier_size_kernel", "barrier_build_kernel"):
        assert any(name in k for k in kernels), (name, sorted(kernels))
    for sym, f in kernels.items():
        assert f.get("vgpr_count", 999) <= 64, (sym, f.get("vgpr_count"))
        assert f.get("private_segment_fixed_size", 0) == 0, sym
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, sym


# ------------------------------------------------------------------------------------- GPU
def against_model(cuda, oracle, held, off, log, what, b=0, keep=None, consider=None, inside=False, bare=None, variant=0,
                  mutate=None, hashes=None, slack=None, **kw):
    """The call over the arena (held, off, keep) and record b of the list of Rec `log` against
    the model.  inside: the hashes are computed by the call (the model uses the oracle's);
    mutate: a function that changes the host records before both see them; slack: the arena's
    bytes behind the used ones (None: what the model appends, and 37 more)."""
    file, recs = am.build_log(log) if bare is None else am.bare_log(log, bare)
    if mutate is not None:
        mutate(recs, len(file))
    hs = _hashes(oracle, log, variant) if hashes is None else hashes
    m = bm.barrier_model(held, off, keep, file, recs, b, consider, hs)
    slack = m.result[2] + 37 if slack is None else slack
    got = bm.run_barrier(cuda, held, off, keep, file, recs, b, consider=consider, hashes=None if inside else hs,
                         flags=variant if inside else 0, slack=slack, **kw)
    bm.assert_barrier(got, m, what, len(held))
    return got, m


def _held(oracle, table, lead=b""):
    keys = sorted(table)
    hs = am.hashes_of(oracle, keys)
    return rm.join([layout(hs[k], k, *(x or b"" for x in table[k])) for k in keys], lead=lead)


def _pattern(n, salt=0):
    return bytes((salt + 7 * i + (i >> 8)) & 0xFF for i in range(n))


@pytest.mark.gpu
def test_the_golden_archive(cuda, oracle):
    """The OW_VAL and RENAME records the reference wrote, executed against a stream that holds
    their keys: the exdata parsing on the reference's own bytes."""
    f = (GOLDEN / "archive.k2har").read_bytes()
    recs = archive.scan(f)
    log = fm.recs_of(f, recs)
    hs = _hashes(oracle, log)
    barriers = [i for i, r in enumerate(log) if r.type in (OW_VAL, RENAME)]
    assert len(barriers) == 18 and {len(log[i].exdata) for i in barriers if log[i].type == OW_VAL} == {8}
    table = {log[i].key: (_pattern(400 if k % 3 else 5000, k), b"sub-%d" % k if k % 2 else None, b"att" if k % 4 else None)
             for k, i in enumerate(barriers)}
    held, off = _held(oracle, table, lead=b"\x66" * 3)
    flags = set()
    for inside in (False, True):
        for i in barriers:
            m = bm.barrier_model(held, off, None, f, recs, i, None, hs)
            got = bm.run_barrier(cuda, held, off, None, f, recs, i, hashes=None if inside else hs, slack=m.result[2] + 5)
            bm.assert_barrier(got, m, f"golden record {i}", len(held))
            assert m.result[:2] == [EXECUTED, 1] and m.result[4] == 1
            flags.add(m.result[3])
    assert flags == {0, GAP}
    # ... and against the empty stream: every RENAME finds nothing, every OW_VAL creates its key
    for i in barriers:
        m = bm.barrier_model(b"", [0], None, f, recs, i, None, hs)
        bm.assert_barrier(bm.run_barrier(cuda, b"", [0], None, f, recs, i, slack=m.result[2] + 1), m, f"golden {i}, na = 0", 0)
        assert m.result[0] == (NOT_FOUND if log[i].type == RENAME else EXECUTED)
        assert log[i].type == RENAME or m.result[3] == CREATED | GAP


@pytest.mark.gpu
def test_rename_cases(cuda, oracle):
    old, new, other = b"the-old-key", b"a-new-key-of-another-length", b"someone-else"
    table = {old: (b"value-bytes", b"subkeys", b"attrs"), other: (b"o", None, None)}
    held, off = _held(oracle, table, lead=b"\x21" * 5)
    got, m = against_model(cuda, oracle, held, off, [ren(old, new)], "without attrs")
    assert _table(m) == {new: table[old], other: table[other]} and m.result[4:6] == [1, 1]
    got, m = against_model(cuda, oracle, held, off, [ren(old, new, b"the-record's")], "with attrs")
    assert _table(m)[new] == (b"value-bytes", b"subkeys", b"the-record's")

    def attrs_outside(recs, size):
        recs[0]["attrs_off"] = size - 3
    got, m = against_model(cuda, oracle, held, off, [ren(old, new, b"the-record's")], "attrs outside the file", mutate=attrs_outside)
    assert _table(m)[new] == table[old]
    got, m = against_model(cuda, oracle, held, off, [ren(b"not-held", new)], "not held")
    assert m.result[0] == NOT_FOUND
    got, m = against_model(cuda, oracle, held, off, [ren(old, other)], "the new key is held")
    assert m.result[0] == NEW_EXISTS
    got, m = against_model(cuda, oracle, held, off, [ren(b"not-held", other)], "not held, new key held")
    assert m.result[0] == NOT_FOUND
    got, m = against_model(cuda, oracle, held, off, [ren(old, other)], "the new key is held but not kept", keep=[0, 1])
    assert m.result[0] == EXECUTED       # (sorted keys: someone-else, the-old-key)
    got, m = against_model(cuda, oracle, held, off, [ren(old, old, b"A2")], "onto itself")
    assert m.result[0] == EXECUTED and _table(m)[old] == (b"value-bytes", b"subkeys", b"A2") and m.held_keep.tolist() == [1, 0, 1]
    got, m = against_model(cuda, oracle, held, off, [ren(old, new)], "held but not kept", keep=[1, 0])
    assert m.result[0] == NOT_FOUND
    for what, mutate in (("no exdata", lambda r, size: r[0].__setitem__("exdata_len", 0)),
                         ("exdata outside the file", lambda r, size: r[0].__setitem__("exdata_off", size - 2))):
        got, m = against_model(cuda, oracle, held, off, [ren(old, new)], what, mutate=mutate)
        assert m.result[0] == BAD_RECORD
    # three copies: all three cleared, the last decides
    hs = am.hashes_of(oracle, [old, other])
    blobs = [layout(hs[k], k, b"copy-%d" % c, b"S%d" % c if c != 1 else b"", b"A%d" % c) for c in range(3) for k in (old, other)]
    held3, off3 = rm.join(blobs, lead=b"\x11" * 7)
    got, m = against_model(cuda, oracle, held3, off3, [ren(old, new)], "held three times")
    assert m.held_keep.tolist() == [0, 1, 0, 1, 0, 1, 1] and m.result[4:6] == [3, 4] and _table(m)[new] == (b"copy-2", b"S2", b"A2")
    got, m = against_model(cuda, oracle, held3, off3, [ren(old, new)], "held three times, the last not kept",
                           keep=[1, 1, 1, 1, 0, 1])
    assert m.held_keep.tolist() == [0, 1, 0, 1, 0, 1, 1] and m.result[4:6] == [2, 2] and _table(m)[new] == (b"copy-1", None, b"A1")
    # a wrong stored hash or subhash: never matched
    for which in (0, 1):
        h = list(hs[old])
        h[which] ^= 1 << 40
        heldw, offw = rm.join([layout(h, old, b"stale", b"", b"")])
        got, m = against_model(cuda, oracle, heldw, offw, [ren(old, new)], "a wrong stored hash")
        assert m.result[0] == NOT_FOUND
    # the target's hashes and length over a key that differs in one byte, as the old and as the new key
    for at in (0, len(old) - 1):
        twin = bytearray(old)
        twin[at] ^= 0x20
        heldt, offt = rm.join([layout(hs[old], bytes(twin), b"twin", b"", b""), layout(hs[other], other, b"o", b"", b"")])
        got, m = against_model(cuda, oracle, heldt, offt, [ren(old, new)], f"one key byte differs at {at}")
        assert m.result[0] == NOT_FOUND
        hn = am.hashes_of(oracle, [bytes(twin)])[bytes(twin)]
        heldt, offt = rm.join([layout(hs[old], old, b"v", b"", b""), layout(hn, old, b"twin of the new key", b"", b"")])
        got, m = against_model(cuda, oracle, heldt, offt, [ren(old, bytes(twin))], f"the new key's twin at {at}")
        assert m.result[0] == EXECUTED and m.held_keep.tolist() == [0, 1, 1]


@pytest.mark.gpu
def test_rename_key_lengths_and_file_offsets(cuda, oracle):
    """Keys of 1..100 bytes, the record's key at file offsets 0..15."""
    keys = [bytes((11 * j + ln) & 0xFF for j in range(ln)) for ln in range(1, 101)]
    table = {k: (b"v" + k[:5], None, b"a") for k in keys}
    held, off = _held(oracle, table)
    cases = [(ln, ln % 16) for ln in range(1, 101)] + [(ln, at) for ln in (1, 15, 16, 17, 33, 100) for at in range(16)]
    for ln, at in cases:
        k = keys[ln - 1]
        got, m = against_model(cuda, oracle, held, off, [ren(k, k[::-1] + b"+")], f"key of {ln} bytes at {at}", bare=at,
                               fshift=(5 * at + 1) % 16)
        assert m.result[0] == EXECUTED and m.result[2] == 80 + ln + 1 + len(table[k][0]) + 1


@pytest.mark.gpu
def test_rename_forged_sources(cuda, oracle):
    """Permuted, gapped and overlapping segments with slack in the deciding blob."""
    k1, k2, k3 = b"forged-one", b"forged-two-with-a-longer-key", b"f3"
    hs = am.hashes_of(oracle, [k1, k2, k3])
    f1 = ra.forge(k1, b"value-one" * 5, b"subkeys-1", b"attrs-1", order=(3, 1, 0, 2), gaps=(5, 0, 9, 1), slack=13, hashes=hs[k1])
    f2 = ra.forge(k2, b"v2", b"s" * 33, b"a" * 17, order=(2, 3, 1, 0), gaps=(0, 3, 0, 7), slack=1, hashes=hs[k2])
    f3 = ra.forge(k3, b"0123456789abcdefXYZ", hashes=hs[k3], slack=4)
    rm.put(f3, 0, rm.F_SLEN, 7), rm.put(f3, 0, rm.F_SPOS, 80 + len(k3) + 3)     # the subkeys lie inside the value
    rm.put(f3, 0, rm.F_ALEN, 5), rm.put(f3, 0, rm.F_APOS, 80 + len(k3) - 1)     # the attrs across key and value
    held, off = rm.join([f1, f2, f3], lead=b"\x22")
    for i, k in enumerate((k1, k2, k3)):
        for hshift in (0, 9):
            got, m = against_model(cuda, oracle, held, off, [ren(k, b"renamed-" + k)], f"forged source {i}", hshift=hshift)
            assert m.result[0] == EXECUTED
            got, m = against_model(cuda, oracle, held, off, [ow(k, 1, b"PATCH-OVER-IT")], f"forged source {i}, OW_VAL", hshift=hshift)
    assert _table(m)[k3] == (b"0PATCH-OVER-ITefXYZ", b"3456789", b"30123")


SIZES = (0, 1, 15, 16, 17, 4096, 65536)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_rename_segment_sizes_at_every_output_alignment(cuda, oracle, size):
    rng = ra._rng(44, size)
    key = b"shape-key"
    v, s, a = (ra.rbytes(rng, size) for _ in range(3))
    hs = am.hashes_of(oracle, [key])
    blobs = [layout(hs[key], key, v, s, a), layout(hs[key], key, v, b"", b""), layout(hs[key], key, b"", s, b"x"),
             layout(hs[key], key, b"y", b"", a)]
    for hshift in range(16):            # the arena's shift is the output's alignment
        j = hshift % 4
        held, off = rm.join(blobs[:j + 1], lead=b"\x33" * hshift)
        got, m = against_model(cuda, oracle, held, off, [ren(key, b"renamed")], f"segments of {size} at {hshift}", hshift=hshift,
                               fshift=(3 * hshift + 1) % 16)
        assert m.result[0] == EXECUTED and m.result[5] == j and m.result[4] == j + 1


@pytest.mark.gpu
def test_ow_val_cases(cuda, oracle):
    key = b"direct-access"
    value = _pattern(40)
    held, off = _held(oracle, {key: (value, b"sk", b"at"), b"z": (b"zz", None, None)}, lead=b"\x09")
    for what, r, flags, vlen in (("offset 0", ow(key, 0, b"HEAD"), 0, 40), ("in the middle", ow(key, 17, b"MIDDLE"), 0, 40),
                                 ("across the end", ow(key, 38, b"ACROSS"), 0, 44), ("at the end", ow(key, 40, b"APPEND"), 0, 46),
                                 ("past the end", ow(key, 57, b"FAR"), GAP, 60),
                                 ("absent", ow(b"absent", 0, b"NEW"), CREATED, 3),
                                 ("absent, past 0", ow(b"absent", 33, b"NEW"), CREATED | GAP, 36),
                                 ("exdata of 1 byte", ow(key, 7, b"x", exlen=1), 0, 40),
                                 ("exdata of 4 bytes", ow(key, 0x0101, b"x", exlen=4), GAP, 0x102)):
        got, m = against_model(cuda, oracle, held, off, [r], what)
        assert m.result[0] == EXECUTED and m.result[3] == flags and m.result[6] == vlen, what
        t = _table(m)
        assert t[r.key][1:] == ((b"sk", b"at") if r.key == key else (None, None)) and t[b"z"] == (b"zz", None, None)
    for what, r in (("exdata of 9 bytes", Rec(OW_VAL, key, b"xx", b"", b"", b"\x01" + b"\0" * 8)),
                    ("no exdata", ow(key, 0, b"xx", exlen=0)), ("a negative offset", ow(key, -1, b"xx")),
                    ("the lowest offset", ow(key, -(1 << 63), b"xx")), ("no data", ow(key, 3, b""))):
        got, m = against_model(cuda, oracle, held, off, [r], what)
        assert m.result[0] == BAD_RECORD, what
    for what, field in (("val outside the file", "val_off"), ("exdata outside the file", "exdata_off")):
        got, m = against_model(cuda, oracle, held, off, [ow(key, 3, b"data")], what,
                               mutate=lambda r, size, f=field: r[0].__setitem__(f, size - 1))
        assert m.result[0] == BAD_RECORD, what
    for what, mutate in (("a bad status", lambda r, size: r[0].__setitem__("status", 2)),
                         ("another type", lambda r, size: r[0].__setitem__("type", 1)),
                         ("no key", lambda r, size: r[0].__setitem__("key_len", 0)),
                         ("the key outside the file", lambda r, size: r[0].__setitem__("key_off", size))):
        got, m = against_model(cuda, oracle, held, off, [ow(key, 3, b"data")], what, mutate=mutate)
        assert m.result[0] == NOT_A_BARRIER, what
    got, m = against_model(cuda, oracle, held, off, [ow(key, 3, b"data")], "not considered", consider=[0])
    assert m.result[0] == NOT_A_BARRIER
    # the largest offset: the value does not fit any arena, and the call says how much it needs
    file, recs = am.build_log([ow(key, (1 << 63) - 1, b"x")])
    got = bm.run_barrier(cuda, held, off, None, file, recs, 0, slack=64)
    assert got[0] == _native.K2H_AMD_EINVAL and got[4][:2] == [EXECUTED, 1] and got[4][6] == 1 << 63
    assert got[1][len(held):] == bytes([bm.ARENA_FILL]) * 64 and got[3].tolist() == [1, 1, 0xEE]


DATA = (1, 15, 16, 17, 4096, 65536)


@pytest.mark.gpu
@pytest.mark.parametrize("vlen", (0, 1, 15, 16, 17, 4096, 65536, (1 << 20) + 3))
def test_ow_val_sizes_and_alignments(cuda, oracle, vlen):
    """Data of every size onto a value of vlen bytes -- at its start, inside it, across its end and
    behind it -- the file's shift walking through the 16 relative alignments of source and
    destination; for the 17-byte and 4,096-byte data every one of the 16."""
    key = b"sized"
    value = _pattern(vlen, 3)
    held, off = _held(oracle, {key: (value, b"subkeys", b"a")}, lead=b"\x0c" * 3)
    step = 0
    for dlen in DATA:
        data = _pattern(dlen, 101)
        places = sorted({0, max(vlen - dlen, 0) // 2 + 1, max(vlen - dlen // 2, 0), vlen, vlen + 5})
        for at in places:
            shifts = range(16) if dlen in (17, 4096) and at == places[1] and vlen in (17, 4096) else (step % 16,)
            for fshift in shifts:
                got, m = against_model(cuda, oracle, held, off, [ow(key, at, data)], f"{dlen} bytes at {at} of {vlen}, file at {fshift}",
                                       fshift=fshift, hshift=(7 * step + 5) % 16)
                step += 1
                assert m.result[6] == max(vlen, at + dlen) and m.result[3] == (GAP if at > vlen else 0)
    assert step >= 16


def _run_log(key, n, kind):
    if kind == "save":            # ascending disjoint appends: K2HArchive::Save's chunks
        return [ow(key, 13 * i, _pattern(13, i)) for i in range(n)]
    if kind == "overlap":         # every write half over the one before it
        return [ow(key, 5 * i, _pattern(11, i)) for i in range(n)]
    if kind == "hidden":          # the last write hides all before it
        return [ow(key, 3 + (7 * i) % 50, _pattern(1 + i % 9, i)) for i in range(n - 1)] + [ow(key, 0, _pattern(80, 200))][:n]
    assert kind == "disorder"     # descending and interleaved offsets, gaps between them
    return [ow(key, 40 * ((n - 1 - i) ^ 1) + (i % 3), _pattern(1 + (17 * i) % 37, i)) for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 2, 64, 65, 256, 257))
def test_runs(cuda, oracle, n):
    key = b"a-long-value"
    held, off = _held(oracle, {key: (_pattern(100, 9), b"s", None), b"bystander": (b"b", None, None)})
    for kind in ("save", "overlap", "hidden", "disorder"):
        log = _run_log(key, n, kind) + [fm.letter("set-v", b"bystander", 0)]
        for h, o, prior in ((held, off, "held"), (b"", [0], "absent")):
            got, m = against_model(cuda, oracle, h, o, log, f"{kind} run of {n}, {prior}", fshift=n % 16)
            assert m.result[1] == min(n, 256)
            want = {} if prior == "absent" else {key: (_pattern(100, 9), b"s", None)}
            for r in log[:m.result[1]]:
                bm.execute(want, r)
            assert _table(m).get(key) == want[key], (kind, n, prior)
    # the run that starts in the middle of the log
    log = [fm.letter("set-v", key, 0)] * 3 + _run_log(key, n, "overlap")
    got, m = against_model(cuda, oracle, held, off, log, f"run of {n} from record 3", b=3)
    assert m.result[1] == min(n, 256)


@pytest.mark.gpu
def test_what_ends_a_run(cuda, oracle):
    key, twin = b"run-key-0123456789", b"run-key-012345678X"
    held, off = _held(oracle, {key: (b"old", None, b"A")})
    base = _run_log(key, 9, "overlap")
    enders = {"another key": ow(twin, 0, b"t"), "a shorter key": ow(key[:-1], 0, b"t"), "another type": fm.letter("rep-v", key, 5),
              "a rename": ren(key, b"n"), "a bad status": base[5]._replace(status=2), "no data": ow(key, 2, b""),
              "a negative offset": ow(key, -5, b"x"), "an exdata of 9 bytes": Rec(OW_VAL, key, b"x", b"", b"", b"\0" * 9)}
    for what, r in enders.items():
        for at in (1, 5, 8):
            log = base[:at] + [r] + base[at + 1:]
            got, m = against_model(cuda, oracle, held, off, log, f"{what} at {at}")
            assert m.result[:2] == [EXECUTED, at], what
    for at in (1, 5, 8):
        cons = np.ones(9, np.uint8)
        cons[at] = 0
        got, m = against_model(cuda, oracle, held, off, base, f"not considered at {at}", consider=cons)
        assert m.result[:2] == [EXECUTED, at]
        got, m = against_model(cuda, oracle, held, off, base, f"val outside the file at {at}",
                               mutate=lambda r, size, at=at: r[at].__setitem__("val_len", size))
        assert m.result[:2] == [EXECUTED, at]


def _mutants(oracle, key):
    """Blobs of `key` that take no part, beside the one that does: EMPTY, NO_KEY, BAD_RANGE, a
    span of 79 bytes; (blobs, the index of the good one)."""
    hs = am.hashes_of(oracle, [key])[key]
    blobs = [bytearray(layout(hs, key, b"value-%d" % i, b"", b"AT")) for i in range(6)]
    for f in (rm.F_KLEN, rm.F_VLEN, rm.F_ALEN):
        rm.put(blobs[0], 0, f, 0)
    rm.put(blobs[1], 0, rm.F_KLEN, 0)
    rm.put(blobs[2], 0, rm.F_VPOS, len(blobs[2]) - 3)
    blobs[4] = blobs[4][:79]
    rm.put(blobs[5], 0, rm.F_APOS, 79)
    return blobs, 3


@pytest.mark.gpu
def test_arena(cuda, oracle):
    key = b"the-target"
    # na = 0
    got, m = against_model(cuda, oracle, b"", [0], [ow(key, 0, b"first")], "na = 0, OW_VAL")
    assert m.result == [EXECUTED, 1, 80 + len(key) + 5, CREATED, 0, bm.NONE, 5, 0] and m.held_keep.tolist() == [1]
    got, m = against_model(cuda, oracle, b"", [0], [ren(key, b"n")], "na = 0, RENAME")
    assert m.result[0] == NOT_FOUND
    # non-participants and bad spans beside the target
    blobs, good = _mutants(oracle, key)
    held, off = rm.join(blobs, lead=b"\x2a" * 11)
    for r in (ren(key, b"moved"), ow(key, 2, b"++")):
        got, m = against_model(cuda, oracle, held, off, [r], "mutants beside the target")
        assert m.result[4:6] == [1, good] and m.held_keep.tolist() == [1, 1, 1, 0, 1, 1, 1]
        bad = list(off)
        bad[1], bad[2] = off[2], off[1]          # blob 0 ends behind blob 1's start, blob 1 runs backwards
        got, m = against_model(cuda, oracle, held, bad, [r], "bad spans")
        assert m.result[4:6] == [1, good]
    # 700 blobs, more than one block: the target first, last, and as copies in three blocks
    ks, vs, ss, as_ = ra.records(ra._rng(9), 700, p_extra=0.4)
    ks = [b"%04d" % i + k for i, k in enumerate(ks)]
    hs = am.hashes_of(oracle, ks + [key])
    blobs = [layout(hs[k], k, v, s, a) for k, v, s, a in zip(ks, vs, ss, as_)]
    target = lambda c: layout(hs[key], key, b"copy-%d" % c, b"S", b"")  # noqa: E731
    for where in ([0], [699], [3, 300, 650], [255, 256]):
        bl = list(blobs)
        for c, j in enumerate(where):
            bl[j] = target(c)
        held, off = rm.join(bl, lead=b"\x44" * 5)
        for r in (ren(key, ks[1] + b"-new"), ow(key, 4, b"!")):
            got, m = against_model(cuda, oracle, held, off, [r], f"700 blobs, the target at {where}", hshift=where[0] % 16)
            assert m.result[4:6] == [len(where), where[-1]] and m.held_keep.sum() == 701 - len(where)
        got, m = against_model(cuda, oracle, held, off, [ren(key, ks[698])], "700 blobs, the new key held")
        assert m.result[0] == NEW_EXISTS


@pytest.mark.gpu
def test_count_and_capacity(cuda, oracle):
    key = b"capacity"
    hs = am.hashes_of(oracle, [key])
    held, off = rm.join([layout(hs[key], key, _pattern(300), b"sub", b""), layout(hs[key], key, _pattern(500), b"", b"at")])
    for r in (ren(key, b"renamed"), ow(key, 499, _pattern(77, 5))):
        log = [r]
        file, recs = am.build_log(log)
        hh = _hashes(oracle, log)
        m = bm.barrier_model(held, off, None, file, recs, 0, None, hh)
        need = m.result[2]
        # count only: result complete, nothing written
        got = bm.run_barrier(cuda, held, off, None, file, recs, 0, hashes=hh, flags=bm.COUNT_ONLY, slack=need)
        bm.assert_barrier(got, m, "count only", len(held), written=False, keep_before=[1, 1])
        got = bm.run_barrier(cuda, held, off, None, file, recs, 0, hashes=hh, flags=bm.COUNT_ONLY, slack=0)
        bm.assert_barrier(got, m, "count only, no room", len(held), written=False, keep_before=[1, 1])
        # one byte short: EINVAL that names both figures, result set, nothing written
        got = bm.run_barrier(cuda, held, off, None, file, recs, 0, hashes=hh, slack=need - 1)
        assert got[0] == _native.K2H_AMD_EINVAL
        text = bytes(_native.batch_lib().k2h_amd_strerror(got[0]))
        assert b"%d" % need in text and b"%d" % (need - 1) in text
        bm.assert_barrier((0,) + got[1:], m, "one byte short", len(held), written=False, keep_before=[1, 1])
        # exactly enough, and the arena's last byte the allocation's last byte
        for tail in (64, 0):
            got = bm.run_barrier(cuda, held, off, None, file, recs, 0, hashes=hh, slack=need, tail=tail, hshift=16 - (len(held) + need) % 16)
            bm.assert_barrier(got, m, f"exactly enough, {tail} bytes behind", len(held))
    # held_size below the arena's written bytes: the blob lands at held_size
    log = [ow(b"fresh", 0, b"data")]
    file, recs = am.build_log(log)
    m = bm.barrier_model(held, off, None, file, recs, 0, None, _hashes(oracle, log))
    got = bm.run_barrier(cuda, held + b"\xc3" * 100, off, None, file, recs, 0, slack=0, held_size=len(held))
    bm.assert_barrier(got, m, "room inside the allocation", len(held))


@pytest.mark.gpu
def test_hashes_inside_and_what_the_arena_feeds(cuda, oracle):
    import torch

    from k2hash_amd import ralledata
    ks, vs, ss, as_ = ra.records(ra._rng(21), 300, klen=(4, 41), p_extra=0.5)
    for variant in (0, 1):
        hv = am.hashes_of(oracle, ks, variant)
        held, off = rm.join([layout(hv[k], k, v, s, a) for k, v, s, a in zip(ks, vs, ss, as_)], lead=b"\x05" * 9)
        for r in (ren(ks[17], b"another name for it", b"ATTRS"), ow(ks[250], 3, b"overwritten"), ow(b"not held", 2, b"created")):
            got, m = against_model(cuda, oracle, held, off, [r], f"hashed inside, variant {variant}", inside=True, variant=variant)
            assert m.result[0] == EXECUTED
            # the appended blob is a good one to k2h_amd_ralledata_check, under the table's seed
            arena = torch.from_numpy(np.frombuffer(m.arena, np.uint8).copy()).to(cuda)
            aoff = torch.from_numpy(m.held_off.view(np.int64).copy()).to(cuda)
            assert got[1][:len(m.arena)] == m.arena
            st = ralledata.check_ralledata(arena, aoff, std_fnv=bool(variant)).status.cpu().numpy()
            assert (st == rm.OK).all()
            # the arena with its keep bytes through k2h_amd_archive_apply with no record: select of the model
            data, soff, index = rm.select_model(np.frombuffer(m.arena, np.uint8), m.held_off, m.held_keep)
            rc, out, ooff, origin, touched, counts, stop = am.run_apply(
                cuda, got[1][:len(m.arena)], got[2], np.zeros(0, archive.REC_DTYPE), b"", keep=got[3])
            assert rc == 0 and out == data.tobytes() and (ooff == soff).all() and (origin == index).all()
            assert counts[0] == 301 - m.result[4] and am.table_of(out, ooff) == _table(m)


# ------------------------------------------------------------------------ the wrappers
def _dev(cuda, b):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()).to(cuda)


@pytest.mark.gpu
def test_execute_barrier_wrapper(cuda, oracle):
    import torch

    from k2hash_amd import archive as arc, barrier
    key = b"wrapped"
    held, off = _held(oracle, {key: (b"0123456789", b"s", None)})
    log = [ow(key, 8, b"ABCD"), ow(key, 0, b"ab"), ren(key, b"renamed"), ren(b"nobody", b"x")]
    file, _r = am.build_log(log)
    d_file = _dev(cuda, file)
    recs, h1, h2, n1, n2 = arc.scan_prehash_device(d_file, rename=True)
    arena = torch.full((len(held) + 4096,), 0xC3, dtype=torch.uint8, device=cuda)
    arena[:len(held)] = _dev(cuda, held)
    aoff = torch.zeros(8, dtype=torch.int64, device=cuda)
    aoff[:2] = torch.tensor(off, dtype=torch.int64)
    keep = torch.ones(8, dtype=torch.uint8, device=cuda)
    c = barrier.execute_barrier(arena, aoff, keep, 1, len(held), d_file, recs, 0, count_only=True)
    assert (c.outcome, c.executed, c.na, c.used) == (EXECUTED, 2, 1, len(held)) and keep.cpu().tolist() == [1] * 8
    a = barrier.execute_barrier(arena, aoff, keep, 1, len(held), d_file, recs, 0, hashes=(h1, h2, n1, n2))
    assert (a.outcome, a.executed, a.flags, a.na, a.cleared, a.deciding, a.value_len) == (EXECUTED, 2, 0, 2, 1, 0, 12)
    assert a.used == len(held) + a.appended and a.appended == c.appended
    b = barrier.execute_barrier(arena, aoff, keep, a.na, a.used, d_file, recs, 2)
    assert (b.outcome, b.executed, b.na, b.cleared, b.deciding) == (EXECUTED, 1, 3, 1, 1)
    d = barrier.execute_barrier(arena, aoff, keep, b.na, b.used, d_file, recs, 3)
    assert (d.outcome, d.executed, d.na, d.used, d.deciding) == (NOT_FOUND, 0, 3, b.used, -1)
    assert keep.cpu().tolist()[:3] == [0, 0, 1]
    t = am.table_of(arena[int(aoff[2]):b.used].cpu().numpy().tobytes(), (aoff[2:4] - aoff[2]).cpu().numpy())
    assert t == {b"renamed": (b"ab234567ABCD", b"s", None)}
    with pytest.raises(_native.NativeError):
        barrier.execute_barrier(arena[:len(held) + 5], aoff, torch.ones(8, dtype=torch.uint8, device=cuda), 1, len(held), d_file,
                                recs, 0)
    with pytest.raises(ValueError):
        barrier.execute_barrier(arena, aoff[:2], keep, 1, len(held), d_file, recs, 0)


def _replay_case(seed, n=120, nkeys=10):
    """A log over a few keys with every record type, runs of OW_VAL chunks and renames between
    held, absent and fresh names; and a prior table."""
    rng = np.random.default_rng([808, seed])
    keys = [b"key-%d" % k * (1 + k % 3) for k in range(nkeys)]
    letters = tuple(x for x in fm.TWELVE if x != "ow")
    log = []
    while len(log) < n:
        u, key = rng.random(), keys[int(rng.integers(0, nkeys))]
        if u < 0.08:
            at = int(rng.integers(0, 30))
            for c in range(int(rng.integers(1, 6))):
                log.append(ow(key, at + 4 * c, _pattern(int(rng.integers(1, 9)), len(log))))
        elif u < 0.14:
            log.append(ren(key, b"fresh-%d" % len(log), b"ra" if rng.random() < 0.5 else b""))
            keys[keys.index(key)] = log[-1].exdata
        elif u < 0.16:
            log.append(ren(b"nobody-%d" % len(log), b"x"))                        # NOT_FOUND
        elif u < 0.18:
            log.append(ow(key, 1, b""))                                           # BAD_RECORD
        else:
            log.append(fm.letter(letters[int(rng.integers(0, 11))], key, len(log)))
    prior = {k: fm.priors(k)[("absent", "v", "s", "vsa")[int(rng.integers(0, 4))]].get(k) for k in keys}
    return log[:n], {k: v for k, v in prior.items() if v is not None}


@pytest.mark.gpu
def test_replay_log(cuda, oracle):
    """The whole log on the device against the sequential replay: the table the final stream
    leaves, where the replay ends and why."""
    import torch

    from k2hash_amd import barrier
    stopped = executed = 0
    for seed in range(6):
        log, prior = _replay_case(seed)
        held, off = _held(oracle, prior)
        d_file = _dev(cuda, am.build_log(log)[0])
        d_held, d_off = (_dev(cuda, held), torch.tensor(off, dtype=torch.int64, device=cuda)) if seed % 3 else (None, None)
        if d_held is None:
            prior = {}
        for err_skip in (False, True):
            want, at, outcome = bm.replay_all(log, prior, err_skip)
            r = barrier.replay_log(d_held, d_off, d_file, fold=bool(seed % 2), err_skip=err_skip)
            assert (r.stopped_at, r.outcome) == (at, outcome), (seed, err_skip)
            got = am.table_of(r.blobs.cpu().numpy().tobytes(), r.blob_off.cpu().numpy())
            assert got == {k: v for k, v in want.items()}, (seed, err_skip)
            assert r.blob_off.numel() - 1 == len(want) and int(r.blob_off[-1]) == r.blobs.numel()     # compact: one blob per key
            stopped += at < len(log)
            executed += r.barriers
    assert stopped >= 6 and executed > 30
    # NEW_EXISTS ends the replay under err_skip too; no barrier at all is apply_log
    log = [fm.letter("set-v", b"a", 0), fm.letter("set-v", b"b", 1), ren(b"a", b"b"), fm.letter("del", b"a", 3)]
    r = barrier.replay_log(None, None, _dev(cuda, am.build_log(log)[0]), err_skip=True)
    assert (r.stopped_at, r.outcome, r.barriers) == (2, NEW_EXISTS, 0)
    assert am.table_of(r.blobs.cpu().numpy().tobytes(), r.blob_off.cpu().numpy()) == {b"a": (b"v0", None, None), b"b": (b"v1", None, None)}
    r = barrier.replay_log(None, None, _dev(cuda, am.build_log(log[:2])[0]))
    assert (r.stopped_at, r.outcome, r.barriers, r.segments) == (2, EXECUTED, 0, 1)


@pytest.mark.gpu
def test_replay_log_save_pattern_and_growth(cuda, oracle):
    """K2HArchive::Save's form of a large value -- SET_ALL with an empty value, then chunks at
    ascending offsets, here 600 of 1,000 bytes: three runs back to back on one arena, which the
    second run outgrows; then a RENAME of the value, and records behind it."""
    from k2hash_amd import barrier
    key, x = b"the-large-value", _pattern(600 * 1000, 77)
    log = [Rec(fm.SET_ALL, b"small", b"s"), Rec(fm.SET_ALL, key, b"", b"subkeys", b"attrs")]
    log += [ow(key, at, x[at:at + 1000]) for at in range(0, len(x), 1000)]
    log += [ren(key, b"its-new-name"), fm.letter("rep-a", b"small", 9), fm.letter("del", key, 10)]
    want, at, outcome = bm.replay_all(log, {})
    assert want == {b"its-new-name": (x, b"subkeys", b"attrs"), b"small": (b"s", None, b"a9")} and at == len(log)
    r = barrier.replay_log(None, None, _dev(cuda, am.build_log(log)[0]))
    assert (r.stopped_at, r.outcome, r.barriers, r.segments) == (len(log), EXECUTED, 4, 2)
    assert am.table_of(r.blobs.cpu().numpy().tobytes(), r.blob_off.cpu().numpy()) == want
