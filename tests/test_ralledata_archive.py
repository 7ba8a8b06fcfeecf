"""A RALLEDATA stream written as a k2hash archive (include/k2hash_amd.h section 4d:
k2h_amd_ralledata_archive; k2hash_amd/csrc/k2h_ralledata_archive.hip) and its Python forms.

Expected bytes never come from the code under test: they come from ralle_archive_model.scom_set_all,
a struct.pack restatement of the SCOM_SET_ALL record that the first test pins to the ten records the
reference's own K2HCommandArchive wrote into tests/golden/archive.k2har.  Blobs come from
oracle.build_ralledata or are forged by hand.  Every comparison is byte for byte: out[:total],
rec_off, records and total, the stream between canaries and `out` and rec_off between sentinels.
"""
import ctypes
import json
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN

import ralle_archive_model as m
import ralle_check_model as rm
import ralle_recs_model as rr

from k2hash_amd import _native, archive, ralledata

HIPCC = "/opt/rocm/bin/hipcc"
B = m.B
SHIFTS = (0, 1, 15)
_CACHE = {}


def cached(name, fn, *args):
    if name not in _CACHE:
        _CACHE[name] = fn(*args)
    return _CACHE[name]


def golden_archive():
    """(file bytes, host-scan records, the 64 records' bytes, which of them are SET_ALL)."""
    f = (GOLDEN / "archive.k2har").read_bytes()
    recs = archive.scan(f)                 # the host scan, pinned to archive.json by test_archive.py
    ends = [int(r["offset"]) for r in recs[1:]] + [len(f)]
    parts = [f[int(r["offset"]):e] for r, e in zip(recs, ends)]
    return f, recs, parts, [int(r["type"]) == 0 and int(r["status"]) == 0 for r in recs]


def rec_segments(f, r):
    return [f[int(r[o]):int(r[o]) + int(r[n])] for o, n in (("key_off", "key_len"), ("val_off", "val_len"),
                                                             ("skey_off", "skey_len"), ("attrs_off", "attrs_len"))]


# ------------------------------------------------------------------------------ scenarios
def flip_hashes(blobs, every=3):
    """Wrong hash and subhash fields in every `every`-th blob: the writer must not care."""
    for b in blobs[::every]:
        if len(b) >= rm.HEADER:
            rm.put(b, 0, rm.F_HASH, rm.get(b, 0, rm.F_HASH) ^ (1 << 40))
            rm.put(b, 0, rm.F_SUBHASH, rm.get(b, 0, rm.F_SUBHASH) ^ 1)
    return blobs


EDGE_N = (1, B - 1, B, B + 1, 2 * B + 1)
EDGE_KEYS = (1, 15, 16, 17)


def edge_stream(oracle, n):
    """n blobs: key lengths 1, 15, 16, 17 in turn; value, subkeys and attrs empty or not in all
    eight combinations (all three empty: a key-only blob)."""
    rng = m._rng(1, n)
    ks = [m.rbytes(rng, EDGE_KEYS[i % 4]) for i in range(n)]
    combo = [(i // 4) % 8 if n > 1 else 5 for i in range(n)]
    vs = [m.rbytes(rng, 1 + i % 37) if c & 1 else b"" for i, c in enumerate(combo)]
    ss = [m.rbytes(rng, 1 + i % 19) if c & 2 else b"" for i, c in enumerate(combo)]
    as_ = [m.rbytes(rng, 1 + i % 23) if c & 4 else b"" for i, c in enumerate(combo)]
    blobs = flip_hashes(m.blobs_of(oracle, ks, vs, ss, as_))
    if n >= B:
        assert {(len(k), c) for k, c in zip(ks, combo)} >= {(kl, c) for kl in EDGE_KEYS for c in range(8)}
    return rm.join(blobs, lead=b"edge!")


def ordinary(oracle, rng, n, p_extra=0.3):
    return m.blobs_of(oracle, *m.records(rng, n, p_extra=p_extra))


def no_key(rng):
    return m.forge(b"", m.rbytes(rng, 9))


def empty():
    return m.forge(b"")


def hostile_stream(oracle):
    """Four blocks: 0 staged (slack, garbage positions of empty segments, every kind of header the
    writer refuses, a short blob), 1 direct once its headers are seen (permuted and overlapping
    segments), 2 none (a whole block of non-participants), 3 direct by its offsets (one steps back;
    the last blob ends past size).
    Returns (buf, off, size, claim, {name: blob index})."""
    rng = m._rng(2)
    at = {}
    blk0 = ordinary(oracle, rng, B)
    at["slack"] = 3
    blk0[3] = m.forge(m.rbytes(rng, 7), m.rbytes(rng, 20), slack=13)
    at["garbage-pos"] = 5
    blk0[5] = m.forge(m.rbytes(rng, 9), b"", b"", m.rbytes(rng, 5))
    rm.put(blk0[5], 0, rm.F_VPOS, 0xDEADBEEFDEADBEEF)     # negative as an off_t, length 0
    rm.put(blk0[5], 0, rm.F_SPOS, 3)                      # below the header, length 0
    at["empty"], at["no-key"] = 7, 8
    blk0[7], blk0[8] = empty(), no_key(rng)
    at["pos<80"] = 10
    blk0[10] = m.forge(m.rbytes(rng, 6), m.rbytes(rng, 6))
    rm.put(blk0[10], 0, rm.F_KPOS, 79)
    at["end-past-blob"] = 11
    blk0[11] = m.forge(m.rbytes(rng, 6), m.rbytes(rng, 6))
    rm.put(blk0[11], 0, rm.F_VPOS, len(blk0[11]) + 1 - 6)
    at["wrap"] = 12
    blk0[12] = m.forge(m.rbytes(rng, 6), m.rbytes(rng, 6))
    rm.put(blk0[12], 0, rm.F_VPOS, m.U64 - 3)             # pos + len wraps to 3; pos is negative too
    at["wrap-len"] = 13
    blk0[13] = m.forge(m.rbytes(rng, 6), m.rbytes(rng, 6))
    rm.put(blk0[13], 0, rm.F_VLEN, m.U64 - 80)            # pos + len wraps, pos itself in range
    at["short"] = 14
    blk0[14] = bytearray(b"\x01" * 79)
    at["key-only"] = 15
    blk0[15] = m.forge(m.rbytes(rng, 33))
    blk1 = ordinary(oracle, rng, B)
    at["permuted"] = B + 4
    blk1[4] = m.forge(m.rbytes(rng, 17), m.rbytes(rng, 30), m.rbytes(rng, 8), m.rbytes(rng, 12), order=(3, 1, 0, 2),
                      gaps=(0, 2, 0, 5), slack=3)
    at["overlap"] = B + 9
    blk1[9] = m.forge(m.rbytes(rng, 24), m.rbytes(rng, 40))
    rm.put(blk1[9], 0, rm.F_VPOS, rm.HEADER + 10)         # the value starts inside the key
    blk2 = [empty() if i % 2 else no_key(rng) for i in range(B)]
    blk3 = ordinary(oracle, rng, B - 5)
    blobs = flip_hashes(blk0 + blk1 + blk2 + blk3, every=4)
    buf, off = rm.join(blobs, lead=b"abc")
    at["steps-back"] = 3 * B + 6
    off[3 * B + 7] = off[3 * B + 5]        # blob 3B+6 decreases; 3B+7 is blob 3B+5 again, the next two as its slack
    at["past-size"] = len(off) - 2
    return buf, off, off[-1] - 10, ["staged", "direct-late", "none", "direct"], at


def keep_masks(n):
    every_other = (np.arange(n) % 2).astype(np.uint8)
    first, last = np.ones(n, np.uint8), np.ones(n, np.uint8)
    first[0] = last[-1] = 0
    return {"all": None, "not-first": first, "not-last": last, "every-other": every_other}


BIG_VALUE = 64 << 10


def large_stream(oracle):
    """Four blocks of B blobs; blocks 1 and 3 hold one 64 KiB value in their middle."""
    rng = m._rng(3)
    ks, vs, ss, as_ = m.records(rng, 4 * B, p_extra=0.3)
    for blk in (1, 3):
        vs[blk * B + B // 2] = m.rbytes(rng, BIG_VALUE)
    return rm.join(m.blobs_of(oracle, ks, vs, ss, as_)) + (["staged", "direct", "staged", "direct"],)


RANDOM_N = 20000


def random_stream(oracle):
    rng = m._rng(4)
    ks, vs, ss, as_ = m.records(rng, RANDOM_N, klen=(1, 301), vlen=(0, 261), p_extra=1 / 3, slen=(1, 65),
                                alen=(1, 49))
    return rm.join(flip_hashes(m.blobs_of(oracle, ks, vs, ss, as_), every=5), lead=b"x" * 7)


# ---------------------------------------------------------------------------------- CPU
def test_model_is_pinned_to_the_reference():
    """scom_set_all of each SET_ALL record's four segments is that record's bytes in the file the
    reference's K2HCommandArchive wrote."""
    f, recs, parts, is_set = golden_archive()
    assert len(parts) == 64 and sum(is_set) == 10
    seen = set()
    for r, p, s in zip(recs, parts, is_set):
        if s:
            segs = rec_segments(f, r)
            assert m.scom_set_all(*segs) == p, int(r["offset"])
            assert int(r["exdata_len"]) == 0 and len(p) == m.SCOM + sum(len(x) for x in segs)
            seen.add(tuple(bool(x) for x in segs))
    assert len(seen) >= 2 and all(k[0] for k in seen)      # the fixture has records with and without a value


def test_symbol_declared_bound_and_exported():
    import inspect

    import k2hash_amd
    header = (m.ROOT / "include" / "k2hash_amd.h").read_text()
    assert re.search(r"\bint k2h_amd_ralledata_archive\(const void\* blobs, uint64_t size,", header)
    assert re.search(r"#define K2H_AMD_SCOM_HEADER 104\b", header)
    assert len(_native.SIGNATURES["k2h_amd_ralledata_archive"][1]) == 11
    assert hasattr(_native.batch_lib(), "k2h_amd_ralledata_archive")
    assert _native.K2H_AMD_SCOM_HEADER == m.SCOM == ralledata.SCOM_HEADER
    for name in ("ralledata_to_archive", "import_file_to_archive"):
        assert name in k2hash_amd.__all__ and callable(getattr(k2hash_amd, name)), name
    assert ralledata.Archived._fields == ("bytes", "rec_off", "records", "total")
    assert list(inspect.signature(ralledata.ralledata_to_archive).parameters) == [
        "blobs", "blob_off", "keep", "out", "count_only", "stream"]
    assert list(inspect.signature(ralledata.import_file_to_archive).parameters) == ["file", "fmt", "stream"]
    assert "k2h_ralledata_archive.hip" in (m.ROOT / "k2hash_amd" / "csrc" / "Makefile").read_text()


def test_host_side_answers():
    """n == 0, each NULL argument and the overflow are judged on the host, with a NULL stream and
    before any device is needed; each error has its own message."""
    lib = _native.batch_lib()
    fn = lib.k2h_amd_ralledata_archive
    one = ctypes.c_void_p(1)
    msg = lambda: bytes(lib.k2h_amd_strerror(m.EINVAL))  # noqa: E731
    total, recs = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
    tp, rp = ctypes.byref(total), ctypes.byref(recs)
    # n == 0 without rec_off: answered with no device work at all
    assert fn(None, 0, None, 0, None, None, 0, None, rp, tp, None) == m.OK and (total.value, recs.value) == (0, 0)
    total.value = recs.value = 0xDEAD
    assert fn(one, 100, one, 0, one, one, 50, None, None, tp, None) == m.OK and total.value == 0
    assert recs.value == 0xDEAD
    texts = set()
    cases = {
        "NULL total": (one, 100, one, 5, None, None, 0, one, rp, None, None),
        "NULL rec_off": (one, 100, one, 5, None, None, 0, None, rp, tp, None),
        "NULL blobs": (None, 100, one, 5, None, None, 0, one, rp, tp, None),
        "NULL blob_off": (one, 100, None, 5, None, None, 0, one, rp, tp, None),
    }
    for needle, args in cases.items():
        total.value = recs.value = 0xDEAD
        assert fn(*args) == m.EINVAL, needle
        assert needle.encode() in msg() and msg().startswith(b"ralledata_archive: "), (needle, msg())
        assert needle == "NULL total" or (total.value, recs.value) == (0, 0)
        texts.add(msg())
    assert fn(None, 0, None, 0, None, None, 0, None, None, None, None) == m.EINVAL and b"NULL total" in msg()
    # n * (104 + 4 size) overflows 64 bits: by n, by size, and either side of the largest product
    size = 1 << 20
    per = m.SCOM + 4 * size
    over = (one, size, one, (m.U64 - 1) // per + 1, None, None, 0, one, rp, tp, None)
    assert fn(*over) == m.EINVAL and b"overflow" in msg()
    texts.add(msg())
    assert len(texts) == 5
    assert fn(one, 1 << 62, one, 1, None, None, 0, one, rp, tp, None) == m.EINVAL and b"overflow" in msg()
    assert fn(one, (m.U64 - 1 - m.SCOM) // 4 + 1, one, 1, None, None, 0, one, rp, tp, None) == m.EINVAL
    assert b"overflow" in msg()
    assert fn(one, 1 << 40, one, 1 << 30, None, None, 0, one, rp, tp, None) == m.EINVAL and b"overflow" in msg()
    # the largest product that fits passes the host's judgement: on a machine without a device the
    # call then stops at the device gate, with another code; with one it would run, so it is only
    # made where there is none
    import torch
    if not torch.cuda.is_available():
        fits = (one, size, one, (m.U64 - 1) // per, None, None, 0, one, rp, tp, None)
        assert fn(*fits) not in (m.OK, m.EINVAL)


def _kernel_meta(asm):
    meta = {}
    for block in re.split(r"\n\s*- \.agpr_count:", asm)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", "\n.agpr_count:" + block,
                                                                   flags=re.M)}
    return meta


def test_kernels_fit_their_budget(tmp_path):
    """No scratch, no spills, and the registers and LDS of the occupancy the build kernel declares
    (amdgpu_waves_per_eu: 512 VGPRs per SIMD lane; a block is four waves, one per SIMD, so
    waves_per_eu blocks share a CU's 160 KiB of LDS)."""
    if not m.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "k2h_ralledata_archive.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    f"-I{m.ROOT / 'include'}", str(m.SRC_PATH), "-o", str(out)], check=True, capture_output=True)
    meta = {k: v for k, v in _kernel_meta(out.read_text()).items() if "scom_archive_" in k}
    assert len(meta) == 2 and all(any(k in sym for sym in meta) for k in m.KERNELS), sorted(meta)
    assert not any("ralledata_recs_" in k for k in meta)
    for sym, f in meta.items():
        assert f["private_segment_fixed_size"] == 0, sym
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, sym
        assert f["vgpr_count"] + f["agpr_count"] <= 512 // m.WAVES, (sym, f["vgpr_count"], f["agpr_count"])
    build = [f for sym, f in meta.items() if m.BUILD_KERNEL in sym]
    assert len(build) == 1 and build[0]["group_segment_fixed_size"] <= 160 * 1024 // m.WAVES


def test_scenarios_reach_the_forms_they_claim(oracle):
    assert m.HULL == m.kArcPool - 32 and 8 * B == 256 and BIG_VALUE > m.kArcPool
    for n in EDGE_N:
        buf, off = cached(("edge", n), edge_stream, oracle, n)
        assert m.forms(m.stream_segments(buf, off), off) == ["staged"] * -(-n // B), n
    buf, off, size, claim, at = cached("hostile", hostile_stream, oracle)
    for name, keep in keep_masks(len(off) - 1).items():
        got = m.forms(m.stream_segments(buf, off, size, keep), off)
        assert got == claim, (name, got)
    segs = m.stream_segments(buf, off, size)
    for name in ("slack", "garbage-pos", "key-only", "permuted", "overlap"):
        assert segs[at[name]] is not None, name
    for name in ("empty", "no-key", "pos<80", "end-past-blob", "wrap", "wrap-len", "short", "steps-back", "past-size"):
        assert segs[at[name]] is None, name
    statuses = {name: rm.header_status(bytes(buf), off[i], off[i + 1], size)[0] for name, i in at.items()}
    assert statuses["empty"] == rm.EMPTY and statuses["no-key"] == rm.NO_KEY
    assert {statuses[k] for k in ("pos<80", "end-past-blob", "wrap", "wrap-len")} == {rm.BAD_RANGE}
    assert {statuses[k] for k in ("short", "steps-back", "past-size")} == {rm.BAD_SPAN}
    (k0, kl), (v0, vl) = segs[at["overlap"]][:2]
    assert k0 < v0 < k0 + kl                               # two segments overlap
    buf, off, claim = cached("large", large_stream, oracle)
    assert m.forms(m.stream_segments(buf, off), off) == claim
    buf, off = cached("random", random_stream, oracle)
    got = m.forms(m.stream_segments(buf, off), off)
    assert set(got) <= {"staged", "direct"} and got.count("staged") > got.count("direct")


# ---------------------------------------------------------------------------------- GPU
def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def walk(data, want_segs):
    """The host archive scan over an output: as many records as participants, status 0, type 0,
    the expected lengths."""
    recs = archive.scan(bytes(data))
    kept = [s for s in want_segs if s is not None]
    assert len(recs) == len(kept)
    assert not recs["status"].any() and not recs["type"].any() and not recs["exdata_len"].any()
    for name, j in (("key_len", 0), ("val_len", 1), ("skey_len", 2), ("attrs_len", 3)):
        assert recs[name].tolist() == [s[j][1] for s in kept], name
    return recs


@pytest.mark.gpu
def test_golden_round_trip(cuda):
    """archive.k2har on the device -> scan_device -> archive_to_ralledata -> the writer: the ten
    reference-written SET_ALL records, in file order; the 54 other records (0-byte blobs) yield
    0 bytes.  Then 200 records drawn from the fixture."""
    import torch
    f, recs, parts, is_set = golden_archive()
    cases = [("golden", f, recs, parts, is_set)]
    for c in rr.archive_cases():
        if c.name in ("mixed-200", "set-all-200"):
            ends = [int(r["offset"]) for r in c.recs[1:]] + [len(c.data)]
            cases.append((c.name, c.data, c.recs, [c.data[int(r["offset"]):e] for r, e in zip(c.recs, ends)],
                          [int(r["type"]) == 0 and int(r["status"]) == 0 for r in c.recs]))
    for k, (name, data, hrecs, rparts, rset) in enumerate(cases):
        want = b"".join(p for p, s in zip(rparts, rset) if s)
        want_off = np.concatenate([[0], np.cumsum([len(p) if s else 0 for p, s in zip(rparts, rset)])]).astype(np.uint64)
        file = m.place(cuda, data, SHIFTS[k])
        drecs = archive.scan_device(file)
        blobs, boff = ralledata.archive_to_ralledata(file, drecs)
        torch.cuda.synchronize()
        h_off = boff.cpu().numpy()
        assert [(h_off[i + 1] > h_off[i]) for i in range(len(rset))] == rset, name
        res = m.run(cuda, blobs, blobs.numel(), h_off, oshift=SHIFTS[(k + 1) % 3])
        m.check(name, res, (np.frombuffer(want, np.uint8), want_off, sum(rset)))
        out = res["out"][:len(want)]
        scanned = archive.scan(out.tobytes())
        assert len(scanned) == sum(rset) and not scanned["status"].any() and not scanned["type"].any()
        sets = [r for r, s in zip(hrecs, rset) if s]
        for fld in ("key_len", "val_len", "skey_len", "attrs_len", "exdata_len"):
            assert scanned[fld].tolist() == [int(r[fld]) for r in sets], (name, fld)
        if name == "golden":
            assert res["records"] == 10 and len(rset) == 64


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGE_N)
def test_block_edges_and_lengths(cuda, oracle, n):
    buf, off = cached(("edge", n), edge_stream, oracle, n)
    for shift in SHIFTS:
        want, _ = m.against_model(cuda, buf, off, ("edge", n, shift), shift=shift, oshift=shift,
                                  claim=["staged"] * -(-n // B))
        assert want[2] == n
    walk(want[0], want[3])


@pytest.mark.gpu
@pytest.mark.parametrize("mask", ["all", "not-first", "not-last", "every-other"])
def test_hostile_and_non_canonical_blobs(cuda, oracle, mask):
    """Every overshoot the forged headers ask for stays inside the stream's own padded allocation,
    so a missing guard shows as a wrong byte, never as a fault."""
    buf, off, size, claim, at = cached("hostile", hostile_stream, oracle)
    keep = keep_masks(len(off) - 1)[mask]
    shift = SHIFTS[sorted(keep_masks(4)).index(mask) % 3]
    want, _ = m.against_model(cuda, buf, off, ("hostile", mask), size=size, keep=keep, shift=shift, oshift=15 - shift,
                              claim=claim)
    n = len(off) - 1
    assert 0 < want[2] < n and int(want[1][3 * B]) == int(want[1][2 * B])    # block 2 yields nothing
    walk(want[0], want[3])
    if mask == "all":
        # without a records pointer: the same bytes
        res = m.run(cuda, m.place(cuda, buf, 1), size, off, want_records=False)
        m.check("hostile, records NULL", res, want)


@pytest.mark.gpu
def test_one_large_value(cuda, oracle):
    buf, off, claim = cached("large", large_stream, oracle)
    for shift in (0, 15):
        want, _ = m.against_model(cuda, buf, off, ("large", shift), shift=shift, oshift=1, claim=claim)
    assert want[2] == 4 * B and int(want[1][-1]) > 2 * BIG_VALUE


@pytest.mark.gpu
def test_alignment_and_containment(cuda, oracle):
    buf, off = cached(("edge", B + 1), edge_stream, oracle, B + 1)
    want = m.model(buf, off)
    total = int(want[1][-1])
    for shift in SHIFTS:
        blobs = m.place(cuda, buf, shift)
        for oshift in SHIFTS:
            m.check(("align", shift, oshift), m.run(cuda, blobs, len(buf), off, oshift=oshift), want)
    res = m.run(cuda, blobs, len(buf), off, cap="none")                    # out = NULL: sizes and counts only
    assert (res["rc0"], res["total0"], res["records0"]) == (0, total, B + 1) and np.array_equal(res["off0"], want[1])
    res = m.run(cuda, blobs, len(buf), off, cap=total - 1)
    assert res["rc"] == m.EINVAL and (res["total"], res["records"]) == (total, B + 1)
    assert np.array_equal(res["off"], want[1])
    assert b"out_cap" in _native.batch_lib().k2h_amd_strerror(m.EINVAL)
    assert (res["out"] == m.OUT_FILL).all() and (res["before"] == m.OUT_FILL).all() and (res["after"] == m.OUT_FILL).all()
    m.check("cap = total + 100", m.run(cuda, blobs, len(buf), off, cap=total + 100, oshift=1), want)


@pytest.mark.gpu
def test_no_blobs_on_the_device(cuda):
    import torch
    fn = _native.batch_lib().k2h_amd_ralledata_archive
    off = torch.full((4,), m.OFF_FILL, dtype=torch.int64, device=cuda)
    total, recs = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
    assert fn(None, 0, None, 0, None, None, 0, ctypes.c_void_p(off.data_ptr()), ctypes.byref(recs),
              ctypes.byref(total), None) == 0
    torch.cuda.synchronize()
    assert (total.value, recs.value) == (0, 0) and off.cpu().tolist() == [0] + [m.OFF_FILL] * 3


@pytest.mark.gpu
def test_random_stream(cuda, oracle):
    buf, off = cached("random", random_stream, oracle)
    want, forms = m.against_model(cuda, buf, off, "random", shift=7, oshift=9)
    assert want[2] == RANDOM_N and "staged" in forms
    walk(want[0], want[3])


@pytest.mark.gpu
def test_python_forms(cuda, oracle):
    import torch
    buf, off = cached(("edge", 2 * B + 1), edge_stream, oracle, 2 * B + 1)
    n = len(off) - 1
    t, d_off = m.place(cuda, buf, 3), _dev(cuda, np.array(off, np.int64))
    want = m.model(buf, off)
    res = ralledata.ralledata_to_archive(t, d_off)
    torch.cuda.synchronize()
    assert (res.records, res.total) == (want[2], int(want[1][-1]))
    assert np.array_equal(res.bytes.cpu().numpy(), want[0])
    assert np.array_equal(res.rec_off.cpu().numpy().view(np.uint64), want[1])
    cnt = ralledata.ralledata_to_archive(t, d_off, count_only=True)
    assert cnt.bytes is None and (cnt.records, cnt.total) == (res.records, res.total)
    assert np.array_equal(cnt.rec_off.cpu().numpy().view(np.uint64), want[1])
    keep = np.arange(n) % 3 != 0
    wk = m.model(buf, off, keep=keep)
    out = torch.full((int(wk[1][-1]) + 32,), m.OUT_FILL, dtype=torch.uint8, device=cuda)
    rk = ralledata.ralledata_to_archive(t, d_off, keep=_dev(cuda, keep), out=out)     # a bool keep, a roomy out
    torch.cuda.synchronize()
    assert rk.records == wk[2] and np.array_equal(rk.bytes.cpu().numpy(), wk[0])
    assert bool((out[rk.total:] == m.OUT_FILL).all())
    small = torch.full((rk.total - 1,), m.OUT_FILL, dtype=torch.uint8, device=cuda)
    with pytest.raises(_native.NativeError, match="out_cap"):
        ralledata.ralledata_to_archive(t, d_off, keep=_dev(cuda, keep), out=small)
    assert bool((small == m.OUT_FILL).all())
    with pytest.raises(ValueError, match="keep needs"):
        ralledata.ralledata_to_archive(t, d_off, keep=_dev(cuda, keep[:-1]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fmt", [("basic.tsv", "tsv"), ("good.mdbm", "mdbm")])
def test_import_file_to_archive(cuda, name, fmt):
    """Every line becomes the SET_ALL record of key + NUL and value + NUL; the strings are the
    ones the reference's own loops printed into import.json."""
    import torch
    g = json.loads((GOLDEN / "import.json").read_text())["inputs"][name]
    assert not g["error"] and g["format"] == fmt and g["records"]
    file = m.place(cuda, (GOLDEN / "import" / name).read_bytes(), 1)
    res = ralledata.import_file_to_archive(file, fmt)
    torch.cuda.synchronize()
    want = b"".join(m.scom_set_all(bytes.fromhex(x["key"]) + b"\0", bytes.fromhex(x["val"]) + b"\0") for x in g["records"])
    assert res.records == len(g["records"]) and res.total == len(want)
    assert res.bytes.cpu().numpy().tobytes() == want


@pytest.mark.gpu
def test_compaction_pipeline(cuda, oracle):
    """A stream with repeated keys: dedup, write the survivors as an archive, scan it, turn it
    back into blobs: the result is select_ralledata of the deduplicated stream."""
    import torch
    rng = m._rng(9)
    ks, vs, _s, _a = m.records(rng, 150)
    pick = rng.integers(0, 150, 400)
    vals = [m.rbytes(rng, rng.integers(0, 60)) for _ in pick]
    buf, off = rm.join(m.blobs_of(oracle, [ks[i] for i in pick], vals))
    t, d_off = m.place(cuda, buf, 5), _dev(cuda, np.array(off, np.int64))
    keep, _by, dropped = ralledata.dedup_ralledata(t, d_off)
    assert 200 < dropped < 400
    arc = ralledata.ralledata_to_archive(t, d_off, keep=keep)
    assert arc.records == 400 - dropped
    recs = archive.scan_device(arc.bytes)
    blobs, boff = ralledata.archive_to_ralledata(arc.bytes, recs)
    sel = ralledata.select_ralledata(t, d_off, keep)
    torch.cuda.synchronize()
    assert recs.shape[0] == arc.records == sel.kept
    assert torch.equal(blobs, sel.blobs) and torch.equal(boff, sel.blob_off)
