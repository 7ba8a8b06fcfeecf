"""RALLEDATA blobs straight from range records (include/k2hash_amd.h section 4c;
k2hash_amd/csrc/k2h_ralledata_recs.hip): k2h_amd_import_ralledata / k2h_amd_archive_ralledata and
their Python forms.

Expected bytes never come from the code under test: records from the getline restatement
(import_scenarios.ref_scan), tests/golden/import.json and the host archive scan of the golden
archive; blobs from oracle.build_ralledata over Python-sliced byte strings (ralle_recs_model).
Every record of every scenario is compared: out[:total], blob_off and total, byte for byte, the
file between non-zero canaries at shifts 0 / 1 / 15 and `out` between sentinel bytes.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import ralle_recs_model as m
from import_scenarios import PAD, SHIFTS, place

from k2hash_amd import _native

HIPCC = "/opt/rocm/bin/hipcc"
CANARY = 0xA5

IMPORT_CASES = {c.name: c for c in m.import_cases()}
GOLDEN_CASES = {c.name: c for c in m.golden_import_cases()}
_ARCHIVE = {}
_EXPECT = {}


def archive_cases():
    if not _ARCHIVE:
        _ARCHIVE.update({c.name: c for c in m.archive_cases()})
    return _ARCHIVE


ARCHIVE_NAMES = ("golden", "set-all-200", "mixed-200", "no-set-all-200", "forged")


def want(oracle, case, std_fnv=False):
    """The expected stream of a case, computed once."""
    key = (case.kind, case.name, std_fnv)
    if key not in _EXPECT:
        blobs, off = m.expected(oracle, case.data, m.segments_of(case), case.kind == "import", std_fnv)
        blobs.setflags(write=False)
        off.setflags(write=False)
        _EXPECT[key] = (blobs, off)
    return _EXPECT[key]


def run_case(cuda, oracle, case, shift, std_fnv=False):
    blobs, off = want(oracle, case, std_fnv)
    file = place(cuda, case.data, shift, CANARY)
    res = m.run(cuda, case.kind, file, m.recs_words(case), std_fnv=std_fnv, oshift=shift)
    m.check_stream((case.name, shift, std_fnv), res, blobs, off)
    return res


# ---------------------------------------------------------------------------------- CPU
def test_symbols_declared_and_bound():
    header = (m.ROOT / "include" / "k2hash_amd.h").read_text()
    lib = _native.batch_lib()
    for name in ("k2h_amd_import_ralledata", "k2h_amd_archive_ralledata"):
        assert re.search(r"\bint " + name + r"\(const void\* file, uint64_t size,", header), name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == 10, name
        assert hasattr(lib, name), name
    import k2hash_amd
    for name in ("import_to_ralledata", "archive_to_ralledata", "import_file_to_ralledata"):
        assert name in k2hash_amd.__all__ and callable(getattr(k2hash_amd, name)), name


@pytest.mark.parametrize("name", ["k2h_amd_import_ralledata", "k2h_amd_archive_ralledata"])
def test_host_side_answers(name):
    """n == 0 and the argument errors are judged on the host, before any device is needed."""
    fn = getattr(_native.batch_lib(), name)
    one = ctypes.c_void_p(1)
    total = ctypes.c_uint64(0xDEAD)
    assert fn(None, 0, None, 0, None, 0, None, ctypes.byref(total), 0, None) == 0 and total.value == 0
    total = ctypes.c_uint64(0xDEAD)
    assert fn(one, 100, one, 0, None, 0, None, ctypes.byref(total), _native.K2H_AMD_FLAG_STD_FNV, None) == 0
    assert total.value == 0
    assert fn(one, 100, one, 5, None, 0, one, ctypes.byref(total), _native.K2H_AMD_FLAG_CSTR, None) == m.EINVAL
    assert fn(None, 0, None, 0, None, 0, None, ctypes.byref(total), _native.K2H_AMD_FLAG_CSTR, None) == m.EINVAL
    assert fn(one, 100, one, 5, None, 0, one, None, 0, None) == m.EINVAL                       # NULL total
    assert fn(None, 0, None, 0, None, 0, None, None, 0, None) == m.EINVAL
    assert fn(one, 100, one, 5, None, 0, None, ctypes.byref(total), 0, None) == m.EINVAL       # NULL blob_off
    # n * (82 + 4 size) overflows 64 bits: by n, by size, and the largest products either side
    size = 1 << 20
    per = 82 + 4 * size
    assert fn(one, size, one, m.U64 // per + 1, None, 0, one, ctypes.byref(total), 0, None) == m.EINVAL
    assert fn(one, 1 << 62, one, 1, None, 0, one, ctypes.byref(total), 0, None) == m.EINVAL
    assert fn(one, 1 << 40, one, 1 << 30, None, 0, one, ctypes.byref(total), 0, None) == m.EINVAL
    assert b"overflow" in _native.batch_lib().k2h_amd_strerror(m.EINVAL)


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
    out = tmp_path / "k2h_ralledata_recs.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    f"-I{m.ROOT / 'include'}", str(m.SRC_PATH), "-o", str(out)], check=True, capture_output=True)
    meta = {k: v for k, v in _kernel_meta(out.read_text()).items() if "ralledata_recs_" in k}
    build = {k: v for k, v in meta.items() if "ralledata_recs_kernel" in k}
    assert len(build) == 2 and len(meta) == 4, sorted(meta)
    assert any("ImportReader" in k for k in build) and any("ArchiveReader" in k for k in build)
    for sym, f in meta.items():
        assert f["private_segment_fixed_size"] == 0, sym
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, sym
    for sym, f in build.items():
        assert f["vgpr_count"] + f["agpr_count"] <= 512 // m.WAVES, (sym, f["vgpr_count"], f["agpr_count"])
        assert f["group_segment_fixed_size"] <= 160 * 1024 // m.WAVES, (sym, f["group_segment_fixed_size"])
        assert f["group_segment_fixed_size"] < 20 * 1024


def test_model_constants():
    assert m.R == 64 and m.WAVES == 8
    assert m.HULL == m.kRecPool - 32   # first start .. last end plus 15 bytes of alignment either side fits the pool


def _all_cases(oracle):
    d, r = m.random_file(oracle)
    rnd = m.Case("random-50000", "import", d, r, {"staged", "direct"}, "tsv")
    return list(IMPORT_CASES.values()) + list(GOLDEN_CASES.values()) + list(archive_cases().values()) + [rnd]


def test_scenarios_reach_the_forms_they_claim(oracle):
    seen = {"import": set(), "archive": set()}
    for case in _all_cases(oracle):
        ok, got = m.claim_holds(case)
        assert ok, (case.name, case.claim, got)
        seen[case.kind] |= set(got)
    assert seen["import"] == {"staged", "direct", "none"}
    assert seen["archive"] == {"staged", "direct", "none"}
    # the golden files reach both forms as well (the large fuzz files hold long values)
    g = set()
    for case in GOLDEN_CASES.values():
        g |= set(m.forms(m.segments_of(case)))
    assert "staged" in g
    assert len(GOLDEN_CASES) >= 35
    for name in ("eof_tab.tsv", "eof_value.tsv", "edge.tsv", "notab.tsv", "empty.tsv", "fuzz_00300.tsv",
                 "fuzz_00300.mdbm"):
        assert "golden-" + name in GOLDEN_CASES, name
    assert len(GOLDEN_CASES["golden-empty.tsv"].recs) == 0


def test_block_edge_spans_start_aligned_and_not(oracle):
    """Blob sizes vary, so the blocks' output spans start at every alignment: over the block-edge
    scenarios at least one span starts 16-aligned and one does not; over all import scenarios
    every combination of an aligned / unaligned start and end occurs."""
    starts, both = set(), set()
    for case in IMPORT_CASES.values():
        _, off = want(oracle, case)
        n = len(case.recs)
        for b in range(0, n, m.R):
            s, e = int(off[b]) % 16 == 0, int(off[min(b + m.R, n)]) % 16 == 0
            if off[b] != off[min(b + m.R, n)]:
                both.add((s, e))
                if case.name.startswith("edge-"):
                    starts.add(s)
    assert starts == {True, False}
    assert both == {(True, True), (True, False), (False, True), (False, False)}, both


def test_lengths_scenario_terminators(oracle):
    """The expected stream itself: key_length = strlen + 1 and a 0x00 where the file holds a TAB."""
    from k2hash_amd.ralledata import parse_blob
    case = IMPORT_CASES["lengths"]
    blobs, off = want(oracle, case)
    raw = blobs.tobytes()
    for i, (ko, kl, vo, vl) in enumerate(case.recs.tolist()):
        b = parse_blob(raw[int(off[i]):int(off[i + 1])])
        assert b.key == case.data[ko:ko + kl] + b"\0" and b.val == case.data[vo:vo + vl] + b"\0"
        assert int(off[i + 1] - off[i]) == 82 + kl + vl
    assert {len(parse_blob(raw[int(off[i]):int(off[i + 1])]).key) for i in range(len(case.recs))} >= \
        {1, 2, 15, 16, 17, 18, 32, 33, 255}


# ---------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_golden_import_files(cuda, oracle, name):
    """Through import_file_to_ralledata (device scan, then the builder), and the C ABI between
    sentinels over the golden records."""
    import k2hash_amd
    case = GOLDEN_CASES[name]
    idx = sorted(GOLDEN_CASES).index(name)
    for std_fnv in (False, True) if "fuzz_00300" in name else (False,):
        blobs, off = want(oracle, case, std_fnv)
        shift = SHIFTS[(idx + std_fnv) % 3]
        file = place(cuda, case.data, shift, CANARY)
        got, got_off = k2hash_amd.import_file_to_ralledata(file, case.fmt, std_fnv=std_fnv)
        assert got_off.cpu().numpy().view(np.uint64).tolist() == off.tolist(), name
        assert got.numel() == blobs.size and np.array_equal(got.cpu().numpy(), blobs), name
        run_case(cuda, oracle, case, SHIFTS[(idx + 1 + std_fnv) % 3], std_fnv)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", m.BLOCK_EDGE_N)
def test_block_edges(cuda, oracle, n, shift):
    run_case(cuda, oracle, IMPORT_CASES[f"edge-n{n}"], shift)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("name", ["lengths", "lengths-reversed"])
def test_key_and_value_lengths(cuda, oracle, name, shift):
    """Staged and (reversed) direct: the last value ends at the file's last byte, the byte after it
    is the non-zero canary, so a copied terminator shows."""
    run_case(cuda, oracle, IMPORT_CASES[name], shift)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["direct-one-20k-value", "direct-mdbm-key-line-at-eof", "direct-reversed",
                                  "direct-duplicate-5", "alternate-staged-direct"])
def test_direct_form(cuda, oracle, name):
    for shift in SHIFTS:
        run_case(cuda, oracle, IMPORT_CASES[name], shift)


@pytest.mark.gpu
def test_skips_and_hostile_ranges(cuda, oracle):
    """Every overshoot stays inside the file's own padded allocation, so a missing guard shows as
    a wrong byte, never as a fault."""
    case = IMPORT_CASES["skips"]
    size = len(case.data)
    for ko, kl, vo, vl in case.recs.tolist():
        for o, n in ((ko, kl), (vo, vl)):
            assert m.inside(o, n, size) or o + n <= size + PAD or o >= m.U64 - PAD
    segs = m.segments_of(case)
    assert [s is None for s in segs].count(True) == 1 + 1 + 64 + 1 and segs[10] == [tuple(case.recs[10][:2]), (size, 0)]
    for shift in SHIFTS:
        res = run_case(cuda, oracle, case, shift)
        assert (np.diff(res["off"].astype(np.int64)) == 0).sum() == 67


@pytest.mark.gpu
def test_capacity(cuda, oracle):
    case = IMPORT_CASES[f"edge-n{m.R + 1}"]
    blobs, off = want(oracle, case)
    total = int(off[-1])
    file = place(cuda, case.data, 1, CANARY)
    res = m.run(cuda, "import", file, m.recs_words(case), cap="none")      # out = NULL: sizes only
    assert res["rc0"] == 0 and res["total0"] == total and np.array_equal(res["off0"], off)
    res = m.run(cuda, "import", file, m.recs_words(case), cap=total - 1)
    assert res["rc"] == m.EINVAL and res["total"] == total and np.array_equal(res["off"], off)
    assert (res["out"] == m.OUT_FILL).all() and (res["before"] == m.OUT_FILL).all() and (res["after"] == m.OUT_FILL).all()
    res = m.run(cuda, "import", file, m.recs_words(case), cap=total)
    m.check_stream("cap = total", res, blobs, off)
    res = m.run(cuda, "import", file, m.recs_words(case), cap=total + 100)
    m.check_stream("cap = total + 100", res, blobs, off)


@pytest.mark.gpu
def test_no_records_on_the_device(cuda):
    import torch
    lib = _native.batch_lib()
    off = torch.full((4,), m.OFF_FILL, dtype=torch.int64, device=cuda)
    total = ctypes.c_uint64(0xDEAD)
    for fn in (lib.k2h_amd_import_ralledata, lib.k2h_amd_archive_ralledata):
        off.fill_(m.OFF_FILL)
        assert fn(None, 0, None, 0, None, 0, ctypes.c_void_p(off.data_ptr()), ctypes.byref(total), 0, None) == 0
        torch.cuda.synchronize()
        assert total.value == 0 and off.cpu().tolist() == [0] + [m.OFF_FILL] * 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ARCHIVE_NAMES)
def test_archive(cuda, oracle, name):
    import k2hash_amd
    from k2hash_amd import archive
    case = archive_cases()[name]
    segs = m.segments_of(case)
    if name == "golden":
        assert len(segs) == 64 and sum(s is not None for s in segs) == 10
    if name == "no-set-all-200":
        assert int(want(oracle, case)[1][-1]) == 0
    if name == "forged":
        assert [s is not None for s in segs] == [True, False, True, False, True, False]
    for shift in SHIFTS:
        run_case(cuda, oracle, case, shift)
    if name == "golden":
        run_case(cuda, oracle, case, 1, std_fnv=True)
    # the Python form over the device scan's records
    blobs, off = want(oracle, case)
    file = place(cuda, case.data, 15, CANARY)
    recs = archive.scan_device(file)
    assert np.array_equal(archive.recs_to_numpy(recs), case.recs)
    got, got_off = k2hash_amd.archive_to_ralledata(file, recs)
    assert got_off.cpu().numpy().view(np.uint64).tolist() == off.tolist()
    assert np.array_equal(got.cpu().numpy(), blobs)


@pytest.mark.gpu
def test_round_trip_through_check(cuda, oracle):
    """An extra, not the pin: the consumer side accepts what the producer wrote -- OK for every
    blob, BAD_SPAN for every 0-byte one."""
    import torch

    import k2hash_amd
    from k2hash_amd import ralledata
    for case in (IMPORT_CASES[f"edge-n{2 * m.R + 1}"], IMPORT_CASES["skips"]):
        file = place(cuda, case.data, 1, CANARY)
        recs = torch.from_numpy(m.recs_words(case)).to(cuda)
        blobs, off = k2hash_amd.import_to_ralledata(file, recs)
        st = ralledata.check_ralledata(blobs, off).status.cpu().numpy()
        empty = np.diff(off.cpu().numpy()) == 0
        assert (st[~empty] == ralledata.OK).all() and (st[empty] == ralledata.BAD_SPAN).all()
        assert empty.sum() == (67 if case.name == "skips" else 0)


@pytest.mark.gpu
def test_random_50000(cuda, oracle):
    import torch

    import k2hash_amd
    data, recs = m.random_file(oracle)
    case = m.Case("random-50000", "import", data, recs, None, "tsv")
    blobs, off = want(oracle, case)
    file = place(cuda, data, 1, CANARY)
    got, got_off = k2hash_amd.import_to_ralledata(file, torch.from_numpy(m.recs_words(case)).to(cuda))
    assert np.array_equal(got_off.cpu().numpy().view(np.uint64), off)
    g = got.cpu().numpy()
    bad = np.flatnonzero(g != blobs)
    assert bad.size == 0, (bad.size, int(bad[0]), int(np.searchsorted(off, bad[0], side="right") - 1))
