"""The device import scan (k2h_import_dev.hip: tsv_a_kernel, tsv_scan_kernel, tsv_b_kernel) at the
spans, slots, units and EOF states it branches on, every record and every hash of every case
against an independent reference.

The scenarios (import_scenarios.py) are built from the kernel's constants as its source states
them, one builder per row of the matrix in DESIGN.md 5.5.  The reference for the records is
ref_scan, a restatement of k2himport's two std::getline loops with bytes.find; for the hashes the
oracle's k2h_hash / k2h_second_hash of key + NUL.  Neither is a result of the library: the host
scanner and the host prehash are themselves checked against them here.

CPU part (no GPU): ref_scan against the recorded output of the reference tool
(tests/golden/import.json), the host scanner against ref_scan on every scenario, each scenario's
claims against span_model (a scenario that does not reach the path it names fails here), and the
union of the claims against the list of paths the matrix has to reach.

GPU part: every scenario through check() -- count exact, the rows below min(count, cap) equal to
ref_scan field by field, h1 / h2 equal to the oracle, every row at or past the bound still the
sentinel, the return code K2H_AMD_EINVAL exactly for count > cap and for a bad mdbm header -- on
the arms, allocation shifts and canary bytes of import_scenarios.matrix().  The canaries are TAB,
newline, NUL and 0xA5: bytes outside the file that are themselves events show a scanner that reads
one byte too far.

What these tests cannot see: a speculative key that falls back to the file gives the same hash as
one taken from pass A's state.  A mistake that only turns hits into misses is a matter of speed
(bench.py's import rows), not of results, and passes here.
"""
import json

import numpy as np
import pytest

import import_scenarios as S
from conftest import GOLDEN

from k2hash_amd import archive

SCENARIOS = S.all_scenarios()
ROWS = sorted({(s.row, s.fmt) for s in SCENARIOS})
INDEX = {(s.row, s.name): i for i, s in enumerate(SCENARIOS)}


@pytest.fixture(scope="module")
def refs():
    """ref_scan of every scenario, computed once: (row, name) -> (error, records)."""
    return {(s.row, s.name): S.ref_scan(s.data, s.fmt) for s in SCENARIOS}


@pytest.fixture(scope="module")
def summaries():
    return {(s.row, s.name): S.summary(S.span_model(s.data, s.fmt)) for s in SCENARIOS}


# ------------------------------------------------------------------------------------- CPU
def test_constants_are_the_ones_the_builders_assume():
    assert S.B == S.kTThreads * S.T and S.U * 2 == S.B and S.US == S.SPU * S.kSlots
    assert S.EC == 6 and S.kHdrRecs == 3            # the span table's six 2-bit types; five header lines
    assert S.kPre < S.T < S.SL < 2 * S.T + 46 and S.SPU < S.SR < S.US and S.T % 4 == 0
    assert max(len(s.data) for s in SCENARIOS if s.row != 11) <= 3 * S.B
    assert max(len(s.data) for s in SCENARIOS) <= 4 * S.B


def test_ref_scan_matches_the_reference_tool():
    """Count, key and value bytes, key_off, val_off and the error flag of every fixture input, as
    the reference's own loops over libstdc++ getline printed them."""
    fixture = json.loads((GOLDEN / "import.json").read_text())["inputs"]
    assert len(fixture) >= 43
    for name, exp in sorted(fixture.items()):
        data = (GOLDEN / "import" / name).read_bytes()
        error, recs = S.ref_scan(data, exp["format"])
        assert error == exp["error"], name
        assert len(recs) == len(exp["records"]), name
        for (ko, kl, vo, vl), e in zip(recs, exp["records"]):
            assert data[ko:ko + kl] == bytes.fromhex(e["key"]), (name, e)
            assert data[vo:vo + vl] == bytes.fromhex(e["val"]), (name, e)
            assert ko == e["key_off"], (name, e)
            if e["val_off"] >= 0:  # tellg is -1 once the stream hit EOF
                assert vo == e["val_off"], (name, e)


def test_host_scanner_matches_ref_scan(refs):
    for s in SCENARIOS:
        error, recs = refs[(s.row, s.name)]
        if error:
            with pytest.raises(Exception):
                archive.import_scan(s.data, s.fmt)
            continue
        got = archive.import_scan(s.data, s.fmt)
        want = S.recs_array(recs)
        assert got.size == len(recs), (s.row, s.name)
        for c, name in enumerate(archive.IMPORT_DTYPE.names):
            assert np.array_equal(got[name], want[:, c]), (s.row, s.name, name)


def test_model_machine_matches_ref_scan(refs):
    """span_model's own getline machine (the one the device runs) yields ref_scan's records, so
    what it classifies are the real keys."""
    for s in SCENARIOS:
        error, recs = refs[(s.row, s.name)]
        m = S.span_model(s.data, s.fmt)
        if not error:
            assert m["count"] == len(recs) and m["records"] == recs, (s.row, s.name)


def test_scenarios_reach_what_they_claim(summaries):
    for s in SCENARIOS:
        q = summaries[(s.row, s.name)]
        assert not S.claims_hold(q, s.claims), (s.row, s.name)
        if s.fmt == "tsv":   # every miss has a reason the model knows
            assert not q["misses"].get("other"), (s.row, s.name, q["misses"])


def test_claims_cover_every_path():
    """The union of what the scenarios claim (and test_scenarios_reach_what_they_claim proves):
    every miss reason, both store forms with both hash sources, the 7-bit ballot count, the over
    path, the second slot load and pass A's second hashing round."""
    def claimed(name):
        out = []
        for s in SCENARIOS:
            w = s.claims.get(name)
            if w is not None:
                out.append(w)
        return out

    def members(name):
        got = set()
        for w in claimed(name):
            if isinstance(w, tuple) and w[0] == "has":
                got |= w[1] if isinstance(w[1], (set, frozenset)) else {w[1]}
        return got

    assert members("misses") >= {"newline_in_key", "head_beyond_pre", "fourth_cut", "over", "len", "rank", "over_between"}
    assert members("sources") == {("staged", "hit"), ("staged", "miss"), ("direct", "hit"), ("direct", "miss")}
    assert members("split_kv") == {("staged", "direct"), ("direct", "staged")}
    assert members("hit_kinds") == {"open", "head"} and members("hit_cuts") >= {0, 1, 2}
    assert members("unused_slots") >= {"head"}
    assert True in claimed("nb7") and True in claimed("second_load") and True in claimed("second_round")
    assert False in claimed("second_load") and False in claimed("second_round")
    assert any(w == 3 or w == ("has", 3) for w in claimed("max_ends_in_span") + claimed("ends_in_span"))
    assert {w for w in claimed("max_ends_in_span") if isinstance(w, int)} >= {4, S.T // 2 - 1, S.T // 2}
    assert any(isinstance(w, int) and w > 0 or isinstance(w, tuple) and w[1] > 0 for w in claimed("over_spans"))
    assert any(w == ("at", 2, 1) for w in claimed("unit_modes"))
    assert {w[2] for w in claimed("staged")} == {True, False}
    assert {w[2] for w in claimed("nrec")} >= {S.SR - 1, S.SR, S.SR + 1}
    assert {w[2] for w in claimed("named")} >= {S.SPU - 1, S.SPU, S.SPU + 1, S.SR, S.US - 1, S.US, S.US + 1}
    assert {w[2] for w in claimed("nk")} >= {0, 1, S.kTThreads - 1, S.kTThreads, S.kTThreads + 1, 2 * S.US}
    assert {r for r, _ in ROWS} == set(range(1, 16))
    # every arm, shift and canary occurs; one scenario per format runs the std-FNV arm
    runs = [r for i, s in enumerate(SCENARIOS) for r in S.matrix(s, i)]
    assert {r[0] for r in runs} == set(S.ARMS) and {r[1] for r in runs} == set(S.SHIFTS)
    assert {r[2] for r in runs} == set(S.CANARIES) and {r[3] for r in runs} >= {None, "-1", "+1", 0, 1}
    assert {s.fmt for s in SCENARIOS if s.row in S.STD_FNV_ROWS} == {"tsv", "mdbm"} and any(r[4] for r in runs)


# ------------------------------------------------------------------------------------- GPU
def _cap_of(cap, n):
    if cap is None:
        return n
    if isinstance(cap, str):
        return max(n + int(cap), 0)
    return cap


@pytest.mark.gpu
@pytest.mark.parametrize("row,fmt", ROWS)
def test_row(cuda, oracle, refs, row, fmt):
    """Every scenario of the row through every run of its matrix."""
    for s in (x for x in SCENARIOS if (x.row, x.fmt) == (row, fmt)):
        error, recs = refs[(s.row, s.name)]
        hashes = {}
        files = {}
        for arm, shift, canary, cap, std in S.matrix(s, INDEX[(s.row, s.name)]):
            if std not in hashes:
                hashes[std] = S.oracle_hashes(oracle, s.data, recs, std)
            if (shift, canary) not in files:
                files[(shift, canary)] = S.place(cuda, s.data, shift, canary)
            c = _cap_of(cap, len(recs))
            what = (row, s.name, arm, f"shift {shift}", f"canary {canary:#x}", f"cap {c}", "std-fnv" if std else "k2h")
            rc, count, got = S.run_scan(cuda, files[(shift, canary)], s.fmt, arm, c, std)
            print(what, "rc", rc, "count", count, "expected", "error" if error else len(recs))
            S.check(what, arm, c, rc, count, got, error, recs, *hashes[std])


@pytest.mark.gpu
def test_host_prehash_matches_the_oracle(cuda, oracle, refs):
    """k2h_amd_import_prehash_host (the host scanner's companion) on the first scenario with
    records of every row, against the oracle."""
    seen = set()
    for s in SCENARIOS:
        error, recs = refs[(s.row, s.name)]
        if (s.row, s.fmt) in seen or error or not recs:
            continue
        seen.add((s.row, s.fmt))
        h1, h2 = archive.import_prehash(s.data, archive.import_scan(s.data, s.fmt), s.fmt)
        w1, w2 = S.oracle_hashes(oracle, s.data, recs)
        assert np.array_equal(h1, w1) and np.array_equal(h2, w2), (s.row, s.name)
