"""Every launch arm x output arm x seed, against the oracle.

launch_fixed / launch_fixed_long / launch_csr_tile pick a kernel by key length and base
alignment and an instantiation by with_h2_epi(h2, index); K2H_AMD_FLAG_STD_FNV reaches each as
a runtime seed (the four-key fixed32 statement holds it in an SGPR pair, the chunk walkers in
the S_p table, the line-DMA kernel as the start state).  Each launch arm below is the smallest
n that covers a full block plus a straddling one; it runs {h1 only, h1 + h2, h1 + h2 + fused
index} x {builtin seed, std seed}, every key compared with the oracle's variant 0 or 1.

The second half runs the host forms and the archive / import prehash calls with std_fnv=True
against variant 1 (archive keys as stored, import keys as key + NUL).
"""
import json

import numpy as np
import pytest

import csr_scenarios as cs
from conftest import GOLDEN

from k2hash_amd import archive, batch

# name -> (key_len, shift of the base in a 128-aligned allocation, n)
FIXED_ARMS = {
    "fixed32-quad-or-two-key": (32, 16, 256 + 3),
    "fixed-short-21": (21, 0, 256 + 3),
    "fixed-short-32-unaligned": (32, 1, 256 + 3),
    "direct-100": (100, 0, 256 + 3),
    "ring-200": (200, 0, 256 + 3),
    "ring-256-base16": (256, 16, 256 + 3),
    "lines-256": (256, 0, 64 + 3),
    "lines-384": (384, 0, 64 + 3),
}
CSR_ARMS = {"csr-staged": (1, 60), "csr-oversize": (150, 400)}
SEEDS = [pytest.param(False, id="builtin"), pytest.param(True, id="std")]


def test_arm_table_reaches_each_launch_path():
    """launch_fixed's conditions, restated: which kernel each row of FIXED_ARMS takes."""
    def path(key_len, shift):
        if key_len == 32 and shift % 16 == 0:
            return "fixed32"
        if key_len <= 32:
            return "short"
        if key_len % 128 == 0 and shift % 128 == 0:
            return "lines"
        return "direct" if key_len < 128 else "ring"
    assert {k: path(v[0], v[1]) for k, v in FIXED_ARMS.items()} == {
        "fixed32-quad-or-two-key": "fixed32", "fixed-short-21": "short", "fixed-short-32-unaligned": "short",
        "direct-100": "direct", "ring-200": "ring", "ring-256-base16": "ring", "lines-256": "lines",
        "lines-384": "lines"}
    for key_len, shift, n in FIXED_ARMS.values():
        block = 64 if path(key_len, shift) == "lines" else 256  # keys per block (fixed32: 256 or 128)
        assert n > block and n % block and n % 128  # one full block and a straddling one
    for lo, hi in CSR_ARMS.values():
        span = 600 * (lo + hi) // 2
        assert (span > cs.STAGE + 20000) == (lo >= 150) and (span < cs.STAGE - 20000) == (lo < 150)


@pytest.mark.gpu
@pytest.mark.parametrize("std", SEEDS)
@pytest.mark.parametrize("name", sorted(FIXED_ARMS))
def test_fixed_arm(cuda, oracle, name, std):
    key_len, shift, n = FIXED_ARMS[name]
    data = oracle.gen_bytes(key_len * n, byte_off=31 * key_len + shift)
    r1, r2 = oracle.hash_fixed(data, key_len, variant=int(std))
    for arm in cs.ARMS:
        want = cs.expect(oracle, r1, r2, arm)
        for canary in cs.CANARIES:
            buf = cs.place(cuda, data, shift, canary)
            assert buf.data_ptr() % 128 == shift
            cs.assert_equal(cs.run_fixed(cuda, buf, key_len, arm, std_fnv=std), want, (name, arm, std, hex(canary)))


@pytest.mark.gpu
@pytest.mark.parametrize("std", SEEDS)
@pytest.mark.parametrize("name", sorted(CSR_ARMS))
def test_csr_arm(cuda, oracle, name, std):
    lo, hi = CSR_ARMS[name]
    lengths = np.random.default_rng(lo).integers(lo, hi + 1, 600)
    off = cs.offsets_of(lengths, 3)
    tiles = cs.tile_model(lengths, 3, 1)
    assert [t["staged"] for t in tiles] == [name == "csr-staged", True]  # the 88-key last tile is staged
    data = oracle.gen_bytes(int(off[-1]), byte_off=55)
    r1, r2 = oracle.hash_csr(data, off.astype(np.uint64), variant=int(std))
    for arm in cs.ARMS:
        want = cs.expect(oracle, r1, r2, arm)
        for canary in cs.CANARIES:
            buf = cs.place(cuda, data, 1, canary)
            cs.assert_equal(cs.run_csr(cuda, buf, off, arm, std_fnv=std), want, (name, arm, std, hex(canary)))


# ------------------------------------------------------------------ std seed: the host forms
@pytest.mark.gpu
@pytest.mark.parametrize("key_len", [32, 21])
def test_fixed_host_std(cuda, oracle, key_len):
    data = oracle.gen_bytes(key_len * 3001, byte_off=9)
    r1, r2 = oracle.hash_fixed(data, key_len, variant=1)
    h1, h2 = batch.hash_fixed_host(data, key_len, second=True, std_fnv=True)
    assert np.array_equal(h1, r1) and np.array_equal(h2, r2)
    g1, _ = batch.hash_fixed_host(data, key_len, std_fnv=True)
    assert np.array_equal(g1, r1)


@pytest.mark.gpu
def test_csr_host_std(cuda, oracle):
    off = oracle.gen_offsets(3001, 0, 300, base=5)
    data = oracle.gen_bytes(int(off[-1]), byte_off=3)
    r1, r2 = oracle.hash_csr(data, off, variant=1)
    h1, h2 = batch.hash_csr_host(data, off, second=True, std_fnv=True)
    assert np.array_equal(h1, r1) and np.array_equal(h2, r2)
    g1, _ = batch.hash_csr_host(data, off, std_fnv=True)
    assert np.array_equal(g1, r1)


# ----------------------------------------------------------- std seed: archive and import
def _u64(t):
    return [int(x) for x in (t if isinstance(t, np.ndarray) else t.cpu().numpy()).view(np.uint64)]


@pytest.mark.gpu
def test_archive_prehash_std(cuda, oracle):
    """archive.prehash, prehash_device and scan_prehash_device(rename=True) over the reference's
    own archive with the std seed: every record's key, and the new key of RENAME records."""
    import torch
    f = (GOLDEN / "archive.k2har").read_bytes()
    recs = json.loads((GOLDEN / "archive.json").read_text())["records"]
    keys = [bytes.fromhex(e["key"]) for e in recs]
    new = [bytes.fromhex(e["exdata"]) if e["type"] == archive.SCOM_RENAME else None for e in recs]
    assert any(new) and len(keys) > 7
    w1 = [oracle.k2h_hash(k, 1) for k in keys]
    w2 = [oracle.k2h_second_hash(k, 1) for k in keys]
    n1 = [oracle.k2h_hash(k, 1) if k is not None else 0 for k in new]
    n2 = [oracle.k2h_second_hash(k, 1) if k is not None else 0 for k in new]
    assert w1 != [oracle.k2h_hash(k, 0) for k in keys]
    want = [w1, w2, n1, n2]
    assert [_u64(x) for x in archive.prehash(f, rename=True, std_fnv=True)] == want
    assert [_u64(x) for x in archive.prehash(f, std_fnv=True)] == want[:2]
    d = torch.from_numpy(np.frombuffer(f, np.uint8).copy()).to(cuda)
    rows = archive.scan_device(d)
    assert rows.shape[0] == len(recs)
    assert [_u64(x) for x in archive.prehash_device(d, rows, rename=True, std_fnv=True)] == want
    out = archive.scan_prehash_device(d, rename=True, std_fnv=True)
    assert out[0].shape[0] == len(recs)
    assert [_u64(x) for x in out[1:]] == want


IMPORT_FILES = ("basic.tsv", "edge.tsv", "random.tsv", "fuzz_00300.tsv", "fuzz_04097.tsv", "good.mdbm",
                "fuzz_00300.mdbm", "fuzz_04097.mdbm")


@pytest.mark.gpu
@pytest.mark.parametrize("name", IMPORT_FILES)
def test_import_prehash_std(cuda, oracle, name):
    """import_prehash (host pipeline), import_prehash_device and the fused scan over the committed
    k2himport inputs with the std seed: each key hashed as key + NUL."""
    import torch
    exp = json.loads((GOLDEN / "import.json").read_text())["inputs"][name]
    assert not exp["error"] and exp["records"]
    fmt = "mdbm" if name.endswith(".mdbm") else "tsv"
    keys = [bytes.fromhex(e["key"]) + b"\0" for e in exp["records"]]
    want = [[oracle.k2h_hash(k, 1) for k in keys], [oracle.k2h_second_hash(k, 1) for k in keys]]
    data = (GOLDEN / "import" / name).read_bytes()
    assert [_u64(x) for x in archive.import_prehash(data, fmt=fmt, std_fnv=True)] == want
    d = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(cuda)
    rows = archive.import_scan_device(d, fmt)
    assert rows.shape[0] == len(keys)
    assert [_u64(x) for x in archive.import_prehash_device(d, rows, std_fnv=True)] == want
    out = archive.import_scan_prehash_device(d, fmt, std_fnv=True)
    assert out[0].shape[0] == len(keys)
    assert [_u64(x) for x in out[1:]] == want
