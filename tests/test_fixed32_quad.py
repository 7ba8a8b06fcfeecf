"""The four-keys-per-lane fixed32 kernel (fnv_fixed32_quad_kernel) against the oracle.

Its blocks own 256 keys: a block whose keys all exist takes the one-statement fast path,
the block that straddles n hashes key by key.  The shapes here sit on that block edge and
on the full-block / tail switch; every comparison is with the oracle's hashes, never with
the library itself.  The last test needs no GPU: it reads the kernel's register budget
from the gfx950 assembly.
"""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import k2hash_amd
from k2hash_amd import batch

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "k2hash_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"

NMAX = 65536 + 129
EDGES = [1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 511, 512, 513, 767, 769, 1025, NMAX]
ARMS = [255, 256, 257, 513]
SENTINEL = -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def ref(oracle):
    """(key bytes, h1, h2) of NMAX seeded 32-byte keys; key i's hashes depend on its own
    bytes only, so the first n keys are the reference for every n <= NMAX.  Read-only."""
    data = oracle.gen_bytes(32 * NMAX, byte_off=32 * 2468)
    r1, r2 = oracle.hash_fixed(data, 32)
    for a in (data, r1, r2):
        a.setflags(write=False)
    return data, r1, r2


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def dev_keys(torch, data, device, front=0, back=16):
    """Device copy of `data` starting `front` bytes into a 0xA5-filled allocation with
    `back` more bytes behind it; returns (whole allocation, the key view)."""
    buf = torch.full((front + data.size + back,), 0xA5, dtype=torch.uint8, device=device)
    buf[front:front + data.size] = torch.from_numpy(np.array(data))
    return buf, buf[front:front + data.size]


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_block_edges(cuda, ref, n):
    import torch
    data, r1, _ = ref
    _, keys = dev_keys(torch, data[:32 * n], cuda)
    h1, _ = k2hash_amd.hash_fixed(keys, 32, second=False)
    torch.cuda.synchronize()
    assert np.array_equal(host_u64(h1), r1[:n])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["high", "low", "random"])
def test_sign_path_in_every_lane_and_row(cuda, oracle, ref, kind):
    """n = 512 is two full blocks: every lane of every key row hashes bytes that are all
    >= 0x80 (sign-extended), all < 0x80, or mixed."""
    import torch
    n = 512
    data = np.array(ref[0][:32 * n])
    if kind == "high":
        data |= 0x80
    elif kind == "low":
        data &= 0x7F
    r1, _ = oracle.hash_fixed(data, 32)
    _, keys = dev_keys(torch, data, cuda)
    h1, _ = k2hash_amd.hash_fixed(keys, 32, second=False)
    torch.cuda.synchronize()
    assert np.array_equal(host_u64(h1), r1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ARMS)
def test_canaries(cuda, ref, n):
    """Nothing before keys[0], after the last key, before h1[0] or after h1[n-1] changes."""
    import torch
    data, r1, _ = ref
    buf, keys = dev_keys(torch, data[:32 * n], cuda, front=64, back=64)
    before = buf.clone()
    hb = torch.full((n + 16,), SENTINEL, dtype=torch.int64, device=cuda)
    k2hash_amd.hash_fixed(keys, 32, second=False, out=(hb[8:8 + n], None))
    torch.cuda.synchronize()
    assert np.array_equal(host_u64(hb[8:8 + n]), r1[:n])
    assert bool((hb[:8] == SENTINEL).all()) and bool((hb[8 + n:] == SENTINEL).all())
    assert bool((buf == before).all())
    assert bool((buf[:64] == 0xA5).all()) and bool((buf[64 + 32 * n:] == 0xA5).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, 1025])
def test_alignment(cuda, ref, n):
    """Keys 16 B into an allocation (16-aligned, not 32-aligned) and an h1 view one element in
    are served by the fast path; keys at +8 B fall back to the generic kernel.  All match."""
    import torch
    data, r1, _ = ref
    for front in (16, 8):
        _, keys = dev_keys(torch, data[:32 * n], cuda, front=front)
        assert keys.data_ptr() % 32 == front
        hb = torch.full((n + 2,), SENTINEL, dtype=torch.int64, device=cuda)
        k2hash_amd.hash_fixed(keys, 32, second=False, out=(hb[1:1 + n], None))
        torch.cuda.synchronize()
        assert np.array_equal(host_u64(hb[1:1 + n]), r1[:n]), front
        assert int(hb[0]) == SENTINEL and int(hb[n + 1]) == SENTINEL, front


@pytest.mark.gpu
@pytest.mark.parametrize("n", ARMS)
def test_second_hash_and_index_arms(cuda, oracle, ref, n):
    import torch
    data, r1, r2 = ref
    _, keys = dev_keys(torch, data[:32 * n], cuda)
    h1, h2 = k2hash_amd.hash_fixed(keys, 32, second=True)
    cur, cm = (1 << 28) - 1, 0xF
    rk, rc = oracle.bucket_index(r1[:n], cur, cm)
    outs = [batch.hash_fixed_index(keys, 32, cur, cm, second=s) for s in (False, True)]
    torch.cuda.synchronize()
    assert np.array_equal(host_u64(h1), r1[:n])
    assert np.array_equal(host_u64(h2), r2[:n])
    for g1, g2, k, c in outs:
        assert np.array_equal(host_u64(g1), r1[:n])
        assert g2 is None or np.array_equal(host_u64(g2), r2[:n])
        assert np.array_equal(host_u64(k), rk)
        assert np.array_equal(host_u64(c), rc)


@pytest.mark.gpu
def test_non_default_stream(cuda, ref):
    import torch
    n = 1025
    data, r1, _ = ref
    _, keys = dev_keys(torch, data[:32 * n], cuda)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        h1, _ = k2hash_amd.hash_fixed(keys, 32, second=False, stream=s)
    s.synchronize()
    assert np.array_equal(host_u64(h1), r1[:n])


def test_register_budget(tmp_path):
    """vgpr_count <= 64 (8 waves per SIMD), no spills, no scratch: from the metadata of the
    assembly that the Makefile's `asm` target writes."""
    if not Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    subprocess.run(["make", "-C", str(CSRC), "asm", f"OUT={tmp_path}", "HIP_SRCS=k2h_kernels.hip"], check=True,
                   capture_output=True)
    asm = (tmp_path / "asm" / "k2h_kernels.s").read_text()
    meta = {}
    for block in re.split(r"\n\s+- \.agpr_count:", asm):
        m = re.search(r"\.name:\s+(_Z\w+)", block)
        if m:
            meta[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, flags=re.M)}
    quad = {k: v for k, v in meta.items() if "fnv_fixed32_quad_kernel" in k}
    assert quad, sorted(meta)
    for sym, f in quad.items():
        assert f["vgpr_count"] <= 64, (sym, f["vgpr_count"])
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, sym
        assert f.get("private_segment_fixed_size", 0) == 0, sym
