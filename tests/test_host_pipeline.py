"""The host CSR / fixed pipelines (k2h_batch.cc) across their chunk cuts, against the oracle.

k2h_amd_hash_csr_host cuts a call into chunks of at most kChunkKeysMax keys and kChunkBytes
bytes (one key always fits), launches each with the byte base d_in - offsets[first], lays the
outputs out as d_out / d_out + cnt and drains them into the caller's h1 + first / h2 + first.
The two constants are read from the source; chunk_cuts() restates the cutting loop so that each
case can state where its cuts fall.  Every key's h1 and h2 is compared.
"""
import numpy as np
import pytest

from csr_scenarios import CHUNK_BYTES, CHUNK_KEYS, offsets_of

from k2hash_amd import batch

MIB = 1 << 20


def chunk_cuts(off):
    """(first, last) key ranges of the chunks k2h_amd_hash_csr_host makes of these offsets."""
    n, first, out = len(off) - 1, 0, []
    while first < n:
        cap = n if n - first < CHUNK_KEYS else first + CHUNK_KEYS
        # while (last < cap && off[last + 1] - off[first] <= kChunkBytes) ++last, from first + 1
        within = int(np.searchsorted(off, off[first] + CHUNK_BYTES, side="right")) - 1
        last = max(first + 1, min(cap, within))
        out.append((first, last))
        first = last
    return out


def key_cap_case():
    return np.ones(CHUNK_KEYS + 64, np.int64), 0


BIG = MIB - 3


def byte_cut_case():
    """70 keys of 1 MiB - 3 B; the first chunk is filled to the byte by a 187-byte and a 5-byte
    key and still takes the empty key that follows; the second starts with a 5-byte and an empty
    key.  offsets[0] = 5."""
    per = CHUNK_BYTES // BIG
    fill = CHUNK_BYTES - per * BIG - 5
    return np.array([BIG] * per + [fill, 5, 0, 5, 0] + [BIG] * (70 - per)), 5


def giant_key_case():
    return np.array([10, CHUNK_BYTES + 4097, 10]), 0


def test_cases_cut_where_they_claim():
    assert (CHUNK_BYTES, CHUNK_KEYS) == (64 * MIB, 4 * MIB)
    L, first = key_cap_case()
    assert chunk_cuts(offsets_of(L, first)) == [(0, CHUNK_KEYS), (CHUNK_KEYS, CHUNK_KEYS + 64)]
    L, first = byte_cut_case()
    off = offsets_of(L, first)
    (a0, a1), (b0, b1) = chunk_cuts(off)
    assert (L == BIG).sum() == 70 and first == 5
    assert off[a1] - off[a0] == CHUNK_BYTES and L[a1 - 2:a1].tolist() == [5, 0] and L[b0:b0 + 2].tolist() == [5, 0]
    assert b1 == L.size and a1 < CHUNK_KEYS  # cut by bytes, not by the key cap
    L, first = giant_key_case()
    assert chunk_cuts(offsets_of(L, first)) == [(0, 1), (1, 2), (2, 3)] and L[1] > CHUNK_BYTES


@pytest.mark.gpu
@pytest.mark.parametrize("case", [key_cap_case, byte_cut_case, giant_key_case], ids=["key-cap", "bytes", "giant-key"])
def test_csr_host_across_cuts(cuda, oracle, case):
    L, first = case()
    off = offsets_of(L, first).astype(np.uint64)
    data = oracle.gen_bytes(int(off[-1]), byte_off=12345)
    r1, r2 = oracle.hash_csr(data, off)
    h1 = np.full(L.size, 0x5A5A5A5A5A5A5A5A, np.uint64)
    h2 = h1.copy()
    batch.hash_csr_host(data, off, second=True, out=(h1, h2))
    assert np.array_equal(h1, r1), np.flatnonzero(h1 != r1)[:8]
    assert np.array_equal(h2, r2), np.flatnonzero(h2 != r2)[:8]


@pytest.mark.gpu
def test_fixed_host_one_key_per_chunk(cuda, oracle):
    """key_len = 48 MiB: per = kChunkBytes / key_len = 1, three chunks of one key, h1 + h2."""
    key_len = 48 * MIB
    assert CHUNK_BYTES // key_len == 1
    data = oracle.gen_bytes(3 * key_len, byte_off=99)
    r1, r2 = oracle.hash_fixed(data, key_len)
    h1, h2 = batch.hash_fixed_host(data, key_len, second=True)
    assert np.array_equal(h1, r1) and np.array_equal(h2, r2)
