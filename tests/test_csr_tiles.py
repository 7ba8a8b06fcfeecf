"""The CSR kernel (k2h_csr.hip: fnv_csr_staged_kernel, pair_walk, oversize_tile, ring_hash) at
the shapes it branches on, every key of every case against the oracle.

The scenarios (csr_scenarios.py) are built from kTileKeys and kStageBytes as the kernel source
states them.  Each runs through three output arms -- h1 only (the benchmark's instantiation),
h1 + h2, h1 + h2 + the fused bucket index -- from a buffer that starts `shift` bytes into its
allocation, between canary bytes that differ between two runs; both runs must equal the
oracle.  Outputs are sentinel-filled first, so a key the kernel never stores is a mismatch
(an empty key's hash is 0, which fresh memory often holds).

test_scenarios_have_the_properties_their_rows_claim runs without a GPU: it recomputes span,
delta, the chunk counts in sort order, pair_walk's (k0, k1) pairs and ring_hash's mis / first /
rounds from each scenario and checks that the scenario reaches what it was built for.
"""
import numpy as np
import pytest

import csr_scenarios as cs
from csr_scenarios import STAGE, TK

SCENARIOS = cs.scenarios()


def payload_of(oracle, lengths, first_offset, salt):
    """Bytes of both signs for the keys and for the first_offset bytes in front of them."""
    return oracle.gen_bytes(first_offset + int(np.sum(lengths)), byte_off=1000 * salt + 17)


def check_arms(cuda, oracle, payload, off, shift, what, host=None, host_off=None):
    """All three arms, both canaries, against the oracle over the host bytes."""
    r1, r2 = oracle.hash_csr(payload if host is None else host, (off if host_off is None else host_off).astype(np.uint64))
    for arm in cs.ARMS:
        want = cs.expect(oracle, r1, r2, arm)
        for canary in cs.CANARIES:
            buf = cs.place(cuda, payload, shift, canary)
            cs.assert_equal(cs.run_csr(cuda, buf, off, arm), want, (what, arm, hex(canary)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_scenario(cuda, oracle, name):
    lengths, first, shift = SCENARIOS[name]
    payload = payload_of(oracle, lengths, first, sorted(SCENARIOS).index(name))
    check_arms(cuda, oracle, payload, cs.offsets_of(lengths, first), shift, name)


@pytest.mark.gpu
@pytest.mark.parametrize("delta,first", sorted(cs.SLACK_PLACES))
def test_front_slack(cuda, oracle, delta, first):
    """Chunk 0 of a tile's first key starts in the 16 slack bytes in front of the stage (or in
    the delta bytes in front of the key) for every pad p = 0..15."""
    for r in range(len(cs.SLACK_LENGTHS)):
        lengths, f, shift = cs.front_slack(r, delta, first)
        payload = payload_of(oracle, lengths, f, 100 + r)
        check_arms(cuda, oracle, payload, cs.offsets_of(lengths, f), shift, ("front-slack", r, delta, first))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["parities", "ring-rounds-24"])
def test_table_index_arm(cuda, oracle, name):
    """k2h_amd_hash_csr_index_table over one staged and one oversize scenario, the bitmap that
    of a table whose top area is half assigned."""
    import torch

    from k2hash_amd import batch
    lengths, first, shift = SCENARIOS[name]
    assert cs.tile_model(lengths, first, shift)[0]["staged"] == (name == "parities")
    payload = payload_of(oracle, lengths, first, 7)
    off = cs.offsets_of(lengths, first)
    cur = (1 << 16) - 1
    bm = batch.expanded_table_bitmap(cur, 0.5, seed=11)
    assigned = torch.from_numpy(bm.view(np.int32).copy()).to(cuda)
    r1, r2 = oracle.hash_csr(payload, off.astype(np.uint64))
    k, c, f = oracle.bucket_index_table(r1, cur, cs.COL_MASK, bm)
    assert 0 < int(f.sum()) and len(np.unique(k)) > 100
    want = {"h1": r1, "h2": r2, "kindex": k, "ckindex": c, "found": f}
    for canary in cs.CANARIES:
        buf = cs.place(cuda, payload, shift, canary)
        out = batch.hash_csr_index_table(buf, torch.from_numpy(off).to(cuda), cur, cs.COL_MASK, assigned, second=True)
        torch.cuda.synchronize()
        got = {n: t.cpu().numpy().view(np.uint64 if n != "found" else np.uint8) for n, t in zip(want, out)}
        cs.assert_equal(got, want, (name, "table", hex(canary)))


@pytest.mark.gpu
def test_tile_straddles_byte_offset_2_pow_32(cuda, oracle):
    """A staged and an oversize tile that each contain byte offset 2^32 of their buffer (the
    kernel keeps a tile's offsets as 32-bit values relative to its first).  Only the last
    512 KiB of the 2^32 + 256 KiB buffer are written; the oracle hashes the host copy of that
    tail with rebased offsets."""
    import torch
    tail0 = cs.STRADDLE + (256 << 10) - cs.STRADDLE_TAIL
    big = torch.empty(cs.STRADDLE + (256 << 10), dtype=torch.uint8, device=cuda)
    assert big.data_ptr() % 128 == 0
    for kind in ("staged", "oversize"):
        lengths, first, _ = cs.straddle(kind)
        off = cs.offsets_of(lengths, first)
        r1 = r2 = None
        for canary in cs.CANARIES:
            tail = np.full(cs.STRADDLE_TAIL, canary, np.uint8)
            keys = oracle.gen_bytes(int(off[-1] - off[0]), byte_off=4242)
            tail[off[0] - tail0:off[-1] - tail0] = keys
            if r1 is None:
                r1, r2 = oracle.hash_csr(tail, (off - tail0).astype(np.uint64))
            big[tail0:] = torch.from_numpy(tail).to(cuda)
            for arm in cs.ARMS:
                cs.assert_equal(cs.run_csr(cuda, big, off, arm), cs.expect(oracle, r1, r2, arm),
                                ("straddle", kind, arm, hex(canary)))
    del big


# ------------------------------------------------------------------------------------- CPU
def _one(lengths, first, shift):
    (t,) = cs.tile_model(lengths, first, shift)
    return t


def test_scenarios_have_the_properties_their_rows_claim(oracle):
    sample = oracle.gen_bytes(4096, byte_off=17)
    assert (sample >= 0x80).any() and (sample < 0x80).any()  # key bytes of both signs
    assert TK % 64 == 0 and TK >= 256 and cs.GIANT < STAGE < cs.FILLER  # what the fixed sizes below assume

    # last-tile counts
    last = {1: 1, 2: 2, 3: 3, 63: 63, 65: 65, 511: 511, 512: 512, 513: 513 - TK, 1025: 1025 - 2 * TK}
    for n in cs.LAST_COUNTS:
        tiles = cs.tile_model(*cs.last_tile_staged(n))
        assert all(t["staged"] for t in tiles) and tiles[-1]["cnt"] == last[n]
        assert 1 <= tiles[-1]["lengths"].min() and tiles[-1]["lengths"].max() <= 40
        L, first, shift = cs.last_tile_long(n)
        assert L.size == n and 150 <= L.min() and L.max() <= 400
        tiles = cs.tile_model(L, first, shift)
        assert [t["staged"] for t in tiles] == [t["cnt"] < TK - 1 for t in tiles]
        tiles = cs.tile_model(*cs.last_tile_oversize(n))
        t = tiles[-1]
        assert not t["staged"] and t["cnt"] == last[n] and len(t["groups"]) == (t["cnt"] + 63) // 64
        assert t["idle_lanes"] == -t["cnt"] % 64 and t["waves_without_group"] == max(0, 4 - len(t["groups"]))
    assert {last[n] & 1 for n in cs.LAST_COUNTS} == {0, 1}
    assert cs.tile_model(*cs.last_tile_long(511))[0]["idle_lanes"] == 1          # a partial 64-key group
    assert cs.tile_model(*cs.last_tile_oversize(3))[0]["waves_without_group"] == 3  # cnt < 64

    # stage boundary
    for edge in cs.STAGE_EDGES:
        for delta in cs.STAGE_DELTAS:
            a, b = cs.tile_model(*cs.stage_boundary(edge, delta))
            assert (a["cnt"], a["delta"], a["span"]) == (TK, delta, STAGE + edge)
            assert a["staged"] == (edge <= 0) and a["lengths"][-1] >= 1
            assert b["staged"] and 0 < b["cnt"] < TK
    assert {cs.STAGE_DELTAS[d][0] for d in cs.STAGE_DELTAS} != {0} and \
        {cs.STAGE_DELTAS[d][1] for d in cs.STAGE_DELTAS} != {0}  # set through the shift and offsets[0]

    # front slack
    for (delta, first) in cs.SLACK_PLACES:
        below = set()
        for r in range(32):
            t = _one(*cs.front_slack(r, delta, first))
            assert t["staged"] and t["delta"] == delta and t["o0"] == first
            assert t["lengths"][0] == cs.SLACK_LENGTHS[r] and t["p"][0] == -cs.SLACK_LENGTHS[r] % 16
            assert -16 <= t["first_chunk0"] < 16  # inside the slack: never below the stage array
            if t["first_chunk0"] < 0:
                below.add(int(t["p"][0]))
        assert below == set(range(delta + 1, 16))  # pads larger than delta reach into the slack
    assert {-x % 16 for x in cs.SLACK_LENGTHS} == set(range(16))

    # switch parities
    tiles = cs.tile_model(*cs.switch_parities())
    assert len(tiles) == len(cs.PARITY_PAIRS) == 10
    for t, (a, b) in zip(tiles, cs.PARITY_PAIRS):
        assert t["staged"] and t["cnt"] == TK and t["pairs"] == [(a, b)] * (TK // 2)
        assert set(t["p"].tolist()) == set(range(16))
    assert {(a & 1, b & 1) for a, b in cs.PARITY_PAIRS} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert [_one(*cs.small_walk(w))["pairs"] for w in ("k1", "k2", "k1k1")] == [[(1, 0)], [(2, 0)], [(1, 1)]]

    # empties
    a, e, b = cs.tile_model(*cs.empty_tile_between())
    assert a["dma"] and b["dma"] and not e["dma"] and e["cnt"] == TK and e["oN"] == e["o0"] and e["pairs"] == []
    for pos in (0, TK // 2 - 1, TK - 1):
        t = _one(*cs.lone_byte(pos))
        assert t["cnt"] == TK and t["lengths"].sum() == 1 and t["lengths"][pos] == 1 and t["span"] == 1 + t["delta"]
        assert t["pairs"] == [(1, 0)] and t["only_b"] == 1 and t["both_empty"] == TK // 2 - 1
    t = _one(*cs.mostly_empty())
    assert (t["lengths"] == 0).sum() == 300 and t["lengths"].max() <= 64
    assert t["only_b"] == TK - 300 and t["both_empty"] == 300 - TK // 2 and all(kb == 0 for _, kb in t["pairs"])

    # giant in a staged tile
    for pos in (0, TK // 2 - 1, TK - 1):
        t = _one(*cs.giant_staged(pos))
        assert t["staged"] and t["cnt"] == TK and t["lengths"][pos] == 70000 and t["cls"][pos] >= 96
        assert np.delete(t["lengths"], pos).max() <= 8 and (t["lengths"] == 0).any()
        assert t["order"][-1] == pos and 4375 in t["pairs"][0]

    # oversize ring rounds
    t = _one(*cs.ring_rounds(5))
    assert not t["staged"] and t["cnt"] == 41 and len(t["groups"]) == 1
    assert t["idle_lanes"] == 23 and t["waves_without_group"] == 3
    assert set(t["rounds"].tolist()) >= {0, 1, 2, 3, 4} and (t["k"] == 0).sum() == 5
    t = _one(*cs.ring_rounds(24))
    assert not t["staged"] and len(t["groups"]) == 4 and t["waves_without_group"] == 0
    mixed = [len({int(t["rounds"][i]) for i in g}) for g in t["groups"]]
    assert max(mixed) >= 3 and t["idle_lanes"] == 63 and (t["k"][t["groups"][0]] == 0).any()
    assert set(t["k"].tolist()) == set(cs.RING_K) | {5000}
    t = _one(*cs.ring_mis())
    assert not t["staged"] and t["cnt"] <= TK
    have = set(zip(t["k"].tolist(), t["p"].tolist(), t["mis"].tolist()))
    assert have >= {(k, p, m) for k in cs.RING_MIS_K for p in cs.RING_MIS_P for m in cs.RING_MIS}
    assert set(t["first"].tolist()) == {0, 1}
    f1 = t["first"] == 1
    assert (t["p"][f1] > 0).all() and ((t["mis"] + t["p"])[f1] >= 128).all() and (t["k"][f1] >= 9).any()
    # chunk 8 of a key with mis >= 113 is read at ring byte mis + 128 > 240: through the mirror
    assert ((t["mis"] >= 113) & (t["k"] >= 9)).any()

    # 2^32 straddle
    for kind in ("staged", "oversize"):
        t = cs.tile_model(*cs.straddle(kind))[0]
        assert t["cnt"] == TK and t["staged"] == (kind == "staged")
        assert cs.STRADDLE + (256 << 10) - cs.STRADDLE_TAIL <= t["o0"] < cs.STRADDLE < t["oN"] <= cs.STRADDLE + (256 << 10)

    # the scenario table holds every row
    names = set(SCENARIOS)
    assert len(names) == 3 * len(cs.LAST_COUNTS) + 9 + 1 + 3 + 1 + 3 + 1 + 3 + 3
