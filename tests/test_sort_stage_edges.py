"""The calls that sort (hash, index) pairs, at the pair counts where the stage around the sort can
go wrong: one pair, two, and 255, 256, 257 and 513 -- on both sides of a 256-slot tile of the
gather and compact kernels, and of a second one.  k2h_amd_ralledata_dedup, k2h_amd_ralledata_subkeys,
k2h_amd_archive_fold and k2h_amd_archive_apply, each against the model its own tests use, every
output element compared.

Every stream holds identities that repeat and blobs or records that take no part, so the compact
kernel places participants and the others on both sides of each edge.  Beyond the sizes:
  subkeys  E = 0 (no pair but the blobs'), and E that carries n + E over a tile edge that n is
           short of (the tiles are the blobs', the pairs the blobs' and the names');
  fold     a RENAME on each side of every tile edge, so that the high half of the packed tile
           counts and of their scan is what gives the records behind it their segment;
  apply    each pair count as held blobs alone (n = 0), as records alone (na = 0) and as both.

k2h_amd_ralledata_diff is left out: tests/test_ralledata_diff.py::test_sizes runs na over 1, 255,
256, 257 and nb over 0, 1, 255, 256, 257 against the model, which has nb = 0 and every pair count
here (1 + 0, 1 + 1, 255 + 0, 256 + 0, 257 + 0, 256 + 257) among its 20 shapes.
"""
import numpy as np
import pytest

import archive_apply_model as am
import archive_fold_model as fm
import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_subkeys_model as sm
import ralle_times_model as tm
from archive_fold_model import Rec
from ralle_unlink_model import layout

from k2hash_amd import archive

SIZES = (1, 2, 255, 256, 257, 513)
TILE = 256


def _consider(n):
    """Every sixth blob or record takes no part, from the fifth on."""
    return (np.arange(n) % 6 != 4).astype(np.uint8)


# --------------------------------------------------------------------------------------- dedup
@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_dedup(cuda, oracle, n):
    nkeys = max(1, n - n // 4)                       # the last quarter lays earlier keys down again
    keys = [b"dedup-edge-%04d" % (i * 5 % nkeys) for i in range(n)]
    blobs = dm.blobs_of(oracle, keys, [b"v%d" % i for i in range(n)])
    buf, off = rm.join(blobs)
    consider = _consider(n)
    want = dm.dedup_model(buf, off, consider=consider)
    got = tm.run_dedup_mtime(cuda, tm.place(cuda, buf, n % 16), len(buf), off, None, consider, plain=True)
    tm.assert_dedup(got, want, f"dedup of {n} blobs")
    assert want[2] == (0 if n < 255 else int((want[1] != dm.NONE).sum())) and (n < 255 or want[2] > n // 8)


# ------------------------------------------------------------------------------------- subkeys
SUBKEYS = [(1, 0), (1, 1), (2, 1), (255, 0), (255, 1), (255, 2), (250, 10), (256, 0), (256, 1), (257, 3), (513, 0),
           (513, 200)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,E", SUBKEYS)
def test_subkeys(cuda, oracle, n, E):
    nkeys = max(1, n - n // 8)
    keys = [b"sk-edge-%04d" % (i % nkeys) for i in range(n)]
    consider = _consider(n)
    owners = np.flatnonzero(consider)
    names = [[] for _ in range(n)]
    for j in range(E):                               # every fourth name has no blob
        name = b"nobody-%d" % j if j % 4 == 3 else b"sk-edge-%04d" % ((7 * j + 1) % nkeys)
        names[int(owners[3 * j % owners.size])].append(name)
    blobs = sm.blobs_with_lists(oracle, keys, [sm.serialize(x) if x else b"" for x in names])
    buf, off = rm.join(blobs)
    want = sm.edges_model(oracle, buf, off, consider=consider)
    assert want.counts[3] == E and (n + E - 1) // TILE >= (n - 1) // TILE
    got = sm.run_subkeys(cuda, tm.place(cuda, buf, (n + E) % 16), len(buf), off, consider)
    sm.assert_edges(got, want, f"subkeys of {n} blobs with {E} names")


def test_subkeys_cases_cross_a_tile_edge_by_their_names_alone():
    assert any(n % TILE and (n - 1) // TILE < (n + E - 1) // TILE for n, E in SUBKEYS)
    assert {n + E for n, E in SUBKEYS} >= {1, 2, 255, 256, 257, 513} and {n for n, E in SUBKEYS if E == 0} >= {1, 256}


# ---------------------------------------------------------------------------------------- fold
def _fold_log(n):
    """n records over n // 3 + 1 keys; from 255 records on a RENAME in the last slot of every
    tile (the log's last record where the tile is not full), in the first slot of the next tile, and
    one early in the log."""
    rng = np.random.default_rng(n)
    keys = [b"fold-edge-%04d" % k for k in range(n // 3 + 1)]
    which = [int(rng.integers(0, len(keys))) for _ in range(n)]
    log = [fm.letter(fm.TWELVE[int(rng.integers(0, 12))], keys[which[i]], i) for i in range(n)]
    renames = set()
    if n >= TILE - 1:
        renames = {i for edge in range(TILE, n + TILE, TILE) for i in (min(edge, n) - 1, edge) if i < n} | {n // 3}
    renames = sorted(renames)
    for at in renames:
        log[at] = Rec(fm.RENAME, keys[which[at]], b"", b"", b"ren-attrs", b"renamed-%d" % at)
    return log, np.array(which, np.uint64), renames


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_fold(cuda, n):
    log, which, renames = _fold_log(n)
    data = b"".join(fm.record_bytes(r) for r in log)
    recs = archive.scan(data)
    assert recs.size == n and not recs["status"].any()
    want = fm.fold_model(log)
    assert all(want[0][i] for i in renames)
    if n >= 255:                                     # both sides of the edge, and records behind each RENAME
        assert {i % TILE for i in renames} >= ({TILE - 1, 0} if n > TILE else {(n - 1) % TILE})
        assert want[2] > n // 8
    # h1: computed by the call, and the caller's -- any function of the key serves as the grouping hash
    for name, h1 in (("h1 computed", None), ("h1 passed", (which + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))):
        fm.assert_same(fm.run_fold(cuda, data, recs, h1=h1, shift=n % 16), want, f"fold of {n} records, {name}")


# --------------------------------------------------------------------------------------- apply
APPLY = sorted({(na, N - na) for N in SIZES for na in (0, N // 2, N)})


@pytest.mark.gpu
@pytest.mark.parametrize("na,n", APPLY)
def test_apply(cuda, oracle, na, n):
    nkeys = max(1, na - na // 10)                    # the last tenth of the held blobs repeats earlier identities
    hkeys = [b"apply-edge-%04d" % (j * 3 % nkeys) for j in range(na)]
    strangers = [b"apply-stranger-%04d" % j for j in range(n // 4 + 1)]
    pool = sorted(set(hkeys)) + strangers
    log = [fm.letter(("rep-v", "set-vs", "del", "rep-a", "rep-s", "set-v")[i % 6], pool[i * 7 % len(pool)], i) for i in range(n)]
    hs = am.hashes_of(oracle, hkeys)
    blobs = [layout(hs[k], k, b"held-%d" % j, b"S%d" % j if j % 3 else b"", b"A%d" % j if j % 2 else b"")
             for j, k in enumerate(hkeys)]
    held, off = rm.join(blobs, lead=b"\x66" * 3) if na else (b"", [0])
    keep = _consider(na) if na else None
    consider = _consider(n) if n else None
    file, recs = am.build_log(log)
    h1, h2 = am.rec_hashes(oracle, log)
    want = am.apply_model(bytes(held), off, keep, fm.recs_of(file, recs), consider, h1, h2)
    assert want.stop == n
    if na >= 255 and n == 0:
        assert want.counts[4] > 0                    # superseded copies
    if na >= 127 and n >= 127:
        assert min(want.counts[3:]) > 0 and want.counts[0] > want.counts[2] > 0
    got = am.run_apply(cuda, bytes(held), off, recs, file, keep=keep, consider=consider, h1=h1, h2=h2)
    am.assert_applied(got, want, f"apply of {n} records to {na} held blobs")


def test_apply_cases_hold_both_empty_sides_at_every_size():
    assert {na + n for na, n in APPLY} == set(SIZES)
    assert all((0, N) in APPLY and (N, 0) in APPLY for N in SIZES)
