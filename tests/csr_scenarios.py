"""Helper for tests/test_csr_tiles.py, test_hash_arms.py and test_ranges.py (not a test module).

* The CSR kernel's two constants, read from its source, and a model of what it derives from a
  call's offsets: per tile the span, delta and staged / oversize decision, the keys' chunk
  counts in sort-class order, the (k0, k1) pairs pair_walk is handed, and for an oversize tile
  each key's line-ring quantities (mis, first, rounds) and its 64-key groups.
* One scenario builder per row of the tile matrix, each returning
  (lengths, first_offset, buffer_shift): key i has lengths[i] bytes, offsets[0] = first_offset,
  and the byte buffer handed to the API starts buffer_shift bytes into a 128-aligned
  allocation and ends at the last key's last byte.
* place(): such a buffer on the device, canary bytes on either side; run_csr() / run_fixed():
  one output arm of one call into sentinel-filled outputs, returned as host arrays.

Within one sort class the device order is free (LDS atomics), but every key of a class below
96 has the same chunk count, so everything modelled here is determined as long as a class >= 96
holds one key at most -- tile_model asserts that.
"""
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "k2hash_amd" / "csrc"


def _const(text, name):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, name
    expr = re.sub(r"(?<=\d)(ull|u|ul)\b", "", m.group(1).strip(), flags=re.I)
    assert re.fullmatch(r"[\d\s*<>+()x0-9a-fA-F]+", expr), (name, expr)
    return int(eval(expr, {"__builtins__": {}}))  # noqa: S307  (digits and operators only)


_CSR = (CSRC / "k2h_csr.hip").read_text()
TK = _const(_CSR, "kTileKeys")        # keys per tile (512)
STAGE = _const(_CSR, "kStageBytes")   # LDS stage (72 KiB)
_BATCH = (CSRC / "k2h_batch.cc").read_text()
CHUNK_BYTES = _const(_BATCH, "kChunkBytes")      # host pipeline: bytes per chunk (64 MiB)
CHUNK_KEYS = _const(_BATCH, "kChunkKeysMax")     # host pipeline: keys per chunk (4 M)

PAD = 128            # canary bytes on either side of a placed buffer (keeps the 128-alignment)
CANARIES = (0x00, 0xA5)
SENTINEL = 0x5A5AA5A55A5AA5A5
CUR_MASK, COL_MASK = (1 << 28) - 1, 0xF
ARMS = ("h1", "h1h2", "index")


# --------------------------------------------------------------------------- the kernel model
def offsets_of(lengths, first_offset):
    off = np.empty(len(lengths) + 1, np.int64)
    off[0] = first_offset
    off[1:] = first_offset + np.cumsum(np.asarray(lengths, np.int64))
    return off


def chunks(length):
    return (np.asarray(length, np.int64) + 15) >> 4


def pads(length):
    return (-np.asarray(length, np.int64)) & 15


def sort_class(length):
    """len_bin128: the chunk count below 96, then four classes per octave, capped at 127."""
    out = []
    for k in chunks(length).tolist():
        if k < 96:
            out.append(k)
        else:
            lg = k.bit_length() - 1
            out.append(min(96 + (lg - 6) * 4 + ((k >> (lg - 2)) & 3), 127))
    return np.array(out, np.int64)


def tile_model(lengths, first_offset, shift):
    """One dict per tile of the call, with what fnv_csr_staged_kernel derives for it."""
    lengths = np.asarray(lengths, np.int64)
    off = offsets_of(lengths, first_offset)
    tiles = []
    for t0 in range(0, lengths.size, TK):
        cnt = min(TK, lengths.size - t0)
        L = lengths[t0:t0 + cnt]
        o0, oN = int(off[t0]), int(off[t0 + cnt])
        delta = (shift + o0) & 15
        span = oN - o0 + delta
        cls = sort_class(L)
        big = cls[cls >= 96]
        assert np.unique(big).size == big.size, "two keys share a class >= 96: order not determined"
        order = np.argsort(cls, kind="stable")
        k, p = chunks(L), pads(L)
        t = dict(t0=t0, cnt=cnt, o0=o0, oN=oN, delta=delta, span=span, staged=span <= STAGE, lengths=L,
                 k=k, p=p, cls=cls, order=order, dma=oN > o0)
        if t["staged"]:
            pairs, only_b, both_empty = [], 0, 0
            for i in range((cnt + 1) // 2):
                ka = int(k[order[i]])
                kb = int(k[order[cnt - 1 - i]]) if i < cnt // 2 else 0
                if ka == 0:  # only_b: key A empty, key B walked alone
                    only_b += kb > 0
                    both_empty += kb == 0
                    ka, kb = kb, 0
                if ka:
                    pairs.append((ka, kb))
            t.update(pairs=pairs, only_b=only_b, both_empty=both_empty)
            # bytes of the stage in front of the tile's first staged byte that chunk 0 of the
            # tile's first key covers (masked pad bytes): its start relative to the stage
            t["first_chunk0"] = delta + int(L[0]) - 16 * int(k[0])
        else:
            end = shift + off[t0 + 1:t0 + cnt + 1]
            cp = end - 16 * k
            mis = cp & 127
            first = np.where(k > 0, ((end - L) - (cp & ~127)) >> 7, 0)
            rounds = (k + 7) >> 3
            groups = [order[g:g + 64] for g in range(0, cnt, 64)]
            t.update(mis=mis, first=first, rounds=rounds, groups=groups,
                     idle_lanes=64 * len(groups) - cnt, waves_without_group=max(0, 4 - len(groups)))
        tiles.append(t)
    return tiles


# ------------------------------------------------------------------------ scenario builders
def _rng(*salt):
    return np.random.default_rng([20240 + int(x) for x in salt])


LAST_COUNTS = (1, 2, 3, 63, 65, 511, 512, 513, 1025)


def last_tile_staged(n):
    """n keys of 1-40 B: the last tile holds 1, 2, 3, 63, 65, 511 or 512 keys."""
    return _rng(1, n).integers(1, 41, n), 3, 1


def last_tile_long(n):
    """The same n with keys of 150-400 B.  A tile of these exceeds the stage only from about 270
    keys on, so n >= 511 gives oversize tiles (with a partial last 64-key group for 511) and the
    smaller n, and the one-key last tiles of 513 and 1025, stay staged; last_tile_oversize
    carries every count into the oversize path."""
    return _rng(2, n).integers(150, 401, n), 3, 1


def last_tile_oversize(n):
    """last_tile_long with the middle key of the last tile grown to kStageBytes + 1 bytes, so that
    the last tile is oversize at every count: partial 64-key groups, and waves with no group
    when it holds fewer than 193 keys."""
    L = _rng(2, n).integers(150, 401, n)
    cnt = n - (n - 1) // TK * TK
    L[n - cnt + cnt // 2] = STAGE + 1
    return L, 3, 1


STAGE_EDGES = (-1, 0, 1)
STAGE_DELTAS = {0: (0, 0), 1: (1, 0), 15: (12, 3)}  # delta -> (shift, first_offset)


def stage_boundary(edge, delta):
    """A full tile whose span (key bytes + delta) is kStageBytes + edge, its last key ending at
    the span's last byte, then a short second tile."""
    shift, first = STAGE_DELTAS[delta]
    rng = _rng(3, edge + 1, delta)
    mean = STAGE // TK
    L = rng.integers(mean - 40, mean + 41, TK)
    diff = STAGE + edge - delta - int(L.sum())  # spread evenly: the key bytes sum to the target
    L += diff // TK
    L[:diff % TK] += 1
    assert L.min() >= 1
    return np.concatenate([L, rng.integers(1, 41, 20)]), first, shift


SLACK_LENGTHS = tuple(range(16, 0, -1)) + tuple(range(17, 33))
SLACK_PLACES = {(0, 0): 0, (0, 3): 13, (7, 0): 7, (7, 3): 4, (15, 0): 15, (15, 3): 12}  # (delta, first) -> shift


def front_slack(r, delta, first):
    """One tile of the 32 lengths 16..1, 17..32 rotated so that length r comes first: with
    p > 0 chunk 0 of that key starts below the tile's first staged byte."""
    return np.array(SLACK_LENGTHS[r:] + SLACK_LENGTHS[:r]), first, SLACK_PLACES[(delta, first)]


PARITY_PAIRS = tuple((a, b) for a in range(1, 5) for b in range(a, 5))


def switch_parities():
    """Ten full tiles, tile (a, b) with 256 keys of a chunks and 256 of b chunks in mixed
    order and with mixed pads: every lane walks (k0, k1) = (a, b)."""
    rng = _rng(4)
    out = []
    for a, b in PARITY_PAIRS:
        k = np.array([a] * (TK // 2) + [b] * (TK // 2))
        rng.shuffle(k)
        out.append(16 * k - rng.integers(0, 16, TK))
    return np.concatenate(out), 5, 2


SMALL_WALKS = {"k1": (9,), "k2": (23,), "k1k1": (16, 1)}


def small_walk(name):
    """cnt = 1 with one and with two chunks (T = 1, T = 2 without a switch), cnt = 2 with
    (1, 1) (T = 2, the switch at the only step)."""
    return np.array(SMALL_WALKS[name]), 7, 3


def empty_tile_between():
    """A tile of 512 empty keys (oN == o0: no DMA) between two non-empty tiles."""
    rng = _rng(5)
    return np.concatenate([rng.integers(1, 41, TK), np.zeros(TK, np.int64), rng.integers(1, 41, 100)]), 1, 5


def lone_byte(pos):
    """A tile that is empty but for one 1-byte key at position pos."""
    L = np.zeros(TK, np.int64)
    L[pos] = 1
    return L, 9, 2


def mostly_empty():
    """300 empty keys and 212 keys of 1-64 B in one tile: only_b lanes, and lanes whose two
    keys are both empty."""
    rng = _rng(6)
    L = np.concatenate([np.zeros(300, np.int64), rng.integers(1, 65, TK - 300)])
    rng.shuffle(L)
    return L, 0, 9


GIANT = 70000


def giant_staged(pos):
    """511 keys of 0-8 B and one key of 70 000 B (4375 chunks: an octave class) at tile
    position pos; the span stays below the stage."""
    L = _rng(7, pos).integers(0, 9, TK)
    L[pos] = GIANT
    return L, 4, 6


FILLER = 80000
RING_K = (0, 1, 8, 9, 16, 17, 24, 25)


def ring_rounds(per_k):
    """A tile made oversize by one 80 000-B key, its other keys with 0, 1, 8, 9, 16, 17, 24 and
    25 chunks (0 to 4 rounds of 8) interleaved, per_k of each.  per_k = 5: 41 keys, one group
    with empties, five round counts and 23 idle lanes, three waves without a group; per_k = 24:
    193 keys, four groups, the last one key and 63 idle lanes."""
    rng = _rng(8, per_k)
    L = [max(0, 16 * k - int(rng.integers(0, 16))) if k else 0 for _ in range(per_k) for k in RING_K]
    L.insert(len(L) // 2, FILLER)
    return np.array(L), 3, 11


RING_MIS = (0, 112, 113, 127)
RING_MIS_K = (1, 8, 9, 16, 17, 24, 25)
RING_MIS_P = (0, 1, 15)


def ring_mis():
    """An oversize tile whose keys sit at chosen places of their 128-byte lines: for every
    k, pad p and mis = (key_end - 16 k) & 127 of the three tuples above one key, each behind a
    spacer key of 0-127 B that moves its start to (mis + p) & 127.  mis >= 113 with k >= 9
    reads through the ring's 16-byte mirror; mis + p >= 128 puts the key's first byte in line
    1 (first = 1, only pad in line 0)."""
    first, shift = 6, 21
    L, pos = [FILLER], shift + first + FILLER
    for k in RING_MIS_K:
        for p in RING_MIS_P:
            for mis in RING_MIS:
                spacer = (mis + p - pos) % 128
                L += [spacer, 16 * k - p]
                pos += spacer + 16 * k - p
    return np.array(L), first, shift


STRADDLE = 1 << 32
STRADDLE_TAIL = 512 << 10   # written bytes: the last 512 KiB of a buffer of 2^32 + 256 KiB


def straddle(kind):
    """One full tile that contains byte offset 2^32 of its buffer: staged (1-40 B keys) or
    oversize (150-400 B keys).  buffer_shift is 0; the buffer is the straddle test's own."""
    rng = _rng(9, kind == "oversize")
    L = rng.integers(1, 41, TK) if kind == "staged" else rng.integers(150, 401, TK)
    return L, STRADDLE - int(L[:TK // 2].sum()) - 3, 0


def scenarios():
    """name -> (lengths, first_offset, buffer_shift) for every row but the 2^32 straddle."""
    s = {}
    for n in LAST_COUNTS:
        s[f"last-staged-{n}"] = last_tile_staged(n)
        s[f"last-long-{n}"] = last_tile_long(n)
        s[f"last-oversize-{n}"] = last_tile_oversize(n)
    for edge in STAGE_EDGES:
        for delta in STAGE_DELTAS:
            s[f"stage{edge:+d}-delta{delta}"] = stage_boundary(edge, delta)
    s["parities"] = switch_parities()
    for name in SMALL_WALKS:
        s[f"walk-{name}"] = small_walk(name)
    s["empty-tile-between"] = empty_tile_between()
    for pos in (0, TK // 2 - 1, TK - 1):
        s[f"lone-byte-{pos}"] = lone_byte(pos)
    s["mostly-empty"] = mostly_empty()
    for pos in (0, TK // 2 - 1, TK - 1):
        s[f"giant-{pos}"] = giant_staged(pos)
    s["ring-rounds-5"] = ring_rounds(5)
    s["ring-rounds-24"] = ring_rounds(24)
    s["ring-mis"] = ring_mis()
    return s


# ----------------------------------------------------------------------------- device side
def place(cuda, payload, shift, canary):
    """payload (uint8 array) as a device buffer that starts `shift` bytes into a 128-aligned
    place of its allocation and ends at the payload's last byte, PAD canary bytes before
    (plus the shift) and after."""
    import torch
    a = np.full(PAD + shift + payload.size + PAD, canary, np.uint8)
    a[PAD + shift:PAD + shift + payload.size] = payload
    t = torch.from_numpy(a).to(cuda)
    assert t.data_ptr() % 128 == 0, "device allocations are expected 128-aligned"
    return t[PAD + shift:PAD + shift + payload.size]


def sentinel_outs(torch, cuda, n, names):
    """Sentinel-filled int64 outputs of n entries, each the head of a tensor 64 entries longer."""
    full = {k: torch.full((n + 64,), SENTINEL, dtype=torch.int64, device=cuda) for k in names}
    return full, {k: v[:n] for k, v in full.items()}


def collect(torch, full, n):
    torch.cuda.synchronize()
    got = {}
    for k, v in full.items():
        a = v.cpu().numpy().view(np.uint64)
        assert (a[n:] == np.uint64(SENTINEL)).all(), f"{k}: written past entry n"
        got[k] = a[:n]
    return got


def run_csr(cuda, buf, off, arm, std_fnv=False):
    """One output arm of k2h_amd_hash_csr / _index over buf; host uint64 arrays by name."""
    import torch

    from k2hash_amd import batch
    n = off.size - 1
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.int64)).to(cuda)
    names = {"h1": ("h1",), "h1h2": ("h1", "h2"), "index": ("h1", "h2", "kindex", "ckindex")}[arm]
    full, o = sentinel_outs(torch, cuda, n, names)
    if arm == "index":
        batch.hash_csr_index(buf, d_off, CUR_MASK, COL_MASK, second=True, std_fnv=std_fnv,
                             out=(o["h1"], o["h2"], o["kindex"], o["ckindex"]))
    else:
        batch.hash_csr(buf, d_off, second=arm == "h1h2", std_fnv=std_fnv, out=(o["h1"], o.get("h2")))
    return collect(torch, full, n)


def run_fixed(cuda, buf, key_len, arm, std_fnv=False):
    """One output arm of k2h_amd_hash_fixed / _index over buf."""
    import torch

    from k2hash_amd import batch
    n = buf.numel() // key_len
    names = {"h1": ("h1",), "h1h2": ("h1", "h2"), "index": ("h1", "h2", "kindex", "ckindex")}[arm]
    full, o = sentinel_outs(torch, cuda, n, names)
    if arm == "index":
        batch.hash_fixed_index(buf, key_len, CUR_MASK, COL_MASK, second=True, std_fnv=std_fnv,
                               out=(o["h1"], o["h2"], o["kindex"], o["ckindex"]))
    else:
        batch.hash_fixed(buf, key_len, second=arm == "h1h2", std_fnv=std_fnv, out=(o["h1"], o.get("h2")))
    return collect(torch, full, n)


def expect(oracle, r1, r2, arm):
    """The oracle's values for an arm's outputs, from the oracle's own h1 / h2."""
    want = {"h1": r1}
    if arm != "h1":
        want["h2"] = r2
    if arm == "index":
        want["kindex"], want["ckindex"] = oracle.bucket_index(r1, CUR_MASK, COL_MASK)
    return want


def assert_equal(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (what, k, f"{bad.size} of {want[k].size} differ, first at key {int(bad[0])}: "
                               f"{int(got[k][bad[0]]):#x} != {int(want[k][bad[0]]):#x}")
