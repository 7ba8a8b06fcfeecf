"""k2h_amd_ralledata_index, _find and _fetch with byte offset 2^32 inside the stream, inside the
query keys and inside what fetch writes (the techniques of big_offsets.py).

* find: one big buffer, the stream at base 0 and the keys at base GAP, each across ITS OWN offset
  2^32 inside the written tail.  Side.koff = b + kpos, blobs + blob_off[found] with the attrs walk
  behind it, keys + e - 16 k of the hash kernel and keys + b of the compare all pass 2^32.  The
  buffer's first HEAD bytes hold canary bytes, so an offset cut to 32 bits reads canaries.
* fetch, source: a segment of the stream that straddles the line, moved by a slot's 16 lanes or by
  the whole block.
* fetch, output (ballast): `which` repeats one blob whose value is half a MiB until the slots total
  2048 bytes less than 2^32; out_off passes the line inside a tail slot.

Expected values come from ralle_find_model.find_model and fetch_model over the small byte strings at
offsets from 0, and from closed forms for the ballast."""
import ctypes
import struct

import numpy as np
import pytest

import big_offsets as bo
import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_find_model as fm
import ralle_times_model as tm
from big_offsets import BIG, CANARY, GAP, LINE, TAIL0
from ralle_find_model import ATTRS, EXPIRED, FOUND, NONE, PART

from k2hash_amd import _native

NOW = tm.NOW
M32 = (1 << 32) - 1
HEAD = 2 * GAP           # canary bytes at the big buffer's start: where offsets cut to 32 bits point
LINE_BLOB, DUP_FIRST, DUP_LAST, DEAD, LIVE = 5, 1, 9, 7, 8
LINE_QUERY = 3
KINDS = ("group", "wave")


# ------------------------------------------------------------------------ find: the scenario
def find_scenario(oracle, cstr):
    """14 blobs, blob 5 with the stream's offset 2^32 23 bytes into its 57-byte key (four compare
    chunks); one identity at blob 1 (below the line) and again at blob 9 (above it); blob 7, above
    the line, with attrs that have expired at NOW and blob 8 with attrs that have not.  12 queries
    from the keys' base pointer, query 3 -- the key of blob 5 -- with the keys' own offset 2^32 7
    bytes into it and eight queries wholly above.  cstr: the stream stores key + NUL, the queries
    are the bare strings.  Returns a dict: the small byte strings with offsets from 0 (buf, off, keys,
    koff), their places in the big buffer (first, kfirst), the hashes and the image."""
    rng = np.random.default_rng(70 + cstr)
    rb = lambda k: bytes(rng.integers(1, 256, k, dtype=np.uint8))  # noqa: E731  (no NUL inside a key)
    names = [b"k%02d-" % i + rb(4 + 3 * i) for i in range(14)]
    names[LINE_BLOB] = b"the-line-runs-through-this-key-" + rb(26)
    names[DUP_LAST] = names[DUP_FIRST]
    names[DEAD], names[LIVE] = b"expired-above-the-line", b"alive-above-the-line-" + rb(20)
    vals = [b"value-%02d-" % i + rb(5 * i) for i in range(14)]
    attrs = [b""] * 14
    attrs[DEAD], attrs[LIVE], attrs[2] = tm.ATTRS_KINDS["m950-expired"], tm.ATTRS_KINDS["m950-live"], tm.ATTRS_KINDS["expired-only"]
    stored = [k + b"\0" for k in names] if cstr else names
    blobs = dm.at_odd_offsets(dm.blobs_of(oracle, stored, vals, None, attrs), seed=3)
    buf, off = rm.join(blobs)
    first = LINE - off[LINE_BLOB] - rm.get(buf, off[LINE_BLOB], rm.F_KPOS) - 23
    queries = [names[DUP_FIRST], names[0], b"absent-below", names[LINE_BLOB], names[DEAD], names[LIVE], names[DUP_LAST],
               names[2], names[12], b"absent-above-the-line-" + rb(30), names[LINE_BLOB][:-1] + b"?", names[13]]
    keys, koff = fm.csr(queries)
    kfirst = LINE - int(koff[LINE_QUERY]) - 7
    h1, h2 = fm.hashes_of(oracle, queries, 0, cstr)
    img = bo.image([(first, buf), (GAP + kfirst, keys)])
    return dict(buf=bytes(buf), off=off, first=first, keys=keys, koff=koff, kfirst=kfirst, h1=h1, h2=h2, img=img,
                queries=queries, cstr=cstr)


def find_wants(s, now):
    return fm.find_model(s["buf"], s["off"], s["keys"], s["koff"], s["h1"], s["h2"], cstr=s["cstr"], now=now)


def _in_head(at, length):
    """[at, at + length) cut to 32 bits lies in the canary head."""
    return 0 <= (at & M32) and (at & M32) + length <= HEAD


@pytest.mark.parametrize("cstr", [False, True])
def test_find_scenario_holds_the_line_in_stream_and_keys(oracle, cstr):
    s = find_scenario(oracle, cstr)
    buf, off, first, koff, kfirst = s["buf"], s["off"], s["first"], [int(x) for x in s["koff"]], s["kfirst"]
    f = [struct.unpack_from("<10Q", buf, o) for o in off[:-1]]
    absolute = [first + o for o in off]
    # the stream's line lies inside the key of blob 5, a key of four compare chunks
    k0 = absolute[LINE_BLOB] + f[LINE_BLOB][6]
    assert bo.holds_line(k0, k0 + f[LINE_BLOB][2]) and k0 + 23 == LINE and f[LINE_BLOB][2] >= 57
    match, status, hit, counts = find_wants(s, NOW)
    assert match[LINE_QUERY] == LINE_BLOB and status[LINE_QUERY] == PART | FOUND
    assert status[10] == PART                                     # the same key but for its last byte: a miss
    # the last copy, not the first, is above the line
    assert absolute[DUP_FIRST + 1] < LINE < absolute[DUP_LAST] and match[0] == match[6] == DUP_LAST
    assert buf[off[DUP_FIRST] + f[DUP_FIRST][7]:][:8] != buf[off[DUP_LAST] + f[DUP_LAST][7]:][:8]   # another value
    # a match above the line whose attrs expire: blob_off[found] + attrs_pos is past 2^32
    assert absolute[DEAD] + f[DEAD][9] > LINE and status[4] == PART | FOUND | ATTRS | EXPIRED
    assert absolute[LIVE] + f[LIVE][9] > LINE and status[5] == PART | FOUND | ATTRS
    assert status[7] == PART | FOUND | ATTRS | EXPIRED and absolute[3] < LINE       # and one below it
    assert counts == [12, 9, 2] and find_wants(s, None)[3] == [12, 9, 0]
    # the keys' own line lies inside query 3; eight queries lie wholly above it
    ka = [kfirst + x for x in koff]
    assert bo.holds_line(ka[LINE_QUERY], ka[LINE_QUERY + 1]) and ka[LINE_QUERY] + 7 == LINE
    assert ka[LINE_QUERY - 1] < LINE and all(x > LINE for x in ka[LINE_QUERY + 1:]) and len(ka) - 2 - LINE_QUERY == 8
    # both fit the written tail without touching each other
    assert TAIL0 <= first and absolute[-1] < GAP + ka[0] and GAP + ka[-1] <= BIG
    # every offset above a line, cut to 32 bits, points into the canary head, where no key is: a kernel
    # that truncates Side.koff, blob_off[found] or key_off compares against canaries or parses them as attrs
    for i in range(LINE_BLOB + 1, 14):
        assert _in_head(absolute[i] + f[i][6], f[i][2]) and _in_head(absolute[i] + f[i][9], f[i][5])
        assert bytes([CANARY]) * f[i][2] != buf[off[i] + f[i][6]:off[i] + f[i][6] + f[i][2]]
    for i in range(LINE_QUERY + 1, 12):
        assert _in_head(GAP + ka[i], ka[i + 1] - ka[i])
    assert tm.parse_attrs(bytes([CANARY]) * len(tm.ATTRS_KINDS["m950-expired"])) == ({}, True)   # canaries never expire


# ----------------------------------------------------------------- fetch: source across the line
FETCH_N, FETCH_LINE_BLOB = 10, 4


def fetch_scenario(oracle, kind, segment):
    """10 blobs with all four segments; the `segment` of blob 4 has 300 bytes ("group": the slot's 16
    lanes) or 6,000 ("wave": kFetchBig and more, the whole block) and the line a third of its length
    and 5 bytes into it.  Returns (bytes, offsets from 0, first, which)."""
    rng = np.random.default_rng(80 + KINDS.index(kind))
    rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))  # noqa: E731
    cols = {name: [rb(10 + 7 * i) for i in range(FETCH_N)] for name in fm.SEGS}
    long_ = 6000 if kind == "wave" else 300
    cols[segment][FETCH_LINE_BLOB] = rb(long_)
    blobs = dm.at_odd_offsets(dm.blobs_of(oracle, cols["key"], cols["value"], cols["subkeys"], cols["attrs"]), seed=4)
    buf, off = rm.join(blobs)
    pos = rm.get(buf, off[FETCH_LINE_BLOB], rm.F_KPOS + 8 * fm.SEGS.index(segment))
    first = LINE - off[FETCH_LINE_BLOB] - pos - (long_ // 3 + 5)
    which = np.array([FETCH_LINE_BLOB, 0, FETCH_LINE_BLOB, 9, NONE, 3, 5, FETCH_LINE_BLOB, 8], np.uint64)
    return bytes(buf), off, first, which


@pytest.mark.parametrize("segment", ["value", "attrs"])
@pytest.mark.parametrize("kind", KINDS)
def test_fetch_scenario_holds_the_line_in_the_segment(oracle, kind, segment):
    buf, off, first, which = fetch_scenario(oracle, kind, segment)
    s = fm.SEGS.index(segment)
    f = struct.unpack_from("<10Q", buf, off[FETCH_LINE_BLOB])
    a = first + off[FETCH_LINE_BLOB] + f[6 + s]
    assert bo.holds_line(a, a + f[2 + s]) and (f[2 + s] >= 4096) == (kind == "wave") and LINE - a == f[2 + s] // 3 + 5
    assert TAIL0 <= first and first + off[-1] <= BIG and first + off[FETCH_LINE_BLOB + 1] > LINE
    data, ooff, bad = fm.fetch_model(buf, off, which, segment)
    assert not bad.any() and len(data) > 3 * f[2 + s]


# ---------------------------------------------------------------- fetch: output across the line
class FetchBallast:
    """Blob 0 with an 8-byte key and a value of VAL bytes (generated on the device), asked for NB
    times: the ballast slots end 2048 bytes below the line.  Then 12 tail blobs and 9 tail slots;
    the third tail slot -- 3,000 bytes ("group") or 6,000 ("wave") -- holds the line."""
    NB = 8192 - 64
    VAL = (LINE - 2048) // NB
    KEY = 8
    BLOB0 = rm.HEADER + KEY + VAL

    def __init__(self, oracle, kind):
        assert self.NB * self.VAL == LINE - 2048
        rng = np.random.default_rng(90 + KINDS.index(kind))
        rb = lambda k: bytes(rng.integers(0, 256, k, dtype=np.uint8))  # noqa: E731
        vals = [rb(40 + 11 * i) for i in range(12)]
        vals[0], vals[1], vals[2], vals[7] = rb(1000), rb(700), rb(6000 if kind == "wave" else 3000), rb(4096)
        blobs = dm.at_odd_offsets(dm.blobs_of(oracle, [b"tail-%02d" % i for i in range(12)], vals), seed=5)
        self.tail, toff = rm.join(blobs)
        self.head = struct.pack("<10Q", 0, 0, self.KEY, self.VAL, 0, 0, rm.HEADER, rm.HEADER + self.KEY, self.BLOB0, self.BLOB0)
        self.off = [0] + [self.BLOB0 + x for x in toff]
        self.n, self.size = 13, self.BLOB0 + len(self.tail)
        self.tail_which = np.array([1, 2, 3, NONE, 8, 3, 12, 5, 1], np.uint64)
        self.which = np.concatenate([np.zeros(self.NB, np.uint64), self.tail_which])
        self.m = self.which.size
        # the tail's bytes and offsets from the model over the tail alone (its blob i is blob i + 1)
        shifted = np.where(self.tail_which == NONE, NONE, self.tail_which - np.uint64(1))
        self.tail_bytes, tail_off, bad = fm.fetch_model(self.tail, toff, shifted, "value")
        assert not bad.any()
        self.ballast_bytes = self.NB * self.VAL
        self.out_off = np.concatenate([np.arange(self.NB, dtype=np.uint64) * np.uint64(self.VAL),
                                       tail_off + np.uint64(self.ballast_bytes)])
        self.total = self.ballast_bytes + len(self.tail_bytes)


@pytest.mark.parametrize("kind", KINDS)
def test_fetch_ballast_crosses_the_line_in_a_tail_slot(oracle, kind):
    s = FetchBallast(oracle, kind)
    assert s.NB * s.VAL == LINE - 2048 == s.ballast_bytes and s.total > LINE and s.out_off.size == s.m + 1
    lo, hi = int(s.out_off[s.NB + 2]), int(s.out_off[s.NB + 3])
    assert bo.holds_line(lo, hi) and (hi - lo >= 4096) == (kind == "wave") and min(LINE - lo, hi - LINE) > 300
    assert rm.header_status(s.head + bytes(8), 0, s.BLOB0, s.BLOB0)[0] == rm.OK and len(s.head) == rm.HEADER
    assert s.off[-1] == s.size and int(s.out_off[-1]) == s.total
    assert sum(1 for i in range(s.NB, s.m) if s.out_off[i] > LINE) == 6            # slots wholly above the line


# ------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def device_memory(cuda):
    """What these tests free stays with torch's caching allocator until the module ends."""
    import torch
    yield
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big(cuda, device_memory):
    t = bo.big_buffer(cuda)
    t[:HEAD] = CANARY
    yield t
    del t


@pytest.mark.gpu
@pytest.mark.parametrize("cstr", [False, True])
def test_find_stream_and_keys_cross_the_line(cuda, oracle, big, cstr):
    """Hashes passed and computed, with and without `now`; the index built from absolute offsets."""
    s = find_scenario(oracle, cstr)
    bo.load_tail(big, s["img"])
    n, m = len(s["off"]) - 1, len(s["koff"]) - 1
    off = [s["first"] + x for x in s["off"]]
    koff = s["koff"] + np.uint64(s["kfirst"])
    index, parts, doff = fm.run_index(cuda, big, BIG, off)
    assert parts == n
    flags = _native.K2H_AMD_FLAG_CSTR if cstr else 0
    for now in (None, NOW):
        want = find_wants(s, now)
        for name, h1, h2 in (("passed", s["h1"], s["h2"]), ("computed", None, None)):
            got = fm.run_find(cuda, big, BIG, doff, n, index, big[GAP:], BIG - GAP, koff, h1, h2, flags, now)
            fm.assert_found(got, want, f"across 2^32, cstr {cstr}, now {now}, hashes {name}")
    assert m == 12


@pytest.mark.gpu
@pytest.mark.parametrize("segment", ["value", "attrs"])
@pytest.mark.parametrize("kind", KINDS)
def test_fetch_source_crosses_the_line(cuda, oracle, big, kind, segment):
    import torch
    buf, off, first, which = fetch_scenario(oracle, kind, segment)
    bo.load_tail(big, bo.image([(first, buf)]))
    want = fm.fetch_model(buf, off, which, segment)
    doff = torch.tensor([first + x for x in off], dtype=torch.int64, device=cuda)
    rc, data, ooff, bad, total = fm.run_fetch(cuda, big, BIG, doff, len(off) - 1, which, segment)
    assert rc == 0 and total == len(want[0]) and (ooff == want[1]).all() and not bad.any()
    assert data == want[0], f"fetch of {segment} across 2^32 ({kind}): bytes differ"


def _all_equal(t, value, step=256 << 20):
    """Whether every byte of the device tensor is `value`, a piece at a time."""
    return all(bool((t[a:a + step] == value).all()) for a in range(0, t.numel(), step))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_fetch_output_crosses_the_line(cuda, oracle, device_memory, kind):
    """out_off passes 2^32 inside the third tail slot; six slots lie wholly above it.  First with
    out_cap one byte short: K2H_AMD_EINVAL, *total right, out untouched."""
    import torch

    from k2hash_amd import batch
    s = FetchBallast(oracle, kind)
    lib = _native.batch_lib()
    inp = batch.synth_bytes(s.size, cuda, byte_off=5151)
    inp[:rm.HEADER] = torch.from_numpy(np.frombuffer(s.head, np.uint8).copy()).to(cuda)
    inp[s.BLOB0:] = torch.from_numpy(np.frombuffer(bytes(s.tail), np.uint8).copy()).to(cuda)
    d_off = torch.tensor(s.off, dtype=torch.int64, device=cuda)
    d_which = torch.from_numpy(s.which.view(np.int64)).to(cuda)
    whole, out = bo.guarded(torch, cuda, s.total, shift=7)
    bw, bad = bo.guarded(torch, cuda, s.m, fill=0xEE)
    total = ctypes.c_uint64(77)

    def call(cap, ooff):
        return lib.k2h_amd_ralledata_fetch(bo._p(inp), s.size, bo._p(d_off), s.n, bo._p(d_which), s.m, None, 1, bo._p(out), cap,
                                           bo._p(ooff), bo._p(bad), ctypes.byref(total), bo._stream())
    try:
        full, ooff = bo.sentinel_words(torch, cuda, s.m + 1)
        rc = call(s.total - 1, ooff)
        torch.cuda.synchronize()
        assert rc == _native.K2H_AMD_EINVAL and int(total.value) == s.total
        assert _all_equal(whole, bo.OUT_FILL), "out_cap one byte short: out written"
        full, ooff = bo.sentinel_words(torch, cuda, s.m + 1)
        total.value = 77
        _native.check(call(s.total, ooff))
        torch.cuda.synchronize()
        assert int(total.value) == s.total
        assert np.array_equal(bo.words_back(torch, full, s.m + 1, "out_off"), s.out_off)
        assert bo.guards_intact(torch, whole, out), "bytes outside out written"
        assert bo.guards_intact(torch, bw, bad, 0xEE) and not bad.any()
        value = inp[rm.HEADER + s.KEY:s.BLOB0]
        assert bo.rows_equal(torch, out[:s.ballast_bytes].view(s.NB, s.VAL), value.unsqueeze(0).expand(s.NB, s.VAL), rows=512)
        got = out[s.ballast_bytes:].cpu().numpy()
        diff = np.flatnonzero(got != np.frombuffer(s.tail_bytes, np.uint8))
        assert diff.size == 0, f"{diff.size} tail bytes differ, first at {int(diff[0])}"
    finally:
        del whole, out, inp
