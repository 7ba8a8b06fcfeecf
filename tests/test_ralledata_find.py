"""Keys looked up in a held RALLEDATA stream (include/k2hash_amd.h section 4e: k2h_amd_ralledata_index,
_find and _fetch; k2h_ralledata_find.hip) against the model of ralle_find_model.py, entry for entry
and byte for byte.

The planted stream is deterministic and every blob in it is there for one reason:

* dup: three copies of a key apart from each other, each with another value: the last one is
  the match;
* step: a later blob that shares the true match's stored hash (or only its sorted low bits)
  without sharing its identity -- other subhash, other key of the same length, other key length,
  other high hash bit;
* brk: the would-be last copy takes no part (masked, bad span, no key, key range outside) or takes
  part under another identity (wrong stored hash), so the earlier copy is the match;
* exp: every kind of attrs of ralle_times_model, and two keys whose copies differ in expiry.

A second, smaller plant (_ones_plant) puts stored hashes of all ones -- in the 16 sorted bits, and ~0
itself -- at the end of the participants' sorted column, next to the pairs of four non-participants.

Keys run from 9 to 57 bytes, one to four 16-byte chunks of the compare.  The CPU tests state why
a device test on this stream cannot pass for the wrong reason: the model's lookup is "feed the
blobs in order, the last one wins", and every blob the kernel must not choose would have given
another answer.  Expected values never come from a device call; every device output is
sentinel-filled and guarded, and the inputs stand at odd shifts from a 16-byte boundary between
canaries.
"""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_find_model as fm
import ralle_times_model as tm
import test_ralledata_diff_held as dh
from ralle_find_model import ATTRS, BAD_INDEX, EXPIRED, FOUND, NONE, PART

from k2hash_amd import _native

CS = (0, 2, 7, 12, 23, 30, 39, 40)           # key_of's c: keys of one to four 16-byte chunks under every prefix
VARIANTS = dh.VARIANTS
NOW = tm.NOW
_CACHE = {}


def _value(i):
    return b"value-%05d-" % i + b"v" * (i % 23)


def _planted(oracle):
    """(blobs, consider, queries, info).  info: dup[key] = (first, second, last), step[key] =
    (match, decoy, variant), brk[key] = (match, broken copy, how), exp[key] = (copies, kinds)."""
    keys, attrs = [], []

    def add(key, a=b""):
        keys.append(key)
        attrs.append(a)
        return len(keys) - 1
    info = dict(dup={}, step={}, brk={}, exp={})
    first, second = {}, {}
    for c in CS:                                                              # round A
        first[c] = add(dh.key_of(b"dup-key", c))
        for v in range(len(VARIANTS)):
            info["step"][dh.key_of(b"step%d" % v, c)] = [add(dh.key_of(b"step%d" % v, c)), None, v]
        for w, how in enumerate(dh.BREAKS):
            info["brk"][dh.key_of(b"brk%d" % w, c)] = [add(dh.key_of(b"brk%d" % w, c)), None, how]
    for kind, a in tm.ATTRS_KINDS.items():
        info["exp"][b"exp-" + kind.encode()] = ([add(b"exp-" + kind.encode(), a)], [kind])
    mix = {b"exp-mix-dead-then-live": ("expired-only", "m950-live"), b"exp-mix-live-then-dead": ("m950-live", "expired-only")}
    for k, (x, _y) in mix.items():
        info["exp"][k] = ([add(k, tm.ATTRS_KINDS[x])], [x])
    for c in CS:                                                              # round B
        second[c] = add(dh.key_of(b"dup-key", c))
    for c in CS:                                                              # round C: the copies behind
        info["dup"][dh.key_of(b"dup-key", c)] = (first[c], second[c], add(dh.key_of(b"dup-key", c)))
        for v in range(len(VARIANTS)):
            k = dh.key_of(b"step%d" % v, c)
            other = k[:-1] + b"~" if v == 1 else k + b"-longer" if v == 2 else k
            info["step"][k][1] = add(other, tm.ATTRS_KINDS["expired-only"] if c % 2 else b"")
        for w in range(len(dh.BREAKS)):
            k = dh.key_of(b"brk%d" % w, c)
            info["brk"][k][1] = add(k)
    for k, (_x, y) in mix.items():
        info["exp"][k][0].append(add(k, tm.ATTRS_KINDS[y]))
        info["exp"][k][1].append(y)
    n = len(keys)
    blobs = dm.blobs_of(oracle, keys, [_value(i) for i in range(n)], None, attrs)
    consider = np.ones(n, np.uint8)
    for k, (x, d, v) in info["step"].items():
        h, s = rm.get(blobs[x], 0, rm.F_HASH), rm.get(blobs[x], 0, rm.F_SUBHASH)
        dm.set_hash(blobs[d], h ^ (1 << 63) if v == 3 else h, s ^ 1 if v == 0 else s)
    whole = {k: bytearray(blobs[d]) for k, (_x, d, _how) in info["brk"].items()}
    for k, (_x, d, how) in info["brk"].items():
        blobs[d] = dh.broken(blobs[d], how)
        if how == "masked":
            consider[d] = 0
    info["whole"] = whole
    queries = list(info["dup"]) + list(info["step"]) + list(info["brk"]) + list(info["exp"]) + \
        [dh.key_of(b"miss", c) for c in CS]
    return blobs, consider, queries, info


def planted(oracle):
    if "planted" not in _CACHE:
        _CACHE["planted"] = _planted(oracle)
    return _CACHE["planted"]


def _model(oracle, blobs, consider, queries, now=None, cstr=False):
    buf, off = rm.join(blobs)
    data, koff = fm.csr(queries)
    h1, h2 = fm.hashes_of(oracle, queries, 0, cstr)
    return fm.find_model(buf, off, data, koff, h1, h2, cstr=cstr, now=now, consider=consider), (buf, off, h1, h2)


def _val(blob):
    f = np.frombuffer(bytes(blob[:rm.HEADER]), "<u8")
    return bytes(blob[int(f[7]):int(f[7]) + int(f[3])])


# ------------------------------------------------------------------------------------- CPU
def test_model_lookup_is_last_one_wins(oracle):
    """The model's scan agrees with a dict built by feeding the participants in order."""
    blobs, consider, queries, _info = planted(oracle)
    (match, status, hit, counts), (buf, off, h1, h2) = _model(oracle, blobs, consider, queries)
    table = fm.last_wins(buf, off, consider=consider)
    for q, k in enumerate(queries):
        want = table.get((int(h1[q]), int(h2[q]), k))
        assert (match[q] == NONE) == (want is None) and (want is None or match[q] == want), k
        assert bool(status[q] & FOUND) == (want is not None) and status[q] & PART
    assert counts[0] == len(queries) and counts[1] == len(queries) - len(CS) and counts[2] == 0
    assert hit.sum() == counts[1] and set(np.nonzero(hit)[0]) <= set(table.values())


def test_every_decoy_would_answer_otherwise(oracle):
    blobs, consider, queries, info = planted(oracle)
    (match, status, _hit, _c), (_buf, _off, h1, _h2) = _model(oracle, blobs, consider, queries, now=NOW)
    at = {k: q for q, k in enumerate(queries)}
    chunks = set()
    for k, (a, b, last) in info["dup"].items():                      # an earlier copy: another index and value
        assert match[at[k]] == last and a < b < last and b - a > 1 and last - b > 1
        assert len({_val(blobs[a]), _val(blobs[b]), _val(blobs[last])}) == 3
        chunks.add(dh.chunks(blobs[last]))
    assert chunks == {1, 2, 3, 4}
    for k, (x, d, v) in info["step"].items():                        # the later blob the walk steps over
        assert match[at[k]] == x and d > x and _val(blobs[d]) != _val(blobs[x])
        hx, hd = rm.get(blobs[x], 0, rm.F_HASH), rm.get(blobs[d], 0, rm.F_HASH)
        assert (hx == hd) == (v != 3) and (hx ^ hd) & 0xFFFFFFFFFFFF == 0 and hx == int(h1[at[k]])
        if dh.attrs_of(blobs[d]):                                     # the decoy expired, the match without attrs
            assert not status[at[k]] & (ATTRS | EXPIRED)
    for k, (x, d, how) in info["brk"].items():                       # unbroken, the later copy would be the match
        assert match[at[k]] == x and d > x, (k, how)
        mended = list(blobs)
        mended[d] = info["whole"][k]
        (m2, _s, _h, _c2), _ = _model(oracle, mended, None, [k])
        assert m2[0] == d and _val(info["whole"][k]) != _val(blobs[x]), (k, how)
    for k, (copies, kinds) in info["exp"].items():
        q = at[k]
        dead = [tm.is_expire(tm.ATTRS_KINDS[x], NOW) for x in kinds]
        assert match[q] == copies[-1] and bool(status[q] & EXPIRED) == dead[-1], k
        assert bool(status[q] & ATTRS) == bool(tm.ATTRS_KINDS[kinds[-1]])
        if len(copies) == 2:
            assert dead[0] != dead[1]                                # the earlier copy's attrs say the opposite
    assert sum(1 for q in range(len(queries)) if status[q] & EXPIRED) == 3


def test_invalid_queries_in_the_model():
    data = b"abcdefgh"
    koff = np.array([0, 3, 2, 5, 9, 4, 4, 8], np.uint64)               # ok, decreasing, ok, past the end, decreasing, empty, ok
    spans = [fm.query_span(koff, i, len(data), False) for i in range(7)]
    assert spans == [(0, 3), None, (2, 5), None, None, None, (4, 8)]
    assert fm.query_span(koff, 5, len(data), True) == (4, 4)


def test_fetch_model_slices(oracle):
    blobs, _consider, _q, _info = planted(oracle)
    buf, off = rm.join(blobs)
    which = [3, NONE, 3, len(blobs), 0]
    data, ooff, bad = fm.fetch_model(buf, off, which, "value", take=[1, 1, 1, 1, 0])
    assert data == _val(blobs[3]) * 2 and bad.tolist() == [0, 0, 0, 1, 0]
    assert ooff.tolist() == [0, len(_val(blobs[3])), len(_val(blobs[3])), len(data), len(data), len(data)]


def test_kernels_keep_the_register_budget(tmp_path):
    """Every kernel of k2h_ralledata_find.hip: no scratch, no spills; the find kernel at most 64
    VGPRs (8 waves per SIMD) and no LDS."""
    import test_archive_device as tad
    if not Path(tad.HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "k2h_ralledata_find.s"
    subprocess.run([tad.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    f"-I{tad.ROOT / 'include'}", str(tad.CSRC / "k2h_ralledata_find.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    kernels = {k: v for k, v in tad._kernel_meta(out.read_text()).items() if "ralledata_" in k or "ralle_compact" in k}
    for name in ("ralledata_index_gather_kernel", "ralledata_index_head_kernel", "ralle_compact_kernel",
                 "ralledata_find_hash_kernel", "ralledata_find_kernel", "ralledata_fetch_sizes_kernel",
                 "ralledata_fetch_copy_kernel"):
        assert any(name in k for k in kernels), (name, sorted(kernels))
    for sym, f in kernels.items():
        assert f.get("private_segment_fixed_size", 0) == 0, sym
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, sym
        assert f.get("vgpr_count", 999) <= 64, (sym, f.get("vgpr_count"))
        if "ralledata_find_kernel" in sym:
            assert f.get("group_segment_fixed_size", 0) == 0, sym
    assert sum(1 for k in kernels if "ralledata_find_kernel" in k) == 2     # plain and C string


def test_every_einval_without_a_device():
    """Judged on the host before any device is touched, each with its own message."""
    lib = _native.batch_lib()
    n, m = 2, 3
    blobs, off = np.zeros(200, np.uint8), np.arange(n + 1, dtype=np.uint64) * 100
    need = lib.k2h_amd_ralledata_index_size(n)
    raw = np.zeros(need + 512, np.uint8)
    at = (-raw.ctypes.data) % 256
    index = raw[at:at + need]
    keys, koff, h = np.zeros(30, np.uint8), np.arange(m + 1, dtype=np.uint64) * 10, np.zeros(m, np.uint64)
    status, which = np.full(m, 0xEE, np.uint8), np.zeros(m, np.uint64)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    msg = lambda: bytes(lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL))  # noqa: E731
    parts, total = ctypes.c_uint64(7), ctypes.c_uint64(7)
    counts = (ctypes.c_uint64 * 3)(7, 7, 7)
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))

    def index_args(**kw):
        d = dict(blobs=p(blobs), off=p(off), n=n, index=p(index), cap=need)
        d.update(kw)
        return d["blobs"], blobs.size, d["off"], d["n"], None, d["index"], d["cap"], ctypes.byref(parts), None
    texts = set()
    for kw, text in ((dict(blobs=None), b"NULL blobs"), (dict(off=None), b"NULL blob_off"), (dict(index=None), b"NULL index"),
                     (dict(cap=need - 1), b"index_cap"), (dict(index=ctypes.c_void_p(index.ctypes.data + 16)), b"256-byte aligned"),
                     (dict(n=(1 << 32) - 1), b"2^32 - 2")):
        parts.value = 7
        assert lib.k2h_amd_ralledata_index(*index_args(**kw)) == _native.K2H_AMD_EINVAL, kw
        assert text in msg() and msg().startswith(b"ralledata_index: ") and parts.value == 0, (kw, msg())
        texts.add(msg())
    assert len(texts) == 6

    def find_args(**kw):
        d = dict(blobs=p(blobs), off=p(off), n=n, index=p(index), keys=p(keys), koff=p(koff), m=m, h1=p(h), h2=p(h), flags=0,
                 status=p(status))
        d.update(kw)
        return (d["blobs"], blobs.size, d["off"], d["n"], d["index"], d["keys"], keys.size, d["koff"], d["m"], d["h1"],
                d["h2"], d["flags"], None, None, d["status"], None, cp, None)
    texts = set()
    for kw, text in ((dict(status=None), b"NULL status"), (dict(keys=None), b"NULL keys"), (dict(koff=None), b"NULL key_off"),
                     (dict(index=None), b"NULL index"), (dict(blobs=None), b"NULL blobs"), (dict(off=None), b"NULL blob_off"),
                     (dict(h1=None), b"go together"), (dict(h2=None), b"go together"), (dict(flags=4), b"unknown flags"),
                     (dict(flags=1), b"only when h1 and h2 are NULL"), (dict(n=(1 << 32) - 1), b"2^32 - 2")):
        for i in range(3):
            counts[i] = 7
        assert lib.k2h_amd_ralledata_find(*find_args(**kw)) == _native.K2H_AMD_EINVAL, kw
        assert text in msg() and msg().startswith(b"ralledata_find: ") and list(counts) == [0, 0, 0], (kw, msg())
        texts.add(msg())
    assert len(texts) == 10 and (status == 0xEE).all()
    # m == 0 without hit, and n == 0 with NULL blobs, are no errors and touch no device
    assert lib.k2h_amd_ralledata_find(*find_args(m=0, status=None, koff=None)) == 0 and list(counts) == [0, 0, 0]

    def fetch_args(**kw):
        d = dict(blobs=p(blobs), off=p(off), which=p(which), m=m, seg=1, out=None, ooff=None, total=ctypes.byref(total))
        d.update(kw)
        return (d["blobs"], blobs.size, d["off"], n, d["which"], d["m"], None, d["seg"], d["out"], 0, d["ooff"], None,
                d["total"], None)
    texts = set()
    for kw, text in ((dict(total=None), b"NULL total"), (dict(which=None), b"NULL which"), (dict(blobs=None), b"NULL blobs"),
                     (dict(off=None), b"NULL blob_off"), (dict(seg=4), b"unknown segment"),
                     (dict(out=p(keys)), b"out given without out_off")):
        total.value = 7
        assert lib.k2h_amd_ralledata_fetch(*fetch_args(**kw)) == _native.K2H_AMD_EINVAL, kw
        assert text in msg() and msg().startswith(b"ralledata_fetch: "), (kw, msg())
        assert "total" in kw or total.value == 0
        texts.add(msg())
    assert len(texts) == 6
    total.value = 7
    assert lib.k2h_amd_ralledata_fetch(*fetch_args(m=0, which=None)) == 0 and total.value == 0


def test_exports():
    import k2hash_amd
    from k2hash_amd import find
    for name in ("index_stream", "find_keys", "fetch_segments", "get_values", "StreamIndex", "Found"):
        assert name in k2hash_amd.__all__ and getattr(k2hash_amd, name) is getattr(find, name)
    assert find.StreamIndex._fields == ("buffer", "n", "size", "participants")
    assert find.Found._fields == ("match", "status", "hit", "counts")
    assert (find.FIND_PART, find.FIND_FOUND, find.FIND_ATTRS, find.FIND_EXPIRED, find.FIND_BAD_INDEX) == \
        (PART, FOUND, ATTRS, EXPIRED, BAD_INDEX)
    assert [find.SEGMENTS[s] for s in fm.SEGS] == [0, 1, 2, 3]
    assert len(_native.SIGNATURES["k2h_amd_ralledata_index"][1]) == 9
    assert len(_native.SIGNATURES["k2h_amd_ralledata_find"][1]) == 18
    assert len(_native.SIGNATURES["k2h_amd_ralledata_fetch"][1]) == 14


# ------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("hashes", ["oracle", None])
@pytest.mark.parametrize("now", [None, NOW])
def test_planted_stream(cuda, oracle, hashes, now):
    blobs, consider, queries, _info = planted(oracle)
    buf, off = rm.join(dm.at_odd_offsets(blobs, 3))
    _got, want = fm.find_against_model(cuda, oracle, buf, off, queries, f"planted, hashes {hashes}, now {now}", hashes=hashes,
                                       now=now, consider=consider, shift=5, key_shift=11)
    assert want[3] == [len(queries), len(queries) - len(CS), 3 if now else 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 700])
def test_sizes(cuda, oracle, n):
    """Around the gather's 256-blob tile, one query block and several; every key a hit, as many
    misses, the queries in another order than the stream; both seeds with the hashes computed."""
    recs = rm.records(oracle, n, klen=(1, 70), seed=n)
    keys = recs[0]
    rng = np.random.default_rng(n)
    queries = [keys[i] for i in rng.permutation(n)] + [k + b"?" for k in keys]
    for variant, hashes, shift in ((0, "oracle", 0), (0, None, 9), (1, None, 15)):
        buf, off = rm.stream_of(oracle, recs, variant)
        _got, want = fm.find_against_model(cuda, oracle, buf, off, queries, f"n {n}, variant {variant}, hashes {hashes}",
                                           hashes=hashes, variant=variant, shift=shift, key_shift=16 - shift, tail_pad=0)
        assert want[3][0] == 2 * n and want[3][1] >= n


def _ones_plant(oracle):
    """(blobs, consider, queries, h1, h2): 40 blobs (16 sorted bits).  Blob 4 stores its hash with the
    low 16 bits set, blob 9 -- another key of the same length -- the same hash and subhash, blob 20
    stores ~0 and blob 30, again another key of that length, ~0 with blob 20's subhash.  Blobs 2, 11,
    25 and 33 take no part (masked, bad span, no key, key range outside): the compact lays them out as
    (~0, kNone) behind blobs 20 and 30.  The queries: the keys of blobs 4, 9, 20 and 30 under the
    stored hashes, a key no blob has under ~0 and blob 20's subhash, and blob 25's key under ~0."""
    keys = [b"ones-%02d-" % i + b"x" * 11 for i in range(40)]
    blobs = dm.blobs_of(oracle, keys, [_value(i) for i in range(40)], None, None)
    h4 = rm.get(blobs[4], 0, rm.F_HASH) | 0xFFFF
    dm.set_hash(blobs[4], h4)
    dm.set_hash(blobs[9], h4, rm.get(blobs[4], 0, rm.F_SUBHASH))
    dm.set_hash(blobs[20], NONE)
    dm.set_hash(blobs[30], NONE, rm.get(blobs[20], 0, rm.F_SUBHASH))
    consider = np.ones(40, np.uint8)
    for i, how in zip((2, 11, 25, 33), dh.BREAKS):
        blobs[i] = dh.broken(blobs[i], how)
        consider[i] = how != "masked"
    queries = [keys[4], keys[9], keys[20], keys[30], b"ones-no-" + b"x" * 11, keys[25]]
    s4, s20 = rm.get(blobs[4], 0, rm.F_SUBHASH), rm.get(blobs[20], 0, rm.F_SUBHASH)
    h1 = np.array([h4, h4, NONE, NONE, NONE, NONE], np.uint64)
    h2 = np.array([s4, s4, s20, s20, s20, rm.get(blobs[25], 0, rm.F_SUBHASH)], np.uint64)
    return blobs, consider, queries, h1, h2


def test_ones_plant_in_the_model(oracle):
    blobs, consider, queries, h1, h2 = _ones_plant(oracle)
    buf, off = rm.join(blobs)
    data, koff = fm.csr(queries)
    match, status, hit, counts = fm.find_model(buf, off, data, koff, h1, h2, consider=consider)
    assert match.tolist() == [4, 9, 20, 30, NONE, NONE] and counts == [6, 4, 0]
    parts = [i for i, _f in fm.participants(buf, off, consider=consider)]
    assert len(parts) == 36 and len(blobs) <= 256
    sorted_low = sorted(rm.get(blobs[i], 0, rm.F_HASH) & 0xFFFF for i in parts)
    assert sorted_low[-4:] == [0xFFFF] * 4 and sorted_low[-5] < 0xFFFF      # the four end the participants' column


@pytest.mark.gpu
def test_hashes_of_all_ones_next_to_non_participants(cuda, oracle):
    """Stored hashes whose sorted bits are all set, and ~0 itself, sort to the end of the participants,
    where the compact's (~0, kNone) pairs of the four non-participants follow: the search runs over
    [0, participants), and a miss under ~0 ends in the run without reading a kNone entry's side."""
    blobs, consider, queries, h1, h2 = _ones_plant(oracle)
    buf, off = rm.join(dm.at_odd_offsets(blobs, 6))
    for shift in (0, 13):
        _got, want = fm.find_against_model(cuda, oracle, buf, off, queries, f"ones plant, shift {shift}", hashes=(h1, h2),
                                           consider=consider, shift=shift, key_shift=16 - shift)
        assert want[0].tolist() == [4, 9, 20, 30, NONE, NONE] and want[3] == [6, 4, 0]


@pytest.mark.gpu
def test_queries_at_the_buffer_start_and_judged_alone(cuda, oracle):
    """A query that starts fewer than 16 bytes into the keys buffer (chunk 0 must not be loaded
    whole), and offsets that are no CSR: decreasing, past the end, empty.  Such a query takes no
    part whether the hashes are passed or computed."""
    blobs, consider, _queries, info = planted(oracle)
    buf, off = rm.join(blobs)
    pick = [k for k in info["dup"]][:4]                                # 14 .. 31 bytes
    for lead in (b"", b"x", b"0123456789abcde"):
        fm.find_against_model(cuda, oracle, buf, off, pick, f"lead {len(lead)}", lead=lead, consider=consider, tail_pad=0)
        fm.find_against_model(cuda, oracle, buf, off, pick, f"lead {len(lead)}, computed", lead=lead, hashes=None,
                              consider=consider, tail_pad=0)
    k0, k1 = pick[0], pick[1]
    data = k0 + k1
    a, b = len(k0), len(k0) + len(k1)
    #                 k0      bad     k1 (again a start)   bad: past the end   empty   k0 again
    spans = [(0, a), (a, 3), (a, b), (b, b + 9), (5, 5), (0, a)]
    h = fm.hashes_of(oracle, [k0, k1])
    t, kt = tm.place(cuda, buf, 3), tm.place(cuda, data, 7, tail_pad=0)
    index, _parts, doff = fm.run_index(cuda, t, len(buf), off, consider)
    for q, (s, e) in enumerate(spans):                                  # one query per call: key_off has two entries
        koff = np.array([s, e], np.uint64)
        src = 0 if (s, e) == (0, a) else 1
        h1, h2 = h[0][src:src + 1], h[1][src:src + 1]
        want = fm.find_model(buf, off, data, koff, h1, h2, consider=consider)
        assert bool(want[1][0] & PART) == (q in (0, 2, 5))
        fm.assert_found(fm.run_find(cuda, t, len(buf), doff, len(off) - 1, index, kt, len(data), koff, h1, h2), want, f"span {q}")
        fm.assert_found(fm.run_find(cuda, t, len(buf), doff, len(off) - 1, index, kt, len(data), koff), want, f"span {q}, computed")


@pytest.mark.gpu
def test_c_strings(cuda, oracle):
    """K2H_AMD_FLAG_CSTR: the stream stores key + NUL, the queries are the bare strings, the empty
    one included.  A later blob of the same key length whose last byte is not 0, under the
    query's hashes, is not the match."""
    names = [b"", b"a", b"fifteen-bytes-x", b"sixteen-bytes-xy", b"seventeen-bytes-x", b"k" * 47]
    stored = [k + b"\0" for k in names]
    blobs = dm.blobs_of(oracle, stored + [k + b"x" for k in names], [b"v%d" % i for i in range(12)], None, None)
    for i in range(6):
        dm.set_hash(blobs[6 + i], rm.get(blobs[i], 0, rm.F_HASH), rm.get(blobs[i], 0, rm.F_SUBHASH))
    buf, off = rm.join(dm.at_odd_offsets(blobs, 1))
    queries = names + [b"absent"]
    for hashes in ("oracle", None):
        got, want = fm.find_against_model(cuda, oracle, buf, off, queries, f"cstr, hashes {hashes}", hashes=hashes, cstr=True,
                                          shift=1, key_shift=2, tail_pad=0)
        assert want[0].tolist() == [0, 1, 2, 3, 4, 5, NONE] and want[3] == [7, 6, 0]
    # without the flag the bare strings are other keys: nothing is found, and the empty one takes no part
    _got, want = fm.find_against_model(cuda, oracle, buf, off, queries, "no cstr", hashes=None)
    assert want[3] == [6, 0, 0]


@pytest.mark.gpu
def test_call_shapes(cuda, oracle):
    """n == 0, m == 0, outputs left out, the asynchronous forms, and an index that is not the
    stream's."""
    import torch
    blobs, consider, queries, _info = planted(oracle)
    buf, off = rm.join(blobs)
    n = len(off) - 1
    data, koff = fm.csr(queries)
    h1, h2 = fm.hashes_of(oracle, queries)
    want = fm.find_model(buf, off, data, koff, h1, h2, consider=consider)
    t, kt = tm.place(cuda, buf, 2), tm.place(cuda, data, 4)
    index, parts, doff = fm.run_index(cuda, t, len(buf), off, consider, count=False)
    assert parts is None
    args = (cuda, t, len(buf), doff, n, index, kt, len(data), koff, h1, h2)
    fm.assert_found(fm.run_find(*args, count=False), want, "count=False")
    got = fm.run_find(*args, want_hit=False, want_match=False)
    fm.assert_found(got, want, "status only", want_hit=False, want_match=False)
    assert (got[2] == 0x5A).all() and (got[0] == 0x5A5A5A5A5A5A5A5A).all()
    # the index of another stream: one blob fewer
    got = fm.run_find(cuda, t, off[n - 1], doff[:n], n - 1, index, kt, len(data), koff, h1, h2)
    assert (got[1] == BAD_INDEX).all() and (got[0] == NONE).all() and (got[2] == 0).all() and got[3] == [0, 0, 0]
    # ... and a buffer that holds no index at all
    junk = torch.full((index.numel(),), 0xC3, dtype=torch.uint8, device=cuda)
    got = fm.run_find(cuda, t, len(buf), doff, n, junk, kt, len(data), koff, h1, h2)
    assert (got[1] == BAD_INDEX).all() and (got[0] == NONE).all()
    # m == 0: hit is zeroed, counts too
    got = fm.run_find(cuda, t, len(buf), doff, n, index, kt, 0, np.zeros(1, np.uint64))
    assert (got[2] == 0).all() and got[3] == [0, 0, 0] and got[1].size == 0
    # n == 0: an ordinary call in which nothing is found
    fm.find_against_model(cuda, oracle, b"", [0], queries[:5], "n == 0")
    fm.find_against_model(cuda, oracle, b"", [0], queries[:5], "n == 0, computed", hashes=None)


def _fetch_stream(oracle):
    recs = rm.records(oracle, 300, klen=(1, 40), vlen=(0, 300), slen=(0, 64), alen=(0, 48), seed=77)
    recs[1][5], recs[1][6], recs[1][7] = b"a" * 4095, b"b" * 4096, b"c" * 9001      # around the whole-block threshold
    return rm.split(*rm.stream_of(oracle, recs))


@pytest.mark.gpu
@pytest.mark.parametrize("segment", fm.SEGS)
def test_fetch(cuda, oracle, segment):
    """Every segment, in random order with repeats, ~0 and indices past n among the slots, with
    and without take; values around the 4 KiB whole-block threshold; one slot, and several blocks."""
    blobs = _fetch_stream(oracle)
    n = len(blobs)
    buf, off = rm.join(dm.at_odd_offsets(blobs, 9))
    rng = np.random.default_rng(5)
    which = np.concatenate([rng.integers(0, n, 900).astype(np.uint64), np.array([5, 6, 7, 6, NONE, n, n + 5, 1 << 40], np.uint64)])
    which = which[rng.permutation(which.size)]
    take = (rng.random(which.size) < 0.8).astype(np.uint8)
    want = fm.fetch_against_model(cuda, buf, off, which, segment, "random", shift=7, tail_pad=0)
    assert want[2].sum() == 3
    fm.fetch_against_model(cuda, buf, off, which, segment, "random, take", take=take, shift=0)
    fm.fetch_against_model(cuda, buf, off, np.arange(n, dtype=np.uint64), segment, "stream order", shift=15)
    fm.fetch_against_model(cuda, buf, off, np.array([7], np.uint64), segment, "one slot", shift=1)
    fm.fetch_against_model(cuda, buf, off, np.array([NONE, NONE], np.uint64), segment, "nothing", shift=1)


@pytest.mark.gpu
def test_fetch_bad_blobs_and_cap(cuda, oracle):
    """Spans and segment ranges that are bad yield nothing and are flagged; a pos + len that wraps
    is not formed; segments may overlap or lie in the header; out_cap one byte short writes
    nothing."""
    import torch
    blobs = _fetch_stream(oracle)[:40]
    L = [len(b) for b in blobs]
    rm.put(blobs[1], 0, rm.F_VLEN, L[1])                                          # len alone passes the end
    rm.put(blobs[2], 0, rm.F_VLEN + 32, L[2] - 3), rm.put(blobs[2], 0, rm.F_VLEN, 4)   # pos + len one past the end
    rm.put(blobs[3], 0, rm.F_VLEN + 32, (1 << 64) - 8), rm.put(blobs[3], 0, rm.F_VLEN, 16)   # the sum wraps
    rm.put(blobs[4], 0, rm.F_VLEN + 32, L[4] - 4), rm.put(blobs[4], 0, rm.F_VLEN, 4)   # ends with the blob: good
    rm.put(blobs[5], 0, rm.F_VLEN + 32, 8), rm.put(blobs[5], 0, rm.F_VLEN, 24)         # inside the header: good
    rm.put(blobs[6], 0, rm.F_VLEN + 32, (1 << 63) + 5), rm.put(blobs[6], 0, rm.F_VLEN, 0)   # length 0: pos ignored
    blobs[7] = blobs[7][:79]
    buf, off = rm.join(blobs)
    off2 = list(off)
    off2[10] = off2[11] + 1                                                       # blob 9 is long, blob 10 runs backwards
    which = np.arange(12, dtype=np.uint64)
    want = fm.fetch_against_model(cuda, buf, off, which, "value", "bad ranges", shift=3, tail_pad=0)
    assert want[2].tolist() == [0, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0]
    want = fm.fetch_against_model(cuda, buf, off2, which, "value", "bad spans", shift=3, tail_pad=0)
    assert want[2][7] == 1 and want[2][9] == 0 and want[2][10] == 1
    t = tm.place(cuda, buf, 3)
    doff = torch.from_numpy(np.asarray(off, np.int64)).to(cuda)
    need = len(fm.fetch_model(buf, off, which, "value")[0])
    rc, data, _ooff, _bad, total = fm.run_fetch(cuda, t, len(buf), doff, len(off) - 1, which, "value", cap=need - 1)
    assert rc == _native.K2H_AMD_EINVAL and total == need and data == b"\x5a" * (need - 1)
    assert b"out_cap" in bytes(_native.batch_lib().k2h_amd_strerror(rc))


@pytest.mark.gpu
def test_python_wrappers_on_a_side_stream(cuda, oracle):
    """index_stream, find_keys, fetch_segments and get_values on a stream that is not current."""
    import torch

    from k2hash_amd import find
    blobs, consider, queries, _info = planted(oracle)
    buf, off = rm.join(blobs)
    data, koff = fm.csr(queries)
    h1, h2 = fm.hashes_of(oracle, queries)
    want = fm.find_model(buf, off, data, koff, h1, h2, now=NOW, consider=consider)
    s = torch.cuda.Stream(device=cuda)
    with torch.cuda.stream(s):
        d = [torch.from_numpy(np.frombuffer(bytes(x), np.uint8).copy()).to(cuda) for x in (buf, data)]
        o = [torch.from_numpy(np.asarray(x, np.uint64).astype(np.int64)).to(cuda) for x in (off, koff)]
        con = torch.from_numpy(consider).to(cuda)
    ix = find.index_stream(d[0], o[0], consider=con, stream=s)
    assert ix.participants == len(fm.participants(buf, off, consider=consider)) and (ix.n, ix.size) == (len(off) - 1, len(buf))
    f = find.find_keys(d[0], o[0], ix, d[1], o[1], now=NOW, want_hit=True, stream=s)
    s.synchronize()
    assert tuple(f.counts) == tuple(want[3])
    assert (f.match.cpu().numpy().view(np.uint64) == want[0]).all() and (f.status.cpu().numpy() == want[1]).all()
    assert (f.hit.cpu().numpy() == want[2]).all()
    take = [(int(x) & (FOUND | EXPIRED)) == FOUND for x in want[1]]
    vals = fm.fetch_model(buf, off, want[0], "value", take)
    out, out_off, status = find.get_values(d[0], o[0], ix, d[1], o[1], now=NOW, stream=s)
    s.synchronize()
    assert out.cpu().numpy().tobytes() == vals[0] and (out_off.cpu().numpy().view(np.uint64) == vals[1]).all()
    assert (status.cpu().numpy() == want[1]).all()
    keys_back, koff_back, bad = find.fetch_segments(d[0], o[0], f.match, "key", want_bad=True, stream=s)
    s.synchronize()
    kb = fm.fetch_model(buf, off, want[0], "key")
    assert keys_back.cpu().numpy().tobytes() == kb[0] and (koff_back.cpu().numpy().view(np.uint64) == kb[1]).all()
    assert not bad.cpu().numpy().any()
