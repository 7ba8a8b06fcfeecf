"""Helper for tests/test_ralledata_from_records.py (not a test module).

* The constants of k2h_ralledata_recs.hip, parsed from the source, and forms(): a restatement of
  the kernel's block-uniform staged / direct choice, so that every scenario can say in advance
  which form each of its blocks takes.
* expected(): the blob stream a list of range records must give -- oracle.build_ralledata over
  Python-sliced byte strings (b"\\0" appended for the import form), a skipped record left out and
  its offset repeated.  Nothing here calls the code under test.
* The scenarios (import and archive), each a Case of file bytes, records and the forms it claims.
* run(): one call pair of the C ABI (sizes only, then build) over a file placed between canary
  bytes, into sentinel-filled outputs.
"""
import ctypes
import functools
import json
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

from import_scenarios import HDR74, fill, ordinary, ref_scan

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
SRC_PATH = ROOT / "k2hash_amd" / "csrc" / "k2h_ralledata_recs.hip"
_SRC = SRC_PATH.read_text()


def _const(name, env=None):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", _SRC)
    assert m, name
    expr = re.sub(r"(?<=\d)(ull|u|ul)\b", "", m.group(1).strip(), flags=re.I)
    assert re.fullmatch(r"[\w\s*<>+()/-]+", expr), (name, expr)
    return int(eval(expr, {"__builtins__": {}}, dict(env or {})))  # noqa: S307  (numbers, names, operators)


R = kRecRecs = _const("kRecRecs")                                  # records per block (64)
kRecPool = _const("kRecPool")                                      # staged bytes (12 KiB)
HULL = kRecHullMax = _const("kRecHullMax", dict(kRecPool=kRecPool))  # first start .. last end of a staged block
WAVES = int(re.search(r"amdgpu_waves_per_eu\((\d+)\)", _SRC).group(1))

U64 = 1 << 64
EINVAL = -1
OUT_FILL, OFF_FILL = 0xC3, 0x5A5AA5A55A5AA5A5
GUARD = 64


# ------------------------------------------------------------------------------- the model
def inside(off, ln, size):
    return off <= size and ln <= size - off


def import_segments(rec, size):
    """The file segments (key, value) of an import record, or None when it yields no blob."""
    ko, kl, vo, vl = (int(x) for x in rec)
    return [(ko, kl), (vo, vl)] if inside(ko, kl, size) and inside(vo, vl, size) else None


def archive_segments(r, size):
    """The file segments (key, value, subkeys, attrs) of an archive record (a REC_DTYPE row), or
    None: only a SCOM_SET_ALL record of status 0 with a key and all four ranges in the file."""
    if int(r["status"]) != 0 or int(r["type"]) != 0 or int(r["key_len"]) == 0:
        return None
    segs = [(int(r[o]), int(r[n])) for o, n in (("key_off", "key_len"), ("val_off", "val_len"),
                                                 ("skey_off", "skey_len"), ("attrs_off", "attrs_len"))]
    return segs if all(inside(o, n, size) for o, n in segs) else None


def forms(segs):
    """Per block of kRecRecs records: "none" (no record yields a blob: the block returns),
    "staged" or "direct".  Staged: walking the kept records in order and each one's segments of
    length > 0 in blob order, every segment starts at or after the end of the one before it, and
    the first start .. the last end is at most kRecHullMax."""
    out = []
    for b in range(0, len(segs), R):
        blk = [s for s in segs[b:b + R] if s is not None]
        if not blk:
            out.append("none")
            continue
        ordered, first, end = True, None, 0
        for rec in blk:
            for o, n in rec:
                if n:
                    ordered = ordered and o >= end
                    first = o if first is None else first
                    end = max(end, o + n)
        out.append("staged" if ordered and (first is None or end - first <= HULL) else "direct")
    return out


def expected(oracle, data, segs, nul, std_fnv=False):
    """(blob bytes, blob_off of n + 1 uint64) of the records whose segments are `segs`."""
    data = bytes(data)
    tail = b"\0" if nul else b""
    kept = [s for s in segs if s is not None]
    nseg = len(kept[0]) if kept else 0     # 2 (import: key, value) or 4 (archive)
    cols = [[data[s[j][0]:s[j][0] + s[j][1]] + tail for s in kept] if j < nseg else None for j in range(4)]
    if kept:
        blobs, off = oracle.build_ralledata(cols[0], cols[1], cols[2], cols[3], 1 if std_fnv else 0)
    else:
        blobs, off = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    full = np.zeros(len(segs) + 1, np.uint64)
    k = 0
    for i, s in enumerate(segs):
        full[i] = off[k]
        k += s is not None
    full[len(segs)] = off[k]
    assert k == len(kept) and int(off[k]) == blobs.size
    return np.asarray(blobs, np.uint8), full


# --------------------------------------------------------------------------- the scenarios
# claim: what forms(...) of the scenario must be -- "staged" / "direct": every block with a blob;
# a list: exactly that; a set: exactly those forms occur
Case = namedtuple("Case", "name kind data recs claim fmt")


def _imp(name, data, recs, claim, fmt="tsv"):
    return Case(name, "import", bytes(data), np.array(recs, np.uint64).reshape(-1, 4), claim, fmt)


@functools.lru_cache(None)
def ordinary_file(n, salt=0):
    """n whole records of import_scenarios.ordinary (130 .. 192 bytes each): (data, records)."""
    data = ordinary(200 * n + 400, b"\t", 900 + salt, n)
    recs = ref_scan(data, "tsv")[1][:n]
    assert len(recs) == n
    return data[:recs[-1][2] + recs[-1][3] + 1], recs


BLOCK_EDGE_N = (1, R - 1, R, R + 1, 2 * R, 2 * R + 1)
KEY_LENS = (0, 1, 14, 15, 16, 17, 31, 32, 254)
VAL_LENS = (0, 1, 15, 16)


def lengths_file():
    """Every key length x value length, a NUL-cut key, a NUL-cut value, and a last value that ends
    exactly at the file's end with no newline."""
    out = []
    for i, kl in enumerate(KEY_LENS):
        for j, vl in enumerate(VAL_LENS):
            out.append(fill(kl, 910, i, j) + b"\t" + fill(vl, 911, i, j) + b"\n")
    out.append(fill(5, 912) + b"\0" + fill(7, 913) + b"\t" + fill(9, 914) + b"\n")     # key cut at 5
    out.append(fill(6, 915) + b"\t" + fill(4, 916) + b"\0" + fill(20, 917) + b"\n")    # value cut at 4
    out.append(fill(8, 918) + b"\t" + fill(21, 919))                                   # ends at size
    data = b"".join(out)
    recs = ref_scan(data, "tsv")[1]
    assert len(recs) == len(out) and recs[-3][1] == 5 and recs[-2][3] == 4
    assert recs[-1][2] + recs[-1][3] == len(data)
    assert {(r[1], r[3]) for r in recs} >= {(k, v) for k in KEY_LENS for v in VAL_LENS}
    return data, recs


def big_value_file(nblocks_pattern, big):
    """One block of kRecRecs records per pattern entry: "s" = ordinary records, "d" = the same with
    one value of `big` bytes in the middle."""
    parts = []
    for b, kind in enumerate(nblocks_pattern):
        d, _ = ordinary_file(R, 20 + b)
        if kind == "d":
            recs = ref_scan(d, "tsv")[1]
            cut = recs[R // 2][2] + recs[R // 2][3]       # the end of record 32's value
            d = d[:cut] + fill(big, 920, b) + d[cut:]
        parts.append(d)
    data = b"".join(parts)
    recs = ref_scan(data, "tsv")[1]
    assert len(recs) == R * len(nblocks_pattern)
    return data, recs


def skip_file():
    """Four blocks (64, 64, 64, 1 records) with hostile ranges: the first record, one in the
    middle, the last one, and all 64 of block 2; one record keeps the valid empty value at size."""
    data, recs = ordinary_file(3 * R + 1, 30)
    size = len(data)
    recs = [list(r) for r in recs]
    recs[0][1] = size + 1 - recs[0][0]                     # key: off + len = size + 1
    recs[10][2:] = [size, 0]                               # valid: the empty value at size
    recs[R + 6][2:] = [size + 1, 0]                        # value: off = size + 1, len = 0
    for j in range(R):                                     # off + len = size + 1 .. size + 64
        r = recs[2 * R + j]
        if j % 2:
            r[3] = size + 1 + j - r[2]
        else:
            r[1] = size + 1 + j - r[0]
    recs[3 * R][0:2] = [U64 - 4, 8]                        # the wrapping pair
    return data, [tuple(r) for r in recs]


def random_file(oracle, n=50000):
    """About n TSV records: keys 1-300 bytes, values 0-260 bytes, a fifth of the values empty,
    payload from the oracle's byte stream with the delimiter bytes masked out."""
    rng = np.random.default_rng(77)
    kl = rng.integers(1, 301, n)
    vl = np.where(rng.random(n) < 0.2, 0, rng.integers(0, 261, n))
    a = oracle.gen_bytes(int(kl.sum() + vl.sum() + 2 * n), 0x52414C4C).copy()
    a[(a == 0) | (a == 9) | (a == 10)] = 0x41
    end = np.cumsum(kl + vl + 2)
    a[end - 1] = 10
    a[end - vl - 2] = 9
    beg = end - (kl + vl + 2)
    recs = np.stack([beg, kl, beg + kl + 1, vl], 1).astype(np.uint64)
    return a.tobytes(), recs


def import_cases():
    out = []
    for n in BLOCK_EDGE_N:
        d, r = ordinary_file(n)
        out.append(_imp(f"edge-n{n}", d, r, "staged"))
    d, r = lengths_file()
    out.append(_imp("lengths", d, r, "staged"))
    out.append(_imp("lengths-reversed", d, r[::-1], "direct"))
    d, r = big_value_file("d", 20 * 1024)
    out.append(_imp("direct-one-20k-value", d, r, ["direct"]))
    d = HDR74 + b"key1\nvalue1\n" + b"lastkey"
    r = ref_scan(d, "mdbm")[1]
    assert len(r) == 2 and r[1][2:] == r[0][2:]
    out.append(_imp("direct-mdbm-key-line-at-eof", d, r, ["direct"], "mdbm"))
    d, r = ordinary_file(2 * R + 1)
    out.append(_imp("direct-reversed", d, r[::-1], ["direct", "direct", "staged"]))
    out.append(_imp("direct-duplicate-5", d, r[:6] + r[5:], ["direct", "staged", "staged"]))
    d, r = big_value_file("sdsd", kRecPool)
    out.append(_imp("alternate-staged-direct", d, r, ["staged", "direct", "staged", "direct"]))
    d, r = skip_file()
    out.append(_imp("skips", d, r, ["staged", "staged", "none", "none"]))
    return out


def golden_import_cases():
    """Every golden import file that scans without error.  Its records are ref_scan's, held against
    import.json (what the reference's own loops printed): the same strings, and the same offsets
    wherever the reference could report one (its tellg is -1 once the stream hit EOF)."""
    g = json.loads((GOLDEN / "import.json").read_text())["inputs"]
    out = []
    for name in sorted(g):
        if g[name]["error"]:
            continue
        data = (GOLDEN / "import" / name).read_bytes()
        err, recs = ref_scan(data, g[name]["format"])
        assert not err and len(recs) == len(g[name]["records"]), name
        for (ko, kl, vo, vl), x in zip(recs, g[name]["records"]):
            assert data[ko:ko + kl].hex() == x["key"] and data[vo:vo + vl].hex() == x["val"], name
            assert x["key_off"] in (-1, ko) and x["val_off"] in (-1, vo), name
        out.append(_imp(f"golden-{name}", data, recs, None, g[name]["format"]))
    return out


def archive_cases():
    from k2hash_amd import archive
    f = (GOLDEN / "archive.k2har").read_bytes()
    recs = archive.scan(f)                 # the host scan, pinned to archive.json by test_archive.py
    ends = [int(r["offset"]) for r in recs[1:]] + [len(f)]
    parts = [f[int(r["offset"]):e] for r, e in zip(recs, ends)]
    is_set = [int(r["type"]) == 0 for r in recs]
    assert len(parts) == 64 and sum(is_set) == 10
    sets = [p for p, s in zip(parts, is_set) if s]
    rest = [p for p, s in zip(parts, is_set) if not s]
    rng = np.random.default_rng(78)

    def case(name, data, claim):
        return Case(name, "archive", bytes(data), archive.scan(data), claim, None)
    out = [case("golden", f, ["staged"])]
    out.append(case("set-all-200", b"".join(sets[i] for i in rng.integers(0, 10, 200)),
                    ["direct", "direct", "direct", "staged"]))   # 64 records with their 104-byte headers exceed the pool
    out.append(case("mixed-200", b"".join(parts[i] for i in rng.integers(0, 64, 200)), "staged"))
    out.append(case("no-set-all-200", b"".join(rest[i] for i in rng.integers(0, 54, 200)), ["none"] * 4))
    # forged headers among SET_ALL records: key_length = 0 (its bytes counted as exdata, so that
    # the next record still starts where it did), an unknown type, and, last, a value past EOF
    nokey = bytearray(sets[1])
    kl = int.from_bytes(nokey[24:32], "little")
    nokey[24:32] = (0).to_bytes(8, "little")
    nokey[56:64] = (int.from_bytes(nokey[56:64], "little") + kl).to_bytes(8, "little")
    badtype = bytearray(sets[2])
    badtype[16:24] = (9).to_bytes(8, "little")
    trunc = bytearray(sets[3])
    trunc[32:40] = (1 << 40).to_bytes(8, "little")
    c = case("forged", sets[0] + bytes(nokey) + sets[4] + bytes(badtype) + sets[5] + bytes(trunc), ["staged"])
    assert [int(x) for x in c.recs["status"]] == [0, 0, 0, 1, 0, 2] and int(c.recs["key_len"][1]) == 0
    out.append(c)
    return out


def segments_of(case):
    size = len(case.data)
    if case.kind == "import":
        return [import_segments(r, size) for r in case.recs]
    return [archive_segments(r, size) for r in case.recs]


def claim_holds(case):
    got = forms(segments_of(case))
    c = case.claim
    if c is None:
        return True, got
    if isinstance(c, str):
        return all(x in (c, "none") for x in got) and c in got, got
    if isinstance(c, set):
        return set(got) == c, got
    return got == c, got


# ------------------------------------------------------------------------------ device side
def recs_words(case):
    """The records as the (n, 4) or (n, 13) int64 array the device calls take."""
    a = np.ascontiguousarray(case.recs)
    return a.view(np.int64).reshape(len(case.recs), 4 if case.kind == "import" else 13)


def run(cuda, kind, file, recs_i64, std_fnv=False, cap=None, oshift=0):
    """Sizes only, then the build with out_cap = cap (None: the total; "none": sizes only).
    Returns dict(rc0, total0, off0, rc, total, off, out, before, after): host arrays, `out` the
    whole capacity and the guard bytes either side of it."""
    import torch

    from k2hash_amd import _native
    from k2hash_amd.batch import _stream_handle
    lib = _native.batch_lib()
    fn = {"import": lib.k2h_amd_import_ralledata, "archive": lib.k2h_amd_archive_ralledata}[kind]
    n = recs_i64.shape[0]
    recs = torch.from_numpy(np.ascontiguousarray(recs_i64)).to(cuda) if n else None
    rp = ctypes.c_void_p(recs.data_ptr()) if n else None
    fp = ctypes.c_void_p(file.data_ptr() or 1)
    flags = _native.K2H_AMD_FLAG_STD_FNV if std_fnv else 0
    st = _stream_handle(None)
    res = {}

    def call(tag, out, out_cap):
        off = torch.full((n + 1 + GUARD,), OFF_FILL, dtype=torch.int64, device=cuda)
        total = ctypes.c_uint64(0xDEAD)
        rc = fn(fp, file.numel(), rp, n, out, out_cap, ctypes.c_void_p(off.data_ptr()), ctypes.byref(total), flags, st)
        torch.cuda.synchronize()
        o = off.cpu().numpy().view(np.uint64)
        assert (o[n + 1:] == np.uint64(OFF_FILL)).all(), "blob_off written past entry n"
        res["rc" + tag], res["total" + tag], res["off" + tag] = rc, total.value, o[:n + 1]
    call("0", None, 0)
    if cap == "none":
        return res
    cap = res["total0"] if cap is None else cap
    buf = torch.full((GUARD + oshift + cap + GUARD,), OUT_FILL, dtype=torch.uint8, device=cuda)
    call("", ctypes.c_void_p(buf.data_ptr() + GUARD + oshift), cap)
    h = buf.cpu().numpy()
    res["before"], res["out"], res["after"] = h[:GUARD + oshift], h[GUARD + oshift:GUARD + oshift + cap], h[-GUARD:]
    return res


def check_stream(what, res, want_blobs, want_off):
    """The whole contract of one successful run against the expected stream."""
    total = int(want_off[-1])
    for tag in ("0", ""):
        assert res["rc" + tag] == 0, (what, "rc" + tag, res["rc" + tag])
        assert res["total" + tag] == total, (what, "total" + tag, res["total" + tag], total)
        bad = np.flatnonzero(res["off" + tag] != want_off)
        assert bad.size == 0, (what, "blob_off" + tag, f"{bad.size} differ, first at {int(bad[0])}: "
                               f"{int(res['off' + tag][bad[0]])} != {int(want_off[bad[0]])}")
    assert (res["before"] == OUT_FILL).all(), (what, "bytes before out written")
    assert (res["after"] == OUT_FILL).all(), (what, "bytes after the capacity written")
    assert (res["out"][total:] == OUT_FILL).all(), (what, "bytes from total on written")
    bad = np.flatnonzero(res["out"][:total] != want_blobs)
    if bad.size:
        i = int(np.searchsorted(want_off, bad[0], side="right") - 1)
        raise AssertionError((what, f"{bad.size} of {total} bytes differ, first at {int(bad[0])} = byte "
                              f"{int(bad[0]) - int(want_off[i])} of blob {i}: "
                              f"{int(res['out'][bad[0]]):#x} != {int(want_blobs[bad[0]]):#x}"))
