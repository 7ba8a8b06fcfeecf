"""Helper for tests/test_ralledata_archive.py and test_ralledata_archive_4gib.py (not a test
module, not a conftest).

* scom_set_all(): a Python restatement of the SCOM_SET_ALL record K2HCommandArchive::SetAll
  produces (lib/k2hcommand.cc:69-135, scom_init at lib/k2hcommand.h:99-113); the CPU test pins it
  to the ten records the reference wrote into tests/golden/archive.k2har.
* model(): what k2h_amd_ralledata_archive must give for a stream -- the participants by
  ralle_check_model.header_status (the rule of _dedup), their records by scom_set_all over
  Python-sliced segments.  Nothing here calls the code under test except run(), which only
  launches it.
* The constants of k2h_ralledata_archive.hip, parsed from the source, and forms(): a restatement
  of the build kernel's block-uniform staged / direct choice.
* Blob forgers: segments permuted, overlapping, with slack, garbage positions.
"""
import ctypes
import re
import struct
from pathlib import Path

import numpy as np

import ralle_check_model as rm

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden"
SRC_PATH = ROOT / "k2hash_amd" / "csrc" / "k2h_ralledata_archive.hip"
_SRC = SRC_PATH.read_text()


def _const(name, env=None):
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", _SRC)
    assert m, name
    expr = m.group(1).strip()
    assert re.fullmatch(r"[\w\s*<>+()/-]+", expr), (name, expr)
    return int(eval(expr, {"__builtins__": {}}, dict(env or {})))  # noqa: S307  (numbers, names, operators)


SCOM = 104                                                    # sizeof(SCOM), packed
B = kArcBlobs = _const("kArcBlobs")                           # blobs per block
kArcPool = _const("kArcPool")                                 # staged bytes
HULL = kArcHullMax = _const("kArcHullMax", dict(kArcPool=kArcPool))
WAVES = int(re.search(r"amdgpu_waves_per_eu\((\d+)\)", _SRC).group(1))
KERNELS = ("scom_archive_size_kernel", "scom_archive_build_kernel")
BUILD_KERNEL = "scom_archive_build_kernel"

U64 = 1 << 64
OK, EINVAL = 0, -1
OUT_FILL, OFF_FILL = 0xC3, 0x5A5AA5A55A5AA5A5
GUARD = 64
COMMAND = b"\nK2H_SET_ALL" + bytes(4)


# ------------------------------------------------------------------------------- the model
def scom_set_all(key, val=b"", skey=b"", attrs=b""):
    """The archive record of one element: szCommand, type 0, the four lengths and exdata_length
    0, the four running positions from 104 and exdata_pos = 104, then the segments."""
    k, v, s, a = len(key), len(val), len(skey), len(attrs)
    head = struct.pack("<16sq5Q5q", COMMAND, 0, k, v, s, a, 0, SCOM, SCOM + k, SCOM + k + v, SCOM + k + v + s, SCOM)
    assert len(head) == SCOM
    return head + bytes(key) + bytes(val) + bytes(skey) + bytes(attrs)


def segments(buf, b, e, size, kept=True):
    """The absolute (offset, length) of the key, value, subkeys and attrs of blob [b, e) of the
    stream when it takes part, else None."""
    if not kept:
        return None
    st, f = rm.header_status(buf, b, e, size)
    if st != rm.OK:
        return None
    return [(b + f[6 + s] if f[2 + s] else 0, f[2 + s]) for s in range(4)]


def stream_segments(buf, off, size=None, keep=None):
    buf = bytes(buf)
    size = len(buf) if size is None else size
    return [segments(buf, int(off[i]), int(off[i + 1]), size, keep is None or bool(keep[i]))
            for i in range(len(off) - 1)]


def model(buf, off, size=None, keep=None):
    """(archive bytes as a uint8 array, rec_off of n + 1 uint64, records, segments per blob)."""
    buf = bytes(buf)
    segs = stream_segments(buf, off, size, keep)
    recs, rec_off = [], np.zeros(len(segs) + 1, np.uint64)
    at = 0
    for i, s in enumerate(segs):
        rec_off[i] = at
        if s is not None:
            recs.append(scom_set_all(*(buf[o:o + n] for o, n in s)))
            at += len(recs[-1])
    rec_off[len(segs)] = at
    data = np.frombuffer(b"".join(recs), np.uint8)
    assert data.size == at
    return data, rec_off, len(recs), segs


def forms(segs, off):
    """Per block of kArcBlobs blobs: "none" (no blob yields a record: the block returns),
    "staged" or "direct".  Staged: the participants lie in stream order without overlap (each
    starts at or after the end of the one before it), the first one's start .. the last one's
    end is at most kArcHullMax, and inside each the segments of length > 0 lie in record order
    without overlap.  "direct" when the offsets already say so, "direct-late" when only the
    blobs' headers do (the kernel has staged the run by then)."""
    out = []
    for b in range(0, len(segs), B):
        blk = [i for i in range(b, min(b + B, len(segs))) if segs[i] is not None]
        if not blk:
            out.append("none")
            continue
        ordered, end = True, 0
        for i in blk:
            ordered = ordered and int(off[i]) >= end
            end = max(end, int(off[i + 1]))
        if not ordered or end - int(off[blk[0]]) > HULL:
            out.append("direct")
            continue
        inner = True
        for i in blk:
            hi = 0
            for o, n in segs[i]:
                if n:
                    inner = inner and o >= hi
                    hi = o + n
        out.append("staged" if inner else "direct-late")
    return out


# ------------------------------------------------------------------------------ blob forgers
def _rng(*salt):
    return np.random.default_rng([10400 + int(x) for x in salt])


def rbytes(rng, n):
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


def blobs_of(oracle, keys, vals=None, skeys=None, attrs=None):
    """The reference producer's blobs of the records, as a list of bytearrays."""
    out, boff = oracle.build_ralledata(keys, vals, skeys, attrs)
    return rm.split(bytearray(out.tobytes()), [int(x) for x in boff])


def forge(key, val=b"", skey=b"", attrs=b"", order=(0, 1, 2, 3), gaps=(0, 0, 0, 0), slack=0, hashes=(0x1111, 0x2222),
          fill=0xEE):
    """A blob by hand: the four segments laid out behind the header in `order`, gaps[j] filler
    bytes before the j-th placed one, `slack` filler bytes behind the last.  The hash fields
    are whatever `hashes` says (the writer must not care)."""
    seg = [bytes(key), bytes(val), bytes(skey), bytes(attrs)]
    pos, body = [0] * 4, bytearray()
    for j, s in enumerate(order):
        body += bytes([fill]) * gaps[j]
        pos[s] = rm.HEADER + len(body)
        body += seg[s]
    body += bytes([fill]) * slack
    head = struct.pack("<10Q", hashes[0], hashes[1], *(len(x) for x in seg), *pos)
    return bytearray(head) + body


def records(rng, n, klen=(1, 41), vlen=(0, 101), p_extra=0.0, slen=(1, 17), alen=(1, 25)):
    """n records as four lists of bytes; subkeys / attrs non-empty with probability p_extra."""
    ks = [rbytes(rng, x) for x in rng.integers(klen[0], klen[1], n)]
    vs = [rbytes(rng, x) for x in rng.integers(vlen[0], vlen[1], n)]
    ss = [rbytes(rng, rng.integers(slen[0], slen[1])) if rng.random() < p_extra else b"" for _ in range(n)]
    as_ = [rbytes(rng, rng.integers(alen[0], alen[1])) if rng.random() < p_extra else b"" for _ in range(n)]
    return ks, vs, ss, as_


# ------------------------------------------------------------------------------ device side
def place(cuda, buf, shift=0, canary=0xA5):
    """buf on the device, starting `shift` bytes past a 16-byte boundary, canary bytes around it."""
    import torch
    whole = np.full(GUARD + shift + len(buf) + GUARD, canary, np.uint8)
    whole[GUARD + shift:GUARD + shift + len(buf)] = np.frombuffer(bytes(buf), np.uint8)
    t = torch.from_numpy(whole).to(cuda)
    assert t.data_ptr() % 16 == 0
    return t[GUARD + shift:GUARD + shift + len(buf)]


def run(cuda, blobs, size, off, keep=None, cap=None, oshift=0, want_records=True):
    """Sizes only, then the build with out_cap = cap (None: the total; "none": sizes only).
    blobs: a device uint8 view.  Returns dict(rc0, total0, records0, off0, rc, total, records,
    off, out, before, after): host arrays, `out` the whole capacity and the guard bytes either
    side of it; rec_off is surrounded by sentinels."""
    import torch

    from k2hash_amd import _native
    from k2hash_amd.batch import _stream_handle
    fn = _native.batch_lib().k2h_amd_ralledata_archive
    n = len(off) - 1
    d_off = torch.from_numpy(np.ascontiguousarray(np.array([int(x) for x in off], np.uint64).view(np.int64))).to(cuda)
    d_keep = torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).to(cuda) if keep is not None else None
    st = _stream_handle(None)
    res = {}

    def call(tag, out, out_cap):
        full = torch.full((GUARD + n + 1 + GUARD,), OFF_FILL, dtype=torch.int64, device=cuda)
        total, recs = ctypes.c_uint64(0xDEAD), ctypes.c_uint64(0xDEAD)
        rc = fn(ctypes.c_void_p(blobs.data_ptr() or 1), size, ctypes.c_void_p(d_off.data_ptr()), n,
                ctypes.c_void_p(d_keep.data_ptr()) if d_keep is not None else None, out, out_cap,
                ctypes.c_void_p(full.data_ptr() + 8 * GUARD), ctypes.byref(recs) if want_records else None,
                ctypes.byref(total), st)
        torch.cuda.synchronize()
        o = full.cpu().numpy().view(np.uint64)
        assert (o[:GUARD] == np.uint64(OFF_FILL)).all(), "words before rec_off written"
        assert (o[GUARD + n + 1:] == np.uint64(OFF_FILL)).all(), "rec_off written past entry n"
        res["rc" + tag], res["total" + tag], res["off" + tag] = rc, total.value, o[GUARD:GUARD + n + 1]
        res["records" + tag] = recs.value if want_records else None
    call("0", None, 0)
    if cap == "none":
        return res
    cap = res["total0"] if cap is None else cap
    buf = torch.full((GUARD + oshift + cap + GUARD,), OUT_FILL, dtype=torch.uint8, device=cuda)
    assert buf.data_ptr() % 16 == 0
    call("", ctypes.c_void_p(buf.data_ptr() + GUARD + oshift), cap)
    h = buf.cpu().numpy()
    res["before"], res["out"], res["after"] = h[:GUARD + oshift], h[GUARD + oshift:GUARD + oshift + cap], h[-GUARD:]
    return res


def check(what, res, want):
    """The whole contract of one successful run against model()'s (bytes, rec_off, records, _)."""
    data, rec_off, records = want[0], want[1], want[2]
    total = int(rec_off[-1])
    for tag in ("0", ""):
        assert res["rc" + tag] == 0, (what, "rc" + tag, res["rc" + tag])
        assert res["total" + tag] == total, (what, "total" + tag, res["total" + tag], total)
        assert res["records" + tag] in (None, records), (what, "records" + tag, res["records" + tag], records)
        bad = np.flatnonzero(res["off" + tag] != rec_off)
        assert bad.size == 0, (what, "rec_off" + tag, f"{bad.size} differ, first at {int(bad[0])}: "
                               f"{int(res['off' + tag][bad[0]])} != {int(rec_off[bad[0]])}")
    assert (res["before"] == OUT_FILL).all(), (what, "bytes before out written")
    assert (res["after"] == OUT_FILL).all(), (what, "bytes after the capacity written")
    assert (res["out"][total:] == OUT_FILL).all(), (what, "bytes from total on written")
    bad = np.flatnonzero(res["out"][:total] != data)
    if bad.size:
        i = int(np.searchsorted(rec_off, bad[0], side="right") - 1)
        raise AssertionError((what, f"{bad.size} of {total} bytes differ, first at {int(bad[0])} = byte "
                              f"{int(bad[0]) - int(rec_off[i])} of the record of blob {i}: "
                              f"{int(res['out'][bad[0]]):#x} != {int(data[bad[0]]):#x}"))


def against_model(cuda, buf, off, what, size=None, keep=None, shift=0, oshift=0, claim=None):
    """The call pair over the stream placed `shift` bytes past a 16-byte boundary into an out of
    exactly the expected bytes `oshift` bytes past one; everything compared with the model.
    claim: the forms the blocks must take (a list), checked before the device is asked."""
    size = len(buf) if size is None else size
    want = model(buf, off, size, keep)
    got_forms = forms(want[3], off)
    assert claim is None or got_forms == claim, (what, got_forms, claim)
    res = run(cuda, place(cuda, buf, shift), size, off, keep, oshift=oshift)
    check(what, res, want)
    return want, got_forms
