"""RALLEDATA producer: packed direct-set blobs with precomputed
hashes, built on the GPU (include/k2hash_amd.h section 4), and the consumer side: a blob
stream checked, routed by hash range and compacted on the GPU (section 4b); and the hop
between the device scans and those two: blobs built straight from the range records of a
scanned import file or archive (section 4c); and a stream's portable exit, the same elements
written as a k2hash archive that loads into a table of any seed (section 4d).

A blob is what K2HShm::GetElementToBinary writes (lib/k2hshmdirect.cc:59-88) on the
packed struct of lib/k2hshmdirect.h:36-47, and what k2h_set_element_by_binary
(lib/k2hash.cc:1562-1581) consumes -- trusting the hash / subhash fields, so a bulk load
fed from these blobs never hashes a key on the CPU.
"""
from __future__ import annotations

import ctypes
import struct
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _native
from .archive import import_scan_device
from .batch import FLAG_STD_FNV, _check_dev, _dev_ptr, _stream_handle, _torch

HEADER = 80  # sizeof(RALLEDATA)
_FIELDS = ("hash", "subhash", "key_length", "val_length", "skey_length", "attrs_length", "key_pos", "val_pos",
           "skey_pos", "attrs_pos")


class Blob(NamedTuple):
    hash: int
    subhash: int
    key: bytes
    val: bytes
    skey: bytes
    attrs: bytes


def parse_blob(b: bytes) -> Blob:
    """Decode one RALLEDATA blob (field order of lib/k2hshmdirect.h:36-47)."""
    f = dict(zip(_FIELDS, struct.unpack_from("<10Q", b, 0)))
    seg = lambda p, n: bytes(b[p:p + n])  # noqa: E731
    return Blob(f["hash"], f["subhash"], seg(f["key_pos"], f["key_length"]), seg(f["val_pos"], f["val_length"]),
                seg(f["skey_pos"], f["skey_length"]), seg(f["attrs_pos"], f["attrs_length"]))


def ralledata_size(n: int, key_bytes: int, val_bytes: int = 0, skey_bytes: int = 0, attr_bytes: int = 0) -> int:
    return int(_native.batch_lib().k2h_amd_ralledata_size(n, key_bytes, val_bytes, skey_bytes, attr_bytes))


def _seg_bytes(off, stream=None) -> int:
    if off is None or off.numel() == 0:
        return 0
    torch = _torch()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        return int(off[-1].item()) - int(off[0].item())


def build_ralledata(keys, key_off, vals=None, val_off=None, skeys=None, skey_off=None, attrs=None, attr_off=None,
                    std_fnv: bool = False, out=None, blob_off=None, stream=None, total: Optional[int] = None):
    """Device form.  Each segment is (uint8 bytes tensor, int64 offsets tensor of n+1) or
    (None, None).  Returns (blobs uint8 tensor, blob_off int64 tensor of n+1).

    The blob size is computed from the first and last offset of every segment, which
    reads them back from the device (a stream sync); a caller that already knows it
    (`ralledata_size`) passes `total` together with `out` and the call stays async."""
    torch = _torch()
    _check_dev(key_off, "key_off", torch.int64)
    n = key_off.numel() - 1
    segs = [(keys, key_off), (vals, val_off), (skeys, skey_off), (attrs, attr_off)]
    args = []
    nbytes = []
    for name, (b, o) in zip(("keys", "vals", "skeys", "attrs"), segs):
        if o is None:
            args += [None, None]
            nbytes.append(0)
            continue
        _check_dev(o, f"{name} offsets", torch.int64)
        _check_dev(b, name, torch.uint8)
        args += [ctypes.c_void_p(b.data_ptr() or 1), _dev_ptr(o)]
        nbytes.append(0 if total is not None and out is not None else _seg_bytes(o, stream))
    if total is None or out is None:
        total = ralledata_size(n, *nbytes)
    elif out.numel() < total:
        raise ValueError("out is smaller than total")
    dev = key_off.device
    if out is None:
        out = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    if blob_off is None:
        blob_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    rc = _native.batch_lib().k2h_amd_build_ralledata(*args, n, _dev_ptr(out), _dev_ptr(blob_off),
                                                     FLAG_STD_FNV if std_fnv else 0, _stream_handle(stream))
    _native.check(rc)
    return out[:total], blob_off


def _csr(parts: Optional[Sequence[bytes]]):
    if parts is None:
        return None, None
    data = np.frombuffer(b"".join(parts), np.uint8) if any(parts) else np.zeros(1, np.uint8)
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in parts])
    return np.ascontiguousarray(data), off


def build_ralledata_host(keys: Sequence[bytes], vals=None, skeys=None, attrs=None, std_fnv: bool = False,
                         device: int = 0):
    """Host form over lists of byte strings (None = segment empty for every record).
    Returns (blobs as one uint8 array, blob offsets n+1 uint64)."""
    n = len(keys)
    segs = [_csr(keys)] + [_csr(x) for x in (vals, skeys, attrs)]
    args, nbytes = [], []
    for d, o in segs:
        if o is None:
            args += [None, None]
            nbytes.append(0)
        else:
            args += [ctypes.c_void_p(d.ctypes.data), ctypes.c_void_p(o.ctypes.data)]
            nbytes.append(int(o[-1]))
    total = ralledata_size(n, *nbytes)
    out = np.zeros(max(total, 1), np.uint8)
    boff = np.zeros(n + 1, np.uint64)
    rc = _native.batch_lib().k2h_amd_build_ralledata_host(*args, n, ctypes.c_void_p(out.ctypes.data),
                                                          ctypes.c_void_p(boff.ctypes.data),
                                                          FLAG_STD_FNV if std_fnv else 0, device)
    _native.check(rc)
    return out[:total], boff


# ------------------------------------------------------------ blobs from scanned records
def _recs_to_ralledata(name: str, width: int, file, recs, std_fnv: bool, stream):
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    _check_dev(recs, "recs", torch.int64)
    if recs.dim() != 2 or recs.shape[1] != width:
        raise ValueError(f"recs must be a contiguous (n, {width}) int64 tensor")
    if recs.device != file.device:
        raise ValueError("file and recs are on different devices")
    n = recs.shape[0]
    fn = getattr(_native.batch_lib(), name)
    fp, rp = ctypes.c_void_p(file.data_ptr() or 1), ctypes.c_void_p(recs.data_ptr() or 1)
    blob_off = torch.empty(n + 1, dtype=torch.int64, device=file.device)
    total = ctypes.c_uint64(0)
    flags = FLAG_STD_FNV if std_fnv else 0

    def call(out, cap):
        _native.check(fn(fp, file.numel(), rp, n, out, cap, _dev_ptr(blob_off), ctypes.byref(total), flags,
                         _stream_handle(stream)))
    call(None, 0)  # sizes only
    out = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=file.device)
    if total.value:
        call(_dev_ptr(out), out.numel())
    return out[:int(total.value)], blob_off


def import_to_ralledata(file, recs, std_fnv: bool = False, stream=None):
    """Blobs of the records of a k2himport file in device memory (k2h_amd_import_ralledata):
    `recs` is the (n, 4) int64 tensor of import_scan_device.  Every record becomes the blob of
    key + NUL and value + NUL, the strings K2HShm::Set(const char*, const char*) stores, with
    the hashes of key + NUL; a record whose ranges leave the file becomes a 0-byte blob.
    Returns (blobs, blob_off): uint8 and int64 (n + 1) device tensors, blob i =
    blobs[blob_off[i]:blob_off[i + 1]], in record order.  Two calls (size, then build), each
    synchronising the stream once."""
    return _recs_to_ralledata("k2h_amd_import_ralledata", 4, file, recs, std_fnv, stream)


def archive_to_ralledata(file, recs, std_fnv: bool = False, stream=None):
    """Blobs of the SCOM_SET_ALL records of a k2hash archive in device memory
    (k2h_amd_archive_ralledata): `recs` is the (n, 13) int64 tensor of archive.scan_device.
    A record with status 0, type 0, a key and all four ranges inside the file becomes the
    blob of its segments as stored; every other record becomes a 0-byte blob.  Returns
    (blobs, blob_off) as import_to_ralledata."""
    return _recs_to_ralledata("k2h_amd_archive_ralledata", 13, file, recs, std_fnv, stream)


def import_file_to_ralledata(file, fmt: str = "tsv", std_fnv: bool = False, stream=None):
    """import_scan_device, then import_to_ralledata: a TSV or mdbm_export file in device
    memory to its blob stream.  Returns (blobs, blob_off)."""
    return import_to_ralledata(file, import_scan_device(file, fmt, stream=stream), std_fnv=std_fnv, stream=stream)


# ------------------------------------------------------------------ the consumer side
# status[i] of check_ralledata (K2H_AMD_RALLE_*): the first that applies, in this order
OK, BAD_SPAN, EMPTY, NO_KEY, BAD_RANGE, BAD_HASH, BAD_SUBHASH = range(7)
STATUS_NAMES = ("OK", "BAD_SPAN", "EMPTY", "NO_KEY", "BAD_RANGE", "BAD_HASH", "BAD_SUBHASH")
ROUTE_TARGET, ROUTE_OLD = 1, 2  # route[i] bits: the stored hash is in the target / the old range
NO_OLD_HASH = (1 << 64) - 1     # old_hash of a HashRange without an old range (lib/k2hshmdirect.cc:119)

HashRange = _native.HashRange


def make_hash_range(target_hash: int, target_max_hash: int, target_hash_range: int = 1, old_hash: int = NO_OLD_HASH,
                    old_max_hash: int = 0) -> HashRange:
    """The selection arguments of K2HShm::GetElementListToBinary (lib/k2hshmdirect.cc:103)."""
    return HashRange(target_hash, target_max_hash, target_hash_range, old_hash, old_max_hash)


class CheckResult(NamedTuple):
    status: object           # uint8 tensor, n
    route: Optional[object]  # uint8 tensor, n (None without a hash range)
    h1: Optional[object]     # int64 tensors, n: the recomputed hashes (None unless want_hashes)
    h2: Optional[object]


def _check_stream(blobs, blob_off, torch):
    _check_dev(blobs, "blobs", torch.uint8)
    _check_dev(blob_off, "blob_off", torch.int64)
    if blob_off.device != blobs.device:
        raise ValueError("blobs and blob_off are on different devices")
    if blob_off.numel() < 1:
        raise ValueError("blob_off needs n + 1 entries")
    return blob_off.numel() - 1


def check_ralledata(blobs, blob_off, hash_range: Optional[HashRange] = None, std_fnv: bool = False,
                    want_hashes: bool = False, stream=None) -> CheckResult:
    """Verify a blob stream on the device (k2h_amd_ralledata_check): blob i =
    blobs[blob_off[i], blob_off[i+1]).  status[i] is OK or the first of BAD_SPAN ..
    BAD_SUBHASH that applies; with `hash_range`, route[i] carries ROUTE_TARGET / ROUTE_OLD for
    the blobs whose status is OK.  Asynchronous on the stream."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    dev = blobs.device
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    route = torch.empty(n, dtype=torch.uint8, device=dev) if hash_range is not None else None
    h1 = torch.empty(n, dtype=torch.int64, device=dev) if want_hashes else None
    h2 = torch.empty(n, dtype=torch.int64, device=dev) if want_hashes else None
    opt = lambda t: _dev_ptr(t) if t is not None else None  # noqa: E731
    rc = _native.batch_lib().k2h_amd_ralledata_check(
        ctypes.c_void_p(blobs.data_ptr() or 1), blobs.numel(), _dev_ptr(blob_off), n,
        ctypes.byref(hash_range) if hash_range is not None else None, FLAG_STD_FNV if std_fnv else 0,
        _dev_ptr(status), opt(route), opt(h1), opt(h2), _stream_handle(stream))
    _native.check(rc)
    return CheckResult(status, route, h1, h2)


class Selected(NamedTuple):
    blobs: object     # uint8 tensor: the kept blobs back to back (None when only counting)
    blob_off: object  # int64 tensor, kept + 1, relative to `blobs`, from 0
    index: object     # int64 tensor, kept: the kept blobs' indices in the input stream
    kept: int
    kept_bytes: int


def select_ralledata(blobs, blob_off, keep, out=None, count_only: bool = False, want_index: bool = True,
                     stream=None) -> Selected:
    """Pack the blobs with keep[i] != 0 (and a valid span) back to back, in order
    (k2h_amd_ralledata_select).  keep: uint8 or bool tensor of n.  Without `out` the kept
    bytes are counted first and an exact buffer is allocated (two calls, each synchronising
    the stream once); an `out` too small for them raises with nothing written.
    count_only: only the counts (blobs, blob_off and index are None)."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    if keep.dtype == torch.bool:
        keep = keep.view(torch.uint8)
    _check_dev(keep, "keep", torch.uint8)
    if keep.numel() != n or keep.device != blobs.device:
        raise ValueError("keep needs n entries on the blobs' device")
    dev = blobs.device
    lib = _native.batch_lib()
    kept, kept_bytes = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def call(o, cap, ooff, idx):
        return lib.k2h_amd_ralledata_select(
            ctypes.c_void_p(blobs.data_ptr() or 1), blobs.numel(), _dev_ptr(blob_off), n, _dev_ptr(keep), o, cap,
            ooff, idx, ctypes.byref(kept), ctypes.byref(kept_bytes), _stream_handle(stream))
    if count_only or out is None:
        _native.check(call(None, 0, None, None))
        if count_only:
            return Selected(None, None, None, int(kept.value), int(kept_bytes.value))
        out = torch.empty(max(int(kept_bytes.value), 1), dtype=torch.uint8, device=dev)
    else:
        _check_dev(out, "out", torch.uint8)
        if out.device != dev:
            raise ValueError("out is on another device than the blobs")
    out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev) if want_index else None
    _native.check(call(_dev_ptr(out), out.numel(), _dev_ptr(out_off), _dev_ptr(index) if want_index else None))
    k, kb = int(kept.value), int(kept_bytes.value)
    return Selected(out[:kb], out_off[:k + 1], index[:k] if want_index else None, k, kb)


PART_MAX = _native.K2H_AMD_PART_MAX
PART_NONE = _native.K2H_AMD_PART_NONE  # part_of[i] of a blob left out (-1 as int32)


class Partitioned(NamedTuple):
    blobs: object      # uint8 tensor: part 0's blobs, then part 1's, ... (None when only counting)
    blob_off: object   # int64 tensor, kept + 1, relative to `blobs`, from 0
    index: object      # int64 tensor, kept: the blobs' indices in the input stream, in output order
    part_of: object    # int32 tensor, n: each input blob's part, -1 (PART_NONE) if left out (want_parts)
    part_first: list   # parts + 1 ints: part p is blobs [part_first[p], part_first[p + 1]) of the output
    part_byte: list    # parts + 1 ints: and bytes [part_byte[p], part_byte[p + 1]) of `blobs`
    kept: int
    kept_bytes: int


def partition_ralledata(blobs, blob_off, parts: int, *, ids=None, owner=None, mask=None, consider=None, out=None,
                        count_only: bool = False, want_index: bool = True, want_parts: bool = False,
                        stream=None) -> Partitioned:
    """Group the blobs of a stream by part, in stream order within each part
    (k2h_amd_ralledata_partition).  Exactly one rule is given: ids, an int32 tensor of n (a blob
    with ids[i] outside [0, parts) is left out); owner=(max_hash, span), part = (stored hash %
    max_hash) // span with parts == ceil(max_hash / span); or mask, part = (stored hash & mask) %
    parts.  The hash rules trust the stored hash and leave out blobs shorter than a header.
    consider: uint8 or bool tensor of n, the blobs that take part (None: all).  Without `out` the
    kept bytes are counted first and an exact buffer is allocated (two calls, each synchronising
    the stream once); an `out` too small for them raises with nothing written.  count_only: only
    the counts and, with want_parts, part_of (blobs, blob_off and index are None)."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    dev = blobs.device
    if (ids is not None) + (owner is not None) + (mask is not None) != 1:
        raise ValueError("exactly one of ids, owner and mask selects the rule")
    if not 1 <= parts <= PART_MAX:
        raise ValueError(f"parts must be 1 .. {PART_MAX}")
    if ids is not None:
        _check_dev(ids, "ids", torch.int32)
        if ids.numel() != n or ids.device != dev:
            raise ValueError("ids needs n entries on the blobs' device")
        rule = _native.PartRule(_native.K2H_AMD_PART_IDS, parts, 0, 0, 0)
    elif owner is not None:
        rule = _native.PartRule(_native.K2H_AMD_PART_OWNER, parts, int(owner[0]), int(owner[1]), 0)
    else:
        rule = _native.PartRule(_native.K2H_AMD_PART_MASK, parts, 0, 0, int(mask))
    if consider is not None:
        if consider.dtype == torch.bool:
            consider = consider.view(torch.uint8)
        _check_dev(consider, "consider", torch.uint8)
        if consider.numel() != n or consider.device != dev:
            raise ValueError("consider needs n entries on the blobs' device")
    lib = _native.batch_lib()
    first, byte = (ctypes.c_uint64 * (parts + 1))(), (ctypes.c_uint64 * (parts + 1))()
    part_of = torch.empty(n, dtype=torch.int32, device=dev) if want_parts else None
    opt = lambda t: ctypes.c_void_p(t.data_ptr() or 1) if t is not None else None  # noqa: E731

    def call(o, cap, ooff, idx, pout):
        return lib.k2h_amd_ralledata_partition(
            ctypes.c_void_p(blobs.data_ptr() or 1), blobs.numel(), _dev_ptr(blob_off), n, ctypes.byref(rule),
            opt(ids), opt(consider), o, cap, ooff, idx, pout, first, byte, _stream_handle(stream))
    if count_only or out is None:
        _native.check(call(None, 0, None, None, opt(part_of)))
        if count_only:
            return Partitioned(None, None, None, part_of, list(first), list(byte), int(first[parts]),
                               int(byte[parts]))
        out = torch.empty(max(int(byte[parts]), 1), dtype=torch.uint8, device=dev)
    else:
        _check_dev(out, "out", torch.uint8)
        if out.device != dev:
            raise ValueError("out is on another device than the blobs")
    out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev) if want_index else None
    _native.check(call(_dev_ptr(out), out.numel(), _dev_ptr(out_off), opt(index), opt(part_of)))
    k, kb = int(first[parts]), int(byte[parts])
    if n == 0:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            out_off[:1] = 0
    return Partitioned(out[:kb], out_off[:k + 1], index[:k] if want_index else None, part_of, list(first), list(byte),
                       k, kb)


SCOM_HEADER = _native.K2H_AMD_SCOM_HEADER  # sizeof(SCOM): the header of an archive record


class Archived(NamedTuple):
    bytes: object    # uint8 tensor: the SET_ALL records back to back, a k2hash archive (None when only counting)
    rec_off: object  # int64 tensor, n + 1: blob i's record is bytes[rec_off[i]:rec_off[i + 1]] (0 bytes: none)
    records: int     # the blobs that yielded a record
    total: int       # rec_off[n]


def ralledata_to_archive(blobs, blob_off, keep=None, out=None, count_only: bool = False, stream=None) -> Archived:
    """Write a blob stream as a k2hash archive on the device (k2h_amd_ralledata_archive): one
    SCOM_SET_ALL record, as K2HArchive::Save writes it, for every blob with keep[i] != 0 (None:
    all), a good span and a header that is not EMPTY, NO_KEY or BAD_RANGE; the stored hashes are
    not looked at, and the result loads into a table of any hash function (k2h_load_archive).
    keep: uint8 or bool tensor of n.  Without `out` the records are sized first and an exact
    buffer is allocated (two calls, each synchronising the stream once); an `out` too small for
    them raises with nothing written.  count_only: only rec_off and the counts (bytes is None).
    A value above 10 MiB still becomes one SET_ALL record (Save would split it; Load does not
    mind)."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    dev = blobs.device
    if keep is not None:
        if keep.dtype == torch.bool:
            keep = keep.view(torch.uint8)
        _check_dev(keep, "keep", torch.uint8)
        if keep.numel() != n or keep.device != dev:
            raise ValueError("keep needs n entries on the blobs' device")
    lib = _native.batch_lib()
    rec_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    records, total = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def call(o, cap):
        _native.check(lib.k2h_amd_ralledata_archive(
            ctypes.c_void_p(blobs.data_ptr() or 1), blobs.numel(), _dev_ptr(blob_off), n,
            _dev_ptr(keep) if keep is not None and n else None, o, cap, _dev_ptr(rec_off), ctypes.byref(records),
            ctypes.byref(total), _stream_handle(stream)))
    if count_only or out is None:
        call(None, 0)  # sizes only
        if count_only:
            return Archived(None, rec_off, int(records.value), int(total.value))
        out = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=dev)
        if not total.value:
            return Archived(out[:0], rec_off, 0, 0)
    else:
        _check_dev(out, "out", torch.uint8)
        if out.device != dev:
            raise ValueError("out is on another device than the blobs")
    call(_dev_ptr(out), out.numel())
    return Archived(out[:int(total.value)], rec_off, int(records.value), int(total.value))


def import_file_to_archive(file, fmt: str = "tsv", stream=None) -> Archived:
    """import_file_to_ralledata, then ralledata_to_archive: a TSV or mdbm_export file in device
    memory converted to k2hash's other bulk format.  Every line becomes the SET_ALL record of
    key + NUL and value + NUL that K2HArchive::Save writes after k2himport's Set."""
    blobs, blob_off = import_file_to_ralledata(file, fmt, stream=stream)
    return ralledata_to_archive(blobs, blob_off, stream=stream)


NO_LATER = (1 << 64) - 1  # by[i] of dedup_ralledata when no later blob has blob i's identity (-1 as int64)


def _consider_arg(consider, n, dev, torch):
    if consider is None:
        return None
    if consider.dtype == torch.bool:
        consider = consider.view(torch.uint8)
    _check_dev(consider, "consider", torch.uint8)
    if consider.numel() != n or consider.device != dev:
        raise ValueError("consider needs n entries on the blobs' device")
    return consider


TIMES_MTIME, TIMES_EXPIRE = _native.K2H_AMD_TIMES_MTIME, _native.K2H_AMD_TIMES_EXPIRE
TIMES_CUT, TIMES_ATTRS = _native.K2H_AMD_TIMES_CUT, _native.K2H_AMD_TIMES_ATTRS


class TimeWindow:
    """The time arguments of K2HShm::GetElementListToBinary (lib/k2hshmdirect.cc:103): start and
    end bound the mtime (pstartts, pendts), now switches the expiry check on (is_expire_check,
    with the clock's value passed in).  Each is a (sec, nsec) tuple or None."""

    def __init__(self, start=None, end=None, now=None):
        self.start, self.end, self.now = start, end, now

    def ctypes(self) -> "_native.TimeWindowStruct":
        flags = 0
        ts = []
        for bit, t in ((_native.K2H_AMD_WIN_START, self.start), (_native.K2H_AMD_WIN_END, self.end),
                       (_native.K2H_AMD_WIN_EXPIRE, self.now)):
            flags |= bit if t is not None else 0
            ts.append(_native.Timespec(*(int(x) for x in t)) if t is not None else _native.Timespec(0, 0))
        return _native.TimeWindowStruct(flags, 0, *ts)


class Times(NamedTuple):
    flags: object   # uint8 tensor, n: TIMES_MTIME | TIMES_EXPIRE | TIMES_CUT | TIMES_ATTRS
    mtime: object   # int64 tensor, (n, 2): sec, nsec; 0, 0 when absent
    expire: object  # int64 tensor, (n, 2)
    keep: object    # uint8 tensor, n


def blob_times(blobs, blob_off, consider=None, window: Optional[TimeWindow] = None, route=None,
               stream=None) -> Times:
    """The builtin mtime and expire inside every blob's serialized attrs, and the time selection
    of GetElementListToBinary (k2h_amd_ralledata_times).  consider: the blobs that take part
    (None: all); a blob that does not, or whose span or header is bad, gets flags 0, zero times
    and keep 0.  keep[i] of a participant: 0 when window.now is given and the blob is expired
    then; else, for a blob with an mtime, 0 when it is before window.start (only for blobs whose
    route byte has ROUTE_OLD; route None: for all) or after window.end; else 1.  Without a
    window keep is the participants.  route: the uint8 tensor of check_ralledata (needs a
    window).  Asynchronous on the stream."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    dev = blobs.device
    consider = _consider_arg(consider, n, dev, torch)
    if route is not None:
        if window is None:
            raise ValueError("route needs a window")
        _check_dev(route, "route", torch.uint8)
        if route.numel() != n or route.device != dev:
            raise ValueError("route needs n entries on the blobs' device")
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    mtime = torch.empty((n, 2), dtype=torch.int64, device=dev)
    expire = torch.empty((n, 2), dtype=torch.int64, device=dev)
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    win = window.ctypes() if window is not None else None
    opt = lambda t: ctypes.c_void_p(t.data_ptr() or 1) if t is not None and n else None  # noqa: E731
    full = lambda t: ctypes.c_void_p(t.data_ptr() or 1)  # noqa: E731
    rc = _native.batch_lib().k2h_amd_ralledata_times(
        full(blobs), blobs.numel(), _dev_ptr(blob_off), n, opt(consider),
        ctypes.byref(win) if win is not None else None, opt(route), full(flags), full(mtime), full(expire),
        full(keep), _stream_handle(stream))
    _native.check(rc)
    return Times(flags, mtime, expire, keep)


def dedup_ralledata(blobs, blob_off, consider=None, want_by: bool = False, count: bool = True, stream=None,
                    pts=None):
    """The blobs of a stream worth feeding to k2h_set_element_by_binary
    (k2h_amd_ralledata_dedup).  Two blobs have the same identity when their stored hash,
    stored subhash, key length and key bytes are equal; blob i is superseded -- keep[i] = 0 --
    when the nearest later blob of its identity exists and neither of the two carries attrs.
    pts: the (sec, nsec) the whole stream will be fed with; with it the mtime rule applies
    instead (k2h_amd_ralledata_dedup_mtime): blob i is superseded by the nearest later blob j of
    its identity when i has no mtime, or both have one and m_i < m_j and m_i < pts -- so blobs
    with attrs are dropped too, and every blob the plain rule drops.
    consider: uint8 or bool tensor of n, the blobs that take part (None: all); a blob that
    does not, or whose span or header is bad, gets keep[i] = 0 and supersedes nothing.
    Returns (keep, by, dropped): keep a uint8 tensor of n; by (want_by) an int64 tensor of n,
    the nearest later participant of the same identity or -1 (NO_LATER as unsigned); dropped
    (count) the number of superseded blobs, which synchronises the stream once -- with
    count=False the call is asynchronous and dropped is None."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    dev = blobs.device
    if consider is not None:
        if consider.dtype == torch.bool:
            consider = consider.view(torch.uint8)
        _check_dev(consider, "consider", torch.uint8)
        if consider.numel() != n or consider.device != dev:
            raise ValueError("consider needs n entries on the blobs' device")
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    by = torch.empty(n, dtype=torch.int64, device=dev) if want_by else None
    dropped = ctypes.c_uint64(0)
    args = (ctypes.c_void_p(blobs.data_ptr() or 1), blobs.numel(), _dev_ptr(blob_off), n,
            _dev_ptr(consider) if consider is not None and n else None, ctypes.c_void_p(keep.data_ptr() or 1),
            _dev_ptr(by) if want_by and n else None, ctypes.byref(dropped) if count else None)
    if pts is None:
        rc = _native.batch_lib().k2h_amd_ralledata_dedup(*args, _stream_handle(stream))
    else:
        ts = _native.Timespec(int(pts[0]), int(pts[1]))
        rc = _native.batch_lib().k2h_amd_ralledata_dedup_mtime(*args, ctypes.byref(ts), _stream_handle(stream))
    _native.check(rc)
    return keep, by, int(dropped.value) if count else None


DIFF_PART, DIFF_FOUND, DIFF_VAL, DIFF_SKEY = (_native.K2H_AMD_DIFF_PART, _native.K2H_AMD_DIFF_FOUND,
                                              _native.K2H_AMD_DIFF_VAL, _native.K2H_AMD_DIFF_SKEY)
DIFF_ATTRS, DIFF_DATA, DIFF_REPEAT, DIFF_APPLY = (_native.K2H_AMD_DIFF_ATTRS, _native.K2H_AMD_DIFF_DATA,
                                                  _native.K2H_AMD_DIFF_REPEAT, _native.K2H_AMD_DIFF_APPLY)
NO_MATCH = (1 << 64) - 1  # match[i] of diff_ralledata when B holds no blob of i's identity (-1 as int64)


class Diff(NamedTuple):
    rel: object           # uint8 tensor, na: DIFF_* bits
    match: object         # int64 tensor, na, or None: the matched blob of B, -1 without one
    seen: object          # uint8 tensor, nb, or None: 1 for a blob of B some blob of A matched
    participants: object  # the four counts (None with count=False): participants of A,
    found: object         # ... those with a held blob of their identity,
    same: object          # ... those of them whose three segments all equal the held blob's,
    apply: object         # ... and the blobs SetElementByBinArray would go on to write (0 without pts)
    feed: object          # uint8 tensor, na, or None without pts: the blobs worth feeding


def diff_ralledata(a_blobs, a_off, b_blobs, b_off, a_consider=None, b_consider=None, pts=None, now=None,
                   want_match: bool = False, want_seen: bool = False, count: bool = True, stream=None) -> Diff:
    """What the incoming stream A changes in a table whose elements the held stream B dumps
    (k2h_amd_ralledata_diff).  Every participant of A is joined with the last participant of B
    of its identity -- stored hash, stored subhash, key length, key bytes -- and the value,
    subkeys and attrs segments of the pair are compared: rel[i] carries DIFF_PART, DIFF_DATA,
    DIFF_FOUND, one of DIFF_VAL / DIFF_SKEY / DIFF_ATTRS per segment that differs, and
    DIFF_REPEAT when another participant of A stores i's hash.  pts and now ((sec, nsec) each,
    given together or not at all): the pts the whole of A will be fed with and the clock then;
    with them DIFF_APPLY says that SetElementByBinArray, meeting the matched blob as the existing
    element, would not return early, and feed is the mask of the blobs worth feeding,
    PART and (REPEAT or (APPLY and (FOUND ? a segment differs : DATA))): feeding them leaves the
    table that feeding all of A leaves, when B holds exactly the table's elements for A's
    identities.  Held elements A does not mention are only reported here (seen == 0);
    delta.delta_log turns them into DEL_KEY records.
    count: the four counts, which synchronises the stream once; with count=False the call is
    asynchronous and they are None."""
    torch = _torch()
    na = _check_stream(a_blobs, a_off, torch)
    nb = _check_stream(b_blobs, b_off, torch)
    dev = a_blobs.device
    if b_blobs.device != dev:
        raise ValueError("the two streams are on different devices")
    if (pts is None) != (now is None):
        raise ValueError("pts and now are given together or not at all")
    a_consider = _consider_arg(a_consider, na, dev, torch)
    b_consider = _consider_arg(b_consider, nb, dev, torch)
    rel = torch.empty(na, dtype=torch.uint8, device=dev)
    match = torch.empty(na, dtype=torch.int64, device=dev) if want_match else None
    seen = torch.empty(nb, dtype=torch.uint8, device=dev) if want_seen else None
    counts = (ctypes.c_uint64 * 4)()
    times = None
    if pts is not None:
        times = _native.DiffTimes(_native.Timespec(int(pts[0]), int(pts[1])), _native.Timespec(int(now[0]), int(now[1])))
    full = lambda t: ctypes.c_void_p(t.data_ptr() or 1)  # noqa: E731
    opt = lambda t, n: ctypes.c_void_p(t.data_ptr() or 1) if t is not None and n else None  # noqa: E731
    rc = _native.batch_lib().k2h_amd_ralledata_diff(
        full(a_blobs), a_blobs.numel(), _dev_ptr(a_off), na, opt(a_consider, na),
        full(b_blobs), b_blobs.numel(), _dev_ptr(b_off), nb, opt(b_consider, nb),
        ctypes.byref(times) if times is not None else None, full(rel), opt(match, na), opt(seen, nb),
        ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64)) if count else None, _stream_handle(stream))
    _native.check(rc)
    feed = None
    if times is not None:
        feed = torch.empty(na, dtype=torch.uint8, device=dev)  # as every output: from the current stream's pool
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            differs = (rel & (DIFF_VAL | DIFF_SKEY | DIFF_ATTRS)) != 0
            change = torch.where((rel & DIFF_FOUND) != 0, differs, (rel & DIFF_DATA) != 0)
            feed.copy_(((rel & DIFF_PART) != 0) & (((rel & DIFF_REPEAT) != 0) | (((rel & DIFF_APPLY) != 0) & change)))
    c = [int(x) for x in counts] if count else [None] * 4
    return Diff(rel, match, seen, c[0], c[1], c[2], c[3], feed)


def route_ralledata(blobs, blob_off, hash_range: HashRange, std_fnv: bool = False, stream=None,
                    dedup: bool = False, window: Optional[TimeWindow] = None, pts=None):
    """What a receiver that owns `hash_range` does with a stream: check it, then keep the
    blobs that are OK and whose hash is in the target range (status == 0 and route & 1).
    window: of those, only the ones GetElementListToBinary's time selection lets through
    (blob_times with the check's route, so the start bound applies to the old range only).
    dedup: of those, also leave out the ones a later one supersedes (dedup_ralledata; with pts
    by the mtime rule).
    Returns (Selected, CheckResult); the kept blobs feed k2h_set_element_by_binary."""
    torch = _torch()
    res = check_ralledata(blobs, blob_off, hash_range, std_fnv=std_fnv, stream=stream)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        keep = ((res.status == OK) & ((res.route & ROUTE_TARGET) != 0)).to(torch.uint8)
    if window is not None:
        timed = blob_times(blobs, blob_off, consider=keep, window=window, route=res.route, stream=stream).keep
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            keep = keep & timed
    if dedup:
        live, _by, _dropped = dedup_ralledata(blobs, blob_off, consider=keep, count=False, stream=stream, pts=pts)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            keep = keep & live
    return select_ralledata(blobs, blob_off, keep, stream=stream), res
