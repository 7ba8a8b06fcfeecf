"""Bulk key streams: keys at arbitrary ranges of a buffer, and
k2hash archive files (include/k2hash_amd.h section 5).

An archive is what K2HArchive::Save writes and K2HArchive::Load replays record by
record, hashing each key on the CPU inside ReplaceAll / Remove / Rename
(lib/k2harchive.cc:82-383).  scan() walks the records the way Load does; prehash()
hashes every key of the file in one GPU batch.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np

from . import _native
from .batch import FLAG_STD_FNV, _check_dev, _dev_ptr, _stream_handle, _torch

FLAG_CSTR = _native.K2H_AMD_FLAG_CSTR
SCOM_SET_ALL, SCOM_REPLACE_VAL, SCOM_REPLACE_SKEY, SCOM_DEL_KEY, SCOM_OW_VAL, SCOM_REPLACE_ATTRS, SCOM_RENAME = range(7)
STATUS_OK, STATUS_BAD_TYPE, STATUS_TRUNCATED = 0, 1, 2
STATUS_NO_MAGIC = 3  # scan_device only: the chain of records arrives where no "\nK2H_" starts

# struct k2h_amd_archive_rec (include/k2hash_amd.h)
REC_DTYPE = np.dtype([("type", "<i8"), ("offset", "<u8"), ("key_off", "<u8"), ("key_len", "<u8"),
                      ("val_off", "<u8"), ("val_len", "<u8"), ("skey_off", "<u8"), ("skey_len", "<u8"),
                      ("attrs_off", "<u8"), ("attrs_len", "<u8"), ("exdata_off", "<u8"), ("exdata_len", "<u8"),
                      ("status", "<i4"), ("reserved", "<i4")])


def _buf(data) -> np.ndarray:
    return np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
        np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)


def scan(data) -> np.ndarray:
    """Records of an archive (structured array, REC_DTYPE), in file order."""
    f = _buf(data)
    ptr = ctypes.c_void_p(f.ctypes.data if f.size else 1)
    lib = _native.batch_lib()
    cnt = ctypes.c_uint64()
    _native.check(lib.k2h_amd_archive_scan(ptr, f.size, None, 0, ctypes.byref(cnt)))
    recs = np.zeros(cnt.value, REC_DTYPE)
    _native.check(lib.k2h_amd_archive_scan(ptr, f.size, ctypes.c_void_p(recs.ctypes.data if recs.size else 1),
                                           recs.size, ctypes.byref(cnt)))
    return recs


def prehash(data, recs=None, rename: bool = False, std_fnv: bool = False, device: int = 0):
    """(h1, h2[, new_h1, new_h2]) of every record's key (uint64 arrays, 0 for records whose
    status is not STATUS_OK); with rename=True also the new key of SCOM_RENAME records."""
    f = _buf(data)
    if recs is None:
        recs = scan(f)
    n = recs.size
    h1, h2 = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    nh1, nh2 = (np.zeros(n, np.uint64), np.zeros(n, np.uint64)) if rename else (None, None)
    p = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None  # noqa: E731
    if n:
        _native.check(_native.batch_lib().k2h_amd_archive_prehash_host(
            ctypes.c_void_p(f.ctypes.data if f.size else 1), f.size, p(recs), n, p(h1), p(h2), p(nh1), p(nh2),
            FLAG_STD_FNV if std_fnv else 0, device))
    return (h1, h2, nh1, nh2) if rename else (h1, h2)


REC_WORDS = REC_DTYPE.itemsize // 8  # a record as a row of 13 int64: status in the low half of column 12


def scan_device(file, stream=None):
    """scan for an archive already in device memory (uint8 device tensor), with no host
    pass (k2h_amd_archive_scan_device).  Returns an (n, 13) int64 device tensor, each row one
    struct k2h_amd_archive_rec (recs_to_numpy gives the REC_DTYPE view).  Where the chain of
    records arrives at an offset that does not start with "\\nK2H_", the scan ends with one
    record of status STATUS_NO_MAGIC (the host scan walks on)."""
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    lib = _native.batch_lib()
    fp = ctypes.c_void_p(file.data_ptr() or 1)
    cnt = ctypes.c_uint64()
    # one pass when the guess holds (records of >= 128 bytes on average); otherwise the call
    # reports the count with K2H_AMD_EINVAL and a second pass fills exact storage
    cap = max(1024, file.numel() // 128)
    rc = 0
    for _ in range(2):
        recs = torch.empty((cap, REC_WORDS), dtype=torch.int64, device=file.device)
        rc = lib.k2h_amd_archive_scan_device(fp, file.numel(), _dev_ptr(recs), cap, ctypes.byref(cnt),
                                             _stream_handle(stream))
        if not (rc == _native.K2H_AMD_EINVAL and cnt.value > cap):
            break
        cap = cnt.value
    _native.check(rc)
    return recs[: cnt.value]


def recs_to_numpy(t) -> np.ndarray:
    """The records of scan_device as a REC_DTYPE array on the host."""
    a = np.ascontiguousarray(t.detach().cpu().numpy()).reshape(-1, REC_WORDS)
    return a.view(REC_DTYPE).reshape(-1)


def _check_recs(torch, recs):
    _check_dev(recs, "recs", torch.int64)
    if recs.dim() != 2 or recs.shape[1] != REC_WORDS or not recs.is_contiguous():
        raise ValueError(f"recs must be a contiguous (n, {REC_WORDS}) int64 tensor")


def prehash_device(file, recs, rename: bool = False, std_fnv: bool = False, stream=None):
    """(h1, h2[, new_h1, new_h2]) int64 device tensors of every record's key hashed as
    stored, from the device-resident file and the records of scan_device (asynchronous).
    Zeros for a record whose status is not STATUS_OK or whose key range is not inside the
    file; with rename=True also the new key (exdata) of SCOM_RENAME records."""
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    _check_recs(torch, recs)
    n = recs.shape[0]
    out = [torch.empty(n, dtype=torch.int64, device=file.device) for _ in range(4 if rename else 2)]
    ptrs = [_dev_ptr(x) for x in out] + [None] * (4 - len(out))
    _native.check(_native.batch_lib().k2h_amd_archive_prehash(
        ctypes.c_void_p(file.data_ptr() or 1), file.numel(), _dev_ptr(recs), n, *ptrs,
        FLAG_STD_FNV if std_fnv else 0, _stream_handle(stream)))
    return tuple(out)


def scan_prehash_device(file, rename: bool = False, std_fnv: bool = False, stream=None):
    """scan_device + prehash_device in one call (k2h_amd_archive_scan_prehash_device):
    (recs, h1, h2[, new_h1, new_h2])."""
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    lib = _native.batch_lib()
    fp = ctypes.c_void_p(file.data_ptr() or 1)
    flags = FLAG_STD_FNV if std_fnv else 0
    cnt = ctypes.c_uint64()
    cap = max(1024, file.numel() // 128)  # as scan_device: one pass when the guess holds
    rc = 0
    for _ in range(2):
        recs = torch.empty((cap, REC_WORDS), dtype=torch.int64, device=file.device)
        out = [torch.empty(cap, dtype=torch.int64, device=file.device) for _ in range(4 if rename else 2)]
        ptrs = [_dev_ptr(x) for x in out] + [None] * (4 - len(out))
        rc = lib.k2h_amd_archive_scan_prehash_device(fp, file.numel(), _dev_ptr(recs), cap, ctypes.byref(cnt), *ptrs,
                                                     flags, _stream_handle(stream))
        if not (rc == _native.K2H_AMD_EINVAL and cnt.value > cap):
            break
        cap = cnt.value
    _native.check(rc)
    n = cnt.value
    return (recs[:n],) + tuple(x[:n] for x in out)


NO_LATER = (1 << 64) - 1  # by[i] without a later record of the same key (-1 in the int64 tensor)


class Folded(NamedTuple):
    keep: object              # uint8 tensor, n: 1 for the records that still matter
    by: Optional[object]      # int64 tensor, n (want_by): the nearest later participant of the same key, or -1
    dropped: Optional[int]    # the number of dropped participants (count)
    recs: object              # the (n, 13) int64 records the fold ran over


def fold_device(file, recs=None, h1=None, want_by: bool = False, count: bool = True, stream=None) -> Folded:
    """The records of a transaction archive in device memory that still matter under
    K2HArchive::Load's rule (k2h_amd_archive_fold): record i is dropped -- keep[i] = 0 -- when
    the fields it writes (SET_ALL: the value, and subkeys / attrs when its own are non-empty;
    REPLACE_*: the one field; DEL_KEY: all three) are all written again by later records of its
    key, before any OW_VAL or RENAME of that key and any RENAME of the log.  Replaying the kept
    records in order leaves the table the whole log leaves.  Records Load skips get keep 0.
    recs: the records of scan_device (None: scan_prehash_device runs here and its hashes are
    passed on); h1: k2h_hash of each key as prehash_device gives it (only a grouping key; None
    with recs given: computed inside the call).  The call synchronises the stream once after
    its link stage, once per cover round (about log2 of the longest run of one key's records)
    and once more for the count."""
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    if recs is None:
        recs, h1 = scan_prehash_device(file, stream=stream)[:2]
    _check_recs(torch, recs)
    n = recs.shape[0]
    dev = file.device
    if recs.device != dev:
        raise ValueError("file and recs are on different devices")
    if h1 is not None:
        _check_dev(h1, "h1", torch.int64)
        if h1.numel() != n or h1.device != dev:
            raise ValueError("h1 needs n entries on the file's device")
    keep = torch.empty(n, dtype=torch.uint8, device=dev)
    by = torch.empty(n, dtype=torch.int64, device=dev) if want_by else None
    dropped = ctypes.c_uint64(0)
    _native.check(_native.batch_lib().k2h_amd_archive_fold(
        ctypes.c_void_p(file.data_ptr() or 1), file.numel(), ctypes.c_void_p(recs.data_ptr() or 1), n,
        _dev_ptr(h1) if h1 is not None and n else None, ctypes.c_void_p(keep.data_ptr() or 1),
        _dev_ptr(by) if want_by and n else None, ctypes.byref(dropped) if count else None, _stream_handle(stream)))
    return Folded(keep, by, int(dropped.value) if count else None, recs)


class Compacted(NamedTuple):
    bytes: object      # uint8 tensor: the compacted archive, the kept records byte for byte, in order
    index: object      # int64 tensor, kept: the kept records' indices in the input
    kept: int
    kept_bytes: int
    records: int       # records of the input


def compact_device(file, stream=None) -> Compacted:
    """A transaction archive in device memory compacted by Load's rule: scan_prehash_device,
    fold_device, then k2h_amd_ralledata_select as the byte copier over the records' own spans
    (record i = file[offset[i], offset[i + 1]), the last one 104 + its five lengths long).  The
    output is a k2hash archive that K2HArchive::Load replays into the table the input gives."""
    torch = _torch()
    from .ralledata import select_ralledata  # (ralledata imports this module)
    folded = fold_device(file, count=False, stream=stream)
    recs = folded.recs
    n = recs.shape[0]
    if n == 0:
        return Compacted(file[:0].clone(), torch.empty(0, dtype=torch.int64, device=file.device), 0, 0, 0)
    rec_off = torch.empty(n + 1, dtype=torch.int64, device=file.device)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rec_off[:n] = recs[:, 1]
        rec_off[n] = recs[n - 1, 1] + _native.K2H_AMD_SCOM_HEADER + recs[n - 1, 3:12:2].sum()
    sel = select_ralledata(file, rec_off, folded.keep, stream=stream)
    return Compacted(sel.blobs, sel.index, sel.kept, sel.kept_bytes, n)


def hash_ranges(base, starts, lens, second: bool = False, cstr: bool = False, std_fnv: bool = False, stream=None):
    """Device form: key i = base[starts[i] : starts[i] + lens[i]] (uint8 / int64 / int64
    device tensors).  cstr=True hashes key + NUL (K2HShm::Set(const char*))."""
    torch = _torch()
    _check_dev(base, "base", torch.uint8)
    _check_dev(starts, "starts", torch.int64)
    _check_dev(lens, "lens", torch.int64)
    n = starts.numel()
    h1 = torch.empty(n, dtype=torch.int64, device=base.device)
    h2 = torch.empty(n, dtype=torch.int64, device=base.device) if second else None
    flags = (FLAG_CSTR if cstr else 0) | (FLAG_STD_FNV if std_fnv else 0)
    rc = _native.batch_lib().k2h_amd_hash_ranges(ctypes.c_void_p(base.data_ptr() or 1), _dev_ptr(starts),
                                                 _dev_ptr(lens), n, _dev_ptr(h1),
                                                 _dev_ptr(h2) if h2 is not None else None, flags,
                                                 _stream_handle(stream))
    _native.check(rc)
    return h1, h2


# ---------------------------------------------------------------------------
# k2himport inputs (tests/k2himport.cc:74-117): TSV and mdbm_export files.
# ---------------------------------------------------------------------------
IMPORT_TSV, IMPORT_MDBM = _native.K2H_AMD_IMPORT_TSV, _native.K2H_AMD_IMPORT_MDBM
# struct k2h_amd_import_rec (include/k2hash_amd.h)
IMPORT_DTYPE = np.dtype([("key_off", "<u8"), ("key_len", "<u8"), ("val_off", "<u8"), ("val_len", "<u8")])


def import_scan(data, fmt: str = "tsv") -> np.ndarray:
    """Records of a k2himport input, split exactly as the tool's getline loops do, each key
    and value as the C string K2HShm::Set(const char*, const char*) stores (lengths are
    strlen).  fmt: "tsv" or "mdbm"; a bad mdbm header raises (the tool exits)."""
    f = _buf(data)
    code = {"tsv": IMPORT_TSV, "mdbm": IMPORT_MDBM}[fmt]
    ptr = ctypes.c_void_p(f.ctypes.data if f.size else 1)
    lib = _native.batch_lib()
    cnt = ctypes.c_uint64()
    _native.check(lib.k2h_amd_import_scan(ptr, f.size, code, None, 0, ctypes.byref(cnt)))
    recs = np.zeros(cnt.value, IMPORT_DTYPE)
    _native.check(lib.k2h_amd_import_scan(ptr, f.size, code, ctypes.c_void_p(recs.ctypes.data if recs.size else 1),
                                          recs.size, ctypes.byref(cnt)))
    return recs


def import_prehash(data, recs=None, fmt: str = "tsv", std_fnv: bool = False, device: int = 0):
    """(h1, h2) of every record's key hashed as key + NUL on the GPU -- the bytes
    K2HShm::Set(const char*) hashes (lib/k2hshm.cc:2081-2083)."""
    f = _buf(data)
    if recs is None:
        recs = import_scan(f, fmt)
    n = recs.size
    h1, h2 = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    if n:
        _native.check(_native.batch_lib().k2h_amd_import_prehash_host(
            ctypes.c_void_p(f.ctypes.data if f.size else 1), f.size, ctypes.c_void_p(recs.ctypes.data), n,
            ctypes.c_void_p(h1.ctypes.data), ctypes.c_void_p(h2.ctypes.data), FLAG_STD_FNV if std_fnv else 0,
            device))
    return h1, h2


def import_scan_device(file, fmt: str = "tsv", stream=None):
    """import_scan for a file already in device memory (uint8 device tensor), with no
    host pass (k2h_amd_import_scan_device).  Returns an (n, 4) int64 device tensor of
    (key_off, key_len, val_off, val_len) rows -- struct k2h_amd_import_rec."""
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    code = {"tsv": IMPORT_TSV, "mdbm": IMPORT_MDBM}[fmt]
    lib = _native.batch_lib()
    fp = ctypes.c_void_p(file.data_ptr() or 1)
    cnt = ctypes.c_uint64()
    # one pass when the guess holds (records of >= 64 bytes on average); otherwise the
    # call reports the count with K2H_AMD_EINVAL and a second pass fills exact storage
    cap = max(1024, file.numel() // 64)
    recs = torch.empty((cap, 4), dtype=torch.int64, device=file.device)
    rc = lib.k2h_amd_import_scan_device(fp, file.numel(), code, _dev_ptr(recs), cap, ctypes.byref(cnt),
                                        _stream_handle(stream))
    if rc == _native.K2H_AMD_EINVAL and cnt.value > cap:
        recs = torch.empty((cnt.value, 4), dtype=torch.int64, device=file.device)
        rc = lib.k2h_amd_import_scan_device(fp, file.numel(), code, _dev_ptr(recs), cnt.value, ctypes.byref(cnt),
                                            _stream_handle(stream))
    _native.check(rc)
    return recs[: cnt.value]


def import_prehash_device(file, recs, std_fnv: bool = False, stream=None):
    """(h1, h2) device tensors of every record's key hashed as key + NUL, from the
    device-resident file and the records of import_scan_device."""
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    _check_dev(recs, "recs", torch.int64)
    if recs.dim() != 2 or recs.shape[1] != 4 or not recs.is_contiguous():
        raise ValueError("recs must be a contiguous (n, 4) int64 tensor")
    n = recs.shape[0]
    h1 = torch.empty(n, dtype=torch.int64, device=file.device)
    h2 = torch.empty(n, dtype=torch.int64, device=file.device)
    _native.check(_native.batch_lib().k2h_amd_import_prehash(
        ctypes.c_void_p(file.data_ptr() or 1), file.numel(), _dev_ptr(recs), n, _dev_ptr(h1), _dev_ptr(h2),
        FLAG_STD_FNV if std_fnv else 0, _stream_handle(stream)))
    return h1, h2


def import_scan_prehash_device(file, fmt: str = "tsv", std_fnv: bool = False, stream=None):
    """import_scan_device + import_prehash_device in one call: the records and their keys'
    (h1, h2) from the same kernel (k2h_amd_import_scan_prehash_device)."""
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    code = {"tsv": IMPORT_TSV, "mdbm": IMPORT_MDBM}[fmt]
    lib = _native.batch_lib()
    fp = ctypes.c_void_p(file.data_ptr() or 1)
    flags = FLAG_STD_FNV if std_fnv else 0
    cnt = ctypes.c_uint64()
    rc = 0
    cap = max(1024, file.numel() // 64)  # as import_scan_device: one pass when the guess holds
    for _ in range(2):
        recs = torch.empty((cap, 4), dtype=torch.int64, device=file.device)
        h1 = torch.empty(cap, dtype=torch.int64, device=file.device)
        h2 = torch.empty(cap, dtype=torch.int64, device=file.device)
        rc = lib.k2h_amd_import_scan_prehash_device(fp, file.numel(), code, _dev_ptr(recs), cap, ctypes.byref(cnt),
                                                    _dev_ptr(h1), _dev_ptr(h2), flags, _stream_handle(stream))
        if not (rc == _native.K2H_AMD_EINVAL and cnt.value > cap):
            break
        cap = cnt.value
    _native.check(rc)
    n = cnt.value
    return recs[:n], h1[:n], h2[:n]
