"""A transaction log applied to a held RALLEDATA stream on the device (include/k2hash_amd.h
section 5c): replication without a table.  A peer holds yesterday's elements as a blob stream and
receives the K2HTransaction log; apply_log gives the stream that holds the new state -- the held
blobs no record touches, copied through, then one blob per touched key that still exists.  With an
empty held stream it turns a log with REPLACE_* and DEL_KEY records into a snapshot, which
archive_to_ralledata (SET_ALL only) cannot.  delta.delta_log is the inverse: from the held and the new
stream to the log that, applied here, gives the new stream's elements.

OW_VAL and RENAME are not executed by these calls.  The first of them ends the log: ``stop`` is
its index.  barrier.execute_barrier (include/k2hash_amd.h section 5d) executes that one record on
this call's output, and the caller calls again with the rest and that stream; barrier.replay_log
is the loop (INTEGRATION.md shows it).

The ``stream`` argument is that of batch.py's module docstring: None means the current torch
stream; otherwise every device operation of the call, the wrappers' own torch ops included, is
ordered on ``stream``.  Every call here synchronises the stream to read its counts back.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

from . import _native
from .archive import _check_recs, fold_device, scan_prehash_device
from .batch import FLAG_STD_FNV, _check_dev, _dev_ptr, _stream_handle, _torch
from .ralledata import _check_stream, _consider_arg

APPLY_TOUCHED, APPLY_SUPERSEDED, APPLY_LEFT_OUT = (_native.K2H_AMD_APPLY_TOUCHED, _native.K2H_AMD_APPLY_SUPERSEDED,
                                                   _native.K2H_AMD_APPLY_LEFT_OUT)


class ApplyCounts(NamedTuple):
    emitted: int        # blobs emitted
    emitted_bytes: int  # their bytes in the output
    unchanged: int      # part 1: held blobs copied through
    touched: int        # held blobs whose identity has applied records
    superseded: int     # held blobs that are an earlier copy of an identity
    absent: int         # touched identities that no longer exist
    applied: int        # records that took part


class Applied(NamedTuple):
    blobs: object         # uint8 tensor: part 1 then part 2, back to back (None when only counting)
    blob_off: object      # int64 tensor, emitted + 1, relative to `blobs`, from 0 (None when only counting)
    origin: object        # int64 tensor, emitted: j for a part-1 blob, na + i (the key's last applied record) for part 2
    touched: object       # uint8 tensor, na: 0, APPLY_TOUCHED, APPLY_SUPERSEDED or APPLY_LEFT_OUT per held blob
    counts: ApplyCounts
    stop: int             # the first considered OW_VAL or RENAME record with status 0; n when there is none
    first_changed: int    # the index of the first part-2 blob: blobs[blob_off[first_changed]:] is the incremental dump


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() or 1)


def apply_records(held, held_off, file, recs, h1=None, h2=None, held_keep=None, consider=None, std_fnv: bool = False,
                  out=None, count_only: bool = False, stream=None) -> Applied:
    """k2h_amd_archive_apply: the records [0, stop) of a scanned log applied to the held stream
    (held None: no held blob).  recs: the (n, 13) records of scan_device; h1 / h2: the keys'
    hashes as prehash_device gives them, both or neither (None: hashed inside the call, std_fnv
    choosing the seed -- they end up in the blobs' headers, so they must be the table's);
    held_keep / consider: uint8 or bool masks of na / n entries.  Without `out` the bytes are
    counted first and an exact buffer is allocated (two calls, each synchronising the stream
    once); an `out` too small raises with nothing written.  count_only: blobs, blob_off and
    origin are None."""
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    _check_recs(torch, recs)
    dev = file.device
    n = recs.shape[0]
    if recs.device != dev:
        raise ValueError("file and recs are on different devices")
    if held is None:
        na = 0
        held, held_off = file[:0], None
    else:
        na = _check_stream(held, held_off, torch)
        if held.device != dev:
            raise ValueError("the held stream and the file are on different devices")
    held_keep = _consider_arg(held_keep, na, dev, torch)
    consider = _consider_arg(consider, n, dev, torch)
    if (h1 is None) != (h2 is None):
        raise ValueError("h1 and h2 are given together or not at all")
    for name, h in (("h1", h1), ("h2", h2)):
        if h is not None:
            _check_dev(h, name, torch.int64)
            if h.numel() != n or h.device != dev:
                raise ValueError(f"{name} needs n entries on the file's device")
    if h1 is not None and std_fnv:
        raise ValueError("std_fnv chooses the hash only when h1 and h2 are None")
    touched = torch.empty(na, dtype=torch.uint8, device=dev)
    counts = (ctypes.c_uint64 * 7)()
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    stop = ctypes.c_uint64(0)
    lib = _native.batch_lib()
    opt = lambda t, k: _ptr(t) if t is not None and k else None  # noqa: E731

    def call(o, cap, ooff, org):
        return lib.k2h_amd_archive_apply(
            opt(held, na), held.numel(), opt(held_off, na), na, opt(held_keep, na), opt(file, n), file.numel(),
            opt(recs, n), n, opt(consider, n), opt(h1, n), opt(h2, n), FLAG_STD_FNV if std_fnv else 0, o, cap, ooff, org,
            opt(touched, na), cp, ctypes.byref(stop), _stream_handle(stream))
    if count_only or out is None:
        _native.check(call(None, 0, None, None))
        if count_only:
            c = ApplyCounts(*(int(x) for x in counts))
            return Applied(None, None, None, touched, c, int(stop.value), c.unchanged)
        out = torch.empty(max(int(counts[1]), 1), dtype=torch.uint8, device=dev)
    else:
        _check_dev(out, "out", torch.uint8)
        if out.device != dev:
            raise ValueError("out is on another device than the file")
    out_off = torch.empty(na + n + 1, dtype=torch.int64, device=dev)
    origin = torch.empty(max(na + n, 1), dtype=torch.int64, device=dev)
    _native.check(call(_ptr(out), out.numel(), _dev_ptr(out_off), _dev_ptr(origin)))
    c = ApplyCounts(*(int(x) for x in counts))
    return Applied(out[:c.emitted_bytes], out_off[:c.emitted + 1], origin[:c.emitted], touched, c, int(stop.value),
                   c.unchanged)


def apply_log(held, held_off, file, fold: bool = True, std_fnv: bool = False, stream=None) -> Applied:
    """A log in device memory applied to a held stream (held None: log -> snapshot):
    scan_prehash_device; the stop from the record columns; with fold=True fold_device over the
    prefix [0, stop) alone (its keep is valid as a consider mask only for exactly the records the
    apply sees), which spares every key's anchor the walk over records that no longer matter;
    then apply_records over the prefix, count and fill.  `stop` is the index, in the scanned
    log, of the OW_VAL or RENAME record the caller has to handle itself (the number of records
    when there is none); file[recs[stop, 1]:] is the rest of the log."""
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    recs, h1, h2 = scan_prehash_device(file, std_fnv=std_fnv, stream=stream)[:3]
    n = recs.shape[0]
    stop = n
    if n:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            typ, status = recs[:, 0], recs[:, 12] & 0xFFFFFFFF
            barrier = ((typ == 4) | (typ == 6)) & (status == 0)
            first = torch.where(barrier, torch.arange(n, device=file.device), n).min()
            stop = int(first.item())
    recs, h1, h2 = recs[:stop], h1[:stop], h2[:stop]
    consider: Optional[object] = None
    if fold and stop:
        consider = fold_device(file, recs, h1, count=False, stream=stream).keep
    a = apply_records(held, held_off, file, recs, h1, h2, consider=consider, stream=stream)
    return a._replace(stop=stop)
