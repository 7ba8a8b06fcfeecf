"""The barrier records of a transaction log, OW_VAL and RENAME, executed on a held RALLEDATA stream
on the device (include/k2hash_amd.h section 5d), and with them a whole log replayed there.

apply.apply_records stops at the first OW_VAL or RENAME.  execute_barrier executes that record --
for OW_VAL the whole run of chunks on the one key, as K2HArchive::Save writes them for every value
above 10 MiB -- in place: the held stream is an arena with room behind its last blob, the call
clears the keep byte of every copy of the addressed key and appends the one blob that holds the
new element.  The next apply_records takes the arena with its keep bytes and compacts the dead
copies away.  replay_log alternates the two until the log is used up.

The ``stream`` argument is that of batch.py's module docstring.  Every call here synchronises the
stream to read its result back.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

from . import _native
from .apply import apply_records
from .archive import _check_recs, fold_device, scan_prehash_device
from .batch import FLAG_STD_FNV, _check_dev, _stream_handle, _torch
from .ralledata import _consider_arg

(BARRIER_EXECUTED, BARRIER_NOT_FOUND, BARRIER_NEW_EXISTS, BARRIER_BAD_RECORD, BARRIER_NOT_A_BARRIER) = (
    _native.K2H_AMD_BARRIER_EXECUTED, _native.K2H_AMD_BARRIER_NOT_FOUND, _native.K2H_AMD_BARRIER_NEW_EXISTS,
    _native.K2H_AMD_BARRIER_BAD_RECORD, _native.K2H_AMD_BARRIER_NOT_A_BARRIER)
BARRIER_CREATED, BARRIER_GAP = _native.K2H_AMD_BARRIER_CREATED, _native.K2H_AMD_BARRIER_GAP
BARRIER_MAX_RUN = _native.K2H_AMD_BARRIER_MAX_RUN
REPLAY_SLACK = 64 << 10   # replay_log: arena bytes beyond the coming barriers' own file bytes


class Executed(NamedTuple):
    outcome: int      # BARRIER_EXECUTED, _NOT_FOUND, _NEW_EXISTS, _BAD_RECORD or _NOT_A_BARRIER
    executed: int     # records executed: the log continues at b + executed
    flags: int        # BARRIER_CREATED | BARRIER_GAP
    appended: int     # bytes of the appended blob
    na: int           # blobs in the arena after the call
    used: int         # bytes in use after the call
    cleared: int      # held copies whose keep byte was cleared
    deciding: int     # the deciding blob's index, -1 when there is none
    value_len: int    # the final value length


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() or 1)


def _barrier_call(held, held_off, held_keep, na, used, file, recs, b, consider, hashes, std_fnv, count_only, stream):
    """(rc, result words) of one k2h_amd_archive_barrier."""
    n = recs.shape[0]
    result = (ctypes.c_uint64 * 8)()
    hp = [None] * 4 if hashes is None else [_ptr(h) for h in hashes]
    flags = (FLAG_STD_FNV if std_fnv else 0) | (_native.K2H_AMD_BARRIER_COUNT_ONLY if count_only else 0)
    rc = _native.batch_lib().k2h_amd_archive_barrier(
        _ptr(held), used, held.numel(), _ptr(held_off), na, _ptr(held_keep), _ptr(file), file.numel(), _ptr(recs), n, b,
        _ptr(consider) if consider is not None else None, *hp, flags,
        ctypes.cast(result, ctypes.POINTER(ctypes.c_uint64)), _stream_handle(stream))
    return rc, [int(x) for x in result]


def _executed(r, na, used, written):
    ok = written and r[0] == BARRIER_EXECUTED
    return Executed(r[0], r[1], r[3], r[2], na + 1 if ok else na, used + r[2] if ok else used, r[4],
                    -1 if r[5] == (1 << 64) - 1 else r[5], r[6])


def execute_barrier(held, held_off, held_keep, na: int, used: int, file, recs, b: int, consider=None, hashes=None,
                    std_fnv: bool = False, count_only: bool = False, stream=None) -> Executed:
    """k2h_amd_archive_barrier: record b of a scanned log executed on the arena.  held: the
    arena's whole allocation (uint8, held.numel() its capacity) of which `used` bytes hold `na`
    blobs; held_off: int64 with room for na + 2 entries, held_off[na] == used; held_keep: uint8
    with room for na + 1, read and written.  recs: the (n, 13) records of scan_device; hashes:
    (h1, h2, new_h1, new_h2) as scan_prehash_device(rename=True) gives them, or None -- then the
    call hashes what it needs, std_fnv choosing the seed.  An EXECUTED call has cleared the keep
    byte of every copy of the record's key, appended one blob at held[used:], written
    held_off[na + 1] and set held_keep[na]; the returned na and used are the arena's new ones.
    Any other outcome, and count_only, write nothing.  An arena too small raises with nothing
    written."""
    torch = _torch()
    _check_dev(held, "held", torch.uint8)
    _check_dev(held_off, "held_off", torch.int64)
    _check_dev(held_keep, "held_keep", torch.uint8)
    _check_dev(file, "file", torch.uint8)
    _check_recs(torch, recs)
    dev = file.device
    n = recs.shape[0]
    if any(t.device != dev for t in (held, held_off, held_keep, recs)):
        raise ValueError("the arena, the file and recs are on different devices")
    if not 0 <= used <= held.numel():
        raise ValueError("used is not inside the arena")
    if held_off.numel() < na + 2 or held_keep.numel() < na + 1:
        raise ValueError("held_off needs room for na + 2 entries and held_keep for na + 1")
    if not 0 <= b < n:
        raise ValueError("b is not a record of the log")
    consider = _consider_arg(consider, n, dev, torch)
    if hashes is not None:
        if len(hashes) != 4:
            raise ValueError("hashes are (h1, h2, new_h1, new_h2)")
        for h in hashes:
            _check_dev(h, "hashes", torch.int64)
            if h.numel() != n or h.device != dev:
                raise ValueError("every hash array needs n entries on the file's device")
        if std_fnv:
            raise ValueError("std_fnv chooses the hash only when hashes is None")
    rc, r = _barrier_call(held, held_off, held_keep, na, used, file, recs, b, consider, hashes, std_fnv, count_only, stream)
    _native.check(rc)
    return _executed(r, na, used, not count_only)


class Replayed(NamedTuple):
    blobs: object       # uint8 tensor: the stream that holds the new state, compact
    blob_off: object    # int64 tensor, blobs + 1
    segments: int       # apply_records calls that wrote a stream
    barriers: int       # execute_barrier calls that executed
    stopped_at: int     # the record the replay ended at; the number of records when it used the log up
    outcome: int        # BARRIER_EXECUTED, or what that record's call answered


def replay_log(held, held_off, file, fold: bool = True, std_fnv: bool = False, err_skip: bool = False,
               stream=None) -> Replayed:
    """A whole transaction log in device memory replayed onto a held stream (held None: no held
    blob), OW_VAL and RENAME included: scan_prehash_device(rename=True) once; the barrier
    positions from the type and status columns; then per segment [s, stop) between barriers
    apply_records -- with fold=True under fold_device's keep over exactly that slice -- into an
    arena, and execute_barrier on that arena in place, s = stop + executed.  Barriers with no
    record between them run back to back on the same arena with no apply in between; after the
    last barrier one apply (of no record, if none follows) brings the arena back to a compact
    stream.

    The arena is the apply's output with slack behind it: the file bytes of the coming barriers'
    records plus 64 KiB.  An executed barrier copies its key's whole element, so a RENAME of a
    large value or the second run onto one can need more: then the call answers with the bytes it
    needs and nothing written, the arena is grown by one device copy, and the call is repeated.

    A barrier that is not executed ends the replay there: `stopped_at` is its index and `outcome`
    what the call answered; blobs / blob_off hold the state before it.  err_skip=True passes over
    NOT_FOUND and BAD_RECORD records as Load does under isErrSkip; NEW_EXISTS always ends the
    replay."""
    torch = _torch()
    _check_dev(file, "file", torch.uint8)
    dev = file.device
    recs, h1, h2, nh1, nh2 = scan_prehash_device(file, rename=True, std_fnv=std_fnv, stream=stream)
    hashes = (h1, h2, nh1, nh2)
    n = recs.shape[0]
    on = torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream())
    bpos = []
    if n:
        with on:
            typ, status = recs[:, 0], recs[:, 12] & 0xFFFFFFFF
            bpos = torch.nonzero(((typ == 4) | (typ == 6)) & (status == 0)).flatten().tolist()
    cur, cur_off, cur_keep = held, held_off, None
    arena: Optional[object] = None
    na = used = 0
    s = bi = segments = barriers = 0
    stopped_at, outcome = n, BARRIER_EXECUTED

    def apply_slice(lo, hi, slack):
        """[lo, hi) applied to the current stream: exact, or into an out with `slack` bytes behind."""
        consider = None
        if fold and hi > lo:
            consider = fold_device(file, recs[lo:hi], h1[lo:hi], count=False, stream=stream).keep
        kw = dict(held_keep=cur_keep, consider=consider, stream=stream)
        if slack is None:
            return apply_records(cur, cur_off, file, recs[lo:hi], h1[lo:hi], h2[lo:hi], **kw)
        c = apply_records(cur, cur_off, file, recs[lo:hi], h1[lo:hi], h2[lo:hi], count_only=True, **kw).counts
        out = torch.empty(c.emitted_bytes + slack, dtype=torch.uint8, device=dev)
        return apply_records(cur, cur_off, file, recs[lo:hi], h1[lo:hi], h2[lo:hi], out=out, **kw), out

    while True:
        while bi < len(bpos) and bpos[bi] < s:
            bi += 1
        if bi == len(bpos) or stopped_at < n:
            break
        stop = bpos[bi]
        group = 1                       # the barriers that follow each other from stop on
        while bi + group < len(bpos) and bpos[bi + group] == stop + group:
            group += 1
        if arena is None or stop > s:   # (an arena and no record before the barrier: back to back)
            with on:
                slack = int(recs[stop:stop + group, 3:12:2].sum().item()) + _native.K2H_AMD_SCOM_HEADER * group + REPLAY_SLACK
            a, arena = apply_slice(s, stop, slack)
            segments += 1
            na, used = a.counts.emitted, a.counts.emitted_bytes
            with on:
                arena_off = torch.empty(na + 1 + group + 1, dtype=torch.int64, device=dev)
                arena_off[:na + 1] = a.blob_off
                arena_keep = torch.ones(na + group + 1, dtype=torch.uint8, device=dev)
        b = stop
        while b < n and bi < len(bpos) and bpos[bi] == b:
            if arena_off.numel() < na + 2:          # (a group's calls are at most its records)
                with on:
                    arena_off = torch.cat([arena_off, torch.empty(group + 1, dtype=torch.int64, device=dev)])
                    arena_keep = torch.cat([arena_keep, torch.ones(group + 1, dtype=torch.uint8, device=dev)])
            rc, r = _barrier_call(arena, arena_off, arena_keep, na, used, file, recs, b, None, hashes, False, False, stream)
            if rc == _native.K2H_AMD_EINVAL and r[0] == BARRIER_EXECUTED and r[2] > arena.numel() - used:
                with on:
                    grown = torch.empty(used + r[2] + REPLAY_SLACK, dtype=torch.uint8, device=dev)
                    grown[:used] = arena[:used]
                arena = grown
                rc, r = _barrier_call(arena, arena_off, arena_keep, na, used, file, recs, b, None, hashes, False, False,
                                      stream)
            _native.check(rc)
            ex = _executed(r, na, used, True)
            if ex.outcome == BARRIER_EXECUTED:
                na, used, barriers = ex.na, ex.used, barriers + 1
                b += ex.executed
            elif err_skip and ex.outcome in (BARRIER_NOT_FOUND, BARRIER_BAD_RECORD):
                b += 1
            else:
                stopped_at, outcome = b, ex.outcome
                break
            while bi < len(bpos) and bpos[bi] < b:
                bi += 1
        s = b
        cur, cur_off, cur_keep = arena[:used], arena_off[:na + 1], arena_keep[:na]
    # the rest of the log, or nothing: the compact stream
    end = n if stopped_at == n else s
    a = apply_slice(s, end, None)
    segments += 1
    return Replayed(a.blobs, a.blob_off, segments, barriers, stopped_at, outcome)
