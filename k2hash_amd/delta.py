"""From two dumps to a log (include/k2hash_amd.h section 4d'): yesterday's held stream and
today's stream give the transaction log that K2HArchive::Load replays onto yesterday's table to
get today's -- SET_ALL for new keys, one REPLACE_VAL / REPLACE_SKEY / REPLACE_ATTRS per field that
differs (empty data clears the field), DEL_KEY for held keys the new stream no longer has.  It
is the inverse of apply.apply_log, which replays the same log onto yesterday's stream: a sender
with two dumps in device memory ships the delta, not a dump, and
``apply_log(held, held_off, delta_log(new, new_off, held, held_off).log)`` holds the elements of
``new``.

The ``stream`` argument is that of batch.py's module docstring: None means the current torch
stream; otherwise every device operation of the call, the wrappers' own torch ops included, is
ordered on ``stream``.  Every call here synchronises the stream to read its counts back.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

from . import _native
from .batch import _check_dev, _dev_ptr, _stream_handle, _torch
from .ralledata import _check_stream, _consider_arg, diff_ralledata

DELTA_SET_ALL, DELTA_REPLACE_VAL, DELTA_REPLACE_SKEY = (_native.K2H_AMD_DELTA_SET_ALL, _native.K2H_AMD_DELTA_REPLACE_VAL,
                                                        _native.K2H_AMD_DELTA_REPLACE_SKEY)
DELTA_REPLACE_ATTRS, DELTA_DEL_KEY = _native.K2H_AMD_DELTA_REPLACE_ATTRS, _native.K2H_AMD_DELTA_DEL_KEY


class DeltaCounts(NamedTuple):
    records: int        # records written
    bytes: int          # their bytes
    set_all: int        # per type, in the order of the DELTA_* bits
    replace_val: int
    replace_skey: int
    replace_attrs: int
    del_key: int
    refused: int        # slots whose bits asked for a record but whose blob is no participant


class Delta(NamedTuple):
    log: object       # uint8 tensor: the records back to back, a k2hash archive (None when only counting)
    slot_off: object  # int64 tensor, na + nb + 1: slot s's records are log[slot_off[s]:slot_off[s + 1]] (None when only counting)
    made: object      # uint8 tensor, na + nb, or None: a DELTA_* bit per record the slot yielded
    counts: DeltaCounts


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() or 1)


def delta_records(a, a_off, rel, b, b_off, seen, b_consider=None, out=None, count_only: bool = False,
                  want_made: bool = False, stream=None) -> Delta:
    """k2h_amd_ralledata_delta: A (a, a_off) is the new stream, B (b, b_off) the held one, rel
    and seen what diff_ralledata (without pts, want_seen=True) said of the two under the same
    consider masks.  A blob i is slot i, B blob j slot na + j.  seen None: no deletions, and b /
    b_off may be None.  Without `out` the bytes are counted first and an exact buffer is
    allocated (two calls, each synchronising the stream once); an `out` too small raises with
    nothing written.  count_only: log and slot_off are None."""
    torch = _torch()
    na = _check_stream(a, a_off, torch)
    dev = a.device
    _check_dev(rel, "rel", torch.uint8)
    if rel.numel() != na or rel.device != dev:
        raise ValueError("rel needs na entries on the streams' device")
    if b is None:
        if seen is not None:
            raise ValueError("seen is given without the held stream")
        nb, b, b_off = 0, a[:0], None
    else:
        nb = _check_stream(b, b_off, torch)
        if b.device != dev:
            raise ValueError("the two streams are on different devices")
    if seen is not None:
        if seen.dtype == torch.bool:
            seen = seen.view(torch.uint8)
        _check_dev(seen, "seen", torch.uint8)
        if seen.numel() != nb or seen.device != dev:
            raise ValueError("seen needs nb entries on the streams' device")
    b_consider = _consider_arg(b_consider, nb, dev, torch)
    made = torch.empty(na + nb, dtype=torch.uint8, device=dev) if want_made else None
    counts = (ctypes.c_uint64 * 8)()
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    lib = _native.batch_lib()
    opt = lambda t, k: _ptr(t) if t is not None and k else None  # noqa: E731

    def call(o, cap, soff):
        return lib.k2h_amd_ralledata_delta(
            opt(a, na), a.numel(), opt(a_off, na), na, opt(rel, na), opt(b, nb), b.numel(), opt(b_off, nb), nb,
            opt(b_consider, nb), opt(seen, nb), o, cap, soff, opt(made, na + nb), cp, _stream_handle(stream))
    if count_only or out is None:
        _native.check(call(None, 0, None))
        if count_only:
            return Delta(None, None, made, DeltaCounts(*(int(x) for x in counts)))
        out = torch.empty(max(int(counts[1]), 1), dtype=torch.uint8, device=dev)
    else:
        _check_dev(out, "out", torch.uint8)
        if out.device != dev:
            raise ValueError("out is on another device than the streams")
    slot_off = torch.empty(na + nb + 1, dtype=torch.int64, device=dev)
    _native.check(call(_ptr(out), out.numel(), _dev_ptr(slot_off)))
    c = DeltaCounts(*(int(x) for x in counts))
    return Delta(out[:c.bytes], slot_off, made, c)


def _last_copies(blobs, blob_off, consider, stream):
    """The mask of the last considered copy of every identity: a count-only apply over an empty
    log marks the earlier copies APPLY_SUPERSEDED and the blobs left out APPLY_LEFT_OUT."""
    from .apply import apply_records
    torch = _torch()
    recs = torch.empty((0, 13), dtype=torch.int64, device=blobs.device)
    touched = apply_records(blobs, blob_off, blobs[:0], recs, held_keep=consider, count_only=True, stream=stream).touched
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        return (touched == 0).to(torch.uint8)


def delta_log(new, new_off, held, held_off, new_consider=None, held_consider=None, last_copies: bool = True,
              stream=None, want_made: bool = False) -> Delta:
    """The log that turns the held stream into the new one: diff_ralledata(new, held,
    want_seen=True, count=False) without times, then delta_records.  The rule is right only when
    each stream has one participant per identity -- two new-key copies in `new` would give two
    SET_ALLs of which the second cannot clear what the first set, and an earlier copy in `held`
    is not seen and would delete a key `new` still has -- so with last_copies=True each stream
    is first reduced to the last considered copy of every identity (a count-only apply_records
    over an empty log; its touched == 0 is the consider mask of the diff and of the delta).
    last_copies=False is for callers whose streams are dumps, one blob per key."""
    torch = _torch()
    na = _check_stream(new, new_off, torch)
    nb = _check_stream(held, held_off, torch)
    dev = new.device
    new_consider = _consider_arg(new_consider, na, dev, torch)
    held_consider = _consider_arg(held_consider, nb, dev, torch)
    if last_copies:
        if na:
            new_consider = _last_copies(new, new_off, new_consider, stream)
        if nb:
            held_consider = _last_copies(held, held_off, held_consider, stream)
    d = diff_ralledata(new, new_off, held, held_off, new_consider, held_consider, want_seen=True, count=False,
                       stream=stream)
    return delta_records(new, new_off, d.rel, held, held_off, d.seen, b_consider=held_consider, want_made=want_made,
                         stream=stream)
