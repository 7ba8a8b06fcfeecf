"""Keys looked up in a held blob stream (include/k2hash_amd.h section 4e): what does the stream
hold for this key?  ``index_stream`` sorts the held stream once into an index, ``find_keys``
looks a batch of keys up through it -- K2HShm::Get for a batch, answered from device memory with
no table -- and ``fetch_segments`` gathers one segment of a list of blobs into a packed CSR
column, the inverse of build_ralledata.  ``get_values`` is find followed by a fetch of the values
of the keys that were found and have not expired.

The ``stream`` argument is that of batch.py's module docstring: None means the current torch
stream; otherwise every device operation of the call, the wrappers' own torch ops included, is
ordered on ``stream``.  index_stream and find_keys do not wait for the device with count=False;
fetch_segments synchronises the stream once per call of the library, twice in all.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

from . import _native
from .batch import _check_dev, _stream_handle, _torch
from .ralledata import _check_stream, _consider_arg

FIND_PART, FIND_FOUND, FIND_ATTRS = _native.K2H_AMD_FIND_PART, _native.K2H_AMD_FIND_FOUND, _native.K2H_AMD_FIND_ATTRS
FIND_EXPIRED, FIND_BAD_INDEX = _native.K2H_AMD_FIND_EXPIRED, _native.K2H_AMD_FIND_BAD_INDEX
SEGMENTS = {"key": _native.K2H_AMD_SEG_KEY, "value": _native.K2H_AMD_SEG_VAL, "subkeys": _native.K2H_AMD_SEG_SKEY,
            "attrs": _native.K2H_AMD_SEG_ATTRS}


class StreamIndex(NamedTuple):
    buffer: object        # uint8 tensor, opaque: valid for exactly the stream it was built from
    n: int                # the stream's blobs
    size: int             # the stream's bytes
    participants: object  # int, or None with count=False


class FindCounts(NamedTuple):
    part: int     # queries that take part
    found: int
    expired: int


class Found(NamedTuple):
    match: object   # int64 tensor, m: the blob index, -1 (~0) where nothing matched; None with want_match=False
    status: object  # uint8 tensor, m: FIND_* bits
    hit: object     # uint8 tensor, n: 1 for a blob that is some query's match; None without want_hit
    counts: object  # FindCounts, or None with count=False


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() or 1)


def _opt(t, k=1):
    return _ptr(t) if t is not None and k else None


def index_size(n: int) -> int:
    """k2h_amd_ralledata_index_size: the bytes of the index of a stream of n blobs."""
    return int(_native.batch_lib().k2h_amd_ralledata_index_size(n))


def index_stream(blobs, blob_off, consider=None, count: bool = True, stream=None) -> StreamIndex:
    """k2h_amd_ralledata_index: the stream's participants (consider: uint8 or bool mask, n
    entries) gathered and sorted once.  count=False: participants is None and nothing waits for
    the device."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    dev = blobs.device
    consider = _consider_arg(consider, n, dev, torch)
    lib = _native.batch_lib()
    buf = torch.empty(index_size(n), dtype=torch.uint8, device=dev)
    parts = ctypes.c_uint64(0)
    _native.check(lib.k2h_amd_ralledata_index(_opt(blobs, n), blobs.numel(), _opt(blob_off, n), n, _opt(consider, n),
                                              _ptr(buf), buf.numel(), ctypes.byref(parts) if count else None,
                                              _stream_handle(stream)))
    return StreamIndex(buf, n, blobs.numel(), int(parts.value) if count else None)


def _check_keys(keys, key_off, dev, torch):
    _check_dev(keys, "keys", torch.uint8)
    _check_dev(key_off, "key_off", torch.int64)
    if keys.device != dev or key_off.device != dev:
        raise ValueError("keys and key_off must be on the stream's device")
    if key_off.numel() < 1:
        raise ValueError("key_off needs m + 1 entries")
    return key_off.numel() - 1


def find_keys(blobs, blob_off, index: StreamIndex, keys, key_off, h1=None, h2=None, std_fnv: bool = False,
              cstr: bool = False, now=None, want_match: bool = True, want_hit: bool = False, count: bool = True,
              stream=None) -> Found:
    """k2h_amd_ralledata_find: query i = keys[key_off[i]:key_off[i + 1]] looked up in the stream
    through `index`.  h1 / h2 (int64, m each): the queries' hashes, else they are computed
    (std_fnv picks the seed).  cstr: a query stands for its bytes plus a NUL.  now: (sec, nsec),
    switches the expiry check on.  count=False: counts is None and nothing waits for the device."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    dev = blobs.device
    m = _check_keys(keys, key_off, dev, torch)
    if index.buffer.device != dev:
        raise ValueError("the index is on another device than the stream")
    if (h1 is None) != (h2 is None):
        raise ValueError("h1 and h2 go together")
    for name, h in (("h1", h1), ("h2", h2)):
        if h is not None:
            _check_dev(h, name, torch.int64)
            if h.numel() != m or h.device != dev:
                raise ValueError(f"{name} needs m entries on the stream's device")
    flags = (_native.K2H_AMD_FLAG_STD_FNV if std_fnv else 0) | (_native.K2H_AMD_FLAG_CSTR if cstr else 0)
    ts = _native.Timespec(*now) if now is not None else None
    match = torch.empty(m, dtype=torch.int64, device=dev) if want_match else None
    status = torch.empty(m, dtype=torch.uint8, device=dev)
    hit = torch.empty(n, dtype=torch.uint8, device=dev) if want_hit else None
    counts = (ctypes.c_uint64 * 3)()
    _native.check(_native.batch_lib().k2h_amd_ralledata_find(
        _opt(blobs, n), blobs.numel(), _opt(blob_off, n), n, _ptr(index.buffer), _opt(keys, keys.numel()), keys.numel(),
        _ptr(key_off), m, _opt(h1, m), _opt(h2, m), flags, ctypes.byref(ts) if ts is not None else None, _opt(match, m),
        _ptr(status), _opt(hit, n), ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64)) if count else None,
        _stream_handle(stream)))
    return Found(match, status, hit, FindCounts(*(int(x) for x in counts)) if count else None)


def fetch_segments(blobs, blob_off, which, segment: str = "value", take=None, want_bad: bool = False, stream=None):
    """k2h_amd_ralledata_fetch: the chosen segment ("key", "value", "subkeys" or "attrs") of blob
    which[i] for every slot i (int64, -1: nothing; take: uint8 or bool mask, m entries), packed in
    slot order.  A count call and a fill.  Returns (out, out_off, bad): slot i's bytes are
    out[out_off[i]:out_off[i + 1]]; bad (uint8, m) is None without want_bad."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    dev = blobs.device
    if segment not in SEGMENTS:
        raise ValueError(f"segment must be one of {sorted(SEGMENTS)}")
    _check_dev(which, "which", torch.int64)
    if which.device != dev:
        raise ValueError("which is on another device than the stream")
    m = which.numel()
    if take is not None:
        if take.dtype == torch.bool:
            take = take.view(torch.uint8)
        _check_dev(take, "take", torch.uint8)
        if take.numel() != m or take.device != dev:
            raise ValueError("take needs m entries on the stream's device")
    bad = torch.empty(m, dtype=torch.uint8, device=dev) if want_bad else None
    out_off = torch.empty(m + 1, dtype=torch.int64, device=dev)
    total = ctypes.c_uint64(0)
    lib = _native.batch_lib()

    def call(o, cap):
        return lib.k2h_amd_ralledata_fetch(_opt(blobs, n), blobs.numel(), _opt(blob_off, n), n, _opt(which, m), m,
                                           _opt(take, m), SEGMENTS[segment], o, cap, _ptr(out_off), _opt(bad, m),
                                           ctypes.byref(total), _stream_handle(stream))
    _native.check(call(None, 0))
    out = torch.empty(max(int(total.value), 1), dtype=torch.uint8, device=dev)
    _native.check(call(_ptr(out), out.numel()))
    return out[:int(total.value)], out_off, bad


def get_values(blobs, blob_off, index: StreamIndex, keys, key_off, now=None, stream=None, **kw):
    """Get for a batch: find_keys (kw: h1, h2, std_fnv, cstr), then the values of the queries
    with FIND_FOUND and without FIND_EXPIRED.  Returns (values, value_off, status): query i's value
    is values[value_off[i]:value_off[i + 1]], empty for a key that is absent or has expired."""
    torch = _torch()
    f = find_keys(blobs, blob_off, index, keys, key_off, now=now, count=False, stream=stream, **kw)
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        take = ((f.status & (FIND_FOUND | FIND_EXPIRED | FIND_BAD_INDEX)) == FIND_FOUND).to(torch.uint8)
    out, out_off, _bad = fetch_segments(blobs, blob_off, f.match, "value", take=take, stream=stream)
    return out, out_off, f.status
