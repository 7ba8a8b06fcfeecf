"""Subkeys followed through a RALLEDATA blob stream on the device (include/k2hash_amd.h section
4b''''''): the names in every blob's subkeys segment as edges to the blobs they address, what a
set of root blobs reaches over them, the stream with such a subtree kept or removed, and
(section 4b''''''') the stream with subkey names unlinked from the lists that carry them.

"The table the stream leaves" is taken as: the last participant of an identity wins.  That holds
for a feed without the mtime attribute or with non-decreasing times; with mtime-bearing blobs
pass the keep of ``dedup_ralledata(pts=...)`` as ``consider`` first.  Expiry is not applied, as
K2HShm::Remove does not apply it; compose ``blob_times`` for that.

The ``stream`` argument is that of batch.py's module docstring: None means the current torch
stream; otherwise every device operation of the call, the wrapper's own torch ops included, is
ordered on ``stream``.  No function here is asynchronous: ``subkey_edges`` reads the number of
edges back, ``reach_subkeys`` the size of every frontier.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

from . import _native
from .batch import FLAG_STD_FNV, _check_dev, _dev_ptr, _stream_handle, _torch
from .ralledata import Selected, _check_stream, _consider_arg, select_ralledata

SKEY_PART, SKEY_HAS, SKEY_BAD = _native.K2H_AMD_SKEY_PART, _native.K2H_AMD_SKEY_HAS, _native.K2H_AMD_SKEY_BAD
NO_BLOB = (1 << 64) - 1  # child[e] of a dangling name, rep[i] of a non-participant (-1 as int64)


class SubkeyCounts(NamedTuple):
    participants: int  # blobs that take part
    with_edges: int    # ... of them, those with at least one edge
    bad: int           # ... and those whose segment the strict walk rejected
    edges: int         # E
    dangling: int      # edges whose name addresses no participant (0 with count_only)


class SubkeyEdges(NamedTuple):
    flags: object     # uint8 tensor, n: SKEY_PART | SKEY_HAS | SKEY_BAD
    edge_off: object  # int64 tensor, n + 1: blob i's edges are [edge_off[i], edge_off[i + 1])
    child: object     # int64 tensor, E, or None (count_only): the addressed blob, -1 for a dangling name
    rep: object       # int64 tensor, n, or None: the last participant of blob i's identity, -1 for a non-participant
    counts: SubkeyCounts


class Reach(NamedTuple):
    mask: object      # uint8 tensor, n: 1 for every copy of a reached key
    reached: int      # their number
    levels: int       # levels run
    converged: bool   # the last level found nothing new


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() or 1)


def subkey_edges(blobs, blob_off, consider=None, std_fnv: bool = False, want_rep: bool = True,
                 count_only: bool = False, stream=None) -> SubkeyEdges:
    """The subkey names of a stream as edges between its blobs (k2h_amd_ralledata_subkeys).
    Every participant's subkeys segment is walked by the strict rule of the header; every name
    of non-zero length is an edge, and child[e] is the last participant whose stored hash,
    stored subhash and key equal the name's computed hashes and bytes -- what the table would
    find -- or -1 for a dangling name.  rep[i] (want_rep) is the last participant of blob i's own
    identity.  Two native calls, count then fill (count_only: the first alone, child and rep
    None); each synchronises the stream, the fill twice."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    dev = blobs.device
    consider = _consider_arg(consider, n, dev, torch)
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    edge_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    counts = (ctypes.c_uint64 * 5)()
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    lib = _native.batch_lib()

    def call(rep, child, cap):
        return lib.k2h_amd_ralledata_subkeys(
            _ptr(blobs), blobs.numel(), _dev_ptr(blob_off), n, _ptr(consider) if consider is not None and n else None,
            FLAG_STD_FNV if std_fnv else 0, _ptr(flags), _ptr(edge_off), rep, child, cap, cp, _stream_handle(stream))
    _native.check(call(None, None, 0))
    if count_only:
        return SubkeyEdges(flags, edge_off, None, None, SubkeyCounts(*(int(c) for c in counts)))
    edges = int(counts[3])
    child = torch.empty(edges, dtype=torch.int64, device=dev)
    rep = torch.empty(n, dtype=torch.int64, device=dev) if want_rep else None
    if n:
        _native.check(call(_ptr(rep) if want_rep else None, _ptr(child), edges))
    return SubkeyEdges(flags, edge_off, child, rep, SubkeyCounts(*(int(c) for c in counts)))


def _roots_mask(roots, n, dev, stream, torch):
    if roots.dtype == torch.bool:
        roots = roots.view(torch.uint8)
    if roots.dtype == torch.int64:
        if not roots.is_cuda or roots.device != dev:
            raise ValueError("roots must be on the blobs' device")
        mask = torch.empty(n, dtype=torch.uint8, device=dev)  # as every output: from the current stream's pool
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            mask.zero_()
            mask.index_fill_(0, roots.reshape(-1), 1)
        return mask
    _check_dev(roots, "roots", torch.uint8)
    if roots.numel() != n or roots.device != dev:
        raise ValueError("roots needs n entries on the blobs' device")
    return roots


def reach_subkeys(edges: SubkeyEdges, roots, max_levels: int = 0, stream=None) -> Reach:
    """What the root blobs reach over the edges (k2h_amd_ralledata_reach): the blobs
    K2HShm::Remove(key, true) of every root would remove from the table the stream leaves.
    roots: a uint8 or bool mask of n, or an int64 tensor of blob indices.  A root that is an
    earlier copy of a key stands for the key; every copy of a reached key is marked.  max_levels:
    0 for no limit, else the traversal stops after that many levels and converged says whether
    it was done.  Synchronises the stream once per level and twice more."""
    torch = _torch()
    if edges.child is None or edges.rep is None:
        raise ValueError("reach_subkeys needs the child and rep of subkey_edges (want_rep=True, count_only=False)")
    n = edges.edge_off.numel() - 1
    dev = edges.edge_off.device
    roots = _roots_mask(roots, n, dev, stream, torch)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = (ctypes.c_uint64 * 3)()
    rc = _native.batch_lib().k2h_amd_ralledata_reach(
        _ptr(edges.edge_off), _ptr(edges.child), _ptr(edges.rep), n, _ptr(roots), int(max_levels), _ptr(mask),
        ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64)), _stream_handle(stream))
    _native.check(rc)
    return Reach(mask, int(counts[0]), int(counts[1]), bool(counts[2]))


def subtree_ralledata(blobs, blob_off, roots, *, remove: bool = False, consider=None, std_fnv: bool = False,
                      out=None, stream=None) -> Selected:
    """The subtrees of the root blobs as a stream of their own, or (remove=True) the stream
    without them: subkey_edges, reach_subkeys and select_ralledata with keep = reach, or
    consider & ~reach (consider None: every blob).  With ralledata_to_archive the result is
    "this subtree as an archive"."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    consider = _consider_arg(consider, n, blobs.device, torch)
    edges = subkey_edges(blobs, blob_off, consider=consider, std_fnv=std_fnv, stream=stream)
    reach = reach_subkeys(edges, roots, stream=stream).mask
    keep = reach
    if remove:
        keep = torch.empty(n, dtype=torch.uint8, device=blobs.device)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            torch.eq(reach, 0, out=keep.view(torch.bool))
            if consider is not None:
                keep.mul_((consider != 0).to(torch.uint8))
    return select_ralledata(blobs, blob_off, keep, out=out, stream=stream)


# Section 4b''''''': names unlinked from the lists that carry them.  The wrappers live in unlink.py
# (they build on the ones above) and are part of this module's interface.
from .unlink import (UNLINK_EMPTIED, UNLINK_KEY_ONLY, UNLINK_REWRITTEN, UnlinkCounts, Unlinked,  # noqa: E402,F401
                     drop_mask, prune_ralledata, unlink_subkeys)
