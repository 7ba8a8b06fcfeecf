"""Subkey names unlinked from a RALLEDATA blob stream on the device (include/k2hash_amd.h section
4b'''''''): the first half of K2HShm::Remove(key, subkey) -- the name erased from the parent's
list, the list serialized again -- applied to the blobs of a stream before they are fed, fused
with select_ralledata's keep mask.  The first calls of the package that rewrite blobs; they build
on subkeys.py, which also exports them.

The ``stream`` argument is that of batch.py's module docstring: None means the current torch
stream; otherwise every device operation of the call, the wrapper's own torch ops included, is
ordered on ``stream``.  ``drop_mask`` only enqueues work; ``unlink_subkeys`` synchronises the
stream to read its counts back, ``prune_ralledata`` is that and ``subkey_edges`` and
``reach_subkeys``.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

from . import _native
from .batch import _check_dev, _dev_ptr, _stream_handle, _torch
from .ralledata import _check_stream, _consider_arg
from .subkeys import SubkeyEdges, _ptr, reach_subkeys, subkey_edges

UNLINK_REWRITTEN, UNLINK_EMPTIED, UNLINK_KEY_ONLY = (_native.K2H_AMD_UNLINK_REWRITTEN, _native.K2H_AMD_UNLINK_EMPTIED,
                                                     _native.K2H_AMD_UNLINK_KEY_ONLY)


class UnlinkCounts(NamedTuple):
    emitted: int        # blobs emitted
    emitted_bytes: int  # their bytes in the output
    rewritten: int      # blobs whose list was re-serialized
    dropped: int        # entries left out of those lists by their drop byte
    emptied: int        # lists left without a name: skey_length is now 0
    key_only: int       # ... of them, blobs left with a key and nothing else (they leave no element when fed)
    mismatches: int     # blobs with a drop byte set whose header or walk disagrees with sk_flags / edge_off: copied


class Unlinked(NamedTuple):
    blobs: object     # uint8 tensor: the emitted blobs back to back (None when only counting)
    blob_off: object  # int64 tensor, emitted + 1, relative to `blobs`, from 0 (None when only counting)
    index: object     # int64 tensor, emitted: the blobs' indices in the input stream (None when only counting)
    changed: object   # uint8 tensor, n: UNLINK_REWRITTEN | UNLINK_EMPTIED | UNLINK_KEY_ONLY per INPUT blob
    counts: UnlinkCounts


def drop_mask(edges: SubkeyEdges, gone=None, dangling: bool = False, stream=None):
    """A uint8 tensor of E for unlink_subkeys (k2h_amd_subkeys_drop_mask): 1 for every edge whose
    child is a blob with gone[child] != 0 (gone: a uint8 or bool mask of n, such as
    reach_subkeys(...).mask; None: no such edge) and, with dangling=True, for every edge whose
    name addresses no participant.  Asynchronous on the stream."""
    torch = _torch()
    if edges.child is None:
        raise ValueError("drop_mask needs the child of subkey_edges (count_only=False)")
    n = edges.edge_off.numel() - 1
    dev = edges.edge_off.device
    if gone is not None:
        if gone.dtype == torch.bool:
            gone = gone.view(torch.uint8)
        _check_dev(gone, "gone", torch.uint8)
        if gone.numel() != n or gone.device != dev:
            raise ValueError("gone needs n entries on the blobs' device")
    E = edges.child.numel()
    drop = torch.empty(E, dtype=torch.uint8, device=dev)
    rc = _native.batch_lib().k2h_amd_subkeys_drop_mask(
        _ptr(edges.child), E, _ptr(gone) if gone is not None and n else None, n, 1 if dangling else 0, _ptr(drop),
        _stream_handle(stream))
    _native.check(rc)
    return drop


def unlink_subkeys(blobs, blob_off, edges: SubkeyEdges, drop, keep=None, out=None, count_only: bool = False,
                   stream=None) -> Unlinked:
    """The stream packed as select_ralledata packs it (keep None: every blob), with the names of
    the dropped edges taken out of the lists that carry them (k2h_amd_ralledata_unlink).  edges:
    subkey_edges over the same stream (its flags and edge_off are used); drop: a uint8 or bool
    tensor of E, non-zero leaves edge e's entry out, or None (nothing is dropped: the result is
    select_ralledata's).  A blob with a dropped edge has its list serialized again as
    K2HSubKeys::Serialize writes it and is laid out as GetElementToBinary lays a blob out; every
    other emitted blob is copied byte for byte.  changed and counts say what was done; a blob
    marked UNLINK_KEY_ONLY leaves no element when fed.  Without `out` the bytes are counted first
    and an exact buffer is allocated (two calls, each synchronising the stream once); an `out`
    too small raises with nothing written.  count_only: blobs, blob_off and index are None."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    dev = blobs.device
    if edges.flags.numel() != n or edges.edge_off.numel() != n + 1 or edges.flags.device != dev:
        raise ValueError("edges are not subkey_edges of this stream (n differs, or another device)")
    keep = _consider_arg(keep, n, dev, torch)  # (the same checks; its messages say consider)
    if drop is not None:
        if drop.dtype == torch.bool:
            drop = drop.view(torch.uint8)
        _check_dev(drop, "drop", torch.uint8)
        if drop.numel() != edges.counts.edges or drop.device != dev:
            raise ValueError("drop needs E entries on the blobs' device")
    changed = torch.empty(n, dtype=torch.uint8, device=dev)
    counts = (ctypes.c_uint64 * 7)()
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    lib = _native.batch_lib()

    def call(o, cap, ooff, idx):
        return lib.k2h_amd_ralledata_unlink(
            _ptr(blobs), blobs.numel(), _dev_ptr(blob_off), n, _ptr(keep) if keep is not None and n else None,
            _ptr(edges.flags), _ptr(edges.edge_off), _ptr(drop) if drop is not None else None, o, cap, ooff, idx,
            _ptr(changed), cp, _stream_handle(stream))
    if count_only or out is None:
        _native.check(call(None, 0, None, None))
        if count_only:
            return Unlinked(None, None, None, changed, UnlinkCounts(*(int(c) for c in counts)))
        out = torch.empty(max(int(counts[1]), 1), dtype=torch.uint8, device=dev)
    else:
        _check_dev(out, "out", torch.uint8)
        if out.device != dev:
            raise ValueError("out is on another device than the blobs")
    out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev)
    _native.check(call(_ptr(out), out.numel(), _ptr(out_off), _ptr(index)))
    c = UnlinkCounts(*(int(x) for x in counts))
    return Unlinked(out[:c.emitted_bytes], out_off[:c.emitted + 1], index[:c.emitted], changed, c)


def prune_ralledata(blobs, blob_off, roots=None, *, dangling: bool = False, consider=None, std_fnv: bool = False,
                    out=None, stream=None) -> Unlinked:
    """The stream without the subtrees of the root blobs and without the names that would then
    address nothing: subkey_edges; reach_subkeys (when roots are given); keep = consider & ~reach;
    drop = drop_mask(edges, gone=reach, dangling=dangling); unlink_subkeys.  With dangling=True
    the names that addressed no participant to begin with go too; roots None removes no blob.

    This is a cleanup policy on top of the reference's rule, not a restatement of it.  The
    reference itself erases a name only from the one parent Remove(parent, name) is called on
    (K2HShm::Remove(key, subkey), lib/k2hshm.cc:2567-2667), and it leaves other dangling names
    alone: RemoveSubkeys skips names it does not find.  Here EVERY name of a removed key is
    unlinked, from every list that carries it.  To replay Remove(parent, name) exactly, set the
    drop bytes of those edges alone and call unlink_subkeys (INTEGRATION.md has the recipe)."""
    torch = _torch()
    n = _check_stream(blobs, blob_off, torch)
    consider = _consider_arg(consider, n, blobs.device, torch)
    edges = subkey_edges(blobs, blob_off, consider=consider, std_fnv=std_fnv, stream=stream)
    reach = reach_subkeys(edges, roots, stream=stream).mask if roots is not None else None
    keep = consider
    if reach is not None:
        keep = torch.empty(n, dtype=torch.uint8, device=blobs.device)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
            torch.eq(reach, 0, out=keep.view(torch.bool))
            if consider is not None:
                keep.mul_((consider != 0).to(torch.uint8))
    drop = drop_mask(edges, gone=reach, dangling=dangling, stream=stream)
    return unlink_subkeys(blobs, blob_off, edges, drop, keep=keep, out=out, stream=stream)
