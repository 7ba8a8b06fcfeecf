"""Helper for tests/test_ralledata_partition*.py (not a test module, not a conftest).

* A pure-Python model of k2h_amd_ralledata_partition (include/k2hash_amd.h section 4b''): one
  sequential pass that gives every blob its part, then the parts laid down one after the other.
* The partition kernels' tile, read from the source.  The kernels have one form each (no
  staged / direct split), so there is no per-tile arithmetic to restate beyond the tile itself
  and the length from which the whole block moves a blob.
* A device-side runner that only launches the entry point, into sentinel-filled outputs.
"""
import ctypes
import re
import struct
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
_SRC = (ROOT / "k2hash_amd" / "csrc" / "k2h_ralledata_part.hip").read_text()


def _const(name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", _SRC)
    assert m, name
    return int(m.group(1))


TILE = _const("kPartBlobs")   # blobs per block
LONG = _const("kPartLong")    # a blob of at least this many bytes is moved by the whole block

HEADER = 80
PART_MAX = 256
NONE = 0xFFFFFFFF
IDS, OWNER, MASK = 0, 1, 2


class Rule:
    """k2h_amd_part_rule as plain integers."""

    def __init__(self, kind, parts, max_hash=0, span=0, mask=0):
        self.kind, self.parts, self.max_hash, self.span, self.mask = kind, parts, max_hash, span, mask

    def ctypes(self):
        from k2hash_amd._native import PartRule
        return PartRule(self.kind, self.parts, self.max_hash, self.span, self.mask)

    def kwargs(self, ids=None):
        """The rule as partition_ralledata's keyword arguments."""
        if self.kind == IDS:
            return dict(ids=ids)
        return dict(owner=(self.max_hash, self.span)) if self.kind == OWNER else dict(mask=self.mask)


def ids_rule(parts):
    return Rule(IDS, parts)


def owner_rule(max_hash, span):
    return Rule(OWNER, -(-max_hash // span), max_hash, span)


def mask_rule(mask, parts):
    return Rule(MASK, parts, mask=mask)


def hash_part(h, rule):
    """The part of a stored hash under a hash rule."""
    if rule.kind == OWNER:
        return (h % rule.max_hash) // rule.span
    return (h & rule.mask) % rule.parts


def parts_of(buf, off, size, rule, ids=None, consider=None):
    """part_out of the call: each blob's part, or NONE."""
    raw = bytes(buf)
    off = [int(x) for x in off]
    out = np.full(len(off) - 1, NONE, np.uint32)
    for i in range(len(off) - 1):
        b, e = off[i], off[i + 1]
        if consider is not None and not consider[i]:
            continue
        if not b <= e <= size:
            continue
        if rule.kind == IDS:
            if 0 <= int(ids[i]) < rule.parts:
                out[i] = int(ids[i])
        elif e - b >= HEADER:
            out[i] = hash_part(struct.unpack_from("<Q", raw, b)[0], rule)
    return out


def partition_model(buf, off, size, rule, ids=None, consider=None):
    """(bytes, out_off, index, part_out, part_first, part_byte) of k2h_amd_ralledata_partition."""
    buf = np.ascontiguousarray(np.frombuffer(bytes(buf), np.uint8))
    off = [int(x) for x in off]
    part = parts_of(buf, off, size, rule, ids, consider)
    pieces, ooff, index, first, byte = [], [0], [], [], []
    for p in range(rule.parts):
        first.append(len(index))
        byte.append(ooff[-1])
        for i in np.flatnonzero(part == p):
            pieces.append(buf[off[i]:off[i + 1]])
            ooff.append(ooff[-1] + off[i + 1] - off[i])
            index.append(int(i))
    first.append(len(index))
    byte.append(ooff[-1])
    data = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    return data, np.array(ooff, np.uint64), np.array(index, np.uint64), part, first, byte


# ================================================================================ device side
def run_partition(cuda, blobs, size, off, rule, ids=None, consider=None, out=None, out_cap=None, want_index=True,
                  want_parts=True, expect=0):
    """k2h_amd_ralledata_partition over a device stream into `out` (a byte tensor, usually a
    guarded view; None: counts only) and sentinel-filled out_off / index / part_out.  Returns a
    dict: rc, first, byte (lists), and out_off, index, part_out as host arrays -- out_off and
    index cut at kept, their entries behind it checked to hold the sentinel."""
    import torch

    import big_offsets as bo
    from k2hash_amd import _native
    n = len(off) - 1
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.int64)).to(cuda)
    d_ids = None if ids is None else torch.from_numpy(np.ascontiguousarray(ids, np.uint32).view(np.int32)).to(cuda)
    d_con = None if consider is None else torch.from_numpy(np.ascontiguousarray(consider, np.uint8)).to(cuda)
    fo, ooff = bo.sentinel_words(torch, cuda, n + 1)
    fi, index = bo.sentinel_words(torch, cuda, n)
    pw, pout = bo.guarded(torch, cuda, 4 * n, fill=0xEE)
    first = (ctypes.c_uint64 * (rule.parts + 1))(*([0xDEAD] * (rule.parts + 1)))
    byte = (ctypes.c_uint64 * (rule.parts + 1))(*([0xDEAD] * (rule.parts + 1)))
    r = rule.ctypes()
    opt = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() or 1)  # noqa: E731
    rc = _native.batch_lib().k2h_amd_ralledata_partition(
        ctypes.c_void_p(blobs.data_ptr() or 1), size, bo._p(d_off), n, ctypes.byref(r), opt(d_ids), opt(d_con),
        opt(out), (out.numel() if out is not None else 0) if out_cap is None else out_cap,
        bo._p(ooff) if out is not None else None, bo._p(index) if out is not None and want_index else None,
        opt(pout) if want_parts else None, first, byte, bo._stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, _native.batch_lib().k2h_amd_strerror(rc))
    assert bo.guards_intact(torch, pw, pout, 0xEE), "bytes outside part_out written"
    first, byte = list(first), list(byte)
    k = first[rule.parts] if out is not None and rc == 0 else -1
    a = fo.cpu().numpy().view(np.uint64)
    assert (a[k + 1:] == np.uint64(bo.SENTINEL)).all(), "out_off written past entry kept"
    b = fi.cpu().numpy().view(np.uint64)
    assert (b[max(k, 0) if want_index else 0:] ==np.uint64(bo.SENTINEL)).all(), "index written past entry kept - 1"
    part = pout.cpu().numpy().view(np.uint32) if want_parts else None
    if not want_parts:
        assert bool((pout == 0xEE).all())
    return dict(rc=rc, first=first, byte=byte, out_off=a[:k + 1], index=b[:max(k, 0)] if want_index else None,
                part_out=part)
