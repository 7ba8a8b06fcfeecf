"""Helper for tests/test_archive_barrier*.py (not a test module, not a conftest): the model of
k2h_amd_archive_barrier (include/k2hash_amd.h section 5d).

* execute: the two barrier arms of K2HArchive::Load (lib/k2harchive.cc:343-362) over the dict
  table of archive_fold_model.replay, line by line: K2HShm::Rename (lib/k2hshm.cc:3364-3502) and
  K2HDAccess::Open / SetWriteOffset / Write (lib/k2hdaccess.cc:168-455).  Bytes the reference
  leaves uninitialised are zero here and flagged GAP; a RENAME onto a live key, which the
  reference turns into two elements under one key, is refused as NEW_EXISTS.
* barrier_model: the call itself -- the arena's bytes, held_off, held_keep and the eight result
  words, the absorbed run of OW_VAL records included.  It works on the file's bytes and the host
  records, because a range outside the file is a BAD_RECORD and not an empty segment.
* replay_all: a whole log replayed in order, archive_fold_model.replay's arms between the barriers.
* run_barrier: the C call over a sentinel-filled, guarded arena.

Nothing here calls the code under test except run_barrier at the end, which only launches it.
"""
import ctypes
import struct
from typing import NamedTuple

import numpy as np

import archive_fold_model as fm
import ralle_check_model as rm
from archive_fold_model import OW_VAL, RENAME
from ralle_unlink_model import layout

EXECUTED, NOT_FOUND, NEW_EXISTS, BAD_RECORD, NOT_A_BARRIER = range(5)
CREATED, GAP = 1, 2
COUNT_ONLY = 0x100
MAX_RUN = 256
NONE = (1 << 64) - 1
SKIPPED = (NOT_FOUND, BAD_RECORD)     # the outcomes Load passes over under isErrSkip


def offset_of(exdata):
    """OWVAL_EXDATA (lib/k2hcommand.h:90-93): the bytes copied over a zeroed off_t; None where the
    record is bad -- no exdata (lib/k2harchive.cc:344), more than the union holds, or negative
    (SetWriteOffset, lib/k2hdaccess.cc:266)."""
    if not 1 <= len(exdata) <= 8:
        return None
    off = struct.unpack("<q", exdata.ljust(8, b"\0"))[0]
    return None if off < 0 else off


def overwrite(old, off, data):
    """(value, gap) of Write at `off` (lib/k2hdaccess.cc:392-455): a value shorter than the
    offset is stretched to it, the stretch zero here; the data is laid over it."""
    gap = off > len(old)
    v = bytearray(old.ljust(off, b"\0"))
    v[off:off + len(data)] = data
    return bytes(v), gap


def execute(table, r, rename_attrs=lambda rec, old: rec or old):
    """One OW_VAL or RENAME Rec executed on the dict table {key: (V, S, A)} (a field None when
    empty), in place.  Returns (outcome, flags); anything but EXECUTED leaves the table alone.
    rename_attrs: the rule under test -- the record's attrs when it has any, else the old
    element's (lib/k2hshm.cc:3427-3436)."""
    if r.status != 0 or r.type not in (OW_VAL, RENAME) or not r.key:
        return NOT_A_BARRIER, 0
    if r.type == RENAME:
        if not r.exdata:                                         # :3366
            return BAD_RECORD, 0
        if r.key not in table:                                   # :3389-3392
            return NOT_FOUND, 0
        if r.exdata != r.key and r.exdata in table:              # InsertElement would leave two elements under one key
            return NEW_EXISTS, 0
        v, s, a = table.pop(r.key)                               # TakeOffElement, FreeElement
        table[r.exdata] = (v, s, rename_attrs(r.attrs or None, a))
        return EXECUTED, 0
    off = offset_of(r.exdata)
    if off is None or not r.val:                                 # lib/k2harchive.cc:344, lib/k2hdaccess.cc:266, :394
        return BAD_RECORD, 0
    flags = 0
    if r.key not in table:                                       # Open: Set(key, NULL, 0), lib/k2hdaccess.cc:168-214
        table[r.key] = (None, None, None)
        flags |= CREATED
    v, s, a = table[r.key]
    new, gap = overwrite(v or b"", off, r.val)
    table[r.key] = (new, s, a)
    return EXECUTED, flags | (GAP if gap else 0)


def replay_all(recs, prior, err_skip=False):
    """(table, stopped_at, outcome): the log replayed record by record.  A barrier that is not
    executed ends the replay, unless err_skip passes over it as Load does under isErrSkip;
    NEW_EXISTS always ends it.  stopped_at: the index of that record, len(recs) at the end."""
    t = dict(prior)
    for i, r in enumerate(recs):
        if r.status == 0 and r.type in (OW_VAL, RENAME) and r.key:
            outcome, _flags = execute(t, r)
            if outcome == EXECUTED or (err_skip and outcome in SKIPPED):
                continue
            return t, i, outcome
        if r.status == 0 and r.type in (OW_VAL, RENAME):        # no key: Load skips it like every record without one
            continue
        t = fm.replay([r], t)
    return t, len(recs), EXECUTED


# ------------------------------------------------------------------------------- the call
class Model(NamedTuple):
    arena: bytes          # held[:held_size] and the appended blob
    held_off: np.ndarray  # uint64, na + 2 (na + 1 when nothing is appended)
    held_keep: np.ndarray  # uint8, na + 1 (na when nothing is appended)
    result: list          # 8


def _seg(file, r, name):
    """The bytes of a record's range, None when it is not inside the file."""
    off, ln = int(r[name + "_off"]), int(r[name + "_len"])
    return bytes(file[off:off + ln]) if off <= len(file) and ln <= len(file) - off else None


def _ow(file, r):
    """(offset, data) of an OW_VAL record, None for a BAD_RECORD."""
    x, v = _seg(file, r, "exdata"), _seg(file, r, "val")
    if x is None or not v:
        return None
    off = offset_of(x)
    return None if off is None else (off, v)


def barrier_model(held, off, keep, file, recs, b, consider, hashes, size=None):
    """held: the arena's used bytes, off its na + 1 offsets, keep its na keep bytes; file / recs:
    the log's bytes and host records (archive.REC_DTYPE); hashes: (h1, h2, new_h1, new_h2) of the
    records."""
    raw, file = bytes(held), bytes(file)
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    na = len(off) - 1
    keep = np.ones(na, np.uint8) if keep is None else np.array(keep, np.uint8)

    def nothing(outcome):
        return Model(raw, np.array(off, np.uint64), keep.copy(), [outcome, 0, 0, 0, 0, NONE, 0, 0])
    considered = lambda i: consider is None or bool(consider[i])  # noqa: E731
    r = recs[b]
    key = _seg(file, r, "key")
    if int(r["status"]) != 0 or not considered(b) or int(r["type"]) not in (OW_VAL, RENAME) or not key:
        return nothing(NOT_A_BARRIER)
    typ = int(r["type"])

    # the held side: the participants of an identity, in stream order
    def copies(h1, h2, k):
        out = []
        for j in range(na):
            st, f = rm.header_status(raw, off[j], off[j + 1], size)
            if keep[j] and st == rm.OK and (f[0], f[1]) == (h1, h2) and raw[off[j] + f[6]:off[j] + f[6] + f[2]] == k:
                out.append(j)
        return out

    def fields(j):
        f = struct.unpack_from("<10Q", raw, off[j])
        return tuple(raw[off[j] + f[6 + s]:off[j] + f[6 + s] + f[2 + s]] if f[2 + s] else b"" for s in (1, 2, 3))
    h1, h2, nh1, nh2 = (int(h[b]) for h in hashes)
    flags = 0
    if typ == RENAME:
        new = _seg(file, r, "exdata")
        if not new:
            return nothing(BAD_RECORD)
        old = copies(h1, h2, key)
        if not old:
            return nothing(NOT_FOUND)
        if new != key and copies(nh1, nh2, new):
            return nothing(NEW_EXISTS)
        v, s, a = fields(old[-1])
        blob = layout((nh1, nh2), new, v, s, _seg(file, r, "attrs") or a)
        executed = 1
    else:
        if _ow(file, r) is None:
            return nothing(BAD_RECORD)
        executed = 0
        while executed < MAX_RUN and b + executed < len(recs):
            c = recs[b + executed]
            if int(c["status"]) != 0 or not considered(b + executed) or int(c["type"]) != OW_VAL or \
                    _seg(file, c, "key") != key or _ow(file, c) is None:
                break
            executed += 1
        old = copies(h1, h2, key)
        v, s, a = fields(old[-1]) if old else (b"", b"", b"")
        flags = 0 if old else CREATED
        # GAP is the call's, not a record's: a byte of the FINAL value that neither the old value
        # nor any write of the run covers.  A stretch that a later write of the run fills is no gap.
        covered = [(0, len(v))]
        for i in range(b, b + executed):
            at, data = _ow(file, recs[i])
            v, _stretched = overwrite(v, at, data)
            covered.append((at, at + len(data)))
        reach = 0
        for lo, hi in sorted(covered):
            if lo > reach:
                flags |= GAP
            reach = max(reach, hi)
        blob = layout((h1, h2), key, v, s, a)
    keep = np.append(keep, np.uint8(1))
    keep[old] = 0
    vlen = struct.unpack_from("<Q", blob, rm.F_VLEN)[0]
    return Model(raw[:size] + blob, np.array(off + [size + len(blob)], np.uint64), keep,
                 [EXECUTED, executed, len(blob), flags, len(old), old[-1] if old else NONE, vlen, 0])


# ------------------------------------------------------------------------------ device side
ARENA_FILL = 0xC3


def run_barrier(cuda, held, off, keep, file, recs, b, consider=None, hashes=None, flags=0, slack=None, hshift=5,
                fshift=11, tail=64, held_size=None):
    """k2h_amd_archive_barrier over an arena of len(held) + slack bytes (slack None: 1 MiB) that lies `hshift` bytes off alignment between
    canaries, with `tail` canary bytes behind it; held_off and held_keep are sentinel-filled behind
    their na + 1 / na entries.  Returns (rc, arena bytes, held_off, held_keep, result): the arena
    whole (len(held) + slack bytes), held_off with na + 2 and held_keep with na + 1 entries."""
    import torch

    import big_offsets as bo
    from k2hash_amd import _native, archive
    na, n = len(off) - 1, len(recs)
    used = len(held) if held_size is None else held_size
    slack = (1 << 20) if slack is None else slack
    cap = len(held) + slack
    whole = torch.full((bo.GUARD + hshift + cap + tail,), 0xA5, dtype=torch.uint8, device=cuda)
    arena = whole[bo.GUARD + hshift:bo.GUARD + hshift + cap]
    arena[:] = ARENA_FILL
    if len(held):
        arena[:len(held)] = torch.from_numpy(np.frombuffer(bytes(held), np.uint8).copy()).to(cuda)
    fw, d_file = bo.guarded(torch, cuda, max(len(file), 1), shift=fshift, fill=0xA5)
    if len(file):
        d_file[:len(file)] = torch.from_numpy(np.frombuffer(bytes(file), np.uint8).copy()).to(cuda)
    fo, d_off = bo.sentinel_words(torch, cuda, na + 2)
    d_off[:na + 1] = torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)
    kw, d_keep = bo.guarded(torch, cuda, na + 1, fill=0xEE)
    d_keep[:na] = torch.from_numpy(np.ones(na, np.uint8) if keep is None else np.ascontiguousarray(keep, np.uint8).copy()).to(cuda)
    words = np.ascontiguousarray(recs).view(np.int64).reshape(-1, archive.REC_WORDS)
    d_recs = torch.from_numpy(words.copy()).to(cuda)
    d_cons = None if consider is None else torch.from_numpy(np.ascontiguousarray(consider, np.uint8).copy()).to(cuda)
    d_h = [None] * 4 if hashes is None else [
        torch.from_numpy(np.ascontiguousarray(h, np.uint64).view(np.int64).copy()).to(cuda) for h in hashes]
    result = (ctypes.c_uint64 * 8)(*[0xDEAD] * 8)
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = _native.batch_lib().k2h_amd_archive_barrier(
        p(arena), used, cap, p(d_off), na, p(d_keep), p(d_file), len(file), p(d_recs), n, b, p(d_cons), *[p(h) for h in d_h],
        flags, ctypes.cast(result, ctypes.POINTER(ctypes.c_uint64)), bo._stream())
    torch.cuda.synchronize()
    assert bo.guards_intact(torch, whole, arena, 0xA5), "bytes outside the arena written"
    assert bo.guards_intact(torch, fw, d_file, 0xA5), "the file's guards changed"
    assert bo.guards_intact(torch, kw, d_keep, 0xEE), "bytes outside held_keep written"
    assert (fo.cpu().numpy().view(np.uint64)[na + 2:] == np.uint64(bo.SENTINEL)).all(), "held_off written past entry na + 1"
    return (rc, arena.cpu().numpy().tobytes(), d_off.cpu().numpy().view(np.uint64), d_keep.cpu().numpy(),
            [int(x) for x in result])


def assert_barrier(got, m, what, held_len, written=True, keep_before=None):
    """The call's answer against the model: result, and -- for an executed call that wrote --
    the appended bytes, held_off[na + 1] and the keep bytes; otherwise an untouched arena."""
    import big_offsets as bo
    rc, arena, hoff, hkeep, result = got
    assert rc == 0, (what, rc)
    assert result == m.result, f"{what}: result {result}, want {m.result}"
    na = len(m.held_off) - (2 if m.result[0] == EXECUTED else 1)
    size = int(m.held_off[na])
    assert arena[:held_len] == m.arena[:held_len], f"{what}: the held bytes changed"
    assert (hoff[:na + 1] == m.held_off[:na + 1]).all(), f"{what}: held_off[:na + 1] changed"
    if m.result[0] == EXECUTED and written:
        end = int(m.held_off[na + 1])
        if arena[size:end] != m.arena[size:end]:
            a, w = np.frombuffer(arena[size:end], np.uint8), np.frombuffer(m.arena[size:end], np.uint8)
            at = int(np.nonzero(a != w)[0][0])
            raise AssertionError(f"{what}: the appended blob differs at byte {at} of {end - size}: got {a[at]}, want {w[at]}")
        assert (np.frombuffer(arena[end:], np.uint8) == ARENA_FILL).all(), f"{what}: bytes behind the appended blob written"
        assert int(hoff[na + 1]) == end, f"{what}: held_off[na + 1] {int(hoff[na + 1])}, want {end}"
        assert hkeep.tolist() == m.held_keep.tolist(), f"{what}: held_keep {hkeep.tolist()}, want {m.held_keep.tolist()}"
    else:
        assert (np.frombuffer(arena[max(size, held_len):], np.uint8) == ARENA_FILL).all(), f"{what}: the arena was written"
        assert int(hoff[na + 1]) == bo.SENTINEL, f"{what}: held_off[na + 1] written"
        keep0 = m.held_keep[:na] if m.result[0] != EXECUTED else keep_before
        assert hkeep[na] == 0xEE, f"{what}: held_keep[na] written"
        if keep0 is not None:
            assert hkeep[:na].tolist() == [int(x) for x in keep0], f"{what}: held_keep changed"
