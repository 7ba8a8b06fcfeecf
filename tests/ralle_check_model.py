"""Helper for tests/test_ralledata_check.py (not a test module, not a conftest).

* A pure-Python model of what k2h_amd_ralledata_check reports: the status precedence of
  include/k2hash_amd.h section 4b (the header tests in the order of
  K2HShm::SetElementByBinArray, lib/k2hshmdirect.cc:351, 355, 361-364) and the hash-range
  test of K2HShm::GetElementListToBinary, transliterated line by line from
  lib/k2hshmdirect.cc:118-131 and 165-176 with the 64-bit wrap masked explicitly.  The
  hashes come from the oracle.
* Stream builders: blobs from oracle.build_ralledata, header fields mutated with
  struct.pack_into, streams cut into blobs and joined again.
* The check kernel's two constants, read from its source, and the hull arithmetic that
  decides between its staged and direct forms.
"""
import re
import struct
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
_SRC = (ROOT / "k2hash_amd" / "csrc" / "k2h_ralledata_check.hip").read_text()


def _const(name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", _SRC)
    assert m, name
    return int(m.group(1))


TILE = _const("kCheckBlobs")   # blobs per block
STAGE = _const("kCheckStage")  # staged hull bytes
SEL_TILE = _const("kSelBlobs")        # select: blobs per block
SEL_TAB = _const("kSelTabPieces")     # select: 16-byte pieces of a tile's kept bytes its table covers

M64 = (1 << 64) - 1
HEADER = 80
OK, BAD_SPAN, EMPTY, NO_KEY, BAD_RANGE, BAD_HASH, BAD_SUBHASH = range(7)
# byte offsets of the header fields (lib/k2hshmdirect.h:36-47)
F_HASH, F_SUBHASH, F_KLEN, F_VLEN, F_SLEN, F_ALEN, F_KPOS, F_VPOS, F_SPOS, F_APOS = range(0, 80, 8)


# ------------------------------------------------------------------------- the range model
class Range:
    """k2h_amd_hash_range as plain integers."""

    def __init__(self, target_hash, target_max_hash, target_hash_range=1, old_hash=M64, old_max_hash=0):
        self.target_hash, self.target_max_hash, self.target_hash_range = target_hash, target_max_hash, target_hash_range
        self.old_hash, self.old_max_hash = old_hash, old_max_hash

    def ctypes(self):
        from k2hash_amd._native import HashRange
        return HashRange(self.target_hash, self.target_max_hash, self.target_hash_range, self.old_hash,
                         self.old_max_hash)


def is_target(h, r):
    """lib/k2hshmdirect.cc:118, 122-131."""
    end_target_hash = ((r.target_hash + ((r.target_hash_range - 1) if 0 < r.target_hash_range else 0)) & M64) \
        % r.target_max_hash
    is_target = True
    if r.target_hash <= end_target_hash:
        if (h % r.target_max_hash) < r.target_hash or end_target_hash < (h % r.target_max_hash):
            is_target = False
    else:
        if end_target_hash < (h % r.target_max_hash) and (h % r.target_max_hash) < r.target_hash:
            is_target = False
    return is_target


def in_old_range(h, r):
    """lib/k2hshmdirect.cc:119, 165-176: whether need_check_start stays true.  old_hash == ~0:
    the range does not exist (:119) and no modulo is taken."""
    if r.old_hash == M64:
        return False
    end_old_hash = ((r.old_hash + ((r.target_hash_range - 1) if 0 < r.target_hash_range else 0)) & M64) \
        % r.old_max_hash
    need_check_start = True
    if r.old_hash <= end_old_hash:
        if (h % r.old_max_hash) < r.old_hash or end_old_hash < (h % r.old_max_hash):
            need_check_start = False
    else:
        if end_old_hash < (h % r.old_max_hash) and (h % r.old_max_hash) < r.old_hash:
            need_check_start = False
    return need_check_start


def route_of(h, r):
    return (1 if is_target(h, r) else 0) | (2 if in_old_range(h, r) else 0)


# ------------------------------------------------------------------------ the status model
def header_status(buf, b, e, size):
    """Statuses 0-4 of blob [b, e) of buf, and its header fields (None for BAD_SPAN)."""
    if e < b or e > size or e - b < HEADER:
        return BAD_SPAN, None
    f = struct.unpack_from("<10Q", buf, b)
    L = e - b
    if f[2] == 0 and f[3] == 0 and f[4] == 0 and f[5] == 0:
        return EMPTY, f
    if f[2] == 0:
        return NO_KEY, f
    for s in range(4):
        ln, pos = f[2 + s], f[6 + s]
        if ln == 0:
            continue
        spos = pos - (1 << 64) if pos >> 63 else pos  # off_t
        if spos < HEADER or pos + ln > M64 or pos + ln > L:
            return BAD_RANGE, f
    return OK, f


def expected(oracle, buf, off, size=None, variant=0, rng=None):
    """(status, route, h1, h2) of the stream as numpy arrays; route is None without rng."""
    buf = np.ascontiguousarray(buf, np.uint8)
    raw = buf.tobytes()
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    n = len(off) - 1
    status = np.zeros(n, np.uint8)
    fields = [None] * n
    keys, which = [], []
    for i in range(n):
        st, f = header_status(raw, off[i], off[i + 1], size)
        status[i], fields[i] = st, f
        if st == OK:
            keys.append(raw[off[i] + f[6]:off[i] + f[6] + f[2]])
            which.append(i)
    h1 = np.zeros(n, np.uint64)
    h2 = np.zeros(n, np.uint64)
    if keys:
        koff = np.zeros(len(keys) + 1, np.uint64)
        koff[1:] = np.cumsum([len(k) for k in keys])
        r1, r2 = oracle.hash_csr(np.frombuffer(b"".join(keys), np.uint8), koff, variant)
        h1[which], h2[which] = r1, r2
    for i in which:
        if fields[i][0] != int(h1[i]):
            status[i] = BAD_HASH
        elif fields[i][1] != int(h2[i]):
            status[i] = BAD_SUBHASH
    route = None
    if rng is not None:
        route = np.zeros(n, np.uint8)
        for i in which:
            if status[i] == OK:
                route[i] = route_of(fields[i][0], rng)
    return status, route, h1, h2


def select_model(buf, off, keep, size=None):
    """(bytes, out_off, index) of k2h_amd_ralledata_select."""
    buf = np.ascontiguousarray(buf, np.uint8)
    size = buf.size if size is None else size
    off = [int(x) for x in off]
    parts, ooff, index = [], [0], []
    for i in range(len(off) - 1):
        b, e = off[i], off[i + 1]
        if keep[i] and b <= e <= size:
            parts.append(buf[b:e])
            ooff.append(ooff[-1] + e - b)
            index.append(i)
    data = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return data, np.array(ooff, np.uint64), np.array(index, np.uint64)


# ------------------------------------------------------------------------- stream builders
def records(oracle, n, klen=(1, 65), vlen=(0, 201), slen=None, alen=None, seed=0, p_empty=0.2):
    """n records: (keys, vals, skeys, attrs) as lists of bytes (None = segment absent); keys are
    never empty, the other segments are empty with probability p_empty."""
    rng = np.random.default_rng(seed)
    data = oracle.gen_bytes(1 << 20, byte_off=31 * seed + 5)

    def take(rr, p0):
        if rr is None:
            return None
        lens = rng.integers(rr[0], rr[1], n)
        if p0:
            lens[rng.random(n) < p0] = rr[0]
        starts = rng.integers(0, data.size - max(int(lens.max()), 1), n)
        return [data[int(s):int(s) + int(ln)].tobytes() for s, ln in zip(starts, lens)]
    return take(klen, 0), take(vlen, p_empty), take(slen, 0.5), take(alen, 0.5)


def stream_of(oracle, recs, variant=0):
    """(bytearray of the blobs, offsets as a list of ints) from the oracle's producer."""
    out, boff = oracle.build_ralledata(*recs, variant=variant)
    return bytearray(out.tobytes()), [int(x) for x in boff]


def split(buf, off):
    return [bytearray(buf[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def join(blobs, lead=b""):
    """Blobs laid end to end after `lead` bytes: (bytearray, offsets)."""
    off = [len(lead)]
    for b in blobs:
        off.append(off[-1] + len(b))
    return bytearray(lead) + bytearray(b"".join(bytes(b) for b in blobs)), off


def put(buf, at, field, value):
    struct.pack_into("<Q", buf, at + field, value & M64)


def get(buf, at, field):
    return struct.unpack_from("<Q", buf, at + field)[0]


def value_before_key(blob):
    """The same element with its value placed before its key (SetElementByBinArray honours any
    positions); the blob must have no subkeys and no attributes."""
    kl, vl = get(blob, 0, F_KLEN), get(blob, 0, F_VLEN)
    kp, vp = get(blob, 0, F_KPOS), get(blob, 0, F_VPOS)
    key, val = bytes(blob[kp:kp + kl]), bytes(blob[vp:vp + vl])
    out = bytearray(blob[:HEADER]) + val + key
    put(out, 0, F_VPOS, HEADER)
    put(out, 0, F_KPOS, HEADER + vl)
    return out


# --------------------------------------------------------------------------- kernel forms
def tile_forms(base_mod16, off, size):
    """Per tile of TILE blobs: 'staged' or 'direct', by the kernel's rule (every span good and
    the aligned hull of the tile's bytes within STAGE); base_mod16 = the stream's address & 15."""
    n = len(off) - 1
    forms = []
    for r0 in range(0, n, TILE):
        nr = min(TILE, n - r0)
        good = all(off[i] <= off[i + 1] <= size and off[i + 1] - off[i] >= HEADER for i in range(r0, r0 + nr))
        lo = (base_mod16 + off[r0]) & ~15
        hi = (base_mod16 + off[r0 + nr] + 15) & ~15
        forms.append("staged" if good and hi - lo <= STAGE else "direct")
    return forms
