"""Helper for tests/test_ralledata_dedup.py (not a test module, not a conftest).

* dedup_model: what k2h_amd_ralledata_dedup reports (include/k2hash_amd.h section 4b'), as one
  sequential pass over the stream with a dict from identity -- stored hash, stored subhash,
  key bytes (and with them the key length) -- to the last participant seen.
* set_element_by_bin_array: K2HShm::SetElementByBinArray, lib/k2hshmdirect.cc:377-473,
  transliterated branch by branch over a dict table.  The attrs are opaque bytes of this
  file's own encoding (encode_attrs); all the transliteration asks of them is whether they are
  expired (K2hAttrOpsMan::IsExpire) and whether they carry an mtime, and which (GetMTime).
  replay() feeds a list of blobs to it.  libk2hash itself is not built here.
* Stream builders on top of ralle_check_model's, and the resolve kernel's block width read
  from its source.
"""
import re
import struct

import numpy as np

import ralle_check_model as rm
from ralle_check_model import (F_ALEN, F_HASH, F_KLEN, F_KPOS, F_SLEN, F_SUBHASH, F_VLEN, HEADER,  # noqa: F401
                               M64, ROOT)

_SRC = (ROOT / "k2hash_amd" / "csrc" / "k2h_ralledata_dedup.hip").read_text()


def _const(name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", _SRC)
    assert m, name
    return int(m.group(1))


RESOLVE_BLOCK = _const("kResolveBlock")  # sorted positions per block of the resolve kernel
WAVE = 64
NONE = M64                               # by[i] without a later blob of the same identity


# ------------------------------------------------------------------------------- the model
def identity(raw, b, f):
    """(stored hash, stored subhash, key bytes) of the blob at b with header fields f."""
    return f[0], f[1], bytes(raw[b + f[6]:b + f[6] + f[2]])


def dedup_model(buf, off, size=None, consider=None):
    """(keep uint8, by uint64, dropped) of the stream."""
    raw = bytes(buf)
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    n = len(off) - 1
    keep = np.zeros(n, np.uint8)
    by = np.full(n, NONE, np.uint64)
    last = {}        # identity -> (index, has attrs) of the last participant seen
    dropped = 0
    for i in range(n):
        if consider is not None and not consider[i]:
            continue
        st, f = rm.header_status(raw, off[i], off[i + 1], size)
        if st != rm.OK:
            continue
        keep[i] = 1
        ident, attrs = identity(raw, off[i], f), f[5] != 0
        if ident in last:
            p, p_attrs = last[ident]
            by[p] = i
            if not p_attrs and not attrs:
                keep[p] = 0
                dropped += 1
        last[ident] = (i, attrs)
    return keep, by, dropped


# ------------------------------------------------------------------ the reference's replay
def encode_attrs(mtime=None, expired=False, salt=0):
    """The test's own attrs bytes: a flag byte (1: has an mtime, 2: expired), the mtime as
    (sec, nsec), and a salt that tells two attrs of the same meaning apart."""
    sec, nsec = mtime if mtime is not None else (0, 0)
    return struct.pack("<BqqI", (1 if mtime is not None else 0) | (2 if expired else 0), sec, nsec, salt)


def attrs_expired(attrs):
    return bool(attrs[0] & 2)


def attrs_mtime(attrs):
    """None without an mtime (GetMTime returns false), else (sec, nsec)."""
    if not attrs[0] & 1:
        return None
    return struct.unpack_from("<qq", attrs, 1)


def set_element_by_bin_array(table, blob, pts):
    """lib/k2hshmdirect.cc:343-478 over table: {(hash, subhash, key): (value, subkeys, attrs)},
    each of the three bytes or None (an element without that page).  pts: (sec, nsec)."""
    f = struct.unpack_from("<10Q", blob, 0)
    if f[2] + f[3] + f[4] + f[5] == 0:                                                   # :351
        return False
    if f[2] == 0:                                                                        # :355
        return False
    by_key = bytes(blob[f[6]:f[6] + f[2]])                                               # :361
    by_value = bytes(blob[f[7]:f[7] + f[3]]) if 0 < f[3] else None                       # :362
    by_subkeys = bytes(blob[f[8]:f[8] + f[4]]) if 0 < f[4] else None                     # :363
    by_attrs = bytes(blob[f[9]:f[9] + f[5]]) if 0 < f[5] else None                       # :364
    ident = (f[0], f[1], by_key)          # GetCKIndex(hash), GetElementList(hash, subhash), GetElement(key): :373-378
    element = table.get(ident)
    if element is not None:                                                              # :377-379
        exist_attr = element[2]           # GetAttrs: NULL for an element without an attrs page
        if exist_attr is not None:                                                       # :382
            if attrs_expired(exist_attr):                                                # :390
                pass
            else:
                mtime = attrs_mtime(exist_attr)
                if mtime is None:                                                        # :395
                    pass
                else:
                    if pts[0] < mtime[0] or (pts[0] == mtime[0] and pts[1] <= mtime[1]):  # :402
                        return True
                    new_mtime = attrs_mtime(by_attrs) if by_attrs else None              # :414
                    if new_mtime is not None:
                        if new_mtime[0] < mtime[0] or (new_mtime[0] == mtime[0] and new_mtime[1] <= mtime[1]):  # :416
                            return True
                    else:
                        return True                                                      # :427
    new_element = None
    if by_value is not None or by_subkeys is not None or by_attrs is not None:            # :438
        new_element = (by_value, by_subkeys, by_attrs)
    if element is not None:                                                              # :446
        del table[ident]
    if new_element is not None:                                                          # :462
        table[ident] = new_element
    return True


def replay(blobs, prior, pts):
    """The table after feeding `blobs` in order, starting from a copy of `prior`."""
    table = dict(prior)
    for b in blobs:
        set_element_by_bin_array(table, b, pts)
    return table


# ------------------------------------------------------------------------- stream builders
def blobs_of(oracle, keys, vals=None, skeys=None, attrs=None):
    """One bytearray per record, from the oracle's producer."""
    return rm.split(*rm.stream_of(oracle, (keys, vals, skeys, attrs)))


def set_hash(blob, h=None, sub=None):
    if h is not None:
        rm.put(blob, 0, F_HASH, h)
    if sub is not None:
        rm.put(blob, 0, F_SUBHASH, sub)
    return blob


def at_odd_offsets(blobs, seed=0):
    """The blobs with 0-15 slack bytes inside each (trailing slack is allowed), so that
    their keys fall on every alignment: returns the padded blobs."""
    rng = np.random.default_rng(seed)
    return [bytearray(b) + bytes(int(rng.integers(0, 16))) for b in blobs]
