"""Helper for the tests of k2h_amd_ralledata_times and k2h_amd_ralledata_dedup_mtime (not a test
module, not a conftest).

* serialize_attrs / parse_attrs: the serialized K2HAttrs format, written and parsed as
  K2HAttrs::Serialize does (lib/k2hattrs.cc:59-166); get_time and is_expire on top of the parse,
  K2hAttrBuiltin::GetTime and IsExpire (lib/k2hattrbuiltin.cc:830-883) with the clock passed in.
  tests/golden/ralle_attrs.json, written by the reference's own parser, pins parse_attrs.
* times_model: what k2h_amd_ralledata_times reports (include/k2hash_amd.h section 4b''''), the
  window test being lib/k2hshmdirect.cc:137-197 branch by branch.
* dedup_mtime_model: what k2h_amd_ralledata_dedup_mtime reports, one sequential pass.
* real_attrs: ralle_dedup_model's transliteration of SetElementByBinArray with its two attrs
  hooks swapped for get_time and is_expire over real serialized attrs.
* The enumeration of attrs kinds, prior table states and pts values the replay property and the
  GPU tests share.
"""
import contextlib
import functools
import struct

import numpy as np

import ralle_check_model as rm
import ralle_dedup_model as dm
from ralle_dedup_model import NONE  # noqa: F401

M64 = (1 << 64) - 1
MTIME, EXPIRE = b"mtime\0", b"expire\0"
T_MTIME, T_EXPIRE, T_CUT, T_ATTRS = 1, 2, 4, 8
WIN_START, WIN_END, WIN_EXPIRE = 1, 2, 4
ROUTE_OLD = 2


# --------------------------------------------------------------------------- the attrs format
def timeval(sec, nsec):
    return struct.pack("<qq", sec, nsec)


def serialize_attrs(entries, count=None):
    """count, then (keylength, vallength, key, value) per entry, in the order given."""
    out = struct.pack("<Q", len(entries) if count is None else count & M64)
    for k, v in entries:
        out += struct.pack("<QQ", len(k), len(v)) + bytes(k) + bytes(v)
    return out


def written_attrs(entries):
    """As K2HAttrs::insert and Serialize(out) write them: unique keys, sorted as K2HATTR::compare
    sorts (memcmp over the common length, then the shorter first)."""
    d = {}
    for k, v in entries:
        if len(k):
            d[bytes(k)] = bytes(v)
    return serialize_attrs(sorted(d.items()))


@functools.lru_cache(maxsize=None)
def parse_attrs(a):
    """(accepted: dict key -> value, cut) of the segment `a` (bytes)."""
    got = {}
    if len(a) < 8:
        return got, 0 < len(a)
    count = struct.unpack_from("<Q", a, 0)[0]
    pos, rest, read = 8, len(a) - 8, 0
    while read < count:
        if rest < 16:
            break
        kl, vl = struct.unpack_from("<QQ", a, pos)
        if kl > rest - 16 or vl > rest - 16 - kl:
            break
        if kl:
            got[a[pos + 16:pos + 16 + kl]] = a[pos + 16 + kl:pos + 16 + kl + vl]
        pos += 16 + kl + vl
        rest -= 16 + kl + vl
        read += 1
    return got, read < count


def get_time(a, key):
    """None when GetTime fails, else (sec, nsec)."""
    v = parse_attrs(bytes(a))[0].get(key)
    if v is None or len(v) != 16:
        return None
    return struct.unpack("<qq", v)


def is_expire(a, now):
    e = get_time(a, EXPIRE)
    return e is not None and (e[0] < now[0] or (e[0] == now[0] and e[1] < now[1]))


# ------------------------------------------------------------------------------- the models
class Window:
    """start, end, now: (sec, nsec) or None."""

    def __init__(self, start=None, end=None, now=None):
        self.start, self.end, self.now = start, end, now

    def ctypes(self):
        from k2hash_amd import ralledata
        return ralledata.TimeWindow(self.start, self.end, self.now).ctypes()


def _less(a, b):
    return a[0] < b[0] or (a[0] == b[0] and a[1] < b[1])


def window_keeps(a, window, need_start):
    """lib/k2hshmdirect.cc:137-197 for an element whose attrs segment is `a` (b"": no attrs)."""
    if window.start is None and window.end is None and window.now is None:       # :137
        return True
    if not a:                                                                    # :139
        return True
    if window.now is not None and is_expire(a, window.now):                      # :146
        return False
    if window.start is None and window.end is None:                              # :153
        return True
    mtime = get_time(a, MTIME)
    if mtime is None:                                                            # :155
        return True
    if need_start and window.start is not None and _less(mtime, window.start):   # :179
        return False
    if window.end is not None and _less(window.end, mtime):                      # :184
        return False
    return True


def _participants(raw, off, size, consider):
    for i in range(len(off) - 1):
        if consider is not None and not consider[i]:
            continue
        st, f = rm.header_status(raw, off[i], off[i + 1], size)
        if st == rm.OK:
            yield i, f


def times_model(buf, off, size=None, consider=None, window=None, route=None):
    """(tflags uint8 n, mtime int64 (n, 2), expire int64 (n, 2), keep uint8 n)."""
    raw = bytes(buf)
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    n = len(off) - 1
    flags, keep = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    mtime, expire = np.zeros((n, 2), np.int64), np.zeros((n, 2), np.int64)
    for i, f in _participants(raw, off, size, consider):
        a = raw[off[i] + f[9]:off[i] + f[9] + f[5]] if f[5] else b""
        m, e = get_time(a, MTIME), get_time(a, EXPIRE)
        flags[i] = (T_ATTRS if f[5] else 0) | (T_MTIME if m else 0) | (T_EXPIRE if e else 0) | \
            (T_CUT if parse_attrs(a)[1] else 0)
        mtime[i] = m if m else (0, 0)
        expire[i] = e if e else (0, 0)
        need_start = route is None or bool(route[i] & ROUTE_OLD)
        keep[i] = 1 if window is None or window_keeps(a, window, need_start) else 0
    return flags, mtime, expire, keep


def dedup_mtime_model(buf, off, pts, size=None, consider=None):
    """(keep uint8, by uint64, dropped) under the mtime rule."""
    raw = bytes(buf)
    size = len(raw) if size is None else size
    off = [int(x) for x in off]
    n = len(off) - 1
    keep = np.zeros(n, np.uint8)
    by = np.full(n, NONE, np.uint64)
    last = {}        # identity -> (index, mtime or None) of the last participant seen
    dropped = 0
    for i, f in _participants(raw, off, size, consider):
        keep[i] = 1
        ident = dm.identity(raw, off[i], f)
        m = get_time(raw[off[i] + f[9]:off[i] + f[9] + f[5]], MTIME) if f[5] else None
        if ident in last:
            p, pm = last[ident]
            by[p] = i
            if pm is None or (m is not None and _less(pm, m) and _less(pm, pts)):
                keep[p] = 0
                dropped += 1
        last[ident] = (i, m)
    return keep, by, dropped


# ------------------------------------------------------------------------------- the replay
@contextlib.contextmanager
def real_attrs(now):
    """ralle_dedup_model.set_element_by_bin_array over real serialized attrs: its IsExpire hook
    reads the expire entry against `now`, its GetMTime hook the mtime entry."""
    saved = dm.attrs_expired, dm.attrs_mtime
    dm.attrs_expired = lambda a: is_expire(a, now)
    dm.attrs_mtime = lambda a: get_time(a, MTIME)
    try:
        yield
    finally:
        dm.attrs_expired, dm.attrs_mtime = saved


# -------------------------------------------------------------------------- the enumeration
NOW = (1500, 0)
TIMES = ((900, 0), (950, 0), (950, 1), (1000, 500))
PTS = ((800, 0), (950, 0), (950, 1), (1000, 500), (2000, 0))   # below, equal to each m_i that has a neighbour, above
_UNIQ = (b"uniqid\0", b"a1-b2\0")
_DEAD, _LIVE = (EXPIRE, timeval(1400, 0)), (EXPIRE, timeval(1600, 0))

# attrs a blob can carry, by what GetMTime and IsExpire(NOW) make of them
ATTRS_KINDS = {
    "none": b"",
    "uniqid-only": written_attrs([_UNIQ]),
    "mtime-vl8": written_attrs([(MTIME, bytes(8)), _UNIQ]),
    "m900": written_attrs([(MTIME, timeval(*TIMES[0]))]),
    "m950": written_attrs([(MTIME, timeval(*TIMES[1])), _UNIQ]),
    "m950.1": written_attrs([(MTIME, timeval(*TIMES[2]))]),
    "m1000.500": written_attrs([(MTIME, timeval(*TIMES[3]))]),
    "m950-expired": written_attrs([(MTIME, timeval(*TIMES[1])), _DEAD]),
    "m950-live": written_attrs([(MTIME, timeval(*TIMES[1])), _LIVE, _UNIQ]),
    "expired-only": written_attrs([_DEAD]),
}


def prior_states(ident):
    """The 12 kinds of element a key can have before the stream arrives."""
    val = b"prior-value"
    el = lambda a: {ident: (val, None, a)}  # noqa: E731
    return {
        "absent": {},
        "no-attrs": el(None),
        "uniqid-only": el(ATTRS_KINDS["uniqid-only"]),
        "mtime-vl8": el(ATTRS_KINDS["mtime-vl8"]),
        "m900": el(ATTRS_KINDS["m900"]),
        "m950": el(ATTRS_KINDS["m950"]),
        "m950.1": el(ATTRS_KINDS["m950.1"]),
        "m1000.500": el(ATTRS_KINDS["m1000.500"]),
        "m3000": el(written_attrs([(MTIME, timeval(3000, 0))])),
        "m1000.500-expired": el(written_attrs([(MTIME, timeval(*TIMES[3])), _DEAD])),
        "expired-only": el(ATTRS_KINDS["expired-only"]),
        "m950-live": el(ATTRS_KINDS["m950-live"]),
    }


def pair_cases():
    """(kind of i, key-only i, kind of j, key-only j): every pair of attrs kinds, each blob with
    and without a value."""
    kinds = list(ATTRS_KINDS)
    return [((a, ka), (b, kb)) for a in kinds for ka in (False, True) for b in kinds for kb in (False, True)]


def chain_cases():
    """Three blobs of one key, every triple of attrs kinds (all with a value)."""
    kinds = list(ATTRS_KINDS)
    return [((a, False), (b, False), (c, False)) for a in kinds for b in kinds for c in kinds]


def case_blobs(oracle, cases, distinct_keys):
    """The blobs of the cases laid end to end: a list of bytearrays and, per case, its slice.
    distinct_keys: case c uses the key b"case-%06d" % c, else every blob's key is b"k"."""
    keys, vals, attrs, spans = [], [], [], []
    for c, case in enumerate(cases):
        spans.append((len(keys), len(keys) + len(case)))
        for r, (kind, key_only) in enumerate(case):
            keys.append(b"case-%06d" % c if distinct_keys else b"k")
            vals.append(b"" if key_only else b"v%d" % r)
            attrs.append(ATTRS_KINDS[kind])
    return dm.blobs_of(oracle, keys, vals, None, attrs), spans


# ------------------------------------------------------------------------------ device side
PAD = 64


def place(cuda, buf, shift=0, canary=0xA5, tail_pad=PAD):
    """buf on the device, starting `shift` bytes past a 16-byte boundary, canary bytes around
    it (tail_pad = 0: the tensor ends with buf's last byte)."""
    import torch
    whole = np.full(PAD + shift + len(buf) + tail_pad, canary, np.uint8)
    whole[PAD + shift:PAD + shift + len(buf)] = np.frombuffer(bytes(buf), np.uint8)
    t = torch.from_numpy(whole).to(cuda)
    assert t.data_ptr() % 16 == 0
    return t[PAD + shift:PAD + shift + len(buf)]


def run_times(cuda, t, size, off, consider=None, window=None, route=None):
    """k2h_amd_ralledata_times into sentinel-filled outputs: (tflags, mtime, expire, keep) on
    the host, shaped as times_model's."""
    import ctypes

    import torch

    import big_offsets as bo
    from k2hash_amd import _native
    n = len(off) - 1
    d_off = torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)
    fw, flags = bo.guarded(torch, cuda, n, fill=0xEE)
    kw, keep = bo.guarded(torch, cuda, n, fill=0xEE)
    mfull, mt = bo.sentinel_words(torch, cuda, 2 * n)
    efull, ex = bo.sentinel_words(torch, cuda, 2 * n)
    dev = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.uint8)).to(cuda)  # noqa: E731
    cons, rt = dev(consider), dev(route)
    win = window.ctypes() if window is not None else None
    _native.check(_native.batch_lib().k2h_amd_ralledata_times(
        bo._p(t), size, bo._p(d_off), n, None if cons is None else bo._p(cons),
        None if win is None else ctypes.byref(win), None if rt is None else bo._p(rt), bo._p(flags), bo._p(mt),
        bo._p(ex), bo._p(keep), bo._stream()))
    torch.cuda.synchronize()
    assert bo.guards_intact(torch, fw, flags, 0xEE) and bo.guards_intact(torch, kw, keep, 0xEE), "bytes outside written"
    return (flags.cpu().numpy(), bo.words_back(torch, mfull, 2 * n, "mtime").view(np.int64).reshape(n, 2),
            bo.words_back(torch, efull, 2 * n, "expire").view(np.int64).reshape(n, 2), keep.cpu().numpy())


def assert_times(got, want, what):
    for name, g, w in zip(("tflags", "mtime", "expire", "keep"), got, want):
        bad = np.nonzero(np.asarray(g != w).reshape(len(w), -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {name} differs at blob {int(bad[0])}: got {g[bad[0]]}, want {w[bad[0]]}"


def times_against_model(cuda, buf, off, what, shift=0, consider=None, window=None, route=None, tail_pad=PAD):
    want = times_model(buf, off, consider=consider, window=window, route=route)
    got = run_times(cuda, place(cuda, buf, shift, tail_pad=tail_pad), len(buf), off, consider, window, route)
    assert_times(got, want, what)
    return want


def run_dedup_mtime(cuda, t, size, off, pts, consider=None, plain=False):
    """k2h_amd_ralledata_dedup_mtime (plain: k2h_amd_ralledata_dedup) into sentinel-filled
    outputs: (keep, by, dropped) on the host."""
    import ctypes

    import torch

    import big_offsets as bo
    from k2hash_amd import _native
    n = len(off) - 1
    d_off = torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)
    kw, keep = bo.guarded(torch, cuda, n, fill=0xEE)
    full, by = bo.sentinel_words(torch, cuda, n)
    cons = None if consider is None else torch.from_numpy(np.asarray(consider, np.uint8)).to(cuda)
    dropped = ctypes.c_uint64(0xDEAD)
    lib = _native.batch_lib()
    head = (bo._p(t), size, bo._p(d_off), n, None if cons is None else bo._p(cons), bo._p(keep), bo._p(by),
            ctypes.byref(dropped))
    if plain:
        _native.check(lib.k2h_amd_ralledata_dedup(*head, bo._stream()))
    else:
        ts = _native.Timespec(*pts)
        _native.check(lib.k2h_amd_ralledata_dedup_mtime(*head, ctypes.byref(ts), bo._stream()))
    torch.cuda.synchronize()
    assert bo.guards_intact(torch, kw, keep, 0xEE), "bytes outside keep written"
    return keep.cpu().numpy(), bo.words_back(torch, full, n, "by"), int(dropped.value)


def assert_dedup(got, want, what):
    for name, g, w in zip(("keep", "by"), got[:2], want[:2]):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {name} differs at blob {int(bad[0])}: got {g[bad[0]]}, want {w[bad[0]]}"
    assert got[2] == want[2], f"{what}: dropped {got[2]}, want {want[2]}"
