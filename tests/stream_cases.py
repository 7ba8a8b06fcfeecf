"""The case table of test_stream_contract.py: every public wrapper of k2hash_amd.batch,
k2hash_amd.archive and k2hash_amd.ralledata that takes a `stream`, each with

  build(oracle, seed)   real host inputs: a dict of numpy arrays (they become device tensors) and
                        host values (passed as they are)
  decoy(oracle, inputs) a second valid input set with the same keys, shapes, dtypes and byte
                        sizes -- the same blobs, records or lines in another order, other bytes
                        of the same lengths -- so a kernel that runs before its inputs arrive
                        computes a wrong answer and reads no wild offset
  expect(oracle, inputs) the outputs, from the oracle and the CPU models of the suite, never from
                        a device call
  run(d, stream)        the wrapper called on the device inputs; returns a dict of the outputs
                        (device tensors and host numbers) under the names expect uses

CASES maps "module.function" to the variants of that function; the completeness test holds
its keys against what inspect finds in the three modules.
"""
from typing import Callable, NamedTuple

import numpy as np

import archive_fold_model as am_fold
import ralle_archive_model as am
import ralle_check_model as rm
import ralle_dedup_model as dm
import ralle_diff_model as fm
import ralle_part_model as pm
import ralle_recs_model as rr
import ralle_times_model as tm

from k2hash_amd import archive, batch, ralledata

N = 600          # blobs, records, keys or lines per case: past a 256-thread block and a 64-lane wave, and odd-sized
SENTINEL = 0xEE  # caller-supplied outputs are filled with it on the call's stream first


class Case(NamedTuple):
    name: str
    build: Callable
    decoy: Callable
    expect: Callable
    run: Callable
    is_async: bool = False     # the header documents this form as asynchronous on `stream`
    inert: bool = False        # no input byte reaches an output (n == 0): the decoy cannot change the answer
    by_shape: tuple = ()       # outputs that the inputs' sizes alone fix: equal for every decoy


def _rng(*salt):
    return np.random.default_rng([7700] + [int(x) for x in salt])


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def _i64(x):
    return np.array([int(v) for v in x], np.uint64).view(np.int64)


def _current(torch, stream):
    return stream if stream is not None else torch.cuda.current_stream()


# ----------------------------------------------------------------------------- key batches
def _fixed_build(oracle, seed, key_len=37):
    return dict(keys=oracle.gen_bytes(N * key_len, byte_off=1000 * seed + 3), key_len=key_len)


def _fixed_decoy(oracle, d):
    return dict(d, keys=oracle.gen_bytes(d["keys"].size, seed=oracle.SEED_LENS, byte_off=17))


def _csr_build(oracle, seed):
    lens = _rng(1, seed).integers(0, 300, N)
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return dict(data=oracle.gen_bytes(int(off[-1]), byte_off=2000 * seed + 5), offsets=off.view(np.int64))


def _csr_decoy(oracle, d):
    """The same lengths in another order over other bytes: the same total."""
    off = d["offsets"].view(np.uint64)
    lens = np.diff(off)[_rng(2, off.size).permutation(off.size - 1)]
    o = np.zeros_like(off)
    o[1:] = np.cumsum(lens)
    return dict(d, data=oracle.gen_bytes(d["data"].size, seed=oracle.SEED_LENS, byte_off=23), offsets=o.view(np.int64))


CUR_MASK, COL_MASK = 0xFFF, 0xF


def _index_of(oracle, h1):
    k, c = oracle.bucket_index(h1, CUR_MASK, COL_MASK)
    return dict(kindex=k, ckindex=c)


def _bitmap(seed):
    """A sparse table snapshot: few entries assigned, so that the walk down cur_mask ends at
    every depth and for some hashes finds nothing."""
    bits = _rng(7, seed).random(CUR_MASK + 1) < 0.15
    return np.packbits(bits, bitorder="little").view(np.int32)


def _table_build(base):
    def build(oracle, seed):
        return dict(base(oracle, seed), assigned=_bitmap(seed))
    return build


def _table_decoy(base):
    def decoy(oracle, d):
        return dict(base(oracle, d), assigned=_bitmap(991))
    return decoy


def _table_of(oracle, h1, d):
    k, c, f = oracle.bucket_index_table(h1, CUR_MASK, COL_MASK, d["assigned"].view(np.uint32))
    return dict(kindex=k, ckindex=c, found=f)


def _fixed_h(oracle, d):
    return oracle.hash_fixed(d["keys"], d["key_len"])


def _csr_h(oracle, d):
    return oracle.hash_csr(d["data"], d["offsets"].view(np.uint64))


def _h1_build(oracle, seed):
    return dict(h1=_rng(3, seed).integers(0, 1 << 63, N, dtype=np.int64) * 2 + 1)


def _h1_decoy(oracle, d):
    return dict(d, h1=_rng(4).integers(0, 1 << 63, N, dtype=np.int64) * 2)


def _named(names, values):
    return {k: v for k, v in zip(names, values) if v is not None}


def _run_hash_fixed_out(d, stream):
    import torch
    with torch.cuda.stream(_current(torch, stream)):
        out = tuple(torch.full((N,), -0x1212121212121212, dtype=torch.int64, device=d["keys"].device) for _ in range(2))
    return _named(("h1", "h2"), batch.hash_fixed(d["keys"], d["key_len"], second=True, out=out, stream=stream))


def _ranges_build(oracle, seed):
    rng = _rng(5, seed)
    lens = rng.integers(0, 120, N)
    return dict(base=oracle.gen_bytes(40000, byte_off=77 * seed), starts=rng.integers(0, 40000 - 120, N).astype(np.int64),
                lens=lens.astype(np.int64))


def _ranges_decoy(oracle, d):
    p = _rng(6).permutation(N)
    return dict(base=oracle.gen_bytes(40000, seed=oracle.SEED_LENS), starts=d["starts"][p], lens=d["lens"][p])


def _ranges_expect(oracle, d):
    keys = [d["base"][int(s):int(s) + int(n)].tobytes() for s, n in zip(d["starts"], d["lens"])]
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum([len(k) for k in keys])
    h1, h2 = oracle.hash_csr(_u8(b"".join(keys) or b"\0"), off)
    return dict(h1=h1, h2=h2)


# --------------------------------------------------------------------------- synthetic data
def _synth_build(oracle, seed):
    return dict(seed=batch.SEED_BYTES + seed, first=11 * seed + 1)


def _synth_decoy(oracle, d):
    return dict(seed=d["seed"] ^ 0x5555, first=d["first"] + 7)


# ---------------------------------------------------------------------------- blob streams
def _blobs(oracle, seed, n=N):
    """n blobs of mixed lengths: keys that repeat, values on both sides of the diff's wave
    threshold, real serialized attrs with and without an mtime, and some stored hashes wrong."""
    rng = _rng(10, seed)
    kinds = list(tm.ATTRS_KINDS.values())
    ids = rng.integers(0, max(n // 2, 1), n)
    keys = [b"key-%d-%d" % (seed, i) + b"k" * int(i % 29) for i in ids]
    vals = [b"" if rng.random() < 0.1 else rng.bytes(int(rng.integers(1, 2 * fm.WAVE_BYTES))) for _ in range(n)]
    skeys = [rng.bytes(int(rng.integers(1, 40))) if rng.random() < 0.2 else b"" for _ in range(n)]
    attrs = [kinds[int(rng.integers(0, len(kinds)))] if rng.random() < 0.6 else b"" for _ in range(n)]
    blobs = dm.blobs_of(oracle, keys, vals, skeys, attrs)
    for i in np.flatnonzero(rng.random(n) < 0.08):
        rm.put(blobs[i], 0, rm.F_HASH, rm.get(blobs[i], 0, rm.F_HASH) ^ 0x10)
    for i in np.flatnonzero(rng.random(n) < 0.04):
        rm.put(blobs[i], 0, rm.F_SUBHASH, rm.get(blobs[i], 0, rm.F_SUBHASH) ^ 0x4000)
    return blobs


def _joined(blobs, prefix=""):
    buf, off = rm.join(blobs)
    return {prefix + "blobs": _u8(buf) if len(buf) else np.zeros(0, np.uint8), prefix + "blob_off": _i64(off)}


def _mask(seed, n=N, p=0.6):
    return (_rng(11, seed).random(n) < p).astype(np.uint8)


def _stream_build(**extra):
    def build(oracle, seed):
        d = _joined(_blobs(oracle, seed))
        for k, make in extra.items():
            d[k] = make(seed)
        return d
    return build


def _shuffled(d, prefix="", salt=0):
    """The stream's blobs in another order, a third of them under another stored hash."""
    buf, off = bytes(d[prefix + "blobs"]), d[prefix + "blob_off"]
    blobs = rm.split(bytearray(buf), [int(x) for x in off])
    rng = _rng(12, salt, len(blobs))
    blobs = [blobs[i] for i in rng.permutation(len(blobs))]
    for b in blobs:
        if len(b) >= rm.HEADER and rng.random() < 0.33:
            rm.put(b, 0, rm.F_HASH, int(rng.integers(0, 1 << 62)))
    return _joined(blobs, prefix)


def _stream_decoy(oracle, d):
    out = dict(d, **_shuffled(d))
    for k in ("keep", "consider"):
        if k in d:
            out[k] = _other_mask(d[k])
    return out


def _other_mask(m):
    """Another mask of the same size with another number of ones."""
    out = m[::-1].copy()
    out[np.flatnonzero(out)[::7]] = 0
    return out


def _raw(d, prefix=""):
    return bytes(d[prefix + "blobs"]), [int(x) for x in d[prefix + "blob_off"]]


RANGE = rm.Range(3, 16, 6, 1, 8)
WINDOW = dict(start=(940, 0), end=(1000, 0), now=tm.NOW)
PTS = (950, 1)
OWNER = pm.owner_rule(1000, 130)


def _check_expect(oracle, d):
    return _named(("status", "route", "h1", "h2"), rm.expected(oracle, d["blobs"], d["blob_off"], rng=RANGE))


def _run_check(d, stream):
    res = ralledata.check_ralledata(d["blobs"], d["blob_off"], RANGE.ctypes(), want_hashes=True, stream=stream)
    return res._asdict()


def _selected(sel):
    return dict(blobs=sel.blobs, blob_off=sel.blob_off, index=sel.index, kept=sel.kept, kept_bytes=sel.kept_bytes)


def _select_expect(oracle, d):
    data, ooff, index = rm.select_model(_u8(d["blobs"]), d["blob_off"], d["keep"])
    return dict(blobs=data, blob_off=ooff, index=index, kept=len(index), kept_bytes=int(data.size))


def _partition_expect(oracle, d):
    buf, off = _raw(d)
    data, ooff, index, part, first, byte = pm.partition_model(buf, off, len(buf), OWNER, consider=d.get("consider"))
    return dict(blobs=data, blob_off=ooff, index=index, part_of=part, part_first=[int(x) for x in first],
                part_byte=[int(x) for x in byte], kept=len(index), kept_bytes=int(data.size))


def _run_partition(d, stream):
    return ralledata.partition_ralledata(d["blobs"], d["blob_off"], OWNER.parts, owner=(OWNER.max_hash, OWNER.span),
                                         consider=d.get("consider"), want_parts=True, stream=stream)._asdict()


def _empty_build(oracle, seed):
    return dict(blobs=np.zeros(0, np.uint8), blob_off=np.zeros(1, np.int64))


def _to_archive_expect(oracle, d):
    data, rec_off, records, _segs = am.model(*_raw(d), keep=d.get("keep"))
    return dict(bytes=data, rec_off=rec_off, records=records, total=int(data.size))


def _times_expect(oracle, d):
    return _named(("flags", "mtime", "expire", "keep"),
                  tm.times_model(*_raw(d), consider=d["consider"], window=tm.Window(**WINDOW)))


def _run_times(d, stream):
    return ralledata.blob_times(d["blobs"], d["blob_off"], consider=d["consider"], window=ralledata.TimeWindow(**WINDOW),
                                stream=stream)._asdict()


def _dedup_case(name, pts, count):
    def expect(oracle, d):
        model = dm.dedup_model(*_raw(d), consider=d["consider"]) if pts is None else \
            tm.dedup_mtime_model(*_raw(d), pts, consider=d["consider"])
        return _named(("keep", "by", "dropped"), model[:2] + ((model[2],) if count else (None,)))

    def run(d, stream):
        return _named(("keep", "by", "dropped"), ralledata.dedup_ralledata(
            d["blobs"], d["blob_off"], consider=d["consider"], want_by=True, count=count, stream=stream, pts=pts))
    return Case(name, _stream_build(consider=lambda s: _mask(s, p=0.9)), _stream_decoy, expect, run, is_async=not count)


def _diff_build(oracle, seed, na=N, nb=N // 2):
    """A: a stream; B: blobs of A's identities, some as A holds them, some with a byte of the
    value changed, so that pairs on both sides of the wave threshold compare equal and unequal."""
    a = _blobs(oracle, seed, na)
    rng = _rng(13, seed)
    b = []
    for i in rng.integers(0, na, nb):
        x = bytearray(a[i])
        vl, vp = rm.get(x, 0, rm.F_VLEN), rm.get(x, 0, rm.F_VPOS)
        if vl and rng.random() < 0.5:
            x[vp + vl - 1] ^= 0x21
        b.append(x)
    d = dict(_joined(a, "a_"), **_joined(b, "b_"))
    d["a_consider"], d["b_consider"] = _mask(seed, na, 0.9), _mask(seed + 1, nb, 0.9)
    return d


def _diff_decoy(oracle, d):
    out = dict(d, **_shuffled(d, "a_", 1))
    out.update(_shuffled(d, "b_", 2))
    out["a_consider"], out["b_consider"] = _other_mask(d["a_consider"]), _other_mask(d["b_consider"])
    return out


def _diff_case(name, count, build=_diff_build):
    def expect(oracle, d):
        rel, match, seen, counts = fm.diff_model(*_raw(d, "a_"), *_raw(d, "b_"), d["a_consider"], d["b_consider"],
                                                 times=(PTS, tm.NOW))
        out = dict(rel=rel, match=match, seen=seen, feed=fm.feed_of(rel).astype(np.uint8))
        if count:
            out.update(zip(("participants", "found", "same", "apply"), counts))
        return out

    def run(d, stream):
        res = ralledata.diff_ralledata(d["a_blobs"], d["a_blob_off"], d["b_blobs"], d["b_blob_off"], d["a_consider"],
                                       d["b_consider"], pts=PTS, now=tm.NOW, want_match=True, want_seen=True, count=count,
                                       stream=stream)
        return {k: v for k, v in res._asdict().items() if v is not None}
    return Case(name, build, _diff_decoy, expect, run, is_async=not count)


def _route_expect(oracle, d):
    buf, off = _raw(d)
    status, route, _h1, _h2 = rm.expected(oracle, d["blobs"], off, rng=RANGE)
    keep = ((status == rm.OK) & ((route & 1) != 0)).astype(np.uint8)
    keep &= tm.times_model(buf, off, consider=keep, window=tm.Window(**WINDOW), route=route)[3]
    keep &= tm.dedup_mtime_model(buf, off, PTS, consider=keep)[0]
    return dict(_select_expect(oracle, dict(d, keep=keep)), status=status, route=route)


def _run_route(d, stream):
    sel, res = ralledata.route_ralledata(d["blobs"], d["blob_off"], RANGE.ctypes(), stream=stream, dedup=True,
                                         window=ralledata.TimeWindow(**WINDOW), pts=PTS)
    return dict(_selected(sel), status=res.status, route=res.route)


# ------------------------------------------------------------------------ host structs
# The other valid value each host struct is overwritten with while its call still waits
# (test_host_struct_is_consumed_before_return), next to the one the cases above use.
RANGE_2 = rm.Range(1, 5, 2, 0, 3)
WINDOW_2 = dict(start=None, end=(900, 0), now=None)
PTS_2, NOW_2 = (100, 0), (100, 0)
MASKS_2 = (0xFF, 0x3)     # smaller masks read a prefix of the same bitmap


def abi_expect(oracle, entry, d, other=False):
    """What C entry point `entry` writes for the inputs d of its wrapper's case, under the
    struct of the case table or (other) under the value it is overwritten with."""
    if entry == "k2h_amd_ralledata_check":
        return _named(("status", "route", "h1", "h2"),
                      rm.expected(oracle, d["blobs"], d["blob_off"], rng=RANGE_2 if other else RANGE))
    if entry == "k2h_amd_ralledata_times":
        window = tm.Window(**(WINDOW_2 if other else WINDOW))
        return _named(("flags", "mtime", "expire", "keep"), tm.times_model(*_raw(d), consider=d["consider"], window=window))
    if entry == "k2h_amd_ralledata_dedup_mtime":
        return _named(("keep", "by"), tm.dedup_mtime_model(*_raw(d), PTS_2 if other else PTS, consider=d["consider"]))
    if entry == "k2h_amd_ralledata_diff":
        times = (PTS_2, NOW_2) if other else (PTS, tm.NOW)
        return _named(("rel", "match", "seen"), fm.diff_model(*_raw(d, "a_"), *_raw(d, "b_"), d["a_consider"],
                                                              d["b_consider"], times=times))
    cur, col = MASKS_2 if other else (CUR_MASK, COL_MASK)
    hashes = {"k2h_amd_bucket_index_table": lambda: (d["h1"].view(np.uint64), None),
              "k2h_amd_hash_fixed_index_table": lambda: _fixed_h(oracle, d),
              "k2h_amd_hash_csr_index_table": lambda: _csr_h(oracle, d)}[entry]()
    k, c, f = oracle.bucket_index_table(hashes[0], cur, col, d["assigned"].view(np.uint32))
    out = dict(kindex=k, ckindex=c, found=f)
    if hashes[1] is not None:
        out.update(h1=hashes[0], h2=hashes[1])
    return out


# ------------------------------------------------------------------- blobs from four segments
_SEG_CAP = {"keys": 40, "vals": 120, "attrs": 60}   # bytes per record each segment's tensor has room for


def _segs_build(lo_frac, hi_frac):
    def build(oracle, seed):
        rng = _rng(14, seed)
        d = {}
        for name, cap in _SEG_CAP.items():
            lo = max(int(cap * lo_frac), 1 if name == "keys" else 0)
            parts = [rng.bytes(int(x)) for x in rng.integers(lo, int(cap * hi_frac), N)]
            data = np.zeros(cap * N, np.uint8)
            joined = b"".join(parts)
            data[:len(joined)] = _u8(joined) if joined else 0
            off = np.zeros(N + 1, np.int64)
            off[1:] = np.cumsum([len(p) for p in parts])
            d[name], d[name[:-1] + "_off"] = data, off
        return d
    return build


def _segs_decoy(oracle, d):
    """Longer segments in tensors of the same sizes: the offsets end elsewhere, and a size
    read from them too early is too large, never too small."""
    out = _segs_build(0.5, 1.0)(oracle, 424242)
    assert all(out[k][-1] > d[k][-1] for k in ("key_off", "val_off", "attr_off"))
    return out


def _segs_permuted(oracle, d):
    """The same records in another order: every size and the total stay."""
    p = _rng(19).permutation(N)
    out = dict(d)
    for name, parts in zip(("keys", "vals", "attrs"), (x for x in _segs_lists(d) if x is not None)):
        joined = b"".join(parts[i] for i in p)
        data = np.zeros_like(d[name])
        data[:len(joined)] = _u8(joined) if joined else 0
        off = np.zeros(N + 1, np.int64)
        off[1:] = np.cumsum([len(parts[i]) for i in p])
        out[name], out[name[:-1] + "_off"] = data, off
    return out


def _segs_lists(d):
    def cut(name):
        data, off = d[name], d[name[:-1] + "_off"]
        return [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(N)]
    return cut("keys"), cut("vals"), None, cut("attrs")


def _segs_expect(oracle, d):
    out, boff = oracle.build_ralledata(*_segs_lists(d))
    return dict(blobs=out, blob_off=boff)


def _run_build(d, stream):
    blobs, off = ralledata.build_ralledata(d["keys"], d["key_off"], d["vals"], d["val_off"], None, None, d["attrs"],
                                           d["attr_off"], stream=stream)
    return dict(blobs=blobs, blob_off=off)


def _segs_build_total(oracle, seed):
    d = _segs_build(0.0, 0.5)(oracle, seed)
    d["total"] = ralledata.HEADER * N + sum(int(d[k][-1]) for k in ("key_off", "val_off", "attr_off"))
    return d


def _run_build_total(d, stream):
    import torch
    dev = d["keys"].device
    with torch.cuda.stream(_current(torch, stream)):
        out = torch.full((d["total"],), SENTINEL, dtype=torch.uint8, device=dev)
        boff = torch.full((N + 1,), -1, dtype=torch.int64, device=dev)
    blobs, off = ralledata.build_ralledata(d["keys"], d["key_off"], d["vals"], d["val_off"], None, None, d["attrs"],
                                           d["attr_off"], out=out, blob_off=boff, total=d["total"], stream=stream)
    return dict(blobs=blobs, blob_off=off)


# ---------------------------------------------------------------------------- import files
def _lines(seed, n=N):
    rng = _rng(15, seed)
    return [b"k%d-%d-" % (seed, i) + bytes(rng.integers(97, 123, int(rng.integers(1, 40))).astype(np.uint8)) + b"\t" +
            bytes(rng.integers(97, 123, int(rng.integers(0, 60))).astype(np.uint8)) + b"\n" for i in range(n)]


def _import_build(with_recs):
    def build(oracle, seed):
        data = b"".join(_lines(seed))
        d = dict(file=_u8(data))
        if with_recs:
            d["recs"] = archive.import_scan(data, "tsv").view(np.int64).reshape(-1, 4).copy()
        return d
    return build


def _import_decoy(oracle, d):
    lines = bytes(d["file"]).splitlines(keepends=True)
    data = b"".join(lines[i] for i in _rng(16).permutation(len(lines)))
    out = dict(file=_u8(data))
    if "recs" in d:
        out["recs"] = archive.import_scan(data, "tsv").view(np.int64).reshape(-1, 4).copy()
    return out


def _import_recs(d):
    data = bytes(d["file"])
    return data, (d["recs"].view(np.uint64) if "recs" in d else
                  archive.import_scan(data, "tsv").view(np.uint64).reshape(-1, 4))


def _import_hashes(oracle, d):
    data, recs = _import_recs(d)
    keys = [data[int(r[0]):int(r[0]) + int(r[1])] + b"\0" for r in recs]   # K2HShm::Set(const char*): key + NUL
    return dict(h1=np.array([oracle.k2h_hash(k) for k in keys], np.uint64),
                h2=np.array([oracle.k2h_second_hash(k) for k in keys], np.uint64))


def _import_scan_expect(oracle, d):
    return dict(recs=_import_recs(d)[1])


def _import_blobs_expect(oracle, d):
    data, recs = _import_recs(d)
    blobs, off = rr.expected(oracle, data, [rr.import_segments(r, len(data)) for r in recs], nul=True)
    return dict(blobs=blobs, blob_off=off)


def _import_archive_expect(oracle, d):
    s = _import_blobs_expect(oracle, d)
    return _to_archive_expect(oracle, dict(blobs=s["blobs"], blob_off=s["blob_off"]))


# --------------------------------------------------------------------------- archive files
def _archive_records(seed, n=N):
    rng = _rng(17, seed)
    types = rng.choice(7, n, p=[0.5, 0.14, 0.08, 0.1, 0.06, 0.08, 0.04])
    out = []
    for i, t in enumerate(types):
        key = b"key-%d-%d" % (seed, int(rng.integers(0, n // 4)))
        out.append(am_fold.scom_record(int(t), key, rng.bytes(int(rng.integers(0, 90))),
                                       rng.bytes(int(rng.integers(0, 20))) if rng.random() < 0.3 else b"",
                                       rng.bytes(int(rng.integers(0, 30))) if rng.random() < 0.3 else b"",
                                       b"new-%d" % i if t in (am_fold.OW_VAL, am_fold.RENAME) else b""))
    return out


def _host_recs(data):
    return archive.scan(data).view(np.int64).reshape(-1, archive.REC_WORDS).copy()


def _archive_build(with_recs):
    def build(oracle, seed):
        data = b"".join(_archive_records(seed))
        d = dict(file=_u8(data))
        if with_recs:
            d["recs"] = _host_recs(data)
        return d
    return build


def _archive_decoy(oracle, d):
    data = bytes(d["file"])
    recs = archive.scan(data)
    ends = [int(o) for o in recs["offset"][1:]] + [len(data)]
    pieces = [data[int(b):e] for b, e in zip(recs["offset"], ends)]
    data = b"".join(pieces[i] for i in _rng(18).permutation(len(pieces)))
    out = dict(file=_u8(data))
    if "recs" in d:
        out["recs"] = _host_recs(data)
    return out


def _scan_expect(oracle, d):
    return dict(recs=_host_recs(bytes(d["file"])))


def _prehash_expect(oracle, d):
    data = bytes(d["file"])
    recs = archive.scan(data)
    out = {k: np.zeros(recs.size, np.uint64) for k in ("h1", "h2", "new_h1", "new_h2")}
    for i, r in enumerate(recs):
        assert int(r["status"]) == 0
        key = data[int(r["key_off"]):int(r["key_off"]) + int(r["key_len"])]
        out["h1"][i], out["h2"][i] = oracle.k2h_hash(key), oracle.k2h_second_hash(key)
        if int(r["type"]) == archive.SCOM_RENAME and int(r["exdata_len"]):
            new = data[int(r["exdata_off"]):int(r["exdata_off"]) + int(r["exdata_len"])]
            out["new_h1"][i], out["new_h2"][i] = oracle.k2h_hash(new), oracle.k2h_second_hash(new)
    return out


_HNAMES = ("h1", "h2", "new_h1", "new_h2")


def _fold_expect(oracle, d):
    data = bytes(d["file"])
    keep, by, dropped = am_fold.fold_model(am_fold.recs_of(data, archive.scan(data)))
    return dict(keep=keep, by=by, dropped=dropped, recs=_host_recs(data))


def _compact_expect(oracle, d):
    data = bytes(d["file"])
    recs = archive.scan(data)
    keep = am_fold.fold_model(am_fold.recs_of(data, recs))[0]
    ends = [int(o) for o in recs["offset"][1:]] + [len(data)]
    kept = [i for i in range(recs.size) if keep[i]]
    out = b"".join(data[int(recs["offset"][i]):ends[i]] for i in kept)
    return dict(bytes=_u8(out), index=np.array(kept, np.uint64), kept=len(kept), kept_bytes=len(out), records=int(recs.size))


def _archive_blobs_expect(oracle, d):
    data = bytes(d["file"])
    blobs, off = rr.expected(oracle, data, [rr.archive_segments(r, len(data)) for r in archive.scan(data)], nul=False)
    return dict(blobs=blobs, blob_off=off)


# ------------------------------------------------------------------------------- the table
def _one(func, build, decoy, expect, run, **kw):
    return [Case(func, build, decoy, expect, run, **kw)]


_S = _stream_build
CASES = {
    "batch.hash_fixed": [
        Case("batch.hash_fixed", _fixed_build, _fixed_decoy,
             lambda o, d: _named(("h1", "h2"), _fixed_h(o, d)),
             lambda d, s: _named(("h1", "h2"), batch.hash_fixed(d["keys"], d["key_len"], second=True, stream=s)),
             is_async=True),
        Case("batch.hash_fixed[out]", _fixed_build, _fixed_decoy,
             lambda o, d: _named(("h1", "h2"), _fixed_h(o, d)), _run_hash_fixed_out, is_async=True)],
    "batch.hash_csr": _one(
        "batch.hash_csr", _csr_build, _csr_decoy, lambda o, d: _named(("h1", "h2"), _csr_h(o, d)),
        lambda d, s: _named(("h1", "h2"), batch.hash_csr(d["data"], d["offsets"], second=True, stream=s)), is_async=True),
    "batch.bucket_index": _one(
        "batch.bucket_index", _h1_build, _h1_decoy, lambda o, d: _index_of(o, d["h1"]),
        lambda d, s: _named(("kindex", "ckindex"), batch.bucket_index(d["h1"], CUR_MASK, COL_MASK, stream=s)),
        is_async=True),
    "batch.hash_fixed_index": _one(
        "batch.hash_fixed_index", _fixed_build, _fixed_decoy,
        lambda o, d: dict(_named(("h1", "h2"), _fixed_h(o, d)), **_index_of(o, _fixed_h(o, d)[0])),
        lambda d, s: _named(("h1", "h2", "kindex", "ckindex"), batch.hash_fixed_index(
            d["keys"], d["key_len"], CUR_MASK, COL_MASK, second=True, stream=s)), is_async=True),
    "batch.hash_csr_index": _one(
        "batch.hash_csr_index", _csr_build, _csr_decoy,
        lambda o, d: dict(_named(("h1", "h2"), _csr_h(o, d)), **_index_of(o, _csr_h(o, d)[0])),
        lambda d, s: _named(("h1", "h2", "kindex", "ckindex"), batch.hash_csr_index(
            d["data"], d["offsets"], CUR_MASK, COL_MASK, second=True, stream=s)), is_async=True),
    "batch.bucket_index_table": _one(
        "batch.bucket_index_table", _table_build(_h1_build), _table_decoy(_h1_decoy),
        lambda o, d: _table_of(o, d["h1"].view(np.uint64), d),
        lambda d, s: _named(("kindex", "ckindex", "found"), batch.bucket_index_table(
            d["h1"], CUR_MASK, COL_MASK, d["assigned"], stream=s)), is_async=True),
    "batch.hash_fixed_index_table": _one(
        "batch.hash_fixed_index_table", _table_build(_fixed_build), _table_decoy(_fixed_decoy),
        lambda o, d: dict(_named(("h1", "h2"), _fixed_h(o, d)), **_table_of(o, _fixed_h(o, d)[0], d)),
        lambda d, s: _named(("h1", "h2", "kindex", "ckindex", "found"), batch.hash_fixed_index_table(
            d["keys"], d["key_len"], CUR_MASK, COL_MASK, d["assigned"], second=True, stream=s)), is_async=True),
    "batch.hash_csr_index_table": _one(
        "batch.hash_csr_index_table", _table_build(_csr_build), _table_decoy(_csr_decoy),
        lambda o, d: dict(_named(("h1", "h2"), _csr_h(o, d)), **_table_of(o, _csr_h(o, d)[0], d)),
        lambda d, s: _named(("h1", "h2", "kindex", "ckindex", "found"), batch.hash_csr_index_table(
            d["data"], d["offsets"], CUR_MASK, COL_MASK, d["assigned"], second=True, stream=s)), is_async=True),
    "batch.synth_bytes": _one(
        "batch.synth_bytes", _synth_build, _synth_decoy,
        lambda o, d: dict(bytes=o.gen_bytes(50001, seed=d["seed"], byte_off=d["first"])),
        lambda d, s: dict(bytes=batch.synth_bytes(50001, "cuda:0", seed=d["seed"], byte_off=d["first"], stream=s)),
        is_async=True),
    "batch.synth_offsets": _one(
        "batch.synth_offsets", _synth_build, _synth_decoy,
        lambda o, d: dict(offsets=o.gen_offsets(N, 3, 200, seed=d["seed"], first_key=d["first"])),
        lambda d, s: dict(offsets=batch.synth_offsets(N, "cuda:0", 3, 200, seed=d["seed"], first_key=d["first"],
                                                      stream=s))),
    "archive.hash_ranges": _one(
        "archive.hash_ranges", _ranges_build, _ranges_decoy, _ranges_expect,
        lambda d, s: _named(("h1", "h2"), archive.hash_ranges(d["base"], d["starts"], d["lens"], second=True, stream=s))),
    "archive.scan_device": _one(
        "archive.scan_device", _archive_build(False), _archive_decoy, _scan_expect,
        lambda d, s: dict(recs=archive.scan_device(d["file"], stream=s))),
    "archive.prehash_device": _one(
        "archive.prehash_device", _archive_build(True), _archive_decoy, _prehash_expect,
        lambda d, s: _named(_HNAMES, archive.prehash_device(d["file"], d["recs"], rename=True, stream=s)), is_async=True),
    "archive.scan_prehash_device": _one(
        "archive.scan_prehash_device", _archive_build(False), _archive_decoy,
        lambda o, d: dict(_prehash_expect(o, d), **_scan_expect(o, d)),
        lambda d, s: _named(("recs",) + _HNAMES, archive.scan_prehash_device(d["file"], rename=True, stream=s))),
    "archive.fold_device": _one(
        "archive.fold_device", _archive_build(False), _archive_decoy, _fold_expect,
        lambda d, s: archive.fold_device(d["file"], want_by=True, stream=s)._asdict()),
    "archive.compact_device": _one(
        "archive.compact_device", _archive_build(False), _archive_decoy, _compact_expect,
        lambda d, s: archive.compact_device(d["file"], stream=s)._asdict(), by_shape=("records",)),
    "archive.import_scan_device": _one(
        "archive.import_scan_device", _import_build(False), _import_decoy, _import_scan_expect,
        lambda d, s: dict(recs=archive.import_scan_device(d["file"], "tsv", stream=s))),
    "archive.import_prehash_device": _one(
        "archive.import_prehash_device", _import_build(True), _import_decoy, _import_hashes,
        lambda d, s: _named(("h1", "h2"), archive.import_prehash_device(d["file"], d["recs"], stream=s)), is_async=True),
    "archive.import_scan_prehash_device": _one(
        "archive.import_scan_prehash_device", _import_build(False), _import_decoy,
        lambda o, d: dict(_import_hashes(o, d), **_import_scan_expect(o, d)),
        lambda d, s: _named(("recs", "h1", "h2"), archive.import_scan_prehash_device(d["file"], "tsv", stream=s))),
    "ralledata.build_ralledata": [
        Case("ralledata.build_ralledata", _segs_build(0.0, 0.5), _segs_decoy, _segs_expect, _run_build),
        Case("ralledata.build_ralledata[total,out]", _segs_build_total, _segs_permuted, _segs_expect, _run_build_total,
             is_async=True)],
    "ralledata.import_to_ralledata": _one(
        "ralledata.import_to_ralledata", _import_build(True), _import_decoy, _import_blobs_expect,
        lambda d, s: _named(("blobs", "blob_off"), ralledata.import_to_ralledata(d["file"], d["recs"], stream=s))),
    "ralledata.archive_to_ralledata": _one(
        "ralledata.archive_to_ralledata", _archive_build(True), _archive_decoy, _archive_blobs_expect,
        lambda d, s: _named(("blobs", "blob_off"), ralledata.archive_to_ralledata(d["file"], d["recs"], stream=s))),
    "ralledata.import_file_to_ralledata": _one(
        "ralledata.import_file_to_ralledata", _import_build(False), _import_decoy, _import_blobs_expect,
        lambda d, s: _named(("blobs", "blob_off"), ralledata.import_file_to_ralledata(d["file"], "tsv", stream=s))),
    "ralledata.check_ralledata": _one(
        "ralledata.check_ralledata", _S(), _stream_decoy, _check_expect, _run_check, is_async=True),
    "ralledata.select_ralledata": _one(
        "ralledata.select_ralledata", _S(keep=_mask), _stream_decoy, _select_expect,
        lambda d, s: _selected(ralledata.select_ralledata(d["blobs"], d["blob_off"], d["keep"], stream=s))),
    "ralledata.partition_ralledata": [
        Case("ralledata.partition_ralledata", _S(consider=lambda s: _mask(s, p=0.9)), _stream_decoy, _partition_expect,
             _run_partition),
        Case("ralledata.partition_ralledata[n=0]", _empty_build, lambda o, d: _empty_build(o, 0), _partition_expect,
             _run_partition, inert=True)],
    "ralledata.ralledata_to_archive": _one(
        "ralledata.ralledata_to_archive", _S(keep=_mask), _stream_decoy, _to_archive_expect,
        lambda d, s: ralledata.ralledata_to_archive(d["blobs"], d["blob_off"], keep=d["keep"], stream=s)._asdict()),
    "ralledata.import_file_to_archive": _one(
        "ralledata.import_file_to_archive", _import_build(False), _import_decoy, _import_archive_expect,
        lambda d, s: ralledata.import_file_to_archive(d["file"], "tsv", stream=s)._asdict(),
        by_shape=("records", "total")),
    "ralledata.blob_times": _one(
        "ralledata.blob_times", _S(consider=lambda s: _mask(s, p=0.9)), _stream_decoy, _times_expect, _run_times,
        is_async=True),
    "ralledata.dedup_ralledata": [
        _dedup_case("ralledata.dedup_ralledata[count=False]", None, False),
        _dedup_case("ralledata.dedup_ralledata[count=False,pts]", PTS, False),
        _dedup_case("ralledata.dedup_ralledata[count]", None, True)],
    "ralledata.diff_ralledata": [
        _diff_case("ralledata.diff_ralledata[count=False]", False),
        _diff_case("ralledata.diff_ralledata[count]", True)],
    "ralledata.route_ralledata": _one(
        "ralledata.route_ralledata", _S(), _stream_decoy, _route_expect, _run_route),
}

ALL = [c for variants in CASES.values() for c in variants]
BY_NAME = {c.name: c for c in ALL}

_memo = {}


def inputs(oracle, name, seed):
    """(real, decoy, expected of real, expected of decoy) of a case at a seed; computed once
    and shared, so treat them as read-only."""
    key = (name, seed)
    if key not in _memo:
        c = BY_NAME[name]
        real = c.build(oracle, seed)
        decoy = c.decoy(oracle, real)
        _memo[key] = (real, decoy, c.expect(oracle, real), c.expect(oracle, decoy))
    return _memo[key]


def same(got, want):
    """got == want exactly: arrays by shape and bit pattern, host numbers and lists by value."""
    if isinstance(want, np.ndarray):
        got = np.ascontiguousarray(got)
        want = np.ascontiguousarray(want)
        if got.dtype != want.dtype and got.dtype.itemsize == want.dtype.itemsize and got.dtype.kind in "iu":
            got = got.view(want.dtype)
        return got.shape == want.shape and got.dtype == want.dtype and bool((got == want).all())
    return type(got) in (int, list) and got == want


def public_stream_functions():
    """"module.function" of every public function of the three modules with a `stream` parameter."""
    import inspect
    found = set()
    for mod in (batch, archive, ralledata):
        for name, fn in inspect.getmembers(mod, inspect.isfunction):
            if fn.__module__ == mod.__name__ and not name.startswith("_") and \
                    "stream" in inspect.signature(fn).parameters:
                found.add(mod.__name__.rsplit(".", 1)[1] + "." + name)
    return found

