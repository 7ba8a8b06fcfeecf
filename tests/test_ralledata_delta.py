"""From two dumps to a log (include/k2hash_amd.h section 4d': k2h_amd_ralledata_delta;
k2h_ralledata_delta.hip) against the model of ralle_delta_model.py, byte for byte and entry for
entry: out, slot_off, made and counts.

That the model's rule is right -- that Load, replaying the log onto the held table, leaves the new
one -- is shown on the CPU against the reviewed transliteration of Load
(archive_fold_model.replay), with rel and seen from ralle_diff_model; libk2hash itself is not
built here, so parity with it is a restatement.  Expected values never come from a device call,
every device output is sentinel-filled and guarded first, and both streams stand at odd shifts
from a 16-byte boundary between canaries.
"""
import ctypes

import numpy as np
import pytest

import archive_apply_model as am
import archive_fold_model as fm
import ralle_archive_model as ra
import ralle_check_model as rm
import ralle_delta_model as dl
import ralle_diff_model as df
from ralle_delta_model import DEL_KEY, REPLACE_ATTRS, REPLACE_SKEY, REPLACE_VAL, SET_ALL
from ralle_unlink_model import layout

from k2hash_amd import _native, archive


@pytest.fixture(scope="module")
def the_grid(oracle):
    """The state grid: 216 present-present cells (6 states of (held, new) per field), 8 held-only
    and 8 new-only, one key per cell, as one pair of streams."""
    cells, held, new, hs = dl.grid(lambda keys: am.hashes_of(oracle, keys))
    return cells, held, new, hs, dl.stream_from(new, hs), dl.stream_from(held, hs)


def _model(a, b, a_consider=None, b_consider=None, **kw):
    d = df.diff_model(a[0], a[1], b[0], b[1], a_consider, b_consider)
    return dl.delta_model(a[0], a[1], d[0], b[0], b[1], b_consider, d[2], **kw), d


# ------------------------------------------------------------------------------------- CPU
def test_state_grid_round_trip(the_grid):
    """Load, replaying the delta onto the held table, leaves the new one; every cell gets one
    record per differing field, one for a new key and one for a key that is gone."""
    cells, held, new, _hs, a, b = the_grid
    (log, slot_off, made, counts), d = _model(a, b)
    assert fm.replay(dl.log_recs(log), dl.table_of(*b)) == dl.table_of(*a) == dl.as_table(new)
    assert dl.table_of(*b) == dl.as_table(held)
    slot = {k: i for i, k in enumerate(new)}
    slot.update({k: len(new) + j for j, k in enumerate(held) if k not in new})
    held_slot = {k: len(new) + j for j, k in enumerate(held)}
    per_type = [0] * 5
    for key, kind, owed in cells:
        g = held_slot[key] if kind == "held-only" else slot[key]
        m = int(made[g])
        assert bin(m).count("1") == owed, (key, kind, m)
        assert m == (DEL_KEY if kind == "held-only" else SET_ALL if kind == "new-only" else m & 14), (key, kind, m)
        for k, bit in enumerate(dl.BITS):
            per_type[k] += bool(m & bit)
    for key in new:                                 # a held blob of a key the new stream has yields nothing
        if key in held:
            assert made[held_slot[key]] == 0
    assert counts[2:7] == per_type and counts[0] == sum(per_type) == sum(c[2] for c in cells) and counts[7] == 0
    assert per_type[0] == 8 and per_type[4] == 8 and per_type[1] == per_type[2] == per_type[3] == 4 * 36
    assert int((made == 14).sum()) == 4 ** 3        # the slots with three records


def test_the_set_all_route_is_told_apart(the_grid):
    """The control: one SET_ALL per changed blob leaves the old subkeys and attrs where they went
    from something to nothing -- ReplaceAll writes them only when the record's own are non-empty."""
    cells, held, new, _hs, a, b = the_grid
    (log, _so, made, counts), _d = _model(a, b, wrong_rule=True)
    assert set(int(x) for x in made) == {0, SET_ALL, DEL_KEY}
    got, want = fm.replay(dl.log_recs(log), dl.table_of(*b)), dl.table_of(*a)
    assert got != want
    wrong = {k for k in want if got.get(k) != want[k]}
    cleared = {k for k in new if k in held and ((held[k][1] and not new[k][1]) or (held[k][2] and not new[k][2]))}
    assert wrong == cleared and len(cleared) == 216 - 5 * 5 * 6


def test_random_tables_round_trip(oracle):
    """200 pairs of streams with duplicates, non-participants and consider masks, each reduced
    to the last copy of every identity as delta_log does: the same round trip."""
    hs_of = lambda keys: am.hashes_of(oracle, keys)  # noqa: E731
    records = refused = dups = 0
    for seed in range(200):
        (a, a_off, ca), (b, b_off, cb) = dl.random_pair(seed, hs_of)
        ra_, rb_ = dl.last_copies(a, a_off, ca), dl.last_copies(b, b_off, cb)
        dups += int((ra_ == 0).sum() + (rb_ == 0).sum())
        (log, _so, made, counts), _d = _model((a, a_off), (b, b_off), ra_, rb_)
        assert fm.replay(dl.log_recs(log), dl.table_of(b, b_off, cb)) == dl.table_of(a, a_off, ca), seed
        assert dl.table_of(a, a_off, ra_) == dl.table_of(a, a_off, ca)
        records += counts[0]
        refused += counts[7]
    assert records > 1000 and dups > 500 and refused > 20   # (unseen held blobs that are no participants)


def test_a_repeated_held_key_needs_the_reduction(oracle):
    """Without the reduction the earlier held copy is not seen and deletes a key the new stream
    still has."""
    key = b"twice-held"
    hs = am.hashes_of(oracle, [key])
    b = rm.join([layout(hs[key], key, b"old", b"", b""), layout(hs[key], key, b"newer", b"s", b"")])
    a = rm.join([layout(hs[key], key, b"newer", b"s", b"")])
    (log, _so, made, _c), _d = _model(a, b)
    assert made.tolist() == [0, DEL_KEY, 0]
    assert fm.replay(dl.log_recs(log), dl.table_of(*b)) == {} != dl.table_of(*a)
    (log, _so, made, _c), _d = _model(a, b, None, dl.last_copies(*b))
    assert made.tolist() == [0, 0, 0] and log == b""


def test_the_host_scan_walks_the_output(the_grid):
    _cells, _held, _new, _hs, a, b = the_grid
    (log, slot_off, made, counts), _d = _model(a, b)
    recs = archive.scan(log)
    assert len(recs) == counts[0] and not recs["status"].any()
    types = [t for m in made for bit, t in dl.TYPE_OF.items() if int(m) & bit]
    assert recs["type"].tolist() == types
    starts = set(int(x) for x in slot_off[:-1][made != 0])
    assert starts <= set(int(x) for x in recs["offset"])


def test_every_einval_without_a_device():
    """Judged on the host before any device is touched: the same answers with and without a
    GPU, each with its own message."""
    lib = _native.batch_lib()
    na, nb = 2, 3
    a, aoff = np.zeros(200, np.uint8), np.arange(na + 1, dtype=np.uint64) * 100
    b, boff = np.zeros(300, np.uint8), np.arange(nb + 1, dtype=np.uint64) * 100
    rel, seen = np.zeros(na, np.uint8), np.ones(nb, np.uint8)
    out, soff = np.full(400, 0xEE, np.uint8), np.full(na + nb + 1, 7, np.uint64)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    counts = (ctypes.c_uint64 * 8)()
    cp = ctypes.cast(counts, ctypes.POINTER(ctypes.c_uint64))
    msg = lambda: bytes(lib.k2h_amd_strerror(_native.K2H_AMD_EINVAL))  # noqa: E731

    def args(**kw):
        d = dict(a=p(a), aoff=p(aoff), na=na, rel=p(rel), b=p(b), boff=p(boff), nb=nb, seen=p(seen), out=p(out),
                 soff=p(soff), counts=cp)
        d.update(kw)
        return (d["a"], a.size, d["aoff"], d["na"], d["rel"], d["b"], b.size, d["boff"], d["nb"], None, d["seen"],
                d["out"], out.size, d["soff"], None, d["counts"], None)
    for i in range(8):
        counts[i] = 7
    nothing = dict(a=None, aoff=None, na=0, rel=None, b=None, boff=None, nb=0, seen=None, out=None, soff=None)
    assert lib.k2h_amd_ralledata_delta(*args(**nothing)) == 0 and list(counts) == [0] * 8
    texts = set()
    cases = ((dict(counts=None), b"NULL counts"), (dict(rel=None), b"NULL rel"), (dict(a=None), b"NULL a_blobs"),
             (dict(aoff=None), b"NULL a_off"), (dict(b=None), b"NULL b_blobs"), (dict(boff=None), b"NULL b_off"),
             (dict(soff=None), b"out given without slot_off"), (dict(na=(1 << 32) - 4), b"2^32 - 2"),
             (dict(nb=(1 << 32) - 3), b"2^32 - 2"), (dict(na=(1 << 64) - 1, nb=2), b"2^32 - 2"))
    for kw, text in cases:
        for i in range(8):
            counts[i] = 7
        assert lib.k2h_amd_ralledata_delta(*args(**kw)) == _native.K2H_AMD_EINVAL, kw
        assert text in msg() and msg().startswith(b"ralledata_delta: "), (kw, msg())
        if "counts" not in kw:
            assert list(counts) == [0] * 8
        texts.add(msg())
    assert len(texts) == 8 and (out == 0xEE).all() and (soff == 7).all()


def test_exports():
    import k2hash_amd
    from k2hash_amd import delta
    for name in ("delta_log", "delta_records", "Delta"):
        assert name in k2hash_amd.__all__ and getattr(k2hash_amd, name) is getattr(delta, name)
    assert delta.Delta._fields == ("log", "slot_off", "made", "counts")
    assert delta.DeltaCounts._fields == ("records", "bytes", "set_all", "replace_val", "replace_skey", "replace_attrs",
                                         "del_key", "refused")
    assert (delta.DELTA_SET_ALL, delta.DELTA_REPLACE_VAL, delta.DELTA_REPLACE_SKEY, delta.DELTA_REPLACE_ATTRS,
            delta.DELTA_DEL_KEY) == dl.BITS
    assert len(_native.SIGNATURES["k2h_amd_ralledata_delta"][1]) == 17


def test_kernels_keep_the_register_budget(tmp_path):
    """Every kernel of k2h_ralledata_delta.hip: at most 64 VGPRs, no scratch, no spills."""
    import subprocess
    from pathlib import Path

    import test_archive_device as tad
    if not Path(tad.HIPCC).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "k2h_ralledata_delta.s"
    subprocess.run([tad.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    f"-I{tad.ROOT / 'include'}", str(tad.CSRC / "k2h_ralledata_delta.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    kernels = {k: v for k, v in tad._kernel_meta(out.read_text()).items() if "delta_" in k}
    for name in ("delta_size_kernel", "delta_compact_kernel", "delta_build_kernel"):
        assert any(name in k for k in kernels), (name, sorted(kernels))
    for sym, f in kernels.items():
        assert f.get("vgpr_count", 999) <= 64, (sym, f.get("vgpr_count"))
        assert f.get("private_segment_fixed_size", 0) == 0, sym
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, sym


# ------------------------------------------------------------------------------------- GPU
def _stream(oracle, n, seed, tag, p_extra=0.4):
    """(keys, elements {key: (V, S, A)}, hashes) of n records with keys of their own."""
    ks, vs, ss, as_ = ra.records(ra._rng(seed), n, p_extra=p_extra)
    ks = [tag + b"%05d" % i + k for i, k in enumerate(ks)]
    return ks, {k: (v, s, a) for k, v, s, a in zip(ks, vs, ss, as_)}, am.hashes_of(oracle, ks)


@pytest.mark.gpu
def test_boundary_sizes(cuda, oracle):
    # na = nb = 0: no device work but slot_off[0] = 0
    rc, out, so, made, counts = dl.run_delta(cuda, b"", [0], [], b"", [0], None, [])
    assert rc == 0 and out == b"" and so.tolist() == [0] and counts == [0] * 8
    ks, el, hs = _stream(oracle, 300, 1, b"held")
    b = dl.stream_from(el, hs)
    # na = 0: every held participant becomes a DEL_KEY
    got, m = dl.against_model(cuda, (b"", [0]), b, "na = 0")
    assert m[3] == [300, m[3][1], 0, 0, 0, 0, 300, 0] and (m[2] == DEL_KEY).all()
    # nb = 0 and seen = NULL: only upserts, B's pointers NULL
    got, m = dl.against_model(cuda, b, None, "nb = 0", seen=None)
    assert m[3][:3] == [300, len(m[0]), 300]
    # ... and seen = NULL with a held stream given: no deletions, the B slots are there and empty
    half = dl.stream_from({k: el[k] for k in ks[:150]}, hs)
    got, m = dl.against_model(cuda, half, b, "seen = NULL, nb > 0", seen=None, pass_b=False)
    assert m[3][0] == 0 and len(m[1]) == 150 + 300 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["in-order", "reversed"])
def test_state_grid(cuda, the_grid, order):
    cells, held, new, hs, a, b = the_grid
    if order == "reversed":
        a, b = dl.stream_from(new, hs, list(new)[::-1]), dl.stream_from(held, hs, list(held)[::-1])
    got, m = dl.against_model(cuda, a, b, f"the grid, {order}")
    assert m[3][0] == sum(c[2] for c in cells) and int((m[2] == 14).sum()) == 4 ** 3
    assert fm.replay(dl.log_recs(m[0]), dl.table_of(*b)) == dl.table_of(*a)


SIZES = (0, 1, 15, 16, 17, 4096, 65536)
KLENS = (1, 15, 16, 17, 100)


@pytest.mark.gpu
def test_field_sizes_and_alignments(cuda, oracle):
    """A carried field of each size in each of the four carrying types, keys of 1 .. 100 bytes,
    the output at each of the 16 alignments."""
    rng = ra._rng(77)
    held, new, n = {}, {}, 0
    for i, sz in enumerate(SIZES):
        d = [ra.rbytes(rng, SIZES[(i + j) % len(SIZES)]) for j in range(3)]      # sz and the two sizes behind it
        for t in range(4):
            key = (b"%02d" % n + b"k" * 100)[:KLENS[n % len(KLENS)]] if KLENS[n % len(KLENS)] > 1 else bytes([0x80 + n])
            n += 1
            if t == 0:
                new[key] = (d[0], d[1], d[2])                                    # SET_ALL: a new key
            else:
                f = t - 1                                                        # REPLACE of field f, sz bytes
                new[key] = tuple(d[0] if x == f else b"same" for x in range(3))
                held[key] = tuple(b"before" if x == f else b"same" for x in range(3))
    assert len(new) == 28 and {len(k) for k in new} == set(KLENS)
    hs = am.hashes_of(oracle, list(new))
    a, b = dl.stream_from(new, hs), dl.stream_from(held, hs)
    for oshift in range(16):
        got, m = dl.against_model(cuda, a, b, f"field sizes, out at {oshift}", oshift=oshift,
                                  ashift=(7 * oshift + 3) % 16, bshift=(3 * oshift + 1) % 16)
    assert m[3][2:7] == [7, 7, 7, 7, 0] and m[3][1] > 6 * 65536
    # every record's own start: all 16 alignments occur over the calls (the first record starts at oshift)
    assert fm.replay(dl.log_recs(m[0]), dl.table_of(*b)) == dl.table_of(*a)


@pytest.mark.gpu
def test_three_records_of_one_slot(cuda, oracle):
    key = b"all-three-fields-change"
    hs = am.hashes_of(oracle, [key])
    for fields in ((b"v" * 5000, b"s" * 33, b""), (b"", b"", b""), (b"v", b"s" * 4096, b"a" * 70000)):
        a = rm.join([layout(hs[key], key, *fields)], lead=b"\x01" * 3)
        b = rm.join([layout(hs[key], key, b"hv", b"hs", b"ha")])
        got, m = dl.against_model(cuda, a, b, "three records")
        assert m[2].tolist() == [14, 0] and m[3][0] == 3
        assert m[0] == fm.scom_record(fm.REPLACE_VAL, key, val=fields[0]) + fm.scom_record(fm.REPLACE_SKEY, key, skey=fields[1]) \
            + fm.scom_record(fm.REPLACE_ATTRS, key, attrs=fields[2])


@pytest.mark.gpu
def test_segment_positions(cuda, oracle):
    """Permuted, gapped and overlapping segments inside A blobs, and the pos of a length-0
    segment pointing outside the blob."""
    k1, k2, k3, k4 = b"forged-one", b"forged-two-with-a-longer-key", b"f3", b"forged-four"
    hs = am.hashes_of(oracle, [k1, k2, k3, k4])
    f1 = ra.forge(k1, b"value-one" * 5, b"subkeys-1", b"attrs-1", order=(3, 1, 0, 2), gaps=(5, 0, 9, 1), slack=13, hashes=hs[k1])
    f2 = ra.forge(k2, b"v2", b"s" * 33, b"a" * 17, order=(2, 3, 1, 0), gaps=(0, 3, 0, 7), slack=1, hashes=hs[k2])
    f3 = ra.forge(k3, b"0123456789abcdefXYZ", hashes=hs[k3], slack=4)
    rm.put(f3, 0, rm.F_SLEN, 7), rm.put(f3, 0, rm.F_SPOS, 80 + len(k3) + 3)     # the subkeys lie inside the value
    rm.put(f3, 0, rm.F_ALEN, 5), rm.put(f3, 0, rm.F_APOS, 80 + len(k3) - 1)     # the attrs across key and value
    f4 = ra.forge(k4, b"only-a-value", hashes=hs[k4])
    rm.put(f4, 0, rm.F_SPOS, 1 << 40), rm.put(f4, 0, rm.F_APOS, (1 << 64) - 8)  # length 0: the pos is ignored
    a = rm.join([f1, f2, f3, f4], lead=b"\x22")
    got, m = dl.against_model(cuda, a, (b"", [0]), "forged, all new", oshift=9)
    assert m[2].tolist() == [SET_ALL] * 4
    assert dl.table_of(*a)[k3] == (b"0123456789abcdefXYZ", b"3456789", b"30123")
    held = {k: (b"held-v", b"held-s", b"held-a") for k in (k1, k2, k3, k4)}
    got, m = dl.against_model(cuda, a, dl.stream_from(held, hs), "forged, all replaced", oshift=2)
    assert m[2].tolist() == [14] * 4 + [0] * 4
    assert fm.replay(dl.log_recs(m[0]), dl.as_table(held)) == dl.table_of(*a)


def _mutants(oracle, tag):
    """Twelve blobs, two each: EMPTY, NO_KEY, BAD_RANGE, consider 0, a span of 79 bytes, and
    sound ones; (blobs, consider)."""
    keys = [tag + b"-mutant-%d" % i * 2 for i in range(12)]
    hs = am.hashes_of(oracle, keys)
    blobs = [bytearray(layout(hs[k], k, b"value-of-" + k, b"", b"AT")) for k in keys]
    cons = np.ones(12, np.uint8)
    for i in (0, 1):
        for f in (rm.F_KLEN, rm.F_VLEN, rm.F_ALEN):
            rm.put(blobs[i], 0, f, 0)
    for i in (2, 3):
        rm.put(blobs[i], 0, rm.F_KLEN, 0)
    for i in (4, 5):
        rm.put(blobs[i], 0, rm.F_VPOS, len(blobs[i]) - 3)
    for i in (6, 7):
        cons[i] = 0
    for i in (8, 9):
        blobs[i] = blobs[i][:79]
    return blobs, cons


@pytest.mark.gpu
def test_refused_slots(cuda, oracle):
    ba, ca = _mutants(oracle, b"new")
    bb, cb = _mutants(oracle, b"held")
    a, b = rm.join(ba, lead=b"\x66" * 3), rm.join(bb)
    # as the diff reports them: nothing of A's mutants; B's are not seen, so each one considered asks for a DEL_KEY
    got, m = dl.against_model(cuda, a, b, "mutants", a_consider=ca, b_consider=cb)
    assert m[2].tolist() == [0] * 10 + [SET_ALL] * 2 + [0] * 10 + [DEL_KEY] * 2
    assert m[3] == [4, len(m[0]), 2, 0, 0, 0, 2, 8]
    # rel bits set on the non-participants: refused, counted
    rel = np.array([df.PART, df.PART | df.FOUND | df.VAL] * 6, np.uint8)
    rel[10] = df.PART | df.FOUND                                        # asks for nothing
    got, m = dl.against_model(cuda, a, b, "forged rel", rel=rel, b_consider=cb)
    assert m[2].tolist() == [0] * 6 + [SET_ALL, REPLACE_VAL] + [0] * 3 + [REPLACE_VAL] + [0] * 10 + [DEL_KEY] * 2
    assert m[3][7] == 8 + 8
    # bad spans in both streams: an end behind the stream, a decreasing pair; seen = 0 on them
    # (behind one sound blob each, which yields its record)
    sa, sb = rm.join(ba[10:], lead=b"\x66"), rm.join(bb[10:])
    bad_a = [1, sa[1][1], sa[1][1] - 10, len(sa[0]) + 1, len(sa[0])]
    bad_b = [0, sb[1][1], sb[1][1] - 10, len(sb[0]) + 1, len(sb[0])]
    got, m = dl.against_model(cuda, (sa[0], bad_a), (sb[0], bad_b), "bad spans", rel=np.full(4, df.PART, np.uint8),
                              seen=np.zeros(4, np.uint8))
    assert m[2].tolist() == [SET_ALL, 0, 0, 0, DEL_KEY, 0, 0, 0] and m[3][7] == 6 and m[3][0] == 2


@pytest.mark.gpu
def test_sparse_and_dense(cuda, oracle):
    """5,000 A blobs of which every 50th changed and 1,000 B blobs of which every 40th is not seen:
    more than one block of the compacted list, a build block with A and B slots, slot blocks that
    emit nothing.  Then every blob changed."""
    ks, el, hs = _stream(oracle, 5000, 5, b"n", p_extra=0.3)
    kb, eb, hb = _stream(oracle, 1000, 6, b"h", p_extra=0.3)
    a, b = dl.stream_from(el, hs), dl.stream_from(eb, hb)
    rel = np.full(5000, df.PART | df.FOUND | df.DATA, np.uint8)
    changed = np.arange(0, 5000, 50)
    rel[changed] = [(df.PART | df.DATA, df.PART | df.FOUND | df.VAL, df.PART | df.FOUND | df.SKEY | df.ATTRS)[i % 3]
                    for i in range(100)]
    seen = np.ones(1000, np.uint8)
    seen[::40] = 0
    got, m = dl.against_model(cuda, a, b, "sparse", rel=rel, seen=seen)
    assert int((m[2] != 0).sum()) == 125 and m[3][0] == 34 + 33 + 2 * 33 + 25 and m[3][7] == 0
    rel[1024:2048] = 0                                                   # as under a consider mask: four slot blocks emit nothing
    got, m = dl.against_model(cuda, a, b, "sparse, a stretch left out", rel=rel, seen=seen)
    assert int((m[2] != 0).sum()) == 125 - 20
    # dense: every blob of A differs from its held blob in the value, every third also in the attrs
    held = {k: (v + b"!", s, a_ + (b"?" if i % 3 == 0 else b"")) for i, (k, (v, s, a_)) in enumerate(list(el.items())[:700])}
    new = {k: el[k] for k in held}
    got, m = dl.against_model(cuda, dl.stream_from(new, hs), dl.stream_from(held, hs), "dense")
    assert m[3][2:7] == [0, 700, 0, 234, 0]


@pytest.mark.gpu
def test_call_shapes(cuda, the_grid):
    _cells, _held, _new, _hs, a, b = the_grid
    got, m = dl.against_model(cuda, a, b, "count only", count_only=True)
    assert got[1] is None and got[2] is None and got[4] == m[3]
    # out_cap one byte short: EINVAL that names both figures; counts and slot_off set, nothing written
    d = df.diff_model(a[0], a[1], b[0], b[1])
    rc, out, so, made, counts = dl.run_delta(cuda, a[0], a[1], d[0], b[0], b[1], None, d[2], cap=m[3][1] - 1)
    assert rc == _native.K2H_AMD_EINVAL and counts == m[3] and (so == m[1]).all() and (made == m[2]).all()
    text = bytes(_native.batch_lib().k2h_amd_strerror(rc))
    assert b"%d" % m[3][1] in text and b"%d" % (m[3][1] - 1) in text
    dl.against_model(cuda, a, b, "made NULL", want_made=False)
    cons = (np.arange(len(b[1]) - 1) % 3 != 0).astype(np.uint8)
    got, mc = dl.against_model(cuda, a, b, "b_consider given", b_consider=cons)
    assert mc[3] != m[3]


def _on_device(cuda, buf, off):
    import torch
    return (torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(cuda) if len(buf) else
            torch.empty(0, dtype=torch.uint8, device=cuda)), torch.tensor([int(x) for x in off], dtype=torch.int64, device=cuda)


@pytest.mark.gpu
def test_round_trip_on_the_device(cuda, oracle, the_grid):
    """delta_log, then apply_log of its log onto the held stream: the result holds the new
    stream's elements.  For the grid, and for a pair of streams with duplicates in both."""
    from k2hash_amd import apply, delta
    _cells, _held, _new, _hs, a, b = the_grid
    rng = np.random.default_rng(4711)
    keys = [b"dup-%03d" % k + b"x" * (k % 9) for k in range(150)]
    hs = am.hashes_of(oracle, keys)

    def copies(n):
        pick = rng.integers(0, 150, n)
        f = lambda nm: b"" if rng.random() < 0.3 else nm + b"%d" % rng.integers(0, 4)  # noqa: E731
        return rm.join([layout(hs[keys[k]], keys[k], f(b"v"), f(b"s"), f(b"a")) for k in pick], lead=b"\x77" * 5)
    pairs = {"the grid": (a, b), "duplicates in both": (copies(400), copies(400))}
    for what, (new, held) in pairs.items():
        d_new, d_held = _on_device(cuda, *new), _on_device(cuda, *held)
        d = delta.delta_log(*d_new, *d_held, want_made=True)
        log = d.log.cpu().numpy().tobytes()
        want = dl.delta_model(new[0], new[1], *_reduced_diff(new, held))
        assert log == want[0] and (d.slot_off.cpu().numpy().view(np.uint64) == want[1]).all(), what
        assert (d.made.cpu().numpy() == want[2]).all() and list(d.counts) == want[3], what
        assert d.counts.records > 100 and d.counts.refused == 0
        recs = archive.recs_to_numpy(archive.scan_device(d.log))
        assert len(recs) == d.counts.records and not (recs["status"] == archive.STATUS_NO_MAGIC).any()
        for fold in (True, False):
            r = apply.apply_log(*d_held, d.log, fold=fold)
            got = dl.table_of(r.blobs.cpu().numpy().tobytes(), r.blob_off.cpu().numpy())
            assert got == dl.table_of(*new), (what, fold)
        # last_copies=False over the same streams is the plain diff's delta
        plain = delta.delta_log(*d_new, *d_held, last_copies=False)
        dm_ = df.diff_model(new[0], new[1], held[0], held[1])
        assert plain.log.cpu().numpy().tobytes() == dl.delta_model(new[0], new[1], dm_[0], held[0], held[1], None, dm_[2])[0]


def _reduced_diff(new, held):
    """(rel, b, b_off, b_consider, seen) of delta_model for the pair under the last-copies masks."""
    ca, cb = dl.last_copies(*new), dl.last_copies(*held)
    d = df.diff_model(new[0], new[1], held[0], held[1], ca, cb)
    return d[0], held[0], held[1], cb, d[2]
