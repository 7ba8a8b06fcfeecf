"""Time of k2h_amd_archive_fold: a transaction log of --records records composed
on the device with torch ops -- 24-byte keys, 16 bytes of data, 144 bytes per record (128 for a
DEL_KEY); roughly 70 % SET_ALL, 15 % REPLACE_VAL, 10 % DEL_KEY, 2.5 % each REPLACE_SKEY and
REPLACE_ATTRS; a quarter of the records rewrite the key of an earlier record.  Two logs are used
in turn (so the 256 MB Infinity Cache does not serve them).  Timed, whole calls between HIP
events and by the host's clock, the median of --reps runs after warm-up with the fastest and the
slowest: the fold with h1 passed in, with h1 computed, without the count; the scan + prehash that
feeds it; compact_device; and, as the yardstick, k2h_amd_ralledata_dedup on a blob stream of the
same number of blobs, a quarter of them copies of earlier ones.  Then the hot-key case: one chain
of --chain records of a single key (a REPLACE_SKEY, then REPLACE_VALs) against an ordinary log of
the same size.  The number of cover rounds is computed here, on the device, by the same doubling
over (`by`, W) with torch ops.

    python tools/archive_fold_rate.py [--records N] [--chain N] [--reps R] [--lib PATH] > archive_fold_rate.json

--lib: time another build of the library (for the resident-waves comparison: the link and cover
kernels built with -DK2H_FOLD_LINK_LDS=0 / -DK2H_FOLD_COVER_LDS=65536).  Per-kernel times come
from a run of this tool with --stage-trace under `rocprofv3 --kernel-trace --stats`, in a process
of its own.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402

KEY, DATA, SCOM = 24, 16, 104
SET_ALL, REPLACE_VAL, REPLACE_SKEY, DEL_KEY, OW_VAL, REPLACE_ATTRS, RENAME = range(7)
COMMANDS = {SET_ALL: b"\nK2H_SET_ALL", REPLACE_VAL: b"\nK2H_REP_VAL", REPLACE_SKEY: b"\nK2H_REP_SKEY",
            DEL_KEY: b"\nK2H_DEL_KEY", REPLACE_ATTRS: b"\nK2H_REP_ATTRS"}
MIX = ((SET_ALL, 0.70), (REPLACE_VAL, 0.15), (DEL_KEY, 0.10), (REPLACE_SKEY, 0.025), (REPLACE_ATTRS, 0.025))
W = {SET_ALL: 1, REPLACE_VAL: 1, REPLACE_SKEY: 2, DEL_KEY: 7, REPLACE_ATTRS: 4}


def header_table():
    """(7, 13) int64: the SCOM header of each type the logs use, as K2HCommandArchive::Put lays it
    out (lib/k2hcommand.cc:69-201): the one data segment right behind the key, every position the
    type does not use at 104."""
    t = np.zeros((7, 13), np.int64)
    data = SCOM + KEY
    for typ, cmd in COMMANDS.items():
        lens, pos = [KEY, 0, 0, 0, 0], [SCOM] * 5
        seg = {SET_ALL: 1, REPLACE_VAL: 1, REPLACE_SKEY: 2, REPLACE_ATTRS: 3}.get(typ)
        if seg:
            lens[seg], pos[seg] = DATA, data
        if typ == SET_ALL:
            pos[2] = pos[3] = data + DATA
        t[typ, :2] = np.frombuffer(cmd.ljust(16, b"\0"), "<i8")
        t[typ, 2] = typ
        t[typ, 3:8], t[typ, 8:13] = lens, pos
    return t


def make_log(torch, dev, n, seed, chain=False):
    """(file bytes, types, key ids) on the device."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    i = torch.arange(n, device=dev, dtype=torch.int64)
    if chain:
        typ = torch.full((n,), REPLACE_VAL, device=dev, dtype=torch.int64)
        typ[0] = REPLACE_SKEY
        kid = torch.zeros(n, device=dev, dtype=torch.int64)
    else:
        u = torch.rand(n, device=dev, generator=gen)
        typ, acc = torch.full((n,), SET_ALL, device=dev, dtype=torch.int64), 0.0
        for t, p in MIX:
            typ = torch.where((u >= acc) & (u < acc + p), torch.full_like(typ, t), typ)
            acc += p
        rewrite = torch.rand(n, device=dev, generator=gen) < 0.25
        earlier = (torch.rand(n, device=dev, generator=gen, dtype=torch.float64) * i).to(torch.int64)
        kid = torch.where(rewrite & (i > 0), earlier, i)
        for _ in range(5):      # a rewrite of a rewrite is a rewrite of that one's key: kid[i] <= i, doubled
            kid = kid[kid]
    rows = torch.empty((n, 18), dtype=torch.int64, device=dev)
    rows[:, :13] = torch.from_numpy(header_table()).to(dev)[typ]
    rows[:, 13] = kid * -7046029254386353131 + seed   # (wraps: the low bytes of a key differ from its neighbours')
    rows[:, 14] = kid
    rows[:, 15] = 0x6B2D79656B2D7965
    rows[:, 16] = i
    rows[:, 17] = ~i
    words = torch.where(typ == DEL_KEY, 16, 18)
    mask = torch.arange(18, device=dev)[None, :] < words[:, None]
    return rows[mask].view(torch.uint8), typ, kid


def rounds_of(torch, by, typ):
    """The cover rounds the fold needs for these `by` and types (no barriers, one seg), by the
    same doubling with torch ops: how often U |= U[nxt], nxt = nxt[nxt] runs until every record
    either has W inside U or no nxt."""
    w = torch.tensor([W.get(t, 0) for t in range(7)], device=by.device)[typ]
    n = by.numel()
    nxt = torch.where(by < 0, torch.full_like(by, n), by)        # n: none
    wpad = torch.cat([w, w.new_zeros(1)])
    u = wpad[nxt]
    rounds = 0
    while bool(((nxt < n) & ((w & ~u) != 0)).any()):
        upad, npad = torch.cat([u, u.new_zeros(1)]), torch.cat([nxt, nxt.new_full((1,), n)])
        u, nxt = u | upad[nxt], npad[nxt]
        rounds += 1
    return rounds, int((((w & ~u) == 0) & (w != 0)).sum().item())


def self_check(torch, dev):
    """A small log of this generator against the host scan and the tests' model."""
    import archive_fold_model as fm
    from k2hash_amd import archive
    file, typ, kid = make_log(torch, dev, 4096, 5)
    data = file.cpu().numpy().tobytes()
    recs = archive.scan(data)
    assert recs.size == 4096 and not recs["status"].any() and (recs["type"] == typ.cpu().numpy()).all()
    want = fm.fold_model(fm.recs_of(data, recs))
    f = archive.fold_device(file, want_by=True)
    torch.cuda.synchronize()
    assert (f.keep.cpu().numpy() == want[0]).all() and f.dropped == want[2]
    assert (f.by.cpu().numpy().view(np.uint64) == want[1]).all()
    assert rounds_of(torch, f.by, typ)[1] == want[2]
    return {"records": 4096, "dropped": int(want[2])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--chain", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--stage-trace", action="store_true",
                    help="for a run under rocprofv3: only folds of the big logs (h1 passed and computed), so "
                         "that every kernel's average is over launches of one size")
    a = ap.parse_args()
    from k2hash_amd import _native
    if a.lib:
        _native.BATCH_LIB = Path(a.lib).resolve()
    import torch

    import bench
    from k2hash_amd import archive, ralledata
    dev = torch.device("cuda", 0)
    n = a.records
    out = {"lib": str(_native.BATCH_LIB.relative_to(ROOT)) if _native.BATCH_LIB.is_relative_to(ROOT) else a.lib,
           "reps": a.reps, "records": n, "self_check": None if a.stage_trace else self_check(torch, dev)}

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0, r

    def summarise(ts, count):
        ev, wall = [t[0] for t in ts], [t[1] for t in ts]
        m = float(np.median(ev))
        return {"median_s": m, "min_s": float(np.min(ev)), "max_s": float(np.max(ev)),
                "host_clock_median_s": float(np.median(wall)), "records_per_s": count / m}

    def time_logs(logs, calls, reps):
        prepared = []
        for file in logs:
            recs, h1 = archive.scan_prehash_device(file)[:2]
            prepared.append((file, recs.contiguous(), h1.contiguous()))
        for i in range(4):
            for fn in calls.values():
                fn(*prepared[i % len(prepared)])
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for i in range(reps):
            for j, (k, fn) in enumerate(calls.items()):
                args = prepared[(i + j) % len(prepared)]
                t[k].append(ev_time(lambda: fn(*args))[:2])
        return {k: summarise(v, prepared[0][1].shape[0]) for k, v in t.items()}, prepared

    calls = {
        "fold_h1_passed": lambda f, r, h: archive.fold_device(f, r, h),
        "fold_h1_computed": lambda f, r, h: archive.fold_device(f, r),
        "fold_h1_passed_no_count": lambda f, r, h: archive.fold_device(f, r, h, count=False),
        "scan_prehash": lambda f, r, h: archive.scan_prehash_device(f),
        "compact_device": lambda f, r, h: archive.compact_device(f),
    }
    if a.stage_trace:
        calls = {k: calls[k] for k in ("fold_h1_passed", "fold_h1_computed")}
    logs, facts = [], []
    for s in range(2):
        file, typ, kid = make_log(torch, dev, n, 100 + s)
        f = archive.fold_device(file, want_by=True)
        f2 = archive.fold_device(file, f.recs, None)
        assert f.recs.shape[0] == n and torch.equal(f.keep, f2.keep) and f.dropped == f2.dropped
        rounds, covered = rounds_of(torch, f.by, typ)
        assert covered == f.dropped == n - int(f.keep.sum().item())
        facts.append({"file_bytes": int(file.numel()), "dropped": f.dropped, "cover_rounds": rounds,
                      "synchronisations_with_count": 1 + rounds + 1, "synchronisations_without_count": 1 + rounds,
                      "records_with_a_later_one_of_their_key": int((f.by >= 0).sum().item()),
                      "types": {str(t): int((typ == t).sum().item()) for t in range(7)}})
        logs.append(file)
        del f, f2, typ, kid
    out["workload"] = (f"2 logs of {n} records composed on the device: {KEY}-byte keys, {DATA} data bytes, 144 bytes "
                       "per record (DEL_KEY 128); 70 % SET_ALL, 15 % REPLACE_VAL, 10 % DEL_KEY, 2.5 % REPLACE_SKEY, "
                       "2.5 % REPLACE_ATTRS; a quarter of the records rewrite an earlier record's key; used in turn")
    out["logs"] = facts
    timed, _prep = time_logs(logs, calls, a.reps)
    out.update(timed)
    del logs, _prep
    torch.cuda.empty_cache()
    if a.stage_trace:
        print(json.dumps(out))
        return

    if not a.no_yardstick:
        streams = []
        for s in range(2):
            m = n * 3 // 4
            (kd, ko, vd, vo), _o, _t = bench.ralledata_set(dev, m, s)
            del _o
            blobs, boff = ralledata.build_ralledata(kd, ko, vd, vo)
            del kd, vd
            again = torch.zeros(m, dtype=torch.uint8, device=dev)
            again[torch.randperm(m, device=dev)[:n - m]] = 1
            sel = ralledata.select_ralledata(blobs, boff, again, want_index=False)
            streams.append((torch.cat([blobs, sel.blobs]), torch.cat([boff, sel.blob_off[1:] + boff[-1]])))
            del sel, blobs, boff
        for i in range(4):
            keep, _by, dropped = ralledata.dedup_ralledata(*streams[i & 1])
        assert dropped >= n - n * 3 // 4 and streams[0][1].numel() - 1 == n
        ts = [ev_time(lambda: ralledata.dedup_ralledata(*streams[i & 1]))[:2] for i in range(a.reps)]
        out["yardstick_ralledata_dedup"] = dict(summarise(ts, n), blobs=n, superseded=int(dropped),
                                                stream_bytes=int(streams[0][0].numel()))
        del streams
        torch.cuda.empty_cache()

    # the hot key: one chain against an ordinary log of the same size
    c = a.chain
    chain_file = make_log(torch, dev, c, 7, chain=True)[0]
    plain_file, ptyp, _k = make_log(torch, dev, c, 8)
    fc = archive.fold_device(chain_file, want_by=True)
    assert fc.dropped == c - 2 and int(fc.keep[0].item()) == 1 and int(fc.keep[-1].item()) == 1
    ctyp = torch.full((c,), REPLACE_VAL, device=dev, dtype=torch.int64)
    ctyp[0] = REPLACE_SKEY
    fp = archive.fold_device(plain_file, want_by=True)
    hot = {"records": c, "chain_cover_rounds": rounds_of(torch, fc.by, ctyp)[0],
           "ordinary_cover_rounds": rounds_of(torch, fp.by, ptyp)[0]}
    one = {"fold": lambda f, r, h: archive.fold_device(f, r, h)}
    hot["chain"] = time_logs([chain_file], one, a.reps)[0]["fold"]
    hot["ordinary"] = time_logs([plain_file], one, a.reps)[0]["fold"]
    out["hot_key"] = hot
    print(json.dumps(out))


if __name__ == "__main__":
    main()
