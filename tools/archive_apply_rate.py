"""Time of k2h_amd_archive_apply.  The held stream: --records blobs built from
bench.ralledata_set (keys 8-64 B, values 0-256 B).  The log: --records records of the mix
tools/archive_fold_rate.py measures (70 % SET_ALL, 15 % REPLACE_VAL, 10 % DEL_KEY, 2.5 % each
REPLACE_SKEY and REPLACE_ATTRS, 16 data bytes); three quarters of its keys are drawn from the held
stream, the others are fresh 24-byte keys, and a quarter of the records rewrite the key of an
earlier record.  The file has no record headers: the call reads nothing of a record but the
ranges in recs, so a record's key range points at the held stream's own key bytes, which the file
carries in front.  Timed, whole native calls between HIP events and by the host's clock, the
median of --reps runs after warm-up with the fastest and the slowest: the apply filling a buffer
given to it (one native call), with the fold's keep as its consider mask and without; the count-only
call; and as yardsticks in the same run k2h_amd_ralledata_diff of two streams of the same sizes,
k2h_amd_archive_fold on the log, and k2h_amd_ralledata_select of the held stream with everything
kept -- the copy floor.  The apply is reported as a multiple of diff + select, which between them
do the same join and the same copying.

    python tools/archive_apply_rate.py [--records N] [--reps R] [--lib PATH] > archive_apply_rate.json

--lib: time another build of the library (for the resident-waves comparison: the plan kernel
built with -DK2H_APPLY_PLAN_LDS=65536).  Per-kernel times come from a run of this tool with
--stage-trace under `rocprofv3 --kernel-trace --stats`, in a process of its own.
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

FRESH, DATA = 24, 16
SET_ALL, REPLACE_VAL, REPLACE_SKEY, DEL_KEY, OW_VAL, REPLACE_ATTRS, RENAME = range(7)
MIX = ((SET_ALL, 0.70), (REPLACE_VAL, 0.15), (DEL_KEY, 0.10), (REPLACE_SKEY, 0.025), (REPLACE_ATTRS, 0.025))


def make_log(torch, dev, kd, ko, n, seed):
    """(file, recs): the held stream's key bytes kd, n fresh keys and n data rows; recs (n, 13)."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    na = ko.numel() - 1
    i = torch.arange(n, device=dev, dtype=torch.int64)
    u = torch.rand(n, device=dev, generator=gen)
    typ, acc = torch.full((n,), SET_ALL, device=dev, dtype=torch.int64), 0.0
    for t, p in MIX:
        typ = torch.where((u >= acc) & (u < acc + p), torch.full_like(typ, t), typ)
        acc += p
    rewrite = torch.rand(n, device=dev, generator=gen) < 0.25
    earlier = (torch.rand(n, device=dev, generator=gen, dtype=torch.float64) * i).to(torch.int64)
    kid = torch.where(rewrite & (i > 0), earlier, i)
    for _ in range(5):      # a rewrite of a rewrite is a rewrite of that one's key
        kid = kid[kid]
    from_held = (torch.rand(n, device=dev, generator=gen) < 0.75)[kid]
    hidx = torch.randint(0, na, (n,), device=dev, generator=gen)[kid]
    fresh = torch.empty((n, 3), dtype=torch.int64, device=dev)
    fresh[:, 0] = i * -7046029254386353131 + seed
    fresh[:, 1] = i
    fresh[:, 2] = 0x6B2D79656B2D7965
    data = torch.stack([i, ~i], 1)
    f0 = (kd.numel() + 15) // 16 * 16
    file = torch.cat([kd, kd.new_zeros(f0 - kd.numel()), fresh.view(torch.uint8).view(-1), data.view(torch.uint8).view(-1)])
    d0 = f0 + FRESH * n
    recs = torch.zeros((n, 13), dtype=torch.int64, device=dev)
    recs[:, 0] = typ
    recs[:, 1] = d0 + DATA * i
    recs[:, 2] = torch.where(from_held, ko[hidx], f0 + FRESH * kid)
    recs[:, 3] = torch.where(from_held, ko[hidx + 1] - ko[hidx], torch.full_like(i, FRESH))
    for col, types in ((4, (SET_ALL, REPLACE_VAL)), (6, (REPLACE_SKEY,)), (8, (REPLACE_ATTRS,))):
        on = torch.zeros(n, dtype=torch.bool, device=dev)
        for t in types:
            on |= typ == t
        recs[:, col] = d0 + DATA * i
        recs[:, col + 1] = torch.where(on, DATA, 0)
    recs[:, 10] = d0
    return file, recs, typ


def self_check(torch, dev):
    """A small stream and log of this generator against the tests' model, byte for byte."""
    import archive_apply_model as am
    import archive_fold_model as fm
    import bench
    from k2hash_amd import apply, archive, ralledata
    na = n = 3000
    (kd, ko, vd, vo), _o, _t = bench.ralledata_set(dev, na, 0)
    blobs, boff = ralledata.build_ralledata(kd, ko, vd, vo)
    file, recs, _typ = make_log(torch, dev, kd, ko, n, 5)
    h1, h2 = archive.prehash_device(file, recs)
    a = apply.apply_records(blobs, boff, file, recs, h1, h2)
    torch.cuda.synchronize()
    host = archive.recs_to_numpy(recs)
    m = am.apply_model(blobs.cpu().numpy().tobytes(), boff.cpu().numpy(), None, fm.recs_of(file.cpu().numpy().tobytes(), host),
                       None, h1.cpu().numpy().view(np.uint64), h2.cpu().numpy().view(np.uint64))
    assert list(a.counts) == m.counts and a.blobs.cpu().numpy().tobytes() == m.out
    assert (a.touched.cpu().numpy() == m.touched).all() and (a.origin.cpu().numpy() == m.origin.view(np.int64)).all()
    return {"blobs": na, "records": n, "counts": m.counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--stage-trace", action="store_true",
                    help="for a run under rocprofv3: only the apply without a mask, so that every kernel's "
                         "average is over launches of one size")
    a = ap.parse_args()
    from k2hash_amd import _native
    if a.lib:
        _native.BATCH_LIB = Path(a.lib).resolve()
    import torch

    import bench
    from k2hash_amd import apply, archive, ralledata
    dev = torch.device("cuda", 0)
    n = na = a.records
    out = {"lib": str(_native.BATCH_LIB.relative_to(ROOT)) if _native.BATCH_LIB.is_relative_to(ROOT) else a.lib,
           "reps": a.reps, "records": n, "held_blobs": na, "self_check": None if a.stage_trace else self_check(torch, dev)}

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0, r

    def summarise(ts):
        ev, wall = [t[0] for t in ts], [t[1] for t in ts]
        return {"median_s": float(np.median(ev)), "min_s": float(np.min(ev)), "max_s": float(np.max(ev)),
                "host_clock_median_s": float(np.median(wall))}

    (kd, ko, vd, vo), _o, _t = bench.ralledata_set(dev, na, 0)
    del _o
    held, hoff = ralledata.build_ralledata(kd, ko, vd, vo)
    del vd, vo
    file, recs, typ = make_log(torch, dev, kd, ko, n, 100)
    h1, h2 = archive.prehash_device(file, recs)
    keep = archive.fold_device(file, recs, h1, count=False).keep
    first = apply.apply_records(held, hoff, file, recs, h1, h2, count_only=True)
    folded = apply.apply_records(held, hoff, file, recs, h1, h2, consider=keep, count_only=True)
    assert first.stop == n and tuple(first.counts)[:6] == tuple(folded.counts)[:6]
    buf = torch.empty(first.counts.emitted_bytes, dtype=torch.uint8, device=dev)
    out["workload"] = {"held_bytes": int(held.numel()), "file_bytes": int(file.numel()),
                       "types": {str(t): int((typ == t).sum().item()) for t in range(7)},
                       "counts": first.counts._asdict(), "applied_with_folds_keep": folded.counts.applied,
                       "records_dropped_by_fold": n - int(keep.sum().item())}
    calls = {
        "apply": lambda: apply.apply_records(held, hoff, file, recs, h1, h2, out=buf),
        "apply_with_folds_keep": lambda: apply.apply_records(held, hoff, file, recs, h1, h2, consider=keep, out=buf),
        "apply_count_only": lambda: apply.apply_records(held, hoff, file, recs, h1, h2, count_only=True),
        "apply_hashes_computed": lambda: apply.apply_records(held, hoff, file, recs, out=buf),
    }
    if a.stage_trace:
        calls = {"apply": calls["apply"]}
    else:
        (kd2, ko2, vd2, vo2), _o, _t = bench.ralledata_set(dev, n, 1)
        del _o
        inc, ioff = ralledata.build_ralledata(kd2, ko2, vd2, vo2)
        del kd2, vd2, ko2, vo2
        ones = torch.ones(na, dtype=torch.uint8, device=dev)
        sel = torch.empty(held.numel(), dtype=torch.uint8, device=dev)
        calls.update({
            "yardstick_diff": lambda: ralledata.diff_ralledata(inc, ioff, held, hoff),
            "yardstick_fold": lambda: archive.fold_device(file, recs, h1),
            "yardstick_select_all": lambda: ralledata.select_ralledata(held, hoff, ones, out=sel),
        })
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, fn in calls.items():
            ts[k].append(ev_time(fn)[:2])
    out.update({k: summarise(v) for k, v in ts.items()})
    if not a.stage_trace:
        floor = out["yardstick_diff"]["median_s"] + out["yardstick_select_all"]["median_s"]
        out["diff_plus_select_s"] = floor
        out["apply_over_diff_plus_select"] = out["apply"]["median_s"] / floor
        out["apply_with_folds_keep_over_diff_plus_select"] = out["apply_with_folds_keep"]["median_s"] / floor
    print(json.dumps(out))


if __name__ == "__main__":
    main()
