"""Time of k2h_amd_ralledata_dedup: bench.ralledata_set's two 8M-record sets
built into blob streams by the producer, used in turn (so the 256 MB Infinity Cache does not
serve them), once as built -- no duplicates -- and once with a random quarter of each
stream's blobs laid down a second time behind it, so that about a fifth of the longer stream
is superseded.  Per variant: the whole call (HIP events; it synchronises once inside to
return the count), and from the same run two yardsticks: k2h_amd_ralledata_check over the
same stream and a torch device-to-device clone of it.  Medians of --reps runs after warm-up.

    python tools/ralledata_dedup_rate.py [--records N] [--reps R] > ralledata_dedup_rate.json

The call's three stages (gather: the gather kernel, the tile scan and the compact kernel;
sort: the library's radix sort; resolve) are kernel times, so they come from a kernel trace of
this same program, taken in a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/ralledata_dedup_rate.py --reps R
    python tools/ralledata_dedup_rate.py --reps R --stages-from DIR/.../run_kernel_trace.csv

The timed loop calls dedup on the plain and the doubled stream alternately, nothing else
between a call's first and last kernel, so the trace's last 2 R calls are R of each.
"""
import argparse
import csv
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

VARIANTS = ("no_duplicates", "quarter_relaid")


def fold_stages(path, reps):
    """Per variant the median time of each stage over the trace's last 2 * reps dedup calls.
    A call runs from a gather kernel to the next resolve kernel; what lies up to and including
    the compact kernel is the gather stage, what lies between compact and resolve the sort."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur, stage = [], None, None
    for r in rows:
        name, dur = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
        if "ralledata_dedup_gather_kernel" in name:
            cur, stage = {"gather": 0.0, "sort": 0.0, "resolve": 0.0, "sort_kernels": 0}, "gather"
        if cur is None:
            continue
        if "ralledata_dedup_resolve_kernel" in name:
            cur["resolve"] = dur
            calls.append(cur)
            cur = None
            continue
        cur[stage] += dur
        cur["sort_kernels"] += stage == "sort"
        if "ralle_compact_kernel" in name:
            stage = "sort"
    assert len(calls) >= 2 * reps, f"{len(calls)} dedup calls in the trace, {2 * reps} wanted"
    calls = calls[-2 * reps:]
    out = {}
    for v, name in enumerate(VARIANTS):
        mine = calls[v::2]
        med = {k: float(np.median([c[k] for c in mine])) for k in ("gather", "sort", "resolve")}
        total = sum(med.values())
        out[name] = {"calls": len(mine), "kernels_in_sort": mine[0]["sort_kernels"],
                     **{k + "_s": s for k, s in med.items()}, "kernel_sum_s": total,
                     "sort_share_of_kernel_time": med["sort"] / total}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stages-from", default=None, help="a rocprofv3 kernel trace csv of this program")
    a = ap.parse_args()
    if a.stages_from:
        print(json.dumps({"source": "rocprofv3 --kernel-trace of tools/ralledata_dedup_rate.py", "reps": a.reps,
                          "stages": fold_stages(a.stages_from, a.reps)}))
        return
    import torch

    import bench
    from k2hash_amd import ralledata
    dev = torch.device("cuda", 0)
    n = a.records
    sets = [bench.ralledata_set(dev, n, s) for s in range(2)]
    for (kd, ko, vd, vo), (blob, boff), total in sets:
        ralledata.build_ralledata(kd, ko, vd, vo, out=blob, blob_off=boff, total=total)
    torch.cuda.synchronize()
    plain = [(blob[:total], boff) for _io, (blob, boff), total in sets]
    del sets
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    doubled, expect = [], []
    for blobs, boff in plain:  # a random quarter of the blobs again, behind the stream
        again = (torch.rand(n, device=dev, generator=gen) < 0.25).to(torch.uint8)
        sel = ralledata.select_ralledata(blobs, boff, again, want_index=False)
        doubled.append((torch.cat([blobs, sel.blobs]), torch.cat([boff, sel.blob_off[1:] + boff[-1]])))
        expect.append(sel.kept)
        del sel
    streams = {VARIANTS[0]: plain, VARIANTS[1]: doubled}

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, r

    dropped = {}
    for i in range(4):  # warm-up: code objects, the call's scratch at its largest, torch's allocator
        for name in VARIANTS:
            blobs, boff = streams[name][i & 1]
            keep, _by, d = ralledata.dedup_ralledata(blobs, boff)
            dropped[name, i & 1] = d
            ralledata.check_ralledata(blobs, boff)
            blobs.clone()
    torch.cuda.synchronize()
    # the plain streams may hold equal keys of their own (none are expected at these key lengths)
    own = [dropped[VARIANTS[0], s] for s in range(2)]
    assert [dropped[VARIANTS[1], s] for s in range(2)] == [own[s] + expect[s] for s in range(2)], (dropped, expect)
    t = {(name, k): [] for name in VARIANTS for k in ("dedup", "check", "clone")}
    for i in range(a.reps):
        for name in VARIANTS:  # the order fold_stages relies on
            blobs, boff = streams[name][i & 1]
            t[name, "dedup"].append(ev_time(lambda: ralledata.dedup_ralledata(blobs, boff))[0])
        for name in VARIANTS:
            blobs, boff = streams[name][(i + 1) & 1]
            t[name, "check"].append(ev_time(lambda: ralledata.check_ralledata(blobs, boff))[0])
            blobs, boff = streams[name][i & 1]
            t[name, "clone"].append(ev_time(lambda: blobs.clone())[0])
    torch.cuda.synchronize()
    out = {"workload": f"bench.ralledata_set: 2 sets of {n} records (keys 8-64 B, values 0-256 B) built by "
                       "k2h_amd_build_ralledata, used in turn; quarter_relaid: a random quarter of each stream's "
                       "blobs copied behind it", "reps": a.reps, "records": n}
    for name in VARIANTS:
        m = {k: float(np.median(t[name, k])) for k in ("dedup", "check", "clone")}
        blobs_n = max(int(o.numel()) - 1 for _b, o in streams[name])
        out[name] = {"blobs": blobs_n, "stream_bytes": max(int(b.numel()) for b, _o in streams[name]),
                     "superseded": [dropped[name, s] for s in range(2)],
                     "dedup_s": m["dedup"], "dedup_blobs_per_s": blobs_n / m["dedup"],
                     "dedup_spread_s": [float(np.min(t[name, "dedup"])), float(np.max(t[name, "dedup"]))],
                     "check_s": m["check"], "d2d_clone_s": m["clone"],
                     "dedup_over_check": m["dedup"] / m["check"], "dedup_over_clone": m["dedup"] / m["clone"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
