"""Time of k2h_amd_ralledata_partition: bench.ralledata_set's two 8M-record
sets built into blob streams by the producer, used in turn (so the 256 MB Infinity Cache does
not serve them), split three ways: MASK at 16 parts, OWNER at max_hash = 4 / span = 1 and MASK
at 256 parts.  Per configuration, from the same process and on the same stream:

  partition   the whole call into a preallocated `out` (HIP events; it synchronises once inside
              to return the part tables)
  selects     what the library offered for the same split before: P calls of
              k2h_amd_ralledata_select, one per part, their keep masks prepared outside the
              timed region and all writing one preallocated buffer (which favours them)

and once per stream the two yardsticks on this byte mix: one _select that keeps everything (the
1-way rate) and a torch device-to-device clone of the stream (the copy floor).  Medians of
--reps runs after warm-up.  Every blob takes part, so a call moves 2 x stream bytes.

    python tools/ralledata_partition_rate.py [--records N] [--reps R] > ralledata_partition_rate.json

The call's stages (count; scan: the two library scans and the bounds kernel; copy) are kernel
times, so they come from a kernel trace of this same program, taken in a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/ralledata_partition_rate.py --reps R
    python tools/ralledata_partition_rate.py --reps R --stages-from DIR/.../run_kernel_trace.csv

The timed loop calls partition for the three configurations in the order above, so the trace's
last 3 R partition calls are R of each.
"""
import argparse
import csv
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

CONFIGS = (("mask_16", 16, dict(mask=0xF)), ("owner_4", 4, dict(owner=(4, 1))), ("mask_256", 256, dict(mask=0xFF)))
HBM_BYTES_PER_S = 8e12


def fold_stages(path, reps):
    """Per configuration the median time of each stage over the trace's last 3 * reps partition
    calls.  A call runs from a count kernel to the next copy kernel; what lies between them is
    the scan stage."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        name, dur = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
        if "ralledata_part_count_kernel" in name:
            cur = {"count": dur, "scan": 0.0, "copy": 0.0, "scan_kernels": 0}
        elif cur is not None and "ralledata_part_copy_kernel" in name:
            cur["copy"] = dur
            calls.append(cur)
            cur = None
        elif cur is not None:
            cur["scan"] += dur
            cur["scan_kernels"] += 1
    assert len(calls) >= 3 * reps, f"{len(calls)} partition calls in the trace, {3 * reps} wanted"
    calls = calls[-3 * reps:]
    out = {}
    for c, (name, _parts, _rule) in enumerate(CONFIGS):
        mine = calls[c::3]
        med = {k: float(np.median([x[k] for x in mine])) for k in ("count", "scan", "copy")}
        total = sum(med.values())
        out[name] = {"calls": len(mine), "kernels_in_scan": mine[0]["scan_kernels"],
                     **{k + "_s": s for k, s in med.items()}, "kernel_sum_s": total,
                     "largest_stage": max(med, key=med.get), "largest_share_of_kernel_time": max(med.values()) / total}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stages-from", default=None, help="a rocprofv3 kernel trace csv of this program")
    a = ap.parse_args()
    if a.stages_from:
        print(json.dumps({"source": "rocprofv3 --kernel-trace of tools/ralledata_partition_rate.py", "reps": a.reps,
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
    streams = [(blob[:total], boff) for _io, (blob, boff), total in sets]
    del sets
    room = max(int(b.numel()) for b, _o in streams)
    out = torch.empty(room, dtype=torch.uint8, device=dev)        # the one destination every timed call writes
    everything = torch.ones(n, dtype=torch.uint8, device=dev)

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, r

    # the baseline's keep masks, and the check that both ways give the same split
    masks, tables = {}, {}
    for name, parts, rule in CONFIGS:
        for s, (blobs, boff) in enumerate(streams):
            res = ralledata.partition_ralledata(blobs, boff, parts, out=out, want_parts=True, **rule)
            assert res.kept == n and res.kept_bytes == blobs.numel(), (name, s, res.kept, res.kept_bytes)
            masks[name, s] = [(res.part_of == p).to(torch.uint8) for p in range(parts)]
            for p in {0, parts // 2, parts - 1}:
                sel = ralledata.select_ralledata(blobs, boff, masks[name, s][p])
                assert sel.kept == res.part_first[p + 1] - res.part_first[p]
                assert torch.equal(sel.blobs, res.blobs[res.part_byte[p]:res.part_byte[p + 1]]), (name, s, p)
                assert torch.equal(sel.index, res.index[res.part_first[p]:res.part_first[p + 1]]), (name, s, p)
                del sel
            tables[name, s] = (res.part_first, res.part_byte)
            del res
    torch.cuda.synchronize()

    def partition(name, parts, rule, s):
        blobs, boff = streams[s]
        return ralledata.partition_ralledata(blobs, boff, parts, out=out, **rule)

    def selects(name, parts, s):
        blobs, boff = streams[s]
        for keep in masks[name, s]:
            ralledata.select_ralledata(blobs, boff, keep, out=out)

    for i in range(2):  # warm-up: code objects, both calls' scratch at its largest, torch's allocator
        for name, parts, rule in CONFIGS:
            partition(name, parts, rule, i & 1)
            selects(name, parts, i & 1)
        ralledata.select_ralledata(streams[i & 1][0], streams[i & 1][1], everything, out=out)
        streams[i & 1][0].clone()
    torch.cuda.synchronize()
    t = {(name, k): [] for name, _p, _r in CONFIGS for k in ("partition", "selects")}
    t["select_all"], t["clone"] = [], []
    for i in range(a.reps):
        for name, parts, rule in CONFIGS:  # the order fold_stages relies on
            t[name, "partition"].append(ev_time(lambda: partition(name, parts, rule, i & 1))[0])
        for name, parts, rule in CONFIGS:
            t[name, "selects"].append(ev_time(lambda: selects(name, parts, (i + 1) & 1))[0])
        blobs, boff = streams[i & 1]
        t["select_all"].append(ev_time(lambda: ralledata.select_ralledata(blobs, boff, everything, out=out))[0])
        t["clone"].append(ev_time(lambda: blobs.clone())[0])
    torch.cuda.synchronize()
    stream_bytes = [int(b.numel()) for b, _o in streams]
    moved = 2 * float(np.mean(stream_bytes))
    clone, sel_all = float(np.median(t["clone"])), float(np.median(t["select_all"]))
    res = {"workload": f"bench.ralledata_set: 2 sets of {n} records (keys 8-64 B, values 0-256 B) built by "
                       "k2h_amd_build_ralledata, used in turn; every blob takes part",
           "note": "one box, one run", "reps": a.reps, "records": n, "stream_bytes": stream_bytes,
           "bytes_moved_per_call": moved, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S,
           "select_all_s": sel_all, "d2d_clone_s": clone, "select_all_over_clone": sel_all / clone}
    for name, parts, _rule in CONFIGS:
        p, b = float(np.median(t[name, "partition"])), float(np.median(t[name, "selects"]))
        sizes = np.diff(np.array(tables[name, 0][0]))
        res[name] = {"parts": parts, "partition_s": p,
                     "partition_spread_s": [float(np.min(t[name, "partition"])), float(np.max(t[name, "partition"]))],
                     "moved_bytes_per_s": moved / p, "share_of_hbm_rate": moved / p / HBM_BYTES_PER_S,
                     "p_selects_s": b, "partition_over_p_selects": p / b, "partition_over_clone": p / clone,
                     "partition_over_select_all": p / sel_all,
                     "part_blobs_min_max": [int(sizes.min()), int(sizes.max())]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
