"""Time of k2h_amd_ralledata_diff.  S is a bench.ralledata_set stream (keys
8-64 B, values 0-256 B) of --records * 16 / 15 blobs; B, the held stream, is S without a random
blob in 16, so about --records blobs; A, the incoming stream, is S with one value byte changed in
a random quarter of the blobs that have a value.  Two variants: `plain`, blobs without attrs and
no times; `attrs_times`, every blob with the 124 bytes of serialized {expire, mtime, uniqid}
attrs of tools/ralledata_times_rate.py (the changed quarter of A with a later mtime) and times
given.  Per variant: the whole call between HIP events (it synchronises once inside to return
the counts), and from the same run k2h_amd_ralledata_dedup (with times: _dedup_mtime) over A
and B laid end to end, a stream of na + nb blobs: the yardstick for gather + sort.  The bytes
the compare stage must read (both headers and both copies of every equal-length segment of the
matched pairs) are reported for the read floor.  Medians of --reps runs after warm-up, with the
fastest and the slowest.

    python tools/ralledata_diff_rate.py [--records N] [--reps R] > ralledata_diff_rate.json

The call's stages (gather: gather kernel, tile scan, compact kernel; sort: the library's radix
sort; resolve: mark kernel, max-scan, resolve kernel; compare) are kernel times, so they come
from a kernel trace of this same program, taken in a run of its own:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python tools/ralledata_diff_rate.py --reps R
    python tools/ralledata_diff_rate.py --reps R --stages-from DIR/.../run_kernel_trace.csv

The timed loop calls diff on the two variants alternately, so the trace's last 2 R calls are R
of each.
"""
import argparse
import csv
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

VARIANTS = ("plain", "attrs_times")
STAGES = ("gather", "sort", "resolve", "compare")


def fold_stages(path, reps):
    """Per variant the median time of each stage over the trace's last 2 * reps diff calls.  A
    call runs from a diff gather kernel to the next diff compare kernel."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur, stage = [], None, None
    for r in rows:
        name, dur = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
        if "ralledata_diff_gather_kernel" in name:
            cur, stage = dict.fromkeys(STAGES, 0.0), "gather"
        if cur is None:
            continue
        if "ralle_mark_kernel" in name:
            stage = "resolve"
        if "ralledata_diff_compare_kernel" in name:
            cur["compare"] = dur
            calls.append(cur)
            cur = None
            continue
        cur[stage] += dur
        if "ralle_compact_kernel" in name:
            stage = "sort"
    assert len(calls) >= 2 * reps, f"{len(calls)} diff calls in the trace, {2 * reps} wanted"
    calls = calls[-2 * reps:]
    out = {}
    for v, name in enumerate(VARIANTS):
        mine = calls[v::2]
        med = {k: float(np.median([c[k] for c in mine])) for k in STAGES}
        out[name] = {"calls": len(mine), **{k + "_s": s for k, s in med.items()}, "kernel_sum_s": sum(med.values()),
                     "compare_min_max_s": [float(min(c["compare"] for c in mine)), float(max(c["compare"] for c in mine))]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stages-from", default=None, help="a rocprofv3 kernel trace csv of this program")
    a = ap.parse_args()
    if a.stages_from:
        print(json.dumps({"source": "rocprofv3 --kernel-trace of tools/ralledata_diff_rate.py", "reps": a.reps,
                          "stages": fold_stages(a.stages_from, a.reps)}))
        return
    import torch

    import bench
    from k2hash_amd import ralledata
    from ralledata_times_rate import PTS, SEC0, SEC_LATER, attrs_row
    dev = torch.device("cuda", 0)
    n = a.records * 16 // 15
    row, sec_at = attrs_row()
    R = len(row)
    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    (kd, ko, vd, vo), _out, _total = bench.ralledata_set(dev, n, 0)
    del _out
    vlen = vo[1:] - vo[:-1]
    absent = torch.rand(n, device=dev, generator=gen) < 1.0 / 16
    changed = (torch.rand(n, device=dev, generator=gen) < 0.25) & (vlen > 0)
    at8 = torch.arange(8, device=dev)[None, :]

    def field(blobs, boff, byte):
        """The u64 header field at `byte` of every blob."""
        return blobs[(boff[:-1, None] + byte + at8).reshape(-1)].view(torch.int64)

    streams, facts = {}, {}
    for name in VARIANTS:
        if name == "plain":
            s_blobs, s_off = ralledata.build_ralledata(kd, ko, vd, vo)
            alen = 0
        else:
            ad = torch.from_numpy(np.frombuffer(row, np.uint8).copy()).to(dev).repeat(n)
            ao = torch.arange(n + 1, device=dev, dtype=torch.int64) * R
            s_blobs, s_off = ralledata.build_ralledata(kd, ko, vd, vo, attrs=ad, attr_off=ao)
            del ad
            alen = R
        held = ralledata.select_ralledata(s_blobs, s_off, (~absent).to(torch.uint8), want_index=False)
        b_blobs, b_off = held.blobs, held.blob_off
        a_blobs = s_blobs.clone()
        where = (s_off[:-1] + field(s_blobs, s_off, 56))[changed]     # val_pos: the value's first byte
        a_blobs[where] ^= 1
        if alen:   # the changed blobs carry a later mtime (the attrs are each blob's last R bytes)
            tv = s_off[1:][changed] - (R - sec_at)
            secs = torch.full((tv.numel(),), SEC_LATER, device=dev, dtype=torch.int64)
            a_blobs[(tv[:, None] + at8).reshape(-1)] = secs.view(torch.uint8).reshape(-1)
        both = (torch.cat([a_blobs, b_blobs]), torch.cat([s_off, b_off[1:] + s_off[-1]]))
        streams[name] = (a_blobs, s_off, b_blobs, b_off, both)
        found = ~absent
        facts[name] = {
            "na": n, "nb": int(held.kept), "a_bytes": int(a_blobs.numel()), "b_bytes": int(b_blobs.numel()),
            "expect_found": int(found.sum().item()), "expect_changed": int((changed & found).sum().item()),
            # both headers and both copies of the value (and attrs) of every matched pair
            "compare_read_bytes": int((found * (2 * (vlen + alen) + 160)).sum().item()),
        }
        del s_blobs, held
    del kd, vd
    torch.cuda.synchronize()
    now = (SEC0 + 100, 0)

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, r

    def diff(name):
        ab, ao, bb, bo, _both = streams[name]
        t = dict(pts=PTS, now=now) if name == "attrs_times" else {}
        return ralledata.diff_ralledata(ab, ao, bb, bo, **t)

    def dedup(name):
        both = streams[name][4]
        return ralledata.dedup_ralledata(*both, pts=PTS if name == "attrs_times" else None)

    for _ in range(3):  # warm-up: code objects, the calls' scratch at its largest, torch's allocator
        for name in VARIANTS:
            d = diff(name)
            f = facts[name]
            assert (d.participants, d.found) == (f["na"], f["expect_found"]), (d[3:7], f)
            changed_bits = ralledata.DIFF_VAL | (ralledata.DIFF_ATTRS if name == "attrs_times" else 0)
            assert d.found - d.same == f["expect_changed"], (d[3:7], f)
            assert int(((d.rel & 0x1c) == changed_bits).sum().item()) == f["expect_changed"]
            f["apply"] = d.apply
            f["feed"] = None if d.feed is None else int(d.feed.sum().item())
            f["dedup_superseded"] = dedup(name)[2]
            del d
    torch.cuda.synchronize()
    t = {(name, k): [] for name in VARIANTS for k in ("diff", "dedup")}
    for _ in range(a.reps):
        for name in VARIANTS:
            t[name, "diff"].append(ev_time(lambda: diff(name))[0])
    for _ in range(a.reps):
        for name in VARIANTS:
            t[name, "dedup"].append(ev_time(lambda: dedup(name))[0])
    torch.cuda.synchronize()
    out = {"workload": f"bench.ralledata_set: S of {n} records (keys 8-64 B, values 0-256 B); B = S without a random "
                       "blob in 16, A = S with one value byte changed in a random quarter; attrs_times: 124 attrs bytes "
                       "(expire, mtime, uniqid) per blob, the changed quarter of A with a later mtime, times given",
           "reps": a.reps, "records": a.records}
    for name in VARIANTS:
        out[name] = dict(facts[name])
        for k in ("diff", "dedup"):
            v = t[name, k]
            m = float(np.median(v))
            out[name][k] = {"median_s": m, "min_s": float(np.min(v)), "max_s": float(np.max(v)),
                            "blobs_per_s": (facts[name]["na"] + facts[name]["nb"]) / m}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
