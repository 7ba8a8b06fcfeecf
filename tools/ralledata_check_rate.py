"""Rate of the RALLEDATA consumer side: bench.ralledata_set's two 8M-record
sets built into blob streams by the producer, then, over the streams in turn (so the 256 MB
Infinity Cache does not serve them): k2h_amd_ralledata_check alone, check + route
(target_max_hash = 2), k2h_amd_ralledata_select with the routed half kept, the producer's own
kernel over the same records, and a torch device-to-device clone of the stream as the memory
yardstick.  Medians of --reps runs after warm-up, HIP events around each call (select
synchronises once inside; its time includes that).

    python tools/ralledata_check_rate.py [--records N] [--reps R] > ralledata_check_rate.json
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second, the MI355X's specification


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch

    import bench
    from k2hash_amd import ralledata
    dev = torch.device("cuda", 0)
    n = a.records
    sets = [bench.ralledata_set(dev, n, s) for s in range(2)]

    def produce(i):
        (kd, ko, vd, vo), (blob, boff), total = sets[i & 1]
        ralledata.build_ralledata(kd, ko, vd, vo, out=blob, blob_off=boff, total=total)

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, r

    for i in range(2):
        produce(i)
    torch.cuda.synchronize()
    streams = [(blob[:total], boff) for _io, (blob, boff), total in sets]
    rng = ralledata.make_hash_range(0, 2)
    keeps, outs = [], []
    for blobs, boff in streams:
        res = ralledata.check_ralledata(blobs, boff, rng, want_hashes=True)
        assert not res.status.any().item(), "the producer's stream does not check OK"
        keeps.append(((res.status == ralledata.OK) & ((res.route & 1) != 0)).to(torch.uint8))
        outs.append(torch.empty_like(blobs))
    for i in range(3):  # warm-up: code objects, the select's scratch, torch's allocator
        blobs, boff = streams[i & 1]
        ralledata.check_ralledata(blobs, boff)
        ralledata.check_ralledata(blobs, boff, rng)
        sel = ralledata.select_ralledata(blobs, boff, keeps[i & 1], out=outs[i & 1])
        blobs.clone()
        produce(i)
    torch.cuda.synchronize()
    t = {k: [] for k in ("check", "check_route", "select", "clone", "producer")}
    for i in range(a.reps):
        blobs, boff = streams[i & 1]
        t["check"].append(ev_time(lambda: ralledata.check_ralledata(blobs, boff))[0])
        blobs, boff = streams[(i + 1) & 1]
        t["check_route"].append(ev_time(lambda: ralledata.check_ralledata(blobs, boff, rng))[0])
        blobs, boff = streams[i & 1]
        s, sel = ev_time(lambda: ralledata.select_ralledata(blobs, boff, keeps[i & 1], out=outs[i & 1]))
        t["select"].append(s)
        blobs, boff = streams[(i + 1) & 1]
        t["clone"].append(ev_time(lambda: blobs.clone())[0])
        t["producer"].append(ev_time(lambda: produce(i))[0])
    torch.cuda.synchronize()
    med = {k: float(np.median(v)) for k, v in t.items()}
    size = max(int(b.numel()) for b, _o in streams)
    read = size + 8 * (n + 1)            # the check reads the stream and its offsets
    wrote = n                            # and writes a status byte per blob (+ a route byte)
    kept_bytes, kept = sel.kept_bytes, sel.kept
    sel_moved = 9 * n + 8 + 2 * kept_bytes + 16 * kept + 8  # keep + offsets, the kept bytes in and out, out_off + index
    prod_moved = max(bench.ralledata_algo_bytes(io) for io, _o, _t in sets)

    def rate(nbytes, s):
        return {"s": s, "GB_per_s": nbytes / s / 1e9, "fraction_of_8TBps": nbytes / s / HBM_PEAK}
    print(json.dumps({
        "workload": f"bench.ralledata_set: 2 sets of {n} records (keys 8-64 B, values 0-256 B) built by "
                    f"k2h_amd_build_ralledata, {size} stream bytes, used in turn",
        "reps": a.reps, "records": n, "stream_bytes": size,
        "check": {"bytes_read": read, "bytes_written": wrote, **rate(read + wrote, med["check"]),
                  "records_per_s": n / med["check"]},
        "check_route": {"bytes_read": read, "bytes_written": 2 * wrote, **rate(read + 2 * wrote, med["check_route"]),
                        "records_per_s": n / med["check_route"]},
        "select_half": {"kept": kept, "kept_bytes": kept_bytes, "bytes_moved": sel_moved,
                        **rate(sel_moved, med["select"])},
        "d2d_clone": {"bytes_moved": 2 * size, **rate(2 * size, med["clone"])},
        "producer": {"bytes_moved": prod_moved, **rate(prod_moved, med["producer"])},
        "check_over_producer_time": med["check"] / med["producer"],
    }))


if __name__ == "__main__":
    main()
