"""Rate of the device-resident archive prehash: an archive of N records drawn
from tests/golden/archive.k2har, resident in HBM -> k2h_amd_archive_scan_prehash_device (and
its scan and prehash halves), against the only route the host entries offer for the same
device-resident bytes: a D2H copy, archive.scan (k2h_archive.cc) and archive.prehash.

Two copies of the file are kept in HBM and the timed calls alternate between them, so the
256 MB Infinity Cache does not serve the file.  Medians of --reps runs after warm-up; HIP
events where the call is asynchronous, a wall clock around the calls that synchronise.

    python tools/archive_rate.py [--records N] [--reps R] > archive_rate.json
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from k2hash_amd import archive  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second, the MI355X's specification


def replicate(n: int, seed: int, with_pick: bool = False):
    """n records drawn from the golden file's 64, appended as K2HArchive::Save appends; with_pick:
    also which golden record each one is."""
    f = np.frombuffer((ROOT / "tests" / "golden" / "archive.k2har").read_bytes(), np.uint8)
    recs = archive.scan(f)
    start = recs["offset"].astype(np.int64)
    length = np.diff(np.concatenate([start, [f.size]]))
    pick = np.random.default_rng(seed).integers(0, recs.size, n)
    out = np.empty(int(length[pick].sum()), np.uint8)
    at = 0
    for lo in range(0, n, 1 << 19):  # in pieces: the gather index is 8 bytes per file byte
        p = pick[lo:lo + (1 << 19)]
        lens = length[p]
        rel = np.concatenate([[0], np.cumsum(lens)])
        # byte i of the piece comes from start[p[r]] + (i - rel[r]) for its record r
        src = np.repeat(start[p] - rel[:-1], lens) + np.arange(int(rel[-1]), dtype=np.int64)
        out[at:at + src.size] = f[src]
        at += src.size
    return (out, pick) if with_pick else out


def median(xs):
    return float(np.median(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-only", action="store_true", help="build the file and time the host scan only (no GPU)")
    a = ap.parse_args()
    n = a.records
    data = replicate(n, seed=7)
    size = int(data.size)
    if a.host_only:
        t0 = time.perf_counter()
        host = archive.scan(data)
        print(json.dumps({"records": int(host.size), "bytes": size, "host_scan_s": time.perf_counter() - t0}))
        return
    import torch
    dev = torch.device("cuda", 0)
    files = [torch.from_numpy(data).to(dev), torch.from_numpy(data).to(dev)]
    torch.cuda.synchronize()

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, r

    for i in range(3):  # warm-up: code objects, the scan's scratch, torch's allocator
        recs, h1, h2 = archive.scan_prehash_device(files[i & 1])
        archive.prehash_device(files[i & 1], archive.scan_device(files[i & 1]))
        files[0].clone()
    torch.cuda.synchronize()
    fused, scan, pre, copy = [], [], [], []
    for i in range(a.reps):
        f = files[i & 1]
        t0 = time.perf_counter()
        recs, h1, h2 = archive.scan_prehash_device(f)  # synchronises (the record count)
        torch.cuda.synchronize()
        fused.append(time.perf_counter() - t0)
        f = files[(i + 1) & 1]
        t0 = time.perf_counter()
        r = archive.scan_device(f)
        scan.append(time.perf_counter() - t0)
        pre.append(ev_time(lambda: archive.prehash_device(f, r))[0])
        copy.append(ev_time(lambda: files[i & 1].clone())[0])
    assert recs.shape[0] == n

    # the host route, from the same device-resident bytes
    d2h, hscan, hpre = [], [], []
    for i in range(a.host_reps):
        t0 = time.perf_counter()
        back = files[i & 1].cpu().numpy()
        t1 = time.perf_counter()
        host = archive.scan(back)
        t2 = time.perf_counter()
        g1, g2 = archive.prehash(back, host)
        t3 = time.perf_counter()
        d2h.append(t1 - t0), hscan.append(t2 - t1), hpre.append(t3 - t2)
    # the two routes give the same records and hashes
    got = archive.recs_to_numpy(recs)
    same = all(np.array_equal(got[k], host[k]) for k in archive.REC_DTYPE.names)
    same = same and np.array_equal(h1.cpu().numpy().view(np.uint64), g1) and \
        np.array_equal(h2.cpu().numpy().view(np.uint64), g2)
    assert same, "device and host routes differ"

    dev_s = median(fused)
    host_s = median(d2h) + median(hscan) + median(hpre)
    copy_s = median(copy)
    print(json.dumps({
        "workload": f"{n} archive records drawn from tests/golden/archive.k2har (seed 7), {size} bytes, "
                    "two copies in HBM used in turn",
        "reps": a.reps, "host_reps": a.host_reps, "outputs_equal": bool(same),
        "device": {"scan_prehash_s": dev_s, "scan_s": median(scan), "prehash_s": median(pre),
                   "records_per_s": n / dev_s, "file_GB_per_s": size / dev_s / 1e9,
                   "fraction_of_8TBps": size / dev_s / HBM_PEAK},
        "host_route": {"d2h_s": median(d2h), "scan_s": median(hscan), "prehash_s": median(hpre), "total_s": host_s,
                       "records_per_s": n / host_s, "scan_threads": 1},
        "device_over_host_route": host_s / dev_s,
        "d2d_copy": {"s": copy_s, "file_GB_per_s": size / copy_s / 1e9},
    }))


if __name__ == "__main__":
    main()
