"""Time of k2h_amd_ralledata_archive: bench.ralledata_set's two 8M-record sets
built into blob streams by the producer (the streams of tools/ralledata_partition_rate.py), used
in turn (so the 256 MB Infinity Cache does not serve them), every blob written as a SET_ALL
record.  From the same process and on the same stream, HIP events around

  archive      the whole call into a preallocated `out` (sizing kernel, scan, one synchronise
               inside to return the counts, build kernel)
  sizes_only   the same call with out = NULL: what of it is not the build
  select_all   k2h_amd_ralledata_select with every blob kept, into the same `out`: the closest
               existing copy of the same payload (whole blobs, 80-byte headers included)
  clone        a torch device-to-device clone of the stream (the copy floor)
  archive_half the writer with a keep mask that drops a random half of the blobs (nearly every
               block then has blobs that take no part between two that do)

Medians of --reps runs after warm-up.  Bytes: _select reads and writes the stream; the writer
reads the stream, reads the 80-byte headers once more in the sizing pass, and writes the stream
plus 24 bytes per record (a 104-byte header where the blob had 80).

    python tools/ralledata_archive_rate.py [--records N] [--reps R] > ralledata_archive_rate.json

Before timing, the output of each stream is scanned on the device and turned back into blobs
(archive.scan_device, archive_to_ralledata): they must equal the stream.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 8e12
SCOM, HEADER = 104, 80


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch

    import bench
    from k2hash_amd import archive, ralledata
    dev = torch.device("cuda", 0)
    n = a.records
    sets = [bench.ralledata_set(dev, n, s) for s in range(2)]
    for (kd, ko, vd, vo), (blob, boff), total in sets:
        ralledata.build_ralledata(kd, ko, vd, vo, out=blob, blob_off=boff, total=total)
    torch.cuda.synchronize()
    streams = [(blob[:total], boff) for _io, (blob, boff), total in sets]
    del sets
    stream_bytes = [int(b.numel()) for b, _o in streams]
    room = max(stream_bytes) + (SCOM - HEADER) * n
    out = torch.empty(room, dtype=torch.uint8, device=dev)        # the one destination every timed call writes
    everything = torch.ones(n, dtype=torch.uint8, device=dev)
    half = (torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(15)) < 0.5).to(torch.uint8)

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, r

    for s, (blobs, boff) in enumerate(streams):     # the round trip gives the stream back
        res = ralledata.ralledata_to_archive(blobs, boff, out=out)
        assert res.records == n and res.total == stream_bytes[s] + (SCOM - HEADER) * n, (s, res.records, res.total)
        recs = archive.scan_device(res.bytes)
        back, back_off = ralledata.archive_to_ralledata(res.bytes, recs)
        assert recs.shape[0] == n and torch.equal(back_off, boff) and torch.equal(back, blobs), s
        del res, recs, back, back_off
    torch.cuda.synchronize()

    calls = {
        "archive": lambda b, o: ralledata.ralledata_to_archive(b, o, out=out),
        "sizes_only": lambda b, o: ralledata.ralledata_to_archive(b, o, count_only=True),
        "select_all": lambda b, o: ralledata.select_ralledata(b, o, everything, out=out),
        "clone": lambda b, o: b.clone(),
        "archive_half": lambda b, o: ralledata.ralledata_to_archive(b, o, keep=half, out=out),
    }
    for i in range(2):  # warm-up: code objects, select's scratch, torch's allocator
        for fn in calls.values():
            fn(*streams[i & 1])
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for i in range(a.reps):
        for j, (k, fn) in enumerate(calls.items()):
            blobs, boff = streams[(i + j) & 1]
            t[k].append(ev_time(lambda: fn(blobs, boff))[0])
    torch.cuda.synchronize()
    med = {k: float(np.median(v)) for k, v in t.items()}
    s_mean = float(np.mean(stream_bytes))
    payload = s_mean / n - HEADER
    moved_archive = 2 * s_mean + (SCOM - HEADER) * n + HEADER * n     # read, write, the sizing pass's headers
    moved_select = 2 * s_mean
    res = {"workload": f"bench.ralledata_set: 2 sets of {n} records (keys 8-64 B, values 0-256 B) built by "
                       "k2h_amd_build_ralledata, used in turn; every blob takes part",
           "note": "one box, one run", "reps": a.reps, "records": n, "stream_bytes": stream_bytes,
           "mean_payload_bytes_per_blob": payload, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S,
           "archive_s": med["archive"], "archive_spread_s": [float(np.min(t["archive"])), float(np.max(t["archive"]))],
           "sizes_only_s": med["sizes_only"], "build_by_difference_s": med["archive"] - med["sizes_only"],
           "select_all_s": med["select_all"],
           "select_all_spread_s": [float(np.min(t["select_all"])), float(np.max(t["select_all"]))],
           "d2d_clone_s": med["clone"], "archive_half_kept_s": med["archive_half"],
           "archive_bytes_moved": moved_archive, "select_all_bytes_moved": moved_select,
           "byte_ratio": moved_archive / moved_select,
           "byte_ratio_write_side_only": (SCOM + payload) / (HEADER + payload),
           "time_ratio": med["archive"] / med["select_all"],
           "time_ratio_over_byte_ratio": med["archive"] / med["select_all"] / (moved_archive / moved_select),
           "archive_moved_bytes_per_s": moved_archive / med["archive"],
           "archive_share_of_hbm_rate": moved_archive / med["archive"] / HBM_BYTES_PER_S,
           "select_all_moved_bytes_per_s": moved_select / med["select_all"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
