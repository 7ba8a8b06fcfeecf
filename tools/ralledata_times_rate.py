"""Time of k2h_amd_ralledata_times and k2h_amd_ralledata_dedup_mtime: bench's two
8 Mi-record sets (keys 8-64 B, values 0-256 B) built into blob streams by the producer, every blob
with the 124 bytes of serialized {expire, mtime, uniqid} attrs a table with the builtin mtime and
expire attributes gives its elements, composed with torch ops; a random quarter of each stream's
blobs is laid down a second time behind it with a later mtime, so that under the mtime rule every
first copy is superseded.  The two streams are used in turn (so the 256 MB Infinity Cache does
not serve them).  Timed, whole calls between HIP events, the median of --reps runs after warm-up
with the fastest and the slowest: blob_times with a window, dedup_mtime (it synchronises once
inside to return the count), and for scale k2h_amd_ralledata_check and k2h_amd_ralledata_dedup
over the same stream.

    python tools/ralledata_times_rate.py [--records N] [--reps R] > ralledata_times_rate.json
"""
import argparse
import json
import struct
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

SEC0, SEC_LATER, PTS = 1_700_000_000, 1_700_010_000, (1_800_000_000, 0)
UNIQ = b"0123456789abcde\0"


def attrs_row():
    """One blob's attrs as K2HAttrs::Serialize writes them (keys sorted): returns the bytes and
    the offset of the mtime's tv_sec in them."""
    ent = lambda k, v: struct.pack("<QQ", len(k), len(v)) + k + v  # noqa: E731
    head = struct.pack("<Q", 3) + ent(b"expire\0", struct.pack("<qq", SEC0 + 3600, 0))
    row = head + ent(b"mtime\0", struct.pack("<qq", SEC0, 0)) + ent(b"uniqid\0", UNIQ)
    return row, len(head) + 16 + 6


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
    row, sec_at = attrs_row()
    R = len(row)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)

    def set_sec(blobs, boff, first, secs):
        """tv_sec of the mtime of blobs first .. first + len(secs): the attrs are each blob's last R bytes."""
        at = boff[first + 1:first + 1 + secs.numel()] - (R - sec_at)
        idx = at[:, None] + torch.arange(8, device=dev)[None, :]
        blobs[idx.reshape(-1)] = secs.view(torch.uint8).reshape(-1)

    streams, expect = [], []
    for s in range(2):
        (kd, ko, vd, vo), _out, _total = bench.ralledata_set(dev, n, s)
        del _out
        ad = torch.from_numpy(np.frombuffer(row, np.uint8).copy()).to(dev).repeat(n)
        ao = torch.arange(n + 1, device=dev, dtype=torch.int64) * R
        blobs, boff = ralledata.build_ralledata(kd, ko, vd, vo, attrs=ad, attr_off=ao)
        del kd, vd, ad
        set_sec(blobs, boff, 0, SEC0 + (torch.arange(n, device=dev, dtype=torch.int64) & 1023))
        again = (torch.rand(n, device=dev, generator=gen) < 0.25).to(torch.uint8)
        sel = ralledata.select_ralledata(blobs, boff, again, want_index=False)
        blobs, boff = torch.cat([blobs, sel.blobs]), torch.cat([boff, sel.blob_off[1:] + boff[-1]])
        set_sec(blobs, boff, n, torch.full((sel.kept,), SEC_LATER, device=dev, dtype=torch.int64))
        streams.append((blobs, boff))
        expect.append(sel.kept)
        del sel
    torch.cuda.synchronize()
    window = ralledata.TimeWindow(start=(SEC0 + 512, 0), end=(SEC_LATER, 0), now=(SEC0 + 100, 0))

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, r

    calls = {
        "blob_times": lambda b, o: ralledata.blob_times(b, o, window=window),
        "dedup_mtime": lambda b, o: ralledata.dedup_ralledata(b, o, pts=PTS),
        "check": lambda b, o: ralledata.check_ralledata(b, o),
        "dedup": lambda b, o: ralledata.dedup_ralledata(b, o),
    }
    facts = {}
    for i in range(4):  # warm-up: code objects, the calls' scratch at its largest, torch's allocator
        blobs, boff = streams[i & 1]
        res = {k: fn(blobs, boff) for k, fn in calls.items()}
        facts[i & 1] = {"superseded_mtime_rule": res["dedup_mtime"][2], "superseded_plain_rule": res["dedup"][2],
                        "kept_by_window": int(res["blob_times"].keep.sum().item()),
                        "with_mtime": int((res["blob_times"].flags & 1).ne(0).sum().item())}
        del res
    torch.cuda.synchronize()
    # the plain streams may hold equal keys of their own (none are expected at these key lengths)
    for s in range(2):
        assert facts[s]["superseded_mtime_rule"] >= expect[s], (facts, expect)
        assert facts[s]["superseded_plain_rule"] == 0, facts
        assert facts[s]["with_mtime"] == streams[s][1].numel() - 1
    t = {k: [] for k in calls}
    for i in range(a.reps):
        for k, fn in calls.items():
            blobs, boff = streams[(i + (k in ("check", "dedup"))) & 1]
            t[k].append(ev_time(lambda: fn(blobs, boff))[0])
    torch.cuda.synchronize()
    blobs_n = max(int(o.numel()) - 1 for _b, o in streams)
    out = {"workload": f"bench.ralledata_set: 2 sets of {n} records (keys 8-64 B, values 0-256 B), {R} attrs bytes "
                       "(expire, mtime, uniqid) per blob, a random quarter of each stream's blobs copied behind it "
                       "with a later mtime; the two streams used in turn", "reps": a.reps, "records": n,
           "blobs": blobs_n, "stream_bytes": max(int(b.numel()) for b, _o in streams), "relaid": expect,
           "facts": [facts[0], facts[1]]}
    for k, v in t.items():
        m = float(np.median(v))
        out[k] = {"median_s": m, "min_s": float(np.min(v)), "max_s": float(np.max(v)), "blobs_per_s": blobs_n / m}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
