"""Times of k2h_amd_ralledata_subkeys and k2h_amd_ralledata_reach.  The stream,
built on the device: --records blobs with 16-byte keys and 16-byte values, then one blob in 16
of them once more under the same key (relaid: the later copy is the key's representative).  One
blob in eight carries a subkeys list of eight 16-byte names of keys of the stream, one name in 16
changed into a name of no key (dangling).  Timed between HIP events, medians of --reps runs after
warm-up with the fastest and the slowest:

  count        subkey_edges(count_only=True): the count pass, its scan and read-back
  edges        subkey_edges(): the count call and the fill call (count pass again, emit, hash, sort,
               resolve)
  reach_1      reach_subkeys from one root;  reach_4096 from 4096 roots (levels and blobs reached
               are reported: the time of a traversal is its levels' synchronisations first)
  diff, times  diff_ralledata of the stream against itself and blob_times of it, in the same
               process, as context: the join resembles _diff's, the walk _times'
  long_list    the count pass over a stream of --long-records blobs, and over the same stream with
               one blob that carries a list of --long-list names: what one lane walking a very long
               list costs

    python tools/ralledata_subkeys_rate.py [--records N] [--reps R] > ralledata_subkeys_rate.json
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

MIX = -7046029254386353131          # 0x9E3779B97F4A7C15 as int64: key i = (i, i * MIX)


def build(torch, ralledata, dev, n, gen, relaid=16, long_list=0):
    """(blobs, blob_off, facts) of the stream described above; long_list: blob 0 carries that
    many names instead of eight."""
    extra = n // relaid if relaid else 0
    kidx = torch.cat([torch.arange(n, device=dev, dtype=torch.int64),
                      torch.randint(0, n, (extra,), device=dev, generator=gen, dtype=torch.int64)])
    tot = kidx.numel()
    kd = torch.stack([kidx, kidx * MIX], 1).contiguous().view(torch.uint8).reshape(-1)
    ko = torch.arange(tot + 1, device=dev, dtype=torch.int64) * 16
    has = (torch.arange(tot, device=dev) % 8) == 0
    nl = int(has.sum().item())

    def lists(rows, names):
        t = torch.randint(0, n, (rows, names), device=dev, generator=gen, dtype=torch.int64)
        hi = t * MIX
        dangle = torch.rand((rows, names), device=dev, generator=gen) < 1.0 / 16
        hi = torch.where(dangle, hi ^ 1, hi)
        w = torch.empty((rows, 1 + 3 * names), device=dev, dtype=torch.int64)
        w[:, 0] = names
        w[:, 1::3], w[:, 2::3], w[:, 3::3] = 16, t, hi
        return w.view(torch.uint8).reshape(-1)
    seg = lists(nl, 8)
    slen = has.to(torch.int64) * 200
    names = 8 * nl
    if long_list:
        first = lists(1, long_list)
        seg = torch.cat([first, seg[200:]])
        slen[0] = first.numel()
        names += long_list - 8
    so = torch.zeros(tot + 1, device=dev, dtype=torch.int64)
    so[1:] = torch.cumsum(slen, 0)
    blobs, off = ralledata.build_ralledata(kd, ko, kd, ko, skeys=seg, skey_off=so)
    return blobs, off, {"blobs": tot, "relaid": extra, "with_list": nl, "names": names, "bytes": int(blobs.numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--long-records", type=int, default=1 << 20)
    ap.add_argument("--long-list", type=int, default=10000)
    a = ap.parse_args()
    import torch

    from k2hash_amd import ralledata, subkeys
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(8642)

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, r

    def timed(fn, reps, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        v = [ev_time(fn)[0] for _ in range(reps)]
        return {"median_s": float(np.median(v)), "min_s": float(np.min(v)), "max_s": float(np.max(v))}

    blobs, off, facts = build(torch, ralledata, dev, a.records, gen)
    n = facts["blobs"]
    edges = subkeys.subkey_edges(blobs, off)
    c = edges.counts
    assert (c.participants, c.with_edges, c.bad, c.edges) == (n, facts["with_list"], 0, facts["names"]), (c, facts)
    assert 0 < c.dangling < c.edges // 8
    rep_is_self = int((edges.rep == torch.arange(n, device=dev)).sum().item())
    assert rep_is_self < n and rep_is_self >= n - 2 * facts["relaid"]
    out = {"workload": f"{a.records} blobs (16-byte keys and values) and {facts['relaid']} of them relaid; one blob in "
                       "eight with a list of eight 16-byte names of keys of the stream, one name in 16 dangling",
           "reps": a.reps, "records": a.records, **facts, "counts": c._asdict()}
    out["count"] = timed(lambda: subkeys.subkey_edges(blobs, off, count_only=True), a.reps)
    out["edges"] = timed(lambda: subkeys.subkey_edges(blobs, off), a.reps)
    roots = torch.arange(0, n, 8, device=dev, dtype=torch.int64)      # blobs with a list
    for label, k in (("reach_1", 1), ("reach_4096", 4096)):
        r = subkeys.reach_subkeys(edges, roots[:k])
        out[label] = dict(timed(lambda: subkeys.reach_subkeys(edges, roots[:k]), a.reps), roots=k, reached=r.reached,
                          levels=r.levels, converged=r.converged)
    d = ralledata.diff_ralledata(blobs, off, blobs, off)
    assert d.participants == d.found == n
    out["diff"] = dict(timed(lambda: ralledata.diff_ralledata(blobs, off, blobs, off), a.reps), na=n, nb=n)
    out["times"] = timed(lambda: ralledata.blob_times(blobs, off), a.reps)
    del blobs, off, edges, d
    torch.cuda.empty_cache()
    long = {}
    for label, k in (("without", 0), ("with", a.long_list)):
        gen.manual_seed(97)
        b, o, f = build(torch, ralledata, dev, a.long_records, gen, relaid=0, long_list=k)
        e = subkeys.subkey_edges(b, o, count_only=True)
        assert e.counts.edges == f["names"] and e.counts.bad == 0, (e.counts, f)
        long[label] = dict(timed(lambda: subkeys.subkey_edges(b, o, count_only=True), a.reps), names=f["names"])
        del b, o, e
    out["long_list"] = dict(long, records=a.long_records, list=a.long_list)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
