"""Times of k2h_amd_ralledata_unlink over the stream of ralledata_subkeys_rate.py:
--records blobs with 16-byte keys and values, one in 16 relaid, one blob in eight with a list of
eight 16-byte names, one name in 16 dangling.  Every call writes into a buffer allocated before
(one native call each), timed between HIP events: medians of --reps runs after warm-up, with the
fastest and the slowest.

  select        select_ralledata with everything kept: existing code, the copy floor
  count         subkey_edges(count_only=True): the _subkeys count pass, which walks the same lists
  no_mask       unlink with drop NULL: select's rule by this call's kernels
  no_drop       unlink with an all-zero drop mask: every list is walked and verified, none rewritten
  one_percent   one name dropped in 1 % of the lists
  dangling      every dangling name dropped (drop_mask(edges, dangling=True))

    python tools/ralledata_unlink_rate.py [--records N] [--reps R] > ralledata_unlink_rate.json
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

from ralledata_subkeys_rate import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=10)
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
    E = edges.counts.edges
    assert E == facts["names"] and edges.counts.bad == 0
    out_buf = torch.empty(blobs.numel(), dtype=torch.uint8, device=dev)
    everything = torch.ones(n, dtype=torch.uint8, device=dev)
    res = {"workload": f"{a.records} blobs (16-byte keys and values) and {facts['relaid']} of them relaid; one blob in eight "
                       "with a list of eight 16-byte names of keys of the stream, one name in 16 dangling",
           "reps": a.reps, "records": a.records, **facts, "edges": E, "dangling_names": edges.counts.dangling}

    sel = ralledata.select_ralledata(blobs, off, everything, out=out_buf)
    assert sel.kept == n and sel.kept_bytes == blobs.numel() and torch.equal(sel.blobs, blobs)
    res["select"] = timed(lambda: ralledata.select_ralledata(blobs, off, everything, out=out_buf), a.reps)
    res["count"] = timed(lambda: subkeys.subkey_edges(blobs, off, count_only=True), a.reps)

    with_list = torch.nonzero(edges.flags & subkeys.SKEY_HAS).reshape(-1)
    some = with_list[torch.randperm(with_list.numel(), device=dev, generator=gen)[:max(with_list.numel() // 100, 1)]]
    one = torch.zeros(E, dtype=torch.uint8, device=dev)
    one[edges.edge_off[some] + torch.randint(0, 8, (some.numel(),), device=dev, generator=gen)] = 1
    cases = (("no_mask", None), ("no_drop", torch.zeros(E, dtype=torch.uint8, device=dev)), ("one_percent", one),
             ("dangling", subkeys.drop_mask(edges, dangling=True)))
    for label, drop in cases:
        out_buf.fill_(0xC3)
        u = subkeys.unlink_subkeys(blobs, off, edges, drop, out=out_buf)
        c = u.counts
        assert c.emitted == n and c.mismatches == 0, c
        if label in ("no_mask", "no_drop"):
            assert c.rewritten == 0 and torch.equal(u.blobs, blobs)
        elif label == "one_percent":
            assert c.rewritten == c.dropped == some.numel() and c.emitted_bytes == blobs.numel() - 24 * some.numel()
        else:
            assert c.dropped == edges.counts.dangling and c.emitted_bytes == blobs.numel() - 24 * c.dropped - 8 * c.emptied
            again = subkeys.subkey_edges(u.blobs, u.blob_off, count_only=False)
            assert again.counts.dangling == 0 and again.counts.bad == 0 and again.counts.edges == E - c.dropped
            del again
        res[label] = dict(timed(lambda: subkeys.unlink_subkeys(blobs, off, edges, drop, out=out_buf), a.reps), counts=c._asdict())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
