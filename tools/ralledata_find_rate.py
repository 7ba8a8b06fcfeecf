"""Times of k2h_amd_ralledata_index, _find and _fetch: bench.ralledata_set's two
8M-record sets built into blob streams by the producer, used in turn (so the 256 MB Infinity
Cache does not serve them).  HIP events around whole calls, medians of --reps runs after
warm-up, each figure next to its yardstick from the same run:

  index   the whole call, next to k2h_amd_ralledata_dedup over the same stream (the same gather,
          compact and sort, and a resolve on top);
  find    m = 1,000 / 65,536 / --records keys of the stream in random order plus as many misses
          (the same keys with their first byte changed), hashes computed and hashes passed,
          against the index of the whole stream, and at m = 1,000 also against the index of the
          stream's first 65,536 blobs; next to k2h_amd_ralledata_diff without times at na = m
          (the m blobs themselves), nb = n, the one-shot join a lookup replaces;
  fetch   the values of all the stream's keys, in the random order of the lookup and in stream
          order (the library's fill call alone, and the wrapper's count + fill), next to
          k2h_amd_ralledata_select keeping about as many bytes and a torch device-to-device
          clone of as many bytes.

    python tools/ralledata_find_rate.py [--records N] [--reps R] > profiles/ralledata_find_rate.json
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

SMALL = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch

    import bench
    from k2hash_amd import batch, find, ralledata
    dev = torch.device("cuda", 0)
    n = a.records
    sets = [bench.ralledata_set(dev, n, s) for s in range(2)]
    for (kd, ko, vd, vo), (blob, boff), total in sets:
        ralledata.build_ralledata(kd, ko, vd, vo, out=blob, blob_off=boff, total=total)
    torch.cuda.synchronize()
    streams = [(blob[:total], boff) for _io, (blob, boff), total in sets]
    del sets
    small = [(b[:int(o[min(SMALL, n)].item())], o[:min(SMALL, n) + 1].contiguous()) for b, o in streams]
    gen = torch.Generator(device=dev)
    gen.manual_seed(2718)

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, r

    def med(v):
        return {"median_s": float(np.median(v)), "min_s": float(np.min(v)), "max_s": float(np.max(v))}

    out = {"workload": f"bench.ralledata_set: 2 sets of {n} records (keys 8-64 B, values 0-256 B) built by "
                       "k2h_amd_build_ralledata, used in turn", "reps": a.reps, "records": n,
           "index_bytes": find.index_size(n)}

    # ---- index, next to dedup
    t = {"index": [], "dedup": []}
    for i in range(a.reps + 2):
        blobs, boff = streams[i & 1]
        ti, ix = ev_time(lambda: find.index_stream(blobs, boff))
        assert ix.participants == n
        td, d = ev_time(lambda: ralledata.dedup_ralledata(blobs, boff))
        if i >= 2:
            t["index"].append(ti)
            t["dedup"].append(td)
        del ix, d
    out["index"] = {k: med(v) for k, v in t.items()}

    # ---- find, next to diff
    index = [find.index_stream(b, o) for b, o in streams]
    index_small = [find.index_stream(b, o) for b, o in small]

    def queries(s, held_n, m):
        """m keys of stream s's first held_n blobs in random order and as many misses."""
        blobs, boff = streams[s]
        pick = torch.randperm(held_n, device=dev, generator=gen)[:m].contiguous()
        qd, qo, _bad = find.fetch_segments(blobs, boff, pick, "key")
        miss = qd.clone()
        miss[qo[:-1]] ^= 0x80
        keys, koff = torch.cat([qd, miss]), torch.cat([qo, qo[1:] + qo[-1]])
        h1, h2 = batch.hash_csr(keys, koff, second=True)
        mask = torch.zeros(held_n, dtype=torch.uint8, device=dev)
        mask[pick] = 1
        return pick, keys, koff, h1, h2, mask

    out["find"] = {}
    for label, held, idx, held_n, ms in (("index_of_all", streams, index, n, sorted({min(1000, n), min(SMALL, n), n})),
                                         ("index_of_65536", small, index_small, min(SMALL, n), [min(1000, n)])):
        for m in ms:
            q = [queries(s, held_n, m) for s in range(2)]
            t = {"find_hashes_computed": [], "find_hashes_passed": [], "diff_na_m": []}
            for i in range(a.reps + 2):
                s = i & 1
                (blobs, boff), (pick, keys, koff, h1, h2, mask) = held[s], q[s]
                tc, f = ev_time(lambda: find.find_keys(blobs, boff, idx[s], keys, koff))
                assert tuple(f.counts) == (2 * m, m, 0) and bool((f.match[:m] == pick).all())
                tp, f = ev_time(lambda: find.find_keys(blobs, boff, idx[s], keys, koff, h1=h1, h2=h2))
                assert tuple(f.counts) == (2 * m, m, 0)
                inc = ralledata.select_ralledata(blobs, boff, mask, want_index=False)
                td, d = ev_time(lambda: ralledata.diff_ralledata(inc.blobs, inc.blob_off, blobs, boff))
                assert d.found == m
                if i >= 2:
                    t["find_hashes_computed"].append(tc)
                    t["find_hashes_passed"].append(tp)
                    t["diff_na_m"].append(td)
                del f, d, inc
            out["find"][f"{label}/m={m}+{m}"] = {k: med(v) for k, v in t.items()}
            del q
    del index_small

    # ---- fetch, next to select and a clone
    lib_fill = {}
    t = {"fetch_random_fill": [], "fetch_random_wrapper": [], "fetch_stream_order_fill": [],
         "fetch_stream_order_wrapper": [], "select_as_many_bytes": [], "clone_as_many_bytes": []}
    facts = []
    for s in range(2):
        blobs, boff = streams[s]
        order = torch.randperm(n, device=dev, generator=gen)
        qd, qo, _bad = find.fetch_segments(blobs, boff, order, "key")
        f = find.find_keys(blobs, boff, index[s], qd, qo)
        assert f.counts.found == n and bool((f.match == order).all())
        vals, voff, _bad = find.fetch_segments(blobs, boff, f.match, "value")
        keep = (torch.rand(n, device=dev, generator=gen) < vals.numel() / blobs.numel()).to(torch.uint8)
        lib_fill[s] = (f.match, torch.arange(n, device=dev, dtype=torch.int64), torch.empty_like(vals),
                       torch.empty(n + 1, dtype=torch.int64, device=dev), keep)
        facts.append({"value_bytes": int(vals.numel()), "stream_bytes": int(blobs.numel())})
        del qd, qo, f, vals, voff
    import ctypes

    from k2hash_amd import _native
    lib = _native.batch_lib()

    def fill(s, which):
        blobs, boff = streams[s]
        buf, ooff = lib_fill[s][2], lib_fill[s][3]
        total = ctypes.c_uint64(0)
        _native.check(lib.k2h_amd_ralledata_fetch(blobs.data_ptr(), blobs.numel(), boff.data_ptr(), n, which.data_ptr(), n,
                                                  None, _native.K2H_AMD_SEG_VAL, buf.data_ptr(), buf.numel(),
                                                  ooff.data_ptr(), None, ctypes.byref(total),
                                                  torch.cuda.current_stream().cuda_stream))
        assert total.value == buf.numel()

    for i in range(a.reps + 2):
        s = i & 1
        blobs, boff = streams[s]
        rand, seq, buf, _ooff, keep = lib_fill[s]
        row = {"fetch_random_fill": ev_time(lambda: fill(s, rand))[0],
               "fetch_random_wrapper": ev_time(lambda: find.fetch_segments(blobs, boff, rand, "value"))[0],
               "fetch_stream_order_fill": ev_time(lambda: fill(s, seq))[0],
               "fetch_stream_order_wrapper": ev_time(lambda: find.fetch_segments(blobs, boff, seq, "value"))[0],
               "select_as_many_bytes": ev_time(lambda: ralledata.select_ralledata(blobs, boff, keep, want_index=False))[0],
               "clone_as_many_bytes": ev_time(lambda: buf.clone())[0]}
        if i >= 2:
            for k, v in row.items():
                t[k].append(v)
    out["fetch"] = {"sets": facts, **{k: med(v) for k, v in t.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
