"""Time of k2h_amd_ralledata_delta.  The held stream: --records blobs built from
bench.ralledata_set (keys 8-64 B, values 0-256 B).  The new stream: the same with a fraction f of
the blobs given a new value of the same length (the first value byte flipped; a blob without a
value stays as it is), f / 4 of the blobs removed and f / 4 as many blobs of fresh keys appended,
for each f of --fractions.  Timed, whole native calls between HIP events and by the host's clock,
into buffers allocated before, the median of --reps runs after warm-up with the fastest and the
slowest: the delta alone (rel and seen given), the diff alone, and the two together; and as
yardsticks in the same run the existing incremental route -- the diff, k2h_amd_ralledata_select of
the changed blobs and k2h_amd_ralledata_archive over them, which writes more bytes and no
deletions --, its select and its archive's size pass alone, and at f = 1 the archive of the whole
new stream.  The project's rule is evaluated per fraction: at f = 1 the delta
against twice the archive's time per output byte, below it against the archive's size pass plus
twice the select's time on the same kept bytes.

    python tools/ralledata_delta_rate.py [--records N] [--reps R] [--fractions F,..] [--libs PATH,..] > ralledata_delta_rate.json

--libs: other builds of the library, loaded into the same process; their delta is timed in the same
loop as this build's, after its log was compared with this build's (the build kernel over every
slot against the compacted list: a build with -DK2H_DELTA_ALL_SLOTS=1).  Per-kernel times come from a run of this tool with --stage-trace under
`rocprofv3 --kernel-trace --stats`, in a process of its own.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np  # noqa: E402


def make_new(torch, dev, parts, n, f, seed):
    """The new stream of fraction f over the held stream's inputs `parts`: (blobs, blob_off, what)."""
    import bench
    from k2hash_amd import ralledata
    kd, ko, vd, vo = parts
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    u = torch.rand(n, device=dev, generator=gen)
    changed = u < f
    removed = (u >= f) & (u < f + f / 4) if f < 1 else torch.rand(n, device=dev, generator=gen) < 0.25
    has_val = vo[1:] > vo[:-1]
    vd2 = vd.clone()
    at = vo[:-1][changed & has_val]
    vd2[at] ^= 0xFF
    mod, moff = ralledata.build_ralledata(kd, ko, vd2, vo)
    del vd2
    kept = ralledata.select_ralledata(mod, moff, (~removed).to(torch.uint8), want_index=False)
    del mod, moff
    fresh = max(int(n * f / 4), 1)
    (kd1, ko1, vd1, vo1), _o, _t = bench.ralledata_set(dev, fresh, 1)
    del _o
    extra, eoff = ralledata.build_ralledata(kd1, ko1, vd1, vo1)
    blobs = torch.cat([kept.blobs, extra])
    off = torch.cat([kept.blob_off, eoff[1:] + kept.blob_off[-1]])
    what = {"changed_values": int((changed & has_val & ~removed).sum().item()), "removed": int(removed.sum().item()),
            "fresh_keys": fresh, "new_blobs": int(off.numel() - 1), "new_bytes": int(blobs.numel())}
    return blobs, off, what


def self_check(torch, dev):
    """A small pair of this generator against the tests' model, byte for byte."""
    import bench
    import ralle_delta_model as dl
    import ralle_diff_model as df
    from k2hash_amd import delta, ralledata
    n = 3000
    parts, _o, _t = bench.ralledata_set(dev, n, 0)
    held, hoff = ralledata.build_ralledata(*parts)
    new, noff, what = make_new(torch, dev, parts, n, 0.25, 5)
    d = delta.delta_log(new, noff, held, hoff, last_copies=False, want_made=True)
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy()  # noqa: E731
    m = df.diff_model(h(new).tobytes(), h(noff), h(held).tobytes(), h(hoff))
    want = dl.delta_model(h(new).tobytes(), h(noff), m[0], h(held).tobytes(), h(hoff), None, m[2])
    assert h(d.log).tobytes() == want[0] and list(d.counts) == want[3] and (h(d.made) == want[2]).all()
    return {"blobs": n, "counts": want[3], **what}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fractions", default="0.01,0.25,1")
    ap.add_argument("--stage-trace", action="store_true",
                    help="for a run under rocprofv3: only the delta filling its buffer, a few times per fraction")
    ap.add_argument("--libs", default="",
                    help="comma list of other builds of the library whose delta is timed beside this one's, in the "
                         "same process (the all-slots build: make OUT=<dir> EXTRA_HIPFLAGS=-DK2H_DELTA_ALL_SLOTS=1)")
    a = ap.parse_args()
    import ctypes

    import torch

    import bench
    from k2hash_amd import _native, delta, ralledata
    _native.batch_lib()
    others = {p: _native._bind(ctypes.CDLL(str(Path(p).resolve())), _native.SIGNATURES.keys())
              for p in a.libs.split(",") if p}
    from k2hash_amd.ralledata import DIFF_ATTRS, DIFF_DATA, DIFF_FOUND, DIFF_PART, DIFF_SKEY, DIFF_VAL
    dev = torch.device("cuda", 0)
    n = a.records
    out = {"reps": a.reps, "held_blobs": n, "self_check": None if a.stage_trace else self_check(torch, dev), "fractions": {}}

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0, r

    def summarise(ts):
        ev, wall = [t[0] for t in ts], [t[1] for t in ts]
        return {"median_s": float(np.median(ev)), "min_s": float(np.min(ev)), "max_s": float(np.max(ev)),
                "host_clock_median_s": float(np.median(wall))}

    parts, _o, _t = bench.ralledata_set(dev, n, 0)
    del _o
    held, hoff = ralledata.build_ralledata(*parts)
    out["held_bytes"] = int(held.numel())
    for f in (float(x) for x in a.fractions.split(",")):
        new, noff, what = make_new(torch, dev, parts, n, f, 100)
        d = ralledata.diff_ralledata(new, noff, held, hoff, want_seen=True, count=False)
        rel, seen = d.rel, d.seen
        first = delta.delta_records(new, noff, rel, held, hoff, seen, count_only=True)
        buf = torch.empty(max(first.counts.bytes, 1), dtype=torch.uint8, device=dev)

        def changed_of(r):
            differs = (r & (DIFF_VAL | DIFF_SKEY | DIFF_ATTRS)) != 0
            return (((r & DIFF_PART) != 0) & torch.where((r & DIFF_FOUND) != 0, differs, (r & DIFF_DATA) != 0)).to(torch.uint8)
        mask = changed_of(rel)
        sel0 = ralledata.select_ralledata(new, noff, mask, count_only=True)
        selbuf = torch.empty(max(sel0.kept_bytes, 1), dtype=torch.uint8, device=dev)
        sel = ralledata.select_ralledata(new, noff, mask, out=selbuf, want_index=False)
        arc0 = ralledata.ralledata_to_archive(sel.blobs, sel.blob_off, count_only=True)
        arcbuf = torch.empty(max(arc0.total, 1), dtype=torch.uint8, device=dev)
        res = {"workload": what, "counts": first.counts._asdict(), "route_kept_blobs": int(sel0.kept),
               "route_kept_bytes": int(sel0.kept_bytes), "route_archive_bytes": int(arc0.total)}

        def route():
            x = ralledata.diff_ralledata(new, noff, held, hoff, want_seen=True, count=False)
            s = ralledata.select_ralledata(new, noff, changed_of(x.rel), out=selbuf, want_index=False)
            return ralledata.ralledata_to_archive(s.blobs, s.blob_off, out=arcbuf)

        def both():
            x = ralledata.diff_ralledata(new, noff, held, hoff, want_seen=True, count=False)
            return delta.delta_records(new, noff, x.rel, held, hoff, x.seen, out=buf)
        calls = {"delta": lambda: delta.delta_records(new, noff, rel, held, hoff, seen, out=buf)}
        if not a.stage_trace:
            calls.update({
                "delta_count_only": lambda: delta.delta_records(new, noff, rel, held, hoff, seen, count_only=True),
                "diff": lambda: ralledata.diff_ralledata(new, noff, held, hoff, want_seen=True, count=False),
                "diff_plus_delta": both,
                "yardstick_route_diff_select_archive": route,
                "yardstick_select_changed": lambda: ralledata.select_ralledata(new, noff, mask, out=selbuf, want_index=False),
                "yardstick_archive_size_pass": lambda: ralledata.ralledata_to_archive(new, noff, keep=mask, count_only=True),
            })
            if f >= 1:
                whole0 = ralledata.ralledata_to_archive(new, noff, count_only=True)
                wholebuf = torch.empty(whole0.total, dtype=torch.uint8, device=dev)
                res["whole_archive_bytes"] = int(whole0.total)
                calls["yardstick_archive_whole_new_stream"] = lambda: ralledata.ralledata_to_archive(new, noff, out=wholebuf)
        for path, lib in others.items():   # another build's delta, interleaved with this one's in the same loop
            def other(lib=lib):
                mine, _native._batch = _native._batch, lib
                try:
                    return delta.delta_records(new, noff, rel, held, hoff, seen, out=buf)
                finally:
                    _native._batch = mine
            calls["delta"]()
            want = buf.clone()
            buf.zero_()
            other()
            assert torch.equal(buf, want), f"{path}: another log than this build's"
            calls[f"delta[{path}]"] = other
        for _ in range(3):
            for fn in calls.values():
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(3 if a.stage_trace else a.reps):
            for k, fn in calls.items():
                ts[k].append(ev_time(fn)[:2])
        res.update({k: summarise(v) for k, v in ts.items()})
        if not a.stage_trace:
            t = res["delta"]["median_s"]
            if f >= 1:
                per_byte = res["yardstick_archive_whole_new_stream"]["median_s"] / res["whole_archive_bytes"]
                bound = 2 * per_byte * first.counts.bytes
                res["rule"] = {"kind": "twice the archive's time per output byte", "bound_s": bound, "delta_s": t,
                               "exceeded": bool(t > bound)}
            else:
                bound = res["yardstick_archive_size_pass"]["median_s"] + 2 * res["yardstick_select_changed"]["median_s"]
                res["rule"] = {"kind": "the archive's size pass plus twice the select of the kept bytes", "bound_s": bound,
                               "delta_s": t, "exceeded": bool(t > bound)}
        out["fractions"][str(f)] = res
        del new, noff, buf, selbuf, arcbuf, rel, seen, mask, sel, d
        if f >= 1 and not a.stage_trace:
            del wholebuf
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
