"""Rate of the blob build from range records: the synthetic TSV of
tools/import_rate.py (N records, keys 8-64 B, values 0-200 B) resident in HBM and already scanned
-> k2h_amd_import_ralledata, against the route the parent commit offers for the same job: gather
key + NUL and value + NUL into CSR buffers with torch index ops, then k2h_amd_build_ralledata.

Same process, the two routes alternating, device events, two rotated output buffers per route so
that no output line is still in a cache; median and spread over --reps repetitions.  The build
kernel alone is not a separate call: it is reported as (size + build call) - (size-only call).

    python tools/import_ralledata_rate.py [--records N] [--reps R] > import_ralledata_rate.json
"""
import argparse
import ctypes
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from k2hash_amd import _native, archive, ralledata  # noqa: E402
from k2hash_amd.batch import _stream_handle  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X


def stats(ms):
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]),
            "p10_ms": float(a[int(0.1 * (a.size - 1))]), "p90_ms": float(a[int(round(0.9 * (a.size - 1)))]), "reps": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 23)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    n = a.records
    kl = rng.integers(8, 65, n)
    vl = rng.integers(0, 201, n)
    off = np.concatenate([[0], np.cumsum(kl + vl + 2)])
    data = rng.integers(32, 127, int(off[-1]), dtype=np.uint8)
    data[off[:-1] + kl] = 9
    data[off[1:] - 1] = 10
    size = data.size
    dev = torch.device("cuda", 0)
    f = torch.from_numpy(data).to(dev)
    recs = archive.import_scan_device(f)
    assert recs.shape[0] == n
    lib = _native.batch_lib()
    st = _stream_handle(None)
    fp, rp = ctypes.c_void_p(f.data_ptr()), ctypes.c_void_p(recs.data_ptr())
    total = ctypes.c_uint64(0)
    blob_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    bp = ctypes.c_void_p(blob_off.data_ptr())

    def size_only():
        _native.check(lib.k2h_amd_import_ralledata(fp, size, rp, n, None, 0, bp, ctypes.byref(total), 0, st))

    size_only()
    nbytes = int(total.value)
    outs = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
    outs_old = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
    boff_old = torch.empty(n + 1, dtype=torch.int64, device=dev)

    def build(k):
        _native.check(lib.k2h_amd_import_ralledata(fp, size, rp, n, ctypes.c_void_p(outs[k].data_ptr()), nbytes, bp,
                                                   ctypes.byref(total), 0, st))

    def new_path(k):  # what import_to_ralledata does, into a rotated buffer
        size_only()
        build(k)

    def gather(starts, lens):
        """CSR bytes of range + NUL per record, by index ops: (bytes, offsets n + 1)."""
        l1 = lens + 1
        o = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(l1, 0, out=o[1:])
        nb = int(o[-1].item())
        rec = torch.repeat_interleave(torch.arange(n, device=dev), l1, output_size=nb)
        src = torch.arange(nb, device=dev) - o[rec] + starts[rec]
        b = f[src]
        b[o[1:] - 1] = 0
        return b, o

    def parent_route(k):
        kb, ko = gather(recs[:, 0], recs[:, 1])
        vb, vo = gather(recs[:, 2], recs[:, 3])
        return ralledata.build_ralledata(kb, ko, vb, vo, out=outs_old[k], blob_off=boff_old, total=nbytes)

    def timed(fn, *args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*args)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the CSR producer alone over the same records, its inputs gathered once outside the timing:
    # the yardstick for the build kernel on this byte mix (same blobs out, the payload in)
    kb0, ko0 = gather(recs[:, 0], recs[:, 1])
    vb0, vo0 = gather(recs[:, 2], recs[:, 3])

    def csr_producer(k):
        ralledata.build_ralledata(kb0, ko0, vb0, vo0, out=outs_old[k], blob_off=boff_old, total=nbytes)

    for k in range(2):  # warm up, and the two routes agree
        new_path(k)
        parent_route(k)
    torch.cuda.synchronize()
    assert torch.equal(outs[1], outs_old[1]) and torch.equal(blob_off, boff_old)
    t_new, t_old, t_size, t_build, t_csr = [], [], [], [], []
    for i in range(a.reps):
        k = i & 1
        t_new.append(timed(new_path, k))
        t_old.append(timed(parent_route, k))
        t_size.append(timed(size_only))
        t_build.append(timed(build, k))
        t_csr.append(timed(csr_producer, k))
    kernel_ms = float(np.median(t_build)) - float(np.median(t_size))
    algo = size + nbytes + 32 * n + 8 * n  # file read + blobs written + recs + blob_off
    csr_ms = float(np.median(t_csr))
    csr_algo = int(kb0.numel() + vb0.numel()) + nbytes + 24 * n  # payload read + blobs + two offsets in, one out
    print(json.dumps({
        "workload": f"{n} TSV records, keys 8-64 B, values 0-200 B, {size} file bytes, {nbytes} blob bytes",
        "new_path": stats(t_new), "parent_route": stats(t_old),
        "size_only_call": stats(t_size), "size_and_build_call": stats(t_build),
        "new_below_parent": bool(np.median(t_new) < np.median(t_old)),
        "speedup_of_medians": float(np.median(t_old) / np.median(t_new)),
        "build_kernel": {"ms": kernel_ms, "algorithmic_bytes": int(algo), "TB_per_s": algo / kernel_ms / 1e9,
                         "fraction_of_hbm_peak": algo / (kernel_ms * 1e-3) / HBM_PEAK,
                         "derived_as": "median(size + build call) - median(size-only call)"},
        "csr_producer_same_records": {**stats(t_csr), "algorithmic_bytes": csr_algo, "TB_per_s": csr_algo / csr_ms / 1e9,
                                      "fraction_of_hbm_peak": csr_algo / (csr_ms * 1e-3) / HBM_PEAK},
    }))


if __name__ == "__main__":
    main()
