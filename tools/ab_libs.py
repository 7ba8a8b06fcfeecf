#!/usr/bin/env python3
"""A/B timing of two builds of the batch library in ONE process (interleaved rounds):
the working tree's k2hash_amd/lib/libk2hash_amd.so against other builds (tools/build_ab.sh).
Every library's output is checked against the golden digest before it is timed.

  python tools/ab_libs.py --libs k2hash_amd/lib/ab/HEAD/libk2hash_amd.so [--config csr] [--variant 0]

Configs: fixed32, csr, fixed4096, fixed21 (golden digests); fixedNN for any other key length
(4M keys, checked against the oracle); ralledata; archive (k2h_amd_archive_prehash with the new
keys of RENAME records over 1M records drawn from tests/golden/archive.k2har, checked against
tests/golden/archive.json) and archive_scan (the fused k2h_amd_archive_scan_prehash_device).
List a library twice (under two paths) to see the run's A/A difference; the order of the
libraries rotates from round to round, and a copy of the tree's own library among --libs shows
what the load order alone does.
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from k2hash_amd import _native, batch  # noqa: E402
import oracle  # noqa: E402  (checker only)

p = argparse.ArgumentParser()
p.add_argument("--libs", default="", help="comma list of extra library paths (the tree's own is always first)")
p.add_argument("--config", default="csr")
p.add_argument("--variant", type=int, default=0)
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--reps", type=int, default=10)
p.add_argument("--warm-ms", type=float, default=300.0, help="GPU work before the first timed round (clock ramp)")
p.add_argument("--second", action="store_true")
p.add_argument("--index", action="store_true", help="fixed keys: the fused bucket-index form (kindex + ckindex)")
a = p.parse_args()

dev = torch.device("cuda:0")
if a.config == "ralledata":  # the bench's RALLEDATA workload, checked against its oracle digest
    import bench  # noqa: E402
    _, n, ((klo, khi), (vlo, vhi)), _ = bench.CONFIGS["ralledata"]
    cfg = {"kind": "ralledata"}
    gr = json.loads((ROOT / "tests" / "golden" / "ralledata_digest.json").read_text())
    ko = batch.synth_offsets(n, dev, klo, khi)
    vo = batch.synth_offsets(n, dev, vlo, vhi, seed=batch.SEED_LENS + 7)
    kb, vb = int(ko[-1].item()), int(vo[-1].item())
    kd = batch.synth_bytes(kb, dev)
    vd = batch.synth_bytes(vb, dev, byte_off=1 << 33)
    total = 80 * n + kb + vb
    blob = torch.zeros((total + 7) // 8 * 8, dtype=torch.uint8, device=dev)
    boff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    algo = 2 * (kb + vb) + 104 * n  # input + blob bytes, two offset arrays in, blob offsets out
elif a.config in ("archive", "archive_scan"):
    import archive_rate  # noqa: E402  (tools/: the replicated golden archive)
    from k2hash_amd import archive  # noqa: E402
    n = 1 << 20
    cfg = {"kind": "archive"}
    data, pick = archive_rate.replicate(n, seed=7, with_pick=True)
    gold = json.loads((ROOT / "tests" / "golden" / "archive.json").read_text())["records"]
    # h1 / h2 from the golden file; new_h1 / new_h2: the oracle's hashes of a RENAME record's exdata
    new = [bytes.fromhex(g["exdata"]) if g["type"] == 6 else None for g in gold]
    cols = [[int(g["h1"], 16) for g in gold], [int(g["h2"], 16) for g in gold],
            [oracle.k2h_hash(x) if x is not None else 0 for x in new],
            [oracle.k2h_second_hash(x) if x is not None else 0 for x in new]]
    want = [np.array(c, np.uint64)[pick] for c in cols]
    assert any(x is not None for x in new)
    recs_host = archive.scan(data)
    assert recs_host.size == n
    afile = torch.from_numpy(data).to(dev)
    arecs = torch.from_numpy(recs_host.view(np.int64).reshape(-1, archive.REC_WORDS).copy()).to(dev)
    arecs_out = torch.empty_like(arecs)
    aout = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
    algo = int(data.size) if a.config == "archive_scan" else 104 * n + 32 * n
else:
    dig = json.loads((ROOT / "tests/golden/digests.json").read_text())["configs"]
    name = {"fixed32": "fixed32_16M", "csr": "csr_8_256_64M", "fixed4096": "fixed4096_1M", "fixed21": "fixed21_1M"}.get(a.config)
    if name:
        cfg = dig[name]
    else:  # fixedNN: no golden digest, the oracle hashes the same synthetic bytes
        cfg = {"kind": "fixed", "n": 1 << 22, "key_len": int(a.config[len("fixed"):])}
        ref = oracle.hash_fixed(oracle.gen_bytes(cfg["n"] * cfg["key_len"]), cfg["key_len"])
        cfg["h1"], cfg["h2"] = ([f"{x:016x}" for x in oracle.digest(r)] for r in ref)
    n = cfg["n"]
sets = []
for s in range(2 if cfg["kind"] in ("fixed", "csr") else 0):
    if cfg["kind"] == "fixed":
        sets.append((batch.synth_bytes(n * cfg["key_len"], dev), None))
        algo = n * cfg["key_len"] + 8 * n
    else:
        off = batch.synth_offsets(n, dev, cfg["min_len"], cfg["max_len"])
        sets.append((batch.synth_bytes(int(off[-1].item()), dev), off))
        algo = int(off[-1].item()) + 16 * n + 8
if a.second:
    algo += 8 * n
if a.index:
    algo += 16 * n
    idx = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev))
out = (torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev))

paths = [str(_native.BATCH_LIB.relative_to(ROOT))] + [x for x in a.libs.split(",") if x]
libs = []
for path in paths:
    lib = _native._bind(ctypes.CDLL(str(Path(ROOT, path).resolve())), _native.SIGNATURES.keys())
    if a.variant:
        lib.k2h_amd_set_variant(a.variant)
    libs.append(lib)


def run(lib, i):
    if cfg["kind"] == "ralledata":
        rc = lib.k2h_amd_build_ralledata(kd.data_ptr(), ko.data_ptr(), vd.data_ptr(), vo.data_ptr(), None, None, None,
                                         None, n, blob.data_ptr(), boff.data_ptr(), 0,
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        return
    if cfg["kind"] == "archive":
        stream = torch.cuda.current_stream().cuda_stream
        if a.config == "archive_scan":
            cnt = ctypes.c_uint64()
            rc = lib.k2h_amd_archive_scan_prehash_device(afile.data_ptr(), afile.numel(), arecs_out.data_ptr(), n,
                                                         ctypes.byref(cnt), *[x.data_ptr() for x in aout], 0, stream)
            assert rc == 0 and cnt.value == n, (rc, cnt.value)
        else:
            rc = lib.k2h_amd_archive_prehash(afile.data_ptr(), afile.numel(), arecs.data_ptr(), n,
                                             *[x.data_ptr() for x in aout], 0, stream)
            assert rc == 0, rc
        return
    keys, off = sets[i & 1]
    h2 = out[1].data_ptr() if a.second else None
    stream = torch.cuda.current_stream().cuda_stream
    if off is None and a.index:
        rc = lib.k2h_amd_hash_fixed_index(keys.data_ptr(), cfg["key_len"], n, out[0].data_ptr(), h2, 0,
                                          (1 << 28) - 1, 0xF, idx[0].data_ptr(), idx[1].data_ptr(), stream)
    elif off is None:
        rc = lib.k2h_amd_hash_fixed(keys.data_ptr(), cfg["key_len"], n, out[0].data_ptr(), h2, 0, stream)
    else:
        rc = lib.k2h_amd_hash_csr(keys.data_ptr(), off.data_ptr(), n, out[0].data_ptr(), h2, 0, stream)
    assert rc == 0, rc


for path, lib in zip(paths, libs):
    if cfg["kind"] == "ralledata":
        blob.zero_()
        boff.zero_()
        run(lib, 0)
        torch.cuda.synchronize()
        ok = gr["n"] == n and gr["bytes"] == total and bench.digest_dev(blob.view(torch.int64), 0) == gr["blob"] \
            and bench.digest_dev(boff, 0) == gr["blob_off"]
        print(f"{path}: parity {'OK' if ok else 'MISMATCH'}", flush=True)
        if not ok:
            sys.exit(1)
        continue
    if cfg["kind"] == "archive":
        for x in aout:
            x.zero_()
        run(lib, 0)
        torch.cuda.synchronize()
        ok = all(np.array_equal(aout[j].cpu().numpy().view(np.uint64), want[j]) for j in range(4))
        print(f"{path}: parity {'OK' if ok else 'MISMATCH'}", flush=True)
        if not ok:
            sys.exit(1)
        continue
    out[0].zero_()
    run(lib, 0)
    torch.cuda.synchronize()
    ok = [f"{x:016x}" for x in oracle.digest(out[0].cpu().numpy().view(np.uint64))] == cfg["h1"]
    if a.second:
        ok = ok and [f"{x:016x}" for x in oracle.digest(out[1].cpu().numpy().view(np.uint64))] == cfg["h2"]
    print(f"{path}: parity {'OK' if ok else 'MISMATCH'}", flush=True)
    if not ok:
        sys.exit(1)

# The chip ramps its clock over the first ~150 ms of work after the (idle) parity phase; without
# a warm-up the first timed region -- always the tree's library -- measures that ramp.
t_warm = time.perf_counter()
while time.perf_counter() - t_warm < a.warm_ms / 1e3:
    for lib in libs:
        for i in range(20):
            run(lib, i)
    torch.cuda.synchronize()

times = {p_: [] for p_ in paths}
for r in range(a.rounds):
    order = list(zip(paths, libs))
    order = order[r % len(order):] + order[:r % len(order)]  # every library takes every place in a round
    for path, lib in order:
        for i in range(3):
            run(lib, i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.reps):
            run(lib, i)
        e1.record()
        torch.cuda.synchronize()
        times[path].append(e0.elapsed_time(e1) / a.reps)
for path in paths:
    med = statistics.median(times[path])
    print(json.dumps({"config": a.config, "lib": path, "variant": a.variant, "ms_median": med,
                      "ms_min": min(times[path]), "ms_rounds": times[path], "frac_8TBps": algo / med / 1e6 / 8000,
                      "Gkeys_s": n / med / 1e6}), flush=True)
