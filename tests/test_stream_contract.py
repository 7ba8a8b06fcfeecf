"""The `stream` argument of every device entry point (k2hash_amd/batch.py's module docstring,
include/k2hash_amd.h section 2): stream=None is the current torch stream; otherwise every
device operation of the call, the wrapper's own torch ops included, is ordered on `stream` and
none on the current stream.

The rest of the suite runs on an idle default stream and synchronises the device afterwards, so
a launch, a memset or a torch op issued to the wrong stream passes it: its inputs were ready
long before.  Here the call names a stream `s` while another stream `c` is current, and one of
the two is held up by a delay (stream_harness.stall):

  late inputs    `s` is stalled and the real inputs arrive on it behind the stall, over a decoy;
                 work issued anywhere but `s` reads the decoy and computes its answer
  busy current   `c` is stalled; work issued to `c`, or a read-back on it, is not done when the
                 results have reached the host through `s` (or the host waited for `c`)
  host structs   overwritten while the call's kernels still wait behind the stall
  shared scratch two calls on two streams share one per-device scratch: the second waits for the
                 first's event

Expected values come from the oracle and the CPU models through stream_cases.py, never from a
device call.  Every test that relies on a stall asserts stalled(ev) where it relies on it.
"""
import concurrent.futures
import ctypes
import re
import time

import numpy as np
import pytest

from conftest import ROOT

import ralle_times_model as tm
import stream_cases as sc
import stream_harness as sh
from stream_harness import independent_streams, stall, stalled

from k2hash_amd import _native, ralledata

NAMES = [c.name for c in sc.ALL]
SEED_LATE, SEED_BUSY, SEED_ABI, SEED_X, SEED_Y = 1, 2, 3, 4, 5   # SEED_BUSY is used by the busy-current test alone
PIN_WAIT_MS = 10.0   # what the scratch pin gives the second call: a sixth of a stall, far more than the call needs


# ------------------------------------------------------------------------------------- CPU
def test_every_wrapper_with_a_stream_parameter_has_a_case():
    found = sc.public_stream_functions()
    assert len(found) >= 32
    assert found == set(sc.CASES), sorted(found ^ set(sc.CASES))
    for func, variants in sc.CASES.items():
        assert variants and all(c.name.split("[")[0] == func for c in variants), func
    assert len(set(NAMES)) == len(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_decoy_has_the_shapes_and_another_answer(oracle, name):
    case = sc.BY_NAME[name]
    real, decoy, want, other = sc.inputs(oracle, name, SEED_LATE)
    assert set(real) == set(decoy) and set(want) == set(other) and want
    for k, v in real.items():
        if isinstance(v, np.ndarray):
            assert decoy[k].shape == v.shape and decoy[k].dtype == v.dtype, k
    for k in want:
        if case.inert or k in case.by_shape:
            assert sc.same(other[k], want[k]), k     # the exemption is no wider than it has to be
        else:
            assert not sc.same(other[k], want[k]), f"{name}: the decoy's {k} equals the real one"


def test_the_asynchronous_forms_are_the_ones_the_header_names():
    """is_async of the table against the header: every form it calls asynchronous, and no form
    whose section says it synchronises `stream`."""
    header = re.sub(r"\s*\n\s*\*\s*", " ", (ROOT / "include" / "k2hash_amd.h").read_text())
    for phrase in ("the call is asynchronous on it unless its section says how often it synchronises `stream`",
                   "k2h_amd_ralledata_check (async on `stream`)", "k2h_amd_ralledata_times (async on `stream`",
                   "dropped == NULL: asynchronous on `stream`", "k2h_amd_archive_prehash (async on `stream`)",
                   "record (async on `stream`)", "counts != NULL: `stream` is synchronised once; else the call is "
                   "asynchronous"):
        assert phrase in header, phrase
    want = {"batch.hash_fixed", "batch.hash_fixed[out]", "batch.hash_csr", "batch.bucket_index", "batch.hash_fixed_index",
            "batch.hash_csr_index", "batch.bucket_index_table", "batch.hash_fixed_index_table",
            "batch.hash_csr_index_table", "batch.synth_bytes", "archive.prehash_device", "archive.import_prehash_device",
            "ralledata.check_ralledata", "ralledata.blob_times", "ralledata.dedup_ralledata[count=False]",
            "ralledata.dedup_ralledata[count=False,pts]", "ralledata.diff_ralledata[count=False]",
            "ralledata.build_ralledata[total,out]"}
    assert {c.name for c in sc.ALL if c.is_async} == want


# ------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module", autouse=True)
def _stall_report():
    """Once, after the module's tests: the stall's unit and length and how many candidate pairs
    the stream probe passed over (shown with -s or -rA)."""
    yield
    if sh.report().get("stall_unit"):
        print("\nstream_harness:", sh.report())


def _to_dev(torch, cuda, arrays, host=None):
    """arrays' numpy entries as device tensors; host values from `host` (default: arrays)."""
    host = arrays if host is None else host
    return {k: torch.from_numpy(v).to(cuda) if isinstance(v, np.ndarray) else host[k] for k, v in arrays.items()}


def _back(torch, out, s):
    """The outputs on the host, read through `s`."""
    with torch.cuda.stream(s):
        got = {k: v.cpu() if torch.is_tensor(v) else v for k, v in out.items()}
    s.synchronize()
    return {k: v.numpy() if torch.is_tensor(v) else v for k, v in got.items()}


def _compare(name, got, want):
    assert set(got) == set(want), (name, sorted(got), sorted(want))
    for k in want:
        assert sc.same(got[k], want[k]), f"{name}: {k} differs from the model"


def _warm(torch, case, dev, c, s):
    """One call on the default stream and one as the tests make it (c current, stream=s): the
    scratch of the launchers is grown (its hipFree waits for the whole device) and both
    streams' allocator pools hold blocks of these sizes before anything is stalled."""
    keep = [case.run(dev, None)]
    torch.cuda.synchronize()
    with torch.cuda.stream(c):
        keep.append(case.run(dev, s))
    torch.cuda.synchronize()


def _poison(torch, c, cuda):
    """Memory the current stream's pool will hand out next holds 0x5A, not an earlier answer.
    The warm-up ran on this test's decoy, so for an output no decoy can change (out_off of
    partition's n == 0, the outputs a case lists in by_shape) this fill alone stands between a
    write that was never ordered and the right value left in a reused block.  torch keeps one
    pool per stream for requests of up to 1 MiB and one for larger ones, and hands out the
    smallest free block that fits: hence many of the smallest blocks (what an 8-byte out_off
    takes), a 1 MiB fill that covers the rest of a small-pool segment, and a large one."""
    with torch.cuda.stream(c):
        junk = [torch.full((512,), 0x5A, dtype=torch.uint8, device=cuda) for _ in range(64)]
        junk += [torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device=cuda),
                 torch.full((8 << 20,), 0x5A, dtype=torch.uint8, device=cuda)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_late_inputs(cuda, oracle, name):
    """The inputs arrive on `stream` behind a stall, over a decoy; another, idle stream is
    current.  Whatever the call issues off `stream` runs at once, on the decoy."""
    import torch
    case = sc.BY_NAME[name]
    c, s = independent_streams(cuda)
    real, decoy, want, _other = sc.inputs(oracle, name, SEED_LATE)
    _warm(torch, case, _to_dev(torch, cuda, decoy), c, s)
    dev = _to_dev(torch, cuda, decoy, host=real)
    staged = _to_dev(torch, cuda, real)
    torch.cuda.synchronize()
    ev = stall(s)
    with torch.cuda.stream(s):
        for k, v in staged.items():
            if torch.is_tensor(v):
                dev[k].copy_(v)
    out = {}
    with torch.cuda.stream(c):
        ms = sh.host_ms(lambda: out.update(case.run(dev, s)))
        if case.is_async:
            assert stalled(ev), f"{name} is documented asynchronous: it returned after {ms:.2f} ms, the stall was over"
    print(f"{name}: host {ms:.3f} ms" + ("" if case.is_async else " (synchronises)"))
    _compare(name, _back(torch, out, s), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_busy_current_stream(cuda, oracle, name):
    """The current stream is stalled, the call names another: the results reach the host
    through `stream` while the current one is still stalled, so the call neither waited for the
    current stream nor left work on it."""
    import torch
    case = sc.BY_NAME[name]
    c, s = independent_streams(cuda)
    real, decoy, want, _other = sc.inputs(oracle, name, SEED_BUSY)
    _warm(torch, case, _to_dev(torch, cuda, decoy), c, s)
    dev = _to_dev(torch, cuda, real)
    _poison(torch, c, cuda)
    torch.cuda.synchronize()
    with torch.cuda.stream(c):
        ev = stall(c)
        out = {}
        ms = sh.host_ms(lambda: out.update(case.run(dev, s)))
    got = _back(torch, out, s)
    still = stalled(ev)
    print(f"{name}: host {ms:.3f} ms")
    assert still, f"{name}: the current stream's stall was over when the results arrived (call: {ms:.2f} ms on the host)"
    _compare(name, got, want)
    del out


# ---------------------------------------------------------- host structs, at the C ABI
def _p(t):
    return ctypes.c_void_p(t.data_ptr() or 1)


def _abi_check(torch, lib, d, h):
    n = d["blob_off"].numel() - 1
    o = dict(status=torch.empty(n, dtype=torch.uint8, device=d["blobs"].device),
             route=torch.empty(n, dtype=torch.uint8, device=d["blobs"].device),
             h1=torch.empty(n, dtype=torch.int64, device=d["blobs"].device),
             h2=torch.empty(n, dtype=torch.int64, device=d["blobs"].device))
    st = sc.RANGE.ctypes()
    rc = lib.k2h_amd_ralledata_check(_p(d["blobs"]), d["blobs"].numel(), _p(d["blob_off"]), n, ctypes.byref(st), 0,
                                     _p(o["status"]), _p(o["route"]), _p(o["h1"]), _p(o["h2"]), h)
    return rc, o, st, sc.RANGE_2.ctypes()


def _abi_times(torch, lib, d, h):
    n, dev = d["blob_off"].numel() - 1, d["blobs"].device
    o = dict(flags=torch.empty(n, dtype=torch.uint8, device=dev), mtime=torch.empty((n, 2), dtype=torch.int64, device=dev),
             expire=torch.empty((n, 2), dtype=torch.int64, device=dev), keep=torch.empty(n, dtype=torch.uint8, device=dev))
    st = ralledata.TimeWindow(**sc.WINDOW).ctypes()
    rc = lib.k2h_amd_ralledata_times(_p(d["blobs"]), d["blobs"].numel(), _p(d["blob_off"]), n, _p(d["consider"]),
                                     ctypes.byref(st), None, _p(o["flags"]), _p(o["mtime"]), _p(o["expire"]),
                                     _p(o["keep"]), h)
    return rc, o, st, ralledata.TimeWindow(**sc.WINDOW_2).ctypes()


def _abi_dedup_mtime(torch, lib, d, h):
    n, dev = d["blob_off"].numel() - 1, d["blobs"].device
    o = dict(keep=torch.empty(n, dtype=torch.uint8, device=dev), by=torch.empty(n, dtype=torch.int64, device=dev))
    st = _native.Timespec(*sc.PTS)
    rc = lib.k2h_amd_ralledata_dedup_mtime(_p(d["blobs"]), d["blobs"].numel(), _p(d["blob_off"]), n, _p(d["consider"]),
                                           _p(o["keep"]), _p(o["by"]), None, ctypes.byref(st), h)
    return rc, o, st, _native.Timespec(*sc.PTS_2)


def _abi_diff(torch, lib, d, h):
    na, nb, dev = d["a_blob_off"].numel() - 1, d["b_blob_off"].numel() - 1, d["a_blobs"].device
    o = dict(rel=torch.empty(na, dtype=torch.uint8, device=dev), match=torch.empty(na, dtype=torch.int64, device=dev),
             seen=torch.empty(nb, dtype=torch.uint8, device=dev))
    st = _native.DiffTimes(_native.Timespec(*sc.PTS), _native.Timespec(*tm.NOW))
    rc = lib.k2h_amd_ralledata_diff(_p(d["a_blobs"]), d["a_blobs"].numel(), _p(d["a_blob_off"]), na, _p(d["a_consider"]),
                                    _p(d["b_blobs"]), d["b_blobs"].numel(), _p(d["b_blob_off"]), nb, _p(d["b_consider"]),
                                    ctypes.byref(st), _p(o["rel"]), _p(o["match"]), _p(o["seen"]), None, h)
    return rc, o, st, _native.DiffTimes(_native.Timespec(*sc.PTS_2), _native.Timespec(*sc.NOW_2))


def _table_outs(torch, d, dev, hashes):
    n = sc.N
    o = dict(kindex=torch.empty(n, dtype=torch.int64, device=dev), ckindex=torch.empty(n, dtype=torch.int64, device=dev),
             found=torch.empty(n, dtype=torch.uint8, device=dev))
    if hashes:
        o.update(h1=torch.empty(n, dtype=torch.int64, device=dev), h2=torch.empty(n, dtype=torch.int64, device=dev))
    bitmap = d["assigned"].data_ptr()
    return o, _native.Table(sc.CUR_MASK, sc.COL_MASK, bitmap), _native.Table(*sc.MASKS_2, bitmap)


def _abi_index_table(torch, lib, d, h):
    o, st, other = _table_outs(torch, d, d["h1"].device, False)
    rc = lib.k2h_amd_bucket_index_table(_p(d["h1"]), sc.N, ctypes.byref(st), _p(o["kindex"]), _p(o["ckindex"]),
                                        _p(o["found"]), h)
    return rc, o, st, other


def _abi_fixed_table(torch, lib, d, h):
    o, st, other = _table_outs(torch, d, d["keys"].device, True)
    rc = lib.k2h_amd_hash_fixed_index_table(_p(d["keys"]), d["key_len"], sc.N, _p(o["h1"]), _p(o["h2"]), 0,
                                            ctypes.byref(st), _p(o["kindex"]), _p(o["ckindex"]), _p(o["found"]), h)
    return rc, o, st, other


def _abi_csr_table(torch, lib, d, h):
    o, st, other = _table_outs(torch, d, d["data"].device, True)
    rc = lib.k2h_amd_hash_csr_index_table(_p(d["data"]), _p(d["offsets"]), sc.N, _p(o["h1"]), _p(o["h2"]), 0,
                                          ctypes.byref(st), _p(o["kindex"]), _p(o["ckindex"]), _p(o["found"]), h)
    return rc, o, st, other


# entry point -> (the case whose inputs it shares, the call, the outputs its host struct decides)
ABI = {
    "k2h_amd_ralledata_check": ("ralledata.check_ralledata", _abi_check, ("route",)),
    "k2h_amd_ralledata_times": ("ralledata.blob_times", _abi_times, ("keep",)),
    "k2h_amd_ralledata_dedup_mtime": ("ralledata.dedup_ralledata[count=False,pts]", _abi_dedup_mtime, ("keep",)),
    "k2h_amd_ralledata_diff": ("ralledata.diff_ralledata[count=False]", _abi_diff, ("rel",)),
    "k2h_amd_bucket_index_table": ("batch.bucket_index_table", _abi_index_table, ("kindex", "ckindex", "found")),
    "k2h_amd_hash_fixed_index_table": ("batch.hash_fixed_index_table", _abi_fixed_table, ("kindex", "ckindex", "found")),
    "k2h_amd_hash_csr_index_table": ("batch.hash_csr_index_table", _abi_csr_table, ("kindex", "ckindex", "found")),
}


@pytest.mark.parametrize("entry", list(ABI))
def test_the_overwriting_struct_gives_another_answer(oracle, entry):
    """What test_host_struct_is_consumed_before_return overwrites the struct with would change
    every output the struct decides: a call that read it late could not pass."""
    name, _call, decided = ABI[entry]
    real = sc.inputs(oracle, name, SEED_ABI)[0]
    want, other = sc.abi_expect(oracle, entry, real), sc.abi_expect(oracle, entry, real, other=True)
    assert set(want) == set(other) and set(decided) <= set(want)
    for k in decided:
        assert not sc.same(other[k], want[k]), f"{entry}: {k} is the same under both structs"


@pytest.mark.gpu
@pytest.mark.parametrize("entry", list(ABI))
def test_host_struct_is_consumed_before_return(cuda, oracle, entry):
    """The struct a call takes by pointer is overwritten in place, with another valid value,
    while the call's kernels still wait behind the stall: the results are those of the original."""
    import torch
    name, call, _decided = ABI[entry]
    case = sc.BY_NAME[name]
    c, s = independent_streams(cuda)
    real, decoy, _want, _other = sc.inputs(oracle, name, SEED_ABI)
    _warm(torch, case, _to_dev(torch, cuda, decoy), c, s)
    dev = _to_dev(torch, cuda, real)
    torch.cuda.synchronize()
    ev = stall(s)
    with torch.cuda.stream(c):
        rc, out, st, other = call(torch, _native.batch_lib(), dev, ctypes.c_void_p(s.cuda_stream))
        _native.check(rc)
        assert stalled(ev), f"{entry} returned after the stall was over"
        ctypes.memmove(ctypes.byref(st), ctypes.byref(other), ctypes.sizeof(st))
        assert stalled(ev), f"{entry}: the struct was overwritten only after the stall was over"
    _compare(entry, _back(torch, out, s), sc.abi_expect(oracle, entry, real))


# ------------------------------------------------------------------ the shared scratch
def _head(name, d, n):
    """The first n blobs, records or lines of a case's inputs (n of the two-stream case: of A,
    and half as many of B)."""
    def cut(blobs, off, m):
        return blobs[:int(off[m])].copy(), off[:m + 1].copy()
    out = dict(d)
    if "a_blobs" in d:
        out["a_blobs"], out["a_blob_off"] = cut(d["a_blobs"], d["a_blob_off"], n)
        out["b_blobs"], out["b_blob_off"] = cut(d["b_blobs"], d["b_blob_off"], n // 2)
        out["a_consider"], out["b_consider"] = d["a_consider"][:n].copy(), d["b_consider"][:n // 2].copy()
    elif "blobs" in d:
        out["blobs"], out["blob_off"] = cut(d["blobs"], d["blob_off"], n)
        for k in ("keep", "consider"):
            if k in d:
                out[k] = d[k][:n].copy()
    else:
        from k2hash_amd import archive
        recs = archive.scan(bytes(d["file"]))
        out["file"] = d["file"][:int(recs["offset"][n])].copy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ralledata.dedup_ralledata[count=False]", "ralledata.dedup_ralledata[count=False,pts]",
                                  "ralledata.diff_ralledata[count=False]"])
def test_shared_scratch_pin_second_stream_waits_for_the_first(cuda, oracle, name):
    """A pin on the present design: the launcher's temporaries are one grow-only scratch per
    device, so call Y on one stream waits for the event call X recorded on another.  X sits
    behind a stall; Y, issued after it on a stream that runs beside X's, is then given
    PIN_WAIT_MS -- dozens of times the device time a warm Y needs alone -- and must still not be
    done, with X's stall still running: only the wait on X's event holds it.  Without the
    hipStreamWaitEvent, or without the hipEventRecord it waits for, Y finishes within that
    time and the test fails; it is deterministic in both directions.  Both results equal their
    models.  (Y is the smaller call; a larger one would grow the scratch, whose hipFree waits
    for the device on the host.)"""
    import torch
    case = sc.BY_NAME[name]
    s1, s2 = independent_streams(cuda)
    x, x_decoy, x_want, _ = sc.inputs(oracle, name, SEED_X)
    y = _head(name, sc.inputs(oracle, name, SEED_Y)[0], sc.N // 2)
    y_want = case.expect(oracle, y)
    _warm(torch, case, _to_dev(torch, cuda, x_decoy), s1, s2)
    dx, dy = _to_dev(torch, cuda, x), _to_dev(torch, cuda, y)
    with torch.cuda.stream(s2):                     # Y alone, warm: what it needs when nothing holds it
        alone = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        alone[0].record(s2)
        keep = case.run(dy, s2)
        alone[1].record(s2)
    torch.cuda.synchronize()
    y_ms = alone[0].elapsed_time(alone[1])
    del keep
    ev = stall(s1)
    out_x = case.run(dx, s1)
    out_y = case.run(dy, s2)
    end = time.perf_counter() + PIN_WAIT_MS / 1e3
    while time.perf_counter() < end and not s2.query():
        pass
    y_done, still = s2.query(), stalled(ev)
    got_x, got_y = _back(torch, out_x, s1), _back(torch, out_y, s2)   # both streams are drained before any assert
    print(f"{name}: Y alone {y_ms:.3f} ms on the device, given {PIN_WAIT_MS} ms")
    assert still, "the first stream's stall was over before the second call had had its time"
    assert y_ms * 10 < PIN_WAIT_MS, f"Y alone takes {y_ms:.3f} ms: {PIN_WAIT_MS} ms is no proof that it waited"
    assert not y_done, "the second stream ran ahead of the first call's use of the shared scratch"
    _compare(name + " (X)", got_x, x_want)
    _compare(name + " (Y)", got_y, y_want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ralledata.select_ralledata", "ralledata.partition_ralledata",
                                  "ralledata.ralledata_to_archive", "archive.fold_device", "archive.scan_device"])
def test_shared_scratch_concurrent_threads(cuda, oracle, name):
    """The launchers that synchronise their stream, called from four host threads at once, each
    on its own stream with inputs of its own size: every call returns its own inputs' result.
    This detector is probabilistic -- the calls have to overlap for a missing guard to show --
    where test_shared_scratch_pin_second_stream_waits_for_the_first is not."""
    import torch
    case = sc.BY_NAME[name]
    work = []
    for k, n in enumerate((sc.N, sc.N - 149, sc.N // 2, sc.N // 4 + 1)):
        d = _head(name, sc.inputs(oracle, name, 10 + k)[0], n) if n < sc.N else sc.inputs(oracle, name, 10 + k)[0]
        work.append((d, case.expect(oracle, d)))
    case.run(_to_dev(torch, cuda, work[0][0]), None)   # the largest first: the scratch is grown once
    torch.cuda.synchronize()

    def thread(k):
        d, want = work[k]
        s = torch.cuda.Stream(device=cuda)
        with torch.cuda.stream(s):
            dev = _to_dev(torch, cuda, d)
            for _ in range(4):
                out = case.run(dev, s)
                _compare(f"{name} thread {k}", _back(torch, out, s), want)
        return True

    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        assert all(ex.map(thread, range(4)))
