"""Stalls and stream pairs for the tests that pin where and when device work runs
(test_stream_contract.py).

stall(stream) queues a delay on a stream and returns an event recorded right behind it;
stalled(ev) says whether that delay is still running.  A test that relies on a stall asserts
stalled(ev) at the point where it relies on it, so a stall that is too short fails the test
instead of letting it pass vacuously: the stall's length is never a pass criterion.

independent_streams(device) hands out two streams the hardware really runs side by side.  A
process has a handful of hardware queues and two torch streams can share one; a stalled stream
then holds the other one up, and a test that expects the second to proceed would fail for no
fault of the project.  So the pair is probed, in both directions, before it is handed out.
"""
import time

import pytest

# The delay one stall queues.  What runs on the host while a stall is relied on is one warm
# call and the read-back of its outputs: 0.01 - 0.04 ms for the asynchronous entry points,
# 0.05 - 0.4 ms for the synchronising and composite ones on the other stream (compact_device,
# route_ralledata and import_file_to_archive are the slowest) as measured on an MI355X, so
# this is more than a hundred times the slowest of them, and well under a second: a delay,
# not a hang.  test_late_inputs and test_busy_current_stream print each call's host time.
STALL_MS = 60.0
CANDIDATES = 12          # streams independent_streams tries before it gives up
_PROBE_CYCLES = 4_000_000
_PROBE_STALL_MS = 40.0   # the stream probe's own stalls: one tiny op has to finish beside them
_MATMUL_N = 2048

_unit = {}               # device index -> ("sleep", cycles per ms) or ("matmul", ms per matmul, a, b)
_pairs = {}              # device index -> (c, s)
_report = {}             # what calibration and the probe saw, for the record


def report():
    """What the calibration and the stream probe observed (for logs and the summary)."""
    return dict(_report, stall_ms=STALL_MS)


def _timed(torch, stream, queue):
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        b.record(stream)
        queue()
        e.record(stream)
    e.synchronize()
    return b.elapsed_time(e)


def _calibrate(torch, stream):
    dev = stream.device.index
    if dev in _unit:
        return _unit[dev]
    _timed(torch, stream, lambda: torch.cuda._sleep(1000))   # first launch of the kernel
    ms = _timed(torch, stream, lambda: torch.cuda._sleep(_PROBE_CYCLES))
    if ms >= 0.5:
        _unit[dev] = ("sleep", _PROBE_CYCLES / ms)
        _report["stall_unit"] = "torch.cuda._sleep, %.0f cycles per ms" % (_PROBE_CYCLES / ms)
        return _unit[dev]
    # _sleep does not hold the queue here: a chain of matmuls, timed the same way
    with torch.cuda.stream(stream):
        a = torch.ones((_MATMUL_N, _MATMUL_N), device=stream.device)
        b = torch.empty_like(a)
        torch.mm(a, a, out=b)

    def chain():
        for _ in range(8):
            torch.mm(a, a, out=b)
    per = _timed(torch, stream, chain) / 8
    _unit[dev] = ("matmul", per, a, b)
    _report["stall_unit"] = "%d^2 fp32 matmul, %.3f ms each (_sleep of %d cycles took %.3f ms)" % (
        _MATMUL_N, per, _PROBE_CYCLES, ms)
    return _unit[dev]


def stall(stream, ms=STALL_MS):
    """Queue a delay of about `ms` on `stream`; returns an event recorded right after it."""
    import torch
    unit = _calibrate(torch, stream)
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        if unit[0] == "sleep":
            torch.cuda._sleep(int(unit[1] * ms))
        else:
            _kind, per, a, b = unit
            for _ in range(max(1, int(ms / per + 0.5))):
                torch.mm(a, a, out=b)
        ev.record(stream)
    return ev


def stalled(ev):
    """The delay in front of `ev` has not run out yet."""
    return not ev.query()


def _proceeds_beside(torch, held, free):
    """Work on `free` finishes while `held` is stalled."""
    ev = stall(held, _PROBE_STALL_MS)
    with torch.cuda.stream(free):
        t = torch.zeros(64, device=free.device) + 1
    free.synchronize()
    ok = stalled(ev)
    held.synchronize()
    del t
    return ok


def independent_streams(device):
    """(c, s): two torch streams of `device` that run side by side, each while the other is
    stalled.  Cached; pytest.fail when no such pair is found among CANDIDATES streams."""
    import torch
    dev = torch.device(device).index or 0
    if dev in _pairs:
        return _pairs[dev]
    tried = [torch.cuda.Stream(device=device)]
    _calibrate(torch, tried[0])
    skipped = 0
    while len(tried) < CANDIDATES:
        s = torch.cuda.Stream(device=device)
        for c in tried:
            if c.cuda_stream != s.cuda_stream and _proceeds_beside(torch, c, s) and _proceeds_beside(torch, s, c):
                _pairs[dev] = (c, s)
                _report["probe_skipped"] = skipped
                return c, s
            skipped += 1
        tried.append(s)
    _report["probe_skipped"] = skipped
    pytest.fail("no two of %d torch streams ran side by side on %s: every pair shared a hardware queue, so a "
                "stalled stream holds every other one up and the stream tests cannot tell the project's streams "
                "apart (the process has too few hardware queues; this is no fault of the wrappers)" % (CANDIDATES, device))


def host_ms(fn):
    """Wall time of one host call, in ms."""
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3
