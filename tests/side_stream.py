"""Helpers that make a stage enqueued on the wrong stream visible, deterministically.  No tests here: tests/test_stream_order.py
holds the cases and the controls.

Every exec entry point of include/hssfsst.h takes a stream and promises to enqueue all of its work there.  On the default stream
a stage that strayed to stream 0 changes nothing, so the suite cannot see it.  Two scenarios can:

A, the side stream held.  The input buffer is filled with poison on the side stream, a device-side busy wait (``torch.cuda._sleep``:
   one wave, so a kernel that needs every CU still gets them) is enqueued there, then the copy of the real input, then the call.
   A call that does not block must have returned while the wait is still running (``not end.query()``): every stage was enqueued
   before the real input existed, and one that strayed to another stream ran on poison, or wrote before the rest and was
   overwritten.
B, the null stream held.  The wait runs on stream 0, the call on the side stream; every output is cloned on the side stream, the side
   stream is synchronised, and the wait must STILL be running: the whole result was produced without stream 0.  A stage that
   strayed there has not run yet and the clone misses it.  B needs warmed plans: creating a plan uploads tables with a
   synchronous copy and growing a buffer frees memory, and both wait for stream 0 by right.

The expected value is the same call on the default stream, synchronised, on a context of its own: all outputs bit for bit.
A context is warmed on DIFFERENT data first (under the stream it will run on), so that blocks the caching allocator hands out
again hold a wrong answer, and ``out=`` tensors are filled with NaN before the wait.

How long the wait is: 4 x the host wall time of the same call on the idle default stream (that time bounds the enqueue time and,
for B, the whole call from above; 4 covers host jitter), at least DEFAULT_DELAY_S, and a case that would need more than
MAX_DELAY_S fails: its shape is to be split down, not the module lengthened.  ``torch.cuda._sleep`` counts cycles of a clock whose
rate is measured once per session with events on the idle device.

Whether a ``torch.cuda.Stream()`` and stream 0 run side by side at all is probed once per session (``streams``): at most 8 fresh
streams are tried, each in both directions; if none is independent every caller fails with that message.

With HSS_STREAM_ORDER_REPORT=<path> a record of the session (calibration, probe, per-case default-stream times, what the controls
reported) is written there (profiles/stream_order.txt)."""
import contextlib
import os
import time

import numpy as np
import torch

DEFAULT_DELAY_S = 0.03
MAX_DELAY_S = 0.25
MAX_STREAMS = 8

_S = {}                                                  # the session: cycles per ms, streams, expected values, the record
_LINES = []


class StreamOrderError(AssertionError):
    """What a scenario raises: the message says which scenario, which case and what was seen."""


# ------------------------------------------------------------------------------------------------ the record
def report(line):
    _LINES.append(line)
    path = os.environ.get("HSS_STREAM_ORDER_REPORT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(_LINES) + "\n")


def _clock():
    _S.setdefault("t0", time.perf_counter())
    return time.perf_counter() - _S["t0"]


# ------------------------------------------------------------------------------------------------ the delay
def _null():
    return torch.cuda.default_stream()


def _sleep_ms(cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(int(cycles))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate():
    """Cycles of ``torch.cuda._sleep`` per millisecond, measured once with events on the idle device."""
    if "cycles_per_ms" in _S:
        return _S["cycles_per_ms"]
    _clock()
    torch.cuda.synchronize()
    _sleep_ms(1000)                                      # (the first launch loads the kernel: not measured)
    cycles = 1_000_000
    ms = _sleep_ms(cycles)
    while ms < 2.0 and cycles < (1 << 40):               # long enough that launch overhead does not count
        cycles *= 8
        ms = _sleep_ms(cycles)
    ms = min(ms, _sleep_ms(cycles))                      # (the shorter of two: the delay then errs on the long side)
    _S["cycles_per_ms"] = cycles / ms
    check = _sleep_ms(DEFAULT_DELAY_S * 1e3 * _S["cycles_per_ms"])
    report(f"calibration: torch.cuda._sleep({cycles}) took {ms:.3f} ms -> {_S['cycles_per_ms']:.0f} cycles per ms; "
           f"a {DEFAULT_DELAY_S * 1e3:.0f} ms delay measured {check:.2f} ms")
    if not 0.8 * DEFAULT_DELAY_S * 1e3 <= check <= 2.0 * DEFAULT_DELAY_S * 1e3:
        raise StreamOrderError(f"the delay is not linear in its cycles: asked for {DEFAULT_DELAY_S * 1e3:.0f} ms, measured {check:.2f} ms")
    return _S["cycles_per_ms"]


def delay(stream, seconds):
    """A busy wait of ``seconds`` enqueued on ``stream`` -> the event recorded behind it."""
    cycles = int(seconds * 1e3 * calibrate())
    end = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        end.record(stream)
    return end


def delay_for(name, wall_s):
    secs = max(DEFAULT_DELAY_S, 4.0 * wall_s)
    if secs > MAX_DELAY_S:
        raise StreamOrderError(f"{name}: the call takes {wall_s * 1e3:.1f} ms on the idle default stream, so its delay would be "
                               f"{secs * 1e3:.0f} ms, over the limit of {MAX_DELAY_S * 1e3:.0f} ms: split the case's shape down")
    return secs


# ------------------------------------------------------------------------------------------------ the probe
def _runs_beside(held, other):
    """With a delay running on ``held``, does a trivial op on ``other`` complete while the delay's end is still pending?"""
    with torch.cuda.stream(other):
        t = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    end = delay(held, DEFAULT_DELAY_S)
    done = torch.cuda.Event()
    with torch.cuda.stream(other):
        t.add_(1.0)
        done.record(other)
    while not done.query() and not end.query():          # (bounded by the delay itself)
        pass
    ok = done.query() and not end.query()
    torch.cuda.synchronize()
    return bool(ok)


def streams():
    """(side, second side): streams that run independently of stream 0, found by trying at most MAX_STREAMS fresh ones.  The second
    is a further independent one when there is one, else just another stream (the hand-over cases need no independence of it)."""
    if "streams" in _S:
        if isinstance(_S["streams"], str):
            raise StreamOrderError(_S["streams"])
        return _S["streams"]
    calibrate()
    found, others, tried = [], [], 0
    while tried < MAX_STREAMS and len(found) < 2:
        s = torch.cuda.Stream()
        tried += 1
        if _runs_beside(_null(), s) and _runs_beside(s, _null()):
            found.append(s)
        else:
            others.append(s)
    report(f"probe: {tried} fresh streams tried, {len(found)} independent of stream 0 in both directions"
           f" (GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')})")
    if not found:
        _S["streams"] = (f"none of {tried} fresh torch.cuda.Stream() objects runs independently of stream 0 on this device: "
                         "a held stream holds every other one, and neither scenario can show anything")
        raise StreamOrderError(_S["streams"])
    second = found[1] if len(found) > 1 else (others[0] if others else torch.cuda.Stream())
    _S["streams"] = (found[0], second)
    return _S["streams"]


# ------------------------------------------------------------------------------------------------ results
def flatten(res):
    """Every tensor of a result, in a fixed order: tensors, numpy arrays, sequences, RaggedFeatures (arena, scores), the items of
    the corpus builders (features, labels)."""
    if res is None:
        return []
    if isinstance(res, torch.Tensor):
        return [res]
    if isinstance(res, np.ndarray):
        return [torch.from_numpy(np.ascontiguousarray(res))]
    if isinstance(res, (float, int)):
        return [torch.tensor(res)]
    if isinstance(res, dict):
        return [t for k in sorted(res) for t in flatten(res[k])]
    if hasattr(res, "data") and hasattr(res, "_off"):    # RaggedFeatures / RaggedStates
        return [res.data] + flatten(getattr(res, "scores", None))
    if hasattr(res, "features") and hasattr(res, "labels"):
        return flatten(res.features) + flatten(res.labels)
    if isinstance(res, (list, tuple)):
        return [t for r in res for t in flatten(r)]
    raise TypeError(f"side_stream.flatten: {type(res)}")


def bits(t):
    t = t.detach()
    if t.is_complex():
        t = torch.view_as_real(t)
    return (tuple(t.shape), str(t.dtype), t.cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())


def _compare(what, got, want):
    if len(got) != len(want):
        raise StreamOrderError(f"{what}: {len(got)} outputs, the default stream gave {len(want)}")
    for i, (g, w) in enumerate(zip(got, want)):
        if g[:2] != w[:2]:
            raise StreamOrderError(f"{what}: output {i} is {g[:2]}, the default stream gave {w[:2]}")
        if g[2] != w[2]:
            a, b = np.frombuffer(g[2], dtype=np.uint8), np.frombuffer(w[2], dtype=np.uint8)
            raise StreamOrderError(f"{what}: output {i} {g[:2]} differs from the default-stream result in {int((a != b).sum())} of {a.size} bytes")


# ------------------------------------------------------------------------------------------------ a case
class Case:
    """One call under test.
    name      unique
    covers    the C entry points with a ``stream`` parameter the call reaches
    sites     the package's functions that read ``torch.cuda.current_stream`` on its way, as "module:Qualified.name"
    inputs    seed -> list of HOST tensors, the device inputs of the call (seed 0: the data of the case, seed 1: the warm-up's)
    context   () -> the plans / modules of one run, fresh and deterministic; ``call`` may change them
    call      (context, list of device inputs, out) -> result (anything ``flatten`` takes), on the current stream
    out       (context, device inputs) -> the tensor handed to the call's ``out=``, or None
    reset     (context) -> puts a warmed context back to its first state (stateful ones)
    check     (result, host inputs) -> the family's float64 check, run on the default-stream result
    after     (context, what) -> a further assertion on the context after every run (e.g. which kernel ran)
    poison    what the input holds before the real data: NaN for floats unless given, 0 for integers
    blocking  the call ends in a host wait (host outputs): no query() assertion in A
    scenarios "AB" or "A"; warm: False for the cold-plan case (A only)
    host      the inputs stay on the host and go to the call as they are (nothing to poison or delay: the held stream is the test)"""

    def __init__(self, name, covers, sites, inputs, call, context=lambda: None, out=None, reset=None, check=None, after=None,
                 poison=None, blocking=False, scenarios="AB", warm=True, why_not_b=None, host=False):
        self.name, self.covers, self.sites = name, frozenset(covers), frozenset(sites)
        self.inputs, self.call, self.context, self.out, self.reset, self.check, self.after = inputs, call, context, out, reset, check, after
        self.poison, self.blocking, self.scenarios, self.warm, self.why_not_b = poison, blocking, scenarios, warm, why_not_b
        self.host = host
        assert scenarios in ("AB", "A") and (scenarios == "AB" or why_not_b), name
        assert warm or scenarios == "A", name

    def __repr__(self):
        return self.name


def _poison(case, t):
    if case.poison is not None:
        return case.poison
    return float("nan") if (t.is_floating_point() or t.is_complex()) else 0


def _upload(case, ts):
    return list(ts) if case.host else [t.cuda() for t in ts]


def _fill_out(out):
    if out is not None:
        out.fill_(float("nan") if (out.is_floating_point() or out.is_complex()) else -1)


def _prepare(case, stream):
    """A context for ``case``: made, warmed on other data and put back, all under ``stream`` (None: the default), synchronised."""
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        ctx = case.context()
        if case.warm:
            xs = _upload(case, case.inputs(1))
            res = case.call(ctx, xs, case.out(ctx, xs) if case.out else None)
            torch.cuda.synchronize()
            del res, xs
            if case.reset:
                case.reset(ctx)
    torch.cuda.synchronize()
    return ctx


def expected(case):
    """The case on the default stream, synchronised, on a context of its own -> {"bits", "wall"}; computed once per session."""
    E = _S.setdefault("expected", {})
    if case.name in E:
        return E[case.name]
    streams()
    ctx = _prepare(case, None)
    host = case.inputs(0)
    xs = _upload(case, host)
    out = case.out(ctx, xs) if case.out else None
    _fill_out(out)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = case.call(ctx, xs, out)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    if case.after:
        case.after(ctx, f"{case.name} (default stream)")
    if case.check:
        case.check(res, host)
    flat = flatten(res)
    E[case.name] = {"bits": [bits(t) for t in flat], "wall": wall, "keep": (flat, xs, out)}
    report(f"case {case.name}: {wall * 1e3:.2f} ms on the idle default stream ({'blocking' if case.blocking else 'not blocking'}, "
           f"scenarios {case.scenarios}{', float64 check passed' if case.check else ''})")
    return E[case.name]


def scenario_a(case, side=None):
    """The side stream held behind the call's input.  Raises StreamOrderError on any difference."""
    exp = expected(case)
    side = side or streams()[0]
    what = f"scenario A (side stream held), {case.name}"
    ctx = _prepare(case, side) if case.warm else None
    real = _upload(case, case.inputs(0))
    torch.cuda.synchronize()
    secs = delay_for(case.name, exp["wall"])
    with torch.cuda.stream(side):
        if ctx is None:
            ctx = case.context()
        bufs = list(real) if case.host else [torch.empty_like(t) for t in real]
        for b in ([] if case.host else bufs):
            b.fill_(_poison(case, b))
        out = case.out(ctx, bufs) if case.out else None
        _fill_out(out)
        end = delay(side, secs)
        for b, t in ([] if case.host else zip(bufs, real)):
            b.copy_(t, non_blocking=True)
        res = case.call(ctx, bufs, out)
        in_time = not end.query()
    side.synchronize()
    torch.cuda.synchronize()
    _clock()
    if not case.blocking and not in_time:
        raise StreamOrderError(f"{what}: the {secs * 1e3:.0f} ms delay had ended before the call returned: the call waited for the "
                               "device, or enqueueing took longer than 4 x the whole call on an idle stream")
    if case.after:
        case.after(ctx, what)
    _compare(what, [bits(t) for t in flatten(res)], exp["bits"])


def scenario_b(case, side=None):
    """The null stream held; the call and the snapshot of its outputs on the side stream.  Raises StreamOrderError."""
    assert "B" in case.scenarios, case.name
    exp = expected(case)
    side = side or streams()[0]
    what = f"scenario B (null stream held), {case.name}"
    ctx = _prepare(case, side)
    with torch.cuda.stream(side):
        xs = _upload(case, case.inputs(0))
        out = case.out(ctx, xs) if case.out else None
        _fill_out(out)
    torch.cuda.synchronize()
    secs = delay_for(case.name, exp["wall"])
    end = delay(_null(), secs)
    with torch.cuda.stream(side):
        res = case.call(ctx, xs, out)
        snap = [t.clone() for t in flatten(res)]
        side.synchronize()
    pending = not end.query()
    torch.cuda.synchronize()
    _clock()
    if not pending:
        raise StreamOrderError(f"{what}: the {secs * 1e3:.0f} ms delay on stream 0 had ended when the side stream was through: the call "
                               "waited for stream 0, or took longer than 4 x its time on an idle stream")
    if case.after:
        case.after(ctx, what)
    _compare(what, [bits(t) for t in snap], exp["bits"])


def finish():
    """The last line of the record: the time from the first calibration to the last scenario of the session."""
    if "t0" in _S:
        report(f"total: {_clock():.1f} s from the calibration to the end of the last scenario, {len(_S.get('expected', {}))} cases")
