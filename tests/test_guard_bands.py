"""Every entry point through a guard arena: no write past a buffer, any alignment.

The tool is tests/guard_arena.py, the table of calls tests/guard_cases.py.  Three parts:

  controls   the tool itself, on the CPU and once on the GPU: carved addresses have the skew asked for, bands adjoin the buffer,
             and stand-ins with one planted defect each -- a write one element past either edge, an element left unwritten, a read
             one sample past the end that is used -- are reported, the first with the right offset.  Every deliberate out-of-range
             access is a torch access inside the arena's own allocation.
  cases      each case twice on the same inputs: on ordinary tensors, then with every caller-owned pointer carved, workspaces at
             exactly their documented minimum.  Same bits, bands intact, and for the FSST rows of tests/launch_cases.py the kernel
             that table records.  Then one pointer at a time off its 16-byte boundary: same bits again ((a) of guard_cases.py), or
             the stated refusal ((b), on the CPU).
  census     every pointer parameter of every hssfsst_* function of include/hssfsst.h has a case or an exemption of an allowed kind.

With HSS_GUARD_REPORT=<path> the GPU walk writes what ran, per subsystem, and its wall times there (profiles/guard_bands.txt)."""
import ctypes
import os
import re
import time

import numpy as np
import pytest
import torch

from tests import guard_arena as ga
from tests import guard_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- controls
def _past(view, k):
    """The ``view``'s storage ``k`` elements past its end (k >= 1) or before its start (k <= -1), as a one-element tensor: legal
    memory of the arena's allocation, outside the buffer."""
    n = view.numel()
    off = view.storage_offset() + (n + k - 1 if k > 0 else k)
    return torch.as_strided(view, (1,), (1,), off)


def _controls(device):
    arena = ga.GuardArena(device, capacity_bytes=4 << 20)
    # addresses and adjoining bands, every dtype and skew a case uses
    for dtype in (torch.uint8, torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int64, torch.complex64):
        es = ga.elem_size(dtype)
        for skew in range(0, 16, es):
            for kind in ("in", "out", "work"):
                data = torch.zeros(5, 3, dtype=dtype) if kind == "in" else None
                v = arena.carve((5, 3), dtype, skew, kind, f"{dtype} {kind} +{skew}", data)
                assert v.data_ptr() % 16 == skew and v.is_contiguous() and v.dtype == dtype and tuple(v.shape) == (5, 3)
                lo, hi = arena.bands()
                assert lo.numel() == hi.numel() == ga.BAND_BYTES
                assert lo.data_ptr() + ga.BAND_BYTES == v.data_ptr() and hi.data_ptr() == v.data_ptr() + 15 * es
                if kind != "in":
                    assert bool((v.reshape(-1).view(torch.uint8) == ga.FILL_BYTE).all())
                    if dtype.is_floating_point or dtype.is_complex:
                        assert not bool(torch.isfinite(torch.view_as_real(v) if dtype.is_complex else v.float()).any())
            arena.check()
            arena.reset()
    for bad in (1, 2, 3, 5, 16, -4):                     # not a multiple of 4 bytes, or outside 0 .. 15
        with pytest.raises(ValueError):
            arena.carve((4,), torch.float32, bad)
    with pytest.raises(ValueError):
        arena.carve((4,), torch.float64, 4)
    with pytest.raises(MemoryError):
        arena.carve((4 << 20,), torch.uint8)
    arena.reset()

    # an input's bands are NaN on the buffer's own element grid
    x = arena.carve((7,), torch.float32, 4, "in", "x", torch.arange(7.0))
    assert bool(torch.isnan(_past(x, 1)).all()) and bool(torch.isnan(_past(x, -1)).all()) and bool(torch.isnan(_past(x, 1000)).all())
    h = arena.carve((3,), torch.float16, 2, "in", "h", torch.ones(3, dtype=torch.float16))
    assert bool(torch.isnan(_past(h, 1)).all()) and bool(torch.isnan(_past(h, -7)).all())
    arena.check()
    arena.reset()

    # planted defect 1: one element written past either edge
    for dtype, skew in ((torch.float32, 0), (torch.float32, 4), (torch.float16, 2), (torch.uint8, 1)):
        es = ga.elem_size(dtype)
        for k, side, first in ((1, "high", 0), (-1, "low", -es), (3, "high", 2 * es), (-2, "low", -2 * es)):
            arena.carve((8,), torch.float32, 0, "out", "neighbour")
            out = arena.carve((11,), dtype, skew, "out", "victim")
            arena.carve((8,), torch.float32, 0, "work", "other neighbour")
            out.fill_(1)
            arena.check()
            _past(out, k).fill_(1)
            assert arena.damage() == [("victim", side, first, first + es - 1)]
            with pytest.raises(ga.GuardError, match=rf"victim: the {side} band, bytes {first} \.\. {first + es - 1} relative to the buffer's "
                                                     + ("end" if side == "high" else "start")):
                arena.check()
            arena.reset()
    # ... and a stray store far from the edge, still inside the band, with a second one: first and last are both named
    out = arena.carve((16,), torch.float32, 0, "out", "victim")
    hi = arena.bands()[1]
    hi[12288] = 0
    hi[ga.BAND_BYTES - 1] = 0
    assert arena.damage() == [("victim", "high", 12288, ga.BAND_BYTES - 1)]
    arena.reset()

    # planted defect 2: one element left unwritten
    want = torch.arange(24.0, device=device).reshape(2, 12)
    out = arena.carve((2, 12), torch.float32, 8, "out", "out")
    out.copy_(want)
    ga.same_bits("control", out, want)
    out = arena.carve((2, 12), torch.float32, 8, "out", "out")
    out.reshape(-1)[:17].copy_(want.reshape(-1)[:17])
    out.reshape(-1)[18:].copy_(want.reshape(-1)[18:])
    with pytest.raises(ga.GuardError, match=r"1 of 24 elements differ from the plain call, the first at flat index 17 \(last 17\); 1 of them still hold"):
        ga.same_bits("control", out, want)
    arena.check()
    arena.reset()

    # planted defect 3: a stand-in that reads one sample past the end and uses it.  y[i] = x[i] + x[i + 1], x[n] := 0
    def smooth(x, out, overread):
        n = x.numel()
        nxt = torch.as_strided(x, (n,), (1,), x.storage_offset() + 1) if overread else torch.cat([x[1:], x.new_zeros(1)])
        out.copy_(x + nxt)

    X = torch.arange(1.0, 10.0)
    plain_x, plain_y = torch.cat([X, torch.zeros(1)]).to(device)[:9], torch.empty(9, device=device)      # (its slack holds a 0)
    smooth(plain_x, plain_y, True)                       # on plain tensors the over-read meets slack and nothing shows
    good = torch.empty(9, device=device)
    smooth(plain_x, good, False)
    ga.same_bits("control", plain_y, good)
    x, y = arena.carve((9,), torch.float32, 0, "in", "x", X), arena.carve((9,), torch.float32, 0, "out", "y")
    smooth(x, y, False)
    ga.same_bits("control", y, good)
    smooth(x, y, True)
    with pytest.raises(ga.GuardError, match=r"1 of 9 elements differ from the plain call, the first at flat index 8 "):
        ga.same_bits("control", y, good)
    arena.check()


def test_the_arena_reports_three_planted_defects():
    _controls("cpu")


@pytest.mark.gpu
def test_the_arena_reports_three_planted_defects_on_the_device():
    _controls("cuda")


def test_allocators_hand_out_the_same_buffers_on_the_cpu():
    """The two allocators of guard_cases.py, without a device: same shapes and dtypes, a skew where asked, the prefill."""
    host = ga.GuardArena("cpu", capacity_bytes=2 << 20)
    for A in (gc.Plain("cpu"), gc.Carved(None, host, skew={"x": gc.ELEM, "out": 8})):
        x = A.inp("x", torch.arange(6, dtype=torch.float16), host=True)
        out = A.out("out", (2, 3), torch.float32, host=True)
        w = A.work("w", (5,), torch.uint8, host=True)
        assert x.dtype == torch.float16 and torch.equal(x, torch.arange(6, dtype=torch.float16)) and tuple(out.shape) == (2, 3)
        assert bool(torch.isnan(out).all()) and bool((w == ga.FILL_BYTE).all())
        if A.carved:
            assert x.data_ptr() % 16 == 2 and out.data_ptr() % 16 == 8 and w.data_ptr() % 16 == 0
    host.check()


# ---------------------------------------------------------------------------------------------------- the walk
_REPORT = {"lines": [], "cases": {}, "t0": None}


def _write_report():
    path = os.environ.get("HSS_GUARD_REPORT")
    if not path:
        return
    per = {}
    for name, rec in _REPORT["cases"].items():
        s = per.setdefault(rec["subsystem"], {"cases": 0, "combos": set(), "variants": 0, "secs": 0.0})
        s["cases"] += 1
        s["variants"] += rec["variants"]
        s["secs"] += rec["secs"]
        s["combos"] |= rec["combos"]
    lines = ["guard-band walk (tests/test_guard_bands.py -m gpu), per subsystem: cases, calls through the arena, distinct (entry, pointer, skew) combinations, wall time"]
    for sub, s in per.items():
        lines.append(f"  {sub}: {s['cases']} cases, {s['variants']} carved calls, {len(s['combos'])} (entry, pointer, skew) combinations, {s['secs']:.2f} s")
    slow = max(_REPORT["cases"].items(), key=lambda kv: kv[1]["secs"], default=None)
    total = sum(r["secs"] for r in _REPORT["cases"].values())
    lines.append(f"  all: {len(_REPORT['cases'])} cases, {sum(r['variants'] for r in _REPORT['cases'].values())} carved calls, {total:.2f} s"
                 + (f"; the slowest case is '{slow[0]}' with {slow[1]['secs']:.2f} s" if slow else ""))
    lines += _REPORT["lines"]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


@pytest.fixture(scope="module")
def arenas():
    dev = ga.GuardArena("cuda", capacity_bytes=gc.DEV_CAPACITY)
    host = ga.GuardArena("cpu", capacity_bytes=gc.HOST_CAPACITY)
    pin = ga.GuardArena("cpu", capacity_bytes=2 << 20, pinned=True)
    return dev, host, pin


def _run_case(case, dev, host, pin, device):
    """The plain call, then every variant through the arenas -> the number of carved calls."""
    sync = torch.cuda.synchronize if device != "cpu" else (lambda: None)
    ctx = case.make()
    want = case.call(ctx, gc.Plain(device))
    sync()
    want = {k: v.clone() for k, v in want.items()}
    if case.python:
        ref = case.python(ctx)
        sync()
        for k, v in ref.items():
            ga.same_bits(f"{case.name}: {k} of the plain C call against the package's entry point", want[k], v)
    combos = set()
    variants = case.variants()
    for label, skew in variants:
        A = gc.Carved(dev, host, pin, skew)
        A.reset()
        got = case.call(ctx, A)
        sync()
        assert set(got) == set(want)
        # the variant is what its label says: the named buffer sits off its boundary every time it is carved, every other one on it
        for name, at in A.placed:
            assert (at != 0) == (name in skew), (case.name, label, name, at)
        assert all(any(n == name for n, _ in A.placed) for name in skew), (case.name, label)
        for k in want:
            ga.same_bits(f"{case.name} [{label}]: {k}", got[k], want[k])
        for arena in A.arenas():
            arena.check()
        if label == "aligned" and case.kernel:
            name = case.kernel(ctx)
            assert name.split(" [")[0] == case.kernel_is, (case.name, name, case.kernel_is)
        for entry, params in case.covers.items():
            for p in params:
                s = skew.get(p)
                combos.add((entry, p, "aligned" if s is None else str(s)))
    return len(variants), combos


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in gc.CASES if c.gpu], ids=lambda c: c.name)
def test_carved_call_has_the_plain_call_bits_and_intact_bands(case, arenas, built_lib):
    dev, host, pin = arenas
    t0 = time.perf_counter()
    n, combos = _run_case(case, dev, host, pin, "cuda")
    _REPORT["cases"][case.name] = {"subsystem": case.subsystem, "variants": n, "secs": time.perf_counter() - t0, "combos": combos}
    _write_report()


@pytest.mark.parametrize("case", [c for c in gc.CASES if not c.gpu], ids=lambda c: c.name)
def test_host_only_case_through_the_host_arena(case, built_lib):
    host = ga.GuardArena("cpu", capacity_bytes=2 << 20)
    _run_case(case, None, host, None, "cpu")


# ---------------------------------------------------------------------------------------------------- (b): the refusals
@pytest.mark.parametrize("r", gc.REFUSALS, ids=lambda r: f"{r['entry']}:{r['name']}")
def test_stated_alignment_is_refused_before_any_device_work(r, built_lib):
    """A pointer the header holds to 16 bytes, one float off: HSSFSST_EINVAL and the text that names it.  Every address is fake and
    the plan is never looked at: the check stands before the first use of the plan or a device."""
    L = built_lib
    args = list(r["args"])
    args[r["index"]] = gc.ODD
    rc = getattr(L, r["entry"])(*args)
    assert rc == -1, (r["entry"], rc)
    assert L.hssfsst_last_error().decode() == r["text"]
    args[r["index"]] = gc.FAKE + 8                       # 8 bytes are not enough either
    assert getattr(L, r["entry"])(*args) == -1 and L.hssfsst_last_error().decode() == r["text"]


def test_refusals_are_stated_in_the_header():
    with open(os.path.join(ROOT, "include", "hssfsst.h")) as fh:
        text = fh.read()
    for r in gc.REFUSALS:
        decl = text.index(f"int {r['entry']}(")
        comment = text[text.rfind("/*", 0, decl):decl]
        assert re.search(rf"{r['name']}\b[^.]*16-byte aligned", comment) or re.search(rf"16-byte aligned[^.]*\b{r['name']}\b", comment), \
            (r["entry"], r["name"])


# ---------------------------------------------------------------------------------------------------- the census
_PLAN_TYPES = ("hssfsst_plan", "hssfsst_resample_plan", "hssfsst_segmenter", "hssfsst_bilstm")


def header_pointer_parameters():
    """[(function, parameter, its declared type)] for every pointer or array parameter of every hssfsst_* function of the header."""
    with open(os.path.join(ROOT, "include", "hssfsst.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    out = []
    for m in re.finditer(r"\b(hssfsst_\w+)\s*\(([^()]*)\)\s*;", text):
        fn, params = m.group(1), " ".join(m.group(2).split())
        if params in ("", "void"):
            continue
        for p in params.split(","):
            p = p.strip()
            name = re.search(r"(\w+)\s*(\[\d*\])?$", p)
            assert name, (fn, p)
            if "*" in p or name.group(2):
                out.append((fn, name.group(1), p[:name.start(1)].strip() + (name.group(2) or "")))
    return out


def _exemption(fn, name, ctype):
    """The reason (fn, name) needs no case, or None."""
    if any(re.fullmatch(rf"(const )?{t}\s?\*\*?", ctype) for t in _PLAN_TYPES):
        return gc.HANDLE
    if name in ("stream", "nccl_comm") and ctype == "void*":
        return gc.STREAM
    if fn.endswith("_info"):
        return gc.SCALAR
    return gc.EXEMPT.get((fn, name))


def test_every_device_pointer_has_a_guard_case():
    params = header_pointer_parameters()
    fns = {fn for fn, _, _ in params}
    assert len(params) > 150 and {"hssfsst_exec", "hssfsst_stitch_windows", "hssfsst_bilstm_backward_ragged", "hssfsst_plan_timing"} <= fns
    covered = {(entry, p) for c in gc.CASES for entry, ps in c.covers.items() for p in ps}
    missing, both = [], []
    for fn, name, ctype in params:
        reason = _exemption(fn, name, ctype)
        if reason is not None:
            assert reason in gc.ALLOWED_REASONS, (fn, name, reason)
            if (fn, name) in covered:
                both.append((fn, name))
        elif (fn, name) not in covered:
            missing.append(f"{fn}({ctype} {name})")
    assert not missing, "pointer parameters without a guard case or an exemption: " + ", ".join(missing)
    assert not both, f"exempt and covered at once: {both}"
    declared = {(fn, name) for fn, name, _ in params}
    stale = sorted(covered - declared) + sorted(set(gc.EXEMPT) - declared)
    assert not stale, f"cases or exemptions that name no parameter of the header: {stale}"
    # (b) pointers are stated ones: each is a parameter, and none of them is skewed by a case
    for entry, names in list(gc.STATED.items()) + [(r["entry"], (r["name"],)) for r in gc.REFUSALS]:
        for n in names:
            assert (entry, n) in declared, (entry, n)
            for c in gc.CASES:
                if entry in c.covers:
                    assert n not in c.inputs + c.outputs, (c.name, n)


def test_every_case_skews_only_buffers_it_carves():
    """A name in ``inputs`` / ``outputs`` that no carve uses would make its variant a second aligned run."""
    import inspect
    for c in gc.CASES:
        src = inspect.getsource(c.call)
        helpers = "".join(inspect.getsource(f) for f in (gc._segmenter_plan, gc._bilstm_plan, gc._pointer_table))
        for n in c.inputs + c.outputs:
            assert f'"{n}"' in src or f'"{n}"' in helpers or n in gc._BILSTM_W, (c.name, n)
