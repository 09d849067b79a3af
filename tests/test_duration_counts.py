"""Expected run-length counts under the explicit-duration (semi-Markov) model -- the sufficient statistic of the duration tables:
hssfsst_posteriors_durations_counts (C ABI), consumer.duration_posteriors(return_counts=True),
consumer.duration_nll(learn_durations=True), consumer.durations_from_counts.

The contract is csrc/duration_counts_layout.hpp's arithmetic restated in numpy in tests/duration_count_cases.py (vectorised over t,
so equal to rounding, not bit for bit).  CPU tests check the restatement itself (brute-force enumeration of every segmentation,
five identities, float64 autograd of logZ in the two tables, an 80-bit log-space twin), the ABI, the argument errors (all raised
before any device work), both kernels with their lanes simulated under sanitizers (tests/native/duration_counts_check.cpp) and the
shipped kernels' resources.  Every GPU comparison is with the restatement or a CPU twin, never with the code under test; the first
seven outputs of the new entry are compared bit for bit with hssfsst_posteriors_durations' on the same input.

Gates.  counts: 8 x the largest difference MEASURED between the restatement and the 80-bit twin over T in {3000, 6000} x
D in {300, 2048} on tests/test_duration_posteriors.py's emissions (log_softmax of N(0, 30^2) logits) and models, which was
    counts 6.86e-11        (T 6000, D 300; the other three: 2.19e-11 at T 3000 D 300, 3.11e-12 at T 3000 D 2048, 3.6e-11 at T 6000 D 2048)
absolute, where the largest count is 858 and they sum to 3754 (the error grows with the emissions' prefix sums, |E_j(T)| x 2^-53:
|E| reaches ~4e5 there).  The gradients of
duration_nll: 1e-4 of each tensor's maximum, the project's gradient gate."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, consumer, synth
from heart_sounds_segmentation_amd.consumer import (HipSegmenterHead, SegmenterHead, duration_nll, duration_posteriors, durations_from_counts,
                                                    edge_durations)
from heart_sounds_segmentation_amd.transforms import FSST, RaggedFeatures
from tests import decode_cases as dc
from tests import duration_cases as duc
from tests import duration_count_cases as dcc
from tests import duration_posterior_cases as dpc
from tests import test_duration_posteriors as tdp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hssfsst.h")
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")
NINF = float("-inf")
I64P = ctypes.POINTER(ctypes.c_int64)
COUNTS_GATE = 8 * 6.86e-11
PARENT_SWEEP = dict(vgpr_count=256, group_segment_fixed_size=131760, private_segment_fixed_size=0)     # read on the parent commit
NEW_KERNELS = ("seg_duration_runs_sweep_kernel", "seg_duration_run_counts_kernel")
OLD_MATCHES = ("seg_duration_posteriors_kernel", "seg_duration_posteriors_fill_kernel", "seg_decode_durations_kernel", "seg_durations_fill_kernel",
               "seg_decode_kernel", "seg_posteriors_kernel", "seg_rec_kernel", "seg_bwd_rec_kernel")


def counts_info(lib):
    per, rec, dur, grp = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
    assert lib.hssfsst_posteriors_durations_counts_info(ctypes.byref(per), ctypes.byref(rec), ctypes.byref(dur), ctypes.byref(grp)) == 0
    return per.value, rec.value, dur.value, grp.value


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_library_and_info(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    assert "int hssfsst_posteriors_durations_counts(" in text and "int hssfsst_posteriors_durations_counts_info(" in text
    fn, old = built_lib.hssfsst_posteriors_durations_counts, built_lib.hssfsst_posteriors_durations
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 19 and len(old.argtypes) == 18
    assert list(fn.argtypes[:14]) == list(old.argtypes[:14]) and list(fn.argtypes[15:]) == list(old.argtypes[14:])
    assert fn.argtypes[14] is ctypes.c_void_p                                             # counts, before work
    per, rec, dur, grp = counts_info(built_lib)
    assert built_lib.hssfsst_posteriors_durations_counts_info(None, None, None, None) == 0
    assert consumer.duration_counts_info() == (per, rec, dur, grp) == (97, 48, 96, 128)
    assert tdp.info(built_lib)[3:] == (49, 32, 96)                                        # the plain entry's factors stay
    with open(os.path.join(CSRC, "duration_counts_layout.hpp")) as fh:
        layout = fh.read()
    assert "constexpr i64 kGBytesPerStep = 48;" in layout and "constexpr i64 kInvzBytesPerRecording = 16;" in layout
    assert "constexpr int kDurationsPerGroup = kLanes / 4;" in layout and '#include "duration_posterior_layout.hpp"' in layout
    import heart_sounds_segmentation_amd as pkg
    for name in ("durations_from_counts", "duration_counts_info"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(consumer, name)
    for name in NEW_KERNELS:
        assert not any(m in name for m in OLD_MATCHES), name


@pytest.mark.parametrize("kind", dc.KINDS)
def test_restatement_equals_brute_force(kind):
    """Every segmentation enumerated (T <= 7, D in {1, 2, 3, 4, 7}), random tables with 30 % forbidden entries: the counts to 1e-12,
    and sum counts[1] = 2 - P(one run)."""
    rng = np.random.default_rng(71)
    worst = 0.0
    for D in (1, 2, 3, 4, 7):
        for T in range(1, 8):
            A, pi, dur, edge = tdp.random_model(rng, D)
            e = dc.emissions(kind, T, rng)
            got = dcc.run_counts(e, A, pi, dur, edge)
            want, one = dcc.brute_force_counts(e, A, pi, dur, edge)
            worst = max(worst, float(np.abs(got - want).max()))
            assert worst <= 1e-12, (kind, D, T, worst)
            if want.any():
                assert abs(got[1].sum() - (2.0 - one)) <= 1e-12, (kind, D, T)
    print(kind, "worst", worst)


def test_restatement_identities():
    """sum_d d counts = sum_t gamma_t, sum counts = 1 + sum Xi, sum_d counts = sum_t S_t (S_0 included), sum counts[1] = 2 - P(one
    run) (P(one run) from the tables directly), all to T 2^-50; a recording nothing fits has counts 0."""
    rng = np.random.default_rng(72)
    for T, D in ((1, 3), (12, 5), (90, 16), (400, 64)):
        A, pi, dur, edge = tdp.random_model(rng, D)
        e = dc.emissions("dirichlet1", T, rng)
        c = dcc.run_counts(e, A, pi, dur, edge)
        fb = dpc.forward_backward(e, A, pi, dur, edge)
        tol = T * 2.0 ** -50
        both = c[0] + c[1]
        d = np.arange(1, D + 1)
        assert np.abs((both * d).sum(axis=1) - fb["raw_gamma"].sum(axis=0)).max() <= tol * D, (T, D)
        assert abs(c.sum() - (1.0 + fb["xi"].sum())) <= tol, (T, D)
        assert np.abs(both.sum(axis=1) - fb["onsets"].sum(axis=0)).max() <= tol, (T, D)
        one = 0.0
        if T <= D:                                       # one run of state j over the whole recording
            w = dpc._f64(pi) + dpc._f64(edge)[:, T - 1] + dpc.emissions64(e).sum(axis=0)
            one = float(np.exp(w - fb["logz"]).sum())
        assert abs(c[1].sum() - (2.0 - one)) <= tol, (T, D)
    none = np.full((4, 5), NINF, dtype=np.float32)
    assert not dcc.run_counts(dc.emissions("dirichlet1", 9, rng), A, pi, duc.random_tables(rng, 5)[0], none).any()


def test_counts_are_the_gradient_of_logz_in_the_tables():
    """Float64 autograd through duration_posterior_cases.torch_log_z in dur and edge equals counts[0] and counts[1] (1e-11)."""
    rng = np.random.default_rng(73)
    for T, D in ((1, 3), (7, 4), (40, 9), (90, 16)):
        A, pi, dur, edge = tdp.random_model(rng, D, forbidden=0.0)
        e = dc.emissions("dirichlet1", T, rng)
        td, tg = (torch.from_numpy(v).double().requires_grad_(True) for v in (dur, edge))
        dpc.torch_log_z(torch.from_numpy(e).double(), torch.from_numpy(A).double(), torch.from_numpy(pi).double(), td, tg).backward()
        c = dcc.run_counts(e, A, pi, dur, edge)
        gd, gg = (t.grad.numpy() if t.grad is not None else np.zeros((4, D)) for t in (td, tg))      # (T = 1 has no interior run)
        assert np.abs(gd - c[0]).max() <= 1e-11 and np.abs(gg - c[1]).max() <= 1e-11, (T, D)
        assert c[1].any() and (c[0].any() or T == 1)


@functools.lru_cache(maxsize=None)
def long_case(T, D):
    """tests/test_duration_posteriors.py's long case: the same generator, emissions and model."""
    rng = np.random.default_rng(7000 + T + D)
    e = torch.log_softmax(torch.from_numpy(rng.normal(0, 30, size=(T, 4))).float(), dim=1).numpy()
    A, pi, dur, edge = tdp.random_model(rng, D)
    return dcc.run_counts(e, A, pi, dur, edge), dcc.longdouble_run_counts(e, A, pi, dur, edge)


@pytest.mark.parametrize("D", (300, 2048))
@pytest.mark.parametrize("T", (3000, 6000))
def test_restatement_against_the_longdouble_twin(T, D):
    """An 80-bit log-space twin: the gate of this file's docstring, 8 x what was measured here."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is not wider than float64 here")
    got, want = long_case(T, D)
    diff = float(np.abs(got - want).max())
    print(f"T {T} D {D}: largest count {float(want.max()):.3f}, sum {float(want.sum()):.3f}, dcounts {diff:.3g}")
    assert want.sum() > 10 and diff <= COUNTS_GATE, diff


def test_counts_kernels_under_sanitizers(tmp_path):
    """csrc/duration_counts_layout.hpp in a program of its own (tests/native/duration_counts_check.cpp) built with
    -fsanitize=address,undefined: the runs variant of the sweeps and the counts kernel with lanes, stages, stashes and windows
    simulated give duration_counts_reference()'s outputs bit for bit, and no index leaves its array or its recording."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "duration_counts_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "duration_counts_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "duration counts check ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_argument_errors_need_no_device(built_lib):
    """Those of hssfsst_posteriors_durations, and counts NULL or misaligned; the workspace is the larger one."""
    F = built_lib.hssfsst_posteriors_durations_counts
    err = built_lib.hssfsst_last_error
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below ends before any device work
    ok = tdp.i64([0, 5])
    big = 1 << 40
    Dmax, _, mx = tdp.info(built_lib)[:3]
    per, rec, per_d, _ = counts_info(built_lib)

    def call(logp=fake, offs=ok, count=1, tab=fake, dur=fake, edge=fake, D=7, labels=None, gamma=fake, onsets=None, loglik=fake, score=None,
             xi=None, s0=None, counts=fake, work=fake, wb=big, device=0):
        return F(logp, offs, count, tab, dur, edge, D, labels, gamma, onsets, loglik, score, xi, s0, counts, work, wb, device, None)

    assert call(offs=tdp.i64([0]), count=0) == 0                                          # count == 0: nothing to do
    for kw, word in ((dict(logp=None), b"logp"), (dict(offs=None), b"offsets"), (dict(tab=None), b"a_pi"), (dict(dur=None), b"durations"),
                     (dict(edge=None), b"edge"), (dict(gamma=None), b"gamma"), (dict(loglik=None), b"loglik"), (dict(work=None), b"work"),
                     (dict(counts=None), b"counts")):
        assert call(**kw) == _lib.E_INVAL and word in err() and b"NULL" in err(), word
    assert b"posteriors_durations_counts" in err()
    assert call(score=fake) == _lib.E_INVAL and b"labels is NULL while score is not" in err()
    assert call(count=-1) == _lib.E_INVAL and b"negative" in err()
    assert call(device=-1) == _lib.E_INVAL and b"device" in err()
    for D in (0, -3, Dmax + 1):
        assert call(D=D) == _lib.E_INVAL and b"max_duration" in err(), D
    assert call(offs=tdp.i64([2, 4])) == _lib.E_INVAL and b"offsets[0]" in err()
    for bad in ([0, 5, 5], [0, 7, 3], [0, 4, 4, 9]):
        assert call(offs=tdp.i64(bad), count=len(bad) - 1) == _lib.E_INVAL and b"index 2" in err(), bad
    odd4, odd8 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    for kw, word in ((dict(logp=odd8), b"logp"), (dict(gamma=ctypes.c_void_p(4104)), b"gamma"), (dict(onsets=ctypes.c_void_p(4104)), b"onsets"),
                     (dict(work=ctypes.c_void_p(4104)), b"work"), (dict(tab=odd4), b"a_pi"), (dict(dur=odd4), b"durations"),
                     (dict(edge=odd4), b"edge"), (dict(loglik=odd8), b"loglik"), (dict(labels=fake, score=odd8), b"score"),
                     (dict(xi=odd8), b"xi"), (dict(s0=odd8), b"s0"), (dict(counts=odd8), b"counts")):
        assert call(**kw) == _lib.E_INVAL and word in err() and b"aligned" in err(), word
    need = per * 5 + rec + per_d * 7
    assert call(wb=need - 1) == _lib.E_INVAL and b"too small" in err() and str(need).encode() in err()
    # (enough workspace passes every argument check: a device index no machine has keeps the fake pointers from a kernel)
    assert call(wb=need, device=1 << 20) != _lib.E_INVAL or b"too small" not in err()
    assert call(offs=tdp.i64([0, 3, 3 + mx + 1]), count=2) == _lib.E_UNSUPPORTED and b"recording 1" in err()
    many = [i * mx for i in range(2049)]                                                  # 2^31 steps in all
    assert call(offs=tdp.i64(many), count=2048) == _lib.E_UNSUPPORTED and b"in all" in err()


def test_python_argument_errors_need_no_device():
    """What the Python layer refuses before it looks for a device, and the M-step, which runs on the host."""
    logp = torch.zeros((5, 4))
    dur = np.zeros((4, 6), dtype=np.float32)
    with pytest.raises(ValueError):
        duration_posteriors(logp, dur, return_counts=True)                                # log-probs on the host
    y = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(ValueError):
        duration_nll(logp, y, dur, learn_durations=True, reduction="median")
    with pytest.raises(ValueError):
        durations_from_counts(np.ones((4, 6)), fit="kernel")
    for bad in (np.ones((3, 6)), np.ones((2, 3, 6)), np.ones(6), np.full((4, 6), np.nan)):
        with pytest.raises(ValueError):
            durations_from_counts(bad)
    c = np.ones((4, 6))
    c[2] = 0.0
    with pytest.raises(ValueError, match="state 2"):
        durations_from_counts(c)
    # the fits: mean and population std of d under the counts (at least 0.5), and the log of the relative mass
    c = np.zeros((2, 4, 9))
    c[0, :, 3], c[0, :, 5] = 1.0, 3.0                    # d = 4 once, d = 6 three times: mean 5.5, std sqrt(0.75)
    c[0, 1] = 0.0
    c[0, 1, 6] = 2.5                                     # one duration only: std 0, raised to 0.5
    c[1] = 100.0                                         # the edge table is not used
    c[0, 3, 0] = -1e-18                                  # rounding below zero counts as zero
    want = consumer.gaussian_durations([5.5, 7.0, 5.5, 5.5], [np.sqrt(0.75), 0.5, np.sqrt(0.75), np.sqrt(0.75)], 9)
    assert np.array_equal(durations_from_counts(c), want) and np.array_equal(durations_from_counts(torch.from_numpy(c[0])), want)
    h = durations_from_counts(c, fit="histogram")
    assert h.dtype == np.float32 and h.shape == (4, 9) and np.isneginf(h[0, 0]) and np.isneginf(h[3, 0])
    assert np.allclose(np.exp(h[0]), np.array([0, 0, 0, 0.25, 0, 0.75, 0, 0, 0])) and np.exp(h[1, 6]) == 1.0


def test_shipped_kernel_resources(built_lib):
    """The two new kernels: no scratch, no AGPR, LDS within the CU's 160 KiB; splitting the sweeps into a template left
    seg_duration_posteriors_kernel with exactly the figures read on the parent commit."""
    for name in NEW_KERNELS:
        res = _lib.kernel_resources(name)
        assert len(res) == 1, res
        (facts,) = res.values()
        assert facts["private_segment_fixed_size"] == 0 and facts["agpr_count"] == 0, (name, facts)
        assert 0 < facts["group_segment_fixed_size"] <= 160 * 1024 and facts["vgpr_count"] <= 256, (name, facts)
    (old,) = _lib.kernel_resources("seg_duration_posteriors_kernel").values()
    assert {k: old[k] for k in PARENT_SWEEP} == PARENT_SWEEP and old["agpr_count"] == 0, old
    (runs,) = _lib.kernel_resources("seg_duration_runs_sweep_kernel").values()
    assert runs["group_segment_fixed_size"] == old["group_segment_fixed_size"], runs


# ---------------------------------------------------------------------------------------------------- GPU
OUTPUTS = ("logz", "score", "xi", "s0")


def gpu_counts(es, A, pi, dur, edge, labels=None):
    """tdp.gpu_post through hssfsst_posteriors_durations_counts: its dict, and counts (N, 2, 4, D)."""
    lib = _lib.lib()
    n = len(es)
    D = int(np.asarray(dur).shape[1])
    offs = np.concatenate([[0], np.cumsum([e.shape[0] for e in es])]).astype(np.int64)
    total = int(offs[-1])
    arena = torch.from_numpy(np.concatenate(es)).cuda()
    tab = torch.from_numpy(np.concatenate([np.asarray(A, dtype=np.float32).ravel(), np.asarray(pi, dtype=np.float32).ravel()])).cuda()
    tdur, tedge = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda() for v in (dur, edge))
    lab = torch.from_numpy(np.concatenate(labels).astype(np.uint8)).cuda() if labels is not None else None
    gamma = torch.full((total, 4), 7.0, dtype=torch.float32, device="cuda")
    onsets = torch.full((total, 4), 7.0, dtype=torch.float32, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    loglik, score = torch.full((n,), 7.0, **f64), torch.full((n,), 7.0, **f64)
    xi, s0 = torch.full((n, 16), 7.0, **f64), torch.full((n, 4), 7.0, **f64)
    counts = torch.full((n, 2, 4, D), 7.0, **f64)
    per, rec, per_d, _ = counts_info(lib)
    work = torch.empty(per * total + rec * n + per_d * D, dtype=torch.uint8, device="cuda")
    rc = lib.hssfsst_posteriors_durations_counts(arena.data_ptr(), offs.ctypes.data_as(I64P), n, tab.data_ptr(), tdur.data_ptr(), tedge.data_ptr(), D,
                                                 lab.data_ptr() if lab is not None else None, gamma.data_ptr(), onsets.data_ptr(),
                                                 loglik.data_ptr(), score.data_ptr() if lab is not None else None, xi.data_ptr(), s0.data_ptr(),
                                                 counts.data_ptr(), work.data_ptr(), work.numel(), 0, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "hssfsst_posteriors_durations_counts")
    g, o = gamma.cpu().numpy(), onsets.cpu().numpy()
    cut = lambda a: [a[offs[i]:offs[i + 1]] for i in range(n)]       # noqa: E731
    return dict(gamma=cut(g), onsets=cut(o), logz=loglik.cpu().numpy(), score=score.cpu().numpy(), xi=xi.cpu().numpy().reshape(n, 4, 4),
                s0=s0.cpu().numpy(), counts=counts.cpu().numpy())


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def assert_first_seven_are_the_plain_call(got, plain, labelled, what):
    for k in OUTPUTS:
        if k != "score" or labelled:
            assert same_bits(got[k], plain[k]), (what, k)
    for k in ("gamma", "onsets"):
        assert all(same_bits(a, b) for a, b in zip(got[k], plain[k])), (what, k)


def assert_counts_meet_the_gate(es, A, pi, dur, edge, got, labels=None, what="", want=None):
    D = int(np.asarray(dur).shape[1])
    for i, e in enumerate(es):
        w = want[i] if want is not None else dcc.run_counts(e, A, pi, dur, edge)
        if labels is not None:
            w = w - dcc.label_run_counts(labels[i], D)
        assert not np.isnan(got["counts"][i]).any(), (what, i)
        diff = float(np.abs(got["counts"][i] - w).max())
        assert diff <= COUNTS_GATE, (what, i, e.shape[0], diff)


@pytest.mark.gpu
@pytest.mark.parametrize("D", tdp.DURATIONS)
def test_meets_the_gate_against_the_restatement(built_lib, D):
    """tests/test_duration_posteriors.py's matrix: the shortest recordings, lengths around D, the segment borders; D below, at and
    above one block of durations and with all sixteen: one ragged call without labels and one with.  counts within the gate, the
    other seven outputs bit-identical to hssfsst_posteriors_durations on the same input."""
    rng = np.random.default_rng(400 + D)
    lens = tdp.matrix_lengths(D)
    A, pi, dur, edge = tdp.random_model(rng, D)
    es = [dc.emissions(dc.KINDS[k % 4], T, rng) for k, T in enumerate(lens)]
    labels = [dpc.legal_labels(T, rng, D) for T in lens]
    want = [dcc.run_counts(e, A, pi, dur, edge) for e in es]
    for lab in (None, labels):
        got = gpu_counts(es, A, pi, dur, edge, lab)
        assert_counts_meet_the_gate(es, A, pi, dur, edge, got, lab, what=(D, lab is not None), want=want)
        assert_first_seven_are_the_plain_call(got, tdp.gpu_post(es, A, pi, dur, edge, lab), lab is not None, (D, lab is not None))


@pytest.mark.gpu
def test_batching_neighbours_and_determinism(built_lib):
    """More recordings than one launch takes (300 > 256), T = 1 next to T = 5000: a recording's counts are bit-identical alone, in
    another place of the list and next to other neighbours; two calls give the same bits; the Python forms are the ragged call."""
    rng = np.random.default_rng(412)
    D = 33
    A, pi, dur, edge = tdp.random_model(rng, D)
    lens = [int(v) for v in rng.integers(1, 60, size=300)]
    lens[6], lens[7], lens[8], lens[270] = 1, 5000, 1, 600
    es = [dc.emissions("dirichlet1", T, rng) for T in lens]
    labels = [dpc.legal_labels(T, rng, D) for T in lens]
    full = gpu_counts(es, A, pi, dur, edge, labels)
    again = gpu_counts(es, A, pi, dur, edge, labels)
    assert same_bits(full["counts"], again["counts"])
    assert_first_seven_are_the_plain_call(full, tdp.gpu_post(es, A, pi, dur, edge, labels), True, "300")
    pick = [270, 7, 6, 0, 299, 256, 255, 100]
    some = gpu_counts([es[i] for i in pick], A, pi, dur, edge, [labels[i] for i in pick])
    for n, i in enumerate(pick):
        alone = gpu_counts([es[i]], A, pi, dur, edge, [labels[i]])
        assert same_bits(some["counts"][n], full["counts"][i]) and same_bits(alone["counts"][0], full["counts"][i]), i
    sub = [6, 7, 8, 270] + [i for i in range(300) if lens[i] <= 40][:10]
    assert_counts_meet_the_gate([es[i] for i in sub], A, pi, dur, edge, dict(counts=full["counts"][sub]), [labels[i] for i in sub], what="batched")

    dense = np.stack([dc.emissions("dirichlet0.2", 37, rng) for _ in range(5)])
    t = torch.from_numpy(dense).cuda()
    rag = RaggedFeatures(t.reshape(-1, 4), torch.arange(6, dtype=torch.int64) * 37, 4, False)
    g_r, z_r, o_r, c_r = duration_posteriors(rag, dur, A, pi, edge, return_loglik=True, return_onsets=True, return_counts=True)
    g_b, c_b = duration_posteriors(t, dur, A, pi, edge, return_counts=True)
    assert c_r.shape == c_b.shape == (5, 2, 4, D) and c_b.dtype == torch.float64 and c_b.is_cuda and torch.equal(c_r, c_b)
    plain = duration_posteriors(t, dur, A, pi, edge, return_loglik=True, return_onsets=True)
    assert torch.equal(g_r.data, plain[0].reshape(-1, 4)) and torch.equal(z_r, plain[1]) and torch.equal(o_r.data, plain[2].reshape(-1, 4))
    assert torch.equal(g_b, plain[0])
    g_1, z_1, c_1 = duration_posteriors(t[3], dur, A, pi, edge, return_loglik=True, return_counts=True)
    assert c_1.shape == (2, 4, D) and torch.equal(c_1, c_b[3]) and torch.equal(g_1, g_b[3]) and z_1.shape == ()
    want = [dcc.run_counts(dense[i], A, pi, dur, edge) for i in range(5)]
    assert_counts_meet_the_gate(list(dense), A, pi, dur, edge, dict(counts=c_b.cpu().numpy()), what="dense", want=want)


@pytest.mark.gpu
def test_special_inputs(built_lib):
    """-inf and NaN emissions; a recording no segmentation fits gets counts 0 (minus the labels' terms); a labelled run longer
    than D takes nothing off; D < 128, where most lanes idle (every case here)."""
    rng = np.random.default_rng(411)
    seg = consumer.duration_posteriors_info()[1]
    A, pi, dur, edge = tdp.random_model(rng, 9)
    es = [dc.emissions("dirichlet1", T, rng) for T in (30, seg + 3, 2, 1)]
    es[0][4, 1], es[0][0, 2], es[1][seg, 0], es[1][seg + 2, 3], es[2][1, 1] = np.nan, NINF, np.nan, NINF, np.nan
    es[0][11], es[3][0] = NINF, NINF
    got = gpu_counts(es, A, pi, dur, edge)
    assert_counts_meet_the_gate(es, A, pi, dur, edge, got, what="NaN and -inf")
    assert_first_seven_are_the_plain_call(got, tdp.gpu_post(es, A, pi, dur, edge), False, "NaN and -inf")

    none = np.full((4, 9), NINF, dtype=np.float32)
    es = [dc.emissions("dirichlet1", T, rng) for T in (10, 40, 5)]
    got = gpu_counts(es, A, pi, dur, none)
    assert (got["logz"] == NINF).all() and not got["counts"].any()
    labels = [dpc.legal_labels(T, rng, 9) for T in (10, 40, 5)]
    got = gpu_counts(es, A, pi, dur, none, labels)
    for i in range(3):
        assert np.array_equal(got["counts"][i], -dcc.label_run_counts(labels[i], 9)), i
    mixed = np.full((4, 9), NINF, dtype=np.float32)
    mixed[:, 8] = 0.0                                    # only cut-off runs of 9 steps: T = 9 and T = 18 fit, T = 10 does not
    es = [dc.emissions("dirichlet1", T, rng) for T in (9, 10, 18)]
    got = gpu_counts(es, A, pi, dur, mixed)
    assert not got["counts"][1].any() and got["counts"][0][1, :, 8].sum() == pytest.approx(1.0, abs=1e-12)
    assert got["counts"][2][1, :, 8].sum() == pytest.approx(2.0, abs=1e-12) and not got["counts"][2][0].any()
    assert_counts_meet_the_gate(es, A, pi, dur, mixed, got, what="edge of 9 only")

    e = dc.emissions("dirichlet1", 25, rng)
    y = np.array([0] * 10 + [1] * 9 + [2] * 6, dtype=np.uint8)                            # a run of 10 > D = 9, at the edge
    got = gpu_counts([e], A, pi, dur, edge, [y])
    assert np.isinf(got["score"][0]) and dcc.label_run_counts(y, 9).sum() == 2.0
    assert_counts_meet_the_gate([e], A, pi, dur, edge, got, [y], what="a labelled run of 10")


def twin_grads(es, labels, A, pi, dur, edge, weights, reduction):
    """The float64 CPU twin of duration_nll on the float32-rounded inputs: the value and the gradients in e, A, pi, dur, edge of
    sum_i weights_i nll_i ("none"), or of weights x the reduced loss."""
    tes = [torch.from_numpy(e).double().requires_grad_(True) for e in es]
    tabs = [torch.from_numpy(np.asarray(v, dtype=np.float32)).double().requires_grad_(True) for v in (A, pi, dur, edge)]
    nll = torch.stack([dpc.torch_nll(e, y, *tabs) for e, y in zip(tes, labels)])
    total = sum(e.shape[0] for e in es)
    value = nll if reduction == "none" else (nll.sum() if reduction == "sum" else nll.sum() / total)
    (value * torch.as_tensor(weights, dtype=torch.float64)).sum().backward()
    return value.detach(), [e.grad for e in tes], [t.grad for t in tabs]


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ("mean", "sum", "none"))
def test_gradients_against_the_cpu_twin(built_lib, reduction):
    """duration_nll(learn_durations=True) on a ragged list with float64 durations and edge (and A, pi) that require grad and a
    non-unit incoming gradient: the value and the gradients in logp, A, pi, durations and edge (1e-4 of each tensor's maximum)
    against float64 autograd through duration_posterior_cases.torch_nll; -inf entries get exactly 0."""
    rng = np.random.default_rng(414)
    lens = [1, 2, 9, 64, 33]
    es = [dc.emissions("dirichlet1", T, rng) for T in lens]
    for k, D in enumerate((16, 5)):
        dur, edge = duc.random_tables(rng, D)
        if k == 0:                                       # every duration allowed, random runs around the cycle
            A, pi = consumer.cyclic_transitions(float(np.log(0.9)), float(np.log(0.1)))
            dur = np.where(np.isneginf(dur), np.float32(-6.0), dur)
            labels = [dpc.legal_labels(T, rng, D) for T in lens]
        else:                                            # 30 % of dur forbidden: runs of D steps, which random_tables always allows
            A, pi = dc.dense_transitions(11), np.log(rng.dirichlet(np.ones(4))).astype(np.float32)
            labels = [(np.arange(T) // D % 4).astype(np.uint8) for T in lens]
        weights = rng.uniform(0.25, 1.0, size=len(lens)) if reduction == "none" else 0.75
        want, wge, wtabs = twin_grads(es, labels, A, pi, dur, edge, weights, reduction)
        assert torch.isfinite(want).all()
        logp = [torch.from_numpy(e).cuda().requires_grad_(True) for e in es]
        offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)
        tabs = [torch.from_numpy(v).double().cuda().requires_grad_(True) for v in (A, pi, dur, edge)]
        got = duration_nll(RaggedFeatures(torch.cat(logp), offs, 4, False), [torch.from_numpy(y) for y in labels], tabs[2], tabs[0], tabs[1],
                           tabs[3], reduction=reduction, learn_durations=True)
        assert got.dtype == (torch.float64 if reduction == "none" else torch.float32) and got.shape == want.shape
        assert torch.allclose(got.double().cpu(), want, rtol=1e-6 if reduction != "none" else 1e-11, atol=1e-12)
        (got.double() * torch.as_tensor(weights, dtype=torch.float64).cuda()).sum().backward()
        top = max(float(g.abs().max()) for g in wge)
        for i in range(len(lens)):
            assert float((logp[i].grad.double().cpu() - wge[i]).abs().max()) <= 1e-4 * top, (k, i)
        for name, t, w in zip(("A", "pi", "durations", "edge"), tabs, wtabs):
            assert t.grad.dtype == torch.float64 and t.grad.shape == w.shape
            diff, top_t = float((t.grad.cpu() - w).abs().max()), float(w.abs().max())
            print(reduction, k, name, "diff", diff, "max", top_t)
            assert top_t > 0 and diff <= 1e-4 * top_t, (k, name, diff, top_t)
            assert (t.grad[torch.isinf(t.detach())] == 0).all(), (k, name)
        if k == 1:
            assert torch.isinf(tabs[2]).any()
    # float32 tables get float32 gradients; without learn_durations a table that requires grad still raises
    d32, e32 = (torch.from_numpy(v).cuda().requires_grad_(True) for v in (dur, edge))
    lp = RaggedFeatures(torch.cat([t.detach() for t in logp]), offs, 4, False)
    ys = [torch.from_numpy(y) for y in labels]
    duration_nll(lp, ys, d32, A, pi, e32, learn_durations=True).backward()
    assert d32.grad.dtype == e32.grad.dtype == torch.float32 and d32.grad.shape == (4, 5)
    with pytest.raises(ValueError):
        duration_nll(lp, ys, d32, A, pi, e32)
    for kw in (dict(durations=dur, edge=e32), dict(durations=d32, edge=None), dict(durations=d32, edge=e32.cpu()), dict(durations=d32.half(), edge=e32),
               dict(durations=d32, edge=e32[:, :4])):
        with pytest.raises(ValueError):
            duration_nll(lp, ys, transitions=A, initial=pi, learn_durations=True, **kw)


@pytest.mark.gpu
def test_training_end_to_end_with_a_learnable_duration_table():
    """tests/test_duration_posteriors.py's twelve Adam steps on a tiny HipSegmenterHead (H 16, three recordings), with the duration
    table among the parameters: every loss is within 1e-4 relative of the float64 CPU twin's, and the table moves."""
    from tests.test_segmenter_train_ragged import looped64, twin64
    lens, D = [100, 140, 123], 10
    sig = synth.pcg_windows(3, 400, seed=23)
    recs = [torch.from_numpy(sig[i, :n].copy()).cuda() for i, n in enumerate(lens)]
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True)
    feats = tf.ragged(recs)
    xs = [feats[i].detach().clone() for i in range(3)]
    rng = np.random.default_rng(415)
    labels = [dpc.legal_labels(T, rng, D) for T in lens]
    dur0 = consumer.gaussian_durations([4.0, 5.0, 4.0, 6.0], 2.5, D)
    edge0 = edge_durations(dur0)
    torch.manual_seed(5)
    base = SegmenterHead(44, 16, 1)
    head = HipSegmenterHead(44, 16, 1, h0=base.h0.clone(), c0=base.c0.clone())
    head.load_state_dict(base.state_dict())
    head.cuda()
    ref = twin64(base)
    A0, pi0 = consumer.cyclic_transitions(float(np.log(0.9)), float(np.log(0.1)))

    def fit(m, loss_fn, device):
        m.eval()
        dur = torch.from_numpy(dur0).double().to(device).requires_grad_(True)
        edge = torch.from_numpy(edge0).double().to(device)
        opt = torch.optim.Adam(list(m.parameters()) + [dur], lr=0.01)
        out = []
        for _ in range(12):
            opt.zero_grad()
            loss = loss_fn(dur, edge)
            loss.backward()
            opt.step()
            out.append(float(loss.detach()))
        return out, dur.detach().cpu()
    xs64 = [x.double().cpu() for x in xs]
    total = sum(lens)
    A64, pi64 = torch.from_numpy(A0).double(), torch.from_numpy(pi0).double()

    def twin_loss(dur, edge):
        # (the kernel sees the table rounded to float32; a straight-through rounding keeps the twin's gradient)
        d32 = dur + (dur.float().double() - dur).detach()
        lp = looped64(ref, xs64, ref.h0, ref.c0)
        offs = np.concatenate([[0], np.cumsum(lens)])
        return sum(dpc.torch_nll(lp[offs[i]:offs[i + 1]], labels[i], A64, pi64, d32, edge) for i in range(3)) / total
    want, wdur = fit(ref, twin_loss, "cpu")
    ylist = [torch.from_numpy(y) for y in labels]
    got, gdur = fit(head, lambda dur, edge: duration_nll(head.ragged(xs), ylist, dur, A0, pi0, edge, learn_durations=True), "cuda")
    print("twin", [f"{v:.5f}" for v in want], "hip", [f"{v:.5f}" for v in got])
    assert all(abs(g_ - w) <= 1e-4 * abs(w) for g_, w in zip(got, want)), (got, want)
    assert got[-1] < got[0] and want[-1] < want[0]
    assert float((gdur - torch.from_numpy(dur0).double()).abs().max()) > 0.05 and float((gdur - wdur).abs().max()) <= 1e-3


def em_case():
    """Three recordings whose emissions are peaked (12 nats) on label sequences with runs of 5 .. 12 steps, under tables that
    prefer no duration: (es, labels, A, pi, dur, edge, lo)."""
    rng = np.random.default_rng(416)
    D, lo = 24, 5
    labels = [dpc.legal_labels(T, rng, D, lo=lo) for T in (300, 411, 257)]
    es = [torch.log_softmax(torch.from_numpy(12.0 * np.eye(4)[y] + rng.normal(0, 1, size=(len(y), 4))).float(), dim=1).numpy() for y in labels]
    A, pi = consumer.cyclic_transitions()
    dur = np.zeros((4, D), dtype=np.float32)
    return es, labels, A, pi, dur, dur.copy(), lo


def mass_on_the_true_runs(counts, lo):
    p = np.exp(durations_from_counts(counts, "histogram").astype(np.float64))
    assert np.abs(p.sum(axis=1) - 1).max() <= 1e-6
    return p[:, lo - 1:lo + 7].sum(axis=1)


def test_e_and_m_step_on_the_restatement():
    """The restatement alone: the histogram fit of the summed counts puts at least 0.99 of each state's mass on the true runs'
    durations lo .. lo + 7."""
    es, _, A, pi, dur, edge, lo = em_case()
    counts = sum(dcc.run_counts(e, A, pi, dur, edge) for e in es)
    mass = mass_on_the_true_runs(counts, lo)
    print("mass on lo .. lo + 7:", mass)
    assert (mass >= 0.99).all(), mass
    g = durations_from_counts(counts)                    # the gaussian fit's mean lies among the true durations
    assert ((np.argmax(g, axis=1) + 1 >= lo) & (np.argmax(g, axis=1) + 1 <= lo + 7)).all()


@pytest.mark.gpu
def test_e_and_m_step(built_lib):
    """One E-step on the device and one M-step: durations_from_counts(counts.sum(0), "histogram") puts at least 0.99 of each
    state's mass on lo .. lo + 7, from tables that preferred no duration."""
    es, _, A, pi, dur, edge, lo = em_case()
    offs = torch.tensor(np.concatenate([[0], np.cumsum([len(e) for e in es])]), dtype=torch.int64)
    rag = RaggedFeatures(torch.from_numpy(np.concatenate(es)).cuda(), offs, 4, False)
    _, counts = duration_posteriors(rag, dur, A, pi, edge, return_counts=True)
    assert counts.shape == (3, 2, 4, 24)
    mass = mass_on_the_true_runs(counts.sum(0), lo)
    assert (mass >= 0.99).all(), mass
    assert_counts_meet_the_gate(es, A, pi, dur, edge, dict(counts=counts.cpu().numpy()), what="E-step")
