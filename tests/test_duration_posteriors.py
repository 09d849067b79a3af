"""Log-probs -> state posteriors, run-onset posteriors and the sequence loss under the explicit-duration (semi-Markov) model:
hssfsst_posteriors_durations (C ABI), consumer.duration_posteriors, consumer.duration_nll,
segment_recordings(posteriors=..., durations=dur).

The contract is csrc/duration_posterior_layout.hpp's arithmetic -- float64 mantissas with integer exponents, every sum in a fixed
order -- restated in numpy in tests/duration_posterior_cases.py (vectorised over the duration, so equal to rounding, not bit for
bit).  CPU tests check the restatement itself (brute-force enumeration of every segmentation, an 80-bit log-space twin of the
recurrence, the first-order model where the two coincide, finite differences), the ABI, the argument errors (all raised before any
device work), the kernel's two sweeps with its lanes simulated under sanitizers (tests/native/duration_posteriors_check.cpp) and
the shipped kernel's resources.  Every GPU comparison is with the restatement or the CPU twin, never with the code under test.

Gates.  gamma and the onsets as the kernel stores them: 2^-23 absolute, the project's gamma gate (the float32 rounding of a value
<= 1, doubled).  The float64 outputs: 8 x the largest difference MEASURED between the restatement and the 80-bit twin over
T in {3000, 6000} x D in {300, 2048} on log_softmax emissions of N(0, 30^2) logits (down to -185), which was
    logZ 5.54e-10    gamma 3.81e-12    Xi 5.19e-11    onsets 3.73e-12
(the error grows with the emissions' prefix sums, |E_j(T)| x 2^-53: |E| reaches ~4e5 there).  The same gates hold the GPU's logZ,
score, Xi and S_0 against the restatement.  Against the first-order forward-backward under geometric tables, T = 700, the four emission kinds, measured
    gamma 6.2e-15    logZ 2.3e-13    Xi 8.6e-14
and gated at 8 x that."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, consumer, synth
from heart_sounds_segmentation_amd.consumer import (HipSegmenterHead, SegmenterHead, decode_durations, duration_nll, duration_posteriors,
                                                    edge_durations, segment_recordings, state_posteriors)
from heart_sounds_segmentation_amd.transforms import FSST, RaggedFeatures
from tests import decode_cases as dc
from tests import duration_cases as duc
from tests import duration_posterior_cases as dpc
from tests import posterior_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hssfsst.h")
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")
NINF = float("-inf")
I64P = ctypes.POINTER(ctypes.c_int64)
GAMMA_GATE = 2.0 ** -23                                  # float32 gamma and onsets
Z_GATE = 8 * 5.54e-10                                    # logZ and score, absolute
G64_GATE = 8 * 3.81e-12                                  # float64 gamma, onsets, S_0
XI_GATE = 8 * 5.19e-11
GEO_GATES = dict(gamma=8 * 6.2e-15, logz=8 * 2.3e-13, xi=8 * 8.6e-14)
DURATIONS = (1, 2, 127, 128, 129, 512, 2048)


def i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def info(lib):
    D, seg = ctypes.c_int(0), ctypes.c_int(0)
    mx, per, rec, dur = (ctypes.c_int64(0) for _ in range(4))
    assert lib.hssfsst_posteriors_durations_info(ctypes.byref(D), ctypes.byref(seg), ctypes.byref(mx), ctypes.byref(per), ctypes.byref(rec),
                                                 ctypes.byref(dur)) == 0
    return D.value, seg.value, mx.value, per.value, rec.value, dur.value


def random_model(rng, D, forbidden=0.3):
    """(A, pi, dur, edge): dense random transitions with a share forbidden (the cycle's moves stay), random duration tables."""
    A = dc.dense_transitions(int(rng.integers(1 << 30)))
    A[rng.random((4, 4)) < forbidden] = NINF
    for i in range(4):
        A[i, (i + 1) % 4] = np.float32(-0.7)
    pi = np.log(rng.dirichlet(np.ones(4))).astype(np.float32)
    dur, edge = duc.random_tables(rng, D, forbidden)
    return A, pi, dur, edge


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_library_and_info(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    assert "int hssfsst_posteriors_durations(" in text and "int hssfsst_posteriors_durations_info(" in text
    fn = built_lib.hssfsst_posteriors_durations
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 18
    D, seg, mx, per, rec, dur = info(built_lib)
    assert built_lib.hssfsst_posteriors_durations_info(None, None, None, None, None, None) == 0
    assert consumer.duration_posteriors_info() == (D, seg, mx, per, rec, dur)
    with open(os.path.join(CSRC, "duration_posterior_layout.hpp")) as fh:
        layout = fh.read()

    def constant(name):
        import re
        return re.search(r"constexpr \w+ " + name + r" = ([^;]+);", layout).group(1)
    assert D == consumer.decode_durations_info()[0] == 2048 and mx == 2 ** 20
    assert str(seg) == constant("kSegSteps") and constant("kMaxSteps") == "i64(1) << 20"
    assert constant("kStashBytesPerStep") == "48" and per == 49 <= 64 and rec == int(constant("kCheckpointBytes")) == 32
    assert dur == int(constant("kWorkBytesPerDuration")) == 96
    import heart_sounds_segmentation_amd as pkg
    for name in ("duration_posteriors", "duration_nll", "duration_posteriors_info"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(consumer, name)
    for f in ("segmenter_duration_posteriors.hpp", "duration_posterior_layout.hpp"):
        assert os.path.exists(os.path.join(CSRC, f))


@pytest.mark.parametrize("kind", dc.KINDS)
def test_restatement_equals_brute_force(kind):
    """Every segmentation enumerated (T <= 7, D in {1, 2, 3, 4, 7}), random tables with 30 % forbidden entries: gamma, logZ, Xi
    and the onsets to 1e-12 (measured: 3e-15)."""
    rng = np.random.default_rng(61)
    worst = 0.0
    for D in (1, 2, 3, 4, 7):
        for T in range(1, 8):
            A, pi, dur, edge = random_model(rng, D)
            e = dc.emissions(kind, T, rng)
            got, want = dpc.forward_backward(e, A, pi, dur, edge), dpc.brute_force(e, A, pi, dur, edge)
            if np.isinf(want["logz"]):
                assert got["logz"] == want["logz"], (D, T)
            else:
                worst = max(worst, abs(got["logz"] - want["logz"]))
            worst = max([worst] + [np.abs(got[k] - want[k]).max() for k in ("gamma", "xi", "onsets")])
            assert worst <= 1e-12, (kind, D, T, worst)
    print(kind, "worst", worst)


@functools.lru_cache(maxsize=None)
def long_case(T, D):
    rng = np.random.default_rng(7000 + T + D)
    e = torch.log_softmax(torch.from_numpy(rng.normal(0, 30, size=(T, 4))).float(), dim=1).numpy()
    A, pi, dur, edge = random_model(rng, D)
    return dpc.forward_backward(e, A, pi, dur, edge), dpc.longdouble_forward_backward(e, A, pi, dur, edge), float(e.min())


@pytest.mark.parametrize("D", (300, 2048))
@pytest.mark.parametrize("T", (3000, 6000))
def test_restatement_against_the_longdouble_twin(T, D):
    """An 80-bit log-space twin of the recurrence: the gates of this file's docstring, 8 x what was measured here."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is not wider than float64 here")
    got, want, low = long_case(T, D)
    dz = float(abs(got["logz"] - want["logz"]))
    dg, dx, do = (float(np.abs(got[a] - want[b]).max()) for a, b in (("raw_gamma", "gamma"), ("xi", "xi"), ("onsets", "onsets")))
    print(f"T {T} D {D} lowest emission {low:.1f} logZ {got['logz']:.3f}: dlogZ {dz:.3g} dgamma {dg:.3g} dXi {dx:.3g} donsets {do:.3g}")
    assert low < -140
    assert dz <= Z_GATE and dg <= G64_GATE and dx <= XI_GATE and do <= G64_GATE, (dz, dg, dx, do)


def test_restatement_matches_the_first_order_model_under_geometric_tables():
    """dur = edge = stay (d - 1), A[i][i] = stay, D >= T: every path weighs the same in both models: gamma and logZ equal
    posterior_cases.forward_backward's, Xi its off-diagonal part."""
    rng = np.random.default_rng(62)
    T = 700
    A = duc.geometric_transitions()
    dur, edge = duc.geometric_tables(T)
    for kind in dc.KINDS:
        pi = np.log(rng.dirichlet(np.ones(4))).astype(np.float32)
        e = dc.emissions(kind, T, rng)
        got = dpc.forward_backward(e, A, pi, dur, edge)
        (wg,), wlz, wxi = pc.forward_backward([e], [A], [pi])
        off = wxi[0] * (1.0 - np.eye(4))
        d = dict(gamma=np.abs(got["gamma"] - wg).max(), logz=abs(got["logz"] - wlz[0]), xi=np.abs(got["xi"] - off).max())
        print(kind, d)
        assert all(d[k] <= GEO_GATES[k] for k in d), (kind, d)


def test_restatement_further_checks():
    """gamma rows sum to 1, gamma_0 = S_0, starts and ends balance, logZ >= the score of decode()'s path, and gamma is the
    finite-difference gradient of logZ in the emissions."""
    rng = np.random.default_rng(63)
    for T, D in ((1, 3), (12, 5), (90, 20), (400, 64)):
        A, pi, dur, edge = random_model(rng, D)
        e = dc.emissions("dirichlet1", T, rng)
        got = dpc.forward_backward(e, A, pi, dur, edge)
        assert np.abs(got["raw_gamma"].sum(axis=1) - 1).max() <= T * 2.0 ** -50, (T, D)
        assert np.abs(got["raw_gamma"][0] - got["s0"]).max() <= T * 2.0 ** -50
        # every run that starts ends: the starts at 0 .. T - 1 and the ends before 1 .. T balance state by state
        assert np.abs(got["onsets"].sum(axis=0) - got["ends"][1:].sum(axis=0)).max() <= T * 2.0 ** -50
        path, _ = duc.decode(e, A, pi, dur, edge)
        best = duc.path_score(e, A, pi, dur, edge, path, exact=False)
        assert got["logz"] >= best - 1e-9 * abs(best), (T, D, got["logz"], best)
    # central differences, h = 1e-3: the truncation error is h^2 / 6 x the third derivative of logZ in one emission, a third
    # cumulant of an indicator (<= 0.1): 2e-8; the rounding of logZ (~30 x 2^-53) / h is 3e-12.  Gate 1e-7.
    T, D, h = 12, 5, 1e-3
    A, pi, dur, edge = random_model(rng, D)
    e = dc.emissions("dirichlet1", T, rng).astype(np.float64)
    gamma = dpc.forward_backward(e, A, pi, dur, edge)["gamma"]
    for t in range(T):
        for j in range(4):
            hi, lo = e.copy(), e.copy()
            hi[t, j] += h
            lo[t, j] -= h
            fd = (dpc.forward_backward(hi, A, pi, dur, edge)["logz"] - dpc.forward_backward(lo, A, pi, dur, edge)["logz"]) / (2 * h)
            assert abs(fd - gamma[t, j]) <= 1e-7, (t, j, fd, gamma[t, j])


def test_duration_posteriors_sweeps_under_sanitizers(tmp_path):
    """csrc/duration_posterior_layout.hpp in a program of its own (tests/native/duration_posteriors_check.cpp) built with
    -fsanitize=address,undefined: the kernel's two sweeps with lanes, ring, stages, stash and checkpoints simulated give the
    sequential reference loop's outputs bit for bit and no index leaves its array."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "duration_posteriors_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "duration_posteriors_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "duration posteriors check ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_argument_errors_need_no_device(built_lib):
    F = built_lib.hssfsst_posteriors_durations
    err = built_lib.hssfsst_last_error
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below ends before any device work
    ok = i64([0, 5])
    big = 1 << 40
    Dmax, _, mx, per, rec, per_d = info(built_lib)

    def call(logp=fake, offs=ok, count=1, tab=fake, dur=fake, edge=fake, D=7, labels=None, gamma=fake, onsets=None, loglik=fake, score=None,
             xi=None, s0=None, work=fake, wb=big, device=0):
        return F(logp, offs, count, tab, dur, edge, D, labels, gamma, onsets, loglik, score, xi, s0, work, wb, device, None)

    assert call(offs=i64([0]), count=0) == 0                                              # count == 0: nothing to do
    for kw, word in ((dict(logp=None), b"logp"), (dict(offs=None), b"offsets"), (dict(tab=None), b"a_pi"), (dict(dur=None), b"durations"),
                     (dict(edge=None), b"edge"), (dict(gamma=None), b"gamma"), (dict(loglik=None), b"loglik"), (dict(work=None), b"work")):
        assert call(**kw) == _lib.E_INVAL and word in err() and b"NULL" in err(), word
    assert call(score=fake) == _lib.E_INVAL and b"labels is NULL while score is not" in err()
    assert call(count=-1) == _lib.E_INVAL and b"negative" in err()
    assert call(device=-1) == _lib.E_INVAL and b"device" in err()
    for D in (0, -3, Dmax + 1):
        assert call(D=D) == _lib.E_INVAL and b"max_duration" in err(), D
    assert call(offs=i64([2, 4])) == _lib.E_INVAL and b"offsets[0]" in err()
    for bad in ([0, 5, 5], [0, 7, 3], [0, 4, 4, 9]):
        assert call(offs=i64(bad), count=len(bad) - 1) == _lib.E_INVAL and b"index 2" in err(), bad
    odd4, odd8 = ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    for kw, word in ((dict(logp=odd8), b"logp"), (dict(gamma=ctypes.c_void_p(4104)), b"gamma"), (dict(onsets=ctypes.c_void_p(4104)), b"onsets"),
                     (dict(work=ctypes.c_void_p(4104)), b"work"), (dict(tab=odd4), b"a_pi"), (dict(dur=odd4), b"durations"),
                     (dict(edge=odd4), b"edge"), (dict(loglik=odd8), b"loglik"), (dict(labels=fake, score=odd8), b"score"),
                     (dict(xi=odd8), b"xi"), (dict(s0=odd8), b"s0")):
        assert call(**kw) == _lib.E_INVAL and word in err() and b"aligned" in err(), word
    need = per * 5 + rec + per_d * 7
    assert call(wb=need - 1) == _lib.E_INVAL and b"too small" in err() and str(need).encode() in err()
    assert call(offs=i64([0, 3, 3 + mx + 1]), count=2) == _lib.E_UNSUPPORTED and b"recording 1" in err()
    many = [i * mx for i in range(2049)]                                                  # 2^31 steps in all
    assert call(offs=i64(many), count=2048) == _lib.E_UNSUPPORTED and b"in all" in err()


def test_python_argument_errors_need_no_device():
    """What the Python layer refuses before it looks for a device."""
    logp = torch.zeros((5, 4))
    dur = np.zeros((4, 6), dtype=np.float32)
    with pytest.raises(ValueError):
        duration_posteriors(logp, dur)                                                    # log-probs on the host
    with pytest.raises(ValueError):
        duration_nll(logp, torch.zeros(5, dtype=torch.int64), dur, reduction="median")
    with pytest.raises(ValueError):
        segment_recordings(None, None, [], durations=dur)                                 # durations without decode or posteriors
    with pytest.raises(ValueError):
        segment_recordings(None, None, [], decode=True, posteriors=True, durations=dur)


def test_shipped_kernel_resources(built_lib):
    """No scratch, no AGPR; the ring of 2049 steps (12 bytes a word, four words a step) and the stages fit the CU's 160 KiB."""
    res = _lib.kernel_resources("seg_duration_posteriors_kernel")
    assert len(res) == 1, res
    (facts,) = res.values()
    assert facts["private_segment_fixed_size"] == 0 and facts["agpr_count"] == 0, facts
    assert 2049 * 4 * 12 <= facts["group_segment_fixed_size"] <= 160 * 1024, facts
    assert 32 <= facts["vgpr_count"] <= 256, facts
    fill = _lib.kernel_resources("seg_duration_posteriors_fill_kernel")
    assert len(fill) == 1 and next(iter(fill.values()))["private_segment_fixed_size"] == 0, fill


# ---------------------------------------------------------------------------------------------------- GPU
def gpu_post(es, A, pi, dur, edge, labels=None, tables=True, want_onsets=True):
    """One ragged call through the C ABI on the list of (T, 4) numpy emissions -> dict of numpy results: gamma, onsets (lists of
    (T, 4) float32), logz, score (N,), xi (N, 4, 4), s0 (N, 4); labels: a list of uint8 arrays."""
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
    _, _, _, per, rec, per_d = info(lib)
    work = torch.empty(per * total + rec * n + per_d * D, dtype=torch.uint8, device="cuda")
    rc = lib.hssfsst_posteriors_durations(arena.data_ptr(), offs.ctypes.data_as(I64P), n, tab.data_ptr(), tdur.data_ptr(), tedge.data_ptr(), D,
                                          lab.data_ptr() if lab is not None else None, gamma.data_ptr(),
                                          onsets.data_ptr() if want_onsets else None, loglik.data_ptr(),
                                          score.data_ptr() if lab is not None else None, xi.data_ptr() if tables else None,
                                          s0.data_ptr() if tables else None, work.data_ptr(), work.numel(), 0,
                                          torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "hssfsst_posteriors_durations")
    g, o = gamma.cpu().numpy(), onsets.cpu().numpy()
    cut = lambda a: [a[offs[i]:offs[i + 1]] for i in range(n)]       # noqa: E731
    return dict(gamma=cut(g), onsets=cut(o), logz=loglik.cpu().numpy(), score=score.cpu().numpy(), xi=xi.cpu().numpy().reshape(n, 4, 4),
                s0=s0.cpu().numpy())


def assert_meets_the_gates(es, A, pi, dur, edge, got, labels=None, what="", want=None):
    """`got` (gpu_post's) against the restatement of every recording (`want`: those already computed)."""
    for i, e in enumerate(es):
        T = e.shape[0]
        w = want[i] if want is not None else dpc.forward_backward(e, A, pi, dur, edge)
        onehot = np.eye(4)[labels[i]] if labels is not None else np.zeros((T, 4))
        counts = dpc.label_counts(labels[i]) if labels is not None else 0.0
        assert not np.isnan(got["gamma"][i]).any() and not np.isnan(got["onsets"][i]).any(), (what, i, T)
        dg = np.abs(got["gamma"][i].astype(np.float64) - (w["gamma"] - onehot)).max()
        do = np.abs(got["onsets"][i].astype(np.float64) - w["onsets"]).max()
        assert dg <= GAMMA_GATE and do <= GAMMA_GATE, (what, i, T, dg, do)
        if np.isinf(w["logz"]):
            assert got["logz"][i] == w["logz"], (what, i, T, got["logz"][i])
        else:
            assert abs(got["logz"][i] - w["logz"]) <= Z_GATE, (what, i, T, got["logz"][i], w["logz"])
        assert np.abs(got["xi"][i] - (w["xi"] - counts)).max() <= XI_GATE, (what, i, T)
        assert np.abs(got["s0"][i] - (w["s0"] - onehot[0])).max() <= G64_GATE, (what, i, T)
        if labels is not None:
            sc = dpc.label_score(e, A, pi, dur, edge, labels[i])
            assert got["score"][i] == sc if np.isinf(sc) else abs(got["score"][i] - sc) <= Z_GATE, (what, i, T, got["score"][i], sc)


def matrix_lengths(D):
    seg = consumer.duration_posteriors_info()[1]
    return sorted({T for T in (1, 2, 3, D - 1, D, D + 1, 2 * (D + 1) + 3, seg - 1, seg, seg + 1, 2 * seg + 1) if T >= 1})


@pytest.mark.gpu
@pytest.mark.parametrize("D", DURATIONS)
def test_meets_the_gates_against_the_restatement(built_lib, D):
    """The shortest recordings, lengths around D, a wrapped ring, the stage borders; D below, at and above one duration per lane
    and with all sixteen: one ragged call without labels and one with, under random tables with 30 % forbidden entries."""
    rng = np.random.default_rng(300 + D)
    lens = matrix_lengths(D)
    A, pi, dur, edge = random_model(rng, D)
    es = [dc.emissions(dc.KINDS[k % 4], T, rng) for k, T in enumerate(lens)]
    labels = [dpc.legal_labels(T, rng, D) for T in lens]
    want = [dpc.forward_backward(e, A, pi, dur, edge) for e in es]
    assert_meets_the_gates(es, A, pi, dur, edge, gpu_post(es, A, pi, dur, edge), what=(D, "plain"), want=want)
    assert_meets_the_gates(es, A, pi, dur, edge, gpu_post(es, A, pi, dur, edge, labels), labels, what=(D, "labels"), want=want)


@pytest.mark.gpu
def test_a_minimum_duration_of_20(built_lib):
    """minimum_duration_tables(D, 20): interior runs below 20 steps are forbidden, cut-off ones are not; the cycle's transitions."""
    rng = np.random.default_rng(310)
    A, pi = consumer.cyclic_transitions()
    for D in (40, 150):
        dur, edge = duc.minimum_duration_tables(D, 20)
        lens = (1, 19, 20, 21, 45, 300)
        es = [dc.emissions("dirichlet1", T, rng) for T in lens]
        labels = [dpc.legal_labels(T, rng, D, lo=20) for T in lens]
        got = gpu_post(es, A, pi, dur, edge, labels)
        assert_meets_the_gates(es, A, pi, dur, edge, got, labels, what=("min 20", D))
        assert np.isfinite(got["score"]).all()
        short = [(np.arange(T) // 3 % 4).astype(np.uint8) for T in lens]                 # runs of 3: forbidden inside a recording
        got = gpu_post(es, A, pi, dur, edge, short)
        assert list(np.isinf(got["score"])) == [False, True, True, True, True, True]      # (T = 1 is one cut-off run)
        assert_meets_the_gates(es, A, pi, dur, edge, got, short, what=("min 20, short labels", D))


@pytest.mark.gpu
def test_special_inputs(built_lib):
    """-inf and NaN emissions and a step of four -inf count as -32768; a recording no segmentation fits gets logZ = -inf, gamma = 0,
    Xi = 0; a labelled run longer than D makes the loss +inf."""
    rng = np.random.default_rng(311)
    seg = consumer.duration_posteriors_info()[1]
    A, pi, dur, edge = random_model(rng, 9)
    es = [dc.emissions("dirichlet1", T, rng) for T in (30, seg + 3, 2, 1)]
    es[0][4, 1], es[0][0, 2], es[1][seg, 0], es[1][seg + 2, 3], es[2][1, 1] = np.nan, NINF, np.nan, NINF, np.nan
    es[0][11], es[3][0] = NINF, NINF
    assert_meets_the_gates(es, A, pi, dur, edge, gpu_post(es, A, pi, dur, edge), what="NaN and -inf")

    none = np.full((4, 9), NINF, dtype=np.float32)
    es = [dc.emissions("dirichlet1", T, rng) for T in (10, 40, 5)]
    got = gpu_post(es, A, pi, dur, none)
    assert (got["logz"] == NINF).all() and not any(g.any() for g in got["gamma"]) and not got["xi"].any() and not got["s0"].any()
    assert not any(o.any() for o in got["onsets"])
    assert_meets_the_gates(es, A, pi, dur, none, got, what="nothing fits")
    mixed = edge.copy()
    mixed[:, :] = NINF
    mixed[:, 8] = 0.0                                    # only cut-off runs of 9 steps: T = 9 and T = 18 fit, T = 10 does not
    es = [dc.emissions("dirichlet1", T, rng) for T in (9, 10, 18)]
    got = gpu_post(es, A, pi, dur, mixed)
    assert list(np.isinf(got["logz"])) == [False, True, False]
    assert_meets_the_gates(es, A, pi, dur, mixed, got, what="edge of 9 only")

    e = torch.from_numpy(dc.emissions("dirichlet1", 25, rng)).cuda()
    y = np.array([0] * 10 + [1] * 9 + [2] * 6)                                            # a run of 10 > D = 9
    loss = duration_nll(e, torch.from_numpy(y), dur, A, pi, edge, reduction="none")
    assert loss.shape == (1,) and float(loss[0]) == float("inf")
    y = np.array([0] * 9 + [1] * 9 + [2] * 7)
    assert np.isfinite(float(duration_nll(e, torch.from_numpy(y), np.zeros((4, 9), dtype=np.float32), A, pi, reduction="sum")))


@pytest.mark.gpu
def test_batching_neighbours_and_determinism(built_lib):
    """More recordings than one launch takes (300 > 256), T = 1 next to T = 5000: a recording's outputs are bit-identical alone, in
    another place of the list and next to other neighbours; two runs give the same bits; the dense forms are the ragged call."""
    rng = np.random.default_rng(312)
    D = 33
    A, pi, dur, edge = random_model(rng, D)
    lens = [int(v) for v in rng.integers(1, 60, size=300)]
    lens[6], lens[7], lens[8], lens[270] = 1, 5000, 1, 600
    es = [dc.emissions("dirichlet1", T, rng) for T in lens]
    labels = [dpc.legal_labels(T, rng, D) for T in lens]
    keys = ("logz", "score", "xi", "s0")
    full = gpu_post(es, A, pi, dur, edge, labels)
    again = gpu_post(es, A, pi, dur, edge, labels)
    for k in keys:
        assert np.array_equal(full[k], again[k]), k
    for k in ("gamma", "onsets"):
        assert all(np.array_equal(a, b) for a, b in zip(full[k], again[k])), k
    pick = [270, 7, 6, 0, 299, 256, 255, 100]
    some = gpu_post([es[i] for i in pick], A, pi, dur, edge, [labels[i] for i in pick])
    for n, i in enumerate(pick):
        alone = gpu_post([es[i]], A, pi, dur, edge, [labels[i]])
        for other, at in ((some, n), (alone, 0)):
            assert np.array_equal(other["gamma"][at], full["gamma"][i]) and np.array_equal(other["onsets"][at], full["onsets"][i]), i
            assert all(np.array_equal(other[k][at], full[k][i]) for k in keys), i
    sub = [6, 7, 8] + [i for i in range(300) if lens[i] <= 40][:10]
    assert_meets_the_gates([es[i] for i in sub], A, pi, dur, edge,
                           {k: [v[i] for i in sub] if isinstance(v, list) else v[sub] for k, v in full.items()}, [labels[i] for i in sub], what="batched")

    dense = np.stack([dc.emissions("dirichlet0.2", 37, rng) for _ in range(5)])
    t = torch.from_numpy(dense).cuda()
    rag = RaggedFeatures(t.reshape(-1, 4), torch.arange(6, dtype=torch.int64) * 37, 4, False)
    g_r, z_r, o_r = duration_posteriors(rag, dur, A, pi, edge, return_loglik=True, return_onsets=True)
    g_b, z_b, o_b = duration_posteriors(t, dur, A, pi, edge, return_loglik=True, return_onsets=True)
    assert isinstance(g_r, RaggedFeatures) and isinstance(o_r, RaggedFeatures) and g_b.shape == o_b.shape == (5, 37, 4) and g_b.dtype == torch.float32
    assert z_b.is_cuda and z_b.dtype == torch.float64 and z_b.shape == (5,)
    assert torch.equal(g_b.reshape(-1, 4), g_r.data) and torch.equal(z_b, z_r) and torch.equal(o_b.reshape(-1, 4), o_r.data)
    g_1, z_1 = duration_posteriors(t[3], dur, A, pi, edge, return_loglik=True)
    assert torch.equal(g_1, g_b[3]) and z_1.shape == () and torch.equal(z_1, z_b[3])
    g_o, o_1 = duration_posteriors(t[3], dur, A, pi, edge, return_onsets=True)
    assert torch.equal(g_o, g_1) and torch.equal(o_1, o_b[3]) and torch.equal(duration_posteriors(t, dur, A, pi, edge), g_b)
    # the default edge is edge_durations(dur); tables on the device are taken as they are
    want = duration_posteriors(t, dur, A, pi, edge_durations(dur))
    assert torch.equal(duration_posteriors(t, dur, A, pi), want)
    assert torch.equal(duration_posteriors(t, torch.from_numpy(dur).cuda(), torch.from_numpy(A).cuda(), torch.from_numpy(pi).cuda(),
                                           torch.from_numpy(edge_durations(dur)).cuda()), want)
    assert not duration_posteriors(t.clone().requires_grad_(True), dur, A, pi).requires_grad
    for bad in (t.double(), t.cpu(), t[:, :, :3]):
        with pytest.raises(ValueError):
            duration_posteriors(bad, dur, A, pi)
    for kw in (dict(durations=torch.from_numpy(dur).requires_grad_(True)), dict(durations=dur, edge=torch.from_numpy(edge).cuda().requires_grad_(True))):
        with pytest.raises(ValueError):
            duration_nll(t, torch.zeros((5, 37), dtype=torch.int64), transitions=A, initial=pi, **kw)
    with pytest.raises(ValueError):
        duration_posteriors(t, np.zeros((4, 2049), dtype=np.float32), A, pi)
    with pytest.raises(ValueError):
        duration_posteriors(t, dur, A, pi, edge[:, :5])


@pytest.mark.gpu
def test_consistency_with_the_first_order_kernel_and_the_decoder(built_lib):
    """Geometric tables with D >= T: the result matches state_posteriors on the same input within the gates.  logZ >= the score of
    decode_durations' path (less the quantiser's T 2^-19)."""
    rng = np.random.default_rng(313)
    T = 500
    A = duc.geometric_transitions()
    dur, edge = duc.geometric_tables(T)
    pi = np.log(rng.dirichlet(np.ones(4))).astype(np.float32)
    e = torch.from_numpy(np.stack([dc.emissions(k, T, rng) for k in dc.KINDS])).cuda()
    g, z = duration_posteriors(e, dur, A, pi, edge, return_loglik=True)
    wg, wz = state_posteriors(e, A, pi, return_loglik=True)
    assert float((g - wg).abs().max()) <= GAMMA_GATE and float((z - wz).abs().max()) <= Z_GATE
    A2, pi2, dur2, edge2 = random_model(rng, 24)
    for T in (1, 400, 3000):
        e = torch.from_numpy(dc.emissions("dirichlet1", T, rng)).cuda()
        _, sc = decode_durations(e, dur2, A2, pi2, edge2, return_scores=True)
        _, lz = duration_posteriors(e, dur2, A2, pi2, edge2, return_loglik=True)
        assert float(lz) >= float(sc) - T * 2.0 ** -19 - 1e-9, (T, float(lz), float(sc))


def twin_grads(es, labels, A, pi, dur, edge, weights, reduction):
    """The float64 CPU twin of duration_nll on the float32-rounded inputs: the value and the gradients in e, A, pi of
    sum_i weights_i nll_i ("none"), or of weights x the reduced loss."""
    tes = [torch.from_numpy(e).double().requires_grad_(True) for e in es]
    tA, tpi = (torch.from_numpy(np.asarray(v, dtype=np.float32)).double().requires_grad_(True) for v in (A, pi))
    td, tg = (torch.from_numpy(np.asarray(v, dtype=np.float32)).double() for v in (dur, edge))
    nll = torch.stack([dpc.torch_nll(e, y, tA, tpi, td, tg) for e, y in zip(tes, labels)])
    total = sum(e.shape[0] for e in es)
    value = nll if reduction == "none" else (nll.sum() if reduction == "sum" else nll.sum() / total)
    (value * torch.as_tensor(weights, dtype=torch.float64)).sum().backward()
    return value.detach(), [e.grad for e in tes], tA.grad, tpi.grad


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ("mean", "sum", "none"))
def test_gradients_against_the_cpu_twin(built_lib, reduction):
    """duration_nll on a ragged list with learnable float64 A and pi on the device and a non-unit incoming gradient: the value
    (1e-6 relative in float32, 1e-11 in float64) and the gradients in logp, A and pi (1e-4 of each tensor's maximum) against
    float64 autograd through a log-space O(T D) loop; the diagonal and forbidden entries of A get gradient 0."""
    rng = np.random.default_rng(314)
    lens = [1, 2, 9, 64, 33]
    es = [dc.emissions("dirichlet1", T, rng) for T in lens]
    for k, D in enumerate((16, 5)):
        dur, edge = duc.random_tables(rng, D)
        if k == 0:
            A, pi = consumer.cyclic_transitions(float(np.log(0.9)), float(np.log(0.1)))
        else:
            A, pi = dc.dense_transitions(11), np.log(rng.dirichlet(np.ones(4))).astype(np.float32)
        if k == 0:                                       # every duration allowed, random runs around the cycle
            dur = np.where(np.isneginf(dur), np.float32(-6.0), dur)
            labels = [dpc.legal_labels(T, rng, D) for T in lens]
        else:                                            # 30 % of dur forbidden: runs of D steps, which random_tables always allows
            labels = [(np.arange(T) // D % 4).astype(np.uint8) for T in lens]
        weights = rng.uniform(0.25, 1.0, size=len(lens)) if reduction == "none" else 0.75
        want, wge, wgA, wgpi = twin_grads(es, labels, A, pi, dur, edge, weights, reduction)
        assert torch.isfinite(want).all()
        logp = [torch.from_numpy(e).cuda().requires_grad_(True) for e in es]
        offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)
        gA = torch.from_numpy(A).double().cuda().requires_grad_(True)
        gpi = torch.from_numpy(pi).double().cuda().requires_grad_(True)
        got = duration_nll(RaggedFeatures(torch.cat(logp), offs, 4, False), [torch.from_numpy(y) for y in labels], dur, gA, gpi, edge,
                           reduction=reduction)
        assert got.dtype == (torch.float64 if reduction == "none" else torch.float32) and got.shape == want.shape
        assert torch.allclose(got.double().cpu(), want, rtol=1e-6 if reduction != "none" else 1e-11, atol=1e-12)
        (got.double() * torch.as_tensor(weights, dtype=torch.float64).cuda()).sum().backward()
        top = max(float(g.abs().max()) for g in wge)
        for i in range(len(lens)):
            assert float((logp[i].grad.double().cpu() - wge[i]).abs().max()) <= 1e-4 * top, (k, i)
        assert float((gA.grad.cpu() - wgA).abs().max()) <= 1e-4 * float(wgA.abs().max()), k
        assert float((gpi.grad.cpu() - wgpi).abs().max()) <= 1e-4 * float(wgpi.abs().max()), k
        assert (gA.grad[torch.isinf(gA.detach())] == 0).all() and (torch.diagonal(gA.grad) == 0).all()


@pytest.mark.gpu
def test_training_end_to_end():
    """A tiny HipSegmenterHead (H 16), three synthetic recordings of different lengths, twelve Adam steps on
    duration_nll(head.ragged(feats), labels, dur) with learnable transitions: the loss falls, and every loss is within 1e-4
    relative of the float64 CPU twin's (the gate of tests/test_posteriors.py's twelve-step test)."""
    from tests.test_segmenter_train_ragged import looped64, twin64
    lens, D = [100, 140, 123], 10
    sig = synth.pcg_windows(3, 400, seed=23)
    recs = [torch.from_numpy(sig[i, :n].copy()).cuda() for i, n in enumerate(lens)]
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True)
    feats = tf.ragged(recs)
    xs = [feats[i].detach().clone() for i in range(3)]
    rng = np.random.default_rng(315)
    labels = [dpc.legal_labels(T, rng, D) for T in lens]
    dur = consumer.gaussian_durations([4.0, 5.0, 4.0, 6.0], 2.5, D)
    edge = edge_durations(dur)
    torch.manual_seed(5)
    base = SegmenterHead(44, 16, 1)
    head = HipSegmenterHead(44, 16, 1, h0=base.h0.clone(), c0=base.c0.clone())
    head.load_state_dict(base.state_dict())
    head.cuda()
    ref = twin64(base)
    A0, pi0 = consumer.cyclic_transitions(float(np.log(0.9)), float(np.log(0.1)))

    def fit(m, loss_fn, device):
        m.eval()
        A = torch.from_numpy(A0).double().to(device).requires_grad_(True)
        pi = torch.from_numpy(pi0).double().to(device).requires_grad_(True)
        opt = torch.optim.Adam(list(m.parameters()) + [A, pi], lr=0.01)
        out = []
        for _ in range(12):
            opt.zero_grad()
            loss = loss_fn(A, pi)
            loss.backward()
            opt.step()
            out.append(float(loss.detach()))
        return out
    xs64 = [x.double().cpu() for x in xs]
    total = sum(lens)
    d64, g64 = torch.from_numpy(dur).double(), torch.from_numpy(edge).double()

    def twin_loss(A, pi):
        # (the kernel sees the tables rounded to float32; a straight-through rounding keeps the twin's gradient; -inf stays)
        A32 = A + torch.nan_to_num(A.float().double() - A, nan=0.0).detach()
        pi32 = pi + torch.nan_to_num(pi.float().double() - pi, nan=0.0).detach()
        lp = looped64(ref, xs64, ref.h0, ref.c0)
        offs = np.concatenate([[0], np.cumsum(lens)])
        return sum(dpc.torch_nll(lp[offs[i]:offs[i + 1]], labels[i], A32, pi32, d64, g64) for i in range(3)) / total
    want = fit(ref, twin_loss, "cpu")
    ylist = [torch.from_numpy(y) for y in labels]
    got = fit(head, lambda A, pi: duration_nll(head.ragged(xs), ylist, dur, A, pi), "cuda")
    print("twin", [f"{v:.5f}" for v in want], "hip", [f"{v:.5f}" for v in got])
    assert all(abs(g_ - w) <= 1e-4 * abs(w) for g_, w in zip(got, want)), (got, want)
    assert got[-1] < got[0] and want[-1] < want[0]


@pytest.mark.gpu
def test_integration_with_the_segmenter_and_stream_order():
    """duration_posteriors right behind the segmenter call, with no synchronisation in between, and on a side stream, gives what
    the synchronised sequence gives; segment_recordings(posteriors=..., durations=dur) is that; durations alone still raise, and so
    do decode and posteriors together."""
    torch.manual_seed(31)
    seg = SegmenterHead(44, 16, 3).eval().hip()
    sig = synth.pcg_windows(3, 2000, seed=22)
    recs = [torch.from_numpy(sig[i, :n].copy()).cuda() for i, n in enumerate((100, 700, 333))]
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True)
    feats = tf.ragged(recs)
    dur = consumer.gaussian_durations([30.0, 50.0, 25.0, 80.0], [8.0, 12.0, 6.0, 30.0], 200, min_duration=5)
    logp = seg.ragged(feats)
    torch.cuda.synchronize()
    gamma, logz = duration_posteriors(logp, dur, return_loglik=True)
    torch.cuda.synchronize()
    host = logp.data.cpu().numpy()
    offs = logp.offsets.tolist()
    A, pi = consumer.cyclic_transitions()
    for i in range(3):
        w = dpc.forward_backward(host[offs[i]:offs[i + 1]], A, pi, dur, edge_durations(dur))
        assert np.abs(gamma[i].cpu().numpy().astype(np.float64) - w["gamma"]).max() <= GAMMA_GATE
        assert abs(float(logz[i]) - w["logz"]) <= Z_GATE
    unsynced = duration_posteriors(seg.ragged(feats), dur)       # enqueued behind the segmenter on the current stream
    assert torch.equal(unsynced.data, gamma.data)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = duration_posteriors(seg.ragged(feats), dur)
    side.synchronize()
    assert torch.equal(on_side.data, gamma.data)
    e2e = segment_recordings(tf, seg, recs, posteriors=True, durations=dur)
    assert isinstance(e2e, RaggedFeatures) and torch.equal(e2e.data, gamma.data) and e2e.lengths().tolist() == [100, 700, 333]
    A2, pi2 = consumer.cyclic_transitions(float(np.log(0.9)), float(np.log(0.1)))
    pi2 = pi2 + np.array([0.0, -1.0, -2.0, -0.5], dtype=np.float32)
    custom = segment_recordings(tf, seg, recs, posteriors=(A2, pi2), durations=dur)
    assert torch.equal(custom.data, duration_posteriors(logp, dur, A2, pi2).data) and not torch.equal(custom.data, gamma.data)
    assert torch.equal(segment_recordings(tf, seg, recs, posteriors=True).data, state_posteriors(logp).data)     # without durations: unchanged
    with pytest.raises(ValueError):
        segment_recordings(tf, seg, recs, durations=dur)
    for kw in (dict(decode=True, posteriors=True, durations=dur), dict(decode=(A, pi), posteriors=True)):
        with pytest.raises(ValueError):
            segment_recordings(tf, seg, recs, **kw)
