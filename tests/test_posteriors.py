"""Log-probs -> state posteriors and the sequence loss under the transition model: hssfsst_posteriors (C ABI),
consumer.state_posteriors, consumer.sequence_nll, segment_recordings(posteriors=True).

The contract is float64 inside (linear domain, scaled by exact powers of two) and float32 gamma out -- restated in numpy in
tests/posterior_cases.py.  CPU tests check the restatement itself (brute-force enumeration of all paths, an np.longdouble
log-space forward-backward, the closed form without transitions, torch float64 autograd), the ABI, the argument errors (all raised
before any device work), the kernel's sweeps with its lanes simulated under sanitizers (tests/native/posteriors_check.cpp) and the
shipped kernel's resources.  Every GPU comparison is with the restatement or the CPU twin, never with the code under test.

Gates, derived: gamma 2^-23 absolute (the float32 rounding of a value <= 1, doubled); logZ and score 8 T 2^-53 + 2^-50 |value|
(T float64 steps of a few roundings each, and the roundings of a sum of that size); Xi T 2^-40 absolute."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

from heart_sounds_segmentation_amd import _lib, consumer, synth
from heart_sounds_segmentation_amd.consumer import (HipSegmenterHead, RaggedStates, SegmenterHead, cyclic_transitions, decode_states,
                                                    segment_recordings, sequence_nll, state_posteriors, transitions_from_labels)
from heart_sounds_segmentation_amd.transforms import FSST, RaggedFeatures
from tests import decode_cases as dc
from tests import posterior_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hssfsst.h")
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")
NINF = float("-inf")
I64P = ctypes.POINTER(ctypes.c_int64)
GAMMA_GATE = 2.0 ** -23
LANES = 256                                              # include/hssfsst.h: segment_steps = 256 lanes x the steps a lane owns


def z_gate(T, value):
    return 8 * T * 2.0 ** -53 + 2.0 ** -50 * abs(value)


def xi_gate(T):
    return T * 2.0 ** -40


def i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def info(lib):
    seg, mx, per, rec = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.hssfsst_posteriors_info(ctypes.byref(seg), ctypes.byref(mx), ctypes.byref(per), ctypes.byref(rec)) == 0
    return seg.value, mx.value, per.value, rec.value


def cyclic91():
    return cyclic_transitions(float(np.log(0.9)), float(np.log(0.1)))


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_library_and_info(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    assert "int hssfsst_posteriors(" in text and "int hssfsst_posteriors_info(" in text and "700 nats" in text
    fn = built_lib.hssfsst_posteriors
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    seg, mx, per, rec = info(built_lib)
    assert seg % LANES == 0 and seg >= LANES and mx == 2 ** 20 and per >= 1 and rec >= 32
    assert built_lib.hssfsst_posteriors_info(None, None, None, None) == 0
    assert consumer.posteriors_info() == (seg, mx, per, rec)
    import heart_sounds_segmentation_amd as pkg
    for name in ("state_posteriors", "sequence_nll"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(consumer, name)
    for f in ("segmenter_posteriors.hpp", "posterior_layout.hpp"):
        assert os.path.exists(os.path.join(CSRC, f))


@pytest.mark.parametrize("kind", dc.KINDS)
def test_restatement_equals_brute_force(kind):
    """All 4^T paths enumerated (T <= 6): logZ, gamma and Xi, under dense random tables and the cycle, uniform and one-state pi."""
    rng = np.random.default_rng(41)
    for case in range(10):
        T = int(rng.integers(1, 7))
        A = cyclic91()[0] if case % 2 else dc.dense_transitions(case)
        pi = dc.STATE0 if case % 3 == 0 else np.log(rng.dirichlet(np.ones(4))).astype(np.float32)
        e = dc.emissions(kind, T, rng)
        (g,), lz, xi = pc.forward_backward([e], [A], [pi])
        wg, wlz, wxi = pc.brute_force(e, A, pi)
        assert abs(lz[0] - wlz) <= 1e-13 * max(1.0, abs(wlz)), (case, T)
        assert np.abs(g - wg).max() <= 1e-13 and np.abs(xi[0] - wxi).max() <= 1e-13, (case, T)
        assert abs(g.sum() - T) <= 1e-12 and abs(xi[0].sum() - (T - 1)) <= 1e-12


@pytest.mark.parametrize("kind", dc.KINDS)
def test_restatement_against_longdouble_log_space(kind):
    """An 80-bit log-space forward-backward at T up to 5000: |dlogZ| <= 8 T 2^-53 + 2^-50 |logZ|, |dgamma| <= 1e-12."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is not wider than float64 here")
    rng = np.random.default_rng(42)
    A, pi = cyclic91()
    for T in (1, 2, 2049, 5000):
        e = dc.emissions(kind, T, rng)
        (g,), lz, _ = pc.forward_backward([e], [A], [pi])
        wg, wlz = pc.longdouble_forward_backward(e, A, pi)
        dz, dg = float(abs(np.longdouble(lz[0]) - wlz)), float(np.abs(g.astype(np.longdouble) - wg).max())
        print(kind, T, "dlogZ", dz, "dgamma", dg)
        assert dz <= z_gate(T, float(wlz)), (kind, T, dz)
        assert dg <= 1e-12, (kind, T, dg)


def test_restatement_closed_form_without_transitions():
    """A = 0, pi = 0: the steps are independent: logZ = sum_t logsumexp(e_t), gamma_t = softmax(e_t), Xi = sum_t gamma_(t-1) x gamma_t."""
    rng = np.random.default_rng(43)
    A, pi = np.zeros((4, 4), dtype=np.float32), np.zeros(4, dtype=np.float32)
    for kind in dc.KINDS:
        e = dc.emissions(kind, 700, rng)
        e64 = torch.from_numpy(e).double()
        (g,), lz, xi = pc.forward_backward([e], [A], [pi])
        sm = torch.softmax(e64, dim=1).numpy()
        want = float(torch.logsumexp(e64, dim=1).sum())
        assert abs(lz[0] - want) <= z_gate(700, want) and np.abs(g - sm).max() <= 1e-14
        assert np.abs(xi[0] - np.einsum("ti,tj->ij", sm[:-1], sm[1:])).max() <= 1e-11


def test_restatement_is_the_gradient_of_log_z():
    """torch float64 autograd through a log-space loop: dlogZ/de = gamma, dlogZ/dA = Xi, dlogZ/dpi = gamma_0."""
    rng = np.random.default_rng(44)
    for T, A in ((1, dc.dense_transitions(1)), (9, dc.dense_transitions(2)), (60, cyclic91()[0])):
        pi = np.log(rng.dirichlet(np.ones(4))).astype(np.float32)
        e = dc.emissions("dirichlet1", T, rng)
        te, tA, tpi = (torch.from_numpy(np.asarray(v)).double().requires_grad_(True) for v in (e, A, pi))
        pc.torch_log_z(te, tA, tpi).backward()
        (g,), _, xi = pc.forward_backward([e], [A], [pi])
        assert np.abs(te.grad.numpy() - g).max() <= 1e-12
        grad_A = tA.grad.numpy() if tA.grad is not None else np.zeros((4, 4))              # (T = 1 has no transition)
        assert np.abs(grad_A - xi[0]).max() <= 1e-11 and np.abs(tpi.grad.numpy() - g[0]).max() <= 1e-12


def test_posteriors_sweeps_under_sanitizers(tmp_path):
    """csrc/posterior_layout.hpp in a program of its own (tests/native/posteriors_check.cpp) built with
    -fsanitize=address,undefined: the kernel's two sweeps with lanes, scans and segments simulated equal the sequential reference
    loop to 1e-13 relative, no index leaves the stage or the workspace, zero matrices renormalise without UB."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "posteriors_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "posteriors_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "posteriors check ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_argument_errors_need_no_device(built_lib):
    F = built_lib.hssfsst_posteriors
    err = built_lib.hssfsst_last_error
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below ends before any device work
    ok = i64([0, 5])
    big = 1 << 40
    _, mx, per, rec = info(built_lib)

    def call(logp=fake, offs=ok, count=1, tab=fake, labels=None, gamma=fake, loglik=fake, score=None, xi=None, g0=None, work=fake, wb=big,
             device=0):
        return F(logp, offs, count, tab, labels, gamma, loglik, score, xi, g0, work, wb, device, None)

    assert call(offs=i64([0]), count=0) == 0                                              # count == 0: nothing to do
    for kw, word in ((dict(logp=None), b"logp"), (dict(offs=None), b"offsets"), (dict(tab=None), b"a_pi"), (dict(gamma=None), b"gamma"),
                     (dict(loglik=None), b"loglik"), (dict(work=None), b"work")):
        assert call(**kw) == _lib.E_INVAL and word in err() and b"NULL" in err(), word
    assert call(score=fake) == _lib.E_INVAL and b"labels is NULL while score is not" in err()
    assert call(count=-1) == _lib.E_INVAL and b"negative" in err()
    assert call(device=-1) == _lib.E_INVAL and b"device" in err()
    assert call(offs=i64([2, 4])) == _lib.E_INVAL and b"offsets[0]" in err()
    for bad in ([0, 5, 5], [0, 7, 3], [0, 4, 4, 9]):
        assert call(offs=i64(bad), count=len(bad) - 1) == _lib.E_INVAL and b"index 2" in err(), bad
    for kw, word in ((dict(logp=ctypes.c_void_p(4100)), b"logp"), (dict(gamma=ctypes.c_void_p(4104)), b"gamma"),
                     (dict(work=ctypes.c_void_p(4104)), b"work"), (dict(tab=ctypes.c_void_p(4098)), b"a_pi"), (dict(loglik=ctypes.c_void_p(4100)), b"loglik"),
                     (dict(labels=fake, score=ctypes.c_void_p(4100)), b"score"), (dict(xi=ctypes.c_void_p(4100)), b"xi"),
                     (dict(g0=ctypes.c_void_p(4100)), b"gamma0")):
        assert call(**kw) == _lib.E_INVAL and word in err() and b"aligned" in err(), word
    need = per * 5 + rec
    assert call(wb=need - 1) == _lib.E_INVAL and b"too small" in err() and str(need).encode() in err()
    assert call(offs=i64([0, 3, 3 + mx + 1]), count=2) == _lib.E_UNSUPPORTED and b"recording 1" in err()
    many = [i * mx for i in range(2049)]                                                  # 2^31 steps in all
    assert call(offs=i64(many), count=2048) == _lib.E_UNSUPPORTED and b"in all" in err()


def test_shipped_kernel_resources(built_lib):
    """No scratch, no AGPR, at most 256 VGPRs; the staged segment (four float64 a step) fits the CU's 160 KiB of LDS."""
    res = _lib.kernel_resources("seg_posteriors_kernel")
    assert len(res) == 1, res
    (facts,) = res.values()
    assert facts["private_segment_fixed_size"] == 0 and facts["agpr_count"] == 0, facts
    seg = info(built_lib)[0]
    assert seg * 32 <= facts["group_segment_fixed_size"] <= 160 * 1024, facts
    assert 32 <= facts["vgpr_count"] <= 256, facts


# ---------------------------------------------------------------------------------------------------- GPU
def gpu_post(es, A, pi, labels=None, tables=True):
    """One ragged call through the C ABI on the list of (T, 4) numpy emissions -> (list of (T, 4) float32 gamma, logZ, score, Xi
    (N, 4, 4), gamma0 (N, 4)) as numpy; labels: a list of uint8 arrays."""
    lib = _lib.lib()
    n = len(es)
    offs = np.concatenate([[0], np.cumsum([e.shape[0] for e in es])]).astype(np.int64)
    total = int(offs[-1])
    arena = torch.from_numpy(np.concatenate(es)).cuda()
    tab = torch.from_numpy(np.concatenate([np.asarray(A, dtype=np.float32).ravel(), np.asarray(pi, dtype=np.float32).ravel()])).cuda()
    lab = torch.from_numpy(np.concatenate(labels).astype(np.uint8)).cuda() if labels is not None else None
    gamma = torch.full((total, 4), 7.0, dtype=torch.float32, device="cuda")
    f64 = dict(dtype=torch.float64, device="cuda")
    loglik, score = torch.full((n,), 7.0, **f64), torch.full((n,), 7.0, **f64)
    xi, g0 = torch.full((n, 16), 7.0, **f64), torch.full((n, 4), 7.0, **f64)
    _, _, per, rec = info(lib)
    work = torch.empty(per * total + rec * n, dtype=torch.uint8, device="cuda")
    rc = lib.hssfsst_posteriors(arena.data_ptr(), offs.ctypes.data_as(I64P), n, tab.data_ptr(), lab.data_ptr() if lab is not None else None,
                                gamma.data_ptr(), loglik.data_ptr(), score.data_ptr() if lab is not None else None,
                                xi.data_ptr() if tables else None, g0.data_ptr() if tables else None, work.data_ptr(), work.numel(), 0,
                                torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "hssfsst_posteriors")
    g = gamma.cpu().numpy()
    return ([g[offs[i]:offs[i + 1]] for i in range(n)], loglik.cpu().numpy(), score.cpu().numpy(), xi.cpu().numpy().reshape(n, 4, 4),
            g0.cpu().numpy())


def assert_meets_the_gates(es, A, pi, got, labels=None, what=""):
    n = len(es)
    wg, wlz, wxi = pc.forward_backward(es, [A] * n, [pi] * n)
    g, lz, sc, xi, g0 = got
    for i, e in enumerate(es):
        T = e.shape[0]
        onehot = np.eye(4)[labels[i]] if labels is not None else 0.0
        counts = pc.label_counts(labels[i]) if labels is not None else 0.0
        assert not np.isnan(g[i]).any(), (what, i, T)
        dg = np.abs(g[i].astype(np.float64) - (wg[i] - onehot)).max()
        assert dg <= GAMMA_GATE, (what, i, T, dg)
        if np.isinf(wlz[i]):
            assert lz[i] == wlz[i], (what, i, T, lz[i])
        else:
            assert abs(lz[i] - wlz[i]) <= z_gate(T, wlz[i]), (what, i, T, lz[i], wlz[i])
        assert np.abs(xi[i] - (wxi[i] - counts)).max() <= xi_gate(T), (what, i, T)
        assert np.abs(g0[i] - (wg[i][0] - (onehot[0] if labels is not None else 0.0))).max() <= 1e-12, (what, i, T)
        if labels is not None:
            want = pc.path_score(e, A, pi, labels[i])
            assert abs(sc[i] - want) <= z_gate(T, want), (what, i, T, sc[i], want)


def matrix_lengths():
    seg = consumer.posteriors_info()[0]
    lc = seg // LANES                                    # the steps one lane owns; a recording's step 0 is outside the segments
    return sorted({T for T in (1, 2, lc - 1, lc, lc + 1, lc + 2, seg - 1, seg, seg + 1, seg + 2, 2 * seg + 3, 2 * seg + 4, 5000) if T >= 1})


@pytest.mark.gpu
@pytest.mark.parametrize("kind", dc.KINDS)
def test_meets_the_gates_against_the_restatement(built_lib, kind):
    """Lengths around a lane's steps and the segment x {cyclic (.9, .1), dense, counted from labels} tables, one ragged call each,
    without labels and with labels the table allows: gamma (or gamma - onehot), logZ, score, Xi (or Xi - counts), gamma_0."""
    rng = np.random.default_rng(200)
    lens = matrix_lengths()
    es = [dc.emissions(kind, T, rng) for T in lens]
    cyc = [pc.legal_labels(T, rng) for T in lens]
    tables = (cyclic91() + (cyc,), (dc.dense_transitions(5), np.log(rng.dirichlet(np.ones(4))).astype(np.float32),
                                    [rng.integers(0, 4, size=T).astype(np.uint8) for T in lens]),
              transitions_from_labels(cyc) + (cyc,))
    for k, (A, pi, labels) in enumerate(tables):
        assert_meets_the_gates(es, A, pi, gpu_post(es, A, pi), what=(kind, k))
        assert_meets_the_gates(es, A, pi, gpu_post(es, A, pi, labels), labels, what=(kind, k, "labels"))


@pytest.mark.gpu
def test_special_emissions(built_lib):
    """An all -inf step: logZ = -inf, gamma = 0, no NaN, the neighbours untouched.  A forced path (advance only, start in state 0):
    gamma exactly one-hot.  Single NaN and -inf emissions; emissions spread to 200 below their step's maximum."""
    rng = np.random.default_rng(201)
    seg = consumer.posteriors_info()[0]
    A, pi = cyclic91()
    es = [dc.emissions("dirichlet1", T, rng) for T in (5, seg + 9, 40, 1)]
    es[1][seg + 2] = NINF
    es[3][0] = NINF
    got = gpu_post(es, A, pi)
    assert got[1][1] == NINF and got[1][3] == NINF and not got[0][1].any() and not got[0][3].any() and not got[3][1].any()
    assert_meets_the_gates(es, A, pi, got, what="all -inf step")

    step = np.full((4, 4), NINF, dtype=np.float32)
    for i in range(4):
        step[i, (i + 1) % 4] = -0.25
    es = [dc.emissions("dirichlet1", T, rng) for T in (1, 7, seg + 5)]
    g, lz, _, xi, _ = gpu_post(es, step, dc.STATE0)
    for e, gi in zip(es, g):
        path = np.arange(e.shape[0]) % 4
        assert np.array_equal(gi, np.eye(4, dtype=np.float32)[path])
    assert abs(lz[2] - pc.path_score(es[2], step, dc.STATE0, np.arange(seg + 5) % 4)) <= z_gate(seg + 5, lz[2])
    assert np.abs(xi[1] - pc.label_counts(np.arange(7) % 4)).max() <= xi_gate(7)

    es = [dc.emissions("dirichlet1", T, rng) for T in (30, seg + 3, 2)]
    es[0][4, 1], es[0][0, 2], es[1][seg, 0], es[1][seg + 2, 3], es[2][1, 1] = np.nan, NINF, np.nan, NINF, np.nan
    for A2, pi2 in ((A, pi), (dc.dense_transitions(9), dc.UNIFORM)):
        assert_meets_the_gates(es, A2, pi2, gpu_post(es, A2, pi2), what="NaN and -inf")

    es = []
    for T in (3, 100, seg + 77):
        e = -rng.uniform(0.0, 200.0, size=(T, 4)).astype(np.float32)
        e[np.arange(T), rng.integers(0, 4, size=T)] = 0.0
        e[::3] = np.where(e[::3] < 0, np.float32(-200.0), e[::3])
        es.append(e)
    for A2, pi2 in ((A, pi), (dc.dense_transitions(10), dc.UNIFORM)):
        assert_meets_the_gates(es, A2, pi2, gpu_post(es, A2, pi2), what="spread 200")


@pytest.mark.gpu
def test_batching_neighbours_and_determinism(built_lib):
    """More recordings than one launch takes (300 > 256); a recording's outputs are bit-identical alone, in another place of the
    list and next to other neighbours; the dense forms are the ragged call; two runs give the same bits."""
    rng = np.random.default_rng(202)
    seg = consumer.posteriors_info()[0]
    lens = [int(v) for v in rng.integers(1, 60, size=300)]
    lens[7], lens[270] = seg + 11, 2 * seg + 5
    es = [dc.emissions("dirichlet1", T, rng) for T in lens]
    labels = [pc.legal_labels(T, rng) for T in lens]
    A, pi = cyclic91()
    full = gpu_post(es, A, pi, labels)
    again = gpu_post(es, A, pi, labels)
    for a, b in zip(full[1:], again[1:]):
        assert np.array_equal(a, b)
    assert all(np.array_equal(a, b) for a, b in zip(full[0], again[0]))
    pick = [270, 7, 0, 299, 256, 255, 100]
    some = gpu_post([es[i] for i in pick], A, pi, [labels[i] for i in pick])
    for k, i in enumerate(pick):
        assert np.array_equal(some[0][k], full[0][i]), i
        for a, b in zip(some[1:], full[1:]):
            assert np.array_equal(a[k], b[i]), i
        alone = gpu_post([es[i]], A, pi, [labels[i]])
        assert np.array_equal(alone[0][0], full[0][i]) and all(np.array_equal(a[0], b[i]) for a, b in zip(alone[1:], full[1:])), i
    sub = [i for i in range(300) if lens[i] <= 40][:20]
    assert_meets_the_gates([es[i] for i in sub], A, pi, ([full[0][i] for i in sub],) + tuple(x[sub] for x in full[1:]),
                           [labels[i] for i in sub], what="batched")

    dense = np.stack([dc.emissions("dirichlet0.2", 37, rng) for _ in range(5)])
    t = torch.from_numpy(dense).cuda()
    rag = RaggedFeatures(t.reshape(-1, 4), torch.arange(6, dtype=torch.int64) * 37, 4, False)
    g_r, z_r = state_posteriors(rag, return_loglik=True)
    g_b, z_b = state_posteriors(t, return_loglik=True)
    assert isinstance(g_r, RaggedFeatures) and g_b.shape == (5, 37, 4) and g_b.dtype == torch.float32
    assert z_b.is_cuda and z_b.dtype == torch.float64 and z_b.shape == (5,)
    assert torch.equal(g_b.reshape(-1, 4), g_r.data) and torch.equal(z_b, z_r)
    g_1, z_1 = state_posteriors(t[3], return_loglik=True)
    assert torch.equal(g_1, g_b[3]) and z_1.shape == () and torch.equal(z_1, z_b[3])
    assert torch.equal(g_r[3], g_1) and torch.equal(state_posteriors(t), g_b)


@pytest.mark.gpu
def test_consistency_with_the_rest_of_the_pipeline(built_lib):
    """A = 0, pi = 0 on real log_softmax outputs: sequence_nll("sum") is nll_loss("sum") to 1e-6 relative and so is its gradient.
    Under the cycle argmax gamma differs from the per-step argmax.  logZ >= decode_states' score - T 2^-19."""
    torch.manual_seed(3)
    lens = [50, 333, 2100]
    logits = [torch.randn(T, 4).cuda() for T in lens]
    labels = [torch.randint(0, 4, (T,)).cuda() for T in lens]
    zero = (np.zeros((4, 4), dtype=np.float32), np.zeros(4, dtype=np.float32))

    def losses(fn):
        xs = [v.clone().requires_grad_(True) for v in logits]
        logp = torch.cat([torch.log_softmax(x, dim=1) for x in xs])
        loss = fn(logp)
        loss.backward()
        return float(loss.detach()), torch.cat([x.grad for x in xs])
    offs = torch.tensor([0, 50, 383, 2483])
    got, ggrad = losses(lambda lp: sequence_nll(RaggedFeatures(lp, offs, 4, False), labels, *zero, reduction="sum"))
    want, wgrad = losses(lambda lp: nn.functional.nll_loss(lp, torch.cat(labels), reduction="sum"))
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert float((ggrad - wgrad).abs().max()) <= 1e-6 * float(wgrad.abs().max())

    rng = np.random.default_rng(203)
    e = torch.from_numpy(dc.emissions("dirichlet1", 400, rng)).cuda()
    gamma, logz = state_posteriors(e, return_loglik=True)
    assert int((gamma.argmax(1) != e.argmax(1)).sum()) > 0
    assert float((gamma.sum(1) - 1).abs().max()) <= 4 * GAMMA_GATE
    for T in (1, 400, 5000):
        e = torch.from_numpy(dc.emissions("dirichlet1", T, rng)).cuda()
        _, sc = decode_states(e, return_scores=True)
        _, lz = state_posteriors(e, return_loglik=True)
        assert float(lz) >= float(sc) - T * 2.0 ** -19, (T, float(lz), float(sc))


def twin_grads(es, labels, A, pi, weights, reduction):
    """The float64 CPU twin of sequence_nll on the float32-rounded inputs: the value and the gradients in e, A, pi of
    sum_i weights_i nll_i ("none"), or of weights x the reduced loss."""
    tes = [torch.from_numpy(e).double().requires_grad_(True) for e in es]
    tA, tpi = (torch.from_numpy(np.asarray(v, dtype=np.float32)).double().requires_grad_(True) for v in (A, pi))
    nll = torch.stack([pc.torch_nll(e, y, tA, tpi) for e, y in zip(tes, labels)])
    total = sum(e.shape[0] for e in es)
    value = nll if reduction == "none" else (nll.sum() if reduction == "sum" else nll.sum() / total)
    (value * torch.as_tensor(weights, dtype=torch.float64)).sum().backward()
    return value.detach(), [e.grad for e in tes], tA.grad, tpi.grad


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ("mean", "sum", "none"))
def test_gradients_against_the_cpu_twin(built_lib, reduction):
    """sequence_nll on a ragged list with learnable float64 A and pi on the device, a non-unit incoming gradient (<= 1): the value
    and the gradients in logp (2^-22 absolute), A and pi (1e-9 of each tensor's maximum) against float64 autograd.  The value of
    "none" is float64 on both sides, each a difference of two sums of T terms of size |score|: 1e-11 relative leaves it room;
    "mean" and "sum" are float32."""
    rng = np.random.default_rng(204)
    lens = [1, 2, 9, 150, 64]
    es = [dc.emissions("dirichlet1", T, rng) for T in lens]
    for k, (A, pi) in enumerate((cyclic91(), (dc.dense_transitions(11), np.log(rng.dirichlet(np.ones(4))).astype(np.float32)))):
        labels = [pc.legal_labels(T, rng) if k == 0 else rng.integers(0, 4, size=T).astype(np.uint8) for T in lens]
        weights = rng.uniform(0.25, 1.0, size=len(lens)) if reduction == "none" else 0.75
        want, wge, wgA, wgpi = twin_grads(es, labels, A, pi, weights, reduction)
        logp = [torch.from_numpy(e).cuda().requires_grad_(True) for e in es]
        arena = torch.cat(logp)
        offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64)
        gA = torch.from_numpy(A).double().cuda().requires_grad_(True)
        gpi = torch.from_numpy(pi).double().cuda().requires_grad_(True)
        got = sequence_nll(RaggedFeatures(arena, offs, 4, False), [torch.from_numpy(y) for y in labels], gA, gpi, reduction=reduction)
        assert got.dtype == (torch.float64 if reduction == "none" else torch.float32) and got.shape == want.shape
        assert torch.allclose(got.double().cpu(), want, rtol=1e-6 if reduction != "none" else 1e-11, atol=0)
        (got.double() * torch.as_tensor(weights, dtype=torch.float64).cuda()).sum().backward()
        for i in range(len(lens)):
            assert float((logp[i].grad.double().cpu() - wge[i]).abs().max()) <= 2.0 ** -22, (k, i)
        assert float((gA.grad.cpu() - wgA).abs().max()) <= 1e-9 * float(wgA.abs().max()), k
        assert float((gpi.grad.cpu() - wgpi).abs().max()) <= 1e-9 * float(wgpi.abs().max()), k
        assert (gA.grad[torch.isinf(gA.detach())] == 0).all()


@pytest.mark.gpu
def test_label_kinds_and_argument_checks(built_lib):
    """The label forms give the same loss; mismatched lengths and host labels outside 0..3 raise ValueError, as do bad inputs."""
    rng = np.random.default_rng(205)
    dense = torch.from_numpy(np.stack([dc.emissions("dirichlet1", 12, rng) for _ in range(3)])).cuda()
    y = np.stack([pc.legal_labels(12, rng) for _ in range(3)])
    rag = RaggedFeatures(dense.reshape(-1, 4), torch.arange(4, dtype=torch.int64) * 12, 4, False)
    want = sequence_nll(dense, torch.from_numpy(y), reduction="none")
    forms = ((rag, [torch.from_numpy(r).long() for r in y]), (rag, [torch.from_numpy(r).cuda() for r in y]),
             (rag, RaggedStates(torch.from_numpy(y.reshape(-1)).cuda(), rag.offsets)), (rag, torch.from_numpy(y.reshape(-1)).cuda()),
             (dense, torch.from_numpy(y).cuda().int()))
    for lp, lab in forms:
        assert torch.equal(sequence_nll(lp, lab, reduction="none"), want)
    assert torch.equal(sequence_nll(dense[1], y[1], reduction="none"), want[1:2])
    for lp, lab in ((rag, [torch.from_numpy(r) for r in y[:2]]), (rag, [torch.from_numpy(y[0]), torch.from_numpy(y[1][:5]), torch.from_numpy(y[2])]),
                    (dense, torch.from_numpy(y[:, :7])), (dense, torch.from_numpy(y.astype(np.int64) + 4)), (dense, torch.from_numpy(y).float()),
                    (rag, RaggedStates(torch.from_numpy(y.reshape(-1)).cuda(), torch.tensor([0, 10, 24, 36])))):
        with pytest.raises(ValueError):
            sequence_nll(lp, lab)
    with pytest.raises(ValueError):
        sequence_nll(dense, torch.from_numpy(y), reduction="median")
    for bad in (dense.double(), dense.cpu(), dense[:, :, :3]):
        with pytest.raises(ValueError):
            state_posteriors(bad)
    with pytest.raises(ValueError):
        state_posteriors(dense, transitions=np.zeros((4, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        state_posteriors(dense, np.zeros((3, 4), dtype=np.float32), np.zeros(4, dtype=np.float32))
    assert not state_posteriors(dense.requires_grad_(True)).requires_grad


@pytest.mark.gpu
def test_training_end_to_end():
    """A tiny HipSegmenterHead (H 16), three synthetic recordings of different lengths, twelve Adam steps on
    sequence_nll(head.ragged(feats), labels) with learnable transitions: the loss falls, and every loss is within 1e-4 relative of
    the float64 CPU twin's (the gate of tests/test_segmenter_train_ragged.py's twelve-step test)."""
    from tests.test_segmenter_train_ragged import looped64, twin64
    lens = [100, 260, 173]
    sig = synth.pcg_windows(3, 400, seed=23)
    recs = [torch.from_numpy(sig[i, :n].copy()).cuda() for i, n in enumerate(lens)]
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True)
    feats = tf.ragged(recs)
    xs = [feats[i].detach().clone() for i in range(3)]
    rng = np.random.default_rng(206)
    labels = [pc.legal_labels(T, rng) for T in lens]
    torch.manual_seed(5)
    base = SegmenterHead(44, 16, 1)
    head = HipSegmenterHead(44, 16, 1, h0=base.h0.clone(), c0=base.c0.clone())
    head.load_state_dict(base.state_dict())
    head.cuda()
    ref = twin64(base)
    A0, pi0 = cyclic91()

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

    def twin_loss(A, pi):
        # (the kernel sees the tables rounded to float32; a straight-through rounding keeps the twin's gradient; -inf stays)
        A32 = A + torch.nan_to_num(A.float().double() - A, nan=0.0).detach()
        pi32 = pi + torch.nan_to_num(pi.float().double() - pi, nan=0.0).detach()
        lp = looped64(ref, xs64, ref.h0, ref.c0)
        offs = np.concatenate([[0], np.cumsum(lens)])
        return sum(pc.torch_nll(lp[offs[i]:offs[i + 1]], labels[i], A32, pi32) for i in range(3)) / total
    want = fit(ref, twin_loss, "cpu")
    ylist = [torch.from_numpy(y) for y in labels]
    got = fit(head, lambda A, pi: sequence_nll(head.ragged(xs), ylist, A, pi), "cuda")
    print("twin", [f"{v:.5f}" for v in want], "hip", [f"{v:.5f}" for v in got])
    assert all(abs(g_ - w) <= 1e-4 * abs(w) for g_, w in zip(got, want)), (got, want)
    assert got[-1] < got[0] and want[-1] < want[0]


@pytest.mark.gpu
def test_integration_with_the_segmenter_and_stream_order():
    """state_posteriors right behind the segmenter call, with no synchronisation in between, and on a side stream, gives what the
    synchronised sequence gives; segment_recordings(posteriors=True) is that; posteriors exclude decode."""
    torch.manual_seed(31)
    seg = SegmenterHead(44, 16, 3).eval().hip()
    sig = synth.pcg_windows(3, 2000, seed=22)
    recs = [torch.from_numpy(sig[i, :n].copy()).cuda() for i, n in enumerate((100, 700, 333))]
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True)
    feats = tf.ragged(recs)
    logp = seg.ragged(feats)
    torch.cuda.synchronize()
    gamma, logz = state_posteriors(logp, return_loglik=True)
    torch.cuda.synchronize()
    host = logp.data.cpu().numpy()
    offs = logp.offsets.tolist()
    es = [host[offs[i]:offs[i + 1]] for i in range(3)]
    A, pi = cyclic_transitions()
    wg, wlz, _ = pc.forward_backward(es, [A] * 3, [pi] * 3)
    for i in range(3):
        assert np.abs(gamma[i].cpu().numpy().astype(np.float64) - wg[i]).max() <= GAMMA_GATE
        assert abs(float(logz[i]) - wlz[i]) <= z_gate(es[i].shape[0], wlz[i])
    unsynced = state_posteriors(seg.ragged(feats))       # enqueued behind the segmenter on the current stream
    assert torch.equal(unsynced.data, gamma.data)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = state_posteriors(seg.ragged(feats))
    side.synchronize()
    assert torch.equal(on_side.data, gamma.data)
    e2e = segment_recordings(tf, seg, recs, posteriors=True)
    assert isinstance(e2e, RaggedFeatures) and torch.equal(e2e.data, gamma.data) and e2e.lengths().tolist() == [100, 700, 333]
    A2, pi2 = cyclic91()
    custom = segment_recordings(tf, seg, recs, posteriors=(A2, pi2))
    assert torch.equal(custom.data, state_posteriors(logp, A2, pi2).data) and not torch.equal(custom.data, gamma.data)
    assert torch.equal(segment_recordings(tf, seg, recs).data, logp.data)                 # the default: unchanged
    for kw in (dict(decode=True, posteriors=True), dict(decode=(A, pi), posteriors=True)):
        with pytest.raises(ValueError):
            segment_recordings(tf, seg, recs, **kw)
