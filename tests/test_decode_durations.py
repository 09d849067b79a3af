"""Log-probs -> state sequences under per-state duration scores: hssfsst_decode_durations (C ABI), consumer.decode_durations and
its helpers.

The contract is exact: int64 fixed point (2^-20), the tie rules of include/hssfsst.h -- restated in numpy in
tests/duration_cases.py.  The GPU tests ask for equality with that restatement in every state and every int64 score.  CPU tests
check the restatement itself (against brute-force enumeration, against the first-order restatement on geometric tables, against
float64), the ABI, the argument errors (all raised before any device work), the host helpers, the kernel's ring with its lanes
simulated under sanitizers (tests/native/decode_durations_check.cpp) and the shipped kernel's resources."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, consumer, synth
from heart_sounds_segmentation_amd.consumer import (SegmenterHead, cyclic_transitions, decode_durations, decode_states, durations_from_labels,
                                                    edge_durations, gaussian_durations, segment_recordings)
from heart_sounds_segmentation_amd.transforms import FSST, RaggedFeatures
from tests import decode_cases as dc
from tests import duration_cases as du

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hssfsst.h")
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")
NINF = float("-inf")
FP = ctypes.POINTER(ctypes.c_float)


def i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def f32(values):
    return (ctypes.c_float * len(values))(*values)


def limits(lib):
    D, mx, per = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.hssfsst_decode_durations_info(ctypes.byref(D), ctypes.byref(mx), ctypes.byref(per)) == 0
    return D.value, mx.value, per.value


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_library_and_info(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    assert "int hssfsst_decode_durations(" in text and "int hssfsst_decode_durations_info(" in text
    fn = built_lib.hssfsst_decode_durations
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 14
    D, mx, per = limits(built_lib)
    assert D >= 2048 and mx == 2 ** 24 and per == 8
    assert built_lib.hssfsst_decode_durations_info(None, None, None) == 0
    assert consumer.decode_durations_info() == (D, mx, per)
    import heart_sounds_segmentation_amd as pkg
    for name in ("decode_durations", "edge_durations", "gaussian_durations", "durations_from_labels"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(consumer, name)


@pytest.mark.parametrize("kind", ("dirichlet1", "zeros", "integers"))
def test_restatement_equals_brute_force(kind):
    """Every segmentation enumerated (T <= 8, D <= 5): the loop's score is the best one and its path attains it; where nothing
    fits, both say so.  30 % of dur forbidden; cyclic and dense A; zeros and integers give heavy ties."""
    rng = np.random.default_rng(21)
    fits = 0
    for case in range(12):
        T, D = int(rng.integers(1, 9)), int(rng.integers(1, 6))
        A = dc.cyclic() if case % 2 else dc.dense_transitions(case)
        pi = dc.STATE0 if case % 3 == 0 else dc.UNIFORM
        dur, edge = du.random_tables(rng, D, forbidden=0.3)
        if case % 4 == 3:
            edge = dur.copy()                            # forbidden entries at the ends too
        e = dc.emissions(kind, T, rng)
        path, score = du.decode(e, A, pi, dur, edge)
        best, paths = du.brute_force(e, A, pi, dur, edge)
        assert int(score) == best, (case, T, D)
        if best == du.NEG:
            assert not path.any()
            continue
        fits += 1
        assert tuple(path.tolist()) in paths, (case, T, D, path.tolist())
        assert du.path_score(e, A, pi, dur, edge, path) == best
    assert fits >= 8


def test_restatement_equals_the_first_order_restatement_on_geometric_tables():
    """dur[j][d] = edge[j][d] = -0.5 (d - 1) with D >= T scores a run as d - 1 stays under A[i][i] = -0.5: every path has the
    same int64 score in both models (-0.5, -1.25 and their multiples are exact in float32 and multiples of 2^-20)."""
    rng = np.random.default_rng(22)
    A = du.geometric_transitions()
    for T in (1, 2, 37, 150):
        dur, edge = du.geometric_tables(max(T, 3))
        for kind in ("dirichlet1", "integers"):
            e = dc.emissions(kind, T, rng)
            for pi in (dc.UNIFORM, dc.STATE0):
                path, score = du.decode(e, A, pi, dur, edge)
                _, want = dc.viterbi([e], [A], [pi])
                assert int(score) == int(want[0]), (T, kind)
                assert du.path_score(e, A, pi, dur, edge, path) == int(score)


@pytest.mark.parametrize("kind", ("dirichlet1", "dirichlet0.2", "integers"))
def test_restatement_is_within_the_quantisation_bound_of_float64(kind):
    """The path of the quantised loop, scored in float64 on the unquantised inputs, is within 3 T x 2^-20 of the float64 loop's
    optimum: a path has at most 3 T terms (pi, T emissions, at most T run scores, at most T - 1 moves), each moved by at most
    2^-21 by the quantiser, on each of the two paths compared.  Derived, not measured."""
    rng = np.random.default_rng(23)
    A, pi = dc.dense_transitions(3), dc.UNIFORM
    for T, D in ((1, 4), (2, 4), (50, 7), (777, 60), (1500, 300)):
        dur, edge = du.random_tables(rng, D, forbidden=0.2)
        e = np.maximum(dc.emissions(kind, T, rng), np.float32(-100.0))                    # (a Dirichlet(0.2) draw may be exactly 0)
        path, _ = du.decode(e, A, pi, dur, edge, exact=True)
        fpath, fs = du.decode(e, A, pi, dur, edge, exact=False)
        assert np.isfinite(fs)
        assert abs(du.path_score(e, A, pi, dur, edge, fpath, exact=False) - fs) <= 1e-9 * max(1.0, abs(fs))
        assert du.path_score(e, A, pi, dur, edge, path, exact=False) >= fs - 3 * T * 2.0 ** -20, (kind, T, D)


def test_host_helpers_against_hand_written_answers():
    dur = np.array([[-3, -1, -2, NINF], [NINF, NINF, -5, -4], [0, -1, -2, -3], [NINF, -2, NINF, -7]], dtype=np.float32)
    want = np.array([[-1, -1, -2, NINF], [-4, -4, -4, -4], [0, -1, -2, -3], [-2, -2, -7, -7]], dtype=np.float32)
    got = edge_durations(dur)
    assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want)
    assert np.array_equal(edge_durations(torch.from_numpy(dur)), want)
    with pytest.raises(ValueError):
        edge_durations(np.zeros((3, 4), dtype=np.float32))

    g = gaussian_durations(3.0, 1.0, 5)
    assert g.shape == (4, 5) and g.dtype == np.float32
    w = np.exp(-0.5 * (np.arange(1, 6) - 3.0) ** 2)
    assert np.allclose(g, np.tile(np.log(w / w.sum()), (4, 1)), rtol=1e-6, atol=0)
    g = gaussian_durations([2, 3, 4, 5], [1, 2, 1, 0.5], 6, min_duration=3)
    assert np.isneginf(g[:, :2]).all() and np.isfinite(g[:, 2:]).all()
    assert np.allclose(np.exp(g.astype(np.float64)).sum(axis=1), 1.0, rtol=1e-6)
    w = np.exp(-0.5 * ((np.arange(3, 7) - 3.0) / 2.0) ** 2)
    assert np.allclose(g[1, 2:], np.log(w / w.sum()), rtol=1e-6) and g[3].argmax() == 4
    for bad in (dict(mean=3, std=0.0, max_duration=5), dict(mean=3, std=1, max_duration=5, min_duration=6), dict(mean=3, std=1, max_duration=0)):
        with pytest.raises(ValueError):
            gaussian_durations(**bad)

    # runs: (0 x 5) 1 x 3, 2 x 1, 3 x 2, 0 x 2, 1 x 1, 2 x 1 (3 x 1); (2 x 9) 3 x 2, 0 x 4 (1 x 1); (3 x 3) -- the bracketed ones, the
    # first and the last of their sequence, are censored.  Interior: state 0: 2, 4; state 1: 3, 1; state 2: 1, 1; state 3: 2, 2
    labels = [torch.tensor([0] * 5 + [1] * 3 + [2] + [3] * 2 + [0] * 2 + [1] + [2] + [3]),
              np.array([2] * 9 + [3] * 2 + [0] * 4 + [1]),
              torch.tensor([3, 3, 3], dtype=torch.uint8)]
    h = durations_from_labels(labels, 6, fit="histogram")
    want = np.full((4, 6), NINF)
    want[0, 1], want[0, 3] = np.log(1 / 2), np.log(1 / 2)            # state 0: runs of 2 and 4
    want[1, 2], want[1, 0] = np.log(1 / 2), np.log(1 / 2)            # state 1: runs of 3 and 1
    want[2, 0] = 0.0                                                 # state 2: runs of 1 and 1
    want[3, 1] = 0.0                                                 # state 3: runs of 2 and 2
    assert h.dtype == np.float32 and np.allclose(h, want.astype(np.float32), rtol=1e-6, atol=0) and np.array_equal(np.isneginf(h), np.isneginf(want))
    g = durations_from_labels(labels, 6)                             # means 3, 2, 1, 2; std 1, 1, 0 -> 0.5, 0 -> 0.5
    assert np.allclose(g, gaussian_durations([3, 2, 1, 2], [1, 1, 0.5, 0.5], 6), rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        durations_from_labels(labels, 3, fit="histogram")            # a run of 4
    with pytest.raises(ValueError):
        durations_from_labels([torch.tensor([0, 1, 1, 2])], 6)       # states without an interior run
    with pytest.raises(ValueError):
        durations_from_labels(labels, 6, fit="kernel")
    with pytest.raises(ValueError):
        durations_from_labels([torch.tensor([0, 4, 1])], 6)


def test_argument_errors_need_no_device(built_lib):
    F = built_lib.hssfsst_decode_durations
    err = built_lib.hssfsst_last_error
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below ends before any device work
    A, pi = (np.ascontiguousarray(v) for v in cyclic_transitions())
    D = 4
    dur = np.zeros((4, D), dtype=np.float32)
    cA, cpi, cd = f32(A.ravel().tolist()), f32(pi.tolist()), f32(dur.ravel().tolist())
    ok = i64([0, 5])
    big = 1 << 40

    def call(logp=fake, offs=ok, count=1, tA=cA, tpi=cpi, td=cd, te=cd, md=D, states=fake, work=fake, wb=big, device=0):
        return F(logp, offs, count, tA, tpi, td, te, md, states, None, work, wb, device, None)

    assert call(offs=i64([0]), count=0) == 0                                              # count == 0: nothing to do
    for kw, word in ((dict(logp=None), b"logp"), (dict(offs=None), b"offsets"), (dict(tA=None), b"transitions"), (dict(tpi=None), b"initial"),
                     (dict(td=None), b"durations"), (dict(te=None), b"edge"), (dict(states=None), b"states"), (dict(work=None), b"workspace")):
        assert call(**kw) == _lib.E_INVAL and word in err() and b"NULL" in err(), word
    assert call(count=-1) == _lib.E_INVAL and b"negative" in err()
    assert call(device=-1) == _lib.E_INVAL and b"device" in err()
    assert call(offs=i64([2, 4])) == _lib.E_INVAL and b"offsets[0]" in err()
    for bad in ([0, 5, 5], [0, 7, 3], [0, 4, 4, 9]):
        assert call(offs=i64(bad), count=len(bad) - 1) == _lib.E_INVAL and b"index 2" in err(), bad
    nanA = A.copy()
    nanA[2, 3] = np.nan
    assert call(tA=f32(nanA.ravel().tolist())) == _lib.E_INVAL and b"transitions[2][3] is NaN" in err()
    assert call(tpi=f32([0, np.nan, 0, 0])) == _lib.E_INVAL and b"initial[1] is NaN" in err()
    nand = dur.copy()
    nand[3, 2] = np.nan
    assert call(td=f32(nand.ravel().tolist())) == _lib.E_INVAL and b"durations[3][2] is NaN" in err()
    assert call(te=f32(nand.ravel().tolist())) == _lib.E_INVAL and b"edge[3][2] is NaN" in err()
    mx = limits(built_lib)[0]
    for md in (0, -3, mx + 1):
        assert call(md=md) == _lib.E_INVAL and b"max_duration" in err(), md
    dead = dur.copy()
    dead[2, :] = NINF
    assert call(td=f32(dead.ravel().tolist())) == _lib.E_INVAL and b"row 2 of durations" in err()
    assert call(te=f32(dead.ravel().tolist())) == _lib.E_INVAL and b"row 2 of edge" in err()
    stayA = A.copy()
    stayA[1, 2] = NINF                                   # row 1 keeps its diagonal only, which the decoder ignores
    assert call(tA=f32(stayA.ravel().tolist())) == _lib.E_INVAL and b"row 1 of transitions" in err() and b"off-diagonal" in err()
    assert call(tpi=f32([NINF] * 4)) == _lib.E_INVAL and b"initial is all -inf" in err()
    assert call(logp=ctypes.c_void_p(4100)) == _lib.E_INVAL and b"logp" in err() and b"aligned" in err()
    assert call(work=ctypes.c_void_p(4104)) == _lib.E_INVAL and b"workspace" in err() and b"aligned" in err()
    need = 8 * (5 + 8 * D)
    assert call(wb=need - 1) == _lib.E_INVAL and b"too small" in err() and str(need).encode() in err()
    assert call(offs=i64([0, 3, 3 + 2 ** 24 + 1]), count=2) == _lib.E_UNSUPPORTED and b"recording 1" in err()
    many = [i * 2 ** 24 for i in range(129)]                                              # 2^31 steps in all
    assert call(offs=i64(many), count=128) == _lib.E_UNSUPPORTED and b"in all" in err()


def test_decode_durations_ring_under_sanitizers(tmp_path):
    """csrc/decode_durations_layout.hpp in a program of its own (tests/native/decode_durations_check.cpp) built with
    -fsanitize=address,undefined: the kernel's ring with its lanes simulated equals the sequential pull loop, no index leaves the
    ring, the table or the workspace, and no int64 sum overflows."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "decode_durations_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "decode_durations_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "decode durations check ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_shipped_kernel_resources(built_lib):
    """No scratch, no AGPR; the ring, its 16-bit arguments and the staged emissions fit the CU's 160 KiB of LDS and hold D = 2048:
    4 x 2049 candidates of 8 bytes and 4 x 2049 arguments of 2; a lane's sixteen dur values stay in registers, and two waves per
    SIMD (512 lanes) leave each at most 256."""
    res = _lib.kernel_resources("seg_decode_durations_kernel")
    assert len(res) == 1, res
    (facts,) = res.values()
    assert facts["private_segment_fixed_size"] == 0 and facts["agpr_count"] == 0, facts
    assert 4 * 2049 * (8 + 2) <= facts["group_segment_fixed_size"] <= 160 * 1024, facts
    assert 32 <= facts["vgpr_count"] <= 256, facts                                        # 16 int64 of dur alone are 32
    fill = _lib.kernel_resources("seg_durations_fill_kernel")
    assert len(fill) == 1 and next(iter(fill.values()))["private_segment_fixed_size"] == 0, fill


# ---------------------------------------------------------------------------------------------------- GPU
def gpu_decode(es, A, pi, dur, edge, slack=0):
    """One ragged call through the C ABI on the list of (T, 4) numpy emissions -> (list of numpy paths, int64 scores)."""
    offs = np.concatenate([[0], np.cumsum([e.shape[0] for e in es])]).astype(np.int64)
    arena = torch.from_numpy(np.concatenate(es)).cuda()
    states = torch.full((int(offs[-1]),), 255, dtype=torch.uint8, device="cuda")
    scores = torch.zeros(len(es), dtype=torch.int64, device="cuda")
    A, pi, dur, edge = (np.ascontiguousarray(v, dtype=np.float32) for v in (A, pi, dur, edge))
    D = dur.shape[1]
    work = torch.empty(8 * (int(offs[-1]) + 8 * D) + slack, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().hssfsst_decode_durations(arena.data_ptr(), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(es),
                                             A.ctypes.data_as(FP), pi.ctypes.data_as(FP), dur.ctypes.data_as(FP), edge.ctypes.data_as(FP), D,
                                             states.data_ptr(), scores.data_ptr(), work.data_ptr(), work.numel(), 0,
                                             torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "hssfsst_decode_durations")
    st = states.cpu().numpy()
    return [st[offs[i]:offs[i + 1]] for i in range(len(es))], scores.cpu().numpy()


def assert_equal_lists(want, wscore, got, gscore, what):
    for n, (w, g) in enumerate(zip(want, got)):
        bad = np.flatnonzero(w != g)
        assert bad.size == 0, (what, n, w.shape[0], int(bad[0]), int(w[bad[0]]), int(g[bad[0]]))
    assert np.array_equal(wscore, gscore), (what, wscore.tolist(), gscore.tolist())


def matrix_lengths(D):
    R = D + 1                                            # the ring
    return sorted({T for T in (1, 2, D - 1, D, D + 1, 2 * R + 3, 5000) if T >= 1})


@pytest.mark.gpu
@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("D", (1, 2, 255, 256, 257, 2048))
def test_equals_the_restatement_exactly(built_lib, D, kind):
    """Lengths x {cyclic, dense A} x {uniform pi, state 0 only} x {minimum duration 1, 40}, one ragged call each: every state and
    every int64 score equals the numpy restatement -- also where a recording fits no segmentation (D = 1 or 2 under the cycle)."""
    rng = np.random.default_rng(100 + D)
    es = [dc.emissions(kind, T, rng) for T in matrix_lengths(D)]
    for A, pi, dmin in ((dc.cyclic(), dc.UNIFORM, 1), (dc.dense_transitions(7), dc.STATE0, 40), (dc.cyclic(), dc.STATE0, 40),
                        (dc.dense_transitions(8), dc.UNIFORM, 1)):
        dur, edge = du.random_tables(rng, D, forbidden=0.3, min_duration=dmin)
        want, wscore = du.decode_list(es, A, pi, dur, edge)
        got, gscore = gpu_decode(es, A, pi, dur, edge)
        assert_equal_lists(want, wscore, got, gscore, (kind, D, dmin, pi.tolist()))
        for g, sc in zip(got, gscore):
            if sc != du.NEG:
                assert max(d for _, d in du.runs_of(g)) <= D
                assert pi is dc.UNIFORM or g[0] == 0


@pytest.mark.gpu
def test_a_recording_no_segmentation_fits(built_lib):
    """A user edge that lets a cut-off run last one step only, interior runs of exactly D = 9: T = 50 is not 2 + 9 k, T = 47 is.
    The first gets the score NEG and every state 0; its neighbours are decoded as usual."""
    rng = np.random.default_rng(31)
    D = 9
    dur = np.full((4, D), NINF, dtype=np.float32)
    dur[:, D - 1] = 0.0
    edge = np.full((4, D), NINF, dtype=np.float32)
    edge[:, 0] = 0.0
    es = [dc.emissions("dirichlet1", T, rng) for T in (47, 50, 11, 3)]
    A, pi = dc.dense_transitions(4), dc.UNIFORM
    want, wscore = du.decode_list(es, A, pi, dur, edge)
    got, gscore = gpu_decode(es, A, pi, dur, edge)
    assert_equal_lists(want, wscore, got, gscore, "no fit")
    assert gscore[1] == du.NEG and not got[1].any() and gscore[3] == du.NEG and not got[3].any()
    assert gscore[0] != du.NEG and gscore[2] != du.NEG and [d for _, d in du.runs_of(got[0])] == [1, 9, 9, 9, 9, 9, 1]
    out, sc = decode_durations(torch.from_numpy(es[1]).cuda(), dur, A, pi, edge=edge, return_scores=True)
    assert sc == NINF and not out.any()


@pytest.mark.gpu
def test_special_emissions(built_lib):
    """-inf and NaN count as -32768, +inf and values past the clamp as the clamp: equal to the restatement, and finite scores."""
    rng = np.random.default_rng(32)
    D = 300
    es = [dc.emissions("dirichlet1", T, rng) for T in (40, 700, 1300, 9)]
    es[0][10, :] = np.nan
    es[1][512, 1] = NINF
    es[1][7, 2] = np.inf
    es[2][513, 0] = 1e6
    es[2][1024, 3] = -1e6
    es[2][5, 1] = 40000.0
    es[3][4, :] = NINF                                   # an all -inf step costs 32768, it does not forbid the recording
    for A, pi in ((dc.cyclic(), dc.UNIFORM), (dc.dense_transitions(8), dc.STATE0)):
        dur, edge = du.random_tables(rng, D, forbidden=0.3)
        want, wscore = du.decode_list(es, A, pi, dur, edge)
        got, gscore = gpu_decode(es, A, pi, dur, edge)
        assert_equal_lists(want, wscore, got, gscore, "special")
        assert (gscore != du.NEG).all() and gscore[3] < -32768 * 2 ** 20


@pytest.mark.gpu
def test_more_recordings_than_one_launch_takes(built_lib):
    """The offsets travel as kernel arguments, 256 recordings per launch: 256, 257 and 300 short recordings, scores included; a
    workspace with room to spare and D = 500, whose table takes five fill launches."""
    rng = np.random.default_rng(33)
    es = [dc.emissions("dirichlet1", int(T), rng) for T in rng.integers(1, 12, size=300)]
    A, pi = dc.dense_transitions(10), dc.UNIFORM
    for D, counts in ((6, (256, 257, 300)), (500, (300,))):
        dur, edge = du.random_tables(rng, D, forbidden=0.3)
        want, wscore = du.decode_list(es, A, pi, dur, edge)
        for count in counts:
            got, gscore = gpu_decode(es[:count], A, pi, dur, edge, slack=4096)
            assert_equal_lists(want[:count], wscore[:count], got, gscore, (D, count))


@pytest.fixture(scope="module")
def mixed(built_lib):
    """15 recordings of mixed lengths as one arena on the GPU, a Gaussian table with D = 130, and their decoding as one list
    (computed once, never changed)."""
    lens = [1, 2, 15, 64, 131, 40, 333, 1100, 5, 130, 64, 7, 7, 3, 600]
    rng = np.random.default_rng(34)
    es = [torch.from_numpy(dc.emissions("dirichlet1", T, rng)).cuda() for T in lens]
    offs = np.concatenate([[0], np.cumsum(lens)])
    rag = RaggedFeatures(torch.cat(es), torch.tensor(offs, dtype=torch.int64), 4, False)
    dur = gaussian_durations([12, 30, 9, 60], [3, 8, 2, 20], 130, min_duration=2)
    out = decode_durations(rag, dur, return_scores=True)
    return es, rag, dur, out[0], out[1]


@pytest.mark.gpu
def test_a_recording_does_not_depend_on_its_neighbours(mixed):
    es, rag, dur, states, scores = mixed
    assert isinstance(states, consumer.RaggedStates) and states.data.dtype == torch.uint8 and states.data.shape == (rag.data.shape[0],)
    assert states.lengths().tolist() == rag.lengths().tolist() and scores.dtype == torch.float64 and scores.shape == (len(es),)
    A, pi = cyclic_transitions()
    want, wscore = du.decode_list([e.cpu().numpy() for e in es], A, pi, dur, edge_durations(dur))      # the defaults, spelled out
    rev = RaggedFeatures(torch.cat(es[::-1]), torch.tensor(np.concatenate([[0], np.cumsum([e.shape[0] for e in es[::-1]])])), 4, False)
    back, back_scores = decode_durations(rev, dur, return_scores=True)
    for i, e in enumerate(es):
        assert np.array_equal(states[i].cpu().numpy(), want[i]) and scores[i] == wscore[i] / 2.0 ** 20, i
        alone, sc = decode_durations(e, torch.from_numpy(dur), return_scores=True)
        assert alone.shape == (e.shape[0],) and torch.equal(alone, states[i]), i
        assert sc == scores[i] and back_scores[len(es) - 1 - i] == scores[i]
        assert torch.equal(back[len(es) - 1 - i], states[i]), i


@pytest.mark.gpu
def test_dense_forms_equal_the_ragged_call(mixed):
    dur = mixed[2]
    rng = np.random.default_rng(35)
    B, T = 5, 521
    x = torch.from_numpy(np.stack([dc.emissions("dirichlet1", T, rng) for _ in range(B)])).cuda()
    A, pi = dc.dense_transitions(9), dc.UNIFORM
    edge = np.zeros_like(dur)
    rag = decode_durations(RaggedFeatures(x.reshape(B * T, 4), torch.arange(B + 1) * T, 4, False), dur, A, pi, edge)
    got = decode_durations(x, dur, A, pi, edge)
    assert got.shape == (B, T) and got.dtype == torch.uint8 and torch.equal(got.reshape(-1), rag.data)
    for b in range(B):
        assert torch.equal(decode_durations(x[b], dur, torch.from_numpy(A), torch.from_numpy(pi), torch.from_numpy(edge)), rag[b])
    assert rag.padded().shape == (B, T) and torch.equal(rag.padded(), got)


@pytest.mark.gpu
def test_score_equals_decode_states_on_geometric_tables(built_lib):
    """The new kernel crossed with the tested one, on the device: dur = edge = -0.5 (d - 1), D >= T, against A[i][i] = -0.5 --
    every path scores alike in both models, so the int64 optima are equal."""
    rng = np.random.default_rng(36)
    lens = (1, 2, 37, 150)
    es = [dc.emissions("dirichlet1", T, rng) for T in lens]
    A = du.geometric_transitions()
    dur, edge = du.geometric_tables(150)
    for pi in (dc.UNIFORM, dc.STATE0):
        got, gscore = gpu_decode(es, A, pi, dur, edge)
        offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]))
        first, fscore = decode_states(RaggedFeatures(torch.from_numpy(np.concatenate(es)).cuda(), offs, 4, False), A, pi, return_scores=True)
        assert np.array_equal(gscore.astype(np.float64) / 2.0 ** 20, fscore.numpy()), (gscore.tolist(), fscore.tolist())
        for i, g in enumerate(got):                      # (Dirichlet emissions: no ties, so the paths agree too)
            assert np.array_equal(g, first[i].cpu().numpy()), i


@pytest.mark.gpu
def test_a_minimum_duration_holds(built_lib):
    """400 steps of Dirichlet(1) emissions: decode_states under the cycle flickers (a run of one step); under a 20-step minimum
    with D = 64 every interior run has 20 .. 64 steps, the cut-off ones at most 64, and every move advances the cycle."""
    e = torch.from_numpy(dc.emissions("dirichlet1", 400, np.random.default_rng(37))).cuda()
    dur, edge = du.minimum_duration_tables(64, 20)
    runs = du.runs_of(decode_durations(e, dur, edge=edge).cpu().numpy())
    steps = [d for _, d in runs]
    assert len(runs) >= 400 // 64 and sum(steps) == 400
    assert min(steps[1:-1]) >= 20 and max(steps) <= 64
    assert all((b - a) % 4 == 1 for (a, _), (b, _) in zip(runs[:-1], runs[1:]))
    plain = [d for _, d in du.runs_of(decode_states(e).cpu().numpy())]
    assert min(plain[1:-1]) < 20


@pytest.mark.gpu
def test_integration_with_the_segmenter_and_stream_order():
    """A small seeded head (H 16) on three recordings of 100-700 samples: the decoded log-probs equal the restatement on the same
    log-probs copied to the CPU; segment_recordings(decode=True, durations=dur) gives the same states; and decoding right behind
    the segmenter call, with no synchronisation in between, gives what the synchronised sequence gives."""
    torch.manual_seed(31)
    head = SegmenterHead(44, 16, 3).eval()
    seg = head.hip()
    sig = synth.pcg_windows(3, 2000, seed=22)
    recs = [torch.from_numpy(sig[i, :n].copy()).cuda() for i, n in enumerate((100, 700, 333))]
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True)
    dur = gaussian_durations([20, 40, 15, 80], [5, 10, 4, 30], 200, min_duration=5)
    feats = tf.ragged(recs)
    logp = seg.ragged(feats)
    torch.cuda.synchronize()
    states = decode_durations(logp, dur)
    torch.cuda.synchronize()
    host = logp.data.cpu().numpy()
    offs = logp.offsets.tolist()
    es = [host[offs[i]:offs[i + 1]] for i in range(3)]
    want, _ = du.decode_list(es, dc.cyclic(), dc.UNIFORM, dur, edge_durations(dur))
    for i in range(3):
        assert np.array_equal(states[i].cpu().numpy(), want[i]), i
        steps = [d for _, d in du.runs_of(want[i])]
        assert min(steps[1:-1], default=5) >= 5 and max(steps) <= 200
    unsynced = decode_durations(seg.ragged(feats), dur)  # enqueued behind the segmenter on the current stream
    assert torch.equal(unsynced.data, states.data)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = decode_durations(seg.ragged(feats), dur)
    side.synchronize()
    assert torch.equal(on_side.data, states.data)
    e2e = segment_recordings(tf, seg, recs, decode=True, durations=dur)
    assert torch.equal(e2e.data, states.data) and e2e.lengths().tolist() == [100, 700, 333]
    A, pi = cyclic_transitions(-0.01, -4.0)
    custom = segment_recordings(tf, seg, recs, decode=(A, pi), durations=dur)
    want, _ = du.decode_list(es, A, pi, dur, edge_durations(dur))
    for i in range(3):
        assert np.array_equal(custom[i].cpu().numpy(), want[i]), i
    assert torch.equal(segment_recordings(tf, seg, recs, decode=True).data, decode_states(logp).data)   # without durations: unchanged
    with pytest.raises(ValueError):
        segment_recordings(tf, seg, recs, durations=dur)


@pytest.mark.gpu
def test_argument_checks(mixed):
    es, dur = mixed[0], mixed[2]
    for bad in (es[6].double(), es[6].half(), es[6].cpu(), es[6][:, :3], es[6].reshape(-1), [es[6]], es[6].cpu().numpy()):
        with pytest.raises(ValueError):
            decode_durations(bad, dur)
    with pytest.raises(ValueError):
        decode_durations(es[6], dur, transitions=dc.cyclic())                             # transitions without initial
    with pytest.raises(ValueError):
        decode_durations(es[6], dur[:3])
    with pytest.raises(ValueError):
        decode_durations(es[6], dur, edge=np.zeros((4, 7), dtype=np.float32))
    with pytest.raises(ValueError):
        decode_durations(es[6], np.zeros((4, 2049), dtype=np.float32))
    dead = dur.copy()
    dead[2, :] = NINF
    with pytest.raises(ValueError):
        decode_durations(es[6], dead)
