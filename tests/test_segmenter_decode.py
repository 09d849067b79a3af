"""Log-probs -> state sequences on the device: hssfsst_decode_states (C ABI), consumer.decode_states and its helpers.

The contract is exact: int64 fixed point (2^-20), ties to the smaller state -- include/hssfsst.h -- restated in numpy in
tests/decode_cases.py.  The GPU tests ask for equality with that restatement in every state and every int64 score.  CPU tests
check the ABI, the argument errors (all raised before any device work), the host helpers, the kernel's arithmetic and geometry
under sanitizers (tests/native/decode_check.cpp), the shipped kernel's scratch size, and the restatement itself against float64."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, consumer, synth
from heart_sounds_segmentation_amd.consumer import (HipSegmenter, SegmenterHead, cyclic_transitions, decode_states, segment_recordings,
                                                    state_runs, transitions_from_labels)
from heart_sounds_segmentation_amd.transforms import FSST, RaggedFeatures
from tests import decode_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hssfsst.h")
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")
NINF = float("-inf")


def i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def f32(values):
    return (ctypes.c_float * len(values))(*values)


def geometry(lib):
    seg, mx = ctypes.c_int(0), ctypes.c_int64(0)
    assert lib.hssfsst_decode_info(ctypes.byref(seg), ctypes.byref(mx)) == 0
    return seg.value, mx.value


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_library_and_info(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    assert "int hssfsst_decode_states(" in text and "int hssfsst_decode_info(" in text
    fn = built_lib.hssfsst_decode_states
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    S, mx = geometry(built_lib)
    assert S >= 64 and mx == 2 ** 26
    assert built_lib.hssfsst_decode_info(None, None) == 0
    assert consumer.decode_info() == (S, mx)


def test_argument_errors_need_no_device(built_lib):
    D = built_lib.hssfsst_decode_states
    err = built_lib.hssfsst_last_error
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below ends before any device work
    A, pi = (np.ascontiguousarray(v) for v in cyclic_transitions())
    cA, cpi = f32(A.ravel().tolist()), f32(pi.tolist())
    ok = i64([0, 5])
    assert D(fake, i64([0]), 0, cA, cpi, fake, None, 0, None) == 0                        # count == 0: nothing to do
    for args, word in (((None, ok, 1, cA, cpi, fake, None, 0, None), b"logp"),
                       ((fake, None, 1, cA, cpi, fake, None, 0, None), b"offsets"),
                       ((fake, ok, 1, None, cpi, fake, None, 0, None), b"transitions"),
                       ((fake, ok, 1, cA, None, fake, None, 0, None), b"initial"),
                       ((fake, ok, 1, cA, cpi, None, None, 0, None), b"states")):
        assert D(*args) == _lib.E_INVAL and word in err() and b"NULL" in err(), word
    assert D(fake, ok, -1, cA, cpi, fake, None, 0, None) == _lib.E_INVAL and b"negative" in err()
    assert D(fake, ok, 1, cA, cpi, fake, None, -1, None) == _lib.E_INVAL and b"device" in err()
    assert D(fake, i64([2, 4]), 1, cA, cpi, fake, None, 0, None) == _lib.E_INVAL and b"offsets[0]" in err()
    for bad in ([0, 5, 5], [0, 7, 3], [0, 4, 4, 9]):
        assert D(fake, i64(bad), len(bad) - 1, cA, cpi, fake, None, 0, None) == _lib.E_INVAL and b"index 2" in err(), bad
    nanA = A.copy()
    nanA[2, 3] = np.nan
    assert D(fake, ok, 1, f32(nanA.ravel().tolist()), cpi, fake, None, 0, None) == _lib.E_INVAL and b"transitions[2][3] is NaN" in err()
    assert D(fake, ok, 1, cA, f32([0, np.nan, 0, 0]), fake, None, 0, None) == _lib.E_INVAL and b"initial[1] is NaN" in err()
    deadA = A.copy()
    deadA[1, :] = -np.inf
    assert D(fake, ok, 1, f32(deadA.ravel().tolist()), cpi, fake, None, 0, None) == _lib.E_INVAL and b"row 1" in err()
    assert D(fake, ok, 1, cA, f32([NINF] * 4), fake, None, 0, None) == _lib.E_INVAL and b"initial is all -inf" in err()
    assert D(ctypes.c_void_p(4100), ok, 1, cA, cpi, fake, None, 0, None) == _lib.E_INVAL and b"aligned" in err()
    assert D(fake, i64([0, 3, 3 + 2 ** 26 + 1]), 2, cA, cpi, fake, None, 0, None) == _lib.E_UNSUPPORTED and b"recording 1" in err()
    many = [i * 2 ** 26 for i in range(33)]                                               # 2^31 steps in all
    assert D(fake, i64(many), 32, cA, cpi, fake, None, 0, None) == _lib.E_UNSUPPORTED and b"in all" in err()


def test_host_helpers_against_hand_written_answers():
    A, pi = cyclic_transitions()
    assert A.dtype == np.float32 and pi.dtype == np.float32
    want = [[0, 0, NINF, NINF], [NINF, 0, 0, NINF], [NINF, NINF, 0, 0], [0, NINF, NINF, 0]]
    assert np.array_equal(A, np.array(want, dtype=np.float32)) and np.array_equal(pi, np.zeros(4, dtype=np.float32))
    A, _ = cyclic_transitions(-0.25, -3.0)
    assert A[3, 3] == -0.25 and A[3, 0] == -3.0 and A[0, 1] == -3.0 and np.isneginf(A[0, 2]) and np.isneginf(A[1, 0])
    # 0 -> 0 once, 0 -> 1 twice, 1 -> 1 once, 1 -> 2 twice, 2 -> 3 once, 3 -> 0 once; starts: 0, 1, 0
    A, pi = transitions_from_labels([torch.tensor([0, 0, 1, 1, 2, 3, 0]), np.array([1, 2]), torch.tensor([0, 1], dtype=torch.uint8)])
    third = np.float32(np.log(1 / 3))
    want = np.full((4, 4), NINF, dtype=np.float32)
    want[0, 0], want[0, 1], want[1, 1], want[1, 2], want[2, 3], want[3, 0] = third, np.float32(np.log(2 / 3)), third, np.float32(np.log(2 / 3)), 0, 0
    assert np.allclose(A, want, rtol=1e-6, atol=0) and np.array_equal(np.isneginf(A), np.isneginf(want))
    assert np.allclose(pi[:2], np.log([2 / 3, 1 / 3]), rtol=1e-6) and np.isneginf(pi[2:]).all()
    with pytest.raises(ValueError):
        transitions_from_labels([torch.tensor([0, 4])])
    starts, vals = state_runs(torch.tensor([0, 0, 1, 1, 1, 2, 3, 3, 0], dtype=torch.uint8))
    assert starts.dtype == torch.int64 and vals.dtype == torch.uint8
    assert starts.tolist() == [0, 2, 5, 6, 8] and vals.tolist() == [0, 1, 2, 3, 0]
    starts, vals = state_runs(torch.tensor([2], dtype=torch.uint8))
    assert starts.tolist() == [0] and vals.tolist() == [2]


def test_decode_arithmetic_under_sanitizers(tmp_path):
    """csrc/decode_layout.hpp in a program of its own (tests/native/decode_check.cpp) built with -fsanitize=address,undefined:
    the kernel's chunked algorithm with its lanes simulated equals the sequential loop, and no int64 sum overflows."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "decode_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "decode_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "decode check ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_shipped_kernel_uses_no_scratch(built_lib):
    res = _lib.kernel_resources("seg_decode_kernel")
    assert len(res) == 1, res
    (facts,) = res.values()
    assert facts["private_segment_fixed_size"] == 0 and facts["agpr_count"] == 0, facts
    assert 0 < facts["group_segment_fixed_size"] <= 80 * 1024, facts                     # two workgroups per CU


@pytest.mark.parametrize("kind", ("dirichlet1", "dirichlet0.2", "integers"))
def test_restatement_is_within_the_quantisation_bound_of_float64(kind):
    """The path of the quantised loop, scored in float64 on the unquantised inputs, is within T x 2^-19 of the float64 optimum:
    two terms per step, each moved by at most 2^-21 by the quantiser, on each of the two paths compared.  Derived, not measured."""
    rng = np.random.default_rng(5)
    lens = (1, 2, 50, 777, 3000)
    A, pi = dc.dense_transitions(3), dc.UNIFORM
    es = [dc.emissions(kind, T, rng) for T in lens]
    es = [np.maximum(e, np.float32(-100.0)) for e in es]                                  # (a Dirichlet(0.2) draw may be exactly 0)
    paths, _ = dc.viterbi(es, [A] * len(es), [pi] * len(es), exact=True)
    fpaths, fscores = dc.viterbi(es, [A] * len(es), [pi] * len(es), exact=False)
    for e, p, fp, fs, T in zip(es, paths, fpaths, fscores, lens):
        assert abs(dc.path_score_f64(e, A, pi, fp) - fs) <= 1e-9 * max(1.0, abs(fs))      # the float64 loop scores its own path
        assert dc.path_score_f64(e, A, pi, p) >= fs - T * 2.0 ** -19, (kind, T)


# ---------------------------------------------------------------------------------------------------- GPU
def gpu_decode(es, A, pi):
    """One ragged call on the list of (T, 4) numpy emissions -> (list of numpy paths, int64 scores)."""
    offs = np.concatenate([[0], np.cumsum([e.shape[0] for e in es])]).astype(np.int64)
    arena = torch.from_numpy(np.concatenate(es)).cuda()
    states = torch.full((int(offs[-1]),), 255, dtype=torch.uint8, device="cuda")
    scores = torch.zeros(len(es), dtype=torch.int64, device="cuda")
    A, pi = np.ascontiguousarray(A, dtype=np.float32), np.ascontiguousarray(pi, dtype=np.float32)
    rc = _lib.lib().hssfsst_decode_states(arena.data_ptr(), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(es),
                                          A.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), pi.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                          states.data_ptr(), scores.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "hssfsst_decode_states")
    st = states.cpu().numpy()
    return [st[offs[i]:offs[i + 1]] for i in range(len(es))], scores.cpu().numpy()


def matrix_lengths(S):
    return (1, 2, 3, 63, 64, 65, S - 1, S, S + 1, S + 2, 2 * S + 1, 3 * S + 17)          # (S + 2: the first step of a second segment)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", dc.KINDS)
def test_equals_the_restatement_exactly(built_lib, kind):
    """Lengths x {cyclic A, dense A} x {uniform pi, state 0 only}, one ragged call per (A, pi): every state and every int64 score
    equals the numpy restatement; under the cyclic A every step stays or advances."""
    S, _ = geometry(built_lib)
    rng = np.random.default_rng(11)
    es = [dc.emissions(kind, T, rng) for T in matrix_lengths(S)]
    for A, cyc in ((dc.cyclic(), True), (dc.dense_transitions(7), False)):
        for pi in (dc.UNIFORM, dc.STATE0):
            want, wscore = dc.viterbi(es, [A] * len(es), [pi] * len(es))
            got, gscore = gpu_decode(es, A, pi)
            for e, w, g in zip(es, want, got):
                bad = np.flatnonzero(w != g)
                assert bad.size == 0, (kind, cyc, pi.tolist(), e.shape[0], int(bad[0]), int(w[bad[0]]), int(g[bad[0]]))
            assert np.array_equal(wscore, gscore), (kind, cyc, pi.tolist(), wscore.tolist(), gscore.tolist())
            if cyc and kind != "dirichlet0.2":                                            # (a draw of exactly 0 forbids a state)
                for g in got:
                    assert np.isin(np.diff(g.astype(np.int64)) % 4, (0, 1)).all()
                    assert pi is dc.UNIFORM or g[0] == 0


@pytest.mark.gpu
def test_special_values(built_lib):
    S, _ = geometry(built_lib)
    rng = np.random.default_rng(12)
    es = [dc.emissions("dirichlet1", T, rng) for T in (40, S + 30, 2 * S + 5, 9)]
    es[0][10, :] = np.nan
    es[1][S, 1] = NINF
    es[1][7, 2] = np.inf
    es[2][S + 3, 0] = 1e6
    es[2][2 * S + 2, 3] = -1e6
    es[2][5, 1] = 40000.0
    es[3][4, :] = NINF                                   # an all -inf step: score NEG, the tie rule's path
    for A, pi in ((dc.cyclic(), dc.UNIFORM), (dc.dense_transitions(8), dc.STATE0)):
        want, wscore = dc.viterbi(es, [A] * len(es), [pi] * len(es))
        got, gscore = gpu_decode(es, A, pi)
        for w, g in zip(want, got):
            assert np.array_equal(w, g)
        assert np.array_equal(wscore, gscore) and wscore[3] == dc.NEG


@pytest.mark.gpu
def test_more_recordings_than_one_launch_takes(built_lib):
    """The offsets travel as kernel arguments, 256 recordings per launch: 256, 257 and 600 short recordings, scores included."""
    rng = np.random.default_rng(15)
    es = [dc.emissions("dirichlet1", int(T), rng) for T in rng.integers(1, 12, size=600)]
    A, pi = dc.dense_transitions(10), dc.UNIFORM
    want, wscore = dc.viterbi(es, [A] * len(es), [pi] * len(es))
    for count in (256, 257, 600):
        got, gscore = gpu_decode(es[:count], A, pi)
        assert all(np.array_equal(w, g) for w, g in zip(want, got)) and np.array_equal(wscore[:count], gscore), count


@pytest.fixture(scope="module")
def mixed(built_lib):
    """19 recordings of mixed lengths as one arena on the GPU, and their decoding as one list (computed once, never changed)."""
    S, _ = geometry(built_lib)
    lens = [1, 2, 15, 64, 65, 40, 333, 2 * S + 5, 5, 16, S, 64, 7, 7, S + 1, 3, 1, 90, 600]
    rng = np.random.default_rng(13)
    es = [torch.from_numpy(dc.emissions("dirichlet1", T, rng)).cuda() for T in lens]
    offs = np.concatenate([[0], np.cumsum(lens)])
    rag = RaggedFeatures(torch.cat(es), torch.tensor(offs, dtype=torch.int64), 4, False)
    out = decode_states(rag, return_scores=True)
    return es, rag, out[0], out[1]


@pytest.mark.gpu
def test_a_recording_does_not_depend_on_its_neighbours(mixed):
    es, rag, states, scores = mixed
    assert isinstance(states, RaggedFeatures) and states.data.dtype == torch.uint8 and states.data.shape == (rag.data.shape[0],)
    assert states.lengths().tolist() == rag.lengths().tolist() and scores.dtype == torch.float64 and scores.shape == (len(es),)
    rev = RaggedFeatures(torch.cat(es[::-1]), torch.tensor(np.concatenate([[0], np.cumsum([e.shape[0] for e in es[::-1]])])), 4, False)
    back, back_scores = decode_states(rev, return_scores=True)
    for i, e in enumerate(es):
        alone, sc = decode_states(e, return_scores=True)
        assert alone.shape == (e.shape[0],) and torch.equal(alone, states[i]), i
        assert sc == scores[i] and back_scores[len(es) - 1 - i] == scores[i]
        assert torch.equal(back[len(es) - 1 - i], states[i]), i


@pytest.mark.gpu
def test_dense_forms_equal_the_ragged_call(mixed, built_lib):
    S, _ = geometry(built_lib)
    rng = np.random.default_rng(14)
    B, T = 5, S + 9
    x = torch.from_numpy(np.stack([dc.emissions("dirichlet1", T, rng) for _ in range(B)])).cuda()
    A, pi = dc.dense_transitions(9), dc.UNIFORM
    rag = decode_states(RaggedFeatures(x.reshape(B * T, 4), torch.arange(B + 1) * T, 4, False), A, pi)
    got = decode_states(x, A, pi)
    assert got.shape == (B, T) and got.dtype == torch.uint8 and torch.equal(got.reshape(-1), rag.data)
    for b in range(B):
        assert torch.equal(decode_states(x[b], torch.from_numpy(A), torch.from_numpy(pi)), rag[b])
    assert rag.padded().shape == (B, T) and torch.equal(rag.padded(), got)


@pytest.mark.gpu
def test_integration_with_the_segmenter_and_stream_order():
    """A small seeded head (H 16) on three recordings of 100-700 samples: the decoded log-probs equal the restatement on the same
    log-probs copied to the CPU; segment_recordings(decode=True) gives the same states; and decoding right behind the segmenter
    call, with no synchronisation in between, gives what the synchronised sequence gives."""
    torch.manual_seed(31)
    head = SegmenterHead(44, 16, 3).eval()
    seg = head.hip()
    sig = synth.pcg_windows(3, 2000, seed=22)
    recs = [torch.from_numpy(sig[i, :n].copy()).cuda() for i, n in enumerate((100, 700, 333))]
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True)
    feats = tf.ragged(recs)
    logp = seg.ragged(feats)
    torch.cuda.synchronize()
    states = decode_states(logp)
    torch.cuda.synchronize()
    host = logp.data.cpu().numpy()
    offs = logp.offsets.tolist()
    es = [host[offs[i]:offs[i + 1]] for i in range(3)]
    want, _ = dc.viterbi(es, [dc.cyclic()] * 3, [dc.UNIFORM] * 3)
    for i in range(3):
        assert np.array_equal(states[i].cpu().numpy(), want[i]), i
        assert np.isin(np.diff(want[i].astype(np.int64)) % 4, (0, 1)).all()
    unsynced = decode_states(seg.ragged(feats))          # enqueued behind the segmenter on the current stream
    assert torch.equal(unsynced.data, states.data)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = decode_states(seg.ragged(feats))
    side.synchronize()
    assert torch.equal(on_side.data, states.data)
    e2e = segment_recordings(tf, seg, recs, decode=True)
    assert torch.equal(e2e.data, states.data) and e2e.lengths().tolist() == [100, 700, 333]
    A, pi = cyclic_transitions(-0.01, -4.0)
    custom = segment_recordings(tf, seg, recs, decode=(A, pi))
    want, _ = dc.viterbi(es, [A] * 3, [pi] * 3)
    for i in range(3):
        assert np.array_equal(custom[i].cpu().numpy(), want[i]), i
    assert torch.equal(segment_recordings(tf, seg, recs).data, logp.data)               # the default is unchanged
    starts, vals = state_runs(states[1])
    assert starts[0] == 0 and (vals[1:] != vals[:-1]).all() and starts.is_cuda


@pytest.mark.gpu
def test_argument_checks(mixed):
    es = mixed[0]
    for bad in (es[6].double(), es[6].half(), es[6].cpu(), es[6][:, :3], es[6].reshape(-1), [es[6]], es[6].cpu().numpy()):
        with pytest.raises(ValueError):
            decode_states(bad)
    with pytest.raises(ValueError):
        decode_states(es[6], transitions=dc.cyclic())                                     # transitions without initial
    dead = dc.cyclic()
    dead[2, :] = NINF
    with pytest.raises(ValueError):
        decode_states(es[6], dead, dc.UNIFORM)
    with pytest.raises(ValueError):
        decode_states(es[6], dc.cyclic(), np.full(4, NINF, dtype=np.float32))
