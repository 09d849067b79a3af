"""The rolling FSST step (StreamingFSST / hssfsst_stream_step) against answers it did not make itself.

CPU: the three host restatements of the running state (tests/stream_cases.py) agree with each other and with numpy; the gate of
the normalised output holds for a float32 emulation of the kernels' expression; argument errors need no device.

GPU (-m gpu), over the shapes of ``stream_cases.CASES`` -- both step routes, every transform family, chunks of 1 .. 300 columns,
1 .. 300 channels, tapes that wrap at every step:
  * the un-normalised columns against the float64 oracle (the parity gate of tests/parity.py) and against the offline transform;
  * after every step, every channel's running {count, mean, M2} of both blocks against a two-pass float64 reference over everything
    the stream has emitted, and the normalised output of that step -- both halves -- against the float64 z-score;
  * two different chunks through hssfsst_moments_merge, so that the Chan cross term is not zero;
  * a NaN in one channel stays in that channel; the number of tape slots does not change a bit.
With HSS_STREAMING_REPORT=<path> the largest ratio to each gate per case is written there (profiles/streaming_parity.txt).
Nothing here reads /root/reference."""
import ctypes
import os

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import FSST, _lib
from tests import parity
from tests import stream_cases as sc

CASE_IDS = [c["id"] for c in sc.CASES]

# Shapes whose stream is NOT bit-identical to the offline transform's columns (they meet the oracle gate; measured 2.2e-7, 1.1e-9
# and 5.4e-8 of the largest feature).  The MFMA kernels decide some things per GROUP of frames, and a step's groups are not always
# the offline signal's:
#   * canon128, long_chunk: 128-point windows with the canonical band run fsst_canon_kernel, which scales the samples of every
#     64-frame tile by that tile's own energy before the split-f16 fold; a step's tiles start at its own first column.
#   * short_chunk: a 16-frame group of fsst_core128_kernel whose kept band holds only leakage is redone in float64
#     (fsst_mfma128.hpp "Exact groups"; the Hann window's low sidelobes get the quiet stretches of the signal there), and a chunk of
#     13 columns cuts other groups than the offline transform's.  The same case is bit-identical with chunk = 16 or under the
#     Kaiser(0.5) window; with chunk = 29 it is not.
# The generic and any-length kernels and the other MFMA shapes of the table give the same bits (chunks of whole groups, or no
# group on the float64 path).
OFFLINE_NOT_BIT_EQUAL = frozenset({"canon128", "long_chunk", "short_chunk"})


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def _random_chunks(rng, sizes, K, means, sigmas):
    """float32 chunks with unequal chunk means; real and imaginary blocks with different statistics."""
    out = []
    for n, mu in zip(sizes, means):
        re = mu + sigmas[0] * rng.standard_normal((n, K))
        im = -0.6 * mu + 0.3 + sigmas[1] * rng.standard_normal((n, K))
        out.append(np.concatenate([re, im], axis=1).astype(np.float32))
    return out


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("sizes,K,welford", [((3, 17, 1, 40, 9), 7, True), ((300, 1, 129, 48, 1029), 23, False)])
def test_restatements_agree(sizes, K, welford, built_lib):
    """running_reference (two passes), chan_reference (the merge merge_state claims) and welford_reference (hss.moments'
    recurrences through the library's host functions) give the same state after every step -- count exactly, mean to 1e-13, M2 to
    1e-11 relative -- on chunks whose means differ by several sigma (the Chan cross term carries most of M2); the z-score of
    running_reference is numpy's (v - mean) / std(ddof=1)."""
    rng = np.random.default_rng(sum(sizes) + K)
    means = [1.5, 4.0, -2.5, 6.0, 3.0]
    chunks = _random_chunks(rng, sizes, K, means, (0.5, 1.25))
    assert sum(n * K for n in sizes) <= 20000 or not welford
    two = sc.running_reference(chunks)
    others = {"chan": sc.chan_reference(chunks)}
    if welford:
        others["welford"] = sc.welford_reference(chunks)
    for i in range(len(chunks)):
        seen = np.concatenate(chunks[:i + 1], axis=0).astype(np.float64)
        for b, blk in sc.blocks(seen).items():
            want = two[i][b]
            assert want["count"] == blk.size
            assert _rel(want["mean"], blk.mean()) <= 1e-13 and _rel(want["M2"], blk.var() * blk.size) <= 1e-11
            assert _rel(sc.state_std(want["count"], want["M2"]), blk.std(ddof=1)) <= 1e-12
            for name, ref in others.items():
                got = ref[i][b]
                assert got["count"] == want["count"], (name, i, b)
                assert _rel(got["mean"], want["mean"]) <= 1e-13, (name, i, b, got["mean"], want["mean"])
                assert _rel(got["M2"], want["M2"]) <= 1e-11, (name, i, b, got["M2"], want["M2"])
        # the blocks are told apart: their statistics differ by far more than any gate
        assert _rel(two[i]["re"]["mean"], two[i]["im"]["mean"]) > 0.1 and _rel(two[i]["re"]["M2"], two[i]["im"]["M2"]) > 0.1
        cur = sc.blocks(chunks[i].astype(np.float64))
        z = np.concatenate([(cur[b] - sc.blocks(seen)[b].mean()) / sc.blocks(seen)[b].std(ddof=1) for b in sc.BLOCKS], axis=1)
        assert np.abs(two[i]["z"] - z).max() <= 1e-12 * np.abs(z).max()


def test_output_gate_is_sound():
    """The kernels' float32 expression (v - float(mean)) * (1.0f / float(sigma)), emulated in numpy, stays below HALF of
    output_gate (the gate is twice the derived bound) against the float64 z-score, for offsets 0 .. 3000 sigma and scales
    1e-6 .. 1e5."""
    rng = np.random.default_rng(22)
    worst = 0.0
    for scale in (1e-6, 1e-3, 0.37, 1.0, 41.0, 1e5):
        for offset in (0.0, 0.5, 3.0, 30.0, 1000.0, 3000.0):
            v = (scale * (offset + rng.standard_normal(4096))).astype(np.float32)
            v64 = v.astype(np.float64)
            mean, sigma = v64.mean(), v64.std(ddof=1)
            z = (v64 - mean) / sigma
            got = sc.normalize_f32(v, mean, sigma)
            assert got.dtype == np.float32
            derived = 2.0 ** -22 * np.abs(z) + 2.0 ** -24 * abs(mean) / sigma
            err = np.abs(got.astype(np.float64) - z)
            assert (err <= derived * (1 + 1e-6)).all(), (scale, offset, float((err / derived).max()))
            worst = max(worst, float((err / sc.output_gate(z, mean, sigma)).max()))
    print(f"float32 emulation: worst ratio to the output gate {worst:.3f}")
    assert 0.1 < worst < 0.5, worst


def test_offline_column():
    assert [sc.offline_column(t, 512) for t in (0, 255, 256, 639)] == [-255, 0, 1, 384]
    assert [sc.offline_column(t, 100) for t in (0, 49, 50)] == [-49, 0, 1]
    assert [sc.offline_column(t, 33) for t in (0, 16, 17, 99)] == [-16, 0, 1, 83]
    assert [sc.lookahead(n) for n in (512, 256, 128, 100, 64, 33)] == [255, 127, 63, 49, 31, 16]


def test_case_table():
    """The shapes stay small, and the DC cases' offset is what the table says."""
    assert len(set(CASE_IDS)) == len(CASE_IDS) == 13
    for case in sc.CASES:
        assert case["steps"] * case["chunk"] <= 1200, case["id"]
        assert sc.window(case).shape == (case["nwin"],)
    case = sc.CASE_BY_ID["n256"]
    x = sc.signals(case)
    assert x.shape == (3, 7 * 48) and x.dtype == np.float32
    plain = sc.signals(dict(case, dc=False))
    amp = sc.amplitudes(3)
    assert np.allclose(amp, [1e-3, 1.0, 1e3]) and np.allclose((x - plain).mean(axis=1), 0.25 * amp, rtol=1e-3)


def test_stream_argument_errors(built_lib):
    """A null plan is refused before a device is looked at."""
    buf = np.zeros(64, dtype=np.float64)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert built_lib.hssfsst_stream_step(None, p, 200, 127, p, 16, 0, 1, 16, p, p, None, None) == _lib.E_INVAL
    assert built_lib.hssfsst_moments_merge(None, p, 1, 1, p, None) == _lib.E_INVAL
    assert built_lib.hssfsst_normalize_running(None, p, 1, 1, p, None) == _lib.E_INVAL


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
_UNNORM = {}          # case id -> (the un-normalised outputs of every step as numpy (channels, chunk, 2K), last_kernel(), latency_samples)
_REPORT = {}          # case id -> dict of figures


def _stream(case, normalize, slots=None):
    from heart_sounds_segmentation_amd.streaming import StreamingFSST
    return StreamingFSST(case["channels"], case["fs"], sc.window(case), truncate_freq=case["band"], chunk=case["chunk"],
                         normalize=normalize, slots=case["slots"] if slots is None else slots)


def _chunk(x, case, i):
    return np.ascontiguousarray(x[:, i * case["chunk"]:(i + 1) * case["chunk"]])


def _unnormalized(case):
    """The case's un-normalised stream, run once per session."""
    if case["id"] not in _UNNORM:
        x = sc.signals(case)
        st = _stream(case, normalize=False)
        outs = [st.step(torch.from_numpy(_chunk(x, case, i)).cuda()).cpu().numpy() for i in range(case["steps"])]
        _UNNORM[case["id"]] = (outs, st.last_kernel(), st.latency_samples)
    return _UNNORM[case["id"]]


def _assert_route(case, kernel):
    """One launch per step reads fsst_core128_kernel<..., stream...>; the three-launch route names the plain transform kernel."""
    if case["route"] == "stream":
        assert "fsst_core128_kernel" in kernel and "stream" in kernel, (case["id"], kernel)
    else:
        assert "stream" not in kernel, (case["id"], kernel)
        if case["id"] in ("over_tiny", "nine_groups"):                  # the MFMA family, declined by the one-launch kernel
            assert "fsst_core128_kernel" in kernel, (case["id"], kernel)


def _write_report():
    path = os.environ.get("HSS_STREAMING_REPORT")
    if not path:
        return
    with open(path, "w") as fh:
        fh.write("Streaming FSST against float64 references (tests/test_streaming.py): per case the kernel of the last step and the\n"
                 "largest error as a fraction of its gate (state: count equal, mean 1e-12 max(|mean|, rms), M2 1e-10 M2; output:\n"
                 "stream_cases.output_gate; oracle: max error / max|ref| of the un-normalised columns, gate 1e-4).\n\n")
        for cid in CASE_IDS:
            r = _REPORT.get(cid)
            if not r:
                continue
            fh.write(f"{cid:14s} K {r.get('K', '-'):>3}  mean {r.get('mean', float('nan')):.1e}  M2 {r.get('M2', float('nan')):.1e}  "
                     f"output {r.get('output', float('nan')):.3f}  oracle rel {r.get('oracle_rel', float('nan')):.2e}  "
                     f"offline {r.get('offline', '-'):>15}  mean^2/var {r.get('m2v', float('nan')):.1e}  {r.get('kernel', '-')}\n")


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_unnormalized_stream_matches_oracle_and_offline(cid, oracle_mod, built_lib):
    """The concatenated un-normalised steps are the offline transform's columns shifted by nwin - 1 - nwin // 2 (the odd window
    decides between that and nwin // 2 - 1): within the parity gate of the float64 oracle on at most three channels -- the columns
    whose frames lie in the signal against the oracle of the signal, the columns of the first steps against the oracle of the
    signal behind nwin - 1 - nwin // 2 zeros -- and, on every channel, bit for bit the offline transform of the signal and of the
    signal behind those zeros, except on the shapes of OFFLINE_NOT_BIT_EQUAL (the canonical-band kernel of 128-point windows)."""
    case = sc.CASE_BY_ID[cid]
    x, w, nwin, fs, band = sc.signals(case), sc.window(case), case["nwin"], case["fs"], case["band"]
    outs, kernel, latency = _unnormalized(case)
    stream = np.concatenate(outs, axis=1)
    T, L = case["steps"] * case["chunk"], sc.lookahead(nwin)
    klo, K = oracle_mod.band(nwin, fs, *band)
    assert stream.shape == (case["channels"], T, 2 * K) and stream.dtype == np.float32
    if cid == "odd_k":
        assert K % 2 == 1, K
    _assert_route(case, kernel)

    def features(sig):
        s, f, t, hd = oracle_mod.fsst(sig, fs, w, return_halfdist=True)
        return np.concatenate([s[klo:klo + K].real.T, s[klo:klo + K].imag.T], axis=1).astype(np.float32), hd

    cols = np.arange(L, T)                                              # stream columns whose frames hold no zero history
    oc = sc.offline_column(cols, nwin)
    rel = 0.0
    for c in sc.oracle_channels(case["channels"]):
        if cols.size:
            ref, hd = features(x[c])
            assert oc[0] == 0 and oc[-1] == T - 1 - L
            rel = max(rel, parity.check(stream[c, cols], ref[oc], hd[oc], 0, what=f"{cid} ch{c}")["rel"])
        # every column, the first steps' included: the signal behind L zeros, whose column t is stream column t
        ref, hd = features(np.concatenate([np.zeros(L, dtype=np.float32), x[c]]))
        rel = max(rel, parity.check(stream[c], ref[:T], hd[:T], 0, what=f"{cid} ch{c} with its zero history")["rel"])
    # the offline transform of the signal (its columns 0 .. T - 1 - L), and of the signal behind L zeros (every stream column)
    tf = FSST(fs, w, truncate_freq=band, stack=True)
    off = tf.unnormalized(torch.from_numpy(x).cuda()).cpu().numpy()
    xz = np.concatenate([np.zeros((case["channels"], L), dtype=np.float32), x], axis=1)
    offz = tf.unnormalized(torch.from_numpy(xz).cuda()).cpu().numpy()[:, :T]
    equal = bool(np.array_equal(stream[:, L:], off[:, :max(T - L, 0)])) and bool(np.array_equal(stream, offz))
    diff = float(np.abs(stream - offz).max() / np.abs(offz).max())
    if T > L:
        diff = max(diff, float(np.abs(stream[:, L:] - off[:, :T - L]).max() / np.abs(off).max()))
    print(f"{cid}: {kernel}; oracle rel {rel:.2e}; offline columns {'equal' if equal else f'differ by {diff:.2e} of max'}; latency {latency}")
    _REPORT.setdefault(cid, {}).update(K=K, oracle_rel=rel, kernel=kernel, offline="bit-identical" if equal else f"differs {diff:.1e}")
    _write_report()
    assert latency == L, (latency, L)
    if cid not in OFFLINE_NOT_BIT_EQUAL:
        assert equal, f"{cid}: stream and offline columns differ by {diff:.3e} of the largest feature"


@pytest.mark.gpu
def test_latency_samples(built_lib):
    """The look-ahead the oracle confirmed on the odd window (test_unnormalized_stream_matches_oracle_and_offline[odd33])."""
    from heart_sounds_segmentation_amd.streaming import StreamingFSST
    for nwin, want in ((512, 255), (100, 49), (33, 16)):
        st = StreamingFSST(1, 1000, np.hanning(nwin), truncate_freq=(25, 200), chunk=16, normalize=False, slots=1)
        assert st.latency_samples == want == sc.lookahead(nwin)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_running_state_and_normalized_output(cid, built_lib):
    """After EVERY step, for EVERY channel and BOTH blocks: the device's {count, mean, M2} against running_reference of the
    un-normalised twin's outputs so far (count equal, |d mean| <= 1e-12 max(|mean|, rms), |d M2| <= 1e-10 M2), and the step's
    normalised output against the float64 z-score at stream_cases.output_gate; step, step_unfused and step_host stay bit-identical
    in output and state."""
    case = sc.CASE_BY_ID[cid]
    x = sc.signals(case)
    outs, _, _ = _unnormalized(case)
    C, steps = case["channels"], case["steps"]
    refs = [sc.running_reference([o[c] for o in outs]) for c in range(C)]
    # the DC cases (and every other one) stay where merge_state's M2_b = q - s mean_b loses nothing that matters
    m2v = max(r[i][b]["mean"] ** 2 / (r[i][b]["M2"] / (r[i][b]["count"] - 1)) for r in refs for i in range(steps) for b in sc.BLOCKS
              if r[i][b]["count"] > 1 and r[i][b]["M2"] > 0)
    assert m2v <= sc.MAX_MEAN2_OVER_VAR, m2v
    a, b, h = _stream(case, True), _stream(case, True), _stream(case, True)
    worst = {"count": 0.0, "mean": 0.0, "M2": 0.0, "output": 0.0}
    for i in range(steps):
        xi = _chunk(x, case, i)
        xd = torch.from_numpy(xi).cuda()
        ya = a.step(xd).cpu().numpy()
        yb = b.step_unfused(xd).cpu().numpy()
        yh = h.step_host(xi)
        assert np.array_equal(ya, yb, equal_nan=True) and np.array_equal(ya, yh, equal_nan=True), (cid, i)
        assert torch.equal(a.state, b.state) and torch.equal(a.state, h.state), (cid, i)
        state = a.state.cpu().numpy()
        for c in range(C):
            for k, blk in enumerate(sc.BLOCKS):
                rc, rm, r2 = sc.state_ratios(state[c, 3 * k:3 * k + 3], refs[c][i][blk])
                worst["count"] = max(worst["count"], rc); worst["mean"] = max(worst["mean"], rm); worst["M2"] = max(worst["M2"], r2)
            worst["output"] = max(worst["output"], sc.output_ratio(ya[c], refs[c][i]))
    kernel = a.last_kernel()
    print(f"{cid}: {kernel}; fractions of the gates: mean {worst['mean']:.1e}, M2 {worst['M2']:.1e}, output {worst['output']:.3f}; "
          f"largest mean^2/var {m2v:.2e}")
    _REPORT.setdefault(cid, {}).update(kernel=kernel, m2v=m2v, K=outs[0].shape[2] // 2, **{k: worst[k] for k in ("mean", "M2", "output")})
    _write_report()
    _assert_route(case, kernel)
    assert worst["count"] == 0.0, f"{cid}: a count differs"
    assert worst["mean"] <= 1.0, f"{cid}: mean off by {worst['mean']:.3g} x its gate"
    assert worst["M2"] <= 1.0, f"{cid}: M2 off by {worst['M2']:.3g} x its gate"
    assert worst["output"] <= 1.0, f"{cid}: normalised output off by {worst['output']:.3g} x its gate"


@pytest.mark.gpu
@pytest.mark.parametrize("band,n_a,n_b", [((25, 200), 17, 100), ((25, 210), 17, 33), ((25, 210), 1, 1), ((25, 200), 300, 1029)])
def test_moments_merge_two_different_chunks(band, n_a, n_b, built_lib):
    """hssfsst_moments_merge of chunk A and then of chunk B, whose means lie about 10 sigma apart (the Chan cross term is most of
    M2), against numpy float64 over A || B at the gates of the running state; then hssfsst_normalize_running on B with that state at
    the output gate.  Even and odd K, more than 16 and more than 64 pieces, batch entries that do not start on 16 bytes."""
    tf = FSST(1000, np.kaiser(128, 0.5), truncate_freq=band, stack=True)
    plan = tf._plan(0, _lib.MODE_STACK_UNNORM)
    K, batch = plan.K, 3
    assert K % 2 == (1 if band[1] == 210 else 0)
    if K % 2:
        assert (n_b * 2 * K * 4) % 16 != 0
    rng = np.random.default_rng(n_a + 7 * n_b + K)

    def chunk(n, shift):
        re = 1.5 + shift * 3.0 + 3.0 * rng.standard_normal((batch, n, K))
        im = -0.7 - shift * 0.5 + 0.5 * rng.standard_normal((batch, n, K))
        return np.concatenate([re, im], axis=2).astype(np.float32)

    A, B = chunk(n_a, 0.0), chunk(n_b, 10.0)
    Ad, Bd = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    state = torch.zeros(batch, 6, dtype=torch.float64, device="cuda")
    for Fd, n in ((Ad, n_a), (Bd, n_b)):
        assert built_lib.hssfsst_moments_merge(plan.handle, ctypes.c_void_p(Fd.data_ptr()), batch, n, ctypes.c_void_p(state.data_ptr()), None) == 0
    assert built_lib.hssfsst_normalize_running(plan.handle, ctypes.c_void_p(Bd.data_ptr()), batch, n_b, ctypes.c_void_p(state.data_ptr()), None) == 0
    st, got = state.cpu().numpy(), Bd.cpu().numpy()
    worst = {"mean": 0.0, "M2": 0.0, "output": 0.0}
    for e in range(batch):
        ref = sc.running_reference([A[e], B[e]])[1]
        for k, blk in enumerate(sc.BLOCKS):
            assert ref[blk]["mean"] ** 2 / (ref[blk]["M2"] / (ref[blk]["count"] - 1)) <= sc.MAX_MEAN2_OVER_VAR
            rc, rm, r2 = sc.state_ratios(st[e, 3 * k:3 * k + 3], ref[blk])
            assert rc == 0.0, (e, blk, st[e], ref[blk])
            worst["mean"] = max(worst["mean"], rm); worst["M2"] = max(worst["M2"], r2)
        worst["output"] = max(worst["output"], sc.output_ratio(got[e], ref))
    print(f"K {K}, {n_a} + {n_b} frames: fractions of the gates: mean {worst['mean']:.1e}, M2 {worst['M2']:.1e}, output {worst['output']:.3f}")
    assert worst["mean"] <= 1.0 and worst["M2"] <= 1.0 and worst["output"] <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["canon128", "c5"])
def test_channels_do_not_leak(cid, built_lib):
    """One NaN sample in one channel at the second step: every other channel's outputs and running state are bit-identical to the
    run without it, at every step."""
    case = sc.CASE_BY_ID[cid]
    x = sc.signals(case)
    bad, pos = case["channels"] // 2, case["chunk"] + case["chunk"] // 2
    xn = x.copy()
    xn[bad, pos] = np.nan
    others = [c for c in range(case["channels"]) if c != bad]
    clean, dirty = _stream(case, True), _stream(case, True)
    hit = False
    for i in range(case["steps"]):
        y0 = clean.step(torch.from_numpy(_chunk(x, case, i)).cuda()).cpu().numpy()
        y1 = dirty.step(torch.from_numpy(_chunk(xn, case, i)).cuda()).cpu().numpy()
        assert np.array_equal(y0[others], y1[others]), (cid, i)
        assert np.array_equal(clean.state.cpu().numpy()[others], dirty.state.cpu().numpy()[others]), (cid, i)
        assert np.isfinite(y0).all()
        hit = hit or bool(np.isnan(y1[bad]).any())
        assert i != 1 or hit
    assert hit and not np.isfinite(dirty.state.cpu().numpy()[bad]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["one_channel", "short_chunk"])
def test_tape_wrap(cid, built_lib):
    """slots = 1 (the tape wraps at every step; for chunk < nwin - 1 the history moves onto itself), 2 and 7: un-normalised outputs,
    normalised outputs and the final state are the same bits."""
    case = sc.CASE_BY_ID[cid]
    x = sc.signals(case)
    res = []
    for slots in (1, 2, 7):
        un, no = _stream(case, False, slots), _stream(case, True, slots)
        assert un.tape_len == case["nwin"] - 1 + slots * case["chunk"]
        outs = []
        for i in range(case["steps"]):
            xd = torch.from_numpy(_chunk(x, case, i)).cuda()
            outs.append(un.step(xd).cpu().numpy())
            outs.append(no.step(xd).cpu().numpy())
        res.append((outs, no.state.cpu().numpy()))
    assert all(np.isfinite(o).all() for o in res[0][0])
    for outs, state in res[1:]:
        assert all(np.array_equal(p, q) for p, q in zip(outs, res[0][0]))
        assert np.array_equal(state, res[0][1])
