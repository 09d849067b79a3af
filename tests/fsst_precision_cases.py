"""What float32 itself does on an FSST, per 64-column block: the restatements, the emulation of the canonical fold's arithmetic
class with its defects, the metric and the case table that tests/test_fsst_precision.py holds the kernels to.  CPU only (numpy,
scipy, torch on the host); the reference is the float64 oracle under oracle/, as everywhere else in the suite.

The gate of tests/parity.py (1e-4 of a signal's largest feature: the contract) has about 300 x of slack over what the kernels do,
and is relative to the signal's maximum, so it cannot see an error that is large only where the signal is quiet.  Here an error is
measured against u_j = 2^-24 ||span_j||_2 max|w| of the aligned block of 64 columns it lies in (``block_ratios``), and the bound is
a multiple of what two float32 restatements with float64 rounding decisions reach on the same case (R32): computed at test
time from the reference side only.

Restatements (values only; the synchrosqueezing rows come from ``rows``, float64, restated from oracle/fsst_numpy.py):
  * ``float32_direct``  frames times a float32 window-twiddle table, one float32 matrix product;
  * ``float32_fft``     scipy.fft.fft of the float32 windowed frames (complex64);
  * ``float32_zscore``  the reference's epilogue in float32 torch ops on such values;
  * ``split_f16``       the canonical fold's arithmetic CLASS (per-tile power-of-two scale, x = x1 + x2 and c = c1 + c2 in float16,
                        four products accumulated in float32), with the defects D1 .. D4 as switches;
  * D5 is a switch of ``float32_direct`` (twiddles from the unreduced float32 angle), D6 one of the rows (``rows_d6``).
"""
import numpy as np

from heart_sounds_segmentation_amd import synth
from tests import parity

BLOCK = 64                    # columns per block: the canonical kernels' aligned tile (fsst_canon128.hpp)
MARGIN = 8.0                  # kernel <= MARGIN x float32 (tests/test_segmenter_conditioned.py K_FWD, README "bound 8 x")
BAND = (25, 200)
SMALL_CELL = 1e-4             # D6: cells below this fraction of the signal's largest feature take float32 decisions


# ---- the transform, restated ---------------------------------------------------------------------------------------------------
def frames(x, N):
    """(n, N) frames of the zero-padded signal, hop 1, in x's own type: frame t covers samples t - N // 2 .. t - N // 2 + N - 1."""
    x = np.asarray(x).ravel()
    m = N // 2
    xp = np.concatenate([np.zeros(m, x.dtype), x, np.zeros(N - 1 - m, x.dtype)])
    return np.lib.stride_tricks.sliding_window_view(xp, N)


def dtwin(window, fs):
    """The derivative window: not-a-knot cubic spline through the window at knots 1 .. N, its slope times fs / 2 pi."""
    from scipy.interpolate import CubicSpline
    w = np.asarray(window, dtype=np.float64).ravel()
    knots = np.arange(1, w.size + 1, dtype=np.float64)
    return CubicSpline(knots, w, bc_type="not-a-knot").derivative()(knots) * fs / (2.0 * np.pi)


def freq_vector(N, fs):
    """The two-sided frequency vector of N points (the last point is fs - fs / N, the Nyquist point fs / 2, as stated)."""
    res = fs / N
    f = res * np.arange(N, dtype=np.float64)
    if N % 2 == 0:
        f[N // 2] = fs / 2.0
    if N > 1:
        f[N - 1] = fs - res
    return f


def phase(N):
    """The modified STFT's phase exp(-2 pi i (N // 2) k / N), complex128 (for an even N exactly (-1)^k)."""
    if N % 2 == 0:
        return np.where(np.arange(N) % 2 == 0, 1.0, -1.0).astype(np.complex128)
    return np.exp(-2j * np.pi * (N // 2) * np.arange(N) / N)


def rows_from_shift(fcorr, N, fs):
    """Destination row of every cell from its frequency correction: MATLAB rounding (half away from zero), cyclic modulo."""
    fk = freq_vector(N, fs)
    coord = (fk[:, None] + fcorr - fk[0]) * (N - 1) / (fk[-1] - fk[0])
    r = np.sign(coord) * np.floor(np.abs(coord) + 0.5)
    return np.mod(r, N).astype(np.int64)


def stft64(x, window):
    """(N, n) complex128 STFT before the phase."""
    w = np.asarray(window, dtype=np.float64).ravel()
    return np.fft.fft(frames(np.asarray(x, dtype=np.float64), w.size) * w[None, :], axis=1).T


def rows(x, fs, window):
    """(N, n) int64: the synchrosqueezing row of every (source row, column) cell, float64."""
    w = np.asarray(window, dtype=np.float64).ravel()
    V = stft64(x, w)
    Vd = np.fft.fft(frames(np.asarray(x, dtype=np.float64), w.size) * dtwin(w, fs)[None, :], axis=1).T
    with np.errstate(divide="ignore", invalid="ignore"):
        fcorr = -np.imag(Vd / V)
    fcorr[~np.isfinite(fcorr)] = 0.0
    return rows_from_shift(fcorr, w.size, fs)


def squeeze(V, rws, klo, K):
    """Rows klo .. klo + K - 1 of the synchrosqueezed transform: (N, n) values V (phase not yet applied) added at their rows, in
    V's own precision (complex64 stays complex64), source rows in ascending order."""
    N, n = V.shape
    Vm = V * phase(N).astype(V.dtype)[:, None]
    keep = (rws >= klo) & (rws < klo + K)
    S = np.zeros((K, n), dtype=V.dtype)
    cols = np.broadcast_to(np.arange(n)[None, :], rws.shape)
    np.add.at(S, (rws[keep] - klo, cols[keep]), Vm[keep])
    return S


def _table(window, N, twiddle):
    """(N taps, N bins) float32 real and imaginary window-twiddle tables.  ``twiddle``: "exact" rounds the float64 product once;
    "unreduced" is defect D5: cosf / sinf of the float32 angle 2 pi k n / N as it stands, not reduced modulo the period."""
    n = np.arange(N)
    if twiddle == "exact":
        T = np.asarray(window, np.float64)[:, None] * np.exp(-2j * np.pi * np.outer(n, n) / N)
        return T.real.astype(np.float32), T.imag.astype(np.float32)
    assert twiddle == "unreduced"
    ang = (np.float32(2.0 * np.pi) * np.outer(n, n).astype(np.float32)) / np.float32(N)
    assert ang.dtype == np.float32
    w32 = np.asarray(window).astype(np.float32)[:, None]
    return w32 * np.cos(ang), w32 * -np.sin(ang)


def stft32_direct(x, window, twiddle="exact"):
    """(N, n) complex64: float32 frames times the float32 table, one float32 matrix product per part."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    N = np.asarray(window).size
    tre, tim = _table(window, N, twiddle)
    F = np.ascontiguousarray(frames(x, N))
    vre, vim = F @ tre, F @ tim
    assert vre.dtype == np.float32
    return (vre + 1j * vim).astype(np.complex64).T


def float32_direct(x, window, rws, klo, K, twiddle="exact"):
    """float32 values by the direct product, squeezed on the rows given (``rows``: every decision right)."""
    return squeeze(stft32_direct(x, window, twiddle), rws, klo, K)


def float32_fft(x, window, rws, klo, K):
    """float32 values by scipy.fft.fft of the float32 windowed frames (scipy keeps complex64), squeezed on the rows given."""
    import scipy.fft
    x = np.asarray(x)
    assert x.dtype == np.float32
    w32 = np.asarray(window).astype(np.float32)
    V = scipy.fft.fft(frames(x, w32.size) * w32[None, :], axis=1)
    assert V.dtype == np.complex64, V.dtype
    return squeeze(np.ascontiguousarray(V.T), rws, klo, K)


def float32_zscore(S):
    """The reference's epilogue on (K, n) complex64 values: per half, mean and unbiased std in float32 torch ops over (n, K), then
    (v - m) / sd in float32.  Returns float32 (n, 2K)."""
    import torch
    assert S.dtype == np.complex64
    halves = []
    for part in (S.real, S.imag):
        v = torch.from_numpy(np.ascontiguousarray(part.T))
        assert v.dtype == torch.float32
        halves.append((v - v.mean()) / v.std(unbiased=True))
    return torch.cat(halves, dim=1).numpy()


def zscore64(S):
    """The same epilogue in float64 on (K, n) complex128 values: float64 (n, 2K)."""
    S = np.asarray(S, dtype=np.complex128)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.concatenate([(p.T - p.mean()) / p.std(ddof=1) for p in (S.real, S.imag)], axis=1)


def rows_d6(x, fs, window, rws64, smax):
    """Defect D6: the decision of every cell with |V| < SMALL_CELL x ``smax`` (the signal's largest feature) comes from the float32
    restatement's own shift -- V and the derivative-window transform by ``stft32_direct``, their quotient in complex64 --; float64
    rows everywhere else.  Returns (rows, number of cells whose row changed)."""
    w = np.asarray(window, dtype=np.float64).ravel()
    V = stft32_direct(x, w)
    Vd = stft32_direct(x, dtwin(w, fs))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = Vd / V
    assert q.dtype == np.complex64
    fcorr = -np.imag(q).astype(np.float64)
    fcorr[~np.isfinite(fcorr)] = 0.0
    small = np.abs(V) < SMALL_CELL * smax
    out = np.where(small, rows_from_shift(fcorr, w.size, fs), rws64)
    return out, int((out != rws64).sum())


# ---- the canonical fold's arithmetic class --------------------------------------------------------------------------------------
def _f16_halves(v):
    """v = v1 + v2 with both halves rounded to float16, returned as float32."""
    v = np.asarray(v, dtype=np.float32)
    v1 = v.astype(np.float16).astype(np.float32)
    v2 = (v - v1).astype(np.float16).astype(np.float32)
    return v1, v2


def _pow2_scale(energy):
    """2^(14 - hb) with sqrt(energy) < 2^hb: the tile's samples times it stay below 2^14 (fsst_canon128.hpp, canon_land)."""
    if not (energy > 0.0 and np.isfinite(energy)):
        return 1.0
    hb = (int(np.floor(np.log2(energy))) + 2) >> 1
    return 2.0 ** (14 - hb)


def block_span(j, n, N):
    """[lo, hi) of the samples that the frames of block j read, clipped to the signal."""
    m = N // 2
    return max(BLOCK * j - m, 0), min(BLOCK * j + BLOCK - 1 + N - 1 - m + 1, n)


def split_f16(x, window, rws, klo, K, drop_x2=False, drop_c2=False, drop_c2_tap=None, one_scale=False, finite_energy=False):
    """The split-f16 emulation.  Per aligned 64-frame tile one power-of-two scale from the sum of squares of the samples its frames
    read; samples x = x1 + x2 and constants c = c1 + c2 (c = window x twiddle, scaled by one power of two into [2^13, 2^14)), each
    half rounded to float16; the four products x1 c1 + x1 c2 + x2 c1 + x2 c2 over all taps accumulated in float32 by one float32
    matrix product; scaled back (exact) and squeezed on the rows given.

    It emulates the arithmetic CLASS of fsst_canon_kernel / fsst_team16_kernel (which numbers are rounded to what), NOT their
    instruction order: the kernels fold eight terms per tap on the matrix pipe and finish with float32 radix stages, this takes
    the whole DFT as one product.  Agreement is to a small multiple of float32, not to the bit.

    Defects, one thing each: D1 ``drop_x2``; D2 ``drop_c2``; D3 ``drop_c2_tap=N // 2`` (the lo constants of one tap);
    D4 ``one_scale`` (one scale from the whole signal's energy instead of one per tile).
    A tile whose energy is not finite (it reads a NaN or an infinite sample) takes scale 1, as canon_land does; ``finite_energy``
    takes the energy over the tile's finite samples instead (tests/nonfinite_cases.py)."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    w = np.asarray(window, dtype=np.float64).ravel()
    N, n = w.size, x.size
    taps = np.arange(N)
    C = w[:, None] * np.exp(-2j * np.pi * np.outer(taps, taps) / N)
    cmax = max(np.abs(C.real).max(), np.abs(C.imag).max())
    cs = 2.0 ** (13 - int(np.floor(np.log2(cmax))))
    c1, c2 = _f16_halves(np.concatenate([C.real, C.imag], axis=1) * cs)           # (N taps, 2N)
    if drop_c2:
        c2 = np.zeros_like(c2)
    if drop_c2_tap is not None:
        c2 = c2.copy()
        c2[drop_c2_tap] = 0.0
    cmat = np.concatenate([c1, c2, c1, c2], axis=0)                                # (4N, 2N)
    F = frames(x, N)
    x64 = x.astype(np.float64)
    V = np.empty((N, n), dtype=np.complex64)
    sq = x64 * x64
    if finite_energy:
        sq = np.where(np.isfinite(x64), sq, 0.0)
    whole = _pow2_scale(float(sq.sum()))
    for j in range((n + BLOCK - 1) // BLOCK):
        lo, hi = block_span(j, n, N)
        sx = whole if one_scale else _pow2_scale(float(sq[lo:hi].sum()))
        t0, t1 = BLOCK * j, min(BLOCK * j + BLOCK, n)
        x1, x2 = _f16_halves(F[t0:t1] * np.float32(sx))
        if drop_x2:
            x2 = np.zeros_like(x2)
        acc = np.concatenate([x1, x1, x2, x2], axis=1) @ cmat                      # float32 accumulation
        assert acc.dtype == np.float32
        acc = acc * np.float32(1.0 / (sx * cs))                                    # a power of two
        V[:, t0:t1] = (acc[:, :N] + 1j * acc[:, N:]).astype(np.complex64).T
    return squeeze(V, rws, klo, K)


# ---- the metric ----------------------------------------------------------------------------------------------------------------
def cell_error(out, ref):
    """|out - ref| per cell in float64; complex inputs: the larger of the real and the imaginary part's error."""
    d = np.asarray(out).astype(np.complex128) - np.asarray(ref).astype(np.complex128)
    return np.maximum(np.abs(d.real), np.abs(d.imag))


def block_ratios(out, ref, x, window, halfdist, col0=0):
    """``out`` / ``ref``: (K, ncols) features of one signal (kept rows only; complex, or real for abs), columns col0 .. col0 + ncols - 1
    of the transform of ``x``.  Per aligned block [64 j, 64 j + 64) that holds one of those columns: u_j = 2^-24 ||span_j||_2 max|w|,
    e_j = the largest cell error over the kept rows and the block's columns that are not rounding-fragile (the oracle's halfdist
    < parity.FRAG_EPS, as parity.check), ratio_j = e_j / u_j; a block with u_j = 0 must have e_j = 0 (ratio 0, else inf).
    Returns (list of dicts block / ratio / e / u / row / col, number of fragile columns met, blocks left without a robust column)."""
    x64 = np.asarray(x, dtype=np.float64).ravel()
    w = np.asarray(window, dtype=np.float64).ravel()
    err = cell_error(out, ref)
    K, ncols = err.shape
    colidx = col0 + np.arange(ncols)
    fragile = np.asarray(halfdist)[colidx] < parity.FRAG_EPS
    res, empty = [], 0
    for j in range(col0 // BLOCK, (col0 + ncols - 1) // BLOCK + 1):
        sel = (colidx // BLOCK == j) & ~fragile
        if not sel.any():
            empty += 1
            continue
        lo, hi = block_span(j, x64.size, w.size)
        u = 2.0 ** -24 * float(np.sqrt((x64[lo:hi] ** 2).sum())) * float(np.abs(w).max())
        e = err[:, sel]
        flat = int(np.argmax(e))
        ej = float(e.ravel()[flat])
        if not np.isfinite(ej):
            ratio = float("inf")
        elif u > 0.0:
            ratio = ej / u
        else:
            ratio = 0.0 if ej == 0.0 else float("inf")
        res.append(dict(block=j, ratio=ratio, e=ej, u=u, row=flat // e.shape[1], col=int(colidx[sel][flat % e.shape[1]])))
    return res, int(fragile.sum()), empty


def worst(blocks):
    """The block with the largest ratio."""
    return max(blocks, key=lambda b: b["ratio"])


def z_ratio(z, z64, halfdist):
    """max|z - z64| / max|z64| of one signal's (n, 2K) z-scores over the columns that are not rounding-fragile."""
    robust = np.asarray(halfdist) >= parity.FRAG_EPS
    z64 = np.asarray(z64, dtype=np.float64)
    d = np.abs(np.asarray(z, dtype=np.float64) - z64)[robust]
    if not np.isfinite(d).all():
        return float("inf")
    return float(d.max() / np.abs(z64[robust]).max())


def old_gate(S, ref64, halfdist):
    """(passes, rel max, rel L2): whether (K, n) complex features pass parity.check at 1e-4 against the oracle cast to float32 (the
    suite's gate), and the two figures it gates, over the robust columns.  An emulation is no kernel: the session's tally of
    parity.check is left as it was."""
    S = np.asarray(S).astype(np.complex64)
    ref = np.asarray(ref64).astype(np.complex64)
    rob = np.asarray(halfdist) >= parity.FRAG_EPS
    d = (S.astype(np.complex128) - ref.astype(np.complex128))[:, rob]
    figures = (float(np.abs(d).max() / np.abs(ref).max()), float(np.linalg.norm(d) / np.linalg.norm(ref[:, rob])))
    tally = dict(parity.TALLY)
    try:
        parity.check(S, ref, halfdist, 1)
        return (True,) + figures
    except AssertionError:
        return (False,) + figures
    finally:
        parity.TALLY.update(tally)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def dyn_stretch(n):
    """[a, b) of the stretch that the ``dyn`` input makes 80 dB quieter: samples 640 .. 1343 of a 2000-sample window, and the same
    proportions, on block boundaries, of a shorter one (640: 192 .. 447; 704: 256 .. 447; 48: all of it)."""
    return BLOCK * int(round(0.32 * n / BLOCK)), BLOCK * int(round(0.672 * n / BLOCK))


_SEED = {"pcg": 7101, "noise": 7102, "dyn": 7103, "amp": 7104, "offset": 7105, "deep": 7103}
_SIGNALS = {}


def signals(name, n, fs=1000):
    """The named input set as float32 (2, n), read-only.
      pcg     synth.pcg_windows                          noise   seeded N(0, 1)
      dyn     a pcg window with ``dyn_stretch`` x 1e-4     deep    the same windows with the stretch x 1e-6 (120 dB)
      amp     one pcg window x 2^-40 and x 2^40           offset  pcg + 3
      clicks  unit impulses every 131 and every 193 samples (at most two in any block's span, nothing else)
      tone    cos(2 pi 117.3 t) and the same tone with a phase, amplitude-modulated by 30 % at 3 Hz (off a bin: under a window
              with low sidelobes every leakage cell is small against its frame and moves by many rows)
    ``deep``, ``clicks`` and ``tone`` are the inputs the CPU study needed to tell D4, D3 and D6 from float32 (see
    tests/test_fsst_precision.py)."""
    key = (name, n, fs)
    if key not in _SIGNALS:
        t = np.arange(n, dtype=np.float64) / fs
        if name == "noise":
            x = synth.noise_windows(2, n, seed=_SEED[name] + n)
        elif name == "clicks":
            x = np.zeros((2, n))
            x[0, 65::131] = 1.0
            x[1, 96::193] = 1.0
        elif name == "tone":
            x = np.stack([np.cos(2 * np.pi * 117.3 * t), np.cos(2 * np.pi * 117.3 * t + 0.7) * (1 + 0.3 * np.sin(2 * np.pi * 3 * t))])
        else:
            x = synth.pcg_windows(2, n, fs=fs, seed=_SEED[name] + n).astype(np.float64)
            if name in ("dyn", "deep"):
                a, b = dyn_stretch(n)
                x[:, a:b] *= 1e-4 if name == "dyn" else 1e-6
            elif name == "amp":
                x[1] = x[0]
                x[0] *= 2.0 ** -40
                x[1] *= 2.0 ** 40
            elif name == "offset":
                x = x + 3.0
        x = np.ascontiguousarray(x, dtype=np.float32)
        x.setflags(write=False)
        _SIGNALS[key] = x
    return _SIGNALS[key]


def window(case):
    """The case's analysis window, float64: Kaiser(nwin, 0.5) unless the case says Hann."""
    return np.hanning(case["nwin"]).astype(np.float64) if case.get("window") == "hann" else synth.kaiser_window(case["nwin"], 0.5)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def _case(id, kernel, call, n, inputs, gate, nwin=128, fs=1000, band=BAND, launch=None, **extra):
    """``kernel``: the text last_kernel() must contain; ``launch``: the row of tests/launch_cases.py whose recorded name it must
    contain as well (same call and shape class), None where the table has no such row; ``call``: unnormalized / stack / abs / raw /
    ragged / stream; ``gate``: "block" or "z"."""
    return dict(id=id, kernel=kernel, launch=launch, call=call, n=n, inputs=inputs, gate=gate, nwin=nwin, fs=fs, band=band, **extra)


_CANON = "fsst_canon_kernel<4, 22, false>"
_TEAM = "fsst_team16_kernel<4, 22, 16, 2>"
CASES = [
    # the canonical band: fs 1000, (25, 200)
    _case("canon_2000", _CANON, "unnormalized", 2000, ("pcg", "noise", "dyn", "amp", "offset", "deep"), "block"),
    _case("canon_32", _CANON, "unnormalized", 32, ("pcg", "noise"), "block"),
    # (two rows the CPU study asked for: impulses, whose float32 figure is small enough to show the lo constant of the centre tap;
    #  tones and pcg under a Hann window, where cells far below the signal's maximum move)
    _case("canon_clicks", _CANON, "unnormalized", 640, ("clicks",), "block"),
    _case("canon_hann", _CANON, "unnormalized", 640, ("tone", "pcg"), "block", window="hann"),
    _case("team_2000", _TEAM + " teams of 16", "stack", 2000, ("pcg", "noise", "dyn", "offset", "deep"), "z", launch="the workload's length"),
    _case("team_48", _TEAM + " teams of 1", "stack", 48, ("pcg", "noise", "dyn", "offset"), "z", launch="3 groups: its lower edge"),
    _case("two_launch_2000", _CANON, "stack", 2000, ("pcg",), "z", launch="two launches asked for", zpath="two_launch"),
    _case("canon_2064", _CANON, "stack", 2064, ("pcg",), "z", launch="129 groups: past it"),
    _case("ragged", _CANON[:-1] + ", ragged>", "ragged", (48, 2000, 333), ("pcg",), "z", launch="ragged 128 stack"),
    _case("tile_flag_cols", "fsst_core128_kernel<16, 8, 64, true", "unnormalized", 400, ("pcg",), "block",
          launch="unnormalized, columns (8, 64)", cols=(8, 64)),
    # the second canonical band: fs 2000, (25, 400)
    _case("band2_unnorm", "<2, 24", "unnormalized", 640, ("pcg", "dyn"), "block", fs=2000, band=(25, 400)),
    _case("band2_stack", "<2, 24", "stack", 640, ("pcg", "dyn"), "z", fs=2000, band=(25, 400)),
    # other 128-point configurations
    _case("n128_odd_k", "fsst_core128_kernel", "unnormalized", 640, ("pcg", "dyn"), "block", band=(25, 195)),
    _case("n128_abs", "fsst_core128_kernel", "abs", 640, ("pcg", "dyn"), "block"),
    _case("n128_raw_all", "fsst_core128_kernel", "raw", 640, ("pcg", "dyn"), "block", band=None),
    # other window lengths
    _case("n256_unnorm", "fsst_core128_kernel<16, 16,", "unnormalized", 640, ("pcg", "dyn"), "block", nwin=256),
    _case("n256_raw_all", "fsst_core_kernel<8, 64>", "raw", 640, ("pcg", "dyn"), "block", nwin=256, band=None),
    _case("n512_unnorm", "pairs", "unnormalized", 704, ("pcg", "dyn"), "block", nwin=512),
    _case("n512_raw_all", "fsst_core_kernel<16, 64>", "raw", 704, ("pcg", "dyn"), "block", nwin=512, band=None),
    _case("n64_unnorm", "fsst_core_kernel<2, 64>", "unnormalized", 400, ("pcg", "noise"), "block", nwin=64),
    _case("n32_unnorm", "fsst_core_kernel<1, 64>", "unnormalized", 400, ("pcg", "noise"), "block", nwin=32),
    _case("n100_unnorm", "fsst_dft_kernel", "unnormalized", 400, ("pcg", "noise"), "block", nwin=100),
    _case("n33_hann", "fsst_dft_kernel", "unnormalized", 400, ("pcg", "noise"), "block", nwin=33, window="hann"),
    # (one row per input: pooled with pcg, whose R32 is three times that of noise, D5 on noise is 16 x -- on the line)
    _case("n1024_unnorm", "fsst_dft_kernel", "unnormalized", 320, ("pcg",), "block", nwin=1024),
    _case("n1024_noise", "fsst_dft_kernel", "unnormalized", 320, ("noise",), "block", nwin=1024),
]
CASE_BY_ID = {c["id"]: c for c in CASES}
STREAM_CASE = "canon128"      # of tests/stream_cases.py: the canonical class through the rolling step


def case_signals(case):
    """[(label, float32 signal)] of a case: every signal of every named input set; a ragged case: one recording per length."""
    out = []
    for name in case["inputs"]:
        if case["call"] == "ragged":
            out += [(f"{name}/{n}", signals(name, n, case["fs"])[0]) for n in case["n"]]
        else:
            out += [(f"{name}[{b}]", x) for b, x in enumerate(signals(name, case["n"], case["fs"]))]
    return out


def is_canonical(case):
    """The cases whose kernels run the split-f16 fold: the emulation study covers their inputs."""
    return case["nwin"] == 128 and case["band"] in (BAND, (25, 400)) and case["call"] != "abs" and "cols" not in case
