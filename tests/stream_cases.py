"""The rolling (streaming) FSST step restated on the host: what tests/test_streaming.py holds the device to.  numpy only.

A stream's running state is ``{count, mean, M2}`` of the real block ``[:, :K]`` and of the imaginary block ``[:, K:]`` of every
un-normalised column it has emitted, the columns of the first steps (whose frames reach into the zero history) included; a step's
normalised output is ``(v - mean) / sqrt(M2 / (count - 1))`` with the state AFTER that step.  Three restatements of the state:

* ``running_reference``: two passes over everything seen so far, float64.  The truth.
* ``chan_reference``: the Chan merge of per-chunk ``{sum, sum of squares}`` -- what ``merge_state`` (csrc/fsst_device.hpp) says it does.
* ``welford_reference``: element by element through ``moments.update_mean`` / ``update_variance``, the mirror of the reference
  project's ``hss.moments``.

The gate of the normalised output is stated here once (``output_gate``), with its derivation.
"""
import numpy as np

from heart_sounds_segmentation_amd import synth

BLOCKS = ("re", "im")


def blocks(a):
    """The real and the imaginary block of ``(..., 2K)`` features."""
    K = a.shape[-1] // 2
    return {"re": a[..., :K], "im": a[..., K:]}


def state_std(count, m2):
    """Unbiased standard deviation of a ``{count, mean, M2}`` state (NaN / inf where ``count == 1``, as in the kernel)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(np.float64(m2) / (np.float64(count) - 1.0))


def running_reference(chunks):
    """``chunks``: one channel's un-normalised float32 ``(chunk, 2K)`` arrays, one per step.  Returns one dict per step:
    ``{"re": {count, mean, M2, rms}, "im": {...}, "z": float64 (chunk, 2K)}`` over EVERYTHING seen up to and including that step,
    two-pass in float64; ``z`` is that step's chunk z-scored with those statistics."""
    out = []
    seen = {b: [] for b in BLOCKS}
    for ch in chunks:
        ch = np.asarray(ch)
        assert ch.dtype == np.float32 and ch.ndim == 2 and ch.shape[1] % 2 == 0
        cur = blocks(ch.astype(np.float64))
        step = {}
        z = []
        for b in BLOCKS:
            seen[b].append(cur[b].ravel())
            v = np.concatenate(seen[b])
            count = v.size
            mean = v.sum() / count
            d = v - mean
            m2 = float((d * d).sum())
            step[b] = {"count": count, "mean": float(mean), "M2": m2, "rms": float(np.sqrt((v * v).sum() / count))}
            with np.errstate(divide="ignore", invalid="ignore"):
                z.append((cur[b] - mean) / state_std(count, m2))
        step["z"] = np.concatenate(z, axis=1)
        out.append(step)
    return out


def chan_reference(chunks):
    """The same ``{count, mean, M2}`` per step and block by the Chan merge of per-chunk sums, float64: block b of ``nb`` elements
    with sum ``s`` and sum of squares ``q`` has ``mean_b = s / nb``, ``M2_b = q - s mean_b``; merged into ``{na, mean_a, M2_a}``:
    ``delta = mean_b - mean_a``, ``mean = mean_a + delta nb / n``, ``M2 = M2_a + M2_b + delta^2 na nb / n``, ``n = na + nb``."""
    out = []
    st = {b: (0.0, 0.0, 0.0) for b in BLOCKS}
    for ch in chunks:
        cur = blocks(np.asarray(ch).astype(np.float64))
        step = {}
        for b in BLOCKS:
            v = cur[b].ravel()
            nb, s, q = float(v.size), float(v.sum()), float((v * v).sum())
            mean_b = s / nb
            m2_b = q - s * mean_b
            na, mean_a, m2_a = st[b]
            nn = na + nb
            delta = mean_b - mean_a
            st[b] = (nn, mean_a + delta * (nb / nn), m2_a + m2_b + delta * delta * (na * nb / nn))
            step[b] = {"count": int(st[b][0]), "mean": st[b][1], "M2": st[b][2]}
        out.append(step)
    return out


def welford_reference(chunks):
    """The same per step and block, one element at a time through the library's host functions ``moments.update_mean`` /
    ``moments.update_variance`` (the recurrences of the reference project's ``hss.moments``): needs the built library, no GPU."""
    from heart_sounds_segmentation_amd.moments import update_mean, update_variance
    out = []
    st = {b: [0, 0.0, 0.0] for b in BLOCKS}
    for ch in chunks:
        cur = blocks(np.asarray(ch).astype(np.float64))
        step = {}
        for b in BLOCKS:
            k, m, m2 = st[b]
            for x in cur[b].ravel().tolist():
                k += 1
                m2 = update_variance(x, m, m2, k)        # (takes the mean BEFORE x)
                m = update_mean(m, x, k)
            st[b] = [k, m, m2]
            step[b] = {"count": k, "mean": m, "M2": m2}
        out.append(step)
    return out


# ---- gates -----------------------------------------------------------------------------------------------------------------
# State: the figures tests/test_gpu_parity.py::test_moments_merge_any_shape uses.  merge_state forms M2_b = q - s mean_b, whose
# error grows like (1 + mean^2 / var) times a few tens of ulps of q: with mean^2 / var <= MAX_MEAN2_OVER_VAR (asserted on the
# reference by the tests that use DC offsets) the expected error is around 3e-12, at least 30 x inside the gate.
MEAN_RTOL = 1e-12            # |d mean| <= MEAN_RTOL max(|mean|, rms)
M2_RTOL = 1e-10              # |d M2| <= M2_RTOL M2
MAX_MEAN2_OVER_VAR = 1e3


def state_ratios(got, want):
    """``got``: (count, mean, M2) of the device; ``want``: a block of ``running_reference``.  Returns the errors as fractions of
    their gates (count: 0.0 when equal, inf otherwise)."""
    count, mean, m2 = got
    r_count = 0.0 if count == want["count"] else float("inf")
    r_mean = abs(mean - want["mean"]) / (MEAN_RTOL * max(abs(want["mean"]), want["rms"]))
    r_m2 = abs(m2 - want["M2"]) / (M2_RTOL * want["M2"])
    return r_count, r_mean, r_m2


# Normalised output.  The kernels compute (v - float(mean)) * (1.0f / float(sqrt(var))) in float32 from the float64 state: four
# roundings of relative size 2^-24 each on the path of z = (v - mean) / sigma -- the difference, sqrt(var) to float32, its
# reciprocal, the product -- which is 2^-22 |z|, and the rounding of the mean to float32, an absolute 2^-24 |mean| that the
# division by sigma carries into z.  Derived bound: |err| <= 2^-22 |z| + 2^-24 |mean| / sigma.  The gate is TWICE that, plus
# 1e-9 (1 + |z|) for the state's own error (MEAN_RTOL and M2_RTOL move z by far less).  A numpy float32 emulation of the kernel's
# expression reaches 0.85 of the derived bound over offsets 0 .. 3000 sigma and scales 1e-6 .. 1e5 (tests/test_streaming.py keeps
# it below half the gate).
def output_gate(z, mean, sigma):
    z = np.abs(np.asarray(z, dtype=np.float64))
    return 2.0 * (2.0 ** -22 * z + 2.0 ** -24 * abs(mean) / sigma) + 1e-9 * (1.0 + z)


def normalize_f32(v, mean, sigma):
    """The kernels' expression in numpy float32: ``v`` float32, ``mean`` / ``sigma`` float64."""
    m = np.float32(mean)
    inv = np.float32(1.0) / np.float32(sigma)
    return (np.asarray(v, dtype=np.float32) - m) * inv


def output_ratio(got, step):
    """Largest |got - z| / gate over one step's normalised ``(chunk, 2K)`` output; ``step``: that step of ``running_reference``.
    Where the reference is not finite (count 1, or a constant block) the output must be non-finite in the same places."""
    got = np.asarray(got, dtype=np.float64)
    K = got.shape[1] // 2
    worst = 0.0
    for b, sl in (("re", slice(0, K)), ("im", slice(K, 2 * K))):
        want = step["z"][:, sl]
        sigma = state_std(step[b]["count"], step[b]["M2"])
        ok = np.isfinite(want)
        if not np.array_equal(np.isfinite(got[:, sl]), ok):
            return float("inf")
        if ok.any():
            gate = output_gate(want[ok], step[b]["mean"], sigma)
            worst = max(worst, float((np.abs(got[:, sl][ok] - want[ok]) / gate).max()))
    return worst


# ---- columns ---------------------------------------------------------------------------------------------------------------
def lookahead(nwin):
    """Samples between a stream column's centre and the newest sample of its frame: the frame of the column centred on sample c
    covers ``c - nwin // 2 .. c - nwin // 2 + nwin - 1``."""
    return nwin - 1 - nwin // 2


def offline_column(t, nwin):
    """The column of the offline, zero-padded transform that stream column ``t`` equals; ``t`` counts the stream's columns from
    its first one, whose frame ends on the first real sample (negative: the column lies in the zero history)."""
    return t - lookahead(nwin)


# ---- cases -----------------------------------------------------------------------------------------------------------------
def _case(id, fs, nwin, window, band, channels, chunk, slots, steps, route, dc=False, seed=0):
    return dict(id=id, fs=fs, nwin=nwin, window=window, band=band, channels=channels, chunk=chunk, slots=slots, steps=steps,
                route=route, dc=dc, seed=seed)


KAISER = ("kaiser", 0.5)
# route "stream": the whole step is one launch (fsst_core128_kernel<..., stream>); "three": copy + transform + merge-and-normalise
CASES = [
    _case("c5", 4000, 512, KAISER, (25, 200), 64, 128, 2, 5, "stream", seed=51),            # one launch, wave pairs, several blocks per channel
    _case("one_channel", 4000, 512, KAISER, (25, 200), 1, 128, 1, 4, "stream", seed=52),    # blocks per channel = groups; wraps at every step
    # (rows 8 .. 13: K = 6.  The band (30, 50) keeps 5 rows, and an odd band has no wide-store epilogue, so no one-launch step)
    _case("n256", 1000, 256, KAISER, (30, 52), 3, 48, 3, 7, "stream", dc=True, seed=53),    # one launch, 16 taps
    _case("many_channels", 4000, 512, KAISER, (25, 200), 300, 48, 2, 3, "stream", seed=54),  # 900 <= 1024 group slots, one block per channel
    _case("over_tiny", 4000, 512, KAISER, (25, 200), 300, 80, 2, 3, "three", seed=55),      # 1500 > 1024 group slots
    _case("short_chunk", 4000, 512, "hann", (25, 200), 5, 13, 1, 9, "stream", dc=True, seed=56),   # a partial single group; overlapping wrap copies
    _case("nine_groups", 4000, 512, KAISER, (25, 200), 4, 144, 2, 4, "three", seed=57),     # 9 groups > 8
    _case("canon128", 1000, 128, KAISER, (25, 200), 5, 48, 2, 8, "three", dc=True, seed=58),   # the canonical class through exec_frames
    _case("odd_k", 1000, 128, KAISER, (25, 210), 3, 17, 3, 6, "three", dc=True, seed=59),   # odd K: scalar normalise path, non-wide piece_moments
    _case("long_chunk", 1000, 128, "hann", (25, 200), 2, 300, 2, 3, "three", seed=60),      # 19 pieces > 16; chunk > nwin
    _case("dft100", 1000, 100, "hann", (0, 120), 2, 50, 2, 6, "three", dc=True, seed=61),   # the any-length kernel; the band holds the DC row
    _case("odd33", 1000, 33, "hann", (0, 250), 2, 20, 2, 5, "three", seed=62),              # an odd window: the column shift
    _case("n64_one", 1000, 64, KAISER, (25, 200), 2, 1, 64, 40, "three", seed=63),          # one column per step, the generic kernel
]
CASE_BY_ID = {c["id"]: c for c in CASES}


def window(case):
    """The case's symmetric analysis window, float64."""
    if case["window"] == "hann":
        return np.hanning(case["nwin"]).astype(np.float64)
    kind, beta = case["window"]
    assert kind == "kaiser"
    return np.kaiser(case["nwin"], beta).astype(np.float64)


def amplitudes(channels):
    """Per-channel amplitudes spread over 1e-3 .. 1e3 (a single channel: 1)."""
    return np.ones(1) if channels == 1 else 10.0 ** np.linspace(-3.0, 3.0, channels)


def signals(case):
    """float32 ``(channels, steps * chunk)``: ``synth.pcg_windows`` times the channel's amplitude, plus 0.25 x the amplitude as an
    offset in the cases marked ``dc``."""
    n = case["steps"] * case["chunk"]
    x = synth.pcg_windows(case["channels"], n, fs=case["fs"], seed=case["seed"]).astype(np.float64)
    amp = amplitudes(case["channels"])[:, None]
    x = x * amp
    if case["dc"]:
        x = x + 0.25 * amp
    return x.astype(np.float32)


def oracle_channels(channels):
    """At most three channels for the oracle: the first, one in between, the last."""
    return sorted({0, channels // 2, channels - 1})
