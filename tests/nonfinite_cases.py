"""Inputs that hold a NaN or an infinite value, their clean twins, and the three rules such a call is held to.

  R1  neighbours      every signal, frame, recording or batch row that does not hold the value is bit-identical to the same call
                      without it;
  R2  no silent value in the unit that holds it an output element is non-finite where the float64 reference ON THE SAME DIRTY INPUT is
                      non-finite, and within the existing gate of that reference where the reference is finite (tests/parity.py for
                      features, 2e-5 for log-probs and y / hn / cn, 1e-4 of the tensor's maximum for gradients);
  R3  extent (FSST)   the reference's non-finite set is the one the oracle gives: for raw, abs and un-normalised STACK the columns
                      whose window holds the sample, in every kept row; for z-scored STACK the whole signal.

No tolerance of its own: every comparison is bit equality, an existing gate, or finiteness.  This module holds

  VALUES / positions / dirty                 the values, where they go, and a dirty copy of a clean input;
  nonfinite_set / check_subset / check_r2    the non-finite elements of a reference, parity.check on the columns outside them, and
                                             both together (R2 and R3 of one signal);
  oracle_features                            the oracle in the layout of a launch row (un-normalised STACK from the raw transform);
  seg_dirty / check_seg_rows                 a dirty feature tensor for the segmenter and R1 + R2 on log-probs;
  canon_scale_emulation                      the canonical tile's scale choice on the CPU (tests/fsst_precision_cases.split_f16);
  report                                     the figures of a run, for profiles/nonfinite.txt.

A helper module, not a conftest: the tests import it."""
import math
import os

import numpy as np
import torch

from heart_sounds_segmentation_amd import synth
from tests import fsst_precision_cases as fp
from tests import parity

VALUES = {"nan": math.nan, "+inf": math.inf, "-inf": -math.inf}
SEG_GATE = 2e-5             # log-probs and y / hn / cn (tests/segmenter_cases.py: GATE)
GRAD_GATE = parity.TOL      # gradients: max|g - g64| / max|g64| per tensor


def positions(n):
    """The sample positions, clipped to the signal: the first sample; 190, the last of the 191 samples that the canonical tile of
    columns 64 .. 127 reads, which only that tile's last column holds; the last sample."""
    return sorted({0, min(190, n - 1), n - 1})


def dirty(x, pos, value):
    """A copy of ``x`` (numpy or torch, any shape) with ``value`` at ``pos`` of its last axis ... or at the index tuple ``pos``."""
    y = x.clone() if isinstance(x, torch.Tensor) else np.array(x, copy=True)
    y[(Ellipsis, pos) if isinstance(pos, int) else pos] = value
    return y


# ------------------------------------------------------------------------------------------------ FSST
def nonfinite_set(ref):
    """Boolean array of ref's shape: the elements that are NaN or infinite (complex: either part)."""
    return ~np.isfinite(np.asarray(ref))


def columns(mask, time_axis):
    """(n,) bool: the time columns in which ``mask`` holds anywhere."""
    m = np.moveaxis(np.asarray(mask), time_axis, 0)
    return m.reshape(m.shape[0], -1).any(axis=1)


def window_columns(n, nwin, s):
    """(n,) bool: the columns whose window (frame t covers samples t - nwin // 2 .. t - nwin // 2 + nwin - 1) holds sample s."""
    t = np.arange(n)
    return (t - nwin // 2 <= s) & (s <= t - nwin // 2 + nwin - 1)


def check_subset(out, ref, halfdist, cols, time_axis, what=""):
    """parity.check's two clauses (and its count of fragile columns) on the time columns ``cols`` (bool mask or indices) of one
    signal: the scale is the largest reference feature of that subset, which must be finite there.  Returns parity.check's
    measurements; raises AssertionError."""
    cols = np.flatnonzero(cols) if np.asarray(cols).dtype == bool else np.asarray(cols)
    o, r = np.take(np.asarray(out), cols, axis=time_axis), np.take(np.asarray(ref), cols, axis=time_axis)
    assert np.isfinite(r).all(), f"{what}: the reference is not finite on the subset"
    assert np.isfinite(o).all(), f"{what}: non-finite output where the reference is finite"
    return parity.check(o, r, np.asarray(halfdist)[cols], time_axis, what=what)


def check_r2(out, ref, halfdist, time_axis, what=""):
    """R2 and R3 of one signal against the oracle on the same dirty input: the same elements non-finite, and parity.check on the
    columns the oracle has finite.  Returns {'nonfinite': columns in the set, 'rel', 'rel_l2', 'fragile'}."""
    out, ref = np.asarray(out), np.asarray(ref)
    assert out.shape == ref.shape and out.dtype == ref.dtype, (what, out.shape, ref.shape, out.dtype, ref.dtype)
    bad_o, bad_r = nonfinite_set(out), nonfinite_set(ref)
    co, cr = columns(bad_o, time_axis), columns(bad_r, time_axis)
    silent = int((bad_r & ~bad_o).sum())
    extra = int((bad_o & ~bad_r).sum())
    assert silent == 0, f"{what}: {silent} finite elements where the oracle is non-finite (columns {np.flatnonzero(columns(bad_r & ~bad_o, time_axis))[:8]})"
    assert extra == 0, (f"{what}: {extra} non-finite elements where the oracle is finite: {int((co & ~cr).sum())} whole columns outside the "
                        f"oracle's {int(cr.sum())}, first {np.flatnonzero(co & ~cr)[:8]}")
    res = {"nonfinite": int(cr.sum()), "rel": 0.0, "rel_l2": 0.0, "fragile": 0}
    if (~cr).any():
        m = check_subset(out, ref, halfdist, ~cr, time_axis, what)
        res.update(rel=m["rel"], rel_l2=m["rel_l2"], fragile=m["fragile"])
    return res


def oracle_features(oracle, x, case):
    """The oracle on ONE float32 signal in the layout the launch row's call returns -> (features, halfdist).  An un-normalised row
    (``cols``) is [real | imag] of the raw transform on the band, (n, 2K), cut to its columns."""
    w = synth.kaiser_window(case["nwin"], 0.5)
    if "cols" in case:
        raw, hd = oracle.features(x[None], case["fs"], w, case["band"], "raw", return_halfdist=True)
        col0, ncols = case["cols"]
        un = np.concatenate([raw[0].real.T, raw[0].imag.T], axis=1).astype(np.float32)
        return np.ascontiguousarray(un[col0:col0 + ncols]), hd[0][col0:col0 + ncols]
    out, hd = oracle.features(x[None], case["fs"], w, case["band"], case["mode"], return_halfdist=True)
    return out[0], hd[0]


def time_axis_of(case):
    return 1 if case["mode"] == "raw" else 0


# ------------------------------------------------------------------------------------------------ the canonical tile's scale
def canon_scale_emulation(x, window, fs, band_rows, finite_energy):
    """fsst_canon128.hpp: canon_land's scale choice restated on fsst_precision_cases.split_f16: a 64-column tile takes the power of
    two of its samples' energy, and scale 1 when that energy is not finite.  ``finite_energy``: the energy is taken over the tile's
    finite samples only.  Returns the (K, n) complex64 un-normalised band."""
    klo, K = band_rows
    return fp.split_f16(np.asarray(x, dtype=np.float32), window, fp.rows(x, fs, window), klo, K, finite_energy=finite_energy)


# ------------------------------------------------------------------------------------------------ the segmenter
def seg_rows(B):
    """The batch rows that take the dirty feature: the first, and both sides of the 16-row tile border where they exist."""
    return [b for b in (0, 15, 16) if b < B]


def seg_steps(T):
    return sorted({0, T // 2, T - 1})


def check_seg_rows(got, clean, ref64, dirty_rows, what=""):
    """(B, T, C) outputs.  R1: rows outside ``dirty_rows`` have the bits of ``clean`` (the same call on the clean input).  R2 in the
    dirty rows against the float64 reference on the dirty input: non-finite where it is, within 2e-5 where it is finite.  Returns
    {'nonfinite': elements, 'err': worst finite difference}."""
    got, clean, ref64 = got.detach().cpu(), clean.detach().cpu(), ref64.detach().cpu().double()
    worst, bad = 0.0, 0
    for b in range(got.shape[0]):
        if b not in dirty_rows:
            assert torch.equal(got[b], clean[b]), f"{what}: row {b} holds no dirty value and differs from the clean call"
            continue
        nf_ref, nf_got = ~torch.isfinite(ref64[b]), ~torch.isfinite(got[b])
        assert not (nf_ref & ~nf_got).any(), (f"{what}: row {b} has {int((nf_ref & ~nf_got).sum())} finite values where float64 is not "
                                               f"finite, e.g. {got[b][nf_ref & ~nf_got][:4].tolist()}")
        assert not (nf_got & ~nf_ref).any(), f"{what}: row {b} has {int((nf_got & ~nf_ref).sum())} non-finite values where float64 is finite"
        bad += int(nf_ref.sum())
        if (~nf_ref).any():
            e = float((got[b].double() - ref64[b])[~nf_ref].abs().max())
            worst = max(worst, e)
            assert e <= SEG_GATE, f"{what}: row {b} is {e:.3e} from float64 where it is finite"
    return {"nonfinite": bad, "err": worst}


# ------------------------------------------------------------------------------------------------ the record of a run
_LINES = []


def report(line):
    """Prints the line and keeps it; with HSS_NONFINITE_REPORT=<path> set, the lines kept so far are (re)written there -- that is
    how profiles/nonfinite.txt is made."""
    print(line)
    _LINES.append(line)
    path = os.environ.get("HSS_NONFINITE_REPORT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(_LINES) + "\n")
