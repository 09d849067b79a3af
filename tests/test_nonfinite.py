"""The offline FSST kernels and the BiLSTM segmenter where a sample or a feature is NaN or infinite (tests/nonfinite_cases.py: R1
neighbours, R2 no silent value, R3 extent).  Every comparison is bit equality, an existing gate or finiteness; every reference is
float64 on the SAME dirty input (the C oracle for features, stock nn.LSTM for the segmenter), and the expected non-finite set is
taken from it at test time.

Where a float decides an address or a loop bound in the FSST kernels, and what guards it (read before the first GPU run):

  the shift -> destination row   ``if (!(fabsf(shift) <= 1.0e6f)) shift = 0.0f`` before the row is rounded and converted, then
                                 ``& (NWIN - 1)`` or ``% N`` with the negative case folded back: fsst_kernels.hpp (float32 scatter and
                                 its float64 redo), fsst_mfma128.hpp (displaced_source, resolve_one, float64 ``fabs``),
                                 fsst_canon128.hpp (canon_decide), fsst_dft.hpp (the float32 decision and both float64 ones);
  the tie queues                 a cell is queued when ``fr * fr * den < bound * R2 && den > floor * R2``: with a NaN or infinite R2 or
                                 den the comparison is false, so the cell takes the float32 decision above.  fsst_dft.hpp draws slots
                                 with an atomic and writes only ``slot < kDftTieQueue``; the drain reads ``min(count, kDftTieQueue)``.
                                 The bitmaps of fsst_mfma128.hpp / fsst_canon128.hpp are indexed by (row, frame) of the lane, never
                                 by data;
  tile_energy / dcdom            E, S1 and the offset test are compared (``E > 0 && S1 * S1 >= theta * C * E``: false for NaN): they
                                 choose between the float32 transform, the exact float64 redo and the offset staging, all of which
                                 address by lane and group.  canon_land takes the EXPONENT of E as an integer: 255 (infinite or
                                 NaN) selects scale 1, no shift by it is made;
  the team kernel                fsst_team16_kernel lands its tiles through canon_land<true> like fsst_canon_kernel; what a group
                                 reports to the host is a flag word, and the hand-over to the two-launch kernels is decided from it
                                 on the host.

No site was found unguarded."""

import numpy as np
import pytest
import torch
from torch import nn

from heart_sounds_segmentation_amd import _lib, consumer, synth
from heart_sounds_segmentation_amd.consumer import HipBiLSTM, HipSegmenterHead, SegmenterHead, segment
from heart_sounds_segmentation_amd.transforms import FSST
from oracle import fsst_numpy
from tests import nonfinite_cases as nc
from tests import segmenter_cases as sc
from tests.launch_cases import LAUNCH_CASES, launch_call, launch_kernel, launch_transform
from tests.nonfinite_cases import VALUES, report
from tests.segmenter_cases import LENS18
from tests.test_half_features import same_as_cast

KAISER = synth.kaiser_window(128, 0.5)
BAND = (25, 200)
DENSE_CPU = [(3, 40, 12, 7), (17, 37, 240, 44)]
DENSE_GPU = DENSE_CPU + [(2, 9, 256, 3)]


def same_bits(a, b):
    """two tensors (or arrays) of one shape and type with the same bytes"""
    a, b = torch.as_tensor(a).detach().cpu().contiguous(), torch.as_tensor(b).detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ==================================================================================================== CPU: the references
@pytest.mark.parametrize("nwin", [128, 100, 256])
def test_oracles_agree_on_the_extent(nwin, oracle_mod):
    """The C oracle and oracle/fsst_numpy.py on a 600-sample signal with NaN / +Inf / -Inf at s = 0, 190, n - 1: the same elements
    non-finite -- every row of exactly the columns whose window holds s -- and every other column bit-identical to the clean
    transform.  The same for the band's raw, abs and un-normalised STACK features; z-scored STACK is NaN throughout."""
    n, fs = 600, 1000
    w = synth.kaiser_window(nwin, 0.5)
    x = synth.noise_windows(1, n, seed=nwin)[0]
    clean_c, clean_n = oracle_mod.fsst(x, fs, w)[0], fsst_numpy.fsst(x, fs, w)[0]
    case = dict(nwin=nwin, fs=fs, band=BAND)
    clean = {m: nc.oracle_features(oracle_mod, x, dict(case, mode=m))[0] for m in ("raw", "abs")}
    clean["unnorm"] = nc.oracle_features(oracle_mod, x, dict(case, mode="stack", cols=(0, n)))[0]
    for vname, v in VALUES.items():
        for s in nc.positions(n):
            xd = nc.dirty(x, s, v)
            want = nc.window_columns(n, nwin, s)
            got_c, got_n = oracle_mod.fsst(xd, fs, w)[0], fsst_numpy.fsst(xd, fs, w)[0]
            for name, got, cl in (("C", got_c, clean_c), ("numpy", got_n, clean_n)):
                bad = nc.nonfinite_set(got)
                assert np.array_equal(bad, np.broadcast_to(want[None, :], bad.shape)), (name, nwin, vname, s)
                assert same_bits(got[:, ~want], cl[:, ~want]), (name, nwin, vname, s)
            for mode, axis in (("raw", 1), ("abs", 0), ("unnorm", 0)):
                c = dict(case, mode="stack", cols=(0, n)) if mode == "unnorm" else dict(case, mode=mode)
                got = nc.oracle_features(oracle_mod, xd, c)[0]
                bad = np.moveaxis(nc.nonfinite_set(got), axis, 0)
                assert np.array_equal(bad, np.broadcast_to(want.reshape((-1,) + (1,) * (bad.ndim - 1)), bad.shape)), (mode, nwin, vname, s)
                assert same_bits(np.compress(~want, got, axis=axis), np.compress(~want, clean[mode], axis=axis)), (mode, nwin, vname, s)
            z = oracle_mod.features(xd[None], fs, w, BAND, "stack")
            assert np.isnan(z).all(), (nwin, vname, s)


@pytest.mark.parametrize("B,T,H,F", DENSE_CPU)
def test_stock_segmenter_meets_r1_and_r2(B, T, H, F):
    """Stock SegmenterHead (nn.LSTM, torch.relu) in float64 and float32: a NaN feature at t = 0, mid, T - 1 makes exactly its row
    NaN, at every step; +-Inf features leave everything finite; every other row has the bits of the clean float32 call.  So the
    reference alone meets R1 and R2 on the cases the GPU tests use."""
    case = sc.dense_case(B, T, H, F)
    for b in nc.seg_rows(B):
        for t in nc.seg_steps(T):
            for vname, v in VALUES.items():
                x = nc.dirty(case.x, (b, t, 3 % F), v)
                r64, r32 = sc.stock(case.head, x, torch.float64), sc.stock(case.head, x, torch.float32)
                for r in (r64, r32):
                    if vname == "nan":
                        assert torch.isnan(r[b]).all(), (b, t)
                        assert torch.isfinite(r[[i for i in range(B) if i != b]]).all(), (b, t)
                    else:
                        assert torch.isfinite(r).all(), (b, t, vname)
                others = [i for i in range(B) if i != b]
                assert same_bits(r32[others], case.ref32[others]), (b, t, vname)


def test_twin_with_fmax_relu_is_the_defect():
    """twin_forward(relu='fmax') rectifies as fmaxf does -- NaN becomes 0: the row that holds a NaN feature comes out finite and
    equal to log_softmax(linear.bias) at every step.  With torch's ReLU the row is NaN.  The other rows do not change."""
    case = sc.dense_case(3, 40, 12, 7)
    x = nc.dirty(case.x, (1, 20, 3), float("nan"))
    clean, _ = sc.twin_forward(case.head, case.x)
    good, _ = sc.twin_forward(case.head, x)
    bad, _ = sc.twin_forward(case.head, x, relu="fmax")
    assert torch.isnan(good[1]).all()
    want = torch.log_softmax(case.head.linear.bias.detach().double(), dim=0)
    assert torch.isfinite(bad[1]).all() and torch.equal(bad[1], want.expand(40, 4))
    for r in (good, bad):
        assert torch.equal(r[0], clean[0]) and torch.equal(r[2], clean[2])
    # ... and nc.check_seg_rows, which the GPU tests use, tells the two apart
    nc.check_seg_rows(good, clean, sc.stock(case.head, x, torch.float64), [1], "twin, torch relu")
    with pytest.raises(AssertionError, match="finite values where float64 is not"):
        nc.check_seg_rows(bad, clean, sc.stock(case.head, x, torch.float64), [1], "twin, fmax relu")


@pytest.mark.parametrize("k", [2, 5])
def test_canonical_tile_scale_emulation(k, oracle_mod):
    """canon_land's scale on the CPU: amplitude-1e-6 noise with a NaN at s = 64 k + 126, which only the LAST column of tile k holds.
    With scale 1 for a tile whose energy is not finite (the parent's choice) the tile's other 63 columns are split into mostly
    subnormal f16 halves and fail check_subset against the oracle; with the energy of the finite samples they pass."""
    n, fs = 600, 1000
    x = (synth.noise_windows(1, n, seed=40 + k)[0] * np.float32(1e-6)).astype(np.float32)
    s = 64 * k + 126
    xd = nc.dirty(x, s, np.float32("nan"))
    raw, hd = oracle_mod.features(xd[None], fs, KAISER, BAND, "raw", return_halfdist=True)
    want = nc.window_columns(n, 128, s)
    tile = np.arange(64 * k, 64 * k + 64)
    assert want[tile].sum() == 1 and want[tile[-1]]
    rows = oracle_mod.band(128, fs, *BAND)
    others = tile[:-1]
    good = nc.canon_scale_emulation(xd, KAISER, fs, rows, finite_energy=True)
    m = nc.check_subset(good, raw[0], hd[0], others, 1, what=f"tile {k}, finite-sample energy")
    report(f"canonical tile scale, emulation, tile {k}: finite-sample energy rel {m['rel']:.2e}")
    bad = nc.canon_scale_emulation(xd, KAISER, fs, rows, finite_energy=False)
    with pytest.raises(AssertionError, match="max err|rel L2"):
        nc.check_subset(bad, raw[0], hd[0], others, 1, what=f"tile {k}, scale 1")
    for out in (good, bad):
        assert np.array_equal(nc.columns(nc.nonfinite_set(out), 1), want)


# ==================================================================================================== GPU: FSST
EXTRA = {"the workload's length", "2 groups: below the team kernel", "float16 features", "128 abs", "128 raw, every row", "256 stack",
         "100 points", "unnormalized, columns (16, 64)", "unnormalized, columns (8, 64)", "ragged 128 stack"}
assert EXTRA <= {name for name, _, _ in LAUNCH_CASES}


def _variants(name, n):
    out = [("nan", n // 2, 1.0)]
    if name in EXTRA:
        out += [(v, s, amp) for amp in (1.0, 1e-6) for v in VALUES for s in nc.positions(n)]
    return out


def _row_inputs(case, amp):
    g = torch.Generator().manual_seed(4321)
    if "ragged" in case:
        return [torch.randn(t, generator=g) * amp for t in case["ragged"]]
    return list(torch.randn(3, case["n"], generator=g) * amp)


def _row_call(tf, case, sigs):
    """the row's call on three host signals -> the three signals' outputs as they leave the device (host tensors)"""
    if "ragged" in case:
        out = tf.ragged([s.cuda() for s in sigs])
        res = [out[i].cpu() for i in range(3)]
    else:
        res = list(launch_call(tf, case, [torch.stack(sigs).cuda()]).cpu())
    torch.cuda.synchronize()
    return res


def _fallbacks(tf, case):
    mode = _lib.MODE_STACK_UNNORM if "cols" in case else None
    return int(_lib.lib().hssfsst_plan_fallbacks(tf._plan(0, mode).handle))


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", [(n, c) for n, c, _ in LAUNCH_CASES], ids=[n for n, _, _ in LAUNCH_CASES])
def test_launch_rows(name, case, oracle_mod):
    """Every launch shape at batch 3 with the dirty signal in the middle.  R1: signals 0 and 2 have the bits of the clean call on
    the same plan.  R3 / R2: signal 1 is non-finite exactly where the oracle on the dirty signal is, and passes the parity gate on
    every other column.  A half plan must equal the cast of the float32 plan, which takes the checks."""
    half = case.get("out_dtype", torch.float32) != torch.float32
    tf = launch_transform(case)
    tf32 = launch_transform(dict(case, out_dtype=torch.float32)) if half else tf
    axis = nc.time_axis_of(case)
    clean = {}
    for vname, s, amp in _variants(name, case["ragged"][1] if "ragged" in case else case["n"]):
        sigs = _row_inputs(case, amp)
        if amp not in clean:
            clean[amp] = _row_call(tf, case, sigs)
        sigs[1] = nc.dirty(sigs[1], s, VALUES[vname])
        got = _row_call(tf, case, sigs)
        kernel, fb = launch_kernel(tf, case), _fallbacks(tf, case)
        what = f"{name}: {vname} at {s}, amplitude {amp:g}"
        for i in (0, 2):
            assert same_bits(got[i], clean[amp][i]), f"{what}: signal {i} differs from the clean call"
        if half:
            got32 = _row_call(tf32, case, sigs)
            assert same_as_cast(torch.stack(got), torch.stack(got32), case["out_dtype"]), f"{what}: not the cast of the float32 plan"
            got = got32
        ref, hd = nc.oracle_features(oracle_mod, sigs[1].numpy(), case)
        m = nc.check_r2(got[1].numpy(), ref, hd, axis, what)
        report(f"{what}: {kernel}, fallbacks {fb}, non-finite columns {m['nonfinite']} of {ref.shape[axis]}, "
               f"elsewhere rel {m['rel']:.2e} rel L2 {m['rel_l2']:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("B,rows", [(3, (1,)), (300, (0, 137, 299))])
def test_zscore_paths_give_the_same_bits(B, rows):
    """auto, one_cu and two_launch on 2000-sample signals: identical bits, NaN included, and the clean signals keep the bits of
    the clean call (R1).  The dirty signals are NaN throughout, as the oracle has z-scored STACK."""
    X = torch.from_numpy(synth.pcg_windows(B, 2000, seed=77))
    for vname, v in VALUES.items():
        Xd = X.clone()
        for j, b in enumerate(rows):
            Xd[b, (0, 1000, 1999)[j % 3]] = v
        outs = {}
        for zp in ("auto", "one_cu", "two_launch"):
            tf = FSST(1000, KAISER, truncate_freq=BAND, stack=True)
            tf.set_zpath(zp)
            cl = tf.batch(X.cuda()).cpu()
            outs[zp] = tf.batch(Xd.cuda()).cpu()
            kernel = tf.last_kernel()
            keep = [b for b in range(B) if b not in rows]
            assert same_bits(outs[zp][keep], cl[keep]), (zp, vname)
            assert torch.isnan(outs[zp][list(rows)]).all(), (zp, vname)
            report(f"z-score path {zp}, batch {B}, {vname}: {kernel}, fallbacks {tf.fallbacks()}, {len(rows)} signals NaN throughout")
        for zp in ("one_cu", "two_launch"):
            assert np.array_equal(outs["auto"].numpy(), outs[zp].numpy(), equal_nan=True), (zp, vname)


@pytest.mark.gpu
def test_frames_and_the_corpus_builder():
    """One 5000-sample buffer, frames of 2000 at stride 1000, the dirty sample at 1500: frames 0 and 1 hold it and are NaN
    throughout under STACK, the later frames have the bits of the clean call -- through FSST.frames and through
    build_features(keep_on_device=True)."""
    from heart_sounds_segmentation_amd.corpus import build_features
    x = torch.from_numpy(synth.recording(5000, seed=9))
    tf = FSST(1000, KAISER, truncate_freq=BAND, stack=True)
    starts = [0, 1000, 2000, 3000]
    clean = tf.frames(x.cuda(), starts, 2000).cpu()
    labels = torch.ones(5000, dtype=torch.int64)
    clean_items = build_features([(x, labels)], tf, keep_on_device=True).features.cpu()
    assert clean_items.shape[0] == 3 and same_bits(clean_items, clean[:3])
    for vname, v in VALUES.items():
        xd = nc.dirty(x, 1500, v)
        got = tf.frames(xd.cuda(), starts, 2000).cpu()
        assert torch.isnan(got[:2]).all(), vname
        assert same_bits(got[2:], clean[2:]), vname
        items = build_features([(xd, labels)], tf, keep_on_device=True).features
        assert items.is_cuda
        assert torch.isnan(items[:2]).all() and same_bits(items[2:], clean[2:3]), vname
        report(f"frames, {vname} at 1500: {tf.last_kernel()}, fallbacks {tf.fallbacks()}, frames 0 and 1 NaN throughout")


# ==================================================================================================== GPU: the segmenter
@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,F", DENSE_GPU)
def test_segmenter_dense(B, T, H, F):
    """HipSegmenter, conditioned head: the dirty feature in rows 0, 15, 16 (where they exist) at t = 0, mid, T - 1.  NaN: the row
    is NaN at every step.  +-Inf: within 2e-5 of stock float64, which is finite.  R1 for every other row."""
    case = sc.dense_case(B, T, H, F)
    seg = case.head.hip()
    clean = seg(case.x.cuda()).cpu()
    for vname, v in VALUES.items():
        worst, count = 0.0, 0
        for b in nc.seg_rows(B):
            for t in nc.seg_steps(T):
                x = nc.dirty(case.x, (b, t, 3 % F), v)
                ref = sc.stock(case.head, x, torch.float64)
                got = seg(x.cuda()).cpu()
                if vname == "nan":
                    assert torch.isnan(ref[b]).all()
                m = nc.check_seg_rows(got, clean, ref, [b], f"dense {(B, T, H, F)} {vname} at row {b} step {t}")
                worst, count = max(worst, m["err"]), count + m["nonfinite"]
        report(f"segmenter dense {(B, T, H, F)} {vname}: {count} non-finite log-probs over the calls, worst finite error {worst:.2e}")


@pytest.mark.gpu
@pytest.mark.parametrize("H,F,n", [(12, 7, 7), (240, 44, 18)])
def test_segmenter_ragged(H, F, n):
    """HipSegmenter.ragged: the dirty feature in the recording of length 1, in one of length 17 and in the longest; the reference
    is the float64 module on each recording alone, from its own state row (segmenter_cases.ragged_case)."""
    case = sc.ragged_case(H, F, tuple(LENS18[:n]))
    seg = case.head.hip()
    xs = [x.cuda() for x in case.xs]
    out = seg.ragged(xs, h0=case.h0, c0=case.c0)
    clean = [out[i].cpu() for i in range(n)]
    lens = case.lens
    for i in sorted({lens.index(1), lens.index(17), lens.index(max(lens))}):
        for vname, v in VALUES.items():
            x = nc.dirty(case.xs[i], (lens[i] // 2, 3 % F), v)
            h, c = case.h0[:, i:i + 1].contiguous(), case.c0[:, i:i + 1].contiguous()
            ref = sc.stock(case.head, x[None], torch.float64, h, c)[0]
            out = seg.ragged(xs[:i] + [x.cuda()] + xs[i + 1:], h0=case.h0, c0=case.c0)
            for j in range(n):
                m = nc.check_seg_rows(out[j].cpu()[None], clean[j][None], (ref if j == i else case.ref64[j])[None], [0] if j == i else [],
                                      f"ragged H {H} F {F} {vname} in recording {i} (length {lens[i]}), recording {j}")
                if j == i:
                    report(f"segmenter ragged H {H} F {F} {vname} in the recording of length {lens[i]}: {m['nonfinite']} non-finite, "
                           f"worst finite error {m['err']:.2e}")


@pytest.mark.gpu
def test_segment_with_a_silent_window():
    """segment(tf, head.hip(), X) at the C4 geometry (2000 samples, band (25, 200), hidden 240), B = 3, window 1 all zeros: its
    features are NaN by contract, so its log-probs are NaN, as the stock pipeline has them; rows 0 and 2 have the clean call's bits."""
    torch.manual_seed(5)
    head = SegmenterHead(44, 240, 3).eval()
    X = torch.from_numpy(synth.pcg_windows(3, 2000, seed=21))
    Xd = X.clone()
    Xd[1] = 0.0
    tf = FSST(1000, KAISER, truncate_freq=BAND, stack=True)
    seg = head.hip()
    clean = segment(tf, seg, X.cuda()).cpu()
    got = segment(tf, seg, Xd.cuda()).cpu()
    with torch.no_grad():
        ref = head(tf.batch(Xd.cuda()).cpu())
    assert torch.isnan(ref[1]).all() and torch.isfinite(ref[[0, 2]]).all()
    assert torch.isnan(got[1]).all()
    assert same_bits(got[[0, 2]], clean[[0, 2]])
    report("segment with a silent window: row 1 NaN at all 2000 steps, rows 0 and 2 bit-identical to the clean call")


# ---------------------------------------------------------------------------------------------------- training
def _rows_of(t, kind, offs):
    """a tensor as the list of its rows / recordings: 'steps' (B, T, C) or an arena (sum T, C) with offsets; 'state' (2, B, H)"""
    if kind == "state":
        return [t[:, b] for b in range(t.shape[1])]
    if offs is None:
        return list(t)
    return [t[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def _check_train(where, got, clean, ref, kinds, offs, dirty_row, fwd_names):
    """got / clean / ref: {name: tensor}; kinds: {name: 'steps' | 'state' | 'weight'}.  R1 on the rows of every per-row tensor; R2 on
    the dirty row and on the weight gradients: non-finite where float64 autograd is, and where it is finite within 2e-5 (forward)
    or 1e-4 of the tensor's largest finite reference value (gradients)."""
    figs, wnan = [], [0, 0, 0]
    for name, kind in kinds.items():
        g, c, r = got[name].detach().cpu(), clean[name].detach().cpu(), ref[name].detach().cpu().double()
        fin = torch.isfinite(r)
        scale = float(r[fin].abs().max()) if fin.any() else 0.0
        if kind == "weight":
            parts = [(g, r)]
        else:
            gr, cr, rr = _rows_of(g, kind, offs), _rows_of(c, kind, offs), _rows_of(r, kind, offs)
            for b in range(len(gr)):
                if b != dirty_row:
                    assert same_bits(gr[b], cr[b]), f"{where}: {name} of row {b} differs from the clean run"
            parts = [(gr[dirty_row], rr[dirty_row])]
        for gp, rp in parts:
            nf_g, nf_r = ~torch.isfinite(gp), ~torch.isfinite(rp)
            assert not (nf_r & ~nf_g).any(), f"{where}: {name} has {int((nf_r & ~nf_g).sum())} finite values where float64 autograd is not finite"
            assert not (nf_g & ~nf_r).any(), f"{where}: {name} has {int((nf_g & ~nf_r).sum())} non-finite values where float64 autograd is finite"
            err = float((gp.double() - rp)[~nf_r].abs().max()) if (~nf_r).any() else 0.0
            if name in fwd_names:
                assert err <= nc.SEG_GATE, f"{where}: {name} is {err:.3e} from float64 where that is finite"
            else:
                assert err <= nc.GRAD_GATE * scale, f"{where}: {name} is {err:.3e} from float64, over 1e-4 x {scale:.3e}"
            if kind == "weight":
                wnan[0 if nf_r.all() else 2 if not nf_r.any() else 1] += 1
            else:
                figs.append(f"{name} {int(nf_r.sum())}/{rp.numel()}")
    report(f"{where}: non-finite in the dirty row " + ", ".join(figs) + f"; weight gradients NaN throughout / in part / finite "
           f"{wnan[0]} / {wnan[1]} / {wnan[2]}")


def _layer_run(layer, x, h0, c0, ws, offs, device, dtype):
    """check_layer's loss -- a fixed linear functional of y, hn and cn -- and every gradient, on ``layer`` (nn.LSTM: one call per
    recording when ``offs`` is given; HipBiLSTM: ragged)"""
    layer.zero_grad()
    x, h0, c0 = [t.detach().to(device=device, dtype=dtype).clone().requires_grad_() for t in (x, h0, c0)]
    wy, wh, wc = [w.to(device=device, dtype=dtype) for w in ws]
    if offs is None:
        y, (hn, cn) = layer(x, (h0, c0))
    elif isinstance(layer, HipBiLSTM):
        y, (hn, cn) = layer.ragged(x, offs, (h0, c0))
    else:
        ys, hs, cs = [], [], []
        for i in range(len(offs) - 1):
            yi, (hi, ci) = layer(x[offs[i]:offs[i + 1]][None], (h0[:, i:i + 1].contiguous(), c0[:, i:i + 1].contiguous()))
            ys.append(yi[0]); hs.append(hi); cs.append(ci)
        y, hn, cn = torch.cat(ys), torch.cat(hs, dim=1), torch.cat(cs, dim=1)
    ((y * wy).sum() + (hn * wh).sum() + (cn * wc).sum()).backward()
    out = {"y": y, "hn": hn, "cn": cn, "dx": x.grad, "dh0": h0.grad, "dc0": c0.grad}
    out.update({k: getattr(layer, k).grad for k in consumer._LSTM_KEYS})
    return {k: v.detach().cpu() for k, v in out.items()}


_LAYER_KINDS = dict({"y": "steps", "dx": "steps", "hn": "state", "cn": "state", "dh0": "state", "dc0": "state"},
                    **{k: "weight" for k in consumer._LSTM_KEYS})


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["dense", "ragged"])
def test_training_layer(shape):
    """HipBiLSTM, conditioned, dense (17, 37, 240, 44) and ragged LENS18[:7] at (12, 7), with check_layer's loss: a NaN feature
    in one row, then separately a NaN in one element of that row's dy.  y / hn / cn, dx, dh0 and dc0 of the other rows have the
    bits of the clean run; the dirty row and the weight gradients are NaN where float64 autograd has NaN and within the gates
    where it is finite."""
    if shape == "dense":
        B, T, H, F, offs = 17, 37, 240, 44, None
        xshape, row, at = (B, T, F), 15, (15, T // 2, 3)
    else:
        lens = LENS18[:7]
        B, H, F = len(lens), 12, 7
        offs = [0] + list(np.cumsum(lens))
        xshape, row = (offs[-1], F), lens.index(17)
        at = (offs[row] + 8, 3)
    torch.manual_seed(100 + B + H)
    ref = sc.condition_layer(nn.LSTM(F, H, bidirectional=True, batch_first=True)).double()
    layer = HipBiLSTM(F, H)
    layer.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    layer.cuda()
    x = torch.randn(*xshape)
    h0, c0 = torch.randn(2, B, H), torch.randn(2, B, H)
    ws = [torch.randn(*xshape[:-1], 2 * H), torch.randn(2, B, H), torch.randn(2, B, H)]
    clean = _layer_run(layer, x, h0, c0, ws, offs, "cuda", torch.float32)
    for which in ("feature", "dy"):
        xd, wd = x, list(ws)
        if which == "feature":
            xd = nc.dirty(x, at, float("nan"))
        else:
            wd[0] = nc.dirty(ws[0], at, float("nan"))
        got = _layer_run(layer, xd, h0, c0, wd, offs, "cuda", torch.float32)
        want = _layer_run(ref, xd, h0, c0, wd, offs, "cpu", torch.float64)
        _check_train(f"HipBiLSTM {shape}, NaN in {which}", got, clean, want, _LAYER_KINDS, offs, row, ("y", "hn", "cn"))


def _head_run(head, x, wl, offs, device, dtype):
    head.zero_grad()
    x = x.detach().to(device=device, dtype=dtype).clone().requires_grad_()
    wl = wl.to(device=device, dtype=dtype)
    if offs is None:
        logp = head(x)
    elif isinstance(head, HipSegmenterHead):
        logp = head.ragged([x[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]).data
    else:
        B = len(offs) - 1
        parts = []
        for i in range(B):
            m = SegmenterHead(head.lstm_1.input_size, head.lstm_1.hidden_size, 1, h0=head.h0[:, i:i + 1], c0=head.c0[:, i:i + 1]).to(dtype).eval()
            m.lstm_1, m.lstm_2, m.linear = head.lstm_1, head.lstm_2, head.linear          # (the same parameters: gradients add up)
            parts.append(m(x[offs[i]:offs[i + 1]][None])[0])
        logp = torch.cat(parts)
    (logp * wl).sum().backward()
    out = {"logp": logp, "dx": x.grad}
    out.update({k: p.grad for k, p in head.named_parameters()})
    return {k: v.detach().cpu() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["dense", "ragged"])
def test_training_head(shape):
    """HipSegmenterHead.eval(), conditioned, the same two shapes and the same kind of loss on the log-probs: a NaN feature in one
    row, then a NaN in one element of that row's d log p.  R1 for the log-probs and dx of the other rows, R2 for the dirty row and
    all 18 parameter gradients against float64 autograd; head(x) and head.hip()(x) are NaN in the same rows."""
    if shape == "dense":
        B, T, H, F, offs = 17, 37, 240, 44, None
        xshape, row, at = (B, T, F), 15, (15, T // 2, 3)
    else:
        lens = LENS18[:7]
        B, H, F = len(lens), 12, 7
        offs = [0] + list(np.cumsum(lens))
        xshape, row = (offs[-1], F), lens.index(17)
        at = (offs[row] + 8, 3)
    head = sc.conditioned_head(B, H, F, 7 + B, cls=HipSegmenterHead)
    ref = SegmenterHead(F, H, B, h0=head.h0.double(), c0=head.c0.double()).double().eval()
    ref.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    head.cuda()
    g = torch.Generator().manual_seed(B)
    x, wl = torch.randn(*xshape, generator=g), torch.randn(*xshape[:-1], 4, generator=g)
    kinds = dict({"logp": "steps", "dx": "steps"}, **{k: "weight" for k, _ in ref.named_parameters()})
    clean = _head_run(head, x, wl, offs, "cuda", torch.float32)
    for which in ("feature", "dlogp"):
        xd, wd = x, wl
        if which == "feature":
            xd = nc.dirty(x, at, float("nan"))
        else:
            wd = nc.dirty(wl, at[:-1] + (1,), float("nan"))
        got = _head_run(head, xd, wd, offs, "cuda", torch.float32)
        want = _head_run(ref, xd, wd, offs, "cpu", torch.float64)
        _check_train(f"HipSegmenterHead {shape}, NaN in {which}", got, clean, want, kinds, offs, row, ("logp",))
        seg = head.hip()
        if offs is None:
            inf = seg(xd.cuda()).cpu()
        else:
            out = seg.ragged([xd[offs[i]:offs[i + 1]].cuda() for i in range(B)])
            inf = torch.cat([out[i] for i in range(B)]).cpu()
        nan_rows = lambda t: [bool(torch.isnan(r).any()) for r in _rows_of(t, "steps", offs)]
        assert nan_rows(inf) == nan_rows(got["logp"]) == nan_rows(want["logp"]), (shape, which)
        assert nan_rows(inf) == [(b == row and which == "feature") for b in range(B)]
