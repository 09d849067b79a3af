"""Resample on the device (hssfsst_resample_plan_* / hssfsst_resample_exec, csrc/fourier_resample_gpu.hpp): the batched
Fourier resampler and its wiring into Resample, resample_labels_batch and CorpusBuilder(resample=...).

CPU tests check the C ABI's argument handling and the Python surface without a device; GPU tests (one process) check the
device results against the reference's own outputs (tests/golden/resample.npz), the host helper, and each other."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, synth
from heart_sounds_segmentation_amd.corpus import CorpusBuilder
from heart_sounds_segmentation_amd.framing import frame_batch
from heart_sounds_segmentation_amd.transforms import FSST, Resample
from heart_sounds_segmentation_amd.transforms.resample import resample_labels, resample_labels_batch

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "resample.npz"))
CASES = sorted({k.split("__")[0] for k in GOLD.files if k.endswith("__x")})
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hssfsst.h")
NEW_ENTRY_POINTS = ("hssfsst_resample_plan_create", "hssfsst_resample_plan_destroy", "hssfsst_resample_plan_info",
                    "hssfsst_resample_exec")


def label_tracks(B, T, seed):
    """Label tracks as the corpus has them: cyclic 1 -> 2 -> 3 -> 4 runs of random lengths (int64, (B, T))."""
    rng = np.random.default_rng(seed)
    Y = np.empty((B, T), dtype=np.int64)
    for b in range(B):
        pos, state = 0, int(rng.integers(1, 5))
        while pos < T:
            run = int(rng.integers(20, 400))
            Y[b, pos:pos + run] = state
            pos += run
            state = state % 4 + 1
    return Y


def off_tie(raw32):
    """Where the float32 value the label rule rounds is not within 1e-9 of a .5 tie."""
    r = raw32.astype(np.float64)
    return np.abs(r - np.floor(r) - 0.5) > 1e-9


# ---------------------------------------------------------------------------------------------------- CPU
def test_entry_points_declared_and_bound(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    for name in NEW_ENTRY_POINTS:
        assert f"{name}(" in text, name
        assert getattr(built_lib, name).restype is ctypes.c_int
    assert "HSSFSST_DTYPE_F32" in text and "HSSFSST_DTYPE_F64" in text


def test_bad_sizes_are_einval_without_a_device(built_lib):
    h = ctypes.c_void_p()
    for n, num in [(0, 10), (10, 0), (-1, 5), (5, -3)]:
        assert built_lib.hssfsst_resample_plan_create(ctypes.byref(h), 0, n, num) == _lib.E_INVAL
        assert not h.value
    assert built_lib.hssfsst_resample_plan_create(None, 0, 10, 5) == _lib.E_INVAL
    assert built_lib.hssfsst_resample_plan_create(ctypes.byref(h), -1, 10, 5) == _lib.E_INVAL
    x = (ctypes.c_float * 4)()
    y = (ctypes.c_float * 4)()
    assert built_lib.hssfsst_resample_exec(None, x, 0, 4, 4, None, 0, 1, 0, y, 0, None, 0, None) == _lib.E_INVAL
    assert built_lib.hssfsst_resample_plan_destroy(None) == 0


def test_pickles_without_plans():
    t = Resample(1000, device="cuda")
    t._plans[("sentinel",)] = object()
    u = pickle.loads(pickle.dumps(t))
    assert u.num == 1000 and u.device == "cuda" and u._plans == {}
    assert t._plans                                   # the original keeps its plans


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a visible GPU")
def test_batch_without_device_raises_like_fsst(built_lib):
    X = torch.zeros(2, 2000)
    with pytest.raises(RuntimeError, match="no HIP device"):
        Resample(1000).batch(X)
    with pytest.raises(RuntimeError, match="no HIP device"):
        FSST(1000, synth.kaiser_window(128, 0.5), stack=True).batch(X)
    with pytest.raises(RuntimeError, match="no HIP device"):
        Resample(1000, device="cuda")(torch.zeros(2000))


def test_default_call_stays_on_the_host():
    """Without device= the call is the host helper (works without a GPU) and returns a fresh CPU tensor."""
    y = Resample(7)(torch.arange(5, dtype=torch.float32))
    assert y.shape == (7,) and y.dtype == torch.float32 and y.device.type == "cpu"


# ---------------------------------------------------------------------------------------------------- GPU
DEV = "cuda:0"


def host(x, num):
    return Resample(num)(torch.as_tensor(x), torch.float64).numpy()


@pytest.mark.gpu
def test_golden_cases_through_batch_and_device_call():
    for tag in CASES:
        x, num, ref = GOLD[f"{tag}__x"], int(GOLD[f"{tag}__num"]), GOLD[f"{tag}__y"]
        tol = (1e-12 if ref.dtype == np.float64 else 1e-6) * max(np.abs(ref).max(), 1.0)
        xt = torch.from_numpy(x)
        got_b = Resample(num).batch(xt.reshape(1, -1).to(DEV), torch.float64)[0].cpu().numpy()
        assert np.abs(got_b - ref).max() <= tol, tag
        got_c = Resample(num, device=DEV)(xt, torch.float64)
        assert got_c.device.type == "cpu" and got_c.dtype == torch.float64
        assert np.abs(got_c.numpy() - ref).max() <= tol, tag
        got32 = Resample(num, device=DEV)(xt)
        assert got32.dtype == torch.float32 and np.abs(got32.numpy() - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), tag


SHAPES = [(35500, 8875), (35500, 17751), (2000, 2000), (2, 3), (3, 2), (1024, 1000), (997, 4001),
          (2000, 1000), (4096, 4097), (4099, 2000), (1, 7), (9, 1), (240000, 120000),
          (4096, 4096), (4097, 4096), (35500, 17750)]


@pytest.mark.gpu
def test_against_host_helper_fp64():
    tiers = set()
    for n, num in SHAPES:
        x = np.random.default_rng(n * 7 + num).standard_normal(n)
        t = Resample(num)
        got = t.batch(torch.from_numpy(x).reshape(1, n).to(DEV), torch.float64)[0].cpu().numpy()
        ref = host(x, num)
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1.0)
        assert err <= 1e-12, (n, num, err)
        tiers.add(t.lds_tier(n, 0))
    assert tiers == {True, False}                        # both sides of the LDS / multi-pass boundary


@pytest.mark.gpu
def test_strided_list_and_single_frames_agree_bitwise():
    rec = torch.from_numpy(synth.recording(35500, seed=5))
    t = Resample(1000)
    for dev in (DEV, "cpu"):
        r = rec.to(dev)
        F = frame_batch(r, 1000, 2000)                  # overlapping frames, read in place
        assert F.stride() == (1000, 1)
        strided = t.batch(F, torch.float64)
        assert strided.device == r.device and strided.shape == (F.shape[0], 1000)
        ones = torch.stack([t.batch(F[i:i + 1].contiguous(), torch.float64)[0] for i in range(F.shape[0])])
        assert torch.equal(strided, ones)
        starts = torch.arange(F.shape[0], dtype=torch.int64) * 1000
        listed = t.frames(r, starts.to(dev), 2000, torch.float64)
        assert torch.equal(listed, strided)
        if dev == DEV:
            assert torch.equal(t.frames(r, starts, 2000, torch.float64), strided)    # host starts
    # dtypes: float32 / float64 in and out, results on the input's device
    F = frame_batch(rec.to(DEV), 1000, 2000)
    y64 = t.batch(F.to(torch.float64), torch.float64)
    assert y64.device == F.device
    y32 = t.batch(F, torch.float32)
    assert y32.dtype == torch.float32 and torch.equal(y32, t.batch(F, torch.float64).to(torch.float32))
    assert torch.equal(t.batch(F.to(torch.float64), torch.float32), y64.to(torch.float32))
    # a float32 input is exactly the float64 input of the same values
    assert torch.equal(t.batch(F, torch.float64), t.batch(F.to(torch.float64), torch.float64))
    # the device call equals the batch
    one = Resample(1000, device=DEV)(rec[:2000])
    assert torch.equal(one, y32[0].cpu())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("n,num", [(4097, 1000), (1000, 4097)])
def test_large_tier_frames_agree_bitwise(n, num):
    """The large tier with more than one signal: 3 overlapping frames of one 6 000-sample buffer, read in place at stride 950.
    4097 -> 1000 has the forward convolution (M1 = 16384: two pass launches on each side of the block kernel) above a block and the
    inverse one (M2 = 2048) below; 1000 -> 4097 has them the other way round (M1 = 2048, M2 = 16384)."""
    t = Resample(num)
    assert t.lds_tier(n, 0) is False
    rng = np.random.default_rng(n + num)
    buf = torch.from_numpy(rng.standard_normal(6000)).to(DEV)
    starts = torch.arange(3, dtype=torch.int64) * 950
    F = buf.as_strided((3, n), (950, 1))
    strided = t.batch(F, torch.float64)
    assert strided.shape == (3, num) and strided.dtype == torch.float64
    assert same_bits(t.frames(buf, starts.to(DEV), n, torch.float64), strided)        # device starts
    assert same_bits(t.frames(buf, starts, n, torch.float64), strided)                # host starts
    for i in range(3):
        assert same_bits(t.batch(F[i:i + 1].contiguous(), torch.float64)[0], strided[i]), i
        ref = host(F[i].cpu().numpy(), num)
        assert np.abs(strided[i].cpu().numpy() - ref).max() / max(np.abs(ref).max(), 1.0) <= 1e-12, i
    assert same_bits(t.batch(F, torch.float32), strided.to(torch.float32))
    # the label rule, off the .5 ties
    Y = torch.from_numpy(label_tracks(1, 6000, n)[0])
    lab = t.frames(Y.to(DEV), starts, n, labels=True)
    assert lab.shape == (3, num) and lab.dtype == torch.int64
    assert torch.equal(resample_labels_batch(Y.as_strided((3, n), (950, 1)).to(DEV), t), lab)
    ties = 0
    for i, s in enumerate(starts.tolist()):
        fr = Y[s:s + n]
        ok = off_tie(t(fr).numpy())
        ties += int((~ok).sum())
        assert np.array_equal(lab[i].cpu().numpy()[ok], resample_labels(fr, t).numpy()[ok]), i
    print(f"large-tier label rule: {ties} samples within 1e-9 of a .5 tie")


@pytest.mark.gpu
def test_label_rule_on_device():
    ties = 0
    y = torch.from_numpy(GOLD["labels__y"])
    num = int(GOLD["labels__num"])
    got = resample_labels_batch(y.to(DEV), Resample(num)).cpu().numpy()
    want = resample_labels(y, Resample(num)).numpy()
    raw32 = GOLD["labels__raw"].astype(np.float32)
    ok = off_tie(raw32)
    ties += int((~ok).sum())
    assert np.array_equal(got[ok], want[ok])
    for n, num, seed in [(2000, 1000, 1), (35500, 17750, 2), (4000, 1000, 3), (2000, 2000, 4), (1500, 4001, 5)]:
        Y = torch.from_numpy(label_tracks(3, n, seed))
        t = Resample(num)
        dev_lab = resample_labels_batch(Y.to(DEV), t).cpu().numpy()
        for b in range(Y.shape[0]):
            ref = resample_labels(Y[b], t).numpy()
            raw = t(Y[b]).numpy()                        # the float32 values the rule rounds
            ok = off_tie(raw)
            ties += int((~ok).sum())
            assert np.array_equal(dev_lab[b][ok], ref[ok]), (n, num, b)
        # the device call of a Resample with a device gives the same rule
        assert np.array_equal(resample_labels(Y[0], Resample(num, device=DEV)).numpy(), resample_labels_batch(Y[0], t).numpy())
    print(f"label rule: {ties} samples within 1e-9 of a .5 tie")


@pytest.mark.gpu
def test_corpus_builder_with_resample():
    w = synth.kaiser_window(128, 0.5)
    fsst = FSST(1000, w, truncate_freq=(25, 200), stack=True, device=DEV)
    lens = [35500, 4100, 2000, 12345, 1999]
    recs = []
    for i, T in enumerate(lens):
        x = torch.from_numpy(synth.recording(T, seed=40 + i))
        y = torch.from_numpy(label_tracks(1, T, 60 + i)[0])
        recs.append((x, y))
    rs = Resample(1000)
    b = CorpusBuilder(fsst, device=DEV, windows_per_launch=16, resample=rs)
    items = b.build(recs, keep_on_device=True)
    host_items = CorpusBuilder(fsst, device=DEV, windows_per_launch=16, resample=rs).build(recs)
    kept = [(x, y) for x, y in recs if x.shape[0] >= 2000]
    feats, labs, ties = [], [], 0
    for x, y in kept:
        F = frame_batch(x.to(DEV), 1000, 2000)
        feats.append(fsst.batch(rs.batch(F)))
        for fr in frame_batch(y - 1, 1000, 2000):
            ref = torch.round(Resample(1000)(fr)).type(torch.int64) - 1       # the reference's rule, host Resample
            labs.append((ref.numpy(), off_tie(Resample(1000)(fr).numpy())))
    want = torch.cat(feats)
    assert items.features.shape == (want.shape[0], 1000, want.shape[2])
    assert torch.equal(items.features, want)
    assert torch.equal(host_items.features, want.cpu())
    assert items.labels.shape == (want.shape[0], 1000) and items.labels.dtype == torch.int64
    for i, (ref, ok) in enumerate(labs):
        ties += int((~ok).sum())
        assert np.array_equal(items.labels[i].numpy()[ok], ref[ok]), i
        assert torch.equal(items.labels[i], host_items.labels[i])
    print(f"corpus labels: {ties} samples within 1e-9 of a .5 tie")
    # the builder without resample= is unchanged
    plain = CorpusBuilder(fsst, device=DEV, windows_per_launch=16).build(recs, keep_on_device=True)
    want_plain = torch.cat([fsst.batch(frame_batch(x.to(DEV), 1000, 2000)) for x, _ in kept])
    assert torch.equal(plain.features, want_plain)
    assert torch.equal(plain.labels, torch.cat([frame_batch(y - 1, 1000, 2000) for _, y in kept]))


@pytest.mark.gpu
def test_nan_poisons_every_output_sample():
    for n, num in [(2000, 1000), (35500, 17750)]:
        X = torch.from_numpy(np.random.default_rng(3).standard_normal((2, n)))
        X[0, n // 3] = float("nan")
        got = Resample(num).batch(X.to(DEV), torch.float64).cpu()
        assert torch.isnan(got[0]).all(), (n, num)
        assert not torch.isnan(got[1]).any()
        assert torch.isnan(Resample(num)(X[0], torch.float64)).all()    # as on the host
