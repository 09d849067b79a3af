"""The BiLSTM segmenter as HIP kernels: hssfsst_segmenter_* (C ABI), SegmenterHead.hip() and segment(fsst, head.hip(), X).

References: the two fixtures the reference's own HeartSoundSegmenter produced (tests/golden/segmenter.npz, segmenter_c4.npz) and,
for other shapes, the same module in float64 on the CPU.  The gate on log-probabilities, 2e-5 absolute, is the one the project
applies to the MIOpen path (test_c4_end_to_end_matches_reference_pipeline); a float32 recurrence lands near 2e-7.  CPU tests check
the ABI, the argument errors that need no device and the no-GPU contract."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, synth
from heart_sounds_segmentation_amd.consumer import HipSegmenter, SegmenterHead, segment
from heart_sounds_segmentation_amd.transforms import FSST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hssfsst.h")
GOLD = os.path.join(os.path.dirname(__file__), "golden")
KAISER = synth.kaiser_window(128, 0.5)
BAND = (25, 200)
GATE = 2e-5
NO_GPU = not torch.cuda.is_available()


def small_fixture_head():
    g = np.load(os.path.join(GOLD, "segmenter.npz"))
    sd = {k[4:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd__")}
    head = SegmenterHead(44, 12, 3, h0=torch.from_numpy(g["h0"]), c0=torch.from_numpy(g["c0"]))
    head.load_state_dict(sd, strict=True)
    return g, head.eval()


def seeded_head(B, H, F, seed):
    torch.manual_seed(seed)
    return SegmenterHead(F, H, B).eval()


def host_weights(head):
    """The eighteen float32 host arrays of hssfsst_segmenter_create, kept alive by the returned list."""
    sd = {k: v.detach().float().contiguous() for k, v in head.state_dict().items()}
    keys = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    keys = keys + tuple(k + "_reverse" for k in keys)
    arr = [(ctypes.c_void_p * 8)(*[sd[f"{p}.{k}"].data_ptr() for k in keys]) for p in ("lstm_1", "lstm_2")]
    return sd, arr[0], arr[1], sd["linear.weight"].data_ptr(), sd["linear.bias"].data_ptr()


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_and_loader_declare_the_segmenter_abi(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    for name in ("hssfsst_segmenter_create", "hssfsst_segmenter_exec", "hssfsst_segmenter_destroy", "hssfsst_segmenter_info"):
        assert f"int {name}(" in text
        fn = getattr(built_lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes
    assert len(built_lib.hssfsst_segmenter_exec.argtypes) == 9
    assert re.search(r"typedef struct hssfsst_segmenter hssfsst_segmenter;", text)
    mx = ctypes.c_int()
    assert built_lib.hssfsst_segmenter_info(None, None, None, ctypes.byref(mx), None) == _lib.E_INVAL
    assert mx.value >= 256


def test_create_argument_errors_need_no_device(built_lib):
    head = seeded_head(2, 12, 7, 0)
    keep, l1, l2, lw, lb = host_weights(head)
    plan = ctypes.c_void_p()
    C = built_lib.hssfsst_segmenter_create
    assert C(None, 0, 7, 12, l1, l2, lw, lb) == _lib.E_INVAL
    assert C(ctypes.byref(plan), 0, 0, 12, l1, l2, lw, lb) == _lib.E_INVAL
    assert C(ctypes.byref(plan), 0, 7, 0, l1, l2, lw, lb) == _lib.E_INVAL
    assert C(ctypes.byref(plan), 0, 7, -3, l1, l2, lw, lb) == _lib.E_INVAL
    assert C(ctypes.byref(plan), -1, 7, 12, l1, l2, lw, lb) == _lib.E_INVAL
    assert C(ctypes.byref(plan), 0, 7, 12, None, l2, lw, lb) == _lib.E_INVAL
    assert C(ctypes.byref(plan), 0, 7, 12, l1, l2, None, lb) == _lib.E_INVAL
    assert C(ctypes.byref(plan), 0, 7, 12, l1, l2, lw, None) == _lib.E_INVAL
    holed = (ctypes.c_void_p * 8)(*[l2[i] if i != 5 else None for i in range(8)])
    assert C(ctypes.byref(plan), 0, 7, 12, l1, holed, lw, lb) == _lib.E_INVAL
    assert b"bad argument" in built_lib.hssfsst_last_error()
    mx = ctypes.c_int()
    built_lib.hssfsst_segmenter_info(None, None, None, ctypes.byref(mx), None)
    assert C(ctypes.byref(plan), 0, 7, mx.value + 1, l1, l2, lw, lb) == _lib.E_UNSUPPORTED      # (before the arrays are read)
    assert not plan.value
    assert built_lib.hssfsst_segmenter_exec(None, None, 0, 1, 1, None, None, None, None) == _lib.E_INVAL
    assert built_lib.hssfsst_segmenter_destroy(None) == 0


@pytest.mark.skipif(not NO_GPU, reason="checks the no-device failure mode")
def test_no_gpu_means_runtime_error(built_lib):
    _, head = small_fixture_head()
    with pytest.raises(RuntimeError):
        head.hip()
    keep, l1, l2, lw, lb = host_weights(head)
    plan = ctypes.c_void_p()
    assert built_lib.hssfsst_segmenter_create(ctypes.byref(plan), 0, 44, 12, l1, l2, lw, lb) == _lib.E_NODEVICE and not plan.value
    assert b"no CPU path" in built_lib.hssfsst_last_error()


def test_training_mode_is_refused_before_anything_else(built_lib):
    _, head = small_fixture_head()
    head.train()
    with pytest.raises(RuntimeError, match="training mode"):
        head.hip()


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_small_fixture_matches_the_reference_module():
    """tests/golden/segmenter.npz (hidden 12, batch 3, 40 steps; made by the reference class): max |d log p| < 2e-5."""
    g, head = small_fixture_head()
    seg = head.hip()
    assert isinstance(seg, HipSegmenter)
    y = seg(torch.from_numpy(g["x"]).cuda())
    assert y.shape == (3, 40, 4) and y.dtype == torch.float32 and y.is_cuda and not y.requires_grad
    d = np.abs(y.cpu().numpy() - g["y"]).max()
    print(f"small fixture: max |d log p| = {d:.3e}")
    assert d < GATE


@pytest.mark.gpu
def test_c4_hip_fsst_into_hip_segmenter_matches_reference_pipeline():
    """BASELINE config C4 at its real size (batch 50, hidden 240, 2000 steps), HIP FSST -> HIP segmenter with nothing leaving the
    device, against the log-probabilities of the REFERENCE pipeline (tests/golden/segmenter_c4.npz; weights replayed from the
    seed, checksum asserted).  Gate 2e-5 absolute, as for the MIOpen path (measured on MI355X: 3.6e-7, mean 7.0e-8, every
    argmax decision identical).  Argmax agreement is printed, not gated: 0.106 % of the fixture's steps have their
    two best classes within 4e-5 of each other (an untrained head is near uniform)."""
    g = np.load(os.path.join(GOLD, "segmenter_c4.npz"))
    head = SegmenterHead.seeded_like_reference(int(g["seed"]))
    assert head.checksum() == g["sha256"].tobytes(), "weight replay differs from the reference-made fixture"
    head = head.eval()
    X = torch.from_numpy(synth.pcg_windows(50, 2000, seed=int(g["window_seed"]))).cuda()
    tf = FSST(1000, KAISER, truncate_freq=BAND, stack=True)
    lp = segment(tf, head.hip(), X)
    assert lp.shape == (50, 2000, 4) and lp.is_cuda
    lp = lp.cpu().numpy()
    d = np.abs(lp - g["y"])
    agree = float((lp.argmax(-1) == g["y"].argmax(-1)).mean())
    print(f"C4 HIP segmenter: max |d log p| = {d.max():.3e}, mean = {d.mean():.3e}, argmax agreement = {agree:.6f}")
    assert d.max() < GATE


SHAPES = [(1, 1, 240, 44), (1, 35500, 240, 44), (5, 2000, 16, 44), (17, 333, 240, 44), (16, 2, 240, 44), (64, 257, 240, 22),
          (50, 2000, 240, 44), (3, 40, 12, 7), (2, 9, 256, 3), (33, 70, 1, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,F", SHAPES)
def test_shapes_against_float64_lstm(B, T, H, F):
    """Seeded module and randn features; reference = the same module in float64 on the CPU (nn.LSTM); max |d log p| < 2e-5."""
    head = seeded_head(B, H, F, seed=1000 + B + T + H + F)
    x = torch.randn(B, T, F, generator=torch.Generator().manual_seed(B * 7 + T))
    with torch.no_grad():
        ref = head.double()(x.double()).numpy()
    got = head.float().hip()(x.cuda()).cpu().numpy()
    assert got.shape == (B, T, 4)
    d = np.abs(got - ref).max()
    print(f"shape {(B, T, H, F)}: max |d log p| = {d:.3e}")
    assert np.isfinite(got).all() and d < GATE


@pytest.mark.gpu
def test_batch_invariance_bit_for_bit():
    """Row b of a batch-50 call == the batch-1 call on that row with its own h0 / c0 (rows of the first, a middle and the padded
    last tile); two identical calls give identical bits."""
    head = seeded_head(50, 240, 44, seed=77)
    seg = head.hip()
    x = torch.randn(50, 300, 44, generator=torch.Generator().manual_seed(5)).cuda()
    full = seg(x)
    assert torch.equal(full, seg(x))
    for b in (0, 15, 16, 31, 37, 48, 49):
        one = seg(x[b:b + 1], h0=head.h0[:, b:b + 1], c0=head.c0[:, b:b + 1])
        assert torch.equal(one[0], full[b]), b
    # ... also for a recording that spans several chunks of the time axis
    xl = torch.randn(3, 5000, 44, generator=torch.Generator().manual_seed(6)).cuda()
    h0, c0 = head.h0[:, :3], head.c0[:, :3]
    trio = seg(xl, h0=h0, c0=c0)
    solo = seg(xl[1:2], h0=h0[:, 1:2], c0=c0[:, 1:2])
    assert torch.equal(solo[0], trio[1])


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_half_features_fed_directly(dt):
    """FSST(out_dtype=half) features straight into the segmenter == the float32 path on feats.float(), bit for bit."""
    head = seeded_head(6, 240, 44, seed=3)
    seg = head.hip()
    X = torch.from_numpy(synth.pcg_windows(6, 2000, seed=11)).cuda()
    feats = FSST(1000, KAISER, truncate_freq=BAND, stack=True, out_dtype=dt).batch(X)
    assert feats.dtype == dt
    assert torch.equal(seg(feats), seg(feats.float()))
    tf = FSST(1000, KAISER, truncate_freq=BAND, stack=True, out_dtype=dt)
    assert torch.equal(segment(tf, seg, X), seg(feats.float()))


@pytest.mark.gpu
def test_python_contract():
    g, head = small_fixture_head()
    x = torch.from_numpy(g["x"]).cuda()
    head.train()
    with pytest.raises(RuntimeError):
        head.hip()
    head.eval()
    seg = head.hip()
    want = seg(x)
    with pytest.raises(ValueError):
        seg(x[:2])                                                   # the module's h0 / c0 are for batch 3
    with pytest.raises(ValueError):
        seg(x[:2], h0=head.h0[:, :2])                                # both states or neither
    with pytest.raises(ValueError):
        seg(x[:, :, :40])
    with pytest.raises(ValueError):
        seg(x.double())
    with pytest.raises(ValueError):
        seg(x.cpu())
    two = seg(x[:2], h0=head.h0[:, :2], c0=head.c0[:, :2])
    assert torch.equal(two, want[:2])
    # a plan is a snapshot of the weights: changing the module afterwards does not reach it; a new hip() does
    with torch.no_grad():
        head.linear.bias.add_(1.0)
        head.lstm_1.weight_hh_l0.mul_(0.5)
    assert torch.equal(seg(x), want)
    assert not torch.equal(head.hip()(x), want)
    # the module itself is untouched by all of this: forward still runs nn.LSTM
    with torch.no_grad():
        assert head(torch.from_numpy(g["x"])).shape == (3, 40, 4)
    big = seeded_head(1, 257, 4, seed=0)
    with pytest.raises(RuntimeError, match="not supported"):
        big.hip()
    # a module that lives on the GPU gives a plan there; nothing else changes
    _, head2 = small_fixture_head()
    assert torch.equal(head2.cuda().hip()(x), want)


@pytest.mark.gpu
def test_raw_abi_errors_on_the_device(built_lib):
    _, head = small_fixture_head()
    keep, l1, l2, lw, lb = host_weights(head)
    plan = ctypes.c_void_p()
    assert built_lib.hssfsst_segmenter_create(ctypes.byref(plan), 0, 44, 12, l1, l2, lw, lb) == 0 and plan.value
    F, H, mx, dev = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert built_lib.hssfsst_segmenter_info(plan, ctypes.byref(F), ctypes.byref(H), ctypes.byref(mx), ctypes.byref(dev)) == 0
    assert (F.value, H.value, dev.value) == (44, 12, 0) and mx.value >= 256
    x = torch.zeros(3, 40, 44, device="cuda")
    s = torch.zeros(2, 3, 12, device="cuda")
    out = torch.empty(3, 40, 4, device="cuda")
    E = built_lib.hssfsst_segmenter_exec
    assert E(plan, None, 0, 3, 40, s.data_ptr(), s.data_ptr(), out.data_ptr(), None) == _lib.E_INVAL
    assert E(plan, x.data_ptr(), 0, 0, 40, s.data_ptr(), s.data_ptr(), out.data_ptr(), None) == _lib.E_INVAL
    assert E(plan, x.data_ptr(), 0, 3, 0, s.data_ptr(), s.data_ptr(), out.data_ptr(), None) == _lib.E_INVAL
    assert E(plan, x.data_ptr(), 0, 3, 40, None, s.data_ptr(), out.data_ptr(), None) == _lib.E_INVAL
    assert E(plan, x.data_ptr(), 0, 3, 40, s.data_ptr(), s.data_ptr(), None, None) == _lib.E_INVAL
    assert E(plan, x.data_ptr(), _lib.DTYPE_F64, 3, 40, s.data_ptr(), s.data_ptr(), out.data_ptr(), None) == _lib.E_INVAL
    assert E(plan, x.data_ptr(), 0, 3, 40, s.data_ptr(), s.data_ptr(), out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert built_lib.hssfsst_segmenter_destroy(plan) == 0
