"""Whole recordings of different lengths through the HIP BiLSTM segmenter in one call: hssfsst_segmenter_exec_ragged (C ABI),
HipSegmenter.ragged and segment_recordings(fsst, seg, recordings).

The one rule: recording i of the list gets the bits of the dense call on it alone, seg(x_i[None], h0[:, i:i+1], c0[:, i:i+1])[0] --
forward from its first step, reverse from its own last step, layer 2 seeded at its own ends.  Against float64 (the module on the
CPU, one recording per call) the gate is the project's segmenter gate, 2e-5 absolute on log-probabilities.  CPU tests check the
ABI, the argument errors that need no device and the host-only layout builder under sanitizers (tests/native/)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, consumer, synth
from heart_sounds_segmentation_amd.consumer import HipSegmenter, SegmenterHead, segment_recordings
from heart_sounds_segmentation_amd.transforms import FSST, RaggedFeatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hssfsst.h")
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")
KAISER = synth.kaiser_window(128, 0.5)
BAND = (25, 200)
GATE = 2e-5
# two tiles, the last one padded; length 1, repeated lengths, 16 / 17 around the tile; 1100 crosses two 512-step chunk borders
LENS = [1, 2, 15, 16, 17, 40, 333, 1100, 5, 16, 31, 64, 7, 7, 250, 3, 1, 90, 600]


def seeded_head(B, H, F, seed):
    torch.manual_seed(seed)
    return SegmenterHead(F, H, B).eval()


def host_weights(head):
    sd = {k: v.detach().float().contiguous() for k, v in head.state_dict().items()}
    keys = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    keys = keys + tuple(k + "_reverse" for k in keys)
    arr = [(ctypes.c_void_p * 8)(*[sd[f"{p}.{k}"].data_ptr() for k in keys]) for p in ("lstm_1", "lstm_2")]
    return sd, arr[0], arr[1], sd["linear.weight"].data_ptr(), sd["linear.bias"].data_ptr()


def i64(values):
    return (ctypes.c_int64 * len(values))(*values)


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_and_loader_declare_the_ragged_entry_point(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    assert "int hssfsst_segmenter_exec_ragged(" in text
    fn = built_lib.hssfsst_segmenter_exec_ragged
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10


def test_argument_errors_need_no_device(built_lib):
    E = built_lib.hssfsst_segmenter_exec_ragged
    err = built_lib.hssfsst_last_error
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below ends before the plan is looked at
    assert E(None, None, 0, None, 0, None, None, 1, None, None) == 0                      # count == 0: nothing to do
    assert E(None, fake, 0, i64([0, 5]), 1, fake, fake, 1, fake, None) == _lib.E_INVAL    # NULL plan
    assert b"plan" in err()
    assert E(fake, fake, 0, None, 1, fake, fake, 1, fake, None) == _lib.E_INVAL           # NULL offsets
    assert b"offsets" in err()
    assert E(fake, fake, 0, i64([0, 5]), -1, fake, fake, 1, fake, None) == _lib.E_INVAL   # count = -1
    assert E(None, fake, 0, i64([0, 5, 5]), 2, fake, fake, 2, fake, None) == _lib.E_INVAL
    assert b"index 2" in err()
    assert E(None, fake, 0, i64([0, 7, 3]), 2, fake, fake, 2, fake, None) == _lib.E_INVAL
    assert b"index 2" in err()
    assert E(None, fake, 0, i64([0, 4, 4, 9]), 3, fake, fake, 3, fake, None) == _lib.E_INVAL
    assert b"index 2" in err()
    assert E(None, fake, 0, i64([2, 4]), 1, fake, fake, 1, fake, None) == _lib.E_INVAL    # offsets[0] != 0
    assert E(None, fake, 0, i64([0, 1 << 29]), 1, fake, fake, 1, fake, None) == _lib.E_INVAL
    assert b"recording 0" in err()                                                          # over the dense per-call step limit
    assert E(None, fake, 0, i64([0, 2, 4, 6]), 3, fake, fake, 2, fake, None) == _lib.E_INVAL
    assert b"state_rows" in err()
    assert E(None, fake, _lib.DTYPE_F64, i64([0, 2]), 1, fake, fake, 1, fake, None) == _lib.E_INVAL
    assert b"dtype" in err()


def test_python_surface_exists():
    """Without a GPU head.hip() already raises, so ragged() cannot be reached: the names are the contract here."""
    assert callable(HipSegmenter.ragged) and callable(segment_recordings)
    assert consumer.segment_recordings is segment_recordings


def test_layout_builder_under_sanitizers(tmp_path):
    """csrc/segmenter_layout.hpp alone, in a program of its own (tests/native/segmenter_layout_check.cpp) built with
    -fsanitize=address,undefined: lengths [1], 16 equal, 17, the 19 mixed ones, 1 000 pseudo-random; every recording in exactly one
    slot, padding slots of length 0, non-increasing slot lengths, each tile's walk its maximum, offsets round-trip.
    The launch lists of both execs too: steps covered once and in order, n <= Tc <= kSegMaxChunk, the projection scratch within its
    bound, a launch's tiles those still walking, and the dense list equal to the loop that used to stand inline in the exec."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "segmenter_layout_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "segmenter_layout_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "segmenter layout ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def mixed():
    """H 240, F 44, the 19 recordings of LENS in that (unsorted) order: plan, features, states, and the per-recording dense
    results every test below compares with (computed once, never changed)."""
    head = seeded_head(len(LENS), 240, 44, seed=41)
    seg = head.hip()
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(T, 44, generator=g).cuda() for T in LENS]
    h0, c0 = seg.h0, seg.c0
    want = [seg(x[None], h0=h0[:, i:i + 1], c0=c0[:, i:i + 1])[0] for i, x in enumerate(xs)]
    return seg, xs, h0, c0, want


@pytest.mark.gpu
def test_bit_identity_with_the_per_recording_call(mixed):
    seg, xs, h0, c0, want = mixed
    out = seg.ragged(xs)
    assert isinstance(out, RaggedFeatures) and len(out) == len(LENS) and out.data.shape == (sum(LENS), 4)
    for i in range(len(LENS)):
        assert torch.equal(out[i], want[i]), (i, LENS[i], float((out[i] - want[i]).abs().max()))
    # the same list reversed: other slots, other neighbours, the same bits
    rev = seg.ragged(xs[::-1], h0=h0.flip(1), c0=c0.flip(1))
    for i in range(len(LENS)):
        assert torch.equal(rev[len(LENS) - 1 - i], want[i]), (i, LENS[i])
    again = seg.ragged(xs)
    assert torch.equal(again.data, out.data)


@pytest.mark.gpu
def test_return_to_an_earlier_list():
    """Lists A, A, B, A on one plan: 17 recordings of 1 .. 17 steps and the same reversed -- the same count and total, so the
    tables keep their size; two tiles, one of them nearly all padding.  Every call equals the per-recording dense call."""
    head = seeded_head(17, 12, 7, seed=5)
    seg = head.hip()
    g = torch.Generator().manual_seed(6)
    a = [torch.randn(T, 7, generator=g).cuda() for T in range(1, 18)]
    h0, c0 = seg.h0, seg.c0
    want = [seg(x[None], h0=h0[:, i:i + 1], c0=c0[:, i:i + 1])[0] for i, x in enumerate(a)]
    for step, rev in enumerate((False, False, True, False)):
        out = seg.ragged(a[::-1], h0=h0.flip(1), c0=c0.flip(1)) if rev else seg.ragged(a)
        for i in range(17):
            assert torch.equal(out[16 - i if rev else i], want[i]), (step, i)


@pytest.mark.gpu
def test_equal_lengths_equal_the_dense_call():
    head = seeded_head(18, 240, 44, seed=12)
    seg = head.hip()
    x = torch.randn(18, 70, 44, generator=torch.Generator().manual_seed(3)).cuda()
    out = seg.ragged(list(x))
    assert torch.equal(out.data.view(18, 70, 4), seg(x))


def float64_reference(head, x, h0, c0):
    """The module in float64 on the CPU, one recording (B = 1) from its own state row."""
    with torch.no_grad():
        y, carry = head.lstm_1(x[None].double(), (h0.double().contiguous(), c0.double().contiguous()))
        y, _ = head.lstm_2(torch.relu(y), carry)
        return torch.log_softmax(head.linear(torch.relu(y)), dim=2)[0].numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("H,F", [(12, 7), (240, 44), (256, 3), (1, 1)])
def test_against_float64(H, F):
    lens = [1, 9, 16, 130, 47]
    head = seeded_head(len(lens), H, F, seed=500 + H + F)
    g = torch.Generator().manual_seed(H * 3 + F)
    xs = [torch.randn(T, F, generator=g) for T in lens]
    got = head.hip().ragged([x.cuda() for x in xs])
    h0, c0 = head.h0.clone(), head.c0.clone()
    head = head.double()
    worst = 0.0
    for i, x in enumerate(xs):
        ref = float64_reference(head, x, h0[:, i:i + 1], c0[:, i:i + 1])
        y = got[i].cpu().numpy()
        assert y.shape == (lens[i], 4) and np.isfinite(y).all()
        worst = max(worst, float(np.abs(y - ref).max()))
    print(f"ragged (H, F) = {(H, F)}: max |d log p| = {worst:.3e}")
    assert worst < GATE


@pytest.mark.gpu
def test_max_steps_does_not_change_the_bits(mixed):
    """max_steps = 100: several groups, and 333, 1100, 250 and 600 are longer than the budget (groups of their own)."""
    seg, xs, h0, c0, want = mixed
    out = seg.ragged(xs, max_steps=100)
    assert torch.equal(out.data, torch.cat(want))
    assert torch.equal(out.data, seg.ragged(xs).data)


@pytest.mark.gpu
def test_state_broadcast(mixed):
    seg, xs, h0, c0, want = mixed
    h1, c1 = h0[:, 4:5].contiguous(), c0[:, 4:5].contiguous()
    B = len(xs)
    one = seg.ragged(xs, h0=h1, c0=c1)
    full = seg.ragged(xs, h0=h1.expand(2, B, 240).contiguous(), c0=c1.expand(2, B, 240).contiguous())
    assert torch.equal(one.data, full.data)
    assert torch.equal(one[4], want[4]) and not torch.equal(one[5], want[5])
    assert torch.equal(seg.ragged(xs, h0=h1, c0=c1, max_steps=100).data, one.data)


@pytest.mark.gpu
def test_half_features_and_end_to_end():
    """Synthetic recordings of 700, 2 000 and 1 300 samples: FSST.ragged -> HipSegmenter.ragged with nothing leaving the device."""
    head = seeded_head(3, 240, 44, seed=8)
    seg = head.hip()
    sig = synth.pcg_windows(3, 2000, seed=21)
    recs = [torch.from_numpy(sig[i, :n].copy()).cuda() for i, n in enumerate((700, 2000, 1300))]
    tf = FSST(1000, KAISER, truncate_freq=BAND, stack=True)
    out = segment_recordings(tf, seg, recs)
    assert out.data.is_cuda and out.lengths().tolist() == [700, 2000, 1300]
    for i, rec in enumerate(recs):
        one = seg(tf.batch(rec[None]), h0=seg.h0[:, i:i + 1], c0=seg.c0[:, i:i + 1])[0]
        assert torch.equal(out[i], one), i
    for dt in (torch.float16, torch.bfloat16):
        th = FSST(1000, KAISER, truncate_freq=BAND, stack=True, out_dtype=dt)
        feats = th.ragged(recs)
        assert feats.data.dtype == dt
        half = segment_recordings(th, seg, recs)
        assert torch.equal(half.data, seg.ragged([f.float() for f in feats]).data), dt


@pytest.mark.gpu
def test_contract(mixed, built_lib):
    seg, xs, h0, c0, want = mixed
    tf = FSST(1000, KAISER, truncate_freq=BAND)                                      # raw: complex, frequency-major
    with pytest.raises(ValueError):
        seg.ragged(tf.ragged([torch.randn(300).cuda(), torch.randn(200).cuda()]))
    with pytest.raises(ValueError):
        seg.ragged([x[:, :40] for x in xs])
    with pytest.raises(ValueError):
        seg.ragged([x.cpu() for x in xs])
    with pytest.raises(ValueError):
        seg.ragged([x.int() for x in xs])
    with pytest.raises(ValueError):
        seg.ragged(xs, h0=h0)
    with pytest.raises(ValueError):
        seg.ragged(xs, h0=h0[:, :5], c0=c0[:, :5])
    with pytest.raises(ValueError):
        seg.ragged(xs[:7])                                                           # the module's own state is for 19
    empty = seg.ragged([])
    assert len(empty) == 0 and empty.data.shape == (0, 4)
    feats = RaggedFeatures(torch.cat(xs), torch.tensor(np.concatenate([[0], np.cumsum(LENS)])), 22, False)
    out = seg.ragged(feats)
    assert out.data.device == seg.device and out.data.dtype == torch.float32
    assert torch.equal(out.lengths(), feats.lengths())
    assert out.padded().shape == (len(LENS), max(LENS), 4)
    assert torch.equal(out.data, torch.cat(want))
    # the raw ABI: one offset that does not increase is refused before any device work, and the plan stays usable
    head = seeded_head(3, 12, 7, seed=2)
    keep, l1, l2, lw, lb = host_weights(head)
    plan = ctypes.c_void_p()
    assert built_lib.hssfsst_segmenter_create(ctypes.byref(plan), 0, 7, 12, l1, l2, lw, lb) == 0 and plan.value
    x = torch.randn(12, 7, device="cuda")
    s = torch.zeros(2, 3, 12, device="cuda")
    lp = torch.full((12, 4), float("nan"), device="cuda")
    E = built_lib.hssfsst_segmenter_exec_ragged
    assert E(plan, x.data_ptr(), 0, i64([0, 5, 5, 12]), 3, s.data_ptr(), s.data_ptr(), 3, lp.data_ptr(), None) == _lib.E_INVAL
    assert b"index 2" in built_lib.hssfsst_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(lp).all()
    assert E(plan, x.data_ptr(), 0, i64([0, 5, 6, 12]), 3, s.data_ptr(), s.data_ptr(), 3, lp.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(lp).all()
    assert built_lib.hssfsst_segmenter_destroy(plan) == 0
