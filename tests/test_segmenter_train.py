"""Training on the HIP kernels: the differentiable BiLSTM layer (C ABI hssfsst_bilstm_*, consumer.HipBiLSTM) and the segmenter
built from two of them (consumer.HipSegmenterHead).

The reference of every number is the same module as stock nn.LSTM in float64 on the CPU with its own autograd; weights, h0, c0 and
inputs are copied over.  Forward gate: the segmenter's 2e-5 absolute.  Gradient gate: the project's 1e-4 relative to the
reference's maximum (tests/parity.py: TOL), per tensor: max|g - g64| / max|g64| <= 1e-4.  Stock float32 autograd on the CPU stays
at or under 4.6e-6 by that measure on these shapes, so the gate has a factor 20 over what float32 itself does.  CPU tests check
the ABI, the argument errors that need no device and the index arithmetic of the two new layouts under sanitizers (tests/native/)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch
from torch import nn

from heart_sounds_segmentation_amd import _lib, consumer
from heart_sounds_segmentation_amd.consumer import HipBiLSTM, HipSegmenterHead, SegmenterHead
from tests import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hssfsst.h")
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")
FWD_GATE = 2e-5
GRAD_GATE = parity.TOL
ENTRY_POINTS = {"hssfsst_bilstm_create": 4, "hssfsst_bilstm_destroy": 1, "hssfsst_bilstm_set_weights": 3,
                "hssfsst_bilstm_stash_floats": 4, "hssfsst_bilstm_forward": 11, "hssfsst_bilstm_backward": 12}


def rel(got, want):
    """max|g - g64| / max|g64| (tests/parity.py's measure, per tensor)"""
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def assert_grads(named, where):
    """named: (name, got, float64 reference); prints every figure, then asserts the gate on each"""
    figs = [(n, rel(g, w)) for n, g, w in named]
    print(where, " ".join(f"{n}={v:.2e}" for n, v in figs))
    bad = [(n, v) for n, v in figs if not v <= GRAD_GATE]
    assert not bad, (where, bad)


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_and_loader_declare_the_entry_points(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    assert "#define HSSFSST_VERSION 210" in text
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        fn = getattr(built_lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    i64p = ctypes.POINTER(ctypes.c_int64)
    assert built_lib.hssfsst_bilstm_stash_floats.argtypes == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, i64p]
    assert built_lib.hssfsst_bilstm_forward.argtypes[2:4] == [ctypes.c_int64, ctypes.c_int64]
    assert built_lib.hssfsst_bilstm_backward.argtypes[6:8] == [ctypes.c_int64, ctypes.c_int64]
    assert built_lib.hssfsst_bilstm_create.argtypes[1:] == [ctypes.c_int] * 3


def test_argument_errors_need_no_device(built_lib):
    L, err = built_lib, built_lib.hssfsst_last_error
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below ends before it would be
    plan = ctypes.c_void_p()
    assert L.hssfsst_bilstm_create(None, 0, 44, 240) == _lib.E_INVAL
    assert L.hssfsst_bilstm_create(ctypes.byref(plan), 0, 0, 240) == _lib.E_INVAL
    assert L.hssfsst_bilstm_create(ctypes.byref(plan), 0, 44, -3) == _lib.E_INVAL
    assert L.hssfsst_bilstm_create(ctypes.byref(plan), -1, 44, 240) == _lib.E_INVAL
    assert L.hssfsst_bilstm_create(ctypes.byref(plan), 0, 44, 257) == _lib.E_UNSUPPORTED
    assert b"256" in err() and not plan.value
    assert L.hssfsst_bilstm_destroy(None) == 0
    assert L.hssfsst_bilstm_set_weights(None, (ctypes.c_void_p * 8)(*[4096] * 8), None) == _lib.E_INVAL
    assert L.hssfsst_bilstm_set_weights(fake, None, None) == _lib.E_INVAL
    assert L.hssfsst_bilstm_set_weights(fake, (ctypes.c_void_p * 8)(*([4096] * 5 + [None] + [4096] * 2)), None) == _lib.E_INVAL
    assert b"array 5" in err()
    F, Bk = L.hssfsst_bilstm_forward, L.hssfsst_bilstm_backward
    assert F(None, fake, 2, 3, fake, fake, fake, fake, fake, fake, None) == _lib.E_INVAL
    assert b"plan" in err()
    assert F(fake, fake, 0, 3, fake, fake, fake, fake, fake, fake, None) == _lib.E_INVAL
    assert F(fake, fake, 2, -1, fake, fake, fake, fake, fake, fake, None) == _lib.E_INVAL
    assert F(fake, fake, 2, 1 << 40, fake, fake, fake, fake, fake, fake, None) == _lib.E_INVAL
    assert F(fake, None, 2, 3, fake, fake, fake, fake, fake, fake, None) == _lib.E_INVAL
    assert F(fake, fake, 2, 3, fake, fake, fake, fake, fake, None, None) == _lib.E_INVAL
    assert b"stash" in err()
    assert Bk(None, fake, fake, fake, None, None, 2, 3, fake, fake, fake, None) == _lib.E_INVAL
    assert Bk(fake, None, fake, fake, None, None, 2, 3, fake, fake, fake, None) == _lib.E_INVAL
    assert b"stash" in err()
    assert Bk(fake, fake, fake, fake, None, None, -2, 3, fake, fake, fake, None) == _lib.E_INVAL
    assert Bk(fake, fake, fake, fake, None, None, 2, 0, fake, fake, fake, None) == _lib.E_INVAL
    assert Bk(fake, fake, fake, fake, None, None, 2, 3, None, fake, fake, None) == _lib.E_INVAL
    assert b"dgates" in err()
    # the stash: 2 directions x tiles of 16 rows x steps x 16 unit tiles x (i, f, g, o, c) x 256 floats, whatever the plan
    S = L.hssfsst_bilstm_stash_floats
    n = ctypes.c_int64(-1)
    for B, T in ((1, 1), (16, 7), (17, 37), (50, 2000)):
        assert S(None, B, T, ctypes.byref(n)) == 0
        assert n.value == 16 * ((B + 15) // 16) * T * 2 * 5 * 256, (B, T, n.value)
    assert n.value * 4 == 1_310_720_000                   # the C4 shape: 1.3 GB per layer
    assert S(None, 0, 5, ctypes.byref(n)) == _lib.E_INVAL and n.value == 0
    assert S(None, 5, -1, ctypes.byref(n)) == _lib.E_INVAL
    assert S(None, 5, 5, None) == _lib.E_INVAL


def test_no_cpu_path():
    """Without a GPU the forward raises RuntimeError; with one, a module left on the CPU is refused the same way."""
    layer = HipBiLSTM(3, 5)
    assert [k for k, _ in layer.named_parameters()] == [k for k, _ in nn.LSTM(3, 5, bidirectional=True).named_parameters()]
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer(torch.zeros(1, 2, 3), (torch.zeros(2, 1, 5), torch.zeros(2, 1, 5)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        HipSegmenterHead(3, 5, 1)(torch.zeros(1, 2, 3))


def test_python_surface():
    """The classes live beside SegmenterHead; parameter names, shapes and random draws are nn.LSTM's, so a state_dict moves both
    ways and a seed builds the same weights."""
    assert consumer.HipBiLSTM is HipBiLSTM and issubclass(HipSegmenterHead, SegmenterHead)
    torch.manual_seed(3)
    a = SegmenterHead(7, 5, 2)
    torch.manual_seed(3)
    b = HipSegmenterHead(7, 5, 2)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and len(list(b.parameters())) == 18
    assert all(torch.equal(sa[k], sb[k]) for k in sa) and torch.equal(a.h0, b.h0) and torch.equal(a.c0, b.c0)
    a.load_state_dict(sb)
    b.load_state_dict(sa)
    assert isinstance(b.lstm_1, HipBiLSTM) and isinstance(b.lstm_2, HipBiLSTM) and b.lstm_2.input_size == 10
    b.train()
    with pytest.raises(RuntimeError, match="training mode"):
        b.hip()


def test_layout_functions_under_sanitizers(tmp_path):
    """csrc/segmenter_layout.hpp alone, in a program of its own (tests/native/segmenter_train_layout_check.cpp) built with
    -fsanitize=address,undefined: for H in {1, 5, 16, 240, 256} the stash and backward-stream index functions are in bounds and
    one-to-one, every W_hh element is streamed as exactly one hi and one lo, and the forward tables' index functions equal the
    layout restated there as nested loops."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "segmenter_train_layout_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "segmenter_train_layout_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "segmenter train layout ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU
def twin64(head):
    """the float64 CPU module with stock nn.LSTM on the same weights, h0, c0"""
    H, F, B = head.lstm_1.hidden_size, head.lstm_1.input_size, head.h0.shape[1]
    ref = SegmenterHead(F, H, B, h0=head.h0.detach().cpu().double(), c0=head.c0.detach().cpu().double()).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in head.state_dict().items()})
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,F", [(1, 1, 5, 3), (3, 5, 12, 44), (16, 2, 256, 7), (17, 37, 240, 44), (33, 64, 240, 44)])
def test_layer_gradients(B, T, H, F):
    """HipBiLSTM against nn.LSTM(bidirectional) in float64; x, h0, c0 require grad; the loss is a fixed random linear functional
    of y, hn and cn together, so the seeds d_hn, d_cn are non-zero and dh0 / dc0 are checked."""
    torch.manual_seed(100 + B + T)
    ref = nn.LSTM(F, H, bidirectional=True, batch_first=True).double()
    layer = HipBiLSTM(F, H)
    layer.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    layer.cuda()
    ins = [torch.randn(B, T, F, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64)]
    wy, wh, wc = torch.randn(B, T, 2 * H, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64)
    x64, h64, c64 = [t.clone().requires_grad_() for t in ins]
    y64, (hn64, cn64) = ref(x64, (h64, c64))
    ((y64 * wy).sum() + (hn64 * wh).sum() + (cn64 * wc).sum()).backward()
    x, h0, c0 = [t.float().cuda().requires_grad_() for t in ins]
    y, (hn, cn) = layer(x, (h0, c0))
    ((y * wy.float().cuda()).sum() + (hn * wh.float().cuda()).sum() + (cn * wc.float().cuda()).sum()).backward()
    fwd = [(n, float((g.detach().double().cpu() - w.detach()).abs().max())) for n, g, w in (("y", y, y64), ("hn", hn, hn64), ("cn", cn, cn64))]
    print((B, T, H, F), "forward", fwd)
    assert all(v <= FWD_GATE for _, v in fwd), fwd
    named = [(k, getattr(layer, k).grad, getattr(ref, k).grad) for k in consumer._LSTM_KEYS]
    named += [("dx", x.grad, x64.grad), ("dh0", h0.grad, h64.grad), ("dc0", c0.grad, c64.grad)]
    assert_grads(named, (B, T, H, F))


def model_pair(B, H, F, seed):
    torch.manual_seed(seed)
    head = HipSegmenterHead(F, H, B)
    return head.cuda(), twin64(head)


def loss_and_grads(head, x, labels):
    head.zero_grad()
    x = x.clone().requires_grad_()
    logp = head(x)
    loss = nn.functional.nll_loss(logp.reshape(-1, 4), labels.reshape(-1))
    loss.backward()
    return logp.detach(), x.grad, {k: p.grad.clone() for k, p in head.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,F", [(17, 130, 240, 44), (17, 520, 16, 44), (2, 1030, 16, 44), (2, 4100, 16, 44)])
def test_whole_model_gradients(B, T, H, F):
    """HipSegmenterHead.eval() against the float64 SegmenterHead.eval(), nll_loss on seeded random labels: all 18 parameter
    gradients and dx within the gate, log-probs within 2e-5 of float64 and of head.hip() on the same weights.  520 steps cross
    the forward chunk of 512 steps at two tiles, 1030 cross 1024 at one tile, 4100 the 4096-step launch limit in both passes."""
    head, ref = model_pair(B, H, F, seed=7 + T)
    head.eval(), ref.eval()
    g = torch.Generator().manual_seed(T)
    x64 = torch.randn(B, T, F, generator=g, dtype=torch.float64)
    labels = torch.randint(0, 4, (B, T), generator=g)
    logp64, dx64, grads64 = loss_and_grads(ref, x64, labels)
    logp, dx, grads = loss_and_grads(head, x64.float().cuda(), labels.cuda())
    assert len(grads) == 18
    e64 = float((logp.double().cpu() - logp64).abs().max())
    ehip = float((logp - head.hip()(x64.float().cuda())).abs().max())
    print((B, T, H, F), f"log-probs: vs float64 {e64:.2e}, vs head.hip() {ehip:.2e}")
    assert e64 <= FWD_GATE and ehip <= FWD_GATE
    assert_grads([(k, grads[k], grads64[k]) for k in grads64] + [("dx", dx, dx64)], (B, T, H, F))


@pytest.mark.gpu
def test_determinism():
    head, _ = model_pair(17, 240, 44, seed=5)
    head.eval()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(17, 130, 44, generator=g).cuda()
    labels = torch.randint(0, 4, (17, 130), generator=g).cuda()
    runs = [loss_and_grads(head, x, labels) for _ in range(3)]
    for logp, dx, grads in runs[1:]:
        assert torch.equal(logp, runs[0][0]) and torch.equal(dx, runs[0][1])
        assert all(torch.equal(grads[k], runs[0][2][k]) for k in grads)


@pytest.mark.gpu
def test_weights_follow_the_optimiser():
    """After an in-place update the next forward equals a freshly built module's on the new weights, bit for bit; a backward
    after a repack for other values raises."""
    torch.manual_seed(11)
    layer = HipBiLSTM(7, 12).cuda()
    x = torch.randn(3, 9, 7).cuda()
    st = (torch.randn(2, 3, 12).cuda(), torch.randn(2, 3, 12).cuda())
    y_old, _ = layer(x, st)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(0.25 * torch.randn_like(p))
    y_new, (hn, cn) = layer(x, st)
    fresh = HipBiLSTM(7, 12)
    fresh.load_state_dict(layer.state_dict())
    y_fresh, (hn_f, cn_f) = fresh.cuda()(x, st)
    assert torch.equal(y_new, y_fresh) and torch.equal(hn, hn_f) and torch.equal(cn, cn_f)
    assert not torch.equal(y_new, y_old)
    with pytest.raises(RuntimeError):
        y_old.sum().backward()
    y_new.sum().backward()                               # the latest forward still has its backward
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in layer.parameters())


@pytest.mark.gpu
def test_dropout_and_modes():
    head, _ = model_pair(3, 12, 44, seed=2)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 20, 44, generator=g).cuda()
    labels = torch.randint(0, 4, (3, 20), generator=g).cuda()

    def run(seed):
        torch.manual_seed(seed)
        return loss_and_grads(head, x, labels)
    head.train()
    a, b, c = run(0), run(0), run(1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert not torch.equal(a[0], c[0])
    assert torch.isfinite(a[1]).all() and all(torch.isfinite(v).all() for v in a[2].values())
    head.eval()
    e0, e1 = run(0), run(1)
    assert torch.equal(e0[0], e1[0]) and not torch.equal(e0[0], a[0])


@pytest.mark.gpu
def test_it_trains():
    """Twelve steps of Adam(lr 0.01) with clip_grad_norm_(1.0) in eval() mode on the float64 CPU twin and on HipSegmenterHead:
    every loss within 1e-4 relative of the twin's, the last at most 0.8 x the first (the twin: 1.4640 -> 1.0243)."""
    torch.manual_seed(0)
    base = SegmenterHead(44, 12, 4)
    x = torch.randn(4, 40, 44)
    y = x[:, :, :4].cumsum(1).argmax(2)
    head = HipSegmenterHead(44, 12, 4, h0=base.h0.clone(), c0=base.c0.clone())
    head.load_state_dict(base.state_dict())
    head.cuda()
    ref = twin64(base)

    def fit(m, x, y):
        m.eval()
        opt = torch.optim.Adam(m.parameters(), lr=0.01)
        out = []
        for _ in range(12):
            opt.zero_grad()
            loss = nn.functional.nll_loss(m(x).reshape(-1, 4), y.reshape(-1))
            loss.backward()
            nn.utils.clip_grad_norm_(m.parameters(), 1.0)
            opt.step()
            out.append(float(loss.detach()))
        return out
    want, got = fit(ref, x.double(), y), fit(head, x.cuda(), y.cuda())
    print("twin", [f"{v:.4f}" for v in want], "hip", [f"{v:.4f}" for v in got])
    assert all(abs(g - w) <= 1e-4 * abs(w) for g, w in zip(got, want)), (got, want)
    assert got[-1] <= 0.8 * got[0] and want[-1] <= 0.8 * want[0]
