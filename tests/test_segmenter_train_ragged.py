"""Training on whole recordings of different lengths in one call: hssfsst_bilstm_{stash_floats,forward,backward}_ragged (C ABI),
HipBiLSTM.ragged and HipSegmenterHead.ragged.

Two rules.  Recording i of the list gets the bits of the dense call on it alone, layer(x_i[None], (h0[:, i:i+1], c0[:, i:i+1])), in y,
hn, cn, dh0, dc0 and in its rows of dgates -- forward from its first step, reverse from its own last one.  And against the same
module as stock nn.LSTM in float64 on the CPU, looped over the recordings with their own states, the gates are those of
tests/test_segmenter_train.py: 2e-5 absolute forward, parity.TOL (1e-4) of each tensor's maximum on gradients (the dense path
measures 4.7e-6).  Weight gradients and dx are one matmul over all arena rows, so against the SUM of the per-recording ones they
are held at the gradient gate, not bit for bit.  Measured on gfx950 (max over the tensors of a case): see
profiles/segmenter_train_ragged_bench.txt.  CPU tests check the ABI, the argument errors that need no device, the host layout
under sanitizers (tests/native/) and the registers and scratch of the six recurrence instantiations in the shipped code object."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

from heart_sounds_segmentation_amd import _lib, consumer
from heart_sounds_segmentation_amd.consumer import HipBiLSTM, HipSegmenterHead, SegmenterHead
from heart_sounds_segmentation_amd.transforms import RaggedFeatures
from tests import parity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hssfsst.h")
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")
FWD_GATE = 2e-5
GRAD_GATE = parity.TOL
ENTRY_POINTS = {"hssfsst_bilstm_stash_floats_ragged": 4, "hssfsst_bilstm_forward_ragged": 11, "hssfsst_bilstm_backward_ragged": 12}
# two tiles, the last one padded; lengths 1 and 2, repeated lengths, 16 / 17 around the tile; 1100 crosses the 1024-step forward
# chunk once one tile is left (tests/test_segmenter_ragged.py)
LENS = [1, 2, 15, 16, 17, 40, 333, 1100, 5, 16, 31, 64, 7, 7, 250, 3, 1, 90, 600]
I64P = ctypes.POINTER(ctypes.c_int64)


def i64(values):
    return (ctypes.c_int64 * len(values))(*values)


def offsets_of(lens):
    return [0] + [int(v) for v in np.cumsum(lens)]


def rel(got, want):
    """max|g - g64| / max|g64| (tests/parity.py's measure, per tensor)"""
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def assert_grads(named, where):
    """named: (name, got, reference); prints every figure, then asserts the gate on each"""
    figs = [(n, rel(g, w)) for n, g, w in named]
    print(where, "gradients", " ".join(f"{n}={v:.2e}" for n, v in figs), f"max={max(v for _, v in figs):.2e}")
    bad = [(n, v) for n, v in figs if not v <= GRAD_GATE]
    assert not bad, (where, bad)


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_and_loader_declare_the_entry_points(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    for name, nargs in ENTRY_POINTS.items():
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        fn = getattr(built_lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
    assert built_lib.hssfsst_bilstm_stash_floats_ragged.argtypes == [ctypes.c_void_p, I64P, ctypes.c_int64, I64P]
    assert built_lib.hssfsst_bilstm_forward_ragged.argtypes[2:4] == [I64P, ctypes.c_int64]
    assert built_lib.hssfsst_bilstm_backward_ragged.argtypes[6:8] == [I64P, ctypes.c_int64]


def test_argument_errors_need_no_device(built_lib):
    """The list is judged before the plan: every call below has a NULL plan and still names what is wrong with the list, in the
    words of hssfsst_segmenter_exec_ragged."""
    L, err = built_lib, built_lib.hssfsst_last_error
    fake = ctypes.c_void_p(4096)                         # never dereferenced: every call below ends before it would be
    n = ctypes.c_int64(-1)

    def S(offsets, count):
        return L.hssfsst_bilstm_stash_floats_ragged(None, offsets, count, ctypes.byref(n))

    def F(offsets, count, plan=None):
        return L.hssfsst_bilstm_forward_ragged(plan, fake, offsets, count, fake, fake, fake, fake, fake, fake, None)

    def B(offsets, count, plan=None):
        return L.hssfsst_bilstm_backward_ragged(plan, fake, fake, fake, None, None, offsets, count, fake, fake, fake, None)

    for name, call in (("bilstm_stash_floats_ragged", S), ("bilstm_forward_ragged", F), ("bilstm_backward_ragged", B)):
        assert call(i64([0, 5]), -1) == _lib.E_INVAL, name                                 # negative count
        assert b"negative" in err() and name.encode() in err()
        assert call(None, 1) == _lib.E_INVAL and b"offsets is NULL" in err(), name         # NULL offsets
        assert call(i64([2, 4]), 1) == _lib.E_INVAL and b"offsets[0] is 2, not 0" in err(), name
        assert call(i64([0, 5, 5]), 2) == _lib.E_INVAL and b"do not increase at index 2" in err(), name
        assert call(i64([0, 7, 3]), 2) == _lib.E_INVAL and b"index 2" in err(), name
        assert call(i64([0, 1 << 29]), 1) == _lib.E_INVAL and b"recording 0 has 536870912 steps" in err(), name
        assert call(None, 0) == 0, name                                                    # count == 0: nothing to do
    assert n.value == 0
    assert F(i64([0, 5]), 1) == _lib.E_INVAL and b"plan is NULL" in err()                  # a good list: now the plan is looked at
    assert B(i64([0, 5]), 1) == _lib.E_INVAL and b"plan is NULL" in err()
    assert L.hssfsst_bilstm_stash_floats_ragged(None, i64([0, 5]), 1, None) == _lib.E_INVAL
    # the stash: 2 directions x (sum over tiles of the tile's longest recording) x 80 KiB, whatever the plan
    assert S(i64(offsets_of(LENS)), len(LENS)) == 0 and n.value == 2 * (1100 + 2) * 20480
    assert S(i64(offsets_of([37] * 17)), 17) == 0
    dense = ctypes.c_int64()
    assert L.hssfsst_bilstm_stash_floats(None, 17, 37, ctypes.byref(dense)) == 0 and n.value == dense.value
    assert S(i64(offsets_of([35500] * 16)), 16) == 0 and n.value * 4 == 5_816_320_000     # the documentation's 5.8 GB


def test_python_surface():
    """HipBiLSTM.ragged and HipSegmenterHead.ragged exist; without a GPU they raise RuntimeError: there is no CPU path."""
    assert callable(HipBiLSTM.ragged) and callable(HipSegmenterHead.ragged)
    assert HipSegmenterHead.ragged is not getattr(SegmenterHead, "ragged", None)
    layer = HipBiLSTM(3, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        layer.ragged(torch.zeros(5, 3), [0, 2, 5], (torch.zeros(2, 2, 5), torch.zeros(2, 2, 5)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        HipSegmenterHead(3, 5, 2).ragged([torch.zeros(2, 3), torch.zeros(3, 3)])


def test_layout_functions_under_sanitizers(tmp_path):
    """csrc/segmenter_layout.hpp alone, in a program of its own (tests/native/segmenter_train_ragged_layout_check.cpp) built with
    -fsanitize=address,undefined: for LENS, one recording, 16 equal, 17 equal and a 4100-step recording beside short ones, the
    ragged stash index is in bounds and one-to-one, stash_floats_ragged is the count, equal lengths give the dense stash_floats,
    and ragged_bwd_chunks covers every (tile, step) once, downwards, with n <= kSegMaxChunk."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "segmenter_train_ragged_layout_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "segmenter_train_ragged_layout_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "segmenter train ragged layout ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_recurrences_in_the_shipped_code_object(built_lib):
    """The library holds four seg_rec_kernel and two seg_bwd_rec_kernel instantiations (dense / ragged x inference / training;
    dense / ragged), none of them with scratch: a recurrence that spills pays for it at every step."""
    try:
        rec = _lib.kernel_resources("seg_rec_kernel")
        bwd = _lib.kernel_resources("seg_bwd_rec_kernel")
    except RuntimeError as e:
        if "not found" in str(e):
            pytest.skip(str(e))
        raise
    for name, v in {**rec, **bwd}.items():
        print(name, v)
    assert len(rec) == 4 and len(bwd) == 2, (sorted(rec), sorted(bwd))
    for name, v in {**rec, **bwd}.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 256, (name, v)


# ---------------------------------------------------------------------------------------------------- GPU
def raw_plan(layer, device):
    weights = [getattr(layer, k) for k in consumer._LSTM_KEYS]
    return layer._sync_plan(device, weights)


def raw_ragged(layer, x, offs, h0, c0, dy, dhn, dcn, poison=False):
    """The three ragged entry points through ctypes: y, hn, cn, dgates (2, sum T, 4H), dh0, dc0.  poison: the stash is NaN before
    the forward call, so whatever the backward reads of it was written by this forward."""
    L, H, B, total = _lib.lib(), layer.hidden_size, len(offs) - 1, offs[-1]
    plan, o = raw_plan(layer, x.device), i64(offs)
    n = ctypes.c_int64()
    assert L.hssfsst_bilstm_stash_floats_ragged(plan, o, B, ctypes.byref(n)) == 0
    stash = torch.full((n.value,), float("nan") if poison else 0.0, device=x.device)
    y = torch.empty(total, 2 * H, device=x.device)
    hn, cn, dh0, dc0 = (torch.empty(2, B, H, device=x.device) for _ in range(4))
    dg = torch.empty(2, total, 4 * H, device=x.device)
    _lib.check(L.hssfsst_bilstm_forward_ragged(plan, x.data_ptr(), o, B, h0.data_ptr(), c0.data_ptr(), y.data_ptr(), hn.data_ptr(),
                                               cn.data_ptr(), stash.data_ptr(), None), "forward_ragged")
    _lib.check(L.hssfsst_bilstm_backward_ragged(plan, stash.data_ptr(), c0.data_ptr(), dy.data_ptr(), dhn.data_ptr(), dcn.data_ptr(), o, B,
                                                dg.data_ptr(), dh0.data_ptr(), dc0.data_ptr(), None), "backward_ragged")
    torch.cuda.synchronize()
    return y, hn, cn, dg, dh0, dc0


def raw_dense_dgates(layer, x, h0, c0, dy, dhn, dcn):
    """dgates (2, T, 4H) of the dense entry points on one recording (batch 1)"""
    L, H, T = _lib.lib(), layer.hidden_size, int(x.shape[0])
    plan = raw_plan(layer, x.device)
    n = ctypes.c_int64()
    assert L.hssfsst_bilstm_stash_floats(plan, 1, T, ctypes.byref(n)) == 0
    stash = torch.empty(n.value, device=x.device)
    y = torch.empty(1, T, 2 * H, device=x.device)
    hn, cn, dh0, dc0 = (torch.empty(2, 1, H, device=x.device) for _ in range(4))
    dg = torch.empty(2, 1, T, 4 * H, device=x.device)
    _lib.check(L.hssfsst_bilstm_forward(plan, x.data_ptr(), 1, T, h0.data_ptr(), c0.data_ptr(), y.data_ptr(), hn.data_ptr(), cn.data_ptr(),
                                        stash.data_ptr(), None), "forward")
    _lib.check(L.hssfsst_bilstm_backward(plan, stash.data_ptr(), c0.data_ptr(), dy.data_ptr(), dhn.data_ptr(), dcn.data_ptr(), 1, T,
                                         dg.data_ptr(), dh0.data_ptr(), dc0.data_ptr(), None), "backward")
    torch.cuda.synchronize()
    return dg[:, 0]


class Mixed:
    """H 240, F 44, the 19 recordings of LENS in that (unsorted) order, each with its own randn h0, c0, and a fixed random linear
    functional of y, hn, cn as the loss (test_layer_gradients' loss).  Holds the per-recording dense results every test below
    compares with (computed once, never changed)."""

    def __init__(self, H=240, F=44, lens=LENS, seed=77):
        torch.manual_seed(seed)
        self.lens, self.offs, B = list(lens), offsets_of(lens), len(lens)
        self.layer = HipBiLSTM(F, H).cuda()
        g = torch.Generator().manual_seed(seed + 1)
        self.xs = [torch.randn(T, F, generator=g).cuda() for T in lens]
        self.h0, self.c0 = torch.randn(2, B, H, generator=g).cuda(), torch.randn(2, B, H, generator=g).cuda()
        self.wys = [torch.randn(T, 2 * H, generator=g).cuda() for T in lens]
        self.wh, self.wc = torch.randn(2, B, H, generator=g).cuda(), torch.randn(2, B, H, generator=g).cuda()
        self.one = []                                    # per recording: y, hn, cn, dx, dh0, dc0, dgates
        self.layer.zero_grad()
        for i, x in enumerate(self.xs):
            x = x.clone().requires_grad_()
            h, c = (t[:, i:i + 1].clone().requires_grad_() for t in (self.h0, self.c0))
            y, (hn, cn) = self.layer(x[None], (h, c))
            ((y[0] * self.wys[i]).sum() + (hn * self.wh[:, i:i + 1]).sum() + (cn * self.wc[:, i:i + 1]).sum()).backward()
            dg = raw_dense_dgates(self.layer, x.detach(), h.detach().contiguous(), c.detach().contiguous(), self.wys[i],
                                  self.wh[:, i:i + 1].contiguous(), self.wc[:, i:i + 1].contiguous())
            self.one.append(dict(y=y[0].detach(), hn=hn[:, 0].detach(), cn=cn[:, 0].detach(), dx=x.grad, dh0=h.grad[:, 0], dc0=c.grad[:, 0], dg=dg))
        self.wgrads = {k: p.grad.clone() for k, p in self.layer.named_parameters()}     # the sum over the recordings
        self.layer.zero_grad()

    def run(self, order):
        """the ragged call on the recordings in `order`; returns per ORIGINAL index the same dict, and the weight gradients"""
        lens = [self.lens[i] for i in order]
        offs = offsets_of(lens)
        idx = torch.tensor(order).cuda()
        x = torch.cat([self.xs[i] for i in order]).requires_grad_()
        h, c = (t[:, idx].clone().requires_grad_() for t in (self.h0, self.c0))
        self.layer.zero_grad()
        y, (hn, cn) = self.layer.ragged(x, offs, (h, c))
        ((y * torch.cat([self.wys[i] for i in order])).sum() + (hn * self.wh[:, idx]).sum() + (cn * self.wc[:, idx]).sum()).backward()
        out = {}
        for k, i in enumerate(order):
            a, b = offs[k], offs[k + 1]
            out[i] = dict(y=y[a:b].detach(), hn=hn[:, k].detach(), cn=cn[:, k].detach(), dx=x.grad[a:b], dh0=h.grad[:, k], dc0=c.grad[:, k])
        return out, {k: p.grad.clone() for k, p in self.layer.named_parameters()}

    def assert_bits(self, got, where):
        for i, want in enumerate(self.one):
            for k in ("y", "hn", "cn", "dh0", "dc0"):
                assert torch.equal(got[i][k], want[k]), (where, i, self.lens[i], k, float((got[i][k] - want[k]).abs().max()))


@pytest.fixture(scope="module")
def mixed():
    return Mixed()


@pytest.mark.gpu
def test_bit_identity_with_the_per_recording_call(mixed):
    m = mixed
    got, wgrads = m.run(list(range(len(LENS))))
    m.assert_bits(got, "in order")
    # through the C ABI: every recording's rows of dgates
    B = len(LENS)
    y, hn, cn, dg, dh0, dc0 = raw_ragged(m.layer, torch.cat(m.xs), m.offs, m.h0, m.c0, torch.cat(m.wys), m.wh, m.wc)
    for i in range(B):
        a, b = m.offs[i], m.offs[i + 1]
        assert torch.equal(dg[:, a:b], m.one[i]["dg"]), (i, LENS[i], float((dg[:, a:b] - m.one[i]["dg"]).abs().max()))
        assert torch.equal(y[a:b], m.one[i]["y"]) and torch.equal(dh0[:, i], m.one[i]["dh0"]) and torch.equal(dc0[:, i], m.one[i]["dc0"])
    # one matmul over all rows against the sum of the per-recording ones
    named = [(k, wgrads[k], m.wgrads[k]) for k in m.wgrads]
    named.append(("dx", torch.cat([got[i]["dx"] for i in range(B)]), torch.cat([o["dx"] for o in m.one])))
    assert_grads(named, "ragged vs the sum of the per-recording calls")


@pytest.mark.gpu
def test_neighbour_independence(mixed):
    """Other slots, other neighbours, the same bits: the list reversed, shuffled, and again after another list on the same plan."""
    m, B = mixed, len(LENS)
    m.assert_bits(m.run(list(range(B))[::-1])[0], "reversed")
    m.assert_bits(m.run([int(i) for i in torch.randperm(B, generator=torch.Generator().manual_seed(4))])[0], "shuffled")
    m.assert_bits(m.run(list(range(B)))[0], "after another list")


@pytest.mark.gpu
def test_equal_lengths_equal_the_dense_call():
    torch.manual_seed(8)
    layer = HipBiLSTM(44, 240).cuda()
    ins = [torch.randn(17, 37, 44).cuda(), torch.randn(2, 17, 240).cuda(), torch.randn(2, 17, 240).cuda()]
    wy, wh, wc = torch.randn(17, 37, 480).cuda(), torch.randn(2, 17, 240).cuda(), torch.randn(2, 17, 240).cuda()
    res = []
    for ragged in (False, True):
        x, h, c = (t.clone().requires_grad_() for t in ins)
        if ragged:
            y, (hn, cn) = layer.ragged(x.reshape(17 * 37, 44), offsets_of([37] * 17), (h, c))
            y = y.reshape(17, 37, 480)
        else:
            y, (hn, cn) = layer(x, (h, c))
        ((y * wy).sum() + (hn * wh).sum() + (cn * wc).sum()).backward()
        res.append((y.detach(), hn.detach(), cn.detach(), h.grad, c.grad))
    for name, a, b in zip(("y", "hn", "cn", "dh0", "dc0"), *res):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


def against_float64(H, F, lens, seed):
    """HipBiLSTM.ragged against nn.LSTM(bidirectional) in float64 on the CPU, looped over the recordings with their own states;
    x, h0, c0 require grad; the loss is a fixed random linear functional of y, hn and cn together."""
    torch.manual_seed(seed)
    B, offs = len(lens), offsets_of(lens)
    ref = nn.LSTM(F, H, bidirectional=True, batch_first=True).double()
    layer = HipBiLSTM(F, H)
    layer.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    layer.cuda()
    ins = [torch.randn(offs[-1], F, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64)]
    wy, wh, wc = torch.randn(offs[-1], 2 * H, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64)
    x64, h64, c64 = [t.clone().requires_grad_() for t in ins]
    ys, hns, cns = [], [], []
    for i in range(B):
        y, (hn, cn) = ref(x64[offs[i]:offs[i + 1]][None], (h64[:, i:i + 1].contiguous(), c64[:, i:i + 1].contiguous()))
        ys.append(y[0]), hns.append(hn), cns.append(cn)
    y64, hn64, cn64 = torch.cat(ys), torch.cat(hns, 1), torch.cat(cns, 1)
    ((y64 * wy).sum() + (hn64 * wh).sum() + (cn64 * wc).sum()).backward()
    x, h0, c0 = [t.float().cuda().requires_grad_() for t in ins]
    y, (hn, cn) = layer.ragged(x, offs, (h0, c0))
    ((y * wy.float().cuda()).sum() + (hn * wh.float().cuda()).sum() + (cn * wc.float().cuda()).sum()).backward()
    fwd = [(n, float((g.detach().double().cpu() - w.detach()).abs().max())) for n, g, w in (("y", y, y64), ("hn", hn, hn64), ("cn", cn, cn64))]
    where = f"ragged (H, F) = {(H, F)}, {B} recordings, {offs[-1]} steps:"
    print(where, "forward", " ".join(f"{n}={v:.2e}" for n, v in fwd), f"max={max(v for _, v in fwd):.2e}")
    assert all(v <= FWD_GATE for _, v in fwd), fwd
    named = [(k, getattr(layer, k).grad, getattr(ref, k).grad) for k in consumer._LSTM_KEYS]
    named += [("dx", x.grad, x64.grad), ("dh0", h0.grad, h64.grad), ("dc0", c0.grad, c64.grad)]
    assert_grads(named, where)


@pytest.mark.gpu
@pytest.mark.parametrize("H,F", [(12, 7), (240, 44), (256, 3), (1, 1)])
def test_against_float64(H, F):
    against_float64(H, F, LENS, seed=300 + H + F)


@pytest.mark.gpu
@pytest.mark.parametrize("lens", [list(range(515, 531)) + [522], [4100, 3, 1030]], ids=["17x515-530", "4100-3-1030"])
def test_chunk_borders(lens):
    """H 16.  17 recordings of 515 .. 530 steps cross the 512-step forward chunk at two live tiles; [4100, 3, 1030] crosses the
    4096-step backward launch and the 1024-step forward chunk."""
    against_float64(16, 7, lens, seed=len(lens))


@pytest.mark.gpu
def test_the_stash_is_written_wherever_it_is_read(mixed):
    m = mixed
    y, hn, cn, dg, dh0, dc0 = raw_ragged(m.layer, torch.cat(m.xs), m.offs, m.h0, m.c0, torch.cat(m.wys), m.wh, m.wc, poison=True)
    assert torch.isfinite(dg).all() and torch.isfinite(dh0).all() and torch.isfinite(dc0).all()
    for i in range(len(LENS)):
        a, b = m.offs[i], m.offs[i + 1]
        assert torch.equal(dg[:, a:b], m.one[i]["dg"]), (i, LENS[i])
        assert torch.equal(dh0[:, i], m.one[i]["dh0"]) and torch.equal(dc0[:, i], m.one[i]["dc0"]), (i, LENS[i])


def twin64(head):
    """the float64 CPU module with stock nn.LSTM on the same weights, h0, c0"""
    H, F, B = head.lstm_1.hidden_size, head.lstm_1.input_size, head.h0.shape[1]
    ref = SegmenterHead(F, H, B, h0=head.h0.detach().cpu().double(), c0=head.c0.detach().cpu().double()).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in head.state_dict().items()})
    return ref


def looped64(ref, xs, h0, c0, margin=None):
    """the float64 module, one recording per call from its own state column (or the one shared column): (sum T, 4) log-probs.
    margin: a list that takes the smallest |value| entering a ReLU, per recording and layer."""
    out = []
    for i, x in enumerate(xs):
        k = i if h0.shape[1] > 1 else 0
        y, carry = ref.lstm_1(x[None], (h0[:, k:k + 1].contiguous(), c0[:, k:k + 1].contiguous()))
        y2, _ = ref.lstm_2(ref.drop(torch.relu(y)), carry)
        if margin is not None:
            margin += [float(y.detach().abs().min()), float(y2.detach().abs().min())]
        y = y2
        out.append(torch.log_softmax(ref.linear(ref.drop(torch.relu(y))), dim=2)[0])
    return torch.cat(out)


@pytest.mark.gpu
def test_whole_model_gradients():
    """HipSegmenterHead.ragged in eval() against the float64 SegmenterHead looped over the recordings, nll_loss over all steps on
    seeded labels: log-probs within 2e-5, all 18 parameter gradients within the gate; broadcast (2, 1, H) states give dh0 / dc0 equal
    to the sum over the recordings.

    The case is chosen on the float64 reference alone.  The model has two ReLUs, and where the reference's value entering one is
    nearer to zero than float32 can resolve, the float32 model may stand on the other side of the kink: that element's gradient
    is then switched on or off as a whole, which no rounding bound covers.  (The dense HipSegmenterHead, one recording per call,
    shows it too: at H 240 on this list, model seed 21, the reverse lstm_1 gradients of both are 5.7e-4 from float64 and within
    2e-6 of each other; the reference's smallest ReLU input there is 4.6e-9.)  So the case must have no ReLU input
    below 1e-6 in the reference -- 16 ulp of a float32 in [0.5, 1), above what the recurrence accumulates on |h| < 1 -- which
    the test asserts.  H 16 on this list has 166 000 ReLU inputs; model seed 22 is the first from 21 on that has none so near
    (the smallest is 1.37e-6), for both state layouts."""
    B, H, F = len(LENS), 16, 44
    torch.manual_seed(22)
    head = HipSegmenterHead(F, H, B).cuda().eval()
    ref = twin64(head).eval()
    g = torch.Generator().manual_seed(22)
    xs64 = [torch.randn(T, F, generator=g, dtype=torch.float64) for T in LENS]
    labels = torch.randint(0, 4, (sum(LENS),), generator=g)
    xs = [x.float().cuda() for x in xs64]
    for rows in (B, 1):
        h64, c64 = (t[:, :rows].clone().requires_grad_() for t in (ref.h0, ref.c0))
        ref.zero_grad()
        margin = []
        logp64 = looped64(ref, xs64, h64, c64, margin)
        assert min(margin) >= 1e-6, ("the reference stands on a ReLU kink: the case is ill-posed", min(margin))
        nn.functional.nll_loss(logp64, labels).backward()
        h0, c0 = (t.detach().float().cuda().requires_grad_() for t in (h64, c64))
        head.zero_grad()
        out = head.ragged(xs, h0=h0, c0=c0)
        assert isinstance(out, RaggedFeatures) and out.data.shape == (sum(LENS), 4) and out.lengths().tolist() == LENS
        nn.functional.nll_loss(out.data, labels.cuda()).backward()
        e64 = float((out.data.detach().double().cpu() - logp64.detach()).abs().max())
        print(f"whole model, state rows {rows}: log-probs vs float64 {e64:.2e}")
        assert e64 <= FWD_GATE
        grads, grads64 = dict(head.named_parameters()), dict(ref.named_parameters())
        assert len(grads) == 18
        named = [(k, grads[k].grad, grads64[k].grad) for k in grads64] + [("dh0", h0.grad, h64.grad), ("dc0", c0.grad, c64.grad)]
        assert h0.grad.shape == (2, rows, H)
        assert_grads(named, f"whole model, state rows {rows}")


@pytest.mark.gpu
def test_dropout_and_training():
    """train(): dropout is active and two calls differ.  Then twelve steps of Adam(lr 0.01) with clip_grad_norm_(1.0) in eval()
    mode on a fixed list, on the float64 CPU twin (one recording per call) and on HipSegmenterHead.ragged: every loss within 1e-4
    relative of the twin's, the last at most 0.8 x the first (the twin: 1.3953 -> 1.0919) -- test_it_trains' tolerances, for the
    same reason.  Eight recordings of 1 .. 40 steps, test_it_trains' scale, all started from the module's one (2, 1, H) state: the
    float64 twin walks them one by one on the CPU, twelve times."""
    lens = [40, 25, 40, 9, 33, 1, 2, 17]
    torch.manual_seed(0)
    base = SegmenterHead(44, 12, 1)
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(T, 44, generator=g) for T in lens]
    labels = torch.cat([x[:, :4].cumsum(0).argmax(1) for x in xs])
    head = HipSegmenterHead(44, 12, 1, h0=base.h0.clone(), c0=base.c0.clone())
    head.load_state_dict(base.state_dict())
    head.cuda()
    ref = twin64(base)
    gx = [x.cuda() for x in xs]
    head.train()
    a, b = head.ragged(gx).data, head.ragged(gx).data
    assert torch.isfinite(a).all() and not torch.equal(a, b)

    def fit(m, forward, y):
        m.eval()
        opt = torch.optim.Adam(m.parameters(), lr=0.01)
        out = []
        for _ in range(12):
            opt.zero_grad()
            loss = nn.functional.nll_loss(forward(), y)
            loss.backward()
            nn.utils.clip_grad_norm_(m.parameters(), 1.0)
            opt.step()
            out.append(float(loss.detach()))
        return out
    xs64 = [x.double() for x in xs]
    want = fit(ref, lambda: looped64(ref, xs64, ref.h0, ref.c0), labels)
    got = fit(head, lambda: head.ragged(gx).data, labels.cuda())
    print("twin", [f"{v:.4f}" for v in want], "hip", [f"{v:.4f}" for v in got])
    assert all(abs(g_ - w) <= 1e-4 * abs(w) for g_, w in zip(got, want)), (got, want)
    assert got[-1] <= 0.8 * got[0] and want[-1] <= 0.8 * want[0]


@pytest.mark.gpu
def test_null_seeds_are_zero_seeds():
    """dhn = dcn = NULL is dhn = dcn = 0, bit for bit in dgates, dh0 and dc0, through the raw ABI of both backwards.  17 recordings
    of 1..3 steps (dense: B 17, T 3) at H 5, F 3: two tiles, the second with 15 padding slots, and 251 padded units -- the smallest
    shape at which the state-init kernel meets a NULL source, a padding slot and a padded unit."""
    L, H, F, B, T = _lib.lib(), 5, 3, 17, 3
    torch.manual_seed(5)
    layer = HipBiLSTM(F, H).cuda()
    plan = raw_plan(layer, torch.device("cuda", torch.cuda.current_device()))
    g = torch.Generator().manual_seed(6)
    lens = [1 + i % 3 for i in range(B)]
    offs, n = offsets_of(lens), ctypes.c_int64()
    h0, c0 = torch.randn(2, B, H, generator=g).cuda(), torch.randn(2, B, H, generator=g).cuda()
    zeros = torch.zeros(2, B, H).cuda()

    def backwards(stash, dy, dg_shape, call):
        out = []
        for seed in (None, zeros.data_ptr()):
            dg, dh0, dc0 = (torch.full(shape, float("nan")).cuda() for shape in (dg_shape, (2, B, H), (2, B, H)))
            _lib.check(call(stash.data_ptr(), c0.data_ptr(), dy.data_ptr(), seed, seed, dg.data_ptr(), dh0.data_ptr(), dc0.data_ptr()), "backward")
            torch.cuda.synchronize()
            out.append((dg, dh0, dc0))
        for a, b, what in zip(out[0], out[1], ("dgates", "dh0", "dc0")):
            assert torch.isfinite(a).all() and torch.equal(a, b), what
        return out[0]

    # ragged
    total, o = offs[-1], i64(offs)
    x, dy = torch.randn(total, F, generator=g).cuda(), torch.randn(total, 2 * H, generator=g).cuda()
    assert L.hssfsst_bilstm_stash_floats_ragged(plan, o, B, ctypes.byref(n)) == 0
    stash, y = torch.zeros(n.value).cuda(), torch.empty(total, 2 * H).cuda()
    hn, cn = torch.empty(2, B, H).cuda(), torch.empty(2, B, H).cuda()
    _lib.check(L.hssfsst_bilstm_forward_ragged(plan, x.data_ptr(), o, B, h0.data_ptr(), c0.data_ptr(), y.data_ptr(), hn.data_ptr(),
                                               cn.data_ptr(), stash.data_ptr(), None), "forward_ragged")
    dg, _, _ = backwards(stash, dy, (2, total, 4 * H),
                         lambda s, c, d, dh, dc, g_, a, b: L.hssfsst_bilstm_backward_ragged(plan, s, c, d, dh, dc, o, B, g_, a, b, None))
    assert dg.abs().max() > 0
    # dense
    x, dy = torch.randn(B, T, F, generator=g).cuda(), torch.randn(B, T, 2 * H, generator=g).cuda()
    assert L.hssfsst_bilstm_stash_floats(plan, B, T, ctypes.byref(n)) == 0
    stash, y = torch.zeros(n.value).cuda(), torch.empty(B, T, 2 * H).cuda()
    _lib.check(L.hssfsst_bilstm_forward(plan, x.data_ptr(), B, T, h0.data_ptr(), c0.data_ptr(), y.data_ptr(), hn.data_ptr(), cn.data_ptr(),
                                        stash.data_ptr(), None), "forward")
    dg, _, _ = backwards(stash, dy, (2, B, T, 4 * H),
                         lambda s, c, d, dh, dc, g_, a, b: L.hssfsst_bilstm_backward(plan, s, c, d, dh, dc, B, T, g_, a, b, None))
    assert dg.abs().max() > 0


@pytest.mark.gpu
def test_determinism_and_contract(mixed):
    m, B = mixed, len(LENS)
    order = list(range(B))
    (r1, w1), (r2, w2) = m.run(order), m.run(order)
    for i in range(B):
        assert all(torch.equal(r1[i][k], r2[i][k]) for k in r1[i]), i
    assert all(torch.equal(w1[k], w2[k]) for k in w1)
    # a backward after a repack for other values raises
    torch.manual_seed(11)
    layer = HipBiLSTM(7, 12).cuda()
    x, st = torch.randn(9, 7).cuda(), (torch.randn(2, 2, 12).cuda(), torch.randn(2, 2, 12).cuda())
    y_old, _ = layer.ragged(x, [0, 4, 9], st)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(0.25 * torch.randn_like(p))
    y_new, _ = layer.ragged(x, torch.tensor([0, 4, 9]), st)
    assert not torch.equal(y_new, y_old)
    with pytest.raises(RuntimeError):
        y_old.sum().backward()
    y_new.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in layer.parameters())
    # an empty list
    y, (hn, cn) = layer.ragged(torch.empty(0, 7).cuda(), [0], (torch.empty(2, 0, 12).cuda(), torch.empty(2, 0, 12).cuda()))
    assert y.shape == (0, 24) and hn.shape == (2, 0, 12)
    head = HipSegmenterHead(44, 12, B).cuda().eval()
    empty = head.ragged([])
    assert len(empty) == 0 and empty.data.shape == (0, 4)
    # what is refused
    xs = [x[:, :44] for x in m.xs]
    with pytest.raises(ValueError):
        head.ragged(RaggedFeatures(torch.zeros(22 * 500, dtype=torch.complex64).cuda(), torch.tensor([0, 300, 500]), 22, True))
    with pytest.raises(ValueError):
        head.ragged([x[:, :40] for x in xs])
    with pytest.raises(ValueError):
        head.ragged([x.cpu() for x in xs])
    with pytest.raises(ValueError):
        head.ragged(xs, h0=head.h0[:, :5], c0=head.c0[:, :5])
    with pytest.raises(ValueError):
        head.ragged(xs, h0=head.h0)
    with pytest.raises(ValueError):
        head.ragged(xs[:7])                                                              # the module's own state is for 19
    with pytest.raises(ValueError):
        m.layer.ragged(torch.cat(m.xs), m.offs, (m.h0[:, :5], m.c0[:, :5]))
    # half features: one cast, the float32 call's bits
    full = head.ragged(xs)
    assert torch.equal(head.ragged([x.half() for x in xs]).data, head.ragged([x.half().float() for x in xs]).data)
    assert torch.equal(head.ragged(RaggedFeatures(torch.cat(xs), torch.tensor(m.offs), 22, False)).data, full.data)
