"""The HIP BiLSTM on heads whose recurrence matters (tests/segmenter_cases.py), and the proof on the CPU that it matters there.

Every other segmenter test builds its weights with nn.LSTM's default initialisation, where a recurrence kernel that lost the lo half
of its split-f16 operands still passes the 2e-5 gate (test_untrained_head_cannot_see_a_lost_operand_half pins that).  The CPU tests
here show, with a float64 twin of the forward pass that can lose that half on purpose, that on the conditioned cases the loss fails
the gate fifty-fold while stock float32 passes it with a factor four to spare; the GPU tests then hold the kernels -- dense, ragged
and training, forward and backward -- to the unchanged gates on those cases, and to a second bound of a small multiple of what
stock float32 itself does on the same case, which a partial loss (one cross term, one K block) cannot meet.

Reference everywhere: stock nn.LSTM modules in float64 on the CPU.  Gates: 2e-5 absolute on log-probabilities and on y / hn / cn,
1e-4 on gradients by max|g - g64| / max|g64| per tensor (tests/test_segmenter_train.py).  With HSS_CONDITIONED_REPORT=<path> the
figures of a run are written there (profiles/segmenter_conditioned.txt)."""
import numpy as np
import pytest
import torch
from torch import nn

from heart_sounds_segmentation_amd import consumer
from heart_sounds_segmentation_amd.consumer import HipBiLSTM, HipSegmenterHead, SegmenterHead
from tests import segmenter_cases as sc
from tests.segmenter_cases import GATE, GRAD_GATE, LENS18, report

# HIP error <= K x the error of stock float32 on the CPU on the same case (and never above the gate).
# Forward, K = 8: the HIP path measured 2 x float32 on the C4 fixture (3.6e-7 against 1.8e-7; fast exp and rcp add a few ulp), a lost
# operand half is >= 150 x by the CPU twin.
K_FWD = 8.0
# Gradients: 8 does not hold for the unmodified kernels.  Measured on an MI355X over the four cases of test_training_layer: HIP
# 7.0e-7 .. 7.6e-6 of a tensor's maximum, stock float32 autograd 1.6e-7 .. 2.3e-6, largest ratio 11.9 (weight_hh_l0 at
# (3, 5, 12, 44): 3.5e-6 against 2.9e-7; dh0 at (17, 37, 240, 44): 5.7e-6 against 5.1e-7 = 11.1).  The term: the backward product
# dh_rec = dG . W_hh runs on split-BF16 operands (csrc/segmenter_train.hpp: seg_put_dg, seg_pack_kernel), 8 + 8 significand bits per
# operand where the forward's split f16 keeps 11 + 11, and drops lo.lo: a floor near 2^-17 = 7.6e-6 of the product's scale that
# does not shrink with the problem, while float32's own error does (few steps, few units).  dh0 IS that product's output and sits at
# 3.7e-6 .. 7.6e-6 in every case; the other gradients see it diluted by the gate derivatives.  So K = 2 x 11.9 = 24.  (A lost bf16
# operand half is 2.3e-3 by the CPU emulation, and one lost cross term 2^-9 of an operand: both beyond the 1e-4 gate itself.)
K_GRAD = 24.0

CPU_CASES = [(17, 333, 240, 44, "randn"), (33, 70, 1, 1, "randn"), (17, 333, 240, 44, "spiked")]
DENSE = [(17, 333, 240, 44, "randn"), (64, 257, 240, 22, "randn"), (3, 40, 12, 7, "randn"), (2, 9, 256, 3, "randn"),
         (33, 70, 1, 1, "randn"), (5, 2000, 16, 44, "randn"), (17, 333, 240, 44, "spiked"), (17, 333, 240, 44, "x30")]
BIG_STATE = [(17, 20, 240, 44), (3, 20, 12, 7)]


def err(got, ref64):
    return float((got.detach().double().cpu() - ref64).abs().max())


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def twins():
    """max |d log p| of the twin with exact / single-f16 / split-f16 recurrent operands against stock float64, and the twin's
    pre-activation record, per CPU case: computed once"""
    cache = {}

    def get(case_args):
        if case_args not in cache:
            case = sc.dense_case(*case_args)
            out = {}
            for terms in (0, 1, 2):
                lp, info = sc.twin_forward(case.head, case.x, terms)
                out[terms] = (err(lp, case.ref64), info)
            cache[case_args] = out
        return cache[case_args]
    return get


@pytest.mark.parametrize("args", CPU_CASES, ids=str)
def test_conditioned_cases_separate_a_lost_operand_half_from_float32(args, twins):
    """What makes the GPU tests below mean something, shown without a GPU.  On each case: the twin with exact operands IS the model
    (1e-12 of stock float64); stock float32 is within gate / 4 of float64 (the case is not chaotic: the reference alone passes with
    room); the twin with single-f16 operands is at least 5 x gate away and the one with split-f16 operands within gate / 4 (losing
    an operand half fails the gate, keeping it passes); at most 0.1 % of the steps have their two best float64 classes within
    2 x gate, so argmax can be compared on the rest."""
    case, t = sc.dense_case(*args), twins(args)
    print(f"{args}: float32 {case.err32:.2e}, twin exact {t[0][0]:.2e}, single f16 {t[1][0]:.2e}, split f16 {t[2][0]:.2e}, "
          f"steps with top-2 margin < {sc.MARGIN:g}: {case.left_out:.5f}")
    assert t[0][0] <= 1e-12
    assert case.err32 <= GATE / 4
    assert t[1][0] >= 5 * GATE
    assert t[2][0] <= GATE / 4
    assert case.left_out <= 1e-3


def test_untrained_head_cannot_see_a_lost_operand_half(twins):
    """The reason this file exists: on nn.LSTM's default initialisation at (17, 333, 240, 44) -- a shape of
    test_shapes_against_float64_lstm -- the twin that drops every lo operand stays UNDER the 2e-5 gate, so no test on such weights
    can tell a recurrence that lost half of its product from a correct one.  (If this ever fails, default-initialised heads have
    become sensitive and the premise of the conditioned cases should be looked at again.)"""
    case = sc.dense_case(17, 333, 240, 44, "randn", False)
    lp, _ = sc.twin_forward(case.head, case.x, 1)
    e = err(lp, case.ref64)
    print(f"untrained (17, 333, 240, 44): single f16 {e:.2e} (gate {GATE:g}), float32 {case.err32:.2e}")
    assert e < GATE


def test_spikes_reach_the_overflow_side_of_expf(twins):
    """Features with +-300 spikes drive layer 1's gate pre-activations beyond +-88.7, where __expf returns inf on one side and 0 on
    the other: the GPU cases on these features run seg_sigmoid / seg_tanh there."""
    l1 = twins(CPU_CASES[2])[0][1]["layers"][0]
    print(f"spiked: layer 1 pre-activations in [{l1['pre_min']:.1f}, {l1['pre_max']:.1f}], {l1['saturated']:.3f} of i/f/o gates saturated")
    assert l1["pre_max"] > sc.EXP_LIMIT and l1["pre_min"] < -sc.EXP_LIMIT


@pytest.mark.parametrize("B,T,H,F", BIG_STATE)
def test_large_initial_state_is_a_fair_case_for_float32(B, T, H, F):
    """h0 cells at +-63 and c0 cells at +-50: stock float32 stays within gate / 4 of float64, and the split-f16 twin too (63 x 1024
    is inside f16), so the gate is a fair demand of the kernels there."""
    case = sc.dense_case(B, T, H, F, "randn", True, True)
    assert float(case.h0.abs().max()) == 63.0 and float(case.c0.abs().max()) == 50.0
    lp, info = sc.twin_forward(case.head, case.x, 2, case.h0, case.c0)
    e2 = err(lp, case.ref64)
    print(f"large state {(B, T, H, F)}: float32 {case.err32:.2e}, split f16 {e2:.2e}, pre-activations in "
          f"[{info['pre_min']:.1f}, {info['pre_max']:.1f}]")
    assert case.err32 <= GATE / 4 and e2 <= GATE / 4 and torch.isfinite(lp).all()


def test_helpers_cover_every_module_class():
    """condition_layer / condition_head act alike on nn.LSTM, HipBiLSTM, SegmenterHead and HipSegmenterHead."""
    torch.manual_seed(4)
    a = nn.LSTM(3, 5, bidirectional=True, batch_first=True)
    b = HipBiLSTM(3, 5)
    b.load_state_dict(a.state_dict())
    before = {k: v.clone() for k, v in a.state_dict().items()}
    sc.condition_layer(a), sc.condition_layer(b)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
        want = before[k] * 2 if k.startswith("weight") else before[k]
        if k.startswith("bias_ih"):
            want = before[k].clone()
            want[5:10] += 1
        assert torch.equal(v, want), k
    h1, h2 = sc.conditioned_head(2, 5, 3, 9), sc.conditioned_head(2, 5, 3, 9, cls=HipSegmenterHead)
    assert all(torch.equal(v, h2.state_dict()[k]) for k, v in h1.state_dict().items()) and torch.equal(h1.h0, h2.h0)
    torch.manual_seed(9)
    plain = SegmenterHead(3, 5, 2)
    assert torch.equal(h1.linear.weight, plain.linear.weight * 8) and torch.equal(h1.linear.bias, plain.linear.bias)


# ---------------------------------------------------------------------------------------------------- GPU
def check_logp(where, got, ref64, mask, err32, k=K_FWD):
    """prints and records the figures, then: finite, within min(k x float32's error, gate), argmax equal wherever float64's margin
    allows a comparison"""
    got = got.detach().double().cpu()
    e = float((got - ref64).abs().max())
    agree = float((got.argmax(-1) == ref64.argmax(-1))[mask].double().mean()) if bool(mask.any()) else 1.0
    left = 1.0 - float(mask.double().mean())
    report(f"{where}: hip {e:.2e}, float32 {err32:.2e}, ratio {e / err32:.2f}, argmax agreement {agree:.6f} on margin >= {sc.MARGIN:g} "
           f"(left out {left:.5f})")
    assert torch.isfinite(got).all(), where
    assert e <= GATE and e <= k * err32, (where, e, err32)
    assert agree == 1.0 and left <= 1e-3, (where, agree, left)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,F,kind", DENSE)
def test_dense_inference(B, T, H, F, kind):
    """conditioned_head(...).hip() against float64: the gate, 8 x float32's own error, finite, every comparable argmax equal.
    'spiked' runs the overflow side of __expf, 'x30' has 79 % of layer 1's gates saturated."""
    case = sc.dense_case(B, T, H, F, kind)
    got = case.head.hip()(case.x.cuda())
    assert got.shape == (B, T, 4)
    if kind == "x30":
        _, info = sc.twin_forward(case.head, case.x, 0)
        report(f"dense {(B, T, H, F)} x30: {info['layers'][0]['saturated']:.3f} of layer 1's i/f/o gates outside [0.02, 0.98]")
    check_logp(f"dense {(B, T, H, F)} {kind}", got, case.ref64, case.mask, case.err32)


@pytest.mark.gpu
@pytest.mark.parametrize("H,F,n,kind", [(240, 44, 18, "randn"), (12, 7, 7, "randn"), (240, 44, 18, "spiked")])
def test_ragged_inference(H, F, n, kind):
    """HipSegmenter.ragged with a conditioned head: every recording against the float64 head run on it alone from its own state
    row.  18 recordings are two tiles, the second nearly empty; with spikes, frozen rows must stay frozen while live neighbours
    saturate."""
    case = sc.ragged_case(H, F, tuple(LENS18[:n]), kind)
    out = case.head.hip().ragged([x.cuda() for x in case.xs], h0=case.h0, c0=case.c0)
    got = torch.cat([out[i] for i in range(n)])
    assert got.shape == (sum(case.lens), 4)
    check_logp(f"ragged H {H} F {F}, {n} recordings, {kind}", got, torch.cat(case.ref64), torch.cat(case.masks), case.err32)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,F", BIG_STATE)
def test_large_initial_state_inference(B, T, H, F):
    """h0 at +-63 (the documented bound is |h0| < 64: h x 1024 must stay inside f16), c0 at +-50, dense and ragged."""
    case = sc.dense_case(B, T, H, F, "randn", True, True)
    seg = case.head.hip()
    got = seg(case.x.cuda(), h0=case.h0.cuda(), c0=case.c0.cuda())
    check_logp(f"large state dense {(B, T, H, F)}", got, case.ref64, case.mask, case.err32)
    lens = tuple(1 + (7 * i) % T for i in range(B))
    rc = sc.ragged_case(H, F, lens, "randn", True)
    out = rc.head.hip().ragged([x.cuda() for x in rc.xs], h0=rc.h0.cuda(), c0=rc.c0.cuda())
    check_logp(f"large state ragged H {H} F {F}, {B} recordings", torch.cat([out[i] for i in range(B)]), torch.cat(rc.ref64),
               torch.cat(rc.masks), rc.err32)


def layer_run(layer, ins, ws, device):
    x, h0, c0 = [t.detach().to(device=device, dtype=ws[0].dtype).clone().requires_grad_() for t in ins]
    y, (hn, cn) = layer(x, (h0, c0))
    ((y * ws[0].to(device)).sum() + (hn * ws[1].to(device)).sum() + (cn * ws[2].to(device)).sum()).backward()
    grads = [(k, getattr(layer, k).grad) for k in consumer._LSTM_KEYS] + [("dx", x.grad), ("dh0", h0.grad), ("dc0", c0.grad)]
    return (y, hn, cn), [(k, g.detach().double().cpu()) for k, g in grads]


def check_layer(where, B, T, H, F, kind, big_state, k_grad):
    """HipBiLSTM against nn.LSTM(bidirectional) in float64, both conditioned; stock float32 autograd on the CPU gives the second
    bound (k_grad None: gradients are held to the gate alone).  The loss is test_layer_gradients': a fixed random linear functional
    of y, hn and cn; x, h0, c0 require grad."""
    torch.manual_seed(100 + B + T)
    ref = sc.condition_layer(nn.LSTM(F, H, bidirectional=True, batch_first=True)).double()
    ref32 = nn.LSTM(F, H, bidirectional=True, batch_first=True)
    ref32.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    layer = HipBiLSTM(F, H)
    layer.load_state_dict(ref32.state_dict())
    layer.cuda()
    x = sc.features((B, T, F), 3 * B + T, kind).double()
    h0, c0 = sc.large_state(B, H, 5 * B + T) if big_state else (torch.randn(2, B, H), torch.randn(2, B, H))
    ins = [x, h0.double(), c0.double()]
    ws64 = [torch.randn(B, T, 2 * H, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64), torch.randn(2, B, H, dtype=torch.float64)]
    ws32 = [w.float() for w in ws64]
    out64, g64 = layer_run(ref, ins, ws64, "cpu")
    out32, g32 = layer_run(ref32, ins, ws32, "cpu")
    out, g = layer_run(layer, ins, ws32, "cuda")
    if kind == "x30":
        _, _, _, info = sc.twin_layer(ref, ins[0], ins[1], ins[2], 0)
        report(f"{where}: {info['saturated']:.3f} of i/f/o gates outside [0.02, 0.98], pre-activations in "
               f"[{info['pre_min']:.1f}, {info['pre_max']:.1f}]")
    fwd = [(n, err(a, w.detach()), err(b, w.detach())) for n, a, b, w in zip(("y", "hn", "cn"), out, out32, out64)]
    report(f"{where} forward: " + ", ".join(f"{n} hip {a:.2e} float32 {b:.2e} ratio {a / b:.2f}" for n, a, b in fwd))

    def rel(got, want):
        return float((got - want).abs().max() / want.abs().max())
    figs = [(n, rel(a, w), rel(b, w)) for (n, a), (_, b), (_, w) in zip(g, g32, g64)]
    report(f"{where} gradients (hip / float32 / ratio): " + ", ".join(f"{n} {a:.2e} / {b:.2e} / {a / b:.1f}" for n, a, b in figs))
    assert all(torch.isfinite(a).all() for _, a in g) and all(torch.isfinite(t).all() for t in out), where
    assert all(a <= GATE and a <= K_FWD * b for _, a, b in fwd), (where, fwd)
    bad = [(n, a, b) for n, a, b in figs if not (a <= GRAD_GATE and (k_grad is None or a <= k_grad * b))]
    assert not bad, (where, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,F,kind", [(17, 37, 240, 44, "randn"), (16, 2, 256, 7, "randn"), (3, 5, 12, 44, "randn"),
                                          (17, 37, 240, 44, "x30")])
def test_training_layer(B, T, H, F, kind):
    """Forward within 2e-5 and 8 x float32; every gradient within 1e-4 and K_GRAD x stock float32 autograd's own figure, finite.
    With features x 30, 79 % of the gates are saturated: the backward's 1 - g factors run at g -> 0 and g -> 1."""
    check_layer(f"layer {(B, T, H, F)} {kind}", B, T, H, F, kind, False, K_GRAD)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,H,F", BIG_STATE)
def test_training_layer_large_initial_state(B, T, H, F):
    """The +-63 h0 / +-50 c0 through HipBiLSTM with gradients, dh0 and dc0 included: forward at 2e-5 and 8 x float32, gradients at
    the 1e-4 gate.  No float32 multiple on these gradients: at (3, 20, 12, 7) float32 autograd is as good as 7.6e-8 .. 4.8e-7 while
    the split-bf16 product keeps its floor (dh0 6.6e-6 against 1.9e-7, ratio 35; see K_GRAD); the figures are recorded."""
    check_layer(f"layer large state {(B, T, H, F)}", B, T, H, F, "randn", True, None)


@pytest.mark.gpu
def test_whole_model():
    """HipSegmenterHead.eval(), conditioned, at (17, 130, 240, 44), nll_loss on seeded labels: the 18 parameter gradients and dx
    within 1e-4, log-probs within 2e-5 of float64 and of head.hip(), as test_whole_model_gradients has it on default weights."""
    B, T, H, F = 17, 130, 240, 44
    head = sc.conditioned_head(B, H, F, 7 + T, cls=HipSegmenterHead)
    ref = SegmenterHead(F, H, B, h0=head.h0.double(), c0=head.c0.double()).double().eval()
    ref.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    ref32 = SegmenterHead(F, H, B, h0=head.h0.clone(), c0=head.c0.clone()).eval()
    ref32.load_state_dict(head.state_dict())
    head.cuda()
    g = torch.Generator().manual_seed(T)
    x64 = torch.randn(B, T, F, generator=g, dtype=torch.float64)
    labels = torch.randint(0, 4, (B, T), generator=g)

    def run(m, x, labels):
        x = x.clone().requires_grad_()
        logp = m(x)
        nn.functional.nll_loss(logp.reshape(-1, 4), labels.reshape(-1)).backward()
        grads = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
        grads["dx"] = x.grad.detach().double().cpu()
        return logp.detach(), grads
    logp64, g64 = run(ref, x64, labels)
    logp32, g32 = run(ref32, x64.float(), labels)
    logp, grads = run(head, x64.float().cuda(), labels.cuda())
    assert len(grads) == 19
    e64, e32 = err(logp, logp64), err(logp32, logp64)
    ehip = float((logp - head.hip()(x64.float().cuda())).abs().max())
    report(f"whole model {(B, T, H, F)} log-probs: hip {e64:.2e}, float32 {e32:.2e}, ratio {e64 / e32:.2f}; against head.hip() {ehip:.2e}")
    figs = [(k, float((grads[k] - w).abs().max() / w.abs().max()), float((g32[k] - w).abs().max() / w.abs().max())) for k, w in g64.items()]
    worst = max(figs, key=lambda f: f[1])
    report(f"whole model gradients: worst {worst[0]} hip {worst[1]:.2e} (float32 {worst[2]:.2e}); largest ratio "
           f"{max(a / b for _, a, b in figs):.1f}; float32's worst {max(b for _, _, b in figs):.2e}")
    print(" ".join(f"{k}={a:.2e}/{b:.2e}" for k, a, b in figs))
    assert e64 <= GATE and ehip <= GATE
    assert all(np.isfinite(a) and a <= GRAD_GATE for _, a, _ in figs), [f for f in figs if not f[1] <= GRAD_GATE]
