"""Segmenter heads whose recurrence matters, and a float64 twin that can lose what the kernels must keep.

nn.LSTM's default initialisation at hidden 240 leaves W_hh at U(+-0.065), every gate near 1/2 and the head near uniform: there the
recurrent product h . W_hh^T hardly reaches a log-probability, and a recurrence kernel that dropped the lo half of its split-f16
operands would still pass the 2e-5 gate (tests/test_segmenter_conditioned.py measures exactly that on the CPU).  This module holds

  condition_layer / condition_head / conditioned_head   a seeded module pushed to where the recurrence carries the result and float32
                                                        still follows float64 (W_hh x 2 is contractive; x 2.5 is not any more);
  twin_layer / twin_forward                             the forward pass written out step by step in float64, the recurrent operands
                                                        exact, split f16 (hi + lo, as csrc/segmenter_lstm.hpp: seg_put_h and
                                                        segmenter.hip: seg_upload_layer round them) or single f16 (the lo halves lost);
  features / large_state                                inputs: randn, randn with +-300 spikes, randn x 30; states up to +-63;
  dense_case / ragged_case                              the cases of the tests with their float64 and float32 CPU results, each
                                                        computed once and never changed;
  report                                                the figures of a run, for profiles/segmenter_conditioned.txt.

A helper module, not a conftest: the tests import it."""
import functools
import math
import os

import torch
from torch import nn

from heart_sounds_segmentation_amd.consumer import SegmenterHead

GATE = 2e-5                 # the project's gate on log-probabilities and on y / hn / cn
GRAD_GATE = 1e-4            # ... and on gradients: max|g - g64| / max|g64| per tensor (tests/parity.py: TOL)
MARGIN = 2 * GATE           # argmax is compared where float64's two best classes are at least this far apart
H_SCALE = 1024.0            # kSegHScale: h x 2^10 before the f16 split
EXP_LIMIT = 88.7            # |x| beyond which __expf(x) has left float32
SPIKE = 300.0
# the ragged list of the issue: 18 recordings = two tiles of 16 slots, the second nearly empty; 1, 15 / 16 / 17 around the tile
LENS18 = [1, 2, 15, 16, 17, 40, 333, 64, 3, 100, 257, 31, 33, 5, 129, 7, 48, 200]
_SUFFIXES = ("", "_reverse")


# ------------------------------------------------------------------------------------------------ conditioning
def condition_layer(lstm):
    """In place, on an nn.LSTM or a HipBiLSTM: W_hh x 2, W_ih x 2, +1 on the forget gate's slice of bias_ih, both directions."""
    H = lstm.hidden_size
    with torch.no_grad():
        for s in _SUFFIXES:
            getattr(lstm, "weight_hh_l0" + s).mul_(2.0)
            getattr(lstm, "weight_ih_l0" + s).mul_(2.0)
            getattr(lstm, "bias_ih_l0" + s)[H:2 * H].add_(1.0)
    return lstm


def condition_head(head):
    """In place, on a SegmenterHead or a HipSegmenterHead: both layers as condition_layer, linear.weight x 8."""
    condition_layer(head.lstm_1)
    condition_layer(head.lstm_2)
    with torch.no_grad():
        head.linear.weight.mul_(8.0)
    return head


def conditioned_head(B, H, F, seed, cls=SegmenterHead, h0=None, c0=None):
    torch.manual_seed(seed)
    return condition_head(cls(F, H, B, h0=h0, c0=c0).eval())


def seed_of(B, T, H, F):
    return 1000 + B + T + H + F


# ------------------------------------------------------------------------------------------------ inputs
def features(shape, seed, kind="randn"):
    """float32 features of `shape` (..., T, F): 'randn'; 'spiked' = randn with +-300 (seeded signs) on [..., ::7, ::5], which
    drives layer 1's pre-activations past +-88.7; 'x30' = randn x 30, which saturates most gates."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g)
    if kind == "spiked":
        sub = x[..., ::7, ::5]
        sign = torch.randint(0, 2, sub.shape, generator=g).float() * 2.0 - 1.0
        x[..., ::7, ::5] = SPIKE * sign
    elif kind == "x30":
        x = x * 30.0
    elif kind != "randn":
        raise ValueError(kind)
    return x


def large_state(B, H, seed):
    """(h0, c0) of shape (2, B, H): randn, with h0 cells at +-63 (x 1024 = 64 512, just inside f16) and c0 cells at +-50, in both
    directions, in the first and the last row of the first tile, the first row of the second one and the last row of the batch, at
    the first, a middle and the last unit."""
    g = torch.Generator().manual_seed(seed)
    h0, c0 = torch.randn(2, B, H, generator=g), torch.randn(2, B, H, generator=g)
    rows = sorted({0, min(15, B - 1), min(16, B - 1), B - 1})
    units = sorted({0, H // 2, H - 1})
    n = 0
    for d in range(2):
        for b in rows:
            for u in units:
                sign = 1.0 if n % 2 == 0 else -1.0
                h0[d, b, u] = 63.0 * sign
                c0[d, b, (u + 1) % H] = -50.0 * sign
                n += 1
    return h0, c0


# ------------------------------------------------------------------------------------------------ the float64 twin
def _f16(t):
    return t.to(torch.float16).to(torch.float64)


def _split16(t):
    hi = _f16(t)
    return hi, _f16(t - hi)


def _relu(t, relu):
    """'torch': torch.relu, which keeps a NaN; 'fmax': max(x, 0) as C's fmaxf has it, which turns a NaN into 0"""
    if relu == "torch":
        return torch.relu(t)
    if relu != "fmax":
        raise ValueError(relu)
    return torch.where(t > 0.0, t, torch.zeros_like(t))


def twin_layer(lstm, x, h0, c0, terms=0, relu=None):
    """One bidirectional layer in float64, step by step.  lstm: anything with nn.LSTM's parameter names; x (B, T, F), h0 / c0
    (2, B, H).  terms: 0 = exact recurrent product; 2 = the kernels' operands, h x 2^10 and W_hh x wscale (the power of two that
    puts the layer's largest |W_hh| in [2^12, 2^13)) each split into f16 hi + lo, products hi.hi + hi.lo + lo.hi; 1 = hi.hi only.
    relu: None = x as it is; 'torch' / 'fmax' = x rectified on load, as seg_proj_kernel reads layer 2's input (see _relu).
    Returns y (B, T, 2H), hn, cn (2, B, H) and {'pre_min', 'pre_max': extremes of the gate pre-activations, 'saturated': share of
    i / f / o gates outside [0.02, 0.98]}."""
    H = lstm.hidden_size
    x, h0, c0 = x.double(), h0.double(), c0.double()
    if relu is not None:
        x = _relu(x, relu)
    B, T = x.shape[0], x.shape[1]
    W = [{k: getattr(lstm, f"{k}_l0{s}").detach().double().cpu() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
         for s in _SUFFIXES]
    wmax = max(float(w["weight_hh"].abs().max()) for w in W)
    wscale = 1.0
    if wmax > 0.0 and math.isfinite(wmax):
        wscale = math.ldexp(1.0, 13 - math.frexp(wmax)[1])
    inv_scale = 1.0 / (wscale * H_SCALE)
    y = torch.empty(B, T, 2 * H, dtype=torch.float64)
    hn, cn = torch.empty(2, B, H, dtype=torch.float64), torch.empty(2, B, H, dtype=torch.float64)
    lo, hi, sat, cnt = math.inf, -math.inf, 0, 0
    for d in range(2):
        w = W[d]
        pre = x @ w["weight_ih"].t() + (w["bias_ih"] + w["bias_hh"])
        whh_t = w["weight_hh"].t().contiguous()
        if terms:
            w_hi, w_lo = _split16(whh_t * wscale)
        h, c = h0[d], c0[d]
        acts = torch.empty_like(pre)
        for s in range(T):
            t = T - 1 - s if d else s
            if terms == 0:
                rec = h @ whh_t
            else:
                h_hi, h_lo = _split16(h * H_SCALE)
                rec = h_hi @ w_hi
                if terms == 2:
                    rec = rec + h_hi @ w_lo + h_lo @ w_hi
                rec = rec * inv_scale
            a = pre[:, t] + rec
            acts[:, t] = a
            i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            y[:, t, d * H:(d + 1) * H] = h
        hn[d], cn[d] = h, c
        lo, hi = min(lo, float(acts.min())), max(hi, float(acts.max()))
        ifo = torch.sigmoid(torch.cat((acts[..., :2 * H], acts[..., 3 * H:]), dim=-1))
        sat += int(((ifo < 0.02) | (ifo > 0.98)).sum())
        cnt += ifo.numel()
    return y, hn, cn, {"pre_min": lo, "pre_max": hi, "saturated": sat / cnt}


def twin_forward(head, x, terms=0, h0=None, c0=None, relu="torch"):
    """The whole model in float64 on twin_layer: layer 1 from (h0, c0) (the module's own by default) -> ReLU -> layer 2 seeded with
    layer 1's (hn, cn) -> ReLU -> linear -> log_softmax; dropout is the identity.  ``relu``: see _relu; 'fmax' is the defect of a
    kernel that rectifies with fmaxf (tests/test_nonfinite.py).  Returns the (B, T, 4) log-probs and
    {'pre_min', 'pre_max': over both layers, 'layers': the two layers' own figures}."""
    h0 = head.h0 if h0 is None else h0
    c0 = head.c0 if c0 is None else c0
    y1, hn, cn, s1 = twin_layer(head.lstm_1, x, h0.detach().cpu(), c0.detach().cpu(), terms)
    y2, _, _, s2 = twin_layer(head.lstm_2, y1, hn, cn, terms, relu=relu)
    z = _relu(y2, relu) @ head.linear.weight.detach().double().cpu().t() + head.linear.bias.detach().double().cpu()
    info = {"pre_min": min(s1["pre_min"], s2["pre_min"]), "pre_max": max(s1["pre_max"], s2["pre_max"]), "layers": [s1, s2]}
    return torch.log_softmax(z, dim=2), info


# ------------------------------------------------------------------------------------------------ stock references on the CPU
def stock(head, x, dtype, h0=None, c0=None):
    """The module's own forward (stock nn.LSTM) on the CPU in `dtype`, on a copy: the module is left as it is."""
    h0 = head.h0 if h0 is None else h0
    c0 = head.c0 if c0 is None else c0
    m = SegmenterHead(head.lstm_1.input_size, head.lstm_1.hidden_size, h0.shape[1], h0=h0.detach().cpu().to(dtype),
                      c0=c0.detach().cpu().to(dtype)).to(dtype).eval()
    m.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in head.state_dict().items()})
    with torch.no_grad():
        return m(x.detach().cpu().to(dtype)).double()


def margin_mask(ref64):
    """steps whose two best float64 log-probs are at least MARGIN apart: where an argmax may be compared"""
    top = ref64.topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]) >= MARGIN


class Case:
    """head (float32, on the CPU), x, ref64 / ref32 (stock nn.LSTM on the CPU), err32 = max|ref32 - ref64|, mask"""

    def __init__(self, head, x, h0=None, c0=None):
        self.head, self.x, self.h0, self.c0 = head, x, h0, c0
        self.ref64 = stock(head, x, torch.float64, h0, c0)
        self.ref32 = stock(head, x, torch.float32, h0, c0)
        self.err32 = float((self.ref32 - self.ref64).abs().max())
        self.mask = margin_mask(self.ref64)
        self.left_out = 1.0 - float(self.mask.double().mean())


@functools.lru_cache(maxsize=None)
def dense_case(B, T, H, F, kind="randn", conditioned=True, big_state=False):
    seed = seed_of(B, T, H, F)
    if conditioned:
        head = conditioned_head(B, H, F, seed)
    else:
        torch.manual_seed(seed)
        head = SegmenterHead(F, H, B).eval()
    x = features((B, T, F), B * 7 + T, kind)
    h0, c0 = large_state(B, H, seed + 1) if big_state else (None, None)
    return Case(head, x, h0, c0)


class RaggedCase:
    """A conditioned head and a list of recordings, each with the float64 / float32 module run on it alone from its own state row"""

    def __init__(self, H, F, lens, kind, big_state=False):
        B = len(lens)
        seed = seed_of(B, sum(lens), H, F)
        self.head = conditioned_head(B, H, F, seed)
        self.lens = list(lens)
        self.xs = [features((T, F), seed + 17 * i, kind) for i, T in enumerate(lens)]
        self.h0, self.c0 = large_state(B, H, seed + 1) if big_state else (self.head.h0.clone(), self.head.c0.clone())
        self.ref64, self.ref32 = [], []
        for i, x in enumerate(self.xs):
            h, c = self.h0[:, i:i + 1].contiguous(), self.c0[:, i:i + 1].contiguous()
            self.ref64.append(stock(self.head, x[None], torch.float64, h, c)[0])
            self.ref32.append(stock(self.head, x[None], torch.float32, h, c)[0])
        self.err32 = max(float((a - b).abs().max()) for a, b in zip(self.ref32, self.ref64))
        self.masks = [margin_mask(r) for r in self.ref64]
        self.left_out = 1.0 - sum(float(m.sum()) for m in self.masks) / sum(lens)


@functools.lru_cache(maxsize=None)
def ragged_case(H, F, lens, kind="randn", big_state=False):
    return RaggedCase(H, F, lens, kind, big_state)


# ------------------------------------------------------------------------------------------------ the record of a run
_LINES = []


def report(line):
    """Prints the line and keeps it; with HSS_CONDITIONED_REPORT=<path> set, the lines kept so far are (re)written there -- that is
    how profiles/segmenter_conditioned.txt is made."""
    print(line)
    _LINES.append(line)
    path = os.environ.get("HSS_CONDITIONED_REPORT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(_LINES) + "\n")
