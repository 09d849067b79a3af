"""Build-side counterpart of the feature CONSUMER, for end-to-end checks only (BASELINE config 4).

The reference's ``HeartSoundSegmenter`` (/root/reference/hss/model/segmenter.py:5-87) stays "as-is on
PyTorch-ROCm" (north_star) and is out of scope as code to accelerate; but nothing under
/root/reference exists on the GPU box, so the harness needs a module that loads the same
``state_dict`` (keys ``lstm_1.*``, ``lstm_2.*``, ``linear.*``) and computes the same function:
BiLSTM(in -> 2xH) -> ReLU -> Dropout(0.2) -> BiLSTM(2H -> 2xH), seeded with the first layer's final
(h, c) -> ReLU -> Dropout -> Linear(2H -> 4) -> LogSoftmax over classes (segmenter.py:70-87).
Stock ``nn.LSTM`` (MIOpen): plumbing, not the product.  Pinned by tests/golden/segmenter.npz, which
was produced by the reference class itself (tests/golden/make_golden.py).

``SegmenterHead.hip()`` gives the same forward pass as HIP kernels behind the C ABI (include/hssfsst.h:
hssfsst_segmenter_exec; csrc/segmenter_lstm.hpp), inference only: ``segment(fsst, head.hip(), windows)`` is
config 4 with nothing leaving the device and no torch op between the FSST kernel and the log-probs.  Whole recordings of
different lengths go through ``segment_recordings(fsst, head.hip(), recordings)`` (``HipSegmenter.ragged``,
hssfsst_segmenter_exec_ragged) in one call.

``HipBiLSTM`` is one differentiable bidirectional layer on the HIP recurrences (hssfsst_bilstm_*; csrc/segmenter_train.hpp) and
``HipSegmenterHead`` the same model built from two of them: what a training script uses instead of the ``nn.LSTM`` model.  Both
have a ``ragged`` form that trains on whole recordings of different lengths in one call (hssfsst_bilstm_*_ragged).

``decode_states`` turns log-probs into state sequences: Viterbi decoding under a transition constraint (by default the cardiac
cycle: stay or advance), one HIP call for a whole list of recordings (hssfsst_decode_states; csrc/segmenter_decode.hpp), with
``cyclic_transitions`` / ``transitions_from_labels`` for the transitions and ``state_runs`` for the boundaries.
``decode_durations`` is the same with a score for how long each run lasts (explicit-duration, semi-Markov Viterbi:
hssfsst_decode_durations; csrc/segmenter_decode_durations.hpp), with ``gaussian_durations`` / ``durations_from_labels`` /
``edge_durations`` for its tables.
``state_posteriors`` is the smoothed counterpart of ``decode_states``' path, the per-step state posteriors under the same
transitions, and ``sequence_nll`` the linear-chain sequence loss whose gradient they are: one forward-backward kernel for both
(hssfsst_posteriors; csrc/segmenter_posteriors.hpp).
"""
from __future__ import annotations

from typing import Optional

import ctypes

import numpy as np
import torch
from torch import nn

from . import _lib
from .transforms.synchrosqueeze import RaggedFeatures


class SegmenterHead(nn.Module):
    def __init__(self, input_size: int = 44, hidden_size: int = 240, batch_size: int = 50,
                 h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None):
        super().__init__()
        mk = dict(hidden_size=hidden_size, bidirectional=True, batch_first=True)
        self.lstm_1 = nn.LSTM(input_size=input_size, **mk)
        self.lstm_2 = nn.LSTM(input_size=2 * hidden_size, **mk)
        self.linear = nn.Linear(2 * hidden_size, 4)
        self.drop = nn.Dropout(0.2)
        # the reference keeps random, non-persistent initial states of shape (2, batch, H)
        # (segmenter.py:38-41), which ties the model to one batch size; they are inputs here
        shape = (2, batch_size, hidden_size)
        self.register_buffer("h0", h0 if h0 is not None else torch.randn(shape), persistent=False)
        self.register_buffer("c0", c0 if c0 is not None else torch.randn(shape), persistent=False)

    @classmethod
    def seeded_like_reference(cls, seed: int, input_size: int = 44, hidden_size: int = 240,
                              batch_size: int = 50) -> "SegmenterHead":
        """The module the reference constructor would build under ``torch.manual_seed(seed)``: it draws h0, c0
        first, then initialises lstm_1, lstm_2 and linear (segmenter.py:38-67); same draws, same order here, so a
        fixture only needs the seed and a checksum of the weights (tests/golden/segmenter_c4.npz)."""
        torch.manual_seed(seed)
        shape = (2, batch_size, hidden_size)
        h0, c0 = torch.randn(shape), torch.randn(shape)
        return cls(input_size, hidden_size, batch_size, h0=h0, c0=c0)

    def checksum(self) -> bytes:
        """SHA-256 over the state_dict (sorted keys) and h0 / c0, as written by tests/golden/make_golden.py."""
        import hashlib
        h = hashlib.sha256()
        sd = self.state_dict()
        for k in sorted(sd.keys()):
            h.update(k.encode())
            h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
        h.update(self.h0.detach().cpu().numpy().tobytes())
        h.update(self.c0.detach().cpu().numpy().tobytes())
        return h.digest()

    def forward(self, feats: torch.Tensor) -> torch.Tensor:
        y, carry = self.lstm_1(feats, (self.h0, self.c0))
        y, _ = self.lstm_2(self.drop(torch.relu(y)), carry)
        return torch.log_softmax(self.linear(self.drop(torch.relu(y))), dim=2)

    def hip(self, device=None) -> "HipSegmenter":
        """This module's forward pass as HIP kernels: a callable holding a segmenter plan made from the CURRENT
        ``state_dict``, ``h0`` and ``c0`` (weights changed afterwards do not reach it: call ``hip()`` again).  Inference
        only: a module in training mode is refused with RuntimeError (dropout would be active); no CPU path: without a
        GPU, RuntimeError.  ``device`` defaults to the module's device when that is a GPU, else the current one."""
        return HipSegmenter(self, device)


_LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
              "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")
_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def _ragged_features(name: str, feats, input_size: int, device):
    """The features of a ``ragged`` call as ``(data, offs)``: the ``(sum T, input_size)`` arena (a list is packed with one
    ``torch.cat``, which carries the items' autograd graph; an empty one gives an empty arena on ``device``) and the host list
    of B + 1 offsets.  ``name`` prefixes the messages."""
    if isinstance(feats, RaggedFeatures):
        if feats._raw:
            raise ValueError(f"{name}: raw (complex, frequency-major) features; the segmenter takes abs or stack features")
        data, offs = feats.data, list(feats._off)
    elif isinstance(feats, (list, tuple)):
        for i, f in enumerate(feats):
            if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.shape[0] < 1:
                raise ValueError(f"{name}: item {i} is not a (T, {input_size}) tensor with T >= 1")
        if len({(f.device, f.dtype, int(f.shape[1])) for f in feats}) > 1:
            raise ValueError(f"{name}: the items differ in device, dtype or width")
        offs = [0]
        for f in feats:
            offs.append(offs[-1] + int(f.shape[0]))
        data = torch.cat(list(feats)) if feats else torch.empty((0, input_size), device=device)
    else:
        raise ValueError(f"{name}: a RaggedFeatures or a list of (T, F) tensors expected")
    if data.dim() != 2 or data.shape[1] != input_size or data.shape[0] != offs[-1]:
        raise ValueError(f"{name}: features of shape (sum T, {input_size}) expected, got {tuple(data.shape)}")
    return data, offs


def _ragged_state(name: str, module_h0, module_c0, h0, c0, B: int, H: int):
    """``(h0, c0)`` of a ``ragged`` call on B recordings, checked: the call's own, of shape (2, B, H) or (2, 1, H) and as they
    came (the caller moves them to its device), or the module's when their batch is B or 1."""
    if (h0 is None) != (c0 is None):
        raise ValueError(f"{name}: pass both h0 and c0, or neither")
    if h0 is None:
        if module_h0.shape[1] not in (B, 1) and B:
            raise ValueError(f"{name}: {B} recordings, but the module's h0 / c0 were made for batch {module_h0.shape[1]} "
                             "(pass h0 and c0 of shape (2, B, H) or (2, 1, H) to the call)")
        return module_h0, module_c0
    ok = ((2, B, H), (2, 1, H))
    if tuple(h0.shape) not in ok or tuple(c0.shape) != tuple(h0.shape):
        raise ValueError(f"{name}: h0 and c0 of shape {ok[0]} or {ok[1]} expected, got {tuple(h0.shape)} and {tuple(c0.shape)}")
    return h0, c0


class HipSegmenter:
    """What ``SegmenterHead.hip()`` returns.  ``seg(feats)``: feats a (B, T, F) float32 / float16 / bfloat16 tensor on
    the plan's GPU -> (B, T, 4) float32 log-probs on the same device, no autograd graph, enqueued on the current stream.
    The module's ``h0`` / ``c0`` fix B (the reference ties the model to one batch size, segmenter.py:38-41): another B
    raises ValueError unless ``h0`` and ``c0`` of shape (2, B, H) are passed to the call.

    Limit, here and in ``ragged``: every element of ``h0`` must satisfy ``|h0| < 64`` (``c0``: any finite value).  The kernels feed
    ``h x 1024`` to the recurrent product in float16, sized for an LSTM's own ``|h| < 1``; an ``h0`` element of 64 or more is
    infinite there and its row comes back NaN from the first step on, without an error -- ``h0`` is device memory and the call does
    not synchronise, so nothing checks it.  randn states are far inside; tested up to +-63."""

    def __init__(self, head: SegmenterHead, device=None):
        if head.training:
            raise RuntimeError("SegmenterHead.hip(): the module is in training mode; the HIP path is inference only "
                               "(dropout is the identity): call .eval() first")
        sd = {k: v.detach().to("cpu", torch.float32).contiguous() for k, v in head.state_dict().items()}
        self.input_size, self.hidden_size = head.lstm_1.input_size, head.lstm_1.hidden_size
        if device is None:
            device = head.h0.device if head.h0.device.type == "cuda" else "cuda"
        self._plan = None
        L = _lib.lib()
        _lib.guard_fork()
        if not torch.cuda.is_available():
            raise RuntimeError("SegmenterHead.hip(): no GPU; the segmenter kernels have no CPU path")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"SegmenterHead.hip(): device {self.device} is not a GPU; there is no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

        def ptrs(prefix):
            return (ctypes.c_void_p * 8)(*[sd[f"{prefix}.{k}"].data_ptr() for k in _LSTM_KEYS])
        plan = ctypes.c_void_p()
        _lib.check(L.hssfsst_segmenter_create(ctypes.byref(plan), self.device.index, self.input_size, self.hidden_size,
                                              ptrs("lstm_1"), ptrs("lstm_2"), sd["linear.weight"].data_ptr(),
                                              sd["linear.bias"].data_ptr()), "hssfsst_segmenter_create")
        self._plan = plan
        self.h0 = head.h0.detach().to(self.device, torch.float32).contiguous().clone()
        self.c0 = head.c0.detach().to(self.device, torch.float32).contiguous().clone()

    def __del__(self):
        if getattr(self, "_plan", None):
            try:
                _lib.lib().hssfsst_segmenter_destroy(self._plan)
            except Exception:
                pass
            self._plan = None

    def __call__(self, feats: torch.Tensor, h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None) -> torch.Tensor:
        if feats.dim() != 3 or feats.shape[2] != self.input_size or feats.shape[0] < 1 or feats.shape[1] < 1:
            raise ValueError(f"HipSegmenter: features of shape (B, T, {self.input_size}) expected, got {tuple(feats.shape)}")
        if feats.device != self.device:
            raise ValueError(f"HipSegmenter: features on {feats.device}, the plan on {self.device}")
        if feats.dtype not in _DTYPES:
            raise ValueError(f"HipSegmenter: float32, float16 or bfloat16 features expected, got {feats.dtype}")
        B, T = int(feats.shape[0]), int(feats.shape[1])
        if (h0 is None) != (c0 is None):
            raise ValueError("HipSegmenter: pass both h0 and c0, or neither")
        if h0 is None:
            if self.h0.shape[1] != B:
                raise ValueError(f"HipSegmenter: batch {B}, but the module's h0 / c0 were made for batch {self.h0.shape[1]} "
                                 "(pass h0 and c0 of shape (2, B, H) to the call)")
            h0, c0 = self.h0, self.c0
        else:
            want = (2, B, self.hidden_size)
            if tuple(h0.shape) != want or tuple(c0.shape) != want:
                raise ValueError(f"HipSegmenter: h0 and c0 of shape {want} expected, got {tuple(h0.shape)} and {tuple(c0.shape)}")
            h0 = h0.detach().to(self.device, torch.float32).contiguous()
            c0 = c0.detach().to(self.device, torch.float32).contiguous()
        feats = feats.detach().contiguous()
        out = torch.empty((B, T, 4), dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(_lib.lib().hssfsst_segmenter_exec(self._plan, feats.data_ptr(), _DTYPES[feats.dtype], B, T, h0.data_ptr(),
                                                     c0.data_ptr(), out.data_ptr(), stream), "hssfsst_segmenter_exec")
        return out

    def ragged(self, feats, h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None,
               max_steps: int = 1 << 23) -> RaggedFeatures:
        """Whole recordings of DIFFERENT lengths in one call (``hssfsst_segmenter_exec_ragged``).  ``feats``: the non-raw
        ``RaggedFeatures`` of ``FSST.ragged`` (float32 / float16 / bfloat16, on the plan's GPU), or a list / tuple of ``(T_i, F)``
        tensors, which is packed into one arena on the device.  Returns a ``RaggedFeatures`` over a ``(sum T, 4)`` float32 arena
        with the same offsets; item i equals ``self(feats[i][None], h0[:, i:i+1], c0[:, i:i+1])[0]`` bit for bit: forward from
        the recording's first step, reverse from its own last one, layer 2 seeded at its own ends -- which padding to
        ``(B, T_max, F)`` cannot give.

        ``h0`` / ``c0``: ``(2, B, H)``, or ``(2, 1, H)`` to start every recording from the same state; omitted, the module's own
        are used when their batch is B or 1, else ValueError.

        ``max_steps`` bounds the scratch: the list is processed in consecutive groups whose total steps stay within it (a longer
        recording is a group of its own), all writing into the one output arena; the result does not depend on it.  The layer
        outputs take 2 x steps x 2H x 4 bytes: 2 x 8.4 M x 480 x 4 B = 32 GB at the default with hidden 240 (plus at most
        128 MiB of projected inputs and 16 KiB of state per 16 recordings); lower it on a device that is shared."""
        name = "HipSegmenter.ragged"
        data, offs = _ragged_features(name, feats, self.input_size, self.device)
        B = len(offs) - 1
        if data.device != self.device:
            raise ValueError(f"{name}: features on {data.device}, the plan on {self.device}")
        if data.dtype not in _DTYPES:
            raise ValueError(f"{name}: float32, float16 or bfloat16 features expected, got {data.dtype}")
        own = h0 is not None
        h0, c0 = _ragged_state(name, self.h0, self.c0, h0, c0, B, self.hidden_size)
        if own:
            h0 = h0.detach().to(self.device, torch.float32).contiguous()
            c0 = c0.detach().to(self.device, torch.float32).contiguous()
        if max_steps < 1:
            raise ValueError(f"HipSegmenter.ragged: max_steps {max_steps} must be positive")
        out = torch.empty((offs[-1], 4), dtype=torch.float32, device=self.device)
        result = RaggedFeatures(out, torch.tensor(offs, dtype=torch.int64), 4, False)
        if B == 0:
            return result
        data = data.detach().contiguous()
        rows = 1 if h0.shape[1] == 1 else B
        stream = torch.cuda.current_stream(self.device).cuda_stream
        L = _lib.lib()
        i = 0
        while i < B:                                    # consecutive groups of at most max_steps steps
            j = i + 1
            while j < B and offs[j + 1] - offs[i] <= max_steps:
                j += 1
            sub = np.asarray(offs[i:j + 1], dtype=np.int64) - offs[i]
            hs, cs = (h0, c0) if rows == 1 else (h0[:, i:j].contiguous(), c0[:, i:j].contiguous())
            _lib.check(L.hssfsst_segmenter_exec_ragged(self._plan, data[offs[i]:].data_ptr(), _DTYPES[data.dtype],
                                                       sub.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), j - i, hs.data_ptr(),
                                                       cs.data_ptr(), 1 if rows == 1 else j - i, out[offs[i]:].data_ptr(), stream),
                       "hssfsst_segmenter_exec_ragged")
            i = j
        return result


# What the dense and the ragged autograd Function of HipBiLSTM share; their saved state and their calls differ.
def _forward_outputs(x, y_shape, B: int, H: int):
    """``(y, hn, cn)`` of a forward, uninitialised."""
    y = torch.empty(y_shape, dtype=torch.float32, device=x.device)
    hn = torch.empty((2, B, H), dtype=torch.float32, device=x.device)
    return y, hn, torch.empty_like(hn)


def _backward_inputs(ctx, dy, dhn, dcn):
    """The saved tensors of a backward whose layer still holds the forward's weights, and its seeds as the ABI takes them:
    ``dy`` contiguous (zeros for None), ``dhn`` / ``dcn`` contiguous or None (the ABI's NULL: zero)."""
    if ctx.layer._serial != ctx.serial:
        raise RuntimeError("HipBiLSTM: the layer's weights were repacked for other values between this forward and its "
                           "backward; the backward recurrence would run against the wrong W_hh")
    x, h0, c0, y, stash, *weights = ctx.saved_tensors
    dy = torch.zeros_like(y) if dy is None else dy.contiguous()
    dhn = None if dhn is None else dhn.contiguous()
    dcn = None if dcn is None else dcn.contiguous()
    return x, h0, c0, y, stash, weights, dy, dhn, dcn


def _ptr(t):
    return None if t is None else t.data_ptr()


def _backward_outputs(x, dgates_shape, B: int, H: int):
    """``(dgates, dh0, dc0)`` of a backward, uninitialised."""
    dgates = torch.empty(dgates_shape, dtype=torch.float32, device=x.device)
    dh0 = torch.empty((2, B, H), dtype=torch.float32, device=x.device)
    return dgates, dh0, torch.empty_like(dh0)


def _weight_grads(g_fwd, g_rev, x2d, hprev_fwd, hprev_rev, weights, need_dx: bool):
    """The time-parallel products of a backward over ``rows`` = all steps of all recordings: ``g_*`` (rows, 4H) the directions'
    gate gradients, ``x2d`` (rows, F), ``hprev_*`` (rows, H) the h before each step.  Returns ``(dx (rows, F) or None, the eight
    parameter gradients in _LSTM_KEYS order)``."""
    grads = []
    for g, hprev in ((g_fwd, hprev_fwd), (g_rev, hprev_rev)):
        db = g.sum(0)
        grads += [g.t() @ x2d, g.t() @ hprev, db, db.clone()]
    return (g_fwd @ weights[0] + g_rev @ weights[4] if need_dx else None), grads


class _BiLSTMFunction(torch.autograd.Function):
    """forward: hssfsst_bilstm_forward (projection + recurrence kernels, which also fill the stash); backward:
    hssfsst_bilstm_backward (the backward recurrence, which is sequential) and then the time-parallel products as torch.matmul."""

    @staticmethod
    def forward(ctx, layer, x, h0, c0, *weights):
        B, T, H = int(x.shape[0]), int(x.shape[1]), layer.hidden_size
        plan = layer._sync_plan(x.device, weights)
        L = _lib.lib()
        x, h0, c0 = x.contiguous(), h0.contiguous(), c0.contiguous()
        floats = ctypes.c_int64()
        _lib.check(L.hssfsst_bilstm_stash_floats(plan, B, T, ctypes.byref(floats)), "hssfsst_bilstm_stash_floats")
        stash = torch.empty(floats.value, dtype=torch.float32, device=x.device)
        y, hn, cn = _forward_outputs(x, (B, T, 2 * H), B, H)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(L.hssfsst_bilstm_forward(plan, x.data_ptr(), B, T, h0.data_ptr(), c0.data_ptr(), y.data_ptr(), hn.data_ptr(),
                                            cn.data_ptr(), stash.data_ptr(), stream), "hssfsst_bilstm_forward")
        ctx.layer, ctx.serial = layer, layer._serial
        ctx.save_for_backward(x, h0, c0, y, stash, *weights)
        return y, hn, cn

    @staticmethod
    def backward(ctx, dy, dhn, dcn):
        x, h0, c0, y, stash, weights, dy, dhn, dcn = _backward_inputs(ctx, dy, dhn, dcn)
        B, T, H = int(x.shape[0]), int(x.shape[1]), ctx.layer.hidden_size
        dgates, dh0, dc0 = _backward_outputs(x, (2, B, T, 4 * H), B, H)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(_lib.lib().hssfsst_bilstm_backward(ctx.layer._plan, stash.data_ptr(), c0.data_ptr(), dy.data_ptr(), _ptr(dhn), _ptr(dcn),
                                                      B, T, dgates.data_ptr(), dh0.data_ptr(), dc0.data_ptr(), stream),
                   "hssfsst_bilstm_backward")
        # h before each step: y shifted one step towards the direction's start, with h0 in front
        hf = torch.cat((h0[0].unsqueeze(1), y[:, :-1, :H]), dim=1)
        hr = torch.cat((y[:, 1:, H:], h0[1].unsqueeze(1)), dim=1)
        dx, grads = _weight_grads(dgates[0].reshape(B * T, 4 * H), dgates[1].reshape(B * T, 4 * H), x.reshape(B * T, -1),
                                  hf.reshape(B * T, H), hr.reshape(B * T, H), weights, ctx.needs_input_grad[1])
        return (None, None if dx is None else dx.reshape(x.shape), dh0, dc0, *grads)


class _RaggedBiLSTMFunction(torch.autograd.Function):
    """``_BiLSTMFunction`` on an arena of recordings: hssfsst_bilstm_forward_ragged / hssfsst_bilstm_backward_ragged, then the same
    time-parallel products as torch.matmul over the arena's rows.  ``offs``: the host offsets, an int64 numpy array."""

    @staticmethod
    def forward(ctx, layer, offs, x, h0, c0, *weights):
        B, total, H = len(offs) - 1, int(x.shape[0]), layer.hidden_size
        plan = layer._sync_plan(x.device, weights)
        L = _lib.lib()
        x, h0, c0 = x.contiguous(), h0.contiguous(), c0.contiguous()
        optr = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        floats = ctypes.c_int64()
        _lib.check(L.hssfsst_bilstm_stash_floats_ragged(plan, optr, B, ctypes.byref(floats)), "hssfsst_bilstm_stash_floats_ragged")
        stash = torch.empty(floats.value, dtype=torch.float32, device=x.device)
        y, hn, cn = _forward_outputs(x, (total, 2 * H), B, H)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(L.hssfsst_bilstm_forward_ragged(plan, x.data_ptr(), optr, B, h0.data_ptr(), c0.data_ptr(), y.data_ptr(),
                                                   hn.data_ptr(), cn.data_ptr(), stash.data_ptr(), stream), "hssfsst_bilstm_forward_ragged")
        ctx.layer, ctx.serial, ctx.offs = layer, layer._serial, offs
        ctx.save_for_backward(x, h0, c0, y, stash, *weights)
        return y, hn, cn

    @staticmethod
    def backward(ctx, dy, dhn, dcn):
        x, h0, c0, y, stash, weights, dy, dhn, dcn = _backward_inputs(ctx, dy, dhn, dcn)
        offs = ctx.offs
        B, total, H = len(offs) - 1, int(x.shape[0]), ctx.layer.hidden_size
        dgates, dh0, dc0 = _backward_outputs(x, (2, total, 4 * H), B, H)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(_lib.lib().hssfsst_bilstm_backward_ragged(ctx.layer._plan, stash.data_ptr(), c0.data_ptr(), dy.data_ptr(), _ptr(dhn),
                                                             _ptr(dcn), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), B,
                                                             dgates.data_ptr(), dh0.data_ptr(), dc0.data_ptr(), stream),
                   "hssfsst_bilstm_backward_ragged")
        # h before each step: y shifted by one arena row, with h0 written at each recording's first (reverse: last) row
        edges = torch.from_numpy(offs).to(x.device)
        hf = torch.cat((y.new_zeros(1, H), y[:-1, :H]))
        hf[edges[:-1]] = h0[0]
        hr = torch.cat((y[1:, H:], y.new_zeros(1, H)))
        hr[edges[1:] - 1] = h0[1]
        dx, grads = _weight_grads(dgates[0], dgates[1], x, hf, hr, weights, ctx.needs_input_grad[2])
        return (None, None, dx, dh0, dc0, *grads)


class HipBiLSTM(nn.Module):
    """One bidirectional, batch-first LSTM layer that TRAINS on the HIP kernels: ``y, (hn, cn) = layer(x, (h0, c0))`` with
    x (B, T, input_size), h0 / c0 (2, B, hidden_size), all float32 on the GPU, differentiable in x, h0, c0 and the weights.
    The parameters carry ``nn.LSTM``'s names, shapes and initialisation (``weight_ih_l0`` ... ``bias_hh_l0_reverse``), so a
    ``state_dict`` moves both ways.  The forward pass is the inference kernels' (csrc/segmenter_lstm.hpp) and keeps every step's
    gates and cell state in a stash; the backward recurrence is a HIP kernel (csrc/segmenter_train.hpp), the weight and input
    gradients are ``torch.matmul`` on its output.  The weights are repacked on the device (no host synchronisation) whenever a
    parameter changed since the last forward.  The stash costs 2 x ceil(B / 16) x T x 80 KiB per layer and forward call: about
    1.3 GB at B 50, T 2000, whatever the hidden size.  hidden_size <= 256.  ``|h0| < 64`` in every element (the limit of
    ``HipSegmenter``, for the same reason, unchecked: a larger one makes its row NaN, gradients included); ``c0`` any finite value.
    No CPU path: without a GPU, RuntimeError."""

    def __init__(self, input_size: int, hidden_size: int):
        super().__init__()
        self._take(nn.LSTM(input_size=input_size, hidden_size=hidden_size, bidirectional=True, batch_first=True))

    def _take(self, lstm: nn.LSTM) -> None:
        """The sizes and the parameters of ``lstm``; no plan yet."""
        self.input_size, self.hidden_size = int(lstm.input_size), int(lstm.hidden_size)
        for k in _LSTM_KEYS:
            self.register_parameter(k, getattr(lstm, k))
        self._plan, self._plan_device, self._packed, self._serial = None, None, None, 0

    @classmethod
    def from_lstm(cls, lstm: nn.LSTM) -> "HipBiLSTM":
        """A layer that takes over the parameters of a one-layer bidirectional batch-first ``nn.LSTM``."""
        if lstm.num_layers != 1 or not lstm.bidirectional or not lstm.batch_first or not lstm.bias or lstm.proj_size:
            raise ValueError("HipBiLSTM.from_lstm: a one-layer, bidirectional, batch-first nn.LSTM with biases expected")
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self._take(lstm)
        return self

    def __getstate__(self):                                  # (a copy or a pickle makes its own plan on first use)
        state = self.__dict__.copy()
        state.update(_plan=None, _plan_device=None, _packed=None)
        return state

    def __del__(self):
        if getattr(self, "_plan", None):
            try:
                _lib.lib().hssfsst_bilstm_destroy(self._plan)
            except Exception:
                pass
            self._plan = None

    def _sync_plan(self, device, weights):
        """The plan on ``device`` holding the CURRENT weights: made on first use, repacked when a parameter changed."""
        L = _lib.lib()
        if self._plan is None or self._plan_device != device:
            if self._plan is not None:
                _lib.check(L.hssfsst_bilstm_destroy(self._plan), "hssfsst_bilstm_destroy")
                self._plan = None
            plan = ctypes.c_void_p()
            _lib.check(L.hssfsst_bilstm_create(ctypes.byref(plan), device.index, self.input_size, self.hidden_size),
                       "hssfsst_bilstm_create")
            self._plan, self._plan_device, self._packed = plan, device, None
        key = tuple((w.data_ptr(), w._version) for w in weights)
        if key != self._packed:
            ptrs = (ctypes.c_void_p * 8)(*[w.data_ptr() for w in weights])
            _lib.check(L.hssfsst_bilstm_set_weights(self._plan, ptrs, torch.cuda.current_stream(device).cuda_stream),
                       "hssfsst_bilstm_set_weights")
            self._packed = key
            self._serial += 1
        return self._plan

    @staticmethod
    def _check_layer_inputs(name: str, x, h0, c0, weights) -> None:
        """What the dense and the ragged call ask of their tensors whatever the shapes: the library, a GPU, one device, float32,
        contiguous parameters.  ``name`` prefixes the messages."""
        L = _lib.lib()                                       # (a missing library is said first)
        del L
        _lib.guard_fork()
        if not torch.cuda.is_available():
            raise RuntimeError("HipBiLSTM: no GPU; the BiLSTM kernels have no CPU path")
        if x.device.type != "cuda" or any(t.device != x.device for t in (h0, c0, *weights)):
            raise RuntimeError(f"{name}: input, state and parameters must be on one GPU (input on {x.device}, "
                               f"parameters on {weights[0].device}); there is no CPU path")
        if any(t.dtype != torch.float32 for t in (x, h0, c0, *weights)):
            raise ValueError(f"{name}: float32 input, state and parameters expected (cast half-precision features first)")
        if any(not w.is_contiguous() for w in weights):
            raise ValueError(f"{name}: contiguous parameters expected")

    def forward(self, x: torch.Tensor, state):
        h0, c0 = state
        weights = [getattr(self, k) for k in _LSTM_KEYS]
        self._check_layer_inputs("HipBiLSTM", x, h0, c0, weights)
        if x.dim() != 3 or x.shape[2] != self.input_size or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"HipBiLSTM: input of shape (B, T, {self.input_size}) expected, got {tuple(x.shape)}")
        want = (2, int(x.shape[0]), self.hidden_size)
        if tuple(h0.shape) != want or tuple(c0.shape) != want:
            raise ValueError(f"HipBiLSTM: h0 and c0 of shape {want} expected, got {tuple(h0.shape)} and {tuple(c0.shape)}")
        y, hn, cn = _BiLSTMFunction.apply(self, x, h0, c0, *weights)
        return y, (hn, cn)

    def ragged(self, x: torch.Tensor, offsets, state):
        """The layer on whole recordings of DIFFERENT lengths in one call: ``y, (hn, cn) = layer.ragged(x, offsets, (h0, c0))``.
        ``x``: a ``(sum T, input_size)`` float32 arena on the GPU, recording i in rows ``offsets[i] .. offsets[i + 1]``; ``offsets``:
        a list or an int64 tensor of B + 1 offsets from 0 (read on the host); ``h0`` / ``c0``: ``(2, B, hidden_size)``.  ``y`` is the
        ``(sum T, 2 hidden_size)`` arena, ``hn`` / ``cn`` ``(2, B, hidden_size)`` in list order.  Differentiable in x, h0, c0 and the
        weights like the dense call, and recording i gets the bits of ``layer(x_i[None], (h0[:, i:i+1], c0[:, i:i+1]))`` in y, hn,
        cn, dh0 and dc0: forward from its first step, reverse from its own last one, which padding to ``(B, T_max, F)`` cannot
        give.  (The weight and input gradients are one ``torch.matmul`` over all rows: the sum of the per-recording ones up to
        the rounding of a longer sum.)  The stash costs 2 x (sum over tiles of 16 recordings, longest first, of the tile's longest
        recording) x 80 KiB per layer and call: 5.8 GB per layer for one tile of 35 500-step recordings.  An empty list gives
        empty results.  ``|h0| < 64``, as for the dense call."""
        h0, c0 = state
        weights = [getattr(self, k) for k in _LSTM_KEYS]
        self._check_layer_inputs("HipBiLSTM.ragged", x, h0, c0, weights)
        offs = np.ascontiguousarray(offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64)
        if offs.ndim != 1 or offs.shape[0] < 1:
            raise ValueError("HipBiLSTM.ragged: offsets must be a 1-D sequence of B + 1 step offsets")
        B = int(offs.shape[0]) - 1
        if x.dim() != 2 or x.shape[1] != self.input_size or x.shape[0] != int(offs[-1]) or int(offs[0]) != 0:
            raise ValueError(f"HipBiLSTM.ragged: an arena of shape (offsets[-1], {self.input_size}) and offsets from 0 expected, got "
                             f"{tuple(x.shape)} and offsets {int(offs[0])} .. {int(offs[-1])}")
        want = (2, B, self.hidden_size)
        if tuple(h0.shape) != want or tuple(c0.shape) != want:
            raise ValueError(f"HipBiLSTM.ragged: h0 and c0 of shape {want} expected, got {tuple(h0.shape)} and {tuple(c0.shape)}")
        if B == 0:
            return x.new_empty((0, 2 * self.hidden_size)), (h0.clone(), c0.clone())
        y, hn, cn = _RaggedBiLSTMFunction.apply(self, offs, x, h0, c0, *weights)
        return y, (hn, cn)


class HipSegmenterHead(SegmenterHead):
    """``SegmenterHead`` whose two BiLSTM layers are ``HipBiLSTM``: the same constructor, ``state_dict`` keys, ``h0`` / ``c0``
    buffers, random draws and ``forward`` (layer 1 -> ReLU -> Dropout(0.2) -> layer 2 seeded with layer 1's (hn, cn) -> ReLU ->
    Dropout -> Linear -> log_softmax), in ``train()`` and ``eval()``; everything outside the layers is torch under autograd.
    A training script swaps the class and moves the module to the GPU; ``hip()`` stays the inference-only plan of the base."""

    def __init__(self, input_size: int = 44, hidden_size: int = 240, batch_size: int = 50,
                 h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None):
        super().__init__(input_size, hidden_size, batch_size, h0=h0, c0=c0)
        self.lstm_1 = HipBiLSTM.from_lstm(self.lstm_1)
        self.lstm_2 = HipBiLSTM.from_lstm(self.lstm_2)

    def ragged(self, feats, h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None) -> RaggedFeatures:
        """``forward`` on whole recordings of DIFFERENT lengths in one call, for training: layer 1 -> ReLU -> Dropout -> layer 2
        seeded with layer 1's (hn, cn) -> ReLU -> Dropout -> Linear -> log_softmax, in ``train()`` and ``eval()``, every recording
        from its own first and last step (``HipBiLSTM.ragged``).  ``feats``: a non-raw ``RaggedFeatures`` (``FSST.ragged``) or a list
        of ``(T_i, F)`` tensors on the module's GPU; float16 / bfloat16 features are cast to float32 with one torch op (a copy of the
        arena: half input to the kernels is not there).  Returns a ``RaggedFeatures`` over the ``(sum T, 4)`` arena of log-probs,
        whose ``data`` carries the autograd graph: ``nll_loss(out.data, torch.cat(labels))`` is the loss over all steps.

        ``h0`` / ``c0``: ``(2, B, H)``, or ``(2, 1, H)`` to start every recording from the same state (expanded in torch, so autograd
        sums its gradient); omitted, the module's own are used when their batch is B or 1, else ValueError.

        The stash of the two layers costs 2 x 2 x (sum over tiles of the tile's longest recording) x 80 KiB: 5.8 GB per layer for
        one tile of 35 500-step recordings.  Split the list to bound it."""
        name = "HipSegmenterHead.ragged"
        F, H = self.lstm_1.input_size, self.lstm_1.hidden_size
        L = _lib.lib()
        del L
        _lib.guard_fork()
        if not torch.cuda.is_available():
            raise RuntimeError(f"{name}: no GPU; the BiLSTM kernels have no CPU path")
        device = self.linear.weight.device
        data, offs = _ragged_features(name, feats, F, device)
        B = len(offs) - 1
        if data.device != device:
            raise ValueError(f"{name}: features on {data.device}, the module on {device}")
        if data.dtype not in _DTYPES:
            raise ValueError(f"{name}: float32, float16 or bfloat16 features expected, got {data.dtype}")
        own = h0 is not None
        h0, c0 = _ragged_state(name, self.h0, self.c0, h0, c0, B, H)
        if own:
            h0, c0 = h0.to(device, torch.float32), c0.to(device, torch.float32)     # (carries the autograd graph)
        offsets = torch.tensor(offs, dtype=torch.int64)
        if B == 0:
            return RaggedFeatures(torch.empty((0, 4), dtype=torch.float32, device=device), offsets, 4, False)
        if h0.shape[1] != B:
            h0, c0 = h0.expand(2, B, H), c0.expand(2, B, H)
        x = data.float()                                     # (half features: the one cast, a float32 copy of the arena)
        y, carry = self.lstm_1.ragged(x, offs, (h0.contiguous(), c0.contiguous()))
        y, _ = self.lstm_2.ragged(self.drop(torch.relu(y)), offs, carry)
        logp = torch.log_softmax(self.linear(self.drop(torch.relu(y))), dim=1)
        return RaggedFeatures(logp, offsets, 4, False)


def segment(fsst, head, windows: torch.Tensor) -> torch.Tensor:
    """windows (B, n) -> HIP FSST features (B, n, 2K), kept on the device -> (B, n, 4) log-probs.  ``head``: a
    ``SegmenterHead`` (stock ``nn.LSTM``) or what its ``hip()`` returns (the HIP kernels)."""
    return head(fsst.batch(windows))


def segment_recordings(fsst, seg: HipSegmenter, recordings, decode=None, durations=None, posteriors=None, **kw) -> RaggedFeatures:
    """Whole recordings of different lengths (a list of 1-D signals on the GPU) -> ``FSST.ragged`` features, kept on the device
    -> a ``RaggedFeatures`` of ``(T_i, 4)`` log-probs: ``segment()`` for whole recordings.  ``kw`` goes to
    ``HipSegmenter.ragged`` (h0, c0, max_steps).  ``decode=True`` or ``decode=(A, pi)``: the log-probs go on to ``decode_states``
    (default or given transitions) and the ``RaggedStates`` of ``(T_i,)`` uint8 state sequences is returned instead; with
    ``durations=dur`` (4, D) they go to ``decode_durations`` under that table, its default ``edge`` and the same transitions.
    ``posteriors=True`` or ``posteriors=(A, pi)``: they go on to ``state_posteriors`` instead and the ``RaggedFeatures`` of
    ``(T_i, 4)`` float32 posteriors is returned, with ``durations=dur`` those of ``duration_posteriors`` under that table and its
    default ``edge``; not together with ``decode`` (ValueError).  ``durations`` without either raises ValueError."""
    want_post = not (posteriors is None or posteriors is False)
    want_decode = not (decode is None or decode is False)
    if want_post and want_decode:
        raise ValueError("segment_recordings: posteriors and decode exclude each other: one call returns one of them")
    if durations is not None and not (want_decode or want_post):
        raise ValueError("segment_recordings: durations are for decoding or posteriors: pass decode=True, decode=(A, pi), "
                         "posteriors=True or posteriors=(A, pi) with them")
    logp = seg.ragged(fsst.ragged(recordings), **kw)
    if want_post:
        A, pi = (None, None) if posteriors is True else posteriors
        if durations is not None:
            return duration_posteriors(logp, durations, A, pi)
        return state_posteriors(logp, A, pi)
    if decode is None or decode is False:
        return logp
    A, pi = (None, None) if decode is True else decode
    if durations is not None:
        return decode_durations(logp, durations, A, pi)
    return decode_states(logp, A, pi)


# ------------------------------------------------------------------------------------------- log-probs -> state sequences
class RaggedStates(RaggedFeatures):
    """What ``decode_states`` returns for a ragged input: a ``RaggedFeatures`` whose arena ``data`` is ``(sum T,)`` uint8 and whose
    item i is the ``(T_i,)`` state sequence of recording i (a view).  ``scores``: ``(B,)`` float64 on the host when asked for."""

    def __init__(self, data: torch.Tensor, offsets: torch.Tensor):
        super().__init__(data, offsets, 1, False)
        self.scores = None

    def padded(self, padding_value: int = 0) -> torch.Tensor:
        """``(B, T_max)`` uint8 with ``padding_value`` past each recording's end."""
        B = len(self)
        lens = self.lengths().to(self.data.device)
        T = int(lens.max()) if B else 0
        out = torch.full((B, T), int(padding_value), dtype=self.data.dtype, device=self.data.device)
        if B and T:
            out[torch.arange(T, device=self.data.device)[None, :] < lens[:, None]] = self.data
        return out


def cyclic_transitions(stay_logp: float = 0.0, advance_logp: float = 0.0):
    """``(A, pi)`` of the cardiac cycle S1 -> systole -> S2 -> diastole -> S1: ``A[i][i] = stay_logp``, ``A[i][(i + 1) % 4] =
    advance_logp``, every other move ``-inf`` (forbidden); ``pi`` uniform (zeros).  float32 numpy arrays (4, 4) and (4,)."""
    A = np.full((4, 4), -np.inf, dtype=np.float32)
    for i in range(4):
        A[i, i] = stay_logp
        A[i, (i + 1) % 4] = advance_logp
    return A, np.zeros(4, dtype=np.float32)


def transitions_from_labels(labels):
    """``(A, pi)`` counted from label sequences (a list of 1-D integer tensors or arrays with values 0..3): ``A`` = log of the
    row-normalised transition counts over consecutive steps, ``pi`` = log of the start-state frequencies; ``-inf`` where never
    seen.  Host numpy, float64 counts, float32 result.  A state that is never left (no step follows it in any sequence) has an
    all ``-inf`` row, which ``decode_states`` refuses: such labels do not describe a cycle."""
    counts, starts = np.zeros((4, 4), dtype=np.float64), np.zeros(4, dtype=np.float64)
    for k, lab in enumerate(labels):
        a = lab.detach().cpu().numpy() if isinstance(lab, torch.Tensor) else np.asarray(lab)
        if a.ndim != 1 or a.size < 1 or a.dtype.kind not in "iu":
            raise ValueError(f"transitions_from_labels: item {k} is not a non-empty 1-D integer sequence")
        a = a.astype(np.int64)
        if a.min() < 0 or a.max() > 3:
            raise ValueError(f"transitions_from_labels: item {k} has labels outside 0..3")
        starts[a[0]] += 1
        np.add.at(counts, (a[:-1], a[1:]), 1)
    if starts.sum() == 0:
        raise ValueError("transitions_from_labels: no label sequence")
    with np.errstate(divide="ignore", invalid="ignore"):
        rows = counts.sum(axis=1, keepdims=True)
        A = np.where(counts > 0, np.log(counts / np.where(rows > 0, rows, 1.0)), -np.inf)
        pi = np.where(starts > 0, np.log(starts / starts.sum()), -np.inf)
    return A.astype(np.float32), pi.astype(np.float32)


def decode_info():
    """``(segment_steps, max_steps)`` of the decoder (``hssfsst_decode_info``): the steps a workgroup stages at a time and the
    longest recording it takes.  No device needed."""
    seg, mx = ctypes.c_int(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().hssfsst_decode_info(ctypes.byref(seg), ctypes.byref(mx)), "hssfsst_decode_info")
    return seg.value, mx.value


def _decode_input(name: str, logp):
    """The three input kinds of the decoders -> (the (sum T, 4) arena, the step offsets as a list, the kind)."""
    if isinstance(logp, RaggedFeatures):
        if logp._raw:
            raise ValueError(f"{name}: raw features are not log-probs")
        data, offs, kind = logp.data, [int(o) for o in logp._off], "ragged"
    elif isinstance(logp, torch.Tensor) and logp.dim() == 3:
        B, T = int(logp.shape[0]), int(logp.shape[1])
        data, offs, kind = logp.reshape(B * T, -1) if B * T else logp.reshape(0, logp.shape[2]), [i * T for i in range(B + 1)], "batch"
        if B and T < 1:
            raise ValueError(f"{name}: (B, T, 4) log-probs with T >= 1 expected, got {tuple(logp.shape)}")
    elif isinstance(logp, torch.Tensor) and logp.dim() == 2:
        data, offs, kind = logp, [0, int(logp.shape[0])], "single"
        if logp.shape[0] < 1:
            raise ValueError(f"{name}: (T, 4) log-probs with T >= 1 expected, got {tuple(logp.shape)}")
    else:
        raise ValueError(f"{name}: a RaggedFeatures, a (B, T, 4) or a (T, 4) tensor expected")
    if data.dim() != 2 or data.shape[1] != 4 or data.shape[0] != offs[-1]:
        raise ValueError(f"{name}: log-probs over 4 states expected, got an arena of shape {tuple(data.shape)}")
    if data.dtype != torch.float32:
        raise ValueError(f"{name}: float32 log-probs expected, got {data.dtype}")
    if data.device.type != "cuda":
        raise ValueError(f"{name}: log-probs on a GPU expected, got {data.device}; the decoder has no CPU path")
    return data, offs, kind


def _decode_output(logp, kind: str, states, offs, scores):
    """The states in the kind of the input; with ``scores`` (int64 on the device, or None) also the float64 scores on the host."""
    if kind == "ragged":
        out = RaggedStates(states, torch.tensor(offs, dtype=torch.int64))
    elif kind == "batch":
        out = states.view(int(logp.shape[0]), int(logp.shape[1]))
    else:
        out = states
    if scores is None:
        return out
    # (NEG, the score of a recording with an all -inf step, reads as -inf)
    sc = scores.cpu()
    val = torch.where(sc == torch.iinfo(torch.int64).min, torch.tensor(float("-inf"), dtype=torch.float64), sc.double() / float(1 << 20))
    if kind == "ragged":
        out.scores = val
    return out, (val[0] if kind == "single" else val)


def decode_states(logp, transitions=None, initial=None, return_scores: bool = False):
    """Viterbi decoding on the device (``hssfsst_decode_states``): log-probs -> the best state sequence 0..3 (S1, systole, S2,
    diastole) under log transitions ``transitions`` (4, 4) and log initial scores ``initial`` (4,); ``-inf`` = forbidden; default
    ``cyclic_transitions()``: stay or advance, which a per-step argmax does not respect.

    ``logp``: the ``RaggedFeatures`` of ``HipSegmenter.ragged`` / ``HipSegmenterHead.ragged`` (a ``(sum T, 4)`` arena), a
    ``(B, T, 4)`` tensor or a ``(T, 4)`` tensor; float32 on a GPU, anything else raises ValueError.  Returns the same kind: a
    ``RaggedStates`` (item i a ``(T_i,)`` uint8 view of one arena), a ``(B, T)`` or a ``(T,)`` uint8 tensor.  One call, enqueued
    on the current stream, whatever the lengths; the dense forms are the same call with regular offsets.
    ``return_scores=True``: also the best paths' scores, float64 ``(B,)`` on the host (a scalar tensor for ``(T, 4)``), which
    waits for the device.

    Exact arithmetic (include/hssfsst.h): every value is rounded to a multiple of 2^-20 after clamping to +-32768 (NaN counts as
    -32768), ties go to the smaller state.  The emissions are the caller's: a step whose four emissions are all ``-inf`` makes
    the score -inf and the path arbitrary (the tie rule's)."""
    name = "decode_states"
    if (transitions is None) != (initial is None):
        raise ValueError(f"{name}: pass both transitions and initial, or neither")
    if transitions is None:
        transitions, initial = cyclic_transitions()
    A = np.ascontiguousarray(transitions.detach().cpu().numpy() if isinstance(transitions, torch.Tensor) else transitions, dtype=np.float32)
    pi = np.ascontiguousarray(initial.detach().cpu().numpy() if isinstance(initial, torch.Tensor) else initial, dtype=np.float32)
    if A.shape != (4, 4) or pi.shape != (4,):
        raise ValueError(f"{name}: transitions (4, 4) and initial (4,) expected, got {A.shape} and {pi.shape}")
    data, offs, kind = _decode_input(name, logp)
    L = _lib.lib()
    _lib.guard_fork()
    device = data.device
    data = data.detach().contiguous()
    count = len(offs) - 1
    states = torch.empty((offs[-1],), dtype=torch.uint8, device=device)
    scores = torch.empty((count,), dtype=torch.int64, device=device) if return_scores else None
    if count:
        o = np.asarray(offs, dtype=np.int64)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _lib.check(L.hssfsst_decode_states(data.data_ptr(), o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), count,
                                               A.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), pi.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                               states.data_ptr(), scores.data_ptr() if return_scores else None, device.index, stream),
                       "hssfsst_decode_states")
    return _decode_output(logp, kind, states, offs, scores)


def decode_durations_info():
    """``(max_duration, max_steps, workspace_bytes_per_step)`` of the explicit-duration decoder
    (``hssfsst_decode_durations_info``).  No device needed."""
    D, mx, per = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().hssfsst_decode_durations_info(ctypes.byref(D), ctypes.byref(mx), ctypes.byref(per)), "hssfsst_decode_durations_info")
    return D.value, mx.value, per.value


def _host_table(name: str, what: str, v, shape=None):
    a = np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32)
    if (shape is not None and a.shape != shape) or (shape is None and (a.ndim != 2 or a.shape[0] != 4 or a.shape[1] < 1)):
        raise ValueError(f"{name}: {what} {shape if shape is not None else '(4, D)'} expected, got {a.shape}")
    return a


def edge_durations(dur):
    """The default ``edge`` table of ``decode_durations``: the running maximum of ``dur`` (4, D) from the right, so that a run
    the recording's end cuts off after d steps scores as the best run of at least d steps.  float32 numpy (4, D)."""
    d = _host_table("edge_durations", "durations", dur)
    return np.ascontiguousarray(np.maximum.accumulate(d[:, ::-1], axis=1)[:, ::-1])


def gaussian_durations(mean, std, max_duration: int, min_duration: int = 1):
    """``dur`` (4, max_duration) float32: per state the log of a normal density with the given ``mean`` and ``std`` (steps; a
    scalar or four values each), discretised at d = min_duration .. max_duration and normalised over that support; ``-inf``
    outside it."""
    D, lo = int(max_duration), int(min_duration)
    if not 1 <= lo <= D:
        raise ValueError(f"gaussian_durations: 1 <= min_duration <= max_duration expected, got {lo} and {D}")
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float64), (4,))
    std = np.broadcast_to(np.asarray(std, dtype=np.float64), (4,))
    if not (std > 0).all():
        raise ValueError("gaussian_durations: std > 0 expected")
    d = np.arange(1, D + 1, dtype=np.float64)
    logit = -0.5 * ((d[None, :] - mean[:, None]) / std[:, None]) ** 2
    logit[:, :lo - 1] = -np.inf
    top = logit.max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        out = logit - top - np.log(np.exp(logit - top).sum(axis=1, keepdims=True))
    return out.astype(np.float32)


def durations_from_labels(labels, max_duration: int, fit: str = "gaussian"):
    """``dur`` (4, max_duration) float32 from the INTERIOR runs of label sequences (a list of 1-D integer tensors or arrays with
    values 0..3): the first and the last run of every sequence are cut off by its ends (censored) and left out.
    ``fit="gaussian"``: ``gaussian_durations`` of each state's mean and standard deviation (population; at least half a step);
    ``fit="histogram"``: the log of the relative frequencies, ``-inf`` where never seen.  A run longer than ``max_duration`` or
    a state without an interior run raises ValueError."""
    D = int(max_duration)
    if fit not in ("gaussian", "histogram"):
        raise ValueError(f"durations_from_labels: fit 'gaussian' or 'histogram' expected, got {fit!r}")
    seen = [[] for _ in range(4)]
    for k, lab in enumerate(labels):
        a = lab.detach().cpu().numpy() if isinstance(lab, torch.Tensor) else np.asarray(lab)
        if a.ndim != 1 or a.size < 1 or a.dtype.kind not in "iu":
            raise ValueError(f"durations_from_labels: item {k} is not a non-empty 1-D integer sequence")
        a = a.astype(np.int64)
        if a.min() < 0 or a.max() > 3:
            raise ValueError(f"durations_from_labels: item {k} has labels outside 0..3")
        cut = np.flatnonzero(np.diff(a)) + 1
        starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [a.size]])
        for s, e in list(zip(starts, ends))[1:-1]:
            if e - s > D:
                raise ValueError(f"durations_from_labels: item {k} has a run of {e - s} steps, over max_duration {D}")
            seen[a[s]].append(int(e - s))
    if any(not r for r in seen):
        raise ValueError(f"durations_from_labels: state {[i for i, r in enumerate(seen) if not r][0]} has no interior run")
    if fit == "gaussian":
        return gaussian_durations([np.mean(r) for r in seen], [max(np.std(r), 0.5) for r in seen], D)
    out = np.full((4, D), -np.inf, dtype=np.float64)
    for j, r in enumerate(seen):
        counts = np.bincount(np.asarray(r), minlength=D + 1)[1:].astype(np.float64)
        with np.errstate(divide="ignore"):
            out[j] = np.log(counts / counts.sum())
    return out.astype(np.float32)


def durations_from_counts(counts, fit: str = "gaussian"):
    """The M-step to ``duration_posteriors(..., return_counts=True)``'s E-step, mirroring ``durations_from_labels``: ``dur``
    (4, D) float32 from expected run-length counts ``(4, D)``, or ``(2, 4, D)`` of which the INTERIOR table ``counts[0]`` is used
    (the first and the last run of a recording are cut off by its ends) -- sum the counts of a corpus over its recordings first.
    A tensor or an array; negative entries (rounding) count as 0.  ``fit="gaussian"``: ``gaussian_durations`` of each state's mean
    and standard deviation of d under its counts (population; at least half a step); ``fit="histogram"``: the log of the relative
    mass, ``-inf`` where there is none.  A state without mass raises ValueError.  The scores are not a normalised generative
    model: iterating this with the E-step is the caller's loop, and no convergence is promised."""
    if fit not in ("gaussian", "histogram"):
        raise ValueError(f"durations_from_counts: fit 'gaussian' or 'histogram' expected, got {fit!r}")
    c = np.asarray(counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else counts, dtype=np.float64)
    if c.ndim == 3 and c.shape[0] == 2:
        c = c[0]
    if c.ndim != 2 or c.shape[0] != 4 or c.shape[1] < 1:
        raise ValueError(f"durations_from_counts: counts (4, D) or (2, 4, D) expected, got {c.shape}")
    if np.isnan(c).any():
        raise ValueError("durations_from_counts: counts hold NaN")
    c = np.maximum(c, 0.0)
    D = c.shape[1]
    mass = c.sum(axis=1)
    if not (mass > 0).all():
        raise ValueError(f"durations_from_counts: state {int(np.flatnonzero(~(mass > 0))[0])} has no mass")
    p = c / mass[:, None]
    if fit == "gaussian":
        d = np.arange(1, D + 1, dtype=np.float64)
        mean = (p * d).sum(axis=1)
        std = np.sqrt((p * (d[None, :] - mean[:, None]) ** 2).sum(axis=1))
        return gaussian_durations(mean, np.maximum(std, 0.5), D)
    with np.errstate(divide="ignore"):
        return np.log(p).astype(np.float32)


def decode_durations(logp, durations, transitions=None, initial=None, edge=None, return_scores: bool = False):
    """Explicit-duration (semi-Markov) Viterbi decoding on the device (``hssfsst_decode_durations``): ``decode_states`` with a
    log score ``durations[j][d - 1]`` for an interior run of state j lasting d = 1 .. D steps, D = ``durations.shape[1]`` <= 2048;
    ``-inf`` = forbidden, so no decoded run is longer than D or shorter than the table allows.  ``edge`` (4, D): the same for the
    first and the last run of a recording, which its ends cut off; default ``edge_durations(durations)``.  ``transitions``,
    ``initial``: as for ``decode_states`` (default ``cyclic_transitions()``), but the diagonal of ``transitions`` is ignored: a
    run is never followed by a run of the same state.

    ``logp`` and the result are ``decode_states``' three kinds.  One call, enqueued on the current stream; the workspace (8 bytes
    per step) is allocated here.  A recording no segmentation fits gets the score -inf and the state 0 at every step.

    Exact arithmetic (include/hssfsst.h), with one difference from ``decode_states``: an emission of ``-inf`` or NaN counts as
    -32768 instead of forbidding its state, because the decoder works on prefix sums of the emissions."""
    name = "decode_durations"
    if (transitions is None) != (initial is None):
        raise ValueError(f"{name}: pass both transitions and initial, or neither")
    if transitions is None:
        transitions, initial = cyclic_transitions()
    A, pi = _host_table(name, "transitions", transitions, (4, 4)), _host_table(name, "initial", initial, (4,))
    dur = _host_table(name, "durations", durations)
    D = dur.shape[1]
    eg = edge_durations(dur) if edge is None else _host_table(name, "edge", edge, (4, D))
    data, offs, kind = _decode_input(name, logp)
    L = _lib.lib()
    _lib.guard_fork()
    device = data.device
    data = data.detach().contiguous()
    count = len(offs) - 1
    states = torch.empty((offs[-1],), dtype=torch.uint8, device=device)
    scores = torch.empty((count,), dtype=torch.int64, device=device) if return_scores else None
    if count:
        o = np.asarray(offs, dtype=np.int64)
        per = decode_durations_info()[2]
        work = torch.empty((per * (offs[-1] + 8 * D),), dtype=torch.uint8, device=device)
        fp = ctypes.POINTER(ctypes.c_float)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _lib.check(L.hssfsst_decode_durations(data.data_ptr(), o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), count,
                                                  A.ctypes.data_as(fp), pi.ctypes.data_as(fp), dur.ctypes.data_as(fp), eg.ctypes.data_as(fp), D,
                                                  states.data_ptr(), scores.data_ptr() if return_scores else None, work.data_ptr(),
                                                  work.numel(), device.index, stream),
                       "hssfsst_decode_durations")
    return _decode_output(logp, kind, states, offs, scores)


# ------------------------------------------------------------------- log-probs -> state posteriors and the sequence loss
def posteriors_info():
    """``(segment_steps, max_steps, work_bytes_per_step, work_bytes_per_recording)`` of the forward-backward kernel
    (``hssfsst_posteriors_info``).  No device needed."""
    seg, mx, per, rec = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().hssfsst_posteriors_info(ctypes.byref(seg), ctypes.byref(mx), ctypes.byref(per), ctypes.byref(rec)),
               "hssfsst_posteriors_info")
    return seg.value, mx.value, per.value, rec.value


def _posterior_tables(name: str, transitions, initial, device):
    """``(A, pi)`` as given (default ``cyclic_transitions()``) -> the tensors ``A (4, 4)``, ``pi (4,)`` on ``device``: tensors
    already there are kept (they may carry a gradient), anything else is uploaded as float32."""
    if (transitions is None) != (initial is None):
        raise ValueError(f"{name}: pass both transitions and initial, or neither")
    if transitions is None:
        transitions, initial = cyclic_transitions()
    out = []
    for what, v, shape in (("transitions", transitions, (4, 4)), ("initial", initial, (4,))):
        if isinstance(v, torch.Tensor) and v.device == device:
            if not v.is_floating_point():
                raise ValueError(f"{name}: floating-point {what} expected, got {v.dtype}")
            t = v
        else:
            t = torch.from_numpy(np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32)).to(device)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: {what} {shape} expected, got {tuple(t.shape)}")
        out.append(t)
    return out[0], out[1]


def _posteriors_run(data, offs, a_pi, labels=None, tables_grad: bool = False):
    """One ``hssfsst_posteriors`` call on the current stream -> ``(gamma, loglik, score, xi, gamma0)``; ``score`` only with
    ``labels`` (a uint8 arena on the device), ``xi`` and ``gamma0`` only with ``tables_grad``; None otherwise."""
    L = _lib.lib()
    _lib.guard_fork()
    device = data.device
    count, total = len(offs) - 1, offs[-1]
    f64 = dict(dtype=torch.float64, device=device)
    gamma = torch.empty((total, 4), dtype=torch.float32, device=device)
    loglik = torch.empty((count,), **f64)
    score = torch.empty((count,), **f64) if labels is not None else None
    xi = torch.empty((count, 16), **f64) if tables_grad else None
    gamma0 = torch.empty((count, 4), **f64) if tables_grad else None
    if count:
        _, _, per, rec = posteriors_info()
        work = torch.empty((per * total + rec * count,), dtype=torch.uint8, device=device)
        o = np.asarray(offs, dtype=np.int64)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            _lib.check(L.hssfsst_posteriors(data.data_ptr(), o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), count, a_pi.data_ptr(),
                                            labels.data_ptr() if labels is not None else None, gamma.data_ptr(), loglik.data_ptr(),
                                            score.data_ptr() if score is not None else None, xi.data_ptr() if xi is not None else None,
                                            gamma0.data_ptr() if gamma0 is not None else None, work.data_ptr(), work.numel(),
                                            device.index, stream),
                       "hssfsst_posteriors")
    return gamma, loglik, score, xi, gamma0


def _a_pi(A: torch.Tensor, pi: torch.Tensor) -> torch.Tensor:
    return torch.cat([A.detach().reshape(16).to(torch.float32), pi.detach().reshape(4).to(torch.float32)]).contiguous()


def state_posteriors(logp, transitions=None, initial=None, return_loglik: bool = False):
    """Forward-backward on the device (``hssfsst_posteriors``): log-probs -> the per-step state posteriors ``gamma_t(j) =
    P(state_t = j | the whole recording, A, pi)`` under log transitions ``transitions`` (4, 4) and log initial scores ``initial``
    (4,); ``-inf`` = forbidden; default ``cyclic_transitions()``.  The smoothed counterpart of ``decode_states``' path: a score
    per step and state that respects the cardiac cycle (per-class AUROC, a confidence for a decoded path).

    ``logp``: ``decode_states``' three kinds.  Returns the same kind in float32: a ``RaggedFeatures`` of ``(T_i, 4)``, a
    ``(B, T, 4)`` or a ``(T, 4)`` tensor.  ``return_loglik=True``: also ``logZ``, float64 ``(B,)`` ON THE DEVICE (a 0-d tensor for
    ``(T, 4)``): nothing here waits for the device.  One call, enqueued on the current stream.  Not differentiable (see
    ``sequence_nll``).  The tables may be numpy arrays or tensors; those on the host are uploaded.

    float64 inside, scaled by exact powers of two (include/hssfsst.h): a path more than ~700 nats below the best one reaching the
    same step is dropped; NaN emissions count as ``-inf``; a recording no path fits gets ``logZ = -inf`` and ``gamma = 0``."""
    name = "state_posteriors"
    data, offs, kind = _decode_input(name, logp)
    A, pi = _posterior_tables(name, transitions, initial, data.device)
    gamma, loglik, _, _, _ = _posteriors_run(data.detach().contiguous(), offs, _a_pi(A, pi))
    if kind == "ragged":
        out = RaggedFeatures(gamma, torch.tensor(offs, dtype=torch.int64), 4, False)
    elif kind == "batch":
        out = gamma.view(int(logp.shape[0]), int(logp.shape[1]), 4)
    else:
        out = gamma
    if not return_loglik:
        return out
    return out, (loglik[0] if kind == "single" else loglik)


def _nll_labels(name: str, labels, offs, kind: str, device) -> torch.Tensor:
    """The labels of ``sequence_nll`` -> one uint8 arena ``(sum T,)`` on ``device``.  Lengths are checked always; values are
    checked (0..3) where the labels are on the HOST -- labels on the device are not read back (no synchronisation): the kernel
    looks at their two low bits only."""
    total, count = offs[-1], len(offs) - 1

    def values(t, what):
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError(f"{name}: {what}: integer labels expected")
        if t.device.type == "cpu" and t.numel() and (int(t.min()) < 0 or int(t.max()) > 3):
            raise ValueError(f"{name}: {what} has labels outside 0..3")
        return t

    if isinstance(labels, RaggedFeatures):
        if [int(o) for o in labels._off] != list(offs) or labels.data.dim() != 1:
            raise ValueError(f"{name}: the labels' offsets do not match the log-probs'")
        arena = values(labels.data, "labels")
    elif isinstance(labels, (list, tuple)):
        if len(labels) != count:
            raise ValueError(f"{name}: {len(labels)} label sequences for {count} recordings")
        items = []
        for i, lab in enumerate(labels):
            t = values(lab, f"item {i}")
            if t.dim() != 1 or t.shape[0] != offs[i + 1] - offs[i]:
                raise ValueError(f"{name}: item {i} has labels of shape {tuple(t.shape)} for {offs[i + 1] - offs[i]} steps")
            items.append(t.to(device=device, dtype=torch.uint8))
        arena = torch.cat(items) if items else torch.empty((0,), dtype=torch.uint8, device=device)
    else:
        t = values(labels, "labels")
        if kind == "batch" and t.dim() == 2 and t.shape[0] == count and t.shape[0] * t.shape[1] == total:
            arena = t.reshape(total)
        elif t.dim() == 1 and t.shape[0] == total:
            arena = t
        else:
            raise ValueError(f"{name}: labels of shape {tuple(t.shape)} do not match {count} recordings of {total} steps in all")
    return arena.to(device=device, dtype=torch.uint8).contiguous()


class _SequenceNLL(torch.autograd.Function):
    """``(B,)`` float64 ``logZ - score(labels)`` from one ``hssfsst_posteriors`` call; the backward is a scale of what that call
    left: ``gamma - onehot``, ``Xi - counts``, ``gamma_0 - onehot_0``."""

    @staticmethod
    def forward(ctx, data, A, pi, labels, offs):
        tables_grad = A.requires_grad or pi.requires_grad
        gamma, loglik, score, xi, gamma0 = _posteriors_run(data.detach().contiguous(), offs, _a_pi(A, pi), labels, tables_grad)
        ctx.offs = offs
        ctx.tables_grad = tables_grad
        ctx.dtypes = (A.dtype, pi.dtype)
        ctx.save_for_backward(gamma, xi, gamma0, torch.isinf(A.detach()), torch.isinf(pi.detach()))
        return loglik - score

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gamma, xi, gamma0, a_forbidden, pi_forbidden = ctx.saved_tensors
        offs = ctx.offs
        g = g.to(torch.float64)
        d_data = d_A = d_pi = None
        if ctx.needs_input_grad[0]:
            lens = torch.tensor([offs[i + 1] - offs[i] for i in range(len(offs) - 1)], dtype=torch.int64).to(g.device, non_blocking=True)
            per_step = torch.repeat_interleave(g, lens, output_size=offs[-1])
            d_data = (gamma.to(torch.float64) * per_step[:, None]).to(torch.float32)
        if ctx.tables_grad and ctx.needs_input_grad[1]:
            d_A = (xi * g[:, None]).sum(dim=0).view(4, 4).masked_fill(a_forbidden, 0.0).to(ctx.dtypes[0])
        if ctx.tables_grad and ctx.needs_input_grad[2]:
            d_pi = (gamma0 * g[:, None]).sum(dim=0).masked_fill(pi_forbidden, 0.0).to(ctx.dtypes[1])
        return d_data, d_A, d_pi, None, None


def sequence_nll(logp, labels, transitions=None, initial=None, reduction: str = "mean"):
    """The linear-chain sequence loss ``logZ - score(labels)`` under the transition model the segmenter is decoded with
    (``hssfsst_posteriors``): the negative log-probability of the whole label sequence given ``A``, ``pi`` and the emissions,
    where the per-step ``nll_loss`` never tells the network that impossible sequences cost nothing at inference.

    ``logp``: ``decode_states``' three kinds (the arena of a ``RaggedFeatures`` may carry a gradient: ``HipSegmenterHead.ragged``).
    ``labels``: a list of 1-D integer tensors (one per recording), a ``RaggedStates`` or a uint8 arena ``(sum T,)`` with matching
    offsets, or a ``(B, T)`` / ``(T,)`` tensor.  Mismatched lengths raise ValueError; values outside 0..3 raise ValueError where
    the labels are on the host -- labels on the device are not read back (that would wait for the device) and only their two low
    bits count.  ``reduction``: ``"mean"`` = ``sum_i nll_i / sum_i T_i``, per step and so comparable with ``nll_loss``; ``"sum"``;
    ``"none"`` = ``(B,)``.  The value is float64, cast to float32 for ``"mean"`` and ``"sum"``.

    Differentiable (once) in ``logp`` and, where they are tensors on the log-probs' device that require grad, in ``transitions``
    and ``initial``: ``gamma - onehot(y)``, ``Xi - counts(y)`` and ``gamma_0 - onehot(y_0)`` times the incoming gradient and the
    reduction's factor; forbidden (``-inf``) entries of the tables get gradient 0.  The forward is one kernel call; the backward
    launches no recurrence.  The tables reach the kernel in float32 whatever their dtype."""
    name = "sequence_nll"
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"{name}: reduction 'mean', 'sum' or 'none' expected, got {reduction!r}")
    data, offs, kind = _decode_input(name, logp)
    A, pi = _posterior_tables(name, transitions, initial, data.device)
    arena = _nll_labels(name, labels, offs, kind, data.device)
    nll = _SequenceNLL.apply(data, A, pi, arena, offs)
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum().to(torch.float32)
    return (nll.sum() / max(offs[-1], 1)).to(torch.float32)


# ------------------------------------------------- log-probs -> posteriors and the sequence loss under duration scores
def duration_posteriors_info():
    """``(max_duration, segment_steps, max_steps, work_bytes_per_step, work_bytes_per_recording, work_bytes_per_duration)`` of the
    explicit-duration forward-backward kernel (``hssfsst_posteriors_durations_info``).  No device needed."""
    D, seg = ctypes.c_int(0), ctypes.c_int(0)
    mx, per, rec, dur = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().hssfsst_posteriors_durations_info(ctypes.byref(D), ctypes.byref(seg), ctypes.byref(mx), ctypes.byref(per),
                                                            ctypes.byref(rec), ctypes.byref(dur)), "hssfsst_posteriors_durations_info")
    return D.value, seg.value, mx.value, per.value, rec.value, dur.value


def duration_counts_info():
    """``(work_bytes_per_step, work_bytes_per_recording, work_bytes_per_duration, durations_per_group)`` of the run-length counts
    call (``hssfsst_posteriors_durations_counts_info``); the other limits are ``duration_posteriors_info()``'s.  No device needed."""
    per, rec, dur, grp = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0)
    _lib.check(_lib.lib().hssfsst_posteriors_durations_counts_info(ctypes.byref(per), ctypes.byref(rec), ctypes.byref(dur), ctypes.byref(grp)),
               "hssfsst_posteriors_durations_counts_info")
    return per.value, rec.value, dur.value, grp.value


def _learnable_duration_tables(name: str, durations, edge, device):
    """``duration_nll(learn_durations=True)``: both tables are given as ``(4, D)`` tensors on ``device``, float32 or float64, and
    either may require grad; they are returned as they are (the autograd function rounds them to float32 for the kernel)."""
    for what, v in (("durations", durations), ("edge", edge)):
        if not isinstance(v, torch.Tensor) or v.device != device or v.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{name}: with learn_durations, {what} must be a float32 or float64 tensor on {device}"
                             + (" (no default edge is made: tie it to durations in torch if that is wanted)" if v is None else ""))
    if durations.dim() != 2 or durations.shape[0] != 4 or durations.shape[1] < 1:
        raise ValueError(f"{name}: durations (4, D) expected, got {tuple(durations.shape)}")
    D = int(durations.shape[1])
    if tuple(edge.shape) != (4, D):
        raise ValueError(f"{name}: edge {(4, D)} expected, got {tuple(edge.shape)}")
    if D > duration_posteriors_info()[0]:
        raise ValueError(f"{name}: max_duration {D} is over the limit of {duration_posteriors_info()[0]}")
    return durations, edge


def _duration_tables(name: str, durations, edge, device):
    """``dur``, ``edge`` (default ``edge_durations(dur)``) -> two contiguous float32 ``(4, D)`` tensors on ``device``.  They are
    constants of the model: one that requires grad raises ValueError."""
    for what, v in (("durations", durations), ("edge", edge)):
        if isinstance(v, torch.Tensor) and v.requires_grad:
            raise ValueError(f"{name}: {what} requires grad, but the duration tables are constants: there is no gradient in them")
    if isinstance(durations, torch.Tensor) and durations.device == device and edge is not None:
        dur = durations.detach().to(torch.float32).contiguous()
        if dur.dim() != 2 or dur.shape[0] != 4 or dur.shape[1] < 1:
            raise ValueError(f"{name}: durations (4, D) expected, got {tuple(dur.shape)}")
    else:
        host = _host_table(name, "durations", durations)
        if edge is None:
            edge = edge_durations(host)
        dur = torch.from_numpy(host).to(device)
    D = int(dur.shape[1])
    if isinstance(edge, torch.Tensor) and edge.device == device:
        eg = edge.detach().to(torch.float32).contiguous()
        if tuple(eg.shape) != (4, D):
            raise ValueError(f"{name}: edge {(4, D)} expected, got {tuple(eg.shape)}")
    else:
        eg = torch.from_numpy(_host_table(name, "edge", edge, (4, D))).to(device)
    if D > duration_posteriors_info()[0]:
        raise ValueError(f"{name}: max_duration {D} is over the limit of {duration_posteriors_info()[0]}")
    return dur, eg


def _duration_posteriors_run(data, offs, a_pi, dur, edge, labels=None, tables_grad: bool = False, want_onsets: bool = False,
                             want_counts: bool = False):
    """One ``hssfsst_posteriors_durations`` call on the current stream -> ``(gamma, loglik, score, xi, s0, onsets, counts)``;
    ``score`` only with ``labels`` (a uint8 arena on the device), ``xi`` and ``s0`` only with ``tables_grad``, ``onsets`` only when
    wanted; None otherwise.  ``want_counts``: one ``hssfsst_posteriors_durations_counts`` call instead, and ``counts``
    ``(count, 2, 4, D)`` float64."""
    L = _lib.lib()
    _lib.guard_fork()
    device = data.device
    count, total, D = len(offs) - 1, offs[-1], int(dur.shape[1])
    f64 = dict(dtype=torch.float64, device=device)
    gamma = torch.empty((total, 4), dtype=torch.float32, device=device)
    onsets = torch.empty((total, 4), dtype=torch.float32, device=device) if want_onsets else None
    loglik = torch.empty((count,), **f64)
    score = torch.empty((count,), **f64) if labels is not None else None
    xi = torch.empty((count, 16), **f64) if tables_grad else None
    s0 = torch.empty((count, 4), **f64) if tables_grad else None
    counts = torch.empty((count, 2, 4, D), **f64) if want_counts else None
    if count:
        per, rec, per_d = duration_counts_info()[:3] if want_counts else duration_posteriors_info()[3:]
        work = torch.empty((per * total + rec * count + per_d * D,), dtype=torch.uint8, device=device)
        o = np.asarray(offs, dtype=np.int64)
        opt = lambda t: t.data_ptr() if t is not None else None       # noqa: E731
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream(device).cuda_stream
            head = (data.data_ptr(), o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), count, a_pi.data_ptr(), dur.data_ptr(), edge.data_ptr(), D,
                    opt(labels), gamma.data_ptr(), opt(onsets), loglik.data_ptr(), opt(score), opt(xi), opt(s0))
            tail = (work.data_ptr(), work.numel(), device.index, stream)
            if want_counts:
                _lib.check(L.hssfsst_posteriors_durations_counts(*head, counts.data_ptr(), *tail), "hssfsst_posteriors_durations_counts")
            else:
                _lib.check(L.hssfsst_posteriors_durations(*head, *tail), "hssfsst_posteriors_durations")
    return gamma, loglik, score, xi, s0, onsets, counts


def duration_posteriors(logp, durations, transitions=None, initial=None, edge=None, return_loglik: bool = False,
                        return_onsets: bool = False, return_counts: bool = False):
    """Forward-backward under the explicit-duration (semi-Markov) model of ``decode_durations``
    (``hssfsst_posteriors_durations``): log-probs -> ``gamma_t(j) = P(state_t = j | the whole recording, the tables)``, summed over
    every segmentation into runs of 1 .. D steps that ``decode_durations`` picks the best of.  ``durations`` (4, D), ``edge``
    (default ``edge_durations(durations)``), ``transitions`` (diagonal ignored), ``initial``: as for ``decode_durations``; numpy
    arrays or tensors, those on the host are uploaded; none is read back, except a ``durations`` on the device given without an
    ``edge``, from which the default ``edge`` is made on the host.

    ``logp``: ``decode_states``' three kinds.  Returns the same kind in float32, like ``state_posteriors``.
    ``return_loglik=True``: also ``logZ``, float64 ``(B,)`` on the device (0-d for ``(T, 4)``).  ``return_onsets=True``: also the
    run-onset posteriors ``S_t(j) = P(a run of j starts at step t)`` in the kind of ``gamma`` -- where the S1 onset is, and how
    sure.  ``return_counts=True`` (``hssfsst_posteriors_durations_counts``): also the expected run-length counts, float64
    ``(B, 2, 4, D)`` on the device (``(2, 4, D)`` for ``(T, 4)``): ``counts[.., 0, j, d - 1]`` = the expected number of interior runs
    of state j lasting exactly d steps, ``counts[.., 1, j, d - 1]`` the same for the first and the last run -- the gradients of logZ
    in ``durations`` and ``edge``, and what ``durations_from_counts`` fits a new table to; 64 D bytes per recording (128 KiB at
    D = 2048).  The order is ``(gamma[, logZ][, onsets][, counts])``.  One call on the current stream, nothing waits for the
    device.  Not differentiable (see ``duration_nll``).

    float64 mantissas with integer exponents inside (include/hssfsst.h): nothing underflows, the prefix sums of the emissions must
    stay within +-3.7e8, and the relative error grows with them (x 2^-53).  An emission of ``-inf`` or NaN counts as -32768, as in
    ``decode_durations``; a recording no segmentation fits gets ``logZ = -inf`` and ``gamma = 0``."""
    name = "duration_posteriors"
    data, offs, kind = _decode_input(name, logp)
    A, pi = _posterior_tables(name, transitions, initial, data.device)
    dur, eg = _duration_tables(name, durations, edge, data.device)
    gamma, loglik, _, _, _, onsets, counts = _duration_posteriors_run(data.detach().contiguous(), offs, _a_pi(A, pi), dur, eg,
                                                                      want_onsets=return_onsets, want_counts=return_counts)

    def shaped(t):
        if kind == "ragged":
            return RaggedFeatures(t, torch.tensor(offs, dtype=torch.int64), 4, False)
        return t.view(int(logp.shape[0]), int(logp.shape[1]), 4) if kind == "batch" else t
    out = [shaped(gamma)]
    if return_loglik:
        out.append(loglik[0] if kind == "single" else loglik)
    if return_onsets:
        out.append(shaped(onsets))
    if return_counts:
        out.append(counts[0] if kind == "single" else counts)
    return out[0] if len(out) == 1 else tuple(out)


class _DurationNLL(torch.autograd.Function):
    """``(B,)`` float64 ``logZ - score(labels)`` from one ``hssfsst_posteriors_durations`` call; the backward is a scale of what
    that call left: ``gamma - onehot``, ``Xi - counts(label runs)``, ``S_0 - onehot_0`` and, where a duration table requires grad
    (``learn_durations``), the run-length counts less the label runs' (``hssfsst_posteriors_durations_counts``)."""

    @staticmethod
    def forward(ctx, data, A, pi, dur, edge, labels, offs):
        tables_grad = A.requires_grad or pi.requires_grad
        durations_grad = dur.requires_grad or edge.requires_grad
        d32, e32 = (t.detach().to(torch.float32).contiguous() for t in (dur, edge))
        gamma, loglik, score, xi, s0, _, counts = _duration_posteriors_run(data.detach().contiguous(), offs, _a_pi(A, pi), d32, e32, labels,
                                                                           tables_grad, want_counts=durations_grad)
        ctx.offs = offs
        ctx.tables_grad = tables_grad
        ctx.durations_grad = durations_grad
        ctx.dtypes = (A.dtype, pi.dtype, dur.dtype, edge.dtype)
        forbidden = torch.isinf(A.detach()) | torch.eye(4, dtype=torch.bool, device=A.device)      # (the diagonal is never read)
        none = torch.isinf(torch.stack([d32, e32])) if durations_grad else None
        ctx.save_for_backward(gamma, xi, s0, forbidden, torch.isinf(pi.detach()), counts, none)
        return loglik - score

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gamma, xi, s0, a_forbidden, pi_forbidden, counts, dur_forbidden = ctx.saved_tensors
        offs = ctx.offs
        g = g.to(torch.float64)
        d_data = d_A = d_pi = d_dur = d_edge = None
        if ctx.needs_input_grad[0]:
            lens = torch.tensor([offs[i + 1] - offs[i] for i in range(len(offs) - 1)], dtype=torch.int64).to(g.device, non_blocking=True)
            per_step = torch.repeat_interleave(g, lens, output_size=offs[-1])
            d_data = (gamma.to(torch.float64) * per_step[:, None]).to(torch.float32)
        if ctx.tables_grad and ctx.needs_input_grad[1]:
            d_A = (xi * g[:, None]).sum(dim=0).view(4, 4).masked_fill(a_forbidden, 0.0).to(ctx.dtypes[0])
        if ctx.tables_grad and ctx.needs_input_grad[2]:
            d_pi = (s0 * g[:, None]).sum(dim=0).masked_fill(pi_forbidden, 0.0).to(ctx.dtypes[1])
        if ctx.durations_grad and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4]):
            both = (counts * g[:, None, None, None]).sum(dim=0).masked_fill(dur_forbidden, 0.0)
            if ctx.needs_input_grad[3]:
                d_dur = both[0].to(ctx.dtypes[2])
            if ctx.needs_input_grad[4]:
                d_edge = both[1].to(ctx.dtypes[3])
        return d_data, d_A, d_pi, d_dur, d_edge, None, None


def duration_nll(logp, labels, durations, transitions=None, initial=None, edge=None, reduction: str = "mean",
                 learn_durations: bool = False):
    """The semi-Markov sequence loss ``logZ - score(labels)`` under the model ``decode_durations`` decodes with
    (``hssfsst_posteriors_durations``): the negative log-probability of the labelled segmentation -- the runs of equal labels --
    given the tables and the emissions.  Where ``sequence_nll`` trains against a first-order chain, under which the decoder's
    minimum run costs nothing, this one trains against the duration scores.  ``+inf`` where a labelled run is longer than D or
    forbidden by a table.

    ``logp``, ``labels``, ``reduction`` and the value's dtype: as for ``sequence_nll``.  ``durations``, ``edge``, ``transitions``,
    ``initial``: as for ``duration_posteriors``.  Differentiable (once) in ``logp`` and, where they are tensors on the log-probs'
    device that require grad, in ``transitions`` (the diagonal and forbidden entries get gradient 0) and ``initial``.  By default
    the duration tables are constants: a ``durations`` or ``edge`` that requires grad raises ValueError.

    ``learn_durations=True``: ``durations`` and ``edge`` are both given as ``(4, D)`` tensors on the log-probs' device, float32 or
    float64, and either may require grad (no default ``edge`` is made: tie it to ``durations`` in torch if that is wanted, e.g.
    ``edge=torch.flip(torch.cummax(torch.flip(dur, [1]), 1).values, [1])``).  Their gradients are the expected run-length counts
    less the label runs' (``duration_posteriors(return_counts=True)``), in the table's dtype, 0 at ``-inf`` entries; the kernel
    sees the tables rounded to float32.  The forward is then the counts call, which costs 64 D bytes per recording.

    The forward is one call; the backward launches nothing beyond scaling what the forward left."""
    name = "duration_nll"
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"{name}: reduction 'mean', 'sum' or 'none' expected, got {reduction!r}")
    data, offs, kind = _decode_input(name, logp)
    A, pi = _posterior_tables(name, transitions, initial, data.device)
    dur, eg = (_learnable_duration_tables if learn_durations else _duration_tables)(name, durations, edge, data.device)
    arena = _nll_labels(name, labels, offs, kind, data.device)
    nll = _DurationNLL.apply(data, A, pi, dur, eg, arena, offs)
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum().to(torch.float32)
    return (nll.sum() / max(offs[-1], 1)).to(torch.float32)


def state_runs(states: torch.Tensor):
    """The boundaries of a decoded recording: ``(starts int64, state uint8)`` of the runs of equal states in the 1-D ``states``
    (``torch.unique_consecutive``), on its device.  Run k covers steps ``starts[k] .. starts[k + 1]`` (the last one to the end)."""
    if not isinstance(states, torch.Tensor) or states.dim() != 1:
        raise ValueError("state_runs: a 1-D tensor of states expected")
    vals, counts = torch.unique_consecutive(states, return_counts=True)
    starts = torch.cumsum(counts, 0) - counts
    return starts.to(torch.int64), vals.to(torch.uint8)
