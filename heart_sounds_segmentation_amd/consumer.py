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
hssfsst_segmenter_exec_ragged) in one call, or window by window, as the reference trains its model, through
``segment_windowed(fsst, head.hip(), recordings)``, which stitches the windows' log-probs on the device (hssfsst_stitch_windows).

``HipBiLSTM`` is one differentiable bidirectional layer on the HIP recurrences (hssfsst_bilstm_*; csrc/segmenter_train.hpp) and
``HipSegmenterHead`` the same model built from two of them: what a training script uses instead of the ``nn.LSTM`` model.  Both
have a ``ragged`` form that trains on whole recordings of different lengths in one call (hssfsst_bilstm_*_ragged).

What becomes of the log-probs -- ``decode_states``, ``decode_durations``, ``state_posteriors``, ``sequence_nll``,
``duration_posteriors``, ``duration_nll`` and the helpers for their tables -- lives in ``sequence.py``; its public names are
imported here, so ``consumer.decode_states`` and the rest resolve as before.
"""
from __future__ import annotations

from typing import Optional

import ctypes

import numpy as np
import torch
from torch import nn

from . import _lib
from .framing import cover_starts
from .sequence import (RaggedStates, SegmentationScores, cyclic_transitions, decode_durations, decode_durations_info, decode_info, decode_states,  # noqa: F401
                       duration_counts_info, duration_nll, duration_posteriors, duration_posteriors_info, durations_from_counts,
                       durations_from_labels, edge_durations, gaussian_durations, posteriors_info, score_info, segmentation_scores,
                       sequence_nll, state_posteriors, state_runs, stitch_windows, transitions_from_labels, window_weights)
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
        # (from pinned memory and not blocking: a pageable copy would make the host wait for everything queued on the stream)
        edges = torch.from_numpy(offs).pin_memory().to(x.device, non_blocking=True)
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
    _check_route("segment_recordings", decode, durations, posteriors)
    return _route(seg.ragged(fsst.ragged(recordings), **kw), decode, durations, posteriors)


def _check_route(name: str, decode, durations, posteriors) -> None:
    """What ``decode``, ``durations`` and ``posteriors`` may be together, said before any work."""
    want_post = not (posteriors is None or posteriors is False)
    want_decode = not (decode is None or decode is False)
    if want_post and want_decode:
        raise ValueError(f"{name}: posteriors and decode exclude each other: one call returns one of them")
    if durations is not None and not (want_decode or want_post):
        raise ValueError(f"{name}: durations are for decoding or posteriors: pass decode=True, decode=(A, pi), "
                         "posteriors=True or posteriors=(A, pi) with them")


def _route(logp: RaggedFeatures, decode, durations, posteriors):
    """The log-probs of a list of recordings, on to the decoder or the posteriors that was asked for, or as they are."""
    want_post = not (posteriors is None or posteriors is False)
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


def segment_windowed(fsst, seg: HipSegmenter, recordings, stride: int = 1000, n: int = 2000, weights="triangular", mode: str = "prob",
                     h0: Optional[torch.Tensor] = None, c0: Optional[torch.Tensor] = None, max_windows: int = 1024, decode=None,
                     durations=None, posteriors=None, return_dissent: bool = False):
    """Whole recordings of different lengths (a list of 1-D signals on the GPU), segmented WINDOW BY WINDOW as the reference
    trains its model -- every ``n``-sample window z-scored on its own and started from its own initial state -- and stitched back
    into one ``RaggedFeatures`` of ``(T_i, 4)`` log-probs on the device.  This is the way to run a reference-trained checkpoint on
    a whole recording; ``segment_recordings`` z-scores the recording as one signal and walks one recurrence over all of it, so the
    two differ by design.

    The windows are ``framing.cover_starts(T_i, stride, n)``: they cover every sample (``frame_starts``, the training set, drops
    the tail).  The recordings are packed into one buffer; every full window of every recording goes through ``fsst.frames`` and
    ``seg(...)`` in chunks of at most ``max_windows`` windows (the result does not depend on it: a window's row does not depend
    on its batch); the recordings shorter than ``n`` go through ``fsst.ragged`` and ``seg.ragged`` as one window each; both
    results are laid into one window arena and stitched by ``stitch_windows`` under ``weights`` (a ``window_weights`` kind, None,
    or ``(n,)`` weights) and ``mode``.  ``h0`` / ``c0``: ``(2, 1, H)``, the state every window starts from; omitted, the module's
    own are used when their batch is 1, else ValueError.  ``decode``, ``durations``, ``posteriors``: as for ``segment_recordings``,
    through the same functions.  ``return_dissent``: also ``stitch_windows``' per-step count of disagreeing windows, second."""
    name = "segment_windowed"
    _check_route(name, decode, durations, posteriors)
    n, stride, max_windows = int(n), int(stride), int(max_windows)
    if n < 1 or not 1 <= stride <= n:
        raise ValueError(f"{name}: n >= 1 and 1 <= stride <= n expected, got n {n} and stride {stride}")
    if max_windows < 1:
        raise ValueError(f"{name}: max_windows {max_windows} must be positive")
    recs = []
    for i, x in enumerate(recordings):
        if isinstance(x, torch.Tensor) and x.dim() == 2 and x.shape[1] == 1:
            x = x[:, 0]
        if not isinstance(x, torch.Tensor) or x.dim() != 1 or x.shape[0] < 1 or x.is_complex():
            raise ValueError(f"{name}: recording {i} is not a real 1-D tensor with at least one sample")
        if x.device != seg.device:
            raise ValueError(f"{name}: recording {i} on {x.device}, the plan on {seg.device}")
        recs.append(x.detach().to(torch.float32))
    H = seg.hidden_size
    if (h0 is None) != (c0 is None):
        raise ValueError(f"{name}: pass both h0 and c0, or neither")
    if h0 is None:
        if seg.h0.shape[1] != 1:
            raise ValueError(f"{name}: every window starts from one state, but the module's h0 / c0 were made for batch {seg.h0.shape[1]} "
                             "(pass h0 and c0 of shape (2, 1, H) to the call)")
        h0, c0 = seg.h0, seg.c0
    elif tuple(h0.shape) != (2, 1, H) or tuple(c0.shape) != (2, 1, H):
        raise ValueError(f"{name}: h0 and c0 of shape {(2, 1, H)} expected, got {tuple(h0.shape)} and {tuple(c0.shape)}")
    h0 = h0.detach().to(seg.device, torch.float32).contiguous()
    c0 = c0.detach().to(seg.device, torch.float32).contiguous()
    if isinstance(weights, str):
        weights = window_weights(n, weights, seg.device)
    lens = [int(x.shape[0]) for x in recs]
    at = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    full = [i for i, T in enumerate(lens) if T >= n]
    short = [i for i, T in enumerate(lens) if T < n]
    first = np.zeros(len(recs), dtype=np.int64)
    starts, row = [], 0
    for i in full:
        first[i] = row
        starts.append(cover_starts(lens[i], stride, n)[0] + at[i])
        row += n * int(starts[-1].shape[0])
    starts = np.concatenate(starts) if starts else np.zeros(0, dtype=np.int64)
    for i in short:
        first[i] = row
        row += lens[i]
    parts = []
    if full:
        buf = torch.cat(recs) if len(recs) > 1 else recs[0].contiguous()
        for a in range(0, int(starts.shape[0]), max_windows):
            chunk = starts[a:a + max_windows]
            B = int(chunk.shape[0])
            parts.append(seg(fsst.frames(buf, chunk, n), h0.expand(2, B, H), c0.expand(2, B, H)).view(B * n, 4))
    if short:
        parts.append(seg.ragged(fsst.ragged([recs[i] for i in short]), h0, c0).data)
    win = (torch.cat(parts) if len(parts) > 1 else parts[0]) if parts else torch.empty((0, 4), dtype=torch.float32, device=seg.device)
    out = stitch_windows(win, first, lens, n, stride, weights=weights, mode=mode, return_dissent=return_dissent)
    if return_dissent:
        return _route(out[0], decode, durations, posteriors), out[1]
    return _route(out, decode, durations, posteriors)
