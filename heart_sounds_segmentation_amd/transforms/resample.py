"""Mirror of ``hss.transforms.Resample`` (/root/reference/hss/transforms/resample.py:5-21).

The reference's transform is ``torch.tensor(scipy.signal.resample(x.cpu(), self.num), dtype=dtype)``: Fourier-method
resampling to a fixed number of samples.  The dataset applies it to the label vector of a recording when a
``Resample`` is found in the transform chain (hss/datasets/heart_sounds.py:202-207: ``round(t(y)) - 1``).  Here the
arithmetic is the library's host helper ``hssfsst_resample`` (csrc/fourier_resample.hpp, fp64, any length); scipy is
not imported.  Same constructor, same call signature, same output type (a fresh CPU tensor of ``dtype``).

Extensions, mirroring ``FSST``: ``Resample(num, device=...)`` computes ``__call__`` on that GPU (still a fresh CPU tensor of
``dtype``); ``batch`` / ``frames`` resample many signals at once on the device (``hssfsst_resample_exec``,
csrc/fourier_resample_gpu.hpp: fp64 on the device whatever the dtypes), reading overlapping frames in place; and
``resample_labels_batch`` is the dataset's label rule for a batch, on the device.  ``ragged`` / ``resample_labels_ragged`` do the
same for signals of different lengths in one call (``hssfsst_resample_exec_ragged``, csrc/fourier_resample_ragged.hpp: one ragged
plan per (process, device, num); the forward tables of every length are made on the device).  Without ``device`` the call is the
host helper, as before.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np
import torch

from .. import _lib


class _ResamplePlan:
    """Owner of one ``hssfsst_resample_plan*`` for (device, n, num), created lazily in the calling process (fork-safe)."""

    def __init__(self, device_index: int, n: int, num: int):
        _lib.guard_fork()
        L = _lib.lib()
        self._L = L
        self.handle = ctypes.c_void_p()
        _lib.check(L.hssfsst_resample_plan_create(ctypes.byref(self.handle), int(device_index), int(n), int(num)),
                   "hssfsst_resample_plan_create")
        m1, m2, lds, dev = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(L.hssfsst_resample_plan_info(self.handle, None, None, ctypes.byref(m1), ctypes.byref(m2), ctypes.byref(lds),
                                                ctypes.byref(dev)), "hssfsst_resample_plan_info")
        self.n, self.num, self.m1, self.m2, self.lds_tier, self.device = int(n), int(num), m1.value, m2.value, bool(lds.value), dev.value
        self.pid = os.getpid()

    def exec(self, x: torch.Tensor, x_len: int, x_stride: int, starts: Optional[torch.Tensor], batch: int,
             y: Optional[torch.Tensor], labels: Optional[torch.Tensor]) -> None:
        """x: float32 / float64 samples (its data pointer is the buffer's start); y / labels on x's side (host or device)."""
        on_dev = x.is_cuda
        stream = torch.cuda.current_stream(self.device).cuda_stream     # (host buffers too: staged and waited for on this stream)
        ydt = _lib.DTYPE_F64 if (y is not None and y.dtype == torch.float64) else _lib.DTYPE_F32
        rc = self._L.hssfsst_resample_exec(
            self.handle, ctypes.c_void_p(x.data_ptr()), _lib.DTYPE_F64 if x.dtype == torch.float64 else _lib.DTYPE_F32,
            int(x_len), int(x_stride), ctypes.c_void_p(starts.data_ptr()) if starts is not None else None,
            1 if (starts is not None and starts.is_cuda) else 0, int(batch), 1 if on_dev else 0,
            ctypes.c_void_p(y.data_ptr()) if y is not None else None, ydt,
            ctypes.c_void_p(labels.data_ptr()) if labels is not None else None, 1 if on_dev else 0,
            ctypes.c_void_p(stream) if stream else None)
        _lib.check(rc, "hssfsst_resample_exec")

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value and self.pid == os.getpid():
                self._L.hssfsst_resample_plan_destroy(self.handle)
        except Exception:
            pass


class _RaggedResamplePlan:
    """Owner of one ragged ``hssfsst_resample_plan*`` (any input lengths -> num) for (device, num), created lazily in the calling
    process (fork-safe), like ``_ResamplePlan``."""

    def __init__(self, device_index: int, num: int):
        _lib.guard_fork()
        L = _lib.lib()
        self._L = L
        self.handle = ctypes.c_void_p()
        _lib.check(L.hssfsst_resample_plan_create_ragged(ctypes.byref(self.handle), int(device_index), int(num)),
                   "hssfsst_resample_plan_create_ragged")
        self.num, self.device, self.pid = int(num), int(device_index), os.getpid()

    def exec(self, x: torch.Tensor, starts: np.ndarray, lens: np.ndarray, y: Optional[torch.Tensor],
             labels: Optional[torch.Tensor]) -> None:
        """x: one float32 / float64 buffer (host or device); starts / lens: int64 host arrays; y / labels on x's side."""
        on_dev = x.is_cuda
        stream = torch.cuda.current_stream(self.device).cuda_stream     # (host buffers too: staged and waited for on this stream)
        ydt = _lib.DTYPE_F64 if (y is not None and y.dtype == torch.float64) else _lib.DTYPE_F32
        rc = self._L.hssfsst_resample_exec_ragged(
            self.handle, ctypes.c_void_p(x.data_ptr()), _lib.DTYPE_F64 if x.dtype == torch.float64 else _lib.DTYPE_F32,
            int(x.numel()), ctypes.c_void_p(starts.ctypes.data), ctypes.c_void_p(lens.ctypes.data), int(lens.size), 1 if on_dev else 0,
            ctypes.c_void_p(y.data_ptr()) if y is not None else None, ydt,
            ctypes.c_void_p(labels.data_ptr()) if labels is not None else None, 1 if on_dev else 0,
            ctypes.c_void_p(stream) if stream else None)
        _lib.check(rc, "hssfsst_resample_exec_ragged")

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value and self.pid == os.getpid():
                self._L.hssfsst_resample_plan_destroy(self.handle)
        except Exception:
            pass


def _as_real(x) -> torch.Tensor:
    """float32 / float64 stay as they are (read in place); any other real dtype (labels: int64) becomes float64, exactly."""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    if x.is_complex():
        raise ValueError("Resample: complex input is not supported")
    x = x.detach()
    return x if x.dtype in (torch.float32, torch.float64) else x.to(torch.float64)


class Resample:
    def __init__(self, num: int, device: Optional[torch.device] = None) -> None:
        """
        Args:
            num (int): number of output samples
            device (extension): a HIP device for ``__call__``; None keeps the host helper.  ``batch`` / ``frames`` run on
                their input's device (a CPU input on this one, else the current device)
        """
        self.num = num
        self.device = device
        self._plans = {}

    def __getstate__(self):          # plans hold device handles: never pickle them into workers
        st = self.__dict__.copy()
        st["_plans"] = {}
        return st

    # ------------------------------------------------------------------ device path
    def _device_index(self, like: Optional[torch.Tensor] = None) -> int:
        _lib.guard_fork()
        if like is not None and like.is_cuda:
            return like.device.index if like.device.index is not None else torch.cuda.current_device()
        if not torch.cuda.is_available():
            raise RuntimeError("Resample: no HIP device visible (torch.cuda.is_available() is False); "
                               "the batched path has no CPU fallback")
        if getattr(self, "device", None) is not None:
            d = torch.device(self.device)
            if d.type != "cuda":
                raise RuntimeError(f"Resample: device {d} is not a HIP device; there is no CPU path")
            return d.index if d.index is not None else torch.cuda.current_device()
        return torch.cuda.current_device()

    def _plan(self, device_index: int, n: int) -> _ResamplePlan:
        num = int(self.num)
        if num < 1 or n < 1:
            raise ValueError(f"Resample: need at least one input and one output sample (n={n}, num={num})")
        if not hasattr(self, "_plans"):
            self._plans = {}
        key = (os.getpid(), device_index, int(n), num)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = _ResamplePlan(device_index, n, num)
        return plan

    def _out(self, B: int, dtype: torch.dtype, device, out: Optional[torch.Tensor]) -> torch.Tensor:
        shape = (B, int(self.num))
        if out is None:
            return torch.empty(shape, dtype=dtype, device=device)
        if tuple(out.shape) != shape or out.dtype != dtype or out.device != device or not out.is_contiguous():
            raise ValueError(f"Resample: out must be a contiguous {dtype} tensor of shape {shape} on {device}")
        return out

    def _run(self, X: torch.Tensor, dtype: torch.dtype, out: Optional[torch.Tensor], labels: bool) -> torch.Tensor:
        """X: (B, n) float32 / float64 with unit stride along n and a positive signal stride (read in place)."""
        B, n = int(X.shape[0]), int(X.shape[1])
        dev = self._device_index(X)
        plan = self._plan(dev, n)
        if labels:
            res = self._out(B, torch.int64, X.device, out)
        else:
            if dtype not in (torch.float32, torch.float64):
                raise ValueError(f"Resample.batch: dtype must be float32 or float64, got {dtype}")
            res = self._out(B, dtype, X.device, out)
        if B == 0:
            return res
        xstride = int(X.stride(0)) if B > 1 else n
        plan.exec(X, (B - 1) * xstride + n, xstride, None, B, None if labels else res, res if labels else None)
        return res

    @staticmethod
    def _frames_view(X) -> torch.Tensor:
        X = _as_real(X)
        if X.ndim == 1:
            X = X.unsqueeze(0)
        if X.ndim != 2:
            raise ValueError(f"Resample.batch: expected (B, n), got {tuple(X.shape)}")
        if X.shape[1] > 1 and X.stride(1) != 1 or (X.shape[0] > 1 and X.stride(0) < 1):
            X = X.contiguous()                            # (overlapping frames of one recording are read in place)
        return X

    def batch(self, X: torch.Tensor, dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Extension: resample ``B`` signals at once on the device.  ``X``: ``(B, n)`` float32 / float64 (other real dtypes are
        taken as float64), CPU or cuda; a view of overlapping frames (``framing.frame_batch``) is read in place.  Returns
        ``(B, num)`` of ``dtype`` (float32 / float64: the fp64 result cast) on X's device; ``out`` optionally receives it."""
        return self._run(self._frames_view(X), dtype, out, labels=False)

    def frames(self, x: torch.Tensor, starts, n: int, dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None,
               labels: bool = False) -> torch.Tensor:
        """Extension (batched dataset builder): resample the frames ``x[starts[b] : starts[b] + n]`` of ONE 1-D buffer in one call.
        ``starts``: int64 sequence / tensor (CPU, or on x's device).  Returns ``(len(starts), num)`` of ``dtype`` on x's device,
        or with ``labels=True`` the int64 label rule of ``resample_labels`` applied to every frame."""
        x = _as_real(x)
        if x.ndim != 1:
            raise ValueError(f"Resample.frames: expected one 1-D buffer, got {tuple(x.shape)}")
        x = x.contiguous()
        if not isinstance(starts, torch.Tensor):
            starts = torch.as_tensor(np.asarray(starts, dtype=np.int64))
        starts = starts.to(torch.int64).contiguous()
        if starts.ndim != 1:
            raise ValueError("Resample.frames: starts must be 1-D")
        B, T, n = int(starts.shape[0]), int(x.shape[0]), int(n)
        if n < 1 or T < n:
            raise ValueError(f"Resample.frames: frame length {n} does not fit a buffer of {T} samples")
        if starts.is_cuda and (not x.is_cuda or starts.device != x.device):
            starts = starts.cpu()
        if B and not starts.is_cuda and (int(starts.min()) < 0 or int(starts.max()) > T - n):
            raise ValueError(f"Resample.frames: a frame start lies outside [0, {T - n}]")
        dev = self._device_index(x)
        plan = self._plan(dev, n)
        if labels:
            res = self._out(B, torch.int64, x.device, out)
        else:
            if dtype not in (torch.float32, torch.float64):
                raise ValueError(f"Resample.frames: dtype must be float32 or float64, got {dtype}")
            res = self._out(B, dtype, x.device, out)
        if B == 0:
            return res
        plan.exec(x, T, 0, starts, B, None if labels else res, res if labels else None)
        return res

    def ragged(self, xs, lengths=None, dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None,
               labels: bool = False) -> torch.Tensor:
        """Extension: resample signals of DIFFERENT lengths, every one to ``num`` samples, in one call (``hssfsst_resample_exec_ragged``)
        -- whole recordings, as the reference's lazy dataset resamples them one call each (hss/datasets/heart_sounds.py:175-184,199-212).

        ``xs``: a sequence of 1-D signals (``(T_i,)`` or ``(T_i, 1)``, all on the CPU or all on one cuda device), or ONE packed 1-D
        buffer with ``lengths`` (its signals back to back), as ``FSST.ragged``.  Dtypes as ``batch``: float32 / float64 are read as
        they are, other real dtypes as float64.  Returns ``(len(xs), num)`` of ``dtype`` (float32 / float64) on the input's device,
        or with ``labels=True`` the int64 label rule of ``resample_labels`` for every signal.  Row i is within 1e-12 of
        ``Resample(num)(xs[i])`` and does not depend on the other signals.  ``out`` optionally receives the result."""
        # ---- arguments, all checked before a plan (or the GPU) is touched
        if isinstance(xs, (torch.Tensor, np.ndarray)):
            if lengths is None:
                raise ValueError("Resample.ragged: a single tensor is a packed buffer and needs lengths=; pass a list for separate signals")
            buf = xs if isinstance(xs, torch.Tensor) else torch.as_tensor(xs)
            if buf.ndim == 2 and buf.shape[-1] == 1:
                buf = buf[:, 0]
            if buf.ndim != 1:
                raise ValueError(f"Resample.ragged: a packed buffer must be 1-D, got {tuple(buf.shape)}")
            if buf.is_complex():
                raise ValueError("Resample.ragged: complex input is not supported")
            lens = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths, dtype=np.int64).reshape(-1)
            if lens.size and int(lens.min()) < 1:
                raise ValueError("Resample.ragged: every length must be >= 1")
            if int(lens.sum()) != int(buf.shape[0]):
                raise ValueError(f"Resample.ragged: lengths sum to {int(lens.sum())}, the buffer holds {int(buf.shape[0])} samples")
            X = _as_real(buf).contiguous()
        else:
            if lengths is not None:
                raise ValueError("Resample.ragged: lengths= goes with one packed buffer, not with a list of signals")
            sigs = []
            for i, x in enumerate(xs):
                t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
                if t.ndim == 2 and t.shape[-1] == 1:
                    t = t[:, 0]
                if t.ndim != 1:
                    raise ValueError(f"Resample.ragged: signal {i} has shape {tuple(t.shape)}; expected (T,) or (T, 1)")
                if t.is_complex():
                    raise ValueError(f"Resample.ragged: signal {i} is complex; real input expected")
                if t.shape[0] < 1:
                    raise ValueError(f"Resample.ragged: signal {i} is empty")
                sigs.append(_as_real(t))
            devs = {t.device for t in sigs}
            if len(devs) > 1:
                raise ValueError(f"Resample.ragged: the signals lie on different devices {sorted(str(d) for d in devs)}; "
                                 "pass all on the CPU or all on one cuda device")
            lens = np.asarray([int(t.shape[0]) for t in sigs], dtype=np.int64)
            odev = devs.pop() if devs else torch.device("cpu")
            if not sigs:
                X = torch.empty(0, dtype=torch.float32, device=odev)
            elif len(sigs) == 1:
                X = sigs[0].contiguous()
            else:                                          # (float32 with float64: float64, exactly)
                X = torch.cat([t.reshape(-1) for t in sigs])
        num = int(self.num)
        if num < 1:
            raise ValueError(f"Resample.ragged: need at least one output sample (num={num})")
        if not labels and dtype not in (torch.float32, torch.float64):
            raise ValueError(f"Resample.ragged: dtype must be float32 or float64, got {dtype}")
        B = int(lens.size)
        res = self._out(B, torch.int64 if labels else dtype, X.device, out)
        if B == 0:
            return res
        # ---- one call
        dev = self._device_index(X)
        key = ("ragged", os.getpid(), dev, num)
        if not hasattr(self, "_plans"):
            self._plans = {}
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = _RaggedResamplePlan(dev, num)
        starts = np.ascontiguousarray(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64))
        plan.exec(X, starts, np.ascontiguousarray(lens), None if labels else res, res if labels else None)
        return res

    def lds_tier(self, n: int, device_index: Optional[int] = None) -> bool:
        """Extension: True when (n, num) runs the one-launch LDS kernel, False for the multi-pass tier (whole recordings)."""
        dev = self._device_index() if device_index is None else device_index
        return self._plan(dev, int(n)).lds_tier

    # ------------------------------------------------------------------ the reference's call
    def __call__(self, x: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        if getattr(self, "device", None) is not None:
            return self._call_device(x, dtype)
        xs = x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(x)
        if xs.dim() != 1:
            # scipy resamples along axis 0; the reference only ever passes 1-D signals / label vectors
            if xs.dim() == 2 and xs.shape[1] == 1:
                return self(xs[:, 0], dtype).unsqueeze(1)
            raise ValueError(f"Resample expects a 1-D tensor, got shape {tuple(xs.shape)}")
        if xs.is_complex():
            raise ValueError("Resample: complex input is not supported")
        xin = np.ascontiguousarray(xs.to(torch.float64).numpy())
        num = int(self.num)
        if num < 1 or xin.size < 1:
            raise ValueError(f"Resample: need at least one input and one output sample (n={xin.size}, num={num})")
        y = np.empty(num, dtype=np.float64)
        dp = ctypes.POINTER(ctypes.c_double)
        rc = _lib.lib().hssfsst_resample(xin.ctypes.data_as(dp), xin.size, num, y.ctypes.data_as(dp))
        _lib.check(rc, "hssfsst_resample")
        return torch.from_numpy(y).to(dtype)

    def _call_device(self, x, dtype: torch.dtype) -> torch.Tensor:
        """``__call__`` on ``self.device``: same shapes, errors and result (a fresh CPU tensor of ``dtype``) as the host path."""
        xs = _as_real(x)
        if xs.dim() != 1:
            if xs.dim() == 2 and xs.shape[1] == 1:
                return self._call_device(xs[:, 0], dtype).unsqueeze(1)
            raise ValueError(f"Resample expects a 1-D tensor, got shape {tuple(xs.shape)}")
        n, num = int(xs.shape[0]), int(self.num)
        if num < 1 or n < 1:
            raise ValueError(f"Resample: need at least one input and one output sample (n={n}, num={num})")
        odt = dtype if dtype in (torch.float32, torch.float64) else torch.float64
        y = self._run(xs.contiguous().unsqueeze(0), odt, None, labels=False)[0]
        return y.to("cpu", dtype) if (y.is_cuda or y.dtype != dtype) else y


def resample_labels_batch(Y: torch.Tensor, t: Resample) -> torch.Tensor:
    """Extension: ``resample_labels`` for ``(B, n)`` label tracks (or one ``(n,)`` track) on the device -- ``(B, num)`` int64 on Y's
    device (CPU in, CPU out).  Equal to ``resample_labels`` row by row except where a resampled value sits on a .5 tie."""
    X = t._frames_view(Y)
    res = t._run(X, torch.float32, None, labels=True)
    return res[0] if _as_real(Y).ndim == 1 else res


def resample_labels_ragged(ys, t: Resample) -> torch.Tensor:
    """Extension: ``resample_labels`` for a list of label tracks of DIFFERENT lengths in one device call (``Resample.ragged``) --
    ``(len(ys), num)`` int64 on the tracks' device.  Equal to ``resample_labels`` track by track except where a resampled value
    sits on a .5 tie."""
    return t.ragged(ys, labels=True)


def resample_labels(y: torch.Tensor, t: Resample) -> torch.Tensor:
    """The label rule of DavidSpringerHSS._apply_transform (hss/datasets/heart_sounds.py:205-206)."""
    return torch.round(t(y)).type(torch.int64) - 1
