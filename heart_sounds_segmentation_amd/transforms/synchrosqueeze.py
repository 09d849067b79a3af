"""``FSST`` -- drop-in for the reference's ``hss.transforms.FSST``
(/root/reference/hss/transforms/synchrosqueeze.py:8-111) backed by the gfx950 HIP kernels behind
the C ABI of ``include/hssfsst.h``.

Same constructor, attribute names, call signature, output shapes / dtypes / orientation and error
behaviour as the reference class; the body (native ``ssq.fsst`` + torch epilogue) is replaced by one
``hssfsst_exec`` call.  Extensions that the reference does not have: ``device=`` and ``batch()``.
There is no CPU implementation here: without the HIP library or a GPU every call raises.
"""
from __future__ import annotations

import ctypes
import os
from collections.abc import Sequence as _SequenceABC
from typing import Optional

import numpy as np
import numpy.typing as npt
import torch

from .. import _lib


def _release_pinned(plan, addr: int) -> None:
    """A pinned pool buffer goes back to its plan (the borrower holds the plan alive until then)."""
    try:
        if plan.handle and plan.handle.value and plan.pid == os.getpid():
            plan._L.hssfsst_pinned_release(plan.handle, ctypes.c_void_p(addr))
    except Exception:
        pass


_LENT_TYPES = {}


def _lent_type(nfl: int, elem=ctypes.c_float):
    """ctypes array type (``nfl`` elements of ``elem``: float, or a 2-byte integer for a half-precision plan's elements) over a LENT
    pinned pool buffer: the numpy array / tensor made from an instance keeps it alive, and when the last view of the result is gone the
    instance's ``__del__`` hands the buffer back (``hssfsst_pinned_release``).  (A subclass with ``__del__`` + ``np.frombuffer`` +
    ``torch.from_numpy`` costs 1.4 us per call; ``weakref.finalize`` + ``torch.frombuffer`` + ``view`` cost 3.3.)"""
    T = _LENT_TYPES.get((nfl, elem))
    if T is None:
        class _Lent(elem * nfl):
            _plan = None

            def __del__(self):
                _release_pinned(self._plan, ctypes.addressof(self))
        T = _LENT_TYPES[(nfl, elem)] = _Lent
    return T


# output element types of STACK features (hssfsst_plan_create_ex): torch dtype -> HSSFSST_DTYPE_*
_OUT_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


class _Plan:
    """Owner of one ``hssfsst_plan*`` (created lazily in the calling process: fork-safe)."""

    def __init__(self, device_index: int, window: np.ndarray, fs: float, band, mode: int, out_dtype: torch.dtype = torch.float32):
        _lib.guard_fork()
        L = _lib.lib()
        self._L = L
        self.handle = ctypes.c_void_p()
        w = np.ascontiguousarray(window, dtype=np.float64).ravel()
        has_band = 1 if band else 0
        lo, hi = (float(band[0]), float(band[1])) if band else (0.0, 0.0)
        rc = L.hssfsst_plan_create_ex(ctypes.byref(self.handle), int(device_index), int(w.size),
                                      w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), float(fs),
                                      has_band, lo, hi, int(mode), _OUT_DTYPES[out_dtype])
        _lib.check(rc, "hssfsst_plan_create_ex")
        vals = [ctypes.c_int() for _ in range(7)]
        _lib.check(L.hssfsst_plan_info(self.handle, *[ctypes.byref(v) for v in vals]), "hssfsst_plan_info")
        self.nwin, self.nf, self.klo, self.K, self.ofps, self.mode, self.device = [v.value for v in vals]
        # the element type of the plan's time-major features (RAW is complex64 whatever this says)
        self.out_dtype = out_dtype
        self.pid = os.getpid()

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value and self.pid == os.getpid():
                self._L.hssfsst_plan_destroy(self.handle)
        except Exception:
            pass


class RaggedFeatures(_SequenceABC):
    """The features of ``FSST.ragged``: signals of different lengths, packed back to back in ONE arena.

    ``data``: the arena -- ``(sum T_i, C)`` float32 for ``abs`` / ``stack`` (C = K / 2K; ``stack`` in the transform's ``out_dtype``), ``(K * sum T_i,)`` complex64 for the raw
    transform (signal i's ``(K, T_i)`` block at ``K * offsets[i]``); ``offsets``: int64 ``(B + 1,)`` in samples.  ``len``, iteration
    and ``[i]`` work as on a list; item i is a view with exactly the shape, dtype and device ``FSST.__call__`` / ``FSST.batch`` give
    for signal i alone."""

    def __init__(self, data: torch.Tensor, offsets: torch.Tensor, K: int, raw: bool):
        self.data = data
        self.offsets = offsets
        self._off = [int(v) for v in offsets.tolist()]
        self._K, self._raw = int(K), bool(raw)

    def __len__(self) -> int:
        return len(self._off) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        a, b = self._off[i], self._off[i + 1]
        if self._raw:
            return self.data[self._K * a:self._K * b].view(self._K, b - a)
        return self.data[a:b]

    def lengths(self) -> torch.Tensor:
        """``(B,)`` int64 signal lengths."""
        return self.offsets[1:] - self.offsets[:-1]

    def padded(self, padding_value: float = 0.0) -> torch.Tensor:
        """``abs`` / ``stack``: ``(B, T_max, C)`` with ``padding_value`` past each signal's end -- what
        ``torch.nn.utils.rnn.pad_sequence(list(self), batch_first=True, padding_value=...)`` gives, in one scatter."""
        if self._raw:
            raise ValueError("RaggedFeatures.padded: the raw transform is frequency-major (K, T); pad the items yourself")
        B = len(self)
        lens = self.lengths().to(self.data.device)
        T = int(lens.max()) if B else 0
        out = torch.full((B, T, int(self.data.shape[1])), float(padding_value), dtype=self.data.dtype, device=self.data.device)
        if B and T:
            mask = torch.arange(T, device=self.data.device)[None, :] < lens[:, None]
            out[mask] = self.data                        # (row-major mask order == the arena's signal-major order)
        return out


class FSST:
    """
    Fourier Synchrosqueezed Transform (MI355X / HIP implementation).

    Args mirror the reference constructor (synchrosqueeze.py:13-35):
        fs: sample frequency.
        window: analysis window (numpy array); its length is the FFT length.
        abs: return ``abs(s).t()`` -> float32 ``(n, K)``.
        stack: return the z-scored real and imaginary parts stacked -> float32 ``(n, 2K)``.
        truncate_freq: ``(lo, hi)`` in Hz, inclusive; keeps K rows.  None/empty keeps all.
        dtype: kept for signature parity (the reference only uses it for ``f``/``t``; not the features' type).
        device (extension): torch device for the computation; default ``cuda`` (current device).
        out_dtype (extension): element type of the ``stack`` features -- ``torch.float32`` (default), ``torch.float16`` or
            ``torch.bfloat16``.  A half type is written by the kernels themselves and equals the float32 result cast with
            ``.to(out_dtype)`` bit for bit (NaN where float32 has NaN).  Only with ``stack=True`` and not ``abs``: ``ValueError``
            otherwise.  ``unnormalized()`` stays float32.
    Precedence as in ``__call__`` (synchrosqueeze.py:56-65): truncate, then ``abs`` wins over
    ``stack``, else the raw complex64 ``(K, n)`` spectrum.
    """

    def __init__(
        self,
        fs: float,
        window: npt.NDArray,
        abs: bool = False,
        stack: bool = False,
        truncate_freq: Optional[tuple] = None,
        dtype: torch.dtype = torch.float32,
        device: Optional[torch.device] = None,
        out_dtype: torch.dtype = torch.float32,
    ):
        if out_dtype not in _OUT_DTYPES:
            raise ValueError(f"FSST: out_dtype must be torch.float32, torch.float16 or torch.bfloat16, got {out_dtype}")
        if out_dtype != torch.float32 and (abs or not stack):
            raise ValueError(f"FSST: out_dtype={out_dtype} is for the z-scored stack features only (stack=True, abs=False); "
                             "abs and the raw transform stay float32 / complex64")
        self.fs: float = fs
        self.window: npt.NDArray = window
        self.abs = abs
        self.stack = stack
        self.truncate_freq = truncate_freq
        self.dtype = dtype
        self.device = device
        self.out_dtype = out_dtype
        self._plans = {}
        self._cuda_seen = False
        self._ragged_stage = None                      # pinned staging of ragged() host lists (kept between calls)

    # ------------------------------------------------------------------ plan / geometry
    def _mode(self) -> int:
        if self.abs:
            return _lib.MODE_ABS
        if self.stack:
            return _lib.MODE_STACK
        return _lib.MODE_RAW

    def _device_index(self, like: Optional[torch.Tensor] = None) -> int:
        _lib.guard_fork()
        if like is not None and like.is_cuda:
            return like.device.index if like.device.index is not None else torch.cuda.current_device()
        if not torch.cuda.is_available():
            raise RuntimeError("FSST: no HIP device visible (torch.cuda.is_available() is False); "
                               "this implementation has no CPU fallback")
        if self.device is not None:
            d = torch.device(self.device)
            if d.type != "cuda":
                raise RuntimeError(f"FSST: device {d} is not a HIP device; there is no CPU path")
            return d.index if d.index is not None else torch.cuda.current_device()
        return torch.cuda.current_device()

    def _stack_dtype(self) -> torch.dtype:
        return getattr(self, "out_dtype", torch.float32)

    def _plan(self, device_index: int, mode: Optional[int] = None) -> _Plan:
        mode = self._mode() if mode is None else mode
        odt = self._stack_dtype() if mode == _lib.MODE_STACK else torch.float32      # (unnormalized(): float32 whatever out_dtype)
        key = (os.getpid(), device_index, mode, odt)
        plan = self._plans.get(key)
        if plan is None:
            band = tuple(self.truncate_freq) if self.truncate_freq else None
            plan = _Plan(device_index, np.asarray(self.window), float(self.fs), band, mode, odt)
            self._plans[key] = plan
        return plan

    def __getstate__(self):          # plans hold device handles: never pickle them into workers
        st = self.__dict__.copy()
        st["_plans"] = {}
        st["_cuda_seen"] = False
        st["_ragged_stage"] = None
        return st

    def band(self):
        """(klo, K): first kept row and number of kept rows (host-side; no GPU needed)."""
        klo, K = ctypes.c_int(), ctypes.c_int()
        w = np.asarray(self.window)
        if self.truncate_freq:
            _lib.check(_lib.lib().hssfsst_band(int(w.size), float(self.fs), float(self.truncate_freq[0]),
                                               float(self.truncate_freq[1]), ctypes.byref(klo),
                                               ctypes.byref(K)), "hssfsst_band")
            return klo.value, K.value
        return 0, int(w.size) // 2 + 1

    # ------------------------------------------------------------------ execution
    def _run(self, X: torch.Tensor, mode: Optional[int] = None,
             out: Optional[torch.Tensor] = None, cols: Optional[tuple] = None) -> torch.Tensor:
        """X: (B, n) float32, CPU or cuda, unit stride along n and a positive stride between signals (a dense
        batch, or overlapping frames of one recording as made by framing.frame_batch -- read in place).
        Returns per-mode tensor on X's device.  cols = (col0, ncols) restricts the output to those frame centres."""
        B, n_in = X.shape
        xstride = int(X.stride(0)) if B > 1 else int(n_in)
        if n_in > 1 and X.stride(1) != 1:
            raise ValueError("FSST: samples of a signal must be contiguous")
        col0, n = cols if cols is not None else (0, n_in)
        if col0 < 0 or n < 1 or col0 + n > n_in:
            raise ValueError(f"FSST: column range ({col0}, {n}) outside a signal of {n_in} samples")
        if n_in < 1:
            raise ValueError("FSST: empty signal")
        dev = self._device_index(X)
        plan = self._plan(dev, mode)
        K = plan.K
        m = plan.mode
        on_dev = X.is_cuda
        odev = X.device
        if m == _lib.MODE_RAW:
            shape, dt = (B, K, n), torch.complex64
        elif m == _lib.MODE_ABS:
            shape, dt = (B, n, K), torch.float32
        else:
            shape, dt = (B, n, 2 * K), plan.out_dtype
        if out is None:
            out = torch.empty(shape, dtype=dt, device=odev)
        elif (tuple(out.shape) != shape or out.dtype != dt or out.device != odev
              or not out.is_contiguous()):
            raise ValueError(f"FSST: out must be a contiguous {dt} tensor of shape {shape} on {odev}")
        if B == 0 or K == 0:
            return out
        stream = torch.cuda.current_stream(dev).cuda_stream     # (host buffers too: staged and waited for on this stream)
        rc = _lib.lib().hssfsst_exec_frames(plan.handle, ctypes.c_void_p(X.data_ptr()), int(B), int(n_in), xstride,
                                            int(col0), int(n), 1 if on_dev else 0,
                                            ctypes.c_void_p(out.data_ptr()), 1 if on_dev else 0,
                                            ctypes.c_void_p(stream) if stream else None)
        _lib.check(rc, "hssfsst_exec_frames")
        return out

    @staticmethod
    def _as_f32(x: torch.Tensor, frames: bool = False) -> torch.Tensor:
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(np.asarray(x))
        if x.is_complex():
            raise ValueError("FSST: real input expected")
        x = x.detach().to(torch.float32)
        # frames=True: a (B, n) view with unit stride along n and a positive signal stride is read in place
        # (overlapping frames of one recording: no duplicated copy); anything else is made dense
        if frames and x.ndim == 2 and x.shape[1] > 1 and x.stride(1) == 1 and (x.shape[0] <= 1 or x.stride(0) >= 1):
            return x
        return x.contiguous()

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        """
        Computes the transform of ONE signal, like the reference ``__call__``
        (synchrosqueeze.py:37-65).  Accepts what the reference's callers pass: ``(n,)`` or ``(n, 1)``
        float32 (dataset frames, heart_sounds.py:167,181) or float64 (visualisation script).
        A CPU tensor returns a CPU tensor, a cuda tensor (extension) stays on the device.

        Returns: ``stack`` -> ``(n, 2K)`` of ``out_dtype`` (float32 by default); ``abs`` -> float32 ``(n, K)``; otherwise
        complex64 ``(K, n)``.
        """
        # the dataset loop's call -- a CPU float32 (n,) / (n, 1) frame, once per 2000 samples (heart_sounds.py:166-168,199-201) --
        # goes straight to the C ABI: of a 0.057 ms call the generic path below spent 0.012 ms on conversions and checks
        if (type(x) is torch.Tensor and x.dtype is torch.float32 and x.is_cpu and x.is_contiguous()
                and not x.requires_grad and (x.dim() == 1 or (x.dim() == 2 and 1 in x.shape)) and x.numel() > 0):
            if self.device is None and self._cuda_seen:  # (the checks of _device_index were made by an earlier call of this process)
                _lib.guard_fork()
                plan = self._plan(torch.cuda.current_device())
            else:
                plan = self._plan(self._device_index(x))
                self._cuda_seen = True
            n, K, m = x.numel(), plan.K, plan.mode
            if K > 0:
                L = _lib.lib()
                # the kernels store the features into a pinned buffer of the plan's pool and the returned tensor IS that buffer (no 352 kB
                # copy): it goes back to the pool when the last view of the result dies; a caller that keeps every result finds the pool lent
                # out after 64 frames and gets freshly allocated tensors filled by a copy, as before (hssfsst.h: hssfsst_exec_pinned)
                ptr = ctypes.c_void_p()
                rc = L.hssfsst_exec_pinned(plan.handle, x.data_ptr(), n, ctypes.byref(ptr))
                half = plan.out_dtype is not torch.float32 and m == _lib.MODE_STACK
                if rc == 0:
                    if half:                             # (2-byte elements: numpy has no bfloat16 -- the bits, viewed as the dtype)
                        buf = _lent_type(n * plan.ofps, ctypes.c_int16).from_address(ptr.value)
                        buf._plan = plan
                        return torch.from_numpy(np.frombuffer(buf, dtype=np.int16).reshape(n, 2 * K)).view(plan.out_dtype)
                    buf = _lent_type(n * plan.ofps).from_address(ptr.value)
                    buf._plan = plan
                    if m == _lib.MODE_RAW:
                        return torch.from_numpy(np.frombuffer(buf, dtype=np.complex64).reshape(K, n))
                    return torch.from_numpy(np.frombuffer(buf, dtype=np.float32).reshape(n, K if m == _lib.MODE_ABS else 2 * K))
                if rc < 0:
                    _lib.check(rc, "hssfsst_exec_pinned")
                out = (torch.empty((K, n), dtype=torch.complex64) if m == _lib.MODE_RAW
                       else torch.empty((n, K if m == _lib.MODE_ABS else 2 * K), dtype=plan.out_dtype if half else torch.float32))
                _lib.check(L.hssfsst_exec_frames(plan.handle, x.data_ptr(), 1, n, n, 0, n, 0, out.data_ptr(), 0, None),
                           "hssfsst_exec_frames")
                return out
        x = self._as_f32(x)
        if x.ndim == 2 and 1 in x.shape:
            x = x.reshape(-1)
        if x.ndim != 1:
            raise ValueError(f"FSST: expected a single signal of shape (n,) or (n, 1), got "
                             f"{tuple(x.shape)}; use FSST.batch for (B, n)")
        return self._run(x.unsqueeze(0))[0]

    def batch(self, X: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Extension: transform ``B`` independent signals at once.  ``X``: ``(B, n)`` (CPU or cuda).
        Returns ``(B, n, 2K)`` / ``(B, n, K)`` / complex64 ``(B, K, n)`` on X's device; a CPU input
        is staged through the device by the library.  ``out`` optionally receives the result."""
        X = self._as_f32(X, frames=True)
        if X.ndim == 3 and X.shape[-1] == 1:
            X = X[..., 0]
        if X.ndim != 2:
            raise ValueError(f"FSST.batch: expected (B, n), got {tuple(X.shape)}")
        return self._run(X, out=out)

    def frames(self, x: torch.Tensor, starts, n: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Extension (batched dataset builder): transform the frames
        ``x[starts[b] : starts[b] + n]`` of ONE 1-D buffer -- e.g. many recordings laid back to back, ``starts`` =
        every frame of every recording (``framing.frame_starts``) -- in one call (``hssfsst_exec_list``).
        ``x``: ``(T,)`` float32, CPU or cuda; ``starts``: int64 sequence / tensor (CPU, or on x's device).
        Returns ``(len(starts), n, 2K)`` / ``(.., n, K)`` / complex64 ``(.., K, n)`` on x's device."""
        x = self._as_f32(x)
        if x.ndim != 1:
            raise ValueError(f"FSST.frames: expected one 1-D buffer, got {tuple(x.shape)}")
        if not isinstance(starts, torch.Tensor):
            starts = torch.as_tensor(np.asarray(starts, dtype=np.int64))
        starts = starts.to(torch.int64).contiguous()
        if starts.ndim != 1:
            raise ValueError("FSST.frames: starts must be 1-D")
        B, T, n = int(starts.shape[0]), int(x.shape[0]), int(n)
        if n < 1 or T < n:
            raise ValueError(f"FSST.frames: frame length {n} does not fit a buffer of {T} samples")
        if starts.is_cuda and (not x.is_cuda or starts.device != x.device):
            starts = starts.cpu()
        if B and not starts.is_cuda and (int(starts.min()) < 0 or int(starts.max()) > T - n):
            raise ValueError(f"FSST.frames: a frame start lies outside [0, {T - n}]")
        dev = self._device_index(x)
        plan = self._plan(dev)
        K, m = plan.K, plan.mode
        if m == _lib.MODE_RAW:
            shape, dt = (B, K, n), torch.complex64
        elif m == _lib.MODE_ABS:
            shape, dt = (B, n, K), torch.float32
        else:
            shape, dt = (B, n, 2 * K), plan.out_dtype
        if out is None:
            out = torch.empty(shape, dtype=dt, device=x.device)
        elif tuple(out.shape) != shape or out.dtype != dt or out.device != x.device or not out.is_contiguous():
            raise ValueError(f"FSST.frames: out must be a contiguous {dt} tensor of shape {shape} on {x.device}")
        if B == 0 or K == 0:
            return out
        on_dev = x.is_cuda
        stream = torch.cuda.current_stream(dev).cuda_stream     # (host buffers too: staged and waited for on this stream)
        rc = _lib.lib().hssfsst_exec_list(plan.handle, ctypes.c_void_p(x.data_ptr()), T, ctypes.c_void_p(starts.data_ptr()),
                                          1 if starts.is_cuda else 0, B, n, 1 if on_dev else 0,
                                          ctypes.c_void_p(out.data_ptr()), 1 if on_dev else 0,
                                          ctypes.c_void_p(stream) if stream else None)
        _lib.check(rc, "hssfsst_exec_list")
        return out

    def ragged(self, xs, lengths=None, out: Optional[torch.Tensor] = None) -> RaggedFeatures:
        """Extension: transform signals of DIFFERENT lengths in one call (``hssfsst_exec_ragged``) -- whole recordings, as the
        reference's lazy dataset and PhysioNet loader transform them one call each (hss/datasets/heart_sounds.py:85-106,175-184).

        ``xs``: a sequence of 1-D signals (``(T_i,)`` or ``(T_i, 1)``, float32 / float64, all on the CPU or all on one cuda device),
        or ONE packed 1-D buffer with ``lengths`` (its signals back to back).  float64 is rounded to float32 first, as ``__call__``
        does.  Returns a ``RaggedFeatures`` on the input's device whose item i equals ``self.batch(xs[i][None])[0]`` bit for bit.
        ``out``: an arena to write into (``RaggedFeatures.data``'s shape, dtype and device)."""
        raw = not (self.abs or self.stack)
        # ---- arguments, all checked before a plan (or the GPU) is touched
        if isinstance(xs, torch.Tensor) or isinstance(xs, np.ndarray):
            if lengths is None:
                raise ValueError("FSST.ragged: a single tensor is a packed buffer and needs lengths=; pass a list for separate signals")
            buf = xs if isinstance(xs, torch.Tensor) else torch.as_tensor(xs)
            if buf.ndim == 2 and buf.shape[-1] == 1:
                buf = buf[:, 0]
            if buf.ndim != 1:
                raise ValueError(f"FSST.ragged: a packed buffer must be 1-D, got {tuple(buf.shape)}")
            lens = np.asarray(lengths.cpu() if isinstance(lengths, torch.Tensor) else lengths, dtype=np.int64).reshape(-1)
            if lens.size and int(lens.min()) < 1:
                raise ValueError("FSST.ragged: every length must be >= 1")
            if int(lens.sum()) != int(buf.shape[0]):
                raise ValueError(f"FSST.ragged: lengths sum to {int(lens.sum())}, the buffer holds {int(buf.shape[0])} samples")
            sigs = None
            on_dev, odev = buf.is_cuda, buf.device
            if buf.is_complex():
                raise ValueError("FSST.ragged: real input expected")
        else:
            if lengths is not None:
                raise ValueError("FSST.ragged: lengths= goes with one packed buffer, not with a list of signals")
            sigs = []
            for i, x in enumerate(xs):
                t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
                if t.ndim == 2 and t.shape[-1] == 1:
                    t = t[:, 0]
                if t.ndim != 1:
                    raise ValueError(f"FSST.ragged: signal {i} has shape {tuple(x.shape)}; expected (T,) or (T, 1)")
                if t.is_complex():
                    raise ValueError(f"FSST.ragged: signal {i} is complex; real input expected")
                if t.shape[0] < 1:
                    raise ValueError(f"FSST.ragged: signal {i} is empty")
                sigs.append(t)
            devs = {t.device for t in sigs}
            if len(devs) > 1:
                raise ValueError(f"FSST.ragged: the signals lie on different devices {sorted(str(d) for d in devs)}; "
                                 "pass all on the CPU or all on one cuda device")
            odev = devs.pop() if devs else torch.device("cpu")
            on_dev = odev.type == "cuda"
            lens = np.asarray([int(t.shape[0]) for t in sigs], dtype=np.int64)
        B, total = int(lens.size), int(lens.sum())
        offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
        klo, K = self.band()
        C = K if self.abs else 2 * K
        shape, dt = ((K * total,), torch.complex64) if raw else ((total, C), self._stack_dtype() if self.stack and not self.abs else torch.float32)
        if out is not None and (tuple(out.shape) != shape or out.dtype != dt or out.device != odev or not out.is_contiguous()):
            raise ValueError(f"FSST.ragged: out must be a contiguous {dt} tensor of shape {shape} on {odev}")
        if B == 0:
            return RaggedFeatures(out if out is not None else torch.empty(shape, dtype=dt, device=odev), offsets, K, raw)
        # ---- pack
        dev = self._device_index(torch.empty(0, device=odev) if on_dev else None)
        plan = self._plan(dev)
        L = _lib.lib()
        if sigs is None:
            X = buf.detach().to(torch.float32).contiguous()
            starts = offsets[:-1].numpy()
        elif on_dev:
            X = torch.cat([t.detach().to(torch.float32) for t in sigs]) if B > 1 else sigs[0].detach().to(torch.float32).contiguous()
            starts = offsets[:-1].numpy()
        else:
            # host list: one native call copies the signals (threaded) into a pinned staging buffer, from which the library's one
            # upload is a DMA
            held = [t.detach() if (t.dtype == torch.float32 and t.is_contiguous()) else t.detach().to(torch.float32).contiguous() for t in sigs]
            stage = getattr(self, "_ragged_stage", None)
            if stage is None or stage.numel() < total:
                try:
                    stage = torch.empty(max(total, 1 << 16), dtype=torch.float32, pin_memory=True)
                except RuntimeError:
                    stage = torch.empty(max(total, 1 << 16), dtype=torch.float32)
                self._ragged_stage = stage
            ptrs = np.asarray([t.data_ptr() for t in held], dtype=np.uint64)
            starts = np.empty(B, dtype=np.int64)
            _lib.pack_recordings(ptrs, lens, stage, starts, B)
            X = stage
        if out is None:
            out = torch.empty(shape, dtype=dt, device=odev)
        if K > 0:
            stream = torch.cuda.current_stream(dev).cuda_stream     # (host buffers too: staged and waited for on this stream)
            lens_c = np.ascontiguousarray(lens)
            starts_c = np.ascontiguousarray(starts, dtype=np.int64)
            rc = L.hssfsst_exec_ragged(plan.handle, ctypes.c_void_p(X.data_ptr()), int(X.numel()), ctypes.c_void_p(starts_c.ctypes.data),
                                       ctypes.c_void_p(lens_c.ctypes.data), B, 1 if on_dev else 0, ctypes.c_void_p(out.data_ptr()),
                                       1 if on_dev else 0, ctypes.c_void_p(stream) if stream else None)
            _lib.check(rc, "hssfsst_exec_ragged")
        return RaggedFeatures(out, offsets, K, raw)

    def check(self, device_index: Optional[int] = None) -> int:
        """Extension: waits for the device and raises ``RuntimeError`` if a kernel reported a failed internal wait
        (the library also reports it at the start of the plan's next call, without being asked).  Returns the path of
        the plan's last ``stack`` call: 0 = two launches, 1 = the one-CU-per-signal z-score kernel (when preferred),
        2 = the team kernel (features normalised in registers, written once: the default for the reference's band and
        signals up to 2048 samples); truthy = a single launch."""
        dev = self._device_index() if device_index is None else device_index
        plan = self._plan(dev)
        _lib.check(_lib.lib().hssfsst_plan_check(plan.handle), "hssfsst_plan_check")
        return int(_lib.lib().hssfsst_plan_last_exec_fused(plan.handle))

    def last_kernel(self, device_index: Optional[int] = None) -> str:
        """Extension: the transform kernel that device's plan ran last -- ``"<instantiation> [<waves> waves/block, grid <n>]"``
        (which of the library's kernels a window length / band / mode / shape takes is otherwise only visible in a trace)."""
        dev = self._device_index() if device_index is None else device_index
        buf = ctypes.create_string_buffer(160)
        _lib.check(_lib.lib().hssfsst_plan_last_kernel(self._plan(dev).handle, buf, len(buf)), "hssfsst_plan_last_kernel")
        return buf.value.decode()

    def set_zpath(self, zpath: str = "auto", device_index: Optional[int] = None) -> None:
        """Extension: preference among the z-score paths of the following ``stack`` calls on that device's plan --
        "auto" (the fastest that applies), "two_launch", "one_cu", "team".  Results do not depend on it (bit-identical)."""
        dev = self._device_index() if device_index is None else device_index
        code = {"auto": 0, "two_launch": 1, "one_cu": 2, "team": 3}[zpath]
        _lib.check(_lib.lib().hssfsst_plan_set_zpath(self._plan(dev).handle, code), "hssfsst_plan_set_zpath")

    def fallbacks(self, device_index: Optional[int] = None) -> int:
        """Extension: how many team-kernel launches of that device's plan gave themselves up and were computed by the
        two-launch kernels queued behind them (other processes kept the team's blocks apart): a performance event, not
        an error.  Call after a synchronisation."""
        dev = self._device_index() if device_index is None else device_index
        return int(_lib.lib().hssfsst_plan_fallbacks(self._plan(dev).handle))

    def set_timing(self, enable, device_index: Optional[int] = None) -> None:
        """Extension (bench): record HIP events around the kernels of every following call (``True`` / 1) or of every n-th one
        (an int n > 1: the events themselves cost stream time); ``False`` / 0: off."""
        dev = self._device_index() if device_index is None else device_index
        _lib.check(_lib.lib().hssfsst_plan_set_timing(self._plan(dev).handle, int(enable)),
                   "hssfsst_plan_set_timing")

    def timing(self, device_index: Optional[int] = None):
        """(core_ms_sum, normalize_ms_sum, n_calls) since ``set_timing(True)``; synchronises."""
        dev = self._device_index() if device_index is None else device_index
        ms = (ctypes.c_float * 2)()
        cnt = ctypes.c_int()
        _lib.check(_lib.lib().hssfsst_plan_timing(self._plan(dev).handle, ms, ctypes.byref(cnt)),
                   "hssfsst_plan_timing")
        return float(ms[0]), float(ms[1]), cnt.value

    def unnormalized(self, X: torch.Tensor, cols: Optional[tuple] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Extension (streaming): ``(B, n, 2K)`` [real | imag] features
        WITHOUT the per-signal z-score, for use with running moments.  ``cols=(col0, ncols)``
        computes only those frame centres.  ``out`` optionally receives the result, as in ``batch``."""
        X = self._as_f32(X, frames=True)
        if X.ndim == 1:
            X = X.unsqueeze(0)
        return self._run(X, _lib.MODE_STACK_UNNORM, out=out, cols=cols)

    # ------------------------------------------------------------------ reference helper kept for its contract
    def _truncate_frequencies(self, s: torch.Tensor, f: torch.Tensor):
        """Same contract as the reference helper (synchrosqueeze.py:91-111): raises ``ValueError``
        when ``truncate_freq`` is unset; otherwise slices the rows inside the band."""
        if not self.truncate_freq:
            raise ValueError(f"truncate_freq must be set, got: {self.truncate_freq}")
        klo, K = self.band()
        return s[klo:klo + K, :], f.reshape(-1)[klo:klo + K]
