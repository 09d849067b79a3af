"""What becomes of the segmenter's log-probs, one HIP call each for a whole list of recordings: the Viterbi decoders
(``decode_states``, ``decode_durations``), the posteriors and sequence losses under the same models (``state_posteriors``,
``sequence_nll``, ``duration_posteriors``, ``duration_nll``), the scores (``segmentation_scores``), the stitching of overlapping
windows' log-probs into one sequence per recording (``stitch_windows``) and the helpers that make their tables.  ``consumer``
imports the public names back."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .transforms.synchrosqueeze import RaggedFeatures


# ---------------------------------------------------------------------------------------------- what the entries share
def _info(name: str, *kinds):
    """The out-parameters of the C call ``name(kind *, ...)`` -- ``kinds``: ``ctypes.c_int`` or ``ctypes.c_int64`` each -- as a
    tuple of ints: the ``*_info()`` functions.  No device needed."""
    outs = [k(0) for k in kinds]
    _lib.check(getattr(_lib.lib(), name)(*(ctypes.byref(o) for o in outs)), name)
    return tuple(o.value for o in outs)


def _ready() -> None:
    """What a caller of ``_call`` does BEFORE it allocates anything on the device: the library is there, and a child forked after
    HIP was initialised gets ``guard_fork``'s RuntimeError and its one warning, not torch's."""
    _lib.lib()
    _lib.guard_fork()


def _call(name: str, data: torch.Tensor, offs, *args, lead=None, launch: bool = False):
    """One call of the entry ``name(logp, offsets, count, ..., device, stream)`` on the arena ``data`` and the non-empty list
    ``offs``, on the current stream of ``data``'s device.  ``args``: what stands between ``count`` and ``device``; a tensor and a
    float32 array (a host table) go as their pointers, None as NULL.  ``lead``: what stands before ``offsets`` where that is more
    than ``data`` (which then only names the device); an int64 array among them goes as an ``int64_t*``.  ``launch``: True -- the
    entry takes ``(device, stream)`` as one ``const hssfsst_launch*`` (``hssfsst_score_states``); ``"value"`` -- as one
    ``hssfsst_launch`` by value (``hssfsst_stitch_windows``).  Raises what ``_lib.check`` makes of the status.  The guard runs here
    once more (it compares two pids), so that a caller that forgot ``_ready()`` still gets it, if late."""
    _ready()
    device = data.device
    o = np.asarray(offs, dtype=np.int64)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)

    def pointer(a):
        if isinstance(a, np.ndarray):
            return a.ctypes.data_as(ip if a.dtype == np.int64 else fp)
        return a.data_ptr() if isinstance(a, torch.Tensor) else a
    args = [pointer(a) for a in args]
    lead = [data.data_ptr()] if lead is None else [pointer(a) for a in lead]
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        if launch == "value":
            where = (_lib.Launch(device.index, stream),)
        else:
            where = (ctypes.byref(_lib.Launch(device.index, stream)),) if launch else (device.index, stream)
        _lib.check(getattr(_lib.lib(), name)(*lead, o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(offs) - 1, *args, *where), name)


def _like_input(logp, kind: str, t: torch.Tensor, offs):
    """The per-step result ``t`` -- an arena ``(sum T,)`` of states or ``(sum T, 4)`` -- in the kind of the input ``logp``: a
    ``RaggedStates`` or ``RaggedFeatures`` over the same offsets, ``(B, T[, 4])``, or the arena itself."""
    if kind == "ragged":
        off = torch.tensor(offs, dtype=torch.int64)
        return RaggedStates(t, off) if t.dim() == 1 else RaggedFeatures(t, off, 4, False)
    if kind == "batch":
        return t.view(int(logp.shape[0]), int(logp.shape[1]), *t.shape[1:])
    return t


def _reduce_nll(nll: torch.Tensor, reduction: str, steps: int) -> torch.Tensor:
    if reduction == "none":
        return nll
    if reduction == "sum":
        return nll.sum().to(torch.float32)
    return (nll.sum() / max(steps, 1)).to(torch.float32)


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
    return _info("hssfsst_decode_info", ctypes.c_int, ctypes.c_int64)


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
    out = _like_input(logp, kind, states, offs)
    if scores is None:
        return out
    # (NEG, the score of a recording with an all -inf step, reads as -inf)
    sc = scores.cpu()
    val = torch.where(sc == torch.iinfo(torch.int64).min, torch.tensor(float("-inf"), dtype=torch.float64), sc.double() / float(1 << 20))
    if kind == "ragged":
        out.scores = val
    return out, val[0] if kind == "single" else val


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
    A, pi = _host_array(transitions), _host_array(initial)
    if A.shape != (4, 4) or pi.shape != (4,):            # (one text for both tables: not _host_table's)
        raise ValueError(f"{name}: transitions (4, 4) and initial (4,) expected, got {A.shape} and {pi.shape}")
    data, offs, kind = _decode_input(name, logp)
    _ready()
    data = data.detach().contiguous()
    states = torch.empty((offs[-1],), dtype=torch.uint8, device=data.device)
    scores = torch.empty((len(offs) - 1,), dtype=torch.int64, device=data.device) if return_scores else None
    if len(offs) > 1:
        _call("hssfsst_decode_states", data, offs, A, pi, states, scores)
    return _decode_output(logp, kind, states, offs, scores)


def decode_durations_info():
    """``(max_duration, max_steps, workspace_bytes_per_step)`` of the explicit-duration decoder
    (``hssfsst_decode_durations_info``).  No device needed."""
    return _info("hssfsst_decode_durations_info", ctypes.c_int, ctypes.c_int64, ctypes.c_int64)


def _host_array(v) -> np.ndarray:
    """A table given as a tensor or an array -> contiguous float32 numpy on the host."""
    return np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32)


def _host_table(name: str, what: str, v, shape=None):
    a = _host_array(v)
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
    _ready()
    data = data.detach().contiguous()
    states = torch.empty((offs[-1],), dtype=torch.uint8, device=data.device)
    scores = torch.empty((len(offs) - 1,), dtype=torch.int64, device=data.device) if return_scores else None
    if len(offs) > 1:
        work = torch.empty((decode_durations_info()[2] * (offs[-1] + 8 * D),), dtype=torch.uint8, device=data.device)
        _call("hssfsst_decode_durations", data, offs, A, pi, dur, eg, D, states, scores, work, work.numel())
    return _decode_output(logp, kind, states, offs, scores)


# ------------------------------------------------------------------- log-probs -> state posteriors and the sequence loss
def posteriors_info():
    """``(segment_steps, max_steps, work_bytes_per_step, work_bytes_per_recording)`` of the forward-backward kernel
    (``hssfsst_posteriors_info``).  No device needed."""
    return _info("hssfsst_posteriors_info", ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64)


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
            t = torch.from_numpy(_host_array(v)).to(device)
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: {what} {shape} expected, got {tuple(t.shape)}")
        out.append(t)
    return out[0], out[1]


def _posteriors_run(data, offs, a_pi, labels=None, tables_grad: bool = False):
    """One ``hssfsst_posteriors`` call on the current stream -> ``(gamma, loglik, score, xi, gamma0)``; ``score`` only with
    ``labels`` (a uint8 arena on the device), ``xi`` and ``gamma0`` only with ``tables_grad``; None otherwise."""
    _ready()
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
        _call("hssfsst_posteriors", data, offs, a_pi, labels, gamma, loglik, score, xi, gamma0, work, work.numel())
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
    gamma, loglik = _posteriors_run(data.detach().contiguous(), offs, _a_pi(A, pi))[:2]
    out = _like_input(logp, kind, gamma, offs)
    return (out, loglik[0] if kind == "single" else loglik) if return_loglik else out


def _nll_labels(name: str, labels, offs, kind: str, device, ignore_outside: bool = False) -> torch.Tensor:
    """The labels of ``sequence_nll`` -> one uint8 arena ``(sum T,)`` on ``device``.  Lengths are checked always; values are
    checked (0..3) where the labels are on the HOST -- labels on the device are not read back (no synchronisation): the kernel
    looks at their two low bits only.  ``ignore_outside`` (``segmentation_scores``): values outside 0..3 are allowed anywhere and
    become 255, whatever the integer type (-100 and 256 alike)."""
    total, count = offs[-1], len(offs) - 1

    def u8(t):
        if ignore_outside and t.dtype != torch.uint8:
            t = t.to(torch.int64)                        # (int8 cannot hold 255)
            t = torch.where((t < 0) | (t > 3), torch.full_like(t, 255), t)
        return t.to(device=device, dtype=torch.uint8)

    def values(t, what):
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)
        if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
            raise ValueError(f"{name}: {what}: integer labels expected")
        if not ignore_outside and t.device.type == "cpu" and t.numel() and (int(t.min()) < 0 or int(t.max()) > 3):
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
            items.append(u8(t))
        arena = torch.cat(items) if items else torch.empty((0,), dtype=torch.uint8, device=device)
    else:
        t = values(labels, "labels")
        if kind == "batch" and t.dim() == 2 and t.shape[0] == count and t.shape[0] * t.shape[1] == total:
            arena = t.reshape(total)
        elif t.dim() == 1 and t.shape[0] == total:
            arena = t
        else:
            raise ValueError(f"{name}: labels of shape {tuple(t.shape)} do not match {count} recordings of {total} steps in all")
    return u8(arena).contiguous()


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
    return _reduce_nll(_SequenceNLL.apply(data, A, pi, arena, offs), reduction, offs[-1])


# ------------------------------------------------- log-probs -> posteriors and the sequence loss under duration scores
def duration_posteriors_info():
    """``(max_duration, segment_steps, max_steps, work_bytes_per_step, work_bytes_per_recording, work_bytes_per_duration)`` of the
    explicit-duration forward-backward kernel (``hssfsst_posteriors_durations_info``).  No device needed."""
    return _info("hssfsst_posteriors_durations_info", ctypes.c_int, ctypes.c_int, *[ctypes.c_int64] * 4)


def duration_counts_info():
    """``(work_bytes_per_step, work_bytes_per_recording, work_bytes_per_duration, durations_per_group)`` of the run-length counts
    call (``hssfsst_posteriors_durations_counts_info``); the other limits are ``duration_posteriors_info()``'s.  No device needed."""
    return _info("hssfsst_posteriors_durations_counts_info", *[ctypes.c_int64] * 3, ctypes.c_int)


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
    _ready()
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
        head = (data, offs, a_pi, dur, edge, D, labels, gamma, onsets, loglik, score, xi, s0)
        if want_counts:
            _call("hssfsst_posteriors_durations_counts", *head, counts, work, work.numel())
        else:
            _call("hssfsst_posteriors_durations", *head, work, work.numel())
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
    out = [_like_input(logp, kind, gamma, offs)]
    if return_loglik:
        out.append(loglik[0] if kind == "single" else loglik)
    if return_onsets:
        out.append(_like_input(logp, kind, onsets, offs))
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
    return _reduce_nll(_DurationNLL.apply(data, A, pi, dur, eg, arena, offs), reduction, offs[-1])


def state_runs(states: torch.Tensor):
    """The boundaries of a decoded recording: ``(starts int64, state uint8)`` of the runs of equal states in the 1-D ``states``
    (``torch.unique_consecutive``), on its device.  Run k covers steps ``starts[k] .. starts[k + 1]`` (the last one to the end)."""
    if not isinstance(states, torch.Tensor) or states.dim() != 1:
        raise ValueError("state_runs: a 1-D tensor of states expected")
    vals, counts = torch.unique_consecutive(states, return_counts=True)
    starts = torch.cumsum(counts, 0) - counts
    return starts.to(torch.int64), vals.to(torch.uint8)


# ----------------------------------------------------------------- predictions and labels -> confusion counts and AUROC
def score_info():
    """``(work_bytes_per_step, work_bytes_per_recording, work_bytes_constant, block_items, digit_bits, max_passes)`` of the
    scoring call (``hssfsst_score_info``): the factors of its workspace and the geometry of its radix sort.  No device needed."""
    return _info("hssfsst_score_info", *[ctypes.c_int64] * 3, *[ctypes.c_int] * 3)


def _safe_ratio(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """``num / den`` in float64, 0 where ``den`` is 0 (an empty denominator scores 0, as in torchmetrics)."""
    num, den = num.to(torch.float64), den.to(torch.float64)
    return torch.where(den == 0, torch.zeros_like(num), num / torch.where(den == 0, torch.ones_like(den), den))


class SegmentationScores:
    """What ``segmentation_scores`` returns: the exact integers of the call, on its device, and the usual figures derived from
    them in float64 torch ops -- nothing here waits for the device.  With ``per_recording`` every tensor has a leading ``(B,)``.

    ``confusion`` ``(4, 4)`` int64 ``[label][predicted]``; ``ignored`` int64, the steps left out; ``rank`` ``(4, 3)`` int64
    ``{2U, P, N}`` per class, or None (``auroc=False``, or states scored without ``scores``).

    Derived: ``support`` (4,) = steps per label; ``accuracy`` = correct / counted; per class ``precision``, ``recall``, ``f1``; their
    plain means over the four classes ``macro_precision``, ``macro_recall``, ``macro_f1``; ``auroc`` (4,) = ``2U / (2 P N)``, the exact
    one-vs-rest area with ties at one half, NaN where a class has no positive or no negative; ``macro_auroc``, its mean over the
    classes where it is defined (NaN where none is).  An empty denominator gives 0.  torchmetrics' per-class multiclass
    "accuracy" (``average=None``) is this ``recall``."""

    def __init__(self, confusion: torch.Tensor, ignored: torch.Tensor, rank):
        self.confusion, self.ignored, self.rank = confusion, ignored, rank

    @property
    def _tp(self):
        return torch.diagonal(self.confusion, dim1=-2, dim2=-1)

    @property
    def support(self):
        return self.confusion.sum(dim=-1)

    @property
    def accuracy(self):
        return _safe_ratio(self._tp.sum(dim=-1), self.confusion.sum(dim=(-2, -1)))

    @property
    def precision(self):
        return _safe_ratio(self._tp, self.confusion.sum(dim=-2))

    @property
    def recall(self):
        return _safe_ratio(self._tp, self.support)

    @property
    def f1(self):
        return _safe_ratio(2 * self._tp, self.confusion.sum(dim=-2) + self.support)

    @property
    def macro_precision(self):
        return self.precision.mean(dim=-1)

    @property
    def macro_recall(self):
        return self.recall.mean(dim=-1)

    @property
    def macro_f1(self):
        return self.f1.mean(dim=-1)

    @property
    def auroc(self):
        if self.rank is None:
            raise ValueError("SegmentationScores.auroc: no rank was computed (auroc=False, or states scored without scores)")
        r = self.rank.to(torch.float64)
        return r[..., 0] / (2.0 * r[..., 1] * r[..., 2])

    @property
    def macro_auroc(self):
        return torch.nanmean(self.auroc, dim=-1)


def _score_input(name: str, what: str, pred):
    """``decode_states``' three kinds, of states (uint8, one per step) or of scores (float32, four per step) -> (the arena, the
    step offsets as a list, the kind, whether they are states)."""
    t = pred.data if isinstance(pred, RaggedFeatures) else pred
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{name}: {what}: uint8 states or float32 log-probs expected"
                         + (f", got {t.dtype}" if isinstance(t, torch.Tensor) else ""))
    if t.dtype == torch.float32:
        return (*_decode_input(name, pred), False)
    if isinstance(pred, RaggedFeatures):
        data, offs, kind = pred.data, [int(o) for o in pred._off], "ragged"
    elif pred.dim() == 2:
        B, T = int(pred.shape[0]), int(pred.shape[1])
        if B and T < 1:
            raise ValueError(f"{name}: {what}: (B, T) states with T >= 1 expected, got {tuple(pred.shape)}")
        data, offs, kind = pred.reshape(B * T), [i * T for i in range(B + 1)], "batch"
    elif pred.dim() == 1 and pred.shape[0] >= 1:
        data, offs, kind = pred, [0, int(pred.shape[0])], "single"
    else:
        raise ValueError(f"{name}: {what}: a RaggedStates, a (B, T) or a (T,) tensor with T >= 1 expected")
    if data.dim() != 1 or data.shape[0] != offs[-1]:
        raise ValueError(f"{name}: {what}: one state per step expected, got an arena of shape {tuple(data.shape)}")
    if data.device.type != "cuda":
        raise ValueError(f"{name}: {what} on a GPU expected, got {data.device}; the scoring has no CPU path")
    return data, offs, kind, True


def segmentation_scores(pred, labels, per_recording: bool = False, auroc: bool = True, scores=None) -> SegmentationScores:
    """How good a segmentation is, on the device (``hssfsst_score_states``): the confusion counts of predictions against labels
    and, from log-probs, the exact one-vs-rest AUROC of every class -- the Mann-Whitney statistic with ties, from a radix sort of
    the whole arena --, as exact integers.  What the reference's epochs end in (accuracy, precision, recall, F1, AUROC), for the
    ragged arenas of this package: nothing is padded and nothing is copied to the host.

    ``pred``: ``decode_states``' three kinds, of either dtype.  uint8 = states, one per step (a ``RaggedStates``, ``(B, T)`` or
    ``(T,)``: what the decoders return); float32 = log-probs or any score per step and class (a ``RaggedFeatures``, ``(B, T, 4)`` or
    ``(T, 4)``), whose argmax is the prediction: ties go to the smaller state, NaN reads as ``-inf``.  ``scores``: with states as
    ``pred``, the float32 scores to rank for the AUROC (same list of lengths); the states stay the predictions.
    ``labels``: as for ``sequence_nll`` (a list of 1-D integer tensors, a ``RaggedStates`` or an arena with matching offsets, a
    ``(B, T)`` / ``(T,)`` tensor), but values outside 0..3 are allowed and mean IGNORE (255, -100 ...): such a step is left out of
    every count and of the ranking and counted in ``ignored``; labels on the device are not read back.
    ``per_recording``: one result per recording (a leading ``(B,)``; each recording's steps are ranked among themselves) instead
    of one for all steps pooled, as the reference's test epoch pools them.  The pooled rank is not the sum of the recordings'.
    ``auroc=False`` skips the ranking (and its workspace of 17 bytes per step); states without ``scores`` have none.

    One call on the current stream; the int64 results stay on the device and ``SegmentationScores`` derives the figures from them
    without waiting for it.  All integers are exact and do not depend on the order of the kernels' atomics: two calls give the
    same bits.  The order of scores is float32's: ``-0 == +0``, ``-inf`` lowest, NaN reads as ``-inf``."""
    name = "segmentation_scores"
    data, offs, kind, is_states = _score_input(name, "pred", pred)
    logp, states = (None, data) if is_states else (data, None)
    if scores is not None:
        if not is_states:
            raise ValueError(f"{name}: scores are given beside states; pred already holds float32 scores")
        logp, soffs, _, s_states = _score_input(name, "scores", scores)
        if s_states or soffs != offs or logp.device != data.device:
            raise ValueError(f"{name}: scores must be float32, on the states' device, over the same list of lengths")
    arena = _nll_labels(name, labels, offs, kind, data.device, ignore_outside=True)
    _ready()
    count = len(offs) - 1
    groups = count if per_recording else 1
    want_rank = bool(auroc) and logp is not None
    i64 = dict(dtype=torch.int64, device=data.device)
    confusion = torch.zeros((groups, 4, 4), **i64)
    ignored = torch.zeros((groups,), **i64)
    rank = torch.zeros((groups, 4, 3), **i64) if want_rank else None
    if count:
        work = None
        if want_rank:
            per, rec, const = score_info()[:3]
            work = torch.empty((per * offs[-1] + rec * count + const,), dtype=torch.uint8, device=data.device)
        logp = None if logp is None else logp.detach().contiguous()
        states = None if states is None else states.contiguous()
        _call("hssfsst_score_states", data, offs, 1 if per_recording else 0, confusion, ignored, rank, work,
              work.numel() if work is not None else 0, lead=(logp, states, arena), launch=True)
    if not per_recording:
        confusion, ignored, rank = confusion[0], ignored[0], None if rank is None else rank[0]
    return SegmentationScores(confusion, ignored, rank)


# --------------------------------------------------------------------- overlapping windows' log-probs -> one sequence per recording
STITCH_MODES = {"prob": _lib.STITCH_PROB, "logp": _lib.STITCH_LOGP, "select": _lib.STITCH_SELECT}
STITCH_MAX_RATIO = 15                                    # ceil(n / stride) at most (csrc/stitch_layout.hpp: kMaxRatio)


def window_weights(n: int, kind: str = "triangular", device=None) -> torch.Tensor:
    """``(n,)`` float32 weights of a window's positions for ``stitch_windows``, strictly positive: ``"triangular"`` =
    ``min(p + 1, n - p)``, which trusts a window most in its middle, where the BiLSTM has context on both sides; ``"hann"`` =
    ``sin^2(pi (p + 1/2) / n)``; ``"flat"`` = ones (what ``weights=None`` means).  On ``device`` when given, else on the host."""
    n = int(n)
    if n < 1:
        raise ValueError(f"window_weights: n >= 1 expected, got {n}")
    p = np.arange(n, dtype=np.float64)
    if kind == "triangular":
        w = np.minimum(p + 1, n - p)
    elif kind == "hann":
        w = np.sin(np.pi * (p + 0.5) / n) ** 2
    elif kind == "flat":
        w = np.ones(n)
    else:
        raise ValueError(f"window_weights: kind 'triangular', 'flat' or 'hann' expected, got {kind!r}")
    t = torch.from_numpy(w.astype(np.float32))
    return t if device is None else t.to(device)


def _stitch_rows(T: int, n: int, stride: int) -> int:
    """The rows the windows of a T-step recording take in the window arena (csrc/stitch_layout.hpp: window_rows)."""
    return T if T <= n else ((T - n) // stride + 1 + (1 if (T - n) % stride else 0)) * n


def stitch_windows(win_logp: torch.Tensor, win_first, lengths_or_offsets, n: int, stride: int, weights=None, mode: str = "prob",
                   return_dissent: bool = False):
    """The log-probs of overlapping windows -> one sequence of log-probs per recording, on the device
    (``hssfsst_stitch_windows``): what turns a model trained on ``n``-step windows into a segmenter of whole recordings.

    The window set of a ``T``-step recording is ``framing.cover_starts(T, stride, n)``: it covers every step.  ``win_logp``: the
    ``(W, 4)`` float32 arena of the windows' log-probs on a GPU -- a full window takes ``n`` rows, the one window of a ``T <= n``
    recording ``T`` rows.  ``win_first``: per recording the arena row at which its windows start; they lie back to back in ascending
    start order, the recordings' blocks anywhere.  ``lengths_or_offsets``: the recordings' lengths (as many as ``win_first``) or
    their offsets from 0 (one more).  ``weights``: None (all ones), or ``(n,)`` weights of a window's positions
    (``window_weights``): given on the host they are checked (positive, finite) and uploaded, which waits for the stream; given
    on the device they are used as they are, unchecked.  ``mode``: ``"prob"`` -- the weighted mean of the covering windows'
    probabilities, renormalised; ``"logp"`` -- the weighted mean of their log-probs (the geometric mean), renormalised;
    ``"select"`` -- the row of the covering window with the largest weight, ties to the earlier window.  A step that one window
    covers is copied bit for bit.  float64 inside, rounded once; NaN and ``-inf`` follow IEEE (include/hssfsst.h).

    Returns a ``RaggedFeatures`` over the ``(sum T, 4)`` arena; with ``return_dissent`` also a ``RaggedStates``-shaped uint8 arena:
    per step the number of covering windows whose own argmax is not the stitched row's -- where the windows disagree.  One call
    on the current stream, nothing waits for the device.  ``ceil(n / stride) <= 15``, else RuntimeError."""
    name = "stitch_windows"
    if mode not in STITCH_MODES:
        raise ValueError(f"{name}: mode 'prob', 'logp' or 'select' expected, got {mode!r}")
    n, stride = int(n), int(stride)
    if n < 1 or not 1 <= stride <= n:
        raise ValueError(f"{name}: n >= 1 and 1 <= stride <= n expected, got n {n} and stride {stride}")
    if not isinstance(win_logp, torch.Tensor) or win_logp.dim() != 2 or win_logp.shape[1] != 4:
        raise ValueError(f"{name}: a (W, 4) arena of window log-probs expected")
    if win_logp.dtype != torch.float32:
        raise ValueError(f"{name}: float32 log-probs expected, got {win_logp.dtype}")
    first = np.ascontiguousarray(win_first.cpu().numpy() if isinstance(win_first, torch.Tensor) else win_first, dtype=np.int64).reshape(-1)
    lo = np.asarray(lengths_or_offsets.cpu().numpy() if isinstance(lengths_or_offsets, torch.Tensor) else lengths_or_offsets,
                    dtype=np.int64).reshape(-1)
    if lo.size == first.size + 1 and int(lo[0]) == 0:
        offs = [int(v) for v in lo]
    elif lo.size == first.size:
        offs = [0] + [int(v) for v in np.cumsum(lo)]
    else:
        raise ValueError(f"{name}: {first.size} recordings by win_first, but {lo.size} lengths or offsets (as many lengths, or one "
                         "more offset from 0, expected)")
    W = int(win_logp.shape[0])
    for i in range(first.size):
        T = offs[i + 1] - offs[i]
        if T < 1:
            raise ValueError(f"{name}: recording {i} has {T} steps")
        if first[i] < 0 or first[i] + _stitch_rows(T, n, stride) > W:
            raise ValueError(f"{name}: win_first[{i}] = {int(first[i])}: the {_stitch_rows(T, n, stride)} window rows of recording {i} "
                             f"do not lie within the {W} of the arena")
    if -(-n // stride) > STITCH_MAX_RATIO:
        raise RuntimeError(f"{name}: windows of {n} steps at stride {stride} overlap {-(-n // stride)}-fold, over the limit of "
                           f"{STITCH_MAX_RATIO}")
    w = None
    if weights is not None:
        on_device = isinstance(weights, torch.Tensor) and weights.is_cuda
        w = weights if on_device else torch.from_numpy(_host_array(weights))
        if tuple(w.shape) != (n,):
            raise ValueError(f"{name}: weights ({n},) expected, got {tuple(w.shape)}")
        if on_device and w.dtype != torch.float32:
            raise ValueError(f"{name}: float32 weights expected, got {w.dtype}")
        if not on_device and not bool((torch.isfinite(w) & (w > 0)).all()):
            raise ValueError(f"{name}: positive, finite weights expected")
    if win_logp.device.type != "cuda":
        raise ValueError(f"{name}: log-probs on a GPU expected, got {win_logp.device}; the stitch has no CPU path")
    if w is not None and w.is_cuda and w.device != win_logp.device:
        raise ValueError(f"{name}: weights on {w.device}, the log-probs on {win_logp.device}")
    _ready()
    device = win_logp.device
    w = None if w is None else w.detach().to(device).contiguous()
    out = torch.empty((offs[-1], 4), dtype=torch.float32, device=device)
    dissent = torch.empty((offs[-1],), dtype=torch.uint8, device=device) if return_dissent else None
    if len(offs) > 1:
        data = win_logp.detach().contiguous()
        _call("hssfsst_stitch_windows", data, offs, n, stride, w, STITCH_MODES[mode], out, dissent, lead=(data, first, W), launch="value")
    off = torch.tensor(offs, dtype=torch.int64)
    res = RaggedFeatures(out, off, 4, False)
    return (res, RaggedStates(dissent, off)) if return_dissent else res
