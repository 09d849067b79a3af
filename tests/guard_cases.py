"""The calls tests/test_guard_bands.py walks through a guard arena (tests/guard_arena.py), as one table.  No tests here.

A case makes its call from buffers an ALLOCATOR hands out, so that the same code runs twice: on ordinary torch tensors (``Plain``:
the route the rest of the suite holds to the oracle) and with every caller-owned pointer -- inputs, outputs, workspaces, host
arrays -- carved from an arena (``Carved``).  The outputs must have the same bits and every band must be intact.  Then the carved
call is repeated with one pointer at a time moved off its 16-byte boundary: an input by one element, an output by one element and
by 8 bytes.  What each pointer promises there is the contract of include/hssfsst.h:

  (a) any element-aligned address works and gives the aligned call's bits: the names in a case's ``inputs`` / ``outputs``;
  (b) the header states 16 bytes and the entry refuses with HSSFSST_EINVAL before any device work: REFUSALS below, asserted on
      the CPU with addresses that are never dereferenced.  The sequence entries' own refusals are tests/test_sequence_entries.py's.

``covers`` of a case: {C entry point: the parameters of its header declaration that the case carves}.  tests/test_guard_bands.py
holds every pointer parameter of include/hssfsst.h to this table or to EXEMPT.

Shapes are the smallest at which the kernels take each of their paths (partial 16-frame groups and 64-frame tiles, more than one
block, both sides of every threshold between two kernels), not the workload's."""
import ctypes

import numpy as np
import torch

from heart_sounds_segmentation_amd import _lib, synth
from heart_sounds_segmentation_amd import sequence as seq
from heart_sounds_segmentation_amd.transforms import FSST
from heart_sounds_segmentation_amd.transforms.synchrosqueeze import RaggedFeatures
from tests import guard_arena as ga
from tests.launch_cases import BAND, LAUNCH_CASES, launch_kernel, launch_transform

ELEM = "one element"                                     # a skew of one element of whatever dtype the buffer has
DEV_CAPACITY = 16 << 20                                  # the device arena of the walk: a whole case needs a few MiB
HOST_CAPACITY = 40 << 20                                 # hssfsst_exec's staged case writes 14 MiB of features to the host


# ---------------------------------------------------------------------------------------------------- allocators
def _filled(shape, dtype, device, pinned=False):
    """An ordinary tensor with FILL_BYTE in every byte, as a carved output has."""
    n = ga.elem_size(dtype) * int(np.prod(shape, dtype=np.int64))
    t = torch.full((n,), ga.FILL_BYTE, dtype=torch.uint8, device=device)
    if pinned:
        t = t.pin_memory()
    return t.view(dtype).view(tuple(shape))


class Plain:
    """Ordinary tensors: device ones from torch's allocator, host ones pageable, or pinned when the call needs that."""
    carved = False

    def __init__(self, device):
        self.device = torch.device(device)

    def inp(self, name, data, host=False, pinned=False):
        t = data.detach().cpu().clone()
        if host:
            return t.pin_memory() if pinned else t
        return t.to(self.device)

    def out(self, name, shape, dtype, host=False, pinned=False):
        return _filled(shape, dtype, "cpu" if host else self.device, pinned and host)

    work = out


class Carved:
    """Every buffer from an arena: ``dev`` for device memory, ``host`` for pageable and ``pin`` for page-locked host memory.
    ``skew``: {buffer name: ELEM or a number of bytes}; every other buffer sits on a 16-byte boundary."""
    carved = True

    def __init__(self, dev, host, pin=None, skew=None):
        self.dev, self.host, self.pin, self.skew = dev, host, pin, dict(skew or {})
        self.device = dev.device if dev is not None else torch.device("cpu")
        self.placed = []                                 # (buffer name, data_ptr() % 16) of every carve, for the walk to look at

    def arenas(self):
        return [a for a in (self.dev, self.host, self.pin) if a is not None]

    def reset(self):
        for a in self.arenas():
            a.reset()

    def _where(self, host, pinned):
        return (self.pin if pinned else self.host) if host else self.dev

    def _skew(self, name, dtype):
        s = self.skew.get(name, 0)
        return ga.elem_size(dtype) if s == ELEM else int(s)

    def _carve(self, name, shape, dtype, host, pinned, kind, data=None):
        t = self._where(host, pinned).carve(tuple(shape), dtype, self._skew(name, dtype), kind, name, data)
        self.placed.append((name, t.data_ptr() % 16))
        return t

    def inp(self, name, data, host=False, pinned=False):
        return self._carve(name, data.shape, data.dtype, host, pinned, "in", data)

    def out(self, name, shape, dtype, host=False, pinned=False):
        return self._carve(name, shape, dtype, host, pinned, "out")

    def work(self, name, shape, dtype, host=False, pinned=False):
        return self._carve(name, shape, dtype, host, pinned, "work")


# ---------------------------------------------------------------------------------------------------- a case
class GuardCase:
    """name       unique; subsystem: the heading it is counted under in profiles/guard_bands.txt
    covers     {C entry point: (header parameter names the case carves)}
    make       () -> context (plans, input data on the host), made once
    call       (context, allocator) -> {output name: tensor}; deterministic, repeatable
    inputs     buffer names that are read only and may sit at any element (a): skewed by one element
    outputs    buffer names that are written (in-out ones too) and may sit at any element (a): skewed by one element and by 8 bytes
    kernel     (context) -> last_kernel() of the aligned carved call, and ``kernel_is``, the recorded string it must start with
    python     (context) -> {output name: tensor} from the package's own entry point: the plain call must have its bits
    gpu        False: the call touches host memory only and runs in the CPU suite too"""

    def __init__(self, name, subsystem, covers, make, call, inputs=(), outputs=(), kernel=None, kernel_is=None, python=None, gpu=True):
        self.name, self.subsystem, self.covers = name, subsystem, {k: tuple(v) for k, v in covers.items()}
        self.make, self.call, self.inputs, self.outputs = make, call, tuple(inputs), tuple(outputs)
        self.kernel, self.kernel_is, self.python, self.gpu = kernel, kernel_is, python, gpu

    def __repr__(self):
        return self.name

    def variants(self):
        """[(label, skew)]: the aligned call, then one pointer at a time off its boundary."""
        out = [("aligned", {})]
        out += [(f"{n} + one element", {n: ELEM}) for n in self.inputs]
        for n in self.outputs:
            out += [(f"{n} + one element", {n: ELEM}), (f"{n} + 8 bytes", {n: 8})]
        return out


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    s = torch.cuda.current_stream().cuda_stream
    return ctypes.c_void_p(s) if s else None


def _ok(rc, what):
    _lib.check(rc, what)


def _rand(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dtype)


def _i64(values):
    return torch.tensor([int(v) for v in values], dtype=torch.int64)


def _offsets(lens):
    return [0] + [int(v) for v in np.cumsum(lens)]


CASES = []


def _add(*a, **kw):
    CASES.append(GuardCase(*a, **kw))


# ---------------------------------------------------------------------------------------------------- FSST through out=
def _fsst_out(tf, case, B, n, A):
    klo, K = tf.band()
    if case["mode"] == "raw":
        return A.out("out", (B, K, n), torch.complex64)
    if case["mode"] == "abs":
        return A.out("out", (B, n, K), torch.float32)
    return A.out("out", (B, n, 2 * K), torch.float32 if "cols" in case else case.get("out_dtype", torch.float32))


def _fsst_case(name, case, kernel_is=None, seed=1234):
    """A row in the form of tests/launch_cases.py through ``out=``: ``ragged`` rows on FSST.ragged (one packed buffer), ``cols`` rows
    on FSST.unnormalized, the others on FSST.batch.  ``batch``: signals (2 as in that table unless given)."""
    B = case.get("batch", 2)

    def make():
        tf = launch_transform(case)
        if "ragged" in case:
            return tf, torch.cat([_rand((t,), seed + i) for i, t in enumerate(case["ragged"])])
        return tf, _rand((B, case["n"]), seed)

    def call(ctx, A):
        tf, X = ctx
        x = A.inp("x", X)
        klo, K = tf.band()
        if "ragged" in case:
            total = sum(case["ragged"])
            out = (A.out("out", (K * total,), torch.complex64) if case["mode"] == "raw" else
                   A.out("out", (total, K if case["mode"] == "abs" else 2 * K), case.get("out_dtype", torch.float32)))
            tf.ragged(x, lengths=case["ragged"], out=out)
        elif "cols" in case:
            out = _fsst_out(tf, case, B, case["cols"][1], A)
            tf.unnormalized(x, cols=case["cols"], out=out)
        else:
            if "zpath" in case:
                tf.set_zpath(case["zpath"])
            out = _fsst_out(tf, case, B, case["n"], A)
            tf.batch(x, out=out)
        return {"out": out}

    entry = "hssfsst_exec_ragged" if "ragged" in case else "hssfsst_exec_frames"
    _add(name, "FSST", {entry: ("x", "out")}, make, call, inputs=("x",), outputs=("out",),
         kernel=(lambda ctx: launch_kernel(ctx[0], case)) if kernel_is else None, kernel_is=kernel_is)


for _name, _case, _kernel in LAUNCH_CASES:
    _fsst_case("fsst: " + _name, _case, _kernel)
_N128 = dict(nwin=128, fs=1000, band=BAND, mode="stack")
_fsst_case("fsst: one sample", dict(_N128, n=1, batch=3))
_fsst_case("fsst: 17 samples", dict(_N128, n=17, batch=3))
# (odd K, a row count that is no multiple of 4: n 2K & 3 != 0, the element-wise z-score sweep)
_fsst_case("fsst: odd K, 401 samples", dict(_N128, band=(25, 195), n=401, batch=3))
_fsst_case("fsst: 100 points raw, one sample", dict(_N128, nwin=100, mode="raw", band=None, n=1, batch=3))


def _frames_case(starts_on_device):
    starts = [0, 1000, 3500, 7000]

    def make():
        return launch_transform(_N128), _rand((9000,), 77)

    def call(ctx, A):
        tf, X = ctx
        x = A.inp("x", X)
        st = A.inp("starts", _i64(starts), host=not starts_on_device)
        out = A.out("out", (len(starts), 2000, 2 * tf.band()[1]), torch.float32)
        tf.frames(x, st, 2000, out=out)
        return {"out": out}

    _add(f"fsst: frames of a 9000-sample buffer, {'device' if starts_on_device else 'host'} starts", "FSST",
         {"hssfsst_exec_list": ("x", "starts", "out")}, make, call, inputs=("x", "starts"), outputs=("out",))


_frames_case(False)
_frames_case(True)


def _strided_case():
    B, n, stride = 4, 2000, 999

    def make():
        return launch_transform(_N128), _rand(((B - 1) * stride + n,), 78)

    def call(ctx, A):
        tf, X = ctx
        x = A.inp("x", X)
        out = A.out("out", (B, n, 2 * tf.band()[1]), torch.float32)
        tf.batch(x.as_strided((B, n), (stride, 1)), out=out)
        return {"out": out}

    _add("fsst: frames 999 samples apart, read in place", "FSST", {"hssfsst_exec_frames": ("x", "out")}, make, call,
         inputs=("x",), outputs=("out",))


_strided_case()


# ---------------------------------------------------------------------------------------------------- FSST through the C ABI
def _plan_case():
    """hssfsst_plan_create reads its window on the host; hssfsst_dtwin reads one and writes one.  No device: host arenas only."""
    def make():
        return torch.from_numpy(np.ascontiguousarray(synth.kaiser_window(128, 0.5), dtype=np.float64))

    def call(w, A):
        L = _lib.lib()
        win = A.inp("window", w, host=True)
        dw = A.out("dwindow", (128,), torch.float64, host=True)
        dp = ctypes.POINTER(ctypes.c_double)
        _ok(L.hssfsst_dtwin(ctypes.cast(win.data_ptr(), dp), 128, 1000.0, ctypes.cast(dw.data_ptr(), dp)), "hssfsst_dtwin")
        return {"dwindow": dw}

    _add("host: the derivative window", "FSST", {"hssfsst_dtwin": ("window", "dwindow")}, make, call,
         inputs=("window",), outputs=("dwindow",), gpu=False)


_plan_case()


def _exec_host_case(B):
    """hssfsst_exec with host x and host out: one 2000-sample signal takes the plan's pinned buffers and two memcpys, 40 of them
    the device staging and two copies.  The plan is created from a carved window."""
    n = 2000

    def make():
        return torch.from_numpy(np.ascontiguousarray(synth.kaiser_window(128, 0.5), dtype=np.float64)), _rand((B, n), 79)

    def call(ctx, A):
        w, X = ctx
        L = _lib.lib()
        win = A.inp("window", w, host=True)
        plan = ctypes.c_void_p()
        _ok(L.hssfsst_plan_create(ctypes.byref(plan), 0, 128, ctypes.cast(win.data_ptr(), ctypes.POINTER(ctypes.c_double)), 1000.0,
                                  1, float(BAND[0]), float(BAND[1]), _lib.MODE_STACK), "hssfsst_plan_create")
        try:
            x = A.inp("x", X, host=True)
            out = A.out("out", (B, n, 44), torch.float32, host=True)
            _ok(L.hssfsst_exec(plan, _ptr(x), B, n, 0, _ptr(out), 0, _stream()), "hssfsst_exec")
        finally:
            L.hssfsst_plan_destroy(plan)
        return {"out": out}

    _add(f"exec: {B} x 2000 samples, host in and out", "FSST", {"hssfsst_exec": ("x", "out"), "hssfsst_plan_create": ("window",),
         "hssfsst_plan_create_ex": ("window",)}, make, call, inputs=("x", "window"), outputs=("out",))


_exec_host_case(1)
_exec_host_case(40)


def _exec_cols_case():
    B, n, col0, ncols = 2, 400, 16, 80

    def make():
        return launch_transform(_N128), _rand((B, n), 80)

    def call(ctx, A):
        tf, X = ctx
        plan = tf._plan(0)
        x = A.inp("x", X)
        out = A.out("out", (B, ncols, 2 * plan.K), torch.float32)
        _ok(_lib.lib().hssfsst_exec_cols(plan.handle, _ptr(x), B, n, col0, ncols, 1, _ptr(out), 1, _stream()), "hssfsst_exec_cols")
        return {"out": out}

    _add("exec_cols: columns 16 .. 95 of 400", "FSST", {"hssfsst_exec_cols": ("x", "out")}, make, call, inputs=("x",), outputs=("out",))


_exec_cols_case()


def _exec_ragged_case(nwin):
    """hssfsst_exec_ragged with its two host arrays carved: the one-launch list of the MFMA kernels (128 points), and one exec
    per signal at its own element offset of `out` (64 points, 11 rows: the second signal's block of 44 floats starts 22 floats
    into `out`, 8 bytes off a 16-byte boundary when `out` is aligned, and is a whole number of float4s, which is what the z-score
    sweep asks before it takes its float4 path)."""
    lens = [1, 2, 333] if nwin == 64 else [48, 333, 17]
    case = dict(_N128, nwin=nwin, band=(25, 195) if nwin == 64 else BAND)

    def make():
        return launch_transform(case), _rand((sum(lens),), 81)

    def call(ctx, A):
        tf, X = ctx
        plan = tf._plan(0)
        x = A.inp("x", X)
        starts = A.inp("starts", _i64(_offsets(lens)[:-1]), host=True)
        ln = A.inp("lens", _i64(lens), host=True)
        out = A.out("out", (sum(lens), 2 * plan.K), torch.float32)
        _ok(_lib.lib().hssfsst_exec_ragged(plan.handle, _ptr(x), sum(lens), _ptr(starts), _ptr(ln), len(lens), 1, _ptr(out), 1, _stream()),
            "hssfsst_exec_ragged")
        return {"out": out}

    _add(f"exec_ragged: signals of {lens} samples, {nwin} points", "FSST", {"hssfsst_exec_ragged": ("x", "starts", "lens", "out")}, make, call,
         inputs=("x", "starts", "lens"), outputs=("out",))


_exec_ragged_case(128)
_exec_ragged_case(64)


def _exec_pinned_case():
    n = 2000

    def make():
        return launch_transform(_N128), _rand((n,), 82)

    def call(ctx, A):
        tf, X = ctx
        plan = tf._plan(0)
        L = _lib.lib()
        x = A.inp("x", X, host=True)
        lent = ctypes.c_void_p()
        rc = L.hssfsst_exec_pinned(plan.handle, _ptr(x), n, ctypes.byref(lent))
        _ok(rc if rc < 0 else 0, "hssfsst_exec_pinned")
        assert rc == 0 and lent.value, "the pool lends a buffer for one canonical-band frame"
        got = torch.from_numpy(np.ctypeslib.as_array(ctypes.cast(lent, ctypes.POINTER(ctypes.c_float)), shape=(n, 2 * plan.K)).copy())
        _ok(L.hssfsst_pinned_release(plan.handle, lent), "hssfsst_pinned_release")
        return {"lent": got}

    _add("exec_pinned: one host frame into a lent buffer", "FSST", {"hssfsst_exec_pinned": ("x",)}, make, call, inputs=("x",))


_exec_pinned_case()


# ---------------------------------------------------------------------------------------------------- moments and streaming
def _moments_case(B, n):
    def make():
        tf = FSST(1000, synth.kaiser_window(128, 0.5), stack=True, truncate_freq=BAND)
        return tf, _rand((B, n, 44), 90, 3.0), _rand((B, n, 44), 91, 3.0)

    def call(ctx, A):
        tf, F0, F1 = ctx
        plan = tf._plan(0, _lib.MODE_STACK_UNNORM)
        L = _lib.lib()
        state = A.inp("state", torch.zeros((B, 6), dtype=torch.float64))
        for F in (F0, F1):                               # (the second merge meets a state that holds counts)
            feats = A.inp("feats", F)
            _ok(L.hssfsst_moments_merge(plan.handle, _ptr(feats), B, n, _ptr(state), _stream()), "hssfsst_moments_merge")
        _ok(L.hssfsst_normalize_running(plan.handle, _ptr(feats), B, n, _ptr(state), _stream()), "hssfsst_normalize_running")
        return {"state": state, "feats": feats}

    _add(f"moments: merge twice, normalise, ({B}, {n})", "moments and streaming",
         {"hssfsst_moments_merge": ("feats", "state"), "hssfsst_normalize_running": ("feats", "state")}, make, call,
         outputs=("feats", "state"))


_moments_case(3, 17)
_moments_case(2, 1029)


def _stream_case(nwin, band, pinned):
    """hssfsst_stream_step, 3 channels, chunk 16: 256 points with an even band of 6 rows is the one-launch step, 128 points the
    copy, the exec and the merge-and-normalise launch.  ``pinned``: x_new and out_host in page-locked host memory."""
    C, chunk, hist = 3, 16, nwin - 1
    tape_len = hist + 4 * chunk

    def make():
        tf = FSST(1000, synth.kaiser_window(nwin, 0.5), stack=True, truncate_freq=band)
        return tf, _rand((C, tape_len), 92), _rand((C, chunk), 93)

    def call(ctx, A):
        tf, T0, X = ctx
        plan = tf._plan(0, _lib.MODE_STACK_UNNORM)
        tape = A.inp("tape", T0)
        x_new = A.inp("x_new", X, host=pinned, pinned=pinned)
        out = A.out("out", (C, chunk, 2 * plan.K), torch.float32)
        state = A.inp("state", torch.zeros((C, 6), dtype=torch.float64))
        out_host = A.out("out_host", (C, chunk, 2 * plan.K), torch.float32, host=True, pinned=True) if pinned else None
        _ok(_lib.lib().hssfsst_stream_step(plan.handle, _ptr(tape), tape_len, hist, _ptr(x_new), chunk, 0 if pinned else 1, C, chunk,
                                           _ptr(out), _ptr(state), _ptr(out_host), _stream()), "hssfsst_stream_step")
        res = {"tape": tape, "out": out, "state": state}
        if pinned:
            res["out_host"] = out_host
        return res

    _add(f"stream_step: {nwin} points, {'pinned host' if pinned else 'device'} samples", "moments and streaming",
         {"hssfsst_stream_step": ("tape", "x_new", "out", "state") + (("out_host",) if pinned else ())}, make, call,
         inputs=("x_new",), outputs=("tape", "out", "state") + (("out_host",) if pinned else ()))


for _nwin, _band in ((256, (30, 52)), (128, BAND)):
    _stream_case(_nwin, _band, False)
    _stream_case(_nwin, _band, True)


# ---------------------------------------------------------------------------------------------------- resampler
_RS_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float64: _lib.DTYPE_F64}


def _resample_case(n, num, B, stride, starts_kind, host=False):
    """Dense resampling, every (x dtype, y dtype) pair plus labels.  starts_kind: None (frames `stride` apart), "host" or
    "device" (the same frames as a list).  ``host``: x, y and labels in host memory."""
    x_len = (B - 1) * stride + n
    starts = [b * stride for b in range(B)]

    def make():
        plan = ctypes.c_void_p()
        _ok(_lib.lib().hssfsst_resample_plan_create(ctypes.byref(plan), 0, n, num), "hssfsst_resample_plan_create")
        return plan, _rand((x_len,), 100, dtype=torch.float64)

    def call(ctx, A):
        plan, X = ctx
        res = {}
        st = A.inp("starts", _i64(starts), host=starts_kind == "host") if starts_kind else None
        for xd in (torch.float32, torch.float64):
            x = A.inp("x", X.to(xd), host=host)
            for yd in (torch.float32, torch.float64):
                y = A.out("y", (B, num), yd, host=host)
                labels = A.out("labels", (B, num), torch.int64, host=host)
                _ok(_lib.lib().hssfsst_resample_exec(plan, _ptr(x), _RS_DTYPES[xd], x_len, stride, _ptr(st), 1 if starts_kind == "device" else 0,
                                                     B, 0 if host else 1, _ptr(y), _RS_DTYPES[yd], _ptr(labels), 0 if host else 1, _stream()),
                    "hssfsst_resample_exec")
                res[f"y {xd} -> {yd}"], res[f"labels {xd} -> {yd}"] = y, labels
        return res

    what = {None: f"stride {stride}", "host": "host starts", "device": "device starts"}[starts_kind]
    _add(f"resample: {n} -> {num}, batch {B}, {what}{', host buffers' if host else ''}", "resampler",
         {"hssfsst_resample_exec": ("x", "y", "labels") + (("starts",) if starts_kind else ())}, make, call,
         inputs=("x",) + (("starts",) if starts_kind else ()), outputs=("y", "labels"))


_resample_case(9, 1, 1, 9, None)
for _n in (2000, 4097):                                  # (2000: both convolutions fit the LDS tier; 4097: the multi-pass tier)
    for _kind in (None, "host", "device"):
        _resample_case(_n, 1000, 3, 950, _kind)
_resample_case(2000, 1000, 3, 950, "host", host=True)


def _resample_ragged_case(host):
    lens, num = [1, 2, 300, 4097], 50

    def make():
        plan = ctypes.c_void_p()
        _ok(_lib.lib().hssfsst_resample_plan_create_ragged(ctypes.byref(plan), 0, num), "hssfsst_resample_plan_create_ragged")
        return plan, _rand((sum(lens),), 101, dtype=torch.float64)

    def call(ctx, A):
        plan, X = ctx
        res = {}
        st = A.inp("starts", _i64(_offsets(lens)[:-1]), host=True)
        ln = A.inp("lens", _i64(lens), host=True)
        for xd in (torch.float32, torch.float64):
            x = A.inp("x", X.to(xd), host=host)
            for yd in (torch.float32, torch.float64):
                y = A.out("y", (len(lens), num), yd, host=host)
                labels = A.out("labels", (len(lens), num), torch.int64, host=host)
                _ok(_lib.lib().hssfsst_resample_exec_ragged(plan, _ptr(x), _RS_DTYPES[xd], sum(lens), _ptr(st), _ptr(ln), len(lens),
                                                            0 if host else 1, _ptr(y), _RS_DTYPES[yd], _ptr(labels), 0 if host else 1, _stream()),
                    "hssfsst_resample_exec_ragged")
                res[f"y {xd} -> {yd}"], res[f"labels {xd} -> {yd}"] = y, labels
        return res

    _add(f"resample: ragged lengths {lens} to {num}{', host buffers' if host else ''}", "resampler",
         {"hssfsst_resample_exec_ragged": ("x", "starts", "lens", "y", "labels")}, make, call,
         inputs=("x", "starts", "lens"), outputs=("y", "labels"))


_resample_ragged_case(False)
_resample_ragged_case(True)


# ---------------------------------------------------------------------------------------------------- segmenter inference
def _lstm_weights(F, H, seed):
    """The eight arrays of one bidirectional layer in state_dict order, small enough that |h| stays an LSTM's."""
    out = []
    for d in range(2):
        out += [_rand((4 * H, F), seed + 4 * d, 0.2), _rand((4 * H, H), seed + 4 * d + 1, 0.2),
                _rand((4 * H,), seed + 4 * d + 2, 0.1), _rand((4 * H,), seed + 4 * d + 3, 0.1)]
    return out


def _pointer_table(A, name, tensors):
    """A host array of the tensors' addresses, itself carved."""
    return A.inp(name, _i64([t.data_ptr() for t in tensors]), host=True)


def _segmenter_plan(A, F, H, W1, W2, LW, LB):
    """hssfsst_segmenter_create from carved host arrays (read at creation only)."""
    w1 = [A.inp("lstm_1 array", w, host=True) for w in W1]
    w2 = [A.inp("lstm_2 array", w, host=True) for w in W2]
    t1, t2 = _pointer_table(A, "lstm_1", w1), _pointer_table(A, "lstm_2", w2)
    lw, lb = A.inp("linear_weight", LW, host=True), A.inp("linear_bias", LB, host=True)
    plan = ctypes.c_void_p()
    fpp = ctypes.POINTER(ctypes.c_void_p)
    _ok(_lib.lib().hssfsst_segmenter_create(ctypes.byref(plan), 0, F, H, ctypes.cast(t1.data_ptr(), fpp), ctypes.cast(t2.data_ptr(), fpp),
                                            _ptr(lw), _ptr(lb)), "hssfsst_segmenter_create")
    return plan


_SEG_DTYPES = ((torch.float32, _lib.DTYPE_F32), (torch.float16, _lib.DTYPE_F16), (torch.bfloat16, _lib.DTYPE_BF16))
_SEG_CREATE = ("lstm_1", "lstm_2", "linear_weight", "linear_bias")
_SEG_CREATE_BUFS = ("lstm_1 array", "lstm_2 array", "lstm_1", "lstm_2", "linear_weight", "linear_bias")


def _segmenter_case(B, T, H, F):
    def make():
        return (_lstm_weights(F, H, 200), _lstm_weights(2 * H, H, 220), _rand((4, 2 * H), 240, 0.3), _rand((4,), 241, 0.3),
                _rand((B, T, F), 242), _rand((2, B, H), 243, 0.5), _rand((2, B, H), 244, 0.5))

    def call(ctx, A):
        W1, W2, LW, LB, X, H0, C0 = ctx
        L = _lib.lib()
        plan = _segmenter_plan(A, F, H, W1, W2, LW, LB)
        res = {}
        try:
            h0, c0 = A.inp("h0", H0), A.inp("c0", C0)
            for dt, code in _SEG_DTYPES:
                feats = A.inp("feats", X.to(dt))
                logp = A.out("logp", (B, T, 4), torch.float32)
                _ok(L.hssfsst_segmenter_exec(plan, _ptr(feats), code, B, T, _ptr(h0), _ptr(c0), _ptr(logp), _stream()), "hssfsst_segmenter_exec")
                res[f"logp from {dt}"] = logp
            torch.cuda.synchronize()
        finally:
            L.hssfsst_segmenter_destroy(plan)
        return res

    _add(f"segmenter: batch {B}, {T} steps, hidden {H}, {F} features", "segmenter inference",
         {"hssfsst_segmenter_create": _SEG_CREATE, "hssfsst_segmenter_exec": ("feats", "h0", "c0", "logp")}, make, call,
         inputs=("feats", "h0", "c0") + _SEG_CREATE_BUFS)


_segmenter_case(1, 1, 240, 44)
_segmenter_case(17, 9, 12, 7)
_segmenter_case(3, 40, 256, 3)


def _segmenter_ragged_case(state_rows_one):
    lens, H, F = [1, 40, 17], 12, 7
    rows = 1 if state_rows_one else len(lens)

    def make():
        return (_lstm_weights(F, H, 300), _lstm_weights(2 * H, H, 320), _rand((4, 2 * H), 340, 0.3), _rand((4,), 341, 0.3),
                _rand((sum(lens), F), 342), _rand((2, rows, H), 343, 0.5), _rand((2, rows, H), 344, 0.5))

    def call(ctx, A):
        W1, W2, LW, LB, X, H0, C0 = ctx
        L = _lib.lib()
        plan = _segmenter_plan(A, F, H, W1, W2, LW, LB)
        res = {}
        try:
            h0, c0 = A.inp("h0", H0), A.inp("c0", C0)
            offs = A.inp("offsets", _i64(_offsets(lens)), host=True)
            for dt, code in _SEG_DTYPES:
                feats = A.inp("feats", X.to(dt))
                logp = A.out("logp", (sum(lens), 4), torch.float32)
                _ok(L.hssfsst_segmenter_exec_ragged(plan, _ptr(feats), code, ctypes.cast(offs.data_ptr(), ctypes.POINTER(ctypes.c_int64)), len(lens),
                                                    _ptr(h0), _ptr(c0), rows, _ptr(logp), _stream()), "hssfsst_segmenter_exec_ragged")
                res[f"logp from {dt}"] = logp
            torch.cuda.synchronize()
        finally:
            L.hssfsst_segmenter_destroy(plan)
        return res

    _add(f"segmenter: ragged lengths {lens}, state_rows {'1' if state_rows_one else 'count'}", "segmenter inference",
         {"hssfsst_segmenter_create": _SEG_CREATE, "hssfsst_segmenter_exec_ragged": ("feats", "offsets", "h0", "c0", "logp")}, make, call,
         inputs=("feats", "offsets", "h0", "c0"))


_segmenter_ragged_case(True)
_segmenter_ragged_case(False)


# ---------------------------------------------------------------------------------------------------- training layer
_BILSTM_W = ("weight_ih", "weight_hh", "bias_ih", "bias_hh")


def _bilstm_plan(A, F, H, W):
    L = _lib.lib()
    plan = ctypes.c_void_p()
    _ok(L.hssfsst_bilstm_create(ctypes.byref(plan), 0, F, H), "hssfsst_bilstm_create")
    dev = [A.inp(_BILSTM_W[i % 4], w) for i, w in enumerate(W)]
    table = _pointer_table(A, "weights", dev)
    _ok(L.hssfsst_bilstm_set_weights(plan, ctypes.cast(table.data_ptr(), ctypes.POINTER(ctypes.c_void_p)), _stream()), "hssfsst_bilstm_set_weights")
    return plan, dev


def _bilstm_case(B, T, H, F):
    """Forward, then backward from its stash, which is carved at exactly hssfsst_bilstm_stash_floats floats."""
    def make():
        return (_lstm_weights(F, H, 400), _rand((B, T, F), 420), _rand((2, B, H), 421, 0.5), _rand((2, B, H), 422, 0.5),
                _rand((B, T, 2 * H), 423), _rand((2, B, H), 424), _rand((2, B, H), 425))

    def call(ctx, A):
        W, X, H0, C0, DY, DHN, DCN = ctx
        L = _lib.lib()
        plan, held = _bilstm_plan(A, F, H, W)
        try:
            floats = ctypes.c_int64()
            _ok(L.hssfsst_bilstm_stash_floats(plan, B, T, ctypes.byref(floats)), "hssfsst_bilstm_stash_floats")
            x, h0, c0 = A.inp("x", X), A.inp("h0", H0), A.inp("c0", C0)
            y, hn, cn = A.out("y", (B, T, 2 * H), torch.float32), A.out("hn", (2, B, H), torch.float32), A.out("cn", (2, B, H), torch.float32)
            stash = A.work("stash", (floats.value,), torch.float32)
            _ok(L.hssfsst_bilstm_forward(plan, _ptr(x), B, T, _ptr(h0), _ptr(c0), _ptr(y), _ptr(hn), _ptr(cn), _ptr(stash), _stream()),
                "hssfsst_bilstm_forward")
            dy, dhn, dcn = A.inp("dy", DY), A.inp("dhn", DHN), A.inp("dcn", DCN)
            dgates = A.out("dgates", (2, B, T, 4 * H), torch.float32)
            dh0, dc0 = A.out("dh0", (2, B, H), torch.float32), A.out("dc0", (2, B, H), torch.float32)
            _ok(L.hssfsst_bilstm_backward(plan, _ptr(stash), _ptr(c0), _ptr(dy), _ptr(dhn), _ptr(dcn), B, T, _ptr(dgates), _ptr(dh0), _ptr(dc0),
                                          _stream()), "hssfsst_bilstm_backward")
            torch.cuda.synchronize()
        finally:
            L.hssfsst_bilstm_destroy(plan)
        return {"y": y, "hn": hn, "cn": cn, "dgates": dgates, "dh0": dh0, "dc0": dc0}

    _add(f"bilstm: batch {B}, {T} steps, hidden {H}, {F} features", "training layer",
         {"hssfsst_bilstm_set_weights": ("weights",), "hssfsst_bilstm_forward": ("x", "h0", "c0", "y", "hn", "cn", "stash"),
          "hssfsst_bilstm_backward": ("stash", "c0", "dy", "dhn", "dcn", "dgates", "dh0", "dc0")}, make, call,
         inputs=("x", "h0", "c0", "dy", "dhn", "dcn", "weights") + _BILSTM_W, outputs=("y", "hn", "cn", "dgates", "dh0", "dc0"))


_bilstm_case(3, 5, 12, 44)
_bilstm_case(17, 2, 256, 7)


def _bilstm_ragged_case():
    lens, H, F = [1, 7, 5], 12, 44
    B, total = len(lens), sum(lens)

    def make():
        return (_lstm_weights(F, H, 500), _rand((total, F), 520), _rand((2, B, H), 521, 0.5), _rand((2, B, H), 522, 0.5),
                _rand((total, 2 * H), 523), _rand((2, B, H), 524), _rand((2, B, H), 525))

    def call(ctx, A):
        W, X, H0, C0, DY, DHN, DCN = ctx
        L = _lib.lib()
        plan, held = _bilstm_plan(A, F, H, W)
        ip = ctypes.POINTER(ctypes.c_int64)
        try:
            offs = A.inp("offsets", _i64(_offsets(lens)), host=True)
            op = ctypes.cast(offs.data_ptr(), ip)
            floats = ctypes.c_int64()
            _ok(L.hssfsst_bilstm_stash_floats_ragged(plan, op, B, ctypes.byref(floats)), "hssfsst_bilstm_stash_floats_ragged")
            x, h0, c0 = A.inp("x", X), A.inp("h0", H0), A.inp("c0", C0)
            y, hn, cn = A.out("y", (total, 2 * H), torch.float32), A.out("hn", (2, B, H), torch.float32), A.out("cn", (2, B, H), torch.float32)
            stash = A.work("stash", (floats.value,), torch.float32)
            _ok(L.hssfsst_bilstm_forward_ragged(plan, _ptr(x), op, B, _ptr(h0), _ptr(c0), _ptr(y), _ptr(hn), _ptr(cn), _ptr(stash), _stream()),
                "hssfsst_bilstm_forward_ragged")
            dy, dhn, dcn = A.inp("dy", DY), A.inp("dhn", DHN), A.inp("dcn", DCN)
            dgates = A.out("dgates", (2, total, 4 * H), torch.float32)
            dh0, dc0 = A.out("dh0", (2, B, H), torch.float32), A.out("dc0", (2, B, H), torch.float32)
            _ok(L.hssfsst_bilstm_backward_ragged(plan, _ptr(stash), _ptr(c0), _ptr(dy), _ptr(dhn), _ptr(dcn), op, B, _ptr(dgates), _ptr(dh0),
                                                 _ptr(dc0), _stream()), "hssfsst_bilstm_backward_ragged")
            torch.cuda.synchronize()
        finally:
            L.hssfsst_bilstm_destroy(plan)
        return {"y": y, "hn": hn, "cn": cn, "dgates": dgates, "dh0": dh0, "dc0": dc0}

    _add(f"bilstm: ragged lengths {lens}", "training layer",
         {"hssfsst_bilstm_stash_floats_ragged": ("offsets",),
          "hssfsst_bilstm_forward_ragged": ("x", "offsets", "h0", "c0", "y", "hn", "cn", "stash"),
          "hssfsst_bilstm_backward_ragged": ("stash", "c0", "dy", "dhn", "dcn", "offsets", "dgates", "dh0", "dc0")}, make, call,
         inputs=("x", "offsets", "h0", "c0", "dy", "dhn", "dcn"), outputs=("y", "hn", "cn", "dgates", "dh0", "dc0"))


_bilstm_ragged_case()


# ---------------------------------------------------------------------------------------------------- sequence entries
SEQ_LENS = [1, 2, 63, 64, 65, 300]                       # both sides of a 64-step segment, one step, and a recording of several segments


def _seq_inputs(D, seed):
    """(log-probs (sum T, 4), labels, A with the cyclic zeros and -inf, pi, durations (4, D), edge (4, D)) on the host."""
    total = sum(SEQ_LENS)
    logp = torch.log_softmax(_rand((total, 4), seed, 2.0), dim=1)
    g = torch.Generator().manual_seed(seed + 1)
    labels = torch.randint(0, 4, (total,), generator=g, dtype=torch.uint8)
    A, pi = seq.cyclic_transitions()
    A, pi = torch.from_numpy(np.asarray(A, dtype=np.float32)), torch.from_numpy(np.asarray(pi, dtype=np.float32))
    dur, edge = -_rand((4, D), seed + 2).abs(), -_rand((4, D), seed + 3).abs()
    return logp, labels, A, pi, dur, edge


def _ip(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_int64))


def _fp(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))


def _ragged(logp):
    return RaggedFeatures(logp.cuda(), _i64(_offsets(SEQ_LENS)), 4, False)


def _decode_states_case():
    count, total = len(SEQ_LENS), sum(SEQ_LENS)

    def make():
        return _seq_inputs(1, 600)

    def call(ctx, A):
        LP, _, TA, PI, _, _ = ctx
        logp = A.inp("logp", LP)
        offs = A.inp("offsets", _i64(_offsets(SEQ_LENS)), host=True)
        ta, pi = A.inp("transitions", TA, host=True), A.inp("initial", PI, host=True)
        states, scores = A.out("states", (total,), torch.uint8), A.out("scores", (count,), torch.int64)
        _ok(_lib.lib().hssfsst_decode_states(_ptr(logp), _ip(offs), count, _fp(ta), _fp(pi), _ptr(states), _ptr(scores), 0, _stream()),
            "hssfsst_decode_states")
        return {"states": states, "scores": scores}

    def python(ctx):
        LP, _, TA, PI, _, _ = ctx
        return {"states": seq.decode_states(_ragged(LP), TA.numpy(), PI.numpy()).data}

    _add("sequence: decode_states", "sequence entries",
         {"hssfsst_decode_states": ("logp", "offsets", "transitions", "initial", "states", "scores")}, make, call,
         inputs=("offsets", "transitions", "initial"), outputs=("states",), python=python)


_decode_states_case()


def _decode_durations_case(D):
    count, total = len(SEQ_LENS), sum(SEQ_LENS)

    def make():
        return _seq_inputs(D, 610 + D)

    def call(ctx, A):
        LP, _, TA, PI, DUR, EDGE = ctx
        per = seq.decode_durations_info()[2]
        logp = A.inp("logp", LP)
        offs = A.inp("offsets", _i64(_offsets(SEQ_LENS)), host=True)
        ta, pi = A.inp("transitions", TA, host=True), A.inp("initial", PI, host=True)
        dur, edge = A.inp("durations", DUR, host=True), A.inp("edge", EDGE, host=True)
        states, scores = A.out("states", (total,), torch.uint8), A.out("scores", (count,), torch.int64)
        work = A.work("workspace", (per * (total + 8 * D),), torch.uint8)
        _ok(_lib.lib().hssfsst_decode_durations(_ptr(logp), _ip(offs), count, _fp(ta), _fp(pi), _fp(dur), _fp(edge), D, _ptr(states), _ptr(scores),
                                                _ptr(work), work.numel(), 0, _stream()), "hssfsst_decode_durations")
        return {"states": states, "scores": scores}

    def python(ctx):
        LP, _, TA, PI, DUR, EDGE = ctx
        return {"states": seq.decode_durations(_ragged(LP), DUR.numpy(), TA.numpy(), PI.numpy(), edge=EDGE.numpy()).data}

    _add(f"sequence: decode_durations, D {D}", "sequence entries",
         {"hssfsst_decode_durations": ("logp", "offsets", "transitions", "initial", "durations", "edge", "states", "scores", "workspace")},
         make, call, inputs=("offsets", "transitions", "initial", "durations", "edge"), outputs=("states",), python=python)


def _posteriors_case():
    count, total = len(SEQ_LENS), sum(SEQ_LENS)

    def make():
        return _seq_inputs(1, 620)

    def a_pi(ctx):
        return torch.cat([ctx[2].reshape(16), ctx[3].reshape(4)]).contiguous()

    def call(ctx, A):
        _, _, per, rec = seq.posteriors_info()
        logp, labels, tab = A.inp("logp", ctx[0]), A.inp("labels", ctx[1]), A.inp("a_pi", a_pi(ctx))
        offs = A.inp("offsets", _i64(_offsets(SEQ_LENS)), host=True)
        gamma = A.out("gamma", (total, 4), torch.float32)
        loglik, score = A.out("loglik", (count,), torch.float64), A.out("score", (count,), torch.float64)
        xi, gamma0 = A.out("xi", (count, 16), torch.float64), A.out("gamma0", (count, 4), torch.float64)
        work = A.work("work", (per * total + rec * count,), torch.uint8)
        _ok(_lib.lib().hssfsst_posteriors(_ptr(logp), _ip(offs), count, _ptr(tab), _ptr(labels), _ptr(gamma), _ptr(loglik), _ptr(score), _ptr(xi),
                                          _ptr(gamma0), _ptr(work), work.numel(), 0, _stream()), "hssfsst_posteriors")
        return {"gamma": gamma, "loglik": loglik, "score": score, "xi": xi, "gamma0": gamma0}

    def python(ctx):
        names = ("gamma", "loglik", "score", "xi", "gamma0")
        return dict(zip(names, seq._posteriors_run(ctx[0].cuda(), _offsets(SEQ_LENS), a_pi(ctx).cuda(), ctx[1].cuda(), tables_grad=True)))

    _add("sequence: posteriors", "sequence entries",
         {"hssfsst_posteriors": ("logp", "offsets", "a_pi", "labels", "gamma", "loglik", "score", "xi", "gamma0", "work")}, make, call,
         inputs=("offsets", "a_pi", "labels"), python=python)


def _duration_posteriors_case(D, counts):
    count, total = len(SEQ_LENS), sum(SEQ_LENS)
    entry = "hssfsst_posteriors_durations_counts" if counts else "hssfsst_posteriors_durations"

    def make():
        return _seq_inputs(D, 630 + D)

    def a_pi(ctx):
        return torch.cat([ctx[2].reshape(16), ctx[3].reshape(4)]).contiguous()

    def call(ctx, A):
        per, rec, per_d = seq.duration_counts_info()[:3] if counts else seq.duration_posteriors_info()[3:]
        logp, labels, tab = A.inp("logp", ctx[0]), A.inp("labels", ctx[1]), A.inp("a_pi", a_pi(ctx))
        dur, edge = A.inp("durations", ctx[4]), A.inp("edge", ctx[5])
        offs = A.inp("offsets", _i64(_offsets(SEQ_LENS)), host=True)
        gamma, onsets = A.out("gamma", (total, 4), torch.float32), A.out("onsets", (total, 4), torch.float32)
        loglik, score = A.out("loglik", (count,), torch.float64), A.out("score", (count,), torch.float64)
        xi, s0 = A.out("xi", (count, 16), torch.float64), A.out("s0", (count, 4), torch.float64)
        cnt = A.out("counts", (count, 2, 4, D), torch.float64) if counts else None
        work = A.work("work", (per * total + rec * count + per_d * D,), torch.uint8)
        head = (_ptr(logp), _ip(offs), count, _ptr(tab), _ptr(dur), _ptr(edge), D, _ptr(labels), _ptr(gamma), _ptr(onsets), _ptr(loglik),
                _ptr(score), _ptr(xi), _ptr(s0))
        tail = (_ptr(work), work.numel(), 0, _stream())
        _ok(getattr(_lib.lib(), entry)(*head, *(((_ptr(cnt),) if counts else ()) + tail)), entry)
        res = {"gamma": gamma, "onsets": onsets, "loglik": loglik, "score": score, "xi": xi, "s0": s0}
        if counts:
            res["counts"] = cnt
        return res

    def python(ctx):
        gamma, loglik, score, xi, s0, onsets, cnt = seq._duration_posteriors_run(
            ctx[0].cuda(), _offsets(SEQ_LENS), a_pi(ctx).cuda(), ctx[4].cuda(), ctx[5].cuda(), ctx[1].cuda(), tables_grad=True,
            want_onsets=True, want_counts=counts)
        res = {"gamma": gamma, "onsets": onsets, "loglik": loglik, "score": score, "xi": xi, "s0": s0}
        if counts:
            res["counts"] = cnt
        return res

    _add(f"sequence: posteriors_durations{'_counts' if counts else ''}, D {D}", "sequence entries",
         {entry: ("logp", "offsets", "a_pi", "durations", "edge", "labels", "gamma", "onsets", "loglik", "score", "xi", "s0", "work")
          + (("counts",) if counts else ())}, make, call, inputs=("offsets", "a_pi", "durations", "edge", "labels"), python=python)


_posteriors_case()
for _D in (1, 129):
    _decode_durations_case(_D)
    _duration_posteriors_case(_D, False)
    _duration_posteriors_case(_D, True)


def _score_case(per_recording):
    count, total = len(SEQ_LENS), sum(SEQ_LENS)
    groups = count if per_recording else 1

    def make():
        LP, LAB = _seq_inputs(1, 640)[:2]
        g = torch.Generator().manual_seed(641)
        states = torch.randint(0, 4, (total,), generator=g, dtype=torch.uint8)
        lab = LAB.clone()
        lab[::7] = 255                                   # ignored steps
        return LP, states, lab

    def call(ctx, A):
        per, rec, const = seq.score_info()[:3]
        logp, states, labels = A.inp("logp", ctx[0]), A.inp("states", ctx[1]), A.inp("labels", ctx[2])
        offs = A.inp("offsets", _i64(_offsets(SEQ_LENS)), host=True)
        confusion, ignored = A.out("confusion", (groups, 4, 4), torch.int64), A.out("ignored", (groups,), torch.int64)
        rank = A.out("rank", (groups, 4, 3), torch.int64)
        work = A.work("work", (per * total + rec * count + const,), torch.uint8)
        where = _lib.Launch(0, torch.cuda.current_stream().cuda_stream)
        _ok(_lib.lib().hssfsst_score_states(_ptr(logp), _ptr(states), _ptr(labels), _ip(offs), count, 1 if per_recording else 0, _ptr(confusion),
                                            _ptr(ignored), _ptr(rank), _ptr(work), work.numel(), ctypes.byref(where)), "hssfsst_score_states")
        return {"confusion": confusion, "ignored": ignored, "rank": rank}

    def python(ctx):
        off = _i64(_offsets(SEQ_LENS))
        s = seq.segmentation_scores(seq.RaggedStates(ctx[1].cuda(), off), seq.RaggedStates(ctx[2].cuda(), off), per_recording=per_recording,
                                    scores=_ragged(ctx[0]))
        shape = (lambda t: t) if per_recording else (lambda t: t.unsqueeze(0))
        return {"confusion": shape(s.confusion), "ignored": shape(s.ignored), "rank": shape(s.rank)}

    _add(f"sequence: score_states, {'per recording' if per_recording else 'pooled'}", "sequence entries",
         {"hssfsst_score_states": ("logp", "states", "labels", "offsets", "confusion", "ignored", "rank", "work")}, make, call,
         inputs=("states", "labels", "offsets"), python=python)


_score_case(False)
_score_case(True)


def _stitch_case():
    n, stride = 64, 32
    count, total = len(SEQ_LENS), sum(SEQ_LENS)
    rows = [seq._stitch_rows(T, n, stride) for T in SEQ_LENS]
    first = _offsets(rows)[:-1]

    def make():
        return torch.log_softmax(_rand((sum(rows), 4), 650, 2.0), dim=1), seq.window_weights(n)

    def call(ctx, A):
        win, w = A.inp("win_logp", ctx[0]), A.inp("weights", ctx[1])
        wf = A.inp("win_first", _i64(first), host=True)
        offs = A.inp("offsets", _i64(_offsets(SEQ_LENS)), host=True)
        out, dissent = A.out("out", (total, 4), torch.float32), A.out("dissent", (total,), torch.uint8)
        where = _lib.Launch(0, torch.cuda.current_stream().cuda_stream)
        _ok(_lib.lib().hssfsst_stitch_windows(_ptr(win), _ip(wf), sum(rows), _ip(offs), count, n, stride, _ptr(w), _lib.STITCH_PROB, _ptr(out),
                                              _ptr(dissent), where), "hssfsst_stitch_windows")
        return {"out": out, "dissent": dissent}

    def python(ctx):
        res, dis = seq.stitch_windows(ctx[0].cuda(), first, SEQ_LENS, n, stride, weights=ctx[1].cuda(), mode="prob", return_dissent=True)
        return {"out": res.data, "dissent": dis.data}

    _add("sequence: stitch_windows", "sequence entries",
         {"hssfsst_stitch_windows": ("win_logp", "win_first", "offsets", "weights", "out", "dissent")}, make, call,
         inputs=("win_first", "offsets", "weights"), outputs=("dissent",), python=python)


_stitch_case()
assert len({c.name for c in CASES}) == len(CASES)


# ---------------------------------------------------------------------------------------------------- (b): stated and refused
FAKE, ODD = 4096, 4100                                   # never dereferenced: a 16-byte aligned address, and one a float past it


def _refusal(entry, name, argtypes_index, args):
    """(entry, the refused pointer, its position in ``args``, a good call's arguments with fake non-NULL addresses)."""
    return dict(entry=entry, name=name, index=argtypes_index, args=args,
                text=f"{entry[len('hssfsst_'):]}: {name} is not 16-byte aligned")


_OFF2 = (ctypes.c_int64 * 3)(0, 3, 8)
REFUSALS = [
    _refusal("hssfsst_segmenter_exec", "logp", 7, [FAKE, FAKE, 0, 2, 3, FAKE, FAKE, FAKE, None]),
    _refusal("hssfsst_segmenter_exec_ragged", "logp", 8, [FAKE, FAKE, 0, _OFF2, 2, FAKE, FAKE, 2, FAKE, None]),
    _refusal("hssfsst_bilstm_forward", "stash", 9, [FAKE, FAKE, 2, 3, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None]),
    _refusal("hssfsst_bilstm_backward", "stash", 1, [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 3, FAKE, FAKE, FAKE, None]),
    _refusal("hssfsst_bilstm_forward_ragged", "stash", 9, [FAKE, FAKE, _OFF2, 2, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None]),
    _refusal("hssfsst_bilstm_backward_ragged", "stash", 1, [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, _OFF2, 2, FAKE, FAKE, FAKE, None]),
]
# The sequence entries state 16 bytes for these (8 or 4 for their float64 and float32 tables) and refuse otherwise; the refusals,
# text and order are recorded in tests/golden/sequence_entry_errors.json (the five with `int device`), tests/test_segmentation_scores.py
# and tests/test_stitch_windows.py.
STATED = {
    "hssfsst_decode_states": ("logp",),
    "hssfsst_decode_durations": ("logp", "workspace"),
    "hssfsst_posteriors": ("logp", "gamma", "work", "loglik", "score", "xi", "gamma0"),
    "hssfsst_posteriors_durations": ("logp", "gamma", "onsets", "work", "loglik", "score", "xi", "s0"),
    "hssfsst_posteriors_durations_counts": ("logp", "gamma", "onsets", "work", "loglik", "score", "xi", "s0", "counts"),
    "hssfsst_score_states": ("logp", "work", "confusion", "ignored", "rank"),
    "hssfsst_stitch_windows": ("win_logp", "out"),
}


# ---------------------------------------------------------------------------------------------------- the census' exemptions
HANDLE = "an opaque plan handle"
SCALAR = "a host-only scalar out-parameter or an *_info output"
STREAM = "the stream or communicator handle"
TEXT = "a text buffer"
RCCL = "hssfsst_allgather: the bounds are RCCL's, and more than one rank does not run here"
HOST_HELPER = "a CSV, pack or hssfsst_resample host helper: run under sanitizers in tests/native/"
ALLOWED_REASONS = (HANDLE, SCALAR, STREAM, TEXT, RCCL, HOST_HELPER)
EXEMPT = {
    ("hssfsst_allgather", "sendbuf"): RCCL, ("hssfsst_allgather", "recvbuf"): RCCL,
    ("hssfsst_parse_signal_csv", "text"): HOST_HELPER, ("hssfsst_parse_signal_csv", "signals"): HOST_HELPER,
    ("hssfsst_parse_signal_csv", "labels"): HOST_HELPER,
    ("hssfsst_pack_recordings", "ptrs"): HOST_HELPER, ("hssfsst_pack_recordings", "lens"): HOST_HELPER,
    ("hssfsst_pack_recordings", "stage"): HOST_HELPER, ("hssfsst_pack_recordings", "starts"): HOST_HELPER,
    ("hssfsst_resample", "x"): HOST_HELPER, ("hssfsst_resample", "y"): HOST_HELPER,
    ("hssfsst_plan_last_kernel", "buf"): TEXT,
    ("hssfsst_score_states", "where"): STREAM,
    # a buffer of the plan's pinned pool, lent by hssfsst_exec_pinned and named by its address: the library compares, never dereferences
    ("hssfsst_exec_pinned", "out"): SCALAR, ("hssfsst_pinned_release", "buf"): HANDLE,
    ("hssfsst_plan_timing", "ms_sum"): SCALAR, ("hssfsst_plan_timing", "nexec"): SCALAR,
    ("hssfsst_band", "klo"): SCALAR, ("hssfsst_band", "K"): SCALAR,
    ("hssfsst_plan_out_dtype", "out_dtype"): SCALAR,
    ("hssfsst_bilstm_stash_floats", "floats"): SCALAR, ("hssfsst_bilstm_stash_floats_ragged", "floats"): SCALAR,
}
