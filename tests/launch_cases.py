"""The launch shapes (csrc/fsst_launch_shape.hpp) seen from outside, as a table that tests/test_gpu_parity.py (which kernel each
shape runs) and tests/test_stream_order.py (the same shapes on a side stream) both walk.

A row is (name, case, the text of last_kernel() before " ["); ``case`` holds window length, fs, band, mode, n or ragged lengths
and extras.  The strings were recorded on an MI355X at the commit BEFORE the launch arithmetic moved into that header and are
what that commit ran: instantiation, flags, team size.  The grid is not part of them."""
import ctypes

import torch

from heart_sounds_segmentation_amd import _lib, synth
from heart_sounds_segmentation_amd.transforms import FSST

BAND = (25, 200)

_N128 = dict(nwin=128, fs=1000, band=BAND, mode="stack")
LAUNCH_CASES = [
    ("2 groups: below the team kernel", dict(_N128, n=32), "fsst_canon_kernel<4, 22, false>"),
    ("3 groups: its lower edge", dict(_N128, n=48), "fsst_team16_kernel<4, 22, 16, 2> teams of 1"),
    ("the workload's length", dict(_N128, n=2000), "fsst_team16_kernel<4, 22, 16, 2> teams of 16"),
    ("128 groups: the upper edge", dict(_N128, n=2048), "fsst_team16_kernel<4, 22, 16, 2> teams of 16"),
    ("129 groups: past it", dict(_N128, n=2064), "fsst_canon_kernel<4, 22, false>"),
    ("one CU per signal asked for", dict(_N128, n=2000, zpath="one_cu"), "fsst_canon_kernel<4, 22, false>"),
    ("two launches asked for", dict(_N128, n=2000, zpath="two_launch"), "fsst_canon_kernel<4, 22, false>"),
    ("float16 features", dict(_N128, n=2000, out_dtype=torch.float16), "fsst_team16_kernel<4, 22, 16, 2, f16> teams of 16"),
    ("the second canonical band", dict(_N128, fs=2000, band=(25, 400), n=400), "fsst_team16_kernel<2, 24, 16, 2> teams of 4"),
    ("odd K", dict(_N128, band=(25, 195), n=400), "fsst_core128_kernel<16, 8, 64, false, 16, -1, false>"),
    ("128 abs", dict(_N128, mode="abs", n=400), "fsst_core128_kernel<16, 8, 64, false, 16, -1, false>"),
    ("128 raw, every row", dict(_N128, mode="raw", band=None, n=400), "fsst_core128_kernel<16, 8, 64, false, 8, -1, false>"),
    ("256 stack", dict(_N128, nwin=256, n=400), "fsst_core128_kernel<16, 16, 64, false, 8, 3, false>"),
    ("256 raw, every row", dict(_N128, nwin=256, mode="raw", band=None, n=400), "fsst_core_kernel<8, 64>"),
    ("512 stack", dict(_N128, nwin=512, n=600), "fsst_core128_kernel<32, 16, 64, false, 6, -1, false, pairs>"),
    ("512 raw, every row", dict(_N128, nwin=512, mode="raw", band=None, n=600), "fsst_core_kernel<16, 64>"),
    ("100 points", dict(_N128, nwin=100, n=400), "fsst_dft_kernel<2>"),
    ("64 points", dict(_N128, nwin=64, n=400), "fsst_core_kernel<2, 64>"),
    ("32 points", dict(_N128, nwin=32, n=400), "fsst_core_kernel<1, 64>"),
    ("unnormalized, columns (16, 64)", dict(_N128, n=400, cols=(16, 64)), "fsst_canon_kernel<4, 22, false>"),
    ("unnormalized, columns (8, 64)", dict(_N128, n=400, cols=(8, 64)), "fsst_core128_kernel<16, 8, 64, true, 16, 3, false>"),
    ("ragged 128 stack", dict(_N128, ragged=[48, 2000, 333]), "fsst_canon_kernel<4, 22, false, ragged>"),
    ("ragged 256 raw", dict(_N128, nwin=256, mode="raw", band=None, ragged=[48, 2000, 333]), "fsst_core_kernel<8, 64>"),
]


def launch_transform(case):
    """The FSST object of a row (no plan yet): Kaiser(nwin, 0.5), the row's mode, band, element type and z-score path."""
    c = dict(case)
    return FSST(c["fs"], synth.kaiser_window(c["nwin"], 0.5), abs=c["mode"] == "abs", stack=c["mode"] == "stack",
                truncate_freq=c["band"], out_dtype=c.get("out_dtype", torch.float32))


def launch_inputs(case, seed=1234):
    """The row's input on the host: seeded noise, a list of signals for a ragged row, else one (2, n) batch."""
    g = torch.Generator().manual_seed(seed)
    if "ragged" in case:
        return [torch.randn(t, generator=g) for t in case["ragged"]]
    return [torch.randn(2, case["n"], generator=g)]


def launch_call(tf, case, xs):
    """The row's call on device inputs ``xs`` (launch_inputs, uploaded), on the current stream -> the output tensor."""
    if "ragged" in case:
        return tf.ragged(list(xs)).data
    if "zpath" in case:
        tf.set_zpath(case["zpath"])
    if "cols" in case:
        return tf.unnormalized(xs[0], cols=case["cols"])
    return tf.batch(xs[0])


def launch_kernel(tf, case):
    """last_kernel() of the plan the row's call ran."""
    mode = _lib.MODE_STACK_UNNORM if "cols" in case else None
    buf = ctypes.create_string_buffer(160)
    _lib.check(_lib.lib().hssfsst_plan_last_kernel(tf._plan(0, mode).handle, buf, len(buf)), "hssfsst_plan_last_kernel")
    return buf.value.decode()


def run_launch_case(case):
    """One row of LAUNCH_CASES on cuda:0 -> (last_kernel() of the plan that ran, the output's bytes).  Kaiser(nwin, 0.5), seeded
    noise, batch 2."""
    tf = launch_transform(case)
    out = launch_call(tf, case, [x.cuda() for x in launch_inputs(case)])
    torch.cuda.synchronize()
    name = launch_kernel(tf, case)
    out = torch.view_as_real(out) if out.is_complex() else out
    return name, out.contiguous().view(torch.uint8).cpu().numpy().tobytes()
