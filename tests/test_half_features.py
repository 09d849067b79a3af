"""STACK features in float16 / bfloat16 straight from the kernels: hssfsst_plan_create_ex (C ABI), FSST(out_dtype=...) and the
corpus builder that follows it.

The contract: a half-precision STACK result equals the float32 result of the same call cast with Tensor.to(dtype) -- every finite
element bit for bit, NaN exactly where float32 has NaN.  CPU tests check the ABI, the argument errors (before any device is
touched), pickling, the code-object check of the new team instantiations and the gather of a half arena; GPU tests check the
contract on every z-score path and entry point."""
import ctypes
import os
import pickle
import re
import socket

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, synth
from heart_sounds_segmentation_amd.transforms import FSST

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hssfsst.h")
W128 = synth.kaiser_window(128, 0.5)
HALF = (torch.float16, torch.bfloat16)
DEV = "cuda"


def same_as_cast(got, f32, dt):
    """got == f32.to(dt): finite elements bit for bit, NaN exactly where f32 has NaN (payloads may differ)."""
    want = f32.to(dt)
    if got.dtype != dt or got.shape != want.shape:
        return False
    got, want = got.cpu(), want.cpu()
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    if not torch.equal(nan_g, nan_w):
        return False
    gb, wb = got.contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    return torch.equal(gb[~nan_g], wb[~nan_w])


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_and_library_export_the_half_abi(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    assert re.search(r"#define HSSFSST_DTYPE_F16 2\b", text) and re.search(r"#define HSSFSST_DTYPE_BF16 3\b", text)
    assert "int hssfsst_plan_create_ex(" in text and "int hssfsst_plan_out_dtype(" in text
    assert int(re.search(r"#define HSSFSST_VERSION (\d+)", text).group(1)) == 210
    assert built_lib.hssfsst_version() == 210
    assert (_lib.DTYPE_F32, _lib.DTYPE_F64, _lib.DTYPE_F16, _lib.DTYPE_BF16) == (0, 1, 2, 3)
    for name in ("hssfsst_plan_create_ex", "hssfsst_plan_out_dtype"):
        assert getattr(built_lib, name).restype is ctypes.c_int
    assert len(built_lib.hssfsst_plan_create_ex.argtypes) == 10
    assert built_lib.hssfsst_plan_out_dtype(None, None) == _lib.E_INVAL


def test_create_ex_rejects_bad_dtypes_before_any_device(built_lib):
    """EINVAL (not ENODEVICE): the checks come before the device is looked at, so they hold on a machine without one."""
    plan = ctypes.c_void_p()
    w = np.ascontiguousarray(W128)
    wp = w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for mode in (_lib.MODE_RAW, _lib.MODE_ABS, _lib.MODE_STACK_UNNORM):
        for dt in (_lib.DTYPE_F16, _lib.DTYPE_BF16):
            rc = built_lib.hssfsst_plan_create_ex(ctypes.byref(plan), 0, 128, wp, 1000.0, 1, 25.0, 200.0, mode, dt)
            assert rc == _lib.E_INVAL and not plan.value, (mode, dt, rc)
            assert b"STACK" in built_lib.hssfsst_last_error()
    for dt in (_lib.DTYPE_F64, -1, 7):
        rc = built_lib.hssfsst_plan_create_ex(ctypes.byref(plan), 0, 128, wp, 1000.0, 1, 25.0, 200.0, _lib.MODE_STACK, dt)
        assert rc == _lib.E_INVAL and not plan.value, (dt, rc)


def test_fsst_out_dtype_argument_errors():
    with pytest.raises(ValueError):
        FSST(1000, W128, abs=True, stack=True, truncate_freq=(25, 200), out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        FSST(1000, W128, abs=True, truncate_freq=(25, 200), out_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        FSST(1000, W128, truncate_freq=(25, 200), out_dtype=torch.float16)        # raw transform
    with pytest.raises(ValueError):
        FSST(1000, W128, stack=True, truncate_freq=(25, 200), out_dtype=torch.float64)
    assert FSST(1000, W128, stack=True).out_dtype == torch.float32                  # the default is today's float32
    assert FSST(1000, W128, stack=True, out_dtype=torch.float16).out_dtype == torch.float16


def test_half_fsst_pickles_with_its_out_dtype():
    tf = FSST(1000, W128, stack=True, truncate_freq=(25, 200), out_dtype=torch.bfloat16)
    tf2 = pickle.loads(pickle.dumps(tf))
    assert tf2.out_dtype == torch.bfloat16 and tf2.stack and not tf2.abs and tf2.truncate_freq == (25, 200)
    assert tf2._plans == {}


def test_code_object_check_covers_the_half_team_kernels(built_lib):
    chk = _lib.check_code_object()
    assert chk["kernels"] >= 6, chk                  # <4, 22, ..> and <2, 24, ..> x {float32, f16, bf16}
    assert chk.get("metadata_checked", 0) >= 6, chk


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, tmp):
    import torch.distributed as dist
    from heart_sounds_segmentation_amd.corpus import FrameItems, gather_features
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    rows = 3 if rank == 0 else 2
    g = torch.Generator().manual_seed(rank)
    local = torch.randn((rows, 5, 6), generator=g).to(torch.bfloat16)
    local[0, 0, 0] = float("nan")
    full = gather_features(FrameItems(local, None))
    # a rank without frames passes an empty list: it learns shape and dtype from the others
    part = gather_features(FrameItems(local, None) if rank == 0 else [])
    torch.save({"full": full, "local": local, "part": part}, os.path.join(tmp, f"g{rank}.pt"))
    dist.destroy_process_group()


def test_gather_features_carries_a_bfloat16_arena(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_gather_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "g0.pt"), torch.load(tmp_path / "g1.pt")
    want = torch.cat([r0["local"], r1["local"]])
    for r in (r0, r1):
        assert r["full"].dtype == torch.bfloat16 and r["full"].shape == (5, 5, 6)
        assert torch.equal(r["full"].view(torch.int16), want.view(torch.int16))
        assert r["part"].dtype == torch.bfloat16 and r["part"].shape == (3, 5, 6)
        assert torch.equal(r["part"].view(torch.int16), r0["local"].view(torch.int16))


# ---------------------------------------------------------------------------------------------------- GPU
def pair(band=(25, 200), fs=1000, w=W128, dt=torch.bfloat16):
    return (FSST(fs, w, stack=True, truncate_freq=band, device=DEV),
            FSST(fs, w, stack=True, truncate_freq=band, device=DEV, out_dtype=dt))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("band,fs", [((25, 200), 1000), ((25, 400), 2000)])
def test_every_zpath_of_the_canonical_bands(dt, band, fs):
    f32, fh = pair(band, fs, dt=dt)
    X = torch.from_numpy(synth.pcg_windows(64, 2000, fs=fs, seed=11)).to(DEV)
    for zp in ("auto", "team", "two_launch", "one_cu"):
        f32.set_zpath(zp)
        fh.set_zpath(zp)
        want = f32.batch(X)
        got = fh.batch(X)
        assert same_as_cast(got, want, dt), (zp, fh.last_kernel())
        if zp in ("auto", "team"):
            assert "fsst_team16_kernel" in fh.last_kernel() and ("bf16" if dt is torch.bfloat16 else "f16") in fh.last_kernel()
        fh.check()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF)
def test_batch_sizes_and_inputs(dt):
    f32, fh = pair(dt=dt)
    for B in (1, 3, 50, 1024):
        for X in (synth.pcg_windows(B, 2000, seed=B), synth.noise_windows(B, 2000, seed=B + 1)):
            Xd = torch.from_numpy(X).to(DEV)
            assert same_as_cast(fh.batch(Xd), f32.batch(Xd), dt), B
    X = torch.from_numpy(synth.pcg_windows(3, 2000, seed=5))                         # host in, host out
    got = fh.batch(X)
    assert got.device.type == "cpu" and same_as_cast(got, f32.batch(X), dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF)
def test_other_windows_and_bands(dt):
    X = torch.from_numpy(synth.pcg_windows(20, 2000, seed=21)).to(DEV)
    cases = [(W128, (25, 180)), (W128, (25, 210))]
    cases += [(synth.kaiser_window(nw, 0.5), (25, 200)) for nw in (32, 64, 256, 512)]
    cases += [(np.hanning(100), (25, 200))]                                           # any-length kernel
    for w, band in cases:
        f32, fh = pair(band, 1000, w, dt)
        assert same_as_cast(fh.batch(X), f32.batch(X), dt), (len(w), band, fh.last_kernel())
    # the element-by-element path of the sweep: an odd band and an odd n, 129 * 42 elements per signal, not a multiple of 4
    f32, fh = pair((25, 190), 1000, W128, dt)
    assert fh.band()[1] % 2 == 1
    f32.set_zpath("two_launch")
    fh.set_zpath("two_launch")
    X = torch.from_numpy(synth.pcg_windows(3, 129, seed=22)).to(DEV)
    assert same_as_cast(fh.batch(X), f32.batch(X), dt), fh.last_kernel()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF)
def test_single_frames_lent_copied_and_on_device(dt):
    f32, fh = pair(dt=dt)
    X = torch.from_numpy(synth.pcg_windows(100, 2000, seed=31))
    want = f32.batch(X.to(DEV)).cpu()
    kept = [fh(X[i].reshape(2000, 1)) for i in range(100)]                           # > 64: the lent pool runs dry, copies follow
    for i, r in enumerate(kept):
        assert r.device.type == "cpu" and r.shape == (2000, 44)
        assert same_as_cast(r, want[i], dt), i
    del kept
    one = fh(X[7].to(DEV))
    assert one.is_cuda and same_as_cast(one, want[7], dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF)
def test_frames_list_and_column_ranges(dt):
    from heart_sounds_segmentation_amd.framing import frame_starts
    f32, fh = pair(dt=dt)
    recs = [synth.recording(T, seed=40 + i) for i, T in enumerate((35500, 4100, 12345))]
    x = torch.from_numpy(np.concatenate(recs)).to(DEV)
    starts, base = [], 0
    for r in recs:
        starts.append(frame_starts(len(r), 1000, 2000)[0] + base)
        base += len(r)
    st = torch.from_numpy(np.concatenate(starts))
    assert same_as_cast(fh.frames(x, st, 2000), f32.frames(x, st, 2000), dt)
    assert same_as_cast(fh.frames(x, st.to(DEV), 2000), f32.frames(x, st.to(DEV), 2000), dt)
    X = torch.from_numpy(synth.pcg_windows(9, 2000, seed=41)).to(DEV)
    for col0 in (16, 7):
        assert same_as_cast(fh._run(X, cols=(col0, 1500)), f32._run(X, cols=(col0, 1500)), dt), col0


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF)
@pytest.mark.parametrize("nwin,band,lens", [pytest.param(128, (25, 200), (1, 127, 2000, 35500, 60001), id="128"),
                                           pytest.param(64, (25, 200), (1, 127, 2000, 35500, 60001), id="64"),
                                           pytest.param(100, (25, 200), (1, 127, 2000, 35500, 60001), id="100"),
                                           pytest.param(128, (25, 190), (1, 3, 17, 130), id="128-odd-band")])
def test_ragged_mixed_lengths(dt, nwin, band, lens):
    """nwin 128: one ragged launch (MFMA kernels); nwin 64 and the any-length kernel (100): one exec per recording inside the
    library, each writing at its own element offset of the half arena.  The odd band (21 rows, 42 elements per sample): the second
    and later signals start 2 elements into a 4-element group, so the sweep's head, tail and wrap code runs; and once more into an
    out= that is not 8-byte aligned."""
    w = W128 if nwin == 128 else synth.kaiser_window(64, 0.5) if nwin == 64 else np.hanning(100)
    f32, fh = pair(band=band, w=w, dt=dt)
    odd = band == (25, 190)
    if odd:
        assert fh.band()[1] % 2 == 1
    xs = [torch.from_numpy(synth.recording(T, seed=50 + i)) for i, T in enumerate(lens)]
    for src in (xs, [t.to(DEV) for t in xs]):
        a, b = f32.ragged(src), fh.ragged(src)
        assert b.data.dtype == dt
        for i in range(len(lens)):
            assert same_as_cast(b[i], a[i], dt), (nwin, i)
        pa, pb = a.padded(), b.padded()
        assert pb.dtype == dt and same_as_cast(pb, pa, dt)
    if odd:
        dev = [t.to(DEV) for t in xs]
        r32 = f32.ragged(dev)
        for i, x in enumerate(dev):                                                  # float32: each signal alone
            assert torch.equal(r32[i].view(torch.int32), f32.batch(x.reshape(1, -1))[0].view(torch.int32)), i
        C, n, canary = 2 * fh.band()[1], sum(lens) * 2 * fh.band()[1], 4096
        buf = torch.full((1 + n + canary,), 1234.0, dtype=dt, device=DEV)
        out = buf[1:1 + n].view(-1, C)
        assert out.data_ptr() % 8 != 0
        fh.ragged(dev, out=out)
        assert same_as_cast(out, r32.data, dt)
        assert bool((buf[:1] == 1234.0).all()) and bool((buf[1 + n:] == 1234.0).all())     # (compared in dt: bfloat16 holds 1234 as 1232)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF)
def test_out_arguments_stop_at_the_result(dt):
    """A half out= tensor with a 4 KiB canary tail: nothing past the result is touched."""
    f32, fh = pair(dt=dt)
    canary = 4096
    X = torch.from_numpy(synth.pcg_windows(5, 2000, seed=61)).to(DEV)
    n = 5 * 2000 * 44
    buf = torch.full((n + canary,), 1234.0, dtype=dt, device=DEV)
    fh.batch(X, out=buf[:n].view(5, 2000, 44))
    assert same_as_cast(buf[:n].view(5, 2000, 44), f32.batch(X), dt) and bool((buf[n:] == 1234.0).all())
    x = torch.from_numpy(synth.recording(9000, seed=62)).to(DEV)
    st = torch.tensor([0, 1000, 3500, 7000])
    n = 4 * 2000 * 44
    buf = torch.full((n + canary,), 1234.0, dtype=dt, device=DEV)
    fh.frames(x, st, 2000, out=buf[:n].view(4, 2000, 44))
    assert same_as_cast(buf[:n].view(4, 2000, 44), f32.frames(x, st, 2000), dt) and bool((buf[n:] == 1234.0).all())
    xs = [torch.from_numpy(synth.recording(T, seed=63 + i)).to(DEV) for i, T in enumerate((333, 2000, 5001))]
    n = (333 + 2000 + 5001) * 44
    buf = torch.full((n + canary,), 1234.0, dtype=dt, device=DEV)
    fh.ragged(xs, out=buf[:n].view(-1, 44))
    assert same_as_cast(buf[:n].view(-1, 44), f32.ragged(xs).data, dt) and bool((buf[n:] == 1234.0).all())
    with pytest.raises(ValueError):                                                  # a float32 out= is not reinterpreted
        fh.batch(X, out=torch.empty((5, 2000, 44), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        fh.ragged(xs, out=torch.empty((7334, 44), dtype=torch.float32, device=DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF)
def test_all_zero_window_is_nan(dt):
    f32, fh = pair(dt=dt)
    X = torch.from_numpy(synth.pcg_windows(4, 2000, seed=71)).to(DEV)
    X[2] = 0.0
    want, got = f32.batch(X), fh.batch(X)
    assert torch.isnan(want[2]).all() and torch.isnan(got[2]).all()
    assert same_as_cast(got, want, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", HALF)
def test_corpus_builders_follow_the_transform(dt):
    from heart_sounds_segmentation_amd.corpus import build_features, build_recordings
    from heart_sounds_segmentation_amd.transforms import Resample
    f32, fh = pair(dt=dt)
    lens = [35500, 4100, 2000, 12345, 1999]
    recs = [(torch.from_numpy(synth.recording(T, seed=80 + i)), torch.randint(1, 5, (T,), generator=torch.Generator().manual_seed(i)))
            for i, T in enumerate(lens)]
    for kw in ({}, {"resample": Resample(1000)}):
        for keep in (False, True):
            a = build_features(recs, f32, windows_per_launch=16, keep_on_device=keep, **kw)
            b = build_features(recs, fh, windows_per_launch=16, keep_on_device=keep, **kw)
            assert b.features.dtype == dt and b.features.is_cuda == keep
            assert same_as_cast(b.features, a.features, dt), (kw, keep)
            assert torch.equal(a.labels, b.labels)
            x0, _ = b[3]
            assert x0.dtype == dt
    for keep in (False, True):
        a = build_recordings(recs, f32, keep_on_device=keep)
        b = build_recordings(recs, fh, keep_on_device=keep)
        assert len(a) == len(b) == len(recs)
        for i in range(len(recs)):
            assert same_as_cast(b[i][0], a[i][0], dt) and torch.equal(a[i][1], b[i][1])


_FALLBACK_CHILD = r"""
import sys, torch
from heart_sounds_segmentation_amd import FSST, synth
from tests.test_half_features import same_as_cast
w = synth.kaiser_window(128, 0.5)
for dt in (torch.float16, torch.bfloat16):
    f32 = FSST(1000, w, truncate_freq=(25, 200), stack=True)
    fh = FSST(1000, w, truncate_freq=(25, 200), stack=True, out_dtype=dt)
    # device batches: the team launch finds itself given up and the kernels queued behind it, gated on that event, compute the exec
    # (2000-sample signals; 500-sample ones take the same gated transform + statistics + z-score launches)
    for n in (2000, 500):
        X = torch.from_numpy(synth.pcg_windows(40, n, seed=5)).cuda()
        ok = same_as_cast(fh.batch(X), f32.batch(X), dt)
        # (check() synchronises; fallbacks() samples the plan's give-up word, which names the LAST launch that gave up: once per exec)
        print("BATCH", n, ok, "PATH", fh.check(), "FALLBACKS", fh.fallbacks(), "KERNEL", fh.last_kernel())
    # one CPU frame: no gated launches; the host sees the give-up word and redoes the exec itself
    x = torch.from_numpy(synth.pcg_windows(1, 2000, seed=7)[0]).reshape(2000, 1)
    one = fh(x)
    print("ONE", one.device.type == "cpu" and same_as_cast(one, f32(x), dt), "FALLBACKS", fh.fallbacks())
"""


@pytest.mark.gpu
def test_gated_fallback_writes_half_features(tmp_path):
    """HSSFSST_TEAM_FORCE_FALLBACK=1 (a child process): every team launch finds itself given up.  Half plans then take the gated
    two-launch kernels -- float32 into the plan's scratch, the out-of-place sweep into the 2-byte output -- and, for a single CPU
    frame, the host's re-exec.  Same bits as the float32 result cast."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _FALLBACK_CHILD], cwd=root, env=dict(os.environ, HSSFSST_TEAM_FORCE_FALLBACK="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    lines = r.stdout.splitlines()
    batches = [ln for ln in lines if ln.startswith("BATCH")]
    ones = [ln for ln in lines if ln.startswith("ONE")]
    assert len(batches) == 4 and all(" True " in ln for ln in batches), r.stdout
    assert len(ones) == 2 and all(ln.startswith("ONE True") for ln in ones), r.stdout
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        # every team launch was given up: the two device batches, then the frame (the paths are those of the float32 test,
        # test_gpu_parity.py::test_team_kernel_fallback_and_other_processes)
        assert [ln.split(" KERNEL")[0] for ln in batches] == ["BATCH 2000 True PATH 2 FALLBACKS 1", "BATCH 500 True PATH 2 FALLBACKS 2"] * 2, r.stdout
        assert all(ln == "ONE True FALLBACKS 3" for ln in ones), r.stdout
