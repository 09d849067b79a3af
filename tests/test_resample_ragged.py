"""Ragged resampling (hssfsst_resample_plan_create_ragged / hssfsst_resample_exec_ragged, csrc/fourier_resample_ragged.hpp): signals of
different lengths, every one to `num` samples, in one call -- Resample.ragged, resample_labels_ragged and
corpus.build_resampled_recordings (the reference's lazy dataset with Compose([Resample(num), FSST(...)])).

CPU tests check the C ABI's argument handling and the Python surface without a device; GPU tests (one process) check the rows
against the host helper, the golden fixtures and the dense device plan, their determinism, the label rule and the builder."""
import ctypes
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, synth
from heart_sounds_segmentation_amd.corpus import CorpusBuilder, build_resampled_recordings
from heart_sounds_segmentation_amd.transforms import FSST, Resample
from heart_sounds_segmentation_amd.transforms.resample import resample_labels, resample_labels_ragged

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "resample.npz"))
CASES = sorted({k.split("__")[0] for k in GOLD.files if k.endswith("__x")})
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hssfsst.h")
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")
W128 = synth.kaiser_window(128, 0.5)
NEW_ENTRY_POINTS = ("hssfsst_resample_plan_create_ragged", "hssfsst_resample_exec_ragged")


def label_tracks(lens, seed):
    """Label tracks as the corpus has them: cyclic 1 -> 2 -> 3 -> 4 runs of random lengths (int64)."""
    rng = np.random.default_rng(seed)
    out = []
    for T in lens:
        y = np.empty(T, dtype=np.int64)
        pos, state = 0, int(rng.integers(1, 5))
        while pos < T:
            run = int(rng.integers(20, 400))
            y[pos:pos + run] = state
            pos += run
            state = state % 4 + 1
        out.append(torch.from_numpy(y))
    return out


def off_tie(raw32):
    """Where the float32 value the label rule rounds is not within 1e-9 of a .5 tie."""
    r = np.asarray(raw32).astype(np.float64)
    return np.abs(r - np.floor(r) - 0.5) > 1e-9


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def signals(lens, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(rng.standard_normal(T).astype(dtype)) for T in lens]


# ---------------------------------------------------------------------------------------------------- CPU
def test_entry_points_declared_and_bound(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    for name in NEW_ENTRY_POINTS:
        assert f"{name}(" in text, name
        fn = getattr(built_lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes
    assert len(built_lib.hssfsst_resample_exec_ragged.argtypes) == 13


def test_header_version_still_210(built_lib):
    with open(HEADER) as fh:
        assert "#define HSSFSST_VERSION 210" in fh.read()
    assert built_lib.hssfsst_version() == 210


def test_plan_create_ragged_errors_without_a_device(built_lib):
    h = ctypes.c_void_p()
    for num in (0, -1, -1000):
        assert built_lib.hssfsst_resample_plan_create_ragged(ctypes.byref(h), 0, num) == _lib.E_INVAL
        assert not h.value
    assert built_lib.hssfsst_resample_plan_create_ragged(None, 0, 10) == _lib.E_INVAL
    assert built_lib.hssfsst_resample_plan_create_ragged(ctypes.byref(h), -1, 10) == _lib.E_INVAL
    assert built_lib.hssfsst_resample_plan_create_ragged(ctypes.byref(h), 0, (1 << 26) + 1) == _lib.E_UNSUPPORTED
    assert not h.value


def test_null_plan_is_einval(built_lib):
    x = (ctypes.c_float * 8)()
    y = (ctypes.c_float * 8)()
    st = (ctypes.c_int64 * 2)(0, 4)
    ln = (ctypes.c_int64 * 2)(4, 4)
    assert built_lib.hssfsst_resample_exec_ragged(None, x, 0, 8, st, ln, 2, 0, y, 0, None, 0, None) == _lib.E_INVAL
    assert built_lib.hssfsst_resample_exec_ragged(None, x, 0, 8, st, ln, 0, 0, y, 0, None, 0, None) == _lib.E_INVAL


def test_python_argument_errors_before_any_plan():
    t = Resample(100)
    bad = [
        (lambda: t.ragged(torch.zeros(10)), "needs lengths="),
        (lambda: t.ragged(torch.zeros(10), lengths=[5, 0, 5]), ">= 1"),
        (lambda: t.ragged(torch.zeros(10), lengths=[5, 6]), "lengths sum to 11"),
        (lambda: t.ragged([torch.zeros(5)], lengths=[5]), "goes with one packed buffer"),
        (lambda: t.ragged([torch.zeros(5), torch.zeros(0)]), "signal 1 is empty"),
        (lambda: t.ragged([torch.zeros(5), torch.zeros(3, 2)]), "expected \\(T,\\)"),
        (lambda: t.ragged([torch.zeros(5), torch.zeros(6, device="meta")]), "different devices"),
        (lambda: t.ragged([torch.zeros(5), torch.zeros(6, dtype=torch.complex64)]), "complex"),
        (lambda: t.ragged(torch.zeros(6, dtype=torch.complex64), lengths=[6]), "complex"),
        (lambda: t.ragged([torch.zeros(5)], dtype=torch.float16), "float32 or float64"),
        (lambda: t.ragged([torch.zeros(5)], out=torch.empty(2, 100)), "out must be"),
        (lambda: Resample(0).ragged([torch.zeros(5)]), "num=0"),
    ]
    for fn, msg in bad:
        with pytest.raises(ValueError, match=msg):
            fn()
    assert t._plans == {}
    # an empty list needs no device
    e = t.ragged([])
    assert e.shape == (0, 100) and e.dtype == torch.float32
    assert t.ragged([], labels=True).dtype == torch.int64
    assert t._plans == {}


def test_builder_argument_errors_before_any_plan():
    rs = Resample(100)
    tf = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    raw = FSST(1000, W128, truncate_freq=(25, 200))
    x, y = torch.zeros(3000), torch.ones(3000, dtype=torch.int64)
    dev = torch.device("cuda", 0)
    cases = [
        (lambda: build_resampled_recordings([(x, y), (x, None)], tf, rs, device=dev), "labels for all or for none"),
        (lambda: build_resampled_recordings([(x, y)], raw, rs, device=dev), "stack=True or abs=True"),
        (lambda: build_resampled_recordings([(x.to(torch.complex64), None)], tf, rs, device=dev), "expected real"),
        (lambda: build_resampled_recordings([(torch.zeros(0), None)], tf, rs, device=dev), "T >= 1"),
        (lambda: build_resampled_recordings([(x, y[:10])], tf, rs, device=dev), "labels of recording 0"),
        (lambda: build_resampled_recordings([(x, y)], tf, rs, device="cpu"), "not a HIP device"),
        (lambda: CorpusBuilder(tf, device=dev).build_resampled_recordings([(x, y)]), "no resample="),
    ]
    for fn, msg in cases:
        with pytest.raises(ValueError, match=msg):
            fn()
    assert rs._plans == {} and not getattr(tf, "_plans", None)


def test_pickles_without_ragged_plans():
    t = Resample(1000, device="cuda")
    t._plans[("ragged", os.getpid(), 0, 1000)] = object()
    u = pickle.loads(pickle.dumps(t))
    assert u.num == 1000 and u._plans == {}
    assert t._plans


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a visible GPU")
def test_ragged_without_device_raises_like_batch(built_lib):
    with pytest.raises(RuntimeError, match="no HIP device"):
        Resample(1000).ragged([torch.zeros(2000), torch.zeros(3000)])


def test_layout_planner_under_sanitizers(tmp_path):
    """csrc/fourier_resample_layout.hpp alone, in a program of its own (tests/native/resample_layout_check.cpp) built with
    -fsanitize=address,undefined: lists [1], 16 equal, LENS and 1 000 pseudo-random lengths, each to num 1, 1 000 and 20 000 under the
    library's budget, two that force several chunks and one below any signal's work (one signal per chunk).  Chunks, tables,
    offsets, descriptors, Mt and max_elems equal the loop that used to stand inline in hssfsst_resample_exec_ragged; every signal in
    exactly one chunk, the order stable, a chunk within the budget unless it holds one signal, each descriptor's table that of its own
    length, its row its list index, its start taken from the staged span.  The dense chunk rule against its inline form, and
    bluestein_tables for N in {1, 2, 3, 5, 64, 4097}."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "resample_layout_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "resample_layout_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "resample layout ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------- GPU
DEV = "cuda:0"
LENS = [1, 2, 3, 127, 128, 129, 2000, 4096, 4097, 8191, 35500, 60001, 240000, 2000, 129, 35500, 1]
NUMS = [1, 2, 1000, 1001, 17750, 120000]


def host(x, num):
    return Resample(num)(torch.as_tensor(x), torch.float64).numpy()


def rel_err(got, ref):
    return float(np.abs(np.asarray(got) - ref).max() / max(np.abs(ref).max(), 1.0))


@pytest.mark.gpu
def test_mixed_list_against_host_helper():
    xs = signals(LENS, 7)
    for num in NUMS:
        t = Resample(num)
        y64 = t.ragged([x.to(DEV) for x in xs], dtype=torch.float64)
        assert y64.shape == (len(LENS), num) and y64.dtype == torch.float64 and y64.device == torch.device(DEV)
        Y = y64.cpu().numpy()
        for i, x in enumerate(xs):
            err = rel_err(Y[i], host(x.numpy(), num))
            assert err <= 1e-12, (LENS[i], num, err)
        # float32 output is the float64 result cast; float32 input is the float64 input of the same values
        assert same_bits(t.ragged([x.to(DEV) for x in xs]), y64.to(torch.float32))
        x32 = [x.to(torch.float32) for x in xs]
        a = t.ragged([x.to(DEV) for x in x32], dtype=torch.float64)
        b = t.ragged([x.to(DEV, torch.float64) for x in x32], dtype=torch.float64)
        assert same_bits(a, b)
        for i, x in enumerate(x32):
            assert rel_err(a[i].cpu().numpy(), host(x.double().numpy(), num)) <= 1e-12, (LENS[i], num)


@pytest.mark.gpu
def test_golden_fixtures_packed():
    by_num = {}
    for tag in CASES:
        by_num.setdefault(int(GOLD[f"{tag}__num"]), []).append(tag)
    for num, tags in by_num.items():
        xs = [torch.from_numpy(GOLD[f"{tag}__x"]) for tag in tags]
        buf = torch.cat([x.to(torch.float64) for x in xs]).to(DEV)
        got = Resample(num).ragged(buf, lengths=[x.shape[0] for x in xs], dtype=torch.float64).cpu().numpy()
        for i, tag in enumerate(tags):
            ref = GOLD[f"{tag}__y"]
            tol = (1e-12 if ref.dtype == np.float64 else 1e-6) * max(np.abs(ref).max(), 1.0)
            assert np.abs(got[i] - ref).max() <= tol, tag


@pytest.mark.gpu
def test_against_the_dense_device_plan():
    xs = signals(LENS, 8)
    for num in (1000, 17750):
        t = Resample(num)
        got = t.ragged([x.to(DEV) for x in xs], dtype=torch.float64).cpu().numpy()
        for i, x in enumerate(xs):
            dense = t.batch(x.reshape(1, -1).to(DEV), torch.float64)[0].cpu().numpy()
            assert rel_err(got[i], dense) <= 1e-12, (LENS[i], num)


EDGE_LENS = [1, 2, 3, 64, 65, 2048, 2049, 4097, 4097, 5000]


@pytest.mark.gpu
@pytest.mark.parametrize("num", (1, 2, 50, 4097))
def test_classes_at_the_block_boundaries(num):
    """One-point convolutions (n = 1, and num = 1), first convolutions below, of and above the 4096-point block (M1 = 128, 256,
    4096, 8192, 16384), a repeated length on one table, and the second convolution (M2 = 1, 4, 128, 8192) below and above the
    chunk's largest M1: every row is bitwise the signal resampled alone and within 1e-12 of the host helper, and a float32 list
    gives the bits of the float64 list of the same values."""
    xs = signals(EDGE_LENS, 31)
    xd = [x.to(DEV) for x in xs]
    t = Resample(num)
    got = t.ragged(xd, dtype=torch.float64)
    assert got.shape == (len(EDGE_LENS), num)
    G = got.cpu().numpy()
    for i, x in enumerate(xs):
        assert same_bits(t.ragged([xd[i]], dtype=torch.float64)[0], got[i]), (EDGE_LENS[i], num)
        err = rel_err(G[i], host(x.numpy(), num))
        assert err <= 1e-12, (EDGE_LENS[i], num, err)
    x32 = [x.to(torch.float32) for x in xs]
    a = t.ragged([x.to(DEV) for x in x32], dtype=torch.float64)
    b = t.ragged([x.to(DEV, torch.float64) for x in x32], dtype=torch.float64)
    assert same_bits(a, b)


@pytest.mark.gpu
def test_bitwise_determinism():
    num = 20000
    t = Resample(num)
    rng = np.random.default_rng(9)
    # 150 recordings of 20 k - 60 k samples: more than one chunk of the 256 MiB work budget
    lens = [int(v) for v in rng.integers(20000, 60001, size=150)]
    lens[10] = lens[11] = lens[120]                  # repeated lengths
    xs = signals(lens, 10, np.float32)
    xd = [x.to(DEV) for x in xs]
    full = t.ragged(xd)
    assert torch.isfinite(full).all()
    # a permuted list gives permuted rows
    perm = rng.permutation(len(xs))
    assert same_bits(t.ragged([xd[i] for i in perm]), full[torch.from_numpy(perm).to(DEV)])
    # each signal alone equals the same signal inside the list
    for i in (0, 10, 11, 77, 120, 149):
        assert same_bits(t.ragged([xd[i]])[0], full[i]), i
    # a packed buffer equals the list; host in / out equals device in / out; out= is honoured
    assert same_bits(t.ragged(torch.cat(xd), lengths=lens), full)
    assert same_bits(t.ragged(xs), full.cpu())
    assert same_bits(t.ragged(torch.cat(xs), lengths=torch.tensor(lens)), full.cpu())
    out = torch.full((len(xs), num), 7.0, device=DEV)
    assert t.ragged(xd, out=out) is out and same_bits(out, full)
    out64 = torch.empty((len(xs), num), dtype=torch.float64)
    assert t.ragged(xs, dtype=torch.float64, out=out64) is out64 and same_bits(out64.to(torch.float32), full.cpu())
    # the same call again
    assert same_bits(t.ragged(xd), full)
    assert len([k for k in t._plans if k[0] == "ragged"]) == 1


@pytest.mark.gpu
def test_return_to_an_earlier_list():
    """Lists A, A, B, A on one plan: B has A's count and total but other lengths, so the descriptors keep their size.  Every
    row equals the signal resampled alone."""
    t = Resample(50)
    a = [x.to(DEV) for x in signals([3, 64, 65], 12)]
    b = [a[2], a[0], a[1]]
    alone = {id(x): t.ragged([x], dtype=torch.float64)[0] for x in a}
    for step, xs in enumerate((a, a, b, a)):
        got = t.ragged(xs, dtype=torch.float64)
        assert got.shape == (3, 50)
        for i, x in enumerate(xs):
            assert same_bits(got[i], alone[id(x)]), (step, i, x.shape[0])
    assert len([k for k in t._plans if k[0] == "ragged"]) == 1


@pytest.mark.gpu
def test_labels_follow_the_rule():
    lens = [2000, 35500, 4097, 60001, 129, 35500, 2500]
    ys = label_tracks(lens, 21)
    ys[-1] = torch.from_numpy(GOLD["labels__y"])
    ties = 0
    for num in (1000, 20000, 1001):
        t = Resample(num)
        got = resample_labels_ragged([y.to(DEV) for y in ys], t)
        assert got.dtype == torch.int64 and got.shape == (len(ys), num) and got.is_cuda
        assert torch.equal(resample_labels_ragged(ys, t), got.cpu())
        for i, y in enumerate(ys):
            ref = resample_labels(y, t).numpy()
            ok = off_tie(t(y).numpy())
            ties += int((~ok).sum())
            assert np.array_equal(got[i].cpu().numpy()[ok], ref[ok]), (lens[i], num)
    print(f"ragged label rule: {ties} samples within 1e-9 of a .5 tie")


@pytest.mark.gpu
def test_nan_stays_in_its_row():
    xs = signals([2000, 35500, 35500, 129, 60001], 12)
    xs[1] = xs[1].clone()
    xs[1][1234] = float("nan")
    got = Resample(17750).ragged([x.to(DEV) for x in xs], dtype=torch.float64).cpu()
    assert torch.isnan(got[1]).all()
    for i in (0, 2, 3, 4):
        assert not torch.isnan(got[i]).any(), i


@pytest.mark.gpu
def test_empty_list_on_device():
    t = Resample(500)
    e = t.ragged(torch.empty(0, device=DEV), lengths=[])
    assert e.shape == (0, 500) and e.is_cuda
    assert t.ragged([], labels=True).shape == (0, 500)


def corpus(lens, seed):
    xs = [torch.from_numpy(synth.recording(T, seed=seed + i)) for i, T in enumerate(lens)]
    return list(zip(xs, label_tracks(lens, seed)))


@pytest.mark.gpu
def test_build_resampled_recordings(oracle_mod):
    from tests import parity
    num = 2000
    tf = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    rs = Resample(num)
    lens = [20000, 35500, 4100, 60001, 1200, 35500, 27777, 50000]
    recs = corpus(lens, 300)
    xs = [x for x, _ in recs]
    devk = build_resampled_recordings(recs, tf, rs, device=DEV, keep_on_device=True)
    assert len(devk) == len(recs) and devk.features.shape == (len(recs), num, 44) and devk.features.is_cuda
    # bitwise: one ragged resample call and one batch transform
    assert same_bits(devk.features, tf.batch(rs.ragged([x.to(DEV) for x in xs])))
    # host-returned, in several small groups, equals device-kept in one group
    host = build_resampled_recordings(recs, tf, rs, device=DEV, max_samples=80000)
    assert not host.features.is_cuda and same_bits(host.features, devk.features.cpu())
    assert torch.equal(host.labels, devk.labels)
    b = CorpusBuilder(tf, device=DEV, resample=rs)
    again = b.build_resampled_recordings(recs, keep_on_device=True, max_samples=60001)
    assert same_bits(again.features, devk.features)
    # the lazy dataset's items: tf(Resample(num)(x)) with the host helper, through the parity gate
    for i, x in enumerate(xs):
        xr = Resample(num)(x)                        # float32, as the dataset's transform chain hands it on
        ref = tf(xr)
        _, hd = oracle_mod.features(xr.numpy()[None], 1000, W128, (25, 200), "stack", nthreads=min(16, os.cpu_count() or 1),
                                    return_halfdist=True)
        parity.check(devk[i][0].cpu().numpy(), ref.numpy(), hd[0], 0, what=f"resampled recording {i}")
    # labels: round(Resample(num)(y)) - 1 of the track as given
    ties = 0
    assert devk.labels.shape == (len(recs), num) and devk.labels.dtype == torch.int64 and not devk.labels.is_cuda
    for i, (_, y) in enumerate(recs):
        ref = resample_labels(y, Resample(num)).numpy()
        ok = off_tie(Resample(num)(y).numpy())
        ties += int((~ok).sum())
        assert np.array_equal(devk.labels[i].numpy()[ok], ref[ok]), i
    print(f"builder labels: {ties} samples within 1e-9 of a .5 tie")
    # unlabelled corpus, empty corpus
    unl = build_resampled_recordings([(x, None) for x in xs[:3]], tf, rs, device=DEV)
    assert unl.labels is None and unl[1][1] is None and same_bits(unl.features, devk.features[:3].cpu())
    assert len(build_resampled_recordings([], tf, rs, device=DEV)) == 0
    tf.check()


@pytest.mark.gpu
def test_build_resampled_recordings_half_features():
    num = 2000
    tf32 = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    tf16 = FSST(1000, W128, truncate_freq=(25, 200), stack=True, out_dtype=torch.float16)
    rs = Resample(num)
    recs = corpus([20000, 4100, 35500, 60001], 400)
    items = build_resampled_recordings(recs, tf16, rs, device=DEV, keep_on_device=True)
    assert items.features.dtype == torch.float16 and items.features.shape == (4, num, 44)
    assert same_bits(items.features, tf16.batch(rs.ragged([x.to(DEV) for x, _ in recs])))
    f32 = build_resampled_recordings(recs, tf32, rs, device=DEV, keep_on_device=True)
    assert same_bits(items.features, f32.features.to(torch.float16))
    host = build_resampled_recordings(recs, tf16, rs, device=DEV, max_samples=40000)
    assert same_bits(host.features, items.features.cpu())


@pytest.mark.gpu
def test_one_builder_serves_every_build_in_turn():
    """One CorpusBuilder through framed builds and whole-recording builds in turn, host-returned and device-kept: its staging
    buffers and its device ring are re-used, re-viewed and regrown between calls, and every call has three or more groups, so
    that the waits on a staging buffer's and a ring half's previous use are live.  Every arena equals the direct transform calls."""
    from heart_sounds_segmentation_amd.framing import frame_batch
    num = 500
    tf = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    rs = Resample(num)
    lens = [5200, 2500, 1999, 4100, 7300, 3000]
    recs = corpus(lens, 500)
    xs = [x for x, _ in recs]
    kept = [(x, y) for x, y in recs if x.shape[0] >= 2000]          # the framed build skips the 1999-sample recording
    assert sum(max((T - 2000) // 1000, 1) >= 2 for T in lens if T >= 2000) >= 3     # >= 3 groups at windows_per_launch=2

    frames = [frame_batch(x.to(DEV), 1000, 2000) for x, _ in kept]
    want_framed = torch.cat([tf.batch(F) for F in frames])
    want_framed_rs = torch.cat([tf.batch(rs.batch(F)) for F in frames])
    want_whole = [tf(x).cpu() for x in xs]
    want_whole_rs = tf.batch(rs.ragged([x.to(DEV) for x in xs]))
    plain_labels = torch.cat([frame_batch(y - 1, 1000, 2000) for _, y in kept])
    ties = 0

    def labels_follow_the_rule(got, tracks):
        """``got[i]`` against the host rule round(Resample(num)(track i)) - 1, off the .5 ties."""
        nonlocal ties
        assert got.shape == (len(tracks), num) and got.dtype == torch.int64 and not got.is_cuda
        for i, y in enumerate(tracks):
            ref = resample_labels(y, Resample(num)).numpy()
            ok = off_tie(Resample(num)(y).numpy())
            ties += int((~ok).sum())
            assert np.array_equal(got[i].numpy()[ok], ref[ok]), i

    framed_tracks = [fr for _, y in kept for fr in frame_batch(y - 1, 1000, 2000)]
    whole_tracks = [y for _, y in recs]

    b = CorpusBuilder(tf, device=DEV, windows_per_launch=2, resample=rs)
    for keep in (False, True):
        it = b.build(recs, keep_on_device=keep)
        assert it.features.is_cuda == keep and torch.equal(it.features.to(DEV), want_framed_rs)
        labels_follow_the_rule(it.labels, framed_tracks)
        it = b.build_resampled_recordings(recs, keep_on_device=keep, max_samples=6000)
        assert it.features.is_cuda == keep and torch.equal(it.features.to(DEV), want_whole_rs)
        labels_follow_the_rule(it.labels, whole_tracks)

    b = CorpusBuilder(tf, device=DEV, windows_per_launch=2)
    it = b.build(recs)
    assert not it.features.is_cuda and torch.equal(it.features, want_framed.cpu()) and torch.equal(it.labels, plain_labels)
    def whole_recordings(keep):
        whole = b.build_recordings(recs, keep_on_device=keep, max_samples=6000)
        assert len(whole) == len(recs)
        for i, (f, y) in enumerate(whole):
            assert f.is_cuda == keep and torch.equal(f.cpu(), want_whole[i]), (keep, i)
            assert y is recs[i][1]

    whole_recordings(False)
    it = b.build(recs + recs)                            # the list twice: larger groups, a larger arena (regrow)
    assert torch.equal(it.features, torch.cat([want_framed, want_framed]).cpu())
    assert torch.equal(it.labels, torch.cat([plain_labels, plain_labels]))
    whole_recordings(True)
    tf.check()
    print(f"one builder, every build: {ties} label samples within 1e-9 of a .5 tie")
