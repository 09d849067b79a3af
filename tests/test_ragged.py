"""Signals of different lengths in one call: hssfsst_exec_ragged (C ABI), FSST.ragged / RaggedFeatures (Python) and
corpus.build_recordings (the reference's lazy dataset over a whole corpus, hss/datasets/heart_sounds.py:175-184).

CPU tests check the ABI's argument handling without a device and the Python surface's argument errors before any plan is
made; GPU tests (one process) check that every signal's features are bit-identical to the same signal transformed alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, synth
from heart_sounds_segmentation_amd.corpus import CorpusBuilder, build_recordings
from heart_sounds_segmentation_amd.transforms import FSST, RaggedFeatures, Resample

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hssfsst.h")
W128 = synth.kaiser_window(128, 0.5)
MIXED = [1, 2, 63, 64, 65, 127, 128, 129, 300, 2000, 2001, 2048, 2049, 35500, 120000]


def ragged_call(L, plan, x, x_len, starts, lens, out=None, x_on_device=0, out_on_device=0):
    st = np.ascontiguousarray(starts, dtype=np.int64)
    ln = np.ascontiguousarray(lens, dtype=np.int64)
    return L.hssfsst_exec_ragged(plan, x, x_len, st.ctypes.data if st.size else None, ln.ctypes.data if ln.size else None,
                                 int(ln.size), x_on_device, out, out_on_device, None)


def same_bits(a, b):
    """Bit-identical (NaN included: a z-score over a constant block is NaN, as in a single call)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def last_error(L):
    return L.hssfsst_last_error().decode()


# ---------------------------------------------------------------------------------------------------- CPU
def test_header_declares_ragged_entry_and_version(built_lib):
    with open(HEADER) as fh:
        text = fh.read()
    assert int(re.search(r"#define HSSFSST_VERSION (\d+)", text).group(1)) == 210
    assert built_lib.hssfsst_version() == 210
    assert "int hssfsst_exec_ragged(" in text
    assert built_lib.hssfsst_exec_ragged.restype is ctypes.c_int
    assert len(built_lib.hssfsst_exec_ragged.argtypes) == 10


def test_argument_errors_are_einval_without_a_device(built_lib):
    """Every argument error is HSSFSST_EINVAL and is found before the plan (here NULL) or a device is looked at: the message
    names the argument, not the plan."""
    L = built_lib
    x = (ctypes.c_float * 100)()
    out = (ctypes.c_float * 8800)()
    cases = [
        (dict(x=x, x_len=100, starts=[0], lens=[10], out=out, batch=-1), "batch"),
        (dict(x=None, x_len=100, starts=[0], lens=[10], out=out), "NULL x"),
        (dict(x=x, x_len=100, starts=None, lens=[10], out=out), "NULL starts"),
        (dict(x=x, x_len=100, starts=[0], lens=None, out=out), "NULL lens"),
        (dict(x=x, x_len=100, starts=[0], lens=[10], out=None), "NULL out"),
        (dict(x=x, x_len=100, starts=[0, 5], lens=[10, 0], out=out), "length 0"),
        (dict(x=x, x_len=100, starts=[0], lens=[-3], out=out), "length -3"),
        (dict(x=x, x_len=100, starts=[95], lens=[10], out=out), "outside"),
        (dict(x=x, x_len=100, starts=[-1], lens=[10], out=out), "outside"),
        (dict(x=x, x_len=100, starts=[0], lens=[101], out=out), "outside"),
    ]
    for kw, msg in cases:
        st = np.asarray(kw["starts"] if kw["starts"] is not None else [0], dtype=np.int64)
        ln = np.asarray(kw["lens"] if kw["lens"] is not None else [1], dtype=np.int64)
        batch = kw.get("batch", ln.size)
        rc = L.hssfsst_exec_ragged(None, kw["x"], kw["x_len"], st.ctypes.data if kw["starts"] is not None else None,
                                   ln.ctypes.data if kw["lens"] is not None else None, batch, 0, kw["out"], 0, None)
        assert rc == _lib.E_INVAL, (kw, rc)
        assert msg in last_error(L), (msg, last_error(L))
    # well-formed arguments: the NULL plan is what is refused, still without a device
    assert ragged_call(L, None, x, 100, [0, 40], [50, 60], out) == _lib.E_INVAL
    assert "plan" in last_error(L)


def test_python_argument_errors_before_any_plan():
    tf = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    with pytest.raises(ValueError, match="different devices"):
        tf.ragged([torch.zeros(100), torch.zeros(50, device="meta")])
    with pytest.raises(ValueError, match="expected"):
        tf.ragged([torch.zeros(100), torch.zeros(2, 50)])
    with pytest.raises(ValueError, match="sum to"):
        tf.ragged(torch.zeros(100), lengths=[40, 50])
    with pytest.raises(ValueError, match=">= 1"):
        tf.ragged(torch.zeros(100), lengths=[100, 0])
    with pytest.raises(ValueError, match="needs lengths"):
        tf.ragged(torch.zeros(100))
    with pytest.raises(ValueError, match="empty"):
        tf.ragged([torch.zeros(10), torch.zeros(0)])
    assert tf._plans == {}                            # nothing was created


def test_empty_list_returns_empty_ragged_features():
    for kw, C, dt in [(dict(stack=True), 44, torch.float32), (dict(abs=True), 22, torch.float32), ({}, None, torch.complex64)]:
        tf = FSST(1000, W128, truncate_freq=(25, 200), **kw)
        rf = tf.ragged([])
        assert isinstance(rf, RaggedFeatures) and len(rf) == 0 and list(rf) == []
        assert rf.offsets.tolist() == [0] and rf.data.dtype == dt and rf.data.numel() == 0
        if C is not None:
            assert tuple(rf.data.shape) == (0, C) and tuple(rf.padded().shape) == (0, 0, C)
        assert tf._plans == {}


def test_build_recordings_refuses_resample_and_raw():
    tf = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    with pytest.raises(ValueError, match="resample"):
        build_recordings([(torch.zeros(100), None)], tf, resample=Resample(50))
    with pytest.raises(ValueError, match="resample"):
        CorpusBuilder(tf, device="cpu", resample=Resample(50)).build_recordings([(torch.zeros(100), None)])
    with pytest.raises(ValueError, match="stack=True or abs=True"):
        CorpusBuilder(FSST(1000, W128), device="cpu").build_recordings([(torch.zeros(100), None)])


# ---------------------------------------------------------------------------------------------------- GPU
def signals(lengths, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, T in enumerate(lengths):
        x = synth.pcg_windows(1, n=int(T), seed=seed + i)[0] if T >= 16 else rng.standard_normal(int(T)).astype(np.float32)
        out.append(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))
    return out


def assert_alone(tf, xs, rf, what):
    assert len(rf) == len(xs)
    for i, x in enumerate(xs):
        one = tf.batch(x.reshape(1, -1))[0]
        got = rf[i]
        assert got.shape == one.shape and got.dtype == one.dtype and got.device == one.device, (what, i, got.shape, one.shape)
        assert same_bits(got, one), f"{what}: signal {i} (T={x.shape[0]})"


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(stack=True), dict(abs=True), {}], ids=["stack", "abs", "raw"])
@pytest.mark.parametrize("band", [(25, 200), (25, 180), (25, 190)])
def test_mixed_lengths_bit_identical_nwin128(kw, band):
    tf = FSST(1000, W128, truncate_freq=band, **kw)
    if band == (25, 190):                             # an odd band: 2K % 4 != 0, signals of the arena start off a 16-byte boundary
        assert tf.band()[1] % 2 == 1
    xs = [x.cuda() for x in signals(MIXED, 11)]
    rf = tf.ragged(xs)
    assert "ragged" in tf.last_kernel()               # one launch for the list, the ragged instantiation
    assert rf.data.is_cuda and rf.offsets.tolist() == np.concatenate([[0], np.cumsum(MIXED)]).tolist()
    assert_alone(tf, xs, rf, f"{kw} {band}")
    if kw:
        ref = torch.nn.utils.rnn.pad_sequence(list(rf), batch_first=True)
        assert same_bits(rf.padded(), ref)
        assert same_bits(rf.padded(-1.0), torch.nn.utils.rnn.pad_sequence(list(rf), batch_first=True, padding_value=-1.0))
    tf.check()


@pytest.mark.gpu
@pytest.mark.parametrize("nwin", [256, 512, 64, 100])
@pytest.mark.parametrize("kw", [dict(stack=True), dict(abs=True)], ids=["stack", "abs"])
def test_mixed_lengths_other_windows(nwin, kw):
    lengths = [1, 63, 129, 300, 2001, 2049, 35500] if nwin in (256, 512) else [1, 65, 300, 2001, 9000]
    tf = FSST(1000, synth.kaiser_window(nwin, 0.5), truncate_freq=(25, 200), **kw)
    xs = [x.cuda() for x in signals(lengths, 21)]
    assert_alone(tf, xs, tf.ragged(xs), f"nwin {nwin}")
    tf.check()


@pytest.mark.gpu
def test_neighbours_do_not_leak():
    """Recordings that touch and overlap in one buffer, with amplitudes 1e9 apart: each result equals its signal alone."""
    tf = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    tfa = FSST(1000, W128, truncate_freq=(25, 200), abs=True)
    rng = np.random.default_rng(5)
    buf = rng.standard_normal(20000).astype(np.float32)
    buf[:7000] *= 1e9                                 # the first recording 1e9 louder than its neighbours
    starts = [0, 7000, 6500, 12990, 13000, 100, 19999]
    lens = [7000, 6000, 1000, 20, 7000, 6900, 1]
    X = torch.from_numpy(buf).cuda()
    for t in (tf, tfa):
        out = torch.empty((sum(lens), t._plan(0).ofps), device="cuda")
        rc = ragged_call(_lib.lib(), t._plan(0).handle, ctypes.c_void_p(X.data_ptr()), X.numel(), starts, lens,
                         ctypes.c_void_p(out.data_ptr()), 1, 1)
        _lib.check(rc, "hssfsst_exec_ragged")
        torch.cuda.synchronize()
        assert ragged_call(_lib.lib(), t._plan(0).handle, None, 0, [], [], None, 1, 1) == 0      # batch 0: nothing to do
        big = np.int64(2 ** 31 // (2 * t._plan(0).nf) + 1)
        assert ragged_call(_lib.lib(), t._plan(0).handle, ctypes.c_void_p(X.data_ptr()), int(big), [0], [big],
                           ctypes.c_void_p(out.data_ptr()), 1, 1) == _lib.E_INVAL                # over the per-signal limit
        assert "too long" in last_error(_lib.lib())
        off = 0
        for s, n in zip(starts, lens):
            one = t.batch(X[s:s + n].reshape(1, -1))[0]
            assert same_bits(out[off:off + n], one), (s, n)
            off += n


@pytest.mark.gpu
def test_permutation_host_device_dtype_and_zeros():
    tf = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    lens = [500, 2000, 17, 35500, 4000, 2049, 128]
    xs = signals(lens, 31)
    xs[4] = torch.zeros(4000)                         # all-zero recording: NaN, as a single call
    dev = tf.ragged([x.cuda() for x in xs])
    host = tf.ragged(xs)
    assert not host.data.is_cuda and dev.data.is_cuda
    assert same_bits(host.data, dev.data.cpu())
    assert torch.isnan(dev[4]).all() and torch.isnan(tf(xs[4])).all()
    perm = [3, 0, 6, 2, 5, 1, 4]
    pr = tf.ragged([xs[i].cuda() for i in perm])
    for j, i in enumerate(perm):
        assert same_bits(pr[j], dev[i]), (j, i)
    # float64 input == its float32 rounding; (T, 1) input == (T,)
    x64 = [torch.from_numpy(synth.pcg_windows(1, n=T, seed=40 + T)[0].astype(np.float64) * (1 + 1e-9)) for T in (3000, 700)]
    r64 = tf.ragged(x64)
    r32 = tf.ragged([x.to(torch.float32).reshape(-1, 1) for x in x64])
    assert same_bits(r64.data, r32.data)
    # a packed buffer with lengths == the list
    packed = tf.ragged(torch.cat([x.cuda() for x in xs]), lengths=lens)
    assert same_bits(packed.data, dev.data)
    # host items are what the dataset's call returns
    for i in (0, 2, 3):
        assert same_bits(host[i], tf(xs[i]))
    tf.check()


@pytest.mark.gpu
def test_return_to_an_earlier_list():
    """Lists A, A, B, A on one plan: B has A's count and total (the tables keep their size) but other lengths; every call
    equals each signal alone."""
    tf = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    a = [x.cuda() for x in signals([1, 17, 300], 61)]
    b = [a[2], a[0], a[1]]
    alone = {id(x): tf.batch(x.reshape(1, -1))[0] for x in a}
    for step, xs in enumerate((a, a, b, a)):
        rf = tf.ragged(xs)
        assert "ragged" in tf.last_kernel() and len(rf) == 3
        for i, x in enumerate(xs):
            assert same_bits(rf[i], alone[id(x)]), (step, i, x.shape[0])
    tf.check()


@pytest.mark.gpu
def test_against_oracle(oracle_mod):
    from tests import parity
    tf = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    xs = signals([1500, 2300, 4100], 51)
    rf = tf.ragged([x.cuda() for x in xs])
    for i, x in enumerate(xs):
        ref, hd = oracle_mod.features(x.numpy()[None], 1000, W128, (25, 200), "stack", nthreads=min(16, os.cpu_count() or 1),
                                      return_halfdist=True)
        parity.check(rf[i].cpu().numpy(), ref[0], hd[0], 0, what=f"ragged[{i}]")


@pytest.mark.gpu
def test_output_beyond_2g_floats():
    """ABS, 100 recordings of 1 M samples: 2.2 G floats of output, offsets above 2^31; the last recording equals its single exec."""
    tf = FSST(1000, W128, truncate_freq=(25, 200), abs=True)
    n, B = 1_000_000, 100
    free, _ = torch.cuda.mem_get_info()
    need = B * n * 22 * 4 + B * n * 4 + (n * 22 * 4) * 2
    if free < 2 * need:
        pytest.skip(f"needs {2 * need / 1e9:.0f} GB of device memory, {free / 1e9:.0f} GB free")
    g = torch.Generator(device="cuda").manual_seed(77)
    X = torch.randn(B * n, generator=g, device="cuda")
    base = X[:n]
    rf = tf.ragged(X, lengths=[n] * B)
    assert rf.data.numel() > 2 ** 31
    last = tf.batch(X[(B - 1) * n:].reshape(1, -1))[0]
    assert same_bits(rf[B - 1], last)
    assert same_bits(rf[0], tf.batch(base.reshape(1, -1))[0])
    tf.check()


@pytest.mark.gpu
def test_build_recordings_equals_the_lazy_dataset():
    tf = FSST(1000, W128, truncate_freq=(25, 200), stack=True)
    rng = np.random.default_rng(61)
    lens = [int(v) for v in rng.integers(500, 90000, size=20)]
    lens[3] = 1200                                    # shorter than a frame: build() would drop it
    recs = []
    for i, T in enumerate(lens):
        x = torch.from_numpy(synth.recording(T, seed=100 + i))
        y = torch.from_numpy(rng.integers(1, 5, size=T).astype(np.int64))
        recs.append((x, y))
    want = [(tf(x), y) for x, y in recs]
    # small groups: several ragged calls, double-buffered
    host = build_recordings(recs, tf, max_samples=200_000)
    devk = build_recordings(recs, tf, keep_on_device=True)
    assert len(host) == len(devk) == len(recs)
    for i, ((f, y), (fd, yd), (wf, wy)) in enumerate(zip(host, devk, want)):
        assert not f.is_cuda and fd.is_cuda
        assert f.shape == wf.shape == (lens[i], 44) and same_bits(f, wf), i
        assert same_bits(fd.cpu(), wf), i
        assert y is recs[i][1] and yd is recs[i][1]
    unl = build_recordings([(x, None) for x, _ in recs[:3]], tf)
    assert [y for _, y in unl] == [None] * 3 and same_bits(unl[2][0], want[2][0])
    tf.check()
