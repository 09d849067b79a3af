"""Scoring a segmentation on the device (include/hssfsst.h: hssfsst_score_states; sequence.segmentation_scores): every integer of the
call equals tests/score_cases.py's numpy restatement of the contract, which is itself held to brute force over all pairs and to
scikit-learn.  No device: the restatement, the bad calls of the entry, score_info, csrc/score_layout.hpp in a program of its own
under sanitizers, and the check that every function of the header that takes a ``const hssfsst_launch*`` has a side-stream case
here.  On the GPU: the lengths, list sizes, score and label patterns and prediction inputs of the issue, the neighbours, the
derived figures, decode_states scored end to end, the two side-stream scenarios, and the kernels' resources."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from heart_sounds_segmentation_amd import _lib, consumer
from heart_sounds_segmentation_amd.sequence import (RaggedStates, SegmentationScores, decode_states, score_info, segmentation_scores)
from heart_sounds_segmentation_amd.transforms.synchrosqueeze import RaggedFeatures
from tests import score_cases as sc
from tests import side_stream as ss
from tests.side_stream import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "heart_sounds_segmentation_amd", "csrc")
PATTERNS = ["eighths", "log_softmax", "constant", "ascending", "descending", "byte0", "byte1", "byte2", "byte3", "specials"]


# ------------------------------------------------------------------------------------------------ the restatement (no device)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_restatement_equals_brute_force(pattern):
    """All pairs compared as floats at T <= 40: one recording and three, pooled and per recording, labels with ignored steps and
    an absent class, argmax predictions and given states."""
    for seed, lens in enumerate(([1], [2], [40], [7, 13, 20])):
        n = sum(lens)
        logp = sc.scores(pattern, n, seed)
        for lab_pattern in ("plain", "mixed"):
            labels = sc.labels_for(lab_pattern, lens, seed)
            states = np.random.default_rng(seed).integers(0, 4, size=n).astype(np.uint8) if seed % 2 else None
            for per in (False, True):
                a = sc.restate(logp, states, labels, sc.offsets(lens), per)
                b = sc.brute_force(logp, states, labels, sc.offsets(lens), per)
                for k in ("confusion", "ignored", "rank"):
                    assert np.array_equal(a[k], b[k]), (pattern, lens, lab_pattern, per, k)
                assert a["confusion"].sum() + a["ignored"].sum() == n


def test_key_is_monotone():
    bits = np.concatenate([np.array([0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000,
                                     0x7fc00000, 0xffc00000], dtype=np.uint32),
                           np.random.default_rng(5).integers(0, 1 << 32, size=4000, dtype=np.uint64).astype(np.uint32)])
    x = bits.view(np.float32)
    with np.errstate(invalid="ignore"):                  # (signalling NaNs among the patterns)
        v = np.where(np.isnan(x), -np.inf, x.astype(np.float64))
    k = sc.key32(x).astype(np.int64)
    i, j = np.meshgrid(np.arange(200), np.arange(x.size), indexing="ij")
    assert np.array_equal(v[i] < v[j], k[i] < k[j]) and np.array_equal(v[i] == v[j], k[i] == k[j])
    assert (k != 0).all()


def test_restatement_equals_sklearn():
    """roc_auc_score (one class against the rest), confusion_matrix and precision_recall_fscore_support on the counted steps."""
    metrics = pytest.importorskip("sklearn.metrics")
    for seed, (n, pattern) in enumerate(((70, "eighths"), (3000, "eighths"), (3000, "log_softmax"), (70000, "eighths"))):
        logp = sc.scores(pattern, n, seed)
        labels = sc.labels_for("plain", [n], seed)
        labels[::11] = sc.IGNORE
        r = sc.restate(logp, None, labels, [0, n], False)
        d = sc.derived(r)
        use = labels <= 3
        pred = sc.predicted(logp, None)[use]
        assert np.array_equal(r["confusion"][0], metrics.confusion_matrix(labels[use], pred, labels=[0, 1, 2, 3]))
        p, rc, f, s = metrics.precision_recall_fscore_support(labels[use], pred, labels=[0, 1, 2, 3], zero_division=0)
        for got, want in ((d["precision"][0], p), (d["recall"][0], rc), (d["f1"][0], f)):
            assert np.abs(got - want).max() <= 4e-16
        assert np.array_equal(d["support"][0], s)
        for c in range(4):
            want = metrics.roc_auc_score(labels[use] == c, logp[use, c].astype(np.float64))
            assert abs(d["auroc"][0, c] - want) <= 1e-15, (n, pattern, c, d["auroc"][0, c], want)


# ------------------------------------------------------------------------------------------------ the entry's arguments (no device)
def _entry(lib, logp=64, states=0, labels=64, offs=(0, 5), count=None, per=0, confusion=64, ignored=64, rank=0, work=0, work_bytes=0,
           where=(0, None)):
    """One call with made-up device addresses: every argument error is found before the device is touched."""
    o = (ctypes.c_int64 * len(offs))(*offs) if offs is not None else None
    w = ctypes.byref(_lib.Launch(*where)) if where is not None else None
    rc = lib.hssfsst_score_states(logp or None, states or None, labels or None, o, len(offs) - 1 if count is None else count, per,
                                  confusion or None, ignored or None, rank or None, work or None, work_bytes, w)
    return rc, lib.hssfsst_last_error().decode() if rc else ""


def test_bad_calls_are_refused_before_any_device_work(built_lib):
    per, _, const = score_info()[:3]
    E, U = _lib.E_INVAL, _lib.E_UNSUPPORTED
    cases = [
        (dict(where=None), E, "score_states: bad argument (where is NULL)"),
        (dict(labels=0), E, "score_states: bad argument (labels is NULL)"),
        (dict(confusion=0), E, "score_states: bad argument (confusion is NULL)"),
        (dict(ignored=0), E, "score_states: bad argument (ignored is NULL)"),
        (dict(offs=None, count=1), E, "score_states: bad argument (offsets is NULL)"),
        (dict(count=-1), E, "score_states: count -1 is negative"),
        (dict(logp=0, states=0), E, "score_states: bad argument (states and logp are both NULL)"),
        (dict(logp=0, states=64, rank=64, work=64, work_bytes=1 << 20), E, "score_states: bad argument (logp is NULL while rank is not)"),
        (dict(rank=64), E, "score_states: bad argument (work is NULL while rank is not)"),
        (dict(where=(-1, None)), E, "score_states: device -1 is negative"),
        (dict(logp=68), E, "score_states: logp is not 16-byte aligned"),
        (dict(rank=68, work=64, work_bytes=1 << 20), E, "score_states: rank is not 8-byte aligned"),
        (dict(rank=64, work=72, work_bytes=1 << 20), E, "score_states: work is not 16-byte aligned"),
        (dict(confusion=68), E, "score_states: confusion is not 8-byte aligned"),
        (dict(rank=64, work=64, work_bytes=per * 5 + const - 1), E,
         f"score_states: work of {per * 5 + const - 1} bytes is too small: 5 steps in 1 recordings need {per * 5 + const}"),
        (dict(offs=(1, 5)), E, "score_states: offsets[0] is 1, not 0"),
        (dict(offs=(0, 5, 5)), E, "score_states: offsets do not increase at index 2 (offsets[1] = 5, offsets[2] = 5)"),
        (dict(offs=(0, 1 << 30, 1 << 31)), U, "score_states: 2147483648 steps in all, over the limit of 2^31 - 1"),
        (dict(offs=(0, 1 << 31)), U, "score_states: recording 0 has 2147483648 steps, over the limit of 2147483647"),
    ]
    for kw, code, text in cases:
        assert _entry(built_lib, **kw) == (code, text), kw
    assert _entry(built_lib, offs=(0,)) == (0, "")       # an empty list does nothing, and needs no device
    assert _entry(built_lib, offs=(0,), rank=64, work=64, work_bytes=const) == (0, "")


def test_score_info(built_lib):
    per, rec, const, block, bits, passes = score_info()
    assert (per, rec, const, block, bits, passes) == (17, 0, 4096, 2048, 8, 8) and per <= 24
    assert consumer.score_info() == score_info() and consumer.segmentation_scores is segmentation_scores
    assert built_lib.hssfsst_score_info(None, None, None, None, None, None) == 0


def test_python_arguments_are_checked_on_the_host():
    with pytest.raises(ValueError, match="uint8 states or float32 log-probs"):
        segmentation_scores(torch.zeros(5, 4, dtype=torch.float64), torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="on a GPU expected"):
        segmentation_scores(torch.zeros(5, dtype=torch.uint8), torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="on a GPU expected"):
        segmentation_scores(torch.zeros(5, 4), torch.zeros(5, dtype=torch.uint8))
    s = SegmentationScores(torch.tensor([[5, 1, 0, 0], [0, 3, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0]]), torch.tensor(2), None)
    assert float(s.accuracy) == 8 / 11 and s.recall.tolist() == [5 / 6, 1.0, 0.0, 0.0] and s.precision.tolist() == [5 / 7, 0.75, 0.0, 0.0]
    assert s.support.tolist() == [6, 3, 2, 0] and float(s.macro_recall) == (5 / 6 + 1.0) / 4
    with pytest.raises(ValueError, match="no rank"):
        s.auroc


def test_score_layout_under_sanitizers(tmp_path):
    """csrc/score_layout.hpp in a program of its own built with -fsanitize=address,undefined: the key transform over a sweep of bit
    patterns, the pass count and the partition at their borders, the sequential reference against brute force."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "score_layout_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                        os.path.join(ROOT, "tests", "native", "score_layout_check.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "score layout check ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ------------------------------------------------------------------------------------------------ the device against the restatement
def _run(logp, states, labels, lens, per, auroc=True, form="ragged"):
    """One call on the device from host arrays -> the restatement's dictionary, from the tensors of the result."""
    offs = torch.tensor(sc.offsets(lens), dtype=torch.int64)
    lab = torch.from_numpy(np.ascontiguousarray(labels)).cuda()
    lp = None if logp is None else torch.from_numpy(np.ascontiguousarray(logp)).cuda()
    st = None if states is None else torch.from_numpy(np.ascontiguousarray(states)).cuda()
    if form == "ragged":
        lp = None if lp is None else RaggedFeatures(lp, offs, 4, False)
        st = None if st is None else RaggedStates(st, offs)
    res = segmentation_scores(st if st is not None else lp, lab, per_recording=per, auroc=auroc, scores=lp if st is not None else None)
    return res


def _equal(res, want, per):
    got = {"confusion": res.confusion, "ignored": res.ignored, "rank": res.rank}
    for k, w in want.items():
        if w is None:
            assert got[k] is None, k
            continue
        w = torch.from_numpy(np.asarray(w if per else w[0]))
        assert got[k].dtype == torch.int64 and got[k].is_cuda and torch.equal(got[k].cpu(), w), (k, got[k].cpu().tolist()[:3], w.tolist()[:3])


def _check(logp, states, labels, lens, per, want_rank=True):
    res = _run(logp, states, labels, lens, per, auroc=want_rank)
    _equal(res, sc.restate(logp, states, labels, sc.offsets(lens), per, want_rank and logp is not None), per)
    return res


def _block():
    return score_info()[3]


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["eighths", "constant", "specials"])
def test_lengths(pattern):
    """One recording of every length at which a wave, a block of the sort or a tile of the rank fills, overflows by one or is one
    short; pooled and per recording are the same numbers."""
    B = _block()
    for T in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, B - 1, B, B + 1, 2 * B + 3, 4 * B - 1, 4 * B, 4 * B + 1, 8 * B + 5):
        logp = sc.scores(pattern, T, T)
        labels = sc.labels_for("mixed" if T % 2 else "plain", [T], T)
        for per in (False, True):
            res = _check(logp, None, labels, [T], per)
            if pattern == "constant":
                rk = res.rank.reshape(4, 3).cpu()
                assert torch.equal(rk[:, 0], rk[:, 1] * rk[:, 2])


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2, 17, 300])
@pytest.mark.parametrize("per", [False, True], ids=["pooled", "per recording"])
def test_lists(count, per):
    lens = sc.list_lens(count)
    n = sum(lens)
    for pattern in ("eighths", "log_softmax"):
        _check(sc.scores(pattern, n, count), None, sc.labels_for("mixed", lens, count), lens, per)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
def test_score_patterns(pattern):
    """Three recordings that end inside the first, the third and the fifth block, so that every pattern crosses blocks, workgroups
    and recordings."""
    B = _block()
    lens = [B - 7, B + 100, 2 * B + 50]
    n = sum(lens)
    logp = sc.scores(pattern, n, 3)
    for lab_pattern in ("plain", "mixed"):
        labels = sc.labels_for(lab_pattern, lens, 4)
        for per in (False, True):
            _check(logp, None, labels, lens, per)


@pytest.mark.gpu
def test_label_patterns():
    """A class with no positives, a recording that is all ignored, labels 4 and 255; all labels ignored; labels given as int64
    with -100 and 256, as a list and as (B, T)."""
    lens = [300, 40, 2500]
    n = sum(lens)
    logp = sc.scores("eighths", n, 9)
    labels = sc.labels_for("mixed", lens, 9)
    assert not (labels == 3).any() and (labels == 4).any() and (labels == 255).any() and (labels[300:340] == 255).all()
    for per in (False, True):
        res = _check(logp, None, labels, lens, per)
        rk = res.rank.reshape(-1, 4, 3).cpu()
        assert (rk[:, 3, 1] == 0).all() and (rk[:, 3, 0] == 0).all()
        if per:
            assert int(res.ignored[1]) == 40 and int(res.confusion[1].sum()) == 0 and int(res.rank[1].sum()) == 0
    nothing = np.full(n, 255, dtype=np.uint8)
    res = _check(logp, None, nothing, lens, False)
    assert int(res.ignored) == n and bool(torch.isnan(res.auroc).all()) and bool(torch.isnan(res.macro_auroc))
    wide = labels.astype(np.int64)
    wide[labels == 4] = 256
    wide[labels == 255] = -100
    lp = RaggedFeatures(torch.from_numpy(logp).cuda(), torch.tensor(sc.offsets(lens)), 4, False)
    want = sc.restate(logp, None, labels, sc.offsets(lens), True)
    for given in (torch.from_numpy(wide).cuda(), [torch.from_numpy(wide[a:b]) for a, b in zip(sc.offsets(lens)[:-1], sc.offsets(lens)[1:])]):
        _equal(segmentation_scores(lp, given, per_recording=True), want, True)
    dense = torch.from_numpy(logp[:2400].reshape(3, 800, 4)).cuda()
    _equal(segmentation_scores(dense, torch.from_numpy(wide[:2400].reshape(3, 800)).cuda(), per_recording=True),
           sc.restate(logp[:2400], None, labels[:2400], [0, 800, 1600, 2400], True), True)
    _equal(segmentation_scores(dense[0], torch.from_numpy(wide[:800])), sc.restate(logp[:800], None, labels[:800], [0, 800], False), False)


@pytest.mark.gpu
@pytest.mark.parametrize("per", [False, True], ids=["pooled", "per recording"])
def test_prediction_inputs(per):
    """states alone (no rank), logp alone, both (the states are the predictions, the log-probs are ranked), argmax ties, states
    above 3 (ignored), auroc=False."""
    lens = [5000, 1, 777]
    n = sum(lens)
    g = np.random.default_rng(21)
    logp = sc.scores("eighths", n, 21)
    logp[::3] = logp[::3, [0]]                            # four-way argmax ties
    logp[1::5, 2] = logp[1::5, 3]
    logp[2::7, 1] = np.nan
    labels = sc.labels_for("mixed", lens, 21)
    states = g.integers(0, 4, size=n).astype(np.uint8)
    res = _check(None, states, labels, lens, per)
    assert res.rank is None
    _check(logp, None, labels, lens, per)
    both = _check(logp, states, labels, lens, per)
    alone = _run(logp, None, labels, lens, per)
    assert not torch.equal(both.confusion, alone.confusion) and torch.equal(both.rank, alone.rank)
    states[::13] = 7
    _check(logp, states, labels, lens, per)
    _check(logp, None, labels, lens, per, want_rank=False)
    for form in ("arena",):
        r = _run(logp[:5000], None, labels[:5000], [5000], per, form=form)
        _equal(r, sc.restate(logp[:5000], None, labels[:5000], [0, 5000], per), per)


@pytest.mark.gpu
def test_neighbours_do_not_matter():
    """A recording's per-recording integers are the same alone and inside the list of 300, and two calls give the same bits."""
    lens = sc.list_lens(300)
    offs = sc.offsets(lens)
    n = sum(lens)
    logp, labels = sc.scores("eighths", n, 31), sc.labels_for("mixed", lens, 31)
    whole = _run(logp, None, labels, lens, True)
    again = _run(logp, None, labels, lens, True)
    for k in ("confusion", "ignored", "rank"):
        assert torch.equal(getattr(whole, k), getattr(again, k))
    for i in (0, 1, 7, 150, 299):
        alone = _run(logp[offs[i]:offs[i + 1]], None, labels[offs[i]:offs[i + 1]], [lens[i]], True)
        for k in ("confusion", "ignored", "rank"):
            assert torch.equal(getattr(alone, k)[0], getattr(whole, k)[i]), (i, k)


@pytest.mark.gpu
@pytest.mark.parametrize("per", [False, True], ids=["pooled", "per recording"])
def test_derived_figures(per):
    """accuracy, precision, recall, F1, support, their macro means, AUROC (NaN where P N = 0) and its macro mean against the
    restatement's float64, to 1e-15 relative; float64 tensors on the device."""
    lens = [900, 40, 3000, 5]
    n = sum(lens)
    logp, labels = sc.scores("log_softmax", n, 41), sc.labels_for("mixed", lens, 41)
    res = _run(logp, None, labels, lens, per)
    want = sc.derived(sc.restate(logp, None, labels, sc.offsets(lens), per))
    for k, w in want.items():
        got = getattr(res, k)
        w = w if per else w[0]
        assert got.is_cuda and got.dtype == (torch.int64 if k == "support" else torch.float64), k
        got = got.cpu().numpy()
        assert got.shape == np.shape(w) and np.array_equal(np.isnan(got), np.isnan(w)), k
        ok = ~np.isnan(w)
        assert (np.abs(got[ok] - w[ok]) <= 1e-15 * np.abs(w[ok])).all(), (k, got, w)
    assert np.isnan(want["auroc"]).any() and not np.isnan(want["auroc"]).all()


@pytest.mark.gpu
def test_decoded_states_are_scored():
    """End to end: decode_states' RaggedStates scored against labels, with the log-probs ranked beside them."""
    lens = [1200, 1, 350]
    n = sum(lens)
    logp = sc.scores("log_softmax", n, 51)
    labels = sc.labels_for("plain", lens, 51)
    rf = RaggedFeatures(torch.from_numpy(logp).cuda(), torch.tensor(sc.offsets(lens)), 4, False)
    decoded = decode_states(rf)
    res = segmentation_scores(decoded, torch.from_numpy(labels).cuda(), per_recording=True, scores=rf)
    _equal(res, sc.restate(logp, decoded.data.cpu().numpy(), labels, sc.offsets(lens), True), True)
    assert int(res.confusion.sum()) == n


@pytest.mark.gpu
def test_no_kernel_uses_scratch(built_lib):
    found = _lib.kernel_resources("seg_score_")
    assert len(found) >= 10, sorted(found)
    for name, r in found.items():
        assert r["private_segment_fixed_size"] == 0 and r["agpr_count"] == 0 and r["group_segment_fixed_size"] <= 20 * 1024, (name, r)


# ------------------------------------------------------------------------------------------------ the caller's stream
SEQ = "sequence:_call"
SIDE_LENS = {"three recordings of 1, 130, 5000 steps": (1, 130, 5000), "300 recordings of 1..40 steps": tuple(i * 7 % 40 + 1 for i in range(300))}


def _side_case(tag, lens, per):
    offs = torch.tensor(sc.offsets(lens), dtype=torch.int64)

    def inputs(seed):
        return [torch.from_numpy(sc.scores("eighths", sum(lens), 60 + seed)), torch.from_numpy(sc.labels_for("mixed", lens, 60 + seed))]

    def call(ctx, xs, out):
        res = segmentation_scores(RaggedFeatures(xs[0], offs, 4, False), xs[1], per_recording=per)
        return [res.confusion, res.ignored, res.rank]

    def check(res, host):
        want = sc.restate(host[0].numpy(), None, host[1].numpy(), sc.offsets(lens), per)
        for t, k in zip(res, ("confusion", "ignored", "rank")):
            assert torch.equal(t.cpu(), torch.from_numpy(np.asarray(want[k] if per else want[k][0]))), k
    return Case(f"segmentation_scores {'per recording' if per else 'pooled'}, {tag}", {"hssfsst_score_states"}, {SEQ}, inputs=inputs, call=call,
                check=check)


SIDE_CASES = [_side_case(tag, lens, per) for tag, lens in SIDE_LENS.items() for per in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", SIDE_CASES, ids=lambda c: c.name)
def test_side_stream_held(case):
    """Scenario A of tests/side_stream.py: poison, a delay and the real input on the side stream, then the call: the bits of the
    default stream, and the call returned while the delay ran."""
    ss.scenario_a(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SIDE_CASES, ids=lambda c: c.name)
def test_null_stream_held(case):
    """Scenario B: stream 0 held, the call and a snapshot of its outputs on the side stream, all done while stream 0 still waits."""
    ss.scenario_b(case)


def header_launch_functions():
    with open(os.path.join(ROOT, "include", "hssfsst.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(hssfsst_\w+)\s*\(([^;{}]*)\)\s*;", text) if re.search(r"\bhssfsst_launch\s*\*", m.group(2))}


def test_every_entry_point_with_a_launch_struct_has_a_case():
    """Every function of include/hssfsst.h that takes its device and stream as a ``const hssfsst_launch*`` is reached by a case of
    both scenarios here: tests/test_stream_order.py finds its entries by their ``void* stream`` parameter and does not see these."""
    fns = header_launch_functions()
    assert "hssfsst_score_states" in fns, sorted(fns)
    covered = set().union(*[c.covers for c in SIDE_CASES])
    assert covered <= fns, sorted(covered - fns)
    assert not fns - covered, f"entry points with a hssfsst_launch parameter and no case in tests/test_segmentation_scores.py: {sorted(fns - covered)}"
    assert all(c.scenarios == "AB" and SEQ in c.sites for c in SIDE_CASES)
    for per in ("pooled", "per recording"):
        assert any(per in c.name for c in SIDE_CASES)
