"""Every entry point that takes a stream, held to its default-stream result on a side stream (tests/side_stream.py: scenario A holds
the side stream behind the call's input, scenario B holds stream 0 while the call and a snapshot of its outputs run on the side
stream).  One table of cases, the smallest shapes at which each path exists; controls that prove the harness reports a stray
stage; two CPU tests that fail when an entry point or a ``current_stream`` call site of the package has no case."""
import ast
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from heart_sounds_segmentation_amd import FSST, Resample, _lib, consumer, synth
from heart_sounds_segmentation_amd.corpus import CorpusBuilder
from heart_sounds_segmentation_amd.sequence import (cyclic_transitions, decode_durations, decode_states, duration_nll,
                                                    duration_posteriors, edge_durations, gaussian_durations, sequence_nll,
                                                    state_posteriors)
from heart_sounds_segmentation_amd.streaming import StreamingFSST
from heart_sounds_segmentation_amd.transforms.synchrosqueeze import RaggedFeatures
from tests import decode_cases, duration_cases, parity, segmenter_cases
from tests import duration_posterior_cases as dpc
from tests import posterior_cases as pc
from tests import side_stream as ss
from tests.launch_cases import BAND, LAUNCH_CASES, launch_call, launch_inputs, launch_kernel, launch_transform
from tests.side_stream import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "heart_sounds_segmentation_amd")

# the package's functions that read the current stream, as the call-site test names them
S_RUN, S_FRAMES, S_RAGGED = (f"transforms.synchrosqueeze:FSST.{f}" for f in ("_run", "frames", "ragged"))
R_EXEC, R_RAGGED = "transforms.resample:_ResamplePlan.exec", "transforms.resample:_RaggedResamplePlan.exec"
SEG_CALL, SEG_RAGGED = "consumer:HipSegmenter.__call__", "consumer:HipSegmenter.ragged"
TRAIN = {"consumer:_BiLSTMFunction.forward", "consumer:_BiLSTMFunction.backward", "consumer:HipBiLSTM._sync_plan"}
TRAIN_RAGGED = {"consumer:_RaggedBiLSTMFunction.forward", "consumer:_RaggedBiLSTMFunction.backward", "consumer:HipBiLSTM._sync_plan"}
SEQ = "sequence:_call"
ST_NATIVE, ST_STEP, ST_UNFUSED = (f"streaming:StreamingFSST.{f}" for f in ("_native_step", "step", "step_unfused"))
PIPELINE = "corpus:CorpusBuilder._pipeline"

# entry points with a stream parameter that no case here reaches, and why
EXCLUDED = {"hssfsst_allgather": "a collective over several ranks: exercised by tests/test_dist.py, which owns the process group"}

KAISER = synth.kaiser_window(128, 0.5)


def _canon(**kw):
    return FSST(1000, KAISER, truncate_freq=BAND, stack=True, **kw)


def _randn(seed, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ------------------------------------------------------------------------------------------------ FSST
def _oracle_check(c):
    def check(res, host):
        import oracle
        oracle.build()
        X = host[0].numpy()
        ref, hd = oracle.features(X, c["fs"], synth.kaiser_window(c["nwin"], 0.5), c["band"], "stack", return_halfdist=True)
        got = res.cpu().numpy()
        for b in range(X.shape[0]):
            parity.check(got[b], ref[b], hd[b], 0, what=f"stream order, signal {b}")
    return check


def _launch_case(name, c, want):
    ragged = "ragged" in c

    def after(tf, what):
        got = launch_kernel(tf, c).split(" [")[0]
        assert got == want, (what, got, want)
    return Case(f"fsst launch: {name}", {"hssfsst_exec_ragged"} if ragged else {"hssfsst_exec_frames"}, {S_RAGGED if ragged else S_RUN},
                inputs=lambda seed: launch_inputs(c, 1234 + seed), context=lambda: launch_transform(c),
                call=lambda tf, xs, out: launch_call(tf, c, xs), after=after,
                check=_oracle_check(c) if name == "the workload's length" else None)


def _frame_starts(seed):
    g = torch.Generator().manual_seed(100 + seed)
    return torch.randint(0, 13337 - 333 + 1, (64,), generator=g, dtype=torch.int64)


def _capi(entry):
    """hssfsst_exec / hssfsst_exec_cols, which the Python layer does not call (it goes through hssfsst_exec_frames)."""
    def call(tf, xs, out):
        x = xs[0]
        plan = tf._plan(0)
        B, n = int(x.shape[0]), int(x.shape[1])
        cols = (0, n) if entry == "hssfsst_exec" else (40, 300)
        res = torch.empty((B, cols[1], plan.ofps), dtype=torch.float32, device=x.device)
        vp = ctypes.c_void_p
        stream = vp(torch.cuda.current_stream().cuda_stream)
        if entry == "hssfsst_exec":
            rc = _lib.lib().hssfsst_exec(plan.handle, vp(x.data_ptr()), B, n, 1, vp(res.data_ptr()), 1, stream)
        else:
            rc = _lib.lib().hssfsst_exec_cols(plan.handle, vp(x.data_ptr()), B, n, cols[0], cols[1], 1, vp(res.data_ptr()), 1, stream)
        _lib.check(rc, entry)
        return res
    return Case(f"C ABI: {entry}", {entry}, set(), inputs=lambda seed: [_randn(40 + seed, 2, 500)], context=_canon, call=call)


def fsst_cases():
    out = [_launch_case(*row) for row in LAUNCH_CASES]
    out.append(Case("fsst frames, starts on the device", {"hssfsst_exec_list"}, {S_FRAMES},
                    inputs=lambda seed: [_randn(20 + seed, 13337), _frame_starts(seed)], context=_canon,
                    call=lambda tf, xs, out: tf.frames(xs[0], xs[1], 333)))
    out.append(Case("fsst frames, starts on the host", {"hssfsst_exec_list"}, {S_FRAMES},
                    inputs=lambda seed: [_randn(20 + seed, 13337)], context=_canon,
                    call=lambda tf, xs, out: tf.frames(xs[0], _frame_starts(0), 333)))
    out.append(Case("fsst batch with out=", {"hssfsst_exec_frames"}, {S_RUN}, inputs=lambda seed: [_randn(30 + seed, 3, 500)],
                    context=_canon, out=lambda tf, xs: torch.empty((3, 500, 44), dtype=torch.float32, device="cuda"),
                    call=lambda tf, xs, out: tf.batch(xs[0], out=out)))
    out.append(Case("fsst batch of a host tensor", {"hssfsst_exec_frames"}, {S_RUN}, inputs=lambda seed: [_randn(32 + seed, 2, 2000)],
                    context=_canon, call=lambda tf, xs, out: tf.batch(xs[0]), host=True, blocking=True))
    out.append(Case("fsst single host frame (hssfsst_exec_pinned)", set(), set(), inputs=lambda seed: [_randn(34 + seed, 2000, 1)],
                    context=_canon, call=lambda tf, xs, out: tf(xs[0]).clone(), host=True, blocking=True, scenarios="A",
                    why_not_b="hssfsst_exec_pinned has no stream parameter and runs on stream 0 by contract"))
    out.append(Case("fsst cold plan", {"hssfsst_exec_frames"}, {S_RUN}, inputs=lambda seed: [_randn(36 + seed, 2, 2000)],
                    context=_canon, call=lambda tf, xs, out: tf.batch(xs[0]), warm=False, scenarios="A",
                    why_not_b="creating a plan uploads its tables with a synchronous copy, which waits for stream 0 by right"))
    out += [_capi("hssfsst_exec"), _capi("hssfsst_exec_cols")]
    return out


# ------------------------------------------------------------------------------------------------ streaming
def _streaming_reset(st):
    st.tape.zero_()
    st.state.zero_()
    st.pos = st.hist


def _streaming_case(kind, chunk):
    covers = {"step": {"hssfsst_stream_step"}, "step_host": {"hssfsst_stream_step"},
              "step_unfused": {"hssfsst_exec_frames", "hssfsst_moments_merge", "hssfsst_normalize_running"}}[kind]
    sites = {"step": {ST_NATIVE, ST_STEP}, "step_host": {ST_NATIVE}, "step_unfused": {ST_UNFUSED}}[kind]
    host = kind == "step_host"

    def inputs(seed):
        xs = [_randn(200 + 10 * seed + i, 3, chunk) for i in range(6)]
        return [x.numpy() for x in xs] if host else xs

    def call(st, xs, out):                               # six steps: with slots = 2 the tape wraps every two
        if kind == "step":
            return [st.step(x) for x in xs]
        if kind == "step_unfused":
            return [st.step_unfused(x).clone() for x in xs]
        return [torch.from_numpy(st.step_host(x).copy()) for x in xs]
    return Case(f"streaming {kind}, chunk {chunk}", covers, sites, inputs=inputs, call=call, reset=_streaming_reset, host=host, blocking=host,
                context=lambda: StreamingFSST(3, 1000, KAISER, truncate_freq=BAND, chunk=chunk, slots=2))


def streaming_cases():
    return [_streaming_case(kind, chunk) for kind in ("step", "step_unfused", "step_host") for chunk in (17, 128)]


# ------------------------------------------------------------------------------------------------ resample
def _resample_check(num):
    def check(res, host):
        got = res.cpu().numpy()
        for i in range(got.shape[0]):
            ref = Resample(num)(host[0][i], torch.float64).numpy()
            assert np.abs(got[i] - ref).max() / max(np.abs(ref).max(), 1.0) <= 1e-12, i
    return check


RAGGED_LENS = [4100, 3, 1030, 2000]


def resample_cases():
    def tracks(seed, *shape):                            # label tracks as floats, 1..4 in runs
        g = torch.Generator().manual_seed(300 + seed)
        return torch.randint(1, 5, shape, generator=g).float().repeat_interleave(50, dim=-1)
    return [
        Case("resample batch 3 x 2000 -> 1000 (LDS tier)", {"hssfsst_resample_exec"}, {R_EXEC},
             inputs=lambda seed: [_randn(50 + seed, 3, 2000, dtype=torch.float64)], context=lambda: Resample(1000),
             call=lambda rs, xs, out: rs.batch(xs[0], torch.float64), check=_resample_check(1000)),
        Case("resample strided 3 x 4097 -> 1000 at stride 950 (multi-pass tier)", {"hssfsst_resample_exec"}, {R_EXEC},
             inputs=lambda seed: [_randn(52 + seed, 2 * 950 + 4097)], context=lambda: Resample(1000),
             call=lambda rs, xs, out: rs.batch(xs[0].as_strided((3, 4097), (950, 1)))),
        Case("resample frames with labels", {"hssfsst_resample_exec"}, {R_EXEC},
             inputs=lambda seed: [tracks(seed, 160), torch.tensor([0, 1000, 2500, 6000, 3333 + seed], dtype=torch.int64)],
             context=lambda: Resample(1000), call=lambda rs, xs, out: rs.frames(xs[0], xs[1], 2000, labels=True)),
        Case("resample ragged -> 50", {"hssfsst_resample_exec_ragged"}, {R_RAGGED},
             inputs=lambda seed: [_randn(54 + seed + i, n) for i, n in enumerate(RAGGED_LENS)], context=lambda: Resample(50),
             call=lambda rs, xs, out: rs.ragged(list(xs))),
        Case("resample ragged -> 50 with labels", {"hssfsst_resample_exec_ragged"}, {R_RAGGED},
             inputs=lambda seed: [tracks(seed + i, -(-n // 50))[:n].contiguous() for i, n in enumerate(RAGGED_LENS)], context=lambda: Resample(50),
             call=lambda rs, xs, out: rs.ragged(list(xs), labels=True)),
        Case("resample device call on a host signal", {"hssfsst_resample_exec"}, {R_EXEC}, inputs=lambda seed: [_randn(58 + seed, 2000)],
             context=lambda: Resample(1000, device="cuda"), call=lambda rs, xs, out: rs(xs[0]), host=True, blocking=True),
    ]


# ------------------------------------------------------------------------------------------------ segmenter inference
RAGGED_515 = tuple(range(515, 531)) + (522,)


def _segmenter_dense(B, T, H, Fd, checked):
    def check(res, host):
        ref = segmenter_cases.dense_case(B, T, H, Fd).ref64
        assert float((res.cpu().double() - ref).abs().max()) <= segmenter_cases.GATE
    return Case(f"segmenter dense ({B}, {T}, {H}, {Fd})", {"hssfsst_segmenter_exec"}, {SEG_CALL},
                inputs=lambda seed: [segmenter_cases.dense_case(B, T, H, Fd).x if seed == 0 else segmenter_cases.features((B, T, Fd), 77)],
                context=lambda: segmenter_cases.dense_case(B, T, H, Fd).head.hip(), call=lambda seg, xs, out: seg(xs[0]),
                check=check if checked else None)


def _segmenter_ragged(lens, max_steps=None):
    kw = {} if max_steps is None else {"max_steps": max_steps}
    B = len(lens)
    return Case(f"segmenter ragged {list(lens) if B < 5 else f'{B} recordings of {min(lens)}..{max(lens)} steps'}"
                + (f", max_steps {max_steps}" if max_steps else ""), {"hssfsst_segmenter_exec_ragged"}, {SEG_RAGGED},
                inputs=lambda seed: [segmenter_cases.features((T, 44), 900 + 31 * seed + i) for i, T in enumerate(lens)],
                context=lambda: segmenter_cases.conditioned_head(B, 16, 44, 5).hip(), call=lambda seg, xs, out: seg.ragged(list(xs), **kw))


def segmenter_cases_():
    recs = (100, 700, 333)
    return [
        _segmenter_dense(17, 37, 240, 44, True),
        _segmenter_dense(2, 1030, 16, 44, False),       # crosses the 1024-step launch border
        _segmenter_ragged(RAGGED_515),
        # the Python group loop runs more than once: [1600] is a group of its own, [3, 1030] the second.  (1600 steps, not 4100: one
        #  workgroup walks a recording; [4100, 3, 1030] took 78 ms on the idle default stream and [2100, 3, 1030] 48 ms, and 4 x the
        #  time must stay under the harness's limit of 250 ms with room for a slower day)
        _segmenter_ragged((1600, 3, 1030), max_steps=1500),
        Case("segment_recordings end to end, decoded", {"hssfsst_exec_ragged", "hssfsst_segmenter_exec_ragged", "hssfsst_decode_states"},
             {S_RAGGED, SEG_RAGGED, SEQ},
             inputs=lambda seed: [torch.from_numpy(synth.pcg_windows(3, 2000, seed=22 + seed)[i, :n].copy()) for i, n in enumerate(recs)],
             context=lambda: (_canon(), segmenter_cases.conditioned_head(3, 16, 44, 31).hip()),
             call=lambda ctx, xs, out: consumer.segment_recordings(ctx[0], ctx[1], list(xs), decode=True)),
    ]


# ------------------------------------------------------------------------------------------------ the training layer
def _train_context(B):
    def make():
        head = segmenter_cases.conditioned_head(B, 16, 44, 11, cls=consumer.HipSegmenterHead).cuda()
        ctx = {"head": head, "init": {k: v.detach().clone() for k, v in head.state_dict().items()}}
        _train_reset(ctx)
        return ctx
    return make


def _train_reset(ctx):
    ctx["head"].load_state_dict(ctx["init"])
    for p in ctx["head"].parameters():
        p.grad = None
    ctx["opt"] = torch.optim.Adam(ctx["head"].parameters(), lr=1e-3)


def _train_call(ragged_offsets=None):
    """forward, nll_loss, backward, one Adam step (the next forward repacks the weights: hssfsst_bilstm_set_weights), a second
    forward -> loss, every parameter gradient, dx, the second forward."""
    def call(ctx, xs, out):
        head, opt = ctx["head"], ctx["opt"]
        x, labels = xs[0].requires_grad_(), xs[1]

        def forward(v):
            if ragged_offsets is None:
                return head(v).reshape(-1, 4)
            return head.ragged(RaggedFeatures(v, torch.tensor(ragged_offsets, dtype=torch.int64), 22, False)).data
        loss = F.nll_loss(forward(x), labels.reshape(-1))
        loss.backward()
        grads = [p.grad.clone() for p in head.parameters()]
        opt.step()
        with torch.no_grad():
            second = forward(x.detach())
        return [loss.detach(), grads, x.grad, second]
    return call


def train_cases():
    lens = (100, 700, 333)
    offs = [0] + list(np.cumsum(lens))

    def labels(seed, *shape):
        return torch.randint(0, 4, shape, generator=torch.Generator().manual_seed(400 + seed), dtype=torch.int64)
    return [
        Case("training head dense (3, 37)", {"hssfsst_bilstm_set_weights", "hssfsst_bilstm_forward", "hssfsst_bilstm_backward"}, TRAIN,
             inputs=lambda seed: [segmenter_cases.features((3, 37, 44), 410 + seed), labels(seed, 3, 37)], context=_train_context(3),
             call=_train_call(), reset=_train_reset),
        Case("training head ragged [100, 700, 333]",
             {"hssfsst_bilstm_set_weights", "hssfsst_bilstm_forward_ragged", "hssfsst_bilstm_backward_ragged"}, TRAIN_RAGGED,
             inputs=lambda seed: [segmenter_cases.features((sum(lens), 44), 420 + seed), labels(seed, sum(lens))], context=_train_context(3),
             call=_train_call([int(o) for o in offs]), reset=_train_reset),
    ]


# ------------------------------------------------------------------------------------------------ sequence models
LISTS = {"three recordings of 1, 130, 700 steps": (1, 130, 700), "300 recordings of 1..40 steps": tuple(i * 7 % 40 + 1 for i in range(300))}
D = 129


def _logp(lens, seed):
    return torch.log_softmax(3.0 * _randn(500 + seed, sum(lens), 4), dim=1)


def _cyclic_labels(lens):
    """Legal under cyclic_transitions() and every duration table here: runs of 7 steps, 0 1 2 3 0 ..., per recording."""
    return torch.cat([(torch.arange(T) // 7 % 4).to(torch.uint8) for T in lens])


def _tables():
    A, pi = cyclic_transitions()
    dur = gaussian_durations([30.0, 50.0, 25.0, 80.0], [8.0, 12.0, 6.0, 30.0], D)
    return {"A": np.asarray(A, dtype=np.float32), "pi": np.asarray(pi, dtype=np.float32), "dur": np.asarray(dur, dtype=np.float32),
            "edge": np.asarray(edge_durations(dur), dtype=np.float32)}


def _device_tables():
    return {k: torch.from_numpy(v).cuda() for k, v in _tables().items()}


def _sequence_case(what, tag, lens, covers, call, check=None, labels=False, blocking=False):
    offs = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int64)

    def run(ctx, xs, out):
        return call(ctx, (lambda t: RaggedFeatures(t, offs, 4, False)), xs)
    return Case(f"{what}, {tag}", covers, {SEQ}, inputs=lambda seed: [_logp(lens, seed)] + ([_cyclic_labels(lens)] if labels else []),
                context=_device_tables, call=run, poison=0.0 if not labels else None, blocking=blocking,
                check=(lambda res, host: check(res, host, lens)) if check else None)


def _split(a, lens):
    offs = [0] + list(np.cumsum(lens))
    return [a[offs[i]:offs[i + 1]] for i in range(len(lens))]


def _check_decode(res, host, lens):
    t = _tables()
    es = _split(host[0].numpy(), lens)
    paths, _ = decode_cases.viterbi(es, [t["A"]] * len(es), [t["pi"]] * len(es))
    assert np.array_equal(res.data.cpu().numpy(), np.concatenate(paths))


def _check_decode_durations(res, host, lens):
    t = _tables()
    paths, _ = duration_cases.decode_list(_split(host[0].numpy(), lens), t["A"], t["pi"], t["dur"], t["edge"])
    assert np.array_equal(res.data.cpu().numpy(), np.concatenate(paths))


def _check_posteriors(res, host, lens):
    t = _tables()
    es = _split(host[0].numpy(), lens)
    wg, wlz, _ = pc.forward_backward(es, [t["A"]] * len(es), [t["pi"]] * len(es))
    got = _split(res[0].data.cpu().numpy().astype(np.float64), lens)
    for i in range(len(es)):
        assert np.abs(got[i] - wg[i]).max() <= 2.0 ** -23, i                     # GAMMA_GATE of tests/test_posteriors.py
    assert np.abs(res[1].cpu().numpy() - np.asarray(wlz)).max() <= 8 * 5.54e-10  # Z_GATE of tests/test_duration_posteriors.py


def _check_duration_posteriors(res, host, lens):
    t = _tables()
    got = _split(res[0].data.cpu().numpy().astype(np.float64), lens)
    for i, e in enumerate(_split(host[0].numpy(), lens)):
        w = dpc.forward_backward(e, t["A"], t["pi"], t["dur"], t["edge"])
        assert np.abs(got[i] - w["gamma"]).max() <= 2.0 ** -23, i                # GAMMA_GATE of tests/test_duration_posteriors.py


def _nll(fn, durations):
    def call(ctx, rf, xs):
        x = xs[0].requires_grad_()
        A, pi = (ctx[k].clone().requires_grad_() for k in ("A", "pi"))
        if durations:
            dur, edge = (ctx[k].clone().requires_grad_() for k in ("dur", "edge"))
            loss = fn(rf(x), xs[1], dur, A, pi, edge=edge, learn_durations=True)
            loss.backward()
            return [loss.detach(), x.grad, A.grad, pi.grad, dur.grad, edge.grad]
        loss = fn(rf(x), xs[1], A, pi)
        loss.backward()
        return [loss.detach(), x.grad, A.grad, pi.grad]
    return call


def sequence_cases():
    out = []
    for n, (tag, lens) in enumerate(LISTS.items()):
        first = n == 0                                   # the float64 checks walk Python loops: on the short list only
        out += [
            _sequence_case("decode_states", tag, lens, {"hssfsst_decode_states"},
                           lambda ctx, rf, xs: decode_states(rf(xs[0])), _check_decode if first else None),
            _sequence_case(f"decode_durations at D = {D}", tag, lens, {"hssfsst_decode_durations"},
                           lambda ctx, rf, xs: decode_durations(rf(xs[0]), _tables()["dur"]), _check_decode_durations if first else None),
            _sequence_case("state_posteriors with logZ", tag, lens, {"hssfsst_posteriors"},
                           lambda ctx, rf, xs: state_posteriors(rf(xs[0]), ctx["A"], ctx["pi"], return_loglik=True), _check_posteriors),
            _sequence_case("sequence_nll forward and backward, learnable transitions", tag, lens, {"hssfsst_posteriors"},
                           _nll(sequence_nll, False), labels=True),
            _sequence_case("duration_posteriors with counts and onsets", tag, lens, {"hssfsst_posteriors_durations_counts"},
                           lambda ctx, rf, xs: duration_posteriors(rf(xs[0]), ctx["dur"], ctx["A"], ctx["pi"], edge=ctx["edge"],
                                                                   return_counts=True, return_onsets=True),
                           _check_duration_posteriors if first else None),
            _sequence_case("duration_posteriors", tag, lens, {"hssfsst_posteriors_durations"},
                           lambda ctx, rf, xs: duration_posteriors(rf(xs[0]), ctx["dur"], ctx["A"], ctx["pi"], edge=ctx["edge"])),
            _sequence_case("duration_nll forward and backward, learn_durations", tag, lens, {"hssfsst_posteriors_durations_counts"},
                           _nll(duration_nll, True), labels=True),
        ]
    out.append(_sequence_case("decode_states with scores", "300 recordings of 1..40 steps", LISTS["300 recordings of 1..40 steps"],
                              {"hssfsst_decode_states"}, lambda ctx, rf, xs: decode_states(rf(xs[0]), return_scores=True), blocking=True))
    return out


# ------------------------------------------------------------------------------------------------ corpus builders
REC_LENS = (35000, 2500, 1999, 12345, 4000)
WHY_BUILDERS_NOT_B = ("every build ends in FSST.check(), which is hssfsst_plan_check: a hipDeviceSynchronize by contract "
                      "(\"waits for the device and checks now\"), so the call waits for stream 0 by right")


def _recordings(seed):
    g = torch.Generator().manual_seed(600 + seed)
    return [(torch.from_numpy(synth.recording(T, seed=70 + 5 * seed + i).astype(np.float32)),
             torch.randint(1, 5, (-(-T // 100),), generator=g, dtype=torch.int64).repeat_interleave(100)[:T].contiguous())
            for i, T in enumerate(REC_LENS)]


def corpus_cases():
    out = []
    for keep in (True, False):
        where = "kept on the device" if keep else "copied to the host"
        for rsm in (False, True):
            out.append(Case(f"CorpusBuilder.build{' with Resample(1000)' if rsm else ''}, {where}",
                            {"hssfsst_exec_list"} if not rsm else {"hssfsst_resample_exec", "hssfsst_exec_frames"},
                            {PIPELINE, S_FRAMES} if not rsm else {PIPELINE, R_EXEC, S_RUN},
                            inputs=lambda seed: [_recordings(seed)], host=True, blocking=True, scenarios="A", why_not_b=WHY_BUILDERS_NOT_B,
                            context=(lambda rsm=rsm: CorpusBuilder(_canon(), windows_per_launch=4, resample=Resample(1000) if rsm else None)),
                            call=lambda b, xs, out, keep=keep: b.build(xs[0], keep_on_device=keep)))
        out.append(Case(f"CorpusBuilder.build_recordings, {where}", {"hssfsst_exec_ragged"}, {PIPELINE, S_RAGGED},
                        inputs=lambda seed: [_recordings(seed)], host=True, blocking=True, scenarios="A", why_not_b=WHY_BUILDERS_NOT_B,
                        context=lambda: CorpusBuilder(_canon()),
                        call=lambda b, xs, out, keep=keep: b.build_recordings(xs[0], keep_on_device=keep, max_samples=20000).features))
        out.append(Case(f"CorpusBuilder.build_resampled_recordings, {where}", {"hssfsst_resample_exec_ragged", "hssfsst_exec_frames"},
                        {PIPELINE, R_RAGGED, S_RUN},
                        inputs=lambda seed: [_recordings(seed)], host=True, blocking=True, scenarios="A", why_not_b=WHY_BUILDERS_NOT_B,
                        context=lambda: CorpusBuilder(_canon(), resample=Resample(1000)),
                        call=lambda b, xs, out, keep=keep: b.build_resampled_recordings(xs[0], keep_on_device=keep, max_samples=20000)))
    return out


CASES = fsst_cases() + streaming_cases() + resample_cases() + segmenter_cases_() + train_cases() + sequence_cases() + corpus_cases()
assert len({c.name for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------------ the controls
def _standin(stray):
    """A stand-in entry point written from torch ops on valid tensors: stage 1 clears the scratch, stage 2 adds the input to it and
    writes twice the sum to the output.  ``stray``: the stage that is enqueued on stream 0 instead of the current stream."""
    def call(ctx, xs, out):
        cur, null = torch.cuda.current_stream(), torch.cuda.default_stream()
        with torch.cuda.stream(null if stray == 1 else cur):
            ctx["scratch"].zero_()
        with torch.cuda.stream(null if stray == 2 else cur):
            ctx["scratch"].add_(xs[0])
            torch.mul(ctx["scratch"], 2.0, out=out)
        return out
    return Case(f"control: stand-in with {'no stage' if not stray else f'stage {stray}'} on stream 0", set(), set(),
                inputs=lambda seed: [_randn(800 + seed, 1 << 16)], call=call,
                context=lambda: {"scratch": torch.zeros(1 << 16, device="cuda")},
                reset=lambda ctx: ctx["scratch"].fill_(1.0),      # what the scratch holds before a run: not zero, and known
                out=lambda ctx, xs: torch.empty(1 << 16, device="cuda"))


@pytest.mark.gpu
def test_controls_are_reported():
    """The harness on stand-ins whose fault is known: a second stage on stream 0 is reported by A and by B, a first stage (the
    clear of the scratch) on stream 0 by B, and the stand-in that keeps to the current stream passes both.  They race on valid
    tensors only."""
    clean, first, second = _standin(0), _standin(1), _standin(2)
    ss.scenario_a(clean)
    ss.scenario_b(clean)
    ss.report("control, every stage on the current stream: A passed, B passed")
    for case, scenario in ((second, ss.scenario_a), (second, ss.scenario_b), (first, ss.scenario_b)):
        with pytest.raises(ss.StreamOrderError) as err:
            scenario(case)
        assert "differs from the default-stream result" in str(err.value), str(err.value)
        ss.report(f"control reported: {err.value}")


# ------------------------------------------------------------------------------------------------ the cases
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_side_stream_held(case):
    """Scenario A: poison, a delay and the real input on the side stream, then the call: the bits of the default stream."""
    ss.scenario_a(case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if "B" in c.scenarios], ids=lambda c: c.name)
def test_null_stream_held(case):
    """Scenario B: stream 0 held, the call and a snapshot of its outputs on the side stream, all done while stream 0 still waits."""
    ss.scenario_b(case)


_SIDE_CHILD = r"""
import sys, torch
from heart_sounds_segmentation_amd import FSST, synth
cycles = int(sys.argv[2])
tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True)
side = torch.cuda.Stream() if cycles else None
outs = []
for n, seed in ((2000, 5), (500, 6)):
    X = torch.from_numpy(synth.pcg_windows(40, n, seed=seed)).cuda()
    if side is None:
        got = tf.batch(X)
    else:
        tf.batch(torch.flip(X, [0]))                      # the plan's buffers, on other data
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            buf = torch.full_like(X, float("nan"))
            torch.cuda._sleep(cycles)
            end = torch.cuda.Event()
            end.record(side)
            buf.copy_(X, non_blocking=True)
            got = tf.batch(buf)
            print("IN_TIME", not end.query(), flush=True)
        side.synchronize()
    print("PATH", tf.check(), "FALLBACKS", tf.fallbacks())
    outs.append(got.cpu())
torch.save(outs, sys.argv[1])
"""


@pytest.mark.gpu
def test_gated_fallback_on_a_held_side_stream(tmp_path):
    """The kernels queued behind every team launch, gated on its give-up (HSSFSST_TEAM_FORCE_FALLBACK=1 makes every team launch find
    itself given up), on a side stream behind a delay, at 40 x 2000 (the one-CU-per-signal kernel backs up) and 40 x 500 (three
    launches): the bits of the plain child on the default stream.

    The forced call is a blocking one, so there is no query() assertion here: the switch itself uploads the launch's identity from
    pageable host memory (fsst_team.hip, launch_team16), and such a copy makes the host wait for the stream.  Measured: under a 30 ms
    delay the forced call returned after 30.1 ms, the plain one after 0.08 ms (profiles/stream_order.txt).  The plain team launch on
    a held side stream is the LAUNCH_CASES rows above, which do assert it."""
    cycles = int(1e3 * ss.DEFAULT_DELAY_S * ss.calibrate())
    got = {}
    for name, env, c in (("plain", {}, 0), ("forced", {"HSSFSST_TEAM_FORCE_FALLBACK": "1"}, cycles)):
        f = str(tmp_path / f"{name}.pt")
        r = subprocess.run([sys.executable, "-c", _SIDE_CHILD, f, str(c)], cwd=ROOT, env=dict(os.environ, **env), capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        got[name] = (torch.load(f), r.stdout)
    print(got["forced"][1])
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert got["plain"][1].count("FALLBACKS 0") == 2 and "FALLBACKS 0" not in got["forced"][1], [g[1] for g in got.values()]
    for a, b in zip(got["plain"][0], got["forced"][0]):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ hand-over between streams
def _bilstm_call(layer, x):
    B = int(x.shape[0])
    h0, c0 = (torch.zeros(2, B, layer.hidden_size, device=x.device) for _ in range(2))
    v = x.clone().requires_grad_()
    y, (hn, cn) = layer(v, (h0, c0))
    for p in layer.parameters():
        p.grad = None
    (y.sum() + hn.sum() + cn.sum()).backward()
    return [y.detach(), hn.detach(), cn.detach(), v.grad, [p.grad for p in layer.parameters()]]


def _handover_objects():
    torch.manual_seed(3)
    return [
        ("FSST plan", _canon(), lambda tf, x: tf.batch(x), _randn(1, 3, 2000)),
        ("Resample", Resample(1000), lambda rs, x: rs.batch(x), _randn(2, 3, 2000)),
        ("HipSegmenter", segmenter_cases.conditioned_head(3, 16, 44, 9).hip(), lambda seg, x: seg(x), segmenter_cases.features((3, 37, 44), 3)),
        ("HipBiLSTM", consumer.HipBiLSTM(44, 16).cuda(), _bilstm_call, segmenter_cases.features((3, 37, 44), 4)),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["host synchronisation", "wait_stream"])
def test_plans_are_handed_from_stream_to_stream(order):
    """One plan of each kind used on the default stream, a side stream, a second side stream and the default stream again, the
    streams ordered by a host synchronisation or by events only (include/hssfsst.h: one stream at a time, in device order): every
    result equals the first."""
    side, second = ss.streams()
    null = torch.cuda.default_stream()
    for name, obj, call, x in _handover_objects():
        x = x.cuda()
        torch.cuda.synchronize()
        results, prev = [], None
        for s in (null, side, second, null):
            if prev is not None:
                if order == "wait_stream":
                    s.wait_stream(prev)
                else:
                    prev.synchronize()
            with torch.cuda.stream(s):
                results.append(ss.flatten(call(obj, x)))
            prev = s
        torch.cuda.synchronize()
        want = [ss.bits(t) for t in results[0]]
        for i, r in enumerate(results[1:]):
            assert [ss.bits(t) for t in r] == want, (name, order, i + 1)


@pytest.mark.gpu
def test_the_record_is_closed():
    """Runs last: the total of the session goes to the record."""
    ss.finish()


# ------------------------------------------------------------------------------------------------ keeping the gap closed (no GPU)
def header_stream_functions():
    with open(os.path.join(ROOT, "include", "hssfsst.h")) as fh:
        text = re.sub(r"/\*.*?\*/", " ", fh.read(), flags=re.S)
    return {m.group(1) for m in re.finditer(r"\b(hssfsst_\w+)\s*\(([^;{}]*)\)\s*;", text) if re.search(r"void\s*\*\s*stream\b", m.group(2))}


def test_every_entry_point_with_a_stream_has_a_case():
    """Every function of include/hssfsst.h with a ``void* stream`` parameter is reached by a case, or excluded with a reason; a new
    entry point without a case fails here."""
    fns = header_stream_functions()
    assert len(fns) >= 23 and "hssfsst_exec" in fns and "hssfsst_bilstm_backward_ragged" in fns, sorted(fns)
    covered = set().union(*[c.covers for c in CASES])
    assert covered <= fns, sorted(covered - fns)         # (no stale names)
    assert set(EXCLUDED) <= fns and not (set(EXCLUDED) & covered)
    missing = fns - covered - set(EXCLUDED)
    assert not missing, f"entry points with a stream parameter and no case in tests/test_stream_order.py: {sorted(missing)}"
    assert sorted(EXCLUDED) == ["hssfsst_allgather"]
    only_a = sorted(c.name for c in CASES if c.scenarios == "A")
    assert all(c.why_not_b for c in CASES if c.scenarios == "A"), only_a


def current_stream_sites():
    """"module:Qualified.name" of every function of the package that calls ``current_stream``."""
    found = set()
    for dirpath, _, files in os.walk(PKG):
        for f in files:
            if not f.endswith(".py"):
                continue
            path = os.path.join(dirpath, f)
            mod = os.path.relpath(path, PKG)[:-3].replace(os.sep, ".")
            with open(path) as fh:
                tree = ast.parse(fh.read())

            def walk(node, scope):
                for child in ast.iter_child_nodes(node):
                    if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                        walk(child, scope + [child.name])
                        continue
                    if isinstance(child, ast.Call):
                        fn = child.func
                        if (fn.attr if isinstance(fn, ast.Attribute) else getattr(fn, "id", None)) == "current_stream":
                            found.add(f"{mod}:{'.'.join(scope) or '<module>'}")
                    walk(child, scope)
            walk(tree, [])
    return found


def test_every_current_stream_call_site_has_a_case():
    """Every function of the package that reads the current stream is named by a case: a new call site without one fails here."""
    sites = current_stream_sites()
    assert len(sites) >= 17, sorted(sites)
    named = set().union(*[c.sites for c in CASES])
    assert named <= sites, sorted(named - sites)         # (no stale names)
    assert not sites - named, f"functions that read the current stream and have no case: {sorted(sites - named)}"
