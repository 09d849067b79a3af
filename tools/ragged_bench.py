"""Timing of the ragged transform (FSST.ragged / hssfsst_exec_ragged, corpus.build_recordings) on the C3-shaped stand-in:
792 recordings of seeded lengths in [20 000, 60 000) samples, STACK, Kaiser(128, 0.5), [25, 200] Hz.

    python tools/ragged_bench.py [--out FILE]   (a) device-resident: a loop of tf.batch(x[None]) per recording against one
                                                tf.ragged(list); (b) host-fed: a loop of tf(x_cpu) per recording (the lazy dataset's
                                                call) against build_recordings(..., keep_on_device=False); (c) core kernel time
                                                (plan timing events) of the ragged launch against the SAME kernel on a dense batch
                                                of about the same total columns cut from the same tracks, two-launch path
                                                (fsst_canon_kernel: the canonical band's kernel, ragged or not), in a child process;
                                                beside it the general kernel on that batch (HSSFSST_NO_CANON=1)
    python tools/ragged_bench.py --trace        only the ragged call and the dense batch, for
                                                `rocprofv3 --kernel-trace --stats -- python ...` in a run of its own
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import FSST, synth  # noqa: E402
from heart_sounds_segmentation_amd.corpus import CorpusBuilder  # noqa: E402

DEV = "cuda:0"


def tracks(seed=2016):
    return synth.pcg_windows(16, n=120000, seed=seed)      # PCG-like tracks; recordings are seeded slices of them


def corpus(n_rec, seed=2016):
    rng = np.random.default_rng(seed)
    lens = rng.integers(20000, 60000, size=n_rec)
    tr = tracks(seed)
    offs = rng.integers(0, 120000 - 60000, size=n_rec)
    return [torch.from_numpy(np.ascontiguousarray(tr[i % 16, o:o + T])) for i, (o, T) in enumerate(zip(offs, lens))]


def dense_batch(total_cols, n, seed=2016):
    """B x n signals (B = total_cols / n rounded) cut from the same tracks as the corpus, at seeded offsets."""
    rng = np.random.default_rng(seed + 1)
    B = max(1, round(total_cols / n))
    tr = tracks(seed)
    offs = rng.integers(0, 120000 - n, size=B)
    return torch.from_numpy(np.stack([tr[i % 16, o:o + n] for i, o in enumerate(offs)])).to(DEV)


def tf_canon():
    return FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True, device=DEV)


def events_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(DEV)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def core_ms(tf, fn, reps):
    """(core kernel ms, rest ms) per call from the plan's timing events."""
    fn()
    torch.cuda.synchronize(DEV)
    tf.set_timing(True)
    for _ in range(reps):
        fn()
    core, rest, n = tf.timing()
    tf.set_timing(False)
    return core / n, rest / n


def dense_child(total_cols, n):
    """Core time of a dense batch of about total_cols columns (B x n), two-launch path: JSON on stdout."""
    tf = tf_canon()
    X = dense_batch(total_cols, n)
    B = int(X.shape[0])
    tf.set_zpath("two_launch")
    c, r = core_ms(tf, lambda: tf.batch(X), 10)
    tf.batch(X)
    print(json.dumps({"B": B, "n": n, "cols": B * n, "core_ms": c, "zscore_ms": r, "kernel": tf.last_kernel()}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=792)
    ap.add_argument("--out")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--dense-child", nargs=2, type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.dense_child:
        dense_child(*args.dense_child)
        return
    xs = corpus(args.recordings)
    lens = [int(x.shape[0]) for x in xs]
    total = sum(lens)
    tf = tf_canon()
    xs_d = [x.to(DEV) for x in xs]
    if args.trace:
        for _ in range(3):
            tf.ragged(xs_d)
        X = dense_batch(total, 40000)
        tf.set_zpath("two_launch")
        for _ in range(3):
            tf.batch(X)
        torch.cuda.synchronize(DEV)
        print(json.dumps({"trace": True, "recordings": len(xs), "cols": total}))
        return
    res = {"recordings": len(xs), "total_cols": total, "len_min": min(lens), "len_max": max(lens),
           "len_mean": total / len(xs), "band": [25, 200], "nwin": 128, "mode": "stack"}
    # (a) device-resident
    out = tf.ragged(xs_d)
    res["ragged_kernel"] = tf.last_kernel()
    ok = all(torch.equal(out[i], tf.batch(xs_d[i][None])[0]) for i in range(0, len(xs), 97))
    res["spot_check_bit_identical"] = bool(ok)
    loop_ms = events_ms(lambda: [tf.batch(x[None]) for x in xs_d], 3)
    rag_ms = events_ms(lambda: tf.ragged(xs_d), 10)
    res["device_loop_ms"] = loop_ms
    res["device_ragged_ms"] = rag_ms
    res["device_speedup"] = loop_ms / rag_ms
    # (b) host-fed
    for x in xs[:50]:
        tf(x)
    t0 = time.perf_counter()
    for x in xs:
        tf(x)
    res["host_loop_ms"] = (time.perf_counter() - t0) * 1e3
    cb = CorpusBuilder(tf, device=DEV)
    recs = [(x, None) for x in xs]
    cb.build_recordings(recs)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        cb.build_recordings(recs)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["host_build_recordings_ms"] = min(ts)
    res["host_speedup"] = res["host_loop_ms"] / res["host_build_recordings_ms"]
    tf.ragged(xs)                                        # (allocates the pinned staging)
    t0 = time.perf_counter()
    tf.ragged(xs)
    res["host_ragged_ms"] = (time.perf_counter() - t0) * 1e3     # host list in, pageable host arena out
    # (c) core kernel: ragged against a dense batch of the same total columns
    c, r = core_ms(tf, lambda: tf.ragged(xs_d), 10)
    res["ragged_core_ms"], res["ragged_zscore_ms"] = c, r
    res["ragged_core_Mcols_per_s"] = total / c / 1e3
    for key, e in (("dense_same_kernel", dict(os.environ)), ("dense_general_kernel", dict(os.environ, HSSFSST_NO_CANON="1"))):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--dense-child", str(total), "40000"], env=e,
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            res[key] = {"error": p.stderr[-2000:]}
            continue
        d = json.loads(p.stdout.strip().splitlines()[-1])
        d["Mcols_per_s"] = d["cols"] / d["core_ms"] / 1e3
        res[key] = d
    if "Mcols_per_s" in res["dense_same_kernel"]:
        res["ragged_core_vs_dense_same_kernel"] = res["ragged_core_Mcols_per_s"] / res["dense_same_kernel"]["Mcols_per_s"]
    tf.check()
    s = json.dumps(res)
    print(s)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
