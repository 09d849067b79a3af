"""Timing of the device resampler (Resample(device=...), Resample.batch, CorpusBuilder(resample=...)).

    python tools/resample_bench.py [--out FILE]      (a) one CPU 2000-sample frame -> 1000 through Resample(1000, device=...),
                                                      host path beside it, host-visible ms per call; (b) Resample.batch on
                                                      1024 frames 2000 -> 1000 (device events); (c) single recordings
                                                      35 500 -> 17 750 and 240 000 -> 120 000 (device events); (d) CorpusBuilder
                                                      on the C3-shaped corpus (792 x 35 500 samples) with and without resample=
    python tools/resample_bench.py --trace            only (b) and (c), for `rocprofv3 --kernel-trace --stats -- python ...`
                                                      in a run of its own (kernel time without the profiler's host cost)
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import FSST, synth  # noqa: E402
from heart_sounds_segmentation_amd.corpus import CorpusBuilder  # noqa: E402
from heart_sounds_segmentation_amd.transforms import Resample  # noqa: E402

DEV = "cuda:0"


def events_ms(fn, reps, warmup):
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


def host_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3 / reps


def fft_flops(n, num, B):
    """Radix-2 butterfly work of the two Bluestein convolutions (4 FFTs of M1 / M2 points: 5 M log2 M flops each)."""
    m1 = 1 << int(np.ceil(np.log2(2 * n - 1)))
    m2 = 1 << int(np.ceil(np.log2(2 * num - 1)))
    return B * 2 * 5 * (m1 * np.log2(m1) + m2 * np.log2(m2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    rec = torch.from_numpy(synth.recording(35500, seed=9))
    X = torch.from_numpy(synth.pcg_windows(1024, 2000, seed=4)).to(DEV)
    t = Resample(1000)
    yb = torch.empty((1024, 1000), dtype=torch.float32, device=DEV)
    long = {T: torch.from_numpy(synth.recording(T, seed=T)).reshape(1, T).to(DEV) for T in (35500, 240000)}
    outs = {T: torch.empty((1, T // 2), dtype=torch.float32, device=DEV) for T in long}
    if args.trace:
        for _ in range(50):
            t.batch(X, out=yb)
        for T in long:
            for _ in range(20):
                Resample(T // 2).batch(long[T], out=outs[T])
        torch.cuda.synchronize(DEV)
        print(json.dumps({"trace": "done"}))
        return
    # (a) the dataset's call shape: one CPU frame, CPU result
    fr = rec[:2000].clone()
    td, th = Resample(1000, device=DEV), Resample(1000)
    res["a_device_call_ms"] = host_ms(lambda: td(fr), 2000, 200)
    res["a_host_call_ms"] = host_ms(lambda: th(fr), 200, 20)
    # (b) 1024 frames 2000 -> 1000 on the device
    res["b_batch1024_ms"] = events_ms(lambda: t.batch(X, out=yb), 200, 20)
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True, device=DEV)
    res["b_fsst_of_resampled_ms"] = events_ms(lambda: tf.batch(yb), 200, 20)
    res["b_fp64_gflop"] = fft_flops(2000, 1000, 1024) / 1e9
    res["b_gflops_achieved"] = res["b_fp64_gflop"] / (res["b_batch1024_ms"] * 1e-3)
    # (c) whole recordings
    for T in long:
        r = Resample(T // 2)
        res[f"c_{T}_to_{T // 2}_ms"] = events_ms(lambda: r.batch(long[T], out=outs[T]), 50, 5)
        res[f"c_{T}_host_ms"] = host_ms(lambda: Resample(T // 2)(long[T][0].cpu()), 3, 1)
        res[f"c_{T}_hbm_bytes_per_pass"] = 2 * 16 * (1 << int(np.ceil(np.log2(2 * T - 1))))
    # (d) the C3-shaped corpus: 792 recordings of 35 500 samples, device-kept features
    base = [synth.recording(35500, seed=synth.SEED + 10 + i) for i in range(8)]
    recs = [(torch.from_numpy(np.roll(base[i % 8], 97 * i)), None) for i in range(792)]
    for tag, rs in (("plain", None), ("resample1000", Resample(1000))):
        b = CorpusBuilder(tf, device=DEV, resample=rs)
        b.build(recs[:64], keep_on_device=True)
        items = b.build(recs, keep_on_device=True)
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            items = b.build(recs, keep_on_device=True)
        torch.cuda.synchronize(DEV)
        ms = (time.perf_counter() - t0) * 1e3 / reps
        res[f"d_corpus_{tag}_ms"] = ms
        res[f"d_corpus_{tag}_windows"] = int(items.features.shape[0])
        res[f"d_corpus_{tag}_item_shape"] = list(items.features.shape[1:])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
