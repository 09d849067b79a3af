"""Timing of ragged resampling (Resample.ragged / hssfsst_resample_exec_ragged, corpus.build_resampled_recordings) on a seeded
stand-in corpus: 792 synth.recording()s of lengths uniform in [20 000, 60 000] samples with label tracks, num = 2 000 and 20 000.

    python tools/resample_ragged_bench.py [--out-dir DIR]
        (a) device-resident: one Resample.ragged(list) call (HIP events after a warm-up call);
        (b) the per-recording loop a user has without it: Resample(num, device=...).batch(x[None]) for every recording, once
            with fresh plans (a new Resample: one host table build per length) and once with every plan cached (HIP events);
        (c) host-fed: build_resampled_recordings, device-kept and host-returned (wall clock, best of 3, builder reused), against
            the per-recording loop (tf(rs(x)), round(rs(y)) - 1) with rs = Resample(num, device=...), plans cached;
        writes DIR/resample_ragged_bench.json and .txt (default: profiles/).
    python tools/resample_ragged_bench.py --trace
        three ragged calls per num only, for `rocprofv3 --kernel-trace --stats -- python ...` in a run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from heart_sounds_segmentation_amd import synth  # noqa: E402
from heart_sounds_segmentation_amd.corpus import CorpusBuilder  # noqa: E402
from heart_sounds_segmentation_amd.transforms import FSST, Resample  # noqa: E402

DEV = "cuda:0"
NUMS = (2000, 20000)


def corpus(n_rec=792, seed=2016):
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.integers(20000, 60001, size=n_rec)]
    recs = []
    for i, T in enumerate(lens):
        x = torch.from_numpy(synth.recording(T, seed=seed + i))
        y = np.empty(T, dtype=np.int64)
        pos, state = 0, int(rng.integers(1, 5))
        while pos < T:
            run = int(rng.integers(50, 400))
            y[pos:pos + run] = state
            pos += run
            state = state % 4 + 1
        recs.append((x, torch.from_numpy(y)))
    return recs


def events_ms(fn, reps=1, warmup=1):
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


def wall_ms(fn, reps=3):
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(DEV)
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    recs = corpus()
    xs = [x for x, _ in recs]
    xd = [x.to(DEV) for x in xs]
    lens = [int(x.shape[0]) for x in xs]
    if args.trace:
        for num in NUMS:
            rs = Resample(num)
            for _ in range(3):
                rs.ragged(xd)
        torch.cuda.synchronize(DEV)
        return
    res = {"recordings": len(xs), "samples": int(sum(lens)), "len_min": min(lens), "len_max": max(lens),
           "distinct_lengths": len(set(lens)), "device": torch.cuda.get_device_name(0), "nums": {}}
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True, device=DEV)
    for num in NUMS:
        r = {}
        rs = Resample(num)
        r["a_ragged_ms"] = events_ms(lambda: rs.ragged(xd), reps=5)
        # spot check: the ragged rows against the dense plan of their length
        full = rs.ragged(xd, dtype=torch.float64)
        # (b) the per-recording loop: fresh plans (a new Resample), then every plan cached
        loop = Resample(num, device=DEV)
        r["b_loop_fresh_ms"] = events_ms(lambda: [loop.batch(x[None]) for x in xd], reps=1, warmup=0)
        r["b_loop_cached_ms"] = events_ms(lambda: [loop.batch(x[None]) for x in xd], reps=3)
        r["dense_plans_cached"] = len(loop._plans)
        err = 0.0
        for i in range(0, len(xd), 97):
            d = loop.batch(xd[i][None].double(), torch.float64)[0]
            err = max(err, float((full[i] - d).abs().max() / max(float(d.abs().max()), 1.0)))
        r["spot_rel_err_vs_dense"] = err
        r["a_vs_fresh"] = r["b_loop_fresh_ms"] / r["a_ragged_ms"]
        r["a_vs_cached"] = r["b_loop_cached_ms"] / r["a_ragged_ms"]
        # (c) host-fed: the builder against the lazy dataset's per-recording loop (device Resample, plans cached above)
        b = CorpusBuilder(tf, device=DEV, resample=rs)
        r["c_builder_device_kept_ms"] = wall_ms(lambda: b.build_resampled_recordings(recs, keep_on_device=True))
        r["c_builder_host_returned_ms"] = wall_ms(lambda: b.build_resampled_recordings(recs))

        def lazy_loop():
            for x, y in recs:
                tf(loop(x))
                torch.round(loop(y)).type(torch.int64) - 1
        r["c_loop_ms"] = wall_ms(lazy_loop, reps=1)
        r["c_host_returned_speedup"] = r["c_loop_ms"] / r["c_builder_host_returned_ms"]
        res["nums"][str(num)] = r
        del loop, full
        torch.cuda.empty_cache()
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "resample_ragged_bench.json"), "w") as fh:
        json.dump(res, fh)
    lines = [f"tools/resample_ragged_bench.py on one {res['device']}: Resample.ragged / hssfsst_resample_exec_ragged",
             f"{res['recordings']} synth.recording()s with label tracks, seeded lengths {res['len_min']}..{res['len_max']} samples "
             f"({res['distinct_lengths']} distinct), {res['samples']} samples in all.  Raw numbers: profiles/resample_ragged_bench.json.", ""]
    for num, r in res["nums"].items():
        a20 = "" if num != "20000" else f"   (target <= 40 ms: {'met' if r['a_ragged_ms'] <= 40 else 'NOT met'})"
        lines += [f"num = {num}",
                  "(a) device-resident, HIP events",
                  f"    one Resample.ragged(list)                    {r['a_ragged_ms']:9.2f} ms{a20}",
                  "(b) the per-recording loop Resample(num, device=...).batch(x[None]), HIP events",
                  f"    fresh plans (a new Resample)                 {r['b_loop_fresh_ms']:9.1f} ms   ({r['dense_plans_cached']} host table builds)",
                  f"    every plan cached                            {r['b_loop_cached_ms']:9.2f} ms",
                  f"    (a) faster than fresh / cached               {r['a_vs_fresh']:7.1f} x / {r['a_vs_cached']:.2f} x   "
                  f"(targets >= 50 x: {'met' if r['a_vs_fresh'] >= 50 else 'NOT met'}, >= 2 x: {'met' if r['a_vs_cached'] >= 2 else 'NOT met'})",
                  f"    every 97th row against its dense plan        {r['spot_rel_err_vs_dense']:.1e} relative",
                  "(c) host-fed, wall clock, FSST STACK Kaiser(128, 0.5) [25, 200] Hz, labels included",
                  f"    build_resampled_recordings, device-kept      {r['c_builder_device_kept_ms']:9.1f} ms   (best of 3, builder reused)",
                  f"    build_resampled_recordings, host-returned    {r['c_builder_host_returned_ms']:9.1f} ms",
                  f"    loop (tf(rs(x)), round(rs(y)) - 1), cached   {r['c_loop_ms']:9.1f} ms",
                  f"    host-returned speed-up                       {r['c_host_returned_speedup']:7.1f} x", ""]
    with open(os.path.join(args.out_dir, "resample_ragged_bench.txt"), "w") as fh:
        fh.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
