"""float32 against float16 against bfloat16 STACK features (FSST(out_dtype=...)), same box, same run, interleaved rounds.

    python tools/half_bench.py [--out FILE] [--kernel-stats CSV]
        C2  FSST.batch of 1024 x 2000-sample windows, device in and out: ms per exec (200 execs queued between two events,
            median of the rounds); with --kernel-stats, the per-kernel averages of a rocprofv3 --kernel-stats CSV of --trace;
        C3  build_features of the C3-shaped stand-in (198 recordings x 35 500 samples = 6 534 windows, a quarter of bench.py's
            corpus, as its host_fed leg) to pinned host memory, arena reused: windows/s;
        C1  the reference's in-memory dataset call with every result kept alive, as bench.py measures it: 80 calls of
            FSST(x_cpu (2000, 1)) kept (the 64 lent pool buffers run dry), then 300 timed calls, all kept: median ms per call,
            the first round (fresh memory, bench.py's case) and the median over rounds (memory the earlier round freed).
    python tools/half_bench.py --trace      only the C2 execs of the three dtypes, for a rocprofv3 --kernel-trace --stats run of its own
Prints one JSON object (and writes it to --out, with a text table beside it)."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import FSST, synth  # noqa: E402
from heart_sounds_segmentation_amd.corpus import CorpusBuilder  # noqa: E402
from heart_sounds_segmentation_amd.framing import frame_starts  # noqa: E402

DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
W = synth.kaiser_window(128, 0.5)


def tf(dt):
    return FSST(1000, W, stack=True, truncate_freq=(25, 200), device=DEV, out_dtype=dt)


def c2(rounds, steps):
    X = torch.from_numpy(synth.pcg_windows(1024, 2000, seed=7)).to(DEV)
    t = {k: tf(dt) for k, dt in DTYPES.items()}
    out = {k: torch.empty((1024, 2000, 44), dtype=dt, device=DEV) for k, dt in DTYPES.items()}
    for k in DTYPES:
        for _ in range(5):
            t[k].batch(X, out=out[k])
    torch.cuda.synchronize()
    ms = {k: [] for k in DTYPES}
    for _ in range(rounds):
        for k in DTYPES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                t[k].batch(X, out=out[k])
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / steps)
    for k in DTYPES:
        t[k].check()
    kern = {k: t[k].last_kernel() for k in DTYPES}
    return {k: {"ms_per_exec": round(statistics.median(v), 4), "rounds": [round(x, 4) for x in v], "kernel": kern[k]} for k, v in ms.items()}


def c3(rounds, nrec=198, T=35500):
    base = [synth.recording(T, seed=synth.SEED + 10 + i) for i in range(8)]
    recs = [(torch.from_numpy(np.roll(base[i % 8], 97 * i)), None) for i in range(nrec)]
    total = nrec * int(frame_starts(T, 1000, 2000)[0].shape[0])
    b = {k: CorpusBuilder(tf(dt), device=DEV) for k, dt in DTYPES.items()}
    arena = {}
    for k in DTYPES:
        arena[k] = b[k].build(recs).features                 # warm-up; allocates the pinned arena once
    res = {k: [] for k in DTYPES}
    for _ in range(rounds):
        for k in DTYPES:
            t0 = time.perf_counter()
            b[k].build(recs, out=arena[k])
            res[k].append(total / (time.perf_counter() - t0))
    return {k: {"windows_per_s": round(statistics.median(v), 1), "rounds": [round(x, 1) for x in v], "windows": total,
                "arena_bytes": arena[k].numel() * arena[k].element_size()} for k, v in res.items()}


def c1(rounds, calls=300):
    """bench.py's "results kept" measurement per dtype and round: 80 calls kept first (the 64 lent pool buffers run dry), then `calls`
    timed calls, every result kept alive -- each a copy into a fresh tensor.  The first round of each dtype meets memory the process has
    never used (page faults on every fresh 352 / 176 kB tensor, as bench.py's one series does); later rounds reuse what the earlier
    round freed."""
    X = torch.from_numpy(synth.pcg_windows(calls + 80, 2000, seed=9)).reshape(calls + 80, 2000, 1)
    t = {k: tf(dt) for k, dt in DTYPES.items()}
    for k in DTYPES:
        for i in range(20):
            t[k](X[i])
    per = {k: [] for k in DTYPES}
    for _ in range(rounds):
        for k in DTYPES:
            kept = [t[k](X[i]) for i in range(80)]
            dts = []
            for i in range(80, 80 + calls):
                t0 = time.perf_counter()
                kept.append(t[k](X[i]))
                dts.append((time.perf_counter() - t0) * 1e3)
            per[k].append(statistics.median(dts))
            del kept
    return {k: {"ms_per_call_median": round(statistics.median(v), 4), "first_round_ms": round(v[0], 4), "rounds": [round(x, 4) for x in v],
                "calls_per_round": calls} for k, v in per.items()}


def kernel_stats(path):
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            rows[r["Name"]] = {"calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.trace:
        c2(1, 20)
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(0), "c2": c2(a.rounds, 200), "c3_host_returned": c3(a.rounds), "c1_kept": c1(a.rounds)}
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        res["c2_kernel_stats"] = kernel_stats(a.kernel_stats)
    f = res["c2"]["f32"]["ms_per_exec"], res["c3_host_returned"]["f32"]["windows_per_s"], res["c1_kept"]["f32"]["ms_per_call_median"]
    lines = [f"{'':5s} {'C2 ms/exec':>11s} {'x f32':>6s} {'C3 host windows/s':>18s} {'x f32':>6s} {'C1 kept ms/call':>16s} {'1st round':>9s}"]
    for k in DTYPES:
        c2k, c3k, c1k = res["c2"][k], res["c3_host_returned"][k], res["c1_kept"][k]
        lines.append(f"{k:5s} {c2k['ms_per_exec']:11.4f} {c2k['ms_per_exec'] / f[0]:6.3f} {c3k['windows_per_s']:18.1f} {c3k['windows_per_s'] / f[1]:6.3f} "
                     f"{c1k['ms_per_call_median']:16.4f} {c1k['first_round_ms']:9.4f}")
    if "c2_kernel_stats" in res:
        lines.append("C2 kernels (rocprofv3 --kernel-trace --stats of --trace):")
        for name, v in sorted(res["c2_kernel_stats"].items(), key=lambda kv: -kv[1]["total_ms"]):
            lines.append(f"  {v['avg_us']:10.2f} us x {v['calls']:5d}  {name[:150]}")
    text = "\n".join(lines)
    print(json.dumps(res))
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh)
        with open(os.path.splitext(a.out)[0] + ".txt", "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
