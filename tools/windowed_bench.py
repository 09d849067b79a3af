#!/usr/bin/env python3
"""Window-by-window segmentation of whole recordings (consumer.segment_windowed: FSST.frames, the BiLSTM on dense batches of
windows, hssfsst_stitch_windows) measured next to the one-recurrence path (consumer.segment_recordings), and the stitch alone next
to a torch restatement on the device, interleaved in one process:

  windowed_bench.py [--out FILE] [--recordings 792] [--rounds 3] [--case all|single|corpus|stitch] [--max-windows 1024]

  (a) single   one 35 500-sample recording: segment_windowed against segment_recordings;
  (b) corpus   --recordings recordings of 20 000 - 60 000 samples: the same pair;
  (c) stitch   the stitch alone on the window log-probs of that list (random log-softmax rows: no segmenter), mode "prob" under
               triangular weights, against the same pooling from torch ops on the same arena: exp in float64, index_add_ of the
               weighted probabilities and of the weights per output step, log, log_softmax, a copy for the steps one window
               covers.  The row-to-step index of the torch way is made once, outside the timing.  The two results are held to the
               gates of tests/test_stitch_windows.py: copied rows equal, pooled rows within one float32 ulp.
The model is the reference's (hidden 240, 44 features, seeded); the canonical FSST.  Every way runs once per round, the rounds
alternate, allocation included; the best round of each is reported.  Nothing here is gated on time."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import FSST, _lib, synth
from heart_sounds_segmentation_amd.consumer import SegmenterHead, segment_recordings, segment_windowed
from heart_sounds_segmentation_amd.framing import cover_starts
from heart_sounds_segmentation_amd.sequence import stitch_windows, window_weights

N, STRIDE = 2000, 1000


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(); return time.perf_counter() - t0, out


def rounds_of(ways, rounds):
    for fn in ways.values():                             # (warms the kernels and the plans)
        fn()
    times = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            times[k].append(timed(fn)[0])
    return times


def segment_case(name, lens, a, res, lines, tf, seg):
    recs = [torch.from_numpy(synth.recording(T, seed=500 + i)).cuda() for i, T in enumerate(lens)]
    windows = sum(len(cover_starts(T, STRIDE, N)[0]) for T in lens)
    ways = {"windowed": lambda: segment_windowed(tf, seg, recs, stride=STRIDE, n=N, max_windows=a.max_windows),
            "one_recurrence": lambda: segment_recordings(tf, seg, recs)}
    times = rounds_of(ways, a.rounds)
    best = {k: min(v) * 1e3 for k, v in times.items()}
    w, o = ways["windowed"]().data, ways["one_recurrence"]().data
    agree = float((w.argmax(dim=1) == o.argmax(dim=1)).double().mean())
    res[name] = {"recordings": len(lens), "samples": sum(lens), "windows": windows, "max_windows": a.max_windows,
                 "argmax_agreement_with_one_recurrence": round(agree, 4),
                 **{k + "_ms": round(v, 3) for k, v in best.items()}, **{k + "_rounds_ms": [round(x * 1e3, 3) for x in v] for k, v in times.items()}}
    lines.append(f"{name}: {len(lens)} recordings, {sum(lens)} samples, {windows} windows of {N} at stride {STRIDE}: segment_windowed "
                 f"{best['windowed']:.1f} ms, segment_recordings {best['one_recurrence']:.1f} ms, windowed / one recurrence = "
                 f"{best['windowed'] / best['one_recurrence']:.3f}; rounds of windowed {', '.join(f'{v * 1e3:.1f}' for v in times['windowed'])}; "
                 f"the two argmaxes agree on {100 * agree:.1f} % of the steps (an untrained head; they differ by design)")


def torch_stitch(win, dst, wrow, cover, total):
    """mode "prob" from torch ops: (total, 4) float32.  dst (rows,) the output step of every window row, wrow (rows,) its weight,
    cover (total,) the covering windows of every step."""
    acc = torch.zeros((total, 4), dtype=torch.float64, device=win.device).index_add_(0, dst, torch.exp(win.double()) * wrow[:, None])
    wsum = torch.zeros((total,), dtype=torch.float64, device=win.device).index_add_(0, dst, wrow)
    out = torch.log_softmax(torch.log(acc / wsum[:, None]), dim=1).float()
    one = cover == 1
    copied = torch.zeros((total, 4), dtype=torch.float32, device=win.device).index_add_(0, dst, win)    # (one row where cover == 1)
    return torch.where(one[:, None], copied, out)


def stitch_case(lens, a, res, lines):
    total = sum(lens)
    first, dst, pos, row = [], [], [], 0
    at = np.concatenate([[0], np.cumsum(lens)])
    for i, T in enumerate(lens):
        first.append(row)
        for s, ln in zip(*cover_starts(T, STRIDE, N)):
            dst.append(np.arange(s, s + ln) + at[i]); pos.append(np.arange(ln)); row += int(ln)
    gen = torch.Generator(device="cuda").manual_seed(5)
    win = torch.log_softmax(3.0 * torch.randn(row, 4, device="cuda", generator=gen), dim=1)
    w = window_weights(N, "triangular", "cuda")
    dst = torch.from_numpy(np.concatenate(dst)).cuda()
    wrow = w.double()[torch.from_numpy(np.concatenate(pos)).cuda()]
    cover = torch.bincount(dst, minlength=total)
    ways = {"stitch": lambda: stitch_windows(win, first, lens, N, STRIDE, weights=w, mode="prob"),
            "stitch_with_dissent": lambda: stitch_windows(win, first, lens, N, STRIDE, weights=w, mode="prob", return_dissent=True),
            "stitch_select": lambda: stitch_windows(win, first, lens, N, STRIDE, weights=w, mode="select"),
            "torch": lambda: torch_stitch(win, dst, wrow, cover, total)}
    times = rounds_of(ways, a.rounds)
    best = {k: min(v) * 1e3 for k, v in times.items()}
    got, ref = ways["stitch"]().data, ways["torch"]()
    one = cover == 1
    copied_equal = bool(torch.equal(got[one], ref[one]))
    ulp = torch.from_numpy(np.spacing(np.abs(ref[~one].cpu().numpy()))).cuda()
    over = int(((got[~one] - ref[~one]).abs() > ulp).sum())
    res["stitch"] = {"recordings": len(lens), "steps": total, "window_rows": row, "bytes_per_step": round((16 * row + 16 * total) / total, 1),
                     "copied_rows_equal_torch": copied_equal, "pooled_values_over_one_ulp_from_torch": over, "pooled_values": int((~one).sum()) * 4,
                     **{k + "_ms": round(v, 3) for k, v in best.items()}, **{k + "_rounds_ms": [round(x * 1e3, 3) for x in v] for k, v in times.items()}}
    gbs = (16 * row + 16 * total) / best["stitch"] / 1e6
    lines.append(f"the stitch alone: {len(lens)} recordings, {total} steps from {row} window rows ({res['stitch']['bytes_per_step']} bytes per step read and "
                 f"written): \"prob\" {best['stitch']:.3f} ms ({gbs:.0f} GB/s of those bytes), with dissent {best['stitch_with_dissent']:.3f} ms, "
                 f"\"select\" {best['stitch_select']:.3f} ms; torch on the device {best['torch']:.3f} ms; this call / torch = "
                 f"{best['stitch'] / best['torch']:.2f}; copied rows {'equal' if copied_equal else 'DIFFER FROM'} torch's, {over} of "
                 f"{res['stitch']['pooled_values']} pooled values farther than one float32 ulp from torch's")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--recordings", type=int, default=792); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-windows", type=int, default=1024); ap.add_argument("--case", default="all", choices=("all", "single", "corpus", "stitch"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "windowed_bench.py needs a GPU"
    res, lines = {"kernels": {}}, []
    for k, facts in sorted(_lib.kernel_resources("seg_stitch_").items()):
        res["kernels"][k] = facts
        lines.append(f"{k}: {facts['vgpr_count']} VGPRs, {facts['agpr_count']} AGPRs, {facts['group_segment_fixed_size']} bytes of LDS, "
                     f"{facts['private_segment_fixed_size']} bytes of scratch")
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True)
    seg = SegmenterHead.seeded_like_reference(7, batch_size=1).eval().hip() if a.case != "stitch" else None
    lens = [int(v) for v in np.random.default_rng(8).integers(20000, 60000, size=a.recordings)]
    if a.case in ("all", "single"):
        segment_case("one recording", [35500], a, res, lines, tf, seg)
    if a.case in ("all", "corpus"):
        segment_case("corpus list", lens, a, res, lines, tf, seg)
    if a.case in ("all", "stitch"):
        stitch_case(lens, a, res, lines)
    lines.append("the expectations this was planned with, unmeasured: (a) from the README's 552 ms for one 35 500-step recording and 36 ms "
                 "for 50 windows of 2000 steps, the 35 windows of that recording take a small fraction of the one-recurrence time; "
                 "(c) at about 50 bytes per output step at stride n / 2 the stitch is a small fraction of the window pass.  The lines "
                 "above are the measurement.")
    print("\n".join(lines)); print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
