#!/usr/bin/env python3
"""The BiLSTM segmenter as HIP kernels against stock nn.LSTM (MIOpen), interleaved in one process, at BASELINE config C4
(50 windows x 2000 samples -> FSST -> BiLSTM(44 -> 2 x 240 -> 2 x 240 -> 4)), and the B = 1, T = 35 500 recording.

  segmenter_bench.py [--out FILE] [--kernel-stats CSV]   timings (warm-up / repeat scheme of configs_bench.py, three rounds, the two
                                                        paths alternating); --kernel-stats folds in the kernel_stats CSV of a
                                                        separate `rocprofv3 --kernel-trace --stats -- segmenter_bench.py --trace` run
  segmenter_bench.py --trace                             only the HIP calls (3 x C4, 1 x recording), for that profiler run
Done means: the HIP path takes at most half of the nn.LSTM time OF THE SAME RUN at C4."""
import argparse, csv, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import FSST, synth
from heart_sounds_segmentation_amd.consumer import SegmenterHead, segment

TRACE_C4, TRACE_REC = 3, 1


def timed(fn, reps, warm=2):
    for _ in range(warm): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--kernel-stats"); ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "segmenter_bench.py needs a GPU"
    tf = FSST(1000, synth.kaiser_window(128, 0.5), truncate_freq=(25, 200), stack=True)
    torch.manual_seed(4)
    head = SegmenterHead(44, 240, 50).cuda().eval()
    hip = head.hip()
    X50 = torch.from_numpy(synth.pcg_windows(50, 2000, seed=9)).cuda()
    rec = torch.from_numpy(synth.pcg_windows(1, 35500, seed=5)).cuda()
    h1, c1 = head.h0[:, :1].contiguous(), head.c0[:, :1].contiguous()
    rec_feats = tf.batch(rec)
    if a.trace:
        for _ in range(TRACE_C4): segment(tf, hip, X50)
        for _ in range(TRACE_REC): hip(rec_feats, h0=h1, c0=c1)
        torch.cuda.synchronize()
        return
    res, lines = {}, []
    with torch.no_grad():
        y_ref, y_hip = segment(tf, head, X50), segment(tf, hip, X50)
        res["C4_max_abs_dlogp_hip_vs_nn_lstm"] = float((y_ref - y_hip).abs().max())
        rounds = []
        for _ in range(3):                                   # the two paths alternate: same clocks, same neighbours
            rounds.append((timed(lambda: segment(tf, head, X50), 20, 3), timed(lambda: segment(tf, hip, X50), 20, 3)))
        t_ref, t_hip = min(r[0] for r in rounds), min(r[1] for r in rounds)
        fonly = timed(lambda: tf.batch(X50), 50, 5)
        res["C4_end_to_end_batch50"] = {"ms": round(t_ref * 1e3, 3), "windows_per_s": round(50 / t_ref, 1), "fsst_only_ms": round(fonly * 1e3, 4)}
        res["C4_end_to_end_batch50_hip_segmenter"] = {"ms": round(t_hip * 1e3, 3), "windows_per_s": round(50 / t_hip, 1),
                                                      "ratio_to_nn_lstm": round(t_hip / t_ref, 4)}
        res["C4_rounds_ms"] = [[round(r[0] * 1e3, 3), round(r[1] * 1e3, 3)] for r in rounds]
        head1 = SegmenterHead(44, 240, 1, h0=h1, c0=c1).cuda().eval()
        head1.load_state_dict(head.state_dict())
        r_ref = min(timed(lambda: head1(rec_feats), 3, 1) for _ in range(2))
        r_hip = min(timed(lambda: hip(rec_feats, h0=h1, c0=c1), 3, 1) for _ in range(2))
        res["recording_35500_batch1"] = {"nn_lstm_ms": round(r_ref * 1e3, 3), "hip_ms": round(r_hip * 1e3, 3),
                                         "max_abs_dlogp": float((head1(rec_feats) - hip(rec_feats, h0=h1, c0=c1)).abs().max())}
    lines.append(f"C4 (50 x 2000, hidden 240): nn.LSTM {t_ref * 1e3:.2f} ms, HIP segmenter {t_hip * 1e3:.2f} ms "
                 f"(ratio {t_hip / t_ref:.3f}; FSST alone {fonly * 1e3:.3f} ms); max |d log p| between them {res['C4_max_abs_dlogp_hip_vs_nn_lstm']:.2e}")
    lines.append(f"recording (1 x 35500): nn.LSTM {r_ref * 1e3:.2f} ms, HIP segmenter {r_hip * 1e3:.2f} ms")
    if a.kernel_stats:
        ks = {}
        with open(a.kernel_stats) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("KernelName") or ""
                if "seg_" in name:
                    ks[name.split("(")[0].split("::")[-1]] = {"calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3}
        res["kernel_trace"] = ks
        rec_k = next((v for k, v in ks.items() if "seg_rec" in k), None)
        if rec_k:
            steps = 2 * (TRACE_C4 * 2000 + TRACE_REC * 35500)         # two layers; the two directions share a launch
            tot = sum(v["total_us"] for v in ks.values())
            res["recurrence_us_per_step"] = round(rec_k["total_us"] / steps, 3)
            res["projection_and_head_share"] = round(1.0 - rec_k["total_us"] / tot, 4)
            lines.append(f"kernel trace ({TRACE_C4} x C4 + {TRACE_REC} x recording): " +
                         ", ".join(f"{k} {v['total_us'] / 1e3:.2f} ms / {v['calls']} launches" for k, v in sorted(ks.items())))
            lines.append(f"recurrence: {res['recurrence_us_per_step']} us per step and layer; projection + head + state share of kernel time "
                         f"{100 * res['projection_and_head_share']:.1f} %")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
