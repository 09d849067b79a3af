#!/usr/bin/env python3
"""One training step of the BiLSTM segmenter on the HIP layers (HipSegmenterHead) against stock nn.LSTM (SegmenterHead, MIOpen),
interleaved in one process after warm-up, both with dropout active, at the C4 shape: B 50, T 2000, F 44, H 240.
A step is forward, nll_loss, backward, clip_grad_norm_(1) and Adam.

  segmenter_train_bench.py [--out FILE] [--kernel-stats CSV]   timings (three rounds, the two modules alternating); --kernel-stats
                                                              folds in the kernel_stats CSV of a separate
                                                              `rocprofv3 --kernel-trace --stats -- segmenter_train_bench.py --trace` run
  segmenter_train_bench.py --trace                             only HIP training steps, for that profiler run
There is no speed gate: the stock step is the yardstick and the numbers are reported as measured."""
import argparse, csv, json, os, sys, time
import torch
from torch import nn
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd.consumer import HipSegmenterHead, SegmenterHead

B, T, F, H = 50, 2000, 44, 240
TRACE_STEPS = 3


def make(cls, state=None):
    torch.manual_seed(4)
    m = cls(F, H, B)
    if state is not None:
        m.load_state_dict(state)
    m = m.cuda().train()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3)


def step(m, opt, x, y):
    opt.zero_grad(set_to_none=True)
    loss = nn.functional.nll_loss(m(x).reshape(-1, 4), y.reshape(-1))
    loss.backward()
    nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()
    return loss


def timed(fn, reps, warm):
    for _ in range(warm): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--kernel-stats"); ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "segmenter_train_bench.py needs a GPU"
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, T, F, generator=g).cuda()
    y = torch.randint(0, 4, (B, T), generator=g).cuda()
    hip, hip_opt = make(HipSegmenterHead)
    if a.trace:
        for _ in range(TRACE_STEPS): step(hip, hip_opt, x, y)
        torch.cuda.synchronize()
        return
    ref, ref_opt = make(SegmenterHead, hip.state_dict())
    res, lines = {"shape": {"B": B, "T": T, "F": F, "H": H}}, []
    rounds = []
    for r in range(3):                                           # the two modules alternate: same clocks, same neighbours
        rounds.append((timed(lambda: step(ref, ref_opt, x, y), a.reps, 2 if r == 0 else 1),
                       timed(lambda: step(hip, hip_opt, x, y), a.reps, 2 if r == 0 else 1)))
    t_ref, t_hip = min(r[0] for r in rounds), min(r[1] for r in rounds)
    fwd_ref = timed(lambda: ref(x), a.reps, 1)
    fwd_hip = timed(lambda: hip(x), a.reps, 1)
    res["train_step_ms"] = {"nn_lstm": round(t_ref * 1e3, 2), "hip": round(t_hip * 1e3, 2), "ratio_hip_to_nn_lstm": round(t_hip / t_ref, 4)}
    res["forward_in_train_mode_ms"] = {"nn_lstm": round(fwd_ref * 1e3, 2), "hip": round(fwd_hip * 1e3, 2)}
    res["rounds_ms"] = [[round(r[0] * 1e3, 2), round(r[1] * 1e3, 2)] for r in rounds]
    res["peak_memory_gb"] = round(torch.cuda.max_memory_allocated() / 1e9, 2)
    res["loss_after"] = {"nn_lstm": float(step(ref, ref_opt, x, y).detach()), "hip": float(step(hip, hip_opt, x, y).detach())}
    lines.append(f"training step at B {B}, T {T}, F {F}, H {H}, dropout active: nn.LSTM {t_ref * 1e3:.1f} ms, HipSegmenterHead {t_hip * 1e3:.1f} ms "
                 f"(ratio {t_hip / t_ref:.3f}); forward alone {fwd_ref * 1e3:.1f} / {fwd_hip * 1e3:.1f} ms; peak memory {res['peak_memory_gb']} GB")
    if a.kernel_stats:
        ks = {}
        with open(a.kernel_stats) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name") or row.get("KernelName") or ""
                if "seg_" in name:
                    ks[name.split("(")[0].split("::")[-1]] = {"calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3}
        res["kernel_trace"] = ks
        steps = 2 * TRACE_STEPS * T                                   # two layers; the two directions share a launch
        for key, label in (("seg_bwd_rec", "backward_recurrence_us_per_step"), ("seg_rec", "forward_recurrence_us_per_step")):
            k = next((v for n, v in ks.items() if n.startswith(key)), None)
            if k:
                res[label] = round(k["total_us"] / steps, 3)
        lines.append(f"kernel trace ({TRACE_STEPS} HIP steps): " +
                     ", ".join(f"{k} {v['total_us'] / 1e3:.2f} ms / {v['calls']} launches" for k, v in sorted(ks.items())))
        lines.append(f"recurrences per step and layer: forward {res.get('forward_recurrence_us_per_step')} us, "
                     f"backward {res.get('backward_recurrence_us_per_step')} us")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
