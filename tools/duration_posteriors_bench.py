#!/usr/bin/env python3
"""duration_posteriors and duration_nll (the explicit-duration forward-backward on the device, one call per list) measured next
to what surrounds them, interleaved in one process:

  duration_posteriors_bench.py [--out FILE] [--recordings 792] [--rounds 3] [--prefix 192]

  1. consumer.duration_posteriors on the whole input (workspace allocation and table upload included);
  2. consumer.duration_nll forward + backward on it (the gradient in the log-probs and in learnable transitions);
  3. consumer.decode_durations, the hard decision under the same tables, on the same input;
  4. a torch per-step log-space forward-backward loop on the device (float64, batched over the recordings, a logsumexp over the
     durations per step), run on the first --prefix steps only, taken as a recording of their own, and SCALED to the longest
     recording's steps -- the loop's cost is launches per step, so it is linear;
on the corpus-shaped list (--recordings recordings of 20 000 - 60 000 steps) at D = 512 and D = 2048 and on one recording of
240 000 steps at D = 512, which one workgroup on one CU walks alone: its time over its steps is the per-step cost of a workgroup.
The log-probs are the log-softmax of seeded noise and the tables are Gaussian: the kernel's time does not depend on the values.
Every way runs once per round, the rounds alternate; the best round of each is reported.  Nothing here is gated."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import _lib
from heart_sounds_segmentation_amd.consumer import (cyclic_transitions, decode_durations, duration_nll, duration_posteriors, edge_durations,
                                                    gaussian_durations)
from heart_sounds_segmentation_amd.transforms import RaggedFeatures


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(); return time.perf_counter() - t0, out


def torch_loop(e, A, pi, dur, edge):
    """e (B, P, 4) on the device -> (B, P, 4) posteriors: the log-space recurrences of the duration model as torch ops."""
    e, A, pi, dur, edge = (v.double() for v in (e, A, pi, dur, edge))
    B, T, D = e.shape[0], e.shape[1], dur.shape[1]
    ninf = float("-inf")
    A = A.masked_fill(torch.eye(4, dtype=torch.bool, device=A.device), ninf)
    E = torch.cat([torch.zeros((B, 1, 4), dtype=e.dtype, device=e.device), torch.cumsum(e, dim=1)], dim=1)

    def table(m, first_is_end, all_end):                 # (m, 1, 4): rows d = 1 .. m
        L = edge[:, :m] if all_end else (torch.cat([dur[:, :m - 1], edge[:, m - 1:m]], dim=1) if first_is_end else dur[:, :m])
        return L.T[:, None, :]
    b, c = [pi[None].expand(B, 4)], [None]
    for t in range(1, T + 1):
        m = min(D, t)
        c.append(torch.logsumexp(torch.stack(b[t - m:t]).flip(0) + table(m, m == t, t == T), dim=0))
        if t < T:
            b.append(torch.logsumexp((c[t] + E[:, t])[:, :, None] + A[None], dim=1) - E[:, t])
    logz = torch.logsumexp(c[T] + E[:, T], dim=1)
    g, cb = {T: E[:, T]}, {}
    for t in range(T - 1, -1, -1):
        m = min(D, T - t)
        cb[t] = torch.logsumexp(torch.stack([g[t + d] for d in range(1, m + 1)]) + table(m, t + m == T, t == 0), dim=0)
        if t:
            g[t] = torch.logsumexp(A[None] + (cb[t] - E[:, t])[:, None, :], dim=2) + E[:, t]
    gamma = torch.empty_like(e)
    run = torch.exp(c[T] + g[T] - logz[:, None])
    gamma[:, T - 1] = run
    for t in range(T - 1, 0, -1):
        run = run - torch.exp(b[t] + cb[t] - logz[:, None]) + torch.exp(c[t] + g[t] - logz[:, None])
        gamma[:, t - 1] = run
    return gamma


def case(name, lens, D, a, res, lines):
    total, longest = sum(lens), max(lens)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]))
    gen = torch.Generator(device="cuda").manual_seed(5)
    logp = torch.log_softmax(torch.randn(total, 4, device="cuda", generator=gen), dim=1)
    rag = RaggedFeatures(logp, offs, 4, False)
    labels = (torch.arange(total, device="cuda") // 37 % 4).to(torch.uint8)               # (a legal walk round the cycle)
    A0, pi0 = (torch.from_numpy(v).cuda() for v in cyclic_transitions(0.0, 0.0))
    dur = gaussian_durations([0.12 * D, 0.2 * D, 0.1 * D, 0.4 * D], [0.03 * D, 0.05 * D, 0.03 * D, 0.15 * D], D)
    edge = edge_durations(dur)
    dur_d, edge_d = torch.from_numpy(dur).cuda(), torch.from_numpy(edge).cuda()
    P = min(a.prefix, min(lens))
    prefix = torch.stack([logp[o:o + P] for o in offs[:-1].tolist()])[:64]
    check = duration_posteriors(prefix, dur_d, A0, pi0, edge_d)          # (warms the kernel)
    worst = float((torch_loop(prefix, A0, pi0, dur_d, edge_d) - check).abs().max())

    def train_step():
        lp = logp.detach().requires_grad_(True)
        A, pi = A0.clone().requires_grad_(True), pi0.clone().requires_grad_(True)
        duration_nll(RaggedFeatures(lp, offs, 4, False), labels, dur_d, A, pi, edge_d).backward()
        return lp.grad
    train_step(); decode_durations(rag, dur, A0, pi0, edge)
    t_p, t_n, t_d, t_l = [], [], [], []
    for _ in range(a.rounds):
        t_p.append(timed(lambda: duration_posteriors(rag, dur_d, A0, pi0, edge_d))[0])
        t_n.append(timed(train_step)[0])
        t_d.append(timed(lambda: decode_durations(rag, dur, A0, pi0, edge))[0])
        t_l.append(timed(lambda: torch_loop(prefix, A0, pi0, dur_d, edge_d))[0] * longest / P)
    p, n, d, l = min(t_p), min(t_n), min(t_d), min(t_l)
    res[name] = {"recordings": len(lens), "steps": total, "longest": longest, "max_duration": D, "duration_posteriors_ms": round(p * 1e3, 3),
                 "duration_posteriors_steps_per_s": round(total / p), "duration_nll_fwd_bwd_ms": round(n * 1e3, 3),
                 "decode_durations_ms": round(d * 1e3, 3), "torch_loop_ms_scaled": round(l * 1e3, 1), "torch_loop_prefix_steps": P,
                 "torch_loop_recordings": int(prefix.shape[0]), "torch_loop_max_abs_difference_on_prefix": worst,
                 "duration_posteriors_rounds_ms": [round(v * 1e3, 3) for v in t_p]}
    lines.append(f"{name}, D = {D}: {len(lens)} recordings, {total} steps, longest {longest}: duration_posteriors {p * 1e3:.3f} ms "
                 f"({total / p / 1e6:.1f} M steps/s, {p * 1e6 / longest:.2f} us per step of the longest recording, rounds "
                 f"{', '.join(f'{v * 1e3:.3f}' for v in t_p)}); duration_nll forward + backward {n * 1e3:.3f} ms; decode_durations "
                 f"{d * 1e3:.3f} ms ({p / d:.1f} x); torch per-step log-space loop on {prefix.shape[0]} recordings {l * 1e3:.0f} ms SCALED from "
                 f"its first {P} steps to {longest} (max |gamma difference| on the prefix {worst:.1e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--recordings", type=int, default=792)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--prefix", type=int, default=192)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "duration_posteriors_bench.py needs a GPU"
    facts = next(iter(_lib.kernel_resources("seg_duration_posteriors_kernel").values()))
    res, lines = {"kernel": facts}, [f"seg_duration_posteriors_kernel: {facts['vgpr_count']} VGPRs, {facts['group_segment_fixed_size']} bytes "
                                     f"of LDS, {facts['private_segment_fixed_size']} bytes of scratch"]
    rng = np.random.default_rng(8)
    corpus = [int(v) for v in rng.integers(20000, 60000, size=a.recordings)]
    case("corpus list", corpus, 512, a, res, lines)
    case("corpus list at the largest D", corpus, 2048, a, res, lines)
    case("one long recording", [240000], 512, a, res, lines)
    lines.append("one long recording: one workgroup on one CU; its us per step is the per-step cost of a workgroup (both sweeps)")
    lines.append("the estimate this was planned with: 2 - 3 x the decoder's 1.2 us (D = 512) / 2.5 us (D = 2048) per step and sweep; "
                 "the lines above are the measurement")
    print("\n".join(lines)); print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
