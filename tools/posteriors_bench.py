#!/usr/bin/env python3
"""state_posteriors and sequence_nll (forward-backward on the device, one call per list) measured next to what surrounds them,
interleaved in one process:

  posteriors_bench.py [--out FILE] [--recordings 792] [--rounds 3] [--prefix 512]

  1. consumer.state_posteriors on the whole input (workspace allocation included);
  2. consumer.sequence_nll forward + backward on it (the gradient in the log-probs and in learnable transitions);
  3. consumer.decode_states, the hard decision, on the same input;
  4. a torch per-step log-space forward-backward loop on the device (float64, batched over the recordings), run on the first
     --prefix steps only and SCALED to the longest recording's steps -- the loop's cost is launches per step, so it is linear;
on two inputs: the corpus-shaped list (--recordings recordings of 20 000 - 60 000 steps) and one recording of 240 000 steps, which
one workgroup on one CU walks alone: its time over its steps is the per-step cost of a workgroup.  The log-probs are the
log-softmax of seeded noise: the kernel's time does not depend on the values.  Every way runs once per round, the rounds
alternate; the best round of each is reported."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import _lib
from heart_sounds_segmentation_amd.consumer import cyclic_transitions, decode_states, sequence_nll, state_posteriors
from heart_sounds_segmentation_amd.transforms import RaggedFeatures


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(); return time.perf_counter() - t0, out


def torch_loop(e, A, pi):
    """e (B, P, 4) on the device -> (B, P, 4) posteriors: the log-space recurrences as torch ops, a handful of launches per step."""
    e, A, pi = e.double(), A.double(), pi.double()
    B, P = e.shape[0], e.shape[1]
    la, lb = torch.empty_like(e), torch.zeros_like(e)
    la[:, 0] = pi[None] + e[:, 0]
    for t in range(1, P):
        la[:, t] = torch.logsumexp(la[:, t - 1, :, None] + A[None], dim=1) + e[:, t]
    for t in range(P - 1, 0, -1):
        lb[:, t - 1] = torch.logsumexp(A[None] + (e[:, t] + lb[:, t])[:, None, :], dim=2)
    return torch.exp(la + lb - torch.logsumexp(la[:, -1], dim=1)[:, None, None])


def case(name, lens, a, res, lines):
    total, longest = sum(lens), max(lens)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]))
    gen = torch.Generator(device="cuda").manual_seed(5)
    logp = torch.log_softmax(torch.randn(total, 4, device="cuda", generator=gen), dim=1)
    rag = RaggedFeatures(logp, offs, 4, False)
    labels = (torch.arange(total, device="cuda") // 37 % 4).to(torch.uint8)               # (a legal walk round the cycle)
    A0, pi0 = (torch.from_numpy(v).cuda() for v in cyclic_transitions(float(np.log(0.9)), float(np.log(0.1))))
    P = min(a.prefix, min(lens))
    prefix = torch.stack([logp[o:o + P] for o in offs[:-1].tolist()])
    check = state_posteriors(prefix, A0, pi0)            # (warms the kernel)
    worst = float((torch_loop(prefix, A0, pi0) - check).abs().max())

    def train_step():
        lp = logp.detach().requires_grad_(True)
        A, pi = A0.clone().requires_grad_(True), pi0.clone().requires_grad_(True)
        sequence_nll(RaggedFeatures(lp, offs, 4, False), labels, A, pi).backward()
        return lp.grad
    train_step(); decode_states(rag)
    t_p, t_n, t_d, t_l = [], [], [], []
    for _ in range(a.rounds):
        t_p.append(timed(lambda: state_posteriors(rag, A0, pi0))[0])
        t_n.append(timed(train_step)[0])
        t_d.append(timed(lambda: decode_states(rag))[0])
        t_l.append(timed(lambda: torch_loop(prefix, A0, pi0))[0] * longest / P)
    p, n, d, l = min(t_p), min(t_n), min(t_d), min(t_l)
    res[name] = {"recordings": len(lens), "steps": total, "longest": longest, "state_posteriors_ms": round(p * 1e3, 3),
                 "state_posteriors_steps_per_s": round(total / p), "sequence_nll_fwd_bwd_ms": round(n * 1e3, 3),
                 "decode_states_ms": round(d * 1e3, 3), "torch_loop_ms_scaled": round(l * 1e3, 1), "torch_loop_prefix_steps": P,
                 "torch_loop_max_abs_difference_on_prefix": worst, "state_posteriors_rounds_ms": [round(v * 1e3, 3) for v in t_p]}
    lines.append(f"{name}: {len(lens)} recordings, {total} steps, longest {longest}: state_posteriors {p * 1e3:.3f} ms "
                 f"({total / p / 1e6:.1f} M steps/s, {p * 1e9 / longest:.1f} ns per step of the longest recording, rounds "
                 f"{', '.join(f'{v * 1e3:.3f}' for v in t_p)}); sequence_nll forward + backward {n * 1e3:.3f} ms; decode_states "
                 f"{d * 1e3:.3f} ms ({p / d:.1f} x); torch per-step log-space loop {l * 1e3:.0f} ms SCALED from its first {P} steps to "
                 f"{longest} (max |gamma difference| on the prefix {worst:.1e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--recordings", type=int, default=792)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--prefix", type=int, default=512)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "posteriors_bench.py needs a GPU"
    facts = next(iter(_lib.kernel_resources("seg_posteriors_kernel").values()))
    res, lines = {"kernel": facts}, [f"seg_posteriors_kernel: {facts['vgpr_count']} VGPRs, {facts['group_segment_fixed_size']} bytes of LDS, "
                                     f"{facts['private_segment_fixed_size']} bytes of scratch"]
    rng = np.random.default_rng(8)
    case("corpus list", [int(v) for v in rng.integers(20000, 60000, size=a.recordings)], a, res, lines)
    case("one long recording", [240000], a, res, lines)
    lines.append("one long recording: one workgroup on one CU; its ns per step is the per-step cost of a workgroup")
    print("\n".join(lines)); print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
