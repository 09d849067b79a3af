#!/usr/bin/env python3
"""decode_states (Viterbi decoding of log-probs on the device, one call per list) measured three ways, interleaved in one process:

  decode_bench.py [--out FILE] [--recordings 792] [--rounds 3] [--prefix 512]

  1. the kernel: consumer.decode_states on the whole input;
  2. a torch per-step Viterbi loop on the device (float32, batched over the recordings, forward and backtrace), run on the first
     --prefix steps only and SCALED to the longest recording's steps -- the loop's cost is launches per step, so it is linear;
  3. the HipSegmenter.ragged call that produces such log-probs (hidden 240, 44 float16 features), for proportion.
on two inputs: the corpus-shaped list (--recordings recordings of 20 000 - 60 000 steps) and one recording of 240 000 steps.  The
log-probs are the log-softmax of seeded noise: the kernel's time does not depend on the values.  Every way runs once per round,
the rounds alternate; the best round of each is reported."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import _lib
from heart_sounds_segmentation_amd.consumer import SegmenterHead, cyclic_transitions, decode_states
from heart_sounds_segmentation_amd.transforms import RaggedFeatures


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(); return time.perf_counter() - t0, out


def torch_loop(e, A, pi):
    """e (B, P, 4) float32 on the device -> (B, P) states: the recurrence as torch ops, a handful of launches per step."""
    B, P = e.shape[0], e.shape[1]
    d = pi[None] + e[:, 0]
    psi = torch.empty((B, P, 4), dtype=torch.int64, device=e.device)
    for t in range(1, P):
        best, arg = (d[:, :, None] + A[None]).max(dim=1)
        d = best + e[:, t]
        psi[:, t] = arg
    s = d.argmax(dim=1)
    out = torch.empty((B, P), dtype=torch.uint8, device=e.device)
    rows = torch.arange(B, device=e.device)
    for t in range(P - 1, 0, -1):
        out[:, t] = s
        s = psi[rows, t, s]
    out[:, 0] = s
    return out


def case(name, lens, seg, a, res, lines):
    total, longest = sum(lens), max(lens)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]))
    gen = torch.Generator(device="cuda").manual_seed(5)
    logp = torch.log_softmax(torch.randn(total, 4, device="cuda", generator=gen), dim=1)
    rag = RaggedFeatures(logp, offs, 4, False)
    feats = RaggedFeatures(torch.randn(total, 44, device="cuda", generator=gen).half(), offs, 22, False)
    A, pi = (torch.from_numpy(v).cuda() for v in cyclic_transitions())
    P = min(a.prefix, min(lens))
    prefix = torch.stack([logp[o:o + P] for o in offs[:-1].tolist()])
    check = decode_states(prefix)                        # (warms the kernel; the loop agrees with it wherever float32 has no tie)
    same = float((torch_loop(prefix, A, pi) == check).float().mean())
    seg.ragged(feats, max_steps=1 << 22)                 # (warms the segmenter and grows its scratch)
    t_k, t_l, t_s = [], [], []
    for _ in range(a.rounds):
        t_k.append(timed(lambda: decode_states(rag))[0])
        t_l.append(timed(lambda: torch_loop(prefix, A, pi))[0] * longest / P)
        t_s.append(timed(lambda: seg.ragged(feats, max_steps=1 << 22))[0])
    k, l, s = min(t_k), min(t_l), min(t_s)
    res[name] = {"recordings": len(lens), "steps": total, "longest": longest, "kernel_ms": round(k * 1e3, 3),
                 "kernel_steps_per_s": round(total / k), "torch_loop_ms_scaled": round(l * 1e3, 1), "torch_loop_prefix_steps": P,
                 "torch_loop_agreement_on_prefix": round(same, 4), "segmenter_ragged_ms": round(s * 1e3, 1),
                 "kernel_rounds_ms": [round(v * 1e3, 3) for v in t_k]}
    lines.append(f"{name}: {len(lens)} recordings, {total} steps, longest {longest}: decode kernel {k * 1e3:.3f} ms "
                 f"({total / k / 1e6:.0f} M steps/s, rounds {', '.join(f'{v * 1e3:.3f}' for v in t_k)}); torch per-step loop "
                 f"{l * 1e3:.0f} ms SCALED from its first {P} steps to {longest} (agrees with the kernel on {100 * same:.2f} % of the "
                 f"prefix's steps: float32 against exact ties); HipSegmenter.ragged that makes the log-probs {s * 1e3:.0f} ms: "
                 f"the decode is {100 * k / s:.3f} % of it")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--recordings", type=int, default=792)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--prefix", type=int, default=512)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decode_bench.py needs a GPU"
    torch.manual_seed(4)
    seg = SegmenterHead(44, 240, 1).cuda().eval().hip()
    facts = next(iter(_lib.kernel_resources("seg_decode_kernel").values()))
    res, lines = {"kernel": facts}, [f"seg_decode_kernel: {facts['vgpr_count']} VGPRs, {facts['group_segment_fixed_size']} bytes of LDS, "
                                     f"{facts['private_segment_fixed_size']} bytes of scratch"]
    rng = np.random.default_rng(8)
    case("corpus list", [int(v) for v in rng.integers(20000, 60000, size=a.recordings)], seg, a, res, lines)
    case("one long recording", [240000], seg, a, res, lines)
    print("\n".join(lines)); print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
