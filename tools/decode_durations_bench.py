#!/usr/bin/env python3
"""decode_durations (explicit-duration Viterbi decoding on the device, one call per list) measured next to what surrounds it,
interleaved in one process:

  decode_durations_bench.py [--out FILE] [--recordings 792] [--rounds 3] [--durations 512 2048]

  1. the kernel: consumer.decode_durations on the whole input, once per maximum duration D (workspace allocation included);
  2. consumer.decode_states, the first-order decoder, on the same input;
  3. the HipSegmenter.ragged call that produces such log-probs (hidden 240, 44 float16 features), once, for proportion.
on the decoder bench's two inputs (tools/decode_bench.py): the corpus-shaped list (--recordings recordings of 20 000 - 60 000
steps) and one recording of 240 000 steps.  The log-probs are the log-softmax of seeded noise; the tables are heart-sized
Gaussians at 1 kHz (S1 120 +- 20 ms, systole 200 +- 40, S2 90 +- 20, diastole 400 +- 150, at least 10 ms each) cut at D.  The
forward pass costs the same whatever the values; the backtrace hops once per decoded run, and its share is reported as runs per
recording.  Ways 1 and 2 run once per round, the rounds alternate; the best round of each is reported.  No threshold is set."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import _lib
from heart_sounds_segmentation_amd.consumer import SegmenterHead, decode_durations, decode_states, gaussian_durations
from heart_sounds_segmentation_amd.transforms import RaggedFeatures


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(); return time.perf_counter() - t0, out


def case(name, lens, seg, a, res, lines):
    total, longest = sum(lens), max(lens)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]))
    gen = torch.Generator(device="cuda").manual_seed(5)
    logp = torch.log_softmax(torch.randn(total, 4, device="cuda", generator=gen), dim=1)
    rag = RaggedFeatures(logp, offs, 4, False)
    feats = RaggedFeatures(torch.randn(total, 44, device="cuda", generator=gen).half(), offs, 22, False)
    tables = {D: gaussian_durations([120, 200, 90, 400], [20, 40, 20, 150], D, min_duration=10) for D in a.durations}
    runs = {}
    for D, dur in tables.items():                        # (warms the kernels; the decoded runs respect the table)
        st = decode_durations(rag, dur)
        cuts = int((st.data[1:] != st.data[:-1]).sum())
        runs[D] = (cuts + 1) / len(lens)
    decode_states(rag)
    seg.ragged(feats, max_steps=1 << 22)                 # (warms the segmenter and grows its scratch)
    t_s = timed(lambda: seg.ragged(feats, max_steps=1 << 22))[0]
    t_d, t_f = {D: [] for D in tables}, []
    for _ in range(a.rounds):
        for D, dur in tables.items():
            t_d[D].append(timed(lambda: decode_durations(rag, dur))[0])
        t_f.append(timed(lambda: decode_states(rag))[0])
    f = min(t_f)
    res[name] = {"recordings": len(lens), "steps": total, "longest": longest, "decode_states_ms": round(f * 1e3, 3),
                 "segmenter_ragged_ms": round(t_s * 1e3, 1), "decode_durations": {}}
    lines.append(f"{name}: {len(lens)} recordings, {total} steps, longest {longest}: decode_states {f * 1e3:.3f} ms; "
                 f"HipSegmenter.ragged that makes the log-probs {t_s * 1e3:.0f} ms")
    for D in tables:
        k = min(t_d[D])
        res[name]["decode_durations"][str(D)] = {"kernel_ms": round(k * 1e3, 3), "steps_per_s": round(total / k),
                                                 "us_per_step_of_the_longest": round(k * 1e6 / longest, 4),
                                                 "runs_per_recording": round(runs[D], 1), "rounds_ms": [round(v * 1e3, 3) for v in t_d[D]]}
        lines.append(f"  decode_durations D {D}: {k * 1e3:.3f} ms ({total / k / 1e6:.1f} M steps/s, {k * 1e6 / longest:.3f} us per step of the "
                     f"longest recording, rounds {', '.join(f'{v * 1e3:.3f}' for v in t_d[D])}; {runs[D]:.0f} runs per recording): "
                     f"{k / f:.1f} x decode_states, {100 * k / t_s:.2f} % of the segmenter call")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--recordings", type=int, default=792)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--durations", type=int, nargs="+", default=[512, 2048])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decode_durations_bench.py needs a GPU"
    torch.manual_seed(4)
    seg = SegmenterHead(44, 240, 1).cuda().eval().hip()
    facts = next(iter(_lib.kernel_resources("seg_decode_durations_kernel").values()))
    res, lines = {"kernel": facts}, [f"seg_decode_durations_kernel: {facts['vgpr_count']} VGPRs, {facts['group_segment_fixed_size']} bytes of "
                                     f"LDS, {facts['private_segment_fixed_size']} bytes of scratch"]
    rng = np.random.default_rng(8)
    case("corpus list", [int(v) for v in rng.integers(20000, 60000, size=a.recordings)], seg, a, res, lines)
    case("one long recording", [240000], seg, a, res, lines)
    print("\n".join(lines)); print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
