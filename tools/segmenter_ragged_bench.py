#!/usr/bin/env python3
"""HipSegmenter.ragged (whole recordings of different lengths in one call) against the loop of per-recording B = 1 calls it
replaces, interleaved in one process on the same features, and the ragged call alone at corpus size.

  segmenter_ragged_bench.py [--out FILE] [--recordings 792] [--max-steps N] [--corpus-only]

  loop case     64 recordings of 2 000 - 6 000 steps (seeded), hidden 240, 44 features: two rounds, the two paths alternating
  corpus case   --recordings recordings of 20 000 - 60 000 steps (the stand-in of tools/ragged_bench.py), float16 features,
                processed under --max-steps (default: HipSegmenter.ragged's own)
The features are seeded noise: the kernels' time does not depend on the values.  Wasted-step share = sum over tiles of
16 x the tile's longest recording, over the total steps, minus 1 (per group of max_steps).
HSSFSST_SEG_RAGGED_PRE_MIB=N in the environment runs the ragged calls with a projection scratch of N MiB instead of the dense
call's 128 (same bits, fewer and longer launches): run --corpus-only once per value to see whether a larger bound pays.
Done means: ragged is faster than the loop in the same run; the ratio goes to profiles/ and README."""
import argparse, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd.consumer import SegmenterHead
from heart_sounds_segmentation_amd.transforms import RaggedFeatures


def timed(fn, reps, warm=1):
    for _ in range(warm): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / reps


def groups(lens, max_steps):
    """The consecutive groups HipSegmenter.ragged forms."""
    out, i = [], 0
    while i < len(lens):
        j, tot = i + 1, lens[i]
        while j < len(lens) and tot + lens[j] <= max_steps:
            tot += lens[j]; j += 1
        out.append(lens[i:j]); i = j
    return out


def wasted_share(lens, max_steps):
    walked = 0
    for g in groups(list(lens), max_steps):
        s = sorted(g, reverse=True)
        walked += sum(16 * s[t] for t in range(0, len(s), 16))
    return walked / sum(lens) - 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--recordings", type=int, default=792)
    ap.add_argument("--max-steps", type=int, default=1 << 23); ap.add_argument("--corpus-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "segmenter_ragged_bench.py needs a GPU"
    torch.manual_seed(4)
    head = SegmenterHead(44, 240, 1).cuda().eval()
    seg = head.hip()
    pre_mib = int(os.environ.get("HSSFSST_SEG_RAGGED_PRE_MIB") or 0) or 128
    res, lines = {"pre_scratch_mib": pre_mib}, []
    if not a.corpus_only:
        loop_case(seg, np.random.default_rng(7), res, lines)
    corpus_case(seg, np.random.default_rng(8), a, res, lines, pre_mib)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")


def loop_case(seg, rng, res, lines):
    lens = [int(v) for v in rng.integers(2000, 6001, size=64)]
    xs = [torch.randn(T, 44, device="cuda") for T in lens]

    def loop():
        return [seg(x[None]) for x in xs]
    same = all(torch.equal(a_[0], b_) for a_, b_ in zip(loop(), seg.ragged(xs)))
    # (the check above warmed both paths; the loop costs seconds, so it runs once per round)
    rounds = [(timed(loop, 1, warm=0), timed(lambda: seg.ragged(xs), 3, warm=0)) for _ in range(2)]
    t_loop, t_rag = min(r[0] for r in rounds), min(r[1] for r in rounds)
    res["loop_case"] = {"recordings": 64, "steps": sum(lens), "longest": max(lens), "loop_b1_ms": round(t_loop * 1e3, 2),
                        "ragged_ms": round(t_rag * 1e3, 2), "speedup": round(t_loop / t_rag, 2), "bit_identical": bool(same),
                        "wasted_share": round(wasted_share(lens, 1 << 23), 4),
                        "rounds_ms": [[round(r[0] * 1e3, 2), round(r[1] * 1e3, 2)] for r in rounds]}
    lines.append(f"64 recordings of 2 000 - 6 000 steps ({sum(lens)} steps, longest {max(lens)}): loop of B = 1 calls {t_loop * 1e3:.1f} ms, "
                 f"ragged {t_rag * 1e3:.1f} ms: {t_loop / t_rag:.1f} x; bit-identical {same}; wasted-step share "
                 f"{100 * res['loop_case']['wasted_share']:.1f} %")


def corpus_case(seg, rng, a, res, lines, pre_mib):
    lens = [int(v) for v in rng.integers(20000, 60000, size=a.recordings)]
    arena = torch.randn(sum(lens), 44, device="cuda", dtype=torch.float16)
    feats = RaggedFeatures(arena, torch.tensor(np.concatenate([[0], np.cumsum(lens)])), 22, False)
    t_big = timed(lambda: seg.ragged(feats, max_steps=a.max_steps), 1, warm=1)
    ng = len(groups(lens, a.max_steps))
    w = wasted_share(lens, a.max_steps)
    res["corpus_case"] = {"recordings": a.recordings, "steps": sum(lens), "max_steps": a.max_steps, "groups": ng,
                          "ragged_ms": round(t_big * 1e3, 1), "us_per_recording": round(t_big * 1e6 / a.recordings, 1),
                          "steps_per_s": round(sum(lens) / t_big), "wasted_share": round(w, 4)}
    lines.append(f"{a.recordings} recordings of 20 000 - 60 000 steps ({sum(lens)} steps, float16 features), max_steps {a.max_steps} "
                 f"({ng} groups), projection scratch {pre_mib} MiB: ragged {t_big * 1e3:.0f} ms, {sum(lens) / t_big / 1e6:.2f} M steps/s; wasted-step share {100 * w:.1f} %")


if __name__ == "__main__":
    main()
