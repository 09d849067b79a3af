#!/usr/bin/env python3
"""The scoring call (hssfsst_score_states: counts, then per class keys, a radix sort and the rank) measured next to a torch
restatement on the device, interleaved in one process:

  score_bench.py [--out FILE] [--recordings 792] [--rounds 3] [--case all|corpus|long] [--bench-lines FILE] [--kernel-stats CSV]

  1. consumer.segmentation_scores pooled and per recording, with and without the rank (workspace and output allocation included);
  2. the same integers from torch ops on the same arena, written here: argmax + bincount for the table, and per class torch.sort,
     tie groups by comparing neighbours, cumsum and bincount for 2U (pooled only: per recording torch would sort a padded batch,
     which is what this package does not do).  It reads the number of tie groups back, so it waits for the device once per class;
on 792 recordings of 20 000 - 60 000 steps and on one recording of 240 000 steps.  Every way runs once per round, the rounds
alternate; the best round of each is reported, and the pooled integers of the two are compared.  --bench-lines: a file with
bench.py's result lines (the parent commit's and this tree's), copied into the report.  --kernel-stats: a rocprofv3 --kernel-trace
--stats kernel table (csv) of a run of this tool: the time of every seg_score kernel.  Nothing here is gated."""
import argparse, csv, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import _lib
from heart_sounds_segmentation_amd.consumer import score_info, segmentation_scores
from heart_sounds_segmentation_amd.transforms import RaggedFeatures


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(); return time.perf_counter() - t0, out


def torch_scores(logp, labels, rank=True):
    """confusion (4, 4) and rank (4, 3) = {2U, P, N} of the pooled arena from torch ops (scores without NaN or -0)."""
    use = labels <= 3
    lab, lp = labels[use].long(), logp[use]
    confusion = torch.bincount(4 * lab + lp.argmax(dim=1), minlength=16).view(4, 4)
    if not rank:
        return confusion, None
    out = torch.zeros((4, 3), dtype=torch.int64, device=logp.device)
    for c in range(4):
        s, idx = torch.sort(lp[:, c])
        pos = (lab == c)[idx]
        head = torch.ones_like(pos)
        head[1:] = s[1:] != s[:-1]
        gid = torch.cumsum(head, 0) - 1
        G = int(gid[-1]) + 1 if gid.numel() else 0
        Pg, Ng = torch.bincount(gid[pos], minlength=G), torch.bincount(gid[~pos], minlength=G)
        below = torch.cumsum(Ng, 0) - Ng
        out[c, 0], out[c, 1], out[c, 2] = (Pg * (2 * below + Ng)).sum(), Pg.sum(), Ng.sum()
    return confusion, out


def case(name, lens, a, res, lines):
    total = sum(lens)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]))
    gen = torch.Generator(device="cuda").manual_seed(5)
    logp = torch.log_softmax(3.0 * torch.randn(total, 4, device="cuda", generator=gen), dim=1)
    labels = torch.randint(0, 4, (total,), device="cuda", generator=gen, dtype=torch.uint8)
    labels[::97] = 255
    rag = RaggedFeatures(logp, offs, 4, False)
    ways = {"pooled": lambda: segmentation_scores(rag, labels), "pooled_counts_only": lambda: segmentation_scores(rag, labels, auroc=False),
            "per_recording": lambda: segmentation_scores(rag, labels, per_recording=True),
            "per_recording_counts_only": lambda: segmentation_scores(rag, labels, per_recording=True, auroc=False),
            "torch_pooled": lambda: torch_scores(logp, labels), "torch_pooled_counts_only": lambda: torch_scores(logp, labels, rank=False)}
    first = {k: fn() for k, fn in ways.items()}          # (warms the kernels)
    same = bool(torch.equal(first["pooled"].confusion, first["torch_pooled"][0]) and torch.equal(first["pooled"].rank, first["torch_pooled"][1]))
    folded = bool(torch.equal(first["per_recording"].confusion.sum(0), first["pooled"].confusion))
    del first
    times = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            times[k].append(timed(fn)[0])
    best = {k: min(v) for k, v in times.items()}
    res[name] = {"recordings": len(lens), "steps": total, "longest": max(lens), "work_bytes": score_info()[0] * total + score_info()[2],
                 "pooled_equals_torch": same, "per_recording_tables_sum_to_pooled": folded,
                 **{k + "_ms": round(v * 1e3, 3) for k, v in best.items()}, **{k + "_rounds_ms": [round(x * 1e3, 3) for x in v] for k, v in times.items()}}
    ms = {k: v * 1e3 for k, v in best.items()}
    lines.append(f"{name}: {len(lens)} recordings, {total} steps: pooled {ms['pooled']:.3f} ms (counts only {ms['pooled_counts_only']:.3f}), per recording "
                 f"{ms['per_recording']:.3f} ms (counts only {ms['per_recording_counts_only']:.3f}); torch on the device, pooled {ms['torch_pooled']:.3f} ms "
                 f"(counts only {ms['torch_pooled_counts_only']:.3f}); this call / torch = {ms['pooled'] / ms['torch_pooled']:.2f} pooled, "
                 f"{ms['pooled_counts_only'] / ms['torch_pooled_counts_only']:.2f} counts only; the pooled integers {'equal' if same else 'DIFFER FROM'} "
                 f"torch's; rounds of pooled {', '.join(f'{v * 1e3:.3f}' for v in times['pooled'])}")


def kernel_stats(path):
    """rocprofv3's kernel stats table -> {kernel: (calls, total ms)} of the seg_score kernels."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            if "seg_score_" in name:
                short = name.split("seg_score_")[1].split("(")[0]
                out["seg_score_" + short] = (int(row["Calls"]), float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)")) / 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--recordings", type=int, default=792); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bench-lines"); ap.add_argument("--kernel-stats"); ap.add_argument("--case", default="all", choices=("all", "corpus", "long"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "score_bench.py needs a GPU"
    res, lines = {"kernels": {}}, []
    for k, facts in sorted(_lib.kernel_resources("seg_score_").items()):
        res["kernels"][k] = facts
        lines.append(f"{k}: {facts['vgpr_count']} VGPRs, {facts['agpr_count']} AGPRs, {facts['group_segment_fixed_size']} bytes of LDS, "
                     f"{facts['private_segment_fixed_size']} bytes of scratch")
    rng = np.random.default_rng(8)
    if a.case in ("all", "corpus"):
        case("corpus list", [int(v) for v in rng.integers(20000, 60000, size=a.recordings)], a, res, lines)
    if a.case in ("all", "long"):
        case("one long recording", [240000], a, res, lines)
    lines.append("the expectation this was planned with, unmeasured: the passes are HBM-bound and the pooled call lands in single-digit "
                 "milliseconds on the list; the lines above are the measurement")
    if a.kernel_stats:
        st = kernel_stats(a.kernel_stats)
        res["kernel_stats"] = {k: {"calls": c, "total_ms": round(ms, 3)} for k, (c, ms) in st.items()}
        lines.append("kernel time under rocprofv3 --kernel-trace --stats, a separate run of this tool (warm-up included): "
                     + "; ".join(f"{k} {c} calls, {ms:.1f} ms in all" for k, (c, ms) in sorted(st.items(), key=lambda kv: -kv[1][1])))
    if a.bench_lines:
        lines.append("bench.py --gpus 1 --steps 50 --warmup 10, the parent commit and this tree, alternating (value, ms per step, spread of the step):")
        with open(a.bench_lines) as fh:
            for ln in fh:
                if "{" not in ln:
                    continue
                label, r = ln.split("{", 1)[0].strip(), json.loads(ln[ln.index("{"):])
                lines.append(f"  {label} {r['value']} {r['unit']}, {r['ms_per_step']} ms per step, {json.dumps(r['roofline']['step_ms_spread'])}")
    print("\n".join(lines)); print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
