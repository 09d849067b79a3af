#!/usr/bin/env python3
"""The run-length counts call (hssfsst_posteriors_durations_counts: the sweeps that also leave g, then the counts launches) measured
next to the plain call it extends, interleaved in one process:

  duration_counts_bench.py [--out FILE] [--recordings 792] [--rounds 3] [--case all|corpus|largest|long] [--parent-lib LIB] [--kernel-stats CSV]

  1. consumer.duration_posteriors without and with return_counts (workspace and output allocation included);
  2. consumer.duration_nll forward + backward without and with learn_durations (the tables then require grad);
  3. with --parent-lib, a libhssfsst.so built from the parent commit: hssfsst_posteriors_durations through the C ABI of that
     library and of this tree's, alternating, on the same buffers -- whether the existing path moved;
on tools/duration_posteriors_bench.py's inputs: the corpus-shaped list (--recordings recordings of 20 000 - 60 000 steps) at D = 512
and D = 2048 and one recording of 240 000 steps at D = 512.  Every way runs once per round, the rounds alternate; the best round of
each is reported.  --kernel-stats: a rocprofv3 --kernel-trace --stats kernel table (csv) of a run of this tool, from which the
time of the three kernels is added -- where the extra time of the counts call goes.  Nothing here is gated."""
import argparse, ctypes, csv, json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd import _lib
from heart_sounds_segmentation_amd.consumer import (cyclic_transitions, duration_counts_info, duration_nll, duration_posteriors,
                                                    duration_posteriors_info, edge_durations, gaussian_durations)
from heart_sounds_segmentation_amd.transforms import RaggedFeatures

KERNELS = ("seg_duration_posteriors_kernel", "seg_duration_runs_sweep_kernel", "seg_duration_run_counts_kernel")


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(); return time.perf_counter() - t0, out


def plain_call(lib, logp, offs, a_pi, dur, edge, gamma, loglik, work):
    """hssfsst_posteriors_durations of the library `lib` (a ctypes.CDLL) on the given device buffers."""
    fn = lib.hssfsst_posteriors_durations
    fn.argtypes = _lib.lib().hssfsst_posteriors_durations.argtypes
    fn.restype = ctypes.c_int
    rc = fn(logp.data_ptr(), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(offs) - 1, a_pi.data_ptr(), dur.data_ptr(), edge.data_ptr(),
            int(dur.shape[1]), None, gamma.data_ptr(), None, loglik.data_ptr(), None, None, None, work.data_ptr(), work.numel(), 0,
            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc


def case(name, lens, D, a, parent, res, lines):
    total, longest = sum(lens), max(lens)
    offs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]))
    gen = torch.Generator(device="cuda").manual_seed(5)
    logp = torch.log_softmax(torch.randn(total, 4, device="cuda", generator=gen), dim=1)
    rag = RaggedFeatures(logp, offs, 4, False)
    labels = (torch.arange(total, device="cuda") // 37 % 4).to(torch.uint8)               # (a legal walk round the cycle)
    A0, pi0 = (torch.from_numpy(v).cuda() for v in cyclic_transitions(0.0, 0.0))
    dur = gaussian_durations([0.12 * D, 0.2 * D, 0.1 * D, 0.4 * D], [0.03 * D, 0.05 * D, 0.03 * D, 0.15 * D], D)
    dur_d, edge_d = torch.from_numpy(dur).cuda(), torch.from_numpy(edge_durations(dur)).cuda()

    def train_step(learn):
        lp = logp.detach().requires_grad_(True)
        A, pi = A0.clone().requires_grad_(True), pi0.clone().requires_grad_(True)
        d, e = (dur_d.clone().requires_grad_(True), edge_d.clone().requires_grad_(True)) if learn else (dur_d, edge_d)
        duration_nll(RaggedFeatures(lp, offs, 4, False), labels, d, A, pi, e, learn_durations=learn).backward()
        return lp.grad
    ways = {"duration_posteriors": lambda: duration_posteriors(rag, dur_d, A0, pi0, edge_d),
            "duration_posteriors_counts": lambda: duration_posteriors(rag, dur_d, A0, pi0, edge_d, return_counts=True),
            "duration_nll_fwd_bwd": lambda: train_step(False), "duration_nll_learn_durations_fwd_bwd": lambda: train_step(True)}
    if parent is not None:
        _, _, _, per, rec, per_d = duration_posteriors_info()
        o = np.asarray(offs, dtype=np.int64)
        a_pi = torch.cat([A0.reshape(-1), pi0]).contiguous()
        gamma, loglik = torch.empty((total, 4), device="cuda"), torch.empty((len(lens),), dtype=torch.float64, device="cuda")
        work = torch.empty((per * total + rec * len(lens) + per_d * D,), dtype=torch.uint8, device="cuda")
        ways["plain_call_parent_library"] = lambda: plain_call(parent, logp, o, a_pi, dur_d, edge_d, gamma, loglik, work)
        ways["plain_call_this_library"] = lambda: plain_call(_lib.lib(), logp, o, a_pi, dur_d, edge_d, gamma, loglik, work)
    for fn in ways.values():
        fn()                                             # (warms the kernels)
    times = {k: [] for k in ways}
    for _ in range(a.rounds):
        for k, fn in ways.items():
            times[k].append(timed(fn)[0])
    best = {k: min(v) for k, v in times.items()}
    res[name] = {"recordings": len(lens), "steps": total, "longest": longest, "max_duration": D,
                 "counts_bytes": 64 * D * len(lens), "work_bytes_per_step": duration_counts_info()[0],
                 **{k + "_ms": round(v * 1e3, 3) for k, v in best.items()}, **{k + "_rounds_ms": [round(x * 1e3, 3) for x in v] for k, v in times.items()}}
    p, c = best["duration_posteriors"], best["duration_posteriors_counts"]
    n, m = best["duration_nll_fwd_bwd"], best["duration_nll_learn_durations_fwd_bwd"]
    line = (f"{name}, D = {D}: {len(lens)} recordings, {total} steps, longest {longest}: duration_posteriors {p * 1e3:.3f} ms, with return_counts "
            f"{c * 1e3:.3f} ms (+{(c / p - 1) * 100:.1f} %, rounds {', '.join(f'{v * 1e3:.3f}' for v in times['duration_posteriors_counts'])}; counts "
            f"{64 * D * len(lens) / 2 ** 20:.1f} MiB); duration_nll forward + backward {n * 1e3:.3f} ms, with learn_durations {m * 1e3:.3f} ms "
            f"(+{(m / n - 1) * 100:.1f} %)")
    if parent is not None:
        q, t = best["plain_call_parent_library"], best["plain_call_this_library"]
        line += (f"; hssfsst_posteriors_durations alone: the parent commit's library {q * 1e3:.3f} ms, this one {t * 1e3:.3f} ms "
                 f"({(t / q - 1) * 100:+.2f} %)")
    lines.append(line)


def kernel_stats(path):
    """rocprofv3's kernel stats table -> {kernel: (calls, total ms)} of the three kernels."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            for k in KERNELS:
                if k in name:
                    out[k] = (int(row["Calls"]), float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)")) / 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--recordings", type=int, default=792); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib"); ap.add_argument("--kernel-stats"); ap.add_argument("--case", default="all", choices=("all", "corpus", "largest", "long"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "duration_counts_bench.py needs a GPU"
    res, lines = {"kernels": {}}, []
    for k in KERNELS:
        facts = next(iter(_lib.kernel_resources(k).values()))
        res["kernels"][k] = facts
        lines.append(f"{k}: {facts['vgpr_count']} VGPRs, {facts['agpr_count']} AGPRs, {facts['group_segment_fixed_size']} bytes of LDS, "
                     f"{facts['private_segment_fixed_size']} bytes of scratch")
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    if parent is not None:
        facts = next(iter(_lib.kernel_resources("seg_duration_posteriors_kernel", os.path.abspath(a.parent_lib)).values()))
        res["kernels"]["seg_duration_posteriors_kernel (parent commit)"] = facts
        lines.append(f"seg_duration_posteriors_kernel of the parent commit's library: {facts['vgpr_count']} VGPRs, {facts['agpr_count']} AGPRs, "
                     f"{facts['group_segment_fixed_size']} bytes of LDS, {facts['private_segment_fixed_size']} bytes of scratch")
    rng = np.random.default_rng(8)
    corpus = [int(v) for v in rng.integers(20000, 60000, size=a.recordings)]
    if a.case in ("all", "corpus"):
        case("corpus list", corpus, 512, a, parent, res, lines)
    if a.case in ("all", "largest"):
        case("corpus list at the largest D", corpus, 2048, a, parent, res, lines)
    if a.case in ("all", "long"):
        case("one long recording", [240000], 512, a, parent, res, lines)
    lines.append("the estimate this was planned with: about 20 float64 vector instructions per lane and step for the counts kernel, 17 ms for the "
                 "long recording and a few tens of ms for the list; the lines above are the measurement")
    if a.kernel_stats:
        st = kernel_stats(a.kernel_stats)
        res["kernel_stats"] = {k: {"calls": c, "total_ms": round(ms, 3)} for k, (c, ms) in st.items()}
        lines.append("kernel time under rocprofv3 --kernel-trace --stats, a separate run of this tool (every case, warm-up included): "
                     + "; ".join(f"{k} {c} calls, {ms:.1f} ms in all, {ms / c:.2f} ms a call" for k, (c, ms) in st.items()))
    print("\n".join(lines)); print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
