#!/usr/bin/env python3
"""One training step of the BiLSTM segmenter on a list of whole recordings of DIFFERENT lengths, three ways, interleaved in one
process after warm-up, all with dropout active, F 44, H 240:

  ragged   HipSegmenterHead.ragged on the list: one call per layer and pass, every recording from its own ends;
  loop     the same gradient as a loop of B = 1 HipSegmenterHead calls (one forward and backward per recording, gradients
           accumulated, one clip and one Adam step): one of the 16 rows of each recurrence workgroup does work;
  padded   the dense HipSegmenterHead step on the list padded to (B, T_max, F), the loss over the real steps only.  A DIFFERENT
           model: the reverse direction starts in the padding and layer 2 is seeded from the padded ends.  Here for its time only.

A step is forward, nll_loss over all steps of the arena, backward, clip_grad_norm_(1) and Adam.  The list is seeded: --count
recordings (default 32) of --min .. --max steps (default 200 .. 2000).  The wasted-step share is seglayout::wasted_share of
csrc/segmenter_layout.hpp, restated: recordings sorted longest first into tiles of 16, sum over tiles of 16 x longest / sum T - 1.

  segmenter_train_ragged_bench.py [--out FILE] [--count N] [--min A] [--max B] [--reps R]
The one condition: the ragged step is faster than the loop on a list of 16 or more recordings.  Everything else is reported as
measured."""
import argparse, json, os, sys, time
import torch
from torch import nn
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from heart_sounds_segmentation_amd.consumer import HipSegmenterHead

F, H = 44, 240


def wasted_share(lens):
    order = sorted(lens, reverse=True)
    walked = sum(16 * order[i] for i in range(0, len(order), 16))
    return walked / sum(lens) - 1.0


def make(batch, state=None):
    torch.manual_seed(4)
    m = HipSegmenterHead(F, H, 1)
    if state is not None:
        m.load_state_dict(state)
    if batch > 1:                                                     # the padded step: the one state for every row
        m.h0, m.c0 = m.h0.expand(2, batch, H).contiguous(), m.c0.expand(2, batch, H).contiguous()
    m = m.cuda().train()
    return m, torch.optim.Adam(m.parameters(), lr=1e-3)


def finish(m, opt):
    nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()


def step_ragged(m, opt, xs, labels):
    opt.zero_grad(set_to_none=True)
    loss = nn.functional.nll_loss(m.ragged(xs).data, labels)
    loss.backward()
    finish(m, opt)
    return loss


def step_loop(m, opt, xs, ys, total):
    opt.zero_grad(set_to_none=True)
    for x, y in zip(xs, ys):
        (nn.functional.nll_loss(m(x[None])[0], y, reduction="sum") / total).backward()
    finish(m, opt)


def step_padded(m, opt, xp, yp):
    opt.zero_grad(set_to_none=True)
    nn.functional.nll_loss(m(xp).reshape(-1, 4), yp.reshape(-1), ignore_index=-100).backward()
    finish(m, opt)


def timed(fn, reps, warm):
    for _ in range(warm): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out"); ap.add_argument("--count", type=int, default=32)
    ap.add_argument("--min", type=int, default=200); ap.add_argument("--max", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=2)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "segmenter_train_ragged_bench.py needs a GPU"
    g = torch.Generator().manual_seed(9)
    lens = torch.randint(a.min, a.max + 1, (a.count,), generator=g).tolist()
    total, tmax = sum(lens), max(lens)
    xs = [torch.randn(T, F, generator=g).cuda() for T in lens]
    ys = [torch.randint(0, 4, (T,), generator=g).cuda() for T in lens]
    labels = torch.cat(ys)
    xp = nn.utils.rnn.pad_sequence(xs, batch_first=True)
    yp = nn.utils.rnn.pad_sequence(ys, batch_first=True, padding_value=-100)
    rag, rag_opt = make(1)
    loop, loop_opt = make(1, rag.state_dict())
    pad, pad_opt = make(a.count, rag.state_dict())
    fns = (lambda: step_ragged(rag, rag_opt, xs, labels), lambda: step_loop(loop, loop_opt, xs, ys, total),
           lambda: step_padded(pad, pad_opt, xp, yp))
    rounds = []
    for r in range(3):                                               # the three alternate: same clocks, same neighbours
        rounds.append([timed(fn, a.reps, 1) for fn in fns])
    t_rag, t_loop, t_pad = (min(r[i] for r in rounds) for i in range(3))
    res = {"list": {"count": a.count, "min": min(lens), "max": tmax, "steps": total, "F": F, "H": H},
           "wasted_step_share": round(wasted_share(lens), 4), "padded_share": round(a.count * tmax / total - 1.0, 4),
           "train_step_ms": {"ragged": round(t_rag * 1e3, 2), "loop_of_b1": round(t_loop * 1e3, 2), "padded_dense": round(t_pad * 1e3, 2)},
           "ragged_over_loop": round(t_rag / t_loop, 4), "ragged_over_padded": round(t_rag / t_pad, 4),
           "rounds_ms": [[round(v * 1e3, 2) for v in r] for r in rounds],
           "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2),
           "ragged_faster_than_loop": bool(t_rag < t_loop)}
    line = (f"training step on {a.count} recordings of {min(lens)} .. {tmax} steps ({total} in all), F {F}, H {H}, dropout active: "
            f"ragged {t_rag * 1e3:.1f} ms, loop of B = 1 calls {t_loop * 1e3:.1f} ms (ragged / loop {t_rag / t_loop:.3f}), padded dense "
            f"{t_pad * 1e3:.1f} ms (a different model; ragged / padded {t_rag / t_pad:.3f}); wasted steps {res['wasted_step_share']:.1%} "
            f"of the list's (padding to T_max: {res['padded_share']:.1%}); peak memory {res['peak_memory_gb']} GB")
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n" + json.dumps(res, indent=1) + "\n")
    if a.count >= 16 and not t_rag < t_loop:
        sys.exit("the ragged step is not faster than the loop of B = 1 calls")


if __name__ == "__main__":
    main()
