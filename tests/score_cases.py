"""The contract of hssfsst_score_states (include/hssfsst.h) restated in numpy, with nothing imported from the package, and the
cases of tests/test_segmentation_scores.py.

A step with a label 0..3 and a predicted state 0..3 is counted, any other is ignored.  confusion[label][predicted] counts the
counted steps.  For a class c the counted steps are positives (label == c) or negatives, and 2U = sum over (positive, negative)
pairs of 2 [s_p > s_n] + [s_p == s_n] on column c of the scores, in float32's order with -0 == +0 and NaN read as -inf.
``restate`` ranks with an argsort of an order-preserving integer key and counts tie groups with bincount; ``brute_force`` compares
every pair as floats."""
import numpy as np

IGNORE = 255


# ------------------------------------------------------------------------------------------------ the restatement
def key32(x):
    """float32 array -> uint32 keys that order as the floats do: NaN -> -inf, -0 -> +0."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    u[(u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)] = np.uint32(0xff800000)
    u[(u << np.uint32(1)) == 0] = np.uint32(0)
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def predicted(logp, states):
    """The predicted state per step: the given states, else the argmax with NaN as -inf and ties to the smaller state."""
    if states is not None:
        return np.asarray(states).astype(np.int64)
    v = np.where(np.isnan(logp), -np.inf, logp.astype(np.float64))
    return np.argmax(v, axis=1).astype(np.int64)         # (the first maximum: the smaller state; -0 == +0 under ==)


def rank_of(scores, positive):
    """(2U, P, N) of one class over the counted steps: exact Python ints."""
    k = key32(scores)
    order = np.argsort(k, kind="stable")
    ks, ps = k[order], positive[order]
    group = np.cumsum(np.concatenate([[0], (ks[1:] != ks[:-1]).astype(np.int64)])) if ks.size else np.zeros(0, dtype=np.int64)
    ngroups = int(group[-1]) + 1 if ks.size else 0
    Pg = np.bincount(group[ps], minlength=ngroups).astype(np.int64)
    Ng = np.bincount(group[~ps], minlength=ngroups).astype(np.int64)
    below = np.cumsum(Ng) - Ng
    u2 = sum(int(p) * (2 * int(b) + int(n)) for p, b, n in zip(Pg, below, Ng) if p)
    return u2, int(positive.sum()), int((~positive).sum())


def restate(logp, states, labels, offs, per_recording, want_rank=True):
    """-> {"confusion": (G, 4, 4) int64, "ignored": (G,) int64, "rank": (G, 4, 3) int64 or None}; G = recordings or 1."""
    labels = np.asarray(labels).astype(np.int64)
    pred = predicted(logp, states)
    use = (labels >= 0) & (labels <= 3) & (pred >= 0) & (pred <= 3)
    spans = [(offs[i], offs[i + 1]) for i in range(len(offs) - 1)] if per_recording else [(0, offs[-1])]
    G = len(spans)
    out = {"confusion": np.zeros((G, 4, 4), dtype=np.int64), "ignored": np.zeros((G,), dtype=np.int64),
           "rank": np.zeros((G, 4, 3), dtype=np.int64) if want_rank else None}
    for g, (a, b) in enumerate(spans):
        u = use[a:b]
        lab, pr = labels[a:b][u], pred[a:b][u]
        out["confusion"][g] = np.bincount(4 * lab + pr, minlength=16).reshape(4, 4)
        out["ignored"][g] = int((~u).sum())
        if want_rank:
            for c in range(4):
                out["rank"][g, c] = rank_of(logp[a:b][u, c], lab == c)
    return out


def brute_force(logp, states, labels, offs, per_recording):
    """The same integers from the definition, every pair compared as float32 (NaN read as -inf first)."""
    labels = np.asarray(labels).astype(np.int64)
    pred = predicted(logp, states)
    spans = [(offs[i], offs[i + 1]) for i in range(len(offs) - 1)] if per_recording else [(0, offs[-1])]
    G = len(spans)
    out = {"confusion": np.zeros((G, 4, 4), dtype=np.int64), "ignored": np.zeros((G,), dtype=np.int64),
           "rank": np.zeros((G, 4, 3), dtype=np.int64)}
    s = np.where(np.isnan(logp), np.float32(-np.inf), logp).astype(np.float32)
    for g, (a, b) in enumerate(spans):
        steps = [t for t in range(a, b) if 0 <= labels[t] <= 3 and 0 <= pred[t] <= 3]
        out["ignored"][g] = (b - a) - len(steps)
        for t in steps:
            out["confusion"][g, labels[t], pred[t]] += 1
        for c in range(4):
            pos = [t for t in steps if labels[t] == c]
            neg = [t for t in steps if labels[t] != c]
            u2 = sum(2 if s[p, c] > s[n, c] else (1 if s[p, c] == s[n, c] else 0) for p in pos for n in neg)
            out["rank"][g, c] = (u2, len(pos), len(neg))
    return out


def _ratio(num, den):
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.where(den == 0, 0.0, num / np.where(den == 0, 1.0, den))


def derived(r):
    """The figures of SegmentationScores from the integers, in float64 numpy; leading axis G."""
    cm = r["confusion"]
    tp = np.diagonal(cm, axis1=-2, axis2=-1)
    support, said = cm.sum(axis=-1), cm.sum(axis=-2)
    out = {"support": support, "accuracy": _ratio(tp.sum(axis=-1), cm.sum(axis=(-2, -1))), "precision": _ratio(tp, said),
           "recall": _ratio(tp, support), "f1": _ratio(2 * tp, said + support)}
    for k in ("precision", "recall", "f1"):
        out["macro_" + k] = out[k].mean(axis=-1)
    if r["rank"] is not None:
        rk = r["rank"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["auroc"] = rk[..., 0] / (2.0 * rk[..., 1] * rk[..., 2])
            defined = ~np.isnan(out["auroc"])
            out["macro_auroc"] = np.where(defined.any(axis=-1), np.where(defined, out["auroc"], 0.0).sum(axis=-1) / np.maximum(defined.sum(axis=-1), 1),
                                          np.nan)
    return out


# ------------------------------------------------------------------------------------------------ the cases
def offsets(lens):
    return [0] + [int(v) for v in np.cumsum(lens)]


def scores(pattern, n, seed):
    """(n, 4) float32 in one of the patterns of the issue."""
    g = np.random.default_rng(seed)
    if pattern == "eighths":                             # ties are the rule
        return (np.round(g.normal(size=(n, 4)) * 8.0) / 8.0).astype(np.float32)
    if pattern == "log_softmax":
        x = g.normal(size=(n, 4)) * 3.0
        return (x - np.log(np.exp(x).sum(axis=1, keepdims=True))).astype(np.float32)
    if pattern == "constant":                            # one tie group over every block: 2U = P N
        return np.full((n, 4), -1.25, dtype=np.float32)
    if pattern in ("ascending", "descending"):
        col = np.arange(n, dtype=np.float32) / 4.0 - 3.0
        col = col if pattern == "ascending" else col[::-1]
        return np.ascontiguousarray(np.stack([col, -col, col * 0.5, -col * 2.0], axis=1), dtype=np.float32)
    if pattern.startswith("byte"):                       # keys that differ in exactly one byte, whichever the class
        k = int(pattern[4:])
        base = np.uint32(0x3f000000 if k < 3 else 0)
        bits = (g.integers(0, 256, size=(n, 4)).astype(np.uint32) << np.uint32(8 * k)) | base
        return bits.view(np.float32)
    if pattern == "specials":                            # +-0, -inf, NaN and +inf mixed into rounded scores
        x = (np.round(g.normal(size=(n, 4)) * 4.0) / 4.0).astype(np.float32)
        special = np.array([0.0, -0.0, -np.inf, np.nan, np.inf, -np.nan], dtype=np.float32)
        pick = g.integers(0, 12, size=(n, 4))
        return np.where(pick < 6, special[np.minimum(pick, 5)], x).astype(np.float32)
    raise ValueError(pattern)


def labels_for(pattern, lens, seed):
    """uint8 labels over the list.  "plain": 0..3; "mixed": class 3 never occurs, some steps are 4 or 255 and the second recording
    (where there is one) is ignored altogether."""
    g = np.random.default_rng(1000 + seed)
    n = int(sum(lens))
    if pattern == "plain":
        return g.integers(0, 4, size=n).astype(np.uint8)
    lab = g.integers(0, 3, size=n).astype(np.uint8)
    r = g.integers(0, 10, size=n)
    lab[r == 0] = 4
    lab[r == 1] = IGNORE
    if len(lens) > 1:
        lab[lens[0]:lens[0] + lens[1]] = IGNORE
    return lab


def list_lens(count, seed=0):
    """The list sizes of the issue: recordings of 1 .. 40 steps with a few longer ones."""
    g = np.random.default_rng(2000 + seed + count)
    lens = [int(v) for v in g.integers(1, 41, size=count)]
    for i in range(0, count, 7):
        lens[i] += int(g.integers(100, 700))
    return lens
