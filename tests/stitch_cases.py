"""The contract of hssfsst_stitch_windows (include/hssfsst.h) restated in numpy float64, with nothing imported from the package, an
independent per-step brute force, and the cases of tests/test_stitch_windows.py.

The covering windows of a T-step recording (windows of n steps at stride 1 <= stride <= n): T <= n -- one window [0, T); else
the floor((T - n) / stride) + 1 regular windows [i stride, i stride + n) and, if (T - n) % stride != 0, the tail [T - n, T).  A
recording's windows lie back to back from row win_first on.  For a step, its covering windows in ascending start order give the
rows v_k with weights w_k = w[position]: one window, or mode "select" (the largest w_k, ties to the earlier window) -- a row is
copied; "prob" -- a_j = log(sum_k w_k exp(v_kj - M) / sum_k w_k) + M with M the largest of the values; "logp" -- a_j = sum_k w_k
v_kj / sum_k w_k; both then out_j = a_j - logsumexp_j(a), float64, sums in ascending window order, rounded to float32 once.
dissent = the covering windows whose argmax (ties to the smaller state, NaN as -inf) is not the float32 output row's."""
import math

import numpy as np

MODES = ("prob", "logp", "select")
SHAPES = [(8, 3), (8, 8), (8, 1), (64, 32), (2000, 1000)]


# ------------------------------------------------------------------------------------------------ the window set
def windows(T, n, stride):
    """[(start, length)] in ascending start order, by walking: every regular window that fits, then the tail if the last one
    does not end at T."""
    if T <= n:
        return [(0, T)]
    out, s = [], 0
    while s + n <= T:
        out.append((s, n))
        s += stride
    if out[-1][0] + n != T:
        out.append((T - n, n))
    return out


def window_rows(T, n, stride):
    return sum(ln for _, ln in windows(T, n, stride))


def border_lengths(n, stride):
    """T around every border of the window set, each at least 1, without repeats."""
    out = []
    for T in (n - 1, n, n + 1, n + stride - 1, n + stride, n + stride + 1):
        if T >= 1 and T not in out:
            out.append(T)
    return out


def offsets(lens):
    return [0] + [int(v) for v in np.cumsum(lens)]


def layout(lens, n, stride, order=None, gap=0):
    """(win_first int64 (count,), win_steps): the recordings' blocks laid in the arena in ``order`` (a permutation of the list;
    default the list's order), ``gap`` unused rows in front of every block."""
    order = list(range(len(lens))) if order is None else list(order)
    first, row = np.zeros(len(lens), dtype=np.int64), 0
    for i in order:
        row += gap
        first[i] = row
        row += window_rows(lens[i], n, stride)
    return first, row


def list_lens(count, n, stride, seed=0):
    """``count`` lengths: the borders first, then lengths between 1 and 2 n + 5."""
    g = np.random.default_rng(1000 * count + seed)
    lens = border_lengths(n, stride)[:count]
    return lens + [int(v) for v in g.integers(1, 2 * n + 6, size=count - len(lens))]


# ------------------------------------------------------------------------------------------------ inputs
def rows(count, seed):
    """(count, 4) float32 log-softmax rows of random logits."""
    g = np.random.default_rng(seed)
    z = 3.0 * g.standard_normal((count, 4))
    z -= z.max(axis=1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(np.float32)


def weights(kind, n):
    """None, or (n,) float32: the package's window_weights, restated."""
    p = np.arange(n, dtype=np.float64)
    if kind is None:
        return None
    if kind == "triangular":
        return np.minimum(p + 1, n - p).astype(np.float32)
    if kind == "hann":
        return (np.sin(np.pi * (p + 0.5) / n) ** 2).astype(np.float32)
    if kind == "flat":
        return np.ones(n, dtype=np.float32)
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------ the restatement
def argmax4(v):
    """(.., 4) -> the argmax with NaN read as -inf and ties to the smaller state."""
    return np.argmax(np.where(np.isnan(v), -np.inf, v.astype(np.float64)), axis=-1)


def restate(win, first, lens, n, stride, w, mode):
    """-> {"out": (sum T, 4) float32, "pooled": (sum T, 4) float64 (the values before rounding; of a copied row its values),
    "copied": (sum T,) bool (one covering window, or "select": bit for bit), "cover": (sum T,) int, "dissent": (sum T,) uint8}."""
    assert mode in MODES
    win = np.ascontiguousarray(win, dtype=np.float32)
    offs = offsets(lens)
    total = offs[-1]
    res = {"out": np.zeros((total, 4), dtype=np.float32), "pooled": np.zeros((total, 4)), "copied": np.zeros(total, dtype=bool),
           "cover": np.zeros(total, dtype=np.int64), "dissent": np.zeros(total, dtype=np.uint8)}
    with np.errstate(all="ignore"):
        for r, T in enumerate(lens):
            ws = windows(T, n, stride)
            # slot k of step t: its k-th covering window in ascending start order
            cnt = np.zeros(T, dtype=np.int64)
            for s, ln in ws:
                cnt[s:s + ln] += 1
            m = int(cnt.max())
            V = np.zeros((m, T, 4), dtype=np.float32)
            Wt = np.zeros((m, T))
            valid = np.zeros((m, T), dtype=bool)
            cnt[:] = 0
            row = int(first[r])
            for s, ln in ws:
                t = np.arange(s, s + ln)
                k = cnt[t]
                V[k, t] = win[row:row + ln]
                Wt[k, t] = 1.0 if w is None else w[:ln].astype(np.float64)
                valid[k, t] = True
                cnt[t] += 1
                row += ln
            V64 = V.astype(np.float64)
            pick = np.argmax(np.where(valid, Wt, -np.inf), axis=0)                   # (the first maximum: the earlier window)
            chosen = V[pick, np.arange(T)]
            copied = (cnt == 1) | (mode == "select")
            a = np.zeros((T, 4))
            wsum = np.zeros(T)
            if mode == "prob":
                M = np.fmax.reduce(np.fmax.reduce(np.where(valid[:, :, None], V64, -np.inf), axis=2), axis=0)
                for k in range(m):
                    wsum = wsum + np.where(valid[k], Wt[k], 0.0)
                    a = a + np.where(valid[k][:, None], Wt[k][:, None] * np.exp(V64[k] - M[:, None]), 0.0)
                a = np.log(a / wsum[:, None]) + M[:, None]
            else:
                for k in range(m):
                    wsum = wsum + np.where(valid[k], Wt[k], 0.0)
                    a = a + np.where(valid[k][:, None], Wt[k][:, None] * V64[k], 0.0)
                a = a / wsum[:, None]
            top = np.fmax.reduce(a, axis=1)
            top = np.where(np.isnan(top), -np.inf, top)
            e = np.exp(a - top[:, None])
            lse = top + np.log(((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3])
            pooled = a - lse[:, None]
            out = np.where(copied[:, None], chosen, pooled.astype(np.float32))
            own = argmax4(out)
            dissent = (valid & (argmax4(V) != own[None, :])).sum(axis=0)
            sl = slice(offs[r], offs[r + 1])
            res["out"][sl] = out
            res["out"][sl][copied] = chosen[copied]          # (bit for bit: np.where may quieten a NaN)
            res["pooled"][sl] = np.where(copied[:, None], chosen.astype(np.float64), pooled)
            res["copied"][sl], res["cover"][sl], res["dissent"][sl] = copied, cnt, dissent
    return res


# ------------------------------------------------------------------------------------------------ brute force, per step
def _exp(x):
    if x != x:
        return math.nan
    return math.inf if x == math.inf else 0.0 if x == -math.inf else math.exp(x)


def _log(x):
    if x != x or x < 0:
        return math.nan
    return -math.inf if x == 0 else math.inf if x == math.inf else math.log(x)


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sub(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) - np.float64(b))


def _argmax(v):
    v = [-math.inf if x != x else x for x in v]
    return v.index(max(v))


def brute_force(win, first, lens, n, stride, w, mode):
    """The same quantities from a loop over every step and every window of its recording, in Python floats."""
    offs = offsets(lens)
    out = np.zeros((offs[-1], 4), dtype=np.float32)
    pooled = np.zeros((offs[-1], 4))
    cover = np.zeros(offs[-1], dtype=np.int64)
    dissent = np.zeros(offs[-1], dtype=np.uint8)
    for r, T in enumerate(lens):
        ws = windows(T, n, stride)
        for t in range(T):
            got, row = [], int(first[r])
            for s, ln in ws:                               # (ascending start)
                if s <= t < s + ln:
                    got.append((win[row + t - s], 1.0 if w is None else float(w[t - s])))
                row += ln
            at = offs[r] + t
            cover[at] = len(got)
            if len(got) == 1 or mode == "select":
                best = 0
                for k in range(1, len(got)):
                    if got[k][1] > got[best][1]:
                        best = k
                out[at] = got[best][0]
                pooled[at] = got[best][0].astype(np.float64)
            else:
                wsum = 0.0
                for _, wk in got:
                    wsum += wk
                a = []
                if mode == "prob":
                    vals = [float(x) for v, _ in got for x in v if x == x]
                    M = max(vals) if vals else -math.inf
                    for j in range(4):
                        s_ = 0.0
                        for v, wk in got:
                            s_ += wk * _exp(_sub(float(v[j]), M))
                        a.append(_log(_div(s_, wsum)) + M)
                else:
                    for j in range(4):
                        s_ = 0.0
                        for v, wk in got:
                            s_ += wk * float(v[j])
                        a.append(_div(s_, wsum))
                fin = [x for x in a if x == x]
                top = max(fin) if fin else -math.inf
                tot = 0.0
                for x in a:
                    tot += _exp(_sub(x, top))
                lse = top + _log(tot)
                pooled[at] = [_sub(x, lse) for x in a]
                with np.errstate(all="ignore"):
                    out[at] = pooled[at].astype(np.float32)
            own = _argmax([float(x) for x in out[at]])
            dissent[at] = sum(1 for v, _ in got if _argmax([float(x) for x in v]) != own)
    return {"out": out, "pooled": pooled, "cover": cover, "dissent": dissent}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def same_values(a, b):
    """Equal, with NaN equal to NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


def within(a, b, tol):
    """|a - b| <= tol where both are finite; equal (NaN as NaN, infinities by sign) elsewhere."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    return bool(same_values(np.where(fin, 0.0, a), np.where(fin, 0.0, b)) and (np.abs(a[fin] - b[fin]) <= np.broadcast_to(tol, a.shape)[fin]).all())


# ------------------------------------------------------------------------------------------------ special values
def special_case():
    """One recording of 14 steps under (n, stride) = (8, 3) -- windows [0, 8), [3, 11), [6, 14): steps 0..2 and 11..13 have one
    covering window, 3..5 and 8..10 two, 6..7 three -- with every special value of the contract placed by step:
      4   class 2 is -inf in both covering windows             9   class 1 is -inf in one of two
      6   a NaN in one of three covering windows               1   a NaN in the step's only window
      8   all four classes -inf in both windows                5   two windows with the same row, classes 0 and 1 tied at the top
      10  one window votes class 0, the other class 3, with mirrored rows: the pooled row ties 0 and 3
    -> (win (24, 4) float32, first, lens)."""
    n, stride, T = 8, 3, 14
    win = rows(24, 77)
    ws = windows(T, n, stride)
    assert ws == [(0, 8), (3, 8), (6, 8)]

    def at(k, t):
        return 8 * k + t - ws[k][0]
    ninf = np.float32(-np.inf)
    win[at(0, 4), 2] = win[at(1, 4), 2] = ninf
    win[at(1, 9), 1] = ninf
    win[at(1, 6), 3] = np.nan
    win[at(0, 1), 0] = np.nan
    win[at(1, 8)] = win[at(2, 8)] = ninf
    tie = np.log(np.array([0.4, 0.4, 0.15, 0.05])).astype(np.float32)
    win[at(0, 5)] = win[at(1, 5)] = tie
    row = np.log(np.array([0.6, 0.1, 0.1, 0.2])).astype(np.float32)
    win[at(1, 10)], win[at(2, 10)] = row, row[::-1]
    return win, np.zeros(1, dtype=np.int64), [T]
