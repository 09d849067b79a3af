"""The explicit-duration forward-backward kernel's specification restated in numpy (include/hssfsst.h:
hssfsst_posteriors_durations; csrc/duration_posterior_layout.hpp), with no import from the package: every quantity a float64
mantissa with an integer exponent, exp(x) as (exp2(frac), floor) of x / ln 2, sums aligned with ldexp -- vectorised over the
duration d, so the ORDER of a ring word's additions is numpy's, not the kernel's: the two agree to rounding, not bit for bit.
Next to it, what the restatement is checked against: brute-force enumeration of every segmentation, an np.longdouble log-space twin
of the recurrence, and a differentiable torch float64 log-space loop (the CPU twin of duration_nll)."""
import numpy as np
import torch

NINF = -np.inf
LN2 = float(np.log(2.0))
LOG2E = 1.44269504088896340735992468100
FLOOR = -32768.0                                         # what an emission of -inf or NaN counts as
ZERO_EXP = -(1 << 30)


def _f64(v):
    v = np.asarray(v)
    return (v.astype(np.float32) if v.dtype != np.float64 else v).astype(np.float64)


def emissions64(e):
    """float32 emissions (float64 ones are taken as they are: for finite differences) -> float64 with -inf and NaN at -32768."""
    e = _f64(e)
    return np.where(np.isnan(e) | np.isneginf(e), FLOOR, e)


# ---- scaled scalars: (m, e) arrays, value m x 2^e, m == 0 is zero
def sexp(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        live = x >= -1.0e300
    y = np.where(live, x, 0.0) * LOG2E
    f = np.floor(y)
    return np.where(live, 0.5 * np.exp2(y - f), 0.0), np.where(live, f.astype(np.int64) + 1, ZERO_EXP)


def snorm(a):
    m, e = a
    live = m > 0
    mm, k = np.frexp(np.where(live, m, 1.0))
    return np.where(live, mm, 0.0), np.where(live, e + k, ZERO_EXP)


def smul(a, b):
    m = a[0] * b[0]
    return m, np.where(m > 0, a[1] + b[1], ZERO_EXP)


def ssum(a, axis):
    m, e = a
    live = m > 0
    top = np.where(live, e, np.iinfo(np.int64).min).max(axis=axis, keepdims=True)
    shift = np.clip(np.where(live, e - top, 0), -4000, 0).astype(np.int32)
    s = np.where(live, np.ldexp(m, shift), 0.0).sum(axis=axis)
    return s, np.where(s > 0, top.squeeze(axis), ZERO_EXP)


def sval(a):
    return np.where(a[0] > 0, np.ldexp(a[0], np.clip(a[1], -4000, 4000).astype(np.int32)), 0.0)


def _tables(A, pi, dur, edge):
    P = list(sexp(_f64(A)))
    P[0] = P[0].copy()
    P[0][np.arange(4), np.arange(4)] = 0.0               # a run is never followed by the same state
    return tuple(P), sexp(_f64(pi)), sexp(_f64(dur)), sexp(_f64(edge))


def runs_of(path):
    p = np.asarray(path).astype(np.int64)
    cut = np.flatnonzero(np.diff(p)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(p)]])
    return [(int(p[a]), int(b - a)) for a, b in zip(starts, ends)]


def label_score(e, A, pi, dur, edge, labels):
    """The labelled segmentation's log weight in float64, its terms added in the kernel's order; -inf where forbidden."""
    em, A, pi, dur, edge = emissions64(e), _f64(A), _f64(pi), _f64(dur), _f64(edge)
    y = np.asarray(labels).astype(np.int64) & 3
    T, D = len(y), dur.shape[1]
    s, start = float(pi[y[0]]), 0
    with np.errstate(invalid="ignore"):
        for r in range(T):
            s += em[r, y[r]]
            if r + 1 == T or y[r + 1] != y[r]:
                d = r + 1 - start
                s += NINF if d > D else (edge if start == 0 or r + 1 == T else dur)[y[r], d - 1]
                if r + 1 < T:
                    s += A[y[r], y[r + 1]]
                start = r + 1
    return float(s)


def label_counts(labels):
    """counts[i][j] of the run changes i -> j of a label sequence (no diagonal)."""
    c = np.zeros((4, 4))
    p = np.asarray(labels).astype(np.int64) & 3
    ch = np.flatnonzero(p[1:] != p[:-1])
    np.add.at(c, (p[ch], p[ch + 1]), 1.0)
    return c


def forward_backward(e, A, pi, dur, edge):
    """e (T, 4), A (4, 4) (diagonal ignored), pi (4,), dur, edge (4, D).  Returns a dict: gamma (T, 4) float64 clamped to [0, 1],
    logz, xi (4, 4), onsets (T, 4), s0 (4,) -- and the unclamped sums the further checks look at: ends (T + 1, 4) with ends[t] = N_t."""
    em = emissions64(e)
    T, D = em.shape[0], np.asarray(dur).shape[1]
    P, p0, Ld, Le = _tables(A, pi, dur, edge)
    E = np.zeros((T + 1, 4))
    np.cumsum(em, axis=0, out=E[1:])
    rat = [sexp(E[t][:, None] - E[t][None, :]) for t in range(T + 1)] if T <= 64 else None

    def ratio(t):                                        # [i, j] = exp(E_i(t) - E_j(t))
        return rat[t] if rat is not None else sexp(E[t][:, None] - E[t][None, :])
    bm, be = np.zeros((T, 4)), np.full((T, 4), ZERO_EXP, dtype=np.int64)
    cm, ce = np.zeros((T + 1, 4)), np.full((T + 1, 4), ZERO_EXP, dtype=np.int64)
    bm[0], be[0] = p0
    for t in range(1, T + 1):
        m = min(D, t)
        Lm, Lx = (Le[0][:, :m], Le[1][:, :m]) if t == T else (Ld[0][:, :m].copy(), Ld[1][:, :m].copy())
        if m == t and t != T:
            Lm[:, t - 1], Lx[:, t - 1] = Le[0][:, t - 1], Le[1][:, t - 1]
        src = (bm[t - m:t][::-1].T, be[t - m:t][::-1].T)          # [j, d - 1]
        cm[t], ce[t] = snorm(ssum(smul(src, (Lm, Lx)), axis=1))
        if t < T:
            via = smul(smul((cm[t][:, None], ce[t][:, None]), ratio(t)), P)      # [i, j]
            bm[t], be[t] = snorm(ssum(via, axis=0))
    Z = snorm(ssum(smul((cm[T], ce[T]), sexp(E[T])), axis=0))
    logz = float(np.log(Z[0]) + Z[1] * LN2) if Z[0] > 0 else NINF
    invz = snorm((np.float64(1.0 / Z[0]), -Z[1])) if Z[0] > 0 else (np.float64(0.0), np.int64(ZERO_EXP))
    gm, ge = np.zeros((T + 1, 4)), np.full((T + 1, 4), ZERO_EXP, dtype=np.int64)
    gm[T], ge[T] = sexp(E[T])
    xi, onsets, ends = np.zeros((4, 4)), np.zeros((T, 4)), np.zeros((T + 1, 4))
    ends[T] = sval(smul(smul((cm[T], ce[T]), (gm[T], ge[T])), invz))
    for t in range(T - 1, -1, -1):
        m = min(D, T - t)
        Lm, Lx = (Le[0][:, :m], Le[1][:, :m]) if t == 0 else (Ld[0][:, :m].copy(), Ld[1][:, :m].copy())
        if t + m == T and t != 0:
            Lm[:, m - 1], Lx[:, m - 1] = Le[0][:, m - 1], Le[1][:, m - 1]
        src = (gm[t + 1:t + m + 1].T, ge[t + 1:t + m + 1].T)
        cb = snorm(ssum(smul(src, (Lm, Lx)), axis=1))
        if t == 0:
            onsets[0] = sval(smul(smul(p0, cb), invz))
            break
        r = ratio(t)
        gm[t], ge[t] = snorm(ssum(smul(smul((cb[0][None, :], cb[1][None, :]), r), P), axis=1))
        x = sval(smul(smul(smul(smul((cm[t][:, None], ce[t][:, None]), r), P), (cb[0][None, :], cb[1][None, :])), invz))
        xi += x
        onsets[t] = x.sum(axis=0)
        ends[t] = sval(smul(smul((cm[t], ce[t]), (gm[t], ge[t])), invz))
    gamma = np.zeros((T, 4))
    g = ends[T].copy()
    gamma[T - 1] = g
    for t in range(T - 1, 0, -1):
        g = (g - onsets[t]) + ends[t]
        gamma[t - 1] = g
    return dict(gamma=np.clip(gamma, 0.0, 1.0), raw_gamma=gamma, logz=logz, xi=xi, onsets=onsets, s0=onsets[0].copy(), ends=ends)


def segmentations(T, D):
    """Every (state, duration) list with durations 1 .. D summing to T and no state twice in a row."""
    def walk(t, last):
        if t == T:
            yield []
            return
        for s in range(4):
            if s == last:
                continue
            for d in range(1, min(D, T - t) + 1):
                for rest in walk(t + d, s):
                    yield [(s, d)] + rest
    return walk(0, -1)


def brute_force(e, A, pi, dur, edge):
    """All segmentations (T <= 7 or so): dict of gamma (T, 4), logz, xi (4, 4), onsets (T, 4) in float64."""
    em, A, pi, dur, edge = emissions64(e), _f64(A), _f64(pi), _f64(dur), _f64(edge)
    T, D = em.shape[0], dur.shape[1]
    found = []
    with np.errstate(invalid="ignore"):
        for runs in segmentations(T, D):
            w, t = pi[runs[0][0]], 0
            for k, (s, d) in enumerate(runs):
                w += (edge if k in (0, len(runs) - 1) else dur)[s, d - 1] + em[t:t + d, s].sum()
                if k:
                    w += A[runs[k - 1][0], s]
                t += d
            if np.isfinite(w):
                found.append((float(w), runs))
    gamma, xi, onsets = np.zeros((T, 4)), np.zeros((4, 4)), np.zeros((T, 4))
    if not found:
        return dict(gamma=gamma, logz=NINF, xi=xi, onsets=onsets)
    w = np.array([f[0] for f in found])
    top = w.max()
    pr = np.exp(w - top)
    logz = float(top + np.log(pr.sum()))
    pr = pr / pr.sum()
    for q, (_, runs) in zip(pr, found):
        t = 0
        for k, (s, d) in enumerate(runs):
            gamma[t:t + d, s] += q
            onsets[t, s] += q
            if k:
                xi[runs[k - 1][0], s] += q
            t += d
    return dict(gamma=gamma, logz=logz, xi=xi, onsets=onsets)


def _lse(x, axis):
    top = x.max(axis=axis, keepdims=True)
    safe = np.where(np.isneginf(top), 0, top)
    with np.errstate(divide="ignore"):
        return (safe + np.log(np.exp(x - safe).sum(axis=axis, keepdims=True))).squeeze(axis)


def longdouble_forward_backward(e, A, pi, dur, edge):
    """The recurrence in natural logs in np.longdouble, the sums over d as one logsumexp: dict of gamma, logz, xi as longdouble."""
    ld = np.longdouble
    em, A, pi, dur, edge = (np.asarray(v).astype(ld) for v in (emissions64(e), _f64(A), _f64(pi), _f64(dur), _f64(edge)))
    T, D = em.shape[0], dur.shape[1]
    A = A.copy()
    A[np.arange(4), np.arange(4)] = NINF
    E = np.zeros((T + 1, 4), dtype=ld)
    np.cumsum(em, axis=0, out=E[1:])
    b, c = np.full((T, 4), NINF, dtype=ld), np.full((T + 1, 4), NINF, dtype=ld)
    b[0] = pi
    with np.errstate(invalid="ignore"):
        for t in range(1, T + 1):
            m = min(D, t)
            L = edge[:, :m] if t == T else dur[:, :m].copy()
            if m == t and t != T:
                L[:, t - 1] = edge[:, t - 1]
            c[t] = _lse(b[t - m:t][::-1].T + L, 1)
            if t < T:
                b[t] = _lse((c[t] + E[t])[:, None] + A, 0) - E[t]
        logz = _lse(c[T] + E[T], 0)
        g, cb = np.full((T + 1, 4), NINF, dtype=ld), np.full((T, 4), NINF, dtype=ld)
        g[T] = E[T]
        for t in range(T - 1, -1, -1):
            m = min(D, T - t)
            L = edge[:, :m] if t == 0 else dur[:, :m].copy()
            if t + m == T and t != 0:
                L[:, m - 1] = edge[:, m - 1]
            cb[t] = _lse(g[t + 1:t + m + 1].T + L, 1)
            if t:
                g[t] = _lse(A + (cb[t] - E[t])[None, :], 1) + E[t]
        S = np.exp(b + cb - logz)
        N = np.exp(c[1:] + g[1:] - logz)                 # N[t - 1] = N_t
        gamma = np.zeros((T, 4), dtype=ld)
        run = N[T - 1].copy()
        gamma[T - 1] = run
        for t in range(T - 1, 0, -1):
            run = run - S[t] + N[t - 1]
            gamma[t - 1] = run
        x = np.exp((c[1:T] + E[1:T])[:, :, None] + A[None] + (cb[1:T] - E[1:T])[:, None, :] - logz)
    return dict(gamma=gamma, logz=logz, xi=x.sum(axis=0), onsets=S)


# ---- the differentiable CPU twin: float64 torch, log space, O(T D)
def torch_log_z(e, A, pi, dur, edge):
    """logZ of one sequence: e (T, 4), A (4, 4), pi (4,), dur, edge (4, D) float64 tensors; every run start must be reachable (an
    all -inf logsumexp has no gradient)."""
    T, D = e.shape[0], dur.shape[1]
    em = torch.where(torch.isnan(e) | torch.isneginf(e), torch.full_like(e, FLOOR), e)
    E = torch.cat([torch.zeros((1, 4), dtype=e.dtype), torch.cumsum(em, dim=0)])
    Aoff = A.masked_fill(torch.eye(4, dtype=torch.bool), NINF)
    b = [pi]
    for t in range(1, T + 1):
        m = min(D, t)
        if t == T:
            L = edge[:, :m]
        else:
            L = torch.cat([dur[:, :m - 1], edge[:, m - 1:m]], dim=1) if m == t else dur[:, :m]
        c = torch.logsumexp(torch.stack(b[t - m:t]).flip(0) + L.T, dim=0)        # rows d = 1 .. m
        if t < T:
            b.append(torch.logsumexp((c + E[t])[:, None] + Aoff, dim=0) - E[t])
    return torch.logsumexp(c + E[T], dim=0)


def torch_score(e, labels, A, pi, dur, edge):
    em = torch.where(torch.isnan(e) | torch.isneginf(e), torch.full_like(e, FLOOR), e)
    y = torch.as_tensor(np.asarray(labels).astype(np.int64))
    runs = runs_of(np.asarray(labels))
    s = pi[runs[0][0]] + em[torch.arange(e.shape[0]), y].sum()
    for k, (st, d) in enumerate(runs):
        s = s + (edge if k in (0, len(runs) - 1) else dur)[st, d - 1]
        if k:
            s = s + A[runs[k - 1][0], st]
    return s


def torch_nll(e, labels, A, pi, dur, edge):
    """logZ - score(labels) of one sequence: the CPU twin of duration_nll (float64, differentiable in e, A, pi)."""
    return torch_log_z(e, A, pi, dur, edge) - torch_score(e, labels, A, pi, dur, edge)


def legal_labels(T, rng, D, lo=1):
    """A label sequence of T steps around the cardiac cycle with runs of lo .. min(D, lo + 7) steps, a random start."""
    s, out = int(rng.integers(0, 4)), []
    while len(out) < T:
        out += [s] * int(rng.integers(lo, min(D, lo + 7) + 1))
        s = (s + 1) % 4
    return np.array(out[:T], dtype=np.uint8)
