"""The expected run-length counts of the explicit-duration model (include/hssfsst.h: hssfsst_posteriors_durations_counts;
csrc/duration_counts_layout.hpp) restated in numpy on tests/duration_posterior_cases.py's scaled scalars, with no import from the
package: counts[0 interior, 1 edge][j][d - 1] = sum_t b_t(j) L(j, d) g_(t+d)(j) / Z, vectorised over t (so the ORDER of a sum is
numpy's, not the kernel's: the two agree to rounding, not bit for bit).  Next to it, what the restatement is checked against:
brute-force enumeration of every segmentation and an np.longdouble log-space twin."""
import numpy as np

from tests import duration_posterior_cases as dpc

NINF = -np.inf


def sweeps(e, A, pi, dur, edge):
    """duration_posterior_cases.forward_backward's two recurrences, kept: b (T, 4), g (T + 1, 4; row 0 unused) and 1 / Z as
    (mantissa, exponent) pairs, the linear tables Ld, Le, and logZ."""
    em = dpc.emissions64(e)
    T, D = em.shape[0], np.asarray(dur).shape[1]
    P, p0, Ld, Le = dpc._tables(A, pi, dur, edge)
    E = np.zeros((T + 1, 4))
    np.cumsum(em, axis=0, out=E[1:])

    def ratio(t):                                        # [i, j] = exp(E_i(t) - E_j(t))
        return dpc.sexp(E[t][:, None] - E[t][None, :])
    bm, be = np.zeros((T, 4)), np.full((T, 4), dpc.ZERO_EXP, dtype=np.int64)
    cm, ce = np.zeros((T + 1, 4)), np.full((T + 1, 4), dpc.ZERO_EXP, dtype=np.int64)
    bm[0], be[0] = p0
    for t in range(1, T + 1):
        m = min(D, t)
        Lm, Lx = (Le[0][:, :m], Le[1][:, :m]) if t == T else (Ld[0][:, :m].copy(), Ld[1][:, :m].copy())
        if m == t and t != T:
            Lm[:, t - 1], Lx[:, t - 1] = Le[0][:, t - 1], Le[1][:, t - 1]
        src = (bm[t - m:t][::-1].T, be[t - m:t][::-1].T)          # [j, d - 1]
        cm[t], ce[t] = dpc.snorm(dpc.ssum(dpc.smul(src, (Lm, Lx)), axis=1))
        if t < T:
            via = dpc.smul(dpc.smul((cm[t][:, None], ce[t][:, None]), ratio(t)), P)      # [i, j]
            bm[t], be[t] = dpc.snorm(dpc.ssum(via, axis=0))
    Z = dpc.snorm(dpc.ssum(dpc.smul((cm[T], ce[T]), dpc.sexp(E[T])), axis=0))
    logz = float(np.log(Z[0]) + Z[1] * dpc.LN2) if Z[0] > 0 else NINF
    invz = dpc.snorm((np.float64(1.0 / Z[0]), -Z[1])) if Z[0] > 0 else (np.float64(0.0), np.int64(dpc.ZERO_EXP))
    gm, ge = np.zeros((T + 1, 4)), np.full((T + 1, 4), dpc.ZERO_EXP, dtype=np.int64)
    gm[T], ge[T] = dpc.sexp(E[T])
    for t in range(T - 1, 0, -1):
        m = min(D, T - t)
        Lm, Lx = Ld[0][:, :m].copy(), Ld[1][:, :m].copy()
        if t + m == T:
            Lm[:, m - 1], Lx[:, m - 1] = Le[0][:, m - 1], Le[1][:, m - 1]
        src = (gm[t + 1:t + m + 1].T, ge[t + 1:t + m + 1].T)
        cb = dpc.snorm(dpc.ssum(dpc.smul(src, (Lm, Lx)), axis=1))
        gm[t], ge[t] = dpc.snorm(dpc.ssum(dpc.smul(dpc.smul((cb[0][None, :], cb[1][None, :]), ratio(t)), P), axis=1))
    return dict(b=(bm, be), g=(gm, ge), invz=invz, Ld=Ld, Le=Le, logz=logz)


def run_counts(e, A, pi, dur, edge):
    """e (T, 4), A (4, 4) (diagonal ignored), pi (4,), dur, edge (4, D) -> counts (2, 4, D) float64: [0] the expected number of
    interior runs of state j lasting d steps, [1] of first and last runs.  Vectorised over t, one duration at a time."""
    s = sweeps(e, A, pi, dur, edge)
    T, D = np.asarray(e).shape[0], np.asarray(dur).shape[1]
    (bm, be), (gm, ge), invz = s["b"], s["g"], s["invz"]
    out = np.zeros((2, 4, D))
    for d in range(1, min(D, T) + 1):
        n = T - d + 1                                    # starts t = 0 .. T - d, ends t + d = d .. T
        w = dpc.smul((bm[:n], be[:n]), (gm[d:d + n], ge[d:d + n]))                   # [t, j]
        lz = [dpc.smul((L[0][:, d - 1], L[1][:, d - 1]), invz) for L in (s["Ld"], s["Le"])]
        at_edge = np.zeros(n, dtype=bool)
        at_edge[0] = at_edge[n - 1] = True
        inner = dpc.sval(dpc.smul(w, (lz[0][0][None, :], lz[0][1][None, :])))
        outer = dpc.sval(dpc.smul(w, (lz[1][0][None, :], lz[1][1][None, :])))
        out[0, :, d - 1] = inner[~at_edge].sum(axis=0)
        out[1, :, d - 1] = outer[at_edge].sum(axis=0)
    return out


def label_run_counts(labels, D):
    """(2, 4, D): the runs of a label sequence, the first and the last in [1]; a run longer than D is left out."""
    out = np.zeros((2, 4, D))
    runs = dpc.runs_of(labels)
    for k, (s, d) in enumerate(runs):
        if d <= D:
            out[1 if k in (0, len(runs) - 1) else 0, s & 3, d - 1] += 1.0
    return out


def brute_force_counts(e, A, pi, dur, edge):
    """All segmentations (T <= 7 or so): (counts (2, 4, D), P(one run)) in float64; zeros where nothing fits."""
    em, A, pi, dur, edge = dpc.emissions64(e), dpc._f64(A), dpc._f64(pi), dpc._f64(dur), dpc._f64(edge)
    T, D = em.shape[0], dur.shape[1]
    found = []
    with np.errstate(invalid="ignore"):
        for runs in dpc.segmentations(T, D):
            w, t = pi[runs[0][0]], 0
            for k, (s, d) in enumerate(runs):
                w += (edge if k in (0, len(runs) - 1) else dur)[s, d - 1] + em[t:t + d, s].sum()
                if k:
                    w += A[runs[k - 1][0], s]
                t += d
            if np.isfinite(w):
                found.append((float(w), runs))
    out, one = np.zeros((2, 4, D)), 0.0
    if not found:
        return out, one
    w = np.array([f[0] for f in found])
    pr = np.exp(w - w.max())
    pr = pr / pr.sum()
    for q, (_, runs) in zip(pr, found):
        for k, (s, d) in enumerate(runs):
            out[1 if k in (0, len(runs) - 1) else 0, s, d - 1] += q
        if len(runs) == 1:
            one += q
    return out, one


def longdouble_run_counts(e, A, pi, dur, edge):
    """The recurrences in natural logs in np.longdouble (duration_posterior_cases.longdouble_forward_backward's), and the counts as
    sums of exp(b_t + L + g_(t+d) - logZ) over t: (2, 4, D) longdouble."""
    ld = np.longdouble
    em, A, pi, dur, edge = (np.asarray(v).astype(ld) for v in (dpc.emissions64(e), dpc._f64(A), dpc._f64(pi), dpc._f64(dur), dpc._f64(edge)))
    T, D = em.shape[0], dur.shape[1]
    A = A.copy()
    A[np.arange(4), np.arange(4)] = NINF
    E = np.zeros((T + 1, 4), dtype=ld)
    np.cumsum(em, axis=0, out=E[1:])
    b, c = np.full((T, 4), NINF, dtype=ld), np.full((T + 1, 4), NINF, dtype=ld)
    b[0] = pi
    out = np.zeros((2, 4, D), dtype=ld)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(1, T + 1):
            m = min(D, t)
            L = edge[:, :m] if t == T else dur[:, :m].copy()
            if m == t and t != T:
                L[:, t - 1] = edge[:, t - 1]
            c[t] = dpc._lse(b[t - m:t][::-1].T + L, 1)
            if t < T:
                b[t] = dpc._lse((c[t] + E[t])[:, None] + A, 0) - E[t]
        logz = dpc._lse(c[T] + E[T], 0)
        if np.isneginf(logz):
            return out
        g = np.full((T + 1, 4), NINF, dtype=ld)
        g[T] = E[T]
        for t in range(T - 1, 0, -1):
            m = min(D, T - t)
            L = dur[:, :m].copy()
            if t + m == T:
                L[:, m - 1] = edge[:, m - 1]
            cb = dpc._lse(g[t + 1:t + m + 1].T + L, 1)
            g[t] = dpc._lse(A + (cb - E[t])[None, :], 1) + E[t]
        for d in range(1, min(D, T) + 1):
            n = T - d + 1
            w = b[:n] + g[d:d + n] - logz                # [t, j]
            at_edge = np.zeros(n, dtype=bool)
            at_edge[0] = at_edge[n - 1] = True
            out[0, :, d - 1] = np.exp(w[~at_edge] + dur[None, :, d - 1]).sum(axis=0)
            out[1, :, d - 1] = np.exp(w[at_edge] + edge[None, :, d - 1]).sum(axis=0)
    return out
