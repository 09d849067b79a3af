"""The forward-backward kernel's specification restated in numpy float64 (include/hssfsst.h: hssfsst_posteriors), with no import
from the package: the linear-domain recursion on b = exp(e - max e), P = exp(A), p0 = exp(pi), every running vector a float64
mantissa with an integer exponent renormalised by an exact power of two after every step (frexp / ldexp), NaN emissions as -inf,
Z = 0 as logZ = -inf and gamma = Xi = 0.  Several sequences are walked at once (axis 0), each with its own tables; a sequence
past its own end is frozen.  Next to it, what the restatement itself is checked against: brute-force enumeration of all 4^T paths,
an np.longdouble log-space forward-backward, and a differentiable torch float64 log-space loop (the CPU twin of sequence_nll)."""
import itertools

import numpy as np
import torch

NINF = -np.inf
LN2 = float(np.log(2.0))


def _f64(v):
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def _renorm(a):
    """a (N, ...) >= 0 -> (a / 2^k, k) with 2^k the power of two just above each row's largest entry (k = 0 for a zero row)."""
    top = a.reshape(a.shape[0], -1).max(axis=1)
    k = np.where(top > 0, np.frexp(np.where(top > 0, top, 1.0))[1], 0).astype(np.int64)
    return np.ldexp(a, -k.reshape((-1,) + (1,) * (a.ndim - 1)).astype(np.int32)), k


def forward_backward(es, As, pis):
    """es: list of (T_n, 4) float32; As: list of (4, 4); pis: list of (4,).  Returns (list of (T_n, 4) float64 gamma, logZ (N,),
    Xi (N, 4, 4))."""
    N = len(es)
    lens = np.array([e.shape[0] for e in es], dtype=np.int64)
    Tm = int(lens.max())
    E = np.full((N, Tm, 4), 0.0)
    for n, e in enumerate(es):
        v = _f64(e)
        E[n, :lens[n]] = np.where(np.isnan(v), NINF, v)
    top = E.max(axis=2)
    dead = np.isneginf(top)
    top = np.where(dead, 0.0, top)
    with np.errstate(invalid="ignore"):
        b = np.where(dead[:, :, None], 0.0, np.exp(E - top[:, :, None]))
    P = np.exp(np.stack([_f64(a) for a in As]))
    p0 = np.exp(np.stack([_f64(p) for p in pis]))
    alpha = np.zeros((N, Tm, 4))
    a, expo = _renorm(p0 * b[:, 0])
    alpha[:, 0] = a
    for t in range(1, Tm):
        new, k = _renorm(np.einsum("ni,nij->nj", a, P) * b[:, t])
        live = t < lens
        a = np.where(live[:, None], new, a)
        expo = expo + np.where(live, k, 0)
        alpha[:, t] = a
    z = a.sum(axis=1)
    max_sum = np.array([top[n, :lens[n]].sum() for n in range(N)])
    with np.errstate(divide="ignore"):
        logz = np.where(z > 0, np.log(np.where(z > 0, z, 1.0)) + expo * LN2 + max_sum, NINF)
    beta = np.ones((N, 4))
    gamma = np.zeros((N, Tm, 4))
    xi = np.zeros((N, 4, 4))
    for t in range(Tm - 1, -1, -1):
        live = t < lens
        g = alpha[:, t] * beta
        s = g.sum(axis=1)
        gamma[:, t] = np.where((live & (s > 0))[:, None], g / np.where(s > 0, s, 1.0)[:, None], 0.0)
        if t == 0:
            break
        w = b[:, t] * beta
        num = alpha[:, t - 1, :, None] * P * w[:, None, :]
        s = num.sum(axis=(1, 2))
        xi += np.where((live & (s > 0))[:, None, None], num / np.where(s > 0, s, 1.0)[:, None, None], 0.0)
        new, _ = _renorm(np.einsum("nij,nj->ni", P, w))
        beta = np.where(live[:, None], new, beta)
    return [gamma[n, :lens[n]].copy() for n in range(N)], logz, xi


def path_score(e, A, pi, path):
    """w(path) in float64 on the float32 inputs; NaN emissions count as -inf."""
    e, A, pi = _f64(e), _f64(A), _f64(pi)
    e = np.where(np.isnan(e), NINF, e)
    p = np.asarray(path).astype(np.int64)
    return pi[p[0]] + e[np.arange(len(p)), p].sum() + A[p[:-1], p[1:]].sum()


def label_counts(path):
    c = np.zeros((4, 4))
    p = np.asarray(path).astype(np.int64)
    np.add.at(c, (p[:-1], p[1:]), 1.0)
    return c


def brute_force(e, A, pi):
    """All 4^T paths (T <= 6): (gamma (T, 4), logZ, Xi (4, 4)) in float64."""
    T = e.shape[0]
    paths = np.array(list(itertools.product(range(4), repeat=T)), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        w = np.array([path_score(e, A, pi, p) for p in paths])
    top = w.max()
    if np.isneginf(top):
        return np.zeros((T, 4)), NINF, np.zeros((4, 4))
    pr = np.exp(w - top)
    logz = top + np.log(pr.sum())
    pr = pr / pr.sum()
    gamma = np.zeros((T, 4))
    xi = np.zeros((4, 4))
    for p, q in zip(paths, pr):
        gamma[np.arange(T), p] += q
        np.add.at(xi, (p[:-1], p[1:]), q)
    return gamma, logz, xi


def _lse(x, axis):
    top = x.max(axis=axis, keepdims=True)
    safe = np.where(np.isneginf(top), 0, top)
    with np.errstate(divide="ignore"):
        return (safe + np.log(np.exp(x - safe).sum(axis=axis, keepdims=True))).squeeze(axis)


def longdouble_forward_backward(e, A, pi):
    """The log-space forward-backward in np.longdouble: (gamma (T, 4), logZ) as longdouble."""
    ld = np.longdouble
    e, A, pi = _f64(e).astype(ld), _f64(A).astype(ld), _f64(pi).astype(ld)
    T = e.shape[0]
    la = np.zeros((T, 4), dtype=ld)
    lb = np.zeros((T, 4), dtype=ld)
    la[0] = pi + e[0]
    for t in range(1, T):
        la[t] = _lse(la[t - 1][:, None] + A, 0) + e[t]
    for t in range(T - 1, 0, -1):
        lb[t - 1] = _lse(A + (e[t] + lb[t])[None, :], 1)
    logz = _lse(la[T - 1], 0)
    return np.exp(la + lb - logz), logz


def torch_log_z(e, A, pi):
    """logZ of one sequence by a differentiable float64 log-space loop on the CPU: e (T, 4), A (4, 4), pi (4,) float64 tensors."""
    a = pi + e[0]
    for t in range(1, e.shape[0]):
        a = torch.logsumexp(a[:, None] + A, dim=0) + e[t]
    return torch.logsumexp(a, dim=0)


def torch_nll(e, labels, A, pi):
    """logZ - score(labels) of one sequence: the CPU twin of sequence_nll (float64, differentiable)."""
    y = torch.as_tensor(labels, dtype=torch.int64)
    score = pi[y[0]] + e[torch.arange(e.shape[0]), y].sum() + A[y[:-1], y[1:]].sum()
    return torch_log_z(e, A, pi) - score


def legal_labels(T, rng, A=None):
    """A label sequence of T steps that `A` allows (default: the cardiac cycle): random run lengths, a random start."""
    if A is None:
        s, out = int(rng.integers(0, 4)), []
        while len(out) < T:
            out += [s] * int(rng.integers(1, 9))
            s = (s + 1) % 4
        return np.array(out[:T], dtype=np.uint8)
    ok = np.isfinite(np.asarray(A))
    s = int(rng.integers(0, 4))
    out = [s]
    for _ in range(T - 1):
        s = int(rng.choice(np.flatnonzero(ok[s])))
        out.append(s)
    return np.array(out, dtype=np.uint8)
