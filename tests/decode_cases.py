"""The decoder's specification restated in numpy (include/hssfsst.h: hssfsst_decode_states), with no import from the package:
the quantiser, the sequential loop over int64 with the absorbing NEG, the tie rules, the backtrace -- and the same loop in
float64 without quantisation, for the bound between the two.  Several sequences are walked at once (axis 0), each with its own
transitions; a sequence past its own end is frozen, so every sequence gets exactly its own loop."""
import numpy as np

NEG = np.iinfo(np.int64).min
FRAC = 20
NINF = -np.inf


def quantise(x):
    """q(x) = rint(clamp(x, -32768, 32768) * 2^20), half to even (np.rint); q(NaN) = q(-32768); q(-inf) = NEG; +inf clamps."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    forbidden = np.isneginf(x)
    x = np.where(np.isnan(x), -32768.0, x)
    q = np.rint(np.clip(x, -32768.0, 32768.0) * float(1 << FRAC)).astype(np.int64)
    return np.where(forbidden, NEG, q)


def _add_exact(a, b):
    with np.errstate(over="ignore"):
        return np.where((a == NEG) | (b == NEG), NEG, a + b)


def cyclic():
    A = np.full((4, 4), NINF, dtype=np.float32)
    for i in range(4):
        A[i, i] = 0.0
        A[i, (i + 1) % 4] = 0.0
    return A


def viterbi(es, As, pis, exact=True):
    """es: list of (T_n, 4) float32; As: list of (4, 4); pis: list of (4,).  Returns (list of (T_n,) uint8 paths, scores): int64
    scores in units of 2^-20 when exact, else float64 scores of the unquantised float64 recurrence (same tie rules)."""
    N = len(es)
    lens = np.array([e.shape[0] for e in es], dtype=np.int64)
    Tm = int(lens.max())
    if exact:
        add, conv, pad = _add_exact, quantise, 0
    else:
        add, conv, pad = (lambda a, b: a + b), (lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)), 0.0
    E = np.full((N, Tm, 4), pad, dtype=np.int64 if exact else np.float64)
    for n, e in enumerate(es):
        E[n, :lens[n]] = conv(e)
    A = np.stack([conv(a) for a in As])                  # (N, 4, 4)
    d = add(np.stack([conv(p) for p in pis]), E[:, 0])   # (N, 4)
    psi = np.zeros((N, Tm, 4), dtype=np.uint8)
    for t in range(1, Tm):
        cand = add(d[:, :, None], A)                     # [n, i, j]
        best = cand.max(axis=1)
        arg = cand.argmax(axis=1)                        # the first, i.e. smallest, i that attains the max
        live = (t < lens)[:, None]
        d = np.where(live, add(best, E[:, t]), d)
        psi[:, t] = arg
    scores = d.max(axis=1)
    s = d.argmax(axis=1)                                 # the smallest j that attains the max
    paths = np.zeros((N, Tm), dtype=np.uint8)
    rows = np.arange(N)
    for t in range(Tm - 1, 0, -1):
        live = t < lens
        paths[:, t] = np.where(live, s, 0)
        s = np.where(live, psi[rows, t, s], s)
    paths[:, 0] = s
    return [paths[n, :lens[n]].copy() for n in range(N)], scores


def path_score_f64(e, A, pi, path):
    """The float64 score of `path` under the unquantised float32 inputs."""
    e, A, pi = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (e, A, pi))
    p = path.astype(np.int64)
    return pi[p[0]] + e[np.arange(len(p)), p].sum() + A[p[:-1], p[1:]].sum()


def emissions(kind, T, rng):
    """(T, 4) float32 of one of the four kinds the tests cross with lengths, transitions and initial scores."""
    if kind == "dirichlet1":
        with np.errstate(divide="ignore"):
            return np.log(rng.dirichlet(np.ones(4), size=T)).astype(np.float32)
    if kind == "dirichlet0.2":
        with np.errstate(divide="ignore"):
            return np.log(rng.dirichlet(np.full(4, 0.2), size=T)).astype(np.float32)
    if kind == "zeros":
        return np.zeros((T, 4), dtype=np.float32)
    if kind == "integers":
        return -rng.integers(0, 4, size=(T, 4)).astype(np.float32)
    raise ValueError(kind)


KINDS = ("dirichlet1", "dirichlet0.2", "zeros", "integers")


def dense_transitions(seed):
    """A seeded dense A: the log of a row-stochastic matrix."""
    rng = np.random.default_rng(seed)
    return np.log(rng.dirichlet(np.ones(4), size=4)).astype(np.float32)


UNIFORM = np.zeros(4, dtype=np.float32)
STATE0 = np.array([0.0, NINF, NINF, NINF], dtype=np.float32)
