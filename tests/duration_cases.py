"""The explicit-duration decoder's specification restated in numpy (include/hssfsst.h: hssfsst_decode_durations; the loop of
csrc/decode_durations_layout.hpp: decode_durations_reference), with no import from the package: the two quantisers, the
sequential loop over int64 with the absorbing NEG, vectorised over the duration d, the tie rules, the backtrace -- the same loop
in float64 without quantisation, for the bound between the two -- and a brute-force enumerator of every segmentation."""
import numpy as np

from tests.decode_cases import NEG, NINF, quantise


def quantise_emissions(e):
    """qe(x) = q(x), except that -inf and NaN count as -32768: the decoder works on prefix sums."""
    e = np.asarray(e, dtype=np.float32)
    return quantise(np.where(np.isnan(e) | np.isneginf(e), np.float32(-32768.0), e))


def _add(a, b):
    with np.errstate(over="ignore"):
        return np.where((a == NEG) | (b == NEG), NEG, a + b)


def decode(e, A, pi, dur, edge, exact=True):
    """e (T, 4), A (4, 4) (diagonal ignored), pi (4,), dur, edge (4, D).  Returns (path (T,) uint8, score): the int64 score in
    units of 2^-20 when exact, else the float64 score of the unquantised float64 recurrence (same tie rules; -inf, not NEG)."""
    e = np.asarray(e, dtype=np.float32)
    T, D = e.shape[0], np.asarray(dur).shape[1]
    if exact:
        neg, add = NEG, _add
        qa, qp, qd, qg = (quantise(v) for v in (A, pi, dur, edge))
        qe = quantise_emissions(e)
    else:
        neg, add = NINF, (lambda a, b: a + b)
        qa, qp, qd, qg = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (A, pi, dur, edge))
        qe = np.where(np.isnan(e) | np.isneginf(e), np.float32(-32768.0), e).astype(np.float64)
    E = np.zeros((T + 1, 4), dtype=qe.dtype)
    np.cumsum(qe, axis=0, out=E[1:])
    qa = qa.copy()
    qa[np.arange(4), np.arange(4)] = neg                 # a run is never followed by the same state
    B = np.full((T, 4), neg, dtype=qe.dtype)
    B[0] = qp
    argd = np.zeros((T, 4), dtype=np.int64)
    argi = np.zeros((T, 4), dtype=np.int64)
    for t in range(1, T):
        m = min(D, t)
        c = add(B[t - m:t][::-1].T, qd[:, :m])           # [j, d - 1] for d = 1 .. m
        if m == t:
            c[:, t - 1] = add(B[0], qg[:, t - 1])        # the run that starts the recording
        k = c.argmax(axis=1)                             # the first, i.e. smallest, d that attains the max
        argd[t] = k + 1
        F = add(c[np.arange(4), k], E[t])
        via = add(F[:, None], qa)                        # [i, j]
        i = via.argmax(axis=0)                           # the smallest i (never j itself unless all are forbidden)
        argi[t] = i
        best = via.max(axis=0)
        with np.errstate(over="ignore", invalid="ignore"):
            B[t] = np.where(best == neg, neg, best - E[t])
    m = min(D, T)
    c = add(B[T - m:T][::-1].T, qg[:, :m])
    k = c.argmax(axis=1)
    tot = add(c[np.arange(4), k], E[T])
    s = int(tot.argmax())                                # the smallest j, then (k) the smallest d
    score = tot[s]
    path = np.zeros(T, dtype=np.uint8)
    if score == neg:
        return path, score
    t, d = T, int(k[s]) + 1
    while True:
        path[t - d:t] = s
        t -= d
        if t == 0:
            break
        s = int(argi[t, s])
        d = int(argd[t, s])
    return path, score


def decode_list(es, A, pi, dur, edge):
    """The list form: (list of paths, int64 scores)."""
    out = [decode(e, A, pi, dur, edge) for e in es]
    return [p for p, _ in out], np.array([s for _, s in out], dtype=np.int64)


def runs_of(path):
    """[(state, steps)] of a path."""
    p = np.asarray(path).astype(np.int64)
    cut = np.flatnonzero(np.diff(p)) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(p)]])
    return [(int(p[a]), int(b - a)) for a, b in zip(starts, ends)]


def path_score(e, A, pi, dur, edge, path, exact=True):
    """The score of `path` read as its runs: int64 (NEG when a forbidden entry is used) or float64 on the unquantised inputs."""
    e = np.asarray(e, dtype=np.float32)
    if exact:
        qa, qp, qd, qg, qe = quantise(A), quantise(pi), quantise(dur), quantise(edge), quantise_emissions(e)
    else:
        qa, qp, qd, qg = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (A, pi, dur, edge))
        qe = np.where(np.isnan(e) | np.isneginf(e), np.float32(-32768.0), e).astype(np.float64)
    runs = runs_of(path)
    D = qd.shape[1]
    terms = [qp[runs[0][0]]]
    for k, (s, d) in enumerate(runs):
        if d > D:
            return NEG if exact else NINF
        terms.append((qg if k in (0, len(runs) - 1) else qd)[s, d - 1])
        if k:
            terms.append(qa[runs[k - 1][0], s])
    p = np.asarray(path).astype(np.int64)
    terms.extend(qe[np.arange(len(p)), p].tolist())
    if exact:
        return NEG if any(int(v) == NEG for v in terms) else sum(int(v) for v in terms)
    return float(np.sum(np.array(terms, dtype=np.float64)))


def brute_force(e, A, pi, dur, edge):
    """Every segmentation of the T steps, scored in exact integers: (best score or NEG, set of the paths that attain it, as
    tuples).  4 x 4^(T - 1) segmentations at D >= T: T <= 8 or so."""
    qa, qp, qd, qg = (quantise(v).tolist() for v in (A, pi, dur, edge))
    pre = np.concatenate([np.zeros((1, 4), dtype=np.int64), np.cumsum(quantise_emissions(e), axis=0)]).tolist()
    T, D = len(pre) - 1, len(qd[0])
    found = [NEG, set()]

    def walk(t, last, score, runs):
        if t == T:
            if score > found[0]:
                found[0], found[1] = score, set()
            if score == found[0]:
                found[1].add(tuple(s for s, d in runs for _ in range(d)))
            return
        for s in range(4):
            if s == last:
                continue
            move = qp[s] if last < 0 else qa[last][s]
            if move == NEG:
                continue
            for d in range(1, min(D, T - t) + 1):
                ln = (qg if t == 0 or t + d == T else qd)[s][d - 1]
                if ln != NEG:
                    walk(t + d, s, score + move + ln + pre[t + d][s] - pre[t][s], runs + [(s, d)])

    walk(0, -1, 0, [])
    return found[0], found[1]


def random_tables(rng, D, forbidden=0.3, min_duration=1):
    """(dur, edge) (4, D) float32: uniform scores in [-4, 0), a share of dur forbidden (never a whole row), every duration
    below min_duration forbidden in dur (D itself stays allowed); edge all finite."""
    dur = (-4.0 * rng.random((4, D))).astype(np.float32)
    dur[rng.random((4, D)) < forbidden] = NINF
    dur[:, :min(min_duration, D) - 1] = NINF
    dur[:, D - 1] = np.where(np.isneginf(dur[:, D - 1]), np.float32(-1.0), dur[:, D - 1])
    edge = (-4.0 * rng.random((4, D))).astype(np.float32)
    return dur, edge


def geometric_tables(D, stay=-0.5):
    """dur = edge = stay (d - 1): with A[i][i] = stay in the first-order decoder the two models score every path alike."""
    row = (stay * np.arange(D)).astype(np.float32)
    t = np.tile(row, (4, 1))
    return t, t.copy()


def geometric_transitions(stay=-0.5, advance=-1.25):
    A = np.full((4, 4), NINF, dtype=np.float32)
    for i in range(4):
        A[i, i] = stay
        A[i, (i + 1) % 4] = advance
    return A


def minimum_duration_tables(D, dmin):
    """dur: 0 for dmin <= d <= D, forbidden below; edge: 0 everywhere (a cut-off run may be short)."""
    dur = np.zeros((4, D), dtype=np.float32)
    dur[:, :dmin - 1] = NINF
    return dur, np.zeros((4, D), dtype=np.float32)
