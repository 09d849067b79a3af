// duration_posterior_layout.hpp -- the arithmetic and the geometry of the explicit-duration (semi-Markov) forward-backward kernel
// (hssfsst.h: hssfsst_posteriors_durations), as plain functions shared by the kernel (segmenter_duration_posteriors.hpp) and a CPU
// check (tests/native/duration_posteriors_check.cpp).  No HIP call here.  The sum-product twin of decode_durations_layout.hpp: the
// same model, un-quantised, and the same push-into-a-ring geometry (lane_state, lane_duration, ring_slot are durlayout's).
//
// The model.  A recording of T steps is cut into runs (s_1, d_1) .. (s_K, d_K): sum d_k = T, 1 <= d_k <= D, s_k != s_(k+1); its
// log weight is pi[s_1] + sum_k len_k + sum_k A[s_k][s_(k+1)] + sum_t e[t][s(t)], len_k = edge[s_k][d_k] for the first and the last
// run (once when K = 1), dur[s_k][d_k] otherwise.  The diagonal of A is never read; -inf in pi, A, dur, edge means forbidden (so
// does NaN); an emission of -inf or NaN counts as -32768 (the decoder's rule: the arithmetic runs on prefix sums).
//
// The recurrence, with E_j(t) = sum_(u<t) e[u][j] (float64, summed in step order) and r_ij(t) = exp(E_i(t) - E_j(t)):
//   b_0(j) = exp pi[j];   c_t(j) = sum_(d=1..min(D,t)) b_(t-d)(j) L(j,d)        L = edge if t - d == 0 or t == T, else dur    t = 1 .. T
//                         b_t(j) = sum_(i != j) c_t(i) r_ij(t) P[i][j]                                                        t = 1 .. T-1
//   Z = sum_j c_T(j) exp E_j(T)
//   g_T(j) = exp E_j(T);  cb_t(j) = sum_(d=1..min(D,T-t)) g_(t+d)(j) L(j,d)     L = edge if t == 0 or t + d == T, else dur    t = T-1 .. 0
//                         g_t(i) = sum_(j != i) P[i][j] cb_t(j) r_ij(t)                                                       t = T-1 .. 1
//   x_t(i,j) = c_t(i) r_ij(t) P[i][j] cb_t(j) / Z  (t = 1 .. T-1): Xi[i][j] = sum_t x_t(i,j), S_t(j) = sum_i x_t(i,j) (a run of j starts
//   at t), S_0(j) = b_0(j) cb_0(j) / Z, N_t(j) = c_t(j) g_t(j) / Z (a run of j ends before t);
//   gamma_(T-1) = N_T, gamma_(t-1) = (gamma_t - S_t) + N_t, stored clamped to [0, 1].
//
// The arithmetic.  Every b, c, g, cb, P, L, r and ring word is a Sc: a float64 mantissa with an int exponent (posterior_layout.hpp's
// frexp / ldexp discipline, per scalar).  exp(x) enters as (2^frac, floor) of x / ln 2, 2^frac from a fixed polynomial (scaled_exp).
// A product multiplies the mantissas and adds the exponents and is NOT renormalised; a sum aligns the two exponents with ldexp (exact) and adds; c, b, cb, g
// and Z are renormalised (frexp) where they are formed, so a mantissa is a product of at most five normalised ones or a sum of at
// most D of those.  The sources of one ring word arrive in order of FALLING d, one per step: the first -- source 0, or the owner of
// d = D -- stores, a later one adds; that fixes the order of the additions, and duration_posteriors_reference() adds in that order.
// No exp or log on the O(D) path.
// THE LIMITS.  Exponents are 32-bit and those of two summands are subtracted: every |E_j(t)| must stay below 3.7e8 nats (2^29
// binary exponents): emissions within +-350 at the longest recording of 2^20 steps; -inf / NaN emissions (-32768 each) at no more than
// ~11 000 steps of one state.  The relative error of every output grows with |E_j(T)| 2^-53 (x / ln 2 is rounded before it is
// split).  Nothing underflows otherwise: there is no 700-nat limit as in posterior_layout.hpp.
//
// Geometry of the kernel: decode_durations_layout.hpp's PUSH form, twice.  Lane l works for state l mod 4 and owns the durations
// l / 4 + 1 + 128 k.  Forward: once b_t(j) is known the lane adds b_t(j) L(j,d) to the ring words of the targets t + d; target t's
// four words are c_t.  The c_t are stashed (kStashBytesPerStep a step) and E(t) is checkpointed once per segment of kSegSteps steps,
// so that the reverse sweep -- the same push from the other end, g_u(j) L(j,d) into the targets u - d -- has c_u and, after summing
// the segment's emissions from its checkpoint in the forward order, bit for bit the same E(u).
#pragma once

#include "decode_durations_layout.hpp"

#if defined(__HIPCC__)
#define HSSFSST_DP_UNROLL _Pragma("unroll")              // a loop over the four states left rolled would index registers: scratch
#else
#define HSSFSST_DP_UNROLL
#endif

namespace hssfsst::dplayout {

using declayout::i64;
using durlayout::kLanes;
using durlayout::kLaneStep;
using durlayout::kMaxDuration;
using durlayout::kMaxRing;
using durlayout::kPerLane;
using durlayout::lane_duration;
using durlayout::lane_state;
using durlayout::ring_slot;
using durlayout::ring_slots;
using durlayout::table_index;
using durlayout::table_index_of_source;

constexpr int kSegSteps = 256;                           // steps staged at a time, in either sweep
constexpr i64 kMaxSteps = i64(1) << 20;                  // per recording
constexpr int kZeroExp = -(1 << 30);                     // the exponent a zero carries; never looked at
constexpr double kLn2 = 0.693147180559945309417232121458;
constexpr double kLog2e = 1.44269504088896340735992468100;
constexpr double kEmissionFloor = -32768.0;              // what an emission of -inf or NaN counts as

struct Sc { double m; int e; };                          // value = m x 2^e, m >= 0; m == 0 is zero whatever e says

HSSFSST_DEC_HD inline Sc zero() { return Sc{0.0, kZeroExp}; }
// exponents are added and subtracted modulo 2^32: a zero's exponent may take part, a live one stays far inside (THE LIMITS)
HSSFSST_DEC_HD inline int wadd(int a, int b) { return static_cast<int>(static_cast<unsigned>(a) + static_cast<unsigned>(b)); }
HSSFSST_DEC_HD inline int wsub(int a, int b) { return static_cast<int>(static_cast<unsigned>(a) - static_cast<unsigned>(b)); }

HSSFSST_DEC_HD inline Sc norm(Sc a)                      // mantissa into [0.5, 1); a zero, a negative or a NaN one becomes zero
{
    if (!(a.m > 0.0)) return zero();
    int k;
    a.m = frexp(a.m, &k);
    a.e = wadd(a.e, k);
    return a;
}
HSSFSST_DEC_HD inline Sc mul(Sc a, Sc b)
{
    const double m = a.m * b.m;
    return m > 0.0 ? Sc{m, wadd(a.e, b.e)} : zero();
}
HSSFSST_DEC_HD inline Sc add(Sc a, Sc b)
{
    if (!(b.m > 0.0)) return a;
    if (!(a.m > 0.0)) return b;
    const int e = a.e > b.e ? a.e : b.e;
    return Sc{ldexp(a.m, wsub(a.e, e)) + ldexp(b.m, wsub(b.e, e)), e};
}
HSSFSST_DEC_HD inline double value(Sc a) { return a.m > 0.0 ? ldexp(a.m, a.e) : 0.0; }
HSSFSST_DEC_HD inline Sc inverse(Sc a) { return a.m > 0.0 ? norm(Sc{1.0 / a.m, wsub(0, a.e)}) : zero(); }
HSSFSST_DEC_HD inline double log_of(Sc a)
{
    return a.m > 0.0 ? log(a.m) + static_cast<double>(a.e) * kLn2 : -std::numeric_limits<double>::infinity();
}

// exp(u) for |u| <= ln 2 / 2: the Taylor series to u^14 / 14! (the next term is below 4e-18), one fma a term -- the same bits on the
// host and on the device, and a handful of registers where a library exp2 takes dozens (a reverse step forms eight of these)
HSSFSST_DEC_HD inline double exp_small(double u)
{
    double p = 1.0 / 87178291200.0;
    p = fma(p, u, 1.0 / 6227020800.0);
    p = fma(p, u, 1.0 / 479001600.0);
    p = fma(p, u, 1.0 / 39916800.0);
    p = fma(p, u, 1.0 / 3628800.0);
    p = fma(p, u, 1.0 / 362880.0);
    p = fma(p, u, 1.0 / 40320.0);
    p = fma(p, u, 1.0 / 5040.0);
    p = fma(p, u, 1.0 / 720.0);
    p = fma(p, u, 1.0 / 120.0);
    p = fma(p, u, 1.0 / 24.0);
    p = fma(p, u, 1.0 / 6.0);
    p = fma(p, u, 0.5);
    p = fma(p, u, 1.0);
    return fma(p, u, 1.0);
}

// exp(x) = 2^(f + 1) x (2^-1/2 exp((y - f - 1/2) ln 2)),  y = x / ln 2, f = floor(y); -inf and NaN give zero
HSSFSST_DEC_HD inline Sc scaled_exp(double x)
{
    if (!(x >= -1.0e300)) return zero();
    const double y = x * kLog2e, f = floor(y);
    return Sc{0.70710678118654752440 * exp_small((y - f - 0.5) * kLn2), static_cast<int>(f) + 1};
}

HSSFSST_DEC_HD inline double emission(float x)
{
    return (x != x || x < -std::numeric_limits<float>::max()) ? kEmissionFloor : static_cast<double>(x);
}

HSSFSST_DEC_HD inline double pick4(const double v[4], int j) { return j == 0 ? v[0] : j == 1 ? v[1] : j == 2 ? v[2] : v[3]; }
// (all four read first, then chosen field by field: a conditional between the array's elements themselves selects an ADDRESS, and an
// array indexed that way lives in scratch)
HSSFSST_DEC_HD inline Sc pick4(const Sc v[4], int j)
{
    const Sc a = v[0], b = v[1], c = v[2], d = v[3];
    return Sc{j == 0 ? a.m : j == 1 ? b.m : j == 2 ? c.m : d.m, j == 0 ? a.e : j == 1 ? b.e : j == 2 ? c.e : d.e};
}

// Column j of P = exp(A) (col[i] = P[i][j]), row j (row[i] = P[j][i]) -- the diagonal entry of either is zero -- and p0 = exp(pi[j]),
// from the 20 floats {A row-major, pi}
struct StateTables { Sc col[4], row[4], p0; };
HSSFSST_DEC_HD inline StateTables state_tables(const float* a_pi, int j)
{
    StateTables t;
    HSSFSST_DP_UNROLL
    for (int i = 0; i < 4; ++i) {
        t.col[i] = i == j ? zero() : scaled_exp(static_cast<double>(a_pi[4 * i + j]));
        t.row[i] = i == j ? zero() : scaled_exp(static_cast<double>(a_pi[4 * j + i]));
    }
    t.p0 = scaled_exp(static_cast<double>(a_pi[16 + j]));
    return t;
}

// b_t(j) from c_t (all four), E(t) and column j of P:  sum_i c_t(i) r_ij(t) P[i][j], i ascending
HSSFSST_DEC_HD inline Sc run_start(const Sc C[4], const double E[4], const Sc col[4], int j)
{
    const double ej = pick4(E, j);
    Sc acc = zero();
    HSSFSST_DP_UNROLL
    for (int i = 0; i < 4; ++i) acc = add(acc, mul(mul(C[i], scaled_exp(E[i] - ej)), col[i]));
    return norm(acc);
}
// g_t(i) from cb_t (all four), E(t) and row i of P:  sum_j P[i][j] cb_t(j) r_ij(t), j ascending
HSSFSST_DEC_HD inline Sc run_end(const Sc CB[4], const double E[4], const Sc row[4], int i)
{
    const double ei = pick4(E, i);
    Sc acc = zero();
    HSSFSST_DP_UNROLL
    for (int j = 0; j < 4; ++j) acc = add(acc, mul(mul(CB[j], scaled_exp(ei - E[j])), row[j]));
    return norm(acc);
}
// Z from c_T and E(T)
HSSFSST_DEC_HD inline Sc total(const Sc C[4], const double E[4])
{
    Sc acc = zero();
    HSSFSST_DP_UNROLL
    for (int j = 0; j < 4; ++j) acc = add(acc, mul(C[j], scaled_exp(E[j])));
    return norm(acc);
}
// x_t(i, j), i = 0 .. 3, of state j: x[i] = c_t(i) r_ij(t) P[i][j] cb_t(j) / Z; returns their sum S_t(j)
HSSFSST_DEC_HD inline double run_changes(const Sc C[4], const double E[4], const Sc col[4], int j, Sc cbj, Sc invz, double x[4])
{
    const double ej = pick4(E, j);
    const Sc tail = mul(cbj, invz);
    double s = 0.0;
    HSSFSST_DP_UNROLL
    for (int i = 0; i < 4; ++i) {
        x[i] = value(mul(mul(mul(C[i], scaled_exp(E[i] - ej)), col[i]), tail));
        s += x[i];
    }
    return s;
}
HSSFSST_DEC_HD inline double clamp01(double g) { return g < 0.0 ? 0.0 : (g > 1.0 ? 1.0 : g); }

// Segments: rows r0 = seg kSegSteps .. of a recording, row r = step r of the emissions = c_(r+1) of the stash = E(r+1)
HSSFSST_DEC_HD inline i64 segments(i64 T) { return (T + kSegSteps - 1) / kSegSteps; }

// The workspace, 16-byte aligned, of a list of `total` steps in `count` recordings at duration D:
//   [0, 64 D)                    the mantissas of the linear tables, float64 [dur, edge][d - 1][j]  (durlayout::table_index)
//   [64 D, 96 D)                 their exponents, int32, same index
//   then 32 bytes per step       the mantissas of c_(r+1), four float64, row offsets[i] + r
//   then 16 bytes per step       their exponents, four int32
//   then 32 bytes per slot       E before a segment, four float64; recording number `rec` at step offset `off` has its segments'
//                                slots from off / kSegSteps + rec on (posterior_layout.hpp's argument: consecutive recordings are
//                                floor(T / kSegSteps) + 1 >= segments(T) slots apart at least)
constexpr i64 kStashBytesPerStep = 48;
constexpr i64 kCheckpointBytes = 32;
constexpr i64 kWorkBytesPerStep = kStashBytesPerStep + 1;    // (a segment's steps pay for its checkpoint: 32 <= kSegSteps)
constexpr i64 kWorkBytesPerRecording = kCheckpointBytes;
constexpr i64 kWorkBytesPerDuration = 96;
static_assert(kCheckpointBytes <= kSegSteps, "a segment's steps pay for its checkpoint");
static_assert(kWorkBytesPerStep <= 64, "the stash stays within 64 bytes a step");
HSSFSST_DEC_HD inline i64 table_bytes(int D) { return kWorkBytesPerDuration * static_cast<i64>(D); }
HSSFSST_DEC_HD inline i64 checkpoint_slot(i64 off, i64 rec) { return off / kSegSteps + rec; }
HSSFSST_DEC_HD inline i64 checkpoint_slots(i64 total_steps, i64 count) { return total_steps / kSegSteps + count; }
HSSFSST_DEC_HD inline i64 workspace_bytes(i64 total_steps, i64 count, int D)
{
    return table_bytes(D) + kWorkBytesPerStep * total_steps + kWorkBytesPerRecording * count;
}
struct Workspace { i64 table_mant, table_exp, stash_mant, stash_exp, checkpoints, end; };    // byte offsets
HSSFSST_DEC_HD inline Workspace workspace(i64 total_steps, i64 count, int D)
{
    Workspace w;
    w.table_mant = 0;
    w.table_exp = 64 * static_cast<i64>(D);
    w.stash_mant = table_bytes(D);
    w.stash_exp = w.stash_mant + 32 * total_steps;
    w.checkpoints = w.stash_exp + 16 * total_steps;
    w.end = w.checkpoints + kCheckpointBytes * checkpoint_slots(total_steps, count);
    return w;
}

// the labelled segmentation's terms at step r, in the order they are added to the score (which starts at pi[y_0]): the emission, and
// behind a run's last step its length score and the transition out of it.  *start: the first step of the run that r belongs to.
HSSFSST_DEC_HD inline double label_terms(double em, int y, int ynext, i64 r, i64 T, i64* start, const float* a_pi, const float* dur,
                                         const float* edge, int D)
{
    double s = em;
    if (r + 1 == T || ynext != y) {
        const i64 d = r + 1 - *start;
        const float* tab = (*start == 0 || r + 1 == T) ? edge : dur;
        s += d > D ? -std::numeric_limits<double>::infinity() : static_cast<double>(tab[static_cast<i64>(y) * D + (d - 1)]);
        if (r + 1 < T) s += static_cast<double>(a_pi[4 * y + ynext]);
        *start = r + 1;
    }
    return s;
}

struct Result { double loglik, score; double xi[16]; double s0[4]; };

// The specification: the sequential loop, in the pull form, adding in the ring's order.  e (T, 4), a_pi (20), dur, edge (4, D) float32;
// labels (T) or nullptr; gamma (T, 4) out; onsets (T, 4) out or nullptr.  With labels gamma is gamma - onehot(labels), xi is Xi -
// counts(label runs), s0 is S_0 - onehot(labels[0]) and score is the labelled segmentation's weight; the onsets are never changed.
template <class G>                                       // G: float (what the kernel stores) or double (for a check)
inline Result duration_posteriors_reference(const float* e, i64 T, const float* a_pi, const float* dur, const float* edge, int D,
                                            const uint8_t* labels, G* gamma, G* onsets)
{
    const size_t n = static_cast<size_t>(T), nd = static_cast<size_t>(D);
    StateTables st[4];
    for (int j = 0; j < 4; ++j) st[j] = state_tables(a_pi, j);
    std::vector<Sc> Ld(4 * nd), Le(4 * nd);              // [j D + d - 1]
    for (size_t k = 0; k < 4 * nd; ++k) {
        Ld[k] = scaled_exp(static_cast<double>(dur[k]));
        Le[k] = scaled_exp(static_cast<double>(edge[k]));
    }
    auto len = [&](bool at_edge, int j, i64 d) { return (at_edge ? Le : Ld)[static_cast<size_t>(j) * nd + static_cast<size_t>(d - 1)]; };
    std::vector<double> E(4 * (n + 1), 0.0);
    for (size_t t = 0; t < n; ++t)
        for (int j = 0; j < 4; ++j) E[4 * (t + 1) + j] = E[4 * t + j] + emission(e[4 * t + j]);
    Result out{};
    if (labels) {
        i64 start = 0;
        out.score = static_cast<double>(a_pi[16 + (labels[0] & 3)]);
        for (i64 r = 0; r < T; ++r) {
            const int y = labels[r] & 3, yn = r + 1 < T ? labels[r + 1] & 3 : -1;
            out.score += label_terms(emission(e[4 * r + y]), y, yn, r, T, &start, a_pi, dur, edge, D);
        }
    }
    std::vector<Sc> b(4 * n), c(4 * (n + 1)), g(4 * (n + 1)), cb(4 * n);
    for (int j = 0; j < 4; ++j) b[j] = st[j].p0;
    for (i64 t = 1; t <= T; ++t) {
        for (int j = 0; j < 4; ++j) {
            Sc acc = zero();
            for (i64 d = t < D ? t : D; d >= 1; --d) acc = add(acc, mul(b[4 * (t - d) + j], len(t - d == 0 || t == T, j, d)));
            c[4 * t + j] = norm(acc);
        }
        if (t < T)
            for (int j = 0; j < 4; ++j) b[4 * t + j] = run_start(&c[4 * t], &E[4 * t], st[j].col, j);
    }
    const Sc Z = total(&c[4 * T], &E[4 * T]), invz = inverse(Z);
    out.loglik = log_of(Z);
    for (int j = 0; j < 4; ++j) g[4 * T + j] = scaled_exp(E[4 * T + j]);
    double gam[4] = {0.0, 0.0, 0.0, 0.0};
    for (i64 t = T; t >= 0; --t) {
        if (t < T) {
            for (int j = 0; j < 4; ++j) {
                Sc acc = zero();
                for (i64 d = T - t < D ? T - t : D; d >= 1; --d) acc = add(acc, mul(g[4 * (t + d) + j], len(t == 0 || t + d == T, j, d)));
                cb[4 * t + j] = norm(acc);
            }
            if (t >= 1)
                for (int i = 0; i < 4; ++i) g[4 * t + i] = run_end(&cb[4 * t], &E[4 * t], st[i].row, i);
        }
        if (t == 0) break;
        for (int j = 0; j < 4; ++j) {
            const double N = value(mul(mul(c[4 * t + j], g[4 * t + j]), invz));
            if (t < T) {
                double x[4];
                const double S = run_changes(&c[4 * t], &E[4 * t], st[j].col, j, cb[4 * t + j], invz, x);
                for (int i = 0; i < 4; ++i) out.xi[4 * i + j] += x[i];
                if (onsets) onsets[4 * t + j] = static_cast<G>(S);
                gam[j] = (gam[j] - S) + N;
            } else {
                gam[j] = N;
            }
            // (rounded to G first, as the kernel's staged float32 gamma is, then the label's 1 is taken off)
            gamma[4 * (t - 1) + j] = static_cast<G>(clamp01(gam[j])) - static_cast<G>(labels && (labels[t - 1] & 3) == j ? 1.0 : 0.0);
        }
        if (labels && t < T && (labels[t - 1] & 3) != (labels[t] & 3)) out.xi[4 * (labels[t - 1] & 3) + (labels[t] & 3)] -= 1.0;
    }
    for (int j = 0; j < 4; ++j) {
        const double S = value(mul(mul(st[j].p0, cb[j]), invz));
        if (onsets) onsets[j] = static_cast<G>(S);
        out.s0[j] = S - (labels && (labels[0] & 3) == j ? 1.0 : 0.0);
    }
    return out;
}

}  // namespace hssfsst::dplayout
