// decode_durations_layout.hpp -- the arithmetic and the geometry of the explicit-duration (semi-Markov) Viterbi decoder (hssfsst.h:
// hssfsst_decode_durations), as plain functions shared by the kernel (segmenter_decode_durations.hpp) and a CPU check
// (tests/native/decode_durations_check.cpp).  No HIP call here.  The quantiser, add, kNeg and i64 are decode_layout.hpp's.
//
// A recording of T steps is cut into runs (s_1, d_1) .. (s_K, d_K): sum d_k = T, 1 <= d_k <= D, s_k != s_(k+1).  Its score is
//   q(pi[s_1]) + sum_k len_k + sum_k q(A[s_k][s_(k+1)]) + sum_t qe(e[t][s(t)])
// with len_k = q(edge[s_k][d_k]) for the first and the last run (they are cut off by the recording's ends; for K = 1 it is paid
// once) and q(dur[s_k][d_k]) for every other.  dur, edge: (4, D) float32, column d - 1 holds duration d.  The diagonal of A is
// never read.  -inf in pi, A, dur, edge means "forbidden".
// Emissions: qe(x) = q(x), except that -inf and NaN count as -32768.  The decoder works on the prefix sums E_j(t) = sum_(u<t)
// qe(e[u][j]), and an absorbing element cannot sit inside a prefix sum -- this is the one difference from hssfsst_decode_states,
// where an emission of -inf forbids its state at its step.
//
// decode_durations_reference() is the sequential loop that defines the result bit for bit:
//   B_0(j) = q(pi[j])                                                       (the best score of "a run of j starts at t", less E_j(t))
//   t = 1 .. T - 1:  F_t(j) = E_j(t) + max_(1 <= d <= min(D, t)) (B_(t-d)(j) + len),  len = edge[j][d] if d == t, else dur[j][d];
//                    ties to the SMALLEST d                                 (the best score of "a run of j ends before t")
//                    B_t(j) = max_(i != j) (F_t(i) + A[i][j]) - E_j(t);  ties to the SMALLEST i
//   end:             max over (j, 1 <= d <= min(D, T)) of B_(T-d)(j) + edge[j][d] + E_j(T);  ties to the smallest j, then d
//   the backtrace follows the stored (d, i) pairs; if no segmentation is allowed the score is kNeg and every state is 0.
//
// The bound.  A segmentation of the first t steps has one pi term, t emission terms and at most t runs of one len and one A term
// each: 3 t + 1 terms of at most 2^35.  B_t adds one A term and subtracts a prefix sum of t terms, a candidate adds one len:
// at most 4 t + 3 terms, so with T <= 2^24 no sum leaves (2^26 + 3) 2^35 < 2^62.
//
// Geometry of the kernel: the PUSH form.  Lane l works for ONE state, lane_state(l) = l mod 4, and owns the durations d =
// l / 4 + 1 + 128 k of it (lane_duration).  Once B_t(j) of its state is known -- three candidates of target t in the ring -- it adds
// it to the candidates of the targets t + d in a ring of D + 1 steps (ring_slot): C = max(C, B_t(j) + len).  Distinct lanes hit
// distinct words; the sources of one target arrive in order of FALLING d, one per step, so the first writer -- source 0, or the
// owner of d = D -- overwrites (the ring is never cleared) and a later writer takes a tie (takes()): the smallest d wins.
// Source 0, and the source that reaches target T, push edge instead of dur; target T's slot is the end maximum.
#pragma once

#include "decode_layout.hpp"

namespace hssfsst::durlayout {

using declayout::add;
using declayout::i64;
using declayout::kNeg;
using declayout::quantise;

constexpr int kLanes = 512;                              // the workgroup: two waves per SIMD, which take turns at the issue port
constexpr int kLaneStep = kLanes / 4;                    // lanes per state: a lane's durations are this far apart
constexpr int kPerLane = 16;                             // durations a lane owns
constexpr int kMaxDuration = kLaneStep * kPerLane;       // D <= 2048: 2 s at 1 kHz
constexpr int kMaxRing = kMaxDuration + 1;
constexpr int kSegSteps = 512;                           // emissions staged at a time
constexpr i64 kMaxSteps = i64(1) << 24;                  // per recording
static_assert(4 * kMaxSteps + 3 <= (i64(1) << 62) / declayout::kMaxTerm, "a candidate must stay within 2^62");
constexpr i64 kWorkspaceBytesPerStep = 8;                // a step's four 16-bit duration backpointers
static_assert(kMaxDuration < 65536, "a duration backpointer is a 16-bit word");

// The workspace, 16-byte aligned: first the quantised tables, [dur, edge][d - 1][j] int64 -- 64 D bytes, the size of 8 D steps --
// then 8 bytes per step of the whole list (recording i's step t at 64 D + 8 (offsets[i] + t)).
HSSFSST_DEC_HD inline i64 table_words(int D) { return 8 * static_cast<i64>(D); }
HSSFSST_DEC_HD inline i64 workspace_steps(i64 total_steps, int D) { return total_steps + table_words(D); }
HSSFSST_DEC_HD inline i64 table_index(int which, int d, int j, int D) { return (static_cast<i64>(which) * D + (d - 1)) * 4 + j; }
// ... filled from the caller's two (4, D) float tables, read as one list of 8 D values: value s of that list goes to
HSSFSST_DEC_HD inline i64 table_index_of_source(int s, int D) { return table_index(s / (4 * D), s % D + 1, (s % (4 * D)) / D, D); }

HSSFSST_DEC_HD inline i64 quantise_emission(float x)
{
    if (x != x || x < -std::numeric_limits<float>::max()) x = -declayout::kClamp;
    return quantise(x);
}

HSSFSST_DEC_HD inline int ring_slots(int D) { return D + 1; }
HSSFSST_DEC_HD inline int ring_slot(int cur, int d, int R) { return cur + d >= R ? cur + d - R : cur + d; }   // cur, d < R
// ... and where every lane reads and writes a word whether it owns a duration <= D or not: a duration above D gets the row d,
// which lies behind the ring's D + 1 rows and inside kMaxRing, and is nobody else's
HSSFSST_DEC_HD inline int bulk_slot(int cur, int d, int D, int R) { return d <= D ? ring_slot(cur, d, R) : d; }
HSSFSST_DEC_HD inline int lane_state(int lane) { return lane & 3; }
HSSFSST_DEC_HD inline int lane_duration(int lane, int k) { return (lane >> 2) + 1 + k * kLaneStep; }
// does a later writer's candidate replace the held one?  (kNeg never wins: a forbidden run is nobody's backpointer)
HSSFSST_DEC_HD inline bool takes(i64 cand, i64 held) { return cand != kNeg && cand >= held; }

struct Tables {
    i64 A[4][4];                                         // quantised log transitions; the diagonal is not read
    i64 pi[4];
};

HSSFSST_DEC_HD inline i64 pick4(const i64 v[4], int j) { return j == 0 ? v[0] : j == 1 ? v[1] : j == 2 ? v[2] : v[3]; }

// B_t(j) from the candidates C of target t (C[i] = F_t(i) - E_i(t)), the prefix sums E(t) and column j of A (Acol[i] = A[i][j];
// Acol[j] is not read); *arg <- the predecessor state, the smallest i that attains the max.
HSSFSST_DEC_HD inline i64 run_start(const i64 C[4], const i64 E[4], const i64 Acol[4], int j, unsigned* arg)
{
    i64 best = kNeg;
    unsigned a = j == 0 ? 1u : 0u;
    for (int i = 0; i < 4; ++i) {
        const i64 c = i == j ? kNeg : add(add(C[i], E[i]), Acol[i]);
        if (c > best) { best = c; a = static_cast<unsigned>(i); }
    }
    *arg = a;
    return best == kNeg ? kNeg : best - pick4(E, j);
}

// ... of all four states; returns the four predecessor states packed two bits each, as decode_layout.hpp packs its backpointer byte
HSSFSST_DEC_HD inline unsigned run_starts(const i64 C[4], const i64 E[4], const Tables& tb, i64 B[4])
{
    unsigned byte = 0;
    for (int j = 0; j < 4; ++j) {
        const i64 Acol[4] = {tb.A[0][j], tb.A[1][j], tb.A[2][j], tb.A[3][j]};
        unsigned arg;
        B[j] = run_start(C, E, Acol, j, &arg);
        byte |= arg << (2 * j);
    }
    return byte;
}
// the same byte from the four predecessor states kept as four bytes of one word (state j in byte j)
HSSFSST_DEC_HD inline unsigned pack_states(unsigned four) { return (four & 3u) | ((four >> 6) & 0xCu) | ((four >> 12) & 0x30u) | ((four >> 18) & 0xC0u); }

// the end: C = target T's candidates, E = E(T); the smallest j that attains the max
HSSFSST_DEC_HD inline unsigned end_state(const i64 C[4], const i64 E[4], i64* score)
{
    i64 best = add(C[0], E[0]);
    unsigned arg = 0;
    for (int j = 1; j < 4; ++j) {
        const i64 c = add(C[j], E[j]);
        if (c > best) { best = c; arg = static_cast<unsigned>(j); }
    }
    *score = best;
    return arg;
}

inline Tables quantise_tables(const float* A, const float* pi)
{
    Tables t;
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 4; ++j) t.A[i][j] = quantise(A[4 * i + j]);
        t.pi[i] = quantise(pi[i]);
    }
    return t;
}

// The specification: the sequential loop, in the pull form.  e (T, 4), A (4, 4), pi (4), dur, edge (4, D) float32; states (T)
// out; returns the score.
inline i64 decode_durations_reference(const float* e, i64 T, const float* A, const float* pi, const float* dur, const float* edge, int D,
                                      uint8_t* states)
{
    const Tables tb = quantise_tables(A, pi);
    const size_t n = static_cast<size_t>(T);
    std::vector<i64> B(4 * n), qd(4 * static_cast<size_t>(D)), qe(4 * static_cast<size_t>(D));
    std::vector<uint16_t> argd(4 * n, 0);
    std::vector<uint8_t> argi(n, 0);
    for (size_t k = 0; k < qd.size(); ++k) {
        qd[k] = quantise(dur[k]);
        qe[k] = quantise(edge[k]);
    }
    auto len = [&](const std::vector<i64>& tab, int j, i64 d) { return tab[static_cast<size_t>(j) * D + static_cast<size_t>(d - 1)]; };
    i64 E[4] = {0, 0, 0, 0};
    for (int j = 0; j < 4; ++j) B[j] = tb.pi[j];
    for (i64 t = 1; t < T; ++t) {
        for (int j = 0; j < 4; ++j) E[j] += quantise_emission(e[4 * (t - 1) + j]);
        i64 C[4];
        for (int j = 0; j < 4; ++j) {
            i64 best = kNeg;
            i64 arg = 1;
            for (i64 d = 1; d <= (t < D ? t : D); ++d) {
                const i64 c = add(B[4 * (t - d) + j], len(d == t ? qe : qd, j, d));
                if (c > best) { best = c; arg = d; }
            }
            C[j] = best;
            argd[4 * t + j] = static_cast<uint16_t>(arg);
        }
        argi[t] = static_cast<uint8_t>(run_starts(C, E, tb, &B[4 * t]));
    }
    for (int j = 0; j < 4; ++j) E[j] += quantise_emission(e[4 * (T - 1) + j]);
    i64 C[4], dend[4];
    for (int j = 0; j < 4; ++j) {
        C[j] = kNeg;
        dend[j] = 1;
        for (i64 d = 1; d <= (T < D ? T : D); ++d) {
            const i64 c = add(B[4 * (T - d) + j], len(qe, j, d));
            if (c > C[j]) { C[j] = c; dend[j] = d; }
        }
    }
    i64 score;
    unsigned s = end_state(C, E, &score);
    for (i64 t = 0; t < T; ++t) states[t] = 0;
    if (score == kNeg) return score;
    i64 t = T, d = dend[s];
    for (;;) {
        for (i64 u = t - d; u < t; ++u) states[u] = static_cast<uint8_t>(s);
        t -= d;
        if (t == 0) break;
        s = (argi[t] >> (2 * s)) & 3u;
        d = argd[4 * t + s];
    }
    return score;
}

}  // namespace hssfsst::durlayout
