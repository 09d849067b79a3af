// duration_counts_layout.hpp -- the expected run-length counts of the explicit-duration model (hssfsst.h:
// hssfsst_posteriors_durations_counts): the arithmetic, the ownership, the window and the workspace of the counts kernel
// (segmenter_duration_counts.hpp) as plain functions shared with a CPU check (tests/native/duration_counts_check.cpp).  No HIP call
// here.  Notation, scaled scalars (Sc) and the two sweeps: duration_posterior_layout.hpp's, which this file leaves as it is.
//
// The quantity.  A run of state j that starts at step t and lasts d steps (t + d <= T, 1 <= d <= D) has posterior
//   W(j, t, d) = b_t(j) L(j, d) g_(t+d)(j) / Z,      L = edge if t == 0 or t + d == T, else dur;  b_0 = exp pi;  g_T(j) = exp E_j(T)
// and counts[0][j][d - 1] = sum_t W over the interior runs, counts[1][j][d - 1] over the edge ones: the expected number of runs of j
// lasting exactly d steps, the gradient of logZ in dur and in edge, the E-step of the explicit-duration Baum-Welch.  WITH labels the
// output is counts - counts(label runs): a labelled run of state y and length d <= D takes 1 off (y, d) of the table that scores
// it; a labelled run longer than D takes nothing off.
//
// There is no recurrence: with the c_t of the forward sweep's stash and the g_u the runs variant of the sweep kernel leaves in a
// second stash, every (j, d) is a correlation of two sequences.  The arithmetic of one term:
//   value(mul(mul(b_t(j), g_(t+d)(j)), LZ)),   LZ = mul(L(j, d), 1 / Z)  formed once per (j, d) and table,
// b_t(j) = run_start(c_t, E(t), column j of P, j) as the forward sweep formed it (the same bits: the same c_t, the same E(t) summed from
// the segment's checkpoint in the forward order), added to a plain float64 accumulator in order of ASCENDING t; the label's 1 is
// taken off behind the term of the step the labelled run ends at.  duration_counts_reference() is that loop.
//
// Geometry.  One workgroup of kLanes lanes per recording and block of kDurationsPerGroup durations: lane l works for state l mod 4
// and the ONE duration kDurationsPerGroup block + l / 4 + 1.  It walks the recording in segments of kSegSteps steps t0 .. t0 + n - 1;
// per segment it stages the emissions, the stash rows t0 - 1 .. t0 + n - 2 (c_t is row t - 1; step 0 has none: b_0 = exp pi), E before
// the segment from its checkpoint, and the window of g rows window_first() .. + kWindowRows - 1 clipped to the recording (g_u is row
// u - 1): the lane's term of step t0 + q reads window row q + l / 4.
#pragma once

#include "duration_posterior_layout.hpp"

namespace hssfsst::dclayout {

namespace dp = dplayout;
using dp::i64;
using dp::Sc;

constexpr int kLanes = dp::kLanes;
constexpr int kDurationsPerGroup = kLanes / 4;           // one duration per lane and state
constexpr int kSegSteps = dp::kSegSteps;                 // the sweeps' segments: their checkpoints are the ones read here
constexpr int kWindowRows = kSegSteps + kDurationsPerGroup - 1;
static_assert(kSegSteps % kDurationsPerGroup == 0, "a lane forms kSegSteps / kDurationsPerGroup run starts of a segment");

HSSFSST_DEC_HD inline int groups(int D) { return (D + kDurationsPerGroup - 1) / kDurationsPerGroup; }
HSSFSST_DEC_HD inline int lane_state(int lane) { return lane & 3; }
HSSFSST_DEC_HD inline int lane_duration(int lane, int block) { return kDurationsPerGroup * block + (lane >> 2) + 1; }
// the g row (g_u is row u - 1) of the run that starts at step t and lasts d steps, the first row of a segment's window, and the
// window row the lane reads at the segment's step q
HSSFSST_DEC_HD inline i64 g_row(i64 t, int d) { return t + d - 1; }
HSSFSST_DEC_HD inline i64 window_first(i64 t0, int block) { return t0 + static_cast<i64>(kDurationsPerGroup) * block; }
HSSFSST_DEC_HD inline int window_row(int q, int lane) { return q + (lane >> 2); }
// counts (count, 2, 4, D): [recording][0 interior, 1 edge][state][d - 1]
HSSFSST_DEC_HD inline i64 counts_index(i64 rec, int which, int j, int d, int D) { return ((rec * 2 + which) * 4 + j) * static_cast<i64>(D) + (d - 1); }

// The workspace, 16-byte aligned: dplayout's, laid out as there, and behind its end
//   32 bytes per step        the mantissas of g_(r+1), four float64, row offsets[i] + r
//   16 bytes per step        their exponents, four int32
//   8 bytes per recording    the mantissa of 1 / Z
//   4 bytes per recording    its exponent
constexpr i64 kGBytesPerStep = 48;
constexpr i64 kInvzBytesPerRecording = 16;               // (12 used)
constexpr i64 kWorkBytesPerStep = dp::kWorkBytesPerStep + kGBytesPerStep;
constexpr i64 kWorkBytesPerRecording = dp::kWorkBytesPerRecording + kInvzBytesPerRecording;
constexpr i64 kWorkBytesPerDuration = dp::kWorkBytesPerDuration;
HSSFSST_DEC_HD inline i64 workspace_bytes(i64 total_steps, i64 count, int D)
{
    return kWorkBytesPerDuration * static_cast<i64>(D) + kWorkBytesPerStep * total_steps + kWorkBytesPerRecording * count;
}
struct Workspace { dp::Workspace sweeps; i64 g_mant, g_exp, invz_mant, invz_exp, end; };     // byte offsets
HSSFSST_DEC_HD inline Workspace workspace(i64 total_steps, i64 count, int D)
{
    Workspace w;
    w.sweeps = dp::workspace(total_steps, count, D);
    w.g_mant = w.sweeps.end;                             // (a multiple of 16: every part before it is)
    w.g_exp = w.g_mant + 32 * total_steps;
    w.invz_mant = w.g_exp + 16 * total_steps;
    w.invz_exp = w.invz_mant + 8 * count;
    w.end = w.invz_exp + 4 * count;
    return w;
}

// one term: the posterior of the run that starts with b and ends before g, LZ = L / Z
HSSFSST_DEC_HD inline double run_weight(Sc b, Sc g, Sc LZ) { return dp::value(dp::mul(dp::mul(b, g), LZ)); }
// does the run (t, d) of a recording of T steps pay edge?
HSSFSST_DEC_HD inline bool at_edge(i64 t, int d, i64 T) { return t == 0 || t + d == T; }

// The labelled segmentation at step r: does a run end behind it?  If so *len <- its length, *edge <- whether it pays edge, and
// *start moves on (label_terms' walk, without the score).
HSSFSST_DEC_HD inline bool label_run_ends(int y, int ynext, i64 r, i64 T, i64* start, i64* len, bool* edge)
{
    if (!(r + 1 == T || ynext != y)) return false;
    *len = r + 1 - *start;
    *edge = *start == 0 || r + 1 == T;
    *start = r + 1;
    return true;
}

// The specification: the sequential loops, adding in the kernel's order.  Arguments as duration_posteriors_reference; counts
// (2, 4, D) out.  Returns that function's Result: the first seven outputs are its, untouched.
template <class G>
inline dp::Result duration_counts_reference(const float* e, i64 T, const float* a_pi, const float* dur, const float* edge, int D,
                                            const uint8_t* labels, G* gamma, G* onsets, double* counts)
{
    const dp::Result out = dp::duration_posteriors_reference(e, T, a_pi, dur, edge, D, labels, gamma, onsets);
    const size_t n = static_cast<size_t>(T), nd = static_cast<size_t>(D);
    dp::StateTables st[4];
    for (int j = 0; j < 4; ++j) st[j] = dp::state_tables(a_pi, j);
    std::vector<Sc> Ld(4 * nd), Le(4 * nd);              // [j D + d - 1]
    for (size_t k = 0; k < 4 * nd; ++k) {
        Ld[k] = dp::scaled_exp(static_cast<double>(dur[k]));
        Le[k] = dp::scaled_exp(static_cast<double>(edge[k]));
    }
    auto len = [&](bool edge_run, int j, i64 d) { return (edge_run ? Le : Ld)[static_cast<size_t>(j) * nd + static_cast<size_t>(d - 1)]; };
    std::vector<double> E(4 * (n + 1), 0.0);
    for (size_t t = 0; t < n; ++t)
        for (int j = 0; j < 4; ++j) E[4 * (t + 1) + j] = E[4 * t + j] + dp::emission(e[4 * t + j]);
    // b, c, g as duration_posteriors_reference forms them
    std::vector<Sc> b(4 * n), c(4 * (n + 1)), g(4 * (n + 1)), cb(4 * n);
    for (int j = 0; j < 4; ++j) b[j] = st[j].p0;
    for (i64 t = 1; t <= T; ++t) {
        for (int j = 0; j < 4; ++j) {
            Sc acc = dp::zero();
            for (i64 d = t < D ? t : D; d >= 1; --d) acc = dp::add(acc, dp::mul(b[4 * (t - d) + j], len(t - d == 0 || t == T, j, d)));
            c[4 * t + j] = dp::norm(acc);
        }
        if (t < T)
            for (int j = 0; j < 4; ++j) b[4 * t + j] = dp::run_start(&c[4 * t], &E[4 * t], st[j].col, j);
    }
    const Sc invz = dp::inverse(dp::total(&c[4 * T], &E[4 * T]));
    for (int j = 0; j < 4; ++j) g[4 * T + j] = dp::scaled_exp(E[4 * T + j]);
    for (i64 t = T - 1; t >= 1; --t) {
        for (int j = 0; j < 4; ++j) {
            Sc acc = dp::zero();
            for (i64 d = T - t < D ? T - t : D; d >= 1; --d) acc = dp::add(acc, dp::mul(g[4 * (t + d) + j], len(t + d == T, j, d)));
            cb[4 * t + j] = dp::norm(acc);
        }
        for (int i = 0; i < 4; ++i) g[4 * t + i] = dp::run_end(&cb[4 * t], &E[4 * t], st[i].row, i);
    }
    for (int j = 0; j < 4; ++j)
        for (int d = 1; d <= D; ++d) {
            const Sc lz[2] = {dp::mul(len(false, j, d), invz), dp::mul(len(true, j, d), invz)};
            double acc[2] = {0.0, 0.0};
            i64 start = 0;
            for (i64 t = 0; t < T; ++t) {
                if (t + d <= T) {
                    const int which = at_edge(t, d, T) ? 1 : 0;
                    acc[which] += run_weight(b[4 * t + j], g[4 * (t + d) + j], lz[which]);
                }
                if (labels) {
                    i64 run;
                    bool edge_run;
                    const int y = labels[t] & 3, yn = t + 1 < T ? labels[t + 1] & 3 : -1;
                    if (label_run_ends(y, yn, t, T, &start, &run, &edge_run) && y == j && run == d) acc[edge_run ? 1 : 0] -= 1.0;
                }
            }
            counts[counts_index(0, 0, j, d, D)] = acc[0];
            counts[counts_index(0, 1, j, d, D)] = acc[1];
        }
    return out;
}

}  // namespace hssfsst::dclayout
