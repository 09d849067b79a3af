// stitch_layout.hpp -- stitching overlapping windows' log-probs back into one sequence per recording (hssfsst.h:
// hssfsst_stitch_windows): the covering window set, where a window's rows lie, the covering windows of a step, the arithmetic of
// one step and a sequential reference of the whole call, as plain functions shared by the kernel (segmenter_stitch.hpp), the entry
// (sequence.hip) and a CPU check (tests/native/stitch_layout_check.cpp).  No HIP call here.  stitch_reference() is the
// specification: the kernel runs stitch_step() on the same rows in the same order.
//
// The window set.  A recording of T >= 1 steps, windows of n >= 1 steps, 1 <= stride <= n:
//   T <= n   one window [0, T)
//   T >  n   the R = floor((T - n) / stride) + 1 regular windows [i stride, i stride + n), i = 0 .. R - 1, and, if
//            (T - n) % stride != 0, one tail window [T - n, T), which is window R
// Every step is covered; the tail starts after the last regular window, so ascending window index is ascending start.  A step has
// at most ceil(n / stride) regular covering windows, and the tail: kMaxCover with ceil(n / stride) <= kMaxRatio.
//
// The rows.  A recording's windows lie back to back from row win_first on: window k of a T > n recording takes rows
// win_first + k n .. + n, position p of it is step start(k) + p; the one window of a T <= n recording takes T rows.
//
// One step.  Its covering windows in ascending start order are k = 1 .. m, window k gives the row v_k (four float32) at its position
// p_k, with weight w_k = w[p_k] (1 without weights).
//   m == 1, or SELECT   a row is copied bit for bit; SELECT takes the largest w_k, ties to the earlier start
//   PROB                M = the largest of the 4 m values; a_j = log(sum_k w_k exp(v_kj - M) / sum_k w_k) + M
//   LOGP                a_j = sum_k w_k v_kj / sum_k w_k
//   both                out_j = a_j - logsumexp_j(a), float64 throughout, sums over k in ascending order, rounded to float32 once
// and IEEE rules do the rest: a NaN among the values makes the four outputs NaN, a class that is -inf in every window (PROB) or in
// any (LOGP) comes out -inf, a step without mass gives four NaN.  dissent = the number of covering windows whose own argmax differs
// from the argmax of the float32 output; the argmax is the scorer's (score_layout.hpp: ties to the smaller state, NaN as -inf).
#pragma once

#include <cmath>
#include <cstdint>

#include "score_layout.hpp"                              // argmax4, HSSFSST_DEC_HD

namespace hssfsst::stitchlayout {

using i64 = long long;

constexpr int kProb = 0, kLogp = 1, kSelect = 2;         // HSSFSST_STITCH_*
constexpr int kMaxRatio = 15;                            // ceil(n / stride) at most
constexpr int kMaxCover = kMaxRatio + 1;                 // covering windows of a step at most
constexpr int kStitchBatch = 256;                        // recordings of a launch: their descriptors travel as kernel arguments
constexpr int kThreads = 256;                            // lanes of a workgroup, one step each

HSSFSST_DEC_HD inline int ratio(int n, int stride) { return (n + stride - 1) / stride; }
HSSFSST_DEC_HD inline bool supported(int n, int stride) { return ratio(n, stride) <= kMaxRatio; }

// ---- the window set ---------------------------------------------------------------------------------------------------------------
HSSFSST_DEC_HD inline i64 regular_windows(i64 T, int n, int stride) { return T <= n ? 1 : (T - n) / stride + 1; }
HSSFSST_DEC_HD inline bool has_tail(i64 T, int n, int stride) { return T > n && (T - n) % stride != 0; }
HSSFSST_DEC_HD inline i64 window_count(i64 T, int n, int stride) { return regular_windows(T, n, stride) + (has_tail(T, n, stride) ? 1 : 0); }
HSSFSST_DEC_HD inline i64 window_start(i64 k, i64 T, int n, int stride)
{
    return T <= n ? 0 : k < regular_windows(T, n, stride) ? k * stride : T - n;
}
HSSFSST_DEC_HD inline i64 window_len(i64 T, int n) { return T <= n ? T : n; }
// the rows a recording's windows take in the arena
HSSFSST_DEC_HD inline i64 window_rows(i64 T, int n, int stride) { return T <= n ? T : window_count(T, n, stride) * n; }
inline i64 launch_groups(i64 steps) { return (steps + kThreads - 1) / kThreads; }

// The covering windows of step t, in ascending start order: the regular windows lo .. lo + regular - 1, then the tail (window R).
struct Cover {
    i64 lo;
    int regular;
    bool tail;
    i64 R;
};
HSSFSST_DEC_HD inline Cover cover_of(i64 t, i64 T, int n, int stride)
{
    if (T <= n) return {0, 1, false, 1};
    const i64 R = regular_windows(T, n, stride);
    const i64 lo = t >= n ? (t - n) / stride + 1 : 0;    // the first i with i stride + n > t
    const i64 last = t / stride < R - 1 ? t / stride : R - 1;                        // the last i < R with i stride <= t
    return {lo, last >= lo ? static_cast<int>(last - lo + 1) : 0, has_tail(T, n, stride) && t >= T - n, R};
}
HSSFSST_DEC_HD inline int cover_size(const Cover& c) { return c.regular + (c.tail ? 1 : 0); }
HSSFSST_DEC_HD inline i64 cover_window(const Cover& c, int k) { return k < c.regular ? c.lo + k : c.R; }

// ---- one step -----------------------------------------------------------------------------------------------------------------------
struct Row {
    float v[4];
};
struct Step {
    Row out;                                             // the float32 result
    double pooled[4];                                    // the same before its rounding (of a copied row: its values)
    int dissent;
};

HSSFSST_DEC_HD inline double neg_inf() { return -__builtin_huge_val(); }

// a -> a - logsumexp(a)
HSSFSST_DEC_HD inline void normalise(double* a)
{
    double top = neg_inf();
    for (int j = 0; j < 4; ++j) top = a[j] > top ? a[j] : top;
    double sum = 0.0;
    for (int j = 0; j < 4; ++j) sum += std::exp(a[j] - top);
    const double lse = top + std::log(sum);
    for (int j = 0; j < 4; ++j) a[j] -= lse;
}

// row(k) -> the Row of covering window k, weight(k) -> its weight as a float; k = 0 .. m - 1 in ascending start order.  Both may
// be called more than once per k: the kernel loads again what it does not keep.
template <class RowOf, class WeightOf>
HSSFSST_DEC_HD inline Step stitch_step(int m, int mode, RowOf row, WeightOf weight, bool want_dissent)
{
    Step s{};
    if (m == 1 || mode == kSelect) {
        int pick = 0;
        float best = weight(0);
        for (int k = 1; k < m; ++k) {
            const float w = weight(k);
            if (w > best) { best = w; pick = k; }
        }
        s.out = row(pick);
        for (int j = 0; j < 4; ++j) s.pooled[j] = static_cast<double>(s.out.v[j]);
    } else {
        double a[4] = {0.0, 0.0, 0.0, 0.0}, wsum = 0.0;
        if (mode == kProb) {
            double top = neg_inf();
            for (int k = 0; k < m; ++k) {
                const Row r = row(k);
                for (int j = 0; j < 4; ++j) top = static_cast<double>(r.v[j]) > top ? static_cast<double>(r.v[j]) : top;
            }
            for (int k = 0; k < m; ++k) {
                const Row r = row(k);
                const double w = static_cast<double>(weight(k));
                wsum += w;
                for (int j = 0; j < 4; ++j) a[j] += w * std::exp(static_cast<double>(r.v[j]) - top);
            }
            for (int j = 0; j < 4; ++j) a[j] = std::log(a[j] / wsum) + top;
        } else {
            for (int k = 0; k < m; ++k) {
                const Row r = row(k);
                const double w = static_cast<double>(weight(k));
                wsum += w;
                for (int j = 0; j < 4; ++j) a[j] += w * static_cast<double>(r.v[j]);
            }
            for (int j = 0; j < 4; ++j) a[j] /= wsum;
        }
        normalise(a);
        for (int j = 0; j < 4; ++j) {
            s.pooled[j] = a[j];
            s.out.v[j] = static_cast<float>(a[j]);
        }
    }
    if (want_dissent) {
        const int own = scorelayout::argmax4(s.out.v);
        for (int k = 0; k < m; ++k) {
            const Row r = row(k);
            s.dissent += scorelayout::argmax4(r.v) != own ? 1 : 0;
        }
    }
    return s;
}

// ---- the sequential reference: the specification ------------------------------------------------------------------------------------
// win (win rows, 4), win_first (count), offsets (count + 1), weights (n) or nullptr -> out (sum T, 4), pooled (sum T, 4) float64 or
// nullptr, dissent (sum T) or nullptr.  The arguments are the entry's, checked by it.
inline void stitch_reference(const float* win, const int64_t* win_first, const int64_t* offsets, int64_t count, int n, int stride,
                             const float* weights, int mode, float* out, double* pooled, uint8_t* dissent)
{
    for (int64_t r = 0; r < count; ++r) {
        const i64 T = offsets[r + 1] - offsets[r];
        for (i64 t = 0; t < T; ++t) {
            const Cover c = cover_of(t, T, n, stride);
            auto position = [&](int k) { return t - window_start(cover_window(c, k), T, n, stride); };
            auto row = [&](int k) {
                const float* p = win + 4 * (win_first[r] + cover_window(c, k) * n + position(k));
                return Row{{p[0], p[1], p[2], p[3]}};
            };
            auto weight = [&](int k) { return weights ? weights[position(k)] : 1.0f; };
            const Step s = stitch_step(cover_size(c), mode, row, weight, dissent != nullptr);
            const i64 at = offsets[r] + t;
            for (int j = 0; j < 4; ++j) {
                out[4 * at + j] = s.out.v[j];
                if (pooled) pooled[4 * at + j] = s.pooled[j];
            }
            if (dissent) dissent[at] = static_cast<uint8_t>(s.dissent);
        }
    }
}

}  // namespace hssfsst::stitchlayout
