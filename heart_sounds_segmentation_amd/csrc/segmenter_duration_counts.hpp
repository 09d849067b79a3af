// segmenter_duration_counts.hpp -- the expected run-length counts of the explicit-duration model (hssfsst.h:
// hssfsst_posteriors_durations_counts): N[j][d] = E[number of runs of state j lasting exactly d steps], kept apart for interior runs
// (scored by dur) and for the first and the last run (scored by edge) -- the gradient of logZ in the two tables.  The arithmetic, the
// ownership, the window and the order of every sum are csrc/duration_counts_layout.hpp's; this file is the workgroup around them.
//
// It runs behind seg_duration_runs_sweep_kernel (segmenter_duration_posteriors.hpp), which leaves c_t, the checkpoints of E, g_u and
// 1 / Z in the workspace.  There is no recurrence left: one workgroup of kLanes lanes per recording and block of 128 durations, lane l
// for state l mod 4 and ONE duration.  The workgroup walks the recording's steps in ascending order, a segment of kSegSteps at a
// time: it stages the segment's emissions and c rows, rebuilds E(t) from the checkpoint in the forward order (lanes 0 .. 3), forms
// b_t(j) once per step and state into LDS (two per lane), stages the window of g rows the segment's runs end in, and then every lane
// adds its term of each step to one of two float64 accumulators.  Nobody waits for another workgroup, nothing is atomic: a
// recording's counts do not depend on its neighbours, bit for bit.  A lane's state is a run-time number: no array is indexed by it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "duration_counts_layout.hpp"
#include "segmenter_duration_posteriors.hpp"

namespace hssfsst {

__global__ __launch_bounds__(dclayout::kLanes) void seg_duration_run_counts_kernel(
    const float* __restrict__ logp, const float* __restrict__ a_pi, const uint8_t* __restrict__ labels, double* __restrict__ counts,
    const double* __restrict__ tabm, const int* __restrict__ tabe, const double* __restrict__ stash_m, const int* __restrict__ stash_e,
    const double* __restrict__ checkpoints, const DurRunsOut runs, const DurPostArgs args)
{
    namespace dp = dplayout;
    namespace dc = dclayout;
    using dp::i64;
    using dp::Sc;
    constexpr int kSeg = dc::kSegSteps;
    __shared__ __attribute__((aligned(16))) float est[kSeg][4];          // a segment's emissions
    __shared__ __attribute__((aligned(16))) double Est[kSeg][4];         // E(t0 + q): before the row
    __shared__ __attribute__((aligned(16))) double cstm[kSeg][4];        // c_(t0+q): stash row t0 + q - 1
    __shared__ __attribute__((aligned(16))) int cste[kSeg][4];
    __shared__ __attribute__((aligned(16))) double bstm[kSeg][4];        // b_(t0+q)
    __shared__ __attribute__((aligned(16))) int bste[kSeg][4];
    __shared__ __attribute__((aligned(16))) double gwm[dc::kWindowRows][4];      // g rows window_first() ..
    __shared__ __attribute__((aligned(16))) int gwe[dc::kWindowRows][4];
    __shared__ uint8_t lst[kSeg + 4];                                    // labels of the rows and of the one behind them
    __shared__ double tblm[20];                                          // exp of {A row-major, pi}
    __shared__ int tble[20];

    const int tid = static_cast<int>(threadIdx.x), j = dc::lane_state(tid);
    const int D = args.D, block = static_cast<int>(blockIdx.y), d = dc::lane_duration(tid, block);
    const bool owner = d <= D;                           // the others idle: they stage, and wait at the barriers
    const i64 base = args.off[blockIdx.x];
    const int T = static_cast<int>(args.off[blockIdx.x + 1] - base);     // <= kMaxSteps
    double* out0 = counts + dc::counts_index(static_cast<i64>(blockIdx.x), 0, j, owner ? d : 1, D);
    double* out1 = counts + dc::counts_index(static_cast<i64>(blockIdx.x), 1, j, owner ? d : 1, D);
    const uint8_t* lab = labels ? labels + base : nullptr;
    if (dc::lane_duration(0, block) > T) {               // (uniform) no run of this block's durations fits, nor does a labelled one
        if (owner) {
            *out0 = 0.0;
            *out1 = 0.0;
        }
        return;
    }
    const float4* e4 = reinterpret_cast<const float4*>(logp) + base;
    const double* sm = stash_m + 4 * base;
    const int* se = stash_e + 4 * base;
    const double* gm = runs.g_m + 4 * base;
    const int* ge = runs.g_e + 4 * base;
    const double* ckpt = checkpoints + 4 * dp::checkpoint_slot(base, args.rec0 + blockIdx.x);

    if (tid < 20) {                                      // (state_tables(), one entry per lane; the diagonal of A is zero)
        const Sc x = tid < 16 && tid / 4 == tid % 4 ? dp::zero() : dp::scaled_exp(static_cast<double>(a_pi[tid]));
        tblm[tid] = x.m;
        tble[tid] = x.e;
    }
    const Sc invz{runs.invz_m[blockIdx.x], runs.invz_e[blockIdx.x]};
    Sc lzd = dp::zero(), lze = dp::zero();               // L / Z of the lane's duration: interior, edge
    if (owner) {
        const i64 at = dp::table_index(0, d, j, D), tedge = dp::table_index(1, 1, 0, D);
        lzd = dp::mul(Sc{tabm[at], tabe[at]}, invz);
        lze = dp::mul(Sc{tabm[tedge + at], tabe[tedge + at]}, invz);
    }
    double acc0 = 0.0, acc1 = 0.0;                       // interior, edge
    i64 run_first = 0;                                   // the labelled run's start: the same in every lane

    for (int t0 = 0; t0 < T; t0 += kSeg) {
        const int n = T - t0 < kSeg ? T - t0 : kSeg;
        __syncthreads();                                 // the stages are free (and, the first time, the tables are there)
        for (int q = tid; q < n; q += dc::kLanes) {
            *reinterpret_cast<float4*>(est[q]) = e4[t0 + q];
            if (t0 + q >= 1) {                           // c_(t0+q); step 0 has none
                const double* qm = sm + 4 * static_cast<i64>(t0 + q - 1);
                *reinterpret_cast<double2*>(cstm[q]) = *reinterpret_cast<const double2*>(qm);
                *reinterpret_cast<double2*>(cstm[q] + 2) = *reinterpret_cast<const double2*>(qm + 2);
                *reinterpret_cast<int4*>(cste[q]) = *reinterpret_cast<const int4*>(se + 4 * static_cast<i64>(t0 + q - 1));
            }
        }
        {
            const i64 first = dc::window_first(t0, block);
            for (int w = tid; w < dc::kWindowRows && first + w < T; w += dc::kLanes) {
                const double* qm = gm + 4 * (first + w);
                *reinterpret_cast<double2*>(gwm[w]) = *reinterpret_cast<const double2*>(qm);
                *reinterpret_cast<double2*>(gwm[w] + 2) = *reinterpret_cast<const double2*>(qm + 2);
                *reinterpret_cast<int4*>(gwe[w]) = *reinterpret_cast<const int4*>(ge + 4 * (first + w));
            }
        }
        if (lab)
            for (int q = tid; q <= n && t0 + q < T; q += dc::kLanes) lst[q] = lab[t0 + q];
        __syncthreads();
        if (tid < 4) {                                   // E(t0 + q), summed as the forward sweep summed them
            double acc = ckpt[4 * (t0 / kSeg) + j];
            for (int q = 0; q < n; ++q) {
                Est[q][j] = acc;
                acc += dp::emission(est[q][j]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSeg / dc::kDurationsPerGroup; ++k) {        // b_(t0+q)(j), once per step and state
            const int q = (tid >> 2) + k * dc::kDurationsPerGroup;
            if (q < n) {
                Sc b{tblm[16 + j], tble[16 + j]};
                if (t0 + q >= 1) {
                    const double2 a = *reinterpret_cast<const double2*>(Est[q]), c = *reinterpret_cast<const double2*>(Est[q] + 2);
                    const double E[4] = {a.x, a.y, c.x, c.y};
                    const double2 ma = *reinterpret_cast<const double2*>(cstm[q]), mc = *reinterpret_cast<const double2*>(cstm[q] + 2);
                    const int4 x = *reinterpret_cast<const int4*>(cste[q]);
                    const Sc C[4] = {Sc{ma.x, x.x}, Sc{ma.y, x.y}, Sc{mc.x, x.z}, Sc{mc.y, x.w}};
                    Sc col[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) col[i] = Sc{tblm[4 * i + j], tble[4 * i + j]};
                    b = dp::run_start(C, E, col, j);
                }
                bstm[q][j] = b.m;
                bste[q][j] = b.e;
            }
        }
        __syncthreads();
        for (int q = 0; q < n; ++q) {
            const int t = t0 + q;
            if (owner && t + d <= T) {
                const int w = dc::window_row(q, tid);    // g row t + d - 1, less the window's first
                const Sc b{bstm[q][j], bste[q][j]}, g{gwm[w][j], gwe[w][j]};
                const bool edge_run = dc::at_edge(t, d, T);
                const double v = dc::run_weight(b, g, edge_run ? lze : lzd);
                acc0 += edge_run ? 0.0 : v;
                acc1 += edge_run ? v : 0.0;
            }
            if (lab) {
                i64 run;
                bool edge_run;
                const int y = lst[q] & 3, yn = t + 1 < T ? lst[q + 1] & 3 : -1;
                if (dc::label_run_ends(y, yn, t, T, &run_first, &run, &edge_run) && owner && y == j && run == d) {
                    if (edge_run) acc1 -= 1.0; else acc0 -= 1.0;
                }
            }
        }
    }
    if (owner) {
        *out0 = acc0;
        *out1 = acc1;
    }
}

}  // namespace hssfsst
