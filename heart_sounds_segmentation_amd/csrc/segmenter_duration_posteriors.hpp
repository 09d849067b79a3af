// segmenter_duration_posteriors.hpp -- forward-backward over the segmenter's log-probs under the explicit-duration (semi-Markov)
// model of hssfsst_decode_durations (hssfsst.h: hssfsst_posteriors_durations): the per-step state posteriors gamma, logZ, the
// expected run changes Xi, the step-0 posterior, the run-onset posteriors and, with labels, the labelled segmentation's score and
// the gradients of logZ - score.  The arithmetic (float64 mantissas with int exponents, linear domain), the order of every sum and
// the geometry are csrc/duration_posterior_layout.hpp's; this file is the workgroup around them.
//
// One workgroup of kLanes lanes per recording, no workgroup waits for another; every loop is bounded by T and D.  Lane l works for
// state j = l mod 4 and holds the linear dur values of the up to kPerLane durations it owns in registers for the whole recording.
//   Forward, sources r = 0 .. T - 1, one __syncthreads() per step: the lane pushes b_r(j) L(j, d) into the ring words of the targets
//   r + d (the first writer of a word stores, a later one adds), and behind the barrier reads the four words of target r + 1 -- c_(r+1)
//   -- and forms b_(r+1)(j) from them and the prefix sums E(r + 1) it carries in registers.  Source 0 and the source that reaches
//   target T push edge (read from the table).  The emissions are staged kSegSteps steps at a time; the c of a segment are kept in
//   LDS for as long and then written to the workspace by all lanes, and E before the segment goes to its checkpoint.  Lane 0 adds up
//   the labelled segmentation's score on the way.
//   Reverse, sources u = T .. 1, the same push from the other end: g_u(j) L(j, d) into the targets u - d.  A segment's c come back
//   from the workspace, its E(u) from the checkpoint and the staged emissions (lanes 0 .. 3, one state each, in the forward order).
//   Every step forms N_u, the Xi terms, S_u and the running gamma; gamma and the onsets are staged and written float4 by float4.
// A lane's state is a run-time number: vectors are indexed by selects (pick4) and unrolled loops, never by it: no scratch.
// The body is seg_duration_sweeps<kRuns>; seg_duration_posteriors_kernel is its plain instantiation, and
// seg_duration_runs_sweep_kernel the one that also stores g_u and 1 / Z for the run-length counts (segmenter_duration_counts.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "duration_posterior_layout.hpp"

namespace hssfsst {

constexpr int kDurPostBatch = 256;                       // recordings per launch: their offsets travel as kernel arguments
constexpr int kDurPostFillLanes = 256;

struct DurPostArgs {
    long long off[kDurPostBatch + 1];                    // step offsets of the launch's recordings in the arenas
    long long rec0;                                      // the first one's number in the list (its checkpoint slots)
    int D;
};

// the two (4, D) log tables -> the linear tables of the workspace, one value per lane
__global__ __launch_bounds__(kDurPostFillLanes) void seg_duration_posteriors_fill_kernel(const float* __restrict__ dur,
                                                                                       const float* __restrict__ edge,
                                                                                       double* __restrict__ tabm, int* __restrict__ tabe, int D)
{
    namespace dp = dplayout;
    const int s = static_cast<int>(blockIdx.x) * kDurPostFillLanes + static_cast<int>(threadIdx.x);
    if (s >= 8 * D) return;
    const float v = s < 4 * D ? dur[s] : edge[s - 4 * D];
    const dp::Sc x = dp::scaled_exp(static_cast<double>(v));
    const long long at = dp::table_index_of_source(s, D);
    tabm[at] = x.m;
    tabe[at] = x.e;
}

// what the runs variant of the sweeps leaves for the counts kernel (segmenter_duration_counts.hpp; the layout is
// csrc/duration_counts_layout.hpp's): g_u(j), u = T .. 1, in row u - 1 of a second stash, and 1 / Z of each recording of the launch
struct DurRunsOut {
    double* g_m;
    int* g_e;
    double* invz_m;
    int* invz_e;
};

// Both sweeps of one recording.  kRuns: also leave DurRunsOut -- every other output is bit for bit that of the plain instantiation.
// static and NOT __forceinline__: each instantiation has one caller, so the inliner folds it into its kernel anyway (no call is
// left), but after the body has been simplified on its own -- which gives the plain kernel the code it had as a kernel body (the
// same instruction mix to three instructions).  Forced inlining happens before that and cost 3.5 % at D = 2048 (more SGPR spills).
template <bool kRuns>
static __device__ void seg_duration_sweeps(
    const float* __restrict__ logp, const float* __restrict__ a_pi, const float* __restrict__ dur, const float* __restrict__ edge,
    const uint8_t* __restrict__ labels, float* __restrict__ gamma, float* __restrict__ onsets, double* __restrict__ loglik,
    double* __restrict__ score, double* __restrict__ xi_out, double* __restrict__ s0_out, const double* __restrict__ tabm,
    const int* __restrict__ tabe, double* __restrict__ stash_m, int* __restrict__ stash_e, double* __restrict__ checkpoints,
    const DurPostArgs& args, const DurRunsOut runs)
{
    namespace dp = dplayout;
    using dp::i64;
    using dp::Sc;
    constexpr int kSeg = dp::kSegSteps;
    __shared__ __attribute__((aligned(16))) double ringm[dp::kMaxRing][4];
    __shared__ __attribute__((aligned(16))) int ringe[dp::kMaxRing][4];
    __shared__ __attribute__((aligned(16))) float est[kSeg][4];          // a segment's emissions
    __shared__ __attribute__((aligned(16))) double Est[kSeg][4];         // reverse: E(r + 1) of the segment's rows
    __shared__ __attribute__((aligned(16))) double cstm[kSeg][4];        // c_(r+1): mantissas ...
    __shared__ __attribute__((aligned(16))) int cste[kSeg][4];           // ... and exponents
    __shared__ __attribute__((aligned(16))) float gst[kSeg][4];          // reverse: gamma of the segment's rows ...
    __shared__ __attribute__((aligned(16))) float ost[kSeg][4];          // ... and the onsets of the rows one further
    __shared__ uint8_t lst[kSeg + 4];                                    // labels of the rows and of the one behind them
    __shared__ double xis[4][4];                                         // Xi so far: column j is lane j's
    __shared__ double tblm[20];                                          // exp of {A row-major, pi}: read where it is used, not held
    __shared__ int tble[20];                                             // in 60 registers over both sweeps

    const int tid = static_cast<int>(threadIdx.x), j = dp::lane_state(tid);
    const int D = args.D, R = dp::ring_slots(D);
    const i64 base = args.off[blockIdx.x];
    const int T = static_cast<int>(args.off[blockIdx.x + 1] - base);     // <= kMaxSteps
    const float4* e4 = reinterpret_cast<const float4*>(logp) + base;
    const uint8_t* lab = labels ? labels + base : nullptr;
    double* sm = stash_m + 4 * base;
    int* se = stash_e + 4 * base;
    double* ckpt = checkpoints + 4 * dp::checkpoint_slot(base, args.rec0 + blockIdx.x);
    const i64 tedge = dp::table_index(1, 1, 0, D);

    if (tid < 20) {                                      // (state_tables(), one entry per lane; the diagonal of A is zero)
        const Sc x = tid < 16 && tid / 4 == tid % 4 ? dp::zero() : dp::scaled_exp(static_cast<double>(a_pi[tid]));
        tblm[tid] = x.m;
        tble[tid] = x.e;
    }
    __syncthreads();
    auto column = [&](Sc col[4]) {                       // col[i] = P[i][j]
#pragma unroll
        for (int i = 0; i < 4; ++i) col[i] = Sc{tblm[4 * i + j], tble[4 * i + j]};
    };
    auto row_of = [&](Sc row[4]) {                       // row[i] = P[j][i]
#pragma unroll
        for (int i = 0; i < 4; ++i) row[i] = Sc{tblm[4 * j + i], tble[4 * j + i]};
    };
    double durm[dp::kPerLane];
    int dure[dp::kPerLane];
#pragma unroll
    for (int k = 0; k < dp::kPerLane; ++k) {
        const int d = dp::lane_duration(tid, k);
        durm[k] = d <= D ? tabm[dp::table_index(0, d, j, D)] : 0.0;
        dure[k] = d <= D ? tabe[dp::table_index(0, d, j, D)] : dp::kZeroExp;
    }

    // x L(j, d) of the owned durations into the ring words of the targets d steps on, of which `left` remain; at_end: this source is
    // the recording's end (0 or T) and pushes edge throughout; a target that is the other end takes edge as well
    auto push = [&](Sc x, int cur, int left, bool at_end) {
#pragma unroll
        for (int k = 0; k < dp::kPerLane; ++k) {
            if (dp::lane_duration(0, k) > D) break;      // (uniform: nobody owns a duration of this chunk)
            const int d = dp::lane_duration(tid, k);
            if (d <= D && d <= left) {
                Sc L{durm[k], dure[k]};
                if (at_end || d == left) {
                    const i64 at = tedge + dp::table_index(0, d, j, D);
                    L = Sc{tabm[at], tabe[at]};
                }
                Sc w = dp::mul(x, L);
                const int slot = dp::ring_slot(cur, d, R);
                if (!(at_end || d == D)) w = dp::add(Sc{ringm[slot][j], ringe[slot][j]}, w);
                ringm[slot][j] = w.m;
                ringe[slot][j] = w.e;
            }
        }
    };
    auto ring_read = [&](int cur, Sc C[4]) {
        const double2 a = *reinterpret_cast<const double2*>(ringm[cur]), b = *reinterpret_cast<const double2*>(ringm[cur] + 2);
        const int4 x = *reinterpret_cast<const int4*>(ringe[cur]);
        C[0] = dp::norm(Sc{a.x, x.x});
        C[1] = dp::norm(Sc{a.y, x.y});
        C[2] = dp::norm(Sc{b.x, x.z});
        C[3] = dp::norm(Sc{b.y, x.w});
    };

    // ---- forward sweep
    double E[4] = {0.0, 0.0, 0.0, 0.0};                  // E(r): the same in every lane
    Sc b{tblm[16 + j], tble[16 + j]};
    Sc C[4];
    int cur = 0;                                         // r mod R
    double sc = 0.0;                                     // lane 0: the labelled segmentation's score
    i64 run_first = 0;
    if (lab && tid == 0) sc = static_cast<double>(a_pi[16 + (lab[0] & 3)]);
    auto flush_stash = [&](int first, int n) {           // rows first .. first + n - 1, all of one segment
        for (int s = tid; s < n; s += dp::kLanes) {
            double* qm = sm + 4 * static_cast<i64>(first + s);
            *reinterpret_cast<double2*>(qm) = *reinterpret_cast<const double2*>(cstm[s]);
            *reinterpret_cast<double2*>(qm + 2) = *reinterpret_cast<const double2*>(cstm[s] + 2);
            *reinterpret_cast<int4*>(se + 4 * static_cast<i64>(first + s)) = *reinterpret_cast<const int4*>(cste[s]);
        }
    };
    for (int r = 0; r < T; ++r) {
        const int s = r % kSeg;
        if (s == 0) {
            if (r > 0) {
                __syncthreads();                         // the last row's c is in the stage
                flush_stash(r - kSeg, kSeg);
            }
            if (tid < 4) ckpt[4 * (r / kSeg) + j] = dp::pick4(E, j);
            const int left = T - r;
            for (int q = tid; q < kSeg && q < left; q += dp::kLanes) *reinterpret_cast<float4*>(est[q]) = e4[r + q];
            if (lab)
                for (int q = tid; q <= kSeg && q < left; q += dp::kLanes) lst[q] = lab[r + q];
            __syncthreads();
        }
        push(b, cur, T - r, r == 0);
        const float4 v = *reinterpret_cast<const float4*>(est[s]);
        if (lab && tid == 0) {
            const int y = lst[s] & 3, yn = r + 1 < T ? lst[s + 1] & 3 : -1;
            const float ev = y == 0 ? v.x : y == 1 ? v.y : y == 2 ? v.z : v.w;
            sc += dp::label_terms(dp::emission(ev), y, yn, r, T, &run_first, a_pi, dur, edge, D);
        }
        E[0] += dp::emission(v.x);
        E[1] += dp::emission(v.y);
        E[2] += dp::emission(v.z);
        E[3] += dp::emission(v.w);
        cur = cur + 1 == R ? 0 : cur + 1;
        __syncthreads();
        ring_read(cur, C);                               // c_(r+1)
        if (tid < 4) {
            const Sc cj = dp::pick4(C, j);
            cstm[s][j] = cj.m;
            cste[s][j] = cj.e;
        }
        if (r + 1 < T) {
            Sc col[4];
            column(col);
            b = dp::run_start(C, E, col, j);
        }
    }
    __syncthreads();
    flush_stash((T - 1) / kSeg * kSeg, (T - 1) % kSeg + 1);
    const Sc Z = dp::total(C, E), invz = dp::inverse(Z);
    if (tid == 0) {
        loglik[blockIdx.x] = dp::log_of(Z);
        if (score) score[blockIdx.x] = sc;
        if constexpr (kRuns) {
            runs.invz_m[blockIdx.x] = invz.m;
            runs.invz_e[blockIdx.x] = invz.e;
        }
    }

    // ---- reverse sweep
    double gam = 0.0;                                    // the running gamma_(u-1)(j)
    if (tid < 16) xis[tid / 4][tid % 4] = 0.0;           // (column j is read and written by lane j only from here on)
    auto flush_out = [&](int first, int n) {             // gamma rows first .. first + n - 1, onset rows one further (below T)
        for (int s = tid; s < n; s += dp::kLanes) {
            float4 gv = *reinterpret_cast<const float4*>(gst[s]);
            if (lab) {
                const int y = lab[first + s] & 3;
                gv.x -= y == 0 ? 1.0f : 0.0f;
                gv.y -= y == 1 ? 1.0f : 0.0f;
                gv.z -= y == 2 ? 1.0f : 0.0f;
                gv.w -= y == 3 ? 1.0f : 0.0f;
            }
            reinterpret_cast<float4*>(gamma)[base + first + s] = gv;
            if (onsets && first + s + 1 < T) reinterpret_cast<float4*>(onsets)[base + first + s + 1] = *reinterpret_cast<const float4*>(ost[s]);
        }
    };
    cur = 0;                                             // (T - u) mod R
    for (int u = T; u >= 1; --u) {
        const int r = u - 1, s = r % kSeg;
        if (u == T || s == kSeg - 1) {                   // a segment begins: rows r - s .. r
            const int first = r - s, n = s + 1;
            __syncthreads();                             // the stages are free; the segment above has its gamma and onsets staged
            if (u != T) flush_out(first + kSeg, T - (first + kSeg) < kSeg ? T - (first + kSeg) : kSeg);
            for (int q = tid; q < n; q += dp::kLanes) {
                const double* qm = sm + 4 * static_cast<i64>(first + q);
                *reinterpret_cast<double2*>(cstm[q]) = *reinterpret_cast<const double2*>(qm);
                *reinterpret_cast<double2*>(cstm[q] + 2) = *reinterpret_cast<const double2*>(qm + 2);
                *reinterpret_cast<int4*>(cste[q]) = *reinterpret_cast<const int4*>(se + 4 * static_cast<i64>(first + q));
                *reinterpret_cast<float4*>(est[q]) = e4[first + q];
            }
            if (lab)
                for (int q = tid; q <= n && first + q < T; q += dp::kLanes) lst[q] = lab[first + q];
            __syncthreads();
            if (tid < 4) {                               // E(first + q + 1), summed as the forward sweep summed them
                double acc = ckpt[4 * (first / kSeg) + j];
                for (int q = 0; q < n; ++q) {
                    acc += dp::emission(est[q][j]);
                    Est[q][j] = acc;
                }
            }
            __syncthreads();
        }
        {
            const double2 a = *reinterpret_cast<const double2*>(Est[s]), c = *reinterpret_cast<const double2*>(Est[s] + 2);
            E[0] = a.x; E[1] = a.y; E[2] = c.x; E[3] = c.y;                   // E(u)
            const double2 ma = *reinterpret_cast<const double2*>(cstm[s]), mc = *reinterpret_cast<const double2*>(cstm[s] + 2);
            const int4 x = *reinterpret_cast<const int4*>(cste[s]);
            C[0] = Sc{ma.x, x.x}; C[1] = Sc{ma.y, x.y}; C[2] = Sc{mc.x, x.z}; C[3] = Sc{mc.y, x.w};      // c_u
        }
        Sc g;
        double S = 0.0;
        if (u == T) {
            g = dp::scaled_exp(dp::pick4(E, j));
            gam = dp::value(dp::mul(dp::mul(dp::pick4(C, j), g), invz));
        } else {
            Sc CB[4], tab[4];
            ring_read(cur, CB);                          // cb_u
            row_of(tab);
            g = dp::run_end(CB, E, tab, j);
            double x[4];
            column(tab);
            S = dp::run_changes(C, E, tab, j, dp::pick4(CB, j), invz, x);
            const double N = dp::value(dp::mul(dp::mul(dp::pick4(C, j), g), invz));
            if (tid < 4) {
                int yp = -1;                             // a labelled run change into j here: from yp
                if (lab && (lst[s + 1] & 3) == j && (lst[s] & 3) != j) yp = lst[s] & 3;
#pragma unroll
                for (int i = 0; i < 4; ++i) xis[i][j] = (xis[i][j] + x[i]) - (yp == i ? 1.0 : 0.0);
            }
            gam = (gam - S) + N;
        }
        if (tid < 4) {
            gst[s][j] = static_cast<float>(dp::clamp01(gam));
            ost[s][j] = static_cast<float>(S);           // (row u; there is no row T: the flush leaves it out)
            if constexpr (kRuns) {                       // g_u(j) into row u - 1 of the second stash
                const i64 at = 4 * (base + r) + j;
                runs.g_m[at] = g.m;
                runs.g_e[at] = g.e;
            }
        }
        push(g, cur, u, u == T);
        cur = cur + 1 == R ? 0 : cur + 1;
        __syncthreads();
    }
    flush_out(0, T < kSeg ? T : kSeg);
    {
        Sc CB[4];
        ring_read(cur, CB);                              // cb_0
        const double S0 = dp::value(dp::mul(dp::mul(Sc{tblm[16 + j], tble[16 + j]}, dp::pick4(CB, j)), invz));
        if (tid < 4) {
            if (onsets) onsets[4 * base + j] = static_cast<float>(S0);
            if (s0_out) s0_out[4 * static_cast<i64>(blockIdx.x) + j] = S0 - (lab && (lab[0] & 3) == j ? 1.0 : 0.0);
            if (xi_out) {
#pragma unroll
                for (int i = 0; i < 4; ++i) xi_out[16 * static_cast<i64>(blockIdx.x) + 4 * i + j] = xis[i][j];
            }
        }
    }
}

__global__ __launch_bounds__(dplayout::kLanes) void seg_duration_posteriors_kernel(
    const float* __restrict__ logp, const float* __restrict__ a_pi, const float* __restrict__ dur, const float* __restrict__ edge,
    const uint8_t* __restrict__ labels, float* __restrict__ gamma, float* __restrict__ onsets, double* __restrict__ loglik,
    double* __restrict__ score, double* __restrict__ xi_out, double* __restrict__ s0_out, const double* __restrict__ tabm,
    const int* __restrict__ tabe, double* __restrict__ stash_m, int* __restrict__ stash_e, double* __restrict__ checkpoints,
    const DurPostArgs args)
{
    seg_duration_sweeps<false>(logp, a_pi, dur, edge, labels, gamma, onsets, loglik, score, xi_out, s0_out, tabm, tabe, stash_m, stash_e,
                               checkpoints, args, DurRunsOut{});
}

// the same two sweeps, which also leave g and 1 / Z for seg_duration_run_counts_kernel (hssfsst_posteriors_durations_counts)
__global__ __launch_bounds__(dplayout::kLanes) void seg_duration_runs_sweep_kernel(
    const float* __restrict__ logp, const float* __restrict__ a_pi, const float* __restrict__ dur, const float* __restrict__ edge,
    const uint8_t* __restrict__ labels, float* __restrict__ gamma, float* __restrict__ onsets, double* __restrict__ loglik,
    double* __restrict__ score, double* __restrict__ xi_out, double* __restrict__ s0_out, const double* __restrict__ tabm,
    const int* __restrict__ tabe, double* __restrict__ stash_m, int* __restrict__ stash_e, double* __restrict__ checkpoints,
    const DurRunsOut runs, const DurPostArgs args)
{
    seg_duration_sweeps<true>(logp, a_pi, dur, edge, labels, gamma, onsets, loglik, score, xi_out, s0_out, tabm, tabe, stash_m, stash_e,
                              checkpoints, args, runs);
}

}  // namespace hssfsst
