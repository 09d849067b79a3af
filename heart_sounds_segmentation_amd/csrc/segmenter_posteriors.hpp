// segmenter_posteriors.hpp -- forward-backward over the segmenter's log-probs under a transition model (hssfsst.h:
// hssfsst_posteriors): per-step state posteriors gamma, the sequence log-likelihood logZ, the expected transition counts Xi and,
// with labels, the labelled path's score and gamma - onehot(labels), the gradient of logZ - score in the emissions.
// The arithmetic (float64, linear domain, scaled by exact powers of two) and the geometry are csrc/posterior_layout.hpp's; this
// file is the workgroup around them.
//
// THE LIMIT (posterior_layout.hpp): a path whose weight falls more than ~700 nats (float64 underflow) below the best path reaching
// the same step is dropped; everything is renormalised after every step of a lane's walk and every product of a scan, so nothing
// else underflows.  Emissions within 200 of their step's maximum cannot trigger it.  NaN emissions count as -inf; Z = 0 gives
// logZ = -inf, gamma = 0, Xi = 0.
//
// One workgroup of kLanes lanes per recording, no workgroup waits for another.  Step 0 is alpha_0 = p0 . b_0; steps 1 .. T - 1 are
// walked in segments of kSegSteps steps.
//   Forward sweep, per segment: the emissions are loaded coalesced (one float4 per step), turned into b = exp(e - max e) and
//   staged in LDS; lane l composes the 4 x 4 transfer matrix of its kLc steps; an inclusive scan inside each wave (shuffles) and
//   the four wave totals (LDS) carry alpha over the segment.  The alpha BEFORE the segment goes to the caller's workspace.  The
//   step maxima and, with labels, the path's score are summed on the way (per lane, then a fixed-order tree).
//   Reverse sweep, segments in reverse: staged again; a prefix scan gives each lane the alpha before its first step (from the
//   checkpoint), a suffix scan the beta behind its last one; the lane walks its steps forwards for the alphas and back for beta,
//   writes gamma as one float4 per step and accumulates its 16 Xi terms, which a fixed-order workgroup reduction adds up per
//   segment (so they are not carried in registers across the scans).
// 4-vectors and 4 x 4 matrices are unrolled: no run-time-indexed private array, no scratch.  A scan holds four matrices (128
// registers); exp(A), exp(pi) live in LDS and the walk holds kLc / 2 alphas at a time: 256 registers, no AGPR.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "posterior_layout.hpp"

namespace hssfsst {

constexpr int kPostBatch = 256;                          // recordings per launch: their offsets travel as kernel arguments

struct PostArgs {
    long long off[kPostBatch + 1];                       // step offsets of the launch's recordings in the arenas
    long long rec0;                                      // the first one's number in the list (its checkpoint slots)
};

__device__ inline postlayout::SMat post_shfl_up(const postlayout::SMat& m, int delta)
{
    postlayout::SMat r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) r.m[i][j] = __shfl_up(m.m[i][j], delta, 64);
    r.e = __shfl_up(m.e, delta, 64);
    return r;
}
__device__ inline postlayout::SMat post_shfl_down(const postlayout::SMat& m, int delta)
{
    postlayout::SMat r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) r.m[i][j] = __shfl_down(m.m[i][j], delta, 64);
    r.e = __shfl_down(m.e, delta, 64);
    return r;
}

// P = exp(A) and p0 = exp(pi) are kept in LDS (20 float64) and read where they are used, not held in 40 registers over the scans
__device__ inline postlayout::Tables post_tables(const double* tbl)
{
    postlayout::Tables t;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double2 a = *reinterpret_cast<const double2*>(tbl + 4 * i), b = *reinterpret_cast<const double2*>(tbl + 4 * i + 2);
        t.P[i][0] = a.x, t.P[i][1] = a.y, t.P[i][2] = b.x, t.P[i][3] = b.y;
    }
    const double2 a = *reinterpret_cast<const double2*>(tbl + 16), b = *reinterpret_cast<const double2*>(tbl + 18);
    t.p0[0] = a.x, t.p0[1] = a.y, t.p0[2] = b.x, t.p0[3] = b.y;
    return t;
}

struct PostB { double b[4]; };
__device__ inline PostB post_staged(const double* stage, int idx)
{
    const double2 a = *reinterpret_cast<const double2*>(stage + idx), b = *reinterpret_cast<const double2*>(stage + idx + 2);
    return PostB{{a.x, a.y, b.x, b.y}};
}

// the sum over the workgroup of n <= 18 per-lane values, in a fixed order: a shuffle tree in each wave, then the waves in order.
// Every lane gets the sums.  (Two barriers.)
template <int N>
__device__ inline void post_reduce(double* v, double (*red)[18], int lane, int wave)
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double x = v[i];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0) red[wave][i] = x;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
    __syncthreads();
}

// Stages a segment's b; FORWARD also sums the step maxima and the labelled path's terms of these steps into acc[0], acc[1].
template <bool FORWARD>
__device__ inline void post_stage(double* stage, const float4* e4, const uint8_t* lab, const float* a_pi, long long first, int nsteps, int tid,
                                  double* acc)
{
    namespace pl = postlayout;
#pragma unroll
    for (int k = 0; k < pl::kLc; ++k) {
        const int s = k * pl::kLanes + tid;
        if (s < nsteps) {
            const float4 v = e4[first + s];
            double b[4];
            const double top = pl::step_weights(v.x, v.y, v.z, v.w, b);
            double* q = stage + pl::stage_index(s);
            *reinterpret_cast<double2*>(q) = make_double2(b[0], b[1]);
            *reinterpret_cast<double2*>(q + 2) = make_double2(b[2], b[3]);
            if (FORWARD) {
                acc[0] += top;
                if (lab) {
                    const int y = lab[first + s] & 3, yp = lab[first + s - 1] & 3;
                    const float ev = y == 0 ? v.x : (y == 1 ? v.y : (y == 2 ? v.z : v.w));
                    acc[1] += static_cast<double>(ev != ev ? -__builtin_inff() : ev) + static_cast<double>(a_pi[4 * yp + y]);
                }
            }
        }
    }
}

__global__ __launch_bounds__(postlayout::kLanes, 2) void seg_posteriors_kernel(const float* __restrict__ logp, const float* __restrict__ a_pi,
                                                                            const uint8_t* __restrict__ labels, float* __restrict__ gamma,
                                                                            double* __restrict__ loglik, double* __restrict__ score,
                                                                            double* __restrict__ xi_out, double* __restrict__ gamma0,
                                                                            double* __restrict__ work, const PostArgs args)
{
    namespace pl = postlayout;
    using pl::i64;
    __shared__ __attribute__((aligned(16))) double stage[pl::kStageWords];
    __shared__ double wtot[pl::kLanes / 64][16];
    __shared__ int wexp[pl::kLanes / 64];
    __shared__ double red[pl::kLanes / 64][18];
    __shared__ __attribute__((aligned(16))) double tbl[20];
    __shared__ double xi_acc[16];                        // Xi so far: lane 0 adds every segment's sums (registers for the scans)

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const i64 base = args.off[blockIdx.x], T = args.off[blockIdx.x + 1] - base;
    const float4* e4 = reinterpret_cast<const float4*>(logp) + base;
    float4* g4 = reinterpret_cast<float4*>(gamma) + base;
    const uint8_t* lab = labels ? labels + base : nullptr;
    double* ckpt = work + 4 * pl::checkpoint_slot(base, args.rec0 + blockIdx.x);
    const i64 nseg = pl::segments(T);
    if (tid < 20) tbl[tid] = exp(static_cast<double>(a_pi[tid]));      // (make_tables(), one entry per lane)
    if (tid < 16) xi_acc[tid] = 0.0;                     // (read and written by lane 0 only from here on)
    __syncthreads();

    double acc[2] = {0.0, 0.0};                          // this lane's share of sum_t max e and of the labelled path's score
    pl::SVec alpha0;                                     // alpha_0 = p0 . b_0, kept for gamma_0
    {
        const float4 v = e4[0];
        double b[4];
        const double top = pl::step_weights(v.x, v.y, v.z, v.w, b);
        const pl::Tables tb = post_tables(tbl);
        alpha0 = pl::SVec{{tb.p0[0] * b[0], tb.p0[1] * b[1], tb.p0[2] * b[2], tb.p0[3] * b[3]}, 0};
        pl::renorm(alpha0);
        if (tid == 0) {
            acc[0] = top;
            if (lab) {
                const int y = lab[0] & 3;
                const float ev = y == 0 ? v.x : (y == 1 ? v.y : (y == 2 ? v.z : v.w));
                acc[1] = static_cast<double>(ev != ev ? -__builtin_inff() : ev) + static_cast<double>(a_pi[16 + y]);
            }
        }
    }

    // ---- forward sweep: the alpha behind the last step, a checkpoint before every segment
    pl::SVec alpha = alpha0;                             // the same in every lane
    for (i64 seg = 0; seg < nseg; ++seg) {
        const i64 first = pl::segment_first(seg);
        const int nsteps = pl::segment_steps(T, seg), n = pl::lane_steps(nsteps, tid);
        post_stage<true>(stage, e4, lab, a_pi, first, nsteps, tid, acc);
        __syncthreads();
        pl::SMat P = pl::identity();
        {
            const pl::Tables tb = post_tables(tbl);
#pragma unroll
            for (int k = 0; k < pl::kLc; ++k)
                if (k < n) pl::step_matrix(P, tb, post_staged(stage, tid * pl::kLaneStride + 4 * k).b);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const pl::SMat Q = post_shfl_up(P, off);
            if (lane >= off) P = pl::matmul(Q, P);
        }
        if (lane == 63) {
#pragma unroll
            for (int i = 0; i < 16; ++i) wtot[wave][i] = P.m[i / 4][i % 4];
            wexp[wave] = P.e;
        }
        if (tid == 0) {
            *reinterpret_cast<double2*>(ckpt + 4 * seg) = make_double2(alpha.v[0], alpha.v[1]);
            *reinterpret_cast<double2*>(ckpt + 4 * seg + 2) = make_double2(alpha.v[2], alpha.v[3]);
        }
        __syncthreads();
        for (int w = 0; w < pl::kLanes / 64; ++w) {
            pl::SMat W;
#pragma unroll
            for (int i = 0; i < 16; ++i) W.m[i / 4][i % 4] = wtot[w][i];
            W.e = wexp[w];
            alpha = pl::vecmat(alpha, W);
        }
        __syncthreads();                                 // the stage and the totals are free again
    }
    post_reduce<2>(acc, red, lane, wave);
    if (tid == 0) {
        loglik[blockIdx.x] = pl::log_z(alpha, acc[0]);
        if (score) score[blockIdx.x] = acc[1];
    }

    // ---- reverse sweep
    pl::SVec beta_end{{1.0, 1.0, 1.0, 1.0}, 0};          // beta at the last step of the segment about to be walked: in every lane
    for (i64 seg = nseg - 1; seg >= 0; --seg) {
        const i64 first = pl::segment_first(seg);
        const int nsteps = pl::segment_steps(T, seg), n = pl::lane_steps(nsteps, tid);
        post_stage<false>(stage, e4, lab, a_pi, first, nsteps, tid, acc);
        __syncthreads();
        pl::SMat M = pl::identity();
        {
            const pl::Tables tb = post_tables(tbl);
#pragma unroll
            for (int k = 0; k < pl::kLc; ++k)
                if (k < n) pl::step_matrix(M, tb, post_staged(stage, tid * pl::kLaneStride + 4 * k).b);
        }
        pl::SMat P = M;                                  // inclusive prefix scan in the wave: M_0 M_1 .. M_l
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const pl::SMat Q = post_shfl_up(P, off);
            if (lane >= off) P = pl::matmul(Q, P);
        }
        if (lane == 63) {
#pragma unroll
            for (int i = 0; i < 16; ++i) wtot[wave][i] = P.m[i / 4][i % 4];
        }
        pl::SMat X = post_shfl_up(P, 1);                 // the lanes before this one, in its wave
        if (lane == 0) X = pl::identity();
        __syncthreads();

        pl::SVec a_lane{{ckpt[4 * seg], ckpt[4 * seg + 1], ckpt[4 * seg + 2], ckpt[4 * seg + 3]}, 0};
        {
            pl::SVec run = a_lane;
            for (int w = 0; w + 1 < pl::kLanes / 64; ++w) {
                pl::SMat W;
#pragma unroll
                for (int i = 0; i < 16; ++i) W.m[i / 4][i % 4] = wtot[w][i];
                W.e = 0;
                run = pl::vecmat(run, W);
                if (w + 1 == wave) a_lane = run;         // (wave-uniform)
            }
            a_lane = pl::vecmat(a_lane, X);              // alpha before this lane's first step
        }
        P = M;                                           // inclusive suffix scan in the wave: M_l M_(l+1) .. M_63
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const pl::SMat Q = post_shfl_down(P, off);
            if (lane + off < 64) P = pl::matmul(P, Q);
        }
        pl::SMat Y = post_shfl_down(P, 1);               // the lanes behind this one, in its wave
        if (lane == 63) Y = pl::identity();
        pl::SVec b_lane = beta_end;
        {
            pl::SVec run = beta_end;
            for (int w = pl::kLanes / 64 - 1; w >= 0; --w) {
                if (w == wave) b_lane = run;             // beta at the last step of this lane's wave
                pl::SMat W;
#pragma unroll
                for (int i = 0; i < 16; ++i) W.m[i / 4][i % 4] = wtot[w][i];
                W.e = 0;
                run = pl::matvec(W, run);
            }
            beta_end = run;                              // beta at the step before the segment's first
            b_lane = pl::matvec(Y, b_lane);              // beta at this lane's last step
        }

        // The walk, in two halves so that kLc / 2 alphas are held at a time: the alpha before the upper half first.
        constexpr int kHalf = pl::kLc / 2;
        const i64 t0 = first + static_cast<i64>(tid) * pl::kLc;
        double xi[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) xi[i] = 0.0;
        const pl::Tables tb = post_tables(tbl);
        pl::SVec a_mid = a_lane;
#pragma unroll
        for (int k = 0; k < kHalf; ++k)
            if (k < n) pl::step_alpha(a_mid, tb, post_staged(stage, tid * pl::kLaneStride + 4 * k).b);
#pragma unroll
        for (int half = 1; half >= 0; --half) {
            const int k0 = half * kHalf;
            pl::SVec a[kHalf];                           // a[j]: alpha before the lane's step k0 + j
            a[0] = half ? a_mid : a_lane;
#pragma unroll
            for (int j = 0; j + 1 < kHalf; ++j) {
                a[j + 1] = a[j];
                if (k0 + j + 1 < n) pl::step_alpha(a[j + 1], tb, post_staged(stage, tid * pl::kLaneStride + 4 * (k0 + j)).b);
            }
#pragma unroll
            for (int j = kHalf - 1; j >= 0; --j) {
                const int k = k0 + j;
                if (k < n) {
                    double g[4];
                    pl::step_back(a[j], tb, post_staged(stage, tid * pl::kLaneStride + 4 * k).b, b_lane, xi, g);
                    if (lab) {
                        const int y = lab[t0 + k] & 3, yp = lab[t0 + k - 1] & 3;
#pragma unroll
                        for (int c = 0; c < 4; ++c) g[c] -= y == c ? 1.0 : 0.0;
#pragma unroll
                        for (int i = 0; i < 16; ++i) xi[i] -= (4 * yp + y) == i ? 1.0 : 0.0;
                    }
                    g4[t0 + k] = make_float4(static_cast<float>(g[0]), static_cast<float>(g[1]), static_cast<float>(g[2]), static_cast<float>(g[3]));
                }
            }
        }
        if (xi_out) {                                    // (uniform) the segment's sums, in a fixed order; its two barriers free
            post_reduce<16>(xi, red, lane, wave);        // the stage and the totals as well
            if (tid == 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) xi_acc[i] += xi[i];
            }
        } else {
            __syncthreads();                             // the stage and the totals are free again
        }
    }
    if (tid == 0) {
        double g[4];
        pl::step_zero(alpha0, beta_end, g);
        if (lab) {
            const int y = lab[0] & 3;
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] -= y == j ? 1.0 : 0.0;
        }
        g4[0] = make_float4(static_cast<float>(g[0]), static_cast<float>(g[1]), static_cast<float>(g[2]), static_cast<float>(g[3]));
        if (gamma0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) gamma0[4 * static_cast<i64>(blockIdx.x) + j] = g[j];
        }
    }
    if (xi_out && tid == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) xi_out[16 * static_cast<i64>(blockIdx.x) + i] = xi_acc[i];
    }
}

}  // namespace hssfsst
