// segmenter_decode.hpp -- Viterbi decoding of the segmenter's log-probs into state sequences (hssfsst.h: hssfsst_decode_states).
// The arithmetic (int64 fixed point, exact) and the geometry are csrc/decode_layout.hpp's; this file is the workgroup around them.
//
// One workgroup of kLanes lanes per recording, no workgroup waits for another.  Step 0 is d_0 = q(pi) + q(e[0]); steps 1 .. T - 1
// are walked in segments of kSegSteps steps, and the number of segments is the same for every lane of the workgroup.
//   Forward, per segment: the emissions are loaded coalesced (one float4 per step), quantised and staged in LDS; lane l computes the
//   4 x 4 (max, +) transfer matrix of its kLc steps; an inclusive scan of the matrices inside each wave (shuffles) and the four wave
//   totals (LDS) give every lane the true d before its first step; the lane walks its steps again from that d and writes one
//   backpointer byte per step INTO THE PATH OUTPUT.  The d behind the segment is carried in registers.
//   Backward, segments in reverse: lane l reads its kLc bytes back and composes them into the map (state at its last step) ->
//   (state before its first step); a suffix scan of the maps gives the lane its true last state; it walks back, storing the state
//   over each byte it read.  A byte is read and written by the lane that wrote it, so no lane depends on another lane's stores.
// States are indexed by shifts on the packed byte and by unrolled 4-vectors: no run-time-indexed array, no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "decode_layout.hpp"

namespace hssfsst {

constexpr int kDecodeBatch = 256;                        // recordings per launch: their offsets travel as kernel arguments

struct DecodeArgs {
    declayout::Mat A;                                    // quantised log transitions
    declayout::Vec pi;                                   // quantised log initial scores
    long long off[kDecodeBatch + 1];                     // step offsets of the launch's recordings in the arenas
};

__device__ inline declayout::Mat dec_shfl_up(const declayout::Mat& m, int delta)
{
    declayout::Mat r;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) r.m[i][j] = __shfl_up(m.m[i][j], delta, 64);
    return r;
}

__device__ inline declayout::Vec dec_staged(const long long* stage, int idx)
{
    const longlong2 a = *reinterpret_cast<const longlong2*>(stage + idx), b = *reinterpret_cast<const longlong2*>(stage + idx + 2);
    return declayout::Vec{{a.x, a.y, b.x, b.y}};
}

__global__ __launch_bounds__(declayout::kLanes) void seg_decode_kernel(const float* __restrict__ logp, uint8_t* __restrict__ states,
                                                                       long long* __restrict__ scores, const DecodeArgs args)
{
    namespace dl = declayout;
    using dl::i64;
    __shared__ __attribute__((aligned(16))) long long stage[dl::kStageWords];
    __shared__ long long wtot[dl::kLanes / 64][16];
    __shared__ unsigned wmap[dl::kLanes / 64];

    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const i64 base = args.off[blockIdx.x], T = args.off[blockIdx.x + 1] - base;
    const float4* e4 = reinterpret_cast<const float4*>(logp) + base;
    uint8_t* path = states + base;
    const dl::Mat A = args.A;
    const i64 nseg = dl::segments(T);

    dl::Vec d;                                           // d behind the last step walked: the same in every lane
    {
        const float4 e0 = e4[0];
        d.v[0] = dl::add(args.pi.v[0], dl::quantise(e0.x));
        d.v[1] = dl::add(args.pi.v[1], dl::quantise(e0.y));
        d.v[2] = dl::add(args.pi.v[2], dl::quantise(e0.z));
        d.v[3] = dl::add(args.pi.v[3], dl::quantise(e0.w));
    }

    for (i64 seg = 0; seg < nseg; ++seg) {
        const i64 first = dl::segment_first(seg);
        const int nsteps = dl::segment_steps(T, seg), n = dl::lane_steps(nsteps, tid);
#pragma unroll
        for (int k = 0; k < dl::kLc; ++k) {
            const int s = k * dl::kLanes + tid;
            if (s < nsteps) {
                const float4 v = e4[first + s];
                long long* q = stage + dl::stage_index(s);
                *reinterpret_cast<longlong2*>(q) = make_longlong2(dl::quantise(v.x), dl::quantise(v.y));
                *reinterpret_cast<longlong2*>(q + 2) = make_longlong2(dl::quantise(v.z), dl::quantise(v.w));
            }
        }
        __syncthreads();

        dl::Mat P = dl::identity();                      // the lane's transfer matrix, then the wave's inclusive scan
#pragma unroll
        for (int k = 0; k < dl::kLc; ++k)
            if (k < n) dl::step_matrix(P, A, dec_staged(stage, tid * dl::kLaneStride + 4 * k));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const dl::Mat Q = dec_shfl_up(P, off);
            if (lane >= off) P = dl::matmul(Q, P);
        }
        if (lane == 63) {
#pragma unroll
            for (int i = 0; i < 16; ++i) wtot[wave][i] = P.m[i / 4][i % 4];
        }
        dl::Mat X = dec_shfl_up(P, 1);                   // the lanes before this one, in its wave
        if (lane == 0) X = dl::identity();
        __syncthreads();

        dl::Vec din = d, dnext = d;
        for (int w = 0; w < dl::kLanes / 64; ++w) {
            dl::Mat W;
#pragma unroll
            for (int i = 0; i < 16; ++i) W.m[i / 4][i % 4] = wtot[w][i];
            dnext = dl::vecmat(dnext, W);
            if (w + 1 == wave) din = dnext;              // (wave-uniform)
        }
        din = dl::vecmat(din, X);
        const i64 t0 = first + static_cast<i64>(tid) * dl::kLc;
#pragma unroll
        for (int k = 0; k < dl::kLc; ++k)
            if (k < n) path[t0 + k] = static_cast<uint8_t>(dl::step(din, A, dec_staged(stage, tid * dl::kLaneStride + 4 * k)));
        d = dnext;
        __syncthreads();                                 // the stage and the totals are free again
    }

    i64 score;
    unsigned s_end = dl::end_state(d, &score);           // the state at the last step of the segment about to be walked back
    if (tid == 0 && scores) scores[blockIdx.x] = score;

    for (i64 seg = nseg - 1; seg >= 0; --seg) {
        const i64 first = dl::segment_first(seg);
        const int nsteps = dl::segment_steps(T, seg), n = dl::lane_steps(nsteps, tid);
        const i64 t0 = first + static_cast<i64>(tid) * dl::kLc;
        unsigned b[dl::kLc];
        unsigned g = dl::kIdentityMap;                   // state at the lane's last step -> state before its first
#pragma unroll
        for (int k = 0; k < dl::kLc; ++k) {
            b[k] = k < n ? static_cast<unsigned>(path[t0 + k]) : dl::kIdentityMap;
            g = dl::map_compose(g, b[k]);
        }
        unsigned R = g;                                  // suffix scan in the wave: g_l o g_(l+1) o ... o g_63
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned Q = __shfl_down(R, off, 64);
            if (lane + off < 64) R = dl::map_compose(R, Q);
        }
        if (lane == 0) wmap[wave] = R;
        unsigned X = __shfl_down(R, 1, 64);              // the lanes behind this one, in its wave
        if (lane == 63) X = dl::kIdentityMap;
        __syncthreads();

        unsigned s = s_end, s_lane = s_end;              // walking the waves back from the segment's end
#pragma unroll
        for (int w = dl::kLanes / 64 - 1; w >= 0; --w) {
            if (w == wave) s_lane = s;                   // the state at the last step of this lane's wave
            s = dl::map_apply(wmap[w], s);
        }
        s_end = s;                                       // the state before the segment's first step
        s = dl::map_apply(X, s_lane);
#pragma unroll
        for (int k = dl::kLc - 1; k >= 0; --k)
            if (k < n) {
                path[t0 + k] = static_cast<uint8_t>(s);
                s = dl::map_apply(b[k], s);
            }
        __syncthreads();                                 // the wave maps are free again
    }
    if (tid == 0) path[0] = static_cast<uint8_t>(s_end);
}

}  // namespace hssfsst
