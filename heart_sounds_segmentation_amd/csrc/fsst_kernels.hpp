// fsst_kernels.hpp -- hand-written HIP kernels (gfx950 / CDNA4, wave64) of the FSST feature path.
//
// What the path computes (reference boundary: /root/reference/hss/transforms/synchrosqueeze.py:48
// `ssq.fsst(x, fs, window)` + the epilogue :50-111; algorithm steps as restated in
// oracle/fsst_oracle.c): for every sample t of a signal, the nwin-point DFT of the zero-padded
// hop-1 frame under the window w (V) and under the derivative window dw (Vd); the instantaneous
// frequency coordinate a = k - Im(Vd/V) * nwin/fs; the cyclic scatter S[round(a) mod nwin, t] +=
// (-1)^k V[k, t]; then band truncation and abs / z-score-stack / raw output.
//
// MI355X mapping (not a translation of an FFT-library call pattern):
//   * one frame per lane, one 64-frame tile per wavefront; the signal tile (+ nwin-1 halo) and the
//     per-lane scatter accumulators live in LDS, so HBM sees 4 B in and 4*out_floats B out per
//     sample and nothing else;
//   * nwin = 32*R.  The first radix-R decimation-in-frequency stage is FOLDED into the window
//     multiply: class r (bins k = R*j + r) is the 32-point FFT of
//         y_r[n] = sum_q x[t + n + 32 q] * C_r[n, q],   C_r[n,q] = win[n+32q] * W_R^{rq} * W_nwin^{rn}
//     with C_r precomputed on the host in fp64 and read through the scalar cache (wave-uniform),
//     so windowing, the first butterfly stage and its twiddles cost one FMA per (output, q);
//   * real input => only classes r <= R/2 are transformed.  The self-conjugate classes r = 0 and
//     r = R/2 carry V and Vd packed in ONE complex FFT (two-for-one, partner bin in the same
//     class); classes 0 < r < R/2 run one FFT for w and one for dw: bins j < 16 are class r's
//     one-sided bins, bins j >= 16 are (conjugated) the one-sided bins of class R - r;
//   * every one-sided source bin k' also feeds its negative-frequency mirror nwin - k' (value
//     conj, row (nwin - row) mod nwin), which reproduces the reference's two-sided cyclic scatter
//     exactly, including wrap-around into the kept band;
//   * the 32-point FFT is a fully unrolled radix-2 DIT in registers, twiddles as constants,
//     6 FMA-class ops per general butterfly (second output as 2e - first);
//   * MFMA is deliberately unused: at fp32 the matrix pipe has no rate advantage and the only
//     dense contraction (the folded first stage) is K <= 16 deep.
#pragma once
#include "fsst_device.hpp"

namespace hssfsst {

// Per-signal statistics from the partials: one wave per signal.
// stats[b] = {mean_re, 1/std_re, mean_im, 1/std_im}.
// (gate != nullptr: the launch is the fallback of a team-kernel exec and runs only if that launch gave up -- *gate == gate_val)
__global__ __launch_bounds__(64) void fsst_stats_kernel(const float* partials, float4* stats, int nparts, int fpp,
                                                        int n, int K, const unsigned* gate = nullptr, unsigned gate_val = 0u)
{
    if (gate != nullptr && *gate != gate_val) return;
    const long long b = blockIdx.x;
    const float4 st = signal_stats(partials + b * nparts * kPartFloats, nparts, fpp, n, K, threadIdx.x & 63);
    if (threadIdx.x == 0) stats[b] = st;
}

// ------------------------------------------------------------------------------------------------
// Core kernel: one block = one TILE-sample stretch of one signal; one lane = one hop-1 frame.
// LDS: xs[TILE + nwin - 1 (+pad)] | own[2K][TILE + 1] | disp[2K][TILE + 1]; red[] aliases xs.
// p.oneplane != 0: own and disp are the same plane (half the LDS; every own-row value then costs a read-modify-write
// instead of a store) -- used by the host when two planes of the kept band do not fit 160 KB (nwin = 512, wide bands).
// ------------------------------------------------------------------------------------------------
template <int R, int TILE>
__global__ __launch_bounds__(TILE, 2) void fsst_core_kernel(CoreParams p)
{
    constexpr int NWIN = 32 * R;
    constexpr int XS = ((TILE + NWIN - 1 + 3) / 4) * 4;
    constexpr int LD = TILE + 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;
    float* own = smem + XS;

    const int tid = threadIdx.x;
    const int blk = blockIdx.x % p.nblk;
    const long long b = blockIdx.x / p.nblk;
    const int t0 = p.col0 + blk * TILE;
    const int n = p.n;
    const int ncols = p.ncols, tr0 = t0 - p.col0;      // output rows are relative to col0
    const int K = p.K;
    const float* xsig = p.x + b * p.xstride;

    // stage the zero-padded signal tile: xs[i] = xpad[t0 + i] = x[t0 + i - nwin/2]
    float e2 = 0.0f, s1 = 0.0f, cnt = 0.0f;              // sum x^2 of the tile: error-bound scale of displaced cells; sum x, samples
    for (int i = tid; i < TILE + NWIN - 1; i += TILE) {
        const int g = t0 + i - NWIN / 2;
        const bool in = (g >= 0 && g < n);
        const float v = in ? xsig[g] : 0.0f;
        xs[i] = v;
        e2 = fmaf(v, v, e2); s1 += v; cnt += in ? 1.0f : 0.0f;
    }
    static_assert(TILE == 64, "tile_energy reduces one wave");
    const TileEnergy te = tile_energy(e2, s1, cnt);
    const float R2 = p.r2scale * te.E;
    const bool oneplane = p.oneplane != 0;
    float* disp = oneplane ? own : own + 2 * K * LD;
    for (int c = 0; c < 2 * K; ++c) disp[c * LD + tid] = 0.0f;
    __syncthreads();

    const Scatter<LD> sc{own + tid, disp + tid, p.klo, K, oneplane, xs + tid, p.wtab, p.twtab, R2};
    const float* myx = xs + tid;
    ctab_ptr tab = (ctab_ptr)p.ctab;
    packed_class<R, false, LD>(tab, myx, sc);
    if constexpr (R >= 2) packed_class<R, true, LD>(tab + (R / 2) * 32 * 4 * R, myx, sc);
    if constexpr (R >= 4 && R <= 8) {
        static_for<R / 2 - 1>([&](auto RR) {
            constexpr int r = decltype(RR)::value + 1;
            pair_class<R, LD>(tab + r * 32 * 4 * R, r, myx, sc);
        });
    } else if constexpr (R > 8) {
        for (int r = 1; r < R / 2; ++r) pair_class<R, LD>(tab + r * 32 * 4 * R, r, myx, sc);
    }
    __syncthreads();
    // fold the displaced plane into the own plane (each lane its own column: no hazard)
    if (!oneplane) {
        for (int c = 0; c < 2 * K; ++c) own[c * LD + tid] += disp[c * LD + tid];
    }
    __syncthreads();
    float* acc = own;
    // ---- "Exact groups" (fsst_mfma128.hpp): no kept cell of the tile reaches 1e-2 R (R^2 = the bound of the tile's spectrum
    //      norms: the band holds only the far leakage of something outside it, and float32 resolves ~4e-7 of the frame's
    //      spectrum norm, not of the band) -> every lane redoes its frame in float64: all one-sided sources, float64 DFT
    //      of V and Vd', the float64 coordinate rounded half away from zero, the two-sided cyclic scatter into the kept rows.
    {
        float mxc = 0.0f;
        for (int k = 0; k < K; ++k) { const float re = acc[k * LD + tid], im = acc[(K + k) * LD + tid]; mxc = fmaxf(mxc, fmaf(re, re, im * im)); }
        if ((__builtin_amdgcn_ballot_w64(mxc > 1.0e-4f * R2) == 0ull || te.dcdom) && R2 > 0.0f) {
            for (int c = 0; c < 2 * K; ++c) acc[c * LD + tid] = 0.0f;
            const int klo = p.klo;
            for (int kp = 0; kp <= NWIN / 2; ++kp) {
                double vr = 0.0, vi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll 4
                for (int nn = 0; nn < NWIN; ++nn) {
                    const double x = static_cast<double>(xs[tid + nn]);
                    const double2 wd = reinterpret_cast<const double2*>(p.wtab)[nn];
                    const double2 cs = reinterpret_cast<const double2*>(p.twtab)[(kp * nn) & (NWIN - 1)];
                    const double xw = x * wd.x, xd = x * wd.y;
                    vr = fma(xw, cs.x, vr); vi = fma(-xw, cs.y, vi);
                    dr = fma(xd, cs.x, dr); di = fma(-xd, cs.y, di);
                }
                double shift = (dr * vi - di * vr) / (vr * vr + vi * vi);
                if (!(fabs(shift) <= 1.0e6)) shift = 0.0;           // V == 0 or absurd -> 0 (fsst.m: ~isfinite)
                const double a = static_cast<double>(kp) + shift;
                const double r = (a >= 0.0) ? floor(a + 0.5) : -floor(0.5 - a);
                const int row = static_cast<int>(static_cast<long long>(r)) & (NWIN - 1);
                const double sg = (kp & 1) ? -1.0 : 1.0;              // the modified-STFT phase for even nwin
                const float re = static_cast<float>(vr * sg), im = static_cast<float>(vi * sg);
                const int idx = row - klo;
                if (static_cast<unsigned>(idx) < static_cast<unsigned>(K)) { acc[idx * LD + tid] += re; acc[(K + idx) * LD + tid] += im; }
                if (kp != 0 && kp != NWIN / 2) {                      // the negative-frequency twin N - k' lands in N - row, conjugated
                    const int idm = ((NWIN - row) & (NWIN - 1)) - klo;
                    if (static_cast<unsigned>(idm) < static_cast<unsigned>(K)) { acc[idm * LD + tid] += re; acc[(K + idm) * LD + tid] -= im; }
                }
            }
        }
    }

    const int valid = min(TILE, p.col0 + ncols - t0);
    if (p.mode == kModeRaw) {
        // complex64 [K][n], frequency-major: lane tid owns sample t0 + tid
        if (tid < valid) {
            float2* dst = reinterpret_cast<float2*>(p.out) + (b * K) * static_cast<long long>(ncols) + tr0 + tid;
            for (int k = 0; k < K; ++k)
                dst[static_cast<long long>(k) * ncols] = make_float2(acc[k * LD + tid], acc[(K + k) * LD + tid]);
        }
        return;
    }
    // time-major outputs: the tile's block of `valid * C` floats is contiguous in HBM
    const int C = (p.mode == kModeAbs) ? K : 2 * K;
    float* dst = p.out + (b * static_cast<long long>(ncols) + tr0) * C;
    const int total = valid * C;
    int tt = tid / C, c = tid - tt * C;
    const int dtt = TILE / C, dc = TILE - dtt * C;
    static_assert(TILE == 64, "one wave per tile: the statistics partial is a single-wave reduction");
    // pivots of this tile's statistics partial: its first frame's first kept row (a value of the data itself)
    const float p_re = pivot_med3(acc[0], acc[(K >> 1) * LD], acc[(K - 1) * LD]);
    const float p_im = pivot_med3(acc[K * LD], acc[(K + (K >> 1)) * LD], acc[(2 * K - 1) * LD]);
    float s_re = 0.0f, q_re = 0.0f, s_im = 0.0f, q_im = 0.0f;
    for (int e = tid; e < total; e += TILE) {
        float val;
        if (p.mode == kModeAbs) {
            const float re = acc[c * LD + tt], im = acc[(K + c) * LD + tt];
            val = sqrtf(fmaf(re, re, im * im));
        } else {
            val = acc[c * LD + tt];
            if (c < K) { const float d = val - p_re; s_re += d; q_re = fmaf(d, d, q_re); }
            else       { const float d = val - p_im; s_im += d; q_im = fmaf(d, d, q_im); }
        }
        dst[e] = val;
        c += dc; tt += dtt;
        if (c >= C) { c -= C; ++tt; }
    }
    if (p.mode != kModeStack) return;
    // per-tile statistics partial (fixed reduction order => run-to-run deterministic)
    const float w = piece_sums(s_re, q_re, s_im, q_im);
    store_partial(p.partials + (b * p.nblk + blk) * kPartFloats, w, p_re, p_im);
}

// grid = any number of blocks of 256 (the host sizes it to a fraction of the chip so the sweep can
// share the GPU with a concurrently running core kernel); block b handles signals b, b + grid, ...
// in = float32 [nsignals][n][2K] (16-byte aligned), out = OT [nsignals][n][2K]: float is the in-place sweep (the host passes
// in == out: no __restrict__ here), a 2-byte OT the out-of-place one of a half plan (fsst_half.hpp).
// With `partials` != nullptr the block first reduces the signal's nblk fp64 partials itself (the arithmetic of
// fsst_stats_kernel, same order, same result) instead of reading `stats`: one launch less per transform.
// `slices` > 1 cuts every signal into that many contiguous pieces, one block each (small batches: a block per
// signal would leave most of the chip idle); the fused reduction is only used with slices == 1.
template <class OT>
__global__ __launch_bounds__(256) void fsst_normalize_kernel(const float* in, OT* out, const float4* stats, const float* partials,
                                                             int nblk, int fpp, int n, int K, int nsignals, int slices,
                                                             const unsigned* gate = nullptr, unsigned gate_val = 0u)
{
    if (gate != nullptr && *gate != gate_val) return;    // (see fsst_stats_kernel)
    __shared__ float4 st_sh;
    const int tid = threadIdx.x;
    const int C = 2 * K;
    const int total = n * C;                             // per-signal element count (< 2^31, checked on the host)
    const bool vec = (total & 3) == 0 && zscore_store4_aligned(out);
    for (int unit = blockIdx.x; unit < nsignals * slices; unit += gridDim.x) {
        const int sig = unit / slices, sl = unit - sig * slices;
        float4 st;
        if (partials != nullptr) {
            if (tid < 64) {
                const float4 r = signal_stats(partials + static_cast<long long>(sig) * nblk * kPartFloats, nblk, fpp, n, K, tid);
                if (tid == 0) st_sh = r;
            }
            __syncthreads();
            st = st_sh;
            __syncthreads();                             // st_sh is rewritten for the block's next signal
        } else {
            st = stats[sig];
        }
        const float m_re = st.x, i_re = st.y, m_im = st.z, i_im = st.w;
        const float* src = in + static_cast<long long>(sig) * total;
        OT* dst = out + static_cast<long long>(sig) * total;
        if (vec) {
            // linear float4 sweep of the signal's block (its start is 16-byte aligned because total % 4 == 0); the
            // column of a chunk is tracked incrementally (no integer division in the loop).  When 2K is not a
            // multiple of 4 a float4 can wrap from the end of one row into the next: per-element wrap test.
            const float4* s4 = reinterpret_cast<const float4*>(src);
            const int tot4 = total >> 2;
            const int i0 = static_cast<int>(static_cast<long long>(tot4) * sl / slices);
            const int i1 = static_cast<int>(static_cast<long long>(tot4) * (sl + 1) / slices);
            int c = static_cast<int>((static_cast<unsigned>(i0 + tid) * 4u) % static_cast<unsigned>(C));
            const int dc = static_cast<int>(1024u % static_cast<unsigned>(C));
            const bool rowwrap = (C & 3) != 0;
#pragma unroll 4
            for (int i = i0 + tid; i < i1; i += 256) {
                const float4 v = s4[i];                  // (streaming load / store hints measured here: 0.147 vs 0.119 ms, worse)
                int c1 = c + 1, c2 = c + 2, c3 = c + 3;
                if (rowwrap) {
                    if (c1 >= C) c1 -= C;
                    if (c2 >= C) c2 -= C;
                    if (c3 >= C) c3 -= C;
                }
                zscore_store4<OT>(dst + 4ll * i,
                                  (c < K) ? (v.x - m_re) * i_re : (v.x - m_im) * i_im,
                                  (c1 < K) ? (v.y - m_re) * i_re : (v.y - m_im) * i_im,
                                  (c2 < K) ? (v.z - m_re) * i_re : (v.z - m_im) * i_im,
                                  (c3 < K) ? (v.w - m_re) * i_re : (v.w - m_im) * i_im);
                c += dc;
                if (c >= C) c -= C;
            }
        } else {
            const int i0 = static_cast<int>(static_cast<long long>(total) * sl / slices);
            const int i1 = static_cast<int>(static_cast<long long>(total) * (sl + 1) / slices);
            for (int i = i0 + tid; i < i1; i += 256) {
                const int c = i % C;
                const float v = src[i];
                dst[i] = static_cast<OT>((c < K) ? (v - m_re) * i_re : (v - m_im) * i_im);
            }
        }
    }
}

__global__ __launch_bounds__(kMomThreads) void fsst_moments_merge_kernel(const float* feats, double* state, int n, int K)
{
    __shared__ double sh[64][4];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const int total = n * 2 * K;                         // < 2^31, checked on the host
    double m[4];
    chunk_moments(feats + b * static_cast<long long>(total), n, 2 * K, K, tid, sh, m);
    if (tid < 2) merge_state(state + b * 6 + tid * 3, m[2 * tid], m[2 * tid + 1], static_cast<double>(K) * static_cast<double>(n));
}

// Running-moments normalisation (streaming): stats[b] from the {count, mean, M2} state of
// fsst_moments_merge_kernel, i.e. mean and unbiased std of everything seen so far.
__global__ __launch_bounds__(64) void fsst_stats_from_state_kernel(const double* state, float4* stats, int nsig)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nsig) return;
    const double* st = state + static_cast<long long>(b) * 6;
    const double vr = st[2] / (st[0] - 1.0), vi = st[5] / (st[3] - 1.0);
    stats[b] = make_float4(static_cast<float>(st[1]), 1.0f / static_cast<float>(sqrt(vr)),
                           static_cast<float>(st[4]), 1.0f / static_cast<float>(sqrt(vi)));
}

// One streaming step's tail in ONE launch (hssfsst_stream_step): block b merges the new un-normalised chunk of channel b
// into its running {count, mean, M2} and then normalises that chunk with the updated moments.  Same arithmetic, same
// order as fsst_moments_merge_kernel -> fsst_stats_from_state_kernel -> fsst_normalize_kernel: bit-identical results,
// two launches (and the statistics round trip through HBM) fewer per step.  grid = channels, block = 1024.
__global__ __launch_bounds__(kMomThreads) void fsst_stream_finish_kernel(float* feats, double* state, int n, int K)
{
    __shared__ double sh[64][4];
    __shared__ float4 st_sh;
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    float* base = feats + b * static_cast<long long>(n) * (2 * K);
    double m[4];
    chunk_moments(base, n, 2 * K, K, tid, sh, m);
    if (tid < 2) {
        const float2 r = merge_state(state + b * 6 + tid * 3, m[2 * tid], m[2 * tid + 1], static_cast<double>(K) * static_cast<double>(n));
        if (tid == 0) { st_sh.x = r.x; st_sh.y = r.y; } else { st_sh.z = r.x; st_sh.w = r.y; }
    }
    __syncthreads();
    stream_normalize_block<kMomThreads>(base, n, K, tid, st_sh);
}

}  // namespace hssfsst
