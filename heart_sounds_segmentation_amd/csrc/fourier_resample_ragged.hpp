// fourier_resample_ragged.hpp -- fourier_resample_gpu.hpp for a LIST of signals of different lengths n_i, all resampled to the
// same num (hssfsst.h: hssfsst_resample_exec_ragged).  Same algorithm (fp64 Bluestein on power-of-two FFTs) on the same kernels: the
// large tier of fourier_resample_gpu.hpp, whose steps ask RaggedResampleArgs below about each signal.  Three differences:
//
//   * the forward tables of every length are made ON THE DEVICE, per call, in fp64: the chirp
//       c1[m] = conj(w1[m]),  w1[m] = exp(+i pi (m^2 mod 2n) / n)      (m^2 mod 2n exactly in int64, as the host does)
//     is generated inline where it is used, and the bit-reversed spectrum B1 / M1 of the wrapped chirp is a device DIF FFT
//     (natural order in, bit-reversed order out: the DIF passes, the LDS DIF stages and a last len-2 stage with the 1 / M1
//     scale -- resample_ragged_table_kernel, resample_dif_pass_kernel, resample_ragged_table_block_kernel).  One table per
//     distinct length of a chunk: repeated lengths share it.
//   * signals are grouped by their convolution length M1_i (the host sorts the list by n, so a class is a contiguous run):
//     one pass launch covers every signal of a class in the chunk, and every signal has a descriptor (RaggedResampleSig:
//     start, n, M1, table offset, output row);
//   * the inverse side (num, c2, B2) is shared: the middle step, the second convolution and the store run ONCE over the
//     whole chunk, with the plan's host-made c2 / B2 and twiddle table (grown to the largest M of a call).
//
// Work layout of a chunk (made on the host: fourier_resample_layout.hpp): signal d of the chunk at work + d * Mw, Mw = max(M2, the
// chunk's largest M1) (a uniform stride, as the pass kernels and resample_block_kernel take it), then the chunk's tables back to back.
// A signal's result depends only on its own samples, n and num: not on its neighbours, its place in the list or the chunking
// (the twiddle table of a larger Mt holds the same bits at the indices a smaller one uses: k * 2^j / (Mt * 2^j) is exact).
#pragma once
#include <hip/hip_runtime.h>

#include "fourier_resample_gpu.hpp"
#include "fourier_resample_layout.hpp"

namespace hssfsst {

// w[m] = exp(+i pi (m^2 mod 2n) / n), m < n <= 2^26 (m^2 < 2^52: exact in int64)
__device__ __forceinline__ double2 rg_chirp(long long n, long long m)
{
    const long long r = (m * m) % (2 * n);
    double s, c;
    sincos(M_PI * static_cast<double>(r) / static_cast<double>(n), &s, &c);
    return make_double2(c, s);
}

// The signals of a chunk (ResampleArgs' counterpart): descriptor d of `sig`; the chirp and the Nyquist rule from the signal's own n.
struct RaggedResampleArgs {
    const void* x;                   // float32 or float64 samples
    long long num;
    int x_f64, y_f64, num_even, M2;
    const double2* c2;               // [num]: the inverse chirp (plan)
    void* y;                         // [count][num] float32 / float64, or null
    long long* labels;               // [count][num] int64, or null
    const RaggedResampleSig* sig;    // the chunk's descriptors

    __device__ __forceinline__ long long signal(long long d) const { return d; }
    __device__ __forceinline__ long long start(long long d) const { return sig[d].start; }
    __device__ __forceinline__ long long len(long long d) const { return sig[d].n; }
    __device__ __forceinline__ long long row(long long d) const { return sig[d].row; }
    __device__ __forceinline__ double scale(long long d) const { return 1.0 / static_cast<double>(sig[d].n); }
    // (w.x, -w.y): a product with it rounds as the product with w.y, sign flipped
    __device__ __forceinline__ double2 conj_chirp(long long d, long long m) const { const double2 w = rg_chirp(sig[d].n, m); return make_double2(w.x, -w.y); }
    __device__ __forceinline__ long long kept(long long d) const { return sig[d].n < num ? sig[d].n : num; }
    __device__ __forceinline__ long long kept_bins(long long d) const { return kept(d) / 2 + 1; }
    __device__ __forceinline__ long long nyquist_bin(long long d) const { return kept(d) % 2 == 0 && sig[d].n != num ? kept(d) / 2 : -1; }
    __device__ __forceinline__ double nyquist_scale(long long d) const { return num < sig[d].n ? 2.0 : 0.5; }
    __device__ __forceinline__ long long mid_reads(long long d) const { return kept_bins(d); } // (only the bins it keeps)
    // a signal takes Mw threads (the chunk's stride); those from its M1 on load nothing
    __device__ __forceinline__ bool load_point(long long t, long long Mw, long long& d, long long& m) const { d = t / Mw; m = t - d * Mw; return m < sig[d].M1; }
};

// the wrapped chirp of n on M points: b[0] = w[0], b[m] = b[M - m] = w[m] for 0 < m < n, zero between; one thread per point of
// every table of a class (tables of M points back to back, tn[u] = the length of table u)
__global__ __launch_bounds__(kRsThreads) void resample_ragged_table_kernel(double2* tabs, const long long* __restrict__ tn, int M,
                                                                          long long total)
{
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long u = t / M, j = t - u * M, n = tn[u];
    double2 v = make_double2(0.0, 0.0);
    if (j < n) v = rg_chirp(n, j);
    else if (j > M - n) v = rg_chirp(n, M - j);
    tabs[t] = v;
}

// the in-LDS end of a table's DIF FFT: blocks of S = min(M, kRsBlock) contiguous points (blockIdx.x = table * (M / S) + block),
// stages len = S .. 4, then the last stage (len 2, twiddle 1) with the 1 / M scale, stored from registers
__global__ __launch_bounds__(kRsThreads) void resample_ragged_table_block_kernel(double2* tabs, int M, int S,
                                                                                const double2* __restrict__ tw, int Mt)
{
    __shared__ double2 s[kRsBlock];
    const int nblk = M / S;
    const long long u = blockIdx.x / nblk;
    double2* w = tabs + u * M + static_cast<long long>(blockIdx.x - u * nblk) * S;
    for (int m = threadIdx.x; m < S; m += blockDim.x) s[m] = w[m];
    __syncthreads();
    rs_lds_dif(s, S, S, tw, Mt);
    const double inv = 1.0 / static_cast<double>(M);
    if (S == 1) {
        if (threadIdx.x == 0) w[0] = make_double2(s[0].x * inv, s[0].y * inv);
    } else {
        for (int t = threadIdx.x; t < (S >> 1); t += blockDim.x) {
            const int i = t << 1;
            const double2 a = s[i], b = s[i + 1];
            w[i] = make_double2((a.x + b.x) * inv, (a.y + b.y) * inv);
            w[i + 1] = make_double2((a.x - b.x) * inv, (a.y - b.y) * inv);
        }
    }
}

// resample_block_kernel with each signal's own B1 / M1 table, in the chunk's table region `tabs`
struct RsRaggedB {
    const RaggedResampleSig* __restrict__ sig;
    const double2* __restrict__ tabs;
};
__device__ __forceinline__ const double2* rs_kernel_of(const RsRaggedB& t, long long b) { return t.tabs + t.sig[b].tab; }

}  // namespace hssfsst
