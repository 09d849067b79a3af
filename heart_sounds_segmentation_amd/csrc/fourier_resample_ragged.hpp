// fourier_resample_ragged.hpp -- fourier_resample_gpu.hpp for a LIST of signals of different lengths n_i, all resampled to the
// same num (hssfsst.h: hssfsst_resample_exec_ragged).  Same algorithm (fp64 Bluestein on power-of-two FFTs), same butterflies
// (the large tier's DIF / DIT pass kernels and the LDS stages of fourier_resample_gpu.hpp), three differences:
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
// Work layout of a chunk: signal d of the chunk at work + d * Mw, Mw = max(M2, the chunk's largest M1) (a uniform stride: the
// existing pass kernels and resample_block_kernel run on it unchanged), then the chunk's tables back to back.
// A signal's result depends only on its own samples, n and num: not on its neighbours, its place in the list or the chunking
// (the twiddle table of a larger Mt holds the same bits at the indices a smaller one uses: k * 2^j / (Mt * 2^j) is exact).
#pragma once
#include <hip/hip_runtime.h>

#include "fourier_resample_gpu.hpp"

namespace hssfsst {

struct RaggedResampleSig {
    long long start;                 // first sample in x
    long long n;                     // samples
    long long M1;                    // forward convolution length (power of two >= 2n - 1)
    long long tab;                   // offset (double2) of its B1 / M1 table in the chunk's table region
    long long row;                   // output row (its index in the caller's list)
};

struct RaggedResampleArgs {
    const void* x;                   // float32 or float64 samples
    long long num;
    int x_f64, y_f64, num_even, M2;
    const double2* c2;               // [num]: the inverse chirp (plan)
    void* y;                         // [count][num] float32 / float64, or null
    long long* labels;               // [count][num] int64, or null
};

// w[m] = exp(+i pi (m^2 mod 2n) / n), m < n <= 2^26 (m^2 < 2^52: exact in int64)
__device__ __forceinline__ double2 rg_chirp(long long n, long long m)
{
    const long long r = (m * m) % (2 * n);
    double s, c;
    sincos(M_PI * static_cast<double>(r) / static_cast<double>(n), &s, &c);
    return make_double2(c, s);
}

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

// first convolution's input of every signal of the chunk: the chirp-weighted signal, zero from n to its M1
__global__ __launch_bounds__(kRsThreads) void resample_ragged_load_kernel(RaggedResampleArgs a, const RaggedResampleSig* __restrict__ sig,
                                                                         double2* work, long long Mw, long long total)
{
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long d = t / Mw, m = t - d * Mw;
    const RaggedResampleSig s = sig[d];
    if (m >= s.M1) return;
    double2 v = make_double2(0.0, 0.0);
    if (m < s.n) {
        const long long o = s.start + m;
        const double xv = a.x_f64 ? static_cast<const double*>(a.x)[o] : static_cast<double>(static_cast<const float*>(a.x)[o]);
        const double2 w = rg_chirp(s.n, m);                  // c1[m] = conj(w[m])
        v = make_double2(xv * w.x, -xv * w.y);
    }
    work[t] = v;
}

// the in-LDS middle of the first convolution of a class: as resample_block_kernel, with each signal's own B1 / M1 table
__global__ __launch_bounds__(kRsThreads) void resample_ragged_block_kernel(double2* work, long long Mw, int M, int S,
                                                                          const RaggedResampleSig* __restrict__ sig,
                                                                          const double2* __restrict__ tabs,
                                                                          const double2* __restrict__ tw, int Mt)
{
    __shared__ double2 s[kRsBlock];
    const int nblk = M / S;
    const long long b = blockIdx.x / nblk;
    const long long g0 = static_cast<long long>(blockIdx.x - b * nblk) * S;
    double2* w = work + b * Mw + g0;
    for (int m = threadIdx.x; m < S; m += blockDim.x) s[m] = w[m];
    __syncthreads();
    rs_lds_dif(s, S, S, tw, Mt);
    rs_lds_pointwise(s, S, tabs + sig[b].tab, g0);
    rs_lds_dit(s, S, S, tw, Mt);
    for (int m = threadIdx.x; m < S; m += blockDim.x) w[m] = s[m];
}

// between the convolutions (rs_mid with the signal's own n): bin k -> the kept half spectrum -> the second convolution's input
__global__ __launch_bounds__(kRsThreads) void resample_ragged_mid_kernel(RaggedResampleArgs a, const RaggedResampleSig* __restrict__ sig,
                                                                        double2* work, long long Mw, long long total)
{
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long d = t / a.M2, k = t - d * a.M2;
    const RaggedResampleSig s = sig[d];
    double2* w = work + d * Mw;
    const long long N = s.n < a.num ? s.n : a.num, nyq = N / 2 + 1;
    if (k >= nyq) { w[k] = make_double2(0.0, 0.0); return; }
    const double2 c = rg_chirp(s.n, k);
    double2 X = rs_mul(w[k], make_double2(c.x, -c.y));
    if (N % 2 == 0 && s.n != a.num && k == N / 2) {
        const double sc = a.num < s.n ? 2.0 : 0.5;
        X.x *= sc; X.y *= sc;
    }
    if (k == 0 || (a.num_even && 2 * k == a.num)) X = make_double2(X.x, 0.0);
    else { X.x *= 2.0; X.y *= 2.0; }
    w[k] = rs_mul(X, a.c2[k]);
}

// last step: sample i of every signal of the chunk, into its output row
__global__ __launch_bounds__(kRsThreads) void resample_ragged_store_kernel(RaggedResampleArgs a, const RaggedResampleSig* __restrict__ sig,
                                                                          const double2* work, long long Mw, long long total)
{
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long d = t / a.num, i = t - d * a.num;
    const RaggedResampleSig s = sig[d];
    const double2 conv = work[d * Mw + i], c = a.c2[i];
    const double v = (conv.x * c.x - conv.y * c.y) * (1.0 / static_cast<double>(s.n));
    const long long o = s.row * a.num + i;
    if (a.y) {
        if (a.y_f64) static_cast<double*>(a.y)[o] = v;
        else static_cast<float*>(a.y)[o] = static_cast<float>(v);
    }
    if (a.labels) a.labels[o] = static_cast<long long>(rintf(static_cast<float>(v))) - 1;     // the label rule of rs_store
}

}  // namespace hssfsst
