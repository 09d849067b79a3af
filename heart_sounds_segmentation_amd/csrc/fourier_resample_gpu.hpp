// fourier_resample_gpu.hpp -- device counterpart of fourier_resample.hpp: scipy.signal.resample(x, num) for a BATCH of real
// signals of n samples, in fp64 on the device whatever the input / output dtypes.
//
// Same algorithm as the host helper: both DFTs run as Bluestein chirp-z convolutions on power-of-two FFTs.  Everything that
// depends only on (n, num) is made once on the host, in fp64, by the plan (resample.hip: hssfsst_resample_plan_create):
//   c1[m] = conj(w1[m]), m < n          w1[m] = exp(+i pi (m^2 mod 2n) / n)        forward chirp (N = n)
//   B1[j] = FFT_M1(b1)[bitrev(j)] / M1  b1 = w1 wrapped symmetrically into M1 >= 2n - 1 points
//   c2, B2: the same for the inverse DFT (N = num, chirp sign flipped, M2 >= 2 num - 1)
//   tw[k]  = exp(-2 pi i k / Mt), k < Mt / 2, Mt = max(M1, M2): the twiddles of every FFT stage (table, no recurrence)
// A convolution is a decimation-in-frequency FFT (natural order in, bit-reversed out), a pointwise product with the
// bit-reversed B, and a decimation-in-time inverse FFT (bit-reversed in, natural out): no bit-reversal pass anywhere.
//
// Between the two convolutions the half spectrum is formed in place.  The irfft of length num is written as the real part
// of a length-num inverse DFT of a sequence that is zero above the kept bins:
//   y[i] = Re sum_{k < nyq} Y'[k] exp(+2 pi i i k / num),  Y'[0] = Re Y[0],  Y'[num/2] = Re Y[num/2] (num even),
//   Y'[k] = 2 Y[k] otherwise
// which equals the host helper's Hermitian extension mathematically and needs no permutation of the LDS array.
//
// Two tiers:
//   resample_lds_kernel     max(M1, M2) <= kRsLdsMax: one workgroup per signal, the whole convolution in LDS (up to 128 KiB),
//                           input read from global memory, output and labels stored from LDS: one launch.
//   large tier              longer signals (whole recordings): the convolution lives in a global scratch array; the stages
//                           whose butterflies span more than kRsBlock points run as one launch per stage
//                           (resample_dif_pass_kernel / resample_dit_pass_kernel, one thread per butterfly over all signals
//                           of the chunk), the remaining log2(kRsBlock) stages on each side and the pointwise product as ONE
//                           launch of resample_block_kernel per convolution (contiguous kRsBlock-point blocks in LDS).
//                           Its steps are templates over the launch's signals: this file's ResampleArgs (a plan's n and tables) or
//                           fourier_resample_ragged.hpp's RaggedResampleArgs (a list of lengths, one descriptor per signal).
// A NaN anywhere in a signal reaches every butterfly of the first FFT and so every output sample, as on the host.
#pragma once
#include <hip/hip_runtime.h>

namespace hssfsst {

constexpr int kRsThreads = 256;
constexpr int kRsLdsMax = 8192;      // complex fp64 points held by the LDS tier (128 KiB of the 160 KiB per CU)
constexpr int kRsBlock = 4096;       // points per in-LDS block of the large tier (64 KiB: two workgroups per CU)

struct ResampleArgs {
    const void* x;                   // float32 or float64 samples
    long long x_stride;              // strided form: signal b starts at b * x_stride
    const long long* starts;         // list form (non-null): signal b starts at starts[b]
    long long n, num, nyq;           // nyq = min(n, num) / 2 + 1 kept bins
    long long nyq_bin;               // bin scaled by nyq_scale (min(n, num) even and n != num), else -1
    double nyq_scale, inv_n;
    int x_f64, y_f64, num_even;
    int M1, M2, Mt;                  // convolution lengths (powers of two) and twiddle-table length
    const double2* c1; const double2* B1; const double2* c2; const double2* B2; const double2* tw;
    void* y;                         // [batch][num] float32 / float64, or null
    long long* labels;               // [batch][num] int64, or null
    long long b0;                    // first signal of this launch (large tier: chunks of the batch)

    // The signals of a launch as every step sees them: what is asked about signal b, here answered from the plan's host-made
    // tables (RaggedResampleArgs, fourier_resample_ragged.hpp: from a list's descriptors).  Both have x, y, labels, num,
    // num_even, M2, c2 and the dtypes as members.
    __device__ __forceinline__ long long signal(long long d) const { return b0 + d; }          // b of the launch's d-th signal
    __device__ __forceinline__ long long start(long long b) const { return starts ? starts[b] : b * x_stride; }
    __device__ __forceinline__ long long len(long long) const { return n; }
    __device__ __forceinline__ long long row(long long b) const { return b; }
    __device__ __forceinline__ double scale(long long) const { return inv_n; }                 // 1 / n
    __device__ __forceinline__ double2 conj_chirp(long long, long long m) const { return c1[m]; }
    __device__ __forceinline__ long long kept_bins(long long) const { return nyq; }
    __device__ __forceinline__ long long nyquist_bin(long long) const { return nyq_bin; }
    __device__ __forceinline__ double nyquist_scale(long long) const { return nyq_scale; }
    __device__ __forceinline__ long long mid_reads(long long) const { return M1; }             // bins the large tier's middle step reads (>= nyq)
    // large tier: thread t of the load -> point m of the launch's d-th signal (false: none); a signal takes M1 threads
    __device__ __forceinline__ bool load_point(long long t, long long, long long& d, long long& m) const { d = t / M1; m = t - d * M1; return true; }
};

__device__ __forceinline__ double2 rs_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 rs_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 rs_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 rs_mulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a conj(b)

template <class V>
__device__ __forceinline__ double rs_load_x(const V& a, long long b, long long m)
{
    const long long base = a.start(b);
    return a.x_f64 ? static_cast<const double*>(a.x)[base + m] : static_cast<double>(static_cast<const float*>(a.x)[base + m]);
}

// first convolution's input: the chirp-weighted signal, zero above n
template <class V>
__device__ __forceinline__ double2 rs_conv1_in(const V& a, long long b, long long m)
{
    if (m >= a.len(b)) return make_double2(0.0, 0.0);
    const double v = rs_load_x(a, b, m);
    const double2 c = a.conj_chirp(b, m);
    return make_double2(v * c.x, v * c.y);
}

// between the convolutions: bin k of the forward DFT -> the kept half spectrum Y' -> the second convolution's input
template <class V>
__device__ __forceinline__ double2 rs_mid(const V& a, long long b, double2 conv, long long k)
{
    if (k >= a.kept_bins(b)) return make_double2(0.0, 0.0);
    double2 X = rs_mul(conv, a.conj_chirp(b, k));
    if (k == a.nyquist_bin(b)) { const double sc = a.nyquist_scale(b); X.x *= sc; X.y *= sc; }
    if (k == 0 || (a.num_even && 2 * k == a.num)) X = make_double2(X.x, 0.0);
    else { X.x *= 2.0; X.y *= 2.0; }
    return rs_mul(X, a.c2[k]);
}

// last step: sample i of signal b
template <class V>
__device__ __forceinline__ void rs_store(const V& a, long long b, double2 conv, long long i)
{
    const double2 c = a.c2[i];
    const double v = (conv.x * c.x - conv.y * c.y) * a.scale(b);
    const long long o = a.row(b) * a.num + i;
    if (a.y) {
        if (a.y_f64) static_cast<double*>(a.y)[o] = v;
        else static_cast<float*>(a.y)[o] = static_cast<float>(v);
    }
    // the dataset's label rule (hss/datasets/heart_sounds.py:205-206): round(t(y)) - 1 with t's default dtype float32,
    // torch.round = round half to even = rintf
    if (a.labels) a.labels[o] = static_cast<long long>(rintf(static_cast<float>(v))) - 1;
}

// Decimation-in-frequency stages len = Lhi, Lhi/2, ..., 4 over S points in LDS (each len-block transformed in place).
__device__ __forceinline__ void rs_lds_dif(double2* s, int S, int Lhi, const double2* __restrict__ tw, int Mt)
{
    for (int len = Lhi; len >= 4; len >>= 1) {
        const int half = len >> 1, step = Mt / len;
        for (int t = threadIdx.x; t < (S >> 1); t += blockDim.x) {
            const int j = t & (half - 1), i = ((t - j) << 1) + j;
            const double2 u = s[i], v = s[i + half];
            s[i] = rs_add(u, v);
            s[i + half] = rs_mul(rs_sub(u, v), tw[j * step]);
        }
        __syncthreads();
    }
}

// Decimation-in-time stages len = 4, 8, ..., Lhi (conjugate twiddles: the inverse transform, unscaled).
__device__ __forceinline__ void rs_lds_dit(double2* s, int S, int Lhi, const double2* __restrict__ tw, int Mt)
{
    for (int len = 4; len <= Lhi; len <<= 1) {
        const int half = len >> 1, step = Mt / len;
        for (int t = threadIdx.x; t < (S >> 1); t += blockDim.x) {
            const int j = t & (half - 1), i = ((t - j) << 1) + j;
            const double2 u = s[i], v = rs_mulc(s[i + half], tw[j * step]);
            s[i] = rs_add(u, v);
            s[i + half] = rs_sub(u, v);
        }
        __syncthreads();
    }
}

// The last DIF stage (len 2), the product with B (bit-reversed order: position g0 + i of the convolution) and the first DIT
// stage (len 2) act on the same pairs: one pass.
__device__ __forceinline__ void rs_lds_pointwise(double2* s, int S, const double2* __restrict__ B, long long g0)
{
    if (S == 1) {
        if (threadIdx.x == 0) s[0] = rs_mul(s[0], B[g0]);
    } else {
        for (int t = threadIdx.x; t < (S >> 1); t += blockDim.x) {
            const int i = t << 1;
            const double2 u = s[i], v = s[i + 1];
            const double2 p = rs_mul(rs_add(u, v), B[g0 + i]), q = rs_mul(rs_sub(u, v), B[g0 + i + 1]);
            s[i] = rs_add(p, q);
            s[i + 1] = rs_sub(p, q);
        }
    }
    __syncthreads();
}

// A whole convolution of M <= S points in LDS.
__device__ __forceinline__ void rs_lds_conv(double2* s, int M, const double2* __restrict__ B, const double2* __restrict__ tw, int Mt)
{
    rs_lds_dif(s, M, M, tw, Mt);
    rs_lds_pointwise(s, M, B, 0);
    rs_lds_dit(s, M, M, tw, Mt);
}

// LDS tier: one workgroup per signal (blockIdx.x), dynamic LDS of max(M1, M2) complex doubles.
__global__ __launch_bounds__(kRsThreads) void resample_lds_kernel(ResampleArgs a)
{
    extern __shared__ double2 rs_lds[];
    const long long b = a.b0 + blockIdx.x;
    for (int m = threadIdx.x; m < a.M1; m += blockDim.x) rs_lds[m] = rs_conv1_in(a, b, m);
    __syncthreads();
    rs_lds_conv(rs_lds, a.M1, a.B1, a.tw, a.Mt);
    // each thread reads and writes only its own indices: no barrier inside
    for (int k = threadIdx.x; k < a.M2; k += blockDim.x) rs_lds[k] = rs_mid(a, b, k < a.M1 ? rs_lds[k] : make_double2(0.0, 0.0), k);
    __syncthreads();
    rs_lds_conv(rs_lds, a.M2, a.B2, a.tw, a.Mt);
    for (int i = threadIdx.x; i < a.num; i += blockDim.x) rs_store(a, b, rs_lds[i], i);
}

// ---------------------------------------------------------------------------------------------------- large tier
// work: [chunk][Mw] complex doubles, signal d of the chunk at work + d * Mw.  V: the chunk's signals (ResampleArgs, RaggedResampleArgs).

template <class V>
__global__ __launch_bounds__(kRsThreads) void resample_load_kernel(V a, double2* work, long long Mw, long long total)
{
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= total) return;
    long long d, m;
    if (!a.load_point(t, Mw, d, m)) return;
    work[d * Mw + m] = rs_conv1_in(a, a.signal(d), m);
}

template <class V>
__global__ __launch_bounds__(kRsThreads) void resample_mid_kernel(V a, double2* work, long long Mw, long long total)
{
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long M2 = a.M2, d = t / M2, k = t - d * M2;
    double2* w = work + d * Mw;
    const long long b = a.signal(d);
    w[k] = rs_mid(a, b, k < a.mid_reads(b) ? w[k] : make_double2(0.0, 0.0), k);
}

template <class V>
__global__ __launch_bounds__(kRsThreads) void resample_store_kernel(V a, const double2* work, long long Mw, long long total)
{
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long d = t / a.num, i = t - d * a.num;
    rs_store(a, a.signal(d), work[d * Mw + i], i);
}

// one DIF stage of length len over convolutions of M points; total = chunk * M / 2 butterflies
__global__ __launch_bounds__(kRsThreads) void resample_dif_pass_kernel(double2* work, long long Mw, int M, int len,
                                                                      const double2* __restrict__ tw, int Mt, long long total)
{
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long hb = M >> 1, b = t / hb;
    const int r = static_cast<int>(t - b * hb), half = len >> 1, j = r & (half - 1), i = ((r - j) << 1) + j;
    double2* w = work + b * Mw;
    const double2 u = w[i], v = w[i + half];
    w[i] = rs_add(u, v);
    w[i + half] = rs_mul(rs_sub(u, v), tw[static_cast<long long>(j) * (Mt / len)]);
}

__global__ __launch_bounds__(kRsThreads) void resample_dit_pass_kernel(double2* work, long long Mw, int M, int len,
                                                                      const double2* __restrict__ tw, int Mt, long long total)
{
    const long long t = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long hb = M >> 1, b = t / hb;
    const int r = static_cast<int>(t - b * hb), half = len >> 1, j = r & (half - 1), i = ((r - j) << 1) + j;
    double2* w = work + b * Mw;
    const double2 u = w[i], v = rs_mulc(w[i + half], tw[static_cast<long long>(j) * (Mt / len)]);
    w[i] = rs_add(u, v);
    w[i + half] = rs_sub(u, v);
}

// BS, where the kernel B (bit-reversed spectrum / M) of signal b of a launch is: RsSharedB, one B for every signal (a plan's B1 or
// B2), or fourier_resample_ragged.hpp's RsRaggedB, each signal's own table
using RsSharedB = const double2* __restrict__;
__device__ __forceinline__ const double2* rs_kernel_of(RsSharedB B, long long) { return B; }

// the in-LDS middle of a convolution of M points: blocks of S = min(M, kRsBlock) contiguous points, blockIdx.x =
// signal * (M / S) + block
template <class BS>
__global__ __launch_bounds__(kRsThreads) void resample_block_kernel(double2* work, long long Mw, int M, int S, BS B,
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
    rs_lds_pointwise(s, S, rs_kernel_of(B, b), g0);
    rs_lds_dit(s, S, S, tw, Mt);
    for (int m = threadIdx.x; m < S; m += blockDim.x) w[m] = s[m];
}

}  // namespace hssfsst
