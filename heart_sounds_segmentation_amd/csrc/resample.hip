// resample.hip -- the Fourier resampler's host side: the dense and the ragged device plan (kernels: fourier_resample_gpu.hpp,
// fourier_resample_ragged.hpp) and the CPU hssfsst_resample.  C ABI: include/hssfsst.h.
#include "host_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "fourier_resample.hpp"
#include "fourier_resample_layout.hpp"
#include "fourier_resample_gpu.hpp"
#include "fourier_resample_ragged.hpp"

namespace rslayout = hssfsst::rslayout;
using namespace hssfsst::host;

// Device resampler (hssfsst.h: hssfsst_resample_plan_create): the chirps, the convolution kernels' spectra and the twiddle
// table of one (n, num), made on the host in fp64 (csrc/fourier_resample_gpu.hpp), plus the staging of host buffers.
struct hssfsst_resample_plan {
    int device = -1;
    int64_t n = 0, num = 0;
    int M1 = 1, M2 = 1, Mt = 1;
    DevBuf<double2> d_tab;                               // c1[n] | B1[M1] | c2[num] | B2[M2] | tw[max(Mt / 2, 1)]
    const double2 *c1 = nullptr, *B1 = nullptr, *c2 = nullptr, *B2 = nullptr, *tw = nullptr;
    DevBuf<unsigned char> d_x, d_y;                      // a host input / output, staged
    DevBuf<long long> d_lab, d_starts;                   // host labels / frame starts, staged
    DevBuf<double2> d_work;                              // the large tier's convolutions [chunk][max(M1, M2)]
    // ragged plans (hssfsst_resample_plan_create_ragged, n = 0): d_tab holds c2 | B2 only; the twiddle table is its own buffer,
    // grown to the largest M of a call; the list's descriptors are made on the host and uploaded once per call
    bool ragged = false;
    DevBuf<double2> d_tw; int tw_M = 0;                  // tw[k] = exp(-2 pi i k / tw_M), k < tw_M / 2
    UploadedTable desc{"resample_exec_ragged"};          // RaggedResampleSig[count] | table lengths (int64); no key: made at every call
};

namespace {

constexpr int64_t kRsMaxLen = int64_t(1) << 26;          // n, num: convolutions of up to 2^27 points (2 GiB per signal)
using rslayout::bluestein_tables;                        // (the resampler's host arithmetic: csrc/fourier_resample_layout.hpp)
using rslayout::pow2_at_least;
constexpr long long kRsWorkElems = static_cast<long long>(rslayout::kRsWorkBytes / sizeof(double2));

unsigned rs_grid(long long total) { return static_cast<unsigned>((total + hssfsst::kRsThreads - 1) / hssfsst::kRsThreads); }

int rs_check_dtypes(const char* what, int x_dtype, const void* y, int y_dtype)
{
    if ((x_dtype != HSSFSST_DTYPE_F32 && x_dtype != HSSFSST_DTYPE_F64) || (y && y_dtype != HSSFSST_DTYPE_F32 && y_dtype != HSSFSST_DTYPE_F64))
        return fail(HSSFSST_EINVAL, "%s: unknown dtype (x %d, y %d)", what, x_dtype, y_dtype);
    return 0;
}

// A resample exec's host buffers: x_bytes of x staged in front of the launches; y (nout elements of ysz bytes) and labels (nout) given
// device buffers that rs_finish copies back.  Args: ResampleArgs or RaggedResampleArgs.
template <class Args>
int rs_stage(hssfsst_resample_plan* p, Args& a, const void* x, size_t x_bytes, int x_on_device, void* y, size_t ysz, int64_t* labels,
             size_t nout, int out_on_device, hipStream_t st)
{
    int rc;
    a.x = x;
    if (!x_on_device) {
        if ((rc = p->d_x.grow(x_bytes)) != 0) return rc;
        HIP_TRY(hipMemcpyAsync(p->d_x.get(), x, x_bytes, hipMemcpyHostToDevice, st));
        a.x = p->d_x.get();
    }
    a.y = y;
    a.labels = reinterpret_cast<long long*>(labels);
    if (!out_on_device) {
        if (y) {
            if ((rc = p->d_y.grow(nout * ysz)) != 0) return rc;
            a.y = p->d_y.get();
        }
        if (labels) {
            if ((rc = p->d_lab.grow(nout)) != 0) return rc;
            a.labels = p->d_lab.get();
        }
    }
    return 0;
}

template <class Args>
int rs_finish(const Args& a, void* y, size_t ysz, int64_t* labels, size_t nout, int x_on_device, int out_on_device, hipStream_t st)
{
    if (!out_on_device) {
        if (y) HIP_TRY(hipMemcpyAsync(y, a.y, nout * ysz, hipMemcpyDeviceToHost, st));
        if (labels) HIP_TRY(hipMemcpyAsync(labels, a.labels, nout * sizeof(long long), hipMemcpyDeviceToHost, st));
    }
    if (!out_on_device || !x_on_device) HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// Convolutions of M points, cnt of them at w (stride Mw), against a twiddle table of twM points: global DIF stages down to the block
// length S, the block kernel, global DIT stages back up.  entry: the entry point, for errors
int rs_dif(const char* entry, hipStream_t st, double2* w, long long Mw, long long cnt, int M, const double2* tw, int twM)
{
    const int S = M < hssfsst::kRsBlock ? M : hssfsst::kRsBlock;
    const long long nb = cnt * (M / 2);
    for (int len = M; len > S; len >>= 1) {
        hipLaunchKernelGGL(hssfsst::resample_dif_pass_kernel, dim3(rs_grid(nb)), dim3(hssfsst::kRsThreads), 0, st, w, Mw, M, len, tw, twM, nb);
        if (int r = launch_check(entry, "resample_dif_pass_kernel")) return r;
    }
    return 0;
}
int rs_dit(const char* entry, hipStream_t st, double2* w, long long Mw, long long cnt, int M, const double2* tw, int twM)
{
    const int S = M < hssfsst::kRsBlock ? M : hssfsst::kRsBlock;
    const long long nb = cnt * (M / 2);
    for (int len = 2 * S; len <= M; len <<= 1) {
        hipLaunchKernelGGL(hssfsst::resample_dit_pass_kernel, dim3(rs_grid(nb)), dim3(hssfsst::kRsThreads), 0, st, w, Mw, M, len, tw, twM, nb);
        if (int r = launch_check(entry, "resample_dit_pass_kernel")) return r;
    }
    return 0;
}
// BS: RsSharedB (named by the caller: deduction drops its __restrict__) or RsRaggedB
template <class BS>
int rs_conv(const char* entry, hipStream_t st, double2* w, long long Mw, long long cnt, int M, BS B, const double2* tw, int twM)
{
    const int S = M < hssfsst::kRsBlock ? M : hssfsst::kRsBlock;
    if (int r = rs_dif(entry, st, w, Mw, cnt, M, tw, twM)) return r;
    hipLaunchKernelGGL(hssfsst::resample_block_kernel<BS>, dim3(static_cast<unsigned>(cnt * (M / S))), dim3(hssfsst::kRsThreads), 0, st,
                       w, Mw, M, S, B, tw, twM);
    if (int r = launch_check(entry, "resample_block_kernel")) return r;
    return rs_dit(entry, st, w, Mw, cnt, M, tw, twM);
}

// The inverse half of a large-tier chunk, cnt signals (a: ResampleArgs or RaggedResampleArgs) whose first convolutions stand in work:
// the half spectrum in place, the second convolution (M2 points, the plan's B2), the samples and labels
template <class Args>
int rs_inverse_half(const char* entry, hipStream_t st, const Args& a, double2* work, long long Mw, long long cnt, const double2* B2,
                    const double2* tw, int twM)
{
    const long long t2 = cnt * a.M2, t3 = cnt * a.num;
    hipLaunchKernelGGL(hssfsst::resample_mid_kernel<Args>, dim3(rs_grid(t2)), dim3(hssfsst::kRsThreads), 0, st, a, work, Mw, t2);
    if (int r = launch_check(entry, "resample_mid_kernel")) return r;
    if (int r = rs_conv<hssfsst::RsSharedB>(entry, st, work, Mw, cnt, a.M2, B2, tw, twM)) return r;
    hipLaunchKernelGGL(hssfsst::resample_store_kernel<Args>, dim3(rs_grid(t3)), dim3(hssfsst::kRsThreads), 0, st, a, work, Mw, t3);
    return launch_check(entry, "resample_store_kernel");
}

// The two creates behind their argument checks: the plan on `device` with its tables c1[n] | B1[M1] | c2[num] | B2[M2] | tw[Mt / 2],
// made on the host and uploaded in one piece.  n = 0: a ragged plan, which holds c2 | B2 only (its twiddles: rs_ragged_twiddles).
int rs_plan_create(const char* what, hssfsst_resample_plan** out, int device, int64_t n, int64_t num)
{
    if (int rc = check_device(what, device)) return rc;
    DEVICE_SCOPE(device);
    using hssfsst::resample_detail::cd;
    static_assert(sizeof(cd) == sizeof(double2), "std::complex<double> and double2 share a layout");
    std::unique_ptr<hssfsst_resample_plan> p(new (std::nothrow) hssfsst_resample_plan());
    if (!p) return fail(HSSFSST_ENOMEM, "%s: host allocation failed", what);
    p->device = device; p->n = n; p->num = num; p->ragged = n == 0;
    p->M1 = p->ragged ? 0 : pow2_at_least(2 * n - 1); p->M2 = pow2_at_least(2 * num - 1);
    p->Mt = p->M1 > p->M2 ? p->M1 : p->M2;
    const size_t o_B1 = static_cast<size_t>(n), o_c2 = o_B1 + p->M1, o_B2 = o_c2 + static_cast<size_t>(num), o_tw = o_B2 + p->M2;
    const size_t total = o_tw + (p->ragged ? 0 : rslayout::twiddle_count(p->Mt));
    try {
        std::vector<cd> tab(total);
        if (!p->ragged) {
            bluestein_tables(n, p->M1, 1.0, tab.data(), tab.data() + o_B1);
            rslayout::twiddle_table(p->Mt, tab.data() + o_tw);
        }
        bluestein_tables(num, p->M2, -1.0, tab.data() + o_c2, tab.data() + o_B2);
        if (int rc = p->d_tab.upload(reinterpret_cast<const double2*>(tab.data()), total)) return rc;
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "%s: out of host memory", what);
    }
    const double2* t = p->d_tab.get();
    if (!p->ragged) { p->c1 = t; p->B1 = t + o_B1; p->tw = t + o_tw; }
    p->c2 = t + o_c2; p->B2 = t + o_B2;
    *out = p.release();
    return 0;
}

// the ragged plan's twiddle table, grown to Mt points: exp(-2 pi i k / Mt), k < Mt / 2, made on the host as the dense plan's.
// A larger table holds the same bits at the indices a smaller one uses (k 2^j / (Mt 2^j) is exact): results do not depend on it.
int rs_ragged_twiddles(hssfsst_resample_plan* p, int Mt)
{
    if (Mt <= p->tw_M) return 0;
    try {
        std::vector<hssfsst::resample_detail::cd> tw(rslayout::twiddle_count(Mt));
        rslayout::twiddle_table(Mt, tw.data());
        p->tw_M = 0;                                     // (upload's hipFree of the old table waits for the device: no earlier launch still reads it)
        if (int rc = p->d_tw.upload(reinterpret_cast<const double2*>(tw.data()), tw.size())) return rc;
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "resample_exec_ragged: out of host memory");
    }
    p->tw_M = Mt;
    return 0;
}

// The forward half of a ragged call's chunk (a.sig: its descriptors; tn: the call's table lengths on the device): B1 / M1 of every
// distinct length, the chirp-weighted signals, the first convolutions -- tables and convolutions one class of equal M1 at a time
int rs_ragged_forward_half(hssfsst_resample_plan* p, const rslayout::RaggedPlan& lay, const rslayout::Chunk& ch,
                           const hssfsst::RaggedResampleArgs& a, const long long* tn, hipStream_t st)
{
    constexpr const char* kEntry = "resample_exec_ragged";
    const double2* tw = p->d_tw.get();
    const int twM = p->tw_M;
    double2* work = p->d_work.get();
    double2* tabs = work + ch.cnt * ch.Mw;
    int rc;
    for (long long u = ch.t0; u < ch.t0 + ch.ntab;) {
        long long v = u;
        const int M = static_cast<int>(lay.tabs[static_cast<size_t>(u)].M), S = M < hssfsst::kRsBlock ? M : hssfsst::kRsBlock;
        while (v < ch.t0 + ch.ntab && lay.tabs[static_cast<size_t>(v)].M == M) ++v;
        double2* t0 = tabs + lay.tabs[static_cast<size_t>(u)].off;
        const long long tot = (v - u) * M;
        hipLaunchKernelGGL(hssfsst::resample_ragged_table_kernel, dim3(rs_grid(tot)), dim3(hssfsst::kRsThreads), 0, st, t0, tn + u, M, tot);
        if ((rc = launch_check(kEntry, "resample_ragged_table_kernel")) != 0) return rc;
        if ((rc = rs_dif(kEntry, st, t0, M, v - u, M, tw, twM)) != 0) return rc;
        hipLaunchKernelGGL(hssfsst::resample_ragged_table_block_kernel, dim3(static_cast<unsigned>((v - u) * (M / S))), dim3(hssfsst::kRsThreads),
                           0, st, t0, M, S, tw, twM);
        if ((rc = launch_check(kEntry, "resample_ragged_table_block_kernel")) != 0) return rc;
        u = v;
    }
    const long long t1 = ch.cnt * ch.Mw;
    hipLaunchKernelGGL(hssfsst::resample_load_kernel<hssfsst::RaggedResampleArgs>, dim3(rs_grid(t1)), dim3(hssfsst::kRsThreads), 0, st, a, work, ch.Mw, t1);
    if ((rc = launch_check(kEntry, "resample_load_kernel")) != 0) return rc;
    const hssfsst::RaggedResampleSig* sig = lay.sig.data() + ch.d0;
    for (long long e0 = 0; e0 < ch.cnt;) {
        long long e1 = e0;
        const int M = static_cast<int>(sig[e0].M1);
        while (e1 < ch.cnt && sig[e1].M1 == M) ++e1;
        if ((rc = rs_conv(kEntry, st, work + e0 * ch.Mw, ch.Mw, e1 - e0, M, hssfsst::RsRaggedB{a.sig + e0, tabs}, tw, twM)) != 0) return rc;
        e0 = e1;
    }
    return 0;
}

}  // namespace

extern "C" {

int hssfsst_resample_plan_create(hssfsst_resample_plan** out, int device, int64_t n, int64_t num)
{
    if (!out) return fail(HSSFSST_EINVAL, "resample_plan_create: out is NULL");
    *out = nullptr;
    if (n < 1 || num < 1 || device < 0)
        return fail(HSSFSST_EINVAL, "resample_plan_create: bad argument (device=%d n=%lld num=%lld)", device, static_cast<long long>(n),
                    static_cast<long long>(num));
    if (n > kRsMaxLen || num > kRsMaxLen)
        return fail(HSSFSST_EUNSUPPORTED, "resample_plan_create: lengths above %lld samples are not supported (n=%lld num=%lld)",
                    static_cast<long long>(kRsMaxLen), static_cast<long long>(n), static_cast<long long>(num));
    return rs_plan_create("resample_plan_create", out, device, n, num);
}

int hssfsst_resample_plan_destroy(hssfsst_resample_plan* p)
{
    if (!p) return 0;
    DeviceGuard device_guard_(p->device);
    delete p;                                            // (the buffers free themselves)
    return 0;
}

int hssfsst_resample_plan_info(const hssfsst_resample_plan* p, int64_t* n, int64_t* num, int* m1, int* m2, int* lds_tier, int* device)
{
    if (!p) return fail(HSSFSST_EINVAL, "resample_plan_info: plan is NULL");
    if (n) *n = p->n;
    if (num) *num = p->num;
    if (m1) *m1 = p->ragged ? 0 : p->M1;
    if (m2) *m2 = p->M2;
    if (lds_tier) *lds_tier = !p->ragged && p->Mt <= hssfsst::kRsLdsMax ? 1 : 0;
    if (device) *device = p->device;
    return 0;
}

int hssfsst_resample_exec(hssfsst_resample_plan* p, const void* x, int x_dtype, int64_t x_len, int64_t x_stride,
                          const int64_t* starts, int starts_on_device, int64_t batch, int x_on_device,
                          void* y, int y_dtype, int64_t* labels, int out_on_device, void* stream)
{
    if (!p || !x || (!y && !labels) || batch < 0 || x_len < 1)
        return fail(HSSFSST_EINVAL, "resample_exec: bad argument (batch=%lld x_len=%lld)", static_cast<long long>(batch),
                    static_cast<long long>(x_len));
    if (int rc = rs_check_dtypes("resample_exec", x_dtype, y, y_dtype)) return rc;
    if (batch > 0x7fffffffLL) return fail(HSSFSST_EINVAL, "resample_exec: batch %lld too large", static_cast<long long>(batch));
    if (p->ragged) return fail(HSSFSST_EINVAL, "resample_exec: a ragged plan (hssfsst_resample_plan_create_ragged) takes hssfsst_resample_exec_ragged");
    const int64_t n = p->n, num = p->num;
    if (batch == 0) return 0;
    if (!starts) {
        if (batch > 1 && x_stride < 1) return fail(HSSFSST_EINVAL, "resample_exec: signal stride %lld < 1", static_cast<long long>(x_stride));
        const int64_t span = (batch - 1) * (batch > 1 ? x_stride : 0) + n;
        if (span > x_len)
            return fail(HSSFSST_EINVAL, "resample_exec: %lld signals of %lld samples, stride %lld, need %lld samples, x holds %lld",
                        static_cast<long long>(batch), static_cast<long long>(n), static_cast<long long>(x_stride),
                        static_cast<long long>(span), static_cast<long long>(x_len));
        if (!x_on_device) x_len = span;                  // (only that much is staged)
    } else if (!starts_on_device) {
        if (x_len < n) return fail(HSSFSST_EINVAL, "resample_exec: x holds %lld samples, a signal %lld", static_cast<long long>(x_len),
                                   static_cast<long long>(n));
        for (int64_t b = 0; b < batch; ++b)
            if (starts[b] < 0 || starts[b] > x_len - n)
                return fail(HSSFSST_EINVAL, "resample_exec: signal %lld starts at %lld, outside [0, %lld]", static_cast<long long>(b),
                            static_cast<long long>(starts[b]), static_cast<long long>(x_len - n));
    }
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t xsz = x_dtype == HSSFSST_DTYPE_F64 ? sizeof(double) : sizeof(float);
    const size_t ysz = y_dtype == HSSFSST_DTYPE_F64 ? sizeof(double) : sizeof(float);
    const size_t nout = static_cast<size_t>(batch) * static_cast<size_t>(num);
    int rc;
    hssfsst::ResampleArgs a{};
    if ((rc = rs_stage(p, a, x, static_cast<size_t>(x_len) * xsz, x_on_device, y, ysz, labels, nout, out_on_device, st)) != 0) return rc;
    a.starts = reinterpret_cast<const long long*>(starts);
    if (starts && !starts_on_device) {
        if ((rc = p->d_starts.grow(static_cast<size_t>(batch))) != 0) return rc;
        HIP_TRY(hipMemcpyAsync(p->d_starts.get(), starts, static_cast<size_t>(batch) * sizeof(long long), hipMemcpyHostToDevice, st));
        a.starts = p->d_starts.get();
    }
    a.x_stride = x_stride;
    a.n = n; a.num = num;
    const int64_t N = n < num ? n : num;
    a.nyq = N / 2 + 1;
    a.nyq_bin = (N % 2 == 0 && n != num) ? N / 2 : -1;
    a.nyq_scale = num < n ? 2.0 : 0.5;
    a.inv_n = 1.0 / static_cast<double>(n);
    a.x_f64 = x_dtype == HSSFSST_DTYPE_F64; a.y_f64 = y_dtype == HSSFSST_DTYPE_F64; a.num_even = num % 2 == 0;
    a.M1 = p->M1; a.M2 = p->M2; a.Mt = p->Mt;
    a.c1 = p->c1; a.B1 = p->B1; a.c2 = p->c2; a.B2 = p->B2; a.tw = p->tw;
    a.b0 = 0;
    if (p->Mt <= hssfsst::kRsLdsMax) {
        static std::atomic<unsigned long long> lds_ok{0};
        if ((rc = allow_full_lds(hssfsst::resample_lds_kernel, p->device, lds_ok)) != 0) return rc;
        hipLaunchKernelGGL(hssfsst::resample_lds_kernel, dim3(static_cast<unsigned>(batch)), dim3(hssfsst::kRsThreads),
                           static_cast<size_t>(p->Mt) * sizeof(double2), st, a);
        if ((rc = launch_check("resample_exec", "resample_lds_kernel")) != 0) return rc;
    } else {
        const long long Mw = p->Mt;
        const long long chunk = rslayout::dense_chunk(kRsWorkElems, Mw, batch);
        if ((rc = p->d_work.grow(static_cast<size_t>(chunk) * static_cast<size_t>(Mw))) != 0) return rc;
        double2* work = p->d_work.get();
        for (long long b0 = 0; b0 < batch; b0 += chunk) {
            const long long cb = batch - b0 < chunk ? batch - b0 : chunk, t1 = cb * p->M1;
            a.b0 = b0;
            hipLaunchKernelGGL(hssfsst::resample_load_kernel<hssfsst::ResampleArgs>, dim3(rs_grid(t1)), dim3(hssfsst::kRsThreads), 0, st, a, work, Mw, t1);
            if ((rc = launch_check("resample_exec", "resample_load_kernel")) != 0) return rc;
            if ((rc = rs_conv<hssfsst::RsSharedB>("resample_exec", st, work, Mw, cb, p->M1, p->B1, p->tw, p->Mt)) != 0) return rc;
            if ((rc = rs_inverse_half("resample_exec", st, a, work, Mw, cb, p->B2, p->tw, p->Mt)) != 0) return rc;
        }
    }
    return rs_finish(a, y, ysz, labels, nout, x_on_device, out_on_device, st);
}

int hssfsst_resample_plan_create_ragged(hssfsst_resample_plan** out, int device, int64_t num)
{
    if (!out) return fail(HSSFSST_EINVAL, "resample_plan_create_ragged: out is NULL");
    *out = nullptr;
    if (num < 1 || device < 0)
        return fail(HSSFSST_EINVAL, "resample_plan_create_ragged: bad argument (device=%d num=%lld)", device, static_cast<long long>(num));
    if (num > kRsMaxLen)
        return fail(HSSFSST_EUNSUPPORTED, "resample_plan_create_ragged: lengths above %lld samples are not supported (num=%lld)",
                    static_cast<long long>(kRsMaxLen), static_cast<long long>(num));
    return rs_plan_create("resample_plan_create_ragged", out, device, 0, num);
}

int hssfsst_resample_exec_ragged(hssfsst_resample_plan* p, const void* x, int x_dtype, int64_t x_len, const int64_t* starts,
                                 const int64_t* lens, int64_t count, int x_on_device, void* y, int y_dtype, int64_t* labels,
                                 int out_on_device, void* stream)
{
    if (!p || !x || !starts || !lens || (!y && !labels) || count < 0 || x_len < 0)
        return fail(HSSFSST_EINVAL, "resample_exec_ragged: bad argument (count=%lld x_len=%lld)", static_cast<long long>(count),
                    static_cast<long long>(x_len));
    if (!p->ragged) return fail(HSSFSST_EINVAL, "resample_exec_ragged: a dense plan (hssfsst_resample_plan_create) takes hssfsst_resample_exec");
    if (int rc = rs_check_dtypes("resample_exec_ragged", x_dtype, y, y_dtype)) return rc;
    if (count > 0x7fffffffLL) return fail(HSSFSST_EINVAL, "resample_exec_ragged: count %lld too large", static_cast<long long>(count));
    bool too_long = false;
    long long xlo = x_len, xhi = 0;
    for (int64_t i = 0; i < count; ++i) {
        if (lens[i] < 1) return fail(HSSFSST_EINVAL, "resample_exec_ragged: signal %lld has %lld samples", static_cast<long long>(i),
                                     static_cast<long long>(lens[i]));
        if (starts[i] < 0 || starts[i] > x_len - lens[i])
            return fail(HSSFSST_EINVAL, "resample_exec_ragged: signal %lld spans [%lld, %lld), outside [0, %lld]", static_cast<long long>(i),
                        static_cast<long long>(starts[i]), static_cast<long long>(starts[i]) + static_cast<long long>(lens[i]),
                        static_cast<long long>(x_len));
        too_long = too_long || lens[i] > kRsMaxLen;
        xlo = std::min<long long>(xlo, starts[i]);
        xhi = std::max<long long>(xhi, starts[i] + lens[i]);
    }
    if (too_long) return fail(HSSFSST_EUNSUPPORTED, "resample_exec_ragged: signals above %lld samples are not supported", static_cast<long long>(kRsMaxLen));
    if (count == 0) return 0;
    if (x_on_device) xlo = 0;
    const int64_t num = p->num;
    const int M2 = p->M2;
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    int rc;
    // the call's plan (chunks, tables, descriptors), made on the host and uploaded; the twiddles and the work grown to it
    rslayout::RaggedPlan lay;
    if (!rslayout::plan_ragged(starts, lens, count, M2, xlo, kRsWorkElems, lay))
        return fail(HSSFSST_ENOMEM, "resample_exec_ragged: out of host memory");
    unsigned char* h_desc = nullptr;
    if ((rc = p->desc.begin(lay.desc_bytes(), &h_desc)) != 0) return rc;
    rslayout::write_descriptors(lay, h_desc);
    if ((rc = rs_ragged_twiddles(p, lay.Mt)) != 0) return rc;
    if ((rc = p->desc.commit(st)) != 0) return rc;
    const auto* dsig = reinterpret_cast<const hssfsst::RaggedResampleSig*>(p->desc.get());
    const auto* dtn = reinterpret_cast<const long long*>(p->desc.get() + lay.sig_bytes());
    if ((rc = p->d_work.grow(static_cast<size_t>(lay.max_elems))) != 0) return rc;
    // staging of host buffers, as hssfsst_resample_exec
    const size_t xsz = x_dtype == HSSFSST_DTYPE_F64 ? sizeof(double) : sizeof(float);
    const size_t ysz = y_dtype == HSSFSST_DTYPE_F64 ? sizeof(double) : sizeof(float);
    const size_t nout = static_cast<size_t>(count) * static_cast<size_t>(num);
    hssfsst::RaggedResampleArgs a{};
    if ((rc = rs_stage(p, a, static_cast<const unsigned char*>(x) + (x_on_device ? 0 : static_cast<size_t>(xlo) * xsz), static_cast<size_t>(xhi - xlo) * xsz,
                       x_on_device, y, ysz, labels, nout, out_on_device, st)) != 0) return rc;
    a.num = num; a.M2 = M2; a.c2 = p->c2;
    a.x_f64 = x_dtype == HSSFSST_DTYPE_F64; a.y_f64 = y_dtype == HSSFSST_DTYPE_F64; a.num_even = num % 2 == 0;
    for (const rslayout::Chunk& ch : lay.chunks) {
        a.sig = dsig + ch.d0;
        if ((rc = rs_ragged_forward_half(p, lay, ch, a, dtn, st)) != 0) return rc;
        if ((rc = rs_inverse_half("resample_exec_ragged", st, a, p->d_work.get(), ch.Mw, ch.cnt, p->B2, p->d_tw.get(), p->tw_M)) != 0) return rc;
    }
    return rs_finish(a, y, ysz, labels, nout, x_on_device, out_on_device, st);
}

int hssfsst_resample(const double* x, int64_t n, int64_t num, double* y)
{
    if (!x || !y || n < 1 || num < 1) return fail(HSSFSST_EINVAL, "hssfsst_resample: bad argument (n=%lld num=%lld)",
                                                   static_cast<long long>(n), static_cast<long long>(num));
    try {
        if (!hssfsst::fourier_resample(x, n, num, y)) return fail(HSSFSST_EINVAL, "hssfsst_resample: bad argument");
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "hssfsst_resample: out of host memory");
    }
    return 0;
}

}  // extern "C"
