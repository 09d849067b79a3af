// fsst_generic.hip -- the unit of the FSST kernels that are neither the MFMA core nor the canonical-band kernels: the generic VALU
// kernel (fsst_kernels.hpp: nwin 32 / 64 and the fallback of the MFMA lengths), the any-length kernel (fsst_dft.hpp), the z-score as
// its own launches, dense (fsst_kernels.hpp) and ragged (fsst_ragged.hpp), the frame gather (fsst_gather.hpp), the running moments
// and a streaming step's tail.  No other unit instantiates these kernels.
#include "fsst_plan.hpp"

#include "fsst_kernels.hpp"
#include "fsst_dft.hpp"
#include "fsst_gather.hpp"
#include "fsst_ragged.hpp"

namespace hssfsst {
namespace host __attribute__((visibility("hidden"))) {

template <int R>
int launch_core(hssfsst_plan* pl, ExecCtx& cx, hssfsst::CoreParams cp, long long nblocks)
{
    constexpr int NWIN = 32 * R;
    constexpr int XS = ((kTile + NWIN - 1 + 3) / 4) * 4;
    size_t lds = (static_cast<size_t>(XS) + static_cast<size_t>(4 * pl->K) * (kTile + 1)) * sizeof(float);
    cp.oneplane = 0;
    // wide band: own and displaced values share one plane.  Needed above 160 KiB (nwin 512, > ~150 kept rows) and
    // already worth it above 40 KiB, where LDS is what limits the resident waves (measured, 1024 x 2000, band
    // [25,200] Hz: nwin 256 core 2.25 -> 1.44 ms, nwin 512 18.9 -> 9.4 ms)
    if (lds > 40 * 1024) {
        lds = (static_cast<size_t>(XS) + static_cast<size_t>(2 * pl->K) * (kTile + 1)) * sizeof(float);
        cp.oneplane = 1;
    }
    if (lds > 160 * 1024) return fail(HSSFSST_EUNSUPPORTED, "LDS request %zu B exceeds 160 KiB", lds);
    auto kern = hssfsst::fsst_core_kernel<R, kTile>;
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = allow_full_lds(kern, pl->device, lds_ok)) return rc;
    name_kernel(cx.kernel, 1, nblocks, "fsst_core_kernel<%d, %d>", R, kTile);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(nblocks)), dim3(kTile), lds, cx.st, cp);
    HIP_TRY(hipGetLastError());
    return 0;
}

// f(o) with an exec's output `out` as what the plan says it holds: float*, _Float16* or __bf16*
template <class F>
void out_dispatch(const hssfsst_plan* p, void* out, F&& f)
{
    if (p->out_dtype == HSSFSST_DTYPE_F16) f(static_cast<_Float16*>(out));
    else if (p->out_dtype == HSSFSST_DTYPE_BF16) f(static_cast<__bf16*>(out));
    else f(static_cast<float*>(out));
}

// the generic kernel of the plan's radix R = nwin / 32
int launch_core_radix(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::CoreParams& cp, long long nblocks)
{
    switch (pl->R) {
    case 1: return launch_core<1>(pl, cx, cp, nblocks);
    case 2: return launch_core<2>(pl, cx, cp, nblocks);
    case 4: return launch_core<4>(pl, cx, cp, nblocks);
    case 8: return launch_core<8>(pl, cx, cp, nblocks);
    case 16: return launch_core<16>(pl, cx, cp, nblocks);
    default: return fail(HSSFSST_EUNSUPPORTED, "exec: unsupported radix %d", pl->R);
    }
}

// The any-length kernel (fsst_dft.hpp) for one exec: its tile search and launch
int launch_dft(hssfsst_plan* p, ExecCtx& cx, const float* dx, float* kout, int64_t batch, int n, int64_t x_stride, int col0, int ncols)
{
    hssfsst::DftParams dp{};
    dp.x = dx; dp.out = kout; dp.partials = p->d_partials.get(); dp.atab = p->d_dtab.get();
    dp.wtab = p->d_wtab.get(); dp.twtab = p->d_wtab.get() + 2 * p->nwin;
    dp.n = n; dp.nwin = p->nwin; dp.nf = p->nf; dp.klo = p->klo; dp.K = p->K; dp.mode = p->mode; dp.col0 = col0; dp.ncols = ncols;
    dp.nk4 = (p->nwin + 3) / 4; dp.nblk4 = (p->nf + 3) / 4;
    dp.xstride = x_stride; dp.r2scale = p->r2scale;
    const hssfsst::DftShape sh = hssfsst::dft_shape(dp.nk4, p->K, ncols, batch);
    const int G = sh.G, waves = sh.waves;
    const size_t per_wave = static_cast<size_t>(hssfsst::dft_wave_lds_floats(dp.nk4, p->K, G)) * sizeof(float);
    if (waves < 1) return fail(HSSFSST_EUNSUPPORTED, "exec: LDS request %zu B per wave exceeds 160 KiB", per_wave);
    dp.nitems = sh.nitems;
    auto launch = [&](auto kern) -> int {
        static std::atomic<unsigned long long> lds_ok{0};
        if (int r2 = allow_full_lds(kern, p->device, lds_ok)) return r2;
        name_kernel(cx.kernel, waves, sh.blocks, "fsst_dft_kernel<%d>", G);
        hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(sh.blocks)), dim3(64 * waves), per_wave * waves, cx.st, dp);
        return (hipGetLastError() == hipSuccess) ? 0 : fail(HSSFSST_EHIP, "exec: fsst_dft_kernel launch failed");
    };
    return (G == 4) ? launch(hssfsst::fsst_dft_kernel<4>) : (G == 2) ? launch(hssfsst::fsst_dft_kernel<2>) : launch(hssfsst::fsst_dft_kernel<1>);
}

// The z-score of a dense STACK exec whose core launch left it to do: `feats` = the un-normalised float32 features [batch][ncols][2K]
// with their statistics partials in d_partials, `out` = the exec's output in the plan's element type (float32: feats itself, swept
// in place; a half plan: out of place from its float32 scratch).  (cx.gate non-null: a team launch went first; these launches are
// its gated fallback.)
int launch_zscore(hssfsst_plan* p, const ExecCtx& cx, const float* feats, void* out, int64_t batch, int nblk, int fpp, int ncols)
{
    float4* stats = reinterpret_cast<float4*>(p->d_stats.get());
    const float* partials = p->d_partials.get();
    const hssfsst::ZscoreShape z = hssfsst::zscore_shape(batch);
    if (!z.fused)
        hipLaunchKernelGGL(hssfsst::fsst_stats_kernel, dim3(static_cast<unsigned>(batch)), dim3(64), 0, cx.st,
                           partials, stats, nblk, fpp, ncols, p->K, cx.gate, cx.gate_val);
    out_dispatch(p, out, [&](auto* o) {
        hipLaunchKernelGGL(hssfsst::fsst_normalize_kernel<std::remove_pointer_t<decltype(o)>>, dim3(static_cast<unsigned>(z.grid)), dim3(256), 0, cx.st,
                           feats, o, stats, z.fused ? partials : nullptr, nblk, fpp, ncols, p->K, static_cast<int>(batch), z.slices,
                           cx.gate, cx.gate_val);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// The z-score of a ragged STACK exec (fsst_ragged.hpp): per-signal statistics, then one sweep over the list's `nunits` units;
// feats and out as in launch_zscore, rsig and unit0 the list's device tables
int launch_zscore_ragged(hssfsst_plan* p, const ExecCtx& cx, const float* feats, void* out, int64_t batch,
                         const hssfsst::RaggedSignal* rsig, const int* unit0, long long nunits)
{
    float4* stats = reinterpret_cast<float4*>(p->d_stats.get());
    hipLaunchKernelGGL(hssfsst::fsst_ragged_stats_kernel, dim3(static_cast<unsigned>(batch)), dim3(64), 0, cx.st, p->d_partials.get(), rsig, stats, p->K);
    const long long zgrid = std::min<long long>(nunits, 65536);
    out_dispatch(p, out, [&](auto* o) {
        hipLaunchKernelGGL(hssfsst::fsst_ragged_normalize_kernel<std::remove_pointer_t<decltype(o)>>, dim3(static_cast<unsigned>(zgrid)), dim3(256), 0, cx.st,
                           feats, o, rsig, unit0, stats, static_cast<int>(batch), p->K);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

// A frame list's frames, gathered into the dense [batch][n] block `frames` (exec_impl)
int launch_gather_frames(const float* dx, const long long* d_starts, float* frames, int64_t batch, int n, hipStream_t st)
{
    const long long quads = (static_cast<long long>(n) + 3) / 4;
    long long blocks = (static_cast<long long>(batch) * quads + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(hssfsst::fsst_gather_frames_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st,
                       dx, d_starts, frames, static_cast<long long>(batch), n);
    HIP_TRY(hipGetLastError());
    return 0;
}

// hssfsst_moments_merge
int launch_moments_merge(const hssfsst_plan* p, const float* feats, int64_t batch, int n, double* state, hipStream_t st)
{
    hipLaunchKernelGGL(hssfsst::fsst_moments_merge_kernel, dim3(static_cast<unsigned>(batch)), dim3(hssfsst::kMomThreads), 0,
                       st, feats, state, n, p->K);
    HIP_TRY(hipGetLastError());
    return 0;
}

// hssfsst_normalize_running: the statistics of the running state into `stats` (4 floats per signal), then the in-place sweep
int launch_normalize_running(const hssfsst_plan* p, float* feats, int64_t batch, int n, const double* state, float4* stats, hipStream_t st)
{
    hipLaunchKernelGGL(hssfsst::fsst_stats_from_state_kernel, dim3(static_cast<unsigned>((batch + 63) / 64)), dim3(64), 0, st,
                       state, stats, static_cast<int>(batch));
    const int64_t zgrid = batch < 4096 ? batch : 4096;
    hipLaunchKernelGGL(hssfsst::fsst_normalize_kernel<float>, dim3(static_cast<unsigned>(zgrid)), dim3(256), 0, st,
                       static_cast<const float*>(feats), feats, stats, static_cast<const float*>(nullptr), 0, 0, n, p->K, static_cast<int>(batch), 1);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the tail of a streaming step that took the three-launch route: merge the chunk into the running moments and normalise it
int launch_stream_finish(const hssfsst_plan* p, float* out, double* state, int channels, int chunk, hipStream_t st)
{
    hipLaunchKernelGGL(hssfsst::fsst_stream_finish_kernel, dim3(static_cast<unsigned>(channels)), dim3(hssfsst::kMomThreads), 0, st, out, state, chunk, p->K);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace host
}  // namespace hssfsst
