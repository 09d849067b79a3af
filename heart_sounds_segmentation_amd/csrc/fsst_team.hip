// fsst_team.hip -- the unit of the canonical-band kernels (nwin 128, STACK modes, the band a compile-time constant: kCanonBands of
// fsst_plan.hpp): the team kernel (fsst_team16.hpp) and fsst_canon_kernel (fsst_canon128.hpp) as two launches, ragged, and with the
// z-score in the same launch.  Both are made of canon_group; no other unit instantiates either.
#include "fsst_plan.hpp"

#include "fsst_canon128.hpp"
#include "fsst_team16.hpp"

namespace hssfsst {
namespace host __attribute__((visibility("hidden"))) {

// Team kernels: [0] arrival counter, [1] abort word on the device; the identity of the last launch that gave up in pinned host memory.
int ensure_team_words(hssfsst_plan* pl, hipStream_t st)
{
    if (pl->d_arrive.get()) return 0;
    if (int rc = pl->d_arrive.grow(4)) return rc;
    HIP_TRY(hipMemsetAsync(pl->d_arrive.get(), 0, 4 * sizeof(unsigned), st));
    pl->arrive_total = 0;
    pl->done_total = 0;
    void* h = nullptr;
    HIP_TRY(hipHostMalloc(&h, 4 * sizeof(unsigned), hipHostMallocMapped));
    for (int i = 0; i < 4; ++i) static_cast<volatile unsigned*>(h)[i] = 0u;
    void* d = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&d, h, 0));
    pl->h_fallback = static_cast<volatile unsigned*>(h);
    pl->d_fallback = static_cast<unsigned*>(d);
    return 0;
}

// Team kernel at four waves per SIMD (fsst_team16.hpp): canonical band, STACK, one 16-frame group per ticket, one group image
// held in registers.  Returns 1 when it launched, 0 when this exec should take another path, < 0 on error.
// the team kernel of output type OT: the float32 kernel, or the half-precision one (fsst_team16.hpp)
template <int KLO, int KC, int WPB, int DEPTH, class OT>
constexpr auto team16_kernel()
{
    return &hssfsst::fsst_team16_kernel<KLO, KC, WPB, DEPTH, OT>;
}
template <class OT>
constexpr const char* out_type_suffix() { return sizeof(OT) == 4 ? "" : std::is_same<OT, _Float16>::value ? ", f16" : ", bf16"; }

// OT = _Float16 / __bf16: a half plan's team launch; it stores its z-scores as 2-byte elements at hout (8-byte aligned, else 0)
template <int KLO, int KC, int WPB, int DEPTH, class OT = float>
int launch_team16(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t batch, int ngroups, void* hout = nullptr)
{
    using namespace hssfsst;
    hipStream_t st = cx.st;
    if constexpr (sizeof(OT) == 2) {
        if (hout == nullptr || (reinterpret_cast<uintptr_t>(hout) & 7) != 0) return 0;
    }
    // (at least 84 KiB: one block per CU whatever its size -- the teams count on it)
    constexpr int PSLOTS = t16_pslots<KLO, KC>();        // signals whose partials a CU keeps in LDS at a time
    constexpr int MS = t16_slots<KLO, KC>();             // statistics / mailbox slots the kernel's LDS has room for
    size_t lds = canon_lds_bytes(t16_ctl_floats(PSLOTS, MS), CanonCfg<KLO, KC>::wave_floats(), WPB);
    if (lds > static_cast<size_t>(kMaxLdsBytes)) return 0;
    if (lds < 84 * 1024) lds = 84 * 1024;
    auto kern = team16_kernel<KLO, KC, WPB, DEPTH, OT>();
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = allow_full_lds(kern, pl->device, lds_ok)) return rc;
    if (int rc = resident_blocks(pl, pl->team16_cus, kern, 64 * WPB, lds, true)) return rc;
    if (pl->team16_cus < 1) return 0;
    const Team16Geometry geo = team16_geometry(ngroups, batch, cp.xstride, pl->team16_cus, WPB, DEPTH, PSLOTS, MS);
    if (!geo.ok) return 0;
    const int T = geo.T, nteams = geo.nteams, grid = geo.grid, slots = geo.slots;
    int rc;
    if ((rc = ensure_status(pl)) != 0) return rc;
    const size_t words = static_cast<size_t>(nteams) * slots * kT16SlotWords;
    if (words > pl->d_mail.cap) {
        if ((rc = pl->d_mail.grow(words)) != 0) return rc;
        HIP_TRY(hipMemsetAsync(pl->d_mail.get(), 0, pl->d_mail.cap * sizeof(unsigned long long), st));
        pl->team_seq = 0;
    }
    if (++pl->team_seq > 0xffffu) {                      // tags would repeat: start over from clean mailboxes
        HIP_TRY(hipMemsetAsync(pl->d_mail.get(), 0, pl->d_mail.cap * sizeof(unsigned long long), st));
        pl->team_seq = 1;
    }
    Team16Params tp{};
    tp.x = cp.x; tp.out = sizeof(OT) == 4 ? cp.out : static_cast<float*>(hout); tp.atab = pl->d_atab16.get(); tp.wtab = cp.wtab; tp.twtab = cp.twtab;
    tp.mail = pl->d_mail.get(); tp.status = pl->d_status; tp.r2scale_s = pl->canon_r2s; tp.inv_c = pl->canon_inv_c;
    tp.n = cp.n; tp.nsig = cp.nsig; tp.col0 = cp.col0; tp.ncols = cp.ncols; tp.xstride = cp.xstride;
    tp.team = T; tp.cpc_shift = geo.cpc_shift; tp.slots = slots; tp.seq = pl->team_seq;
    {   // the two float64 divisions of stats_finish (correctly rounded here as there: the same bits)
        const double total = static_cast<double>(KC) * static_cast<double>(cp.ncols);
        tp.inv_total = 1.0 / total; tp.inv_total1 = 1.0 / (total - 1.0);
    }
    tp.spin_ticks = 500u * 100u;                         // a wait gives up after 500 us (100 MHz ticks)
    if ((rc = ensure_team_words(pl, st)) != 0) return rc;
    if (++pl->team_launch == 0u) pl->team_launch = 1u;
    tp.abort_word = pl->d_arrive.get() + 1; tp.fallbacks = pl->d_fallback; tp.launch = pl->team_launch;
    const bool force_fallback = debug_switches().team_force_fallback;   // tests: every team launch finds itself given up
    if (force_fallback) {
        HIP_TRY(hipMemcpyAsync(pl->d_arrive.get() + 1, &pl->team_launch, sizeof(unsigned), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(pl->d_fallback, &pl->team_launch, sizeof(unsigned), hipMemcpyHostToDevice, st));
    }
    tp.arrive = pl->d_arrive.get(); tp.arrive_base = pl->arrive_total;
    pl->arrive_total += static_cast<unsigned>(grid);     // (a plan is single-stream: every block of the earlier launches has arrived)
    if (cx.want_done_word && !force_fallback) {          // (hssfsst_exec_pinned & co: the host waits for this exec alone)
        tp.done = pl->d_arrive.get() + 2; tp.done_base = pl->done_total; tp.host_done = pl->d_fallback + 2;
        pl->done_total += static_cast<unsigned>(grid);
        cx.flagged_launch = pl->team_launch;
    }
    name_kernel(cx.kernel, WPB, grid, "fsst_team16_kernel<%d, %d, %d, %d%s> teams of %d", KLO, KC, WPB, DEPTH, out_type_suffix<OT>(), T);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(64 * WPB), lds, st, tp);
    HIP_TRY(hipGetLastError());
    cx.team_launch = pl->team_launch;
    return 1;
}

hssfsst::CanonParams canon_params(const hssfsst_plan* pl, const ExecCtx& cx, const hssfsst::Core128Params& cp)
{
    hssfsst::CanonParams q{};
    q.x = cp.x; q.out = cp.out; q.partials = cp.partials; q.atab = pl->d_atab16.get(); q.wtab = cp.wtab; q.twtab = cp.twtab;
    q.r2scale_s = pl->canon_r2s; q.inv_c = pl->canon_inv_c;
    q.n = cp.n; q.mode = cp.mode; q.nsig = cp.nsig; q.col0 = cp.col0; q.ncols = cp.ncols; q.xstride = cp.xstride; q.reg = cp.reg;
    q.status = cp.status;
    q.gate = cx.gate; q.gate_val = cx.gate_val;
    return q;
}

template <int KLO, int KC, bool RAGGED = false>
int launch_canon_band(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks)
{
    constexpr int WPB = 16;
    constexpr size_t lds = hssfsst::canon_lds_bytes(hssfsst::kCanonCtlFloats, hssfsst::CanonCfg<KLO, KC>::wave_floats(), WPB);
    static_assert(lds <= static_cast<size_t>(kMaxLdsBytes), "16 wave regions must fit");
    auto kern = hssfsst::fsst_canon_kernel<KLO, KC, false, RAGGED>;
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = allow_full_lds(kern, pl->device, lds_ok)) return rc;
    int& slots = RAGGED ? pl->ragged_slots : pl->canon_slots;
    if (int rc = resident_blocks(pl, slots, kern, 64 * WPB, lds, false)) return rc;
    int64_t blocks = nchunks < slots ? nchunks : slots;
    // (a gated launch -- the fallback behind a team launch -- almost always finds its gate closed: a quarter of the chip keeps
    //  the empty launch at ~2 us instead of ~4; when it does run, the GPU is shared anyway)
    if (cx.gate != nullptr && blocks > 64) blocks = 64;
    if (cx.gate == nullptr) name_kernel(cx.kernel, WPB, blocks, "fsst_canon_kernel<%d, %d, false%s>", KLO, KC, RAGGED ? ", ragged" : "");
    hssfsst::CanonParams q = canon_params(pl, cx, cp);
    if constexpr (RAGGED) { q.rsig = cp.rsig; q.rchunk = cp.rchunk; q.rnchunks = cp.rnchunks; }
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(64 * WPB), lds, cx.st, q);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the team kernel of the plan's band and output type (16 waves per block, two held groups per wave); hout: a half plan's output
int launch_team(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t batch, int ngroups, void* hout)
{
    return canon_dispatch(pl, [&](auto KL, auto KN) {
        constexpr int kl = decltype(KL)::value, kn = decltype(KN)::value;
        if (pl->out_dtype == HSSFSST_DTYPE_F16) return launch_team16<kl, kn, 16, 2, _Float16>(pl, cx, cp, batch, ngroups, hout);
        if (pl->out_dtype == HSSFSST_DTYPE_BF16) return launch_team16<kl, kn, 16, 2, __bf16>(pl, cx, cp, batch, ngroups, hout);
        return launch_team16<kl, kn, 16, 2>(pl, cx, cp, batch, ngroups);
    });
}

int launch_canon(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks)
{
    return canon_dispatch(pl, [&](auto KL, auto KN) { return launch_canon_band<decltype(KL)::value, decltype(KN)::value>(pl, cx, cp, nchunks); });
}

int launch_canon_ragged(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks)
{
    return canon_dispatch(pl, [&](auto KL, auto KN) { return launch_canon_band<decltype(KL)::value, decltype(KN)::value, true>(pl, cx, cp, nchunks); });
}

// One CU per signal with the z-score in the same launch (see launch_fused): 1 = launched, 0 = take another path
// gated = the fallback queued behind a team launch (cx.gate set): any batch size -- the block count is what a launch that
// almost always finds its gate closed should cost, not what would be fast.
template <int KLO, int KC>
int launch_canon_fused_band(hssfsst_plan* pl, ExecCtx& cx, hssfsst::Core128Params cp, int64_t batch, int ngroups)
{
    const bool gated = cx.gate != nullptr;
    constexpr int WPB = 16, GPC = hssfsst::kCanonTileFrames / 16;
    if (ngroups > hssfsst::kFusedMaxGroups || (ngroups + GPC - 1) / GPC < hssfsst::kFusedMinChunks) return 0;
    constexpr size_t lds = hssfsst::canon_lds_bytes(hssfsst::kCanonCtlFusedFloats, hssfsst::CanonCfg<KLO, KC>::wave_floats(), WPB);
    // (rows 2..25: 16 wave regions of 8.6 kB and the two signals' partials do not fit the 160 KiB together: team kernel or two launches)
    if constexpr (lds > static_cast<size_t>(kMaxLdsBytes)) return 0;
    else {
    auto kern = hssfsst::fsst_canon_kernel<KLO, KC, true>;
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = allow_full_lds(kern, pl->device, lds_ok)) return rc;
    if (int rc = resident_blocks(pl, pl->fused_slots, kern, 64 * WPB, lds, true)) return rc;
    if (pl->fused_slots < 1) return 0;
    int64_t grid = pl->fused_slots;
    // (gated = behind a team launch: almost always the gate is closed and 64 blocks keep the empty launch short)
    if (gated) grid = batch < 64 ? batch : 64;
    else if (!hssfsst::fused_rounds_full(batch, grid)) return 0;
    if (int rcs = ensure_status(pl)) return rcs;
    cp.status = pl->d_status;
    if (!gated) name_kernel(cx.kernel, WPB, grid, "fsst_canon_kernel<%d, %d, true>", KLO, KC);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(64 * WPB), lds, cx.st, canon_params(pl, cx, cp));
    HIP_TRY(hipGetLastError());
    return 1;
    }
}
int launch_canon_fused(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t batch, int ngroups)
{
    return canon_dispatch(pl, [&](auto KL, auto KN) { return launch_canon_fused_band<decltype(KL)::value, decltype(KN)::value>(pl, cx, cp, batch, ngroups); });
}

}  // namespace host
}  // namespace hssfsst
