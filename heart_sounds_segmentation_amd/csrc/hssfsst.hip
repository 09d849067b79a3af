// hssfsst.hip -- the FSST unit of libhssfsst.so's host side: the plan (fsst_plan.hpp) and every entry point that takes one (C ABI:
// include/hssfsst.h).  Plan creation does, once and in fp64, everything of the reference's `ssq.fsst(x, fs, window)`
// (call site /root/reference/hss/transforms/synchrosqueeze.py:48) that depends only on
// (fs, window); exec routes to the launchers of the gfx950 kernels, which live in the kernel families' own units -- fsst_team.hip,
// fsst_core128_n128.hip / _n256.hip / _n512.hip / _n512_pairs.hip, fsst_generic.hip -- so no kernel is compiled here.
// There is no CPU compute path here by design (the CPU restatement is oracle/, test-only).
// The other units: resample.hip, segmenter.hip, sequence.hip, host_io.hip; what all share: host_common.hpp.
#include "fsst_plan.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>

#include "fsst_tables.hpp"

namespace tables = hssfsst::tables;
using namespace hssfsst::host;

namespace {

void exec_report(hssfsst_plan* p, const ExecCtx& cx)
{
    std::memcpy(p->last_kernel, cx.kernel, sizeof(p->last_kernel));
    p->last_fused = (cx.fused || cx.team_launch != 0u) ? 1 : 0;      // (a team launch whose gated fallback is two launches counts as fused too)
    p->last_zpath = cx.zpath;
}

int out_floats_per_sample(const hssfsst_plan* p) { return p->mode == HSSFSST_MODE_ABS ? p->K : 2 * p->K; }

// What the host has just learnt about the plan's team launches: `gave_up` of them (seen since the last look) among `total` it knows to have
// finished.  kTeamGiveUps give-ups without a success in between -> the next kTeamPause execs skip the team kernel (hssfsst.h).
constexpr int kTeamGiveUps = 4, kTeamPause = 256;
void note_team_outcome(hssfsst_plan* p, bool gave_up)
{
    if (!gave_up) { p->giveups_in_a_row = 0; return; }
    if (++p->giveups_in_a_row >= kTeamGiveUps) { p->giveups_in_a_row = 0; p->team_pause = kTeamPause; }
}

int plan_next_event(hssfsst_plan* p, hipEvent_t* out_ev)
{
    if (p->ev.size() <= p->ev_used) {
        hipEvent_t e2 = nullptr;
        HIP_TRY(hipEventCreate(&e2));
        p->ev.push_back(e2);
    }
    *out_ev = p->ev[p->ev_used++];
    return 0;
}

// hssfsst_plan_timing: every timing_every-th exec records an event in front of its core launch, one behind it and a closing one
// behind its z-score -- or only the first two when one kernel did everything (ev_chunks -1)
void timing_begin(hssfsst_plan* p, ExecCtx& cx)
{
    cx.timing = p->timing_every > 0 && (p->timing_seq++ % static_cast<unsigned>(p->timing_every)) == 0u;
}
int timing_event(hssfsst_plan* p, const ExecCtx& cx)
{
    if (!cx.timing) return 0;
    hipEvent_t evt = nullptr;
    if (int rc = plan_next_event(p, &evt)) return rc;
    HIP_TRY(hipEventRecord(evt, cx.st));
    return 0;
}
int timing_core_done(hssfsst_plan* p, const ExecCtx& cx)   // (the team path has recorded it already, right behind the team kernel)
{
    return cx.timing_closed ? 0 : timing_event(p, cx);
}
int timing_end(hssfsst_plan* p, const ExecCtx& cx, bool one_kernel)
{
    if (!cx.timing) return 0;
    if (!one_kernel)
        if (int rc = timing_event(p, cx)) return rc;
    p->ev_chunks.push_back(one_kernel ? -1 : 1);
    return 0;
}

// The tables of a ragged exec's list, into the host block h (laid out by t): signal i reads x at starts[i] - xlo, its features
// are `ofps` floats per sample behind those of the signals before it, its statistics partials one per 16-frame group likewise;
// its z-score units (fsst_ragged.hpp) follow from its 2K floats per sample.  t.nunits is set here.
static_assert(sizeof(hssfsst::RaggedChunk) == sizeof(int2) && alignof(hssfsst::RaggedChunk) == alignof(int2), "the kernels read a chunk as int2");
void fill_ragged_tables(unsigned char* h, hssfsst_plan::RaggedTabs& t, const std::vector<hssfsst::RaggedChunk>& chunks, const int64_t* starts,
                        const int64_t* lens, int64_t batch, long long xlo, int ofps, int K)
{
    std::memset(h, 0, t.chunk);
    auto* rs = reinterpret_cast<hssfsst::RaggedSignal*>(h);
    int* unit0 = reinterpret_cast<int*>(h + t.unit);
    long long o = 0, g = 0, u = 0;
    for (int64_t i = 0; i < batch; ++i) {
        rs[i].xoff = starts[i] - xlo; rs[i].ooff = o * ofps; rs[i].poff = g * hssfsst::kPartFloats;
        rs[i].n = static_cast<int>(lens[i]); rs[i].pad = 0;
        unit0[i] = static_cast<int>(u);
        u += (lens[i] * 2 * K + hssfsst::kRaggedUnitFloats - 1) / hssfsst::kRaggedUnitFloats;
        o += lens[i]; g += (lens[i] + 15) / 16;
    }
    unit0[batch] = static_cast<int>(u);
    std::memcpy(h + t.chunk, chunks.data(), chunks.size() * sizeof(int2));
    t.nunits = u;
}

// ... on the device: p->rtab holds them and p->rtabs says where, for the list (lens, starts - xlo); made and uploaded only when
// that is not the list they were last made for
int ragged_tables(hssfsst_plan* p, const int64_t* starts, const int64_t* lens, int64_t batch, long long xlo, hipStream_t st)
{
    auto key = [&](size_t i) -> int64_t { return (i & 1) ? starts[i >> 1] - xlo : lens[i >> 1]; };
    const size_t nkey = static_cast<size_t>(2 * batch);
    if (p->rtab.same(nkey, key)) return 0;
    std::vector<int> ng(static_cast<size_t>(batch));
    for (int64_t i = 0; i < batch; ++i) ng[i] = static_cast<int>((lens[i] + 15) / 16);
    std::vector<hssfsst::RaggedChunk> chunks;
    hssfsst::core128_ragged_chunks(ng.data(), batch, chunks);
    if (chunks.size() >= 0x7fffffffull) return fail(HSSFSST_EINVAL, "exec_ragged: %zu chunks exceed the launch limit; split the list", chunks.size());
    hssfsst_plan::RaggedTabs t;
    t.unit = (static_cast<size_t>(batch) * sizeof(hssfsst::RaggedSignal) + 15) & ~size_t(15);
    t.chunk = (t.unit + static_cast<size_t>(batch + 1) * sizeof(int) + 15) & ~size_t(15);
    t.bytes = t.chunk + chunks.size() * sizeof(int2);
    t.nchunks = static_cast<long long>(chunks.size());
    unsigned char* h = nullptr;
    if (int rc = p->rtab.begin(t.bytes, &h)) return rc;
    fill_ragged_tables(h, t, chunks, starts, lens, batch, xlo, out_floats_per_sample(p), p->K);
    if (int rc = p->rtab.commit(st, nkey, key)) return rc;
    p->rtabs = t;
    return 0;
}

// The plain (two-launch) core kernel of an MFMA plan: the row of kCore128Plain (fsst_launch_shape.hpp) that plan creation
// chose, in the unit that holds the instantiations of its length (512 points: of its length and pairing).  ragged: the
// instantiations of hssfsst_exec_ragged (the same rows, chunk list from the host).
int launch_core128_plain(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, bool ragged)
{
    // (not reached: mfma_facts calls a plan MFMA only when 4 wave regions fit, 2 at 512 points, and the table has a row of that
    //  many waves for every (nt, rq, fast) -- at 128 points with the wide-store epilogue K <= 24 and 16 regions fit;
    //  tests/native/launch_shape_check.cpp sweeps every band)
    if (pl->plain_row < 0) return fail(HSSFSST_EUNSUPPORTED, "LDS request %zu B per wave exceeds the 160 KiB budget", pl->mf.lds_per_wave);
    if (pl->mf.nt == 32)
        return hssfsst::kCore128Plain[pl->plain_row].pair ? launch_core128_plain_n512_pairs(pl, cx, cp, nchunks, ragged)
                                                          : launch_core128_plain_n512(pl, cx, cp, nchunks, ragged);
    return pl->mf.rq == 16 ? launch_core128_plain_n256(pl, cx, cp, nchunks, ragged) : launch_core128_plain_n128(pl, cx, cp, nchunks, ragged);
}


// Is the team kernel wanted for a STACK exec of columns [col0, col0 + ncols) under the preference zpref?  Stated once: exec_impl
// asks before it decides where the features are written, launch_core128 before it launches.  Yes: the canonical band, a range that
// starts on a 16-frame group boundary (tiles are aligned in absolute columns), signals of at most 128 groups, and not switched off
// (HSSFSST_NO_TEAM, a preference for another path).  Paused: it would be, but the team kernel sits execs out after give-ups in a
// row (note_team_outcome) -- unless team_only, the caller's "team kernel or two launches", overrides the pause; the pause counts
// execs of any length.  No side effect (launch_core128 counts a paused exec off where it skips it), and nothing of
// launch_team16's geometry: an exec wanted here may still be declined there.
enum class Team { No, Paused, Yes };
Team team_wanted(const hssfsst_plan* pl, int zpref, int col0, int ncols, bool team_only)
{
    if (!plan_is_canon(pl) || (col0 & 15) != 0 || debug_switches().no_team || zpref == HSSFSST_ZPATH_ONE_CU || zpref == HSSFSST_ZPATH_TWO_LAUNCH)
        return Team::No;
    if (pl->team_pause > 0 && !team_only) return Team::Paused;
    return (ncols + 15) / 16 <= hssfsst::kFusedMaxGroups ? Team::Yes : Team::No;
}

// hout != nullptr (half plans): the team kernel stores the features there as 2-byte elements; every other kernel writes float32
// features to dout for a second, out-of-place z-score sweep (exec_impl) -- the single-launch kernels that normalise in float32 in
// place (one CU per signal, fsst_core128_kernel's fused epilogues) are not taken
int launch_core128(hssfsst_plan* pl, ExecCtx& cx, const float* dx, long long xstride, float* dout, float* partials, int n, int col0,
                   int ncols, int64_t batch, bool try_fused, void* hout = nullptr)
{
    const bool half = hout != nullptr;
    const int ngroups = (ncols + 15) / 16;
    hssfsst::Core128Params cp = core128_params(pl);
    cp.x = dx; cp.xstride = xstride; cp.out = dout; cp.partials = partials;
    cp.n = n; cp.nsig = static_cast<int>(batch); cp.col0 = col0; cp.ncols = ncols;
    cp.reg = hssfsst::core128_regions(ngroups, batch);
    const int64_t nchunks = batch * hssfsst::core128_chunks_per_signal(cp.reg);
    const int rq = pl->mf.rq, nt = pl->mf.nt;
    const bool fast = pl->mf.fast, canon = pl->mf.stripes03;
    // (tiles are aligned in absolute columns: a column range must start on a 16-frame group boundary -- on a 64-frame tile
    //  boundary for the team kernel, whose chunks are whole tiles; other ranges take fsst_core128_kernel)
    const bool canon16 = fast && nt == 16 && rq == 8 && plan_is_canon(pl) && (col0 & 15) == 0;
    if (try_fused && fast && nt == 16 && rq == 8 && pl->mode == HSSFSST_MODE_STACK) {
        // two single-launch z-score kernels.  The team kernel (fsst_team16.hpp: features written once, from registers) is at least as
        // fast as one CU per signal on full batches and 1.3-1.8x faster on small or ragged ones (profiles/r04_batch_sweep.txt): it
        // goes first wherever it applies -- the canonical band, signals of at most 128 groups; one CU per signal (the tile makes a
        // round trip through HBM inside the launch) for the other even bands of <= 24 rows, and as the team kernel's gated fallback
        const bool team_only = debug_switches().team_only || cx.zpref == HSSFSST_ZPATH_TEAM;      // (the switch: A/B and tests)
        int rc = 0;
        // (the host learns of give-ups where it synchronises anyway -- host-output execs, hssfsst_plan_fallbacks, hssfsst_plan_check -- and lets
        //  the team kernel sit out a while when they come in a row: note_team_outcome)
        const Team team = team_wanted(pl, cx.zpref, col0, ncols, team_only);
        if (team == Team::Paused) --pl->team_pause;
        if (team == Team::Yes) {
            rc = launch_team(pl, cx, cp, batch, ngroups, hout);
            if (rc == 1) {
                // the team kernel may give the launch up (its blocks wait for each other; other processes on the GPU can keep
                // them apart: fsst_team16.hpp "Progress"): the same exec is queued behind it, every kernel of it gated on the
                // abort word -- a few microseconds of empty launches when nothing went wrong
                cx.zpath = 2;
                if (int rce = timing_event(pl, cx)) return rce;      // the kernel's own time: the closing event goes in front of the gated launches
                cx.timing_closed = cx.timing;
                if (cx.host_waits) {                     // (exec_impl: a host-output exec synchronises anyway and checks the give-up word then)
                    cx.fused = true;
                    return 0;
                }
                cx.gate = pl->d_arrive.get() + 1; cx.gate_val = cx.team_launch;
                // ONE gated launch where the one-CU-per-signal kernel applies (signals of 16 .. 32 chunks; its batch
                // conditions are about speed only): 4 us behind the team kernel instead of 11 for transform + statistics +
                // z-score launches -- a third of a 50-window exec
                const int rc1 = half ? 0 : launch_canon_fused(pl, cx, cp, batch, ngroups);
                if (rc1 < 0) return rc1;
                if (rc1 == 1) { cx.fused = true; return 0; }
                return launch_canon(pl, cx, cp, nchunks);    // (exec_impl adds the gated statistics + z-score launches)
            }
            if (rc < 0) return rc;
        }
        if (!team_only && !half) {
            rc = canon16 ? launch_canon_fused(pl, cx, cp, batch, ngroups) : launch_fused_n128(pl, cx, cp, batch, ngroups, true, canon);
        }
        if (rc < 0) return rc;
        if (rc == 1) { cx.fused = true; cx.zpath = 1; return 0; }
    }
    if (try_fused && !half && !fast && nt == 16 && pl->mode == HSSFSST_MODE_STACK && cx.zpref != HSSFSST_ZPATH_TEAM) {
        // the general epilogue: one CU per signal, the z-score as tickets of the same launch.  nwin 128, a band the wide-store epilogue does
        // not take (odd K or K > 24): 16 waves per block; nwin 256: as on the two-launch path (what fits the LDS: 8 for the canonical band).
        // (512 points: two launches, on wave pairs: 2.6 ms per 1024 windows against 3.0 for the single launch, whose instantiations are gone)
        int rc = 0;
        if (rq == 8 && core128_lds_bytes(pl, 16, false) <= kMaxLdsBytes) rc = launch_fused_n128(pl, cx, cp, batch, ngroups, false, false);
        else if (rq == 16 && core128_lds_bytes(pl, 8, false) <= kMaxLdsBytes) rc = launch_fused_n256(pl, cx, cp, batch, ngroups, canon);
        if (rc < 0) return rc;
        if (rc == 1) { cx.fused = true; cx.zpath = 1; return 0; }
    }
    if (canon16) return launch_canon(pl, cx, cp, nchunks);
    return launch_core128_plain(pl, cx, cp, nchunks, false);
}

// Plan creation, step 1: which kernels the plan runs, with the MFMA kernels' shape nwin = nt x rq and LDS bytes (mfma_facts).
int choose_family(hssfsst_plan* p)
{
    const int nwin = p->nwin;
    const bool stack = p->mode == HSSFSST_MODE_STACK || p->mode == HSSFSST_MODE_STACK_UNNORM;
    // (force_dft, cross-check: every length on the any-length kernel; force_generic: every radix length on the generic one)
    const bool dft = !(nwin == 32 || nwin == 64 || tables::mfma_length(nwin)) || debug_switches().force_dft;
    p->mf = hssfsst::mfma_facts(dft || debug_switches().force_generic ? 0 : nwin, p->klo, p->K, stack);
    if (dft) {
        p->family = Family::Dft;
        const size_t per_wave = static_cast<size_t>(hssfsst::dft_wave_lds_floats((nwin + 3) / 4, p->K > 0 ? p->K : 1)) * sizeof(float);
        if (per_wave <= static_cast<size_t>(kMaxLdsBytes)) return 0;
        return fail(HSSFSST_EUNSUPPORTED, "plan_create: window length %d with %d kept rows needs %zu B of LDS per wave (> 160 KiB): "
                                          "narrow the band", nwin, p->K, per_wave);
    }
    if (p->mf.rq != 0) p->family = Family::Mfma;         // (else: not an MFMA length, or too few wave regions of this band fit)
    return 0;
}

// Step 2: the constant tables (fsst_tables.hpp) that the plan's kernels read.  Every plan has the generic table (zeros for the
// any-length kernel) and the float64 tables of the rounding-tie path; the canonical-band tables exist for every MFMA plan of nwin 128.
int upload_tables(hssfsst_plan* p, const double* window, const double* dwb)
{
    const int nwin = p->nwin;
    auto up = [](auto& buf, const auto& host) { return buf.upload(host.data(), host.size()); };
    if (int rc = up(p->d_ctab, tables::generic_table(window, dwb, nwin, p->family != Family::Dft))) return rc;
    if (int rc = up(p->d_wtab, tables::tie_table(window, dwb, nwin, &p->r2scale))) return rc;
    if (p->family == Family::Dft) return up(p->d_dtab, tables::dft_table(window, dwb, nwin));
    if (p->family != Family::Mfma) return 0;
    if (int rc = up(p->d_atab, tables::mfma_table(window, dwb, nwin, p->klo, p->K))) return rc;
    if (nwin != 128) return 0;
    int sc = 0;
    if (int rc = up(p->d_atab16, tables::canon_table(window, dwb, &sc))) return rc;
    p->canon_inv_c = static_cast<float>(std::ldexp(1.0, -sc));
    p->canon_r2s = static_cast<float>(static_cast<double>(p->r2scale) * std::ldexp(1.0, sc) * std::ldexp(1.0, sc));
    return 0;
}

// Step 3: what the exec paths would otherwise work out per call
void set_derived_facts(hssfsst_plan* p)
{
    const bool stack = p->mode == HSSFSST_MODE_STACK || p->mode == HSSFSST_MODE_STACK_UNNORM;
    if (p->family == Family::Mfma) p->plain_row = hssfsst::core128_plain_row(p->mf, debug_switches().no_pair);
    if (debug_switches().no_canon || !p->d_atab16.get() || !stack) return;      // (no_canon: A/B and cross-check tests)
    for (int i = 0; i < static_cast<int>(sizeof(kCanonBands) / sizeof(kCanonBands[0])); ++i)
        if (p->klo == kCanonBands[i][0] && p->K == kCanonBands[i][1]) p->canon_idx = i;
}

}  // namespace

extern "C" {

int hssfsst_version(void) { return HSSFSST_VERSION; }
const char* hssfsst_last_error(void) { return g_err; }

int hssfsst_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int hssfsst_dtwin(const double* window, int nwin, double fs, double* dwindow)
{
    if (!window || !dwindow || nwin < 1 || !(fs > 0.0)) return fail(HSSFSST_EINVAL, "hssfsst_dtwin: bad argument");
    if (int rc = tables::dwindow(window, nwin, fs / (2.0 * M_PI), dwindow)) return fail(rc, "hssfsst_dtwin: singular spline system");
    return 0;
}

int hssfsst_band(int nwin, double fs, double f_lo, double f_hi, int* klo, int* K)
{
    if (nwin < 1 || !(fs > 0.0) || !klo || !K) return fail(HSSFSST_EINVAL, "hssfsst_band: bad argument");
    tables::band_rows(nwin, fs, f_lo, f_hi, klo, K);
    return 0;
}

double hssfsst_update_mean(double m, double x, int64_t k) { return m + (x - m) / static_cast<double>(k); }

double hssfsst_update_variance(double x, double m, double var, int64_t k)
{
    const double delta = x - m;
    return var + delta * (x - (m + delta / static_cast<double>(k)));
}

int hssfsst_plan_create(hssfsst_plan** out, int device, int nwin, const double* window, double fs,
                        int has_band, double f_lo, double f_hi, int mode)
{
    return hssfsst_plan_create_ex(out, device, nwin, window, fs, has_band, f_lo, f_hi, mode, HSSFSST_DTYPE_F32);
}

int hssfsst_plan_create_ex(hssfsst_plan** out, int device, int nwin, const double* window, double fs,
                           int has_band, double f_lo, double f_hi, int mode, int out_dtype)
{
    if (!out) return fail(HSSFSST_EINVAL, "plan_create: out is NULL");
    *out = nullptr;
    if (!window || nwin < 1 || !(fs > 0.0) || mode < 0 || mode > HSSFSST_MODE_STACK_UNNORM)
        return fail(HSSFSST_EINVAL, "plan_create: bad argument (nwin=%d fs=%g mode=%d)", nwin, fs, mode);
    // (before any device is touched) half-precision output is the z-scored STACK features' only: RAW stays complex64, ABS and the
    // streaming STACK_UNNORM stay float32; float64 output does not exist
    if (out_dtype != HSSFSST_DTYPE_F32 && out_dtype != HSSFSST_DTYPE_F16 && out_dtype != HSSFSST_DTYPE_BF16)
        return fail(HSSFSST_EINVAL, "plan_create: output dtype %d is not HSSFSST_DTYPE_F32 / F16 / BF16", out_dtype);
    if (out_dtype != HSSFSST_DTYPE_F32 && mode != HSSFSST_MODE_STACK)
        return fail(HSSFSST_EINVAL, "plan_create: half-precision output (dtype %d) is for HSSFSST_MODE_STACK only, not mode %d", out_dtype, mode);
    if (nwin > 65535) return fail(HSSFSST_EUNSUPPORTED, "plan_create: window length %d exceeds 65535", nwin);
    if (int rc = check_device("plan_create", device)) return rc;
    DEVICE_SCOPE(device);
    std::unique_ptr<hssfsst_plan> p(new (std::nothrow) hssfsst_plan());    // (every error path frees what was made, under device_guard_)
    if (!p) return fail(HSSFSST_ENOMEM, "plan_create: host allocation failed");
    p->device = device; p->nwin = nwin; p->R = nwin / 32; p->nf = nwin / 2 + 1; p->mode = mode;
    p->out_dtype = out_dtype; p->out_es = out_dtype == HSSFSST_DTYPE_F32 ? sizeof(float) : 2;
    if (has_band) tables::band_rows(nwin, fs, f_lo, f_hi, &p->klo, &p->K);
    else { p->klo = 0; p->K = p->nf; }
    std::vector<double> dwb(nwin);                        // derivative window in bin units
    if (int rc = tables::dwindow(window, nwin, static_cast<double>(nwin) / (2.0 * M_PI), dwb.data())) return fail(rc, "plan_create: singular spline system");
    if (int rc = choose_family(p.get())) return rc;
    if (int rc = upload_tables(p.get(), window, dwb.data())) return rc;
    set_derived_facts(p.get());
    *out = p.release();
    return 0;
}

int hssfsst_plan_destroy(hssfsst_plan* p)
{
    if (!p) return 0;
    DeviceGuard device_guard_(p->device);
    if (p->h_status) (void)hipHostFree(const_cast<unsigned*>(p->h_status));
    if (p->h_fallback) (void)hipHostFree(const_cast<unsigned*>(p->h_fallback));
    for (auto& ev : p->ev) if (ev) (void)hipEventDestroy(ev);
    delete p;                                            // (the buffers free themselves)
    return 0;
}

int hssfsst_plan_info(const hssfsst_plan* p, int* nwin, int* nf, int* klo, int* K,
                      int* ofps, int* mode, int* device)
{
    if (!p) return fail(HSSFSST_EINVAL, "plan_info: plan is NULL");
    if (nwin) *nwin = p->nwin;
    if (nf) *nf = p->nf;
    if (klo) *klo = p->klo;
    if (K) *K = p->K;
    if (ofps) *ofps = out_floats_per_sample(p);
    if (mode) *mode = p->mode;
    if (device) *device = p->device;
    return 0;
}


int hssfsst_plan_out_dtype(const hssfsst_plan* p, int* out_dtype)
{
    if (!p || !out_dtype) return fail(HSSFSST_EINVAL, "plan_out_dtype: bad argument");
    *out_dtype = p->out_dtype;
    return 0;
}

int hssfsst_plan_last_exec_fused(const hssfsst_plan* p) { return (p && p->last_fused) ? p->last_zpath : 0; }

int hssfsst_plan_last_kernel(const hssfsst_plan* p, char* buf, int len)
{
    if (!p || !buf || len < 1) return fail(HSSFSST_EINVAL, "plan_last_kernel: bad argument");
    snprintf(buf, static_cast<size_t>(len), "%s", p->last_kernel);
    return 0;
}

int hssfsst_plan_fallbacks(hssfsst_plan* p)
{
    if (!p) return fail(HSSFSST_EINVAL, "plan_fallbacks: plan is NULL");
    if (p->h_fallback) {
        const unsigned now = *p->h_fallback;
        if (now != p->seen_fallback) { p->seen_fallback = now; ++p->fallbacks; note_team_outcome(p, true); }
    }
    return p->fallbacks;
}

int hssfsst_plan_set_zpath(hssfsst_plan* p, int zpath)
{
    if (!p || zpath < HSSFSST_ZPATH_AUTO || zpath > HSSFSST_ZPATH_TEAM) return fail(HSSFSST_EINVAL, "plan_set_zpath: bad argument");
    p->zpath_pref = zpath;
    return 0;
}

int hssfsst_plan_check(hssfsst_plan* p)
{
    if (!p) return fail(HSSFSST_EINVAL, "plan_check: plan is NULL");
    if (!p->d_status) return 0;
    DEVICE_SCOPE(p->device);
    HIP_TRY(hipDeviceSynchronize());                     // every exec of this plan has finished
    const unsigned code = *p->h_status;
    if (code != 0) {
        *p->h_status = 0u;
        return fail(HSSFSST_EHIP, "fused z-score: a wait inside the kernel gave up (code %u); results of that exec are invalid", code);
    }
    return 0;
}

int hssfsst_plan_set_timing(hssfsst_plan* p, int enable)
{
    if (!p) return fail(HSSFSST_EINVAL, "plan_set_timing: plan is NULL");
    p->timing_every = enable > 0 ? enable : 0;
    p->timing_seq = 0;
    p->ev_used = 0;
    p->ev_chunks.clear();
    return 0;
}

int hssfsst_plan_timing(hssfsst_plan* p, float ms_sum[2], int* nexec)
{
    if (!p || !ms_sum || !nexec) return fail(HSSFSST_EINVAL, "plan_timing: bad argument");
    ms_sum[0] = ms_sum[1] = 0.0f;
    *nexec = static_cast<int>(p->ev_chunks.size());
    if (p->ev_used == 0) return 0;
    DEVICE_SCOPE(p->device);
    HIP_TRY(hipEventSynchronize(p->ev[p->ev_used - 1]));
    size_t i = 0;
    for (int nc : p->ev_chunks) {
        if (nc < 0) {                                    // fused exec: (before, after) only
            float a = 0.0f;
            HIP_TRY(hipEventElapsedTime(&a, p->ev[i], p->ev[i + 1]));
            ms_sum[0] += a;
            i += 2;
            continue;
        }
        float core = 0.0f, total = 0.0f;
        for (int c = 0; c < nc; ++c) {
            float a = 0.0f;
            HIP_TRY(hipEventElapsedTime(&a, p->ev[i + 2 * c], p->ev[i + 2 * c + 1]));
            core += a;
        }
        HIP_TRY(hipEventElapsedTime(&total, p->ev[i], p->ev[i + 2 * nc]));
        ms_sum[0] += core;
        ms_sum[1] += total - core;
        i += 2 * static_cast<size_t>(nc) + 1;
    }
    return 0;
}

int hssfsst_exec(hssfsst_plan* p, const float* x, int64_t batch, int n, int x_on_device,
                 float* out, int out_on_device, void* stream)
{
    return hssfsst_exec_cols(p, x, batch, n, 0, n, x_on_device, out, out_on_device, stream);
}

int hssfsst_exec_cols(hssfsst_plan* p, const float* x, int64_t batch, int n, int col0, int ncols, int x_on_device,
                      float* out, int out_on_device, void* stream)
{
    return hssfsst_exec_frames(p, x, batch, n, static_cast<int64_t>(n), col0, ncols, x_on_device, out, out_on_device, stream);
}

// ---- what every exec entry point shares

// A wait inside an EARLIER exec's kernel gave up (pinned status word, no synchronisation): that exec's features are invalid and
// the caller of a device-output exec has not been told yet -- refuse, once, until the plan is checked.
static int take_pending_status(hssfsst_plan* p, const char* what)
{
    if (!p->h_status || *p->h_status == 0u) return 0;
    const unsigned code = *p->h_status;
    *p->h_status = 0u;
    return fail(HSSFSST_EHIP, "%s: a wait inside a previous exec's z-score kernel gave up (code %u); the results of that exec are invalid",
                what, code);
}

// nx floats of a host input into the plan's device staging buffer; *dx then points there
static int stage_input(hssfsst_plan* p, const float* x, size_t nx, const float** dx, hipStream_t st)
{
    if (int rc = p->d_xstage.grow(nx)) return rc;
    HIP_TRY(hipMemcpyAsync(p->d_xstage.get(), x, nx * sizeof(float), hipMemcpyHostToDevice, st));
    *dx = p->d_xstage.get();
    return 0;
}

// The device side of an exec's `no` output elements: *dout (staged when the output is a host one), *kout where the kernels write
// float32 features (half plans: the plan's float32 scratch, from which the z-score sweep writes the 2-byte elements to *dout), and
// for STACK the statistics partials (`pieces` of them) and statistics of `nsig` signals.
static int exec_buffers(hssfsst_plan* p, size_t no, bool stage_out, size_t pieces, int64_t nsig, float** dout, float** kout)
{
    int rc;
    if (stage_out) {
        if ((rc = p->d_ostage.grow((no * p->out_es + sizeof(float) - 1) / sizeof(float))) != 0) return rc;
        *dout = p->d_ostage.get();
    }
    *kout = *dout;
    if (p->out_es != sizeof(float)) {
        if ((rc = p->d_f32.grow(no)) != 0) return rc;
        *kout = p->d_f32.get();
    }
    if (p->mode == HSSFSST_MODE_STACK) {
        if ((rc = p->d_partials.grow(pieces * hssfsst::kPartFloats)) != 0) return rc;
        if ((rc = p->d_stats.grow(static_cast<size_t>(nsig) * 4)) != 0) return rc;
    }
    return 0;
}

// A device `out` of 4-byte elements that is not 16-byte aligned (a view one float into a tensor, say): every float32 kernel stores
// float4s relative to `out` and the in-place z-score sweeps load them, so such an exec runs on the plan's own output staging, as a
// host-output exec does, and a device copy on the exec's stream puts the features where the caller wants them (exec_finish).  The
// 2-byte outputs of a half plan look at their own alignment in the kernels (fsst_half.hpp) and are not staged.
static bool out_needs_staging(const hssfsst_plan* p, const void* out, int out_on_device)
{
    return out_on_device && p->out_es == sizeof(float) && (reinterpret_cast<uintptr_t>(out) & 15) != 0;
}

// The end of an exec: a host output is copied back, the stream synchronised and the plan checked; a device output that was staged
// (out_needs_staging) is copied on the stream, nothing waits; a host input is only waited for (the caller may reuse it)
static int exec_finish(hssfsst_plan* p, void* out, const void* dout, size_t bytes, int x_on_device, int out_on_device, hipStream_t st)
{
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return hssfsst_plan_check(p);
    }
    if (dout != out) HIP_TRY(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToDevice, st));
    if (!x_on_device) HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// The end of an exec whose kernels stored the features to pinned host memory (exec_impl: tiny_out): waits for them.  *redo: the
// exec's team launch gave itself up and the caller computes the exec again without the team kernel.
static int finish_pinned_exec(hssfsst_plan* p, const ExecCtx& cx, bool* redo)
{
    // The team launch of this exec, if it was asked to (want_done_word): its last wave stores the launch's identity to h_fallback[2] behind a
    // system-scope release of every wave's stores -- the features are in pinned host memory by then.  Waiting for that word instead of
    // the stream's completion signal spares the end-of-kernel cache flush and the signal's way to the host: 6 us of a 35 us call
    // (tools/sync_latency.hip).  A launch that gave itself up never stores it: the give-up word ends the wait, as does a bound.
    bool seen = false;
    const unsigned fl = cx.flagged_launch;
    if (fl != 0u && p->h_fallback) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned it = 0;; ++it) {
            if (p->h_fallback[2] == fl) { seen = true; break; }
            if (p->h_fallback[0] == fl) break;                                   // given up: the usual way below
            if ((it & 255u) == 255u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(2000)) break;
            __builtin_ia32_pause();
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!seen) {
        HIP_TRY(hipStreamSynchronize(cx.st));
        if (fl != 0u) {                               // (the blocks of a given-up launch did not all count themselves in: start the count over)
            HIP_TRY(hipMemsetAsync(p->d_arrive.get() + 2, 0, sizeof(unsigned), cx.st));
            p->done_total = 0;
        }
    }
    if (cx.host_waits && cx.team_launch != 0u) {
        // no gated kernels were queued behind this exec's team launch: if that launch gave itself up (pinned word, written with
        // system scope before the kernel ended), the exec is computed now by the kernels that would have been queued
        const bool gave = p->h_fallback && p->h_fallback[0] == cx.team_launch;      // (launch identities count up; 0 is never one)
        note_team_outcome(p, gave);
        if (gave) { *redo = true; return 0; }
    }
    if (seen) {                                       // (the status word is pinned host memory too: written before the wave that wrote it counted itself in)
        if (p->h_status && *p->h_status != 0u) {
            const unsigned code = *p->h_status;
            *p->h_status = 0u;
            return fail(HSSFSST_EHIP, "fused z-score: a wait inside the kernel gave up (code %u); results of that exec are invalid", code);
        }
    } else if (p->d_status) return hssfsst_plan_check(p);
    return 0;
}

// The one exec: `batch` signals of n samples, signal b at x + b * x_stride, or -- d_starts != nullptr (device array) --
// at x + d_starts[b] inside a buffer of x_len samples.  A frame list is first gathered into a dense [batch][n] staging
// buffer (fsst_gather_frames_kernel: 8 kB read + 8 kB written per frame, against 360 kB of output) and then takes the
// same kernels as a dense batch: the transform kernels sit at the 128-VGPR limit of their occupancy and a second
// addressing mode in them cost spilled registers.
// (pin_d != nullptr: `out` is a pinned buffer of the plan's pool and pin_d its device alias -- hssfsst_exec_pinned: the kernels store the
//  features there and nothing is copied; returns 1 when this exec is not one the kernels can write straight to host memory)
// (redo: the second pass of a host-output exec whose team launch gave up -- no team kernel, no direct-to-host output: it runs as
//  under HSSFSST_ZPATH_ONE_CU)
static int exec_impl(hssfsst_plan* p, const float* x, int64_t batch, int n, int64_t x_stride, const long long* d_starts,
                     size_t x_len, int col0, int ncols, int x_on_device, float* out, int out_on_device, void* stream, float* pin_d = nullptr,
                     bool redo = false)
{
    if (!p || !x || !out || batch < 0 || n < 1 || col0 < 0 || ncols < 1 || col0 > n - ncols || x_stride < 1)
        return fail(HSSFSST_EINVAL, "exec: bad argument (batch=%lld n=%d stride=%lld col0=%d ncols=%d)",
                    static_cast<long long>(batch), n, static_cast<long long>(x_stride), col0, ncols);
    if (batch == 0 || p->K == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DEVICE_SCOPE(p->device);
    int rc;
    if ((rc = take_pending_status(p, "exec")) != 0) return rc;
    ExecCtx cx;
    cx.st = st;
    cx.zpref = redo ? HSSFSST_ZPATH_ONE_CU : p->zpath_pref;
    const int ofps = out_floats_per_sample(p);
    // statistics partials per signal: one per 16-frame group (MFMA and any-length kernels) / per 64-frame tile (generic kernel)
    const int fpp = p->family == Family::Generic ? kTile : 16;
    const int nblk = (ncols + fpp - 1) / fpp;
    const long long nblocks = static_cast<long long>(batch) * nblk;
    if (nblocks > 0x7fffffffLL) return fail(HSSFSST_EINVAL, "exec: batch*tiles = %lld exceeds the grid limit; split the batch", nblocks);
    if (static_cast<long long>(n) * 2 * p->nf >= 0x7fffffffLL) return fail(HSSFSST_EINVAL, "exec: signal too long (n = %d)", n);
    // input extent: `batch` signals of n samples whose starts are x_stride apart (they may overlap)
    const size_t nx = d_starts ? x_len : static_cast<size_t>(batch > 0 ? batch - 1 : 0) * static_cast<size_t>(x_stride) + n;
    const size_t no = static_cast<size_t>(batch) * ncols * ofps;               // output elements
    const size_t es = p->out_es, no_f = (no * es + sizeof(float) - 1) / sizeof(float);   // their bytes per element; floats that hold them
    const bool half = es != sizeof(float);

    const float* dx = x;
    float* dout = out;
    // Small host-to-host execs -- the reference's dataset loop calls the transform once per 2000-sample frame with CPU tensors
    // (/root/reference/hss/datasets/heart_sounds.py:166-168,199-201) -- do not go through hipMemcpyAsync from / to pageable memory
    // (two staged copies by the runtime, ~0.03 ms of a 0.068 ms call): the samples are copied into a pinned, device-mapped buffer
    // that the kernels read in place, and where the output is written exactly once (every mode but a STACK whose z-score is a
    // second pass over the features) the kernels store it into a pinned buffer too -- the mechanism of hssfsst_stream_step.
    const bool tiny_in = !x_on_device && nx <= (static_cast<size_t>(1) << 16);
    // (STACK: only where the team kernel will take the exec -- its features are written once; a z-score that is a second pass would
    //  read and rewrite them in place over PCIe: signals of more than 128 groups keep the device staging buffer + one copy;
    //  the HSSFSST_TEAM_ONLY switch overrides a pause at the launch only: a paused exec under it keeps the staging buffer too)
    const bool tiny_out = tiny_in && !out_on_device && no_f <= (static_cast<size_t>(1) << 21) &&
                          (p->mode != HSSFSST_MODE_STACK || team_wanted(p, cx.zpref, col0, ncols, cx.zpref == HSSFSST_ZPATH_TEAM) == Team::Yes);
    auto pin = [&](PinnedBuf<float>& b, size_t need) -> int {
        if (b.h && b.cap < need) HIP_TRY(hipStreamSynchronize(st));     // (earlier work on the stream may still use the old block)
        return b.grow(need, sizeof(float));
    };
    if (tiny_in) {
        if ((rc = pin(p->xpin, nx)) != 0) return rc;
        std::memcpy(p->xpin.h, x, nx * sizeof(float));
        dx = p->xpin.d;
    } else if (!x_on_device) {
        if ((rc = stage_input(p, x, nx, &dx, st)) != 0) return rc;
    }
    if (d_starts) {
        const size_t nd = static_cast<size_t>(batch) * n;
        if ((rc = p->d_frames.grow(nd)) != 0) return rc;
        if ((rc = launch_gather_frames(dx, d_starts, p->d_frames.get(), batch, n, st)) != 0) return rc;
        dx = p->d_frames.get();
        x_stride = n;
    }
    if (pin_d && !tiny_out) return 1;                    // (not an exec whose features are written once: the caller takes the copying call)
    if (tiny_out) {
        if (pin_d) dout = pin_d;
        else {
            if ((rc = pin(p->opin, no_f)) != 0) return rc;
            dout = p->opin.d;
        }
        cx.host_waits = cx.zpref != HSSFSST_ZPATH_ONE_CU && !d_starts;
    }
    float* kout = nullptr;
    if ((rc = exec_buffers(p, no, (!tiny_out && !out_on_device) || out_needs_staging(p, out, out_on_device), static_cast<size_t>(nblocks), batch,
                           &dout, &kout)) != 0) return rc;

    timing_begin(p, cx);
    // STACK: core (FP32-issue-bound) then the z-score sweep (HBM-bound, in place).  Measured and rejected (git history, DESIGN.md
    // section 4.3): a k-chunk two-stream pipeline that overlaps the sweep of one chunk with the core of the next -- the saturating
    // sweep back-pressures the core's own stores (core 0.25 -> 0.32-0.41 ms per 1024 windows); fusing the z-score into the
    // core launch -- "last ticket normalises the signal" (write-through stores + one agent acquire: 0.62 ms; with an L2
    // write-back release per block: 0.99 ms) and "blocks of a signal wait for each other, then normalise their own tiles"
    // (bounded spin + fix-up kernel: 0.58 ms) -- both bit-identical to, and slower than, the two-pass 0.37 ms per 1024 windows.
    // a host-output exec of one team launch: the launch's last wave says "done" in pinned host memory and this call waits for that word
    // instead of synchronising the stream (below)
    cx.want_done_word = cx.host_waits && !cx.timing;
    hssfsst::CoreParams cp;
    cp.x = dx; cp.out = kout; cp.partials = p->d_partials.get(); cp.ctab = p->d_ctab.get();
    cp.n = n; cp.klo = p->klo; cp.K = p->K; cp.mode = p->mode; cp.nblk = nblk; cp.col0 = col0; cp.ncols = ncols; cp.xstride = x_stride;
    cp.wtab = p->d_wtab.get(); cp.twtab = p->d_wtab.get() + 2 * p->nwin; cp.r2scale = p->r2scale;
    if ((rc = timing_event(p, cx)) != 0) return rc;
    const bool no_fused = debug_switches().no_fused;      // A/B and bit-equality tests
    if (p->family == Family::Dft) {
        rc = launch_dft(p, cx, dx, kout, batch, n, x_stride, col0, ncols);
    } else if (p->family == Family::Mfma) {
        rc = launch_core128(p, cx, dx, x_stride, kout, cp.partials, n, col0, ncols, batch, !no_fused && cx.zpref != HSSFSST_ZPATH_TWO_LAUNCH,
                            half ? dout : nullptr);
    } else {
        rc = launch_core_radix(p, cx, cp, nblocks);
    }
    if (rc != 0) return rc;
    if ((rc = timing_core_done(p, cx)) != 0) return rc;
    if (p->mode == HSSFSST_MODE_STACK && !cx.fused && (rc = launch_zscore(p, cx, kout, dout, batch, nblk, fpp, ncols)) != 0) return rc;
    exec_report(p, cx);
    if ((rc = timing_end(p, cx, p->last_fused != 0)) != 0) return rc;
    if (tiny_out) {
        bool gave_up = false;
        if ((rc = finish_pinned_exec(p, cx, &gave_up)) != 0) return rc;
        if (gave_up)                                      // (copies into `out`: a pool buffer is host memory too)
            return exec_impl(p, x, batch, n, x_stride, d_starts, x_len, col0, ncols, x_on_device, out, out_on_device, stream, nullptr, true);
        if (!pin_d) std::memcpy(out, p->opin.h, no * es);
    } else return exec_finish(p, out, dout, no * es, x_on_device, out_on_device, st);
    return 0;
}

int hssfsst_exec_frames(hssfsst_plan* p, const float* x, int64_t batch, int n, int64_t x_stride, int col0, int ncols,
                        int x_on_device, float* out, int out_on_device, void* stream)
{
    return exec_impl(p, x, batch, n, x_stride, nullptr, 0, col0, ncols, x_on_device, out, out_on_device, stream);
}

// The dataset loop's call without the copy into the caller's tensor: the kernels store the features into a pinned, device-mapped buffer
// of the plan's pool and the caller is LENT that buffer (hssfsst.h).  hssfsst_pinned_release may run on another host thread at the same
// time (whichever drops the caller's last reference): the pool is a fixed array, and pin_mu guards the choice of a buffer, its
// replacement and every `used` flag; the exec itself runs on a reserved buffer with the lock released.
int hssfsst_exec_pinned(hssfsst_plan* p, const float* x, int n, float** out)
{
    if (!p || !x || !out || n < 1) return fail(HSSFSST_EINVAL, "exec_pinned: bad argument");
    *out = nullptr;
    if (p->K == 0) return 1;
    DEVICE_SCOPE(p->device);
    const size_t no = static_cast<size_t>(n) * out_floats_per_sample(p);      // elements (2 bytes each in a half plan); caps count elements
    hssfsst_plan::PoolBuf* b = nullptr;
    {
        std::lock_guard<std::mutex> lock(p->pin_mu);
        for (auto& c : p->pin_pool) if (!c.used && c.buf.cap >= no) { b = &c; break; }
        if (!b) {
            for (auto& c : p->pin_pool) if (!c.used) { b = &c; break; }   // (a free one that is too small, or none yet, is replaced)
            if (!b) return 1;                                              // every buffer is still in the caller's hands: take the copying call
            if (int rc = b->buf.grow(no, p->out_es)) return rc;
        }
        b->used = true;
    }
    const int rc = exec_impl(p, x, 1, n, static_cast<int64_t>(n), nullptr, 0, 0, n, 0, b->buf.h, 0, nullptr, b->buf.d);
    if (rc != 0) {
        std::lock_guard<std::mutex> lock(p->pin_mu);
        b->used = false;
        return rc;
    }
    *out = b->buf.h;
    return 0;
}

int hssfsst_pinned_release(hssfsst_plan* p, float* buf)
{
    if (!p || !buf) return fail(HSSFSST_EINVAL, "pinned_release: bad argument");
    std::lock_guard<std::mutex> lock(p->pin_mu);
    for (auto& c : p->pin_pool) if (c.buf.h == buf) { c.used = false; return 0; }
    return fail(HSSFSST_EINVAL, "pinned_release: not a buffer of this plan's pool");
}

int hssfsst_exec_list(hssfsst_plan* p, const float* x, int64_t x_len, const int64_t* starts, int starts_on_device,
                      int64_t batch, int n, int x_on_device, float* out, int out_on_device, void* stream)
{
    if (!p || !x || !starts || !out || batch < 0 || n < 1 || x_len < n)
        return fail(HSSFSST_EINVAL, "exec_list: bad argument (batch=%lld n=%d x_len=%lld)", static_cast<long long>(batch), n,
                    static_cast<long long>(x_len));
    if (batch == 0 || p->K == 0) return 0;
    static_assert(sizeof(long long) == sizeof(int64_t), "frame starts are 64-bit");
    const long long* d_starts = reinterpret_cast<const long long*>(starts);
    if (!starts_on_device) {
        for (int64_t b = 0; b < batch; ++b)
            if (starts[b] < 0 || starts[b] > x_len - n)
                return fail(HSSFSST_EINVAL, "exec_list: frame %lld starts at %lld, outside [0, %lld]", static_cast<long long>(b),
                            static_cast<long long>(starts[b]), static_cast<long long>(x_len - n));
        DEVICE_SCOPE(p->device);
        int rc;
        if ((rc = p->d_starts.grow(static_cast<size_t>(batch))) != 0) return rc;
        HIP_TRY(hipMemcpyAsync(p->d_starts.get(), starts, static_cast<size_t>(batch) * sizeof(long long), hipMemcpyHostToDevice,
                               static_cast<hipStream_t>(stream)));
        d_starts = p->d_starts.get();
    }
    return exec_impl(p, x, batch, n, 1, d_starts, static_cast<size_t>(x_len), 0, n, x_on_device, out, out_on_device, stream);
}

// Signals of different lengths in one exec (hssfsst.h).  Plans of the MFMA kernel (nwin 128 / 256 / 512): ONE core launch for the
// whole list (fsst_core128_kernel<.., RAGGED>: a host-made chunk list, each signal cut as it would be alone) and, for STACK, one
// statistics and one z-score launch (fsst_ragged.hpp).  Other plans: one exec per signal on the caller's stream.
int hssfsst_exec_ragged(hssfsst_plan* p, const float* x, int64_t x_len, const int64_t* starts, const int64_t* lens, int64_t batch,
                        int x_on_device, float* out, int out_on_device, void* stream)
{
    // argument errors first, and all of them before the plan or a device is looked at
    if (batch < 0 || batch > 0x7fffffffLL) return fail(HSSFSST_EINVAL, "exec_ragged: batch = %lld", static_cast<long long>(batch));
    if (batch > 0 && (!x || !starts || !lens || !out))
        return fail(HSSFSST_EINVAL, "exec_ragged: NULL %s", !x ? "x" : !starts ? "starts" : !lens ? "lens" : "out");
    for (int64_t i = 0; i < batch; ++i) {
        if (lens[i] < 1) return fail(HSSFSST_EINVAL, "exec_ragged: signal %lld has length %lld", static_cast<long long>(i), static_cast<long long>(lens[i]));
        if (starts[i] < 0 || x_len < lens[i] || starts[i] > x_len - lens[i])
            return fail(HSSFSST_EINVAL, "exec_ragged: signal %lld ([%lld, %lld + %lld)) lies outside x[0, %lld)", static_cast<long long>(i),
                        static_cast<long long>(starts[i]), static_cast<long long>(starts[i]), static_cast<long long>(lens[i]),
                        static_cast<long long>(x_len));
    }
    if (!p) return fail(HSSFSST_EINVAL, "exec_ragged: plan is NULL");
    for (int64_t i = 0; i < batch; ++i)
        if (lens[i] >= (0x7fffffffLL + 2 * p->nf - 1) / (2 * p->nf))          // (n * 2 nf >= 2^31 - 1, as exec_impl)
            return fail(HSSFSST_EINVAL, "exec_ragged: signal %lld too long (n = %lld)", static_cast<long long>(i), static_cast<long long>(lens[i]));
    if (batch == 0 || p->K == 0) return 0;
    const int ofps = out_floats_per_sample(p);
    if (p->family != Family::Mfma) {
        // the generic and any-length kernels: one exec per signal (the kernels of hssfsst_exec, on the caller's stream)
        long long off = 0;
        for (int64_t i = 0; i < batch; ++i) {
            const int n = static_cast<int>(lens[i]);
            float* o = reinterpret_cast<float*>(reinterpret_cast<char*>(out) + static_cast<size_t>(off) * ofps * p->out_es);
            if (int rc = exec_impl(p, x + starts[i], 1, n, n, nullptr, 0, 0, n, x_on_device, o, out_on_device, stream)) return rc;
            off += n;
        }
        return 0;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    DEVICE_SCOPE(p->device);
    int rc;
    if ((rc = take_pending_status(p, "exec")) != 0) return rc;
    // host input: the extent the list covers, uploaded once
    long long xlo = starts[0], xhi = starts[0] + lens[0];
    for (int64_t i = 1; i < batch; ++i) {
        xlo = std::min<long long>(xlo, starts[i]);
        xhi = std::max<long long>(xhi, starts[i] + lens[i]);
    }
    if (x_on_device) xlo = 0;
    long long cols = 0, groups = 0;
    for (int64_t i = 0; i < batch; ++i) { cols += lens[i]; groups += (lens[i] + 15) / 16; }
    const size_t no = static_cast<size_t>(cols) * ofps;                       // output elements

    if ((rc = ragged_tables(p, starts, lens, batch, xlo, st)) != 0) return rc;
    const hssfsst_plan::RaggedTabs& t = p->rtabs;
    const auto* d_rsig = reinterpret_cast<const hssfsst::RaggedSignal*>(p->rtab.get());
    const int* d_unit0 = reinterpret_cast<const int*>(p->rtab.get() + t.unit);
    const int2* d_chunks = reinterpret_cast<const int2*>(p->rtab.get() + t.chunk);

    const float* dx = x;
    float* dout = out;
    float* kout = nullptr;
    if (!x_on_device && (rc = stage_input(p, x + xlo, static_cast<size_t>(xhi - xlo), &dx, st)) != 0) return rc;
    if ((rc = exec_buffers(p, no, !out_on_device || out_needs_staging(p, out, out_on_device), static_cast<size_t>(groups), batch, &dout, &kout)) != 0) return rc;

    ExecCtx cx;
    cx.st = st;
    timing_begin(p, cx);
    if ((rc = timing_event(p, cx)) != 0) return rc;
    hssfsst::Core128Params cp = core128_params(p);
    cp.x = dx; cp.out = kout; cp.partials = p->d_partials.get();
    cp.n = 1; cp.nsig = static_cast<int>(std::min<int64_t>(batch, 0x7fffffff)); cp.col0 = 0; cp.ncols = 1; cp.xstride = 0;
    cp.rsig = d_rsig; cp.rchunk = d_chunks; cp.rnchunks = static_cast<int>(t.nchunks);
    // (the canonical-class band in STACK modes takes the canonical kernel's arithmetic, as every single exec of it does; the
    //  general kernels give other -- equally accurate -- bits there)
    if (p->mf.fast && p->mf.nt == 16 && p->mf.rq == 8 && plan_is_canon(p))
        rc = launch_canon_ragged(p, cx, cp, t.nchunks);
    else
        rc = launch_core128_plain(p, cx, cp, t.nchunks, true);
    if (rc != 0) return rc;
    if ((rc = timing_core_done(p, cx)) != 0) return rc;
    if (p->mode == HSSFSST_MODE_STACK && (rc = launch_zscore_ragged(p, cx, kout, dout, batch, d_rsig, d_unit0, t.nunits)) != 0) return rc;
    exec_report(p, cx);
    if ((rc = timing_end(p, cx, false)) != 0) return rc;
    return exec_finish(p, out, dout, no * p->out_es, x_on_device, out_on_device, st);
}

int hssfsst_moments_merge(hssfsst_plan* p, const float* feats, int64_t batch, int n, double* state, void* stream)
{
    if (!p || !feats || !state || batch < 0 || n < 1) return fail(HSSFSST_EINVAL, "moments_merge: bad argument");
    if (batch == 0 || p->K == 0) return 0;
    if (batch > 0x7fffffffLL || static_cast<long long>(n) * 2 * p->K >= 0x7fffffffLL) return fail(HSSFSST_EINVAL, "moments_merge: too large");
    DEVICE_SCOPE(p->device);
    return launch_moments_merge(p, feats, batch, n, state, static_cast<hipStream_t>(stream));
}

int hssfsst_normalize_running(hssfsst_plan* p, float* feats, int64_t batch, int n, const double* state, void* stream)
{
    if (!p || !feats || !state || batch < 0 || n < 1) return fail(HSSFSST_EINVAL, "normalize_running: bad argument");
    if (batch == 0 || p->K == 0) return 0;
    if (batch > 0x7fffffffLL || static_cast<long long>(n) * 2 * p->K >= 0x7fffffffLL) return fail(HSSFSST_EINVAL, "normalize_running: too large");
    DEVICE_SCOPE(p->device);
    int rc;
    if ((rc = p->d_stats.grow(static_cast<size_t>(batch) * 4)) != 0) return rc;
    return launch_normalize_running(p, feats, batch, n, state, reinterpret_cast<float4*>(p->d_stats.get()), static_cast<hipStream_t>(stream));
}

int hssfsst_stream_step(hssfsst_plan* p, float* tape, int64_t tape_len, int64_t pos, const float* x_new, int64_t x_stride,
                        int x_on_device, int channels, int chunk, float* out, double* state, float* out_host,
                        void* stream)
{
    if (!p || !tape || !x_new || !out || channels < 1 || chunk < 1 || x_stride < chunk)
        return fail(HSSFSST_EINVAL, "stream_step: bad argument");
    if (p->mode != HSSFSST_MODE_STACK_UNNORM) return fail(HSSFSST_EINVAL, "stream_step: the plan must be STACK_UNNORM");
    const int64_t hist = p->nwin - 1;
    if (pos < hist || pos + chunk > tape_len)
        return fail(HSSFSST_EINVAL, "stream_step: pos %lld outside [nwin - 1, tape_len - chunk] (tape_len %lld, chunk %d)",
                    static_cast<long long>(pos), static_cast<long long>(tape_len), chunk);
    if (hist + chunk > 0x7fffffffLL || static_cast<long long>(chunk) * 2 * p->K >= 0x7fffffffLL)
        return fail(HSSFSST_EINVAL, "stream_step: chunk too large");
    if (p->K == 0) return 0;
    if (int rc = take_pending_status(p, "stream_step")) {     // an earlier step's wait between blocks gave up (see hssfsst_plan_check)
        // (a step that gave up may have left its channels' arrival counters short of a full round: later steps would never
        //  normalise -- start them from zero again)
        if (p->d_stream_arrive.cap > 0) {
            DEVICE_SCOPE(p->device);
            (void)hipMemsetAsync(p->d_stream_arrive.get(), 0, p->d_stream_arrive.cap * sizeof(unsigned), static_cast<hipStream_t>(stream));
        }
        return rc;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    DEVICE_SCOPE(p->device);
    // one launch for the whole step where the transform is the wide-store MFMA kernel in one-group chunks (nwin 256 / 512, an even
    // band of <= 24 rows: BASELINE config 5); host samples are copied into the tape first and the kernel reads them there
    const bool one_launch = p->family == Family::Mfma && p->mf.rq == 16 && p->mf.fast && !debug_switches().no_stream_fuse &&
                            (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                            static_cast<long long>(channels) * ((chunk + 15) / 16) < 0x7fffffffLL;
    int launched = 0;
    float* mirror = nullptr;
    if (one_launch) {
        // host samples in PINNED memory are read by the kernel where they lie (32 KiB per step over the link: no copy operation
        // in front of the launch); pageable memory is copied into the tape first and the kernel reads it there
        const float* xd = x_on_device ? x_new : nullptr;
        if (!x_on_device) {
            // (asked at every step: a cached answer would outlive the caller's buffer)
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, const_cast<float*>(x_new), 0) == hipSuccess && dp) xd = static_cast<const float*>(dp);
            else (void)hipGetLastError();
            if (!xd)
                HIP_TRY(hipMemcpy2DAsync(tape + pos, static_cast<size_t>(tape_len) * sizeof(float), x_new, static_cast<size_t>(x_stride) * sizeof(float),
                                         static_cast<size_t>(chunk) * sizeof(float), static_cast<size_t>(channels), hipMemcpyHostToDevice, st));
        }
        // a pinned host destination is written by the kernel itself (the last block of a channel stores the normalised chunk to
        // both places): no copy operation behind the launch either
        if (out_host && (reinterpret_cast<uintptr_t>(out_host) & 15) == 0) {
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, out_host, 0) == hipSuccess && dp) mirror = static_cast<float*>(dp);
            else (void)hipGetLastError();
        }
        // (wave pairs: the step's latency is one group's; regions of a block = 2)
        float* tape_at = tape + (pos - hist);
        const bool pair = !debug_switches().no_pair;
        if (p->mf.nt != 32) launched = launch_stream_n256(p, tape_at, tape_len, xd, x_stride, channels, chunk, out, state, mirror, st, pair);
        else launched = pair ? launch_stream_n512_pairs(p, tape_at, tape_len, xd, x_stride, channels, chunk, out, state, mirror, st)
                             : launch_stream_n512(p, tape_at, tape_len, xd, x_stride, channels, chunk, out, state, mirror, st);
        if (launched < 0) return launched;
        if (launched == 0 && xd)                         // (not this kernel's shape after all: the chunk goes into the tape by a copy)
            HIP_TRY(hipMemcpy2DAsync(tape + pos, static_cast<size_t>(tape_len) * sizeof(float), x_new, static_cast<size_t>(x_stride) * sizeof(float),
                                     static_cast<size_t>(chunk) * sizeof(float), static_cast<size_t>(channels),
                                     x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    } else {
        HIP_TRY(hipMemcpy2DAsync(tape + pos, static_cast<size_t>(tape_len) * sizeof(float), x_new, static_cast<size_t>(x_stride) * sizeof(float),
                                 static_cast<size_t>(chunk) * sizeof(float), static_cast<size_t>(channels),
                                 x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    if (launched == 0) {
        // frame j of the chunk = samples [pos - hist + j, pos - hist + j + nwin): column nwin/2 + j of the zero-padded
        // transform of the last hist + chunk samples
        int rc = hssfsst_exec_frames(p, tape + (pos - hist), channels, static_cast<int>(hist + chunk), tape_len, p->nwin / 2, chunk, 1, out, 1, stream);
        if (rc != 0) return rc;
        if (state) {
            if ((rc = launch_stream_finish(p, out, state, channels, chunk, st)) != 0) return rc;
        }
    }
    if (out_host && launched == 1 && mirror) {
        HIP_TRY(hipStreamSynchronize(st));
    } else if (out_host) {
        HIP_TRY(hipMemcpyAsync(out_host, out, static_cast<size_t>(channels) * chunk * 2 * p->K * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

}  // extern "C"
