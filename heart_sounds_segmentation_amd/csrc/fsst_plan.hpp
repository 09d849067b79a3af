// fsst_plan.hpp -- what the FSST units of libhssfsst.so share on the host: the plan (the C ABI's hssfsst_plan), one exec's launch
// state, the process's A-B switches, the small helpers every launcher calls, and the launchers' entry points.  No kernel here: the
// kernels are instantiated in the launcher units -- fsst_team.hip (team and canonical-band kernels), fsst_core128_n128.hip /
// _n256.hip / _n512.hip / _n512_pairs.hip (the MFMA core, by transform length) and fsst_generic.hip (generic, any-length and the
// small kernels) -- and hssfsst.hip, which creates plans and routes execs, reaches them through the declarations at the end.
// Everything but the C struct lives in hssfsst::host (hidden visibility, host_common.hpp).
#pragma once
#include "host_common.hpp"

#include <algorithm>
#include <array>
#include <cstdlib>
#include <mutex>
#include <type_traits>
#include <utility>

#include "fsst_device.hpp"                                 // CoreParams, Core128Params, RaggedSignal (and fsst_launch_shape.hpp)

namespace hssfsst {
namespace host __attribute__((visibility("hidden"))) {

// A-B and test switches, read ONCE per process (first use) from the environment, one variable per key: HSSFSST_<KEY in capitals>
// is on when set to an empty string, a non-zero number or a word that starts with y or t (HSSFSST_FORCE_GENERIC: a value that
// starts with 1).  Defaults are the measured best; no switch changes a result (every path gives the same bits, which is what most
// of them exist to show).  Nothing else in the library reads the environment, but for the segmenter's one switch, read the same
// way in segmenter.hip (seg_ragged_pre_mib).  (An inline function: its one static is the one reading for all units.)
struct DebugSwitches {
    bool no_fused = false;        // z-score always as a second kernel
    bool no_canon = false;        // the canonical band on the general kernels (fsst_mfma128.hpp)
    bool no_team = false;         // never the team kernel
    bool team_only = false;       // the team kernel or two launches, never one CU per signal
    bool team_force_fallback = false;   // every team launch finds itself given up (tests of the gated fallback)
    bool force_dft = false;       // every window length on the any-length kernel
    bool force_generic = false;   // every radix length on the generic VALU kernel
    bool no_stream_fuse = false;  // a streaming step as copy + transform + merge-and-normalise launches
    bool no_pair = false;         // nwin 256 / 512: one wave per wave region (no wave pairs)
};
inline const DebugSwitches& debug_switches()
{
    static const DebugSwitches sw = [] {
        auto on = [](const char* name) {
            const char* v = std::getenv(name);
            return v != nullptr && (v[0] == '\0' || std::atoi(v) != 0 || v[0] == 'y' || v[0] == 't');
        };
        DebugSwitches d;
        d.no_fused = on("HSSFSST_NO_FUSED");
        d.no_canon = on("HSSFSST_NO_CANON");
        d.no_team = on("HSSFSST_NO_TEAM");
        d.team_only = on("HSSFSST_TEAM_ONLY");
        d.team_force_fallback = on("HSSFSST_TEAM_FORCE_FALLBACK");
        d.force_dft = on("HSSFSST_FORCE_DFT");
        const char* fg = std::getenv("HSSFSST_FORCE_GENERIC");
        d.force_generic = fg != nullptr && fg[0] == '1';
        d.no_stream_fuse = on("HSSFSST_NO_STREAM_FUSE");
        d.no_pair = on("HSSFSST_NO_PAIR");
        return d;
    }();
    return sw;
}

constexpr int kTile = 64;
using hssfsst::kFpw128;

constexpr size_t kPinPoolMax = 64;                       // hssfsst_exec_pinned: buffers lent at a time (hssfsst.h)

// The kernels a plan runs (choose_family): generic VALU (nwin 32 / 64, and the fallback of 128 / 256 / 512), any-length, MFMA
enum class Family { Generic, Dft, Mfma };

}  // namespace host
}  // namespace hssfsst

struct hssfsst_plan {
    int device = -1;
    int nwin = 0, R = 0, nf = 0, klo = 0, K = 0, mode = 0;
    int out_dtype = HSSFSST_DTYPE_F32;                       // HSSFSST_DTYPE_F32, or F16 / BF16 (STACK only): element type of every exec's `out`
    size_t out_es = sizeof(float);                           // ... its size in bytes
    hssfsst::host::DevBuf<float> d_f32;                                     // half plans: float32 features of the paths whose z-score is a second sweep
    hssfsst::host::DevBuf<float> d_ctab;         // generic kernel: class-folded scalar tables
    hssfsst::host::DevBuf<float> d_dtab;         // any-length kernel (fsst_dft.hpp): A operand [source block][k-step][64 lanes]
    hssfsst::host::Family family = hssfsst::host::Family::Generic;
    float r2scale = 0.0f;         // 4 nwin max |(w + i dw') / 2|^2: error-bound scale of the rounding-tie path
    hssfsst::host::DevBuf<double> d_wtab;        // float64 {w, dw' in bin units}[nwin], then {cos, sin}(2 pi m / nwin)[nwin]: rounding-tie path
    hssfsst::host::DevBuf<float> d_atab;         // nwin == 128 / 256 / 512: MFMA A-operand constants [pass][taps][64 lanes][k-step]
    hssfsst::host::DevBuf<float> d_atab16;       // canonical-band kernels (fsst_canon128.hpp): f16 split A operand [16 taps][64 lanes][8 halves]
    float canon_inv_c = 0.0f;     // ... 1 / (power-of-two scale of those constants)
    float canon_r2s = 0.0f;       // ... r2scale x scale^2
    int canon_slots = 0;          // resident blocks of fsst_canon_kernel<.., false> (0 = not queried yet)
    // what follows from the fields above, stated once at creation (choose_family, set_derived_facts):
    hssfsst::MfmaFacts mf;        // nt, rq, fast, stripes03 and the LDS bytes (fsst_launch_shape.hpp; rq = 0 unless Family::Mfma)
    int plain_row = -1;           // MFMA plans: the row of kCore128Plain that the two-launch path runs, dense and ragged (-1: none fits)
    int canon_idx = -1;           // index of the band in kCanonBands when the canonical-band kernels apply, else -1
    hssfsst::host::DevBuf<float> d_partials;                                // kPartFloats per statistics piece
    unsigned* d_status = nullptr;                            // fused z-score: status word (0 = ok) as the device sees it ...
    volatile unsigned* h_status = nullptr;                   // ... and the same word in pinned host memory: read without a sync
    hssfsst::host::DevBuf<unsigned long long> d_mail;                       // team kernel: mailboxes [teams][slots][32 blocks][8] (8-byte words)
    unsigned team_seq = 0;                                   // launch sequence number (upper half of the mailbox tags)
    hssfsst::host::DevBuf<unsigned> d_arrive; unsigned arrive_total = 0;    // team kernel: [0] arrival counter (and its value after the launches so far), [1] abort word, [2] blocks done
    unsigned done_total = 0;                                 // ... [2]'s value after the flagged launches so far
    unsigned team_launch = 0;                                // identity of the last team launch (never 0)
    volatile unsigned* h_fallback = nullptr; unsigned* d_fallback = nullptr;   // pinned host word: identity of the last team launch that gave up
    unsigned seen_fallback = 0; int fallbacks = 0;           // ... as last seen by the host, and how many distinct ones
    int giveups_in_a_row = 0, team_pause = 0;                // a GPU shared with many processes: after kTeamGiveUps give-ups in a row the team kernel sits out
                                                             // the plan's next kTeamPause execs that would take it (each give-up costs its 0.5 ms bound first)
    int team16_cus = 0;                                      // CUs usable by the team kernel (fsst_team16.hpp; 0 = not queried yet, -1 = none)
    char last_kernel[112] = "";                              // the transform kernel of the last exec: instantiation, waves per block, grid (hssfsst_plan_last_kernel)
    int last_fused = 0;                                      // the last exec ran a single-launch z-score kernel
    int zpath_pref = 0;                                      // HSSFSST_ZPATH_*: preference among the z-score paths
    int last_zpath = 0;                                      // ... which one: 1 = one CU per signal, 2 = team kernel
    int core128_slots = 0;                    // resident blocks of the core kernel on this device (0 = not queried yet)
    int ragged_slots = 0;                     // the same for its ragged instantiation
    int stream_slots = 0;                     // the same for the streaming-step kernel
    hssfsst::host::DevBuf<unsigned> d_stream_arrive;         // streaming step: blocks delivered per channel
    hssfsst::host::DevBuf<double> d_stream_pieces;           // and the groups' float64 sums [channels][groups][4]
    int fused_slots = 0;                      // CUs usable by the fused kernel (0 = not queried yet, -1 = none)
    hssfsst::host::DevBuf<float> d_stats;                                   // 4 per signal
    hssfsst::host::DevBuf<float> d_xstage, d_ostage;                        // a host input / output, staged
    // small host-to-host execs (the unchanged dataset loop: one 2000-sample frame per call): pinned, device-mapped staging that the
    // kernels read and write in place
    hssfsst::host::PinnedBuf<float> xpin, opin;
    struct PoolBuf { hssfsst::host::PinnedBuf<float> buf; bool used = false; };
    std::array<PoolBuf, hssfsst::host::kPinPoolMax> pin_pool;              // hssfsst_exec_pinned: pinned, device-mapped result buffers lent to the caller
    std::mutex pin_mu;                                       // ... guards `used` and the buffers' replacement (hssfsst_pinned_release may
                                                             // come from another host thread)
    hssfsst::host::DevBuf<long long> d_starts;                              // frame-list staging (hssfsst_exec_list with host starts)
    hssfsst::host::DevBuf<float> d_frames;                                  // frames gathered from a list, dense [batch][n]
    // hssfsst_exec_ragged: the list's tables -- RaggedSignal[batch], z-score unit starts int[batch + 1], chunk list int2[] -- in one
    // block, kept while the next list has the same lengths and offsets; where they lie in it and how many they are
    hssfsst::host::UploadedTable rtab{"exec_ragged"};
    struct RaggedTabs {
        size_t unit = 0, chunk = 0, bytes = 0;               // byte offsets of the unit starts and of the chunk list, and the block's size
        long long nchunks = 0, nunits = 0;
    } rtabs;                                                 // (of rtab's key: written behind its commit)
    int timing_every = 0;         // hssfsst_plan_set_timing(n): every n-th exec is timed (0: off)
    unsigned timing_seq = 0;
    std::vector<hipEvent_t> ev;   // per timed exec: (before, after) per core launch + one closing event
    size_t ev_used = 0;           // events used since timing was enabled
    std::vector<int> ev_chunks;   // core launches of each timed exec
};

namespace hssfsst {
namespace host __attribute__((visibility("hidden"))) {

using hssfsst::kMaxLdsBytes;

// Resident blocks of `kern` (threads per block, dynamic LDS) on the plan's device, asked once and kept in `cache` (0 = not asked
// yet; launchers that share a cache share the first answer).  whole_cus: one block per CU -- the CU count, or -1 when the kernel
// does not fit; otherwise blocks per CU x CUs, each factor at least 1.
template <class Kern>
int resident_blocks(const hssfsst_plan* pl, int& cache, Kern kern, int threads, size_t lds, bool whole_cus)
{
    if (cache != 0) return 0;
    int per_cu = 0, cus = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kern), threads, lds));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, pl->device));
    cache = whole_cus ? ((per_cu >= 1 && cus >= 1) ? cus : -1) : std::max(per_cu, 1) * std::max(cus, 1);
    return 0;
}

// One exec's launch state: made on the stack by exec_impl / hssfsst_exec_ragged and handed to the launchers.  Nothing of it
// outlives the exec; what the C ABI reports afterwards goes to the plan in one place (exec_report).
struct ExecCtx {
    hipStream_t st = nullptr;
    // in
    int zpref = HSSFSST_ZPATH_AUTO;           // the z-score path preference this exec runs under (the plan's; ONE_CU for a redo)
    bool host_waits = false;                  // this exec synchronises before it returns: no gated launches behind a team launch, the host
                                              // looks at the pinned give-up word afterwards and redoes the exec itself
    bool want_done_word = false;              // the team launch is asked to say in pinned host memory (h_fallback[2]) when its last wave is done
    // set by launch_core128 behind a team launch: the kernels that follow it in the same exec are its gated fallback
    const unsigned* gate = nullptr; unsigned gate_val = 0;
    // out
    unsigned team_launch = 0;                 // identity of this exec's team launch (at most one), or 0
    unsigned flagged_launch = 0;              // ... when it was asked for its done word, else 0
    bool fused = false;                       // the z-score was part of the launches so far (no statistics + z-score launches to add)
    int zpath = 0;                            // ... by which path: 1 = one CU per signal, 2 = team kernel
    char kernel[sizeof(hssfsst_plan::last_kernel)] = "";     // the transform kernel: instantiation, waves per block, grid
    bool timing = false;                      // this exec records kernel events
    bool timing_closed = false;               // ... and has recorded its closing kernel event already (team path: right behind the team kernel)
};

// which kernel instantiation the exec that is being queued runs (hssfsst_plan_last_kernel: the dispatch made observable)
inline void name_kernel(char (&name)[sizeof(hssfsst_plan::last_kernel)], int waves, long long grid, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    const int k = vsnprintf(name, sizeof(name), fmt, ap);
    va_end(ap);
    if (k > 0 && static_cast<size_t>(k) < sizeof(name))
        snprintf(name + k, sizeof(name) - static_cast<size_t>(k), " [%d waves/block, grid %lld]", waves, grid);
}

inline size_t core128_lds_bytes(const hssfsst_plan* pl, int wpb, bool pair) { return hssfsst::core128_lds_bytes(pl->mf, wpb, pair); }

// the Core128Params every launch of an MFMA plan starts from: the plan-constant fields
inline hssfsst::Core128Params core128_params(const hssfsst_plan* pl)
{
    hssfsst::Core128Params cp{};
    cp.atab = pl->d_atab.get(); cp.wtab = pl->d_wtab.get(); cp.twtab = pl->d_wtab.get() + 2 * pl->nwin; cp.r2scale = pl->r2scale;
    cp.klo = pl->klo; cp.K = pl->K; cp.mode = pl->mode;
    return cp;
}

// The status word of the in-kernel waits lives in pinned, device-mapped host memory: a kernel that gave up writes it
// with a system-scope store, and the host looks at it without synchronising (at the start of the next exec, in
// hssfsst_plan_check after a synchronisation, at plan destruction).
inline int ensure_status(hssfsst_plan* pl)
{
    if (pl->d_status) return 0;
    void* h = nullptr;
    HIP_TRY(hipHostMalloc(&h, sizeof(unsigned), hipHostMallocMapped));
    *static_cast<volatile unsigned*>(h) = 0u;
    void* d = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&d, h, 0));
    pl->h_status = static_cast<volatile unsigned*>(h);
    pl->d_status = static_cast<unsigned*>(d);
    return 0;
}

// Canonical-class kernels (fsst_canon128.hpp): nwin = 128, STACK / STACK_UNNORM, the kept band a compile-time constant.  Two bands
// are instantiated: rows 4..25 = [25, 200] Hz at fs = 1000 (/root/reference/main.py:153-158, the reference's own configuration) and
// rows 2..25 = [25, 400] Hz at fs = 2000 -- the pass band of the Springer / Schmidt heart-sound segmenters on recordings at
// PhysioNet 2016's native rate (/root/reference/hss/datasets/heart_sounds.py:36-113 loads them un-resampled).  Every other band keeps
// fsst_core128_kernel.  (A third band is one line here: the template takes any even band of <= 24 rows inside rows 0..31.)
constexpr int kCanonBands[][2] = {{4, 22}, {2, 24}};

inline bool plan_is_canon(const hssfsst_plan* pl) { return pl->canon_idx >= 0; }
// f(KLO, KC) with the plan's band as integral constants
template <class F>
int canon_dispatch(const hssfsst_plan* pl, F&& f)
{
    switch (pl->canon_idx) {
    case 0: return f(std::integral_constant<int, kCanonBands[0][0]>{}, std::integral_constant<int, kCanonBands[0][1]>{});
    case 1: return f(std::integral_constant<int, kCanonBands[1][0]>{}, std::integral_constant<int, kCanonBands[1][1]>{});
    default: return fail(HSSFSST_EINVAL, "canon_dispatch: not a canonical-class plan");
    }
}

// ---- The launchers' entry points: each kernel family is instantiated in the unit named, and nowhere else -----------------------
// The conventions of the launchers behind them: 0 = launched (or < 0, an error); the single-launch z-score kernels and the
// streaming step return 1 when they launched and 0 when this exec should take another path.

// fsst_team.hip: the team kernel (the plan's band and output type), and the canonical-band kernel as two launches, ragged, and at
// one CU per signal
int launch_team(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t batch, int ngroups, void* hout);
int launch_canon(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks);
int launch_canon_ragged(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks);
int launch_canon_fused(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t batch, int ngroups);

// fsst_core128_n128.hip, _n256.hip, _n512.hip, _n512_pairs.hip: the MFMA core.  Each unit expands its own rows of kCore128Plain
// (fsst_launch_shape.hpp; the 512-point rows on wave pairs are a unit of their own) for the plan's plain_row, dense and ragged,
// and holds the fused and streaming instantiations of its length.  fast / stripes03: the plan's facts (MfmaFacts).
int launch_core128_plain_n128(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, bool ragged);
int launch_core128_plain_n256(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, bool ragged);
int launch_core128_plain_n512(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, bool ragged);
int launch_core128_plain_n512_pairs(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, bool ragged);
int launch_fused_n128(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t batch, int ngroups, bool fast, bool stripes03);
int launch_fused_n256(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t batch, int ngroups, bool stripes03);
int launch_stream_n256(hssfsst_plan* pl, float* tape_at, long long tape_len, const float* x_new_dev, long long x_stride, int channels,
                       int chunk, float* out, double* state, float* mirror, hipStream_t st, bool pair);
int launch_stream_n512(hssfsst_plan* pl, float* tape_at, long long tape_len, const float* x_new_dev, long long x_stride, int channels,
                       int chunk, float* out, double* state, float* mirror, hipStream_t st);
int launch_stream_n512_pairs(hssfsst_plan* pl, float* tape_at, long long tape_len, const float* x_new_dev, long long x_stride, int channels,
                             int chunk, float* out, double* state, float* mirror, hipStream_t st);

// fsst_generic.hip: the generic VALU kernel (the plan's radix), the any-length kernel, the z-score as its own launches (dense and
// ragged), the frame gather, the running moments and a streaming step's tail
int launch_core_radix(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::CoreParams& cp, long long nblocks);
int launch_dft(hssfsst_plan* p, ExecCtx& cx, const float* dx, float* kout, int64_t batch, int n, int64_t x_stride, int col0, int ncols);
int launch_zscore(hssfsst_plan* p, const ExecCtx& cx, const float* feats, void* out, int64_t batch, int nblk, int fpp, int ncols);
int launch_zscore_ragged(hssfsst_plan* p, const ExecCtx& cx, const float* feats, void* out, int64_t batch,
                         const hssfsst::RaggedSignal* rsig, const int* unit0, long long nunits);
int launch_gather_frames(const float* dx, const long long* d_starts, float* frames, int64_t batch, int n, hipStream_t st);
int launch_moments_merge(const hssfsst_plan* p, const float* feats, int64_t batch, int n, double* state, hipStream_t st);
int launch_normalize_running(const hssfsst_plan* p, float* feats, int64_t batch, int n, const double* state, float4* stats, hipStream_t st);
int launch_stream_finish(const hssfsst_plan* p, float* out, double* state, int channels, int chunk, hipStream_t st);

}  // namespace host
}  // namespace hssfsst
