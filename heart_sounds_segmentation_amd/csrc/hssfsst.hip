// hssfsst.hip -- host side of libhssfsst.so: the C ABI declared in include/hssfsst.h.
// Plan creation does, once and in fp64, everything of the reference's `ssq.fsst(x, fs, window)`
// (call site /root/reference/hss/transforms/synchrosqueeze.py:48) that depends only on
// (fs, window); exec launches the gfx950 kernels of fsst_kernels.hpp.
// There is no CPU compute path here by design (the CPU restatement is oracle/, test-only).
#include "../../include/hssfsst.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <mutex>
#include <dlfcn.h>
#include <cstdlib>
#include <array>
#include <atomic>
#include <memory>
#include <new>
#include <thread>
#include <vector>
#include <type_traits>
#include <utility>

#include "fsst_kernels.hpp"
#include "fsst_mfma128.hpp"
#include "fsst_canon128.hpp"
#include "fsst_team16.hpp"
#include "fsst_dft.hpp"
#include "fsst_gather.hpp"
#include "fsst_ragged.hpp"
#include "fsst_half.hpp"
#include "fourier_resample.hpp"
#include "fourier_resample_layout.hpp"
#include "fourier_resample_gpu.hpp"
#include "fourier_resample_ragged.hpp"
#include "segmenter_lstm.hpp"
#include "segmenter_layout.hpp"
#include "segmenter_train.hpp"
#include "decode_durations_layout.hpp"
#include "decode_layout.hpp"
#include "sequence_args.hpp"
#include "segmenter_decode.hpp"
#include "segmenter_decode_durations.hpp"
#include "posterior_layout.hpp"
#include "segmenter_posteriors.hpp"
#include "segmenter_duration_posteriors.hpp"
#include "segmenter_duration_counts.hpp"
#include "score_layout.hpp"
#include "segmenter_score.hpp"
#include "stitch_layout.hpp"
#include "segmenter_stitch.hpp"
#include "fsst_tables.hpp"

namespace tables = hssfsst::tables;
namespace rslayout = hssfsst::rslayout;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(HSSFSST_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                                   \
    } while (0)

// behind a kernel launch of the entry point `entry`
int launch_check(const char* entry, const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(HSSFSST_EHIP, "%s: launch of %s failed: %s", entry, what, hipGetErrorString(e));
    return 0;
}

// A-B and test switches, read ONCE per process (first use) from the environment, one variable per key: HSSFSST_<KEY in capitals>
// is on when set to an empty string, a non-zero number or a word that starts with y or t (HSSFSST_FORCE_GENERIC: a value that
// starts with 1).  Defaults are the measured best; no switch changes a result (every path gives the same bits, which is what most
// of them exist to show).  Nothing else in the library reads the environment.
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
    int seg_ragged_pre_mib = 0;   // ragged segmenter: bound of the projection scratch in MiB (a number; 0 or unset: the dense call's 128)
};
const DebugSwitches& debug_switches()
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
        const char* pm = std::getenv("HSSFSST_SEG_RAGGED_PRE_MIB");
        d.seg_ragged_pre_mib = pm != nullptr ? std::min(std::max(std::atoi(pm), 0), 1 << 16) : 0;
        return d;
    }();
    return sw;
}

// Makes `device` current for the scope and restores the caller's device on every exit path (a process
// that drives several GPUs must not find its current HIP device changed by a library call).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = (err == hipSuccess);
        }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define DEVICE_SCOPE(dev)                                                                      \
    DeviceGuard device_guard_(dev);                                                            \
    if (device_guard_.err != hipSuccess)                                                       \
        return fail(HSSFSST_EHIP, "selecting device %d failed: %s", (dev), hipGetErrorString(device_guard_.err))

// the plan creates' device argument: a HIP device must exist (this library has no CPU path) and `device` must be one
int check_device(const char* what, int device)
{
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(HSSFSST_ENODEVICE, "%s: no HIP device (%s); this library has no CPU path", what,
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    }
    if (device < 0 || device >= ndev) return fail(HSSFSST_EINVAL, "%s: device %d out of range [0,%d)", what, device, ndev);
    return 0;
}

constexpr int kTile = 64;
using hssfsst::kFpw128;

// A plan's device buffer: capacity in elements of T; grow() frees the old block and allocates a larger one (contents are not
// kept), upload() makes a fresh block holding a host table.  Freed with its owner.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    T* get() const { return p; }
    int grow(size_t need)
    {
        if (need <= cap) return 0;
        if (p) { HIP_TRY(hipFree(p)); p = nullptr; cap = 0; }
        void* v = nullptr;
        const hipError_t e = hipMalloc(&v, need * sizeof(T));
        if (e != hipSuccess) return fail(HSSFSST_ENOMEM, "hipMalloc(%zu B): %s", need * sizeof(T), hipGetErrorString(e));
        p = static_cast<T*>(v);
        cap = need;
        return 0;
    }
    int upload(const T* host, size_t n)                 // (into an empty or smaller buffer: grow() makes it fresh)
    {
        if (int rc = grow(n)) return rc;
        HIP_TRY(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
};

// A plan's pinned host buffer.  Mapped (the staging of small execs, the lent pool): hipHostMallocMapped with its device alias d,
// a power of two from 4096 elements; otherwise default flags, no alias, 1.5x what is needed.  Capacity in elements of es bytes.
template <class T>
struct PinnedBuf {
    T* h = nullptr;
    T* d = nullptr;
    size_t cap = 0;
    bool mapped = true;
    PinnedBuf() = default;
    explicit PinnedBuf(bool mapped_) : mapped(mapped_) {}
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() { if (h) (void)hipHostFree(h); }
    int grow(size_t need, size_t es)
    {
        if (need <= cap) return 0;
        if (h) { HIP_TRY(hipHostFree(h)); h = nullptr; d = nullptr; cap = 0; }
        size_t c = need + need / 2;
        if (mapped) for (c = size_t(1) << 12; c < need; c *= 2) {}
        void* hp = nullptr;
        HIP_TRY(hipHostMalloc(&hp, c * es, mapped ? hipHostMallocMapped : hipHostMallocDefault));
        void* dp = nullptr;
        const hipError_t e = mapped ? hipHostGetDevicePointer(&dp, hp, 0) : hipSuccess;
        if (e != hipSuccess) {
            (void)hipHostFree(hp);
            return fail(HSSFSST_EHIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
        }
        h = static_cast<T*>(hp); d = static_cast<T*>(dp); cap = c;
        return 0;
    }
};

// A table that is made on the host for a list and read on the device: a ring of kRing pinned (not mapped) host blocks, a device
// block, per host block the event of its last upload (a host block is not rewritten before that copy is done) and the key of the
// list the device block holds.
//   if (!t.same(n, key)) { t.begin(bytes, &h); ...fill h...; t.commit(stream, n, key); }     key(i): the i-th of n 64-bit words
// begin() drops the key first and commit() stores it last, behind the queued copy: whatever fails in between, the next call with
// the same list makes the table again.  A user without a key (n = 0) uploads at every call.  `what`: the entry point, for errors.
// Why a ring: with ONE host block a call whose list differs from the previous call's had to wait on the host for the previous
// upload, i.e. for everything queued on the stream before it -- a caller that walks groups of a long list (HipSegmenter.ragged
// with max_steps) behind other work stalled at its second group.  With the ring only the upload kRing list changes back is waited
// for.  The device block is one: the uploads and the kernels that read it are ordered by the plan's one stream.
struct UploadedTable {
    static constexpr int kRing = 4;
    const char* what;
    PinnedBuf<unsigned char> h[kRing];
    DevBuf<unsigned char> d;
    hipEvent_t ev[kRing] = {};
    int cur = 0;
    std::vector<int64_t> key;
    size_t bytes = 0;
    explicit UploadedTable(const char* what_) : what(what_) { for (auto& b : h) b.mapped = false; }
    UploadedTable(const UploadedTable&) = delete;
    UploadedTable& operator=(const UploadedTable&) = delete;
    ~UploadedTable() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    const unsigned char* get() const { return d.get(); }
    template <class Key>
    bool same(size_t n, Key&& at) const
    {
        if (key.empty() || key.size() != n) return false;
        for (size_t i = 0; i < n; ++i) if (key[i] != at(i)) return false;
        return true;
    }
    int begin(size_t nbytes, unsigned char** host)
    {
        key.clear();
        cur = (cur + 1) % kRing;
        if (ev[cur]) HIP_TRY(hipEventSynchronize(ev[cur]));  // (the upload kRing changes back may still read this host block)
        if (int rc = h[cur].grow(nbytes, 1)) return rc;
        if (int rc = d.grow(nbytes)) return rc;
        bytes = nbytes;
        *host = h[cur].h;
        return 0;
    }
    template <class Key>
    int commit(hipStream_t st, size_t n, Key&& at)
    {
        if (!ev[cur]) HIP_TRY(hipEventCreateWithFlags(&ev[cur], hipEventDisableTiming));
        HIP_TRY(hipMemcpyAsync(d.get(), h[cur].h, bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(ev[cur], st));
        try {
            key.resize(n);
        } catch (const std::bad_alloc&) {
            return fail(HSSFSST_ENOMEM, "%s: out of host memory", what);
        }
        for (size_t i = 0; i < n; ++i) key[i] = at(i);
        return 0;
    }
    int commit(hipStream_t st) { return commit(st, 0, [](size_t) { return int64_t(0); }); }
};

constexpr size_t kPinPoolMax = 64;                       // hssfsst_exec_pinned: buffers lent at a time (hssfsst.h)

// The kernels a plan runs (choose_family): generic VALU (nwin 32 / 64, and the fallback of 128 / 256 / 512), any-length, MFMA
enum class Family { Generic, Dft, Mfma };

}  // namespace

struct hssfsst_plan {
    int device = -1;
    int nwin = 0, R = 0, nf = 0, klo = 0, K = 0, mode = 0;
    int out_dtype = HSSFSST_DTYPE_F32;                       // HSSFSST_DTYPE_F32, or F16 / BF16 (STACK only): element type of every exec's `out`
    size_t out_es = sizeof(float);                           // ... its size in bytes
    DevBuf<float> d_f32;                                     // half plans: float32 features of the paths whose z-score is a second sweep
    DevBuf<float> d_ctab;         // generic kernel: class-folded scalar tables
    DevBuf<float> d_dtab;         // any-length kernel (fsst_dft.hpp): A operand [source block][k-step][64 lanes]
    Family family = Family::Generic;
    float r2scale = 0.0f;         // 4 nwin max |(w + i dw') / 2|^2: error-bound scale of the rounding-tie path
    DevBuf<double> d_wtab;        // float64 {w, dw' in bin units}[nwin], then {cos, sin}(2 pi m / nwin)[nwin]: rounding-tie path
    DevBuf<float> d_atab;         // nwin == 128 / 256 / 512: MFMA A-operand constants [pass][taps][64 lanes][k-step]
    DevBuf<float> d_atab16;       // canonical-band kernels (fsst_canon128.hpp): f16 split A operand [16 taps][64 lanes][8 halves]
    float canon_inv_c = 0.0f;     // ... 1 / (power-of-two scale of those constants)
    float canon_r2s = 0.0f;       // ... r2scale x scale^2
    int canon_slots = 0;          // resident blocks of fsst_canon_kernel<.., false> (0 = not queried yet)
    // what follows from the fields above, stated once at creation (choose_family, set_derived_facts):
    hssfsst::MfmaFacts mf;        // nt, rq, fast, stripes03 and the LDS bytes (fsst_launch_shape.hpp; rq = 0 unless Family::Mfma)
    int plain_row = -1;           // MFMA plans: the row of kCore128Plain that the two-launch path runs, dense and ragged (-1: none fits)
    int canon_idx = -1;           // index of the band in kCanonBands when the canonical-band kernels apply, else -1
    DevBuf<float> d_partials;                                // kPartFloats per statistics piece
    unsigned* d_status = nullptr;                            // fused z-score: status word (0 = ok) as the device sees it ...
    volatile unsigned* h_status = nullptr;                   // ... and the same word in pinned host memory: read without a sync
    DevBuf<unsigned long long> d_mail;                       // team kernel: mailboxes [teams][slots][32 blocks][8] (8-byte words)
    unsigned team_seq = 0;                                   // launch sequence number (upper half of the mailbox tags)
    DevBuf<unsigned> d_arrive; unsigned arrive_total = 0;    // team kernel: [0] arrival counter (and its value after the launches so far), [1] abort word, [2] blocks done
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
    DevBuf<unsigned> d_stream_arrive;         // streaming step: blocks delivered per channel
    DevBuf<double> d_stream_pieces;           // and the groups' float64 sums [channels][groups][4]
    int fused_slots = 0;                      // CUs usable by the fused kernel (0 = not queried yet, -1 = none)
    DevBuf<float> d_stats;                                   // 4 per signal
    DevBuf<float> d_xstage, d_ostage;                        // a host input / output, staged
    // small host-to-host execs (the unchanged dataset loop: one 2000-sample frame per call): pinned, device-mapped staging that the
    // kernels read and write in place
    PinnedBuf<float> xpin, opin;
    struct PoolBuf { PinnedBuf<float> buf; bool used = false; };
    std::array<PoolBuf, kPinPoolMax> pin_pool;              // hssfsst_exec_pinned: pinned, device-mapped result buffers lent to the caller
    std::mutex pin_mu;                                       // ... guards `used` and the buffers' replacement (hssfsst_pinned_release may
                                                             // come from another host thread)
    DevBuf<long long> d_starts;                              // frame-list staging (hssfsst_exec_list with host starts)
    DevBuf<float> d_frames;                                  // frames gathered from a list, dense [batch][n]
    // hssfsst_exec_ragged: the list's tables -- RaggedSignal[batch], z-score unit starts int[batch + 1], chunk list int2[] -- in one
    // block, kept while the next list has the same lengths and offsets; where they lie in it and how many they are
    UploadedTable rtab{"exec_ragged"};
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

namespace {

// The dynamic-LDS limit is a property of the kernel instantiation (per device), not of a plan: raise it ONCE to
// the full 160 KiB, so that plans with different band widths sharing an instantiation cannot lower it under each
// other and the hot path makes no driver call for it.
using hssfsst::kMaxLdsBytes;
template <class Kern>
int allow_full_lds(Kern kern, int device, std::atomic<unsigned long long>& done)
{
    const unsigned long long bit = 1ull << (device & 63);
    if (done.load(std::memory_order_acquire) & bit) return 0;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes));
    done.fetch_or(bit, std::memory_order_release);
    return 0;
}

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
void name_kernel(char (&name)[sizeof(hssfsst_plan::last_kernel)], int waves, long long grid, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    const int k = vsnprintf(name, sizeof(name), fmt, ap);
    va_end(ap);
    if (k > 0 && static_cast<size_t>(k) < sizeof(name))
        snprintf(name + k, sizeof(name) - static_cast<size_t>(k), " [%d waves/block, grid %lld]", waves, grid);
}

void exec_report(hssfsst_plan* p, const ExecCtx& cx)
{
    std::memcpy(p->last_kernel, cx.kernel, sizeof(p->last_kernel));
    p->last_fused = (cx.fused || cx.team_launch != 0u) ? 1 : 0;      // (a team launch whose gated fallback is two launches counts as fused too)
    p->last_zpath = cx.zpath;
}

int out_floats_per_sample(const hssfsst_plan* p) { return p->mode == HSSFSST_MODE_ABS ? p->K : 2 * p->K; }

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

inline size_t core128_lds_bytes(const hssfsst_plan* pl, int wpb, bool pair) { return hssfsst::core128_lds_bytes(pl->mf, wpb, pair); }

// the Core128Params every launch of an MFMA plan starts from: the plan-constant fields
hssfsst::Core128Params core128_params(const hssfsst_plan* pl)
{
    hssfsst::Core128Params cp{};
    cp.atab = pl->d_atab.get(); cp.wtab = pl->d_wtab.get(); cp.twtab = pl->d_wtab.get() + 2 * pl->nwin; cp.r2scale = pl->r2scale;
    cp.klo = pl->klo; cp.K = pl->K; cp.mode = pl->mode;
    return cp;
}

int ensure_status(hssfsst_plan* pl);
template <int NT, int RQ, bool FAST, int WPB, int S1C = -1, bool PAIR = false, bool RAGGED = false>
int launch_core128_wpb(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks)
{
    size_t lds = core128_lds_bytes(pl, WPB, PAIR);
    auto kern = hssfsst::fsst_core128_kernel<NT, RQ, kFpw128, FAST, WPB, S1C, false, false, PAIR, RAGGED>;
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = allow_full_lds(kern, pl->device, lds_ok)) return rc;
    int& slots = RAGGED ? pl->ragged_slots : pl->core128_slots;
    if (int rc = resident_blocks(pl, slots, kern, 64 * WPB, lds, false)) return rc;     // persistent grid = what is resident at once
    int64_t blocks = nchunks;                            // small launches: one chunk per block, spread over the CUs
    if (blocks > slots) blocks = slots;
    name_kernel(cx.kernel, WPB, blocks, "fsst_core128_kernel<%d, %d, %d, %s, %d, %d, false%s%s>", NT, RQ, kFpw128, FAST ? "true" : "false", WPB, S1C,
                PAIR ? ", pairs" : "", RAGGED ? ", ragged" : "");
    hssfsst::Core128Params cq = cp;
    if constexpr (PAIR) {                                // (a pair's bounded wait reports through the status word)
        if (int rcs = ensure_status(pl)) return rcs;
        cq.status = pl->d_status;
    }
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(64 * WPB), lds, cx.st, cq);
    HIP_TRY(hipGetLastError());
    return 0;
}

// One rolling step in ONE launch (fsst_core128_kernel<.., STREAM>, fsst_mfma128.hpp): the chunk's groups, one per ticket, blocks
// bound to channels; tape append, transform, running-moments merge and normalisation.  Returns 1 when it launched, 0 when the
// step should take the three-launch route (a shape whose plain transform would not be this kernel's one-group chunks).
template <int NT, int RQ, int WPB, bool PAIR>
int launch_stream(hssfsst_plan* pl, float* tape_at, long long tape_len, const float* x_new_dev, long long x_stride, int channels, int chunk,
                  float* out, double* state, float* mirror, hipStream_t st)
{
    const int ngroups = (chunk + 15) / 16;
    const hssfsst::Core128Regions reg = hssfsst::core128_regions(ngroups, channels);
    if (!(reg.npc[0] == 0 && reg.npc[1] == 0 && reg.gpc[2] == 1)) return 0;      // (the plain kernel's chunks are not single groups)
    const size_t lds = core128_lds_bytes(pl, WPB, PAIR);
    if (lds > kMaxLdsBytes) return 0;
    auto kern = hssfsst::fsst_core128_kernel<NT, RQ, kFpw128, true, WPB, -1, false, true, PAIR>;
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = allow_full_lds(kern, pl->device, lds_ok)) return rc;
    if (int rc = resident_blocks(pl, pl->stream_slots, kern, 64 * WPB, lds, false)) return rc;
    if (state && pl->d_stream_arrive.cap < static_cast<size_t>(channels)) {
        if (int rc = pl->d_stream_arrive.grow(static_cast<size_t>(channels))) return rc;
        HIP_TRY(hipMemsetAsync(pl->d_stream_arrive.get(), 0, static_cast<size_t>(channels) * sizeof(unsigned), st));
    }
    if (state) {
        if (int rc = pl->d_stream_pieces.grow(static_cast<size_t>(channels) * ngroups * 4)) return rc;
    }
    if (int rcs = ensure_status(pl)) return rcs;
    int bpc = pl->stream_slots / channels;                // blocks per channel: spread a small step over the chip
    if (bpc > ngroups) bpc = ngroups;
    if (bpc < 1) bpc = 1;
    hssfsst::Core128Params cp = core128_params(pl);
    cp.x = tape_at; cp.xstride = tape_len; cp.out = out; cp.partials = nullptr;
    cp.n = pl->nwin - 1 + chunk; cp.nsig = channels; cp.col0 = pl->nwin / 2; cp.ncols = chunk; cp.reg = reg;
    cp.xnew = x_new_dev; cp.xnew_stride = x_stride; cp.hist = pl->nwin - 1; cp.bpc = bpc; cp.state = state; cp.arrive = pl->d_stream_arrive.get(); cp.pieces = pl->d_stream_pieces.get(); cp.mirror = mirror;
    const long long grid = static_cast<long long>(channels) * bpc;
    cp.status = pl->d_status;
    name_kernel(pl->last_kernel, WPB, grid, "fsst_core128_kernel<%d, %d, %d, true, %d, -1, false, stream%s>", NT, RQ, kFpw128, WPB, PAIR ? ", pairs" : "");
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(64 * WPB), lds, st, cp);
    HIP_TRY(hipGetLastError());
    return 1;
}

// Fused z-score launch (STACK; fsst_mfma128.hpp "Fused z-score"): one persistent block per CU, every CU owns whole signals.  FAST: the
// wide-store epilogue (nwin 128, even K <= 24); otherwise the general one (any K: nwin 256, or nwin 128 with an odd or wide band), whose
// z-score tickets sweep a chunk as float4s: every signal's feature block has to start on a 16-byte boundary.  Returns 1 when it launched, 0 when
// this exec should take the two-kernel path (signal too long for the LDS partials, or a batch that would leave CUs idle for a whole signal), < 0 on error.
template <int NT, int RQ, bool FAST, int WPB, int S1C>
int launch_fused(hssfsst_plan* pl, ExecCtx& cx, hssfsst::Core128Params cp, int64_t batch, int ngroups)
{
    if (ngroups > hssfsst::kFusedMaxGroups || (ngroups + kFpw128 / 16 - 1) / (kFpw128 / 16) < hssfsst::kFusedMinChunks) return 0;
    if (!FAST && (((static_cast<long long>(cp.ncols) * 2 * pl->K) & 3) != 0 || (reinterpret_cast<uintptr_t>(cp.out) & 15) != 0)) return 0;
    const size_t lds = core128_lds_bytes(pl, WPB, false) + (FAST ? hssfsst::kCtlFusedFloats - hssfsst::kCtlFloats : 0) * sizeof(float);
    if (lds > static_cast<size_t>(kMaxLdsBytes)) return 0;
    auto kern = hssfsst::fsst_core128_kernel<NT, RQ, kFpw128, FAST, WPB, S1C, true>;
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = allow_full_lds(kern, pl->device, lds_ok)) return rc;
    if (int rc = resident_blocks(pl, pl->fused_slots, kern, 64 * WPB, lds, true)) return rc;       // one block per CU
    if (pl->fused_slots < 1) return 0;
    const int64_t grid = pl->fused_slots;
    if (!hssfsst::fused_rounds_full(batch, grid)) return 0;
    if (int rcs = ensure_status(pl)) return rcs;
    cp.status = pl->d_status;
    name_kernel(cx.kernel, WPB, grid, "fsst_core128_kernel<%d, %d, %d, %s, %d, %d, true>", NT, RQ, kFpw128, FAST ? "true" : "false", WPB, S1C);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(64 * WPB), lds, cx.st, cp);
    HIP_TRY(hipGetLastError());
    return 1;
}

// The status word of the in-kernel waits lives in pinned, device-mapped host memory: a kernel that gave up writes it
// with a system-scope store, and the host looks at it without synchronising (at the start of the next exec, in
// hssfsst_plan_check after a synchronisation, at plan destruction).
int ensure_status(hssfsst_plan* pl)
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

// Canonical-class kernels (fsst_canon128.hpp): nwin = 128, STACK / STACK_UNNORM, the kept band a compile-time constant.  Two bands
// are instantiated: rows 4..25 = [25, 200] Hz at fs = 1000 (/root/reference/main.py:153-158, the reference's own configuration) and
// rows 2..25 = [25, 400] Hz at fs = 2000 -- the pass band of the Springer / Schmidt heart-sound segmenters on recordings at
// PhysioNet 2016's native rate (/root/reference/hss/datasets/heart_sounds.py:36-113 loads them un-resampled).  Every other band keeps
// fsst_core128_kernel.  (A third band is one line here: the template takes any even band of <= 24 rows inside rows 0..31.)
constexpr int kCanonBands[][2] = {{4, 22}, {2, 24}};

bool plan_is_canon(const hssfsst_plan* pl) { return pl->canon_idx >= 0; }
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
int launch_canon(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks)
{
    return canon_dispatch(pl, [&](auto KL, auto KN) { return launch_canon_band<decltype(KL)::value, decltype(KN)::value>(pl, cx, cp, nchunks); });
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

// f(o) with an exec's output `out` as what the plan says it holds: float*, _Float16* or __bf16*
template <class F>
void out_dispatch(const hssfsst_plan* p, void* out, F&& f)
{
    if (p->out_dtype == HSSFSST_DTYPE_F16) f(static_cast<_Float16*>(out));
    else if (p->out_dtype == HSSFSST_DTYPE_BF16) f(static_cast<__bf16*>(out));
    else f(static_cast<float*>(out));
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

// The plain (two-launch) core kernel of an MFMA plan: the row of kCore128Plain (fsst_launch_shape.hpp) that plan creation
// chose, turned into its instantiation by expanding that same table.  RAGGED: the instantiations of hssfsst_exec_ragged (the
// same rows, chunk list from the host).
template <bool RAGGED, size_t... I>
int launch_core128_row(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, std::index_sequence<I...>)
{
    using hssfsst::kCore128Plain;
    int rc = 0;
    (void)((static_cast<size_t>(pl->plain_row) == I
            && (rc = launch_core128_wpb<kCore128Plain[I].nt, kCore128Plain[I].rq, kCore128Plain[I].fast, kCore128Plain[I].wpb, kCore128Plain[I].s1c,
                                        kCore128Plain[I].pair, RAGGED>(pl, cx, cp, nchunks), true)) || ...);
    return rc;
}
template <bool RAGGED>
int launch_core128_plain(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks)
{
    // (not reached: mfma_facts calls a plan MFMA only when 4 wave regions fit, 2 at 512 points, and the table has a row of that
    //  many waves for every (nt, rq, fast) -- at 128 points with the wide-store epilogue K <= 24 and 16 regions fit;
    //  tests/native/launch_shape_check.cpp sweeps every band)
    if (pl->plain_row < 0) return fail(HSSFSST_EUNSUPPORTED, "LDS request %zu B per wave exceeds the 160 KiB budget", pl->mf.lds_per_wave);
    return launch_core128_row<RAGGED>(pl, cx, cp, nchunks, std::make_index_sequence<hssfsst::kCore128PlainRows>{});
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
            rc = canon_dispatch(pl, [&](auto KL, auto KN) {      // (16 waves per block, two held groups per wave)
                constexpr int kl = decltype(KL)::value, kn = decltype(KN)::value;
                if (pl->out_dtype == HSSFSST_DTYPE_F16) return launch_team16<kl, kn, 16, 2, _Float16>(pl, cx, cp, batch, ngroups, hout);
                if (pl->out_dtype == HSSFSST_DTYPE_BF16) return launch_team16<kl, kn, 16, 2, __bf16>(pl, cx, cp, batch, ngroups, hout);
                return launch_team16<kl, kn, 16, 2>(pl, cx, cp, batch, ngroups);
            });
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
            rc = canon16 ? launch_canon_fused(pl, cx, cp, batch, ngroups)
                 : canon ? launch_fused<16, 8, true, 16, 3>(pl, cx, cp, batch, ngroups) : launch_fused<16, 8, true, 16, -1>(pl, cx, cp, batch, ngroups);
        }
        if (rc < 0) return rc;
        if (rc == 1) { cx.fused = true; cx.zpath = 1; return 0; }
    }
    if (try_fused && !half && !fast && nt == 16 && pl->mode == HSSFSST_MODE_STACK && cx.zpref != HSSFSST_ZPATH_TEAM) {
        // the general epilogue: one CU per signal, the z-score as tickets of the same launch.  nwin 128, a band the wide-store epilogue does
        // not take (odd K or K > 24): 16 waves per block; nwin 256: as on the two-launch path (what fits the LDS: 8 for the canonical band).
        // (512 points: two launches, on wave pairs: 2.6 ms per 1024 windows against 3.0 for the single launch, whose instantiations are gone)
        int rc = 0;
        if (rq == 8 && core128_lds_bytes(pl, 16, false) <= kMaxLdsBytes) rc = launch_fused<16, 8, false, 16, -1>(pl, cx, cp, batch, ngroups);
        else if (rq == 16 && core128_lds_bytes(pl, 8, false) <= kMaxLdsBytes)
            rc = canon ? launch_fused<16, 16, false, 8, 3>(pl, cx, cp, batch, ngroups) : launch_fused<16, 16, false, 8, -1>(pl, cx, cp, batch, ngroups);
        if (rc < 0) return rc;
        if (rc == 1) { cx.fused = true; cx.zpath = 1; return 0; }
    }
    if (canon16) return launch_canon(pl, cx, cp, nchunks);
    return launch_core128_plain<false>(pl, cx, cp, nchunks);
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

// ---- hssfsst_allgather: ncclAllGather through dlopen (no link-time dependency on RCCL)
namespace {
struct RcclApi {
    void* handle = nullptr;
    int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    const char* (*error_string)(int) = nullptr;
    bool tried = false;
    std::string why;                                     // why RCCL is not available (dlerror() answers once: kept)
};
RcclApi& rccl_api()
{
    static RcclApi api;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (!api.tried) {
        api.tried = true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            api.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (api.handle) break;
            const char* e = dlerror();
            if (e && api.why.empty()) api.why = e;
        }
        if (api.handle) api.why = "symbol ncclAllGather missing";
        if (api.handle) {
            api.all_gather = reinterpret_cast<decltype(api.all_gather)>(dlsym(api.handle, "ncclAllGather"));
            api.error_string = reinterpret_cast<decltype(api.error_string)>(dlsym(api.handle, "ncclGetErrorString"));
        }
    }
    return api;
}
}  // namespace

int hssfsst_allgather(const float* sendbuf, float* recvbuf, int64_t count, void* nccl_comm, void* stream, int timeout_ms)
{
    if (!sendbuf || !recvbuf || !nccl_comm || count < 0 || timeout_ms < 0) return fail(HSSFSST_EINVAL, "allgather: bad argument");
    if (count == 0) return 0;
    RcclApi& api = rccl_api();
    if (!api.all_gather) return fail(HSSFSST_EUNSUPPORTED, "allgather: RCCL (librccl.so.1: ncclAllGather) is not available: %s", api.why.empty() ? "dlopen failed" : api.why.c_str());
    hipStream_t st = static_cast<hipStream_t>(stream);
    constexpr int kNcclFloat32 = 7;                      // ncclFloat (rccl.h)
    const int rc = api.all_gather(sendbuf, recvbuf, static_cast<size_t>(count), kNcclFloat32, nccl_comm, st);
    if (rc != 0) return fail(HSSFSST_EHIP, "allgather: ncclAllGather: %s", api.error_string ? api.error_string(rc) : "error");
    if (timeout_ms == 0) return 0;
    hipEvent_t ev = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, st);
    const auto t0 = std::chrono::steady_clock::now();
    while (e == hipSuccess) {
        e = hipEventQuery(ev);
        if (e == hipSuccess) break;
        if (e != hipErrorNotReady) break;
        e = hipSuccess;
        if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > timeout_ms) {
            (void)hipEventDestroy(ev);
            return fail(HSSFSST_EHIP, "allgather: the collective did not complete within %d ms (a rank is missing?); it is still enqueued on the stream and owns both buffers", timeout_ms);
        }
        std::this_thread::yield();
    }
    (void)hipEventDestroy(ev);
    if (e != hipSuccess) return fail(HSSFSST_EHIP, "allgather: %s", hipGetErrorString(e));
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

// The end of an exec: a host output is copied back, the stream synchronised and the plan checked; a host input is only waited for
// (the caller may reuse it)
static int exec_finish(hssfsst_plan* p, void* out, const void* dout, size_t bytes, int x_on_device, int out_on_device, hipStream_t st)
{
    if (!out_on_device) {
        HIP_TRY(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return hssfsst_plan_check(p);
    }
    if (!x_on_device) HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// The any-length kernel (fsst_dft.hpp) for one exec: its tile search and launch
static int launch_dft(hssfsst_plan* p, ExecCtx& cx, const float* dx, float* kout, int64_t batch, int n, int64_t x_stride, int col0, int ncols)
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
        const long long quads = (static_cast<long long>(n) + 3) / 4;
        long long blocks = (static_cast<long long>(batch) * quads + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        hipLaunchKernelGGL(hssfsst::fsst_gather_frames_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, st,
                           dx, d_starts, p->d_frames.get(), static_cast<long long>(batch), n);
        HIP_TRY(hipGetLastError());
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
    if ((rc = exec_buffers(p, no, !tiny_out && !out_on_device, static_cast<size_t>(nblocks), batch, &dout, &kout)) != 0) return rc;

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
    } else switch (p->R) {
        case 1: rc = launch_core<1>(p, cx, cp, nblocks); break;
        case 2: rc = launch_core<2>(p, cx, cp, nblocks); break;
        case 4: rc = launch_core<4>(p, cx, cp, nblocks); break;
        case 8: rc = launch_core<8>(p, cx, cp, nblocks); break;
        case 16: rc = launch_core<16>(p, cx, cp, nblocks); break;
        default: rc = fail(HSSFSST_EUNSUPPORTED, "exec: unsupported radix %d", p->R);
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
    if ((rc = exec_buffers(p, no, !out_on_device, static_cast<size_t>(groups), batch, &dout, &kout)) != 0) return rc;

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
        rc = canon_dispatch(p, [&](auto KL, auto KN) { return launch_canon_band<decltype(KL)::value, decltype(KN)::value, true>(p, cx, cp, t.nchunks); });
    else
        rc = launch_core128_plain<true>(p, cx, cp, t.nchunks);
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
    hipLaunchKernelGGL(hssfsst::fsst_moments_merge_kernel, dim3(static_cast<unsigned>(batch)), dim3(hssfsst::kMomThreads), 0,
                       static_cast<hipStream_t>(stream), feats, state, n, p->K);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"

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
    const size_t total = o_tw + (p->ragged ? 0 : tables::twiddle_count(p->Mt));
    try {
        std::vector<cd> tab(total);
        if (!p->ragged) {
            bluestein_tables(n, p->M1, 1.0, tab.data(), tab.data() + o_B1);
            tables::twiddle_table(p->Mt, tab.data() + o_tw);
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
        std::vector<hssfsst::resample_detail::cd> tw(tables::twiddle_count(Mt));
        tables::twiddle_table(Mt, tw.data());
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

int64_t hssfsst_pack_recordings(const float* const* ptrs, const int64_t* lens, int64_t count, int stride, int n,
                                float* stage, int64_t stage_cap, int64_t* starts, int64_t starts_cap, int threads)
{
    if (!ptrs || !lens || !stage || !starts || count < 0 || stride < 1 || n < 1)
        return fail(HSSFSST_EINVAL, "pack_recordings: bad argument");
    std::vector<int64_t> pos(static_cast<size_t>(count) + 1, 0);
    int64_t nf = 0;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t T = lens[i];
        if (T < 0 || !ptrs[i]) return fail(HSSFSST_EINVAL, "pack_recordings: recording %lld is NULL or negative", static_cast<long long>(i));
        pos[i + 1] = pos[i] + T;
        // frame_signal: L = floor((T - n) / stride) frames, one fewer than fit; L <= 0 -> the single frame x[:n]
        int64_t L = (T - n >= 0) ? (T - n) / stride : -1;
        if (L <= 0) L = 1;
        if (nf + L > starts_cap) return fail(HSSFSST_EINVAL, "pack_recordings: more than %lld frames", static_cast<long long>(starts_cap));
        for (int64_t k = 0; k < L; ++k) starts[nf + k] = pos[i] + k * stride;
        nf += L;
    }
    const int64_t total = pos[count];
    if (total > stage_cap) return fail(HSSFSST_EINVAL, "pack_recordings: %lld samples exceed the staging capacity %lld",
                                       static_cast<long long>(total), static_cast<long long>(stage_cap));
    int nt = threads > 0 ? threads : static_cast<int>(total / (1 << 20)) + 1;     // one thread per 4 MB of float32
    if (nt > 8) nt = 8;
    if (nt > count) nt = static_cast<int>(count > 0 ? count : 1);
    auto work = [&](int t) {
        // thread t copies the recordings whose first sample falls into its share of the staging buffer
        const int64_t lo = total * t / nt, hi = total * (t + 1) / nt;
        for (int64_t i = 0; i < count; ++i)
            if (pos[i] >= lo && pos[i] < hi && lens[i] > 0) std::memcpy(stage + pos[i], ptrs[i], static_cast<size_t>(lens[i]) * sizeof(float));
    };
    if (nt <= 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
        work(0);
        for (auto& x : th) x.join();
    }
    return nf;
}

int64_t hssfsst_parse_signal_csv(const char* text, int64_t len, float* signals, int64_t* labels, int64_t cap)
{
    if (!text || len < 0 || cap < 0 || (cap > 0 && (!signals || !labels))) return fail(HSSFSST_EINVAL, "parse_signal_csv: bad argument");
    const char* p = text;
    const char* end = text + len;
    while (p < end && *p != '\n') ++p;                  // skiprows=1
    if (p < end) ++p;
    int64_t rows = 0;
    while (p < end) {
        const char* eol = p;
        while (eol < end && *eol != '\n') ++eol;
        const char* q = p;
        while (q < eol && (*q == ' ' || *q == '\t' || *q == '\r')) ++q;
        if (q < eol) {                                  // non-empty line
            char* stop = nullptr;
            const double sig = std::strtod(q, &stop);
            if (stop == q || stop >= eol || *stop != ',')
                return fail(HSSFSST_EINVAL, "parse_signal_csv: malformed row %lld", static_cast<long long>(rows + 2));
            const char* l0 = stop + 1;
            const double lab = std::strtod(l0, &stop);
            if (stop == l0) return fail(HSSFSST_EINVAL, "parse_signal_csv: malformed label in row %lld", static_cast<long long>(rows + 2));
            if (rows < cap) { signals[rows] = static_cast<float>(sig); labels[rows] = static_cast<int64_t>(lab); }
            ++rows;
        }
        p = (eol < end) ? eol + 1 : end;
    }
    return rows;
}

int hssfsst_normalize_running(hssfsst_plan* p, float* feats, int64_t batch, int n, const double* state, void* stream)
{
    if (!p || !feats || !state || batch < 0 || n < 1) return fail(HSSFSST_EINVAL, "normalize_running: bad argument");
    if (batch == 0 || p->K == 0) return 0;
    if (batch > 0x7fffffffLL || static_cast<long long>(n) * 2 * p->K >= 0x7fffffffLL) return fail(HSSFSST_EINVAL, "normalize_running: too large");
    DEVICE_SCOPE(p->device);
    int rc;
    if ((rc = p->d_stats.grow(static_cast<size_t>(batch) * 4)) != 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float4* stats = reinterpret_cast<float4*>(p->d_stats.get());
    hipLaunchKernelGGL(hssfsst::fsst_stats_from_state_kernel, dim3(static_cast<unsigned>((batch + 63) / 64)), dim3(64), 0, st,
                       state, stats, static_cast<int>(batch));
    const int64_t zgrid = batch < 4096 ? batch : 4096;
    hipLaunchKernelGGL(hssfsst::fsst_normalize_kernel<float>, dim3(static_cast<unsigned>(zgrid)), dim3(256), 0, st,
                       static_cast<const float*>(feats), feats, stats, static_cast<const float*>(nullptr), 0, 0, n, p->K, static_cast<int>(batch), 1);
    HIP_TRY(hipGetLastError());
    return 0;
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
        if (debug_switches().no_pair)
            launched = (p->mf.nt == 32) ? launch_stream<32, 16, 4, false>(p, tape + (pos - hist), tape_len, xd, x_stride, channels, chunk, out, state, mirror, st)
                                     : launch_stream<16, 16, 4, false>(p, tape + (pos - hist), tape_len, xd, x_stride, channels, chunk, out, state, mirror, st);
        else
            launched = (p->mf.nt == 32) ? launch_stream<32, 16, 4, true>(p, tape + (pos - hist), tape_len, xd, x_stride, channels, chunk, out, state, mirror, st)
                                     : launch_stream<16, 16, 4, true>(p, tape + (pos - hist), tape_len, xd, x_stride, channels, chunk, out, state, mirror, st);
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
            hipLaunchKernelGGL(hssfsst::fsst_stream_finish_kernel, dim3(static_cast<unsigned>(channels)), dim3(hssfsst::kMomThreads), 0, st, out, state, chunk, p->K);
            HIP_TRY(hipGetLastError());
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

// What the sequence-model entry points (hssfsst_decode_states .. hssfsst_posteriors_durations_counts) share: the decisions of
// csrc/sequence_args.hpp put into words -- every text stands here, once -- and the loop over a list's launches.  Each entry
// calls the checks in its own order: that order is which of two errors a caller sees.
namespace {

namespace seqargs = hssfsst::seqargs;

int seq_check_list(const char* entry, const int64_t* offsets, int64_t count, int64_t max_steps)
{
    using Fault = seqargs::ListFault;
    const seqargs::ListFinding f = seqargs::check_list(offsets, count, max_steps);
    const long long i = f.index, limit = max_steps;
    if (f.fault == Fault::kNone) return 0;
    if (f.fault == Fault::kFirstNotZero) return fail(HSSFSST_EINVAL, "%s: offsets[0] is %lld, not 0", entry, static_cast<long long>(offsets[0]));
    if (f.fault == Fault::kTooManySteps)
        return fail(HSSFSST_EUNSUPPORTED, "%s: %lld steps in all, over the limit of 2^31 - 1", entry, static_cast<long long>(offsets[i]));
    const long long from = offsets[i], to = offsets[i + 1];
    if (f.fault == Fault::kNotIncreasing)
        return fail(HSSFSST_EINVAL, "%s: offsets do not increase at index %lld (offsets[%lld] = %lld, offsets[%lld] = %lld)", entry, i + 1, i,
                    from, i + 1, to);
    return fail(HSSFSST_EUNSUPPORTED, "%s: recording %lld has %lld steps, over the limit of %lld", entry, i, to - from, limit);
}

int seq_check_nonnull(const char* entry, std::initializer_list<seqargs::NamedPointer> required)
{
    if (const char* name = seqargs::first_null(required)) return fail(HSSFSST_EINVAL, "%s: bad argument (%s is NULL)", entry, name);
    return 0;
}

int seq_check_aligned(const char* entry, std::initializer_list<seqargs::NamedPointer> pointers)
{
    const seqargs::NamedPointer p = seqargs::first_misaligned(pointers);
    if (p.name) return fail(HSSFSST_EINVAL, "%s: %s is not %u-byte aligned", entry, p.name, p.alignment);
    return 0;
}

int seq_check_duration_table(const char* entry, const char* name, const float* table, int D)
{
    const seqargs::TableFinding f = seqargs::check_duration_table(table, D);
    if (f.fault == seqargs::TableFault::kNaN)
        return fail(HSSFSST_EINVAL, "%s: %s[%d][%d] is NaN (duration %d)", entry, name, f.row, f.column, f.column + 1);
    if (f.fault == seqargs::TableFault::kDeadRow)
        return fail(HSSFSST_EINVAL, "%s: row %d of %s is all -inf: state %d has no allowed duration", entry, f.row, name, f.row);
    return 0;
}

// (transitions, initial) and, with `durations`, the host tables of the explicit-duration model, whose diagonal is not read: the
// NaNs of the first two, then the two duration tables, then what the first two leave of a path.
int seq_check_model(const char* entry, const float* transitions, const float* initial, const float* durations = nullptr,
                    const float* edge = nullptr, int D = 0)
{
    const seqargs::ModelFinding f = seqargs::check_model(transitions, initial, durations != nullptr);
    if (f.nan_at >= 16) return fail(HSSFSST_EINVAL, "%s: initial[%d] is NaN", entry, f.nan_at - 16);
    if (f.nan_at >= 0) return fail(HSSFSST_EINVAL, "%s: transitions[%d][%d] is NaN", entry, f.nan_at / 4, f.nan_at % 4);
    if (durations) {
        if (int rc = seq_check_duration_table(entry, "durations", durations, D)) return rc;
        if (int rc = seq_check_duration_table(entry, "edge", edge, D)) return rc;
    }
    if (f.dead_row >= 0)
        return fail(HSSFSST_EINVAL,
                    durations ? "%s: row %d of transitions has no finite off-diagonal entry: state %d has no successor"
                              : "%s: row %d of transitions is all -inf: state %d has no successor", entry, f.dead_row, f.dead_row);
    if (f.no_start) return fail(HSSFSST_EINVAL, "%s: initial is all -inf: no state to start in", entry);
    return 0;
}

// The recordings of a list, `batch` per launch (the kernel's k*Batch: their offsets travel as kernel arguments).  For the
// recordings r0 .. r0 + nrec of each launch args.off[] is filled, launch(r0, nrec) enqueues `kernel` -- after setting args.rec0,
// where the kernel has one -- and the launch is checked.
template <class Args, class Launch>
int seq_for_each_batch(const char* entry, const char* kernel, const int64_t* offsets, int64_t count, int batch, Args& args, Launch launch)
{
    for (int64_t r0 = 0; r0 < count; r0 += batch) {
        const int nrec = static_cast<int>(std::min<int64_t>(batch, count - r0));
        for (int i = 0; i <= nrec; ++i) args.off[i] = offsets[r0 + i];
        launch(r0, nrec);
        if (int rc = launch_check(entry, kernel)) return rc;
    }
    return 0;
}

}  // namespace

// BiLSTM segmenter (hssfsst.h: hssfsst_segmenter_create): the model's weights, uploaded once in the layouts the kernels of
// csrc/segmenter_lstm.hpp consume, plus the scratch of its execs (owned by the plan, grown on demand, freed with it).
namespace {

// The forward tables of one BiLSTM layer, as the kernels of csrc/segmenter_lstm.hpp consume them (seglayout::wt_source,
// gate_col_row, fwd_stream_source): made on the host by seg_upload_layer or on the device by seg_pack_kernel.
struct SegLayer {
    int F = 0, Fp = 0;                                   // input width and its multiple of 32
    DevBuf<float> d_wt;                                  // [dir][Fp][4 Hp]: W_ih^T, columns in (unit tile, gate, unit) order
    DevBuf<float> d_bias;                                // [dir][4 Hp]: b_ih + b_hh, same order
    DevBuf<hssfsst::seg_h8> d_whh;                       // [dir][wave][K block][tile x gate][lane]{hi, lo}: W_hh x wscale, split f16
};

// The list of a ragged call on the device: its layout (segmenter_layout.hpp) and the layout's tables in one block
// (seglayout::table_block), made and uploaded only when the offsets differ from the last call's.
struct SegListTables {
    struct Views {
        const long long *off, *base;
        const int *len, *rec, *walk;
        int slots;
        long long walked;                                // base[tiles]: the steps one direction walks
    };
    hssfsst::seglayout::Layout lay;                      // (of tab's key: rebuilt between its begin and commit)
    UploadedTable tab;
    explicit SegListTables(const char* what) : tab(what) {}
    // offsets: checked by seg_check_list.  May throw std::bad_alloc.
    int acquire(const int64_t* offsets, int64_t count, hipStream_t st, Views* out)
    {
        namespace seglayout = hssfsst::seglayout;
        const seglayout::TableBlock b = seglayout::table_block(count);
        auto key = [&](size_t i) { return offsets[i]; };
        if (!tab.same(static_cast<size_t>(count + 1), key)) {
            unsigned char* h = nullptr;
            if (int rc = tab.begin(b.bytes, &h)) return rc;
            seglayout::build(offsets, count, lay);
            const std::vector<long long> base = seglayout::tile_base(lay);
            std::memcpy(h + b.o_off, lay.slot_off.data(), b.slots * sizeof(long long));
            std::memcpy(h + b.o_base, base.data(), (b.tiles + 1) * sizeof(long long));
            std::memcpy(h + b.o_len, lay.slot_len.data(), b.slots * sizeof(int));
            std::memcpy(h + b.o_rec, lay.slot_rec.data(), b.slots * sizeof(int));
            std::memcpy(h + b.o_walk, lay.tile_walk.data(), b.tiles * sizeof(int));
            if (int rc = tab.commit(st, static_cast<size_t>(count + 1), key)) return rc;
        }
        out->off = reinterpret_cast<const long long*>(tab.get() + b.o_off);
        out->base = reinterpret_cast<const long long*>(tab.get() + b.o_base);
        out->len = reinterpret_cast<const int*>(tab.get() + b.o_len);
        out->rec = reinterpret_cast<const int*>(tab.get() + b.o_rec);
        out->walk = reinterpret_cast<const int*>(tab.get() + b.o_walk);
        out->slots = static_cast<int>(b.slots);
        out->walked = seglayout::stash_floats_ragged(lay) / (2 * seglayout::kStashStepFloats);
        return 0;
    }
};

}  // namespace

struct hssfsst_segmenter {
    int device = -1;
    int F = 0, H = 0;
    struct Layer : SegLayer {
        float inv_scale = 1.0f;                          // 1 / (wscale x kSegHScale)
    } layer[2];
    DevBuf<float> d_lin;                                 // linear.weight (4, 2H) | linear.bias (4)
    DevBuf<float> d_pre;                                 // [dir][batch tile][Tc][gate tile][lane][4]: one chunk's input projection
    DevBuf<float> d_y1, d_y2;                            // (B, T, 2H): the layers' outputs
    DevBuf<float> d_state;                               // [h, c][dir][Bp][Hp]: carried from chunk to chunk and from layer 1 to layer 2
    SegListTables list{"segmenter_exec_ragged"};         // hssfsst_segmenter_exec_ragged: kept while the next call has the same offsets
};

namespace {

// src: {weight_ih, weight_hh, bias_ih, bias_hh} x {forward, reverse} of one nn.LSTM layer, as in its state_dict.  Every table is
// filled by its output index through the functions seg_pack_kernel uses; the scale is seg_pack_scale_kernel's.
int seg_upload_layer(hssfsst_segmenter::Layer& L, int F, int H, const float* const* src)
{
    namespace sl = hssfsst::seglayout;
    L.F = F;
    L.Fp = (F + 31) / 32 * 32;
    float wmax = 0.0f;
    for (int d = 0; d < 2; ++d) {
        const float* whh = src[4 * d + 1];
        for (size_t i = 0; i < static_cast<size_t>(4) * H * H; ++i) wmax = std::fmax(wmax, std::fabs(whh[i]));
    }
    // power-of-two scale that puts the largest |W_hh| in [2^12, 2^13): the lo halves of the split are normal f16 numbers down to
    // weights 2^-26 times the largest one, and a sum of 256 products with |h| x 2^10 stays far below the f32 range
    int e = 0;
    float wscale = 1.0f;
    if (wmax > 0.0f && std::isfinite(wmax)) { (void)std::frexp(wmax, &e); wscale = std::ldexp(1.0f, 13 - e); }
    L.inv_scale = 1.0f / (wscale * hssfsst::kSegHScale);
    const long long per_wt = static_cast<long long>(L.Fp) * sl::kGateCols, per_f = sl::kWtStreamHalves / 2;
    std::vector<float> wt(static_cast<size_t>(2 * per_wt)), bias(static_cast<size_t>(2) * sl::kGateCols);
    std::vector<_Float16> stream(static_cast<size_t>(2 * per_f));
    for (int d = 0; d < 2; ++d) {
        const float *wih = src[4 * d], *whh = src[4 * d + 1], *bih = src[4 * d + 2], *bhh = src[4 * d + 3];
        for (long long i = 0; i < per_wt; ++i) {
            const long long s = sl::wt_source(i, F, H);
            wt[static_cast<size_t>(d * per_wt + i)] = s >= 0 ? wih[s] : 0.0f;
        }
        for (int n = 0; n < sl::kGateCols; ++n) {
            const long long row = sl::gate_col_row(n, H);
            bias[static_cast<size_t>(d) * sl::kGateCols + n] = row >= 0 ? bih[row] + bhh[row] : 0.0f;
        }
        for (long long i = 0; i < per_f; ++i) {
            int lo = 0;
            const long long s = sl::fwd_stream_source(i, H, &lo);
            _Float16 out = static_cast<_Float16>(0.0f);
            if (s >= 0) {
                const float v = whh[s] * wscale;
                const _Float16 hi = static_cast<_Float16>(v);
                out = lo ? static_cast<_Float16>(v - static_cast<float>(hi)) : hi;
            }
            stream[static_cast<size_t>(d * per_f + i)] = out;
        }
    }
    if (int rc = L.d_wt.upload(wt.data(), wt.size())) return rc;
    if (int rc = L.d_bias.upload(bias.data(), bias.size())) return rc;
    return L.d_whh.upload(reinterpret_cast<const hssfsst::seg_h8*>(stream.data()), stream.size() / 8);
}

constexpr int64_t kSegMaxSteps = 0x7fffffffLL / 8;       // steps of one dense exec, and of one recording of a ragged one
constexpr int64_t kSegMaxBatch = 16 * 32768;
static_assert(hssfsst::seglayout::kSlotRows == hssfsst::kSegRows, "a tile of the layout is the recurrence workgroup's rows");

constexpr size_t kSegTileStepBytes = static_cast<size_t>(2) * hssfsst::kSegGateTiles * hssfsst::kSegTileFloats * sizeof(float);   // seglayout::Chunk

int seg_check_dtype(const char* what, int feats_dtype)
{
    if (feats_dtype != HSSFSST_DTYPE_F32 && feats_dtype != HSSFSST_DTYPE_F16 && feats_dtype != HSSFSST_DTYPE_BF16)
        return fail(HSSFSST_EINVAL, "%s: unknown feature dtype %d", what, feats_dtype);
    return 0;
}

// The list of a ragged call (count >= 1): count + 1 host offsets from 0, strictly increasing, no recording over the dense step
// limit, fewer than 2^31 steps in all.  One text for every entry point that takes such a list.
int seg_check_list(const char* what, const int64_t* offsets, int64_t count)
{
    namespace seglayout = hssfsst::seglayout;
    if (!offsets) return fail(HSSFSST_EINVAL, "%s: offsets is NULL", what);
    if (count > kSegMaxBatch) return fail(HSSFSST_EINVAL, "%s: count %lld too large", what, static_cast<long long>(count));
    if (offsets[0] != 0) return fail(HSSFSST_EINVAL, "%s: offsets[0] is %lld, not 0", what, static_cast<long long>(offsets[0]));
    if (const int64_t i = seglayout::first_bad_length(offsets, count, kSegMaxSteps); i >= 0) {
        if (offsets[i + 1] <= offsets[i])
            return fail(HSSFSST_EINVAL, "%s: offsets do not increase at index %lld (offsets[%lld] = %lld, offsets[%lld] = %lld)", what,
                        static_cast<long long>(i + 1), static_cast<long long>(i), static_cast<long long>(offsets[i]),
                        static_cast<long long>(i + 1), static_cast<long long>(offsets[i + 1]));
        return fail(HSSFSST_EINVAL, "%s: recording %lld has %lld steps, over the limit of %lld", what, static_cast<long long>(i),
                    static_cast<long long>(offsets[i + 1] - offsets[i]), static_cast<long long>(kSegMaxSteps));
    }
    if (offsets[count] > 0x7fffffffLL)
        return fail(HSSFSST_EINVAL, "%s: %lld steps in all, over the limit of 2^31 - 1", what, static_cast<long long>(offsets[count]));
    return 0;
}

// The geometry of a call as the forward kernels take it.  Dense: B rows of T steps, Bp padded rows.  Ragged: the list's tables.
void seg_dense_args(int B, int T, int Bp, hssfsst::SegProjArgs* pa, hssfsst::SegRecArgs* ra)
{
    pa->B = ra->B = B;
    pa->T = ra->T = T;
    ra->Bp = Bp;
}
void seg_ragged_args(const SegListTables::Views& t, hssfsst::SegProjArgs* pa, hssfsst::SegRecArgs* ra)
{
    ra->Bp = t.slots;
    pa->slot_off = ra->slot_off = t.off;
    pa->slot_len = ra->slot_len = t.len;
    pa->tile_walk = ra->tile_walk = t.walk;
    ra->tile_base = t.base;                              // (read by the TRAIN kernels only)
    ra->walked = t.walked;
}

// state [2][dir][Bp][Hp] <- (p0, p1): grown, then seeded by seg_pair_init_kernel.  slot_rec: the slots' recordings of a ragged call
// (B: the rows of p0 / p1), NULL for a dense one.
int seg_seed_state(const char* what, hipStream_t st, DevBuf<float>& state, const float* p0, const float* p1, int B, int H, int Bp,
                   const int* slot_rec)
{
    const size_t nstate = static_cast<size_t>(4) * Bp * hssfsst::kSegHp;
    if (int rc = state.grow(nstate)) return rc;
    hipLaunchKernelGGL((slot_rec ? hssfsst::seg_pair_init_kernel<true> : hssfsst::seg_pair_init_kernel<false>),
                       dim3(static_cast<unsigned>((nstate + 255) / 256)), dim3(256), 0, st, p0, p1, state.get(), B, H, Bp, slot_rec);
    return launch_check(what, slot_rec ? "seg_pair_init_kernel<ragged>" : "seg_pair_init_kernel");
}

// One layer, forwards: a launch pair (projection, recurrence) per chunk.  pa / ra come with the call's fields -- the geometry
// (seg_dense_args, seg_ragged_args), x and y, the scratch, H, the scale and, for TRAIN, the stash; the layer's and the chunk's are
// filled in here.  `what`: the entry point, for errors.
template <bool RAGGED, bool TRAIN>
int seg_forward_layer(const char* what, hipStream_t st, const SegLayer& L, hssfsst::SegProjArgs pa, hssfsst::SegRecArgs ra,
                      const std::vector<hssfsst::seglayout::Chunk>& chunks)
{
    pa.F = L.F; pa.Fp = L.Fp; pa.H = ra.H;
    pa.wt = L.d_wt.get(); pa.bias = L.d_bias.get();
    ra.whh = L.d_whh.get();
    for (const hssfsst::seglayout::Chunk& c : chunks) {
        pa.n = ra.n = c.n;
        pa.Tc = ra.Tc = c.Tc;
        if constexpr (RAGGED) {
            pa.s0 = ra.s0 = c.s0;
        } else {
            // the forward direction takes its chunks upwards, the reverse direction the mirrored ones downwards
            pa.t0[0] = ra.t0[0] = c.s0;
            pa.t0[1] = ra.t0[1] = ra.T - c.s0 - c.n;
        }
        hipLaunchKernelGGL(hssfsst::seg_proj_kernel<RAGGED>, dim3(4 * hssfsst::kSegHp / 64, static_cast<unsigned>(c.tiles * ((c.n + 7) / 8)), 2),
                           dim3(256), 0, st, pa);
        if (int rc = launch_check(what, RAGGED ? "seg_proj_kernel<ragged>" : "seg_proj_kernel")) return rc;
        hipLaunchKernelGGL((hssfsst::seg_rec_kernel<RAGGED, TRAIN>), dim3(static_cast<unsigned>(c.tiles), 2), dim3(64 * hssfsst::kSegWaves), 0, st, ra);
        if (int rc = launch_check(what, RAGGED ? (TRAIN ? "seg_rec_kernel<ragged, train>" : "seg_rec_kernel<ragged>")
                                               : (TRAIN ? "seg_rec_kernel<train>" : "seg_rec_kernel"))) return rc;
    }
    return 0;
}

// The two layers of an inference exec and its head: layer 2 reads layer 1's output rectified and starts from its final state.
// pa / ra: the call's geometry; rows: B T, or the list's steps.
template <bool RAGGED>
int seg_run_layers(hssfsst_segmenter* p, hipStream_t st, const void* feats, int feats_dtype, hssfsst::SegProjArgs pa, hssfsst::SegRecArgs ra,
                   const std::vector<hssfsst::seglayout::Chunk>& chunks, long long rows, float* logp)
{
    ra.pre = pa.pre = p->d_pre.get();
    ra.state = p->d_state.get();
    ra.H = p->H;
    pa.x = feats; pa.x_dtype = feats_dtype; pa.relu = 0;
    ra.y = p->d_y1.get(); ra.inv_scale = p->layer[0].inv_scale;
    if (int rc = seg_forward_layer<RAGGED, false>("segmenter_exec", st, p->layer[0], pa, ra, chunks)) return rc;
    pa.x = p->d_y1.get(); pa.x_dtype = HSSFSST_DTYPE_F32; pa.relu = 1;
    ra.y = p->d_y2.get(); ra.inv_scale = p->layer[1].inv_scale;
    if (int rc = seg_forward_layer<RAGGED, false>("segmenter_exec", st, p->layer[1], pa, ra, chunks)) return rc;
    hipLaunchKernelGGL(hssfsst::seg_head_kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, st, p->d_y2.get(), p->d_lin.get(),
                       p->d_lin.get() + static_cast<size_t>(8) * p->H, logp, rows, 2 * p->H);
    return launch_check("segmenter_exec", "seg_head_kernel");
}

// the scratch of an inference exec, in elements: one chunk's projection and the two layers' outputs of ylen elements each
int seg_grow_scratch(hssfsst_segmenter* p, size_t pre, size_t ylen)
{
    if (int rc = p->d_pre.grow(pre)) return rc;
    if (int rc = p->d_y1.grow(ylen)) return rc;
    return p->d_y2.grow(ylen);
}

}  // namespace

extern "C" {

int hssfsst_segmenter_create(hssfsst_segmenter** out, int device, int input_size, int hidden, const float* const* lstm_1,
                             const float* const* lstm_2, const float* linear_weight, const float* linear_bias)
{
    if (!out) return fail(HSSFSST_EINVAL, "segmenter_create: out is NULL");
    *out = nullptr;
    if (input_size < 1 || hidden < 1 || device < 0 || !lstm_1 || !lstm_2 || !linear_weight || !linear_bias)
        return fail(HSSFSST_EINVAL, "segmenter_create: bad argument (device=%d input_size=%d hidden=%d, or a NULL array)", device, input_size, hidden);
    for (int i = 0; i < 8; ++i)
        if (!lstm_1[i] || !lstm_2[i]) return fail(HSSFSST_EINVAL, "segmenter_create: bad argument (weight array %d of a layer is NULL)", i);
    if (hidden > hssfsst::kSegHp)
        return fail(HSSFSST_EUNSUPPORTED, "segmenter_create: hidden sizes above %d are not supported (hidden=%d)", hssfsst::kSegHp, hidden);
    if (input_size > (1 << 20)) return fail(HSSFSST_EUNSUPPORTED, "segmenter_create: input sizes above 2^20 are not supported (input_size=%d)", input_size);
    if (int rc = check_device("segmenter_create", device)) return rc;
    DEVICE_SCOPE(device);
    std::unique_ptr<hssfsst_segmenter> p(new (std::nothrow) hssfsst_segmenter());
    if (!p) return fail(HSSFSST_ENOMEM, "segmenter_create: host allocation failed");
    p->device = device; p->F = input_size; p->H = hidden;
    try {
        if (int rc = seg_upload_layer(p->layer[0], input_size, hidden, lstm_1)) return rc;
        if (int rc = seg_upload_layer(p->layer[1], 2 * hidden, hidden, lstm_2)) return rc;
        std::vector<float> lin(static_cast<size_t>(8) * hidden + 4);
        std::memcpy(lin.data(), linear_weight, static_cast<size_t>(8) * hidden * sizeof(float));
        std::memcpy(lin.data() + static_cast<size_t>(8) * hidden, linear_bias, 4 * sizeof(float));
        if (int rc = p->d_lin.upload(lin.data(), lin.size())) return rc;
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "segmenter_create: out of host memory");
    }
    *out = p.release();
    return 0;
}

int hssfsst_segmenter_destroy(hssfsst_segmenter* p)
{
    if (!p) return 0;
    DeviceGuard device_guard_(p->device);
    delete p;                                            // (the buffers free themselves)
    return 0;
}

int hssfsst_segmenter_info(const hssfsst_segmenter* p, int* input_size, int* hidden, int* max_hidden, int* device)
{
    if (max_hidden) *max_hidden = hssfsst::kSegHp;       // (a property of the library: answered for a NULL plan too)
    if (!p) return fail(HSSFSST_EINVAL, "segmenter_info: plan is NULL");
    if (input_size) *input_size = p->F;
    if (hidden) *hidden = p->H;
    if (device) *device = p->device;
    return 0;
}

int hssfsst_segmenter_exec(hssfsst_segmenter* p, const void* feats, int feats_dtype, int64_t batch, int64_t steps, const float* h0,
                           const float* c0, float* logp, void* stream)
{
    if (!p || !feats || !h0 || !c0 || !logp || batch < 1 || steps < 1)
        return fail(HSSFSST_EINVAL, "segmenter_exec: bad argument (batch=%lld steps=%lld, or a NULL pointer)", static_cast<long long>(batch),
                    static_cast<long long>(steps));
    if (int rc = seg_check_dtype("segmenter_exec", feats_dtype)) return rc;
    if (batch > kSegMaxBatch || steps > kSegMaxSteps)
        return fail(HSSFSST_EINVAL, "segmenter_exec: batch %lld or steps %lld too large", static_cast<long long>(batch), static_cast<long long>(steps));
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = static_cast<int>(batch), T = static_cast<int>(steps), H = p->H;
    const int nbt = (B + hssfsst::kSegRows - 1) / hssfsst::kSegRows, Bp = nbt * hssfsst::kSegRows;
    std::vector<hssfsst::seglayout::Chunk> chunks;
    try {
        chunks = hssfsst::seglayout::dense_chunks(T, nbt, kSegTileStepBytes, hssfsst::seglayout::kSegPreBytes);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "segmenter_exec: out of host memory");
    }
    if (int rc = seg_grow_scratch(p, hssfsst::seglayout::pre_floats(chunks, kSegTileStepBytes), static_cast<size_t>(B) * T * 2 * H)) return rc;
    if (int rc = seg_seed_state("segmenter_exec", st, p->d_state, h0, c0, B, H, Bp, nullptr)) return rc;
    hssfsst::SegProjArgs pa{};
    hssfsst::SegRecArgs ra{};
    seg_dense_args(B, T, Bp, &pa, &ra);
    return seg_run_layers<false>(p, st, feats, feats_dtype, pa, ra, chunks, static_cast<long long>(B) * T, logp);
}

int hssfsst_segmenter_exec_ragged(hssfsst_segmenter* p, const void* feats, int feats_dtype, const int64_t* offsets, int64_t count,
                                  const float* h0, const float* c0, int state_rows, float* logp, void* stream)
{
    namespace seglayout = hssfsst::seglayout;
    // the list first: what is wrong with it is said before the plan is looked at
    if (count < 0) return fail(HSSFSST_EINVAL, "segmenter_exec_ragged: count %lld is negative", static_cast<long long>(count));
    if (count == 0) return 0;
    if (int rc = seg_check_list("segmenter_exec_ragged", offsets, count)) return rc;
    if (state_rows != 1 && state_rows != count)
        return fail(HSSFSST_EINVAL, "segmenter_exec_ragged: state_rows %d is neither 1 nor count %lld", state_rows, static_cast<long long>(count));
    if (int rc = seg_check_dtype("segmenter_exec_ragged", feats_dtype)) return rc;
    if (!p || !feats || !h0 || !c0 || !logp)
        return fail(HSSFSST_EINVAL, "segmenter_exec_ragged: bad argument (%s is NULL)",
                    !p ? "plan" : !feats ? "feats" : !h0 ? "h0" : !c0 ? "c0" : "logp");
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int H = p->H;
    const seglayout::Layout& lay = p->list.lay;
    SegListTables::Views t{};
    std::vector<seglayout::Chunk> chunks;
    try {
        if (int rc = p->list.acquire(offsets, count, st, &t)) return rc;
        const int mib = debug_switches().seg_ragged_pre_mib;          // (A-B switch of tools/segmenter_ragged_bench.py: same bits)
        chunks = seglayout::ragged_chunks(lay, kSegTileStepBytes, mib > 0 ? static_cast<size_t>(mib) << 20 : seglayout::kSegPreBytes);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "segmenter_exec_ragged: out of host memory");
    }
    if (int rc = seg_grow_scratch(p, seglayout::pre_floats(chunks, kSegTileStepBytes), static_cast<size_t>(lay.total) * 2 * H)) return rc;
    if (int rc = seg_seed_state("segmenter_exec", st, p->d_state, h0, c0, state_rows, H, t.slots, t.rec)) return rc;
    hssfsst::SegProjArgs pa{};
    hssfsst::SegRecArgs ra{};
    seg_ragged_args(t, &pa, &ra);
    return seg_run_layers<true>(p, st, feats, feats_dtype, pa, ra, chunks, lay.total, logp);
}

}  // extern "C"

// Viterbi decoding of log-probs into state sequences (hssfsst.h: hssfsst_decode_states; csrc/segmenter_decode.hpp).  Stateless: the
// quantised transitions and the launch's offsets travel as kernel arguments, kDecodeBatch recordings per launch.
extern "C" {

int hssfsst_decode_info(int* segment_steps, int64_t* max_steps)
{
    if (segment_steps) *segment_steps = hssfsst::declayout::kSegSteps;
    if (max_steps) *max_steps = hssfsst::declayout::kMaxSteps;
    return 0;
}

int hssfsst_decode_states(const float* logp, const int64_t* offsets, int64_t count, const float* transitions, const float* initial,
                          uint8_t* states, int64_t* scores, int device, void* stream)
{
    namespace dl = hssfsst::declayout;
    constexpr const char* kEntry = "decode_states";
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"logp", logp}, {"offsets", offsets}, {"transitions", transitions}, {"initial", initial},
                                            {"states", states}})) return rc;
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (int rc = seq_check_aligned(kEntry, {{"logp", logp, 16}})) return rc;
    if (int rc = seq_check_model(kEntry, transitions, initial)) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, dl::kMaxSteps)) return rc;
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hssfsst::DecodeArgs args{};
    args.A = dl::quantise_transitions(transitions);
    args.pi = dl::quantise4(initial);
    return seq_for_each_batch(kEntry, "seg_decode_kernel", offsets, count, hssfsst::kDecodeBatch, args, [&](int64_t r0, int nrec) {
        hipLaunchKernelGGL(hssfsst::seg_decode_kernel, dim3(static_cast<unsigned>(nrec)), dim3(dl::kLanes), 0, st, logp, states,
                           scores ? reinterpret_cast<long long*>(scores) + r0 : nullptr, args);
    });
}

}  // extern "C"

// Explicit-duration Viterbi decoding (hssfsst.h: hssfsst_decode_durations; csrc/segmenter_decode_durations.hpp).  Stateless: the
// quantised transitions and the launch's offsets travel as kernel arguments, kDurDecodeBatch recordings per launch; the two
// duration tables travel as the arguments of fill launches into the head of the caller's workspace, so nothing is copied from
// host memory and every launch is stream-ordered.
extern "C" {

int hssfsst_decode_durations_info(int* max_duration, int64_t* max_steps, int64_t* workspace_bytes_per_step)
{
    if (max_duration) *max_duration = hssfsst::durlayout::kMaxDuration;
    if (max_steps) *max_steps = hssfsst::durlayout::kMaxSteps;
    if (workspace_bytes_per_step) *workspace_bytes_per_step = hssfsst::durlayout::kWorkspaceBytesPerStep;
    return 0;
}

int hssfsst_decode_durations(const float* logp, const int64_t* offsets, int64_t count, const float* transitions, const float* initial,
                             const float* durations, const float* edge, int max_duration, uint8_t* states, int64_t* scores,
                             void* workspace, int64_t workspace_bytes, int device, void* stream)
{
    namespace dl = hssfsst::declayout;
    namespace ul = hssfsst::durlayout;
    constexpr const char* kEntry = "decode_durations";
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"logp", logp}, {"offsets", offsets}, {"transitions", transitions}, {"initial", initial},
                                            {"durations", durations}, {"edge", edge}, {"states", states}, {"workspace", workspace}}))
        return rc;
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (max_duration < 1 || max_duration > ul::kMaxDuration)
        return fail(HSSFSST_EINVAL, "%s: max_duration %d is outside 1..%d", kEntry, max_duration, ul::kMaxDuration);
    const int D = max_duration;
    if (int rc = seq_check_aligned(kEntry, {{"logp", logp, 16}, {"workspace", workspace, 16}})) return rc;
    if (int rc = seq_check_model(kEntry, transitions, initial, durations, edge, D)) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, ul::kMaxSteps)) return rc;
    const int64_t need = ul::kWorkspaceBytesPerStep * ul::workspace_steps(offsets[count], D);
    if (workspace_bytes < need)
        return fail(HSSFSST_EINVAL, "%s: workspace of %lld bytes is too small: %lld steps and max_duration %d need %lld", kEntry,
                    static_cast<long long>(workspace_bytes), static_cast<long long>(offsets[count]), D, static_cast<long long>(need));
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    long long* table = static_cast<long long*>(workspace);
    unsigned short* back = reinterpret_cast<unsigned short*>(table + ul::table_words(D));
    hssfsst::DurFillArgs fa{};
    fa.D = D;
    for (int first = 0; first < 8 * D; first += hssfsst::kDurFillValues) {
        fa.first = first;
        fa.n = std::min(hssfsst::kDurFillValues, 8 * D - first);
        for (int i = 0; i < fa.n; ++i) fa.v[i] = first + i < 4 * D ? durations[first + i] : edge[first + i - 4 * D];
        hipLaunchKernelGGL(hssfsst::seg_durations_fill_kernel, dim3(1), dim3(hssfsst::kDurFillValues), 0, st, table, fa);
        if (int rc = launch_check(kEntry, "seg_durations_fill_kernel")) return rc;
    }
    hssfsst::DurDecodeArgs args{};
    args.tb = ul::quantise_tables(transitions, initial);
    args.D = D;
    return seq_for_each_batch(kEntry, "seg_decode_durations_kernel", offsets, count, hssfsst::kDurDecodeBatch, args, [&](int64_t r0, int nrec) {
        hipLaunchKernelGGL(hssfsst::seg_decode_durations_kernel, dim3(static_cast<unsigned>(nrec)), dim3(ul::kLanes), 0, st, logp, states,
                           scores ? reinterpret_cast<long long*>(scores) + r0 : nullptr, back, table, args);
    });
}

}  // extern "C"

// Forward-backward under the transition model (hssfsst.h: hssfsst_posteriors; csrc/segmenter_posteriors.hpp).  Stateless: the
// launch's offsets travel as kernel arguments, kPostBatch recordings per launch; the tables are read from device memory.
extern "C" {

int hssfsst_posteriors_info(int* segment_steps, int64_t* max_steps, int64_t* work_bytes_per_step, int64_t* work_bytes_per_recording)
{
    if (segment_steps) *segment_steps = hssfsst::postlayout::kSegSteps;
    if (max_steps) *max_steps = hssfsst::postlayout::kMaxSteps;
    if (work_bytes_per_step) *work_bytes_per_step = hssfsst::postlayout::kWorkBytesPerStep;
    if (work_bytes_per_recording) *work_bytes_per_recording = hssfsst::postlayout::kWorkBytesPerRecording;
    return 0;
}

int hssfsst_posteriors(const float* logp, const int64_t* offsets, int64_t count, const float* a_pi, const uint8_t* labels, float* gamma,
                       double* loglik, double* score, double* xi, double* gamma0, void* work, int64_t work_bytes, int device, void* stream)
{
    namespace pl = hssfsst::postlayout;
    constexpr const char* kEntry = "posteriors";
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"logp", logp}, {"offsets", offsets}, {"a_pi", a_pi}, {"gamma", gamma}, {"loglik", loglik},
                                            {"work", work}})) return rc;
    if (score && !labels) return fail(HSSFSST_EINVAL, "%s: bad argument (labels is NULL while score is not)", kEntry);
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (int rc = seq_check_aligned(kEntry, {{"logp", logp, 16}, {"gamma", gamma, 16}, {"work", work, 16}, {"a_pi", a_pi, 4}, {"loglik", loglik, 8},
                                            {"score", score, 8}, {"xi", xi, 8}, {"gamma0", gamma0, 8}})) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, pl::kMaxSteps)) return rc;
    const int64_t need = pl::workspace_bytes(offsets[count], count);
    if (work_bytes < need)
        return fail(HSSFSST_EINVAL, "%s: work of %lld bytes is too small: %lld steps in %lld recordings need %lld", kEntry,
                    static_cast<long long>(work_bytes), static_cast<long long>(offsets[count]), static_cast<long long>(count),
                    static_cast<long long>(need));
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hssfsst::PostArgs args{};
    return seq_for_each_batch(kEntry, "seg_posteriors_kernel", offsets, count, hssfsst::kPostBatch, args, [&](int64_t r0, int nrec) {
        args.rec0 = r0;
        hipLaunchKernelGGL(hssfsst::seg_posteriors_kernel, dim3(static_cast<unsigned>(nrec)), dim3(pl::kLanes), 0, st, logp, a_pi, labels, gamma,
                           loglik + r0, score ? score + r0 : nullptr, xi ? xi + 16 * r0 : nullptr, gamma0 ? gamma0 + 4 * r0 : nullptr,
                           static_cast<double*>(work), args);
    });
}

}  // extern "C"

// Forward-backward under the explicit-duration model (hssfsst.h: hssfsst_posteriors_durations;
// csrc/segmenter_duration_posteriors.hpp).  Stateless: the launch's offsets travel as kernel arguments, kDurPostBatch recordings per
// launch; all four tables are read from device memory, the two duration tables through a fill launch into the workspace's head.
// hssfsst_posteriors_durations_counts is the same call with the runs variant of the sweeps (it also leaves g and 1 / Z in a
// workspace that is larger by csrc/duration_counts_layout.hpp's parts) and, behind them, the counts launches
// (csrc/segmenter_duration_counts.hpp).
namespace {

// both entries: `with_counts` is the second one, whose `counts` is required
int posteriors_durations_run(const char* kEntry, bool with_counts, const float* logp, const int64_t* offsets, int64_t count, const float* a_pi,
                             const float* durations, const float* edge, int max_duration, const uint8_t* labels, float* gamma, float* onsets,
                             double* loglik, double* score, double* xi, double* s0, double* counts, void* work, int64_t work_bytes, int device,
                             void* stream)
{
    namespace dp = hssfsst::dplayout;
    namespace dc = hssfsst::dclayout;
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"logp", logp}, {"offsets", offsets}, {"a_pi", a_pi}, {"durations", durations}, {"edge", edge},
                                            {"gamma", gamma}, {"loglik", loglik}, {"work", work}})) return rc;
    if (with_counts)
        if (int rc = seq_check_nonnull(kEntry, {{"counts", counts}})) return rc;
    if (score && !labels) return fail(HSSFSST_EINVAL, "%s: bad argument (labels is NULL while score is not)", kEntry);
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (max_duration < 1 || max_duration > dp::kMaxDuration)
        return fail(HSSFSST_EINVAL, "%s: max_duration %d is outside 1..%d", kEntry, max_duration, dp::kMaxDuration);
    const int D = max_duration;
    if (int rc = seq_check_aligned(kEntry, {{"logp", logp, 16}, {"gamma", gamma, 16}, {"onsets", onsets, 16}, {"work", work, 16}, {"a_pi", a_pi, 4},
                                            {"durations", durations, 4}, {"edge", edge, 4}, {"loglik", loglik, 8}, {"score", score, 8},
                                            {"xi", xi, 8}, {"s0", s0, 8}, {"counts", counts, 8}})) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, dp::kMaxSteps)) return rc;
    const int64_t need = with_counts ? dc::workspace_bytes(offsets[count], count, D) : dp::workspace_bytes(offsets[count], count, D);
    if (work_bytes < need)
        return fail(HSSFSST_EINVAL, "%s: work of %lld bytes is too small: %lld steps in %lld recordings and max_duration %d need %lld", kEntry,
                    static_cast<long long>(work_bytes), static_cast<long long>(offsets[count]), static_cast<long long>(count), D,
                    static_cast<long long>(need));
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dc::Workspace wc = dc::workspace(offsets[count], count, D);
    const dp::Workspace& ws = wc.sweeps;                 // (dp::workspace(): the plain entry uses nothing behind it)
    char* w = static_cast<char*>(work);
    double* tabm = reinterpret_cast<double*>(w + ws.table_mant);
    int* tabe = reinterpret_cast<int*>(w + ws.table_exp);
    double* stash_m = reinterpret_cast<double*>(w + ws.stash_mant);
    int* stash_e = reinterpret_cast<int*>(w + ws.stash_exp);
    double* checkpoints = reinterpret_cast<double*>(w + ws.checkpoints);
    hipLaunchKernelGGL(hssfsst::seg_duration_posteriors_fill_kernel,
                       dim3(static_cast<unsigned>((8 * D + hssfsst::kDurPostFillLanes - 1) / hssfsst::kDurPostFillLanes)),
                       dim3(hssfsst::kDurPostFillLanes), 0, st, durations, edge, tabm, tabe, D);
    if (int rc = launch_check(kEntry, "seg_duration_posteriors_fill_kernel")) return rc;
    hssfsst::DurPostArgs args{};
    args.D = D;
    auto runs_of = [&](int64_t r0) {                     // what the launch of the recordings r0 .. sees of the second stash
        return hssfsst::DurRunsOut{reinterpret_cast<double*>(w + wc.g_mant), reinterpret_cast<int*>(w + wc.g_exp),
                                   reinterpret_cast<double*>(w + wc.invz_mant) + r0, reinterpret_cast<int*>(w + wc.invz_exp) + r0};
    };
    const char* sweep = with_counts ? "seg_duration_runs_sweep_kernel" : "seg_duration_posteriors_kernel";
    int rc = seq_for_each_batch(kEntry, sweep, offsets, count, hssfsst::kDurPostBatch, args, [&](int64_t r0, int nrec) {
        args.rec0 = r0;
        if (with_counts)
            hipLaunchKernelGGL(hssfsst::seg_duration_runs_sweep_kernel, dim3(static_cast<unsigned>(nrec)), dim3(dp::kLanes), 0, st, logp, a_pi,
                               durations, edge, labels, gamma, onsets, loglik + r0, score ? score + r0 : nullptr, xi ? xi + 16 * r0 : nullptr,
                               s0 ? s0 + 4 * r0 : nullptr, tabm, tabe, stash_m, stash_e, checkpoints, runs_of(r0), args);
        else
            hipLaunchKernelGGL(hssfsst::seg_duration_posteriors_kernel, dim3(static_cast<unsigned>(nrec)), dim3(dp::kLanes), 0, st, logp, a_pi,
                               durations, edge, labels, gamma, onsets, loglik + r0, score ? score + r0 : nullptr, xi ? xi + 16 * r0 : nullptr,
                               s0 ? s0 + 4 * r0 : nullptr, tabm, tabe, stash_m, stash_e, checkpoints, args);
    });
    if (rc || !with_counts) return rc;
    return seq_for_each_batch(kEntry, "seg_duration_run_counts_kernel", offsets, count, hssfsst::kDurPostBatch, args, [&](int64_t r0, int nrec) {
        args.rec0 = r0;
        hipLaunchKernelGGL(hssfsst::seg_duration_run_counts_kernel, dim3(static_cast<unsigned>(nrec), static_cast<unsigned>(dc::groups(D))),
                           dim3(dc::kLanes), 0, st, logp, a_pi, labels, counts + dc::counts_index(r0, 0, 0, 1, D), tabm, tabe, stash_m, stash_e,
                           checkpoints, runs_of(r0), args);
    });
}

}  // namespace

extern "C" {

int hssfsst_posteriors_durations_info(int* max_duration, int* segment_steps, int64_t* max_steps, int64_t* work_bytes_per_step,
                                      int64_t* work_bytes_per_recording, int64_t* work_bytes_per_duration)
{
    namespace dp = hssfsst::dplayout;
    if (max_duration) *max_duration = dp::kMaxDuration;
    if (segment_steps) *segment_steps = dp::kSegSteps;
    if (max_steps) *max_steps = dp::kMaxSteps;
    if (work_bytes_per_step) *work_bytes_per_step = dp::kWorkBytesPerStep;
    if (work_bytes_per_recording) *work_bytes_per_recording = dp::kWorkBytesPerRecording;
    if (work_bytes_per_duration) *work_bytes_per_duration = dp::kWorkBytesPerDuration;
    return 0;
}

int hssfsst_posteriors_durations(const float* logp, const int64_t* offsets, int64_t count, const float* a_pi, const float* durations,
                                 const float* edge, int max_duration, const uint8_t* labels, float* gamma, float* onsets, double* loglik,
                                 double* score, double* xi, double* s0, void* work, int64_t work_bytes, int device, void* stream)
{
    return posteriors_durations_run("posteriors_durations", false, logp, offsets, count, a_pi, durations, edge, max_duration, labels, gamma,
                                    onsets, loglik, score, xi, s0, nullptr, work, work_bytes, device, stream);
}

int hssfsst_posteriors_durations_counts_info(int64_t* work_bytes_per_step, int64_t* work_bytes_per_recording, int64_t* work_bytes_per_duration,
                                             int* durations_per_group)
{
    namespace dc = hssfsst::dclayout;
    if (work_bytes_per_step) *work_bytes_per_step = dc::kWorkBytesPerStep;
    if (work_bytes_per_recording) *work_bytes_per_recording = dc::kWorkBytesPerRecording;
    if (work_bytes_per_duration) *work_bytes_per_duration = dc::kWorkBytesPerDuration;
    if (durations_per_group) *durations_per_group = dc::kDurationsPerGroup;
    return 0;
}

int hssfsst_posteriors_durations_counts(const float* logp, const int64_t* offsets, int64_t count, const float* a_pi, const float* durations,
                                        const float* edge, int max_duration, const uint8_t* labels, float* gamma, float* onsets,
                                        double* loglik, double* score, double* xi, double* s0, double* counts, void* work, int64_t work_bytes,
                                        int device, void* stream)
{
    return posteriors_durations_run("posteriors_durations_counts", true, logp, offsets, count, a_pi, durations, edge, max_duration, labels,
                                    gamma, onsets, loglik, score, xi, s0, counts, work, work_bytes, device, stream);
}

}  // extern "C"

// Scoring a segmentation (hssfsst.h: hssfsst_score_states; csrc/segmenter_score.hpp, csrc/score_layout.hpp).  Stateless: the
// launch's offsets travel as kernel arguments, kScoreBatch recordings per launch of the kernels that read the arenas; the sort and
// the rank work on the caller's workspace, class after class, and the host decides the number of passes.
namespace {

// the launches of one class behind its items: the passes of the sort, then the three of the rank.  items_a holds the items.
int score_rank_class(const char* entry, hipStream_t st, unsigned char* work, const hssfsst::scorelayout::Workspace& w, int64_t n,
                     int passes, int per_recording, int64_t groups, unsigned long long* out)
{
    namespace sl = hssfsst::scorelayout;
    unsigned long long* src = reinterpret_cast<unsigned long long*>(work + w.items_a);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(work + w.items_b);
    unsigned* hist = reinterpret_cast<unsigned*>(work + w.hist);
    unsigned* sums = reinterpret_cast<unsigned*>(work + w.sums);
    unsigned* tile_agg = reinterpret_cast<unsigned*>(work + w.tile_agg);
    unsigned* tile_carry = reinterpret_cast<unsigned*>(work + w.tile_carry);
    const long long nblocks = sl::blocks(n), entries = sl::hist_entries(n), chunks = sl::scan_chunks(n), tiles = sl::rank_tiles(n);
    const dim3 sort_grid(static_cast<unsigned>(sl::sort_groups(n))), sort_block(sl::kSortThreads);
    const dim3 scan_grid(static_cast<unsigned>(chunks)), scan_block(sl::kScanThreads);
    for (int pass = 0; pass < passes; ++pass) {
        hipLaunchKernelGGL(hssfsst::seg_score_hist_kernel, sort_grid, sort_block, 0, st, src, hist, static_cast<long long>(n), nblocks, pass);
        if (int rc = launch_check(entry, "seg_score_hist_kernel")) return rc;
        hipLaunchKernelGGL(hssfsst::seg_score_scan_sums_kernel, scan_grid, scan_block, 0, st, hist, sums, entries);
        if (int rc = launch_check(entry, "seg_score_scan_sums_kernel")) return rc;
        hipLaunchKernelGGL(hssfsst::seg_score_scan_top_kernel, dim3(1), scan_block, 0, st, sums, chunks);
        if (int rc = launch_check(entry, "seg_score_scan_top_kernel")) return rc;
        hipLaunchKernelGGL(hssfsst::seg_score_scan_apply_kernel, scan_grid, scan_block, 0, st, hist, sums, entries);
        if (int rc = launch_check(entry, "seg_score_scan_apply_kernel")) return rc;
        hipLaunchKernelGGL(hssfsst::seg_score_scatter_kernel, sort_grid, sort_block, 0, st, src, dst, hist, static_cast<long long>(n), nblocks,
                           pass);
        if (int rc = launch_check(entry, "seg_score_scatter_kernel")) return rc;
        std::swap(src, dst);
    }
    const dim3 rank_grid(static_cast<unsigned>(tiles)), rank_block(sl::kRankThreads);
    hipLaunchKernelGGL(hssfsst::seg_score_rank_kernel<false>, rank_grid, rank_block, 0, st, src, static_cast<long long>(n), tile_agg, tile_carry,
                       out, per_recording, static_cast<long long>(groups));
    if (int rc = launch_check(entry, "seg_score_rank_kernel<false>")) return rc;
    hipLaunchKernelGGL(hssfsst::seg_score_rank_scan_kernel, dim3(1), dim3(64), 0, st, tile_agg, tile_carry, tiles);
    if (int rc = launch_check(entry, "seg_score_rank_scan_kernel")) return rc;
    hipLaunchKernelGGL(hssfsst::seg_score_rank_kernel<true>, rank_grid, rank_block, 0, st, src, static_cast<long long>(n), tile_agg, tile_carry,
                       out, per_recording, static_cast<long long>(groups));
    return launch_check(entry, "seg_score_rank_kernel<true>");
}

}  // namespace

extern "C" {

int hssfsst_score_info(int64_t* work_bytes_per_step, int64_t* work_bytes_per_recording, int64_t* work_bytes_constant, int* block_items,
                       int* digit_bits, int* max_passes)
{
    namespace sl = hssfsst::scorelayout;
    if (work_bytes_per_step) *work_bytes_per_step = sl::kWorkBytesPerStep;
    if (work_bytes_per_recording) *work_bytes_per_recording = sl::kWorkBytesPerRecording;
    if (work_bytes_constant) *work_bytes_constant = sl::kWorkBytesConstant;
    if (block_items) *block_items = sl::kBlockItems;
    if (digit_bits) *digit_bits = sl::kDigitBits;
    if (max_passes) *max_passes = sl::kMaxPasses;
    return 0;
}

int hssfsst_score_states(const float* logp, const uint8_t* states, const uint8_t* labels, const int64_t* offsets, int64_t count,
                         int per_recording, int64_t* confusion, int64_t* ignored, int64_t* rank, void* work, int64_t work_bytes,
                         const hssfsst_launch* where)
{
    namespace sl = hssfsst::scorelayout;
    constexpr const char* kEntry = "score_states";
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"labels", labels}, {"offsets", offsets}, {"confusion", confusion}, {"ignored", ignored},
                                            {"where", where}})) return rc;
    if (!states && !logp) return fail(HSSFSST_EINVAL, "%s: bad argument (states and logp are both NULL)", kEntry);
    if (rank && !logp) return fail(HSSFSST_EINVAL, "%s: bad argument (logp is NULL while rank is not)", kEntry);
    if (rank && !work) return fail(HSSFSST_EINVAL, "%s: bad argument (work is NULL while rank is not)", kEntry);
    const int device = where->device;
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (int rc = seq_check_aligned(kEntry, {{"logp", logp, 16}, {"work", work, 16}, {"confusion", confusion, 8}, {"ignored", ignored, 8},
                                            {"rank", rank, 8}})) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, seqargs::kMaxTotalSteps)) return rc;
    const int64_t total = offsets[count];
    const int64_t need = rank ? sl::workspace_bytes(total, count) : 0;
    if (work_bytes < need)
        return fail(HSSFSST_EINVAL, "%s: work of %lld bytes is too small: %lld steps in %lld recordings need %lld", kEntry,
                    static_cast<long long>(work_bytes), static_cast<long long>(total), static_cast<long long>(count),
                    static_cast<long long>(need));
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(where->stream);
    const int64_t groups = per_recording ? count : 1;
    const int64_t pooled[2] = {0, total};
    const int64_t* list = per_recording ? offsets : pooled;
    const int64_t nlist = per_recording ? count : 1;
    const std::pair<void*, size_t> outputs[3] = {{confusion, 128 * static_cast<size_t>(groups)}, {ignored, 8 * static_cast<size_t>(groups)},
                                                 {rank, 96 * static_cast<size_t>(groups)}};
    for (const auto& z : outputs) {                      // the kernels add into them
        if (!z.first) continue;
        const hipError_t e = hipMemsetAsync(z.first, 0, z.second, st);
        if (e != hipSuccess) return fail(HSSFSST_EHIP, "%s: clearing the outputs failed: %s", kEntry, hipGetErrorString(e));
    }
    hssfsst::ScoreArgs args{};
    args.per_recording = per_recording ? 1 : 0;
    auto grid_of = [&](int nrec) { return dim3(static_cast<unsigned>(sl::count_groups(args.off[nrec] - args.off[0]))); };
    if (int rc = seq_for_each_batch(kEntry, "seg_score_counts_kernel", list, nlist, sl::kScoreBatch, args, [&](int64_t r0, int nrec) {
            args.rec0 = r0;
            args.nrec = nrec;
            hipLaunchKernelGGL(hssfsst::seg_score_counts_kernel, grid_of(nrec), dim3(sl::kCountThreads), 0, st, logp, states, labels,
                               reinterpret_cast<unsigned long long*>(confusion), reinterpret_cast<unsigned long long*>(ignored),
                               reinterpret_cast<unsigned long long*>(rank), args);
        })) return rc;
    if (!rank) return 0;
    const sl::Workspace w = sl::workspace(total);
    const int passes = sl::passes(count, args.per_recording);
    for (int cls = 0; cls < 4; ++cls) {
        if (int rc = seq_for_each_batch(kEntry, "seg_score_keys_kernel", list, nlist, sl::kScoreBatch, args, [&](int64_t r0, int nrec) {
                args.rec0 = r0;
                args.nrec = nrec;
                hipLaunchKernelGGL(hssfsst::seg_score_keys_kernel, grid_of(nrec), dim3(sl::kCountThreads), 0, st, logp, states, labels,
                                   reinterpret_cast<unsigned long long*>(static_cast<unsigned char*>(work) + w.items_a), cls, args);
            })) return rc;
        if (int rc = score_rank_class(kEntry, st, static_cast<unsigned char*>(work), w, total, passes, args.per_recording, groups,
                                      reinterpret_cast<unsigned long long*>(rank) + 3 * cls)) return rc;
    }
    return 0;
}

}  // extern "C"

// Stitching overlapping windows' log-probs (hssfsst.h: hssfsst_stitch_windows; csrc/segmenter_stitch.hpp, csrc/stitch_layout.hpp).
// Stateless: the launch's offsets and window blocks travel as kernel arguments, kStitchBatch recordings per launch; nothing is
// copied from host memory and nothing waits.
namespace {

template <int MODE>
void stitch_launch(bool weighted, dim3 grid, hipStream_t st, const float* win, const float* weights, float* out, unsigned char* dissent,
                   const hssfsst::StitchArgs& args)
{
    const dim3 block(hssfsst::stitchlayout::kThreads);
    if (weighted) hipLaunchKernelGGL((hssfsst::seg_stitch_kernel<MODE, true>), grid, block, 0, st, win, weights, out, dissent, args);
    else hipLaunchKernelGGL((hssfsst::seg_stitch_kernel<MODE, false>), grid, block, 0, st, win, weights, out, dissent, args);
}

}  // namespace

extern "C" {

int hssfsst_stitch_windows(const float* win_logp, const int64_t* win_first, int64_t win_steps, const int64_t* offsets, int64_t count,
                           int n, int stride, const float* weights, int mode, float* out, uint8_t* dissent, hssfsst_launch where)
{
    namespace stl = hssfsst::stitchlayout;
    constexpr const char* kEntry = "stitch_windows";
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"win_logp", win_logp}, {"win_first", win_first}, {"offsets", offsets}, {"out", out}})) return rc;
    if (win_steps < 0) return fail(HSSFSST_EINVAL, "%s: win_steps %lld is negative", kEntry, static_cast<long long>(win_steps));
    if (n < 1) return fail(HSSFSST_EINVAL, "%s: window length %d is not positive", kEntry, n);
    if (stride < 1 || stride > n) return fail(HSSFSST_EINVAL, "%s: stride %d is outside 1 .. %d", kEntry, stride, n);
    if (mode != HSSFSST_STITCH_PROB && mode != HSSFSST_STITCH_LOGP && mode != HSSFSST_STITCH_SELECT)
        return fail(HSSFSST_EINVAL, "%s: unknown mode %d", kEntry, mode);
    const int device = where.device;
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (int rc = seq_check_aligned(kEntry, {{"win_logp", win_logp, 16}, {"out", out, 16}, {"weights", weights, 4}})) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, seqargs::kMaxTotalSteps)) return rc;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t rows = stl::window_rows(offsets[i + 1] - offsets[i], n, stride);
        if (win_first[i] < 0 || win_first[i] > win_steps - rows)
            return fail(HSSFSST_EINVAL, "%s: win_first[%lld] = %lld: the %lld window rows of recording %lld do not lie within the %lld of the arena",
                        kEntry, static_cast<long long>(i), static_cast<long long>(win_first[i]), static_cast<long long>(rows),
                        static_cast<long long>(i), static_cast<long long>(win_steps));
    }
    if (!stl::supported(n, stride))
        return fail(HSSFSST_EUNSUPPORTED, "%s: windows of %d steps at stride %d overlap %d-fold, over the limit of %d", kEntry, n, stride,
                    stl::ratio(n, stride), stl::kMaxRatio);
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(where.stream);
    hssfsst::StitchArgs args{};
    args.n = n;
    args.stride = stride;
    // (args.off is int: seq_check_list has held the list to 2^31 - 1 steps)
    return seq_for_each_batch(kEntry, "seg_stitch_kernel", offsets, count, stl::kStitchBatch, args, [&](int64_t r0, int nrec) {
        for (int i = 0; i < nrec; ++i) args.first[i] = win_first[r0 + i];
        args.nrec = nrec;
        const dim3 grid(static_cast<unsigned>(stl::launch_groups(offsets[r0 + nrec] - offsets[r0])));
        if (mode == HSSFSST_STITCH_PROB) stitch_launch<stl::kProb>(weights != nullptr, grid, st, win_logp, weights, out, dissent, args);
        else if (mode == HSSFSST_STITCH_LOGP) stitch_launch<stl::kLogp>(weights != nullptr, grid, st, win_logp, weights, out, dissent, args);
        else stitch_launch<stl::kSelect>(weights != nullptr, grid, st, win_logp, weights, out, dissent, args);
    });
}

}  // extern "C"

// One trainable BiLSTM layer (hssfsst.h: hssfsst_bilstm_create): the tables of its current weights, packed on the device by
// hssfsst_bilstm_set_weights (csrc/segmenter_train.hpp), and the scratch of its forward and backward calls.
struct hssfsst_bilstm {
    int device = -1;
    int H = 0;
    bool packed = false;
    SegLayer layer;                                      // the forward tables, of the weights set last
    DevBuf<hssfsst::seg_b8> d_bwd;                       // backward stream: W_hh, split bf16, as the B operand of dG . W_hh
    DevBuf<float> d_scale;                               // {wscale, inv_scale}: made and read on the device only
    DevBuf<float> d_pre;                                 // one chunk's input projection
    DevBuf<float> d_state;                               // forward [h, c][dir][Bp][Hp]; backward [dh_rec, dc][dir][Bp][Hp]
    SegListTables list{"bilstm_ragged"};                 // hssfsst_bilstm_*_ragged: kept while the next call has the same offsets
};

namespace {

int bilstm_check_shape(const char* what, int64_t batch, int64_t steps)
{
    if (batch < 1 || steps < 1)
        return fail(HSSFSST_EINVAL, "%s: bad argument (batch=%lld steps=%lld)", what, static_cast<long long>(batch), static_cast<long long>(steps));
    if (batch > kSegMaxBatch || steps > kSegMaxSteps)
        return fail(HSSFSST_EINVAL, "%s: batch %lld or steps %lld too large", what, static_cast<long long>(batch), static_cast<long long>(steps));
    return 0;
}

// out0, out1 (2, B, H) <- the state seg_seed_state made, after the launches chained through it; slot_rec as there
int bilstm_state_out(const char* what, hipStream_t st, const hssfsst_bilstm* p, float* out0, float* out1, int B, int Bp, const int* slot_rec)
{
    const size_t nout = static_cast<size_t>(4) * (slot_rec ? Bp : B) * p->H;
    hipLaunchKernelGGL((slot_rec ? hssfsst::seg_pair_out_kernel<true> : hssfsst::seg_pair_out_kernel<false>),
                       dim3(static_cast<unsigned>((nout + 255) / 256)), dim3(256), 0, st, p->d_state.get(), out0, out1, B, p->H, Bp, slot_rec);
    return launch_check(what, slot_rec ? "seg_pair_out_kernel<ragged>" : "seg_pair_out_kernel");
}

// A training forward: (h0, c0) in, the layer over the chunks with its stash, (hn, cn) out.  pa / ra: the call's geometry
// (seg_dense_args, seg_ragged_args); B: the rows of the states; slot_rec as in seg_seed_state.
template <bool RAGGED>
int bilstm_forward(const char* what, hssfsst_bilstm* p, hipStream_t st, const float* x, const float* h0, const float* c0, float* y, float* hn,
                   float* cn, float* stash, int B, const int* slot_rec, hssfsst::SegProjArgs pa, hssfsst::SegRecArgs ra,
                   const std::vector<hssfsst::seglayout::Chunk>& chunks)
{
    if (int rc = p->d_pre.grow(hssfsst::seglayout::pre_floats(chunks, kSegTileStepBytes))) return rc;
    if (int rc = seg_seed_state(what, st, p->d_state, h0, c0, B, p->H, ra.Bp, slot_rec)) return rc;
    pa.x = x; pa.x_dtype = HSSFSST_DTYPE_F32; pa.relu = 0;
    ra.pre = pa.pre = p->d_pre.get();
    ra.state = p->d_state.get(); ra.y = y; ra.H = p->H;
    ra.stash = stash; ra.inv_scale_dev = p->d_scale.get() + 1;
    if (int rc = seg_forward_layer<RAGGED, true>(what, st, p->layer, pa, ra, chunks)) return rc;
    return bilstm_state_out(what, st, p, hn, cn, B, ra.Bp, slot_rec);
}

// what both backwards give seg_bwd_rec_kernel; the state is seeded by then
hssfsst::SegBwdArgs bilstm_bwd_args(const hssfsst_bilstm* p, const float* stash, const float* c0, const float* dy, float* dgates, int B, int Bp)
{
    hssfsst::SegBwdArgs a{};
    a.stash = stash; a.c0 = c0; a.dy = dy; a.wbwd = p->d_bwd.get(); a.state = p->d_state.get(); a.dgates = dgates;
    a.B = B; a.H = p->H; a.Bp = Bp;
    return a;
}

}  // namespace

extern "C" {

int hssfsst_bilstm_create(hssfsst_bilstm** out, int device, int input_size, int hidden)
{
    if (!out) return fail(HSSFSST_EINVAL, "bilstm_create: out is NULL");
    *out = nullptr;
    if (input_size < 1 || hidden < 1 || device < 0)
        return fail(HSSFSST_EINVAL, "bilstm_create: bad argument (device=%d input_size=%d hidden=%d)", device, input_size, hidden);
    if (hidden > hssfsst::kSegHp)
        return fail(HSSFSST_EUNSUPPORTED, "bilstm_create: hidden sizes above %d are not supported (hidden=%d)", hssfsst::kSegHp, hidden);
    if (input_size > (1 << 20)) return fail(HSSFSST_EUNSUPPORTED, "bilstm_create: input sizes above 2^20 are not supported (input_size=%d)", input_size);
    if (int rc = check_device("bilstm_create", device)) return rc;
    DEVICE_SCOPE(device);
    std::unique_ptr<hssfsst_bilstm> p(new (std::nothrow) hssfsst_bilstm());
    if (!p) return fail(HSSFSST_ENOMEM, "bilstm_create: host allocation failed");
    p->device = device; p->H = hidden;
    SegLayer& L = p->layer;
    L.F = input_size;
    L.Fp = (input_size + 31) / 32 * 32;
    namespace sl = hssfsst::seglayout;
    if (int rc = L.d_wt.grow(static_cast<size_t>(2) * L.Fp * sl::kGateCols)) return rc;
    if (int rc = L.d_bias.grow(static_cast<size_t>(2) * sl::kGateCols)) return rc;
    if (int rc = L.d_whh.grow(static_cast<size_t>(sl::kWtStreamHalves / 8))) return rc;
    if (int rc = p->d_bwd.grow(static_cast<size_t>(sl::kBwdStreamHalves / 8))) return rc;
    if (int rc = p->d_scale.grow(2)) return rc;
    *out = p.release();
    return 0;
}

int hssfsst_bilstm_destroy(hssfsst_bilstm* p)
{
    if (!p) return 0;
    DeviceGuard device_guard_(p->device);
    delete p;
    return 0;
}

int hssfsst_bilstm_set_weights(hssfsst_bilstm* p, const float* const* weights, void* stream)
{
    if (!p || !weights) return fail(HSSFSST_EINVAL, "bilstm_set_weights: bad argument (%s is NULL)", !p ? "plan" : "weights");
    for (int i = 0; i < 8; ++i)
        if (!weights[i]) return fail(HSSFSST_EINVAL, "bilstm_set_weights: bad argument (weight array %d is NULL)", i);
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    namespace sl = hssfsst::seglayout;
    hssfsst::SegPackArgs a{};
    for (int i = 0; i < 8; ++i) a.src[i] = weights[i];
    const SegLayer& L = p->layer;
    a.F = L.F; a.Fp = L.Fp; a.H = p->H;
    a.scale = p->d_scale.get(); a.wt = L.d_wt.get(); a.bias = L.d_bias.get();
    a.whh = reinterpret_cast<_Float16*>(L.d_whh.get());
    a.bwd = reinterpret_cast<__bf16*>(p->d_bwd.get());
    hipLaunchKernelGGL(hssfsst::seg_pack_scale_kernel, dim3(1), dim3(1024), 0, st, a);
    if (int rc = launch_check("bilstm_set_weights", "seg_pack_scale_kernel")) return rc;
    const long long most = std::max<long long>(static_cast<long long>(2) * L.Fp * sl::kGateCols, std::max(sl::kWtStreamHalves, sl::kBwdStreamHalves));
    hipLaunchKernelGGL(hssfsst::seg_pack_kernel, dim3(static_cast<unsigned>((most + 255) / 256)), dim3(256), 0, st, a);
    if (int rc = launch_check("bilstm_set_weights", "seg_pack_kernel")) return rc;
    p->packed = true;
    return 0;
}

int hssfsst_bilstm_stash_floats(const hssfsst_bilstm* p, int64_t batch, int64_t steps, int64_t* floats)
{
    if (!floats) return fail(HSSFSST_EINVAL, "bilstm_stash_floats: floats is NULL");
    *floats = 0;
    (void)p;                                             // (every hidden size runs on the padded geometry: answered for a NULL plan too)
    if (int rc = bilstm_check_shape("bilstm_stash_floats", batch, steps)) return rc;
    *floats = hssfsst::seglayout::stash_floats(batch, steps);
    return 0;
}

int hssfsst_bilstm_forward(hssfsst_bilstm* p, const float* x, int64_t batch, int64_t steps, const float* h0, const float* c0, float* y,
                           float* hn, float* cn, float* stash, void* stream)
{
    if (!p) return fail(HSSFSST_EINVAL, "bilstm_forward: plan is NULL");
    if (int rc = bilstm_check_shape("bilstm_forward", batch, steps)) return rc;
    if (!x || !h0 || !c0 || !y || !hn || !cn || !stash)
        return fail(HSSFSST_EINVAL, "bilstm_forward: bad argument (%s is NULL)",
                    !x ? "x" : !h0 ? "h0" : !c0 ? "c0" : !y ? "y" : !hn ? "hn" : !cn ? "cn" : "stash");
    if (!p->packed) return fail(HSSFSST_EINVAL, "bilstm_forward: no weights yet (call hssfsst_bilstm_set_weights first)");
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = static_cast<int>(batch), T = static_cast<int>(steps);
    const int nbt = (B + hssfsst::kSegRows - 1) / hssfsst::kSegRows, Bp = nbt * hssfsst::kSegRows;
    std::vector<hssfsst::seglayout::Chunk> chunks;
    try {
        chunks = hssfsst::seglayout::dense_chunks(T, nbt, kSegTileStepBytes, hssfsst::seglayout::kSegPreBytes);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "bilstm_forward: out of host memory");
    }
    hssfsst::SegProjArgs pa{};
    hssfsst::SegRecArgs ra{};
    seg_dense_args(B, T, Bp, &pa, &ra);
    return bilstm_forward<false>("bilstm_forward", p, st, x, h0, c0, y, hn, cn, stash, B, nullptr, pa, ra, chunks);
}

int hssfsst_bilstm_backward(hssfsst_bilstm* p, const float* stash, const float* c0, const float* dy, const float* dhn, const float* dcn,
                            int64_t batch, int64_t steps, float* dgates, float* dh0, float* dc0, void* stream)
{
    if (!p) return fail(HSSFSST_EINVAL, "bilstm_backward: plan is NULL");
    if (int rc = bilstm_check_shape("bilstm_backward", batch, steps)) return rc;
    if (!stash || !c0 || !dy || !dgates || !dh0 || !dc0)
        return fail(HSSFSST_EINVAL, "bilstm_backward: bad argument (%s is NULL)",
                    !stash ? "stash" : !c0 ? "c0" : !dy ? "dy" : !dgates ? "dgates" : !dh0 ? "dh0" : "dc0");
    if (!p->packed) return fail(HSSFSST_EINVAL, "bilstm_backward: no weights yet (call hssfsst_bilstm_set_weights first)");
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = static_cast<int>(batch), T = static_cast<int>(steps);
    const int nbt = (B + hssfsst::kSegRows - 1) / hssfsst::kSegRows, Bp = nbt * hssfsst::kSegRows;
    if (int rc = seg_seed_state("bilstm_backward", st, p->d_state, dhn, dcn, B, p->H, Bp, nullptr)) return rc;
    hssfsst::SegBwdArgs a = bilstm_bwd_args(p, stash, c0, dy, dgates, B, Bp);
    a.T = T;
    // at most kSegMaxChunk steps per launch, chained through the carried (dh_rec, dc)
    for (int s0 = 0; s0 < T; s0 += hssfsst::seglayout::kSegMaxChunk) {
        a.s0 = s0;
        a.n = std::min(hssfsst::seglayout::kSegMaxChunk, T - s0);
        hipLaunchKernelGGL(hssfsst::seg_bwd_rec_kernel<false>, dim3(static_cast<unsigned>(nbt), 2), dim3(64 * hssfsst::kSegWaves), 0, st, a);
        if (int rc = launch_check("bilstm_backward", "seg_bwd_rec_kernel")) return rc;
    }
    return bilstm_state_out("bilstm_backward", st, p, dh0, dc0, B, Bp, nullptr);
}

int hssfsst_bilstm_stash_floats_ragged(const hssfsst_bilstm* p, const int64_t* offsets, int64_t count, int64_t* floats)
{
    if (!floats) return fail(HSSFSST_EINVAL, "bilstm_stash_floats_ragged: floats is NULL");
    *floats = 0;
    (void)p;                                             // (as hssfsst_bilstm_stash_floats: answered for a NULL plan too)
    if (count < 0) return fail(HSSFSST_EINVAL, "bilstm_stash_floats_ragged: count %lld is negative", static_cast<long long>(count));
    if (count == 0) return 0;
    if (int rc = seg_check_list("bilstm_stash_floats_ragged", offsets, count)) return rc;
    try {
        hssfsst::seglayout::Layout lay;
        hssfsst::seglayout::build(offsets, count, lay);
        *floats = hssfsst::seglayout::stash_floats_ragged(lay);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "bilstm_stash_floats_ragged: out of host memory");
    }
    return 0;
}

int hssfsst_bilstm_forward_ragged(hssfsst_bilstm* p, const float* x, const int64_t* offsets, int64_t count, const float* h0, const float* c0,
                                  float* y, float* hn, float* cn, float* stash, void* stream)
{
    namespace seglayout = hssfsst::seglayout;
    // the list first: what is wrong with it is said before the plan is looked at
    if (count < 0) return fail(HSSFSST_EINVAL, "bilstm_forward_ragged: count %lld is negative", static_cast<long long>(count));
    if (count == 0) return 0;
    if (int rc = seg_check_list("bilstm_forward_ragged", offsets, count)) return rc;
    if (!p) return fail(HSSFSST_EINVAL, "bilstm_forward_ragged: plan is NULL");
    if (!x || !h0 || !c0 || !y || !hn || !cn || !stash)
        return fail(HSSFSST_EINVAL, "bilstm_forward_ragged: bad argument (%s is NULL)",
                    !x ? "x" : !h0 ? "h0" : !c0 ? "c0" : !y ? "y" : !hn ? "hn" : !cn ? "cn" : "stash");
    if (!p->packed) return fail(HSSFSST_EINVAL, "bilstm_forward_ragged: no weights yet (call hssfsst_bilstm_set_weights first)");
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    SegListTables::Views t{};
    std::vector<seglayout::Chunk> chunks;
    try {
        if (int rc = p->list.acquire(offsets, count, st, &t)) return rc;
        chunks = seglayout::ragged_chunks(p->list.lay, kSegTileStepBytes, seglayout::kSegPreBytes);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "bilstm_forward_ragged: out of host memory");
    }
    hssfsst::SegProjArgs pa{};
    hssfsst::SegRecArgs ra{};
    seg_ragged_args(t, &pa, &ra);
    return bilstm_forward<true>("bilstm_forward_ragged", p, st, x, h0, c0, y, hn, cn, stash, static_cast<int>(count), t.rec, pa, ra, chunks);
}

int hssfsst_bilstm_backward_ragged(hssfsst_bilstm* p, const float* stash, const float* c0, const float* dy, const float* dhn, const float* dcn,
                                   const int64_t* offsets, int64_t count, float* dgates, float* dh0, float* dc0, void* stream)
{
    namespace seglayout = hssfsst::seglayout;
    if (count < 0) return fail(HSSFSST_EINVAL, "bilstm_backward_ragged: count %lld is negative", static_cast<long long>(count));
    if (count == 0) return 0;
    if (int rc = seg_check_list("bilstm_backward_ragged", offsets, count)) return rc;
    if (!p) return fail(HSSFSST_EINVAL, "bilstm_backward_ragged: plan is NULL");
    if (!stash || !c0 || !dy || !dgates || !dh0 || !dc0)
        return fail(HSSFSST_EINVAL, "bilstm_backward_ragged: bad argument (%s is NULL)",
                    !stash ? "stash" : !c0 ? "c0" : !dy ? "dy" : !dgates ? "dgates" : !dh0 ? "dh0" : "dc0");
    if (!p->packed) return fail(HSSFSST_EINVAL, "bilstm_backward_ragged: no weights yet (call hssfsst_bilstm_set_weights first)");
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    SegListTables::Views t{};
    std::vector<seglayout::BwdChunk> chunks;
    try {
        if (int rc = p->list.acquire(offsets, count, st, &t)) return rc;
        chunks = seglayout::ragged_bwd_chunks(p->list.lay);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "bilstm_backward_ragged: out of host memory");
    }
    const int B = static_cast<int>(count);
    if (int rc = seg_seed_state("bilstm_backward_ragged", st, p->d_state, dhn, dcn, B, p->H, t.slots, t.rec)) return rc;
    hssfsst::SegBwdArgs a = bilstm_bwd_args(p, stash, c0, dy, dgates, B, t.slots);
    a.slot_off = t.off; a.slot_len = t.len; a.slot_rec = t.rec; a.tile_walk = t.walk; a.tile_base = t.base;
    a.walked = t.walked; a.total = p->list.lay.total;
    // highest steps first, at most kSegMaxChunk per launch, chained through the carried (dh_rec, dc); a tile joins at its last step
    for (const seglayout::BwdChunk& c : chunks) {
        a.s0 = c.s0;
        a.n = c.n;
        hipLaunchKernelGGL(hssfsst::seg_bwd_rec_kernel<true>, dim3(static_cast<unsigned>(c.tiles), 2), dim3(64 * hssfsst::kSegWaves), 0, st, a);
        if (int rc = launch_check("bilstm_backward_ragged", "seg_bwd_rec_kernel<ragged>")) return rc;
    }
    return bilstm_state_out("bilstm_backward_ragged", st, p, dh0, dc0, B, t.slots, t.rec);
}

}  // extern "C"
