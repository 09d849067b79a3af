// fsst_launch_shape.hpp -- what the host works out before an FSST launch: for a plan and a shape, which kernel instantiation
// runs, with how many waves per block, how much LDS, which grid and which chunk pattern.  The device headers read the same
// layout functions, so host and kernel cannot disagree about a byte count.
// No HIP type and no HIP call here: numbers in, numbers out, so all of it also compiles into a stand-alone program
// (tests/native/launch_shape_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hssfsst {

constexpr int kMaxLdsBytes = 160 * 1024;        // LDS of a CU: what a block may ask for (allow_full_lds of host_common.hpp raises a kernel's limit to it)
constexpr int kFpw128 = 64;                  // frames per wave tile of the MFMA kernels
constexpr int kPartFloats = 8;               // a statistics partial (fsst_device.hpp "Statistics")

// ---- Chunk pattern ------------------------------------------------------------------------------------------------------
// Work distribution: one persistent block of 16 waves per CU.  The launch is cut into CHUNKS of consecutive 16-frame
// groups of one signal; the chunk list is ordered by region -- all region-0 chunks of all signals (8 groups each),
// then region 1 (4 groups), then region 2 (2 groups).  Block B owns chunks B, B + grid, B + 2 grid, ... (the same
// mix of big and small chunks for every CU) and its waves draw them in that order from a counter in LDS, so the 16
// waves of a CU finish within one small chunk of each other.  Why: the SIMD arbiter favours the oldest wave, so with
// equal static work per wave the four waves of a SIMD finished at 114 / 125 / 140 / 162 us, and with one fixed chunk
// per wave and several rounds of 4-wave blocks the last 20 % of the kernel ran at falling occupancy
// (profiles/r01_block_timeline.txt).  A ticket counter in HBM instead of LDS costs ~4 ns per draw, serialised
// chip-wide: 23 552 draws made the kernel 0.29 ms.  The chunk pattern of a signal depends only on the number of
// columns, not on the batch, and every chunk writes its own statistics partial: results are independent of the
// batch composition and run-to-run deterministic whichever wave processes a chunk.
struct Core128Regions {
    int g0[3];            // first 16-frame group of the region (per signal)
    int gpc[3];           // groups per chunk
    int npc[3];           // chunks per signal
};

// Chunk pattern for `ngroups` 16-frame groups per signal: 8-group chunks, then 4-group chunks over the last
// quarter or so, then 2-group chunks at the very end (each chunk costs a counter draw, a tile staging and a
// statistics reduction, so the small ones are kept to the tail).  Measured (tail4, tail2): (16, 6) 0.1691 ms,
// (24, 2) 0.1683, (32, 6) 0.1701, (8, 4) 0.1738, 8-group chunks only 0.1749.
inline Core128Regions core128_regions(int ngroups, long long nsig = -1)
{
    Core128Regions r{};
    const int tail2 = ngroups >= 32 ? 6 : 0;             // groups wanted as 2-group chunks
    const int tail4 = ngroups >= 32 ? 16 : 0;            // groups wanted as 4-group chunks
    if (ngroups < 32) {
        // short signals / streaming steps (a rolling transform adds 8 groups per step): parallelism matters more than
        // the per-chunk overhead -- 2-group chunks up to 8 groups, 4-group chunks up to 31; and single groups when
        // the whole launch is smaller than the chip (one streaming step of 64 channels = 512 groups for 1024 SIMDs:
        // the step's latency is then one group, not two)
        const bool tiny = nsig >= 0 && ngroups <= 8 && nsig * ngroups <= 1024;
        const int gpc = tiny ? 1 : ngroups <= 8 ? 2 : 4;
        r.g0[0] = 0; r.gpc[0] = 8; r.npc[0] = 0;
        r.g0[1] = 0; r.gpc[1] = 4; r.npc[1] = gpc == 4 ? (ngroups + 3) / 4 : 0;
        r.g0[2] = 0; r.gpc[2] = gpc == 1 ? 1 : 2; r.npc[2] = gpc == 1 ? ngroups : gpc == 2 ? (ngroups + 1) / 2 : 0;
        return r;
    }
    int big = ngroups - tail2 - tail4;
    big -= big % 8;                                      // whole 8-group chunks only
    if (big < 0) big = 0;
    int mid = ngroups - big - tail2;
    if (tail2 > 0) mid -= mid % 4;                       // whole 4-group chunks; the remainder joins the 2-group tail
    const int rest = ngroups - big - mid;
    r.g0[0] = 0;          r.gpc[0] = 8; r.npc[0] = big / 8;
    r.g0[1] = big;        r.gpc[1] = 4; r.npc[1] = (mid + 3) / 4;
    r.g0[2] = big + mid;  r.gpc[2] = 2; r.npc[2] = (rest + 1) / 2;
    return r;
}
constexpr int core128_chunks_per_signal(const Core128Regions& r) { return r.npc[0] + r.npc[1] + r.npc[2]; }

constexpr long long kRaggedUnitFloats = 1 << 16;       // floats of a ragged exec's z-score unit, fsst_ragged.hpp (256 kB: 64 float4 per thread)
constexpr int kRaggedGroupBits = 24;         // groups of a signal below 2^24 (n < 2^28: the host allows n * 2 nf < 2^31)
struct alignas(8) RaggedChunk {              // the kernels read it as int2 (hssfsst.hip asserts size and alignment)
    int sig;                                 // signal
    int groups;                              // first group | (groups - 1) << kRaggedGroupBits
};

// Chunk list of a ragged exec: each signal cut as core128_regions(its groups, 1) cuts it alone, and the list ordered by region
// across signals -- every 8-group chunk first, then the 4-group ones, then the 2- / 1-group ones -- so the small chunks stay in
// the tail as in a dense launch.  Entry {signal, first group | (groups - 1) << kRaggedGroupBits}.
inline void core128_ragged_chunks(const int* ngroups, long long nsig, std::vector<RaggedChunk>& out)
{
    out.clear();
    std::vector<Core128Regions> regs(static_cast<size_t>(nsig));
    for (long long s = 0; s < nsig; ++s) regs[s] = core128_regions(ngroups[s], 1);
    for (int rg = 0; rg < 3; ++rg)
        for (long long s = 0; s < nsig; ++s) {
            const Core128Regions& r = regs[s];
            for (int c = 0; c < r.npc[rg]; ++c) {
                const int g0 = r.g0[rg] + c * r.gpc[rg];
                const int ng = std::min(r.gpc[rg], ngroups[s] - g0);
                out.push_back(RaggedChunk{static_cast<int>(s), g0 | ((ng - 1) << kRaggedGroupBits)});
            }
        }
}

// ---- LDS layout of the MFMA kernels (fsst_mfma128.hpp) --------------------------------------------------------------------
// LDS planes of one 16-frame group (per wave), packed complex (re, im) per cell:
//   own  [16 frames][own_ld]  columns for rows 8*s0 .. 8*s1+7, the 8-aligned cover of the kept band:
//                             source k' stores (-1)^k' V[k'] into its column unconditionally
//                             (address = per-lane base + compile-time offset); sources whose
//                             8-row stripe lies outside the cover skip the store (wave-uniform);
//   disp [16 frames][LDF(K)]  kept rows only, zero-initialised: corrections from displaced sources.
constexpr int odd_up(int v) { return (v & 1) ? v : v + 1; }      // odd => b64 conflict-free
constexpr int plane_ldf(int K) { return odd_up(K); }
// rq = first-stage radix = rows per stripe (8 for nwin = 128, 16 for nwin = 256): source k' = rq * s + r sits in stripe s
constexpr int own_s0(int klo, int rq = 8) { return klo / rq; }
constexpr int own_s1(int klo, int K, int rq = 8) { return (klo + K - 1) / rq; }   // inclusive stripe
constexpr int own_ld(int klo, int K, int rq = 8)
{
    return odd_up(rq * (own_s1(klo, K, rq) - own_s0(klo, rq) + 1) + 1);
}
// MFMA A-operand constants: [pass][nt taps][k-step][64 lanes] floats, rq / 8 passes of rq / 4 k-steps
constexpr int core128_atab_floats(int rq = 8, int nt = 16) { return (rq / 8) * nt * (rq / 4) * 64; }
// the float64 fold constants of an "exact group" (resolve_group_f64, fsst_mfma128.hpp): [pass][tap][k-step][lane]
constexpr int fold64_doubles(int rq, int nt) { return (rq / 8) * nt * (rq / 4) * 64; }
// FAST epilogue: byte offsets, inside a wave's own plane, of the two (re,re) / (im,im) pairs that make up
// float4 number f = lane + 64 i of a 16-frame group's contiguous [16][2K] output image (K even, K <= 24).
// tab[i][lane] = first pair, tab[3 + i][lane] = second pair; a pair's second element is 8 bytes further.
inline void core128_store_offsets(int klo, int K, int* tab /* [6][64] */, int rq = 8)
{
    const int Q = (K >> 1) > 0 ? (K >> 1) : 1;
    const int old = own_ld(klo, K, rq), koff0 = klo - rq * own_s0(klo, rq);
    for (int i = 0; i < 3; ++i)
        for (int lane = 0; lane < 64; ++lane) {
            const int f = lane + 64 * i;
            const int jj = (f / Q < 15) ? f / Q : 15, c = 4 * (f - (f / Q) * Q);
            const int rowb = jj * old + koff0;
            tab[i * 64 + lane] = (c < K) ? (rowb + c) * 8 : (rowb + c - K) * 8 + 4;
            tab[(3 + i) * 64 + lane] = (c + 2 < K) ? (rowb + c + 2) * 8 : (rowb + c + 2 - K) * 8 + 4;
        }
}
constexpr int kCtlFloats = 16 + 192;         // block control words in LDS: [0] work counter, [16..207] the wide-store offset
                                             // table (3 words per lane: held in registers it costs the 16-wave kernels a spill)
// FUSED kernel: [0] ticket counter, [1..2] groups delivered per signal slot (monotone), [3] a wait gave up, [4..7] epoch
// of the resolved statistics (4 slots), [8..15] (unused), [16..79] per-lane column classes of the z-score
// pass, [80..271] the wide-store offset table (3 words per lane; the fused kernel has no register to spare for it),
// [272..287] four float4 statistics, [288 ..] the statistics partials of two signals [2][kFusedMaxGroups][kPartFloats]
constexpr int kFusedMaxGroups = 128;         // signals of at most 2048 frames
constexpr int kFusedMinChunks = 16;          // and of at least 16 chunks: see "Slots" in the kernel
constexpr int kCtlFusedFloats = 288 + 2 * kFusedMaxGroups * kPartFloats;
constexpr int tie_words(int nwin) { return nwin / 4; }     // the rounding-tie bitmap (flag[1] = "some bit is set")
constexpr int wave_lds_floats(int fpw, int klo, int K, int rq = 8, int nt = 16)
{
    return ((fpw + nt * rq - 1 + 3) / 4) * 4 + 2 * 16 * (own_ld(klo, K, rq) + plane_ldf(K)) + 4   // + dirty flag
           + tie_words(nt * rq);                                                                     // + tie queues
}
// PAIR (two waves share one wave region, fsst_mfma128.hpp "PAIR"): what a region holds besides
constexpr int kPairFloats = 4 + 64 + 3 * 256;  // [0..1] phase words, [2] the pair's ticket, [3] the odd wave's list count, [4..67] its per-lane
                                             // max |V|^2, then its list of additions (PairList: 256 cells, 256 values)

// the any-length kernel (fsst_dft.hpp): its rounding-tie queue, {bin | frame << 16, V.re, V.im} per entry (the MFMA kernel's is more compact)
constexpr int kDftTieQueue = 256;
constexpr int kDftTieWords = 4 + 3 * kDftTieQueue;
// G = 16-frame groups per work item (a tile of 16 G frames): every A-operand load feeds G MFMAs on G independent
// accumulators (the constants come from L2: one group per item is bound by those loads -- nwin 1024: 1.3 k windows/s).
constexpr int dft_xs_floats(int nk4, int G = 1) { return ((16 * G + 4 * nk4 + 3) / 4) * 4; }
constexpr int dft_wave_lds_floats(int nk4, int K, int G = 1)
{
    return dft_xs_floats(nk4, G) + 2 * 16 * G * plane_ldf(K) + 4 + kDftTieWords;
}

// the canonical-band kernels (fsst_canon128.hpp, fsst_team16.hpp): their tables in LDS, and a block's bytes -- tables, the
// kernel's control floats, one region of CanonCfg<KLO, KC>::wave_floats() per wave
constexpr int kCanonOpFloats = 16 * 64 * 4;              // f16 A operand: [16 taps][64 lanes][8 halves] = 16 kB
constexpr int kCanonAtabFloats = kCanonOpFloats + 4 * 128;   // + {cos, sin}(2 pi m / 128) as float64 (rounding-tie path), 2 kB
constexpr int kCanonLdsTabFloats = kCanonAtabFloats + 4 * 33 * 2;   // what the kernels keep in LDS: + the interior frame of the offset table ("Offsets"), 1 kB
// the offset table behind the operand table (fsst_canon128.hpp "Offsets"; built by fsst_tables.hpp canon_offset_spectra)
constexpr int kCanonYcGroup = 33;                         // float2 per lane group: za[0..15] | zb[0..15] | pad (the four lane groups of a wave read 264 bytes apart: different LDS banks)
constexpr int kCanonYcFrame = 4 * kCanonYcGroup * 2;      // floats per frame: [lane group][za[0..15] | zb[0..15] | -] as float2 (the lane's two 16-point spectra)
constexpr int kCanonYcRight = 80;                         // right-edge frames tabulated: 0..62 samples to the end, then 17 copies of the interior (a group of 16 frames that
                                                          // reaches into the last 63 columns reads one table whatever its first frame)
// interior [lane group][33] | left edge [lane group][entry][output column 0..63] | right edge [lane group][entry][samples to the end 0..79], float2 each:
// the 16 lanes of a lane group (consecutive frames) read consecutive words of the edge tables
constexpr int kCanonZcFloats = kCanonYcFrame + 4 * 32 * 64 * 2 + 4 * 32 * kCanonYcRight * 2;
constexpr size_t canon_lds_bytes(int ctl_floats, int wave_floats, int wpb = 16)
{
    return (kCanonLdsTabFloats + ctl_floats + static_cast<size_t>(wpb) * wave_floats) * sizeof(float);
}

// ---- The facts of an MFMA plan ------------------------------------------------------------------------------------------
// the MFMA kernels' window lengths and their taps (per-lane FFT size); the first-stage radix is nwin / taps
constexpr bool mfma_length(int nwin) { return nwin == 128 || nwin == 256 || nwin == 512; }
constexpr int mfma_taps(int nwin) { return nwin == 512 ? 32 : 16; }

struct MfmaFacts {
    int nt = 16;                  // taps (per-lane FFT size) of the MFMA kernel: nwin = nt * rq
    int rq = 0;                   // its first-stage radix; 0 = not an MFMA plan (the generic or the any-length kernel)
    bool fast = false;            // the wide-store epilogue applies: STACK modes, even K <= 24
    bool stripes03 = false;       // the band starts in stripe 0 of the own plane and ends in stripe 3 (the canonical [25, 200] Hz at fs = 1000, nwin 128 / 256)
    size_t lds_fixed = 0, lds_per_wave = 0;   // LDS bytes of the core kernel beside its wave regions, and of one wave region
};
// For a window of nwin points with kept rows [klo, klo + K), stack = one of the STACK modes.  rq stays 0 where nwin is not an
// MFMA length, and where too few wave regions of this band fit beside the A table -- at least 4 (2 at 512 points); long windows
// with very wide bands: generic kernel.
constexpr MfmaFacts mfma_facts(int nwin, int klo, int K, bool stack)
{
    MfmaFacts f;
    f.fast = stack && (K & 1) == 0 && K <= 24;
    if (!mfma_length(nwin)) return f;
    const int nt = mfma_taps(nwin), rq = nwin / nt, min_waves = (nwin == 512) ? 2 : 4;
    const size_t fixed = (core128_atab_floats(rq, nt) + kCtlFloats) * sizeof(float);
    const size_t per_wave = static_cast<size_t>(wave_lds_floats(kFpw128, klo, K, rq, nt)) * sizeof(float);
    if (fixed + min_waves * per_wave > static_cast<size_t>(kMaxLdsBytes)) return f;
    f.nt = nt; f.rq = rq; f.lds_fixed = fixed; f.lds_per_wave = per_wave;
    f.stripes03 = own_s0(klo, rq) == 0 && own_s1(klo, K, rq) == 3;
    return f;
}
// bytes of LDS of a core launch of an MFMA plan: wpb waves, pair: two waves per wave region
constexpr size_t core128_lds_bytes(const MfmaFacts& f, int wpb, bool pair)
{
    const size_t regions = pair ? wpb / 2 : wpb;
    return f.lds_fixed + regions * (f.lds_per_wave + (pair ? kPairFloats * sizeof(float) : 0));
}

// ---- The plain (two-launch) core kernel of an MFMA plan: fsst_core128_kernel<nt, rq, kFpw128, fast, wpb, s1c, .., pair> ------
// In priority order: a plan runs the first row of its (nt, rq, fast) whose s1c it satisfies (s1c = 3 wants stripes03) and whose
// wpb waves -- wpb / 2 regions of a pair -- fit the LDS: as many waves per block as fit beside the shared tables.
struct Core128PlainRow { int nt, rq; bool fast; int wpb, s1c; bool pair; };
constexpr Core128PlainRow kCore128Plain[] = {
    // nwin 128.  (fast is K <= 24: 16 regions always fit)
    {16, 8, true, 16, 3, false}, {16, 8, true, 16, -1, false},
    {16, 8, false, 16, -1, false}, {16, 8, false, 8, -1, false}, {16, 8, false, 4, -1, false},
    // nwin 256: 8 waves per block at most -- two per SIMD, up to 256 VGPRs, no scratch.  (Wave pairs lose here: 16 waves at 128
    // registers spill, core 0.770 vs 0.587 ms per 1024 windows; 12 waves at 170 registers: 0.739 ms)
    {16, 16, true, 8, -1, false}, {16, 16, false, 8, 3, false}, {16, 16, false, 8, -1, false},
    {16, 16, false, 4, -1, false}, {16, 16, true, 4, -1, false},
    // nwin 512: two waves per SIMD at most (32-point spectra in registers); wave pairs first, unless switched off
    {32, 16, true, 8, -1, true}, {32, 16, false, 8, -1, true}, {32, 16, false, 6, -1, true}, {32, 16, false, 4, -1, true},
    {32, 16, true, 8, -1, false}, {32, 16, false, 8, -1, false}, {32, 16, false, 6, -1, false}, {32, 16, true, 4, -1, false},
    {32, 16, false, 4, -1, false}, {32, 16, false, 3, -1, false}, {32, 16, false, 2, -1, false}, {32, 16, true, 2, -1, false},
};
constexpr int kCore128PlainRows = static_cast<int>(sizeof(kCore128Plain) / sizeof(kCore128Plain[0]));
// index of the plan's row in kCore128Plain, or -1 (no_pair: the process's HSSFSST_NO_PAIR switch)
constexpr int core128_plain_row(const MfmaFacts& f, bool no_pair)
{
    for (int i = 0; i < kCore128PlainRows; ++i) {
        const Core128PlainRow& r = kCore128Plain[i];
        if (r.nt == f.nt && r.rq == f.rq && r.fast == f.fast && (r.s1c < 0 || f.stripes03) && !(r.pair && no_pair)
            && core128_lds_bytes(f, r.wpb, r.pair) <= static_cast<size_t>(kMaxLdsBytes))
            return i;
    }
    return -1;
}

// ---- The one-CU-per-signal kernels: signals are dealt to the blocks round-robin and a signal is never split, so the last
// round must be nearly full -- at least 88 % (a quarter-full last round of 4 costs 4 / 3.25 = 23 %); otherwise the
// chunk-balanced two-kernel path wins
constexpr bool fused_rounds_full(int64_t batch, int64_t grid)
{
    const int64_t rounds = (batch + grid - 1) / grid;
    return !(batch < grid || rounds * grid * 100 > batch * 112);
}

// ---- The team kernel's geometry (fsst_team16.hpp "Progress": the conditions that header calls host-checked) ---------------
constexpr int kT16MaxCpc = 8;                // groups of a signal per CU (two blocks)
struct Team16Geometry {
    bool ok = false;                         // false: declined, this exec takes another path
    int T = 0;                               // CUs per team (power of two)
    int cpc_shift = 0;                       // log2 of the list positions per CU and signal
    int nteams = 0, grid = 0;                // grid = nteams * T blocks
    int slots = 0;                           // mailbox / statistics slots (power of two)
};
// G = 16-frame groups per signal; cus = CUs the kernel may use (one block each); WPB waves per block holding DEPTH group images
// each; the kernel's LDS keeps the partials of pslots signals and has ms statistics / mailbox slots.
constexpr Team16Geometry team16_geometry(int G, int64_t batch, long long xstride, int cus, int WPB, int DEPTH, int pslots, int ms)
{
    Team16Geometry g;
    if (G < 1 || G > kFusedMaxGroups) return g;          // (the resolver's LDS copy of a signal's partials: 128 groups)
    // team size: the smallest power of two that leaves a CU at most 16 groups of a signal (its 16 waves then have all of them in
    // flight at once and the kernel's progress argument holds)
    int T = 1;
    while ((WPB / 2) * T < G) T *= 2;                    // (cpc <= WPB is the kernel's progress argument; cpc <= WPB / 2 measured faster:
                                                         //  a signal's groups are handed out within half a round of the CU's waves)
    if (T > cus || T > 64) return g;
    int cpc = 1, cpc_shift = 0;                          // list positions per CU and signal (power of two; surplus ones are skipped)
    while (cpc * T < G) { cpc *= 2; ++cpc_shift; }
    if (cpc > WPB || cpc > kT16MaxCpc || G / T < 1) return g;
    if (cpc < 4 && T > 1) return g;                      // (a CU publishes whole blocks of four groups)
    // as many teams as the chip has room for, but no more than there are signals: the dataset loop's one frame per call
    // (/root/reference/hss/datasets/heart_sounds.py:166-168) starts one team's 16 blocks, not 256 of which 240 find nothing to do
    int nteams = cus / T;
    if (batch < nteams) nteams = static_cast<int>(batch);
    if ((batch + nteams - 1) / nteams > 65535) return g;
    if (xstride < 1 || xstride > 0x7fffffffLL || batch > 0x7fffffffLL) return g;      // (the kernel's 32-bit signal index and stride)
    // slots: a CU runs at most held_pos list positions ahead of its oldest unresolved signal = lead signals; a slot is reused
    // 2 lead + 2 signals later at the earliest (fsst_team16.hpp "Progress")
    const int held_pos = WPB * (DEPTH + 3);             // list positions a CU's waves hold: DEPTH held + transformed + landed + drawn each
    const int lead = (held_pos + G / T - 1) / (G / T) + 1;
    int slots = 8;
    while (slots < 2 * lead + 2) slots *= 2;
    if (slots > ms) return g;
    if (lead + 1 > pslots) return g;                     // (very short signals: more signals in flight per CU than its LDS keeps partials for)
    g.ok = true; g.T = T; g.cpc_shift = cpc_shift; g.nteams = nteams; g.grid = nteams * T; g.slots = slots;
    return g;
}

// ---- The z-score of a dense STACK exec as its own launches (fsst_normalize_kernel) ----------------------------------------
struct ZscoreShape {
    int64_t grid;         // blocks of the z-score sweep
    int slices;           // blocks per signal
    bool fused;           // the sweep's blocks reduce their signal's partials themselves (no fsst_stats_kernel launch)
};
constexpr ZscoreShape zscore_shape(int64_t batch)
{
    int64_t zgrid = 4096;
    // small batches: several blocks per signal, else one block per signal would leave most CUs idle
    int slices = 1;
    if (batch < 1024) {
        slices = static_cast<int>(1024 / batch);
        if (slices > 32) slices = 32;
    }
    if (zgrid > batch * slices) zgrid = batch * slices;
    // big batches, a block per signal: it reduces the signal's partials itself (no separate statistics
    // launch, 4-7 us per step); otherwise a tiny kernel does all reductions at once
    const bool fused = slices == 1 && zgrid == batch && batch >= 512;
    return {zgrid, slices, fused};
}

// ---- The any-length kernel's tile search (fsst_dft_kernel<G>) ------------------------------------------------------------
struct DftShape {
    int G;                // 16-frame groups per work item
    int waves;            // per block; 0: not even one wave's LDS fits
    long long nitems;     // batch x tiles
    long long blocks;
};
constexpr DftShape dft_shape(int nk4, int K, int ncols, int64_t batch)
{
    // groups per work item: 4 when four planes fit the LDS of a wave (each A-operand load then feeds four MFMAs),
    // else 2, else 1; then as many waves per block as fit (at most 8)
    // largest tile that still leaves >= 16 waves resident per CU (the MFMA chains are dependent: latency is hidden
    // by waves, not by the tile), else whatever keeps the most waves (measured: nwin 100 is fastest with small tiles)
    int G = 1, best_waves = -1;
    for (int cand = 4; cand >= 1; cand >>= 1) {
        const size_t pw = static_cast<size_t>(dft_wave_lds_floats(nk4, K, cand)) * sizeof(float);
        int w = static_cast<int>(static_cast<size_t>(kMaxLdsBytes) / pw);
        if (w > 8) w = 8;
        if (w < 1) continue;
        int per_cu = static_cast<int>(static_cast<size_t>(kMaxLdsBytes) / (pw * w)) * w;
        if (per_cu > 32) per_cu = 32;
        if (per_cu >= 16) { G = cand; best_waves = per_cu; break; }
        if (per_cu > best_waves) { G = cand; best_waves = per_cu; }
    }
    if (ncols <= 16) G = 1;
    const size_t per_wave = static_cast<size_t>(dft_wave_lds_floats(nk4, K, G)) * sizeof(float);
    int waves = static_cast<int>(static_cast<size_t>(kMaxLdsBytes) / per_wave);
    if (waves > 8) waves = 8;
    if (waves < 1) return {G, 0, 0, 0};
    const int ntiles = (ncols + 16 * G - 1) / (16 * G);
    const long long nitems = static_cast<long long>(batch) * ntiles;
    long long blocks = (nitems + waves - 1) / waves;
    if (blocks > 256 * 64) blocks = 256 * 64;                       // grid-stride beyond that
    return {G, waves, nitems, blocks};
}

}  // namespace hssfsst
