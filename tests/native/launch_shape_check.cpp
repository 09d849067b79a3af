// Stand-alone check of the FSST launch arithmetic (csrc/fsst_launch_shape.hpp: host only, no HIP): the plan facts and the
// plain-kernel table against the if-ladder that stood in launch_core128_plain, team16_geometry against the arithmetic that stood
// in launch_team16 -- and, on their own, the conditions the team kernel's progress argument names --, the chunk patterns, the
// z-score rule and the any-length kernel's tile search against their inline forms.  Built with -fsanitize=address,undefined by
// tests/test_host.py.  Any failed property or sanitizer report ends the run non-zero.
#include "fsst_launch_shape.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

using namespace hssfsst;

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { if (failures < 40) { std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } \
    } while (0)

// ---- the rules as they stood inline before this header, copied from hssfsst.hip --------------------------------------------
namespace parent {

constexpr int kMaxLdsBytes = 160 * 1024;
constexpr int kFpw128 = 64;
struct Plan {                                            // the fields choose_family / set_derived_facts filled
    int nwin = 0, klo = 0, K = 0;
    bool stack = false, mfma = false;
    int rq = 0, nt = 16;
    bool fast = false, stripes03 = false;
    size_t lds_fixed = 0, lds_per_wave = 0;
};
static bool g_no_pair = false;
struct Row { int nt, rq; bool fast; int wpb, s1c; bool pair; bool ok; };

inline size_t core128_lds_bytes(const Plan* pl, int wpb, bool pair)
{
    const size_t regions = pair ? wpb / 2 : wpb;
    return pl->lds_fixed + regions * (pl->lds_per_wave + (pair ? (4 + 64 + 3 * 256) * sizeof(float) : 0));
}

// choose_family's MFMA part and set_derived_facts
void make_facts(Plan* p)
{
    const int nwin = p->nwin;
    p->fast = p->stack && (p->K & 1) == 0 && p->K <= 24;
    if (!(nwin == 128 || nwin == 256 || nwin == 512)) return;
    // enough wave regions of this band must fit beside the A table (long windows with very wide bands: generic kernel)
    const int nt = nwin == 512 ? 32 : 16, rq = nwin / nt, min_waves = (nwin == 512) ? 2 : 4;
    const size_t fixed = ((rq / 8) * nt * (rq / 4) * 64 + (16 + 192)) * sizeof(float);
    const int s0 = p->klo / rq, s1 = (p->klo + p->K - 1) / rq;
    auto odd_up = [](int v) { return (v & 1) ? v : v + 1; };
    const int own_ld = odd_up(rq * (s1 - s0 + 1) + 1);
    const int wave_floats = ((kFpw128 + nt * rq - 1 + 3) / 4) * 4 + 2 * 16 * (own_ld + odd_up(p->K)) + 4 + (nt * rq) / 4;
    const size_t per_wave = static_cast<size_t>(wave_floats) * sizeof(float);
    if (fixed + min_waves * per_wave > 160 * 1024) return;
    p->mfma = true; p->rq = rq; p->nt = nt; p->lds_fixed = fixed; p->lds_per_wave = per_wave;
    p->stripes03 = s0 == 0 && s1 == 3;
}

template <int NT, int RQ, bool FAST, int WPB, int S1C = -1, bool PAIR = false, bool RAGGED = false>
Row launch_core128_wpb() { return Row{NT, RQ, FAST, WPB, S1C, PAIR, true}; }

template <bool RAGGED>
Row launch_core128_plain(const Plan* pl)
{
    const int rq = pl->rq, nt = pl->nt;
    const bool fast = pl->fast, canon = pl->stripes03;
    const size_t fixed = pl->lds_fixed, per_wave = pl->lds_per_wave, room = 160 * 1024;
    if (nt == 16 && rq == 8) {
        if (fast && canon) return launch_core128_wpb<16, 8, true, 16, 3, false, RAGGED>();
        if (fast) return launch_core128_wpb<16, 8, true, 16, -1, false, RAGGED>();   // K <= 24: 16 regions always fit
        if (fixed + 16 * per_wave <= room) return launch_core128_wpb<16, 8, false, 16, -1, false, RAGGED>();
        if (fixed + 8 * per_wave <= room) return launch_core128_wpb<16, 8, false, 8, -1, false, RAGGED>();
        if (fixed + 4 * per_wave <= room) return launch_core128_wpb<16, 8, false, 4, -1, false, RAGGED>();
    } else if (nt == 16 && rq == 16) {                                               // nwin = 256
        if (fast && fixed + 8 * per_wave <= room) return launch_core128_wpb<16, 16, true, 8, -1, false, RAGGED>();
        if (!fast && canon && fixed + 8 * per_wave <= room) return launch_core128_wpb<16, 16, false, 8, 3, false, RAGGED>();
        if (!fast && fixed + 8 * per_wave <= room) return launch_core128_wpb<16, 16, false, 8, -1, false, RAGGED>();
        if (!fast && fixed + 4 * per_wave <= room) return launch_core128_wpb<16, 16, false, 4, -1, false, RAGGED>();
        if (fast && fixed + 4 * per_wave <= room) return launch_core128_wpb<16, 16, true, 4, -1, false, RAGGED>();
    } else {                                                                         // nt == 32, rq == 16: nwin = 512
        if (!g_no_pair) {                                                            // (two waves per SIMD at most: 32-point spectra in registers)
            if (fast && core128_lds_bytes(pl, 8, true) <= room) return launch_core128_wpb<32, 16, true, 8, -1, true, RAGGED>();
            if (!fast && core128_lds_bytes(pl, 8, true) <= room) return launch_core128_wpb<32, 16, false, 8, -1, true, RAGGED>();
            if (!fast && core128_lds_bytes(pl, 6, true) <= room) return launch_core128_wpb<32, 16, false, 6, -1, true, RAGGED>();
            if (!fast && core128_lds_bytes(pl, 4, true) <= room) return launch_core128_wpb<32, 16, false, 4, -1, true, RAGGED>();
        }
        if (fast && fixed + 8 * per_wave <= room) return launch_core128_wpb<32, 16, true, 8, -1, false, RAGGED>();
        if (!fast && fixed + 8 * per_wave <= room) return launch_core128_wpb<32, 16, false, 8, -1, false, RAGGED>();
        if (!fast && fixed + 6 * per_wave <= room) return launch_core128_wpb<32, 16, false, 6, -1, false, RAGGED>();
        if (fast && fixed + 4 * per_wave <= room) return launch_core128_wpb<32, 16, true, 4, -1, false, RAGGED>();
        if (!fast && fixed + 4 * per_wave <= room) return launch_core128_wpb<32, 16, false, 4, -1, false, RAGGED>();
        if (!fast && fixed + 3 * per_wave <= room) return launch_core128_wpb<32, 16, false, 3, -1, false, RAGGED>();
        if (!fast && fixed + 2 * per_wave <= room) return launch_core128_wpb<32, 16, false, 2, -1, false, RAGGED>();
        if (fast && fixed + 2 * per_wave <= room) return launch_core128_wpb<32, 16, true, 2, -1, false, RAGGED>();
    }
    return Row{0, 0, false, 0, 0, false, false};         // (fail(HSSFSST_EUNSUPPORTED, "LDS request ... exceeds the 160 KiB budget"))
}

// launch_team16 from `G < 1` down to `lead + 1 > PSLOTS`: 0 = declined
struct Team { int ok, T, cpc_shift, nteams, grid, slots, lead; };
Team team16(int ngroups, int64_t batch, long long xstride, int team16_cus, int WPB, int DEPTH, int PSLOTS, int MS)
{
    const int kFusedMaxGroups = 128, kT16MaxCpc = 8;
    const Team no{0, 0, 0, 0, 0, 0, 0};
    const int G = ngroups;
    if (G < 1 || G > kFusedMaxGroups) return no;
    int T = 1;
    while ((WPB / 2) * T < G) T *= 2;
    if (T > team16_cus || T > 64) return no;
    int cpc = 1, cpc_shift = 0;
    while (cpc * T < G) { cpc *= 2; ++cpc_shift; }
    if (cpc > WPB || cpc > kT16MaxCpc || G / T < 1) return no;
    if (cpc < 4 && T > 1) return no;
    int nteams = team16_cus / T;
    if (batch < nteams) nteams = static_cast<int>(batch);
    const int grid = nteams * T;
    if ((batch + nteams - 1) / nteams > 65535) return no;
    if (xstride < 1 || xstride > 0x7fffffffLL || batch > 0x7fffffffLL) return no;
    const int held_pos = WPB * (DEPTH + 3);
    const int lead = (held_pos + G / T - 1) / (G / T) + 1;
    int slots = 8;
    while (slots < 2 * lead + 2) slots *= 2;
    if (slots > MS) return no;
    if (lead + 1 > PSLOTS) return no;
    return Team{1, T, cpc_shift, nteams, grid, slots, lead};
}

// launch_zscore
struct Z { int64_t zgrid; int slices; bool fused; };
Z zscore(int64_t batch)
{
    int64_t zgrid = 4096;
    int slices = 1;
    if (batch < 1024) {
        slices = static_cast<int>(1024 / batch);
        if (slices > 32) slices = 32;
    }
    if (zgrid > batch * slices) zgrid = batch * slices;
    const bool fused = slices == 1 && zgrid == batch && batch >= 512;
    return Z{zgrid, slices, fused};
}

// launch_dft's tile search (dft_wave_lds_floats of fsst_dft.hpp written out)
struct D { int G, waves; long long nitems, blocks; };
D dft(int nwin, int K, int ncols, int64_t batch)
{
    const int nk4 = (nwin + 3) / 4;
    auto wave_floats = [&](int g) { return ((16 * g + 4 * nk4 + 3) / 4) * 4 + 2 * 16 * g * ((K & 1) ? K : K + 1) + 4 + (4 + 3 * 256); };
    int G = 1, best_waves = -1;
    for (int cand = 4; cand >= 1; cand >>= 1) {
        const size_t pw = static_cast<size_t>(wave_floats(cand)) * sizeof(float);
        int w = static_cast<int>(static_cast<size_t>(kMaxLdsBytes) / pw);
        if (w > 8) w = 8;
        if (w < 1) continue;
        int per_cu = static_cast<int>(static_cast<size_t>(kMaxLdsBytes) / (pw * w)) * w;
        if (per_cu > 32) per_cu = 32;
        if (per_cu >= 16) { G = cand; best_waves = per_cu; break; }
        if (per_cu > best_waves) { G = cand; best_waves = per_cu; }
    }
    if (ncols <= 16) G = 1;
    const size_t per_wave = static_cast<size_t>(wave_floats(G)) * sizeof(float);
    int waves = static_cast<int>(static_cast<size_t>(kMaxLdsBytes) / per_wave);
    if (waves > 8) waves = 8;
    if (waves < 1) return D{G, 0, 0, 0};                 // (fail(HSSFSST_EUNSUPPORTED, ...))
    const int ntiles = (ncols + 16 * G - 1) / (16 * G);
    const long long nitems = static_cast<long long>(batch) * ntiles;
    long long blocks = (nitems + waves - 1) / waves;
    if (blocks > 256 * 64) blocks = 256 * 64;
    return D{G, waves, nitems, blocks};
}

}  // namespace parent

static bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

static long check_plain_choice()
{
    const char* name = "plain choice";
    long plans = 0, mfma = 0, rows_used[kCore128PlainRows] = {};
    for (int nwin : {128, 256, 512}) {
        const int nf = nwin / 2 + 1;
        for (int klo = 0; klo < nf; ++klo)
            for (int K = 1; K <= nf - klo; ++K)
                for (int stack = 0; stack < 2; ++stack) {
                    parent::Plan pp;
                    pp.nwin = nwin; pp.klo = klo; pp.K = K; pp.stack = stack != 0;
                    parent::make_facts(&pp);
                    const MfmaFacts f = mfma_facts(nwin, klo, K, stack != 0);
                    ++plans;
                    CHECK((f.rq != 0) == pp.mfma && f.fast == pp.fast, "nwin %d klo %d K %d stack %d: MFMA %d / %d", nwin, klo, K, stack, f.rq != 0, pp.mfma);
                    if (!pp.mfma) continue;
                    ++mfma;
                    CHECK(f.nt == pp.nt && f.rq == pp.rq && f.stripes03 == pp.stripes03 && f.lds_fixed == pp.lds_fixed && f.lds_per_wave == pp.lds_per_wave,
                          "nwin %d klo %d K %d stack %d: facts differ", nwin, klo, K, stack);
                    for (int wpb : {2, 3, 4, 6, 8, 16})
                        for (int pair = 0; pair < 2; ++pair)
                            CHECK(core128_lds_bytes(f, wpb, pair != 0) == parent::core128_lds_bytes(&pp, wpb, pair != 0), "lds bytes (%d, %d)", wpb, pair);
                    for (int no_pair = 0; no_pair < 2; ++no_pair) {
                        parent::g_no_pair = no_pair != 0;
                        const parent::Row want = parent::launch_core128_plain<false>(&pp);
                        const int got = core128_plain_row(f, no_pair != 0);
                        // every plan the facts call MFMA gets a row: the ladder's EUNSUPPORTED line is not reached
                        CHECK(want.ok && got >= 0, "nwin %d klo %d K %d stack %d no_pair %d: no row (ladder %d, table %d)", nwin, klo, K, stack, no_pair, want.ok, got);
                        if (!want.ok || got < 0) continue;
                        const Core128PlainRow& r = kCore128Plain[got];
                        CHECK(r.nt == want.nt && r.rq == want.rq && r.fast == want.fast && r.wpb == want.wpb && r.s1c == want.s1c && r.pair == want.pair,
                              "nwin %d klo %d K %d stack %d no_pair %d: row %d = <%d, %d, %d, %d, %d, %d>, the ladder ran <%d, %d, %d, %d, %d, %d>", nwin, klo, K,
                              stack, no_pair, got, r.nt, r.rq, r.fast, r.wpb, r.s1c, r.pair, want.nt, want.rq, want.fast, want.wpb, want.s1c, want.pair);
                        ++rows_used[got];
                    }
                }
    }
    std::printf("plain choice: %ld plans, %ld of them MFMA, each with a row, pairs on and off; rows no band takes (as in the ladder):", plans, mfma);
    for (int i = 0; i < kCore128PlainRows; ++i)
        if (rows_used[i] == 0) std::printf(" <%d, %d, %s, %d, %d%s>", kCore128Plain[i].nt, kCore128Plain[i].rq, kCore128Plain[i].fast ? "true" : "false",
                                           kCore128Plain[i].wpb, kCore128Plain[i].s1c, kCore128Plain[i].pair ? ", pairs" : "");
    std::printf("\n");
    return mfma;
}

static long check_team_geometry()
{
    const char* name = "team geometry";
    const int WPB = 16, DEPTH = 2;
    const int64_t batches[] = {1, 2, 15, 16, 17, 255, 256, 257, 1024, 65535 * 16, 65535 * 16 + 1};
    const int cus_list[] = {1, 8, 16, 64, 256, 304};
    const int ps_ms[][2] = {{32, 64}, {16, 64}, {16, 32}, {0, 32}};
    const long long strides[] = {0, 1, 2000, 1LL << 31};
    long accepted = 0, total = 0;
    for (int G = 0; G <= 130; ++G)
        for (int64_t batch : batches)
            for (int cus : cus_list)
                for (const auto& pm : ps_ms)
                    for (long long xs : strides) {
                        const int pslots = pm[0], ms = pm[1];
                        const parent::Team want = parent::team16(G, batch, xs, cus, WPB, DEPTH, pslots, ms);
                        const Team16Geometry g = team16_geometry(G, batch, xs, cus, WPB, DEPTH, pslots, ms);
                        ++total;
                        CHECK(g.ok == (want.ok != 0), "G %d batch %lld cus %d (%d, %d) stride %lld: accepted %d, inline %d", G, (long long)batch, cus, pslots, ms, xs, g.ok, want.ok);
                        if (!g.ok || !want.ok) continue;
                        ++accepted;
                        CHECK(g.T == want.T && g.cpc_shift == want.cpc_shift && g.nteams == want.nteams && g.grid == want.grid && g.slots == want.slots,
                              "G %d batch %lld cus %d (%d, %d): {%d, %d, %d, %d, %d}, inline {%d, %d, %d, %d, %d}", G, (long long)batch, cus, pslots, ms,
                              g.T, g.cpc_shift, g.nteams, g.grid, g.slots, want.T, want.cpc_shift, want.nteams, want.grid, want.slots);
                        // what fsst_team16.hpp "Progress" rests on, each on its own
                        const int cpc = 1 << g.cpc_shift;
                        const int lead = (WPB * (DEPTH + 3) + G / g.T - 1) / (G / g.T) + 1;      // signals a CU runs ahead of its oldest unresolved one
                        CHECK(pow2(g.T) && pow2(g.slots), "G %d: T %d, slots %d not powers of two", G, g.T, g.slots);
                        CHECK(cpc * g.T >= G, "G %d: cpc %d x T %d does not cover the signal", G, cpc, g.T);
                        CHECK(cpc <= WPB && cpc <= kT16MaxCpc, "G %d: cpc %d", G, cpc);
                        CHECK(g.T == 1 || cpc >= 4, "G %d: T %d with cpc %d (a CU publishes whole blocks of four groups)", G, g.T, cpc);
                        CHECK(g.grid == g.nteams * g.T && g.grid <= cus, "G %d cus %d: grid %d = %d x %d", G, cus, g.grid, g.nteams, g.T);
                        CHECK(g.nteams >= 1 && g.nteams <= batch, "G %d batch %lld: %d teams", G, (long long)batch, g.nteams);
                        CHECK((batch + g.nteams - 1) / g.nteams <= 65535, "G %d batch %lld: %d teams, too many signals per team", G, (long long)batch, g.nteams);
                        CHECK(g.slots >= 2 * lead + 2, "G %d: slots %d < 2 x %d + 2", G, g.slots, lead);
                        CHECK(g.slots <= ms, "G %d: slots %d > %d", G, g.slots, ms);
                        CHECK(lead + 1 <= pslots, "G %d: lead %d + 1 > %d", G, lead, pslots);
                    }
    std::printf("team geometry: %ld shapes, %ld accepted, all as the inline arithmetic and within the kernel's progress conditions\n", total, accepted);
    return accepted;
}

// the chunks of one signal, from its regions: {first group, groups}
static std::vector<std::pair<int, int>> chunks_of(const Core128Regions& r, int ngroups)
{
    std::vector<std::pair<int, int>> out;
    for (int rg = 0; rg < 3; ++rg)
        for (int c = 0; c < r.npc[rg]; ++c) {
            const int g0 = r.g0[rg] + c * r.gpc[rg];
            out.push_back({g0, std::min(r.gpc[rg], ngroups - g0)});
        }
    return out;
}

static void check_chunks()
{
    const char* name = "chunk patterns";
    for (int ngroups = 1; ngroups <= 4200; ++ngroups)
        for (long long nsig : {-1LL, 1LL, 64LL}) {
            const Core128Regions r = core128_regions(ngroups, nsig);
            const auto ch = chunks_of(r, ngroups);
            CHECK(static_cast<int>(ch.size()) == core128_chunks_per_signal(r), "%d groups: %zu chunks, %d counted", ngroups, ch.size(), core128_chunks_per_signal(r));
            int next = 0;                                // regions follow each other and chunks are in order within one: exactly once
            for (const auto& c : ch) {
                CHECK(c.first == next && c.second >= 1, "%d groups, nsig %lld: chunk at %d (%d groups), expected at %d", ngroups, nsig, c.first, c.second, next);
                next = c.first + c.second;
            }
            CHECK(next == ngroups, "%d groups, nsig %lld: chunks end at %d", ngroups, nsig, next);
        }
    std::vector<std::vector<int>> lists;
    lists.push_back({1});
    lists.push_back(std::vector<int>(16, 125));
    std::vector<int> rnd;
    unsigned long long s = 0x9e3779b97f4a7c15ull;
    for (int i = 0; i < 1000; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        rnd.push_back(1 + static_cast<int>((s >> 33) % ((i % 7 == 0) ? 4200 : 300)));
    }
    lists.push_back(rnd);
    for (const auto& ng : lists) {
        std::vector<RaggedChunk> got;
        core128_ragged_chunks(ng.data(), static_cast<long long>(ng.size()), got);
        std::vector<std::vector<std::pair<int, int>>> per(ng.size());
        for (const RaggedChunk& c : got) {
            CHECK(c.sig >= 0 && c.sig < static_cast<int>(ng.size()), "signal %d of %zu", c.sig, ng.size());
            if (c.sig < 0 || c.sig >= static_cast<int>(ng.size())) continue;
            const int g0 = c.groups & ((1 << kRaggedGroupBits) - 1), n = (c.groups >> kRaggedGroupBits) + 1;
            per[c.sig].push_back({g0, n});
        }
        // the list's order: region 0 of every signal, then region 1, then region 2, signals in list order within a region
        size_t at = 0;
        for (int rg = 0; rg < 3; ++rg)
            for (size_t i = 0; i < ng.size(); ++i) {
                const Core128Regions r = core128_regions(ng[i], 1);
                for (int c = 0; c < r.npc[rg]; ++c, ++at) {
                    CHECK(at < got.size() && got[at].sig == static_cast<int>(i) && (got[at].groups & ((1 << kRaggedGroupBits) - 1)) == r.g0[rg] + c * r.gpc[rg],
                          "list of %zu: entry %zu is not region %d chunk %d of signal %zu", ng.size(), at, rg, c, i);
                }
            }
        CHECK(at == got.size(), "list of %zu: %zu entries, %zu expected", ng.size(), got.size(), at);
        for (size_t i = 0; i < ng.size(); ++i) {         // per signal: the chunks it gets alone (in region order = ascending groups)
            const auto alone = chunks_of(core128_regions(ng[i], 1), ng[i]);
            CHECK(per[i] == alone, "list of %zu: signal %zu (%d groups) is not cut as alone", ng.size(), i, ng[i]);
        }
    }
    std::printf("chunk patterns: 1 .. 4200 groups x nsig {-1, 1, 64} cover every group once, in order; ragged lists of 1, 16 and 1000 signals cut each as alone, by region\n");
}

static void check_small_rules()
{
    const char* name = "small rules";
    for (int64_t batch = 1; batch <= 5000; ++batch) {
        const parent::Z want = parent::zscore(batch);
        const ZscoreShape z = zscore_shape(batch);
        CHECK(z.grid == want.zgrid && z.slices == want.slices && z.fused == want.fused, "z-score, batch %lld", (long long)batch);
    }
    long unsupported = 0;
    for (int nwin = 1; nwin <= 1000; ++nwin)
        for (int K : {1, 22, nwin / 2 + 1})
            for (int ncols : {1, 16, 17, 400, 2000})
                for (int64_t batch : {int64_t(1), int64_t(2), int64_t(1024)}) {
                    const parent::D want = parent::dft(nwin, K, ncols, batch);
                    const DftShape d = dft_shape((nwin + 3) / 4, K, ncols, batch);
                    CHECK(d.G == want.G && d.waves == want.waves && d.nitems == want.nitems && d.blocks == want.blocks,
                          "tile search, nwin %d K %d ncols %d batch %lld: {%d, %d, %lld}, inline {%d, %d, %lld}", nwin, K, ncols, (long long)batch,
                          d.G, d.waves, d.blocks, want.G, want.waves, want.blocks);
                    unsupported += d.waves < 1;
                }
    // the 88 % rule against its inline form (launch_fused, launch_canon_fused_band)
    for (int64_t grid : {int64_t(1), int64_t(8), int64_t(64), int64_t(256), int64_t(304)})
        for (int64_t batch = 1; batch <= 2000; ++batch) {
            const int64_t rounds = (batch + grid - 1) / grid;
            const bool declined = batch < grid || rounds * grid * 100 > batch * 112;
            CHECK(fused_rounds_full(batch, grid) == !declined, "88 %% rule, batch %lld grid %lld", (long long)batch, (long long)grid);
        }
    // the canonical kernels' bytes against the sum written out in the launchers
    for (int ctl : {208, 2336, 3000})
        for (int wf : {1400, 2146, 2210})
            CHECK(canon_lds_bytes(ctl, wf) == (static_cast<size_t>(16 * 64 * 4 + 4 * 128 + 4 * 33 * 2) + ctl + size_t(16) * wf) * sizeof(float), "canon bytes (%d, %d)", ctl, wf);
    std::printf("small rules: z-score rule for batch 1 .. 5000, tile search for nwin 1 .. 1000 x K {1, 22, nf} (%ld shapes without room for a wave), "
                "the 88 %% rule and the canonical kernels' bytes as their inline forms\n", unsupported);
}

int main()
{
    const long mfma = check_plain_choice();
    const long accepted = check_team_geometry();
    check_chunks();
    check_small_rules();
    if (mfma < 1000 || accepted < 1000) { std::printf("FAIL: the sweeps were empty (%ld MFMA plans, %ld geometries)\n", mfma, accepted); ++failures; }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("launch shape ok\n");
    return 0;
}
