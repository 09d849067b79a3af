// Stand-alone check of the device resampler's host arithmetic (csrc/fourier_resample_layout.hpp: host only, no HIP): the plan of a
// ragged call against the loop that stood inline in hssfsst_resample_exec_ragged, the dense chunk rule and the Bluestein tables.
// Built with -fsanitize=address,undefined by tests/test_resample_ragged.py.  Any failed property or sanitizer report ends the run
// non-zero.
#include "fourier_resample_layout.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

namespace rl = hssfsst::rslayout;
using hssfsst::RaggedResampleSig;

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } \
    } while (0)

// the plan as hssfsst_resample_exec_ragged made it inline before the planner was a function
struct Inline {
    struct Chunk { long long d0, cnt, Mw, t0, ntab, elems; };
    std::vector<Chunk> chunks;
    std::vector<long long> ord, tabM, tabOff, tabN;
    std::vector<int> M1s;
    std::vector<unsigned char> desc;                                 // RaggedResampleSig[count] | table lengths
    int Mt = 0;
    long long max_elems = 0;
};

static Inline inline_loop(const std::vector<int64_t>& starts, const std::vector<int64_t>& lens, int M2, long long xlo, long long budget)
{
    Inline r;
    const int64_t count = static_cast<int64_t>(lens.size());
    r.ord.resize(static_cast<size_t>(count));
    for (int64_t i = 0; i < count; ++i) r.ord[static_cast<size_t>(i)] = i;
    std::stable_sort(r.ord.begin(), r.ord.end(), [&](long long a, long long b) { return lens[a] < lens[b]; });
    r.M1s.resize(static_cast<size_t>(count));
    for (int64_t i = 0; i < count; ++i) {
        int m = 1;
        while (m < 2 * lens[r.ord[static_cast<size_t>(i)]] - 1) m <<= 1;
        r.M1s[static_cast<size_t>(i)] = m;
    }
    Inline::Chunk c{0, 0, 0, 0, 0, 0};
    long long tab_elems = 0;
    for (long long d = 0; d < count; ++d) {
        const long long n = lens[r.ord[static_cast<size_t>(d)]], M1 = r.M1s[static_cast<size_t>(d)];
        const long long Mw = std::max<long long>(M1, M2);
        bool fresh = c.cnt == 0 || n != lens[r.ord[static_cast<size_t>(d - 1)]];
        if (c.cnt > 0 && (c.cnt + 1) * Mw + tab_elems + (fresh ? M1 : 0) > budget) {
            c.elems = c.cnt * c.Mw + tab_elems;
            r.chunks.push_back(c);
            c = Inline::Chunk{d, 0, 0, static_cast<long long>(r.tabN.size()), 0, 0};
            tab_elems = 0;
            fresh = true;
        }
        if (fresh) {
            r.tabN.push_back(n); r.tabM.push_back(M1); r.tabOff.push_back(tab_elems);
            tab_elems += M1;
            ++c.ntab;
        }
        ++c.cnt;
        c.Mw = Mw;
    }
    c.elems = c.cnt * c.Mw + tab_elems;
    r.chunks.push_back(c);
    const size_t sig_bytes = static_cast<size_t>(count) * sizeof(RaggedResampleSig);
    r.desc.resize(sig_bytes + r.tabN.size() * sizeof(long long));    // exactly sized: a write past the end is a report
    auto* sig = reinterpret_cast<RaggedResampleSig*>(r.desc.data());
    for (const Inline::Chunk& ch : r.chunks) {
        long long u = ch.t0 - 1;
        for (long long d = ch.d0; d < ch.d0 + ch.cnt; ++d) {
            const long long i = r.ord[static_cast<size_t>(d)];
            if (d == ch.d0 || lens[i] != lens[r.ord[static_cast<size_t>(d - 1)]]) ++u;
            sig[d] = RaggedResampleSig{starts[i] - xlo, lens[i], r.M1s[static_cast<size_t>(d)], r.tabOff[static_cast<size_t>(u)], i};
        }
    }
    std::memcpy(r.desc.data() + sig_bytes, r.tabN.data(), r.tabN.size() * sizeof(long long));
    r.Mt = M2;
    for (int m : r.M1s) r.Mt = std::max(r.Mt, m);
    for (const Inline::Chunk& ch : r.chunks) r.max_elems = std::max(r.max_elems, ch.elems);
    return r;
}

// one_each: the budget is below one signal's work, so every chunk holds exactly one signal
static void run_case(const char* name, const std::vector<int64_t>& lens, int64_t num, long long budget, bool one_each = false)
{
    const int64_t count = static_cast<int64_t>(lens.size());
    const long long xlo = 5;                                         // a host call stages x from its lowest start on
    std::vector<int64_t> starts(lens.size());                        // packed back to back behind xlo, in list order
    long long at = xlo;
    for (size_t i = 0; i < lens.size(); ++i) { starts[i] = at; at += lens[i]; }
    const int M2 = rl::pow2_at_least(2 * num - 1);
    rl::RaggedPlan p;
    CHECK(rl::plan_ragged(starts.data(), lens.data(), count, M2, xlo, budget, p), "the planner ran out of memory");
    const Inline want = inline_loop(starts, lens, M2, xlo, budget);

    // equal to the inline loop: chunks, tables, offsets, descriptors, Mt, max_elems
    CHECK(p.chunks.size() == want.chunks.size(), "%zu chunks, the inline loop made %zu", p.chunks.size(), want.chunks.size());
    for (size_t c = 0; c < p.chunks.size() && c < want.chunks.size(); ++c) {
        const rl::Chunk& g = p.chunks[c];
        const Inline::Chunk& w = want.chunks[c];
        CHECK(g.d0 == w.d0 && g.cnt == w.cnt && g.Mw == w.Mw && g.t0 == w.t0 && g.ntab == w.ntab && g.elems == w.elems,
              "chunk %zu: {%lld, %lld, %lld, %lld, %lld, %lld}, the inline loop made {%lld, %lld, %lld, %lld, %lld, %lld}", c, g.d0, g.cnt, g.Mw,
              g.t0, g.ntab, g.elems, w.d0, w.cnt, w.Mw, w.t0, w.ntab, w.elems);
    }
    CHECK(p.tabs.size() == want.tabN.size(), "%zu tables, the inline loop made %zu", p.tabs.size(), want.tabN.size());
    for (size_t u = 0; u < p.tabs.size() && u < want.tabN.size(); ++u)
        CHECK(p.tabs[u].n == want.tabN[u] && p.tabs[u].M == want.tabM[u] && p.tabs[u].off == want.tabOff[u], "table %zu: {%lld, %lld, %lld}", u,
              p.tabs[u].n, p.tabs[u].M, p.tabs[u].off);
    CHECK(p.Mt == want.Mt && p.max_elems == want.max_elems, "Mt %d, max_elems %lld; the inline loop made %d, %lld", p.Mt, p.max_elems, want.Mt,
          want.max_elems);
    CHECK(p.sig.size() == static_cast<size_t>(count) && p.sig_bytes() == static_cast<size_t>(count) * sizeof(RaggedResampleSig), "descriptor count");
    CHECK(p.desc_bytes() == want.desc.size(), "%zu descriptor bytes, the inline loop made %zu", p.desc_bytes(), want.desc.size());
    std::vector<unsigned char> block(p.desc_bytes());                // exactly sized
    rl::write_descriptors(p, block.data());
    CHECK(block.size() == want.desc.size() && std::memcmp(block.data(), want.desc.data(), block.size()) == 0, "descriptor block differs");
    if (p.sig.size() != static_cast<size_t>(count) || p.desc_bytes() != want.desc.size()) return;
    const auto* sig = reinterpret_cast<const RaggedResampleSig*>(block.data());
    const auto* tn = reinterpret_cast<const long long*>(block.data() + p.sig_bytes());
    for (int64_t d = 0; d < count; ++d)
        CHECK(sig[d].row == want.ord[static_cast<size_t>(d)] && sig[d].M1 == want.M1s[static_cast<size_t>(d)], "sorted position %lld", static_cast<long long>(d));

    // every signal in exactly one chunk; the sort is by length and stable
    std::vector<int> seen(lens.size(), 0);
    long long next = 0, next_tab = 0;
    for (const rl::Chunk& ch : p.chunks) {
        CHECK(ch.d0 == next && ch.cnt >= 1 && ch.t0 == next_tab && ch.ntab >= 1, "chunk at %lld (%lld signals), expected at %lld", ch.d0, ch.cnt, next);
        next = ch.d0 + ch.cnt;
        next_tab = ch.t0 + ch.ntab;
        for (long long d = ch.d0; d < ch.d0 + ch.cnt && d < count; ++d)
            if (sig[d].row >= 0 && sig[d].row < count) ++seen[static_cast<size_t>(sig[d].row)];
    }
    CHECK(next == count && next_tab == static_cast<long long>(p.tabs.size()), "chunks end at signal %lld of %lld, table %lld of %zu", next,
          static_cast<long long>(count), next_tab, p.tabs.size());
    for (size_t i = 0; i < seen.size(); ++i) CHECK(seen[i] == 1, "signal %zu lies in %d chunks", i, seen[i]);
    for (int64_t d = 1; d < count; ++d)
        CHECK(sig[d - 1].n < sig[d].n || (sig[d - 1].n == sig[d].n && sig[d - 1].row < sig[d].row), "sorted positions %lld, %lld out of order",
              static_cast<long long>(d - 1), static_cast<long long>(d));

    // a chunk: within the budget unless it holds one signal; a uniform stride that fits every signal and the inverse side; its
    // tables back to back behind the work; each descriptor's table that of its own n, its row its list index, its start from xlo
    for (const rl::Chunk& ch : p.chunks) {
        CHECK(ch.elems <= budget || ch.cnt == 1, "chunk at %lld: %lld elements of %lld signals exceed %lld", ch.d0, ch.elems, ch.cnt, budget);
        CHECK(!one_each || ch.cnt == 1, "chunk at %lld holds %lld signals under a budget below one signal's work", ch.d0, ch.cnt);
        long long off = 0;
        for (long long u = ch.t0; u < ch.t0 + ch.ntab; ++u) {
            const rl::Table& t = p.tabs[static_cast<size_t>(u)];
            CHECK(t.off == off && t.M == rl::pow2_at_least(2 * t.n - 1) && tn[u] == t.n, "table %lld of the chunk at %lld", u, ch.d0);
            CHECK(u == ch.t0 || p.tabs[static_cast<size_t>(u - 1)].n < t.n, "table %lld repeats a length of its chunk", u);
            off += t.M;
        }
        CHECK(ch.elems == ch.cnt * ch.Mw + off, "chunk at %lld: %lld elements", ch.d0, ch.elems);
        for (long long d = ch.d0; d < ch.d0 + ch.cnt; ++d) {
            const RaggedResampleSig& s = sig[d];
            const size_t i = static_cast<size_t>(s.row);
            CHECK(s.n == lens[i] && s.start == starts[i] - xlo && s.M1 == rl::pow2_at_least(2 * s.n - 1), "descriptor %lld", d);
            CHECK(s.M1 <= ch.Mw && M2 <= ch.Mw, "descriptor %lld: M1 %lld, M2 %d, stride %lld", d, s.M1, M2, ch.Mw);
            bool found = false;
            for (long long u = ch.t0; u < ch.t0 + ch.ntab; ++u)
                found = found || (p.tabs[static_cast<size_t>(u)].n == s.n && p.tabs[static_cast<size_t>(u)].off == s.tab);
            CHECK(found, "descriptor %lld: no table of its chunk has length %lld at offset %lld", d, s.n, s.tab);
        }
    }
    std::printf("%-28s %5lld signals -> num %6lld: %3zu chunks, %4zu tables, Mt %d\n", name, static_cast<long long>(count), static_cast<long long>(num),
                p.chunks.size(), p.tabs.size(), p.Mt);
}

// the dense large tier's chunk as it stood inline in hssfsst_resample_exec
static void run_dense(long long Mw, long long batch)
{
    const char* name = "dense chunk";
    const size_t bytes = rl::kRsWorkBytes;
    const long long per = static_cast<long long>(bytes / (static_cast<size_t>(Mw) * 16));
    const long long want = per < 1 ? 1 : (per < batch ? per : batch);
    const long long got = rl::dense_chunk(static_cast<long long>(bytes / 16), Mw, batch);
    CHECK(got == want && got >= 1 && got <= batch, "Mw %lld, batch %lld: %lld signals, the inline rule gave %lld", Mw, batch, got, want);
}

// c and B of an N-point DFT against their definitions: c = conj(w), and the convolution they stand for reproduces a direct DFT
static void run_tables(int64_t N)
{
    char name[48];
    std::snprintf(name, sizeof(name), "bluestein N=%lld", static_cast<long long>(N));
    using hssfsst::resample_detail::cd;
    const int M = rl::pow2_at_least(2 * N - 1);
    std::vector<cd> c(static_cast<size_t>(N)), B(static_cast<size_t>(M));   // exactly sized
    rl::bluestein_tables(N, M, 1.0, c.data(), B.data());
    CHECK(M >= 2 * N - 1 && (M & (M - 1)) == 0 && (M == 1 || M / 2 < 2 * N - 1), "M = %d", M);
    double worst = 0.0;
    for (int64_t m = 0; m < N; ++m) {
        const double ang = M_PI * static_cast<double>((m * m) % (2 * N)) / static_cast<double>(N);
        worst = std::max(worst, std::abs(c[static_cast<size_t>(m)] - cd(std::cos(ang), -std::sin(ang))));
    }
    CHECK(worst == 0.0, "chirp off by %g", worst);
    // B in natural order times M is the FFT of the wrapped chirp: its inverse DFT at point 0 is w[0] = 1, so sum_j B[j] = 1
    cd sum(0.0, 0.0);
    for (const cd& v : B) sum += v;
    CHECK(std::abs(sum - cd(1.0, 0.0)) <= 1e-12 * std::sqrt(static_cast<double>(M)), "sum of B = (%g, %g)", sum.real(), sum.imag());
    for (const cd& v : B) CHECK(std::isfinite(v.real()) && std::isfinite(v.imag()), "a non-finite B");
    std::printf("%-28s M %d\n", name, M);
}

int main()
{
    const long long lib = static_cast<long long>(rl::kRsWorkBytes / 16);     // the library's budget, in complex fp64 elements
    const std::vector<int64_t> one{1}, equal16(16, 3000);
    const std::vector<int64_t> mixed{1, 2, 3, 127, 128, 129, 2000, 4096, 4097, 8191, 35500, 60001, 240000, 2000, 129, 35500, 1};   // the test file's LENS
    std::vector<int64_t> many(1000);
    unsigned long long x = 0x9e3779b97f4a7c15ull;
    for (int64_t& v : many) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        v = 1 + static_cast<int64_t>((x >> 33) % 70000);
    }
    many[17] = many[500] = many[999];                                // repeated lengths, far apart in the list
    struct { const char* name; const std::vector<int64_t>* lens; } lists[] = {{"one", &one}, {"equal16", &equal16}, {"mixed17", &mixed}, {"random1k", &many}};
    for (const auto& l : lists)
        for (int64_t num : {int64_t(1), int64_t(1000), int64_t(20000)}) {
            char name[64];
            std::snprintf(name, sizeof(name), "%s library budget", l.name);
            run_case(name, *l.lens, num, lib);
            std::snprintf(name, sizeof(name), "%s 64 Ki elements", l.name);      // several chunks on the small lists
            run_case(name, *l.lens, num, 1 << 16);
            std::snprintf(name, sizeof(name), "%s 3 Mi elements", l.name);
            run_case(name, *l.lens, num, 3 << 20);
            std::snprintf(name, sizeof(name), "%s budget 1", l.name);            // below any signal's work: one signal per chunk
            run_case(name, *l.lens, num, 1, true);
        }
    for (long long Mw : {16384LL, 131072LL, 1LL << 24, 1LL << 25, 1LL << 27})
        for (long long batch : {1LL, 2LL, 7LL, 1024LL, 100000LL}) run_dense(Mw, batch);
    for (int64_t N : {1, 2, 3, 5, 64, 4097}) run_tables(N);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("resample layout ok\n");
    return 0;
}
