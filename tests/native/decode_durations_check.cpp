// Stand-alone check of the explicit-duration decoder's arithmetic and geometry (csrc/decode_durations_layout.hpp: host only, no
// HIP), built with -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_decode_durations.py.  decode_ring() below
// is the kernel of csrc/segmenter_decode_durations.hpp with its lanes simulated: the same functions, the same ring of D + 1 slots
// that is never cleared (it starts poisoned here), the same owner of every (state, duration), the same first-writer rule, the quantised
// tables in the workspace's layout, the backpointer bytes kept in the path itself and the durations in a workspace, the
// backtrace in rounds of kLanes runs.  It must equal decode_durations_reference(), the sequential pull loop, in every state and
// in the score.  Any failed property or sanitizer report ends the run non-zero.
#include "decode_durations_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

namespace ul = hssfsst::durlayout;
using ul::i64;

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } \
    } while (0)

static i64 decode_ring(const float* e, int T, const float* Af, const float* pif, const float* durf, const float* edgef, int D, uint8_t* path)
{
    const ul::Tables tb = ul::quantise_tables(Af, pif);
    const int R = ul::ring_slots(D);
    std::vector<i64> table(static_cast<size_t>(ul::table_words(D)), 12345);            // exactly sized, as the fill launches fill it
    for (int s = 0; s < 8 * D; ++s) table[static_cast<size_t>(ul::table_index_of_source(s, D))] = ul::quantise(s < 4 * D ? durf[s] : edgef[s - 4 * D]);
    std::vector<i64> cand(4 * static_cast<size_t>(ul::kMaxRing), 777);                 // the kernel's size; poisoned: the first writer must overwrite
    std::vector<uint16_t> argd(4 * static_cast<size_t>(ul::kMaxRing), 60000);
    std::vector<uint16_t> back(4 * static_cast<size_t>(T), 0);
    auto C_of = [&](int slot, i64 C[4]) { for (int j = 0; j < 4; ++j) C[j] = cand[static_cast<size_t>(j) * ul::kMaxRing + slot]; };

    i64 E[4] = {0, 0, 0, 0};
    int cur = 0;
    for (int t = 0; t < T; ++t) {
        i64 B[4];
        if (t == 0) {
            for (int j = 0; j < 4; ++j) B[j] = tb.pi[j];
        } else {
            i64 C[4];
            C_of(cur, C);
            unsigned four = 0;                           // lanes 0 .. 3 leave their state's predecessor as a byte each
            for (int tid = 0; tid < 4; ++tid) {
                const int j = ul::lane_state(tid);
                const i64 Acol[4] = {tb.A[0][j], tb.A[1][j], tb.A[2][j], tb.A[3][j]};
                unsigned pre;
                B[j] = ul::run_start(C, E, Acol, j, &pre);
                four |= pre << (8 * j);
            }
            path[t] = static_cast<uint8_t>(ul::pack_states(four));
            i64 B4[4];
            if (path[t] != ul::run_starts(C, E, tb, B4) || B4[0] != B[0] || B4[1] != B[1] || B4[2] != B[2] || B4[3] != B[3]) {
                std::printf("FAIL run_start: step %d\n", t);
                ++failures;
            }
            for (int j = 0; j < 4; ++j) back[4 * static_cast<size_t>(t) + j] = argd[static_cast<size_t>(j) * ul::kMaxRing + cur];
        }
        const bool bulk = t > 0 && t + D < T;            // every target before T: the kernel's path without a branch
        for (int tid = ul::kLanes - 1; tid >= 0; --tid)                                 // (any lane order: distinct words)
            for (int k = 0; k < ul::kPerLane; ++k) {
                const int d = ul::lane_duration(tid, k), j = ul::lane_state(tid);
                if (bulk) {                              // reads its word and writes it or the candidate back, whatever d
                    if (ul::lane_duration(0, k / 4 * 4) > D) continue;   // (the kernel leaves a chunk of four nobody owns)
                    const int slot = ul::bulk_slot(cur, d, D, R);
                    const i64 c = ul::add(B[j], d <= D ? table[static_cast<size_t>(ul::table_index(0, d, j, D))] : ul::kNeg);
                    i64& held = cand[static_cast<size_t>(j) * ul::kMaxRing + slot];
                    uint16_t& harg = argd[static_cast<size_t>(j) * ul::kMaxRing + slot];
                    const bool w = d == D || ul::takes(c, held);
                    held = w ? c : held;
                    harg = w ? static_cast<uint16_t>(d) : harg;
                    continue;
                }
                if (!(d <= D && t + d <= T)) continue;
                const int which = (t == 0 || t + d == T) ? 1 : 0;
                const int slot = ul::ring_slot(cur, d, R);
                const i64 c = ul::add(B[j], table[static_cast<size_t>(ul::table_index(which, d, j, D))]);
                i64& held = cand[static_cast<size_t>(j) * ul::kMaxRing + slot];
                if (t == 0 || d == D || ul::takes(c, held)) {
                    held = c;
                    argd[static_cast<size_t>(j) * ul::kMaxRing + slot] = static_cast<uint16_t>(d);
                }
            }
        for (int j = 0; j < 4; ++j) E[j] += ul::quantise_emission(e[4 * static_cast<size_t>(t) + j]);
        cur = cur + 1 == R ? 0 : cur + 1;
    }
    i64 C[4], score;
    C_of(cur, C);
    const unsigned s_end = ul::end_state(C, E, &score);
    if (score == ul::kNeg) {
        for (int u = 0; u < T; ++u) path[u] = 0;
        return score;
    }
    int t = T, s = static_cast<int>(s_end), d = argd[static_cast<size_t>(s_end) * ul::kMaxRing + cur];
    std::vector<int> runs(3 * ul::kLanes);
    for (;;) {
        int n = 0;
        while (n < ul::kLanes && t > 0) {
            if (d < 1 || d > t) { std::printf("FAIL backtrace: duration %d at boundary %d\n", d, t); ++failures; return score; }
            runs[3 * n] = t - d; runs[3 * n + 1] = d; runs[3 * n + 2] = s;
            ++n;
            t -= d;
            if (t > 0) {
                s = (path[t] >> (2 * s)) & 3;
                d = back[4 * static_cast<size_t>(t) + s];
            }
        }
        for (int r = 0; r < n; ++r)
            for (int u = 0; u < runs[3 * r + 1]; ++u) path[runs[3 * r] + u] = static_cast<uint8_t>(runs[3 * r + 2]);
        if (t == 0) break;
    }
    return score;
}

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<unsigned>(rng_state >> 33);
}
static float rnd_logp() { return -static_cast<float>(rnd() % 100000) / 8192.0f - 1e-3f; }

static const float NINF = -std::numeric_limits<float>::infinity();
static const float kCyclic[16] = {0, 0, NINF, NINF, NINF, 0, 0, NINF, NINF, NINF, 0, 0, 0, NINF, NINF, 0};
static const float kUniform[4] = {0, 0, 0, 0};
static const float kState0[4] = {0, NINF, NINF, NINF};

static void run_case(const char* name, const std::vector<float>& e, const float* A, const float* pi, const std::vector<float>& dur,
                     const std::vector<float>& edge, int D, bool expect_neg = false)
{
    const int T = static_cast<int>(e.size() / 4);
    std::vector<uint8_t> want(static_cast<size_t>(T)), got(static_cast<size_t>(T), 255);   // exactly sized
    const i64 sw = ul::decode_durations_reference(e.data(), T, A, pi, dur.data(), edge.data(), D, want.data());
    const i64 sg = decode_ring(e.data(), T, A, pi, dur.data(), edge.data(), D, got.data());
    CHECK(sw == sg, "T %d D %d: score %lld, reference %lld", T, D, sg, sw);
    CHECK((sw == ul::kNeg) == expect_neg, "T %d D %d: score %lld", T, D, sw);
    int bad = -1;
    for (int t = 0; t < T && bad < 0; ++t)
        if (want[t] != got[t]) bad = t;
    CHECK(bad < 0, "T %d D %d: state differs at step %d (%d, reference %d)", T, D, bad, got[bad < 0 ? 0 : bad], want[bad < 0 ? 0 : bad]);
    if (sw != ul::kNeg) {                                // the reference's own path: runs of at most D steps, allowed moves only
        int run = 1;
        for (int t = 1; t <= T; ++t) {
            if (t < T && want[t] == want[t - 1]) { ++run; continue; }
            CHECK(run <= D, "a run of %d steps ends at %d, D %d", run, t, D);
            if (t < T) CHECK(ul::quantise(A[4 * want[t - 1] + want[t]]) != ul::kNeg, "forbidden move at %d", t);
            run = 1;
        }
    }
}

// (4, D) tables: random scores, every duration below `dmin` forbidden, `holes` in 8 of the rest forbidden too
static std::vector<float> table(int D, int dmin, int holes)
{
    std::vector<float> t(4 * static_cast<size_t>(D));
    for (int j = 0; j < 4; ++j)
        for (int d = 1; d <= D; ++d)
            t[static_cast<size_t>(j) * D + d - 1] = (d < dmin && d < D) || (d < D && static_cast<int>(rnd() % 8) < holes) ? NINF : rnd_logp();
    return t;
}

int main()
{
    const char* name = "constants";
    CHECK(ul::kMaxSteps == (i64(1) << 24) && ul::kMaxDuration == 2048 && ul::kLanes * ul::kPerLane == 4 * ul::kMaxDuration, "limits");
    CHECK((4 * ul::kMaxSteps + 3) * hssfsst::declayout::kMaxTerm < (i64(1) << 62), "the bound is not below 2^62");
    CHECK(ul::quantise_emission(NINF) == -hssfsst::declayout::kMaxTerm, "qe(-inf)");
    CHECK(ul::quantise_emission(std::numeric_limits<float>::quiet_NaN()) == -hssfsst::declayout::kMaxTerm, "qe(NaN)");
    CHECK(ul::quantise_emission(-1.5f) == ul::quantise(-1.5f) && ul::quantise_emission(-NINF) == hssfsst::declayout::kMaxTerm, "qe");
    CHECK(!ul::takes(ul::kNeg, ul::kNeg) && ul::takes(5, 5) && !ul::takes(4, 5) && ul::takes(-7, ul::kNeg), "takes");
    for (unsigned b = 0; b < 256; ++b)
        CHECK(ul::pack_states((b & 3u) | ((b >> 2) & 3u) << 8 | ((b >> 4) & 3u) << 16 | ((b >> 6) & 3u) << 24) == b, "pack_states %u", b);
    {   // every duration of every state has one owner; the table's two index functions agree and fill it exactly
        std::vector<int> owners(4 * (ul::kMaxDuration + 1), 0);
        for (int l = 0; l < ul::kLanes; ++l)
            for (int k = 0; k < ul::kPerLane; ++k) ++owners[static_cast<size_t>(4 * ul::lane_duration(l, k) + ul::lane_state(l))];
        for (int w = 4; w < 4 * (ul::kMaxDuration + 1); ++w) CHECK(owners[static_cast<size_t>(w)] == 1, "duration %d of state %d has %d owners", w / 4, w % 4, owners[static_cast<size_t>(w)]);
        for (int D : {1, 3, 257}) {
            std::vector<int> hit(static_cast<size_t>(ul::table_words(D)), 0);
            for (int s = 0; s < 8 * D; ++s) ++hit[static_cast<size_t>(ul::table_index_of_source(s, D))];
            for (int h : hit) CHECK(h == 1, "table of D %d: a word filled %d times", D, h);
            CHECK(ul::table_index_of_source(4 * D + 2 * D + (D - 1), D) == ul::table_index(1, D, 2, D), "edge[2][D - 1]");
        }
    }

    float dense[16];
    for (float& v : dense) v = rnd_logp();
    for (int D : {1, 2, 5, 255, 256, 257, 700}) {
        const int R = ul::ring_slots(D);
        for (int T : {1, 2, D - 1, D, D + 1, 2 * R + 3}) {
            if (T < 1) continue;
            std::vector<float> e(4 * static_cast<size_t>(T));
            for (int kind = 0; kind < 3; ++kind) {
                for (float& v : e) v = kind == 0 ? rnd_logp() : kind == 1 ? 0.0f : -static_cast<float>(rnd() % 4);
                name = kind == 0 ? "random emissions" : kind == 1 ? "all-equal emissions" : "emissions in {-3..0}";
                for (int dmin : {1, 40}) {
                    const std::vector<float> dur = table(D, dmin, kind), edge = table(D, 1, 0);
                    run_case(name, e, kCyclic, kUniform, dur, edge, D);
                    run_case(name, e, dense, kState0, dur, edge, D);
                }
                if (kind == 1) {                         // all-equal tables too: every comparison is a tie
                    const std::vector<float> flat(4 * static_cast<size_t>(D), 0.0f);
                    run_case("all ties", e, kCyclic, kUniform, flat, flat, D);
                }
            }
        }
    }
    {   // special emissions; a recording nothing fits
        name = "special values";
        const int D = 9, T = 50;
        std::vector<float> e(4 * static_cast<size_t>(T));
        for (float& v : e) v = rnd_logp();
        for (int j = 0; j < 4; ++j) e[4 * 10 + j] = std::numeric_limits<float>::quiet_NaN();
        e[4 * 20 + 1] = NINF;
        e[4 * 30 + 2] = -NINF;
        e[4 * 31 + 3] = 1e6f;
        for (int j = 0; j < 4; ++j) e[4 * 40 + j] = NINF;
        const std::vector<float> dur = table(D, 1, 2);
        run_case(name, e, dense, kUniform, dur, table(D, 1, 0), D);
        name = "nothing fits";
        std::vector<float> only1(4 * static_cast<size_t>(D), NINF);
        for (int j = 0; j < 4; ++j) only1[static_cast<size_t>(j) * D] = 0.0f;          // an edge run lasts one step ...
        std::vector<float> none(4 * static_cast<size_t>(D), NINF);
        for (int j = 0; j < 4; ++j) none[static_cast<size_t>(j) * D + D - 1] = 0.0f;   // ... an interior one D: T = 50 is 2 + 48, not 2 + 9 k
        run_case(name, e, dense, kUniform, none, only1, D, true);
    }
    {   // worst-case magnitude: every term at the clamp, both signs; the overflow check of the sanitizer is the proof
        const int D = 3, T = 20000;
        std::vector<float> e(4 * static_cast<size_t>(T)), big(4 * static_cast<size_t>(D));
        float bigA[16], bigpi[4];
        for (int sign = -1; sign <= 1; sign += 2) {
            name = sign < 0 ? "every term at -clamp" : "every term at +clamp";
            for (float& v : e) v = sign * 1e9f;
            for (float& v : big) v = sign * 1e9f;
            for (float& v : bigA) v = sign * 1e9f;
            for (float& v : bigpi) v = sign * 1e9f;
            run_case(name, e, bigA, bigpi, big, big, D);
        }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("decode durations check ok\n");
    return 0;
}
