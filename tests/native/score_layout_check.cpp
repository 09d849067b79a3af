// Stand-alone check of csrc/score_layout.hpp (host only, no HIP): the key transform is monotone over a sweep of float32 bit
// patterns that includes +-0, +-inf, NaN and denormals; the pass count, the block partition and the workspace at their borders;
// the Agg operator is associative; the sequential reference equals brute force over all pairs, pooled and per recording, with
// ties, ignored steps, NaN, -inf and +-0.  Built with -fsanitize=address,undefined by tests/test_segmentation_scores.py: every
// array here is exactly as long as the function under test may read.  Any failed property or sanitizer report ends the run
// non-zero.
#include "score_layout.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

using namespace hssfsst::scorelayout;

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { if (failures < 40) { std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } \
    } while (0)

static const float kNaN = std::numeric_limits<float>::quiet_NaN();
static const float kInf = std::numeric_limits<float>::infinity();

static float from_bits(u32 u) { float x; std::memcpy(&x, &u, 4); return x; }
static float value(float x) { return x != x ? -kInf : x; }

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u32 rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<u32>(rng_state >> 33);
}

static void key_checks()
{
    const char* name = "key";
    std::vector<u32> sweep = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x80800000u,
                              0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7f800001u, 0xffc00000u, 0x7fc00000u, 0xffffffffu,
                              0x7fffffffu, 0x3f800000u, 0xbf800000u};
    for (u32 u = 0; u < 0xff000000u; u += 0x00010001u * 37u) sweep.push_back(u);
    for (int i = 0; i < 20000; ++i) sweep.push_back(rnd() * 2u + (rnd() & 1u));
    for (size_t i = 0; i < sweep.size(); ++i) {
        const float a = from_bits(sweep[i]);
        CHECK(key32(a) != 0u, "key 0 is taken by %08x", sweep[i]);
        CHECK(key32(a) >= key32(-kInf), "%08x below -inf", sweep[i]);
        const size_t j = (i * 7919u + 13u) % sweep.size();
        for (size_t k : {j, (i + 1) % sweep.size()}) {
            const float b = from_bits(sweep[k]);
            const float va = value(a), vb = value(b);
            const u32 ka = key32(a), kb = key32(b);
            CHECK((va < vb) == (ka < kb) && (va == vb) == (ka == kb), "order of %08x and %08x: keys %08x %08x", sweep[i], sweep[k], ka, kb);
        }
    }
    CHECK(key32(0.0f) == key32(-0.0f), "-0 and +0");
    CHECK(key32(kNaN) == key32(-kInf) && key32(-kNaN) == key32(-kInf), "NaN reads as -inf");
    CHECK(key32(-kInf) == 0x007fffffu && key32(kInf) == 0xff800000u, "the ends");
    CHECK(key32(from_bits(0x00000001u)) > key32(0.0f) && key32(from_bits(0x80000001u)) < key32(0.0f), "denormals around 0");
    // the item: fields do not overlap, the is-positive bit is below every digit
    const u64 it = item(0xffffffffu, true, (1LL << 31) - 1);
    CHECK(it == ~0ull, "all fields full");
    CHECK(item_rec(it) == (1LL << 31) - 1 && item_positive(it) == 1u && item_negative(it) == 0u, "fields");
    CHECK(item_negative(ignored_item(5)) == 0u && item_positive(ignored_item(5)) == 0u && item_rec(ignored_item(5)) == 5, "an ignored item");
    CHECK(item_negative(item(key32(-kInf), false, 0)) == 1u, "a negative at -inf");
    for (int p = 0; p < kMaxPasses; ++p) CHECK(digit(1ull, p) == 0, "bit 0 in the digit of pass %d", p);
    CHECK(digit(item(0x000000ffu, false, 0), 0) == 255 && digit(item(0xff000000u, false, 0), 3) == 255 && digit(item(0, false, 1), 4) == 1,
          "digits");
    float e[4] = {kNaN, -kInf, -kInf, kNaN};
    CHECK(argmax4(e) == 0, "argmax of nothing");
    float e2[4] = {-1.0f, 0.0f, -0.0f, kNaN};
    CHECK(argmax4(e2) == 1, "argmax with -0 == +0");
    float e3[4] = {kNaN, -3.0f, kInf, kInf};
    CHECK(argmax4(e3) == 2, "argmax ties");
}

static void geometry_checks()
{
    const char* name = "geometry";
    CHECK(rec_bits(1) == 0 && rec_bits(2) == 1 && rec_bits(3) == 2 && rec_bits(256) == 8 && rec_bits(257) == 9, "rec_bits");
    CHECK(rec_bits((1LL << 31) - 1) == 31, "rec_bits at the limit");
    CHECK(passes(1000000, 0) == 4 && passes(1, 1) == 4 && passes(2, 1) == 5 && passes(256, 1) == 5 && passes(257, 1) == 6, "passes");
    CHECK(passes(1 << 16, 1) == 6 && passes((1 << 16) + 1, 1) == 7 && passes((1LL << 31) - 1, 1) == 8 && kMaxPasses == 8, "passes at the limit");
    for (i64 count : {1LL, 2LL, 255LL, 256LL, 257LL, 65536LL, 65537LL, (1LL << 31) - 1}) {
        const int np = passes(count, 1);
        CHECK(kKeyShift + kDigitBits * np >= kRecShift + rec_bits(count) && np <= kMaxPasses, "the passes cover count %lld", count);
        // no bit of the largest recording index is above the last pass, and one pass fewer would miss one (count > 1)
        const int top = kKeyShift + kDigitBits * np;
        CHECK(top >= 64 || (item(0xffffffffu, true, count - 1) >> top) == 0, "a bit above the passes at count %lld", count);
        CHECK((item(0xffffffffu, true, count - 1) >> (top - kDigitBits)) != 0, "a pass too many at count %lld", count);
    }
    for (i64 n : {1LL, 2047LL, 2048LL, 2049LL, 8191LL, 8192LL, 8193LL, (1LL << 31) - 1}) {
        CHECK(blocks(n) == (n + 2047) / 2048 && sort_groups(n) * kWavesPerGroup >= blocks(n) && (sort_groups(n) - 1) * kWavesPerGroup < blocks(n),
              "blocks of %lld", n);
        i64 sum = 0;
        for (i64 b : {0LL, blocks(n) - 1}) sum += block_items(b, n);
        CHECK(block_items(blocks(n) - 1, n) == n - (blocks(n) - 1) * kBlockItems && block_items(blocks(n), n) == 0 && sum > 0, "the last block of %lld", n);
        CHECK(hist_index(kDigits - 1, blocks(n) - 1, blocks(n)) == hist_entries(n) - 1, "the histogram of %lld", n);
        CHECK(scan_chunks(n) * kScanChunk >= hist_entries(n) && (scan_chunks(n) - 1) * kScanChunk < hist_entries(n), "chunks of %lld", n);
        CHECK(rank_tiles(n) * kRankTile >= n && (rank_tiles(n) - 1) * kRankTile < n, "tiles of %lld", n);
        const Workspace w = workspace(n);
        CHECK(w.items_b >= 8 * n && w.hist - w.items_b >= 8 * n && w.sums - w.hist >= 4 * hist_entries(n) && w.tile_agg - w.sums >= 4 * scan_chunks(n)
                  && w.tile_carry - w.tile_agg >= 4 * kAggWords * rank_tiles(n) && w.end - w.tile_carry >= 4 * kAggWords * rank_tiles(n),
              "the parts of the workspace of %lld overlap", n);
        CHECK(w.end <= workspace_bytes(n, 1) && w.items_b % 16 == 0 && w.hist % 16 == 0 && w.sums % 16 == 0 && w.tile_agg % 16 == 0, "workspace of %lld", n);
    }
    CHECK(kWorkBytesPerStep <= 24, "bytes per step");
    CHECK(kCountLdsBytes <= 64 * 1024 && kSortLdsBytes == 4096, "LDS");
}

static void agg_checks()
{
    const char* name = "agg";
    auto same = [](const Agg& a, const Agg& b) {
        return a.sP == b.sP && a.sN == b.sN && a.flags == b.flags && (!(a.flags & 1u) || (a.hP == b.hP && a.hN == b.hN)) && (!(a.flags & 2u) || a.rN == b.rN);
    };
    for (int trial = 0; trial < 2000; ++trial) {
        Agg x[3];
        for (Agg& a : x) {
            a.sP = rnd() % 9; a.sN = rnd() % 9; a.flags = rnd() % 4;
            if (a.flags & 2u) a.flags |= 1u;
            a.hP = (a.flags & 1u) ? rnd() % (a.sP + 1) : 0u; a.hN = (a.flags & 1u) ? rnd() % (a.sN + 1) : 0u;
            a.rN = (a.flags & 2u) ? rnd() % (a.hN + 1) : 0u;
        }
        CHECK(same(combine(combine(x[0], x[1]), x[2]), combine(x[0], combine(x[1], x[2]))), "not associative at trial %d", trial);
        const Agg zero{0, 0, 0, 0, 0, 0};
        CHECK(same(combine(zero, x[0]), x[0]) && same(combine(x[0], zero), x[0]), "zero is not neutral at trial %d", trial);
    }
}

static void reference_case(const char* name, const std::vector<i64>& lens, int kind, bool with_states)
{
    std::vector<i64> offs = {0};
    for (i64 T : lens) offs.push_back(offs.back() + T);
    const i64 n = offs.back(), count = static_cast<i64>(lens.size());
    std::vector<float> logp(static_cast<size_t>(4 * n));
    std::vector<unsigned char> labels(static_cast<size_t>(n)), states(static_cast<size_t>(n));
    const float special[8] = {0.0f, -0.0f, -kInf, kNaN, kInf, 1.0f, -1.0f, from_bits(0x00000001u)};
    for (i64 t = 0; t < n; ++t) {
        for (int c = 0; c < 4; ++c) {
            float v;
            if (kind == 0) v = static_cast<float>(static_cast<int>(rnd() % 17) - 8) / 8.0f;          // ties are the rule
            else if (kind == 1) v = 0.25f;                                                            // one tie group
            else if (kind == 2) v = special[rnd() % 8];
            else v = from_bits(rnd() * 2u + (rnd() & 1u));                                            // any bit pattern
            logp[static_cast<size_t>(4 * t + c)] = v;
        }
        const u32 r = rnd() % 16;
        labels[static_cast<size_t>(t)] = r < 12 ? static_cast<unsigned char>(r % 3) : (r == 12 ? 4 : (r == 13 ? 255 : 2));     // class 3 has no positives
        states[static_cast<size_t>(t)] = static_cast<unsigned char>(rnd() % 4);
    }
    if (count > 1) for (i64 t = offs[1]; t < offs[2]; ++t) labels[static_cast<size_t>(t)] = 255;    // a recording that is all ignored
    for (bool per : {false, true}) {
        const unsigned char* st = with_states ? states.data() : nullptr;
        const Scores a = score_reference(logp.data(), st, labels.data(), offs.data(), count, per, true);
        const Scores b = score_brute_force(logp.data(), st, labels.data(), offs.data(), count, per);
        CHECK(a.confusion == b.confusion && a.ignored == b.ignored, "counts (per_recording %d)", per);
        CHECK(a.rank == b.rank, "rank (per_recording %d)", per);
        i64 all = 0;
        for (i64 v : a.confusion) all += v;
        for (i64 v : a.ignored) all += v;
        CHECK(all == n, "%lld steps accounted for, of %lld", all, n);
        if (kind == 1)
            for (size_t g = 0; g < a.rank.size() / 12; ++g)
                for (int c = 0; c < 4; ++c) CHECK(a.rank[12 * g + 3 * c] == a.rank[12 * g + 3 * c + 1] * a.rank[12 * g + 3 * c + 2], "2U = P N under one value");
    }
}

int main()
{
    key_checks();
    geometry_checks();
    agg_checks();
    for (int kind = 0; kind < 4; ++kind) {
        reference_case("reference, one step", {1}, kind, false);
        reference_case("reference, one recording", {40}, kind, false);
        reference_case("reference, three recordings", {7, 13, 20}, kind, kind % 2 == 0);
        reference_case("reference, many short recordings", {1, 2, 3, 1, 5, 2, 9, 1, 1, 4, 6, 3}, kind, kind % 2 == 1);
    }
    const Scores none = score_reference(nullptr, nullptr, nullptr, nullptr, 0, true, true);
    if (!none.confusion.empty() || !none.rank.empty()) { std::printf("FAIL an empty list\n"); ++failures; }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("score layout check ok\n");
    return 0;
}
