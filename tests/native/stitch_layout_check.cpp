// Stand-alone check of csrc/stitch_layout.hpp (host only, no HIP).  Without an argument: the window set against a walk over the
// recording -- every step covered, the last window ends at T, the covering windows of a step in ascending start order and never
// more than ceil(n / stride) + 1 of them, the rows a recording takes -- for n in {1, 8, 2000}, every stride that matters and T
// around every border; ends with "stitch layout check ok".  With the path of a case file (written by
// tests/test_stitch_windows.py): runs stitch_reference() on every case in it, in the three modes, and prints the float32 rows as
// bit patterns, the float64 pooled rows and the dissent counts, which the test compares with its numpy restatement.  Built with
// -fsanitize=address,undefined: every array here is exactly as long as the function under test may read.
//
// The case file, whitespace separated: per case "case count n stride win_steps has_weights", then count win_first, count + 1
// offsets, n weights and 4 win_steps rows as float32 bit patterns in hex.
#include "stitch_layout.hpp"

#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace hssfsst::stitchlayout;

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { if (failures < 40) { std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } \
    } while (0)

static void window_set_checks()
{
    const char* name = "window set";
    const int ns[3] = {1, 8, 2000};
    for (int n : ns) {
        std::vector<int> strides;
        for (int s = 1; s <= n; ++s)
            if (n <= 8 || n % s == 0 || s == 999 || s == 1999) strides.push_back(s);
        for (int stride : strides) {
            std::vector<i64> Ts;
            for (i64 T = 1; T <= (n <= 8 ? 5 * n : 0); ++T) Ts.push_back(T);
            for (i64 T : {i64(n) - 1, i64(n), i64(n) + 1, i64(n) + stride - 1, i64(n) + stride, i64(n) + stride + 1, 3 * i64(n) + 7})
                if (T >= 1) Ts.push_back(T);
            for (i64 T : Ts) {
                // the walk: every regular window that fits, then the tail if the last one does not end at T
                std::vector<i64> starts;
                if (T <= n) starts.push_back(0);
                else {
                    for (i64 s = 0; s + n <= T; s += stride) starts.push_back(s);
                    if (starts.back() + n != T) starts.push_back(T - n);
                }
                const i64 count = window_count(T, n, stride);
                CHECK(count == static_cast<i64>(starts.size()), "n %d stride %d T %lld: %lld windows, the walk finds %zu", n, stride, T, count,
                      starts.size());
                if (count != static_cast<i64>(starts.size())) continue;
                for (i64 k = 0; k < count; ++k)
                    CHECK(window_start(k, T, n, stride) == starts[k], "n %d stride %d T %lld: window %lld starts at %lld, not %lld", n, stride, T,
                          k, window_start(k, T, n, stride), starts[k]);
                CHECK(starts.back() + window_len(T, n) == T, "n %d stride %d T %lld: the last window ends at %lld", n, stride, T,
                      starts.back() + window_len(T, n));
                CHECK(window_rows(T, n, stride) == count * window_len(T, n), "n %d stride %d T %lld: rows", n, stride, T);
                if (n > 8 && ratio(n, stride) > 40) continue;        // (the per-step walk below is quadratic)
                for (i64 t = 0; t < T; ++t) {
                    std::vector<i64> want;
                    for (i64 k = 0; k < count; ++k)
                        if (starts[k] <= t && t < starts[k] + window_len(T, n)) want.push_back(k);
                    const Cover c = cover_of(t, T, n, stride);
                    bool same = cover_size(c) == static_cast<int>(want.size());
                    for (int k = 0; same && k < cover_size(c); ++k) same = cover_window(c, k) == want[k];
                    CHECK(same, "n %d stride %d T %lld step %lld: %d covering windows, the walk finds %zu", n, stride, T, t, cover_size(c),
                          want.size());
                    CHECK(!want.empty(), "n %d stride %d T %lld: step %lld is not covered", n, stride, T, t);
                    CHECK(static_cast<int>(want.size()) <= ratio(n, stride) + 1, "n %d stride %d T %lld step %lld: %zu covering windows", n,
                          stride, T, t, want.size());
                }
            }
        }
    }
    CHECK(supported(2000, 1000) && supported(15, 1) && !supported(16, 1) && supported(2000, 134) && !supported(2000, 133), "the overlap limit");
    CHECK(kMaxCover == 16 && launch_groups(1) == 1 && launch_groups(kThreads) == 1 && launch_groups(kThreads + 1) == 2, "constants");
}

static bool read_u32(std::FILE* fh, uint32_t* out)
{
    unsigned v;
    if (std::fscanf(fh, "%x", &v) != 1) return false;
    *out = v;
    return true;
}

static int run_cases(const char* path)
{
    std::FILE* fh = std::fopen(path, "r");
    if (!fh) { std::printf("cannot open %s\n", path); return 2; }
    char word[16];
    int cases = 0;
    while (std::fscanf(fh, "%15s", word) == 1) {
        long long count, win_steps;
        int n, stride, has_weights;
        if (std::strcmp(word, "case") != 0 || std::fscanf(fh, "%lld %d %d %lld %d", &count, &n, &stride, &win_steps, &has_weights) != 5) return 3;
        std::vector<int64_t> first(static_cast<size_t>(count)), offsets(static_cast<size_t>(count) + 1);
        for (auto& v : first) { long long x; if (std::fscanf(fh, "%lld", &x) != 1) return 3; v = x; }
        for (auto& v : offsets) { long long x; if (std::fscanf(fh, "%lld", &x) != 1) return 3; v = x; }
        std::vector<float> weights(has_weights ? static_cast<size_t>(n) : 0), win(4 * static_cast<size_t>(win_steps));
        for (auto* vec : {&weights, &win})
            for (float& v : *vec) { uint32_t u; if (!read_u32(fh, &u)) return 3; std::memcpy(&v, &u, 4); }
        const size_t total = static_cast<size_t>(offsets.back());
        for (int mode : {kProb, kLogp, kSelect}) {
            std::vector<float> out(4 * total);
            std::vector<double> pooled(4 * total);
            std::vector<uint8_t> dissent(total);
            stitch_reference(win.data(), first.data(), offsets.data(), count, n, stride, has_weights ? weights.data() : nullptr, mode,
                             out.data(), pooled.data(), dissent.data());
            std::printf("result %d %d %zu\n", cases, mode, total);
            for (size_t t = 0; t < total; ++t) {
                for (int j = 0; j < 4; ++j) { uint32_t u; std::memcpy(&u, &out[4 * t + j], 4); std::printf("%08" PRIx32 " ", u); }
                for (int j = 0; j < 4; ++j) std::printf("%.17g ", pooled[4 * t + j]);
                std::printf("%d\n", static_cast<int>(dissent[t]));
            }
        }
        ++cases;
    }
    std::fclose(fh);
    std::printf("stitch reference ran %d cases\n", cases);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1) return run_cases(argv[1]);
    window_set_checks();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("stitch layout check ok\n");
    return 0;
}
