// Stand-alone check of the ragged training layout (csrc/segmenter_layout.hpp: host only, no HIP), built with
// -fsanitize=address,undefined by tests/test_segmenter_train_ragged.py.  For several lists of recording lengths: the ragged stash
// index is in bounds and one-to-one over every (dir, tile, step < walk, wave, unit tile, quantity, lane, row), the stash size is
// the count of those, equal lengths give the dense stash size, and the backward launch list covers every (tile, step) exactly once,
// from the top down, in launches of at most kSegMaxChunk steps.  Any failed property or sanitizer report ends the run non-zero.
#include "segmenter_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace sl = hssfsst::seglayout;

static int failures = 0;
static const char* list_name = "";
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (failures < 20) { std::printf("FAIL %s: ", list_name); std::printf(__VA_ARGS__); std::printf("\n"); } \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

static void check_list(const char* name, const std::vector<int>& lens, bool with_stash = true)
{
    list_name = name;
    std::vector<int64_t> offsets(lens.size() + 1, 0);
    for (size_t i = 0; i < lens.size(); ++i) offsets[i + 1] = offsets[i] + lens[i];
    sl::Layout lay;
    sl::build(offsets.data(), static_cast<int64_t>(lens.size()), lay);
    const std::vector<long long> base = sl::tile_base(lay);
    const int tiles = lay.tiles();
    CHECK(static_cast<int>(base.size()) == tiles + 1 && base[0] == 0, "tile_base has %zu entries for %d tiles", base.size(), tiles);
    for (int t = 0; t < tiles; ++t) CHECK(base[t + 1] - base[t] == lay.tile_walk[t], "tile %d: pitch %lld, walk %d", t, base[t + 1] - base[t], lay.tile_walk[t]);
    const long long walked = base[static_cast<size_t>(tiles)], total = sl::stash_floats_ragged(lay);
    CHECK(total == 2 * walked * sl::kStashStepFloats, "stash_floats_ragged = %lld for %lld walked steps", total, walked);

    // one bit per float4 (a lane's four rows are consecutive: checked for each), exactly sized
    std::vector<unsigned char> hit(static_cast<size_t>(total / 4), 0);
    long long n = with_stash ? 0 : total;                              // (the launch list alone for the largest list)
    for (int dir = 0; dir < (with_stash ? 2 : 0); ++dir)
        for (int t = 0; t < tiles; ++t)
            for (int s = 0; s < lay.tile_walk[t]; ++s)
                for (int w = 0; w < sl::kWaves; ++w)
                    for (int tl = 0; tl < 2; ++tl)
                        for (int q = 0; q < sl::kStashQ; ++q)
                            for (int lane = 0; lane < 64; ++lane) {
                                const long long i = sl::stash_index_ragged(walked, base[t], dir, s, w, tl, q, lane, 0);
                                n += 4;
                                if (i < 0 || i + 3 >= total || i % 4 != 0) { CHECK(false, "stash index %lld outside [0, %lld) or unaligned", i, total); continue; }
                                for (int r = 1; r < 4; ++r)
                                    CHECK(sl::stash_index_ragged(walked, base[t], dir, s, w, tl, q, lane, r) == i + r, "rows apart at %lld", i);
                                CHECK(hit[static_cast<size_t>(i / 4)] == 0, "stash index %lld taken twice", i);
                                hit[static_cast<size_t>(i / 4)] = 1;
                            }
    CHECK(n == total, "%lld coordinates for %lld floats", n, total);

    bool equal = true;
    for (int v : lens) equal = equal && v == lens[0];
    if (equal)
        CHECK(total == sl::stash_floats(static_cast<long long>(lens.size()), lens[0]), "equal lengths: %lld floats, the dense stash has %lld", total,
              sl::stash_floats(static_cast<long long>(lens.size()), lens[0]));

    // the backward launches: each (tile, step) walked once, a tile's steps from its top down across the launches
    const std::vector<sl::BwdChunk> chunks = sl::ragged_bwd_chunks(lay);
    std::vector<int> next(static_cast<size_t>(tiles));                 // the step a tile must walk next
    for (int t = 0; t < tiles; ++t) next[t] = lay.tile_walk[t] - 1;
    int last_s0 = lay.tile_walk[0];
    for (const sl::BwdChunk& c : chunks) {
        CHECK(c.n >= 1 && c.n <= sl::kSegMaxChunk, "launch at %d walks %d steps", c.s0, c.n);
        CHECK(c.s0 >= 0 && c.s0 + c.n == last_s0, "launch [%d, %d) does not end where the one above began (%d)", c.s0, c.s0 + c.n, last_s0);
        last_s0 = c.s0;
        CHECK(c.tiles >= 1 && c.tiles <= tiles, "launch at %d has %d tiles", c.s0, c.tiles);
        for (int t = 0; t < tiles; ++t) {
            const bool takes_part = lay.tile_walk[t] > c.s0;
            CHECK(takes_part == (t < c.tiles), "launch at %d: tile %d (walk %d) %s", c.s0, t, lay.tile_walk[t], takes_part ? "left out" : "taken in");
            if (t >= c.tiles || !takes_part) continue;
            // what the kernel walks: min(s0 + n, walk) - 1 down to s0
            const int top = std::min(c.s0 + c.n, lay.tile_walk[t]) - 1;
            CHECK(top == next[t], "tile %d: launch at %d starts at step %d, step %d is due", t, c.s0, top, next[t]);
            next[t] = c.s0 - 1;
        }
    }
    CHECK(last_s0 == 0, "the launches stop at step %d", last_s0);
    for (int t = 0; t < tiles; ++t) CHECK(next[t] == -1, "tile %d: steps down to %d never walked", t, next[t]);
    std::printf("%-24s %3zu recordings, %2d tiles, %6lld walked steps, %zu backward launches ok\n", name, lens.size(), tiles, walked, chunks.size());
}

int main()
{
    check_list("mixed", {1, 2, 15, 16, 17, 40, 333, 1100, 5, 16, 31, 64, 7, 7, 250, 3, 1, 90, 600});
    check_list("one", {37});
    check_list("16 equal", std::vector<int>(16, 37));
    check_list("17 equal", std::vector<int>(17, 37));
    check_list("long beside short", {4100, 3, 1030});
    check_list("exactly one launch", {4096, 9});
    check_list("two tiles over a launch", [] { std::vector<int> v(17, 4097); v.push_back(5000); return v; }(), false);
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("segmenter train ragged layout ok\n");
    return 0;
}
