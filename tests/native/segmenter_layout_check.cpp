// Stand-alone check of the ragged segmenter's slot / tile layout builder and of the segmenter's launch lists
// (csrc/segmenter_layout.hpp: host only, no HIP), built with -fsanitize=address,undefined by tests/test_segmenter_ragged.py.
// Any failed property or sanitizer report ends the run non-zero.
#include "segmenter_layout.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace sl = hssfsst::seglayout;

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } \
    } while (0)

static void run_case(const char* name, const std::vector<int>& lens)
{
    const int64_t count = static_cast<int64_t>(lens.size());
    std::vector<int64_t> offsets(lens.size() + 1, 0);                // exactly sized: a read past the end is a report
    for (size_t i = 0; i < lens.size(); ++i) offsets[i + 1] = offsets[i] + lens[i];
    CHECK(sl::first_bad_length(offsets.data(), count, int64_t(1) << 28) == -1, "valid offsets refused");
    sl::Layout lay;
    sl::build(offsets.data(), count, lay);
    const int tiles = static_cast<int>((count + sl::kSlotRows - 1) / sl::kSlotRows);
    CHECK(lay.tiles() == tiles && lay.slots() == tiles * sl::kSlotRows, "%d tiles, %d slots for %lld recordings", lay.tiles(), lay.slots(),
          static_cast<long long>(count));
    CHECK(lay.slot_rec.size() == lay.slot_len.size() && lay.slot_off.size() == lay.slot_len.size(), "table sizes differ");
    CHECK(lay.total == offsets[count], "total %lld", lay.total);
    // every recording occupies exactly one slot; padding slots have length 0; offsets round-trip
    std::vector<int> seen(lens.size(), 0);
    for (int s = 0; s < lay.slots(); ++s) {
        const int r = lay.slot_rec[s];
        if (r < 0) {
            CHECK(lay.slot_len[s] == 0, "padding slot %d has length %d", s, lay.slot_len[s]);
            CHECK(s >= count, "padding slot %d before the last recording", s);
            continue;
        }
        CHECK(r < count, "slot %d names recording %d", s, r);
        if (r >= count) continue;
        ++seen[r];
        CHECK(lay.slot_off[s] == offsets[r], "slot %d: offset %lld, recording %d starts at %lld", s, lay.slot_off[s], r,
              static_cast<long long>(offsets[r]));
        CHECK(lay.slot_off[s] + lay.slot_len[s] == offsets[r + 1], "slot %d: end does not round-trip", s);
    }
    for (size_t r = 0; r < seen.size(); ++r) CHECK(seen[r] == 1, "recording %zu occupies %d slots", r, seen[r]);
    // slot lengths are non-increasing; each tile's walk equals its maximum
    for (int s = 1; s < lay.slots(); ++s) CHECK(lay.slot_len[s] <= lay.slot_len[s - 1], "slot %d longer than slot %d", s, s - 1);
    long long walked = 0;
    for (int t = 0; t < lay.tiles(); ++t) {
        int mx = 0;
        for (int j = 0; j < sl::kSlotRows; ++j) mx = lay.slot_len[t * sl::kSlotRows + j] > mx ? lay.slot_len[t * sl::kSlotRows + j] : mx;
        CHECK(lay.tile_walk[t] == mx && mx > 0, "tile %d walks %d, its longest slot is %d", t, lay.tile_walk[t], mx);
        walked += static_cast<long long>(sl::kSlotRows) * mx;
    }
    const double w = sl::wasted_share(lay);
    CHECK(w >= 0.0 && w == static_cast<double>(walked) / static_cast<double>(lay.total) - 1.0, "wasted share %g", w);
    std::printf("%-8s %5lld recordings, %3d tiles, wasted share %.4f\n", name, static_cast<long long>(count), lay.tiles(), w);
}

// what every launch list promises: steps 0 .. walk once and in order; n <= Tc <= kSegMaxChunk; the projection scratch of a launch
// within pre_bytes unless it is down to one step
static void check_chunks(const char* name, const std::vector<sl::Chunk>& chunks, int walk, size_t tile_step_bytes, size_t pre_bytes)
{
    int next = 0;
    for (const sl::Chunk& c : chunks) {
        CHECK(c.s0 == next && c.n >= 1, "chunk starts at step %d with %d steps, expected step %d", c.s0, c.n, next);
        CHECK(c.n <= c.Tc && c.Tc <= sl::kSegMaxChunk, "chunk at step %d: n %d, Tc %d", c.s0, c.n, c.Tc);
        CHECK(c.tiles >= 1, "chunk at step %d has %d tiles", c.s0, c.tiles);
        CHECK(c.Tc == 1 || static_cast<size_t>(c.tiles) * c.Tc * tile_step_bytes <= pre_bytes, "chunk at step %d: %d tiles x %d steps exceed %zu bytes",
              c.s0, c.tiles, c.Tc, pre_bytes);
        next = c.s0 + c.n;
    }
    CHECK(next == walk, "chunks end at step %d of %d", next, walk);
}

// the dense exec's chunk loop as it stood inline in hssfsst_segmenter_exec before the list was a function
static std::vector<sl::Chunk> inline_dense_loop(int T, int nbt, size_t tile_step_bytes)
{
    const size_t step_bytes = tile_step_bytes * nbt;
    int Tc = static_cast<int>(std::max<size_t>(1, sl::kSegPreBytes / step_bytes));
    Tc = std::min(std::min(Tc, sl::kSegMaxChunk), T);
    std::vector<sl::Chunk> out;
    for (int t0 = 0; t0 < T; t0 += Tc) out.push_back({t0, std::min(Tc, T - t0), nbt, Tc});
    return out;
}

static void run_dense(int T, int nbt, size_t tile_step_bytes)
{
    char name[64];
    std::snprintf(name, sizeof(name), "dense T=%d nbt=%d", T, nbt);
    const std::vector<sl::Chunk> got = sl::dense_chunks(T, nbt, tile_step_bytes, sl::kSegPreBytes), want = inline_dense_loop(T, nbt, tile_step_bytes);
    check_chunks(name, got, T, tile_step_bytes, sl::kSegPreBytes);
    CHECK(got.size() == want.size(), "%zu chunks, the inline loop made %zu", got.size(), want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); ++i)
        CHECK(got[i].s0 == want[i].s0 && got[i].n == want[i].n && got[i].tiles == want[i].tiles && got[i].Tc == want[i].Tc,
              "chunk %zu: {%d, %d, %d, %d}, the inline loop made {%d, %d, %d, %d}", i, got[i].s0, got[i].n, got[i].tiles, got[i].Tc,
              want[i].s0, want[i].n, want[i].tiles, want[i].Tc);
    for (const sl::Chunk& c : got) CHECK(c.tiles == nbt, "a dense launch of %d of %d tiles", c.tiles, nbt);
    std::printf("%-24s %zu launches per layer\n", name, got.size());
}

static void run_ragged(const char* name, const std::vector<int>& lens, size_t tile_step_bytes, size_t pre_bytes)
{
    std::vector<int64_t> offsets(lens.size() + 1, 0);
    for (size_t i = 0; i < lens.size(); ++i) offsets[i + 1] = offsets[i] + lens[i];
    sl::Layout lay;
    sl::build(offsets.data(), static_cast<int64_t>(lens.size()), lay);
    const std::vector<sl::Chunk> chunks = sl::ragged_chunks(lay, tile_step_bytes, pre_bytes);
    check_chunks(name, chunks, lay.tile_walk[0], tile_step_bytes, pre_bytes);
    for (const sl::Chunk& c : chunks) {                              // the launch's tiles: exactly those still walking at its first step
        int live = 0;
        for (int w : lay.tile_walk) live += w > c.s0 ? 1 : 0;
        CHECK(c.tiles == live, "chunk at step %d takes %d tiles, %d still walk", c.s0, c.tiles, live);
    }
    std::printf("%-24s %zu launches per layer\n", name, chunks.size());
}

// the block of a list's device tables: five arrays in the stated order, back to back, each aligned to its element, and the byte
// offsets as they stood inline in the ragged BiLSTM's table builder before table_block() was a function
static void run_table_block(int64_t count)
{
    char name[64];
    std::snprintf(name, sizeof(name), "table block count=%lld", static_cast<long long>(count));
    const sl::TableBlock b = sl::table_block(count);
    const size_t tiles = static_cast<size_t>((count + sl::kSlotRows - 1) / sl::kSlotRows), slots = tiles * sl::kSlotRows;
    const size_t o_base = slots * sizeof(long long), o_len = o_base + (tiles + 1) * sizeof(long long);
    const size_t o_rec = o_len + slots * sizeof(int), o_walk = o_rec + slots * sizeof(int);
    CHECK(b.tiles == tiles && b.slots == slots, "%zu tiles, %zu slots", b.tiles, b.slots);
    CHECK(b.o_off == 0 && b.o_base == o_base && b.o_len == o_len && b.o_rec == o_rec && b.o_walk == o_walk,
          "offsets {%zu, %zu, %zu, %zu, %zu}, the inline arithmetic made {0, %zu, %zu, %zu, %zu}", b.o_off, b.o_base, b.o_len, b.o_rec, b.o_walk,
          o_base, o_len, o_rec, o_walk);
    CHECK(b.bytes == o_walk + tiles * sizeof(int), "%zu bytes, the inline arithmetic made %zu", b.bytes, o_walk + tiles * sizeof(int));
    // slot_off | tile_base | slot_len | slot_rec | tile_walk: each starts where the one before ends
    const size_t start[5] = {b.o_off, b.o_base, b.o_len, b.o_rec, b.o_walk};
    const size_t size[5] = {slots * sizeof(long long), (tiles + 1) * sizeof(long long), slots * sizeof(int), slots * sizeof(int), tiles * sizeof(int)};
    const size_t align[5] = {8, 8, 4, 4, 4};
    size_t end = 0, sum = 0;
    for (int i = 0; i < 5; ++i) {
        CHECK(start[i] == end, "array %d starts at byte %zu, the one before ends at %zu", i, start[i], end);
        CHECK(start[i] % align[i] == 0, "array %d at byte %zu is not %zu-byte aligned", i, start[i], align[i]);
        end = start[i] + size[i];
        sum += size[i];
    }
    CHECK(b.bytes == end && b.bytes == sum, "%zu bytes, the arrays end at %zu and sum to %zu", b.bytes, end, sum);
    std::printf("%-24s %zu bytes\n", name, b.bytes);
}

int main()
{
    run_case("one", {1});
    run_case("equal16", std::vector<int>(16, 70));
    run_case("seventeen", {9, 8, 7, 6, 5, 4, 3, 2, 1, 10, 11, 12, 13, 14, 15, 16, 17});
    run_case("mixed19", {1, 2, 15, 16, 17, 40, 333, 1100, 5, 16, 31, 64, 7, 7, 250, 3, 1, 90, 600});
    std::vector<int> many(1000);
    unsigned long long x = 0x9e3779b97f4a7c15ull;
    for (int& v : many) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        v = 1 + static_cast<int>((x >> 33) % 60000);
    }
    run_case("random1k", many);
    run_case("three", {5, 5, 5});

    // the launch lists: tile_step = 128 KiB is the library's (2 directions x 64 gate tiles x 256 floats), the small one reaches kSegMaxChunk
    const size_t tile_step = size_t(2) * 64 * 256 * sizeof(float);
    run_dense(1, 1, tile_step);
    run_dense(70, 2, tile_step);
    run_dense(1024, 1, tile_step);
    run_dense(1025, 1, tile_step);
    run_dense(5000, 3, tile_step);
    run_dense(9, 2000, tile_step);                                   // more tiles than steps fit: one step per launch
    run_dense(10000, 1, 1024);
    run_dense(4096, 1, 1024);
    run_dense(4097, 2, 1024);
    run_ragged("ragged seventeen 1MiB", {9, 8, 7, 6, 5, 4, 3, 2, 1, 10, 11, 12, 13, 14, 15, 16, 17}, tile_step, size_t(1) << 20);
    run_ragged("ragged seventeen", {9, 8, 7, 6, 5, 4, 3, 2, 1, 10, 11, 12, 13, 14, 15, 16, 17}, tile_step, sl::kSegPreBytes);
    run_ragged("ragged mixed19 1MiB", {1, 2, 15, 16, 17, 40, 333, 1100, 5, 16, 31, 64, 7, 7, 250, 3, 1, 90, 600}, tile_step, size_t(1) << 20);
    run_ragged("ragged random1k", many, tile_step, sl::kSegPreBytes);
    run_ragged("ragged random1k small", many, 1024, sl::kSegPreBytes);
    run_ragged("ragged one", {1}, tile_step, size_t(1) << 16);       // the bound below one step of one tile: Tc = 1

    for (int64_t count : {1, 16, 17, 33, 1000}) run_table_block(count);

    // what the entry point refuses, and at which index
    const char* name = "bad";
    const int64_t flat[] = {0, 5, 5}, back[] = {0, 7, 3}, lng[] = {0, 4, 104}, good[] = {0, 4, 9};
    CHECK(sl::first_bad_length(flat, 2, 1000) == 1, "[0, 5, 5]");
    CHECK(sl::first_bad_length(back, 2, 1000) == 1, "[0, 7, 3]");
    CHECK(sl::first_bad_length(lng, 2, 99) == 1, "a recording over the limit");
    CHECK(sl::first_bad_length(good, 2, 5) == -1, "[0, 4, 9]");
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("segmenter layout ok\n");
    return 0;
}
