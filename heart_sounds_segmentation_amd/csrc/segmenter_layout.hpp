// segmenter_layout.hpp -- slot / tile layout of a ragged segmenter exec (hssfsst.h: hssfsst_segmenter_exec_ragged) and the launch
// lists of both segmenter execs, made on the host.
// No HIP call and no plan here: offsets in, tables out, so the builders also compile into a stand-alone program (tests/native/).
//
// A tile is 16 row slots, the rows of one recurrence workgroup (segmenter_lstm.hpp).  Recordings take the slots in descending
// length order (ties in list order), so a tile holds similar lengths and the tiles still walking at any step are a prefix of the
// tile list; the last tile is filled up with slots of length 0.  The order decides how many steps are wasted, never a result:
// a row's arithmetic does not depend on its neighbours.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace hssfsst::seglayout {

constexpr int kSlotRows = 16;                            // == kSegRows

struct Layout {
    std::vector<int> slot_rec;                           // [slots] the slot's recording, -1 for a padding slot
    std::vector<long long> slot_off;                     // [slots] first step of the recording in the arena
    std::vector<int> slot_len;                           // [slots] its steps, 0 for a padding slot; non-increasing
    std::vector<int> tile_walk;                          // [tiles] steps the tile's workgroups walk: its longest recording
    long long total = 0;                                 // steps of the whole list == offsets[count]
    int tiles() const { return static_cast<int>(tile_walk.size()); }
    int slots() const { return static_cast<int>(slot_len.size()); }
};

// The first index i whose recording offsets[i] .. offsets[i + 1] is empty, reversed or longer than max_len; -1 when there is none.
inline int64_t first_bad_length(const int64_t* offsets, int64_t count, int64_t max_len)
{
    for (int64_t i = 0; i < count; ++i)
        if (offsets[i + 1] <= offsets[i] || offsets[i + 1] - offsets[i] > max_len) return i;
    return -1;
}

// offsets: count + 1 increasing step offsets (checked by the caller: first_bad_length), count >= 1
inline void build(const int64_t* offsets, int64_t count, Layout& out)
{
    const int64_t tiles = (count + kSlotRows - 1) / kSlotRows, slots = tiles * kSlotRows;
    std::vector<int> order(static_cast<size_t>(count));
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b]; });
    out.slot_rec.assign(static_cast<size_t>(slots), -1);
    out.slot_off.assign(static_cast<size_t>(slots), 0);
    out.slot_len.assign(static_cast<size_t>(slots), 0);
    out.tile_walk.assign(static_cast<size_t>(tiles), 0);
    for (int64_t s = 0; s < count; ++s) {
        const int r = order[static_cast<size_t>(s)];
        out.slot_rec[s] = r;
        out.slot_off[s] = offsets[r] - offsets[0];
        out.slot_len[s] = static_cast<int>(offsets[r + 1] - offsets[r]);
        out.tile_walk[s / kSlotRows] = std::max(out.tile_walk[s / kSlotRows], out.slot_len[s]);
    }
    out.total = offsets[count] - offsets[0];
}

// Σ_tiles 16 · walk / Σ T − 1: the share of slot steps that compute nothing
inline double wasted_share(const Layout& l)
{
    long long walked = 0;
    for (int w : l.tile_walk) walked += static_cast<long long>(kSlotRows) * w;
    return l.total > 0 ? static_cast<double>(walked) / static_cast<double>(l.total) - 1.0 : 0.0;
}

constexpr size_t kSegPreBytes = size_t(128) << 20;       // bound of the projection scratch: sets the steps per chunk
constexpr int kSegMaxChunk = 4096;                       // ... and no launch walks more steps than this

// One launch pair (projection + recurrence) of a layer: the first `tiles` tiles walk steps s0 .. s0 + n (n <= Tc, the pitch of the
// projection scratch).  Both directions walk the same n steps: the reverse one's are the mirrored ones, taken downwards.
struct Chunk { int s0, n, tiles, Tc; };

// tile_step_bytes: projection scratch of one step of one tile (both directions)
inline size_t pre_floats(const std::vector<Chunk>& chunks, size_t tile_step_bytes)
{
    size_t m = 0;
    for (const Chunk& c : chunks) m = std::max(m, tile_step_bytes / sizeof(float) * c.tiles * c.Tc);
    return m;
}

// A dense exec (nbt tiles of T steps each): every launch takes all tiles and as many steps as fit pre_bytes.
inline std::vector<Chunk> dense_chunks(int T, int nbt, size_t tile_step_bytes, size_t pre_bytes)
{
    const size_t fit = std::max<size_t>(1, pre_bytes / (tile_step_bytes * nbt));
    const int Tc = std::min(static_cast<int>(std::min<size_t>(fit, kSegMaxChunk)), T);
    std::vector<Chunk> out;
    for (int s0 = 0; s0 < T; s0 += Tc) out.push_back({s0, std::min(Tc, T - s0), nbt, Tc});
    return out;
}

// A ragged exec: tiles finish in order (the layout sorts them), so fewer and fewer take part and the steps per launch that fit
// pre_bytes grow.
inline std::vector<Chunk> ragged_chunks(const Layout& lay, size_t tile_step_bytes, size_t pre_bytes)
{
    std::vector<Chunk> out;
    int live = lay.tiles();
    for (int s0 = 0; s0 < lay.tile_walk[0];) {
        while (lay.tile_walk[live - 1] <= s0) --live;
        const size_t fit = std::max<size_t>(1, pre_bytes / (tile_step_bytes * live));
        const int Tc = static_cast<int>(std::min<size_t>(fit, kSegMaxChunk));
        const int n = std::min(Tc, lay.tile_walk[0] - s0);
        out.push_back({s0, n, live, Tc});
        s0 += n;
    }
    return out;
}

}  // namespace hssfsst::seglayout
