// segmenter_layout.hpp -- slot / tile layout of a ragged segmenter exec (hssfsst.h: hssfsst_segmenter_exec_ragged), made on the host.
// No HIP call and no plan here: offsets in, tables out, so the builder also compiles into a stand-alone program (tests/native/).
//
// A tile is 16 row slots, the rows of one recurrence workgroup (segmenter_lstm.hpp).  Recordings take the slots in descending
// length order (ties in list order), so a tile holds similar lengths and the tiles still walking at any step are a prefix of the
// tile list; the last tile is filled up with slots of length 0.  The order decides how many steps are wasted, never a result:
// a row's arithmetic does not depend on its neighbours.
#pragma once

#include <algorithm>
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

}  // namespace hssfsst::seglayout
