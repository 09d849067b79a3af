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

// ---- Index arithmetic of the trainable layer (hssfsst.h: hssfsst_bilstm_*; kernels in segmenter_train.hpp) ----------------------
// Plain functions of integers, shared by the device-side weight pack, the kernels, the host and tests/native/.  A table's
// *_source function answers, for element i of the table, which element of the nn.LSTM tensor it holds (-1: padding, zero).
#if defined(__HIPCC__)
#define HSSFSST_SEG_HD __host__ __device__
#else
#define HSSFSST_SEG_HD
#endif

constexpr int kHp = 256;                                 // == kSegHp: the padded hidden size of every table
constexpr int kGateCols = 4 * kHp;                       // gate columns of a direction, in (unit tile, gate, unit) order
constexpr int kWaves = 8;                                // == kSegWaves
constexpr long long kWtStreamHalves = 2LL * kWaves * (kHp / 32) * 8 * 64 * 16;       // forward W_hh stream, f16 elements
constexpr long long kBwdStreamHalves = 2LL * kWaves * (kGateCols / 32) * 2 * 64 * 16; // backward W_hh^T stream, bf16 elements

// gate column n = (unit tile * 4 + gate) * 16 + c  ->  row gate * H + unit of the (4H, .) tensors, -1 for a padded unit
HSSFSST_SEG_HD inline long long gate_col_row(int n, int H)
{
    const int u = (n >> 6) * 16 + (n & 15), g = (n >> 4) & 3;
    return u < H ? static_cast<long long>(g) * H + u : -1;
}

// wt [dir][Fp][4 Hp]: element i of one direction's table -> index into weight_ih (4H, F)
HSSFSST_SEG_HD inline long long wt_source(long long i, int F, int H)
{
    const int k = static_cast<int>(i / kGateCols), n = static_cast<int>(i % kGateCols);
    const long long row = gate_col_row(n, H);
    return row >= 0 && k < F ? row * F + k : -1;
}

// forward stream [wave][K block 8][tile x gate 8][lane 64]{hi[8], lo[8]}: element i of one direction -> index into weight_hh
// (4H, H), *lo = 1 for the low half of the split
HSSFSST_SEG_HD inline long long fwd_stream_source(long long i, int H, int* lo)
{
    const int j = static_cast<int>(i & 7), lane = static_cast<int>(i >> 4) & 63, q = static_cast<int>(i >> 10) & 7;
    const int kb = static_cast<int>(i >> 13) & 7, w = static_cast<int>(i >> 16) & 7;
    *lo = static_cast<int>(i >> 3) & 1;
    const int u = (w * 2 + (q >> 2)) * 16 + (lane & 15), g = q & 3, k = kb * 32 + 8 * (lane >> 4) + j;
    return u < H && k < H ? (static_cast<long long>(g) * H + u) * H + k : -1;
}

// backward stream [wave][K block 32][output tile 2][lane 64]{hi[8], lo[8]}: the B operand of dh = dG . W_hh.  The product sums over
// the gate columns kappa = K block * 32 + 8 (lane >> 4) + j (the order of the dG image) and wave w's output columns are the units
// (2 w + tile) * 16 + (lane & 15) it owns in the forward pass.
HSSFSST_SEG_HD inline long long bwd_stream_index(int w, int kb, int ot, int lane, int lo, int j)
{
    return ((((static_cast<long long>(w) * (kGateCols / 32) + kb) * 2 + ot) * 64 + lane) * 2 + lo) * 8 + j;
}
HSSFSST_SEG_HD inline long long bwd_stream_source(long long i, int H, int* lo)
{
    const int j = static_cast<int>(i & 7), lane = static_cast<int>(i >> 4) & 63, ot = static_cast<int>(i >> 10) & 1;
    const int kb = static_cast<int>(i >> 11) & 31, w = static_cast<int>(i >> 16) & 7;
    *lo = static_cast<int>(i >> 3) & 1;
    const int kout = (2 * w + ot) * 16 + (lane & 15);
    const long long row = gate_col_row(kb * 32 + 8 * (lane >> 4) + j, H);
    return row >= 0 && kout < H ? row * H + kout : -1;
}

// The stash of a training forward: [dir][tile][t][wave][unit tile of the wave 2][i, f, g, o, c][lane 64][4 rows], float32
constexpr int kStashQ = 5;
constexpr long long kStashStepFloats = static_cast<long long>(kWaves) * 2 * kStashQ * 256;      // one (dir, tile, t): 80 KiB
HSSFSST_SEG_HD inline long long stash_floats(long long batch, long long steps)
{
    return 2 * ((batch + kSlotRows - 1) / kSlotRows) * steps * kStashStepFloats;
}
HSSFSST_SEG_HD inline long long stash_index(long long tiles, long long steps, int dir, long long tile, long long t, int w, int tl, int q,
                                            int lane, int r)
{
    return (((dir * tiles + tile) * steps + t) * (kWaves * 2) + (w * 2 + tl)) * (kStashQ * 256) + q * 256 + lane * 4 + r;
}

// The stash of a RAGGED training forward (hssfsst_bilstm_forward_ragged) is indexed by the step s a slot has walked, and a tile's
// pitch is its own walk: [dir][tile_base[tile] + s][wave][unit tile of the wave 2][i, f, g, o, c][lane 64][4 rows].  A float4 holds
// four rows, so a step of a tile is stored for all 16 of them; steps past a tile's walk do not exist.
// tile_base: [tiles + 1] prefix sums of the walks; the last one is the walked steps of one direction.
inline std::vector<long long> tile_base(const Layout& l)
{
    std::vector<long long> out(static_cast<size_t>(l.tiles()) + 1, 0);
    for (int i = 0; i < l.tiles(); ++i) out[static_cast<size_t>(i) + 1] = out[static_cast<size_t>(i)] + l.tile_walk[static_cast<size_t>(i)];
    return out;
}
inline long long stash_floats_ragged(const Layout& l)
{
    long long walked = 0;
    for (int w : l.tile_walk) walked += w;
    return 2 * walked * kStashStepFloats;
}

// The device tables of a list, in one block: slot_off long long[slots] | tile_base long long[tiles + 1] | slot_len int[slots] |
// slot_rec int[slots] | tile_walk int[tiles].  Byte offsets of the five arrays and the size of the block; they follow from count
// alone.  The 8-byte arrays come first, so every array is aligned to its element in a block that is.
struct TableBlock { size_t tiles, slots, o_off, o_base, o_len, o_rec, o_walk, bytes; };
inline TableBlock table_block(int64_t count)
{
    TableBlock b{};
    b.tiles = static_cast<size_t>((count + kSlotRows - 1) / kSlotRows);
    b.slots = b.tiles * kSlotRows;
    b.o_off = 0;
    b.o_base = b.o_off + b.slots * sizeof(long long);
    b.o_len = b.o_base + (b.tiles + 1) * sizeof(long long);
    b.o_rec = b.o_len + b.slots * sizeof(int);
    b.o_walk = b.o_rec + b.slots * sizeof(int);
    b.bytes = b.o_walk + b.tiles * sizeof(int);
    return b;
}
// walked: tile_base[tiles]; base: tile_base[tile]; s < the tile's walk
HSSFSST_SEG_HD inline long long stash_index_ragged(long long walked, long long base, int dir, long long s, int w, int tl, int q, int lane, int r)
{
    return (((dir * walked + base + s) * (kWaves * 2)) + (w * 2 + tl)) * (kStashQ * 256) + q * 256 + lane * 4 + r;
}

// One launch of the ragged backward recurrence: the first `tiles` tiles -- those whose walk exceeds s0 -- walk the steps
// min(s0 + n, walk) - 1 down to s0.  Highest range first, n <= kSegMaxChunk; a tile enters at the launch that holds its last step.
struct BwdChunk { int s0, n, tiles; };
inline std::vector<BwdChunk> ragged_bwd_chunks(const Layout& lay)
{
    std::vector<BwdChunk> out;
    const int top = lay.tile_walk[0];
    int live = 0;
    for (int s0 = (top - 1) / kSegMaxChunk * kSegMaxChunk; s0 >= 0; s0 -= kSegMaxChunk) {
        while (live < lay.tiles() && lay.tile_walk[static_cast<size_t>(live)] > s0) ++live;
        out.push_back({s0, std::min(kSegMaxChunk, top - s0), live});
    }
    return out;
}

}  // namespace hssfsst::seglayout
