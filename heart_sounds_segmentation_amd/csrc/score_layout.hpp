// score_layout.hpp -- scoring a segmentation (hssfsst.h: hssfsst_score_states): the key transform, the digit of a sort pass, the
// pass count, the block partition, the workspace and a sequential reference of the whole computation, as plain functions shared by
// the kernels (segmenter_score.hpp), the entry (sequence.hip) and a CPU check (tests/native/score_layout_check.cpp).  No HIP call
// here.  score_reference() is the specification: the kernels give its integers.
//
// The quantities.  A step with a label 0..3 is COUNTED, any other label makes it IGNORED.  Its predicted state is states[t] where
// states are given (a value above 3 makes the step ignored as well), else the argmax of its four log-probs with ties to the
// smaller state and NaN read as -inf.  confusion[label][predicted] counts the counted steps, ignored the others.  For a class c
// the counted steps are positives (label == c) or negatives, and with s = column c of logp
//   2U = sum over (positive p, negative n) of 2 [s_p > s_n] + [s_p == s_n]
// in float32's order with -0 == +0 and NaN read as -inf: the Mann-Whitney statistic with ties, doubled so that it is an integer.
//
// How it is computed.  A step becomes one 64-bit item
//   bit 0        1 for a positive
//   bits 1..32   key32(s): unsigned, monotone in s (below); 0 -- which no score maps to -- marks an ignored step
//   bits 33..    the recording's index (per_recording), else 0
// and the items are sorted by bits 1 and up with a least-significant-digit radix sort of kDigitBits bits per pass: a BLOCK of
// kBlockItems consecutive items is histogrammed by one wave, the histograms -- digit-major, block-minor -- are scanned, and the same
// wave scatters its block in order, so the sort is stable and its result is a function of the items alone.  In sorted order a TIE
// GROUP is a maximal run of items equal in bits 1 and up; with P_g positives and N_g negatives in group g and N_below(g) negatives
// of the same recording in earlier groups
//   2U = sum_g P_g (2 N_below(g) + N_g),
// which the rank kernels form with a scan over the sorted order: the running counts of positives and negatives, their values at
// the last group's and the last recording's first item.  Ignored items sort first in their recording and weigh nothing.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "decode_layout.hpp"                             // HSSFSST_DEC_HD

namespace hssfsst::scorelayout {

using i64 = long long;
using u64 = unsigned long long;
using u32 = unsigned int;

// ---- the item ----------------------------------------------------------------------------------------------------------------
constexpr int kKeyShift = 1;                             // bit 0 is the is-positive bit and is not sorted by
constexpr int kRecShift = 33;
constexpr u32 kNegInfBits = 0xff800000u;

// float32 bits -> a key that orders as the floats do: -0 -> +0, NaN -> -inf, then the sign bit is set for non-negatives and all
// bits are flipped for negatives.  The smallest key is key32(-inf) = 0x007fffff: 0 stays free for the ignored steps.
HSSFSST_DEC_HD inline u32 key32_of_bits(u32 u)
{
    if ((u & 0x7fffffffu) > 0x7f800000u) u = kNegInfBits;
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline u32 float_bits(float x) { u32 u; std::memcpy(&u, &x, 4); return u; }
inline u32 key32(float x) { return key32_of_bits(float_bits(x)); }

HSSFSST_DEC_HD inline bool counted(unsigned label, unsigned predicted) { return label < 4u && predicted < 4u; }
HSSFSST_DEC_HD inline u64 item(u32 key, bool positive, i64 rec)
{
    return (static_cast<u64>(rec) << kRecShift) | (static_cast<u64>(key) << kKeyShift) | (positive ? 1u : 0u);
}
HSSFSST_DEC_HD inline u64 ignored_item(i64 rec) { return static_cast<u64>(rec) << kRecShift; }
HSSFSST_DEC_HD inline u32 item_positive(u64 it) { return static_cast<u32>(it & 1u); }
HSSFSST_DEC_HD inline u32 item_negative(u64 it) { return ((it & 1u) == 0u && static_cast<u32>(it >> kKeyShift) != 0u) ? 1u : 0u; }
HSSFSST_DEC_HD inline u64 item_group(u64 it) { return it >> kKeyShift; }          // equal <=> the same tie group
HSSFSST_DEC_HD inline i64 item_rec(u64 it) { return static_cast<i64>(it >> kRecShift); }

// the argmax of four log-probs: NaN reads as -inf, ties go to the smaller state (-0 == +0 is a tie)
HSSFSST_DEC_HD inline int argmax4(const float* e)
{
    int best = 0;
    float vb = e[0] != e[0] ? -__builtin_huge_valf() : e[0];
    for (int j = 1; j < 4; ++j) {
        const float v = e[j] != e[j] ? -__builtin_huge_valf() : e[j];
        if (v > vb) { vb = v; best = j; }
    }
    return best;
}

// ---- the sort ------------------------------------------------------------------------------------------------------------------
constexpr int kDigitBits = 8;
constexpr int kDigits = 1 << kDigitBits;
constexpr int kWave = 64;
constexpr int kRounds = 32;                              // items of a block per lane
constexpr int kBlockItems = kWave * kRounds;             // 2048: one wave's block, one column of the histogram
constexpr int kWavesPerGroup = 4;                        // blocks of a workgroup: each wave on its own, none waits for another
constexpr int kSortThreads = kWave * kWavesPerGroup;
constexpr int kMaxPasses = (64 - kKeyShift + kDigitBits - 1) / kDigitBits;        // 8

HSSFSST_DEC_HD inline int digit(u64 it, int pass) { return static_cast<int>((it >> (kKeyShift + kDigitBits * pass)) & (kDigits - 1)); }
// bits that hold a recording index 0 .. count - 1
HSSFSST_DEC_HD inline int rec_bits(i64 count)
{
    int b = 0;
    while (b < 31 && (1LL << b) < count) ++b;
    return b;
}
HSSFSST_DEC_HD inline int passes(i64 count, int per_recording)
{
    const int bits = 32 + (per_recording ? rec_bits(count) : 0);
    return (bits + kDigitBits - 1) / kDigitBits;
}
HSSFSST_DEC_HD inline i64 blocks(i64 n) { return (n + kBlockItems - 1) / kBlockItems; }
HSSFSST_DEC_HD inline i64 sort_groups(i64 n) { return (blocks(n) + kWavesPerGroup - 1) / kWavesPerGroup; }
HSSFSST_DEC_HD inline i64 block_first(i64 block) { return block * kBlockItems; }
HSSFSST_DEC_HD inline i64 block_items(i64 block, i64 n) { const i64 r = n - block * kBlockItems; return r < 0 ? 0 : (r < kBlockItems ? r : kBlockItems); }
// the histogram: digit-major, so that its exclusive scan is where (digit, block)'s first item goes
HSSFSST_DEC_HD inline i64 hist_index(int d, i64 block, i64 nblocks) { return static_cast<i64>(d) * nblocks + block; }
HSSFSST_DEC_HD inline i64 hist_entries(i64 n) { return static_cast<i64>(kDigits) * blocks(n); }

// the scan of the histogram: chunks of kScanChunk entries (sum per chunk; one workgroup scans the sums; each chunk is scanned
// again from its sum), three launches
constexpr int kScanThreads = 256;
constexpr int kScanPerThread = 8;
constexpr int kScanChunk = kScanThreads * kScanPerThread;                         // 2048 entries
HSSFSST_DEC_HD inline i64 scan_chunks(i64 n) { return (hist_entries(n) + kScanChunk - 1) / kScanChunk; }

// ---- the rank -------------------------------------------------------------------------------------------------------------------
constexpr int kRankThreads = 256;
constexpr int kRankPerThread = 4;                        // consecutive items of a lane
constexpr int kRankRounds = 8;
constexpr int kRankTile = kRankThreads * kRankPerThread * kRankRounds;            // 8192 items per workgroup
HSSFSST_DEC_HD inline i64 rank_tiles(i64 n) { return (n + kRankTile - 1) / kRankTile; }

// What a run of consecutive sorted items says to the items behind it.  The h and r fields are relative to the run's first item:
// the exclusive counts at the run's last group head / recording head, valid with the flag.  combine() is associative.
struct Agg {
    u32 sP, sN;                                          // positives, negatives in the run
    u32 hP, hN;                                          // those before the last group head in the run
    u32 rN;                                              // negatives before the last recording head in the run
    u32 flags;                                           // 1: the run holds a group head, 2: a recording head
};
constexpr int kAggWords = 8;                             // u32 per stored Agg (6 used)
HSSFSST_DEC_HD inline Agg combine(const Agg& a, const Agg& b)
{
    Agg o;
    o.sP = a.sP + b.sP;
    o.sN = a.sN + b.sN;
    o.hP = (b.flags & 1u) ? a.sP + b.hP : a.hP;
    o.hN = (b.flags & 1u) ? a.sN + b.hN : a.hN;
    o.rN = (b.flags & 2u) ? a.sN + b.rN : a.rN;
    o.flags = a.flags | b.flags;
    return o;
}
// one item: `prev` is the item before it in sorted order (ignored when first)
HSSFSST_DEC_HD inline Agg agg_of(u64 it, u64 prev, bool first)
{
    Agg o;
    o.sP = item_positive(it);
    o.sN = item_negative(it);
    o.hP = o.hN = o.rN = 0u;
    o.flags = (first || item_group(it) != item_group(prev) ? 1u : 0u) | (first || item_rec(it) != item_rec(prev) ? 2u : 0u);
    return o;
}
// what the item closing a tie group adds to 2U of its recording, from the inclusive scan up to it
HSSFSST_DEC_HD inline u64 group_term(const Agg& inc)
{
    return static_cast<u64>(inc.sP - inc.hP) * (static_cast<u64>(inc.hN - inc.rN) + static_cast<u64>(inc.sN - inc.rN));
}

// ---- the counts kernel ----------------------------------------------------------------------------------------------------------
constexpr int kCountThreads = 256;
constexpr int kCountPerThread = 16;
constexpr int kCountTile = kCountThreads * kCountPerThread;                       // steps per workgroup
constexpr int kScoreBatch = 256;                         // recordings per launch: their offsets travel as kernel arguments
constexpr int kCells = 17;                               // 16 of the confusion table, then ignored
constexpr int kCountLdsBytes = kScoreBatch * kCells * 4 + (kScoreBatch + 1) * 8;  // 19 464: counters and the launch's offsets
constexpr int kSortLdsBytes = kWavesPerGroup * kDigits * 4;                       // 4096: one histogram / cursor table per wave
HSSFSST_DEC_HD inline i64 count_groups(i64 steps) { return (steps + kCountTile - 1) / kCountTile; }

// ---- the workspace --------------------------------------------------------------------------------------------------------------
// two item buffers (8 bytes per step each), the histogram (4 x 256 bytes per block of 2048), its chunk sums, and per rank tile the
// tile's Agg and the scan of those: 16.6 bytes per step; kWorkBytesPerStep x steps + kWorkBytesConstant covers it.  Needed only
// where a rank is asked for.
constexpr i64 kWorkBytesPerStep = 17;
constexpr i64 kWorkBytesPerRecording = 0;
constexpr i64 kWorkBytesConstant = 4096;
struct Workspace { i64 items_a, items_b, hist, sums, tile_agg, tile_carry, end; };            // byte offsets, 16-byte aligned
HSSFSST_DEC_HD inline i64 align16(i64 v) { return (v + 15) & ~static_cast<i64>(15); }
HSSFSST_DEC_HD inline Workspace workspace(i64 n)
{
    Workspace w;
    w.items_a = 0;
    w.items_b = align16(w.items_a + 8 * n);
    w.hist = align16(w.items_b + 8 * n);
    w.sums = align16(w.hist + 4 * hist_entries(n));
    w.tile_agg = align16(w.sums + 4 * scan_chunks(n));
    w.tile_carry = align16(w.tile_agg + 4 * kAggWords * rank_tiles(n));
    w.end = align16(w.tile_carry + 4 * kAggWords * rank_tiles(n));
    return w;
}
HSSFSST_DEC_HD inline i64 workspace_bytes(i64 total_steps, i64 count)
{
    return kWorkBytesPerStep * total_steps + kWorkBytesPerRecording * count + kWorkBytesConstant;
}

// ---- the sequential reference ---------------------------------------------------------------------------------------------------
// groups = count (per_recording) or 1.  confusion (groups, 4, 4), ignored (groups), rank (groups, 4, 3) = {2U, P, N} or empty.
struct Scores {
    std::vector<i64> confusion, ignored, rank;
};

inline Scores score_reference(const float* logp, const unsigned char* states, const unsigned char* labels, const i64* offsets, i64 count,
                              bool per_recording, bool want_rank)
{
    const i64 groups = per_recording ? count : (count > 0 ? 1 : 0);
    const i64 n = count > 0 ? offsets[count] : 0;
    Scores out;
    out.confusion.assign(static_cast<size_t>(16 * groups), 0);
    out.ignored.assign(static_cast<size_t>(groups), 0);
    if (want_rank) out.rank.assign(static_cast<size_t>(12 * groups), 0);
    std::vector<i64> rec(static_cast<size_t>(n), 0);
    if (per_recording)
        for (i64 r = 0; r < count; ++r)
            for (i64 t = offsets[r]; t < offsets[r + 1]; ++t) rec[static_cast<size_t>(t)] = r;
    std::vector<char> use(static_cast<size_t>(n), 0);
    for (i64 t = 0; t < n; ++t) {
        const unsigned pred = states ? states[t] : static_cast<unsigned>(argmax4(logp + 4 * t));
        const i64 g = rec[static_cast<size_t>(t)];
        if (counted(labels[t], pred)) {
            use[static_cast<size_t>(t)] = 1;
            ++out.confusion[static_cast<size_t>(16 * g + 4 * labels[t] + pred)];
        } else {
            ++out.ignored[static_cast<size_t>(g)];
        }
    }
    if (!want_rank) return out;
    std::vector<u64> a(static_cast<size_t>(n)), b(static_cast<size_t>(n));
    const int np = passes(count, per_recording ? 1 : 0);
    for (int c = 0; c < 4; ++c) {
        for (i64 t = 0; t < n; ++t) {
            const i64 g = rec[static_cast<size_t>(t)];
            a[static_cast<size_t>(t)] = use[static_cast<size_t>(t)] ? item(key32(logp[4 * t + c]), labels[t] == c, g) : ignored_item(g);
            if (use[static_cast<size_t>(t)]) ++out.rank[static_cast<size_t>(12 * g + 3 * c + (labels[t] == c ? 1 : 2))];
        }
        // the passes, as the kernels run them: a counting sort per digit is the stable scatter
        for (int p = 0; p < np; ++p) {
            i64 first[kDigits + 1] = {0};
            for (i64 t = 0; t < n; ++t) ++first[digit(a[static_cast<size_t>(t)], p) + 1];
            for (int d = 0; d < kDigits; ++d) first[d + 1] += first[d];
            for (i64 t = 0; t < n; ++t) b[static_cast<size_t>(first[digit(a[static_cast<size_t>(t)], p)]++)] = a[static_cast<size_t>(t)];
            a.swap(b);
        }
        Agg run{0, 0, 0, 0, 0, 0};
        for (i64 t = 0; t < n; ++t) {
            const u64 it = a[static_cast<size_t>(t)];
            run = combine(run, agg_of(it, t ? a[static_cast<size_t>(t - 1)] : 0, t == 0));
            if (t + 1 == n || item_group(a[static_cast<size_t>(t + 1)]) != item_group(it))
                out.rank[static_cast<size_t>(12 * item_rec(it) + 3 * c)] += static_cast<i64>(group_term(run));
        }
    }
    return out;
}

// the same integers from the definition: every (positive, negative) pair compared as floats.  For the checks, at small sizes.
inline Scores score_brute_force(const float* logp, const unsigned char* states, const unsigned char* labels, const i64* offsets, i64 count,
                                bool per_recording)
{
    Scores out = score_reference(logp, states, labels, offsets, count, per_recording, false);
    const i64 groups = per_recording ? count : (count > 0 ? 1 : 0);
    out.rank.assign(static_cast<size_t>(12 * groups), 0);
    auto value = [](float x) { return x != x ? -__builtin_huge_valf() : x; };
    for (i64 g = 0; g < groups; ++g) {
        const i64 lo = per_recording ? offsets[g] : 0, hi = per_recording ? offsets[g + 1] : offsets[count];
        for (int c = 0; c < 4; ++c) {
            i64 u2 = 0, P = 0, N = 0;
            for (i64 p = lo; p < hi; ++p) {
                const unsigned pp = states ? states[p] : static_cast<unsigned>(argmax4(logp + 4 * p));
                if (!counted(labels[p], pp)) continue;
                (labels[p] == c ? P : N) += 1;
                if (labels[p] != c) continue;
                for (i64 q = lo; q < hi; ++q) {
                    const unsigned pq = states ? states[q] : static_cast<unsigned>(argmax4(logp + 4 * q));
                    if (!counted(labels[q], pq) || labels[q] == c) continue;
                    const float sp = value(logp[4 * p + c]), sn = value(logp[4 * q + c]);
                    u2 += sp > sn ? 2 : (sp == sn ? 1 : 0);
                }
            }
            out.rank[static_cast<size_t>(12 * g + 3 * c)] = u2;
            out.rank[static_cast<size_t>(12 * g + 3 * c + 1)] = P;
            out.rank[static_cast<size_t>(12 * g + 3 * c + 2)] = N;
        }
    }
    return out;
}

}  // namespace hssfsst::scorelayout
