// segmenter_score.hpp -- the kernels of hssfsst_score_states (hssfsst.h): confusion counts, and per class the items, a radix sort
// of them and the rank sums on the sorted order.  The arithmetic, the partition and the sequential loop that defines every
// integer: score_layout.hpp.  Every kernel ends on its own: a stage that needs another workgroup's result is another launch (the
// histogram's scan is three, the rank's scan is three), and all sums are integers, so the atomics that fold them are exact in
// any order.
#pragma once

#include <hip/hip_runtime.h>

#include "score_layout.hpp"

namespace hssfsst {

namespace sl = scorelayout;

struct ScoreArgs {
    long long off[sl::kScoreBatch + 1];                  // the step offsets of the launch's recordings (pooled: {0, steps})
    long long rec0;                                      // the first of them in the list
    int nrec;
    int per_recording;
};

// the recording of step t among off[0 .. nrec]: the largest r with off[r] <= t
__device__ __forceinline__ int score_rec_of(const long long* off, int nrec, long long t)
{
    int lo = 0, hi = nrec - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ unsigned score_predicted(const float* __restrict__ logp, const unsigned char* __restrict__ states, long long t)
{
    if (states) return states[t];
    const float4 e = reinterpret_cast<const float4*>(logp)[t];
    const float v[4] = {e.x, e.y, e.z, e.w};
    return static_cast<unsigned>(sl::argmax4(v));
}

// ---- counts: a workgroup takes kCountTile consecutive steps of the launch, counts per recording into LDS and folds -------------
__global__ __launch_bounds__(sl::kCountThreads) void seg_score_counts_kernel(const float* __restrict__ logp,
                                                                              const unsigned char* __restrict__ states,
                                                                              const unsigned char* __restrict__ labels,
                                                                              unsigned long long* __restrict__ confusion,
                                                                              unsigned long long* __restrict__ ignored,
                                                                              unsigned long long* __restrict__ rank, ScoreArgs args)
{
    __shared__ unsigned cnt[sl::kScoreBatch * sl::kCells];
    __shared__ long long off[sl::kScoreBatch + 1];
    const int tid = static_cast<int>(threadIdx.x), nrec = args.nrec;
    for (int i = tid; i <= nrec; i += sl::kCountThreads) off[i] = args.off[i];
    for (int i = tid; i < nrec * sl::kCells; i += sl::kCountThreads) cnt[i] = 0u;
    __syncthreads();
    const long long t0 = off[0] + static_cast<long long>(blockIdx.x) * sl::kCountTile;
    const long long t1 = t0 + sl::kCountTile < off[nrec] ? t0 + sl::kCountTile : off[nrec];
    if (t0 >= t1) return;                                // (uniform)
    int r = score_rec_of(off, nrec, t0 + tid < t1 ? t0 + tid : t0);
    for (long long t = t0 + tid; t < t1; t += sl::kCountThreads) {
        while (t >= off[r + 1]) ++r;
        const unsigned label = labels[t], pred = score_predicted(logp, states, t);
        atomicAdd(&cnt[r * sl::kCells + (sl::counted(label, pred) ? 4 * label + pred : 16u)], 1u);
    }
    __syncthreads();
    const int rfirst = score_rec_of(off, nrec, t0), rlast = score_rec_of(off, nrec, t1 - 1);
    for (int i = rfirst * sl::kCells + tid; i < (rlast + 1) * sl::kCells; i += sl::kCountThreads) {
        const unsigned v = cnt[i];
        if (!v) continue;
        const int rr = i / sl::kCells, cell = i % sl::kCells;
        const long long g = args.per_recording ? args.rec0 + rr : 0;
        if (cell < 16) atomicAdd(&confusion[16 * g + cell], static_cast<unsigned long long>(v));
        else atomicAdd(&ignored[g], static_cast<unsigned long long>(v));
    }
    if (!rank) return;
    // P and N of every class: the row sums of the table and what is left of the counted steps
    for (int i = rfirst * 4 + tid; i < (rlast + 1) * 4; i += sl::kCountThreads) {
        const int rr = i >> 2, c = i & 3;
        unsigned all = 0u, row = 0u;
        for (int k = 0; k < 16; ++k) {
            const unsigned v = cnt[rr * sl::kCells + k];
            all += v;
            row += (k >> 2) == c ? v : 0u;
        }
        const long long g = args.per_recording ? args.rec0 + rr : 0;
        if (row) atomicAdd(&rank[12 * g + 3 * c + 1], static_cast<unsigned long long>(row));
        if (all - row) atomicAdd(&rank[12 * g + 3 * c + 2], static_cast<unsigned long long>(all - row));
    }
}

// ---- items of one class -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(sl::kCountThreads) void seg_score_keys_kernel(const float* __restrict__ logp,
                                                                            const unsigned char* __restrict__ states,
                                                                            const unsigned char* __restrict__ labels,
                                                                            unsigned long long* __restrict__ items, int cls, ScoreArgs args)
{
    __shared__ long long off[sl::kScoreBatch + 1];
    const int tid = static_cast<int>(threadIdx.x), nrec = args.nrec;
    for (int i = tid; i <= nrec; i += sl::kCountThreads) off[i] = args.off[i];
    __syncthreads();
    const long long t0 = off[0] + static_cast<long long>(blockIdx.x) * sl::kCountTile;
    const long long t1 = t0 + sl::kCountTile < off[nrec] ? t0 + sl::kCountTile : off[nrec];
    if (t0 >= t1) return;
    int r = score_rec_of(off, nrec, t0 + tid < t1 ? t0 + tid : t0);
    for (long long t = t0 + tid; t < t1; t += sl::kCountThreads) {
        while (t >= off[r + 1]) ++r;
        const unsigned label = labels[t], pred = states ? states[t] : 0u;
        const long long g = args.per_recording ? args.rec0 + r : 0;
        const unsigned bits = __float_as_uint(logp[4 * t + cls]);
        items[t] = sl::counted(label, pred) ? sl::item(sl::key32_of_bits(bits), label == static_cast<unsigned>(cls), g) : sl::ignored_item(g);
    }
}

// ---- the sort: one wave per block of kBlockItems items, kWavesPerGroup of them in a workgroup --------------------------------
__global__ __launch_bounds__(sl::kSortThreads) void seg_score_hist_kernel(const unsigned long long* __restrict__ src,
                                                                           unsigned* __restrict__ hist, long long n, long long nblocks, int pass)
{
    __shared__ unsigned h[sl::kWavesPerGroup][sl::kDigits];
    const int wave = static_cast<int>(threadIdx.x) >> 6, lane = static_cast<int>(threadIdx.x) & 63;
    const long long block = static_cast<long long>(blockIdx.x) * sl::kWavesPerGroup + wave;
    for (int d = lane; d < sl::kDigits; d += sl::kWave) h[wave][d] = 0u;
    __syncthreads();
    if (block < nblocks) {
        const long long first = sl::block_first(block);
#pragma unroll 4
        for (int r = 0; r < sl::kRounds; ++r) {
            const long long i = first + r * sl::kWave + lane;
            if (i < n) atomicAdd(&h[wave][sl::digit(src[i], pass)], 1u);
        }
    }
    __syncthreads();
    if (block < nblocks)
        for (int d = lane; d < sl::kDigits; d += sl::kWave) hist[sl::hist_index(d, block, nblocks)] = h[wave][d];
}

// hist holds the exclusive scan: where (digit, block)'s first item goes.  A round of 64 items: the lanes of one digit are found
// with eight ballots, their first lane moves the digit's cursor on by their number, each takes its place behind it: in order.
__global__ __launch_bounds__(sl::kSortThreads) void seg_score_scatter_kernel(const unsigned long long* __restrict__ src,
                                                                              unsigned long long* __restrict__ dst,
                                                                              const unsigned* __restrict__ hist, long long n, long long nblocks,
                                                                              int pass)
{
    __shared__ unsigned cursor[sl::kWavesPerGroup][sl::kDigits];
    const int wave = static_cast<int>(threadIdx.x) >> 6, lane = static_cast<int>(threadIdx.x) & 63;
    const long long block = static_cast<long long>(blockIdx.x) * sl::kWavesPerGroup + wave;
    if (block < nblocks)
        for (int d = lane; d < sl::kDigits; d += sl::kWave) cursor[wave][d] = hist[sl::hist_index(d, block, nblocks)];
    __syncthreads();
    if (block >= nblocks) return;                        // (a whole wave: no barrier follows)
    const long long first = sl::block_first(block);
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int r = 0; r < sl::kRounds; ++r) {
        const long long i = first + r * sl::kWave + lane;
        const bool valid = i < n;
        const unsigned long long it = valid ? src[i] : 0ull;
        const int d = sl::digit(it, pass);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < sl::kDigitBits; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        unsigned at = 0u;
        const int leader = valid ? __ffsll(static_cast<long long>(same)) - 1 : lane;
        if (valid && lane == leader) at = atomicAdd(&cursor[wave][d], static_cast<unsigned>(__popcll(same)));
        at = __shfl(at, leader);
        if (valid) {
            const unsigned to = at + static_cast<unsigned>(__popcll(same & below));
            if (to < static_cast<unsigned long long>(n)) dst[to] = it;          // (always: the bound keeps a wrong table inside the buffer)
        }
    }
}

// exclusive scan over the kScanThreads lanes of a workgroup -> the lane's prefix; total: the sum.  lds: kScanThreads / 64 words.
__device__ __forceinline__ unsigned score_block_scan(unsigned v, unsigned* lds, unsigned& total)
{
    const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
    unsigned x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    unsigned before = 0u;
    total = 0u;
#pragma unroll
    for (int w = 0; w < sl::kScanThreads / 64; ++w) {
        const unsigned s = lds[w];
        before += w < wave ? s : 0u;
        total += s;
    }
    __syncthreads();
    return before + x - v;
}

__global__ __launch_bounds__(sl::kScanThreads) void seg_score_scan_sums_kernel(const unsigned* __restrict__ hist, unsigned* __restrict__ sums,
                                                                                long long entries)
{
    __shared__ unsigned lds[sl::kScanThreads / 64];
    const long long first = static_cast<long long>(blockIdx.x) * sl::kScanChunk + static_cast<long long>(threadIdx.x) * sl::kScanPerThread;
    unsigned s = 0u;
#pragma unroll
    for (int k = 0; k < sl::kScanPerThread; ++k) s += first + k < entries ? hist[first + k] : 0u;
    unsigned total;
    score_block_scan(s, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: the chunk sums -> their exclusive scan, in place
__global__ __launch_bounds__(sl::kScanThreads) void seg_score_scan_top_kernel(unsigned* __restrict__ sums, long long chunks)
{
    __shared__ unsigned lds[sl::kScanThreads / 64];
    unsigned carry = 0u;
    for (long long base = 0; base < chunks; base += sl::kScanThreads) {
        const long long i = base + threadIdx.x;
        const unsigned v = i < chunks ? sums[i] : 0u;
        unsigned total;
        const unsigned before = score_block_scan(v, lds, total);
        if (i < chunks) sums[i] = carry + before;
        carry += total;
    }
}

__global__ __launch_bounds__(sl::kScanThreads) void seg_score_scan_apply_kernel(unsigned* __restrict__ hist, const unsigned* __restrict__ sums,
                                                                                 long long entries)
{
    __shared__ unsigned lds[sl::kScanThreads / 64];
    const long long first = static_cast<long long>(blockIdx.x) * sl::kScanChunk + static_cast<long long>(threadIdx.x) * sl::kScanPerThread;
    unsigned v[sl::kScanPerThread], s = 0u;
#pragma unroll
    for (int k = 0; k < sl::kScanPerThread; ++k) {
        v[k] = first + k < entries ? hist[first + k] : 0u;
        s += v[k];
    }
    unsigned total;
    unsigned at = sums[blockIdx.x] + score_block_scan(s, lds, total);
#pragma unroll
    for (int k = 0; k < sl::kScanPerThread; ++k) {
        if (first + k < entries) hist[first + k] = at;
        at += v[k];
    }
}

// ---- the rank -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ sl::Agg score_agg_zero() { return sl::Agg{0u, 0u, 0u, 0u, 0u, 0u}; }
__device__ __forceinline__ sl::Agg score_agg_shfl_up(const sl::Agg& a, int d)
{
    return sl::Agg{__shfl_up(a.sP, d), __shfl_up(a.sN, d), __shfl_up(a.hP, d), __shfl_up(a.hN, d), __shfl_up(a.rN, d), __shfl_up(a.flags, d)};
}
__device__ __forceinline__ sl::Agg score_agg_shfl(const sl::Agg& a, int from)
{
    return sl::Agg{__shfl(a.sP, from), __shfl(a.sN, from), __shfl(a.hP, from), __shfl(a.hN, from), __shfl(a.rN, from), __shfl(a.flags, from)};
}
__device__ __forceinline__ sl::Agg score_agg_wave_scan(sl::Agg x, int lane)          // inclusive over the wave
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const sl::Agg y = score_agg_shfl_up(x, d);
        if (lane >= d) x = sl::combine(y, x);
    }
    return x;
}
__device__ __forceinline__ void score_agg_store(unsigned* p, const sl::Agg& a)
{
    p[0] = a.sP; p[1] = a.sN; p[2] = a.hP; p[3] = a.hN; p[4] = a.rN; p[5] = a.flags;
}
__device__ __forceinline__ sl::Agg score_agg_load(const unsigned* p) { return sl::Agg{p[0], p[1], p[2], p[3], p[4], p[5]}; }

// A workgroup walks its tile of kRankTile sorted items in rounds of kRankThreads x kRankPerThread.  kFinal = false: the tile's
// Agg goes to tile_agg.  kFinal = true: with the scan of those in tile_carry every item that closes a tie group adds its term
// to 2U of its recording (out = rank + 3 class, 12 int64 per recording, `groups` of them: a bound that no item reaches).
template <bool kFinal>
__global__ __launch_bounds__(sl::kRankThreads) void seg_score_rank_kernel(const unsigned long long* __restrict__ src, long long n,
                                                                           unsigned* __restrict__ tile_agg, const unsigned* __restrict__ tile_carry,
                                                                           unsigned long long* __restrict__ out, int per_recording,
                                                                           long long groups)
{
    __shared__ unsigned lds[sl::kRankThreads / 64][sl::kAggWords];
    __shared__ unsigned long long acc_lds[sl::kRankThreads / 64];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const long long tile_first = static_cast<long long>(blockIdx.x) * sl::kRankTile;
    const long long tile_last = (tile_first + sl::kRankTile < n ? tile_first + sl::kRankTile : n) - 1;
    sl::Agg run = score_agg_zero();
    bool one_rec = true;
    long long rec_first = 0;
    if (kFinal) {
        run = score_agg_load(tile_carry + sl::kAggWords * blockIdx.x);
        rec_first = sl::item_rec(src[tile_first]);
        one_rec = !per_recording || rec_first == sl::item_rec(src[tile_last]);
    }
    unsigned long long acc = 0ull;
    for (int round = 0; round < sl::kRankRounds; ++round) {
        const long long base = tile_first + static_cast<long long>(round) * (sl::kRankThreads * sl::kRankPerThread) + tid * sl::kRankPerThread;
        unsigned long long it[sl::kRankPerThread + 2];   // the item before, the lane's, the item behind
        it[0] = (base > 0 && base - 1 < n) ? src[base - 1] : 0ull;
#pragma unroll
        for (int k = 0; k <= sl::kRankPerThread; ++k) it[k + 1] = base + k < n ? src[base + k] : 0ull;
        sl::Agg inc[sl::kRankPerThread];
        sl::Agg mine = score_agg_zero();
#pragma unroll
        for (int k = 0; k < sl::kRankPerThread; ++k) {
            if (base + k < n) mine = sl::combine(mine, sl::agg_of(it[k + 1], it[k], base + k == 0));
            inc[k] = mine;
        }
        const sl::Agg scanned = score_agg_wave_scan(mine, lane);
        if (lane == 63) score_agg_store(lds[wave], scanned);
        __syncthreads();
        sl::Agg before = score_agg_zero(), total = score_agg_zero();
#pragma unroll
        for (int w = 0; w < sl::kRankThreads / 64; ++w) {
            const sl::Agg a = score_agg_load(lds[w]);
            if (w < wave) before = sl::combine(before, a);
            total = sl::combine(total, a);
        }
        __syncthreads();
        if (kFinal) {
            sl::Agg left = score_agg_shfl_up(scanned, 1);
            if (lane == 0) left = score_agg_zero();
            const sl::Agg pre = sl::combine(run, sl::combine(before, left));
#pragma unroll
            for (int k = 0; k < sl::kRankPerThread; ++k) {
                const long long i = base + k;
                if (i >= n) continue;
                if (i + 1 < n && sl::item_group(it[k + 2]) == sl::item_group(it[k + 1])) continue;
                const unsigned long long term = sl::group_term(sl::combine(pre, inc[k]));
                if (one_rec) acc += term;
                else if (term && sl::item_rec(it[k + 1]) < groups) atomicAdd(&out[12 * sl::item_rec(it[k + 1])], term);   // (always inside)
            }
        }
        run = sl::combine(run, total);
    }
    if (!kFinal) {
        if (tid == 0) score_agg_store(tile_agg + sl::kAggWords * blockIdx.x, run);
        return;
    }
    if (!one_rec) return;                                // (uniform)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_down(acc, d);
    if (lane == 0) acc_lds[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        unsigned long long s = 0ull;
        for (int w = 0; w < sl::kRankThreads / 64; ++w) s += acc_lds[w];
        if (s && rec_first < groups) atomicAdd(&out[12 * (per_recording ? rec_first : 0)], s);
    }
}

// one wave: the tiles' Aggs -> for every tile the Agg of all items before it
__global__ __launch_bounds__(64) void seg_score_rank_scan_kernel(const unsigned* __restrict__ tile_agg, unsigned* __restrict__ tile_carry, long long tiles)
{
    const int lane = static_cast<int>(threadIdx.x);
    sl::Agg carry = score_agg_zero();
    for (long long base = 0; base < tiles; base += 64) {
        const long long i = base + lane;
        const sl::Agg a = i < tiles ? score_agg_load(tile_agg + sl::kAggWords * i) : score_agg_zero();
        const sl::Agg scanned = score_agg_wave_scan(a, lane);
        sl::Agg left = score_agg_shfl_up(scanned, 1);
        if (lane == 0) left = score_agg_zero();
        if (i < tiles) score_agg_store(tile_carry + sl::kAggWords * i, sl::combine(carry, left));
        carry = sl::combine(carry, score_agg_shfl(scanned, 63));
    }
}

}  // namespace hssfsst
