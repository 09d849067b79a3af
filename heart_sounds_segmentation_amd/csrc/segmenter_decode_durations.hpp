// segmenter_decode_durations.hpp -- explicit-duration (semi-Markov) Viterbi decoding of the segmenter's log-probs (hssfsst.h:
// hssfsst_decode_durations).  The arithmetic (int64 fixed point, exact), the tie rules and the geometry are
// csrc/decode_durations_layout.hpp's; this file is the workgroup around them.
//
// One workgroup of kLanes lanes per recording, no workgroup waits for another; every loop is bounded by T and D.
//   Forward, sources t = 0 .. T - 1, one __syncthreads() per step and no global access between two of them.  Lane l works for
//   state j = l mod 4: it works out B_t(j) from the four candidates of target t in the LDS ring and the prefix sums E(t) it
//   carries in registers, then pushes B_t(j) + len into the candidates of the targets t + d for the up to kPerLane durations it
//   owns, whose dur values it holds in registers for the whole recording: first it reads all the candidates it may replace,
//   then it compares and writes, so that the LDS round trips overlap.  Source 0 and the source that reaches target T push edge
//   (read from the table once per owned d).  The candidates are interleaved, cand[slot][j], so the lanes of one access are 8
//   bytes apart.  The emissions are quantised and staged kSegSteps steps at a time; a step's backpointers -- four predecessor
//   states, four 16-bit durations -- are kept in LDS for as long and then written out by all lanes: the states as one byte INTO
//   THE PATH OUTPUT, the durations into the workspace.
//   End: target T's slot is the end maximum.
//   Backward: lane 0 hops from run to run -- a run's duration from the workspace, its predecessor's state from the byte at its
//   first step, both read before that run is filled -- and lists up to kLanes runs in LDS; all lanes fill the listed runs' bytes.
// A lane's state is a run-time number: vectors are indexed by selects (pick4) and unrolled loops, never by it: no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "decode_durations_layout.hpp"

namespace hssfsst {

constexpr int kDurDecodeBatch = 256;                     // recordings per launch: their offsets travel as kernel arguments
constexpr int kDurFillValues = 896;                      // table values per fill launch: they travel as kernel arguments

struct DurDecodeArgs {
    durlayout::Tables tb;
    int D;
    long long off[kDurDecodeBatch + 1];                  // step offsets of the launch's recordings in the arenas
};

struct DurFillArgs {
    float v[kDurFillValues];                             // values first .. first + n - 1 of the list [durations (4, D), edge (4, D)]
    int first, n, D;
};

__global__ __launch_bounds__(kDurFillValues) void seg_durations_fill_kernel(long long* __restrict__ table, const DurFillArgs a)
{
    const int i = static_cast<int>(threadIdx.x);
    if (i < a.n) table[durlayout::table_index_of_source(a.first + i, a.D)] = durlayout::quantise(a.v[i]);
}

__device__ inline void dur_load4(const long long* p, long long v[4])
{
    const longlong2 a = *reinterpret_cast<const longlong2*>(p), b = *reinterpret_cast<const longlong2*>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}

__global__ __launch_bounds__(durlayout::kLanes) void seg_decode_durations_kernel(const float* __restrict__ logp, uint8_t* __restrict__ states,
                                                                                 long long* __restrict__ scores,
                                                                                 unsigned short* __restrict__ back,
                                                                                 const long long* __restrict__ table, const DurDecodeArgs args)
{
    namespace ul = durlayout;
    using ul::i64;
    constexpr int kChunk = 4;                            // candidates read before the first of them is written
    __shared__ __attribute__((aligned(16))) long long cand[ul::kMaxRing][4];
    __shared__ __attribute__((aligned(16))) long long stage[ul::kSegSteps * 4];     // the backtrace's run list lives here too
    __shared__ __attribute__((aligned(8))) unsigned short argd[ul::kMaxRing][4];
    __shared__ __attribute__((aligned(8))) unsigned short bdur[ul::kSegSteps][4];   // a segment's backpointers: durations ...
    __shared__ __attribute__((aligned(4))) uint8_t bpre[ul::kSegSteps][4];          // ... and predecessor states
    __shared__ int hop[4];                               // the backtrace: runs listed, boundary, state, duration

    const int tid = static_cast<int>(threadIdx.x), j = ul::lane_state(tid);
    const int D = args.D, R = ul::ring_slots(D);
    const i64 base = args.off[blockIdx.x];
    const int T = static_cast<int>(args.off[blockIdx.x + 1] - base);               // <= kMaxSteps
    const float4* e4 = reinterpret_cast<const float4*>(logp) + base;
    uint8_t* path = states + base;
    unsigned short* bk = back + 4 * base;
    const long long* tedge = table + ul::table_index(1, 1, 0, D);

    i64 Acol[4];                                         // column j of A
#pragma unroll
    for (int i = 0; i < 4; ++i) Acol[i] = ul::pick4(args.tb.A[i], j);
    i64 dur[ul::kPerLane];
#pragma unroll
    for (int k = 0; k < ul::kPerLane; ++k) {
        const int d = ul::lane_duration(tid, k);
        dur[k] = d <= D ? table[ul::table_index(0, d, j, D)] : ul::kNeg;
    }

    // the backpointers of steps first .. first + n - 1, all of one segment, from LDS to the path and the workspace
    auto flush = [&](int first, int n) {
        for (int s = tid; s < n; s += ul::kLanes) {
            path[first + s] = static_cast<uint8_t>(ul::pack_states(*reinterpret_cast<const unsigned*>(bpre[s])));
            *reinterpret_cast<ushort4*>(bk + 4 * static_cast<i64>(first + s)) = *reinterpret_cast<const ushort4*>(bdur[s]);
        }
    };

    i64 E[4] = {0, 0, 0, 0};                             // E(t): the same in every lane
    int cur = 0;                                         // t mod R
    for (int t = 0; t < T; ++t) {
        const int ts = t % ul::kSegSteps;
        if (ts == 0) {                                   // (the last step's barrier has freed the stage and completed the backpointers)
            if (t > 0) flush(t - ul::kSegSteps, ul::kSegSteps);
            const int left = T - t;
            for (int s = tid; s < ul::kSegSteps && s < left; s += ul::kLanes) {
                const float4 v = e4[t + s];
                *reinterpret_cast<longlong2*>(stage + 4 * s) = make_longlong2(ul::quantise_emission(v.x), ul::quantise_emission(v.y));
                *reinterpret_cast<longlong2*>(stage + 4 * s + 2) = make_longlong2(ul::quantise_emission(v.z), ul::quantise_emission(v.w));
            }
            __syncthreads();
        }
        i64 q[4];
        dur_load4(stage + 4 * ts, q);
        i64 B;
        unsigned pre = 0;
        if (t == 0) {
            B = ul::pick4(args.tb.pi, j);
        } else {
            i64 C[4];
            dur_load4(cand[cur], C);
            B = ul::run_start(C, E, Acol, j, &pre);
        }
        if (tid < 4) {                                   // (step 0 has no backpointers: zeros)
            bpre[ts][j] = static_cast<uint8_t>(pre);
            bdur[ts][j] = t == 0 ? static_cast<unsigned short>(0) : argd[cur][j];
        }
        if (t > 0 && t + D < T) {
            // the bulk of a recording: every target lies before T and takes dur, so nothing below branches -- a lane reads the word
            // it may replace and writes it or the candidate back; for a duration above D that word is a row of its own behind
            // the ring (bulk_slot), and its dur of kNeg never wins
#pragma unroll
            for (int k0 = 0; k0 < ul::kPerLane; k0 += kChunk) {
                if (ul::lane_duration(0, k0) > D) break; // (uniform: nobody owns a duration of this chunk)
                i64 held[kChunk];
                unsigned short harg[kChunk];
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    const int slot = ul::bulk_slot(cur, ul::lane_duration(tid, k0 + k), D, R);
                    held[k] = cand[slot][j];
                    harg[k] = argd[slot][j];
                }
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    const int d = ul::lane_duration(tid, k0 + k), slot = ul::bulk_slot(cur, d, D, R);
                    const i64 c = ul::add(B, dur[k0 + k]);
                    const bool w = d == D || ul::takes(c, held[k]);
                    cand[slot][j] = w ? c : held[k];
                    argd[slot][j] = w ? static_cast<unsigned short>(d) : harg[k];
                }
            }
        } else {
            // source 0 and the last D sources: edge scores, targets that end at T
#pragma unroll
            for (int k0 = 0; k0 < ul::kPerLane; k0 += kChunk) {
                if (ul::lane_duration(0, k0) > D) break;     // (uniform: nobody owns a duration of this chunk)
                i64 held[kChunk];
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    const int d = ul::lane_duration(tid, k0 + k);
                    held[k] = (d <= D && t + d <= T) ? cand[ul::ring_slot(cur, d, R)][j] : 0;
                }
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    const int d = ul::lane_duration(tid, k0 + k);
                    if (d <= D && t + d <= T) {
                        i64 len = dur[k0 + k];
                        if (t == 0 || t + d == T) len = tedge[ul::table_index(0, d, j, D)];
                        const int slot = ul::ring_slot(cur, d, R);
                        const i64 c = ul::add(B, len);
                        if (t == 0 || d == D || ul::takes(c, held[k])) {
                            cand[slot][j] = c;
                            argd[slot][j] = static_cast<unsigned short>(d);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) E[i] += q[i];
        cur = cur + 1 == R ? 0 : cur + 1;
        __syncthreads();
    }
    flush((T - 1) / ul::kSegSteps * ul::kSegSteps, (T - 1) % ul::kSegSteps + 1);
    __syncthreads();                                     // lane 0 reads them back below

    // the end: target T
    i64 score;
    unsigned s_end;
    int d_end;
    {
        i64 C[4];
        dur_load4(cand[cur], C);
        s_end = ul::end_state(C, E, &score);
        d_end = argd[cur][s_end];
    }
    if (tid == 0 && scores) scores[blockIdx.x] = score;
    if (score == ul::kNeg) {                             // no segmentation is allowed: every state is 0
        for (int u = tid; u < T; u += ul::kLanes) path[u] = 0;
        return;
    }

    int* runs = reinterpret_cast<int*>(stage);           // {first step, steps, state} x kLanes
    if (tid == 0) { hop[1] = T; hop[2] = static_cast<int>(s_end); hop[3] = d_end; }
    for (;;) {                                           // every round lists at least one run of at least one step
        if (tid == 0) {
            int t = hop[1], s = hop[2], d = hop[3], n = 0;
            while (n < ul::kLanes && t > 0) {
                d = d < 1 ? 1 : (d > t ? t : d);         // (always true of a followed path: keeps the walk inside the recording)
                const int start = t - d;
                runs[3 * n] = start; runs[3 * n + 1] = d; runs[3 * n + 2] = s;
                ++n;
                t = start;
                if (t > 0) {
                    s = static_cast<int>((static_cast<unsigned>(path[t]) >> (2 * s)) & 3u);
                    const ushort4 a = *reinterpret_cast<const ushort4*>(bk + 4 * static_cast<i64>(t));
                    d = s == 0 ? a.x : s == 1 ? a.y : s == 2 ? a.z : a.w;
                }
            }
            hop[0] = n; hop[1] = t; hop[2] = s; hop[3] = d;
        }
        __syncthreads();
        const int n = hop[0], left = hop[1];
        for (int r = 0; r < n; ++r) {
            const int start = runs[3 * r], steps = runs[3 * r + 1];
            const uint8_t s = static_cast<uint8_t>(runs[3 * r + 2]);
            for (int u = tid; u < steps; u += ul::kLanes) path[start + u] = s;
        }
        __syncthreads();                                 // the list is free again
        if (left == 0) break;
    }
}

}  // namespace hssfsst
