// segmenter_lstm.hpp -- inference kernels of the BiLSTM segmenter (hssfsst.h: hssfsst_segmenter_exec).
//
// The reference's HeartSoundSegmenter.forward (hss/model/segmenter.py:70-87): BiLSTM -> ReLU -> BiLSTM seeded with the first
// layer's final (h, c) -> ReLU -> Linear(2H -> 4) -> log_softmax.  Three kernels per layer chunk plus one head pass:
//
//   seg_proj_kernel   pre[dir][batch tile][t][gate tile][lane] = x[b, t, :] . W_ih^T + b_ih + b_hh for both directions, exact f32
//                     matrix instruction (v_mfma_f32_16x16x4_f32), LDS tiled, parallel over time; written in the register
//                     image of the recurrence's accumulators so that kernel reads one float4 per lane and tile;
//   seg_rec_kernel    the recurrence: one workgroup per (direction, 16 batch rows), 8 waves, loops over the chunk's steps itself;
//                     h (as split f16 operands, in LDS) and c (registers) never leave the CU; h . W_hh^T as f16 hi + lo products
//                     (hi.hi + hi.lo + lo.hi) on v_mfma_f32_16x16x32_f16 with W_hh streamed from L2 in the order the waves eat it;
//                     no workgroup waits for another one;
//   seg_head_kernel   ReLU -> Linear -> log_softmax, one wave per (b, t).
//
// Every hidden size runs on the one padded geometry kSegHp = 256 units (16 unit tiles x 4 gates, K = 256): padded units have zero
// weights and zero state, so they stay exactly zero (i = f = o = 1/2, g = 0, c' = c / 2 = 0); the projection writes their gate
// columns as zero whatever x holds (seg_proj_kernel's epilogue), so an infinite feature does not reach them as 0 . Inf.
//
// RAGGED instantiations (hssfsst_segmenter_exec_ragged): the 16 rows of a tile are SLOTS, each holding a whole recording of its own
// length from an arena (segmenter_layout.hpp: longest first, so the tiles still walking are a prefix).  Everything is indexed by the
// step s a slot has walked, not by time: slot b is live while s < T_b and stands at t = s (forward) or t = T_b - 1 - s (reverse), so
// both directions start together and a launch covers steps s0 .. s0 + n of its tiles.  A slot past its end freezes: selects keep c
// and h (hence the h image), nothing is stored to y, and the state written back is the recording's own final state.  A live row's
// arithmetic is the dense kernel's, instruction for instruction: a recording's bits are those of the dense call on it alone.
#pragma once
#include <hip/hip_runtime.h>

#include "segmenter_layout.hpp"

namespace hssfsst {

constexpr int kSegHp = 256;                    // padded hidden size == the supported maximum
constexpr int kSegRows = 16;                   // batch rows of one workgroup (the matrix instruction's M)
constexpr int kSegWaves = 8;                   // waves of a recurrence workgroup; each owns two unit tiles (x 4 gates)
constexpr int kSegKb = kSegHp / 32;            // K blocks of the recurrent product
constexpr int kSegGateTiles = 4 * kSegHp / 16; // 16-column tiles of a direction's 4 Hp gate columns: tile = unit tile * 4 + gate
constexpr int kSegTileFloats = 256;            // one 16 x 16 tile as the accumulator image [lane 64][4]
constexpr float kSegHScale = 1024.0f;          // power-of-two scale of h before the f16 split (|h| < 1)

using seg_h8 = _Float16 __attribute__((ext_vector_type(8)));
using seg_f4 = float __attribute__((ext_vector_type(4)));

// element type of a layer input: 0 float32, 2 float16, 3 bfloat16 (HSSFSST_DTYPE_*), converted on load
__device__ __forceinline__ float seg_load_x(const void* x, size_t i, int dtype)
{
    if (dtype == 2) return static_cast<float>(static_cast<const _Float16*>(x)[i]);
    if (dtype == 3) return static_cast<float>(static_cast<const __bf16*>(x)[i]);
    return static_cast<const float*>(x)[i];
}

// ReLU as torch.relu has it: a NaN stays a NaN (fmaxf(NaN, 0) is 0, which made a row without a single valid number look like a
// confident one).  One compare and one select; every other value keeps its bits.
__device__ __forceinline__ float seg_relu(float v) { return v < 0.0f ? 0.0f : v; }

struct SegProjArgs {
    const void* x;          // (B, T, F) of x_dtype
    int x_dtype, relu;      // relu: rectify on load (layer 2 reads layer 1's un-rectified output)
    int B, T, F, Fp;        // Fp = F rounded up to 32: rows of wt
    int H;                  // hidden size: the gate columns of units H .. Hp - 1 are padding and are written as zero
    const float* wt;        // [dir][Fp][4 Hp]: W_ih transposed, columns permuted to (unit tile, gate, unit), zero padded
    const float* bias;      // [dir][4 Hp]: b_ih + b_hh, same column order
    float* pre;             // [dir][batch tile][Tc][gate tile][lane][4]
    int Tc, n;              // chunk pitch of pre and the steps of this launch
    int t0[2];              // first time step of the launch's chunk, per direction
    // RAGGED: x is the arena (sum T, F); pre is indexed by step; n is the longest walk of the launch (tile 0's), Tc the pitch
    const long long* slot_off;   // [slots] first arena row of the slot's recording
    const int* slot_len;         // [slots] its steps (0: padding slot)
    const int* tile_walk;        // [tiles] the tile's longest recording
    int s0;                      // first step of the launch
};

// Block = 4 waves: 8 time steps x 16 batch rows (M = 128) by 64 gate columns; wave w: steps 2w, 2w + 1, all four column tiles.
// Grid (16 column blocks, batch tiles x ceil(n / 8), 2 directions).  RAGGED: row (step, slot) gathers x[offset + t(step, dir)], zero
// past the slot's end; blocks past their tile's walk exit at once.
template <bool RAGGED>
__global__ __launch_bounds__(256) void seg_proj_kernel(SegProjArgs a)
{
    constexpr int KB = 32, AS = KB + 1, BS = 80;
    __shared__ float As[128 * AS];
    __shared__ __attribute__((aligned(16))) float Bs[KB * BS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int dir = blockIdx.z;
    const int tblocks = (a.n + 7) / 8;
    const int bt = blockIdx.y / tblocks, tb = blockIdx.y - bt * tblocks;
    const int n0 = blockIdx.x * 64;
    const int nbt = RAGGED ? static_cast<int>(gridDim.y) / tblocks : (a.B + kSegRows - 1) / kSegRows;
    int nt = a.n;                                                       // steps of this tile in the launch
    if constexpr (RAGGED) {
        nt = min(a.n, a.tile_walk[bt] - a.s0);
        if (tb * 8 >= nt) return;
    }
    const float* wt = a.wt + static_cast<size_t>(dir) * a.Fp * (4 * kSegHp);
    seg_f4 acc[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = seg_f4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < a.Fp; k0 += KB) {
        // A: row m = step * 16 + batch row, 32 consecutive k per 32 threads
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int m = (tid >> 5) + 8 * i, k = k0 + (tid & 31);
            const int tl = tb * 8 + (m >> 4), b = bt * kSegRows + (m & 15);
            float v = 0.0f;
            if constexpr (RAGGED) {
                const int len = a.slot_len[b], s = a.s0 + tl;           // (b is the slot)
                if (s < len && k < a.F) {
                    const long long row = a.slot_off[b] + (dir ? len - 1 - s : s);
                    v = seg_load_x(a.x, static_cast<size_t>(row) * a.F + k, a.x_dtype);
                    if (a.relu) v = seg_relu(v);
                }
            } else if (tl < a.n && b < a.B && k < a.F) {
                v = seg_load_x(a.x, (static_cast<size_t>(b) * a.T + (a.t0[dir] + tl)) * a.F + k, a.x_dtype);
                if (a.relu) v = seg_relu(v);
            }
            As[m * AS + (tid & 31)] = v;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + 256 * i, k = e >> 4, c4 = (e & 15) * 4;
            const float4 v = *reinterpret_cast<const float4*>(wt + static_cast<size_t>(k0 + k) * (4 * kSegHp) + n0 + c4);
            *reinterpret_cast<float4*>(&Bs[k * BS + c4]) = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < KB / 4; ++kk) {
            const int k = kk * 4 + (lane >> 4);
            const float a0 = As[((2 * w) * 16 + (lane & 15)) * AS + k], a1 = As[((2 * w + 1) * 16 + (lane & 15)) * AS + k];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float b = Bs[k * BS + i * 16 + (lane & 15)];
                acc[0][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b, acc[0][i], 0, 0, 0);
                acc[1][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b, acc[1][i], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // accumulator image: lane l, register r = row 4 (l >> 4) + r (batch row), column l & 15
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int tl = tb * 8 + 2 * w + j;
        if (tl >= nt) continue;
        float* dst = a.pre + ((static_cast<size_t>(dir) * nbt + bt) * a.Tc + tl) * (kSegGateTiles * kSegTileFloats);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int col = n0 + i * 16, unit0 = (col >> 6) * 16;           // column = (unit tile x 4 + gate) x 16 + unit
            const float bv = a.bias[dir * (4 * kSegHp) + col + (lane & 15)];
            seg_f4 v = acc[j][i];
            v += bv;
            // a padded unit's column holds zero weights and a zero bias: 0 for every finite x, but 0 . Inf = NaN, and a NaN in a
            // padded unit's h reaches every real unit of the row through the zero rows of W_hh.  Written as the zero it stands for.
            if (unit0 + (lane & 15) >= a.H) v = seg_f4{0.0f, 0.0f, 0.0f, 0.0f};
            *reinterpret_cast<seg_f4*>(dst + (col >> 4) * kSegTileFloats + lane * 4) = v;
        }
    }
}

// state[0][dir][padded batch][Hp] <- p0, state[1] <- p1, both (2, B, H), either NULL for zero; the padding is zero.  The forwards
// seed (h, c) with it, the backwards (dh_rec, dc).  RAGGED: row b is a slot and takes the row of its recording slot_rec[b] (none:
// a padding slot, zero); B is the rows of p0 / p1, 1 = the same row for every recording.
template <bool RAGGED>
__global__ __launch_bounds__(256) void seg_pair_init_kernel(const float* p0, const float* p1, float* state, int B, int H, int Bp,
                                                            const int* slot_rec)
{
    const size_t per = static_cast<size_t>(2) * Bp * kSegHp;
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= 2 * per) return;
    const int which = static_cast<int>(i / per);
    const size_t r = i - which * per;
    const int u = static_cast<int>(r % kSegHp);
    const int b = static_cast<int>((r / kSegHp) % Bp);
    const int dir = static_cast<int>(r / (static_cast<size_t>(kSegHp) * Bp));
    const float* src = which ? p1 : p0;
    int row = b;
    if constexpr (RAGGED) {
        row = slot_rec[b];
        if (B == 1 && row > 0) row = 0;
    }
    state[i] = src != nullptr && row >= 0 && row < B && u < H ? src[(static_cast<size_t>(dir) * B + row) * H + u] : 0.0f;
}

struct SegRecArgs {
    const float* pre;       // [dir][batch tile][Tc][gate tile][lane][4]
    const seg_h8* whh;      // [dir][wave][K block][tile x gate][lane]{hi, lo}: W_hh x wscale, split, in consumption order
    float* state;           // [h, c][dir][Bp][Hp]: read at the start, written at the end (chunks and layers chain through it)
    float* y;               // (B, T, 2 H) float32 layer output, un-rectified
    int B, T, H, Bp, Tc, n;
    int t0[2];
    float inv_scale;        // 1 / (wscale x kSegHScale)
    // RAGGED: y is (sum T, 2 H) in arena order; Bp the slots; the launch's tiles walk steps s0 .. s0 + min(Tc, walk - s0)
    const long long* slot_off;
    const int* slot_len;
    const int* tile_walk;
    int s0;
    // TRAIN (segmenter_train.hpp): what the backward pass needs of every step, and the scale where the device-side pack left it
    float* stash;               // [dir][batch tile][T][wave][tile of the wave][i, f, g, o, c][lane][4] (seglayout::stash_index)
    const float* inv_scale_dev;
    // RAGGED and TRAIN: the stash is indexed by step, a tile's pitch is its walk (seglayout::stash_index_ragged)
    const long long* tile_base; // [tiles + 1] prefix sums of tile_walk
    long long walked;           // tile_base[tiles]
};

__device__ __forceinline__ float seg_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float seg_tanh(float x) { return 2.0f * __builtin_amdgcn_rcpf(1.0f + __expf(-2.0f * x)) - 1.0f; }

// h of one lane's (unit, 4 rows) into the split-f16 A-operand image: [K block][k quarter][row 16][8 halves], hi and lo planes
__device__ __forceinline__ void seg_put_h(_Float16* hi, _Float16* lo, int unit, int row0, seg_f4 h)
{
    const int base = ((unit >> 3) * kSegRows) * 8 + (unit & 7);          // ((kb * 4 + quarter) * 16 + row) * 8 + j
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float v = h[r] * kSegHScale;
        const _Float16 x1 = static_cast<_Float16>(v);
        const _Float16 x2 = static_cast<_Float16>(v - static_cast<float>(x1));
        hi[base + (row0 + r) * 8] = x1;
        lo[base + (row0 + r) * 8] = x2;
    }
}

// Grid (batch tiles, 2 directions), block 512.  Direction 0 walks the chunk's steps upwards, direction 1 downwards.  RAGGED: both
// walk step indices upwards; the trip count is the tile's (uniform in the workgroup), the rows' ends are selects.
// TRAIN: the same arithmetic; each wave also stores the activated gates and c of the cells it holds, per step.
// RAGGED and TRAIN: a step of the tile is stored for all 16 rows (a float4 of the stash spans four); what an ended row leaves there
// is finite and never read.  The rows' ends live in LDS and the gates are taken one at a time -- activated, stored, folded into
// c -- so that no register is held for them: the kernel has none to spare.  A live row's operations are the dense kernel's.
template <bool RAGGED, bool TRAIN = false>
__global__ __launch_bounds__(512) void seg_rec_kernel(SegRecArgs a)
{
    constexpr int HB = kSegKb * 4 * kSegRows * 8;                       // halves of one plane of the h image
    __shared__ __attribute__((aligned(16))) _Float16 hbuf[2][2][HB];   // [buffer][hi, lo]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int bt = blockIdx.x, dir = blockIdx.y;
    const int nbt = gridDim.x;
    const int row0 = (lane >> 4) * 4, b0 = bt * kSegRows;
    const size_t plane = static_cast<size_t>(2) * a.Bp * kSegHp;
    float* hst = a.state + (static_cast<size_t>(dir) * a.Bp + b0) * kSegHp;
    float* cst = hst + plane;
    const int n = RAGGED ? min(a.Tc, a.tile_walk[bt] - a.s0) : a.n;
    float inv_scale = a.inv_scale;
    if constexpr (TRAIN) inv_scale = *a.inv_scale_dev;
    [[maybe_unused]] int rem[4], yrow[4];                               // RAGGED: row r is live while s < rem[r]; its y row at s = 0
    [[maybe_unused]] const int* ends = nullptr;                         // RAGGED and TRAIN: the same two, [rem 16][yrow 16] in LDS
    [[maybe_unused]] float* sp0 = nullptr;                              // ... and this lane's place in the stash at step s0
    if constexpr (RAGGED && TRAIN) {
        __shared__ __attribute__((aligned(16))) int ends_lds[2 * kSegRows];
        if (tid < kSegRows) {
            const int len = a.slot_len[b0 + tid], off = static_cast<int>(a.slot_off[b0 + tid]);
            ends_lds[tid] = len - a.s0;
            ends_lds[kSegRows + tid] = dir ? off + len - a.s0 - 1 : off + a.s0;
        }
        ends = ends_lds + row0;
        sp0 = a.stash + seglayout::stash_index_ragged(a.walked, a.tile_base[bt], dir, a.s0, w, 0, 0, lane, 0);
    } else if constexpr (RAGGED) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int len = a.slot_len[b0 + row0 + r], off = static_cast<int>(a.slot_off[b0 + row0 + r]);
            rem[r] = len - a.s0;
            yrow[r] = dir ? off + rem[r] - 1 : off + a.s0;
        }
    }

    seg_f4 c[2], h[2];
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) {
        const int unit = (w * 2 + tl) * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            h[tl][r] = hst[(row0 + r) * kSegHp + unit];
            c[tl][r] = cst[(row0 + r) * kSegHp + unit];
        }
        seg_put_h(hbuf[0][0], hbuf[0][1], unit, row0, h[tl]);
    }

    // this wave's weight stream: per K block 8 (tile, gate) fragments of {hi, lo} x 64 lanes
    const seg_h8* const wq0 = a.whh + ((static_cast<size_t>(dir) * kSegWaves + w) * kSegKb * 8 * 64 + lane) * 2;
    const seg_h8* wq = wq0;
    const float* prew = a.pre + (static_cast<size_t>(dir) * nbt + bt) * a.Tc * (kSegGateTiles * kSegTileFloats)
                        + (w * 8) * kSegTileFloats + lane * 4;
    auto pre_at = [&](int s) { return prew + static_cast<size_t>(!RAGGED && dir ? n - 1 - s : s) * (kSegGateTiles * kSegTileFloats); };

    seg_h8 wres[8][2];                                                  // K block 0 of every tile: resident for the whole launch
    seg_h8 wb[2][4][2];                                                 // the rest streams: double buffer of half a K block
    seg_f4 pn[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        wres[q][0] = wq[q * 128];
        wres[q][1] = wq[q * 128 + 1];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        wb[0][q][0] = wq[(8 + q) * 128];
        wb[0][q][1] = wq[(8 + q) * 128 + 1];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) pn[q] = *reinterpret_cast<const seg_f4*>(pre_at(0) + q * kSegTileFloats);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");

    int cur = 0;
    for (int s = 0; s < n; ++s) {
        // (the stream's addresses do not change from step to step: hidden from the compiler, which would otherwise hoist the
        // loads out of the time loop and spill what it cannot hold)
        int zero = 0;
        asm volatile("" : "+v"(zero));
        wq = wq0 + zero;
        seg_f4 acc[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] = seg_f4{0.0f, 0.0f, 0.0f, 0.0f};
        const seg_h8* ahi = reinterpret_cast<const seg_h8*>(hbuf[cur][0]) + lane;
        const seg_h8* alo = reinterpret_cast<const seg_h8*>(hbuf[cur][1]) + lane;
        {
            const seg_h8 xh = ahi[0], xl = alo[0];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wres[q][0], acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wres[q][1], acc[q], 0, 0, 0);
                acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, wres[q][0], acc[q], 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 2; i < 2 * kSegKb; ++i) {                          // half K blocks: fragments 4 (i & 1) .. + 3 of block i / 2
            const int nb = (i + 1) & 1, cb = i & 1;
            const int ni = i + 1 < 2 * kSegKb ? i + 1 : 2;              // (the last one fetches the next step's first: same weights)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                wb[nb][q][0] = wq[(ni * 4 + q) * 128];
                wb[nb][q][1] = wq[(ni * 4 + q) * 128 + 1];
            }
            __builtin_amdgcn_sched_barrier(0);                          // (the loads stay ahead of the products they overlap)
            const seg_h8 xh = ahi[(i >> 1) * 64], xl = alo[(i >> 1) * 64];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int g = 4 * (i & 1) + q;
                acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wb[cb][q][0], acc[g], 0, 0, 0);
                acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wb[cb][q][1], acc[g], 0, 0, 0);
                acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, wb[cb][q][0], acc[g], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const int t = RAGGED ? 0 : a.t0[dir] + (dir ? n - 1 - s : s);
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            const int unit = (w * 2 + tl) * 16 + (lane & 15);
            if constexpr (RAGGED && TRAIN) {
                float* sp = sp0 + static_cast<size_t>(s) * seglayout::kStashStepFloats + tl * (seglayout::kStashQ * kSegTileFloats);
                seg_f4 u, v;
#pragma unroll
                for (int r = 0; r < 4; ++r) u[r] = seg_sigmoid(fmaf(acc[tl * 4 + 0][r], inv_scale, pn[tl * 4 + 0][r]));
                *reinterpret_cast<seg_f4*>(sp) = u;
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = seg_tanh(fmaf(acc[tl * 4 + 2][r], inv_scale, pn[tl * 4 + 2][r]));
                *reinterpret_cast<seg_f4*>(sp + 2 * kSegTileFloats) = v;
#pragma unroll
                for (int r = 0; r < 4; ++r) u[r] = u[r] * v[r];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = seg_sigmoid(fmaf(acc[tl * 4 + 1][r], inv_scale, pn[tl * 4 + 1][r]));
                *reinterpret_cast<seg_f4*>(sp + kSegTileFloats) = v;
#pragma unroll
                for (int r = 0; r < 4; ++r) u[r] = fmaf(v[r], c[tl][r], u[r]);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = seg_sigmoid(fmaf(acc[tl * 4 + 3][r], inv_scale, pn[tl * 4 + 3][r]));
                *reinterpret_cast<seg_f4*>(sp + 3 * kSegTileFloats) = v;
                // (the address is hidden like the weight stream's: hoisted, the eight values would be held for the whole launch)
                const int4 rm = *reinterpret_cast<const int4*>(ends + zero);
                const int4 yr = *reinterpret_cast<const int4*>(ends + kSegRows + zero);
                const int rmv[4] = {rm.x, rm.y, rm.z, rm.w}, yrv[4] = {yr.x, yr.y, yr.z, yr.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool live = s < rmv[r];
                    const float hn = v[r] * seg_tanh(u[r]);
                    c[tl][r] = live ? u[r] : c[tl][r];
                    h[tl][r] = live ? hn : h[tl][r];
                    const int row = dir ? yrv[r] - s : yrv[r] + s;
                    if (live && unit < a.H) a.y[static_cast<size_t>(row) * (2 * a.H) + dir * a.H + unit] = hn;
                }
                *reinterpret_cast<seg_f4*>(sp + 4 * kSegTileFloats) = c[tl];
            } else {
                [[maybe_unused]] seg_f4 sg[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float gi = seg_sigmoid(fmaf(acc[tl * 4 + 0][r], inv_scale, pn[tl * 4 + 0][r]));
                    const float gf = seg_sigmoid(fmaf(acc[tl * 4 + 1][r], inv_scale, pn[tl * 4 + 1][r]));
                    const float gg = seg_tanh(fmaf(acc[tl * 4 + 2][r], inv_scale, pn[tl * 4 + 2][r]));
                    const float go = seg_sigmoid(fmaf(acc[tl * 4 + 3][r], inv_scale, pn[tl * 4 + 3][r]));
                    if constexpr (RAGGED) {
                        const bool live = s < rem[r];
                        const float cn = fmaf(gf, c[tl][r], gi * gg);
                        const float hn = go * seg_tanh(cn);
                        c[tl][r] = live ? cn : c[tl][r];
                        h[tl][r] = live ? hn : h[tl][r];
                        const int row = dir ? yrow[r] - s : yrow[r] + s;
                        if (live && unit < a.H) a.y[static_cast<size_t>(row) * (2 * a.H) + dir * a.H + unit] = hn;
                    } else {
                        c[tl][r] = fmaf(gf, c[tl][r], gi * gg);
                        h[tl][r] = go * seg_tanh(c[tl][r]);
                        const int b = b0 + row0 + r;
                        if (b < a.B && unit < a.H) a.y[(static_cast<size_t>(b) * a.T + t) * (2 * a.H) + dir * a.H + unit] = h[tl][r];
                        if constexpr (TRAIN) { sg[0][r] = gi; sg[1][r] = gf; sg[2][r] = gg; sg[3][r] = go; }
                    }
                }
                if constexpr (TRAIN) {
                    float* sp = a.stash + seglayout::stash_index(nbt, a.T, dir, bt, t, w, tl, 0, lane, 0);
#pragma unroll
                    for (int q = 0; q < 4; ++q) *reinterpret_cast<seg_f4*>(sp + q * kSegTileFloats) = sg[q];
                    *reinterpret_cast<seg_f4*>(sp + 4 * kSegTileFloats) = c[tl];
                }
            }
            seg_put_h(hbuf[cur ^ 1][0], hbuf[cur ^ 1][1], unit, row0, h[tl]);
        }
        if (s + 1 < n) {                                                 // the next step's pre: a barrier and a product away from its use
            const float* pp = pre_at(s + 1);
#pragma unroll
            for (int q = 0; q < 8; ++q) pn[q] = *reinterpret_cast<const seg_f4*>(pp + q * kSegTileFloats);
        }
        // every wave has read hbuf[cur] before it wrote hbuf[cur ^ 1]: one barrier per step.  (Not __syncthreads: that would
        // also wait for the weight and pre loads in flight for the next step.)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        cur ^= 1;
    }
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) {
        const int unit = (w * 2 + tl) * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            hst[(row0 + r) * kSegHp + unit] = h[tl][r];
            cst[(row0 + r) * kSegHp + unit] = c[tl][r];
        }
    }
}

// logp[b, t, :] = log_softmax(W . relu(y[b, t, :]) + bias): one wave per row, four rows per block
__global__ __launch_bounds__(256) void seg_head_kernel(const float* y, const float* lw, const float* lb, float* logp, long long rows, int H2)
{
    const int lane = threadIdx.x & 63;
    const long long row = static_cast<long long>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* yr = y + row * H2;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    for (int k = lane; k < H2; k += 64) {
        const float v = seg_relu(yr[k]);
        s0 = fmaf(v, lw[k], s0);
        s1 = fmaf(v, lw[H2 + k], s1);
        s2 = fmaf(v, lw[2 * H2 + k], s2);
        s3 = fmaf(v, lw[3 * H2 + k], s3);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        s0 += __shfl_xor(s0, m);
        s1 += __shfl_xor(s1, m);
        s2 += __shfl_xor(s2, m);
        s3 += __shfl_xor(s3, m);
    }
    if (lane == 0) {
        s0 += lb[0]; s1 += lb[1]; s2 += lb[2]; s3 += lb[3];
        const float mx = fmaxf(fmaxf(s0, s1), fmaxf(s2, s3));
        const float lse = mx + logf(expf(s0 - mx) + expf(s1 - mx) + expf(s2 - mx) + expf(s3 - mx));
        *reinterpret_cast<float4*>(logp + row * 4) = make_float4(s0 - lse, s1 - lse, s2 - lse, s3 - lse);
    }
}

}  // namespace hssfsst
