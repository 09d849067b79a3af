// segmenter_train.hpp -- kernels of the trainable BiLSTM layer (hssfsst.h: hssfsst_bilstm_*), beside the inference kernels of
// segmenter_lstm.hpp.
//
//   seg_pack_scale_kernel   max|W_hh| of both directions -> {wscale, inv_scale} in device memory (seg_upload_layer's arithmetic);
//   seg_pack_kernel         one layer's eight nn.LSTM tensors (device pointers) -> wt, bias and the split-f16 W_hh stream of the
//                           forward kernels, through the index functions seg_upload_layer walks on the host, plus the bf16 hi + lo
//                           stream of W_hh as the B operand of the backward product (seglayout::bwd_stream_source);
//   seg_rec_kernel<., true>   (segmenter_lstm.hpp) the forward recurrence, which also stores i, f, g, o, c of every step;
//   seg_bwd_rec_kernel      the backward recurrence: one workgroup per (direction, 16 batch rows), 8 waves, walks the steps against
//                           the forward order; dc and dh_rec stay in registers, dG goes through LDS as the split-bf16 A operand
//                           image and dh_rec = dG . W_hh runs on v_mfma_f32_16x16x32_bf16 (hi.hi + hi.lo + lo.hi) with W_hh
//                           streamed from L2 in the order the waves eat it; one barrier per step; no workgroup waits for another.
//
// RAGGED instantiations (hssfsst_bilstm_*_ragged): rows are the slots of segmenter_layout.hpp, everything is indexed by the step s a
// slot has walked, x / y / dy / dgates are arenas of sum T rows and the states come and go in list order through slot_rec.
//
// No host synchronisation anywhere: the scale never leaves the device.
#pragma once
#include <hip/hip_runtime.h>

#include "segmenter_layout.hpp"
#include "segmenter_lstm.hpp"

namespace hssfsst {

using seg_b8 = __bf16 __attribute__((ext_vector_type(8)));

constexpr int kSegBwdKb = 4 * kSegHp / 32;               // K blocks of the backward product: the 4 Hp gate columns

struct SegPackArgs {
    const float* src[8];    // {weight_ih, weight_hh, bias_ih, bias_hh} x {forward, reverse}
    int F, Fp, H;
    float* scale;           // {wscale, inv_scale = 1 / (wscale x kSegHScale)}
    float* wt;              // [dir][Fp][4 Hp]
    float* bias;            // [dir][4 Hp]
    _Float16* whh;          // forward stream (seglayout::fwd_stream_source)
    __bf16* bwd;            // backward stream (seglayout::bwd_stream_source)
};

// One block.  The power-of-two scale that puts the largest |W_hh| in [2^12, 2^13), as seg_upload_layer has it.
__global__ __launch_bounds__(1024) void seg_pack_scale_kernel(SegPackArgs a)
{
    __shared__ float part[16];
    const size_t n = static_cast<size_t>(4) * a.H * a.H;
    float m = 0.0f;
    for (int d = 0; d < 2; ++d) {
        const float* whh = a.src[4 * d + 1];
        for (size_t i = threadIdx.x; i < n; i += 1024) m = fmaxf(m, fabsf(whh[i]));
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 16; ++i) m = fmaxf(m, part[i]);
        int e = 0;
        float wscale = 1.0f;
        if (m > 0.0f && isfinite(m)) { (void)frexpf(m, &e); wscale = ldexpf(1.0f, 13 - e); }
        a.scale[0] = wscale;
        a.scale[1] = 1.0f / (wscale * kSegHScale);        // (powers of two: exact)
    }
}

// One thread per element of the larger of the four tables.
__global__ __launch_bounds__(256) void seg_pack_kernel(SegPackArgs a)
{
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const long long per_wt = static_cast<long long>(a.Fp) * seglayout::kGateCols;
    if (i < 2 * per_wt) {
        const int d = static_cast<int>(i / per_wt);
        const long long s = seglayout::wt_source(i - d * per_wt, a.F, a.H);
        a.wt[i] = s >= 0 ? a.src[4 * d][s] : 0.0f;
    }
    if (i < 2 * seglayout::kGateCols) {
        const int d = static_cast<int>(i / seglayout::kGateCols);
        const long long row = seglayout::gate_col_row(static_cast<int>(i % seglayout::kGateCols), a.H);
        a.bias[i] = row >= 0 ? a.src[4 * d + 2][row] + a.src[4 * d + 3][row] : 0.0f;
    }
    constexpr long long per_f = seglayout::kWtStreamHalves / 2, per_b = seglayout::kBwdStreamHalves / 2;
    if (i < 2 * per_f) {
        const int d = static_cast<int>(i / per_f);
        int lo = 0;
        const long long s = seglayout::fwd_stream_source(i - d * per_f, a.H, &lo);
        _Float16 out = static_cast<_Float16>(0.0f);
        if (s >= 0) {
            const float v = a.src[4 * d + 1][s] * a.scale[0];
            const _Float16 hi = static_cast<_Float16>(v);
            out = lo ? static_cast<_Float16>(v - static_cast<float>(hi)) : hi;
        }
        a.whh[i] = out;
    }
    if (i < 2 * per_b) {
        const int d = static_cast<int>(i / per_b);
        int lo = 0;
        const long long s = seglayout::bwd_stream_source(i - d * per_b, a.H, &lo);
        __bf16 out = static_cast<__bf16>(0.0f);
        if (s >= 0) {
            const float v = a.src[4 * d + 1][s];
            const __bf16 hi = static_cast<__bf16>(v);
            out = lo ? static_cast<__bf16>(v - static_cast<float>(hi)) : hi;
        }
        a.bwd[i] = out;
    }
}

// out0, out1 (2, B, H) <- state[0], state[1]: what seg_pair_init_kernel (segmenter_lstm.hpp) seeded, after the launches chained
// through it.  RAGGED: one thread per (slot, unit); slot b's state goes to row slot_rec[b] of the outputs, which are in list order.
template <bool RAGGED>
__global__ __launch_bounds__(256) void seg_pair_out_kernel(const float* state, float* out0, float* out1, int B, int H, int Bp,
                                                           const int* slot_rec)
{
    const int rows = RAGGED ? Bp : B;
    const size_t per = static_cast<size_t>(2) * rows * H;
    const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= 2 * per) return;
    const int which = static_cast<int>(i / per);
    const size_t r = i - which * per;
    const int u = static_cast<int>(r % H);
    const int b = static_cast<int>((r / H) % rows);
    const int dir = static_cast<int>(r / (static_cast<size_t>(H) * rows));
    const float v = state[((static_cast<size_t>(which) * 2 + dir) * Bp + b) * kSegHp + u];
    if constexpr (RAGGED) {
        const int rec = slot_rec[b];
        if (rec >= 0 && rec < B) (which ? out1 : out0)[(static_cast<size_t>(dir) * B + rec) * H + u] = v;
    } else {
        (which ? out1 : out0)[r] = v;
    }
}

struct SegBwdArgs {
    const float* stash;     // the training forward's (seglayout::stash_index)
    const float* c0;        // (2, B, H): c before the direction's first step
    const float* dy;        // (B, T, 2 H)
    const seg_b8* wbwd;     // [dir][wave][K block 32][tile 2][lane]{hi, lo}
    float* state;           // [dh_rec, dc][dir][Bp][Hp]: read at the start, written at the end (launches chain through it)
    float* dgates;          // (2, B, T, 4 H), nn.LSTM's gate order
    int B, T, H, Bp;
    int s0, n;              // this launch walks the direction's steps T - 1 - s0 downwards, n of them
    // RAGGED: dy is (sum T, 2 H) and dgates (2, sum T, 4 H) in arena order; B the recordings (rows of c0), Bp the slots; the stash
    // is the ragged forward's (seglayout::stash_index_ragged); a tile walks the steps min(s0 + n, walk) - 1 down to s0
    const long long* slot_off;
    const int* slot_len;
    const int* slot_rec;
    const int* tile_walk;
    const long long* tile_base;
    long long walked, total;    // tile_base[tiles] and sum T
};

// dG of one lane's (unit, gate, 4 rows) into the split-bf16 A-operand image [K block 32][k quarter][row 16][8], hi and lo planes.
// Gate column kappa = (unit tile * 4 + gate) * 16 + c, so K block = unit tile * 2 + gate / 2 and k = 16 (gate & 1) + c.
__device__ __forceinline__ void seg_put_dg(__bf16* hi, __bf16* lo, int unit, int gate, int row0, seg_f4 v)
{
    const int kb = (unit >> 4) * 2 + (gate >> 1), k = 16 * (gate & 1) + (unit & 15);
    const int base = ((kb * 4 + (k >> 3)) * kSegRows) * 8 + (k & 7);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const __bf16 x1 = static_cast<__bf16>(v[r]);
        const __bf16 x2 = static_cast<__bf16>(v[r] - static_cast<float>(x1));
        hi[base + (row0 + r) * 8] = x1;
        lo[base + (row0 + r) * 8] = x2;
    }
}

// Grid (batch tiles, 2 directions), block 512.  Step sigma of a direction is t = sigma (forward) or T - 1 - sigma (reverse); the
// launch walks sigma = T - 1 - s0 - s for s = 0 .. n - 1.  Wave w owns units (2 w + tl) * 16 + (lane & 15), rows 4 (lane >> 4) + r,
// as in the forward kernel, so a cell's dc, the dh_rec it receives and its stash never leave the lane.
// RAGGED: sigma is the step s of the slots.  Row r is live while sigma < len_r and stands at arena row off_r + sigma (forward) or
// off_r + len_r - 1 - sigma (reverse).  Until then its (dh_rec, dc) stay the seed of its recording through selects, it stores
// nothing and puts zeros into the dG image, so the product gives it nothing.  The trip count is the tile's, uniform in the
// workgroup; a live row's operations are the dense kernel's.
template <bool RAGGED>
__global__ __launch_bounds__(512) void seg_bwd_rec_kernel(SegBwdArgs a)
{
    constexpr int GB = kSegBwdKb * 4 * kSegRows * 8;                    // bf16 of one plane of the dG image: 32 KiB
    __shared__ __attribute__((aligned(16))) __bf16 gbuf[2][2][GB];     // [buffer][hi, lo]: 128 KiB
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int bt = blockIdx.x, dir = blockIdx.y;
    const int nbt = gridDim.x;
    const int row0 = (lane >> 4) * 4, b0 = bt * kSegRows;
    const size_t plane = static_cast<size_t>(2) * a.Bp * kSegHp;
    float* dhst = a.state + (static_cast<size_t>(dir) * a.Bp + b0) * kSegHp;
    float* dcst = dhst + plane;
    const int H4 = 4 * a.H;
    int n = a.n;
    if constexpr (RAGGED) n = min(a.n, a.tile_walk[bt] - a.s0);
    [[maybe_unused]] const int* rows = nullptr;                         // RAGGED: [len 16][first arena row 16][recording 16] in LDS
    [[maybe_unused]] long long base = 0;
    if constexpr (RAGGED) {
        __shared__ __attribute__((aligned(16))) int rows_lds[3 * kSegRows];
        if (tid < kSegRows) {
            rows_lds[tid] = a.slot_len[b0 + tid];
            rows_lds[kSegRows + tid] = static_cast<int>(a.slot_off[b0 + tid]);
            rows_lds[2 * kSegRows + tid] = a.slot_rec[b0 + tid];
        }
        __syncthreads();
        rows = rows_lds + row0;
        base = a.tile_base[bt];
    }

    seg_f4 dh[2], dc[2];
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) {
        const int unit = (w * 2 + tl) * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dh[tl][r] = dhst[(row0 + r) * kSegHp + unit];
            dc[tl][r] = dcst[(row0 + r) * kSegHp + unit];
        }
    }

    auto time_of = [&](int sigma) { return dir ? a.T - 1 - sigma : sigma; };
    auto stash_at = [&](int sigma, int tl) {
        if constexpr (RAGGED) return a.stash + seglayout::stash_index_ragged(a.walked, base, dir, sigma, w, tl, 0, lane, 0);
        else return a.stash + seglayout::stash_index(nbt, a.T, dir, bt, time_of(sigma), w, tl, 0, lane, 0);
    };
    // RAGGED: word k of row r's entry (the LDS address is hidden from the compiler: hoisted out of the step loop, the rows' ends
    // would be held in registers for the whole launch), and the arena row of row r at step sigma, -1 while the row is not live
    [[maybe_unused]] auto row_word = [&](int k, int r) {
        int hide = k * kSegRows + r;
        asm volatile("" : "+v"(hide));
        return rows[hide];
    };
    [[maybe_unused]] auto arena_row = [&](int sigma, int r) {
        const int len = row_word(0, r), off = row_word(1, r);
        return sigma < len ? off + (dir ? len - 1 - sigma : sigma) : -1;
    };
    // c before step sigma: the stash of step sigma - 1, or c0
    auto c_before = [&](int sigma, int tl) {
        seg_f4 v;
        if (sigma > 0) {
            v = *reinterpret_cast<const seg_f4*>(stash_at(sigma - 1, tl) + 4 * kSegTileFloats);
        } else {
            const int unit = (w * 2 + tl) * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (RAGGED) {
                    const int rec = row_word(2, r);
                    v[r] = rec >= 0 && unit < a.H ? a.c0[(static_cast<size_t>(dir) * a.B + rec) * a.H + unit] : 0.0f;
                } else {
                    const int b = b0 + row0 + r;
                    v[r] = b < a.B && unit < a.H ? a.c0[(static_cast<size_t>(dir) * a.B + b) * a.H + unit] : 0.0f;
                }
            }
        }
        return v;
    };
    auto dy_at = [&](int sigma, int tl) {
        seg_f4 v;
        const int unit = (w * 2 + tl) * 16 + (lane & 15), t = time_of(sigma);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if constexpr (RAGGED) {
                const int row = arena_row(sigma, r);
                v[r] = row >= 0 && unit < a.H ? a.dy[static_cast<size_t>(row) * (2 * a.H) + dir * a.H + unit] : 0.0f;
            } else {
                const int b = b0 + row0 + r;
                v[r] = b < a.B && unit < a.H ? a.dy[(static_cast<size_t>(b) * a.T + t) * (2 * a.H) + dir * a.H + unit] : 0.0f;
            }
        }
        return v;
    };

    // this wave's weight stream: per K block 2 output tiles of {hi, lo} x 64 lanes
    const seg_b8* const wq0 = a.wbwd + ((static_cast<size_t>(dir) * kSegWaves + w) * kSegBwdKb * 2 * 64 + lane) * 2;
    const int sig0 = RAGGED ? a.s0 + n - 1 : a.T - 1 - a.s0;

    // the first step's operands; every later step's are fetched one step ahead, behind the product
    seg_f4 gt[2][4], ct[2], cp[2], dyv[2];
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) {
#pragma unroll
        for (int q = 0; q < 4; ++q) gt[tl][q] = *reinterpret_cast<const seg_f4*>(stash_at(sig0, tl) + q * kSegTileFloats);
        ct[tl] = *reinterpret_cast<const seg_f4*>(stash_at(sig0, tl) + 4 * kSegTileFloats);
        cp[tl] = c_before(sig0, tl);
        dyv[tl] = dy_at(sig0, tl);
    }

    seg_b8 wb[2][2][2][2];                                              // double buffer of two K blocks x 2 tiles x {hi, lo}
#pragma unroll
    for (int q = 0; q < 8; ++q) wb[0][q >> 2][(q >> 1) & 1][q & 1] = wq0[(q >> 1) * 64 * 2 + (q & 1)];

    int cur = 0;
    for (int s = 0; s < n; ++s) {
        const int sigma = sig0 - s, t = time_of(sigma);
        [[maybe_unused]] int arow[4], lives = 0;                         // RAGGED: the rows' arena rows at this step, -1: not live
        if constexpr (RAGGED) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                arow[r] = arena_row(sigma, r);
                lives |= (arow[r] >= 0) << r;
            }
        }
#pragma unroll
        for (int tl = 0; tl < 2; ++tl) {
            const int unit = (w * 2 + tl) * 16 + (lane & 15);
            seg_f4 dg[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float gi = gt[tl][0][r], gf = gt[tl][1][r], gg = gt[tl][2][r], go = gt[tl][3][r];
                const float d = dyv[tl][r] + dh[tl][r];
                const float tc = seg_tanh(ct[tl][r]);
                dg[3][r] = d * tc * go * (1.0f - go);
                const float dcv = fmaf(d * go, 1.0f - tc * tc, dc[tl][r]);
                dg[0][r] = dcv * gg * gi * (1.0f - gi);
                dg[2][r] = dcv * gi * (1.0f - gg * gg);
                dg[1][r] = dcv * cp[tl][r] * gf * (1.0f - gf);
                if constexpr (RAGGED) {
                    const bool live = arow[r] >= 0;
                    dc[tl][r] = live ? dcv * gf : dc[tl][r];
#pragma unroll
                    for (int q = 0; q < 4; ++q) dg[q][r] = live ? dg[q][r] : 0.0f;
                    if (live && unit < a.H) {
                        float* dst = a.dgates + (static_cast<size_t>(dir) * a.total + arow[r]) * H4 + unit;
#pragma unroll
                        for (int q = 0; q < 4; ++q) dst[q * a.H] = dg[q][r];
                    }
                } else {
                    dc[tl][r] = dcv * gf;
                    const int b = b0 + row0 + r;
                    if (b < a.B && unit < a.H) {
                        float* dst = a.dgates + ((static_cast<size_t>(dir) * a.B + b) * a.T + t) * H4 + unit;
#pragma unroll
                        for (int q = 0; q < 4; ++q) dst[q * a.H] = dg[q][r];
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) seg_put_dg(gbuf[cur][0], gbuf[cur][1], unit, q, row0, dg[q]);
            ct[tl] = cp[tl];                                             // c before this step is c of the next one walked
        }
        if (s + 1 < n) {
#pragma unroll
            for (int tl = 0; tl < 2; ++tl) {
#pragma unroll
                for (int q = 0; q < 4; ++q) gt[tl][q] = *reinterpret_cast<const seg_f4*>(stash_at(sigma - 1, tl) + q * kSegTileFloats);
                cp[tl] = c_before(sigma - 1, tl);
                dyv[tl] = dy_at(sigma - 1, tl);
            }
        }
        // every wave wrote its part of gbuf[cur]; the other buffer is written next step, after every wave passed this barrier
        // and so finished reading it: one barrier per step
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");

        // (the stream's addresses do not change from step to step: hidden from the compiler, as in the forward kernel)
        int zero = 0;
        asm volatile("" : "+v"(zero));
        const seg_b8* wq = wq0 + zero;
        const seg_b8* ahi = reinterpret_cast<const seg_b8*>(gbuf[cur][0]) + lane;
        const seg_b8* alo = reinterpret_cast<const seg_b8*>(gbuf[cur][1]) + lane;
        seg_f4 acc[2] = {seg_f4{0.0f, 0.0f, 0.0f, 0.0f}, seg_f4{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
        for (int i = 0; i < kSegBwdKb / 2; ++i) {                        // pairs of K blocks
            const int cb = i & 1, nb = cb ^ 1;
            const int ni = i + 1 < kSegBwdKb / 2 ? i + 1 : 0;           // (the last one fetches the next step's first: same weights)
#pragma unroll
            for (int q = 0; q < 8; ++q) wb[nb][q >> 2][(q >> 1) & 1][q & 1] = wq[(ni * 4 + (q >> 1)) * 64 * 2 + (q & 1)];
            __builtin_amdgcn_sched_barrier(0);                          // (the loads stay ahead of the products they overlap)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const seg_b8 xh = ahi[(2 * i + k) * 64], xl = alo[(2 * i + k) * 64];
#pragma unroll
                for (int ot = 0; ot < 2; ++ot) {
                    acc[ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wb[cb][k][ot][0], acc[ot], 0, 0, 0);
                    acc[ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, wb[cb][k][ot][1], acc[ot], 0, 0, 0);
                    acc[ot] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, wb[cb][k][ot][0], acc[ot], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (RAGGED) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = (lives >> r) & 1;
                dh[0][r] = live ? acc[0][r] : dh[0][r];
                dh[1][r] = live ? acc[1][r] : dh[1][r];
            }
        } else {
            dh[0] = acc[0];
            dh[1] = acc[1];
        }
        cur ^= 1;
    }
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) {
        const int unit = (w * 2 + tl) * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            dhst[(row0 + r) * kSegHp + unit] = dh[tl][r];
            dcst[(row0 + r) * kSegHp + unit] = dc[tl][r];
        }
    }
}

}  // namespace hssfsst
