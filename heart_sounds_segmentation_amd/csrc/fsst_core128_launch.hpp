// fsst_core128_launch.hpp -- the launchers of fsst_core128_kernel (fsst_mfma128.hpp) as templates: the plain (two-launch) kernel
// of a row of kCore128Plain, the fused z-score kernel and the streaming step.  Included by the MFMA core's units only
// (fsst_core128_n128.hip, _n256.hip, _n512.hip, _n512_pairs.hip); each instantiates the kernels of its own rows and length behind
// the entry points that fsst_plan.hpp declares.
#pragma once
#include "fsst_plan.hpp"

#include "fsst_mfma128.hpp"

namespace hssfsst {
namespace host __attribute__((visibility("hidden"))) {

template <int NT, int RQ, bool FAST, int WPB, int S1C = -1, bool PAIR = false, bool RAGGED = false>
int launch_core128_wpb(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks)
{
    size_t lds = core128_lds_bytes(pl, WPB, PAIR);
    auto kern = hssfsst::fsst_core128_kernel<NT, RQ, kFpw128, FAST, WPB, S1C, false, false, PAIR, RAGGED>;
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = allow_full_lds(kern, pl->device, lds_ok)) return rc;
    int& slots = RAGGED ? pl->ragged_slots : pl->core128_slots;
    if (int rc = resident_blocks(pl, slots, kern, 64 * WPB, lds, false)) return rc;     // persistent grid = what is resident at once
    int64_t blocks = nchunks;                            // small launches: one chunk per block, spread over the CUs
    if (blocks > slots) blocks = slots;
    name_kernel(cx.kernel, WPB, blocks, "fsst_core128_kernel<%d, %d, %d, %s, %d, %d, false%s%s>", NT, RQ, kFpw128, FAST ? "true" : "false", WPB, S1C,
                PAIR ? ", pairs" : "", RAGGED ? ", ragged" : "");
    hssfsst::Core128Params cq = cp;
    if constexpr (PAIR) {                                // (a pair's bounded wait reports through the status word)
        if (int rcs = ensure_status(pl)) return rcs;
        cq.status = pl->d_status;
    }
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(blocks)), dim3(64 * WPB), lds, cx.st, cq);
    HIP_TRY(hipGetLastError());
    return 0;
}

// One rolling step in ONE launch (fsst_core128_kernel<.., STREAM>, fsst_mfma128.hpp): the chunk's groups, one per ticket, blocks
// bound to channels; tape append, transform, running-moments merge and normalisation.  Returns 1 when it launched, 0 when the
// step should take the three-launch route (a shape whose plain transform would not be this kernel's one-group chunks).
template <int NT, int RQ, int WPB, bool PAIR>
int launch_stream(hssfsst_plan* pl, float* tape_at, long long tape_len, const float* x_new_dev, long long x_stride, int channels, int chunk,
                  float* out, double* state, float* mirror, hipStream_t st)
{
    const int ngroups = (chunk + 15) / 16;
    const hssfsst::Core128Regions reg = hssfsst::core128_regions(ngroups, channels);
    if (!(reg.npc[0] == 0 && reg.npc[1] == 0 && reg.gpc[2] == 1)) return 0;      // (the plain kernel's chunks are not single groups)
    const size_t lds = core128_lds_bytes(pl, WPB, PAIR);
    if (lds > kMaxLdsBytes) return 0;
    auto kern = hssfsst::fsst_core128_kernel<NT, RQ, kFpw128, true, WPB, -1, false, true, PAIR>;
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = allow_full_lds(kern, pl->device, lds_ok)) return rc;
    if (int rc = resident_blocks(pl, pl->stream_slots, kern, 64 * WPB, lds, false)) return rc;
    if (state && pl->d_stream_arrive.cap < static_cast<size_t>(channels)) {
        if (int rc = pl->d_stream_arrive.grow(static_cast<size_t>(channels))) return rc;
        HIP_TRY(hipMemsetAsync(pl->d_stream_arrive.get(), 0, static_cast<size_t>(channels) * sizeof(unsigned), st));
    }
    if (state) {
        if (int rc = pl->d_stream_pieces.grow(static_cast<size_t>(channels) * ngroups * 4)) return rc;
    }
    if (int rcs = ensure_status(pl)) return rcs;
    int bpc = pl->stream_slots / channels;                // blocks per channel: spread a small step over the chip
    if (bpc > ngroups) bpc = ngroups;
    if (bpc < 1) bpc = 1;
    hssfsst::Core128Params cp = core128_params(pl);
    cp.x = tape_at; cp.xstride = tape_len; cp.out = out; cp.partials = nullptr;
    cp.n = pl->nwin - 1 + chunk; cp.nsig = channels; cp.col0 = pl->nwin / 2; cp.ncols = chunk; cp.reg = reg;
    cp.xnew = x_new_dev; cp.xnew_stride = x_stride; cp.hist = pl->nwin - 1; cp.bpc = bpc; cp.state = state; cp.arrive = pl->d_stream_arrive.get(); cp.pieces = pl->d_stream_pieces.get(); cp.mirror = mirror;
    const long long grid = static_cast<long long>(channels) * bpc;
    cp.status = pl->d_status;
    name_kernel(pl->last_kernel, WPB, grid, "fsst_core128_kernel<%d, %d, %d, true, %d, -1, false, stream%s>", NT, RQ, kFpw128, WPB, PAIR ? ", pairs" : "");
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(64 * WPB), lds, st, cp);
    HIP_TRY(hipGetLastError());
    return 1;
}

// Fused z-score launch (STACK; fsst_mfma128.hpp "Fused z-score"): one persistent block per CU, every CU owns whole signals.  FAST: the
// wide-store epilogue (nwin 128, even K <= 24); otherwise the general one (any K: nwin 256, or nwin 128 with an odd or wide band), whose
// z-score tickets sweep a chunk as float4s: every signal's feature block has to start on a 16-byte boundary.  Returns 1 when it launched, 0 when
// this exec should take the two-kernel path (signal too long for the LDS partials, or a batch that would leave CUs idle for a whole signal), < 0 on error.
template <int NT, int RQ, bool FAST, int WPB, int S1C>
int launch_fused(hssfsst_plan* pl, ExecCtx& cx, hssfsst::Core128Params cp, int64_t batch, int ngroups)
{
    if (ngroups > hssfsst::kFusedMaxGroups || (ngroups + kFpw128 / 16 - 1) / (kFpw128 / 16) < hssfsst::kFusedMinChunks) return 0;
    if (!FAST && (((static_cast<long long>(cp.ncols) * 2 * pl->K) & 3) != 0 || (reinterpret_cast<uintptr_t>(cp.out) & 15) != 0)) return 0;
    const size_t lds = core128_lds_bytes(pl, WPB, false) + (FAST ? hssfsst::kCtlFusedFloats - hssfsst::kCtlFloats : 0) * sizeof(float);
    if (lds > static_cast<size_t>(kMaxLdsBytes)) return 0;
    auto kern = hssfsst::fsst_core128_kernel<NT, RQ, kFpw128, FAST, WPB, S1C, true>;
    static std::atomic<unsigned long long> lds_ok{0};
    if (int rc = allow_full_lds(kern, pl->device, lds_ok)) return rc;
    if (int rc = resident_blocks(pl, pl->fused_slots, kern, 64 * WPB, lds, true)) return rc;       // one block per CU
    if (pl->fused_slots < 1) return 0;
    const int64_t grid = pl->fused_slots;
    if (!hssfsst::fused_rounds_full(batch, grid)) return 0;
    if (int rcs = ensure_status(pl)) return rcs;
    cp.status = pl->d_status;
    name_kernel(cx.kernel, WPB, grid, "fsst_core128_kernel<%d, %d, %d, %s, %d, %d, true>", NT, RQ, kFpw128, FAST ? "true" : "false", WPB, S1C);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(64 * WPB), lds, cx.st, cp);
    HIP_TRY(hipGetLastError());
    return 1;
}

// The plain (two-launch) core kernel of an MFMA plan: the row of kCore128Plain (fsst_launch_shape.hpp) that plan creation
// chose, turned into its instantiation by expanding that same table -- the rows that are MINE, the including unit's, and no
// other: hssfsst.hip sends a plan to the unit whose rows its (nt, rq, pair) are.  RAGGED: the instantiations of
// hssfsst_exec_ragged (the same rows, chunk list from the host).
template <bool (*MINE)(const hssfsst::Core128PlainRow&), bool RAGGED, size_t... I>
int launch_core128_row(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, std::index_sequence<I...>)
{
    using hssfsst::kCore128Plain;
    int rc = 0;
    (void)((static_cast<size_t>(pl->plain_row) == I && (rc = [&] {
                if constexpr (MINE(kCore128Plain[I]))
                    return launch_core128_wpb<kCore128Plain[I].nt, kCore128Plain[I].rq, kCore128Plain[I].fast, kCore128Plain[I].wpb, kCore128Plain[I].s1c,
                                              kCore128Plain[I].pair, RAGGED>(pl, cx, cp, nchunks);
                else return fail(HSSFSST_EINVAL, "launch_core128_row: row %d of the plain-kernel table is another unit's", pl->plain_row);
            }(), true)) || ...);
    return rc;
}
template <bool (*MINE)(const hssfsst::Core128PlainRow&)>
int launch_core128_rows(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, bool ragged)
{
    constexpr auto rows = std::make_index_sequence<hssfsst::kCore128PlainRows>{};
    return ragged ? launch_core128_row<MINE, true>(pl, cx, cp, nchunks, rows) : launch_core128_row<MINE, false>(pl, cx, cp, nchunks, rows);
}

}  // namespace host
}  // namespace hssfsst
