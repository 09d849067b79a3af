// fsst_ragged.hpp -- the z-score of a ragged exec (hssfsst_exec_ragged): FSST._stack_real_imag (synchrosqueeze.py:78-85) for a
// list of signals of different lengths whose features lie back to back in one buffer.  Two launches for the whole list, as the
// two-launch path of a dense batch: per-signal statistics from the core kernel's partials (the arithmetic and order of
// fsst_stats_kernel: signal_stats), then one sweep whose blocks take UNITS of about kRaggedUnitFloats floats -- a long recording
// is spread over many blocks, a short one is one unit.  The z-score is elementwise, (v - mean) * (1 / std) in float32, so the
// results are bit-identical to a single exec of each signal, whichever path that takes.
#pragma once

#include "fsst_mfma128_device.hpp"

namespace hssfsst {

// (kRaggedUnitFloats, the floats of a z-score unit: fsst_launch_shape.hpp -- the host cuts the list into units with it)

// stats[s] = {mean_re, 1/std_re, mean_im, 1/std_im} of signal s; one wave per signal
__global__ __launch_bounds__(64) void fsst_ragged_stats_kernel(const float* partials, const RaggedSignal* sig, float4* stats, int K)
{
    const RaggedSignal s = sig[blockIdx.x];
    const float4 st = signal_stats(partials + s.poff, (s.n + 15) >> 4, 16, s.n, K, threadIdx.x & 63);
    if (threadIdx.x == 0) stats[blockIdx.x] = st;
}

// unit0[s] .. unit0[s + 1] - 1: the units of signal s (unit0[nsig] = all units).  Block u (grid-stride) finds its signal by
// bisection and z-scores its share of the signal's float4 -- counted from the 16-byte boundary at or below the signal's first
// feature, so that every full float4 is one aligned load and store; the first and last float4 of a signal may be shared with its
// neighbours and are done element by element.
// Signal s's float32 features lie at in + sig[s].ooff, its result goes to out + sig[s].ooff (offsets in elements): float is the
// in-place sweep (the host passes in == out: no __restrict__ here), a 2-byte OT the out-of-place one of a half plan
// (fsst_half.hpp) -- there `in` is 16-byte aligned, so with an 8-byte aligned `out` a float4 of `in` and its four OT share their
// position in the 4-element grid; an unaligned `out` goes element by element throughout.
template <class OT>
__global__ __launch_bounds__(256) void fsst_ragged_normalize_kernel(const float* in, OT* out, const RaggedSignal* sig, const int* unit0,
                                                                    const float4* stats, int nsig, int K)
{
    const int tid = threadIdx.x;
    const int C = 2 * K;
    const bool vec = zscore_store4_aligned(out);
    const int nunits = unit0[nsig];
    for (int u = blockIdx.x; u < nunits; u += gridDim.x) {
        int lo = 0, hi = nsig;                                   // unit0[lo] <= u < unit0[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (unit0[mid] <= u) lo = mid; else hi = mid;
        }
        const int s = lo;
        const RaggedSignal rs = sig[s];
        const float4 st = stats[s];
        const float m_re = st.x, i_re = st.y, m_im = st.z, i_im = st.w;
        const int a = static_cast<int>((reinterpret_cast<uintptr_t>(in + rs.ooff) >> 2) & 3);   // floats below the signal's first in its float4
        const float* src = in + (rs.ooff - a);
        OT* dst = out + (rs.ooff - a);
        const int total = rs.n * C;                              // (< 2^31: checked on the host)
        const int q = static_cast<int>((static_cast<long long>(a) + total + 3) >> 2);
        const int slices = unit0[s + 1] - unit0[s], sl = u - unit0[s];
        const int i0 = static_cast<int>(static_cast<long long>(q) * sl / slices);
        const int i1 = static_cast<int>(static_cast<long long>(q) * (sl + 1) / slices);
        long long e = 4ll * (i0 + tid) - a;                      // element of the float4's first lane (-a .. )
        int c = static_cast<int>(e % C);                         // its column (tracked incrementally below)
        if (c < 0) c += C;
        const int dc = 1024 % C;
        auto zs = [&](float v, int col) -> float { return (col < K) ? (v - m_re) * i_re : (v - m_im) * i_im; };
        auto wrap = [&](int col) -> int { if (col >= C) col -= C; if (col >= C) col -= C; return col; };   // (C >= 2: c + 3 < 3 C)
        for (int i = i0 + tid; i < i1; i += 256) {
            if (vec && e >= 0 && e + 4 <= total) {
                const float4 v = reinterpret_cast<const float4*>(src)[i];
                zscore_store4<OT>(dst + 4ll * i, zs(v.x, c), zs(v.y, wrap(c + 1)), zs(v.z, wrap(c + 2)), zs(v.w, wrap(c + 3)));
            } else {
                for (int k = 0; k < 4; ++k)
                    if (e + k >= 0 && e + k < total) dst[4ll * i + k] = static_cast<OT>(zs(src[4ll * i + k], wrap(c + k)));
            }
            e += 1024;
            c = wrap(c + dc);
        }
    }
}

}  // namespace hssfsst
