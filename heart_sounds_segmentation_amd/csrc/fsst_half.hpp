// fsst_half.hpp -- the z-score sweeps of half-precision STACK plans (HSSFSST_DTYPE_F16 / BF16, hssfsst_plan_create_ex).
// Every z-score path but the team kernel sweeps the un-normalised float32 features a second time, which a 2-byte output cannot
// hold: in a half plan those paths write them to a float32 scratch of the plan, and the sweeps here read it and write the result
// OUT OF PLACE as 2-byte elements (4 B read, 2 B written per element).  The arithmetic is that of fsst_normalize_kernel /
// fsst_ragged_normalize_kernel -- (v - mean) * (1 / std) in float32, the statistics from signal_stats() -- and the float32 value
// is then rounded to nearest even by the compiler's conversion (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32: NaN stays NaN), i.e. the
// result is the float32 path's, cast as Tensor.to(dtype) casts it.
#pragma once

#include "fsst_kernels.hpp"
#include "fsst_mfma128.hpp"

namespace hssfsst {

// four float32 values -> four OT at dst (8 bytes; dst 8-byte aligned)
template <class OT>
__device__ __forceinline__ void half_store4(OT* dst, float a, float b, float c, float d)
{
    using o2 = OT __attribute__((ext_vector_type(2)));
    using w2 = unsigned __attribute__((ext_vector_type(2)));
    const w2 w = {__builtin_bit_cast(unsigned, __builtin_convertvector(f2{a, b}, o2)), __builtin_bit_cast(unsigned, __builtin_convertvector(f2{c, d}, o2))};
    *reinterpret_cast<w2*>(dst) = w;
}

// fsst_normalize_kernel, out of place: in = float32 [nsignals][n][2K] (16-byte aligned), out = OT [nsignals][n][2K].  Same grid,
// slices and statistics (stats[], or the block's own reduction of `partials`) as that kernel.  The float4 sweep needs
// total % 4 == 0 and an 8-byte aligned `out`; otherwise element by element.
template <class OT>
__global__ __launch_bounds__(256) void fsst_normalize_to_kernel(const float* in, OT* out, const float4* stats, const float* partials,
                                                                int nblk, int fpp, int n, int K, int nsignals, int slices,
                                                                const unsigned* gate = nullptr, unsigned gate_val = 0u)
{
    static_assert(sizeof(OT) == 2, "2-byte output elements");
    if (gate != nullptr && *gate != gate_val) return;    // (the gated fallback behind a team launch: see fsst_stats_kernel)
    __shared__ float4 st_sh;
    const int tid = threadIdx.x;
    const int C = 2 * K;
    const int total = n * C;                             // per-signal element count (< 2^31, checked on the host)
    const bool vec = (total & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0;
    for (int unit = blockIdx.x; unit < nsignals * slices; unit += gridDim.x) {
        const int sig = unit / slices, sl = unit - sig * slices;
        float4 st;
        if (partials != nullptr) {
            if (tid < 64) {
                const float4 r = signal_stats(partials + static_cast<long long>(sig) * nblk * kPartFloats, nblk, fpp, n, K, tid);
                if (tid == 0) st_sh = r;
            }
            __syncthreads();
            st = st_sh;
            __syncthreads();
        } else {
            st = stats[sig];
        }
        const float m_re = st.x, i_re = st.y, m_im = st.z, i_im = st.w;
        const float* src = in + static_cast<long long>(sig) * total;
        OT* dst = out + static_cast<long long>(sig) * total;
        if (vec) {
            const float4* s4 = reinterpret_cast<const float4*>(src);
            const int tot4 = total >> 2;
            const int i0 = static_cast<int>(static_cast<long long>(tot4) * sl / slices);
            const int i1 = static_cast<int>(static_cast<long long>(tot4) * (sl + 1) / slices);
            int c = static_cast<int>((static_cast<unsigned>(i0 + tid) * 4u) % static_cast<unsigned>(C));
            const int dc = static_cast<int>(1024u % static_cast<unsigned>(C));
            const bool rowwrap = (C & 3) != 0;
#pragma unroll 4
            for (int i = i0 + tid; i < i1; i += 256) {
                const float4 v = s4[i];
                int c1 = c + 1, c2 = c + 2, c3 = c + 3;
                if (rowwrap) {
                    if (c1 >= C) c1 -= C;
                    if (c2 >= C) c2 -= C;
                    if (c3 >= C) c3 -= C;
                }
                half_store4<OT>(dst + 4ll * i,
                                (c < K) ? (v.x - m_re) * i_re : (v.x - m_im) * i_im,
                                (c1 < K) ? (v.y - m_re) * i_re : (v.y - m_im) * i_im,
                                (c2 < K) ? (v.z - m_re) * i_re : (v.z - m_im) * i_im,
                                (c3 < K) ? (v.w - m_re) * i_re : (v.w - m_im) * i_im);
                c += dc;
                if (c >= C) c -= C;
            }
        } else {
            const int i0 = static_cast<int>(static_cast<long long>(total) * sl / slices);
            const int i1 = static_cast<int>(static_cast<long long>(total) * (sl + 1) / slices);
            for (int i = i0 + tid; i < i1; i += 256) {
                const int c = i % C;
                const float v = src[i];
                dst[i] = static_cast<OT>((c < K) ? (v - m_re) * i_re : (v - m_im) * i_im);
            }
        }
    }
}

// fsst_ragged_normalize_kernel, out of place: signal s's float32 features at in + sig[s].ooff, its result at out + sig[s].ooff
// (offsets in elements).  `in` is 16-byte aligned; with an 8-byte aligned `out` a float4 of `in` and its four OT share their
// position in the 4-element grid, and every full one is one load and one 8-byte store; the first and last of a signal, and an
// unaligned `out`, go element by element.
template <class OT>
__global__ __launch_bounds__(256) void fsst_ragged_normalize_to_kernel(const float* in, OT* out, const RaggedSignal* sig, const int* unit0,
                                                                       const float4* stats, int nsig, int K)
{
    static_assert(sizeof(OT) == 2, "2-byte output elements");
    const int tid = threadIdx.x;
    const int C = 2 * K;
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 7) == 0;
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
        const int a = static_cast<int>(rs.ooff & 3);             // elements below the signal's first in its 4-element group
        const float* src = in + (rs.ooff - a);
        OT* dst = out + (rs.ooff - a);
        const int total = rs.n * C;                              // (< 2^31: checked on the host)
        const int q = static_cast<int>((static_cast<long long>(a) + total + 3) >> 2);
        const int slices = unit0[s + 1] - unit0[s], sl = u - unit0[s];
        const int i0 = static_cast<int>(static_cast<long long>(q) * sl / slices);
        const int i1 = static_cast<int>(static_cast<long long>(q) * (sl + 1) / slices);
        long long e = 4ll * (i0 + tid) - a;                      // element of the group's first lane (-a .. )
        int c = static_cast<int>(e % C);
        if (c < 0) c += C;
        const int dc = 1024 % C;
        auto zs = [&](float v, int col) -> float { return (col < K) ? (v - m_re) * i_re : (v - m_im) * i_im; };
        auto wrap = [&](int col) -> int { if (col >= C) col -= C; if (col >= C) col -= C; return col; };   // (C >= 2: c + 3 < 3 C)
        for (int i = i0 + tid; i < i1; i += 256) {
            if (vec && e >= 0 && e + 4 <= total) {
                const float4 v = reinterpret_cast<const float4*>(src)[i];
                half_store4<OT>(dst + 4ll * i, zs(v.x, c), zs(v.y, wrap(c + 1)), zs(v.z, wrap(c + 2)), zs(v.w, wrap(c + 3)));
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
