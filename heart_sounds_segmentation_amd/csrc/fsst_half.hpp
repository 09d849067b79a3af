// fsst_half.hpp -- how the z-score sweeps (fsst_normalize_kernel<OT>, fsst_ragged_normalize_kernel<OT>) store an output element
// type OT: float, or the 2-byte elements of a half-precision STACK plan (HSSFSST_DTYPE_F16 / BF16, hssfsst_plan_create_ex).
// Every z-score path but the team kernel sweeps the un-normalised float32 features a second time, which a 2-byte output cannot
// hold: in a half plan those paths write them to a float32 scratch of the plan, and the sweeps read it and write the result
// OUT OF PLACE as 2-byte elements (4 B read, 2 B written per element).  The arithmetic does not depend on OT -- (v - mean) *
// (1 / std) in float32, the statistics from signal_stats() -- and the float32 value is then rounded to nearest even by the
// compiler's conversion (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32: NaN stays NaN), i.e. the result is the float32 path's, cast as
// Tensor.to(dtype) casts it.
#pragma once

#include <hip/hip_runtime.h>

namespace hssfsst {

// four float32 values -> four OT at dst (8 bytes; dst 8-byte aligned)
template <class OT>
__device__ __forceinline__ void half_store4(OT* dst, float a, float b, float c, float d)
{
    using i2 = float __attribute__((ext_vector_type(2)));
    using o2 = OT __attribute__((ext_vector_type(2)));
    using w2 = unsigned __attribute__((ext_vector_type(2)));
    const w2 w = {__builtin_bit_cast(unsigned, __builtin_convertvector(i2{a, b}, o2)), __builtin_bit_cast(unsigned, __builtin_convertvector(i2{c, d}, o2))};
    *reinterpret_cast<w2*>(dst) = w;
}

// the sweeps' four-element store: one float4, or half_store4
template <class OT>
__device__ __forceinline__ void zscore_store4(OT* dst, float a, float b, float c, float d)
{
    static_assert(sizeof(OT) == 4 || sizeof(OT) == 2, "float, _Float16 or __bf16");
    if constexpr (sizeof(OT) == 4) *reinterpret_cast<float4*>(dst) = make_float4(a, b, c, d);
    else half_store4<OT>(dst, a, b, c, d);
}

// ... and what it asks of `out` beyond what the float32 side of a sweep has checked: 8-byte alignment of a 2-byte output
template <class OT>
__device__ __forceinline__ bool zscore_store4_aligned(const OT* out)
{
    return sizeof(OT) == 4 || (reinterpret_cast<uintptr_t>(out) & 7) == 0;
}

}  // namespace hssfsst
