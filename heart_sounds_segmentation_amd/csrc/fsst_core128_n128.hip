// fsst_core128_n128.hip -- the MFMA core's unit for nwin 128 (16 taps x radix 8): its rows of kCore128Plain (fsst_launch_shape.hpp), dense and ragged, and the
// fused and streaming instantiations of that length.  The launchers are fsst_core128_launch.hpp's; the other lengths: the sibling units.
#include "fsst_core128_launch.hpp"

namespace hssfsst {
namespace host __attribute__((visibility("hidden"))) {

namespace {
constexpr bool mine(const hssfsst::Core128PlainRow& r) { return r.nt == 16 && r.rq == 8; }
}  // namespace

int launch_core128_plain_n128(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, bool ragged)
{
    return launch_core128_rows<mine>(pl, cx, cp, nchunks, ragged);
}

// the one-CU-per-signal z-score kernels of the bands the canonical-band kernels do not take: wide-store epilogue (fast) or general
int launch_fused_n128(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t batch, int ngroups, bool fast, bool stripes03)
{
    if (!fast) return launch_fused<16, 8, false, 16, -1>(pl, cx, cp, batch, ngroups);
    return stripes03 ? launch_fused<16, 8, true, 16, 3>(pl, cx, cp, batch, ngroups) : launch_fused<16, 8, true, 16, -1>(pl, cx, cp, batch, ngroups);
}

}  // namespace host
}  // namespace hssfsst
