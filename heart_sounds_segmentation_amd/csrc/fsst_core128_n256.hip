// fsst_core128_n256.hip -- the MFMA core's unit for nwin 256 (16 taps x radix 16): its rows of kCore128Plain (fsst_launch_shape.hpp), dense and ragged, and the
// fused and streaming instantiations of that length.  The launchers are fsst_core128_launch.hpp's; the other lengths: the sibling units.
#include "fsst_core128_launch.hpp"

namespace hssfsst {
namespace host __attribute__((visibility("hidden"))) {

namespace {
constexpr bool mine(const hssfsst::Core128PlainRow& r) { return r.nt == 16 && r.rq == 16; }
}  // namespace

int launch_core128_plain_n256(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, bool ragged)
{
    return launch_core128_rows<mine>(pl, cx, cp, nchunks, ragged);
}

// the general epilogue at one CU per signal: as many waves as on the two-launch path (8)
int launch_fused_n256(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t batch, int ngroups, bool stripes03)
{
    return stripes03 ? launch_fused<16, 16, false, 8, 3>(pl, cx, cp, batch, ngroups) : launch_fused<16, 16, false, 8, -1>(pl, cx, cp, batch, ngroups);
}

// (pair: on wave pairs -- the step's latency is one group's; regions of a block = 2)
int launch_stream_n256(hssfsst_plan* pl, float* tape_at, long long tape_len, const float* x_new_dev, long long x_stride, int channels,
                       int chunk, float* out, double* state, float* mirror, hipStream_t st, bool pair)
{
    return pair ? launch_stream<16, 16, 4, true>(pl, tape_at, tape_len, x_new_dev, x_stride, channels, chunk, out, state, mirror, st)
                : launch_stream<16, 16, 4, false>(pl, tape_at, tape_len, x_new_dev, x_stride, channels, chunk, out, state, mirror, st);
}

}  // namespace host
}  // namespace hssfsst
