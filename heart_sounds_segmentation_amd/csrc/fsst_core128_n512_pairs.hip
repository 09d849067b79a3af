// fsst_core128_n512_pairs.hip -- the MFMA core's unit for nwin 512 (32 taps x radix 16) on wave pairs: its rows of kCore128Plain (fsst_launch_shape.hpp), dense and ragged, and the
// fused and streaming instantiations of that length.  The launchers are fsst_core128_launch.hpp's; the other lengths: the sibling units.
#include "fsst_core128_launch.hpp"

namespace hssfsst {
namespace host __attribute__((visibility("hidden"))) {

namespace {
constexpr bool mine(const hssfsst::Core128PlainRow& r) { return r.nt == 32 && r.pair; }
}  // namespace

int launch_core128_plain_n512_pairs(hssfsst_plan* pl, ExecCtx& cx, const hssfsst::Core128Params& cp, int64_t nchunks, bool ragged)
{
    return launch_core128_rows<mine>(pl, cx, cp, nchunks, ragged);
}

int launch_stream_n512_pairs(hssfsst_plan* pl, float* tape_at, long long tape_len, const float* x_new_dev, long long x_stride, int channels,
                             int chunk, float* out, double* state, float* mirror, hipStream_t st)
{
    return launch_stream<32, 16, 4, true>(pl, tape_at, tape_len, x_new_dev, x_stride, channels, chunk, out, state, mirror, st);
}

}  // namespace host
}  // namespace hssfsst
