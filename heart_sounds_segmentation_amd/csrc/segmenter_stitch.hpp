// segmenter_stitch.hpp -- the kernel of hssfsst_stitch_windows (hssfsst.h): a gather.  One lane per output step; it finds the step's
// recording among the launch's offsets, walks the step's covering windows in ascending start order (stitch_layout.hpp: cover_of)
// and runs stitch_step() on their rows, the function the sequential reference runs.  Every output row is written once, by one
// lane, as one 16-byte store; every window row is read as one 16-byte load.  Consecutive lanes take consecutive steps, so within a
// recording each covering window's reads are consecutive rows.  No atomics, no LDS, no scratch, and no workgroup waits for
// another.  The rows of a step are loaded again for each pass over them (the maximum, the sum, the dissent count) instead of being
// kept in an array indexed by a loop counter: the second and third load of a row hit the cache the first one filled.
#pragma once

#include <hip/hip_runtime.h>

#include "stitch_layout.hpp"

namespace hssfsst {

namespace stl = stitchlayout;

struct StitchArgs {
    long long first[stl::kStitchBatch];                  // win_first of the launch's recordings
    int off[stl::kStitchBatch + 1];                      // their step offsets: a list holds at most 2^31 - 1 steps
    int nrec;
    int n, stride;
};

template <int MODE, bool WEIGHTS>
__global__ __launch_bounds__(stl::kThreads) void seg_stitch_kernel(const float* __restrict__ win, const float* __restrict__ weights,
                                                                   float* __restrict__ out, unsigned char* __restrict__ dissent,
                                                                   StitchArgs args)
{
    const long long at = args.off[0] + static_cast<long long>(blockIdx.x) * stl::kThreads + static_cast<long long>(threadIdx.x);
    if (at >= args.off[args.nrec]) return;
    int r = 0, hi = args.nrec - 1;                       // the largest r with off[r] <= at
    while (r < hi) {
        const int mid = (r + hi + 1) >> 1;
        if (args.off[mid] <= at) r = mid; else hi = mid - 1;
    }
    const int n = args.n, stride = args.stride;
    const long long T = args.off[r + 1] - args.off[r], t = at - args.off[r];
    const stl::Cover c = stl::cover_of(t, T, n, stride);
    const float4* rows = reinterpret_cast<const float4*>(win) + args.first[r];
    auto position = [&](int k) { return t - stl::window_start(stl::cover_window(c, k), T, n, stride); };
    auto row = [&](int k) {
        const float4 e = rows[stl::cover_window(c, k) * n + position(k)];
        return stl::Row{{e.x, e.y, e.z, e.w}};
    };
    auto weight = [&](int k) { return WEIGHTS ? weights[position(k)] : 1.0f; };
    const stl::Step s = stl::stitch_step(stl::cover_size(c), MODE, row, weight, dissent != nullptr);
    reinterpret_cast<float4*>(out)[at] = make_float4(s.out.v[0], s.out.v[1], s.out.v[2], s.out.v[3]);
    if (dissent) dissent[at] = static_cast<unsigned char>(s.dissent);
}

}  // namespace hssfsst
