// Stand-alone check of the trainable BiLSTM layer's index arithmetic (csrc/segmenter_layout.hpp: host only, no HIP), built with
// -fsanitize=address,undefined by tests/test_segmenter_train.py.  The stash and the backward weight stream are in bounds and
// one-to-one; the forward tables' index functions, which seg_upload_layer (csrc/segmenter.hip) and seg_pack_kernel both walk, equal
// the nested loops that seg_upload_layer was before it called them, kept here as the independent statement of the layout.
// Any failed property or sanitizer report ends the run non-zero.
#include "segmenter_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

namespace sl = hssfsst::seglayout;

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (failures < 20) { std::printf("FAIL H=%d: ", H); std::printf(__VA_ARGS__); std::printf("\n"); } \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

// every (dir, tile, t, wave, tl, q, lane, r) lands in [0, stash_floats) and no two land on the same float
static void check_stash(int H, long long batch, long long steps)
{
    const long long tiles = (batch + 15) / 16, total = sl::stash_floats(batch, steps);
    CHECK(total == 2 * tiles * steps * 8 * 2 * 5 * 256, "stash_floats(%lld, %lld) = %lld", batch, steps, total);
    std::vector<unsigned char> hit(static_cast<size_t>(total), 0);   // exactly sized: an index past the end is a report
    long long n = 0;
    for (int dir = 0; dir < 2; ++dir)
        for (long long tile = 0; tile < tiles; ++tile)
            for (long long t = 0; t < steps; ++t)
                for (int w = 0; w < 8; ++w)
                    for (int tl = 0; tl < 2; ++tl)
                        for (int q = 0; q < sl::kStashQ; ++q)
                            for (int lane = 0; lane < 64; ++lane)
                                for (int r = 0; r < 4; ++r, ++n) {
                                    const long long i = sl::stash_index(tiles, steps, dir, tile, t, w, tl, q, lane, r);
                                    if (i < 0 || i >= total) { CHECK(false, "stash index %lld outside [0, %lld)", i, total); continue; }
                                    CHECK(hit[static_cast<size_t>(i)] == 0, "stash index %lld taken twice", i);
                                    hit[static_cast<size_t>(i)] = 1;
                                    // a lane's four rows are one float4
                                    if (r > 0) CHECK(i == sl::stash_index(tiles, steps, dir, tile, t, w, tl, q, lane, 0) + r, "rows apart");
                                }
    CHECK(n == total, "%lld coordinates for %lld floats", n, total);
}

// the backward stream: B operand of dh[b, kout] = sum_kappa dG[b, kappa] W_hh[row(kappa), kout]
static void check_bwd_stream(int H)
{
    const long long per = sl::kBwdStreamHalves / 2;
    std::vector<unsigned char> hit(static_cast<size_t>(per), 0);
    std::vector<int> used(static_cast<size_t>(4) * H * H, 0);
    for (int w = 0; w < 8; ++w)
        for (int kb = 0; kb < 32; ++kb)
            for (int ot = 0; ot < 2; ++ot)
                for (int lane = 0; lane < 64; ++lane)
                    for (int lo = 0; lo < 2; ++lo)
                        for (int j = 0; j < 8; ++j) {
                            const long long i = sl::bwd_stream_index(w, kb, ot, lane, lo, j);
                            if (i < 0 || i >= per) { CHECK(false, "stream index %lld outside [0, %lld)", i, per); continue; }
                            CHECK(hit[static_cast<size_t>(i)] == 0, "stream index %lld taken twice", i);
                            hit[static_cast<size_t>(i)] = 1;
                            CHECK(i % 8 == j && (i / 8) % 2 == lo, "a lane's fragment is not {hi[8], lo[8]}");
                            // what the matrix instruction multiplies there: B[k = 8 (lane >> 4) + j][column lane & 15]
                            const int kappa = kb * 32 + 8 * (lane >> 4) + j, ut = kappa / 64, g = (kappa / 16) % 4, c = kappa % 16;
                            const int u = ut * 16 + c, kout = (2 * w + ot) * 16 + (lane & 15);
                            const long long want = u < H && kout < H ? (static_cast<long long>(g) * H + u) * H + kout : -1;
                            int got_lo = -1;
                            const long long got = sl::bwd_stream_source(i, H, &got_lo);
                            CHECK(got == want && got_lo == lo, "stream element %lld holds W_hh[%lld] (lo %d), expected [%lld] (lo %d)", i, got,
                                  got_lo, want, lo);
                            if (got >= 0 && got < static_cast<long long>(used.size())) ++used[static_cast<size_t>(got)];
                        }
    for (size_t s = 0; s < used.size(); ++s) CHECK(used[s] == 2, "W_hh[%zu] is streamed %d times, not as one hi and one lo", s, used[s]);
}

// the layout as nested loops over (unit tile, gate, unit) and (wave, K block, tile x gate, lane, j), writing source indices instead
// of values (-1: the zero the tables start with)
static void check_forward_tables(int H, int F)
{
    constexpr int Hp = sl::kHp, N = 4 * Hp, kWaves = 8, kKb = Hp / 32;
    const int Fp = (F + 31) / 32 * 32;
    std::vector<long long> wt(static_cast<size_t>(Fp) * N, -1), bias(static_cast<size_t>(N), -1);
    std::vector<long long> stream(static_cast<size_t>(kWaves) * kKb * 8 * 64 * 16, -1);
    for (int ut = 0; ut < Hp / 16; ++ut)
        for (int g = 0; g < 4; ++g)
            for (int c = 0; c < 16; ++c) {
                const int u = ut * 16 + c, n = (ut * 4 + g) * 16 + c;
                if (u >= H) continue;
                const size_t row = static_cast<size_t>(g) * H + u;
                bias[n] = static_cast<long long>(row);
                for (int k = 0; k < F; ++k) wt[static_cast<size_t>(k) * N + n] = static_cast<long long>(row * F + k);
            }
    for (int w = 0; w < kWaves; ++w)
        for (int kb = 0; kb < kKb; ++kb)
            for (int q = 0; q < 8; ++q)
                for (int lane = 0; lane < 64; ++lane) {
                    const int u = (w * 2 + (q >> 2)) * 16 + (lane & 15), g = q & 3;
                    if (u >= H) continue;
                    long long* dst = stream.data() + (((static_cast<size_t>(w) * kKb + kb) * 8 + q) * 64 + lane) * 16;
                    for (int j = 0; j < 8; ++j) {
                        const int k = kb * 32 + 8 * (lane >> 4) + j;
                        if (k >= H) continue;
                        dst[j] = dst[8 + j] = (static_cast<long long>(g) * H + u) * H + k;
                    }
                }
    CHECK(static_cast<long long>(stream.size()) == sl::kWtStreamHalves / 2, "forward stream of %zu halves per direction", stream.size());
    for (size_t i = 0; i < wt.size(); ++i) {
        const long long got = sl::wt_source(static_cast<long long>(i), F, H);
        CHECK(got == wt[i], "F=%d: wt[%zu] from weight_ih[%lld], the loops say [%lld]", F, i, got, wt[i]);
        CHECK(got < static_cast<long long>(4) * H * F, "F=%d: wt[%zu] reads past weight_ih", F, i);
    }
    for (int n = 0; n < N; ++n) CHECK(sl::gate_col_row(n, H) == bias[n], "bias[%d] from row %lld, the loops say %lld", n, sl::gate_col_row(n, H), bias[n]);
    for (size_t i = 0; i < stream.size(); ++i) {
        int lo = -1;
        const long long got = sl::fwd_stream_source(static_cast<long long>(i), H, &lo);
        CHECK(got == stream[i] && lo == static_cast<int>((i >> 3) & 1), "forward stream[%zu] from W_hh[%lld] (lo %d), the loops say [%lld]", i, got, lo,
              stream[i]);
        CHECK(got < static_cast<long long>(4) * H * H, "forward stream[%zu] reads past weight_hh", i);
    }
}

int main()
{
    for (int H : {1, 5, 16, 240, 256}) {
        check_stash(H, 1, 1);
        check_stash(H, 16, 3);
        check_stash(H, 17, 2);
        check_stash(H, 33, 5);
        check_bwd_stream(H);
        for (int F : {1, 7, 44, 2 * H}) check_forward_tables(H, F);
        std::printf("H=%3d ok\n", H);
    }
    // the figure of the documentation: batch 50 x 2000 steps
    { const int H = 240; CHECK(sl::stash_floats(50, 2000) * 4 == 1310720000LL, "stash of the C4 shape: %lld bytes", sl::stash_floats(50, 2000) * 4); }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("segmenter train layout ok\n");
    return 0;
}
