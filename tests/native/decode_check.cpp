// Stand-alone check of the Viterbi decoder's arithmetic and geometry (csrc/decode_layout.hpp: host only, no HIP), built with
// -fsanitize=address,undefined -fno-sanitize-recover=all by tests/test_segmenter_decode.py.  decode_chunked() below is the kernel of
// csrc/segmenter_decode.hpp with its lanes simulated: the same functions, the same segments, the same staging indices, the same
// scan orders, the backpointer bytes kept in the path itself.  It must equal decode_reference(), the sequential loop, in every
// state and in the score.  Any failed property or sanitizer report ends the run non-zero.
#include "decode_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

namespace dl = hssfsst::declayout;
using dl::i64;

static int failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) { std::printf("FAIL %s: ", name); std::printf(__VA_ARGS__); std::printf("\n"); ++failures; } \
    } while (0)

static i64 decode_chunked(const float* e, i64 T, const float* Af, const float* pif, uint8_t* path)
{
    const dl::Mat A = dl::quantise_transitions(Af);
    const dl::Vec pi = dl::quantise4(pif), e0 = dl::quantise4(e);
    constexpr int W = dl::kLanes / 64;
    std::vector<i64> stage(dl::kStageWords);             // exactly sized: an index past the end is a report
    std::vector<dl::Mat> P(dl::kLanes), X(dl::kLanes);
    dl::Vec d;
    for (int j = 0; j < 4; ++j) d.v[j] = dl::add(pi.v[j], e0.v[j]);
    const i64 nseg = dl::segments(T);
    auto staged = [&](int idx) { return dl::Vec{{stage[idx], stage[idx + 1], stage[idx + 2], stage[idx + 3]}}; };

    for (i64 seg = 0; seg < nseg; ++seg) {
        const i64 first = dl::segment_first(seg);
        const int nsteps = dl::segment_steps(T, seg);
        for (int tid = 0; tid < dl::kLanes; ++tid)
            for (int k = 0; k < dl::kLc; ++k) {
                const int s = k * dl::kLanes + tid;
                if (s >= nsteps) continue;
                const dl::Vec q = dl::quantise4(e + 4 * (first + s));
                for (int j = 0; j < 4; ++j) stage[dl::stage_index(s) + j] = q.v[j];
            }
        for (int tid = 0; tid < dl::kLanes; ++tid) {
            const int n = dl::lane_steps(nsteps, tid);
            P[tid] = dl::identity();
            for (int k = 0; k < n; ++k) dl::step_matrix(P[tid], A, staged(tid * dl::kLaneStride + 4 * k));
        }
        for (int off = 1; off < 64; off <<= 1) {         // the waves' inclusive scans, all lanes at once
            const std::vector<dl::Mat> old = P;
            for (int tid = 0; tid < dl::kLanes; ++tid)
                if ((tid & 63) >= off) P[tid] = dl::matmul(old[tid - off], old[tid]);
        }
        for (int tid = 0; tid < dl::kLanes; ++tid) X[tid] = (tid & 63) == 0 ? dl::identity() : P[tid - 1];
        dl::Vec dnext = d;
        std::vector<dl::Vec> dwave(W);
        for (int w = 0; w < W; ++w) {
            dwave[w] = dnext;
            dnext = dl::vecmat(dnext, P[64 * w + 63]);
        }
        for (int tid = 0; tid < dl::kLanes; ++tid) {
            const int n = dl::lane_steps(nsteps, tid);
            dl::Vec din = dl::vecmat(dwave[tid >> 6], X[tid]);
            const i64 t0 = first + static_cast<i64>(tid) * dl::kLc;
            for (int k = 0; k < n; ++k) path[t0 + k] = static_cast<uint8_t>(dl::step(din, A, staged(tid * dl::kLaneStride + 4 * k)));
        }
        d = dnext;
    }

    i64 score;
    unsigned s_end = dl::end_state(d, &score);
    std::vector<unsigned> R(dl::kLanes);
    std::vector<std::vector<unsigned>> b(dl::kLanes, std::vector<unsigned>(dl::kLc));
    for (i64 seg = nseg - 1; seg >= 0; --seg) {
        const i64 first = dl::segment_first(seg);
        const int nsteps = dl::segment_steps(T, seg);
        for (int tid = 0; tid < dl::kLanes; ++tid) {
            const int n = dl::lane_steps(nsteps, tid);
            const i64 t0 = first + static_cast<i64>(tid) * dl::kLc;
            unsigned g = dl::kIdentityMap;
            for (int k = 0; k < dl::kLc; ++k) {
                b[tid][k] = k < n ? path[t0 + k] : dl::kIdentityMap;
                g = dl::map_compose(g, b[tid][k]);
            }
            R[tid] = g;
        }
        for (int off = 1; off < 64; off <<= 1) {
            const std::vector<unsigned> old = R;
            for (int tid = 0; tid < dl::kLanes; ++tid)
                if ((tid & 63) + off < 64) R[tid] = dl::map_compose(old[tid], old[tid + off]);
        }
        unsigned s = s_end;
        std::vector<unsigned> swave(W);
        for (int w = W - 1; w >= 0; --w) {
            swave[w] = s;
            s = dl::map_apply(R[64 * w], s);
        }
        s_end = s;
        for (int tid = 0; tid < dl::kLanes; ++tid) {
            const int n = dl::lane_steps(nsteps, tid);
            const i64 t0 = first + static_cast<i64>(tid) * dl::kLc;
            const unsigned Xm = (tid & 63) == 63 ? dl::kIdentityMap : R[tid + 1];
            unsigned st = dl::map_apply(Xm, swave[tid >> 6]);
            for (int k = n - 1; k >= 0; --k) {
                path[t0 + k] = static_cast<uint8_t>(st);
                st = dl::map_apply(b[tid][k], st);
            }
        }
    }
    path[0] = static_cast<uint8_t>(s_end);
    return score;
}

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<unsigned>(rng_state >> 33);
}
static float rnd_logp() { return -static_cast<float>(rnd() % 100000) / 8192.0f - 1e-3f; }

static const float NINF = -std::numeric_limits<float>::infinity();
static const float kCyclic[16] = {0, 0, NINF, NINF, NINF, 0, 0, NINF, NINF, NINF, 0, 0, 0, NINF, NINF, 0};
static const float kUniform[4] = {0, 0, 0, 0};
static const float kState0[4] = {0, NINF, NINF, NINF};

static void run_case(const char* name, const std::vector<float>& e, const float* A, const float* pi)
{
    const i64 T = static_cast<i64>(e.size() / 4);
    std::vector<uint8_t> want(static_cast<size_t>(T)), got(static_cast<size_t>(T));   // exactly sized
    const i64 sw = dl::decode_reference(e.data(), T, A, pi, want.data());
    const i64 sg = decode_chunked(e.data(), T, A, pi, got.data());
    CHECK(sw == sg, "T %lld: score %lld, reference %lld", T, sg, sw);
    i64 bad = -1;
    for (i64 t = 0; t < T && bad < 0; ++t)
        if (want[t] != got[t]) bad = t;
    CHECK(bad < 0, "T %lld: state differs at step %lld (%d, reference %d)", T, bad, got[bad < 0 ? 0 : bad], want[bad < 0 ? 0 : bad]);
    // the segment list covers steps 1 .. T - 1 once and in order
    i64 next = 1;
    for (const dl::Segment& s : dl::segment_list(T)) {
        CHECK(s.first == next && s.steps >= 1 && s.steps <= dl::kSegSteps, "segment at %lld with %d steps, expected at %lld", s.first, s.steps, next);
        next = s.first + s.steps;
    }
    CHECK(next == (T > 1 ? T : 1), "segments end at %lld of %lld", next, T);
}

int main()
{
    const char* name = "constants";
    // the 2^62 bound, from the constants: two terms per step, each at most 2^35 in magnitude, over the longest recording
    CHECK(dl::quantise(dl::kClamp) == dl::kMaxTerm && dl::quantise(-dl::kClamp) == -dl::kMaxTerm, "q(clamp) is not 2^35");
    CHECK(dl::kMaxSteps == (i64(1) << 26), "max steps");
    CHECK(2 * dl::kMaxSteps * dl::kMaxTerm == (i64(1) << 62), "the bound is not 2^62");
    CHECK(-(i64(1) << 62) > dl::kNeg, "NEG is not below every sum");
    // the quantiser
    CHECK(dl::quantise(1.5f / 1048576.0f) == 2 && dl::quantise(2.5f / 1048576.0f) == 2 && dl::quantise(-0.5f / 1048576.0f) == 0, "half to even");
    CHECK(dl::quantise(std::numeric_limits<float>::quiet_NaN()) == -dl::kMaxTerm, "q(NaN)");
    CHECK(dl::quantise(NINF) == dl::kNeg && dl::quantise(-NINF) == dl::kMaxTerm, "q(+-inf)");
    CHECK(dl::quantise(1e9f) == dl::kMaxTerm && dl::quantise(-1e9f) == -dl::kMaxTerm, "clamp");
    CHECK(dl::add(dl::kNeg, -5) == dl::kNeg && dl::add(7, dl::kNeg) == dl::kNeg && dl::max2(dl::kNeg, -dl::kMaxTerm) == -dl::kMaxTerm, "NEG");
    // maps
    for (unsigned a = 0; a < 256; ++a)
        for (unsigned b = 0; b < 256; b += 7)
            for (unsigned s = 0; s < 4; ++s)
                CHECK(dl::map_apply(dl::map_compose(a, b), s) == dl::map_apply(a, dl::map_apply(b, s)), "compose %u %u", a, b);
    CHECK(dl::map_compose(dl::kIdentityMap, 0x1Bu) == 0x1Bu && dl::map_compose(0x1Bu, dl::kIdentityMap) == 0x1Bu, "identity map");

    float dense[16];
    for (float& v : dense) v = rnd_logp();
    const int S = dl::kSegSteps;
    const i64 lens[] = {1, 2, 3, 63, 64, 65, S - 1, S, S + 1, S + 2, 2 * S + 1, 3 * S + 17};
    for (i64 T : lens) {
        std::vector<float> e(static_cast<size_t>(4 * T));
        for (int kind = 0; kind < 3; ++kind) {
            for (float& v : e) v = kind == 0 ? rnd_logp() : kind == 1 ? 0.0f : -static_cast<float>(rnd() % 4);
            name = kind == 0 ? "random emissions" : kind == 1 ? "all-equal emissions" : "emissions in {-3..0}";
            run_case(name, e, kCyclic, kUniform);
            run_case(name, e, dense, kUniform);
            run_case(name, e, kCyclic, kState0);
            run_case(name, e, dense, kState0);
        }
    }
    {   // special values: NaN, +-inf, beyond the clamp; a step that is all -inf
        name = "special values";
        const i64 T = 2 * S + 5;
        std::vector<float> e(static_cast<size_t>(4 * T));
        for (float& v : e) v = rnd_logp();
        for (int j = 0; j < 4; ++j) e[4 * 10 + j] = std::numeric_limits<float>::quiet_NaN();
        e[4 * 100 + 1] = NINF;
        e[4 * 200 + 2] = -NINF;
        e[4 * 300 + 3] = 1e6f;
        e[4 * 400 + 0] = -1e6f;
        e[4 * (S + 1) + 2] = NINF;
        run_case(name, e, kCyclic, kUniform);
        run_case(name, e, dense, kState0);
        for (int j = 0; j < 4; ++j) e[4 * (S + 9) + j] = NINF;
        name = "an all -inf step";
        run_case(name, e, kCyclic, kUniform);
        std::vector<uint8_t> p(static_cast<size_t>(T));
        CHECK(dl::decode_reference(e.data(), T, kCyclic, kUniform, p.data()) == dl::kNeg, "score is not NEG");
    }
    {   // worst-case magnitude: every term at the clamp, both signs; the overflow check of the sanitizer is the proof
        const i64 T = 40 * S + 3;
        std::vector<float> e(static_cast<size_t>(4 * T));
        float big[16], bigpi[4];
        for (int sign = -1; sign <= 1; sign += 2) {
            name = sign < 0 ? "every term at -clamp" : "every term at +clamp";
            for (float& v : e) v = sign * 1e9f;
            for (float& v : big) v = sign * 1e9f;
            for (float& v : bigpi) v = sign * 1e9f;
            run_case(name, e, big, bigpi);
            std::vector<uint8_t> p(static_cast<size_t>(T));
            CHECK(dl::decode_reference(e.data(), T, big, bigpi, p.data()) == sign * 2 * T * dl::kMaxTerm, "score is not 2 T 2^35");
        }
        // ... and at the longest recording the same sum is the bound itself
        name = "bound";
        i64 sum = 0;
        for (i64 t = 0; t < 64; ++t) sum += 2 * (dl::kMaxSteps / 64) * dl::kMaxTerm;   // (signed adds under the sanitizer)
        CHECK(sum == (i64(1) << 62), "sum over 2^26 steps");
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("decode check ok\n");
    return 0;
}
