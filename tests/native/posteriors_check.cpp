// posteriors_check.cpp -- csrc/posterior_layout.hpp in a program of its own, built with -fsanitize=address,undefined by
// tests/test_posteriors.py: the kernel's sweeps (csrc/segmenter_posteriors.hpp) with the lanes, the wave scans and the segment
// loop simulated on the host equal the sequential reference loop to 1e-13 relative, every stage and workspace index stays inside
// its bounds, no two recordings share a checkpoint slot, and zero matrices (Z = 0) renormalise without undefined behaviour.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "posterior_layout.hpp"

namespace pl = hssfsst::postlayout;
using pl::i64;

static int failures = 0;
#define CHECK(cond, ...)                                                                                                                   \
    do {                                                                                                                                   \
        if (!(cond)) {                                                                                                                     \
            if (++failures < 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                                                  \
    } while (0)

struct Stage {
    std::vector<double> w = std::vector<double>(pl::kStageWords, -1.0);
    double* at(int idx)
    {
        CHECK(idx >= 0 && idx + 4 <= pl::kStageWords, "stage index %d", idx);
        return &w.at(static_cast<size_t>(idx));
    }
};

struct Out { std::vector<double> gamma; double loglik, score; double xi[16]; double g0[4]; };

constexpr int kWaves = pl::kLanes / 64;

// one workgroup: recording `rec` of the list, its steps at `base` of the arenas
static Out simulate(const float* logp, i64 base, i64 T, const float* a_pi, const uint8_t* labels, std::vector<double>& work, std::vector<int>& owner,
                    i64 rec)
{
    const float* e = logp + 4 * base;
    const uint8_t* lab = labels ? labels + base : nullptr;
    const i64 slot0 = pl::checkpoint_slot(base, rec);
    const pl::Tables tb = pl::make_tables(a_pi);
    const i64 nseg = pl::segments(T);
    Out out{};
    out.gamma.assign(static_cast<size_t>(4 * T), -7.0);
    Stage stage;
    auto ckpt = [&](i64 seg) -> double* {
        const i64 slot = slot0 + seg;
        CHECK(slot >= 0 && 4 * slot + 4 <= static_cast<i64>(work.size()), "checkpoint slot %lld of %zu doubles", slot, work.size());
        CHECK(owner.at(static_cast<size_t>(slot)) == -1 || owner.at(static_cast<size_t>(slot)) == rec, "slot %lld shared", slot);
        owner.at(static_cast<size_t>(slot)) = static_cast<int>(rec);
        return &work.at(static_cast<size_t>(4 * slot));
    };
    auto stage_segment = [&](i64 first, int nsteps, std::vector<double>* acc) {
        for (int tid = 0; tid < pl::kLanes; ++tid)
            for (int k = 0; k < pl::kLc; ++k) {
                const int s = k * pl::kLanes + tid;
                if (s >= nsteps) continue;
                CHECK(first + s >= 1 && first + s < T, "step %lld of %lld", first + s, T);
                const float* v = e + 4 * (first + s);
                const double top = pl::step_weights(v[0], v[1], v[2], v[3], stage.at(pl::stage_index(s)));
                if (acc) {
                    (*acc)[2 * tid] += top;
                    if (lab) {
                        const int y = lab[first + s] & 3, yp = lab[first + s - 1] & 3;
                        (*acc)[2 * tid + 1] += static_cast<double>(v[y] != v[y] ? -INFINITY : v[y]) + static_cast<double>(a_pi[4 * yp + y]);
                    }
                }
            }
    };
    auto lane_matrix = [&](int tid, int n) {
        pl::SMat M = pl::identity();
        for (int k = 0; k < n; ++k) pl::step_matrix(M, tb, stage.at(tid * pl::kLaneStride + 4 * k));
        return M;
    };
    auto reduce = [&](const std::vector<double>& v, int stride, int which) {      // the shuffle tree per wave, then the waves in order
        double waves[kWaves];
        for (int w = 0; w < kWaves; ++w) {
            double x[64];
            for (int l = 0; l < 64; ++l) x[l] = v[static_cast<size_t>((64 * w + l) * stride + which)];
            for (int off = 32; off >= 1; off >>= 1)
                for (int l = 0; l < 64; ++l) x[l] += l + off < 64 ? x[l + off] : x[l];    // (a lane past the end reads itself)
            waves[w] = x[0];
        }
        return ((waves[0] + waves[1]) + waves[2]) + waves[3];
    };

    std::vector<double> acc(2 * pl::kLanes, 0.0);
    double b0[4];
    const double top0 = pl::step_weights(e[0], e[1], e[2], e[3], b0);
    pl::SVec alpha0{{tb.p0[0] * b0[0], tb.p0[1] * b0[1], tb.p0[2] * b0[2], tb.p0[3] * b0[3]}, 0};
    pl::renorm(alpha0);
    acc[0] = top0;
    if (lab) acc[1] = static_cast<double>(e[lab[0] & 3] != e[lab[0] & 3] ? -INFINITY : e[lab[0] & 3]) + static_cast<double>(a_pi[16 + (lab[0] & 3)]);

    pl::SVec alpha = alpha0;
    std::vector<pl::SMat> P(pl::kLanes), M(pl::kLanes);
    for (i64 seg = 0; seg < nseg; ++seg) {
        const i64 first = pl::segment_first(seg);
        const int nsteps = pl::segment_steps(T, seg);
        CHECK(nsteps >= 1 && nsteps <= pl::kSegSteps, "segment of %d steps", nsteps);
        stage_segment(first, nsteps, &acc);
        for (int tid = 0; tid < pl::kLanes; ++tid) P[tid] = lane_matrix(tid, pl::lane_steps(nsteps, tid));
        for (int off = 1; off < 64; off <<= 1) {
            const std::vector<pl::SMat> Q = P;
            for (int tid = 0; tid < pl::kLanes; ++tid)
                if ((tid & 63) >= off) P[tid] = pl::matmul(Q[tid - off], Q[tid]);
        }
        double* c = ckpt(seg);
        for (int j = 0; j < 4; ++j) c[j] = alpha.v[j];
        for (int w = 0; w < kWaves; ++w) alpha = pl::vecmat(alpha, P[64 * w + 63]);
    }
    out.loglik = pl::log_z(alpha, reduce(acc, 2, 0));
    out.score = reduce(acc, 2, 1);

    for (int i = 0; i < 16; ++i) out.xi[i] = 0.0;
    pl::SVec beta_end{{1.0, 1.0, 1.0, 1.0}, 0};
    for (i64 seg = nseg - 1; seg >= 0; --seg) {
        const i64 first = pl::segment_first(seg);
        const int nsteps = pl::segment_steps(T, seg);
        stage_segment(first, nsteps, nullptr);
        for (int tid = 0; tid < pl::kLanes; ++tid) M[tid] = lane_matrix(tid, pl::lane_steps(nsteps, tid));
        P = M;
        for (int off = 1; off < 64; off <<= 1) {
            const std::vector<pl::SMat> Q = P;
            for (int tid = 0; tid < pl::kLanes; ++tid)
                if ((tid & 63) >= off) P[tid] = pl::matmul(Q[tid - off], Q[tid]);
        }
        std::vector<pl::SMat> S = M;
        for (int off = 1; off < 64; off <<= 1) {
            const std::vector<pl::SMat> Q = S;
            for (int tid = 0; tid < pl::kLanes; ++tid)
                if ((tid & 63) + off < 64) S[tid] = pl::matmul(Q[tid], Q[tid + off]);
        }
        pl::SMat W[kWaves];
        for (int w = 0; w < kWaves; ++w) {
            W[w] = P[64 * w + 63];
            W[w].e = 0;
        }
        const double* c = ckpt(seg);
        const pl::SVec a_seg{{c[0], c[1], c[2], c[3]}, 0};
        std::vector<double> xi(16 * pl::kLanes, 0.0);
        pl::SVec beta_next = beta_end;
        for (int tid = 0; tid < pl::kLanes; ++tid) {
            const int lane = tid & 63, wave = tid >> 6, n = pl::lane_steps(nsteps, tid);
            pl::SVec a_lane = a_seg, run = a_seg;
            for (int w = 0; w + 1 < kWaves; ++w) {
                run = pl::vecmat(run, W[w]);
                if (w + 1 == wave) a_lane = run;
            }
            a_lane = pl::vecmat(a_lane, lane == 0 ? pl::identity() : P[tid - 1]);
            pl::SVec b_lane = beta_end;
            run = beta_end;
            for (int w = kWaves - 1; w >= 0; --w) {
                if (w == wave) b_lane = run;
                run = pl::matvec(W[w], run);
            }
            beta_next = run;
            b_lane = pl::matvec(lane == 63 ? pl::identity() : S[tid + 1], b_lane);
            constexpr int kHalf = pl::kLc / 2;
            pl::SVec a_mid = a_lane;
            for (int k = 0; k < kHalf; ++k)
                if (k < n) pl::step_alpha(a_mid, tb, stage.at(tid * pl::kLaneStride + 4 * k));
            const i64 t0 = first + static_cast<i64>(tid) * pl::kLc;
            for (int half = 1; half >= 0; --half) {
                const int k0 = half * kHalf;
                pl::SVec a[kHalf];
                a[0] = half ? a_mid : a_lane;
                for (int j = 0; j + 1 < kHalf; ++j) {
                    a[j + 1] = a[j];
                    if (k0 + j + 1 < n) pl::step_alpha(a[j + 1], tb, stage.at(tid * pl::kLaneStride + 4 * (k0 + j)));
                }
                for (int j = kHalf - 1; j >= 0; --j) {
                    const int k = k0 + j;
                    if (k >= n) continue;
                    double g[4];
                    pl::step_back(a[j], tb, stage.at(tid * pl::kLaneStride + 4 * k), b_lane, &xi[static_cast<size_t>(16 * tid)], g);
                    CHECK(t0 + k >= 1 && t0 + k < T, "gamma row %lld of %lld", t0 + k, T);
                    if (lab) {
                        const int y = lab[t0 + k] & 3, yp = lab[t0 + k - 1] & 3;
                        g[y] -= 1.0;
                        xi[static_cast<size_t>(16 * tid + 4 * yp + y)] -= 1.0;
                    }
                    for (int j2 = 0; j2 < 4; ++j2) {
                        CHECK(out.gamma[static_cast<size_t>(4 * (t0 + k) + j2)] == -7.0, "gamma row %lld written twice", t0 + k);
                        out.gamma[static_cast<size_t>(4 * (t0 + k) + j2)] = g[j2];
                    }
                }
            }
        }
        beta_end = beta_next;
        for (int i = 0; i < 16; ++i) out.xi[i] += reduce(xi, 16, i);
    }
    pl::step_zero(alpha0, beta_end, out.g0);
    if (lab) out.g0[lab[0] & 3] -= 1.0;
    for (int j = 0; j < 4; ++j) out.gamma[static_cast<size_t>(j)] = out.g0[j];
    return out;
}

static bool close(double got, double want, double scale)
{
    if (std::isinf(want) || std::isinf(got)) return got == want;
    return std::fabs(got - want) <= 1e-13 * std::fmax(scale, std::fabs(want));
}

int main()
{
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    const float ninf = -INFINITY;
    const int L = pl::kLc, S = pl::kSegSteps;
    const std::vector<i64> lengths = {1, 2, L - 1, L, L + 1, L + 2, 65 * L + 3, S - 1, S, S + 1, S + 2, 2 * S + 3, 5000};
    int cases = 0;
    for (int table = 0; table < 3; ++table)
        for (int mode = 0; mode < 4; ++mode) {            // 0 plain, 1 labels, 2 one all -inf step per recording (Z = 0), 3 NaN / -inf / wide
            float a_pi[20];
            for (int i = 0; i < 16; ++i) {
                const int r = i / 4, c = i % 4;
                if (table == 0) a_pi[i] = (c == r || c == (r + 1) % 4) ? (c == r ? std::log(0.9f) : std::log(0.1f)) : ninf;
                if (table == 1) a_pi[i] = std::log(0.05f + uni(rng));
                if (table == 2) a_pi[i] = (c == r || c == (r + 1) % 4) ? 0.0f : ninf;
            }
            for (int j = 0; j < 4; ++j) a_pi[16 + j] = table == 2 ? (j == 0 ? 0.0f : ninf) : std::log(0.1f + uni(rng));
            std::vector<i64> offs = {0};
            for (i64 T : lengths) offs.push_back(offs.back() + T);
            const i64 total = offs.back(), count = static_cast<i64>(lengths.size());
            std::vector<float> logp(static_cast<size_t>(4 * total));
            for (auto& v : logp) v = std::log(1e-3f + uni(rng)) * (mode == 3 ? 30.0f : 1.0f);
            std::vector<uint8_t> labels(static_cast<size_t>(total));
            for (i64 r = 0; r < count; ++r) {
                int s = table == 2 ? 0 : static_cast<int>(rng() % 4);
                for (i64 t = offs[r]; t < offs[r + 1]; ++t) {
                    labels[static_cast<size_t>(t)] = static_cast<uint8_t>(s);
                    if (rng() % 5 == 0) s = (s + 1) % 4;
                }
                const i64 T = offs[r + 1] - offs[r], mid = offs[r] + T / 2;
                if (mode == 2)
                    for (int j = 0; j < 4; ++j) logp[static_cast<size_t>(4 * mid + j)] = ninf;
                if (mode == 3) {
                    logp[static_cast<size_t>(4 * mid + 1)] = NAN;
                    logp[static_cast<size_t>(4 * (offs[r] + T - 1) + 2)] = ninf;
                }
            }
            CHECK(pl::workspace_bytes(total, count) >= pl::kCheckpointBytes * pl::checkpoint_slots(total, count), "workspace too small by its own rule");
            std::vector<double> work(static_cast<size_t>(pl::workspace_bytes(total, count) / 8), NAN);
            std::vector<int> owner(static_cast<size_t>(pl::checkpoint_slots(total, count)), -1);
            for (i64 r = 0; r < count; ++r) {
                const i64 T = offs[r + 1] - offs[r];
                const uint8_t* lab = mode == 1 ? labels.data() : nullptr;
                const Out got = simulate(logp.data(), offs[r], T, a_pi, lab, work, owner, r);
                std::vector<double> want(static_cast<size_t>(4 * T));
                const pl::Result ref = pl::posteriors_reference(logp.data() + 4 * offs[r], T, a_pi, lab ? lab + offs[r] : nullptr, want.data());
                CHECK(close(got.loglik, ref.loglik, 1.0), "logZ %.17g vs %.17g (T %lld table %d mode %d)", got.loglik, ref.loglik, T, table, mode);
                if (lab) CHECK(close(got.score, ref.score, 1.0), "score %.17g vs %.17g (T %lld)", got.score, ref.score, T);
                if (mode == 2) CHECK(std::isinf(got.loglik) && got.loglik < 0, "Z = 0 gives logZ %.17g", got.loglik);
                for (int i = 0; i < 16; ++i)
                    CHECK(close(got.xi[i], ref.xi[i], static_cast<double>(T)), "xi[%d] %.17g vs %.17g (T %lld table %d mode %d)", i, got.xi[i],
                          ref.xi[i], T, table, mode);
                for (size_t i = 0; i < want.size(); ++i) {
                    CHECK(close(got.gamma[i], want[i], 1.0), "gamma[%zu] %.17g vs %.17g (T %lld table %d mode %d)", i, got.gamma[i], want[i], T,
                          table, mode);
                    if (mode == 2) CHECK(got.gamma[i] == 0.0, "Z = 0 gives gamma %.17g", got.gamma[i]);
                }
                ++cases;
            }
        }
    // zero and denormal matrices renormalise without UB
    pl::SMat Z{};
    pl::renorm(Z);
    const pl::SMat ZZ = pl::matmul(Z, pl::identity());
    CHECK(ZZ.m[0][0] == 0.0 && ZZ.e == 0, "zero matrix");
    pl::SVec tiny{{5e-324, 0.0, 0.0, 0.0}, 0};
    pl::renorm(tiny);
    CHECK(tiny.v[0] == 0.5 && tiny.e == -1073, "denormal renormalises exactly: %g x 2^%d", tiny.v[0], tiny.e);
    if (failures) {
        std::printf("posteriors check FAILED: %d\n", failures);
        return 1;
    }
    std::printf("posteriors check ok: %d recordings\n", cases);
    return 0;
}
