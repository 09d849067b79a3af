// duration_counts_check.cpp -- csrc/duration_counts_layout.hpp in a program of its own, built with -fsanitize=address,undefined by
// tests/test_duration_counts.py: the runs variant of the two sweeps (csrc/segmenter_duration_posteriors.hpp, as
// tests/native/duration_posteriors_check.cpp simulates them, with the second stash and 1 / Z) and the counts kernel
// (csrc/segmenter_duration_counts.hpp) with its lanes, stages, window and workspace simulated on the host give
// duration_counts_reference()'s outputs bit for bit -- the counts and the first seven outputs --, and every stage, window, stash
// and output index stays inside its bounds and inside its recording.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "duration_counts_layout.hpp"

namespace dp = hssfsst::dplayout;
namespace dc = hssfsst::dclayout;
using dp::i64;
using dp::Sc;

static int failures = 0;
#define CHECK(cond, ...)                                                                                                                   \
    do {                                                                                                                                   \
        if (!(cond)) {                                                                                                                     \
            if (++failures < 20) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                                                                                  \
    } while (0)

struct Out { std::vector<float> gamma, onsets; dp::Result res; };

struct Work {                                            // the caller's workspace, as the C entry point lays it out
    dc::Workspace all;
    dp::Workspace lay;                                   // the sweeps' part of it
    std::vector<unsigned char> bytes;
    std::vector<int> owner;                              // of each checkpoint slot
    int D;
    Work(i64 total, i64 count, int D_) : all(dc::workspace(total, count, D_)), lay(all.sweeps),
                                          bytes(static_cast<size_t>(dc::workspace_bytes(total, count, D_)), 0xA5),
                                          owner(static_cast<size_t>(dp::checkpoint_slots(total, count)), -1), D(D_)
    {
        const dp::Workspace plain = dp::workspace(total, count, D_);
        CHECK(std::memcmp(&plain, &lay, sizeof plain) == 0, "the sweeps' part is dplayout's");
        CHECK(lay.end <= dp::workspace_bytes(total, count, D_) && lay.end <= all.g_mant, "the sweeps' part ends at %lld", lay.end);
        CHECK(all.end <= static_cast<i64>(bytes.size()), "layout %lld over %zu bytes", all.end, bytes.size());
        CHECK(all.g_mant % 16 == 0 && all.g_exp % 16 == 0 && all.invz_mant % 8 == 0 && all.invz_exp % 4 == 0, "alignment");
        CHECK(all.g_exp == all.g_mant + 32 * total && all.invz_mant == all.g_exp + 16 * total && all.invz_exp == all.invz_mant + 8 * count, "parts");
    }
    template <class V> V* at(i64 byte, i64 n)
    {
        CHECK(byte >= 0 && byte + n * static_cast<i64>(sizeof(V)) <= all.end, "workspace bytes %lld + %lld", byte, n);
        return reinterpret_cast<V*>(&bytes.at(static_cast<size_t>(byte)));
    }
    void fill(const float* dur, const float* edge)       // the fill launch
    {
        for (int s = 0; s < 8 * D; ++s) {
            const Sc x = dp::scaled_exp(static_cast<double>(s < 4 * D ? dur[s] : edge[s - 4 * D]));
            const i64 k = dp::table_index_of_source(s, D);
            CHECK(k >= 0 && k < 8 * static_cast<i64>(D), "table index %lld", k);
            *at<double>(lay.table_mant + 8 * k, 1) = x.m;
            *at<int>(lay.table_exp + 4 * k, 1) = x.e;
        }
    }
    Sc table(int which, int d, int j) { const i64 k = dp::table_index(which, d, j, D); return Sc{*at<double>(lay.table_mant + 8 * k, 1), *at<int>(lay.table_exp + 4 * k, 1)}; }
};

// one workgroup of the runs variant of the sweeps: recording `rec` of the list, its steps at `base` of the arenas
static Out simulate(const float* logp, i64 base, i64 T, const float* a_pi, const float* dur, const float* edge, int D, const uint8_t* labels,
                    Work& work, i64 rec)
{
    constexpr int kSeg = dp::kSegSteps, kL = dp::kLanes;
    const float* e = logp + 4 * base;
    const uint8_t* lab = labels ? labels + base : nullptr;
    const int R = dp::ring_slots(D);
    const i64 slot0 = dp::checkpoint_slot(base, rec);
    Out out{};
    out.gamma.assign(static_cast<size_t>(4 * T), -7.0f);
    out.onsets.assign(static_cast<size_t>(4 * T), -7.0f);
    std::vector<Sc> ring(static_cast<size_t>(4 * dp::kMaxRing), Sc{-1.0, 0});
    std::vector<Sc> cst(4 * kSeg);
    std::vector<double> Est(4 * kSeg), gst(4 * kSeg), ost(4 * kSeg);
    auto ring_at = [&](int slot, int j) -> Sc& {
        CHECK(slot >= 0 && slot < R && R <= dp::kMaxRing, "ring slot %d of %d", slot, R);
        return ring.at(static_cast<size_t>(4 * slot + j));
    };
    auto ckpt = [&](i64 seg) -> double* {
        const i64 slot = slot0 + seg;
        CHECK(slot >= 0 && slot < static_cast<i64>(work.owner.size()), "checkpoint slot %lld of %zu", slot, work.owner.size());
        CHECK(work.owner.at(static_cast<size_t>(slot)) == -1 || work.owner.at(static_cast<size_t>(slot)) == rec, "slot %lld shared", slot);
        work.owner.at(static_cast<size_t>(slot)) = static_cast<int>(rec);
        return work.at<double>(work.lay.checkpoints + 32 * slot, 4);
    };
    auto stash_m = [&](i64 row) { CHECK(row >= 0 && row < T, "stash row %lld", row); return work.at<double>(work.lay.stash_mant + 32 * (base + row), 4); };
    auto stash_e = [&](i64 row) { return work.at<int>(work.lay.stash_exp + 16 * (base + row), 4); };
    std::vector<dp::StateTables> tb(kL);
    std::vector<Sc> own(static_cast<size_t>(kL) * dp::kPerLane);
    for (int tid = 0; tid < kL; ++tid) {
        tb[tid] = dp::state_tables(a_pi, dp::lane_state(tid));
        for (int k = 0; k < dp::kPerLane; ++k) {
            const int d = dp::lane_duration(tid, k);
            own[static_cast<size_t>(tid) * dp::kPerLane + k] = d <= D ? work.table(0, d, dp::lane_state(tid)) : dp::zero();
        }
    }
    std::vector<int> writers(static_cast<size_t>(4 * dp::kMaxRing), 0);
    auto push = [&](int tid, Sc x, int cur, i64 left, bool at_end) {
        const int j = dp::lane_state(tid);
        for (int k = 0; k < dp::kPerLane; ++k) {
            if (dp::lane_duration(0, k) > D) break;
            const int d = dp::lane_duration(tid, k);
            if (d <= D && d <= left) {
                Sc L = own[static_cast<size_t>(tid) * dp::kPerLane + k];
                if (at_end || d == left) L = work.table(1, d, j);
                Sc w = dp::mul(x, L);
                const int slot = dp::ring_slot(cur, d, R);
                if (!(at_end || d == D)) w = dp::add(ring_at(slot, j), w);
                ring_at(slot, j) = w;
                CHECK(++writers.at(static_cast<size_t>(4 * slot + j)) == 1, "two lanes write ring word (%d, %d) in one step", slot, j);
            }
        }
    };

    // forward
    std::vector<double> E(static_cast<size_t>(4 * kL), 0.0);
    std::vector<Sc> b(kL), C(static_cast<size_t>(4 * kL));
    for (int tid = 0; tid < kL; ++tid) b[tid] = tb[tid].p0;
    int cur = 0;
    double sc = lab ? static_cast<double>(a_pi[16 + (lab[0] & 3)]) : 0.0;
    i64 run_first = 0;
    auto flush_stash = [&](i64 first, int n) {
        for (int s = 0; s < n; ++s)
            for (int i = 0; i < 4; ++i) { stash_m(first + s)[i] = cst.at(4 * s + i).m; stash_e(first + s)[i] = cst.at(4 * s + i).e; }
    };
    for (i64 r = 0; r < T; ++r) {
        const int s = static_cast<int>(r % kSeg);
        if (s == 0) {
            if (r > 0) flush_stash(r - kSeg, kSeg);
            for (int j = 0; j < 4; ++j) ckpt(r / kSeg)[j] = E[4 * j + j];       // lane j's own E[j]
        }
        std::fill(writers.begin(), writers.end(), 0);
        for (int tid = 0; tid < kL; ++tid) push(tid, b[tid], cur, T - r, r == 0);
        if (lab) {
            const int y = lab[r] & 3, yn = r + 1 < T ? lab[r + 1] & 3 : -1;
            sc += dp::label_terms(dp::emission(e[4 * r + y]), y, yn, r, T, &run_first, a_pi, dur, edge, D);
        }
        for (int tid = 0; tid < kL; ++tid)
            for (int i = 0; i < 4; ++i) E[4 * tid + i] += dp::emission(e[4 * r + i]);
        cur = cur + 1 == R ? 0 : cur + 1;
        for (int tid = 0; tid < kL; ++tid) {             // behind the barrier
            for (int i = 0; i < 4; ++i) C[4 * tid + i] = dp::norm(ring_at(cur, i));
            if (tid < 4) cst.at(4 * s + tid) = C[4 * tid + tid];
            if (r + 1 < T) b[tid] = dp::run_start(&C[4 * tid], &E[4 * tid], tb[tid].col, dp::lane_state(tid));
        }
    }
    flush_stash((T - 1) / kSeg * kSeg, static_cast<int>((T - 1) % kSeg) + 1);
    const Sc Z = dp::total(&C[0], &E[0]), invz = dp::inverse(Z);
    out.res.loglik = dp::log_of(Z);
    out.res.score = sc;
    *work.at<double>(work.all.invz_mant + 8 * rec, 1) = invz.m;
    *work.at<int>(work.all.invz_exp + 4 * rec, 1) = invz.e;

    // reverse
    std::vector<double> gam(kL, 0.0), xi(static_cast<size_t>(4 * kL), 0.0);
    std::vector<Sc> cseg(4 * kSeg);
    auto flush_out = [&](i64 first, i64 n) {
        for (i64 s = 0; s < n; ++s)
            for (int j = 0; j < 4; ++j) {
                CHECK(first + s < T, "gamma row %lld", first + s);
                out.gamma.at(static_cast<size_t>(4 * (first + s) + j)) = static_cast<float>(gst.at(4 * s + j)) - (lab && (lab[first + s] & 3) == j ? 1.0f : 0.0f);
                if (first + s + 1 < T) out.onsets.at(static_cast<size_t>(4 * (first + s + 1) + j)) = static_cast<float>(ost.at(4 * s + j));
            }
    };
    cur = 0;
    for (i64 u = T; u >= 1; --u) {
        const i64 r = u - 1;
        const int s = static_cast<int>(r % kSeg);
        if (u == T || s == kSeg - 1) {
            const i64 first = r - s;
            const int n = s + 1;
            if (u != T) flush_out(first + kSeg, T - (first + kSeg) < kSeg ? T - (first + kSeg) : kSeg);
            for (int q = 0; q < n; ++q)
                for (int i = 0; i < 4; ++i) cseg.at(4 * q + i) = Sc{stash_m(first + q)[i], stash_e(first + q)[i]};
            for (int j = 0; j < 4; ++j) {
                double acc = ckpt(first / kSeg)[j];
                for (int q = 0; q < n; ++q) {
                    acc += dp::emission(e[4 * (first + q) + j]);
                    Est.at(4 * q + j) = acc;
                }
            }
        }
        std::fill(writers.begin(), writers.end(), 0);
        std::vector<Sc> g(kL);
        for (int tid = 0; tid < kL; ++tid) {
            const int j = dp::lane_state(tid);
            const double* Eu = &Est.at(4 * s);
            const Sc* Cu = &cseg.at(4 * s);
            double S = 0.0;
            if (u == T) {
                g[tid] = dp::scaled_exp(Eu[j]);
                gam[tid] = dp::value(dp::mul(dp::mul(Cu[j], g[tid]), invz));
            } else {
                Sc CB[4];
                for (int i = 0; i < 4; ++i) CB[i] = dp::norm(ring_at(cur, i));
                g[tid] = dp::run_end(CB, Eu, tb[tid].row, j);
                double x[4];
                S = dp::run_changes(Cu, Eu, tb[tid].col, j, CB[j], invz, x);
                const double N = dp::value(dp::mul(dp::mul(Cu[j], g[tid]), invz));
                for (int i = 0; i < 4; ++i) xi[4 * tid + i] += x[i];
                if (lab && (lab[u - 1] & 3) != (lab[u] & 3) && (lab[u] & 3) == j) xi[4 * tid + (lab[u - 1] & 3)] -= 1.0;
                gam[tid] = (gam[tid] - S) + N;
            }
            if (tid < 4) {
                gst.at(4 * s + j) = static_cast<float>(dp::clamp01(gam[tid]));
                ost.at(4 * s + j) = static_cast<float>(S);
                CHECK(r >= 0 && r < T, "g row %lld", r);
                work.at<double>(work.all.g_mant + 32 * (base + r), 4)[j] = g[tid].m;      // g_u(j) into row u - 1
                work.at<int>(work.all.g_exp + 16 * (base + r), 4)[j] = g[tid].e;
            }
        }
        for (int tid = 0; tid < kL; ++tid) push(tid, g[tid], cur, u, u == T);
        cur = cur + 1 == R ? 0 : cur + 1;
    }
    flush_out(0, T < kSeg ? T : kSeg);
    for (int j = 0; j < 4; ++j) {
        const double S0 = dp::value(dp::mul(dp::mul(tb[j].p0, dp::norm(ring_at(cur, j))), invz));
        out.onsets.at(j) = static_cast<float>(S0);
        out.res.s0[j] = S0 - (lab && (lab[0] & 3) == j ? 1.0 : 0.0);
        for (int i = 0; i < 4; ++i) out.res.xi[4 * i + j] = xi[4 * j + i];
    }
    return out;
}

// one workgroup of the counts kernel: recording `rec`, block `block` of durations; counts: the launch's (count, 2, 4, D)
static void simulate_counts(const float* logp, i64 base, i64 T, const float* a_pi, int D, const uint8_t* labels, Work& work, i64 rec, int block,
                            std::vector<double>& counts, std::vector<int>& written)
{
    constexpr int kSeg = dc::kSegSteps, kL = dc::kLanes;
    const float* e = logp + 4 * base;
    const uint8_t* lab = labels ? labels + base : nullptr;
    auto put = [&](int which, int j, int d, double v) {
        CHECK(d >= 1 && d <= D && j >= 0 && j < 4, "output (%d, %d)", j, d);
        const size_t at = static_cast<size_t>(dc::counts_index(rec, which, j, d, D));
        counts.at(at) = v;
        CHECK(++written.at(at) == 1, "counts word %zu written twice", at);
    };
    if (dc::lane_duration(0, block) > T) {
        for (int tid = 0; tid < kL; ++tid)
            if (dc::lane_duration(tid, block) <= D) { put(0, dc::lane_state(tid), dc::lane_duration(tid, block), 0.0); put(1, dc::lane_state(tid), dc::lane_duration(tid, block), 0.0); }
        return;
    }
    std::vector<dp::StateTables> tb(4);
    for (int j = 0; j < 4; ++j) tb[static_cast<size_t>(j)] = dp::state_tables(a_pi, j);
    const Sc invz{*work.at<double>(work.all.invz_mant + 8 * rec, 1), *work.at<int>(work.all.invz_exp + 4 * rec, 1)};
    std::vector<Sc> lzd(kL, dp::zero()), lze(kL, dp::zero());
    for (int tid = 0; tid < kL; ++tid) {
        const int d = dc::lane_duration(tid, block), j = dc::lane_state(tid);
        if (d <= D) { lzd[tid] = dp::mul(work.table(0, d, j), invz); lze[tid] = dp::mul(work.table(1, d, j), invz); }
    }
    std::vector<double> acc0(kL, 0.0), acc1(kL, 0.0);
    std::vector<i64> run_first(kL, 0);
    std::vector<Sc> cst(4 * kSeg), bst(4 * kSeg), gw(4 * dc::kWindowRows);
    std::vector<double> Est(4 * kSeg);
    std::vector<char> cst_set(kSeg), gw_set(dc::kWindowRows);
    const i64 slot0 = dp::checkpoint_slot(base, rec);
    for (i64 t0 = 0; t0 < T; t0 += kSeg) {
        const int n = static_cast<int>(T - t0 < kSeg ? T - t0 : kSeg);
        std::fill(cst_set.begin(), cst_set.end(), 0);
        std::fill(gw_set.begin(), gw_set.end(), 0);
        for (int q = 0; q < n; ++q)
            if (t0 + q >= 1) {
                const i64 row = t0 + q - 1;
                CHECK(row >= 0 && row < T, "stash row %lld of %lld", row, T);
                for (int i = 0; i < 4; ++i)
                    cst.at(4 * q + i) = Sc{work.at<double>(work.lay.stash_mant + 32 * (base + row), 4)[i], work.at<int>(work.lay.stash_exp + 16 * (base + row), 4)[i]};
                cst_set.at(q) = 1;
            }
        const i64 first = dc::window_first(t0, block);
        for (int w = 0; w < dc::kWindowRows && first + w < T; ++w) {
            CHECK(first + w >= 0 && first + w < T, "g row %lld of %lld", first + w, T);
            for (int i = 0; i < 4; ++i)
                gw.at(4 * w + i) = Sc{work.at<double>(work.all.g_mant + 32 * (base + first + w), 4)[i], work.at<int>(work.all.g_exp + 16 * (base + first + w), 4)[i]};
            gw_set.at(w) = 1;
        }
        for (int j = 0; j < 4; ++j) {
            const i64 slot = slot0 + t0 / kSeg;
            CHECK(work.owner.at(static_cast<size_t>(slot)) == rec, "checkpoint slot %lld is recording %d's", slot, work.owner.at(static_cast<size_t>(slot)));
            double acc = work.at<double>(work.lay.checkpoints + 32 * slot, 4)[j];
            for (int q = 0; q < n; ++q) {
                Est.at(4 * q + j) = acc;
                acc += dp::emission(e[4 * (t0 + q) + j]);
            }
        }
        for (int tid = 0; tid < kL; ++tid)
            for (int k = 0; k < kSeg / dc::kDurationsPerGroup; ++k) {
                const int q = (tid >> 2) + k * dc::kDurationsPerGroup, j = dc::lane_state(tid);
                if (q < n) {
                    Sc b = tb[static_cast<size_t>(j)].p0;
                    if (t0 + q >= 1) {
                        CHECK(cst_set.at(q), "c row %d not staged", q);
                        b = dp::run_start(&cst.at(4 * q), &Est.at(4 * q), tb[static_cast<size_t>(j)].col, j);
                    }
                    bst.at(4 * q + j) = b;
                }
            }
        for (int tid = 0; tid < kL; ++tid) {
            const int d = dc::lane_duration(tid, block), j = dc::lane_state(tid);
            const bool owner = d <= D;
            for (int q = 0; q < n; ++q) {
                const i64 t = t0 + q;
                if (owner && t + d <= T) {
                    const int w = dc::window_row(q, tid);
                    CHECK(w >= 0 && w < dc::kWindowRows && gw_set.at(w), "window row %d not staged (t %lld d %d T %lld)", w, t, d, T);
                    CHECK(first + w == dc::g_row(t, d), "window row %d is g row %lld, not %lld", w, first + w, dc::g_row(t, d));
                    const bool edge_run = dc::at_edge(t, d, T);
                    const double v = dc::run_weight(bst.at(4 * q + j), gw.at(4 * w + j), edge_run ? lze[tid] : lzd[tid]);
                    acc0[tid] += edge_run ? 0.0 : v;
                    acc1[tid] += edge_run ? v : 0.0;
                }
                if (lab) {
                    i64 run;
                    bool edge_run;
                    const int y = lab[t] & 3, yn = t + 1 < T ? lab[t + 1] & 3 : -1;
                    if (dc::label_run_ends(y, yn, t, T, &run_first[tid], &run, &edge_run) && owner && y == j && run == d) {
                        if (edge_run) acc1[tid] -= 1.0; else acc0[tid] -= 1.0;
                    }
                }
            }
        }
    }
    for (int tid = 0; tid < kL; ++tid)
        if (dc::lane_duration(tid, block) <= D) {
            put(0, dc::lane_state(tid), dc::lane_duration(tid, block), acc0[tid]);
            put(1, dc::lane_state(tid), dc::lane_duration(tid, block), acc1[tid]);
        }
}

static bool same(double a, double b) { return a == b || (a != a && b != b); }

int main()
{
    std::mt19937_64 rng(78);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    const int kSeg = dc::kSegSteps;
    static_assert(dc::kWorkBytesPerStep == 97 && dc::kWorkBytesPerRecording == 48 && dc::kWorkBytesPerDuration == 96, "the documented factors");
    struct Case { int D; std::vector<i64> lens; int special; };      // special 1: an edge table that forbids everything; 2: -inf / NaN emissions
    const std::vector<Case> cases = {
        {1, {1, 2, 3, 9, kSeg + 1}, 0}, {2, {1, 2, 3, 7, kSeg, 2 * kSeg + 1}, 0}, {127, {126, 127, 128, 2 * 128 + 3, kSeg - 1}, 0},
        {128, {1, 127, 128, 129, kSeg, kSeg + 1, 2 * 129 + 3}, 0}, {129, {1, 128, 129, 130, 2 * 130 + 3, kSeg - 1, kSeg, 2 * kSeg + 1}, 0},
        {512, {3, 511, 512, 513, kSeg + 1, 2 * 513 + 3}, 0}, {2048, {1, 300, 2047, 2049}, 0}, {5, {3, 20}, 1}, {4, {6, kSeg + 2}, 2}};
    for (size_t ci = 0; ci < cases.size(); ++ci) {
        const Case& cs = cases[ci];
        const int D = cs.D;
        std::vector<float> a_pi(20), dur(4 * static_cast<size_t>(D)), edge(4 * static_cast<size_t>(D));
        for (auto& v : a_pi) v = uni(rng) < 0.2 ? -INFINITY : static_cast<float>(-3.0 * uni(rng));
        for (int i = 0; i < 4; ++i) a_pi[static_cast<size_t>(4 * i + (i + 1) % 4)] = -0.5f;
        a_pi[16] = -0.25f;
        for (auto& v : dur) v = uni(rng) < 0.3 ? -INFINITY : static_cast<float>(-4.0 * uni(rng));
        for (auto& v : edge) v = cs.special == 1 ? -INFINITY : static_cast<float>(-4.0 * uni(rng));
        for (int j = 0; j < 4; ++j) dur[static_cast<size_t>(j) * D + (D - 1)] = -1.0f;
        std::vector<i64> off{0};
        for (i64 T : cs.lens) off.push_back(off.back() + T);
        const i64 total = off.back(), count = static_cast<i64>(cs.lens.size());
        std::vector<float> logp(static_cast<size_t>(4 * total));
        std::vector<uint8_t> labels(static_cast<size_t>(total));
        for (auto& v : logp) v = static_cast<float>(-30.0 * uni(rng) * uni(rng));
        if (cs.special == 2) { logp[1] = -INFINITY; logp[6] = NAN; for (int i = 8; i < 12; ++i) logp[static_cast<size_t>(i)] = -INFINITY; }
        for (i64 i = 0; i < count; ++i) {
            int s = static_cast<int>(rng() % 4);
            for (i64 t = off[i]; t < off[i + 1];) {
                const i64 d = 1 + static_cast<i64>(rng() % static_cast<unsigned>(D < 9 ? D + 1 : 9));    // (a run of D + 1 at times: nothing is taken off)
                for (i64 k = 0; k < d && t < off[i + 1]; ++k) labels[static_cast<size_t>(t++)] = static_cast<uint8_t>(s);
                s = (s + 1) % 4;
            }
        }
        for (int with_labels = 0; with_labels < 2; ++with_labels) {
            Work work(total, count, D);
            work.fill(dur.data(), edge.data());
            const uint8_t* lab = with_labels ? labels.data() : nullptr;
            std::vector<Out> outs;
            for (i64 i = 0; i < count; ++i)              // the sweep launch
                outs.push_back(simulate(logp.data(), off[i], cs.lens[static_cast<size_t>(i)], a_pi.data(), dur.data(), edge.data(), D, lab, work, i));
            std::vector<double> counts(static_cast<size_t>(8 * count * D), -7.0);
            std::vector<int> written(counts.size(), 0);
            for (i64 i = 0; i < count; ++i)              // the counts launch
                for (int block = 0; block < dc::groups(D); ++block)
                    simulate_counts(logp.data(), off[i], cs.lens[static_cast<size_t>(i)], a_pi.data(), D, lab, work, i, block, counts, written);
            for (size_t k = 0; k < written.size(); ++k) CHECK(written[k] == 1, "case %zu: counts word %zu written %d times", ci, k, written[k]);
            for (i64 i = 0; i < count; ++i) {
                const i64 T = cs.lens[static_cast<size_t>(i)];
                const Out& got = outs[static_cast<size_t>(i)];
                std::vector<float> wg(static_cast<size_t>(4 * T)), wo(static_cast<size_t>(4 * T), -7.0f);
                std::vector<double> wc(static_cast<size_t>(8 * D), -7.0);
                const dp::Result want = dc::duration_counts_reference(logp.data() + 4 * off[i], T, a_pi.data(), dur.data(), edge.data(), D,
                                                                      lab ? lab + off[i] : nullptr, wg.data(), wo.data(), wc.data());
                CHECK(same(got.res.loglik, want.loglik), "case %zu rec %lld: logZ %.17g vs %.17g", ci, i, got.res.loglik, want.loglik);
                if (lab) CHECK(same(got.res.score, want.score), "case %zu rec %lld: score %.17g vs %.17g", ci, i, got.res.score, want.score);
                for (int k = 0; k < 16; ++k) CHECK(same(got.res.xi[k], want.xi[k]), "case %zu rec %lld: xi[%d] %.17g vs %.17g", ci, i, k, got.res.xi[k], want.xi[k]);
                for (int k = 0; k < 4; ++k) CHECK(same(got.res.s0[k], want.s0[k]), "case %zu rec %lld: s0[%d]", ci, i, k);
                CHECK(std::memcmp(got.gamma.data(), wg.data(), wg.size() * sizeof(float)) == 0, "case %zu rec %lld (T %lld, D %d): gamma", ci, i, T, D);
                CHECK(std::memcmp(got.onsets.data(), wo.data(), wo.size() * sizeof(float)) == 0, "case %zu rec %lld (T %lld, D %d): onsets", ci, i, T, D);
                double sum = 0.0, steps = 0.0;
                for (int k = 0; k < 8 * D; ++k) {
                    const double g = counts[static_cast<size_t>(8 * i * D + k)];
                    CHECK(same(g, wc[static_cast<size_t>(k)]), "case %zu rec %lld (T %lld, D %d, labels %d): counts[%d] %.17g vs %.17g", ci, i, T, D, with_labels, k, g, wc[static_cast<size_t>(k)]);
                    sum += g;
                    steps += g * (k % D + 1);
                }
                if (cs.special == 1 && T > D) CHECK(sum == 0.0 || with_labels, "case %zu rec %lld: counts %g where nothing fits", ci, i, sum);
                // every step belongs to one run: sum_d d counts = T (without labels, where something fits)
                if (!with_labels && std::isfinite(want.loglik)) CHECK(std::fabs(steps - static_cast<double>(T)) <= 1e-9 * static_cast<double>(T), "case %zu rec %lld: %g steps in runs, T = %lld", ci, i, steps, T);
            }
        }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("duration counts check ok\n");
    return 0;
}
