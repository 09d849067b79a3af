// posterior_layout.hpp -- the arithmetic and the geometry of the forward-backward kernel (hssfsst.h: hssfsst_posteriors), as plain
// functions shared by the kernel (segmenter_posteriors.hpp) and a CPU check (tests/native/posteriors_check.cpp).  No HIP call here.
//
// Linear domain, float64, scaled.  With b_t[j] = exp(e[t][j] - max_j e[t][j]), P = exp(A), p0 = exp(pi):
//   alpha_0 = p0 . b_0;   alpha_t = (alpha_(t-1) P) . b_t;   beta_(T-1) = 1;   beta_(t-1) = P (b_t . beta_t)
// Every running vector or 4 x 4 transfer matrix is a float64 mantissa with an integer exponent and is renormalised after EVERY
// product by the power of two of its largest entry (frexp / ldexp: exact), so nothing underflows that is within ~700 nats of the
// largest entry, and there is no subtraction anywhere: all entries are >= 0 and any association order of the products is safe.
//   logZ = log sum_j alpha_(T-1)[j] + exponent ln 2 + sum_t max_j e[t][j]
// gamma_t and the terms of Xi are normalised per step, so their exponents cancel and only the forward sweep carries one.
// THE LIMIT: a path whose weight is more than ~700 nats (float64 underflow) below the best path reaching the same step is dropped.
// Emissions within 200 of their step's maximum cannot trigger it with four states (3 x 200 < 708).  A and pi must be -inf or
// below ~700.  NaN emissions count as -inf; a step whose emissions are all -inf makes Z = 0: logZ = -inf, gamma = 0, Xi = 0.
//
// Geometry (decode_layout.hpp's).  Step 0 of a recording is computed directly; steps 1 .. T - 1 are walked in segments of
// kSegSteps = kLanes x kLc steps; lane l owns steps first + l kLc .. first + l kLc + kLc - 1 of its segment.  The forward sweep
// leaves the (mantissa of the) alpha BEFORE each segment in the caller's workspace; the reverse sweep walks the segments back.
// posteriors_reference() is the sequential loop and the specification.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define HSSFSST_POST_HD __host__ __device__
#else
#define HSSFSST_POST_HD
#endif

namespace hssfsst::postlayout {

using i64 = long long;

constexpr i64 kMaxSteps = i64(1) << 20;                  // per recording: at most ~2^11 binary exponents a step, 2^31 in an int
constexpr int kLanes = 256;                              // the workgroup
constexpr int kLc = 8;                                   // steps per lane and segment
constexpr int kSegSteps = kLanes * kLc;                  // steps per staged segment
// a staged step is four float64 (32 bytes); a lane's kLc steps are followed by 16 bytes of padding (decode_layout.hpp's reason)
constexpr int kLaneStride = kLc * 4 + 2;                 // in float64
constexpr int kStageWords = kLanes * kLaneStride;        // float64 of LDS: 69 632 bytes

HSSFSST_POST_HD inline int stage_index(int step_in_segment) { return (step_in_segment / kLc) * kLaneStride + (step_in_segment % kLc) * 4; }

struct SVec { double v[4]; int e; };                     // value = v x 2^e
struct SMat { double m[4][4]; int e; };                  // m[i][j]: weight from state i before to state j after, x 2^e

// x <- x / 2^k with 2^k the power of two just above the largest entry, e += k; a zero (or NaN) vector is left as it is
HSSFSST_POST_HD inline void renorm4(double* x, int* e)
{
    const double top = fmax(fmax(x[0], x[1]), fmax(x[2], x[3]));
    if (!(top > 0.0)) return;
    int k;
    (void)frexp(top, &k);
    for (int j = 0; j < 4; ++j) x[j] = ldexp(x[j], -k);
    *e += k;
}
HSSFSST_POST_HD inline void renorm(SVec& a) { renorm4(a.v, &a.e); }
HSSFSST_POST_HD inline void renorm(SMat& a)
{
    double top = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) top = fmax(top, a.m[i][j]);
    if (!(top > 0.0)) return;
    int k;
    (void)frexp(top, &k);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) a.m[i][j] = ldexp(a.m[i][j], -k);
    a.e += k;
}

HSSFSST_POST_HD inline SMat identity()
{
    SMat r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) r.m[i][j] = i == j ? 1.0 : 0.0;
    r.e = 0;
    return r;
}

// the (+, x) products, renormalised: a's steps first, then b's
HSSFSST_POST_HD inline SMat matmul(const SMat& a, const SMat& b)
{
    SMat r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j] + a.m[i][3] * b.m[3][j];
    r.e = a.e + b.e;
    renorm(r);
    return r;
}
HSSFSST_POST_HD inline SVec vecmat(const SVec& a, const SMat& b)      // row vector x matrix: alpha through b's steps
{
    SVec r;
    for (int j = 0; j < 4; ++j) r.v[j] = a.v[0] * b.m[0][j] + a.v[1] * b.m[1][j] + a.v[2] * b.m[2][j] + a.v[3] * b.m[3][j];
    r.e = a.e + b.e;
    renorm(r);
    return r;
}
HSSFSST_POST_HD inline SVec matvec(const SMat& a, const SVec& b)      // matrix x column vector: beta back through a's steps
{
    SVec r;
    for (int i = 0; i < 4; ++i) r.v[i] = a.m[i][0] * b.v[0] + a.m[i][1] * b.v[1] + a.m[i][2] * b.v[2] + a.m[i][3] * b.v[3];
    r.e = a.e + b.e;
    renorm(r);
    return r;
}

// The tables in the linear domain: P = exp(A), p0 = exp(pi), from the 20 floats {A row-major, pi}.  exp(-inf) = 0.
struct Tables { double P[4][4]; double p0[4]; };
HSSFSST_POST_HD inline Tables make_tables(const float* a_pi)
{
    Tables t;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) t.P[i][j] = exp(static_cast<double>(a_pi[4 * i + j]));
    for (int j = 0; j < 4; ++j) t.p0[j] = exp(static_cast<double>(a_pi[16 + j]));
    return t;
}

// One step's emissions -> b[j] = exp(e[j] - max e), NaN as -inf; returns max e, or 0 with b = 0 when the step is all -inf.
HSSFSST_POST_HD inline double step_weights(float e0, float e1, float e2, float e3, double* b)
{
    const float ninf = -std::numeric_limits<float>::infinity();
    e0 = e0 != e0 ? ninf : e0;
    e1 = e1 != e1 ? ninf : e1;
    e2 = e2 != e2 ? ninf : e2;
    e3 = e3 != e3 ? ninf : e3;
    const float top = fmaxf(fmaxf(e0, e1), fmaxf(e2, e3));
    if (top == ninf) {
        b[0] = b[1] = b[2] = b[3] = 0.0;
        return 0.0;
    }
    const double t = static_cast<double>(top);
    b[0] = e0 == top ? 1.0 : exp(static_cast<double>(e0) - t);
    b[1] = e1 == top ? 1.0 : exp(static_cast<double>(e1) - t);
    b[2] = e2 == top ? 1.0 : exp(static_cast<double>(e2) - t);
    b[3] = e3 == top ? 1.0 : exp(static_cast<double>(e3) - t);
    return t;
}

// alpha <- (alpha P) . b, renormalised
HSSFSST_POST_HD inline void step_alpha(SVec& a, const Tables& tb, const double* b)
{
    SVec r;
    for (int j = 0; j < 4; ++j) r.v[j] = (a.v[0] * tb.P[0][j] + a.v[1] * tb.P[1][j] + a.v[2] * tb.P[2][j] + a.v[3] * tb.P[3][j]) * b[j];
    r.e = a.e;
    renorm(r);
    a = r;
}
// ... and of a transfer matrix: every row is an alpha of its own
HSSFSST_POST_HD inline void step_matrix(SMat& M, const Tables& tb, const double* b)
{
    SMat r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            r.m[i][j] = (M.m[i][0] * tb.P[0][j] + M.m[i][1] * tb.P[1][j] + M.m[i][2] * tb.P[2][j] + M.m[i][3] * tb.P[3][j]) * b[j];
    r.e = M.e;
    renorm(r);
    M = r;
}

// What one step t >= 1 gives, from alpha_(t-1) (any scale), b_t and beta_t (any scale): the joint num[i][j] proportional to
// P(s_(t-1) = i, s_t = j | everything), normalised by its own sum (0 when that is 0): xi[16] += it, g[j] = its column sums =
// gamma_t; then beta <- P (b . beta), renormalised: beta_(t-1).
HSSFSST_POST_HD inline void step_back(const SVec& aprev, const Tables& tb, const double* b, SVec& beta, double* xi, double* g)
{
    double w[4], num[4][4], s = 0.0;
    for (int j = 0; j < 4; ++j) w[j] = b[j] * beta.v[j];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            num[i][j] = aprev.v[i] * tb.P[i][j] * w[j];
            s += num[i][j];
        }
    const double inv = s > 0.0 ? 1.0 / s : 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            num[i][j] = s > 0.0 ? num[i][j] * inv : 0.0;
            xi[4 * i + j] += num[i][j];
        }
    for (int j = 0; j < 4; ++j) g[j] = num[0][j] + num[1][j] + num[2][j] + num[3][j];
    SVec r;
    for (int i = 0; i < 4; ++i) r.v[i] = tb.P[i][0] * w[0] + tb.P[i][1] * w[1] + tb.P[i][2] * w[2] + tb.P[i][3] * w[3];
    r.e = 0;
    renorm(r);
    beta = r;
}

// gamma_0 from alpha_0 and beta_0
HSSFSST_POST_HD inline void step_zero(const SVec& a0, const SVec& beta, double* g)
{
    double s = 0.0;
    for (int j = 0; j < 4; ++j) {
        g[j] = a0.v[j] * beta.v[j];
        s += g[j];
    }
    const double inv = s > 0.0 ? 1.0 / s : 0.0;
    for (int j = 0; j < 4; ++j) g[j] = s > 0.0 ? g[j] * inv : 0.0;
}

// logZ from the alpha behind the last step and the sum of the step maxima
HSSFSST_POST_HD inline double log_z(const SVec& a, double max_sum)
{
    const double s = a.v[0] + a.v[1] + a.v[2] + a.v[3];
    if (!(s > 0.0)) return -std::numeric_limits<double>::infinity();
    return log(s) + static_cast<double>(a.e) * 0.693147180559945309417232121458 + max_sum;
}

// the segments of a recording of T steps: they cover steps 1 .. T - 1
HSSFSST_POST_HD inline i64 segments(i64 T) { return (T - 1 + kSegSteps - 1) / kSegSteps; }
HSSFSST_POST_HD inline i64 segment_first(i64 seg) { return 1 + seg * kSegSteps; }
HSSFSST_POST_HD inline int segment_steps(i64 T, i64 seg)
{
    const i64 left = T - segment_first(seg);
    return static_cast<int>(left < kSegSteps ? left : kSegSteps);
}
HSSFSST_POST_HD inline int lane_steps(int nsteps, int lane)
{
    const int left = nsteps - lane * kLc;
    return left < 0 ? 0 : (left < kLc ? left : kLc);
}

// The workspace: one checkpoint of four float64 (the alpha before a segment) per segment.  The recording that starts at step
// offset `off` as number `rec` of the list has its checkpoints from slot off / kSegSteps + rec on: consecutive recordings are
// floor(T / kSegSteps) + 1 >= segments(T) slots apart at least, and the list needs at most total / kSegSteps + count slots.
constexpr int kCheckpointBytes = 32;
constexpr i64 kWorkBytesPerStep = 1;                     // (generous: 32 / kSegSteps would do)
constexpr i64 kWorkBytesPerRecording = kCheckpointBytes;
HSSFSST_POST_HD inline i64 checkpoint_slot(i64 off, i64 rec) { return off / kSegSteps + rec; }
inline i64 checkpoint_slots(i64 total_steps, i64 count) { return total_steps / kSegSteps + count; }
inline i64 workspace_bytes(i64 total_steps, i64 count) { return kWorkBytesPerStep * total_steps + kWorkBytesPerRecording * count; }
static_assert(kCheckpointBytes <= kWorkBytesPerStep * kSegSteps, "a segment's steps pay for its checkpoint");

struct Result { double loglik, score; double xi[16]; };

// The specification: the sequential loop.  e (T, 4), a_pi (20) float32; labels (T) or nullptr; gamma (T, 4) out: gamma, or
// gamma - onehot(labels) with labels, in which case xi is Xi - counts(labels) as well.
template <class G>                                       // G: float (what the kernel stores) or double (for a check)
inline Result posteriors_reference(const float* e, i64 T, const float* a_pi, const uint8_t* labels, G* gamma)
{
    const Tables tb = make_tables(a_pi);
    std::vector<double> b(static_cast<size_t>(T) * 4);
    std::vector<SVec> alpha(static_cast<size_t>(T));
    Result out{};
    double max_sum = 0.0, score = 0.0;
    for (i64 t = 0; t < T; ++t) {
        max_sum += step_weights(e[4 * t], e[4 * t + 1], e[4 * t + 2], e[4 * t + 3], &b[static_cast<size_t>(t) * 4]);
        if (labels) {
            const float ev = e[4 * t + labels[t]];
            score += static_cast<double>(ev != ev ? -std::numeric_limits<float>::infinity() : ev) +
                     static_cast<double>(t ? a_pi[4 * labels[t - 1] + labels[t]] : a_pi[16 + labels[0]]);
        }
    }
    SVec a{{tb.p0[0] * b[0], tb.p0[1] * b[1], tb.p0[2] * b[2], tb.p0[3] * b[3]}, 0};
    renorm(a);
    alpha[0] = a;
    for (i64 t = 1; t < T; ++t) {
        step_alpha(a, tb, &b[static_cast<size_t>(t) * 4]);
        alpha[static_cast<size_t>(t)] = a;
    }
    out.loglik = log_z(a, max_sum);
    out.score = score;
    SVec beta{{1.0, 1.0, 1.0, 1.0}, 0};
    double g[4];
    for (i64 t = T - 1; t >= 0; --t) {
        if (t)
            step_back(alpha[static_cast<size_t>(t - 1)], tb, &b[static_cast<size_t>(t) * 4], beta, out.xi, g);
        else
            step_zero(alpha[0], beta, g);
        for (int j = 0; j < 4; ++j) gamma[4 * t + j] = static_cast<G>(labels ? g[j] - (labels[t] == j ? 1.0 : 0.0) : g[j]);
        if (labels && t) out.xi[4 * labels[t - 1] + labels[t]] -= 1.0;
    }
    return out;
}

}  // namespace hssfsst::postlayout
