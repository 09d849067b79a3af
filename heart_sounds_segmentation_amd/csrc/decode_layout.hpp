// decode_layout.hpp -- the arithmetic and the geometry of the Viterbi decoder (hssfsst.h: hssfsst_decode_states), as plain
// functions shared by the kernel (segmenter_decode.hpp) and a CPU check (tests/native/decode_check.cpp).  No HIP call here.
//
// Every input (emission, log transition, log initial score) becomes an int64 fixed-point number with 20 fraction bits; from there
// on the decoder only adds and takes maxima of int64, so the (max, +) products below are exactly associative and a recording may
// be cut into per-lane chunks whose 4 x 4 transfer matrices are combined in any order: the result is the sequential loop's, bit
// for bit.  decode_reference() is that loop and the specification.
//
// Geometry.  Step 0 of a recording has no predecessor: d_0 = q(pi) + q(e[0]) is computed directly.  Steps 1 .. T - 1 are walked
// in segments of kSegSteps = kLanes x kLc steps; lane l of the workgroup owns steps first + l kLc .. first + l kLc + kLc - 1 of
// its segment, in the forward pass (which writes one backpointer byte per step into the path output) and in the backtrace (which
// reads each byte back and overwrites it with the state), so a byte is only ever touched by the lane that wrote it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define HSSFSST_DEC_HD __host__ __device__
#else
#define HSSFSST_DEC_HD
#endif

namespace hssfsst::declayout {

using i64 = long long;

constexpr i64 kNeg = std::numeric_limits<i64>::min();    // "forbidden": absorbs every add, loses every max
constexpr int kFracBits = 20;
constexpr float kClamp = 32768.0f;                       // |x| is clamped to this before scaling: |q| <= 2^35
constexpr i64 kMaxTerm = i64(1) << 35;
constexpr i64 kMaxSteps = i64(1) << 26;                  // per recording: 2 terms per step, 2^26 x 2 x 2^35 = 2^62 < 2^63
static_assert(kMaxSteps * 2 <= (i64(1) << 62) / kMaxTerm, "a path's score must stay within 2^62");

constexpr int kLanes = 256;                              // the workgroup
constexpr int kLc = 8;                                   // steps per lane and segment
constexpr int kSegSteps = kLanes * kLc;                  // steps per staged segment
// a staged step is four int64 (32 bytes); a lane's kLc steps are followed by 16 bytes of padding, so the lanes of one 128-bit
// LDS read are 68 dwords apart instead of 64 and fall on different banks
constexpr int kLaneStride = kLc * 4 + 2;                 // in int64
constexpr int kStageWords = kLanes * kLaneStride;        // int64 of LDS: 69 632 bytes

HSSFSST_DEC_HD inline int stage_index(int step_in_segment) { return (step_in_segment / kLc) * kLaneStride + (step_in_segment % kLc) * 4; }

// q(x) = rint(clamp(x, -32768, +32768) 2^20), half to even; q(NaN) = q(-32768); q(-inf) = kNeg; +inf clamps.
HSSFSST_DEC_HD inline i64 quantise(float x)
{
    if (x != x) x = -kClamp;
    if (x < -std::numeric_limits<float>::max()) return kNeg;
    x = x < -kClamp ? -kClamp : (x > kClamp ? kClamp : x);
    return static_cast<i64>(rint(static_cast<double>(x) * static_cast<double>(i64(1) << kFracBits)));
}

HSSFSST_DEC_HD inline i64 add(i64 a, i64 b) { return (a == kNeg || b == kNeg) ? kNeg : a + b; }
HSSFSST_DEC_HD inline i64 max2(i64 a, i64 b) { return b > a ? b : a; }

struct Vec { i64 v[4]; };
struct Mat { i64 m[4][4]; };                             // m[i][j]: best score from state i before to state j after

HSSFSST_DEC_HD inline Mat identity()
{
    Mat r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) r.m[i][j] = i == j ? 0 : kNeg;
    return r;
}

// the (max, +) products: (a b)[i][j] = max_k a[i][k] + b[k][j]: a's steps first, then b's
HSSFSST_DEC_HD inline Mat matmul(const Mat& a, const Mat& b)
{
    Mat r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            i64 best = add(a.m[i][0], b.m[0][j]);
            for (int k = 1; k < 4; ++k) best = max2(best, add(a.m[i][k], b.m[k][j]));
            r.m[i][j] = best;
        }
    return r;
}
HSSFSST_DEC_HD inline Vec vecmat(const Vec& d, const Mat& b)
{
    Vec r;
    for (int j = 0; j < 4; ++j) {
        i64 best = add(d.v[0], b.m[0][j]);
        for (int k = 1; k < 4; ++k) best = max2(best, add(d.v[k], b.m[k][j]));
        r.v[j] = best;
    }
    return r;
}

// One step of the recurrence: d <- (max_i d[i] + A[i][j]) + e[j]; returns the step's backpointer byte, psi[j] -- the SMALLEST i
// that attains the max -- in bits 2j, 2j + 1.
HSSFSST_DEC_HD inline unsigned step(Vec& d, const Mat& A, const Vec& e)
{
    Vec n;
    unsigned byte = 0;
    for (int j = 0; j < 4; ++j) {
        i64 best = add(d.v[0], A.m[0][j]);
        unsigned arg = 0;
        for (int i = 1; i < 4; ++i) {
            const i64 c = add(d.v[i], A.m[i][j]);
            if (c > best) { best = c; arg = static_cast<unsigned>(i); }
        }
        n.v[j] = add(best, e.v[j]);
        byte |= arg << (2 * j);
    }
    d = n;
    return byte;
}
// ... and of a transfer matrix: every row is a d of its own (the emission added after the max is the same number)
HSSFSST_DEC_HD inline void step_matrix(Mat& M, const Mat& A, const Vec& e)
{
    for (int r = 0; r < 4; ++r) {
        Vec d{{M.m[r][0], M.m[r][1], M.m[r][2], M.m[r][3]}};
        (void)step(d, A, e);
        for (int j = 0; j < 4; ++j) M.m[r][j] = d.v[j];
    }
}

// A backpointer byte is a map state at t -> state at t - 1, four 2-bit entries.
constexpr unsigned kIdentityMap = 0xE4u;                 // 3, 2, 1, 0
HSSFSST_DEC_HD inline unsigned map_apply(unsigned map, unsigned s) { return (map >> (2 * s)) & 3u; }
// (outer o inner)(s) = outer(inner(s)): inner is the LATER step's map
HSSFSST_DEC_HD inline unsigned map_compose(unsigned outer, unsigned inner)
{
    return map_apply(outer, inner & 3u) | (map_apply(outer, (inner >> 2) & 3u) << 2) | (map_apply(outer, (inner >> 4) & 3u) << 4) |
           (map_apply(outer, (inner >> 6) & 3u) << 6);
}

// the smallest j that attains max d
HSSFSST_DEC_HD inline unsigned end_state(const Vec& d, i64* score)
{
    i64 best = d.v[0];
    unsigned arg = 0;
    for (int j = 1; j < 4; ++j)
        if (d.v[j] > best) { best = d.v[j]; arg = static_cast<unsigned>(j); }
    *score = best;
    return arg;
}

// the segments of a recording of T steps: they cover steps 1 .. T - 1
HSSFSST_DEC_HD inline i64 segments(i64 T) { return (T - 1 + kSegSteps - 1) / kSegSteps; }
HSSFSST_DEC_HD inline i64 segment_first(i64 seg) { return 1 + seg * kSegSteps; }
HSSFSST_DEC_HD inline int segment_steps(i64 T, i64 seg) 
{
    const i64 left = T - segment_first(seg);
    return static_cast<int>(left < kSegSteps ? left : kSegSteps);
}
// the steps of lane `lane` in a segment of nsteps steps
HSSFSST_DEC_HD inline int lane_steps(int nsteps, int lane) 
{
    const int left = nsteps - lane * kLc;
    return left < 0 ? 0 : (left < kLc ? left : kLc);
}

struct Segment { i64 first; int steps; };
inline std::vector<Segment> segment_list(i64 T)
{
    std::vector<Segment> out;
    for (i64 s = 0; s < segments(T); ++s) out.push_back({segment_first(s), segment_steps(T, s)});
    return out;
}

inline Mat quantise_transitions(const float* A)
{
    Mat r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) r.m[i][j] = quantise(A[4 * i + j]);
    return r;
}
inline Vec quantise4(const float* p) { return Vec{{quantise(p[0]), quantise(p[1]), quantise(p[2]), quantise(p[3])}}; }

// The specification: the sequential loop.  e (T, 4), A (4, 4), pi (4) float32; states (T) out; returns the score.
inline i64 decode_reference(const float* e, i64 T, const float* A, const float* pi, uint8_t* states)
{
    const Mat qa = quantise_transitions(A);
    const Vec qp = quantise4(pi), e0 = quantise4(e);
    Vec d;
    for (int j = 0; j < 4; ++j) d.v[j] = add(qp.v[j], e0.v[j]);
    std::vector<uint8_t> psi(static_cast<size_t>(T), 0);
    for (i64 t = 1; t < T; ++t) psi[static_cast<size_t>(t)] = static_cast<uint8_t>(step(d, qa, quantise4(e + 4 * t)));
    i64 score;
    unsigned s = end_state(d, &score);
    for (i64 t = T - 1; t >= 1; --t) {
        states[t] = static_cast<uint8_t>(s);
        s = map_apply(psi[static_cast<size_t>(t)], s);
    }
    states[0] = static_cast<uint8_t>(s);
    return score;
}

}  // namespace hssfsst::declayout
