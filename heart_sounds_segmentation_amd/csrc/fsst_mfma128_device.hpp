// fsst_mfma128_device.hpp -- the MFMA core's device functions, and no kernel: the per-lane FFTs, the displaced-source and
// rounding-tie machinery, the float64 "exact group" pass, process_stripe.  fsst_core128_kernel (fsst_mfma128.hpp, where the design is
// described) is made of them, and the canonical-band, team, any-length and ragged kernels use them too.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "fsst_device.hpp"
#include "fsst_launch_shape.hpp"

namespace hssfsst {

using f2 = float __attribute__((ext_vector_type(2)));
using f4 = float __attribute__((ext_vector_type(4)));
using lds_float = __attribute__((address_space(3))) float;

// (Work distribution -- the chunk pattern of a launch, Core128Regions -- and the LDS layout functions: fsst_launch_shape.hpp)

// (RaggedSignal, Core128Params: fsst_device.hpp, the kernel-free header the host reads them from)


// cos / sin of 2*pi*j/16, j = 0..7
__device__ constexpr float kCos16[8] = {1.0f, 0.92387953251128674f, 0.70710678118654757f, 0.38268343236508978f,
                                        0.0f, -0.38268343236508973f, -0.70710678118654746f, -0.92387953251128674f};
__device__ constexpr float kSin16[8] = {0.0f, 0.38268343236508978f, 0.70710678118654746f, 0.92387953251128674f,
                                        1.0f, 0.92387953251128674f, 0.70710678118654757f, 0.38268343236508984f};

// (cos / sin of 2*pi*j/32 for the 32-tap variant, nwin = 512: kCos32 / kSin32 of fsst_device.hpp)
constexpr __host__ __device__ int bitrev4(int n) { return ((n & 1) << 3) | ((n & 2) << 1) | ((n & 4) >> 1) | ((n & 8) >> 3); }
template <int N>
constexpr __host__ __device__ int bitrev_n(int n)
{
    return N == 16 ? bitrev4(n) : ((bitrev4(n & 15) << 1) | (n >> 4));        // N == 32: 5 bits
}

__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

// Packed complex helpers with VOP3P operand swizzles (op_sel) and sign modifiers (neg_lo/neg_hi):
// hipcc materialises (y, -x)-style operands with v_xor + v_mov instead of using the modifiers.
// Inputs of these statements are always results of ordinary VALU instructions (never MFMA
// destinations), so no manual hazard padding is needed inside the strings.
// Two-for-one unpack of a source bin X = Z[k'] with conjugate partner P = Z[128 - k'], emitted directly in
// the operand layout of the packed den/num product below:
//   V   = X + conj(P)       = (X.x + P.x, X.y - P.y)
//   Vd' = (X - conj(P)) / i = (X.y + P.y, P.x - X.x)
__device__ __forceinline__ f2 mix_re(f2 x, f2 p)         // (V.re, Vd'.im) = (p.x + x.x, p.x - x.x)
{
    f2 d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,0] neg_hi:[0,1]" : "=v"(d) : "v"(p), "v"(x)); return d;
}
__device__ __forceinline__ f2 mix_im(f2 x, f2 p)         // (V.im, Vd'.re) = (x.y - p.y, x.y + p.y)
{
    f2 d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,1] neg_lo:[0,1]" : "=v"(d) : "v"(x), "v"(p)); return d;
}
// (den, num) = (|V|^2, Vd'.re V.im - Vd'.im V.re) in two packed FMAs: t1 = mix_re, t2 = mix_im
__device__ __forceinline__ f2 dn_first(f2 t1, f2 c)      // (t1.lo^2, -t1.lo t1.hi) + c
{
    f2 d; asm("v_pk_fma_f32 %0, %1, %1, %2 op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_hi:[0,1,0]" : "=v"(d) : "v"(t1), "s"(c)); return d;
}
__device__ __forceinline__ f2 dn_second(f2 t2, f2 m)     // (t2.lo^2, t2.lo t2.hi) + m
{
    f2 d; asm("v_pk_fma_f32 %0, %1, %1, %2 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "=v"(d) : "v"(t2), "v"(m)); return d;
}
__device__ __forceinline__ f2 add_mi(f2 e, f2 o)         // e + (-i) o
{
    f2 d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(d) : "v"(e), "v"(o)); return d;
}
__device__ __forceinline__ f2 sub_mi(f2 e, f2 o)         // e - (-i) o
{
    f2 d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(d) : "v"(e), "v"(o)); return d;
}
// Radix-2 DIT butterfly on packed complex values, twiddle W = exp(-2*pi*i*TW/N), N = 16 or 32.
template <int N, int TW>
__device__ __forceinline__ void bfly_n(f2& e, f2& o)
{
    f2 a, b;
    if constexpr (TW == 0) {
        a = e + o; b = e - o;
    } else if constexpr (TW == N / 4) {                 // W = -i: W o = (o.im, -o.re)
        a = add_mi(e, o); b = sub_mi(e, o);
    } else {                                            // W = wr + i wi, wr = cos, wi = -sin
        constexpr float wr = (N == 16) ? kCos16[TW & 7] : kCos32[TW & 15];
        constexpr float wi = (N == 16) ? -kSin16[TW & 7] : -kSin32[TW & 15];
        const f2 t1 = pk_fma(f2{o.x, o.x}, f2{wr, wi}, e);
        a = pk_fma(f2{o.y, o.y}, f2{-wi, wr}, t1);      // e + W o
        b = pk_fma(e, f2{2.0f, 2.0f}, -a);              // e - W o = 2e - (e + W o)
    }
    e = a; o = b;
}

// In-place N-point complex FFT (forward), N = 16 or 32; input in bit-reversed order, output natural order.
template <int N>
__device__ __forceinline__ void fft_n(f2 (&z)[N])
{
    constexpr int LOG2N = (N == 16) ? 4 : 5;
    static_for<LOG2N>([&](auto S) {
        constexpr int L = 2 << decltype(S)::value;
        constexpr int H = L / 2;
        constexpr int STEP = N / L;
        static_for<N / 2>([&](auto B) {
            constexpr int b = decltype(B)::value;
            constexpr int j = b % H;
            constexpr int a = (b / H) * L + j;
            bfly_n<N, j * STEP>(z[a], z[a + H]);
        });
    });
}

constexpr int kMaxWavesPerBlock = 16;        // 16 = one block owns a whole CU (4 waves per SIMD); fewer when LDS is short

// (core128_store_offsets, the FAST epilogue's offset table, and fold64_doubles: fsst_launch_shape.hpp -- the host builds the tables)
// Rounding ties.  A displaced source lands in row round(k' + shift).  The float32 estimate of the shift carries an
// error of ~1e-7 (1 + |shift|) max|Z| / |V|: for a cell that is small against its frame's spectrum and moves tens of
// bins (Hann-, Blackman-, Kaiser(beta >> 1)-class windows) that is up to ~1e-2 bins, enough to put the cell into the
// neighbouring row of the float64 reference.  The kernel therefore carries an error bound with every displaced cell:
// with R^2 = 4 nwin max|c|^2 sum x^2 over the staged tile (Parseval: an upper bound of sum |Z|^2 of every frame of the tile,
// c = (w + i dw') / 2) the coordinate is good to about  tau = 1e-6 (1 + |shift|) R / |V|.  A displaced cell whose float32
// coordinate lies within tau of a half-integer is NOT moved on the spot: it goes to a per-wave queue in LDS (frame, bin,
// value) and, once the group's spectra are done and their registers free, the whole wave recomputes that one bin of V
// and Vd' by a float64 DFT of the frame (two taps per lane for nwin = 128, window and twiddle tables in float64 from
// HBM, a float64 butterfly sum) and rounds the float64 coordinate.  Cells below 1e-6 R are left to float32: they
// cannot change a feature by 1e-4 of the largest feature wherever they land.  Large cells have tau ~ 1e-6 and are
// practically never queued; the queue holds the small far-moving cells that float32 cannot place.
// No queues (rounds 1-2 queued such cells, 240 + 24 per group, and fell back to float32 beyond that: tonal and offset-
// dominated inputs under low-sidelobe windows overflowed them -- profiles/r02_adversarial_parity.txt class iii): an undecided
// cell sets ONE BIT of a per-group bitmap in LDS, bit 16 (k' & 1) + frame of word k' >> 1, k' = 0 .. nwin/2 - 1, so their number
// is not limited by anything and the bitmap is a sixth of the queues' size.  Resolution (resolve_bitmap): from kTieGroup64
// cells per 64 sources on, the whole group at once by the float64 fold + DFT factorisation (resolve_group_f64); below that, per
// set of 64 sources, up to kTieCoop cells one by one with the whole wave on one float64 DFT, more than that lane l takes source
// k' = l of the set and the wave walks the frames that have a bit set (one frame per round: its windowed samples are handed
// round by v_readlane).  The float32 V of a cell inside the stored cover of the own plane is read back from -- and cleared
// in -- its own column; for a cell outside it V is the float64 DFT's own result, rounded once.
constexpr int kTieCoop = 6;                  // up to this many undecided cells of a 64-source set the wave resolves one by one
constexpr float kTieMargin = 1.0f / 64.0f;   // the stay-in-row test hands |shift| > 1/2 - this to the rare path
constexpr float kTieErr2 = 1.0e-12f;         // (1e-6)^2: tau^2 = kTieErr2 (1 + |shift|)^2 R^2 / |V|^2  (4e-7 left 2 of 1000
                                             // random configurations 1.4-1.8x over the gate: tools/fuzz_parity.py 1000 3)
constexpr float kTieFloor2 = 1.0e-12f;       // (1e-6)^2: cells with |V|^2 below this times R^2 stay with float32.  R over-
                                             // estimates the frame's spectrum norm by up to ~5x and that norm is at most
                                             // sqrt(nwin) times the largest bin, so 1e-6 R is < 1e-4 of the largest feature
                                             // (1e-5 R was not: 3 of 2000 random narrow-band configurations failed the gate)

__device__ __forceinline__ void wave_sync()
{
    // LDS traffic of one wave is executed in program order: only the compiler must not reorder.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Moves a source k' -> row in a frame's displaced plane: the own plane holds V in the source's own column
// (unconditional store), so V is taken out again there, added at `row` and -- conjugated -- at the negative-frequency
// twin's row nwin - row (oracle/fsst_oracle.c step 6: two-sided cyclic scatter, one-sided rows kept).
// The odd wave of a PAIR (fsst_core128_kernel) does not add into the displaced plane while the even wave does: it LISTS its
// additions -- (cell, re, im) in program order, lanes in order (ballot prefix: no atomics) -- and the even wave replays the list
// behind its own additions: the plane receives every addition in the order of the one-wave kernel, whichever wave runs faster.
constexpr int kPairListCap = 256;
struct PairList {
    int* cell;            // [kPairListCap] float index into the displaced plane (re component; im = + 1)
    f2* val;              // [kPairListCap]
    int* cnt;             // (in LDS) additions listed; > kPairListCap: entries were dropped, the group is redone without the list
    int rowoff;           // this lane's frame row of the displaced plane, in cells
};
// COLS (K <= 24): flag[2..7] collect WHICH columns of the displaced plane were added to (a byte per column), so that the fold looks at
// those only; flag[0] says that there is something to fold, as without COLS.
template <int NWIN, bool LANE_OWNS = false, bool LIST = false, bool COLS = false>
__device__ __forceinline__ void move_source(f2* row_disp, int* flag, int klo, int K, int kpi, int row, f2 V,
                                            f2* own_cell = nullptr, bool stored = false, PairList* pl = nullptr)
{
    auto add = [&](int idx, float re, float im) {
        if constexpr (LIST) {
            // (the count lives in LDS: a variable updated under a divergent branch would be per-lane, stale in the lanes that
            //  did not take it; the first active lane reserves the slots of all of them)
            const unsigned long long m = __builtin_amdgcn_ballot_w64(true);      // the lanes that add here, in lane order
            const int below = static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u)));
            int base = 0;
            if (below == 0) base = __hip_atomic_fetch_add(pl->cnt, static_cast<int>(__builtin_popcountll(m)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int slot = __builtin_amdgcn_readfirstlane(base) + below;
            if (slot < kPairListCap) { pl->cell[slot] = 2 * (pl->rowoff + idx); pl->val[slot] = f2{re, im}; }
        } else {
            float* q = reinterpret_cast<float*>(row_disp + idx);
            __hip_atomic_fetch_add(q, re, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(q + 1, im, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    if (row == kpi) return;                             // rounds back into its own row after all
    if constexpr (COLS && LANE_OWNS && !LIST) if (klo >= 1 && klo + K <= NWIN / 2) {
        // a band inside rows 1 .. nwin/2 - 1 (the canonical-band kernels; row 0 is its own twin and keeps the general form below): a
        // destination is in the band, or -- only above nwin/2 -- its twin is; the twin's arithmetic is spent on the few sources that
        // wrap around row 0
        if (stored) *own_cell = f2{0.0f, 0.0f};
        const int idx = row - klo;
        unsigned char* colb = reinterpret_cast<unsigned char*>(flag + 2);     // one byte per column (K <= 24): plain stores, no atomic
        if (static_cast<unsigned>(idx) < static_cast<unsigned>(K)) {
            add(idx, V.x, V.y);
            colb[idx] = 1; *flag = 1;
        } else if (row > NWIN / 2 && kpi != 0) {
            const int idm = (NWIN - row) - klo;
            if (static_cast<unsigned>(idm) < static_cast<unsigned>(K)) {
                add(idm, V.x, -V.y);
                colb[idm] = 1; *flag = 1;
            }
        }
        return;
    }
    const int own = kpi - klo, idx = row - klo;
    const int idm = ((NWIN - row) & (NWIN - 1)) - klo;  // negative-frequency twin: row -> nwin - row, value conj
    const bool in_row = static_cast<unsigned>(idx) < static_cast<unsigned>(K);
    const bool in_twin = kpi != 0 && static_cast<unsigned>(idm) < static_cast<unsigned>(K);     // (k' = nwin/2 never moves)
    bool touched = in_row | in_twin;
    // taking V out of its own column: the lane that stored it a moment ago (LANE_OWNS; own_cell = its cell of the own
    // plane, `stored` = wave-uniform: the source's stripe lies inside the stored cover, outside it there is nothing to
    // take out) simply clears it; the float64 path, which runs later and for any lane's cell, subtracts it in the
    // displaced plane
    if constexpr (LANE_OWNS) {
        if (stored) *own_cell = f2{0.0f, 0.0f};
    } else if (static_cast<unsigned>(own) < static_cast<unsigned>(K)) {
        add(own, -V.x, -V.y);
        touched = true;
    }
    if (in_row) add(idx, V.x, V.y);
    if (in_twin) add(idm, V.x, -V.y);
    if constexpr (COLS) {                               // (bands that take the general form: row 0 inside the band)
        unsigned char* colb = reinterpret_cast<unsigned char*>(flag + 2);
        if (in_row) colb[idx] = 1;
        if (in_twin) colb[idm] = 1;
    }
    if (touched) *flag = 1;                             // this wave's displaced plane is no longer zero: ONE write
}

// The move for a plane that takes the displaced additions ITSELF (fsst_canon128.hpp, "One plane"; bands inside rows 1 .. nwin/2 - 1): the
// source's own cell has been cleared by whoever found it moving, V is added at `row` (its own row included: it "rounds back") or, for a
// source that wraps around row 0, conjugated at the twin's.  `row0` = this frame's row of the plane, indexed by spectrum row.
template <int NWIN>
__device__ __forceinline__ void acc_source(f2* row0, int klo, int K, int kpi, int row, f2 V)
{
    if (static_cast<unsigned>(row - klo) < static_cast<unsigned>(K)) {
        float* q = reinterpret_cast<float*>(row0 + row);
        __hip_atomic_fetch_add(q, V.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(q + 1, V.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else if (row > NWIN / 2 && kpi != 0) {
        const int idm = NWIN - row;                      // negative-frequency twin: row -> nwin - row, value conj
        if (static_cast<unsigned>(idm - klo) < static_cast<unsigned>(K)) {
            float* q = reinterpret_cast<float*>(row0 + idm);
            __hip_atomic_fetch_add(q, V.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(q + 1, -V.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// Rare path for a displaced source: oracle/fsst_oracle.c steps 4-6 in fp32, except for coordinates too close to a
// rounding tie, which are queued for resolve_ties().  `row_disp` points at this lane's frame row (frame j of the
// group) in the displaced plane.
template <int NWIN, int ERRMUL = 1, bool LIST = false>
__device__ __forceinline__ void displaced_source(f2* row_disp, int* flag, int* tq, int klo, int K, int kpi, int j,
                                                 float num, float den, f2 V, float R2, f2* own_cell, bool stored, PairList* pl = nullptr)
{
    float shift = num * __builtin_amdgcn_rcpf(den);
    if (!(fabsf(shift) <= 1.0e6f)) shift = 0.0f;        // NaN / inf / absurd -> 0 (fsst.m: ~isfinite)
    const float a = static_cast<float>(kpi) + shift;
    float fr = a - floorf(a) - 0.5f;
    const float s1 = 1.0f + fabsf(shift);
    // (opaque: otherwise the two independent product chains below are packed into v_pk_mul_f32 pairs whose operand
    //  shuffles and hazard nops cost more than the five plain multiplies)
    asm volatile("" : "+v"(fr));
    if (fr * fr * den < (kTieErr2 * ERRMUL) * s1 * s1 * R2 && den > kTieFloor2 * R2) {     // too close to call in float32
        __hip_atomic_fetch_or(reinterpret_cast<unsigned*>(tq) + (kpi >> 1), 1u << (((kpi & 1) << 4) + j), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        flag[1] = 1;
        return;
    }
    const float r = truncf(a + copysignf(0.5f, a));     // MATLAB round: half away from zero
    move_source<NWIN, true, LIST>(row_disp, flag, klo, K, kpi, static_cast<int>(r) & (NWIN - 1), V, own_cell, stored, pl);
}

// The whole wave, after the group's spectra: every undecided cell's bin of V and Vd' by a float64 DFT of its frame
// (sample(i) = sample i of the group's first frame as a double: the float32 signal itself; wtab[n] = {w, dw'}[n],
// twtab[m] = {cos, sin}(2 pi m / nwin), float64), the float64 coordinate k' - Im(Vd'/V) rounded half away from zero, then the
// move.  [cov0, cov1) = the sources whose float32 V sits in the own plane (leading dimension OLD): it is read back from --
// and cleared in -- its own column; a source outside the cover has no own cell and none in the band: its V is the float64
// DFT's, times the plane's sign (-1)^k' (even nwin: the modified-STFT phase) and `plane_scale` (1 unless the plane holds
// scaled values, fsst_canon128.hpp).
// REFRESH (the exact mode of a group, see "Exact groups" below): the own cell is first rewritten with the float64 value.
// ACC: the own plane takes the additions itself and holds nothing of an undecided source (its cell was cleared when it was found
// undecided: fsst_canon128.hpp, "One plane"): V is the float64 DFT's, rounded once, added where it belongs -- its own row included.
template <int NWIN, bool REFRESH = false, bool ACC = false>
__device__ __forceinline__ void resolve_one(f2* disp_base, int LDF, int* flag, int klo, int K, f2* own_base, int OLD, int cov0, int cov1,
                                            int kpi, int jf, double vr, double vi, double dr, double di, double plane_scale)
{
    const double den = vr * vr + vi * vi;
    double shift = (dr * vi - di * vr) / den;
    if (!(fabs(shift) <= 1.0e6)) shift = 0.0;           // V == 0 or absurd -> 0 (fsst.m: ~isfinite)
    const double a = static_cast<double>(kpi) + shift;
    const double r = (a >= 0.0) ? floor(a + 0.5) : -floor(0.5 - a);
    const int row = static_cast<int>(static_cast<long long>(r)) & (NWIN - 1);
    const double sg = (kpi & 1) ? -plane_scale : plane_scale;
    if constexpr (ACC) {
        acc_source<NWIN>(own_base + jf * OLD - cov0, klo, K, kpi, row, f2{static_cast<float>(vr * sg), static_cast<float>(vi * sg)});
        return;
    }
    if (kpi >= cov0 && kpi < cov1) {
        f2* cell = own_base + jf * OLD + (kpi - cov0);
        f2 V;
        if constexpr (REFRESH) { V = f2{static_cast<float>(vr * sg), static_cast<float>(vi * sg)}; *cell = V; }
        else V = *cell;
        move_source<NWIN, true>(disp_base + jf * LDF, flag, klo, K, kpi, row, V, cell, true);
    } else {
        const f2 V = {static_cast<float>(vr * sg), static_cast<float>(vi * sg)};
        move_source<NWIN, true>(disp_base + jf * LDF, flag, klo, K, kpi, row, V, nullptr, false);
    }
}

// Exact groups.  float32 resolves a feature to ~4e-7 of its FRAME's spectrum norm, whatever the feature's own size: when the kept
// band holds nothing but the far leakage of an out-of-band component (a tone or an offset 1e3 times the in-band content under
// a low-sidelobe window) that is more than 1e-4 of the band's largest feature (profiles/r02_adversarial_parity.txt, classes i
// and ii).  A group none of whose stored cells reaches kExactTheta R (R = the spectrum-norm bound of the group's own samples)
// is therefore redone in float64: REFRESH = true treats EVERY cell as undecided -- lane l takes source k' = l, walks all 16
// frames, rewrites the own cell with the float64 value, rounds the float64 coordinate, moves.  ~50x the cost of the group;
// ordinary signals never get there (white noise: largest cell 0.09 R).
constexpr float kExactTheta2 = 1.0e-4f;      // (1e-2)^2
__device__ __forceinline__ double readlane_f64(double v, int l)      // lane l's value in every lane (l wave-uniform)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(b), l));
    const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(b >> 32), l));
    return __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo));
}
// TWLDS: `twtab` points into LDS (the canonical-band kernels keep the 2 kB of twiddles beside their operand table).
using d2v = double __attribute__((ext_vector_type(2)));
using lds_d2v = __attribute__((address_space(3))) d2v;
template <bool TWLDS>
__device__ __forceinline__ d2v tie_twiddle(const double* twtab, int idx)
{
    if constexpr (TWLDS) return ((const lds_d2v*)reinterpret_cast<const d2v*>(twtab))[idx];
    else return reinterpret_cast<const d2v*>(twtab)[idx];
}
// Heavily undecided groups (an on-bin tone under a near-rectangular window, a band that holds only leakage: ~all of the group's
// 16 nwin / 2 (source, frame) cells).  One float64 DFT per cell is nwin taps x 4 FMAs; done for all cells it is the fold +
// NT-point DFT factorisation of the float32 kernel in float64 instead: per tap ONE chain of RQ / 4 v_mfma_f64_16x16x4_f64
// gives lane (g, j) the folded {Za, Zb}[tap] of its two classes for frame j (A operand: the float64 table a64 behind the
// twiddles of `wtab`, made by the host with the row order of the float64 instruction; B operand: the float32 samples, exact
// in float64), and the lane accumulates the NT-point DFT outputs of SPP stripes at a time (registers) -- X = Z[RQ s + r] and
// its conjugate partner, as process_stripe.  NT complex multiply-adds per cell instead of nwin real-complex ones.
// Measured at 128 points on an on-bin tone (every group): 22.8 -> 2.9 ms per 1024 windows, 1.0 of it the displaced cells
// themselves.  The fold is redone in every pass (64 cycles per float64 matrix instruction on this chip: ~40 % of the path at 128
// points); holding its NT x 4 doubles per lane would take 128 / 256 registers, two stripes per pass made the 128-register
// kernels spill (SPP = 1 there; the 256-register kernels of 256 / 512 points take 4 / 2), and making the A operand on the spot
// from the window pair and twiddles in LDS instead of loading it was slower (4.3 ms).
// XREG: the B operand's samples are fetched once into registers (the canonical-band kernels: sample() is a load from HBM / L2);
// otherwise sample() is called per tap (a read of the float32 tile in LDS).  sample(i): sample i of the group's first frame.
__device__ __forceinline__ d2v uniform_d2v(d2v v)
{
    auto u = [](double x) -> double {
        const long long b = __double_as_longlong(x);
        const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(b)));
        const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(b >> 32)));
        return __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo));
    };
    return d2v{u(v.x), u(v.y)};
}
using d4v = double __attribute__((ext_vector_type(4)));
template <int NT, int RQ, int SPP, bool XREG, bool REFRESH, bool TWLDS, class Sample>
__device__ __forceinline__ void resolve_group_f64(const unsigned* tb, Sample sample, f2* disp_base, int LDF, int* flag, int klo, int K,
                                                  f2* own_base, int OLD, int cov0, int cov1, const double* a64, const double* twtab,
                                                  double plane_scale, int lane)
{
    constexpr int NWIN = NT * RQ, NPASS = RQ / 8, KST = RQ / 4;
    static_assert((NT / 2) % SPP == 0, "whole passes");
    const int g = lane >> 4, j = lane & 15;
    float xs[XREG ? KST : 1][XREG ? NT : 1];             // B operand rows kk = g + 4 ks of every tap: x[j + n + NT kk]
    if constexpr (XREG) {
#pragma unroll
        for (int h = 0; h < KST; ++h)
#pragma unroll
            for (int n = 0; n < NT; ++n) xs[h][n] = static_cast<float>(sample(j + n + NT * (g + 4 * h)));
    }
    // this lane's flagged frames: bit (k' & 1) * 16 + j of word k' >> 1
    auto flagged = [&](int kp) -> bool { return REFRESH || ((tb[kp >> 1] >> (((kp & 1) << 4) + j)) & 1u) != 0u; };
    auto cmac = [](double& ar, double& ai, double zr, double zi, d2v cs) {      // a += z (cos - i sin)
        ar = fma(zr, cs.x, ar); ar = fma(zi, cs.y, ar);
        ai = fma(zi, cs.x, ai); ai = fma(-zr, cs.y, ai);
    };
#pragma unroll 1
    for (int pz = 0; pz < NPASS; ++pz) {
        const int pair = 4 * pz + g;
        const bool isg0 = pair == 0;                         // the self-conjugate classes {0, RQ / 2}
        const int rA = pair, rB = isg0 ? RQ / 2 : RQ - pair;
        const double* ap = a64 + pz * (NT * KST * 64);       // (uniform base + lane index: no per-lane 64-bit pointer to hold)
#pragma unroll 1
        for (int s0 = 0; s0 < NT / 2; s0 += SPP) {
            double xa[SPP][2], xb[SPP][2], pza[SPP][2], pzb[SPP][2];
#pragma unroll
            for (int u = 0; u < SPP; ++u) { xa[u][0] = xa[u][1] = xb[u][0] = xb[u][1] = pza[u][0] = pza[u][1] = pzb[u][0] = pzb[u][1] = 0.0; }
#pragma unroll 4
            for (int n = 0; n < NT; ++n) {
                d4v z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int ks = 0; ks < KST; ++ks) {
                    const double a = ap[(n * KST + ks) * 64 + lane];
                    double x;
                    if constexpr (XREG) x = static_cast<double>(xs[ks][n]);
                    else x = sample(j + n + NT * (g + 4 * ks));
                    z = __builtin_amdgcn_mfma_f64_16x16x4f64(a, x, z, 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < SPP; ++u) {
                    const int s = s0 + u;
                    const int ia = isg0 ? ((NT - s) & (NT - 1)) : NT - 1 - s;    // partner index in array a (process_stripe)
                    // (t1, t2 are the same in every lane: scalar registers -- eight vector registers the 128-register kernels lack)
                    const d2v t1 = uniform_d2v(tie_twiddle<TWLDS>(twtab, (RQ * s * n) & (NWIN - 1)));
                    const d2v t2 = uniform_d2v(tie_twiddle<TWLDS>(twtab, (RQ * (NT - 1 - s) * n) & (NWIN - 1)));
                    const d2v t3 = tie_twiddle<TWLDS>(twtab, (RQ * ia * n) & (NWIN - 1));
                    cmac(xa[u][0], xa[u][1], z.x, z.y, t1);
                    cmac(xb[u][0], xb[u][1], z.z, z.w, t1);
                    cmac(pzb[u][0], pzb[u][1], z.z, z.w, t2);
                    cmac(pza[u][0], pza[u][1], z.x, z.y, t3);
                }
            }
#pragma unroll
            for (int u = 0; u < SPP; ++u) {
                const int s = s0 + u;
                const double par = isg0 ? pza[u][0] : pzb[u][0], pai = isg0 ? pza[u][1] : pzb[u][1];      // partner of source a
                const double pbr = isg0 ? pzb[u][0] : pza[u][0], pbi = isg0 ? pzb[u][1] : pza[u][1];      // partner of source b
                const int ka = RQ * s + rA, kb = RQ * s + rB;
                // plane values (-1)^k' V = X + conj(P), (-1)^k' Vd' = (X - conj(P)) / i; resolve_one takes V, Vd' themselves
                const double sa = (ka & 1) ? -1.0 : 1.0, sb = (kb & 1) ? -1.0 : 1.0;
                if (flagged(ka))
                    resolve_one<NWIN, REFRESH>(disp_base, LDF, flag, klo, K, own_base, OLD, cov0, cov1, ka, j,
                                               sa * (xa[u][0] + par), sa * (xa[u][1] - pai), sa * (xa[u][1] + pai), sa * (par - xa[u][0]), plane_scale);
                if (flagged(kb))
                    resolve_one<NWIN, REFRESH>(disp_base, LDF, flag, klo, K, own_base, OLD, cov0, cov1, kb, j,
                                               sb * (xb[u][0] + pbr), sb * (xb[u][1] - pbi), sb * (xb[u][1] + pbi), sb * (pbr - xb[u][0]), plane_scale);
            }
        }
    }
}

// nwin = 128 (16 taps, radix 8, one stripe per pass, samples in registers): the same, written out for the 128-register kernels
// -- the general form above needs a few registers more than they have.
template <bool REFRESH, bool TWLDS, bool ACC = false, class Sample>
__device__ __forceinline__ void resolve_group_f64_128(const unsigned* tb, Sample sample, f2* disp_base, int LDF, int* flag, int klo, int K,
                                                  f2* own_base, int OLD, int cov0, int cov1, const double* a64, const double* twtab,
                                                  double plane_scale, int lane)
{
    constexpr int NWIN = 128, NT = 16, RQ = 8;
    const int g = lane >> 4, j = lane & 15;
    const bool isg0 = g == 0;
    const int rA = g, rB = isg0 ? RQ / 2 : RQ - g;
    float xs[2][NT];                                     // B operand rows kk = g and g + 4 of every tap: x[j + n + 16 kk]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int n = 0; n < NT; ++n) xs[h][n] = static_cast<float>(sample(j + n + 16 * (g + 4 * h)));
    // this lane's flagged frames: bit (k' & 1) * 16 + j of word k' >> 1
    auto flagged = [&](int kp) -> bool { return REFRESH || ((tb[kp >> 1] >> (((kp & 1) << 4) + j)) & 1u) != 0u; };
    auto cmac = [](double& ar, double& ai, double zr, double zi, d2v cs) {      // a += z (cos - i sin)
        ar = fma(zr, cs.x, ar); ar = fma(zi, cs.y, ar);
        ai = fma(zi, cs.x, ai); ai = fma(-zr, cs.y, ai);
    };
#pragma unroll 1
    for (int s = 0; s < NT / 2; ++s) {                   // (one stripe per pass: 16 accumulator registers; two made the 128-register kernels spill)
        double xa[2] = {0.0, 0.0}, xb[2] = {0.0, 0.0}, pza[2] = {0.0, 0.0}, pzb[2] = {0.0, 0.0};
        const int ia = isg0 ? ((NT - s) & (NT - 1)) : NT - 1 - s;                // partner index in array a (process_stripe)
#pragma unroll 2
        for (int n = 0; n < NT; ++n) {
            const double a0 = a64[(2 * n) * 64 + lane], a1 = a64[(2 * n + 1) * 64 + lane];
            d4v z = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, static_cast<double>(xs[0][n]), d4v{0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
            z = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, static_cast<double>(xs[1][n]), z, 0, 0, 0);
            // (t1, t2 are the same in every lane: scalar registers -- eight vector registers the 128-register kernels lack)
            const d2v t1 = uniform_d2v(tie_twiddle<TWLDS>(twtab, (RQ * s * n) & (NWIN - 1)));
            const d2v t2 = uniform_d2v(tie_twiddle<TWLDS>(twtab, (RQ * (NT - 1 - s) * n) & (NWIN - 1)));
            const d2v t3 = tie_twiddle<TWLDS>(twtab, (RQ * ia * n) & (NWIN - 1));
            cmac(xa[0], xa[1], z.x, z.y, t1);
            cmac(xb[0], xb[1], z.z, z.w, t1);
            cmac(pzb[0], pzb[1], z.z, z.w, t2);
            cmac(pza[0], pza[1], z.x, z.y, t3);
        }
        const double par = isg0 ? pza[0] : pzb[0], pai = isg0 ? pza[1] : pzb[1];      // partner of source a
        const double pbr = isg0 ? pzb[0] : pza[0], pbi = isg0 ? pzb[1] : pza[1];      // partner of source b
        const int ka = RQ * s + rA, kb = RQ * s + rB;
        // plane values (-1)^k' V = X + conj(P), (-1)^k' Vd' = (X - conj(P)) / i; resolve_one takes V, Vd' themselves
        const double sa = (ka & 1) ? -1.0 : 1.0, sb = (kb & 1) ? -1.0 : 1.0;
        if (flagged(ka))
            resolve_one<NWIN, REFRESH, ACC>(disp_base, LDF, flag, klo, K, own_base, OLD, cov0, cov1, ka, j,
                                       sa * (xa[0] + par), sa * (xa[1] - pai), sa * (xa[1] + pai), sa * (par - xa[0]), plane_scale);
        if (flagged(kb))
            resolve_one<NWIN, REFRESH, ACC>(disp_base, LDF, flag, klo, K, own_base, OLD, cov0, cov1, kb, j,
                                       sb * (xb[0] + pbr), sb * (xb[1] - pbi), sb * (xb[1] + pbi), sb * (pbr - xb[0]), plane_scale);
    }
}

constexpr int kTieGroup64 = 24;              // nwin = 128: from this many undecided cells on the group is redone by resolve_group_f64
template <int NWIN, bool REFRESH = false, bool TWLDS = false, bool ACC = false, class Sample>
__device__ __forceinline__ void resolve_bitmap(unsigned* tb, Sample sample, f2* disp_base, int LDF, int* flag, int klo, int K,
                                               f2* own_base, int OLD, int cov0, int cov1,
                                               const double* wtab, const double* twtab, double plane_scale, int lane_in)
{
    constexpr int NSETS = NWIN / 128;                   // sets of 32 words = 64 sources
    int lane = lane_in;                                 // opaque HERE, inside the rare branch: nothing this function derives
    asm volatile("" : "+v"(lane));                      // from the lane id is computed per chunk, held across the transform and spilled
    if constexpr (NWIN == 128 || NWIN == 256 || NWIN == 512) {
        // from kTieGroup64 undecided cells per 64 sources on (and for every exact group): the whole group in float64 at once
        int total = 0;
        if constexpr (!REFRESH) {
            int cnt = 0;
#pragma unroll
            for (int set = 0; set < NSETS; ++set) cnt += (lane < 32) ? __popc(tb[32 * set + lane]) : 0;
#pragma unroll
            for (int b = 0; b < 8; ++b) total += __builtin_popcountll(__builtin_amdgcn_ballot_w64((cnt >> b) & 1)) << b;
        }
        if (REFRESH || total >= kTieGroup64 * NSETS) {
            constexpr int NT = NWIN == 512 ? 32 : 16, RQ = NWIN / NT;
            constexpr int SPP = NWIN == 128 ? 1 : 4;
            if constexpr (NWIN == 128)
                resolve_group_f64_128<REFRESH, TWLDS, ACC>(tb, sample, disp_base, LDF, flag, klo, K, own_base, OLD, cov0, cov1, wtab + 4 * NWIN, twtab,
                                                      plane_scale, lane);
            else
                resolve_group_f64<NT, RQ, SPP, false, REFRESH, TWLDS>(tb, sample, disp_base, LDF, flag, klo, K, own_base, OLD, cov0, cov1,
                                                                     wtab + 4 * NWIN, twtab, plane_scale, lane);
            for (int i = lane; i < 32 * NSETS; i += 64) tb[i] = 0u;
            if constexpr (REFRESH) {
                if (cov1 > NWIN / 2 && lane < 16) {          // the Nyquist row (see below)
                    double vr = 0.0;
#pragma unroll 1
                    for (int n = 0; n < NWIN; ++n) {
                        const double xw = sample(lane + n) * wtab[2 * n];
                        vr = (n & 1) ? vr - xw : vr + xw;
                    }
                    own_base[lane * OLD + (NWIN / 2 - cov0)] = f2{static_cast<float>(vr * plane_scale), 0.0f};
                }
            }
            if (lane == 0) flag[1] = 0;
            return;
        }
    }
#pragma unroll 1
    for (int set = 0; set < NSETS; ++set) {
        unsigned* tbs = tb + 32 * set;
        const int k0 = 64 * set;
        unsigned w = (lane < 32) ? tbs[lane] : 0u;
        const int cnt = __popc(w);                       // <= 32 per lane: the wave's total from six ballots (scalar unit only)
        int total = 0;
#pragma unroll
        for (int b = 0; b < 6; ++b) total += __builtin_popcountll(__builtin_amdgcn_ballot_w64((cnt >> b) & 1)) << b;
        if constexpr (REFRESH) total = 1024;
        if (total == 0) continue;
        if (total <= kTieCoop) {
            // few cells: one by one, all lanes on one cell (NWIN / 64 taps per lane, float64 butterfly sum)
            for (int it = 0; it < total; ++it) {
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(w != 0u);
                const int l0 = __builtin_ctzll(mask);
                const unsigned ww = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(w), l0));
                const int bit = __builtin_ctz(ww);
                if (lane == l0) w &= w - 1u;
                const int kpi = k0 + 2 * l0 + (bit >> 4), jf = bit & 15;
                double vr = 0.0, vi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll 1
                for (int n = lane; n < NWIN; n += 64) {
                    const double x = sample(jf + n);
                    const double2 wd = reinterpret_cast<const double2*>(wtab)[n];
                    const d2v cs = tie_twiddle<TWLDS>(twtab, (kpi * n) & (NWIN - 1));
                    const double xw = x * wd.x, xd = x * wd.y;
                    vr = fma(xw, cs.x, vr); vi = fma(-xw, cs.y, vi);
                    dr = fma(xd, cs.x, dr); di = fma(-xd, cs.y, di);
                }
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    vr += shfl_xor_f64(vr, off, lane); vi += shfl_xor_f64(vi, off, lane);
                    dr += shfl_xor_f64(dr, off, lane); di += shfl_xor_f64(di, off, lane);
                }
                if (lane == 0) resolve_one<NWIN, false, ACC>(disp_base, LDF, flag, klo, K, own_base, OLD, cov0, cov1, kpi, jf, vr, vi, dr, di, plane_scale);
            }
        } else {
            // many cells (tonal or offset-dominated signals under low-sidelobe windows): lane l owns source k' = k0 + l, and
            // the wave walks the FRAMES that have a bit set in some lane.  One frame per round: its windowed samples x w,
            // x dw' are the same for every source, so each lane computes NWIN / 64 of them (coalesced loads) and the round
            // hands them round through v_readlane; per tap a lane then loads only its twiddle (the 16 nwin byte table, L1 /
            // L2).  Same products, same order of additions as the one-by-one branch above.  (The first version let every
            // lane walk its own frames -- three dependent-latency loads per tap and lane: 730 cycles per tap, 23 ms per
            // 1024 windows of an on-bin tone; profiles/r03_input_cost.txt.)
            const unsigned hw = REFRESH ? 0xffffu : (tbs[lane >> 1] >> ((lane & 1) << 4)) & 0xffffu;
            const int kpi = k0 + lane;
            unsigned fm = 0u;                                    // frames with work (wave-uniform)
#pragma unroll
            for (int b = 0; b < 16; ++b) fm |= (__builtin_amdgcn_ballot_w64((hw >> b) & 1u) != 0ull ? 1u : 0u) << b;
            while (fm != 0u) {
                const int jf = __builtin_ctz(fm);
                fm &= fm - 1u;
                constexpr int TPL = NWIN / 64;                   // taps per lane
                double xw[TPL], xd[TPL];
#pragma unroll
                for (int t = 0; t < TPL; ++t) {
                    const int n = lane + 64 * t;
                    const double x = sample(jf + n);
                    const double2 wd = reinterpret_cast<const double2*>(wtab)[n];
                    xw[t] = x * wd.x; xd[t] = x * wd.y;
                }
                double vr = 0.0, vi = 0.0, dr = 0.0, di = 0.0;
#pragma unroll
                for (int t = 0; t < TPL; ++t) {
#pragma unroll 8
                    for (int l = 0; l < 64; ++l) {
                        const int n = 64 * t + l;
                        const double a = readlane_f64(xw[t], l), b = readlane_f64(xd[t], l);
                        const d2v cs = tie_twiddle<TWLDS>(twtab, (kpi * n) & (NWIN - 1));
                        vr = fma(a, cs.x, vr); vi = fma(-a, cs.y, vi);
                        dr = fma(b, cs.x, dr); di = fma(-b, cs.y, di);
                    }
                }
                if ((hw >> jf) & 1u) resolve_one<NWIN, REFRESH, ACC>(disp_base, LDF, flag, klo, K, own_base, OLD, cov0, cov1, kpi, jf, vr, vi, dr, di, plane_scale);
            }
        }
        if (lane < 32) tbs[lane] = 0u;
    }
    if constexpr (REFRESH) {
        // the Nyquist row (its own partner, never moves: V = sum x w (-1)^n is real) when the stored cover holds it
        if (cov1 > NWIN / 2 && lane < 16) {
            double vr = 0.0;
#pragma unroll 1
            for (int n = 0; n < NWIN; ++n) {
                const double xw = sample(lane + n) * wtab[2 * n];
                vr = (n & 1) ? vr - xw : vr + xw;
            }
            own_base[lane * OLD + (NWIN / 2 - cov0)] = f2{static_cast<float>(vr * plane_scale), 0.0f};
        }
    }
    if (lane == 0) flag[1] = 0;
}
template <int NWIN>
__device__ __forceinline__ void resolve_ties(int* tq, const float* xg, f2* disp_base, int LDF, int* flag, int klo, int K,
                                             f2* own_base, int OLD, int cov0, int cov1,
                                             const double* wtab, const double* twtab, int lane)
{
    resolve_bitmap<NWIN>(reinterpret_cast<unsigned*>(tq), [xg](int i) -> double { return static_cast<double>(xg[i]); }, disp_base, LDF, flag,
                         klo, K, own_base, OLD, cov0, cov1, wtab, twtab, 1.0, lane);
}

// One one-sided source bin k' held as packed spectrum value X = Z[k'] with conjugate partner
// P = Z[128 - k'] (Z = FFT of x (w + i dw') / 2 with the sign (-1)^k' folded into the constants):
//   V = X + conj(P) = (-1)^k' V[k'],   Vd' = (X - conj(P)) / i,   shift = -Im(Vd'/V) = num / den.
// The source stays in its own row iff |shift| < 1/2 iff |num| < den/2 (no division); den carries +1e-37
// so that V == 0 (which contributes nothing wherever it lands) never takes the rare path.  V is stored
// unconditionally into the source's own column; only when some lane of the wave has a displaced cell does
// the wave run the exact rounding path for it.  (Folding the 1/2 into the constants by doubling dw' saves
// one more multiply per source, 1 % of the kernel, but doubles the cancellation error of V for far-moving
// cells: measured 5 instead of 3 rounding flips per 918 k robust Hann columns, so it is not done.)
// The two sources of one stripe (classes a and b of this lane) with ONE rare-path branch for both (a branch per
// source -- v_cmp + s_and_saveexec + s_cbranch + s_or each -- measured 1.8 % slower; one branch per two stripes: no
// further gain).
template <int S, int RQ, int NWIN, bool LIST = false>
__device__ __forceinline__ void process_stripe(f2 XA, f2 PA, f2 XB, f2 PB, f2 tiny, f2* ownA, f2* ownB, bool store,
                                               f2* row_disp, int* flag, int* tq, int j, int klo, int K, int rA, int rB, float R2, float& mx,
                                               PairList* pl = nullptr)
{
    const f2 a1 = mix_re(XA, PA), a2 = mix_im(XA, PA);
    const f2 b1 = mix_re(XB, PB), b2 = mix_im(XB, PB);
    const f2 dna = dn_second(a2, dn_first(a1, tiny)), dnb = dn_second(b2, dn_first(b1, tiny));
    if (store) {                                        // wave-uniform predicate
        float* qa = reinterpret_cast<float*>(ownA);
        float* qb = reinterpret_cast<float*>(ownB);
        qa[0] = a1.x; qa[1] = a2.x;
        qb[0] = b1.x; qb[1] = b2.x;
        // largest |V|^2 among the stored cells ("Exact groups"); in the cover's FIRST stripe only rows of the band count:
        // an offset (row 0 and its main lobe) sits there, below the band, and is exactly what must not pass for content
        if (RQ * S <= klo) mx = fmaxf(mx, fmaxf(rA + RQ * S >= klo ? dna.x : 0.0f, rB + RQ * S >= klo ? dnb.x : 0.0f));
        else mx = fmaxf(mx, fmaxf(dna.x, dnb.x));
    }
    // (the threshold sits kTieMargin below 1/2 so that a cell whose |shift| is within the margin of 1/2 -- a rounding
    //  tie as well -- reaches the rare path and its float64 decision)
    constexpr float kStay = 0.5f - kTieMargin;
    const bool ma = fabsf(dna.y) >= kStay * dna.x, mb = fabsf(dnb.y) >= kStay * dnb.x;
    if (ma | mb) {                                      // skipped when no lane moved (execz)
        if (ma) displaced_source<NWIN, 1, LIST>(row_disp, flag, tq, klo, K, rA + RQ * S, j, dna.y, dna.x, f2{a1.x, a2.x}, R2, ownA, store, pl);
        if (mb) displaced_source<NWIN, 1, LIST>(row_disp, flag, tq, klo, K, rB + RQ * S, j, dnb.y, dnb.x, f2{b1.x, b2.x}, R2, ownB, store, pl);
    }
}

using gu32 = __attribute__((address_space(1))) unsigned;
constexpr unsigned kSpinLimit = 1u << 18;          // polls before a wait gives up (a poll takes ~0.1 us: ~30 ms; a healthy
                                                   // wait is microseconds).  After the first give-up of a block its other
                                                   // waits give up at once (LDS word `dead`), so a broken launch ends fast

}  // namespace hssfsst
