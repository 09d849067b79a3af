// fsst_tables.hpp -- the constant tables of a plan, made on the host in float64.  No HIP call and no plan here: a builder takes (window, dwb,
// nwin, ...) and returns one host table in the layout its kernel reads (the comments are the kernels' operand formats).  Included behind the kernel
// headers, whose layout constants it uses.  The order of the float64 operations is part of the results (tests/golden/ was made from these bytes).
#pragma once

#include <cmath>
#include <cstring>
#include <vector>

namespace hssfsst::tables {

// Knot slopes of the not-a-knot cubic spline through (1..n, w): the derivative window of
// ssq.fsst's instantaneous-frequency estimator before its fs/(2*pi) scaling (MATLAB fsst.m, local
// function dtwin).  Tridiagonal system (unit spacing):
//     s0 + 2 s1 = (5 d0 + d1)/2;  s_{i-1} + 4 s_i + s_{i+1} = 3 (w_{i+1} - w_{i-1});
//     2 s_{n-2} + s_{n-1} = (5 d_{n-2} + d_{n-3})/2,            d_i = w_{i+1} - w_i
// solved by Gaussian elimination with partial pivoting specialised to tridiagonal matrices
// (second super-diagonal as fill-in), O(n).
inline int spline_knot_slopes(const double* w, int n, double* s)
{
    if (n < 1) return HSSFSST_EINVAL;
    if (n == 1) { s[0] = 0.0; return 0; }
    if (n == 2) { s[0] = s[1] = w[1] - w[0]; return 0; }
    if (n == 3) {
        const double d0 = w[1] - w[0], d1 = w[2] - w[1];
        s[0] = d0 - 0.5 * (d1 - d0); s[1] = 0.5 * (d0 + d1); s[2] = d1 + 0.5 * (d1 - d0);
        return 0;
    }
    std::vector<double> dl(n, 0.0), d(n, 0.0), du(n, 0.0), du2(n, 0.0), b(n, 0.0);
    d[0] = 1.0; du[0] = 2.0; b[0] = (5.0 * (w[1] - w[0]) + (w[2] - w[1])) / 2.0;
    for (int i = 1; i < n - 1; ++i) {
        dl[i] = 1.0; d[i] = 4.0; du[i] = 1.0; b[i] = 3.0 * (w[i + 1] - w[i - 1]);
    }
    dl[n - 1] = 2.0; d[n - 1] = 1.0;
    b[n - 1] = (5.0 * (w[n - 1] - w[n - 2]) + (w[n - 2] - w[n - 3])) / 2.0;
    for (int i = 0; i < n - 1; ++i) {            // row i+1 has sub-diagonal dl[i+1]
        if (std::fabs(d[i]) >= std::fabs(dl[i + 1])) {
            if (d[i] == 0.0) return HSSFSST_EINVAL;
            const double f = dl[i + 1] / d[i];
            d[i + 1] -= f * du[i];
            if (i + 2 < n) du[i + 1] -= f * du2[i];
            b[i + 1] -= f * b[i];
        } else {                                 // swap rows i and i+1
            const double f = d[i] / dl[i + 1];
            const double di = dl[i + 1], dui = d[i + 1], du2i = (i + 2 < n) ? du[i + 1] : 0.0;
            const double bi = b[i + 1];
            d[i + 1] = du[i] - f * dui;
            if (i + 2 < n) du[i + 1] = du2[i] - f * du2i;
            b[i + 1] = b[i] - f * bi;
            d[i] = di; du[i] = dui; du2[i] = du2i; b[i] = bi;
        }
    }
    if (d[n - 1] == 0.0) return HSSFSST_EINVAL;
    s[n - 1] = b[n - 1] / d[n - 1];
    s[n - 2] = (b[n - 2] - du[n - 2] * s[n - 1]) / d[n - 2];
    for (int i = n - 3; i >= 0; --i) s[i] = (b[i] - du[i] * s[i + 1] - du2[i] * s[i + 2]) / d[i];
    return 0;
}

// the derivative window, slope * scale: scale = fs / (2 pi) is ssq.fsst's; the kernels take it in BIN units, dw * nwin / fs, scale = nwin / (2 pi)
inline int dwindow(const double* window, int nwin, double scale, double* dw)
{
    if (int rc = spline_knot_slopes(window, nwin, dw)) return rc;
    for (int i = 0; i < nwin; ++i) dw[i] *= scale;
    return 0;
}

// FSST._truncate_frequencies (synchrosqueeze.py:91-111): f is a float32 tensor (:52) compared
// with the Python bounds in float32, both inclusive; f_k = k*fs/nwin, Nyquist row = fs/2.
inline void band_rows(int nwin, double fs, double f_lo, double f_hi, int* klo, int* K)
{
    const int nf = nwin / 2 + 1;
    const double res = fs / static_cast<double>(nwin);
    int first = -1, cnt = 0;
    for (int k = 0; k < nf; ++k) {
        double fk = res * k;
        if ((nwin % 2) == 0 && k == nwin / 2) fk = fs / 2.0;
        const float f32 = static_cast<float>(fk);
        if (f32 >= static_cast<float>(f_lo) && f32 <= static_cast<float>(f_hi)) {
            if (first < 0) first = k;
            ++cnt;
        }
    }
    *klo = first < 0 ? 0 : first;
    *K = cnt;
}

// the MFMA kernels' window lengths and their taps (per-lane FFT size); the first-stage radix is nwin / taps
using hssfsst::mfma_length;          // (fsst_launch_shape.hpp)
using hssfsst::mfma_taps;

// The fold constant of a window split as nwin = NT taps x RQ fold terms (the first stage of every radix kernel):
//   C_r[n, q] = (w + i dw')[n + NT q] * exp(-2 pi i (r q / RQ + r n / nwin)),   class r, tap n, fold term q,
// stated once, as its four real products: C_r = (wc - ds) + i (ws + dc).  The tables are layouts of it: scaling (+-0.5, exact), type, order.
struct Fold {
    const double *window, *dwb;
    int nwin, NT, RQ;
    struct Products { double wc, ws, dc, ds; };          // w cos, w sin, dw' cos, dw' sin
    Products at(int r, int n, int q) const
    {
        const double ang = -2.0 * M_PI * (static_cast<double>(r) * q / RQ + static_cast<double>(r) * n / nwin);
        const double c = std::cos(ang), s = std::sin(ang), wv = window[n + NT * q], dv = dwb[n + NT * q];
        return {wv * c, wv * s, dv * c, dv * s};
    }
    // class pair m of the MFMA operands holds the classes ca = m, cb = (m ? RQ - m : RQ / 2) as sub = {ca re, ca im, cb re, cb im}
    int cls(int m, int sub) const { return sub < 2 ? m : (m ? RQ - m : RQ / 2); }
    double component(int m, int sub, int n, int q) const        // ... of (-1)^r 0.5 C_r[n, q]
    {
        const Products p = at(cls(m, sub), n, q);
        return ((cls(m, sub) & 1) ? -0.5 : 0.5) * ((sub & 1) ? p.ws + p.dc : p.wc - p.ds);
    }
};

// Generic kernels (fsst_kernels.hpp): class-folded scalar tables [class r <= R / 2][32 taps][4 R], R = nwin / 32.  The self-paired
// classes (r = 0, R / 2) hold 0.5 C_r as {re[R] | im[R]}, the others {w cos | w sin | dw' cos | dw' sin}[R].  Only the radix
// kernels read it: a plan of the any-length kernel carries the zero table of R = 2.
inline std::vector<float> generic_table(const double* window, const double* dwb, int nwin, bool radix)
{
    const int R = radix ? nwin / 32 : 2, ncls = R / 2 + 1;
    std::vector<float> tab(static_cast<size_t>(ncls) * 32 * 4 * R, 0.0f);
    const Fold f{window, dwb, nwin, 32, R};
    for (int r = 0; radix && r < ncls; ++r) {
        const bool packed = (r == 0) || (2 * r == R);
        for (int n = 0; n < 32; ++n) {
            float* row = tab.data() + (static_cast<size_t>(r) * 32 + n) * 4 * R;
            for (int q = 0; q < R; ++q) {
                const Fold::Products p = f.at(r, n, q);
                if (packed) {            // 0.5 (w + i dw') * phase
                    row[q] = static_cast<float>(0.5 * (p.wc - p.ds)); row[R + q] = static_cast<float>(0.5 * (p.ws + p.dc));
                } else {                 // w * phase | dw' * phase
                    row[q] = static_cast<float>(p.wc); row[R + q] = static_cast<float>(p.ws);
                    row[2 * R + q] = static_cast<float>(p.dc); row[3 * R + q] = static_cast<float>(p.ds);
                }
            }
        }
    }
    return tab;
}

// float64 tables of the rounding-tie path: the window pair {w, dw'}[nwin], then the twiddles {cos, sin}(2 pi m / nwin)[nwin].
// nwin 128 / 256 / 512 (whichever kernel the plan ends up with): behind them the A operand of the fold for heavily undecided
// groups of the MFMA kernels (resolve_group_f64, fsst_mfma128.hpp) -- the constants of mfma_table below, [pass][tap][k-step][lane],
// in float64 for v_mfma_f64_16x16x4_f64 (16 / 64 / 128 kB).  The float64 instruction hands lane group g the rows g, g + 4, g + 8,
// g + 12 of D (measured: tools/mfma_f64_layout.hip) where the float32 one hands it rows 4 g .. 4 g + 3: row i of A is class pair
// 4 pz + (i & 3), component i >> 2.  *r2scale = 4 nwin max |(w + i dw') / 2|^2, the error-bound scale of that path.
inline std::vector<double> tie_table(const double* window, const double* dwb, int nwin, float* r2scale)
{
    std::vector<double> wt(static_cast<size_t>(4) * nwin);
    double cmax2 = 0.0;
    for (int i = 0; i < nwin; ++i) cmax2 = std::fmax(cmax2, 0.25 * (window[i] * window[i] + dwb[i] * dwb[i]));
    *r2scale = static_cast<float>(4.0 * nwin * cmax2);
    for (int i = 0; i < nwin; ++i) {
        wt[2 * i] = window[i]; wt[2 * i + 1] = dwb[i];
        const double ang = 2.0 * M_PI * static_cast<double>(i) / static_cast<double>(nwin);
        wt[2 * nwin + 2 * i] = std::cos(ang); wt[2 * nwin + 2 * i + 1] = std::sin(ang);
    }
    if (!mfma_length(nwin)) return wt;
    const int nt = mfma_taps(nwin), rq = nwin / nt, npass = rq / 8, kst = rq / 4;
    const Fold f{window, dwb, nwin, nt, rq};
    wt.resize(static_cast<size_t>(4) * nwin + static_cast<size_t>(fold64_doubles(rq, nt)));
    double* f64 = wt.data() + static_cast<size_t>(4) * nwin;
    for (int pz = 0; pz < npass; ++pz)
        for (int n = 0; n < nt; ++n)
            for (int ks = 0; ks < kst; ++ks)
                for (int l = 0; l < 64; ++l) {
                    const int i = l & 15, q = (l >> 4) + 4 * ks;
                    f64[(((pz * nt + n) * kst) + ks) * 64 + l] = f.component(4 * pz + (i & 3), i >> 2, n, q);
                }
    return wt;
}

// Any-length kernel (fsst_dft.hpp): A operand [source block][k-step][64 lanes].
// A[i][k] of v_mfma_f32_16x16x4_f32 for source block blk, k-step ks: lane l holds row i = l & 15, k = l >> 4.
// Row i: source k' = 4 blk + (i >> 2), component i & 3 of {V.re, V.im, Vd'.re, Vd'.im}; tap n = 4 ks + k:
//   V  [k'] = sum_n x[t + n] w  [n] e^{-2 pi i k' (n + m) / N},  m = floor(N / 2) (the modified-STFT phase, step 5)
//   Vd'[k'] = sum_n x[t + n] dw'[n] e^{-2 pi i k' (n + m) / N}
// (k' (n + m) is reduced modulo N in integers before the angle is formed)
inline std::vector<float> dft_table(const double* window, const double* dwb, int nwin)
{
    const int nf = nwin / 2 + 1, nk4 = (nwin + 3) / 4, nblk4 = (nf + 3) / 4, m = nwin / 2;
    std::vector<float> dt(static_cast<size_t>(nblk4) * nk4 * 64, 0.0f);
    for (int blk = 0; blk < nblk4; ++blk)
        for (int ks = 0; ks < nk4; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int i = l & 15, n = 4 * ks + (l >> 4), kp = 4 * blk + (i >> 2), sub = i & 3;
                if (kp >= nf || n >= nwin) continue;
                const long long red = (static_cast<long long>(kp) * (n + m)) % nwin;
                const double ang = -2.0 * M_PI * static_cast<double>(red) / static_cast<double>(nwin);
                const double amp = (sub < 2) ? window[n] : dwb[n];
                dt[(static_cast<size_t>(blk) * nk4 + ks) * 64 + l] = static_cast<float>(amp * ((sub & 1) ? std::sin(ang) : std::cos(ang)));
            }
    return dt;
}

// MFMA kernels (fsst_mfma128.hpp), nwin = nt x rq: the float32 A operand, then the FAST epilogue's store offsets (ints).
// A[i][k] of v_mfma_f32_16x16x4_f32 for pass pz, tap n, k-step ks: lane l holds row i = l & 15, k = l >> 4.
// Row i: lane group gg = i >> 2 owns class pair m = 4 pz + gg, sub = i & 3.  Entry = Fold::component, q = k + 4 ks.
inline std::vector<float> mfma_table(const double* window, const double* dwb, int nwin, int klo, int K)
{
    const int nt = mfma_taps(nwin), rq = nwin / nt, npass = rq / 8, kst = rq / 4, atab_floats = core128_atab_floats(rq, nt);
    const Fold f{window, dwb, nwin, nt, rq};
    std::vector<float> at(atab_floats + 6 * 64);
    for (int pz = 0; pz < npass; ++pz)
        for (int n = 0; n < nt; ++n)
            for (int ks = 0; ks < kst; ++ks)
                for (int l = 0; l < 64; ++l) {
                    const int i = l & 15, q = (l >> 4) + 4 * ks;
                    // [pass][tap][lane][k-step]: the kernel's LDS layout
                    at[((pz * nt + n) * 64 + l) * kst + ks] = static_cast<float>(f.component(4 * pz + (i >> 2), i & 3, n, q));
                }
    static_assert(sizeof(int) == sizeof(float), "offset table shares the float buffer");
    int offs[6 * 64];
    core128_store_offsets(klo, K > 0 ? K : 2, offs, rq);
    std::memcpy(at.data() + atab_floats, offs, sizeof(offs));
    return at;
}

// fsst_canon128.hpp "Offsets": what a frame of ones contributes to the spectra the source stage starts from.
//   Zc[k] = (-1)^k 0.5 sum_{m inside the signal} (w + i dw')[m] e^{-2 pi i k m / 128}  (x cs: plane units),
// lane group g holds the classes g and (g ? 8 - g : 4): za[s] = Z[8 s + g], zb[s] = Z[8 s + (g ? 8 - g : 4)], s = 0..15.
// Frame 0 = interior (every m), 1 + t = the frame of output column t < 64 (m >= 64 - t), 65 + r = the frame r < 63 samples
// before the end (m <= r + 64).  Layout (fsst_canon128.hpp kCanonZcFloats): interior [g][za[0..15] | zb[0..15] | -];
// left edge [g][entry][t]; right edge [g][entry][r], r = 63 .. 79 = the interior once more
inline void canon_offset_spectra(const double* window, const double* dwb, double cs, float* zc /* [kCanonZcFloats], zeroed */)
{
    float* zleft = zc + kCanonYcFrame;
    float* zright = zleft + 4 * 32 * 64 * 2;
    for (int fr = 0; fr < 1 + 64 + 63; ++fr) {
        const int m0 = (fr >= 1 && fr <= 64) ? 64 - (fr - 1) : 0;
        const int m1 = (fr >= 65) ? (fr - 65) + 64 : 127;
        double zr[128], zi[128];
        for (int k = 0; k < 128; ++k) {
            double re = 0.0, im = 0.0;
            for (int m = m0; m <= m1; ++m) {
                const double ang = -2.0 * M_PI * static_cast<double>((k * m) % 128) / 128.0;
                const double c = std::cos(ang), sn = std::sin(ang);
                re += window[m] * c - dwb[m] * sn;
                im += window[m] * sn + dwb[m] * c;
            }
            const double sg = (k & 1) ? -0.5 : 0.5;
            zr[k] = sg * re * cs; zi[k] = sg * im * cs;
        }
        for (int gg = 0; gg < 4; ++gg)
            for (int s16 = 0; s16 < 16; ++s16) {
                const int ks[2] = {8 * s16 + gg, 8 * s16 + (gg ? 8 - gg : 4)};       // the lane group's two classes: za[s], zb[s]
                for (int ab = 0; ab < 2; ++ab) {
                    const int ent = ab * 16 + s16;
                    const float vr = static_cast<float>(zr[ks[ab]]), vi = static_cast<float>(zi[ks[ab]]);
                    auto put = [&](float* e) { e[0] = vr; e[1] = vi; };
                    if (fr == 0) {
                        put(zc + (gg * kCanonYcGroup + ent) * 2);
                        for (int r = 63; r < kCanonYcRight; ++r) put(zright + ((gg * 32 + ent) * kCanonYcRight + r) * 2);
                    } else if (fr <= 64) put(zleft + ((gg * 32 + ent) * 64 + (fr - 1)) * 2);
                    else put(zright + ((gg * 32 + ent) * kCanonYcRight + (fr - 65)) * 2);
                }
            }
    }
}

// Canonical-band kernels (fsst_canon128.hpp), nwin = 128 = 16 taps x 8: the constants of mfma_table as pairs of halves c1 + c2,
// scaled by 2^sc into [2^13, 2^14), [16 taps][64 lanes][8 halves]; the float64 twiddles of the rounding-tie path (2 kB: the
// kernels copy the whole table into LDS); the offset spectra above.  Entry (tap n, lane l = (kk, row i), half h): fold term
// q = kk + 4 (h >> 2), c1 for even h, c2 for odd h (products x1 c1, x1 c2, x2 c1, x2 c2 against the sample record {x1, x1, x2, x2}).
// *sc: the scale's exponent (the kernels undo it with 2^-sc; it comes from the same components that are split here).
inline std::vector<float> canon_table(const double* window, const double* dwb, int* sc)
{
    const Fold f{window, dwb, 128, 16, 8};
    auto comp = [&](int n, int i, int q) { return f.component(i >> 2, i & 3, n, q); };
    double cmax = 0.0;
    for (int n = 0; n < 16; ++n) for (int i = 0; i < 16; ++i) for (int q = 0; q < 8; ++q) cmax = std::fmax(cmax, std::fabs(comp(n, i, q)));
    int ex = 0;
    if (cmax > 0.0 && std::isfinite(cmax)) (void)std::frexp(cmax, &ex);          // cmax = f 2^ex, f in [0.5, 1)
    *sc = 14 - ex;                                                                // cmax 2^sc in [2^13, 2^14)
    const double cs = std::ldexp(1.0, *sc);
    static_assert(kCanonAtabFloats == 16 * 64 * 4 + 4 * 128, "f16 operand table + 128 {cos, sin} doubles");
    std::vector<float> t16(static_cast<size_t>(kCanonAtabFloats) + kCanonZcFloats, 0.0f);
    unsigned short* ht = reinterpret_cast<unsigned short*>(t16.data());
    for (int i = 0; i < 128; ++i) {
        const double ang = 2.0 * M_PI * static_cast<double>(i) / 128.0;
        const double cs2[2] = {std::cos(ang), std::sin(ang)};
        std::memcpy(ht + static_cast<size_t>(16) * 64 * 8 + static_cast<size_t>(i) * 8, cs2, sizeof(cs2));
    }
    for (int n = 0; n < 16; ++n)
        for (int l = 0; l < 64; ++l)
            for (int h = 0; h < 8; ++h) {
                const int i = l & 15, kk = l >> 4, q = kk + 4 * (h >> 2);
                const double v = comp(n, i, q) * cs;
                const _Float16 c1 = static_cast<_Float16>(v);
                const _Float16 c2 = static_cast<_Float16>(v - static_cast<double>(c1));
                const _Float16 pick = (h & 1) ? c2 : c1;
                std::memcpy(ht + (static_cast<size_t>(n) * 64 + l) * 8 + h, &pick, sizeof(pick));
            }
    canon_offset_spectra(window, dwb, cs, t16.data() + kCanonAtabFloats);
    return t16;
}

}  // namespace hssfsst::tables
