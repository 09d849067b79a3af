// fourier_resample_layout.hpp -- what the device resampler (fourier_resample_gpu.hpp, fourier_resample_ragged.hpp) makes on the
// host: the Bluestein tables of a plan, the chunk rule of the dense large tier and the plan of a ragged call.
// No HIP call and no plan here: lengths in, tables out, so all of it also compiles into a stand-alone program (tests/native/).
//
// A ragged call: the list by length (a class of equal M1 is a contiguous run, equal lengths adjacent, ties in list order), cut
// into chunks of at most `budget` elements of work and tables (at least one signal each).  Work layout of a chunk: signal d at
// work + d * Mw, Mw = max(M2, the chunk's largest M1), then one B1 / M1 table per distinct length of the chunk, back to back.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <new>
#include <numeric>
#include <vector>

#include "fourier_resample.hpp"

namespace hssfsst {

struct RaggedResampleSig {
    long long start;                 // first sample in x
    long long n;                     // samples
    long long M1;                    // forward convolution length (power of two >= 2n - 1)
    long long tab;                   // offset (double2) of its B1 / M1 table in the chunk's table region
    long long row;                   // output row (its index in the caller's list)
};

namespace rslayout {

constexpr size_t kRsWorkBytes = size_t(256) << 20;       // large tier: signals per chunk bounded by this much scratch

inline int pow2_at_least(int64_t v)
{
    int m = 1;
    while (m < v) m <<= 1;
    return m;
}

// chirp conj(w) and the bit-reversed spectrum / M of the wrapped chirp w, for a DFT of N points on M (sign: +1 forward)
inline void bluestein_tables(int64_t N, int M, double sgn, resample_detail::cd* c, resample_detail::cd* B)
{
    using resample_detail::cd;
    std::vector<cd> w(static_cast<size_t>(N)), b(static_cast<size_t>(M), cd(0.0, 0.0));
    for (int64_t m = 0; m < N; ++m) {
        const int64_t r = (m * m) % (2 * N);             // m^2 reduced mod 2N keeps the angle exact
        const double ang = sgn * M_PI * static_cast<double>(r) / static_cast<double>(N);
        w[static_cast<size_t>(m)] = cd(std::cos(ang), std::sin(ang));
        c[m] = std::conj(w[static_cast<size_t>(m)]);
    }
    b[0] = w[0];
    for (int64_t m = 1; m < N; ++m) b[static_cast<size_t>(m)] = b[static_cast<size_t>(M - m)] = w[static_cast<size_t>(m)];
    resample_detail::fft_pow2(b, false);
    int lg = 0;
    while ((1 << lg) < M) ++lg;
    for (int j = 0; j < M; ++j) {
        int r = 0;
        for (int k = 0; k < lg; ++k) r |= ((j >> k) & 1) << (lg - 1 - k);
        B[j] = b[static_cast<size_t>(r)] / static_cast<double>(M);
    }
}

// twiddle table of the resample plans' convolutions on Mt points: exp(-2 pi i k / Mt), k < max(Mt / 2, 1)
inline size_t twiddle_count(int Mt) { return static_cast<size_t>(Mt > 1 ? Mt / 2 : 1); }
inline void twiddle_table(int Mt, resample_detail::cd* tw)
{
    for (size_t k = 0; k < twiddle_count(Mt); ++k) {
        const double ang = -2.0 * M_PI * static_cast<double>(k) / static_cast<double>(Mt);
        tw[k] = resample_detail::cd(std::cos(ang), std::sin(ang));
    }
}

// dense large tier: signals per chunk, each with Mw elements of work
inline long long dense_chunk(long long budget, long long Mw, long long batch)
{
    const long long per = budget / Mw;
    return per < 1 ? 1 : (per < batch ? per : batch);
}

struct Chunk { long long d0, cnt, Mw, t0, ntab, elems; };    // sorted signals d0 .. d0 + cnt, tables t0 .. t0 + ntab, elems of work + tables
struct Table { long long n, M, off; };                   // B1 / M of length n: M elements at `off` of its chunk's table region

struct RaggedPlan {
    std::vector<RaggedResampleSig> sig;                  // [count] in sorted order: sig[d].row is d's index in the caller's list
    std::vector<Chunk> chunks;
    std::vector<Table> tabs;                             // all chunks' tables, in chunk order
    int Mt = 1;                                          // the largest convolution of the call: max(M2, every M1)
    long long max_elems = 0;                             // the largest chunk
    size_t sig_bytes() const { return sig.size() * sizeof(RaggedResampleSig); }
    size_t desc_bytes() const { return sig_bytes() + tabs.size() * sizeof(long long); }
};

// starts / lens: count >= 1 signals, every length >= 1 (checked by the caller); start = starts[i] - xlo.  false: out of host memory
inline bool plan_ragged(const int64_t* starts, const int64_t* lens, int64_t count, int M2, long long xlo, long long budget, RaggedPlan& out)
{
    try {
        out = RaggedPlan{};
        std::vector<long long> ord(static_cast<size_t>(count));
        std::iota(ord.begin(), ord.end(), 0LL);
        std::stable_sort(ord.begin(), ord.end(), [&](long long a, long long b) { return lens[a] < lens[b]; });
        out.sig.resize(static_cast<size_t>(count));
        out.Mt = M2;
        Chunk c{0, 0, 0, 0, 0, 0};
        long long tab_elems = 0, prev_n = 0;
        for (long long d = 0; d < count; ++d) {
            const long long i = ord[static_cast<size_t>(d)], n = lens[i], M1 = pow2_at_least(2 * n - 1);
            const long long Mw = std::max<long long>(M1, M2);
            bool fresh = c.cnt == 0 || n != prev_n;
            if (c.cnt > 0 && (c.cnt + 1) * Mw + tab_elems + (fresh ? M1 : 0) > budget) {
                c.elems = c.cnt * c.Mw + tab_elems;
                out.chunks.push_back(c);
                c = Chunk{d, 0, 0, static_cast<long long>(out.tabs.size()), 0, 0};
                tab_elems = 0;
                fresh = true;
            }
            if (fresh) {
                out.tabs.push_back(Table{n, M1, tab_elems});
                tab_elems += M1;
                ++c.ntab;
            }
            ++c.cnt;
            c.Mw = Mw;
            out.sig[static_cast<size_t>(d)] = RaggedResampleSig{starts[i] - xlo, n, M1, out.tabs.back().off, i};
            out.Mt = std::max(out.Mt, static_cast<int>(M1));
            prev_n = n;
        }
        c.elems = c.cnt * c.Mw + tab_elems;
        out.chunks.push_back(c);
        for (const Chunk& ch : out.chunks) out.max_elems = std::max(out.max_elems, ch.elems);
    } catch (const std::bad_alloc&) {
        return false;
    }
    return true;
}

// the device's view of the plan into `block` (desc_bytes() of it): RaggedResampleSig[count] in sorted order, then the table lengths
inline void write_descriptors(const RaggedPlan& p, unsigned char* block)
{
    std::copy(p.sig.begin(), p.sig.end(), reinterpret_cast<RaggedResampleSig*>(block));
    auto* tn = reinterpret_cast<long long*>(block + p.sig_bytes());
    for (size_t u = 0; u < p.tabs.size(); ++u) tn[u] = p.tabs[u].n;
}

}  // namespace rslayout
}  // namespace hssfsst
