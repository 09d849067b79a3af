// fsst_mfma128.hpp -- second-generation synchrosqueeze core for the canonical window length
// nwin = 128 (the reference's Kaiser(128) configuration, /root/reference/main.py:153-158); the same kernel with a
// radix-16 first stage in two passes also serves nwin = 256 and, with 32 taps, nwin = 512 (template parameters NT = taps,
// RQ = first-stage radix, nwin = NT RQ; the description below is written for (16, 8)).
//
// Why a second kernel: measured on MI355X (profiles/r01_valu_ubench.txt) a 3-operand fp32 FMA
// costs ~4 cycles per wave64 instruction, an add ~2.8, a PACKED v_pk_{add,mul,fma}_f32 ~4.3 for two
// results, one wave per SIMD issues a VALU op only every ~5.4 cycles, and wave-uniform table
// constants cost SALU issue slots.  So this kernel
//   * runs the one dense contraction of the path -- the window multiply fused with the first
//     radix-8 decimation-in-frequency stage,  y_r[n] = sum_{q<8} x[t+n+16q] * C_r[n,q]  (a constant
//     16 x 8 real matrix applied at every tap n, for 16 frames at a time) -- as 32
//     v_mfma_f32_16x16x4_f32 per 16 frames (bit-exact fp32 FMA chain).  Measured
//     (profiles/r01_mfma_valu_overlap_ubench.txt): on this chip MFMA time does NOT hide behind VALU
//     time of the same SIMD, so the gain is not concurrency but issue economy: 32 instructions
//     instead of 256 v_pk_fma_f32 + their constant-operand traffic for the same ALU time; the
//     constants come from a shared 8 kB LDS table (one ds_read_b64 per tap), the frame operand is
//     one contiguous ds_read2_b32 per tap (hop-1 frames are shifted copies);
//   * finishes with two 16-point FFTs per lane written in packed (re,im) math: 74 v_pk ops each;
//   * 4 lanes per frame: lane group g = lane>>4 owns bin classes {g, 8-g} ({0,4} for g = 0), so a
//     bin k = 8j + r and its conjugate partner 128 - k are always in the same lane (two-for-one
//     real-FFT unpack without cross-lane traffic); the MFMA output fragment
//     D[row = 4g + {0,1,2,3}][frame] = {re, im} of class a, {re, im} of class b is exactly that.
//
// The arithmetic after the FFT (instantaneous-frequency test, cyclic scatter with the
// negative-frequency mirror, band truncation, abs / stack / raw epilogue, fp64 statistics partials)
// is the same as in fsst_kernels.hpp (its device code: fsst_device.hpp) and follows oracle/fsst_oracle.c steps 4-7.
#pragma once
#include "fsst_mfma128_device.hpp"

namespace hssfsst {

// ------------------------------------------------------------------------------------------------
// grid = persistent blocks of WPB waves (see "Work distribution" above); each WAVE draws chunks of one signal from
// the block's LDS counter, stages FPW + 127 samples per FPW frames and walks them in groups of 16 frames,
// independently of its sibling waves (no block barrier after the prologue).
// LDS: atab[16 taps][64 lanes][2] (shared, 8 KB) | control words + FAST store-offset table | per wave: xs[FPW+127] |
//      own plane | displaced plane | flag.
// ------------------------------------------------------------------------------------------------
// FAST: the time-major [re | im] epilogue with 16-byte stores (mode STACK / STACK_UNNORM, K even, K <= 24 -- the
// canonical configuration); otherwise the general epilogue (raw / abs / any K).  The host picks.
// WPB: waves per block -- 16 (a whole CU) whenever 16 wave regions fit the 160 KB of LDS, else 8 / 4 / 2 / 1.
// NT, RQ: taps (= size of the per-lane FFT) and radix of the first (matrix-pipe) stage, nwin = NT RQ.  (16, 8) is the
// canonical nwin = 128; (16, 16) = nwin 256 runs the same 8-class structure twice per group of frames ("passes":
// classes {0,8,1,15,2,14,3,13}, then {4,12,...,7,9}), each tap as a chain of RQ / 4 MFMA k-steps; (32, 16) = nwin 512
// does the same with 32 taps and 32-point FFTs per lane (two waves per SIMD, up to 256 VGPRs).
// S1C >= 0: the host guarantees that the kept band starts in stripe 0 and ends in stripe S1C (the canonical band
// [25, 200] Hz at fs = 1000 is stripes 0..3 for every RQ); the per-source "does this stripe have a column in the own
// plane" tests and their branches are then compile-time (measured 3.3-3.6 % of the kernel; making the whole band
// (klo, K) a compile-time constant gave nothing more).  S1C = -1: any band.
// FUSED (z-score inside the core launch; STACK, FAST epilogue, signals of at most kFusedMaxGroups groups): see the section
// "Fused z-score" inside the kernel.

// STREAM (one step of the rolling transform, BASELINE config 5; FAST epilogue, un-normalised): ONE launch per step instead of
// copy + transform + merge-and-normalise.  Blocks are bound to channels (bpc blocks per channel, block `part` takes the groups
// part, part + bpc, ... one group per ticket, staged exactly as the one-group chunks of the plain kernel: same tiles, same bits);
// a group's samples come from the tape or, from index hist on, straight from the step's new samples, which the group's wave also
// appends to the tape (nobody reads the tape there during the step); the block that delivers last for its channel (one counter
// per channel in HBM) runs the arithmetic of fsst_stream_finish_kernel on the channel's chunk.
// PAIR (nwin 256 / 512, whose transform is two passes over the same 16 frames): TWO waves share one wave region -- wave 2 r does
// pass 0 of region r's group, wave 2 r + 1 pass 1, at the same time; the passes write disjoint columns of the own plane, and the
// odd wave LISTS its additions into the displaced plane instead of making them (PairList): the even wave replays the list behind
// its own additions, so the plane receives every addition in the order of the one-wave kernel -- the same bits whoever runs
// faster.  The even wave then runs everything that follows the passes.  The pair
// meets through two phase words in LDS (pair_sync: LDS operations of a wave are executed in order, so a phase word written
// after a wave's data is seen after it): twice the waves on the same LDS -- 6 instead of 3 per CU for nwin 512 with 90 kept
// rows -- and half the latency of a lone group (one streaming step).
constexpr unsigned kPairSpinLimit = 1u << 24;       // looks at the partner's phase word before a pair's wait ends on its own (~1 s)
// RAGGED (hssfsst_exec_ragged: signals of different lengths in one launch): a chunk's signal, first group and groups come from
// the host-made list p.rchunk, and the signal's length, input, output and partials from p.rsig; everything else -- staging,
// transform, ties, epilogue -- is the plain kernel's, on that signal alone (reads past its own length see zeros).
template <int NT, int RQ, int FPW, bool FAST, int WPB, int S1C, bool FUSED = false, bool STREAM = false, bool PAIR = false,
          bool RAGGED = false>
__global__ __launch_bounds__(64 * WPB, (NT == 32 ? 2 : WPB == 16 ? 4 : WPB == 12 ? 3 : 2)) void fsst_core128_kernel(Core128Params p)
{
    static_assert(!STREAM || (FAST && !FUSED), "the streaming step: wide-store epilogue, no per-signal z-score");
    static_assert(!PAIR || (RQ == 16 && !FUSED && WPB % 2 == 0), "wave pairs: two passes, whole pairs");
    static_assert(!RAGGED || (!FUSED && !STREAM), "ragged lists: the plain kernel");
    // (FUSED && !FAST: the general epilogue's STACK mode -- any K, nwin 256 / 512 -- with the linear z-score sweep of
    //  fsst_normalize_kernel as the B ticket; the host sends only STACK execs whose signal blocks are 16-byte aligned)
    constexpr int NWIN = NT * RQ, NPASS = RQ / 8, KST = RQ / 4;
    constexpr int ATAB = core128_atab_floats(RQ, NT);
    // (FUSED && !FAST: the plain control block -- the statistics partials stay in HBM as on the two-launch path, the wave
    //  regions of nwin 256 / 512 leave no LDS for them --, resolved statistics at [16..31])
    constexpr int CTL = (FUSED && FAST) ? kCtlFusedFloats : kCtlFloats;
    constexpr int XS = ((FPW + NWIN - 1 + 3) / 4) * 4;
    using avec = float __attribute__((ext_vector_type(KST)));          // one tap's A operand, all k-steps
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int K = p.K, klo = p.klo;
    int n = p.n;                                         // (RAGGED: per chunk, as ncols, cend, ngroups)
    const int LDF = plane_ldf(K);
    const int OLD = own_ld(klo, K, RQ);
    const int s0 = (S1C >= 0) ? 0 : own_s0(klo, RQ), s1 = (S1C >= 0) ? S1C : own_s1(klo, K, RQ);

    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, j = lane & 15;
    float* atab = smem;                                                      // [pass][NT taps][64 lanes][KST]
    int* next_q = reinterpret_cast<int*>(smem + ATAB);                       // block's work counter
    unsigned* done_a = reinterpret_cast<unsigned*>(smem + ATAB) + 1;         // FUSED: [2] groups delivered (monotone)
    unsigned* dead = done_a + 2;                                             // FUSED: a wait of this block gave up
    unsigned* ready = dead + 1;                                              // FUSED: [4] epoch of fin_stats[]
    float4* fin_stats = reinterpret_cast<float4*>(smem + ATAB + (FAST ? 272 : 16));   // FUSED: [4] resolved statistics
    unsigned* cls_lds = reinterpret_cast<unsigned*>(smem + ATAB + 16);       // FUSED: [64] see "cls" below
    unsigned* ppk_lds = reinterpret_cast<unsigned*>(smem + ATAB + (FUSED ? 80 : 16));   // [3][64] wide-store offsets (FAST)
    float* part_lds = smem + ATAB + 288;                                     // FUSED: [2][kFusedMaxGroups][kPartFloats]
    const int role = PAIR ? (wv & 1) : 0;                                    // PAIR: the pass this wave does
    float* wbase = smem + ATAB + CTL + (PAIR ? (wv >> 1) : wv) * (wave_lds_floats(FPW, klo, K, RQ, NT) + (PAIR ? kPairFloats : 0));
    float* xs = wbase;
    f2* own_base = reinterpret_cast<f2*>(wbase + XS);
    f2* disp_base = own_base + 16 * OLD;
    int* flag = reinterpret_cast<int*>(disp_base + 16 * LDF);
    int* tq = flag + 4;                                                       // rounding-tie bitmap (tie_words(NWIN))
    int* pw = tq + tie_words(NWIN);                                           // PAIR: phase words, ticket
    float* pmx = reinterpret_cast<float*>(pw + 4);                            // PAIR: the odd wave's per-lane max
    PairList plist{pw + 4 + 64, reinterpret_cast<f2*>(pw + 4 + 64 + kPairListCap), pw + 3, 0};      // PAIR: the odd wave's additions
    bool pordered = false;                               // PAIR: a list overflowed: this pair forms the odd wave's sources behind the even wave's
    if constexpr (PAIR) { if (lane < 4) pw[lane] = 0; }
    int pphase = 0;
    auto pair_sync = [&]() {
        if constexpr (PAIR) {
            wave_sync();
            ++pphase;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) __hip_atomic_store(pw + role, pphase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            // (bounded like every wait of this library: the partner is a wave of the same workgroup and cannot stay away, but a
            //  kernel that could spin for ever is a kernel that can hang a GPU)
            bool met = false;
            for (unsigned spins = 0; spins < kPairSpinLimit; ++spins) {
                int v = 0;
                if (lane == 0) v = __hip_atomic_load(pw + (role ^ 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (__builtin_amdgcn_readfirstlane(v) - pphase >= 0) { met = true; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            // (a wait that ran out: the wave goes on -- on planes its partner may still be writing -- but not silently: the status word
            //  makes hssfsst_plan_check / the next exec / the next streaming step fail, as the bounded waits of the other kernels do)
            if (!met && lane == 0 && p.status) __hip_atomic_store((gu32*)(p.status), 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            wave_sync();
        }
    };

    // STREAM: tickets are dealt statically (wave region r takes the block's tickets r, r + regions, ...), so the first group's
    // samples can be on their way while the operand table is staged
    constexpr int NREG = PAIR ? WPB / 2 : WPB;
    constexpr int NPRE = (FPW + NWIN - 1 + 63) / 64;
    float pre[NPRE];
    int st_q = PAIR ? (wv >> 1) : wv;
    auto stream_sample = [&](long long ch, int gi) -> float {     // sample gi of the step's hist + chunk samples of channel ch
        const float* src = (p.xnew != nullptr && gi >= p.hist) ? p.xnew + ch * p.xnew_stride + (gi - p.hist) : p.x + ch * p.xstride + gi;
        return *src;
    };
    if constexpr (STREAM) {
        const int ch0 = static_cast<int>(blockIdx.x) / p.bpc, g0 = static_cast<int>(blockIdx.x) - ch0 * p.bpc + st_q * p.bpc;
#pragma unroll
        for (int k = 0; k < NPRE; ++k) {
            const int gi = g0 * 16 + lane + 64 * k;          // (t0 - NWIN / 2 = 16 g0: the step's frames start at col0 = NWIN / 2)
            pre[k] = (g0 * 16 < p.ncols && lane + 64 * k < FPW + NWIN - 1 && gi < p.n) ? stream_sample(ch0, gi) : 0.0f;
        }
    }
    // shared MFMA A operand, [pass * NT + tap][lane][k-step]: a lane reads all k-steps of a tap with one LDS instruction
    // (the host lays the table out like this: a straight 16-byte copy, 64 KiB of it for nwin 512)
    if constexpr ((ATAB / 4) % (64 * WPB) == 0 && ATAB / 4 / (64 * WPB) <= 16) {
        constexpr int NA = ATAB / 4 / (64 * WPB);            // all of a thread's loads in flight at once (one memory round trip)
        float4 t[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) t[k] = reinterpret_cast<const float4*>(p.atab)[threadIdx.x + k * 64 * WPB];
#pragma unroll
        for (int k = 0; k < NA; ++k) reinterpret_cast<float4*>(atab)[threadIdx.x + k * 64 * WPB] = t[k];
    } else {
        for (int i = threadIdx.x; i < ATAB / 4; i += 64 * WPB)
            reinterpret_cast<float4*>(atab)[i] = reinterpret_cast<const float4*>(p.atab)[i];
    }
    int ncols = p.ncols, cend = p.col0 + p.ncols;         // output rows are relative to col0
    for (int i = lane; i < 16 * LDF; i += 64) disp_base[i] = f2{0.0f, 0.0f};
    if (lane < 4) flag[lane] = 0;
    for (int i = lane; i < tie_words(NWIN); i += 64) tq[i] = 0;
    if (threadIdx.x < (FUSED ? 8 : 1)) next_q[threadIdx.x] = 0;
    if constexpr (FUSED && FAST) {
        if (wv == 0) {
            // bit 2i / 2i+1 of cls: the first / second pair of this lane's float4 i (of a group's [16][2K] image) is an
            // imaginary column
            unsigned cls = 0u;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const unsigned c = (4u * static_cast<unsigned>(lane + 64 * i)) % static_cast<unsigned>(2 * K);
                cls |= (c >= static_cast<unsigned>(K) ? 1u : 0u) << (2 * i);
                cls |= (c + 2 >= static_cast<unsigned>(K) ? 1u : 0u) << (2 * i + 1);
            }
            cls_lds[lane] = cls;
        }
    }
    // wide-store epilogue (time-major [re | im] rows, K even, <= 3 float4 per lane and group): every lane's six LDS byte
    // offsets of the store pass (host-made table, core128_store_offsets), two 16-bit offsets per word
    if constexpr (FAST) {
        if (wv == 0) {
            const int* ptab = reinterpret_cast<const int*>(p.atab + ATAB);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                ppk_lds[i * 64 + lane] = static_cast<unsigned>(ptab[i * 64 + lane]) | (static_cast<unsigned>(ptab[(3 + i) * 64 + lane]) << 16);
        }
    }
    __syncthreads();

    // chunk bookkeeping (wave-uniform)
    const int nc0 = p.nsig * p.reg.npc[0];               // (the host keeps nsig * chunks per signal below 2^31)
    const int nc1 = nc0 + p.nsig * p.reg.npc[1];
    const int nchunks = nc1 + p.nsig * p.reg.npc[2];
    int ngroups = (ncols + 15) >> 4;
    // FUSED work list of this block (wave-uniform): signals blockIdx, blockIdx + grid, ... (nk of them), each cut into
    // NC chunks of FPW / 16 groups; see "Fused z-score" below for the order of the 2 NC nk tickets
    constexpr int GPCF = FPW / 16;
    const int nk = (FUSED && p.nsig > static_cast<int>(blockIdx.x)) ? (p.nsig - static_cast<int>(blockIdx.x) + static_cast<int>(gridDim.x) - 1) / static_cast<int>(gridDim.x) : 0;
    const int NC = (ngroups + GPCF - 1) / GPCF;
    const int lead = min(8, NC);
    const int st_ch = STREAM ? static_cast<int>(blockIdx.x) / p.bpc : 0;              // STREAM: this block's channel and
    const int st_part = STREAM ? static_cast<int>(blockIdx.x) - st_ch * p.bpc : 0;    // its first group
    const int nwork = STREAM ? (st_part < ngroups ? (ngroups - st_part + p.bpc - 1) / p.bpc : 0) : FUSED ? 2 * NC * nk : RAGGED ? p.rnchunks : nchunks;
    auto draw = [&]() -> int {                           // next work item of this block, or nwork when none is left
        int q = 0;
        if (lane == 0) q = __hip_atomic_fetch_add(next_q, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        q = __builtin_amdgcn_readfirstlane(q);
        if constexpr (FUSED || STREAM) return q < nwork ? q : nwork;
        const long long c = static_cast<long long>(blockIdx.x) + static_cast<long long>(q) * gridDim.x;
        return c < nwork ? static_cast<int>(c) : nwork;
    };
    auto draw_pair = [&]() -> int {                      // PAIR: the even wave draws, the pair takes the ticket together
        if constexpr (STREAM) { const int q = st_q; st_q += NREG; return q < nwork ? q : nwork; }
        if constexpr (!PAIR) return draw();
        if (role == 0) { const int c = draw(); if (lane == 0) pw[2] = c; }
        pair_sync();
        return __builtin_amdgcn_readfirstlane(pw[2]);
    };
    const float* const rx = p.x;                         // RAGGED: the packed buffers (p.x / out / partials move to a chunk's signal)
    float* const rout = p.out;
    float* const rpart = p.partials;
    int chunk = draw_pair();
    bool first_tile = STREAM;                            // STREAM: the first ticket's samples are in `pre`
    const float* myA = atab + lane * KST;
    f2 tiny = {1.0e-37f, 0.0f};
    asm volatile("" : "+s"(tiny));                       // keep it in an SGPR pair (VOP3P takes no literal)
    while (chunk < nwork) {
    // decode: signal, first group, number of groups
    long long b;
    int grp0, ngrp;
    long long ksig = 0;                                  // FUSED: index of the signal in this block's list
    bool zpass = false;                                  // FUSED: this ticket is a z-score chunk
    if constexpr (FUSED) {
        // ------------------------------------------------------------------------------------------------
        // Fused z-score (FSST._stack_real_imag, synchrosqueeze.py:78-85) inside the core launch.
        // One CU owns whole signals; nothing crosses CUs (no flags in HBM, no placement assumption, no way to hang on
        // another block).  Its 16 waves draw TICKETS from one LDS counter.  A ticket is either a transform chunk A(k, c)
        // -- FPW / 16 groups of the block's k-th signal: transform, un-normalised features to HBM with ordinary stores,
        // one statistics partial per group into LDS -- or a z-score chunk B(k, c): read the same chunk back, z-score it
        // with the arithmetic of fsst_normalize_kernel, store it for good (streaming).  Ticket order: all A(0, .); then
        // for k = 1 .. nk-1 the first `lead` chunks of A(k, .), then B(k-1, 0), A(k, lead), B(k-1, 1), A(k, lead+1), ...
        // and what is left of B(k-1, .); finally B(nk-1, .).  The wave that delivers the last group of a signal turns
        // the signal's partials into {mean, 1/std} with signal_stats() -- the very function, order and data of the
        // two-kernel path, hence bit-identical results -- while its siblings already transform the next signal; a B
        // ticket waits (bounded) for that, which in the steady state it never has to: the B tickets of a signal start
        // `lead` chunks after its last A ticket was handed out.
        // Visibility: the un-normalised tile is written and read back by waves of ONE workgroup; the chain writer
        // (release on the delivery counter) -> resolver (acquire / release on `ready`) -> reader (acquire) is
        // workgroup scope, the waves share the CU's L1, and a line of `out` is read by this kernel exactly once.
        // Slots: the partials of signal k live in LDS slot k & 1, written by the A(k, .) tickets and read once by the
        // resolver of k.  A(k+2, .) tickets are handed out only after ALL NC tickets B(k, .) were handed out, and a B(k, .)
        // ticket is held (waiting) until the resolver of k is done; the 15 waves other than the resolver cannot hold NC
        // >= 16 of them, so slot reuse is safe by construction -- which is why the host sends signals of fewer than
        // kFusedMinChunks chunks down the two-kernel path.  {mean, 1/std} are copied to registers at the start of a B
        // ticket and live in 4 slots.
        // (An earlier variant -- teams of 8 CUs per signal with the tile meant to stay in the XCD's L2 -- was built,
        // bit-identical and slower; PMC showed that the L2 does not retain the written lines:
        // profiles/r02_fused_team_variant.txt.)
        // ------------------------------------------------------------------------------------------------
        int c;
        if (chunk < NC) {
            ksig = 0; c = chunk;
        } else {
            const int u = chunk - NC;
            const int kk = 1 + u / (2 * NC), v = u - (kk - 1) * (2 * NC);
            if (kk < nk) {
                const int npairs = NC - lead;
                if (v < lead) { ksig = kk; c = v; }
                else if (v - lead < 2 * npairs) {
                    const int w = v - lead;
                    if (w & 1) { ksig = kk; c = lead + (w >> 1); }
                    else { ksig = kk - 1; c = w >> 1; zpass = true; }
                } else { ksig = kk - 1; c = npairs + (v - lead - 2 * npairs); zpass = true; }
            } else { ksig = nk - 1; c = v; zpass = true; }
        }
        b = static_cast<long long>(blockIdx.x) + ksig * gridDim.x;
        grp0 = c * GPCF;
        ngrp = min(GPCF, ngroups - grp0);
    } else if constexpr (STREAM) {
        b = st_ch; grp0 = st_part + chunk * p.bpc; ngrp = 1;
    } else if constexpr (RAGGED) {
        // the chunk's signal becomes "signal 0" of a launch of its own: bases moved to it, its length as n and columns
        const int2 cd = p.rchunk[chunk];
        const RaggedSignal* rs = p.rsig + cd.x;
        const long long xoff = rs->xoff, ooff = rs->ooff, poff = rs->poff;
        n = rs->n; ncols = n; cend = n; ngroups = (n + 15) >> 4;
        p.x = rx + xoff; p.out = rout + ooff; p.partials = rpart + poff;
        b = 0;
        grp0 = cd.y & ((1 << kRaggedGroupBits) - 1);
        ngrp = (cd.y >> kRaggedGroupBits) + 1;
    } else {
        const int rg = (chunk < nc0) ? 0 : (chunk < nc1) ? 1 : 2;
        const int local = chunk - ((rg == 0) ? 0 : (rg == 1) ? nc0 : nc1);
        const int npc = p.reg.npc[rg], gpc = p.reg.gpc[rg];
        b = local / npc;
        const int cidx = local - static_cast<int>(b) * npc;
        grp0 = p.reg.g0[rg] + cidx * gpc;
        ngrp = min(gpc, ngroups - grp0);
    }
    // opaque copies of the lane coordinates for the HBM addressing below: otherwise the per-lane 64-bit address
    // parts are hoisted out of the chunk loop, held in registers across it and spilled to scratch (a kernel with
    // scratch costs isolated launches ~200 us on this runtime)
    int lane_o = lane;
    asm volatile("" : "+v"(lane_o));
    int g_o = lane_o >> 4, j_o = lane_o & 15;
    asm volatile("" : "+v"(g_o), "+v"(j_o));
    const int g = lane_o >> 4, j = lane_o & 15;          // (re-derived per work item: two registers fewer across the loop)
    f2* row_disp = disp_base + j * LDF;
    if (FUSED && zpass) {
        // ---- B(ksig, c): z-score of ngrp groups of a signal whose statistics are (about to be) in LDS
        const int sl = static_cast<int>(ksig) & 3;
        const unsigned epoch = static_cast<unsigned>(ksig) + 1u;
        const int C = 2 * K;
        float4* d4 = reinterpret_cast<float4*>(p.out + (b * static_cast<long long>(ncols) + grp0 * 16) * C) + lane_o;
        const int per = 8 * K;                           // float4 per full group = 16 * 2K / 4
        for (unsigned spins = 0;; ++spins) {
            unsigned have = 0;
            if (lane == 0) have = __hip_atomic_load(ready + sl, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (__builtin_amdgcn_readfirstlane(have) == epoch) break;
            if (spins >= kSpinLimit || __hip_atomic_load(dead, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                if (lane == 0) {
                    __hip_atomic_store((gu32*)(p.status), 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(dead, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                break;
            }
            __builtin_amdgcn_s_sleep(4);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const float4 st = fin_stats[sl];
        if constexpr (!FAST) {
            // general K: the chunk's frames x 2K floats are one contiguous, 16-byte aligned run of `out`; float4 sweep with
            // the column tracked incrementally and a per-element wrap test, the arithmetic of fsst_normalize_kernel
            // (kZB float4 per lane in flight at a time: one memory round trip per 64 kZB float4)
            constexpr int kZB = 12;
            const int frames = min(ngrp * 16, ncols - grp0 * 16);
            const int nfl = frames * C;                      // even
            const int nf4 = nfl >> 2;
            f4* b4 = reinterpret_cast<f4*>(p.out + (b * static_cast<long long>(ncols) + grp0 * 16) * C);
            int c = static_cast<int>((4u * static_cast<unsigned>(lane_o)) % static_cast<unsigned>(C));
            const int dc = static_cast<int>(256u % static_cast<unsigned>(C));
            auto zs1 = [&](float v, int col) -> float { return (col < K) ? (v - st.x) * st.y : (v - st.z) * st.w; };
            for (int i0 = 0; i0 < nf4; i0 += 64 * kZB) {
                f4 o[kZB];
#pragma unroll
                for (int u = 0; u < kZB; ++u) {
                    const int idx = i0 + 64 * u + lane_o;
                    o[u] = __builtin_nontemporal_load(b4 + (idx < nf4 ? idx : 0));
                }
#pragma unroll
                for (int u = 0; u < kZB; ++u) {
                    const int idx = i0 + 64 * u + lane_o;
                    int c1 = c + 1, c2 = c + 2, c3 = c + 3;
                    if (c1 >= C) c1 -= C;
                    if (c2 >= C) c2 -= C;
                    if (c3 >= C) c3 -= C;
                    const f4 r = {zs1(o[u].x, c), zs1(o[u].y, c1), zs1(o[u].z, c2), zs1(o[u].w, c3)};
                    if (idx < nf4) __builtin_nontemporal_store(r, b4 + idx);
                    c += dc;
                    if (c >= C) c -= C;
                }
            }
            if ((nfl & 2) && lane_o == 0) {                  // frames x 2K = 2 mod 4: the last two floats of the chunk
                float* tl = p.out + (b * static_cast<long long>(ncols) + grp0 * 16) * C + (nfl - 2);
                const int ct = C - 2;                        // (they end a row)
                tl[0] = zs1(tl[0], ct);
                tl[1] = zs1(tl[1], ct + 1);
            }
        } else {
        const unsigned cls = cls_lds[lane_o];
        // One memory round trip per ticket: all 12 pieces (4 groups x 3 float4) of the chunk in flight at once.  The loads
        // are unconditional (a lane without a piece re-reads the chunk's first float4): conditionally defined registers
        // made the allocator spill here although 100 registers are free.
        const float4* base0 = reinterpret_cast<const float4*>(p.out + (b * static_cast<long long>(ncols) + grp0 * 16) * C);
        auto glim = [&](int q) { return (q < ngrp) ? min(16, ncols - (grp0 + q) * 16) * (K >> 1) : 0; };
        {
            f4 o[GPCF][3];
#pragma unroll
            for (int q = 0; q < GPCF; ++q) {
                const int lim = glim(q);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float4* src = (lane_o + 64 * i < lim) ? (d4 + q * per + 64 * i) : base0;
                    // streaming loads: read once, must not displace anything (measured 0.247 vs 0.261 ms per launch
                    // with ordinary loads; streaming stores in the transform chunks on top of that give the gain back)
                    o[q][i] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(src));
                }
            }
            // this lane's {mean, 1/std} per float4 and pair, once per ticket (the column classes do not depend on the group)
            f2 mu[3][2], rs[3][2];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const bool im0 = (cls >> (2 * i)) & 1u, im1 = (cls >> (2 * i + 1)) & 1u;
                const float m0 = im0 ? st.z : st.x, r0 = im0 ? st.w : st.y;
                const float m1 = im1 ? st.z : st.x, r1 = im1 ? st.w : st.y;
                mu[i][0] = f2{m0, m0}; rs[i][0] = f2{r0, r0};
                mu[i][1] = f2{m1, m1}; rs[i][1] = f2{r1, r1};
            }
#pragma unroll
            for (int q = 0; q < GPCF; ++q) {
                const int lim = glim(q);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    if (lane_o + 64 * i < lim) {
                        const f2 lo = (f2{o[q][i].x, o[q][i].y} - mu[i][0]) * rs[i][0];     // (v - mean) * (1 / std): two roundings,
                        const f2 hi = (f2{o[q][i].z, o[q][i].w} - mu[i][1]) * rs[i][1];     // exactly as fsst_normalize_kernel
                        __builtin_nontemporal_store(f4{lo.x, lo.y, hi.x, hi.y}, reinterpret_cast<f4*>(d4 + q * per + 64 * i));
                    }
                }
            }
        }
        }
    } else {
    const float* xsig = p.x + b * p.xstride;
    auto stage_tile = [&](int t0) -> TileEnergy {        // xs[i] = xpad[t0 + i] = x[t0 + i - 64]; the tile's energy / offset test
        float e = 0.0f, s1 = 0.0f, cnt = 0.0f;
        int lane_t = lane;                               // (opaque per tile: the tile's lane addresses are not hoisted out of
        asm volatile("" : "+v"(lane_t));                 //  the chunk loop, held across the transform and spilled)
        if constexpr (STREAM) {
#pragma unroll
            for (int k = 0; k < NPRE; ++k) {                 // (the same elements in the same order as the loop below)
                const int i = lane_t + 64 * k;
                if (i < FPW + NWIN - 1) {
                    const int gi = t0 + i - NWIN / 2;
                    const bool in = (gi >= 0 && gi < n);
                    const float v = first_tile ? pre[k] : (in ? stream_sample(b, gi) : 0.0f);
                    xs[i] = v;
                    e = fmaf(v, v, e); s1 += v; cnt += in ? 1.0f : 0.0f;
                }
            }
            first_tile = false;
            return tile_energy(e, s1, cnt);
        }
        for (int i = lane_t; i < FPW + NWIN - 1; i += 64) {
            const int gi = t0 + i - NWIN / 2;
            const bool in = (gi >= 0 && gi < n);
            const float v = in ? xsig[gi] : 0.0f;
            xs[i] = v;
            e = fmaf(v, v, e); s1 += v; cnt += in ? 1.0f : 0.0f;
        }
        return tile_energy(e, s1, cnt);
    };
    for (int sub = 0; sub < ngrp; sub += FPW / 16) {
    const int t0 = p.col0 + (grp0 + sub) * 16;
    // R^2 of the tile's frames for the error bound of displaced cells (see "Rounding ties")
    const TileEnergy te = stage_tile(t0);
    const float R2 = p.r2scale * te.E;
    wave_sync();
    if constexpr (STREAM) {
        // the group's 16 new samples (hist + 16 grp0 + lane: the last sample of its frame `lane`) go to the tape; the groups of a
        // channel cover the chunk once
        if (p.xnew != nullptr && role == 0 && lane < 16 && grp0 * 16 + lane < ncols)
            const_cast<float*>(xsig)[p.hist + grp0 * 16 + lane] = p.xnew[b * p.xnew_stride + grp0 * 16 + lane];
    }
    const int gend = min(FPW / 16, ngrp - sub);
    for (int grp = 0; grp < gend; ++grp) {
    const int tg = t0 + grp * 16;
        const int tr = tg - p.col0;
        // the tile's LDS byte address as ONE opaque register: every tap is then an immediate offset of it
        // (otherwise each merged ds_read2 gets its own "base + 0x2000 + tap" v_add).  Lane (kk = lane >> 4, f = lane & 15)
        // is row kk of the B operand for frame f: sample f + tap + NT (kk + 4 ks); for NT = 16 that is lane + tap + 64 ks.
        unsigned xaddr = static_cast<unsigned>(reinterpret_cast<size_t>((lds_float*)(xs + grp * 16 + j + NT * g)));
        asm volatile("" : "+v"(xaddr));
        const lds_float* xb = (const lds_float*)static_cast<size_t>(xaddr);
        float mx = 0.0f;
        // ---- NPASS passes over the same 16 frames: pass pz handles class pairs 4 pz + g (pair 0 = the two
        //      self-conjugate classes {0, RQ/2}, pair m = {m, RQ - m})
        auto one_pass = [&](auto PZ) {
        constexpr int pz = decltype(PZ)::value;
        // keep the per-lane class ids opaque inside the loop: otherwise LICM hoists every
        // "rA + RQ s" of the rare path out of the loop and pins ~30 VGPRs for the whole kernel
        int pair = 4 * pz + g;
        asm volatile("" : "+v"(pair));
        const bool isg0 = (pz == 0) && (pair == 0);          // lane holds the self-conjugate pair
        const int rAi = pair, rBi = isg0 ? RQ / 2 : RQ - pair;
        f2* ownA = own_base + j * OLD + rAi - RQ * s0;       // column of k' = RQ s + rA at + RQ s
        f2* ownB = own_base + j * OLD + rBi - RQ * s0;
        const float* myAp = myA + pz * NT * 64 * KST;

        // ---- folded window + radix-RQ stage on the matrix pipe: NT taps x KST k-steps
        f2 za[NT], zb[NT];
        // four taps at a time, k-step by k-step (the dependent MFMA of a tap is issued three MFMAs after the
        // previous k-step of the same tap; measured 1 % faster than tap by tap)
        static_for<NT / 4>([&](auto GG) {
            constexpr int g0 = decltype(GG)::value * 4;
            f4 acc[4];
            avec a2[4];
            static_for<4>([&](auto I) {
                constexpr int i = decltype(I)::value;
                a2[i] = *reinterpret_cast<const avec*>(myAp + (g0 + i) * 64 * KST);
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[i][0], xb[g0 + i], f4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
            });
            static_for<KST - 1>([&](auto KS) {
                constexpr int ks = decltype(KS)::value + 1;
                __builtin_amdgcn_sched_barrier(0);
                static_for<4>([&](auto I) {
                    constexpr int i = decltype(I)::value;
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[i][ks], xb[g0 + i + 4 * NT * ks], acc[i], 0, 0, 0);
                });
            });
            static_for<4>([&](auto I) {
                constexpr int i = decltype(I)::value;
                za[bitrev_n<NT>(g0 + i)] = f2{acc[i].x, acc[i].y};
                zb[bitrev_n<NT>(g0 + i)] = f2{acc[i].z, acc[i].w};
            });
        });
        fft_n<NT>(za);
        fft_n<NT>(zb);
        // ---- one-sided sources of this lane: classes rA (array a) and rB (array b)
        bool listed = false;
        if constexpr (PAIR && pz == 1) {
            if (!pordered) {
                // the odd wave's sources at the same time as the even wave's: its additions into the displaced plane go to a list
                // (PairList) that the even wave replays behind its own -- the order of the one-wave kernel, the same bits
                listed = true;
                plist.rowoff = j * LDF;
                if (lane == 0) pw[3] = 0;
                wave_sync();
        static_for<NT / 2>([&](auto SS) {
                constexpr int s = decltype(SS)::value;
                // partner of a[s]: class 0 -> a[(NT-s) mod NT];  else b[NT-1-s].  partner of b[s]: class RQ/2 -> b[NT-1-s]; else a[NT-1-s]
                const f2 pa0 = za[(NT - s) & (NT - 1)], pb = zb[NT - 1 - s], pa = za[NT - 1 - s];
                f2 PA, PB;
                if constexpr (pz == 0) {
                    PA = f2{isg0 ? pa0.x : pb.x, isg0 ? pa0.y : pb.y};
                    PB = f2{isg0 ? pb.x : pa.x, isg0 ? pb.y : pa.y};
                } else {                                         // no self-conjugate class in the later passes
                    PA = pb; PB = pa;
                }
                const bool st = (s >= s0) && (s <= s1);
                process_stripe<s, RQ, NWIN, true>(za[s], PA, zb[s], PB, tiny, ownA + RQ * s, ownB + RQ * s, st, row_disp, flag, tq, j, klo, K, rAi, rBi, R2, mx, &plist);
            });
            } else {
                // (a list overflowed earlier: the odd wave forms its sources once the even wave is through its pass -- it has arrived
                //  at the sync behind it --, adding into the plane itself: the same order)
                bool met = false;
                for (unsigned spins = 0; spins < kPairSpinLimit; ++spins) {
                    int v = 0;
                    if (lane == 0) v = __hip_atomic_load(pw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (__builtin_amdgcn_readfirstlane(v) - (pphase + 1) >= 0) { met = true; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                if (!met && lane == 0 && p.status) __hip_atomic_store((gu32*)(p.status), 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                wave_sync();
                if (lane == 0) pw[3] = 0;
            }
        }
        if (!listed)
        static_for<NT / 2>([&](auto SS) {
            constexpr int s = decltype(SS)::value;
            // partner of a[s]: class 0 -> a[(NT-s) mod NT];  else b[NT-1-s].  partner of b[s]: class RQ/2 -> b[NT-1-s]; else a[NT-1-s]
            const f2 pa0 = za[(NT - s) & (NT - 1)], pb = zb[NT - 1 - s], pa = za[NT - 1 - s];
            f2 PA, PB;
            if constexpr (pz == 0) {
                PA = f2{isg0 ? pa0.x : pb.x, isg0 ? pa0.y : pb.y};
                PB = f2{isg0 ? pb.x : pa.x, isg0 ? pb.y : pa.y};
            } else {                                         // no self-conjugate class in the later passes
                PA = pb; PB = pa;
            }
            const bool st = (s >= s0) && (s <= s1);
            process_stripe<s, RQ, NWIN>(za[s], PA, zb[s], PB, tiny, ownA + RQ * s, ownB + RQ * s, st, row_disp, flag, tq, j, klo, K, rAi, rBi, R2, mx);
        });
        // k' = nwin/2 (class 0, j = 8) is its own partner: V = 2 Re(Z[nwin/2]) is real, its shift is exactly 0
        if constexpr (pz == 0) {
            if (s1 == NT / 2 && isg0) own_base[j * OLD + NWIN / 2 - RQ * s0] = f2{2.0f * za[NT / 2].x, 0.0f};
        }
        };
        if constexpr (PAIR) {
            for (int attempt = 0; attempt < 2; ++attempt) {
                mx = 0.0f;
                if (role == 0) one_pass(std::integral_constant<int, 0>{});
                else { one_pass(std::integral_constant<int, 1>{}); pmx[lane] = mx; }
                pair_sync();                                 // both passes are in the planes, the odd wave's additions in its list
                const int cnt = __builtin_amdgcn_readfirstlane(pw[3]);
                if (cnt <= kPairListCap) {
                    if (role == 0 && cnt > 0) {              // replay: list order = the one-wave kernel's order of pass 1
                        float* dpl = reinterpret_cast<float*>(disp_base);
                        for (int base = 0; base < cnt; base += 64) {
                            const int i = base + lane;
                            if (i < cnt) {
                                float* q = dpl + plist.cell[i];
                                const f2 v = plist.val[i];
                                __hip_atomic_fetch_add(q, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                __hip_atomic_fetch_add(q + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        }
                        wave_sync();
                    }
                    break;
                }
                // (rare) more additions than the list holds: the planes are cleaned and the group is done again with the odd wave's
                // sources behind the even wave's -- for the rest of this pair's launch (a tonal input that moves everything)
                if (role == 0) {
                    for (int i = lane; i < 16 * LDF; i += 64) disp_base[i] = f2{0.0f, 0.0f};
                    if (lane == 0) flag[0] = 0;
                    wave_sync();
                }
                pordered = true;
                pair_sync();
            }
            if (role == 0) mx = fmaxf(mx, pmx[lane]);
        } else {
            static_for<NPASS>(one_pass);
            wave_sync();
        }
        if (!PAIR || role == 0) {                            // (PAIR: the odd wave waits at the sync that ends the group)
        // one LDS round trip for both per-group flags (dirty displaced plane, queued rounding ties)
        int f_dirty = flag[0];
        const int f_ties = flag[1];
        bool exact = false;
        // ---- "Exact groups": no stored cell reaches kExactTheta R of the tile -> the R of the group's own samples -> float64
        if (__builtin_amdgcn_ballot_w64(mx > kExactTheta2 * R2) == 0ull && R2 > 0.0f) {
            float e2 = 0.0f;
            int lane_e = lane;
            asm volatile("" : "+v"(lane_e));
            for (int i = lane_e; i < 16 + NWIN - 1; i += 64) { const float v = xs[grp * 16 + i]; e2 = fmaf(v, v, e2); }
            const float R2g = p.r2scale * __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(piece_sums(e2, 0.0f, 0.0f, 0.0f))));
            exact = __builtin_amdgcn_ballot_w64(mx > kExactTheta2 * R2g) == 0ull && R2g > 0.0f;
        }
        if (te.dcdom) exact = true;                      // (an offset with little on top: tile_energy, fsst_device.hpp)
        if (exact) {
            for (int i = lane_o; i < 16 * LDF; i += 64) disp_base[i] = f2{0.0f, 0.0f};
            if (lane_o < 2) flag[lane_o] = 0;
            wave_sync();
            const float* xg = xs + grp * 16;
            resolve_bitmap<NWIN, true>(reinterpret_cast<unsigned*>(tq), [xg](int i) -> double { return static_cast<double>(xg[i]); }, disp_base, LDF,
                                       flag, klo, K, own_base, OLD, RQ * s0, RQ * (s1 + 1), p.wtab, p.twtab, 1.0, lane_o);
            wave_sync();
            f_dirty = flag[0];
        } else if (__builtin_amdgcn_readfirstlane(f_ties) != 0) {       // (rare) cells whose rounding float32 cannot decide
            resolve_ties<NWIN>(tq, xs + grp * 16, disp_base, LDF, flag, klo, K, own_base, OLD, RQ * s0, RQ * (s1 + 1), p.wtab, p.twtab, lane_o);
            wave_sync();
            f_dirty = flag[0];
        }

        // ---- epilogue for these 16 frames: element f -> (frame jj, kept row k)
        const bool wdirty = __builtin_amdgcn_readfirstlane(f_dirty) != 0;
        const int nvalid = min(16, cend - tg);
        const int koff = klo - RQ * s0;
        const int gidx = grp0 + sub + grp;                   // group index in the signal = statistics partial slot
        if constexpr (FAST) {
            // lane (g, j): frame j, kept rows k = g + 4 u (u < 6 covers K <= 24) as packed (re, im) cells
            f2* src = own_base + j * OLD + koff + g;
            if (wdirty) {                                    // (rare) fold the displaced plane into the own plane
                const f2* dsp = disp_base + j * LDF + g;
#pragma unroll
                for (int u = 0; u < 6; ++u)
                    if (g + 4 * u < K) src[4 * u] += dsp[4 * u];
                wave_sync();
            }
            if (p.mode == kModeStack) {
                // statistics partial of this group (see "Statistics" in fsst_device.hpp): sums of (v - pivot) and
                // (v - pivot)^2 about a pivot (pivot_med3).  Six unconditional cell reads (a row past the
                // band still lies inside this wave's LDS), then only the one row group that is partial across lanes
                // pays for a select
                // (pivot: median of frame 0's first, middle and last kept row -- pivot_med3, fsst_device.hpp; broadcast reads)
                const f2 pv0 = own_base[koff], pv1 = own_base[koff + (K >> 1)], pv2 = own_base[koff + K - 1];
                const f2 piv = f2{pivot_med3(pv0.x, pv1.x, pv2.x), pivot_med3(pv0.y, pv1.y, pv2.y)};
                f2 v[6];
#pragma unroll
                for (int u = 0; u < 6; ++u) v[u] = src[4 * u];
                const int ufull = (nvalid == 16) ? (K >> 2) : 0;     // rows 4u + 3 < K: valid in every lane
                const bool jv = j < nvalid;
                f2 st_s = {0.0f, 0.0f}, st_q = {0.0f, 0.0f};
#pragma unroll
                for (int u = 0; u < 6; ++u) {
                    const f2 d = v[u] - piv;
                    if (u < ufull) {
                        st_s += d; st_q = pk_fma(d, d, st_q);
                    } else if (4 * u < K) {
                        const bool ok = jv && (g + 4 * u < K);
                        const f2 dm = {ok ? d.x : 0.0f, ok ? d.y : 0.0f};
                        st_s += dm; st_q = pk_fma(dm, dm, st_q);
                    }
                }
                const float w = piece_sums(st_s.x, st_q.x, st_s.y, st_q.y);
                if constexpr (FUSED) store_partial(part_lds + ((static_cast<int>(ksig) & 1) * kFusedMaxGroups + gidx) * kPartFloats, w, piv.x, piv.y);
                else store_partial(p.partials + (b * ngroups + gidx) * kPartFloats, w, piv.x, piv.y);
            }
            // the group's nvalid x 2K floats are contiguous in HBM: 16-byte stores, lane-linear; each float4 =
            // two adjacent (re,re) or (im,im) pairs of one frame row.  All LDS reads first, then the stores.
            const int C = 2 * K;
            const char* ob = reinterpret_cast<const char*>(own_base);
            float4* dst4 = reinterpret_cast<float4*>(p.out + (b * static_cast<long long>(ncols) + tr) * C) + lane_o;
            const int lim = nvalid * (K >> 1);
            f4 o[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const unsigned pk = ppk_lds[i * 64 + lane_o];
                const int p0 = static_cast<int>(pk & 0xffffu), p1 = static_cast<int>(pk >> 16);
                o[i].x = *reinterpret_cast<const float*>(ob + p0);
                o[i].y = *reinterpret_cast<const float*>(ob + p0 + 8);
                o[i].z = *reinterpret_cast<const float*>(ob + p1);
                o[i].w = *reinterpret_cast<const float*>(ob + p1 + 8);
            }
            asm volatile("" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]));   // keep the reads ahead of the predicated stores
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                if (lane + 64 * i < lim) {
                    // FUSED: ordinary stores (a wave of this CU reads the tile back for the z-score).  Otherwise
                    // streaming stores: the features are not read again by this kernel, and lines left dirty in L2 by
                    // 256 CUs that all write until the last microsecond cost ~10 us of write-back after the kernel
                    if constexpr (FUSED) *reinterpret_cast<f4*>(dst4 + 64 * i) = o[i];
                    else if constexpr (STREAM) {
                        if (p.state != nullptr) {
                            // read back by the channel's last block, which may sit on another XCD: agent-scope stores (sc1, written
                            // through) and agent-scope loads there -- no L2 write-back / invalidate fences (measured: they made
                            // the step 51 us instead of 33)
                            unsigned long long* q = reinterpret_cast<unsigned long long*>(dst4 + 64 * i);
                            __hip_atomic_store(q, static_cast<unsigned long long>(__float_as_uint(o[i].x)) | (static_cast<unsigned long long>(__float_as_uint(o[i].y)) << 32),
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_store(q + 1, static_cast<unsigned long long>(__float_as_uint(o[i].z)) | (static_cast<unsigned long long>(__float_as_uint(o[i].w)) << 32),
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        } else {
                            __builtin_nontemporal_store(o[i], reinterpret_cast<f4*>(dst4 + 64 * i));
                            if (p.mirror != nullptr)         // (no normalisation: the features are final, the host copy is written here)
                                __builtin_nontemporal_store(o[i], reinterpret_cast<f4*>(p.mirror + (b * static_cast<long long>(ncols) + tr) * C) + lane_o + 64 * i);
                        }
                    }
                    else __builtin_nontemporal_store(o[i], reinterpret_cast<f4*>(dst4 + 64 * i));
                }
            }
            if constexpr (STREAM) {
                // the group IS a piece of the running moments' summation order (fsst_device.hpp, chunk_moments): its float64
                // sums from the image registers -- the elements and the order piece_moments takes from memory
                if (p.state != nullptr) {
                    double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        if (lane_o + 64 * i < lim) mom_acc4(a, make_float4(o[i].x, o[i].y, o[i].z, o[i].w), lane_o + 64 * i, C, K);
                    unsigned long long* pq = reinterpret_cast<unsigned long long*>(p.pieces + (b * ngroups + gidx) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double t = wave_sum(a[e]);
                        if (lane_o == 0) __hip_atomic_store(pq + e, static_cast<unsigned long long>(__double_as_longlong(t)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
        } else if (p.mode == kModeRaw) {
            float2* dst = reinterpret_cast<float2*>(p.out) + (b * K) * static_cast<long long>(ncols) + tr;
            int e0 = lane_o;                                 // opaque per GROUP (see the general epilogue below)
            asm volatile("" : "+v"(e0));
            for (int e = e0; e < K * 16; e += 64) {
                const int k = e >> 4, jj = e & 15;
                if (jj < nvalid) {
                    f2 v = own_base[jj * OLD + koff + k];
                    if (wdirty) v += disp_base[jj * LDF + k];
                    dst[static_cast<long long>(k) * ncols + jj] = make_float2(v.x, v.y);
                }
            }
        } else {
            // lane (g, j): frame j, kept rows k = g, g + 4, g + 8 ... as packed (re, im) pairs
            const bool isabs = (p.mode == kModeAbs);
            f2 pv0 = own_base[koff], pv1 = own_base[koff + (K >> 1)], pv2 = own_base[koff + K - 1];     // statistics pivot: pivot_med3 of frame 0
            if (wdirty) { pv0 += disp_base[0]; pv1 += disp_base[K >> 1]; pv2 += disp_base[K - 1]; }
            const f2 piv = f2{pivot_med3(pv0.x, pv1.x, pv2.x), pivot_med3(pv0.y, pv1.y, pv2.y)};
            f2 st_s = {0.0f, 0.0f}, st_q = {0.0f, 0.0f};
            if (j < nvalid) {
                const int C = isabs ? K : 2 * K;
                const int steps = (K - g + 3) >> 2;          // rows g + 4 i < K
                const f2* src = own_base + j * OLD + koff + g;
                const f2* dsp = disp_base + j * LDF + g;
                // (uniform 64-bit base + a 32-bit lane offset: no per-lane 64-bit address pair to keep or spill)
                float* gbase = p.out + (b * static_cast<long long>(ncols) + tr) * C;
                int g_g = g_o, j_g = j_o;                    // opaque per GROUP: otherwise the two addresses are computed per
                asm volatile("" : "+v"(g_g), "+v"(j_g));     // chunk, held through the transform and spilled
                const int loff = j_g * C + g_g;
                float* dst = gbase + loff;
                float* dsti = gbase + (loff + K);
                for (int i = 0; i < steps; ++i) {
                    f2 v = src[4 * i];
                    if (wdirty) v += dsp[4 * i];
                    if (isabs) {
                        dst[4 * i] = sqrtf(fmaf(v.x, v.x, v.y * v.y));
                    } else {
                        dst[4 * i] = v.x;
                        dsti[4 * i] = v.y;
                        const f2 d = v - piv;
                        st_s += d;
                        st_q = pk_fma(d, d, st_q);
                    }
                }
            }
            if (p.mode == kModeStack) {
                const float w = piece_sums(st_s.x, st_q.x, st_s.y, st_q.y);
                store_partial(p.partials + (b * ngroups + gidx) * kPartFloats, w, piv.x, piv.y);     // (FUSED too: see CTL)
            }
        }
        wave_sync();
        if (wdirty) {
            for (int i = lane_o; i < 16 * LDF; i += 64) disp_base[i] = f2{0.0f, 0.0f};
            if (lane_o == 0) *flag = 0;
            wave_sync();
        }
        }
        pair_sync();                                         // the planes are free for the next group's passes
    }
    }
    if constexpr (FUSED) {
        // ---- A(ksig, c) delivered: count its groups; whoever completes the signal resolves its statistics
        const int sl = static_cast<int>(ksig) & 1;
        unsigned before = 0;
        if (lane == 0) before = __hip_atomic_fetch_add(done_a + sl, static_cast<unsigned>(ngrp), __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        before = __builtin_amdgcn_readfirstlane(before);
        // (monotone counter: slot sl has seen the signals sl, sl + 2, ..., ksig; no reset, no window for a race)
        if (before + static_cast<unsigned>(ngrp) == static_cast<unsigned>(ngroups) * (static_cast<unsigned>(ksig >> 1) + 1u)) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            int ncols_o = ncols, K_o = K, ng_o = ngroups;    // opaque: nothing of the float64 arithmetic below may be
            asm volatile("" : "+s"(ncols_o), "+s"(K_o), "+s"(ng_o));   // hoisted out of the work loop (it would be spilled)
            // (!FAST: the partials were written to HBM by waves of this workgroup, each wave's stores complete before its
            //  release on the delivery counter, and no line of them was read by this CU before)
            const float* parts = FAST ? part_lds + sl * kFusedMaxGroups * kPartFloats : p.partials + b * ngroups * kPartFloats;
            const float4 st = signal_stats(parts, ng_o, 16, ncols_o, K_o, lane_o);
            if (lane == 0) {
                fin_stats[static_cast<int>(ksig) & 3] = st;
                __hip_atomic_store(ready + (static_cast<int>(ksig) & 3), static_cast<unsigned>(ksig) + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            wave_sync();
        }
    }
    }
    chunk = draw_pair();
    }
    if constexpr (STREAM) {
        if (p.state != nullptr) {
            // the channel's last block to get here merges the chunk into the running moments and normalises it
            // this wave's feature stores (agent scope, written through) are out; the counter below and the loads of the last block
            // are agent-scope accesses issued after that
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                                          // (the operand table in LDS is dead from here on)
            unsigned* last_sh = reinterpret_cast<unsigned*>(smem);
            if (threadIdx.x == 0) {
                const unsigned before = __hip_atomic_fetch_add(p.arrive + st_ch, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool last = before + 1u == static_cast<unsigned>(p.bpc);
                if (last) __hip_atomic_store(p.arrive + st_ch, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (steps are stream-ordered)
                last_sh[0] = last ? 1u : 0u;
            }
            __syncthreads();
            if (last_sh[0] != 0u) {
                float4* st_sh = reinterpret_cast<float4*>(smem + 4);
                float* cbase = p.out + static_cast<long long>(st_ch) * ncols * (2 * K);
                constexpr int NPF = 6;                       // the chunk's first float4s per thread, in flight during the merge
                float4 cpre[NPF];
                stream_normalize_load<64 * WPB, NPF>(cbase, ncols, K, static_cast<int>(threadIdx.x), cpre, AgentLoad4());
                if (wv == 0) {
                    const unsigned long long* pq = reinterpret_cast<const unsigned long long*>(p.pieces + static_cast<long long>(st_ch) * ngroups * 4);
                    double m[4];
                    moments_from_pieces(ngroups, lane, [&](int q, int e) {
                        return __longlong_as_double(static_cast<long long>(__hip_atomic_load(pq + q * 4 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
                    }, m);
                    if (lane < 2) {
                        const float2 r = merge_state(p.state + static_cast<long long>(st_ch) * 6 + lane * 3, m[2 * lane], m[2 * lane + 1],
                                                     static_cast<double>(K) * static_cast<double>(ncols));
                        float* sf = reinterpret_cast<float*>(st_sh);
                        sf[2 * lane] = r.x; sf[2 * lane + 1] = r.y;
                    }
                }
                __syncthreads();
                stream_normalize_apply<64 * WPB, NPF>(cbase, ncols, K, static_cast<int>(threadIdx.x), *st_sh, cpre, AgentLoad4(),
                                                      p.mirror ? p.mirror + static_cast<long long>(st_ch) * ncols * (2 * K) : nullptr);
            }
        }
    }
}

}  // namespace hssfsst
