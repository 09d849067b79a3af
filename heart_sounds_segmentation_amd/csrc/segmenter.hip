// segmenter.hip -- the BiLSTM's host side: the inference segmenter (hssfsst_segmenter*) and the trainable layer
// (hssfsst_bilstm*), with the forward path, the list tables and the pack they share.  C ABI: include/hssfsst.h.
#include "host_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "segmenter_lstm.hpp"
#include "segmenter_layout.hpp"
#include "segmenter_train.hpp"

using namespace hssfsst::host;

// BiLSTM segmenter (hssfsst.h: hssfsst_segmenter_create): the model's weights, uploaded once in the layouts the kernels of
// csrc/segmenter_lstm.hpp consume, plus the scratch of its execs (owned by the plan, grown on demand, freed with it).
namespace {

// The forward tables of one BiLSTM layer, as the kernels of csrc/segmenter_lstm.hpp consume them (seglayout::wt_source,
// gate_col_row, fwd_stream_source): made on the host by seg_upload_layer or on the device by seg_pack_kernel.
struct SegLayer {
    int F = 0, Fp = 0;                                   // input width and its multiple of 32
    DevBuf<float> d_wt;                                  // [dir][Fp][4 Hp]: W_ih^T, columns in (unit tile, gate, unit) order
    DevBuf<float> d_bias;                                // [dir][4 Hp]: b_ih + b_hh, same order
    DevBuf<hssfsst::seg_h8> d_whh;                       // [dir][wave][K block][tile x gate][lane]{hi, lo}: W_hh x wscale, split f16
};

// The list of a ragged call on the device: its layout (segmenter_layout.hpp) and the layout's tables in one block
// (seglayout::table_block), made and uploaded only when the offsets differ from the last call's.
struct SegListTables {
    struct Views {
        const long long *off, *base;
        const int *len, *rec, *walk;
        int slots;
        long long walked;                                // base[tiles]: the steps one direction walks
    };
    hssfsst::seglayout::Layout lay;                      // (of tab's key: rebuilt between its begin and commit)
    UploadedTable tab;
    explicit SegListTables(const char* what) : tab(what) {}
    // offsets: checked by seg_check_list.  May throw std::bad_alloc.
    int acquire(const int64_t* offsets, int64_t count, hipStream_t st, Views* out)
    {
        namespace seglayout = hssfsst::seglayout;
        const seglayout::TableBlock b = seglayout::table_block(count);
        auto key = [&](size_t i) { return offsets[i]; };
        if (!tab.same(static_cast<size_t>(count + 1), key)) {
            unsigned char* h = nullptr;
            if (int rc = tab.begin(b.bytes, &h)) return rc;
            seglayout::build(offsets, count, lay);
            const std::vector<long long> base = seglayout::tile_base(lay);
            std::memcpy(h + b.o_off, lay.slot_off.data(), b.slots * sizeof(long long));
            std::memcpy(h + b.o_base, base.data(), (b.tiles + 1) * sizeof(long long));
            std::memcpy(h + b.o_len, lay.slot_len.data(), b.slots * sizeof(int));
            std::memcpy(h + b.o_rec, lay.slot_rec.data(), b.slots * sizeof(int));
            std::memcpy(h + b.o_walk, lay.tile_walk.data(), b.tiles * sizeof(int));
            if (int rc = tab.commit(st, static_cast<size_t>(count + 1), key)) return rc;
        }
        out->off = reinterpret_cast<const long long*>(tab.get() + b.o_off);
        out->base = reinterpret_cast<const long long*>(tab.get() + b.o_base);
        out->len = reinterpret_cast<const int*>(tab.get() + b.o_len);
        out->rec = reinterpret_cast<const int*>(tab.get() + b.o_rec);
        out->walk = reinterpret_cast<const int*>(tab.get() + b.o_walk);
        out->slots = static_cast<int>(b.slots);
        out->walked = seglayout::stash_floats_ragged(lay) / (2 * seglayout::kStashStepFloats);
        return 0;
    }
};

}  // namespace

struct hssfsst_segmenter {
    int device = -1;
    int F = 0, H = 0;
    struct Layer : SegLayer {
        float inv_scale = 1.0f;                          // 1 / (wscale x kSegHScale)
    } layer[2];
    DevBuf<float> d_lin;                                 // linear.weight (4, 2H) | linear.bias (4)
    DevBuf<float> d_pre;                                 // [dir][batch tile][Tc][gate tile][lane][4]: one chunk's input projection
    DevBuf<float> d_y1, d_y2;                            // (B, T, 2H): the layers' outputs
    DevBuf<float> d_state;                               // [h, c][dir][Bp][Hp]: carried from chunk to chunk and from layer 1 to layer 2
    SegListTables list{"segmenter_exec_ragged"};         // hssfsst_segmenter_exec_ragged: kept while the next call has the same offsets
};

namespace {

// src: {weight_ih, weight_hh, bias_ih, bias_hh} x {forward, reverse} of one nn.LSTM layer, as in its state_dict.  Every table is
// filled by its output index through the functions seg_pack_kernel uses; the scale is seg_pack_scale_kernel's.
int seg_upload_layer(hssfsst_segmenter::Layer& L, int F, int H, const float* const* src)
{
    namespace sl = hssfsst::seglayout;
    L.F = F;
    L.Fp = (F + 31) / 32 * 32;
    float wmax = 0.0f;
    for (int d = 0; d < 2; ++d) {
        const float* whh = src[4 * d + 1];
        for (size_t i = 0; i < static_cast<size_t>(4) * H * H; ++i) wmax = std::fmax(wmax, std::fabs(whh[i]));
    }
    // power-of-two scale that puts the largest |W_hh| in [2^12, 2^13): the lo halves of the split are normal f16 numbers down to
    // weights 2^-26 times the largest one, and a sum of 256 products with |h| x 2^10 stays far below the f32 range
    int e = 0;
    float wscale = 1.0f;
    if (wmax > 0.0f && std::isfinite(wmax)) { (void)std::frexp(wmax, &e); wscale = std::ldexp(1.0f, 13 - e); }
    L.inv_scale = 1.0f / (wscale * hssfsst::kSegHScale);
    const long long per_wt = static_cast<long long>(L.Fp) * sl::kGateCols, per_f = sl::kWtStreamHalves / 2;
    std::vector<float> wt(static_cast<size_t>(2 * per_wt)), bias(static_cast<size_t>(2) * sl::kGateCols);
    std::vector<_Float16> stream(static_cast<size_t>(2 * per_f));
    for (int d = 0; d < 2; ++d) {
        const float *wih = src[4 * d], *whh = src[4 * d + 1], *bih = src[4 * d + 2], *bhh = src[4 * d + 3];
        for (long long i = 0; i < per_wt; ++i) {
            const long long s = sl::wt_source(i, F, H);
            wt[static_cast<size_t>(d * per_wt + i)] = s >= 0 ? wih[s] : 0.0f;
        }
        for (int n = 0; n < sl::kGateCols; ++n) {
            const long long row = sl::gate_col_row(n, H);
            bias[static_cast<size_t>(d) * sl::kGateCols + n] = row >= 0 ? bih[row] + bhh[row] : 0.0f;
        }
        for (long long i = 0; i < per_f; ++i) {
            int lo = 0;
            const long long s = sl::fwd_stream_source(i, H, &lo);
            _Float16 out = static_cast<_Float16>(0.0f);
            if (s >= 0) {
                const float v = whh[s] * wscale;
                const _Float16 hi = static_cast<_Float16>(v);
                out = lo ? static_cast<_Float16>(v - static_cast<float>(hi)) : hi;
            }
            stream[static_cast<size_t>(d * per_f + i)] = out;
        }
    }
    if (int rc = L.d_wt.upload(wt.data(), wt.size())) return rc;
    if (int rc = L.d_bias.upload(bias.data(), bias.size())) return rc;
    return L.d_whh.upload(reinterpret_cast<const hssfsst::seg_h8*>(stream.data()), stream.size() / 8);
}

constexpr int64_t kSegMaxSteps = 0x7fffffffLL / 8;       // steps of one dense exec, and of one recording of a ragged one
constexpr int64_t kSegMaxBatch = 16 * 32768;
static_assert(hssfsst::seglayout::kSlotRows == hssfsst::kSegRows, "a tile of the layout is the recurrence workgroup's rows");

constexpr size_t kSegTileStepBytes = static_cast<size_t>(2) * hssfsst::kSegGateTiles * hssfsst::kSegTileFloats * sizeof(float);   // seglayout::Chunk

// The segmenter's A-B switch, read ONCE per process (first use) from the environment like the FSST switches (fsst_plan.hpp:
// debug_switches): HSSFSST_SEG_RAGGED_PRE_MIB, the ragged exec's bound of the projection scratch in MiB (a number; 0 or unset: the
// dense call's 128).  It changes no result.
int seg_ragged_pre_mib()
{
    static const int mib = [] {
        const char* pm = std::getenv("HSSFSST_SEG_RAGGED_PRE_MIB");
        return pm != nullptr ? std::min(std::max(std::atoi(pm), 0), 1 << 16) : 0;
    }();
    return mib;
}

int seg_check_dtype(const char* what, int feats_dtype)
{
    if (feats_dtype != HSSFSST_DTYPE_F32 && feats_dtype != HSSFSST_DTYPE_F16 && feats_dtype != HSSFSST_DTYPE_BF16)
        return fail(HSSFSST_EINVAL, "%s: unknown feature dtype %d", what, feats_dtype);
    return 0;
}

// The one pointer of each entry point here that a kernel touches sixteen bytes at a time: logp (seg_head_kernel stores a row as one
// float4) and the training stash (seg_rec_kernel<.., TRAIN> and seg_bwd_rec_kernel move it in float4s).  Every other tensor is read
// and written one element at a time and may sit at any float.  The text is the sequence entries' (sequence.hip: seq_check_aligned).
int seg_check_aligned16(const char* what, const char* name, const void* ptr)
{
    if ((reinterpret_cast<uintptr_t>(ptr) & 15) != 0) return fail(HSSFSST_EINVAL, "%s: %s is not 16-byte aligned", what, name);
    return 0;
}

// The list of a ragged call (count >= 1): count + 1 host offsets from 0, strictly increasing, no recording over the dense step
// limit, fewer than 2^31 steps in all.  One text for every entry point that takes such a list.
int seg_check_list(const char* what, const int64_t* offsets, int64_t count)
{
    namespace seglayout = hssfsst::seglayout;
    if (!offsets) return fail(HSSFSST_EINVAL, "%s: offsets is NULL", what);
    if (count > kSegMaxBatch) return fail(HSSFSST_EINVAL, "%s: count %lld too large", what, static_cast<long long>(count));
    if (offsets[0] != 0) return fail(HSSFSST_EINVAL, "%s: offsets[0] is %lld, not 0", what, static_cast<long long>(offsets[0]));
    if (const int64_t i = seglayout::first_bad_length(offsets, count, kSegMaxSteps); i >= 0) {
        if (offsets[i + 1] <= offsets[i])
            return fail(HSSFSST_EINVAL, "%s: offsets do not increase at index %lld (offsets[%lld] = %lld, offsets[%lld] = %lld)", what,
                        static_cast<long long>(i + 1), static_cast<long long>(i), static_cast<long long>(offsets[i]),
                        static_cast<long long>(i + 1), static_cast<long long>(offsets[i + 1]));
        return fail(HSSFSST_EINVAL, "%s: recording %lld has %lld steps, over the limit of %lld", what, static_cast<long long>(i),
                    static_cast<long long>(offsets[i + 1] - offsets[i]), static_cast<long long>(kSegMaxSteps));
    }
    if (offsets[count] > 0x7fffffffLL)
        return fail(HSSFSST_EINVAL, "%s: %lld steps in all, over the limit of 2^31 - 1", what, static_cast<long long>(offsets[count]));
    return 0;
}

// The geometry of a call as the forward kernels take it.  Dense: B rows of T steps, Bp padded rows.  Ragged: the list's tables.
void seg_dense_args(int B, int T, int Bp, hssfsst::SegProjArgs* pa, hssfsst::SegRecArgs* ra)
{
    pa->B = ra->B = B;
    pa->T = ra->T = T;
    ra->Bp = Bp;
}
void seg_ragged_args(const SegListTables::Views& t, hssfsst::SegProjArgs* pa, hssfsst::SegRecArgs* ra)
{
    ra->Bp = t.slots;
    pa->slot_off = ra->slot_off = t.off;
    pa->slot_len = ra->slot_len = t.len;
    pa->tile_walk = ra->tile_walk = t.walk;
    ra->tile_base = t.base;                              // (read by the TRAIN kernels only)
    ra->walked = t.walked;
}

// state [2][dir][Bp][Hp] <- (p0, p1): grown, then seeded by seg_pair_init_kernel.  slot_rec: the slots' recordings of a ragged call
// (B: the rows of p0 / p1), NULL for a dense one.
int seg_seed_state(const char* what, hipStream_t st, DevBuf<float>& state, const float* p0, const float* p1, int B, int H, int Bp,
                   const int* slot_rec)
{
    const size_t nstate = static_cast<size_t>(4) * Bp * hssfsst::kSegHp;
    if (int rc = state.grow(nstate)) return rc;
    hipLaunchKernelGGL((slot_rec ? hssfsst::seg_pair_init_kernel<true> : hssfsst::seg_pair_init_kernel<false>),
                       dim3(static_cast<unsigned>((nstate + 255) / 256)), dim3(256), 0, st, p0, p1, state.get(), B, H, Bp, slot_rec);
    return launch_check(what, slot_rec ? "seg_pair_init_kernel<ragged>" : "seg_pair_init_kernel");
}

// One layer, forwards: a launch pair (projection, recurrence) per chunk.  pa / ra come with the call's fields -- the geometry
// (seg_dense_args, seg_ragged_args), x and y, the scratch, H, the scale and, for TRAIN, the stash; the layer's and the chunk's are
// filled in here.  `what`: the entry point, for errors.
template <bool RAGGED, bool TRAIN>
int seg_forward_layer(const char* what, hipStream_t st, const SegLayer& L, hssfsst::SegProjArgs pa, hssfsst::SegRecArgs ra,
                      const std::vector<hssfsst::seglayout::Chunk>& chunks)
{
    pa.F = L.F; pa.Fp = L.Fp; pa.H = ra.H;
    pa.wt = L.d_wt.get(); pa.bias = L.d_bias.get();
    ra.whh = L.d_whh.get();
    for (const hssfsst::seglayout::Chunk& c : chunks) {
        pa.n = ra.n = c.n;
        pa.Tc = ra.Tc = c.Tc;
        if constexpr (RAGGED) {
            pa.s0 = ra.s0 = c.s0;
        } else {
            // the forward direction takes its chunks upwards, the reverse direction the mirrored ones downwards
            pa.t0[0] = ra.t0[0] = c.s0;
            pa.t0[1] = ra.t0[1] = ra.T - c.s0 - c.n;
        }
        hipLaunchKernelGGL(hssfsst::seg_proj_kernel<RAGGED>, dim3(4 * hssfsst::kSegHp / 64, static_cast<unsigned>(c.tiles * ((c.n + 7) / 8)), 2),
                           dim3(256), 0, st, pa);
        if (int rc = launch_check(what, RAGGED ? "seg_proj_kernel<ragged>" : "seg_proj_kernel")) return rc;
        hipLaunchKernelGGL((hssfsst::seg_rec_kernel<RAGGED, TRAIN>), dim3(static_cast<unsigned>(c.tiles), 2), dim3(64 * hssfsst::kSegWaves), 0, st, ra);
        if (int rc = launch_check(what, RAGGED ? (TRAIN ? "seg_rec_kernel<ragged, train>" : "seg_rec_kernel<ragged>")
                                               : (TRAIN ? "seg_rec_kernel<train>" : "seg_rec_kernel"))) return rc;
    }
    return 0;
}

// The two layers of an inference exec and its head: layer 2 reads layer 1's output rectified and starts from its final state.
// pa / ra: the call's geometry; rows: B T, or the list's steps.
template <bool RAGGED>
int seg_run_layers(hssfsst_segmenter* p, hipStream_t st, const void* feats, int feats_dtype, hssfsst::SegProjArgs pa, hssfsst::SegRecArgs ra,
                   const std::vector<hssfsst::seglayout::Chunk>& chunks, long long rows, float* logp)
{
    ra.pre = pa.pre = p->d_pre.get();
    ra.state = p->d_state.get();
    ra.H = p->H;
    pa.x = feats; pa.x_dtype = feats_dtype; pa.relu = 0;
    ra.y = p->d_y1.get(); ra.inv_scale = p->layer[0].inv_scale;
    if (int rc = seg_forward_layer<RAGGED, false>("segmenter_exec", st, p->layer[0], pa, ra, chunks)) return rc;
    pa.x = p->d_y1.get(); pa.x_dtype = HSSFSST_DTYPE_F32; pa.relu = 1;
    ra.y = p->d_y2.get(); ra.inv_scale = p->layer[1].inv_scale;
    if (int rc = seg_forward_layer<RAGGED, false>("segmenter_exec", st, p->layer[1], pa, ra, chunks)) return rc;
    hipLaunchKernelGGL(hssfsst::seg_head_kernel, dim3(static_cast<unsigned>((rows + 3) / 4)), dim3(256), 0, st, p->d_y2.get(), p->d_lin.get(),
                       p->d_lin.get() + static_cast<size_t>(8) * p->H, logp, rows, 2 * p->H);
    return launch_check("segmenter_exec", "seg_head_kernel");
}

// the scratch of an inference exec, in elements: one chunk's projection and the two layers' outputs of ylen elements each
int seg_grow_scratch(hssfsst_segmenter* p, size_t pre, size_t ylen)
{
    if (int rc = p->d_pre.grow(pre)) return rc;
    if (int rc = p->d_y1.grow(ylen)) return rc;
    return p->d_y2.grow(ylen);
}

}  // namespace

extern "C" {

int hssfsst_segmenter_create(hssfsst_segmenter** out, int device, int input_size, int hidden, const float* const* lstm_1,
                             const float* const* lstm_2, const float* linear_weight, const float* linear_bias)
{
    if (!out) return fail(HSSFSST_EINVAL, "segmenter_create: out is NULL");
    *out = nullptr;
    if (input_size < 1 || hidden < 1 || device < 0 || !lstm_1 || !lstm_2 || !linear_weight || !linear_bias)
        return fail(HSSFSST_EINVAL, "segmenter_create: bad argument (device=%d input_size=%d hidden=%d, or a NULL array)", device, input_size, hidden);
    for (int i = 0; i < 8; ++i)
        if (!lstm_1[i] || !lstm_2[i]) return fail(HSSFSST_EINVAL, "segmenter_create: bad argument (weight array %d of a layer is NULL)", i);
    if (hidden > hssfsst::kSegHp)
        return fail(HSSFSST_EUNSUPPORTED, "segmenter_create: hidden sizes above %d are not supported (hidden=%d)", hssfsst::kSegHp, hidden);
    if (input_size > (1 << 20)) return fail(HSSFSST_EUNSUPPORTED, "segmenter_create: input sizes above 2^20 are not supported (input_size=%d)", input_size);
    if (int rc = check_device("segmenter_create", device)) return rc;
    DEVICE_SCOPE(device);
    std::unique_ptr<hssfsst_segmenter> p(new (std::nothrow) hssfsst_segmenter());
    if (!p) return fail(HSSFSST_ENOMEM, "segmenter_create: host allocation failed");
    p->device = device; p->F = input_size; p->H = hidden;
    try {
        if (int rc = seg_upload_layer(p->layer[0], input_size, hidden, lstm_1)) return rc;
        if (int rc = seg_upload_layer(p->layer[1], 2 * hidden, hidden, lstm_2)) return rc;
        std::vector<float> lin(static_cast<size_t>(8) * hidden + 4);
        std::memcpy(lin.data(), linear_weight, static_cast<size_t>(8) * hidden * sizeof(float));
        std::memcpy(lin.data() + static_cast<size_t>(8) * hidden, linear_bias, 4 * sizeof(float));
        if (int rc = p->d_lin.upload(lin.data(), lin.size())) return rc;
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "segmenter_create: out of host memory");
    }
    *out = p.release();
    return 0;
}

int hssfsst_segmenter_destroy(hssfsst_segmenter* p)
{
    if (!p) return 0;
    DeviceGuard device_guard_(p->device);
    delete p;                                            // (the buffers free themselves)
    return 0;
}

int hssfsst_segmenter_info(const hssfsst_segmenter* p, int* input_size, int* hidden, int* max_hidden, int* device)
{
    if (max_hidden) *max_hidden = hssfsst::kSegHp;       // (a property of the library: answered for a NULL plan too)
    if (!p) return fail(HSSFSST_EINVAL, "segmenter_info: plan is NULL");
    if (input_size) *input_size = p->F;
    if (hidden) *hidden = p->H;
    if (device) *device = p->device;
    return 0;
}

int hssfsst_segmenter_exec(hssfsst_segmenter* p, const void* feats, int feats_dtype, int64_t batch, int64_t steps, const float* h0,
                           const float* c0, float* logp, void* stream)
{
    if (!p || !feats || !h0 || !c0 || !logp || batch < 1 || steps < 1)
        return fail(HSSFSST_EINVAL, "segmenter_exec: bad argument (batch=%lld steps=%lld, or a NULL pointer)", static_cast<long long>(batch),
                    static_cast<long long>(steps));
    if (int rc = seg_check_dtype("segmenter_exec", feats_dtype)) return rc;
    if (batch > kSegMaxBatch || steps > kSegMaxSteps)
        return fail(HSSFSST_EINVAL, "segmenter_exec: batch %lld or steps %lld too large", static_cast<long long>(batch), static_cast<long long>(steps));
    if (int rc = seg_check_aligned16("segmenter_exec", "logp", logp)) return rc;
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = static_cast<int>(batch), T = static_cast<int>(steps), H = p->H;
    const int nbt = (B + hssfsst::kSegRows - 1) / hssfsst::kSegRows, Bp = nbt * hssfsst::kSegRows;
    std::vector<hssfsst::seglayout::Chunk> chunks;
    try {
        chunks = hssfsst::seglayout::dense_chunks(T, nbt, kSegTileStepBytes, hssfsst::seglayout::kSegPreBytes);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "segmenter_exec: out of host memory");
    }
    if (int rc = seg_grow_scratch(p, hssfsst::seglayout::pre_floats(chunks, kSegTileStepBytes), static_cast<size_t>(B) * T * 2 * H)) return rc;
    if (int rc = seg_seed_state("segmenter_exec", st, p->d_state, h0, c0, B, H, Bp, nullptr)) return rc;
    hssfsst::SegProjArgs pa{};
    hssfsst::SegRecArgs ra{};
    seg_dense_args(B, T, Bp, &pa, &ra);
    return seg_run_layers<false>(p, st, feats, feats_dtype, pa, ra, chunks, static_cast<long long>(B) * T, logp);
}

int hssfsst_segmenter_exec_ragged(hssfsst_segmenter* p, const void* feats, int feats_dtype, const int64_t* offsets, int64_t count,
                                  const float* h0, const float* c0, int state_rows, float* logp, void* stream)
{
    namespace seglayout = hssfsst::seglayout;
    // the list first: what is wrong with it is said before the plan is looked at
    if (count < 0) return fail(HSSFSST_EINVAL, "segmenter_exec_ragged: count %lld is negative", static_cast<long long>(count));
    if (count == 0) return 0;
    if (int rc = seg_check_list("segmenter_exec_ragged", offsets, count)) return rc;
    if (state_rows != 1 && state_rows != count)
        return fail(HSSFSST_EINVAL, "segmenter_exec_ragged: state_rows %d is neither 1 nor count %lld", state_rows, static_cast<long long>(count));
    if (int rc = seg_check_dtype("segmenter_exec_ragged", feats_dtype)) return rc;
    if (!p || !feats || !h0 || !c0 || !logp)
        return fail(HSSFSST_EINVAL, "segmenter_exec_ragged: bad argument (%s is NULL)",
                    !p ? "plan" : !feats ? "feats" : !h0 ? "h0" : !c0 ? "c0" : "logp");
    if (int rc = seg_check_aligned16("segmenter_exec_ragged", "logp", logp)) return rc;
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int H = p->H;
    const seglayout::Layout& lay = p->list.lay;
    SegListTables::Views t{};
    std::vector<seglayout::Chunk> chunks;
    try {
        if (int rc = p->list.acquire(offsets, count, st, &t)) return rc;
        const int mib = seg_ragged_pre_mib();                         // (A-B switch of tools/segmenter_ragged_bench.py: same bits)
        chunks = seglayout::ragged_chunks(lay, kSegTileStepBytes, mib > 0 ? static_cast<size_t>(mib) << 20 : seglayout::kSegPreBytes);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "segmenter_exec_ragged: out of host memory");
    }
    if (int rc = seg_grow_scratch(p, seglayout::pre_floats(chunks, kSegTileStepBytes), static_cast<size_t>(lay.total) * 2 * H)) return rc;
    if (int rc = seg_seed_state("segmenter_exec", st, p->d_state, h0, c0, state_rows, H, t.slots, t.rec)) return rc;
    hssfsst::SegProjArgs pa{};
    hssfsst::SegRecArgs ra{};
    seg_ragged_args(t, &pa, &ra);
    return seg_run_layers<true>(p, st, feats, feats_dtype, pa, ra, chunks, lay.total, logp);
}

}  // extern "C"

// One trainable BiLSTM layer (hssfsst.h: hssfsst_bilstm_create): the tables of its current weights, packed on the device by
// hssfsst_bilstm_set_weights (csrc/segmenter_train.hpp), and the scratch of its forward and backward calls.
struct hssfsst_bilstm {
    int device = -1;
    int H = 0;
    bool packed = false;
    SegLayer layer;                                      // the forward tables, of the weights set last
    DevBuf<hssfsst::seg_b8> d_bwd;                       // backward stream: W_hh, split bf16, as the B operand of dG . W_hh
    DevBuf<float> d_scale;                               // {wscale, inv_scale}: made and read on the device only
    DevBuf<float> d_pre;                                 // one chunk's input projection
    DevBuf<float> d_state;                               // forward [h, c][dir][Bp][Hp]; backward [dh_rec, dc][dir][Bp][Hp]
    SegListTables list{"bilstm_ragged"};                 // hssfsst_bilstm_*_ragged: kept while the next call has the same offsets
};

namespace {

int bilstm_check_shape(const char* what, int64_t batch, int64_t steps)
{
    if (batch < 1 || steps < 1)
        return fail(HSSFSST_EINVAL, "%s: bad argument (batch=%lld steps=%lld)", what, static_cast<long long>(batch), static_cast<long long>(steps));
    if (batch > kSegMaxBatch || steps > kSegMaxSteps)
        return fail(HSSFSST_EINVAL, "%s: batch %lld or steps %lld too large", what, static_cast<long long>(batch), static_cast<long long>(steps));
    return 0;
}

// out0, out1 (2, B, H) <- the state seg_seed_state made, after the launches chained through it; slot_rec as there
int bilstm_state_out(const char* what, hipStream_t st, const hssfsst_bilstm* p, float* out0, float* out1, int B, int Bp, const int* slot_rec)
{
    const size_t nout = static_cast<size_t>(4) * (slot_rec ? Bp : B) * p->H;
    hipLaunchKernelGGL((slot_rec ? hssfsst::seg_pair_out_kernel<true> : hssfsst::seg_pair_out_kernel<false>),
                       dim3(static_cast<unsigned>((nout + 255) / 256)), dim3(256), 0, st, p->d_state.get(), out0, out1, B, p->H, Bp, slot_rec);
    return launch_check(what, slot_rec ? "seg_pair_out_kernel<ragged>" : "seg_pair_out_kernel");
}

// A training forward: (h0, c0) in, the layer over the chunks with its stash, (hn, cn) out.  pa / ra: the call's geometry
// (seg_dense_args, seg_ragged_args); B: the rows of the states; slot_rec as in seg_seed_state.
template <bool RAGGED>
int bilstm_forward(const char* what, hssfsst_bilstm* p, hipStream_t st, const float* x, const float* h0, const float* c0, float* y, float* hn,
                   float* cn, float* stash, int B, const int* slot_rec, hssfsst::SegProjArgs pa, hssfsst::SegRecArgs ra,
                   const std::vector<hssfsst::seglayout::Chunk>& chunks)
{
    if (int rc = p->d_pre.grow(hssfsst::seglayout::pre_floats(chunks, kSegTileStepBytes))) return rc;
    if (int rc = seg_seed_state(what, st, p->d_state, h0, c0, B, p->H, ra.Bp, slot_rec)) return rc;
    pa.x = x; pa.x_dtype = HSSFSST_DTYPE_F32; pa.relu = 0;
    ra.pre = pa.pre = p->d_pre.get();
    ra.state = p->d_state.get(); ra.y = y; ra.H = p->H;
    ra.stash = stash; ra.inv_scale_dev = p->d_scale.get() + 1;
    if (int rc = seg_forward_layer<RAGGED, true>(what, st, p->layer, pa, ra, chunks)) return rc;
    return bilstm_state_out(what, st, p, hn, cn, B, ra.Bp, slot_rec);
}

// what both backwards give seg_bwd_rec_kernel; the state is seeded by then
hssfsst::SegBwdArgs bilstm_bwd_args(const hssfsst_bilstm* p, const float* stash, const float* c0, const float* dy, float* dgates, int B, int Bp)
{
    hssfsst::SegBwdArgs a{};
    a.stash = stash; a.c0 = c0; a.dy = dy; a.wbwd = p->d_bwd.get(); a.state = p->d_state.get(); a.dgates = dgates;
    a.B = B; a.H = p->H; a.Bp = Bp;
    return a;
}

}  // namespace

extern "C" {

int hssfsst_bilstm_create(hssfsst_bilstm** out, int device, int input_size, int hidden)
{
    if (!out) return fail(HSSFSST_EINVAL, "bilstm_create: out is NULL");
    *out = nullptr;
    if (input_size < 1 || hidden < 1 || device < 0)
        return fail(HSSFSST_EINVAL, "bilstm_create: bad argument (device=%d input_size=%d hidden=%d)", device, input_size, hidden);
    if (hidden > hssfsst::kSegHp)
        return fail(HSSFSST_EUNSUPPORTED, "bilstm_create: hidden sizes above %d are not supported (hidden=%d)", hssfsst::kSegHp, hidden);
    if (input_size > (1 << 20)) return fail(HSSFSST_EUNSUPPORTED, "bilstm_create: input sizes above 2^20 are not supported (input_size=%d)", input_size);
    if (int rc = check_device("bilstm_create", device)) return rc;
    DEVICE_SCOPE(device);
    std::unique_ptr<hssfsst_bilstm> p(new (std::nothrow) hssfsst_bilstm());
    if (!p) return fail(HSSFSST_ENOMEM, "bilstm_create: host allocation failed");
    p->device = device; p->H = hidden;
    SegLayer& L = p->layer;
    L.F = input_size;
    L.Fp = (input_size + 31) / 32 * 32;
    namespace sl = hssfsst::seglayout;
    if (int rc = L.d_wt.grow(static_cast<size_t>(2) * L.Fp * sl::kGateCols)) return rc;
    if (int rc = L.d_bias.grow(static_cast<size_t>(2) * sl::kGateCols)) return rc;
    if (int rc = L.d_whh.grow(static_cast<size_t>(sl::kWtStreamHalves / 8))) return rc;
    if (int rc = p->d_bwd.grow(static_cast<size_t>(sl::kBwdStreamHalves / 8))) return rc;
    if (int rc = p->d_scale.grow(2)) return rc;
    *out = p.release();
    return 0;
}

int hssfsst_bilstm_destroy(hssfsst_bilstm* p)
{
    if (!p) return 0;
    DeviceGuard device_guard_(p->device);
    delete p;
    return 0;
}

int hssfsst_bilstm_set_weights(hssfsst_bilstm* p, const float* const* weights, void* stream)
{
    if (!p || !weights) return fail(HSSFSST_EINVAL, "bilstm_set_weights: bad argument (%s is NULL)", !p ? "plan" : "weights");
    for (int i = 0; i < 8; ++i)
        if (!weights[i]) return fail(HSSFSST_EINVAL, "bilstm_set_weights: bad argument (weight array %d is NULL)", i);
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    namespace sl = hssfsst::seglayout;
    hssfsst::SegPackArgs a{};
    for (int i = 0; i < 8; ++i) a.src[i] = weights[i];
    const SegLayer& L = p->layer;
    a.F = L.F; a.Fp = L.Fp; a.H = p->H;
    a.scale = p->d_scale.get(); a.wt = L.d_wt.get(); a.bias = L.d_bias.get();
    a.whh = reinterpret_cast<_Float16*>(L.d_whh.get());
    a.bwd = reinterpret_cast<__bf16*>(p->d_bwd.get());
    hipLaunchKernelGGL(hssfsst::seg_pack_scale_kernel, dim3(1), dim3(1024), 0, st, a);
    if (int rc = launch_check("bilstm_set_weights", "seg_pack_scale_kernel")) return rc;
    const long long most = std::max<long long>(static_cast<long long>(2) * L.Fp * sl::kGateCols, std::max(sl::kWtStreamHalves, sl::kBwdStreamHalves));
    hipLaunchKernelGGL(hssfsst::seg_pack_kernel, dim3(static_cast<unsigned>((most + 255) / 256)), dim3(256), 0, st, a);
    if (int rc = launch_check("bilstm_set_weights", "seg_pack_kernel")) return rc;
    p->packed = true;
    return 0;
}

int hssfsst_bilstm_stash_floats(const hssfsst_bilstm* p, int64_t batch, int64_t steps, int64_t* floats)
{
    if (!floats) return fail(HSSFSST_EINVAL, "bilstm_stash_floats: floats is NULL");
    *floats = 0;
    (void)p;                                             // (every hidden size runs on the padded geometry: answered for a NULL plan too)
    if (int rc = bilstm_check_shape("bilstm_stash_floats", batch, steps)) return rc;
    *floats = hssfsst::seglayout::stash_floats(batch, steps);
    return 0;
}

int hssfsst_bilstm_forward(hssfsst_bilstm* p, const float* x, int64_t batch, int64_t steps, const float* h0, const float* c0, float* y,
                           float* hn, float* cn, float* stash, void* stream)
{
    if (!p) return fail(HSSFSST_EINVAL, "bilstm_forward: plan is NULL");
    if (int rc = bilstm_check_shape("bilstm_forward", batch, steps)) return rc;
    if (!x || !h0 || !c0 || !y || !hn || !cn || !stash)
        return fail(HSSFSST_EINVAL, "bilstm_forward: bad argument (%s is NULL)",
                    !x ? "x" : !h0 ? "h0" : !c0 ? "c0" : !y ? "y" : !hn ? "hn" : !cn ? "cn" : "stash");
    if (int rc = seg_check_aligned16("bilstm_forward", "stash", stash)) return rc;
    if (!p->packed) return fail(HSSFSST_EINVAL, "bilstm_forward: no weights yet (call hssfsst_bilstm_set_weights first)");
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = static_cast<int>(batch), T = static_cast<int>(steps);
    const int nbt = (B + hssfsst::kSegRows - 1) / hssfsst::kSegRows, Bp = nbt * hssfsst::kSegRows;
    std::vector<hssfsst::seglayout::Chunk> chunks;
    try {
        chunks = hssfsst::seglayout::dense_chunks(T, nbt, kSegTileStepBytes, hssfsst::seglayout::kSegPreBytes);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "bilstm_forward: out of host memory");
    }
    hssfsst::SegProjArgs pa{};
    hssfsst::SegRecArgs ra{};
    seg_dense_args(B, T, Bp, &pa, &ra);
    return bilstm_forward<false>("bilstm_forward", p, st, x, h0, c0, y, hn, cn, stash, B, nullptr, pa, ra, chunks);
}

int hssfsst_bilstm_backward(hssfsst_bilstm* p, const float* stash, const float* c0, const float* dy, const float* dhn, const float* dcn,
                            int64_t batch, int64_t steps, float* dgates, float* dh0, float* dc0, void* stream)
{
    if (!p) return fail(HSSFSST_EINVAL, "bilstm_backward: plan is NULL");
    if (int rc = bilstm_check_shape("bilstm_backward", batch, steps)) return rc;
    if (!stash || !c0 || !dy || !dgates || !dh0 || !dc0)
        return fail(HSSFSST_EINVAL, "bilstm_backward: bad argument (%s is NULL)",
                    !stash ? "stash" : !c0 ? "c0" : !dy ? "dy" : !dgates ? "dgates" : !dh0 ? "dh0" : "dc0");
    if (int rc = seg_check_aligned16("bilstm_backward", "stash", stash)) return rc;
    if (!p->packed) return fail(HSSFSST_EINVAL, "bilstm_backward: no weights yet (call hssfsst_bilstm_set_weights first)");
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = static_cast<int>(batch), T = static_cast<int>(steps);
    const int nbt = (B + hssfsst::kSegRows - 1) / hssfsst::kSegRows, Bp = nbt * hssfsst::kSegRows;
    if (int rc = seg_seed_state("bilstm_backward", st, p->d_state, dhn, dcn, B, p->H, Bp, nullptr)) return rc;
    hssfsst::SegBwdArgs a = bilstm_bwd_args(p, stash, c0, dy, dgates, B, Bp);
    a.T = T;
    // at most kSegMaxChunk steps per launch, chained through the carried (dh_rec, dc)
    for (int s0 = 0; s0 < T; s0 += hssfsst::seglayout::kSegMaxChunk) {
        a.s0 = s0;
        a.n = std::min(hssfsst::seglayout::kSegMaxChunk, T - s0);
        hipLaunchKernelGGL(hssfsst::seg_bwd_rec_kernel<false>, dim3(static_cast<unsigned>(nbt), 2), dim3(64 * hssfsst::kSegWaves), 0, st, a);
        if (int rc = launch_check("bilstm_backward", "seg_bwd_rec_kernel")) return rc;
    }
    return bilstm_state_out("bilstm_backward", st, p, dh0, dc0, B, Bp, nullptr);
}

int hssfsst_bilstm_stash_floats_ragged(const hssfsst_bilstm* p, const int64_t* offsets, int64_t count, int64_t* floats)
{
    if (!floats) return fail(HSSFSST_EINVAL, "bilstm_stash_floats_ragged: floats is NULL");
    *floats = 0;
    (void)p;                                             // (as hssfsst_bilstm_stash_floats: answered for a NULL plan too)
    if (count < 0) return fail(HSSFSST_EINVAL, "bilstm_stash_floats_ragged: count %lld is negative", static_cast<long long>(count));
    if (count == 0) return 0;
    if (int rc = seg_check_list("bilstm_stash_floats_ragged", offsets, count)) return rc;
    try {
        hssfsst::seglayout::Layout lay;
        hssfsst::seglayout::build(offsets, count, lay);
        *floats = hssfsst::seglayout::stash_floats_ragged(lay);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "bilstm_stash_floats_ragged: out of host memory");
    }
    return 0;
}

int hssfsst_bilstm_forward_ragged(hssfsst_bilstm* p, const float* x, const int64_t* offsets, int64_t count, const float* h0, const float* c0,
                                  float* y, float* hn, float* cn, float* stash, void* stream)
{
    namespace seglayout = hssfsst::seglayout;
    // the list first: what is wrong with it is said before the plan is looked at
    if (count < 0) return fail(HSSFSST_EINVAL, "bilstm_forward_ragged: count %lld is negative", static_cast<long long>(count));
    if (count == 0) return 0;
    if (int rc = seg_check_list("bilstm_forward_ragged", offsets, count)) return rc;
    if (!p) return fail(HSSFSST_EINVAL, "bilstm_forward_ragged: plan is NULL");
    if (!x || !h0 || !c0 || !y || !hn || !cn || !stash)
        return fail(HSSFSST_EINVAL, "bilstm_forward_ragged: bad argument (%s is NULL)",
                    !x ? "x" : !h0 ? "h0" : !c0 ? "c0" : !y ? "y" : !hn ? "hn" : !cn ? "cn" : "stash");
    if (int rc = seg_check_aligned16("bilstm_forward_ragged", "stash", stash)) return rc;
    if (!p->packed) return fail(HSSFSST_EINVAL, "bilstm_forward_ragged: no weights yet (call hssfsst_bilstm_set_weights first)");
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    SegListTables::Views t{};
    std::vector<seglayout::Chunk> chunks;
    try {
        if (int rc = p->list.acquire(offsets, count, st, &t)) return rc;
        chunks = seglayout::ragged_chunks(p->list.lay, kSegTileStepBytes, seglayout::kSegPreBytes);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "bilstm_forward_ragged: out of host memory");
    }
    hssfsst::SegProjArgs pa{};
    hssfsst::SegRecArgs ra{};
    seg_ragged_args(t, &pa, &ra);
    return bilstm_forward<true>("bilstm_forward_ragged", p, st, x, h0, c0, y, hn, cn, stash, static_cast<int>(count), t.rec, pa, ra, chunks);
}

int hssfsst_bilstm_backward_ragged(hssfsst_bilstm* p, const float* stash, const float* c0, const float* dy, const float* dhn, const float* dcn,
                                   const int64_t* offsets, int64_t count, float* dgates, float* dh0, float* dc0, void* stream)
{
    namespace seglayout = hssfsst::seglayout;
    if (count < 0) return fail(HSSFSST_EINVAL, "bilstm_backward_ragged: count %lld is negative", static_cast<long long>(count));
    if (count == 0) return 0;
    if (int rc = seg_check_list("bilstm_backward_ragged", offsets, count)) return rc;
    if (!p) return fail(HSSFSST_EINVAL, "bilstm_backward_ragged: plan is NULL");
    if (!stash || !c0 || !dy || !dgates || !dh0 || !dc0)
        return fail(HSSFSST_EINVAL, "bilstm_backward_ragged: bad argument (%s is NULL)",
                    !stash ? "stash" : !c0 ? "c0" : !dy ? "dy" : !dgates ? "dgates" : !dh0 ? "dh0" : "dc0");
    if (int rc = seg_check_aligned16("bilstm_backward_ragged", "stash", stash)) return rc;
    if (!p->packed) return fail(HSSFSST_EINVAL, "bilstm_backward_ragged: no weights yet (call hssfsst_bilstm_set_weights first)");
    DEVICE_SCOPE(p->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    SegListTables::Views t{};
    std::vector<seglayout::BwdChunk> chunks;
    try {
        if (int rc = p->list.acquire(offsets, count, st, &t)) return rc;
        chunks = seglayout::ragged_bwd_chunks(p->list.lay);
    } catch (const std::bad_alloc&) {
        return fail(HSSFSST_ENOMEM, "bilstm_backward_ragged: out of host memory");
    }
    const int B = static_cast<int>(count);
    if (int rc = seg_seed_state("bilstm_backward_ragged", st, p->d_state, dhn, dcn, B, p->H, t.slots, t.rec)) return rc;
    hssfsst::SegBwdArgs a = bilstm_bwd_args(p, stash, c0, dy, dgates, B, t.slots);
    a.slot_off = t.off; a.slot_len = t.len; a.slot_rec = t.rec; a.tile_walk = t.walk; a.tile_base = t.base;
    a.walked = t.walked; a.total = p->list.lay.total;
    // highest steps first, at most kSegMaxChunk per launch, chained through the carried (dh_rec, dc); a tile joins at its last step
    for (const seglayout::BwdChunk& c : chunks) {
        a.s0 = c.s0;
        a.n = c.n;
        hipLaunchKernelGGL(hssfsst::seg_bwd_rec_kernel<true>, dim3(static_cast<unsigned>(c.tiles), 2), dim3(64 * hssfsst::kSegWaves), 0, st, a);
        if (int rc = launch_check("bilstm_backward_ragged", "seg_bwd_rec_kernel<ragged>")) return rc;
    }
    return bilstm_state_out("bilstm_backward_ragged", st, p, dh0, dc0, B, t.slots, t.rec);
}

}  // extern "C"
