// sequence.hip -- the sequence-model entry points over lists of log-probs: Viterbi and forward-backward, with and without
// duration scores, the duration counts, scoring and window stitching.  All stateless.  C ABI: include/hssfsst.h.
#include "host_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "decode_durations_layout.hpp"
#include "decode_layout.hpp"
#include "sequence_args.hpp"
#include "segmenter_decode.hpp"
#include "segmenter_decode_durations.hpp"
#include "posterior_layout.hpp"
#include "segmenter_posteriors.hpp"
#include "segmenter_duration_posteriors.hpp"
#include "segmenter_duration_counts.hpp"
#include "score_layout.hpp"
#include "segmenter_score.hpp"
#include "stitch_layout.hpp"
#include "segmenter_stitch.hpp"

using namespace hssfsst::host;

// What the sequence-model entry points (hssfsst_decode_states .. hssfsst_posteriors_durations_counts) share: the decisions of
// csrc/sequence_args.hpp put into words -- every text stands here, once -- and the loop over a list's launches.  Each entry
// calls the checks in its own order: that order is which of two errors a caller sees.
namespace {

namespace seqargs = hssfsst::seqargs;

int seq_check_list(const char* entry, const int64_t* offsets, int64_t count, int64_t max_steps)
{
    using Fault = seqargs::ListFault;
    const seqargs::ListFinding f = seqargs::check_list(offsets, count, max_steps);
    const long long i = f.index, limit = max_steps;
    if (f.fault == Fault::kNone) return 0;
    if (f.fault == Fault::kFirstNotZero) return fail(HSSFSST_EINVAL, "%s: offsets[0] is %lld, not 0", entry, static_cast<long long>(offsets[0]));
    if (f.fault == Fault::kTooManySteps)
        return fail(HSSFSST_EUNSUPPORTED, "%s: %lld steps in all, over the limit of 2^31 - 1", entry, static_cast<long long>(offsets[i]));
    const long long from = offsets[i], to = offsets[i + 1];
    if (f.fault == Fault::kNotIncreasing)
        return fail(HSSFSST_EINVAL, "%s: offsets do not increase at index %lld (offsets[%lld] = %lld, offsets[%lld] = %lld)", entry, i + 1, i,
                    from, i + 1, to);
    return fail(HSSFSST_EUNSUPPORTED, "%s: recording %lld has %lld steps, over the limit of %lld", entry, i, to - from, limit);
}

int seq_check_nonnull(const char* entry, std::initializer_list<seqargs::NamedPointer> required)
{
    if (const char* name = seqargs::first_null(required)) return fail(HSSFSST_EINVAL, "%s: bad argument (%s is NULL)", entry, name);
    return 0;
}

int seq_check_aligned(const char* entry, std::initializer_list<seqargs::NamedPointer> pointers)
{
    const seqargs::NamedPointer p = seqargs::first_misaligned(pointers);
    if (p.name) return fail(HSSFSST_EINVAL, "%s: %s is not %u-byte aligned", entry, p.name, p.alignment);
    return 0;
}

int seq_check_duration_table(const char* entry, const char* name, const float* table, int D)
{
    const seqargs::TableFinding f = seqargs::check_duration_table(table, D);
    if (f.fault == seqargs::TableFault::kNaN)
        return fail(HSSFSST_EINVAL, "%s: %s[%d][%d] is NaN (duration %d)", entry, name, f.row, f.column, f.column + 1);
    if (f.fault == seqargs::TableFault::kDeadRow)
        return fail(HSSFSST_EINVAL, "%s: row %d of %s is all -inf: state %d has no allowed duration", entry, f.row, name, f.row);
    return 0;
}

// (transitions, initial) and, with `durations`, the host tables of the explicit-duration model, whose diagonal is not read: the
// NaNs of the first two, then the two duration tables, then what the first two leave of a path.
int seq_check_model(const char* entry, const float* transitions, const float* initial, const float* durations = nullptr,
                    const float* edge = nullptr, int D = 0)
{
    const seqargs::ModelFinding f = seqargs::check_model(transitions, initial, durations != nullptr);
    if (f.nan_at >= 16) return fail(HSSFSST_EINVAL, "%s: initial[%d] is NaN", entry, f.nan_at - 16);
    if (f.nan_at >= 0) return fail(HSSFSST_EINVAL, "%s: transitions[%d][%d] is NaN", entry, f.nan_at / 4, f.nan_at % 4);
    if (durations) {
        if (int rc = seq_check_duration_table(entry, "durations", durations, D)) return rc;
        if (int rc = seq_check_duration_table(entry, "edge", edge, D)) return rc;
    }
    if (f.dead_row >= 0)
        return fail(HSSFSST_EINVAL,
                    durations ? "%s: row %d of transitions has no finite off-diagonal entry: state %d has no successor"
                              : "%s: row %d of transitions is all -inf: state %d has no successor", entry, f.dead_row, f.dead_row);
    if (f.no_start) return fail(HSSFSST_EINVAL, "%s: initial is all -inf: no state to start in", entry);
    return 0;
}

// The recordings of a list, `batch` per launch (the kernel's k*Batch: their offsets travel as kernel arguments).  For the
// recordings r0 .. r0 + nrec of each launch args.off[] is filled, launch(r0, nrec) enqueues `kernel` -- after setting args.rec0,
// where the kernel has one -- and the launch is checked.
template <class Args, class Launch>
int seq_for_each_batch(const char* entry, const char* kernel, const int64_t* offsets, int64_t count, int batch, Args& args, Launch launch)
{
    for (int64_t r0 = 0; r0 < count; r0 += batch) {
        const int nrec = static_cast<int>(std::min<int64_t>(batch, count - r0));
        for (int i = 0; i <= nrec; ++i) args.off[i] = offsets[r0 + i];
        launch(r0, nrec);
        if (int rc = launch_check(entry, kernel)) return rc;
    }
    return 0;
}

}  // namespace

// Viterbi decoding of log-probs into state sequences (hssfsst.h: hssfsst_decode_states; csrc/segmenter_decode.hpp).  Stateless: the
// quantised transitions and the launch's offsets travel as kernel arguments, kDecodeBatch recordings per launch.
extern "C" {

int hssfsst_decode_info(int* segment_steps, int64_t* max_steps)
{
    if (segment_steps) *segment_steps = hssfsst::declayout::kSegSteps;
    if (max_steps) *max_steps = hssfsst::declayout::kMaxSteps;
    return 0;
}

int hssfsst_decode_states(const float* logp, const int64_t* offsets, int64_t count, const float* transitions, const float* initial,
                          uint8_t* states, int64_t* scores, int device, void* stream)
{
    namespace dl = hssfsst::declayout;
    constexpr const char* kEntry = "decode_states";
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"logp", logp}, {"offsets", offsets}, {"transitions", transitions}, {"initial", initial},
                                            {"states", states}})) return rc;
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (int rc = seq_check_aligned(kEntry, {{"logp", logp, 16}})) return rc;
    if (int rc = seq_check_model(kEntry, transitions, initial)) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, dl::kMaxSteps)) return rc;
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hssfsst::DecodeArgs args{};
    args.A = dl::quantise_transitions(transitions);
    args.pi = dl::quantise4(initial);
    return seq_for_each_batch(kEntry, "seg_decode_kernel", offsets, count, hssfsst::kDecodeBatch, args, [&](int64_t r0, int nrec) {
        hipLaunchKernelGGL(hssfsst::seg_decode_kernel, dim3(static_cast<unsigned>(nrec)), dim3(dl::kLanes), 0, st, logp, states,
                           scores ? reinterpret_cast<long long*>(scores) + r0 : nullptr, args);
    });
}

}  // extern "C"

// Explicit-duration Viterbi decoding (hssfsst.h: hssfsst_decode_durations; csrc/segmenter_decode_durations.hpp).  Stateless: the
// quantised transitions and the launch's offsets travel as kernel arguments, kDurDecodeBatch recordings per launch; the two
// duration tables travel as the arguments of fill launches into the head of the caller's workspace, so nothing is copied from
// host memory and every launch is stream-ordered.
extern "C" {

int hssfsst_decode_durations_info(int* max_duration, int64_t* max_steps, int64_t* workspace_bytes_per_step)
{
    if (max_duration) *max_duration = hssfsst::durlayout::kMaxDuration;
    if (max_steps) *max_steps = hssfsst::durlayout::kMaxSteps;
    if (workspace_bytes_per_step) *workspace_bytes_per_step = hssfsst::durlayout::kWorkspaceBytesPerStep;
    return 0;
}

int hssfsst_decode_durations(const float* logp, const int64_t* offsets, int64_t count, const float* transitions, const float* initial,
                             const float* durations, const float* edge, int max_duration, uint8_t* states, int64_t* scores,
                             void* workspace, int64_t workspace_bytes, int device, void* stream)
{
    namespace dl = hssfsst::declayout;
    namespace ul = hssfsst::durlayout;
    constexpr const char* kEntry = "decode_durations";
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"logp", logp}, {"offsets", offsets}, {"transitions", transitions}, {"initial", initial},
                                            {"durations", durations}, {"edge", edge}, {"states", states}, {"workspace", workspace}}))
        return rc;
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (max_duration < 1 || max_duration > ul::kMaxDuration)
        return fail(HSSFSST_EINVAL, "%s: max_duration %d is outside 1..%d", kEntry, max_duration, ul::kMaxDuration);
    const int D = max_duration;
    if (int rc = seq_check_aligned(kEntry, {{"logp", logp, 16}, {"workspace", workspace, 16}})) return rc;
    if (int rc = seq_check_model(kEntry, transitions, initial, durations, edge, D)) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, ul::kMaxSteps)) return rc;
    const int64_t need = ul::kWorkspaceBytesPerStep * ul::workspace_steps(offsets[count], D);
    if (workspace_bytes < need)
        return fail(HSSFSST_EINVAL, "%s: workspace of %lld bytes is too small: %lld steps and max_duration %d need %lld", kEntry,
                    static_cast<long long>(workspace_bytes), static_cast<long long>(offsets[count]), D, static_cast<long long>(need));
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    long long* table = static_cast<long long*>(workspace);
    unsigned short* back = reinterpret_cast<unsigned short*>(table + ul::table_words(D));
    hssfsst::DurFillArgs fa{};
    fa.D = D;
    for (int first = 0; first < 8 * D; first += hssfsst::kDurFillValues) {
        fa.first = first;
        fa.n = std::min(hssfsst::kDurFillValues, 8 * D - first);
        for (int i = 0; i < fa.n; ++i) fa.v[i] = first + i < 4 * D ? durations[first + i] : edge[first + i - 4 * D];
        hipLaunchKernelGGL(hssfsst::seg_durations_fill_kernel, dim3(1), dim3(hssfsst::kDurFillValues), 0, st, table, fa);
        if (int rc = launch_check(kEntry, "seg_durations_fill_kernel")) return rc;
    }
    hssfsst::DurDecodeArgs args{};
    args.tb = ul::quantise_tables(transitions, initial);
    args.D = D;
    return seq_for_each_batch(kEntry, "seg_decode_durations_kernel", offsets, count, hssfsst::kDurDecodeBatch, args, [&](int64_t r0, int nrec) {
        hipLaunchKernelGGL(hssfsst::seg_decode_durations_kernel, dim3(static_cast<unsigned>(nrec)), dim3(ul::kLanes), 0, st, logp, states,
                           scores ? reinterpret_cast<long long*>(scores) + r0 : nullptr, back, table, args);
    });
}

}  // extern "C"

// Forward-backward under the transition model (hssfsst.h: hssfsst_posteriors; csrc/segmenter_posteriors.hpp).  Stateless: the
// launch's offsets travel as kernel arguments, kPostBatch recordings per launch; the tables are read from device memory.
extern "C" {

int hssfsst_posteriors_info(int* segment_steps, int64_t* max_steps, int64_t* work_bytes_per_step, int64_t* work_bytes_per_recording)
{
    if (segment_steps) *segment_steps = hssfsst::postlayout::kSegSteps;
    if (max_steps) *max_steps = hssfsst::postlayout::kMaxSteps;
    if (work_bytes_per_step) *work_bytes_per_step = hssfsst::postlayout::kWorkBytesPerStep;
    if (work_bytes_per_recording) *work_bytes_per_recording = hssfsst::postlayout::kWorkBytesPerRecording;
    return 0;
}

int hssfsst_posteriors(const float* logp, const int64_t* offsets, int64_t count, const float* a_pi, const uint8_t* labels, float* gamma,
                       double* loglik, double* score, double* xi, double* gamma0, void* work, int64_t work_bytes, int device, void* stream)
{
    namespace pl = hssfsst::postlayout;
    constexpr const char* kEntry = "posteriors";
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"logp", logp}, {"offsets", offsets}, {"a_pi", a_pi}, {"gamma", gamma}, {"loglik", loglik},
                                            {"work", work}})) return rc;
    if (score && !labels) return fail(HSSFSST_EINVAL, "%s: bad argument (labels is NULL while score is not)", kEntry);
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (int rc = seq_check_aligned(kEntry, {{"logp", logp, 16}, {"gamma", gamma, 16}, {"work", work, 16}, {"a_pi", a_pi, 4}, {"loglik", loglik, 8},
                                            {"score", score, 8}, {"xi", xi, 8}, {"gamma0", gamma0, 8}})) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, pl::kMaxSteps)) return rc;
    const int64_t need = pl::workspace_bytes(offsets[count], count);
    if (work_bytes < need)
        return fail(HSSFSST_EINVAL, "%s: work of %lld bytes is too small: %lld steps in %lld recordings need %lld", kEntry,
                    static_cast<long long>(work_bytes), static_cast<long long>(offsets[count]), static_cast<long long>(count),
                    static_cast<long long>(need));
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    hssfsst::PostArgs args{};
    return seq_for_each_batch(kEntry, "seg_posteriors_kernel", offsets, count, hssfsst::kPostBatch, args, [&](int64_t r0, int nrec) {
        args.rec0 = r0;
        hipLaunchKernelGGL(hssfsst::seg_posteriors_kernel, dim3(static_cast<unsigned>(nrec)), dim3(pl::kLanes), 0, st, logp, a_pi, labels, gamma,
                           loglik + r0, score ? score + r0 : nullptr, xi ? xi + 16 * r0 : nullptr, gamma0 ? gamma0 + 4 * r0 : nullptr,
                           static_cast<double*>(work), args);
    });
}

}  // extern "C"

// Forward-backward under the explicit-duration model (hssfsst.h: hssfsst_posteriors_durations;
// csrc/segmenter_duration_posteriors.hpp).  Stateless: the launch's offsets travel as kernel arguments, kDurPostBatch recordings per
// launch; all four tables are read from device memory, the two duration tables through a fill launch into the workspace's head.
// hssfsst_posteriors_durations_counts is the same call with the runs variant of the sweeps (it also leaves g and 1 / Z in a
// workspace that is larger by csrc/duration_counts_layout.hpp's parts) and, behind them, the counts launches
// (csrc/segmenter_duration_counts.hpp).
namespace {

// both entries: `with_counts` is the second one, whose `counts` is required
int posteriors_durations_run(const char* kEntry, bool with_counts, const float* logp, const int64_t* offsets, int64_t count, const float* a_pi,
                             const float* durations, const float* edge, int max_duration, const uint8_t* labels, float* gamma, float* onsets,
                             double* loglik, double* score, double* xi, double* s0, double* counts, void* work, int64_t work_bytes, int device,
                             void* stream)
{
    namespace dp = hssfsst::dplayout;
    namespace dc = hssfsst::dclayout;
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"logp", logp}, {"offsets", offsets}, {"a_pi", a_pi}, {"durations", durations}, {"edge", edge},
                                            {"gamma", gamma}, {"loglik", loglik}, {"work", work}})) return rc;
    if (with_counts)
        if (int rc = seq_check_nonnull(kEntry, {{"counts", counts}})) return rc;
    if (score && !labels) return fail(HSSFSST_EINVAL, "%s: bad argument (labels is NULL while score is not)", kEntry);
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (max_duration < 1 || max_duration > dp::kMaxDuration)
        return fail(HSSFSST_EINVAL, "%s: max_duration %d is outside 1..%d", kEntry, max_duration, dp::kMaxDuration);
    const int D = max_duration;
    if (int rc = seq_check_aligned(kEntry, {{"logp", logp, 16}, {"gamma", gamma, 16}, {"onsets", onsets, 16}, {"work", work, 16}, {"a_pi", a_pi, 4},
                                            {"durations", durations, 4}, {"edge", edge, 4}, {"loglik", loglik, 8}, {"score", score, 8},
                                            {"xi", xi, 8}, {"s0", s0, 8}, {"counts", counts, 8}})) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, dp::kMaxSteps)) return rc;
    const int64_t need = with_counts ? dc::workspace_bytes(offsets[count], count, D) : dp::workspace_bytes(offsets[count], count, D);
    if (work_bytes < need)
        return fail(HSSFSST_EINVAL, "%s: work of %lld bytes is too small: %lld steps in %lld recordings and max_duration %d need %lld", kEntry,
                    static_cast<long long>(work_bytes), static_cast<long long>(offsets[count]), static_cast<long long>(count), D,
                    static_cast<long long>(need));
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dc::Workspace wc = dc::workspace(offsets[count], count, D);
    const dp::Workspace& ws = wc.sweeps;                 // (dp::workspace(): the plain entry uses nothing behind it)
    char* w = static_cast<char*>(work);
    double* tabm = reinterpret_cast<double*>(w + ws.table_mant);
    int* tabe = reinterpret_cast<int*>(w + ws.table_exp);
    double* stash_m = reinterpret_cast<double*>(w + ws.stash_mant);
    int* stash_e = reinterpret_cast<int*>(w + ws.stash_exp);
    double* checkpoints = reinterpret_cast<double*>(w + ws.checkpoints);
    hipLaunchKernelGGL(hssfsst::seg_duration_posteriors_fill_kernel,
                       dim3(static_cast<unsigned>((8 * D + hssfsst::kDurPostFillLanes - 1) / hssfsst::kDurPostFillLanes)),
                       dim3(hssfsst::kDurPostFillLanes), 0, st, durations, edge, tabm, tabe, D);
    if (int rc = launch_check(kEntry, "seg_duration_posteriors_fill_kernel")) return rc;
    hssfsst::DurPostArgs args{};
    args.D = D;
    auto runs_of = [&](int64_t r0) {                     // what the launch of the recordings r0 .. sees of the second stash
        return hssfsst::DurRunsOut{reinterpret_cast<double*>(w + wc.g_mant), reinterpret_cast<int*>(w + wc.g_exp),
                                   reinterpret_cast<double*>(w + wc.invz_mant) + r0, reinterpret_cast<int*>(w + wc.invz_exp) + r0};
    };
    const char* sweep = with_counts ? "seg_duration_runs_sweep_kernel" : "seg_duration_posteriors_kernel";
    int rc = seq_for_each_batch(kEntry, sweep, offsets, count, hssfsst::kDurPostBatch, args, [&](int64_t r0, int nrec) {
        args.rec0 = r0;
        if (with_counts)
            hipLaunchKernelGGL(hssfsst::seg_duration_runs_sweep_kernel, dim3(static_cast<unsigned>(nrec)), dim3(dp::kLanes), 0, st, logp, a_pi,
                               durations, edge, labels, gamma, onsets, loglik + r0, score ? score + r0 : nullptr, xi ? xi + 16 * r0 : nullptr,
                               s0 ? s0 + 4 * r0 : nullptr, tabm, tabe, stash_m, stash_e, checkpoints, runs_of(r0), args);
        else
            hipLaunchKernelGGL(hssfsst::seg_duration_posteriors_kernel, dim3(static_cast<unsigned>(nrec)), dim3(dp::kLanes), 0, st, logp, a_pi,
                               durations, edge, labels, gamma, onsets, loglik + r0, score ? score + r0 : nullptr, xi ? xi + 16 * r0 : nullptr,
                               s0 ? s0 + 4 * r0 : nullptr, tabm, tabe, stash_m, stash_e, checkpoints, args);
    });
    if (rc || !with_counts) return rc;
    return seq_for_each_batch(kEntry, "seg_duration_run_counts_kernel", offsets, count, hssfsst::kDurPostBatch, args, [&](int64_t r0, int nrec) {
        args.rec0 = r0;
        hipLaunchKernelGGL(hssfsst::seg_duration_run_counts_kernel, dim3(static_cast<unsigned>(nrec), static_cast<unsigned>(dc::groups(D))),
                           dim3(dc::kLanes), 0, st, logp, a_pi, labels, counts + dc::counts_index(r0, 0, 0, 1, D), tabm, tabe, stash_m, stash_e,
                           checkpoints, runs_of(r0), args);
    });
}

}  // namespace

extern "C" {

int hssfsst_posteriors_durations_info(int* max_duration, int* segment_steps, int64_t* max_steps, int64_t* work_bytes_per_step,
                                      int64_t* work_bytes_per_recording, int64_t* work_bytes_per_duration)
{
    namespace dp = hssfsst::dplayout;
    if (max_duration) *max_duration = dp::kMaxDuration;
    if (segment_steps) *segment_steps = dp::kSegSteps;
    if (max_steps) *max_steps = dp::kMaxSteps;
    if (work_bytes_per_step) *work_bytes_per_step = dp::kWorkBytesPerStep;
    if (work_bytes_per_recording) *work_bytes_per_recording = dp::kWorkBytesPerRecording;
    if (work_bytes_per_duration) *work_bytes_per_duration = dp::kWorkBytesPerDuration;
    return 0;
}

int hssfsst_posteriors_durations(const float* logp, const int64_t* offsets, int64_t count, const float* a_pi, const float* durations,
                                 const float* edge, int max_duration, const uint8_t* labels, float* gamma, float* onsets, double* loglik,
                                 double* score, double* xi, double* s0, void* work, int64_t work_bytes, int device, void* stream)
{
    return posteriors_durations_run("posteriors_durations", false, logp, offsets, count, a_pi, durations, edge, max_duration, labels, gamma,
                                    onsets, loglik, score, xi, s0, nullptr, work, work_bytes, device, stream);
}

int hssfsst_posteriors_durations_counts_info(int64_t* work_bytes_per_step, int64_t* work_bytes_per_recording, int64_t* work_bytes_per_duration,
                                             int* durations_per_group)
{
    namespace dc = hssfsst::dclayout;
    if (work_bytes_per_step) *work_bytes_per_step = dc::kWorkBytesPerStep;
    if (work_bytes_per_recording) *work_bytes_per_recording = dc::kWorkBytesPerRecording;
    if (work_bytes_per_duration) *work_bytes_per_duration = dc::kWorkBytesPerDuration;
    if (durations_per_group) *durations_per_group = dc::kDurationsPerGroup;
    return 0;
}

int hssfsst_posteriors_durations_counts(const float* logp, const int64_t* offsets, int64_t count, const float* a_pi, const float* durations,
                                        const float* edge, int max_duration, const uint8_t* labels, float* gamma, float* onsets,
                                        double* loglik, double* score, double* xi, double* s0, double* counts, void* work, int64_t work_bytes,
                                        int device, void* stream)
{
    return posteriors_durations_run("posteriors_durations_counts", true, logp, offsets, count, a_pi, durations, edge, max_duration, labels,
                                    gamma, onsets, loglik, score, xi, s0, counts, work, work_bytes, device, stream);
}

}  // extern "C"

// Scoring a segmentation (hssfsst.h: hssfsst_score_states; csrc/segmenter_score.hpp, csrc/score_layout.hpp).  Stateless: the
// launch's offsets travel as kernel arguments, kScoreBatch recordings per launch of the kernels that read the arenas; the sort and
// the rank work on the caller's workspace, class after class, and the host decides the number of passes.
namespace {

// the launches of one class behind its items: the passes of the sort, then the three of the rank.  items_a holds the items.
int score_rank_class(const char* entry, hipStream_t st, unsigned char* work, const hssfsst::scorelayout::Workspace& w, int64_t n,
                     int passes, int per_recording, int64_t groups, unsigned long long* out)
{
    namespace sl = hssfsst::scorelayout;
    unsigned long long* src = reinterpret_cast<unsigned long long*>(work + w.items_a);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(work + w.items_b);
    unsigned* hist = reinterpret_cast<unsigned*>(work + w.hist);
    unsigned* sums = reinterpret_cast<unsigned*>(work + w.sums);
    unsigned* tile_agg = reinterpret_cast<unsigned*>(work + w.tile_agg);
    unsigned* tile_carry = reinterpret_cast<unsigned*>(work + w.tile_carry);
    const long long nblocks = sl::blocks(n), entries = sl::hist_entries(n), chunks = sl::scan_chunks(n), tiles = sl::rank_tiles(n);
    const dim3 sort_grid(static_cast<unsigned>(sl::sort_groups(n))), sort_block(sl::kSortThreads);
    const dim3 scan_grid(static_cast<unsigned>(chunks)), scan_block(sl::kScanThreads);
    for (int pass = 0; pass < passes; ++pass) {
        hipLaunchKernelGGL(hssfsst::seg_score_hist_kernel, sort_grid, sort_block, 0, st, src, hist, static_cast<long long>(n), nblocks, pass);
        if (int rc = launch_check(entry, "seg_score_hist_kernel")) return rc;
        hipLaunchKernelGGL(hssfsst::seg_score_scan_sums_kernel, scan_grid, scan_block, 0, st, hist, sums, entries);
        if (int rc = launch_check(entry, "seg_score_scan_sums_kernel")) return rc;
        hipLaunchKernelGGL(hssfsst::seg_score_scan_top_kernel, dim3(1), scan_block, 0, st, sums, chunks);
        if (int rc = launch_check(entry, "seg_score_scan_top_kernel")) return rc;
        hipLaunchKernelGGL(hssfsst::seg_score_scan_apply_kernel, scan_grid, scan_block, 0, st, hist, sums, entries);
        if (int rc = launch_check(entry, "seg_score_scan_apply_kernel")) return rc;
        hipLaunchKernelGGL(hssfsst::seg_score_scatter_kernel, sort_grid, sort_block, 0, st, src, dst, hist, static_cast<long long>(n), nblocks,
                           pass);
        if (int rc = launch_check(entry, "seg_score_scatter_kernel")) return rc;
        std::swap(src, dst);
    }
    const dim3 rank_grid(static_cast<unsigned>(tiles)), rank_block(sl::kRankThreads);
    hipLaunchKernelGGL(hssfsst::seg_score_rank_kernel<false>, rank_grid, rank_block, 0, st, src, static_cast<long long>(n), tile_agg, tile_carry,
                       out, per_recording, static_cast<long long>(groups));
    if (int rc = launch_check(entry, "seg_score_rank_kernel<false>")) return rc;
    hipLaunchKernelGGL(hssfsst::seg_score_rank_scan_kernel, dim3(1), dim3(64), 0, st, tile_agg, tile_carry, tiles);
    if (int rc = launch_check(entry, "seg_score_rank_scan_kernel")) return rc;
    hipLaunchKernelGGL(hssfsst::seg_score_rank_kernel<true>, rank_grid, rank_block, 0, st, src, static_cast<long long>(n), tile_agg, tile_carry,
                       out, per_recording, static_cast<long long>(groups));
    return launch_check(entry, "seg_score_rank_kernel<true>");
}

}  // namespace

extern "C" {

int hssfsst_score_info(int64_t* work_bytes_per_step, int64_t* work_bytes_per_recording, int64_t* work_bytes_constant, int* block_items,
                       int* digit_bits, int* max_passes)
{
    namespace sl = hssfsst::scorelayout;
    if (work_bytes_per_step) *work_bytes_per_step = sl::kWorkBytesPerStep;
    if (work_bytes_per_recording) *work_bytes_per_recording = sl::kWorkBytesPerRecording;
    if (work_bytes_constant) *work_bytes_constant = sl::kWorkBytesConstant;
    if (block_items) *block_items = sl::kBlockItems;
    if (digit_bits) *digit_bits = sl::kDigitBits;
    if (max_passes) *max_passes = sl::kMaxPasses;
    return 0;
}

int hssfsst_score_states(const float* logp, const uint8_t* states, const uint8_t* labels, const int64_t* offsets, int64_t count,
                         int per_recording, int64_t* confusion, int64_t* ignored, int64_t* rank, void* work, int64_t work_bytes,
                         const hssfsst_launch* where)
{
    namespace sl = hssfsst::scorelayout;
    constexpr const char* kEntry = "score_states";
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"labels", labels}, {"offsets", offsets}, {"confusion", confusion}, {"ignored", ignored},
                                            {"where", where}})) return rc;
    if (!states && !logp) return fail(HSSFSST_EINVAL, "%s: bad argument (states and logp are both NULL)", kEntry);
    if (rank && !logp) return fail(HSSFSST_EINVAL, "%s: bad argument (logp is NULL while rank is not)", kEntry);
    if (rank && !work) return fail(HSSFSST_EINVAL, "%s: bad argument (work is NULL while rank is not)", kEntry);
    const int device = where->device;
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (int rc = seq_check_aligned(kEntry, {{"logp", logp, 16}, {"work", work, 16}, {"confusion", confusion, 8}, {"ignored", ignored, 8},
                                            {"rank", rank, 8}})) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, seqargs::kMaxTotalSteps)) return rc;
    const int64_t total = offsets[count];
    const int64_t need = rank ? sl::workspace_bytes(total, count) : 0;
    if (work_bytes < need)
        return fail(HSSFSST_EINVAL, "%s: work of %lld bytes is too small: %lld steps in %lld recordings need %lld", kEntry,
                    static_cast<long long>(work_bytes), static_cast<long long>(total), static_cast<long long>(count),
                    static_cast<long long>(need));
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(where->stream);
    const int64_t groups = per_recording ? count : 1;
    const int64_t pooled[2] = {0, total};
    const int64_t* list = per_recording ? offsets : pooled;
    const int64_t nlist = per_recording ? count : 1;
    const std::pair<void*, size_t> outputs[3] = {{confusion, 128 * static_cast<size_t>(groups)}, {ignored, 8 * static_cast<size_t>(groups)},
                                                 {rank, 96 * static_cast<size_t>(groups)}};
    for (const auto& z : outputs) {                      // the kernels add into them
        if (!z.first) continue;
        const hipError_t e = hipMemsetAsync(z.first, 0, z.second, st);
        if (e != hipSuccess) return fail(HSSFSST_EHIP, "%s: clearing the outputs failed: %s", kEntry, hipGetErrorString(e));
    }
    hssfsst::ScoreArgs args{};
    args.per_recording = per_recording ? 1 : 0;
    auto grid_of = [&](int nrec) { return dim3(static_cast<unsigned>(sl::count_groups(args.off[nrec] - args.off[0]))); };
    if (int rc = seq_for_each_batch(kEntry, "seg_score_counts_kernel", list, nlist, sl::kScoreBatch, args, [&](int64_t r0, int nrec) {
            args.rec0 = r0;
            args.nrec = nrec;
            hipLaunchKernelGGL(hssfsst::seg_score_counts_kernel, grid_of(nrec), dim3(sl::kCountThreads), 0, st, logp, states, labels,
                               reinterpret_cast<unsigned long long*>(confusion), reinterpret_cast<unsigned long long*>(ignored),
                               reinterpret_cast<unsigned long long*>(rank), args);
        })) return rc;
    if (!rank) return 0;
    const sl::Workspace w = sl::workspace(total);
    const int passes = sl::passes(count, args.per_recording);
    for (int cls = 0; cls < 4; ++cls) {
        if (int rc = seq_for_each_batch(kEntry, "seg_score_keys_kernel", list, nlist, sl::kScoreBatch, args, [&](int64_t r0, int nrec) {
                args.rec0 = r0;
                args.nrec = nrec;
                hipLaunchKernelGGL(hssfsst::seg_score_keys_kernel, grid_of(nrec), dim3(sl::kCountThreads), 0, st, logp, states, labels,
                                   reinterpret_cast<unsigned long long*>(static_cast<unsigned char*>(work) + w.items_a), cls, args);
            })) return rc;
        if (int rc = score_rank_class(kEntry, st, static_cast<unsigned char*>(work), w, total, passes, args.per_recording, groups,
                                      reinterpret_cast<unsigned long long*>(rank) + 3 * cls)) return rc;
    }
    return 0;
}

}  // extern "C"

// Stitching overlapping windows' log-probs (hssfsst.h: hssfsst_stitch_windows; csrc/segmenter_stitch.hpp, csrc/stitch_layout.hpp).
// Stateless: the launch's offsets and window blocks travel as kernel arguments, kStitchBatch recordings per launch; nothing is
// copied from host memory and nothing waits.
namespace {

template <int MODE>
void stitch_launch(bool weighted, dim3 grid, hipStream_t st, const float* win, const float* weights, float* out, unsigned char* dissent,
                   const hssfsst::StitchArgs& args)
{
    const dim3 block(hssfsst::stitchlayout::kThreads);
    if (weighted) hipLaunchKernelGGL((hssfsst::seg_stitch_kernel<MODE, true>), grid, block, 0, st, win, weights, out, dissent, args);
    else hipLaunchKernelGGL((hssfsst::seg_stitch_kernel<MODE, false>), grid, block, 0, st, win, weights, out, dissent, args);
}

}  // namespace

extern "C" {

int hssfsst_stitch_windows(const float* win_logp, const int64_t* win_first, int64_t win_steps, const int64_t* offsets, int64_t count,
                           int n, int stride, const float* weights, int mode, float* out, uint8_t* dissent, hssfsst_launch where)
{
    namespace stl = hssfsst::stitchlayout;
    constexpr const char* kEntry = "stitch_windows";
    if (count < 0) return fail(HSSFSST_EINVAL, "%s: count %lld is negative", kEntry, static_cast<long long>(count));
    if (int rc = seq_check_nonnull(kEntry, {{"win_logp", win_logp}, {"win_first", win_first}, {"offsets", offsets}, {"out", out}})) return rc;
    if (win_steps < 0) return fail(HSSFSST_EINVAL, "%s: win_steps %lld is negative", kEntry, static_cast<long long>(win_steps));
    if (n < 1) return fail(HSSFSST_EINVAL, "%s: window length %d is not positive", kEntry, n);
    if (stride < 1 || stride > n) return fail(HSSFSST_EINVAL, "%s: stride %d is outside 1 .. %d", kEntry, stride, n);
    if (mode != HSSFSST_STITCH_PROB && mode != HSSFSST_STITCH_LOGP && mode != HSSFSST_STITCH_SELECT)
        return fail(HSSFSST_EINVAL, "%s: unknown mode %d", kEntry, mode);
    const int device = where.device;
    if (device < 0) return fail(HSSFSST_EINVAL, "%s: device %d is negative", kEntry, device);
    if (int rc = seq_check_aligned(kEntry, {{"win_logp", win_logp, 16}, {"out", out, 16}, {"weights", weights, 4}})) return rc;
    if (int rc = seq_check_list(kEntry, offsets, count, seqargs::kMaxTotalSteps)) return rc;
    for (int64_t i = 0; i < count; ++i) {
        const int64_t rows = stl::window_rows(offsets[i + 1] - offsets[i], n, stride);
        if (win_first[i] < 0 || win_first[i] > win_steps - rows)
            return fail(HSSFSST_EINVAL, "%s: win_first[%lld] = %lld: the %lld window rows of recording %lld do not lie within the %lld of the arena",
                        kEntry, static_cast<long long>(i), static_cast<long long>(win_first[i]), static_cast<long long>(rows),
                        static_cast<long long>(i), static_cast<long long>(win_steps));
    }
    if (!stl::supported(n, stride))
        return fail(HSSFSST_EUNSUPPORTED, "%s: windows of %d steps at stride %d overlap %d-fold, over the limit of %d", kEntry, n, stride,
                    stl::ratio(n, stride), stl::kMaxRatio);
    if (count == 0) return 0;
    if (int rc = check_device(kEntry, device)) return rc;
    DEVICE_SCOPE(device);
    const hipStream_t st = static_cast<hipStream_t>(where.stream);
    hssfsst::StitchArgs args{};
    args.n = n;
    args.stride = stride;
    // (args.off is int: seq_check_list has held the list to 2^31 - 1 steps)
    return seq_for_each_batch(kEntry, "seg_stitch_kernel", offsets, count, stl::kStitchBatch, args, [&](int64_t r0, int nrec) {
        for (int i = 0; i < nrec; ++i) args.first[i] = win_first[r0 + i];
        args.nrec = nrec;
        const dim3 grid(static_cast<unsigned>(stl::launch_groups(offsets[r0 + nrec] - offsets[r0])));
        if (mode == HSSFSST_STITCH_PROB) stitch_launch<stl::kProb>(weights != nullptr, grid, st, win_logp, weights, out, dissent, args);
        else if (mode == HSSFSST_STITCH_LOGP) stitch_launch<stl::kLogp>(weights != nullptr, grid, st, win_logp, weights, out, dissent, args);
        else stitch_launch<stl::kSelect>(weights != nullptr, grid, st, win_logp, weights, out, dissent, args);
    });
}

}  // extern "C"
