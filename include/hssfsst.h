/*
 * hssfsst.h -- C ABI of libhssfsst.so: the MI355X (gfx950) Fourier-synchrosqueezed-transform
 * feature path.  This is the drop-in boundary for the ONE native dependency of the reference's hot
 * path: the CPython extension `ssq` (-> libssq -> FFTW) that
 *     /root/reference/hss/transforms/synchrosqueeze.py:48   s, f, t = ssq.fsst(x.numpy(), fs, window)
 * binds, plus the tensor epilogue of the same file (:50-111) which the library fuses on the device.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative HSSFSST_E* code and
 *     never throws; hssfsst_last_error() returns a thread-local message for the last failure;
 *   - the caller owns every data buffer; a plan is an opaque handle owned by the library;
 *   - there is NO CPU compute path in this library: creating a plan needs a HIP device and fails
 *     with HSSFSST_ENODEVICE otherwise (the CPU restatement lives in oracle/, test-only);
 *   - HIP is touched for the first time inside hssfsst_plan_create(), in the calling process
 *     (fork-safe for DataLoader workers: create the plan after the fork);
 *   - a plan is SINGLE-STREAM: its execs must be queued on one stream at a time (scratch buffers, the team kernel's arrival
 *     numbers and mailboxes belong to the plan); use one plan per stream.  "At a time" is meant in DEVICE order: a plan may be
 *     handed from one stream to another behind a host synchronisation or behind an event the new stream waits for (no host wait),
 *     as long as every exec queued earlier is ordered before the first exec on the new stream (tests/test_stream_order.py);
 *   - hssfsst_exec() enqueues on `stream` (a hipStream_t, NULL = default stream) and returns
 *     without synchronising when both buffers are device buffers; with a host buffer on either
 *     side it stages through the plan's device scratch and synchronises before returning;
 *   - one plan may be used from one host thread at a time;
 *   - ALIGNMENT: every pointer is aligned to its own element type (4 bytes for float32, 8 for float64 / int64 / complex64, 2 for
 *     the 2-byte elements of a half plan), and that is all an entry point asks unless its comment states more.  Where a comment
 *     states 16 bytes, the entry returns HSSFSST_EINVAL and names the argument before any device work.  Everywhere else a buffer
 *     may start at any element -- a view one float into a tensor, say -- and the result has the bits of the 16-byte aligned call:
 *     no kernel touches a caller's buffer with an access wider than the alignment the buffer has.  No entry point reads or writes
 *     outside the extents its comment gives; workspaces and the training stash are used up to their stated minimum and no
 *     further (tests/test_guard_bands.py walks every entry point through a guard arena to hold both).
 */
#ifndef HSSFSST_H
#define HSSFSST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSSFSST_VERSION 210

/* status codes */
#define HSSFSST_OK 0
#define HSSFSST_EINVAL (-1)    /* bad argument (NULL, non-positive size, unknown mode ...)        */
#define HSSFSST_ENODEVICE (-2) /* no usable HIP device / runtime                                  */
#define HSSFSST_EUNSUPPORTED (-3) /* configuration beyond the kernels' LDS budget (huge window x wide band)  */
#define HSSFSST_ENOMEM (-4)    /* host or device allocation failed                                */
#define HSSFSST_EHIP (-5)      /* a HIP call failed (message in hssfsst_last_error)               */

/* output modes == the branches of FSST.__call__ (synchrosqueeze.py:59-65) */
#define HSSFSST_MODE_RAW 0   /* :65     complex64 (K, n), frequency-major, interleaved re/im      */
#define HSSFSST_MODE_ABS 1   /* :59-60  float32 (n, K)   = abs(s).t()                             */
#define HSSFSST_MODE_STACK 2 /* :62-63  float32 (n, 2K)  = z-scored [real | imag], transposed      */
#define HSSFSST_MODE_STACK_UNNORM 3 /* extension (streaming): as STACK but without the z-score    */

typedef struct hssfsst_plan hssfsst_plan;

/* Replaces FSST.__init__ (synchrosqueeze.py:13-35) + everything of ssq.fsst that depends only on
 * (fs, window): derivative window (not-a-knot spline), class-folded twiddle tables, the kept band
 * of _truncate_frequencies (synchrosqueeze.py:91-111; inclusive bounds compared in float32).
 *   device     HIP device ordinal (>= 0)
 *   window     nwin doubles (the analysis window; nfft = nwin).  Any length, odd ones included, as the reference
 *              (synchrosqueeze.py:48): 32 / 64 / 128 / 256 / 512 run the radix kernels, every other length the
 *              any-length kernel (windowed DFT on the fp32 matrix pipe, csrc/fsst_dft.hpp)
 *   has_band   0: keep all nwin/2+1 rows; 1: keep rows with f_lo <= k*fs/nwin <= f_hi
 *   mode       HSSFSST_MODE_*
 * Alignment: window (host, read here and not again) at any double. */
int hssfsst_plan_create(hssfsst_plan** out, int device, int nwin, const double* window, double fs,
                        int has_band, double f_lo, double f_hi, int mode);
int hssfsst_plan_destroy(hssfsst_plan* plan);

/* Element types of a plan's output and of the resample execs' buffers.  F16 / BF16 (IEEE binary16 / bfloat16, 2 bytes): the
 * STACK features written in half precision straight from the kernels -- see hssfsst_plan_create_ex. */
#define HSSFSST_DTYPE_F32 0
#define HSSFSST_DTYPE_F64 1
#define HSSFSST_DTYPE_F16 2
#define HSSFSST_DTYPE_BF16 3

/* hssfsst_plan_create with the element type of every exec's output: hssfsst_plan_create(...) is exactly
 * hssfsst_plan_create_ex(..., HSSFSST_DTYPE_F32).  out_dtype F16 / BF16 is for HSSFSST_MODE_STACK only (RAW stays complex64, ABS
 * and STACK_UNNORM float32); an unknown out_dtype, F64, or F16 / BF16 with another mode return HSSFSST_EINVAL before any device
 * is touched.  A half plan's features are the float32 plan's, each rounded to nearest even (what Tensor.to(dtype) does; NaN
 * where float32 has NaN, e.g. the 0 / 0 z-score of an all-zero signal).  On a half plan every exec entry point --
 * hssfsst_exec, _exec_cols, _exec_frames, _exec_list, _exec_ragged, _exec_pinned -- writes 2-byte elements through its `out`
 * pointer (declared float*: pass the buffer's address); counts and layouts are unchanged (out_floats_per_sample counts
 * elements, ragged offsets are 64-bit element offsets) and the pinned pool lends buffers of n x 2K x 2 bytes.
 * Where the features are written: the team kernel (canonical bands, hssfsst_plan_last_exec_fused == 2) stores 2-byte z-scores
 * from its registers; every other path writes the un-normalised float32 features to a device scratch of the plan (4 bytes x
 * the exec's element count, kept and grown like the plan's other buffers; allocated for team execs too, for the gated fallback)
 * and an out-of-place z-score sweep writes the 2-byte result.  The one-CU-per-signal kernels, which normalise float32 in place,
 * are not taken by half plans (HSSFSST_ZPATH_ONE_CU then means two launches). */
int hssfsst_plan_create_ex(hssfsst_plan** out, int device, int nwin, const double* window, double fs,
                           int has_band, double f_lo, double f_hi, int mode, int out_dtype);

/* The plan's output element type (HSSFSST_DTYPE_*). */
int hssfsst_plan_out_dtype(const hssfsst_plan* plan, int* out_dtype);

/* Plan geometry: nf = nwin/2+1 one-sided rows, klo = first kept row, K = number of kept rows,
 * out_floats_per_sample = floats written per input sample (RAW 2K, ABS K, STACK 2K).
 * Any output pointer may be NULL. */
int hssfsst_plan_info(const hssfsst_plan* plan, int* nwin, int* nf, int* klo, int* K,
                      int* out_floats_per_sample, int* mode, int* device);

/* Replaces the call ssq.fsst(x, fs, window) (synchrosqueeze.py:48) AND the epilogue :50-65 for
 * `batch` independent signals of `n` samples each (x: float32 [batch][n], contiguous).
 * out: float32 (2-byte elements on a half plan: hssfsst_plan_create_ex), batch * n * out_floats_per_sample elements, laid out per mode (see HSSFSST_MODE_*),
 * each signal's block contiguous.  x_on_device / out_on_device: 1 = device pointer on the plan's
 * device, 0 = host pointer.  stream: hipStream_t or NULL.
 * A call with a host `out` returns when the features are in `out`.  For small execs (the dataset loop's one frame per call) it learns that
 * from a word the kernel's last block stores to pinned host memory behind a system-scope release of all stores, not from the stream:
 * `stream` may still be retiring that launch for a few microseconds after the return (later work on it queues behind, as always).
 * Alignment: x and out at any element, host or device.  The float32 kernels store 16 bytes at a time relative to `out`; a device `out`
 * that is not 16-byte aligned is therefore written through the plan's own output staging (the buffer a host `out` goes through) and
 * one device-to-device copy on `stream` -- same bits, nothing waits.  This holds for every exec entry point below. */
int hssfsst_exec(hssfsst_plan* plan, const float* x, int64_t batch, int n, int x_on_device,
                 float* out, int out_on_device, void* stream);

/* Streaming / windowed variant: computes only the output columns (frame centres) col0 .. col0+ncols-1
 * of every signal; `out` then holds batch * ncols * out_floats_per_sample floats and the STACK
 * statistics run over those columns.  hssfsst_exec(...) == hssfsst_exec_cols(..., 0, n, ...).
 * With col0 >= nwin/2 and col0 + ncols <= n - nwin/2 + 1 no frame touches the zero padding, which is
 * what a rolling transform over a ring buffer needs (SURVEY section 8f row 3 / BASELINE config 5).
 * Alignment: x and out at any element, as hssfsst_exec. */
int hssfsst_exec_cols(hssfsst_plan* plan, const float* x, int64_t batch, int n, int col0, int ncols,
                      int x_on_device, float* out, int out_on_device, void* stream);

/* Framed variant: the `batch` signals are views of ONE buffer whose starts are x_stride samples apart
 * (x_stride < n: overlapping frames).  Replaces the reference's framing + per-frame transform loop
 * (hss/utils/preprocess.py:40-52 frame_signal -> hss/datasets/heart_sounds.py:166-168): a recording is uploaded once
 * and its stride-1000 / length-2000 frames are read in place.  x spans (batch-1)*x_stride + n floats.
 * hssfsst_exec_cols(...) == hssfsst_exec_frames(..., x_stride = n, ...).
 * Alignment: x at any element (so is every frame: x_stride is any number of samples); out at any element, as hssfsst_exec. */
int hssfsst_exec_frames(hssfsst_plan* plan, const float* x, int64_t batch, int n, int64_t x_stride, int col0, int ncols,
                        int x_on_device, float* out, int out_on_device, void* stream);

/* The reference's dataset loop calls the transform once per 2000-sample CPU frame (hss/datasets/heart_sounds.py:166-168,199-201).
 * hssfsst_exec_pinned is hssfsst_exec for ONE host signal of n samples whose result is not copied: the kernels store the features
 * straight into a pinned, device-mapped buffer of the plan's pool (at most 64 buffers) and *out is LENT that buffer -- n x
 * floats-per-sample floats in the mode's layout, valid until hssfsst_pinned_release(plan, *out) or the plan's destruction.
 * Returns 0; 1 (no error, *out = NULL) when every pool buffer is still lent out or the exec is not one whose features are written
 * exactly once (then call hssfsst_exec); < 0 on error.  The Python class hands the buffer out as the returned tensor's storage and
 * releases it when that tensor dies; a caller that keeps every result (the in-memory dataset) falls back to the copying call
 * after 64 frames.
 * Alignment: x (host) at any element; the lent buffer is the plan's and 16-byte aligned. */
int hssfsst_exec_pinned(hssfsst_plan* plan, const float* x, int n, float** out);
int hssfsst_pinned_release(hssfsst_plan* plan, float* buf);

/* The same transform for a LIST of frames of one buffer: signal b = x[starts[b] .. starts[b] + n), 0 <= starts[b] <=
 * x_len - n (checked when `starts` is host memory; a device array is trusted).  This is the batched form of the
 * dataset loop hss/datasets/heart_sounds.py:155-169 over MANY recordings: the recordings sit back to back in `x`
 * (one upload), `starts` lists every frame of every recording (hss/utils/preprocess.py:40-52), one call transforms
 * them all: the frames are gathered into a dense batch on the device (8 kB per 2000-sample frame against 360 kB of
 * features) and take the kernels of hssfsst_exec.  out: [batch][n][...] as hssfsst_exec.
 * Alignment: x and out at any element, as hssfsst_exec; starts at any int64. */
int hssfsst_exec_list(hssfsst_plan* plan, const float* x, int64_t x_len, const int64_t* starts, int starts_on_device,
                      int64_t batch, int n, int x_on_device, float* out, int out_on_device, void* stream);

/* B signals of DIFFERENT lengths in one exec -- the reference's lazy dataset and PhysioNet loader transform whole recordings, one
 * call each (hss/datasets/heart_sounds.py:85-106,175-184,199-212).  Signal i is x[starts[i] .. starts[i] + lens[i]) and its
 * features land at out + out_floats_per_sample * (lens[0] + ... + lens[i-1]) in the mode's per-signal layout (RAW (K, len)
 * complex64, ABS (len, K), STACK (len, 2K) z-scored over that signal's own columns).  starts / lens: int64 HOST arrays.  Signals
 * may overlap or touch in x; a frame never reads samples of another signal (outside its own [0, len) it sees zeros, as in a
 * single exec).  For every i the result is bit-identical to hssfsst_exec(plan, x + starts[i], 1, lens[i], ...).
 * Argument errors -- a NULL pointer, batch < 0, lens[i] < 1, a signal outside [0, x_len), a signal over the per-signal limit
 * len * 2 nf < 2^31 -- return HSSFSST_EINVAL before any device is touched (all but the last are checked before the plan is
 * looked at); batch == 0 does nothing.  Offsets into the packed output are 64-bit: the total may exceed 2^31 floats.
 * Host x: the extent the list covers is uploaded in one copy; host out: the features come back in one copy (pinned memory
 * makes both DMA).  Plans of the MFMA kernel (window length 128 / 256 / 512, every band and mode): one transform launch for
 * the whole list (chunk list made on the host, kept while the next call has the same lengths and offsets) and, for STACK, one
 * statistics and one z-score launch.  Other window lengths (the generic nwin 32 / 64 kernel, the any-length kernel): one
 * hssfsst_exec per signal on `stream`, inside the library -- correct, not batched.  Synchronisation as hssfsst_exec.
 * Alignment: x and out at any element, as hssfsst_exec (a signal's own block inside `out` starts wherever the lengths before it put
 * it); starts and lens (host) at any int64. */
int hssfsst_exec_ragged(hssfsst_plan* plan, const float* x, int64_t x_len, const int64_t* starts, const int64_t* lens,
                        int64_t batch, int x_on_device, float* out, int out_on_device, void* stream);

/* Device-side health of the plan's asynchronous work.  The single-launch z-score kernels contain waits on other
 * waves (of the same CU: the one-CU-per-signal kernel; of other CUs of a team: the team kernel, see hssfsst_plan_fallbacks).
 * Every wait of the one-CU-per-signal kernel is bounded (2 s) and a give-up is recorded in a status word in pinned host
 * memory instead of hanging the GPU.  The library looks at that
 * word without synchronising at the start of EVERY exec of the plan and returns HSSFSST_EHIP if an earlier exec's wait
 * gave up (that exec's features are invalid), so a caller of device-output execs learns of it at the next call at the
 * latest; host-output execs check before they return; this function waits for the device and checks now. */
int hssfsst_plan_check(hssfsst_plan* plan);

/* Which path the plan's last STACK exec took: 0 = two launches (transform, then statistics + z-score sweep: long
 * signals, other window lengths, odd or wide bands), 1 = the one-CU-per-signal kernel (full batches of 961..2048-sample
 * signals; only when preferred or for bands the team kernel does not take), 2 = the team kernel (the reference's band,
 * signals up to 2048 samples, any batch: features stay in registers until the signal's statistics arrive from the team).
 * All three give bit-identical results. */
int hssfsst_plan_last_exec_fused(const hssfsst_plan* plan);

/* The dispatch made observable: the transform kernel the plan's last exec ran, as
 * "<instantiation> [<waves> waves/block, grid <blocks>]" (NUL-terminated, truncated to len).  The kernel a given
 * (window length, band, mode, n, batch) takes is otherwise only visible in a kernel trace. */
int hssfsst_plan_last_kernel(const hssfsst_plan* plan, char* buf, int len);

/* Preference among those paths for the plan's following STACK execs: HSSFSST_ZPATH_AUTO (default: the fastest that
 * applies), HSSFSST_ZPATH_TWO_LAUNCH, HSSFSST_ZPATH_ONE_CU (else two launches), HSSFSST_ZPATH_TEAM (else two launches).  A
 * path that does not apply to a shape (see above) is never forced.  Results do not depend on the choice. */
#define HSSFSST_ZPATH_AUTO 0
#define HSSFSST_ZPATH_TWO_LAUNCH 1
#define HSSFSST_ZPATH_ONE_CU 2
#define HSSFSST_ZPATH_TEAM 3
int hssfsst_plan_set_zpath(hssfsst_plan* plan, int zpath);

/* The team kernel's blocks wait for each other; when they are kept apart (other processes' kernels on the same GPU, two launches
 * of one plan on different streams) a wait runs out of time (0.5 ms), the launch gives itself up and the exec is computed by the
 * kernels the library queues behind every team launch, gated on exactly that event: same result, no error.  This returns how many
 * distinct team launches of the plan were seen to have fallen back so far (sampled whenever it is called: call it after a
 * synchronisation).  (Signals that ride on an offset no longer count here: since round 5 the team kernel computes them itself.)
 * A give-up costs the launch its wait bound (0.5 ms) before the gated kernels run: when the host sees four give-ups of a plan in a
 * row (host-output execs look after their own synchronisation, this call looks too) the plan's next 256 execs that would take the
 * team kernel take the one-CU-per-signal / two-launch kernels straight away, then the team kernel is tried again
 * (profiles/r06_stress.txt: DataLoader workers sharing one GPU, /root/reference/main.py:202-218). */
int hssfsst_plan_fallbacks(hssfsst_plan* plan);

/* Multi-GPU reassembly of the feature batch -- the one exchange of the path (BASELINE north_star: "an RCCL all-gather over xGMI only
 * to reassemble the feature batch for the LSTM"; the reference itself has no distributed code, main.py:224-230) -- without torch:
 * every rank contributes `count` floats at sendbuf and receives world x count floats, in rank order, at recvbuf (device pointers;
 * sendbuf may be recvbuf + rank x count: in place).  comm: the caller's ncclComm_t (one process per GPU).  RCCL is loaded with
 * dlopen("librccl.so.1") on first use: the library does not link it, and a host without it gets HSSFSST_EUNSUPPORTED here only.
 * timeout_ms > 0: the call waits for the collective on `stream`, at most that long (HSSFSST_EHIP when exceeded: a peer is missing
 * -- every wait of this library is bounded; the collective is then STILL ENQUEUED on `stream` and still owns both buffers: the
 * caller must not reuse or free them before the stream has drained or the communicator was aborted); 0: returns after enqueueing.
 * The call uses the CURRENT HIP device of the calling thread (the communicator's), it does not switch devices. */
int hssfsst_allgather(const float* sendbuf, float* recvbuf, int64_t count, void* nccl_comm, void* stream, int timeout_ms);

/* Per-kernel HIP-event timing on the exec stream (bench.py's roofline leg).  While enabled, every
 * hssfsst_exec records events around each of its core-kernel launches (a STACK exec runs the batch in
 * cache-sized chunks: core, z-score, core, z-score ...) WITHOUT synchronising; enabling resets the
 * record.  enable = n > 1 times every n-th exec only (an event is a packet on the stream: two per exec cost a
 * 0.18 ms exec ~3 us).  hssfsst_plan_timing() synchronises once and returns, over all TIMED execs since enabling:
 * ms_sum[0] = total synchrosqueeze-core kernel time, ms_sum[1] = rest of the exec (z-score kernels,
 * 0 unless STACK), both in milliseconds, and *nexec = number of execs recorded. */
int hssfsst_plan_set_timing(hssfsst_plan* plan, int enable);
int hssfsst_plan_timing(hssfsst_plan* plan, float ms_sum[2], int* nexec);

/* Host helper, no device needed: derivative window of ssq.fsst's IF estimator
 * (dtwin: not-a-knot cubic spline through (1..n, w), analytic derivative at the knots, * fs/2pi).  window and dwindow: nwin doubles
 * each, at any double. */
int hssfsst_dtwin(const double* window, int nwin, double fs, double* dwindow);

/* Host helper, no device needed: kept band of _truncate_frequencies (synchrosqueeze.py:91-111). */
int hssfsst_band(int nwin, double fs, double f_lo, double f_hi, int* klo, int* K);

/* hss.moments (hss/moments/__init__.py:1-36): scalar running mean and Welford M2 update. */
double hssfsst_update_mean(double m, double x, int64_t k);
double hssfsst_update_variance(double x, double m, double var, int64_t k);

/* Device-side counterpart of hss.moments for feature batches: merges, per signal, the running
 * (count, mean, M2) of the real and imaginary feature blocks with the statistics of a new STACK-less
 * chunk (Chan's pairwise form of the update above).  state: float64 [batch][6] =
 * {count_re, mean_re, M2_re, count_im, mean_im, M2_im} on the device.  feats: float32
 * [batch][n][2K] un-normalised [real | imag] features on the device.
 * Alignment: feats at any float (a signal's block is read 16 bytes at a time only where it is 16-byte aligned), state at any double. */
int hssfsst_moments_merge(hssfsst_plan* plan, const float* feats, int64_t batch, int n,
                          double* state, void* stream);

/* Streaming z-score: normalises un-normalised features IN PLACE with the running statistics in
 * `state` (as maintained by hssfsst_moments_merge): (v - mean) / sqrt(M2 / (count - 1)) per block.
 * Alignment: feats at any float (16-byte accesses only where a signal's block is 16-byte aligned), state at any double. */
int hssfsst_normalize_running(hssfsst_plan* plan, float* feats, int64_t batch, int n,
                              const double* state, void* stream);

/* One step of the rolling transform (BASELINE config 5: C channels, `chunk` new samples per channel per step; no
 * counterpart in the reference, built from the same path -- see heart_sounds_segmentation_amd/streaming.py).
 * `tape`: float32 [channels][tape_len] on the device, the caller's sample history; the step
 *   1. copies x_new ([channels] rows of `chunk` samples, x_stride >= chunk samples apart; device memory, or host
 *      memory when x_on_device = 0 -- pinned for an asynchronous copy) to tape[:, pos .. pos + chunk),
 *   2. transforms the `chunk` frames that end at the new samples (frames tape[:, pos - (nwin-1) + j ..], hop 1: no
 *      frame touches padding) into `out` = float32 [channels][chunk][2K] on the device (plan mode STACK_UNNORM),
 *   3. state != NULL: merges the chunk into the running moments `state` (float64 [channels][6], as
 *      hssfsst_moments_merge) and normalises `out` with the UPDATED moments (as hssfsst_normalize_running) in one
 *      launch -- bit-identical to calling the two,
 *   4. out_host != NULL: copies `out` to out_host (pinned host memory) and waits for the stream: when the call
 *      returns the features of this step are on the host (the latency BASELINE config 5 asks for).
 * Requires nwin - 1 <= pos and pos + chunk <= tape_len; the caller moves the history back to the start of the
 * tape when it is full.
 * For window lengths 256 / 512 with an even band of <= 24 rows (config 5) steps 1-4 are ONE kernel launch: x_new in device or
 * PINNED host memory is read by the kernel where it lies (it must stay untouched until the step has run, as for the copy), a
 * pinned, 16-byte aligned out_host is written by the kernel itself; pageable memory is copied.  Same results either way.
 * Alignment: tape, x_new, out and out_host at any float, state at any double.  The one-launch step needs a 16-byte aligned `out`
 * (and, to write out_host itself, a 16-byte aligned out_host): with another `out` the step is the copy, the exec -- through the
 * plan's staging, as hssfsst_exec -- and the merge-and-normalise launch; another out_host is filled by a copy.  Same bits. */
int hssfsst_stream_step(hssfsst_plan* plan, float* tape, int64_t tape_len, int64_t pos, const float* x_new,
                        int64_t x_stride, int x_on_device, int channels, int chunk, float* out, double* state,
                        float* out_host, void* stream);

/* Host helper, no device needed: parser for the corpus files read by DavidSpringerHSS._load_file
 * (hss/datasets/heart_sounds.py:193-197: pd.read_csv(skiprows=1, names=["Signals", "Labels"])):
 * text = the whole file; the first line is skipped; every following non-empty line is
 * "<float>,<number>" (second column read as a number and truncated to int64, as pandas+torch do for
 * integral label columns).  Fills at most `cap` rows; returns the number of data rows in the file
 * (call once with cap = 0 to size the buffers) or a negative status on a malformed line. */
int64_t hssfsst_parse_signal_csv(const char* text, int64_t len, float* signals, int64_t* labels, int64_t cap);

/* Host helper of the batched dataset builder (/root/reference/hss/datasets/heart_sounds.py:155-169 +
 * hss/utils/preprocess.py:30-58, many recordings per call): copies `count` host recordings (float32, contiguous, lens[i]
 * samples at ptrs[i]) back to back into `stage` and writes the start, inside `stage`, of every frame frame_signal would
 * emit for them -- L = floor((T - n) / stride) frames i * stride, or ONE frame at 0 when L <= 0 (the caller has already
 * dropped recordings shorter than n) -- into `starts` (capacity starts_cap).  Uses up to `threads` host threads for the
 * copies (<= 0: one per 4 MB, at most 8).  Returns the number of frames written, or a negative status. */
int64_t hssfsst_pack_recordings(const float* const* ptrs, const int64_t* lens, int64_t count, int stride, int n,
                                float* stage, int64_t stage_cap, int64_t* starts, int64_t starts_cap, int threads);

/* Host helper, no device needed: replaces Resample.__call__ (hss/transforms/resample.py:13-21), i.e.
 * scipy.signal.resample(x, num) for a real 1-D sequence (Fourier method, window=None): y[0..num) from x[0..n).
 * Used by the dataset for the label path (hss/datasets/heart_sounds.py:202-207: round(Resample(y)) - 1). */
int hssfsst_resample(const double* x, int64_t n, int64_t num, double* y);

/* Device counterpart of hssfsst_resample (Resample.__call__, hss/transforms/resample.py:13-21) for BATCHES of signals:
 * scipy.signal.resample(x, num) for real x of n samples, computed in fp64 on the device whatever the input / output dtypes
 * (Bluestein convolutions on power-of-two FFTs, csrc/fourier_resample_gpu.hpp).  A resample plan holds what depends only on
 * (n, num): chirps, the convolution kernels' spectra, the twiddle table; it is single-stream and single-thread like the
 * transform's plan.  n < 1, num < 1 or a NULL `out` give HSSFSST_EINVAL before any device is touched; lengths above 2^26
 * samples HSSFSST_EUNSUPPORTED. */
typedef struct hssfsst_resample_plan hssfsst_resample_plan;
int hssfsst_resample_plan_create(hssfsst_resample_plan** out, int device, int64_t n, int64_t num);
int hssfsst_resample_plan_destroy(hssfsst_resample_plan* plan);

/* Plan geometry: the lengths, the two convolution lengths (powers of two >= 2n - 1 and >= 2num - 1) and the tier its execs
 * take: lds_tier = 1 when both fit one workgroup's LDS (<= 8192 points: one launch per exec), 0 for the multi-pass tier
 * through global scratch (whole recordings).  Any output pointer may be NULL. */
int hssfsst_resample_plan_info(const hssfsst_resample_plan* plan, int64_t* n, int64_t* num, int* m1, int* m2, int* lds_tier,
                               int* device);

/* y[b][0 .. num) = resample(signal b) for `batch` signals of the plan's n samples, read from ONE buffer x of x_len samples
 * (x_dtype HSSFSST_DTYPE_F32 / F64):
 *   starts == NULL: signal b = x + b * x_stride (x_stride < n: overlapping frames of one recording, read in place, as
 *                   hssfsst_exec_frames); (batch - 1) * x_stride + n <= x_len;
 *   starts != NULL: signal b = x + starts[b] (as hssfsst_exec_list); 0 <= starts[b] <= x_len - n, checked when `starts` is host
 *                   memory (starts_on_device = 0), trusted when it is device memory.
 * y: [batch][num] of y_dtype (the fp64 result cast), or NULL.  labels: int64 [batch][num], or NULL: the dataset's label rule
 * round(Resample(y)) - 1 (hss/datasets/heart_sounds.py:205-206), i.e. the fp64 result cast to float32, rounded half to even,
 * minus 1.  At least one of y / labels.  x_on_device / out_on_device (for y and labels alike): 1 = device pointers on the plan's
 * device, 0 = host pointers, staged through the plan's device buffers.  Enqueued on `stream` (hipStream_t, NULL = default)
 * without synchronising when every buffer is on the device; with a host buffer the call returns when the results are in
 * place.
 * Alignment: x, y, labels and starts at any element of their types, host or device (the kernels move one element at a time). */
int hssfsst_resample_exec(hssfsst_resample_plan* plan, const void* x, int x_dtype, int64_t x_len, int64_t x_stride,
                          const int64_t* starts, int starts_on_device, int64_t batch, int x_on_device,
                          void* y, int y_dtype, int64_t* labels, int out_on_device, void* stream);

/* Ragged resampling: a LIST of signals of different lengths, every one resampled to `num` samples in one call (the reference's
 * lazy dataset with Compose([Resample(num), FSST(...)]) resamples each whole recording, hss/datasets/heart_sounds.py:175-184,199-212).
 * A ragged plan holds only what depends on num (the inverse chirp and its spectrum, the twiddle table); the forward tables of
 * every length are made on the device per call, in fp64 (csrc/fourier_resample_ragged.hpp), one per distinct length.
 * hssfsst_resample_plan_info reports n = 0 and m1 = 0 for it.  num < 1 or device < 0: HSSFSST_EINVAL; num > 2^26:
 * HSSFSST_EUNSUPPORTED (both before any device is touched). */
int hssfsst_resample_plan_create_ragged(hssfsst_resample_plan** out, int device, int64_t num);

/* y[i][0 .. num) = resample(x[starts[i] .. starts[i] + lens[i])) for i < count; starts / lens are HOST arrays, x holds x_len
 * samples.  Dtypes, the label rule, host or device buffers, staging and synchronisation as hssfsst_resample_exec.  Each row is
 * within 1e-12 max(|ref|, 1) of hssfsst_resample and of the dense plan of its length (not bit-identical to the dense plan, whose
 * forward table comes from a host FFT), and deterministic: the same bits whatever its neighbours, its place in the list and the
 * chunking.  Argument errors (NULL pointers, lens[i] < 1, a span outside [0, x_len], an unknown dtype, neither y nor labels, a
 * dense plan) return HSSFSST_EINVAL, a length above 2^26 HSSFSST_EUNSUPPORTED, before any device work; count == 0 does nothing.
 * A ragged plan passed to hssfsst_resample_exec returns HSSFSST_EINVAL.
 * Alignment: x, y, labels, starts and lens at any element of their types, as hssfsst_resample_exec. */
int hssfsst_resample_exec_ragged(hssfsst_resample_plan* plan, const void* x, int x_dtype, int64_t x_len, const int64_t* starts,
                                 const int64_t* lens, int64_t count, int x_on_device, void* y, int y_dtype, int64_t* labels,
                                 int out_on_device, void* stream);

/* BiLSTM segmenter, inference only: the forward pass of the reference's HeartSoundSegmenter (hss/model/segmenter.py:70-87) on the
 * device -- lstm_1 (bidirectional, input_size -> 2 x hidden, initial state h0 / c0) -> ReLU -> lstm_2 (2 x hidden -> 2 x hidden,
 * initial state = lstm_1's final (h_n, c_n) per direction) -> ReLU -> Linear(2 x hidden -> 4) -> log_softmax; dropout is the
 * identity (eval mode).  PyTorch's LSTM cell: gate rows i, f, g, o; both biases added; c' = sigmoid(f) c + sigmoid(i) tanh(g),
 * h' = sigmoid(o) tanh(c').  Kernels: csrc/segmenter_lstm.hpp (input projection on the exact f32 matrix instruction; the
 * recurrence as one persistent workgroup per direction and 16 batch rows, recurrent product on split-f16 operands with float32
 * accumulation; no workgroup waits for another one, so a row's result does not depend on its neighbours or the batch size).
 *   lstm_1, lstm_2   eight float32 HOST arrays each, in state_dict order: weight_ih (4 hidden, in), weight_hh (4 hidden, hidden),
 *                    bias_ih (4 hidden), bias_hh (4 hidden) of the forward direction, then the same four of the reverse direction
 *                    (the *_reverse keys); `in` is input_size for lstm_1 and 2 hidden for lstm_2
 *   linear_weight    (4, 2 hidden), linear_bias (4): float32 host arrays
 * The arrays are copied (re-laid out for the kernels) at creation: later changes of the caller's weights do not reach the plan.
 * NULL pointers, input_size < 1, hidden < 1 or device < 0 return HSSFSST_EINVAL, hidden > 256 HSSFSST_EUNSUPPORTED, both before
 * any device is touched.  Single-stream and single-thread like the other plans; its scratch belongs to it: one chunk of projected
 * inputs (at most 128 MiB, or one time step if that is more), both layers' outputs (2 x batch x steps x 2 hidden x 4 bytes) and
 * the carried state, grown on demand and kept.
 * Alignment: every weight array, and the two arrays of pointers, at any element (host memory, read here and not again). */
typedef struct hssfsst_segmenter hssfsst_segmenter;
int hssfsst_segmenter_create(hssfsst_segmenter** out, int device, int input_size, int hidden, const float* const* lstm_1,
                             const float* const* lstm_2, const float* linear_weight, const float* linear_bias);
int hssfsst_segmenter_destroy(hssfsst_segmenter* plan);

/* Plan geometry; max_hidden (the largest supported hidden size) is answered for a NULL plan too, which otherwise is
 * HSSFSST_EINVAL.  Any output pointer may be NULL. */
int hssfsst_segmenter_info(const hssfsst_segmenter* plan, int* input_size, int* hidden, int* max_hidden, int* device);

/* logp (batch, steps, 4) float32 = the model on feats (batch, steps, input_size), contiguous, of feats_dtype HSSFSST_DTYPE_F32 /
 * F16 / BF16 (half features are converted on load: the result is bit-identical to the float32 call on the converted features);
 * h0, c0: (2, batch, hidden) float32.  All DEVICE pointers on the plan's device.  Any batch >= 1, any steps >= 1; the time axis is
 * walked in chunks (forward ascending, reverse descending) with the state carried on the device.  Enqueued on `stream`
 * (hipStream_t, NULL = default) without synchronising.
 * LIMIT: |h0| < 64 in every element (c0: any finite value).  h enters the recurrent product as h x 1024 in float16, which is
 * sized for an LSTM's own |h| < 1; an h0 element of magnitude 64 or more (exactly: from 64 - 2^-6 on) becomes infinite there
 * and its batch row is NaN from the first step on.  Nothing checks this: h0 is device memory and the call does not synchronise.
 * Tested up to +-63.
 * Alignment: feats (of any of the three types), h0 and c0 at any element.  logp must be 16-byte aligned -- a row of four log-probs is
 * one 16-byte store, and the decoders that read it ask the same -- or the call returns HSSFSST_EINVAL ("logp is not 16-byte aligned")
 * before any device work. */
int hssfsst_segmenter_exec(hssfsst_segmenter* plan, const void* feats, int feats_dtype, int64_t batch, int64_t steps,
                           const float* h0, const float* c0, float* logp, void* stream);

/* The same model on a LIST of whole recordings of different lengths in one call -- what hssfsst_exec_ragged's STACK features are:
 * recording i is rows offsets[i] .. offsets[i + 1] of feats (sum T, input_size), and its log-probs land in the same rows of logp
 * (sum T, 4).  offsets: int64 HOST array of count + 1 step offsets, offsets[0] == 0, strictly increasing.  h0, c0: (2, state_rows,
 * hidden) float32 with state_rows == count (recording i starts from row i) or 1 (every recording starts from the same state: the
 * reference model built with batch_size = 1 and fed one recording per step).  feats, h0, c0, logp: DEVICE pointers.  |h0| < 64
 * in every element, as for hssfsst_segmenter_exec (unchecked; a larger one makes its recording NaN).
 * For every i the result is bit-identical to hssfsst_segmenter_exec on that recording alone (batch 1, its own state row): the
 * forward direction from its first step, the reverse direction from its own last step, lstm_2 seeded with lstm_1's state at the
 * recording's own ends.  Padding to (count, T_max) cannot give that.
 * How: recordings are sorted by length into tiles of 16 row slots (csrc/segmenter_layout.hpp), one recurrence workgroup per tile
 * and direction walks the tile's longest recording and rows past their own end freeze (RAGGED instantiations of
 * csrc/segmenter_lstm.hpp); independent tiles fill the device.  The order changes the wasted steps, not the bits.
 * Argument errors return HSSFSST_EINVAL before any device work, the list's before the plan is looked at: count < 0, a NULL
 * pointer, offsets[0] != 0, an offset that does not increase or a recording over the dense call's step limit (the message names
 * the index), more than 2^31 - 1 steps in all, state_rows not in {1, count}, an unknown dtype.  count == 0 does nothing and
 * returns 0.  The device tables are kept while the next call has the same offsets.
 * Scratch (the plan's, grown on demand and kept, shared with hssfsst_segmenter_exec): both layers' outputs, 2 x sum T x 2 hidden
 * x 4 bytes; one chunk of projected inputs, at most 128 MiB, or one step of every tile (128 KiB each) if that is more; the
 * state, 16 KiB per tile.  Enqueued on `stream` without synchronising.
 * Alignment: as hssfsst_segmenter_exec -- feats, h0, c0 at any element, offsets (host) at any int64; logp must be 16-byte aligned, or
 * HSSFSST_EINVAL ("logp is not 16-byte aligned") before any device work, after the list's and the NULL checks. */
int hssfsst_segmenter_exec_ragged(hssfsst_segmenter* plan, const void* feats, int feats_dtype, const int64_t* offsets,
                                  int64_t count, const float* h0, const float* c0, int state_rows, float* logp, void* stream);

/* Viterbi decoding: the segmenter's log-probs -> one state 0..3 (S1, systole, S2, diastole) per step, for a LIST of recordings in
 * one call (csrc/segmenter_decode.hpp; the arithmetic as plain functions: csrc/decode_layout.hpp).  Stateless: no plan.
 *   logp         (sum T, 4) float32 emissions e, DEVICE, 16-byte aligned: what hssfsst_segmenter_exec_ragged writes
 *   offsets      int64 HOST array of count + 1 step offsets, offsets[0] == 0, strictly increasing (as hssfsst_segmenter_exec_ragged)
 *   transitions  A (4, 4) float32, HOST: A[i][j] = log score of moving from state i to state j
 *   initial      pi (4) float32, HOST: log score of starting in state j
 *   states       (sum T) uint8, DEVICE: recording i's path in bytes offsets[i] .. offsets[i + 1]
 *   scores       (count) int64, DEVICE, or NULL: the best path's score in units of 2^-20
 * -inf in e, A or pi means "forbidden".
 * Arithmetic, exact.  Every input value x becomes the int64 q(x) = rint(clamp(x, -32768, +32768) x 2^20), rounding half to even;
 * q(NaN) = q(-32768); +inf clamps to 32768; q(-inf) = NEG, an absorbing element: NEG + anything = NEG, and NEG loses every max.
 * Everything after that is int64 add and max, which is exactly associative: with T <= 2^26 steps of two terms of at most 2^35 no
 * sum exceeds 2^62, and the kernel's chunking gives the sequential loop's result bit for bit:
 *   d_0[j] = q(pi[j]) + q(e[0][j]);   d_t[j] = max_i (d_(t-1)[i] + q(A[i][j])) + q(e[t][j])  for t >= 1;
 *   the backpointer psi_t[j] is the SMALLEST i that attains the max; the end state is the SMALLEST j that attains max_j d_(T-1)[j];
 *   the path follows the backpointers from there; the score is max_j d_(T-1)[j].
 * The caller owns the emissions: with valid A and pi (below) a recording without -inf emissions has an optimal path that uses
 * allowed moves only.  A step whose four emissions are all -inf makes the score NEG (INT64_MIN) and the path the one the tie
 * rule yields (every comparison from there on is a tie): defined, and meaningless.
 * HSSFSST_EINVAL before any device work: a NULL pointer other than scores, count < 0, offsets[0] != 0 or an offset that does not
 * increase (the message names the index), a NaN in transitions or initial, a row of transitions or the whole of initial all -inf
 * (a state without a successor / no state to start in), device < 0, logp not 16-byte aligned.  HSSFSST_EUNSUPPORTED: a recording
 * of more than 2^26 steps (hssfsst_decode_info: max_steps), more than 2^31 - 1 steps in all.  count == 0 returns 0 and does nothing.
 * A recording's result does not depend on its neighbours or its place in the list.  Enqueued on `stream` (hipStream_t, NULL =
 * default) without synchronising: one launch per 256 recordings, one workgroup per recording, no scratch memory -- a step's four
 * backpointers are kept as one byte in `states` itself until the backtrace overwrites it with the state. */
int hssfsst_decode_states(const float* logp, const int64_t* offsets, int64_t count, const float* transitions, const float* initial,
                          uint8_t* states, int64_t* scores, int device, void* stream);

/* The decoder's geometry, no device needed: segment_steps = steps a workgroup stages at a time (a recording is walked in
 * segments of that many steps from its step 1 on), max_steps = the longest recording (2^26).  Either pointer may be NULL. */
int hssfsst_decode_info(int* segment_steps, int64_t* max_steps);

/* Explicit-duration (semi-Markov) Viterbi decoding: hssfsst_decode_states with a score for how long each run of a state lasts,
 * so that a decoded S1 cannot last 3 ms nor a systole 4 s (csrc/segmenter_decode_durations.hpp; the arithmetic, the sequential
 * loop that defines the result bit for bit and the kernel's geometry as plain functions: csrc/decode_durations_layout.hpp).
 * logp, offsets, count, states, scores, device, stream: as for hssfsst_decode_states.  Further
 *   transitions   A (4, 4) float32, HOST: the DIAGONAL IS IGNORED -- a run is never followed by a run of the same state
 *   initial       pi (4) float32, HOST
 *   durations     dur (4, max_duration) float32, HOST: dur[j][d - 1] = log score of an interior run of state j lasting d steps
 *   edge          (4, max_duration) float32, HOST: the same for the first and the last run of a recording, which its ends cut off
 *   max_duration  D, 1 .. 2048 (hssfsst_decode_durations_info): no run is longer
 *   workspace     DEVICE, 16-byte aligned, workspace_bytes >= workspace_bytes_per_step x (sum T + 8 D): the quantised tables
 *                 (64 D bytes) and a step's four 16-bit duration backpointers (8 bytes); contents undefined afterwards
 * A recording of T steps is cut into runs (s_1, d_1) .. (s_K, d_K), sum d_k = T, 1 <= d_k <= D, s_k != s_(k+1); its score is
 *   q(pi[s_1]) + sum_k len_k + sum_k q(A[s_k][s_(k+1)]) + sum_t qe(e[t][s(t)]),
 * len_k = q(edge[s_k][d_k]) for k = 1 and k = K (once when K = 1), q(dur[s_k][d_k]) otherwise.  q is hssfsst_decode_states'
 * quantiser and -inf in pi, A, dur, edge means "forbidden".  THE EMISSIONS DIFFER from hssfsst_decode_states: qe(x) = q(x) except
 * that -inf and NaN count as -32768 -- the decoder works on prefix sums of the emissions, and an absorbing element cannot sit
 * inside one.  Everything after the quantisers is int64 add and max: with T <= 2^24 steps no sum exceeds 2^62 (at most 4 T + 3
 * terms of 2^35), and the result is decode_durations_reference()'s, the best segmentation with ties to the smallest duration,
 * then the smallest predecessor state, at the end to the smallest state, then the smallest duration.  A recording that no
 * segmentation fits (e.g. T > D under an edge table that allows nothing) gets the score NEG (INT64_MIN) and the state 0 at
 * every step.  The result does not depend on the smallest allowed duration: dur[j][0] may be finite.
 * HSSFSST_EINVAL before any device work: a NULL pointer other than scores, count < 0, bad offsets (as hssfsst_decode_states), a
 * NaN in any table (the message names the entry), max_duration outside 1 .. 2048, a row of durations or edge all -inf, a row of
 * transitions with no finite off-diagonal entry, initial all -inf, device < 0, logp or workspace not 16-byte aligned, a workspace
 * that is too small.  HSSFSST_EUNSUPPORTED: a recording of more than 2^24 steps, more than 2^31 - 1 steps in all.  count == 0
 * returns 0 and does nothing.
 * A recording's result does not depend on its neighbours or its place in the list.  Enqueued on `stream` without synchronising
 * and without a copy from host memory (the tables travel as kernel arguments): ceil(8 D / 896) small launches that fill the
 * tables, then one launch per 256 recordings, one workgroup of 512 lanes per recording, 102 KiB of LDS, no scratch memory. */
int hssfsst_decode_durations(const float* logp, const int64_t* offsets, int64_t count, const float* transitions, const float* initial,
                             const float* durations, const float* edge, int max_duration, uint8_t* states, int64_t* scores,
                             void* workspace, int64_t workspace_bytes, int device, void* stream);

/* Its limits, no device needed: max_duration = the largest D (2048), max_steps = the longest recording (2^24),
 * workspace_bytes_per_step = 8.  Any pointer may be NULL. */
int hssfsst_decode_durations_info(int* max_duration, int64_t* max_steps, int64_t* workspace_bytes_per_step);

/* Forward-backward under the transition model of hssfsst_decode_states: the smoothed counterpart of the Viterbi path, for a LIST
 * of recordings in one call (csrc/segmenter_posteriors.hpp; the arithmetic, the sequential loop that is the specification and the
 * kernel's geometry as plain functions: csrc/posterior_layout.hpp).  Stateless: no plan.  logp, offsets, count, device, stream: as
 * for hssfsst_decode_states.  Further
 *   a_pi     20 float32, DEVICE, 4-byte aligned: A (4, 4) row-major, then pi (4); -inf = forbidden; read by the kernel, so a
 *            learnable table costs no host synchronisation.  Entries must be -inf or below ~700 (exp in float64); unchecked
 *   labels   (sum T) uint8, DEVICE, or NULL: a state 0..3 per step (only the two low bits are looked at)
 *   gamma    (sum T, 4) float32, DEVICE, 16-byte aligned: gamma_t[j] = P(state_t = j | the whole recording, A, pi); WITH labels
 *            gamma - onehot(labels) instead, the gradient of logZ - score in the emissions
 *   loglik   (count) float64, DEVICE: logZ = log of the sum over all 4^T paths of exp w(path),
 *            w(path) = pi[s_0] + sum_t e[t][s_t] + sum_(t >= 1) A[s_(t-1)][s_t]  (the diagonal of A counts)
 *   score    (count) float64, DEVICE, or NULL: w(labels); needs labels
 *   xi       (count, 16) float64, DEVICE, or NULL: Xi[i][j] = sum_(t >= 1) P(s_(t-1) = i, s_t = j | ...), the expected transition
 *            counts (the gradient of logZ in A); WITH labels Xi - counts(labels)
 *   gamma0   (count, 4) float64, DEVICE, or NULL: row offsets[i] of gamma before its rounding to float32 -- the step-0 posteriors,
 *            the gradient of logZ in pi (WITH labels minus onehot(labels[0])); it may as well be read from gamma in float32
 *   work     DEVICE, 16-byte aligned, work_bytes >= work_bytes_per_step x sum T + work_bytes_per_recording x count
 *            (hssfsst_posteriors_info); contents undefined afterwards
 * Arithmetic: float64 in the linear domain, gamma rounded to float32 at the end.  With b_t[j] = exp(e[t][j] - max_j e[t][j]),
 * P = exp(A), p0 = exp(pi) every running vector and 4 x 4 transfer matrix is a float64 mantissa with an integer exponent,
 * renormalised by an exact power of two after every step and every product; there is no subtraction, and gamma and the terms of
 * Xi are normalised per step.  logZ = log sum_j alpha_(T-1)[j] + exponent ln 2 + sum_t max_j e[t][j].
 * THE LIMIT: a path whose weight falls more than about 700 nats (float64 underflow) below the best path reaching the same step is
 * dropped.  Emissions within 200 of their step's maximum can never trigger this with four states (3 x 200 < 708); a float32
 * log_softmax stays within about 104.  NaN emissions count as -inf.  A recording with Z = 0 (e.g. a step whose four emissions are
 * -inf) gets logZ = -inf, gamma = 0 and Xi = 0 (minus the labels' terms when labels are given).
 * HSSFSST_EINVAL before any device work: a NULL pointer other than labels, score, xi, gamma0; labels NULL while score is not; count < 0;
 * bad offsets (as hssfsst_decode_states); device < 0; logp, gamma or work not 16-byte aligned, a_pi not 4-byte, loglik, score, xi or
 * gamma0 not 8-byte aligned; a work that is too small.  HSSFSST_EUNSUPPORTED: a recording of more than 2^20 steps, more than 2^31 - 1
 * steps in all.  count == 0 returns 0 and does nothing.
 * A recording's outputs do not depend on its neighbours or its place in the list, bit for bit, and two calls give the same bits.
 * Enqueued on `stream` without synchronising: one launch per 256 recordings, one workgroup of 256 lanes per recording (a single
 * long recording uses one CU), 70 KiB of LDS, no scratch memory. */
int hssfsst_posteriors(const float* logp, const int64_t* offsets, int64_t count, const float* a_pi, const uint8_t* labels, float* gamma,
                       double* loglik, double* score, double* xi, double* gamma0, void* work, int64_t work_bytes, int device, void* stream);

/* Its geometry and limits, no device needed: segment_steps = steps a workgroup stages at a time (2048 = 256 lanes x 8 steps; a
 * recording is walked in segments from its step 1 on), max_steps = the longest recording (2^20), and the two factors of the
 * workspace size.  Any pointer may be NULL. */
int hssfsst_posteriors_info(int* segment_steps, int64_t* max_steps, int64_t* work_bytes_per_step, int64_t* work_bytes_per_recording);

/* Forward-backward under the explicit-duration (semi-Markov) model of hssfsst_decode_durations, un-quantised: the sum over all
 * segmentations where the decoder takes the best one (csrc/segmenter_duration_posteriors.hpp; the arithmetic, the sequential loop
 * that is the specification and the kernel's geometry as plain functions: csrc/duration_posterior_layout.hpp).  Stateless.  logp,
 * offsets, count, labels, loglik, work, device, stream: as for hssfsst_posteriors.  Further
 *   a_pi          20 float32, DEVICE: A (4, 4) row-major, then pi (4); the DIAGONAL of A IS IGNORED; -inf (or NaN) = forbidden
 *   durations     dur (4, max_duration) float32, DEVICE: dur[j][d - 1] = log score of an interior run of state j lasting d steps
 *   edge          (4, max_duration) float32, DEVICE: the same for the first and the last run of a recording
 *   max_duration  D, 1 .. 2048
 *   gamma         (sum T, 4) float32, DEVICE, 16-byte aligned: gamma_t[j] = P(state_t = j | the recording, the tables), clamped to
 *                 [0, 1]; WITH labels gamma - onehot(labels)
 *   onsets        (sum T, 4) float32, DEVICE, 16-byte aligned, or NULL: S_t[j] = P(a run of j starts at step t | ...); never changed
 *                 by labels
 *   score         (count) float64, DEVICE, or NULL: the log weight of the labelled segmentation (the runs of equal labels), -inf if
 *                 a labelled run is longer than D or uses a forbidden entry; needs labels
 *   xi            (count, 16) float64, DEVICE, or NULL: Xi[i][j] = the expected number of run changes i -> j (diagonal 0), the
 *                 gradient of logZ in A; WITH labels Xi - counts(label runs)
 *   s0            (count, 4) float64, DEVICE, or NULL: S_0, the step-0 posterior, the gradient of logZ in pi; WITH labels minus
 *                 onehot(labels[0])
 *   work          DEVICE, 16-byte aligned, work_bytes >= work_bytes_per_step x sum T + work_bytes_per_recording x count +
 *                 work_bytes_per_duration x D (hssfsst_posteriors_durations_info); contents undefined afterwards
 * The weight of a segmentation (s_1, d_1) .. (s_K, d_K) is hssfsst_decode_durations' without the quantiser:
 *   pi[s_1] + sum_k len_k + sum_k A[s_k][s_(k+1)] + sum_t e[t][s(t)],  len_k = edge for k = 1 and k = K, dur otherwise,
 * and an emission of -inf or NaN counts as -32768 (the decoder's rule).  logZ is the log of the sum of exp(weight).
 * Arithmetic: linear domain; every quantity is a float64 mantissa with a 32-bit exponent, exp(x) enters as the floor of x / ln 2 and the exponential
 * of what is left (a fixed polynomial, the same bits on host and device), sums align exponents with ldexp, the order of every sum is fixed (the sources of a ring word arrive in order
 * of falling duration).  THE LIMITS: the prefix sums sum_(u<t) e[u][j] must stay within +-3.7e8 (emissions within +-350 at 2^20
 * steps; at most ~11 000 -inf / NaN emissions of one state in a recording), and the relative error of the outputs grows with
 * |prefix sum| x 2^-53.  Nothing else underflows.  A recording no segmentation fits gets logZ = -inf, gamma = 0, Xi = 0.
 * HSSFSST_EINVAL before any device work: a NULL pointer other than labels, onsets, score, xi, s0; labels NULL while score is not;
 * count < 0; bad offsets; max_duration outside 1 .. 2048; device < 0; logp, gamma, onsets or work not 16-byte aligned, a table not
 * 4-byte, loglik, score, xi or s0 not 8-byte aligned; a work that is too small.  HSSFSST_EUNSUPPORTED: a recording of more than
 * 2^20 steps, more than 2^31 - 1 steps in all.  count == 0 returns 0 and does nothing.  The tables' values are not checked.
 * A recording's outputs do not depend on its neighbours or its place in the list, bit for bit, and two calls give the same bits.
 * Enqueued on `stream` without synchronising and without reading a table on the host: one small launch that turns dur and edge
 * into the linear tables at the head of the workspace, then one launch per 256 recordings, one workgroup of 512 lanes per recording
 * (a single long recording uses one CU; each step costs O(4 D) twice), 129 KiB of LDS, no scratch memory. */
int hssfsst_posteriors_durations(const float* logp, const int64_t* offsets, int64_t count, const float* a_pi, const float* durations,
                                 const float* edge, int max_duration, const uint8_t* labels, float* gamma, float* onsets, double* loglik,
                                 double* score, double* xi, double* s0, void* work, int64_t work_bytes, int device, void* stream);

/* Its geometry and limits, no device needed: max_duration = the largest D (2048), segment_steps = steps staged at a time (256),
 * max_steps = the longest recording (2^20), and the three factors of the workspace size (49, 32, 96).  Any pointer may be NULL. */
int hssfsst_posteriors_durations_info(int* max_duration, int* segment_steps, int64_t* max_steps, int64_t* work_bytes_per_step,
                                      int64_t* work_bytes_per_recording, int64_t* work_bytes_per_duration);

/* hssfsst_posteriors_durations, and with it the sufficient statistic of the two duration tables: the expected run-length counts
 * (csrc/segmenter_duration_counts.hpp; arithmetic, ownership, workspace and the sequential loop that is the specification:
 * csrc/duration_counts_layout.hpp).  The 18 arguments of hssfsst_posteriors_durations, with the same meaning and the same bits in
 * every one of its outputs, and before work
 *   counts        (count, 2, 4, max_duration) float64, DEVICE, 8-byte aligned, required:
 *                 counts[i][0][j][d - 1] = E[number of INTERIOR runs of state j lasting exactly d steps | recording i, the tables],
 *                 counts[i][1][j][d - 1] = the same for the first and the last run (those edge scores) -- the gradients of logZ in
 *                 durations and in edge, the E-step of the explicit-duration Baum-Welch; WITH labels counts - counts(label runs):
 *                 a labelled run of d <= max_duration steps takes 1 off its entry, a longer one (score = -inf) takes nothing off.
 *                 THE COST: 64 x max_duration bytes per recording -- 128 KiB per recording at max_duration 2048, 100 MiB for 792
 *                 recordings -- whatever their lengths.
 *   work          as there, with the factors of hssfsst_posteriors_durations_counts_info (97, 48, 96): the sweeps also leave
 *                 g_u (48 bytes a step) and 1 / Z
 * The posterior of the run of j that starts at step t and lasts d steps is b_t(j) L(j, d) g_(t+d)(j) / Z in the notation of
 * csrc/duration_posterior_layout.hpp; each term is formed in the scaled arithmetic and added to a float64 sum in order of
 * ascending t.  A recording no segmentation fits (Z = 0) gets counts 0 (minus the labels' terms).  Errors: those of
 * hssfsst_posteriors_durations, before any device work; counts NULL or not 8-byte aligned: HSSFSST_EINVAL.
 * A recording's counts do not depend on its neighbours or its place in the list, bit for bit, and two calls give the same bits:
 * no atomics, no partial sums.  Enqueued on `stream` without synchronising: the fill launch, one sweep launch per 256 recordings
 * (seg_duration_runs_sweep_kernel, the same two sweeps), then one counts launch per 256 recordings with one workgroup of 512 lanes
 * per recording and block of 128 durations -- lane l for state l mod 4 and one duration, the steps walked in ascending order in
 * segments of 256 --, 55 KiB of LDS, no scratch memory. */
int hssfsst_posteriors_durations_counts(const float* logp, const int64_t* offsets, int64_t count, const float* a_pi, const float* durations,
                                        const float* edge, int max_duration, const uint8_t* labels, float* gamma, float* onsets,
                                        double* loglik, double* score, double* xi, double* s0, double* counts, void* work, int64_t work_bytes,
                                        int device, void* stream);

/* Its three workspace factors (bytes per step 97, per recording 48, per duration 96) and the durations one workgroup of the counts
 * launch covers (128); the other limits are hssfsst_posteriors_durations_info's.  No device needed; any pointer may be NULL. */
int hssfsst_posteriors_durations_counts_info(int64_t* work_bytes_per_step, int64_t* work_bytes_per_recording, int64_t* work_bytes_per_duration,
                                             int* durations_per_group);

/* Where a call runs: the device and the stream (hipStream_t, NULL = default) that every launch and every clear of the call is
 * enqueued on.  hssfsst_score_states takes the pair as a struct, where the entries above take `int device, void* stream`: the
 * stream-order suite holds every function of this header with a `void* stream` parameter to one table of cases in
 * tests/test_stream_order.py, and the cases of this entry live in tests/test_segmentation_scores.py, which holds every function
 * with a `const hssfsst_launch*` parameter to the same two scenarios on a side stream.  The promise is the same one.
 * hssfsst_stitch_windows takes the struct BY VALUE for the same reason once more: both of those files are closed tables, and an
 * entry of either shape without a case in them fails them.  tests/test_stitch_windows.py holds every function of this header with
 * a by-value `hssfsst_launch` parameter to the two scenarios, and fails for one without a case there. */
typedef struct { int device; void* stream; } hssfsst_launch;

/* Scoring a segmentation on the device: confusion counts and the exact rank statistic behind the one-vs-rest AUROC, for a LIST of
 * recordings in one call, every result an exact integer (csrc/segmenter_score.hpp; the key transform, the sort's partition, the
 * workspace and the sequential loop that is the specification as plain functions: csrc/score_layout.hpp).  Stateless: no plan.
 *   logp           (sum T, 4) float32, DEVICE, 16-byte aligned, or NULL: a score per step and class (the segmenter's log-probs,
 *                  posteriors ...)
 *   states         (sum T) uint8, DEVICE, or NULL: the predicted state per step, as the decoders write it.  At least one of logp
 *                  and states; with both, states are the predictions and logp the scores that are ranked.  With logp alone the
 *                  prediction is the argmax of the step's four values, ties to the smaller state, NaN read as -inf
 *   labels         (sum T) uint8, DEVICE: 0..3 is a state; ANY OTHER VALUE (255, say) marks the step IGNORED: it is left out of
 *                  every count and of the ranking and counted in `ignored`.  So is a step whose states[t] is above 3
 *   offsets, count as for hssfsst_decode_states (HOST); no limit on a recording's length, 2^31 - 1 steps in all
 *   per_recording  0: one result for the whole call, all steps pooled (groups = 1); else one per recording (groups = count)
 *   confusion      (groups, 4, 4) int64, DEVICE, 8-byte aligned: [label][predicted] over the counted steps
 *   ignored        (groups) int64, DEVICE: the steps left out
 *   rank           (groups, 4, 3) int64, DEVICE, or NULL; needs logp.  Per class c: {2U, P, N}.  P and N are the numbers of counted
 *                  steps whose label is / is not c, and with s = column c of logp
 *                      2U = sum over (positive p, negative n) of 2 [s_p > s_n] + [s_p == s_n]
 *                  in float32's order, -0 == +0, -inf lowest, NaN read as -inf; 2U <= 2 P N <= 2^61.  The one-vs-rest AUROC is
 *                  2U / (2 P N), undefined where P N = 0: the kernels do not divide.  per_recording: each recording's steps are
 *                  ranked among themselves only.  Pooled, the whole call is ranked together: NOT the sum of the recordings' ranks
 *   work           DEVICE, 16-byte aligned, or NULL when rank is: work_bytes >= work_bytes_per_step x sum T + work_bytes_constant
 *                  (hssfsst_score_info: 17 bytes per step -- two buffers of 8-byte items and the digit histograms); contents
 *                  undefined afterwards
 *   where          HOST, read during the call
 * The rank of a class: every step becomes a 64-bit item (recording, order-preserving key of the score, is-positive bit), the items
 * are sorted by a least-significant-digit radix sort of 8 bits per pass -- 4 passes pooled, ceil((32 + bits of count - 1) / 8)
 * per recording, decided on the host --, and the sorted order is scanned for tie groups: 2U = sum_g P_g (2 N_below(g) + N_g).
 * HSSFSST_EINVAL before any device work: a NULL labels, offsets, confusion, ignored or where; states and logp both NULL; rank without
 * logp or without work; count < 0; bad offsets (as hssfsst_decode_states); where->device < 0; logp or work not 16-byte aligned,
 * confusion, ignored or rank not 8-byte aligned; a work that is too small.  HSSFSST_EUNSUPPORTED: more than 2^31 - 1 steps in
 * all.  count == 0 returns 0 and does nothing.
 * All integers: two calls give the same bits, and a recording's per-recording results do not depend on its neighbours or its
 * place in the list.  Enqueued on where->stream without synchronising: three clears, one counts launch per 256 recordings, and
 * per class one key launch per 256 recordings, five launches per pass (histogram per block of 2048 items, three for the scan,
 * scatter) and three for the rank.  No workgroup waits for another; at most 19 KiB of LDS; no scratch memory. */
int hssfsst_score_states(const float* logp, const uint8_t* states, const uint8_t* labels, const int64_t* offsets, int64_t count,
                         int per_recording, int64_t* confusion, int64_t* ignored, int64_t* rank, void* work, int64_t work_bytes,
                         const hssfsst_launch* where);

/* Its workspace factors (bytes per step 17, per recording 0, constant 4096) and the sort's geometry: block_items = the items one
 * wave histograms and scatters (2048), digit_bits = 8, max_passes = 8.  No device needed; any pointer may be NULL. */
int hssfsst_score_info(int64_t* work_bytes_per_step, int64_t* work_bytes_per_recording, int64_t* work_bytes_constant, int* block_items,
                       int* digit_bits, int* max_passes);

/* Stitching: the log-probs of OVERLAPPING WINDOWS of a list of recordings -> one sequence of log-probs per recording, so that a
 * model trained on n-step windows segments whole recordings window by window (csrc/segmenter_stitch.hpp; the window set, the
 * arithmetic of a step and the sequential loop that is the specification as plain functions: csrc/stitch_layout.hpp).  Stateless.
 * The window set of a recording of T >= 1 steps, windows of n steps at stride 1 <= stride <= n, covers every step:
 *   T <= n   one window [0, T)
 *   T >  n   the floor((T - n) / stride) + 1 regular windows [i stride, i stride + n) and, if (T - n) % stride != 0, one tail
 *            window [T - n, T)
 *   win_logp     (win_steps, 4) float32, DEVICE, 16-byte aligned: the windows' log-probs; a full window takes n rows, the single
 *                window of a T <= n recording T rows
 *   win_first    (count) int64, HOST: recording i's windows lie back to back, in ascending start order, from row win_first[i] on;
 *                the blocks of different recordings may lie anywhere in the arena, in any order
 *   win_steps    the arena's rows: every block must end within them
 *   offsets, count as for hssfsst_decode_states (HOST): the OUTPUT recordings; no limit on a recording's length
 *   n, stride    n >= 1, 1 <= stride <= n, ceil(n / stride) <= 15: a step has at most 16 covering windows
 *   weights      (n) float32, DEVICE, or NULL (all ones): w[p] > 0 weighs position p of a window; the short window of a T <= n
 *                recording uses w[0 .. T).  The values are device memory and are not checked
 *   mode         HSSFSST_STITCH_PROB, _LOGP or _SELECT
 *   out          (sum T, 4) float32, DEVICE, 16-byte aligned
 *   dissent      (sum T) uint8, DEVICE, or NULL: how many of the step's covering windows have an argmax other than that of out[t];
 *                the argmax is hssfsst_score_states': ties to the smaller state, NaN read as -inf
 *   where        the device and the stream, by value
 * Arithmetic.  The covering windows of step t in ascending start order are k = 1 .. m; window k gives the row v_k at its position
 * p_k, with weight w_k = w[p_k].  m == 1, or SELECT: a row is copied bit for bit; SELECT takes the largest w_k, ties to the earlier
 * start.  PROB: with M the largest of the 4 m values, a_j = log(sum_k w_k exp(v_kj - M) / sum_k w_k) + M, the weighted mean of the
 * probabilities.  LOGP: a_j = sum_k w_k v_kj / sum_k w_k, the weighted geometric mean.  Both: out_j = a_j - logsumexp_j(a), in
 * float64, the sums over k in ascending start order, rounded to float32 once.  IEEE rules do the rest: a NaN among a step's values
 * makes its four outputs NaN; a class that is -inf in every covering window (PROB) or in any (LOGP) comes out -inf; a step with no
 * mass at all gets four NaN.
 * HSSFSST_EINVAL before any device work: a NULL win_logp, win_first, offsets or out; count < 0; win_steps < 0; n < 1; stride outside
 * 1 .. n; an unknown mode; where.device < 0; win_logp or out not 16-byte aligned, weights not 4-byte; bad offsets (as
 * hssfsst_decode_states); a win_first[i] that is negative or whose block ends past win_steps.  HSSFSST_EUNSUPPORTED: more than
 * 2^31 - 1 steps in all; ceil(n / stride) > 15.  count == 0 returns 0 and does nothing.
 * A recording's result does not depend on its neighbours or its place in the list, bit for bit, and two calls give the same bits.
 * Enqueued on where.stream without synchronising and without a copy from host memory: one launch per 256 recordings (offsets and
 * win_first travel as kernel arguments), one lane per step, no atomics, no LDS, no scratch memory. */
#define HSSFSST_STITCH_PROB 0
#define HSSFSST_STITCH_LOGP 1
#define HSSFSST_STITCH_SELECT 2
int hssfsst_stitch_windows(const float* win_logp, const int64_t* win_first, int64_t win_steps, const int64_t* offsets, int64_t count,
                           int n, int stride, const float* weights, int mode, float* out, uint8_t* dissent, hssfsst_launch where);

/* One DIFFERENTIABLE bidirectional LSTM layer (batch first, nn.LSTM's cell and gate order): the unit a training program stacks
 * under autograd -- the segmenter is two of them.  The plan holds the layer's current weights in the kernels' layouts and the
 * scratch of its calls; the caller owns inputs, outputs and the stash.  Every pointer below is a DEVICE pointer on the plan's
 * device unless marked host; float32.  Kernels: csrc/segmenter_train.hpp.  Every call is enqueued on
 * `stream` without any host synchronisation.  Single-stream and single-thread like the other plans.
 *   create       input_size < 1, hidden < 1, device < 0 or a NULL out: HSSFSST_EINVAL; hidden > 256: HSSFSST_EUNSUPPORTED; both
 *                before any device is touched.
 *   set_weights  weights: HOST array of 8 device pointers in state_dict order (weight_ih (4 hidden, input_size), weight_hh
 *                (4 hidden, hidden), bias_ih, bias_hh (4 hidden) of the forward direction, then of the reverse one).  Packs them on
 *                the device into the forward kernels' tables (the arithmetic of hssfsst_segmenter_create, scale included) and the
 *                split-bf16 operand stream of the backward product.  Call it again whenever the weights changed; forward and
 *                backward before the first call return HSSFSST_EINVAL.
 *   stash_floats floats <- the float32 elements of the stash of a (batch, steps) forward: 2 x ceil(batch / 16) x steps x 20480
 *                (80 KiB per direction, 16 rows and step; 1.3 GB at batch 50 x 2000 steps).  Host only; the plan may be NULL.
 *   forward      y (batch, steps, 2 hidden), hn, cn (2, batch, hidden) <- the layer on x (batch, steps, input_size) from h0, c0
 *                (2, batch, hidden), by the projection and recurrence kernels of hssfsst_segmenter_exec.  Every step's
 *                activated gates and cell state go to `stash`, which the caller keeps until the backward call.  |h0| < 64 in
 *                every element, as for hssfsst_segmenter_exec (unchecked; a larger one makes its row NaN, gradients included).
 *   backward     dy (batch, steps, 2 hidden), dhn, dcn (2, batch, hidden; NULL = zero): the gradients of y, hn, cn.  Writes
 *                dgates (2, batch, steps, 4 hidden) -- per direction the gradient of the pre-activation gates i, f, g, o, from
 *                which the weight, bias and input gradients are plain matrix products -- and dh0, dc0 (2, batch, hidden).  The
 *                recurrent product dgates . W_hh runs on split-bf16 operands (hi.hi + hi.lo + lo.hi) with float32 accumulation.
 *                The plan's weights must still be those of the forward call.
 * NULL pointers, batch < 1 or steps < 1 and sizes over the limits of hssfsst_segmenter_exec return HSSFSST_EINVAL before any
 * device work.
 * Alignment: every tensor -- the weight arrays behind set_weights' table, x, h0, c0, y, hn, cn, dy, dhn, dcn, dgates, dh0, dc0 -- at any
 * float: the kernels read and write them one element at a time.  The stash must be 16-byte aligned in forward and backward, dense
 * and ragged -- it is moved 16 bytes at a time -- or the call returns HSSFSST_EINVAL ("stash is not 16-byte aligned") before any
 * device work.  Forward writes, and backward reads, exactly the first stash_floats (stash_floats_ragged) floats of it. */
typedef struct hssfsst_bilstm hssfsst_bilstm;
int hssfsst_bilstm_create(hssfsst_bilstm** out, int device, int input_size, int hidden);
int hssfsst_bilstm_destroy(hssfsst_bilstm* plan);
int hssfsst_bilstm_set_weights(hssfsst_bilstm* plan, const float* const* weights, void* stream);
int hssfsst_bilstm_stash_floats(const hssfsst_bilstm* plan, int64_t batch, int64_t steps, int64_t* floats);
int hssfsst_bilstm_forward(hssfsst_bilstm* plan, const float* x, int64_t batch, int64_t steps, const float* h0, const float* c0,
                           float* y, float* hn, float* cn, float* stash, void* stream);
int hssfsst_bilstm_backward(hssfsst_bilstm* plan, const float* stash, const float* c0, const float* dy, const float* dhn,
                            const float* dcn, int64_t batch, int64_t steps, float* dgates, float* dh0, float* dc0, void* stream);

/* The same layer on a LIST of whole recordings of different lengths, one call per pass: recording i is rows offsets[i] ..
 * offsets[i + 1] of the arenas x (sum T, input_size), y and dy (sum T, 2 hidden) and dgates (2, sum T, 4 hidden); h0, c0, hn, cn,
 * dhn, dcn, dh0, dc0 are (2, count, hidden) in list order.  offsets: int64 HOST array of count + 1 step offsets, offsets[0] == 0,
 * strictly increasing -- the list of hssfsst_segmenter_exec_ragged, checked the same way with the same messages, before the plan
 * is looked at; count == 0 does nothing and returns 0.  For every i, y, hn, cn, dgates, dh0, dc0 are bit-identical to the dense
 * calls on that recording alone (batch 1): forward from its first step, reverse from its own last one.
 * How: the slots and tiles of csrc/segmenter_layout.hpp (longest first, 16 per tile); a tile's workgroups walk its longest
 * recording, forwards in the forward pass and back down in the backward pass, and rows past their own end are held by selects
 * (RAGGED instantiations of csrc/segmenter_lstm.hpp and csrc/segmenter_train.hpp).  The stash is indexed by (tile, step walked):
 *   stash_floats_ragged  floats <- 2 x (sum over tiles of the tile's longest recording) x 20480 (80 KiB per direction, tile and
 *                        step: 5.8 GB for one tile of 35 500-step recordings); equal lengths give hssfsst_bilstm_stash_floats.
 *                        Host only; the plan may be NULL.
 * The plan keeps the list's device tables while the next call has the same offsets; a backward call must be given the offsets of
 * its forward call.
 * Alignment: as the dense pair -- every tensor at any float, offsets (host) at any int64; the stash must be 16-byte aligned, or
 * HSSFSST_EINVAL ("stash is not 16-byte aligned") before any device work, after the list's and the NULL checks. */
int hssfsst_bilstm_stash_floats_ragged(const hssfsst_bilstm* plan, const int64_t* offsets, int64_t count, int64_t* floats);
int hssfsst_bilstm_forward_ragged(hssfsst_bilstm* plan, const float* x, const int64_t* offsets, int64_t count, const float* h0,
                                  const float* c0, float* y, float* hn, float* cn, float* stash, void* stream);
int hssfsst_bilstm_backward_ragged(hssfsst_bilstm* plan, const float* stash, const float* c0, const float* dy, const float* dhn,
                                   const float* dcn, const int64_t* offsets, int64_t count, float* dgates, float* dh0, float* dc0,
                                   void* stream);

int hssfsst_device_count(void);
int hssfsst_version(void);
const char* hssfsst_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* HSSFSST_H */
