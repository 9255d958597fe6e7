/* avz.h — C ABI of the MI355X-native mask-driven MVDR engine (libavz.so).
 *
 * The reference (Senpai-sama06/real-time-audio-visual-zooming) is pure Python and
 * binds no FFI; its operator surface for this path is a set of module-level
 * functions. Each entry point below states the reference interface it replaces
 * (paths relative to the reference root). Host code reaches it through ctypes
 * (real-time-audio-visual-zooming_amd/avz/_lib.py); see INTEGRATION.md.
 *
 * Conventions
 *  - Plain pointers and sizes only. Array pointers are DEVICE pointers (HBM),
 *    caller-owned; strides are in elements. No allocation on the hot call.
 *  - Every function returns 0 on success or a negative AVZ_ERR_* code and never
 *    throws across the ABI (the reference reports errors by print-and-return,
 *    e.g. oracle_debug.py:31-33; singular solves fall back to w = [1, 0],
 *    oracle_debug.py:78-79 — the kernels reproduce that fallback per bin).
 *  - A plan's configuration and steering table are immutable after creation. Every
 *    avz_mvdr_batch call needs a per-call device workspace (chunk partials, mask words,
 *    apply coefficients, seam halves, peak words). A call that passes its own
 *    (avz_batch_args.workspace, sized by avz_mvdr_workspace_bytes) shares nothing
 *    mutable with other calls, so calls with distinct workspaces may run concurrently
 *    on different streams. A call that passes workspace = NULL uses the plan's own
 *    workspace: such calls (and avz_srp_scan, which always uses it) must be ordered
 *    on one stream or otherwise serialised by the caller. The diagnostic timing state
 *    (avz_plan_set_timing) is not thread-safe.
 *  - Device lengths len[b] are clamped to the call's host-validated max_len in every
 *    kernel, so an inconsistent len[] cannot move an access outside the caller's rows.
 */
#ifndef AVZ_H_
#define AVZ_H_

#ifdef __cplusplus
extern "C" {
#endif

#define AVZ_OK 0
#define AVZ_ERR_ARG (-1)         /* null/invalid argument                       */
#define AVZ_ERR_SHAPE (-2)       /* length/stride/batch outside the plan        */
#define AVZ_ERR_HIP (-3)         /* HIP runtime error (launch / allocation)     */
#define AVZ_ERR_UNSUPPORTED (-4) /* configuration not implemented              */
#define AVZ_ERR_ALIGN (-5)       /* pointer/stride below its element/vector alignment */

/* mask sources */
#define AVZ_MASK_IBM 0      /* oracle ideal binary mask from refs, oracle_debug.py:49-53  */
#define AVZ_MASK_IPD 1      /* heuristic phase mask, masked_mvdr.py:37-46                 */
#define AVZ_MASK_EXTERNAL 2 /* caller-provided target probability M, noise = 1 - M,
                               full_audio_generating_pipeline/inference.py:99-106          */
#define AVZ_MASK_ONES 3     /* every bin weight 1: full-signal covariance (MPDR; the SRP
                               scan's R, scripts/debug_srp.py:56-59)                       */

/* post-filters (A10) */
#define AVZ_PF_NONE 0       /* masked_mvdr.py: none                                      */
#define AVZ_PF_IBM_TARGET 1 /* x (1 - mask_noise), oracle_debug.py:84-90                 */
#define AVZ_PF_EXT_FLOOR 2  /* x max(M, floor), full_audio.../inference.py:116           */
#define AVZ_PF_EXT_MUL 3    /* x M, Final_pipeline/src/inference.py:219                  */
#define AVZ_PF_IRM 4        /* x sqrt(|S_t|^2 / (|S_t|^2 + |S_i|^2 + 1e-10)) from the two
                               references (AVZ_MASK_IBM only), oracle_reverb.py:143-156   */

/* weights of a bin whose loaded covariance is singular (A8) */
#define AVZ_FALLBACK_MIC0 0 /* w = [1, 0], oracle_debug.py:78-79, masked_mvdr.py:120-122  */
#define AVZ_FALLBACK_MEAN 1 /* w = ones/2, oracle_reverb.py:133-135                       */
#define AVZ_FALLBACK_BATCH 2 /* batch_mvdr (tf_lite_version/inference.py:143-157): one
                               np.linalg.solve over all bins of a call, so a singular bin sends
                               EVERY bin of that item to w~ = [1, 0]^T, which is then
                               normalised like the others: w = [1/(conj(d0) + 1e-10), 0]     */

/* beamformers (A8 / A14) */
#define AVZ_BF_MVDR 0       /* (R/(sum m + 1e-6) + sigma I)^-1 d, normalised; oracle_debug.py:66-79 */
#define AVZ_BF_HYBRID_NULL 1 /* principal eigenvector of the noise covariance as a hard null
                               next to the phase-normalised target steering vector; delay-and-sum
                               when cond([v_tgt, v_int]) > cond_max; mic 0 below bypass_hz;
                               Final_pipeline/src/inference.py:16-98                          */

/* output normalisation (A12) */
#define AVZ_NORM_NONE 0     /* un-normalised; peak[] reports max|out|                     */
#define AVZ_NORM_PEAK 1     /* out /= (max|out| + norm_eps), oracle_debug.py:94 (eps 0),
                               masked_mvdr.py:128 (eps 1e-6)                              */

typedef struct avz_config {
  int fs;            /* sample rate, masked_mvdr.py:9 (16000)                         */
  int n_fft;         /* 512 (rt_av_zoom core) or 1024 (Final_pipeline/config.py:15)   */
  int hop;           /* must be n_fft/2 (every reference call site uses 50% overlap)  */
  double sigma;      /* diagonal loading: 1 (oracle_debug.py:24), 1e-7, 1e-5          */
  double angle_deg;  /* target direction, 90 (masked_mvdr.py:12)                     */
  double mic_d;      /* mic spacing in m: 0.01 (masked_mvdr.py:10), 0.04, 0.08        */
  double c_sound;    /* 343 (masked_mvdr.py:11)                                      */
  double fmin_hz;    /* bins with f < fmin get w = 0 (oracle_debug.py:67: 100)       */
  int mask_mode;     /* AVZ_MASK_*                                                   */
  int postfilter;    /* AVZ_PF_*                                                     */
  double pf_floor;   /* floor for AVZ_PF_EXT_FLOOR (0.05)                           */
  double weight_eps; /* covariance weight sqrt(m + eps)^2: 0, or 1e-10 as in
                        tf_lite_version/inference.py:109                            */
  int normalize;     /* AVZ_NORM_*                                                   */
  double norm_eps;   /* 0 (oracle_debug), 1e-6 (masked_mvdr), 1e-9 (oracle_reverb)   */
  int max_batch;     /* utterances per call                                          */
  int max_samples;   /* longest utterance (samples)                                  */
  int beamformer;    /* AVZ_BF_*                                                     */
  double bypass_hz;  /* AVZ_BF_HYBRID_NULL: bins with f < bypass_hz pass mic 0 (200)  */
  double cond_max;   /* AVZ_BF_HYBRID_NULL: delay-and-sum above this 2-norm condition
                        number of [v_tgt, v_int] (10, inference.py:80)               */
  int singular_fallback; /* AVZ_FALLBACK_*                                            */
  double ibm_kappa;  /* AVZ_MASK_IBM, reference-exact decisions (oracle_debug.py:42-53):
                        every (bin, frame) decision of the fp32 reference transform must
                        clear an error bound of ibm_kappa * 2^-24 * ||windowed frame||, or
                        the frame's decision is recomputed from fp64 reference spectra
                        rounded to complex64 with numpy's |.|.
                        A frame whose reference energy is outside the range in which fp32
                        neither underflows nor overflows in that test (2^-56 .. 2^100 for
                        N = 1024 at kappa 16) is recomputed whole unless it is all zeros.
                        0 = AVZ_IBM_KAPPA; < 0 = no certificate (fp32 decisions only). */
} avz_config;
/* 16: the bound 3.9 kappa eps ||z|| max|Z| covers the largest fp32-transform error seen in
 * 1.5 M decisions of the configs[1] generator (49 eps ||z|| max|Z|, tools/dbg/kappa_sweep.py
 * and DESIGN.md section 2) by 1.27x; each doubling of kappa adds ~1 % of the frames. */
#define AVZ_IBM_KAPPA 16.0

typedef struct avz_plan avz_plan;

/* Fused batch call. Replaces, per utterance b, the body of
 * rt_av_zoom/core/oracle_debug.py:42-94 (IBM), rt_av_zoom/core/masked_mvdr.py:76-128
 * (IPD) and full_audio_generating_pipeline/inference.py:88-118 (external mask):
 * STFT -> mask -> masked covariance -> MVDR solve -> apply + post-filter -> iSTFT
 * (-> peak normalise). out[b] has (ceil(len[b]/hop)) * hop samples
 * (scipy.signal.istft length); nothing of the row is written past them.
 * A row shorter than a frame (len[b] < n_fft, 0 included; scipy needs nperseg <= len) is
 * skipped, on every kernel path of the chain: its row of out is not written at all and
 * peak[b] is NaN (as the rows avz_srp_scan and avz_delay_mask do not process). Its
 * neighbours in the batch are computed as if it were not there. */
typedef struct avz_batch_args {
  int batch;
  const int* len;          /* [batch] samples per utterance (device), n_fft <= len <= max_samples;
                              a shorter row is skipped (above)                                  */
  int max_len;             /* host-side upper bound of len[] (validated against strides)         */
  const float* mix;        /* [batch][2][ch_stride]: mic channels planar (y_mix [2,S])          */
  long long mix_stride;    /* elements between utterances                                       */
  long long ch_stride;     /* elements between the two mic channels                             */
  const float* ref_tgt;    /* [batch][ref_stride] target reference (IBM) or NULL                */
  const float* ref_int;    /* [batch][ref_stride] interference reference (IBM) or NULL          */
  long long ref_stride;
  const float* ext_mask;   /* target probability M[b][k][t] (EXTERNAL) or NULL. Only k < F and
                              t < frames(len[b]) of row b are used: entries at later frames, row
                              padding between the strides and bins >= F never influence an
                              output. Strides in floats, any layout; mask_stride_b = 0 (one
                              mask for the whole batch) is allowed                             */
  long long mask_stride_b, mask_stride_f, mask_stride_t;
  float* out;              /* [batch][out_stride], out_stride % 4 == 0, 16-byte aligned          */
  long long out_stride;
  float* peak;             /* [batch] max|out| before normalisation (NaN for a skipped row), or
                              NULL                                                               */
  double* cov_out;         /* debug: [batch][F][5] sum m|y0|^2, sum m|y1|^2, Re/Im sum m y0 y1*,
                              sum m   (or NULL)                                                  */
  float* w_out;            /* debug: [batch][F][4] Re w0, Im w0, Re w1, Im w1 (or NULL)         */
  int mask_bins;           /* EXTERNAL: bins of ext_mask (>= F) and frames (>= frames of max_len) */
  int mask_frames;
  void* workspace;         /* per-call device workspace (256-byte aligned), or NULL: the plan's */
  long long workspace_bytes; /* >= avz_mvdr_workspace_bytes(plan, batch, max_len)              */
} avz_batch_args;

int avz_plan_create(avz_plan** plan, const avz_config* cfg);
int avz_plan_destroy(avz_plan* plan);
int avz_plan_get_config(const avz_plan* plan, avz_config* cfg);
/* Frames of an utterance of len samples: ceil(len/hop) + 1 (scipy padded/boundary). */
int avz_num_frames(const avz_plan* plan, int len);
int avz_mvdr_batch(const avz_plan* plan, const avz_batch_args* args, void* hip_stream);
/* Device bytes of a per-call workspace for `batch` utterances of at most max_len samples
 * (negative AVZ_ERR_* on bad arguments). */
long long avz_mvdr_workspace_bytes(const avz_plan* plan, int batch, int max_len);

/* ------------------------------------------------------------------ stage exports
 * The chain of avz_mvdr_batch, one stage at a time (stage-wise parity with
 * rt_av_zoom/core/oracle_debug.py:42-64 / :66-79 / :80-94):
 *  avz_mvdr_covariance  STFT -> mask -> masked covariance sums, args->cov_out[b][F][5]
 *                       (sum m|y0|^2, sum m|y1|^2, Re/Im sum m y0 y1*, sum m; fp64);
 *                       args->out unused. Inputs as avz_mvdr_batch for the plan's mask mode.
 *  avz_solve_covariance cov[b][F][5] -> weights w[b][F][4] (Re w0, Im w0, Re w1, Im w1;
 *                       16-byte aligned) with the plan's beamformer, sigma, fmin and
 *                       fallback; steer = optional [F][2] complex128 steering vectors
 *                       (NULL: the plan's); fallback = optional [batch] flags (NULL: the
 *                       plan's own buffer, calls then serialised).
 *  avz_apply_istft      STFT of args->mix -> S = w^H y (x args->ext_mask as a gain when
 *                       non-NULL, mask_bins / mask_frames as for EXTERNAL) -> iSTFT/OLA ->
 *                       args->out (peak-normalised per the plan), args->peak. The gain is
 *                       applied as given: no clamp to [0, 1], no floor (the plan's
 *                       post-filter and pf_floor play no part here).
 * Device arrays; the same workspace rules as avz_mvdr_batch. */
int avz_mvdr_covariance(const avz_plan* plan, const avz_batch_args* args, void* hip_stream);
int avz_solve_covariance(const avz_plan* plan, int batch, const double* cov, float* w,
                         const double* steer, int* fallback, void* hip_stream);
int avz_apply_istft(const avz_plan* plan, const avz_batch_args* args, const float* w,
                    void* hip_stream);

/* ------------------------------------------------------------------ spectral domain
 * For callers that already hold an STFT. avz_beamform_spectral replaces, per item b,
 *  - beamformer AVZ_BF_MVDR: batch_mvdr(Y, mask, f_bins, d_vectors, sigma)
 *    (rt_av_zoom/core/tf_lite_version/inference.py:85-179; plan: weight_eps 1e-10,
 *    fmin_hz 0, singular_fallback AVZ_FALLBACK_BATCH, sigma = SIGMA);
 *  - beamformer AVZ_BF_HYBRID_NULL: hybrid_hard_null_bf(Y, mask, f_bins)
 *    (Final_pipeline/src/inference.py:28-98; plan: weight_eps 0, bypass_hz 200,
 *    cond_max 10),
 * with the plan's post-filter fused (AVZ_PF_EXT_FLOOR: x max(M, pf_floor), the TFLite
 * driver's S_out * np.maximum(mask, 0.05), inference.py:350; AVZ_PF_EXT_MUL: x M,
 * Final_pipeline/src/inference.py:219; AVZ_PF_NONE: the bare operator). The plan's mask
 * mode must be AVZ_MASK_EXTERNAL (mask = target probability, noise weight 1 - M).
 * Y: complex64 [b][m][k][t] (interleaved re/im; m = mic 0, 1; t contiguous), strides in
 * complex elements; mask [b][k][t] float; S: complex64 [b][k][t]. steer: optional [F][2]
 * complex128 (batch_mvdr's d_vectors; NULL: the plan's table). Y and S 8-byte, mask 4-byte
 * aligned (else AVZ_ERR_ALIGN). cov_out / w_out: optional
 * per-bin covariance sums / weights; fallback: optional [batch] int flags (1 where an
 * item took the item-level fallback; NULL: the plan's own buffer). */
typedef struct avz_spectral_args {
  int batch;               /* items (one reference call each)                              */
  int frames;              /* T frames per item                                            */
  const float* Y;
  long long y_stride_b, y_stride_m, y_stride_f;
  const float* mask;
  long long mask_stride_b, mask_stride_f;
  const double* steer;
  float* S;
  long long s_stride_b, s_stride_f;
  double* cov_out;
  float* w_out;
  int* fallback;
} avz_spectral_args;
int avz_beamform_spectral(const avz_plan* plan, const avz_spectral_args* args, void* hip_stream);

/* WPE dereverberation of a two-mic spectrum: the first stage of the reference's reverberant
 * chain, apply_wpe's wpe(Y, taps=10, delay=3, iterations=3, psd_context=0,
 * statistics_mode='full') call (rt_av_zoom/core/dereverb.py:76-78), as offline batch WPE
 * (Nakatani et al. 2010; the algorithm itself is the contract). Per
 * (item, bin), with Y [2, T] and n = 2 taps: Yt[2 tau + m, t] = Y[m, t - delay - tau] (0
 * before the first frame); X = Y; `iterations` times p[t] = mean_m |X[m,t]|^2,
 * lambda[t] = 1 / max(p[t], 1e-10 max_t p), R = sum_t lambda Yt Yt^H, P = sum_t lambda Yt Y^H,
 * G = R^-1 P (fp64 sums, fp64 Cholesky), X = Y - G^H Yt; Z = X.
 * status[b][k]: 0 = dereverberated; the other bins pass Y through unchanged: 2 where
 * frames_b[b] - delay < 2 taps (fewer regressor frames than unknowns; decided first and by
 * the count alone) or a Cholesky pivot is <= (2 taps + 1) 2^-52 R_jj or not finite, 1 where
 * max_t p == 0.
 * Y, Z: the layout of avz_beamform_spectral's Y with `bins` bins, 8-byte aligned (else
 * AVZ_ERR_ALIGN); Z may be Y itself (same strides), no other overlap. frames_b[b] is clamped
 * to [0, frames]; frames t >= frames_b[b] of Z are copies of Y and enter no sum.
 * taps 1..16, delay >= 1, iterations 1..10 (else AVZ_ERR_ARG); frames 1..2048 (else
 * AVZ_ERR_SHAPE: a problem's 24 bytes per frame and up to 16 KiB of R, P and partial sums
 * stay in 64 KiB of LDS). No plan, no workspace, no allocation. */
typedef struct avz_wpe_args {
  int batch, bins, frames;      /* frames = T of the arrays                          */
  const int* frames_b;          /* device [batch] valid frames per item, or NULL = T */
  int taps, delay, iterations;
  const float* Y;               /* complex64 [b][m][k][t], t contiguous; strides in complex elements */
  long long y_stride_b, y_stride_m, y_stride_f;
  float* Z;                     /* same layout; may alias Y exactly                  */
  long long z_stride_b, z_stride_m, z_stride_f;
  int* status;                  /* optional device [batch][bins]: 0, 1, 2 as above   */
} avz_wpe_args;
int avz_wpe_spectral(const avz_wpe_args* args, void* hip_stream);

/* scipy.signal.istft(S, fs, nperseg=n_fft, noverlap=n_fft/2) of complex64 S[b][k][t]
 * (t contiguous; strides in complex elements) for `frames` frames per item: out[b] gets
 * (frames - 1) * hop samples (<= max_samples), peak-normalised per the plan; peak[b] =
 * max|out| before normalisation (or NULL). frames >= 3: (frames - 1) * hop < n_fft, which
 * scipy accepts (two frames), returns AVZ_ERR_SHAPE, as a time-domain row shorter than a frame
 * is not processed. The imaginary parts of the DC and Nyquist bins are ignored (as irfft
 * ignores them). The same workspace rules as avz_mvdr_batch
 * (workspace bytes: avz_mvdr_workspace_bytes(plan, batch, (frames - 1) * hop)). Replaces
 * the istft calls at oracle_debug.py:93, tf_lite_version/inference.py:352,
 * Final_pipeline/src/inference.py:222. */
int avz_istft(const avz_plan* plan, int batch, int frames, const float* S, long long s_stride_b,
              long long s_stride_f, float* out, long long out_stride, float* peak,
              void* workspace, long long workspace_bytes, void* hip_stream);

/* Diagnostics: time the kernels of every avz_mvdr_batch call on this plan with HIP
 * events carried by the kernels' own dispatches (hipExtLaunchKernel start / stop events,
 * no marker packets between launches): enable 1 = all four (analysis, solve, synthesis,
 * finalize), 2 = the analysis kernel only, 0 = off; enabling also resets the sums.
 * avz_plan_get_timing waits for the outstanding calls and returns the average
 * milliseconds per kernel over the calls recorded since enabling (NaN for kernels not
 * timed; a kernel folded into another counts 0: with N = 512 or 1024, peak normalisation
 * and the IBM or no post-filter the per-utterance synthesis kernel folds finalize in, and
 * for plain MVDR plans without the item-level fallback or cov / w outputs the solve too --
 * except that a batch below the CU count that the N = 1024 kernel splits into step pieces
 * launches a piece finalize, which the finalize slot then times; the pieces of a partial
 * last round after whole rounds finalize inside the synthesis kernel). Not thread-safe. */
int avz_plan_set_timing(avz_plan* plan, int enable);
/* Time one avz_mvdr_batch call in `period` (>= 1; default 1): the calls in between carry no
 * events, so a sampled timing run costs the other calls nothing. */
int avz_plan_set_timing_period(avz_plan* plan, int period);
int avz_plan_get_timing(avz_plan* plan, double* ms_avg /*[4]*/, int* calls);
/* Diagnostics of the reference-exact IBM path (avz_config.ibm_kappa): every later call on
 * this plan adds to counts[0] the frames decided on the exact path and to counts[1] the
 * (bin, frame) decisions taken there (device array of two unsigned long long, zeroed by the
 * caller; NULL = off). Not thread-safe with calls on the plan. */
int avz_plan_set_ibm_stats(avz_plan* plan, unsigned long long* counts);
/* Diagnostics: kernel-path A/B of this plan's later calls (tests and tools only; the
 * results are the same up to the fp32 association of the partial sums):
 *  synth_variant 2 (default) = the per-utterance synthesis kernel solving its own bins,
 *  1 = the same after the solve kernel, 0 = the two-block chunk grid + finalize kernel;
 *  ipf_mode 0 (default) = the in-kernel piece finalize as shipped, 1 = every piece but its
 *  utterance's last arriver hands its interior back at once, 2 = pieces ignore the published
 *  1/peak until their next utterance's end (the protocol's rare paths, forced).
 * Not thread-safe with calls on the plan. */
int avz_plan_set_diagnostics(avz_plan* plan, int synth_variant, int ipf_mode);
/* The reference's fp32 analysis window, np.float32(scipy.signal.get_window('hann', n)), as the
 * exact IBM path uses it (n = 512 or 1024; host memory; for tests). */
int avz_ibm_window(int n, float* out);

/* Stage API: STFT of [batch][channels][x_stride] real signals into complex64
 * Y[b][c][k][t] (interleaved re/im floats) with element strides; replaces the
 * reference's scipy.signal.stft(x, fs, nperseg=n_fft, noverlap=n_fft/2) calls
 * (oracle_debug.py:42-44, masked_mvdr.py:76, Final_pipeline/src/inference.py:198). */
int avz_stft(const avz_plan* plan, int batch, int channels, const int* len, int max_len,
             const float* x, long long x_stride, long long ch_stride, float* Y,
             long long y_stride_b, long long y_stride_c, long long y_stride_f,
             void* hip_stream);

/* Final_pipeline driver chunking (Final_pipeline/src/inference.py:171-188): copy
 * item i = samples [item_start[i], item_start[i] + chunk) of utterance item_utt[i]
 * (zero beyond len[utt], the driver's np.pad of the tail chunk) for each of
 * `channels` planar channels into items[i][c][0..chunk). Device arrays. */
int avz_chunk_split(int n_items, int channels, int chunk, const int* item_utt,
                    const int* item_start, const int* len, const float* x, long long x_stride,
                    long long x_ch_stride, float* items, long long item_stride,
                    long long item_ch_stride, void* hip_stream);

/* Final_pipeline driver overlap-add (inference.py:224-236): for utterance b with
 * chunks c = 0 .. ceil(len[b]/hop) - 1 stored as items item_base[b] + c, each adding
 * item_out[...][0 .. min(item_out_len, len[b] - c hop)) at sample c hop:
 * y[b][n] = (sum of the covering chunk outputs) / max(count, 1); peak[b] = max|y[b]|;
 * with normalize != 0, y[b] /= peak[b] + norm_eps (1e-9 in the reference). */
int avz_chunk_merge(int batch, int max_len, int hop, int item_out_len, const int* len,
                    const int* item_base, const float* item_out, long long item_out_stride,
                    float* y, long long y_stride, float* peak, int normalize, double norm_eps,
                    void* hip_stream);

/* Mask-model input features straight from the time-domain mic pair (device arrays):
 *  AVZ_FEAT_LOGMAG_IPD: feat[b*s_b + c*s_c + k*s_f + t*s_t], c = 0: log(|Y0| + 1e-7),
 *    c = 1: angle(Y0) - angle(Y1) — the U-Net input of
 *    full_audio_generating_pipeline/inference.py:90-94 (NCHW with s_t = 1);
 *  AVZ_FEAT_TFLITE: c = 0..3: log_mag, sin(ipd), cos(ipd), linspace(0, 1, F)[k] — the
 *    TFLite input of Final_pipeline/src/inference.py:198-203, 117-128 (NHWC: s_c = 1,
 *    s_t = 4, s_f = 4 T).
 * Y = scipy.signal.stft(x, nperseg=n_fft, noverlap=n_fft/2) of the plan's n_fft. */
#define AVZ_FEAT_LOGMAG_IPD 1
#define AVZ_FEAT_TFLITE 2
int avz_mask_features(const avz_plan* plan, int layout, int batch, const int* len, int max_len,
                      const float* x, long long x_stride, long long ch_stride, float* feat,
                      long long s_b, long long s_c, long long s_f, long long s_t,
                      void* hip_stream);

/* One training batch of the mask estimator, the sample of
 * full_audio_generating_pipeline/model_training.py:80-92 (SpatialDataset.__getitem__) for
 * `batch` items in one kernel (device arrays; no plan workspace, no allocation):
 *  feat:  exactly what avz_mask_features writes for `layout` from `mix` (the same bits);
 *  label[b*l_b + k*l_f + t*l_t] = 1.0f where |S_t[k,t]| > |S_i[k,t]|, else 0.0f, S_t / S_i
 *    the STFTs (as above) of tgt[b] / itf[b] (at ref_stride floats per item).
 * The label is decided on the kernel's own fp32 transforms, as the chain's ibm_kappa < 0 tier
 * decides its mask: it is not the reference-exact decision of the IBM plans, so a (bin,
 * frame) whose two magnitudes agree to within the fp32 transform's error may differ from
 * numpy's np.where. Where both reference frames are all zeros the label is 0, exactly.
 * Scaling tgt and itf by one power of two leaves every label unchanged.
 * Frames t >= ceil(len[b]/hop) + 1 and items with len[b] < n_fft are not written (as
 * avz_stft). The plan's mask mode is irrelevant. AVZ_ERR_ARG: a NULL pointer or an unknown
 * layout; AVZ_ERR_SHAPE: batch > the plan's max_batch, max_len outside [n_fft,
 * max_samples], ch_stride < max_len, or (batch > 1) mix_stride < ch_stride + max_len or
 * ref_stride < max_len. */
int avz_mask_training_batch(const avz_plan* plan, int layout, int batch, const int* len,
                            int max_len, const float* mix, long long mix_stride,
                            long long ch_stride, const float* tgt, const float* itf,
                            long long ref_stride, float* feat, long long s_b, long long s_c,
                            long long s_f, long long s_t, float* label, long long l_b,
                            long long l_f, long long l_t, void* hip_stream);

/* Steered response power scan, scripts/debug_srp.py:46-62 for a batch: for the
 * angles np.linspace(angle_lo, angle_hi, n_angles) (degrees, the plan's mic_d and
 * c_sound, debug_srp.py:17-23 geometry), P = sum over bins f_lo <= f <= f_hi and all
 * frames of |d^H y|^2; power_db[b][i] = 10 log10(P_i) - max_j 10 log10(P_j) (device).
 * Both band edges are inclusive (f_k = k fs / n_fft compared in fp64). n_angles = 1 scans
 * angle_lo alone and gives exactly 0.0; n_angles is not limited by the block size. The plan's
 * mask mode is irrelevant (the scan sums the unmasked covariance); of the plan's workspace
 * the call overwrites only what every avz_mvdr_batch call rebuilds (the covariance
 * partials), so it may sit between two such calls on the same plan and stream.
 * A row with len[b] < n_fft is not scanned: its n_angles values come back NaN (unlike
 * avz_stft and avz_mask_features, which leave such a row unwritten). Degenerate maps follow
 * the reference's arithmetic: when every scanned power is 0 (an all-zero mixture, or a band
 * [f_lo, f_hi] that holds no bin) each value is -inf - (-inf) = NaN, as
 * debug_srp.py:61-62 gives. */
int avz_srp_scan(const avz_plan* plan, int batch, const int* len, int max_len,
                 const float* mix, long long mix_stride, long long ch_stride, int n_angles,
                 double angle_lo, double angle_hi, double f_lo, double f_hi, double* power_db,
                 void* hip_stream);

/* Projection metrics of a batch (device arrays, float32 signals of len[b] samples, the
 * caller having aligned them to the minimum length as metrics.py:91-98 does):
 * metrics[b] = { OSINR, OSIR } of Final_pipeline/src/metrics.py:102-123
 *              (calculate_osnr_osir; output not normalised) and
 *              { SDR, SIR } of scripts/run_metrics.py:6-36 (calculate_metrics_manual),
 * in dB, from fp64 inner products; sums[b][6] is caller-provided workspace
 * (<o,o>, <t,t>, <i,i>, <o,t>, <o,i>, <t,i> on return). */
int avz_projection_metrics(int batch, int max_len, const int* len, const float* est,
                           long long est_stride, const float* tgt, long long tgt_stride,
                           const float* itf, long long itf_stride, double* sums,
                           double* metrics, void* hip_stream);
/* The same metrics of est[b] / (est_peak[b] + est_eps): an un-normalised output (a plan
 * with AVZ_NORM_NONE, whose peak[] it returns) scored as the peak-normalised one without
 * the normalisation pass over the samples (the scale enters the fp64 sums). */
int avz_projection_metrics_scaled(int batch, int max_len, const int* len, const float* est,
                                  long long est_stride, const float* est_peak, double est_eps,
                                  const float* tgt, long long tgt_stride, const float* itf,
                                  long long itf_stride, double* sums, double* metrics,
                                  void* hip_stream);

/* Short-time objective intelligibility of a batch: the stoi(s_tgt, s_est, config.FS,
 * extended=False) score of Final_pipeline/src/metrics.py:157-160, as the published algorithm
 * (Taal, Hendriks, Heusdens, Jensen 2011; avz/stoi.py stoi_numpy is the
 * fp64 restatement), not pystoi's bits. Per pair (clean x, processed y, len[b] samples each):
 * 16 kHz -> 10 kHz by the 581-tap 5/8 polyphase Kaiser filter (fp64 sums, fp32 storage;
 * 10 kHz passes through); frames of 256 at hop 128 starting at 0, 128, ... < n10 - 256 under
 * hanning(258)[1:-1]; the frames whose clean energy is within 40 dB of the loudest are kept
 * (K of them) and overlap-added; the J = K - 1 frames of the joined signals are windowed
 * again and transformed (512 points, fp32); 15 third-octave bands from 150 Hz (fp64 sums);
 * d = the mean over the J - 29 segments of 30 frames and the bands of the correlation of the
 * mean-removed x with the scaled, clipped (-15 dB) and mean-removed y (fp64).
 * info[b] = { status, frames, K, segments }: status 0; 1 = fewer than 30 joined frames (or
 * none at all), stoi[b] = 1e-5; 2 = a clean frame energy is not finite, stoi[b] = NaN. A NaN
 * in y alone gives status 0 and stoi[b] = NaN. An utterance's values never reach another's.
 * Repeated calls give identical bits. stoi does not depend on the scale of y.
 * fs: 16000 or 10000 (else AVZ_ERR_UNSUPPORTED). len[b] is clamped to [0, max_len].
 * batch <= 32767, max_len < 2^30, strides (elements) >= max_len, res_stride >= the 10-kHz
 * length of max_len (ceil(5 max_len / 8) at 16 kHz), tob_stride >= its frame count - 1,
 * workspace_bytes >= avz_stoi_workspace_bytes() (else AVZ_ERR_SHAPE); workspace 256-byte
 * aligned. The stage exports hold the 10-kHz signals (x then y) and the band values of the
 * first K - 1 frames. No plan, no allocation on the call. Device arrays. */
typedef struct avz_stoi_args {
  int batch, max_len;
  const int* len;            /* device [batch], or NULL = max_len                      */
  double fs;                 /* 16000 or 10000, else AVZ_ERR_UNSUPPORTED               */
  const float* clean; long long clean_stride;
  const float* est;   long long est_stride;
  double* stoi;              /* device [batch]                                          */
  int* info;                 /* optional device [batch][4]: status, frames, kept K, segments */
  float* resampled;          /* optional debug: [batch][2][res_stride] 10-kHz signals   */
  long long res_stride;
  double* tob;               /* optional debug: [batch][2][15][tob_stride] band values  */
  long long tob_stride;
  void* workspace; long long workspace_bytes;
} avz_stoi_args;
long long avz_stoi_workspace_bytes(int batch, int max_len, double fs);
int avz_stoi_batch(const avz_stoi_args* args, void* hip_stream);

/* Synthetic scene mixing on the device — the anechoic far-field generator of
 * full_audio_generating_pipeline/world_building.py:47-59 (per-mic fractional delay by an
 * rfft phase shift over the whole signal, d = mic_d, c = c_sound) with the SIR gain
 * (Final_pipeline/src/simulation.py:167-179, on mic 1), AWGN at snr_db per channel
 * (world.py:93-98, noise = sqrt(mean(clean^2)/10^(snr/10)) * z) and the shared peak
 * normalisation of simulation.py:197-202 (peak = max|mix| + 1e-9).
 * src[b][s][0..n) are the mono sources (s = 0 the target, 1..n_src-1 interferers) at
 * angles_deg[b][s]; noise[b][c][0..n) unit-normal draws for mic c. Writes
 * mix[b][c] (at mix_stride / ch_stride), tgt[b] = mic-1 target image / peak,
 * itf[b] = mic-1 interference image / peak. `workspace` holds
 * avz_scene_workspace_bytes(batch, n_src, n) bytes. All arrays device-resident.
 * n even. When n factors into 2, 3 and 5 the delays run as fp64 mixed-radix FFTs
 * (O(n log n)); otherwise as the exact O(n^2) circular convolution (fp32 sums). Both paths
 * take every even n >= 2 and every delay, |delay| > n samples included; a delay of a whole
 * number of samples (within 1e-12 in |sin(pi delay)|) is the circular shift by that number,
 * 0 included (on the O(n^2) path a rotated copy of the source, no sum). */
long long avz_scene_workspace_bytes(int batch, int n_src, int n);
int avz_scene_mix(int batch, int n_src, int n, const float* src, const double* angles_deg,
                  const float* noise, double mic_d, double c_sound, double fs, double sir_db,
                  double snr_db, float* mix, long long mix_stride, long long ch_stride,
                  float* tgt, float* itf, long long ref_stride, void* workspace,
                  long long workspace_bytes, void* hip_stream);

/* The whole scene on the device (the sharded batch driver's input path): utterance
 * start_idx + b draws from counter-based Philox4x32-10 streams keyed by (start_idx + b,
 * 0x5CE7E5ED ^ seed) — Box-Muller normals for the speech-like sources (AR(2) poles 0.9 /
 * 0.5, |sin(2 pi 4 t + phi)| envelope, 25 % of 250-ms blocks silenced: synth.speech_like)
 * and the AWGN, uniforms for the envelope phases, the kept blocks and the azimuths of
 * interferers 2.. (target 90 deg, interferer 1 at 40 deg) — then avz_scene_mix's model.
 * avz/synth.py make_scene_philox is the host restatement. `workspace` holds
 * avz_scene_generate_workspace_bytes(batch, n_interferers, n) bytes. */
long long avz_scene_generate_workspace_bytes(int batch, int n_interferers, int n);
int avz_scene_generate(int batch, long long start_idx, int n_interferers, int n, unsigned seed,
                       double mic_d, double c_sound, double fs, double sir_db, double snr_db,
                       float* mix, long long mix_stride, long long ch_stride, float* tgt,
                       float* itf, long long ref_stride, void* workspace,
                       long long workspace_bytes, void* hip_stream);

/* Reverberant shoebox scenes: the `reverb` mode of the reference's scene builders
 * (Final_pipeline/src/simulation.py:105-165, rt_av_zoom/core/world.py:125-190), which build a
 * pyroomacoustics ShoeBox and convolve every source with its room impulse response (RIR).
 * The contract here is the classic image-source model (Allen & Berkley 1979), not
 * pyroomacoustics' bits (avz/synth.py room_rir is the restatement):
 * one energy absorption for all six walls (beta = sqrt(1 - absorption)); images q with
 * |qx| + |qy| + |qz| <= max_order; per image the amplitude beta^order / (4 pi d), the delay
 * d fs / c and an 81-tap Hann-windowed sinc centred on the continuous delay. No air
 * absorption, scattering, ray tracing, RIR high-pass filter or per-wall materials. */
typedef struct avz_room {
  double dim[3];      /* shoebox edges, m (world.py:22) */
  double absorption;  /* energy absorption of all six walls, 0 < a <= 1 */
  int max_order;      /* 0 .. 20 */
  double mic[2][3];   /* inside the room */
  double c_sound, fs;
} avz_room;

/* Samples per RIR, floor(fs / c * Dmax) + 42 with Dmax the largest image distance bound, or
 * a negative AVZ_ERR_* code (AVZ_ERR_ARG: invalid room; AVZ_ERR_SHAPE: more than 8192). */
int avz_room_rir_len(const avz_room* room);

/* Stage export: rir[b][s][mic][rir_len] as fp64 from src_pos[b][s][3] (device arrays).
 * Results are bit-identical from call to call. */
int avz_room_rir(const avz_room* room, int batch, int n_src, const double* src_pos,
                 double* rir, void* hip_stream);

/* avz_scene_mix in the room: source s of utterance b sits at src_pos[b][s][3] (device,
 * fp64) and reaches mic c as fftconvolve(src, rir)[:n]; then avz_scene_mix's SIR gain, AWGN
 * and shared peak. tgt / itf are the reverberant mic-1 images. The geometry, fs and c come
 * from `room`. n >= 2, odd included. `workspace` holds avz_scene_reverb_workspace_bytes()
 * bytes: 32 (ceil(n_src / 2) + n_src) Lc per utterance, Lc the smallest length 2^a 3^b 5^c
 * >= n + rir_len - 1 (13.3 MB for 4 s, 4 sources, max_order 15 in the reference room), and
 * 4 batch n_src bytes of flags rounded up to 256. A source that is all zeros stays exactly out
 * of the scene here and in avz_scene_mix (all-zero interferers: itf = 0 and no SIR gain; an
 * all-zero target: every output 0), as in synth._mix_images. */
long long avz_scene_reverb_workspace_bytes(const avz_room* room, int batch, int n_src, int n);
int avz_scene_reverb_mix(const avz_room* room, int batch, int n_src, int n, const float* src,
                         const double* src_pos, const float* noise, double sir_db,
                         double snr_db, float* mix, long long mix_stride, long long ch_stride,
                         float* tgt, float* itf, long long ref_stride, void* workspace,
                         long long workspace_bytes, void* hip_stream);

/* avz_scene_generate in the room: its sources and noise (the same Philox draws), source 0
 * at target_pos, source 1 at interferer_pos (host arrays, inside the room), sources s >= 2
 * at (1 + u0 (dim_x - 2), 1 + u1 (dim_y - 2), target_pos[2]) with u0, u1 the utterance's
 * uniform draws 0x2000 + 2 (s - 2) + {0, 1} (simulation.py:133-136); more than one
 * interferer needs dim_x, dim_y > 2 m. synth.make_reverb_scene_philox is the restatement. */
long long avz_scene_reverb_generate_workspace_bytes(const avz_room* room, int batch,
                                                    int n_interferers, int n);
int avz_scene_reverb_generate(const avz_room* room, int batch, long long start_idx,
                              int n_interferers, int n, unsigned seed, const double* target_pos,
                              const double* interferer_pos, double sir_db, double snr_db,
                              float* mix, long long mix_stride, long long ch_stride, float* tgt,
                              float* itf, long long ref_stride, void* workspace,
                              long long workspace_bytes, void* hip_stream);

/* ------------------------------------------------------------------ streaming causal MVDR
 * The chain of avz_mvdr_batch run hop by hop with state carried between calls: the causal
 * ("real-time") form of oracle_debug.enhance / process_chunk, which the reference leaves as
 * its open latency item. The algorithm is the contract (avz/stream.py
 * stream_numpy is the fp64 restatement). With H = n_fft / 2, x_t the t-th hop pushed since
 * the last reset (both mics) and x_-1 = 0:
 *  - frame t = [x_t-1 | x_t] under the plan's fp32 periodic Hann, scaled by 1 / sum(w): frame
 *    t of scipy.signal.stft(x, nperseg=n_fft, noverlap=n_fft/2);
 *  - noise weight n_t[k] of the plan's mask mode: AVZ_MASK_EXTERNAL 1 - M[k][t] (covariance
 *    weight n_t + weight_eps, as the chain); AVZ_MASK_IBM 1 where |S_i| > |S_t| on the
 *    kernel's own fp32 reference transforms (the ibm_kappa < 0 tier, as
 *    avz_mask_training_batch; two all-zero reference frames give exactly 0); AVZ_MASK_ONES 1;
 *  - sums, fp64, per bin: c_t = forget c_t-1 + n_t (|y0|^2, |y1|^2, Re y0 y1*, Im y0 y1*, 1)
 *    where the stream's adapt flag is non-zero, else c_t = c_t-1 (covariance gating: the
 *    weights freeze);
 *  - weights w_t = the plan's MVDR solve of c_t (sigma, fmin_hz, singular_fallback MIC0 or
 *    MEAN) with the STREAM's steering vector; S_t = w_t^H Y_t times the plan's post-filter
 *    gain of frame t (NONE, IBM_TARGET 1 - n_t, EXT_FLOOR max(M, pf_floor), EXT_MUL M);
 *  - g_t = irfft(S_t) sum(w) w; output hop t = (g_t-1[H:] + g_t[:H]) / (w^2[m] + w^2[m + H])
 *    for t >= 1 and zeros for t = 0: scipy.signal.istft of the causal S delayed by one hop,
 *    the algorithmic latency. One extra hop of zeros drains the last H samples.
 * forget in (0, 1]; 1 gives running sums, which after the drain hop equal the offline sums.
 * AVZ_ERR_UNSUPPORTED (before any device work): AVZ_BF_HYBRID_NULL, AVZ_MASK_IPD, AVZ_PF_IRM,
 * AVZ_FALLBACK_BATCH, AVZ_NORM_PEAK (a peak is not causal).
 *
 * The state is one caller-owned device buffer of avz_stream_state_bytes(plan, streams) bytes,
 * 256-byte aligned, for streams <= the plan's max_batch; its layout is private (per stream:
 * a 64-bit frame count, the previous hop of the mics and references, the synthesis tail, the
 * sums [F][5] and the steering table [F][4] in fp64; about 47 KB at n_fft = 1024). No call
 * allocates.
 *  avz_stream_reset  zeroes the selected streams (select[s] != 0; NULL = all) and copies the
 *                    plan's steering table into them. A new buffer must be reset first.
 *  avz_stream_steer  rewrites the table of every stream whose angle_deg[s] is not NaN, on
 *                    the device: tau1 = (d/2) cos(theta) / c, tau2 = (d/2) cos(theta - pi) / c,
 *                    d_m = exp(-2 pi i f_k tau_m) (masked_mvdr.py:22-35), in fp64. The new
 *                    direction applies from the next pushed frame.
 *  avz_stream_push   `hops` >= 1 new hops per stream; out gets the same number of samples.
 * Checks, all on the host before any HIP call: a NULL plan, args, mix, out, state (or the
 * mask mode's ref_tgt / ref_int / ext_mask, or angle_deg), hops < 1 or forget outside (0, 1]:
 * AVZ_ERR_ARG; streams outside 1 .. max_batch, ch_stride or out_stride < hops * hop,
 * (streams > 1) mix_stride < ch_stride + hops * hop or ref_stride < hops * hop, or
 * state_bytes too small: AVZ_ERR_SHAPE; state not 256-byte aligned, out not 16-byte aligned
 * or out_stride % 4 != 0: AVZ_ERR_ALIGN.
 * Guarantees: a stream's outputs and final state are bit-identical however its hops are
 * grouped into calls (1 x T, T x 1 or ragged), whatever its index in the buffer and whatever
 * the other streams hold; a NaN in one stream never reaches another. Calls on one state
 * buffer must be stream-ordered; calls on distinct state buffers may run concurrently. */
long long avz_stream_state_bytes(const avz_plan* plan, int streams);
int avz_stream_reset(const avz_plan* plan, void* state, long long state_bytes, int streams,
                     const int* select /* device [streams] or NULL = all */, void* hip_stream);
int avz_stream_steer(const avz_plan* plan, void* state, long long state_bytes, int streams,
                     const double* angle_deg /* device [streams]; NaN = keep */,
                     void* hip_stream);
typedef struct avz_stream_args {
  int streams, hops;                 /* hops >= 1 new hops per stream in this call            */
  double forget;
  const int* active;                 /* device [streams] or NULL: 0 = stream skipped, its state
                                        and its rows of out untouched                        */
  const int* adapt;                  /* device [streams] or NULL = all adapt                  */
  const float* mix;  long long mix_stride, ch_stride;      /* [streams][2][hops*hop]         */
  const float* ref_tgt; const float* ref_int; long long ref_stride;   /* IBM                  */
  const float* ext_mask; long long mask_stride_b, mask_stride_f, mask_stride_t; /* [s][F][hops] */
  float* out; long long out_stride;  /* [streams][hops*hop], 16-byte aligned, stride % 4 == 0 */
  float* w_out;  double* cov_out;    /* optional: weights [streams][F][4] / sums [streams][F][5]
                                        after the call's last frame                          */
  float* mask_out;                   /* optional debug: n_t used, [streams][F][hops] contiguous */
  void* state; long long state_bytes;
} avz_stream_args;
int avz_stream_push(const avz_plan* plan, const avz_stream_args* args, void* hip_stream);

/* ------------------------------------------------------------------ streaming online WPE
 * The causal form of WPE: recursive-least-squares (RLS) online WPE (Yoshioka et al. 2009;
 * Caroselli et al. 2017), run hop by hop with the framing and the state rules of
 * avz_stream_push, whose first stage it is. The algorithm is the contract (DESIGN.md section
 * 15; avz/dereverb.py wpe_stream_numpy is the fp64 restatement); no bit parity with nara_wpe
 * is claimed. Per stream, with H = n_fft / 2, x_t the t-th hop pushed since the last reset
 * (two mics), x_-1 = 0, K = taps, D = delay, n = 2 K and W = K + D + 1; per frame t and bin k
 * (all F bins, DC and Nyquist included):
 *  - analysis: Y_t = rfft(w [x_t-1 | x_t]) / sum(w) under the plan's fp32 periodic Hann, the
 *    frame avz_stream_push forms, rounded to complex64; everything below takes that value,
 *    promoted to fp64;
 *  - regressor y~_t in C^n: row 2 tau + m is Y[m, t - D - tau], tau = 0 .. K-1, and 0 where
 *    that frame index is negative (the row order of avz_wpe_spectral);
 *  - output z_t = y_t - G_t-1^H y~_t (both mics): the a-priori prediction error;
 *  - power p_t = (1 / (2 W)) sum_{s = max(0, t-W+1)}^{t} sum_m |Y[m, s]|^2 (fixed divisor);
 *  - RLS step, where the stream's adapt flag is non-zero: u = Q_t-1 y~_t,
 *    den = forget max(p_t, power_floor) + Re(y~_t^H u), k = u / den, G_t = G_t-1 + k z_t^H,
 *    Q_t = (Q_t-1 - k u^H) / forget, taken as a product with 1 / forget rounded once. Q_t is
 *    kept exactly Hermitian: the lower triangle is computed and mirrored, the diagonal is
 *    real. With adapt = 0, G and Q stay and z_t is computed with the frozen filter;
 *  - start: G_-1 = 0, Q_-1 = q_init I. All state arithmetic is fp64;
 *  - synthesis per mic, as avz_stream_push: g_t = irfft(z_t) sum(w) w, output hop t =
 *    (g_t-1[H:] + g_t[:H]) / (w^2[j] + w^2[j + H]) for t >= 1 and zeros for t = 0: one hop of
 *    algorithmic latency; one extra hop of zeros drains the tail.
 * The plan supplies n_fft, the window and max_batch; its mask, beamformer and normalisation
 * settings are ignored.
 *
 * The state is one caller-owned device buffer of avz_wpe_stream_state_bytes(plan, streams,
 * taps, delay) bytes, 256-byte aligned; its layout is private. Per stream: a header (frame
 * count, taps, delay, n_fft), the previous hop of both mics, both synthesis tails, a complex64
 * ring of the W most recent frames plus the 8 of a call's current round, the round's Z, and in
 * fp64 G [F][n][2] and the lower triangle of Q [F][n (n + 1) / 2]: per bin
 * 16 (K + D + 17) + 64 K + 16 K (2 K + 1) bytes, i.e. 4480 B at K = 10, D = 3 and 10048 B at
 * K = 16, D = 3; a stream takes 1.15 MB (n_fft 512) or 2.30 MB (1024) at K = 10 and 2.58 /
 * 5.16 MB at K = 16. No call allocates device memory.
 *  avz_wpe_stream_reset  starts the selected streams (select[s] != 0; NULL = all): zero
 *                        history, G = 0, Q = q_init I. A new buffer must be reset first. taps
 *                        and delay are fixed here: they are recorded in each stream's header
 *                        and, on the host, against the buffer's address.
 *  avz_wpe_stream_push   `hops` >= 1 new hops per stream; out gets the same number of samples
 *                        per mic. A push whose taps or delay differ from those the buffer was
 *                        last reset with at this address (or on a buffer never reset in this
 *                        process) returns AVZ_ERR_ARG; the kernels also skip a stream whose
 *                        header differs.
 * Checks, all on the host before any HIP call: a NULL plan, args, mix, out or state, taps
 * outside 1 .. 16, delay outside 1 .. 8, forget outside (0, 1], power_floor <= 0, q_init <= 0
 * or hops < 1: AVZ_ERR_ARG; streams outside 1 .. max_batch, ch_stride or out_ch_stride <
 * hops * hop, (streams > 1) mix_stride < ch_stride + hops * hop or out_stride < out_ch_stride
 * + hops * hop, or state_bytes too small: AVZ_ERR_SHAPE; state not 256-byte aligned, out not
 * 16-byte aligned or out_stride / out_ch_stride not a multiple of 4: AVZ_ERR_ALIGN.
 * Guarantees, as avz_stream_push: a stream's outputs and whole final state are bit-identical
 * however its hops are grouped into calls, whatever its index and whatever the other streams
 * hold; a NaN in one stream never reaches another. Calls on one state buffer must be
 * stream-ordered. out [streams][2][hops*hop] can be pushed straight into avz_stream_push as
 * its mix (two hops of latency in all). */
long long avz_wpe_stream_state_bytes(const avz_plan* plan, int streams, int taps, int delay);
int avz_wpe_stream_reset(const avz_plan* plan, void* state, long long state_bytes, int streams,
                         int taps, int delay, double q_init,
                         const int* select /* device [streams] or NULL = all */,
                         void* hip_stream);
typedef struct avz_wpe_stream_args {
  int streams, hops, taps, delay;
  double forget, power_floor;
  const int* active;            /* device [streams] or NULL; 0 = state and out rows untouched */
  const int* adapt;             /* device [streams] or NULL = all adapt */
  const float* mix; long long mix_stride, ch_stride;        /* [streams][2][hops*hop] */
  float* out;       long long out_stride, out_ch_stride;    /* [streams][2][hops*hop] */
  float* Y_out; float* Z_out;   /* optional debug, complex64 [streams][2][F][hops] contiguous */
  double* G_out;                /* optional, complex128 [streams][F][n][2] after the last frame */
  void* state; long long state_bytes;
} avz_wpe_stream_args;
int avz_wpe_stream_push(const avz_plan* plan, const avz_wpe_stream_args* args, void* hip_stream);

/* ------------------------------------------------------------------ blind delay-histogram mask
 * A target-probability mask for AVZ_MASK_EXTERNAL plans that needs neither references nor a
 * trained model: the delay-only form of DUET (Yilmaz & Rickard 2004). The algorithm is the
 * contract (avz/delay_mask.py delay_mask_numpy is the fp64 restatement).
 * The plan supplies N = n_fft, H = N / 2, F = H + 1, fs, d = mic_d and c = c_sound; its mask
 * mode, beamformer and post-filter are ignored. Y0, Y1: the two mic spectra of avz_stft.
 * omega_k = 2 pi k / N; delta_max = d fs / c samples; R = 1.25 delta_max; hist_bins bins of
 * width D = 2 R / hist_bins, bin i centred at -R + (i + 1/2) D. With mic 0 at +d/2 a far-field
 * source at azimuth theta gives Y1 / Y0 = e^{+i omega_k delta}, delta = delta_max cos(theta).
 *  1. Histogram, per utterance: for k_lo = max(1, ceil(f_lo_hz N / fs)) <= k <= k_hi =
 *     min(N / 2, ceil(N / (2 R)) - 1) (no delay inside the range aliases) and every frame:
 *     X = Y1 conj(Y0), w = |X|, delta = arg(X) / omega_k, u = (delta + R) / D - 1/2,
 *     i0 = floor(u), phi = u - i0; h[i0] += (1 - phi) w and h[i0 + 1] += phi w, each where the
 *     index lies in 0 .. hist_bins - 1. A pair whose u or w is not finite deposits nothing.
 *     k_hi < k_lo: h = 0. The spectra and w are fp32 (atan2f); h is summed in fp64.
 *  2. Peaks (fp64): `smooth` passes of hs[i] = hs[i-1]/4 + hs[i]/2 + hs[i+1]/4 (zeros
 *     outside). Bin i is a candidate when max hs > 0, hs[i] > hs[i-1], hs[i] >= hs[i+1] and
 *     hs[i] >= rel_height max hs; its delay is -R + (i + 1/2 + o) D with l = hs[i-1],
 *     r = hs[i+1], o = (l - r) / (2 (l - 2 hs[i] + r)), or 0 when that denominator is 0.
 *     Candidates with |delay - delta_t| <= min_sep delta_max, delta_t = delta_max
 *     cos(angle), are the target itself and are dropped; of the others the J <= max_peaks
 *     highest are kept (ties: the lower bin first). The list is delta_0 = delta_t (always the
 *     geometric value) followed by the J kept delays, highest first.
 *  3. Mask, for every bin 0 .. F - 1 and every frame: cost_j = |Y1 - e^{i omega_k delta_j}
 *     Y0|^2 (fp32; rotations from fp64); M = 0 if some j >= 1 has cost_j < cost_0 strictly,
 *     else 1. Ties, k = 0, an all-zero mixture, J = 0 and NaNs all give 1.
 * M is the target probability ext_mask takes (noise weight 1 - M). Frames past an utterance's
 * own count are not written (as avz_stft); a row with len < n_fft is not processed: its
 * n_peaks is -1 and nothing else of it is written.
 * Checks, all on the host before any HIP call (avz_delay_mask_check runs them on a bare
 * configuration): a NULL plan, args, len, mix, mask or workspace, hist_bins even or outside
 * 9 .. 257, smooth outside 0 .. 8, max_peaks outside 0 .. 7, rel_height outside (0, 1],
 * min_sep or f_lo_hz negative or NaN: AVZ_ERR_ARG; batch outside 1 .. max_batch, max_len
 * outside [n_fft, max_samples], ch_stride < max_len, (batch > 1) mix_stride < ch_stride +
 * max_len, mask strides that are not positive or let two of the F x T elements of a row (or
 * two rows) share an address, or workspace_bytes too small: AVZ_ERR_SHAPE; workspace not
 * 256-byte aligned: AVZ_ERR_ALIGN. No call allocates device memory.
 * Guarantees: results are bit-identical from call to call, whatever the utterance's index and
 * whatever the other utterances hold (a NaN in one never reaches another); scaling a mixture
 * by a power of two changes neither its delays nor its mask. */
typedef struct avz_delay_mask_args {
  int batch; const int* len; int max_len;           /* as avz_stft */
  const float* mix; long long mix_stride, ch_stride;
  const double* angle_deg;     /* optional device [batch]: target azimuth per utterance (the
                                  camera's); NULL = the plan's angle_deg */
  int hist_bins, smooth, max_peaks;  /* odd 9..257; 0..8; 0..7 */
  double rel_height, min_sep, f_lo_hz;  /* (0, 1]; >= 0; >= 0 */
  float* mask; long long mask_stride_b, mask_stride_f, mask_stride_t;  /* ext_mask's layout */
  double* hist_out;            /* optional [batch][hist_bins]: h before smoothing */
  double* delays_out;          /* optional [batch][8]: delta_t, then the J kept delays, NaN-padded */
  int* n_peaks;                /* optional [batch]: J, or -1 for a row with len < n_fft */
  void* workspace; long long workspace_bytes;       /* 256-byte aligned */
} avz_delay_mask_args;
long long avz_delay_mask_workspace_bytes(const avz_plan* plan, int batch, int max_len,
                                         int hist_bins);
int avz_delay_mask(const avz_plan* plan, const avz_delay_mask_args* args, void* hip_stream);
int avz_delay_mask_check(const avz_config* cfg, const avz_delay_mask_args* args); /* host checks only */

/* ------------------------------------------------------------------ streaming blind delay mask
 * avz_delay_mask hop by hop: a recursive histogram with causal labels, on the frames
 * avz_stream_push forms, so that its mask feeds an AVZ_MASK_EXTERNAL plan's avz_stream_push of
 * the same hops. The algorithm is the contract (avz/delay_mask.py
 * delay_mask_stream_numpy is the fp64 restatement). From the plan: N = n_fft, H = N / 2,
 * F = H + 1, fs, d = mic_d, c = c_sound, max_batch; its mask mode, beamformer, post-filter and
 * normalisation are ignored. The grid is avz_delay_mask's, unchanged: omega_k, delta_max,
 * R = 1.25 delta_max, hist_bins bins of width D, the band k_lo .. k_hi.
 * Per stream, x_t is the t-th hop pushed since the last reset (two mics) and x_-1 = 0. For
 * every frame t, in order:
 *  1. Frame. Y_t is the frame avz_stream_push forms: [x_t-1 | x_t] under the plan's fp32
 *     periodic Hann, scaled by 1 / sum(w).
 *  2. Deposit. d_t[i] is avz_delay_mask's stage 1 restricted to frame t's band bins: u, w and
 *     the two-bin split in fp32 (w = |Y0| |Y1|, atan2f); the deposits of one frame are summed
 *     in fp64 in an order that depends on the frame alone. A pair whose u or w is not finite
 *     deposits nothing.
 *  3. Recursion (fp64, state): h_t = forget h_t-1 + d_t where the stream's adapt flag is
 *     non-zero, else h_t = h_t-1 (the histogram freezes, for example while the target is known
 *     absent); h_-1 = 0.
 *  4. Peaks. avz_delay_mask's stage 2 on h_t with the call's smooth, rel_height, min_sep and
 *     max_peaks and the stream's target azimuth: the list (delta_0 = delta_max cos(theta), then
 *     the J_t kept delays).
 *  5. Labels. avz_delay_mask's stage 3 on frame t with the list of step 4: every bin
 *     0 .. F - 1, the rotations from fp64. Ties, k = 0, a zero frame, J_t = 0 and NaNs give 1.
 *     M[:, t] uses frames <= t only: it is causal.
 * Relation to the offline mask: with forget = 1, after a signal of T hops plus one drain hop
 * of zeros, h is the offline histogram of that T H-sample signal (the frames are scipy's padded
 * frames; up to fp64 association and the two transforms' fp32 rounding). With forget < 1, h
 * tracks moving interferers. Scaling a stream's input by a power of two changes no delay and
 * no label.
 * The state is one caller-owned device buffer of avz_delay_stream_state_bytes(plan, streams,
 * hist_bins) bytes, 256-byte aligned; its layout is private. Per stream: a 64-byte header (the
 * 64-bit frame count, hist_bins, n_fft), the previous hop of both mics [2][H] f32 and h
 * [hist_bins] f64, rounded up to 256 bytes: 4864 bytes per stream at N = 1024, hist_bins = 65
 * (2816 at N = 512).
 *  avz_delay_stream_reset  starts the selected streams (select[s] != 0; NULL = all): zero
 *                          history, h = 0. hist_bins is fixed here: it is recorded in each
 *                          stream's header and, on the host, against the buffer's address. A
 *                          partial reset (select != NULL) must repeat the buffer's hist_bins.
 *  avz_delay_stream_push   `hops` >= 1 new hops per stream; mask gets one column per hop. A
 *                          push whose hist_bins differs from that record, or a push on a
 *                          buffer never reset in this process, returns AVZ_ERR_ARG; the kernel
 *                          also leaves a stream untouched when its header differs. A stream
 *                          with active[s] == 0 keeps its state, and its rows of every output
 *                          stay unwritten.
 * Checks, all on the host before any HIP call (avz_delay_stream_check runs the push's on a bare
 * configuration): a NULL plan, args, mix, mask or state, hops < 1, forget outside (0, 1],
 * hist_bins even or outside 9 .. 257, smooth outside 0 .. 8, max_peaks outside 0 .. 7,
 * rel_height outside (0, 1], min_sep or f_lo_hz negative or NaN: AVZ_ERR_ARG; streams outside
 * 1 .. max_batch, ch_stride < hops * hop, (streams > 1) mix_stride < ch_stride + hops * hop,
 * mask strides that are not positive or let two of the [streams][F][hops] elements share an
 * address, or state_bytes too small: AVZ_ERR_SHAPE; state not 256-byte aligned: AVZ_ERR_ALIGN.
 * Guarantees: a stream's masks, per-frame delay lists and whole final state are bit-identical
 * however its hops are grouped into calls, whatever its index and whatever the other streams
 * hold, as long as the per-call parameters stay the same; a NaN in one stream never reaches
 * another; no call allocates device memory; no atomics and no inter-block traffic. */
long long avz_delay_stream_state_bytes(const avz_plan* plan, int streams, int hist_bins);
int avz_delay_stream_reset(const avz_plan* plan, void* state, long long state_bytes, int streams,
                           int hist_bins, const int* select /* device or NULL = all */,
                           void* hip_stream);
typedef struct avz_delay_stream_args {
  int streams, hops;                 /* hops >= 1 new hops per stream */
  double forget;                     /* (0, 1] */
  const int* active; const int* adapt;          /* device [streams] or NULL, as avz_stream_args */
  const float* mix; long long mix_stride, ch_stride;   /* [streams][2][hops*hop] */
  const double* angle_deg;           /* optional device [streams]; NULL or a NaN entry = the plan's */
  int hist_bins, smooth, max_peaks; double rel_height, min_sep, f_lo_hz;   /* ranges of avz_delay_mask */
  float* mask; long long mask_stride_b, mask_stride_f, mask_stride_t;     /* [streams][F][hops]: avz_stream_args.ext_mask's layout */
  double* hist_out;                  /* optional [streams][hist_bins]: h after the call's last frame */
  double* delays_out;                /* optional [streams][hops][8]: each frame's list, NaN-padded */
  int* n_peaks;                      /* optional [streams][hops]: J_t */
  void* state; long long state_bytes;
} avz_delay_stream_args;
int avz_delay_stream_push(const avz_plan* plan, const avz_delay_stream_args* args, void* hip_stream);
int avz_delay_stream_check(const avz_config* cfg, const avz_delay_stream_args* args); /* host checks only */

const char* avz_strerror(int code);
/* Last HIP error string recorded by the library on this thread (diagnostics). */
const char* avz_last_hip_error(void);
int avz_version(void);

#ifdef __cplusplus
}
#endif
#endif /* AVZ_H_ */
