// avz_internal.h — host/device shared argument blocks (not part of the public ABI).
#pragma once
#include <stdint.h>
#include <string.h>

namespace avz {

enum : int { MASK_IBM = 0, MASK_IPD = 1, MASK_EXTERNAL = 2, MASK_ONES = 3 };
enum : int { PF_NONE = 0, PF_IBM_TARGET = 1, PF_EXT_FLOOR = 2, PF_EXT_MUL = 3, PF_IRM = 4 };
enum : int { NORM_NONE = 0, NORM_PEAK = 1 };

enum : int { BF_MVDR = 0, BF_HYBRID_NULL = 1 };

// Everything the analysis / solve / synthesis / finalize chain needs, passed by value.
struct PieceState {
  uint32_t cnt, fin;
  unsigned long long st;
};
static_assert(sizeof(PieceState) == 16, "one 16-B store resets it");

// Pieces a shared unit of the exact IBM path splits into at most (avz_chain_exact.hpp XPieces).
constexpr int kXPieces = 8;

// Level rule of the exact-IBM certificate (avz_chain_common.hpp ibm_uncertain): the frame
// energies E for which an fp32 decision may be certified at all, as float bits [lo, lo + span]
// (positive floats order as their bits, so the kernels test `bits(E) - lo > span`, unsigned:
// one compare that also sends 0, inf and NaN outside). c is delta per unit sqrt(E): delta =
// c sqrt(E), with E the energy the kernel sums -- raw samples and c = cert 2 / N on the
// reference-bit path (2 / N: the scaled window's maximum), windowed samples and c = cert on
// the per-bin paths. Either way every windowed sample, transform intermediate and spectrum
// component of the frame is at most sqrt(2 N) sqrt(E) <= 2^6 sqrt(E) in magnitude (N <= 1024).
// u = 2^-126 is the smallest normal fp32 number: a result below it may be flushed or lose
// bits, an absolute error of at most u per operation, which the relative-error bound delta
// does not cover. The thresholds keep those errors 2^12 below the quantities they touch (the
// certificate's own slack, 3.9 against 2 sqrt 2 + 1, is 2^-5.8):
//   E >= 2^-100      E sums 2 N <= 2^11 squares, each off by at most u: 2^-115 in all
//   c^2 E >= 2^-114  every bound compared is at least 3.9 delta^2 >= 2^12 u, so the product D
//                    (two roundings that can underflow) is trusted against it; delta >= 2^-57
//                    also dwarfs the transform's summed underflow errors (< 2^15 u)
//   E <= 2^100       E, the components (<= 2^56) and D (<= 2^113) stay finite
//   c max(2^6, c) E <= 2^124  the bound 3.9 delta max(|component|, delta) stays finite
// An empty range (an absurd kappa) is returned as lo = bits(1), span = 0: no frame but an
// all-zero one is certified.
inline void ibm_level_range(double c, uint32_t* lo_bits, uint32_t* span) {
  auto bits = [](double x) {
    const float f = (float)x;
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
  };
  auto value = [](uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return (double)f;
  };
  double lo = 0x1p-100, hi = 0x1p100;
  if (c > 0.0) {
    if (0x1p-114 / (c * c) > lo) lo = 0x1p-114 / (c * c);
    const double m = c > 64.0 ? c : 64.0;
    if (0x1p124 / (c * m) < hi) hi = 0x1p124 / (c * m);
  }
  if (!(lo <= hi) || !(lo >= 0x1p-126) || !(hi <= 0x1p127)) lo = hi = 1.0;
  uint32_t a = bits(lo), b = bits(hi);
  if (value(a) < lo) ++a;  // lo rounded up, hi down
  if (value(b) > hi) --b;
  if (a > b) a = b = bits(1.0);
  *lo_bits = a;
  *span = b - a;
}

struct ChainArgs {
  int batch;
  const int* len;             // [B] samples per utterance (device; kernels clamp to max_len)
  int max_len;                // host-validated upper bound of len[] (the buffers' extent)
  const float* mix;           // [B][2][..] planar
  long long mix_stride;       // floats between utterances
  long long ch_stride;        // floats between the two mic channels
  const float* ref_tgt;       // [B][..] or null
  const float* ref_int;       // [B][..] or null
  long long ref_stride;
  const float* ext_mask;      // target-probability mask M[b][k][t] or null
  long long mask_sb, mask_sf, mask_st;
  float* out;                 // [B][out_stride]
  long long out_stride;
  float* peak;                // [B] or null: max|out| before normalisation
  double* cov_out;            // [B][F][5] or null: sum m|y0|^2, sum m|y1|^2, Re/Im sum m y0 y1*, sum m
  float* w_out;               // [B][F][4] or null: Re w0, Im w0, Re w1, Im w1
  double fs, sigma, tau1, tau2, fmin_hz;
  double mic_d, c_sound;
  float weight_eps, pf_floor, norm_eps;
  int postfilter, normalize;
  int beamformer;             // BF_*
  double bypass_hz, cond_max; // hybrid null: mic-0 bypass below, delay-and-sum above
  // chunked path workspace (plan-owned)
  int max_frames;             // frames of the longest utterance (grid extent)
  int nchunk;                 // allocated 32-frame chunks per utterance (workspace stride)
  float* part;                // [B][nchunk][5][F] masked covariance partials (fp32)
  uint32_t* mwords;           // [B][nchunk][F] IBM bits, bit i = frame 32 c + i is noise
  const double* steer;        // [F][4] steering vector d0 (re, im), d1 (re, im), fp64
  float* coef;                // [B][F][4] apply coefficients alpha (re, im), beta (re, im)
  float* heads;               // [B][nchunk][H] chunk's first frame, first-half contribution
  float* tails;               // [B][nchunk][H] chunk's last frame, second-half contribution
  uint32_t* peak_u;           // [B] max |out| over chunk interiors (float bits, atomicMax)
  float* pf_gain;             // [B][nchunk][32][F] IRM post-filter gain (PF_IRM) or null
  int singular_fallback;      // 0: w = [1, 0]; 1: w = [1/2, 1/2]
  // spectrum-input synthesis (avz_istft): S[b][k][t] complex64 replaces the forward FFT of
  // the mixture and the apply step (post-filter still applied); len == null means every
  // utterance is max_len samples long
  const float* spec;
  long long spec_sb, spec_sf; // complex elements; t stride 1
  int spec_frames;            // frames present in S (frames >= spec_frames read as zero)
  int cov_only;               // solve kernel: write cov_out only (the covariance stage export)
  int* flag;                  // [B] item-level (batch_mvdr) fallback flags, zeroed per call
  // Tail splitting of the persistent grids (set per launch by the launcher; zero = off).
  // Analysis: items [0, a_whole) run whole, each later (chunk, utterance) item in a_pieces
  // step-range pieces whose partials go to tpart[(item - a_whole) * a_pieces + p][5][F]
  // (the solve sums them in fp64) and whose IBM bits are merged into mwords atomically.
  int a_whole, a_pieces;
  float* tpart;               // [tpart_slots][5][F]
  int tpart_slots;
  // Per-utterance synthesis: utterances [0, s_whole) whole (in-block seams, peak, rescale),
  // utterances [s_whole, batch) in s_pieces pieces of s_steps steps each, whose boundary
  // half-frames go to pheads / ptails[(b - s_whole) * s_pieces + p][H] for the piece
  // finalize kernel (seams, peak, rescale).
  int s_whole, s_pieces, s_steps;
  float* pheads;
  float* ptails;
  int pseam_slots;
  int b_lo;                   // solve launches: first utterance solved (0 in the chain)
  // In-kernel piece finalize (s_ipf = 1; batches with whole rounds): the piece units run
  // first, the last piece of utterance b to arrive (pstate[b].cnt) forms its seams and peak
  // and publishes 1/peak in pstate[b].fin (float bits, 0 = not yet); each piece rescales its
  // own interior during its block's next utterance, or hands it back to that last arriver
  // (pstate[b].st: bit p = piece p handed back, bit 32 + p = the last arriver has passed
  // it). Reset with peak_u by the analysis kernel.
  int s_ipf;
  PieceState* pstate;
  int dbg_ipf;                // diagnostic (avz_plan_set_diagnostics): 1 = every piece but the
                              // last arriver hands itself back at once, 2 = pieces ignore 1/peak
                              // until their next utterance's end (the protocol's rare paths)
  // Reference-exact IBM decisions (avz_ibm_exact.hpp): ibm_cert = kappa * 2^-24, the error
  // bound of the fp32 reference transform per unit of frame norm (0: every decision from the
  // fp32 transform); xwin [N] the reference's fp32 Hann window, xtw [N][2] W_N^j in fp64
  // (plan tables); xstat (optional, [2]): deferred (bin, frame) decisions, exact noise ones.
  float ibm_cert;
  uint32_t ibm_en_lo, ibm_en_span;  // the certificate's level rule (ibm_level_range)
  const float* xwin;
  const double* xtw;
  unsigned long long* xstat;
  uint32_t* xpend;            // [units][4] per analysis unit (item b * gx + c, or piece
                              // gx * B + q): frames with a deferred decision, frames deferred
                              // whole, the Nyquist bin's deferrals (IBM plans' workspace)
  uint32_t* xdfr;             // [units][F] per-bin deferred frames (IBM without the
                              // reference-bit hand-off), written only for units with deferrals
  uint32_t* xunc;             // [units][32 frames][32] reference-bit path: the frame's
                              // uncertain bins (word l bit k: bin l + 32 k), deferred frames only
  uint32_t* xst;              // [units][2] exact-path work sharing: state, arrivals (closed
                              // between launches; avz_chain_exact.hpp kXOpen)
  float* xres;                // [units][kXPieces][5][F] a shared unit's piece sums
  uint32_t* xhint;            // [units / 32] published units (one bit each)
  long long xst_reset;        // host-only: bytes of xst to zero before the launch (a caller's
                              // workspace, whose contents the library does not know)
  int synth_variant;          // host-only (avz_plan_set_diagnostics): synthesis path, 2 default
  void* const* events;        // host-only: (start, stop) hipEvent_t pairs of the 4 launches, or null
  int n_events;               // host-only: how many of them to use (8, or 2: analysis only)
};

// Spectral-domain beamformer (avz_beamform_spectral) and the solve stage export
// (avz_solve_covariance). Solve parameters come from a ChainArgs (fs, sigma, fmin_hz,
// weight_eps, singular_fallback, bypass_hz, cond_max, postfilter, pf_floor).
struct SpecArgs {
  int batch, frames;
  const float* Y;             // complex64 Y[b][m][k][t], m = 0, 1 (t contiguous)
  long long y_sb, y_sm, y_sf; // complex elements
  const float* M;             // target probability M[b][k][t] (t contiguous)
  long long m_sb, m_sf;
  const double* steer;        // [F][4] d0 (re, im), d1 (re, im)
  float* S;                   // complex64 S[b][k][t] (t contiguous)
  long long s_sb, s_sf;
  double* cov_out;            // [B][F][5] or null
  float* w_out;               // [B][F][4] or null
  const double* cov_in;       // solve stage: [B][F][5] covariance sums
  int* flag;                  // [B] item-level fallback flags (zeroed by the launcher)
};

// WPE dereverberation of a two-mic spectrum (avz_wpe_spectral, avz_wpe.hip).
struct WpeArgs {
  int batch, bins, frames;
  const int* frames_b;        // [B] valid frames per item (clamped to [0, frames]) or null
  int taps, delay, iterations;
  const float* Y;             // complex64 Y[b][m][k][t], m = 0, 1 (t contiguous)
  long long y_sb, y_sm, y_sf; // complex elements
  float* Z;                   // same layout; may be Y itself
  long long z_sb, z_sm, z_sf;
  int* status;                // [B][bins] or null
};

// Batched STOI (avz_stoi_batch, avz_stoi.hip).
struct StoiArgs {
  int batch, max_len;
  const int* len;             // [B] samples (clamped to [0, max_len]) or null = max_len
  int resample;               // 1: 16-kHz input through the 5/8 resampler; 0: 10-kHz input
  int n10_max, nf_max;        // 10-kHz samples / frames of a max_len utterance
  const float* clean;         // [B][clean_stride]
  const float* est;           // [B][est_stride]
  long long clean_stride, est_stride;
  float* res;                 // [B][2][res_stride] 10-kHz signals, or null (resample == 0
  long long res_stride;       // and no export: the resample kernel is not launched)
  const float* x10;           // the 10-kHz clean / processed rows the later kernels read
  const float* y10;
  long long x10_stride, y10_stride;
  double* energy;             // [B][nf_max] frame energies, dB
  int* kept;                  // [B][nf_max] kept-frame list
  int* info;                  // [B][4] status, frames, kept K, segments
  double* tob;                // [B][2][15][tob_stride] band values
  long long tob_stride;
  double* stoi;               // [B]
};

struct StftArgs {
  int batch, channels;        // channels 1 or 2
  const int* len;             // clamped to max_len in the kernel
  int max_len;
  const float* x;             // [B][C][..]
  long long x_stride, ch_stride;
  float* Y;                   // complex64 [B][C][F][t_stride] as float2
  long long y_stride_b, y_stride_c, y_stride_f;  // in complex elements
  int max_frames;
  int feat;                   // 0: write Y; FEAT_*: mask-model features into `F_out`
  float* F_out;
  long long f_sb, f_sc, f_sf, f_st;  // feature strides in floats
};
enum : int { FEAT_NONE = 0, FEAT_LOGMAG_IPD = 1, FEAT_TFLITE = 2 };

// Mask-estimator training batch (avz_mask_training_batch, avz_train.hip): the features of
// `s` (x = the mic pair, feat != FEAT_NONE) and the IBM label of the two references.
struct TrainArgs {
  StftArgs s;
  const float* tgt;           // [B][ref_stride] target reference
  const float* itf;           // [B][ref_stride] interference reference
  long long ref_stride;
  float* label;               // label[b*l_sb + k*l_sf + t*l_st] = 1.0f or 0.0f
  long long l_sb, l_sf, l_st;
};

// Streaming causal MVDR (avz_stream_push / _reset / _steer, avz_stream.hip). The per-stream
// state block (private layout; StreamLayout) is caller-owned device memory.
struct StreamArgs {
  int streams, hops;
  double forget;
  const int* active;          // [streams] or null: 0 = the stream is skipped
  const int* adapt;           // [streams] or null: 0 = the sums (and so the weights) freeze
  const float* mix;           // [streams][2][hops * H] planar
  long long mix_stride, ch_stride;
  const float* ref_tgt;       // [streams][hops * H] (IBM) or null
  const float* ref_int;
  long long ref_stride;
  const float* ext_mask;      // target probability M[s][k][j], j = hop of this call, or null
  long long mask_sb, mask_sf, mask_st;
  float* out;                 // [streams][hops * H]
  long long out_stride;
  float* w_out;               // [streams][F][4] or null
  double* cov_out;            // [streams][F][5] or null
  float* mask_out;            // [streams][F][hops] or null: the noise weight used
  unsigned char* state;       // [streams][state_stride bytes]
  long long state_stride;
  const int* select;          // reset: [streams] or null = all
  const double* angle_deg;    // steer: [streams], NaN = keep
};

// Bytes of one stream's state block for n_fft = N (H = N / 2, F = H + 1): the frame count
// (64-bit, in a 64-byte header), the previous hop of mic 0, mic 1, target and interference
// reference [4][H] f32, the synthesis tail g[H:] [H] f32, the sums c[F][5] f64 and the
// steering table [F][4] f64 (d0 re, im, d1 re, im); rounded up to 256 bytes.
struct StreamLayout {
  long long prev_off = 0, tail_off = 0, cov_off = 0, steer_off = 0, stride = 0;
  constexpr explicit StreamLayout(int n_fft) {  // constexpr: host and device
    const long long H = n_fft / 2, F = H + 1;
    prev_off = 64;
    tail_off = prev_off + 4 * H * 4;
    cov_off = tail_off + H * 4;
    steer_off = cov_off + F * 5 * 8;
    stride = (steer_off + F * 4 * 8 + 255) & ~255LL;
  }
};

// Streaming online WPE (avz_wpe_stream_push / _reset, avz_wpe_stream.hip).
struct WpeStreamArgs {
  int streams, hops, taps, delay;
  double forget, inv_forget, power_floor, q_init;
  const int* active;          // [streams] or null: 0 = the stream is skipped
  const int* adapt;           // [streams] or null: 0 = G and Q freeze
  const float* mix;           // [streams][2][hops * H] planar
  long long mix_stride, ch_stride;
  float* out;                 // [streams][2][hops * H]
  long long out_stride, out_ch_stride;
  float* Y_out;               // complex64 [streams][2][F][hops] or null
  float* Z_out;
  double* G_out;              // complex128 [streams][F][n][2] or null
  unsigned char* state;       // [streams][state_stride bytes]
  long long state_stride;
  const int* select;          // reset: [streams] or null = all
  int j0, nf;                 // the round: hops [j0, j0 + nf) of the call, nf <= 8
};

constexpr int kWpeStreamRound = 8;  // frames per round: the lane groups of a 256-thread block

// One stream's state block for n_fft = N (H = N / 2, F = H + 1), K taps, delay D, n = 2 K,
// W = K + D + 1, R = W + 8 ring slots:
//   header 256 B: frame count (u64), taps, delay, n_fft (i32)
//   prev  [2][H] f32      the previous hop of both mics
//   tail  [2][H] f32      g[H:] of the last frame, both mics
//   ring  [F][R][2] c64   frame t of bin k at slot t mod R (bin-major)
//   zr    [8][F][2] c64   Z of frame t at slot t mod 8: the round's hand-over to the synthesis
//   G     [F][n][2] c128
//   Q     [F][n (n + 1) / 2] c128   lower triangle, row-major: Q[i][j], j <= i
// every section 256-byte aligned, the block rounded up to 256 bytes.
struct WpeStreamLayout {
  long long prev_off = 0, tail_off = 0, ring_off = 0, zr_off = 0, g_off = 0, q_off = 0, stride = 0;
  int n = 0, W = 0, R = 0, tri = 0;
  constexpr WpeStreamLayout(int n_fft, int taps, int delay) {  // constexpr: host and device
    const long long H = n_fft / 2, F = H + 1;
    auto up = [](long long v) { return (v + 255) & ~255LL; };
    n = 2 * taps;
    W = taps + delay + 1;
    R = W + kWpeStreamRound;
    tri = n * (n + 1) / 2;
    prev_off = 256;
    tail_off = up(prev_off + 2 * H * 4);
    ring_off = up(tail_off + 2 * H * 4);
    zr_off = up(ring_off + F * R * 16);
    g_off = up(zr_off + kWpeStreamRound * F * 16);
    q_off = up(g_off + F * n * 32);
    stride = up(q_off + F * tri * 16);
  }
};

struct SrpArgs {
  int n_angles;
  double angle_lo, angle_hi;  // np.linspace(angle_lo, angle_hi, n_angles)
  double f_lo, f_hi;          // bins with f_lo <= f <= f_hi
  double* power_db;           // [B][n_angles]
};

struct MetricsArgs {
  int batch, max_len;
  const int* len;             // [B] samples to score (the aligned minimum length)
  const float* est;           // [B][est_stride] output
  const float* tgt;           // [B][tgt_stride] target reference
  const float* itf;           // [B][itf_stride] interference reference
  long long est_stride, tgt_stride, itf_stride;
  double* sums;               // [B][6] workspace
  double* metrics;            // [B][4] OSINR, OSIR, SDR, SIR (dB)
  const float* est_peak;      // [B] or null: score est / (est_peak[b] + est_eps)
  double est_eps;
};

struct ChunkSplitArgs {
  int n_items, channels, chunk;
  const int* item_utt;        // [n_items] source utterance
  const int* item_start;      // [n_items] first sample
  const int* len;             // [B] utterance lengths
  const float* x;             // [B][channels][..]
  long long x_stride, x_ch_stride;
  float* items;               // [n_items][channels][..]
  long long item_stride, item_ch_stride;
};

struct ChunkMergeArgs {
  int batch, max_len, hop, item_out_len;
  const int* len;             // [B]
  const int* item_base;       // [B] index of each utterance's first item
  const float* item_out;      // [n_items][item_out_stride]
  long long item_out_stride;
  float* y;                   // [B][y_stride]
  long long y_stride;
  float* peak;                // [B] max |y| before normalisation
  int normalize;
  float norm_eps;
};

struct SceneArgs {
  int batch, n_src, n;        // utterances, sources per utterance (target first), samples
  const float* src;           // [B][n_src][n]
  const double* angles_deg;   // [B][n_src] azimuths
  const float* noise;         // [B][2][n] unit-normal AWGN draws
  double mic_d, c_sound, fs, sir_db, snr_db;
  float* hk;                  // O(n^2) fallback workspace [B][n_src][2][n] delay kernels
  float* img;                 // O(n^2) fallback workspace [B][n_src][2][n] source images
  float* mix;                 // [B][mix_stride]: mic channels at ch_stride
  long long mix_stride, ch_stride;
  float* tgt;                 // [B][ref_stride] mic-1 target image / peak
  float* itf;                 // [B][ref_stride] mic-1 interference image / peak
  long long ref_stride;
};

// Shoebox room of the image-source scenes (avz_room, validated; avz_scene.hip).
struct RoomArgs {
  double dim[3];              // edges, m
  double beta;                // wall reflection coefficient sqrt(1 - absorption)
  double mic[2][3];
  double c_sound, fs;
  int max_order, rir_len;     // rir_len from avz_room_rir_samples
};

}  // namespace avz

extern "C" {
// Samples per RIR: floor(fs / c * Dmax) + 42 (may exceed the 8192 the kernel accepts).
long long avz_room_rir_samples(const double* dim, int max_order, double fs, double c_sound);
int avz_room_conv_len(int n, int rir_len);  // smallest 2-3-5-smooth length >= n + rir_len - 1
int avz_launch_room_rir(const avz::RoomArgs* r, int batch, int n_src, const double* src_pos,
                        double* rir, void* stream);
long long avz_scene_reverb_ws(const avz::RoomArgs* r, int batch, int n_src, int n);
// a->angles_deg carries src_pos[b][s][3] here
int avz_launch_scene_reverb(const avz::RoomArgs* r, const avz::SceneArgs* a, void* ws, void* stream);
long long avz_scene_reverb_gen_ws(const avz::RoomArgs* r, int batch, int n_src, int n);
int avz_launch_scene_reverb_generate(const avz::RoomArgs* r, avz::SceneArgs* a, long long start,
                                     uint32_t seed, const double* target_pos,
                                     const double* interferer_pos, void* ws, void* stream);
int avz_launch_scene(const avz::SceneArgs* a, void* ws, void* stream);
int avz_launch_scene_generate(avz::SceneArgs* a, long long start, uint32_t seed, void* ws,
                              void* stream);
long long avz_scene_mix_ws(int batch, int n_src, int n);
int avz_scene_fft_len(int n);  // 1: n factors into 8, 4, 2, 5, 3 (the FFT path)
long long avz_scene_gen_ws(int batch, int n_src, int n);
int avz_launch_chunk_split(const avz::ChunkSplitArgs* a, void* stream);
int avz_launch_metrics(const avz::MetricsArgs* a, void* stream);
int avz_launch_chunk_merge(const avz::ChunkMergeArgs* a, void* stream);
int avz_launch_chunked(int n_fft, int mask_mode, const avz::ChainArgs* a, void* stream);
// Kernels avz_launch_chunked launches for these arguments, bit i = kernel i (analysis,
// solve, synthesis, finalize): the per-utterance synthesis folds finalize in (bit 3 clear)
// and, for plain MVDR plans, the solve too (bit 1 clear); unlaunched kernels' events stay
// unrecorded.
int avz_chain_kernels(int n_fft, const avz::ChainArgs* a);
// stage exports: analysis + partial sums -> cov_out; w [B][F][4] -> coef -> synthesis +
// finalize (post-filter PF_NONE or PF_EXT_MUL with ext_mask as the gain); S -> synthesis
// (spectrum input) + finalize
int avz_launch_covariance(int n_fft, int mask_mode, const avz::ChainArgs* a, void* stream);
int avz_launch_apply_istft(int n_fft, const avz::ChainArgs* a, const float* w, void* stream);
int avz_launch_istft(int n_fft, const avz::ChainArgs* a, void* stream);
int avz_launch_spectral(int n_fft, const avz::SpecArgs* s, const avz::ChainArgs* p, void* stream);
int avz_launch_solve_cov(int n_fft, const avz::SpecArgs* s, const avz::ChainArgs* p, void* stream);
int avz_wpe_max_frames(void);
int avz_launch_wpe(const avz::WpeArgs* a, void* stream);
int avz_launch_stoi(const avz::StoiArgs* a, void* stream);
int avz_stoi_taps(double* out /*[291]*/);  // h'[290 + t], t = 0 .. 290, of the 16 -> 10 kHz resampler
int avz_launch_srp(int n_fft, const avz::ChainArgs* a, const avz::SrpArgs* s, void* stream);
int avz_chunk_frames(void);
int avz_launch_stft(int n_fft, const avz::StftArgs* a, void* stream);
int avz_launch_train(int n_fft, const avz::TrainArgs* a, void* stream);
int avz_launch_stream_push(int n_fft, int mask_mode, const avz::StreamArgs* s,
                           const avz::ChainArgs* p, void* stream);
int avz_launch_stream_reset(int n_fft, const avz::StreamArgs* s, const double* plan_steer,
                            void* stream);
int avz_launch_stream_steer(int n_fft, const avz::StreamArgs* s, double mic_d, double c_sound,
                            double fs, void* stream);
int avz_launch_wpe_stream_push(int n_fft, const avz::WpeStreamArgs* a, const float* xwin,
                               void* stream);
int avz_launch_wpe_stream_reset(int n_fft, const avz::WpeStreamArgs* a, void* stream);
}
