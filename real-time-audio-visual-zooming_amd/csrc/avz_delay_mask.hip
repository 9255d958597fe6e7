// avz_delay_mask.hip — blind delay-histogram (DUET-style) target mask of a two-mic mixture
// (avz_delay_mask; the contract is in include/avz.h and DESIGN.md section 17, the fp64
// restatement in avz/delay_mask.py).
//
// Three launches, no spectrum in memory; the arithmetic of each stage (pair, deposit, peaks,
// rotation, cost) is avz_delay_common.hpp's, this file holds the batch layout around it:
//   avz_delay_hist_kernel<N>   one block per (utterance, 16 frames), avz_stft_kernel's framing
//                              and packed two-mic transform. Thread (bin k, frame group) turns
//                              its bins into (u, w) pairs in place in the LDS slots (only that
//                              thread ever reads Z[k] and Z[N - k]); then thread (histogram bin
//                              i, segment s) scans its segment of the band's pairs in a fixed
//                              order and the segments are added in order: the block's partial
//                              histogram, written to the workspace. No atomics anywhere.
//   avz_delay_peaks_kernel     one block per utterance: adds the partials in block order
//                              (fp64), then delay_peaks: the candidate list (delta_t first) to
//                              the workspace and the optional outputs.
//   avz_delay_label_kernel<N>  the transform again; thread (bin k, frame group) holds the 1 + J
//                              rotations of its bin in registers, writes its decisions in place
//                              into the slots, and the block stores them frame-fastest.
// Every sum has a fixed order that depends on the utterance alone, so the results are
// bit-identical from call to call and whatever the utterance's index or neighbours; a power-
// of-two scaling of the mixture scales every weight exactly and changes no delay and no label.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avz_delay_mask.hpp"
#include "avz_frame.hpp"

namespace avz {

static_assert(Geo<1024, kStftThreads>::NSLOT == kDelayFrames, "16 frames per block");
static_assert(Geo<512, kStftThreads>::NSLOT == kDelayFrames, "16 frames per block");

// LDS of both kernels: avz_stft_kernel's map (slots, then the twiddles at TW_OFF); the
// histogram kernel's segment sums [S][nb] f64 (S nb <= 512: 4 KB) start at CARRY_OFF, which
// reaches the twiddles exactly at N = 1024 (2 H f32 = 4 KB) and past the map's end at N = 512.
template <int N>
constexpr int delay_lds_bytes() {
  using G = Geo<N, kStftThreads>;
  static_assert(G::TW_OFF - G::CARRY_OFF >= 4096 || KCfg<N>::TW_BYTES == 0, "segment sums");
  static_assert(G::CARRY_OFF % 8 == 0, "f64 alignment");
  return G::LDS_BYTES > G::CARRY_OFF + 4096 ? G::LDS_BYTES : G::CARRY_OFF + 4096;
}

// This lane group's frame of the mixture's packed mic pair into its slot (avz_stft_kernel's
// framing and scaling: frame_transform of avz_frame.hpp).
template <int N>
__device__ __forceinline__ void delay_mix_frame(const DelayArgs& A, const FrameBlock<N>& B,
                                                unsigned char* lds) {
  Lanes<N> ln;
  ln.init(lds, threadIdx.x);
  const float* xb = A.mix + (long long)B.b * A.mix_stride;
  const rsrc_t re = make_rsrc(xb, B.L), im = make_rsrc(xb + A.ch_stride, B.L);
  StftWindow<N> win;
  win.init(ln.lm);
  frame_transform<N>(ln, re, im, B.s0(ln), win, B.twid);
}

// Thread -> (bin, frames) of the per-bin phases: bin kk = tid mod N/2 with the Nyquist bin in
// place of DC (DC is outside every band and its label is the constant 1), frames
// [fa, fa + 16 / Q) of the block, Q = 512 / (N / 2) threads per bin.
template <int N>
struct BinMap {
  static constexpr int NB = N / 2, Q = kStftThreads / NB, FPT = kDelayFrames / Q;
  int kk, fa;
  bool dc;
  __device__ __forceinline__ void init(int tid) {
    const int k = tid % NB;
    dc = k == 0;
    kk = dc ? NB : k;
    fa = (tid / NB) * FPT;
  }
};

template <int N>
__global__ void __launch_bounds__(kStftThreads, 1) avz_delay_hist_kernel(DelayArgs A) {
  using G = Geo<N, kStftThreads>;
  extern __shared__ __align__(16) unsigned char lds[];
  FrameBlock<N> B;
  if (!B.init(lds, A.len, A.max_len)) return;
  const int b = B.b, f0 = B.f0, T = B.T, tid = threadIdx.x;
  delay_mix_frame<N>(A, B, lds);
  __syncthreads();

  // (u, w) of every band pair, in place: Z_f[kk] <- (u, w)
  BinMap<N> bm;
  bm.init(tid);
  if (bm.kk >= A.p.k_lo && bm.kk <= A.p.k_hi) {
    const float cu = delay_u_scale(N, bm.kk, A.p.bin_w);
    const float u0 = 0.5f * (float)A.p.nb - 0.5f;
#pragma unroll
    for (int q = 0; q < BinMap<N>::FPT; ++q) {
      const int f = bm.fa + q;
      cf* Z = slot_ptr<N>(lds, f);
      Z[bm.kk] = delay_pair(Z[bm.kk], Z[(N - bm.kk) & (N - 1)], cu, u0, f0 + f < T);
    }
  }
  __syncthreads();

  // owner-computes: thread (bin i, segment s) scans pairs [p0, p1) of the band in order
  const int nb = A.p.nb;
  const int S = kStftThreads / nb;
  const int nband = A.p.k_hi >= A.p.k_lo ? A.p.k_hi - A.p.k_lo + 1 : 0;
  const int P = nband * kDelayFrames;
  double* seg = reinterpret_cast<double*>(lds + G::CARRY_OFF);  // [S][nb] <= 512 f64
  const int i = tid % nb, s = tid / nb;
  if (s < S) {
    const int p0 = (int)((long long)P * s / S), p1 = (int)((long long)P * (s + 1) / S);
    const float fi = (float)i;
    double acc = 0.0;
    for (int p = p0; p < p1; ++p) {
      acc += delay_deposit(slot_ptr<N>(lds, p % kDelayFrames)[A.p.k_lo + p / kDelayFrames], fi);
    }
    seg[s * nb + i] = acc;
  }
  __syncthreads();
  if (tid < nb) {
    double h = 0.0;
    for (int q = 0; q < S; ++q) h += seg[q * nb + tid];
    A.part[((long long)b * A.nblk + blockIdx.y) * nb + tid] = h;
  }
}

constexpr int kPeakThreads = 256;

__global__ void __launch_bounds__(kPeakThreads) avz_delay_peaks_kernel(DelayArgs A, int n_fft) {
  __shared__ double hs[2][kDelayMaxBins + 3];
  __shared__ double c_h[kDelayMaxBins + 3], c_d[kDelayMaxBins + 3];
  const int b = blockIdx.x, tid = threadIdx.x, nb = A.p.nb;
  const int H = n_fft / 2;
  const int L = min(A.len[b], A.max_len);
  if (L < n_fft) {
    if (tid == 0) {
      A.count[b] = -1;
      if (A.n_peaks) A.n_peaks[b] = -1;
    }
    return;
  }
  const int T = (L + H - 1) / H + 1;
  const int nblk = (T + kDelayFrames - 1) / kDelayFrames;
  for (int i = tid; i < nb; i += kPeakThreads) {
    double h = 0.0;
    const double* p = A.part + (long long)b * A.nblk * nb + i;
    for (int q = 0; q < nblk; ++q) h += p[(long long)q * nb];
    hs[0][i] = h;
    if (A.hist_out) A.hist_out[(long long)b * nb + i] = h;
  }
  __syncthreads();
  const double d_t = delay_target(A.p, A.angle_deg ? A.angle_deg[b] : A.p.plan_angle);
  const int J = delay_peaks<kPeakThreads>(
      A.p, hs[0], kDelayMaxBins + 3, c_h, c_d, d_t, A.list + (long long)b * kDelayList,
      A.delays_out ? A.delays_out + (long long)b * kDelayList : nullptr);
  if (tid == 0) {
    A.count[b] = J;
    if (A.n_peaks) A.n_peaks[b] = J;
  }
}

template <int N>
__global__ void __launch_bounds__(kStftThreads, 1) avz_delay_label_kernel(DelayArgs A) {
  constexpr int F = N / 2 + 1;
  extern __shared__ __align__(16) unsigned char lds[];
  FrameBlock<N> B;
  if (!B.init(lds, A.len, A.max_len)) return;
  const int b = B.b, f0 = B.f0, T = B.T, tid = threadIdx.x;
  delay_mix_frame<N>(A, B, lds);

  // the bin's rotations e^{i omega_k delta_j}, j = 0 .. J: fp64, rounded to fp32
  BinMap<N> bm;
  bm.init(tid);
  const int J = min(max(A.count[b], 0), kDelayList - 1);
  const double* list = A.list + (long long)b * kDelayList;
  cf rot[kDelayList];
  static_for<0, kDelayList>([&](auto j) {
    rot[j] = {1.0f, 0.0f};
    if (j <= J) rot[j] = delay_rotation(bm.kk, list[j], N);  // block-uniform
  });
  __syncthreads();

#pragma unroll
  for (int q = 0; q < BinMap<N>::FPT; ++q) {
    cf* Z = slot_ptr<N>(lds, bm.fa + q);
    cf y0, y1;
    split_pair(Z[bm.kk], Z[(N - bm.kk) & (N - 1)], y0, y1);
    float cost[kDelayList];
    static_for<0, kDelayList>([&](auto j) { cost[j] = delay_cost(rot[j], y0, y1); });
    bool other = false;
    static_for<1, kDelayList>([&](auto j) { other = other || (j <= J && cost[j] < cost[0]); });
    Z[bm.kk].x = other ? 0.0f : 1.0f;
    if (bm.dc) Z[0].x = 1.0f;  // omega = 0: every cost ties
  }
  __syncthreads();

  float* M = A.mask + (long long)b * A.m_sb;
  for (int idx = tid; idx < F * kDelayFrames; idx += kStftThreads) {
    const int k = idx / kDelayFrames, f = idx % kDelayFrames;
    const int t = f0 + f;
    if (t >= T) continue;
    M[(long long)k * A.m_sf + (long long)t * A.m_st] = slot_ptr<N>(lds, f)[k].x;
  }
}

}  // namespace avz

using namespace avz;

extern "C" int avz_launch_delay_mask(int n_fft, const DelayArgs* a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (a->batch <= 0) return 0;
  if (a->p.nb < 1 || a->p.nb > kDelayMaxBins) return -1;
  return dispatch_n_fft(n_fft, [&](auto n) {
    constexpr int N = decltype(n)::value, lds = delay_lds_bytes<N>();
    const dim3 grid(a->batch, a->nblk);
    if (!lds_ready<avz_delay_hist_kernel<N>>(lds) || !lds_ready<avz_delay_label_kernel<N>>(lds))
      return -3;  // both attributes before the first launch
    int rc = launch<avz_delay_hist_kernel<N>>(grid, kStftThreads, lds, st, *a);
    if (rc == 0) rc = launch<avz_delay_peaks_kernel>(dim3(a->batch), kPeakThreads, 0, st, *a, N);
    if (rc == 0) rc = launch<avz_delay_label_kernel<N>>(grid, kStftThreads, lds, st, *a);
    return rc;
  });
}
