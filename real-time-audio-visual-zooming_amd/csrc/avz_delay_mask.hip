// avz_delay_mask.hip — blind delay-histogram (DUET-style) target mask of a two-mic mixture
// (avz_delay_mask; the contract is in include/avz.h and DESIGN.md section 17, the fp64
// restatement in avz/delay_mask.py).
//
// Three launches, no spectrum in memory:
//   avz_delay_hist_kernel<N>   one block per (utterance, 16 frames), avz_stft_kernel's framing
//                              and packed two-mic transform. Thread (bin k, frame group) turns
//                              its bins into (u, w) pairs in place in the LDS slots (only that
//                              thread ever reads Z[k] and Z[N - k]); then thread (histogram bin
//                              i, segment s) scans its segment of the band's pairs in a fixed
//                              order and the segments are added in order: the block's partial
//                              histogram, written to the workspace. No atomics anywhere.
//   avz_delay_peaks_kernel     one block per utterance: adds the partials in block order
//                              (fp64), smooths, finds and ranks the peaks, writes the candidate
//                              list (delta_t first) to the workspace and the optional outputs.
//   avz_delay_label_kernel<N>  the transform again; thread (bin k, frame group) holds the 1 + J
//                              rotations of its bin in registers, writes its decisions in place
//                              into the slots, and the block stores them frame-fastest.
// Every sum has a fixed order that depends on the utterance alone, so the results are
// bit-identical from call to call and whatever the utterance's index or neighbours; a power-
// of-two scaling of the mixture scales every weight exactly and changes no delay and no label.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avz_common.hpp"
#include "avz_delay_mask.hpp"
#include "avz_features.hpp"

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

// Windowed forward transform of this lane group's frame of block (b, f0) into its slot
// (avz_stft_kernel's: scipy scaling, 2 / N times the periodic Hann).
template <int N>
__device__ __forceinline__ void delay_transform(const DelayArgs& A, int b, int f0, int L,
                                                unsigned char* lds, const cf* twid) {
  using C = KCfg<N>;
  constexpr int H = N / 2, PPL = C::PPL;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  typename C::Fft fft;
  fft.init(lane);
  LaneMap<N> lm;
  lm.init(lane);
  const int my_slot = wave * C::FPW + lm.grp;
  cf* spec = slot_ptr<N>(lds, my_slot);
  const float* xb = A.mix + (long long)b * A.mix_stride;
  const rsrc_t re = make_rsrc(xb, L);
  const rsrc_t im = make_rsrc(xb + A.ch_stride, L);
  float wa0, wac, was;
  {
    double s, c;
    sincospi(2.0 * lm.in0 / N, &s, &c);
    const double sc = 2.0 / N;
    wa0 = (float)(0.5 * sc);
    wac = (float)(0.5 * sc * c);
    was = (float)(0.5 * sc * s);
  }
  cf v[PPL];
  const int s0 = (f0 + my_slot) * H - N / 2 + lm.in0;
  static_for<0, PPL>([&](auto r) {
    constexpr int j = (C::IN_STRIDE * 32 / N) * r;
    constexpr float cr = W32::c[j % 32], sr = -W32::s[j % 32];
    const float w = fmaf(was, sr, fmaf(-wac, cr, wa0));
    v[r] = {bload(re, s0 + C::IN_STRIDE * r) * w, bload(im, s0 + C::IN_STRIDE * r) * w};
  });
  fft.forward(v, spec, twid);
  static_for<0, PPL>([&](auto k) { spec[lm.out0 + C::OUT_STRIDE * k] = v[k]; });
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
  using C = KCfg<N>;
  using G = Geo<N, kStftThreads>;
  constexpr int H = G::H;
  extern __shared__ __align__(16) unsigned char lds[];
  cf* twid = reinterpret_cast<cf*>(lds + G::TW_OFF);
  C::Fft::fill_twiddles(twid, threadIdx.x, kStftThreads);
  const int b = blockIdx.x;
  const int f0 = blockIdx.y * kDelayFrames;
  const int tid = threadIdx.x;
  const int L = min(A.len[b], A.max_len);
  const int T = (L + H - 1) / H + 1;
  if (f0 >= T || L < N) return;
  __syncthreads();
  delay_transform<N>(A, b, f0, L, lds, twid);
  __syncthreads();

  // (u, w) of every band pair, in place: Z_f[kk] <- (u, w)
  BinMap<N> bm;
  bm.init(tid);
  if (bm.kk >= A.k_lo && bm.kk <= A.k_hi) {
    // u = arg(X) / (omega_k bin_w) + nb / 2 - 1 / 2
    const float cu = (float)((double)N / (6.283185307179586476925 * bm.kk * A.bin_w));
    const float u0 = 0.5f * (float)A.nb - 0.5f;
#pragma unroll
    for (int q = 0; q < BinMap<N>::FPT; ++q) {
      const int f = bm.fa + q;
      cf* Z = slot_ptr<N>(lds, f);
      cf y0, y1;
      split_pair(Z[bm.kk], Z[(N - bm.kk) & (N - 1)], y0, y1);
      // X = Y1 conj(Y0); w = |X| as |Y0| |Y1| (X^2 would leave fp32's range at low levels)
      const float xr = fmaf(y1.x, y0.x, y1.y * y0.y);
      const float xi = fmaf(y1.y, y0.x, -(y1.x * y0.y));
      float w = sqrtf(fmaf(y0.x, y0.x, y0.y * y0.y)) * sqrtf(fmaf(y1.x, y1.x, y1.y * y1.y));
      float u = fmaf(atan2f(xi, xr), cu, u0);
      if (!(fabsf(u) < __builtin_inff()) || !(w < __builtin_inff()) || f0 + f >= T) {
        u = -4.0f;  // no deposit: a non-finite pair, or a frame past the utterance
        w = 0.0f;
      }
      Z[bm.kk] = {u, w};
    }
  }
  __syncthreads();

  // owner-computes: thread (bin i, segment s) scans pairs [p0, p1) of the band in order
  const int nb = A.nb;
  const int S = kStftThreads / nb;
  const int nband = A.k_hi >= A.k_lo ? A.k_hi - A.k_lo + 1 : 0;
  const int P = nband * kDelayFrames;
  double* seg = reinterpret_cast<double*>(lds + G::CARRY_OFF);  // [S][nb] <= 512 f64
  const int i = tid % nb, s = tid / nb;
  if (s < S) {
    const int p0 = (int)((long long)P * s / S), p1 = (int)((long long)P * (s + 1) / S);
    const float fi = (float)i;
    double acc = 0.0;
    for (int p = p0; p < p1; ++p) {
      const cf e = slot_ptr<N>(lds, p % kDelayFrames)[A.k_lo + p / kDelayFrames];
      const float fl = floorf(e.x);
      const float phi = e.x - fl;
      const float t = fi - fl;  // 0: this bin is i0, 1: it is i0 + 1
      const float wt = t == 0.0f ? 1.0f - phi : (t == 1.0f ? phi : 0.0f);
      acc += (double)(wt * e.y);
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
  const int b = blockIdx.x, tid = threadIdx.x, nb = A.nb;
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
  int cur = 0;
  for (int pass = 0; pass < A.smooth; ++pass) {
    for (int i = tid; i < nb; i += kPeakThreads) {
      const double l = i > 0 ? hs[cur][i - 1] : 0.0, r = i + 1 < nb ? hs[cur][i + 1] : 0.0;
      hs[cur ^ 1][i] = 0.25 * l + 0.5 * hs[cur][i] + 0.25 * r;
    }
    cur ^= 1;
    __syncthreads();
  }
  const double* h = hs[cur];
  double top = h[0];  // numpy's max: a NaN stays
  for (int i = 1; i < nb; ++i) {
    const double v = h[i];
    top = (v > top || v != v) ? v : top;
  }
  const double theta = A.angle_deg ? A.angle_deg[b] : A.plan_angle;
  const double d_t = A.dmax * cos(theta * (3.14159265358979323846 / 180.0));
  for (int i = tid; i < nb; i += kPeakThreads) {
    const double l = i > 0 ? h[i - 1] : 0.0, r = i + 1 < nb ? h[i + 1] : 0.0, m = h[i];
    bool cand = top > 0.0 && m > l && m >= r && m >= A.rel_height * top;
    const double den = l - 2.0 * m + r;
    const double o = den == 0.0 ? 0.0 : 0.5 * (l - r) / den;
    const double d = -A.R + ((double)i + 0.5 + o) * A.bin_w;
    if (cand && fabs(d - d_t) <= A.min_sep * A.dmax) cand = false;  // the target itself
    c_h[i] = cand ? m : -1.0;  // a candidate's height is > 0
    c_d[i] = d;
  }
  __syncthreads();
  // rank among the candidates: higher first, ties to the lower bin
  int total = 0;
  for (int j = 0; j < nb; ++j) total += c_h[j] >= 0.0 ? 1 : 0;
  const int J = min(total, A.max_peaks);
  double* list = A.list + (long long)b * kDelayList;
  double* dout = A.delays_out ? A.delays_out + (long long)b * kDelayList : nullptr;
  for (int i = tid; i < nb; i += kPeakThreads) {
    const double m = c_h[i];
    if (!(m >= 0.0)) continue;
    int rank = 0;
    for (int j = 0; j < nb; ++j) {
      const double v = c_h[j];
      rank += (v > m || (v == m && j < i)) ? 1 : 0;
    }
    if (rank < J) {
      list[1 + rank] = c_d[i];
      if (dout) dout[1 + rank] = c_d[i];
    }
  }
  if (tid == 0) {
    list[0] = d_t;
    if (dout) dout[0] = d_t;
    A.count[b] = J;
    if (A.n_peaks) A.n_peaks[b] = J;
  }
  if (tid > J && tid < kDelayList) {
    list[tid] = __builtin_nan("");
    if (dout) dout[tid] = __builtin_nan("");
  }
}

template <int N>
__global__ void __launch_bounds__(kStftThreads, 1) avz_delay_label_kernel(DelayArgs A) {
  using C = KCfg<N>;
  using G = Geo<N, kStftThreads>;
  constexpr int H = G::H, F = G::F;
  extern __shared__ __align__(16) unsigned char lds[];
  cf* twid = reinterpret_cast<cf*>(lds + G::TW_OFF);
  C::Fft::fill_twiddles(twid, threadIdx.x, kStftThreads);
  const int b = blockIdx.x;
  const int f0 = blockIdx.y * kDelayFrames;
  const int tid = threadIdx.x;
  const int L = min(A.len[b], A.max_len);
  const int T = (L + H - 1) / H + 1;
  if (f0 >= T || L < N) return;
  __syncthreads();
  delay_transform<N>(A, b, f0, L, lds, twid);

  // the bin's rotations e^{i omega_k delta_j}, j = 0 .. J: fp64, rounded to fp32
  BinMap<N> bm;
  bm.init(tid);
  const int J = min(max(A.count[b], 0), kDelayList - 1);
  const double* list = A.list + (long long)b * kDelayList;
  cf rot[kDelayList];
  static_for<0, kDelayList>([&](auto j) {
    rot[j] = {1.0f, 0.0f};
    if (j <= J) {  // block-uniform
      double sn, cs;
      sincospi(2.0 * (double)bm.kk * list[j] / (double)N, &sn, &cs);
      rot[j] = {(float)cs, (float)sn};
    }
  });
  __syncthreads();

#pragma unroll
  for (int q = 0; q < BinMap<N>::FPT; ++q) {
    cf* Z = slot_ptr<N>(lds, bm.fa + q);
    cf y0, y1;
    split_pair(Z[bm.kk], Z[(N - bm.kk) & (N - 1)], y0, y1);
    float cost[kDelayList];
    static_for<0, kDelayList>([&](auto j) {
      const cf r = c_mul(rot[j], y0);
      const float dx = y1.x - r.x, dy = y1.y - r.y;
      cost[j] = fmaf(dx, dx, dy * dy);
    });
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

template <int N>
static int launch_delay_t(const DelayArgs* a, hipStream_t st) {
  const int lds = delay_lds_bytes<N>();
  if (!lds_ready<avz_delay_hist_kernel<N>>(lds)) return -3;
  if (!lds_ready<avz_delay_label_kernel<N>>(lds)) return -3;
  const dim3 grid(a->batch, a->nblk);
  hipLaunchKernelGGL(avz_delay_hist_kernel<N>, grid, dim3(kStftThreads), lds, st, *a);
  if (hipGetLastError() != hipSuccess) return -3;
  hipLaunchKernelGGL(avz_delay_peaks_kernel, dim3(a->batch), dim3(kPeakThreads), 0, st, *a, N);
  if (hipGetLastError() != hipSuccess) return -3;
  hipLaunchKernelGGL(avz_delay_label_kernel<N>, grid, dim3(kStftThreads), lds, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int avz_launch_delay_mask(int n_fft, const DelayArgs* a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (a->batch <= 0) return 0;
  if (a->nb < 1 || a->nb > kDelayMaxBins) return -1;
  if (n_fft == 1024) return launch_delay_t<1024>(a, st);
  if (n_fft == 512) return launch_delay_t<512>(a, st);
  return -4;
}
