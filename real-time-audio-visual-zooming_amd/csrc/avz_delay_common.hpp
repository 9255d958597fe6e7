// avz_delay_common.hpp — what the blind delay-histogram mask (avz_delay_mask.hip) and its
// streaming form (avz_delay_stream.hip) share: the limits, the grid and peak parameters of a
// call, and the arithmetic of the three stages as device helpers. The streaming mask is the
// batch mask's stages run hop by hop because both kernels call these (the fp64 restatement
// avz/delay_mask.py has the same shape: one delay_histogram, one delay_peaks, one
// delay_labels). Not part of the public ABI.
#pragma once
#include "avz_common.hpp"

namespace avz {

constexpr int kDelayMaxBins = 257;  // hist_bins <= this
constexpr int kDelayList = 8;       // delta_t + at most 7 kept delays

// The histogram's grid and the peak rule of one call (filled by avz_capi.cpp delay_params).
struct DelayParams {
  double plan_angle;      // the target angle where the call gives none
  int nb, smooth, max_peaks;
  double rel_height, min_sep;
  double dmax, R, bin_w;  // delta_max = d fs / c, R = 1.25 delta_max, bin_w = 2 R / nb (samples)
  int k_lo, k_hi;         // the histogram's band (k_hi < k_lo: empty)
};

// ---- stage 1: a band pair's histogram coordinate u and weight w, and what it deposits

// The slope of u over arg(X) at bin k: 1 / (omega_k bin_w).
__device__ __forceinline__ float delay_u_scale(int N, int k, double bin_w) {
  return (float)((double)N / (6.283185307179586476925 * k * bin_w));
}

// Z[k], Z[N - k] of the packed two-mic transform -> (u, w), u = arg(X) cu + u0 with
// u0 = nb / 2 - 1 / 2. A non-finite pair or one that is not `live` (a frame past the
// utterance) deposits nothing.
__device__ __forceinline__ cf delay_pair(cf z, cf zp, float cu, float u0, bool live) {
  cf y0, y1;
  split_pair(z, zp, y0, y1);
  // X = Y1 conj(Y0); w = |X| as |Y0| |Y1| (X^2 would leave fp32's range at low levels)
  const float xr = fmaf(y1.x, y0.x, y1.y * y0.y);
  const float xi = fmaf(y1.y, y0.x, -(y1.x * y0.y));
  float w = sqrtf(fmaf(y0.x, y0.x, y0.y * y0.y)) * sqrtf(fmaf(y1.x, y1.x, y1.y * y1.y));
  float u = fmaf(atan2f(xi, xr), cu, u0);
  if (!(fabsf(u) < __builtin_inff()) || !(w < __builtin_inff()) || !live) {
    u = -4.0f;
    w = 0.0f;
  }
  return {u, w};
}

// What the pair e = (u, w) adds to histogram bin i (fi = (float)i): w split between the two
// bins around u.
__device__ __forceinline__ double delay_deposit(cf e, float fi) {
  const float fl = floorf(e.x);
  const float phi = e.x - fl;
  const float t = fi - fl;  // 0: this bin is i0, 1: it is i0 + 1
  const float wt = t == 0.0f ? 1.0f - phi : (t == 1.0f ? phi : 0.0f);
  return (double)(wt * e.y);
}

// ---- stage 2: the peaks of a histogram

// The target's delay at angle theta (degrees).
__device__ __forceinline__ double delay_target(const DelayParams& P, double theta) {
  return P.dmax * cos(theta * (3.14159265358979323846 / 180.0));
}

// The candidate list of the histogram in row 0 of hs: P.smooth passes of (1/4, 1/2, 1/4)
// between the two rows of hs (hs + stride is row 1), the local maxima of at least
// P.rel_height of the top that are not the target itself, the P.max_peaks highest of them by
// descending height. Writes list[0 .. 8) (and dout[0 .. 8) unless null): d_t, the kept delays,
// NaN beyond them. Returns their number J, the same in every thread.
// Barriers: every one of the block's THREADS threads calls this, with row 0 of hs written and
// synchronised. It synchronises after each pass and before the ranking, and not at its end:
// the caller synchronises before any thread reads the list or writes hs, c_h or c_d again.
template <int THREADS>
__device__ __forceinline__ int delay_peaks(const DelayParams& P, double* hs, int stride,
                                           double* c_h, double* c_d, double d_t, double* list,
                                           double* dout) {
  const int tid = threadIdx.x, nb = P.nb;
  int cur = 0;
  for (int pass = 0; pass < P.smooth; ++pass) {
    const double* a = hs + cur * stride;
    double* o = hs + (cur ^ 1) * stride;
    for (int i = tid; i < nb; i += THREADS) {
      const double l = i > 0 ? a[i - 1] : 0.0, r = i + 1 < nb ? a[i + 1] : 0.0;
      o[i] = 0.25 * l + 0.5 * a[i] + 0.25 * r;
    }
    cur ^= 1;
    __syncthreads();
  }
  const double* h = hs + cur * stride;
  double top = h[0];  // numpy's max: a NaN stays
  for (int i = 1; i < nb; ++i) {
    const double v = h[i];
    top = (v > top || v != v) ? v : top;
  }
  for (int i = tid; i < nb; i += THREADS) {
    const double l = i > 0 ? h[i - 1] : 0.0, r = i + 1 < nb ? h[i + 1] : 0.0, m = h[i];
    bool cand = top > 0.0 && m > l && m >= r && m >= P.rel_height * top;
    const double den = l - 2.0 * m + r;
    const double o = den == 0.0 ? 0.0 : 0.5 * (l - r) / den;
    const double d = -P.R + ((double)i + 0.5 + o) * P.bin_w;
    if (cand && fabs(d - d_t) <= P.min_sep * P.dmax) cand = false;  // the target itself
    c_h[i] = cand ? m : -1.0;  // a candidate's height is > 0
    c_d[i] = d;
  }
  __syncthreads();
  // rank among the candidates: higher first, ties to the lower bin
  int total = 0;
  for (int j = 0; j < nb; ++j) total += c_h[j] >= 0.0 ? 1 : 0;
  const int J = min(total, P.max_peaks);
  for (int i = tid; i < nb; i += THREADS) {
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
  if (tid > J && tid < kDelayList) {
    list[tid] = __builtin_nan("");
    if (dout) dout[tid] = __builtin_nan("");
  }
  if (tid == 0) {  // last: the caller's own thread-0 writes follow
    list[0] = d_t;
    if (dout) dout[0] = d_t;
  }
  return J;
}

// ---- stage 3: a bin's label

// e^{i omega_kk delta}: fp64, rounded to fp32.
__device__ __forceinline__ cf delay_rotation(int kk, double delta, int N) {
  double sn, cs;
  sincospi(2.0 * (double)kk * delta / (double)N, &sn, &cs);
  return {(float)cs, (float)sn};
}

// |Y1 - rot Y0|^2: the bin goes to the delay of the least cost.
__device__ __forceinline__ float delay_cost(cf rot, cf y0, cf y1) {
  const cf r = c_mul(rot, y0);
  const float dx = y1.x - r.x, dy = y1.y - r.y;
  return fmaf(dx, dx, dy * dy);
}

}  // namespace avz
