// avz_stoi.hip — batched STOI (Taal, Hendriks, Heusdens, Jensen 2011) on gfx950.
//
// The reference scores stoi(s_tgt, s_est, FS, extended=False) with pystoi
// (Final_pipeline/src/metrics.py:157-160). The contract is the published algorithm as
// avz/stoi.py stoi_numpy states it in fp64, per utterance pair
// (x clean, y processed):
//   1. 16 kHz -> 10 kHz: s10[m] = sum_i s[i] h'[8 m - 5 i + 290], h' = 5 h / sum h, h the
//      581-tap Kaiser design of resample_taps (10 kHz input passes through);
//   2. frames of 256 at hop 128 from 0, 128, ... < n10 - 256 under w = hanning(258)[1:-1];
//      e_j = 20 log10(||w x_j|| + 2^-52); frame j kept iff e_j > max e - 40; the K kept
//      windowed frames of x and y are overlap-added at hop 128;
//   3. the J = K - 1 frames of the joined signals, windowed again, 512-point transform;
//   4. 15 third-octave bands: sqrt of the summed |X[k]|^2 over bins [lo, hi);
//   5. per segment m = 30 .. J and band: alpha = ||X|| / (||Y|| + eps), Y' = min(alpha Y,
//      X (1 + 10^(15/20))), rho = the correlation of the mean-removed unit vectors;
//      d = sum rho / (15 (J - 29));
//   6. J < 30: d = 1e-5, status 1.  A non-finite clean frame energy: d = NaN, status 2.
//
// Four kernels, every floating sum in a fixed order and no atomics (equal bits from call to
// call); an utterance's values never enter another utterance's sums:
//  - resample: one thread per 10-kHz sample, fp64 accumulation over its <= 117 taps (the
//    taps arrive by value in the kernel arguments, 291 doubles of the symmetric h', and are
//    spread into LDS as the five polyphase branches g_p[q] = h'[5 q + p], so that a wave reads
//    at most five distinct, conflict-free LDS addresses per tap; the block's 526 input
//    samples are staged in LDS too, zero outside the signal, so every thread runs the same
//    117 steps with no global load in the loop), stored as fp32;
//  - silence: one block per utterance; a wave sums a frame's windowed energy in fp64, the
//    block takes the maximum, decides in fp64 and scans the decisions (ballot + popcount)
//    into the kept-frame list and K;
//  - band: a block covers 32 joined frames. A joined frame is assembled in fp64 from the up
//    to three kept frames that overlap it, so the overlap-added signals never exist in
//    HBM; it is windowed, rounded to fp32 and transformed with Fft512x2. One complex
//    transform carries two consecutive frames of the SAME signal (lane group 0: x, 1: y):
//    the fp32 transform's error on a frame is then a few 2^-24 of that signal's own frame
//    pair, not of the other signal's, so y's level does not matter (x + i y packing would
//    bury a y 80 dB below x). Band sums of the split spectra in fp64;
//  - segment: one block per utterance over the (band, segment) pairs, 30-term statistics
//    in fp64 registers, one rho per pair, summed per thread in index order, then lanes,
//    then waves.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "avz_fft.hpp"
#include "avz_internal.h"

namespace avz {

constexpr int kStoiThreads = 256;
constexpr int kStoiFrame = 256, kStoiHop = 128, kStoiSeg = 30, kStoiBands = 15;
constexpr int kStoiHalf = 290;        // taps -290 .. 290
constexpr int kStoiBranch = 117;      // taps of a polyphase branch: q = 0 .. 116 (5 q + p <= 580)
constexpr int kStoiBranchStride = 118;  // doubles between branches: 236 dwords = 44 mod 64 banks,
                                        // so the five branches' words at one q share no bank
// input samples a block of 256 outputs touches: i0(last) - (i0(first) - 116) + 1 <= 408 + 118
constexpr int kStoiSpan = 528;
constexpr int kStoiTile = 32;         // joined frames per band-stage block
constexpr double kStoiEps = 0x1p-52;

// bins [edge[b], edge[b + 1]) of band b: nearest bins to 150 2^((2 b -+ 1) / 6) Hz on the
// grid k 10000 / 512 (avz/stoi.py band_edges)
__constant__ int kStoiEdge[kStoiBands + 1] = {7,  9,  11, 14, 17,  22,  27,  34,
                                              43, 55, 69, 87, 109, 138, 174, 219};

struct StoiTaps {
  double h[kStoiHalf + 1];  // h'[290 + t] = h'[290 - t], t = 0 .. 290
};

__device__ __forceinline__ int stoi_len(const StoiArgs& A, int b) {
  const int n = A.len ? A.len[b] : A.max_len;
  return n < 0 ? 0 : (n > A.max_len ? A.max_len : n);
}
__device__ __forceinline__ int stoi_n10(const StoiArgs& A, int len) {
  return A.resample ? (int)((5LL * len + 7) / 8) : len;
}
// np.hanning(258)[1:-1]
__device__ __forceinline__ double stoi_window(int n) {
  return 0.5 - 0.5 * cospi(2.0 * (n + 1) / 257.0);
}
__device__ __forceinline__ void stoi_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ------------------------------------------------------------------------------ resample
// grid (ceil(n10_max / 256), 2 batch): signal blockIdx.y & 1 of utterance blockIdx.y >> 1.
// With resample == 0 (10 kHz input, the stage export asked for) it copies.
__global__ void __launch_bounds__(kStoiThreads) avz_stoi_resample_kernel(StoiArgs A, StoiTaps T) {
  // g[p][q] = h'[5 q + p] (0 past tap 580): sample m with c = 8 m + 290 = 5 i0 + p sums
  // s[i0 - q] g[p][q] over q
  __shared__ double g[5 * kStoiBranchStride];
  const int tid = threadIdx.x;
  for (int i = tid; i < 5 * kStoiBranchStride; i += kStoiThreads) {
    const int p = i / kStoiBranchStride, q = i - p * kStoiBranchStride;
    const int t = 5 * q + p;
    g[i] = (q < kStoiBranch && t <= 2 * kStoiHalf)
               ? T.h[t < kStoiHalf ? kStoiHalf - t : t - kStoiHalf] : 0.0;
  }
  __syncthreads();
  const int b = blockIdx.y >> 1, sig = blockIdx.y & 1;
  const int len = stoi_len(A, b), n10 = stoi_n10(A, len);
  const long long m0 = (long long)blockIdx.x * kStoiThreads, m = m0 + tid;
  if (m0 >= n10) return;  // the whole block
  const float* src = sig ? A.est + (long long)b * A.est_stride : A.clean + (long long)b * A.clean_stride;
  float* dst = A.res + (2LL * b + sig) * A.res_stride;
  if (!A.resample) {
    if (m < n10) dst[m] = src[m];
    return;
  }
  // the block's input span [i_lo, i_lo + kStoiSpan), zero outside [0, len)
  __shared__ float sx[kStoiSpan];
  const long long i_lo = (8 * m0 + kStoiHalf) / 5 - (kStoiBranch - 1);
  for (int k = tid; k < kStoiSpan; k += kStoiThreads) {
    const long long i = i_lo + k;
    sx[k] = (i >= 0 && i < len) ? src[i] : 0.0f;
  }
  __syncthreads();
  const long long c = 8 * m + kStoiHalf;
  const long long i0 = c / 5;
  const double* gp = g + (int)(c - 5 * i0) * kStoiBranchStride;
  const float* sp = sx + (int)(i0 - i_lo);  // sample i0; i0 - i_lo in [116, 524]
  double acc = 0.0;
#pragma unroll 13
  for (int q = 0; q < kStoiBranch; ++q) acc = fma((double)sp[-q], gp[q], acc);
  if (m < n10) dst[m] = (float)acc;
}

// ------------------------------------------------------------------------------- silence
// one block per utterance -> energy[b][j], kept[b][0 .. K), info[b] = status, frames, K,
// segments
__global__ void __launch_bounds__(kStoiThreads) avz_stoi_silence_kernel(StoiArgs A) {
  __shared__ double w[kStoiFrame];
  __shared__ double red[4];
  __shared__ int flag[4];
  __shared__ int wcnt[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int n10 = stoi_n10(A, stoi_len(A, b));
  const int nf = n10 > kStoiFrame ? (n10 - kStoiFrame + kStoiHop - 1) / kStoiHop : 0;
  w[tid] = stoi_window(tid);
  __syncthreads();
  const float* x = A.x10 + (long long)b * A.x10_stride;
  double* e = A.energy + (long long)b * A.nf_max;
  int* kept = A.kept + (long long)b * A.nf_max;

  double vmax = -INFINITY;
  int bad = 0;
  for (int j = wave; j < nf; j += 4) {
    const float* f = x + (long long)j * kStoiHop;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int n = lane + 64 * q;
      const double v = w[n] * (double)f[n];
      s = fma(v, v, s);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const double ej = 20.0 * log10(sqrt(s) + kStoiEps);
    if (lane == 0) e[j] = ej;
    if (!(fabs(ej) <= 1.79769313486231570815e308)) bad = 1;
    vmax = fmax(vmax, ej);
  }
  if (lane == 0) {
    red[wave] = vmax;
    flag[wave] = bad;
  }
  __syncthreads();  // (also orders the e[] stores before the reads below)
  vmax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  bad = flag[0] | flag[1] | flag[2] | flag[3];
  const double thr = vmax - 40.0;

  int K = 0;
  if (!bad) {
    for (int base = 0; base < nf; base += kStoiThreads) {
      const int j = base + tid;
      const bool keep = j < nf && e[j] > thr;
      const unsigned long long m = __ballot(keep);
      if (lane == 0) wcnt[wave] = __popcll(m);
      __syncthreads();
      int off = K;
      for (int q = 0; q < wave; ++q) off += wcnt[q];
      if (keep) kept[off + __popcll(m & ((1ULL << lane) - 1ULL))] = j;
      K += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
      __syncthreads();  // wcnt is rewritten by the next round
    }
  }
  if (tid == 0) {
    const int J = K - 1;
    int* info = A.info + 4LL * b;
    info[0] = bad ? 2 : (J < kStoiSeg ? 1 : 0);
    info[1] = nf;
    info[2] = K;
    info[3] = J >= kStoiSeg ? J - kStoiSeg + 1 : 0;
  }
}

// ---------------------------------------------------------------------------------- band
// grid (ceil((nf_max - 1) / 32), batch). Wave `wave`, round `it` transforms the joined frames
// fa = tile + 2 (wave + 4 it) and fa + 1 of x (lane group 0) and of y (group 1).
__global__ void __launch_bounds__(kStoiThreads) avz_stoi_band_kernel(StoiArgs A) {
  __shared__ __align__(16) cf scr[4][2][Fft512x2::SCRATCH_F2];
  __shared__ double w[kStoiFrame];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.y;
  const int J = A.info[4LL * b + 2] - 1;
  const int tile = blockIdx.x * kStoiTile;
  if (tile >= J) return;  // the whole block
  w[tid] = stoi_window(tid);
  __syncthreads();

  Fft512x2 fft;
  fft.init(lane);
  const int g = lane >> 5, jl = lane & 31;
  const float* s = g ? A.y10 + (long long)b * A.y10_stride : A.x10 + (long long)b * A.x10_stride;
  const int* kept = A.kept + (long long)b * A.nf_max;
  cf* mine = scr[wave][g];

  for (int it = 0; it < kStoiTile / 8; ++it) {
    const int fa = tile + 2 * (wave + 4 * it);
    if (fa >= J) break;  // wave-uniform
    const bool has_b = fa + 1 < J;
    // sample offsets of the kept frames fa - 1 .. fa + 2 (fa + 1 <= J = K - 1 exists)
    const long long o0 = fa >= 1 ? (long long)kept[fa - 1] * kStoiHop : -1;
    const long long o1 = (long long)kept[fa] * kStoiHop;
    const long long o2 = (long long)kept[fa + 1] * kStoiHop;
    const long long o3 = has_b ? (long long)kept[fa + 2] * kStoiHop : -1;
    cf v[16];
    static_for<0, 8>([&](auto r) {
      constexpr int R = decltype(r)::value;
      const int n = jl + 32 * R;
      const double wn = w[n];
      double va, vb = 0.0;
      if constexpr (R < 4) {  // first half: the kept frame's head + its predecessor's tail
        const double wt = w[n + kStoiHop];
        va = wn * (double)s[o1 + n];
        if (o0 >= 0) va += wt * (double)s[o0 + n + kStoiHop];
        if (has_b) vb = wn * (double)s[o2 + n] + wt * (double)s[o1 + n + kStoiHop];
      } else {                // second half: the kept frame's tail + its successor's head
        const double wh = w[n - kStoiHop];
        va = wn * (double)s[o1 + n] + wh * (double)s[o2 + n - kStoiHop];
        if (has_b) vb = wn * (double)s[o2 + n] + wh * (double)s[o3 + n - kStoiHop];
      }
      v[R] = {(float)(va * wn), (float)(vb * wn)};
    });
    static_for<8, 16>([&](auto r) { v[r] = {0.0f, 0.0f}; });  // zero-padded to 512
    fft.forward(v, mine);
    // the group's spectrum in natural order over the transpose scratch (544 >= 512 slots)
    static_for<0, 16>([&](auto k) { mine[fft.k1 + 16 * k + 256 * fft.h2] = v[k]; });
    stoi_wave_lds_sync();
    if (lane < 4 * kStoiBands) {
      const int fr = lane / kStoiBands, band = lane % kStoiBands;
      const int gg = fr >> 1, part = fr & 1;
      const cf* Z = scr[wave][gg];
      double sum = 0.0;
      for (int k = kStoiEdge[band]; k < kStoiEdge[band + 1]; ++k) {
        const cf z = Z[k], zp = Z[512 - k];
        // z = FFT(a + i b): A = (z + conj zp) / 2, B = (z - conj zp) / (2 i)
        const double re = part ? 0.5 * ((double)z.y + (double)zp.y) : 0.5 * ((double)z.x + (double)zp.x);
        const double im = part ? 0.5 * ((double)zp.x - (double)z.x) : 0.5 * ((double)z.y - (double)zp.y);
        sum = fma(re, re, fma(im, im, sum));
      }
      const int f = fa + part;
      if (f < J) A.tob[((2LL * b + gg) * kStoiBands + band) * A.tob_stride + f] = sqrt(sum);
    }
    stoi_wave_lds_sync();  // the next round's transform rewrites the scratch
  }
}

// ------------------------------------------------------------------------------- segment
__global__ void __launch_bounds__(kStoiThreads) avz_stoi_segment_kernel(StoiArgs A) {
  __shared__ double red[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x;
  const int status = A.info[4LL * b], J = A.info[4LL * b + 2] - 1;
  if (status != 0 || J < kStoiSeg) {  // the whole block
    if (tid == 0) A.stoi[b] = status == 2 ? (double)NAN : 1e-5;
    return;
  }
  const int M = J - kStoiSeg + 1;
  const double clip = 1.0 + 5.62341325190349080394;  // 1 + 10^(15/20)
  const double* tx = A.tob + 2LL * b * kStoiBands * A.tob_stride;
  const double* ty = tx + kStoiBands * A.tob_stride;
  double acc = 0.0;
  for (int idx = tid; idx < kStoiBands * M; idx += kStoiThreads) {
    const int band = idx / M, m0 = idx - band * M;
    const double* X = tx + band * A.tob_stride + m0;
    const double* Y = ty + band * A.tob_stride + m0;
    double xv[kStoiSeg], yv[kStoiSeg];
    double sx2 = 0, sy2 = 0, sx = 0;
#pragma unroll
    for (int i = 0; i < kStoiSeg; ++i) {
      xv[i] = X[i];
      yv[i] = Y[i];
      sx2 = fma(xv[i], xv[i], sx2);
      sy2 = fma(yv[i], yv[i], sy2);
      sx += xv[i];
    }
    const double alpha = sqrt(sx2) / (sqrt(sy2) + kStoiEps);
    double syp = 0;
#pragma unroll
    for (int i = 0; i < kStoiSeg; ++i) {
      const double ay = yv[i] * alpha, cx = xv[i] * clip;
      yv[i] = (ay < cx || ay != ay) ? ay : cx;  // np.minimum: a NaN stays
      syp += yv[i];
    }
    const double mx = sx / kStoiSeg, my = syp / kStoiSeg;
    double sxx = 0, syy = 0, sxy = 0;
#pragma unroll
    for (int i = 0; i < kStoiSeg; ++i) {
      const double xc = xv[i] - mx, yc = yv[i] - my;
      sxx = fma(xc, xc, sxx);
      syy = fma(yc, yc, syy);
      sxy = fma(xc, yc, sxy);
    }
    acc += sxy / ((sqrt(sxx) + kStoiEps) * (sqrt(syy) + kStoiEps));
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (tid == 0) A.stoi[b] = (((red[0] + red[1]) + red[2]) + red[3]) / ((double)kStoiBands * M);
}

}  // namespace avz

using namespace avz;

// h' = 5 h / sum h of avz/stoi.py resample_taps, in fp64 on the host: h[t] =
// kaiser(581, 0.1102 (60 - 8.7))[290 + t] * 2 * 5 * (1/16) * sinc(t / 8).
static double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

static const StoiTaps& stoi_taps() {
  static const StoiTaps taps = [] {
    StoiTaps t;
    const double pi = 3.14159265358979323846, beta = 0.1102 * (60.0 - 8.7);
    const double i0b = bessel_i0(beta);
    double sum = 0.0;
    for (int n = 0; n <= kStoiHalf; ++n) {
      const double r = (double)n / kStoiHalf;
      const double kw = bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b;
      const double a = pi * n / 8.0;
      const double sinc = n == 0 ? 1.0 : std::sin(a) / a;
      t.h[n] = kw * 0.625 * sinc;
      sum += n == 0 ? t.h[n] : 2.0 * t.h[n];
    }
    for (int n = 0; n <= kStoiHalf; ++n) t.h[n] *= 5.0 / sum;
    return t;
  }();
  return taps;
}

extern "C" int avz_stoi_taps(double* out /*[291]*/) {
  const StoiTaps& t = stoi_taps();
  for (int n = 0; n <= kStoiHalf; ++n) out[n] = t.h[n];
  return 0;
}

// a->res non-null: run the resampler (or, with resample == 0, the copy for the export)
extern "C" int avz_launch_stoi(const StoiArgs* a, void* stream) {
  if (a->batch <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (a->res && a->n10_max > 0) {
    dim3 grid((unsigned)((a->n10_max + kStoiThreads - 1) / kStoiThreads), 2u * a->batch);
    hipLaunchKernelGGL(avz_stoi_resample_kernel, grid, dim3(kStoiThreads), 0, st, *a, stoi_taps());
  }
  hipLaunchKernelGGL(avz_stoi_silence_kernel, dim3(a->batch), dim3(kStoiThreads), 0, st, *a);
  if (a->nf_max > 1) {
    dim3 grid((unsigned)((a->nf_max - 1 + kStoiTile - 1) / kStoiTile), (unsigned)a->batch);
    hipLaunchKernelGGL(avz_stoi_band_kernel, grid, dim3(kStoiThreads), 0, st, *a);
  }
  hipLaunchKernelGGL(avz_stoi_segment_kernel, dim3(a->batch), dim3(kStoiThreads), 0, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
