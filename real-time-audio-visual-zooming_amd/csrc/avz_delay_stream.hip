// avz_delay_stream.hip — streaming blind delay-histogram mask (avz_delay_stream_push,
// avz_delay_stream_reset): the three stages of avz_delay_mask run hop by hop, the histogram a
// recursion h_t = forget h_t-1 + d_t and frame t labelled with the peaks of h_t, on the frames
// avz_stream_push forms (the contract is in include/avz.h and DESIGN.md section 19; the fp64
// restatement is avz/delay_mask.py delay_mask_stream_numpy).
//
// Layout: one 256-thread block per stream, resident for the whole call; the block walks the
// call's hops in groups of the eight frames its eight lane groups hold (StreamGeo<N>, as
// avz_stream_kernel). Per group:
//   transform   stream_transform of mic0 + i mic1 into the eight slots;
//   pairs       thread (bin k, frame) turns its band bins into (u, w) in place in the slot (only
//               that thread ever reads Z[k] and Z[N - k]): avz_delay_hist_kernel's arithmetic;
//   deposits    all frames at once: thread (frame, segment s, histogram bin i) scans its fixed
//               share of that frame's band pairs in order and adds what falls on bin i (fp64);
//   recursion   frame by frame, the only serial part: h <- forget h + (the segments added in
//   and peaks   order), the smoothing passes, the candidate test and the ranking by counting of
//               avz_delay_peaks_kernel; the frame's list and J go to a table in LDS and to
//               delays_out / n_peaks;
//   transform   again (the pairs overwrote the band's bins);
//   labels      all frames at once: thread (bin k) holds delta_0's rotation once and forms the
//               others per frame from the table (fp64 sincospi rounded to fp32), writes its
//               decisions in place and the block stores them through the caller's strides.
// A frame's arithmetic is the same instruction sequence whatever its slot, group or call and
// reads nothing of another stream, and every sum has a fixed order that depends on the frame
// alone: a stream's results do not depend on how its hops are grouped into calls, on its index
// or on the other streams. No atomics, no inter-block traffic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avz_common.hpp"
#include "avz_delay_stream.hpp"
#include "avz_stream_common.hpp"

namespace avz {

// LDS map: StreamGeo<N>'s, then h [NBP] f64, two smoothing rows, the candidates' heights and
// delays, the segment sums [8 frames][S nb <= 257] f64, the lists [8][8] f64 and J [8] i32.
template <int N>
struct DelayStreamGeo {
  using SG = StreamGeo<N>;
  static constexpr int NBP = 264;  // a histogram row, padded
  static constexpr int H_OFF = SG::LDS_BYTES;
  static constexpr int HS_OFF = H_OFF + NBP * 8;
  static constexpr int CH_OFF = HS_OFF + 2 * NBP * 8;
  static constexpr int CD_OFF = CH_OFF + NBP * 8;
  static constexpr int SEG_OFF = CD_OFF + NBP * 8;
  static constexpr int LIST_OFF = SEG_OFF + SG::NSLOT * NBP * 8;
  static constexpr int J_OFF = LIST_OFF + SG::NSLOT * kDelayStreamList * 8;
  static constexpr int LDS_BYTES = J_OFF + ((SG::NSLOT * 4 + 15) & ~15);
  static_assert(NBP >= kDelayStreamMaxBins, "a row holds every histogram size");
  static_assert(H_OFF % 8 == 0, "f64 alignment");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// Scan segments per (frame, histogram bin): a function of the histogram size alone.
__device__ __forceinline__ int delay_stream_segments(int nb) {
  return nb >= kStreamThreads ? 1 : kStreamThreads / nb;
}

template <int N>
__global__ void __launch_bounds__(kStreamThreads, 1) avz_delay_stream_kernel(DelayStreamArgs A) {
  using C = KCfg<N>;
  using SG = StreamGeo<N>;
  using DG = DelayStreamGeo<N>;
  constexpr int H = SG::H, F = SG::F, NSLOT = SG::NSLOT, L8 = kDelayStreamList;
  const int s = blockIdx.x;
  if (A.active && A.active[s] == 0) return;
  const int nb = A.nb;
  const DelayStreamLayout lay(N, nb);
  unsigned char* st = A.state + (long long)s * A.state_stride;
  DelayStreamHeader* hdr = reinterpret_cast<DelayStreamHeader*>(st);
  if (hdr->nb != nb || hdr->n_fft != N) return;  // not reset for this call's layout
  float* prev = reinterpret_cast<float*>(st + lay.prev_off);  // [2][H]
  double* h_g = reinterpret_cast<double*>(st + lay.hist_off);
  const unsigned long long count0 = hdr->count;

  extern __shared__ __align__(16) unsigned char lds[];
  cf* twid = reinterpret_cast<cf*>(lds + SG::TW_OFF);
  float* win = reinterpret_cast<float*>(lds + SG::WIN_OFF);
  double* h = reinterpret_cast<double*>(lds + DG::H_OFF);
  double* hs0 = reinterpret_cast<double*>(lds + DG::HS_OFF);
  double* c_h = reinterpret_cast<double*>(lds + DG::CH_OFF);
  double* c_d = reinterpret_cast<double*>(lds + DG::CD_OFF);
  double* seg = reinterpret_cast<double*>(lds + DG::SEG_OFF);
  double* tab = reinterpret_cast<double*>(lds + DG::LIST_OFF);  // [8][8]
  int* Jt = reinterpret_cast<int*>(lds + DG::J_OFF);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  const bool adapt = !A.adapt || A.adapt[s] != 0;
  const double lam = A.forget;
  double theta = A.angle_deg ? A.angle_deg[s] : A.plan_angle;
  if (theta != theta) theta = A.plan_angle;  // NaN: the plan's
  const double d_t = A.dmax * cos(theta * (3.14159265358979323846 / 180.0));

  C::Fft::fill_twiddles(twid, tid, kStreamThreads);
  for (int n = tid; n < N; n += kStreamThreads) win[n] = A.xwin[n];
  for (int i = tid; i < nb; i += kStreamThreads) h[i] = h_g[i];
  __syncthreads();

  typename C::Fft fft;
  fft.init(lane);
  LaneMap<N> lm;
  lm.init(lane);
  const int my_slot = wave * C::FPW + lm.grp;
  cf* spec = slot_ptr<N>(lds, my_slot);

  const float* x0 = A.mix + (long long)s * A.mix_stride;
  const float* x1 = x0 + A.ch_stride;
  float* M = A.mask + (long long)s * A.m_sb;
  const int nband = A.k_hi >= A.k_lo ? A.k_hi - A.k_lo + 1 : 0;
  const int S = delay_stream_segments(nb);
  const int per = S * nb;  // deposit items of one frame: <= 257

  for (int j0 = 0; j0 < A.hops; j0 += NSLOT) {
    const int nf = min(NSLOT, A.hops - j0);
    const bool valid = my_slot < nf;

    stream_transform<N>(fft, lm, x0, x1, prev, prev + H, j0 + my_slot, valid, win, spec, twid);
    __syncthreads();

    // (u, w) of every band pair, in place: Z_f[k] <- (u, w)
    {
      const float u0 = 0.5f * (float)nb - 0.5f;
      for (int idx = tid; idx < nf * nband; idx += kStreamThreads) {
        const int f = idx / nband, k = A.k_lo + idx % nband;
        // u = arg(X) / (omega_k bin_w) + nb / 2 - 1 / 2
        const float cu = (float)((double)N / (6.283185307179586476925 * k * A.bin_w));
        cf* Z = slot_ptr<N>(lds, f);
        cf y0, y1;
        split_pair(Z[k], Z[(N - k) & (N - 1)], y0, y1);
        // X = Y1 conj(Y0); w = |X| as |Y0| |Y1| (X^2 would leave fp32's range at low levels)
        const float xr = fmaf(y1.x, y0.x, y1.y * y0.y);
        const float xi = fmaf(y1.y, y0.x, -(y1.x * y0.y));
        float w = sqrtf(fmaf(y0.x, y0.x, y0.y * y0.y)) * sqrtf(fmaf(y1.x, y1.x, y1.y * y1.y));
        float u = fmaf(atan2f(xi, xr), cu, u0);
        if (!(fabsf(u) < __builtin_inff()) || !(w < __builtin_inff())) {
          u = -4.0f;  // no deposit: a non-finite pair
          w = 0.0f;
        }
        Z[k] = {u, w};
      }
    }
    __syncthreads();

    // owner-computes: item (frame f, segment sg, bin i) scans pairs [p0, p1) of f's band in order
    for (int idx = tid; idx < nf * per; idx += kStreamThreads) {
      const int f = idx / per, r = idx % per;
      const int sg = r / nb, i = r % nb;
      const int p0 = (int)((long long)nband * sg / S), p1 = (int)((long long)nband * (sg + 1) / S);
      const cf* Zb = slot_ptr<N>(lds, f) + A.k_lo;
      const float fi = (float)i;
      double acc = 0.0;
      for (int p = p0; p < p1; ++p) {
        const cf e = Zb[p];
        const float fl = floorf(e.x);
        const float phi = e.x - fl;
        const float t = fi - fl;  // 0: this bin is i0, 1: it is i0 + 1
        const float wt = t == 0.0f ? 1.0f - phi : (t == 1.0f ? phi : 0.0f);
        acc += (double)(wt * e.y);
      }
      seg[idx] = acc;  // [f][sg][i]
    }
    __syncthreads();

    // frame by frame: the recursion, then avz_delay_peaks_kernel's stage 2 on h_t
    for (int f = 0; f < nf; ++f) {
      for (int i = tid; i < nb; i += kStreamThreads) {
        double hv = h[i];
        if (adapt) {
          double d = 0.0;
          for (int q = 0; q < S; ++q) d += seg[(f * S + q) * nb + i];
          hv = fma(lam, hv, d);
          h[i] = hv;
        }
        hs0[i] = hv;
      }
      __syncthreads();
      int cur = 0;
      for (int pass = 0; pass < A.smooth; ++pass) {
        const double* a = hs0 + cur * DG::NBP;
        double* o = hs0 + (cur ^ 1) * DG::NBP;
        for (int i = tid; i < nb; i += kStreamThreads) {
          const double l = i > 0 ? a[i - 1] : 0.0, r = i + 1 < nb ? a[i + 1] : 0.0;
          o[i] = 0.25 * l + 0.5 * a[i] + 0.25 * r;
        }
        cur ^= 1;
        __syncthreads();
      }
      const double* hh = hs0 + cur * DG::NBP;
      double top = hh[0];  // numpy's max: a NaN stays
      for (int i = 1; i < nb; ++i) {
        const double v = hh[i];
        top = (v > top || v != v) ? v : top;
      }
      for (int i = tid; i < nb; i += kStreamThreads) {
        const double l = i > 0 ? hh[i - 1] : 0.0, r = i + 1 < nb ? hh[i + 1] : 0.0, m = hh[i];
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
      double* list = tab + f * L8;
      const long long row = (long long)s * A.hops + (j0 + f);
      double* dout = A.delays_out ? A.delays_out + row * L8 : nullptr;
      for (int i = tid; i < nb; i += kStreamThreads) {
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
        Jt[f] = J;
        if (A.n_peaks) A.n_peaks[row] = J;
      }
      if (tid > J && tid < L8) {
        list[tid] = __builtin_nan("");
        if (dout) dout[tid] = __builtin_nan("");
      }
      __syncthreads();  // the list is complete; hs, c_h and c_d are free for the next frame
    }

    // the spectra again: the pairs overwrote the band's bins
    stream_transform<N>(fft, lm, x0, x1, prev, prev + H, j0 + my_slot, valid, win, spec, twid);
    __syncthreads();

    // labels: bin kk = k with the Nyquist bin in place of DC (omega = 0: every cost ties)
    for (int k = tid; k < N / 2; k += kStreamThreads) {
      const bool dc = k == 0;
      const int kk = dc ? N / 2 : k;
      cf rot0;
      {
        double sn, cs;
        sincospi(2.0 * (double)kk * d_t / (double)N, &sn, &cs);
        rot0 = {(float)cs, (float)sn};
      }
      for (int f = 0; f < nf; ++f) {
        cf* Z = slot_ptr<N>(lds, f);
        cf y0, y1;
        split_pair(Z[kk], Z[(N - kk) & (N - 1)], y0, y1);
        const cf r0 = c_mul(rot0, y0);
        const float dx0 = y1.x - r0.x, dy0 = y1.y - r0.y;
        const float cost0 = fmaf(dx0, dx0, dy0 * dy0);
        const int J = Jt[f];
        bool other = false;
        for (int j = 1; j <= J; ++j) {
          double sn, cs;
          sincospi(2.0 * (double)kk * tab[f * L8 + j] / (double)N, &sn, &cs);
          const cf rj = {(float)cs, (float)sn};
          const cf r = c_mul(rj, y0);
          const float dx = y1.x - r.x, dy = y1.y - r.y;
          other = other || fmaf(dx, dx, dy * dy) < cost0;
        }
        Z[kk].x = other ? 0.0f : 1.0f;
        if (dc) Z[0].x = 1.0f;
      }
    }
    __syncthreads();

    if (A.m_st == 1) {  // frame-fastest
      for (int idx = tid; idx < F * nf; idx += kStreamThreads) {
        const int k = idx / nf, f = idx % nf;
        M[(long long)k * A.m_sf + (j0 + f)] = slot_ptr<N>(lds, f)[k].x;
      }
    } else {
      for (int idx = tid; idx < F * nf; idx += kStreamThreads) {
        const int f = idx / F, k = idx % F;
        M[(long long)k * A.m_sf + (long long)(j0 + f) * A.m_st] = slot_ptr<N>(lds, f)[k].x;
      }
    }
    __syncthreads();  // every slot has been read before the next group's transform
  }

  // the state after the call's last frame
  const long long qlast = (long long)(A.hops - 1) * H;
  for (int m = tid; m < H; m += kStreamThreads) {
    prev[m] = x0[qlast + m];
    prev[H + m] = x1[qlast + m];
  }
  for (int i = tid; i < nb; i += kStreamThreads) {
    h_g[i] = h[i];
    if (A.hist_out) A.hist_out[(long long)s * nb + i] = h[i];
  }
  if (tid == 0) hdr->count = count0 + (unsigned long long)A.hops;
}

// Zero the selected streams' state and write their header.
__global__ void __launch_bounds__(kStreamThreads) avz_delay_stream_reset_kernel(DelayStreamArgs A,
                                                                                int n_fft) {
  const int s = blockIdx.x;
  if (A.select && A.select[s] == 0) return;
  unsigned char* st = A.state + (long long)s * A.state_stride;
  uint32_t* words = reinterpret_cast<uint32_t*>(st);
  const int n_words = (int)(A.state_stride / 4);
  for (int i = 4 + threadIdx.x; i < n_words; i += kStreamThreads) words[i] = 0u;
  if (threadIdx.x == 0) {
    DelayStreamHeader* hdr = reinterpret_cast<DelayStreamHeader*>(st);
    hdr->count = 0ull;
    hdr->nb = A.nb;
    hdr->n_fft = n_fft;
  }
}

}  // namespace avz

using namespace avz;

static_assert(sizeof(DelayStreamHeader) == 16, "the reset kernel zeroes from word 4");

template <int N>
static int launch_delay_stream_t(const DelayStreamArgs* a, hipStream_t st) {
  const int lds = DelayStreamGeo<N>::LDS_BYTES;
  if (!lds_ready<avz_delay_stream_kernel<N>>(lds)) return -3;
  hipLaunchKernelGGL(avz_delay_stream_kernel<N>, dim3(a->streams), dim3(kStreamThreads), lds, st,
                     *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int avz_launch_delay_stream_push(int n_fft, const DelayStreamArgs* a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (a->nb < 1 || a->nb > kDelayStreamMaxBins) return -1;
  if (n_fft == 1024) return launch_delay_stream_t<1024>(a, st);
  if (n_fft == 512) return launch_delay_stream_t<512>(a, st);
  return -4;
}

extern "C" int avz_launch_delay_stream_reset(int n_fft, const DelayStreamArgs* a, void* stream) {
  if (n_fft != 1024 && n_fft != 512) return -4;
  hipLaunchKernelGGL(avz_delay_stream_reset_kernel, dim3(a->streams), dim3(kStreamThreads), 0,
                     (hipStream_t)stream, *a, n_fft);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
