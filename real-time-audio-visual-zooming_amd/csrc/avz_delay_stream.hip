// avz_delay_stream.hip — streaming blind delay-histogram mask (avz_delay_stream_push,
// avz_delay_stream_reset): the three stages of avz_delay_mask run hop by hop, the histogram a
// recursion h_t = forget h_t-1 + d_t and frame t labelled with the peaks of h_t, on the frames
// avz_stream_push forms (the contract is in include/avz.h and DESIGN.md section 19; the fp64
// restatement is avz/delay_mask.py delay_mask_stream_numpy).
//
// Layout: one 256-thread block per stream, resident for the whole call; the block walks the
// call's hops in groups of the eight frames its eight lane groups hold (StreamGeo<N>, as
// avz_stream_kernel). The arithmetic of each stage (pair, deposit, peaks, rotation, cost) is
// avz_delay_common.hpp's, shared with avz_delay_mask.hip; this file holds the streaming layout
// around it. Per group:
//   transform   stream_transform of mic0 + i mic1 into the eight slots;
//   pairs       thread (bin k, frame) turns its band bins into (u, w) in place in the slot (only
//               that thread ever reads Z[k] and Z[N - k]);
//   deposits    all frames at once: thread (frame, segment s, histogram bin i) scans its fixed
//               share of that frame's band pairs in order and adds what falls on bin i (fp64);
//   recursion   frame by frame, the only serial part: h <- forget h + (the segments added in
//   and peaks   order), then delay_peaks on h_t; the frame's list and J go to a table in LDS and
//               to delays_out / n_peaks;
//   transform   again (the pairs overwrote the band's bins);
//   labels      all frames at once: thread (bin k) holds delta_0's rotation once and forms the
//               others per frame from the table, writes its decisions in place and the block
//               stores them through the caller's strides.
// A frame's arithmetic is the same instruction sequence whatever its slot, group or call and
// reads nothing of another stream, and every sum has a fixed order that depends on the frame
// alone: a stream's results do not depend on how its hops are grouped into calls, on its index
// or on the other streams. No atomics, no inter-block traffic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avz_delay_stream.hpp"
#include "avz_frame.hpp"

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
  static constexpr int J_OFF = LIST_OFF + SG::NSLOT * kDelayList * 8;
  static constexpr int LDS_BYTES = J_OFF + ((SG::NSLOT * 4 + 15) & ~15);
  static_assert(NBP >= kDelayMaxBins, "a row holds every histogram size");
  static_assert(H_OFF % 8 == 0, "f64 alignment");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// Scan segments per (frame, histogram bin): a function of the histogram size alone.
__device__ __forceinline__ int delay_stream_segments(int nb) {
  return nb >= kStreamThreads ? 1 : kStreamThreads / nb;
}

template <int N>
__global__ void __launch_bounds__(kStreamThreads, 1) avz_delay_stream_kernel(DelayStreamArgs A) {
  using SG = StreamGeo<N>;
  using DG = DelayStreamGeo<N>;
  constexpr int H = SG::H, F = SG::F, NSLOT = SG::NSLOT, L8 = kDelayList;
  const int s = blockIdx.x;
  if (A.active && A.active[s] == 0) return;
  const int nb = A.p.nb;
  const DelayStreamLayout lay(N, nb);
  unsigned char* st = A.state + (long long)s * A.state_stride;
  DelayStreamHeader* hdr = reinterpret_cast<DelayStreamHeader*>(st);
  if (hdr->nb != nb || hdr->n_fft != N) return;  // not reset for this call's layout
  float* prev = reinterpret_cast<float*>(st + lay.prev_off);  // [2][H]
  double* h_g = reinterpret_cast<double*>(st + lay.hist_off);
  const unsigned long long count0 = hdr->count;

  extern __shared__ __align__(16) unsigned char lds[];
  double* h = reinterpret_cast<double*>(lds + DG::H_OFF);
  double* hs0 = reinterpret_cast<double*>(lds + DG::HS_OFF);
  double* c_h = reinterpret_cast<double*>(lds + DG::CH_OFF);
  double* c_d = reinterpret_cast<double*>(lds + DG::CD_OFF);
  double* seg = reinterpret_cast<double*>(lds + DG::SEG_OFF);
  double* tab = reinterpret_cast<double*>(lds + DG::LIST_OFF);  // [8][8]
  int* Jt = reinterpret_cast<int*>(lds + DG::J_OFF);
  const int tid = threadIdx.x;

  const bool adapt = !A.adapt || A.adapt[s] != 0;
  const double lam = A.forget;
  double theta = A.angle_deg ? A.angle_deg[s] : A.p.plan_angle;
  if (theta != theta) theta = A.p.plan_angle;  // NaN: the plan's
  const double d_t = delay_target(A.p, theta);

  StreamBlock<N> sb;
  sb.stage(lds, A.xwin, tid);
  for (int i = tid; i < nb; i += kStreamThreads) h[i] = h_g[i];
  __syncthreads();
  sb.init(lds);

  const float* x0 = A.mix + (long long)s * A.mix_stride;
  const float* x1 = x0 + A.ch_stride;
  float* M = A.mask + (long long)s * A.m_sb;
  const int nband = A.p.k_hi >= A.p.k_lo ? A.p.k_hi - A.p.k_lo + 1 : 0;
  const int S = delay_stream_segments(nb);
  const int per = S * nb;  // deposit items of one frame: <= 257

  for (int j0 = 0; j0 < A.hops; j0 += NSLOT) {
    const int nf = min(NSLOT, A.hops - j0);
    const bool valid = sb.my_slot < nf;

    stream_transform<N>(sb, x0, x1, prev, prev + H, j0 + sb.my_slot, valid);
    __syncthreads();

    // (u, w) of every band pair, in place: Z_f[k] <- (u, w)
    {
      const float u0 = 0.5f * (float)nb - 0.5f;
      for (int idx = tid; idx < nf * nband; idx += kStreamThreads) {
        const int f = idx / nband, k = A.p.k_lo + idx % nband;
        cf* Z = slot_ptr<N>(lds, f);
        Z[k] = delay_pair(Z[k], Z[(N - k) & (N - 1)], delay_u_scale(N, k, A.p.bin_w), u0, true);
      }
    }
    __syncthreads();

    // owner-computes: item (frame f, segment sg, bin i) scans pairs [p0, p1) of f's band in order
    for (int idx = tid; idx < nf * per; idx += kStreamThreads) {
      const int f = idx / per, r = idx % per;
      const int sg = r / nb, i = r % nb;
      const int p0 = (int)((long long)nband * sg / S), p1 = (int)((long long)nband * (sg + 1) / S);
      const cf* Zb = slot_ptr<N>(lds, f) + A.p.k_lo;
      const float fi = (float)i;
      double acc = 0.0;
      for (int p = p0; p < p1; ++p) acc += delay_deposit(Zb[p], fi);
      seg[idx] = acc;  // [f][sg][i]
    }
    __syncthreads();

    // frame by frame: the recursion, then delay_peaks on h_t
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
      const long long row = (long long)s * A.hops + (j0 + f);
      const int J = delay_peaks<kStreamThreads>(A.p, hs0, DG::NBP, c_h, c_d, d_t, tab + f * L8,
                                                A.delays_out ? A.delays_out + row * L8 : nullptr);
      if (tid == 0) {
        Jt[f] = J;
        if (A.n_peaks) A.n_peaks[row] = J;
      }
      __syncthreads();  // the list is complete; hs, c_h and c_d are free for the next frame
    }

    // the spectra again: the pairs overwrote the band's bins
    stream_transform<N>(sb, x0, x1, prev, prev + H, j0 + sb.my_slot, valid);
    __syncthreads();

    // labels: bin kk = k with the Nyquist bin in place of DC (omega = 0: every cost ties)
    for (int k = tid; k < N / 2; k += kStreamThreads) {
      const bool dc = k == 0;
      const int kk = dc ? N / 2 : k;
      const cf rot0 = delay_rotation(kk, d_t, N);
      for (int f = 0; f < nf; ++f) {
        cf* Z = slot_ptr<N>(lds, f);
        cf y0, y1;
        split_pair(Z[kk], Z[(N - kk) & (N - 1)], y0, y1);
        const float cost0 = delay_cost(rot0, y0, y1);
        const int J = Jt[f];
        bool other = false;
        for (int j = 1; j <= J; ++j) {
          const float cost = delay_cost(delay_rotation(kk, tab[f * L8 + j], N), y0, y1);
          other = other || cost < cost0;
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
  save_last_hop<H>(prev, x0, x1, A.hops, tid);
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
  static_assert(sizeof(DelayStreamHeader) % 4 == 0, "zero_state works in words");
  zero_state(st, sizeof(DelayStreamHeader), A.state_stride);
  if (threadIdx.x == 0) {
    DelayStreamHeader* hdr = reinterpret_cast<DelayStreamHeader*>(st);
    hdr->count = 0ull;
    hdr->nb = A.p.nb;
    hdr->n_fft = n_fft;
  }
}

}  // namespace avz

using namespace avz;

extern "C" int avz_launch_delay_stream_push(int n_fft, const DelayStreamArgs* a, void* stream) {
  if (a->p.nb < 1 || a->p.nb > kDelayMaxBins) return -1;
  return dispatch_n_fft(n_fft, [&](auto n) {
    constexpr int N = decltype(n)::value;
    return launch<avz_delay_stream_kernel<N>>(dim3(a->streams), kStreamThreads,
                                              DelayStreamGeo<N>::LDS_BYTES, (hipStream_t)stream,
                                              *a);
  });
}

extern "C" int avz_launch_delay_stream_reset(int n_fft, const DelayStreamArgs* a, void* stream) {
  if (n_fft != 1024 && n_fft != 512) return -4;
  return launch<avz_delay_stream_reset_kernel>(dim3(a->streams), kStreamThreads, 0,
                                               (hipStream_t)stream, *a, n_fft);
}
