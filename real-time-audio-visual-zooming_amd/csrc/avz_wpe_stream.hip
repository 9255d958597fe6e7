// avz_wpe_stream.hip — streaming online WPE (avz_wpe_stream_push, avz_wpe_stream_reset):
// recursive-least-squares WPE run hop by hop with the framing and the caller-owned state of
// avz_stream_push (avz/dereverb.py wpe_stream_numpy restates it).
//
// A push runs in rounds of at most eight frames, three kernels per round, launched back to
// back on the caller's stream; everything they hand each other lives in the state block
// (WpeStreamLayout, avz_internal.h):
//   analysis   one 256-thread block per stream: the packed two-mic transform of the round's
//              frames in the eight lane-group slots (stream_transform), split into the two
//              mics' complex64 spectra and written to the ring, bin-major.
//   rls        one 32-lane group per (stream, bin), eight bins per block: Q (n x n complex
//              fp64, mirrored from the stored triangle) sits in LDS for the round, lane i owns
//              row i of Q and of G; the ring frames the round reads are fetched once into
//              LDS with their powers. Per frame: the regressor y~ goes to LDS; u = Q y~ is a
//              row dot per lane; the prediction G^H y~, y~^H u and the power are butterfly
//              sums over the group's lanes (group_sum: one fixed tree, the same bits in every
//              lane); the rank-one update rewrites the lower triangle and mirrors it. Z goes
//              to the state's round buffer.
//   synthesis  one block per stream: per frame one complex inverse of Z0 + i Z1 (both mics),
//              the window, the overlap-add against the state's tails, float4 stores; it
//              advances the frame count.
// A frame's arithmetic is the same instruction sequence wherever it falls in a round or a call
// and reads nothing of another stream: a stream's results do not depend on how its hops are
// grouped, on its index or on the other streams. No atomics, no inter-block traffic.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avz_frame.hpp"

namespace avz {

constexpr int kWpeGroups = kStreamThreads / 32;  // bins per RLS block
static_assert(kWpeGroups == kWpeStreamRound, "a round is one frame per lane group");

template <int N>
struct WpeStreamGeo {
  using SG = StreamGeo<N>;
  static constexpr int H = N / 2, F = N / 2 + 1;
  // LDS map: StreamGeo<N>'s [FFT slots][twiddles][window N f32], then [tails 2 x H f32]
  static constexpr int TAIL_OFF = SG::TAIL_OFF;
  static constexpr int LDS_BYTES = TAIL_OFF + 2 * H * 4;
  static_assert(KCfg<N>::GROUP_BYTES >= N * 8, "a slot holds both mics' frame");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

struct WpeHeader {
  unsigned long long count;
  int taps, delay, n_fft;
};

// The stream's state block, or null where the stream is inactive or its header does not
// carry this call's taps, delay and transform size (the block's layout depends on them).
__device__ __forceinline__ unsigned char* wpe_stream_block(const WpeStreamArgs& S, int s,
                                                           int n_fft) {
  if (S.active && S.active[s] == 0) return nullptr;
  unsigned char* st = S.state + (long long)s * S.state_stride;
  const WpeHeader* h = reinterpret_cast<const WpeHeader*>(st);
  if (h->taps != S.taps || h->delay != S.delay || h->n_fft != n_fft) return nullptr;
  return st;
}

// Row i and column j <= i of element e of a row-major lower triangle.
__device__ __forceinline__ void tri_index(int e, int& i, int& j) {
  i = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > e) --i;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  j = e - i * (i + 1) / 2;
}

// Orders a lane group's LDS stores before its later loads: the two groups of a wave run in
// lockstep and a wave's LDS operations complete in issue order, so keeping the compiler from
// moving them across this point is all that is needed.
__device__ __forceinline__ void group_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sum of v over a 32-lane group, the same bits in every lane: each butterfly step adds the same
// two numbers in both partners (addition commutes), and the tree never changes.
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 32);
  return v;
}

// ---------------------------------------------------------------------------------- analysis
template <int N>
__global__ void __launch_bounds__(kStreamThreads, 1)
    avz_wpe_stream_analysis_kernel(WpeStreamArgs S, const float* xwin) {
  using WG = WpeStreamGeo<N>;
  constexpr int H = WG::H, F = WG::F;
  const int s = blockIdx.x;
  unsigned char* st = wpe_stream_block(S, s, N);
  if (!st) return;
  extern __shared__ __align__(16) unsigned char lds[];
  const int tid = threadIdx.x;

  const WpeStreamLayout lay(N, S.taps, S.delay);
  const unsigned long long count0 = reinterpret_cast<const WpeHeader*>(st)->count;
  float* prev = reinterpret_cast<float*>(st + lay.prev_off);  // [2][H]
  float4* ring = reinterpret_cast<float4*>(st + lay.ring_off);

  StreamBlock<N> sb;
  sb.stage(lds, xwin, tid);
  __syncthreads();
  sb.init(lds);

  const float* x0 = S.mix + (long long)s * S.mix_stride + (long long)S.j0 * H;
  const float* x1 = x0 + S.ch_stride;
  stream_transform<N>(sb, x0, x1, prev, prev + H, sb.my_slot, sb.my_slot < S.nf);
  __syncthreads();

  for (int k = tid; k < F; k += kStreamThreads) {
    const int kp = (N - k) & (N - 1);
    for (int f = 0; f < S.nf; ++f) {
      const cf* Z = slot_ptr<N>(lds, f);
      cf y0, y1;
      split_pair(Z[k], Z[kp], y0, y1);
      const unsigned long long t = count0 + (unsigned long long)f;
      ring[(long long)k * lay.R + (int)(t % (unsigned)lay.R)] = make_float4(y0.x, y0.y, y1.x, y1.y);
      if (S.Y_out) {
        cf* yo = reinterpret_cast<cf*>(S.Y_out);
        yo[((long long)(2 * s) * F + k) * S.hops + (S.j0 + f)] = y0;
        yo[((long long)(2 * s + 1) * F + k) * S.hops + (S.j0 + f)] = y1;
      }
    }
  }
  // the round's last hop is the next round's previous one (the transforms have read prev)
  save_last_hop<H>(prev, x0, x1, S.nf, tid);
}

// --------------------------------------------------------------------------------------- rls
// LDS of one lane group, in bytes: Q [n][n + 1] c128 column-major (the odd leading dimension
// spreads the mirror's column-wise stores over the banks), y~ [n], u [n], the round's ring
// frames [32] (both mics, c64) and their powers [32] f64.
__host__ __device__ constexpr int wpe_group_lds(int n) {
  return 16 * (n * (n + 1) + 2 * n + 32) + 8 * 32;
}

__global__ void __launch_bounds__(kStreamThreads)
    avz_wpe_stream_rls_kernel(WpeStreamArgs S, int n_fft) {
  const int s = blockIdx.y;
  unsigned char* st = wpe_stream_block(S, s, n_fft);
  if (!st) return;
  const int F = n_fft / 2 + 1;
  const int grp = threadIdx.x >> 5, l = threadIdx.x & 31;
  const int k = blockIdx.x * kWpeGroups + grp;
  if (k >= F) return;  // no block-wide barrier below
  const WpeStreamLayout lay(n_fft, S.taps, S.delay);
  const int n = lay.n, W = lay.W, R = lay.R, tri = lay.tri;

  extern __shared__ __align__(16) unsigned char lds[];
  double2* Qc = reinterpret_cast<double2*>(lds + (long long)grp * wpe_group_lds(n));
  const int ld = n + 1;
  double2* sy = Qc + n * ld;
  double2* su = sy + n;
  float4* rg = reinterpret_cast<float4*>(su + n);
  double* pe = reinterpret_cast<double*>(rg + 32);

  const unsigned long long count0 = reinterpret_cast<const WpeHeader*>(st)->count;
  const float4* ring = reinterpret_cast<const float4*>(st + lay.ring_off) + (long long)k * R;
  float4* zr = reinterpret_cast<float4*>(st + lay.zr_off);
  double2* Gg = reinterpret_cast<double2*>(st + lay.g_off) + (long long)k * n * 2;
  double2* Qg = reinterpret_cast<double2*>(st + lay.q_off) + (long long)k * tri;
  const bool adapt = !S.adapt || S.adapt[s] != 0;
  const bool row = l < n;

  // Q[i][j] at Qc[j ld + i]: lane i walks its row with consecutive lanes on consecutive words
  for (int e = l; e < tri; e += 32) {
    int i, j;
    tri_index(e, i, j);
    const double2 v = Qg[e];
    Qc[j * ld + i] = v;
    if (i != j) Qc[i * ld + j] = make_double2(v.x, -v.y);
  }
  double2 g0 = make_double2(0.0, 0.0), g1 = g0;
  if (row) {
    g0 = Gg[2 * l];
    g1 = Gg[2 * l + 1];
  }
  // every ring frame the round reads, once: frames base .. count0 + nf - 1 with base = count0 -
  // (W - 1), the oldest term of the first frame's power (the regressor reaches back W - 2);
  // W - 1 + nf <= 32 of them, lane l takes frame base + l. A frame before the stream's first
  // is zeros.
  const long long base = (long long)count0 - (W - 1);
  if (l < W - 1 + S.nf) {
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (base + l >= 0) y = ring[(int)((base + l) % R)];
    rg[l] = y;
    const double ar = y.x, ai = y.y, br = y.z, bi = y.w;
    pe[l] = (ar * ar + ai * ai) + (br * br + bi * bi);
  }
  group_sync();

#pragma unroll 1
  for (int f = 0; f < S.nf; ++f) {
    const long long t = (long long)count0 + f;
    const int cur = f + W - 1;  // frame t in rg / pe
    // regressor row l = 2 tau + m: Y[m, t - delay - tau]; the lane's terms of G^H y~
    double2 yt = make_double2(0.0, 0.0);
    double c0r = 0.0, c0i = 0.0, c1r = 0.0, c1i = 0.0;
    if (row) {
      const float4 y = rg[cur - S.delay - (l >> 1)];
      yt = (l & 1) ? make_double2((double)y.z, (double)y.w) : make_double2((double)y.x, (double)y.y);
      sy[l] = yt;
      c0r = g0.x * yt.x + g0.y * yt.y;  // conj(G[l][0]) y~_l
      c0i = g0.x * yt.y - g0.y * yt.x;
      c1r = g1.x * yt.x + g1.y * yt.y;  // conj(G[l][1]) y~_l
      c1i = g1.x * yt.y - g1.y * yt.x;
    }
    const float4 yc = rg[cur];
    group_sync();

    // frames t, t - 1, .. t - W + 1, one per lane
    double p = group_sum(l < W ? pe[cur - l] : 0.0);
    p = p / (double)(2 * W);
    double2 z0 = make_double2((double)yc.x, (double)yc.y);
    double2 z1 = make_double2((double)yc.z, (double)yc.w);
    z0.x -= group_sum(c0r);
    z0.y -= group_sum(c0i);
    z1.x -= group_sum(c1r);
    z1.y -= group_sum(c1i);
    double2 u = make_double2(0.0, 0.0);
    if (row) {
#pragma unroll 4
      for (int j = 0; j < n; ++j) {
        const double2 q = Qc[j * ld + l], y = sy[j];
        u.x = fma(q.x, y.x, fma(-q.y, y.y, u.x));
        u.y = fma(q.x, y.y, fma(q.y, y.x, u.y));
      }
      su[l] = u;
    }
    const double q = group_sum(yt.x * u.x + yt.y * u.y);  // Re(y~^H u)
    group_sync();

    if (adapt) {
      const double pf = p < S.power_floor ? S.power_floor : p;
      const double den = S.forget * pf + q;
      if (row) {
        const double2 kk = make_double2(u.x / den, u.y / den);
        // G[l][m] += k_l conj(z_m)
        g0.x += kk.x * z0.x + kk.y * z0.y;
        g0.y += kk.y * z0.x - kk.x * z0.y;
        g1.x += kk.x * z1.x + kk.y * z1.y;
        g1.y += kk.y * z1.x - kk.x * z1.y;
        // Q[l][j] = (Q[l][j] - k_l conj(u_j)) / forget for j <= l, mirrored into Q[j][l]
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
          if (j <= l) {
            const double2 uj = su[j], q0 = Qc[j * ld + l];
            double2 v;
            v.x = (q0.x - (kk.x * uj.x + kk.y * uj.y)) * S.inv_forget;
            v.y = (q0.y - (kk.y * uj.x - kk.x * uj.y)) * S.inv_forget;
            if (j == l) {
              v.y = 0.0;
              Qc[j * ld + l] = v;
            } else {
              Qc[j * ld + l] = v;
              Qc[l * ld + j] = make_double2(v.x, -v.y);
            }
          }
        }
      }
    }
    if (l == 0) {
      const float4 zf = make_float4((float)z0.x, (float)z0.y, (float)z1.x, (float)z1.y);
      zr[(long long)(t % kWpeStreamRound) * F + k] = zf;
      if (S.Z_out) {
        cf* zo = reinterpret_cast<cf*>(S.Z_out);
        zo[((long long)(2 * s) * F + k) * S.hops + (S.j0 + f)] = cf{zf.x, zf.y};
        zo[((long long)(2 * s + 1) * F + k) * S.hops + (S.j0 + f)] = cf{zf.z, zf.w};
      }
    }
    group_sync();
  }

  for (int e = l; e < tri; e += 32) {
    int i, j;
    tri_index(e, i, j);
    Qg[e] = Qc[j * ld + i];
  }
  if (row) {
    Gg[2 * l] = g0;
    Gg[2 * l + 1] = g1;
    if (S.G_out && S.j0 + S.nf == S.hops) {
      double2* go = reinterpret_cast<double2*>(S.G_out) + ((long long)s * F + k) * n * 2;
      go[2 * l] = g0;
      go[2 * l + 1] = g1;
    }
  }
}

// --------------------------------------------------------------------------------- synthesis
template <int N>
__global__ void __launch_bounds__(kStreamThreads, 1)
    avz_wpe_stream_synthesis_kernel(WpeStreamArgs S, const float* xwin) {
  using C = KCfg<N>;
  using WG = WpeStreamGeo<N>;
  constexpr int H = WG::H, F = WG::F;
  const int s = blockIdx.x;
  unsigned char* st = wpe_stream_block(S, s, N);
  if (!st) return;
  extern __shared__ __align__(16) unsigned char lds[];
  float* tail = reinterpret_cast<float*>(lds + WG::TAIL_OFF);  // [2][H]
  const int tid = threadIdx.x;

  const WpeStreamLayout lay(N, S.taps, S.delay);
  WpeHeader* hdr = reinterpret_cast<WpeHeader*>(st);
  const unsigned long long count0 = hdr->count;
  float* tail_g = reinterpret_cast<float*>(st + lay.tail_off);
  const float4* zr = reinterpret_cast<const float4*>(st + lay.zr_off);

  StreamBlock<N> sb;
  sb.stage(lds, xwin, tid);
  for (int m = tid; m < 2 * H; m += kStreamThreads) tail[m] = tail_g[m];
  __syncthreads();
  sb.init(lds);

  // P = Z0 + i Z1 extended Hermitian-wise per mic: ifft(P) = g0 + i g1 with both real. The
  // inverse is conj FFT conj: FFT(conj P)[n] = N (g0[n] - i g1[n]); times sum(w) w[n] / N.
  {
    const bool valid = sb.my_slot < S.nf;
    const unsigned long long t = count0 + (unsigned long long)sb.my_slot;
    const float4* zt = zr + (long long)(t % kWpeStreamRound) * F;
    cf v[C::PPL];
    static_for<0, C::PPL>([&](auto r) {
      const int n = sb.lm.in0 + C::IN_STRIDE * r;
      const int k = n <= H ? n : N - n;
      float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid) z = zt[k];
      if (k == 0 || k == H) z.y = z.w = 0.0f;  // irfft reads the real part only
      const cf P = n <= H ? cf{z.x - z.w, z.y + z.z} : cf{z.x + z.w, z.z - z.y};
      v[r] = c_conj(P);
    });
    __builtin_amdgcn_wave_barrier();
    sb.fft.forward(v, sb.spec, sb.twid);
    static_for<0, C::PPL>([&](auto q) {
      const int n = sb.lm.out0 + C::OUT_STRIDE * q;
      sb.spec[n] = cf{(0.5f * v[q].x) * sb.win[n], (-0.5f * v[q].y) * sb.win[n]};
    });
  }
  __syncthreads();

  // overlap-add per mic: hop t = (g_{t-1}[H:] + g_t[:H]) / (w^2[j] + w^2[j + H]); the
  // stream's first hop is zeros
  for (int idx = tid; idx < S.nf * 2 * (H / 4); idx += kStreamThreads) {
    const int f = idx / (2 * (H / 4)), rem = idx % (2 * (H / 4));
    const int m = rem / (H / 4), q = (rem % (H / 4)) * 4;
    const cf* gc = slot_ptr<N>(lds, f) + q;
    const bool first = count0 + (unsigned long long)f == 0ull;
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float cur = m ? gc[i].y : gc[i].x;
      float pre;
      if (f == 0) {
        pre = tail[m * H + q + i];
      } else {
        const cf g = slot_ptr<N>(lds, f - 1)[H + q + i];
        pre = m ? g.y : g.x;
      }
      o[i] = first ? 0.0f : (pre + cur) / ola_den<H>(sb.win, q + i);
    }
    float* orow = S.out + (long long)s * S.out_stride + (long long)m * S.out_ch_stride;
    *reinterpret_cast<float4*>(orow + (long long)(S.j0 + f) * H + q) =
        make_float4(o[0], o[1], o[2], o[3]);
  }
  const cf* glast = slot_ptr<N>(lds, S.nf - 1) + H;
  for (int j = tid; j < H; j += kStreamThreads) {
    tail_g[j] = glast[j].x;
    tail_g[H + j] = glast[j].y;
  }
  if (tid == 0) hdr->count = count0 + (unsigned long long)S.nf;
}

// Start the selected streams: zero history and filter, Q = q_init I, the header.
__global__ void __launch_bounds__(kStreamThreads)
    avz_wpe_stream_reset_kernel(WpeStreamArgs S, int n_fft) {
  const int s = blockIdx.x;
  if (S.select && S.select[s] == 0) return;
  const WpeStreamLayout lay(n_fft, S.taps, S.delay);
  unsigned char* st = S.state + (long long)s * S.state_stride;
  zero_state(st, 0, lay.q_off);
  double2* Q = reinterpret_cast<double2*>(st + lay.q_off);
  const long long n_q = (long long)(n_fft / 2 + 1) * lay.tri;
  for (long long e = threadIdx.x; e < n_q; e += kStreamThreads) {
    int i, j;
    tri_index((int)(e % lay.tri), i, j);
    Q[e] = make_double2(i == j ? S.q_init : 0.0, 0.0);
  }
  __syncthreads();  // the header's words were zeroed above by other threads
  if (threadIdx.x == 0) {
    WpeHeader* h = reinterpret_cast<WpeHeader*>(st);
    h->count = 0ull;
    h->taps = S.taps;
    h->delay = S.delay;
    h->n_fft = n_fft;
  }
}

}  // namespace avz

using namespace avz;

template <int N>
static int launch_wpe_stream_n(const WpeStreamArgs* a, const float* xwin, hipStream_t st) {
  const int lds = WpeStreamGeo<N>::LDS_BYTES;
  const int n = 2 * a->taps;
  const int rls_lds = kWpeGroups * wpe_group_lds(n);
  if (!lds_ready<avz_wpe_stream_analysis_kernel<N>>(lds) ||
      !lds_ready<avz_wpe_stream_synthesis_kernel<N>>(lds) ||
      !lds_ready<avz_wpe_stream_rls_kernel>(kWpeGroups * wpe_group_lds(32)))
    return -3;
  const int F = N / 2 + 1;
  WpeStreamArgs r = *a;
  for (int j0 = 0; j0 < a->hops; j0 += kWpeStreamRound) {
    r.j0 = j0;
    r.nf = a->hops - j0 < kWpeStreamRound ? a->hops - j0 : kWpeStreamRound;
    hipLaunchKernelGGL(avz_wpe_stream_analysis_kernel<N>, dim3(a->streams), dim3(kStreamThreads),
                       lds, st, r, xwin);
    hipLaunchKernelGGL(avz_wpe_stream_rls_kernel,
                       dim3((F + kWpeGroups - 1) / kWpeGroups, a->streams), dim3(kStreamThreads),
                       rls_lds, st, r, N);
    hipLaunchKernelGGL(avz_wpe_stream_synthesis_kernel<N>, dim3(a->streams),
                       dim3(kStreamThreads), lds, st, r, xwin);
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int avz_launch_wpe_stream_push(int n_fft, const WpeStreamArgs* a, const float* xwin,
                                          void* stream) {
  static_assert(kWpeGroups * wpe_group_lds(32) <= 160 * 1024, "LDS budget at n = 32");
  return dispatch_n_fft(n_fft, [&](auto n) {
    return launch_wpe_stream_n<decltype(n)::value>(a, xwin, (hipStream_t)stream);
  });
}

extern "C" int avz_launch_wpe_stream_reset(int n_fft, const WpeStreamArgs* a, void* stream) {
  return launch<avz_wpe_stream_reset_kernel>(dim3(a->streams), kStreamThreads, 0,
                                             (hipStream_t)stream, *a, n_fft);
}
