// avz_stream.hip — streaming causal MVDR (avz_stream_push, avz_stream_reset, avz_stream_steer):
// the chain of avz_mvdr_batch run hop by hop, with the masked covariance as a recursion
// c_t = forget c_{t-1} + n_t (|y0|^2, |y1|^2, Re y0 y1*, Im y0 y1*, 1) and the weights solved
// from c_t for every frame (avz/stream.py stream_numpy restates it).
//
// Layout: one 256-thread block per stream, resident for the whole call; the block walks the
// call's hops in groups of the eight frames its eight lane groups hold (KCfg<N>: two 32-lane
// transforms per wave, the STFT kernels' slots). Per group:
//   (IBM) packed reference transforms tgt + i itf -> one noise bit per (bin, frame) in LDS;
//   packed mic transforms mic0 + i mic1 into the slots;
//   per bin (thread k, k + 256, ..): the recursion over the group's frames in order, the fp64
//     solve (mvdr_weights_d), S = w^H y times the post-filter gain, written over Z[k] with its
//     Hermitian mirror over Z[N - k];
//   one inverse transform per lane group (conj FFT conj of the Hermitian spectrum: the real
//     part is irfft N), times sum(w) w[n], stored as N floats in the slot;
//   overlap-add of each frame's first half with its predecessor's second half (the state's
//     tail for the group's first frame), divided by w^2[m] + w^2[m + H], float4 stores.
// A frame's arithmetic is the same instruction sequence whatever its slot, group or call and
// reads nothing of another stream, so a stream's results do not depend on how its hops are
// grouped into calls, on its index or on the other streams. No atomics, no inter-block
// traffic. Four of a call's frames could share two packed inverse transforms, but with one
// block per stream the four waves sit on four SIMDs and a wave's second lane group is free:
// one inverse per lane group has the same latency.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avz_frame.hpp"

namespace avz {

template <int N, int MASK>
__global__ void __launch_bounds__(kStreamThreads, 1) avz_stream_kernel(StreamArgs S, ChainArgs P) {
  using C = KCfg<N>;
  using SG = StreamGeo<N>;
  constexpr int H = SG::H, F = SG::F, NSLOT = SG::NSLOT;
  const int s = blockIdx.x;
  if (S.active && S.active[s] == 0) return;
  extern __shared__ __align__(16) unsigned char lds[];
  float* tail = reinterpret_cast<float*>(lds + SG::TAIL_OFF);
  uint32_t* nbits = reinterpret_cast<uint32_t*>(lds + SG::BITS_OFF);
  const int tid = threadIdx.x;

  const StreamLayout lay(N);
  unsigned char* st = S.state + (long long)s * S.state_stride;
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(st);
  float* prev = reinterpret_cast<float*>(st + lay.prev_off);  // [4][H]
  float* tail_g = reinterpret_cast<float*>(st + lay.tail_off);
  double* cov = reinterpret_cast<double*>(st + lay.cov_off);
  const double* steer = reinterpret_cast<const double*>(st + lay.steer_off);
  const unsigned long long count0 = *cnt;
  const bool adapt = !S.adapt || S.adapt[s] != 0;
  const double lam = S.forget;

  StreamBlock<N> sb;
  sb.stage(lds, P.xwin, tid);
  for (int m = tid; m < H; m += kStreamThreads) tail[m] = tail_g[m];
  __syncthreads();
  sb.init(lds);

  const float* x0 = S.mix + (long long)s * S.mix_stride;
  const float* x1 = x0 + S.ch_stride;
  const float* rt = MASK == MASK_IBM ? S.ref_tgt + (long long)s * S.ref_stride : nullptr;
  const float* ri = MASK == MASK_IBM ? S.ref_int + (long long)s * S.ref_stride : nullptr;
  float* orow = S.out + (long long)s * S.out_stride;

  for (int j0 = 0; j0 < S.hops; j0 += NSLOT) {
    const int nf = min(NSLOT, S.hops - j0);
    const bool valid = sb.my_slot < nf;
    const bool last = j0 + nf == S.hops;

    if constexpr (MASK == MASK_IBM) {
      // reference pair -> noise bits: bit f of nbits[k] = frame j0 + f of bin k is noise
      stream_transform<N>(sb, rt, ri, prev + 2 * H, prev + 3 * H, j0 + sb.my_slot, valid);
      __syncthreads();
      for (int k = tid; k < F; k += kStreamThreads) {
        uint32_t bits = 0;
        for (int f = 0; f < nf; ++f) {
          const cf* Z = slot_ptr<N>(lds, f);
          // noise <=> |S_i| > |S_t| <=> Re(Z[k] Z[N - k]) < 0 (avz_chain_common.hpp ibm_noise)
          const cf z = Z[k], zp = Z[(N - k) & (N - 1)];
          bits |= (fmaf(z.x, zp.x, -(z.y * zp.y)) < 0.0f ? 1u : 0u) << f;
        }
        nbits[k] = bits;
      }
      __syncthreads();  // every slot has been read before its lane group overwrites it
    }

    stream_transform<N>(sb, x0, x1, prev, prev + H, j0 + sb.my_slot, valid);
    __syncthreads();

    // per bin: recursion, solve and apply over the group's frames, in order
    for (int k = tid; k < F; k += kStreamThreads) {
      const int kp = (N - k) & (N - 1);
      double c[5], w[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int i = 0; i < 5; ++i) c[i] = cov[5 * k + i];
      const double d0r = steer[4 * k], d0i = steer[4 * k + 1];
      const double d1r = steer[4 * k + 2], d1i = steer[4 * k + 3];
      const uint32_t bits = MASK == MASK_IBM ? nbits[k] : 0u;
      for (int f = 0; f < nf; ++f) {
        cf* Z = slot_ptr<N>(lds, f);
        const cf z = Z[k], zp = Z[kp];
        cf y0, y1;
        split_pair(z, zp, y0, y1);
        float nw, wgt, M = 1.0f;  // noise weight, covariance weight, target probability
        if constexpr (MASK == MASK_IBM) {
          nw = ((bits >> f) & 1u) ? 1.0f : 0.0f;
          wgt = nw;
        } else if constexpr (MASK == MASK_EXTERNAL) {
          M = S.ext_mask[(long long)s * S.mask_sb + (long long)k * S.mask_sf +
                         (long long)(j0 + f) * S.mask_st];
          nw = 1.0f - M;
          wgt = nw + P.weight_eps;
        } else {
          nw = 1.0f;
          wgt = 1.0f;
        }
        if (adapt) {
          const double ar = y0.x, ai = y0.y, er = y1.x, ei = y1.y, wg = wgt;
          c[0] = fma(wg, ar * ar + ai * ai, lam * c[0]);
          c[1] = fma(wg, er * er + ei * ei, lam * c[1]);
          c[2] = fma(wg, ar * er + ai * ei, lam * c[2]);  // Re y0 conj(y1)
          c[3] = fma(wg, ai * er - ar * ei, lam * c[3]);  // Im y0 conj(y1)
          c[4] = lam * c[4] + (double)nw;
        }
        mvdr_weights_d(c, k, N, P, d0r, d0i, d1r, d1i, w, nullptr);
        cf alpha, beta;
        coef_from_w(w[0], w[1], w[2], w[3], alpha, beta, nullptr);
        float g = 1.0f;
        if (P.postfilter == PF_IBM_TARGET) g = 1.0f - nw;
        else if (P.postfilter == PF_EXT_FLOOR) g = fmaxf(M, P.pf_floor);
        else if (P.postfilter == PF_EXT_MUL) g = M;
        const cf sv = apply_bin(alpha, beta, z, zp, g);
        if (kp == k) {
          Z[k] = {sv.x, 0.0f};  // DC / Nyquist: irfft reads the real part only
        } else {
          Z[k] = sv;
          Z[kp] = c_conj(sv);
        }
        if (S.mask_out)
          S.mask_out[((long long)s * F + k) * S.hops + (j0 + f)] = nw;
      }
#pragma unroll
      for (int i = 0; i < 5; ++i) cov[5 * k + i] = c[i];
      if (last) {
        if (S.cov_out) {
#pragma unroll
          for (int i = 0; i < 5; ++i) S.cov_out[((long long)s * F + k) * 5 + i] = c[i];
        }
        if (S.w_out) {
#pragma unroll
          for (int i = 0; i < 4; ++i) S.w_out[((long long)s * F + k) * 4 + i] = (float)w[i];
        }
      }
    }
    __syncthreads();

    // inverse transform of each frame in its own slot: g = irfft(S) sum(w) w = Re(.) / 2 w
    {
      cf v[C::PPL];
      static_for<0, C::PPL>(
          [&](auto r) { v[r] = c_conj(sb.spec[sb.lm.in0 + C::IN_STRIDE * r]); });
      __builtin_amdgcn_wave_barrier();  // the group's reads precede the transform's stores
      sb.fft.forward(v, sb.spec, sb.twid);
      float* gf = reinterpret_cast<float*>(sb.spec);
      static_for<0, C::PPL>([&](auto k) {
        const int n = sb.lm.out0 + C::OUT_STRIDE * k;
        gf[n] = (0.5f * v[k].x) * sb.win[n];
      });
    }
    __syncthreads();

    // overlap-add: hop j = (g_{j-1}[H:] + g_j[:H]) / (w^2[m] + w^2[m + H]); the stream's
    // first hop is zeros
    for (int idx = tid; idx < nf * (H / 4); idx += kStreamThreads) {
      const int f = idx / (H / 4), m = (idx % (H / 4)) * 4;
      const float* gc = reinterpret_cast<const float*>(slot_ptr<N>(lds, f)) + m;
      const float* gp =
          f == 0 ? tail + m : reinterpret_cast<const float*>(slot_ptr<N>(lds, f - 1)) + H + m;
      const bool first = count0 + (unsigned long long)(j0 + f) == 0ull;
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[i] = first ? 0.0f : (gp[i] + gc[i]) / ola_den<H>(sb.win, m + i);
      *reinterpret_cast<float4*>(orow + (long long)(j0 + f) * H + m) =
          make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
    for (int m = tid; m < H; m += kStreamThreads)
      tail[m] = reinterpret_cast<const float*>(slot_ptr<N>(lds, nf - 1))[H + m];
    __syncthreads();
  }

  // the state after the call's last frame
  const long long qlast = (long long)(S.hops - 1) * H;
  for (int m = tid; m < H; m += kStreamThreads) {
    tail_g[m] = tail[m];
    prev[m] = x0[qlast + m];
    prev[H + m] = x1[qlast + m];
    if constexpr (MASK == MASK_IBM) {
      prev[2 * H + m] = rt[qlast + m];
      prev[3 * H + m] = ri[qlast + m];
    }
  }
  if (tid == 0) *cnt = count0 + (unsigned long long)S.hops;
}

// Zero the selected streams' state and copy the plan's steering table into them.
__global__ void __launch_bounds__(kStreamThreads) avz_stream_reset_kernel(StreamArgs S, int n_fft,
                                                                          const double* steer) {
  const int s = blockIdx.x;
  if (S.select && S.select[s] == 0) return;
  const StreamLayout lay(n_fft);
  unsigned char* st = S.state + (long long)s * S.state_stride;
  zero_state(st, 0, lay.steer_off);
  double* d = reinterpret_cast<double*>(st + lay.steer_off);
  const int n_steer = (n_fft / 2 + 1) * 4;
  for (int i = threadIdx.x; i < n_steer; i += kStreamThreads) d[i] = steer[i];
}

// masked_mvdr.get_steering_vector for the stream's new angle: tau1 = (d/2) cos(theta) / c,
// tau2 = (d/2) cos(theta - pi) / c, d_m = exp(-2 pi i f_k tau_m); cospi / sincospi keep the
// argument reduction exact and free of tables.
__global__ void __launch_bounds__(kStreamThreads) avz_stream_steer_kernel(StreamArgs S, int n_fft,
                                                                          double mic_d,
                                                                          double c_sound,
                                                                          double fs) {
  const int s = blockIdx.x;
  const double ang = S.angle_deg[s];
  if (ang != ang) return;  // NaN: keep
  const StreamLayout lay(n_fft);
  double* d = reinterpret_cast<double*>(S.state + (long long)s * S.state_stride + lay.steer_off);
  const double tau1 = (mic_d / 2) * cospi(ang / 180.0) / c_sound;
  const double tau2 = (mic_d / 2) * cospi(ang / 180.0 - 1.0) / c_sound;
  for (int k = threadIdx.x; k < n_fft / 2 + 1; k += kStreamThreads) {
    const double fk = (double)k * fs / (double)n_fft;
    double sn, cs;
    sincospi(2.0 * fk * tau1, &sn, &cs);
    d[4 * k + 0] = cs;
    d[4 * k + 1] = -sn;
    sincospi(2.0 * fk * tau2, &sn, &cs);
    d[4 * k + 2] = cs;
    d[4 * k + 3] = -sn;
  }
}

}  // namespace avz

using namespace avz;

extern "C" int avz_launch_stream_push(int n_fft, int mask_mode, const StreamArgs* s,
                                      const ChainArgs* p, void* stream) {
  return dispatch_n_fft(n_fft, [&](auto n) {
    constexpr int N = decltype(n)::value, lds = StreamGeo<N>::LDS_BYTES;
    const dim3 grid(s->streams);
    hipStream_t st = (hipStream_t)stream;
    switch (mask_mode) {
      case MASK_IBM:
        return launch<avz_stream_kernel<N, MASK_IBM>>(grid, kStreamThreads, lds, st, *s, *p);
      case MASK_EXTERNAL:
        return launch<avz_stream_kernel<N, MASK_EXTERNAL>>(grid, kStreamThreads, lds, st, *s, *p);
      case MASK_ONES:
        return launch<avz_stream_kernel<N, MASK_ONES>>(grid, kStreamThreads, lds, st, *s, *p);
    }
    return -4;
  });
}

extern "C" int avz_launch_stream_reset(int n_fft, const StreamArgs* s, const double* plan_steer,
                                       void* stream) {
  return launch<avz_stream_reset_kernel>(dim3(s->streams), kStreamThreads, 0, (hipStream_t)stream,
                                         *s, n_fft, plan_steer);
}

extern "C" int avz_launch_stream_steer(int n_fft, const StreamArgs* s, double mic_d,
                                       double c_sound, double fs, void* stream) {
  return launch<avz_stream_steer_kernel>(dim3(s->streams), kStreamThreads, 0, (hipStream_t)stream,
                                         *s, n_fft, mic_d, c_sound, fs);
}
