// avz_chain_synthesis.hpp — the chunk-grid synthesis stage of the chain (avz_chunked_k.hpp):
// synthesis_item and the persistent avz_synthesis_kernel (seams: avz_chain_finalize.hpp).
// Needs: avz_chain_common.hpp.
#pragma once
#include "avz_chain_common.hpp"

namespace avz {
// SPEC: the frames' spectra come from A.spec (avz_istft: scipy.signal.istft of a given
// S[b][k][t]) instead of the forward FFT of the mixture and the apply step.
template <int N, int PF, bool SPEC>
__device__ __forceinline__ void synthesis_item(const ChainArgs& A, unsigned char* lds, int c,
                                               int b, const LaneConst<N>& K) {
  static_assert(!SPEC || PF == PF_NONE, "spectrum input carries its own post-filter");
  using C = KCfg<N>;
  using G = SGeo<N, kSynR<N, PF>>;
  constexpr int NT = G::NT, H = G::H, F = G::F, NSLOT = G::NSLOT, BPT = G::BPT, PPL = C::PPL;
  constexpr int FB = NSLOT;           // frames per step
  constexpr int NPAIR = FB / 2;       // packed inverse FFTs per step
  constexpr int M4 = H / 4;           // float4 groups per half frame
  constexpr int NSG = NT / M4;        // segment groups
  constexpr int SPT = FB / NSG;       // segments per thread per step
  static_assert(SPT * NSG == FB, "OLA mapping");

  float* red = reinterpret_cast<float*>(lds + G::MISC_OFF);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int L = utt_len(A, b);
  if (L < N) return;  // host validates; a bad device length reports NaN (finalize)
  const int T = (L + H - 1) / H + 1;
  const int nch = (T + kChunk - 1) / kChunk;
  if (c >= nch) return;
  const int t0 = c * kChunk;
  const int nstep = (min(kChunk, T - t0) + FB - 1) / FB;

  const typename C::Fft fft = K.fft;
  const LaneMap<N> lm = K.lm;
  const WinCoef<N> wc = K.wc;
  const int my_slot = wave * C::FPW + lm.grp;
  cf* my_spec = slot_ptr<N>(lds, my_slot);
  // SGeo::R > 1: the lane group also transforms frames my_slot + NWAVE FPW q, q < R
  constexpr int RSTRIDE = G::NWAVE * C::FPW;

  const float* mixb = A.mix + (long long)b * A.mix_stride;
  const rsrc_t r_m0 = make_rsrc(mixb, L), r_m1 = make_rsrc(mixb + A.ch_stride, L);
  cf v[PPL];
  cf vq[G::R > 1 ? G::R - 1 : 1][G::R > 1 ? PPL : 1];  // frames q >= 1 of the step
  auto load_frame = [&](cf (&x)[PPL], int frame, int wave_frame) {
    const int s0 = frame * H - N / 2 + lm.in0;
    if (wave_frame >= 1) {  // wave-uniform: no negative sample index
      static_for<0, PPL>([&](auto r) {
        x[r].x = bload_nn(r_m0, s0 + C::IN_STRIDE * r);
        x[r].y = bload_nn(r_m1, s0 + C::IN_STRIDE * r);
      });
    } else {
      static_for<0, PPL>([&](auto r) {
        x[r].x = bload(r_m0, s0 + C::IN_STRIDE * r);
        x[r].y = bload(r_m1, s0 + C::IN_STRIDE * r);
      });
    }
  };
  auto issue_loads = [&](int step) {
    const int fb = t0 + step * FB;
    load_frame(v, fb + my_slot, fb + wave * C::FPW);
    if constexpr (G::R > 1) {
#pragma unroll
      for (int q = 1; q < G::R; ++q)
        load_frame(vq[q - 1], fb + my_slot + q * RSTRIDE, fb + wave * C::FPW + q * RSTRIDE);
    }
  };
  AVZ_STAMP_DECL();
  AVZ_STAMP_INIT();
  if constexpr (!SPEC) issue_loads(0);

  // ---- apply coefficients and post-filter bits of this thread's bins tid + 256 j
  const float4* coef = reinterpret_cast<const float4*>(A.coef) + (long long)b * F;
  const uint32_t* MW = A.mwords + ((long long)b * A.nchunk + c) * F;
  cf alpha[BPT], beta[BPT];
  uint32_t bits[BPT];
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    const float4 cw = SPEC ? make_float4(0.f, 0.f, 0.f, 0.f) : coef[tid + j * NT];
    alpha[j] = cf{cw.x, cw.y};
    beta[j] = cf{cw.z, cw.w};
    bits[j] = (PF == PF_IBM_TARGET) ? MW[tid + j * NT] : 0u;
  }
  const bool nyq_wave = (wave == G::NWAVE - 1);
  cf alpha_n{0, 0}, beta_n{0, 0};  // the Nyquist bin N/2 (outside the pairs)
  uint32_t bits_n = 0u;
  // spectrum input: S[b][k][t] rows (t contiguous); frames past spec_frames read as zero
  const float2* Sb = SPEC ? reinterpret_cast<const float2*>(A.spec) + (long long)b * A.spec_sb
                          : nullptr;
  const int TS = SPEC ? min(T, A.spec_frames) : T;
  const bool svec = SPEC && ((A.spec_sb | A.spec_sf) & 1) == 0 &&
                    ((reinterpret_cast<uintptr_t>(A.spec) & 15) == 0);
  if (nyq_wave && !SPEC) {
    const float4 cw = coef[N / 2];
    alpha_n = cf{cw.x, cw.y};
    beta_n = cf{cw.z, cw.w};
    if (PF == PF_IBM_TARGET) bits_n = MW[N / 2];
  }
  const float* irm = (PF == PF_IRM) ? A.pf_gain + ((long long)b * A.nchunk + c) * kChunk * F
                                    : nullptr;
  const bool mask_vec = (PF == PF_EXT_FLOOR || PF == PF_EXT_MUL) && A.mask_st == 1 &&
                        (A.mask_sf & 3) == 0 && (A.mask_sb & 3) == 0 &&
                        ((reinterpret_cast<uintptr_t>(A.ext_mask) & 15) == 0);
  auto gain = [&](uint32_t bb, int i, int t, int k) -> float {  // i: frame bit in chunk
    if (t >= T) return 0.0f;
    if constexpr (PF == PF_IBM_TARGET) {
      return ((bb >> i) & 1u) ? 0.0f : 1.0f;
    } else if constexpr (PF == PF_IRM) {
      return irm[i * F + k];
    } else if constexpr (PF == PF_EXT_FLOOR || PF == PF_EXT_MUL) {
      const float M =
          A.ext_mask[(long long)b * A.mask_sb + (long long)k * A.mask_sf + (long long)t * A.mask_st];
      return PF == PF_EXT_FLOOR ? fmaxf(M, A.pf_floor) : M;
    } else {
      return 1.0f;
    }
  };

  // OLA role: 4 consecutive samples m0.. of segments sgrp + NSG si
  const int m0 = 4 * (tid % M4);
  const int sgrp = tid / M4;
  float inv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) inv[i] = K.inv[i];
  static_assert(M4 == N / 8, "LaneConst's OLA role");
  float4 carry = make_float4(0.f, 0.f, 0.f, 0.f);  // previous frame's second half (sgrp 0)
  float* outb = A.out + (long long)b * A.out_stride;
  float peak = 0.0f;
  const bool ifft_wave = wave < NPAIR / C::FPW;  // waves holding a packed pair

  lds_barrier();  // the previous item's readers
  AVZ_STAMP(4);
  for (int step = 0; step < nstep; ++step) {
    const int f0 = t0 + step * FB;
    const bool more = step + 1 < nstep;
#ifdef AVZ_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    AVZ_STAMP(5);
#endif
    if constexpr (!SPEC) {
      window_fft<N, true>(v, wc, fft, my_spec, lm);
      if constexpr (G::R > 1) {
#pragma unroll
        for (int q = 1; q < G::R; ++q)
          window_fft<N, true>(vq[q - 1], wc, fft, slot_ptr<N>(lds, my_slot + q * RSTRIDE), lm);
      }
      // N = 512: the next step's loads fly through apply, inverse FFT and OLA (the N = 1024
      // inverse runs in the sample registers, so its loads wait until it is done)
      if (N != 1024 && more) issue_loads(step + 1);
    }
    lds_barrier();
    AVZ_STAMP(6);

    // ---- apply w^H y and the post-filter; pack frames (2p, 2p+1) into slot 2p
    auto apply_phase = [&](auto vec) {
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
      const int kb = tid + j * NT;
      const int kp = (N - kb) & (N - 1);
      // Branch-free: frames past T were transformed from zeros and get gain 0, and the
      // OLA never writes the segments they touch, so every pair is processed.
      cf za[NPAIR], zap[NPAIR], zb[NPAIR], zbp[NPAIR];
#pragma unroll
      for (int p = 0; p < NPAIR; ++p) {
        const cf* Za = slot_ptr<N>(lds, 2 * p);
        const cf* Zb = slot_ptr<N>(lds, 2 * p + 1);
        za[p] = lds_read(Za + kb);
        zap[p] = lds_read(Za + kp);
        zb[p] = lds_read(Zb + kb);
        zbp[p] = lds_read(Zb + kp);
      }
      // External mask with t-contiguous, 16-B aligned rows (the U-Net / TFLite outputs):
      // the bin's FB gains of this step in FB/4 16-B loads instead of FB scattered ones,
      // each loaded for the two pairs that use it (all FB at once held 16 more VGPRs at
      // N = 512 and spilled 44-72 B)
      constexpr bool VEC = decltype(vec)::value;
      const float4* mp = VEC ? reinterpret_cast<const float4*>(
                                   A.ext_mask + (long long)b * A.mask_sb + (long long)kb * A.mask_sf + f0)
                             : nullptr;
      float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int p = 0; p < NPAIR; ++p) {
        const int ta = f0 + 2 * p;
        cf* Za = slot_ptr<N>(lds, 2 * p);
        const int ia = step * FB + 2 * p;
        float ga, gb;
        if constexpr (VEC) {
          if (p % 2 == 0) g4 = mp[p / 2];
          ga = (p % 2 == 0) ? g4.x : g4.z;
          gb = (p % 2 == 0) ? g4.y : g4.w;
          if constexpr (PF == PF_EXT_FLOOR) {
            ga = fmaxf(ga, A.pf_floor);
            gb = fmaxf(gb, A.pf_floor);
          }
        } else {
          ga = gain(bits[j], ia, ta, kb);
          gb = gain(bits[j], ia + 1, ta + 1, kb);
        }
        if constexpr (PF == PF_EXT_FLOOR || PF == PF_EXT_MUL) {
          // A gain from memory: the vector and the scalar instance of this phase must give
          // the same bits whatever the mask's layout, so every rounding is spelled out (left
          // to the compiler's contraction, the two instances differed at N = 1024 in how
          // g s folds into the packing sums).
          const cf ua = apply_sum_fma(alpha[j], beta[j], za[p], zap[p]);
          const cf ub = apply_sum_fma(alpha[j], beta[j], zb[p], zbp[p]);
          const float ax = ga * ua.x, ay = ga * ua.y;  // Sa = ga ua
          Za[kp] = {fmaf(gb, ub.y, ax), fmaf(gb, ub.x, -ay)};  // as below, Sb = gb ub
          Za[kb] = (kb == 0) ? cf{ax, gb * ub.x} : cf{fmaf(-gb, ub.y, ax), fmaf(gb, ub.x, ay)};
        } else {
          const cf sa = apply_bin(alpha[j], beta[j], za[p], zap[p], ga);
          const cf sb = apply_bin(alpha[j], beta[j], zb[p], zbp[p], gb);
          Za[kp] = {sa.x + sb.y, sb.x - sa.y};  // conj(Sa) + i conj(Sb) at N - k
          // Sa + i Sb at k; at DC irfft keeps only the real parts (written last: kp == kb)
          Za[kb] = (kb == 0) ? cf{sa.x, sb.x} : cf{sa.x - sb.y, sa.y + sb.x};
        }
      }
    }
    };
    // spectrum input: the step's frames of the thread's bins straight from S, packed as
    // above (16-B row segments when the rows are aligned and the step is complete)
    auto spec_phase = [&](auto vec) {
#pragma unroll
      for (int j = 0; j < BPT; ++j) {
        const int kb = tid + j * NT;
        const int kp = (N - kb) & (N - 1);
        const float2* row = Sb + (long long)kb * A.spec_sf + f0;
        cf sv[FB];
        if constexpr (decltype(vec)::value) {
#pragma unroll
          for (int q = 0; q < FB / 2; ++q) {
            const float4 x = reinterpret_cast<const float4*>(row)[q];
            sv[2 * q] = cf{x.x, x.y};
            sv[2 * q + 1] = cf{x.z, x.w};
          }
        } else {
#pragma unroll
          for (int i = 0; i < FB; ++i) {
            const float2 x = (f0 + i < TS) ? row[i] : make_float2(0.f, 0.f);
            sv[i] = cf{x.x, x.y};
          }
        }
#pragma unroll
        for (int p = 0; p < NPAIR; ++p) {
          cf* Za = slot_ptr<N>(lds, 2 * p);
          const cf sa = sv[2 * p], sb = sv[2 * p + 1];
          Za[kp] = {sa.x + sb.y, sb.x - sa.y};
          Za[kb] = (kb == 0) ? cf{sa.x, sb.x} : cf{sa.x - sb.y, sa.y + sb.x};
        }
      }
    };
    if constexpr (SPEC) {
      if (svec && f0 + FB <= TS)  // block-uniform
        spec_phase(std::true_type{});
      else
        spec_phase(std::false_type{});
    } else if constexpr (PF == PF_EXT_FLOOR || PF == PF_EXT_MUL) {
      if (mask_vec && f0 + FB <= T)  // wave-uniform
        apply_phase(std::true_type{});
      else
        apply_phase(std::false_type{});
    } else {
      apply_phase(std::false_type{});
    }
    if (SPEC && nyq_wave && lane < NPAIR) {  // Nyquist bin from S: real parts (irfft)
      const int ta = f0 + 2 * lane;
      if (ta < T) {
        const float2* row = Sb + (long long)(N / 2) * A.spec_sf;
        const float xa = ta < TS ? row[ta].x : 0.f, xb = ta + 1 < TS ? row[ta + 1].x : 0.f;
        slot_ptr<N>(lds, 2 * lane)[N / 2] = {xa, xb};
      }
    }
    if (!SPEC && nyq_wave && lane < NPAIR) {  // Nyquist bin: frame pair `lane`
      const int ta = f0 + 2 * lane;
      if (ta < T) {
        const int ia = step * FB + 2 * lane;
        cf* Za = slot_ptr<N>(lds, 2 * lane);
        const cf* Zb = slot_ptr<N>(lds, 2 * lane + 1);
        const float ga = gain(bits_n, ia, ta, N / 2), gb = gain(bits_n, ia + 1, ta + 1, N / 2);
        const cf za = Za[N / 2], zb = Zb[N / 2];
        Za[N / 2] = {apply_bin(alpha_n, beta_n, za, za, ga).x,
                     apply_bin(alpha_n, beta_n, zb, zb, gb).x};
      }
    }
    lds_barrier();
    AVZ_STAMP(7);

    // ---- inverse FFT of the packed pairs -> windowed frame contributions in slot 2p+1:
    // one packed pair per lane group, two transforms per wave on the waves holding pairs.
    // The N = 1024 transform runs in the sample registers v (the round-1 x1 form with four
    // waves and the loads in flight ran 77.5 vs 73.6 us), so the next step's loads are
    // issued after it (issuing them on the pairless waves first, inside the inverse, or
    // after the overlap-add measured 1-3 us slower).
    if (ifft_wave) {
      const int p = wave * C::FPW + lm.grp;
      cf* Zi = slot_ptr<N>(lds, 2 * p);
      auto inverse = [&](cf (&u)[PPL]) {
        static_for<0, PPL>([&](auto r) { u[r] = c_conj(Zi[lm.in0 + C::IN_STRIDE * r]); });
        float* Cp = reinterpret_cast<float*>(slot_ptr<N>(lds, 2 * p + 1));
        auto emit = [&](auto k, cf x) {
          constexpr float ck = W32::c[k], sk = -W32::s[k];  // cos, sin of 2 pi k / 32
          const float w = fmaf(wc.ss, sk, fmaf(-wc.sc, ck, wc.s0));
          const int n = lm.out0 + C::OUT_STRIDE * k;
          Cp[n] = x.x * w;       // frame 2p   (real part of the inverse)
          Cp[N + n] = -x.y * w;  // frame 2p+1 (imaginary part; conjugation trick)
        };
        if constexpr (N == 1024) {
          fft.stage1_ab_st(u, Zi);
          fft.transpose_read(u, Zi);
          fft.stage2_emit(u, emit);
        } else {
          fft.forward_emit(u, Zi, emit);
        }
      };
      if constexpr (N == 1024) {
        inverse(v);
      } else {
        cf u[PPL];
        inverse(u);
      }
    }
    if (N == 1024 && !SPEC && more) issue_loads(step + 1);
    lds_barrier();
    AVZ_STAMP(8);

    // ---- overlap-add: segment j = f0 - 1 + s = frame s-1 (2nd half) + frame s (1st half)
    auto cframe = [&](int f) -> const float* {
      return reinterpret_cast<const float*>(slot_ptr<N>(lds, 2 * (f >> 1) + 1)) + (f & 1) * N;
    };
#pragma unroll
    for (int si = 0; si < SPT; ++si) {
      const int s = sgrp + si * NSG;
      const float4 vb = *reinterpret_cast<const float4*>(cframe(s) + m0);
      if (s == 0 && step == 0) {  // chunk's first frame: finalize adds the previous tail
        *reinterpret_cast<float4*>(A.heads + ((long long)b * A.nchunk + c) * H + m0) = vb;
        continue;
      }
      const int j = f0 - 1 + s;
      if (j <= T - 2) {
        // unconditional read + value select: the conditional read compiled to four
        // bank-conflicting ds_read_b32 (as in the per-utterance kernel)
        const float4 vp = *reinterpret_cast<const float4*>(cframe(s == 0 ? 0 : s - 1) + H + m0);
        const float4 va = (s == 0) ? carry : vp;
        float4 o;
        o.x = (va.x + vb.x) * inv[0];
        o.y = (va.y + vb.y) * inv[1];
        o.z = (va.z + vb.z) * inv[2];
        o.w = (va.w + vb.w) * inv[3];
        *reinterpret_cast<float4*>(outb + (long long)j * H + m0) = o;
        peak = fmaxf(peak, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))));
      }
    }
    if (sgrp == 0) carry = *reinterpret_cast<const float4*>(cframe(FB - 1) + H + m0);
    lds_barrier();
    AVZ_STAMP(9);
  }
  if (sgrp == 0 && nstep * FB == kChunk)  // full chunk: its last frame's tail
    *reinterpret_cast<float4*>(A.tails + ((long long)b * A.nchunk + c) * H + m0) = carry;

  // ---- block max |out| -> utterance running max (non-negative floats order as uints)
  for (int o = 32; o > 0; o >>= 1) peak = fmaxf(peak, __shfl_xor(peak, o, 64));
  if (lane == 0) red[wave] = peak;
  __syncthreads();
  if (tid == 0) {
    float pk = red[0];
#pragma unroll
    for (int w = 1; w < G::NWAVE; ++w) pk = fmaxf(pk, red[w]);
    atomicMax(A.peak_u + b, __float_as_uint(pk));
  }
  AVZ_STAMP(10);
}

// Persistent grid over (chunk, utterance) items, as avz_analysis_kernel.
template <int N, int PF, bool SPEC = false>
__global__ void __launch_bounds__(kCThreads, KCfg<N>::SYN_BLOCKS_PER_CU) avz_synthesis_kernel(ChainArgs A) {
  extern __shared__ __align__(16) unsigned char lds[];
  const int gx = (A.max_frames + kChunk - 1) / kChunk;
  LaneConst<N> K;
  K.init(threadIdx.x);
  const int nsyn = gx * A.batch;
  for (int it = blockIdx.x; it < nsyn; it += gridDim.x)
    synthesis_item<N, PF, SPEC>(A, lds, it % gx, it / gx, K);
}
}  // namespace avz
