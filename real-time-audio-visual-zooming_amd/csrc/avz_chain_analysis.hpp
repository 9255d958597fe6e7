// avz_chain_analysis.hpp — the analysis stage of the chain (avz_chunked_k.hpp): one (chunk,
// utterance) item or step-range piece of it (analysis_item), the block's sequence of items
// (analysis_items) and the persistent avz_analysis_kernel, which ends in ibm_exact_units.
// Needs: avz_chain_common.hpp, avz_chain_exact.hpp.
#pragma once
#include "avz_chain_common.hpp"
#include "avz_chain_exact.hpp"

namespace avz {
// piece p of P (P = 1: the whole item) runs the chunk's steps [p SA / P, (p + 1) SA / P), SA =
// steps per chunk; slot >= 0: its partials go to tail slot `slot` of tpart and its IBM bits
// into the chunk's mask words atomically (the other pieces own the word's other bits).
// seq: the block's item count (parity of the IBM pending-frame word, see pendw).
template <int N, int MASK, bool IRM, class TW>
__device__ __forceinline__ void analysis_item(const ChainArgs& A, unsigned char* lds, int c,
                                              int b, int p, int P, int slot, const TW& tw_reg,
                                              const LaneConst<N>& K, int seq) {
  using C = KCfg<N>;
  using G = CGeo<N>;
  constexpr int NT = G::NT, H = G::H, F = G::F, NSLOT = G::NSLOT, BPT = G::BPT, PPL = C::PPL;
  constexpr int FB = (MASK == MASK_IBM) ? NSLOT / 2 : NSLOT;  // frames per step
  static_assert(kChunk % FB == 0, "steps tile the chunk");
  // IBM without the IRM gains: the reference waves publish per-bin noise bits
  // (window_fft_reg_ibm_bits) instead of the whole reference spectrum
  constexpr bool REFBITS = N == 1024 && MASK == MASK_IBM && !IRM && !std::is_same<TW, NoTw>::value;
  // shared-half frame-pair loads (pair_loads); needs the twiddle signs of the register path
  // (not IPD: its decisions are pinned bit-exact to the reference's, and the rotated
  // transform's rounding moved one of 1.3e5 on the ipd_test golden)
  constexpr bool SHARE = N == 1024 && MASK != MASK_IPD && !std::is_same<TW, NoTw>::value;
  // IBM without the reference-bit hand-off: the reference waves publish each frame's
  // certificate scale delta (MISC_OFF + 16: four floats) and the bin phase defers the
  // uncertified (bin, frame) decisions one by one (dfr)
  constexpr bool DLT = MASK == MASK_IBM && !REFBITS;

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int L = utt_len(A, b);
  const int T = (L + H - 1) / H + 1;
  const int nch = (T + kChunk - 1) / kChunk;
  // L < N: host validates; finalize reports NaN for a bad device length. A skipped unit writes
  // no exact-path record (ibm_exact_units skips it the same way).
  if (L < N || c >= nch) return;
  if (c == 0 && p == 0 && tid == 0) {
    A.peak_u[b] = 0u;
    if (A.peak && A.normalize != NORM_PEAK) A.peak[b] = 0.0f;  // finalize's atomicMax target
  }
  const int t0 = c * kChunk;
  const int nframes = min(kChunk, T - t0);
  constexpr int SA = kChunk / FB;  // steps of a full chunk
  const int s_lo = p * SA / P;      // this piece's steps [s_lo, nstep)
  const int nstep = min((nframes + FB - 1) / FB, (p + 1) * SA / P);
  // IBM: frames (bit = chunk frame) with decisions deferred to the exact path
  // (ibm_exact_units), OR-ed in LDS by the deciding waves before a step barrier, read after
  // the item's last one. Two triples of words used by alternate items: the next item clears
  // its own before its first barrier, which no thread passes before it has read this item's.
  uint32_t* const pendw = reinterpret_cast<uint32_t*>(lds + G::MISC_OFF + 32 + 12 * (seq & 1));
  if (MASK == MASK_IBM && tid == 0) {
    int z = 0;
    opaque_i(z);  // formed here (a zero pair held across the items spilled)
    pendw[0] = (uint32_t)z;  // frames with a deferred decision
    pendw[1] = (uint32_t)z;  // frames with uncertain bins in xunc (reference-bit path)
    pendw[2] = (uint32_t)z;  // of those, frames with kSparseMax or more (round frames)
  }

  const typename C::Fft fft = K.fft;
  // the lane map formed per item from an opaque lane (held across the items from the kernel
  // start, three of its offsets spilled)
  LaneMap<N> lm;
  {
    int ln = threadIdx.x & 63;
    opaque_i(ln);
    lm.init(ln);
  }
  const float cert_raw = A.ibm_cert * (2.0f / N);  // REFBITS: delta per unit raw norm (2 a0)
  const WinCoef<N> wc = K.wc;  // SHARE: the rotated frames' (group 1) already swapped
  const int my_slot = wave * C::FPW + lm.grp;
  cf* my_spec = slot_ptr<N>(lds, my_slot);
  // IBM: waves 0-1 transform the mic pair, waves 2-3 the reference pair (wave-uniform)
  const bool ref = (MASK == MASK_IBM) && (wave * C::FPW >= FB);
  const int my_frame = ref ? my_slot - FB : my_slot;
  const int wave_frame0 = ref ? wave * C::FPW - FB : wave * C::FPW;

  const float* mixb = A.mix + (long long)b * A.mix_stride;
  rsrc_t r_re = make_rsrc(mixb, L), r_im = make_rsrc(mixb + A.ch_stride, L);
  if constexpr (MASK == MASK_IBM) {
    if (ref) {
      r_re = make_rsrc(A.ref_tgt + (long long)b * A.ref_stride, L);
      r_im = make_rsrc(A.ref_int + (long long)b * A.ref_stride, L);
    }
  }
  cf v[PPL];
  auto issue_loads = [&](int step) {
    if constexpr (SHARE) {
      const int sp = (t0 + step * FB + wave_frame0) * H - N / 2 + lm.in0;
      if (t0 + step * FB + wave_frame0 >= 1)
        pair_loads<true>(v, r_re, r_im, sp, lm.grp);
      else
        pair_loads<false>(v, r_re, r_im, sp, lm.grp);
      return;
    }
    const int s0 = (t0 + step * FB + my_frame) * H - N / 2 + lm.in0;
    if (t0 + step * FB + wave_frame0 >= 1) {  // wave-uniform: no negative sample index
      static_for<0, PPL>([&](auto r) {
        v[r].x = bload_nn(r_re, s0 + C::IN_STRIDE * r);
        v[r].y = bload_nn(r_im, s0 + C::IN_STRIDE * r);
      });
    } else {
      static_for<0, PPL>([&](auto r) {
        v[r].x = bload(r_re, s0 + C::IN_STRIDE * r);
        v[r].y = bload(r_im, s0 + C::IN_STRIDE * r);
      });
    }
  };

  // IL_LOADS (register-twiddle path): the next step's loads are issued from inside the
  // FFT's last stage, register k right after its spectrum output is stored, so their issue
  // overlaps the butterflies; a chunk's last step loads from an empty descriptor (reads 0,
  // no memory traffic). Frames of a next step are >= FB >= 1: no negative sample index.
  constexpr bool IL_LOADS = N == 1024 && !std::is_same<TW, NoTw>::value;
  const rsrc_t r_none = make_rsrc(nullptr, 0);
  rsrc_t rn_re = r_none, rn_im = r_none;
  int sp_next = 0;
  auto load_reg = [&](auto kc) {
    constexpr int k = decltype(kc)::value;
    if constexpr (SHARE) {
      if constexpr (k < 16) {
        const int e = sp_next + 1024 * lm.grp + 32 * k;
        v[k].x = bload_nn(rn_re, e);
        v[k].y = bload_nn(rn_im, e);
      } else if constexpr ((k - 16) % 2 == 0) {
        const int e = sp_next + 512 + 32 * (k - 16) + 32 * lm.grp;
        v[k].x = bload_nn(rn_re, e);
        v[k].y = bload_nn(rn_im, e);
      }
    } else {
      v[k].x = bload_nn(rn_re, sp_next + C::IN_STRIDE * k);
      v[k].y = bload_nn(rn_im, sp_next + C::IN_STRIDE * k);
    }
  };

  Acc32 acc[BPT];
  uint32_t bits[BPT];
  uint32_t dfr[BPT];     // DLT: (bin, frame) decisions deferred to the exact path
  int ipd_clear_n[BPT];  // IPD: frames the cross-product test weighted 1
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    acc[j].zero();
    bits[j] = 0u;
    dfr[j] = 0u;
    ipd_clear_n[j] = 0;
  }
  // IRM post-filter gains of this chunk (PF_IRM plans only)
  static_assert(!IRM || MASK == MASK_IBM, "IRM needs the references");
  float* const gain = IRM ? A.pf_gain + ((long long)b * A.nchunk + c) * kChunk * F : nullptr;
  // Nyquist bin N/2: frame `lane` of each step on the last wave's lanes.
  const bool nyq_wave = (wave == G::NWAVE - 1);
  Acc32 an, adc;  // Nyquist; DC (IPD: weighed on the Nyquist wave, not by lane 0)
  an.zero();
  adc.zero();
  uint32_t nyq_bits = 0u, nyq_dfr = 0u;
  // IPD: covariance weight of the main bin loop, 0 on the DC lane (bin tid + 256 j)
  float wone[BPT];
#pragma unroll
  for (int j = 0; j < BPT; ++j) wone[j] = (MASK == MASK_IPD && j == 0 && tid == 0) ? 0.0f : 1.0f;

  AVZ_STAMP_DECL();
  issue_loads(s_lo);
  lds_barrier();  // twiddle table
  AVZ_STAMP_INIT();
  for (int step = s_lo; step < nstep; ++step) {
    const int f0 = t0 + step * FB;
    const bool live = f0 + wave_frame0 < T;  // wave-uniform: any of its frames exist
#ifdef AVZ_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    AVZ_STAMP(0);
#endif
    if (live) {
      if constexpr (SHARE) pair_finish(v);
      // reference-bit path: the two frames' energies (raw samples; the window's maximum 2 a0
      // scales the bound, cert_raw) as wave-uniform values, so nothing extra stays in VGPRs
      // through the FFT (from the windowed input or the spectrum the kernel spilled 5-125)
      float eg0 = 0.0f, eg1 = eg0;
      if constexpr (REFBITS) {
        if (ref) {
          const float eg = group32_sum(frame_energy(v));
          // (kept as bits: the level rule's compare and selects stay scalar)
          int e0 = __builtin_amdgcn_readlane(__float_as_int(eg), 0);
          int e1 = __builtin_amdgcn_readlane(__float_as_int(eg), 32);
          const bool o0 = (uint32_t)e0 - A.ibm_en_lo > A.ibm_en_span;  // ibm_level_out
          const bool o1 = (uint32_t)e1 - A.ibm_en_lo > A.ibm_en_span;
          if ((o0 || o1) && A.ibm_cert > 0.0f) {  // rare (wave-uniform): all-zero frames pass
            uint32_t nz = 0u;
            static_for<0, 32>([&](auto r) { nz |= __float_as_uint(v[r].x) | __float_as_uint(v[r].y); });
            const unsigned long long any = __ballot((nz << 1) != 0u);  // -0 is zero
            const bool f0 = o0 && (uint32_t)any != 0u, f1 = o1 && (any >> 32) != 0ull;
            if (f0 || f1) {
              // deferred whole, through the certificate itself: a zero frame under delta = inf
              // fails the test in every bin, the Nyquist bin included, whatever its samples
              // would have overflowed or underflowed to (the exact path reads them from memory)
              const bool mine = lm.grp ? f1 : f0;
              static_for<0, 32>([&](auto r) {
                v[r].x = mine ? 0.0f : v[r].x;
                v[r].y = mine ? 0.0f : v[r].y;
              });
              e0 = f0 ? 0x7f800000 : e0;  // inf
              e1 = f1 ? 0x7f800000 : e1;
            }
          }
          eg0 = __int_as_float(e0);
          eg1 = __int_as_float(e1);
        }
      }
      if constexpr (MASK == MASK_IPD) {
        // Bitwise-identical channel samples give bitwise-identical pocketfft spectra in the
        // reference, hence equal angles (weight 0.01) in every bin of the frame; the packed
        // FFT's split does not reproduce that equality, so the frame is flagged here.
        bool same = true;
        static_for<0, PPL>([&](auto r) {
          same &= __float_as_uint(v[r].x) == __float_as_uint(v[r].y);
        });
        const unsigned long long nb = __ballot(!same);
        const bool ident = (C::FPW == 1) ? nb == 0ull : ((nb >> (32 * lm.grp)) & 0xffffffffull) == 0ull;
        if ((lane & (64 / C::FPW - 1)) == 0) lds[G::MISC_OFF + my_slot] = ident ? 1 : 0;
      }
      if constexpr (IL_LOADS) {
        const bool more = step + 1 < nstep;
        rn_re = more ? r_re : r_none;
        rn_im = more ? r_im : r_none;
        sp_next = (t0 + (step + 1) * FB + (SHARE ? wave_frame0 : my_frame)) * H - N / 2 + lm.in0;
      }
      float en = 0.0f;
      if constexpr (!IL_LOADS) {
        window_fft<N>(v, wc, fft, my_spec, lm, NoAfter{}, (DLT && ref) ? &en : nullptr);
      } else if constexpr (REFBITS) {
        // block-uniform: a chunk's last step issues no loads (analysis 79.7 -> 77.0-78.3 us,
        // profiles/r04/ab_last_step_loads.txt; the other masks' kernels keep the
        // empty-descriptor loads: a second copy of their FFT spills)
        uint32_t um = 0u;
        if (step + 1 < nstep) {
          if (ref)
            um = window_fft_reg_ibm_bits(v, wc, fft, my_spec, tw_reg, lm, eg0, eg1, cert_raw, en,
                                         load_reg);
          else
            window_fft_reg(v, wc, fft, my_spec, tw_reg, lm, load_reg);
        } else {
          if (ref)
            um = window_fft_reg_ibm_bits(v, wc, fft, my_spec, tw_reg, lm, eg0, eg1, cert_raw, en);
          else
            window_fft_reg(v, wc, fft, my_spec, tw_reg, lm);
        }
        const unsigned long long ua = __ballot(um != 0u);
        if (ua != 0ull) {  // rare (wave-uniform): uncertain bins, the exact path's (xunc)
          if ((ua >> (32 * lm.grp)) & 0xffffffffull) {
            KArgs& Ak = kernarg_chain_args();
            const int gxi = (Ak.max_frames + kChunk - 1) / kChunk;
            const int unit = slot < 0 ? b * gxi + c : gxi * Ak.batch + slot;
            Ak.xunc[((long long)unit * kChunk + step * FB + my_frame) * 32 + (lane & 31)] = um;
            int nu = __popc(um);  // the frame's uncertain bins (its lane group's 32 words)
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) nu += __shfl_xor(nu, o, 64);
            if ((lane & 31) == 0) {  // a frame with a deferral, one with its xunc words written
              atomicOr(pendw, 1u << (step * FB + my_frame));
              atomicOr(pendw + 1, 1u << (step * FB + my_frame));
              if (nu >= kSparseMax) atomicOr(pendw + 2, 1u << (step * FB + my_frame));
            }
          }
        }
      } else {
        window_fft_reg(v, wc, fft, my_spec, tw_reg, lm, load_reg, (DLT && ref) ? &en : nullptr);
      }
      if constexpr (DLT) {
        static_assert(C::FPW == 2, "lane groups of 32");
        if (ref) {  // the level rule on the windowed energy
          const bool o = ibm_level_out(en, A.ibm_en_lo, A.ibm_en_span);
          if (__ballot(o) != 0ull && A.ibm_cert > 0.0f) {  // rare (wave-uniform)
            // the frame's samples once more (v holds its spectrum, or the next step's loads):
            // an all-zero frame passes
            const int sf = (t0 + step * FB + my_frame) * H - N / 2 + (lane & 31);
            uint32_t nz = 0u;
#pragma unroll 1
            for (int r = 0; r < N / 32; r += 4) {
#pragma unroll
              for (int q = 0; q < 4; ++q)
                nz |= __float_as_uint(bload(r_re, sf + 32 * (r + q))) |
                      __float_as_uint(bload(r_im, sf + 32 * (r + q)));
            }
            const unsigned long long any = __ballot((nz << 1) != 0u);  // -0 is zero
            if (o && ((any >> (32 * lm.grp)) & 0xffffffffull) != 0ull) en = __builtin_nanf("");
          }
        }
      }
      // IBM: the reference waves publish each frame's certificate scale delta (the bin phase's
      // per-bin deferrals, the Nyquist bin's); the reference-bit path returns delta itself
      if (MASK == MASK_IBM && ref && (lane & 31) == 0)
        reinterpret_cast<float*>(lds + G::MISC_OFF + 16)[my_frame] = REFBITS ? en : A.ibm_cert * sqrtf(en);
    }
    AVZ_STAMP(3);
    if (!IL_LOADS && step + 1 < nstep) issue_loads(step + 1);
    AVZ_STAMP(11);
    lds_barrier();
    AVZ_STAMP(1);
    const int nvalid = min(FB, T - f0);
    // Thread-per-bin over the step's frames. A full step runs unguarded so all of its
    // LDS reads can issue back to back; only a chunk's last step may be partial.
    uint32_t ipd_fix[BPT];
#pragma unroll
    for (int j = 0; j < BPT; ++j) ipd_fix[j] = 0u;
    // IPD: frames whose two channels are bitwise identical (bit 8 i: slot i)
    const unsigned long long ident_w =
        (MASK == MASK_IPD) ? *reinterpret_cast<const unsigned long long*>(lds + G::MISC_OFF) : 0ull;
    const bool mask_vec = MASK == MASK_EXTERNAL && A.mask_st == 1 && (A.mask_sf & 3) == 0 &&
                          (A.mask_sb & 3) == 0 &&
                          ((reinterpret_cast<uintptr_t>(A.ext_mask) & 15) == 0) && (f0 & 3) == 0;
    float dlt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (DLT) {  // the step's frames' certificate scales
      const float4 q = *reinterpret_cast<const float4*>(lds + G::MISC_OFF + 16);
      dlt[0] = q.x;
      dlt[1] = q.y;
      dlt[2] = q.z;
      dlt[3] = q.w;
    }
    auto bin_phase = [&](auto full, auto vec) {
      // frames whose LDS reads are batched together
      constexpr int G = FB < 4 ? FB : 4;
#pragma unroll
      for (int j = 0; j < BPT; ++j) {
        const int kb = tid + j * NT;
        const int kp = (N - kb) & (N - 1);
#pragma unroll
        for (int g0 = 0; g0 < FB; g0 += G) {
          // External mask with t-contiguous, 16-B aligned rows: the bin's G mask values
          // of a full step in one 16-B load (as the synthesis post-filter).
          float mv[MASK == MASK_EXTERNAL ? 4 : 1];
          if constexpr (MASK == MASK_EXTERNAL && G == 4 && decltype(vec)::value) {
            const float4 m4 = *reinterpret_cast<const float4*>(
                A.ext_mask + (long long)b * A.mask_sb + (long long)kb * A.mask_sf + f0 + g0);
            mv[0] = m4.x;
            mv[1] = m4.y;
            mv[2] = m4.z;
            mv[3] = m4.w;
          }
          cf zm[G], zmp[G], zr[G], zrp[G];
          uint32_t zw[G];  // REFBITS: the frame's noise word of bin column kb & 31
#pragma unroll
          for (int i = 0; i < G; ++i) {
            if (decltype(full)::value || g0 + i < nvalid) {
              const cf* Zm = slot_ptr<N>(lds, g0 + i);
              zm[i] = Zm[kb];
              zmp[i] = Zm[kp];
              if constexpr (REFBITS) {
                zw[i] = reinterpret_cast<const uint32_t*>(slot_ptr<N>(lds, FB + g0 + i))[kb & 31];
              } else if constexpr (MASK == MASK_IBM) {
                const cf* Zr = slot_ptr<N>(lds, FB + g0 + i);
                zr[i] = Zr[kb];
                zrp[i] = Zr[kp];
              }
            }
          }
#pragma unroll
          for (int i = 0; i < G; ++i) {
            if (decltype(full)::value || g0 + i < nvalid) {
              cf x0, x1;
              split_pair2(zm[i], zmp[i], x0, x1);  // 2 y0, 2 y1
              if constexpr (MASK == MASK_IPD) {
                // the exact angle test of near-colinear bins runs after the loop;
                // ipd_clear on the covariance products themselves: |x0|^2 |x1|^2 and
                // Im x0 conj(x1) are the test's norm and cross product. Every frame's
                // products go in at weight 1 (wone: 0 on the DC lane, weighed by the Nyquist
                // wave); the frames the test leaves open get w - 1 after the loop.
                const float p0 = x0.x * x0.x + x0.y * x0.y;
                const float p1 = x1.x * x1.x + x1.y * x1.y;
                const float re = x0.x * x1.x + x0.y * x1.y;
                const float im = x0.y * x1.x - x0.x * x1.y;
                const bool clear = im * im > 1e-10f * (p0 * p1) &&
                                   !((ident_w >> (8 * (g0 + i))) & 1ull);
                ipd_fix[j] |= (clear ? 0u : 1u) << (g0 + i);
                acc[j].c00 = fmaf(wone[j], p0, acc[j].c00);
                acc[j].c11 = fmaf(wone[j], p1, acc[j].c11);
                acc[j].c01r = fmaf(wone[j], re, acc[j].c01r);
                acc[j].c01i = fmaf(wone[j], im, acc[j].c01i);
                continue;
              }
              if constexpr (MASK == MASK_IBM) {
                bool noise;
                if constexpr (REFBITS) {
                  noise = (zw[i] >> (kb >> 5)) & 1u;
                } else {
                  noise = ibm_noise(zr[i], zrp[i]);
                  if (ibm_uncertain(zr[i], zrp[i], dlt[g0 + i])) {  // rare: the exact path's
                    noise = false;
                    dfr[j] |= 1u << (step * FB + g0 + i);
                    atomicOr(pendw, 1u << (step * FB + g0 + i));
                  }
                }
                bits[j] |= (noise ? 1u : 0u) << (step * FB + g0 + i);
                acc[j].add_sel(x0, x1, noise);  // weight count: popcount of bits at the end
                if constexpr (IRM) gain[(step * FB + g0 + i) * F + kb] = irm_gain(zr[i], zrp[i]);
                continue;
              }
              bool noise = false;
              float wgt;
              float m;
              if constexpr (MASK == MASK_EXTERNAL && G == 4 && decltype(vec)::value) {
                m = 1.0f - mv[i];
                wgt = m + A.weight_eps;
              } else {
                m = bin_mask<MASK>(A, b, x0, x1, zr[i], zrp[i], kb, f0 + g0 + i, noise, wgt);
              }
              bits[j] |= (noise ? 1u : 0u) << (step * FB + g0 + i);
              acc[j].add(x0, x1, wgt, m);
              if constexpr (IRM) gain[(step * FB + g0 + i) * F + kb] = irm_gain(zr[i], zrp[i]);
            }
          }
        }
      }
    };
    if (nvalid == FB) {
      if constexpr (MASK == MASK_EXTERNAL) {
        if (mask_vec)
          bin_phase(std::true_type{}, std::true_type{});
        else
          bin_phase(std::true_type{}, std::false_type{});
      } else {
        bin_phase(std::true_type{}, std::false_type{});
      }
    } else {
      bin_phase(std::false_type{}, std::false_type{});
    }
    if constexpr (MASK == MASK_IPD) {
      // Near-colinear (bin, frame) pairs (rare; DC, always one, is the Nyquist wave's):
      // exact weight from the spectra still in LDS. Waves with no such lane skip this.
#pragma unroll
      for (int j = 0; j < BPT; ++j) {
        const int kb = tid + j * NT;
        const int kp = (N - kb) & (N - 1);
        uint32_t f = ipd_fix[j];
        const bool dc = (j == 0 && tid == 0);
        if (dc) f = 0u;
        ipd_clear_n[j] += dc ? 0 : nvalid - __popc(f);  // weight count: exact integers
        while (f) {
          const int i = __builtin_ctz(f);
          f &= f - 1u;
          const cf* Zm = slot_ptr<N>(lds, i);
          cf x0, x1;
          split_pair2(Zm[kb], Zm[kp], x0, x1);
          const float w = ((ident_w >> (8 * i)) & 1ull) ? 0.01f : ipd_weight_exact(x0, x1);
          acc[j].add(x0, x1, w - 1.0f, w);  // the products went in at weight 1
        }
      }
    }
    if (nyq_wave) {
      bool noise = false, nunc = false;
      if (lane < nvalid) {
        int ln = lane;
        opaque_i(ln);  // its slot addresses formed here (held across the items they spilled)
        const cf* Zm = slot_ptr<N>(lds, ln);
        cf y0, y1, zr{0, 0};
        split_pair2(Zm[N / 2], Zm[N / 2], y0, y1);
        if constexpr (MASK == MASK_IBM) zr = slot_ptr<N>(lds, FB + ln)[N / 2];
        float wn;
        float mn = bin_mask<MASK>(A, b, y0, y1, zr, zr, N / 2, f0 + lane, noise, wn);
        if (MASK == MASK_IPD && ((ident_w >> (8 * lane)) & 1ull)) wn = mn = 0.01f;
        if (MASK == MASK_IBM &&
            ibm_uncertain(zr, zr, reinterpret_cast<const float*>(lds + G::MISC_OFF + 16)[lane])) {
          noise = false;  // rare: the exact path's
          wn = mn = 0.0f;
          nunc = true;
          atomicOr(pendw, 1u << (step * FB + lane));
        }
        an.add(y0, y1, wn, mn);
        if constexpr (MASK == MASK_IPD) {  // DC of frame `lane`
          cf d0, d1;
          const cf z0 = Zm[0];
          split_pair2(z0, z0, d0, d1);
          const float wd = ((ident_w >> (8 * lane)) & 1ull) ? 0.01f : ipd_weight_exact(d0, d1);
          adc.add(d0, d1, wd, wd);
        }
        if constexpr (IRM) gain[(step * FB + lane) * F + N / 2] = irm_gain(zr, zr);
      }
      const unsigned long long bal = __ballot(noise);
      nyq_bits |= ((uint32_t)bal & ((1u << FB) - 1u)) << (step * FB);
      if constexpr (MASK == MASK_IBM)
        nyq_dfr |= ((uint32_t)__ballot(nunc) & ((1u << FB) - 1u)) << (step * FB);
    }
    AVZ_STAMP(12);
    lds_barrier();
    AVZ_STAMP(2);
  }

  // ---- reference-exact decisions of the deferred frames (avz_ibm_exact.hpp)
  if constexpr (MASK == MASK_IBM) {
    // the unit's exact-path record (ibm_exact_units, after the block's loop): frames with a
    // deferral, frames with xunc words (reference-bit path), the Nyquist bin's deferrals; the
    // per-bin deferrals
    const uint32_t pend = pendw[0], full = pendw[1];  // block-uniform (after the last barrier)
    // round frames (published units): the reference-bit path's counted ones; every deferred
    // frame of the per-bin kernels (their exact path is rounds only)
    const uint32_t big = REFBITS ? pendw[2] : pend;
    KArgs& Ak = kernarg_chain_args();  // pointers not held through the loop
    const int gxi = (Ak.max_frames + kChunk - 1) / kChunk;  // analysis_items' units
    const int unit = slot < 0 ? b * gxi + c : gxi * Ak.batch + slot;
    if (nyq_wave && lane == 0) {
      reinterpret_cast<uint4*>(Ak.xpend)[unit] = make_uint4(pend, full, nyq_dfr, big);
      // the block's units with deferrals, by position in its item sequence (bit 31: any
      // past the 31st); ibm_exact_units reads only their records
      if (pend) *reinterpret_cast<uint32_t*>(lds + G::MISC_OFF + 56) |= 1u << min(seq, 31);
    }
    if (DLT && pend != 0u) {
#pragma unroll
      for (int j = 0; j < BPT; ++j) Ak.xdfr[(long long)unit * F + tid + j * NT] = dfr[j];
    }
  }

  // ---- chunk partials (a piece's: its tail slot; its bits merged into the chunk's words)
  float* Pt = slot < 0 ? A.part + ((long long)b * A.nchunk + c) * 5 * F
                       : A.tpart + (long long)slot * 5 * F;
  uint32_t* MW = A.mwords + ((long long)b * A.nchunk + c) * F;
  // the piece's bit range (nominal: bits past the chunk's frames are cleared too)
  const uint32_t rng = (P == 1) ? ~0u : ((1u << (kChunk / P)) - 1u) << (kChunk / P * p);
  auto put_word = [&](int k, uint32_t w) {
    if (slot < 0) {
      MW[k] = w;
    } else {
      atomicAnd(MW + k, ~rng);
      atomicOr(MW + k, w);
    }
  };
  constexpr bool DC_NYQ = MASK == MASK_IPD;  // DC sums come from the Nyquist wave
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    const int kb = tid + j * NT;
    if (DC_NYQ && kb == 0) continue;
    // binary weights were folded into the selects: their count is exact in fp32
    if constexpr (MASK == MASK_IBM) acc[j].cm = (float)__popc(bits[j]);
    if constexpr (MASK == MASK_IPD) acc[j].cm += (float)ipd_clear_n[j];
    Pt[0 * F + kb] = acc[j].c00;
    Pt[1 * F + kb] = acc[j].c11;
    Pt[2 * F + kb] = acc[j].c01r;
    Pt[3 * F + kb] = acc[j].c01i;
    Pt[4 * F + kb] = acc[j].cm;
    if constexpr (MASK == MASK_IBM) put_word(kb, bits[j]);
  }
  if (nyq_wave) {
    for (int o = 1; o < 64; o <<= 1) {
      an.c00 += __shfl_xor(an.c00, o, 64);
      an.c11 += __shfl_xor(an.c11, o, 64);
      an.c01r += __shfl_xor(an.c01r, o, 64);
      an.c01i += __shfl_xor(an.c01i, o, 64);
      an.cm += __shfl_xor(an.cm, o, 64);
      if constexpr (DC_NYQ) {
        adc.c00 += __shfl_xor(adc.c00, o, 64);
        adc.c11 += __shfl_xor(adc.c11, o, 64);
        adc.c01r += __shfl_xor(adc.c01r, o, 64);
        adc.c01i += __shfl_xor(adc.c01i, o, 64);
        adc.cm += __shfl_xor(adc.cm, o, 64);
      }
    }
    if (DC_NYQ && lane == 0) {
      Pt[0 * F] = adc.c00;
      Pt[1 * F] = adc.c11;
      Pt[2 * F] = adc.c01r;
      Pt[3 * F] = adc.c01i;
      Pt[4 * F] = adc.cm;
    }
    if (lane == 0) {
      Pt[0 * F + N / 2] = an.c00;
      Pt[1 * F + N / 2] = an.c11;
      Pt[2 * F + N / 2] = an.c01r;
      Pt[3 * F + N / 2] = an.c01i;
      Pt[4 * F + N / 2] = an.cm;
      if constexpr (MASK == MASK_IBM) put_word(N / 2, nyq_bits);
    }
  }

  // ---- a unit with round frames is published for the grid to share (ibm_exact_units): its
  // record, words (per-bin deferrals), partials and mask words (stored above) released at
  // agent scope first
  if constexpr (MASK == MASK_IBM) {
    const uint32_t big = REFBITS ? pendw[2] : pendw[0];  // block-uniform
    if (big != 0u) {
      AVZ_XT_BEGIN(tp);
      __syncthreads();
      if (tid == 0) {
        KArgs& Ak = kernarg_chain_args();
        const int gxi = (Ak.max_frames + kChunk - 1) / kChunk;
        const int unit = slot < 0 ? b * gxi + c : gxi * Ak.batch + slot;
        const XPieces q = x_pieces(pendw[0], big);
        Ak.xst[2 * unit + 1] = 0u;  // arrivals
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_store(Ak.xst + 2 * unit, kXOpen | ((uint32_t)q.n << 16), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_or(Ak.xhint + (unit >> 5), 1u << (unit & 31), __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT);
#ifdef AVZ_XTRACE  // (a count beside the interval: not the pair's form)
        if (g_stamps) {
          g_stamps[blockIdx.x * 16 + 12] += __builtin_amdgcn_s_memrealtime() - tp;
          g_stamps[blockIdx.x * 16 + 13] += 1 + 256 * q.n;  // units published, their pieces
        }
#endif
      }
    }
  }
}

// The block's work units: whole items i, i + gridDim.x, ... below a_whole (a multiple of the
// grid), then the tail items' pieces on the same stride (tail splitting, ChainArgs).
template <int N, int MASK, bool IRM, bool SPLIT, class TW>
__device__ __forceinline__ void analysis_items(const ChainArgs& A, unsigned char* lds, int gx,
                                               int n_items, const TW& tw_reg,
                                               const LaneConst<N>& K) {
  const int P = SPLIT && A.a_pieces > 1 ? A.a_pieces : 1;
  const int n_whole = P > 1 ? A.a_whole : n_items;
  const int n_end = n_whole + (n_items - n_whole) * P;  // whole items, then the pieces
  // one call site (two inlined copies of the item, whole and piece, spilled)
  int seq = 0;
  for (int u = blockIdx.x; u < n_end; u += gridDim.x) {
    const bool whole = u < n_whole;
    const int q = u - n_whole, it = whole ? u : n_whole + q / P;
    analysis_item<N, MASK, IRM>(A, lds, it % gx, it / gx, whole ? 0 : q % P, whole ? 1 : P,
                                whole ? -1 : q, tw_reg, K, seq++);
  }
}

// Persistent grid (about two blocks per CU): block i takes the (chunk, utterance) items
// i, i + gridDim.x, ... so the twiddle table is built once per block and the batch is
// spread evenly over the resident blocks (no second, partly idle round of short blocks);
// a partial last round is split into step-range pieces (analysis_items; the SPLIT instance,
// launched only when the tail splitting is on, so the whole-rounds instance carries none of
// its code).
template <int N, int MASK, bool IRM, bool SPLIT = false>
__global__ void __launch_bounds__(kCThreads, KCfg<N>::BLOCKS_PER_CU) avz_analysis_kernel(ChainArgs A) {
  using G = CGeo<N>;
  extern __shared__ __align__(16) unsigned char lds[];
  AVZ_XT(0, __builtin_amdgcn_s_memrealtime());
  if (MASK == MASK_IBM && threadIdx.x == 0)  // ibm_exact_units' unit mask (after a barrier)
    *reinterpret_cast<uint32_t*>(lds + G::MISC_OFF + 56) = 0u;
  // the per-utterance synthesis' piece finalize state, reset here (the next launch reads it)
  if (A.pstate)
    for (int b = blockIdx.x * kCThreads + threadIdx.x; b < A.batch; b += gridDim.x * kCThreads)
      A.pstate[b] = PieceState{};
  KCfg<N>::Fft::fill_twiddles(reinterpret_cast<cf*>(lds + G::TW_OFF), threadIdx.x, G::NT);
  const int gx = (A.max_frames + kChunk - 1) / kChunk;
  const int n_items = gx * A.batch;
  if constexpr (N == 1024) {
    __syncthreads();
    cf tw_reg[31];
    Fft1024x2 f;
    f.init(threadIdx.x & 63);
    f.load_twiddles(tw_reg, reinterpret_cast<const cf*>(lds + G::TW_OFF));
    if (MASK != MASK_IPD && (threadIdx.x & 32)) {  // rotated frames: (-1)^k1 (pair_loads)
      static_for<0, 16>([&](auto i) { tw_reg[2 * i] = cf{-tw_reg[2 * i].x, -tw_reg[2 * i].y}; });
    }
    LaneConst<N> K;
    K.init(threadIdx.x);
    if (MASK != MASK_IPD && (threadIdx.x & 32)) {  // rotated frames (pair_loads): window
      K.wc.ac = -K.wc.ac;                          // halves swapped, once per kernel (per item
      K.wc.as = -K.wc.as;                          // both signs stayed live and one spilled)
    }
    analysis_items<N, MASK, IRM, SPLIT>(A, lds, gx, n_items, tw_reg, K);
    if constexpr (MASK == MASK_IBM) ibm_exact_units<N, MASK, IRM, SPLIT, Tw1024>(lds, gx, n_items);
  } else {
    LaneConst<N> K;
    K.init(threadIdx.x);
    analysis_items<N, MASK, IRM, SPLIT>(A, lds, gx, n_items, NoTw{}, K);
    if constexpr (MASK == MASK_IBM) ibm_exact_units<N, MASK, IRM, SPLIT, NoTw>(lds, gx, n_items);
  }
}
}  // namespace avz
