// avz_chain_common.hpp — what the stages of the chain share (overview: avz_chunked_k.hpp):
// geometry (kChunk, CGeo, SGeo), window terms and lane constants (WinCoef, LaneConst), window
// + forward FFT (window_apply, window_fft*), shared-half pair loads (pair_loads, pair_finish),
// the IBM decision and its certificate test (ibm_noise, ibm_uncertain), bin_mask, irm_gain,
// utt_len, the kernarg view of ChainArgs (KArgs) and an analysis unit's item (unit_item).
// Needs: avz_common.hpp (with it avz_fft.hpp, avz_internal.h).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "avz_common.hpp"

namespace avz {
// Rejected variants of the chain kernels (round-chained synthesis, finalize folded into
// synthesis, the half-size real inverse, precomputed synthesis windows, LDS-twiddle stage-1
// stores, ...): DESIGN.md §6 and tools/experiments/; these headers hold the shipped paths.

constexpr int kChunk = 32;      // frames per chunk = bits of one mask word
constexpr int kSC1 = 16;        // buffer-op cache policy bit: sc1 (L1-bypassing loads, gfx940+)
typedef int v4i_t __attribute__((ext_vector_type(4)));
constexpr int kCThreads = 256;  // 4 waves

template <int N>
struct CGeo {
  using C = KCfg<N>;
  static constexpr int NT = kCThreads;
  static constexpr int NWAVE = NT / 64;
  static constexpr int H = N / 2;
  static constexpr int F = N / 2 + 1;
  static constexpr int NSLOT = NWAVE * C::FPW;     // 8 frame slots
  static constexpr int BPT = (N / 2) / NT;          // bins k < N/2 per thread
  static constexpr int SLOT_LDS = NWAVE * C::WAVE_BYTES;
  static constexpr int TW_OFF = SLOT_LDS;
  static constexpr int MISC_OFF = TW_OFF + C::TW_BYTES;
  static constexpr int LDS_BYTES = MISC_OFF + 64;
  static_assert(BPT >= 1 && BPT * NT == N / 2, "bin mapping");
  static constexpr int BLOCKS = C::BLOCKS_PER_CU;  // resident blocks per CU (= waves per SIMD)
  static_assert(BLOCKS * LDS_BYTES <= 160 * 1024, "resident blocks per CU");
};

// Synthesis frames per lane group per step: KCfg's SYN_R, except the N = 512 external-mask
// post-filters, whose strided mask reads need the registers of the second frame (at R = 2
// they spilled 44-72 B per lane).
template <int N, int PF>
constexpr int kSynR = (N == 512 && (PF == PF_EXT_FLOOR || PF == PF_EXT_MUL)) ? 1 : KCfg<N>::SYN_R;

// Synthesis geometry: as CGeo with R frames per lane group per step (NSLOT frame slots,
// each a lane group's transform area; slot s is "virtual wave" s / FPW of the slot area).
template <int N, int R_ = KCfg<N>::SYN_R>
struct SGeo {
  using C = KCfg<N>;
  static constexpr int NT = kCThreads;
  static constexpr int NWAVE = NT / 64;
  static constexpr int R = R_;
  static constexpr int H = N / 2;
  static constexpr int F = N / 2 + 1;
  static constexpr int NSLOT = NWAVE * C::FPW * R;
  static constexpr int BPT = (N / 2) / NT;
  static constexpr int SLOT_LDS = NWAVE * C::WAVE_BYTES * R;
  static constexpr int TW_OFF = SLOT_LDS;
  static constexpr int MISC_OFF = TW_OFF + C::TW_BYTES;
  static constexpr int LDS_BYTES = MISC_OFF + 64;
  static constexpr int BLOCKS = C::SYN_BLOCKS_PER_CU;
  static_assert(BLOCKS * LDS_BYTES <= 160 * 1024, "resident synthesis blocks per CU");
};

// Per-lane analysis window * 1/sum(win) and synthesis window * sum(win)/N terms.
template <int N>
struct WinCoef {
  float a0, ac, as, s0, sc, ss;
  __device__ __forceinline__ void init(const LaneMap<N>& lm) {
    double s, c;
    sincospi(2.0 * lm.in0 / N, &s, &c);
    const double sca = 2.0 / N;
    a0 = (float)(0.5 * sca);
    ac = (float)(0.5 * sca * c);
    as = (float)(0.5 * sca * s);
    sincospi(2.0 * lm.out0 / N, &s, &c);
    s0 = 0.25f;
    sc = (float)(0.25 * c);
    ss = (float)(0.25 * s);
  }
};

// 1 / (win[m]^2 + win[m + N/2]^2): the istft window-sum normalisation of one sample.
template <int N>
__device__ __forceinline__ float inv_wsum(int m) {
  const float c1 = cospif(2.0f * (float)m / (float)N);
  const float wa = 0.5f - 0.5f * c1, wb = 0.5f + 0.5f * c1;
  return 1.0f / (wa * wa + wb * wb);
}

// Lane constants of the chain kernels (FFT twiddle registers, lane map, window terms,
// the synthesis OLA normalisation and inverse window terms): computed once per block by
// the persistent kernels, not per item (the fp64 sincospi calls cost 1-2 us per item).
template <int N>
struct LaneConst {
  typename KCfg<N>::Fft fft;
  LaneMap<N> lm;
  WinCoef<N> wc;
  float inv[4];  // synthesis OLA: 1 / window-square sum of samples m0 .. m0 + 3
  __device__ __forceinline__ void init(int tid) {
    const int lane = tid & 63;
    fft.init(lane);
    lm.init(lane);
    wc.init(lm);
    const int m0 = 4 * (tid % (N / 8));  // synthesis OLA role (N/2 / 4 float4 groups)
#pragma unroll
    for (int i = 0; i < 4; ++i) inv[i] = inv_wsum<N>(m0 + i);
  }
};

// Analysis window of a lane's points: register r holds sample n0 + IN_STRIDE r, weight
// w = a0 - ac cos(2 pi IN_STRIDE r / N) + as sin(...) (angle addition on the lane's n0).
// Registers PPL/2 apart are N/2 samples apart, where the periodic Hann window satisfies
// w[n + N/2] = 2 a0 - w[n]: one subtraction instead of two FMAs for the upper half.
template <int N = 1024, int PPL>
__device__ __forceinline__ void window_apply(cf (&v)[PPL], float a0, float ac, float as) {
  using C = KCfg<N>;
  static_assert(C::IN_STRIDE * (PPL / 2) == N / 2, "upper-half registers are N/2 later");
  const float a2 = a0 + a0;
  static_for<0, PPL / 2>([&](auto r) {
    constexpr int j = (C::IN_STRIDE * 32 / N) * r;  // 2 pi (IN_STRIDE r)/N = 2 pi j/32
    constexpr float cr = W32::c[j % 32], sr = -W32::s[j % 32];
    const float w = fmaf(as, sr, fmaf(-ac, cr, a0));
    v[r] = c_scale(v[r], w);
    v[r + PPL / 2] = c_scale(v[r + PPL / 2], a2 - w);
  });
}

// IBM decision |S_int| > |S_tgt| (oracle_debug.py:49-53, strict) from the packed reference
// pair z = tgt + i int: 2T = zr + conj(zrp), 2I = (zr - conj zrp)/i, and
// |2T|^2 - |2I|^2 = 4 Re(zr zrp), so noise <=> Re(zr zrp) < 0 (one product, one fma).
__device__ __forceinline__ bool ibm_noise(cf zr, cf zrp) {
  return fmaf(zr.x, zrp.x, -(zr.y * zrp.y)) < 0.0f;
}

// Sum over the 32 lanes of a lane group (DPP within rows, v_permlane16_swap across them).
__device__ __forceinline__ float group32_sum(float e) {
  e += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(e), 0xB1, 0xF, 0xF, false));
  e += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(e), 0x4E, 0xF, 0xF, false));
  e += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(e), 0x141, 0xF, 0xF, false));
  e += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(e), 0x140, 0xF, 0xF, false));
  float lo, hi;
  xhalf<16>(e, lo, hi);
  return lo + hi;
}
__device__ __forceinline__ float frame_energy(const cf (&v)[32]) {
  float e = 0.0f;
  static_for<0, 32>([&](auto r) {
    e = fmaf(v[r].x, v[r].x, e);
    e = fmaf(v[r].y, v[r].y, e);
  });
  return e;
}
// Window + forward FFT with the lane's twiddles in registers (N = 1024 analysis). Both
// FFT stages store each output pair as it is formed (the transpose scratch, then the
// spectrum); after(k) runs right after spectrum output k is stored (the next step's load
// into register k).
struct NoAfter {
  template <class K>
  __device__ __forceinline__ void operator()(K) const {}
};
// en (non-null: IBM reference waves of the plans without the reference-bit hand-off): the
// group's windowed frame energy, the exact-IBM certificate's scale (ibm_exact_frames).
template <class After = NoAfter>
__device__ __forceinline__ void window_fft_reg(cf (&v)[32], const WinCoef<1024>& wc,
                                               const Fft1024x2& fft, cf* spec,
                                               const cf (&tw_reg)[31], const LaneMap<1024>& lm,
                                               After&& after = After{}, float* en = nullptr) {
  window_apply(v, wc.a0, wc.ac, wc.as);
  if (en) *en = group32_sum(frame_energy(v));
  fft.stage1_reg_st(v, spec, tw_reg);
  fft.transpose_read(v, spec);
  fft.stage2_emit(v, [&](auto k, cf x) {
    spec[lm.out0 + 32 * k] = x;
    after(k);
  });
}

// Reference pair of the IBM mask (N = 1024, register twiddles): the reference spectrum is
// only needed for one bit per bin, noise <=> Re(Zr[k] Zr[N - k]) < 0 (ibm_noise). Lane l
// holds Zr[l + 32 k]. Only the upper-half outputs (k >= 16) are stored, as formed, their
// registers taking their next-step loads during the stage; the lower half stays in
// registers, the lane reads the partners N - (l + 32 k), k < 16, back (all in the stored
// upper half but DC's, which is its own partner), publishes the 16 bits as word l of the
// slot (bytes 0..127) and only then reloads registers 0-15 (analysis 80.7-80.9 -> 79.1-79.5
// us against storing all 32 and reading both operands back, profiles/r04/ab_ref_half.txt).
// The Nyquist bin (lane 0, k = 16) stays readable at spec[N / 2].
//
// Certificate (avz_ibm_exact.hpp): the group's windowed frame energy gives delta = cert
// ||z|| (cert = kappa eps, ChainArgs::ibm_cert), a bound on every output bin's error; a bin
// pair whose |Re(Zr[k] Zr[N - k])| does not clear (2 sqrt 2 + 1) delta max(|components|,
// delta) could be decided either way by that error. A frame with such a bin (DC included)
// publishes no noise bits and returns true: the item's exact path decides it
// (ibm_exact_item). delta goes to dl; the Nyquist bin (lane 0, k = 16, left in spec[N / 2])
// is certified by the bin phase's Nyquist wave with it.
//
// Level rule (ibm_level_range, avz_internal.h): the test above is trusted only on fp32 values
// that neither underflowed nor overflowed, which the frame's energy settles. A frame whose
// energy is outside [ibm_en_lo, ibm_en_lo + ibm_en_span] (one unsigned compare on its bits; 0,
// inf and NaN are outside) is deferred whole -- every bin uncertain, the Nyquist bin by a
// delta of inf (reference-bit path) or NaN -- unless every reference sample of it is exactly
// 0 (zero padding, the generator's silent blocks: the reference's 0 > 0 is false, as the fp32
// decision).
// true when the pair's decision is not certified by the error bound dl (= delta); the negated
// compare makes a NaN bound (a frame the level rule defers) or a NaN product uncertain
__device__ __forceinline__ bool ibm_uncertain(cf zr, cf zrp, float dl) {
  const float d = fmaf(zr.x, zrp.x, -(zr.y * zrp.y));
  const float m = fmaxf(fmaxf(fabsf(zr.x), fabsf(zr.y)), fmaxf(fmaxf(fabsf(zrp.x), fabsf(zrp.y)), dl));
  return !(fabsf(d) >= 3.9f * dl * m);
}
// the level rule's compare: the energy's bits outside [lo, lo + span] (negative: never)
__device__ __forceinline__ bool ibm_level_out(float en, uint32_t lo, uint32_t span) {
  return __float_as_uint(en) - lo > span;
}
template <class After = NoAfter>
__device__ __forceinline__ uint32_t window_fft_reg_ibm_bits(cf (&v)[32], const WinCoef<1024>& wc,
                                                        const Fft1024x2& fft, cf* spec,
                                                        const cf (&tw_reg)[31],
                                                        const LaneMap<1024>& lm, float eg0,
                                                        float eg1, float cert, float& dl,
                                                        After&& after = After{}) {
  constexpr int N = 1024;
  window_apply(v, wc.a0, wc.ac, wc.as);
  const int l = lm.out0;
  fft.stage1_reg_st(v, spec, tw_reg);
  fft.transpose_read(v, spec);
  fft.stage2_emit(v, [&](auto k, cf x) {
    if constexpr (decltype(k)::value >= 16) {
      spec[l + 32 * k] = x;
      after(k);
    }
  });
  dl = cert * sqrtf(lm.grp ? eg1 : eg0);  // delta >= kappa eps ||z|| (the caller's scale)
  __builtin_amdgcn_wave_barrier();
  // the word is built from bit 15 down (w = 2 w + bit): a select of 1 << k per bin held the
  // 16 constants in VGPRs for the whole kernel
  uint32_t w = 0u;
  float slack = __builtin_inff();  // min over bins of |D| - 3.9 dl m (< 0: uncertain)
  const float dl39 = 3.9f * dl;
  static_for<0, 16>([&](auto kk) {
    constexpr int k = 15 - decltype(kk)::value;
    const int m = l + 32 * k;
    cf zp = spec[(N - m) & (N - 1)];
    if (k == 0 && l == 0) zp = v[0];  // DC: its own partner (index 0 is not stored)
    w = (w << 1) | (ibm_noise(v[k], zp) ? 1u : 0u);
    const float d = fmaf(v[k].x, zp.x, -(v[k].y * zp.y));
    const float mm = fmaxf(fmaxf(fabsf(v[k].x), fabsf(v[k].y)),
                           fmaxf(fmaxf(fabsf(zp.x), fabsf(zp.y)), dl));
    slack = fminf(slack, fmaf(-dl39, mm, fabsf(d)));
  });
  const bool unc = slack < 0.0f;
  uint32_t um = 0u;  // the lane's uncertain bins (bit k: bin l + 32 k), as its word w
  if (__ballot(unc) != 0ull) {  // rare (wave-uniform): which bins, by the same test
    static_for<0, 16>([&](auto kk) {
      constexpr int k = 15 - decltype(kk)::value;
      const int m = l + 32 * k;
      cf zp = spec[(N - m) & (N - 1)];
      if (k == 0 && l == 0) zp = v[0];
      const float d = fmaf(v[k].x, zp.x, -(v[k].y * zp.y));
      const float mm = fmaxf(fmaxf(fabsf(v[k].x), fabsf(v[k].y)),
                             fmaxf(fmaxf(fabsf(zp.x), fabsf(zp.y)), dl));
      um = (um << 1) | (fmaf(-dl39, mm, fabsf(d)) < 0.0f ? 1u : 0u);
    });
    w &= ~um;  // their decisions are the exact path's
  }
  reinterpret_cast<uint32_t*>(spec)[l] = w;
  static_for<0, 16>([&](auto k) { after(k); });
  return um;
}

// Window + forward FFT of the synthesis kernel and of the N = 512 analysis kernel:
//  N = 1024: factored register twiddles (Fft1024x2::stage1_ab_st), both stages' outputs
//            stored as formed (synthesis 73.7-74.1 -> 72.7-73.1 us, profiles/r03d/ab_more.txt);
//  N = 512, IL512: the interleaved Fft512x2 (the two-block synthesis kernel: 81.0 -> 80.3
//            us; the three-block N = 512 analysis kernel ran slower with it, 81.3 -> 82.5 us).
template <int N, bool IL512 = false, class After = NoAfter>
__device__ __forceinline__ void window_fft(cf (&v)[KCfg<N>::PPL], const WinCoef<N>& wc,
                                           const typename KCfg<N>::Fft& fft, cf* spec,
                                           const LaneMap<N>& lm, After&& after = After{},
                                           float* en = nullptr) {
  using C = KCfg<N>;
  float a0 = wc.a0, ac = wc.ac, as = wc.as;
  opaque(a0);
  opaque(ac);
  opaque(as);
  window_apply<N>(v, a0, ac, as);
  if (en) {  // the lane group's windowed frame energy (exact-IBM certificate scale)
    float e = 0.0f;
    static_for<0, C::PPL>([&](auto r) {
      e = fmaf(v[r].x, v[r].x, e);
      e = fmaf(v[r].y, v[r].y, e);
    });
    *en = group32_sum(e);
  }
  if constexpr (N == 1024) {
    fft.stage1_ab_st(v, spec);
    fft.transpose_read(v, spec);
    fft.stage2_emit(v, [&](auto k, cf x) {
      spec[lm.out0 + C::OUT_STRIDE * k] = x;
      after(k);
    });
  } else if constexpr (IL512) {
    fft.forward_emit(v, spec, [&](auto k, cf x) {
      spec[lm.out0 + C::OUT_STRIDE * k] = x;
      after(k);
    });
  } else {
    fft.forward(v, spec);
    static_for<0, C::PPL>([&](auto k) { spec[lm.out0 + C::OUT_STRIDE * k] = v[k]; });
  }
}

// Shared-half loads of a wave's frame pair (Fft1024x2, N = 1024): frames 2w and 2w + 1
// overlap by N/2 = 16 registers, so the wave loads 1536 samples per stream (24 loads)
// instead of 2 x 1024 (32). Lane group 1 holds its frame rotated by N/2 — register r < 16
// is sample 512 + 32 r + l of the frame, r >= 16 is sample 32 (r - 16) + l, i.e. the
// second half of frame 2w — so both groups take the shared half in the same registers:
//   v[j], j < 16:   group 0 samples sp + 32 j, group 1 sp + 1024 + 32 j (own halves);
//   v[16 + 2 i]:    group 0 sample sp + 512 + 64 i, group 1 the next 32 (shared half),
//                   spread to v[16 + 2 i] / v[17 + 2 i] on every lane by one
//                   v_permlane32_swap per float once the loads have landed (pair_finish).
// sp = the pair's first sample + l. The rotation is a circular shift by N/2 of group 1's
// frame: its window weights swap halves (ac, as negated: window_apply's w <-> 2 a0 - w)
// and its spectrum comes out as (-1)^k X[k], undone by (-1)^k1 folded into the stage-1
// twiddles. Analysis kernel only: in the synthesis kernel (LDS twiddles, the sign folded
// into the odd frames' post-filter gain) it measured 73.1 -> 75.1 us against the analysis
// kernel's 80.3 -> 79.0 (profiles/r02z/ab_experiments.txt).
template <bool NONNEG>
__device__ __forceinline__ void pair_loads(cf (&v)[32], rsrc_t r0, rsrc_t r1, int sp, int g) {
  static_for<0, 16>([&](auto j) {
    const int e = sp + 1024 * g + 32 * j;
    v[j].x = NONNEG ? bload_nn(r0, e) : bload(r0, e);
    v[j].y = NONNEG ? bload_nn(r1, e) : bload(r1, e);
  });
  static_for<0, 8>([&](auto i) {
    const int e = sp + 512 + 32 * (2 * i) + 32 * g;
    v[16 + 2 * i].x = NONNEG ? bload_nn(r0, e) : bload(r0, e);
    v[16 + 2 * i].y = NONNEG ? bload_nn(r1, e) : bload(r1, e);
  });
}
__device__ __forceinline__ void pair_finish(cf (&v)[32]) {
  static_for<0, 8>([&](auto i) {
    const auto rx = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[16 + 2 * i].x),
                                                     __float_as_uint(v[16 + 2 * i].x), false, false);
    const auto ry = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[16 + 2 * i].y),
                                                     __float_as_uint(v[16 + 2 * i].y), false, false);
    v[16 + 2 * i] = cf{__uint_as_float(rx[0]), __uint_as_float(ry[0])};
    v[17 + 2 * i] = cf{__uint_as_float(rx[1]), __uint_as_float(ry[1])};
  });
}

// Samples of utterance b: the device length clamped to the host-validated max_len (so an
// inconsistent len[] never moves an access outside the caller's rows), or max_len for all.
// A piece's seam half: written through to memory (agent-scope stores, sc1), so the last
// piece of the utterance to arrive -- on any XCD -- reads it in the same kernel.
// (row: block-uniform base of n floats; i: the thread's element)
__device__ __forceinline__ void store_through(float* row, int n, int i, float4 v) {
  const v4i_t d = {__float_as_int(v.x), __float_as_int(v.y), __float_as_int(v.z),
                   __float_as_int(v.w)};
  __builtin_amdgcn_raw_buffer_store_b128(d, make_rsrc(row, n), 4 * i, 0, kSC1);
}

// len[] is read-only for the whole chain, so it is read through the constant address space:
// with a wave-uniform b that is one s_load_dword (scalar cache) instead of a vector load
// plus readfirstlane on the item / unit start's dependent latency chain.
template <class CA>
__device__ __forceinline__ int utt_len(CA& A, int b) {
  if (!A.len) return A.max_len;
  const __attribute__((address_space(4))) int* lc =
      (const __attribute__((address_space(4))) int*)(A.len);
  return min(lc[b], A.max_len);
}

// Mask value m and covariance weight of one (bin, frame).
template <int MASK>
__device__ __forceinline__ float bin_mask(const ChainArgs& A, int b, cf x0, cf x1, cf zr,
                                          cf zrp, int k, int t, bool& noise, float& wgt) {
  if constexpr (MASK == MASK_IBM) {
    noise = ibm_noise(zr, zrp);
    wgt = noise ? 1.0f : 0.0f;
    return wgt;
  } else if constexpr (MASK == MASK_IPD) {
    wgt = ipd_weight(x0, x1);
    return wgt;
  } else if constexpr (MASK == MASK_ONES) {  // unmasked covariance (SRP, MPDR)
    wgt = 1.0f;
    return 1.0f;
  } else {
    const float M =
        A.ext_mask[(long long)b * A.mask_sb + (long long)k * A.mask_sf + (long long)t * A.mask_st];
    const float m = 1.0f - M;
    wgt = m + A.weight_eps;
    return m;
  }
}

// IRM post-filter gain of one (bin, frame) from the packed reference pair
// (oracle_reverb.py:143-156): with 2T, 2I the unscaled split, |2T|^2/(|2T|^2+|2I|^2+4e-10)
// equals P_t/(P_t + P_i + 1e-10).
__device__ __forceinline__ float irm_gain(cf zr, cf zrp) {
  const float tr = zr.x + zrp.x, ti = zr.y - zrp.y;
  const float ir = zr.y + zrp.y, ii = zr.x - zrp.x;
  const float pt = tr * tr + ti * ti, pi = ir * ir + ii * ii;
  return sqrtf(pt / (pt + pi + 4e-10f));
}

// The kernel's ChainArgs read afresh from the kernarg segment through an opaque address:
// fields only the exact path uses were otherwise loaded at the kernel's start and held
// through the step loop (12 SGPRs more, spilled into VGPR lanes).
// In the constant address space: its fields are scalar loads (uniform). Through a generic
// pointer they were vector loads the compiler took for divergent: every buffer load of the
// exact path then ran in a descriptor waterfall loop.
using KArgs = const __attribute__((address_space(4))) ChainArgs;
__device__ __forceinline__ KArgs& kernarg_chain_args() {
  uintptr_t u = (uintptr_t)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(u));
  return *(KArgs*)u;
}
struct NoTw {};
using Tw1024 = cf[31];  // the register-twiddle path's twiddles (a type tag here)

// The analysis unit u's item: whole items u < n_items (b = u / gx, c = u % gx), tail pieces
// n_items + q (item n_whole + q / P); its partials (chunk partials / the piece's tail slot).
template <int F, class CA>
__device__ __forceinline__ float* unit_item(CA& A, int u, int gx, int n_items, int n_whole, int P,
                                            int& b, int& c) {
  if (u < n_items) {
    b = u / gx;
    c = u % gx;
    return A.part + ((long long)b * A.nchunk + c) * 5 * F;
  }
  const int q = u - n_items, it = n_whole + q / P;
  b = it / gx;
  c = it % gx;
  return A.tpart + (long long)q * 5 * F;
}
}  // namespace avz
