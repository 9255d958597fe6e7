// avz_chain_utt.hpp — the per-utterance synthesis kernels of the chain (avz_chunked_k.hpp):
// one block synthesises and peak-normalises whole utterances and may solve their bins itself.
// N = 1024: UttGeo, avz_synthesis_utt_kernel; N = 512: Utt512Geo, avz_synthesis_utt512_kernel.
// Needs: avz_chain_common.hpp, avz_chain_solve.hpp (bin_cov_sums_utt).
#pragma once
#include "avz_chain_common.hpp"
#include "avz_chain_solve.hpp"

namespace avz {
// One 8-wave block per CU synthesises WHOLE utterances (b = blockIdx.x, + gridDim.x, ...),
// 16 frames per step, and peak-normalises each one itself at its end: no chunk seams, no
// heads / tails, no finalize launch, and the rescale re-reads the block's own output from
// L2 / Infinity Cache instead of a second HBM pass over the batch. Every wave runs its own
// two frames end to end -- window + forward Fft1024x2 (the next step's loads issued from
// inside its last stage), apply w^H y + post-filter, each frame's real inverse as an
// N/2-point complex Fft512x2 -- with no block barrier in between (the apply reads only the
// wave's own spectra); the block meets twice per step, around the overlap-add of the 16
// segments, which reads neighbouring waves' frames. Reference semantics as the two-block
// kernel + avz_finalize_kernel (oracle_debug.py:80-94, scipy istft's OLA and N/2 trim).
constexpr int kUttThreads = 512;
struct UttGeo {
  static constexpr int N = 1024, H = 512, F = 513, FB = 16;  // frames per step: 8 waves x 2
  static constexpr int SLOT = KCfg<1024>::GROUP_BYTES;       // one frame (transpose rows of 34)
  static constexpr int TW_OFF = FB * SLOT;                   // W1024 table (Fft512x2 inverse)
  static constexpr int COEF_OFF = TW_OFF + KCfg<1024>::TW_BYTES;  // the utterance's alpha, beta
  static constexpr int RED_OFF = COEF_OFF + F * 16;
  static constexpr int LDS_BYTES = RED_OFF + 64;
  static_assert(LDS_BYTES <= 160 * 1024, "one block per CU");
  static_assert(kChunk % FB == 0, "a step stays inside one 32-frame mask chunk");
};
__device__ __forceinline__ cf* utt_frame(unsigned char* lds, int f) {
  return reinterpret_cast<cf*>(lds + f * UttGeo::SLOT);
}

// SOLVE: the block solves its utterance's 513 bins itself (the MVDR solve of
// avz_solve_kernel, one bin per thread, straight into the LDS coefficient table) instead of
// reading the solve kernel's coef[] -- no solve launch (plain MVDR plans without the
// item-level fallback or debug outputs). PIECES: the instance for a split batch (whole
// utterances, then step pieces; synth_split) -- the whole-rounds instance compiles the
// piece logic out (with it the step loop ran 92.7 -> 98.5 us at B = 256).
template <int PF, bool SOLVE, bool PIECES>
__global__ void __launch_bounds__(kUttThreads, 2) avz_synthesis_utt_kernel(ChainArgs A) {
  constexpr int N = UttGeo::N, H = UttGeo::H, F = UttGeo::F, FB = UttGeo::FB;
  extern __shared__ __align__(16) unsigned char lds[];
  cf* twid = reinterpret_cast<cf*>(lds + UttGeo::TW_OFF);
  float* red = reinterpret_cast<float*>(lds + UttGeo::RED_OFF);
  Fft1024x2::fill_twiddles(twid, threadIdx.x, kUttThreads);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7
  const int lane = tid & 63;
  // A wave's two frames (2 wave, 2 wave + 1) overlap by N/2 and are loaded as in the
  // analysis kernel (pair_loads: 24 sample pairs per lane instead of 32, lane group 1's frame
  // rotated by N/2): its window halves swapped (ac, as negated) and its spectrum's (-1)^k
  // undone by (-1)^k1 on the stage-1 twiddles (the odd j factors twa[j - 1] of k1 = 8 m + j)
  Fft1024x2 fft;
  fft.init(lane);
  LaneMap<N> lm;
  lm.init(lane);
  if (lm.grp) {
    static_for<0, 4>([&](auto i) { fft.twa[2 * i] = cf{-fft.twa[2 * i].x, -fft.twa[2 * i].y}; });
  }
  const WinCoef<N> wc0 = [&] {
    WinCoef<N> w;
    w.init(lm);
    if (lm.grp) {
      w.ac = -w.ac;
      w.as = -w.as;
    }
    return w;
  }();
  const int my = 2 * wave + lm.grp;  // frame of the step = slot
  // apply bins: m_j = lane + 64 j (j < 4) pairs bin kA = m with kB = N/2 - m; bin N/4 (its
  // own partner) on lanes 0 (frame 2 wave) and 1 (frame 2 wave + 1)
  cf om[4];  // e^{+2 pi i m_j / N}
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double sn, cs;
    sincospi(2.0 * (lane + 64 * j) / N, &sn, &cs);
    om[j] = cf{(float)cs, (float)sn};
  }
  // inverse output: x[k] = conj(z[m]), m = mh + 16 k -> samples 2m, 2m + 1 (0.5 hann)
  float wh_c[2], wh_s[2];
  const int mh = (lane & 15) + 256 * ((lane >> 4) & 1);
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    double sn, cs;
    sincospi(2.0 * (2 * mh + e) / N, &sn, &cs);
    wh_c[e] = (float)(0.25 * cs);
    wh_s[e] = (float)(0.25 * sn);
  }
  // overlap-add role: 4 consecutive samples m0.. of segments sgrp + 4 si
  float inv[4];  // (filled after a first piece's pre-solve: live across it, they spilled)
  __syncthreads();  // twiddle table
  AVZ_STAMP_DECL();
  AVZ_STAMP_INIT();

  // The block's work units g = blockIdx.x, + gridDim.x, ...: the whole utterances g <
  // s_whole, then the pieces q = g - s_whole of the utterances [s_whole, batch) (ChainArgs
  // s_pieces, s_steps): utterance s_whole + q / s_pieces, its steps [p s_steps, (p + 1) s_steps),
  // p = q % s_pieces (the host splits only a partial last round or a batch below the CU
  // count). With the in-kernel piece finalize (s_ipf: the batch has whole rounds, and its
  // rem * s_pieces piece units fit one round) the pieces come FIRST: unit index g < G is
  // piece q = g (none for g >= rem * s_pieces), g >= G whole utterance g - G, so every block
  // runs at most one piece and then its whole utterances, during which the piece's interior
  // is rescaled once its utterance's last piece has published 1/peak. A whole utterance with
  // a bad device length (host validates) reports NaN, as finalize does; such an utterance's
  // pieces, and pieces past an utterance's last step, are skipped (its first piece, or the
  // piece finalize kernel, reports the NaN).
  const int pieces = PIECES && A.s_pieces > 0 ? A.s_pieces : 0;
  const int s_whole = pieces > 0 ? A.s_whole : A.batch;
  const bool ipf = PIECES && pieces > 0 && A.s_ipf;
  const int G = gridDim.x;
  const int n_pu = (A.batch - s_whole) * pieces;  // piece units
  const int n_units = ipf ? G + s_whole : s_whole + n_pu;
  struct Unit {
    int g, b, s_lo, s_hi, slot;  // slot: the piece's seam slot, -1 for a whole utterance
  };
  auto unit_at = [&](int g) -> Unit {
    for (; g < n_units; g += gridDim.x) {
      // lengths read back as block-uniform values: a loop exit decided on a vector load
      // made the next unit's buffer descriptors divergent (a waterfall loop per load)
      const bool is_whole = ipf ? g >= G : g < s_whole;
      if (is_whole) {
        const int gw = ipf ? g - G : g;
        const int Lg = __builtin_amdgcn_readfirstlane(utt_len(A, gw));
        if (Lg >= N) return Unit{g, gw, 0, ((Lg + H - 1) / H + 1 + FB - 1) / FB, -1};
        if (tid == 0 && A.peak) A.peak[gw] = __builtin_nanf("");
        continue;
      }
      const int pc = pieces > 0 ? pieces : 1;  // (0 only in the whole-rounds instance)
      const int q = ipf ? g : g - s_whole;
      if (q >= n_pu) continue;
      const int bq = s_whole + q / pc, lo = (q % pc) * A.s_steps;
      const int Lq = __builtin_amdgcn_readfirstlane(utt_len(A, bq));
      const int ns = ((Lq + H - 1) / H + 1 + FB - 1) / FB;
      if (Lq >= N && lo < ns) return Unit{g, bq, lo, min(ns, lo + A.s_steps), q};
      if (ipf && Lq < N && lo == 0 && tid == 0 && A.peak) A.peak[bq] = __builtin_nanf("");
    }
    return Unit{n_units, A.batch, 0, 0, -1};
  };
  auto rsrcs = [&](int bb, rsrc_t& a0, rsrc_t& a1) {
    bb = __builtin_amdgcn_readfirstlane(bb);
    const float* mixb = A.mix + (long long)bb * A.mix_stride;
    const int len = __builtin_amdgcn_readfirstlane(utt_len(A, bb));
    a0 = make_rsrc(mixb, len);
    a1 = make_rsrc(mixb + A.ch_stride, len);
  };
  cf v[32];
  // a unit's first step (frames f0 ..): at f0 = 0 wave 0's first frame starts N/2 before
  // sample 0 (range-checked offsets); every other frame starts at sample >= 0
  auto first_loads = [&](rsrc_t a0, rsrc_t a1, int f0) {
    const int sp = (f0 + 2 * wave) * H - N / 2 + lm.in0;
    if (wave >= 1 || f0 > 0)
      pair_loads<true>(v, a0, a1, sp, lm.grp);
    else
      pair_loads<false>(v, a0, a1, sp, lm.grp);
    // Not dead: the retired unshared load path left `my` among this lambda's captures, and
    // without it the compiler schedules all eight instances' first loads and window
    // differently. Pinned until a change to this kernel is measured on its own (Makefile).
    (void)my;
  };
  // the utterance's bins solved into the LDS coefficient table (SOLVE)
  auto solve_coefs = [&](int bb, int TT, auto vf) {
    constexpr int VF = decltype(vf)::value;
    float4* ct = reinterpret_cast<float4*>(lds + UttGeo::COEF_OFF);
    const int nch = (TT + kChunk - 1) / kChunk;
    for (int k = tid; k < F; k += kUttThreads) {
      double R[5], w[4];
      bin_cov_sums_utt<N, PIECES, VF>(A, bb, k, nch, R);
      const double* d = A.steer + 4 * k;
      mvdr_weights_d(R, k, N, A, d[0], d[1], d[2], d[3], w, nullptr);
      cf al, be;
      coef_from_w(w[0], w[1], w[2], w[3], al, be, nullptr);
      ct[k] = make_float4(al.x, al.y, be.x, be.y);
    }
  };
  Unit cu = unit_at(blockIdx.x);
  // A piece (the block's first unit) solves before any sample is loaded: its utterance's
  // chunks may have been split by the analysis tail (up to 8 partial vectors per chunk),
  // summed 16 vectors per round trip with the registers the samples would hold (with the
  // samples in flight, 8 per round trip spilled)
  bool coefs_ready = false;
  if (PIECES && SOLVE && cu.slot >= 0) {
    const int Lp = __builtin_amdgcn_readfirstlane(utt_len(A, cu.b));
    solve_coefs(cu.b, (Lp + H - 1) / H + 1, std::integral_constant<int, 16>{});
    coefs_ready = true;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) inv[i] = inv_wsum<N>(4 * (tid & 127) + i);
  if (cu.b < A.batch) {
    rsrc_t a0, a1;
    rsrcs(cu.b, a0, a1);
    first_loads(a0, a1, PIECES ? cu.s_lo * FB : 0);
  }
  // NORM_PEAK: an utterance's rescale (its own output, L1-bypassing loads) runs spread over
  // the NEXT utterance's steps, one slice per overlap-add phase, so its memory traffic hides
  // under that utterance's FFTs; a block's last utterance rescales at once.
  float* rs_out = nullptr;  // pending rescale: output row, scale, float4 groups, done
  float rs_scale = 0.0f;
  int rs_n4 = 0, rs_done = 0;
  constexpr int RS_U = 4;   // float4 groups per thread per slice (8 slices cover 4 s)
  constexpr int RS_UP = 8;   // the same during a piece's steps (4 slices cover 4 s)
  constexpr int RS_BULK = 32;  // after the loop: a 4-s utterance in one round trip of loads
  // s_ipf: a piece's own interior waits for its utterance's 1/peak (pstate[rs_lazy].fin, piece
  // rs_lp): each slice loads it beside the output and stores only once it is published
  int rs_lazy = -1, rs_lp = 0;
  uint32_t* redu = reinterpret_cast<uint32_t*>(red);  // red[8 ..]: block-uniform hand-offs
  auto rescale_slice = [&](auto uc, int lo, int hi, auto issue_more) -> bool {
    constexpr int U = decltype(uc)::value;
    const rsrc_t ro = make_rsrc(rs_out, 4LL * rs_n4);
    int tq = tid;
    if constexpr (PIECES) opaque_i(tq);  // offsets recomputed per slice (hoisted, they spilled)
    float4 x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const v4i_t d = __builtin_amdgcn_raw_buffer_load_b128(ro, 16 * (lo + u * kUttThreads + tq), 0,
                                                            kSC1);
      x[u] = make_float4(__int_as_float(d.x), __int_as_float(d.y), __int_as_float(d.z),
                         __int_as_float(d.w));
    }
    uint32_t fb = 0;
    if (PIECES && rs_lazy >= 0)
      fb = __hip_atomic_load(&A.pstate[rs_lazy].fin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    issue_more();  // work that overlaps the loads
    if (PIECES && rs_lazy >= 0) {
      fb = __builtin_amdgcn_readfirstlane(fb);
      if (fb == 0u || A.dbg_ipf == 2) return false;  // not yet published: again next step
      rs_scale = __uint_as_float(fb);
      rs_lazy = -1;
    }
    float4* o4 = reinterpret_cast<float4*>(rs_out);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = lo + u * kUttThreads + tq;
      if (i < hi) {
        x[u].x *= rs_scale; x[u].y *= rs_scale; x[u].z *= rs_scale; x[u].w *= rs_scale;
        o4[i] = x[u];
      }
    }
    return true;
  };
  // the pending rescale's remaining part, U float4 loads per thread in flight (a lazy one
  // resolved first, rs_resolve)
  auto rescale_rest = [&](auto uc) {
    constexpr int U = decltype(uc)::value;
    for (; rs_done < rs_n4; rs_done += U * kUttThreads)
      rescale_slice(uc, rs_done, min(rs_n4, rs_done + U * kUttThreads), [] {});
    rs_out = nullptr;
  };
  // A piece's interior still waiting at its block's next utterance end: take 1/peak if it is
  // published, else hand the piece back to the last arriver (.st bit p) -- unless that one
  // has passed it already (bit 32 + p), in which case 1/peak is published by now. Called by
  // every thread after tid 0's redu[12] / redu[10..11] and a barrier (end-of-unit code).
  auto rs_resolve = [&]() {
    const uint32_t fb = redu[12];
    const unsigned long long st = *reinterpret_cast<const unsigned long long*>(redu + 10);
    if (fb != 0u) {
      rs_scale = __uint_as_float(fb);
    } else if ((st >> (32 + rs_lp)) & 1ull) {
      rs_scale = __uint_as_float(__builtin_amdgcn_readfirstlane(
          __hip_atomic_load(&A.pstate[rs_lazy].fin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
    } else {
      rs_out = nullptr;  // handed back
    }
    rs_lazy = -1;
  };
  // A hand-back passes the interior (written by this block's plain stores, complete since
  // the piece's end) to another block on any XCD: released (L2 write-back) before the bit.
  auto hand_back = [&](int bb, int p) -> unsigned long long {  // tid 0
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    return atomicOr(&A.pstate[bb].st, 1ull << p);
  };
  auto rs_resolve_issue = [&]() {  // tid 0, before that barrier
    const uint32_t fb =
        __hip_atomic_load(&A.pstate[rs_lazy].fin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    redu[12] = fb;
    if (fb == 0u) *reinterpret_cast<unsigned long long*>(redu + 10) = hand_back(rs_lazy, rs_lp);
  };
  // the float4 groups of piece p's interior segments [p seg, (p + 1) seg - 2] (<= T - 2)
  auto piece_lo4 = [&](int p, int sg) { return p * sg * H / 4; };
  auto piece_hi4 = [&](int p, int sg, int T) { return min((p + 1) * sg - 1, T - 1) * H / 4; };
  // s_ipf: the last piece of utterance b to arrive forms its np - 1 seams (pieces' halves
  // written through to memory, read the same way) x 1 / sum w^2 -- the OLA's arithmetic --,
  // takes the utterance peak over them and the pieces' interior maxima, writes the seams
  // scaled and peak[b], publishes 1/peak and rescales the interiors handed back to it.
  auto piece_finalize = [&](int b, int T, int np, int sg, float* outb) {
    // thread-derived offsets recomputed here from an opaque tid (hoisted to the kernel start
    // they were held through the steps and spilled)
    int t = tid;
    opaque_i(t);
    const long long slot0 = (long long)(b - s_whole) * pieces;
    const float iw = inv_wsum<N>(t);  // H = kUttThreads: thread t owns sample m = t
    // seam p = tail of piece p - 1 + head of piece p, 8 seams per round trip through
    // descriptors covering the np slots; raw values to the frame slots (free at a unit's end)
    // for the scaled write. Only seams p < np enter the peak: for p = np the tail load still
    // falls inside the descriptor (slot np - 1's tail: no seam, possibly an earlier call's)
    const rsrc_t rt = make_rsrc(A.ptails + slot0 * H, (long long)np * H);
    const rsrc_t rh = make_rsrc(A.pheads + slot0 * H, (long long)np * H);
    float* stash = reinterpret_cast<float*>(lds) + t;
    // the pieces' interior maxima (RMW: after every piece's atomicMax), with the seam loads
    uint32_t pku = 0u;
    if (t == 0) pku = atomicMax(A.peak_u + b, 0u);
    float mx = 0.0f;
    for (int p0 = 1; p0 < np; p0 += 8) {
      float sv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int p = p0 + u;
        sv[u] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rt, 4 * ((p - 1) * H + t), 0, kSC1)) +
                __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rh, 4 * (p * H + t), 0, kSC1));
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (p0 + u < np) {
          sv[u] *= iw;
          mx = fmaxf(mx, fabsf(sv[u]));
          stash[(p0 + u - 1) * H] = sv[u];
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    __syncthreads();  // red[] free
    if (lane == 0) red[wave] = mx;
    if (t == 0) redu[9] = pku;
    __syncthreads();
    float pk = __uint_as_float(redu[9]);
#pragma unroll
    for (int w = 0; w < kUttThreads / 64; ++w) pk = fmaxf(pk, red[w]);
    const float scale = 1.0f / (pk + A.norm_eps);
    float* ot = outb + t;
    for (int p = 1; p < np; ++p) ot[(long long)(p * sg - 1) * H] = stash[(p - 1) * H] * scale;
    if (t == 0) {
      if (A.peak) A.peak[b] = pk;
      __hip_atomic_store(&A.pstate[b].fin, __float_as_uint(scale), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // published before the pass
      uint32_t hi;
      asm volatile("v_mov_b32 %0, -1" : "=v"(hi));  // materialised here (hoisted, it spilled)
      const unsigned long long old = atomicOr(&A.pstate[b].st, (unsigned long long)hi << 32);
      *reinterpret_cast<unsigned long long*>(redu + 10) = old;
      // interiors handed back: their owners' writes, released before their bits, acquired
      if ((uint32_t)old != 0u) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    const unsigned long long hb = *reinterpret_cast<const unsigned long long*>(redu + 10);
    for (int p = 0; p < np; ++p)
      if ((hb >> p) & 1ull) {
        rs_out = outb;
        rs_scale = scale;
        rs_done = piece_lo4(p, sg);
        rs_n4 = piece_hi4(p, sg, T);
        rescale_rest(std::integral_constant<int, 2 * RS_U>{});
      }
  };
  // Across a unit's steps only b and its last step are held (more spilled): a piece is
  // recognised by b >= s_whole, its seam slot and unit index follow from b and the frame.
  const int seg = FB * (A.s_steps > 0 ? A.s_steps : 1);  // frames per piece
  while (cu.b < A.batch) {
    const int b = cu.b;
    const int L = __builtin_amdgcn_readfirstlane(utt_len(A, b));
    const int T = (L + H - 1) / H + 1;
    rsrc_t r0, r1;
    rsrcs(b, r0, r1);
    // the next unit's first step is loaded during this unit's last step (waves >= 1 from
    // inside the FFT, wave 0 right after it) and lands during the rescale (the next unit is
    // looked up again after the loop: held across the steps it spilled)
    int nb = 0, nlen = 0, nf0 = 0;  // the next unit's utterance, length (0: none), 1st frame
    {
      const Unit t = unit_at(cu.g + gridDim.x);
      if (t.b < A.batch) {
        nb = __builtin_amdgcn_readfirstlane(t.b);
        nlen = __builtin_amdgcn_readfirstlane(utt_len(A, t.b));
        nf0 = PIECES ? __builtin_amdgcn_readfirstlane(t.s_lo * FB) : 0;
      }
    }
    // the utterance's apply coefficients into LDS (read per step, so they hold no registers
    // through the FFTs); the previous unit's readers finished at its last barrier. Every
    // piece of an utterance solves its bins too (no solve launch before the kernel).
    {
      float4* ct = reinterpret_cast<float4*>(lds + UttGeo::COEF_OFF);
      if (SOLVE) {
        if (!PIECES || !coefs_ready) solve_coefs(b, T, std::integral_constant<int, 4>{});
        coefs_ready = false;
      } else {
        const float4* coef = reinterpret_cast<const float4*>(A.coef) + (long long)b * F;
        int k0 = tid;
        opaque_i(k0);  // its address computed here (hoisted to the kernel start, it spilled)
        for (int k = k0; k < F; k += kUttThreads) ct[k] = coef[k];
      }
    }
    __syncthreads();
    AVZ_STAMP(15);
    uint32_t bits[9];
    float4 carry = make_float4(0.f, 0.f, 0.f, 0.f);
    float peak = 0.0f;
    float* outb = A.out + (long long)b * A.out_stride;
    const int s_hi = cu.s_hi, s_lo = PIECES ? cu.s_lo : 0;
    int step = s_lo;
    for (; step < s_hi; ++step) {
#ifdef AVZ_STAMPS
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      AVZ_STAMP(13);
#endif
      const int f0 = step * FB, c = f0 / kChunk;
      // lane-derived LDS / global offsets recomputed per step (held across the loop they
      // cost ~100 VGPRs and spilled)
      int ln = lane, tq = tid;
      opaque_i(ln);
      opaque_i(tq);
      if ((f0 % kChunk == 0 || (PIECES && step == s_lo)) && PF == PF_IBM_TARGET) {  // bits
        const uint32_t* MW = A.mwords + ((long long)b * A.nchunk + c) * F;
#pragma unroll
        for (int q = 0; q < 9; ++q)
          bits[q] = MW[q < 4 ? ln + 64 * q : (q < 8 ? H - ln - 64 * (q - 4) : N / 4)];
      }
      // ---- window + forward FFT of frames f0 + 2 wave + g into slot my; the next step's
      // loads go out from inside its last stage (frames >= FB: no negative sample index)
      const bool more = step + 1 < s_hi;
      const bool il = more || wave >= 1 || nf0 > 0;
      // the descriptors of the next step's loads, built from block-uniform scalars (a
      // select between two descriptors went to VGPRs: a waterfall loop around every load)
      rsrc_t q0, q1;
      {
        const int qb = __builtin_amdgcn_readfirstlane(more ? b : nb);
        const int ql = __builtin_amdgcn_readfirstlane(more ? L : nlen);
        const float* qm = A.mix + (long long)qb * A.mix_stride;
        q0 = make_rsrc(qm, ql);
        q1 = make_rsrc(qm + A.ch_stride, ql);
      }
      const int sn = ((more ? f0 + FB : nf0) + 2 * wave) * H - N / 2 + lm.in0;
      // the next step's loads go out after the apply (issued from inside the forward FFT's
      // last stage, after the FFT or after the inverse measured slower)
      // (all 24 after the apply: splitting them, the rest between the inverse's two DFT
      // stages, measured best only with the 32 loads per lane of unshared frames,
      // profiles/r05/ab_next_loads_split.txt, profiles/r05/ab_share_loads.txt)
      auto load_k = [&](auto kc) {  // register k's next sample pair (as pair_loads)
        constexpr int k = decltype(kc)::value;
        if constexpr (k < 16) {
          const int e = sn + 1024 * lm.grp + 32 * k;
          v[k].x = bload_nn(q0, e);
          v[k].y = bload_nn(q1, e);
        } else if constexpr ((k - 16) % 2 == 0) {
          const int e = sn + 512 + 32 * (k - 16) + 32 * lm.grp;
          v[k].x = bload_nn(q0, e);
          v[k].y = bload_nn(q1, e);
        }
      };
      auto next_loads = [&]() {
        if (il)
          static_for<0, 32>(load_k);
        else
          first_loads(q0, q1, 0);  // wave 0, last step: the next utterance (or empty)
      };
      pair_finish(v);
      window_fft<N>(v, wc0, fft, utt_frame(lds, my), lm);
      AVZ_STAMP(4);
      __builtin_amdgcn_wave_barrier();
      const float* irm = (PF == PF_IRM) ? A.pf_gain + ((long long)b * A.nchunk + c) * kChunk * F
                                        : nullptr;
      auto gain = [&](uint32_t bb, int i, int t, int k) -> float {  // i: frame bit in chunk
        if (t >= T) return 0.0f;
        if constexpr (PF == PF_IBM_TARGET) {
          return ((bb >> i) & 1u) ? 0.0f : 1.0f;
        } else if constexpr (PF == PF_IRM) {
          return irm[i * F + k];
        } else if constexpr (PF == PF_EXT_FLOOR || PF == PF_EXT_MUL) {
          const float M = A.ext_mask[(long long)b * A.mask_sb + (long long)k * A.mask_sf +
                                     (long long)t * A.mask_st];
          return PF == PF_EXT_FLOOR ? fmaxf(M, A.pf_floor) : M;
        } else {
          return 1.0f;
        }
      };
      // ---- apply w^H y + post-filter of the wave's frames, folded into each frame's
      // N/2-point inverse input (written in place over the bins just read):
      //   Zh[m] = A + i B, Zh[N/2 - m] = conj(A) + i conj(B),
      //   A = S[m] + conj(S[N/2 - m]),  B = e^{2 pi i m / N} (S[m] - conj(S[N/2 - m]))
      cf al[9], be[9];
      {
        const float4* ct = reinterpret_cast<const float4*>(lds + UttGeo::COEF_OFF);
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const float4 w = ct[q < 4 ? ln + 64 * q : (q < 8 ? H - ln - 64 * (q - 4) : N / 4)];
          al[q] = cf{w.x, w.y};
          be[q] = cf{w.z, w.w};
        }
      }
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const int f = 2 * wave + g, t = f0 + f, ib = f0 % kChunk + f;
        cf* Z = utt_frame(lds, f);
        cf za[4], zap[4], zb[4], zbp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int kA = ln + 64 * j, kB = H - kA;
          za[j] = lds_read(Z + kA);
          zap[j] = lds_read(Z + ((N - kA) & (N - 1)));
          zb[j] = lds_read(Z + kB);
          zbp[j] = lds_read(Z + (N - kB));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int kA = ln + 64 * j, kB = H - kA;
          cf sa = apply_bin(al[j], be[j], za[j], zap[j], gain(bits[j], ib, t, kA));
          cf sb = apply_bin(al[4 + j], be[4 + j], zb[j], zbp[j], gain(bits[4 + j], ib, t, kB));
          if (j == 0 && ln == 0) {  // DC and Nyquist: irfft keeps the real parts
            sa.y = 0.0f;
            sb.y = 0.0f;
          }
          const cf a = {sa.x + sb.x, sa.y - sb.y};
          const cf d = {sa.x - sb.x, sa.y + sb.y};
          const cf bb = c_mul(om[j], d);
          Z[kA] = {a.x - bb.y, a.y + bb.x};
          Z[kB] = {a.x + bb.y, bb.x - a.y};
        }
        if (ln == g) {  // bin N/4: Zh = 2 conj(S)
          const cf s = apply_bin(al[8], be[8], Z[N / 4], Z[3 * N / 4], gain(bits[8], ib, t, N / 4));
          Z[N / 4] = {2.0f * s.x, -2.0f * s.y};
        }
      }
      AVZ_STAMP(5);
      next_loads();
      AVZ_STAMP(6);
      __builtin_amdgcn_wave_barrier();
      // ---- inverse: lane group g transforms frame 2 wave + g; windowed contributions
      // (samples 2m, 2m + 1 as one float2) over the frame's first 4 KB, the transpose in its
      // second half
      {
        cf* Zi = utt_frame(lds, my);
        cf u[16];
        static_for<0, 16>([&](auto r) { u[r] = c_conj(lds_read(Zi + (ln & 31) + 32 * r)); });
        float2* Cp = reinterpret_cast<float2*>(Zi);
        const int mhs = (ln & 15) + 256 * ((ln >> 4) & 1);
        Fft512x2::forward_tw1024_emit(u, Zi + H, twid, ln, [&](auto k, cf x) {
          constexpr float ck = W32::c[k], sk = -W32::s[k];  // cos, sin of 2 pi (32 k) / N
          const float we = fmaf(wh_s[0], sk, fmaf(-wh_c[0], ck, 0.25f));
          const float wo = fmaf(wh_s[1], sk, fmaf(-wh_c[1], ck, 0.25f));
          Cp[mhs + 16 * k] = make_float2(x.x * we, -x.y * wo);
        });
      }
      AVZ_STAMP(7);
      lds_barrier();
      AVZ_STAMP(8);
      // ---- overlap-add: segment j = f0 - 1 + s = frame s-1 (2nd half) + frame s (1st half);
      // segment -1 (frame 0's first half) is scipy's trimmed N/2
      auto cframe = [&](int f) -> const float* {
        return reinterpret_cast<const float*>(utt_frame(lds, f));
      };
      const int m0 = 4 * (tq & 127), sgrp = __builtin_amdgcn_readfirstlane(tq >> 7);
      // a piece's first step (its first segment is a seam) and the piece's seam slot
      const bool pstart = PIECES && b >= s_whole && f0 % seg == 0;
      const long long pslot = (long long)(b - s_whole) * pieces + f0 / seg;
      auto ola = [&]() {
#pragma unroll
      for (int si = 0; si < 4; ++si) {
        const int s = sgrp + 4 * si;
        const int j = f0 - 1 + s;
        if (j >= 0 && j <= T - 2) {
          const float4 vb = *reinterpret_cast<const float4*>(cframe(s) + m0);
          if (s == 0 && pstart) {  // a piece's first segment is a seam: its half for the
            store_through(A.pheads + pslot * H, H, m0, vb);  // piece finalize
            continue;
          }
          // the previous frame's half read unconditionally (frame 0's when s = 0) and the
          // carry selected by value: a conditional read was split into four ds_read_b32
          // (4-way bank conflicts, 15 % of the kernel's LDS cycles), a pointer select with
          // &carry put carry on the stack
          const float4 vp = *reinterpret_cast<const float4*>(cframe(s == 0 ? 0 : s - 1) + H + m0);
          const float4 va = (s != 0) ? vp : carry;
          float4 o;
          o.x = (va.x + vb.x) * inv[0];
          o.y = (va.y + vb.y) * inv[1];
          o.z = (va.z + vb.z) * inv[2];
          o.w = (va.w + vb.w) * inv[3];
          *reinterpret_cast<float4*>(outb + (long long)j * H + m0) = o;
          peak = fmaxf(peak, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))));
        }
      }
      };
      if (rs_out != nullptr && rs_done < rs_n4) {  // a slice of the previous utterance's rescale
        if (PIECES && b >= s_whole) {  // a piece's few steps: larger slices
          const int lo = rs_done, hi = min(rs_n4, rs_done + RS_UP * kUttThreads);
          if (rescale_slice(std::integral_constant<int, RS_UP>{}, lo, hi, ola)) rs_done = hi;
        } else {
          const int lo = rs_done, hi = min(rs_n4, rs_done + RS_U * kUttThreads);
          if (rescale_slice(std::integral_constant<int, RS_U>{}, lo, hi, ola)) rs_done = hi;
        }
      } else {
        ola();
      }
      if (sgrp == 0) carry = *reinterpret_cast<const float4*>(cframe(FB - 1) + H + m0);
      // a piece's last half-frame (seam half): a whole utterance's last step never has a
      // segment f0 + FB - 1 <= T - 2 (its last frame is T - 1 <= f0 + FB - 1)
      if (PIECES && sgrp == 0 && !more && f0 + FB - 1 <= T - 2)
        store_through(A.ptails + pslot * H, H, m0, carry);
      AVZ_STAMP(9);
      lds_barrier();
      AVZ_STAMP(10);
    }
    // ---- utterance peak; NORM_PEAK rescales the block's own output (its stores drained
    // first; L1-bypassing loads), as avz_finalize_kernel did in a second pass over HBM
    for (int o = 32; o > 0; o >>= 1) peak = fmaxf(peak, __shfl_xor(peak, o, 64));
    if (lane == 0) red[wave] = peak;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const bool whole = !PIECES || b < s_whole;
    // s_ipf: a piece interior of this block still waiting for its 1/peak (rs_resolve)
    const bool resolve = PIECES && ipf && whole && rs_lazy >= 0;
    if (resolve && tid == 0) rs_resolve_issue();
    __syncthreads();
    float pk = red[0];
#pragma unroll
    for (int w = 1; w < kUttThreads / 64; ++w) pk = fmaxf(pk, red[w]);
    if (resolve) rs_resolve();
    if (!whole) {  // a piece: its interior's max (non-negative floats order as uints)
      if (ipf) {
        // arrival: the seam halves were written through (sc1) and drained above, the
        // atomicMax completes before the count
        if (tid == 0) {
          atomicMax(A.peak_u + b, __float_as_uint(pk));
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          redu[9] = atomicAdd(&A.pstate[b].cnt, 1u);
        }
        __syncthreads();
        const int p = (step - 1) / A.s_steps;
        const int np = min(pieces, ((T + FB - 1) / FB + A.s_steps - 1) / A.s_steps);
        const bool fin_here = __builtin_amdgcn_readfirstlane(redu[9]) == (uint32_t)(np - 1);
        if (fin_here) piece_finalize(b, T, np, seg, outb);
        // its own interior: rescaled in slices once 1/peak is published
        rs_out = outb;
        rs_lazy = b;
        rs_lp = p;
        rs_done = piece_lo4(p, seg);
        rs_n4 = piece_hi4(p, seg, T);
        if (A.dbg_ipf == 1 && !fin_here) {  // diagnostic: hand back at once (rs_resolve)
          if (tid == 0) {
            redu[12] = 0u;
            *reinterpret_cast<unsigned long long*>(redu + 10) = hand_back(b, p);
          }
          __syncthreads();
          rs_resolve();
        }
      } else if (tid == 0) {
        atomicMax(A.peak_u + b, __float_as_uint(pk));
      }
    } else if (tid == 0 && A.peak) {
      A.peak[b] = pk;
    }
    if (whole && A.normalize == NORM_PEAK) {
      // the previous one's slices left over (an utterance of < 8 steps)
      if (rs_out != nullptr) rescale_rest(std::integral_constant<int, 2 * RS_U>{});
      rs_out = outb;
      rs_scale = 1.0f / (pk + A.norm_eps);
      rs_n4 = (T - 1) * H / 4;
      rs_done = 0;
    }
    __syncthreads();  // red[] of the next unit
    AVZ_STAMP(14);
    // this unit's index (unit_at): from b (whole) or the piece's q, (step - 1) / s_steps its
    // piece
    cu = unit_at((whole ? (ipf ? b + G : b)
                        : (ipf ? 0 : s_whole) + (b - s_whole) * pieces + (step - 1) / A.s_steps) +
                 gridDim.x);
  }
  // a piece interior still lazy: every later unit of the block was skipped (device length
  // < N), so no whole utterance's end resolved it -- take 1/peak or hand it back now
  // (rescale_rest's slices assume a published scale)
  if (PIECES && ipf && rs_lazy >= 0) {
    if (tid == 0) rs_resolve_issue();
    __syncthreads();
    rs_resolve();
  }
  // the block's last utterance, after the loop where the sample registers are dead: every
  // load of a 4-s utterance in flight at once (the single-utterance blocks of B <= #CU
  // rescale here; a latency-bound loop with 8 loads in flight per thread ran ~13 us)
  if (rs_out != nullptr) rescale_rest(std::integral_constant<int, RS_BULK>{});
  AVZ_STAMP(14);
}

// The N = 512 form of avz_synthesis_utt_kernel: one 8-wave block per CU owns whole
// utterances and normalises them itself, but keeps the chunk kernel's step (synthesis_item
// at N = 512): every lane group transforms two frames (R = 2), so a step is 32 frames -- one
// IBM mask chunk -- in 32 slots of 4.3 KB (139 KB), and the 16 packed inverse pairs
// (Sa + i Sb, one complex Fft512x2 per lane group) keep all eight waves busy through the
// inverse (at N = 1024 the same packing would leave half the waves idle, hence that
// kernel's per-frame half-size inverse). Apply: thread t serves bin t & 255 for the frame
// pairs 8 (t >> 8) .. + 8. Seam carried in registers across the chunks, peak and rescale
// in-block (progressive over the next utterance's overlap-add phases), solve in-block
// (SOLVE), as the N = 1024 kernel. Reference semantics as the chunk kernel + finalize.
constexpr int kUtt512Threads = 512;
struct Utt512Geo {
  static constexpr int N = 512, H = 256, F = 257, NWAVE = 8, FPW = 2, R = 2;
  static constexpr int RSTRIDE = NWAVE * FPW;       // 16: a lane group's second frame
  static constexpr int FB = RSTRIDE * R;            // 32 frames per step
  static constexpr int NPAIR = FB / 2;              // 16 packed inverse pairs
  static constexpr int SLOT_LDS = FB * KCfg<512>::GROUP_BYTES;
  static constexpr int COEF_OFF = SLOT_LDS;         // the utterance's alpha, beta
  static constexpr int RED_OFF = COEF_OFF + F * 16;
  static constexpr int LDS_BYTES = RED_OFF + 64;
  static_assert(FB == kChunk, "a step is one mask chunk");
  static_assert(LDS_BYTES <= 160 * 1024, "one block per CU");
  static_assert(KCfg<512>::WAVE_BYTES == FPW * KCfg<512>::GROUP_BYTES, "slot_ptr layout");
};

template <int PF, bool SOLVE>
__global__ void __launch_bounds__(kUtt512Threads, 2) avz_synthesis_utt512_kernel(ChainArgs A) {
  using G = Utt512Geo;
  using C = KCfg<512>;
  constexpr int N = G::N, H = G::H, F = G::F, FB = G::FB, NPAIR = G::NPAIR, RSTRIDE = G::RSTRIDE;
  constexpr int PPL = C::PPL;
  constexpr int M4 = H / 4;                    // float4 groups per half frame
  constexpr int NSG = kUtt512Threads / M4;     // 8 segment groups (one per wave)
  constexpr int SPT = FB / NSG;                // 4 segments per thread per step
  constexpr int PPT = NPAIR / 2;               // 8 frame pairs per apply thread
  extern __shared__ __align__(16) unsigned char lds[];
  float* red = reinterpret_cast<float*>(lds + G::RED_OFF);
  float4* ct = reinterpret_cast<float4*>(lds + G::COEF_OFF);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  Fft512x2 fft;
  fft.init(lane);
  LaneMap<N> lm;
  lm.init(lane);
  const WinCoef<N> wc = [&] { WinCoef<N> w; w.init(lm); return w; }();
  const int my_slot = wave * G::FPW + lm.grp;  // frames my_slot, my_slot + 16 of the step
  const int p0 = PPT * (wave >> 2);  // apply: pairs p0 .. p0 + 7 (wave-uniform)
  const bool nyq_wave = (wave == G::NWAVE - 1);
  const int sgrp = wave;             // overlap-add: segments wave + 8 si
  static_assert(M4 == 64, "one segment group per wave");
  float inv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) inv[i] = inv_wsum<N>(4 * lane + i);
  const rsrc_t r_none = make_rsrc(nullptr, 0);
  AVZ_STAMP_DECL();
  AVZ_STAMP_INIT();

  auto next_valid = [&](int bb) {
    for (; bb < A.batch; bb += gridDim.x) {
      if (utt_len(A, bb) >= N) break;
      if (tid == 0 && A.peak) A.peak[bb] = __builtin_nanf("");
    }
    return bb;
  };
  auto rsrcs = [&](int bb, rsrc_t& a0, rsrc_t& a1) {
    bb = __builtin_amdgcn_readfirstlane(bb);
    const float* mixb = A.mix + (long long)bb * A.mix_stride;
    const int len = __builtin_amdgcn_readfirstlane(utt_len(A, bb));
    a0 = make_rsrc(mixb, len);
    a1 = make_rsrc(mixb + A.ch_stride, len);
  };
  cf v[PPL], vq[PPL];
  // frames fb + my_slot (v) and fb + my_slot + 16 (vq); a step's first wave starts N/2 before
  // sample 0 only at fb = 0 on wave 0 (range-checked offsets there)
  auto load_step = [&](rsrc_t a0, rsrc_t a1, int fb) {
    const int s0 = (fb + my_slot) * H - N / 2 + lm.in0, s1 = s0 + RSTRIDE * H;
    if (fb + wave * G::FPW >= 1) {
      static_for<0, PPL>([&](auto r) {
        v[r].x = bload_nn(a0, s0 + C::IN_STRIDE * r);
        v[r].y = bload_nn(a1, s0 + C::IN_STRIDE * r);
      });
    } else {
      static_for<0, PPL>([&](auto r) {
        v[r].x = bload(a0, s0 + C::IN_STRIDE * r);
        v[r].y = bload(a1, s0 + C::IN_STRIDE * r);
      });
    }
    static_for<0, PPL>([&](auto r) {
      vq[r].x = bload_nn(a0, s1 + C::IN_STRIDE * r);
      vq[r].y = bload_nn(a1, s1 + C::IN_STRIDE * r);
    });
  };
  int b = next_valid(blockIdx.x);
  if (b < A.batch) {
    rsrc_t a0, a1;
    rsrcs(b, a0, a1);
    load_step(a0, a1, 0);
  }
  // NORM_PEAK rescale of the block's previous utterance, one slice per overlap-add phase
  float* rs_out = nullptr;
  float rs_scale = 0.0f;
  int rs_n4 = 0, rs_done = 0;
  constexpr int RS_U = 4, RS_BULK = 32;
  auto rescale_slice = [&](auto uc, int lo, int hi, auto issue_more) {
    constexpr int U = decltype(uc)::value;
    const rsrc_t ro = make_rsrc(rs_out, 4LL * rs_n4);
    float4 x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const v4i_t d = __builtin_amdgcn_raw_buffer_load_b128(ro, 16 * (lo + u * kUtt512Threads + tid),
                                                            0, kSC1);
      x[u] = make_float4(__int_as_float(d.x), __int_as_float(d.y), __int_as_float(d.z),
                         __int_as_float(d.w));
    }
    issue_more();
    float4* o4 = reinterpret_cast<float4*>(rs_out);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = lo + u * kUtt512Threads + tid;
      if (i < hi) {
        x[u].x *= rs_scale; x[u].y *= rs_scale; x[u].z *= rs_scale; x[u].w *= rs_scale;
        o4[i] = x[u];
      }
    }
  };
  auto rescale_rest = [&](auto uc) {
    constexpr int U = decltype(uc)::value;
    for (; rs_done < rs_n4; rs_done += U * kUtt512Threads)
      rescale_slice(uc, rs_done, min(rs_n4, rs_done + U * kUtt512Threads), [] {});
    rs_out = nullptr;
  };

  while (b < A.batch) {
    const int L = utt_len(A, b);
    const int T = (L + H - 1) / H + 1;
    const int nstep = (T + FB - 1) / FB;
    rsrc_t r0, r1;
    rsrcs(b, r0, r1);
    const int nb = next_valid(b + gridDim.x);
    rsrc_t n0 = r_none, n1 = r_none;
    if (nb < A.batch) rsrcs(nb, n0, n1);
    if constexpr (SOLVE) {
      const int nch = (T + kChunk - 1) / kChunk;
      for (int k = tid; k < F; k += kUtt512Threads) {
        double R[5], w[4];
        bin_cov_sums_utt<N>(A, b, k, nch, R);
        const double* d = A.steer + 4 * k;
        mvdr_weights_d(R, k, N, A, d[0], d[1], d[2], d[3], w, nullptr);
        cf al, be;
        coef_from_w(w[0], w[1], w[2], w[3], al, be, nullptr);
        ct[k] = make_float4(al.x, al.y, be.x, be.y);
      }
    } else {
      const float4* coef = reinterpret_cast<const float4*>(A.coef) + (long long)b * F;
      for (int k = tid; k < F; k += kUtt512Threads) ct[k] = coef[k];
    }
    __syncthreads();
    AVZ_STAMP(15);
    cf alpha, beta, alpha_n{0, 0}, beta_n{0, 0};
    {
      const float4 w = ct[tid & 255];
      alpha = cf{w.x, w.y};
      beta = cf{w.z, w.w};
      if (nyq_wave) {
        const float4 wn = ct[N / 2];
        alpha_n = cf{wn.x, wn.y};
        beta_n = cf{wn.z, wn.w};
      }
    }
    float4 carry = make_float4(0.f, 0.f, 0.f, 0.f);
    float peak = 0.0f;
    float* outb = A.out + (long long)b * A.out_stride;
    for (int step = 0; step < nstep; ++step) {
      const int f0 = step * FB;
      // lane-derived offsets recomputed per step (hoisted out of the loop they are held in
      // VGPRs through the FFTs and spill)
      int tq = tid, ln = lane;
      opaque_i(tq);
      opaque_i(ln);
      const int kb = tq & 255, kp = (N - kb) & (N - 1), m0 = 4 * ln;
#ifdef AVZ_STAMPS
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      AVZ_STAMP(13);
#endif
      const uint32_t* MW = A.mwords + ((long long)b * A.nchunk + step) * F;
      const uint32_t bits = (PF == PF_IBM_TARGET) ? MW[kb] : 0u;
      const uint32_t bits_n = (PF == PF_IBM_TARGET && nyq_wave) ? MW[N / 2] : 0u;
      window_fft<N, true>(v, wc, fft, slot_ptr<N>(lds, my_slot), lm);
      window_fft<N, true>(vq, wc, fft, slot_ptr<N>(lds, my_slot + RSTRIDE), lm);
      AVZ_STAMP(4);
      lds_barrier();
      AVZ_STAMP(8);
      auto gain = [&](uint32_t bb, int i, int t) -> float {  // i: frame bit in the chunk
        if (t >= T) return 0.0f;
        if constexpr (PF == PF_IBM_TARGET) return ((bb >> i) & 1u) ? 0.0f : 1.0f;
        return 1.0f;
      };
      // ---- apply w^H y + post-filter; frames (2p, 2p + 1) packed as Sa + i Sb into slot 2p
      {
        cf za[PPT], zap[PPT], zb[PPT], zbp[PPT];
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
          const cf* Za = slot_ptr<N>(lds, 2 * (p0 + q));
          const cf* Zb = slot_ptr<N>(lds, 2 * (p0 + q) + 1);
          za[q] = lds_read(Za + kb);
          zap[q] = lds_read(Za + kp);
          zb[q] = lds_read(Zb + kb);
          zbp[q] = lds_read(Zb + kp);
        }
#pragma unroll
        for (int q = 0; q < PPT; ++q) {
          const int p = p0 + q, ta = f0 + 2 * p;
          cf* Za = slot_ptr<N>(lds, 2 * p);
          const cf sa = apply_bin(alpha, beta, za[q], zap[q], gain(bits, 2 * p, ta));
          const cf sb = apply_bin(alpha, beta, zb[q], zbp[q], gain(bits, 2 * p + 1, ta + 1));
          Za[kp] = {sa.x + sb.y, sb.x - sa.y};  // conj(Sa) + i conj(Sb) at N - k
          Za[kb] = (kb == 0) ? cf{sa.x, sb.x} : cf{sa.x - sb.y, sa.y + sb.x};
        }
      }
      if (nyq_wave && lane < NPAIR) {  // Nyquist bin: frame pair `lane`
        const int ta = f0 + 2 * lane;
        if (ta < T) {
          cf* Za = slot_ptr<N>(lds, 2 * lane);
          const cf* Zb = slot_ptr<N>(lds, 2 * lane + 1);
          const float ga = gain(bits_n, 2 * lane, ta), gb = gain(bits_n, 2 * lane + 1, ta + 1);
          const cf za = Za[N / 2], zb = Zb[N / 2];
          Za[N / 2] = {apply_bin(alpha_n, beta_n, za, za, ga).x,
                       apply_bin(alpha_n, beta_n, zb, zb, gb).x};
        }
      }
      AVZ_STAMP(5);
      lds_barrier();
      AVZ_STAMP(10);
      // ---- inverse of pair p = my_slot (every lane group): windowed contributions of
      // frames 2p (real part) and 2p + 1 (imaginary part) into slot 2p + 1
      {
        const int p = my_slot;
        cf* Zi = slot_ptr<N>(lds, 2 * p);
        cf u[PPL];
        static_for<0, PPL>([&](auto r) { u[r] = c_conj(Zi[lm.in0 + C::IN_STRIDE * r]); });
        float* Cp = reinterpret_cast<float*>(slot_ptr<N>(lds, 2 * p + 1));
        fft.forward_emit(u, Zi, [&](auto k, cf x) {
          constexpr float ck = W32::c[k], sk = -W32::s[k];  // cos, sin of 2 pi k / 32
          const float w = fmaf(wc.ss, sk, fmaf(-wc.sc, ck, wc.s0));
          const int n = lm.out0 + C::OUT_STRIDE * k;
          Cp[n] = x.x * w;
          Cp[N + n] = -x.y * w;
        });
      }
      AVZ_STAMP(7);
      // the next step's (or utterance's) loads fly through the overlap-add (issued before
      // the apply they held 64 more VGPRs through it and spilled 80-96 B; after the apply,
      // through the inverse, 0.5-0.8 us slower, profiles/r04/ab_synth_utt512.txt)
      if (step + 1 < nstep) {
        load_step(r0, r1, f0 + FB);
      } else {
        load_step(n0, n1, 0);  // empty descriptors when this is the block's last utterance
      }
      lds_barrier();
      AVZ_STAMP(9);
      // ---- overlap-add: segment j = f0 - 1 + s = frame s-1 (2nd half) + frame s (1st half)
      auto cframe = [&](int f) -> const float* {
        return reinterpret_cast<const float*>(slot_ptr<N>(lds, 2 * (f >> 1) + 1)) + (f & 1) * N;
      };
      auto ola = [&]() {
#pragma unroll
        for (int si = 0; si < SPT; ++si) {
          const int s = sgrp + si * NSG;
          const int j = f0 - 1 + s;
          if (j >= 0 && j <= T - 2) {
            const float4 vb = *reinterpret_cast<const float4*>(cframe(s) + m0);
            const float4 vp = *reinterpret_cast<const float4*>(cframe(s == 0 ? 0 : s - 1) + H + m0);
            const float4 va = (s != 0) ? vp : carry;
            float4 o;
            o.x = (va.x + vb.x) * inv[0];
            o.y = (va.y + vb.y) * inv[1];
            o.z = (va.z + vb.z) * inv[2];
            o.w = (va.w + vb.w) * inv[3];
            *reinterpret_cast<float4*>(outb + (long long)j * H + m0) = o;
            peak = fmaxf(peak, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))));
          }
        }
      };
      if (rs_out != nullptr && rs_done < rs_n4) {
        const int lo = rs_done, hi = min(rs_n4, rs_done + RS_U * kUtt512Threads);
        rescale_slice(std::integral_constant<int, RS_U>{}, lo, hi, ola);
        rs_done = hi;
      } else {
        ola();
      }
      if (sgrp == 0) carry = *reinterpret_cast<const float4*>(cframe(FB - 1) + H + m0);
      lds_barrier();
      AVZ_STAMP(11);
    }
    // ---- utterance peak; its rescale (own output, drained, L1-bypassing loads)
    for (int o = 32; o > 0; o >>= 1) peak = fmaxf(peak, __shfl_xor(peak, o, 64));
    if (lane == 0) red[wave] = peak;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float pk = red[0];
#pragma unroll
    for (int w = 1; w < G::NWAVE; ++w) pk = fmaxf(pk, red[w]);
    if (tid == 0 && A.peak) A.peak[b] = pk;
    if (A.normalize == NORM_PEAK) {
      if (rs_out != nullptr) rescale_rest(std::integral_constant<int, 2 * RS_U>{});
      rs_out = outb;
      rs_scale = 1.0f / (pk + A.norm_eps);
      rs_n4 = (T - 1) * H / 4;
      rs_done = 0;
    }
    __syncthreads();  // red[] and the coefficient table of the next utterance
    AVZ_STAMP(14);
    b = nb;
  }
  if (rs_out != nullptr) rescale_rest(std::integral_constant<int, RS_BULK>{});
  AVZ_STAMP(14);
}
}  // namespace avz
