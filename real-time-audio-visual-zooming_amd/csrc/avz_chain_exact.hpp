// avz_chain_exact.hpp — the exact-IBM path of the analysis kernel (avz_chunked_k.hpp):
// reference-exact decisions of the frames the fp32 certificate deferred, after the block's
// loop. LDS map and frame slots (XLds, XSlot), a round of fp64 transforms (exact_round),
// frames with few uncertain bins (exact_sparse), a block's own units (exact_unit), published
// units shared over the grid (XPieces, exact_piece, exact_claim); driver: ibm_exact_units.
// Needs: avz_chain_common.hpp, avz_ibm_exact.hpp (the fp64 transforms and tables).
#pragma once
#include "avz_chain_common.hpp"
#include "avz_ibm_exact.hpp"

namespace avz {
// Exact-phase LDS layout (after the persistent loop; nothing of the loop's is live): the
// waves' fp64 transform buffers, then (same bytes, after a barrier) the round's mic spectra in
// frame slots 0-3; the round's reference magnitudes; the fp64 twiddle table. The fp32
// twiddle table (TW_OFF, the mic transforms') is kept.
// The round's frames packed one per byte (0xff: none): frame i, or -1, for a block- or
// lane-varying i by shifts (an int array indexed so went to scratch memory, selects included)
__device__ __forceinline__ int pick(uint32_t packed, int i) {
  return (int)(signed char)(packed >> (8 * i));
}
template <int N>
struct XLds {
  using C = KCfg<N>;
  using X = XGeo<N>;
  static constexpr int FR = 4;                              // frames per round
  static constexpr int MP = N / 2 + 4;                      // magnitude row (16-B aligned)
  static constexpr int MIC_BYTES = FR / C::FPW * C::WAVE_BYTES;
  static constexpr int MAG_OFF = (4 * X::SCRATCH > MIC_BYTES) ? 4 * X::SCRATCH : MIC_BYTES;
  static constexpr int TWL_OFF = MAG_OFF + 2 * FR * MP * 4;
  static constexpr int WIN_OFF = TWL_OFF + (N / 2) * 16;    // fp32 window [N]
  static constexpr int SLOT_OFF = WIN_OFF + N * 4;           // XSlot[FR], the round's frames
  static constexpr int SCAN_OFF = SLOT_OFF + FR * 32;       // int[256]: exact_sparse's items
                                                            // (between pieces: exact_claim's
                                                            // 64 candidates)
  static constexpr int SCAN_INTS = 256;
  static constexpr int WL = 32;                             // frames one block decides
  static constexpr int WL_OFF = SCAN_OFF + 256 * 4;         // int4[WL]: (unit, f, e, -)
  static constexpr int CTL_OFF = WL_OFF + WL * 16;          // int[8]: counts, mode
  static constexpr int END = CTL_OFF + 32;
  static_assert(C::FPW == 2 && END <= CGeo<N>::SLOT_LDS, "exact phase LDS");
};

// One deferred frame of the exact path (block-uniform, in LDS): analysis unit, chunk frame f,
// (e: unused), utterance b and length L, chunk c,
// flags bit 0: the frame deferred whole (reference-bit path), bit 1: its Nyquist bin deferred.
struct XSlot {
  int unit, f, e, b, L, c, flags, pad;
};
// slot g's fields as block-uniform scalars (read from LDS they are VGPRs to the compiler: the
// descriptors built from them put every buffer load in a waterfall loop)
__device__ __forceinline__ XSlot slot_u(const XSlot* sl, int g) {
  const XSlot v = sl[g];
  XSlot s;
  s.unit = __builtin_amdgcn_readfirstlane(v.unit);
  s.f = __builtin_amdgcn_readfirstlane(v.f);
  s.e = 0;
  s.b = __builtin_amdgcn_readfirstlane(v.b);
  s.L = __builtin_amdgcn_readfirstlane(v.L);
  s.c = __builtin_amdgcn_readfirstlane(v.c);
  s.flags = __builtin_amdgcn_readfirstlane(v.flags);
  s.pad = 0;
  return s;
}

// Reference-exact decisions of up to four deferred frames of one unit (avz_ibm_exact.hpp): wave w forms
// the fp64 spectra (ref_spectrum_exact) of reference w & 1 (target / interference) of slots
// w / 2 and w / 2 + 2 -- sample loads first --, waves 0-1 the slots' mic spectra, then thread
// per bin decides |I| > |T| for the slot's deferred bins (the whole frame below N/2, or the
// bins of xdfr[unit][k]; the Nyquist bin when flagged) and adds the frame's covariance terms
// and noise bit to the caller's running sums, in slot (= frame) order.
// After the loop, not in it: inlined at the item's end the step loop's kernels (248-253 of
// 256 VGPRs) spilled 105+ VGPRs; here nothing of the loop is live.
template <int N, bool PER_BIN>
__device__ __forceinline__ void exact_round(KArgs& A, unsigned char* lds, const XSlot* sl, int ns,
                                            Acc32 (&pacc)[CGeo<N>::BPT + 1],
                                            uint32_t (&pbits)[CGeo<N>::BPT + 1]) {
  using C = KCfg<N>;
  using G = CGeo<N>;
  using X = XGeo<N>;
  using XL = XLds<N>;
  constexpr int NT = G::NT, H = G::H, F = G::F, BPT = G::BPT, PPL = C::PPL, MP = XL::MP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* const mag = reinterpret_cast<float*>(lds + XL::MAG_OFF);  // [2 FR][MP]
  const cd* const twl = reinterpret_cast<const cd*>(lds + XL::TWL_OFF);
  const float* const win = reinterpret_cast<const float*>(lds + XL::WIN_OFF);
  cd* const buf = reinterpret_cast<cd*>(lds + wave * X::SCRATCH);
  AVZ_STAMP_DECL();
  AVZ_STAMP_INIT();
  AVZ_XT_LAP_BEGIN(xr_prev);  // diagnostic: phase ticks of the rounds (tools/xtrace.py)
  // lane-derived addresses formed here (hoisted out of the caller's loop they spilled)
  int lane_o = lane;
  opaque_i(lane_o);
  // the wave's two reference frames and (waves 0-1) the mic frames, loads first
  const int ga = wave >> 1, gb = (wave >> 1) + 2;
  const float* const refp = (wave & 1) ? A.ref_int : A.ref_tgt;
  float xa[N / 64], xb[N / 64];
  if (ga < ns) {
    const XSlot s = slot_u(sl, ga);
    ref_frame_load<N>(make_rsrc(refp + (long long)s.b * A.ref_stride, s.L),
                      (s.c * kChunk + s.f) * H - N / 2, lane_o, xa);
  }
  if (gb < ns) {
    const XSlot s = slot_u(sl, gb);
    ref_frame_load<N>(make_rsrc(refp + (long long)s.b * A.ref_stride, s.L),
                      (s.c * kChunk + s.f) * H - N / 2, lane_o, xb);
  }
  if (ga < ns) ref_spectrum_exact<N>(xa, twl, win, buf, mag + (2 * ga + (wave & 1)) * MP, lane_o);
  AVZ_STAMP(4);
  AVZ_XT_LAP(8, xr_prev);
  // waves 0-1: the mic frames' loads (one slot per lane group), in flight through the second
  // transform
  cf v[PPL];
  LaneMap<N> lm;
  lm.init(lane_o);
  const int gm = C::FPW * wave + lm.grp;
  if (wave < XL::FR / C::FPW) {
    // the round's slots are frames of one unit (one utterance): one descriptor pair, the
    // lane group's frame in the offset
    const XSlot s = slot_u(sl, 0);
    const float* mixb = A.mix + (long long)s.b * A.mix_stride;
    const rsrc_t r_m0 = make_rsrc(mixb, s.L), r_m1 = make_rsrc(mixb + A.ch_stride, s.L);
    const bool on = gm < ns;
    const int fm = sl[on ? gm : 0].f;
    const int s0 = (s.c * kChunk + fm) * H - N / 2 + lm.in0;
#pragma unroll
    for (int r = 0; r < PPL; ++r) {
      v[r].x = on ? bload(r_m0, s0 + C::IN_STRIDE * r) : 0.0f;
      v[r].y = on ? bload(r_m1, s0 + C::IN_STRIDE * r) : 0.0f;
    }
  }
  if (gb < ns) {
    int lane_b = lane;
    opaque_i(lane_b);
    ref_spectrum_exact<N>(xb, twl, win, buf, mag + (2 * gb + (wave & 1)) * MP, lane_b);
  }
  AVZ_STAMP(5);
  lds_barrier();  // the transform buffers are the mic spectra's slots
  AVZ_STAMP(6);
  AVZ_XT_LAP(9, xr_prev);
  if (wave < XL::FR / C::FPW) {  // the mic spectra (zeros for an absent slot)
    WinCoef<N> wc;
    wc.init(lm);
    cf* const spec = slot_ptr<N>(lds, gm);
    if constexpr (N == 1024) {
      // the unrotated frame on the LDS twiddle table: the step's register twiddles (and the
      // pair loads' rotation) stay out of this phase, whose registers they would hold
      Fft1024x2 f;
      f.l = lm.out0;
      window_apply(v, wc.a0, wc.ac, wc.as);
      f.forward(v, spec, reinterpret_cast<const cf*>(lds + G::TW_OFF));
      static_for<0, 32>([&](auto k) { spec[lm.out0 + 32 * k] = v[k]; });
    } else {
      Fft512x2 f;
      f.init(lane_o);
      window_fft<N>(v, wc, f, spec, lm);
    }
  }
  AVZ_STAMP(7);
  lds_barrier();
  AVZ_STAMP(8);
  AVZ_XT_LAP(10, xr_prev);
  // decisions |I| > |T| and the frames' covariance terms, thread per bin as the step's,
  // onto the caller's running sums (one unit's frames, in frame order)
  unsigned long long n_exact = 0;
  for (int g = 0; g < ns; ++g) {  // block-uniform
    const XSlot s = slot_u(sl, g);
    const cf* Zm = slot_ptr<N>(lds, g);
    auto put = [&](int j, int k, const Acc32& a, bool dfr, bool noise) {
      if (dfr) {
        pacc[j].c00 += a.c00;
        pacc[j].c11 += a.c11;
        pacc[j].c01r += a.c01r;
        pacc[j].c01i += a.c01i;
        pacc[j].cm += a.cm;
        pbits[j] |= (noise ? 1u : 0u) << s.f;
      }
    };
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
      const int kb = tid + j * NT;
      const int kp = (N - kb) & (N - 1);
      // the reference-bit path: the frame's xunc words (written this launch only for frames
      // flagged by the reference waves, flags bit 0; a frame deferred for its Nyquist bin
      // alone has none)
      const bool dfr =
          PER_BIN ? ((A.xdfr[(long long)s.unit * F + kb] >> s.f) & 1u)
                  : ((s.flags & 1) &&
                     ((A.xunc[((long long)s.unit * kChunk + s.f) * 32 + (kb & 31)] >> (kb >> 5)) & 1u));
      Acc32 a;
      a.zero();
      bool noise = false;
      if (dfr) {
        noise = mag[(2 * g + 1) * MP + kb] > mag[(2 * g) * MP + kb];
        cf x0, x1;
        split_pair2(Zm[kb], Zm[kp], x0, x1);
        a.add_sel(x0, x1, noise);
        a.cm = noise ? 1.0f : 0.0f;
        n_exact += 1;
      }
      put(j, kb, a, dfr, noise);
    }
    if (tid == NT - 1) {  // the Nyquist bin
      const bool dfr = (s.flags >> 1) & 1;
      Acc32 a;
      a.zero();
      bool noise = false;
      if (dfr) {
        noise = mag[(2 * g + 1) * MP + N / 2] > mag[(2 * g) * MP + N / 2];
        cf y0, y1;
        split_pair2(Zm[N / 2], Zm[N / 2], y0, y1);
        const float wn = noise ? 1.0f : 0.0f;
        a.add(y0, y1, wn, wn);
        n_exact += 1;
      }
      put(BPT, N / 2, a, dfr, noise);
    }
  }
  if (A.xstat && n_exact) atomicAdd(A.xstat + 1, n_exact);  // diagnostic: decisions
  AVZ_STAMP(9);
  lds_barrier();
  AVZ_STAMP(10);
  AVZ_XT_LAP(11, xr_prev);
}

// A deferred frame with at most kSparseMax uncertain bins (the Nyquist bin included) is decided
// bin by bin (exact_sparse); the reference-bit path's analysis items mark frames with
// kSparseMax or more uncertain bins as "round" frames (fp64 transforms, exact_round) and
// publish a unit with any for the whole grid to share (ibm_exact_units).
constexpr int kSparseMax = 12;

// Work sharing of the exact path (reference-bit path). A published unit's pieces: its sparse
// frames (if any), then its rounds of kXRound round frames in up to kXPieces - 1 groups (two
// frames a round: one fp64 transform per wave, the round's latency about halved against four).
// xst[u] = {state, arrivals}: state kXOpen | pieces << 16 | next piece while open; claims add
// 1 (a claim past the last piece, or after the reset, finds no piece: harmless; the word stays
// closed, without kXOpen, and the next publish overwrites it); the piece that completes a unit
// resets it to 0. xhint: one bit per published unit, cleared with the reset.
constexpr uint32_t kXOpen = 0x80000000u;
constexpr int kXRound = 2;
struct XPieces {
  uint32_t sp;           // sparse frames
  int n_sp, nr, npr, n;  // sparse pieces (0 / 1), rounds, round pieces, pieces
};
__device__ __forceinline__ XPieces x_pieces(uint32_t pend, uint32_t big) {
  XPieces q;
  q.sp = pend & ~big;
  q.n_sp = q.sp ? 1 : 0;
  q.nr = (__popc(big) + kXRound - 1) / kXRound;
  q.npr = min(q.nr, kXPieces - q.n_sp);
  q.n = q.n_sp + q.npr;
  return q;
}
__device__ __forceinline__ bool x_has_piece(uint32_t v) {
  return (v & kXOpen) && (v & 0xffffu) < ((v >> 16) & 0xffu);
}

// Sparse form of the exact path (reference-bit path): frames with few uncertain bins decide
// them one by one -- per item (frame f, bin k) the fp64 DFT of both references at k (rounded
// to complex64, numpy's |.|: ref_spectrum_exact's arithmetic) and of the packed mic pair at k
// and N - k (scaled as the analysis transform, rounded to fp32, split as the step's), one wave
// per item over the frame's 1024 samples, reduced across the wave. items[]: LDS, f << 16 | k,
// in frame order; the results go through LDS (res, 6 floats per item) to the bins' threads,
// which add them to their running sums in item order.
template <int N>
__device__ __forceinline__ void exact_sparse(KArgs& A, unsigned char* lds, int b, int L, int c,
                                             const int* items, int n,
                                             Acc32 (&pacc)[CGeo<N>::BPT + 1],
                                             uint32_t (&pbits)[CGeo<N>::BPT + 1]) {
  using G = CGeo<N>;
  using XL = XLds<N>;
  constexpr int H = N / 2, NT = G::NT, BPT = G::BPT;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const cd* const twl = reinterpret_cast<const cd*>(lds + XL::TWL_OFF);
  const float* const win = reinterpret_cast<const float*>(lds + XL::WIN_OFF);
  float* const res = reinterpret_cast<float*>(lds);  // [n][6] (the mic-spectra slots: free)
  const rsrc_t rt = make_rsrc(A.ref_tgt + (long long)b * A.ref_stride, L);
  const rsrc_t ri = make_rsrc(A.ref_int + (long long)b * A.ref_stride, L);
  const float* mixb = A.mix + (long long)b * A.mix_stride;
  const rsrc_t rm0 = make_rsrc(mixb, L), rm1 = make_rsrc(mixb + A.ch_stride, L);
  for (int it = wave; it < n; it += NT / 64) {  // wave-uniform
    const int item = __builtin_amdgcn_readfirstlane(items[it]);
    const int f = item >> 16, k = item & 0xffff;
    const int s0 = (c * kChunk + f) * H - N / 2;
    // every sample load in flight at once (a round trip per few samples ran ~6 us per item)
    float st[N / 64], si[N / 64], sm0[N / 64], sm1[N / 64];
#pragma unroll
    for (int r = 0; r < N / 64; ++r) {
      const int m = lane + 64 * r;
      st[r] = bload(rt, s0 + m);
      si[r] = bload(ri, s0 + m);
      sm0[r] = bload(rm0, s0 + m);
      sm1[r] = bload(rm1, s0 + m);
    }
    double tr = 0.0, ti = 0.0, ir = 0.0, ii = 0.0, ac = 0.0, bs = 0.0, as = 0.0, bc = 0.0;
#pragma unroll
    for (int r = 0; r < N / 64; ++r) {
      const int m = lane + 64 * r;
      const double w = (double)win[m];
      const double xt = w * (double)st[r], xi = w * (double)si[r];
      const double a = w * (double)sm0[r], bb = w * (double)sm1[r];
      const cd tw = xtw_at<N>(twl, (k * m) & (N - 1));  // exp(-2 pi i k m / N)
      tr = fma(xt, tw.x, tr);
      ti = fma(xt, tw.y, ti);
      ir = fma(xi, tw.x, ir);
      ii = fma(xi, tw.y, ii);
      ac = fma(a, tw.x, ac);
      bs = fma(bb, tw.y, bs);
      as = fma(a, tw.y, as);
      bc = fma(bb, tw.x, bc);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      tr += __shfl_xor(tr, o, 64);
      ti += __shfl_xor(ti, o, 64);
      ir += __shfl_xor(ir, o, 64);
      ii += __shfl_xor(ii, o, 64);
      ac += __shfl_xor(ac, o, 64);
      bs += __shfl_xor(bs, o, 64);
      as += __shfl_xor(as, o, 64);
      bc += __shfl_xor(bc, o, 64);
    }
    if (lane == 0) {
      const bool noise = np_abs_c64((float)ir, (float)ii) > np_abs_c64((float)tr, (float)ti);
      constexpr double sc = 2.0 / N;  // the analysis transform's scale ((2/N) Hann window)
      const cf zk = {(float)(sc * (ac - bs)), (float)(sc * (as + bc))};   // Z[k]
      const cf zp = {(float)(sc * (ac + bs)), (float)(sc * (bc - as))};   // Z[N - k]
      Acc32 t;
      t.zero();
      cf x0, x1;
      split_pair2(zk, zp, x0, x1);
      if (k == N / 2) {
        const float wn = noise ? 1.0f : 0.0f;
        t.add(x0, x1, wn, wn);
      } else {
        t.add_sel(x0, x1, noise);
        t.cm = noise ? 1.0f : 0.0f;
      }
      float* q = res + 6 * it;
      q[0] = noise ? 1.0f : 0.0f;
      q[1] = t.c00;
      q[2] = t.c11;
      q[3] = t.c01r;
      q[4] = t.c01i;
      q[5] = t.cm;
    }
  }
  __syncthreads();
  for (int it = 0; it < n; ++it) {  // block-uniform, item (frame) order
    const int item = items[it];
    const int f = item >> 16, k = item & 0xffff;
    const int j = k == N / 2 ? BPT : k / NT;
    if (k == N / 2 ? tid == NT - 1 : (k % NT) == tid) {
      const float* q = res + 6 * it;
#pragma unroll
      for (int jj = 0; jj <= BPT; ++jj) {  // a constant index (indexed, the array went to scratch)
        if (jj != j) continue;
        pacc[jj].c00 += q[1];
        pacc[jj].c11 += q[2];
        pacc[jj].c01r += q[3];
        pacc[jj].c01i += q[4];
        pacc[jj].cm += q[5];
        pbits[jj] |= (q[0] != 0.0f ? 1u : 0u) << f;
      }
    }
  }
  if (A.xstat && tid == 0) atomicAdd(A.xstat + 1, (unsigned long long)n);  // diagnostic
  __syncthreads();
}

// The slot of frame f of unit u (one thread): the unit's item, its length, the frame's flags.
template <int N, bool PER_BIN, class CA>
__device__ __forceinline__ void exact_set_slot(CA& A, XSlot* sl, int g, int u, int f, int gx,
                                               int n_items, int n_whole, int P) {
  constexpr int F = N / 2 + 1;
  XSlot s;
  s.unit = u;
  s.f = f;
  s.e = -1;
  unit_item<F>(A, u, gx, n_items, n_whole, P, s.b, s.c);
  s.L = utt_len(A, s.b);
  const uint4 r = reinterpret_cast<const uint4*>(A.xpend)[u];
  s.flags = (PER_BIN ? 0 : (int)((r.y >> f) & 1u)) | (int)(((r.z >> f) & 1u) << 1);
  s.pad = 0;
  sl[g] = s;
}

// Reference-exact decisions of analysis unit u's deferred frames (record xpend[u]: frames with
// a deferral, frames with uncertain-bin words xunc[u][f] (reference-bit path), the Nyquist
// bin's deferrals; xdfr[u][k] the per-bin
// deferrals of the kernels without the reference-bit hand-off), rounds of up to four frames
// in frame order (exact_round): the unit's partials of the thread's bins (kb = tid + j NT;
// the Nyquist bin: the last thread) as running sums, + each frame's terms in frame order,
// stored once; the noise bits OR-ed into the chunk's mask words (pieces of the chunk on other
// blocks own the other bits). The block must have the exact phase's LDS tables (xtab_fill)
// and the fp32 twiddle table (TW_OFF).
template <int N, bool PER_BIN>
__device__ __forceinline__ void exact_unit(KArgs& A, unsigned char* lds, int u, int gx, int n_items,
                                           int n_whole, int P) {
  using G = CGeo<N>;
  using XL = XLds<N>;
  constexpr int F = N / 2 + 1, NT = G::NT, BPT = G::BPT, FR = XL::FR;
  const int tid = threadIdx.x;
  XSlot* const sl = reinterpret_cast<XSlot*>(lds + XL::SLOT_OFF);
  const uint4 rec = reinterpret_cast<const uint4*>(A.xpend)[u];  // block-uniform
  const uint32_t pend = rec.x;
  if (pend == 0u || rec.w != 0u) return;  // published: ibm_exact_units' sharing
  int b, c;
  float* const Pt = unit_item<F>(A, u, gx, n_items, n_whole, P, b, c);
  if (A.xstat && tid == 0) atomicAdd(A.xstat, (unsigned long long)__popc(pend));
  Acc32 pacc[BPT + 1];
  uint32_t pbits[BPT + 1];
#pragma unroll
  for (int j = 0; j <= BPT; ++j) {
    const int kk = j < BPT ? tid + j * NT : N / 2;
    pbits[j] = 0u;
    if (j < BPT || tid == NT - 1) {
      pacc[j].c00 = Pt[0 * F + kk];
      pacc[j].c11 = Pt[1 * F + kk];
      pacc[j].c01r = Pt[2 * F + kk];
      pacc[j].c01i = Pt[3 * F + kk];
      pacc[j].cm = Pt[4 * F + kk];
    } else {
      pacc[j].zero();
    }
  }
  uint32_t rest = pend;
  if constexpr (!PER_BIN) {
    // frames with at most kSparseMax uncertain bins (the Nyquist bin included): their items in
    // frame order (wave 0, one frame at a time), decided one by one (exact_sparse)
    int* const items = reinterpret_cast<int*>(lds + XL::SCAN_OFF);  // [32 kSparseMax / 2]
    int* const ctl = reinterpret_cast<int*>(lds + XL::CTL_OFF);
    // the pending frames' words in LDS first (one round trip; per frame it was one each)
    uint32_t* const wsm = reinterpret_cast<uint32_t*>(lds + 16384);  // [32][32] (slots: free)
    const uint32_t has_words = reinterpret_cast<const uint4*>(A.xpend)[u].y;  // see exact_round
#pragma unroll
    for (int i = 0; i < kChunk / (G::NT / 32); ++i) {
      const int f = (tid >> 5) + (G::NT / 32) * i;
      if ((pend >> f) & 1u)
        wsm[f * 32 + (tid & 31)] =
            ((has_words >> f) & 1u) ? A.xunc[((long long)u * kChunk + f) * 32 + (tid & 31)] : 0u;
    }
    __syncthreads();
    if (tid < 64) {
      const uint32_t nyq = reinterpret_cast<const uint4*>(A.xpend)[u].z;
      int base = 0;
      uint32_t sparse = 0u;
      for (uint32_t todo = pend; todo != 0u; todo &= todo - 1u) {  // wave-uniform
        const int f = __builtin_ctz(todo);
        const uint32_t w = tid < 32 ? wsm[f * 32 + tid] : 0u;
        int inc = __popc(w);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
          const int y = __shfl_up(inc, o, 64);
          if ((tid & 63) >= o) inc += y;
        }
        const int tot = __shfl(inc, 31, 64), ny = (nyq >> f) & 1u;
        if (tot + ny <= kSparseMax && base + tot + ny <= XL::SCAN_INTS) {
          int at = base + inc - __popc(w);
          for (uint32_t x = w; x != 0u; x &= x - 1u) items[at++] = (f << 16) | (tid + 32 * __builtin_ctz(x));
          if (ny && tid == 0) items[base + tot] = (f << 16) | (N / 2);
          base += tot + ny;
          sparse |= 1u << f;
        }
      }
      if (tid == 0) {
        ctl[0] = base;
        ctl[1] = (int)sparse;
      }
    }
    __syncthreads();
    const int n_sp = ctl[0];
    rest &= ~(uint32_t)ctl[1];
    if (n_sp > 0) exact_sparse<N>(A, lds, b, utt_len(A, b), c, items, n_sp, pacc, pbits);
  }
  while (rest != 0u) {  // block-uniform
    if (tid < FR) {
      uint32_t x = rest;
      for (int i = 0; i < tid && x; ++i) x &= x - 1u;
      if (x) exact_set_slot<N, PER_BIN>(A, sl, tid, u, __builtin_ctz(x), gx, n_items, n_whole, P);
    }
    const int ns = min(FR, __popc(rest));
    for (int i = 0; i < ns; ++i) rest &= rest - 1u;
    __syncthreads();
    exact_round<N, PER_BIN>(A, lds, sl, ns, pacc, pbits);
  }
  uint32_t* const MW = A.mwords + ((long long)b * A.nchunk + c) * F;
#pragma unroll
  for (int j = 0; j <= BPT; ++j) {
    const int kk = j < BPT ? tid + j * NT : N / 2;
    if (j < BPT || tid == NT - 1) {
      Pt[0 * F + kk] = pacc[j].c00;
      Pt[1 * F + kk] = pacc[j].c11;
      Pt[2 * F + kk] = pacc[j].c01r;
      Pt[3 * F + kk] = pacc[j].c01i;
      Pt[4 * F + kk] = pacc[j].cm;
      if (pbits[j]) atomicOr(MW + kk, pbits[j]);
    }
  }
}

// The given sparse frames of unit u (reference-bit path), in frame order, in batches of at
// most XLds::SCAN_INTS (bin, frame) items (exact_sparse) onto the running sums.
template <int N>
__device__ __forceinline__ void exact_sparse_frames(KArgs& A, unsigned char* lds, int u, int b,
                                                    int c, uint32_t frames,
                                                    Acc32 (&pacc)[CGeo<N>::BPT + 1],
                                                    uint32_t (&pbits)[CGeo<N>::BPT + 1]) {
  using G = CGeo<N>;
  using XL = XLds<N>;
  const int tid = threadIdx.x;
  int* const items = reinterpret_cast<int*>(lds + XL::SCAN_OFF);
  int* const ctl = reinterpret_cast<int*>(lds + XL::CTL_OFF);
  uint32_t* const wsm = reinterpret_cast<uint32_t*>(lds + 16384);  // [32][32] (slots: free)
  const uint4 rec = reinterpret_cast<const uint4*>(A.xpend)[u];
#pragma unroll
  for (int i = 0; i < kChunk / (G::NT / 32); ++i) {
    const int f = (tid >> 5) + (G::NT / 32) * i;
    if ((frames >> f) & 1u)
      wsm[f * 32 + (tid & 31)] =
          ((rec.y >> f) & 1u) ? A.xunc[((long long)u * kChunk + f) * 32 + (tid & 31)] : 0u;
  }
  __syncthreads();
  uint32_t todo = frames;
  while (todo != 0u) {  // block-uniform
    if (tid < 64) {
      int base = 0;
      uint32_t took = 0u;
      for (uint32_t t = todo; t != 0u; t &= t - 1u) {  // wave-uniform
        const int f = __builtin_ctz(t);
        const uint32_t w = tid < 32 ? wsm[f * 32 + tid] : 0u;
        int inc = __popc(w);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
          const int y = __shfl_up(inc, o, 64);
          if ((tid & 63) >= o) inc += y;
        }
        const int tot = __shfl(inc, 31, 64), ny = (rec.z >> f) & 1u;
        if (base + tot + ny > XL::SCAN_INTS) break;
        int at = base + inc - __popc(w);
        for (uint32_t x = w; x != 0u; x &= x - 1u) items[at++] = (f << 16) | (tid + 32 * __builtin_ctz(x));
        if (ny && tid == 0) items[base + tot] = (f << 16) | (N / 2);
        base += tot + ny;
        took |= 1u << f;
      }
      if (tid == 0) {
        ctl[0] = base;
        ctl[1] = (int)took;
      }
    }
    __syncthreads();
    const int n = ctl[0];
    todo &= ~(uint32_t)ctl[1];
    exact_sparse<N>(A, lds, b, utt_len(A, b), c, items, n, pacc, pbits);  // ends on a barrier
  }
}

// Piece p of published unit u (XPieces): its terms summed from zero, the noise bits OR-ed into
// the chunk's mask words; with one piece added to the unit's partials at once, otherwise
// stored (xres[u][p]) and, by the piece that completes the unit (arrivals xst[u].y, agent-scope
// release / acquire), added to the partials in piece order -- the same sums whichever blocks
// ran the pieces. The unit's state is reset to 0 when it is complete.
template <int N, bool PER_BIN>
__device__ __forceinline__ void exact_piece(KArgs& A, unsigned char* lds, int u, int p, int gx,
                                            int n_items, int n_whole, int P) {
  using G = CGeo<N>;
  using XL = XLds<N>;
  constexpr int F = N / 2 + 1, NT = G::NT, BPT = G::BPT, FR = XL::FR;
  const int tid = threadIdx.x;
  XSlot* const sl = reinterpret_cast<XSlot*>(lds + XL::SLOT_OFF);
  int* const ctl = reinterpret_cast<int*>(lds + XL::CTL_OFF);
  const uint4 rec = reinterpret_cast<const uint4*>(A.xpend)[u];  // block-uniform
  const XPieces q = x_pieces(rec.x, rec.w);
  int b, c;
  float* const Pt = unit_item<F>(A, u, gx, n_items, n_whole, P, b, c);
  Acc32 pacc[BPT + 1];
  uint32_t pbits[BPT + 1];
#pragma unroll
  for (int j = 0; j <= BPT; ++j) {
    pacc[j].zero();
    pbits[j] = 0u;
  }
  if (p < q.n_sp) {
    if (A.xstat && tid == 0) atomicAdd(A.xstat, (unsigned long long)__popc(q.sp));  // diagnostic
    if constexpr (!PER_BIN) exact_sparse_frames<N>(A, lds, u, b, c, q.sp, pacc, pbits);
  } else {
    constexpr int R = kXRound;
    static_assert(R <= FR, "round frames");
    const int g = p - q.n_sp, r0 = g * q.nr / q.npr, r1 = (g + 1) * q.nr / q.npr;
    if (A.xstat && tid == 0)  // diagnostic: the piece's frames
      atomicAdd(A.xstat, (unsigned long long)(min(R * r1, __popc(rec.w)) - R * r0));
    const int L = utt_len(A, b);
    uint32_t rest = rec.w;
    for (int i = 0; i < r0 * R; ++i) rest &= rest - 1u;
    for (int r = r0; r < r1; ++r) {  // block-uniform
      if (tid < R) {  // the round's slots from the record (no per-slot global reads)
        uint32_t x = rest;
        for (int i = 0; i < tid && x; ++i) x &= x - 1u;
        if (x) {
          const int f = __builtin_ctz(x);
          XSlot s;
          s.unit = u;
          s.f = f;
          s.e = -1;
          s.b = b;
          s.L = L;
          s.c = c;
          s.flags = (PER_BIN ? 0 : (int)((rec.y >> f) & 1u)) | (int)(((rec.z >> f) & 1u) << 1);
          s.pad = 0;
          sl[tid] = s;
        }
      }
      const int ns = min(R, __popc(rest));
      for (int i = 0; i < ns; ++i) rest &= rest - 1u;
      __syncthreads();
      exact_round<N, PER_BIN>(A, lds, sl, ns, pacc, pbits);
    }
  }
  uint32_t* const MW = A.mwords + ((long long)b * A.nchunk + c) * F;
  float* const R = A.xres + ((long long)u * kXPieces + p) * 5 * F;
#pragma unroll
  for (int j = 0; j <= BPT; ++j) {
    const int kk = j < BPT ? tid + j * NT : N / 2;
    if (j < BPT || tid == NT - 1) {
      if (pbits[j]) atomicOr(MW + kk, pbits[j]);
      if (q.n == 1) {
        Pt[0 * F + kk] = Pt[0 * F + kk] + pacc[j].c00;
        Pt[1 * F + kk] = Pt[1 * F + kk] + pacc[j].c11;
        Pt[2 * F + kk] = Pt[2 * F + kk] + pacc[j].c01r;
        Pt[3 * F + kk] = Pt[3 * F + kk] + pacc[j].c01i;
        Pt[4 * F + kk] = Pt[4 * F + kk] + pacc[j].cm;
      } else {
        R[0 * F + kk] = pacc[j].c00;
        R[1 * F + kk] = pacc[j].c11;
        R[2 * F + kk] = pacc[j].c01r;
        R[3 * F + kk] = pacc[j].c01i;
        R[4 * F + kk] = pacc[j].cm;
      }
    }
  }
#ifdef AVZ_XTRACE
  const unsigned long long tf = __builtin_amdgcn_s_memrealtime();
#endif
  __syncthreads();
  if (tid == 0) {
    bool last = true;
    if (q.n > 1) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      const uint32_t arrived =
          __hip_atomic_fetch_add(A.xst + 2 * u + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
      last = arrived == (uint32_t)q.n;
      if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    ctl[4] = last ? 1 : 0;
  }
  __syncthreads();
#ifdef AVZ_XTRACE
  const unsigned long long tm = __builtin_amdgcn_s_memrealtime();
  if (tid == 0 && g_stamps) g_stamps[blockIdx.x * 16 + 6] += tm - tf;
#endif
  if (ctl[4]) {  // block-uniform: the unit is complete
    if (q.n > 1) {
      // Pt + piece 0 + piece 1 + ... per element; each piece's loads issued together
      const float* const R0 = A.xres + (long long)u * kXPieces * 5 * F;
      constexpr int M = (5 * F + NT - 1) / NT;
      float v[M];
#pragma unroll
      for (int m = 0; m < M; ++m) v[m] = tid + m * NT < 5 * F ? Pt[tid + m * NT] : 0.0f;
      for (int pp = 0; pp < q.n; ++pp) {  // block-uniform
        float t[M];
#pragma unroll
        for (int m = 0; m < M; ++m)
          t[m] = tid + m * NT < 5 * F ? R0[(long long)pp * 5 * F + tid + m * NT] : 0.0f;
#pragma unroll
        for (int m = 0; m < M; ++m) v[m] += t[m];
      }
#pragma unroll
      for (int m = 0; m < M; ++m)
        if (tid + m * NT < 5 * F) Pt[tid + m * NT] = v[m];
    }
    if (tid == 0) {
      __hip_atomic_store(A.xst + 2 * u + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(A.xst + 2 * u, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_and(A.xhint + (u >> 5), ~(1u << (u & 31)), __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
#ifdef AVZ_XTRACE
  if (tid == 0 && g_stamps) g_stamps[blockIdx.x * 16 + 7] += __builtin_amdgcn_s_memrealtime() - tm;
#endif
}

// One open piece claimed for the block (wave 0; cand: 64 ints of LDS): -1 when no published
// unit has a piece left. Candidates: the units of the hint bits (from a block-dependent word,
// at most 64), their states read at once; the block takes one with a piece left (a
// block-dependent choice among them, so the claimants spread) by adding 1 to its state.
__device__ __forceinline__ int exact_claim(KArgs& A, int n_units, int* cand) {
  const int lane = threadIdx.x & 63;
  const int nw = (n_units + 31) >> 5;
  const int w_start = (int)(((long long)blockIdx.x * nw) / gridDim.x);
  for (;;) {  // wave-uniform; a retry follows another block's claim of a unit's last piece
    int count = 0;
    for (int w0 = 0; w0 < nw && count < 64; w0 += 64) {  // wave-uniform
      const int wi = w0 + lane;
      int wid = w_start + wi;
      if (wid >= nw) wid -= nw;
      const uint32_t bits =
          wi < nw ? __hip_atomic_load(A.xhint + wid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
      const int cnt = __popc(bits);
      int pre = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(pre, o, 64);
        if (lane >= o) pre += y;
      }
      const int tot = __shfl(pre, 63, 64);
      int pos = count + pre - cnt;
      for (uint32_t x = bits; x != 0u && pos < 64; x &= x - 1u) cand[pos++] = wid * 32 + __builtin_ctz(x);
      count += tot;
    }
    count = min(count, 64);
    if (count == 0) return -1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // cand: LDS, lanes to lanes
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int uid = lane < count ? cand[lane] : -1;
    const uint32_t v =
        uid >= 0 ? __hip_atomic_load(A.xst + 2 * uid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const unsigned long long m = __ballot(x_has_piece(v));
    if (m == 0ull) return -1;
    int k = (int)(blockIdx.x % (unsigned)__popcll(m));
    unsigned long long mm = m;
    for (; k > 0; --k) mm &= mm - 1ull;
    const int src = __builtin_ctzll(mm);
    int res = -1;
    if (lane == src) {
      const uint32_t old =
          __hip_atomic_fetch_add(A.xst + 2 * uid, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (x_has_piece(old)) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        res = (uid << 8) | (int)(old & 0xffu);
      }
    }
    res = __shfl(res, src, 64);
    if (res >= 0) return res;
    __builtin_amdgcn_wave_barrier();  // cand is rewritten by the next scan
  }
}

// After the persistent loop: the block's own unpublished units with deferrals (the unit mask,
// in analysis_items' order; sparse frames only), decided here (exact_unit), then pieces of the
// published units claimed from the whole grid (exact_claim, exact_piece) until none is left.
// Blocks end their loops at different times, so the exact work of one overlaps the others'
// loops (a separate launch spreading the units over its grid ran 173 us against 159 us at
// kappa 64, configs[1]; the work sharing took configs[1]'s analysis from 147 to 112 us).
template <int N, int MASK, bool IRM, bool SPLIT, class TW>
__device__ __forceinline__ void ibm_exact_units(unsigned char* lds, int gx, int n_items) {
  KArgs& A = kernarg_chain_args();
  using G = CGeo<N>;
  using XL = XLds<N>;
  constexpr bool SHARE = N == 1024 && !std::is_same<TW, NoTw>::value;
  constexpr bool PER_BIN = !(N == 1024 && !IRM && SHARE);  // not the reference-bit path
  AVZ_XT(1, __builtin_amdgcn_s_memrealtime());
  if (A.ibm_cert <= 0.0f) return;
  const int tid = threadIdx.x;
  const int P = SPLIT && A.a_pieces > 1 ? A.a_pieces : 1;
  const int n_whole = P > 1 ? A.a_whole : n_items;
  __syncthreads();  // the block's records, partials (global stores of other waves), unit mask
  const uint32_t mine = *reinterpret_cast<const uint32_t*>(lds + G::MISC_OFF + 56);
  auto tables = [&]() {
    int t = threadIdx.x;
    opaque_i(t);  // formed here (a thread index held from the kernel start went to scratch)
    xtab_fill<N>(A.xtw, A.xwin, reinterpret_cast<cd*>(lds + XL::TWL_OFF),
                 reinterpret_cast<float*>(lds + XL::WIN_OFF), t, G::NT);
    __syncthreads();
  };
  bool have_tables = false;
  int seq = 0;
  auto one = [&](int u) {  // the block's own unpublished units (published ones are shared)
    const int k = seq++;
    if (!((mine >> min(k, 31)) & 1u)) return;
    const uint4 rec = reinterpret_cast<const uint4*>(A.xpend)[u];  // block-uniform
    if (rec.x == 0u || rec.w != 0u) return;
    if (k >= 31) {
      // bit 31 stands for every unit past the 31st: one of them that analysis_item skipped
      // (its chunk is past the utterance's end) wrote no record, and an earlier call's sits here
      int b, c;
      unit_item<G::F>(A, u, gx, n_items, n_whole, P, b, c);
      const int L = utt_len(A, b);
      if (L < N || c >= ((L + G::H - 1) / G::H + 1 + kChunk - 1) / kChunk) return;
    }
    if (!have_tables) {
      tables();
      have_tables = true;
    }
    exact_unit<N, PER_BIN>(A, lds, u, gx, n_items, n_whole, P);
  };
  const int n_end = n_whole + (n_items - n_whole) * P;  // analysis_items' sequence
  for (int u = blockIdx.x; u < n_end; u += gridDim.x) one(u < n_whole ? u : n_items + u - n_whole);
  AVZ_XT(2, __builtin_amdgcn_s_memrealtime());
  {
    // the published units' pieces, claimed from the whole grid's (the block's own included)
    // until none is left
    const int n_units = n_items + (n_end - n_whole);
    int* const ctl = reinterpret_cast<int*>(lds + XLds<N>::CTL_OFF);
    for (;;) {  // block-uniform
      AVZ_XT_BEGIN(tc);
      if (tid < 64) {
        const int got = exact_claim(A, n_units, reinterpret_cast<int*>(lds + XLds<N>::SCAN_OFF));
        if (tid == 0) ctl[2] = got;
      }
      AVZ_XT_END(14, tc);
      __syncthreads();
      const int got = ctl[2];
      __syncthreads();
      if (got < 0) break;
      if (!have_tables) {
        AVZ_XT_BEGIN(tt);
        tables();
        have_tables = true;
        AVZ_XT_END(15, tt);
      }
      AVZ_XT_BEGIN(t0x);
      exact_piece<N, PER_BIN>(A, lds, got >> 8, got & 0xff, gx, n_items, n_whole, P);
#ifdef AVZ_XTRACE  // (a count beside the interval: not the pair's form)
      if (tid == 0 && g_stamps) {
        unsigned long long* st = g_stamps + blockIdx.x * 16;
        st[4] += 1;
        st[5] += __builtin_amdgcn_s_memrealtime() - t0x;
      }
#endif
    }
  }
  AVZ_XT(3, __builtin_amdgcn_s_memrealtime());
}
}  // namespace avz
