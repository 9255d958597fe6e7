// avz_chain_solve.hpp — the solve stage of the chain and the SRP scan (avz_chunked_k.hpp):
// fp64 sums of a bin's chunk partials (bin_cov_sums; bin_cov_sums_utt for the per-utterance
// kernels' in-block solve), avz_solve_kernel, _lanes_kernel, _fixup_kernel, avz_srp_kernel.
// Needs: avz_chain_common.hpp.
#pragma once
#include "avz_chain_common.hpp"

namespace avz {
// One thread per (utterance, bin): sum the chunk partials in fp64, closed-form MVDR or
// hybrid hard-null weights with the plan's steering table -> coef[b][k] (+ optional
// cov/w debug outputs).
constexpr int kSolveThreads = 256;

// Covariance sums of bin k of utterance b: fp64 sum of its nch chunk partials, scaled back
// by 1/4 (the analysis accumulates (2 y)(2 y)^H).
// V: split-chunk partial vectors per round trip (the per-utterance kernels' fallback takes
// few: its prefetched samples are live there).
template <int N, int V = 8, bool SPLIT = true>
__device__ __forceinline__ void bin_cov_sums(const ChainArgs& A, int b, int k, int nch,
                                             double (&R)[5]) {
  constexpr int F = N / 2 + 1;
  const float* P = A.part + (long long)b * A.nchunk * 5 * F + k;
#pragma unroll
  for (int q = 0; q < 5; ++q) R[q] = 0.0;
  // chunks of a split tail item (analysis_items) sum their pieces' partials
  const long long it0 = (long long)b * ((A.max_frames + kChunk - 1) / kChunk);
  const int cw =
      SPLIT && A.a_pieces > 1 ? (int)max(0LL, min((long long)nch, A.a_whole - it0)) : nch;
  for (int cc = 0; cc < cw; ++cc) {
#pragma unroll
    for (int q = 0; q < 5; ++q) R[q] += (double)P[((long long)cc * 5 + q) * F];
  }
  if (SPLIT && cw < nch) {
    // the split chunks' pieces: (nch - cw) a_pieces consecutive partial vectors of tpart,
    // V per round trip through a descriptor covering exactly them (absent ones read +0,
    // which leaves the sums unchanged); summed in chunk and piece order
    const int nv = (nch - cw) * A.a_pieces;
    const rsrc_t rt =
        make_rsrc(A.tpart + (it0 + cw - A.a_whole) * A.a_pieces * 5 * F, (long long)nv * 5 * F);
    for (int v0 = 0; v0 < nv; v0 += V) {
      float p[V][5];
#pragma unroll
      for (int i = 0; i < V; ++i)
#pragma unroll
        for (int q = 0; q < 5; ++q) p[i][q] = bload_nn(rt, ((v0 + i) * 5 + q) * F + k);
#pragma unroll
      for (int i = 0; i < V; ++i)
#pragma unroll
        for (int q = 0; q < 5; ++q) R[q] += (double)p[i][q];
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) R[q] *= 0.25;
}
// The same for a block-uniform utterance b (the per-utterance synthesis kernel): the
// partials of up to four chunks per round trip through a buffer descriptor covering
// exactly the utterance's nch chunks, so the loads of absent chunks read +0 without
// branches and the sums (chunk order kept, + 0 changes nothing) are bitwise those above.
template <int N, bool SPLIT = true, int VF = 4>
__device__ __forceinline__ void bin_cov_sums_utt(const ChainArgs& A, int b, int k, int nch,
                                                 double (&R)[5]) {
  constexpr int F = N / 2 + 1;
  if (SPLIT && A.a_pieces > 1 &&
      (long long)b * ((A.max_frames + kChunk - 1) / kChunk) + nch > A.a_whole) {
    bin_cov_sums<N, VF>(A, b, k, nch, R);  // some of its chunks were split (block-uniform)
    return;
  }
  const rsrc_t rp = make_rsrc(A.part + (long long)b * A.nchunk * 5 * F, (long long)nch * 5 * F);
#pragma unroll
  for (int q = 0; q < 5; ++q) R[q] = 0.0;
  for (int c0 = 0; c0 < nch; c0 += 4) {
    float p[4][5];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 5; ++q) p[i][q] = bload_nn(rp, ((c0 + i) * 5 + q) * F + k);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 5; ++q) R[q] += (double)p[i][q];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) R[q] *= 0.25;
}
// The solve of bin k of utterance b from its covariance sums: closed-form MVDR or hybrid
// hard-null weights with the plan's steering table -> coef[b][k] (+ the cov / w debug
// outputs, the cov-only stage export, the item-level fallback flag).
template <int N>
__device__ __forceinline__ void solve_bin_out(const ChainArgs& A, int b, int k,
                                              const double (&R)[5]) {
  constexpr int F = N / 2 + 1;
  if (A.cov_only) {  // covariance stage export
#pragma unroll
    for (int q = 0; q < 5; ++q) A.cov_out[((long long)b * F + k) * 5 + q] = R[q];
    return;
  }
  const double* d = A.steer + 4 * k;
  cf al, be;
  float* wdbg = A.w_out ? A.w_out + ((long long)b * F + k) * 4 : nullptr;
  if (A.beamformer == BF_HYBRID_NULL) {
    hybrid_solve_d(R, k, N, A, d[0], d[1], d[2], d[3], al, be, wdbg);
  } else {
    double w[4];
    bool sing = false;
    mvdr_weights_d(R, k, N, A, d[0], d[1], d[2], d[3], w, &sing);
    if (sing && A.singular_fallback == 2) atomicOr(A.flag + b, 1);  // item-level fallback
    coef_from_w(w[0], w[1], w[2], w[3], al, be, wdbg);
  }
  reinterpret_cast<float4*>(A.coef)[(long long)b * F + k] = make_float4(al.x, al.y, be.x, be.y);
  if (A.cov_out) {
#pragma unroll
    for (int q = 0; q < 5; ++q) A.cov_out[((long long)b * F + k) * 5 + q] = R[q];
  }
}

template <int N, bool SPLIT = false>
__global__ void __launch_bounds__(kSolveThreads) avz_solve_kernel(ChainArgs A) {
  constexpr int H = N / 2, F = N / 2 + 1;
  const long long idx = (long long)blockIdx.x * kSolveThreads + threadIdx.x;
  if (idx >= (long long)(A.batch - A.b_lo) * F) return;
  const int b = A.b_lo + (int)(idx / F), k = (int)(idx % F);  // b_lo: first utterance solved
  const int L = utt_len(A, b);
  if (L < N) return;
  const int T = (L + H - 1) / H + 1;
  const int nch = (T + kChunk - 1) / kChunk;
  double R[5];
  bin_cov_sums<N, 8, SPLIT>(A, b, k, nch, R);
  solve_bin_out<N>(A, b, k, R);
}

// The solve of a small split batch (few bins, many partial vectors each: B = 1's 8.23-s
// triple at 512/256 has 17 chunks x 8 pieces): kSolveLanes lanes per bin, each summing a
// contiguous run of the bin's partial vectors (the whole chunks', then the split chunks'
// pieces, bin_cov_sums' order) in fp64, combined by a fixed xor tree -- deterministic, and
// the association differs from the sequential sum only by fp64 rounding. One round trip of
// 20 vectors per lane (160 per bin) where the sequential thread took 17 of 8.
constexpr int kSolveLanes = 8;
template <int N>
__global__ void __launch_bounds__(kSolveThreads) avz_solve_lanes_kernel(ChainArgs A) {
  constexpr int H = N / 2, F = N / 2 + 1, V = 20;
  const int sub = threadIdx.x % kSolveLanes;
  const long long idx = (long long)blockIdx.x * (kSolveThreads / kSolveLanes) +
                        threadIdx.x / kSolveLanes;
  // no early exit: a bin's lanes all take part in the tree (a group is 8 aligned lanes)
  const bool live = idx < (long long)(A.batch - A.b_lo) * F;
  const int b = A.b_lo + (live ? (int)(idx / F) : 0), k = live ? (int)(idx % F) : 0;
  const int L = utt_len(A, b);
  const bool ok = live && L >= N;
  const int T = (max(L, N) + H - 1) / H + 1;
  const int nch = (T + kChunk - 1) / kChunk;
  const long long it0 = (long long)b * ((A.max_frames + kChunk - 1) / kChunk);
  const int cw = A.a_pieces > 1 ? (int)max(0LL, min((long long)nch, A.a_whole - it0)) : nch;
  const int nvec = cw + (nch - cw) * (A.a_pieces > 1 ? A.a_pieces : 0);
  const rsrc_t rp = make_rsrc(A.part + (long long)b * A.nchunk * 5 * F, (long long)cw * 5 * F);
  const rsrc_t rt = cw < nch ? make_rsrc(A.tpart + (it0 + cw - A.a_whole) * A.a_pieces * 5 * F,
                                         (long long)(nvec - cw) * 5 * F)
                             : make_rsrc(nullptr, 0);
  const int per = (nvec + kSolveLanes - 1) / kSolveLanes;
  const int v_lo = sub * per, v_hi = min(nvec, v_lo + per);
  double R[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) R[q] = 0.0;
  for (int v0 = v_lo; v0 < v_hi; v0 += V) {
    float pv[V][5];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int v = v0 + i;  // past v_hi: read, not summed
#pragma unroll
      for (int q = 0; q < 5; ++q)
        pv[i][q] = v < cw ? bload(rp, (v * 5 + q) * F + k) : bload(rt, ((v - cw) * 5 + q) * F + k);
    }
#pragma unroll
    for (int i = 0; i < V; ++i)
      if (v0 + i < v_hi)
#pragma unroll
        for (int q = 0; q < 5; ++q) R[q] += (double)pv[i][q];
  }
#pragma unroll
  for (int o = 1; o < kSolveLanes; o <<= 1)
#pragma unroll
    for (int q = 0; q < 5; ++q) R[q] += __shfl_xor(R[q], o, kSolveLanes);
#pragma unroll
  for (int q = 0; q < 4; ++q) R[q] *= 0.25;
  if (ok && sub == 0) solve_bin_out<N>(A, b, k, R);
}

// batch_mvdr's item-level fallback (AVZ_FALLBACK_BATCH): the items whose solve met a
// singular bin get w = [1 / (conj(d0) + 1e-10), 0] on every bin. No-op otherwise.
template <int N>
__global__ void __launch_bounds__(kSolveThreads) avz_solve_fixup_kernel(ChainArgs A) {
  constexpr int F = N / 2 + 1;
  const long long idx = (long long)blockIdx.x * kSolveThreads + threadIdx.x;
  if (idx >= (long long)A.batch * F) return;
  const int b = (int)(idx / F), k = (int)(idx % F);
  if (A.flag[b] == 0) return;
  double w[4];
  batch_fallback_weights_d(A.steer[4 * k], A.steer[4 * k + 1], w);
  cf al, be;
  coef_from_w(w[0], w[1], w[2], w[3], al, be, A.w_out ? A.w_out + idx * 4 : nullptr);
  reinterpret_cast<float4*>(A.coef)[idx] = make_float4(al.x, al.y, be.x, be.y);
}

// scripts/debug_srp.py:46-62: P(theta) = sum_{f_lo <= f_k <= f_hi} sum_t |d^H y|^2
//   = sum_k R00 + R11 + 2 Re(conj(d0) d1 R01), conj(d0) d1 = exp(i w_k (tau1 - tau2)),
// from the unmasked covariance partials of the analysis kernel (MASK_ONES); one block
// per utterance: partials -> fp64 R in LDS, one thread per angle, dB relative to the max.
constexpr int kSrpThreads = 256;

template <int N>
__global__ void __launch_bounds__(kSrpThreads) avz_srp_kernel(ChainArgs A, SrpArgs S) {
  constexpr int H = N / 2, F = N / 2 + 1;
  __shared__ double R[F][4];
  __shared__ double red[kSrpThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int L = utt_len(A, b);
  double* out = S.power_db + (long long)b * S.n_angles;
  if (L < N) {
    for (int i = tid; i < S.n_angles; i += kSrpThreads) out[i] = __builtin_nan("");
    return;
  }
  const int T = (L + H - 1) / H + 1;
  const int nch = (T + kChunk - 1) / kChunk;
  const float* P = A.part + (long long)b * A.nchunk * 5 * F;
  for (int k = tid; k < F; k += kSrpThreads) {
    double r[4] = {0, 0, 0, 0};
    for (int cc = 0; cc < nch; ++cc) {
#pragma unroll
      for (int q = 0; q < 4; ++q) r[q] += (double)P[((long long)cc * 5 + q) * F + k];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) R[k][q] = 0.25 * r[q];  // analysis sums (2 y)(2 y)^H
  }
  __syncthreads();
  // f_k = rfftfreq(N, 1/fs)[k]; the scanned bins
  const double df = 1.0 / (N * (1.0 / A.fs));
  const double step = (S.n_angles > 1) ? (S.angle_hi - S.angle_lo) / (S.n_angles - 1) : 0.0;
  // -inf, not a finite floor: a map whose powers are all 0 (an all-zero mixture, a band that
  // holds no bin) comes back as -inf - (-inf) = NaN, as debug_srp.py:61-62 gives
  double best = -__builtin_inf();
  for (int i = tid; i < S.n_angles; i += kSrpThreads) {
    const double ang = (i == S.n_angles - 1 && S.n_angles > 1) ? S.angle_hi : S.angle_lo + i * step;
    const double th = ang * (M_PI / 180.0);
    // tau1 - tau2 = (d/2) cos(th)/c - (d/2) cos(th - pi)/c  (debug_srp.py:17-23)
    const double t1 = (A.mic_d / 2) * cos(0.0) * cos(th - 0) / A.c_sound;
    const double t2 = (A.mic_d / 2) * cos(0.0) * cos(th - M_PI) / A.c_sound;
    double p = 0.0;
    for (int k = 0; k < F; ++k) {
      const double f = k * df;
      if (f < S.f_lo || f > S.f_hi) continue;
      double sn, cs;
      sincos(2.0 * M_PI * f * (t1 - t2), &sn, &cs);
      p += R[k][0] + R[k][1] + 2.0 * (cs * R[k][2] - sn * R[k][3]);
    }
    const double db = 10.0 * log10(p);
    out[i] = db;
    best = fmax(best, db);
  }
  for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_xor(best, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  double mx = red[0];
#pragma unroll
  for (int w = 1; w < kSrpThreads / 64; ++w) mx = fmax(mx, red[w]);
  for (int i = tid; i < S.n_angles; i += kSrpThreads) out[i] -= mx;
}
}  // namespace avz
