// avz_chain_finalize.hpp — the finalize stage of the chain (avz_chunked_k.hpp): chunk seams,
// peak and rescale after the chunk-grid synthesis (finalize_item, avz_finalize_kernel), and of
// the N = 1024 per-utterance kernel's pieces (avz_finalize_pieces_kernel).
// Needs: avz_chain_common.hpp, avz_chain_utt.hpp (UttGeo: the pieces' step).
#pragma once
#include "avz_chain_common.hpp"
#include "avz_chain_utt.hpp"

namespace avz {
// Finalize blocks handle FCH consecutive chunks (N = 512: two, so a block rescales the same
// 64 KB as N = 1024's one chunk instead of twice as many blocks moving 31 KB each).
template <int N>
constexpr int kFinChunks = N >= 1024 ? 1 : 1024 / N;

// One finalize item: chunks FCH q .. FCH q + FCH - 1 of utterance b, the standalone
// finalize kernel's block (red: NWAVE floats of LDS).
template <int N>
__device__ __forceinline__ void finalize_item(const ChainArgs& A, int q, int b, float* red) {
  constexpr int NT = kCThreads, H = N / 2, NWAVE = NT / 64, FCH = kFinChunks<N>;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c0 = FCH * q;
  const int L = utt_len(A, b);
  if (L < N) {
    if (c0 == 0 && tid == 0 && A.peak) A.peak[b] = __builtin_nanf("");
    return;
  }
  const int T = (L + H - 1) / H + 1;
  const int nch = (T + kChunk - 1) / kChunk;
  if (c0 >= nch) return;
  const int cend = min(c0 + FCH, nch);  // chunks c0 .. cend - 1
  const float* heads = A.heads + (long long)b * A.nchunk * H;
  const float* tails = A.tails + (long long)b * A.nchunk * H;
  // boundary segment 32 cc - 1 = tail(cc - 1) + head(cc), cc = 1 .. nch - 1
  auto boundary = [&](int cc, int m) -> float {
    return (tails[(long long)(cc - 1) * H + m] + heads[(long long)cc * H + m]) * inv_wsum<N>(m);
  };
  float* outb = A.out + (long long)b * A.out_stride;
  if (A.normalize != NORM_PEAK) {
    // un-normalised output (the batch driver's deferred normalisation): each block writes
    // its chunks' seams and folds their max (chunk 0: the interiors' max) into peak[b],
    // zeroed by the analysis kernel, with an atomicMax on the float's bits (non-negative
    // floats order as unsigned ints) — no redundant reads of the other seams
    float pm = 0.0f;
    for (int c = max(c0, 1); c < cend; ++c) {
      const long long j = (long long)kChunk * c - 1;
      for (int m = tid; m < H; m += NT) {
        const float x = boundary(c, m);
        outb[j * H + m] = x;
        pm = fmaxf(pm, fabsf(x));
      }
    }
    for (int o = 32; o > 0; o >>= 1) pm = fmaxf(pm, __shfl_xor(pm, o, 64));
    if (lane == 0) red[wave] = pm;
    __syncthreads();
    if (tid == 0 && A.peak) {
      float qm = (c0 == 0) ? __uint_as_float(A.peak_u[b]) : 0.0f;
#pragma unroll
      for (int w = 0; w < NWAVE; ++w) qm = fmaxf(qm, red[w]);
      atomicMax(reinterpret_cast<unsigned int*>(A.peak + b), __float_as_uint(qm));
    }
    return;
  }
  // The chunks' interior segments 32c .. 32c+30 are read into registers first: their loads
  // do not depend on the utterance peak, so they stream while the seam maxima below are
  // fetched (all blocks are resident at once; reading them after the peak left every
  // block waiting on its seam loads before any bulk traffic started).
  constexpr int U = ((kChunk - 1) * H / 4 + NT - 1) / NT;
  float4 xin[FCH][U];
#pragma unroll
  for (int g = 0; g < FCH; ++g) {
    const int c = c0 + g;
    const int j0 = kChunk * c, j1 = min(kChunk * c + kChunk - 1, T - 1);
    const float4* o4 = reinterpret_cast<const float4*>(outb + (long long)j0 * H);
    const int n4 = c < cend ? (j1 - j0) * H / 4 : 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * NT;
      if (i < n4) xin[g][u] = o4[i];
    }
  }
  float pk = 0.0f;
#pragma unroll 4
  for (int idx = tid; idx < (nch - 1) * H; idx += NT)
    pk = fmaxf(pk, fabsf(boundary(idx / H + 1, idx % H)));
  for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
  if (lane == 0) red[wave] = pk;
  __syncthreads();
  pk = __uint_as_float(A.peak_u[b]);
#pragma unroll
  for (int w = 0; w < NWAVE; ++w) pk = fmaxf(pk, red[w]);
  if (c0 == 0 && tid == 0 && A.peak) A.peak[b] = pk;
  const float scale = 1.0f / (pk + A.norm_eps);
  for (int c = max(c0, 1); c < cend; ++c) {
    const long long j = (long long)kChunk * c - 1;
    for (int m = tid; m < H; m += NT) outb[j * H + m] = boundary(c, m) * scale;
  }
#pragma unroll
  for (int g = 0; g < FCH; ++g) {
    const int c = c0 + g;
    const int j0 = kChunk * c, j1 = min(kChunk * c + kChunk - 1, T - 1);
    float4* o4 = reinterpret_cast<float4*>(outb + (long long)j0 * H);
    const int n4 = c < cend ? (j1 - j0) * H / 4 : 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = tid + u * NT;
      if (i < n4) {
        float4 x = xin[g][u];
        x.x *= scale; x.y *= scale; x.z *= scale; x.w *= scale;
        o4[i] = x;
      }
    }
  }
}

template <int N>
__global__ void __launch_bounds__(kCThreads) avz_finalize_kernel(ChainArgs A) {
  __shared__ float red[kCThreads / 64];
  finalize_item<N>(A, blockIdx.x, blockIdx.y, red);
}

// Finalize of the per-utterance synthesis kernel's piece utterances b = s_whole + blockIdx.y
// (peak normalisation): the seam segments between its pieces (piece p - 1's last half-frame
// + piece p's first, x 1 / sum w^2), the utterance peak (the pieces' interior maxima in
// peak_u[b] and the seams), peak[b], and the in-place rescale of segments [0, T - 2], block x
// taking kFinPieceU float4 groups per thread of them (every block reduces the few seams
// itself: no cross-block hand-off).
constexpr int kFinPieceU = 4;
constexpr int kMaxPieces = 32;  // pieces per utterance (synth_split; avz_capi.cpp seam_slots)
template <int N>
__global__ void __launch_bounds__(kCThreads) avz_finalize_pieces_kernel(ChainArgs A) {
  constexpr int H = N / 2, NWAVE = kCThreads / 64, FBS = UttGeo::FB;
  __shared__ float red[NWAVE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int b = A.s_whole + blockIdx.y;
  const int L = utt_len(A, b);
  if (L < N) {
    if (blockIdx.x == 0 && tid == 0 && A.peak) A.peak[b] = __builtin_nanf("");
    return;
  }
  const int T = (L + H - 1) / H + 1;
  const int seg = FBS * A.s_steps;               // frames per piece
  const int n4 = (T - 1) * H / 4;                // float4 groups of segments 0 .. T - 2
  const int g0 = blockIdx.x * kFinPieceU * kCThreads;
  if (g0 >= n4) return;
  const long long slot0 = (long long)(b - A.s_whole) * A.s_pieces;
  // seam segment j = p seg - 1 (p >= 1, j <= T - 2): tail of piece p - 1 + head of piece p
  auto seam = [&](int p, int m) -> float {
    return (A.ptails[(slot0 + p - 1) * H + m] + A.pheads[(slot0 + p) * H + m]) * inv_wsum<N>(m);
  };
  const int n_seam = (T - 2 + 1) / seg;          // p = 1 .. n_seam
  const uint32_t pk_int = A.peak_u[b];  // the pieces' interior maxima (loaded with the rest)
  float4 x[kFinPieceU];
  float* outb = A.out + (long long)b * A.out_stride;
  const float4* o4 = reinterpret_cast<const float4*>(outb);
#pragma unroll
  for (int u = 0; u < kFinPieceU; ++u) {
    const int i = g0 + u * kCThreads + tid;
    if (i < n4) x[u] = o4[i];                    // interior values stream while the seams reduce
  }
  // the seams' max: up to 7 seams x H values with all of a thread's loads in flight (more
  // registers for the 31 seams of 32 pieces ran 10.5 -> 17 us at B = 257: 7 seams)
  constexpr int SU = 7 * H / kCThreads;
  float sv[SU];
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    const int idx = tid + u * kCThreads;
    sv[u] = idx < n_seam * H ? seam(idx / H + 1, idx % H) : 0.0f;
  }
  float pk = 0.0f;
#pragma unroll
  for (int u = 0; u < SU; ++u) pk = fmaxf(pk, fabsf(sv[u]));
  for (int idx = tid + SU * kCThreads; idx < n_seam * H; idx += kCThreads)  // more (not split
    pk = fmaxf(pk, fabsf(seam(idx / H + 1, idx % H)));                      // so finely)
  for (int o = 32; o > 0; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
  if (lane == 0) red[wave] = pk;
  __syncthreads();
  pk = __uint_as_float(pk_int);
#pragma unroll
  for (int w = 0; w < NWAVE; ++w) pk = fmaxf(pk, red[w]);
  if (blockIdx.x == 0 && tid == 0 && A.peak) A.peak[b] = pk;
  const float scale = 1.0f / (pk + A.norm_eps);
  float4* w4 = reinterpret_cast<float4*>(outb);
#pragma unroll
  for (int u = 0; u < kFinPieceU; ++u) {
    const int i = g0 + u * kCThreads + tid;
    if (i >= n4) continue;
    const int j = 4 * i / H, m = 4 * i % H;
    float4 y = x[u];
    if ((j + 1) % seg == 0) {                    // a seam (j = p seg - 1 <= T - 2)
      const int p = (j + 1) / seg;
      y = make_float4(seam(p, m), seam(p, m + 1), seam(p, m + 2), seam(p, m + 3));
    }
    y.x *= scale; y.y *= scale; y.z *= scale; y.w *= scale;
    w4[i] = y;
  }
}

// Grid x of the finalize kernel: FCH-chunk groups of the longest utterance.
template <int N>
static inline int fin_groups(int nch) { return (nch + kFinChunks<N> - 1) / kFinChunks<N>; }
}  // namespace avz
