// avz_kernels.hip — standalone STFT kernel (stage API, parity tests) for gfx950.
// The beamforming chain itself lives in avz_chunked.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avz_frame.hpp"

namespace avz {

// ---------------------------------------------------------------------------
// Standalone STFT (stage API / parity): Y[b][c][k][t] = scipy.signal.stft(x[b][c])
// One block per (utterance, NSLOT-frame batch); each lane group transforms one
// frame of the packed channel pair, then threads split the pair per bin.
// (kStftThreads = 512 and the feature writer write_features: avz_features.hpp)
template <int N, int FEAT>
__global__ void __launch_bounds__(kStftThreads, 1) avz_stft_kernel(StftArgs A) {
  using G = Geo<N, kStftThreads>;
  constexpr int F = G::F, NSLOT = G::NSLOT;
  extern __shared__ __align__(16) unsigned char lds[];
  FrameBlock<N> B;
  if (!B.init(lds, A.len, A.max_len)) return;
  const int b = B.b, f0 = B.f0, T = B.T, tid = threadIdx.x;

  Lanes<N> ln;
  ln.init(lds, tid);
  const float* xb = A.x + (long long)b * A.x_stride;
  const rsrc_t re = make_rsrc(xb, B.L);
  const rsrc_t im = make_rsrc(A.channels > 1 ? xb + A.ch_stride : nullptr, B.L);
  StftWindow<N> win;
  win.init(ln.lm);
  frame_transform<N>(ln, re, im, B.s0(ln), win, B.twid);
  __syncthreads();
  float2* Y = reinterpret_cast<float2*>(A.Y);
  for (int idx = tid; idx < F * NSLOT; idx += kStftThreads) {
    const int k = idx / NSLOT, f = idx % NSLOT;
    const int t = f0 + f;
    if (t >= T) continue;
    const cf* Z = slot_ptr<N>(lds, f);
    cf a, c;
    split_pair(Z[k], Z[(N - k) & (N - 1)], a, c);
    if constexpr (FEAT != FEAT_NONE) {
      write_features<FEAT, F>(A, b, k, t, a, c);
    } else {
      const long long o = (long long)b * A.y_stride_b + (long long)k * A.y_stride_f + t;
      Y[o] = make_float2(a.x, a.y);
      if (A.channels > 1) Y[o + A.y_stride_c] = make_float2(c.x, c.y);
    }
  }
}

}  // namespace avz

using namespace avz;

extern "C" int avz_launch_stft(int n_fft, const StftArgs* a, void* stream) {
  if (a->batch <= 0) return 0;
  return dispatch_feat<true>(a->feat, [&](auto feat) {
    return dispatch_n_fft(n_fft, [&](auto n) {
      constexpr int N = decltype(n)::value, FEAT = decltype(feat)::value;
      return launch<avz_stft_kernel<N, FEAT>>(FrameBlock<N>::grid(a->batch, a->max_frames),
                                              kStftThreads, FrameBlock<N>::G::LDS_BYTES,
                                              (hipStream_t)stream, *a);
    });
  });
}
