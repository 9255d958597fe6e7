// avz_train.hip — one mask-estimator training batch per launch (avz_mask_training_batch):
// the U-Net / TFLite input features of the mic pair and the ideal-binary-mask label of the two
// references, the sample model_training.py's SpatialDataset.__getitem__ (:80-92) builds.
//
// Layout: avz_stft_kernel's. 512 threads, one block per (item, 16 frames), twiddles in LDS;
// each lane group transforms its frame twice in the same LDS slot: first the packed mic pair
// mic0 + i mic1, from which the block writes the features (write_features, shared with
// avz_stft_kernel: the same bits as avz_mask_features); then, after a barrier, the packed
// reference pair tgt + i itf, from which the block writes the label. The slot area is not
// doubled, so the LDS footprint and the blocks per CU are the STFT kernel's. Each waveform is
// read once, no spectrum goes to memory.
//
// Label: 1 where |S_t| > |S_i|, decided on this kernel's fp32 transform as the chain's
// ibm_kappa < 0 tier does (avz_chain_common.hpp ibm_noise): with Z = S_t + i S_i,
// |S_t|^2 - |S_i|^2 = Re(Z[k] Z[N - k]), one fused product difference, label = (that > 0).
// This is NOT the reference-exact path of avz_ibm_exact.hpp: a decision whose margin is below
// the fp32 transform's error may differ from numpy's. Two all-zero reference frames give
// Z = 0 and the label 0, exactly; scaling both references by a power of two scales every
// intermediate exactly, so the labels do not change.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avz_frame.hpp"

namespace avz {

template <int N, int FEAT>
__global__ void __launch_bounds__(kStftThreads, 1) avz_train_kernel(TrainArgs T_) {
  using G = Geo<N, kStftThreads>;
  constexpr int F = G::F, NSLOT = G::NSLOT;
  const StftArgs& A = T_.s;
  extern __shared__ __align__(16) unsigned char lds[];
  FrameBlock<N> B;
  if (!B.init(lds, A.len, A.max_len)) return;
  const int b = B.b, f0 = B.f0, L = B.L, T = B.T, tid = threadIdx.x;

  Lanes<N> ln;
  ln.init(lds, tid);
  StftWindow<N> win;
  win.init(ln.lm);
  const int s0 = B.s0(ln);

  // pass 1: the mic pair -> features
  {
    const float* xb = A.x + (long long)b * A.x_stride;
    frame_transform<N>(ln, make_rsrc(xb, L), make_rsrc(xb + A.ch_stride, L), s0, win, B.twid);
  }
  __syncthreads();
  for (int idx = tid; idx < F * NSLOT; idx += kStftThreads) {
    const int k = idx / NSLOT, f = idx % NSLOT;
    const int t = f0 + f;
    if (t >= T) continue;
    const cf* Z = slot_ptr<N>(lds, f);
    cf a, c;
    split_pair(Z[k], Z[(N - k) & (N - 1)], a, c);
    write_features<FEAT, F>(A, b, k, t, a, c);
  }
  __syncthreads();  // every slot has been read before its lane group overwrites it

  // pass 2: the reference pair -> label
  frame_transform<N>(ln, make_rsrc(T_.tgt + (long long)b * T_.ref_stride, L),
                     make_rsrc(T_.itf + (long long)b * T_.ref_stride, L), s0, win, B.twid);
  __syncthreads();
  float* lab = T_.label + (long long)b * T_.l_sb;
  for (int idx = tid; idx < F * NSLOT; idx += kStftThreads) {
    const int k = idx / NSLOT, f = idx % NSLOT;
    const int t = f0 + f;
    if (t >= T) continue;
    const cf* Z = slot_ptr<N>(lds, f);
    const cf z = Z[k], zp = Z[(N - k) & (N - 1)];
    // |S_t|^2 - |S_i|^2 = Re(z zp)
    const float d = fmaf(z.x, zp.x, -(z.y * zp.y));
    lab[(long long)k * T_.l_sf + (long long)t * T_.l_st] = d > 0.0f ? 1.0f : 0.0f;
  }
}

}  // namespace avz

using namespace avz;

extern "C" int avz_launch_train(int n_fft, const TrainArgs* a, void* stream) {
  if (a->s.batch <= 0) return 0;
  return dispatch_feat<false>(a->s.feat, [&](auto feat) {
    return dispatch_n_fft(n_fft, [&](auto n) {
      constexpr int N = decltype(n)::value, FEAT = decltype(feat)::value;
      return launch<avz_train_kernel<N, FEAT>>(FrameBlock<N>::grid(a->s.batch, a->s.max_frames),
                                               kStftThreads, FrameBlock<N>::G::LDS_BYTES,
                                               (hipStream_t)stream, *a);
    });
  });
}
