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

#include "avz_common.hpp"
#include "avz_features.hpp"

namespace avz {

// Windowed forward transform of the frame at sample s0 (lane part included) of the packed
// pair re + i im into the lane group's slot, scipy scaling (2 / N times the periodic Hann).
template <int N>
__device__ __forceinline__ void train_transform(typename KCfg<N>::Fft& fft, const LaneMap<N>& lm,
                                                rsrc_t re, rsrc_t im, int s0, float wa0,
                                                float wac, float was, cf* spec, const cf* twid) {
  using C = KCfg<N>;
  constexpr int PPL = C::PPL;
  cf v[PPL];
  static_for<0, PPL>([&](auto r) {
    constexpr int j = (C::IN_STRIDE * 32 / N) * r;
    constexpr float cr = W32::c[j % 32], sr = -W32::s[j % 32];
    const float w = fmaf(was, sr, fmaf(-wac, cr, wa0));
    v[r] = {bload(re, s0 + C::IN_STRIDE * r) * w, bload(im, s0 + C::IN_STRIDE * r) * w};
  });
  fft.forward(v, spec, twid);
  static_for<0, PPL>([&](auto k) { spec[lm.out0 + C::OUT_STRIDE * k] = v[k]; });
}

template <int N, int FEAT>
__global__ void __launch_bounds__(kStftThreads, 1) avz_train_kernel(TrainArgs T_) {
  using C = KCfg<N>;
  using G = Geo<N, kStftThreads>;
  constexpr int H = G::H, F = G::F, NSLOT = G::NSLOT;
  const StftArgs& A = T_.s;
  extern __shared__ __align__(16) unsigned char lds[];
  cf* twid = reinterpret_cast<cf*>(lds + G::TW_OFF);
  C::Fft::fill_twiddles(twid, threadIdx.x, kStftThreads);
  const int b = blockIdx.x;
  const int f0 = blockIdx.y * NSLOT;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int L = min(A.len[b], A.max_len);
  const int T = (L + H - 1) / H + 1;
  if (f0 >= T || L < N) return;
  __syncthreads();

  typename C::Fft fft;
  fft.init(lane);
  LaneMap<N> lm;
  lm.init(lane);
  const int my_slot = wave * C::FPW + lm.grp;
  cf* spec = slot_ptr<N>(lds, my_slot);
  float wa0, wac, was;
  {
    double s, c;
    sincospi(2.0 * lm.in0 / N, &s, &c);
    const double sc = 2.0 / N;
    wa0 = (float)(0.5 * sc);
    wac = (float)(0.5 * sc * c);
    was = (float)(0.5 * sc * s);
  }
  const int s0 = (f0 + my_slot) * H - N / 2 + lm.in0;

  // pass 1: the mic pair -> features
  {
    const float* xb = A.x + (long long)b * A.x_stride;
    train_transform<N>(fft, lm, make_rsrc(xb, L), make_rsrc(xb + A.ch_stride, L), s0, wa0, wac,
                       was, spec, twid);
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
  train_transform<N>(fft, lm, make_rsrc(T_.tgt + (long long)b * T_.ref_stride, L),
                     make_rsrc(T_.itf + (long long)b * T_.ref_stride, L), s0, wa0, wac, was, spec,
                     twid);
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

template <int N, int FEAT>
static int launch_train_t(const TrainArgs* a, hipStream_t st) {
  auto kern = avz_train_kernel<N, FEAT>;
  const int lds = Geo<N, kStftThreads>::LDS_BYTES;
  if (!lds_ready<avz_train_kernel<N, FEAT>>(lds)) return -3;
  constexpr int NS = Geo<N, kStftThreads>::NSLOT;
  dim3 grid(a->s.batch, (a->s.max_frames + NS - 1) / NS);
  hipLaunchKernelGGL(kern, grid, dim3(kStftThreads), lds, st, *a);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

extern "C" int avz_launch_train(int n_fft, const TrainArgs* a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (a->s.batch <= 0) return 0;
  switch (a->s.feat) {
    case FEAT_LOGMAG_IPD:
      if (n_fft == 1024) return launch_train_t<1024, FEAT_LOGMAG_IPD>(a, st);
      if (n_fft == 512) return launch_train_t<512, FEAT_LOGMAG_IPD>(a, st);
      break;
    case FEAT_TFLITE:
      if (n_fft == 1024) return launch_train_t<1024, FEAT_TFLITE>(a, st);
      if (n_fft == 512) return launch_train_t<512, FEAT_TFLITE>(a, st);
      break;
  }
  return -4;
}
