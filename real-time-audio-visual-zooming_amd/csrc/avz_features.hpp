// avz_features.hpp — the mask-model feature writer shared by the standalone STFT kernel
// (avz_kernels.hip) and the training-batch kernel (avz_train.hip): one definition, so the
// two kernels' features are the same bits.
#pragma once
#include "avz_common.hpp"

namespace avz {

constexpr int kStftThreads = 512;

// Mask-model input features of one (k, t) from the two mic spectra y0, y1:
//  FEAT_LOGMAG_IPD (full_audio_generating_pipeline/inference.py:90-94, NCHW [b][2][F][T]):
//    c=0 log(|y0| + 1e-7), c=1 angle(y0) - angle(y1)
//  FEAT_TFLITE (Final_pipeline/src/inference.py:198-203, 117-128, NHWC [b][F][T][4]):
//    log_mag, sin(ipd), cos(ipd), linspace(0, 1, F)[k]
// float32 throughout, as numpy computes them on scipy's complex64 STFT.
template <int FEAT, int F>
__device__ __forceinline__ void write_features(const StftArgs& A, int b, int k, int t, cf y0,
                                               cf y1) {
  const float lm = logf(sqrtf(y0.x * y0.x + y0.y * y0.y) + 1e-7f);
  const float ipd = atan2f(y0.y, y0.x) - atan2f(y1.y, y1.x);
  float* o = A.F_out + (long long)b * A.f_sb + (long long)k * A.f_sf + (long long)t * A.f_st;
  if constexpr (FEAT == FEAT_LOGMAG_IPD) {
    o[0] = lm;
    o[A.f_sc] = ipd;
  } else {
    // np.linspace(0, 1, F, dtype=float32): k * (1/(F-1)) in fp64, last element exactly 1
    const float fm = (k == F - 1) ? 1.0f : (float)((double)k * (1.0 / (F - 1)));
    float s, c;
    sincosf(ipd, &s, &c);
    o[0] = lm;
    o[A.f_sc] = s;
    o[2 * A.f_sc] = c;
    o[3 * A.f_sc] = fm;
  }
}

}  // namespace avz
