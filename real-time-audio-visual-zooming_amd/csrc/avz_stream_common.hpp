// avz_stream_common.hpp — what the streaming kernels share (avz_stream.hip, avz_wpe_stream.hip):
// the block geometry and the windowed packed two-mic transform of one hop's frame.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avz_common.hpp"

namespace avz {

constexpr int kStreamThreads = 256;

template <int N>
struct StreamGeo {
  using C = KCfg<N>;
  using G = Geo<N, kStreamThreads>;
  static constexpr int H = N / 2, F = N / 2 + 1;
  static constexpr int NSLOT = G::NSLOT;  // 8 frames per group
  // LDS map: [FFT slots][twiddles][window N f32][tail H f32][noise bits F u32]
  static constexpr int TW_OFF = G::SLOT_LDS;
  static constexpr int WIN_OFF = TW_OFF + C::TW_BYTES;
  static constexpr int TAIL_OFF = WIN_OFF + N * 4;
  static constexpr int BITS_OFF = TAIL_OFF + H * 4;
  static constexpr int LDS_BYTES = BITS_OFF + ((F * 4 + 15) & ~15);
  static_assert(NSLOT == 8, "eight frame slots per 256-thread block");
  static_assert(C::GROUP_BYTES >= N * 8, "a slot holds a whole spectrum");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// Windowed forward transform of the packed pair re + i im of hop j's frame [x_{j-1} | x_j]
// into the lane group's slot. Sample q = j H - H + n of the call's rows; q < 0 is the state's
// previous hop. A slot beyond the group's frames transforms zeros.
template <int N>
__device__ __forceinline__ void stream_transform(const typename KCfg<N>::Fft& fft,
                                                 const LaneMap<N>& lm, const float* re,
                                                 const float* im, const float* pre,
                                                 const float* pim, int j, bool valid,
                                                 const float* win, cf* spec, const cf* twid) {
  using C = KCfg<N>;
  constexpr int PPL = C::PPL, H = N / 2;
  cf v[PPL];
  static_for<0, PPL>([&](auto r) {
    const int n = lm.in0 + C::IN_STRIDE * r;
    const long long q = (long long)j * H - H + n;
    float a = 0.0f, b = 0.0f;
    if (valid) {
      a = q < 0 ? pre[q + H] : re[q];
      b = q < 0 ? pim[q + H] : im[q];
    }
    const float w = win[n] * (2.0f / N);  // 1 / sum(w): exact scaling
    v[r] = {a * w, b * w};
  });
  __builtin_amdgcn_wave_barrier();
  fft.forward(v, spec, twid);
  static_for<0, PPL>([&](auto k) { spec[lm.out0 + C::OUT_STRIDE * k] = v[k]; });
}

}  // namespace avz
