// avz_frame.hpp — what the frame kernels outside the chain share (avz_kernels.hip,
// avz_train.hip, avz_delay_mask.hip; avz_stream.hip, avz_wpe_stream.hip, avz_delay_stream.hip):
// the lane-group set-up, the batch block prologue and its windowed packed transform, the
// stream block set-up and its transform, the small state helpers of the streamers, and the
// host-side size dispatch and launch. The chain (avz_chunked*.hip, avz_chain_*.hpp) uses none
// of it: its code layout is tuned on its own (csrc/Makefile).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "avz_common.hpp"
#include "avz_features.hpp"

namespace avz {

// ------------------------------------------------------------------------------- lane groups
// A thread's place in its 32-lane group: the group's transform, its lane map, the frame slot
// the group owns and that slot's address. The same for the 512-thread batch blocks and the
// 256-thread stream blocks (two groups per wave).
template <int N>
struct Lanes {
  typename KCfg<N>::Fft fft;
  LaneMap<N> lm;
  int my_slot;
  cf* spec;
  __device__ __forceinline__ void init(unsigned char* lds, int tid) {
    const int wave = tid >> 6, lane = tid & 63;
    fft.init(lane);
    lm.init(lane);
    my_slot = wave * KCfg<N>::FPW + lm.grp;
    spec = slot_ptr<N>(lds, my_slot);
  }
};

// ------------------------------------------------------------------------------ batch blocks
// Block (b, f0) of a batch frame kernel: avz_stft_kernel's grid and LDS map (Geo<N, 512>), one
// block per (utterance, NSLOT frames).
template <int N>
struct FrameBlock {
  using G = Geo<N, kStftThreads>;
  const cf* twid;
  int b, f0, L, T;  // utterance, first frame, clamped length, the utterance's frame count
  static dim3 grid(int batch, int max_frames) {
    return dim3(batch, (max_frames + G::NSLOT - 1) / G::NSLOT);
  }
  // Fills the twiddles and places the block. False where the block has no frame (past the
  // utterance's last, or an utterance shorter than a frame): the caller returns. Every thread
  // of a block gets the same answer, and the twiddles are visible on return.
  __device__ __forceinline__ bool init(unsigned char* lds, const int* len, int max_len) {
    cf* tw = reinterpret_cast<cf*>(lds + G::TW_OFF);
    KCfg<N>::Fft::fill_twiddles(tw, threadIdx.x, kStftThreads);
    twid = tw;
    b = blockIdx.x;
    f0 = blockIdx.y * G::NSLOT;
    L = min(len[b], max_len);
    T = (L + G::H - 1) / G::H + 1;
    if (f0 >= T || L < N) return false;
    __syncthreads();
    return true;
  }
  // First sample of the lane group's frame, lane part included (scipy's centred framing).
  __device__ __forceinline__ int s0(const Lanes<N>& ln) const {
    return (f0 + ln.my_slot) * G::H - N / 2 + ln.lm.in0;
  }
};

// scipy's STFT window of a lane's samples, 2 / N times the periodic Hann: register r's weight
// follows from the lane's by the angle addition with W32 (frame_transform).
template <int N>
struct StftWindow {
  float a0, ac, as;
  __device__ __forceinline__ void init(const LaneMap<N>& lm) {
    double s, c;
    sincospi(2.0 * lm.in0 / N, &s, &c);
    const double sc = 2.0 / N;
    a0 = (float)(0.5 * sc);
    ac = (float)(0.5 * sc * c);
    as = (float)(0.5 * sc * s);
  }
};

// Windowed forward transform of the frame at sample s0 (lane part included) of the packed
// pair re + i im into the lane group's slot. A null descriptor reads zeros (one channel).
template <int N>
__device__ __forceinline__ void frame_transform(const Lanes<N>& ln, rsrc_t re, rsrc_t im, int s0,
                                                const StftWindow<N>& win, const cf* twid) {
  using C = KCfg<N>;
  constexpr int PPL = C::PPL;
  cf v[PPL];
  static_for<0, PPL>([&](auto r) {
    constexpr int j = (C::IN_STRIDE * 32 / N) * r;
    constexpr float cr = W32::c[j % 32], sr = -W32::s[j % 32];
    const float w = fmaf(win.as, sr, fmaf(-win.ac, cr, win.a0));
    v[r] = {bload(re, s0 + C::IN_STRIDE * r) * w, bload(im, s0 + C::IN_STRIDE * r) * w};
  });
  ln.fft.forward(v, ln.spec, twid);
  static_for<0, PPL>([&](auto k) { ln.spec[ln.lm.out0 + C::OUT_STRIDE * k] = v[k]; });
}

// ----------------------------------------------------------------------------- stream blocks
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

// A stream block's set-up, in the two steps around the block's first barrier: stage() fills the
// twiddles and copies the plan's window into LDS (StreamGeo<N>'s map); the kernel stages its own
// rows (tail, histogram) and ends the staging with __syncthreads(); init() then sets the lane
// groups up. wave and lane are derived in stage(): derived after the barrier, my_slot folds into
// tid >> 5 and the slot addresses of the N = 1024 kernels take thirty more adds.
template <int N>
struct StreamBlock : Lanes<N> {
  const cf* twid;
  const float* win;
  int wave, lane;
  __device__ __forceinline__ void stage(unsigned char* lds, const float* xwin, int tid) {
    using SG = StreamGeo<N>;
    cf* tw = reinterpret_cast<cf*>(lds + SG::TW_OFF);
    float* w = reinterpret_cast<float*>(lds + SG::WIN_OFF);
    KCfg<N>::Fft::fill_twiddles(tw, tid, kStreamThreads);
    for (int n = tid; n < N; n += kStreamThreads) w[n] = xwin[n];
    twid = tw;
    win = w;
    wave = tid >> 6;
    lane = tid & 63;
  }
  // Lanes<N>::init's four lines on the stored wave and lane (calling it with them through an
  // overload changes the batch kernels' schedule as well).
  __device__ __forceinline__ void init(unsigned char* lds) {
    this->fft.init(lane);
    this->lm.init(lane);
    this->my_slot = wave * KCfg<N>::FPW + this->lm.grp;
    this->spec = slot_ptr<N>(lds, this->my_slot);
  }
};

// Windowed forward transform of the packed pair re + i im of hop j's frame [x_{j-1} | x_j]
// into the lane group's slot. Sample q = j H - H + n of the call's rows; q < 0 is the state's
// previous hop. A slot beyond the group's frames transforms zeros.
template <int N>
__device__ __forceinline__ void stream_transform(const StreamBlock<N>& sb, const float* re,
                                                 const float* im, const float* pre,
                                                 const float* pim, int j, bool valid) {
  using C = KCfg<N>;
  constexpr int PPL = C::PPL, H = N / 2;
  cf v[PPL];
  static_for<0, PPL>([&](auto r) {
    const int n = sb.lm.in0 + C::IN_STRIDE * r;
    const long long q = (long long)j * H - H + n;
    float a = 0.0f, b = 0.0f;
    if (valid) {
      a = q < 0 ? pre[q + H] : re[q];
      b = q < 0 ? pim[q + H] : im[q];
    }
    const float w = sb.win[n] * (2.0f / N);  // 1 / sum(w): exact scaling
    v[r] = {a * w, b * w};
  });
  __builtin_amdgcn_wave_barrier();
  sb.fft.forward(v, sb.spec, sb.twid);
  static_for<0, PPL>([&](auto k) { sb.spec[sb.lm.out0 + C::OUT_STRIDE * k] = v[k]; });
}

// The call's last hop becomes the state's previous hop: prev ([2][H]) takes the last H of the
// `hops` hops of the two mic rows.
template <int H>
__device__ __forceinline__ void save_last_hop(float* prev, const float* x0, const float* x1,
                                              int hops, int tid) {
  const long long qlast = (long long)(hops - 1) * H;
  for (int m = tid; m < H; m += kStreamThreads) {
    prev[m] = x0[qlast + m];
    prev[H + m] = x1[qlast + m];
  }
}

// Zero bytes [from, to) of a stream's state block (both multiples of 4), one block's threads.
__device__ __forceinline__ void zero_state(unsigned char* st, long long from, long long to) {
  uint32_t* words = reinterpret_cast<uint32_t*>(st);
  for (long long i = from / 4 + threadIdx.x; i < to / 4; i += kStreamThreads) words[i] = 0u;
}

// Overlap-add denominator of output sample m < H: w^2[m] + w^2[m + H].
template <int H>
__device__ __forceinline__ float ola_den(const float* win, int m) {
  const float w0 = win[m], w1 = win[m + H];
  return fmaf(w1, w1, w0 * w0);
}

// ---------------------------------------------------------------------------------- host side
// f(std::integral_constant<int, n_fft>) for a transform size the library is built for, else -4.
template <typename Fn>
static int dispatch_n_fft(int n_fft, Fn&& f) {
  if (n_fft == 1024) return f(std::integral_constant<int, 1024>{});
  if (n_fft == 512) return f(std::integral_constant<int, 512>{});
  return -4;
}

// f(std::integral_constant<int, feat>) for a mask-model feature layout, else -4; FEAT_NONE
// (spectra, no features) only where the caller has such a kernel.
template <bool WITH_NONE, typename Fn>
static int dispatch_feat(int feat, Fn&& f) {
  switch (feat) {
    case FEAT_NONE:
      if constexpr (WITH_NONE) return f(std::integral_constant<int, FEAT_NONE>{});
      break;
    case FEAT_LOGMAG_IPD: return f(std::integral_constant<int, FEAT_LOGMAG_IPD>{});
    case FEAT_TFLITE: return f(std::integral_constant<int, FEAT_TFLITE>{});
  }
  return -4;
}

// Launch Kern with `lds` bytes of dynamic LDS (its attribute set first, once per device; a
// kernel that asks for none has nothing to set): 0, or -3 where either step fails.
template <auto Kern, typename... Args>
static int launch(dim3 grid, int threads, int lds, hipStream_t st, const Args&... args) {
  if (lds > 0 && !lds_ready<Kern>(lds)) return -3;
  hipLaunchKernelGGL(Kern, grid, dim3(threads), lds, st, args...);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace avz
