// avz_delay_stream.hpp — host/device argument block and state layout of the streaming blind
// delay-histogram mask (avz_delay_stream_push / _reset, avz_delay_stream.hip; not part of the
// public ABI).
#pragma once
#include "avz_delay_common.hpp"

namespace avz {

struct DelayStreamHeader {
  unsigned long long count;  // frames pushed since the reset
  int nb, n_fft;
};

// One stream's state block for n_fft = N (H = N / 2) and nb histogram bins: a 64-byte header
// (DelayStreamHeader), the previous hop of both mics [2][H] f32 and h [nb] f64; rounded up to
// 256 bytes (4864 bytes at N = 1024, nb = 65).
struct DelayStreamLayout {
  long long prev_off = 0, hist_off = 0, stride = 0;
  constexpr DelayStreamLayout(int n_fft, int nb) {  // constexpr: host and device
    const long long H = n_fft / 2;
    prev_off = 64;
    hist_off = prev_off + 2 * H * 4;
    stride = (hist_off + (long long)nb * 8 + 255) & ~255LL;
  }
};

struct DelayStreamArgs {
  int streams, hops;
  double forget;
  const int* active;          // [streams] or null: 0 = the stream is skipped
  const int* adapt;           // [streams] or null: 0 = the histogram freezes
  const float* mix;           // [streams][2][hops * H] planar
  long long mix_stride, ch_stride;
  const double* angle_deg;    // [streams] or null; a NaN entry = p.plan_angle
  DelayParams p;
  float* mask;                // M[s * m_sb + k * m_sf + j * m_st], j = hop of this call
  long long m_sb, m_sf, m_st;
  double* hist_out;           // [streams][nb] or null
  double* delays_out;         // [streams][hops][8] or null
  int* n_peaks;               // [streams][hops] or null
  unsigned char* state;       // [streams][state_stride bytes]
  long long state_stride;
  const int* select;          // reset: [streams] or null = all
  const float* xwin;          // the plan's fp32 periodic Hann [N]
};

}  // namespace avz

extern "C" int avz_launch_delay_stream_push(int n_fft, const avz::DelayStreamArgs* a, void* stream);
extern "C" int avz_launch_delay_stream_reset(int n_fft, const avz::DelayStreamArgs* a,
                                             void* stream);
