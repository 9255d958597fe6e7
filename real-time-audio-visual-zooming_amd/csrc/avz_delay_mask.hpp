// avz_delay_mask.hpp — host/device argument block of the blind delay-histogram mask
// (avz_delay_mask, avz_delay_mask.hip; not part of the public ABI).
#pragma once
#include "avz_delay_common.hpp"

namespace avz {

constexpr int kDelayFrames = 16;  // frames per block of the histogram and label kernels

// Workspace of one call: per-block histogram partials [batch][nblk][hist_bins] f64 (a block's
// sums over its 16 frames; blocks past an utterance's frames are never written nor read), the
// candidate lists [batch][8] f64 and their counts [batch] i32, each 256-byte aligned.
struct DelayLayout {
  long long part_off = 0, list_off = 0, count_off = 0, bytes = 0;
  int nblk = 0;
  DelayLayout(long long batch, int max_frames, int hist_bins) {
    auto up = [](long long v) { return (v + 255) & ~255LL; };
    nblk = (max_frames + kDelayFrames - 1) / kDelayFrames;
    part_off = 0;
    list_off = up(part_off + batch * nblk * hist_bins * 8);
    count_off = up(list_off + batch * kDelayList * 8);
    bytes = up(count_off + batch * 4);
  }
};

struct DelayArgs {
  int batch;
  const int* len;             // clamped to max_len in the kernels
  int max_len, max_frames, nblk;
  const float* mix;           // [B][2][..] planar
  long long mix_stride, ch_stride;
  const double* angle_deg;    // [B] or null = p.plan_angle
  DelayParams p;
  float* mask;                // M[b * m_sb + k * m_sf + t * m_st]
  long long m_sb, m_sf, m_st;
  double* hist_out;           // [B][nb] or null
  double* delays_out;         // [B][8] or null
  int* n_peaks;               // [B] or null
  double* part;               // workspace (DelayLayout)
  double* list;
  int* count;
};

}  // namespace avz

extern "C" int avz_launch_delay_mask(int n_fft, const avz::DelayArgs* a, void* stream);
