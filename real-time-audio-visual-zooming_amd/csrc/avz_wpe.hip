// avz_wpe.hip — offline batch WPE dereverberation of a two-mic spectrum (gfx950).
//
// The first stage of the reference's reverberant chain, rt_av_zoom/core/dereverb.py:76-78
// (wpe(Y, taps=10, delay=3, iterations=3, psd_context=0, statistics_mode='full')), as the
// algorithm of Nakatani et al. 2010 (avz/dereverb.py wpe_numpy is the
// fp64 host restatement). Per (item, bin), with Y [2, T], K = taps, n = 2 K:
//   Yt[2 tau + m, t] = Y[m, t - delay - tau] (0 before the first frame);   X = Y;
//   repeat: p[t] = mean_m |X[m,t]|^2, lambda[t] = 1 / max(p[t], 1e-10 max_t p),
//           R = sum_t lambda Yt Yt^H,  P = sum_t lambda Yt Y^H,  G = R^-1 P,  X = Y - G^H Yt.
//
// One 256-thread block owns one (item, bin) problem for all iterations:
//  - the bin's two T-frame rows are read from HBM once into LDS (complex64) and the final
//    iteration stores Z: one read of Y and one write of Z are the only global traffic;
//  - lambda[t] lives in LDS as fp64; X is never stored: it is recomputed from Y and G
//    (2 n complex multiply-adds per frame) where the next lambda or the output needs it;
//  - R and P are cut into 2 x 2 blocks (tap pair x mic pair; K (K + 1) / 2 lower-triangle
//    blocks of R, K blocks of P). A thread owns one block, eight fp64 accumulators in
//    registers, over every `slices`-th frame; the slices' partial sums are added in a fixed
//    order through LDS (no atomics: the same bits on every call);
//  - fp64 Cholesky of the packed lower triangle in LDS (left-looking, two lanes per row) and
//    the two triangular solves for both right-hand sides, each lane holding one unknown and
//    the solved ones broadcast by a lane shuffle, all on one wave: n columns without a
//    block barrier, and a quarter of the instructions four waves would issue for them.
// A Cholesky pivot <= (n + 1) 2^-52 R_jj or not finite, a zero-power bin, or fewer than n
// regressor frames pass the input through (status 2 / 1 / 2).
//
// LDS: 24 B per frame (two complex64 rows + the fp64 lambda) + at most 16 KiB for the
// packed R (16 B x n (n + 1) / 2), P / G (16 B x 2 n) and the slices' partial sums
// (64 B x (slices - 1) x blocks), so 2048 frames fit the 64 KiB a block may claim without
// opting in to more: kWpeMaxFrames.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "avz_internal.h"

namespace avz {

constexpr int kWpeThreads = 256;
constexpr int kWpeMaxFrames = 2048;
constexpr int kWpeMaxSlices = 4;
constexpr unsigned kWpeMaxLds = 64 * 1024;

struct WpeLayout {
  int n;         // 2 taps
  int nrb;       // lower-triangle 2 x 2 blocks of R: taps (taps + 1) / 2
  int ntasks;    // nrb + taps (the blocks of P)
  int slices;    // frame slices per block task
  unsigned off_g, off_part, off_lam, off_y, bytes;
};

struct WpeX {
  double r0, i0, r1, i1;
};

// packed lower triangle: (i, j), i >= j
__device__ __forceinline__ int wpe_idx(int i, int j) { return i * (i + 1) / 2 + j; }

// X[:, t] = Y[:, t] - G^H Yt[:, t] in fp64 (G [n][2] in LDS; use_g false: X = Y)
__device__ __forceinline__ WpeX wpe_x(const float2* y0, const float2* y1, const double2* G, int t,
                                      int taps, int delay, bool use_g) {
  const float2 c0 = y0[t], c1 = y1[t];
  WpeX x{(double)c0.x, (double)c0.y, (double)c1.x, (double)c1.y};
  if (use_g) {
    for (int tau = 0; tau < taps; ++tau) {
      const int s = t - delay - tau;
      if (s < 0) break;
      const float2 a0 = y0[s], a1 = y1[s];
      const double2 g00 = G[4 * tau], g01 = G[4 * tau + 1];      // row 2 tau:     mic 0, 1
      const double2 g10 = G[4 * tau + 2], g11 = G[4 * tau + 3];  // row 2 tau + 1
      const double ar = a0.x, ai = a0.y, er = a1.x, ei = a1.y;
      // x_m -= conj(g0m) a0 + conj(g1m) a1
      x.r0 -= g00.x * ar + g00.y * ai + g10.x * er + g10.y * ei;
      x.i0 -= g00.x * ai - g00.y * ar + g10.x * ei - g10.y * er;
      x.r1 -= g01.x * ar + g01.y * ai + g11.x * er + g11.y * ei;
      x.i1 -= g01.x * ai - g01.y * ar + g11.x * ei - g11.y * er;
    }
  }
  return x;
}

// Orders one wave's LDS stores before its later LDS loads across lanes.
__device__ __forceinline__ void wpe_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double wpe_block_max(double v, double* red, int tid) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  v = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return v;
}

__global__ void __launch_bounds__(kWpeThreads) avz_wpe_kernel(WpeArgs A, WpeLayout L) {
  extern __shared__ __align__(16) unsigned char wpe_lds[];
  __shared__ double red[4];
  __shared__ double piv[1];  // 1: the factorisation met a singular or non-finite pivot
  double2* Rp = reinterpret_cast<double2*>(wpe_lds);
  double2* G = reinterpret_cast<double2*>(wpe_lds + L.off_g);
  double* part = reinterpret_cast<double*>(wpe_lds + L.off_part);
  double* lam = reinterpret_cast<double*>(wpe_lds + L.off_lam);
  float2* y0 = reinterpret_cast<float2*>(wpe_lds + L.off_y);
  float2* y1 = y0 + A.frames;

  const int tid = threadIdx.x;
  const int b = blockIdx.x / A.bins, k = blockIdx.x % A.bins;
  const int T = A.frames, taps = A.taps, delay = A.delay, n = L.n;
  int Tb = A.frames_b ? A.frames_b[b] : T;
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  const float2* gy0 = reinterpret_cast<const float2*>(A.Y) + b * A.y_sb + k * A.y_sf;
  const float2* gy1 = gy0 + A.y_sm;
  float2* gz0 = reinterpret_cast<float2*>(A.Z) + b * A.z_sb + k * A.z_sf;
  float2* gz1 = gz0 + A.z_sm;

  for (int t = tid; t < T; t += kWpeThreads) {
    const float2 c0 = gy0[t], c1 = gy1[t];
    if (t < Tb) {
      y0[t] = c0;
      y1[t] = c1;
    } else {  // frames beyond the item's length: copied, in no sum
      gz0[t] = c0;
      gz1[t] = c1;
    }
  }
  __syncthreads();

  // this thread's block task: rows (2 ti, 2 ti + 1) of Yt against rows (2 tj, 2 tj + 1) of
  // Yt (a block of R) or against Y itself (a block of P); frames sl, sl + slices, ...
  const bool worker = tid < L.slices * L.ntasks;
  const int u = tid % L.ntasks, sl = tid / L.ntasks;
  const bool is_p = u >= L.nrb;
  int ti = 0, tj = 0;
  if (is_p) {
    ti = u - L.nrb;
  } else {
    while ((ti + 1) * (ti + 2) / 2 <= u) ++ti;
    tj = u - ti * (ti + 1) / 2;
  }
  const int oa = delay + ti, ob = is_p ? 0 : delay + tj;

  int status = 0;
  if (Tb - delay < n) status = 2;  // fewer regressor frames than unknowns

  for (int it = 0; it < A.iterations && status == 0; ++it) {
    // lambda from the current X
    double pm = 0.0;
    for (int t = tid; t < Tb; t += kWpeThreads) {
      const WpeX x = wpe_x(y0, y1, G, t, taps, delay, it > 0);
      const double p = 0.5 * (x.r0 * x.r0 + x.i0 * x.i0 + x.r1 * x.r1 + x.i1 * x.i1);
      lam[t] = p;
      pm = fmax(pm, p);
    }
    pm = wpe_block_max(pm, red, tid);  // (also orders the lam[] writes before the reads)
    if (pm == 0.0) {
      status = 1;
      break;
    }
    const double eps = 1e-10 * pm;
    for (int t = tid; t < Tb; t += kWpeThreads) lam[t] = 1.0 / fmax(lam[t], eps);
    __syncthreads();

    // R and P: this thread's 2 x 2 block over its frames
    double c00r = 0, c00i = 0, c01r = 0, c01i = 0, c10r = 0, c10i = 0, c11r = 0, c11i = 0;
    if (worker) {
      for (int t = oa + sl; t < Tb; t += L.slices) {
        const double w = lam[t];
        const float2 a0 = y0[t - oa], a1 = y1[t - oa];
        const float2 e0 = y0[t - ob], e1 = y1[t - ob];
        const double a0r = w * a0.x, a0i = w * a0.y, a1r = w * a1.x, a1i = w * a1.y;
        const double e0r = e0.x, e0i = e0.y, e1r = e1.x, e1i = e1.y;
        // c[r][c] += lambda a_r conj(e_c)
        c00r = fma(a0r, e0r, fma(a0i, e0i, c00r));
        c00i = fma(a0i, e0r, fma(-a0r, e0i, c00i));
        c01r = fma(a0r, e1r, fma(a0i, e1i, c01r));
        c01i = fma(a0i, e1r, fma(-a0r, e1i, c01i));
        c10r = fma(a1r, e0r, fma(a1i, e0i, c10r));
        c10i = fma(a1i, e0r, fma(-a1r, e0i, c10i));
        c11r = fma(a1r, e1r, fma(a1i, e1i, c11r));
        c11i = fma(a1i, e1r, fma(-a1r, e1i, c11i));
      }
      if (sl > 0) {
        double* q = part + (size_t)(sl - 1) * 8 * L.ntasks + u;
        q[0] = c00r;
        q[L.ntasks] = c00i;
        q[2 * L.ntasks] = c01r;
        q[3 * L.ntasks] = c01i;
        q[4 * L.ntasks] = c10r;
        q[5 * L.ntasks] = c10i;
        q[6 * L.ntasks] = c11r;
        q[7 * L.ntasks] = c11i;
      }
    }
    __syncthreads();
    if (worker && sl == 0) {
      for (int s = 1; s < L.slices; ++s) {
        const double* q = part + (size_t)(s - 1) * 8 * L.ntasks + u;
        c00r += q[0];
        c00i += q[L.ntasks];
        c01r += q[2 * L.ntasks];
        c01i += q[3 * L.ntasks];
        c10r += q[4 * L.ntasks];
        c10i += q[5 * L.ntasks];
        c11r += q[6 * L.ntasks];
        c11i += q[7 * L.ntasks];
      }
      const int i0 = 2 * ti, i1 = i0 + 1;
      if (is_p) {
        G[2 * i0] = make_double2(c00r, c00i);
        G[2 * i0 + 1] = make_double2(c01r, c01i);
        G[2 * i1] = make_double2(c10r, c10i);
        G[2 * i1 + 1] = make_double2(c11r, c11i);
      } else {
        const int j0 = 2 * tj, j1 = j0 + 1;
        Rp[wpe_idx(i0, j0)] = make_double2(c00r, c00i);
        Rp[wpe_idx(i1, j0)] = make_double2(c10r, c10i);
        Rp[wpe_idx(i1, j1)] = make_double2(c11r, c11i);
        if (ti > tj) Rp[wpe_idx(i0, j1)] = make_double2(c01r, c01i);
      }
    }
    __syncthreads();

    // One wave factors and solves (the other waves wait at the barrier below): its LDS
    // accesses execute in order, so a wave-level fence orders them between lanes and the n
    // columns need no block barrier.
    if (tid < 64) {
      // Cholesky R = L L^H in place, left-looking: two lanes share a row's inner product.
      // The diagonal keeps (l_jj, 1 / l_jj).
      const int i = tid >> 1, h = tid & 1;
      const double thr = (double)(n + 1) * 0x1p-52;
      int bad = 0;
      for (int j = 0; j < n; ++j) {
        double sr = 0, si = 0;
        if (i >= j && i < n) {
          for (int c = h; c < j; c += 2) {
            const double2 a = Rp[wpe_idx(i, c)], e = Rp[wpe_idx(j, c)];
            sr = fma(a.x, e.x, fma(a.y, e.y, sr));
            si = fma(a.y, e.x, fma(-a.x, e.y, si));
          }
        }
        sr += __shfl_xor(sr, 1, 64);
        si += __shfl_xor(si, 1, 64);
        const double djj = Rp[wpe_idx(j, j)].x;
        const double d = djj - __shfl(sr, 2 * j, 64);
        if (!(d > thr * djj) || !(fabs(d) <= 1.79769313486231570815e308)) {
          bad = 1;
          break;
        }
        const double l = sqrt(d), rl = 1.0 / l;
        if (h == 0 && i >= j && i < n) {
          const double2 v = Rp[wpe_idx(i, j)];
          Rp[wpe_idx(i, j)] =
              i == j ? make_double2(l, rl) : make_double2((v.x - sr) * rl, (v.y - si) * rl);
        }
        wpe_wave_lds_sync();
      }
      // L Z = P, then L^H G = Z: lane q of each half holds unknown q of one column
      if (!bad) {
        const int c = tid >> 5, q = tid & 31;
        double2 r = q < n ? G[2 * q + c] : make_double2(0, 0);
        for (int u2 = 0; u2 < n; ++u2) {
          const double rl = Rp[wpe_idx(u2, u2)].y;
          const double zr = __shfl(r.x * rl, u2 + 32 * c, 64);
          const double zi = __shfl(r.y * rl, u2 + 32 * c, 64);
          if (q == u2) r = make_double2(zr, zi);
          if (q > u2 && q < n) {
            const double2 a = Rp[wpe_idx(q, u2)];
            r.x -= a.x * zr - a.y * zi;
            r.y -= a.x * zi + a.y * zr;
          }
        }
        for (int u2 = n - 1; u2 >= 0; --u2) {
          const double rl = Rp[wpe_idx(u2, u2)].y;
          const double zr = __shfl(r.x * rl, u2 + 32 * c, 64);
          const double zi = __shfl(r.y * rl, u2 + 32 * c, 64);
          if (q == u2) r = make_double2(zr, zi);
          if (q < u2) {
            const double2 a = Rp[wpe_idx(u2, q)];  // conj(L[u2][q]) g_u2
            r.x -= a.x * zr + a.y * zi;
            r.y -= a.x * zi - a.y * zr;
          }
        }
        if (q < n) G[2 * q + c] = r;
      }
      if (tid == 0) piv[0] = bad ? 1.0 : 0.0;
    }
    __syncthreads();
    if (piv[0] != 0.0) status = 2;
    __syncthreads();  // piv is rewritten by the next iteration
  }

  if (status == 0) {
    for (int t = tid; t < Tb; t += kWpeThreads) {
      const WpeX x = wpe_x(y0, y1, G, t, taps, delay, true);
      gz0[t] = make_float2((float)x.r0, (float)x.i0);
      gz1[t] = make_float2((float)x.r1, (float)x.i1);
    }
  } else {
    for (int t = tid; t < Tb; t += kWpeThreads) {
      gz0[t] = y0[t];
      gz1[t] = y1[t];
    }
  }
  if (tid == 0 && A.status) A.status[blockIdx.x] = status;
}

}  // namespace avz

using namespace avz;

extern "C" int avz_wpe_max_frames(void) { return kWpeMaxFrames; }

extern "C" int avz_launch_wpe(const WpeArgs* a, void* stream) {
  const long long blocks = (long long)a->batch * a->bins;
  if (blocks <= 0) return 0;
  if (blocks > 0x7fffffffLL) return -2;
  auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
  WpeLayout L;
  L.n = 2 * a->taps;
  L.nrb = a->taps * (a->taps + 1) / 2;
  L.ntasks = L.nrb + a->taps;
  L.slices = kWpeThreads / L.ntasks < kWpeMaxSlices ? kWpeThreads / L.ntasks : kWpeMaxSlices;
  size_t o = up16(sizeof(double) * 2 * (size_t)(L.n * (L.n + 1) / 2));
  L.off_g = (unsigned)o;
  o += up16(sizeof(double) * 2 * 2 * (size_t)L.n);
  L.off_part = (unsigned)o;
  o += up16(sizeof(double) * 8 * (size_t)(L.slices - 1) * L.ntasks);
  L.off_lam = (unsigned)o;
  o += up16(sizeof(double) * (size_t)a->frames);
  L.off_y = (unsigned)o;
  o += sizeof(float) * 2 * 2 * (size_t)a->frames;
  L.bytes = (unsigned)o;
  if (o > kWpeMaxLds) return -2;
  hipLaunchKernelGGL(avz_wpe_kernel, dim3((unsigned)blocks), dim3(kWpeThreads), L.bytes,
                     (hipStream_t)stream, *a, L);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}
