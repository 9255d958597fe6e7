// avz_scene.hip — on-device synthetic scene generation and mixing (gfx950): the
// reference's anechoic far-field generator, full_audio_generating_pipeline/
// world_building.py:47-59 (per-mic fractional delay by an rfft phase shift over the WHOLE
// signal) with the SIR / AWGN / shared-peak conventions of Final_pipeline/src/
// simulation.py:167-202 (the bench's generator, avz/synth.py make_scene).
//
// Two entry points share the mixing back end:
//  * avz_scene_mix      — sources, angles and unit-normal noise given (the host RNG draws
//                         of synth.scene_draws, so the device scene is the host scene);
//  * avz_scene_generate — everything on the device: counter-based Philox4x32-10 draws
//                         (Box-Muller normals, 53-bit uniforms), the speech-like AR(2)
//                         source model with its syllabic envelope (synth.speech_like), the
//                         interferer azimuths; synth.make_scene_philox is its host restatement.
//
// The reverberant counterparts (avz_room_rir, avz_scene_reverb_mix, avz_scene_reverb_generate:
// the reference's ShoeBox scenes, simulation.py:105-165) follow the anechoic code: an
// image-source RIR kernel and the convolution with it at a padded FFT length, into the same
// mixing back end.
//
// Fractional delay, O(n log n). Real sources are packed two per complex signal, run
// through a mixed-radix (8, 4, 2, 5, 3) Stockham FFT in fp64, split, multiplied by the
// per-mic phase ramps exp(-2 pi i f tau) with irfft's conventions (DC and Nyquist imaginary
// parts dropped), summed into the target and interference images, packed two mics per
// complex signal and inverse transformed: four length-n FFTs per utterance for up to four
// sources. A length with another prime factor takes the exact O(n^2) circular convolution
// with the periodic kernel h[d] = -(1/n) (-1)^d sin(pi delta) cot(pi (d - delta) / n).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include "avz_internal.h"

namespace avz {

// ================================================================ Philox4x32-10 draws
struct U4 {
  uint32_t x, y, z, w;
};
// Random123's philox4x32 with 10 rounds: ctr (c0..c3), key (k0, k1).
__device__ __forceinline__ U4 philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                         uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return {c0, c1, c2, c3};
}

// Draw streams of utterance idx (key = (idx, kSceneKey ^ seed)); synth.py mirrors these.
constexpr uint32_t kSceneKey = 0x5CE7E5EDu;
constexpr uint32_t kStreamNoise = 0x100u;  // + mic
constexpr uint32_t kStreamUnif = 0x200u;
constexpr uint32_t kUnifPhase = 0x1000u;     // + source: envelope phase
constexpr uint32_t kUnifKeep = 0x100000u;    // * (1 + source) + block: keep flags
constexpr uint32_t kUnifPos = 0x2000u;       // + 2 (source - 2) + {0, 1}: room position x, y
constexpr int kSegLen = 256;                 // AR(2) segment (even: normal pairs stay whole)

__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {
  return (double)((((uint64_t)hi << 32) | lo) >> 11) * 0x1p-53;
}
// Normal pair i of a stream: Box-Muller on (u1 in (0, 1], u2 in [0, 1)).
__device__ __forceinline__ void normal_pair(uint32_t k0, uint32_t k1, uint32_t stream, uint32_t i,
                                            double& z0, double& z1) {
  const U4 r = philox4x32(i, stream, 0u, 0u, k0, k1);
  const double u1 = (double)(((((uint64_t)r.x << 32) | r.y) >> 11) + 1) * 0x1p-53;
  const double u2 = u53(r.z, r.w);
  const double rr = sqrt(-2.0 * log(u1));
  double s, c;
  sincospi(2.0 * u2, &s, &c);
  z0 = rr * c;
  z1 = rr * s;
}
__device__ __forceinline__ double uniform(uint32_t k0, uint32_t k1, uint32_t j) {
  const U4 r = philox4x32(j, kStreamUnif, 0u, 0u, k0, k1);
  return u53(r.x, r.y);
}

struct GenArgs {
  int batch, n_src, n, nseg;
  long long start;
  uint32_t seed;
  double fs;
  float* src;          // [B][n_src][n] speech-like sources
  float* noise;        // [B][2][n] unit normals
  double* angles;      // [B][n_src]
  double* zs;          // [B][n_src][nseg][2] zero-state final (y[e], y[e-1]) per segment
  double* sin_;        // [B][n_src][nseg][2] true state entering each segment
};

__device__ __forceinline__ void gen_key(const GenArgs& G, int b, uint32_t& k0, uint32_t& k1) {
  const unsigned long long idx = (unsigned long long)(G.start + b);
  k0 = (uint32_t)idx;
  k1 = (uint32_t)(idx >> 32) ^ kSceneKey ^ G.seed;
}

// AR(2) x -> y[m] = x[m] + 1.4 y[m-1] - 0.45 y[m-2] (lfilter([1], [1, -1.4, 0.45])) over
// segment `seg` from state (y1, y2); FINAL: write source * envelope, else the final state.
template <bool FINAL>
__global__ void __launch_bounds__(256) scene_ar_kernel(GenArgs G) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long tot = (long long)G.batch * G.n_src * G.nseg;
  if (t >= tot) return;
  const int seg = (int)(t % G.nseg);
  const int s = (int)((t / G.nseg) % G.n_src);
  const int b = (int)(t / ((long long)G.nseg * G.n_src));
  uint32_t k0, k1;
  gen_key(G, b, k0, k1);
  double y1 = 0.0, y2 = 0.0;
  const long long so = (((long long)b * G.n_src + s) * G.nseg + seg) * 2;
  if (FINAL) {
    y1 = G.sin_[so];
    y2 = G.sin_[so + 1];
  }
  const int m0 = seg * kSegLen, m1 = min(G.n, m0 + kSegLen);
  // envelope |sin(2 pi 4 t + phi)| with phi ~ U(0, pi); 250-ms blocks kept with p = 0.75
  const double phi = M_PI * uniform(k0, k1, kUnifPhase + (uint32_t)s);
  const int blk = (int)(0.25 * G.fs);
  float* out = G.src + ((long long)b * G.n_src + s) * G.n;
  int keep_blk = -1;
  bool keep = true;
  for (int m = m0; m < m1; m += 2) {
    double x[2];
    normal_pair(k0, k1, (uint32_t)s, (uint32_t)(m >> 1), x[0], x[1]);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const double y = x[q] + 1.4 * y1 - 0.45 * y2;
      y2 = y1;
      y1 = y;
      if (FINAL && m + q < G.n) {  // odd n: the last pair's second sample falls outside
        const int mm = m + q;
        if (mm / blk != keep_blk) {
          keep_blk = mm / blk;
          keep = uniform(k0, k1, kUnifKeep * (1u + (uint32_t)s) + (uint32_t)keep_blk) >= 0.25;
        }
        const double env = keep ? fabs(sin(2.0 * M_PI * 4.0 * ((double)mm / G.fs) + phi)) : 0.0;
        out[mm] = (float)(y * env);
      }
    }
  }
  if (!FINAL) {
    G.zs[so] = y1;
    G.zs[so + 1] = y2;
  }
}

// Segment states: S_j = A^L S_{j-1} + Z_j (A the AR(2) companion matrix); one thread per
// source. Thread s = 0 also draws the utterance's azimuths (target 90, interferer 1 at 40,
// further ones U(0, 180), as synth.make_scene).
__global__ void __launch_bounds__(64) scene_ar_scan_kernel(GenArgs G) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= G.batch * G.n_src) return;
  const int b = t / G.n_src, s = t % G.n_src;
  uint32_t k0, k1;
  gen_key(G, b, k0, k1);
  if (s == 0) {
    double* ang = G.angles + (long long)b * G.n_src;
    ang[0] = 90.0;
    if (G.n_src > 1) ang[1] = 40.0;
    for (int k = 2; k < G.n_src; ++k) ang[k] = 180.0 * uniform(k0, k1, (uint32_t)(k - 2));
  }
  // M = A^kSegLen, A = [[1.4, -0.45], [1, 0]]
  double m00 = 1.0, m01 = 0.0, m10 = 0.0, m11 = 1.0;
  for (int i = 0; i < kSegLen; ++i) {
    const double a00 = 1.4 * m00 - 0.45 * m10, a01 = 1.4 * m01 - 0.45 * m11;
    m10 = m00;
    m11 = m01;
    m00 = a00;
    m01 = a01;
  }
  double y1 = 0.0, y2 = 0.0;
  const long long so = ((long long)b * G.n_src + s) * G.nseg * 2;
  for (int j = 0; j < G.nseg; ++j) {
    G.sin_[so + 2 * j] = y1;
    G.sin_[so + 2 * j + 1] = y2;
    const double n1 = m00 * y1 + m01 * y2 + G.zs[so + 2 * j];
    const double n2 = m10 * y1 + m11 * y2 + G.zs[so + 2 * j + 1];
    y1 = n1;
    y2 = n2;
  }
}

__global__ void __launch_bounds__(256) scene_noise_kernel(GenArgs G) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int half = (G.n + 1) / 2;  // odd n: the last pair keeps its first normal
  if (t >= (long long)G.batch * 2 * half) return;
  const int i = (int)(t % half);
  const int c = (int)((t / half) & 1);
  const int b = (int)(t / (2LL * half));
  uint32_t k0, k1;
  gen_key(G, b, k0, k1);
  double z0, z1;
  normal_pair(k0, k1, kStreamNoise + (uint32_t)c, (uint32_t)i, z0, z1);
  float* z = G.noise + ((long long)b * 2 + c) * G.n + 2 * i;
  z[0] = (float)z0;
  if (2 * i + 1 < G.n) z[1] = (float)z1;
}

// ================================================================ mixed-radix FFT (fp64)
struct Rad {
  static constexpr double C8 = 0.70710678118654752440;
  static constexpr double S3 = 0.86602540378443864676;
  static constexpr double C5a = 0.30901699437494742410, S5a = 0.95105651629515357212;
  static constexpr double C5b = -0.80901699437494742410, S5b = 0.58778525229247312917;
};
// cos / sin of 2 pi m / R for the radices used
template <int R>
__device__ __forceinline__ void rad_cs(int m, double& c, double& s) {
  m %= R;
  if constexpr (R == 2) {
    c = m ? -1.0 : 1.0; s = 0.0;
  } else if constexpr (R == 4) {
    const double cc[4] = {1, 0, -1, 0}, ss[4] = {0, 1, 0, -1};
    c = cc[m]; s = ss[m];
  } else if constexpr (R == 8) {
    const double cc[8] = {1, Rad::C8, 0, -Rad::C8, -1, -Rad::C8, 0, Rad::C8};
    const double ss[8] = {0, Rad::C8, 1, Rad::C8, 0, -Rad::C8, -1, -Rad::C8};
    c = cc[m]; s = ss[m];
  } else if constexpr (R == 3) {
    const double cc[3] = {1, -0.5, -0.5}, ss[3] = {0, Rad::S3, -Rad::S3};
    c = cc[m]; s = ss[m];
  } else {
    static_assert(R == 5, "radix");
    const double cc[5] = {1, Rad::C5a, Rad::C5b, Rad::C5b, Rad::C5a};
    const double ss[5] = {0, Rad::S5a, Rad::S5b, -Rad::S5b, -Rad::S5a};
    c = cc[m]; s = ss[m];
  }
}

// One Stockham pass (Govindaraju et al.): for j < n/R, v[r] = in[j + r n/R] W^{r (j mod Ns)},
// length-R DFT, out[(j / Ns) Ns R + j mod Ns + r Ns] = V[r]; W = exp(dir 2 pi i / (Ns R)).
// Signals: grid.y utterances (stride sb elements) x grid.z signals (stride n).
template <int R>
__global__ void __launch_bounds__(256) scene_fft_pass(const double2* __restrict__ in,
                                                      double2* __restrict__ out, int n, int Ns,
                                                      long long sb, double dir) {
  const int nr = n / R;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nr) return;
  const long long base = (long long)blockIdx.y * sb + (long long)blockIdx.z * n;
  const int jm = j % Ns;
  double2 v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = in[base + j + (long long)r * nr];
  if (Ns > 1) {
#pragma unroll
    for (int r = 1; r < R; ++r) {
      double s, c;
      sincospi(2.0 * (double)(r * jm) / (double)(Ns * R), &s, &c);
      s *= dir;
      v[r] = make_double2(v[r].x * c - v[r].y * s, v[r].x * s + v[r].y * c);
    }
  }
  double2 o[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    double ax = 0.0, ay = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double c, s;
      rad_cs<R>(r * k, c, s);
      s *= dir;
      ax += v[r].x * c - v[r].y * s;
      ay += v[r].x * s + v[r].y * c;
    }
    o[k] = make_double2(ax, ay);
  }
  const int d0 = (j / Ns) * Ns * R + jm;
#pragma unroll
  for (int r = 0; r < R; ++r) out[base + d0 + (long long)r * Ns] = o[r];
}

// n = product of radices in {8, 4, 2, 5, 3}; returns the count (0: another prime factor).
static int fft_factor(int n, int* rad) {
  int k = 0;
  for (int r : {8, 4, 2, 5, 3})
    while (n % r == 0 && k < 32) {
      rad[k++] = r;
      n /= r;
    }
  return n == 1 ? k : 0;
}

// Transform `nz` signals per utterance in place of the ping-pong pair; returns the buffer
// holding the result.
static double2* fft_run(double2* a, double2* b, int n, int batch, int nz, long long sb,
                        double dir, hipStream_t st) {
  int rad[32];
  const int np = fft_factor(n, rad);
  int Ns = 1;
  for (int p = 0; p < np; ++p) {
    const int R = rad[p];
    const dim3 grid((unsigned)((n / R + 255) / 256), (unsigned)batch, (unsigned)nz);
    switch (R) {
      case 8: hipLaunchKernelGGL(scene_fft_pass<8>, grid, dim3(256), 0, st, a, b, n, Ns, sb, dir); break;
      case 4: hipLaunchKernelGGL(scene_fft_pass<4>, grid, dim3(256), 0, st, a, b, n, Ns, sb, dir); break;
      case 2: hipLaunchKernelGGL(scene_fft_pass<2>, grid, dim3(256), 0, st, a, b, n, Ns, sb, dir); break;
      case 5: hipLaunchKernelGGL(scene_fft_pass<5>, grid, dim3(256), 0, st, a, b, n, Ns, sb, dir); break;
      default: hipLaunchKernelGGL(scene_fft_pass<3>, grid, dim3(256), 0, st, a, b, n, Ns, sb, dir); break;
    }
    Ns *= R;
    double2* t = a;
    a = b;
    b = t;
  }
  return a;
}

// delta of (utterance b, source s, mic c): tau_mic * fs with world_building.py:47-51
// tau_1 = (d/2) cos(theta)/c, tau_2 = (d/2) cos(theta - pi)/c
__device__ __forceinline__ double scene_tau(const SceneArgs& A, int b, int s, int mic) {
  const double th = A.angles_deg[(long long)b * A.n_src + s] * (M_PI / 180.0);
  return (A.mic_d / 2) * cos(th - (mic ? M_PI : 0.0)) / A.c_sound;
}

// live[b][s] = 1 for a source with a non-zero sample (zeroed before the pack kernel; every
// writer stores the same 1). Splitting a packed transform leaves some 1e-16 of a source in
// its partner's spectrum: nothing beside a sounding partner, but an all-zero target or
// all-zero interferers must stay exactly zero (p_i > 0 decides the SIR gain, and a silent
// scene is divided by a peak of 1e-9), so the products skip the sources that are not live.
__device__ __forceinline__ void scene_mark_live(int* live, double re, double im, bool has_im) {
  const int any_re = __syncthreads_or(re != 0.0), any_im = __syncthreads_or(im != 0.0);
  if (threadIdx.x == 0) {
    if (any_re) live[0] = 1;
    if (has_im && any_im) live[1] = 1;
  }
}

// Sources packed two per complex signal: z[b][p][m] = src[2p][m] + i src[2p + 1][m].
__global__ void __launch_bounds__(256) scene_pack_kernel(SceneArgs A, double2* z, long long sb,
                                                         int* live) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y, p = blockIdx.z;
  const bool has_im = 2 * p + 1 < A.n_src;
  const float* y = A.src + (long long)b * A.n_src * A.n;
  double re = 0.0, im = 0.0;
  if (m < A.n) {
    re = (double)y[(long long)(2 * p) * A.n + m];
    if (has_im) im = (double)y[(long long)(2 * p + 1) * A.n + m];
    z[(long long)b * sb + (long long)p * A.n + m] = make_double2(re, im);
  }
  scene_mark_live(live + (long long)b * A.n_src + 2 * p, re, im, has_im);
}

// Frequency-domain mixing, thread per bin k <= n/2 of utterance b: source spectra from the
// packed transforms, per-mic phase ramps (irfft: imaginary parts of DC and Nyquist
// dropped), target / summed-interference images packed two mics per signal, both halves
// of the Hermitian spectrum written: zo[b][0] = T0 + i T1, zo[b][1] = I0 + i I1.
__global__ void __launch_bounds__(256) scene_phase_kernel(SceneArgs A, const double2* zf,
                                                          double2* zo, long long sb,
                                                          const int* __restrict__ live) {
  const int n = A.n, half = n / 2;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k > half) return;
  const int b = blockIdx.y;
  const int kp = (n - k) % n;
  const double f = (double)k * (1.0 / ((double)n * (1.0 / A.fs)));  // np.fft.rfftfreq
  double2 T[2] = {{0, 0}, {0, 0}}, I[2] = {{0, 0}, {0, 0}};
  for (int s = 0; s < A.n_src; ++s) {
    if (!live[(long long)b * A.n_src + s]) continue;
    const double2* zp = zf + (long long)b * sb + (long long)(s >> 1) * n;
    const double2 z = zp[k], zc = zp[kp];  // Z[k], Z[n - k]
    double2 Y;
    if ((s & 1) == 0)
      Y = make_double2(0.5 * (z.x + zc.x), 0.5 * (z.y - zc.y));  // (Z + conj Zc) / 2
    else
      Y = make_double2(0.5 * (z.y + zc.y), 0.5 * (zc.x - z.x));  // (Z - conj Zc) / 2i
#pragma unroll
    for (int mic = 0; mic < 2; ++mic) {
      double sn, cs;
      sincospi(2.0 * f * scene_tau(A, b, s, mic), &sn, &cs);  // exp(-2 pi i f tau)
      double2 h = make_double2(Y.x * cs + Y.y * sn, Y.y * cs - Y.x * sn);
      if (k == 0 || k == half) h.y = 0.0;
      double2& acc = (s == 0) ? T[mic] : I[mic];
      acc.x += h.x;
      acc.y += h.y;
    }
  }
  double2* o = zo + (long long)b * sb;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const double2 a = q ? I[0] : T[0], c = q ? I[1] : T[1];
    o[(long long)q * n + k] = make_double2(a.x - c.y, a.y + c.x);  // a + i c
    if (k != 0 && k != half)
      o[(long long)q * n + (n - k)] = make_double2(a.x + c.y, c.x - a.y);  // conj a + i conj c
  }
}

// ================================================================ O(n^2) fallback
constexpr int kConvThreads = 256;
constexpr int kConvOut = 8;                          // outputs per thread
constexpr int kConvM = kConvThreads * kConvOut;      // 2048 outputs per block
constexpr int kConvJ = 256;                          // inputs per LDS tile
constexpr int kConvH = kConvM + kConvJ;              // kernel values per tile (2304)

// A delay within kIntDelay of an integer (|sin(pi delta)| below it) is the circular shift by
// that integer: exact in the rfft model too, whose Nyquist bin exp(-i pi delta) is then real.
constexpr double kIntDelay = 1e-12;
__device__ __forceinline__ bool scene_int_shift(double delta, int n, int& shift) {
  if (!(fabs(sinpi(delta)) < kIntDelay)) return false;
  shift = (int)(llrint(delta) % n);
  if (shift < 0) shift += n;
  return true;
}

// h tables: one per (utterance, source, mic) signal, h[d] in fp64 -> fp32; an integer delay's
// table is the shift itself (1 at d = delta mod n): the cotangent form is 0 * inf there.
__global__ void __launch_bounds__(256) avz_scene_kernel_fill(SceneArgs A) {
  const long long n = A.n;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long nsig = (long long)A.batch * A.n_src * 2;
  if (idx >= nsig * n) return;
  const int sig = (int)(idx / n);
  const int d = (int)(idx % n);
  const int mic = sig & 1, s = (sig >> 1) % A.n_src, b = (sig >> 1) / A.n_src;
  const double delta = scene_tau(A, b, s, mic) * A.fs;
  int shift;
  if (scene_int_shift(delta, A.n, shift)) {
    A.hk[idx] = (d == shift) ? 1.0f : 0.0f;
    return;
  }
  // cot(pi (d - delta) / n) has period n in d: with delta = r + f, r = rint(delta), take
  // k = (d - r) mod n in [-n/2, n/2) and x = (k - f) / n. (d - delta) / n as it stands loses
  // f where d - delta is near n: at delta = -2 - 1e-9 and n = 2306 the tap of weight 1 was
  // off by 5e-4, and nearer the integer the quotient rounded to 1 and the tap to infinity.
  const double r = rint(delta), f = delta - r;
  long long k = ((long long)d - (long long)r) % n;
  if (k < 0) k += n;
  if (2 * k >= n) k -= n;
  const double x = ((double)k - f) / (double)n;
  double sn, cs;
  sincospi(x, &sn, &cs);
  const double sd = sinpi(delta);
  const double h = -(1.0 / (double)n) * ((d & 1) ? -1.0 : 1.0) * sd * (cs / sn);
  A.hk[idx] = (float)h;
}

// image[sig][m] = sum_j src[b][s][j] h[sig][(m - j) mod n]; grid (ceil(n/2048), nsig).
// Thread t owns outputs M0 + 8t .. M0 + 8t + 7; per 256-input tile the block stages the
// inputs and the 2304 kernel values they meet, and each thread slides an 8-output window
// over 16 kernel values per 8 inputs (4 ds_read_b128 + 2 broadcast reads per 64 FMAs).
__global__ void __launch_bounds__(kConvThreads) avz_scene_conv_kernel(SceneArgs A) {
  __shared__ __align__(16) float y_t[kConvJ];
  __shared__ __align__(16) float h_t[kConvH];
  const int n = A.n;
  const int sig = blockIdx.y;
  const int mic = sig & 1, s = (sig >> 1) % A.n_src, b = (sig >> 1) / A.n_src;
  const float* y = A.src + ((long long)b * A.n_src + s) * n;
  float* img = A.img + (long long)sig * n;
  const int M0 = blockIdx.x * kConvM;
  const int tid = threadIdx.x;
  // integer delay (0 for the broadside target): a copy, rotated by the delay
  int shift;
  if (scene_int_shift(scene_tau(A, b, s, mic) * A.fs, n, shift)) {
    for (int m = M0 + tid; m < min(M0 + kConvM, n); m += kConvThreads)
      img[m] = y[m >= shift ? m - shift : m - shift + n];
    return;
  }
  const float* h = A.hk + (long long)sig * n;
  float acc[kConvOut];
#pragma unroll
  for (int r = 0; r < kConvOut; ++r) acc[r] = 0.0f;
  const int hstep = kConvThreads % n;
  for (int j0 = 0; j0 < n; j0 += kConvJ) {
    __syncthreads();
    y_t[tid] = (j0 + tid < n) ? y[j0 + tid] : 0.0f;
    // h_t[i] = h[(M0 - j0 - 255 + i) mod n]: a true modulo for every n >= 2 (n may be far
    // below the 2304-entry window), stepped by 256 mod n so that no index ever reaches n
    int base = (M0 - j0 - (kConvJ - 1)) % n;
    if (base < 0) base += n;
    int d = (base + tid) % n;
    for (int i = tid; i < kConvH; i += kConvThreads) {
      h_t[i] = h[d];
      d += hstep;
      if (d >= n) d -= n;
    }
    __syncthreads();
#pragma unroll 2
    for (int q0 = 0; q0 < kConvJ; q0 += 8) {
      const int hb = kConvOut * tid - q0 + (kConvJ - 8);  // multiple of 8: 16-B aligned
      float hw[16];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float4 t4 = *reinterpret_cast<const float4*>(h_t + hb + 4 * v);
        hw[4 * v] = t4.x; hw[4 * v + 1] = t4.y; hw[4 * v + 2] = t4.z; hw[4 * v + 3] = t4.w;
      }
      const float4 ya = *reinterpret_cast<const float4*>(y_t + q0);
      const float4 yb = *reinterpret_cast<const float4*>(y_t + q0 + 4);
      const float yq[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int r = 0; r < kConvOut; ++r) acc[r] = fmaf(yq[q], hw[r - q + 7], acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < kConvOut; ++r) {
    const int m = M0 + kConvOut * tid + r;
    if (m < n) img[m] = acc[r];
  }
}

// Per-source images -> the packed target / interference layout of the FFT path (times n,
// so the mix kernel scales both paths alike).
__global__ void __launch_bounds__(256) scene_conv_pack_kernel(SceneArgs A, double2* zo,
                                                              long long sb) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= A.n) return;
  const int b = blockIdx.y;
  const long long n = A.n;
  const float* im = A.img + (long long)b * A.n_src * 2 * n;  // [src][mic][n]
  double t[2], i[2] = {0.0, 0.0};
#pragma unroll
  for (int mic = 0; mic < 2; ++mic) {
    t[mic] = (double)im[mic * n + m];
    for (int k = 1; k < A.n_src; ++k) i[mic] += (double)im[(k * 2 + mic) * n + m];
  }
  const double sc = (double)n;
  zo[(long long)b * sb + m] = make_double2(t[0] * sc, t[1] * sc);
  zo[(long long)b * sb + n + m] = make_double2(i[0] * sc, i[1] * sc);
}

// ================================================================ mixing
// One block per utterance: simulation.py:167-202 on the images.
//   tgt_m = image(target), int_m = g * sum_k image(interferer k), g for SIR sir_db on mic 1;
//   noisy = clean + sqrt(mean(clean^2) / 10^(snr/10)) * z  (world.py:93-98 add_awgn);
//   peak = max |noisy| + 1e-9 over both mics; outputs / peak.
// Images: ti[b][0][m] = nfft (T0 + i T1), ti[b][1][m] = nfft (I0 + i I1), m < n <= nfft: the
// transform length (n on the anechoic paths, the padded length of the room convolution).
constexpr int kMixThreads = 256;
__device__ __forceinline__ double block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < kMixThreads / 64; ++w) t += red[w];
  return t;
}
__device__ __forceinline__ float block_max(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.0f;
#pragma unroll
  for (int w = 0; w < kMixThreads / 64; ++w) t = fmaxf(t, red[w]);
  return t;
}

__global__ void __launch_bounds__(kMixThreads) avz_scene_mix_kernel(SceneArgs A, const double2* ti,
                                                                    long long sb, int nfft) {
  __shared__ double red[kMixThreads / 64];
  __shared__ float redf[kMixThreads / 64];
  const int b = blockIdx.x, tid = threadIdx.x, n = A.n, K = A.n_src - 1;
  const double2* T = ti + (long long)b * sb;
  const double2* I = T + nfft;
  const double sc = 1.0 / (double)nfft;
  auto tgt_img = [&](int mic, int m) -> double { return (mic ? T[m].y : T[m].x) * sc; };
  auto int_img = [&](int mic, int m) -> double { return (mic ? I[m].y : I[m].x) * sc; };
  double st = 0.0, si = 0.0;
  for (int m = tid; m < n; m += kMixThreads) {
    const double t = tgt_img(0, m), i = int_img(0, m);
    st += t * t;
    si += i * i;
  }
  const double p_t = block_sum(st, red) / n;
  const double p_i = block_sum(si, red) / n;
  const double g = (K > 0 && p_i > 0) ? sqrt(p_t / (p_i * pow(10.0, A.sir_db / 10.0))) : 1.0;
  double scl[2] = {0.0, 0.0};
  for (int m = tid; m < n; m += kMixThreads) {
#pragma unroll
    for (int mic = 0; mic < 2; ++mic) {
      const double cl = tgt_img(mic, m) + g * int_img(mic, m);
      scl[mic] += cl * cl;
    }
  }
  double sig_n[2];
#pragma unroll
  for (int mic = 0; mic < 2; ++mic) {
    const double p = block_sum(scl[mic], red) / n;
    sig_n[mic] = (p == 0.0) ? 0.0 : sqrt(p / pow(10.0, A.snr_db / 10.0));
  }
  const float* z = A.noise + (long long)b * 2 * n;
  float pk = 0.0f;
  for (int m = tid; m < n; m += kMixThreads) {
#pragma unroll
    for (int mic = 0; mic < 2; ++mic) {
      const double v = tgt_img(mic, m) + g * int_img(mic, m) + sig_n[mic] * (double)z[(long long)mic * n + m];
      pk = fmaxf(pk, (float)fabs(v));
    }
  }
  // the peak in fp64 would need a second reduction type; |v| rounded to fp32 first
  // changes 1/(peak + 1e-9) by < 1 ulp of fp32
  const double peak = (double)block_max(pk, redf) + 1e-9;
  float* mix = A.mix + (long long)b * A.mix_stride;
  for (int m = tid; m < n; m += kMixThreads) {
#pragma unroll
    for (int mic = 0; mic < 2; ++mic) {
      const double v = tgt_img(mic, m) + g * int_img(mic, m) + sig_n[mic] * (double)z[(long long)mic * n + m];
      mix[(long long)mic * A.ch_stride + m] = (float)(v / peak);
    }
    A.tgt[(long long)b * A.ref_stride + m] = (float)(tgt_img(0, m) / peak);
    A.itf[(long long)b * A.ref_stride + m] = (float)(g * int_img(0, m) / peak);
  }
}

// ================================================================ shoebox rooms
// Image-source model (Allen & Berkley 1979) of synth.room_rir: images q, |qx| + |qy| + |qz|
// <= max_order, in the order of synth.room_images (qx, then qy, then qz ascending); image
// coordinate q L + s (q even) or (q + 1) L - s (q odd); amplitude beta^order / (4 pi d) with
// beta^order by repeated multiplication; delay tau = d fs / c; 81 taps amp w(n - tau)
// sinc(n - tau) at n = floor(tau) - 40 .. + 40, w the Hann window of width 81 centred on tau.
constexpr int kRirHalf = 40;

// Orders one wave's LDS stores before its later LDS loads across lanes.
__device__ __forceinline__ void room_wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double room_lane(double v, int j) {  // lane j's v (j uniform)
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), j);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double room_image_coord(int q, double L, double s) {
#pragma clang fp contract(off)  // the host restatement's roundings
  return (q & 1) ? (double)(q + 1) * L - s : (double)q * L + s;
}

// Where sample i of RIR (b, s, mic) goes: p[b sb + s ss + mic sm + i si] (doubles).
struct RirOut {
  double* p;
  long long sb, ss;
  int sm, si;
};

// One wave per RIR (b, s, mic), accumulated in fp64 in LDS and written once. The wave walks
// the (qx, qy) rows; the lanes compute the row's <= 41 images (one per qz), then the images
// go through the wave one at a time, their 81 taps on the lanes in two passes. A wave's LDS
// operations execute in order, so every sample sums its images in room_images order on
// every call: no atomics, no block barrier. sin(pi (n - tau)) = -(-1)^k sin(pi frac) for
// n = floor(tau) + k, and the window's cosine comes from the lane's cos / sin(2 pi k / 81)
// and the image's cos / sin(2 pi frac / 81): one sinpi and one sincospi per image.
__global__ void __launch_bounds__(64) avz_room_rir_kernel(RoomArgs R, int n_src,
                                                          const double* __restrict__ src_pos,
                                                          RirOut O) {
  extern __shared__ double room_h[];
  const int lane = threadIdx.x;
  const int mic = blockIdx.x & 1;
  const long long bs = blockIdx.x >> 1;
  const int L = R.rir_len, N = R.max_order;
  for (int i = lane; i < L; i += 64) room_h[i] = 0.0;
  room_wave_lds_sync();
  const double sx = src_pos[bs * 3], sy = src_pos[bs * 3 + 1], sz = src_pos[bs * 3 + 2];
  const double mx = R.mic[mic][0], my = R.mic[mic][1], mz = R.mic[mic][2];
  double ck[2], sk[2];  // taps k = lane - 40 and lane + 24
#pragma unroll
  for (int t = 0; t < 2; ++t) sincospi(2.0 * (double)(lane - kRirHalf + 64 * t) / 81.0, &sk[t], &ck[t]);
  const double sgn = (lane & 1) ? 1.0 : -1.0;  // -(-1)^k: both taps have the lane's parity
  for (int qx = -N; qx <= N; ++qx) {
    const int rx = N - abs(qx);
    const double dx = room_image_coord(qx, R.dim[0], sx) - mx;
    for (int qy = -rx; qy <= rx; ++qy) {
      const int rz = rx - abs(qy);
      const double dy = room_image_coord(qy, R.dim[1], sy) - my;
      // lane l <= 2 rz: the image qz = l - rz
      double amp, frac, sp, sf, cf;
      int fl;
      {
#pragma clang fp contract(off)
        const int qz = lane - rz;
        const double dz = room_image_coord(qz, R.dim[2], sz) - mz;
        const double d = fmax(sqrt(dx * dx + dy * dy + dz * dz), 1e-3);
        double bp = 1.0;
        for (int o = abs(qx) + abs(qy) + abs(qz); o > 0; --o) bp *= R.beta;
        amp = bp / (4.0 * M_PI * d);
        const double tau = d * R.fs / R.c_sound;
        // an image past the RIR (or a non-finite source position) leaves no tap inside
        const bool in = tau < (double)(L + kRirHalf + 1);
        const double ft = in ? floor(tau) : 0.0;
        fl = in ? (int)ft : -(1 << 20);
        frac = in ? tau - ft : 0.0;
        sp = sinpi(frac);
        sincospi(2.0 * frac / 81.0, &sf, &cf);
      }
      for (int j = 0; j <= 2 * rz; ++j) {
        const double a_j = room_lane(amp, j), f_j = room_lane(frac, j), sp_j = room_lane(sp, j);
        const double sf_j = room_lane(sf, j), cf_j = room_lane(cf, j);
        const int fl_j = __builtin_amdgcn_readlane(fl, j);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma clang fp contract(off)
          const int k = lane - kRirHalf + 64 * t;
          const double x = (double)k - f_j;
          const int n = fl_j + k;
          if (k <= kRirHalf && n >= 0 && n < L && fabs(x) <= 40.5) {
            const double w = 0.5 * (1.0 + (ck[t] * cf_j + sk[t] * sf_j));
            const double sinc = (x == 0.0) ? 1.0 : sgn * sp_j / (M_PI * x);
            room_h[n] += a_j * w * sinc;
          }
          room_wave_lds_sync();
        }
      }
    }
  }
  double* o = O.p + (long long)(bs / n_src) * O.sb + (long long)(bs % n_src) * O.ss +
              (long long)mic * O.sm;
  for (int i = lane; i < L; i += 64) o[(long long)i * O.si] = room_h[i];
}

// Sources packed two per complex signal and zero padded to the convolution length Lc.
__global__ void __launch_bounds__(256) room_pack_kernel(SceneArgs A, double2* z, long long sb,
                                                        int Lc, int* live) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y, p = blockIdx.z;
  const bool has_im = 2 * p + 1 < A.n_src;
  const float* y = A.src + (long long)b * A.n_src * A.n;
  double re = 0.0, im = 0.0;
  if (m < A.n) {
    re = (double)y[(long long)(2 * p) * A.n + m];
    if (has_im) im = (double)y[(long long)(2 * p + 1) * A.n + m];
  }
  if (m < Lc) z[(long long)b * sb + (long long)p * Lc + m] = make_double2(re, im);
  scene_mark_live(live + (long long)b * A.n_src + 2 * p, re, im, has_im);
}

// Zero padding of the packed RIR signals h0 + i h1 (signals P .. P + n_src - 1).
__global__ void __launch_bounds__(256) room_pad_kernel(double2* z, long long sb, int P, int rir_len,
                                                       int Lc) {
  const int m = rir_len + blockIdx.x * 256 + threadIdx.x;
  if (m >= Lc) return;
  z[(long long)blockIdx.y * sb + (long long)(P + blockIdx.z) * Lc + m] = make_double2(0.0, 0.0);
}

// Thread per bin k < Lc of utterance b: the real source's spectrum Y_s (from the packed
// transform) times the spectrum of h0 + i h1 is the spectrum of image0 + i image1; summed
// over the target and over the interferers: zo[b][0] = T0 + i T1, zo[b][1] = I0 + i I1.
__global__ void __launch_bounds__(256) room_product_kernel(const double2* zf, double2* zo,
                                                           int n_src, int Lc, long long sb,
                                                           const int* __restrict__ live) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= Lc) return;
  const int b = blockIdx.y;
  const int kp = (Lc - k) % Lc;
  const int P = (n_src + 1) / 2;
  const double2* zb = zf + (long long)b * sb;
  double2 T = {0, 0}, I = {0, 0};
  for (int s = 0; s < n_src; ++s) {
    if (!live[(long long)b * n_src + s]) continue;
    const double2* zp = zb + (long long)(s >> 1) * Lc;
    const double2 z = zp[k], zc = zp[kp];
    double2 Y;
    if ((s & 1) == 0)
      Y = make_double2(0.5 * (z.x + zc.x), 0.5 * (z.y - zc.y));  // (Z + conj Zc) / 2
    else
      Y = make_double2(0.5 * (z.y + zc.y), 0.5 * (zc.x - z.x));  // (Z - conj Zc) / 2i
    const double2 H = zb[(long long)(P + s) * Lc + k];
    double2& acc = (s == 0) ? T : I;
    acc.x += Y.x * H.x - Y.y * H.y;
    acc.y += Y.x * H.y + Y.y * H.x;
  }
  double2* o = zo + (long long)b * sb;
  o[k] = T;
  o[(long long)Lc + k] = I;
}

// Source positions of the reverberant generator: the target, interferer 1, and interferers
// 2.. at (1 + u0 (dim_x - 2), 1 + u1 (dim_y - 2), target z) (simulation.py:133-136).
struct RoomPos {
  double t[3], i[3];
};
__global__ void __launch_bounds__(64) room_pos_kernel(GenArgs G, RoomArgs R, RoomPos Q, double* pos) {
#pragma clang fp contract(off)
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= G.batch * G.n_src) return;
  const int b = t / G.n_src, s = t % G.n_src;
  double* p = pos + (long long)t * 3;
  if (s < 2) {
    for (int a = 0; a < 3; ++a) p[a] = s ? Q.i[a] : Q.t[a];
    return;
  }
  uint32_t k0, k1;
  gen_key(G, b, k0, k1);
  const uint32_t j = kUnifPos + 2u * (uint32_t)(s - 2);
  p[0] = 1.0 + uniform(k0, k1, j) * (R.dim[0] - 2.0);
  p[1] = 1.0 + uniform(k0, k1, j + 1u) * (R.dim[1] - 2.0);
  p[2] = Q.t[2];
}

}  // namespace avz

using namespace avz;

extern "C" int avz_scene_fft_len(int n) {
  int rad[32];
  return n > 1 && fft_factor(n, rad) > 0;
}

// The live flags [B][n_src] int behind the packed transforms.
static long long live_bytes(int batch, int n_src) {
  return ((long long)batch * n_src * (long long)sizeof(int) + 255) & ~255LL;
}

// Workspace of the mixing back end: FFT path 2 x [B][max(ceil(n_src/2), 2)][n] double2 and
// the live flags; fallback: fp32 kernels + images [B][n_src][2][n] each, and [B][2][n] double2.
extern "C" long long avz_scene_mix_ws(int batch, int n_src, int n) {
  int rad[32];
  const long long B = batch, N = n;
  if (fft_factor(n, rad) > 0) {
    const long long nz = std::max((n_src + 1) / 2, 2);
    return 2 * B * nz * N * (long long)sizeof(double2) + live_bytes(batch, n_src);
  }
  return 2 * B * n_src * 2 * N * (long long)sizeof(float) + B * 2 * N * (long long)sizeof(double2);
}

extern "C" int avz_launch_scene(const SceneArgs* a, void* ws, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int B = a->batch, n = a->n;
  int rad[32];
  if (fft_factor(n, rad) > 0) {
    const int nz = std::max((a->n_src + 1) / 2, 2);
    const long long sb = (long long)nz * n;
    double2* z0 = static_cast<double2*>(ws);
    double2* z1 = z0 + (long long)B * sb;
    const int P = (a->n_src + 1) / 2;
    int* live = reinterpret_cast<int*>(z1 + (long long)B * sb);
    if (hipMemsetAsync(live, 0, (size_t)B * a->n_src * sizeof(int), st) != hipSuccess) return -3;
    hipLaunchKernelGGL(scene_pack_kernel, dim3((n + 255) / 256, B, P), dim3(256), 0, st, *a, z0, sb,
                       live);
    double2* f = fft_run(z0, z1, n, B, P, sb, -1.0, st);
    double2* o = (f == z0) ? z1 : z0;
    hipLaunchKernelGGL(scene_phase_kernel, dim3((n / 2 + 1 + 255) / 256, B), dim3(256), 0, st, *a,
                       (const double2*)f, o, sb, (const int*)live);
    double2* t = fft_run(o, f, n, B, 2, sb, 1.0, st);
    hipLaunchKernelGGL(avz_scene_mix_kernel, dim3(B), dim3(kMixThreads), 0, st, *a,
                       (const double2*)t, sb, n);
  } else {
    SceneArgs c = *a;
    const long long per = (long long)B * a->n_src * 2 * n;
    c.hk = static_cast<float*>(ws);
    c.img = c.hk + per;
    double2* zo = reinterpret_cast<double2*>(c.img + per);
    const long long nsig = (long long)B * a->n_src * 2;
    hipLaunchKernelGGL(avz_scene_kernel_fill, dim3((unsigned)((nsig * n + 255) / 256)), dim3(256), 0,
                       st, c);
    hipLaunchKernelGGL(avz_scene_conv_kernel, dim3((n + kConvM - 1) / kConvM, (unsigned)nsig),
                       dim3(kConvThreads), 0, st, c);
    hipLaunchKernelGGL(scene_conv_pack_kernel, dim3((n + 255) / 256, B), dim3(256), 0, st, c, zo,
                       2LL * n);
    hipLaunchKernelGGL(avz_scene_mix_kernel, dim3(B), dim3(kMixThreads), 0, st, c,
                       (const double2*)zo, 2LL * n, n);
  }
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// Generation scratch: sources, noise, angles and the AR(2) segment states; the mixing
// back end's workspace follows it.
static long long gen_scratch(int batch, int n_src, int n) {
  const long long nseg = (n + kSegLen - 1) / kSegLen;
  auto al = [](long long x) { return (x + 255) & ~255LL; };
  return al((long long)batch * n_src * n * 4) + al((long long)batch * 2 * n * 4) +
         al((long long)batch * n_src * 8) + 2 * al((long long)batch * n_src * nseg * 16);
}

extern "C" long long avz_scene_gen_ws(int batch, int n_src, int n) {
  return gen_scratch(batch, n_src, n) + avz_scene_mix_ws(batch, n_src, n);
}

// Front end of both generators: the sources and the noise of utterances start .. start +
// B - 1 (and the anechoic azimuths) into the scratch at ws; returns the first byte after it.
// The back ends write only behind the returned pointer, so after a generate call the head of
// the workspace still holds sources [B][S][n] fp32, noise [B][2][n] fp32 and angles [B][S]
// fp64, each padded to 256 B: tests/test_gpu_scene_stages.py reads them back there.
static char* gen_front(SceneArgs* a, long long start, uint32_t seed, void* ws, hipStream_t st,
                       GenArgs& g) {
  const int B = a->batch, S = a->n_src, n = a->n;
  auto al = [](long long x) { return (x + 255) & ~255LL; };
  char* p = static_cast<char*>(ws);
  g = GenArgs{};
  g.batch = B;
  g.n_src = S;
  g.n = n;
  g.nseg = (n + kSegLen - 1) / kSegLen;
  g.start = start;
  g.seed = seed;
  g.fs = a->fs;
  g.src = reinterpret_cast<float*>(p);
  p += al((long long)B * S * n * 4);
  g.noise = reinterpret_cast<float*>(p);
  p += al((long long)B * 2 * n * 4);
  g.angles = reinterpret_cast<double*>(p);
  p += al((long long)B * S * 8);
  g.zs = reinterpret_cast<double*>(p);
  p += al((long long)B * S * g.nseg * 16);
  g.sin_ = reinterpret_cast<double*>(p);
  p += al((long long)B * S * g.nseg * 16);
  const long long nar = (long long)B * S * g.nseg;
  hipLaunchKernelGGL(scene_ar_kernel<false>, dim3((unsigned)((nar + 255) / 256)), dim3(256), 0, st, g);
  hipLaunchKernelGGL(scene_ar_scan_kernel, dim3((B * S + 63) / 64), dim3(64), 0, st, g);
  hipLaunchKernelGGL(scene_ar_kernel<true>, dim3((unsigned)((nar + 255) / 256)), dim3(256), 0, st, g);
  const long long nn = (long long)B * 2 * ((n + 1) / 2);  // normal pairs
  hipLaunchKernelGGL(scene_noise_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, g);
  a->src = g.src;
  a->noise = g.noise;
  a->angles_deg = g.angles;
  return p;
}

extern "C" int avz_launch_scene_generate(SceneArgs* a, long long start, uint32_t seed, void* ws,
                                         void* stream) {
  GenArgs g;
  char* p = gen_front(a, start, seed, ws, (hipStream_t)stream, g);
  if (hipGetLastError() != hipSuccess) return -3;
  return avz_launch_scene(a, p, stream);
}

// ================================================================ shoebox rooms: host side
extern "C" long long avz_room_rir_samples(const double* dim, int max_order, double fs,
                                          double c_sound) {
  double dmax = 0.0;
  for (int a = 0; a < 3; ++a) {
    double q = (max_order + 1) * dim[a];
    q *= q;
    for (int o = 0; o < 3; ++o)
      if (o != a) q += dim[o] * dim[o];
    dmax = std::max(dmax, std::sqrt(q));
  }
  const double v = std::floor(fs / c_sound * dmax) + 42.0;
  return v < 1e15 ? (long long)v : (long long)1e15;
}

extern "C" int avz_room_conv_len(int n, int rir_len) {
  int rad[32];
  int m = n + rir_len - 1;
  while (fft_factor(m, rad) == 0) ++m;
  return m;
}

static void room_rir_launch(const RoomArgs* r, int batch, int n_src, const double* src_pos,
                            const RirOut& o, hipStream_t st) {
  hipLaunchKernelGGL(avz_room_rir_kernel, dim3((unsigned)(2LL * batch * n_src)), dim3(64),
                     (size_t)r->rir_len * sizeof(double), st, *r, n_src, src_pos, o);
}

extern "C" int avz_launch_room_rir(const RoomArgs* r, int batch, int n_src, const double* src_pos,
                                   double* rir, void* stream) {
  const long long L = r->rir_len;
  room_rir_launch(r, batch, n_src, src_pos, RirOut{rir, 2 * L * n_src, 2 * L, (int)L, 1},
                  (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// Workspace of the reverberant back end: 2 x [B][ceil(n_src/2) + n_src][Lc] double2 (the
// packed sources and the packed RIRs, ping-pong) and the live flags.
extern "C" long long avz_scene_reverb_ws(const RoomArgs* r, int batch, int n_src, int n) {
  const long long nz = (n_src + 1) / 2 + n_src;
  return 2LL * batch * nz * avz_room_conv_len(n, r->rir_len) * (long long)sizeof(double2) +
         live_bytes(batch, n_src);
}

extern "C" int avz_launch_scene_reverb(const RoomArgs* r, const SceneArgs* a, void* ws,
                                       void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const int B = a->batch, S = a->n_src, n = a->n, P = (S + 1) / 2, L = r->rir_len;
  const int Lc = avz_room_conv_len(n, L);
  const long long sb = (long long)(P + S) * Lc;
  double2* z0 = static_cast<double2*>(ws);
  double2* z1 = z0 + (long long)B * sb;
  int* live = reinterpret_cast<int*>(z1 + (long long)B * sb);
  if (hipMemsetAsync(live, 0, (size_t)B * S * sizeof(int), st) != hipSuccess) return -3;
  hipLaunchKernelGGL(room_pack_kernel, dim3((Lc + 255) / 256, B, P), dim3(256), 0, st, *a, z0, sb, Lc,
                     live);
  // RIRs straight into the packed layout: mic 0 the real part, mic 1 the imaginary part
  room_rir_launch(r, B, S, a->angles_deg,
                  RirOut{reinterpret_cast<double*>(z0 + (long long)P * Lc), 2 * sb, 2LL * Lc, 1, 2}, st);
  if (Lc > L)
    hipLaunchKernelGGL(room_pad_kernel, dim3((Lc - L + 255) / 256, B, S), dim3(256), 0, st, z0, sb,
                       P, L, Lc);
  double2* f = fft_run(z0, z1, Lc, B, P + S, sb, -1.0, st);
  double2* o = (f == z0) ? z1 : z0;
  hipLaunchKernelGGL(room_product_kernel, dim3((Lc + 255) / 256, B), dim3(256), 0, st,
                     (const double2*)f, o, S, Lc, sb, (const int*)live);
  double2* t = fft_run(o, f, Lc, B, 2, sb, 1.0, st);
  hipLaunchKernelGGL(avz_scene_mix_kernel, dim3(B), dim3(kMixThreads), 0, st, *a,
                     (const double2*)t, sb, Lc);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

static long long room_pos_bytes(int batch, int n_src) {
  return ((long long)batch * n_src * 3 * 8 + 255) & ~255LL;
}

extern "C" long long avz_scene_reverb_gen_ws(const RoomArgs* r, int batch, int n_src, int n) {
  return gen_scratch(batch, n_src, n) + room_pos_bytes(batch, n_src) +
         avz_scene_reverb_ws(r, batch, n_src, n);
}

extern "C" int avz_launch_scene_reverb_generate(const RoomArgs* r, SceneArgs* a, long long start,
                                                uint32_t seed, const double* target_pos,
                                                const double* interferer_pos, void* ws,
                                                void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GenArgs g;
  char* p = gen_front(a, start, seed, ws, st, g);
  double* pos = reinterpret_cast<double*>(p);
  p += room_pos_bytes(a->batch, a->n_src);
  RoomPos q;
  for (int i = 0; i < 3; ++i) {
    q.t[i] = target_pos[i];
    q.i[i] = interferer_pos[i];
  }
  hipLaunchKernelGGL(room_pos_kernel, dim3((a->batch * a->n_src + 63) / 64), dim3(64), 0, st, g, *r,
                     q, pos);
  a->angles_deg = pos;
  if (hipGetLastError() != hipSuccess) return -3;
  return avz_launch_scene_reverb(r, a, p, stream);
}
