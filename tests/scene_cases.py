"""Seeded inputs and fp64 references of the scene-generator tests (test_scene_reference.py,
test_gpu_scene_stages.py): csrc/avz_scene.hip stage by stage, at the lengths where its kernels
take another path. numpy / scipy and avz.synth's host restatements only; nothing here needs
the GPU or the library.

The mixing reference is synth.mix_draws / synth._mix_images kept in fp64 WITHOUT the final
fp32 cast, applied to the fp32-rounded sources, noise and the angles the device is given, so
the device and the reference see the same inputs (mix_reference). Besides the outputs it
returns the fp64 peak, the SIR gain and, for the O(n^2) fallback, a per-sample error bound.

Tolerances (derived, not measured):

* FFT path and copies (fft_tol): 2^-22 |ref| + 2^-40 per sample. The output is one fp32
  rounding of a value <= 1 (relative 2^-24) and the peak enters as an fp32-rounded maximum
  (another 2^-24): 2^-23 together, and a factor 2 over that. The fp64 transforms, sums and
  gains differ from numpy's by some 1e-15, far below 2^-40 = 9.1e-13.
* Fallback (mix_reference(...)["bound"]): the kernel sums image[m] = sum_j y[j] h32[(m - j)
  mod n] in fp32 with FMAs. Rounding h to fp32 (one 2^-24 per tap), n FMAs (the classic
  n 2^-24 sum |terms|) and the fp32 store give |d image| <= E = (n + 2) 2^-24 (|y| (*) |h|)[m],
  (*) the circular convolution; E = 0 for a signal whose delay is an integer, which is a copy.
  To first order that perturbation moves the SIR gain g = sqrt(p_t / (p_i 10^(sir/10))) by
  |dg| <= g (mean(|T0| E_T0) / p_t + mean(|I0| E_I0) / p_i), the clean channel by
  E_cl = E_T + g E_I + |dg| |I|, the noise scale s = sqrt(p_cl / 10^(snr/10)) by
  |ds| <= s mean(|cl| E_cl) / p_cl, the noisy channel by E_v = E_cl + |ds| |z| and the peak by
  at most max E_v; an output o = v / peak then moves by E_v / peak + |o| max(E_v) / peak, and
  the FFT-path term is added. The GPU test takes the smaller of this and the project's 2e-5.
* Generated draws (draw_tol): 2^-24 |ref| + 2^-40 max|ref|: the fp32 store, and the fp64
  differences of log, sin / cos and of the segment scan against lfilter (whose l1 gain is 20).
"""
import functools
from collections import namedtuple

import numpy as np

from avz import synth

FS = 16000.0
C_SOUND = 343.0
U24 = 2.0 ** -24
ANGLES = (0.0, 40.0, 90.0, 180.0, 217.3, -30.0)
INT_DELAY = 1e-12          # |sin(pi delta)| below this: the kernels' integer-delay branch
PROJECT_TOL = 2e-5         # test_gpu_scene.py


def fft_tol(ref):
    return 2.0 ** -22 * np.abs(ref) + 2.0 ** -40


def draw_tol(ref):
    ref = np.asarray(ref)
    return U24 * np.abs(ref) + 2.0 ** -40 * np.max(np.abs(ref), axis=-1, keepdims=True)


def fft_len(n):
    """avz_scene_fft_len: n = 2^a 3^b 5^c."""
    for r in (2, 3, 5):
        while n % r == 0:
            n //= r
    return n == 1


def delays(angle_deg, mic_d, c, fs):
    """delta (samples) at the two mics: world_building.py:47-51 as scene_tau evaluates it."""
    th = angle_deg * (np.pi / 180.0)
    return ((mic_d / 2) * np.cos(th - 0.0) / c * fs, (mic_d / 2) * np.cos(th - np.pi) / c * fs)


def sinpi(x):
    """sin(pi x) with the argument reduced first, as the device's sinpi."""
    r = np.rint(x)
    return np.where(r % 2 == 0, 1.0, -1.0) * np.sin(np.pi * (x - r))


def is_int_delay(delta):
    return abs(sinpi(delta)) < INT_DELAY


def periodic_kernel(n, delta):
    """h[d] = -(1/n) (-1)^d sin(pi delta) cot(pi (d - delta) / n) in fp64 (n even): the circular
    kernel of the rfft phase shift with irfft's real Nyquist bin; the shift itself for an
    integer delta. The cotangent has period n in d, so with delta = r + f (r the nearest
    integer) its argument is taken as (k - f) / n, k = (d - r) mod n in [-n/2, n/2): d - delta
    itself loses f where it is near n."""
    d = np.arange(n)
    r = int(np.rint(delta))
    if is_int_delay(delta):
        return (d == r % n).astype(np.float64)
    k = (d - r) % n
    k = np.where(2 * k >= n, k - n, k)
    x = np.pi * (k - (delta - r)) / n
    return -(1.0 / n) * np.where(d & 1, -1.0, 1.0) * sinpi(delta) * (np.cos(x) / np.sin(x))


def cconv(y, h):
    """sum_j y[j] h[(m - j) mod n] in fp64, directly."""
    n = len(y)
    idx = (np.arange(n)[:, None] - np.arange(n)[None, :]) % n
    return (h[idx] * y[None, :]).sum(axis=1)


def cconv_fft(a, b):
    """Circular convolution by rfft (for the non-negative sums of the error bound)."""
    return np.fft.irfft(np.fft.rfft(a) * np.fft.rfft(b), n=len(a))


def mix_images(T, I, K, z, sir_db, snr_db, ET=None, EI=None):
    """synth._mix_images in fp64 without its fp32 cast, on images T, I [2, n] and noise z
    [2, n]; with per-sample image error bounds ET, EI it also propagates them (module
    docstring). Returns dict(mix [2, n], tgt, itf [n], peak, g, b_mix, b_tgt, b_itf)."""
    n = T.shape[-1]
    ET = np.zeros((2, n)) if ET is None else ET
    EI = np.zeros((2, n)) if EI is None else EI
    p_t, p_i = np.mean(T[0] ** 2), np.mean(I[0] ** 2)
    g, dg = 1.0, 0.0
    if K > 0 and p_i > 0:
        g = np.sqrt(p_t / (p_i * 10 ** (sir_db / 10)))
        dg = g * ((np.mean(np.abs(T[0]) * ET[0]) / p_t if p_t > 0 else 0.0)
                  + np.mean(np.abs(I[0]) * EI[0]) / p_i)
    Ig = g * I
    EIg = g * EI + dg * np.abs(I)
    v = np.zeros((2, n))
    Ev = np.zeros((2, n))
    for mic in range(2):
        cl = T[mic] + Ig[mic]
        Ecl = ET[mic] + EIg[mic]
        p = np.mean(cl ** 2)
        sg = 0.0 if p == 0 else np.sqrt(p / 10 ** (snr_db / 10))
        ds = 0.0 if p == 0 else sg * np.mean(np.abs(cl) * Ecl) / p
        v[mic] = cl + sg * z[mic]
        Ev[mic] = Ecl + ds * np.abs(z[mic])
    peak = np.max(np.abs(v)) + 1e-9
    dpk = np.max(Ev) / peak
    r = dict(mix=v / peak, tgt=T[0] / peak, itf=Ig[0] / peak, peak=peak, g=g)
    for key, E in (("mix", Ev), ("tgt", ET[0]), ("itf", EIg[0])):
        r["b_" + key] = E / peak + np.abs(r[key]) * dpk
    return r


def mix_reference(angles, srcs, noise, mic_d, c=C_SOUND, fs=FS, sir_db=0.0, snr_db=5.0):
    """fp64 mixing of one batch: angles [B, S] fp64, srcs [B, S, n] and noise [B, 2, n] as the
    device holds them (fp32). Returns dict(mix [B, 2, n], tgt, itf [B, n] fp64, peak, g [B],
    b_mix, b_tgt, b_itf: the fallback bound without its FFT-path term (zero on the FFT lengths
    and for copies), tol_mix, tol_tgt, tol_itf = fft_tol(ref) + that bound)."""
    angles = np.asarray(angles, np.float64)
    srcs = np.asarray(srcs, np.float32).astype(np.float64)
    noise = np.asarray(noise, np.float32).astype(np.float64)
    B, S, n = srcs.shape
    fb = not fft_len(n)
    rows = []
    for b in range(B):
        T, I, ET, EI = (np.zeros((2, n)) for _ in range(4))
        for s in range(S):
            dl = delays(angles[b, s], mic_d, c, fs)
            for mic in range(2):
                (T if s == 0 else I)[mic] += synth.frac_delay(srcs[b, s], dl[mic] / fs, fs)
                if fb and not is_int_delay(dl[mic]):
                    (ET if s == 0 else EI)[mic] += (n + 2) * U24 * cconv_fft(
                        np.abs(srcs[b, s]), np.abs(periodic_kernel(n, dl[mic])))
        rows.append(mix_images(T, I, S - 1, noise[b], sir_db, snr_db, ET, EI))
    out = {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
    for k in ("mix", "tgt", "itf"):
        out["tol_" + k] = fft_tol(out[k]) + out["b_" + k]
    return out


# ----------------------------------------------------------------------------- cases
MixCase = namedtuple("MixCase", "name n S B mic_d c fs sir snr angles zero")


def _angles(B, S, rot):
    return np.array([[ANGLES[(rot + 2 * b + 3 * s) % len(ANGLES)] for s in range(S)]
                     for b in range(B)])


def _mc(name, n, S, B=3, mic_d=0.08, c=C_SOUND, fs=FS, sir=0.0, snr=5.0, angles=None, rot=0,
        zero=()):
    a = _angles(B, S, rot) if angles is None else np.broadcast_to(
        np.asarray(angles, np.float64), (B, S)).copy()
    return MixCase(name, n, S, B, mic_d, c, fs, sir, snr, a, tuple(zero))


FFT_LENGTHS = (2, 4, 6, 8, 10, 12, 16, 20, 30, 48, 64, 162, 250, 360, 4320)
FB_LENGTHS = (14, 22, 34, 62, 126, 134, 254, 258, 1150, 1154, 2046, 2050, 2306, 4094, 4102)
INT_D, INT_C = 0.085, 340.0        # (0.0425 / 340) 16000 = 2.0 exactly at 0 and 180 degrees


def _fft_cases():
    out = []
    for i, n in enumerate(FFT_LENGTHS):
        # n_src 1 .. 5 in turn; the spacing in turn 0.08, 1.0 (|delta| to 23 samples, beyond n
        # at the small lengths) and 0.3 m
        out.append(_mc(f"fft-n{n}", n, 1 + i % 5, mic_d=(0.08, 1.0, 0.3)[i % 3], rot=i))
    out.append(_mc("fft-n4320-S4", 4320, 4, mic_d=1.0, rot=2))
    out.append(_mc("fft-n162-S5", 162, 5, mic_d=1.0, rot=1))
    out.append(_mc("fft-n250-S3", 250, 3, mic_d=1.0, rot=3))
    out.append(_mc("fft-n30-int", 30, 3, mic_d=INT_D, c=INT_C, angles=[0.0, 180.0, 0.0]))
    out.append(_mc("fft-n8-int", 8, 2, mic_d=INT_D * 5, c=INT_C, angles=[180.0, 0.0]))  # +-10 > n
    out.append(_mc("fft-n48-zero", 48, 3, mic_d=0.0))
    return out


def _fb_cases():
    out = []
    for i, n in enumerate(FB_LENGTHS):
        out.append(_mc(f"fb-n{n}", n, 1 + i % 3, B=2, mic_d=(1.0, 0.08, 0.3)[i % 3], rot=i))
    for n in (14, 126, 1150, 2306):
        # +-2 exactly on every signal of utterance 0 (copies); utterance 1 fractional
        out.append(_mc(f"fb-n{n}-int", n, 3, B=2, mic_d=INT_D, c=INT_C,
                       angles=[[0.0, 180.0, 0.0], [40.0, 217.3, -30.0]]))
        # 2 + 1e-9: |sin(pi delta)| = 3e-9, just above the branch threshold
        out.append(_mc(f"fb-n{n}-near-int", n, 2, B=2, mic_d=INT_D * (1 + 0.5e-9), c=INT_C,
                       angles=[[0.0, 180.0], [180.0, 0.0]]))
    out.append(_mc("fb-n34-zero", 34, 3, B=2, mic_d=0.0))
    out.append(_mc("fb-n2050-broadside", 2050, 2, B=2, mic_d=0.3, angles=[[90.0, 40.0], [90.0, -30.0]]))
    out.append(_mc("fb-n14-far", 14, 3, B=2, mic_d=1.0, angles=[[0.0, 180.0, 40.0], [180.0, 0.0, -30.0]]))
    return out


def _edge_cases():
    out = []
    for n, p in ((30, "fft"), (34, "fb")):
        kw = dict(B=2, mic_d=0.3, rot=1)
        out += [_mc(f"edge-{p}-K0", n, 1, **kw),
                _mc(f"edge-{p}-K0-silent", n, 1, zero=(0,), **kw),
                _mc(f"edge-{p}-silent-target", n, 3, zero=(0,), **kw),
                _mc(f"edge-{p}-silent-interferers", n, 3, zero=(1, 2), **kw),
                _mc(f"edge-{p}-sir+20", n, 3, sir=20.0, **kw),
                _mc(f"edge-{p}-sir-20", n, 2, sir=-20.0, **kw),
                _mc(f"edge-{p}-snr-10", n, 2, snr=-10.0, **kw),
                _mc(f"edge-{p}-snr60", n, 3, snr=60.0, **kw)]
    return out


FFT_CASES, FB_CASES, EDGE_CASES = _fft_cases(), _fb_cases(), _edge_cases()
BY_NAME = {c.name: c for c in FFT_CASES + FB_CASES + EDGE_CASES}


@functools.lru_cache(maxsize=None)
def mix_inputs(name):
    """(srcs [B, S, n] float32, noise [B, 2, n] float32) of a mixing case, seeded by its name."""
    c = BY_NAME[name]
    rng = np.random.default_rng([sum(map(ord, name)), c.n, c.S])
    srcs = (0.5 * rng.standard_normal((c.B, c.S, c.n))).astype(np.float32)
    for s in c.zero:
        srcs[:, s] = 0.0
    noise = rng.standard_normal((c.B, 2, c.n)).astype(np.float32)
    for a in (srcs, noise):
        a.setflags(write=False)
    return srcs, noise


@functools.lru_cache(maxsize=None)
def mix_case_reference(name):
    c = BY_NAME[name]
    srcs, noise = mix_inputs(name)
    ref = mix_reference(c.angles, srcs, noise, c.mic_d, c.c, c.fs, c.sir, c.snr)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def case_deltas(c):
    """delta [B, S, 2] of a mixing case."""
    return np.array([[delays(c.angles[b, s], c.mic_d, c.c, c.fs) for s in range(c.S)]
                     for b in range(c.B)])


# ----------------------------------------------------------------------------- fallback sums
def fallback_image_fp32(y, h32):
    """The kernel's sum for one signal, emulated in fp32: for each output, the inputs in
    ascending j, acc = fl(acc + fl(y[j] h[(m - j) mod n])). (The kernel fuses the multiply and
    the add, which rounds once: its error is not larger.)"""
    n = len(y)
    y = np.asarray(y, np.float32)
    m = np.arange(n)
    acc = np.zeros(n, np.float32)
    for j in range(n):
        acc = (acc + y[j] * h32[(m - j) % n]).astype(np.float32)
    return acc


# ----------------------------------------------------------------------------- AR(2) scan
SEG = 256


def ar2_segment_scan(x):
    """lfilter([1], [1, -1.4, 0.45]) as the generator runs it: zero-state segments of 256, the
    states carried across segments by A^256 (A the companion matrix, by repeated
    multiplication), then every segment again from its true entering state."""
    n = len(x)
    nseg = -(-n // SEG)

    def run(seg, y1, y2):
        out = []
        for v in x[seg * SEG:min(n, (seg + 1) * SEG)]:
            y = v + 1.4 * y1 - 0.45 * y2
            y2, y1 = y1, y
            out.append(y)
        return np.array(out), y1, y2

    zs = [run(j, 0.0, 0.0)[1:] for j in range(nseg)]
    M = np.eye(2)
    for _ in range(SEG):
        M = np.array([[1.4 * M[0, 0] - 0.45 * M[1, 0], 1.4 * M[0, 1] - 0.45 * M[1, 1]],
                      [M[0, 0], M[0, 1]]])
    y1 = y2 = 0.0
    out = []
    for j in range(nseg):
        out.append(run(j, y1, y2)[0])
        y1, y2 = (M[0, 0] * y1 + M[0, 1] * y2 + zs[j][0], M[1, 0] * y1 + M[1, 1] * y2 + zs[j][1])
    return np.concatenate(out)


# ----------------------------------------------------------------------------- generator
GenCase = namedtuple("GenCase", "name n fs K start seed B mic_d")
GEN_CASES = [
    GenCase("gen-n2", 2, 20.0, 0, 0, 0, 3, 5.0),
    GenCase("gen-n14-fb", 14, 20.0, 2, 0, 7, 2, 30.0),
    GenCase("gen-n254-fb", 254, 100.0, 1, 0, 7, 2, 8.0),
    GenCase("gen-n256", 256, 100.0, 2, 2 ** 33 + 5, 0, 2, 8.0),
    GenCase("gen-n258-fb-fs20", 258, 20.0, 4, 0, 0, 2, 30.0),
    GenCase("gen-n512-fs20-wrap", 512, 20.0, 2, 2 ** 32 - 2, 7, 4, 30.0),
    GenCase("gen-n1000-fs4", 1000, 4.0, 1, 0, 0, 2, 100.0),
    GenCase("gen-n2306-fb", 2306, 1000.0, 1, 3, 7, 2, 1.0),
    GenCase("gen-n8192", 8192, FS, 2, 5, 0, 2, 0.08),
]
GEN_BY_NAME = {c.name: c for c in GEN_CASES}


@functools.lru_cache(maxsize=None)
def gen_reference(name):
    """Host draws of a generator case: (angles [B, S], sources [B, S, n], noise [B, 2, n]) fp64
    from synth.scene_draws_philox (speech_like_philox, philox_normals)."""
    c = GEN_BY_NAME[name]
    d = [synth.scene_draws_philox(c.start + b, c.n, c.K, c.fs, c.seed) for b in range(c.B)]
    out = tuple(np.stack([u[i] for u in d]) for i in range(3))
    for v in out:
        v.setflags(write=False)
    return out


def gen_layout(B, S, n):
    """Byte offsets (sources, noise, angles) of the generation scratch at the head of the
    workspace: [B][S][n] fp32, [B][2][n] fp32, [B][S] fp64, each padded to 256 B
    (csrc/avz_scene.hip gen_front)."""
    al = lambda x: (x + 255) & ~255  # noqa: E731
    o_noise = al(B * S * n * 4)
    return 0, o_noise, o_noise + al(B * 2 * n * 4)


# the odd lengths reach the generator only through avz_scene_reverb_generate
# (room: room_cases.ROOM_B with absorption 0.3, max_order 3)
REVERB_GEN = dict(lengths=(255, 257), K=1, B=2, start=8, seed=7,
                  target_pos=[0.4, 0.7, 1.9], interferer_pos=[2.7, 2.2, 0.3])
