"""Deterministic synthetic 2-mic scenes (the bench/test input generator).

LJ-Speech cannot be fetched offline, so sources are "speech-like" (SURVEY.md 8(d)):
Gaussian noise -> AR(2) spectral tilt (poles 0.9, 0.5) x a 4 Hz syllabic envelope
with 25 % of 250-ms blocks silenced; rng seed 1000 + utterance index.

Mixing follows the reference's anechoic far-field model:
* delays  — full_audio_generating_pipeline/world_building.py:47-51
* frac delay by rfft phase shift — world_building.py:53-59
* interference gain for SIR 0 dB on mic 1 — Final_pipeline/src/simulation.py:167-179
* AWGN per channel at SNR 5 dB — simulation.py:47-56, world.py:25, 93-98
* shared peak normalisation of mix and refs — simulation.py:197-202
* refs = mic-1 target and mic-1 total interference (world.py:236-238).
Geometry: D = 0.08 m (Final_pipeline/src/config.py:29), target 90 deg,
interferer 1 at 40 deg (world.py:33), further interferers uniform in [0, 180].
"""
from __future__ import annotations

import numpy as np
from scipy.signal import lfilter

FS = 16000
C_SOUND = 343.0
MIC_D = 0.08


def speech_like(rng: np.random.Generator, n: int, fs: int = FS) -> np.ndarray:
    x = rng.standard_normal(n)
    # AR(2) with poles 0.9, 0.5: y[n] = 1.4 y[n-1] - 0.45 y[n-2] + x[n]
    y = lfilter([1.0], [1.0, -1.4, 0.45], x)
    t = np.arange(n) / fs
    env = np.abs(np.sin(2 * np.pi * 4.0 * t + rng.uniform(0, np.pi)))
    blk = int(0.25 * fs)
    nb = -(-n // blk)
    keep = rng.random(nb) >= 0.25
    env *= np.repeat(keep, blk)[:n]
    return y * env


def far_field_delays(azimuth_deg: float, d: float = MIC_D, c: float = C_SOUND):
    th = np.deg2rad(azimuth_deg)
    return (d / 2) * np.cos(th - 0) / c, (d / 2) * np.cos(th - np.pi) / c


def frac_delay(y: np.ndarray, delay_s: float, fs: int = FS) -> np.ndarray:
    n = len(y)
    Yf = np.fft.rfft(y)
    f = np.fft.rfftfreq(n, 1.0 / fs)
    return np.fft.irfft(Yf * np.exp(-1j * 2 * np.pi * f * delay_s), n=n)


def add_awgn(rng: np.random.Generator, s: np.ndarray, snr_db: float) -> np.ndarray:
    p = np.mean(s ** 2)
    if p == 0:
        return s
    return s + rng.normal(0, np.sqrt(p / (10 ** (snr_db / 10))), s.shape)


def make_scene(idx: int, n_samples: int = 64000, n_interferers: int = 1, d: float = MIC_D,
               sir_db: float = 0.0, snr_db: float = 5.0, fs: int = FS):
    """One utterance. Returns (mix [2, S], target_ref [S], interference_ref [S]) float32."""
    rng = np.random.default_rng(1000 + idx)
    angles = [40.0] + list(rng.uniform(0.0, 180.0, max(0, n_interferers - 1)))
    tgt = speech_like(rng, n_samples, fs)
    t1, t2 = far_field_delays(90.0, d)
    tgt_m = [frac_delay(tgt, t1, fs), frac_delay(tgt, t2, fs)]
    int_m = [np.zeros(n_samples), np.zeros(n_samples)]
    for a in angles[:n_interferers]:
        s = speech_like(rng, n_samples, fs)
        d1, d2 = far_field_delays(a, d)
        int_m[0] += frac_delay(s, d1, fs)
        int_m[1] += frac_delay(s, d2, fs)
    p_t, p_i = np.mean(tgt_m[0] ** 2), np.mean(int_m[0] ** 2)
    if n_interferers > 0 and p_i > 0:
        g = np.sqrt(p_t / (p_i * 10 ** (sir_db / 10)))
        int_m = [g * int_m[0], g * int_m[1]]
    mix = np.stack([add_awgn(rng, tgt_m[0] + int_m[0], snr_db),
                    add_awgn(rng, tgt_m[1] + int_m[1], snr_db)])
    peak = np.max(np.abs(mix)) + 1e-9
    return ((mix / peak).astype(np.float32), (tgt_m[0] / peak).astype(np.float32),
            (int_m[0] / peak).astype(np.float32))


def write_world_scene(out_dir: str, mix: np.ndarray, tgt: np.ndarray, itf: np.ndarray,
                      fs: int = FS) -> str:
    """rt_av_zoom/core/world.py:236-263 on-disk format (what oracle_debug.py:35-39 and
    masked_mvdr.py read): stereo ``mixture.wav`` [S, 2] and the mic-1 references as mono
    ``target_reference.wav`` / ``interference_reference.wav``, each reference peak-normalised
    on its own (world.py:243-244). 16-bit PCM like soundfile's WAV default."""
    import os

    from . import wavio
    os.makedirs(out_dir, exist_ok=True)
    wavio.write(os.path.join(out_dir, "mixture.wav"), np.asarray(mix).T, fs)
    for name, r in (("target_reference.wav", tgt), ("interference_reference.wav", itf)):
        r = np.asarray(r, np.float64)
        wavio.write(os.path.join(out_dir, name), r / (np.max(np.abs(r)) + 1e-9), fs)
    return out_dir


def write_final_pipeline_scene(save_dir: str, mix: np.ndarray, tgt: np.ndarray,
                               itf: np.ndarray, tgt2: np.ndarray | None = None,
                               itf2: np.ndarray | None = None, fs: int = FS) -> str:
    """Final_pipeline/src/simulation.py:191-211 format (what run.py inf / eval read):
    stereo ``mixture.wav``, ``target.wav`` and ``interference.wav``, all divided by the
    mixture's peak (the arrays here are already on that shared scale, make_scene).
    ``tgt2``/``itf2`` are the mic-2 images (default: the mic-1 ones). Returns mixture.wav."""
    import os

    from . import wavio
    os.makedirs(save_dir, exist_ok=True)
    tgt2 = tgt if tgt2 is None else tgt2
    itf2 = itf if itf2 is None else itf2
    wavio.write(os.path.join(save_dir, "mixture.wav"), np.asarray(mix).T, fs)
    wavio.write(os.path.join(save_dir, "target.wav"), np.stack([tgt, tgt2], axis=1), fs)
    wavio.write(os.path.join(save_dir, "interference.wav"), np.stack([itf, itf2], axis=1), fs)
    return os.path.join(save_dir, "mixture.wav")


def mix_and_save(sources, prefix: str, angles=(90.0, 40.0, 130.0), d: float = 0.04,
                 fs: int = FS, out_dir: str = "."):
    """full_audio_generating_pipeline/world_building.py:68-100 for given mono sources
    (target first): far-field fractional delays per mic, mic-1 target / interference
    references, shared peak normalisation; writes mixture_<prefix>.wav (stereo),
    target_ref_<prefix>.wav, interf_ref_<prefix>.wav. Returns (mix [2, S], tgt, itf)."""
    import os

    from . import wavio
    n = max(len(s) for s in sources)
    # sources keep their dtype: the reference loads float32 (world_building.py:62), so its
    # forward rfft runs in single precision (numpy >= 2)
    raws = [np.pad(np.asarray(s), (0, n - len(s))) for s in sources]
    m1, m2, tgt_ref, int_ref = (np.zeros(n) for _ in range(4))
    for i, (r, a) in enumerate(zip(raws, angles)):
        t1, t2 = far_field_delays(a, d)
        s1 = frac_delay(r, t1, fs)
        m1 += s1
        m2 += frac_delay(r, t2, fs)
        if i == 0:
            tgt_ref += s1
        else:
            int_ref += s1
    mix = np.stack([m1, m2])
    norm = np.max(np.abs(mix)) + 1e-9
    wavio.write(os.path.join(out_dir, f"mixture_{prefix}.wav"), (mix / norm).T, fs)
    wavio.write(os.path.join(out_dir, f"target_ref_{prefix}.wav"), tgt_ref / norm, fs)
    wavio.write(os.path.join(out_dir, f"interf_ref_{prefix}.wav"), int_ref / norm, fs)
    return mix / norm, tgt_ref / norm, int_ref / norm


def scene_draws(idx: int, n_samples: int = 64000, n_interferers: int = 1, fs: int = FS):
    """The random draws of make_scene(idx) in its RNG order: angles [1 + K] (target 90
    deg first), sources [1 + K, S] and the unit-normal AWGN draws [2, S] (rng.normal(0, s)
    is s * standard_normal in numpy's Generator, so the device scales these)."""
    rng = np.random.default_rng(1000 + idx)
    angles = [40.0] + list(rng.uniform(0.0, 180.0, max(0, n_interferers - 1)))
    srcs = [speech_like(rng, n_samples, fs)]
    for _ in angles[:n_interferers]:
        srcs.append(speech_like(rng, n_samples, fs))
    z = np.stack([rng.standard_normal(n_samples), rng.standard_normal(n_samples)])
    return np.array([90.0] + angles[:n_interferers]), np.stack(srcs), z


# ---------------------------------------------------------------- counter-based draws
# The device generator (avz_scene_generate, csrc/avz_scene.hip) draws from Philox4x32-10
# streams keyed by (utterance index, SCENE_KEY ^ seed); this is its host restatement.
SCENE_KEY = 0x5CE7E5ED
STREAM_NOISE, STREAM_UNIF = 0x100, 0x200
UNIF_PHASE, UNIF_KEEP = 0x1000, 0x100000
UNIF_POS = 0x2000  # + 2 (source - 2) + {0, 1}: room position x, y of interferers 2..
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, k0: int, k1: int):
    """Random123 philox4x32-10 on uint32 counter arrays; returns four uint64 arrays < 2^32."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & _M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def _u53(hi, lo):
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def _key(idx: int, seed: int = 0):
    return idx & 0xFFFFFFFF, ((idx >> 32) ^ SCENE_KEY ^ seed) & 0xFFFFFFFF


def philox_normals(key, stream: int, n: int) -> np.ndarray:
    """n standard normals of a stream: pair i = Box-Muller of block i's two 53-bit uniforms."""
    i = np.arange((n + 1) // 2, dtype=np.uint64)
    x, y, z, w = philox4x32(i, stream, 0, 0, *key)
    u1 = (((x << np.uint64(32)) | y) >> np.uint64(11)).astype(np.float64)
    u1 = (u1 + 1.0) * 2.0 ** -53
    u2 = _u53(z, w)
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.empty(2 * len(i))
    out[0::2] = r * np.cos(2.0 * np.pi * u2)
    out[1::2] = r * np.sin(2.0 * np.pi * u2)
    return out[:n]


def philox_uniform(key, j) -> np.ndarray:
    x, y, _, _ = philox4x32(np.asarray(j, np.uint64), STREAM_UNIF, 0, 0, *key)
    return _u53(x, y)


def speech_like_philox(key, s: int, n: int, fs: int = FS) -> np.ndarray:
    """speech_like() on the counter-based streams of source s."""
    y = lfilter([1.0], [1.0, -1.4, 0.45], philox_normals(key, s, n))
    phi = np.pi * philox_uniform(key, UNIF_PHASE + s)
    t = np.arange(n) / fs
    env = np.abs(np.sin(2 * np.pi * 4.0 * t + phi))
    blk = int(0.25 * fs)
    nb = -(-n // blk)
    keep = philox_uniform(key, UNIF_KEEP * (1 + s) + np.arange(nb)) >= 0.25
    env *= np.repeat(keep, blk)[:n]
    return y * env


def scene_draws_philox(idx: int, n_samples: int = 64000, n_interferers: int = 1,
                       fs: int = FS, seed: int = 0):
    """(angles [1 + K], sources [1 + K, S], unit-normal noise [2, S]) of utterance idx."""
    key = _key(idx, seed)
    K = n_interferers
    angles = [90.0] + ([40.0] if K >= 1 else [])
    if K > 1:
        angles += list(180.0 * philox_uniform(key, np.arange(K - 1)))
    srcs = np.stack([speech_like_philox(key, s, n_samples, fs) for s in range(1 + K)])
    z = np.stack([philox_normals(key, STREAM_NOISE + c, n_samples) for c in range(2)])
    return np.array(angles), srcs, z


def mix_draws(angles, srcs, z, d: float = MIC_D, sir_db: float = 0.0, snr_db: float = 5.0,
              fs: int = FS):
    """make_scene's mixing (delays, SIR gain on mic 1, AWGN, shared peak) of given draws."""
    n = srcs.shape[-1]
    K = len(angles) - 1
    t1, t2 = far_field_delays(angles[0], d)
    tgt_m = [frac_delay(srcs[0], t1, fs), frac_delay(srcs[0], t2, fs)]
    int_m = [np.zeros(n), np.zeros(n)]
    for k in range(1, K + 1):
        d1, d2 = far_field_delays(angles[k], d)
        int_m[0] += frac_delay(srcs[k], d1, fs)
        int_m[1] += frac_delay(srcs[k], d2, fs)
    return _mix_images(tgt_m, int_m, K, z, sir_db, snr_db)


def _mix_images(tgt_m, int_m, K, z, sir_db, snr_db):
    """SIR gain on mic 1, AWGN per channel and the shared peak on per-mic target and summed
    interference images (simulation.py:167-202)."""
    p_t, p_i = np.mean(tgt_m[0] ** 2), np.mean(int_m[0] ** 2)
    if K > 0 and p_i > 0:
        g = np.sqrt(p_t / (p_i * 10 ** (sir_db / 10)))
        int_m = [g * int_m[0], g * int_m[1]]
    mix = []
    for c in range(2):
        cl = tgt_m[c] + int_m[c]
        p = np.mean(cl ** 2)
        mix.append(cl if p == 0 else cl + np.sqrt(p / (10 ** (snr_db / 10))) * z[c])
    mix = np.stack(mix)
    peak = np.max(np.abs(mix)) + 1e-9
    return ((mix / peak).astype(np.float32), (tgt_m[0] / peak).astype(np.float32),
            (int_m[0] / peak).astype(np.float32))


def make_scene_philox(idx: int, n_samples: int = 64000, n_interferers: int = 1,
                      d: float = MIC_D, sir_db: float = 0.0, snr_db: float = 5.0,
                      fs: int = FS, seed: int = 0):
    """Host restatement of avz_scene_generate for one utterance (make_scene's model on the
    counter-based draws)."""
    a, s, z = scene_draws_philox(idx, n_samples, n_interferers, fs, seed)
    return mix_draws(a, s, z, d, sir_db, snr_db, fs)


def make_batch_philox(batch: int, start: int = 0, n_samples: int = 64000,
                      n_interferers: int = 2, seed: int = 0, **kw):
    mix = np.empty((batch, 2, n_samples), np.float32)
    tgt = np.empty((batch, n_samples), np.float32)
    itf = np.empty((batch, n_samples), np.float32)
    for b in range(batch):
        mix[b], tgt[b], itf[b] = make_scene_philox(start + b, n_samples, n_interferers,
                                                   seed=seed, **kw)
    return mix, tgt, itf


def make_batch_device(batch: int, start: int = 0, n_samples: int = 64000,
                      n_interferers: int = 2, d: float = MIC_D, sir_db: float = 0.0,
                      snr_db: float = 5.0, fs: int = FS, device=None, rng: str = "host",
                      seed: int = 0):
    """A batch of scenes as device tensors (mix [B, 2, S], tgt [B, S], itf [B, S]).

    rng="host":   make_batch's scenes — the host draws the sources and noise (same RNG
                  stream as make_scene) and avz_scene_mix does the delays, SIR gain, AWGN
                  and peak normalisation.
    rng="philox": avz_scene_generate — draws and all on the device (make_batch_philox is
                  the host restatement); no host work, so a large shard costs milliseconds.
    """
    import torch

    from ._args import call, ptr as p
    from ._lib import lib
    dev = device or torch.device("cuda", torch.cuda.current_device())
    K = n_interferers
    mix = torch.empty((batch, 2, n_samples), dtype=torch.float32, device=dev)
    tgt = torch.empty((batch, n_samples), dtype=torch.float32, device=dev)
    itf = torch.empty((batch, n_samples), dtype=torch.float32, device=dev)
    if rng == "philox":
        ws_bytes = lib.avz_scene_generate_workspace_bytes(batch, K, n_samples)
        ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=dev)
        call("avz_scene_generate", batch, start, K, n_samples, seed, d, C_SOUND, float(fs),
             sir_db, snr_db, p(mix), mix.stride(0), mix.stride(1), p(tgt), p(itf), tgt.stride(0),
             p(ws), ws_bytes)
        return mix, tgt, itf
    if rng != "host":
        raise ValueError(f"rng must be 'host' or 'philox', not {rng!r}")
    angles = np.empty((batch, 1 + K))
    srcs = np.empty((batch, 1 + K, n_samples), np.float32)
    noise = np.empty((batch, 2, n_samples), np.float32)
    for b in range(batch):
        angles[b], srcs[b], noise[b] = scene_draws(start + b, n_samples, K, fs)
    d_ang = torch.from_numpy(angles).to(dev)
    d_src = torch.from_numpy(srcs).to(dev)
    d_noise = torch.from_numpy(noise).to(dev)
    ws_bytes = lib.avz_scene_workspace_bytes(batch, 1 + K, n_samples)
    ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=dev)
    call("avz_scene_mix", batch, 1 + K, n_samples, p(d_src), p(d_ang), p(d_noise), d, C_SOUND,
         float(fs), sir_db, snr_db, p(mix), mix.stride(0), mix.stride(1), p(tgt), p(itf),
         tgt.stride(0), p(ws), ws_bytes)
    return mix, tgt, itf


def make_batch(batch: int, start: int = 0, n_samples: int = 64000, n_interferers: int = 2,
               **kw):
    """[B, 2, S] mix, [B, S] target ref, [B, S] interference ref (float32)."""
    mix = np.empty((batch, 2, n_samples), np.float32)
    tgt = np.empty((batch, n_samples), np.float32)
    itf = np.empty((batch, n_samples), np.float32)
    for b in range(batch):
        mix[b], tgt[b], itf[b] = make_scene(start + b, n_samples, n_interferers, **kw)
    return mix, tgt, itf


# ---------------------------------------------------------------- reverberant shoebox rooms
# The `reverb` mode of the reference's scene builders (Final_pipeline/src/simulation.py:105-
# 165, rt_av_zoom/core/world.py:125-190) builds a pyroomacoustics ShoeBox; pyroomacoustics is
# not installed where this project is built or tested, so the contract is the classic
# image-source model (Allen & Berkley 1979) as stated here, and avz_room_rir /
# avz_scene_reverb_mix / avz_scene_reverb_generate (csrc/avz_scene.hip) compute this
# arithmetic. Not modelled: air absorption, scattering or ray tracing, any RIR high-pass
# filter, per-wall materials.
ROOM_DIM = [4.9, 4.9, 4.9]                          # world.py:22
RT60_TARGET = 0.5                                   # world.py:23
MIC_LOCS = [[2.41, 2.45, 1.5], [2.49, 2.45, 1.5]]   # world.py:28-31, one row per mic
SOURCE_TARGET_POS = [2.45, 3.45, 1.5]               # world.py:33 (90 degrees)
SOURCE_INTERF_POS = [3.22, 3.06, 1.5]               # world.py:34 (40 degrees)
RIR_HALF = 40                                       # taps floor(tau) - 40 .. floor(tau) + 40
RIR_MAX = 8192


def inverse_sabine(rt60: float, dim, c: float = C_SOUND) -> float:
    """Energy absorption of all six walls for a Sabine reverberation time rt60:
    24 ln 10 V / (c S rt60)."""
    lx, ly, lz = (float(v) for v in dim)
    V, S = lx * ly * lz, 2.0 * (lx * ly + ly * lz + lx * lz)
    return 24.0 * np.log(10.0) * V / (c * S * rt60)


class Room:
    """A shoebox room with two mics (avz_room). Defaults: the reference room."""

    def __init__(self, dim=None, absorption=None, max_order: int = 15, mic=None,
                 c: float = C_SOUND, fs: float = FS):
        self.dim = [float(v) for v in (ROOM_DIM if dim is None else dim)]
        self.absorption = float(inverse_sabine(RT60_TARGET, self.dim, c) if absorption is None
                                else absorption)
        self.max_order = int(max_order)
        self.mic = [[float(v) for v in m] for m in (MIC_LOCS if mic is None else mic)]
        self.c, self.fs = float(c), float(fs)

    @property
    def rir_len(self) -> int:
        return room_rir_len(self.dim, self.max_order, self.fs, self.c)


def room_images(order: int) -> np.ndarray:
    """The image triples q, |qx| + |qy| + |qz| <= order, as int [count, 3] in the order the
    RIR sums them: qx, then qy, then qz ascending. count = (2N + 1)(2N^2 + 2N + 3) / 3."""
    out = []
    for qx in range(-order, order + 1):
        rx = order - abs(qx)
        for qy in range(-rx, rx + 1):
            rz = rx - abs(qy)
            out.extend((qx, qy, qz) for qz in range(-rz, rz + 1))
    return np.array(out, dtype=np.int64).reshape(-1, 3)


def room_rir_len(dim, max_order: int, fs: float = FS, c: float = C_SOUND) -> int:
    """floor(fs / c * Dmax) + 42, Dmax = max over axes a of sqrt(((N + 1) L_a)^2 + sum of
    the other L_o^2): a bound on every image distance (the squared distance is convex in the
    per-axis image counts), plus the 40 taps after floor(tau) and one sample of slack."""
    dim = [float(v) for v in dim]
    dmax = 0.0
    for a in range(3):
        q = (max_order + 1) * dim[a]
        q *= q
        for o in range(3):
            if o != a:
                q += dim[o] * dim[o]
        dmax = max(dmax, np.sqrt(q))
    return int(np.floor(fs / c * dmax)) + 42


def frac_delay_taps(tau, amp=1.0, dtype=np.float64):
    """The 81 taps of one image: (n, amp * w(n - tau) * sinc(n - tau)) at n = floor(tau) - 40
    .. floor(tau) + 40, w(x) = 0.5 (1 + cos(2 pi x / 81)) for |x| <= 40.5, else 0: the window
    is centred on the continuous delay, so the taps are continuous in tau. With n = floor(tau)
    + k, sin(pi (n - tau)) = -(-1)^k sin(pi frac), frac = tau - floor(tau). tau, amp: arrays
    [M] -> n int64 [M, 81], values [M, 81]."""
    tau = np.atleast_1d(np.asarray(tau, dtype))
    amp = np.broadcast_to(np.asarray(amp, dtype), tau.shape)
    pi = 4 * np.arctan(dtype(1))
    fl = np.floor(tau)
    frac = tau - fl
    k = np.arange(-RIR_HALF, RIR_HALF + 1)
    x = k.astype(dtype)[None, :] - frac[:, None]
    n = fl.astype(np.int64)[:, None] + k[None, :]
    w = dtype(0.5) * (1 + np.cos(2 * pi * x / 81))
    w = np.where(np.abs(x) <= dtype(40.5), w, dtype(0))
    sgn = np.where(k % 2 == 0, -1.0, 1.0).astype(dtype)[None, :]
    # sin(pi frac) as sin(pi min(frac, 1 - frac)) (1 - frac is exact): accurate to the last
    # bits as frac -> 1, where rounding pi * frac would lose the tap's continuity
    sp = np.sin(pi * np.where(frac > 0.5, 1 - frac, frac))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        sinc = np.where(x == 0, dtype(1), sgn * sp / (pi * x))
    return n, amp[:, None] * w * sinc


def room_rir(dim, src, mic, absorption: float, max_order: int, fs: float = FS,
             c: float = C_SOUND, dtype=np.float64, rir_len: int | None = None) -> np.ndarray:
    """Image-source RIR from `src` to `mic` in the shoebox `dim` (all six walls with energy
    absorption `absorption`, beta = sqrt(1 - absorption)); every operation in `dtype`.
    Image q along axis i sits at q L + s (q even) or (q + 1) L - s (q odd); its amplitude is
    beta^order / (4 pi d) (the power by repeated multiplication, d clamped to >= 1e-3 m), its
    delay tau = d fs / c samples; frac_delay_taps spreads it. Taps outside [0, rir_len) are
    dropped; each sample sums its images in room_images order."""
    L = room_rir_len(dim, max_order, fs, c) if rir_len is None else rir_len
    dim, src, mic = (np.asarray(v, np.float64).astype(dtype) for v in (dim, src, mic))
    pi = 4 * np.arctan(dtype(1))
    q = room_images(max_order)
    odd = (q % 2) == 1
    img = np.where(odd, (q + 1).astype(dtype) * dim[None, :] - src[None, :],
                   q.astype(dtype) * dim[None, :] + src[None, :])
    dx, dy, dz = (img[:, a] - mic[a] for a in range(3))
    d = np.maximum(np.sqrt(dx * dx + dy * dy + dz * dz), dtype(1e-3))
    beta = np.sqrt(dtype(1) - dtype(absorption))
    bp = np.ones(max_order + 1, dtype)
    for o in range(1, max_order + 1):
        bp[o] = bp[o - 1] * beta
    amp = bp[np.abs(q).sum(axis=1)] / (4 * pi * d)
    tau = d * dtype(fs) / dtype(c)
    n, v = frac_delay_taps(tau, amp, dtype)
    h = np.zeros(L, dtype)
    ok = (n >= 0) & (n < L)
    np.add.at(h, n[ok], v[ok])  # unbuffered, in index order: image by image
    return h


def room_rirs(room: Room, positions, dtype=np.float64) -> np.ndarray:
    """[S, 2, rir_len]: the RIRs from positions [S, 3] to the room's two mics."""
    return np.stack([np.stack([room_rir(room.dim, p, m, room.absorption, room.max_order,
                                        room.fs, room.c, dtype) for m in room.mic])
                     for p in np.asarray(positions, np.float64).reshape(-1, 3)])


def reverb_mix_draws(positions, srcs, z, room: Room | None = None, sir_db: float = 0.0,
                     snr_db: float = 5.0):
    """mix_draws in a room: source s at positions[s] reaches mic c as fftconvolve(src,
    rir)[:n] (simulation.py:143-165); then the same SIR gain, AWGN and shared peak. Returns
    (mix [2, S], tgt, itf) float32; tgt / itf are the reverberant mic-1 images."""
    from scipy.signal import fftconvolve
    room = room or Room()
    srcs = np.asarray(srcs, np.float64)
    n = srcs.shape[-1]
    K = srcs.shape[0] - 1
    h = room_rirs(room, positions)
    tgt_m = [fftconvolve(srcs[0], h[0, c])[:n] for c in range(2)]
    int_m = [np.zeros(n), np.zeros(n)]
    for k in range(1, K + 1):
        for c in range(2):
            int_m[c] += fftconvolve(srcs[k], h[k, c])[:n]
    return _mix_images(tgt_m, int_m, K, z, sir_db, snr_db)


def room_positions_philox(key, n_interferers: int, room: Room, target_pos=None,
                          interferer_pos=None) -> np.ndarray:
    """[1 + K, 3]: the target, interferer 1, and interferers s >= 2 at (1 + u0 (dim_x - 2),
    1 + u1 (dim_y - 2), target z) with u = philox_uniform(key, UNIF_POS + 2 (s - 2) + {0, 1})
    (simulation.py:133-136 draws them in [1, dim - 1])."""
    t = SOURCE_TARGET_POS if target_pos is None else target_pos
    i = SOURCE_INTERF_POS if interferer_pos is None else interferer_pos
    pos = [list(map(float, t)), list(map(float, i))][:1 + n_interferers]
    for s in range(2, 1 + n_interferers):
        u = philox_uniform(key, UNIF_POS + 2 * (s - 2) + np.arange(2))
        pos.append([1.0 + u[0] * (room.dim[0] - 2.0), 1.0 + u[1] * (room.dim[1] - 2.0),
                    float(t[2])])
    return np.array(pos, np.float64).reshape(-1, 3)


def reverb_scene_draws_philox(idx: int, n_samples: int = 64000, n_interferers: int = 1,
                              room: Room | None = None, seed: int = 0, target_pos=None,
                              interferer_pos=None):
    """(positions [1 + K, 3], sources [1 + K, S], unit-normal noise [2, S]) of utterance idx:
    scene_draws_philox's sources and noise, positions in place of the azimuths."""
    room = room or Room()
    _, srcs, z = scene_draws_philox(idx, n_samples, n_interferers, room.fs, seed)
    pos = room_positions_philox(_key(idx, seed), n_interferers, room, target_pos, interferer_pos)
    return pos, srcs, z


def make_reverb_scene_philox(idx: int, n_samples: int = 64000, n_interferers: int = 1,
                             room: Room | None = None, sir_db: float = 0.0, snr_db: float = 5.0,
                             seed: int = 0, target_pos=None, interferer_pos=None):
    """Host restatement of avz_scene_reverb_generate for one utterance."""
    room = room or Room()
    pos, srcs, z = reverb_scene_draws_philox(idx, n_samples, n_interferers, room, seed,
                                             target_pos, interferer_pos)
    return reverb_mix_draws(pos, srcs, z, room, sir_db, snr_db)


def make_reverb_batch_philox(batch: int, start: int = 0, n_samples: int = 64000,
                             n_interferers: int = 2, seed: int = 0, **kw):
    mix = np.empty((batch, 2, n_samples), np.float32)
    tgt = np.empty((batch, n_samples), np.float32)
    itf = np.empty((batch, n_samples), np.float32)
    for b in range(batch):
        mix[b], tgt[b], itf[b] = make_reverb_scene_philox(start + b, n_samples, n_interferers,
                                                          seed=seed, **kw)
    return mix, tgt, itf


def reverb_scene_draws(idx: int, n_samples: int = 64000, n_interferers: int = 1,
                       room: Room | None = None, target_pos=None, interferer_pos=None):
    """scene_draws's sources and noise (the host RNG stream of make_scene(idx)); interferers
    2.. are placed in [1, dim - 1] on x and y by default_rng(2000 + idx), at the target's z."""
    room = room or Room()
    ang, srcs, z = scene_draws(idx, n_samples, n_interferers, int(room.fs))
    t = SOURCE_TARGET_POS if target_pos is None else target_pos
    i = SOURCE_INTERF_POS if interferer_pos is None else interferer_pos
    pos = [list(map(float, t)), list(map(float, i))][:1 + n_interferers]
    rng = np.random.default_rng(2000 + idx)
    for s in range(2, 1 + n_interferers):
        u = rng.random(2)
        pos.append([1.0 + u[0] * (room.dim[0] - 2.0), 1.0 + u[1] * (room.dim[1] - 2.0),
                    float(t[2])])
    return np.array(pos, np.float64).reshape(-1, 3), srcs, z


def _room_struct(room: Room):
    from ._lib import AvzRoom
    r = AvzRoom()
    for a in range(3):
        r.dim[a] = room.dim[a]
        r.mic[0][a], r.mic[1][a] = room.mic[0][a], room.mic[1][a]
    r.absorption, r.max_order, r.c_sound, r.fs = room.absorption, room.max_order, room.c, room.fs
    return r


REVERB_SLICE_BYTES = 1 << 30  # workspace per call of make_reverb_batch_device


def make_reverb_batch_device(batch: int, start: int = 0, n_samples: int = 64000,
                             n_interferers: int = 2, room: Room | None = None,
                             sir_db: float = 0.0, snr_db: float = 5.0, device=None,
                             rng: str = "host", seed: int = 0, target_pos=None,
                             interferer_pos=None):
    """make_batch_device in a room (mix [B, 2, S], tgt [B, S], itf [B, S] device tensors).

    rng="host":   the host draws the sources and noise (reverb_scene_draws) and
                  avz_scene_reverb_mix does the RIRs, the convolutions and the mixing
                  (reverb_mix_draws is the restatement).
    rng="philox": avz_scene_reverb_generate, everything on the device
                  (make_reverb_batch_philox is the restatement).
    The workspace is 32 (ceil(S / 2) + S) Lc bytes per utterance for S sources (13.3 MB at
    4 s, 4 sources, max_order 15), so the batch runs in slices of at most REVERB_SLICE_BYTES
    of workspace; the scenes do not depend on the slicing."""
    import ctypes as ct

    import torch

    from ._args import call, ptr as p
    from ._lib import check, lib
    room = room or Room()
    dev = device or torch.device("cuda", torch.cuda.current_device())
    K, n = n_interferers, n_samples
    if rng not in ("host", "philox"):
        raise ValueError(f"rng must be 'host' or 'philox', not {rng!r}")
    r = _room_struct(room)
    mix = torch.empty((batch, 2, n), dtype=torch.float32, device=dev)
    tgt = torch.empty((batch, n), dtype=torch.float32, device=dev)
    itf = torch.empty((batch, n), dtype=torch.float32, device=dev)
    if batch == 0:
        return mix, tgt, itf
    ws_fn = (lib.avz_scene_reverb_generate_workspace_bytes if rng == "philox"
             else lib.avz_scene_reverb_workspace_bytes)
    cnt = K if rng == "philox" else 1 + K
    check(lib.avz_room_rir_len(ct.byref(r)), "avz_room_rir_len")
    per = ws_fn(ct.byref(r), 1, cnt, n)
    step = max(1, min(batch, REVERB_SLICE_BYTES // max(per, 1)))
    ws_bytes = ws_fn(ct.byref(r), step, cnt, n)
    ws = torch.empty((max(ws_bytes, 4) + 3) // 4, dtype=torch.float32, device=dev)
    D3 = ct.c_double * 3
    tp = D3(*(SOURCE_TARGET_POS if target_pos is None else target_pos))
    ip = D3(*(SOURCE_INTERF_POS if interferer_pos is None else interferer_pos))
    for b0 in range(0, batch, step):
        nb = min(step, batch - b0)
        m, t, i = mix[b0:b0 + nb], tgt[b0:b0 + nb], itf[b0:b0 + nb]
        if rng == "philox":
            call("avz_scene_reverb_generate", ct.byref(r), nb, start + b0, K, n, seed, tp, ip,
                 sir_db, snr_db, p(m), mix.stride(0), mix.stride(1), p(t), p(i), tgt.stride(0),
                 p(ws), ws_bytes, device=dev)
            continue
        pos = np.empty((nb, 1 + K, 3))
        srcs = np.empty((nb, 1 + K, n), np.float32)
        noise = np.empty((nb, 2, n), np.float32)
        for b in range(nb):
            pos[b], srcs[b], noise[b] = reverb_scene_draws(start + b0 + b, n, K, room,
                                                           target_pos, interferer_pos)
        d_pos, d_src, d_noise = (torch.from_numpy(a).to(dev) for a in (pos, srcs, noise))
        call("avz_scene_reverb_mix", ct.byref(r), nb, 1 + K, n, p(d_src), p(d_pos), p(d_noise),
             sir_db, snr_db, p(m), mix.stride(0), mix.stride(1), p(t), p(i), tgt.stride(0),
             p(ws), ws_bytes, device=dev)
    return mix, tgt, itf
