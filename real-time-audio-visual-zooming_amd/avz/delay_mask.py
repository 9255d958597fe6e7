"""Blind delay-histogram mask: the delay-only form of DUET (Yilmaz & Rickard 2004).

``delay_mask_numpy`` is the fp64 restatement of ``avz_delay_mask`` (include/avz.h; DESIGN.md
section 17) in its three stages, each a function of its own that takes the spectra, so that a
test can feed perturbed ones. ``enhance_blind`` is the blind counterpart of
``masked_mvdr.enhance``: the device mask, then an external-mask MVDR plan with the floor
post-filter (full_audio_generating_pipeline/inference.py:88-118 without its mask model).

``delay_mask_stream_numpy`` / ``NumpyDelayStream`` restate the streaming form
``avz_delay_stream_push`` with the same stage functions, one frame at a
time: h_t = forget h_t-1 + d_t where the adapt flag is set, the peaks of h_t, frame t's labels.

Steering convention (masked_mvdr.py:22-35, mic 0 at +d/2): a far-field source at azimuth theta
gives Y1 / Y0 = exp(+i omega_k delta) with delta = delta_max cos(theta), delta_max = d fs / c.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

DEFAULTS = dict(hist_bins=65, smooth=3, rel_height=0.25, min_sep=0.2, max_peaks=3, f_lo=100.0)
LIST = 8  # delta_t + at most 7 kept delays


@dataclass
class DelayGrid:
    """The histogram's geometry for one plan."""
    n_fft: int
    nb: int
    dmax: float     # delta_max, samples
    R: float        # half-range 1.25 delta_max
    bin_w: float    # 2 R / nb
    k_lo: int
    k_hi: int       # k_hi < k_lo: an empty band

    def centre(self, i):
        return -self.R + (np.asarray(i, np.float64) + 0.5) * self.bin_w


def delay_grid(n_fft: int, fs=16000, mic_d=0.08, c_sound=343.0, hist_bins=65,
               f_lo=100.0) -> DelayGrid:
    dmax = mic_d * float(fs) / c_sound
    R = 1.25 * dmax
    lo = np.ceil(f_lo * n_fft / float(fs))
    k_lo = n_fft if lo >= n_fft else max(1, int(lo))
    k_hi = -1
    if R > 0 and np.isfinite(R):
        k_hi = int(min(n_fft // 2, np.ceil(n_fft / (2.0 * R)) - 1.0))
    return DelayGrid(n_fft, int(hist_bins), dmax, R, 2.0 * R / hist_bins, k_lo, k_hi)


def delay_histogram(Y0: np.ndarray, Y1: np.ndarray, g: DelayGrid) -> np.ndarray:
    """Stage 1: h [nb] float64 of the spectra Y0, Y1 [F, T] (two-bin deposits of w = |X| at
    delta = arg(X) / omega_k, X = Y1 conj(Y0), over the band's bins and every frame)."""
    h = np.zeros(g.nb)
    if g.k_hi < g.k_lo:
        return h
    k = np.arange(g.k_lo, g.k_hi + 1)
    X = Y1[k].astype(np.complex128) * np.conj(Y0[k].astype(np.complex128))
    w = np.abs(X)
    delta = np.angle(X) / (2.0 * np.pi * k / g.n_fft)[:, None]
    u = (delta + g.R) / g.bin_w - 0.5
    ok = np.isfinite(u) & np.isfinite(w)
    u, w = u[ok], w[ok]
    i0 = np.floor(u)
    phi = u - i0
    i0 = i0.astype(np.int64)
    for idx, wt in ((i0, (1.0 - phi) * w), (i0 + 1, phi * w)):
        m = (idx >= 0) & (idx < g.nb)
        h += np.bincount(idx[m], weights=wt[m], minlength=g.nb)
    return h


def smooth_histogram(h: np.ndarray, smooth: int) -> np.ndarray:
    hs = np.asarray(h, np.float64).copy()
    for _ in range(int(smooth)):
        p = np.concatenate(([0.0], hs, [0.0]))
        hs = 0.25 * p[:-2] + 0.5 * p[1:-1] + 0.25 * p[2:]
    return hs


def delay_peaks(h: np.ndarray, g: DelayGrid, angle=90.0, smooth=3, rel_height=0.25,
                min_sep=0.2, max_peaks=3):
    """Stage 2: (delays [8] float64: delta_t, the J kept delays highest first, NaN; J; the kept
    peaks' bins)."""
    hs = smooth_histogram(h, smooth)
    d_t = g.dmax * np.cos(np.deg2rad(angle))
    out = np.full(LIST, np.nan)
    out[0] = d_t
    top = np.max(hs)
    if not top > 0:
        return out, 0, []
    p = np.concatenate(([0.0], hs, [0.0]))
    l, m, r = p[:-2], p[1:-1], p[2:]
    cand = (m > l) & (m >= r) & (m >= rel_height * top)
    den = l - 2.0 * m + r
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where(den == 0.0, 0.0, 0.5 * (l - r) / den)
    d = -g.R + (np.arange(g.nb) + 0.5 + o) * g.bin_w
    cand &= ~(np.abs(d - d_t) <= min_sep * g.dmax)
    idx = np.nonzero(cand)[0]
    idx = idx[np.argsort(-m[idx], kind="stable")][:int(max_peaks)]  # ties: the lower bin
    out[1:1 + len(idx)] = d[idx]
    return out, len(idx), [int(i) for i in idx]


def delay_labels(Y0: np.ndarray, Y1: np.ndarray, delays: np.ndarray, J: int,
                 n_fft: int) -> np.ndarray:
    """Stage 3: M [F, T] float32: 0 where some kept delay's cost |Y1 - e^{i omega_k delta_j}
    Y0|^2 is strictly below the target's, else 1."""
    F = Y0.shape[0]
    y0, y1 = Y0.astype(np.complex128), Y1.astype(np.complex128)
    k = np.arange(F, dtype=np.float64)[:, None]

    def cost(dj):
        ph = 2.0 * np.pi * k * dj / n_fft
        return np.abs(y1 - (np.cos(ph) + 1j * np.sin(ph)) * y0) ** 2

    with np.errstate(invalid="ignore", over="ignore"):
        c0 = cost(delays[0])
        other = np.zeros(Y0.shape, bool)
        for j in range(1, 1 + int(J)):
            other |= cost(delays[j]) < c0
    return np.where(other, 0.0, 1.0).astype(np.float32)


def delay_mask_numpy(Y0: np.ndarray, Y1: np.ndarray, n_fft: int, fs=16000, mic_d=0.08,
                     c_sound=343.0, angle=90.0, hist_bins=65, smooth=3, rel_height=0.25,
                     min_sep=0.2, max_peaks=3, f_lo=100.0):
    """The three stages on one utterance's spectra Y0, Y1 [F, T] (complex64 of the library's
    STFT): (M [F, T] float32, h [hist_bins], delays [8], J)."""
    g = delay_grid(n_fft, fs, mic_d, c_sound, hist_bins, f_lo)
    h = delay_histogram(Y0, Y1, g)
    delays, J, _ = delay_peaks(h, g, angle, smooth, rel_height, min_sep, max_peaks)
    return delay_labels(Y0, Y1, delays, J, n_fft), h, delays, J


class NumpyDelayStream:
    """One stream of the streaming delay mask in fp64, stateful: push() any number of hops at a
    time (mix [2, hops H]; the frames are avz_stream_push's: [x_t-1 | x_t] under the fp32
    periodic Hann scaled by 1 / sum(w)) or push_spectra() frames given as spectra [F, hops].
    Every frame is computed on its own, so the results do not depend on the grouping. Both
    return (M [F, hops] float32, h [hops, nb], lists [hops, 8], J [hops])."""

    def __init__(self, n_fft, fs=16000, mic_d=0.08, c_sound=343.0, angle=90.0, hist_bins=65,
                 smooth=3, rel_height=0.25, min_sep=0.2, max_peaks=3, f_lo=100.0, forget=1.0):
        if not 0.0 < forget <= 1.0:
            raise ValueError("forget must lie in (0, 1]")
        self.n_fft, self.H, self.forget, self.angle = n_fft, n_fft // 2, float(forget), angle
        self.grid = delay_grid(n_fft, fs, mic_d, c_sound, hist_bins, f_lo)
        self.peak_kw = dict(smooth=smooth, rel_height=rel_height, min_sep=min_sep,
                            max_peaks=max_peaks)
        w = 0.5 + 0.5 * np.cos(np.linspace(-np.pi, np.pi, n_fft + 1)[:-1])
        self.win32 = w.astype(np.float32).astype(np.float64)
        self.reset()

    def reset(self):
        self.count = 0
        self.prev = np.zeros((2, self.H))
        self.h = np.zeros(self.grid.nb)

    def steer(self, angle):
        """New target azimuth (degrees) from the next pushed frame."""
        self.angle = angle

    def push_spectra(self, Y0, Y1, adapt=True):
        T = Y0.shape[1]
        flags = np.broadcast_to(np.asarray(adapt, bool), (T,))
        M = np.empty((Y0.shape[0], T), np.float32)
        hs, lists, Js = np.empty((T, self.grid.nb)), np.empty((T, LIST)), np.empty(T, np.int64)
        for t in range(T):
            y0, y1 = Y0[:, t:t + 1], Y1[:, t:t + 1]
            if flags[t]:
                self.h = self.forget * self.h + delay_histogram(y0, y1, self.grid)
            delays, J, _ = delay_peaks(self.h, self.grid, self.angle, **self.peak_kw)
            M[:, t] = delay_labels(y0, y1, delays, J, self.n_fft)[:, 0]
            hs[t], lists[t], Js[t] = self.h, delays, J
            self.count += 1
        return M, hs, lists, Js

    def push(self, mix, adapt=True):
        mix = np.asarray(mix, dtype=np.float64)
        H = self.H
        hops = mix.shape[-1] // H
        assert mix.shape == (2, hops * H) and hops >= 1
        x = np.concatenate([self.prev, mix], axis=1)
        Y = np.stack([[np.fft.rfft(x[m, j * H:j * H + 2 * H] * self.win32) / self.win32.sum()
                       for j in range(hops)] for m in range(2)]).transpose(0, 2, 1)
        self.prev = mix[:, -H:].copy()
        return self.push_spectra(Y[0].astype(np.complex64), Y[1].astype(np.complex64), adapt)


def delay_mask_stream_numpy(Y0: np.ndarray, Y1: np.ndarray, n_fft: int, fs=16000, mic_d=0.08,
                            c_sound=343.0, hist_bins=65, smooth=3, rel_height=0.25, min_sep=0.2,
                            max_peaks=3, f_lo=100.0, forget=1.0, adapt=None, angle=90.0):
    """The streaming mask on one stream's frames Y0, Y1 [F, T] (complex64), one frame at a
    time: (M [F, T] float32, h per frame [T, hist_bins], lists [T, 8], J [T]). adapt: per-frame
    flags [T] (default all set): 0 freezes the histogram while the labels continue."""
    st = NumpyDelayStream(n_fft, fs, mic_d, c_sound, angle, hist_bins, smooth, rel_height,
                          min_sep, max_peaks, f_lo, forget)
    return st.push_spectra(Y0, Y1, True if adapt is None else np.asarray(adapt, bool))


def enhance_blind(y_mix: np.ndarray, n_fft=1024, mic_d=0.08, sigma=1e-5, angle=90.0,
                  fs=16000, c_sound=343.0, pf_floor=0.05, device="cuda", **mask_kw) -> np.ndarray:
    """y_mix [2, S] float32 -> beamformed waveform (float32 numpy, not normalised): the device
    delay mask, then MVDRPlan(mask="external", postfilter="floor"). No reference, no model.
    ``mask_kw``: engine.delay_mask's options (hist_bins, smooth, rel_height, min_sep,
    max_peaks, f_lo)."""
    import torch

    from . import engine

    S = y_mix.shape[1]
    plan = engine.MVDRPlan(n_fft=n_fft, fs=fs, sigma=sigma, mic_d=mic_d, c_sound=c_sound,
                           angle_deg=angle, mask="external", postfilter="floor",
                           pf_floor=pf_floor, normalize="none", max_batch=1, max_samples=S)
    mix = torch.from_numpy(np.ascontiguousarray(y_mix, dtype=np.float32))[None].to(device)
    mask = engine.delay_mask(plan, mix, **mask_kw)
    out, _ = plan.run(mix, ext_mask=mask)
    return out[0, :plan.out_len(S)].cpu().numpy()
