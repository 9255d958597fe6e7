"""Seeded WPE cases with an fp64 and an extended-precision reference (plain module shared by
test_wpe_reference.py and test_gpu_wpe.py).

* ``wpe_f64``: the package's fp64 restatement of the algorithm (avz.dereverb.wpe_numpy).
* ``wpe_ld``: the same algorithm in ``np.clongdouble`` (80-bit here) with its own regressor,
  Cholesky and substitutions, written entry by entry. ``E_ref,k = max|wpe_f64 - wpe_ld|``
  of a bin is the fp64 reference's own error there: cond(R) reaches 1e11..1e12 on speech, so
  a flat tolerance cannot serve.

Families:
 (a) ``ar_item``: per bin a 2 x 2 MIMO autoregressive reverb, Y[t] = S[t] + sum over
     tau = delay .. delay + 3 of A_tau Y[t - tau], sum ||A_tau||_2 <= 0.8 (so rho < 1), S
     complex Gaussian with a speech-like time-varying variance; cast to complex64.
 (b) ``speech_item``: the scipy STFT (complex64) of tests/golden/inputs_test.npz samples
     40000:64000 at 512/256 or 1024/512, every 8th bin (DC and Nyquist are among them).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import scipy.signal

from avz.dereverb import EPS_FLOOR, pivot_threshold, wpe_numpy
from conftest import triple_f32

wpe_f64 = wpe_numpy

LD = np.longdouble
CLD = np.clongdouble
HAVE_LD = bool(np.finfo(LD).eps < 2e-19)

SEG = (40000, 64000)
AR_LAGS = 4


# ----------------------------------------------------------------------------
# extended-precision reference
# ----------------------------------------------------------------------------
def _wpe_ld_bin(Y, taps, delay, iterations):
    D, T = Y.shape
    n = taps * D
    Y = Y.astype(CLD)
    if T - delay < n:
        return Y, 2
    Yt = np.zeros((n, T), dtype=CLD)
    for t in range(T):
        for tau in range(taps):
            s = t - delay - tau
            if s >= 0:
                for m in range(D):
                    Yt[tau * D + m, t] = Y[m, s]
    thr = LD(pivot_threshold(taps))
    X = Y.copy()
    for _ in range(iterations):
        p = (X.real ** 2 + X.imag ** 2).sum(axis=0) / LD(D)
        pm = p.max()
        if pm == 0:
            return Y, 1
        lam = LD(1) / np.maximum(p, LD(EPS_FLOOR) * pm)
        R = (Yt * lam) @ Yt.conj().T
        P = (Yt * lam) @ Y.conj().T
        L = np.zeros((n, n), dtype=CLD)
        for j in range(n):          # Cholesky-Banachiewicz, row by row
            for c in range(j + 1):
                s = R[j, c]
                for q in range(c):
                    s = s - L[j, q] * np.conj(L[c, q])
                if c == j:
                    d = s.real
                    if not (d > thr * R[j, j].real) or not np.isfinite(d):
                        return Y, 2
                    L[j, j] = np.sqrt(d)
                else:
                    L[j, c] = s / L[c, c].real
        Z = np.zeros((n, D), dtype=CLD)
        for i in range(n):
            Z[i] = (P[i] - L[i, :i] @ Z[:i]) / L[i, i].real
        G = np.zeros((n, D), dtype=CLD)
        for i in range(n - 1, -1, -1):
            G[i] = (Z[i] - L[i + 1:, i].conj() @ G[i + 1:]) / L[i, i].real
        X = Y - G.conj().T @ Yt
    return X, 0


def wpe_ld(Y, taps=10, delay=3, iterations=3, frames=None):
    """Y [2, F, T] -> (X [2, F, T] clongdouble, status [F])."""
    _, F, T = Y.shape
    Tb = T if frames is None else max(0, min(int(frames), T))
    X = Y.astype(CLD)
    status = np.zeros(F, dtype=np.int32)
    for k in range(F):
        X[:, k, :Tb], status[k] = _wpe_ld_bin(Y[:, k, :Tb], taps, delay, iterations)
    return X, status


# ----------------------------------------------------------------------------
# families
# ----------------------------------------------------------------------------
def ar_item(seed: int, bins: int, T: int, delay: int):
    """-> (Y complex64 [2, bins, T], S complex128 [2, bins, T])."""
    rng = np.random.default_rng(seed)
    Y = np.zeros((2, bins, T), dtype=np.complex128)
    S = np.zeros((2, bins, T), dtype=np.complex128)
    t = np.arange(T)
    for k in range(bins):
        # speech-like variance: a slow syllable envelope with pauses, 40 dB of range
        env = np.abs(np.sin(2 * np.pi * t / rng.uniform(9, 23) + rng.uniform(0, 2 * np.pi))) ** 2
        env = env * (rng.random(T // 8 + 1).repeat(8)[:T] > 0.25) + 1e-4
        lvl = 10.0 ** rng.uniform(-2, 0)
        s = (rng.standard_normal((2, T)) + 1j * rng.standard_normal((2, T))) * np.sqrt(env) * lvl
        A = rng.standard_normal((AR_LAGS, 2, 2)) + 1j * rng.standard_normal((AR_LAGS, 2, 2))
        A *= 0.8 / sum(np.linalg.norm(a, 2) for a in A)
        y = np.zeros((2, T), dtype=np.complex128)
        for i in range(T):
            y[:, i] = s[:, i]
            for q in range(AR_LAGS):
                j = i - delay - q
                if j >= 0:
                    y[:, i] += A[q] @ y[:, j]
        Y[:, k], S[:, k] = y, s
    return Y.astype(np.complex64), S


@functools.lru_cache(maxsize=None)
def speech_item(n_fft: int):
    """-> Y complex64 [2, bins, T]: every 8th bin of the excerpt's STFT."""
    mix, _, _ = triple_f32("test", SEG)
    _, _, Y = scipy.signal.stft(mix.astype(np.float64), 16000, nperseg=n_fft, noverlap=n_fft // 2)
    return np.ascontiguousarray(Y[:, ::8].astype(np.complex64))


@dataclass(frozen=True)
class Case:
    name: str
    family: str        # "ar" or "speech"
    T: int
    taps: int
    delay: int
    iterations: int
    batch: int
    bins: int
    frames: tuple      # valid frames per item
    n_fft: int = 0
    seed: int = 0
    lead: int = 0      # leading frames of digital silence (p = 0 there: the floor decides lambda)


def min_frames(taps: int, delay: int) -> int:
    """Shortest synthetic item: 1.5 frames of regressor per unknown (2 taps unknowns), so the
    fp64 reference stays far from the singular threshold."""
    return delay + 3 * taps


def _ar_cases():
    out, idx = [], 0
    for T in (24, 64, 65, 257):
        for taps, delay in ((1, 1), (2, 3), (10, 3), (16, 1)):
            if T < min_frames(taps, delay):
                continue
            for iterations in (1, 3):
                batch = 3 if idx % 2 else 1
                bins = 7 if (idx // 2) % 2 else 5
                lo = min_frames(taps, delay)
                frames = tuple(max(lo, T - d) for d in (0, 3, 7))[:batch]
                out.append(Case(f"ar-T{T}-K{taps}-d{delay}-i{iterations}-B{batch}-F{bins}", "ar", T,
                                taps, delay, iterations, batch, bins, frames, seed=1000 + idx))
                idx += 1
    return out


AR_CASES = _ar_cases() + [Case("ar-T65-K10-d3-i3-B1-F5-silence", "ar", 65, 10, 3, 3, 1, 5, (65,),
                                seed=2000, lead=5)]
SPEECH_CASES = [Case(f"speech-{n}", "speech", 0, 10, 3, 3, 1, n // 16 + 1, (), n_fft=n)
                for n in (512, 1024)]
GPU_CASES = AR_CASES + SPEECH_CASES
# the dereverberation property (taps >= 4 covers the family's four lags)
DENOISE_CASES = [(seed, T, taps, delay) for seed in (1, 2, 3)
                 for T, taps, delay in ((257, 4, 3), (257, 10, 3), (257, 16, 1), (65, 4, 1))]


@functools.lru_cache(maxsize=None)
def case_input(name: str):
    """-> (Y complex64 [B, 2, bins, T], frames tuple [B])."""
    c = next(c for c in GPU_CASES if c.name == name)
    if c.family == "speech":
        Y = speech_item(c.n_fft)[None]
        return Y, (Y.shape[3],)
    Y = np.stack([ar_item(c.seed * 10 + b, c.bins, c.T - c.lead, c.delay)[0]
                  for b in range(c.batch)])
    if c.lead:      # digital silence, then the reverberant signal
        Y = np.concatenate([np.zeros_like(Y[..., :c.lead]), Y], axis=3)
    return Y, c.frames


@functools.lru_cache(maxsize=None)
def case_reference(name: str):
    """-> dict: X (wpe_f64, complex128 [B, 2, bins, T]), status, rel (smallest relative pivot),
    E_ref [B, bins] = max|wpe_f64 - wpe_ld| per bin, ymax [B, bins] = max|Y_k|."""
    c = next(c for c in GPU_CASES if c.name == name)
    Y, frames = case_input(name)
    B, _, F, T = Y.shape
    X = np.zeros(Y.shape, dtype=np.complex128)
    status = np.zeros((B, F), dtype=np.int32)
    rel = np.zeros((B, F))
    E = np.zeros((B, F))
    for b in range(B):
        X[b], status[b], rel[b] = wpe_f64(Y[b], c.taps, c.delay, c.iterations, frames=frames[b],
                                          return_info=True)
        Xl, st = wpe_ld(Y[b], c.taps, c.delay, c.iterations, frames=frames[b])
        assert np.array_equal(st, status[b]), (name, b)
        E[b] = np.abs(X[b] - Xl).max(axis=(0, 2)).astype(np.float64)
    ymax = np.abs(Y).max(axis=(1, 3)).astype(np.float64)
    return {"X": X, "status": status, "rel": rel, "E_ref": E, "ymax": ymax}
