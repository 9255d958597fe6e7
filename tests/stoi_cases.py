"""Seeded STOI cases with the fp64 restatement and an independent extended-precision
statement (plain module shared by test_stoi_reference.py and test_gpu_stoi.py).

* ``stoi_f64``: the package's restatement (avz.stoi.stoi_numpy: resample_poly, np.fft,
  vectorised segments).
* ``stoi_ld``: the algorithm written again in ``np.longdouble`` (80-bit here) with none of
  those: the direct polyphase sum, a direct DFT at bins 7..218 only, explicit loops over the
  segments and bands. ``E_ref = |d_f64 - d_ld|`` is the restatement's own error on a case.
* ``e_pert``: the largest change of the restatement's d over 8 seeded perturbations of its
  frame spectra by ``PERTURBATION * max|X|`` per bin, the bound test_stft_stage holds the
  engine's fp32 transforms to.

The GPU test's tolerance on d is ``1e-6 + 4 E_ref + 4 E_pert``; every GPU case must keep its
keep-decision margin min_j |e_j - (max e - 40)| at or above MARGIN_DB, since the fp32 storage
of the 10-kHz signal moves an energy by about 4e-7 dB.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from avz import stoi as S
from conftest import golden

LD = np.longdouble
HAVE_LD = bool(np.finfo(LD).eps < 2e-19)
PERTURBATION = 2e-6
MARGIN_DB = 1e-3
BAND_TABLE = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43),
              (43, 55), (55, 69), (69, 87), (87, 109), (109, 138), (138, 174), (174, 219)]
PINNED = {"self": 1.0, "mix0": 0.6003809, "est16": 0.9427483}   # the full test triple
EXCERPTS = (16000, 40000)                                       # 1-s excerpts of it
TILE = 32                                                       # the band stage's frames per block


# ----------------------------------------------------------------------------
# the independent statement
# ----------------------------------------------------------------------------
def _window_ld():
    n = np.arange(1, S.N_FRAME + 1, dtype=LD)
    return (LD(1) - np.cos(LD(2) * np.arccos(LD(-1)) * n / LD(S.N_FRAME + 1))) / LD(2)


def resample_ld(s, fs):
    """s10[m] = sum_i s[i] h'[8 m - 5 i + 290], h' = 5 h / sum h, m < ceil(5 len / 8)."""
    s = np.asarray(s, dtype=LD)
    if int(fs) == S.FS_INTERNAL:
        return s
    h = S.resample_taps().astype(LD)
    hp = LD(5) * h / h.sum()
    n, half = len(s), S.RES_HALF
    n10 = -(-5 * n // 8)
    out = np.zeros(n10, dtype=LD)
    for m in range(n10):
        c = 8 * m + half
        lo = max(0, -(-(c - 2 * half) // 5))
        hi = min(n - 1, c // 5)
        if hi >= lo:
            i = np.arange(lo, hi + 1)
            out[m] = np.dot(s[i], hp[c - 5 * i])
    return out


@functools.lru_cache(maxsize=None)
def _dft_matrix():
    pi = np.arccos(LD(-1))
    k = np.arange(BAND_TABLE[0][0], BAND_TABLE[-1][1], dtype=LD)[:, None]
    n = np.arange(S.N_FRAME, dtype=LD)[None, :]
    a = LD(2) * pi * k * n / LD(S.NFFT)
    return np.cos(a), -np.sin(a)


def stoi_ld(x, y, fs):
    """-> dict(d, status, frames, kept, x10, energies): the algorithm in long double."""
    w = _window_ld()
    eps = LD(S.EPS)
    x10, y10 = resample_ld(x, fs), resample_ld(y, fs)
    n10 = len(x10)
    starts = []
    i = 0
    while i < n10 - S.N_FRAME:
        starts.append(i)
        i += S.HOP
    out = dict(x10=x10, y10=y10, frames=len(starts))
    if not starts:
        out.update(d=1e-5, status=1, kept=0, energies=np.zeros(0, dtype=LD))
        return out
    e = np.array([LD(20) * np.log10(np.sqrt(np.sum((w * x10[i:i + S.N_FRAME]) ** 2)) + eps)
                  for i in starts], dtype=LD)
    kept = [j for j in range(len(starts)) if e[j] > e.max() - LD(40)]
    K = len(kept)
    out.update(kept=K, energies=e)
    xs, ys = np.zeros((K - 1) * S.HOP + S.N_FRAME, dtype=LD), np.zeros((K - 1) * S.HOP + S.N_FRAME, dtype=LD)
    for k, j in enumerate(kept):
        xs[k * S.HOP:k * S.HOP + S.N_FRAME] += w * x10[starts[j]:starts[j] + S.N_FRAME]
        ys[k * S.HOP:k * S.HOP + S.N_FRAME] += w * y10[starts[j]:starts[j] + S.N_FRAME]
    J = K - 1
    if J < S.SEG:
        out.update(d=1e-5, status=1)
        return out
    C, Sn = _dft_matrix()
    k0 = BAND_TABLE[0][0]
    xb, yb = np.zeros((S.N_BANDS, J), dtype=LD), np.zeros((S.N_BANDS, J), dtype=LD)
    for sig, dst in ((xs, xb), (ys, yb)):
        fr = np.stack([w * sig[j * S.HOP:j * S.HOP + S.N_FRAME] for j in range(J)])
        p = (fr @ C.T) ** 2 + (fr @ Sn.T) ** 2
        for b, (lo, hi) in enumerate(BAND_TABLE):
            dst[b] = np.sqrt(p[:, lo - k0:hi - k0].sum(axis=1))
    clip = LD(1) + LD(10) ** (LD(15) / LD(20))
    total = LD(0)
    for m in range(S.SEG, J + 1):
        for b in range(S.N_BANDS):
            X, Y = xb[b, m - S.SEG:m], yb[b, m - S.SEG:m]
            alpha = np.sqrt(np.sum(X * X)) / (np.sqrt(np.sum(Y * Y)) + eps)
            Yp = np.minimum(alpha * Y, X * clip)
            Xc, Yc = X - np.sum(X) / LD(S.SEG), Yp - np.sum(Yp) / LD(S.SEG)
            Xc = Xc / (np.sqrt(np.sum(Xc * Xc)) + eps)
            Yc = Yc / (np.sqrt(np.sum(Yc * Yc)) + eps)
            total += np.sum(Xc * Yc)
    out.update(d=float(total / LD(S.N_BANDS * (J - S.SEG + 1))), status=0)
    return out


def e_pert(x, y, fs, runs=8, seed=2024):
    """max |d(perturbed spectra) - d| over `runs` seeded perturbations (0 without segments)."""
    x10, y10 = S.resample(x, fs), S.resample(y, fs)
    xs, ys, keep, _ = S.remove_silent_frames(x10, y10)
    if len(keep) - 1 < S.SEG:
        return 0.0
    X, Y = S.frame_spectra(xs), S.frame_spectra(ys)
    d0 = S.segment_score(S.band_values(X), S.band_values(Y))
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(runs):
        u = []
        for Z in (X, Y):
            v = rng.uniform(-1, 1, Z.shape) + 1j * rng.uniform(-1, 1, Z.shape)
            u.append(v / np.maximum(np.abs(v), 1.0))            # |u| <= 1
        d = S.segment_score(S.band_values(X + PERTURBATION * np.abs(X).max() * u[0]),
                            S.band_values(Y + PERTURBATION * np.abs(Y).max() * u[1]))
        worst = max(worst, abs(d - d0))
    return worst


# ----------------------------------------------------------------------------
# cases: one call of the kernel each (rows padded to the longest; lengths ragged)
# ----------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    fs: int
    speech: bool = False      # bundled speech at its own rate: the tolerance must stay below 5e-5


def stationary(n, seed):
    """A stationary AR(1) noise: every frame within a few dB of the loudest, so all are kept."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(n + 64)
    for i in range(1, len(v)):
        v[i] += 0.7 * v[i - 1]
    return (0.1 * v[64:]).astype(np.float32)


def n10_for_frames(nf, extra=1):
    """The shortest 10-kHz length with nf frames (extra = 1), or the exactly fitting length
    one sample shorter, which has nf - 1 (extra = 0): frames start at 0, 128, .. < n - 256."""
    return S.N_FRAME + S.HOP * (nf - 1) + extra


@functools.lru_cache(maxsize=None)
def full_triple():
    g, r = golden("inputs_test.npz"), golden("report_test.npz")
    f = lambda a: (a.astype(np.float64) / 32768.0).astype(np.float32)  # noqa: E731
    mix, tgt, est = f(g["mix"]), f(g["tgt"]), f(r["est16"])
    est = est[:, 0] if est.ndim > 1 else est
    n = min(len(mix), len(tgt), len(est), len(g["int"]))
    return tgt[:n], mix[:n, 0], est[:n]


@functools.lru_cache(maxsize=None)
def case_pairs(name):
    """-> tuple of (x, y) float32 pairs of the case (each pair its own length)."""
    tgt, mix0, _ = full_triple()
    rng = np.random.default_rng(77)
    if name == "fs10k-ragged":        # speech samples read as a 10-kHz signal
        return tuple((tgt[s:s + n], mix0[s:s + n]) for s, n in
                     ((40000, 10000), (16000, 7000), (60000, 9001)))
    if name == "fs16k-excerpts":
        out = []
        for s in EXCERPTS:
            x = tgt[s:s + 16000]
            out += [(x, mix0[s:s + 16000]),
                    (x, (x + 0.02 * rng.standard_normal(16000)).astype(np.float32))]
        return tuple(out)
    if name == "philox-scene":
        from avz import synth
        mix, t, _ = synth.make_batch_philox(1, start=5, n_samples=16000, n_interferers=2)
        return ((t[0], mix[0, 0]),)
    if name == "frame-rule":          # n10 = 256 + 128 q exactly, and one more
        out = []
        for i, n in enumerate((n10_for_frames(41, 0), n10_for_frames(41, 1))):
            x = stationary(n, 10 + i)
            out.append((x, (x + 0.05 * rng.standard_normal(n)).astype(np.float32)))
        return tuple(out)
    if name == "too-short":           # K = 30, K = 31, one frame short of any, n10 <= 256
        out = []
        for i, n in enumerate((n10_for_frames(30), n10_for_frames(31), 257, 256, 100, 0)):
            x = stationary(n, 20 + i)
            out.append((x, (x + 0.05 * rng.standard_normal(n)).astype(np.float32)))
        return tuple(out)
    if name == "tile-plus-one":       # J = TILE + 1 joined frames: a second block with one frame
        n = n10_for_frames(TILE + 2)
        x = stationary(n, 30)
        return ((x, (x + 0.05 * rng.standard_normal(n)).astype(np.float32)),)
    if name == "scaled-y":            # the packing leak: y 80 dB below
        x, y = case_pairs("fs16k-excerpts")[2]
        return ((x, y), (x, (np.float32(1e-4) * y).astype(np.float32)))
    if name == "identity":
        x = tgt[40000:56000]
        return ((x, x),)
    raise KeyError(name)


GPU_CASES = (Case("fs10k-ragged", 10000), Case("fs16k-excerpts", 16000, True),
             Case("philox-scene", 16000), Case("frame-rule", 10000), Case("too-short", 10000),
             Case("tile-plus-one", 10000), Case("scaled-y", 16000, True),
             Case("identity", 16000, True))


def pair_reference(x, y, fs):
    """The restatement's stages, E_ref, E_pert and the tolerance on d of one pair."""
    st = S.stoi_stages(x, y, fs)
    ld = stoi_ld(x, y, fs)
    e = st["energies"]
    margin = float(np.min(np.abs(e - (e.max() - S.DYN_RANGE_DB)))) if len(e) else float("inf")
    e_ref = abs(st["d"] - ld["d"])
    ep = e_pert(x, y, fs)
    n = min(len(st["x10"]), len(ld["x10"]))
    e_res = float(max(np.abs(st["x10"][:n] - ld["x10"][:n]).max(initial=0),
                      np.abs(st["y10"][:n] - ld["y10"][:n]).max(initial=0)))
    return dict(st=st, ld=ld, margin_db=margin, E_ref=e_ref, E_pert=ep, E_res=e_res,
                tol=1e-6 + 4 * e_ref + 4 * ep)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    fs = next(c.fs for c in GPU_CASES if c.name == name)
    return tuple(pair_reference(x, y, fs) for x, y in case_pairs(name))


def case_batch(name):
    """-> (clean [B, L], est [B, L] float32 zero-padded, lengths [B])."""
    pairs = case_pairs(name)
    L = max(len(x) for x, _ in pairs)
    clean, est = np.zeros((len(pairs), L), np.float32), np.zeros((len(pairs), L), np.float32)
    for b, (x, y) in enumerate(pairs):
        clean[b, :len(x)], est[b, :len(y)] = x, y
    return clean, est, [len(x) for x, _ in pairs]
