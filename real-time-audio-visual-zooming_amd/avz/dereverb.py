"""Mirror of rt_av_zoom/core/dereverb.py on the MI355X engine: WPE dereverberation.

``apply_wpe(y_mix)`` is the reference entry point (dereverb.py:26-106): STFT of the two
channels, WPE per bin (``avz_wpe_spectral``, taps=10, delay=3, iterations=3,
psd_context=0, full-frame statistics as dereverb.py:76-78 calls ``nara_wpe.wpe.wpe``),
inverse STFT, trim / zero-pad to the input length (:93-103). ``main(args)`` reads
``<outdir>/mixture.wav`` and writes ``<outdir>/mixture_wpe.wav`` (:108-138), the input of
``avz.oracle_reverb``. ``dereverb_batch`` is the batched device form.

The contract is the algorithm (offline batch WPE, Nakatani et al. 2010) as ``wpe_numpy``
states it in fp64, not bit parity with nara_wpe, which is not installed anywhere this
project is tested. Departures: degenerate bins pass the input through
with a status instead of NaN or an exception, and the framing is the engine's scipy
periodic-Hann STFT / iSTFT, not nara_wpe.utils.stft.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

FS = 16000
N_FFT = 512
N_HOP = 256
DEFAULT_OUTDIR = "simulation_results/ljspeech_reverb_20251130_215709"

EPS_FLOOR = 1e-10      # lambda = 1 / max(p, EPS_FLOOR * max_t p)


def pivot_threshold(taps: int) -> float:
    """A Cholesky pivot <= this multiple of its original diagonal entry is singular."""
    return (2 * taps + 1) * 2.0 ** -52


def regressor(Y, taps: int, delay: int):
    """Yt [taps * D, T] of Y [D, T]: row tau * D + m at frame t is Y[m, t - delay - tau]."""
    D, T = Y.shape
    Yt = np.zeros((taps * D, T), dtype=Y.dtype)
    for tau in range(taps):
        s = delay + tau
        if s < T:
            Yt[tau * D:(tau + 1) * D, s:] = Y[:, :T - s]
    return Yt


def _cholesky(R, thr):
    """Left-looking Cholesky of a Hermitian R -> (L or None, smallest pivot / R_jj)."""
    n = R.shape[0]
    L = np.zeros_like(R)
    rel = np.inf
    for j in range(n):
        v = R[j:, j] - L[j:, :j] @ L[j, :j].conj()
        d, djj = v[0].real, R[j, j].real
        if not (d > thr * djj) or not np.isfinite(d):
            return None, (d / djj if djj > 0 and np.isfinite(d) else 0.0)
        rel = min(rel, d / djj)
        l = np.sqrt(d)
        L[j, j] = l
        L[j + 1:, j] = v[1:] / l
    return L, rel


def _solve_chol(L, P):
    """G with L L^H G = P."""
    n = L.shape[0]
    Z = np.zeros_like(P)
    for i in range(n):
        Z[i] = (P[i] - L[i, :i] @ Z[:i]) / L[i, i].real
    G = np.zeros_like(P)
    for i in range(n - 1, -1, -1):
        G[i] = (Z[i] - L[i + 1:, i].conj() @ G[i + 1:]) / L[i, i].real
    return G


def wpe_bin(Y, taps=10, delay=3, iterations=3, row_order=None):
    """One bin: Y [D, T] complex -> (X [D, T] complex128, status, smallest relative pivot).
    ``row_order``: an optional permutation of the regressor's rows (X does not depend on it
    beyond rounding)."""
    Y = np.asarray(Y, dtype=np.complex128)
    D, T = Y.shape
    n = taps * D
    if T - delay < n:          # fewer regressor frames than unknowns: by the count alone
        return Y.copy(), 2, np.nan
    Yt = regressor(Y, taps, delay)
    if row_order is not None:
        Yt = Yt[np.asarray(row_order)]
    thr = pivot_threshold(taps)
    X, rel_min = Y.copy(), np.inf
    for _ in range(iterations):
        p = np.mean(X.real ** 2 + X.imag ** 2, axis=0)
        pm = p.max()
        if pm == 0:
            return Y.copy(), 1, rel_min
        lam = 1.0 / np.maximum(p, EPS_FLOOR * pm)
        Yl = Yt * lam
        R = Yl @ Yt.conj().T
        P = Yl @ Y.conj().T
        with np.errstate(invalid="ignore", divide="ignore"):
            L, rel = _cholesky(R, thr)
        if L is None:
            return Y.copy(), 2, rel
        rel_min = min(rel_min, rel)
        G = _solve_chol(L, P)
        X = Y - G.conj().T @ Yt
    return X, 0, rel_min


def wpe_numpy(Y, taps=10, delay=3, iterations=3, frames=None, return_info=False):
    """The algorithm in fp64: Y [2, F, T] complex -> X [2, F, T] complex128 (and, with
    ``return_info``, status [F] and the smallest relative Cholesky pivot per bin). ``frames``:
    only the first ``frames`` frames are processed; the rest are copies of Y."""
    Y = np.asarray(Y)
    _, F, T = Y.shape
    Tb = T if frames is None else max(0, min(int(frames), T))
    X = Y.astype(np.complex128)
    status = np.zeros(F, dtype=np.int32)
    rel = np.full(F, np.nan)
    for k in range(F):
        X[:, k, :Tb], status[k], rel[k] = wpe_bin(Y[:, k, :Tb], taps, delay, iterations)
    return (X, status, rel) if return_info else X


def _plan(n_fft, batch, samples):
    from .engine import MVDRPlan, out_length
    return MVDRPlan(n_fft=n_fft, mask="ones", postfilter="none", normalize="none",
                    max_batch=2 * batch, max_samples=out_length(samples, n_fft // 2))


def dereverb_batch(mix, lengths=None, taps=10, delay=3, iterations=3, n_fft=N_FFT, plan=None,
                   status=None, stream=None):
    """mix [B, 2, S] float32 on the device (lengths: int32 [B] or None = S) -> dereverberated
    [B, 2, S] float32: plan.stft -> avz_wpe_spectral (in place) -> plan.istft per channel,
    trimmed to S; samples at or beyond lengths[b] are zero. ``plan``: an un-normalised
    MVDRPlan of this n_fft with max_batch >= 2 B (made here when None)."""
    import torch
    from .engine import n_frames, wpe_spectral
    if mix.dim() != 3 or mix.shape[1] != 2 or mix.dtype != torch.float32 or not mix.is_cuda:
        raise ValueError("mix must be float32 [B, 2, S] on the device")
    B, _, S = mix.shape
    if plan is None:
        plan = _plan(n_fft, B, S)
    hop = plan.hop
    if lengths is None:
        frames, max_len = None, S
    else:
        max_len = int(lengths.max().item())
        frames = (torch.div(lengths + (hop - 1), hop, rounding_mode="floor") + 1).to(torch.int32)
    Y = plan.stft(mix, lengths, max_len, stream=stream)
    T = n_frames(max_len, hop)
    wpe_spectral(Y, taps, delay, iterations, frames=frames, out=Y, status=status, stream=stream)
    y, _ = plan.istft(Y.view(2 * B, plan.F, T), stream=stream)
    n = min(S, (T - 1) * hop)
    out = torch.zeros((B, 2, S), dtype=torch.float32, device=mix.device)
    out[:, :, :n] = y.view(B, 2, -1)[:, :, :n]
    if lengths is not None:
        out *= (torch.arange(S, device=mix.device)[None, None, :] < lengths[:, None, None])
    return out


def apply_wpe(y_mix, taps=10, delay=3, iterations=3, n_fft=N_FFT, device="cuda"):
    """(Channels, Samples) float32 -> dereverberated (Channels, Samples) float32 numpy
    (dereverb.py:26-106). An input the STFT cannot frame is returned as it is, as the
    reference's error paths do (:37-39)."""
    import torch
    y_mix = np.ascontiguousarray(y_mix, dtype=np.float32)
    print(f"  [WPE] Input Time-Domain Shape: {y_mix.shape}")
    if y_mix.ndim != 2 or y_mix.shape[0] != 2 or y_mix.shape[1] < n_fft:
        print(f"  [Error] STFT failed: need (2, >= {n_fft}) samples")
        return y_mix
    x = torch.from_numpy(y_mix)[None].to(torch.device(device))
    out = dereverb_batch(x, None, taps, delay, iterations, n_fft)[0].cpu().numpy()
    print(f"  [WPE] Output Time-Domain Shape: {out.shape}")
    return out


def main(args):
    from . import wavio
    outdir = args.outdir
    if outdir is None:
        print("Error: No simulation directory found.")
        return None
    print("--- Running Standalone WPE Dereverberation ---")
    print(f"Target Directory: {os.path.basename(outdir)}")
    mix_path = os.path.join(outdir, "mixture.wav")
    if not os.path.exists(mix_path):
        print(f"Error: {mix_path} not found.")
        return None
    y_mix, fs = wavio.read(mix_path, dtype="float32")
    if y_mix.ndim > 1 and y_mix.shape[0] > y_mix.shape[1]:   # (:127-129) to (channels, samples)
        print(f"  [Load] Transposing input from {y_mix.shape} to (Channels, Samples)")
        y_mix = y_mix.T
    y_clean = apply_wpe(y_mix, taps=args.taps, delay=args.delay, iterations=args.iters)
    out_path = os.path.join(outdir, "mixture_wpe.wav")
    wavio.write(out_path, y_clean.T, fs)
    print(f"Success! Saved to: {out_path}")
    return y_clean


def parse_args(argv=None):
    """The reference CLI (dereverb.py:140-148)."""
    p = argparse.ArgumentParser()
    p.add_argument("--outdir", type=str, default=DEFAULT_OUTDIR)
    p.add_argument("--taps", type=int, default=10)
    p.add_argument("--delay", type=int, default=3)
    p.add_argument("--iters", type=int, default=3)
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
