"""Short-time objective intelligibility (STOI; Taal, Hendriks, Heusdens, Jensen 2011).

The reference's ``evaluate_run`` scores ``stoi(s_tgt, s_est, config.FS, extended=False)``
(Final_pipeline/src/metrics.py:157-160) with pystoi. pystoi is installed nowhere this project
is built or tested, so the contract is the published algorithm as ``stoi_numpy`` states it in
fp64, not pystoi's bits:

 1. 16 kHz -> 10 kHz with ``scipy.signal.resample_poly(s, 5, 8, window=h / sum(h))``, h the
    581-tap Octave-compatible Kaiser design (``resample_taps``); 10 kHz passes through;
 2. 256-sample frames at hop 128 under ``np.hanning(258)[1:-1]``, starting at
    0, 128, ... < n10 - 256; the frames whose clean energy is within 40 dB of the loudest are
    kept and overlap-added;
 3. the same framing of the joined signals, windowed again, 512-point rfft;
 4. 15 third-octave bands from 150 Hz (``BANDS``): sqrt of the summed bin powers;
 5. per 30-frame segment and band: scale y to x's norm, clip at x (1 + 10^(15/20)),
    correlate the mean-removed unit vectors; d = the mean correlation;
 6. fewer than 30 joined frames: d = 1e-5 with status 1 (pystoi's warning value).

``stoi_batch`` runs device tensors through ``avz_stoi_batch`` (csrc/avz_stoi.hip) and host
tensors through the restatement.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

FS_INTERNAL = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
N_BANDS = 15
MIN_FREQ = 150.0
SEG = 30                      # frames per segment (384 ms)
BETA_DB = 15.0                # clip: y' <= x (1 + 10^(BETA_DB / 20))
DYN_RANGE_DB = 40.0
EPS = 2.0 ** -52
TOO_SHORT = 1e-5              # pystoi's value when no segment fits
RES_UP, RES_DOWN, RES_HALF = 5, 8, 290

# status values of info[:, 0]
STATUS_OK, STATUS_SHORT, STATUS_NONFINITE = 0, 1, 2


def window() -> np.ndarray:
    """np.hanning(258)[1:-1]: w[n] = 0.5 (1 - cos(2 pi (n + 1) / 257))."""
    return np.hanning(N_FRAME + 2)[1:-1]


def resample_taps() -> np.ndarray:
    """The 581 taps h of pystoi's Octave-compatible 16 -> 10 kHz design (before h / sum h)."""
    fc = 1.0 / (2 * max(RES_UP, RES_DOWN))
    rej = 60.0
    L = int(np.ceil((rej - 8.0) / (28.714 * fc / 10)))
    assert L == RES_HALF
    t = np.arange(-L, L + 1)
    return np.kaiser(2 * L + 1, 0.1102 * (rej - 8.7)) * 2 * RES_UP * fc * np.sinc(2 * fc * t)


def band_edges():
    """[(lo, hi)] bins of the 15 third-octave bands on the grid k * 10000 / 512."""
    f = np.linspace(0, FS_INTERNAL, NFFT + 1)[:NFFT // 2 + 1]
    out = []
    for b in range(N_BANDS):
        lo = MIN_FREQ * 2.0 ** ((2 * b - 1) / 6.0)
        hi = MIN_FREQ * 2.0 ** ((2 * b + 1) / 6.0)
        out.append((int(np.argmin((f - lo) ** 2)), int(np.argmin((f - hi) ** 2))))
    return out


BANDS = band_edges()


def resampled_len(n: int, fs) -> int:
    return -(-RES_UP * n // RES_DOWN) if int(fs) == 16000 else n


def resample(s, fs):
    """Step 1 in fp64."""
    s = np.asarray(s, dtype=np.float64)
    if int(fs) == FS_INTERNAL:
        return s
    if int(fs) != 16000:
        raise ValueError("fs must be 16000 or 10000")
    if len(s) == 0:
        return s
    import scipy.signal
    h = resample_taps()
    return scipy.signal.resample_poly(s, RES_UP, RES_DOWN, window=h / h.sum())


def frame_starts(n: int):
    return range(0, n - N_FRAME, HOP)


def frame_energies(x10):
    """e_j = 20 log10(||w x_frame_j|| + EPS) of the clean 10-kHz signal."""
    w = window()
    fr = np.array([w * x10[i:i + N_FRAME] for i in frame_starts(len(x10))]).reshape(-1, N_FRAME)
    with np.errstate(divide="ignore"):
        return 20 * np.log10(np.sqrt(np.sum(fr * fr, axis=1)) + EPS)


def remove_silent_frames(x10, y10):
    """Step 2 -> (x_sil, y_sil, kept frame indices, energies)."""
    w = window()
    e = frame_energies(x10)
    if len(e) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int64), e
    keep = np.flatnonzero(e > e.max() - DYN_RANGE_DB)
    K = len(keep)
    n = (K - 1) * HOP + N_FRAME if K else 0
    xs, ys = np.zeros(n), np.zeros(n)
    for k, j in enumerate(keep):
        xs[k * HOP:k * HOP + N_FRAME] += w * x10[j * HOP:j * HOP + N_FRAME]
        ys[k * HOP:k * HOP + N_FRAME] += w * y10[j * HOP:j * HOP + N_FRAME]
    return xs, ys, keep, e


def frame_spectra(s):
    """Step 3: rfft of the doubly windowed frames -> complex [J, 257]."""
    w = window()
    fr = np.array([w * s[i:i + N_FRAME] for i in frame_starts(len(s))]).reshape(-1, N_FRAME)
    return np.fft.rfft(fr, n=NFFT, axis=1)


def band_values(spec):
    """Step 4: [J, 257] spectra -> [15, J] third-octave band magnitudes."""
    p = spec.real ** 2 + spec.imag ** 2
    return np.sqrt(np.stack([p[:, lo:hi].sum(axis=1) for lo, hi in BANDS]))


def segment_score(xb, yb):
    """Step 5: band values [15, J] (J >= 30) -> d."""
    J = xb.shape[1]
    idx = np.arange(SEG)[None, :] + np.arange(J - SEG + 1)[:, None]          # [M, 30]
    X, Y = xb[:, idx].transpose(1, 0, 2), yb[:, idx].transpose(1, 0, 2)       # [M, 15, 30]
    nrm = lambda a: np.sqrt(np.sum(a * a, axis=2, keepdims=True))  # noqa: E731
    alpha = nrm(X) / (nrm(Y) + EPS)
    Yp = np.minimum(Y * alpha, X * (1 + 10 ** (BETA_DB / 20)))
    Yp = Yp - Yp.mean(axis=2, keepdims=True)
    Xc = X - X.mean(axis=2, keepdims=True)
    Yp = Yp / (nrm(Yp) + EPS)
    Xc = Xc / (nrm(Xc) + EPS)
    return float(np.sum(Yp * Xc) / (N_BANDS * X.shape[0]))


def stoi_stages(x, y, fs):
    """Every stage of the restatement as a dict: x10, y10, energies, keep, xs, ys (the joined
    signals), xb, yb ([15, J] band values), d, status."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 1:
        raise ValueError("x and y must be 1-d arrays of equal length")
    x10, y10 = resample(x, fs), resample(y, fs)
    xs, ys, keep, e = remove_silent_frames(x10, y10)
    out = dict(x10=x10, y10=y10, energies=e, keep=keep, frames=len(e), xs=xs, ys=ys,
               xb=np.zeros((N_BANDS, 0)), yb=np.zeros((N_BANDS, 0)))
    if len(e) and not np.isfinite(e.max()):
        out.update(d=float("nan"), status=STATUS_NONFINITE)
        return out
    if len(keep) >= 2:
        out["xb"], out["yb"] = band_values(frame_spectra(xs)), band_values(frame_spectra(ys))
    J = out["xb"].shape[1]
    if J < SEG:
        out.update(d=TOO_SHORT, status=STATUS_SHORT)
    else:
        out.update(d=segment_score(out["xb"], out["yb"]), status=STATUS_OK)
    return out


def stoi_numpy(x, y, fs=16000) -> float:
    """The fp64 restatement: clean x, processed y (equal length), fs 16000 or 10000 -> d."""
    return stoi_stages(x, y, fs)["d"]


def stoi_info_numpy(x, y, fs=16000) -> dict:
    """Frame counts of the restatement and its keep-decision margin: status, frames, kept,
    segments, margin_db = min_j |e_j - (max e - 40)| (inf without frames)."""
    s = stoi_stages(x, y, fs)
    e = s["energies"]
    J = s["xb"].shape[1]
    margin = float(np.min(np.abs(e - (e.max() - DYN_RANGE_DB)))) if len(e) else float("inf")
    return dict(status=s["status"], frames=int(s["frames"]), kept=int(len(s["keep"])),
                segments=max(J - SEG + 1, 0), margin_db=margin, d=s["d"])


def workspace_bytes(batch: int, max_len: int, fs=16000) -> int:
    from ._lib import check, lib
    return check(lib.avz_stoi_workspace_bytes(int(batch), int(max_len), float(fs)),
                 "avz_stoi_workspace_bytes")


def stoi_batch(clean, est, lengths=None, fs=16000, stream=None, resampled=None, tob=None,
               workspace=None):
    """STOI of est[b] against clean[b]: float32 [B, L] (or [L]) tensors -> (d float64 [B],
    info int32 [B, 4] = status, frames, kept frames K, segments). ``lengths``: optional
    samples per row. Device tensors run ``avz_stoi_batch``; host tensors the restatement.
    ``resampled`` (float32 [B, 2, >= n10]) and ``tob`` (float64 [B, 2, 15, >= K - 1]) are the
    kernel's optional stage exports (device only). ``workspace``: an optional uint8 device
    tensor of at least workspace_bytes(B, L, fs) bytes (one is allocated otherwise)."""
    import torch
    if clean.dim() == 1:
        clean, est = clean[None], est[None]
    if clean.shape != est.shape or clean.dim() != 2:
        raise ValueError("clean and est must be [B, L] tensors of one shape")
    if int(fs) not in (16000, FS_INTERNAL):
        raise ValueError("fs must be 16000 or 10000")
    B, L = clean.shape
    if not clean.is_cuda:
        lens = [L] * B if lengths is None else [max(0, min(int(n), L)) for n in lengths]
        d = np.empty(B)
        info = np.zeros((B, 4), dtype=np.int32)
        for b in range(B):
            r = stoi_info_numpy(clean[b, :lens[b]].double().numpy(),
                                est[b, :lens[b]].double().numpy(), fs)
            d[b] = r["d"]
            info[b] = r["status"], r["frames"], r["kept"], r["segments"]
        return torch.from_numpy(d), torch.from_numpy(info)

    from . import _args as A
    from ._args import ptr
    from ._lib import AvzStoiArgs
    dev = clean.device
    clean, est = (v if v.dtype == torch.float32 and v.stride(1) == 1 else v.float().contiguous()
                  for v in (clean, est))
    if est.device != dev:
        raise ValueError("clean and est must be on one device")
    if lengths is not None:
        lengths = torch.as_tensor(lengths, dtype=torch.int32).to(dev).contiguous()
    d = torch.empty(B, dtype=torch.float64, device=dev)
    info = torch.empty((B, 4), dtype=torch.int32, device=dev)
    ws = workspace
    if ws is None:
        ws = torch.empty(max(workspace_bytes(B, L, fs), 1), dtype=torch.uint8, device=dev)
    else:
        A.tensor("workspace", ws, torch.uint8, A.ge(0), dev, A.FULL)
    A.outputs((("resampled", resampled, (None, None, None), torch.float32),
               ("tob", tob, (None, None, None, None), torch.float64)), dev)
    a = AvzStoiArgs()
    a.batch, a.max_len = B, L
    a.len = ptr(lengths)
    a.fs = float(fs)
    a.clean, a.clean_stride = ptr(clean), clean.stride(0)
    a.est, a.est_stride = ptr(est), est.stride(0)
    a.stoi, a.info = ptr(d), ptr(info)
    if resampled is not None:
        a.resampled, a.res_stride = ptr(resampled), resampled.shape[2]
    if tob is not None:
        a.tob, a.tob_stride = ptr(tob), tob.shape[3]
    a.workspace, a.workspace_bytes = ptr(ws), ws.numel()
    A.call("avz_stoi_batch", ct.byref(a), stream=stream, device=dev)
    if workspace is None:
        ws.record_stream(stream if stream is not None else torch.cuda.current_stream(dev))
    return d, info
