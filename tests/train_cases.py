"""Shared inputs of the training-batch tests (test_train_reference.py, test_gpu_train.py).

Three items of S = 8192 samples from seeded synth.speech_like sources (with their silenced
250-ms blocks): references tgt = 0.7 s0 and itf = 0.5 s1 + 0.5 s2 as float32, mix = two
channels of their sum plus small noise.
  item 0  as drawn;
  item 1  tgt and itf both zero over samples [2 N, 5 N): frames 5 .. 9 (frame t covers
          samples [(t - 1) H, (t + 1) H)) are all zeros in both references;
  item 2  itf all zero.
Two ragged length sets per transform size N (hop H = N / 2, T = ceil(len / H) + 1); set B
takes the items in the order (2, 0, 1):
  A  item 0: 15 H (T = 16, the block's 16 frames), item 1: 14 H (T = 15), item 2: N (T = 3)
  B  item 2: 14 H + 37 (T = 16, no multiple of the hop), item 0: 16 H (T = 17, a second
     block), item 1: N - 1 (shorter than a frame: not computed)
"""
import numpy as np

from avz import synth

S = 8192
SIZES = (512, 1024)
EPS32 = 2.0 ** -24


def _items(n_fft):
    out = []
    for i in range(3):
        rng = np.random.default_rng(4200 + i)
        s0, s1, s2 = (synth.speech_like(rng, S) for _ in range(3))
        tgt = (0.7 * s0).astype(np.float32)
        itf = (0.5 * s1 + 0.5 * s2).astype(np.float32)
        if i == 1:
            tgt[2 * n_fft:5 * n_fft] = 0.0
            itf[2 * n_fft:5 * n_fft] = 0.0
        if i == 2:
            itf[:] = 0.0
        clean = tgt.astype(np.float64) + itf.astype(np.float64)
        mix = np.stack([clean + 1e-3 * rng.standard_normal(S),
                        clean + 1e-3 * rng.standard_normal(S)]).astype(np.float32)
        out.append((mix, tgt, itf))
    return out


def batches(n_fft):
    """{"A": (mix [3, 2, S], tgt [3, S], itf [3, S], lens [3]), "B": ...} float32 / int32."""
    H = n_fft // 2
    it = _items(n_fft)
    sets = {"A": ((0, 1, 2), (15 * H, 14 * H, n_fft)),
            "B": ((2, 0, 1), (14 * H + 37, 16 * H, n_fft - 1))}
    out = {}
    for name, (order, lens) in sets.items():
        out[name] = (np.stack([it[i][0] for i in order]), np.stack([it[i][1] for i in order]),
                     np.stack([it[i][2] for i in order]), np.array(lens, np.int32))
    return out


def n_frames(length, n_fft):
    return -(-length // (n_fft // 2)) + 1


def band(sample, n_fft):
    """(in_band [F, T], both_zero [T]) of a train.Sample: the decisions a fp32 transform may
    take either way, |a - b| <= tol_t with tol_t = 8 log2(N) 2^-24 (2 / sqrt N) (||w tgt_t|| +
    ||w itf_t||), the norm-wise fp32 FFT error bound of both spectra in scipy's scaling; a
    frame whose two windowed references are all zeros is never in the band."""
    tol = 8 * np.log2(n_fft) * EPS32 * (2 / np.sqrt(n_fft)) * (sample.norms[0] + sample.norms[1])
    both_zero = (sample.norms[0] == 0) & (sample.norms[1] == 0)
    in_band = (np.abs(sample.mag_t - sample.mag_i) <= tol[None, :]) & ~both_zero[None, :]
    return in_band, both_zero


_REF = {}


def reference(n_fft, name):
    """Per item of batch `name`: None (len < N) or (Sample, in_band, both_zero), computed once
    by train.features_labels_numpy on the item's first len samples."""
    from avz import train
    key = (n_fft, name)
    if key not in _REF:
        mix, tgt, itf, lens = batches(n_fft)[name]
        ref = []
        for b, L in enumerate(lens):
            if L < n_fft:
                ref.append(None)
                continue
            s = train.features_labels_numpy(mix[b, :, :L], tgt[b, :L], itf[b, :L], n_fft)
            ref.append((s,) + band(s, n_fft))
        _REF[key] = ref
    return _REF[key]
