"""Shared inputs and fp64 references of the delay-mask tests (test_delay_mask_reference.py,
test_gpu_delay_mask.py).

Cases (N, d) = (512, 0.08), (1024, 0.08), (1024, 0.04), (512, 0.01); three utterances per case:
synth.make_scene_philox(idx, 17 H, 1, d=d, snr_db=20), idx 0, 1, 2, cut to 17 H, 17 H - 37 and
9 H + H / 2 + 5 samples (18, 18 and 11 frames: two blocks of 16 frames with a ragged second
one, and a single ragged block; no last frame that holds only a few samples). buffers() puts
them into NaN-filled rows with strides longer than the rows.

reference() runs the restatement avz.delay_mask once per (case, utterance, angle) and keeps the
result with its perturbation figures: PERTS seeded perturbations of Y by STAGE max|Y| (|u| <= 1
per bin), the repository's STFT tolerance, give E_pert (largest change of h), D_pert (largest
change of a kept delay) and whether every perturbed run kept the same peak bins."""
import numpy as np

from avz import delay_mask as DM
from avz import synth
from oracle import avz_oracle as O

CASES = [(512, 0.08), (1024, 0.08), (1024, 0.04), (512, 0.01)]
UTTS = 3
STAGE = 2e-6
PERTS = 8
FS, C_SOUND = 16000, 343.0


def lengths(n_fft):
    H = n_fft // 2
    return [17 * H, 17 * H - 37, 9 * H + H // 2 + 5]


_MIX, _REF, _LONG = {}, {}, {}


def utterances(n_fft, d):
    """The three cut mixtures, each [2, len] float32."""
    if (n_fft, d) not in _MIX:
        H = n_fft // 2
        _MIX[n_fft, d] = [synth.make_scene_philox(i, 17 * H, 1, d=d, snr_db=20.0)[0][:, :L].copy()
                          for i, L in enumerate(lengths(n_fft))]
    return _MIX[n_fft, d]


def buffers(n_fft, d, order=(0, 1, 2)):
    """(mix [B, 2 ch_stride + 11] float32 NaN-filled rows, lens int32 [B], ch_stride, max_len)
    holding utterances `order`."""
    H = n_fft // 2
    max_len = 17 * H
    ch = max_len + 13
    buf = np.full((len(order), 2 * ch + 11), np.nan, np.float32)
    lens = []
    for r, i in enumerate(order):
        x = utterances(n_fft, d)[i]
        buf[r, :x.shape[1]] = x[0]
        buf[r, ch:ch + x.shape[1]] = x[1]
        lens.append(x.shape[1])
    return buf, np.array(lens, np.int32), ch, max_len


def spectra(x, n_fft):
    """The library's STFT of a [2, len] mixture in the oracle's restatement: complex64
    [2, F, T], T = ceil(len / H) + 1."""
    return O.stft(x, fs=FS, nperseg=n_fft, noverlap=n_fft // 2)[2]


def perturbations(Y, seed):
    """PERTS arrays like Y: STAGE max|Y| u, |u| <= 1 per bin."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(PERTS):
        u = rng.uniform(-1, 1, Y.shape) + 1j * rng.uniform(-1, 1, Y.shape)
        out.append(STAGE * np.abs(Y).max() * u / np.maximum(np.abs(u), 1.0))
    return out


def reference_of(x, n_fft, d, angle=90.0, seed=0, **kw):
    """The restatement on one mixture and its perturbation figures."""
    Y = spectra(x, n_fft)
    g = DM.delay_grid(n_fft, FS, d, C_SOUND, kw.get("hist_bins", 65), kw.get("f_lo", 100.0))
    pk = {k: v for k, v in kw.items() if k in ("smooth", "rel_height", "min_sep", "max_peaks")}
    h = DM.delay_histogram(Y[0], Y[1], g)
    delays, J, bins = DM.delay_peaks(h, g, angle, **pk)
    perts = perturbations(Y, seed)
    e_pert = d_pert = 0.0
    same = True
    for p in perts:
        Yp = Y + p
        hp = DM.delay_histogram(Yp[0], Yp[1], g)
        dp, Jp, bp = DM.delay_peaks(hp, g, angle, **pk)
        e_pert = max(e_pert, np.abs(hp - h).max())
        same = same and bp == bins
        if bp == bins and J:
            d_pert = max(d_pert, np.abs(dp[1:1 + J] - delays[1:1 + J]).max())
    return dict(Y=Y, grid=g, h=h, delays=delays, J=J, bins=bins, perts=perts, e_pert=e_pert,
                d_pert=d_pert, same_peaks=same, peak_kw=pk,
                mask=DM.delay_labels(Y[0], Y[1], delays, J, n_fft))


def reference(n_fft, d, i, angle=90.0):
    k = (n_fft, d, i, angle)
    if k not in _REF:
        _REF[k] = reference_of(utterances(n_fft, d)[i], n_fft, d, angle, seed=4100 + i)
    return _REF[k]


def stable_labels(ref, delays, J, n_fft):
    """(M, stable): the restatement's labels with the given delays, and the decisions that
    none of the reference's perturbations flips."""
    Y = ref["Y"]
    M = DM.delay_labels(Y[0], Y[1], delays, J, n_fft)
    stable = np.ones(M.shape, bool)
    for p in ref["perts"]:
        Yp = Y + p
        stable &= DM.delay_labels(Yp[0], Yp[1], delays, J, n_fft) == M
    return M, stable


def long_scenes(snr_db):
    """The 4-s scenes idx 0-2 at d = 0.08 (N = 1024 tests): [(mix [2, S], tgt, itf)]."""
    if snr_db not in _LONG:
        _LONG[snr_db] = [synth.make_scene_philox(i, 64000, 1, d=0.08, snr_db=snr_db)
                         for i in range(UTTS)]
    return _LONG[snr_db]


def sir_db(out, tgt, itf):
    L = min(len(out), len(tgt))
    return O.projection_sdr_sir(np.asarray(out[:L], np.float64), tgt[:L], itf[:L])[1]
