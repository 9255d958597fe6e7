"""CPU checks of the training-batch surface: avz.train.features_labels_numpy against a direct
transcription of full_audio_generating_pipeline/model_training.py:80-90, the export and the
argument checks of avz_mask_training_batch that need no plan, and the test cases' own
decision band (tests/train_cases.py) measured on scipy's float32 transform. No GPU: the
kernel's checks are in test_gpu_train.py."""
import ctypes as ct

import numpy as np
import pytest
import scipy.signal

import train_cases as TC
from avz import _lib, train


def test_restatement_equals_the_reference_lines():
    N_FFT, HOP, FS = 1024, 512, 16000
    mix, tgt, itf, lens = TC.batches(N_FFT)["A"]
    L = int(lens[0])
    y_mix, tgt, int_sig = (a.astype(np.float64) for a in (mix[0, :, :L], tgt[0, :L], itf[0, :L]))
    # model_training.py:80-90
    f, t, Y = scipy.signal.stft(y_mix, fs=FS, nperseg=N_FFT, noverlap=N_FFT - HOP)
    _, _, S_t = scipy.signal.stft(tgt, fs=FS, nperseg=N_FFT, noverlap=N_FFT - HOP)
    _, _, S_i = scipy.signal.stft(int_sig, fs=FS, nperseg=N_FFT, noverlap=N_FFT - HOP)
    mag = np.abs(Y)
    ipd = np.angle(Y[0]) - np.angle(Y[1])
    feat = np.stack([np.log(mag[0] + 1e-7), ipd], axis=0)
    mask = np.where(np.abs(S_t) > np.abs(S_i), 1.0, 0.0)

    s = train.features_labels_numpy(mix[0, :, :L], tgt, int_sig, N_FFT)
    assert s.feat.dtype == np.float64 and s.feat.shape == (2, 513, TC.n_frames(L, N_FFT))
    assert np.array_equal(s.feat, feat) and np.array_equal(s.label, mask)
    assert np.array_equal(s.mag_t, np.abs(S_t)) and np.array_equal(s.mag_i, np.abs(S_i))
    # the frame norms are those of the frames scipy transformed: Parseval, in scipy's scaling
    # ||S||_2 over all N bins = (2 / sqrt N) ||w x||_2 (the one-sided spectrum doubles the
    # interior bins)
    for S, n in ((S_t, s.norms[0]), (S_i, s.norms[1])):
        full = 2 * (np.abs(S) ** 2).sum(axis=0) - np.abs(S[0]) ** 2 - np.abs(S[-1]) ** 2
        assert np.allclose(np.sqrt(full), 2 / np.sqrt(N_FFT) * n, rtol=1e-12, atol=1e-300)


def test_export_and_null_arguments():
    lib = _lib.lib
    assert "avz_mask_training_batch" in _lib.EXPORTED
    assert lib.avz_version() == 3
    one = ct.c_void_p(8)  # never dereferenced: every call below fails its checks first
    base = dict(plan=one, len=one, mix=one, tgt=one, itf=one, feat=one, label=one)

    def call(layout=_lib.FEAT_LOGMAG_IPD, **kw):
        a = {**base, **kw}
        return lib.avz_mask_training_batch(a["plan"], layout, 1, a["len"], 1024, a["mix"], 2048,
                                           1024, a["tgt"], a["itf"], 1024, a["feat"], 1, 1, 1, 1,
                                           a["label"], 1, 1, 1, None)
    for name in base:
        assert call(**{name: None}) == _lib.AVZ_ERR_ARG, name
    # (a bad layout and the AVZ_ERR_SHAPE checks need a plan: test_gpu_train.py)


@pytest.mark.parametrize("n_fft", TC.SIZES)
def test_case_band_on_scipy_float32(n_fft):
    """The cases' own band, re-checked where no kernel is involved: the share of decisions
    within tol_t (at most the 0.5 % the GPU test allows to be left out), and scipy's float32
    transform of the same inputs against float64: no decision outside the band differs."""
    hop = n_fft // 2
    for name in ("A", "B"):
        mix, tgt, itf, lens = TC.batches(n_fft)[name]
        for b, ref in enumerate(TC.reference(n_fft, name)):
            if ref is None:
                continue
            s, in_band, both_zero = ref
            L = int(lens[b])
            share = in_band.mean()
            kw = dict(fs=16000, nperseg=n_fft, noverlap=n_fft - hop)
            S32 = [scipy.signal.stft(x[b, :L], **kw)[2] for x in (tgt, itf)]
            S64 = [scipy.signal.stft(x[b, :L].astype(np.float64), **kw)[2] for x in (tgt, itf)]
            assert S32[0].dtype == np.complex64 and S64[0].dtype == np.complex128
            lab32 = np.where(np.abs(S32[0]) > np.abs(S32[1]), 1.0, 0.0)
            diff = lab32 != s.label
            tol = 8 * np.log2(n_fft) * TC.EPS32 * (2 / np.sqrt(n_fft)) * (s.norms[0] + s.norms[1])
            err = max((np.abs(a - c).max(axis=0) / np.where(tol > 0, tol, np.inf)).max()
                      for a, c in zip(S32, S64))
            print(f"N={n_fft} {name}[{b}] len {L}: in band {100 * share:.3f} %, float32 "
                  f"decisions differing {int(diff.sum())} of {diff.size}, worst float32 bin "
                  f"error / tol_t {err:.4f}, both-zero frames {int(both_zero.sum())}")
            assert share <= 0.005
            assert not (diff & ~in_band).any()
            assert (lab32[:, both_zero] == 0).all() and (s.label[:, both_zero] == 0).all()


def test_cases_hold_what_they_claim():
    for n_fft in TC.SIZES:
        refs = {n: TC.reference(n_fft, n) for n in ("A", "B")}
        lens = {n: TC.batches(n_fft)[n][3] for n in ("A", "B")}
        T = sorted(TC.n_frames(int(v), n_fft) for n in lens for v in lens[n] if v >= n_fft)
        assert T == [3, 15, 16, 16, 17]
        assert any(v % (n_fft // 2) for v in lens["B"][:2]) and refs["B"][2] is None
        assert list(np.flatnonzero(refs["A"][1][2])[:5]) == [5, 6, 7, 8, 9]   # the zero block
        assert (refs["A"][2][0].mag_i == 0).all() and (refs["B"][0][0].mag_i == 0).all()
