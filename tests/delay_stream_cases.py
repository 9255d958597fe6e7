"""Shared inputs and fp64 references of the streaming delay-mask tests
(test_delay_stream_reference.py, test_gpu_delay_stream.py).

Cases: the four (N, d) of delay_mask_cases.CASES; three streams per case, scenes
synth.make_scene_philox(i, 17 H, 1, d=d, snr_db=20)[0], i = 0, 1, 2, cut after CUTS = 17, 16 and
10 hops, padded to HOPS = 17 hops, plus the drain hop of zeros: T = 18 pushed hops = 18 frames
(two full groups of the kernel's eight frames and a ragged one, as stream_cases). Past its cut
a stream goes on with its own scene at 2^-4 (24 dB down) and not with digital zeros: a frame of
zeros labels every bin by a tie, which any perturbation of the spectrum flips, so zero padding
alone makes 5.6 % of stream 1's and 39 % of stream 2's decisions unstable, against a cap of
1 %. (The zero frame's own contract, M = 1 and no deposit, has a GPU test of its own.)

The restatement's input is delay_mask_cases.spectra of the 17-hop signal: its 18 frames are
the pushed frames. reference() runs avz.delay_mask.delay_mask_stream_numpy once per (case,
stream, forget, ...) and keeps the result with its per-frame perturbation figures over
delay_mask_cases.perturbations (8 seeded, 2e-6 max|Y|): E_pert(t), the largest change of h_t;
D_pert(t), the largest change of a kept delay; stable(t), whether every perturbed run kept frame
t's peak bins. stable_labels() gives the restatement's labels at given lists and the decisions
no perturbation flips at those lists."""
import numpy as np

import delay_mask_cases as DC
from avz import delay_mask as DM
from avz import stream as ST
from avz import synth

CASES = DC.CASES
HOPS, T = 17, 18
STREAMS = 3
CUTS = (17, 16, 10)
TAIL = 2.0 ** -4
GROUPINGS = {"one": [T], "single": [1] * T, "ragged": [3, 1, 8, 6]}
FORGETS = (1.0, 0.9)
FS, C_SOUND = DC.FS, DC.C_SOUND

_IN, _REF, _E2E = {}, {}, {}


def inputs(n_fft, d):
    """mix [3, 2, T H] float32: the three streams' pushed hops (the last one zeros)."""
    if (n_fft, d) not in _IN:
        H = n_fft // 2
        mix = np.zeros((STREAMS, 2, T * H), np.float32)
        for i, cut in enumerate(CUTS):
            x = synth.make_scene_philox(i, HOPS * H, 1, d=d, snr_db=20.0)[0].astype(np.float32)
            x[:, cut * H:] *= np.float32(TAIL)
            mix[i, :, :HOPS * H] = x
        _IN[n_fft, d] = mix
    return _IN[n_fft, d]


def spectra(n_fft, d, s):
    """Y [2, F, T] complex64 of stream s: frame t is the t-th pushed frame."""
    Y = DC.spectra(inputs(n_fft, d)[s][:, :HOPS * (n_fft // 2)], n_fft)
    assert Y.shape[2] == T
    return Y


def run_numpy(Y, n_fft, d, forget=1.0, adapt=None, angle=90.0):
    """The restatement on frames Y [2, F, T]: dict(M, h [T, nb], lists [T, 8], J [T], bins)."""
    M, h, lists, J = DM.delay_mask_stream_numpy(Y[0], Y[1], n_fft, FS, d, C_SOUND,
                                                forget=forget, adapt=adapt, angle=angle)
    g = DM.delay_grid(n_fft, FS, d, C_SOUND)
    bins = [DM.delay_peaks(h[t], g, angle)[2] for t in range(h.shape[0])]
    return dict(M=M, h=h, lists=lists, J=J, bins=bins, grid=g)


def with_perturbations(Y, n_fft, d, seed, forget=1.0, adapt=None, angle=90.0):
    """run_numpy's result with Y, perts, e_pert [T], d_pert [T] and stable [T]."""
    r = run_numpy(Y, n_fft, d, forget, adapt, angle)
    Tn = Y.shape[2]
    perts = DC.perturbations(Y, seed)
    e_pert, d_pert, stable = np.zeros(Tn), np.zeros(Tn), np.ones(Tn, bool)
    for p in perts:
        q = run_numpy(Y + p, n_fft, d, forget, adapt, angle)
        e_pert = np.maximum(e_pert, np.abs(q["h"] - r["h"]).max(axis=1))
        for t in range(Tn):
            same = q["bins"][t] == r["bins"][t]
            stable[t] &= same
            J = int(r["J"][t])
            if same and J:
                d_pert[t] = max(d_pert[t],
                                np.abs(q["lists"][t, 1:1 + J] - r["lists"][t, 1:1 + J]).max())
    r.update(Y=Y, perts=perts, e_pert=e_pert, d_pert=d_pert, stable=stable, angle=angle,
             n_fft=n_fft)
    return r


def reference(n_fft, d, s, forget=1.0, angle=90.0, adapt=None, key=None):
    """The restatement of stream s with its perturbation figures, computed once per `key`
    (required with adapt flags)."""
    assert adapt is None or key is not None
    k = (n_fft, d, s, forget, angle, key)
    if k not in _REF:
        _REF[k] = with_perturbations(spectra(n_fft, d, s), n_fft, d, 5100 + s, forget, adapt,
                                     angle)
    return _REF[k]


def labels_at(Y, lists, J, n_fft):
    """The restatement's stage 3, frame t with lists[t]: M [F, T] float32."""
    return np.concatenate([DM.delay_labels(Y[0][:, t:t + 1], Y[1][:, t:t + 1], lists[t],
                                           int(J[t]), n_fft) for t in range(Y.shape[2])], axis=1)


def stable_labels(ref, lists, J):
    """(M, stable): the restatement's labels at the given per-frame lists, and the decisions
    that none of the reference's perturbations flips at those lists."""
    M = labels_at(ref["Y"], lists, J, ref["n_fft"])
    stable = np.ones(M.shape, bool)
    for p in ref["perts"]:
        stable &= labels_at(ref["Y"] + p, lists, J, ref["n_fft"]) == M
    return M, stable


def hist_tolerance(ref, t):
    """4 E_pert(t) + 2^-20 max h_t."""
    return 4 * ref["e_pert"][t] + 2.0 ** -20 * ref["h"][t].max()


# ------------------------------------------------------------------ the end-to-end chain
E2E = dict(n_fft=1024, d=0.08, sigma=1e-5, pf_floor=0.05, bf_forget=0.99)


def chain_numpy(mix, Y, n_fft=1024, d=0.08, hist_forget=1.0, zero_mask=False, pert=None):
    """The restatement chain on a [2, T H] signal with frames Y [2, F, T + 1]:
    delay_mask_stream_numpy -> stream_numpy (external mask, floor post-filter, sigma 1e-5,
    beamformer forget 0.99), the one-hop delay trimmed. pert: a perturbation of Y for both
    stages. zero_mask: the all-zero mask instead (MPDR)."""
    H = n_fft // 2
    Yp = Y if pert is None else Y + pert
    M = DM.delay_mask_stream_numpy(Yp[0], Yp[1], n_fft, FS, d, C_SOUND, forget=hist_forget)[0]
    if zero_mask:
        M = np.zeros_like(M)
    x = np.concatenate([mix, np.zeros((2, H), mix.dtype)], axis=1)
    hook = None if pert is None else (lambda t, Yt: Yt + pert[:, :, t])
    out, _ = ST.stream_numpy(x, mask=M, drain=False, n_fft=n_fft, fs=FS, sigma=E2E["sigma"],
                             mic_d=d, c_sound=C_SOUND, mask_mode="external", postfilter="floor",
                             pf_floor=E2E["pf_floor"], forget=E2E["bf_forget"], y_hook=hook)
    return out[H:H + mix.shape[1]]


def e2e_reference():
    """The 4-s scene 0 (N = 1024, d = 0.08, SNR 20) through chain_numpy: dict(mix, tgt, itf,
    sir, sir_mpdr, spread), spread = the largest |SIR change| over the 8 perturbations."""
    if not _E2E:
        mix, tgt, itf = DC.long_scenes(20.0)[0]
        Y = DC.spectra(mix, 1024)
        sir = DC.sir_db(chain_numpy(mix, Y), tgt, itf)
        mpdr = DC.sir_db(chain_numpy(mix, Y, zero_mask=True), tgt, itf)
        spread = max(abs(DC.sir_db(chain_numpy(mix, Y, pert=p), tgt, itf) - sir)
                     for p in DC.perturbations(Y, 6100))
        _E2E.update(mix=mix, tgt=tgt, itf=itf, sir=sir, sir_mpdr=mpdr, spread=spread)
    return _E2E
