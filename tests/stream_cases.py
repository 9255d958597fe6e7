"""Shared inputs and fp64 references of the streaming tests (test_stream_reference.py,
test_gpu_stream.py).

Three streams per transform size N (hop H = N / 2): the items of train_cases.batches(N)["A"]
(whole-hop lengths 15 H, 14 H and 2 H; item 1 with an all-zero reference block, item 2 with a
zero interferer), zero-padded to HOPS = 17 hops, plus the drain hop of zeros: T = 18 pushed
hops = 18 frames. Eight frames fit one pass of the kernel, so 18 crosses two full groups and
leaves a ragged one. The external mask is a seeded uniform target probability [3, F, T].

reference() runs avz.stream.stream_numpy once per (size, configuration, forget, stream, ...)
and keeps the result; e_pert() is the restatement's largest change of an output over 8 seeded
perturbations of Y by 2e-6 max|Y| (|u| <= 1 per bin), the stage bound of test_stft_stage."""
import numpy as np

import train_cases as TC
from avz import stream as ST

SIZES = TC.SIZES
HOPS, T = 17, 18
STREAMS = 3
STAGE = 2e-6
GROUPINGS = {"one": [T], "single": [1] * T, "ragged": [3, 1, 8, 6]}

# plan options of the configurations under test (MVDRPlan keywords) and the same for NumpyStream
CONFIGS = {
    "floor": dict(sigma=1e-5, mic_d=0.04, mask="external", postfilter="floor", pf_floor=0.05),
    "none": dict(sigma=1e-7, mic_d=0.01, mask="external", postfilter="none"),
    "ibm": dict(sigma=1.0, mic_d=0.01, mask="ibm", postfilter="ibm"),
}


def numpy_cfg(name, n_fft, forget=1.0, **over):
    c = dict(CONFIGS[name])
    c["mask_mode"] = c.pop("mask")
    c.update(n_fft=n_fft, forget=forget, **over)
    return c


_IN, _REF = {}, {}


def inputs(n_fft):
    """(mix [3, 2, T H], tgt [3, T H], itf [3, T H]) float32: hops >= the item's length zero."""
    if n_fft not in _IN:
        H = n_fft // 2
        mix_h, tgt_h, itf_h, lens = TC.batches(n_fft)["A"]
        mix = np.zeros((STREAMS, 2, T * H), np.float32)
        tgt = np.zeros((STREAMS, T * H), np.float32)
        itf = np.zeros((STREAMS, T * H), np.float32)
        for b, L in enumerate(lens):
            assert L % H == 0 and L <= HOPS * H
            mix[b, :, :L], tgt[b, :L], itf[b, :L] = mix_h[b, :, :L], tgt_h[b, :L], itf_h[b, :L]
        _IN[n_fft] = (mix, tgt, itf)
    return _IN[n_fft]


def ext_mask(n_fft):
    """Target probability [3, F, T] float32, seeded uniform in [0, 1)."""
    rng = np.random.default_rng(7100 + n_fft)
    return rng.random((STREAMS, n_fft // 2 + 1, T)).astype(np.float32)


def run_numpy(n_fft, name, s, forget=1.0, noise=None, adapt=None, steer=None, y_hook=None,
              hops_per_push=None, **over):
    """stream_numpy of stream s over its T hops (the drain hop is the input's own last hop)."""
    mix, tgt, itf = inputs(n_fft)
    kw = {}
    if CONFIGS[name]["mask"] == "external":
        kw["mask"] = ext_mask(n_fft)[s]
    elif noise is None:
        kw.update(ref_tgt=tgt[s], ref_int=itf[s])
    else:
        kw["noise"] = noise
    return ST.stream_numpy(mix[s], drain=False, adapt=adapt, steer=steer,
                           hops_per_push=hops_per_push, y_hook=y_hook,
                           **kw, **numpy_cfg(name, n_fft, forget, **over))


def _w4(st):
    """The last weights as the kernel's w_out row layout [F, 4]."""
    w = st.w
    return np.stack([w[:, 0].real, w[:, 0].imag, w[:, 1].real, w[:, 1].imag], axis=-1)


def reference(n_fft, name, s, forget=1.0, key=None, **kw):
    """{'out', 'w' [F, 4], 'c' [F, 5], 'e_out', 'e_w'} of one stream, computed once per `key`
    (required whenever kw holds arrays)."""
    k = (n_fft, name, s, forget, key)
    assert key is not None or not kw
    if k not in _REF:
        out, st = run_numpy(n_fft, name, s, forget, **kw)
        ymax = max(np.abs(y).max() for y in st.hist["Y"])
        rng = np.random.default_rng(2024 + s)
        e_out = e_w = 0.0
        for _ in range(8):
            u = [rng.uniform(-1, 1, (2, n_fft // 2 + 1)) + 1j * rng.uniform(-1, 1, (2, n_fft // 2 + 1))
                 for _ in range(T)]
            u = [v / np.maximum(np.abs(v), 1.0) for v in u]
            o2, s2 = run_numpy(n_fft, name, s, forget,
                               y_hook=lambda t, Y: Y + STAGE * ymax * u[t], **kw)
            e_out = max(e_out, np.abs(o2 - out).max())
            e_w = max(e_w, np.abs(_w4(s2) - _w4(st)).max())
        _REF[k] = dict(out=out, w=_w4(st), c=st.c.copy(), e_out=e_out, e_w=e_w, stream=st)
    return _REF[k]


def tolerance(ref):
    """(tol_out, tol_w) = 4 E_pert + 2^-23 max|.|, the form test_gpu_wpe.py uses."""
    return (4 * ref["e_out"] + 2.0 ** -23 * np.abs(ref["out"]).max(),
            4 * ref["e_w"] + 2.0 ** -23 * np.abs(ref["w"]).max())
