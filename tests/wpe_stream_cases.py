"""Shared inputs and fp64 references of the streaming-WPE tests (test_wpe_stream_reference.py,
test_gpu_wpe_stream.py).

Three streams per transform size N (hop H = N / 2), cut from the bundled speech excerpt
(tests/golden/inputs_test.npz, two mics) and zero-padded to T pushed hops, the last of which
is always the drain hop of zeros:
  stream 0  T - 1 hops of speech;
  stream 1  two thirds of that, then digital silence;
  stream 2  five hops of digital silence first (the power floor decides lambda there), then
            speech up to hop T - 3.
Cases (taps K, delay D, forget, T): k2 (2, 1, 0.9, 18): the ring of K + D + 9 = 12 slots wraps
in 18 hops and the frame groups of eight end ragged; k10 (10, 3, 0.99, 48): the reference's
taps and delay, n = 20 rows is no power of two, ring of 22 slots wrapped twice; k16
(16, 3, 1.0, 48): n = 32, the lane-group limit, ring of 28. power_floor and q_init are the
defaults (avz.dereverb.default_power_floor, 1.0).

reference() runs avz.dereverb.wpe_stream_numpy on the raw samples once per (size, case,
stream, flags) and keeps the result; e_out / e_g are the restatement's largest change of the
time output / of G over 8 seeded perturbations of Y by STAGE max|Y| (|u| <= 1 per bin), the
bound of the analysis stage, exactly as stream_cases.reference. spectral_reference() runs the
restatement on given spectra in fp64 and in numpy.longdouble: E_ref per bin is their largest
difference (the form wpe_cases.py uses)."""
import numpy as np

from conftest import triple_f32
from avz import dereverb as DV

SIZES = (512, 1024)
STREAMS = 3
STAGE = 2e-6
CASES = {
    "k2": dict(taps=2, delay=1, forget=0.9, T=18),
    "k10": dict(taps=10, delay=3, forget=0.99, T=48),
    "k16": dict(taps=16, delay=3, forget=1.0, T=48),
}
_GROUPS = {18: {"one": [18], "single": [1] * 18, "ragged": [3, 1, 8, 6]},
           48: {"one": [48], "single": [1] * 48, "ragged": [5, 1, 17, 8, 9, 8]}}
_START = (40000, 52000, 64000)     # where each stream's speech starts in the excerpt

_IN, _REF = {}, {}


def groupings(case):
    return _GROUPS[CASES[case]["T"]]


def params(case):
    c = CASES[case]
    return dict(taps=c["taps"], delay=c["delay"], forget=c["forget"])


def inputs(n_fft, T):
    """mix [3, 2, T H] float32."""
    if (n_fft, T) not in _IN:
        H = n_fft // 2
        src = triple_f32("test")[0]                               # [2, L]
        mix = np.zeros((STREAMS, 2, T * H), np.float32)
        spans = ((0, T - 1), (0, 2 * (T - 1) // 3), (5, T - 3))   # active hops [a, b)
        for s, (a, b) in enumerate(spans):
            n = (b - a) * H
            assert _START[s] + n <= src.shape[1]
            mix[s, :, a * H:b * H] = src[:, _START[s]:_START[s] + n]
        _IN[n_fft, T] = mix
    return _IN[n_fft, T]


def run_numpy(n_fft, case, s, adapt=None, y_hook=None, hops_per_push=None, dtype=np.float64):
    mix = inputs(n_fft, CASES[case]["T"])
    return DV.wpe_stream_numpy(mix[s], n_fft=n_fft, adapt=adapt, y_hook=y_hook,
                               hops_per_push=hops_per_push, drain=False, dtype=dtype,
                               **params(case))


def reference(n_fft, case, s, key=None, **kw):
    """{'out' [2, T H], 'G' [F, n, 2], 'Y', 'Z' [2, F, T], 'e_out', 'e_g', 'ymax'} of one
    stream, computed once per `key` (required whenever kw holds arrays)."""
    k = (n_fft, case, s, key)
    assert key is not None or not kw
    if k not in _REF:
        T, F = CASES[case]["T"], n_fft // 2 + 1
        out, st = run_numpy(n_fft, case, s, **kw)
        Y = np.stack(st.hist["Y"], axis=-1)
        ymax = np.abs(Y).max()
        rng = np.random.default_rng(2024 + s)
        e_out = e_g = 0.0
        for _ in range(8):
            u = [rng.uniform(-1, 1, (2, F)) + 1j * rng.uniform(-1, 1, (2, F)) for _ in range(T)]
            u = [v / np.maximum(np.abs(v), 1.0) for v in u]
            o2, s2 = run_numpy(n_fft, case, s, y_hook=lambda t, Yt: Yt + STAGE * ymax * u[t],
                               **kw)
            e_out = max(e_out, np.abs(o2 - out).max())
            e_g = max(e_g, np.abs(s2.G - st.G).max())
        _REF[k] = dict(out=out, G=st.G.copy(), Q=st.Q.copy(), Y=Y,
                       Z=np.stack(st.hist["Z"], axis=-1), e_out=e_out, e_g=e_g, ymax=ymax)
    return _REF[k]


def tolerance(ref):
    """(tol_out, tol_G) = 4 E_pert + 2^-23 max|.|."""
    return (4 * ref["e_out"] + 2.0 ** -23 * np.abs(ref["out"]).max(),
            4 * ref["e_g"] + 2.0 ** -23 * np.abs(ref["G"]).max())


def spectral_reference(Y, n_fft, case, adapt=None):
    """Restatement on the spectra Y [2, F, T] (complex64): (Z [2, F, T] complex128, G,
    E_ref [F]) with E_ref,k = max |fp64 - longdouble| over the bin's Z."""
    _, st = DV.wpe_stream_numpy(Y, n_fft=n_fft, adapt=adapt, **params(case))
    _, sl = DV.wpe_stream_numpy(Y, n_fft=n_fft, adapt=adapt, dtype=np.longdouble, **params(case))
    Z = np.stack(st.hist["Z"], axis=-1)
    Zl = np.stack(sl.hist["Z"], axis=-1)
    e_ref = np.abs(Zl - Z).astype(np.float64).max(axis=(0, 2))
    return Z, st.G, e_ref


def spectral_tolerance(Z, e_ref):
    """Per bin [F]: 2^-23 max|Z_k| + 4 E_ref,k."""
    return 2.0 ** -23 * np.abs(Z).max(axis=(0, 2)) + 4 * e_ref
