"""Built covariances for the per-bin weight solves, with LAPACK and extended-precision
references (plain module shared by test_solve_reference.py and test_gpu_solve_edges.py).

The engine's ``mvdr_weights_d`` / ``hybrid_weights_d`` (csrc/avz_common.hpp) are closed-form
fp64 restatements of what the reference does with LAPACK (``np.linalg.solve``; ``eigh``,
``cond``, ``solve``). Here the two references work from covariance sums ``c[F][5]``
(sum m|y0|^2, sum m|y1|^2, Re / Im sum m y0 conj(y1), sum m: the cov_out layout) and the plan
parameters, in complex128, as ``mvdr_weights_loop`` / ``hybrid_weights_loop`` of
oracle/avz_oracle.py do from Y:

* ``mvdr_lapack`` / ``hybrid_lapack``: LAPACK, the reference's semantics (LinAlgError included).
* ``mvdr_truth`` / ``hybrid_truth``: the closed forms in ``np.longdouble`` (80-bit here; mpmath
  at 40 digits where long double is no wider than double), the "truth" that measures LAPACK's
  own error ``E_ref`` per family (``reference_error()``).

Case families fill all F bins of one batch item from fixed seeds; the sums are Gram sums of
complex64 "frames" cast to complex128 (then edited where a family pins an exact relation).
Every family is evaluated with the oracle's steering table and is meant to be run a second
time with ``steer=None`` (the plan's own table, equal to the oracle's to a few ulp).

Not pinned anywhere: random exactly-rank-1 bins at sigma = 0. There the closed-form
determinant a e - |b|^2 and LAPACK's second pivot e - conj(b) b / a round differently, so
they may disagree on "exactly singular" and the fallback; only the constructed S1 / S2
bins, singular in both whatever the rounding, are compared.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import avz_oracle as O

FS = 16000
N_FFTS = (512, 1024)
SIGMAS = (1.0, 1e-3, 1e-5, 1e-7)
SCALES = (1e-3, 1.0, 1e3)
MIC_D_MVDR = 0.04
MIC_D_HYBRID = 0.08
FMIN_M7 = 125.0
BYPASS_H6 = 250.0
BYPASS = 200.0
COND_MAX = 10.0
# the engine's avz_plan_create rejects cond_max < 1, so a plan forces the fallback branch with
# cond_max = 1 (cond_2 >= 1 always; test_solve_reference asserts cond_2 > 1 on every H1 bin,
# which makes 1 and -1 the same decision)
COND_FORCED = (1e300, -1.0)
H4_MARGIN = 1e-9
FRAMES = 8

LD = np.longdouble
CLD = np.clongdouble
HAVE_LD = bool(np.finfo(LD).eps < 2e-19)

# items per family in one (n_fft, parameter) group: fixed, nothing is dropped at run time
CASE_COUNTS = {"M1": 3, "M2": 6, "M3": 1, "M4": 1, "M5": 1, "M6": 1, "M7": 1,
               "S1": 1, "S2": 1, "S3": 1,
               "H1": 9, "H2": 3, "H3": 1, "H4": 2, "H5": 3, "H6": 1}


def bin_freqs(n_fft: int) -> np.ndarray:
    """k * fs / N: the engine's bin frequency, equal to scipy's f for N = 512 / 1024."""
    return np.arange(n_fft // 2 + 1, dtype=np.float64) * FS / n_fft


def steer_mvdr(n_fft: int) -> np.ndarray:
    return O.steering_vectors(bin_freqs(n_fft), O.ANGLE_TARGET, MIC_D_MVDR, O.C_SOUND)


def steer_hybrid(n_fft: int) -> np.ndarray:
    return np.stack([O.steering_vector_phase_norm(fk, O.ANGLE_TARGET, MIC_D_HYBRID, O.C_SOUND)[:, 0]
                     for fk in bin_freqs(n_fft)])


# ----------------------------------------------------------------------------
# references
# ----------------------------------------------------------------------------
def _R(c):
    nrm = c[:, 4] + 1e-6
    b = (c[:, 2] + 1j * c[:, 3]) / nrm
    R = np.empty((len(c), 2, 2), dtype=np.complex128)
    R[:, 0, 0] = c[:, 0] / nrm
    R[:, 0, 1] = b
    R[:, 1, 0] = b.conj()
    R[:, 1, 1] = c[:, 1] / nrm
    return R


def mvdr_lapack(c, f, sigma, steer, fmin, fallback="mic0"):
    """oracle_debug.py:66-79 from covariance sums: per bin solve(R/(c4 + 1e-6) + sigma I, d),
    w /= d^H w + 1e-10; LinAlgError -> [1, 0] (mic0) / [.5, .5] (mean); for "batch" any
    LinAlgError sends every bin of the item to [1 / (conj d0 + 1e-10), 0]
    (tf_lite_version/inference.py:139-163); bins with f < fmin are zero.
    Returns (W [F, 2] complex128, raised [F] bool)."""
    c = np.asarray(c, dtype=np.float64)
    F = len(c)
    Rl = _R(c) + sigma * np.eye(2)
    W = np.zeros((F, 2), dtype=np.complex128)
    raised = np.zeros(F, dtype=bool)
    live = np.nonzero(~(f < fmin))[0]
    with np.errstate(all="ignore"):
        try:  # one gesv per matrix either way; the stacked call raises if any bin does
            w = np.linalg.solve(Rl[live], steer[live][:, :, None])[:, :, 0]
            W[live] = w / ((steer[live].conj() * w).sum(axis=1) + 1e-10)[:, None]
        except np.linalg.LinAlgError:
            for k in live:
                dv = steer[k][:, None]
                try:
                    w = np.linalg.solve(Rl[k], dv)
                    w = w / (dv.conj().T @ w + 1e-10)
                    W[k] = w[:, 0]
                except np.linalg.LinAlgError:
                    raised[k] = True
                    W[k] = [0.5, 0.5] if fallback == "mean" else [1.0, 0.0]
    if fallback == "batch" and raised.any():
        W[:, 0] = 1.0 / (steer[:, 0].conj() + 1e-10)
        W[:, 1] = 0.0
    return W, raised


def hybrid_lapack(c, f, steer, bypass_hz=BYPASS, cond_max=COND_MAX):
    """Final_pipeline/src/inference.py:28-98 from covariance sums: per bin eigh, last column,
    v_int / (v_int[0] / (|v_int[0]| + 1e-10)), cond([v_tgt, v_int]) > cond_max -> v_tgt / 2,
    else solve(C^H, e1); f < bypass_hz -> [1, 0]. Where the reference itself raises (v_int[0]
    == 0: it divides by zero and cond's SVD fails) the bin is marked and carries v_tgt / 2,
    the engine's documented contract (avz_common.hpp, above hybrid_weights_d).
    Returns (W [F, 2], cond [F], raised [F])."""
    c = np.asarray(c, dtype=np.float64)
    F = len(c)
    R = _R(c)
    W = np.zeros((F, 2), dtype=np.complex128)
    cond = np.full(F, np.nan)
    raised = np.zeros(F, dtype=bool)
    W[f < bypass_hz] = [1.0, 0.0]
    live = np.nonzero(~(f < bypass_hz))[0]
    e1 = np.array([[1.0], [0.0]], dtype=np.complex128)

    def one(k):
        _, vecs = np.linalg.eigh(R[k])
        v_int = vecs[:, -1].reshape(2, 1)
        v_int = v_int / (v_int[0] / (np.abs(v_int[0]) + 1e-10))
        v_tgt = steer[k].reshape(2, 1)
        C = np.column_stack((v_tgt, v_int))
        cn = np.linalg.cond(C)
        if cn > cond_max:
            return v_tgt[:, 0] / 2, cn
        try:
            return np.linalg.solve(C.conj().T, e1)[:, 0], cn
        except np.linalg.LinAlgError:
            return v_tgt[:, 0] / 2, cn

    with np.errstate(all="ignore"):
        try:  # stacked LAPACK calls: the same routine per matrix as the loop
            _, vecs = np.linalg.eigh(R[live])
            v = vecs[:, :, -1]
            v = v / (v[:, :1] / (np.abs(v[:, :1]) + 1e-10))
            C = np.stack([steer[live], v], axis=2)
            if not np.isfinite(C).all():
                raise np.linalg.LinAlgError("non-finite C")
            cn = np.linalg.cond(C)
            w = np.linalg.solve(np.conj(np.swapaxes(C, 1, 2)), e1[None])[:, :, 0]
            W[live] = np.where((cn > cond_max)[:, None], steer[live] / 2, w)
            cond[live] = cn
        except np.linalg.LinAlgError:
            for k in live:
                try:
                    W[k], cond[k] = one(k)
                except np.linalg.LinAlgError:
                    raised[k] = True
                    cond[k] = np.inf
                    W[k] = steer[k] / 2
    return W, cond, raised


def mvdr_truth(c, f, sigma, steer, fmin):
    """The closed form of mvdr_weights_d in long double (singular bins -> NaN)."""
    if not HAVE_LD:
        return np.array([_mp_mvdr(c[k], sigma, steer[k]) if not f[k] < fmin else [0, 0]
                         for k in range(len(c))], dtype=np.complex128)
    c = np.asarray(c, dtype=np.float64).astype(LD)
    nrm = c[:, 4] + LD(1e-6)
    a = c[:, 0] / nrm + LD(sigma)
    e = c[:, 1] / nrm + LD(sigma)
    b = (c[:, 2] + CLD(1j) * c[:, 3]) / nrm
    d0, d1 = steer[:, 0].astype(CLD), steer[:, 1].astype(CLD)
    det = a * e - (b.real * b.real + b.imag * b.imag)
    with np.errstate(all="ignore"):
        t0 = (e * d0 - b * d1) / det
        t1 = (a * d1 - np.conj(b) * d0) / det
        den = np.conj(d0) * t0 + np.conj(d1) * t1 + LD(1e-10)
        W = np.stack([t0 / den, t1 / den], axis=1)
    W[det == 0] = np.nan
    W[f < fmin] = 0
    return W


def hybrid_truth(c, f, steer, bypass_hz=BYPASS, cond_max=COND_MAX):
    """The closed form of hybrid_weights_d in long double: (W [F, 2], cond [F]); cond is inf
    where the eigenvector has v[0] == 0 (delay-and-sum contract)."""
    if not HAVE_LD:
        r = [_mp_hybrid(c[k], steer[k], cond_max) for k in range(len(c))]
        W = np.array([x[0] for x in r], dtype=np.complex128)
        cond = np.array([x[1] for x in r], dtype=np.float64)
        W[f < bypass_hz] = [1.0, 0.0]
        return W, cond
    c = np.asarray(c, dtype=np.float64).astype(LD)
    nrm = c[:, 4] + LD(1e-6)
    a, e = c[:, 0] / nrm, c[:, 1] / nrm
    b = (c[:, 2] + CLD(1j) * c[:, 3]) / nrm
    t0, t1 = steer[:, 0].astype(CLD), steer[:, 1].astype(CLD)
    with np.errstate(all="ignore"):
        hd = (a - e) / 2
        lam = (a + e) / 2 + np.sqrt(hd * hd + b.real * b.real + b.imag * b.imag)
        ge = a >= e
        u0 = np.where(ge, (lam - e).astype(CLD), b)
        u1 = np.where(ge, np.conj(b), (lam - a).astype(CLD))
        un = np.sqrt(np.abs(u0) ** 2 + np.abs(u1) ** 2)
        u0, u1 = u0 / un, u1 / un
        a0 = np.abs(u0)
        v0 = (a0 + LD(1e-10)).astype(CLD)
        v1 = u1 * np.conj(u0) * (a0 + LD(1e-10)) / (a0 * a0)
        det = t0 * v1 - v0 * t1
        p = np.abs(t0) ** 2 + np.abs(t1) ** 2
        q = np.abs(v0) ** 2 + np.abs(v1) ** 2
        r = np.conj(t0) * v0 + np.conj(t1) * v1
        smax2 = (p + q) / 2 + np.sqrt(((p - q) / 2) ** 2 + np.abs(r) ** 2)
        ok = np.isfinite(v1.real) & np.isfinite(v1.imag) & (a0 > 0) & (np.abs(det) > 0)
        cond = np.where(ok, smax2 / np.abs(det), LD(np.inf))
        solve = ok & (cond <= LD(cond_max))
        W = np.where(solve[:, None], np.stack([np.conj(v1), -np.conj(v0)], axis=1)
                     / np.conj(det)[:, None], np.stack([t0, t1], axis=1) / 2)
    W[f < bypass_hz] = [1.0, 0.0]
    return W, cond


# ---- mpmath restatements (spot checks; the truth itself without an 80-bit long double)
def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def _mp_mvdr(c, sigma, d):
    mp = _mp()
    c = [mp.mpf(float(x)) for x in c]
    nrm = c[4] + mp.mpf(1e-6)
    a, e = c[0] / nrm + mp.mpf(float(sigma)), c[1] / nrm + mp.mpf(float(sigma))
    b = mp.mpc(c[2], c[3]) / nrm
    d0, d1 = mp.mpc(complex(d[0])), mp.mpc(complex(d[1]))
    det = a * e - abs(b) ** 2
    t0 = (e * d0 - b * d1) / det
    t1 = (a * d1 - mp.conj(b) * d0) / det
    den = mp.conj(d0) * t0 + mp.conj(d1) * t1 + mp.mpf(1e-10)
    return [t0 / den, t1 / den]


def _mp_hybrid(c, t, cond_max):
    """(w, cond) of one live bin in mpmath (inf cond: delay-and-sum contract)."""
    mp = _mp()
    c = [mp.mpf(float(x)) for x in c]
    nrm = c[4] + mp.mpf(1e-6)
    a, e = c[0] / nrm, c[1] / nrm
    b = mp.mpc(c[2], c[3]) / nrm
    t0, t1 = mp.mpc(complex(t[0])), mp.mpc(complex(t[1]))
    hd = (a - e) / 2
    lam = (a + e) / 2 + mp.sqrt(hd * hd + abs(b) ** 2)
    u0, u1 = (lam - e, mp.conj(b)) if a >= e else (b, lam - a)
    un = mp.sqrt(abs(u0) ** 2 + abs(u1) ** 2)
    if un == 0 or abs(u0) == 0:
        return [t0 / 2, t1 / 2], mp.inf
    u0, u1 = u0 / un, u1 / un
    a0 = abs(u0)
    v0 = a0 + mp.mpf(1e-10)
    v1 = u1 * mp.conj(u0) * v0 / (a0 * a0)
    det = t0 * v1 - v0 * t1
    p = abs(t0) ** 2 + abs(t1) ** 2
    q = abs(v0) ** 2 + abs(v1) ** 2
    r = mp.conj(t0) * v0 + mp.conj(t1) * v1
    smax2 = (p + q) / 2 + mp.sqrt(((p - q) / 2) ** 2 + abs(r) ** 2)
    if abs(det) == 0:
        return [t0 / 2, t1 / 2], mp.inf
    cond = smax2 / abs(det)
    if cond > mp.mpf(float(cond_max)):
        return [t0 / 2, t1 / 2], cond
    return [mp.conj(v1) / mp.conj(det), -mp.conj(v0) / mp.conj(det)], cond


def _mpf_of(x):
    """A long double as an mpf, exactly (two doubles)."""
    mp = _mp()
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


def mp_distance(case, bins):
    """max over ``bins`` of |w_truth - w_mpmath|_inf / |w_mpmath|_inf for one case."""
    mp = _mp()
    worst = 0.0
    Wt = case.truth
    for k in bins:
        if case.beamformer == "mvdr":
            w = _mp_mvdr(case.cov[k], case.sigma, case.steer[k])
        else:
            w, _ = _mp_hybrid(case.cov[k], case.steer[k], case.cond_max)
        got = [mp.mpc(_mpf_of(Wt[k, j].real), _mpf_of(Wt[k, j].imag)) for j in range(2)]
        num = max(max(abs((g - x).real), abs((g - x).imag)) for g, x in zip(got, w))
        den = max(max(abs(x.real), abs(x.imag)) for x in w)
        worst = max(worst, float(num / den))
    return worst


# ----------------------------------------------------------------------------
# case construction
# ----------------------------------------------------------------------------
def _cnormal(rng, shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _frames(rng, F, T, coh, scale, gain=None):
    """Interferer (s, s ph) plus white noise sized for a coherence ``coh``, as complex64
    frames cast to complex128: ph = e^{j phi} (MVDR) or gain e^{j phi} (hybrid)."""
    s = _cnormal(rng, (F, T))
    phi = rng.uniform(-np.pi, np.pi, F)
    ph = np.exp(1j * phi) * (1.0 if gain is None else gain)
    g = np.sqrt(1.0 / coh - 1.0)
    y0 = (s + g * _cnormal(rng, (F, T))) * scale
    y1 = (s * ph[:, None] + g * _cnormal(rng, (F, T))) * scale
    return y0.astype(np.complex64).astype(np.complex128), y1.astype(np.complex64).astype(np.complex128)


def gram(y0, y1, m=None):
    """Covariance sums [F, 5] (fp64) of frames y0 / y1 [F, T] with weights m [F, T]."""
    m = np.ones(y0.shape) if m is None else m
    b = (m * y0 * y1.conj()).sum(axis=1)
    return np.stack([(m * np.abs(y0) ** 2).sum(axis=1), (m * np.abs(y1) ** 2).sum(axis=1),
                     b.real, b.imag, m.sum(axis=1)], axis=1)


@dataclass
class Case:
    family: str
    label: str
    beamformer: str           # "mvdr" | "hybrid"
    n_fft: int
    cov: np.ndarray           # [F, 5] float64
    sigma: float = 0.0
    fmin: float = 0.0
    bypass_hz: float = BYPASS
    cond_max: float = COND_MAX
    steer: np.ndarray = field(default=None, repr=False)
    lapack: np.ndarray = field(default=None, repr=False)   # [F, 2] complex128
    truth: np.ndarray = field(default=None, repr=False)    # [F, 2] clongdouble
    cond: np.ndarray = field(default=None, repr=False)     # hybrid: LAPACK cond_2
    cond_truth: np.ndarray = field(default=None, repr=False)
    raised: np.ndarray = field(default=None, repr=False)

    @property
    def f(self):
        return bin_freqs(self.n_fft)

    @property
    def live(self):
        """Bins the solve reaches (at or above fmin_hz / bypass_hz)."""
        return ~(self.f < (self.fmin if self.beamformer == "mvdr" else self.bypass_hz))


def _seed(*k):
    return np.random.default_rng([20240607, *k])


def _mvdr_items(n_fft, sigma_i):
    """M1 .. M6 of one (n_fft, sigma) group: 13 items (family, label, cov)."""
    F = n_fft // 2 + 1
    items = []
    for si, sc in enumerate(SCALES):
        items.append(("M1", f"coh0.5 x{sc:g}", gram(*_frames(_seed(1, n_fft, sigma_i, si), F, FRAMES, 0.5, sc))))
    for ci, coh in enumerate((0.999, 1.0)):
        for si, sc in enumerate(SCALES):
            items.append(("M2", f"coh{coh:g} x{sc:g}",
                          gram(*_frames(_seed(2, n_fft, sigma_i, ci, si), F, FRAMES, coh, sc))))
    items.append(("M3", "one frame", gram(*_frames(_seed(3, n_fft, sigma_i), F, 1, 0.5, 1.0))))
    c = gram(*_frames(_seed(4, n_fft, sigma_i), F, FRAMES, 0.5, 1.0))
    c[:, :4] *= 1e-10
    c[:, 4] = 0.0
    items.append(("M4", "count 0, weight_eps sums", c))
    rng = _seed(5, n_fft, sigma_i)
    y0, y1 = _frames(rng, F, FRAMES, 0.5, 1.0)
    items.append(("M5", "fractional count", gram(y0, y1, rng.uniform(0.0, 1.0, y0.shape))))
    items.append(("M6", "all sums zero", np.zeros((F, 5))))
    return items


def _hybrid_items(n_fft):
    """H1 (9 items) of one n_fft, also reused under the forced cond_max values."""
    F = n_fft // 2 + 1
    items = []
    for ci, coh in enumerate((0.3, 0.9, 1.0)):
        for si, sc in enumerate(SCALES):
            rng = _seed(11, n_fft, ci, si)
            gain = np.exp(rng.uniform(np.log(0.2), np.log(3.0), F))
            y0, y1 = _frames(rng, F, FRAMES, coh, sc, gain=gain)
            items.append(("H1", f"coh{coh:g} x{sc:g}", gram(y0, y1)))
    return items


def _h2_items(n_fft):
    """a == e exactly with b != 0: every frame has |y1| == |y0| bit for bit (y1 is j y0,
    conj y0, -y0 or y0 with its parts swapped), so both power sums add the same doubles in the
    same order; then c0 one ulp above / below c1."""
    F = n_fft // 2 + 1
    rng = _seed(12, n_fft)
    y0, _ = _frames(rng, F, FRAMES, 0.5, 1.0)
    op = rng.integers(0, 4, y0.shape)
    y1 = np.select([op == 0, op == 1, op == 2], [1j * y0, y0.conj(), -y0], y0.imag + 1j * y0.real)
    c = gram(y0, y1)
    c[:, 1] = c[:, 0]
    assert (np.hypot(c[:, 2], c[:, 3]) > 0).all()
    up, dn = c.copy(), c.copy()
    up[:, 0] = np.nextafter(c[:, 1], np.inf)
    dn[:, 0] = np.nextafter(c[:, 1], 0.0)
    return [("H2", "a == e", c), ("H2", "a = e (1 + 2^-52)", up), ("H2", "a = e (1 - 2^-52)", dn)]


def _h3_item(n_fft):
    F = n_fft // 2 + 1
    c = gram(*_frames(_seed(13, n_fft), F, FRAMES, 0.5, 1.0))
    hi, lo = np.maximum(c[:, 0], c[:, 1]), np.minimum(c[:, 0], c[:, 1])
    assert (hi > lo).all()
    c[:, 0], c[:, 1], c[:, 2], c[:, 3] = hi, lo, 0.0, 0.0
    return [("H3", "b == 0, a > e", c)]


def _h5_items(n_fft):
    F = n_fft // 2 + 1
    c = _h3_item(n_fft)[0][2].copy()
    c[:, [0, 1]] = c[:, [1, 0]]                       # b == 0, a < e
    eq = c.copy()
    eq[:, 0] = eq[:, 1]                               # a == e, b == 0
    return [("H5", "b == 0, a < e", c), ("H5", "all sums zero", np.zeros((F, 5))),
            ("H5", "a == e, b == 0", eq)]


def _h4_items(n_fft, steer, bypass_hz=BYPASS, cond_max=COND_MAX):
    """Threshold bins: R = v v^H, v = [1, r e^{j phi}] with phi close to the target's
    inter-mic phase, r found by bisection on the long-double cond_2 so that cond_2 =
    cond_max (1 -/+ 1e-9): one item just below the threshold (solve) and one just above
    (delay-and-sum), in every bin at or above bypass_hz."""
    F = n_fft // 2 + 1
    f = bin_freqs(n_fft)
    rng = _seed(14, n_fft)
    phi = np.angle(steer[:, 1] / steer[:, 0]) + rng.uniform(0.01, 0.05, F) * rng.choice([-1.0, 1.0], F)

    def cov_of(r):
        c = np.zeros((F, 5))
        c[:, 0], c[:, 1] = 1.0, r * r
        b = r * np.exp(-1j * phi)                     # v0 conj(v1)
        c[:, 2], c[:, 3], c[:, 4] = b.real, b.imag, 1.0
        return c

    out = []
    for side, lab in ((-1.0, "below"), (1.0, "above")):
        target = LD(cond_max) * (LD(1.0) + LD(side * H4_MARGIN))
        lo, hi = np.full(F, 0.01), np.ones(F)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            up = hybrid_truth(cov_of(mid), f, steer, 0.0, cond_max)[1] > target
            hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
        # lo: cond <= target, hi: cond > target, adjacent doubles; keep the side asked for
        live = ~(f < bypass_hz)
        c_lo = hybrid_truth(cov_of(lo), f, steer, 0.0, cond_max)[1][live]
        c_hi = hybrid_truth(cov_of(hi), f, steer, 0.0, cond_max)[1][live]
        assert (c_lo <= target).all() and (c_hi > target).all()
        assert float(np.abs(c_hi / target - 1).max()) < 1e-11
        out.append(("H4", f"cond {lab} cond_max", cov_of(lo if side < 0 else hi)))
    return out


@dataclass
class Group:
    """The items one plan solves in one call."""
    beamformer: str
    n_fft: int
    params: dict              # plan keywords: sigma, fmin_hz | bypass_hz, cond_max
    cases: list
    tag: str

    @property
    def cov(self):
        return np.stack([cs.cov for cs in self.cases])


def _finish_mvdr(family, label, n_fft, cov, sigma, fmin):
    cs = Case(family, label, "mvdr", n_fft, cov, sigma=sigma, fmin=fmin, steer=steer_mvdr(n_fft))
    cs.lapack, cs.raised = mvdr_lapack(cov, cs.f, sigma, cs.steer, fmin)
    cs.truth = mvdr_truth(cov, cs.f, sigma, cs.steer, fmin)
    return cs


def _finish_hybrid(family, label, n_fft, cov, bypass_hz=BYPASS, cond_max=COND_MAX):
    cs = Case(family, label, "hybrid", n_fft, cov, bypass_hz=bypass_hz, cond_max=cond_max,
              steer=steer_hybrid(n_fft))
    cs.lapack, cs.cond, cs.raised = hybrid_lapack(cov, cs.f, cs.steer, bypass_hz, cond_max)
    cs.truth, cs.cond_truth = hybrid_truth(cov, cs.f, cs.steer, bypass_hz, cond_max)
    return cs


def _check_counts(cases, families):
    for fam in families:
        n = sum(cs.family == fam for cs in cases)
        assert n == CASE_COUNTS[fam], (fam, n)


@functools.lru_cache(maxsize=None)
def mvdr_groups():
    """Per (n_fft, sigma): M1 .. M6 (fmin_hz 0, 13 items) and M7 (fmin_hz 125, 1 item)."""
    out = []
    for n_fft in N_FFTS:
        F = n_fft // 2 + 1
        for si, sigma in enumerate(SIGMAS):
            cases = [_finish_mvdr(fam, lab, n_fft, cov, sigma, 0.0)
                     for fam, lab, cov in _mvdr_items(n_fft, si)]
            _check_counts(cases, ("M1", "M2", "M3", "M4", "M5", "M6"))
            out.append(Group("mvdr", n_fft, dict(sigma=sigma, fmin_hz=0.0), cases,
                             f"N{n_fft}-sigma{sigma:g}"))
            c7 = gram(*_frames(_seed(7, n_fft, si), F, FRAMES, 0.5, 1.0))
            m7 = [_finish_mvdr("M7", "fmin_hz on a bin", n_fft, c7, sigma, FMIN_M7)]
            _check_counts(m7, ("M7",))
            out.append(Group("mvdr", n_fft, dict(sigma=sigma, fmin_hz=FMIN_M7), m7,
                             f"N{n_fft}-sigma{sigma:g}-fmin"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def singular_covs(n_fft):
    """S1 all sums zero, S2 c = [x, x, x, 0, T] per bin, S3 an M1 control: [3, F, 5].

    S2: the three normalised entries are the same double v, so the closed-form determinant
    v v - (v v + 0) is exactly 0 for every x. LAPACK's multiplier is v * fl(1 / v), which is
    exactly 1 (second pivot exactly 0, LinAlgError) for most but not all doubles v, so x is
    drawn per bin among seeded candidates until the reference's own solve raises: the case is
    "singular for LAPACK" by construction, on whatever LAPACK build runs the tests."""
    F = n_fft // 2 + 1
    rng = _seed(21, n_fft)
    cand = rng.uniform(0.5, 2.0, (F, 32)) * FRAMES
    x = np.empty(F)
    rhs = np.ones((2, 1), dtype=np.complex128)
    for k in range(F):
        rows = np.zeros((cand.shape[1], 5))
        rows[:, :3], rows[:, 4] = cand[k][:, None], float(FRAMES)
        for xc, Rk in zip(cand[k], _R(rows)):     # the matrix exactly as mvdr_lapack builds it
            try:
                np.linalg.solve(Rk, rhs)
            except np.linalg.LinAlgError:
                x[k] = xc
                break
        else:
            raise AssertionError(f"S2: no LAPACK-singular candidate in bin {k}")
    s2 = np.stack([x, x, x, np.zeros(F), np.full(F, float(FRAMES))], axis=1)
    s3 = gram(*_frames(rng, F, FRAMES, 0.5, 1.0))
    return np.stack([np.zeros((F, 5)), s2, s3])


SINGULAR_FMIN = 100.0


def singular_expected(n_fft, fallback):
    """LAPACK weights [3, F, 2], raised [3, F] and the BATCH flags of the singular group
    (sigma = 0, fmin_hz = 100)."""
    cov = singular_covs(n_fft)
    f, st = bin_freqs(n_fft), steer_mvdr(n_fft)
    res = [mvdr_lapack(cov[b], f, 0.0, st, SINGULAR_FMIN, fallback) for b in range(3)]
    W = np.stack([r[0] for r in res])
    raised = np.stack([r[1] for r in res])
    return W, raised, [int(r.any()) for r in raised]


@functools.lru_cache(maxsize=None)
def hybrid_groups():
    """Per n_fft: H1 .. H5 at cond_max 10 (18 items), H1 under each forced cond_max (9 items
    each), H6 with bypass_hz on a bin (1 item)."""
    out = []
    for n_fft in N_FFTS:
        st = steer_hybrid(n_fft)
        h1 = _hybrid_items(n_fft)
        items = h1 + _h2_items(n_fft) + _h3_item(n_fft) + _h4_items(n_fft, st) + _h5_items(n_fft)
        cases = [_finish_hybrid(fam, lab, n_fft, cov) for fam, lab, cov in items]
        _check_counts(cases, ("H1", "H2", "H3", "H4", "H5"))
        out.append(Group("hybrid", n_fft, dict(bypass_hz=BYPASS, cond_max=COND_MAX), cases,
                         f"N{n_fft}"))
        for cm in COND_FORCED:
            forced = [_finish_hybrid(fam, lab, n_fft, cov, cond_max=cm) for fam, lab, cov in h1]
            _check_counts(forced, ("H1",))
            out.append(Group("hybrid", n_fft, dict(bypass_hz=BYPASS, cond_max=cm), forced,
                             f"N{n_fft}-cond_max{cm:g}"))
        rng = _seed(16, n_fft)
        F = n_fft // 2 + 1
        gain = np.exp(rng.uniform(np.log(0.2), np.log(3.0), F))
        c6 = gram(*_frames(rng, F, FRAMES, 0.9, 1.0, gain=gain))
        h6 = [_finish_hybrid("H6", "bypass_hz on a bin", n_fft, c6, bypass_hz=BYPASS_H6)]
        _check_counts(h6, ("H6",))
        out.append(Group("hybrid", n_fft, dict(bypass_hz=BYPASS_H6, cond_max=COND_MAX), h6,
                         f"N{n_fft}-bypass"))
    return tuple(out)


def case_error(cs):
    """E_ref of one case: max over solved bins of |w_lapack - w_truth|_inf / |w_truth|_inf."""
    k = cs.live & ~cs.raised
    if not k.any():
        return 0.0
    num = np.abs(cs.lapack[k].astype(CLD) - cs.truth[k]).max(axis=1)
    den = np.maximum(np.abs(cs.truth[k]).max(axis=1), LD(1e-300))
    return float((num / den).max())


@functools.lru_cache(maxsize=None)
def reference_error():
    """Per family, LAPACK's worst distance from the long-double value over every case of the
    family (both n_fft, every sigma / cond_max): the reference's own fp64 error."""
    E = {}
    for g in mvdr_groups() + hybrid_groups():
        for cs in g.cases:
            E[cs.family] = max(E.get(cs.family, 0.0), case_error(cs))
    return E
