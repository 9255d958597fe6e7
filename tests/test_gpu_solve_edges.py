"""The per-bin weight solves (mvdr_weights_d / hybrid_weights_d, csrc/avz_common.hpp) against
LAPACK on covariances built to hit their branches (tests/solve_cases.py), through every kernel
that calls them:

(a) the stage export avz_solve_covariance (avz_solve_cov_kernel) on the case families;
(b) avz_beamform_spectral in both layouts (avz_spectral_rows_kernel up to 64 frames,
    avz_spectral_kernel beyond), its covariance read back and compared with an fp64 sum;
(c) the fused chain (avz_solve_kernel / avz_solve_lanes_kernel / the per-utterance synthesis
    kernels' own solves) against the stage export of its own cov_out, bitwise, and LAPACK.

Weight bound, per bin, against w_lapack of the same covariance sums:

    |w_gpu - w_lapack|_inf <= 2^-23 |w_lapack|_inf + 4 E_ref |w_lapack|_inf

2^-23: each component is one fp32 rounding (<= 2^-24 per real part) of an fp64 value. E_ref:
LAPACK's own distance from the long-double value on that family
(solve_cases.reference_error()), x 4 because the kernel and LAPACK are two fp64 orderings of
the same ill-conditioned solve. Zero bins, bypass bins, the singular fallbacks and the BATCH
flags are compared with ==; the cond_2 branch has no tolerance (threshold bins are built
1e-9 from cond_max, LAPACK and the closed form agree on cond_2 to ~1e-14).

Not pinned: random exactly-rank-1 bins at sigma = 0 (LAPACK and the closed form may disagree
on exact singularity) and NaN into the hybrid solve (the reference raises).

Measured on an MI355X: the worst error of any family is 1.00 in units of 2^-24 |w|_inf (on
the complex modulus), i.e. the fp32 rounding alone; the 124 cases run in 3.6 s.

These cases found one kernel bug: with the determinant a e - |b|^2 contracted into an fma the
equal-entry matrices of S2 (two identical channels at sigma = 0) were not singular for the
kernel (its determinant was the rounding residue of a^2): BATCH flags [1, 0, 0] where LAPACK
raises in every bin of S2, and no [1, 0] / [.5, .5] fallback (herm_det_d, avz_common.hpp).
"""
import numpy as np
import pytest
import torch

import solve_cases as C
from conftest import triple_f32
from oracle import avz_oracle as O

pytestmark = pytest.mark.gpu

U23 = 2.0 ** -23


def dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def to_c(w):
    """[..., 4] float32 device weights -> [..., 2] complex128."""
    w = w.cpu().numpy().astype(np.float64)
    return w[..., 0::2] + 1j * w[..., 1::2]


def weight_excess(Wg, Wl, E):
    """Per bin: |w_gpu - w_lapack|_inf / |w_lapack|_inf and the bound it must meet."""
    ref = np.abs(Wl).max(axis=-1)
    err = np.abs(Wg - Wl).max(axis=-1)
    return err, (U23 + 4.0 * E) * ref, ref


def assert_weights(Wg, Wl, E, what, bins=None):
    bins = np.ones(len(Wl), dtype=bool) if bins is None else bins
    err, bound, ref = weight_excess(Wg[bins], Wl[bins], E)
    assert np.isfinite(Wg[bins]).all(), what
    worst = float((err / np.maximum(ref, 1e-300)).max() / 2.0 ** -24) if len(err) else 0.0
    bad = np.nonzero(~(err <= bound))[0]
    assert len(bad) == 0, (what, len(bad), np.nonzero(bins)[0][bad][:8], err[bad][:4], bound[bad][:4])
    return worst


def steer_arg(st, which, dev):
    return dev_t(st.astype(np.complex128), dev) if which == "oracle" else None


# ----------------------------------------------------------------------------
# (a) stage export
# ----------------------------------------------------------------------------
MVDR_GROUPS = {g.tag: g for g in C.mvdr_groups()}
HYBRID_GROUPS = {g.tag: g for g in C.hybrid_groups()}


@pytest.mark.parametrize("steer", ["oracle", "plan"])
@pytest.mark.parametrize("tag", list(MVDR_GROUPS))
def test_mvdr_solve_covariance_vs_lapack(gpu_device, tag, steer):
    import avz
    g = MVDR_GROUPS[tag]
    E = C.reference_error()
    plan = avz.MVDRPlan(n_fft=g.n_fft, mic_d=C.MIC_D_MVDR, mask="external", postfilter="none",
                        normalize="none", max_batch=len(g.cases), max_samples=g.n_fft, **g.params)
    w = plan.solve_covariance(dev_t(g.cov, gpu_device),
                              steer=steer_arg(C.steer_mvdr(g.n_fft), steer, gpu_device))
    Wg = to_c(w)
    worst = {}
    for b, cs in enumerate(g.cases):
        assert (Wg[b][~cs.live] == 0).all(), (tag, cs.family)       # below fmin_hz: exactly 0
        u = assert_weights(Wg[b], cs.lapack, E[cs.family], (tag, cs.family, cs.label), cs.live)
        worst[cs.family] = max(worst.get(cs.family, 0.0), u)
    print(f"mvdr {tag} steer={steer}: worst error in 2^-24 |w|: "
          + ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("steer", ["oracle", "plan"])
@pytest.mark.parametrize("tag", list(HYBRID_GROUPS))
def test_hybrid_solve_covariance_vs_lapack(gpu_device, tag, steer):
    import avz
    g = HYBRID_GROUPS[tag]
    E = C.reference_error()
    # avz_plan_create rejects cond_max < 1; 1 forces the same branch as -1 (cond_2 > 1 on
    # every H1 bin, asserted in test_solve_reference)
    plan = avz.MVDRPlan(n_fft=g.n_fft, mic_d=C.MIC_D_HYBRID, mask="external", postfilter="none",
                        beamformer="hybrid_null", normalize="none", max_batch=len(g.cases),
                        max_samples=g.n_fft, bypass_hz=g.params["bypass_hz"],
                        cond_max=max(g.params["cond_max"], 1.0))
    w = plan.solve_covariance(dev_t(g.cov, gpu_device),
                              steer=steer_arg(C.steer_hybrid(g.n_fft), steer, gpu_device))
    Wg = to_c(w)
    worst = {}
    for b, cs in enumerate(g.cases):
        assert (Wg[b][~cs.live] == [1.0, 0.0]).all(), (tag, cs.family)   # bypass: exactly [1, 0]
        # the branch carries no tolerance: cs.lapack is the solve where LAPACK's cond_2 <=
        # cond_max and v_tgt / 2 where it is above (H4: 1e-9 to either side, every bin)
        u = assert_weights(Wg[b], cs.lapack, E[cs.family], (tag, cs.family, cs.label), cs.live)
        worst[cs.family] = max(worst.get(cs.family, 0.0), u)
    h4 = [cs for cs in g.cases if cs.family == "H4"]
    if h4:  # the two sides are far apart, so matching one excludes the other
        k = h4[0].live
        gap = np.abs(h4[0].lapack[k] - h4[1].lapack[k]).max(axis=1)
        assert (gap > 1e-2).all()
        assert (np.abs(h4[1].lapack[k] - h4[1].steer[k] / 2) == 0).all()
    print(f"hybrid {tag} steer={steer}: worst error in 2^-24 |w|: "
          + ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("steer", ["oracle", "plan"])
@pytest.mark.parametrize("fallback", ["mic0", "mean", "batch"])
@pytest.mark.parametrize("n_fft", C.N_FFTS)
def test_singular_fallbacks_per_item(gpu_device, n_fft, fallback, steer):
    """sigma = 0: S1 (all sums zero) and S2 (c = [x, x, x, 0, T]) are singular in every bin for
    LAPACK and the closed form alike, S3 is an M1 control in the same call."""
    import avz
    cov = C.singular_covs(n_fft)
    Wl, raised, flags_ref = C.singular_expected(n_fft, fallback)
    live = ~(C.bin_freqs(n_fft) < C.SINGULAR_FMIN)
    plan = avz.MVDRPlan(n_fft=n_fft, sigma=0.0, mic_d=C.MIC_D_MVDR, fmin_hz=C.SINGULAR_FMIN,
                        mask="external", postfilter="none", normalize="none", max_batch=3,
                        max_samples=n_fft, singular_fallback=fallback)
    flags = torch.full((3,), 7, dtype=torch.int32, device=gpu_device)
    w = plan.solve_covariance(dev_t(cov, gpu_device), fallback=flags,
                              steer=steer_arg(C.steer_mvdr(n_fft), steer, gpu_device))
    Wg = to_c(w)
    E = C.reference_error()["M1"]
    if fallback == "batch":
        assert flags.tolist() == flags_ref == [1, 1, 0]
        for b in (0, 1):  # every bin of the item, the bins below fmin_hz included
            assert (Wg[b][:, 1] == 0).all()
            assert_weights(Wg[b][:, :1], Wl[b][:, :1], 0.0, (n_fft, "batch", b))
    else:
        assert flags.tolist() == [7, 7, 7]     # only the BATCH policy reports
        for b in (0, 1):
            assert np.array_equal(Wg[b], Wl[b].astype(np.complex64).astype(np.complex128))
            assert (Wg[b][live] == ([0.5, 0.5] if fallback == "mean" else [1.0, 0.0])).all()
            assert (Wg[b][~live] == 0).all()
    assert (Wg[2][~live] == 0).all()
    assert_weights(Wg[2], Wl[2], E, (n_fft, fallback, "S3"), live)


@pytest.mark.parametrize("fallback", ["mic0", "mean"])
def test_nan_sum_stays_in_its_bin(gpu_device, fallback):
    """One NaN covariance sum gives NaN weights in that bin and leaves every other bin's bits."""
    import avz
    g = MVDR_GROUPS["N512-sigma0.001"]
    cov = g.cov[:3].copy()
    plan = avz.MVDRPlan(n_fft=512, mic_d=C.MIC_D_MVDR, mask="external", postfilter="none",
                        normalize="none", max_batch=3, max_samples=512,
                        singular_fallback=fallback, **g.params)
    clean = plan.solve_covariance(dev_t(cov, gpu_device)).cpu().numpy()
    for q, k in ((2, 77), (0, 0), (4, 256)):
        bad = cov.copy()
        bad[1, k, q] = np.nan
        w = plan.solve_covariance(dev_t(bad, gpu_device)).cpu().numpy()
        assert np.isnan(w[1, k]).all()
        w[1, k] = clean[1, k]
        assert np.array_equal(w, clean)


# ----------------------------------------------------------------------------
# (b) spectral kernels, both layouts
# ----------------------------------------------------------------------------
PF_FLOOR = 0.05
SPEC_SIGMA = 1e-5


def spectral_inputs(n_fft, T, B=2):
    """Seeded complex64 Y [B, 2, F, T] and a mask [B, F, T] whose rows mix exact 0, exact 1
    (all-target: count 0), uniform (0, 1), values below pf_floor and a blend of them."""
    F = n_fft // 2 + 1
    rng = np.random.default_rng([77, n_fft, T])
    Y = (rng.standard_normal((B, 2, F, T)) + 1j * rng.standard_normal((B, 2, F, T))).astype(np.complex64)
    M = rng.random((B, F, T)).astype(np.float32)
    kind = (np.arange(F)[None, :] + 2 * np.arange(B)[:, None]) % 5
    M[kind == 0] = 0.0
    M[kind == 1] = 1.0
    M[kind == 3] *= np.float32(0.9 * PF_FLOOR)
    blend = rng.integers(0, 3, (B, F, T))
    M = np.where((kind == 4)[:, :, None] & (blend == 0), np.float32(0), M)
    M = np.where((kind == 4)[:, :, None] & (blend == 1), np.float32(1), M).astype(np.float32)
    return Y, M


def spectral_plan(kind, pf, n_fft, B):
    import avz
    common = dict(n_fft=n_fft, fs=C.FS, mask="external", postfilter=pf, pf_floor=PF_FLOOR,
                  normalize="none", max_batch=B, max_samples=n_fft)
    if kind == "mvdr":
        return avz.MVDRPlan(sigma=SPEC_SIGMA, mic_d=C.MIC_D_MVDR, weight_eps=1e-10, fmin_hz=0.0,
                            singular_fallback="batch", **common)
    return avz.MVDRPlan(beamformer="hybrid_null", mic_d=C.MIC_D_HYBRID, bypass_hz=C.BYPASS,
                        cond_max=C.COND_MAX, **common)


def check_spectral(gpu_device, kind, pf, n_fft, T, steer):
    B, F = 2, n_fft // 2 + 1
    Y, M = spectral_inputs(n_fft, T, B)
    plan = spectral_plan(kind, pf, n_fft, B)
    st = C.steer_mvdr(n_fft) if kind == "mvdr" else C.steer_hybrid(n_fft)
    cov = torch.full((B, F, 5), -1.0, dtype=torch.float64, device=gpu_device)
    w = torch.full((B, F, 4), -1.0, dtype=torch.float32, device=gpu_device)
    flags = torch.full((B,), 7, dtype=torch.int32, device=gpu_device)
    S = plan.beamform_spectral(dev_t(Y, gpu_device), dev_t(M, gpu_device), cov_out=cov, w_out=w,
                               fallback=flags, steer=steer_arg(st, steer, gpu_device))
    S = S.cpu().numpy().astype(np.complex128)
    cg = cov.cpu().numpy()
    # the covariance: fp64 sums of (float32(1 - m) + weight_eps) * terms, the reference in long
    # double so that the bound (an fp64 sum of T terms in any order) is the kernel's alone.
    # weight_eps is the plan's, a float in the kernels' argument block (as numpy's float32
    # "1 - mask + 1e-10" of the reference makes it for an all-target row)
    eps = C.LD(np.float32(1e-10)) if kind == "mvdr" else C.LD(0.0)
    mn = (np.float32(1.0) - M).astype(np.float32).astype(C.LD)
    wg = mn + eps
    y0, y1 = Y[:, 0].astype(C.CLD), Y[:, 1].astype(C.CLD)
    b = (wg * y0 * np.conj(y1)).sum(axis=2)
    ref = np.stack([(wg * np.abs(y0) ** 2).sum(axis=2), (wg * np.abs(y1) ** 2).sum(axis=2),
                    b.real, b.imag, mn.sum(axis=2)], axis=2)
    u = T * 2.0 ** -50
    cross = np.sqrt(ref[..., 0] * ref[..., 1])
    tol = np.stack([u * ref[..., 0], u * ref[..., 1], u * cross, u * cross,
                    u * np.maximum(ref[..., 4], 1.0)], axis=2)
    err = np.abs(cg.astype(C.LD) - ref)
    assert (err <= tol).all(), (kind, T, np.argwhere(~(err <= tol))[:8])
    # the weights: LAPACK on the kernel's own covariance
    f = C.bin_freqs(n_fft)
    E = C.reference_error()["M1"]
    Wg = to_c(w)
    Wl = np.empty((B, F, 2), dtype=np.complex128)
    worst = 0.0
    for bi in range(B):
        if kind == "mvdr":
            Wl[bi], raised = C.mvdr_lapack(cg[bi], f, SPEC_SIGMA, st, 0.0, "batch")
            assert not raised.any()
        else:
            Wl[bi], _, _ = C.hybrid_lapack(cg[bi], f, st, C.BYPASS, C.COND_MAX)
            assert (Wg[bi][f < C.BYPASS] == [1.0, 0.0]).all()
        worst = max(worst, assert_weights(Wg[bi], Wl[bi], E, (kind, pf, T, bi)))
    assert flags.tolist() == ([0, 0] if kind == "mvdr" else [7, 7])
    # S = gain * (w^H y), the gain from the same mask
    gain = {"none": np.ones_like(M), "floor": np.maximum(M, np.float32(PF_FLOOR)), "mul": M}[pf]
    gain = gain.astype(np.float64)
    Yd = Y.astype(np.complex128)
    Sr = gain * (Wl[:, :, 0].conj()[:, :, None] * Yd[:, 0] + Wl[:, :, 1].conj()[:, :, None] * Yd[:, 1])
    tolS = 4 * 2.0 ** -24 * gain * (np.abs(Wl[:, :, 0])[:, :, None] * np.abs(Yd[:, 0])
                                    + np.abs(Wl[:, :, 1])[:, :, None] * np.abs(Yd[:, 1]))
    errS = np.abs(S - Sr)
    assert (errS <= tolS).all(), (kind, pf, T, np.argwhere(~(errS <= tolS))[:8])
    print(f"spectral {kind} pf={pf} N={n_fft} T={T}: weights worst {worst:.2f} x 2^-24 |w|, "
          f"cov worst {float((err / np.maximum(tol, C.LD(1e-300))).max()):.2f} of its bound")


@pytest.mark.parametrize("T", [1, 16, 17, 63, 64, 65, 128, 129])
@pytest.mark.parametrize("pf", ["none", "floor", "mul"])
@pytest.mark.parametrize("kind", ["mvdr", "hybrid"])
def test_spectral_cov_weights_and_output(gpu_device, kind, pf, T):
    """N = 512: 2 x 257 rows, no multiple of the 16 rows per block of the rows kernel (T <= 64)
    nor of the 4 rows per block of the wave kernel (T > 64)."""
    check_spectral(gpu_device, kind, pf, 512, T, "oracle")


@pytest.mark.parametrize("kind", ["mvdr", "hybrid"])
def test_spectral_n1024_instantiation(gpu_device, kind):
    check_spectral(gpu_device, kind, "floor" if kind == "mvdr" else "mul", 1024, 64, "plan")


# ----------------------------------------------------------------------------
# (c) fused chain against its own export
# ----------------------------------------------------------------------------
CHAIN_LEN = 24000
CHAIN_PLANS = {
    "hybrid-ibm": dict(mic_d=C.MIC_D_HYBRID, mask="ibm", postfilter="ibm", beamformer="hybrid_null",
                       normalize="none"),
    "mvdr-batch-external": dict(sigma=1e-5, mic_d=C.MIC_D_MVDR, mask="external", postfilter="floor",
                                weight_eps=1e-10, fmin_hz=0.0, singular_fallback="batch",
                                normalize="none"),
    "mvdr-mic0-ipd": dict(sigma=1e-7, mic_d=0.01, mask="ipd", postfilter="none",
                          normalize="peak", norm_eps=1e-6),
}


@pytest.fixture(scope="module")
def chain_audio():
    return triple_f32("test", seg=(40000, 40000 + CHAIN_LEN))


@pytest.mark.parametrize("ragged", [False, True], ids=["B1", "B3-ragged"])
@pytest.mark.parametrize("n_fft", C.N_FFTS)
@pytest.mark.parametrize("name", list(CHAIN_PLANS))
def test_fused_chain_solves_as_its_export(gpu_device, chain_audio, name, n_fft, ragged):
    import avz
    mix, t, i = chain_audio
    d = gpu_device
    lens = [CHAIN_LEN, n_fft, 16000] if ragged else [CHAIN_LEN]
    B = len(lens)
    kw = CHAIN_PLANS[name]
    plan = avz.MVDRPlan(n_fft=n_fft, max_batch=B, max_samples=CHAIN_LEN, **kw)
    Mx = np.zeros((B, 2, CHAIN_LEN), np.float32)
    Tg = np.zeros((B, CHAIN_LEN), np.float32)
    It = np.zeros((B, CHAIN_LEN), np.float32)
    for b, L in enumerate(lens):
        off = 1000 * b
        Mx[b, :, :L], Tg[b, :L], It[b, :L] = mix[:, off:off + L], t[off:off + L], i[off:off + L]
    args = dict(lengths=dev_t(np.array(lens, np.int32), d), max_len=CHAIN_LEN)
    if kw["mask"] == "ibm":
        args.update(ref_tgt=dev_t(Tg, d), ref_int=dev_t(It, d))
    if kw["mask"] == "external":
        rng = np.random.default_rng([5, n_fft, B])
        em = rng.random((B, plan.F, plan.frames(CHAIN_LEN))).astype(np.float32)
        em[:, 5::7] = 1.0                      # all-target rows: count 0, weight_eps sums
        args.update(ext_mask=dev_t(em, d))
    cov = torch.full((B, plan.F, 5), -1.0, dtype=torch.float64, device=d)
    w = torch.full((B, plan.F, 4), -1.0, dtype=torch.float32, device=d)
    plan.run(dev_t(Mx, d), cov_out=cov, w_out=w, **args)
    w_stage = plan.solve_covariance(cov)
    assert torch.equal(w_stage, w)             # the chain's solve is the export's, bit for bit
    f = C.bin_freqs(n_fft)
    cg = cov.cpu().numpy()
    Wg = to_c(w)
    worst = 0.0
    for b in range(B):
        if kw.get("beamformer") == "hybrid_null":
            st = C.steer_hybrid(n_fft)
            Wl, _, _ = C.hybrid_lapack(cg[b], f, st, C.BYPASS, C.COND_MAX)
            Wt, _ = C.hybrid_truth(cg[b], f, st, C.BYPASS, C.COND_MAX)
            assert (Wg[b][f < C.BYPASS] == [1.0, 0.0]).all()
        else:
            st = O.steering_vectors(f, O.ANGLE_TARGET, kw["mic_d"], O.C_SOUND)
            fmin = kw.get("fmin_hz", O.FMIN_MVDR)
            Wl, raised = C.mvdr_lapack(cg[b], f, kw["sigma"], st, fmin, kw.get("singular_fallback", "mic0"))
            Wt = C.mvdr_truth(cg[b], f, kw["sigma"], st, fmin)
            assert not raised.any()
            assert (Wg[b][f < fmin] == 0).all()
        # E_ref of this very covariance: LAPACK against the long-double value
        num = np.abs(Wl.astype(C.CLD) - Wt).max(axis=1)
        E = float((num / np.maximum(np.abs(Wt).max(axis=1), C.LD(1e-300))).max())
        assert E < 1e-8, E
        worst = max(worst, assert_weights(Wg[b], Wl, E, (name, n_fft, b)))
    print(f"chain {name} N={n_fft} B={B}: weights worst {worst:.2f} x 2^-24 |w|")
