"""GPU: the mask-gain and spectrum-input synthesis paths (chunk-grid avz_synthesis_kernel +
avz_finalize_kernel, the external-mask branch of the analysis kernel) against the fp64
references and memory layouts of tests/gain_cases.py.

  1. fused external-mask plans (post-filter floor / mul / none, MVDR and the hybrid null,
     un-normalised and peak-normalised, weight_eps 0 and 1e-10) on one ragged batch of 29 rows
     per size: Tier 1 (whole chain, 1e-4) and Tier 2 (synthesis isolated, from the call's own
     w_out: 4 E_pert + 2e-6 max|x| + 2^-23 max|x|), extents, peaks, exact noise counts;
  2. the same plans with the mask in layouts B-H: bits of out, peak, cov_out and w_out equal
     layout A's (the vector and the scalar reads run the same fp32 operations; every padding
     entry, extra bin and frame past a row's own count is NaN);
  3. avz_apply_istft with a caller gain in [0, 2) and caller weights; against the fused `mul`
     plan; without a gain against an all-ones gain;
  4. avz_istft at every frame count and spectrum layout, frames = 3 / 2, a caller workspace;
  5. 2 #CU + 5 rows: more (chunk, row) items than blocks of the persistent grid;
  6. a NaN in one row's mask stays in that row; a row shorter than a frame is skipped.

`out`, `cov_out` and `w_out` are pre-filled with NaN (`out` with spare columns), `peak` with 7.
Each fused test first asserts from the plan's kernel timing that its launch ran all four
kernels (utt_cases.assert_path): these plans stay on the chunk grid. A plan without a
post-filter would take the per-utterance kernel when peak-normalised, so those plans are held
on the chunk grid with set_diagnostics(synth_variant=0). Tolerances are the suite's own
(gain_cases: WAVE_TOL, STFT_TOL, ISTFT_TOL, STAGE_TOL); each test prints its largest deviation
as a fraction of its bound (pytest -s); the measured table is DESIGN.md section 20.

Measured on one MI355X (256 CUs) on 2026-10-21, on the commit that adds this file (its parent
is 3ed97a1). The first run found the N = 1024 `floor` / `mul` instances' vector and scalar
reads one ulp apart in `peak` (the compiler contracted the two instances of the apply phase
differently); the memory-gain instances now spell their roundings out and every layout
identity holds bitwise. Largest fractions of the bounds: Tier 1 0.0051, peak 0.0037, Tier 2
0.030; avz_istft 0.13 of 2e-6; apply_istft against the fused mul plan 0.30 and no gain against
unit gain 0.36 of 1e-6. 118 tests, 6.9 s.
"""
import functools

import numpy as np
import pytest
import torch

import gain_cases as GC
import utt_cases as UC

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 7.0
OUT_PAD = 8

MVDR_CASES = [("mvdr", pf, norm, eps) for pf in ("floor", "mul", "none")
              for norm in ("none", "peak") for eps in GC.WEIGHT_EPS]
HYBRID_CASES = [("hybrid", pf, norm, 0.0) for pf in ("mul", "none") for norm in ("none", "peak")]
FUSED_CASES = [(n,) + c for n in GC.SIZES for c in MVDR_CASES + HYBRID_CASES]
H_ROW = len(GC.rows(1024)) - 1   # layout H's one mask: the longest row's (all T_max frames)


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _dev(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)   # a copy: cached inputs are read-only


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _view(buf, spec):
    _, offset, shape, strides = spec
    return torch.as_strided(buf, shape, strides, offset)


# ----------------------------------------------------------------------------- inputs
class Batch:
    """rows(n) (or other lengths) on the device."""

    def __init__(self, n, dev, lens=None):
        self.n, self.H, self.F, self.dev = n, n // 2, n // 2 + 1, dev
        x, lens = GC.batch(n, lens)
        self.lens_h = lens
        self.B, self.S = x.shape[0], x.shape[2]
        self.max_len = int(lens.max())
        self.x, self.lens = _dev(x, dev), _dev(lens, dev)
        self.live_h = lens >= n
        self.T_h = np.array([GC.n_frames(int(L), n) if L >= n else 1 for L in lens])
        self.n_out_h = (self.T_h - 1) * self.H
        self.n_out = _dev(self.n_out_h.astype(np.int64), dev)
        self.live = _dev(self.live_h, dev)
        self.out_cols = (GC.n_frames(self.max_len, n) - 1) * self.H + OUT_PAD
        self.logical = GC.padded_masks(n, lens)

    def valid(self):
        return (torch.arange(self.out_cols, device=self.dev)[None, :] < self.n_out[:, None]) \
            & self.live[:, None]


@functools.lru_cache(maxsize=None)
def _batch(n, dev):
    return Batch(n, dev)


@functools.lru_cache(maxsize=None)
def _mask(n, lid, dev, which="mask"):
    """The batch's masks (which = "mask"), gains ("gain") or layout H's one mask replicated
    ("rep") as the view of layout `lid` of a NaN-filled device buffer."""
    bt = _batch(n, dev)
    Tp = GC.t_pad(n)
    if which == "gain":
        logical = GC.padded_masks(n, bt.lens_h, draw=GC.row_gain)
    elif which == "rep" or lid == "H":
        logical = np.broadcast_to(bt.logical[H_ROW], bt.logical.shape)
    else:
        logical = bt.logical
    spec = GC.mask_layout(lid, bt.B, bt.F, Tp)
    buf = _dev(GC.place(logical[0] if lid == "H" else logical, spec), dev)
    return _view(buf, spec)


def _plan_kw(bf, pf, norm, eps):
    kw = dict(mask="external", postfilter=pf, pf_floor=GC.PF_FLOOR, sigma=GC.SIGMA,
              mic_d=GC.MIC_D, weight_eps=eps, normalize=norm,
              norm_eps=GC.NORM_EPS if norm == "peak" else 0.0)
    if bf == "hybrid":
        kw.update(beamformer="hybrid_null", **GC.HYBRID)
    return kw


@functools.lru_cache(maxsize=None)
def _plan(n, bf, pf, norm, eps, B, S):
    import avz
    return avz.MVDRPlan(n_fft=n, max_batch=B, max_samples=S, **_plan_kw(bf, pf, norm, eps))


class Result:
    def __init__(self, out, peak, cov, w):
        self.out, self.peak, self.cov, self.w = out, peak, cov, w

    def same_bits(self, other, rows=None):
        for k in ("peak", "w", "cov", "out"):
            a, b = getattr(self, k), getattr(other, k)
            if rows is not None:
                a, b = a[rows], b[rows]
            if not _same_bits(a, b):
                bad = torch.nonzero(_bits(a) != _bits(b))
                d = torch.nan_to_num((a.double() - b.double()).abs()).max().item()
                return (f"{k} differs at {bad[:6].tolist()} ({bad.shape[0]} entries, largest "
                        f"|d| {d:.3e}, largest |value| {torch.nan_to_num(b.double()).abs().max().item():.3e})")
        return None


def _run_fused(pl, bt, mask, pf, check_path=True, x=None, lens=None):
    """One avz_mvdr_batch of batch bt with `mask` into NaN / sentinel-filled buffers, all four
    kernels asserted; plans without a post-filter are held on the chunk grid."""
    x = bt.x if x is None else x
    lens = bt.lens if lens is None else lens
    B = x.shape[0]
    out = torch.full((B, bt.out_cols), NAN, device=bt.dev)
    peak = torch.full((B,), SENTINEL, device=bt.dev)
    cov = torch.full((B, bt.F, 5), NAN, dtype=torch.float64, device=bt.dev)
    w = torch.full((B, bt.F, 4), NAN, device=bt.dev)

    def go():
        pl.run(x, lens, max_len=bt.max_len, ext_mask=mask, out=out, peak=peak, cov_out=cov,
               w_out=w)
        torch.cuda.synchronize()

    if pf == "none":
        pl.set_diagnostics(synth_variant=0)
    try:
        if check_path:
            UC.assert_path(pl, go, solve=True, finalize=True)
        else:
            go()
    finally:
        if pf == "none":
            pl.set_diagnostics(synth_variant=2)
    return Result(out, peak, cov, w)


@functools.lru_cache(maxsize=None)
def _base(n, bf, pf, norm, eps, dev, which="mask"):
    """Layout A's run of a fused case (shared by the tests that compare against it)."""
    bt = _batch(n, dev)
    pl = _plan(n, bf, pf, norm, eps, bt.B, bt.S)
    return bt, pl, _run_fused(pl, bt, _mask(n, "A", dev, which), pf)


# ----------------------------------------------------------------------------- checks
def _check_extents(bt, out, peak, norm, eps_n, live=None):
    """Nothing written past (T_b - 1) H or in a skipped row, no NaN inside; the peak against
    the written values. Returns |max|out| - peak / (peak + eps)| (peak plans)."""
    valid = bt.valid() if live is None else bt.valid() & live[:, None]
    lv = bt.live if live is None else bt.live & live
    isn = ~torch.isfinite(out)
    bad = torch.nonzero(~torch.isnan(out) & ~valid)
    assert bad.numel() == 0, ("written outside the extent", bad[:8].tolist())
    bad = torch.nonzero(isn & valid)
    assert bad.numel() == 0, ("non-finite inside a live row", bad[:8].tolist())
    assert bool(torch.isnan(peak[~bt.live]).all())
    pk = peak[lv].double()
    assert bool((torch.isfinite(pk) & (pk > 0)).all())
    amax = torch.where(valid, out.abs(), torch.zeros_like(out)).amax(dim=1)[lv]
    if norm == "none":
        # the un-normalised branch: peak is the max over the very values written
        assert _same_bits(amax, peak[lv]), torch.nonzero(_bits(amax) != _bits(peak[lv]))[:8].tolist()
        return 0.0
    dev_ = (amax.double() - pk / (pk + eps_n)).abs().max().item()
    assert dev_ <= 1e-6, dev_
    return dev_


_T2 = {}


def _tier2_cached(key, n, b, L, w_row, G):
    """gain_cases.tier2 from the call's own w_out; reused by the cases whose w_out row has the
    same bits (a plan's two normalisations)."""
    hit = _T2.get(key)
    if hit is not None and np.array_equal(hit[0], w_row):
        return hit[1]
    res = GC.tier2(n, b, L, GC.weights_from_f32(w_row), G)
    _T2[key] = (w_row.copy(), res)
    return res


def _check_rows_fp64(tag, n, bf, pf, norm, eps, bt, res, rows, one_mask=False):
    """Tier 1 (MVDR plans) and Tier 2 of the given rows, each with its own mask or (one_mask)
    with layout H's; returns the largest fractions of the bounds."""
    oh = res.out.cpu().numpy().astype(np.float64)
    ph = res.peak.cpu().numpy().astype(np.float64)
    wh = res.w.cpu().numpy()
    eps_n = GC.NORM_EPS if norm == "peak" else 0.0
    worst = dict(t1=0.0, pk=0.0, t2=0.0)
    for b in rows:
        L, T = int(bt.lens_h[b]), int(bt.T_h[b])
        M = GC.row_mask(n, H_ROW, max(GC.FRAMES))[:, :T] if one_mask else GC.row_mask(n, b, T)
        got = oh[b, :bt.n_out_h[b]]
        if bf == "mvdr":
            if one_mask:
                ref = GC.chain_reference(GC.row_signal(n, b, L), M, GC.gain_of(M, pf), n, eps)
                r = dict(out=ref, peak=float(np.abs(ref).max()))
            else:
                r = GC.tier1(n, b, L, pf, eps)
            scale = 1.0 / (r["peak"] + eps_n) if norm == "peak" else 1.0
            e1 = np.abs(got - r["out"] * scale).max() / (GC.WAVE_TOL * r["peak"] * scale)
            epk = abs(ph[b] - r["peak"]) / (GC.PEAK_RTOL * r["peak"])
            assert e1 <= 1 and epk <= 1, (tag, b, T, L, e1, epk)
            worst["t1"], worst["pk"] = max(worst["t1"], e1), max(worst["pk"], epk)
        assert np.isfinite(wh[b]).all(), (tag, b)
        x, _, tol = _tier2_cached((n, bf, pf, eps, b, one_mask), n, b, L, wh[b],
                                  GC.gain_of(M, pf))
        scale = 1.0 / (np.abs(x).max() + eps_n) if norm == "peak" else 1.0
        e2 = np.abs(got - x * scale).max() / (tol * scale)
        assert e2 <= 1, (tag, b, T, L, e2)
        worst["t2"] = max(worst["t2"], e2)
    print(f"{tag}: largest fraction of the bound: Tier 1 {worst['t1']:.4f}, peak "
          f"{worst['pk']:.4f}, Tier 2 {worst['t2']:.4f}")
    return worst


def _check_counts(bt, res, logical):
    """cov_out[:, :, 4], the noise count sum (1 - M), is exact where the mask is 0 or 1."""
    cnt = res.cov[:, :, 4].cpu().numpy()
    for b in np.nonzero(bt.live_h)[0]:
        T = int(bt.T_h[b])
        Mb = logical[b, :, :T]
        zero, one = (Mb == 0).all(axis=1), (Mb == 1).all(axis=1)
        assert zero.any() and one.any()
        assert np.array_equal(cnt[b, zero], np.full(zero.sum(), float(T))), b
        assert np.array_equal(cnt[b, one], np.zeros(one.sum())), b


# ----------------------------------------------------------------------------- 1. fused plans
@pytest.mark.parametrize("n,bf,pf,norm,eps", FUSED_CASES)
def test_fused_plan_against_fp64(gpu_device, n, bf, pf, norm, eps):
    bt, pl, res = _base(n, bf, pf, norm, eps, gpu_device)
    tag = f"N={n} {bf} {pf} {norm} weight_eps={eps:g}"
    d = _check_extents(bt, res.out, res.peak, norm, GC.NORM_EPS)
    if norm == "peak":
        print(f"{tag}: largest |max|out| - peak / (peak + eps)| = {d:.2e} (bound 1e-6)")
    _check_counts(bt, res, bt.logical)
    assert bool(torch.isfinite(res.cov).all()) and bool(torch.isfinite(res.w).all())
    _check_rows_fp64(tag, n, bf, pf, norm, eps, bt, res, range(bt.B))


# ----------------------------------------------------------------------------- 2. layouts
@pytest.mark.parametrize("n,bf,pf,norm,eps", FUSED_CASES)
def test_mask_layouts_give_layout_a_bits(gpu_device, n, bf, pf, norm, eps):
    bt, pl, res = _base(n, bf, pf, norm, eps, gpu_device)
    for lid in "BCDEFG":
        r = _run_fused(pl, bt, _mask(n, lid, gpu_device), pf, check_path=False)
        why = r.same_bits(res)
        assert why is None, (lid, GC.MASK_LAYOUTS[lid], why)
    # one mask for the whole batch against the same mask replicated
    _, _, rep = _base(n, bf, pf, norm, eps, gpu_device, "rep")
    r = _run_fused(pl, bt, _mask(n, "H", gpu_device), pf, check_path=False)
    why = r.same_bits(rep)
    assert why is None, ("H", GC.MASK_LAYOUTS["H"], why)
    d = _check_extents(bt, rep.out, rep.peak, norm, GC.NORM_EPS)
    assert d <= 1e-6
    if eps == 0.0 and norm == "none":   # the replicated mask against fp64 on the step-edge rows
        rows = [b for b, (T, L) in enumerate(GC.rows(n)) if T in (9, 33, 65, 97)]
        _check_rows_fp64(f"N={n} {bf} {pf} one mask", n, bf, pf, norm, eps, bt, rep, rows,
                         one_mask=True)


# ----------------------------------------------------------------------------- 3. apply_istft
@functools.lru_cache(maxsize=None)
def _apply_plan(n, norm, B, S):
    import avz
    return avz.MVDRPlan(n_fft=n, max_batch=B, max_samples=S, **_plan_kw("mvdr", "none", norm, 0.0))


def _run_apply(pl, bt, w, gain, variant0=False):
    out = torch.full((bt.B, bt.out_cols), NAN, device=bt.dev)
    peak = torch.full((bt.B,), SENTINEL, device=bt.dev)
    if variant0:
        pl.set_diagnostics(synth_variant=0)
    try:
        pl.apply_istft(bt.x, w, bt.lens, max_len=bt.max_len, gain=gain, out=out, peak=peak)
        torch.cuda.synchronize()
    finally:
        if variant0:
            pl.set_diagnostics(synth_variant=2)
    return out, peak


@pytest.mark.parametrize("norm", ["none", "peak"])
@pytest.mark.parametrize("n", GC.SIZES)
def test_apply_istft_caller_gain(gpu_device, n, norm):
    """Caller weights and a gain in [0, 2) (applied as given: no clamp): Tier 2 on every row,
    layouts C and F give layout A's bits."""
    bt = _batch(n, gpu_device)
    pl = _apply_plan(n, norm, bt.B, bt.S)
    W = GC.caller_weights(n, bt.B)
    w32 = GC.weights_to_f32(W)
    w = _dev(w32, gpu_device)
    out, peak = _run_apply(pl, bt, w, _mask(n, "A", gpu_device, "gain"))
    _check_extents(bt, out, peak, norm, GC.NORM_EPS)
    for lid in "CF":
        o2, p2 = _run_apply(pl, bt, w, _mask(n, lid, gpu_device, "gain"))
        assert _same_bits(o2, out) and _same_bits(p2, peak), (lid, GC.MASK_LAYOUTS[lid])
    oh = out.cpu().numpy().astype(np.float64)
    eps_n = GC.NORM_EPS if norm == "peak" else 0.0
    worst = 0.0
    for b, (T, L) in enumerate(GC.rows(n)):
        x, _, tol = GC.tier2(n, b, L, GC.weights_from_f32(w32[b]), GC.row_gain(n, b, T))
        scale = 1.0 / (np.abs(x).max() + eps_n) if norm == "peak" else 1.0
        e = np.abs(oh[b, :bt.n_out_h[b]] - x * scale).max() / (tol * scale)
        assert e <= 1, (b, T, L, e)
        worst = max(worst, e)
    print(f"apply_istft N={n} {norm}: largest fraction of the Tier 2 bound {worst:.4f}")


@pytest.mark.parametrize("norm", ["none", "peak"])
@pytest.mark.parametrize("n", GC.SIZES)
def test_apply_istft_against_the_fused_mul_plan(gpu_device, n, norm):
    """The fused `mul` plan's w_out and mask through avz_apply_istft: the same synthesis from
    weights rounded to fp32 (STAGE_TOL of the row's scale)."""
    bt, _, res = _base(n, "mvdr", "mul", norm, 0.0, gpu_device)
    pl = _apply_plan(n, norm, bt.B, bt.S)
    out, peak = _run_apply(pl, bt, res.w, _mask(n, "A", gpu_device))
    valid = bt.valid()
    zero = torch.zeros_like(out)
    scale = torch.where(valid, res.out.abs(), zero).amax(dim=1)
    d = (torch.where(valid, (out - res.out).abs(), zero).amax(dim=1) / scale).max().item()
    dp = ((peak - res.peak).abs() / res.peak).max().item()
    print(f"apply_istft N={n} {norm} against the fused mul plan: |d out| {d:.3e} of the row's "
          f"scale ({d / GC.STAGE_TOL:.4f} of the bound), |d peak| / peak {dp:.3e}")
    assert d <= GC.STAGE_TOL and dp <= GC.STAGE_TOL
    assert bool(torch.isnan(out[~valid]).all())


@pytest.mark.parametrize("norm", ["none", "peak"])
@pytest.mark.parametrize("n", GC.SIZES)
def test_apply_istft_without_gain_equals_unit_gain(gpu_device, n, norm):
    """No gain (the PF_NONE instance, held on the chunk grid) against an all-ones gain (the
    PF_EXT_MUL instance; at N = 512 8-frame against 16-frame steps). A product by 1.0f is
    exact, but the two instances round alpha z + beta conj(z') differently: the memory-gain
    instances spell their roundings out so that their vector and scalar reads agree, the
    PF_NONE instance leaves the contraction to the compiler. Not bitwise, then (measured
    3.6e-7 of a row's scale at most): section 14's stage bound."""
    bt = _batch(n, gpu_device)
    pl = _apply_plan(n, norm, bt.B, bt.S)
    w = _dev(GC.weights_to_f32(GC.caller_weights(n, bt.B)), gpu_device)
    ones = torch.ones((bt.B, bt.F, GC.t_pad(n)), device=gpu_device)
    o1, p1 = _run_apply(pl, bt, w, ones)
    o0, p0 = _run_apply(pl, bt, w, None, variant0=True)
    valid = bt.valid()
    zero = torch.zeros_like(o0)
    scale = torch.where(valid, o1.abs(), zero).amax(dim=1)
    d = (torch.where(valid, (o0 - o1).abs(), zero).amax(dim=1) / scale).max().item()
    same = _same_bits(o0, o1) and _same_bits(p0, p1)
    print(f"apply_istft N={n} {norm}: no gain against unit gain: bitwise {same}, largest "
          f"|d out| {d:.3e} of the row's scale ({d / GC.STAGE_TOL:.4f} of the bound)")
    assert d <= GC.STAGE_TOL and _same_bits(torch.isnan(o0), torch.isnan(o1))
    assert (p0 - p1).abs().max().item() <= GC.STAGE_TOL * p1.max().item()


# ----------------------------------------------------------------------------- 4. avz_istft
@functools.lru_cache(maxsize=None)
def _istft_plan(n, norm):
    import avz
    return avz.MVDRPlan(n_fft=n, mask="external", postfilter="none", normalize=norm,
                        norm_eps=GC.NORM_EPS if norm == "peak" else 0.0,
                        max_batch=GC.SPEC_BATCH, max_samples=(max(GC.FRAMES) - 1) * (n // 2))


def _run_istft(pl, S, n_out, dev, workspace=None):
    out = torch.full((S.shape[0], n_out + OUT_PAD), NAN, device=dev)
    peak = torch.full((S.shape[0],), SENTINEL, device=dev)
    pl.istft(S, out=out, peak=peak, workspace=workspace)
    torch.cuda.synchronize()
    return out, peak


@pytest.mark.parametrize("T", GC.FRAMES)
@pytest.mark.parametrize("n", GC.SIZES)
def test_istft_frame_counts_and_layouts(gpu_device, n, T):
    F, H, B = n // 2 + 1, n // 2, GC.SPEC_BATCH
    n_out = (T - 1) * H
    ref = GC.istft_reference(n, T)
    S_h = GC.spectra(n, T)
    views = {}
    for lid in GC.SPEC_LAYOUTS:
        spec = GC.spec_layout(lid, B, F, T)
        views[lid] = _view(_dev(GC.place(S_h, spec), gpu_device), spec)
    pl = _istft_plan(n, "none")
    out, peak = _run_istft(pl, views["A"], n_out, gpu_device)
    assert bool(torch.isnan(out[:, n_out:]).all()) and bool(torch.isfinite(out[:, :n_out]).all())
    got, pk = out[:, :n_out].cpu().numpy(), peak.cpu().numpy()
    scale = np.abs(ref).max(axis=1)
    e = (np.abs(got - ref).max(axis=1) / (GC.ISTFT_TOL * scale)).max()
    ep = (np.abs(pk - scale) / (GC.ISTFT_TOL * scale)).max()
    assert np.array_equal(pk, np.abs(got).max(axis=1))
    for lid in "BCDE":
        o2, p2 = _run_istft(pl, views[lid], n_out, gpu_device)
        assert _same_bits(o2, out) and _same_bits(p2, peak), (lid, GC.SPEC_LAYOUTS[lid])
    # a caller workspace of exactly the stated size (filled with ones) gives the plan's bits
    nbytes = pl.workspace_bytes(B, n_out)
    ws = torch.full((max(nbytes, 1),), 0xFF, dtype=torch.uint8, device=gpu_device)
    o3, p3 = _run_istft(pl, views["A"], n_out, gpu_device, workspace=ws)
    assert _same_bits(o3, out) and _same_bits(p3, peak)
    # peak normalisation: three fp32 roundings (peak + eps, the reciprocal, the product)
    pn = _istft_plan(n, "peak")
    worst_n = 0.0
    for lid in GC.SPEC_LAYOUTS:
        on, pkn = _run_istft(pn, views[lid], n_out, gpu_device)
        assert _same_bits(pkn, peak), lid
        assert bool(torch.isnan(on[:, n_out:]).all())
        want = got.astype(np.float64) / (pk.astype(np.float64)[:, None] + GC.NORM_EPS)
        err = np.abs(on[:, :n_out].cpu().numpy() - want)
        assert (err <= 2.0 ** -22 * np.abs(want)).all(), lid
        nz = want != 0
        worst_n = max(worst_n, float((err[nz] / (2.0 ** -22 * np.abs(want[nz]))).max()))
    print(f"istft N={n} T={T}: {e:.4f} of 2e-6 max|ref|, peak {ep:.4f}; normalised "
          f"{worst_n:.3f} of 2^-22 |y|; layouts and caller workspace bitwise")
    assert e <= 1 and ep <= 1


@pytest.mark.parametrize("n", GC.SIZES)
def test_istft_refuses_two_frames(gpu_device, n):
    """(frames - 1) hop < n_fft is refused (AVZ_ERR_SHAPE) although scipy accepts two frames;
    three frames are the smallest call (include/avz.h)."""
    import avz
    pl = _istft_plan(n, "none")
    S = _dev(GC.spectra(n, 3), gpu_device)
    out = torch.full((GC.SPEC_BATCH, n + OUT_PAD), NAN, device=gpu_device)
    peak = torch.full((GC.SPEC_BATCH,), SENTINEL, device=gpu_device)
    with pytest.raises(avz.AvzError, match=r"\(-2\)"):
        pl.istft(S[:, :, :2].contiguous(), out=out, peak=peak)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((peak == SENTINEL).all())
    pl.istft(S, out=out, peak=peak)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:, :n]).all()) and bool(torch.isnan(out[:, n:]).all())


# ----------------------------------------------------------------------------- 5. many rows
@pytest.mark.parametrize("n", GC.SIZES)
def test_more_items_than_blocks(gpu_device, n):
    """2 #CU + 5 rows of up to three chunks: the persistent grid's `it += gridDim.x` loop with
    a memory gain, un-normalised and peak-normalised; sampled rows against Tier 2 from the
    call's own w_out. (Rows are not compared with a small batch: the analysis tail split
    changes the fp64 association of the covariance sums.)"""
    import avz
    R = _cus(gpu_device)
    T, lens, sampled = GC.many_rows(R, n)
    x_h, M_h = GC.many_inputs(R, n)
    B, S, F, H = len(lens), x_h.shape[2], n // 2 + 1, n // 2
    x, M, lens_d = _dev(x_h, gpu_device), _dev(M_h, gpu_device), _dev(lens, gpu_device)
    n_out_h = (T - 1) * H
    n_out = _dev(n_out_h.astype(np.int64), gpu_device)
    cols = int(n_out_h.max()) + OUT_PAD
    valid = torch.arange(cols, device=gpu_device)[None, :] < n_out[:, None]
    for norm in ("none", "peak"):
        pl = avz.MVDRPlan(n_fft=n, max_batch=B, max_samples=S, **_plan_kw("mvdr", "floor", norm, 0.0))
        runs = []
        for _ in range(2):
            out = torch.full((B, cols), NAN, device=gpu_device)
            peak = torch.full((B,), SENTINEL, device=gpu_device)
            w = torch.full((B, F, 4), NAN, device=gpu_device)

            def go():
                pl.run(x, lens_d, max_len=S, ext_mask=M, out=out, peak=peak, w_out=w)
                torch.cuda.synchronize()

            UC.assert_path(pl, go, solve=True, finalize=True)
            runs.append((out, peak, w))
        (out, peak, w), (o2, p2, w2) = runs
        assert _same_bits(o2, out) and _same_bits(p2, peak) and _same_bits(w2, w)
        assert bool(torch.isfinite(out[valid]).all()) and bool(torch.isnan(out[~valid]).all())
        assert bool((torch.isfinite(peak) & (peak > 0)).all()) and bool(torch.isfinite(w).all())
        amax = torch.where(valid, out.abs(), torch.zeros_like(out)).amax(dim=1)
        if norm == "none":
            assert _same_bits(amax, peak)
        else:
            pk = peak.double()
            assert (amax.double() - pk / (pk + GC.NORM_EPS)).abs().max().item() <= 1e-6
        idx = torch.tensor(sampled, device=gpu_device)
        oh, wh = out[idx].cpu().numpy().astype(np.float64), w[idx].cpu().numpy()
        worst = 0.0
        for i, b in enumerate(sampled):
            Mb = M_h[b, :, :T[b]]
            xr, _, tol = GC.tier2_signal(n, x_h[b, :, :lens[b]], GC.weights_from_f32(wh[i]),
                                         GC.gain_of(Mb, "floor"))
            scale = 1.0 / (np.abs(xr).max() + GC.NORM_EPS) if norm == "peak" else 1.0
            e = np.abs(oh[i, :n_out_h[b]] - xr * scale).max() / (tol * scale)
            assert e <= 1, (b, int(T[b]), e)
            worst = max(worst, e)
        print(f"N={n} {norm}: {B} rows, {len(sampled)} sampled: largest fraction of the Tier 2 "
              f"bound {worst:.4f}; run to run bitwise")


# ----------------------------------------------------------------------------- 6. isolation
@pytest.mark.parametrize("pf,norm", [("floor", "none"), ("mul", "peak")])
@pytest.mark.parametrize("n", GC.SIZES)
def test_nan_in_one_mask_row_stays_there(gpu_device, n, pf, norm):
    bt, pl, res = _base(n, "mvdr", pf, norm, 0.0, gpu_device)
    b = next(i for i, (T, L) in enumerate(GC.rows(n)) if T == 41)
    mask = _mask(n, "A", gpu_device).clone()
    mask[b, 20, 37] = NAN   # a live entry of the row's second chunk
    r = _run_fused(pl, bt, mask, pf, check_path=False)
    others = torch.ones(bt.B, dtype=torch.bool, device=gpu_device)
    others[b] = False
    why = r.same_bits(res, rows=others)
    assert why is None, why
    assert not bool(torch.isfinite(r.out[b, :bt.n_out_h[b]]).all())
    assert bool(torch.isnan(r.out[b, bt.n_out_h[b]:]).all())
    print(f"N={n} {pf} {norm}: NaN in row {b}'s mask: peak[b] = {r.peak[b].item()}, "
          f"{int((~torch.isfinite(r.out[b, :bt.n_out_h[b]])).sum())} of {bt.n_out_h[b]} samples "
          f"non-finite")


@pytest.mark.parametrize("pf,norm", [("floor", "none"), ("mul", "peak")])
@pytest.mark.parametrize("n", GC.SIZES)
def test_short_row_between_live_rows_is_skipped(gpu_device, n, pf, norm):
    """A row shorter than a frame: `out` untouched, peak NaN, its (all-NaN) mask row never
    read; the live rows keep the bits they have beside a live row there."""
    bt, pl, res = _base(n, "mvdr", pf, norm, 0.0, gpu_device)
    b = 12
    lens = bt.lens.clone()
    lens[b] = n - 1
    mask = _mask(n, "A", gpu_device).clone()
    mask[b] = NAN
    x = bt.x.clone()
    x[b] = NAN
    r = _run_fused(pl, bt, mask, pf, check_path=False, x=x, lens=lens)
    others = torch.ones(bt.B, dtype=torch.bool, device=gpu_device)
    others[b] = False
    why = r.same_bits(res, rows=others)
    assert why is None, why
    assert bool(torch.isnan(r.out[b]).all()) and bool(torch.isnan(r.peak[b]))
