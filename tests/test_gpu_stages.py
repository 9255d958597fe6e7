"""GPU: the driver-side stage kernels against the fp64 references of tests/stage_cases.py.

1. MPDR: AVZ_MASK_ONES through avz_mvdr_batch / avz_mvdr_covariance / avz_solve_covariance /
   avz_apply_istft, both sizes, one ragged batch each (T = 3, 4, 5, 32, 33, 66).
2. avz_srp_scan: both sizes and two spacings, ragged, band edges on bins, 1 / 2 / 181 / 300
   angles, an angle range, any mask mode, the shared workspace, the degenerate maps.
3. avz_chunk_split / avz_chunk_merge through ctypes: scalar tails, misaligned rows, three
   covering chunks, gaps, the cross-block peak, the normalise pass.
4. avz_projection_metrics(_scaled): ragged rows on the float4 and the scalar path.
5. avz_mask_features against the fp64 restatement: both sizes and layouts, ragged.

Every output buffer is pre-filled with NaN. Every tolerance is one the project already uses
(test_gpu_parity.py, test_gpu_features.py, test_gpu_host.py) or is derived in stage_cases.py
from the fp64 reference and the number formats. Each test prints its largest deviation as a
fraction of its bound (pytest -s).

Measured on one MI355X on 2026-10-20, on the commit that adds this file (its parent is
2394597); the largest deviation of each section as a fraction of its bound (DESIGN.md
section 14):
  1. covariance sums 0.115 of 2e-6 max R00; weights < 0.0005 of 1e-3 max|W|; output 0.004 and
     peak 0.003 of 1e-4 max|ref|; stage chain against fused 0.238 of 1e-6; every bitwise
     identity held (batch against single runs, debug outputs, the external plan with M = 0).
  2. |dp| / tau at most 0.004 (d = 0.08 m; 0.001 at d = 0.01 m), at most 1.4e-8 dB at
     d = 0.01 m; other mask modes and the chain call around a scan: equal bits; the
     degenerate maps are NaN since this commit (-inf before it).
  3. split exact; merge bitwise equal to the fp32 transcription, 0.250 of 2^-23 sum|terms|
     from the fp64 one; normalised 0.340 of 2^-22 |y|.
  4. sums < 0.0005 of L 2^-53 sum|a b| on both paths; scaled metrics within 2.1e-14 dB.
  5. log-magnitude 0.021, IPD 0.034, sin / cos 0.029 of the propagated bounds; no branch-cut
     wrap occurred.
"""
import ctypes as ct

import numpy as np
import pytest
import torch

import stage_cases as SC
import train_cases as TC
from avz import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _p(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ----------------------------------------------------------------------------- 1. MPDR
OUT_PAD = 8

_MPDR_RUNS = {}


def _mpdr_plan(n, norm, mask="ones", B=6, S=None):
    import avz
    return avz.MVDRPlan(n_fft=n, sigma=SC.MPDR_SIGMA, mic_d=SC.MPDR_D, mask=mask,
                        postfilter="none", weight_eps=0.0, normalize=norm, norm_eps=0.0,
                        max_batch=B, max_samples=S)


def _mpdr_call(plan, x, lens, max_len, debug, ext_mask=None):
    """One avz_mvdr_batch into NaN-filled buffers: (out, peak, cov, w)."""
    B, dev = x.shape[0], x.device
    out = _nan((B, plan.out_len(max_len) + OUT_PAD), dev)
    peak = _nan((B,), dev)
    cov = _nan((B, plan.F, 5), dev, torch.float64) if debug else None
    w = _nan((B, plan.F, 4), dev) if debug else None
    plan.run(x, lens, max_len=max_len, ext_mask=ext_mask, out=out, peak=peak, cov_out=cov,
             w_out=w)
    torch.cuda.synchronize()
    return out, peak, cov, w


def _mpdr_runs(n, norm, dev):
    """Every run of one (size, normalisation), once: the ragged batch with and without the
    debug outputs, each item alone, the external plan with M = 0, the stage chain."""
    key = (n, norm)
    if key in _MPDR_RUNS:
        return _MPDR_RUNS[key]
    xh, lh = SC.mpdr_batch(n)
    B, S = len(lh), xh.shape[2]
    x, lens = _dev(xh, dev), _dev(lh, dev)
    plan = _mpdr_plan(n, norm, S=S)
    r = dict(plan=plan, lens=lh)
    r["debug"] = _mpdr_call(plan, x, lens, S, True)
    r["plain"] = _mpdr_call(plan, x, lens, S, False)
    r["single"] = []
    for b, L in enumerate(lh):
        L = int(L)
        xb = x[b:b + 1, :, :L].contiguous()
        r["single"].append(_mpdr_call(plan, xb, _dev(lh[b:b + 1], dev), L, False))
    ext = _mpdr_plan(n, norm, mask="external", S=S)
    M = torch.zeros((B, plan.F, plan.frames(S)), dtype=torch.float32, device=dev)
    r["external"] = _mpdr_call(ext, x, lens, S, True, ext_mask=M)
    cov = plan.covariance(x, lens, max_len=S, cov_out=_nan((B, plan.F, 5), dev, torch.float64))
    w = plan.solve_covariance(cov, w=_nan((B, plan.F, 4), dev))
    so, sp = plan.apply_istft(x, w, lens, max_len=S, out=_nan((B, plan.out_len(S) + OUT_PAD), dev),
                              peak=_nan((B,), dev))
    torch.cuda.synchronize()
    r["stages"] = (so, sp, cov, w)
    _MPDR_RUNS[key] = r
    return r


MPDR_CASES = [(n, norm) for n in SC.SIZES for norm in ("none", "peak")]


@pytest.mark.parametrize("n,norm", MPDR_CASES)
def test_mpdr_against_fp64(gpu_device, n, norm):
    r = _mpdr_runs(n, norm, gpu_device)
    out, peak, cov, w = (t.cpu().numpy() for t in r["debug"])
    H = n // 2
    worst = dict(cov=0.0, w=0.0, out=0.0, peak=0.0)
    for b, ref in enumerate(SC.mpdr_reference(n)):
        T, c = ref["T"], cov[b]
        assert (c[:, 4] == T).all(), b
        scale = ref["cov"][:, 0].max()
        e_cov = np.abs(c[:, :4] - ref["cov"][:, :4]).max() / (SC.COV_TOL * scale)
        Wg = np.stack([w[b, :, 0] + 1j * w[b, :, 1], w[b, :, 2] + 1j * w[b, :, 3]], 1)
        e_w = np.abs(Wg - ref["W"]).max() / (SC.W_TOL * np.abs(ref["W"]).max())
        n_out = (T - 1) * H
        assert len(ref["out"]) == n_out
        pk = np.abs(ref["out"]).max()
        want = ref["out"] / pk if norm == "peak" else ref["out"]
        e_out = np.abs(out[b, :n_out] - want).max() / (SC.WAVE_TOL * np.abs(want).max())
        e_pk = abs(float(peak[b]) - pk) / (SC.WAVE_TOL * pk)
        print(f"MPDR N={n} {norm} b={b} T={T}: cov {e_cov:.3f}, w {e_w:.3f}, out {e_out:.3f}, "
              f"peak {e_pk:.3f} of their bounds")
        assert e_cov <= 1 and e_w <= 1 and e_out <= 1 and e_pk <= 1, (b, e_cov, e_w, e_out, e_pk)
        assert np.isnan(out[b, n_out:]).all(), b   # nothing written past (T - 1) H
        for k, v in (("cov", e_cov), ("w", e_w), ("out", e_out), ("peak", e_pk)):
            worst[k] = max(worst[k], float(v))
    print(f"MPDR N={n} {norm}: largest fraction of the bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("n,norm", MPDR_CASES)
def test_mpdr_bitwise_identities(gpu_device, n, norm):
    r = _mpdr_runs(n, norm, gpu_device)
    out, peak, cov, w = r["debug"]
    H = n // 2
    # the unfused solve (debug outputs) against the fused run, sentinels included
    assert _same_bits(out, r["plain"][0]) and _same_bits(peak, r["plain"][1])
    # the ragged batch against each item alone
    for b, L in enumerate(r["lens"]):
        n_out = (SC.n_frames(int(L), n) - 1) * H
        o1, p1, _, _ = r["single"][b]
        assert _same_bits(out[b, :n_out], o1[0, :n_out]), b
        assert _same_bits(peak[b:b + 1], p1), b
        assert bool(torch.isnan(o1[0, n_out:]).all()), b
    # an external plan with M = 0 (noise weight 1 - 0, weight_eps 0, no post-filter)
    oe, pe, ce, we = r["external"]
    assert _same_bits(out, oe) and _same_bits(peak, pe)
    assert _same_bits(cov, ce) and _same_bits(w, we)


@pytest.mark.parametrize("n,norm", MPDR_CASES)
def test_mpdr_stage_chain_equals_fused(gpu_device, n, norm):
    """covariance -> solve_covariance -> apply_istft against the fused call: equal weights and
    outputs within 1e-6 of the output's scale (test_stagewise_chain_equals_fused's bound, set
    there on a peak-normalised output)."""
    r = _mpdr_runs(n, norm, gpu_device)
    out, peak, cov, w = r["debug"]
    so, sp, scov, sw = r["stages"]
    assert _same_bits(scov, cov) and _same_bits(sw, w)
    worst = 0.0
    for b, L in enumerate(r["lens"]):
        n_out = (SC.n_frames(int(L), n) - 1) * (n // 2)
        scale = 1.0 if norm == "peak" else float(out[b, :n_out].abs().max())
        d = float((so[b, :n_out] - out[b, :n_out]).abs().max()) / (1e-6 * scale)
        worst = max(worst, d)
        assert d <= 1, (b, d)
        assert abs(float(sp[b]) - float(peak[b])) <= 1e-6 * float(peak[b])
        assert bool(torch.isnan(so[b, n_out:]).all()), b
    print(f"MPDR N={n} {norm}: stage chain vs fused, largest fraction of the bound {worst:.3f}")


# ----------------------------------------------------------------------------- 2. SRP
def _srp(plan, x, lens, max_len, n_angles=181, lo=0.0, hi=180.0, f_lo=200.0, f_hi=4000.0):
    """avz_srp_scan into a NaN-filled buffer with 8 spare doubles: [B, n_angles] numpy."""
    B = x.shape[0]
    out = _nan((B * n_angles + 8,), x.device, torch.float64)
    rc = _lib.lib.avz_srp_scan(plan._h, B, _p(lens), int(max_len), _p(x), x.stride(0),
                               x.stride(1), n_angles, lo, hi, f_lo, f_hi, _p(out), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[B * n_angles:]).all()
    return o[:B * n_angles].reshape(B, n_angles)


def _srp_plan(n, d, S, mask="ones", B=4):
    import avz
    return avz.MVDRPlan(n_fft=n, mic_d=d, mask=mask, postfilter="ibm" if mask == "ibm" else "none",
                        max_batch=B, max_samples=S)


SRP_CALLS = ([dict(f_lo=lo, f_hi=hi) for lo, hi in (SC.SRP_BAND_ON_BINS, SC.SRP_BAND_DEFAULT)] +
             [dict(n_angles=k, f_lo=SC.SRP_BAND_ON_BINS[0], f_hi=SC.SRP_BAND_ON_BINS[1])
              for k in (1, 2, 300)] +
             [dict(n_angles=121, lo=30.0, hi=150.0)])


@pytest.mark.parametrize("n", SC.SIZES)
@pytest.mark.parametrize("d", SC.SRP_SPACINGS)
def test_srp_against_fp64(gpu_device, n, d):
    xh, lh = SC.srp_batch(n, d)
    S = xh.shape[2]
    x, lens = _dev(xh, gpu_device), _dev(lh, gpu_device)
    plan = _srp_plan(n, d, S)
    worst = 0.0
    for kw in SRP_CALLS:
        P = _srp(plan, x, lens, S, **kw)
        assert np.isnan(P[3]).all()              # shorter than a frame: not scanned
        for b in range(3):
            _, ref, tau = SC.srp_reference(
                xh[b, :, :int(lh[b])], n, d, f_lo=kw.get("f_lo", 200.0),
                f_hi=kw.get("f_hi", 4000.0), n_angles=kw.get("n_angles", 181),
                angle_lo=kw.get("lo", 0.0), angle_hi=kw.get("hi", 180.0))
            assert np.isfinite(P[b]).all() and P[b].max() == 0.0
            if kw.get("n_angles") == 1:
                assert P[b].tolist() == [0.0]
            frac = np.abs(10 ** (P[b] / 10) - 10 ** (ref / 10)).max() / tau
            print(f"SRP N={n} d={d} b={b} {kw}: |dp| / tau = {frac:.3f} "
                  f"(max |d dB| {np.abs(P[b] - ref).max():.1e})")
            assert frac <= 1, (kw, b, frac)
            worst = max(worst, float(frac))
    print(f"SRP N={n} d={d}: largest |dp| / tau {worst:.3f}")


@pytest.mark.parametrize("n", SC.SIZES)
def test_srp_mask_mode_and_shared_workspace(gpu_device, n):
    d = 0.08
    xh, lh = SC.srp_batch(n, d)
    S = xh.shape[2]
    x, lens = _dev(xh, gpu_device), _dev(lh, gpu_device)
    want = _srp(_srp_plan(n, d, S), x, lens, S)
    ibm = _srp_plan(n, d, S, "ibm")
    for plan in (ibm, _srp_plan(n, d, S, "ipd")):
        got = _srp(plan, x, lens, S)
        assert np.array_equal(got.view(np.int64), want.view(np.int64))
    # the scan uses the plan's workspace: a chain call before and after it gives equal bits
    x3, l3 = x[:3].contiguous(), lens[:3].contiguous()
    tgt, itf = x3[:, 0].contiguous(), x3[:, 1].contiguous()

    def chain():
        out = _nan((3, ibm.out_len(S) + OUT_PAD), gpu_device)
        peak = _nan((3,), gpu_device)
        ibm.run(x3, l3, max_len=S, ref_tgt=tgt, ref_int=itf, out=out, peak=peak)
        torch.cuda.synchronize()
        return out, peak
    o0, p0 = chain()
    mid = _srp(ibm, x, lens, S)
    o1, p1 = chain()
    assert _same_bits(o0, o1) and _same_bits(p0, p1)
    assert np.array_equal(mid.view(np.int64), want.view(np.int64))
    assert bool(torch.isfinite(p0).all())


@pytest.mark.parametrize("n", SC.SIZES)
def test_srp_degenerate_maps_are_nan(gpu_device, n):
    """All scanned powers 0: -inf - (-inf) = NaN in every angle, as debug_srp.py:61-62 and
    oracle.srp_scan give; the other row of the same call is unaffected."""
    d = 0.08
    xh, lh = SC.srp_batch(n, d)
    L = int(lh[2])
    x2 = np.zeros((2, 2, L), np.float32)
    x2[1] = xh[2, :, :L]
    x, lens = _dev(x2, gpu_device), _dev(np.array([L, L], np.int32), gpu_device)
    plan = _srp_plan(n, d, L, B=2)
    P = _srp(plan, x, lens, L)
    _, ref, tau = SC.srp_reference(x2[1], n, d)
    assert np.isnan(P[0]).all()
    assert np.abs(10 ** (P[1] / 10) - 10 ** (ref / 10)).max() <= tau
    for k in (1, 181, 300):
        P = _srp(plan, x, lens, L, n_angles=k, f_lo=SC.SRP_BAND_EMPTY[0], f_hi=SC.SRP_BAND_EMPTY[1])
        assert np.isnan(P).all(), k
    assert np.isnan(SC.srp_reference(x2[0], n, d)[1]).all()
    assert np.isnan(SC.srp_reference(x2[1], n, d, *SC.SRP_BAND_EMPTY)[1]).all()


# ----------------------------------------------------------------------------- 3. chunks
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("ch_stride", SC.SPLIT_ITEM_CH_STRIDES)
def test_chunk_split_exact(gpu_device, channels, ch_stride):
    xh = SC.split_input(channels)
    ref = SC.split_reference(xh, SC.SPLIT_LENS, SC.SPLIT_ITEMS, SC.SPLIT_CHUNK)
    n_items, chunk = len(SC.SPLIT_ITEMS), SC.SPLIT_CHUNK
    x = _dev(xh, gpu_device)
    utt = _dev(np.array([u for u, _ in SC.SPLIT_ITEMS], np.int32), gpu_device)
    start = _dev(np.array([s for _, s in SC.SPLIT_ITEMS], np.int32), gpu_device)
    lens = _dev(np.array(SC.SPLIT_LENS, np.int32), gpu_device)
    items = _nan((n_items, channels, ch_stride), gpu_device)
    assert items.data_ptr() % 16 == 0
    rc = _lib.lib.avz_chunk_split(n_items, channels, chunk, _p(utt), _p(start), _p(lens), _p(x),
                                  x.stride(0), x.stride(1), _p(items), items.stride(0),
                                  items.stride(1), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = items.cpu().numpy()
    assert np.array_equal(got[:, :, :chunk].view(np.int32), ref.view(np.int32))
    assert np.isnan(got[:, :, chunk:]).all()
    print(f"split channels={channels} item_ch_stride={ch_stride}: exact, "
          f"{int(np.isnan(got).sum())} sentinels kept")


def _merge(io, lens, base, hop, iol, max_len, normalize, eps, dev, peak_fill):
    B = len(lens)
    y = _nan((B, max_len + 3), dev)
    peak = _dev(np.array(peak_fill, np.float32), dev)
    d_io, d_len, d_base = _dev(io, dev), _dev(lens, dev), _dev(base, dev)
    rc = _lib.lib.avz_chunk_merge(B, max_len, hop, iol, _p(d_len), _p(d_base), _p(d_io),
                                  d_io.stride(0), _p(y), y.stride(0), _p(peak), normalize, eps,
                                  None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y.cpu().numpy(), peak.cpu().numpy()


GARBAGE = (1e30, NAN, -5.0, 7.0)


@pytest.mark.parametrize("hop,iol,max_len", SC.MERGE_SETS)
def test_chunk_merge_sum_count_and_peak(gpu_device, hop, iol, max_len):
    io, lens, base = SC.merge_case(hop, iol, max_len)
    y32, pk32 = SC.merge_reference_f32(io, lens, base, hop, iol)
    y64, mag = SC.merge_reference_f64(io, lens, base, hop, iol)
    assert io.shape[1] > iol and max_len + 3 > max_len
    y, peak = _merge(io, lens, base, hop, iol, max_len, 0, 0.0, gpu_device, GARBAGE)
    worst = 0.0
    for u, L in enumerate(lens):
        assert np.array_equal(y[u, :L].view(np.int32), y32[u].view(np.int32)), u
        assert np.isnan(y[u, L:]).all(), u
        assert peak[u] == np.abs(y[u, :L]).max() == pk32[u], u
        err = np.abs(y[u, :L].astype(np.float64) - y64[u])
        assert (err <= 2.0 ** -23 * mag[u]).all(), u
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(mag[u] > 0, err / (2.0 ** -23 * mag[u]), 0))))
    # a NaN in one utterance's items stays there
    bad = io.copy()
    bad[base[0] + 1, 2] = NAN
    yb, pb = _merge(bad, lens, base, hop, iol, max_len, 0, 0.0, gpu_device, GARBAGE)
    assert np.isnan(yb[0, :lens[0]]).any()
    for u in range(1, len(lens)):
        assert np.array_equal(yb[u].view(np.int32), y[u].view(np.int32)), u
        assert pb[u:u + 1].view(np.int32) == peak[u:u + 1].view(np.int32), u
    # the normalise pass: three roundings (peak + eps, the reciprocal, the product)
    worst_n = 0.0
    for eps in (1e-9, 0.0):
        yn, pn = _merge(io, lens, base, hop, iol, max_len, 1, eps, gpu_device, GARBAGE)
        assert np.array_equal(pn.view(np.int32), peak.view(np.int32))
        for u, L in enumerate(lens):
            want = y32[u].astype(np.float64) / (float(pk32[u]) + eps)
            err = np.abs(yn[u, :L] - want)
            assert (err <= 2.0 ** -22 * np.abs(want)).all(), (eps, u)
            assert np.isnan(yn[u, L:]).all(), (eps, u)
            nz = want != 0
            worst_n = max(worst_n, float((err[nz] / (2.0 ** -22 * np.abs(want[nz]))).max()))
    print(f"merge hop={hop} item_out_len={iol} max_len={max_len}: fp32 sum bitwise; vs fp64 "
          f"{worst:.3f} of 2^-23 sum|terms|; normalised {worst_n:.3f} of 2^-22 |y|")


# ----------------------------------------------------------------------------- 4. metrics
def _metrics(o, t, i, lens, dev, offset, peaks=None, eps=0.0):
    """avz_projection_metrics(_scaled) on rows at MET_STRIDE whose bases sit `offset` floats
    past a 16-byte boundary: (sums [B, 6], metrics [B, 4])."""
    B, stride = o.shape
    rows = []
    for a in (o, t, i):
        buf = torch.zeros(B * stride + 4, dtype=torch.float32, device=dev)
        v = buf[offset:offset + B * stride]
        v.copy_(torch.from_numpy(a.reshape(-1)))
        assert v.data_ptr() % 16 == 4 * offset
        rows.append(v)
    d_len = _dev(np.array(lens, np.int32), dev)
    sums = _nan((B, 6), dev, torch.float64)
    met = _nan((B, 4), dev, torch.float64)
    L = max(lens)
    if peaks is None:
        rc = _lib.lib.avz_projection_metrics(B, L, _p(d_len), _p(rows[0]), stride, _p(rows[1]),
                                             stride, _p(rows[2]), stride, _p(sums), _p(met), None)
    else:
        pk = _dev(np.array(peaks, np.float32), dev)
        rc = _lib.lib.avz_projection_metrics_scaled(B, L, _p(d_len), _p(rows[0]), stride, _p(pk),
                                                    eps, _p(rows[1]), stride, _p(rows[2]), stride,
                                                    _p(sums), _p(met), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return sums.cpu().numpy(), met.cpu().numpy()


def test_projection_metrics_both_paths(gpu_device):
    o, t, i = SC.metrics_inputs()
    runs = {off: _metrics(o, t, i, SC.MET_LENS, gpu_device, off) for off in (0, 1)}
    worst = 0.0
    for b, L in enumerate(SC.MET_LENS):
        s, bound = SC.metrics_sums(o[b, :L], t[b, :L], i[b, :L])
        ref = SC.metrics_reference(o[b, :L], t[b, :L], i[b, :L])
        for off, (sums, met) in runs.items():
            assert (np.abs(sums[b] - s) <= bound).all(), (off, b)
            np.testing.assert_allclose(met[b], ref, rtol=1e-9, atol=1e-9)
            if L:
                worst = max(worst, float((np.abs(sums[b] - s) / bound).max()))
        assert (np.abs(runs[0][0][b] - runs[1][0][b]) <= bound).all(), b
        if L == 0:
            assert (runs[0][1][b] == -np.inf).all() and (runs[1][1][b] == -np.inf).all()
    print(f"metrics: sums within {worst:.3f} of L 2^-53 sum|a b| on both paths")


@pytest.mark.parametrize("eps", SC.MET_EPS)
def test_projection_metrics_scaled_against_fp64(gpu_device, eps):
    o, t, i = SC.metrics_inputs()
    worst = 0.0
    for off in (0, 1):
        sums, met = _metrics(o, t, i, SC.MET_LENS, gpu_device, off, peaks=SC.MET_PEAKS, eps=eps)
        for b, L in enumerate(SC.MET_LENS):
            ref = SC.metrics_reference(o[b, :L], t[b, :L], i[b, :L], peak=SC.MET_PEAKS[b], eps=eps)
            np.testing.assert_allclose(met[b], ref, rtol=1e-9, atol=1e-9)
            # the sums stay those of the un-scaled signals
            s, bound = SC.metrics_sums(o[b, :L], t[b, :L], i[b, :L])
            assert (np.abs(sums[b] - s) <= bound).all(), (off, b)
            if L:
                worst = max(worst, float(np.abs(met[b] - ref).max()))
    print(f"scaled metrics eps={eps}: largest |d dB| {worst:.2e} (bound 1e-9 + 1e-9 |ref|)")


# ----------------------------------------------------------------------------- 5. features
LAYOUTS = {"unet": _lib.FEAT_LOGMAG_IPD, "tflite": _lib.FEAT_TFLITE}
PAD_T, PAD_S = 5, 96

_FEAT_PLANS = {}


def _feat_plan(n):
    import avz
    if n not in _FEAT_PLANS:
        _FEAT_PLANS[n] = avz.MVDRPlan(n_fft=n, mask="external", postfilter="none", max_batch=3,
                                      max_samples=TC.S)
    return _FEAT_PLANS[n]


def _features(n, name, layout, padded, scale, dev):
    """avz_mask_features into a NaN-filled buffer: [B, C, F, T(+PAD_T)] numpy."""
    mix_h, lens_h = SC.feature_batch(n, name, scale)
    B, _, S = mix_h.shape
    mix = torch.zeros((B, 2, S + (PAD_S if padded else 0)), dtype=torch.float32, device=dev)
    mix[:, :, :S] = torch.from_numpy(mix_h)
    lens = _dev(lens_h, dev)
    max_len = int(lens_h.max())
    F, T = n // 2 + 1, SC.n_frames(max_len, n)
    Tp = T + (PAD_T if padded else 0)
    if layout == "unet":
        feat = _nan((B, 2, F, Tp), dev)
        sb, sc, sf, st = feat.stride()
    else:
        feat = _nan((B, F, Tp, 4), dev)
        sb, sf, st, sc = feat.stride()
    rc = _lib.lib.avz_mask_features(_feat_plan(n)._h, LAYOUTS[layout], B, _p(lens), max_len,
                                    _p(mix), mix.stride(0), mix.stride(1), _p(feat), sb, sc, sf,
                                    st, None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return (feat if layout == "unet" else feat.permute(0, 3, 1, 2)).cpu().numpy()


FEAT_CASES = [(n, name, layout, padded, scale) for n in SC.SIZES for name in ("A", "B")
              for layout in ("unet", "tflite") for padded in (False, True)
              for scale in SC.FEAT_NOISE_SCALES]


@pytest.mark.parametrize("n,name,layout,padded,scale", FEAT_CASES)
def test_mask_features_against_fp64(gpu_device, n, name, layout, padded, scale):
    ft = _features(n, name, layout, padded, scale, gpu_device)
    lens = SC.feature_batch(n, name, scale)[1]
    F = n // 2 + 1
    worst = dict(lm=0.0, ipd=0.0, sc=0.0)
    wraps = 0
    for b, r in enumerate(SC.feature_reference(n, name, scale)):
        if r is None:
            assert np.isnan(ft[b]).all()   # shorter than a frame: untouched
            continue
        T = SC.n_frames(int(lens[b]), n)
        assert np.isnan(ft[b, :, :, T:]).all() and not np.isnan(ft[b, :, :, :T]).any()
        Y, ref_lm, ref_ipd = r["Y"], r["feat"][0], r["feat"][1]
        if scale == SC.FEAT_CAPPED_SCALE:
            assert (r["tol_ipd"] > SC.FEAT_IPD_LOOSE).mean() <= SC.FEAT_CAP
        e_lm = np.abs(ft[b, 0, :, :T] - ref_lm) / r["tol_lm"]
        assert (e_lm <= 1).all(), (b, e_lm.max())
        worst["lm"] = max(worst["lm"], float(e_lm.max()))
        near = (np.abs(Y[0].imag) <= r["d_abs"]) | (np.abs(Y[1].imag) <= r["d_abs"])
        if layout == "unet":
            d = ft[b, 1, :, :T] - ref_ipd
            wrapped = np.abs(np.abs(d) - 2 * np.pi) < 1e-3
            e = np.abs(d) / r["tol_ipd"]
            assert ((e <= 1) | wrapped).all(), (b, e[~wrapped].max())
            assert near[wrapped].all()     # every 2 pi jump sits on the branch cut
            wraps += int(wrapped.sum())
            worst["ipd"] = max(worst["ipd"], float(e[~wrapped].max()))
        else:
            tol = r["tol_ipd"] + 2e-6
            e_s = np.abs(ft[b, 1, :, :T] - np.sin(ref_ipd)) / tol
            e_c = np.abs(ft[b, 2, :, :T] - np.cos(ref_ipd)) / tol
            assert (e_s <= 1).all() and (e_c <= 1).all(), (b, e_s.max(), e_c.max())
            worst["sc"] = max(worst["sc"], float(e_s.max()), float(e_c.max()))
            lin = np.linspace(0, 1, F, dtype=np.float32)
            assert np.array_equal(ft[b, 3, :, :T], np.tile(lin[:, None], (1, T)))
    print(f"features N={n} {name} {layout} padded={padded} noise x{scale}: largest fraction of "
          f"the bound log-mag {worst['lm']:.3f}, ipd {worst['ipd']:.3f} ({wraps} wraps on the "
          f"cut), sin/cos {worst['sc']:.3f}")
