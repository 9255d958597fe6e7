"""GPU: the IPD mask decisions of the analysis kernel (csrc/avz_chain_analysis.hpp, MASK_IPD)
on silent, identical and colinear channel pairs, against the rows, fp64 references and bounds of
tests/ipd_cases.py (its docstring has the row table and the derivation of the sums' bound).

Sixteen rows a size -- a Gaussian control; one channel +0, -0.0 (x 0) or dead on a span; both
channels silent on spans; identical channels everywhere and on spans that put identical frames
at frame 0, at the last frame, on both sides of a step and of the chunk boundary and alone
between others; ch1 = -ch0; ch1 = +-(ch0 + 1e-4 noise); the control at 2^-56, 2^-20, 2^20,
2^48; a four-frame row -- in three layouts that between them run both instances of the kernel:
`pieces` (every item in 4 step-range pieces: the SPLIT instance), `whole` (chunks x rows = the
resident grid: the unsplit instance, 16 or 24 copies of each row in different blocks) and
`mixed` (one full grid of whole items, then the rows as a split tail, in one launch). The
configuration is the goldens' (utt_cases.PLANS["ipd"]); out, peak and cov_out are pre-filled
with NaN.

  1. counts: cov_out[b, :, 4] equals the row sums of the oracle's mask in every bin of every
     row and copy (no decision differs: round(|d| / 0.99) == 0, the residual within 1e-6
     relative as in test_ipd_identical_channels); in `near` alone a bin may deviate by at most
     its number of tie cells (0 < |d angle| < 1e-6 rad in fp64);
  2. sums: cov_out[b, :, 0:4] against the fp64 sums over the oracle's spectra within
     ipd_cases' derived per-bin bound (at most 1e-4 of max(c00, c11) of the bin; test_ipd_
     reference.py), `near`'s tie-holding bins excluded;
  3. waveform: the rows whose reference solve is well conditioned (cond_2 <= 100 in every
     solved bin at sigma 1e-7: gauss, ch1_dead_span, both_zero_span, ident_spans and the four
     level rows) against O.masked_mvdr_vec at 1e-4, nothing written past (T - 1) H;
  4. across layouts: a row's decisions are the same in every layout and copy, its sums agree
     within 2e-6 (utt_cases.SPLIT_TOL: a changed association of the fp32 partials) of the bin's
     unweighted max(sum |Y0|^2, sum |Y1|^2), the magnitude the fp32 accumulators hold before
     the fix-up takes 0.99 p back out;
  5. stage export: plan.covariance of the `pieces` batches is bitwise the cov_out of plan.run.

Each test prints its largest deviation as a fraction of its bound (pytest -s); the measured
table is DESIGN.md section 22.

Measured on one MI355X (256 CUs) on 2026-10-21, on the commit that adds this file (its parent
is ec441d5; no kernel changed): no defect in the kernel's five pieces. Every
decision of every row and copy equals the oracle's (16 rows in `pieces`, 256 / 384 in `whole`,
272 / 400 in `mixed` at N = 1024 / 512) but for 4 (N = 1024) and 1 (N = 512) on `near`'s tie
cells and for one cell that test_counts_on_zero_sign_rows keeps as a strict xfail: bin 205 of
`short_zero`'s last frame at N = 512, 3.01 against the reference's 4.0 in every layout, where
the reference follows the sign of a pocketfft zero. Largest fractions of the bounds: weight-sum
residual 0.120 of 1e-6; sums 0.170 of the derived bound (`ident_all`; every other row at most
0.058; the bound itself at most 6.7e-5 of max(c00, c11)); waveform and peak 0.0048 of 1e-4;
across layouts 0.150 of 2e-6; the stage export bitwise. 22 passed, 3 xfailed in 2.5 s, the
slowest test 0.33 s.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

import ipd_cases as IC
import stage_cases as SC
import utt_cases as UC
from conftest import PKG

pytestmark = pytest.mark.gpu

NAN = float("nan")
OUT_PAD = 8
COUNT_RTOL = 1e-6   # test_ipd_identical_channels
CASES = [(lay, n) for lay in IC.LAYOUTS for n in IC.SIZES]


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _plan(n, B, S):
    import avz
    return avz.MVDRPlan(n_fft=n, max_batch=B, max_samples=S, **IC.PLAN)


def _check_grid(n):
    """ipd_cases' layouts assume the analysis kernel's blocks per CU: read them as
    test_gpu_ibm_exact_edges.analysis_grid does."""
    src = open(os.path.join(PKG, "csrc", "avz_common.hpp")).read()
    body = src.split(f"struct KCfg<{n}>", 1)[1]
    assert int(re.search(r"\bBLOCKS_PER_CU = (\d+);", body).group(1)) == UC.BLOCKS_PER_CU[n]


class Run:
    """One batch of a layout through plan.run: cov [B, F, 5] and out [B, n_out + pad] on the
    host, the device inputs kept for the stage export."""

    def __init__(self, n, names, dev):
        self.n, self.names = n, names
        mix, lens = IC.batch(n, names)
        self.B, self.S, self.max_len = len(names), mix.shape[2], int(lens.max())
        self.mix, self.lens = _dev(mix, dev), _dev(lens, dev)
        self.plan = pl = _plan(n, self.B, self.S)
        out = torch.full((self.B, pl.out_len(self.max_len) + OUT_PAD), NAN, device=dev)
        peak = torch.full((self.B,), NAN, device=dev)
        self.cov_d = torch.full((self.B, pl.F, 5), NAN, dtype=torch.float64, device=dev)
        pl.run(self.mix, self.lens, max_len=self.max_len, out=out, peak=peak, cov_out=self.cov_d)
        torch.cuda.synchronize()
        self.cov, self.out, self.peak = self.cov_d.cpu().numpy(), out.cpu().numpy(), peak.cpu().numpy()

    def rows(self, name):
        return [b for b, k in enumerate(self.names) if k == name]


@functools.lru_cache(maxsize=None)
def _runs(layout, n, dev):
    _check_grid(n)
    R = _cus(dev)
    batches = IC.layout(layout, R, n)
    G = IC.grid(R, n)
    for names in batches:   # the instance each batch launches (csrc/avz_chunked.hip analysis_tail)
        whole, P = IC.split_of(len(names), R, n)
        assert {"pieces": (whole, P) == (0, 4), "whole": (whole, P) == (G, 1),
                "mixed": whole == G and P >= 2}[layout], (layout, len(names), whole, P)
    return [Run(n, names, dev) for names in batches]


def _instances(runs, name):
    """(run, row) of every copy of a row in a layout's batches."""
    return [(r, b) for r in runs for b in r.rows(name)]


def _decisions(got, ref):
    """Differing decisions per bin and the residual of the weight sum once they are taken out."""
    d = np.abs(got - ref)
    flips = np.round(d / 0.99)
    return flips, np.abs(d - 0.99 * flips)


# ----------------------------------------------------------------------------- 1. counts
@pytest.mark.parametrize("layout,n", CASES)
def test_counts(gpu_device, layout, n):
    runs = _runs(layout, n, gpu_device)
    worst, copies, near_flips, zero_sign = 0.0, 0, 0, 0
    for name in IC.ROWS:
        ref = IC.reference(n, name)
        allowed = ref["ties"].sum(axis=1) if name == "near" else np.zeros(n // 2 + 1)
        for k, _ in IC.ZERO_SIGN.get((n, name), ()):   # test_counts_on_zero_sign_rows holds these
            allowed[k] += 1
        inst = _instances(runs, name)
        assert inst, name
        for r, b in inst:
            got = r.cov[b, :, 4]
            assert np.isfinite(got).all(), (name, b)
            flips, resid = _decisions(got, ref["rowsum"])
            bad = np.nonzero(flips > allowed)[0]
            assert len(bad) == 0, (layout, name, b, bad[:8].tolist(), flips[bad[:8]].tolist(),
                                   got[bad[:8]].tolist(), ref["rowsum"][bad[:8]].tolist())
            frac = float((resid / (COUNT_RTOL * ref["rowsum"])).max())
            assert frac <= 1, (layout, name, b, frac)
            worst = max(worst, frac)
            near_flips = max(near_flips, int(flips.sum())) if name == "near" else near_flips
            zero_sign += int(flips.sum()) if (n, name) in IC.ZERO_SIGN else 0
            copies += 1
    print(f"{layout} N={n}: {copies} rows, no differing decision but {near_flips} on `near`'s tie "
          f"cells and {zero_sign} on zero-sign cells (ipd_cases.ZERO_SIGN); weight-sum residual "
          f"{worst:.4f} of {COUNT_RTOL:g} relative")


@pytest.mark.parametrize("layout", IC.LAYOUTS)
@pytest.mark.parametrize("n,name", [pytest.param(n, k, marks=pytest.mark.xfail(
    strict=True, reason="the reference's decision follows the sign of a pocketfft zero"))
    for n, k in sorted(IC.ZERO_SIGN)])
def test_counts_on_zero_sign_rows(gpu_device, layout, n, name):
    """Check 1 in full on the rows of ipd_cases.ZERO_SIGN, which test_counts allows their
    zero-sign cells. N = 512 `short_zero`: the last frame is [-0, +0, ...] after the window's zero
    in ch0 and +0 in ch1; pocketfft gives bin 205 a -0 real part (angle pi, weight 1.0), the
    kernel gives the frame 0.01 in every bin as the reference does in the other 256: 3.01
    against 4.0 in that bin, in every layout. Silence in both channels made of mixed-sign zeros
    is not pinned."""
    ref = IC.reference(n, name)
    for r, b in _instances(_runs(layout, n, gpu_device), name):
        flips, _ = _decisions(r.cov[b, :, 4], ref["rowsum"])
        assert not flips.any(), (layout, name, b, np.nonzero(flips)[0].tolist())


# ----------------------------------------------------------------------------- 2. sums
@pytest.mark.parametrize("layout,n", CASES)
def test_sums(gpu_device, layout, n):
    runs = _runs(layout, n, gpu_device)
    worst = {}
    for name in IC.ROWS:
        ref = IC.reference(n, name)
        use = ~ref["ties"].any(axis=1) if name == "near" else np.ones(n // 2 + 1, bool)
        w = 0.0
        for r, b in _instances(runs, name):
            got = r.cov[b, :, :4]
            assert np.isfinite(got).all(), (name, b)
            frac = np.abs(got - ref["sums"])[use] / ref["bound"][use]
            k, q = np.unravel_index(np.argmax(frac), frac.shape)
            assert frac.max() <= 1, (layout, name, b, int(np.nonzero(use)[0][k]), int(q),
                                     float(frac.max()))
            w = max(w, float(frac.max()))
        worst[name] = w
    print(f"{layout} N={n}: sums, largest fraction of the bound {max(worst.values()):.4f}; " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ----------------------------------------------------------------------------- 3. waveform
@pytest.mark.parametrize("layout,n", CASES)
def test_waveform(gpu_device, layout, n):
    runs = _runs(layout, n, gpu_device)
    H = n // 2
    well = [k for k in IC.ROWS if IC.reference(n, k)["well"]]
    assert "gauss" in well and len(well) >= 4, well
    worst = {}
    for name in IC.ROWS:
        ref = IC.reference(n, name)
        n_out = (ref["mask"].shape[1] - 1) * H
        assert len(ref["out"]) == n_out
        w = 0.0
        for r, b in _instances(runs, name):
            assert np.isnan(r.out[b, n_out:]).all(), (name, b)   # nothing past (T - 1) H
            if name not in well:
                continue
            got = r.out[b, :n_out].astype(np.float64)
            e = float(np.abs(got - ref["out"]).max()) / SC.WAVE_TOL
            e_pk = abs(float(r.peak[b]) - ref["peak"]) / (UC.PEAK_RTOL * ref["peak"])
            assert e <= 1 and e_pk <= 1, (layout, name, b, e, e_pk)
            w = max(w, e, e_pk)
        if name in well:
            worst[name] = w
    print(f"{layout} N={n}: waveform and peak, largest fraction of the bound "
          f"{max(worst.values()):.4f}; " + ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))


# ----------------------------------------------------------------------------- 4. layouts
@pytest.mark.parametrize("n", IC.SIZES)
def test_across_layouts(gpu_device, n):
    runs = {lay: _runs(lay, n, gpu_device) for lay in IC.LAYOUTS}
    worst = 0.0
    for name in IC.ROWS:
        a = np.abs(IC.reference(n, name)["Y"].astype(np.complex128)) ** 2
        scale = np.maximum(a[0].sum(axis=1), a[1].sum(axis=1))   # unweighted
        inst = [x for lay in IC.LAYOUTS for x in _instances(runs[lay], name)]
        assert len(inst) >= 4, name
        r0, b0 = inst[0]
        for r, b in inst[1:]:
            flips, resid = _decisions(r.cov[b, :, 4], r0.cov[b0, :, 4])
            assert not flips.any(), (name, b, np.nonzero(flips)[0][:8].tolist())
            assert (resid <= COUNT_RTOL * r0.cov[b0, :, 4]).all(), (name, b)
            frac = float((np.abs(r.cov[b, :, :4] - r0.cov[b0, :, :4]) /
                          (UC.SPLIT_TOL * scale[:, None])).max())
            assert frac <= 1, (name, b, frac)
            worst = max(worst, frac)
    print(f"N={n}: a row's sums across layouts and copies: {worst:.4f} of {UC.SPLIT_TOL:g} of "
          "the bin's unweighted sums; the decisions equal")


# ----------------------------------------------------------------------------- 5. stage export
@pytest.mark.parametrize("n", IC.SIZES)
def test_stage_export_bitwise(gpu_device, n):
    for r in _runs("pieces", n, gpu_device):
        cov = torch.full((r.B, r.plan.F, 5), NAN, dtype=torch.float64, device=gpu_device)
        r.plan.covariance(r.mix, r.lens, max_len=r.max_len, cov_out=cov)
        torch.cuda.synchronize()
        assert torch.equal(cov.view(torch.int64), r.cov_d.view(torch.int64))
