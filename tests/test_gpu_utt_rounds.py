"""GPU: the whole-round per-utterance synthesis kernels (csrc/avz_chain_utt.hpp) on ragged
batches, against the fp64 references and layouts of tests/utt_cases.py.

First layout (B = 3 #CU, every block runs three rows whose lengths follow g mod 8: long after
short, skipped rows first / between / last, a block with no live row, step edges), four plans
(IBM + IBM post-filter, IPD, external mask and all-ones mask without a post-filter), both
sizes, all peak-normalised:
  1. sampled rows of the default path against fp64: waveform, SIR (IBM), peak;
  2. every live row peaks at peak / (peak + eps), writes (T - 1) H samples, has a peak > 0;
  3. every skipped row leaves `out` untouched and reports peak = NaN, on all three paths;
  4. synth_variant 1 (per-utterance kernel after the solve kernel) bitwise equal to 2;
  5. synth_variant 0 (chunk grid + finalize) within the parity tolerance of 2 and of fp64;
  6. the rows permuted to other blocks and rounds give the same bits; a NaN sample in one row
     leaves every other row's bits;
  7. run to run, bitwise.
Second layout (B = #CU rows of up to five chunks, N = 1024: the analysis splits the last R
items, row b* straddles the split): 1-5 and 7 on its sampled rows, and the rows from b* on
against the same rows in a batch of 2 #CU rows that has no split (2e-6).

Every test first asserts, from the plan's kernel timing, which kernels its launch ran
(utt_cases.assert_path), so a change of the dispatch cannot leave these tests vacuous. `out` is
pre-filled with NaN and `peak` with 7. Tolerances: BASELINE.md section 4 / test_gpu_parity.py
(1e-4 waveform, 0.01 dB SIR, 1e-4 relative peak, 2e-6 for a changed association of the fp32
partial sums); none is new. Each test prints its largest deviation as a fraction of its bound
(pytest -s); the measured table is DESIGN.md section 18.

Measured on one MI355X (256 CUs) on 2026-10-20, on the commit that adds this file (its parent
is b9aa04e): no defect; largest fractions of the bounds on the sampled rows: waveform 0.005
(IBM, external, ones) and 0.57 (IPD, its `one+` row: four frames, sigma 1e-7), peak 0.041, SIR
0.009; chunk grid + finalize against the per-utterance kernel: bitwise at N = 512, 4.8e-7 at
N = 1024; rows from b* on against the unsplit batch 0.18 of 2e-6; every bitwise identity held.
52 tests, 5.1 s.
"""
import functools

import numpy as np
import pytest
import torch

import utt_cases as UC
from oracle import avz_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENTINEL = 7.0
OUT_PAD = 8

CASES1 = [(p, n) for p in ("ibm", "ipd", "ext", "ones") for n in UC.SIZES]
CASES2 = [(p, v) for p in ("ibm", "ipd") for v in sorted(UC.L2_VARIANTS)]


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ----------------------------------------------------------------------------- batches, runs
class Batch:
    """One layout's inputs on the device (built on the host once, one upload)."""

    def __init__(self, n, lens, classes, keys, dev, refs=True):
        self.n, self.H, self.dev = n, n // 2, dev
        self.lens_h, self.classes, self.keys = lens, classes, keys
        mix, tgt, itf = UC.batch(n, lens, keys, refs=refs)
        self.S = mix.shape[2]
        self.max_len = int(lens.max())
        self.mix, self.lens = _dev(mix, dev), _dev(lens, dev)
        self.tgt = _dev(tgt, dev) if refs else None
        self.itf = _dev(itf, dev) if refs else None
        self._mask = None
        T = np.array([UC.n_frames(int(L), n) if L >= n else 1 for L in lens])
        self.n_out_h = (T - 1) * self.H
        self.n_out = _dev(self.n_out_h.astype(np.int64), dev)
        self.live_h = lens >= n
        self.live = _dev(self.live_h, dev)

    @property
    def B(self):
        return len(self.lens_h)

    def mask(self):
        if self._mask is None:
            self._mask = _dev(UC.masks(self.n, self.keys), self.dev)
        return self._mask


@functools.lru_cache(maxsize=None)
def _batch1(n, dev):
    lens, classes, keys = UC.layout(_cus(dev), n)
    return Batch(n, lens, classes, keys, dev)


@functools.lru_cache(maxsize=None)
def _batch2(variant, dev):
    lens, classes, keys = UC.layout2(_cus(dev), variant)
    return Batch(1024, lens, classes, keys, dev)


@functools.lru_cache(maxsize=None)
def _plan(plan, n, B, S):
    import avz
    return avz.MVDRPlan(n_fft=n, max_batch=B, max_samples=S, **UC.PLANS[plan])


def _run(pl, plan, bt, variant=2, sel=None, check_path=True):
    """One avz_mvdr_batch of batch bt (rows sel, default all) on synthesis path `variant`
    into NaN / sentinel-filled buffers, the launched kernels asserted: (out, peak)."""
    mix, lens, tgt, itf = bt.mix, bt.lens, bt.tgt, bt.itf
    M = bt.mask() if plan == "ext" else None
    if sel is not None:
        mix, lens = mix[sel], lens[sel].contiguous()
        tgt, itf = (tgt[sel], itf[sel]) if plan == "ibm" else (None, None)
        M = M[sel] if M is not None else None
    B = mix.shape[0]
    out = torch.full((B, pl.out_len(bt.max_len) + OUT_PAD), NAN, device=bt.dev)
    peak = torch.full((B,), SENTINEL, device=bt.dev)
    kw = dict(ref_tgt=tgt, ref_int=itf) if plan == "ibm" else {}

    def go():
        pl.run(mix, lens, max_len=bt.max_len, ext_mask=M, out=out, peak=peak, **kw)
        torch.cuda.synchronize()

    pl.set_diagnostics(synth_variant=variant)
    try:
        if check_path:
            UC.assert_path(pl, go, **UC.PATHS[variant])
        else:
            go()
    finally:
        pl.set_diagnostics(synth_variant=2)
    return out, peak


@functools.lru_cache(maxsize=None)
def _base1(plan, n, dev):
    bt = _batch1(n, dev)
    pl = _plan(plan, n, bt.B, bt.S)
    return bt, pl, _run(pl, plan, bt)


@functools.lru_cache(maxsize=None)
def _base2(plan, variant, dev):
    bt = _batch2(variant, dev)
    pl = _plan(plan, 1024, bt.B, bt.S)
    return bt, pl, _run(pl, plan, bt)


# ----------------------------------------------------------------------------- checks
def _sir(o, t, i):
    L = min(len(o), len(t))
    return O.projection_sdr_sir(o[:L], t[:L], i[:L])[1]


def _check_fp64(tag, plan, bt, out, peak, rows):
    """Check 1 on the sampled live rows; returns the largest fractions of the bounds."""
    n = bt.n
    idx = torch.tensor(rows, device=bt.dev)
    oh, ph = out[idx].cpu().numpy().astype(np.float64), peak[idx].cpu().numpy()
    worst = dict(out=0.0, peak=0.0, sir=0.0)
    for i, b in enumerate(rows):
        L = int(bt.lens_h[b])
        if L < n:
            continue
        r = UC.reference(plan, n, int(bt.keys[b]), L)
        n_out = len(r["out"])
        assert n_out == bt.n_out_h[b]
        got = oh[i, :n_out]
        e_out = np.abs(got - r["out"]).max() / UC.WAVE_TOL
        e_pk = abs(float(ph[i]) - r["peak"]) / (UC.PEAK_RTOL * r["peak"])
        e_sir = 0.0
        if plan == "ibm":
            e_sir = abs(_sir(got, r["tgt"], r["itf"]) - _sir(r["out"], r["tgt"], r["itf"])) \
                / UC.SIR_TOL
        print(f"{tag} b={b} ({bt.classes[b]}, L={L}): out {e_out:.4f}, peak {e_pk:.4f}, "
              f"SIR {e_sir:.4f} of their bounds")
        assert e_out <= 1 and e_pk <= 1 and e_sir <= 1, (b, bt.classes[b], e_out, e_pk, e_sir)
        for k, v in (("out", e_out), ("peak", e_pk), ("sir", e_sir)):
            worst[k] = max(worst[k], float(v))
    print(f"{tag}: largest fraction of the bound " +
          ", ".join(f"{k} {v:.4f}" for k, v in worst.items()))
    return worst


def _check_rows(plan, bt, out, peak):
    """Checks 2 and 3 on every row of the batch."""
    eps = UC.PLANS[plan].get("norm_eps", 0.0)
    valid = torch.arange(out.shape[1], device=bt.dev)[None, :] < bt.n_out[:, None]
    valid &= bt.live[:, None]
    isn = torch.isnan(out)
    # nothing written past (T - 1) H, nothing at all in a skipped row; no NaN inside
    bad = torch.nonzero(~isn & ~valid)
    assert bad.numel() == 0, ("written outside the extent", bad[:8].tolist())
    bad = torch.nonzero(isn & valid)
    assert bad.numel() == 0, ("NaN inside a live row", bad[:8].tolist())
    live, skip = bt.live, ~bt.live
    assert bool(torch.isnan(peak[skip]).all()), peak[skip][:16].tolist()
    pk = peak[live].double()
    assert bool((torch.isfinite(pk) & (pk > 0)).all())
    amax = torch.where(valid, out.abs(), torch.zeros_like(out)).amax(dim=1)[live].double()
    dev = (amax - pk / (pk + eps)).abs().max().item()
    print(f"largest |max|out| - peak / (peak + eps)| = {dev:.2e} (bound 1e-6)")
    assert dev <= 1e-6


def _valid_equal_bits(bt, a, b, n_out=None):
    """a == b bitwise on the valid extents, NaN positions included."""
    n_out = bt.n_out if n_out is None else n_out
    valid = torch.arange(a.shape[1], device=a.device)[None, :] < n_out[:, None]
    return torch.nonzero((_bits(a) != _bits(b)) & valid)


def _cross_path(tag, bt, o0, p0, o2, p2, live=None):
    """Check 5's comparison of two implementations of the chain on the same inputs."""
    live = bt.live if live is None else live
    valid = (torch.arange(o0.shape[1], device=bt.dev)[None, :] < bt.n_out[:, None]) & live[:, None]
    d = torch.where(valid, (o0 - o2).abs(), torch.zeros_like(o0)).max().item()
    dp = ((p0[live] - p2[live]).abs() / p2[live]).max().item()
    print(f"{tag}: chunk grid + finalize against the per-utterance kernel: max |d out| "
          f"{d:.3e} ({d / UC.WAVE_TOL:.4f} of the bound), max |d peak| / peak {dp:.3e} "
          f"({dp / UC.PEAK_RTOL:.4f} of the bound)")
    assert d <= UC.WAVE_TOL and dp <= UC.PEAK_RTOL, (d, dp)


# ----------------------------------------------------------------------------- first layout
@pytest.mark.parametrize("plan,n", CASES1)
def test_default_path_against_fp64(gpu_device, plan, n):
    """Checks 1-3 on the default path (the per-utterance kernel solving its own bins)."""
    bt, pl, (out, peak) = _base1(plan, n, gpu_device)
    _check_rows(plan, bt, out, peak)
    _check_fp64(f"{plan} N={n} variant 2", plan, bt, out, peak, UC.sampled_rows(_cus(gpu_device)))


@pytest.mark.parametrize("plan,n", CASES1)
def test_after_solve_kernel_bitwise(gpu_device, plan, n):
    """Check 4: the per-utterance kernel reading the solve kernel's coefficients gives the
    in-block solve's bits on every row (bin_cov_sums_utt sums as bin_cov_sums does)."""
    bt, pl, (out, peak) = _base1(plan, n, gpu_device)
    o1, p1 = _run(pl, plan, bt, variant=1)
    assert _same_bits(p1, peak), torch.nonzero(_bits(p1) != _bits(peak))[:8].tolist()
    assert _same_bits(o1, out), torch.nonzero(_bits(o1) != _bits(out))[:8].tolist()


@pytest.mark.parametrize("plan,n", CASES1)
def test_chunk_grid_path(gpu_device, plan, n):
    """Check 5 (and 2, 3 on that path): the chunk grid + finalize against the per-utterance
    kernel and against fp64."""
    bt, pl, (out, peak) = _base1(plan, n, gpu_device)
    o0, p0 = _run(pl, plan, bt, variant=0)
    _check_rows(plan, bt, o0, p0)
    assert _same_bits(torch.isnan(p0).int(), torch.isnan(peak).int())
    _cross_path(f"{plan} N={n}", bt, o0, p0, out, peak)
    _check_fp64(f"{plan} N={n} variant 0", plan, bt, o0, p0, UC.sampled_rows(_cus(gpu_device)))


@pytest.mark.parametrize("plan,n", CASES1)
def test_rows_do_not_see_neighbours(gpu_device, plan, n):
    """Check 6: without an analysis split a row's partial sums do not depend on the batch, so
    the rows moved to other blocks and rounds, and the rows beside a row holding a NaN sample,
    keep their bits."""
    R = _cus(gpu_device)
    bt, pl, (out, peak) = _base1(plan, n, gpu_device)
    src = _dev(UC.block_permutation(R), gpu_device)
    o2, p2 = _run(pl, plan, bt, sel=src)
    assert _same_bits(p2, peak[src]), torch.nonzero(_bits(p2) != _bits(peak[src]))[:8].tolist()
    bad = _valid_equal_bits(bt, o2, out[src], bt.n_out[src])
    assert bad.numel() == 0, bad[:8].tolist()
    assert bool(torch.isnan(o2[~bt.live[src]]).all())
    # a NaN sample in the round-1 `max` row of a class-0 block (block 8: not the grid's first)
    g = 8
    b = g + R
    assert bt.classes[b] == "max" and bt.classes[g] == "max" and bt.classes[g + 2 * R] == "max"
    pos = (0, 12345) if n == 1024 else (1, 20001)
    keep = bt.mix[b, pos[0], pos[1]].clone()
    try:
        bt.mix[b, pos[0], pos[1]] = NAN
        o3, p3 = _run(pl, plan, bt)
    finally:
        bt.mix[b, pos[0], pos[1]] = keep
    others = torch.ones(bt.B, dtype=torch.bool, device=gpu_device)
    others[b] = False
    for r in (g, g + 2 * R):  # the block's own other rows first: the clearer message
        assert _same_bits(o3[r], out[r]) and _same_bits(p3[r], peak[r]), r
    assert _same_bits(p3[others], peak[others])
    assert _same_bits(o3[others], out[others])


@pytest.mark.parametrize("plan,n", CASES1)
def test_run_to_run_bitwise(gpu_device, plan, n):
    """Check 7."""
    bt, pl, (out, peak) = _base1(plan, n, gpu_device)
    o2, p2 = _run(pl, plan, bt)
    assert _same_bits(o2, out) and _same_bits(p2, peak)


# ----------------------------------------------------------------------------- second layout
def _need_straddle(dev):
    R = _cus(dev)
    if not UC.straddles(R):
        pytest.skip(f"with {R} CUs no row straddles the analysis split (4 R is a multiple of 5)")
    return R


@pytest.mark.parametrize("plan,variant", CASES2)
def test_split_tail_against_fp64(gpu_device, plan, variant):
    """Checks 1, 2, 3 and 7 with a row on the analysis split (the general instance without
    synthesis pieces; bin_cov_sums_utt's fallback for the rows from b* on)."""
    R = _need_straddle(gpu_device)
    bt, pl, (out, peak) = _base2(plan, variant, gpu_device)
    _check_rows(plan, bt, out, peak)
    _check_fp64(f"{plan} split {variant} variant 2", plan, bt, out, peak, UC.sampled_rows2(R))
    o2, p2 = _run(pl, plan, bt)
    assert _same_bits(o2, out) and _same_bits(p2, peak)


@pytest.mark.parametrize("plan,variant", CASES2)
def test_split_tail_paths(gpu_device, plan, variant):
    """Checks 4 and 5 on the split batch."""
    R = _need_straddle(gpu_device)
    bt, pl, (out, peak) = _base2(plan, variant, gpu_device)
    o1, p1 = _run(pl, plan, bt, variant=1)
    assert _same_bits(p1, peak), torch.nonzero(_bits(p1) != _bits(peak))[:8].tolist()
    assert _same_bits(o1, out), torch.nonzero(_bits(o1) != _bits(out))[:8].tolist()
    o0, p0 = _run(pl, plan, bt, variant=0)
    _check_rows(plan, bt, o0, p0)
    _cross_path(f"{plan} split {variant}", bt, o0, p0, out, peak)
    _check_fp64(f"{plan} split {variant} variant 0", plan, bt, o0, p0, UC.sampled_rows2(R))


@pytest.mark.parametrize("plan,variant", CASES2)
def test_split_tail_against_unsplit_batch(gpu_device, plan, variant):
    """The same rows as the first half of a batch of 2 R rows (10 R items: no split): the rows
    below b* keep their bits (their chunks are whole in both), the rows from b* on may differ
    by the association of their split chunks' partial sums."""
    R = _need_straddle(gpu_device)
    bt, _, (out, peak) = _base2(plan, variant, gpu_device)
    pl2 = _plan(plan, 1024, 2 * R, bt.S)
    twice = torch.arange(2 * R, device=gpu_device) % R
    o2, p2 = _run(pl2, plan, bt, sel=twice)
    bs = UC.b_star(R)
    n_out2 = bt.n_out[twice]
    bad = _valid_equal_bits(bt, o2[R:], o2[:R], n_out2[:R])   # the copies among themselves
    assert bad.numel() == 0 and _same_bits(p2[R:], p2[:R]), bad[:8].tolist()
    bad = _valid_equal_bits(bt, o2[:bs], out[:bs], bt.n_out[:bs])
    assert bad.numel() == 0 and _same_bits(p2[:bs], peak[:bs]), bad[:8].tolist()
    live = bt.live.clone()
    live[:bs] = False
    valid = (torch.arange(out.shape[1], device=gpu_device)[None, :] < bt.n_out[:, None]) \
        & live[:, None]
    d = torch.where(valid, (o2[:R] - out).abs(), torch.zeros_like(out)).max().item()
    dp = ((p2[:R][live] - peak[live]).abs() / peak[live]).max().item()
    print(f"{plan} split {variant}: rows >= b* against the unsplit batch: max |d out| {d:.3e} "
          f"({d / UC.SPLIT_TOL:.4f} of the bound), max |d peak| / peak {dp:.3e}")
    assert d <= UC.SPLIT_TOL and dp <= UC.PEAK_RTOL, (d, dp)
    assert bool(torch.isnan(p2[:R][~bt.live]).all())
