"""Reference-exact IBM decisions outside the slice test_gpu_ibm_exact.py pins (DESIGN.md
section 2.1): reference levels from 2^-70 to 2^+70, every kappa tier, the per-bin kernels
(N = 512, IRM post-filter) on batches of several grid rounds, ragged lengths on every frame-
count and chunk edge, the three-interferer family, and blocks with more than 31 analysis units.

The observable is the same everywhere: cov_out[:, :, 4], the per-bin noise-frame counts, must
equal the row sums of the oracle mask ibm_mask_noise(stft(tgt), stft(itf)) exactly. Waveforms
are compared at the suite's tolerances: 1e-4 against the oracle, 2e-6 between two GPU runs
that may differ only in the association of fp32 partial sums (a frame decided on the exact
path joins its unit's sums after the fp32 frames).
"""
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, triple_f32
from oracle import avz_oracle as O

pytestmark = pytest.mark.gpu

WAVE_TOL = 1e-4
ASSOC_TOL = 2e-6
S_GEN = 64000


@pytest.fixture(scope="module")
def avz(gpu_device):
    import avz as _avz
    return _avz


def analysis_grid(dev, n_fft):
    """Resident analysis blocks: CGeo<N>::BLOCKS (KCfg<N>::BLOCKS_PER_CU) x compute units."""
    src = open(os.path.join(PKG, "csrc", "avz_common.hpp")).read()
    body = src.split(f"struct KCfg<{n_fft}>", 1)[1]
    per_cu = int(re.search(r"\bBLOCKS_PER_CU = (\d+);", body).group(1))
    return per_cu * torch.cuda.get_device_properties(dev).multi_processor_count


def gen(dev, B, start=4242, S=S_GEN, K=2):
    from avz import synth
    return synth.make_batch_device(B, start=start, n_samples=S, n_interferers=K, device=dev,
                                   rng="philox")


def make_plan(avz, B, S, n_fft=1024, kappa=0.0, pf="ibm"):
    if pf == "irm":  # the oracle_reverb configuration (avz/oracle_reverb.py)
        return avz.MVDRPlan(n_fft=n_fft, sigma=1e-3, fmin_hz=100.0, mic_d=0.01, mask="ibm",
                            postfilter="irm", singular_fallback="mean", normalize="peak",
                            norm_eps=1e-9, max_batch=B, max_samples=S, ibm_kappa=kappa)
    return avz.MVDRPlan(n_fft=n_fft, sigma=1.0, mic_d=0.01, mask="ibm", postfilter="ibm",
                        normalize="peak", max_batch=B, max_samples=S, ibm_kappa=kappa)


def run(plan, dm, dt, di, lens=None):
    """One call with the count observable: (out, peak, counts [B, F] float64 on the host,
    stats [frames, decisions] on the exact path)."""
    dev = dm.device
    B, S = dt.shape
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    plan.set_ibm_stats(stats)
    cov = torch.zeros((B, plan.F, 5), dtype=torch.float64, device=dev)
    kw = {} if lens is None else dict(lengths=lens, max_len=S)
    out, peak = plan.run(dm, ref_tgt=dt, ref_int=di, cov_out=cov, **kw)
    torch.cuda.synchronize()
    plan.set_ibm_stats(None)
    return (out[:, :plan.out_len(S)].clone(), peak.clone(), cov[:, :, 4].cpu().numpy(),
            [int(x) for x in stats])


def oracle_mask(tgt, itf, n):
    """[..., L] float32 references -> the oracle's noise mask [..., F, T]."""
    kw = dict(nperseg=n, noverlap=n // 2)
    return O.ibm_mask_noise(O.stft(tgt, **kw)[2], O.stft(itf, **kw)[2])


def oracle_counts(tgt, itf, n, block=32):
    return np.concatenate([oracle_mask(tgt[i:i + block], itf[i:i + block], n).sum(axis=-1)
                           for i in range(0, len(tgt), block)])


def assert_counts(got, want, what, rows=None):
    bad = np.argwhere(got != want)
    per_row = np.bincount(bad[:, 0], minlength=len(got))
    print(f"{what}: {len(bad)} of {got.size} bin counts differ from the oracle mask"
          + (f"; per row {dict((rows[i] if rows else i, int(c)) for i, c in enumerate(per_row) if c)}"
             if len(bad) else ""))
    assert len(bad) == 0, (what, bad[:8].tolist())


def max_diff(a, b):
    """max |a - b| over positions where not both are NaN (a NaN against a number: inf)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both = np.isnan(a) & np.isnan(b)
    d = np.where(both, 0.0, np.abs(a - b))
    return float(np.max(np.where(np.isnan(d), np.inf, d), initial=0.0))


# ----------------------------------------------------------------------------- 1. level
LEVELS = [0, -20, -40, -55, -70, 20, 40, 62, 70]


@pytest.mark.parametrize("n", [512, 1024])
def test_triple_decisions_at_reference_levels(avz, gpu_device, n):
    """The decisions depend on the references alone and post-filter `ibm` uses only the bits:
    the bundled triple with its references x 2^k gives the oracle's counts and the k = 0 row's
    output at every k (the oracle's own mask does not move: exact powers of two)."""
    mix, tgt, itf = triple_f32("test")
    ref, st = O.oracle_debug_vec(mix, tgt, itf, n_fft=n, hop=n // 2, sigma=1.0,
                                 return_stages=True)
    want = st["mask"].sum(axis=1)
    sc = [np.float32(2.0 ** k) for k in LEVELS]
    for k, s in zip(LEVELS, sc):  # precondition, on the oracle alone
        assert np.array_equal(oracle_mask(tgt * s, itf * s, n), st["mask"]), k
    B = len(LEVELS)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)  # noqa: E731
    dm = d(np.broadcast_to(mix, (B,) + mix.shape))
    dt, di = d(np.stack([tgt * s for s in sc])), d(np.stack([itf * s for s in sc]))
    out, peak, cnt, stats = run(make_plan(avz, B, len(tgt), n), dm, dt, di)
    out, peak = out[:, :len(ref)].cpu().numpy(), peak.cpu().numpy()
    d0 = [max_diff(out[b], out[0]) for b in range(B)]
    dp = [abs(float(peak[b]) - float(peak[0])) for b in range(B)]
    do = [max_diff(out[b], ref) for b in range(B)]
    bad = [int(np.sum(cnt[b] != want)) for b in range(B)]
    print(f"N={n}: levels 2^{LEVELS}: differing bin counts {bad}; |out - out[k=0]| "
          f"{['%.1e' % x for x in d0]}; |peak - peak[k=0]| {['%.1e' % x for x in dp]}; "
          f"|out - oracle| {['%.1e' % x for x in do]}; peak {float(peak[0]):.6g} (oracle "
          f"{float(st['peak']):.6g}); {stats[0]} frames, {stats[1]} decisions on the exact path")
    assert_counts(cnt, np.broadcast_to(want, cnt.shape), f"triple N={n}", rows=LEVELS)
    assert max(d0) <= ASSOC_TOL and max(dp) <= ASSOC_TOL, (d0, dp)
    assert max(do) <= WAVE_TOL, do
    assert np.max(np.abs(peak - float(st["peak"]))) <= WAVE_TOL


def test_generator_decisions_at_reference_levels(avz, gpu_device):
    """Utterances 4242..4257 (silent-block frames), references x 2^k, N = 1024."""
    ks, U = [0, -30, -40, -60], 16
    dm, dt, di = gen(gpu_device, U)
    tgt, itf = dt.cpu().numpy(), di.cpu().numpy()
    mask = oracle_mask(tgt, itf, 1024)
    want = mask.sum(axis=-1)
    for k in ks[1:]:  # precondition per row, on the oracle alone
        s = np.float32(2.0 ** k)
        same = (oracle_mask(tgt * s, itf * s, 1024) == mask).all(axis=(1, 2))
        assert same.all(), (k, np.nonzero(~same)[0])
    cat = lambda x: torch.cat([x * (2.0 ** k) for k in ks])  # noqa: E731
    out, peak, cnt, stats = run(make_plan(avz, U * len(ks), S_GEN), dm.repeat(len(ks), 1, 1),
                                cat(dt), cat(di))
    rows = [(4242 + u, k) for k in ks for u in range(U)]
    print(f"generator levels 2^{ks}: {stats[0]} frames, {stats[1]} decisions on the exact path")
    assert_counts(cnt, np.tile(want, (len(ks), 1)), "generator levels", rows=rows)


@pytest.mark.parametrize("factor", [1e-3, 1e3, 3.0])
def test_generator_decisions_at_scaled_inputs(avz, gpu_device, factor):
    """Mix and references x a factor that is no power of two: other roundings, other near-ties.
    The oracle runs on the scaled fp32 arrays."""
    U = 16
    dm, dt, di = (x * factor for x in gen(gpu_device, U))
    plan = make_plan(avz, U, S_GEN)
    out, peak, cnt, stats = run(plan, dm, dt, di)
    mix, tgt, itf = dm.cpu().numpy(), dt.cpu().numpy(), di.cpu().numpy()
    out = out.cpu().numpy()
    worst, bad = 0.0, 0
    for b in range(U):
        ref, st = O.oracle_debug_vec(mix[b], tgt[b], itf[b], n_fft=1024, hop=512, sigma=1.0,
                                     return_stages=True)
        bad += int(np.sum(cnt[b] != st["mask"].sum(axis=1)))
        worst = max(worst, max_diff(out[b, :len(ref)], ref))
    print(f"inputs x {factor:g}: {bad} bin counts differ; waveform max |gpu - oracle| "
          f"{worst:.2e}; {stats[0]} frames, {stats[1]} decisions on the exact path")
    assert bad == 0
    assert worst <= WAVE_TOL


# ----------------------------------------------------------------------------- 2. kappa
@pytest.mark.parametrize("n,kappas", [(1024, [16.0, 32.0, 64.0, 128.0, 1024.0, 1e30]),
                                      (512, [16.0, 1024.0])])
def test_every_kappa_gives_the_reference_decisions(avz, gpu_device, n, kappas):
    """kappa only moves frames between the fp32, sparse and round tiers (x_pieces' splits, the
    SCAN_INTS batches of exact_sparse_frames, sparse and round frames inside one unit)."""
    U = 32
    dm, dt, di = gen(gpu_device, U)
    want = oracle_counts(dt.cpu().numpy(), di.cpu().numpy(), n)
    frames, out0 = [], None
    for kappa in kappas:
        out, peak, cnt, stats = run(make_plan(avz, U, S_GEN, n, kappa), dm, dt, di)
        d = 0.0 if out0 is None else max_diff(out.cpu().numpy(), out0)
        out0 = out.cpu().numpy() if out0 is None else out0
        print(f"N={n} kappa {kappa:g}: {stats[0]} frames, {stats[1]} decisions on the exact "
              f"path; |out - out[kappa 16]| {d:.1e}")
        assert_counts(cnt, want, f"N={n} kappa {kappa:g}")
        assert d <= ASSOC_TOL, (kappa, d)
        frames.append(stats[0])
    assert all(a <= b for a, b in zip(frames, frames[1:])), frames
    if kappas[-1] == 1e30:
        assert frames[-1] > frames[0], frames


# ----------------------------------------------------------------------------- 3. per-bin
@pytest.mark.parametrize("size", ["small", "rounds"])
@pytest.mark.parametrize("n,pf", [(512, "ibm"), (1024, "irm"), (512, "irm")])
def test_per_bin_kernels_on_silent_block_frames(avz, gpu_device, n, pf, size):
    """The kernels without the reference-bit hand-off defer (bin, frame) decisions one by one
    and decide them in rounds (PER_BIN): below one round of the analysis grid, and at two
    rounds and a half (whole items, then the partial round's pieces)."""
    G = analysis_grid(gpu_device, n)
    gx = -(-(-(-S_GEN // (n // 2)) + 1) // 32)  # chunks of an utterance
    B = 5 if size == "small" else -(-(2 * G + G // 2) // gx)
    assert (B * gx < G) if size == "small" else (B * gx > 2 * G and (B * gx) % G != 0)
    dm, dt, di = gen(gpu_device, B)
    out, peak, cnt, stats = run(make_plan(avz, B, S_GEN, n, pf=pf), dm, dt, di)
    tgt, itf = dt.cpu().numpy(), di.cpu().numpy()
    print(f"N={n} {pf} B={B} ({B * gx} items on {G} blocks): {stats[0]} frames, {stats[1]} "
          "decisions on the exact path")
    assert_counts(cnt, oracle_counts(tgt, itf, n), f"N={n} {pf} B={B}")
    assert stats[0] > 0
    worst = 0.0
    for b in sorted({0, 1, B // 2, B - 1}):
        mix = dm[b].cpu().numpy()
        if pf == "irm":
            ref = O.oracle_reverb_vec(mix, tgt[b], itf[b], n_fft=n, hop=n // 2, sigma=1e-3,
                                      hp=100.0)
        else:
            ref = O.oracle_debug_vec(mix, tgt[b], itf[b], n_fft=n, hop=n // 2, sigma=1.0)
        worst = max(worst, max_diff(out[b, :len(ref)].cpu().numpy(), ref))
    print(f"N={n} {pf} B={B}: waveform max |gpu - oracle| {worst:.2e}")
    assert worst <= WAVE_TOL


# ----------------------------------------------------------------------------- 4. ragged
@pytest.mark.parametrize("n", [1024, 512])
def test_ragged_lengths_on_every_frame_and_chunk_edge(avz, gpu_device, n):
    """T = ceil(L / H) + 1 frames in chunks of 32: the shortest lengths, both sides of T = 32 ->
    33 -> 34 and of the second chunk's end, the longest; lengths 0 and N - 1 are skipped rows."""
    B, S, H = 64, S_GEN, n // 2
    edges = [S, n, n + 1, n + H - 1, n + H, n + H + 1, 31 * H, 31 * H + 1, 32 * H, 32 * H + 1,
             64 * H - 1, 64 * H, 64 * H + 1, S - 1, S - H + 1, 0, n - 1]
    lens = np.random.default_rng(n).integers(n, S + 1, size=B).astype(np.int32)
    lens[:len(edges)] = edges
    dm, dt, di = gen(gpu_device, B)
    out, peak, cnt, stats = run(make_plan(avz, B, S, n), dm, dt, di,
                                lens=torch.from_numpy(lens).to(gpu_device))
    tgt, itf = dt.cpu().numpy(), di.cpu().numpy()
    bad = {}
    for b in range(B):
        L = int(lens[b])
        if L < n:
            continue
        d = int(np.sum(cnt[b] != oracle_mask(tgt[b, :L], itf[b, :L], n).sum(axis=-1)))
        if d:
            bad[(b, L)] = d
    print(f"N={n} ragged: rows (b, L) with differing bin counts {bad}; {stats[0]} frames, "
          f"{stats[1]} decisions on the exact path")
    assert not bad
    assert stats[0] > 0


# ----------------------------------------------------------------------------- 5. configs[2]
def test_three_interferer_family(avz, gpu_device):
    """512 utterances, 3 interferers, from 0: the certified decisions (kappa 16) equal the
    exact path's own (kappa 1e30) on every row, and the oracle's on rows 0..63."""
    B = 512
    dm, dt, di = gen(gpu_device, B, start=0, K=3)
    _, _, c16, s16 = run(make_plan(avz, B, S_GEN, kappa=16.0), dm, dt, di)
    _, _, cex, sex = run(make_plan(avz, B, S_GEN, kappa=1e30), dm, dt, di)
    bad = np.argwhere(c16 != cex)
    print(f"configs[2] family: {len(bad)} bin counts differ between kappa 16 ({s16[0]} frames, "
          f"{s16[1]} decisions on the exact path) and kappa 1e30 ({sex[0]} frames)")
    assert len(bad) == 0, bad[:8].tolist()
    assert_counts(c16[:64], oracle_counts(dt[:64].cpu().numpy(), di[:64].cpu().numpy(), 1024),
                  "configs[2] family rows 0..63")


# ----------------------------------------------------------------------------- 6. > 31 units
def test_records_past_a_blocks_31st_unit(avz, gpu_device):
    """Blocks of the persistent analysis grid fold every unit past their 31st into one bit of
    their unit mask, so the exact path looks at all of those units' records; a unit the call
    skips (its chunk is past the utterance's end) must not be decided from the record an
    earlier call left. 33 units a block (2 chunks a row, 33 G / 2 rows): call A at full length
    leaves unpublished records with deferrals on the chunk-1 units; call B (every row one
    chunk long: every chunk-1 unit skipped) and call C (chunk-1 units live at the blocks'
    32nd position, skipped at the 33rd) on the same plan equal a fresh plan's bitwise, stats
    included, and their stats and counts equal those of sub-batches of at most 31 units a
    block on fresh plans."""
    n, S, short = 1024, 32256, 15872
    G = analysis_grid(gpu_device, n)
    B = 33 * G // 2
    dm, dt, di = gen(gpu_device, B, S=S)
    used = make_plan(avz, B, S)
    _, _, _, stats_a = run(used, dm, dt, di)
    lens_b = np.full(B, short, np.int32)
    lens_c = lens_b.copy()
    lens_c[31 * G // 2:32 * G // 2] = S
    n_out = {L: used.out_len(L) for L in (short, S)}
    col = torch.arange(n_out[S], device=gpu_device)[None, :]
    print(f"B={B} on {G} blocks; call A: {stats_a[0]} frames, {stats_a[1]} decisions on the "
          "exact path")
    for name, lens in (("B", lens_b), ("C", lens_c)):
        lt = torch.from_numpy(lens).to(gpu_device)
        valid = col < torch.tensor([n_out[int(L)] for L in lens], device=gpu_device)[:, None]
        res = [run(plan, dm, dt, di, lens=lt) for plan in (used, make_plan(avz, B, S))]
        (o_u, p_u, c_u, s_u), (o_f, p_f, c_f, s_f) = res
        print(f"call {name}: used plan {s_u[0]} frames, {s_u[1]} decisions on the exact path; "
              f"fresh plan {s_f[0]}, {s_f[1]}")
        assert s_u == s_f, (name, s_u, s_f)
        z = torch.zeros((), device=gpu_device)
        same = lambda x, y: torch.equal(torch.nan_to_num(x, nan=7.0),  # noqa: E731
                                        torch.nan_to_num(y, nan=7.0))
        assert same(torch.where(valid, o_u[:, :n_out[S]], z), torch.where(valid, o_f[:, :n_out[S]], z))
        assert same(p_u, p_f)
        assert np.array_equal(c_u, c_f)
        del res, o_u, o_f
        step, s_sub, c_sub = 31 * G // 2, [0, 0], []
        for lo in range(0, B, step):
            hi = min(B, lo + step)
            _, _, c, s = run(make_plan(avz, hi - lo, S), dm[lo:hi], dt[lo:hi], di[lo:hi],
                             lens=lt[lo:hi].contiguous())
            c_sub.append(c)
            s_sub = [s_sub[0] + s[0], s_sub[1] + s[1]]
        print(f"call {name}: sub-batches {s_sub[0]} frames, {s_sub[1]} decisions")
        assert s_u == s_sub, (name, s_u, s_sub)
        assert np.array_equal(c_u, np.concatenate(c_sub))
