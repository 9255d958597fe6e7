"""Reference-exact IBM decisions on the GPU (avz_ibm_exact.hpp).

The reference decides noise <=> |S_int| > |S_tgt| on two fp64 scipy STFTs rounded to
complex64 (rt_av_zoom/core/oracle_debug.py:42-53). The engine decides on one fp32 transform of
the packed pair, certifies each decision against the transform's error bound, and recomputes
the uncertified ones from fp64 reference spectra. The configs[1] generator zeroes 25 % of the
250-ms blocks of every source, so about a quarter of its utterances hold frames in which all
three sources are silent at once -- references at digital-silence level, below fp32 resolution
of each other (utterances 2, 6, 9, 37, 4242, 4497 among others). Here:
  * every (bin, frame) decision of >= 64 consecutive utterances (0 .. 95) and of the 256
    utterances 4242 .. 4497 equals the oracle's -- per-bin noise-frame counts (cov_out column
    4) equal the oracle mask's, bin by bin;
  * the headline path's waveforms (fused in-block solve, peak normalisation) are within the
    1e-4 parity tolerance of the oracle on all of them;
  * with the certificate forced on every frame (kappa 1e30) the exact path alone reproduces
    the reference-run goldens' masks bit for bit, at both FFT sizes.
"""
import numpy as np
import pytest
import torch

from conftest import golden, triple_f32
from oracle import avz_oracle as O

pytestmark = pytest.mark.gpu

WAVE_TOL = 1e-4


@pytest.fixture(scope="module")
def avz(gpu_device):
    import avz as _avz
    return _avz


def run_batch(avz, dev, dm, dt, di, n_fft=1024, kappa=0.0, cov=False, stats=None):
    B, S = dt.shape
    plan = avz.MVDRPlan(n_fft=n_fft, sigma=1.0, mic_d=0.01, mask="ibm", postfilter="ibm",
                        normalize="peak", max_batch=B, max_samples=S, ibm_kappa=kappa)
    if stats is not None:
        plan.set_ibm_stats(stats)
    F = n_fft // 2 + 1
    c = torch.zeros((B, F, 5), dtype=torch.float64, device=dev) if cov else None
    out, peak = plan.run(dm, ref_tgt=dt, ref_int=di, cov_out=c)
    torch.cuda.synchronize()
    return plan, out.clone(), peak.clone(), c


@pytest.mark.parametrize("start,B", [(0, 96), (4242, 256)])
def test_generator_decisions_equal_the_reference(avz, gpu_device, start, B):
    from avz import synth
    S = 64000
    dm, dt, di = synth.make_batch_device(B, start=start, n_samples=S, n_interferers=2,
                                         device=gpu_device, rng="philox")
    stats = torch.zeros(2, dtype=torch.int64, device=gpu_device)
    plan, out, peak, _ = run_batch(avz, gpu_device, dm, dt, di, stats=stats)
    _, _, _, cov = run_batch(avz, gpu_device, dm, dt, di, cov=True)
    mix, tgt, itf = (x.cpu().numpy() for x in (dm, dt, di))
    cov = cov.cpu().numpy()
    out = out.cpu().numpy()
    n_out = plan.out_len(S)
    bad_bins, worst, n_exact_frames = 0, 0.0, int(stats[0])
    for b in range(B):
        ref, st = O.oracle_debug_vec(mix[b], tgt[b], itf[b], n_fft=1024, hop=512, sigma=1.0,
                                     return_stages=True)
        msum = st["mask"].sum(axis=1)
        diff = np.nonzero(cov[b, :, 4] != msum)[0]
        bad_bins += len(diff)
        assert len(diff) == 0, (start + b, diff[:8], cov[b, diff[:8], 4], msum[diff[:8]])
        got = out[b, :len(ref)].astype(np.float64)
        assert len(ref) == n_out
        if np.isnan(ref).all():
            assert np.isnan(got).all()
            continue
        e = float(np.max(np.abs(got - ref)))
        worst = max(worst, e)
        assert e <= WAVE_TOL, (start + b, e)
    print(f"utterances {start}..{start + B - 1}: 0 of {B * 513} bin counts differ from the "
          f"oracle mask; waveform max |gpu - oracle| {worst:.2e}; {n_exact_frames} frames and "
          f"{int(stats[1])} decisions on the exact path")
    # the silent-block frames of this generator reach the exact path in every such batch
    assert n_exact_frames > 0


@pytest.mark.parametrize("n", [512, 1024])
def test_exact_path_alone_reproduces_the_goldens(avz, gpu_device, n):
    """kappa = 1e30: no decision is certified, so every frame goes through the fp64 path."""
    g = golden(f"full_test_n{n}_s1.npz")
    mix, tgt, itf = triple_f32("test")
    ref, st = O.oracle_debug_vec(mix, tgt, itf, n_fft=n, hop=n // 2, sigma=1.0,
                                 return_stages=True)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a))[None].to(gpu_device)  # noqa: E731
    stats = torch.zeros(2, dtype=torch.int64, device=gpu_device)
    plan, out, peak, cov = run_batch(avz, gpu_device, d(mix), d(tgt), d(itf), n_fft=n,
                                     kappa=1e30, cov=True, stats=stats)
    T = st["mask"].shape[1]
    np.testing.assert_array_equal(cov[0, :, 4].cpu().numpy(), st["mask"].sum(axis=1))
    got = out[0, :len(ref)].cpu().numpy().astype(np.float64)
    assert len(ref) == int(g["out_len"])
    assert np.max(np.abs(got - ref)) <= WAVE_TOL
    L = min(len(got), len(tgt))
    sir = O.projection_sdr_sir(got[:L], tgt[:L], itf[:L])[1]
    assert abs(sir - float(g["sir_out"])) <= 0.01  # the reference run's output SIR
    # every frame with a nonzero reference went through the exact path
    assert int(stats[0]) >= T - 2, (int(stats[0]), T)
    print(f"N={n}: exact path on {int(stats[0])} of {T} frames, {int(stats[1])} decisions; "
          f"masks equal the reference run's; waveform max |diff| "
          f"{np.max(np.abs(got - ref)):.2e}")


def test_certificate_off_runs_the_fp32_decisions(avz, gpu_device):
    """kappa < 0: the pre-certificate behaviour (decisions from the fp32 transform only); the
    silent-block utterance 4242 then differs from the reference in frames 41-45."""
    from avz import synth
    S = 64000
    dm, dt, di = synth.make_batch_device(1, start=4242, n_samples=S, n_interferers=2,
                                         device=gpu_device, rng="philox")
    stats = torch.zeros(2, dtype=torch.int64, device=gpu_device)
    _, _, _, cov_off = run_batch(avz, gpu_device, dm, dt, di, kappa=-1.0, cov=True, stats=stats)
    assert int(stats[0]) == 0
    _, _, _, cov_on = run_batch(avz, gpu_device, dm, dt, di, cov=True)
    _, st = O.oracle_debug_vec(dm[0].cpu().numpy(), dt[0].cpu().numpy(), di[0].cpu().numpy(),
                               n_fft=1024, hop=512, sigma=1.0, return_stages=True)
    msum = st["mask"].sum(axis=1)
    np.testing.assert_array_equal(cov_on[0, :, 4].cpu().numpy(), msum)
    n_off = int(np.sum(cov_off[0, :, 4].cpu().numpy() != msum))
    print(f"utterance 4242: {n_off} bins' noise counts differ without the certificate, 0 with it")
    assert n_off > 0


@pytest.mark.parametrize("kappa", [16.0, 1e30])
def test_exact_path_is_deterministic(avz, gpu_device, kappa):
    """Two calls on the same plan and workspace: bitwise the same outputs, peaks, covariances
    and exact-path counts (the deferred frames' terms join each unit's partials in frame
    order, on the unit's own block)."""
    from avz import synth
    S, B = 64000, 48
    dm, dt, di = synth.make_batch_device(B, start=4242, n_samples=S, n_interferers=2,
                                         device=gpu_device, rng="philox")
    plan = avz.MVDRPlan(n_fft=1024, sigma=1.0, mic_d=0.01, mask="ibm", postfilter="ibm",
                        normalize="peak", max_batch=B, max_samples=S, ibm_kappa=kappa)
    res = []
    for _ in range(2):
        stats = torch.zeros(2, dtype=torch.int64, device=gpu_device)
        plan.set_ibm_stats(stats)
        cov = torch.zeros((B, 513, 5), dtype=torch.float64, device=gpu_device)
        out, peak = plan.run(dm, ref_tgt=dt, ref_int=di, cov_out=cov)
        torch.cuda.synchronize()
        plan.set_ibm_stats(None)
        res.append((out.clone(), peak.clone(), cov.clone(), stats.clone()))
    assert int(res[0][3][0]) > 0
    for x, y in zip(res[0], res[1]):
        assert torch.equal(x, y)
    print(f"kappa {kappa:g}: {int(res[0][3][0])} frames, {int(res[0][3][1])} decisions on the "
          "exact path; two calls bitwise equal")


def test_exact_path_ignores_an_earlier_calls_words(avz, gpu_device):
    """The uncertain-bin words (xunc) are written only for the frames a call flags; a frame
    deferred for its Nyquist bin alone has none, and must not read an earlier call's. One plan
    runs batch A (utterances 4242..) and then batch B (0..): B's outputs, peaks and covariances
    equal a fresh plan's bitwise."""
    from avz import synth
    S, B = 64000, 64
    kw = dict(n_fft=1024, sigma=1.0, mic_d=0.01, mask="ibm", postfilter="ibm", normalize="peak",
              max_batch=B, max_samples=S)
    a = synth.make_batch_device(B, start=4242, n_samples=S, n_interferers=2, device=gpu_device,
                                rng="philox")
    dm, dt, di = synth.make_batch_device(B, start=0, n_samples=S, n_interferers=2,
                                         device=gpu_device, rng="philox")
    used = avz.MVDRPlan(**kw)
    used.run(a[0], ref_tgt=a[1], ref_int=a[2])
    res = []
    for plan in (used, avz.MVDRPlan(**kw)):
        cov = torch.zeros((B, 513, 5), dtype=torch.float64, device=gpu_device)
        out, peak = plan.run(dm, ref_tgt=dt, ref_int=di, cov_out=cov)
        torch.cuda.synchronize()
        res.append((out.clone(), peak.clone(), cov))
    for x, y in zip(res[0], res[1]):
        assert torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0))


@pytest.mark.gpu
def test_work_sharing_state_in_a_callers_workspace(avz, gpu_device):
    """The exact path's work-sharing state (xst, xhint) must start zero: a caller's workspace
    arrives with arbitrary bytes, which avz_mvdr_batch clears before the launch. A plan run on
    a workspace filled with 0xff, twice, gives the plan-workspace result bitwise (utterances
    4242.. have digital-silence frames: published units, pieces on other blocks)."""
    from avz import synth
    S, B = 64000, 64
    plan = avz.MVDRPlan(n_fft=1024, sigma=1.0, mic_d=0.01, mask="ibm", postfilter="ibm",
                        normalize="peak", max_batch=B, max_samples=S)
    dm, dt, di = synth.make_batch_device(B, start=4242, n_samples=S, n_interferers=2,
                                         device=gpu_device, rng="philox")
    ws = plan.alloc_workspace(B, S, gpu_device)
    ws.fill_(0xff)
    res = []
    for w in (None, ws, ws):
        cov = torch.zeros((B, 513, 5), dtype=torch.float64, device=gpu_device)
        out, peak = plan.run(dm, ref_tgt=dt, ref_int=di, cov_out=cov, workspace=w)
        torch.cuda.synchronize()
        res.append((out.clone(), peak.clone(), cov))
    for r in res[1:]:
        for x, y in zip(res[0], r):
            assert torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0))
