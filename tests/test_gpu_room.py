"""Reverberant shoebox scenes on the device (csrc/avz_scene.hip) against the host restatement
of the image-source model (avz/synth.py; cases in tests/room_cases.py).

* avz_room_rir per sample within 2^-50 max|h| + 4 max_n E_ref of room_rir in fp64: the
  first term is fp64 rounding of the sums, E_ref = |h64 - hld| the restatement's own error
  (the rounding of distant images' delays), the factor 4 allows for the kernel's own sin / cos
  roundings: the form of test_gpu_wpe.py. Worst observed ratios: DESIGN.md section 10.
* avz_scene_reverb_mix / avz_scene_reverb_generate within 2e-5 absolute of the host on the
  peak-normalised outputs, the tolerance of test_gpu_scene.py."""
import ctypes as ct

import numpy as np
import pytest
import torch

import room_cases as R

pytestmark = pytest.mark.gpu

SCENE_TOL = 2e-5


@pytest.fixture(scope="module")
def eng(gpu_device):
    from avz import engine
    return engine


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_rir_matches_the_fp64_model(eng, gpu_device, case):
    ref = R.case_reference(case.name)
    pos = np.asarray(case.pos, np.float64)
    h = eng.room_rir(case.room, pos, device=gpu_device)
    h2 = eng.room_rir(case.room, torch.from_numpy(pos).to(gpu_device))
    torch.cuda.synchronize()
    got = h.cpu().numpy()
    assert got.shape == ref["h64"].shape and got.shape[-1] == case.room.rir_len
    assert np.array_equal(got, h2.cpu().numpy())              # equal bits from call to call
    err = np.abs(got - ref["h64"])
    tol = 2.0 ** -50 * ref["hmax"] + 4 * ref["E_ref"]
    print(f"{case.name}: worst error / tolerance = {err.max() / tol:.3f} (error {err.max():.3e}, "
          f"E_ref {ref['E_ref']:.2e}, max|h| {ref['hmax']:.3e}, rir_len {got.shape[-1]})")
    assert np.all(err <= tol), float(err.max() / tol)
    if case.name.startswith("e-"):                             # the direct sound starts at sample 0
        assert got[0, 0, 0, 0] != 0.0


def _mix(room, pos, srcs, noise, dev, pad=0):
    from avz import synth
    from avz._lib import check, lib
    B, S, n = srcs.shape
    r = synth._room_struct(room)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_pos, d_src, d_noise = d(pos), d(srcs), d(noise)
    big = torch.full((B, 2, n + pad), 7.0, dtype=torch.float32, device=dev)
    mix = big[:, :, :n]
    tgt = torch.empty((B, n), dtype=torch.float32, device=dev)
    itf = torch.empty((B, n), dtype=torch.float32, device=dev)
    ws_bytes = lib.avz_scene_reverb_workspace_bytes(ct.byref(r), B, S, n)
    ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.float32, device=dev)
    p = lambda t: ct.c_void_p(t.data_ptr())  # noqa: E731
    check(lib.avz_scene_reverb_mix(ct.byref(r), B, S, n, p(d_src), p(d_pos), p(d_noise), 0.0, 5.0,
                                   p(mix), mix.stride(0), mix.stride(1), p(tgt), p(itf),
                                   tgt.stride(0), p(ws), ws_bytes, None), "avz_scene_reverb_mix")
    torch.cuda.synchronize()
    return big, mix, tgt, itf


@pytest.mark.parametrize("case", R.MIX_CASES, ids=lambda c: c.name)
def test_reverb_mix_matches_host(gpu_device, case):
    pos, srcs, noise, hm, ht, hi = R.mix_case(case.name)
    pad = 5 if case.name == "small-n4000-K2" else 0           # strided mix rows
    big, mix, tgt, itf = _mix(case.room, pos, srcs, noise, gpu_device, pad)
    worst = max(float(np.max(np.abs(a.cpu().numpy() - h))) for a, h in ((mix, hm), (tgt, ht),
                                                                         (itf, hi)))
    print(f"avz_scene_reverb_mix {case.name}: max |d| {worst:.2e}")
    assert worst <= SCENE_TOL
    if case.K > 0:
        assert abs(float(mix.abs().amax()) - 1.0) <= 1e-6
        assert float(itf.abs().amax()) > 0.05
    else:
        assert not bool(itf.any())
    assert float(tgt.abs().amax()) > 0.05
    if pad:
        assert bool((big[:, :, case.n:] == 7.0).all())         # nothing written between rows


@pytest.mark.parametrize("n,k,batch,start,order", [(16000, 3, 2, 0, 10),
                                                   (8000, 1, 2, 2 ** 33 + 5, 15)])
def test_generated_reverb_scene_matches_restatement(gpu_device, n, k, batch, start, order):
    from avz import synth
    room = synth.Room(max_order=order)
    kw = dict(start=start, n_samples=n, n_interferers=k, room=room)
    mix, tgt, itf = synth.make_reverb_batch_device(batch, device=gpu_device, rng="philox", **kw)
    hm, ht, hi = synth.make_reverb_batch_philox(batch, **kw)
    worst = max(float(np.max(np.abs(a.cpu().numpy() - h))) for a, h in ((mix, hm), (tgt, ht),
                                                                         (itf, hi)))
    print(f"avz_scene_reverb_generate n={n} k={k} start={start} N={order}: max |d| {worst:.2e}")
    assert worst <= SCENE_TOL
    assert abs(float(mix.abs().amax()) - 1.0) <= 1e-6
    m2, _, _ = synth.make_reverb_batch_device(batch, device=gpu_device, rng="philox", seed=1, **kw)
    assert not torch.equal(mix, m2)                            # another seed, another scene
    # the scenes do not depend on how the wrapper slices the batch
    old = synth.REVERB_SLICE_BYTES
    try:
        synth.REVERB_SLICE_BYTES = 1
        m3, t3, _ = synth.make_reverb_batch_device(batch, device=gpu_device, rng="philox", **kw)
    finally:
        synth.REVERB_SLICE_BYTES = old
    assert torch.equal(mix, m3) and torch.equal(tgt, t3)


def test_host_draw_batches_match_host(gpu_device):
    """make_reverb_batch_device(rng="host"): the host RNG's sources and noise through
    avz_scene_reverb_mix, against reverb_mix_draws on the same draws."""
    from avz import synth
    room = synth.Room(max_order=3)
    B, n, K = 2, 4001, 3
    mix, tgt, itf = synth.make_reverb_batch_device(B, start=7, n_samples=n, n_interferers=K,
                                                   room=room, device=gpu_device)
    for b in range(B):
        hm, ht, hi = synth.reverb_mix_draws(*synth.reverb_scene_draws(7 + b, n, K, room), room)
        worst = max(float(np.max(np.abs(a[b].cpu().numpy() - h))) for a, h in ((mix, hm), (tgt, ht),
                                                                                (itf, hi)))
        assert worst <= SCENE_TOL, (b, worst)
    with pytest.raises(ValueError):
        synth.make_reverb_batch_device(1, n_samples=n, room=room, device=gpu_device, rng="mt")


def test_run_batch_reverb(gpu_device):
    from avz import batch_run
    kw = dict(n_interferers=2, seconds=1.0, batch=4, device=gpu_device)
    rev = batch_run.run_batch(4, reverb=True, max_order=3, **kw)
    dry = batch_run.run_batch(4, **kw)
    assert len(rev.rows) == 4 and np.all(np.isfinite(rev.sums)) and rev.sums[4] == 4
    vals = lambda r: [[float(row[k]) for k in ("SIR_Base", "SIR_Enh", "SINR_Base", "SINR_Enh")]  # noqa
                      for row in r.rows]
    assert np.all(np.isfinite(vals(rev)))
    assert vals(rev) != vals(dry)
    print(f"run_batch reverb N=3: SIR {rev.sums[0] / 4:.2f} -> {rev.sums[1] / 4:.2f} dB; "
          f"anechoic {dry.sums[0] / 4:.2f} -> {dry.sums[1] / 4:.2f} dB")


def test_reverberant_scenes_feed_the_chain(eng, gpu_device):
    """A reverberant batch through avz_wpe_spectral and the IBM chain. No SIR is required:
    the figures are printed and recorded in DESIGN.md section 10."""
    import avz
    from avz import dereverb, metrics, synth
    B, S = 4, 16000
    mix, tgt, itf = synth.make_reverb_batch_device(B, start=200, n_samples=S, n_interferers=2,
                                                   device=gpu_device, rng="philox")
    plan = dereverb._plan(dereverb.N_FFT, B, S)
    Y = plan.stft(mix, None, S)
    Yh = Y.cpu().numpy()
    st = torch.full((B, plan.F), -1, dtype=torch.int32, device=gpu_device)
    derev = dereverb.dereverb_batch(mix, plan=plan, status=st)
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    assert bool(torch.isfinite(derev).all()) and set(np.unique(st)) <= {0, 1, 2}
    host_ok = np.stack([dereverb.wpe_numpy(Yh[b], return_info=True)[1] == 0 for b in range(B)])
    assert host_ok.any() and np.all(st[host_ok] == 0)
    chain = avz.MVDRPlan(n_fft=1024, sigma=1.0, mic_d=0.01, mask="ibm", postfilter="ibm",
                         normalize="peak", max_batch=B, max_samples=S)
    sirs = {}
    for name, x in (("mixture", mix), ("wpe", derev)):
        out, _ = chain.run(x.contiguous(), ref_tgt=tgt, ref_int=itf)
        assert bool(torch.isfinite(out).all())
        L = min(out.shape[-1], S)
        m = metrics.projection_metrics(out[:, :L].contiguous(), tgt[:, :L].contiguous(),
                                       itf[:, :L].contiguous())
        assert bool(torch.isfinite(m).all())
        sirs[name] = m[:, 3].mean().item()
    base = metrics.projection_metrics(mix[:, 0].contiguous(), tgt, itf)[:, 3].mean().item()
    print(f"reverberant scenes (N = 15, 1 s, 2 interferers): mic-1 SIR {base:.2f} dB; IBM chain "
          f"{sirs['mixture']:.2f} dB; WPE + IBM chain {sirs['wpe']:.2f} dB; WPE status 0 on "
          f"{int((st == 0).sum())} of {st.size} bins")
