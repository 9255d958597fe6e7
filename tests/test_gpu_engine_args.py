"""Every host wrapper refuses a bad tensor argument with ValueError before any launch entry
point of the library is reached, and takes a good call at the same shapes.

The bad-argument tables are made from one good call per wrapper: each tensor argument in turn
as a host tensor and with a wrong dtype, then the entries written out by hand (int64 / host
``lengths``, wrong ranks, short outputs). While they run, ``lib`` is a stand-in that passes the
size and frame-count queries through and fails the test at anything else."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_FFT, HOP, F = 512, 256, 257
B, S = 3, 2048
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
C64, C128 = torch.complex64, torch.complex128


class NoLaunch:
    """lib without its launch entry points."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name.endswith("_bytes") or name in ("avz_num_frames", "avz_room_rir_len",
                                               "avz_strerror", "avz_last_hip_error"):
            return getattr(self._real, name)

        def reached(*args):
            pytest.fail(f"{name} was reached")
        return reached


@pytest.fixture(scope="module")
def env(gpu_device):
    """Plans, the good tensors and the good call of every wrapper: {name: (fn, kwargs)}."""
    import avz
    from avz import dereverb, engine, metrics, stoi, synth
    dev = gpu_device
    kw = dict(n_fft=N_FFT, max_batch=B, max_samples=S)
    ibm = avz.MVDRPlan(mask="ibm", postfilter="ibm", normalize="peak", **kw)
    ext = avz.MVDRPlan(mask="external", postfilter="floor", normalize="none", **kw)
    sibm = avz.MVDRPlan(mask="ibm", postfilter="ibm", normalize="none", **kw)
    wide = avz.MVDRPlan(mask="ones", postfilter="none", normalize="none", n_fft=N_FFT,
                        max_batch=2 * B, max_samples=engine.out_length(S, HOP))
    g = torch.Generator(device="cpu").manual_seed(0)
    rnd = lambda *shape, dtype=F32: torch.randn(shape, generator=g).to(dtype).to(dev)  # noqa: E731
    z = lambda *shape, dtype=F32: torch.zeros(shape, dtype=dtype, device=dev)  # noqa: E731
    T = engine.n_frames(S, HOP)
    n_out = engine.out_length(S, HOP)
    hops = 3
    n = hops * HOP
    mix, tgt, itf = 0.1 * rnd(B, 2, S), 0.1 * rnd(B, S), 0.1 * rnd(B, S)
    lens = torch.tensor([S, 1500, 700], dtype=I32, device=dev)
    blk = mix[:, :, :n].contiguous()
    Y = torch.complex(rnd(B, 2, F, T), rnd(B, 2, F, T))
    cov = ibm.covariance(mix, ref_tgt=tgt, ref_int=itf)
    states = {k: z(fn(ext, B), dtype=U8) for k, fn in (
        ("mvdr", engine.stream_state_bytes), ("wpe", engine.wpe_stream_state_bytes),
        ("delay", engine.delay_stream_state_bytes))}
    states["ibm"] = z(engine.stream_state_bytes(sibm, B), dtype=U8)
    engine.stream_reset(sibm, states["ibm"], B)
    flags = torch.ones(B, dtype=I32, device=dev)
    angles = torch.full((B,), 60.0, dtype=F64, device=dev)
    engine.stream_reset(ext, states["mvdr"], B)
    engine.wpe_stream_reset(ext, states["wpe"], B)
    engine.delay_stream_reset(ext, states["delay"], B)
    room = synth.Room()
    calls = {
        "run": (ibm.run, dict(mix=mix, lengths=lens, ref_tgt=tgt, ref_int=itf, out=z(B, n_out),
                              peak=z(B), cov_out=z(B, F, 5, dtype=F64), w_out=z(B, F, 4),
                              workspace=ibm.alloc_workspace(B, S, dev))),
        "run_ext": (ext.run, dict(mix=mix, lengths=lens, ext_mask=z(B, F, T) + 0.5)),
        "covariance": (ibm.covariance, dict(mix=mix, lengths=lens, ref_tgt=tgt, ref_int=itf,
                                            cov_out=z(B, F, 5, dtype=F64))),
        "solve_covariance": (ibm.solve_covariance, dict(
            cov=cov, w=z(B, F, 4), steer=torch.ones((F, 2), dtype=C128, device=dev),
            fallback=z(B, dtype=I32))),
        "apply_istft": (ibm.apply_istft, dict(mix=mix, w=z(B, F, 4) + 0.5, lengths=lens,
                                              gain=z(B, F, T) + 1, out=z(B, n_out), peak=z(B))),
        "beamform_spectral": (ext.beamform_spectral, dict(
            Y=Y, mask=z(B, F, T) + 0.5, S=z(B, F, T, dtype=C64), cov_out=z(B, F, 5, dtype=F64),
            w_out=z(B, F, 4), fallback=z(B, dtype=I32))),
        "istft": (ext.istft, dict(S=Y[:, 0].contiguous(), out=z(B, (T - 1) * HOP), peak=z(B),
                                  workspace=ext.alloc_workspace(B, S, dev))),
        "stft": (ext.stft, dict(x=mix, lengths=lens)),
        "mask_features": (lambda **k: engine.mask_features(ext, **k), dict(x=mix, lengths=lens)),
        "mask_training_batch": (lambda **k: engine.mask_training_batch(ext, **k),
                                dict(mix=mix, tgt=tgt, itf=itf, lengths=lens)),
        "srp_scan": (lambda **k: engine.srp_scan(ext, **k), dict(mix=mix, lengths=lens)),
        "stream_reset": (lambda **k: engine.stream_reset(ext, streams=B, **k),
                         dict(state=states["mvdr"], select=flags)),
        "stream_steer": (lambda **k: engine.stream_steer(ext, streams=B, **k),
                         dict(state=states["mvdr"], angles=angles)),
        "stream_push": (lambda **k: engine.stream_push(ext, **k), dict(
            state=states["mvdr"], mix=blk, out=z(B, n), mask=z(B, F, hops) + 0.5, active=flags,
            adapt=flags, w_out=z(B, F, 4), cov_out=z(B, F, 5, dtype=F64),
            mask_out=z(B, F, hops))),
        "stream_push_ibm": (lambda **k: engine.stream_push(sibm, **k), dict(
            state=states["ibm"], mix=blk, out=z(B, n), ref_tgt=tgt[:, :n], ref_int=itf[:, :n])),
        "wpe_stream_reset": (lambda **k: engine.wpe_stream_reset(ext, streams=B, **k),
                             dict(state=states["wpe"], select=flags)),
        "wpe_stream_push": (lambda **k: engine.wpe_stream_push(ext, **k), dict(
            state=states["wpe"], mix=blk, out=z(B, 2, n), active=flags, adapt=flags,
            Y_out=z(B, 2, F, hops, dtype=C64), Z_out=z(B, 2, F, hops, dtype=C64),
            G_out=z(B, F, 20, 2, dtype=C128))),
        "delay_mask": (lambda **k: engine.delay_mask(ext, **k), dict(
            mix=mix, lengths=lens, angles=angles, mask=z(B, F, T),
            workspace=z(engine.delay_mask_workspace_bytes(ext, B, S), dtype=U8))),
        "delay_stream_reset": (lambda **k: engine.delay_stream_reset(ext, streams=B, **k),
                               dict(state=states["delay"], select=flags)),
        "delay_stream_push": (lambda **k: engine.delay_stream_push(ext, **k), dict(
            state=states["delay"], mix=blk, mask=z(B, F, hops), angles=angles, active=flags,
            adapt=flags, hist_out=z(B, 65, dtype=F64), delays_out=z(B, hops, 8, dtype=F64),
            n_peaks=z(B, hops, dtype=I32))),
        "wpe_spectral": (engine.wpe_spectral, dict(Y=Y, out=torch.empty_like(Y),
                                                   frames=z(B, dtype=I32) + T,
                                                   status=z(B, F, dtype=I32))),
        "room_rir": (lambda **k: engine.room_rir(room, **k), dict(
            src_pos=torch.tensor([[[1.0, 1.5, 1.2], [2.0, 2.5, 1.4]]], dtype=F64, device=dev))),
        "dereverb_batch": (lambda **k: dereverb.dereverb_batch(plan=wide, **k),
                           dict(mix=mix, lengths=lens, status=z(B, F, dtype=I32))),
        "projection_metrics": (metrics.projection_metrics,
                               dict(est=tgt + itf, tgt=tgt, itf=itf)),
        "stoi_batch": (stoi.stoi_batch, dict(
            clean=tgt, est=tgt + 0.1 * itf,
            workspace=z(stoi.workspace_bytes(B, S), dtype=U8))),
    }
    return dict(calls=calls, dev=dev, T=T, n_out=n_out, hops=hops, n=n, z=z)


WRAPPERS = ["run", "run_ext", "covariance", "solve_covariance", "apply_istft",
            "beamform_spectral", "istft", "stft", "mask_features", "mask_training_batch",
            "srp_scan", "stream_reset", "stream_steer", "stream_push", "stream_push_ibm",
            "wpe_stream_reset", "wpe_stream_push", "delay_mask", "delay_stream_reset",
            "delay_stream_push", "wpe_spectral", "room_rir", "dereverb_batch",
            "projection_metrics", "stoi_batch"]
# arguments a wrapper converts itself (any dtype, and for stoi_batch a host ``clean`` selects
# the host restatement): no ValueError to ask for
CONVERTED = {("projection_metrics", "est", "dtype"), ("projection_metrics", "tgt", "dtype"),
             ("projection_metrics", "itf", "dtype"), ("stoi_batch", "clean", "dtype"),
             ("stoi_batch", "est", "dtype"), ("stoi_batch", "clean", "host")}
OTHER = {F32: F64, F64: F32, I32: I64, U8: F32, C64: C128, C128: C64}


@pytest.fixture
def no_launch(monkeypatch):
    from avz import _lib, engine
    stand_in = NoLaunch(_lib.lib)
    monkeypatch.setattr(_lib, "lib", stand_in)
    monkeypatch.setattr(engine, "lib", stand_in)


@pytest.mark.parametrize("name", WRAPPERS)
def test_host_tensor_and_wrong_dtype_in_every_position(env, no_launch, name):
    fn, good = env["calls"][name]
    tried = 0
    for arg, t in good.items():
        if not isinstance(t, torch.Tensor):
            continue
        for kind, bad in (("host", t.cpu()), ("dtype", t.to(OTHER[t.dtype]))):
            if (name, arg, kind) in CONVERTED:
                continue
            with pytest.raises(ValueError):
                fn(**{**good, arg: bad})
            tried += 1
    assert tried >= 1


def hand_written(env):
    """(wrapper, changed arguments) rows beyond the generated ones."""
    z, T, n_out, n, hops = env["z"], env["T"], env["n_out"], env["n"], env["hops"]
    lens = env["calls"]["stft"][1]["lengths"]
    rows = []
    for w in ("stft", "mask_features", "mask_training_batch", "srp_scan", "run", "covariance",
              "apply_istft", "delay_mask", "dereverb_batch"):       # the lengths holes, and the rest
        rows += [(w, dict(lengths=lens.long())), (w, dict(lengths=lens.cpu())),
                 (w, dict(lengths=lens[:2])), (w, dict(lengths=lens[None]))]
    mixes = {"run": "mix", "covariance": "mix", "apply_istft": "mix", "stft": "x",
             "mask_features": "x", "mask_training_batch": "mix", "srp_scan": "mix",
             "stream_push": "mix", "wpe_stream_push": "mix", "delay_mask": "mix",
             "delay_stream_push": "mix", "dereverb_batch": "mix"}
    for w, arg in mixes.items():                                     # wrong rank
        t = env["calls"][w][1][arg]
        rows += [(w, {arg: t[0]}), (w, {arg: t[None]})]
    rows += [
        ("run", dict(out=z(B, n_out - 1))), ("run", dict(out=z(B - 1, n_out))),
        ("run", dict(out=z(B * n_out))), ("run", dict(peak=z(B - 1))),
        ("run", dict(ref_tgt=z(B, 100))), ("run", dict(cov_out=z(B, F, 4, dtype=F64))),
        ("run", dict(max_len=S + 1)), ("run_ext", dict(ext_mask=z(B, F, T - 1))),
        ("run_ext", dict(ext_mask=z(B, F * T))),
        ("covariance", dict(cov_out=z(B, F, 4, dtype=F64))),
        ("solve_covariance", dict(cov=z(B, F, 4, dtype=F64))),
        ("solve_covariance", dict(w=z(B, F, 3))), ("solve_covariance", dict(steer=z(F, 2))),
        ("apply_istft", dict(out=z(B, n_out - 1))), ("apply_istft", dict(w=z(B, F, 3))),
        ("beamform_spectral", dict(S=z(B, F, T - 1, dtype=C64))),
        ("beamform_spectral", dict(mask=z(B, F, T + 1))),
        ("beamform_spectral", dict(Y=z(B, 2, F, dtype=C64))),
        ("istft", dict(out=z(B, (T - 1) * HOP - 1))), ("istft", dict(S=z(B, F + 1, T, dtype=C64))),
        ("istft", dict(peak=z(B - 1))),
        ("mask_features", dict(layout="other")),
        ("mask_training_batch", dict(tgt=z(B, S - 1))), ("mask_training_batch", dict(itf=z(S))),
        ("stream_push", dict(out=z(B, n - 1))), ("stream_push", dict(out=z(B, n + HOP))),
        ("stream_push", dict(mix=z(B, 2, n - 1))), ("stream_push", dict(mix=z(B, 2, 0))),
        ("stream_push", dict(mask=z(B, F, hops + 1))), ("stream_push", dict(w_out=z(B, F, 5))),
        ("stream_push", dict(active=z(B - 1, dtype=I32))),
        ("stream_push_ibm", dict(ref_int=None)), ("stream_push_ibm", dict(ref_tgt=z(B, n + 1))),
        ("stream_reset", dict(select=z(B - 1, dtype=I32))),
        ("wpe_stream_reset", dict(select=z(B - 1, dtype=I32))),
        ("delay_stream_reset", dict(select=z(B - 1, dtype=I32))),
        ("stream_steer", dict(angles=z(B - 1, dtype=F64))),
        ("wpe_stream_push", dict(out=z(B, n))), ("wpe_stream_push", dict(out=z(B, 2, n - 1))),
        ("wpe_stream_push", dict(mix=z(B, 2, HOP + 1))),
        ("wpe_stream_push", dict(G_out=z(B, F, 20, dtype=C128))),
        ("delay_mask", dict(mask=z(B, F, T - 1))), ("delay_mask", dict(mask=z(B + 1, F, T))),
        ("delay_mask", dict(angles=z(B - 1, dtype=F64))),
        ("delay_stream_push", dict(mask=z(B, F, hops - 1))),
        ("delay_stream_push", dict(mix=z(B, 2, n + 7))),
        ("delay_stream_push", dict(angles=z(B + 1, dtype=F64))),
        ("delay_stream_push", dict(n_peaks=z(B, hops + 1, dtype=I32))),
        ("wpe_spectral", dict(out=z(B, 2, F, T - 1, dtype=C64))),
        ("wpe_spectral", dict(frames=z(B - 1, dtype=I32))),
        ("wpe_spectral", dict(Y=z(B, 2, F, dtype=C64))),
        ("room_rir", dict(src_pos=z(1, 2, 2, dtype=F64))),
        ("room_rir", dict(out=z(1, 2, 2, 8, dtype=F64))),
        ("projection_metrics", dict(tgt=z(B - 1, S))),
        ("stoi_batch", dict(est=z(B, S - 1))),
    ]
    return rows


def test_hand_written_rows(env, no_launch):
    rows = hand_written(env)
    for w, changed in rows:
        fn, good = env["calls"][w]
        with pytest.raises(ValueError):
            fn(**{**good, **changed})
    assert {w for w, _ in rows} == set(WRAPPERS)


def test_good_calls_are_taken(env):
    """The same calls against the library: no error, and the output shapes."""
    calls, T, n_out, n, hops = env["calls"], env["T"], env["n_out"], env["n"], env["hops"]
    shapes = {
        "run": [(B, n_out), (B,)], "run_ext": [(B, (n_out + 3) // 4 * 4), (B,)],
        "covariance": (B, F, 5), "solve_covariance": (B, F, 4),
        "apply_istft": [(B, n_out), (B,)], "beamform_spectral": (B, F, T),
        "istft": [(B, (T - 1) * HOP), (B,)], "stft": (B, 2, F, T),
        "mask_features": (B, 2, F, T), "mask_training_batch": [(B, 2, F, T), (B, F, T)],
        "srp_scan": (B, 181), "stream_push": (B, n), "stream_push_ibm": (B, n),
        "wpe_stream_push": (B, 2, n), "delay_mask": (B, F, T), "delay_stream_push": (B, F, hops),
        "wpe_spectral": (B, 2, F, T), "dereverb_batch": (B, 2, S),
        "projection_metrics": (B, 4), "stoi_batch": [(B,), (B, 4)],
    }
    for name in WRAPPERS:
        fn, good = calls[name]
        got = fn(**good)
        if name in shapes:
            want = shapes[name]
            if isinstance(want, list):
                assert [tuple(t.shape) for t in got] == want, name
            else:
                assert tuple(got.shape) == want, name
    assert tuple(calls["room_rir"][0](**calls["room_rir"][1]).shape[:3]) == (1, 2, 2)
    torch.cuda.synchronize()


def test_padded_buffers_are_taken(env):
    """Larger out, peak, lengths and ext_mask; an outsized delay mask comes back trimmed."""
    from avz import engine
    calls, z, T, n_out = env["calls"], env["z"], env["T"], env["n_out"]
    fn, good = calls["run_ext"]
    lens = torch.cat([good["lengths"], good["lengths"][:1] * 0])
    out, peak = fn(**{**good, "lengths": lens, "out": z(B + 1, n_out + 8)[:, 4:],
                      "peak": z(B + 2), "ext_mask": z(B + 1, F + 2, T + 3) + 0.5})
    assert tuple(out.shape) == (B + 1, n_out + 4) and tuple(peak.shape) == (B + 2,)
    fn, good = calls["delay_mask"]
    big = z(B, F + 1, T + 2)
    m = fn(**{**good, "mask": big, "lengths": lens})
    assert tuple(m.shape) == (B, F, T) and m.data_ptr() == big.data_ptr()
    for w in ("stft", "mask_features", "srp_scan"):
        fn, good = calls[w]
        assert fn(**{**good, "lengths": lens}).shape[0] == B
    assert engine.n_frames(int(lens[:B].max()), HOP) == T
    torch.cuda.synchronize()
