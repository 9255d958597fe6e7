"""GPU: avz_stream_push / avz_stream_reset / avz_stream_steer (csrc/avz_stream.hip), the engine
wrappers and avz.stream.

Inputs: tests/stream_cases.py (3 streams, N = 512 and 1024, 17 hops plus the drain hop: two
full frame groups of eight and a ragged one). Buffers are pre-filled with NaN and padded in
every stride. Outputs and weights are compared with the fp64 restatement
avz.stream.stream_numpy at 4 E_pert + 2^-23 max|.| (stream_cases.tolerance), E_pert computed
per case from 8 seeded perturbations of Y by the STFT stage bound.
Measured on an MI355X: output errors 0.6 - 2.0e-6 at max|out| 3.5 - 8.5
where E_pert is 3 - 13e-5 (sigma 1e-5 and 1), 2.4 - 11e-5 where E_pert is 1.3 - 11e-3 (sigma
1e-7); the kernel's IBM decisions equalled the fp64 ones in every decision."""
import ctypes as ct

import numpy as np
import pytest
import torch

import stream_cases as SC
import train_cases as TC
from avz import _lib
from oracle import avz_oracle as O

pytestmark = pytest.mark.gpu

PAD_S, PAD_T = 96, 5    # extra samples per signal row / extra columns per mask row
NAN = float("nan")


def _p(t, off=0):
    return None if t is None else ct.c_void_p(t.data_ptr() + off * t.element_size())


@pytest.fixture(scope="module")
def plans(gpu_device):
    import avz
    out = {}
    for n in SC.SIZES:
        for name, kw in SC.CONFIGS.items():
            out[n, name] = avz.MVDRPlan(n_fft=n, normalize="none", max_batch=SC.STREAMS,
                                        max_samples=SC.T * (n // 2), **kw)
    return out


class Runner:
    """`idx`: which of the case's three streams sit at the state buffer's indices. Raw C-ABI
    calls into padded, NaN-filled buffers; keeps everything the tests compare."""

    def __init__(self, plan, n_fft, name, dev, idx=(0, 1, 2), forget=1.0, mix=None):
        self.plan, self.N, self.H, self.F = plan, n_fft, n_fft // 2, n_fft // 2 + 1
        self.name, self.dev, self.forget = name, dev, forget
        self.S = S = len(idx)
        n = SC.T * self.H
        mix_h, tgt_h, itf_h = SC.inputs(n_fft)
        mix_h = mix_h if mix is None else mix
        self.mix = torch.full((S, 2, n + PAD_S), NAN, dtype=torch.float32, device=dev)
        self.mix[:, :, :n] = torch.from_numpy(mix_h[list(idx)])
        self.refs = torch.full((2, S, n + PAD_S), NAN, dtype=torch.float32, device=dev)
        self.refs[0, :, :n] = torch.from_numpy(tgt_h[list(idx)])
        self.refs[1, :, :n] = torch.from_numpy(itf_h[list(idx)])
        self.mask = torch.full((S, self.F, SC.T + PAD_T), NAN, dtype=torch.float32, device=dev)
        self.mask[:, :, :SC.T] = torch.from_numpy(SC.ext_mask(n_fft)[list(idx)])
        self.out = torch.full((S, n + PAD_S), NAN, dtype=torch.float32, device=dev)
        self.w = torch.full((S, self.F, 4), NAN, dtype=torch.float32, device=dev)
        self.cov = torch.full((S, self.F, 5), NAN, dtype=torch.float64, device=dev)
        self.noise = torch.full((S, self.F, SC.T), NAN, dtype=torch.float32, device=dev)
        nbytes = _lib.lib.avz_stream_state_bytes(plan._h, S)
        assert nbytes > 0 and nbytes % 256 == 0
        self.state = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
        self.nbytes = nbytes
        self.j = 0
        self.reset()

    def reset(self, select=None):
        sel = None if select is None else torch.tensor(select, dtype=torch.int32, device=self.dev)
        rc = _lib.lib.avz_stream_reset(self.plan._h, _p(self.state), self.nbytes, self.S, _p(sel),
                                       None)
        assert rc == 0, rc

    def steer(self, angles):
        a = torch.tensor(angles, dtype=torch.float64, device=self.dev)
        rc = _lib.lib.avz_stream_steer(self.plan._h, _p(self.state), self.nbytes, self.S, _p(a),
                                       None)
        assert rc == 0, rc

    def push(self, hops, active=None, adapt=None):
        j, H = self.j, self.H
        flag = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=self.dev)  # noqa
        act, adp = flag(active), flag(adapt)
        mo = torch.full((self.S, self.F, hops), NAN, dtype=torch.float32, device=self.dev)
        a = _lib.AvzStreamArgs(streams=self.S, hops=hops, forget=self.forget)
        a.active, a.adapt = _p(act), _p(adp)
        a.mix, a.mix_stride, a.ch_stride = _p(self.mix, j * H), self.mix.stride(0), self.mix.stride(1)
        a.ref_tgt, a.ref_int = _p(self.refs[0], j * H), _p(self.refs[1], j * H)
        a.ref_stride = self.refs.stride(1)
        a.ext_mask = _p(self.mask, j)
        a.mask_stride_b, a.mask_stride_f, a.mask_stride_t = self.mask.stride()
        a.out, a.out_stride = _p(self.out, j * H), self.out.stride(0)
        a.w_out, a.cov_out, a.mask_out = _p(self.w), _p(self.cov), _p(mo)
        a.state, a.state_bytes = _p(self.state), self.nbytes
        rc = _lib.lib.avz_stream_push(self.plan._h, ct.byref(a), None)
        assert rc == 0, rc
        self.noise[:, :, j:j + hops] = mo
        self.j += hops
        return self

    def run(self, groups=SC.GROUPINGS["ragged"]):
        for g in groups:
            self.push(g)
        torch.cuda.synchronize()
        return self

    def result(self):
        torch.cuda.synchronize()
        n = SC.T * self.H
        assert torch.isnan(self.out[:, n:]).all()                 # the padding is untouched
        assert (self.state[self.nbytes:] == 0xA5).all()
        return dict(out=self.out[:, :n].clone(), w=self.w.clone(), cov=self.cov.clone(),
                    noise=self.noise.clone(), state=self.state[:self.nbytes].clone())


def _bits_equal(a, b):
    return all(torch.equal(a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8))
               for k in ("out", "w", "cov", "state"))


def _compare(tag, got, s, ref):
    tol_o, tol_w = SC.tolerance(ref)
    out = got["out"][s].cpu().numpy().astype(np.float64)
    w = got["w"][s].cpu().numpy().astype(np.float64)
    assert np.isfinite(out).all() and np.isfinite(w).all()
    e_o, e_w = np.abs(out - ref["out"]).max(), np.abs(w - ref["w"]).max()
    print(f"{tag}[{s}]: out error {e_o:.3e} / tol {tol_o:.3e} (E_pert {ref['e_out']:.2e}, "
          f"max|out| {np.abs(ref['out']).max():.3f}); w error {e_w:.3e} / tol {tol_w:.3e} "
          f"(E_pert {ref['e_w']:.2e}, max|w| {np.abs(ref['w']).max():.3f})")
    assert e_o <= tol_o and e_w <= tol_w
    H = len(out) // SC.T
    assert np.all(out[:H] == 0.0)                                 # the algorithmic latency


@pytest.mark.parametrize("forget", [1.0, 0.9])
@pytest.mark.parametrize("name", ["floor", "none"])
@pytest.mark.parametrize("n_fft", SC.SIZES)
def test_external_mask_against_the_restatement(plans, gpu_device, n_fft, name, forget):
    got = Runner(plans[n_fft, name], n_fft, name, gpu_device, forget=forget).run().result()
    for s in range(SC.STREAMS):
        _compare(f"N={n_fft} {name} forget={forget}", got, s,
                 SC.reference(n_fft, name, s, forget))
        assert np.array_equal(got["noise"][s].cpu().numpy(),
                              np.float32(1.0) - SC.ext_mask(n_fft)[s])


@pytest.mark.parametrize("n_fft", SC.SIZES)
def test_ibm_mask_and_postfilter(plans, gpu_device, n_fft):
    got = Runner(plans[n_fft, "ibm"], n_fft, "ibm", gpu_device).run().result()
    lens = TC.batches(n_fft)["A"][3]
    for s, (smp, in_band, both_zero) in enumerate(TC.reference(n_fft, "A")):
        noise = got["noise"][s].cpu().numpy()
        assert np.isin(noise, (0.0, 1.0)).all()
        T_b = TC.n_frames(int(lens[s]), n_fft)
        want = np.zeros_like(noise)                               # frames past the item: zeros
        want[:, :T_b] = smp.mag_i > smp.mag_t                     # the fp64 decision
        band = np.zeros(noise.shape, bool)
        band[:, :T_b] = in_band
        zero = np.ones(SC.T, bool)
        zero[:T_b] = both_zero
        diff = noise != want
        print(f"N={n_fft} ibm[{s}]: in band {100 * band.mean():.3f} %, differing "
              f"{int(diff.sum())} of {diff.size} (outside the band {int((diff & ~band).sum())})")
        assert not (diff & ~band).any()
        assert (noise[:, zero] == 0.0).all()
        assert diff.mean() <= 0.005
        ref = SC.reference(n_fft, "ibm", s, 1.0, key=("kernel mask", noise.tobytes()),
                           noise=noise.astype(np.float64))
        _compare(f"N={n_fft} ibm", got, s, ref)


@pytest.mark.parametrize("name", ["floor", "ibm"])
@pytest.mark.parametrize("n_fft", SC.SIZES)
def test_bitwise_under_regrouping(plans, gpu_device, n_fft, name):
    res = {g: Runner(plans[n_fft, name], n_fft, name, gpu_device, forget=0.9).run(sizes).result()
           for g, sizes in SC.GROUPINGS.items()}
    assert not torch.isnan(res["one"]["out"]).any() and float(res["one"]["out"].abs().max()) > 1e-2
    for g in ("single", "ragged"):
        assert _bits_equal(res[g], res["one"]), g
        assert torch.equal(res[g]["noise"], res["one"]["noise"])


@pytest.mark.parametrize("n_fft", SC.SIZES)
def test_bitwise_under_position(plans, gpu_device, n_fft):
    for name in ("floor", "ibm"):
        alone = Runner(plans[n_fft, name], n_fft, name, gpu_device, idx=(1,)).run().result()
        third = Runner(plans[n_fft, name], n_fft, name, gpu_device, idx=(0, 2, 1)).run().result()
        for k in ("out", "w", "cov"):
            assert torch.equal(alone[k][0].view(torch.int32 if k != "cov" else torch.int64),
                               third[k][2].view(torch.int32 if k != "cov" else torch.int64)), k
        per = alone["state"].numel()
        assert torch.equal(alone["state"], third["state"][2 * per:])


@pytest.mark.parametrize("n_fft", SC.SIZES)
def test_running_sums_are_the_offline_chain_sums(plans, gpu_device, n_fft):
    plan, H = plans[n_fft, "floor"], n_fft // 2
    r = Runner(plan, n_fft, "floor", gpu_device, forget=1.0).run()
    got = r.result()
    n = SC.HOPS * H
    mix = r.mix[:, :, :n].contiguous()
    mask = r.mask[:, :, :SC.T].contiguous()
    cov = plan.covariance(mix, ext_mask=mask)
    torch.cuda.synchronize()
    a, b = got["cov"].cpu().numpy(), cov.cpu().numpy()
    for s in range(SC.STREAMS):
        scale = np.abs(b[s][:, 0]).max()
        err = np.abs(a[s] - b[s])
        print(f"N={n_fft}[{s}]: sums error / (2e-6 scale) = {err[:, :4].max() / (2e-6 * scale):.3f}, "
              f"mask sums error {err[:, 4].max():.2e} of {b[s][:, 4].max():.2f}")
        # test_gpu_parity.py's tolerance for cov_out: 2e-6 of the largest |y0|^2 sum
        assert err[:, :4].max() <= 2e-6 * scale
        assert err[:, 4].max() <= 2e-6 * b[s][:, 4].max()
    # the weights are avz_solve_covariance of the stream's sums: the same fp64 solve, so at
    # most the float32 rounding of a value that differs in its last fp64 bits
    w = plan.solve_covariance(got["cov"])
    torch.cuda.synchronize()
    dw = (w - got["w"]).abs().max().item()
    print(f"N={n_fft}: max|w_stream - w_solve| = {dw:.3e}, max|w| = {w.abs().max().item():.3f}")
    assert dw <= 2.0 ** -23 * w.abs().max().item()


@pytest.mark.parametrize("n_fft", SC.SIZES)
def test_isolation_active_reset_and_adapt(plans, gpu_device, n_fft):
    plan, name, H = plans[n_fft, "floor"], "floor", n_fft // 2
    clean = Runner(plan, n_fft, name, gpu_device, forget=0.9).run().result()
    # a NaN hop in stream 1 reaches its own output and state only
    mix = SC.inputs(n_fft)[0].copy()
    mix[1, 0, 4 * H:5 * H] = np.nan
    dirty = Runner(plan, n_fft, name, gpu_device, forget=0.9, mix=mix).run().result()
    per = clean["state"].numel() // SC.STREAMS
    for s in (0, 2):
        for k in ("out", "w", "cov"):
            assert torch.equal(dirty[k][s], clean[k][s]), (k, s)
        assert torch.equal(dirty["state"][s * per:(s + 1) * per], clean["state"][s * per:(s + 1) * per])
    assert torch.isnan(dirty["out"][1]).any() and not torch.isnan(clean["out"][1]).any()

    # active = 0: the stream's state and output rows stay as they are
    r = Runner(plan, n_fft, name, gpu_device, forget=0.9).push(3)
    torch.cuda.synchronize()
    before = r.state.clone()
    r.push(1, active=[1, 0, 1])
    torch.cuda.synchronize()
    assert torch.equal(r.state[per:2 * per], before[per:2 * per])
    assert not torch.equal(r.state[:per], before[:per])
    assert torch.isnan(r.out[1, 3 * H:4 * H]).all() and torch.isnan(r.noise[1, :, 3]).all()
    assert torch.equal(r.out[0, :4 * H], clean["out"][0, :4 * H])
    assert torch.equal(r.out[2, :4 * H], clean["out"][2, :4 * H])

    # reset(select) of stream 1 after 8 hops: its next outputs are a fresh stream's on the
    # same input, the others continue
    r = Runner(plan, n_fft, name, gpu_device, forget=0.9).push(8)
    r.reset(select=[0, 1, 0])
    r.push(SC.T - 8)
    late = r.result()
    fresh = Runner(plan, n_fft, name, gpu_device, forget=0.9)
    fresh.j = 8
    fresh.push(SC.T - 8)
    fresh = fresh.result()
    assert torch.equal(late["out"][1, 8 * H:], fresh["out"][1, 8 * H:])
    assert torch.equal(late["w"][1], fresh["w"][1]) and torch.equal(late["cov"][1], fresh["cov"][1])
    assert torch.equal(late["state"][per:2 * per], fresh["state"][per:2 * per])
    assert (late["out"][1, 8 * H:9 * H] == 0).all()
    for s in (0, 2):
        assert torch.equal(late["out"][s], clean["out"][s]) and torch.equal(late["w"][s], clean["w"][s])

    # adapt = 0 freezes the sums and the weights
    r = Runner(plan, n_fft, name, gpu_device, forget=0.9).push(5)
    torch.cuda.synchronize()
    w5, c5 = r.w.clone(), r.cov.clone()
    r.push(4, adapt=[1, 0, 1])
    torch.cuda.synchronize()
    assert torch.equal(r.w[1], w5[1]) and torch.equal(r.cov[1], c5[1])
    assert not torch.equal(r.w[0], w5[0]) and not torch.equal(r.cov[2], c5[2])
    ref = SC.reference(n_fft, name, 1, 0.9, key="adapt 5-8 off",
                       adapt=np.array([1] * 5 + [0] * 4 + [1] * (SC.T - 9)))
    r.push(SC.T - 9)
    _compare(f"N={n_fft} adapt", r.result(), 1, ref)


@pytest.mark.parametrize("n_fft", SC.SIZES)
def test_steering_per_stream_and_between_pushes(plans, gpu_device, n_fft):
    name = "floor"
    d = SC.CONFIGS[name]["mic_d"]
    f = np.fft.rfftfreq(n_fft, 1.0 / 16000)
    r = Runner(plans[n_fft, name], n_fft, name, gpu_device, forget=0.9)
    r.steer([60.0, NAN, 120.0])                                   # stream 1 keeps the plan's 90
    r.push(9)
    r.steer([75.0, NAN, NAN])                                     # from frame 9 on
    r.push(SC.T - 9)
    got = r.result()
    sched = [{0: 60.0, 9: 75.0}, {0: 90.0}, {0: 120.0}]
    for s in range(SC.STREAMS):
        steer = {t: O.steering_vectors(f, a, d, O.C_SOUND) for t, a in sched[s].items()}
        ref = SC.reference(n_fft, name, s, 0.9, key=("steer", s), steer=steer)
        _compare(f"N={n_fft} steer", got, s, ref)
    base = SC.reference(n_fft, name, 0, 0.9)
    assert np.abs(got["w"][0].cpu().numpy() - base["w"]).max() > 1e-3   # the direction matters
    assert torch.equal(got["w"][1], Runner(plans[n_fft, name], n_fft, name, gpu_device,
                                           forget=0.9).run().result()["w"][1])


def test_wrappers_and_checks_with_a_plan(plans, gpu_device):
    import avz
    from avz.stream import StreamingBeamformer, enhance_stream
    n_fft, H = 512, 256
    plan = plans[n_fft, "ibm"]
    raw = Runner(plan, n_fft, "ibm", gpu_device).run().result()
    mix_h, tgt_h, itf_h = SC.inputs(n_fft)
    dev = gpu_device
    mix, tgt, itf = (torch.from_numpy(a).to(dev) for a in (mix_h, tgt_h, itf_h))
    sb = StreamingBeamformer(plan, SC.STREAMS, device=dev)
    n = SC.HOPS * H
    outs = [sb.push(mix[:, :, :5 * H], ref_tgt=tgt[:, :5 * H], ref_int=itf[:, :5 * H]),
            sb.push(mix[:, :, 5 * H:n], ref_tgt=tgt[:, 5 * H:n], ref_int=itf[:, 5 * H:n]),
            sb.flush()]
    out = torch.cat(outs, dim=1)
    assert torch.equal(out, raw["out"]) and torch.equal(sb.w, raw["w"])
    assert torch.equal(sb.cov, raw["cov"])
    sb.reset()
    again = sb.push(mix[:, :, :5 * H], ref_tgt=tgt[:, :5 * H], ref_int=itf[:, :5 * H])
    assert torch.equal(again, outs[0])
    # a whole file, hop by hop, the delay trimmed
    L = 15 * H - 37
    y = enhance_stream(mix_h[0][:, :L], (tgt_h[0][:L], itf_h[0][:L]), hops_per_push=2,
                       n_fft=n_fft, sigma=1.0, mic_d=0.01)
    assert y.shape == (L,) and y.dtype == np.float32 and np.isfinite(y).all()
    whole = enhance_stream(mix_h[0][:, :15 * H], (tgt_h[0][:15 * H], itf_h[0][:15 * H]),
                           hops_per_push=7, n_fft=n_fft, sigma=1.0, mic_d=0.01)
    assert np.array_equal(whole, raw["out"][0, H:16 * H].cpu().numpy())
    # plans the streaming path does not take, and arguments it rejects, with a real plan
    lib = _lib.lib
    peak = avz.MVDRPlan(n_fft=n_fft, mask="ibm", postfilter="ibm", normalize="peak", max_batch=3,
                        max_samples=8192)
    assert lib.avz_stream_state_bytes(peak._h, 1) == _lib.AVZ_ERR_UNSUPPORTED
    assert lib.avz_stream_state_bytes(plan._h, 4) == _lib.AVZ_ERR_SHAPE
    with pytest.raises(_lib.AvzError):
        StreamingBeamformer(peak, 1, device=dev)
    a = _lib.AvzStreamArgs(streams=1, hops=1, forget=1.0, mix=4096, ch_stride=H, ref_tgt=4096,
                           ref_int=4096, out=4096, out_stride=H, state=4096, state_bytes=1 << 20)
    assert lib.avz_stream_push(peak._h, ct.byref(a), None) == _lib.AVZ_ERR_UNSUPPORTED
    a.forget = 0.0
    assert lib.avz_stream_push(plan._h, ct.byref(a), None) == _lib.AVZ_ERR_ARG
    a.forget, a.state_bytes = 1.0, 1024
    assert lib.avz_stream_push(plan._h, ct.byref(a), None) == _lib.AVZ_ERR_SHAPE
    a.state_bytes, a.out = 1 << 20, 4100
    assert lib.avz_stream_push(plan._h, ct.byref(a), None) == _lib.AVZ_ERR_ALIGN
