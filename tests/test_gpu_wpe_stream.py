"""GPU: avz_wpe_stream_push / avz_wpe_stream_reset (csrc/avz_wpe_stream.hip), the engine
wrappers and avz.dereverb.StreamingWPE / apply_wpe_stream.

Inputs: tests/wpe_stream_cases.py (3 streams, N = 512 and 1024; K = 2 over 18 hops, K = 10 and
K = 16 over 48: the ring wraps, the rounds of eight frames end ragged). Buffers are pre-filled
with NaN and padded in every stride; the state buffer is followed by a guard. The spectral
stage is compared with the fp64 restatement avz.dereverb.wpe_stream_numpy run on the kernel's
own Y at 2^-23 max|Z_k| + 4 E_ref,k per bin; the time output and G with the restatement on
the raw samples at 4 E_pert + 2^-23 max|.| (wpe_stream_cases.tolerance). Measured figures:
DESIGN.md section 15."""
import ctypes as ct

import numpy as np
import pytest
import scipy.signal
import torch

import stream_cases as SC
import wpe_stream_cases as WC
from avz import _lib
from avz import dereverb as DV
from avz import stream as ST

pytestmark = pytest.mark.gpu

PAD_S = 96              # extra samples per signal row
NAN = float("nan")
CASE_IDS = [(n, c) for n in WC.SIZES for c in WC.CASES]


def _p(t, off=0):
    return None if t is None else ct.c_void_p(t.data_ptr() + off * t.element_size())


@pytest.fixture(scope="module")
def plans(gpu_device):
    import avz
    return {n: avz.MVDRPlan(n_fft=n, mask="ones", postfilter="none", normalize="none",
                            max_batch=WC.STREAMS, max_samples=48 * (n // 2))
            for n in WC.SIZES}


class Runner:
    """`idx`: which of the case's three streams sit at the state buffer's indices. Raw C-ABI
    calls into padded, NaN-filled buffers; keeps everything the tests compare."""

    def __init__(self, plan, n_fft, case, dev, idx=(0, 1, 2), mix=None, debug=True):
        self.plan, self.N, self.H, self.F = plan, n_fft, n_fft // 2, n_fft // 2 + 1
        self.case, self.dev, self.debug = case, dev, debug
        c = WC.CASES[case]
        self.T, self.K, self.D, self.forget = c["T"], c["taps"], c["delay"], c["forget"]
        self.floor = DV.default_power_floor(n_fft)
        self.S = S = len(idx)
        n = self.T * self.H
        mix_h = WC.inputs(n_fft, self.T) if mix is None else mix
        self.mix = torch.full((S, 2, n + PAD_S), NAN, dtype=torch.float32, device=dev)
        self.mix[:, :, :n] = torch.from_numpy(mix_h[list(idx)])
        self.out = torch.full((S, 2, n + PAD_S), NAN, dtype=torch.float32, device=dev)
        self.Y = torch.full((S, 2, self.F, self.T), NAN, dtype=torch.complex64, device=dev)
        self.Z = torch.full((S, 2, self.F, self.T), NAN, dtype=torch.complex64, device=dev)
        self.G = torch.full((S, self.F, 2 * self.K, 2), NAN, dtype=torch.complex128, device=dev)
        nbytes = _lib.lib.avz_wpe_stream_state_bytes(plan._h, S, self.K, self.D)
        assert nbytes > 0 and nbytes % 256 == 0
        self.state = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
        self.nbytes = nbytes
        self.j = 0
        self.reset()

    def reset(self, select=None):
        sel = None if select is None else torch.tensor(select, dtype=torch.int32, device=self.dev)
        rc = _lib.lib.avz_wpe_stream_reset(self.plan._h, _p(self.state), self.nbytes, self.S,
                                           self.K, self.D, 1.0, _p(sel), None)
        assert rc == 0, rc

    def args(self, hops, **over):
        j, H = self.j, self.H
        a = _lib.AvzWpeStreamArgs(streams=self.S, hops=hops, taps=self.K, delay=self.D,
                                  forget=self.forget, power_floor=self.floor)
        a.mix, a.mix_stride, a.ch_stride = _p(self.mix, j * H), self.mix.stride(0), self.mix.stride(1)
        a.out, a.out_stride, a.out_ch_stride = _p(self.out, j * H), self.out.stride(0), self.out.stride(1)
        a.G_out = _p(self.G)
        a.state, a.state_bytes = _p(self.state), self.nbytes
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def push(self, hops, active=None, adapt=None):
        flag = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=self.dev)  # noqa
        act, adp = flag(active), flag(adapt)
        a = self.args(hops, active=_p(act), adapt=_p(adp))
        if self.debug:
            yo = torch.full((self.S, 2, self.F, hops), NAN, dtype=torch.complex64, device=self.dev)
            zo = torch.full_like(yo, NAN)
            a.Y_out, a.Z_out = _p(yo), _p(zo)
        rc = _lib.lib.avz_wpe_stream_push(self.plan._h, ct.byref(a), None)
        assert rc == 0, rc
        if self.debug:
            self.Y[..., self.j:self.j + hops] = yo
            self.Z[..., self.j:self.j + hops] = zo
        self.j += hops
        return self

    def run(self, groups=None):
        for g in (WC.groupings(self.case)["ragged"] if groups is None else groups):
            self.push(g)
        return self

    def result(self):
        torch.cuda.synchronize()
        n = self.T * self.H
        assert torch.isnan(self.out[:, :, n:]).all()              # the padding is untouched
        assert (self.state[self.nbytes:] == 0xA5).all()
        return dict(out=self.out[:, :, :n].clone(), G=self.G.clone(), Y=self.Y.clone(),
                    Z=self.Z.clone(), state=self.state[:self.nbytes].clone())


def _bytes(t):
    return t.contiguous().view(torch.uint8) if not t.is_complex() else \
        torch.view_as_real(t.contiguous()).view(torch.uint8)


def _bits_equal(a, b, keys=("out", "G", "state")):
    return all(torch.equal(_bytes(a[k]), _bytes(b[k])) for k in keys)


_RUNS = {}


@pytest.fixture(scope="module")
def ragged(plans, gpu_device):
    """The ragged run of every (size, case), made once and left unchanged."""
    def get(n_fft, case):
        if (n_fft, case) not in _RUNS:
            _RUNS[n_fft, case] = Runner(plans[n_fft], n_fft, case, gpu_device).run().result()
        return _RUNS[n_fft, case]
    return get


@pytest.mark.parametrize("n_fft,case", CASE_IDS)
def test_spectral_stage_against_the_restatement_on_the_kernels_own_y(ragged, n_fft, case):
    got = ragged(n_fft, case)
    worst, moved = 0.0, 0.0
    for s in range(WC.STREAMS):
        Y = got["Y"][s].cpu().numpy()
        Z = got["Z"][s].cpu().numpy().astype(np.complex128)
        assert np.isfinite(Z.view(np.float64)).all()
        Zr, _, e_ref = WC.spectral_reference(Y, n_fft, case)
        tol = WC.spectral_tolerance(Zr, e_ref)                    # [F]
        err = np.abs(Z - Zr).max(axis=(0, 2))
        live = tol > 0                                            # an all-zero bin: exact
        assert np.all(err[~live] == 0.0)
        ratio = (err[live] / tol[live]).max()
        change = np.abs(Z - Y).max()
        print(f"N={n_fft} {case}[{s}]: worst error / tolerance {ratio:.3f} (max E_ref "
              f"{e_ref.max():.2e}, max|Z| {np.abs(Zr).max():.3e}); max|Z - Y| {change:.3e} = "
              f"{change / tol.max():.1f} x max tolerance")
        worst, moved = max(worst, ratio), max(moved, change / tol.max())
        assert np.all(err <= tol)
    # a pass-through kernel cannot pass
    assert moved > 100.0, moved


@pytest.mark.parametrize("n_fft", WC.SIZES)
def test_analysis_frames_are_scipy_stft_frames(ragged, n_fft):
    got, H, T = ragged(n_fft, "k2"), n_fft // 2, WC.CASES["k2"]["T"]
    for s in range(WC.STREAMS):
        mix = WC.inputs(n_fft, T)[s][:, :(T - 1) * H].astype(np.float64)
        _, _, Ys = scipy.signal.stft(mix, nperseg=n_fft, noverlap=H)      # [2, F, T]
        Y = got["Y"][s].cpu().numpy()
        err, ymax = np.abs(Y - Ys).max(), np.abs(Ys).max()
        print(f"N={n_fft}[{s}]: max|Y - stft| = {err:.3e} = {err / ymax:.2e} max|Y|")
        assert Ys.shape == Y.shape and err <= SC.STAGE * ymax


@pytest.mark.parametrize("n_fft,case", CASE_IDS)
def test_time_output_and_filter_against_the_restatement(ragged, n_fft, case):
    got, H = ragged(n_fft, case), n_fft // 2
    for s in range(WC.STREAMS):
        ref = WC.reference(n_fft, case, s)
        tol_o, tol_g = WC.tolerance(ref)
        out = got["out"][s].cpu().numpy().astype(np.float64)
        G = got["G"][s].cpu().numpy()
        assert np.isfinite(out).all() and np.isfinite(G.view(np.float64)).all()
        e_o, e_g = np.abs(out - ref["out"]).max(), np.abs(G - ref["G"]).max()
        print(f"N={n_fft} {case}[{s}]: out error {e_o:.3e} / tol {tol_o:.3e} (E_pert "
              f"{ref['e_out']:.2e} = {ref['e_out'] / ref['ymax']:.2e} max|Y|, max|out| "
              f"{np.abs(ref['out']).max():.3f}); G error {e_g:.3e} / tol {tol_g:.3e} (E_pert "
              f"{ref['e_g']:.2e}, max|G| {np.abs(ref['G']).max():.3f})")
        assert e_o <= tol_o and e_g <= tol_g
        assert np.all(out[:, :H] == 0.0)                          # the algorithmic latency
        assert np.abs(out).max() > 1e-2


@pytest.mark.parametrize("n_fft,case", CASE_IDS)
def test_grouping_of_hops_changes_no_bit(plans, gpu_device, ragged, n_fft, case):
    base = ragged(n_fft, case)
    for name in ("one", "single"):
        r = Runner(plans[n_fft], n_fft, case, gpu_device).run(WC.groupings(case)[name]).result()
        assert _bits_equal(r, base, ("out", "G", "state", "Y", "Z")), name


@pytest.mark.parametrize("n_fft", WC.SIZES)
def test_index_other_streams_nan_and_active_change_no_bit(plans, gpu_device, ragged, n_fft):
    case = "k10"
    base = ragged(n_fft, case)
    H, T = n_fft // 2, WC.CASES[case]["T"]
    per = base["state"].numel() // WC.STREAMS
    # index 0 of 1 = index 2 of 3
    solo = Runner(plans[n_fft], n_fft, case, gpu_device, idx=(2,)).run().result()
    assert torch.equal(solo["out"][0], base["out"][2])
    assert torch.equal(_bytes(solo["G"][0]), _bytes(base["G"][2]))
    assert torch.equal(solo["state"], base["state"][2 * per:])
    # a NaN hop in stream 1 leaves streams 0 and 2 alone
    mix = WC.inputs(n_fft, T).copy()
    mix[1, :, 4 * H:5 * H] = np.nan
    bad = Runner(plans[n_fft], n_fft, case, gpu_device, mix=mix).run().result()
    assert torch.isnan(bad["out"][1]).any()
    for s in (0, 2):
        assert torch.equal(bad["out"][s], base["out"][s])
        assert torch.equal(_bytes(bad["G"][s]), _bytes(base["G"][s]))
        assert torch.equal(bad["state"][s * per:(s + 1) * per], base["state"][s * per:(s + 1) * per])
    # active = 0: the stream's state and its rows of out stay; the others go on as ever
    r = Runner(plans[n_fft], n_fft, case, gpu_device)
    r.push(5).push(1)
    torch.cuda.synchronize()
    before = r.state[per:2 * per].clone()
    r.out[1, :, 6 * H:T * H] = 7.5
    r.mix[1, :, 6 * H:T * H] = torch.roll(r.mix[1, :, 6 * H:T * H], -17 * H, dims=1)
    rest = WC.groupings(case)["ragged"][2:]
    r.push(rest[0], active=[1, 0, 1])
    torch.cuda.synchronize()
    assert torch.equal(r.state[per:2 * per], before)
    assert (r.out[1, :, 6 * H:T * H] == 7.5).all()
    for g in rest[1:]:
        r.push(g, active=[1, 0, 1])
    got = r.result()
    for s in (0, 2):
        assert torch.equal(got["out"][s], base["out"][s])
        assert torch.equal(got["state"][s * per:(s + 1) * per], base["state"][s * per:(s + 1) * per])


@pytest.mark.parametrize("n_fft", WC.SIZES)
def test_adapt_zero_freezes_the_filter(plans, gpu_device, ragged, n_fft):
    case = "k10"
    T, H = WC.CASES[case]["T"], n_fft // 2
    r = Runner(plans[n_fft], n_fft, case, gpu_device)
    r.push(3).push(6)                                             # hops 0 .. 8 adapt
    torch.cuda.synchronize()
    g8 = r.G.clone()
    r.push(1, adapt=[1, 0, 1]).push(T - 10, adapt=[1, 0, 1])
    got = r.result()
    assert torch.equal(_bytes(got["G"][1]), _bytes(g8[1]))
    base = ragged(n_fft, case)
    for s in (0, 2):                                              # the others adapted as ever
        assert torch.equal(got["out"][s], base["out"][s])
    assert not torch.equal(got["out"][1], base["out"][1])
    flags = np.ones(T, dtype=int)
    flags[9:] = 0
    ref = WC.reference(n_fft, case, 1, key="adapt9", adapt=flags)
    tol_o, tol_g = WC.tolerance(ref)
    out = got["out"][1].cpu().numpy().astype(np.float64)
    e_o = np.abs(out - ref["out"]).max()
    e_g = np.abs(got["G"][1].cpu().numpy() - ref["G"]).max()
    print(f"N={n_fft}: frozen from hop 9: out error {e_o:.3e} / tol {tol_o:.3e}, G error "
          f"{e_g:.3e} / tol {tol_g:.3e}")
    assert e_o <= tol_o and e_g <= tol_g
    # the frozen filter still filters: its output is not the input delayed
    delayed = r.mix[1, :, 11 * H:(T - 2) * H].cpu().numpy()
    assert np.abs(out[:, 12 * H:(T - 1) * H] - delayed).max() > 100 * tol_o


def test_every_refusal_happens_before_any_device_work(plans, gpu_device):
    n_fft, case = 512, "k10"
    r = Runner(plans[n_fft], n_fft, case, gpu_device, debug=False)
    r.push(2)
    torch.cuda.synchronize()
    H = r.H
    r.out[:] = 3.25
    state0 = r.state.clone()
    row = 4 * H
    ARG, SHAPE, ALIGN = _lib.AVZ_ERR_ARG, _lib.AVZ_ERR_SHAPE, _lib.AVZ_ERR_ALIGN
    big = r.nbytes
    cases = [(dict(taps=0), ARG), (dict(taps=17), ARG), (dict(delay=0), ARG),
             (dict(delay=9), ARG), (dict(forget=0.0), ARG), (dict(forget=1.5), ARG),
             (dict(power_floor=0.0), ARG), (dict(hops=0), ARG),
             (dict(streams=0), SHAPE), (dict(streams=WC.STREAMS + 1), SHAPE),
             (dict(ch_stride=row - 4), SHAPE), (dict(out_ch_stride=row - 4), SHAPE),
             (dict(mix_stride=r.mix.stride(1) + row - 4), SHAPE),
             (dict(out_stride=r.out.stride(1) + row - 4), SHAPE),
             (dict(state_bytes=big - 256), SHAPE),
             (dict(state=_p(r.state, 128)), ALIGN), (dict(out=_p(r.out, 2)), ALIGN),
             (dict(out_stride=r.out.stride(0) + 2), ALIGN),
             (dict(out_ch_stride=r.out.stride(1) + 2), ALIGN),
             # taps / delay other than the reset's (the state is large enough for them)
             (dict(taps=9), ARG), (dict(delay=2), ARG), (dict(taps=2, delay=1), ARG)]
    for over, want in cases:
        over = dict(over)
        a = r.args(over.pop("hops", 4), **over)
        rc = _lib.lib.avz_wpe_stream_push(r.plan._h, ct.byref(a), None)
        assert rc == want, (over, rc, want)
    lib = _lib.lib
    assert lib.avz_wpe_stream_reset(r.plan._h, _p(r.state), r.nbytes, r.S, 10, 3, 0.0, None,
                                    None) == ARG
    assert lib.avz_wpe_stream_reset(r.plan._h, _p(r.state), r.nbytes, r.S, 17, 3, 1.0, None,
                                    None) == ARG
    assert lib.avz_wpe_stream_reset(r.plan._h, _p(r.state), r.nbytes - 256, r.S, 10, 3, 1.0,
                                    None, None) == SHAPE
    assert lib.avz_wpe_stream_reset(r.plan._h, _p(r.state, 64), r.nbytes, r.S, 10, 3, 1.0, None,
                                    None) == ALIGN
    sel = torch.ones(r.S, dtype=torch.int32, device=gpu_device)
    # a partial reset may not change the buffer's taps
    assert lib.avz_wpe_stream_reset(r.plan._h, _p(r.state), r.nbytes, r.S, 9, 3, 1.0, _p(sel),
                                    None) == ARG
    assert lib.avz_wpe_stream_state_bytes(r.plan._h, r.S, 0, 3) == ARG
    assert lib.avz_wpe_stream_state_bytes(r.plan._h, WC.STREAMS + 1, 10, 3) == SHAPE
    torch.cuda.synchronize()
    assert (r.out == 3.25).all() and torch.equal(r.state, state0)
    r.out[:] = NAN
    # and the stream goes on where it was
    r.push(3).push(1).push(17).push(8).push(9).push(8)
    base = Runner(plans[n_fft], n_fft, case, gpu_device, debug=False).run().result()
    got = r.result()
    assert torch.equal(got["out"][:, :, 2 * H:], base["out"][:, :, 2 * H:])
    assert torch.equal(got["state"], base["state"])


def test_select_reset_restarts_one_stream(plans, gpu_device, ragged):
    n_fft, case = 512, "k2"
    base = ragged(n_fft, case)
    r = Runner(plans[n_fft], n_fft, case, gpu_device)
    r.push(7)
    r.reset(select=[0, 1, 0])
    r.j = 0
    r.out[:] = NAN
    r.push(18, active=[0, 1, 0])
    got = r.result()
    assert torch.equal(got["out"][1], base["out"][1])
    assert torch.equal(_bytes(got["G"][1]), _bytes(base["G"][1]))


@pytest.mark.parametrize("n_fft", [512])
def test_wpe_into_the_beamformer(plans, gpu_device, n_fft):
    import avz
    case, cfg = "k10", SC.CONFIGS["floor"]
    T, H, F = WC.CASES[case]["T"], n_fft // 2, n_fft // 2 + 1
    dev = gpu_device
    rng = np.random.default_rng(9100 + n_fft)
    M = rng.random((WC.STREAMS, F, T)).astype(np.float32)
    M[:, :, 0] = 1.0      # the WPE's all-zero first hop adds nothing to the beamformer's sums
    mix = WC.inputs(n_fft, T)
    bf_plan = avz.MVDRPlan(n_fft=n_fft, normalize="none", max_batch=WC.STREAMS,
                           max_samples=T * H, **cfg)
    wpe = DV.StreamingWPE(plans[n_fft], WC.STREAMS, device=dev, **WC.params(case))
    bf = ST.StreamingBeamformer(bf_plan, WC.STREAMS, forget=1.0, device=dev)
    x, Md = torch.from_numpy(mix).to(dev), torch.from_numpy(M).to(dev)
    outs, j = [], 0
    for g in WC.groupings(case)["ragged"]:
        d = wpe.push(x[:, :, j * H:(j + g) * H].contiguous())
        outs.append(bf.push(d, mask=Md[:, :, j:j + g].contiguous()))
        j += g
    got = torch.cat(outs, dim=1).cpu().numpy().astype(np.float64)
    ncfg = dict(cfg)
    ncfg["mask_mode"] = ncfg.pop("mask")
    tols = []
    for s in range(WC.STREAMS):
        ref = WC.reference(n_fft, case, s)
        d32 = ref["out"].astype(np.float32)                       # the WPE hands float32 on
        run = lambda hook=None: ST.stream_numpy(d32, mask=M[s], drain=False, n_fft=n_fft,  # noqa
                                                forget=1.0, y_hook=hook, **ncfg)
        o, st = run()
        ymax = max(np.abs(y).max() for y in st.hist["Y"])
        prng, e_bf = np.random.default_rng(2024 + s), 0.0
        for _ in range(8):
            u = [prng.uniform(-1, 1, (2, F)) + 1j * prng.uniform(-1, 1, (2, F)) for _ in range(T)]
            u = [v / np.maximum(np.abs(v), 1.0) for v in u]
            e_bf = max(e_bf, np.abs(run(lambda t, Y: Y + SC.STAGE * ymax * u[t])[0] - o).max())
        tol = WC.tolerance(ref)[0] + 4 * e_bf + 2.0 ** -23 * np.abs(o).max()
        err = np.abs(got[s] - o).max()
        print(f"N={n_fft}[{s}]: composed error {err:.3e} / tol {tol:.3e} (WPE tol "
              f"{WC.tolerance(ref)[0]:.2e}, beamformer E_pert {e_bf:.2e}, max|out| "
              f"{np.abs(o).max():.3f})")
        assert err <= tol and np.all(got[s][:H] == 0.0)
        tols.append(tol)
    # the same through the whole-file forms: apply_wpe_stream, then enhance_stream
    s = 0
    dry = DV.apply_wpe_stream(mix[s], n_fft=n_fft, hops_per_push=5, device=dev,
                              **WC.params(case))
    assert dry.shape == mix[s].shape and dry.dtype == np.float32
    odd = DV.apply_wpe_stream(mix[s][:, :T * H - 37], n_fft=n_fft, device=dev, **WC.params(case))
    assert odd.shape == (2, T * H - 37)
    mask_fn = lambda j0, blk: Md[s, :, j0 + 1:j0 + 1 + blk.shape[1] // H] if \
        j0 + 1 + blk.shape[1] // H <= T else \
        torch.cat([Md[s, :, j0 + 1:], torch.ones((F, 1), device=dev)], dim=1)  # noqa: E731
    whole = ST.enhance_stream(dry, mask_fn, hops_per_push=7, n_fft=n_fft, forget=1.0,
                              device=dev, sigma=cfg["sigma"], mic_d=cfg["mic_d"],
                              postfilter=cfg["postfilter"], pf_floor=cfg["pf_floor"])
    err = np.abs(whole[:(T - 2) * H] - got[s][2 * H:]).max()
    print(f"whole-file forms against the pushed pair: {err:.3e} / tol {tols[s]:.3e}")
    assert err <= tols[s]
