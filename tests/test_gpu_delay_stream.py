"""avz_delay_stream_push on the device against the fp64 restatement
avz.delay_mask.delay_mask_stream_numpy.

Inputs: tests/delay_stream_cases.py (four (N, d) cases, three streams of 18 pushed hops in
NaN-filled rows with padded strides, groupings [18], [1] * 18 and [3, 1, 8, 6], forget 1.0 and
0.9; every output buffer is pre-filled with NaN or a sentinel and the mask is padded in every
stride). Tolerances come from eight seeded perturbations of the restatement's input Y by 2e-6
max|Y|, the repository's STFT tolerance, per frame t:
  histogram  |h_gpu - h_ref| <= 4 E_pert(t) + 2^-20 max h_t, for hist_out after every call of
             every grouping (the [1] * 18 run gives every frame's);
  peaks      the restatement's stage 2 on the kernel's own h_t: the same J and bins, delays
             within 1e-9 samples, on every frame; on the frames whose peak bins no perturbation
             changes: the restatement's J_t and bins, delays within 4 D_pert(t) + 1e-6;
  mask       with the kernel's lists, equal to the restatement's on every decision that no
             perturbation flips; at most 1 % of a stream's decisions may be such.
The bitwise tests compare masks, lists, counts, hist_out and the whole state buffer.
Measured on an MI355X: DESIGN.md section 19."""
import ctypes as ct

import numpy as np
import pytest

import delay_mask_cases as DC
import delay_stream_cases as SC
from avz import _lib
from avz import delay_mask as DM

pytestmark = pytest.mark.gpu

SENT = -7.25  # sentinel of the fp64 outputs (NaN is a value delays_out may hold)
T = SC.T
_PLANS = {}


def _plan(n_fft, d, max_samples=None, max_batch=3):
    import avz
    key = (n_fft, d, max_samples, max_batch)
    if key not in _PLANS:
        _PLANS[key] = avz.MVDRPlan(n_fft=n_fft, mic_d=d, max_batch=max_batch, sigma=1e-5,
                                   mask="external", postfilter="floor", normalize="none",
                                   max_samples=max_samples or T * (n_fft // 2))
    return _PLANS[key]


def _per_call(v, ci):
    if v is None:
        return None
    return v[ci] if isinstance(v, list) else v


class Run:
    """The three (or `order`) streams pushed through the C ABI in `groups`, on sentinel-filled,
    padded buffers: mask [B, F + 2, T + 3] (NaN-filled; call c writes columns j0 .. j0 + g),
    delays [B, T, 8], n [B, T], hists [calls][B, nb] (hist_out after each call), state
    [B, stride] bytes after the last call, rc of each push."""

    def __init__(self, dev, n_fft, d, groups, forget=1.0, order=(0, 1, 2), scale=1.0,
                 nan_rows=(), active=None, adapt=None, angles=None, hist_bins=65, push_bins=None,
                 x=None, reset_after=None, smooth=3, max_peaks=3, rel_height=0.25):
        import torch
        lib = _lib.lib
        plan = _plan(n_fft, d)
        H, F, B = n_fft // 2, n_fft // 2 + 1, len(order)
        x = (SC.inputs(n_fft, d) if x is None else x)[list(order)] * np.float32(scale)
        hops = x.shape[2] // H
        assert sum(groups) == hops
        ch = hops * H + 13
        buf = np.full((B, 2 * ch + 11), np.nan, np.float32)
        buf[:, :hops * H], buf[:, ch:ch + hops * H] = x[:, 0], x[:, 1]
        for r in nan_rows:
            buf[r] = np.nan
        mix = torch.from_numpy(buf).to(dev)
        mask = torch.full((B, F + 2, hops + 3), float("nan"), dtype=torch.float32, device=dev)
        need = lib.avz_delay_stream_state_bytes(plan._h, B, hist_bins)
        assert need > 0 and need % (256 * B) == 0
        state = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)  # no reliance on zeros
        stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.avz_delay_stream_reset(plan._h, state.data_ptr(), need, B, hist_bins, None,
                                              stream), "avz_delay_stream_reset")
        ang = None if angles is None else torch.tensor(angles, dtype=torch.float64, device=dev)
        keep, self.rc = [], []
        delays, n, hists = [], [], []
        j0 = 0
        for ci, g in enumerate(groups):
            dl = torch.full((B, g, 8), SENT, dtype=torch.float64, device=dev)
            nn = torch.full((B, g), -99, dtype=torch.int32, device=dev)
            hh = torch.full((B, hist_bins), SENT, dtype=torch.float64, device=dev)
            a = _lib.AvzDelayStreamArgs(
                streams=B, hops=g, forget=forget, mix=mix.data_ptr() + 4 * j0 * H,
                mix_stride=buf.shape[1], ch_stride=ch, hist_bins=push_bins or hist_bins,
                smooth=smooth, max_peaks=max_peaks, rel_height=rel_height, min_sep=0.2,
                f_lo_hz=100.0,
                mask=mask.data_ptr() + 4 * j0, mask_stride_b=mask.stride(0),
                mask_stride_f=mask.stride(1), mask_stride_t=1, hist_out=hh.data_ptr(),
                delays_out=dl.data_ptr(), n_peaks=nn.data_ptr(), state=state.data_ptr(),
                state_bytes=need)
            for name, v in (("active", active), ("adapt", adapt)):
                v = _per_call(v, ci)
                if v is not None:
                    t = torch.tensor(v, dtype=torch.int32, device=dev)
                    keep.append(t)
                    setattr(a, name, t.data_ptr())
            if ang is not None:
                a.angle_deg = ang.data_ptr()
            self.rc.append(lib.avz_delay_stream_push(plan._h, ct.byref(a), stream))
            if reset_after is not None and ci == reset_after[0]:
                sel = torch.tensor(reset_after[1], dtype=torch.int32, device=dev)
                keep.append(sel)
                _lib.check(lib.avz_delay_stream_reset(plan._h, state.data_ptr(), need, B, hist_bins,
                                                      sel.data_ptr(), stream), "reset")
            delays.append(dl), n.append(nn), hists.append(hh)
            j0 += g
        torch.cuda.synchronize()
        self.F, self.hops, self.ends = F, hops, np.cumsum(groups) - 1
        self.mask = mask.cpu().numpy()
        self.delays = torch.cat(delays, dim=1).cpu().numpy()
        self.n = torch.cat(n, dim=1).cpu().numpy()
        self.hists = [h.cpu().numpy() for h in hists]
        self.state = state.cpu().numpy().reshape(B, -1)

    def bits(self, r):
        """Everything the bitwise guarantees cover, of stream row r."""
        return (self.mask[r].tobytes(), self.delays[r].tobytes(), self.n[r].tobytes(),
                self.hists[-1][r].tobytes(), self.state[r].tobytes())

    def ok(self):
        assert all(rc == _lib.AVZ_OK for rc in self.rc), self.rc
        return self


_RUNS = {}


def shared(dev, n_fft, d, name, forget):
    """The plain run of a case, grouping and forget, made once."""
    k = (n_fft, d, name, forget)
    if k not in _RUNS:
        _RUNS[k] = Run(dev, n_fft, d, SC.GROUPINGS[name], forget).ok()
    return _RUNS[k]


def check_stream(run, r, ref, tag, frames=None):
    """The module docstring's criteria for stream row r of a run whose every call is one hop
    (hists[t] is h_t), against the restatement `ref`, on `frames` (default all)."""
    F, n_fft, g = run.F, ref["n_fft"], ref["grid"]
    frames = range(run.hops) if frames is None else frames
    worst_h = worst_own = worst_ref = 0.0
    for t in frames:
        h, J, gd = run.hists[t][r], int(run.n[r, t]), run.delays[r, t]
        tol = SC.hist_tolerance(ref, t)
        err = np.abs(h - ref["h"][t]).max()
        worst_h = max(worst_h, err / tol)
        assert err <= tol, (tag, t, err, tol)
        d2, J2, bins2 = DM.delay_peaks(h, g, ref["angle"])
        assert J == J2 and np.isnan(gd[1 + J:]).all(), (tag, t, J, J2)
        e_own = np.abs(gd[:1 + J] - d2[:1 + J]).max()
        worst_own = max(worst_own, e_own)
        assert e_own <= 1e-9, (tag, t, e_own)
        if ref["stable"][t]:
            assert J == ref["J"][t] and bins2 == ref["bins"][t], (tag, t, bins2, ref["bins"][t])
            e_ref = np.abs(gd[:1 + J] - ref["lists"][t, :1 + J]).max()
            tol_d = 4 * ref["d_pert"][t] + 1e-6
            worst_ref = max(worst_ref, e_ref / tol_d)
            assert e_ref <= tol_d, (tag, t, e_ref, tol_d)
    M, stable = SC.stable_labels(ref, run.delays[r], run.n[r])
    Mg = run.mask[r]
    cols = np.array(list(frames))
    diff = (Mg[:F, :run.hops] != M)[:, cols]
    flipped = 1.0 - stable.mean()
    print(f"{tag}: hist error <= {worst_h:.2e} of its tolerance, delays {worst_own:.1e} from "
          f"stage 2 on h_t and <= {worst_ref:.2e} of 4 D_pert + 1e-6 from the restatement's, "
          f"{int((~ref['stable']).sum())} unstable frames, {100 * flipped:.3f} % of the "
          f"decisions flip under a perturbation, {int(diff.sum())} of {diff.size} differ")
    assert flipped <= 0.01
    assert not (diff & stable[:, cols]).any()
    assert np.isin(Mg[:F, cols], (0.0, 1.0)).all() and (Mg[0, cols] == 1.0).all()
    # the padding bins and the padding frames keep their NaN
    assert np.isnan(Mg[F:]).all() and np.isnan(Mg[:, run.hops:]).all()


@pytest.mark.parametrize("forget", SC.FORGETS)
@pytest.mark.parametrize("n_fft,d", SC.CASES)
def test_histograms_lists_and_masks_match_the_restatement(gpu_device, n_fft, d, forget):
    single = shared(gpu_device, n_fft, d, "single", forget)
    for s in range(SC.STREAMS):
        ref = SC.reference(n_fft, d, s, forget)
        check_stream(single, s, ref, f"N={n_fft} d={d} forget={forget} [{s}]")
        for name in ("one", "ragged"):
            run = shared(gpu_device, n_fft, d, name, forget)
            for c, t in enumerate(run.ends):
                err = np.abs(run.hists[c][s] - ref["h"][t]).max()
                assert err <= SC.hist_tolerance(ref, t), (name, s, t, err)


@pytest.mark.parametrize("n_fft,d", SC.CASES)
def test_bitwise_guarantees(gpu_device, n_fft, d):
    dev, fg = gpu_device, 0.9
    base = shared(dev, n_fft, d, "ragged", fg)
    names = ("mask", "delays", "n_peaks", "hist_out", "state")

    def same(a, ra, b, rb, what):
        for nm, x, y in zip(names, a.bits(ra), b.bits(rb)):
            assert x == y, (what, nm)

    # the three groupings, for both forgets; hist_out also wherever two groupings' calls end
    for forget in SC.FORGETS:
        runs = {k: shared(dev, n_fft, d, k, forget) for k in SC.GROUPINGS}
        for k in ("single", "ragged"):
            for r in range(SC.STREAMS):
                same(runs["one"], r, runs[k], r, (forget, k, r))
        for c, t in enumerate(runs["ragged"].ends):
            assert runs["ragged"].hists[c].tobytes() == runs["single"].hists[t].tobytes(), t
    # call to call
    again = Run(dev, n_fft, d, SC.GROUPINGS["ragged"], fg).ok()
    for r in range(SC.STREAMS):
        same(base, r, again, r, ("again", r))
    # a stream alone equals the same stream at index 2 of 3
    for i, order in enumerate(((1, 2, 0), (2, 0, 1), (0, 1, 2))):
        three = Run(dev, n_fft, d, SC.GROUPINGS["ragged"], fg, order=order).ok()
        alone = Run(dev, n_fft, d, SC.GROUPINGS["ragged"], fg, order=(i,)).ok()
        same(three, 2, alone, 0, ("alone", i))
        same(three, 2, base, i, ("index", i))
    # a NaN-filled neighbour leaves the others' bits alone and gets M = 1, J = 0, h = 0
    nan = Run(dev, n_fft, d, SC.GROUPINGS["ragged"], fg, nan_rows=(1,)).ok()
    for r in (0, 2):
        same(nan, r, base, r, ("nan neighbour", r))
    assert (nan.n[1] == 0).all() and (nan.mask[1][:nan.F, :T] == 1.0).all()
    assert not nan.hists[-1][1].any() and np.isnan(nan.delays[1][:, 1:]).all()
    # input x 2^-10: identical masks and lists, h scaled exactly
    low = Run(dev, n_fft, d, SC.GROUPINGS["ragged"], fg, scale=2.0 ** -10).ok()
    assert low.mask.tobytes() == base.mask.tobytes()
    assert low.delays.tobytes() == base.delays.tobytes() and low.n.tobytes() == base.n.tobytes()
    for a, b in zip(low.hists, base.hists):
        assert (a * 4.0 ** 10).tobytes() == b.tobytes()


def test_active_adapt_reset_angles_and_hist_bins(gpu_device):
    dev, n_fft, d, fg = gpu_device, 512, 0.08, 0.9
    single = [1] * T
    base = shared(dev, n_fft, d, "single", fg)
    F = base.F
    # active = 0 for stream 1 during hops 5 .. 8: its state and output rows stay untouched, and
    # it goes on as if those hops had never been pushed
    act = [[1, 0 if 5 <= t < 9 else 1, 1] for t in range(T)]
    run = Run(dev, n_fft, d, single, fg, active=act).ok()
    for r in (0, 2):
        assert run.bits(r) == base.bits(r)
    assert np.isnan(run.mask[1][:, 5:9]).all()
    assert (run.delays[1, 5:9] == SENT).all() and (run.n[1, 5:9] == -99).all()
    for t in range(5, 9):
        assert (run.hists[t][1] == SENT).all()
    x = SC.inputs(n_fft, d)
    H = n_fft // 2
    skipped = np.concatenate([x[:, :, :5 * H], x[:, :, 9 * H:]], axis=2)
    short = Run(dev, n_fft, d, [1] * (T - 4), fg, x=skipped).ok()
    assert run.state[1].tobytes() == short.state[1].tobytes()
    assert run.mask[1][:F, 9:T].tobytes() == short.mask[1][:F, 5:T - 4].tobytes()
    assert run.delays[1, 9:].tobytes() == short.delays[1, 5:].tobytes()
    # adapt = 0 for stream 0 during hops 5 .. 8 freezes h while the labels continue
    flags = np.ones(T, int)
    flags[5:9] = 0
    run = Run(dev, n_fft, d, single, fg, adapt=[[int(flags[t]), 1, 1] for t in range(T)]).ok()
    for r in (1, 2):
        assert run.bits(r) == base.bits(r)
    for t in range(5, 9):
        assert run.hists[t][0].tobytes() == run.hists[4][0].tobytes()
        assert run.delays[0, t].tobytes() == run.delays[0, 4].tobytes()
    assert len({run.mask[0][:F, t].tobytes() for t in range(5, 9)}) > 1
    check_stream(run, 0, SC.reference(n_fft, d, 0, fg, adapt=flags, key="gate"), "adapt gate")
    # reset of stream 1 after hop 8 leaves the others alone and restarts it
    run = Run(dev, n_fft, d, single, fg, reset_after=(8, [0, 1, 0])).ok()
    for r in (0, 2):
        assert run.bits(r) == base.bits(r)
    late = Run(dev, n_fft, d, [1] * (T - 9), fg, x=x[:, :, 9 * H:]).ok()
    assert run.state[1].tobytes() == late.state[1].tobytes()
    assert run.mask[1][:F, 9:T].tobytes() == late.mask[1][:F, :T - 9].tobytes()
    # per-stream angle_deg: stream 0 steered to 40 degrees, a NaN entry = the plan's
    st = Run(dev, n_fft, d, single, fg, angles=[40.0, float("nan"), 90.0]).ok()
    for r in (1, 2):
        assert st.bits(r) == base.bits(r)
    ref40 = SC.reference(n_fft, d, 0, fg, angle=40.0)
    check_stream(st, 0, ref40, "steered to 40")
    assert abs(st.delays[0, 0, 0] / ref40["grid"].dmax - 0.766) < 1e-3
    assert st.hists[-1][0].tobytes() == base.hists[-1][0].tobytes()
    # a push with another hist_bins than the buffer's is refused; so is one on a buffer never reset
    bad = Run(dev, n_fft, d, [T], fg, push_bins=33)
    assert bad.rc == [_lib.AVZ_ERR_ARG]
    assert np.isnan(bad.mask).all() and (bad.hists[0] == SENT).all()
    # (an address 256 bytes into an allocation: the allocator hands out 512-byte aligned blocks,
    # so no earlier buffer of this process began there)
    import torch
    plan = _plan(n_fft, d)
    need = _lib.lib.avz_delay_stream_state_bytes(plan._h, 1, 65)
    fresh = torch.zeros(need + 256, dtype=torch.uint8, device=dev)
    assert fresh.data_ptr() % 512 == 0
    mix = torch.zeros((1, 2, H), dtype=torch.float32, device=dev)
    m = torch.ones((1, F, 1), dtype=torch.float32, device=dev)
    a = _lib.AvzDelayStreamArgs(streams=1, hops=1, forget=1.0, mix=mix.data_ptr(), mix_stride=2 * H,
                                ch_stride=H, hist_bins=65, smooth=3, max_peaks=3, rel_height=0.25,
                                min_sep=0.2, f_lo_hz=100.0, mask=m.data_ptr(), mask_stride_b=F,
                                mask_stride_f=1, mask_stride_t=1, state=fresh.data_ptr() + 256,
                                state_bytes=need)
    assert _lib.lib.avz_delay_stream_push(plan._h, ct.byref(a), None) == _lib.AVZ_ERR_ARG


@pytest.mark.parametrize("n_fft,d,nb", [(1024, 0.08, 9), (512, 0.01, 257)])
def test_zero_frames_and_other_histogram_sizes(gpu_device, n_fft, d, nb):
    """hist_bins 9 (28 scan segments per bin) and 257 (more bins than threads) against the
    restatement's histogram; then a stream of digital zeros: nothing deposited, no peak, M = 1."""
    dev = gpu_device
    run = Run(dev, n_fft, d, SC.GROUPINGS["ragged"], 0.9, hist_bins=nb).ok()
    one = Run(dev, n_fft, d, SC.GROUPINGS["one"], 0.9, hist_bins=nb).ok()
    g = DM.delay_grid(n_fft, SC.FS, d, SC.C_SOUND, nb)
    for s in range(SC.STREAMS):
        assert run.bits(s) == one.bits(s)
        Y = SC.spectra(n_fft, d, s)
        h = DM.delay_mask_stream_numpy(Y[0], Y[1], n_fft, SC.FS, d, SC.C_SOUND, hist_bins=nb,
                                       forget=0.9)[1][-1]
        e_pert = 0.0
        for p in DC.perturbations(Y, 5100 + s):
            Yp = Y + p
            hp = DM.delay_mask_stream_numpy(Yp[0], Yp[1], n_fft, SC.FS, d, SC.C_SOUND,
                                            hist_bins=nb, forget=0.9)[1][-1]
            e_pert = max(e_pert, np.abs(hp - h).max())
        err = np.abs(run.hists[-1][s] - h).max()
        print(f"hist_bins {nb} [{s}]: hist error {err / h.max():.2e} of max h (E_pert "
              f"{e_pert / h.max():.2e})")
        assert err <= 4 * e_pert + 2.0 ** -20 * h.max()
        d2, J2, _ = DM.delay_peaks(run.hists[-1][s], g)
        assert run.n[s, -1] == J2
        assert np.abs(run.delays[s, -1][:1 + J2] - d2[:1 + J2]).max() <= 1e-9
    H = n_fft // 2
    x = SC.inputs(n_fft, d).copy()
    x[1] = 0.0
    x[2, :, :4 * H] = 0.0     # four zero frames, then the scene
    z = Run(dev, n_fft, d, SC.GROUPINGS["ragged"], 0.9, hist_bins=nb, x=x).ok()
    assert z.bits(0) == run.bits(0)
    assert (z.mask[1][:z.F, :T] == 1.0).all() and (z.n[1] == 0).all()
    assert not z.hists[-1][1].any() and np.isnan(z.delays[1][:, 1:]).all()
    assert (z.mask[2][:z.F, :4] == 1.0).all() and (z.n[2, :4] == 0).all()
    assert (z.n[2, 5:] > 0).any() and (z.mask[2][:z.F, 5:T] == 0.0).any()


def test_peak_rule_extremes(gpu_device):
    """The peak stage off its defaults, rel_height 0.01: (smooth, max_peaks) = (0, 0) (no pass,
    nothing kept: J = 0 and M = 1), (0, 7) (no pass, the cap binds and the list is full: no NaN
    fill) and (8, 7) (eight passes). N = 512, d = 0.08, forget 0.9, streams 0 and 1, their first
    9 hops pushed as 8 + 1: a full group of frames and a one-frame group; the fp64 restatement
    alone keeps 7 peaks on most of these frames at (0, 7). h_t is hist_out of the same hops pushed
    one by one; stage 2 of the restatement on it: the same J, delays within 1e-9, NaN beyond J."""
    dev, n_fft, d, rh, hops = gpu_device, 512, 0.08, 0.01, 9
    x = SC.inputs(n_fft, d)[:, :, :hops * (n_fft // 2)]
    g = DM.delay_grid(n_fft, SC.FS, d, SC.C_SOUND, 65)
    for smooth, max_peaks in ((0, 0), (0, 7), (8, 7)):
        kw = dict(order=(0, 1), x=x, smooth=smooth, max_peaks=max_peaks, rel_height=rh)
        one = Run(dev, n_fft, d, [1] * hops, 0.9, **kw).ok()
        run = Run(dev, n_fft, d, [8, 1], 0.9, **kw).ok()
        for c, t in enumerate(run.ends):
            assert run.hists[c].tobytes() == one.hists[t].tobytes(), t
        worst = 0.0
        for s in range(2):
            assert run.bits(s) == one.bits(s)
            for t in range(hops):
                J, gd = int(run.n[s, t]), run.delays[s, t]
                d2, J2, _ = DM.delay_peaks(one.hists[t][s], g, 90.0, smooth=smooth, rel_height=rh,
                                           max_peaks=max_peaks)
                assert J == J2 and np.isnan(gd[1 + J:]).all(), (s, t, J, J2)
                worst = max(worst, np.abs(gd[:1 + J] - d2[:1 + J]).max())
        print(f"smooth {smooth} max_peaks {max_peaks}: J {run.n.tolist()}, delays {worst:.1e} "
              f"from stage 2 on h_t")
        assert worst <= 1e-9
        if max_peaks == 0:
            assert (run.n == 0).all() and (run.mask[:, :run.F, :hops] == 1.0).all()
        if (smooth, max_peaks) == (0, 7):
            assert (run.n == 7).any()  # the cap binds


def test_mask_columns_align_with_the_beamformer(gpu_device):
    """StreamingBlindBeamformer.push equals StreamingDelayMask.push, then StreamingBeamformer.push
    of the same hops with that mask, bitwise; the Python layer equals the C call."""
    import torch
    from avz import stream as ST
    dev, n_fft, d = gpu_device, 512, 0.08
    plan = _plan(n_fft, d)
    H = n_fft // 2
    x = torch.from_numpy(SC.inputs(n_fft, d)).to(dev)
    blind = ST.StreamingBlindBeamformer(plan, 3, forget=0.99, hist_forget=0.9, device=dev)
    masker = ST.StreamingDelayMask(plan, 3, forget=0.9, device=dev)
    bf = ST.StreamingBeamformer(plan, 3, forget=0.99, device=dev)
    base = shared(dev, n_fft, d, "ragged", 0.9)
    j0 = 0
    for g in SC.GROUPINGS["ragged"]:
        blk = x[:, :, j0 * H:(j0 + g) * H].contiguous()
        out = blind.push(blk)
        M = masker.push(blk)
        sep = bf.push(blk, mask=M)
        torch.cuda.synchronize()
        assert torch.equal(blind.mask, M) and torch.equal(out, sep)
        assert M.cpu().numpy().tobytes() == \
            np.ascontiguousarray(base.mask[:, :base.F, j0:j0 + g]).tobytes()
        assert masker.delays.cpu().numpy().tobytes() == \
            np.ascontiguousarray(base.delays[:, j0:j0 + g]).tobytes()
        j0 += g
    assert masker.hist.cpu().numpy().tobytes() == base.hists[-1].tobytes()
    assert torch.equal(blind.beamformer.cov, bf.cov)
    assert (out.abs().amax(dim=1) > 0).all() and torch.isfinite(out).all()
    assert torch.equal(blind.flush(), bf.push(torch.zeros_like(x[:, :, :H]),
                                              mask=masker.push(torch.zeros_like(x[:, :, :H]))))


def test_end_to_end_blind_streaming_enhancement(gpu_device):
    """enhance_blind_stream on the 4-s scene 0 (N = 1024, d = 0.08, SNR 20; external mask, floor
    0.05, sigma 1e-5, beamformer forget 0.99): the projection SIR is within 4 x the restatement
    chain's spread over the 8 perturbations of that chain's SIR, and beats the same device chain
    fed an all-zero mask by at least half the restatement's own gain."""
    import torch
    from avz import stream as ST
    e = SC.e2e_reference()
    kw = dict(n_fft=1024, mic_d=0.08, sigma=1e-5, forget=0.99, device=gpu_device)
    y = ST.enhance_blind_stream(e["mix"], hops_per_push=8, **kw)
    zero = ST.enhance_stream(e["mix"], lambda j0, blk: torch.zeros((513, blk.shape[1] // 512),
                                                                   device=blk.device),
                             hops_per_push=8, postfilter="floor", pf_floor=0.05, **kw)
    sir = DC.sir_db(y, e["tgt"], e["itf"])
    mpdr = DC.sir_db(zero, e["tgt"], e["itf"])
    print(f"SIR {sir:.3f} dB (restatement chain {e['sir']:.3f} dB, spread {e['spread']:.4f} dB), "
          f"all-zero mask {mpdr:.3f} dB (restatement {e['sir_mpdr']:.3f} dB)")
    assert abs(sir - e["sir"]) <= 4 * e["spread"]
    assert sir >= mpdr + 0.5 * (e["sir"] - e["sir_mpdr"])
    # the grouping does not change the output
    y1 = ST.enhance_blind_stream(e["mix"][:, :8 * 512], hops_per_push=1, **kw)
    y3 = ST.enhance_blind_stream(e["mix"][:, :8 * 512], hops_per_push=3, **kw)
    assert y1.tobytes() == y3.tobytes()
    # with the streaming WPE in front: two hops of delay trimmed, the same invariance
    short = e["mix"][:, :8 * 512 - 100]
    z1 = ST.enhance_blind_stream(short, hops_per_push=1, dereverb=True, **kw)
    z3 = ST.enhance_blind_stream(short, hops_per_push=3, dereverb=True, **kw)
    assert z1.shape == (short.shape[1],) and np.isfinite(z1).all() and np.abs(z1).max() > 0
    assert z1.tobytes() == z3.tobytes()
