"""avz_delay_mask on the device against the fp64 restatement avz.delay_mask.

Inputs: tests/delay_mask_cases.py (four (N, d) cases, three utterances of 18, 18 and 11 frames
in NaN-filled rows with padded strides; every output buffer is pre-filled with NaN or a
sentinel and padded in every stride). Tolerances come from eight seeded perturbations of the
restatement's input Y by 2e-6 max|Y|, the repository's STFT tolerance:
  histogram  |h_gpu - h_ref| <= 4 E_pert + 2^-20 max h;
  peaks      the restatement's stage 2 on the kernel's own hist_out: the same J and bins, delays
             within 1e-9 samples; against the restatement's own histogram: the same J and bins,
             delays within 4 D_pert + 1e-6 (the perturbed restatement must itself keep its peaks);
  mask       with the kernel's delays, equal to the restatement's on every decision that no
             perturbation flips; at most 1 % of an utterance's decisions may be such.
Measured on an MI355X: DESIGN.md section 17."""
import ctypes as ct

import numpy as np
import pytest

import delay_mask_cases as DC
from avz import _lib
from avz import delay_mask as DM
from oracle import avz_oracle as O

pytestmark = pytest.mark.gpu

SENT = -7.25  # sentinel of the fp64 outputs (NaN is a value delays_out may hold)
_PLANS = {}


def _plan(n_fft, d, max_samples=None, max_batch=3, **kw):
    import avz
    key = (n_fft, d, max_samples, max_batch, tuple(sorted(kw.items())))
    if key not in _PLANS:
        opts = dict(sigma=1e-5, mask="external", postfilter="floor", normalize="none")
        opts.update(kw)
        _PLANS[key] = avz.MVDRPlan(n_fft=n_fft, mic_d=d, max_batch=max_batch,
                                   max_samples=max_samples or 17 * (n_fft // 2), **opts)
    return _PLANS[key]


def run(dev, n_fft, d, order=(0, 1, 2), angles=None, scale=1.0, nan_rows=(), lens=None,
        hist_bins=65, smooth=3, max_peaks=3, rel_height=0.25):
    """One avz_delay_mask call through the C ABI on sentinel-filled, padded buffers:
    dict(mask [B, F + 2, T + 3] (NaN-filled), hist [B, nb], delays [B, 8], n [B], lens, T)."""
    import torch
    plan = _plan(n_fft, d, max_batch=max(3, len(order)))
    buf, ln, ch, max_len = DC.buffers(n_fft, d, order)
    buf = buf * np.float32(scale)
    for r in nan_rows:
        buf[r] = np.nan
    if lens is not None:
        ln = np.array(lens, np.int32)
    B, F, T = len(order), n_fft // 2 + 1, max_len // (n_fft // 2) + 1
    mix = torch.from_numpy(buf).to(dev)
    tl = torch.from_numpy(ln).to(dev)
    mask = torch.full((B, F + 2, T + 3), float("nan"), dtype=torch.float32, device=dev)
    hist = torch.full((B, hist_bins), SENT, dtype=torch.float64, device=dev)
    delays = torch.full((B, 8), SENT, dtype=torch.float64, device=dev)
    n = torch.full((B,), -99, dtype=torch.int32, device=dev)
    need = _lib.lib.avz_delay_mask_workspace_bytes(plan._h, B, max_len, hist_bins)
    assert need > 0 and need % 256 == 0
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=dev)  # the library must not rely on zeros
    a = _lib.AvzDelayMaskArgs(batch=B, len=tl.data_ptr(), max_len=max_len, mix=mix.data_ptr(),
                              mix_stride=buf.shape[1], ch_stride=ch, hist_bins=hist_bins,
                              smooth=smooth, max_peaks=max_peaks, rel_height=rel_height,
                              min_sep=0.2, f_lo_hz=100.0,
                              mask=mask.data_ptr(), mask_stride_b=mask.stride(0),
                              mask_stride_f=mask.stride(1), mask_stride_t=mask.stride(2),
                              hist_out=hist.data_ptr(), delays_out=delays.data_ptr(),
                              n_peaks=n.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=need)
    ang = None
    if angles is not None:
        ang = torch.tensor(angles, dtype=torch.float64, device=dev)
        a.angle_deg = ang.data_ptr()
    rc = _lib.lib.avz_delay_mask(plan._h, ct.byref(a), ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "avz_delay_mask")
    torch.cuda.synchronize()
    return dict(mask=mask.cpu().numpy(), hist=hist.cpu().numpy(), delays=delays.cpu().numpy(),
                n=n.cpu().numpy(), lens=ln, T=T, F=F)


def frames_of(L, n_fft):
    H = n_fft // 2
    return -(-int(L) // H) + 1


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_row(got, r, ref, n_fft, tag):
    """The module docstring's criteria for row r of a call against the restatement `ref`."""
    F, Tb = got["F"], frames_of(got["lens"][r], n_fft)
    h, J = got["hist"][r], int(got["n"][r])
    top = ref["h"].max()
    err = np.abs(h - ref["h"]).max()
    tol = 4 * ref["e_pert"] + 2.0 ** -20 * top
    print(f"{tag}: hist error {err / top:.2e} of max h (tolerance {tol / top:.2e}, E_pert "
          f"{ref['e_pert'] / top:.2e})")
    assert err <= tol
    # peaks: the restatement's stage 2 on the kernel's own histogram
    d2, J2, bins2 = DM.delay_peaks(h, ref["grid"], ref["angle"], **ref["peak_kw"])
    gd = got["delays"][r]
    assert J == J2 and np.isnan(gd[1 + J:]).all()
    e_own = np.abs(gd[:1 + J] - d2[:1 + J]).max()
    # ... and against the restatement's own histogram
    assert ref["same_peaks"], "the perturbed restatement must keep its own peaks"
    assert J == ref["J"] and bins2 == ref["bins"], (J, ref["J"], bins2, ref["bins"])
    e_ref = np.abs(gd[:1 + J] - ref["delays"][:1 + J]).max()
    print(f"{tag}: J {J}, delays {gd[:1 + J]}: {e_own:.1e} from stage 2 on hist_out, {e_ref:.1e} "
          f"from the restatement (D_pert {ref['d_pert']:.1e})")
    assert e_own <= 1e-9
    assert e_ref <= 4 * ref["d_pert"] + 1e-6
    # mask: with the kernel's delays, on every decision no perturbation flips
    M, stable = DC.stable_labels(ref, gd, J, n_fft)
    Mg = got["mask"][r]
    flipped = 1.0 - stable.mean()
    diff = (Mg[:F, :Tb] != M)
    print(f"{tag}: {100 * flipped:.3f} % of the decisions flip under a perturbation, "
          f"{int(diff.sum())} of {M.size} differ, target share {M.mean():.2f}")
    assert flipped <= 0.01
    assert not (diff & stable).any()
    assert np.isin(Mg[:F, :Tb], (0.0, 1.0)).all()
    # frames past the utterance, the padding bins and the padding frames keep their NaN
    assert np.isnan(Mg[:, Tb:]).all() and np.isnan(Mg[F:]).all()


def ref_of(n_fft, d, i, angle=90.0):
    r = dict(DC.reference(n_fft, d, i, angle))
    r["angle"] = angle
    return r


@pytest.mark.parametrize("n_fft,d", DC.CASES)
def test_histogram_peaks_and_mask_match_the_restatement(gpu_device, n_fft, d):
    got = run(gpu_device, n_fft, d)
    for i in range(DC.UTTS):
        check_row(got, i, ref_of(n_fft, d, i), n_fft, f"N={n_fft} d={d} [{i}]")


@pytest.mark.parametrize("n_fft,d", DC.CASES)
def test_guarantees(gpu_device, n_fft, d):
    base = run(gpu_device, n_fft, d)
    F = base["F"]
    # two calls: identical bits
    again = run(gpu_device, n_fft, d)
    for k in ("mask", "hist", "delays", "n"):
        assert same_bits(base[k], again[k]), k
    # an utterance alone equals the same utterance at index 2 of 3
    for i, order in enumerate(((1, 2, 0), (2, 0, 1), (0, 1, 2))):
        three = run(gpu_device, n_fft, d, order=order)
        alone = run(gpu_device, n_fft, d, order=(i,))
        for k in ("mask", "hist", "delays", "n"):
            assert same_bits(three[k][2], alone[k][0]), (i, k)
            assert same_bits(three[k][2], base[k][i]), (i, k)
    # a NaN-filled utterance leaves the others' bits alone and gets M = 1, J = 0
    nan = run(gpu_device, n_fft, d, nan_rows=(1,))
    for r in (0, 2):
        for k in ("mask", "hist", "delays", "n"):
            assert same_bits(nan[k][r], base[k][r]), (r, k)
    T1 = frames_of(nan["lens"][1], n_fft)
    assert nan["n"][1] == 0 and (nan["mask"][1][:F, :T1] == 1.0).all()
    assert np.isnan(nan["mask"][1][:, T1:]).all() and np.isnan(nan["mask"][1][F:]).all()
    assert not nan["hist"][1].any() and np.isnan(nan["delays"][1][1:]).all()
    # mixture x 2^-10: identical mask and delays, the histogram scaled exactly
    low = run(gpu_device, n_fft, d, scale=2.0 ** -10)
    for k in ("mask", "delays", "n"):
        assert same_bits(low[k], base[k]), k
    assert same_bits(low["hist"] * 4.0 ** 10, base["hist"])
    # angle_deg = 40 for row 0: the restatement's steered result; the other rows as with NULL
    st = run(gpu_device, n_fft, d, angles=[40.0, 90.0, 90.0])
    check_row(st, 0, ref_of(n_fft, d, 0, 40.0), n_fft, f"N={n_fft} d={d} [0] steered to 40")
    assert abs(st["delays"][0][0] / ref_of(n_fft, d, 0)["grid"].dmax - 0.766) < 1e-3
    assert same_bits(st["hist"], base["hist"])
    for r in (1, 2):
        for k in ("mask", "delays", "n"):
            assert same_bits(st[k][r], base[k][r]), (r, k)
    # a row shorter than n_fft reports -1 and nothing else of it is written
    short = run(gpu_device, n_fft, d, lens=[base["lens"][0], n_fft - 1, base["lens"][2]])
    assert short["n"][1] == -1
    assert np.isnan(short["mask"][1]).all()
    assert (short["hist"][1] == SENT).all() and (short["delays"][1] == SENT).all()
    for r in (0, 2):
        for k in ("mask", "hist", "delays", "n"):
            assert same_bits(short[k][r], base[k][r]), (r, k)


def test_other_histogram_sizes_and_the_python_wrapper(gpu_device):
    """hist_bins 9 and 257 (one scan segment per bin row instead of seven) against the
    restatement's histogram, and engine.delay_mask's outputs against the C call's."""
    import torch
    from avz import engine
    n_fft, d = 512, 0.08
    for nb in (9, 257):
        got = run(gpu_device, n_fft, d, hist_bins=nb)
        for i in range(DC.UTTS):
            ref = DC.reference_of(DC.utterances(n_fft, d)[i], n_fft, d, seed=4100 + i, hist_bins=nb)
            top = ref["h"].max()
            err = np.abs(got["hist"][i] - ref["h"]).max()
            print(f"hist_bins {nb} [{i}]: hist error {err / top:.2e} of max h "
                  f"(E_pert {ref['e_pert'] / top:.2e})")
            assert err <= 4 * ref["e_pert"] + 2.0 ** -20 * top
            d2, J2, _ = DM.delay_peaks(got["hist"][i], ref["grid"], 90.0)
            assert got["n"][i] == J2
            assert np.abs(got["delays"][i][:1 + J2] - d2[:1 + J2]).max() <= 1e-9
    base = run(gpu_device, n_fft, d)
    buf, ln, ch, max_len = DC.buffers(n_fft, d)
    rows = torch.from_numpy(buf).to(gpu_device)
    mix = torch.as_strided(rows, (3, 2, max_len), (buf.shape[1], ch, 1))
    M, hist, delays, n = engine.delay_mask(_plan(n_fft, d), mix, torch.from_numpy(ln).to(gpu_device),
                                           max_len=max_len, return_debug=True)
    torch.cuda.synchronize()
    assert tuple(M.shape) == (3, base["F"], base["T"])
    assert same_bits(hist.cpu().numpy(), base["hist"]) and same_bits(n.cpu().numpy(), base["n"])
    assert same_bits(delays.cpu().numpy(), base["delays"])
    for r in range(3):
        Tb = frames_of(ln[r], n_fft)
        assert same_bits(M[r, :, :Tb].cpu().numpy(), base["mask"][r][:base["F"], :Tb])
        assert (M[r, :, Tb:] == 0).all()     # a new mask starts as zeros


def test_peak_rule_extremes(gpu_device):
    """The peak stage off its defaults, rel_height 0.01: (smooth, max_peaks) = (0, 0) (no pass,
    nothing kept: J = 0 and M = 1), (0, 7) (no pass, the cap binds and the list is full: no NaN
    fill) and (8, 7) (eight passes). N = 512, d = 0.08, utterances 0 and 2 (18 and 11 frames);
    the fp64 restatement alone finds at least 10 candidates in utterance 0 at (0, 7). Stage 2 of
    the restatement on the kernel's own hist_out: the same J, delays within 1e-9, NaN beyond J."""
    n_fft, d, rh = 512, 0.08, 0.01
    g = DM.delay_grid(n_fft, DC.FS, d, DC.C_SOUND, 65)
    for smooth, max_peaks in ((0, 0), (0, 7), (8, 7)):
        got = run(gpu_device, n_fft, d, order=(0, 2), smooth=smooth, max_peaks=max_peaks,
                  rel_height=rh)
        Js = []
        for r in range(2):
            J, gd = int(got["n"][r]), got["delays"][r]
            d2, J2, _ = DM.delay_peaks(got["hist"][r], g, 90.0, smooth=smooth, rel_height=rh,
                                       max_peaks=max_peaks)
            e_own = np.abs(gd[:1 + J2] - d2[:1 + J2]).max()
            print(f"smooth {smooth} max_peaks {max_peaks} [{r}]: J {J} (stage 2 on hist_out {J2}), "
                  f"delays {e_own:.1e} from it")
            assert J == J2 and np.isnan(gd[1 + J:]).all()
            assert e_own <= 1e-9
            Js.append(J)
            if max_peaks == 0:
                Tb = frames_of(got["lens"][r], n_fft)
                assert J == 0 and (got["mask"][r][:got["F"], :Tb] == 1.0).all()
        if (smooth, max_peaks) == (0, 7):
            assert 7 in Js  # the cap binds


def test_end_to_end_blind_enhancement(gpu_device):
    """Three 4-s utterances (d = 0.08, N = 1024, SNR 20): engine.delay_mask -> MVDRPlan
    external / floor, sigma 1e-5. The projection SIR is at least 10 dB above the same plan fed
    an all-zero mask and within 1 dB of the restatement chain run with the kernel's delays."""
    import torch
    from avz import engine
    scenes = DC.long_scenes(20.0)
    S = 64000
    plan = _plan(1024, 0.08, max_samples=S)
    mix = torch.from_numpy(np.stack([s[0] for s in scenes])).to(gpu_device)
    M, _, delays, n = engine.delay_mask(plan, mix, return_debug=True)
    out, _ = plan.run(mix, ext_mask=M)
    zero, _ = plan.run(mix, ext_mask=torch.zeros_like(M))
    torch.cuda.synchronize()
    delays, n = delays.cpu().numpy(), n.cpu().numpy()
    kw = dict(n_fft=1024, hop=512, sigma=1e-5, d=0.08, floor=0.05)
    for i, (x, tgt, itf) in enumerate(scenes):
        sir = DC.sir_db(out[i].cpu().numpy(), tgt, itf)
        base = DC.sir_db(zero[i].cpu().numpy(), tgt, itf)
        Y = DC.spectra(x, 1024)
        Mr = DM.delay_labels(Y[0], Y[1], delays[i], int(n[i]), 1024)
        ref = DC.sir_db(O.external_mask_vec(x, Mr, **kw), tgt, itf)
        print(f"idx {i}: J {n[i]}, delays {delays[i][:1 + n[i]]}, SIR {sir:.2f} dB (restatement "
              f"chain {ref:.2f} dB, all-zero mask {base:.2f} dB)")
        assert sir >= base + 10.0
        assert abs(sir - ref) <= 1.0
    # enhance_blind is that path for one utterance
    y = DM.enhance_blind(scenes[0][0], n_fft=1024, mic_d=0.08, sigma=1e-5)
    assert DC.sir_db(y, scenes[0][1], scenes[0][2]) >= \
        DC.sir_db(zero[0].cpu().numpy(), scenes[0][1], scenes[0][2]) + 10.0
