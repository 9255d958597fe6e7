"""Blind delay-histogram mask without a GPU: the C ABI's surface (struct layout, exports, the
whole host-side error table through avz_delay_mask_check) and the properties of the fp64
restatement avz.delay_mask that the GPU tests compare the kernels with."""
import ctypes as ct
import os
import subprocess

import numpy as np

from conftest import ROOT

import delay_mask_cases as DC
from avz import _lib
from avz import delay_mask as DM
from oracle import avz_oracle as O


def _cfg(**kw):
    c = _lib.AvzConfig(fs=16000, n_fft=1024, hop=512, sigma=1e-5, angle_deg=90.0, mic_d=0.08,
                       c_sound=343.0, fmin_hz=100.0, mask_mode=_lib.MASK_EXTERNAL,
                       postfilter=_lib.PF_EXT_FLOOR, pf_floor=0.05, weight_eps=0.0,
                       normalize=_lib.NORM_NONE, norm_eps=0.0, max_batch=4, max_samples=64000)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


T64, F1024 = 126, 513  # frames of 64000 samples, bins, at n_fft 1024


def _args(**kw):
    p = 4096  # any non-null, 256-byte aligned address: the checks never dereference
    a = _lib.AvzDelayMaskArgs(batch=2, len=p, max_len=64000, mix=p, mix_stride=2 * 64000,
                              ch_stride=64000, hist_bins=65, smooth=3, max_peaks=3,
                              rel_height=0.25, min_sep=0.2, f_lo_hz=100.0, mask=p,
                              mask_stride_b=F1024 * T64, mask_stride_f=T64, mask_stride_t=1,
                              workspace=p, workspace_bytes=1 << 24)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_exports_version_and_struct_layout(tmp_path):
    lib = _lib.lib
    for n in ("avz_delay_mask_workspace_bytes", "avz_delay_mask", "avz_delay_mask_check"):
        assert n in _lib.EXPORTED and hasattr(lib, n)
    assert lib.avz_version() == _lib.ABI_VERSION == 3
    hdr = os.path.join(ROOT, "include", "avz.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(avz_delay_mask_args));']
    for f, _ in _lib.AvzDelayMaskArgs._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(avz_delay_mask_args, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                  check=True).stdout.splitlines())
    assert int(got["size"]) == ct.sizeof(_lib.AvzDelayMaskArgs)
    for f, _ in _lib.AvzDelayMaskArgs._fields_:
        assert int(got[f]) == getattr(_lib.AvzDelayMaskArgs, f).offset, f


def test_host_side_checks_reject_before_any_device_work():
    lib, E = _lib.lib, _lib
    chk = lambda c=None, **kw: lib.avz_delay_mask_check(ct.byref(c or _cfg()), ct.byref(_args(**kw)))  # noqa
    assert chk() == E.AVZ_OK
    # the public entry points without a plan; NULL configuration or arguments
    assert lib.avz_delay_mask(None, ct.byref(_args()), None) == E.AVZ_ERR_ARG
    assert lib.avz_delay_mask_workspace_bytes(None, 1, 64000, 65) == E.AVZ_ERR_ARG
    assert lib.avz_delay_mask_check(None, ct.byref(_args())) == E.AVZ_ERR_ARG
    assert lib.avz_delay_mask_check(ct.byref(_cfg()), None) == E.AVZ_ERR_ARG
    # AVZ_ERR_ARG: NULL pointers (the optional ones may be NULL), parameters outside their range
    for name in ("len", "mix", "mask", "workspace"):
        assert chk(**{name: None}) == E.AVZ_ERR_ARG, name
    assert chk(angle_deg=None, hist_out=None, delays_out=None, n_peaks=None) == E.AVZ_OK
    assert chk(angle_deg=4096, hist_out=4096, delays_out=4096, n_peaks=4096) == E.AVZ_OK
    for nb in (7, 8, 64, 66, 259, 0, -65):
        assert chk(hist_bins=nb) == E.AVZ_ERR_ARG, nb
    for nb in (9, 65, 257):
        assert chk(hist_bins=nb) == E.AVZ_OK, nb
    for s in (-1, 9):
        assert chk(smooth=s) == E.AVZ_ERR_ARG, s
    for s in (0, 8):
        assert chk(smooth=s) == E.AVZ_OK, s
    for m in (-1, 8):
        assert chk(max_peaks=m) == E.AVZ_ERR_ARG, m
    for m in (0, 7):
        assert chk(max_peaks=m) == E.AVZ_OK, m
    for r in (0.0, -0.25, 1.0000001, float("nan"), float("inf")):
        assert chk(rel_height=r) == E.AVZ_ERR_ARG, r
    assert chk(rel_height=1.0) == E.AVZ_OK
    for name in ("min_sep", "f_lo_hz"):
        for v in (-1e-9, float("nan")):
            assert chk(**{name: v}) == E.AVZ_ERR_ARG, (name, v)
        assert chk(**{name: 0.0}) == E.AVZ_OK, name
    # AVZ_ERR_SHAPE: batch, max_len, strides shorter than a row, workspace too small
    for b in (0, -1, 5):
        assert chk(batch=b) == E.AVZ_ERR_SHAPE, b
    assert chk(batch=4, mask_stride_b=F1024 * T64) == E.AVZ_OK
    for L in (1023, 64001, 0):
        assert chk(max_len=L) == E.AVZ_ERR_SHAPE, L
    assert chk(max_len=1024) == E.AVZ_OK
    assert chk(ch_stride=63999) == E.AVZ_ERR_SHAPE
    assert chk(mix_stride=2 * 64000 - 1) == E.AVZ_ERR_SHAPE
    assert chk(batch=1, mix_stride=0, mask_stride_b=0) == E.AVZ_OK   # one row: no row stride
    assert chk(mask_stride_f=T64 - 1) == E.AVZ_ERR_SHAPE              # bins overlap
    assert chk(mask_stride_b=F1024 * T64 - 1) == E.AVZ_ERR_SHAPE      # rows overlap
    assert chk(mask_stride_t=0) == E.AVZ_ERR_SHAPE
    assert chk(mask_stride_f=0) == E.AVZ_ERR_SHAPE
    assert chk(mask_stride_f=1, mask_stride_t=F1024) == E.AVZ_OK      # [B, T, F]
    assert chk(mask_stride_f=1, mask_stride_t=F1024 - 1) == E.AVZ_ERR_SHAPE
    assert chk(mask_stride_f=1, mask_stride_t=F1024, mask_stride_b=F1024 * T64 - 1) \
        == E.AVZ_ERR_SHAPE
    assert chk(mask_stride_f=2 * T64, mask_stride_t=2, mask_stride_b=2 * F1024 * T64) == E.AVZ_OK
    # the workspace: per-block partials [2][8 blocks of 16 frames][65] f64, the lists [2][8]
    # f64 and the counts [2] i32, each rounded up to 256 bytes (engine.delay_mask asks the
    # library through avz_delay_mask_workspace_bytes, which needs a plan and so a device)
    need = 8448 + 256 + 256
    assert chk(workspace_bytes=need) == E.AVZ_OK
    assert chk(workspace_bytes=need - 1) == E.AVZ_ERR_SHAPE
    assert chk(workspace_bytes=3 * need, hist_bins=257) == E.AVZ_ERR_SHAPE  # 33536 B
    assert chk(workspace_bytes=0) == E.AVZ_ERR_SHAPE
    # AVZ_ERR_ALIGN: the workspace's 256 bytes
    for off in (1, 8, 128):
        assert chk(workspace=4096 + off) == E.AVZ_ERR_ALIGN, off
    # the plan's mask mode, beamformer and post-filter are ignored
    assert chk(_cfg(mask_mode=E.MASK_IBM, postfilter=E.PF_IBM_TARGET)) == E.AVZ_OK
    assert chk(_cfg(beamformer=E.BF_HYBRID_NULL, mask_mode=E.MASK_IPD,
                    postfilter=E.PF_NONE)) == E.AVZ_OK
    small = _cfg(n_fft=512, hop=256)
    assert chk(small, max_len=512, mask_stride_f=3, mask_stride_b=257 * 3) == E.AVZ_OK


def test_grid_and_band():
    g = DM.delay_grid(1024, mic_d=0.08)
    assert abs(g.dmax - 0.08 * 16000 / 343.0) < 1e-12 and g.R == 1.25 * g.dmax
    assert (g.k_lo, g.k_hi) == (7, 109)       # 100 Hz; the largest k with omega_k R < pi
    assert 2 * np.pi * g.k_hi / 1024 * g.R < np.pi <= 2 * np.pi * (g.k_hi + 1) / 1024 * g.R
    assert DM.delay_grid(512, mic_d=0.01).k_hi == 256 and DM.delay_grid(512, mic_d=0.01).k_lo == 4
    assert abs(g.centre(32)) < 1e-12 and abs(g.centre(0) + g.R - 0.5 * g.bin_w) < 1e-12
    empty = DM.delay_grid(1024, mic_d=0.08, f_lo=4000.0)
    assert empty.k_hi < empty.k_lo
    Y = DC.reference(1024, 0.08, 0)["Y"]
    assert not DM.delay_histogram(Y[0], Y[1], empty).any()


def test_silence_dc_and_ties_are_target():
    Z = np.zeros((2, 513, 18), np.complex64)
    M, h, delays, J = DM.delay_mask_numpy(Z[0], Z[1], 1024, mic_d=0.08)
    assert J == 0 and not h.any() and (M == 1.0).all() and np.isnan(delays[1:]).all()
    assert delays[0] == 0.08 * 16000 / 343.0 * np.cos(np.deg2rad(90.0))
    for N, d in DC.CASES:
        for i in range(DC.UTTS):
            r = DC.reference(N, d, i)
            assert (r["mask"][0] == 1.0).all()                    # k = 0 is always 1
            assert 1 <= r["J"] <= 3 and 0.36 <= r["mask"].mean() <= 0.63, (N, d, i, r["J"])
    # NaN spectra: nothing is deposited, no peak, every decision 1
    Yn = np.full((2, 513, 18), np.nan + 0j, np.complex64)
    M, h, _, J = DM.delay_mask_numpy(Yn[0], Yn[1], 1024, mic_d=0.08)
    assert J == 0 and not h.any() and (M == 1.0).all()
    # max_peaks = 0 keeps none
    r = DC.reference(1024, 0.08, 1)
    assert DM.delay_peaks(r["h"], r["grid"], max_peaks=0)[1] == 0


def test_power_of_two_scaling_changes_no_peak_and_no_label():
    for N, d in DC.CASES:
        for i in range(DC.UTTS):
            r = DC.reference(N, d, i)
            for e in (10, -10):
                Y = (r["Y"] * np.float32(2.0 ** e)).astype(np.complex64)
                M, h, delays, J = DM.delay_mask_numpy(Y[0], Y[1], N, mic_d=d)
                assert J == r["J"] and np.array_equal(delays[:1 + J], r["delays"][:1 + J])
                assert np.array_equal(M, r["mask"])
                assert np.array_equal(h, r["h"] * 4.0 ** e)


def test_steering_to_the_interferer_finds_the_target_as_a_peak():
    """On the 4-s scenes at SNR 50, the scenes of the peak-position test below: the property is
    about the steering, so it is checked where the delay cue is clean and both sources are
    active. It is not a property of every scene: at SNR 20 the target's peak of scene 1 merges
    with mixed-source deposits into one plateau (local maxima at 0.86 and 1.15 samples, none
    near 0), and the 17-frame utterances of the shared cases last 0.27 to 0.54 s, one or two of
    the generator's 0.25-s envelope blocks, in which a source may be all but silent. That is
    why the target anchor is the geometric delay and never a found peak."""
    dmax = 0.08 * 16000 / 343.0
    for i, (mix, _, _) in enumerate(DC.long_scenes(50.0)):
        Y = DC.spectra(mix, 1024)
        _, _, delays, J = DM.delay_mask_numpy(Y[0], Y[1], 1024, mic_d=0.08, angle=40.0)
        assert abs(delays[0] / dmax - 0.766) < 1e-3
        kept = delays[1:1 + J]
        print(f"idx {i}: delta_t {delays[0]:.3f}, kept {kept}")
        assert (np.abs(kept) < 0.5).any(), (i, kept)                # the 90-degree source
        assert (np.abs(kept - delays[0]) > 0.2 * dmax).all()


def test_peak_sits_at_the_interferer_delay_at_high_snr():
    true = 0.08 * 16000 / 343.0 * np.cos(np.deg2rad(40.0))
    assert abs(true - 2.86) < 0.005
    for i, (mix, _, _) in enumerate(DC.long_scenes(50.0)):
        Y = DC.spectra(mix, 1024)
        _, _, delays, J = DM.delay_mask_numpy(Y[0], Y[1], 1024, mic_d=0.08)
        near = np.abs(delays[1:1 + J] - true).min()
        print(f"idx {i}: kept {delays[1:1 + J]}, nearest to {true:.3f}: {near:.3f}")
        assert near <= 0.2


def test_mask_gains_at_least_10_db_of_sir_over_the_all_noise_mask():
    kw = dict(n_fft=1024, hop=512, sigma=1e-5, d=0.08, floor=0.05)
    for i, (mix, tgt, itf) in enumerate(DC.long_scenes(20.0)):
        Y = DC.spectra(mix, 1024)
        M = DM.delay_mask_numpy(Y[0], Y[1], 1024, mic_d=0.08)[0]
        sir = DC.sir_db(O.external_mask_vec(mix, M, **kw), tgt, itf)
        base = DC.sir_db(O.external_mask_vec(mix, np.zeros_like(M), **kw), tgt, itf)
        print(f"idx {i}: SIR {sir:.1f} dB with the mask, {base:.1f} dB with the all-noise mask")
        assert sir >= base + 10.0
