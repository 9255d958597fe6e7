"""CPU checks of the streaming beamformer's contract: avz.stream.stream_numpy (the fp64
restatement the GPU tests compare the kernel with) against the oracle's offline stages, its
independence of the grouping of hops into pushes, adapt flags and steering changes, and the
host-side argument checks of the C ABI, which run on a bare configuration without a device
(avz_stream_check_*: the very functions the public entry points call with the plan's
configuration). The kernel's checks are in test_gpu_stream.py."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest

import stream_cases as SC
from avz import _lib
from avz import stream as ST
from conftest import ROOT
from oracle import avz_oracle as O


@pytest.mark.parametrize("n_fft", SC.SIZES)
def test_synthesis_is_istft_of_the_causal_spectrum_delayed_by_one_hop(n_fft):
    H = n_fft // 2
    out, st = SC.run_numpy(n_fft, "floor", 0, forget=0.9)
    S = np.stack(st.hist["S"], axis=-1)                       # [F, T] causal spectrum
    _, x = O.istft(S, nperseg=n_fft, noverlap=H)              # (T - 1) H samples
    assert out.shape == (SC.T * H,) and x.shape == ((SC.T - 1) * H,)
    assert np.all(out[:H] == 0.0)
    err = np.abs(out[H:] - x).max()
    print(f"N={n_fft}: max|stream - istft| = {err:.3e}, max|out| = {np.abs(out).max():.3f}")
    assert np.abs(out).max() > 1e-2 and err <= 1e-12


@pytest.mark.parametrize("n_fft", SC.SIZES)
@pytest.mark.parametrize("name", ["floor", "none"])
def test_running_sums_at_forget_one_are_the_offline_sums(n_fft, name):
    cfg = SC.CONFIGS[name]
    weight_eps = 1e-10
    _, st = SC.run_numpy(n_fft, name, 0, forget=1.0, weight_eps=weight_eps)
    Y = np.stack(st.hist["Y"], axis=-1)                       # [2, F, T]
    noise = np.stack(st.hist["noise"], axis=-1)               # [F, T]
    # the restatement's frames are scipy's frames of the same signal (the oracle windows
    # float64 input with the float64 window: the fp32 window's rounding, 2^-24, remains)
    mix = SC.inputs(n_fft)[0][0][:, :SC.HOPS * (n_fft // 2)]
    _, _, Yo = O.stft(mix.astype(np.float64), nperseg=n_fft, noverlap=n_fft // 2)
    assert Yo.shape == Y.shape and np.abs(Y - Yo).max() <= 2.0 ** -22 * np.abs(Yo).max()
    eps32 = float(np.float32(weight_eps))
    R = O.covariance_vec(Y, noise, eps32)
    sums = R * (noise.sum(axis=1) + 1e-6)[:, None, None]
    c = st.c
    scale = np.abs(sums).max()
    assert np.abs(c[:, 0] - sums[:, 0, 0].real).max() <= 1e-12 * scale
    assert np.abs(c[:, 1] - sums[:, 1, 1].real).max() <= 1e-12 * scale
    assert np.abs(c[:, 2] + 1j * c[:, 3] - sums[:, 0, 1]).max() <= 1e-12 * scale
    assert np.abs(c[:, 4] - noise.sum(axis=1)).max() <= 1e-12 * noise.sum(axis=1).max()
    # the last weights are the oracle's solve of those sums (of the stream's own: at
    # sigma = 1e-7 the solve turns the sums' 1e-12 into 1e-9 by itself)
    Rc = np.empty_like(R)
    nrm = c[:, 4] + 1e-6
    Rc[:, 0, 0], Rc[:, 1, 1] = c[:, 0] / nrm, c[:, 1] / nrm
    Rc[:, 0, 1] = (c[:, 2] + 1j * c[:, 3]) / nrm
    Rc[:, 1, 0] = np.conj(Rc[:, 0, 1])
    W = O.mvdr_weights_vec(Rc, st.f_bins, cfg["sigma"], 90.0, cfg["mic_d"], O.C_SOUND, 100.0)
    err = np.abs(st.w - W).max() / np.abs(W).max()
    print(f"N={n_fft} {name}: weights relative error {err:.3e}")
    assert err <= 1e-9


@pytest.mark.parametrize("n_fft", SC.SIZES)
@pytest.mark.parametrize("name", ["floor", "ibm"])
def test_grouping_of_hops_into_pushes_changes_nothing(n_fft, name):
    res = {g: SC.run_numpy(n_fft, name, 1, forget=0.9, hops_per_push=sizes)
           for g, sizes in SC.GROUPINGS.items()}
    out0, st0 = res["one"]
    for g in ("single", "ragged"):
        out, st = res[g]
        assert np.array_equal(out, out0) and np.array_equal(st.c, st0.c)
        assert np.array_equal(st.w, st0.w) and st.count == SC.T
        assert np.array_equal(st.tail, st0.tail) and np.array_equal(st.prev, st0.prev)


def test_adapt_flags_freeze_and_steering_moves_from_the_next_frame():
    n_fft = 512
    adapt = np.ones(SC.T, dtype=int)
    adapt[6:11] = 0
    _, st = SC.run_numpy(n_fft, "floor", 0, forget=0.9, adapt=adapt)
    c, w = st.hist["c"], st.hist["w"]
    for t in range(6, 11):
        assert np.array_equal(c[t], c[5]) and np.array_equal(w[t], w[5])
    assert not np.array_equal(c[11], c[10]) and not np.array_equal(c[5], c[4])
    # a steering change before hop 9: frames 0 .. 8 as without it, frame 9 on with the new table
    _, base = SC.run_numpy(n_fft, "floor", 0, forget=0.9)
    _, turn = SC.run_numpy(n_fft, "floor", 0, forget=0.9, steer={9: 60.0})
    table = O.steering_vectors(base.f_bins, 60.0, 0.04, O.C_SOUND)
    _, turn2 = SC.run_numpy(n_fft, "floor", 0, forget=0.9, steer={9: table})
    for t in range(SC.T):
        same = np.array_equal(turn.hist["w"][t], base.hist["w"][t])
        assert same == (t < 9), t
        assert np.array_equal(turn.hist["c"][t], base.hist["c"][t])    # the sums do not move
        assert np.allclose(turn.hist["w"][t], turn2.hist["w"][t], rtol=1e-12, atol=1e-15)
    live = base.f_bins >= 100.0
    w9 = ST.mvdr_weights(turn.hist["c"][9], base.f_bins, table, 1e-5, 100.0)
    assert np.allclose(turn.hist["w"][9][live], w9[live], rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------ host-side ABI
def _cfg(**kw):
    c = _lib.AvzConfig(fs=16000, n_fft=1024, hop=512, sigma=1e-5, angle_deg=90.0, mic_d=0.04,
                       c_sound=343.0, fmin_hz=100.0, mask_mode=_lib.MASK_EXTERNAL,
                       postfilter=_lib.PF_EXT_FLOOR, pf_floor=0.05, weight_eps=0.0,
                       normalize=_lib.NORM_NONE, norm_eps=0.0, max_batch=4, max_samples=64000,
                       beamformer=_lib.BF_MVDR, bypass_hz=200.0, cond_max=10.0,
                       singular_fallback=_lib.FALLBACK_MIC0, ibm_kappa=0.0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _args(**kw):
    """Arguments that pass every check for _cfg(); pointers are never dereferenced."""
    p = 4096
    a = _lib.AvzStreamArgs(streams=2, hops=3, forget=1.0, mix=p, mix_stride=2 * 1536,
                           ch_stride=1536, ref_tgt=p, ref_int=p, ref_stride=1536, ext_mask=p,
                           mask_stride_b=513 * 3, mask_stride_f=3, mask_stride_t=1, out=p,
                           out_stride=1536, state=p, state_bytes=1 << 20)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_host_side_checks_reject_before_any_device_work():
    lib = _lib.lib
    E = _lib
    push = lambda c=None, **kw: lib.avz_stream_check_push(ct.byref(c or _cfg()), ct.byref(_args(**kw)))  # noqa
    assert push() == E.AVZ_OK
    nbytes = lib.avz_stream_check_state_bytes(ct.byref(_cfg()), 2)
    assert nbytes % 256 == 0 and 2 * 40000 < nbytes < 2 * 50000        # about 47 KB per stream
    assert lib.avz_stream_check_state_bytes(ct.byref(_cfg(n_fft=512, hop=256)), 1) < nbytes // 3
    assert push(state_bytes=nbytes) == E.AVZ_OK
    # the public entry points without a plan
    assert lib.avz_stream_push(None, ct.byref(_args()), None) == E.AVZ_ERR_ARG
    assert lib.avz_stream_state_bytes(None, 1) == E.AVZ_ERR_ARG
    assert lib.avz_stream_reset(None, 4096, 1 << 20, 1, None, None) == E.AVZ_ERR_ARG
    assert lib.avz_stream_steer(None, 4096, 1 << 20, 1, 4096, None) == E.AVZ_ERR_ARG
    assert lib.avz_stream_check_push(ct.byref(_cfg()), None) == E.AVZ_ERR_ARG
    # AVZ_ERR_ARG: NULL pointers, hops < 1, forget outside (0, 1]
    for name in ("mix", "out", "state", "ext_mask"):
        assert push(**{name: None}) == E.AVZ_ERR_ARG, name
    ibm = dict(mask_mode=E.MASK_IBM, postfilter=E.PF_IBM_TARGET)
    assert push(_cfg(**ibm), ext_mask=None) == E.AVZ_OK
    assert push(_cfg(**ibm), ref_tgt=None) == E.AVZ_ERR_ARG
    assert push(_cfg(**ibm), ref_int=None) == E.AVZ_ERR_ARG
    ones = dict(mask_mode=E.MASK_ONES, postfilter=E.PF_NONE)
    assert push(_cfg(**ones), ext_mask=None, ref_tgt=None, ref_int=None) == E.AVZ_OK
    assert push(hops=0) == E.AVZ_ERR_ARG and push(hops=-1) == E.AVZ_ERR_ARG
    for f in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert push(forget=f) == E.AVZ_ERR_ARG, f
    assert push(forget=1e-3) == E.AVZ_OK
    # AVZ_ERR_SHAPE: strides shorter than a row, streams beyond max_batch, short state
    assert push(streams=5) == E.AVZ_ERR_SHAPE and push(streams=0) == E.AVZ_ERR_SHAPE
    assert push(ch_stride=1535) == E.AVZ_ERR_SHAPE
    assert push(mix_stride=2 * 1536 - 1) == E.AVZ_ERR_SHAPE
    assert push(streams=1, mix_stride=0) == E.AVZ_OK
    assert push(out_stride=1532) == E.AVZ_ERR_SHAPE
    assert push(_cfg(**ibm), ref_stride=1535) == E.AVZ_ERR_SHAPE
    assert push(ref_stride=0) == E.AVZ_OK                               # unused by this plan
    assert push(state_bytes=nbytes - 1) == E.AVZ_ERR_SHAPE
    assert push(hops=1 << 22) == E.AVZ_ERR_SHAPE
    # AVZ_ERR_ALIGN
    assert push(out=4096 + 8) == E.AVZ_ERR_ALIGN
    assert push(out_stride=1538) == E.AVZ_ERR_ALIGN
    assert push(state=4096 + 128) == E.AVZ_ERR_ALIGN
    # reset / steer share the state checks
    st = lambda c=None, state=4096, nb=1 << 20, n=2, ptr=4096, need=1: (  # noqa: E731
        lib.avz_stream_check_state(ct.byref(c or _cfg()), state, nb, n, ptr, need))
    assert st() == E.AVZ_OK and st(ptr=None, need=0) == E.AVZ_OK
    assert st(ptr=None) == E.AVZ_ERR_ARG and st(state=None) == E.AVZ_ERR_ARG
    assert st(n=5) == E.AVZ_ERR_SHAPE and st(nb=nbytes - 1) == E.AVZ_ERR_SHAPE
    assert st(state=4096 + 64) == E.AVZ_ERR_ALIGN
    # AVZ_ERR_UNSUPPORTED plans: even with nothing else valid
    bad = [dict(beamformer=E.BF_HYBRID_NULL), dict(mask_mode=E.MASK_IPD, postfilter=E.PF_NONE),
           dict(mask_mode=E.MASK_IBM, postfilter=E.PF_IRM),
           dict(singular_fallback=E.FALLBACK_BATCH), dict(normalize=E.NORM_PEAK)]
    for kw in bad:
        c = _cfg(**kw)
        assert push(c) == E.AVZ_ERR_UNSUPPORTED, kw
        assert push(c, mix=None, hops=0, streams=99) == E.AVZ_ERR_UNSUPPORTED, kw
        assert lib.avz_stream_check_state_bytes(ct.byref(c), 1) == E.AVZ_ERR_UNSUPPORTED
        assert st(c, state=None) == E.AVZ_ERR_UNSUPPORTED
    assert push(_cfg(singular_fallback=E.FALLBACK_MEAN)) == E.AVZ_OK


def test_exports_version_and_struct_layout(tmp_path):
    lib = _lib.lib
    for n in ("avz_stream_state_bytes", "avz_stream_reset", "avz_stream_steer", "avz_stream_push"):
        assert n in _lib.EXPORTED and hasattr(lib, n)
    assert lib.avz_version() == _lib.ABI_VERSION == 3
    hdr = os.path.join(ROOT, "include", "avz.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(avz_stream_args));']
    for f, _ in _lib.AvzStreamArgs._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(avz_stream_args, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                  check=True).stdout.splitlines())
    assert int(got["size"]) == ct.sizeof(_lib.AvzStreamArgs)
    for f, _ in _lib.AvzStreamArgs._fields_:
        assert int(got[f]) == getattr(_lib.AvzStreamArgs, f).offset, f
