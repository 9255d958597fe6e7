"""CPU checks of the streaming-WPE contract on its fp64 restatement alone
(avz.dereverb.wpe_stream_numpy, which the GPU tests compare the kernels with): the RLS
recursion against the closed-form regularised least-squares solution, that it dereverberates a
synthetic autoregressive mixture, the synthesis against scipy.signal.istft, a long run's Q,
the adapt flag and the grouping of hops; and the C ABI's host-side argument checks on a bare
configuration (avz_wpe_stream_check_*: the functions the public entry points call). The
kernels' checks are in test_gpu_wpe_stream.py."""
import ctypes as ct
import os
import subprocess

import numpy as np
import pytest
import scipy.signal

import wpe_stream_cases as WC
from avz import _lib
from avz import dereverb as DV
from conftest import ROOT, triple_f32


def test_forget_one_is_the_regularised_least_squares_solution():
    # matrix-inversion lemma: G_T = (I / q_init + sum lam y~ y~^H)^-1 sum lam y~ y^H
    F, T, K, D, q_init, floor = 5, 40, 3, 2, 2.0, 1e-3
    rng = np.random.default_rng(1)
    Y = (rng.standard_normal((2, F, T)) + 1j * rng.standard_normal((2, F, T))).astype(np.complex64)
    _, st = DV.wpe_stream_numpy(Y, n_fft=2 * (F - 1), taps=K, delay=D, forget=1.0,
                                power_floor=floor, q_init=q_init)
    Yd, W, worst = Y.astype(complex), K + D + 1, 0.0
    for k in range(F):
        Yt = DV.regressor(Yd[:, k], K, D)
        pw = np.abs(Yd[:, k]) ** 2
        p = np.array([pw[:, max(0, t - W + 1):t + 1].sum() / (2 * W) for t in range(T)])
        lam = 1.0 / np.maximum(p, floor)
        G = np.linalg.solve(np.eye(2 * K) / q_init + (Yt * lam) @ Yt.conj().T,
                            (Yt * lam) @ Yd[:, k].conj().T)
        worst = max(worst, np.abs(G - st.G[k]).max() / np.abs(G).max())
    print(f"max relative |G_rls - G_solve| = {worst:.3e}")
    assert worst <= 1e-10


@pytest.mark.parametrize("forget", [0.99, 1.0])
def test_it_dereverberates_an_autoregressive_mixture(forget):
    # Y_t = S_t + sum_tau A_tau Y_{t - D - tau}: the prediction error recovers S
    bins, T, K, D = 4, 600, 2, 1
    rng = np.random.default_rng(11)
    S = (rng.standard_normal((2, bins, T)) + 1j * rng.standard_normal((2, bins, T))) / np.sqrt(2)
    A = 0.15 * (rng.standard_normal((K, bins, 2, 2)) + 1j * rng.standard_normal((K, bins, 2, 2)))
    Y = np.zeros_like(S)
    for t in range(T):
        y = S[:, :, t].copy()
        for tau in range(K):
            if t - D - tau >= 0:
                y += np.einsum("kab,bk->ak", A[tau], Y[:, :, t - D - tau])
        Y[:, :, t] = y
    _, st = DV.wpe_stream_numpy(Y.astype(np.complex64), n_fft=2 * (bins - 1), taps=K, delay=D,
                                forget=forget, power_floor=1e-6)
    Z = np.stack(st.hist["Z"], axis=-1)
    ratio = (np.abs(Z - S)[:, :, 400:] ** 2).sum() / (np.abs(Y - S)[:, :, 400:] ** 2).sum()
    print(f"forget {forget}: residual reverberation / reverberation = {ratio:.3f}")
    assert ratio < 0.25


@pytest.mark.parametrize("n_fft", WC.SIZES)
def test_synthesis_is_istft_of_z_delayed_by_one_hop(n_fft):
    H, T = n_fft // 2, WC.CASES["k2"]["T"]
    out, st = WC.run_numpy(n_fft, "k2", 0)
    Z = np.stack(st.hist["Z"], axis=-1)                       # [2, F, T]
    _, x = scipy.signal.istft(Z, nperseg=n_fft, noverlap=H)   # [2, (T - 1) H]
    assert out.shape == (2, T * H) and x.shape == (2, (T - 1) * H)
    assert np.all(out[:, :H] == 0.0)
    err = np.abs(out[:, H:] - x).max()
    print(f"N={n_fft}: max|stream - istft| = {err:.3e}, max|out| = {np.abs(out).max():.3f}")
    assert np.abs(out).max() > 1e-2 and err <= 1e-12
    # and its frames are scipy's frames of the input, up to the fp32 window and the rounding
    # to complex64
    mix = WC.inputs(n_fft, T)[0][:, :(T - 1) * H].astype(np.float64)
    _, _, Ys = scipy.signal.stft(mix, nperseg=n_fft, noverlap=H)
    Y = np.stack(st.hist["Y"], axis=-1)
    assert Ys.shape == Y.shape and np.abs(Y - Ys).max() <= 2.0 ** -21 * np.abs(Ys).max()


def test_long_run_keeps_q_hermitian_and_positive():
    n_fft, frames = 512, 2000
    src = triple_f32("test")[0]
    x = np.tile(src, 4)[:, :frames * (n_fft // 2)]
    _, st = DV.wpe_stream_numpy(x, n_fft=n_fft, taps=10, delay=3, forget=0.99, drain=False)
    assert st.count == frames and np.isfinite(st.Q.view(np.float64)).all()
    assert np.array_equal(st.Q, st.Q.conj().transpose(0, 2, 1))
    lo = np.linalg.eigvalsh(st.Q).min()
    print(f"smallest eigenvalue of Q over all bins after {frames} frames: {lo:.3e}")
    assert lo > 0


@pytest.mark.parametrize("case", ["k2", "k10"])
def test_adapt_zero_freezes_the_filter_and_grouping_changes_no_bit(case):
    n_fft, T = 512, WC.CASES[case]["T"]
    adapt = np.ones(T, dtype=int)
    adapt[9:] = 0
    out, st = WC.run_numpy(n_fft, case, 0, adapt=adapt)
    mix = WC.inputs(n_fft, T)[0]
    _, head = DV.wpe_stream_numpy(mix[:, :9 * (n_fft // 2)], n_fft=n_fft, drain=False,
                                  **WC.params(case))
    assert np.array_equal(st.G, head.G) and np.array_equal(st.Q, head.Q)
    _, free = WC.run_numpy(n_fft, case, 0)
    Zf, Zz = np.stack(free.hist["Z"], -1), np.stack(st.hist["Z"], -1)
    assert np.array_equal(Zf[:, :, :9], Zz[:, :, :9])
    assert np.abs(Zz[:, :, 9:]).max() > 0 and not np.array_equal(Zf[:, :, 10:], Zz[:, :, 10:])
    assert np.abs(Zz[:, :, 12:] - np.stack(st.hist["Y"], -1)[:, :, 12:]).max() > 0
    for g in WC.groupings(case).values():
        o2, s2 = WC.run_numpy(n_fft, case, 0, adapt=adapt, hops_per_push=g)
        assert np.array_equal(o2, out) and np.array_equal(s2.G, st.G)
        assert np.array_equal(s2.Q, st.Q)


# ---------------------------------------------------------------------------- host-side checks
def _cfg(n_fft=512, max_batch=3):
    c = _lib.AvzConfig()
    c.fs, c.n_fft, c.hop, c.max_batch, c.max_samples = 16000, n_fft, n_fft // 2, max_batch, 1 << 16
    return c


def _args(c, streams=3, hops=4, taps=10, delay=3, **over):
    row = hops * c.hop
    nbytes = _lib.lib.avz_wpe_stream_check_state_bytes(ct.byref(c), streams, taps, delay)
    a = _lib.AvzWpeStreamArgs(streams=streams, hops=hops, taps=taps, delay=delay, forget=0.99,
                              power_floor=1e-9)
    a.mix, a.mix_stride, a.ch_stride = 0x10000, 2 * row, row
    a.out, a.out_stride, a.out_ch_stride = 0x20000, 2 * row, row
    a.state, a.state_bytes = 0x100000, nbytes
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_state_bytes_follow_the_documented_figures():
    for n_fft, K, D, per_bin in ((512, 10, 3, 4480), (1024, 10, 3, 4480), (1024, 16, 3, 10048)):
        c = _cfg(n_fft)
        F = n_fft // 2 + 1
        one = _lib.lib.avz_wpe_stream_check_state_bytes(ct.byref(c), 1, K, D)
        assert one % 256 == 0 and 0 <= one - (F * per_bin + 8 * n_fft + 256) < 6 * 256
        assert _lib.lib.avz_wpe_stream_check_state_bytes(ct.byref(c), 3, K, D) == 3 * one


def test_push_argument_checks_without_a_device():
    c = _cfg()
    chk = lambda a: _lib.lib.avz_wpe_stream_check_push(ct.byref(c), ct.byref(a))  # noqa: E731
    assert chk(_args(c)) == _lib.AVZ_OK
    row = 4 * c.hop
    ARG, SHAPE, ALIGN = _lib.AVZ_ERR_ARG, _lib.AVZ_ERR_SHAPE, _lib.AVZ_ERR_ALIGN
    for over, want in ((dict(taps=0), ARG), (dict(taps=17), ARG), (dict(delay=0), ARG),
                       (dict(delay=9), ARG), (dict(forget=0.0), ARG), (dict(forget=1.01), ARG),
                       (dict(forget=float("nan")), ARG), (dict(power_floor=0.0), ARG),
                       (dict(power_floor=-1.0), ARG), (dict(hops=0), ARG), (dict(mix=None), ARG),
                       (dict(out=None), ARG), (dict(state=None), ARG),
                       (dict(streams=0), SHAPE), (dict(streams=4), SHAPE),
                       (dict(ch_stride=row - 4), SHAPE), (dict(out_ch_stride=row - 4), SHAPE),
                       (dict(mix_stride=2 * row - 4), SHAPE), (dict(out_stride=2 * row - 4), SHAPE),
                       (dict(state_bytes=256), SHAPE),
                       (dict(state=0x100000 + 128), ALIGN), (dict(out=0x20000 + 8), ALIGN),
                       (dict(out_stride=2 * row + 2), ALIGN),
                       (dict(out_ch_stride=row + 2, out_stride=2 * row + 4), ALIGN)):
        a = _args(c, **over)
        if "state_bytes" not in over and ("taps" in over or "delay" in over):
            a.state_bytes = 1 << 30        # the range check answers, not the size
        assert chk(a) == want, (over, chk(a), want)
    # the state's size follows taps and delay
    assert chk(_args(c, taps=10, state_bytes=_args(c, taps=9).state_bytes)) == SHAPE
    rst = _lib.lib.avz_wpe_stream_check_reset
    nb = _args(c).state_bytes
    assert rst(ct.byref(c), 0x100000, nb, 3, 10, 3, 1.0) == _lib.AVZ_OK
    assert rst(ct.byref(c), 0x100000, nb, 3, 10, 3, 0.0) == ARG
    assert rst(ct.byref(c), 0x100000, nb, 3, 17, 3, 1.0) == ARG
    assert rst(ct.byref(c), 0x100000, nb - 256, 3, 10, 3, 1.0) == SHAPE
    assert rst(ct.byref(c), 0x100040, nb, 3, 10, 3, 1.0) == ALIGN


def test_exports_and_struct_layout(tmp_path):
    lib = _lib.lib
    for n in ("avz_wpe_stream_state_bytes", "avz_wpe_stream_reset", "avz_wpe_stream_push"):
        assert n in _lib.EXPORTED and hasattr(lib, n)
    hdr = os.path.join(ROOT, "include", "avz.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr}"', 'int main(void){',
             'printf("size %zu\\n", sizeof(avz_wpe_stream_args));']
    for f, _ in _lib.AvzWpeStreamArgs._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(avz_wpe_stream_args, {f}));')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                  check=True).stdout.splitlines())
    assert int(got["size"]) == ct.sizeof(_lib.AvzWpeStreamArgs)
    for f, _ in _lib.AvzWpeStreamArgs._fields_:
        assert int(got[f]) == getattr(_lib.AvzWpeStreamArgs, f).offset, f
