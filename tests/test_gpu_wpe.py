"""avz_wpe_spectral (csrc/avz_wpe.hip) against the fp64 statement of the algorithm.

Per bin the kernel's Z must sit within 2^-23 max|Y_k| + 4 E_ref,k of wpe_f64: the first
term is the complex64 rounding of the output, E_ref,k = max|wpe_f64 - wpe_ld| is the fp64
reference's own error on that bin (tests/wpe_cases.py; test_wpe_reference.py keeps every
case accurate and far from the singular threshold), and the factor 4 allows for the
kernel's own fp64 summation order and solve. Worst observed ratios: DESIGN.md section 9."""
import ctypes as ct

import numpy as np
import pytest
import scipy.signal
import torch

import wpe_cases as W
from conftest import triple_f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu_device):
    from avz import engine
    return engine


def run(eng, dev, Y, frames, c, **kw):
    Yd = torch.from_numpy(Y).to(dev)
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32, device=dev)
    st = torch.full(Y.shape[:1] + Y.shape[2:3], -1, dtype=torch.int32, device=dev)
    Z = eng.wpe_spectral(Yd, c.taps, c.delay, c.iterations, frames=fr, status=st, **kw)
    torch.cuda.synchronize()
    return Z.cpu().numpy(), st.cpu().numpy()


def check_against_reference(name, Z, st, Y, frames):
    r = W.case_reference(name)
    assert np.array_equal(st, r["status"]) and np.all(st == 0)
    err = np.abs(Z.astype(np.complex128) - r["X"]).max(axis=(1, 3))
    tol = 2.0 ** -23 * r["ymax"] + 4 * r["E_ref"]
    print(f"{name}: worst error / tolerance = {(err / tol).max():.3f} "
          f"(error {err.max():.3e}, max E_ref/max|Y| = {(r['E_ref'] / r['ymax']).max():.2e})")
    for b, n in enumerate(frames):      # frames beyond an item's length: copies of Y
        assert np.array_equal(Z[b][:, :, n:], Y[b][:, :, n:])
    assert np.all(err <= tol), (name, float((err / tol).max()))


@pytest.mark.parametrize("case", W.GPU_CASES, ids=lambda c: c.name)
def test_kernel_matches_the_fp64_algorithm(eng, gpu_device, case):
    Y, frames = W.case_input(case.name)
    ragged = any(n != Y.shape[3] for n in frames)
    Z, st = run(eng, gpu_device, Y, frames if ragged else None, case)
    check_against_reference(case.name, Z, st, Y, frames)


STRIDE_CASE = next(c for c in W.AR_CASES if c.name.startswith("ar-T65-K10-d3-i3"))


def test_strided_in_place_and_repeated_calls(eng, gpu_device):
    c = STRIDE_CASE
    Y, frames = W.case_input(c.name)
    B, _, F, T = Y.shape
    dev = gpu_device
    fr = torch.tensor(frames, dtype=torch.int32, device=dev)
    Zc, st = run(eng, dev, Y, frames, c)
    check_against_reference(c.name, Zc, st, Y, frames)
    # non-contiguous Y and Z: slices of larger arrays with different paddings
    big_y = torch.zeros((B + 1, 2, F + 3, T + 5), dtype=torch.complex64, device=dev)
    big_z = torch.full((B, 2, F + 1, T + 2), 7.0, dtype=torch.complex64, device=dev)
    ys, zs = big_y[1:, :, 2:F + 2, 3:T + 3], big_z[:, :, :F, 1:T + 1]
    ys.copy_(torch.from_numpy(Y))
    eng.wpe_spectral(ys, c.taps, c.delay, c.iterations, frames=fr, out=zs)
    assert np.array_equal(zs.cpu().numpy(), Zc)
    edge = big_z.clone()
    edge[:, :, :F, 1:T + 1] = 7.0
    assert bool((edge == 7.0).all())                 # nothing written outside the view
    # a second call on the same stream: identical bits
    z2 = torch.empty_like(zs.contiguous())
    eng.wpe_spectral(ys, c.taps, c.delay, c.iterations, frames=fr, out=z2)
    eng.wpe_spectral(ys, c.taps, c.delay, c.iterations, frames=fr, out=zs)
    assert np.array_equal(z2.cpu().numpy(), Zc) and np.array_equal(zs.cpu().numpy(), Zc)
    # in place, Z == Y
    out = eng.wpe_spectral(ys, c.taps, c.delay, c.iterations, frames=fr, out=ys)
    assert out.data_ptr() == ys.data_ptr()
    assert np.array_equal(ys.cpu().numpy(), Zc)


def test_degenerate_bins_pass_through_with_a_status(eng, gpu_device):
    c = STRIDE_CASE                                   # taps 10, delay 3
    Y = W.case_input(c.name)[0].copy()
    Y[0, :, 1] = 0                                    # a zero-power bin
    Y[1, 1, 2] = Y[1, 0, 2]                           # identical mics: singular R
    Y[0, 0, 3, 5] = np.nan                            # a non-finite pivot
    lim = c.delay + 2 * c.taps - 1                    # the longest item the count rule rejects
    frames = (Y.shape[3], 40, lim)
    Z, st = run(eng, gpu_device, Y, frames, c)
    assert list(st[0]) == [0, 1, 0, 2, 0]
    assert st[1, 2] == 2 and np.all(np.delete(st[1], 2) == 0)
    assert np.all(st[2] == 2)
    for b, k in ((0, 1), (0, 3), (1, 2), (2, 0), (2, 3), (2, 4)):
        assert np.array_equal(Z[b][:, k], Y[b][:, k], equal_nan=True), (b, k)
    assert not np.array_equal(Z[0][:, 0], Y[0][:, 0])
    assert np.array_equal(Z[1][:, :, 40:], Y[1][:, :, 40:])


def test_one_frame_and_empty_items_are_safe(eng, gpu_device):
    c = STRIDE_CASE
    rng = np.random.default_rng(11)
    Y = (rng.standard_normal((2, 2, 3, 1)) + 1j * rng.standard_normal((2, 2, 3, 1))).astype(np.complex64)
    Z, st = run(eng, gpu_device, Y, None, c)
    assert np.array_equal(Z, Y) and np.all(st == 2)
    Y = W.case_input(c.name)[0]
    Z, st = run(eng, gpu_device, Y, (0, 0, Y.shape[3]), c)
    assert np.array_equal(Z[:2], Y[:2]) and np.all(st[:2] == 2) and np.all(st[2] == 0)
    Z, st = run(eng, gpu_device, Y, (-5, 10 ** 6, Y.shape[3]), c)   # clamped to [0, T]
    assert np.array_equal(Z[0], Y[0]) and np.all(st[0] == 2) and np.all(st[1:] == 0)
    # the frame limit: 2048 frames run, 2049 are refused before any launch
    Yl = torch.zeros((1, 2, 1, 2049), dtype=torch.complex64, device=gpu_device)
    Yl[..., :2048] = torch.from_numpy(W.ar_item(3, 1, 2048, 1)[0])
    for taps in (11, 14, 16):                         # the largest LDS footprints
        st = torch.full((1, 1), -1, dtype=torch.int32, device=gpu_device)
        Zl = eng.wpe_spectral(Yl[..., :2048], taps, 1, 1, status=st)
        torch.cuda.synchronize()
        assert int(st[0, 0]) == 0 and bool(torch.isfinite(Zl.abs()).all())
    from avz import AvzError
    with pytest.raises(AvzError, match=r"\(-2\)"):
        eng.wpe_spectral(Yl, 10, 3, 3)


def test_argument_errors(eng, gpu_device):
    from avz import _lib
    Y = torch.zeros((1, 2, 4, 65), dtype=torch.complex64, device=gpu_device)
    Z = torch.empty_like(Y)

    def call(taps=10, delay=3, iterations=3, y=Y.data_ptr(), z=Z.data_ptr(), frames=65):
        a = _lib.AvzWpeArgs()
        a.batch, a.bins, a.frames = 1, 4, frames
        a.taps, a.delay, a.iterations = taps, delay, iterations
        a.Y, a.Z = y, z
        a.y_stride_b, a.y_stride_m, a.y_stride_f = Y.stride(0), Y.stride(1), Y.stride(2)
        a.z_stride_b, a.z_stride_m, a.z_stride_f = Z.stride(0), Z.stride(1), Z.stride(2)
        return _lib.lib.avz_wpe_spectral(ct.byref(a), None)

    assert call() == _lib.AVZ_OK
    assert _lib.lib.avz_wpe_spectral(None, None) == _lib.AVZ_ERR_ARG
    for kw in ({"taps": 17}, {"taps": 0}, {"delay": 0}, {"iterations": 0}, {"iterations": 11},
               {"y": None}, {"z": None}):
        assert call(**kw) == _lib.AVZ_ERR_ARG, kw
    assert call(y=Y.data_ptr() + 4) == _lib.AVZ_ERR_ALIGN
    assert call(z=Z.data_ptr() + 4) == _lib.AVZ_ERR_ALIGN
    assert call(frames=66) == _lib.AVZ_ERR_SHAPE      # rows shorter than the frame count
    assert call(frames=0) == _lib.AVZ_ERR_SHAPE
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eng.wpe_spectral(Y[:, :1])


# ----------------------------------------------------------------------------
# time domain
# ----------------------------------------------------------------------------
N_FFT, HOP = 512, 256
PERTURBATION = 2e-6        # the STFT stage bound of test_stft_stage, relative to max|Y|


def cpu_apply_wpe(y, noise=None):
    _, _, Y = scipy.signal.stft(y.astype(np.float64), 16000, nperseg=N_FFT, noverlap=HOP)
    if noise is not None:
        Y = Y + noise * (PERTURBATION * np.abs(Y).max())
    X = W.wpe_f64(Y, 10, 3, 3)
    _, x = scipy.signal.istft(X, 16000, nperseg=N_FFT, noverlap=HOP)
    out = np.zeros(y.shape)
    n = min(y.shape[1], x.shape[1])
    out[:, :n] = x[:, :n]
    return out, Y.shape


def test_apply_wpe_matches_the_cpu_composition(gpu_device):
    from avz import dereverb
    mix, _, _ = triple_f32("test", W.SEG)
    ref, shape = cpu_apply_wpe(mix)
    rng = np.random.default_rng(2024)
    e_pert = 0.0
    for _ in range(8):
        u = rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)
        u /= np.maximum(np.abs(u), 1.0)               # |noise| <= the stage bound
        e_pert = max(e_pert, np.abs(cpu_apply_wpe(mix, u)[0] - ref).max())
    got = dereverb.apply_wpe(mix)
    assert got.shape == mix.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"apply_wpe: error {err:.3e}, E_pert {e_pert:.3e}, bound {4 * e_pert + 1e-6:.3e}")
    assert err <= 4 * e_pert + 1e-6
    # the batched form with ragged lengths: each item as if alone, zero beyond its length
    x = torch.from_numpy(np.stack([mix, mix[:, ::-1].copy()])).to(gpu_device)
    lens = torch.tensor([mix.shape[1], 20000], dtype=torch.int32, device=gpu_device)
    out = dereverb.dereverb_batch(x, lens).cpu().numpy()
    assert np.abs(out[0] - got).max() <= 1e-6
    alone = dereverb.apply_wpe(mix[:, ::-1][:, :20000])
    assert np.abs(out[1][:, :20000] - alone).max() <= 1e-6 and np.all(out[1][:, 20000:] == 0)


def test_dereverb_main_feeds_oracle_reverb_main(gpu_device, tmp_path, capsys):
    from avz import dereverb, oracle_reverb, wavio
    mix, tgt, itf = triple_f32("test", W.SEG)         # int16 / 32768: written back exactly
    wavio.write(str(tmp_path / "mixture.wav"), mix.T, 16000)
    wavio.write(str(tmp_path / "target_reference.wav"), tgt, 16000)
    wavio.write(str(tmp_path / "interference_reference.wav"), itf, 16000)
    args = dereverb.parse_args(["--outdir", str(tmp_path)])
    assert (args.taps, args.delay, args.iters) == (10, 3, 3)
    y = dereverb.main(args)
    assert (tmp_path / "mixture_wpe.wav").exists()
    wpe_wav, fs = wavio.read(str(tmp_path / "mixture_wpe.wav"))
    assert fs == 16000 and wpe_wav.shape == mix.T.shape
    expect = dereverb.apply_wpe(mix)
    assert np.array_equal(y, expect)
    q = np.clip(np.round(expect.T.astype(np.float64) * 32768.0), -32768, 32767) / 32768.0
    assert np.array_equal(wpe_wav, q.astype(np.float32))
    out = oracle_reverb.main(oracle_reverb.parse_args(["--outdir", str(tmp_path)]))
    assert (tmp_path / "output_oracle_reverb.wav").exists()
    assert out is not None and np.all(np.isfinite(out)) and np.all(np.isfinite(wpe_wav))
    # a missing mixture: print and return, nothing written
    assert dereverb.main(dereverb.parse_args(["--outdir", str(tmp_path / "absent")])) is None
    assert "not found" in capsys.readouterr().out
