"""The WPE references against each other and against the algorithm's properties (no GPU).

wpe_f64 (avz.dereverb.wpe_numpy) is what the kernel is compared with in test_gpu_wpe.py;
wpe_ld (tests/wpe_cases.py, 80-bit) measures its error per bin. Every case the GPU test uses
must leave the fp64 reference accurate (E_ref,k <= 1e-4 max|Y_k|) and far from the singular
threshold (smallest relative Cholesky pivot >= 1000 x threshold), so that a kernel
difference is the kernel's."""
import numpy as np
import pytest

import wpe_cases as W
from avz.dereverb import pivot_threshold, regressor, wpe_bin

pytestmark = pytest.mark.skipif(not W.HAVE_LD, reason="long double is no wider than double")


@pytest.mark.parametrize("case", W.GPU_CASES, ids=lambda c: c.name)
def test_fp64_reference_is_accurate_and_regular_on_every_gpu_case(case):
    r = W.case_reference(case.name)
    assert np.all(r["status"] == 0)
    ratio = r["E_ref"] / r["ymax"]
    margin = r["rel"] / pivot_threshold(case.taps)
    print(f"{case.name}: max E_ref/max|Y| = {ratio.max():.3e}, min pivot/threshold = {margin.min():.3e}")
    assert np.all(r["E_ref"] <= 1e-4 * r["ymax"])
    assert np.all(margin >= 1000.0)


def _bins(case):
    Y, frames = W.case_input(case.name)
    r = W.case_reference(case.name)
    for b in range(Y.shape[0]):
        for k in range(Y.shape[2]):
            yield Y[b][:, k, :frames[b]], r["X"][b][:, k, :frames[b]], r["E_ref"][b, k]


# Row order: E_ref,k is ONE draw of the fp64 evaluation's rounding error and a permuted
# evaluation is another, so their distance is bounded by 4 E_ref,k only where that error is
# not widely spread: the cases with at least three regressor frames per unknown
# (T - delay >= 3 * 2 taps, every item). Below that (speech-1024: 45 frames for 20 unknowns)
# single bins differ by more (measured: 3 of 65 bins at 4.3 .. 5.3 E_ref, all with
# E_ref < 1e-8 max|Y|, far inside the complex64 term of the GPU tolerance).
def _frames_per_unknown(c):
    frames = c.frames or (W.case_input(c.name)[1])
    return (min(frames) - c.delay) / (2 * c.taps)


ORDER_CASES = [c for c in W.GPU_CASES
               if c.taps >= 2 and c.iterations == 3 and _frames_per_unknown(c) >= 3]


@pytest.mark.parametrize("case", ORDER_CASES, ids=lambda c: c.name)
def test_row_order_of_the_regressor_does_not_matter(case):
    n = 2 * case.taps
    rng = np.random.default_rng(7)
    for perm in (np.arange(n)[::-1], rng.permutation(n)):
        for Y, X, E in _bins(case):
            Xp, st, _ = wpe_bin(Y, case.taps, case.delay, case.iterations, row_order=perm)
            assert st == 0
            assert np.abs(Xp - X).max() <= 4 * E


@pytest.mark.parametrize("e", [-20, 20])
def test_common_power_of_two_scale_passes_through_exactly(e):
    for case in (W.GPU_CASES[9], W.SPEECH_CASES[0]):
        Y, frames = W.case_input(case.name)
        X = W.case_reference(case.name)["X"][0]
        Xs = W.wpe_f64(Y[0] * np.float32(2.0 ** e), case.taps, case.delay, case.iterations,
                       frames=frames[0])
        assert np.array_equal(Xs, X * 2.0 ** e)


@pytest.mark.parametrize("seed,T,taps,delay", W.DENOISE_CASES)
def test_ar_family_is_dereverberated(seed, T, taps, delay):
    Y, S = W.ar_item(seed, 7, T, delay)
    X, status, _ = W.wpe_f64(Y, taps, delay, 3, return_info=True)
    assert np.all(status == 0)
    for k in range(Y.shape[1]):
        assert np.linalg.norm(X[:, k] - S[:, k]) < np.linalg.norm(Y[:, k] - S[:, k]), k


def test_regressor_layout():
    Y = (np.arange(12).reshape(2, 6) + 1).astype(np.complex128)
    Yt = regressor(Y, taps=2, delay=2)
    assert Yt.shape == (4, 6)
    for tau in range(2):
        for m in range(2):
            for t in range(6):
                s = t - 2 - tau
                assert Yt[tau * 2 + m, t] == (Y[m, s] if s >= 0 else 0)


def test_degenerate_bins_pass_the_input_through():
    Y, _ = W.ar_item(5, 4, 40, 3)
    Y[:, 1] = 0                                   # zero power
    Y[1, 2] = Y[0, 2]                             # two identical mics: singular R
    X, status, _ = W.wpe_f64(Y, 4, 3, 3, return_info=True)
    assert list(status) == [0, 1, 2, 0]
    for k in (1, 2):
        assert np.array_equal(X[:, k], Y[:, k].astype(np.complex128))
    assert not np.array_equal(X[:, 0], Y[:, 0])
    Xl, st = W.wpe_ld(Y, 4, 3, 3)
    assert list(st) == [0, 1, 2, 0]
    # the count rule: T - delay < 2 taps, by the count alone (a zero bin included)
    for T, expect in ((10, 2), (24, 0)):
        X, status, _ = W.wpe_f64(Y[:, :, :T], 4, 3, 3, return_info=True)
        assert status[1] == (2 if expect == 2 else 1)
        assert status[0] == expect and status[3] == expect
        if expect == 2:
            assert np.array_equal(X, Y[:, :, :T].astype(np.complex128))
    # frames: the tail is a copy and enters no sum
    X, status, _ = W.wpe_f64(Y, 4, 3, 3, frames=30, return_info=True)
    assert np.array_equal(X[:, :, 30:], Y[:, :, 30:].astype(np.complex128))
    assert np.array_equal(X[:, 0, :30], W.wpe_f64(Y[:, :, :30], 4, 3, 3)[:, 0])
    # a non-finite bin is a non-finite pivot
    Y[0, 3, 7] = np.nan
    assert W.wpe_f64(Y, 4, 3, 3, return_info=True)[1][3] == 2
