"""CPU: the inputs, layouts and fp64 references of tests/gain_cases.py hold what
test_gpu_gain_paths.py relies on (no GPU, no library)."""
import numpy as np
import pytest

import gain_cases as GC
from oracle import avz_oracle as O


@pytest.mark.parametrize("n", GC.SIZES)
def test_each_length_gives_its_frame_count(n):
    H = n // 2
    rows = GC.rows(n)
    assert sorted(set(T for T, _ in rows)) == sorted(GC.FRAMES)
    for T, L in rows:
        assert L >= n and GC.n_frames(L, n) == T == O.n_frames(L, n, H)
        assert O.stft(np.zeros(L, np.float32), nperseg=n, noverlap=H)[2].shape[-1] == T
    # both lengths of every T but the smallest: the last frame empty, and holding one sample
    assert len(rows) == 2 * len(GC.FRAMES) - 1
    # the step edges the frame counts are there for (gain_cases' docstring)
    for fb in (GC.FB_GAIN[n], GC.FB_PLAIN[n], GC.FB_ANALYSIS):
        assert {fb, fb + 1, 2 * fb - 1, 2 * fb, 2 * fb + 1} <= set(GC.FRAMES)
    for T in (GC.CHUNK - 1, GC.CHUNK, GC.CHUNK + 1, GC.CHUNK + 8, GC.CHUNK + 9, 2 * GC.CHUNK - 1,
              2 * GC.CHUNK, 2 * GC.CHUNK + 1, 3 * GC.CHUNK + 1):
        assert T in GC.FRAMES


@pytest.mark.parametrize("n", GC.SIZES)
def test_masks_hold_their_special_entries(n):
    f32 = np.float32(GC.PF_FLOOR)
    for b, (T, L) in enumerate(GC.rows(n)):
        M = GC.row_mask(n, b, T)
        assert M.dtype == np.float32 and M.shape == (n // 2 + 1, T)
        assert M.min() >= 0 and M.max() <= 1
        ones = np.zeros(M.shape[0], bool)
        ones[GC.ONE_BINS] = True
        zeros = np.zeros(M.shape[0], bool)
        zeros[GC.ZERO_BINS] = True
        assert np.all(M[zeros] == 0) and np.all(M[ones & ~zeros] == 1)
        vals = [M[k, int(round(fr * (T - 1)))] for k, fr, _ in GC.FLOOR_PLANTS]
        assert sum(v == f32 for v in vals) == 3 and sum(v < f32 for v in vals) == 2 \
            and sum(v > f32 for v in vals) == 2
        G = GC.row_gain(n, b, T)
        assert G.max() > 1 and G.min() == 0 and np.all(G[GC.GAIN_ZERO_BIN] == 0)
    S = GC.spectra(n, 9)
    assert np.all(S[:, 0].imag != 0) and np.all(S[:, -1].imag != 0)


def _read_back(buf, spec):
    import torch
    numel, offset, shape, strides = spec
    assert buf.shape == (numel,)
    return torch.as_strided(torch.from_numpy(buf), shape, strides, offset).numpy()


@pytest.mark.parametrize("n", GC.SIZES)
def test_mask_layouts_read_back_the_logical_array(n):
    F, Tp = n // 2 + 1, GC.t_pad(n)
    lens = [L for _, L in GC.rows(n)][:4] + [n - 1]
    logical = GC.padded_masks(n, lens)
    B = len(lens)
    assert np.isnan(logical[-1]).all() and Tp % 4 == 0 and Tp >= max(GC.FRAMES)
    for lid in GC.MASK_LAYOUTS:
        spec = GC.mask_layout(lid, B, F, Tp)
        src = logical[0] if lid == "H" else logical
        view = _read_back(GC.place(src, spec), spec)
        want = np.broadcast_to(logical[0], logical.shape) if lid == "H" else logical
        assert np.array_equal(view[:, :F, :Tp], want, equal_nan=True), lid
        # whatever the view holds beyond the logical array is NaN
        assert np.isnan(view[:, F:, :]).all() and np.isnan(view[:, :, Tp:]).all(), lid
        # the layouts are strided inside their buffer and the stated path is the kernels'
        numel, offset, shape, strides = spec
        last = offset + sum((s - 1) * st for s, st in zip(shape, strides))
        assert 0 <= last < numel, lid
        assert GC.mask_takes_vector_path(offset, strides) == (lid in GC.VECTOR_MASK_LAYOUTS), lid
        assert shape[1] >= F and shape[2] >= Tp
    # the scalar layouts fail the vector condition each for its own reason
    for lid, why in (("C", "offset"), ("D", "sf"), ("E", "sb"), ("F", "st")):
        _, offset, _, (sb, sf, st) = GC.mask_layout(lid, B, F, Tp)
        bad = dict(offset=offset % 4 != 0, sf=sf % 4 != 0, sb=sb % 4 != 0, st=st != 1)
        assert bad[why] and sum(bad.values()) == (2 if lid == "F" else 1), (lid, bad)


@pytest.mark.parametrize("n", GC.SIZES)
def test_spectrum_layouts_read_back_the_logical_array(n):
    F = n // 2 + 1
    for T in (3, 9, 16):
        S = GC.spectra(n, T)
        for lid in GC.SPEC_LAYOUTS:
            spec = GC.spec_layout(lid, GC.SPEC_BATCH, F, T)
            view = _read_back(GC.place(S, spec), spec)
            assert np.array_equal(view, S), lid
            numel, offset, shape, strides = spec
            assert offset + sum((s - 1) * st for s, st in zip(shape, strides)) < numel
            assert GC.spec_takes_vector_path(offset, strides) == (lid in GC.VECTOR_SPEC_LAYOUTS)
            assert strides[1] >= T and strides[0] >= F * strides[1]


@pytest.mark.parametrize("n", GC.SIZES)
def test_references_are_finite_conditioned_and_tier2_is_sharper(n):
    """Every Tier 1 row finite with a peak > 0 and well conditioned in every solved bin (both
    weight_eps); the Tier 2 tolerance (from the fp64 weights, floor gain) below the Tier 1 one."""
    worst_cond, worst_tol = 0.0, 0.0
    for b, (T, L) in enumerate(GC.rows(n)):
        M = GC.row_mask(n, b, T)
        for eps in GC.WEIGHT_EPS:
            for pf in ("floor", "mul", "none"):
                r = GC.tier1(n, b, L, pf, eps)
                assert r["out"].shape == ((T - 1) * (n // 2),)
                assert np.isfinite(r["out"]).all() and r["peak"] > 0
            # the covariance the solve inverts: the reference's R is already R / (sum m + 1e-6)
            cond = GC.cond_solved_bins(r["R"], r["f"])
            assert np.isfinite(cond).all() and cond.max() <= GC.COND_MAX, (b, eps, cond.max())
            worst_cond = max(worst_cond, float(cond.max()))
        r = GC.tier1(n, b, L, "floor", 0.0)
        x, e_pert, tol = GC.tier2(n, b, L, r["W"], GC.gain_of(M, "floor"))
        assert np.isfinite(x).all() and e_pert > 0
        # the fp64 transform against the oracle's complex64-rounded one: far inside Tier 1
        assert np.abs(x - r["out"]).max() <= 1e-6 * r["peak"]
        assert tol < GC.WAVE_TOL * r["peak"], (b, tol / r["peak"])
        worst_tol = max(worst_tol, tol / r["peak"])
    print(f"N={n}: largest cond_2 {worst_cond:.3g}, largest Tier 2 tolerance "
          f"{worst_tol:.3g} of max|ref|")


@pytest.mark.parametrize("n", GC.SIZES)
def test_gain_references_reduce_to_external_mask_vec(n):
    for b in (0, 5, len(GC.rows(n)) - 1):
        T, L = GC.rows(n)[b]
        x, M = GC.row_signal(n, b, L), GC.row_mask(n, b, T)
        for eps in GC.WEIGHT_EPS:
            kw = dict(n_fft=n, hop=n // 2, sigma=GC.SIGMA, d=GC.MIC_D, weight_eps=eps)
            floor = O.external_mask_vec(x, M, floor=GC.PF_FLOOR, **kw)
            none = O.external_mask_vec(x, M, floor=None, **kw)
            assert np.array_equal(GC.tier1(n, b, L, "floor", eps)["out"], floor)
            assert np.array_equal(GC.tier1(n, b, L, "none", eps)["out"], none)
            # mul is the floor chain with the gain array handed in: a gain that is already
            # max(M, floor) gives the floor reference, an all-ones gain gives none
            assert np.array_equal(GC.chain_reference(x, M, np.maximum(M, GC.PF_FLOOR), n, eps),
                                  floor)
            assert np.array_equal(GC.chain_reference(x, M, np.ones_like(M), n, eps), none)
            mul = GC.tier1(n, b, L, "mul", eps)["out"]
            assert np.abs(mul - floor).max() > 1e-3 * np.abs(floor).max()


def test_hybrid_single_chunk_reference():
    """Tier 2 with the oracle's hybrid weights equals oracle.hybrid_hard_null_bf + istft on one
    32000-sample chunk (Final_pipeline's null x M)."""
    n, L = 1024, 32000
    rng = np.random.default_rng(9900)
    m0 = 0.1 * rng.standard_normal(L)
    x = np.stack([m0, 0.7 * m0 + 0.05 * rng.standard_normal(L)]).astype(np.float32)
    f, _, Y = O.stft(x, nperseg=n, noverlap=n // 2)
    M = rng.random(Y.shape[1:], dtype=np.float32)
    W = O.hybrid_weights_loop(Y, M, f, d=GC.HYBRID["mic_d"])
    ref = O.istft(O.hybrid_hard_null_bf(Y, M, f, d=GC.HYBRID["mic_d"]) * M, nperseg=n,
                  noverlap=n // 2)[1]
    got = GC.synth_reference(Y.astype(np.complex128), W, M, n)
    assert ref.shape == got.shape == (32256,)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("n", GC.SIZES)
def test_istft_reference_and_many_rows(n):
    for T in (3, 17):
        ref = GC.istft_reference(n, T)
        assert ref.shape == (GC.SPEC_BATCH, (T - 1) * (n // 2)) and np.isfinite(ref).all()
        # the imaginary parts of DC and Nyquist do not matter
        S = GC.spectra(n, T).astype(np.complex128)
        S[:, 0] = S[:, 0].real
        S[:, -1] = S[:, -1].real
        assert np.array_equal(O.istft(S, nperseg=n, noverlap=n // 2)[1], ref)
    for R in (8, 256, 304):
        T, lens, sampled = GC.many_rows(R, n)
        assert len(lens) == 2 * R + 5 and R in sampled and 2 * R in sampled
        assert set(T[sampled]) == set(GC.MANY_FRAMES) and (lens >= n).all()
        assert all(GC.n_frames(int(L), n) == t for L, t in zip(lens, T))
    x, M = GC.many_inputs(8, n)
    T, lens, _ = GC.many_rows(8, n)
    for b in (0, 1, 20):
        assert np.all(x[b, :, lens[b]:] == 0) and np.isnan(M[b, :, T[b]:]).all()
        assert np.isfinite(M[b, :, :T[b]]).all() and x[b, :, :lens[b]].std() > 0.05
        assert M.nbytes * (2 * 304 + 5) // len(lens) < 100e6
