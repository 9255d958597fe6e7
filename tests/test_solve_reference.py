"""The references and the case table of tests/solve_cases.py, proved on the CPU before any
kernel is compared with them (no GPU): LAPACK against the long-double closed form per family
(E_ref), the cond_2 branch on the constructed threshold bins, the singular families raising
where they must, and an mpmath spot check of the long-double values."""
import numpy as np

import solve_cases as C


def all_cases():
    return [cs for g in C.mvdr_groups() + C.hybrid_groups() for cs in g.cases]


def test_case_table_is_complete():
    groups = C.mvdr_groups() + C.hybrid_groups()
    assert len(C.mvdr_groups()) == 2 * len(C.N_FFTS) * len(C.SIGMAS)
    assert len(C.hybrid_groups()) == 4 * len(C.N_FFTS)
    for g in groups:
        for fam in {cs.family for cs in g.cases}:
            assert sum(cs.family == fam for cs in g.cases) == C.CASE_COUNTS[fam]
        for cs in g.cases:
            assert cs.cov.shape == (g.n_fft // 2 + 1, 5) and cs.cov.dtype == np.float64
    assert {cs.family for cs in all_cases()} == set(C.CASE_COUNTS) - {"S1", "S2", "S3"}
    for n_fft in C.N_FFTS:
        assert np.array_equal(C.bin_freqs(n_fft), np.fft.rfftfreq(n_fft, 1.0 / C.FS))


def test_reference_error_per_family():
    """E_ref < 1e-8 in every family (worst: M2, coherence 1 at sigma 1e-7, ~1e-9; hybrid
    below 1e-13)."""
    E = C.reference_error()
    print({k: f"{v:.2e}" for k, v in sorted(E.items())})
    assert set(E) == set(C.CASE_COUNTS) - {"S1", "S2", "S3"}
    for fam, e in E.items():
        assert e < 1e-8, (fam, e)
    for fam in ("H1", "H2", "H3", "H4", "H6"):
        assert E[fam] < 1e-12, (fam, E[fam])


def test_mvdr_families_are_regular_and_hit_their_edges():
    for g in C.mvdr_groups():
        f = C.bin_freqs(g.n_fft)
        for cs in g.cases:
            assert not cs.raised.any(), (g.tag, cs.family)
            assert np.isfinite(cs.lapack).all()
            if cs.family == "M3":
                c = cs.cov           # one frame: c0 c1 == |b|^2 up to the rounding of the products
                assert (np.abs(c[:, 0] * c[:, 1] - (c[:, 2] ** 2 + c[:, 3] ** 2))
                        <= 16 * np.finfo(float).eps * c[:, 0] * c[:, 1]).all()
            if cs.family == "M4":
                assert (cs.cov[:, 4] == 0).all() and (cs.cov[:, 0] > 0).all()
            if cs.family == "M5":
                assert (cs.cov[:, 4] % 1 != 0).all()
            if cs.family == "M7":
                k = g.n_fft // 128   # 125 Hz: bin 8 at N = 1024, bin 4 at N = 512
                assert f[k] == C.FMIN_M7 and f[k - 1] < C.FMIN_M7
                assert (cs.lapack[:k] == 0).all() and (cs.lapack[k] != 0).any()


def test_singular_families_raise_in_lapack():
    """S1 / S2 raise LinAlgError in every bin at or above fmin_hz, S3 in none."""
    for n_fft in C.N_FFTS:
        live = ~(C.bin_freqs(n_fft) < C.SINGULAR_FMIN)
        for fb, wfb in (("mic0", [1.0, 0.0]), ("mean", [0.5, 0.5])):
            W, raised, flags = C.singular_expected(n_fft, fb)
            assert np.array_equal(raised[0], live) and np.array_equal(raised[1], live)
            assert not raised[2].any() and flags == [1, 1, 0]
            for b in (0, 1):
                assert (W[b][live] == wfb).all() and (W[b][~live] == 0).all()
            assert np.isfinite(W[2]).all() and (W[2][~live] == 0).all()
        W, raised, flags = C.singular_expected(n_fft, "batch")
        d0 = C.steer_mvdr(n_fft)[:, 0]
        for b in (0, 1):
            assert np.array_equal(W[b][:, 0], 1.0 / (d0.conj() + 1e-10)) and (W[b][:, 1] == 0).all()
        assert np.array_equal(W[2], C.singular_expected(n_fft, "mic0")[0][2])


def test_h1_covers_both_eigenvector_forms_and_both_cond_branches():
    for g in C.hybrid_groups():
        h1 = [cs for cs in g.cases if cs.family == "H1"]
        if not h1:
            continue
        a = np.concatenate([cs.cov[cs.live, 0] for cs in h1])
        e = np.concatenate([cs.cov[cs.live, 1] for cs in h1])
        cond = np.concatenate([cs.cond[cs.live] for cs in h1])
        truth = np.concatenate([cs.cond_truth[cs.live] for cs in h1]).astype(np.float64)
        assert (a >= e).sum() > 100 and (a < e).sum() > 100
        assert (cond > C.COND_MAX).sum() >= 8 and (cond <= C.COND_MAX).sum() > 100
        # LAPACK's cond_2 and the closed form's agree to 1e-12 relative
        assert np.abs(cond / truth - 1).max() <= 1e-12
        # cond_2 > 1 everywhere: the engine's smallest cond_max (1) forces what -1 forces
        assert cond.min() > 1.0 + 1e-6
        assert not any(cs.raised.any() for cs in h1)
        cm = h1[0].cond_max
        for cs in h1:
            solved = cs.live & (cs.cond <= cm)
            if cm == 1e300:
                assert np.array_equal(solved, cs.live)
            if cm < 1:
                assert not solved.any()
                assert np.array_equal(cs.lapack[cs.live], cs.steer[cs.live] / 2)


def test_h4_branch_agrees_on_every_constructed_bin():
    """LAPACK's cond and the long-double cond take the same branch in every threshold bin,
    no exclusions, and the bins sit within 1e-9 (relative) of cond_max on the stated side."""
    n = 0
    for g in C.hybrid_groups():
        for cs in g.cases:
            if cs.family != "H4":
                continue
            k = cs.live
            below = "below" in cs.label
            truth = cs.cond_truth[k]
            assert np.array_equal(cs.cond[k] > cs.cond_max, truth > cs.cond_max)
            assert ((cs.cond[k] <= cs.cond_max) == below).all()
            rel = (truth / C.LD(cs.cond_max) - 1).astype(np.float64)
            assert np.abs(np.abs(rel) - C.H4_MARGIN).max() <= 1e-2 * C.H4_MARGIN
            assert ((rel < 0) == below).all()
            assert not cs.raised.any()
            n += int(k.sum())
    assert n == 2 * (250 + 500)


def test_special_hybrid_families():
    for g in C.hybrid_groups():
        f = C.bin_freqs(g.n_fft)
        for cs in g.cases:
            c, k = cs.cov, cs.live
            if cs.family == "H2":
                if cs.label == "a == e":
                    assert (c[:, 0] == c[:, 1]).all()
                else:
                    to = np.inf if "+" in cs.label else 0.0
                    assert np.array_equal(c[:, 0], np.nextafter(c[:, 1], to))
                assert (np.hypot(c[:, 2], c[:, 3]) > 0).all() and not cs.raised.any()
            if cs.family == "H3":
                assert (c[:, 2] == 0).all() and (c[:, 3] == 0).all() and (c[:, 0] > c[:, 1]).all()
                assert not cs.raised.any() and (cs.cond[k] <= cs.cond_max).all()
            if cs.family == "H5":
                # a contract, not a comparison: the reference raises in every live bin (the
                # eigenvector has v[0] == 0) and the engine documents delay-and-sum there
                assert np.array_equal(cs.raised, k)
                assert np.array_equal(cs.lapack[k], cs.steer[k] / 2)
                assert np.array_equal(cs.truth[k].astype(np.complex128), cs.steer[k] / 2)
            if cs.family == "H6":
                kb = g.n_fft // 64    # 250 Hz: bin 16 at N = 1024, bin 8 at N = 512
                assert f[kb] == C.BYPASS_H6 and f[kb - 1] < C.BYPASS_H6
                assert (cs.lapack[:kb] == [1.0, 0.0]).all() and cs.lapack[kb, 1] != 0
            assert (cs.lapack[~k] == [1.0, 0.0]).all()


def test_long_double_truth_vs_mpmath():
    """16 bins per family (spread over its cases) against 40-digit mpmath at 1e-17."""
    if not C.HAVE_LD:  # no 80-bit long double: the truth is this mpmath code itself
        return
    by_family = {}
    for cs in all_cases():
        by_family.setdefault(cs.family, []).append(cs)
    for fam, cases in sorted(by_family.items()):
        worst, n = 0.0, 0
        for j in range(16):
            cs = cases[(j * 7) % len(cases)]
            live = np.nonzero(cs.live)[0]
            k = live[(j * 37 + 5) % len(live)]
            worst = max(worst, C.mp_distance(cs, [k]))
            n += 1
        print(f"{fam}: long double vs mpmath, {n} bins, worst {worst:.2e}")
        assert worst <= 1e-17, (fam, worst)
