"""CPU: the rows, layouts and bounds of tests/ipd_cases.py -- that each row of the GPU test
(test_gpu_ipd_edges.py) is the input it is meant to be (where the reference's 0.01 decisions
lie, which frames are bitwise identical, that no row but `near` is decided by the last bit of a
spectrum), that each layout launches the instance it is meant to launch for any CU count, and
that the derived bound of the covariance sums stays small enough to see a flag applied one
frame off. Every assertion is a condition on the inputs and the oracle alone.

The level rows: the analysis kernel's window carries scipy's 2 / N, so its spectra are the
oracle's and its covariance products 4 |Y|^2. At 2^48 those stay below 2^127; at 2^-56 the
spectra are normal fp32 numbers (the decisions see no underflow) while the products are
subnormal (2e-38 on average; in the last frame, 17 samples under the window's start, at any
normalisation). test_levels_in_range asserts exactly that and ipd_cases' bound carries the
gradual-underflow term.
"""
import numpy as np
import pytest

import ipd_cases as IC
import utt_cases as UC


def _low(n, name):
    return IC.reference(n, name)["mask"] < 1.0


def _silent_in_both(n, name):
    """Frames whose spectra are zero in both channels."""
    Y = IC.reference(n, name)["Y"]
    return (np.abs(Y) == 0).all(axis=(0, 1))


@pytest.mark.parametrize("n", IC.SIZES)
def test_rows_are_what_they_say(n):
    H = n // 2
    for k in IC.ROWS:
        mix = IC.row(n, k)
        assert mix.shape == (2, IC.length(n, k)) and mix.dtype == np.float32
        r = IC.reference(n, k)
        assert r["mask"].shape == (H + 1, UC.n_frames(mix.shape[1], n))
        assert set(np.unique(r["mask"])) <= {0.01, 1.0}
        assert np.isfinite(r["raw"]).all() and (r["peak"] > 0 or not r["well"]), k
    T = {k: IC.reference(n, k)["mask"].shape[1] for k in IC.ROWS}
    assert T["gauss"] == 42 and T["near"] == T["near_anti"] == 11 and T["short_zero"] == 4
    assert all(T[k] == 42 for k in IC.ROWS if k not in ("near", "near_anti", "short_zero"))
    assert not np.signbit(IC.row(n, "ch1_zero")[1]).any()
    assert not IC.row(n, "ch1_zero")[1].any() and not IC.row(n, "ch0_zero")[0].any()
    assert not IC.row(n, "short_zero")[1].any()
    m0 = IC.row(n, "ch1_mul0")
    assert np.array_equal(m0[0], IC.row(n, "ch1_zero")[0]) and not m0[1].any()
    neg = int(np.signbit(m0[1]).sum())
    assert 0.4 * m0.shape[1] < neg < 0.6 * m0.shape[1]   # it really holds negative zeros
    g = IC.row(n, "gauss")
    assert 0.09 < g.std() < 0.11
    for k, e in IC.LEVELS.items():
        assert np.array_equal(IC.row(n, k), g * np.float32(2.0 ** e))
    a = IC.row(n, "anti")
    assert np.array_equal(a[1], -a[0])
    nr, na = IC.row(n, "near"), IC.row(n, "near_anti")
    for d in (nr[1].astype(np.float64) - nr[0], na[1].astype(np.float64) + na[0]):
        assert 0.5e-5 < d.std() < 2e-5
    # the spans: which frames are silent in one or both channels
    L = IC.length(n, "gauss")
    assert IC.silent_frames(n, [IC.dead_span(n)], L) == [14, 15, 16, 17]
    ds = IC.row(n, "ch1_dead_span")
    a_, b_ = IC.dead_span(n)
    assert not ds[1, a_:b_].any() and ds[1, a_ - 1] != 0 and ds[1, b_] != 0 and ds[0, a_:b_].all()
    assert IC.silent_frames(n, IC.both_zero_spans(n), L) == [0, 1, 2, 22, 23, 24]
    assert np.nonzero(_silent_in_both(n, "both_zero_span"))[0].tolist() == [0, 1, 2, 22, 23, 24]


@pytest.mark.parametrize("n", IC.SIZES)
def test_silent_channel_decisions(n):
    """A silent channel has angle 0: 0.01 exactly where the other channel is real and positive,
    that is in bins 0 and N / 2 by sign, and in no inner bin."""
    for k in ("ch1_zero", "ch0_zero", "ch1_mul0"):
        low = _low(n, k)
        assert not low[1:-1].any(), k
        assert not _silent_in_both(n, k).any()
        for e in (0, -1):
            assert 10 <= int(low[e].sum()) <= 29, (k, e, int(low[e].sum()))
        Y = IC.reference(n, k)["Y"]
        live = Y[1] if k == "ch0_zero" else Y[0]
        for e in (0, -1):
            assert np.array_equal(low[e], live[e].real > 0), (k, e)
    assert np.array_equal(IC.reference(n, "ch1_mul0")["mask"], IC.reference(n, "ch1_zero")["mask"])
    # the dead span: its silent frames decide like a silent row; no 0.01 in an inner bin at all
    low = _low(n, "ch1_dead_span")
    assert not low[1:-1].any()
    Y = IC.reference(n, "ch1_dead_span")["Y"]
    assert (np.abs(Y[1][:, 14:18]) == 0).all() and (np.abs(Y[0][:, 14:18]) > 0).all()
    for e in (0, -1):
        assert np.array_equal(low[e, 14:18], Y[0][e, 14:18].real > 0)
    # frames silent in both channels are all 0.01, every other inner cell 1
    low = _low(n, "both_zero_span")
    both = _silent_in_both(n, "both_zero_span")
    assert low[:, both].all() and not low[1:-1][:, ~both].any()
    # the short row: apart from its last frame (zero in both channels after the window's zero)
    low = _low(n, "short_zero")
    both = _silent_in_both(n, "short_zero")
    assert np.nonzero(both)[0].tolist() == [3]
    assert not low[1:-1, :3].any()


def test_zero_sign_cells():
    """The only cells weighted 1.0 on zero spectra (the sign of a pocketfft zero) are those of
    ipd_cases.ZERO_SIGN: bin 205 of `short_zero`'s last frame at N = 512, whose one sample under
    the window's zero is negative; apart from it that frame is all 0.01, as it is at N = 1024."""
    found = {(n, k): IC.zero_sign_cells(n, k) for n in IC.SIZES for k in IC.ROWS}
    assert {key: v for key, v in found.items() if v} == IC.ZERO_SIGN
    assert IC.row(512, "short_zero")[0, 512] < 0 < IC.row(1024, "short_zero")[0, 1024]
    Y = IC.reference(512, "short_zero")["Y"]
    assert Y[0, 205, 3] == 0 and np.signbit(Y[0, 205, 3].real)
    low = _low(512, "short_zero")[:, 3]
    assert low.sum() == 256 and not low[205]
    assert _low(1024, "short_zero")[:, 3].all()


@pytest.mark.parametrize("n", IC.SIZES)
def test_identical_and_colinear_decisions(n):
    assert not _low(n, "anti").any()
    assert not _low(n, "near_anti").any()
    assert _low(n, "ident_all").all()
    assert IC.identical_frames(n, "ident_all") == list(range(42))
    low = _low(n, "ident_spans")
    assert np.nonzero(low.all(axis=0))[0].tolist() == list(IC.IDENT_FRAMES)
    assert IC.identical_frames(n, "ident_spans") == list(IC.IDENT_FRAMES)
    other = np.ones(42, bool)
    other[list(IC.IDENT_FRAMES)] = False
    assert not low[1:-1][:, other].any()
    want = set(IC.IDENT_FRAMES)
    assert {0, 41, 7, 8, 31, 32} <= want and 20 in want and not {19, 21} & want
    for s0 in range(0, 42, IC.STEP):   # every step keeps a frame that is not identical
        assert set(range(s0, min(42, s0 + IC.STEP))) - want
    for k in ("gauss", "anti", "near", "near_anti", "ch1_zero", "ch1_dead_span"):
        assert IC.identical_frames(n, k) == [], k


@pytest.mark.parametrize("n", IC.SIZES)
def test_levels_in_range(n):
    g = IC.reference(n, "gauss")
    tiny, huge = 2.0 ** -126, 2.0 ** 127
    for k in IC.LEVELS:
        r = IC.reference(n, k)
        assert np.array_equal(r["mask"], g["mask"]), k
        a = np.abs(r["Y"].astype(np.complex128))
        nz = a[a > 0]
        assert 2 * nz.min() >= tiny and 2 * nz.max() < 2.0 ** 64, k       # the spectra 2 Y
        p = 4 * (a ** 2)                                                   # the products
        assert p.max() < huge and 4 * r["sums"][:, :2].max() < huge, k
        sub = float((p[a > 0] < tiny).mean())
        print(f"N={n} {k}: 4 |Y|^2 in [{p[a > 0].min():.3g}, {p.max():.3g}], {sub:.3f} of the "
              "non-zero cells subnormal")
        assert sub == 0.0 or k == "lvl_m56"
    # the fast test's norm p0 p1 leaves the fp32 range at the outer levels: it can clear nothing
    for k, cmp in (("lvl_m56", lambda x: x < 2.0 ** -149), ("lvl_p48", lambda x: x > huge)):
        a = np.abs(IC.reference(n, k)["Y"].astype(np.complex128))
        assert np.median(cmp(16 * (a[0] * a[1]) ** 2)) == 1


@pytest.mark.parametrize("n", IC.SIZES)
def test_tie_sets(n):
    for k in ("gauss", "anti", "near_anti") + tuple(IC.LEVELS):
        assert not IC.reference(n, k)["ties"].any(), k
    for k in IC.ROWS:
        if k != "near":   # no other row may excuse a count either
            assert not IC.reference(n, k)["ties"].any(), k
    r = IC.reference(n, "near")
    inner = r["ties"][1:-1].any(axis=1)
    print(f"N={n} near: {int(r['ties'].sum())} tie cells in {int(inner.sum())} of {len(inner)} "
          "inner bins")
    assert 0 < inner.sum() <= len(inner) // 8


@pytest.mark.parametrize("n", IC.SIZES)
def test_conditioning(n):
    well = [k for k in IC.ROWS if IC.reference(n, k)["well"]]
    print(f"N={n}: well-conditioned rows {well}; cond_2 " +
          ", ".join(f"{k} {IC.reference(n, k)['cond']:.3g}" for k in IC.ROWS))
    assert "gauss" in well and len(well) >= 4
    assert set(well) == {"gauss", "ch1_dead_span", "both_zero_span", "ident_spans"} | set(IC.LEVELS)


@pytest.mark.parametrize("n", IC.SIZES)
def test_sums_bound_cap(n):
    """The bound never exceeds SUMS_CAP of max(c00, c11) of its bin, and at that size a mask
    shifted by one frame on `ident_spans` still shows in c00."""
    worst = 0.0
    for k in IC.ROWS:
        r = IC.reference(n, k)
        scale = np.maximum(r["sums"][:, 0], r["sums"][:, 1])
        assert (scale > 0).all(), k
        frac = float((r["bound"] / scale[:, None]).max())
        worst = max(worst, frac)
        assert frac <= IC.SUMS_CAP, (k, frac)
    print(f"N={n}: largest bound {worst:.3g} of max(c00, c11)")
    r = IC.reference(n, "ident_spans")
    shifted = np.roll(r["mask"], 1, axis=1)
    move = np.abs(IC.fp64_sums(r["Y"], shifted)[:, 0] - r["sums"][:, 0])
    seen = move > 2 * r["bound"][:, 0]
    print(f"N={n}: a mask one frame off moves c00 by a median of "
          f"{np.median(move / r['sums'][:, 0]):.3g} of c00; past twice the bound in "
          f"{seen.mean():.3f} of the bins")
    assert seen.mean() >= 0.99


@pytest.mark.parametrize("n", IC.SIZES)
@pytest.mark.parametrize("R", UC.CPU_RS)
def test_layout_arithmetic(R, n):
    G = IC.grid(R, n)
    seen = set()
    for names in IC.layout("pieces", R, n):
        mix, lens = IC.batch(n, names)
        assert -(-UC.n_frames(int(lens.max()), n) // IC.CHUNK) == IC.GX
        assert IC.GX * len(names) <= G // 4
        assert IC.split_of(len(names), R, n) == (0, 4)
        seen |= set(names)
    assert seen == set(IC.ROWS)
    (names,) = IC.layout("whole", R, n)
    assert IC.GX * len(names) == G and IC.split_of(len(names), R, n) == (G, 1)
    assert set(names) == set(IC.ROWS)
    pos = {k: [p for p, x in enumerate(names) if x == k] for k in IC.ROWS}
    assert all(len(v) >= 2 for v in pos.values())
    assert all(len({p % len(IC.ROWS) for p in v[:len(IC.ROWS)]}) == len(v[:len(IC.ROWS)])
               for v in pos.values())   # copies at different places of the cycle
    seen = set()
    for names in IC.layout("mixed", R, n):
        whole, P = IC.split_of(len(names), R, n)
        assert whole == G and P >= 2                      # the tail is split
        assert names[:G // IC.GX] == IC.whole_rows(R, n)
        seen |= set(names[G // IC.GX:])
    assert seen == set(IC.ROWS)
    # zero beyond each row's length, signed zeros kept
    mix, lens = IC.batch(n, ["ch1_mul0", "near", "short_zero"])
    assert mix.shape[2] % 4 == 0 and not mix[1, :, lens[1]:].any()
    assert np.array_equal(mix[0, :, :lens[0]].view(np.uint32), IC.row(n, "ch1_mul0").view(np.uint32))
