"""CPU: the layouts and fp64 references of tests/utt_cases.py -- that the batches the GPU test
(test_gpu_utt_rounds.py) launches have the geometry its kernel paths need for any CU count,
that the sampled rows cover the table, and that the inputs let the project's parity tolerances
apply (finite references with a peak, well-conditioned IBM solves)."""
import numpy as np
import pytest

import utt_cases as UC
from oracle import avz_oracle as O


@pytest.mark.parametrize("n", UC.SIZES)
@pytest.mark.parametrize("R", UC.CPU_RS)
def test_first_layout_geometry(R, n):
    lens, classes, keys = UC.layout(R, n)
    H, fb = n // 2, UC.FB[n]
    B = UC.ROUNDS * R
    assert len(lens) == len(classes) == len(keys) == B and B % R == 0
    assert UC.l_max(n) == {1024: 32256, 512: 32512}[n] == int(lens.max())
    assert UC.n_frames(UC.l_max(n), n) == 4 * fb
    # T(L) of every class is what the table says
    for cls, frames in UC.CLASS_FRAMES.items():
        assert UC.n_frames(UC.class_length(cls, n), n) == frames(fb), cls
    assert UC.class_length("skip0", n) == 0 and UC.class_length("skipN", n) == n - 1
    for b, c in enumerate(classes):
        assert c == UC.CLASS_TABLE[(b % R) % 8][b // R]
        if c == "rand":
            assert n <= lens[b] <= UC.l_max(n)
        else:
            assert lens[b] == UC.class_length(c, n)
    # every class of the table occurs, in every round it is listed for
    for g8, row in enumerate(UC.CLASS_TABLE):
        for r, c in enumerate(row):
            assert classes[g8 + r * R] == c
    # no analysis split and no synthesis pieces: the items fill whole rounds of the analysis
    # grid and the rows whole rounds of the synthesis grid
    nch = -(-UC.n_frames(int(lens.max()), n) // UC.CHUNK)
    assert nch == {1024: 2, 512: 4}[n]
    assert (nch * B) % (UC.BLOCKS_PER_CU[n] * R) == 0
    # the sampled set: block 0, one of the last eight blocks, each (class, round)
    blocks = UC.sampled_blocks(R)
    assert blocks[0] == 0 and R - 8 <= blocks[-1] < R and len(blocks) == 16
    rows = UC.sampled_rows(R)
    seen = {((b % R) % 8, b // R) for b in rows}
    assert seen == {(c, r) for c in range(8) for r in range(UC.ROUNDS)}
    red = UC.sampled_rows(R, UC.reduced_blocks(R))
    assert {((b % R) % 8, b // R) for b in red} == seen and (R - 1) in red
    # the permutation moves every row to another block and another round
    src = UC.block_permutation(R)
    assert sorted(src.tolist()) == list(range(B))
    pos = np.empty(B, np.int64)
    pos[src] = np.arange(B)
    assert (pos % R != np.arange(B) % R).all() and (pos // R != np.arange(B) // R).all()
    # with it the batch still has whole rounds and the same longest row
    assert int(lens[src].max()) == int(lens.max())


@pytest.mark.parametrize("variant", sorted(UC.L2_VARIANTS))
@pytest.mark.parametrize("R", UC.CPU_RS)
def test_second_layout_geometry(R, variant):
    lens, classes, keys = UC.layout2(R, variant)
    bs = UC.b_star(R)
    assert len(lens) == R and int(lens.max()) == UC.L2_MAX
    nch = -(-UC.n_frames(UC.L2_MAX, 1024) // UC.CHUNK)
    assert nch == 5
    # two analysis blocks per CU: 5 R items, four whole rounds and a tail of R items
    G = UC.BLOCKS_PER_CU[1024] * R
    n_items = nch * R
    a_whole = n_items // G * G
    assert a_whole == 4 * R and n_items - a_whole == R and 2 * (n_items - a_whole) <= G
    # b* straddles a_whole (these CU counts; straddles() is the GPU test's skip condition)
    assert UC.straddles(R) and 5 * bs < a_whole < 5 * bs + 5
    assert not UC.straddles(80)
    assert tuple(classes[bs - 1:bs + 4]) == UC.L2_VARIANTS[variant]
    assert all(c == "rand" for i, c in enumerate(classes) if not bs - 1 <= i <= bs + 3)
    assert UC.n_frames(int(lens[bs - 1]), 1024) == 5 * UC.CHUNK
    own = -(-UC.n_frames(int(lens[bs]), 1024) // UC.CHUNK)
    if variant == "straddle":
        assert 5 * bs + own > a_whole          # some chunks whole, the rest split
    else:
        assert own == 1 and 5 * bs + own <= a_whole < 5 * bs + nch
    assert lens[bs + 2] == 0 and lens[bs + 1] == 1024
    assert set(range(bs - 1, bs + 4)) | {0, R - 1} == set(UC.sampled_rows2(R))
    assert ((lens >= 1024) | (lens == 0)).all()


@pytest.mark.parametrize("n", UC.SIZES)
@pytest.mark.parametrize("plan", sorted(UC.PLANS))
def test_sampled_references_finite(plan, n):
    """R = 32: every sampled live row has a finite reference with a raw peak > 0 (no row left
    out for a NaN reference)."""
    R = 32
    lens, classes, keys = UC.layout(R, n)
    H = n // 2
    n_live = 0
    for b in UC.sampled_rows(R):
        L = int(lens[b])
        if classes[b] in UC.SKIPPED:
            assert L < n
            continue
        assert L >= n
        r = UC.reference(plan, n, int(keys[b]), L)
        assert r["raw"].shape == ((UC.n_frames(L, n) - 1) * H,)
        assert np.isfinite(r["raw"]).all() and r["peak"] > 0, (b, classes[b])
        assert np.isfinite(r["out"]).all()
        eps = UC.PLANS[plan].get("norm_eps", 0.0)
        assert abs(np.abs(r["out"]).max() - r["peak"] / (r["peak"] + eps)) <= 1e-12
        n_live += 1
    assert n_live == 36


@pytest.mark.parametrize("plan", ["ibm", "ipd"])
def test_second_layout_references_finite(plan):
    R = 32
    for variant in sorted(UC.L2_VARIANTS):
        lens, classes, keys = UC.layout2(R, variant)
        for b in UC.sampled_rows2(R):
            if classes[b] in UC.SKIPPED:
                continue
            r = UC.reference(plan, 1024, int(keys[b]), int(lens[b]))
            assert np.isfinite(r["raw"]).all() and r["peak"] > 0, (variant, b)


@pytest.mark.parametrize("n", UC.SIZES)
def test_ibm_solves_well_conditioned(n):
    """cond_2(R / (sum m + 1e-6) + sigma I) <= 100 in every solved bin of the sampled rows of
    the IBM plan (sigma = 1): test_stage_reference.py's cap, under which WAVE_TOL applies."""
    R = 32
    lens, classes, keys = UC.layout(R, n)
    sigma = UC.PLANS["ibm"]["sigma"]
    worst = 0.0
    for b in UC.sampled_rows(R):
        if classes[b] in UC.SKIPPED:
            continue
        r = UC.reference("ibm", n, int(keys[b]), int(lens[b]))
        ok = r["f"] >= O.FMIN_MVDR
        cond = np.linalg.cond(r["R"][ok] + sigma * np.eye(2), 2)
        worst = max(worst, float(cond.max()))
    print(f"N={n}: largest cond_2 = {worst:.6f} (cap {UC.COND_MAX})")
    assert worst <= UC.COND_MAX
