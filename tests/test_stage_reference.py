"""CPU: the references of tests/stage_cases.py against direct transcriptions of the reference
lines they restate, the caps on the inputs that let the project's tolerances apply (the
condition number of the MPDR solves, the share of loose IPD bounds), and the argument checks of
avz_chunk_split / avz_chunk_merge that return before any HIP call."""
import ctypes as ct

import numpy as np
import pytest

import stage_cases as SC
import train_cases as TC
from oracle import avz_oracle as O


# ----------------------------------------------------------------------------- 1. MPDR
@pytest.mark.parametrize("n", SC.SIZES)
def test_mpdr_reference_shapes_and_condition(n):
    x, lens = SC.mpdr_batch(n)
    H = n // 2
    assert [SC.n_frames(int(L), n) for L in lens] == [3, 4, 5, 32, 33, 66]
    worst = 0.0
    for b, r in enumerate(SC.mpdr_reference(n)):
        L = int(lens[b])
        assert r["T"] == SC.n_frames(L, n)
        assert r["out"].shape == ((r["T"] - 1) * H,) and np.isfinite(r["out"]).all()
        assert np.isfinite(r["W"]).all() and np.isfinite(r["cov"]).all()
        # the loop-faithful covariance (oracle_debug.py:56-64) with every weight 1
        Y = O.stft(x[b, :, :L], nperseg=n, noverlap=H)[2]
        Rl = O.covariance_loop(Y, np.ones(Y.shape[1:]))
        assert np.abs(Rl - r["R"]).max() <= 1e-12 * np.abs(r["R"]).max()
        s = r["R"] * (r["T"] + 1e-6)
        np.testing.assert_array_equal(r["cov"][:, 2] + 1j * r["cov"][:, 3], s[:, 0, 1])
        assert (r["cov"][:, 4] == r["T"]).all()
        # the loop-faithful solve (oracle_debug.py:66-79)
        Wl = O.mvdr_weights_loop(r["R"], r["f"], SC.MPDR_SIGMA, O.ANGLE_TARGET, SC.MPDR_D,
                                 SC.C_SOUND)
        assert np.abs(Wl - r["W"]).max() <= 1e-9 * np.abs(r["W"]).max()
        # the condition on the inputs: every solved bin is well conditioned
        ok = r["f"] >= O.FMIN_MVDR
        cond = np.linalg.cond(r["R"][ok] + SC.MPDR_SIGMA * np.eye(2), 2)
        worst = max(worst, float(cond.max()))
        assert (r["W"][~ok] == 0).all()
    print(f"N={n}: largest cond_2(R / (T + 1e-6) + sigma I) = {worst:.2f} (cap {SC.COND_MAX})")
    assert worst <= SC.COND_MAX


# ----------------------------------------------------------------------------- 2. SRP
@pytest.mark.parametrize("n", SC.SIZES)
@pytest.mark.parametrize("d", SC.SRP_SPACINGS)
def test_srp_reference(n, d):
    x, lens = SC.srp_batch(n, d)
    assert int(lens[-1]) == n - 1
    f = np.fft.rfftfreq(n, 1.0 / SC.FS)
    for lo, hi in (SC.SRP_BAND_ON_BINS,):
        assert lo in f and hi in f
        assert int(((f >= lo) & (f <= hi)).sum()) == {512: 55, 1024: 109}[n]
    assert not ((f >= SC.SRP_BAND_EMPTY[0]) & (f <= SC.SRP_BAND_EMPTY[1])).any()
    for b in range(3):
        y = x[b, :, :int(lens[b])]
        ang, db, tau = SC.srp_reference(y, n, d)
        # the oracle's restatement and the script's own loop
        a0, p0 = O.srp_scan(y, n_fft=n, d=d)
        assert np.array_equal(ang, a0) and np.abs(db - p0).max() <= 1e-9
        if b == 0:
            _, pt = SC.srp_transcription(y, n, d)
            assert np.abs(db - pt).max() <= 1e-6   # scipy's fp64 spectra, not complex64
        assert db.max() == 0.0 and np.isfinite(db).all()
        tol_db = 10 / np.log(10) * tau / 10 ** (db.min() / 10)
        print(f"N={n} d={d} L={int(lens[b])}: map range {-db.min():.3f} dB, argmax "
              f"{ang[db.argmax()]:.0f} deg, tau {tau:.2e} ({tol_db:.1e} dB at the minimum)")
        assert 0 < tau < 1e-4
        if SC.n_frames(int(lens[b]), n) >= 32:
            assert abs(ang[db.argmax()] - SC.SRP_ANGLE) <= 1.0
    y = x[2, :, :int(lens[2])]
    # an angle range: the sub-range of the whole scan, up to the other maximum
    a2, db2, _ = SC.srp_reference(y, n, d, n_angles=121, angle_lo=30.0, angle_hi=150.0)
    _, db, _ = SC.srp_reference(y, n, d)
    assert np.allclose(a2, np.arange(30, 151))
    assert np.abs((db2 - db2[0]) - (db[30:151] - db[30])).max() <= 1e-9
    assert SC.srp_reference(y, n, d, n_angles=1)[1].tolist() == [0.0]
    # the degenerate maps: all-zero input and a band without a bin are NaN throughout
    assert np.isnan(SC.srp_reference(np.zeros_like(y), n, d)[1]).all()
    assert np.isnan(SC.srp_reference(y, n, d, *SC.SRP_BAND_EMPTY)[1]).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.isnan(O.srp_scan(np.zeros_like(y), n_fft=n, d=d)[1]).all()


# ----------------------------------------------------------------------------- 3. chunks
@pytest.mark.parametrize("channels", [1, 2])
def test_split_reference(channels):
    x = SC.split_input(channels)
    ref = SC.split_reference(x, SC.SPLIT_LENS, SC.SPLIT_ITEMS, SC.SPLIT_CHUNK)
    assert ref.shape == (7, channels, SC.SPLIT_CHUNK)
    # the driver's own lines (inference.py:189-195) on [len, channels] arrays
    for i, (u, s) in enumerate(SC.SPLIT_ITEMS):
        y = x[u, :, :SC.SPLIT_LENS[u]].T
        chunk = y[s:s + SC.SPLIT_CHUNK]
        if len(chunk) < SC.SPLIT_CHUNK:
            chunk = np.pad(chunk, ((0, SC.SPLIT_CHUNK - len(chunk)), (0, 0)))
        np.testing.assert_array_equal(ref[i], chunk.T)
    assert not ref[3].any() and ref[0, :, 1000:].any() == 0 and ref[0, :, :1000].all()
    assert SC.SPLIT_CHUNK % 4 and SC.SPLIT_CHUNK > 1024
    assert (SC.SPLIT_LENS[1] - 0) % 4 and (SC.SPLIT_LENS[2] - 1022) % 4 and 2049 - 1022 > 1024
    assert all(s >= SC.SPLIT_CHUNK for s in SC.SPLIT_ITEM_CH_STRIDES)
    assert SC.SPLIT_ITEM_CH_STRIDES[0] % 4 == 0 and SC.SPLIT_ITEM_CH_STRIDES[1] % 4


@pytest.mark.parametrize("hop,iol,max_len", SC.MERGE_SETS)
def test_merge_references(hop, iol, max_len):
    io, lens, base = SC.merge_case(hop, iol, max_len)
    assert max(lens) == max_len and 1 in lens and any(L % hop for L in lens)
    assert sorted(base.tolist()) != base.tolist()
    y64, mag = SC.merge_reference_f64(io, lens, base, hop, iol)
    y32, peak = SC.merge_reference_f32(io, lens, base, hop, iol)
    plant = SC.merge_plant_positions(lens)
    for u, L in enumerate(lens):
        assert y64[u].shape == y32[u].shape == (L,)
        assert (np.abs(y32[u] - y64[u]) <= 2.0 ** -23 * mag[u]).all()
        # the largest value sits where it was planted
        assert int(np.argmax(np.abs(y32[u]))) == plant[u] and peak[u] == SC.MERGE_PLANT
        n = np.arange(L)
        cnt = sum(((c * hop <= n) & (n < c * hop + iol)).astype(int) for c in range(-(-L // hop)))
        if iol < hop:
            gap = n % hop >= iol
            assert gap.any() or L <= iol
            assert (cnt[gap] == 0).all() and (y32[u][gap] == 0).all() and (y64[u][gap] == 0).all()
        else:
            assert cnt.min() >= 1
        assert cnt.max() <= -(-iol // hop)
    if (hop, iol) == (7, 20):
        assert -(-iol // hop) == 3
    if max_len == 2500:   # the planted peaks: first block, last partial block, last sample
        assert plant[0] < 1024 and plant[2] >= 2048 and plant[3] == lens[3] - 1


def test_chunk_argument_checks():
    """Every AVZ_ERR_SHAPE / AVZ_ERR_ARG return of avz_chunk_split and avz_chunk_merge; each
    call fails a check on the host, so the (never dereferenced) pointers are dummies."""
    from avz import _lib
    lib = _lib.lib
    SHAPE, ARG, OK = _lib.AVZ_ERR_SHAPE, _lib.AVZ_ERR_ARG, _lib.AVZ_OK
    p = ct.c_void_p(4096)

    def split(n_items=2, channels=2, chunk=100, utt=p, start=p, ln=p, x=p, items=p,
              item_stride=200, item_ch_stride=100):
        return lib.avz_chunk_split(n_items, channels, chunk, utt, start, ln, x, 1000, 500, items,
                                   item_stride, item_ch_stride, None)
    assert split(n_items=-1) == SHAPE
    assert split(chunk=0) == SHAPE
    assert split(channels=0) == SHAPE
    assert split(channels=3) == SHAPE
    assert split(n_items=0, utt=None, start=None, ln=None, x=None, items=None) == OK
    assert split(utt=None) == ARG
    assert split(start=None) == ARG
    assert split(ln=None) == ARG
    assert split(x=None) == ARG
    assert split(items=None) == ARG
    assert split(item_ch_stride=99) == SHAPE
    assert split(item_stride=199) == SHAPE

    def merge(batch=2, max_len=100, hop=10, iol=20, ln=p, base=p, io=p, io_stride=20, y=p,
              y_stride=100, peak=p):
        return lib.avz_chunk_merge(batch, max_len, hop, iol, ln, base, io, io_stride, y, y_stride,
                                   peak, 0, 0.0, None)
    assert merge(batch=-1) == SHAPE
    assert merge(max_len=-1) == SHAPE
    assert merge(hop=0) == SHAPE
    assert merge(iol=0) == SHAPE
    assert merge(batch=0, ln=None, base=None, io=None, y=None, peak=None) == OK
    assert merge(max_len=0, ln=None, base=None, io=None, y=None, peak=None) == OK
    assert merge(ln=None) == ARG
    assert merge(base=None) == ARG
    assert merge(io=None) == ARG
    assert merge(y=None) == ARG
    assert merge(peak=None) == ARG
    assert merge(io_stride=19) == SHAPE
    assert merge(y_stride=99) == SHAPE


# ----------------------------------------------------------------------------- 4. metrics
def test_metrics_references():
    o, t, i = SC.metrics_inputs()
    assert SC.MET_STRIDE % 4 == 0 and max(SC.MET_LENS) <= SC.MET_STRIDE
    # a partial float4 at the end of a row (n + 3 < L false with samples left)
    assert sum(L % 4 != 0 for L in SC.MET_LENS) >= 4
    for b, L in enumerate(SC.MET_LENS):
        s, bound = SC.metrics_sums(o[b, :L], t[b, :L], i[b, :L])
        a = [x[b, :L].astype(np.float64) for x in (o, t, i)]
        dots = [a[0] @ a[0], a[1] @ a[1], a[2] @ a[2], a[0] @ a[1], a[0] @ a[2], a[1] @ a[2]]
        assert (np.abs(s - dots) <= bound).all()
        m = SC.metrics_reference(o[b, :L], t[b, :L], i[b, :L])
        if L == 0:
            assert (s == 0).all() and (bound == 0).all() and (m == -np.inf).all()
            continue
        assert np.isfinite(m).all()
        # the same formulas from the sums (how the kernel evaluates them): OSIR and SIR
        eps = 1e-10
        nt, ni, no = np.sqrt(s[1]) + eps, np.sqrt(s[2]) + eps, np.sqrt(s[0]) + eps
        osir = 10 * np.log10((s[3] / nt) ** 2 * s[1] / nt ** 2
                             / ((s[4] / ni) ** 2 * s[2] / ni ** 2 + eps))
        sir = 10 * np.log10((s[3] / (no * nt)) ** 2 * s[1] / nt ** 2
                            / ((s[4] / (no * ni)) ** 2 * s[2] / ni ** 2 + 1e-10))
        np.testing.assert_allclose([osir, sir], [m[1], m[3]], rtol=1e-9, atol=1e-9)
        # scoring o / (peak + eps) moves OSINR / OSIR by the scale only where eps terms are small
        ms = SC.metrics_reference(o[b, :L], t[b, :L], i[b, :L], peak=SC.MET_PEAKS[b], eps=1e-9)
        assert np.isfinite(ms).all()
        if L > 1000:
            assert abs(ms[3] - m[3]) < 1e-6


# ----------------------------------------------------------------------------- 5. features
@pytest.mark.parametrize("n", SC.SIZES)
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("scale", SC.FEAT_NOISE_SCALES)
def test_feature_reference_and_ipd_tolerance_cap(n, name, scale):
    mix, lens = SC.feature_batch(n, name, scale)
    if scale == 1:
        assert mix is TC.batches(n)[name][0] or np.array_equal(mix, TC.batches(n)[name][0])
    else:   # the references are untouched: only the noise grew
        _, tgt, itf, _ = TC.batches(n)[name]
        resid = mix.astype(np.float64) - (tgt.astype(np.float64) + itf)[:, None, :]
        assert 0.9 * scale * 1e-3 < resid.std() < 1.1 * scale * 1e-3
    for b, r in enumerate(SC.feature_reference(n, name, scale)):
        if r is None:
            assert lens[b] < n
            continue
        Y, feat = r["Y"], r["feat"]
        T = SC.n_frames(int(lens[b]), n)
        assert Y.shape == (2, n // 2 + 1, T) and feat.shape == (2, n // 2 + 1, T)
        # the spectra behind Sample.feat: the same bits, and the oracle's complex64 ones
        np.testing.assert_array_equal(np.log(np.abs(Y[0]) + 1e-7), feat[0])
        np.testing.assert_array_equal(np.angle(Y[0]) - np.angle(Y[1]), feat[1])
        Yo = O.stft(mix[b, :, :int(lens[b])], nperseg=n, noverlap=n // 2)[2]
        assert np.abs(Yo - Y).max() <= 2e-7 * np.abs(Y).max()
        share = float((r["tol_ipd"] > SC.FEAT_IPD_LOOSE).mean())
        print(f"N={n} {name}[{b}] noise x{scale}: IPD bound above {SC.FEAT_IPD_LOOSE} rad in "
              f"{100 * share:.3f} % of the entries (cap {100 * SC.FEAT_CAP} %)")
        if scale == SC.FEAT_CAPPED_SCALE:
            assert share <= SC.FEAT_CAP
