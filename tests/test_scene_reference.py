"""CPU checks of tests/scene_cases.py, the references and bounds that test_gpu_scene_stages.py
holds csrc/avz_scene.hip to, and of the scene entry points' host-side argument checks.

* The periodic kernel h[d] = -(1/n) (-1)^d sin(pi delta) cot(pi (d - delta) / n) of the O(n^2)
  fallback, convolved circularly in fp64, equals synth.frac_delay (the rfft phase shift); an
  integer delay is np.roll.
* The fallback's error bound: an fp32 emulation of the kernel's sums stays below half of it,
  and with one kernel table misplaced by one tap exceeds the tolerance built on it.
* The AR(2) recursion as the generator runs it (zero-state segments of 256, A^256 between
  them) equals lfilter.
* Every rejecting branch of scene_check, avz_scene_mix and avz_scene_generate returns its
  code before any device call (no GPU is needed, none is touched)."""
import ctypes as ct

import numpy as np
import pytest
from scipy.signal import lfilter

import scene_cases as C
from avz import synth


# ----------------------------------------------------------------------------- periodic kernel
def _delay_tol(n, delta, y):
    """fp64 roundings of both sides: sums of n terms (16 n 2^-52 is generous) and frac_delay's
    phase 2 pi f tau, up to pi |delta| rad and rounded a few times (4 pi |delta| 2^-52)."""
    return (16 * n + 4 * np.pi * abs(delta)) * 2.0 ** -52 * np.max(np.abs(y))


@pytest.mark.parametrize("n", [14, 22, 126, 128, 1150, 4094])
def test_periodic_kernel_is_the_rfft_phase_shift(n):
    rng = np.random.default_rng(n)
    y = rng.standard_normal(n)
    worst = 0.0
    for delta in (0.3, -0.3, 2.5, -7.25, n + 3.7, -2.0 * n - 0.6, 1e-9, 2 + 1e-9, -2 - 1e-9,
                  -3 + 2e-12, 0.5):
        ref = synth.frac_delay(y, delta / C.FS, C.FS)
        got = C.cconv(y, C.periodic_kernel(n, delta))
        err = float(np.max(np.abs(got - ref)))
        worst = max(worst, err / _delay_tol(n, delta, y))
    print(f"n={n}: max |h (*) y - frac_delay| = {worst:.3f} of the fp64 tolerance")
    assert worst <= 1.0


@pytest.mark.parametrize("n", [14, 30, 126, 2306])
def test_integer_delay_is_a_roll(n):
    rng = np.random.default_rng(n)
    y = rng.standard_normal(n)
    for D in (0, 1, 2, -2, n, n + 3, -2 * n - 5):
        ref = synth.frac_delay(y, D / C.FS, C.FS)
        assert np.max(np.abs(ref - np.roll(y, D))) <= _delay_tol(n, D, y)
        assert np.array_equal(C.cconv(y, C.periodic_kernel(n, float(D))), np.roll(y, D))


def test_cases_hold_the_delays_they_name():
    for c in C.FFT_CASES + C.FB_CASES + C.EDGE_CASES:
        assert c.n % 2 == 0 and C.fft_len(c.n) == (not c.name.startswith(("fb-", "edge-fb")))
    d = C.case_deltas(C.BY_NAME["fb-n14-int"])
    assert np.array_equal(d[0], [[2.0, -2.0], [-2.0, 2.0], [2.0, -2.0]])      # exactly
    assert not any(C.is_int_delay(v) for v in d[1].ravel())
    d = C.case_deltas(C.BY_NAME["fft-n30-int"])
    assert np.array_equal(np.abs(d), np.full(d.shape, 2.0))
    assert np.array_equal(np.abs(C.case_deltas(C.BY_NAME["fft-n8-int"])), np.full((3, 2, 2), 10.0))
    d = C.case_deltas(C.BY_NAME["fb-n126-near-int"])
    s = np.abs(np.sin(np.pi * (np.abs(d) - 2.0)))
    assert np.all(s > 100 * C.INT_DELAY) and np.all(s < 1e-8)                # the convolution runs
    assert not C.case_deltas(C.BY_NAME["fb-n34-zero"]).any()
    d = C.case_deltas(C.BY_NAME["fb-n2050-broadside"])
    assert np.all(np.abs(d[:, 0]) < 1e-14) and all(C.is_int_delay(v) for v in d[:, 0].ravel())
    assert np.abs(C.case_deltas(C.BY_NAME["fb-n14-far"])).max() > 14
    assert np.abs(C.case_deltas(C.BY_NAME["fft-n4"])).max() > 4
    # fractional delays of both signs in every plain fallback case
    for n in C.FB_LENGTHS:
        d = C.case_deltas(C.BY_NAME[f"fb-n{n}"])
        assert d.min() < 0 < d.max()


# ----------------------------------------------------------------------------- fallback bound
def _emulate(c, misplace=False):
    """The fallback in numpy: fp32 tables and fp32 sums (copies for integer delays), then the
    mixing in fp64. misplace: the target's mic-0 table (or copy) of every utterance moved by
    one tap."""
    srcs, noise = C.mix_inputs(c.name)
    dl = C.case_deltas(c)
    out = []
    for b in range(c.B):
        T, I = np.zeros((2, c.n)), np.zeros((2, c.n))
        for s in range(c.S):
            for mic in range(2):
                h = C.periodic_kernel(c.n, dl[b, s, mic]).astype(np.float32)
                if misplace and s == 0 and mic == 0:
                    h = np.roll(h, 1)
                if C.is_int_delay(dl[b, s, mic]):
                    img = np.roll(srcs[b, s], int(np.argmax(h)))
                else:
                    img = C.fallback_image_fp32(srcs[b, s], h)
                (T if s == 0 else I)[mic] += img.astype(np.float64)
        out.append(C.mix_images(T, I, c.S - 1, noise[b].astype(np.float64), c.sir, c.snr))
    return {k: np.stack([r[k] for r in out]) for k in ("mix", "tgt", "itf")}


@pytest.mark.parametrize("case", [c for c in C.FB_CASES + C.EDGE_CASES if not C.fft_len(c.n)],
                         ids=lambda c: c.name)
def test_fallback_bound_holds_an_fp32_emulation_and_catches_a_misplaced_tap(case):
    ref = C.mix_case_reference(case.name)
    emu = _emulate(case)
    worst = 0.0
    for k in ("mix", "tgt", "itf"):
        err = np.abs(emu[k] - ref[k])
        slack = 2.0 ** -40                       # the fp64 restatements differ by rounding
        frac = np.max((err - slack) / np.maximum(ref["b_" + k], 1e-300))
        worst = max(worst, float(frac))
        assert np.all(err <= 0.5 * ref["b_" + k] + slack), (k, float(frac))
    print(f"{case.name}: fp32 emulation at most {max(worst, 0.0):.3f} of the derived bound")
    if "silent" in case.name and 0 in case.zero:
        return                                   # an all-zero target: nothing to misplace
    bad = _emulate(case, misplace=True)
    over = max(float(np.max(np.abs(bad[k] - ref[k]) / np.minimum(C.PROJECT_TOL, ref["tol_" + k])))
               for k in ("mix", "tgt"))
    assert over > 1.0, over


# ----------------------------------------------------------------------------- AR(2) scan
@pytest.mark.parametrize("n", [2, 255, 256, 257, 1000])
def test_segment_scan_is_lfilter(n):
    x = np.random.default_rng(n).standard_normal(n)
    ref = lfilter([1.0], [1.0, -1.4, 0.45], x)
    got = C.ar2_segment_scan(x)
    err = float(np.max(np.abs(got - ref)))
    print(f"n={n}: max |scan - lfilter| = {err:.2e} ({err / np.max(np.abs(ref)):.2e} of max|y|)")
    assert err <= 2.0 ** -40 * np.max(np.abs(ref))    # the fp64 term of scene_cases.draw_tol


def test_generator_cases_have_sound_in_every_source():
    for c in C.GEN_CASES:
        ang, srcs, z = C.gen_reference(c.name)
        assert srcs.shape == (c.B, 1 + c.K, c.n) and z.shape == (c.B, 2, c.n)
        assert np.all(np.abs(srcs).max(axis=-1) > 0), c.name
        blk = int(0.25 * c.fs)
        if c.n > blk:                            # some keep block is silent, some is not
            assert np.any(srcs == 0.0) or c.n < 4 * blk, c.name


def test_odd_length_generator_case_is_audible():
    g = C.REVERB_GEN
    for n in g["lengths"]:
        assert n % 2 == 1 and n < 4000                       # one keep block at 16 kHz
        for b in range(g["B"]):
            key = synth._key(g["start"] + b, g["seed"])
            for s in range(1 + g["K"]):
                assert np.abs(synth.speech_like_philox(key, s, n, 16000.0)).max() > 0


# ----------------------------------------------------------------------------- argument checks
def _lib():
    from avz import _lib
    return _lib


_P = ct.c_void_p(0x1000)       # never dereferenced: every call below returns on the host


def _mix(**kw):
    L = _lib()
    a = dict(batch=2, n_src=2, n=30, src=_P, angles=_P, noise=_P, mic_d=0.08, c=343.0, fs=16000.0,
             sir=0.0, snr=5.0, mix=_P, mix_stride=60, ch_stride=30, tgt=_P, itf=_P, ref_stride=30,
             ws=_P, ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = L.lib.avz_scene_workspace_bytes(max(a["batch"], 1), max(a["n_src"], 1),
                                                        max(a["n"], 1))
    return L.lib.avz_scene_mix(a["batch"], a["n_src"], a["n"], a["src"], a["angles"], a["noise"],
                               a["mic_d"], a["c"], a["fs"], a["sir"], a["snr"], a["mix"],
                               a["mix_stride"], a["ch_stride"], a["tgt"], a["itf"],
                               a["ref_stride"], a["ws"], a["ws_bytes"], None)


def _gen(**kw):
    L = _lib()
    a = dict(batch=2, start=0, k=1, n=30, seed=0, mic_d=0.08, c=343.0, fs=16000.0, sir=0.0,
             snr=5.0, mix=_P, mix_stride=60, ch_stride=30, tgt=_P, itf=_P, ref_stride=30, ws=_P,
             ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = L.lib.avz_scene_generate_workspace_bytes(max(a["batch"], 1),
                                                                 max(a["k"], 0), max(a["n"], 1))
    return L.lib.avz_scene_generate(a["batch"], a["start"], a["k"], a["n"], a["seed"], a["mic_d"],
                                    a["c"], a["fs"], a["sir"], a["snr"], a["mix"], a["mix_stride"],
                                    a["ch_stride"], a["tgt"], a["itf"], a["ref_stride"], a["ws"],
                                    a["ws_bytes"], None)


def test_scene_entry_points_reject_on_the_host():
    L = _lib()
    SHAPE, ARG, UNSUP = L.AVZ_ERR_SHAPE, L.AVZ_ERR_ARG, L.AVZ_ERR_UNSUPPORTED
    nan = float("nan")
    big = 1 << 60
    for f in (_mix, _gen):
        assert f(n=31) == SHAPE and f(n=1) == SHAPE and f(n=0) == SHAPE      # odd n, n < 2
        assert f(batch=-1) == SHAPE
        assert f(batch=0) == L.AVZ_OK
        assert f(batch=0, mix=None, tgt=None, itf=None, ws=None) == L.AVZ_OK
        for name in ("mix", "tgt", "itf", "ws"):
            assert f(**{name: None}) == ARG, name
        for name in ("fs", "c"):
            for v in (0.0, -1.0, nan):
                assert f(**{name: v}) == ARG, (name, v)
        assert f(ch_stride=29) == SHAPE
        assert f(mix_stride=59) == SHAPE                 # < ch_stride + n with batch > 1
        assert f(ref_stride=29) == SHAPE
        assert f(batch=65536, ws_bytes=big) == UNSUP     # grid.y
    # one utterance needs no batch strides, so those alone do not reject it: the next check
    # (the workspace, one byte short) does
    need = L.lib.avz_scene_workspace_bytes(1, 2, 30)
    assert _mix(batch=1, mix_stride=0, ref_stride=0, ws_bytes=need - 1) == SHAPE
    assert _mix(n_src=0) == SHAPE
    for name in ("src", "angles", "noise"):
        assert _mix(**{name: None}) == ARG, name
    assert _mix(ws_bytes=L.lib.avz_scene_workspace_bytes(2, 2, 30) - 1) == SHAPE
    assert _mix(n=34, ws_bytes=L.lib.avz_scene_workspace_bytes(2, 2, 34) - 1) == SHAPE
    # the fallback's grid.y holds batch * n_src * 2 signals
    assert _mix(batch=2, n_src=16384, n=14, ws_bytes=big) == UNSUP
    assert _mix(batch=16384, n_src=2, n=14, mix_stride=28, ch_stride=14, ref_stride=14,
                ws_bytes=big) == UNSUP
    assert _gen(batch=8192, k=3, n=14, mix_stride=28, ch_stride=14, ref_stride=14,
                ws_bytes=big) == UNSUP
    assert _gen(ws_bytes=L.lib.avz_scene_generate_workspace_bytes(2, 1, 30) - 1) == SHAPE
    assert _gen(n=34, ws_bytes=L.lib.avz_scene_generate_workspace_bytes(2, 1, 34) - 1) == SHAPE
    assert _gen(start=-1) == ARG
    assert _gen(k=-1) == ARG and _gen(k=256) == ARG
    assert _gen(fs=3.999) == ARG and _gen(fs=nan) == ARG
    # the workspace sizes: the generator's is its scratch plus the back end's
    o_src, o_noise, o_ang = C.gen_layout(2, 2, 30)
    al = lambda x: (x + 255) & ~255  # noqa: E731
    scratch = o_ang + al(2 * 2 * 8) + 2 * al(2 * 2 * 1 * 16)
    assert L.lib.avz_scene_generate_workspace_bytes(2, 1, 30) == scratch + \
        L.lib.avz_scene_workspace_bytes(2, 2, 30)
