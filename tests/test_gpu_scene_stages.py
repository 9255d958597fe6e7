"""The scene generator's kernels (csrc/avz_scene.hip) against fp64 references at edge lengths
(cases, references and the derivation of every bound: tests/scene_cases.py; CPU checks of
those: tests/test_scene_reference.py).

A. avz_scene_mix on the FFT path: lengths 2 .. 4320 with every radix {8, 4, 2, 5, 3} first and
   later in the pass list, n_src 1 .. 5, delays beyond n, exact integer delays, delta = 0;
   per sample within 2^-22 |ref| + 2^-40.
B. The O(n^2) fallback: lengths 14 .. 4102 around the kernel's 128-, 1151-, 2048- and
   2304-entry edges, fractional delays of both signs, 0, +-2 exactly, +-(2 + 1e-9), |delta| > n;
   within the smaller of 2e-5 and the derived fp32 bound, copies within A's tolerance; no NaN
   in the kernel tables.
C. avz_scene_generate's front end read back from the head of the workspace: angles bit-equal
   to synth.scene_draws_philox, sources and noise within 2^-24 |ref| + 2^-40 max|ref| of
   speech_like_philox / philox_normals; then the outputs against the fp64 mixing of the
   device's own draws at A's and B's tolerances. Odd n through avz_scene_reverb_generate.
D. Mixing edges at n = 30 and 34: K = 0, a silent target (every output exactly 0), silent
   interferers, sir_db +-20, snr_db -10 and 60.

Every call writes into NaN-filled rows with strides larger than needed (odd ones on every other
case) and gets a workspace of exactly the advertised size in front of a sentinel tail: padding
and tail must come back untouched. A, B and D also require equal bits from call to call and
between each utterance of a batch and its single-utterance call.

Largest deviation as a fraction of its bound (one MI355X, 2026-10-20; 76 tests, 2.9 s):
A 0.422 (n = 30, integer delays); B 0.363 on fractional delays (n = 254), 0.406 on copies
(n = 126); C sources and noise 0.993 (the fp32 store's own half ulp), outputs on the device's
draws 0.405 on FFT lengths and 0.058 on the fallback; D 0.418 (FFT, sir_db -20) and 0.121
(fallback). Value-only mutants and the two that cannot be seen: DESIGN.md section 16."""
import ctypes as ct

import numpy as np
import pytest
import torch

import room_cases
import scene_cases as C

pytestmark = pytest.mark.gpu

TAIL = 256
KEYS = ("mix", "tgt", "itf")


class _Bufs:
    """NaN-filled padded outputs and an exact-size workspace before a sentinel tail."""

    def __init__(self, dev, B, n, ws_bytes, odd):
        ch_pad, mix_pad, ref_pad = (3, 5, 7) if odd else (2, 4, 6)
        self.B, self.n, self.ws_bytes = B, n, int(ws_bytes)
        self.ch, self.rs = n + ch_pad, n + ref_pad
        self.ms = 2 * self.ch + mix_pad
        nan = float("nan")
        self.mix = torch.full((B, self.ms), nan, dtype=torch.float32, device=dev)
        self.tgt = torch.full((B, self.rs), nan, dtype=torch.float32, device=dev)
        self.itf = torch.full((B, self.rs), nan, dtype=torch.float32, device=dev)
        assert self.ws_bytes > 0
        self.ws = torch.full((self.ws_bytes + TAIL,), 0xFF, dtype=torch.uint8, device=dev)
        self.ws[self.ws_bytes:] = 0xA5

    def out_args(self):
        p = lambda t: ct.c_void_p(t.data_ptr())  # noqa: E731
        return (p(self.mix), self.ms, self.ch, p(self.tgt), p(self.itf), self.rs, p(self.ws),
                self.ws_bytes, None)

    def results(self):
        """(outputs {mix [B, 2, n], tgt, itf [B, n]}, workspace bytes); checks padding and tail."""
        torch.cuda.synchronize()
        n, ch = self.n, self.ch
        mix, tgt, itf, ws = (t.cpu().numpy() for t in (self.mix, self.tgt, self.itf, self.ws))
        assert np.all(ws[self.ws_bytes:] == 0xA5), "written past the advertised workspace"
        assert np.isnan(mix[:, n:ch]).all() and np.isnan(mix[:, ch + n:]).all()
        assert np.isnan(tgt[:, n:]).all() and np.isnan(itf[:, n:]).all()
        out = dict(mix=np.stack([mix[:, :n], mix[:, ch:ch + n]], axis=1), tgt=tgt[:, :n],
                   itf=itf[:, :n])
        for k in KEYS:
            assert np.isfinite(out[k]).all(), k
        return out, ws[:self.ws_bytes]


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                # a writable copy


def _mix(dev, c, rows=None, odd=False):
    """avz_scene_mix on case c (utterances `rows`, default all)."""
    from avz._lib import check, lib
    srcs, noise = C.mix_inputs(c.name)
    rows = slice(None) if rows is None else rows
    srcs, noise, ang = srcs[rows], noise[rows], c.angles[rows]
    B, S, n = srcs.shape
    d_src, d_noise, d_ang = _dev(srcs, dev), _dev(noise, dev), _dev(ang, dev)
    bufs = _Bufs(dev, B, n, lib.avz_scene_workspace_bytes(B, S, n), odd)
    p = lambda t: ct.c_void_p(t.data_ptr())  # noqa: E731
    check(lib.avz_scene_mix(B, S, n, p(d_src), p(d_ang), p(d_noise), c.mic_d, c.c, c.fs, c.sir,
                            c.snr, *bufs.out_args()), "avz_scene_mix")
    return bufs.results()


def _fraction(got, ref, rows=slice(None)):
    """Largest |got - ref| / tolerance over the three outputs; tolerance: the smaller of the
    project's 2e-5 and the derived one (fft_tol on FFT lengths and for copies)."""
    worst = 0.0
    for k in KEYS:
        tol = np.minimum(C.PROJECT_TOL, ref["tol_" + k][rows])
        worst = max(worst, float(np.max(np.abs(got[k] - ref[k][rows]) / tol)))
    return worst


def _bits(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in KEYS)


def _check_mix_case(dev, c, idx):
    ref = C.mix_case_reference(c.name)
    got, ws = _mix(dev, c, odd=bool(idx & 1))
    frac = _fraction(got, ref)
    print(f"{c.name}: worst error / tolerance = {frac:.3f}")
    assert frac <= 1.0, frac
    again, _ = _mix(dev, c, odd=not idx & 1)                 # other strides, same bits
    assert _bits(got, again)
    for b in range(c.B):
        one, _ = _mix(dev, c, rows=slice(b, b + 1), odd=bool(idx & 1))
        assert _bits(one, {k: got[k][b:b + 1] for k in KEYS}), b
    return got, ws, ref


# ----------------------------------------------------------------------------- A. FFT path
@pytest.mark.parametrize("idx", range(len(C.FFT_CASES)), ids=lambda i: C.FFT_CASES[i].name)
def test_fft_path_matches_fp64(gpu_device, idx):
    c = C.FFT_CASES[idx]
    got, _, ref = _check_mix_case(gpu_device, c, idx)
    # the tolerance is A's alone (no fallback bound, far below 2e-5)
    assert all(np.array_equal(ref["tol_" + k], C.fft_tol(ref[k])) for k in KEYS)
    assert abs(float(np.abs(got["mix"]).max()) - 1.0) <= 1e-6


# ----------------------------------------------------------------------------- B. fallback
@pytest.mark.parametrize("idx", range(len(C.FB_CASES)), ids=lambda i: C.FB_CASES[i].name)
def test_fallback_matches_fp64(gpu_device, idx):
    c = C.FB_CASES[idx]
    got, ws, ref = _check_mix_case(gpu_device, c, idx)
    # workspace head: kernel tables hk, then images, [B][S][2][n] fp32 each
    per = c.B * c.S * 2 * c.n
    hk = ws[:4 * per].view(np.float32).reshape(c.B, c.S, 2, c.n)
    assert np.isfinite(hk).all(), "NaN / inf in a kernel table"
    dl = C.case_deltas(c)
    for b, s, mic in np.ndindex(c.B, c.S, 2):
        if C.is_int_delay(dl[b, s, mic]):
            # a copy: the FFT-path tolerance, and the table is the shift itself
            assert np.array_equal(hk[b, s, mic], C.periodic_kernel(c.n, dl[b, s, mic]))
    copies = [b for b in range(c.B) if all(C.is_int_delay(v) for v in dl[b].ravel())]
    for b in copies:
        assert all(np.array_equal(ref["tol_" + k][b], C.fft_tol(ref[k][b])) for k in KEYS)
    if c.name.endswith(("-int", "-zero")) and "near" not in c.name:
        assert copies


# ----------------------------------------------------------------------------- D. mixing edges
@pytest.mark.parametrize("idx", range(len(C.EDGE_CASES)), ids=lambda i: C.EDGE_CASES[i].name)
def test_mixing_edges(gpu_device, idx):
    c = C.EDGE_CASES[idx]
    got, _, ref = _check_mix_case(gpu_device, c, idx)
    if 0 in c.zero:                                          # a silent target: exact zeros
        assert not any(got[k].any() for k in KEYS)
    if c.S == 1 or set(c.zero) >= set(range(1, c.S)):        # no interference: g = 1, itf = 0
        assert not got["itf"].any() and np.all(ref["g"] == 1.0)
    if "sir" in c.name:
        # the gain moves the mic-1 SIR to sir_db
        sir = 10 * np.log10(np.sum(got["tgt"].astype(np.float64) ** 2, axis=-1)
                            / np.sum(got["itf"].astype(np.float64) ** 2, axis=-1))
        assert np.all(np.abs(sir - c.sir) <= 1e-4), sir


# ----------------------------------------------------------------------------- C. generator
def _draws_from_ws(ws, B, S, n):
    """Sources, noise and angles from the head of a generator workspace. gen_front lays out
    sources [B][S][n] fp32, noise [B][2][n] fp32 and angles [B][S] fp64, each padded to 256 B,
    and the back ends write only behind the generation scratch (csrc/avz_scene.hip)."""
    o_src, o_noise, o_ang = C.gen_layout(B, S, n)
    src = ws[o_src:o_src + 4 * B * S * n].view(np.float32).reshape(B, S, n)
    noise = ws[o_noise:o_noise + 4 * B * 2 * n].view(np.float32).reshape(B, 2, n)
    ang = ws[o_ang:o_ang + 8 * B * S].view(np.float64).reshape(B, S)
    return src, noise, ang


def _draw_fraction(got, ref):
    err, tol = np.abs(got.astype(np.float64) - ref), C.draw_tol(ref)
    assert not err[tol == 0].any()                           # an all-silent source: exact zeros
    return float(np.max(err / np.where(tol > 0, tol, 1.0)))


@pytest.mark.parametrize("idx", range(len(C.GEN_CASES)), ids=lambda i: C.GEN_CASES[i].name)
def test_generator_draws_and_outputs(gpu_device, idx):
    from avz._lib import check, lib
    c = C.GEN_CASES[idx]
    S = 1 + c.K
    bufs = _Bufs(gpu_device, c.B, c.n, lib.avz_scene_generate_workspace_bytes(c.B, c.K, c.n),
                 bool(idx & 1))
    check(lib.avz_scene_generate(c.B, c.start, c.K, c.n, c.seed, c.mic_d, C.C_SOUND, c.fs, 0.0, 5.0,
                                 *bufs.out_args()), "avz_scene_generate")
    got, ws = bufs.results()
    src, noise, ang = _draws_from_ws(ws, c.B, S, c.n)
    r_ang, r_src, r_noise = C.gen_reference(c.name)
    assert np.array_equal(ang, r_ang)                        # bit-equal azimuths
    f_draw = max(_draw_fraction(src, r_src), _draw_fraction(noise, r_noise))
    # silent keep blocks are exact zeros on both sides
    assert np.array_equal(src == 0.0, r_src == 0.0)
    # the back end on the device's own draws
    ref = C.mix_reference(ang, src, noise, c.mic_d, C.C_SOUND, c.fs, 0.0, 5.0)
    f_out = _fraction(got, ref)
    print(f"{c.name}: draws {f_draw:.3f}, outputs {f_out:.3f} of their tolerances")
    assert f_draw <= 1.0, f_draw
    assert f_out <= 1.0, f_out


@pytest.mark.parametrize("n", C.REVERB_GEN["lengths"])
def test_generator_draws_at_odd_lengths(gpu_device, n):
    """Odd n reaches the front end's m + q < n and 2 i + 1 < n branches only through
    avz_scene_reverb_generate, which runs the same gen_front on the head of its workspace."""
    from avz import synth
    from avz._lib import check, lib
    g = C.REVERB_GEN
    room = synth.Room(**room_cases.ROOM_B, absorption=0.3, max_order=3)
    r = synth._room_struct(room)
    B, K = g["B"], g["K"]
    bufs = _Bufs(gpu_device, B, n,
                 lib.avz_scene_reverb_generate_workspace_bytes(ct.byref(r), B, K, n), True)
    D3 = ct.c_double * 3
    check(lib.avz_scene_reverb_generate(ct.byref(r), B, g["start"], K, n, g["seed"],
                                        D3(*g["target_pos"]), D3(*g["interferer_pos"]), 0.0, 5.0,
                                        *bufs.out_args()), "avz_scene_reverb_generate")
    _, ws = bufs.results()
    src, noise, _ = _draws_from_ws(ws, B, 1 + K, n)
    worst = 0.0
    for b in range(B):
        key = synth._key(g["start"] + b, g["seed"])
        for s in range(1 + K):
            worst = max(worst, _draw_fraction(src[b, s], synth.speech_like_philox(key, s, n, room.fs)))
        for mic in range(2):
            worst = max(worst, _draw_fraction(
                noise[b, mic], synth.philox_normals(key, synth.STREAM_NOISE + mic, n)))
    print(f"reverb generator n={n}: draws {worst:.3f} of their tolerance")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("silent", [(0,), (1, 2)], ids=["target", "interferers"])
def test_reverb_mix_keeps_silent_sources_exactly_zero(gpu_device, silent):
    """avz_scene_reverb_mix packs its sources like the FFT path of A: an all-zero target gives
    all-zero outputs, all-zero interferers an all-zero interference reference (p_i = 0, g = 1,
    synth._mix_images), not the 1e-16 the split of a packed transform leaves behind."""
    from avz import synth
    from avz._lib import check, lib
    room = synth.Room(**room_cases.ROOM_B, absorption=0.3, max_order=3)
    r = synth._room_struct(room)
    B, S, n = 2, 3, 255
    rng = np.random.default_rng(5)
    srcs = (0.5 * rng.standard_normal((B, S, n))).astype(np.float32)
    srcs[:, list(silent)] = 0.0
    noise = rng.standard_normal((B, 2, n)).astype(np.float32)
    pos = np.asarray(room_cases.BY_NAME["b-small-N3"].pos, np.float64)[:B]
    d_src, d_noise, d_pos = _dev(srcs, gpu_device), _dev(noise, gpu_device), _dev(pos, gpu_device)
    bufs = _Bufs(gpu_device, B, n, lib.avz_scene_reverb_workspace_bytes(ct.byref(r), B, S, n), True)
    p = lambda t: ct.c_void_p(t.data_ptr())  # noqa: E731
    check(lib.avz_scene_reverb_mix(ct.byref(r), B, S, n, p(d_src), p(d_pos), p(d_noise), 0.0, 5.0,
                                   *bufs.out_args()), "avz_scene_reverb_mix")
    got, _ = bufs.results()
    if 0 in silent:
        assert not any(got[k].any() for k in KEYS)
    else:
        assert not got["itf"].any() and got["tgt"].any()
        hm, ht, _ = (np.stack(v) for v in zip(*[synth.reverb_mix_draws(
            pos[b], srcs[b].astype(np.float64), noise[b].astype(np.float64), room)
            for b in range(B)]))
        assert max(np.abs(got["mix"] - hm).max(), np.abs(got["tgt"] - ht).max()) <= C.PROJECT_TOL
