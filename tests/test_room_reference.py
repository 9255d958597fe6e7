"""The shoebox-room model's host restatement (avz/synth.py room_rir and friends) and the
host-side validation of the room entry points; no GPU. The image-source model is the
contract: pyroomacoustics is not installed, so no run of it is pinned."""
import ctypes as ct

import numpy as np
import pytest

import room_cases as R
from avz import synth


@pytest.mark.parametrize("order", [0, 1, 2, 10, 15])
def test_image_count_and_order(order):
    q = synth.room_images(order)
    assert len(q) == (2 * order + 1) * (2 * order * order + 2 * order + 3) // 3
    assert len(set(map(tuple, q))) == len(q)
    assert np.abs(q).sum(axis=1).max() == order
    assert [tuple(r) for r in q] == sorted(tuple(r) for r in q)   # qx, then qy, then qz


def test_inverse_sabine_of_the_reference_room():
    assert abs(synth.inverse_sabine(0.5, [4.9] * 3, 343.0) - 0.263153) <= 1e-6
    assert synth.Room().absorption == synth.inverse_sabine(synth.RT60_TARGET, synth.ROOM_DIM)
    assert synth.ROOM_DIM == [4.9, 4.9, 4.9] and synth.MIC_LOCS[1][0] - synth.MIC_LOCS[0][0] \
        == pytest.approx(0.08)


def test_order_zero_is_one_windowed_sinc():
    room = synth.Room(absorption=1.0, max_order=0)
    src, mic = np.array(synth.SOURCE_TARGET_POS), np.array(room.mic[0])
    h = synth.room_rir(room.dim, src, mic, 1.0, 0)
    d = np.sqrt(((src - mic) ** 2).sum())
    tau = d * room.fs / room.c
    n = np.arange(len(h))
    x = n - tau
    ref = np.where(np.abs(x) <= 40.5, 0.5 * (1 + np.cos(2 * np.pi * x / 81)), 0.0) * np.sinc(x)
    ref[(n < np.floor(tau) - 40) | (n > np.floor(tau) + 40)] = 0.0
    ref /= 4 * np.pi * d
    assert np.count_nonzero(h) in (80, 81)
    assert np.abs(h - ref).max() <= 1e-13 / (4 * np.pi * d)    # np.sinc rounds pi x


def test_reciprocity():
    room = synth.Room(dim=R.ROOM_B["dim"], absorption=0.3, max_order=6)
    a, b = [0.4, 0.7, 1.9], [2.1, 1.3, 0.6]
    # In long double: in fp64 the swap rounds the image distances differently, and one ulp of
    # a delay of 64..128 samples already moves a tap by 64 2^-52 of its amplitude (measured
    # in fp64 here: 118 2^-52 max|h|; in long double 5e-4 2^-52 max|h|).
    ld = np.longdouble
    h = synth.room_rir(room.dim, a, b, room.absorption, room.max_order, dtype=ld)
    g = synth.room_rir(room.dim, b, a, room.absorption, room.max_order, dtype=ld)
    assert np.abs(h).max() > 0.01
    assert np.abs(h - g).max() <= 64 * 2.0 ** -52 * np.abs(h).max()
    # fp64: the swapped RIR is the same function within the restatement's own error
    h64 = synth.room_rir(room.dim, a, b, room.absorption, room.max_order)
    g64 = synth.room_rir(room.dim, b, a, room.absorption, room.max_order)
    e = np.abs(h64 - h).max() + np.abs(g64 - g).max()
    assert np.abs(h64 - g64).max() <= 64 * 2.0 ** -52 * np.abs(h64).max() + float(e)


@pytest.mark.parametrize("dim,order,want", [([4.9] * 3, 15, 3713), ([4.9] * 3, 10, 2576),
                                            ([3.0, 2.5, 2.2], 3, 622), ([8.0, 6.0, 3.0], 20, None)])
def test_rir_len_bounds_the_last_tap(dim, order, want):
    L = synth.room_rir_len(dim, order)
    assert want is None or L == want
    # a source and a mic in opposite corners: the farthest images there are
    eps = 1e-3
    src, mic = [eps] * 3, [v - eps for v in dim]
    q = synth.room_images(order)
    img = np.where(q % 2 == 1, (q + 1) * np.array(dim) - src, q * np.array(dim) + src)
    tau = np.sqrt(((img - np.array(mic)) ** 2).sum(axis=1)).max() * synth.FS / synth.C_SOUND
    assert np.floor(tau) + 40 < L
    if order <= 3:      # and nothing is dropped at the end: a longer RIR holds the same taps
        h = synth.room_rir(dim, src, mic, 0.3, order)
        h2 = synth.room_rir(dim, src, mic, 0.3, order, rir_len=L + 200)
        assert np.array_equal(h2[:L], h) and not h2[L:].any()


def test_taps_are_continuous_across_an_integer_delay():
    for t0 in (57.0, 3000.0):
        lo = synth.frac_delay_taps(t0 - 1e-9)
        hi = synth.frac_delay_taps(t0 + 1e-9)
        a = dict(zip(lo[0][0], lo[1][0]))
        b = dict(zip(hi[0][0], hi[1][0]))
        assert min(a) == t0 - 41 and min(b) == t0 - 40         # floor went the other way
        worst = max(abs(a.get(n, 0.0) - b.get(n, 0.0)) for n in set(a) | set(b))
        assert worst <= 1e-8
    # on the integer itself the one non-zero tap is the amplitude
    n, v = synth.frac_delay_taps(57.0, 0.25)
    assert v[0][n[0] == 57] == 0.25 and np.count_nonzero(v) == 1


def test_philox_positions():
    room = synth.Room(dim=[5.0, 4.0, 3.0])
    for idx, seed in ((0, 0), (2 ** 33 + 5, 3)):
        key = synth._key(idx, seed)
        pos = synth.room_positions_philox(key, 6, room)
        assert pos.shape == (7, 3)
        assert list(pos[0]) == synth.SOURCE_TARGET_POS and list(pos[1]) == synth.SOURCE_INTERF_POS
        for s in range(2, 7):
            u0, u1 = synth.philox_uniform(key, [0x2000 + 2 * (s - 2), 0x2000 + 2 * (s - 2) + 1])
            assert pos[s, 0] == 1.0 + u0 * 3.0 and pos[s, 1] == 1.0 + u1 * 2.0
            assert pos[s, 2] == synth.SOURCE_TARGET_POS[2]
        assert np.all(pos[2:, :2] >= 1.0) and np.all(pos[2:, :2] <= np.array(room.dim[:2]) - 1.0)
    assert synth.UNIF_POS == 0x2000
    # the draws are those of the anechoic scene, positions aside
    p, s, z = synth.reverb_scene_draws_philox(9, 2000, 3, synth.Room(max_order=1))
    _, s0, z0 = synth.scene_draws_philox(9, 2000, 3)
    assert np.array_equal(s, s0) and np.array_equal(z, z0) and p.shape == (4, 3)


def test_reverb_mix_follows_the_scene_conventions():
    room = synth.Room(**R.ROOM_B, absorption=0.3, max_order=2)
    pos, srcs, z = synth.reverb_scene_draws_philox(3, 3001, 2, room,
                                                   target_pos=[0.5, 2.0, 1.0],
                                                   interferer_pos=[2.5, 0.4, 1.5])
    mix, tgt, itf = synth.reverb_mix_draws(pos, srcs, z, room, sir_db=3.0)
    assert mix.shape == (2, 3001) and abs(np.abs(mix).max() - 1.0) <= 1e-6
    p = lambda v: np.mean(v.astype(np.float64) ** 2)  # noqa: E731
    assert abs(10 * np.log10(p(tgt) / p(itf)) - 3.0) <= 1e-3
    from scipy.signal import fftconvolve
    h = synth.room_rirs(room, pos)
    img = fftconvolve(srcs[0], h[0, 0])[:3001]
    assert np.abs(tgt / np.abs(tgt).max() - img / np.abs(img).max()).max() <= 1e-6


# ---------------------------------------------------------------- C ABI, host-side checks
def _room(**kw):
    from avz import _lib
    kw.setdefault("absorption", 0.263153)
    r = synth._room_struct(synth.Room(**{k: v for k, v in kw.items() if k in
                                         ("dim", "absorption", "max_order", "mic", "c", "fs")}))
    return r, _lib


def test_rir_len_through_the_abi():
    r, L = _room()
    assert L.lib.avz_room_rir_len(ct.byref(r)) == 3713
    r, L = _room(max_order=10)
    assert L.lib.avz_room_rir_len(ct.byref(r)) == 2576
    c = R.BY_NAME["d-large-N20"].room
    assert L.lib.avz_room_rir_len(ct.byref(synth._room_struct(c))) == c.rir_len <= 8192
    assert L.lib.avz_room_rir_len(None) == L.AVZ_ERR_ARG
    assert L.lib.avz_version() == 3


BAD_ROOMS = [
    ("dim zero", dict(dim=[4.9, 0.0, 4.9]), -1), ("dim nan", dict(dim=[4.9, float("nan"), 4.9]), -1),
    ("dim inf", dict(dim=[float("inf"), 4.9, 4.9]), -1), ("dim negative", dict(dim=[4.9, 4.9, -1.0]), -1),
    ("fs zero", dict(fs=0.0), -1), ("fs nan", dict(fs=float("nan")), -1),
    ("c negative", dict(c=-343.0), -1), ("c inf", dict(c=float("inf")), -1),
    ("absorption zero", dict(absorption=0.0), -1), ("absorption above one", dict(absorption=1.01), -1),
    ("absorption nan", dict(absorption=float("nan")), -1),
    ("order negative", dict(max_order=-1), -1), ("order 21", dict(max_order=21), -1),
    ("mic outside", dict(mic=[[2.41, 2.45, 1.5], [5.0, 2.45, 1.5]]), -1),
    ("mic below", dict(mic=[[2.41, -0.1, 1.5], [2.49, 2.45, 1.5]]), -1),
    ("mic nan", dict(mic=[[2.41, 2.45, float("nan")], [2.49, 2.45, 1.5]]), -1),
    ("rir too long", dict(dim=[9.0, 6.0, 3.0], max_order=20), -2),
    ("rir too long at 48 kHz", dict(fs=48000.0, max_order=15), -2),
]


@pytest.mark.parametrize("what,kw,code", BAD_ROOMS, ids=[b[0] for b in BAD_ROOMS])
def test_invalid_rooms_are_rejected_on_the_host(what, kw, code):
    """Every entry point returns the room's code with null device pointers: the validation
    runs before any device work."""
    r, L = _room(**kw)
    lib, rp = L.lib, ct.byref(r)
    assert code in (L.AVZ_ERR_ARG, L.AVZ_ERR_SHAPE)
    D3 = ct.c_double * 3
    t, i = D3(*synth.SOURCE_TARGET_POS), D3(*synth.SOURCE_INTERF_POS)
    assert lib.avz_room_rir_len(rp) == code
    assert lib.avz_room_rir(rp, 1, 1, None, None, None) == code
    assert lib.avz_scene_reverb_mix(rp, 1, 2, 4000, None, None, None, 0.0, 5.0, None, 0, 0, None,
                                    None, 0, None, 0, None) == code
    assert lib.avz_scene_reverb_generate(rp, 1, 0, 1, 4000, 0, t, i, 0.0, 5.0, None, 0, 0, None,
                                         None, 0, None, 0, None) == code
    assert lib.avz_scene_reverb_workspace_bytes(rp, 1, 2, 4000) == 0
    assert lib.avz_scene_reverb_generate_workspace_bytes(rp, 1, 1, 4000) == 0


def test_null_pointers_small_rooms_and_workspace():
    r, L = _room(max_order=3)
    lib, rp = L.lib, ct.byref(r)
    D3 = ct.c_double * 3
    t, i = D3(*synth.SOURCE_TARGET_POS), D3(*synth.SOURCE_INTERF_POS)
    fake = ct.c_void_p(256)      # never dereferenced: every call below fails its validation
    mix = lambda room, *p, ws=0: lib.avz_scene_reverb_mix(  # noqa: E731
        room, 1, 2, 4000, p[0], p[1], p[2], 0.0, 5.0, p[3], 8000, 4000, p[4], p[5], 4000, p[6], ws,
        None)
    gen = lambda room, k, tp, ip, *p, ws=0: lib.avz_scene_reverb_generate(  # noqa: E731
        room, 1, 0, k, 4000, 0, tp, ip, 0.0, 5.0, p[0], 8000, 4000, p[1], p[2], 4000, p[3], ws, None)
    # null pointers
    assert lib.avz_room_rir(rp, 1, 1, None, fake, None) == L.AVZ_ERR_ARG
    assert lib.avz_room_rir(rp, 1, 1, fake, None, None) == L.AVZ_ERR_ARG
    assert lib.avz_room_rir(None, 1, 1, fake, fake, None) == L.AVZ_ERR_ARG
    for hole in range(7):
        p = [fake] * 7
        p[hole] = None
        assert mix(rp, *p, ws=1 << 40) == L.AVZ_ERR_ARG, hole
    assert mix(None, *[fake] * 7, ws=1 << 40) == L.AVZ_ERR_ARG
    for hole in range(4):
        p = [fake] * 4
        p[hole] = None
        assert gen(rp, 1, t, i, *p, ws=1 << 40) == L.AVZ_ERR_ARG, hole
    assert gen(rp, 1, None, i, *[fake] * 4, ws=1 << 40) == L.AVZ_ERR_ARG
    assert gen(rp, 1, t, None, *[fake] * 4, ws=1 << 40) == L.AVZ_ERR_ARG
    assert gen(None, 1, t, i, *[fake] * 4, ws=1 << 40) == L.AVZ_ERR_ARG
    # a workspace one byte short
    need = lib.avz_scene_reverb_workspace_bytes(rp, 1, 2, 4000)
    Lc = 4000 + synth.Room(max_order=3).rir_len - 1
    assert need >= 2 * 3 * Lc * 16
    assert mix(rp, *[fake] * 7, ws=need - 1) == L.AVZ_ERR_SHAPE
    gneed = lib.avz_scene_reverb_generate_workspace_bytes(rp, 1, 1, 4000)
    assert gneed > need
    assert gen(rp, 1, t, i, *[fake] * 4, ws=gneed - 1) == L.AVZ_ERR_SHAPE
    # more than one interferer needs room for the [1, dim - 1] draws
    small, _ = _room(dim=[2.0, 4.0, 3.0], mic=[[0.9, 2.0, 1.5], [1.0, 2.0, 1.5]], max_order=3)
    ts, is_ = D3(1.0, 3.0, 1.5), D3(1.5, 1.0, 1.5)
    assert gen(ct.byref(small), 2, ts, is_, *[None] * 4) == L.AVZ_ERR_ARG
    assert gen(ct.byref(small), 1, ts, is_, *[fake] * 4, ws=0) == L.AVZ_ERR_SHAPE  # one is fine
    small, _ = _room(dim=[4.0, 1.9, 3.0], mic=[[2.0, 0.9, 1.5], [2.0, 1.0, 1.5]], max_order=3)
    assert gen(ct.byref(small), 2, D3(1.0, 1.0, 1.5), D3(3.0, 1.5, 1.5), *[None] * 4) == L.AVZ_ERR_ARG
    assert gen(ct.byref(small), 1, D3(1.0, 1.0, 1.5), D3(3.0, 1.5, 1.5), *[fake] * 4) == L.AVZ_ERR_SHAPE
    # n < 2 is a shape error; odd n is accepted (it reaches the workspace check)
    assert lib.avz_scene_reverb_mix(rp, 1, 2, 1, fake, fake, fake, 0.0, 5.0, fake, 2, 1, fake, fake,
                                    1, fake, 1 << 40, None) == L.AVZ_ERR_SHAPE
    assert lib.avz_scene_reverb_mix(rp, 1, 2, 4001, fake, fake, fake, 0.0, 5.0, fake, 8002, 4001,
                                    fake, fake, 4001, fake, 0, None) == L.AVZ_ERR_SHAPE
    assert lib.avz_scene_reverb_workspace_bytes(rp, 1, 2, 4001) > 0
