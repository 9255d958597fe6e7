"""Shoebox-room cases shared by tests/test_room_reference.py (CPU) and tests/test_gpu_room.py.

Each case is a room, a batch of source positions [B, S, 3] and, from avz/synth.room_rir, the
RIRs [B, S, 2, rir_len] in fp64 (h64) and in long double (hld). E_ref = |h64 - hld| per sample
is the fp64 restatement's own error (dominated by the rounding of the delay d fs / c of distant
images, which moves their windowed sincs). References are computed once per process."""
import functools
from collections import namedtuple

import numpy as np

from avz import synth

RoomCase = namedtuple("RoomCase", "name room pos")

ROOM_B = dict(dim=[3.0, 2.5, 2.2], mic=[[1.31, 1.17, 1.05], [1.39, 1.23, 1.10]])


def _cases():
    ref = synth.Room
    b = lambda **kw: synth.Room(**ROOM_B, **kw)  # noqa: E731
    return [
        # (a) one image: the windowed sinc itself
        RoomCase("a-ref-N0-a1", ref(absorption=1.0, max_order=0), [[synth.SOURCE_TARGET_POS]]),
        # (b) small asymmetric room, 63 images, rir_len 622, an odd source count, B = 3
        RoomCase("b-small-N3", b(absorption=0.3, max_order=3),
                 [[[0.4, 0.7, 1.9], [2.7, 2.2, 0.3], [1.0, 1.9, 1.2]],
                  [[2.1, 0.35, 0.6], [0.25, 2.3, 2.0], [1.6, 1.3, 1.7]],
                  [[2.9, 0.1, 0.1], [1.5, 0.2, 2.1], [0.7, 1.25, 0.45]]]),
        # (c) the reference room as simulation.py builds it: 4991 images, rir_len 3713
        RoomCase("c-ref-N15", ref(absorption=0.263, max_order=15),
                 [[synth.SOURCE_TARGET_POS, synth.SOURCE_INTERF_POS]]),
        # (d) the largest accepted order in a large room: 11521 images, a 63-KB RIR
        RoomCase("d-large-N20", synth.Room(dim=[8.0, 6.0, 3.0], absorption=0.15, max_order=20,
                                           mic=[[3.96, 3.1, 1.4], [4.04, 3.1, 1.4]]),
                 [[[6.3, 1.2, 1.7]]]),
        # (e) a source 0.3 m from mic 0: delay 14 samples, the taps below sample 0 are dropped
        RoomCase("e-small-near", b(absorption=0.3, max_order=3),
                 [[[1.31 + 0.2, 1.17 - 0.2, 1.05 + 0.1]]]),
    ]


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """{"h64", "hld" [B, S, 2, L], "E_ref" (max over samples), "hmax"} of case `name`."""
    c = BY_NAME[name]
    pos = np.asarray(c.pos, np.float64)
    B, S, _ = pos.shape
    out = {}
    for key, dt in (("h64", np.float64), ("hld", np.longdouble)):
        out[key] = np.stack([synth.room_rirs(c.room, pos[b], dtype=dt) for b in range(B)])
    out["E_ref"] = float(np.abs(out["h64"].astype(np.longdouble) - out["hld"]).max())
    out["hmax"] = float(np.abs(out["h64"]).max())
    for v in (out["h64"], out["hld"]):
        v.setflags(write=False)
    return out


# ---------------------------------------------------------------- mixing cases
MixCase = namedtuple("MixCase", "name room n K B")
MIX_CASES = [
    MixCase("small-n4000-K2", synth.Room(**ROOM_B, absorption=0.3, max_order=3), 4000, 2, 3),
    MixCase("small-n4001-odd", synth.Room(**ROOM_B, absorption=0.3, max_order=3), 4001, 2, 3),
    MixCase("ref-N10-n16000-K3", synth.Room(max_order=10), 16000, 3, 2),
    MixCase("small-n4000-K0", synth.Room(**ROOM_B, absorption=0.3, max_order=3), 4000, 0, 2),
]
MIX_BY_NAME = {c.name: c for c in MIX_CASES}


@functools.lru_cache(maxsize=None)
def mix_case(name):
    """Host draws of a mixing case (positions [B, S, 3], float32 sources [B, S, n], float32
    unit-normal noise [B, 2, n]) and reverb_mix_draws on them: (pos, srcs, noise, mix, tgt, itf)."""
    c = MIX_BY_NAME[name]
    rng = np.random.default_rng(77)
    S = 1 + c.K
    lo = np.array([0.2, 0.2, 0.2])
    hi = np.array(c.room.dim) - 0.2
    pos = lo + rng.random((c.B, S, 3)) * (hi - lo)
    srcs = np.stack([synth.scene_draws(40 + b, c.n, c.K)[1] for b in range(c.B)]).astype(np.float32)
    noise = rng.standard_normal((c.B, 2, c.n)).astype(np.float32)
    ref = [synth.reverb_mix_draws(pos[b], srcs[b].astype(np.float64),
                                  noise[b].astype(np.float64), c.room) for b in range(c.B)]
    mix, tgt, itf = (np.stack([r[i] for r in ref]) for i in range(3))
    return pos, srcs, noise, mix, tgt, itf
