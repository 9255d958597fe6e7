#!/usr/bin/env python3
"""Time the reverberant scene generator: ms per call from HIP events, after warm-up, as the
median of --calls calls (>= 20), for avz_room_rir and avz_scene_reverb_generate (one call on
the whole batch, workspace allocated once) at each --orders, next to the anechoic
avz_scene_generate at the same batch.

  python tools/reverb_scene_bench.py                 # B = 256, 4 s, 3 interferers, N = 10, 15
  python tools/reverb_scene_bench.py --batch 64 --seconds 2 --host
--host also times the numpy restatement (synth.make_reverb_scene_philox) on one scene.
Prints one JSON line per measurement."""
import argparse
import ctypes as ct
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-audio-visual-zooming_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, warmup, calls):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"ms_median": round(0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2]), 4),
            "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4), "calls": calls}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--orders", type=int, nargs="*", default=[10, 15])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--interferers", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args(argv)
    if a.calls < 20:
        ap.error("--calls must be at least 20")

    import numpy as np
    import torch
    from avz import engine, synth
    from avz._lib import check, lib
    dev = torch.device("cuda:0")
    B, K, n = a.batch, a.interferers, int(a.seconds * synth.FS)
    S = 1 + K
    mix = torch.empty((B, 2, n), dtype=torch.float32, device=dev)
    tgt = torch.empty((B, n), dtype=torch.float32, device=dev)
    itf = torch.empty((B, n), dtype=torch.float32, device=dev)
    p = lambda t: ct.c_void_p(t.data_ptr())  # noqa: E731
    D3 = ct.c_double * 3
    tp, ip = D3(*synth.SOURCE_TARGET_POS), D3(*synth.SOURCE_INTERF_POS)
    shape = {"batch": B, "samples": n, "interferers": K}

    ws_bytes = lib.avz_scene_generate_workspace_bytes(B, K, n)
    ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.float32, device=dev)
    r = timed(lambda: check(lib.avz_scene_generate(
        B, 0, K, n, 0, synth.MIC_D, synth.C_SOUND, float(synth.FS), 0.0, 5.0, p(mix),
        mix.stride(0), mix.stride(1), p(tgt), p(itf), tgt.stride(0), p(ws), ws_bytes, None),
        "avz_scene_generate"), a.warmup, a.calls)
    print(json.dumps({"what": "avz_scene_generate (anechoic)", **shape, **r,
                      "workspace_bytes": ws_bytes}))
    del ws

    for order in a.orders:
        room = synth.Room(max_order=order)
        rs = synth._room_struct(room)
        pos = torch.from_numpy(np.stack([synth.room_positions_philox(synth._key(b), K, room)
                                         for b in range(B)])).to(dev)
        out = torch.empty((B, S, 2, room.rir_len), dtype=torch.float64, device=dev)
        r = timed(lambda: engine.room_rir(room, pos, out=out), a.warmup, a.calls)
        print(json.dumps({"what": "avz_room_rir", "max_order": order, "batch": B, "sources": S,
                          "rirs": B * S * 2, "images": len(synth.room_images(order)),
                          "rir_len": room.rir_len, **r}))
        ws_bytes = lib.avz_scene_reverb_generate_workspace_bytes(ct.byref(rs), B, K, n)
        ws = torch.empty(ws_bytes // 4 + 1, dtype=torch.float32, device=dev)
        r = timed(lambda: check(lib.avz_scene_reverb_generate(
            ct.byref(rs), B, 0, K, n, 0, tp, ip, 0.0, 5.0, p(mix), mix.stride(0), mix.stride(1),
            p(tgt), p(itf), tgt.stride(0), p(ws), ws_bytes, None), "avz_scene_reverb_generate"),
            a.warmup, a.calls)
        print(json.dumps({"what": "avz_scene_reverb_generate", "max_order": order, **shape, **r,
                          "workspace_bytes": ws_bytes,
                          "workspace_bytes_per_utterance": ws_bytes // B}))
        del ws, out
        if a.host:
            t0 = time.perf_counter()
            synth.make_reverb_scene_philox(0, n, K, room)
            print(json.dumps({"what": "numpy restatement, one scene", "max_order": order,
                              "samples": n, "interferers": K,
                              "s": round(time.perf_counter() - t0, 3)}))


if __name__ == "__main__":
    main()
