#!/usr/bin/env python3
"""Measure the training path. HIP events, --warmup warm-ups, median
of --calls calls (>= 20). One JSON line per mode.

  python tools/train_bench.py kernel            # B = 256, 2 s: avz_mask_training_batch against
                                                # avz_mask_features + 2 x avz_stft + torch
                                                # abs / gt / float, interleaved in one run
  python tools/train_bench.py step              # B = 32: scene + batch + forward / backward /
                                                # Adam, and the share spent making the data
  python tools/train_bench.py run --wall 240    # train for at most --wall seconds, then score
                                                # the initial and the trained weights held out
"""
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


def _stats(ms):
    ms = sorted(ms)
    med = 0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2])
    return {"median": round(med, 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernel(a):
    import torch
    from avz import _lib, train
    from avz.engine import n_frames
    lib = _lib.lib
    dev = torch.device("cuda:0")
    n = int(round(a.seconds * 16000))
    B = a.batch
    plan = train.make_plan(B, n)
    mix, tgt, itf = train.scenes(B, 0, n, device=dev)
    F, T = plan.F, n_frames(n, plan.hop)
    lens = torch.full((B,), n, dtype=torch.int32, device=dev)
    feat = torch.zeros((B, 2, F, T), dtype=torch.float32, device=dev)
    feat_c = torch.zeros_like(feat)
    label = torch.zeros((B, F, T), dtype=torch.float32, device=dev)
    spec = torch.zeros((2, B, 1, F, T), dtype=torch.complex64, device=dev)
    p = lambda t: ct.c_void_p(t.data_ptr())  # noqa: E731
    st = ct.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fused():
        rc = lib.avz_mask_training_batch(plan._h, _lib.FEAT_LOGMAG_IPD, B, p(lens), n, p(mix),
                                         mix.stride(0), mix.stride(1), p(tgt), p(itf),
                                         tgt.stride(0), p(feat), *feat.stride(), p(label),
                                         *label.stride(), st)
        assert rc == 0, rc

    out = {}

    def composed():
        rc = lib.avz_mask_features(plan._h, _lib.FEAT_LOGMAG_IPD, B, p(lens), n, p(mix),
                                   mix.stride(0), mix.stride(1), p(feat_c), *feat_c.stride(), st)
        assert rc == 0, rc
        for r, x in enumerate((tgt, itf)):
            Y = spec[r]
            rc = lib.avz_stft(plan._h, B, 1, p(lens), n, p(x), x.stride(0), x.stride(0), p(Y),
                              Y.stride(0), Y.stride(1), Y.stride(2), st)
            assert rc == 0, rc
        out["label"] = (spec[0, :, 0].abs() > spec[1, :, 0].abs()).float()

    for _ in range(a.warmup):
        fused()
        composed()
    torch.cuda.synchronize()
    ms_f, ms_c = [], []
    for _ in range(a.calls):  # interleaved: both see the same clocks
        ms_f.append(_timed(fused))
        ms_c.append(_timed(composed))
    wave, cell = B * n * 4, B * F * T
    res = {
        "mode": "kernel", "batch": B, "samples": n, "n_fft": 1024, "calls": a.calls,
        "fused_ms": _stats(ms_f), "composed_ms": _stats(ms_c),
        # fused: 4 waveforms in; features (2 floats) and label (1 float) out
        "fused_bytes": 4 * wave + cell * 12,
        # composed: features (2 waveforms in, 2 floats out); 2 x STFT (1 waveform in, 8 B out);
        # 2 x abs (8 in, 4 out); gt (8 in, 1 out); float (1 in, 4 out)
        "composed_bytes": 4 * wave + cell * (8 + 2 * 8 + 2 * 12 + 9 + 5),
        "features_equal": bool(torch.equal(feat, feat_c)),
        "labels_differing": int((label != out["label"]).sum()), "cells": cell,
    }
    print(json.dumps(res))


def step(a):
    import torch
    import torch.nn as nn
    from avz import neural, train
    from avz.engine import mask_training_batch
    dev = torch.device("cuda:0")
    n = int(round(a.seconds * 16000))
    B = a.batch
    plan = train.make_plan(B, n)
    torch.manual_seed(0)
    model = neural.FreqPreservingUNet().to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=train.REF_LR)
    crit = nn.BCELoss()
    state = {"i": 0}

    def data():
        mix, tgt, itf = train.scenes(B, state["i"] * B, n, device=dev)
        state["i"] += 1
        state["xy"] = mask_training_batch(plan, mix, tgt, itf, "unet")

    def full():
        data()
        x, y = state["xy"]
        opt.zero_grad()
        loss = crit(model(x), y)
        loss.backward()
        opt.step()

    for _ in range(a.warmup):
        full()
    torch.cuda.synchronize()
    ms_d, ms_s = [], []
    for _ in range(a.calls):
        ms_d.append(_timed(data))
        ms_s.append(_timed(full))
    d, s = _stats(ms_d), _stats(ms_s)
    print(json.dumps({"mode": "step", "batch": B, "samples": n, "calls": a.calls,
                      "data_ms": d, "step_ms": s,
                      "data_share": round(d["median"] / s["median"], 4),
                      "ref_run_steps": train.REF_STEPS,
                      "ref_run_minutes_at_this_rate": round(train.REF_STEPS * s["median"] / 6e4,
                                                            1)}))


def run(a):
    import numpy as np
    import torch
    from avz import neural, train
    torch.manual_seed(a.seed)
    model = neural.FreqPreservingUNet()
    before = train.evaluate(model, a.eval_scenes, seed=a.seed)
    t0 = time.perf_counter()
    model, losses = train.train(model, steps=a.max_steps, batch_size=a.batch, lr=a.lr,
                                seed=a.seed, max_seconds=a.wall)
    wall = time.perf_counter() - t0
    after = train.evaluate(model, a.eval_scenes, seed=a.seed)
    if a.out:
        torch.save(model.state_dict(), a.out)
    k = min(10, len(losses))
    print(json.dumps({"mode": "run", "batch": a.batch, "lr": a.lr, "steps": len(losses),
                      "train_wall_s": round(wall, 1),
                      "bce_first": round(float(np.mean(losses[:k])), 5),
                      "bce_last": round(float(np.mean(losses[-k:])), 5),
                      "held_out_initial": before, "held_out_trained": after}))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("mode", choices=("kernel", "step", "run"))
    ap.add_argument("--batch", type=int, default=None, help="default 256 (kernel), 32 (step, run)")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--wall", type=float, default=240.0, help="run: training seconds at most")
    ap.add_argument("--max-steps", type=int, default=4687, help="run: the reference's 50 epochs")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--eval-scenes", type=int, default=64)
    ap.add_argument("--out", default=None, help="run: save the trained state_dict here")
    a = ap.parse_args(argv)
    if a.calls < 20:
        ap.error("--calls must be at least 20")
    if a.batch is None:
        a.batch = 256 if a.mode == "kernel" else 32
    {"kernel": kernel, "step": step, "run": run}[a.mode](a)


if __name__ == "__main__":
    main()
