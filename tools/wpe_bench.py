#!/usr/bin/env python3
"""Time avz_wpe_spectral: ms per call from HIP events, after warm-up, as the median of
--calls calls (>= 20), and the fraction of the MI355X fp64 vector peak it implies with
flops = iterations * B * F * T * 8 * (KD (KD + 1) / 2 + 2 KD D), D = 2.

  python tools/wpe_bench.py                 # B = 256, 4 s: 512/256 and 1024/512
  python tools/wpe_bench.py --n-fft 512 --batch 64 --seconds 2
Prints one JSON line per shape."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-audio-visual-zooming_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# MI355X fp64 vector peak: half the 157.3 TFLOPS fp32 vector rate (public datasheet value)
FP64_VECTOR_PEAK = 78.6e12


def wpe_flops(B, F, T, taps, iterations, D=2):
    kd = taps * D
    return iterations * B * F * T * 8 * (kd * (kd + 1) // 2 + 2 * kd * D)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--n-fft", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--taps", type=int, default=10)
    ap.add_argument("--delay", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args(argv)
    if a.calls < 20:
        ap.error("--calls must be at least 20")

    import torch
    from avz import engine
    dev = torch.device("cuda:0")
    for n in a.n_fft:
        hop, F = n // 2, n // 2 + 1
        T = engine.n_frames(int(a.seconds * 16000), hop)
        g = torch.Generator(device=dev).manual_seed(n)
        # complex Gaussian frames under a slowly varying level, so that lambda varies
        lvl = 10.0 ** (torch.rand((a.batch, 1, F, T), generator=g, device=dev) * 2 - 2)
        Y = torch.view_as_complex(torch.randn((a.batch, 2, F, T, 2), generator=g, device=dev)) * lvl
        Z = torch.empty_like(Y)
        st = torch.empty((a.batch, F), dtype=torch.int32, device=dev)
        for _ in range(a.warmup):
            engine.wpe_spectral(Y, a.taps, a.delay, a.iters, out=Z, status=st)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            engine.wpe_spectral(Y, a.taps, a.delay, a.iters, out=Z, status=st)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        med = 0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2])
        flops = wpe_flops(a.batch, F, T, a.taps, a.iters)
        print(json.dumps({
            "n_fft": n, "batch": a.batch, "bins": F, "frames": T, "taps": a.taps,
            "delay": a.delay, "iterations": a.iters, "calls": a.calls,
            "ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
            "gflops": round(flops / med / 1e6, 1),
            "fp64_vector_peak_fraction": round(flops / (med * 1e-3) / FP64_VECTOR_PEAK, 4),
            "bytes_compulsory": 2 * Y.numel() * 8,
            "status_nonzero": int((st != 0).sum().item()),
        }))


if __name__ == "__main__":
    main()
