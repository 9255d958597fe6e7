#!/usr/bin/env python3
"""Time avz_stoi_batch: ms per call from HIP events, after warm-up, as the median of --calls
calls (>= 20), next to the host restatement's time for pairs of the same batch
(DESIGN.md section 11). The pairs are the device generator's scenes: target reference
against mixture channel 0.

  python tools/stoi_bench.py                 # B = 256, 4 s, fs 16000
  python tools/stoi_bench.py --batch 64 --seconds 2 --host-pairs 4
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-audio-visual-zooming_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-pairs", type=int, default=8,
                    help="pairs of the batch the host restatement is timed on")
    a = ap.parse_args(argv)
    if a.calls < 20:
        ap.error("--calls must be at least 20")

    import numpy as np
    import torch
    from avz import stoi, synth
    dev = torch.device("cuda:0")
    n = int(round(a.seconds * synth.FS))
    mix, tgt, _ = synth.make_batch_device(a.batch, start=0, n_samples=n, n_interferers=2,
                                          device=dev, rng="philox")
    est = mix[:, 0, :]
    ws = torch.empty(stoi.workspace_bytes(a.batch, n, synth.FS), dtype=torch.uint8, device=dev)
    for _ in range(a.warmup):
        d, info = stoi.stoi_batch(tgt, est, fs=synth.FS, workspace=ws)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        d, info = stoi.stoi_batch(tgt, est, fs=synth.FS, workspace=ws)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    med = 0.5 * (ms[(len(ms) - 1) // 2] + ms[len(ms) // 2])
    k = max(1, min(a.host_pairs, a.batch))
    x, y = tgt[:k].cpu().numpy(), est[:k].cpu().numpy()
    t0 = time.perf_counter()
    ref = np.array([stoi.stoi_numpy(x[b], y[b], synth.FS) for b in range(k)])
    host_ms = (time.perf_counter() - t0) * 1e3 / k
    dd = d.cpu().numpy()
    print(json.dumps({
        "batch": a.batch, "samples": n, "fs": synth.FS, "calls": a.calls,
        "ms_median": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
        "us_per_pair": round(med * 1e3 / a.batch, 3),
        "host_ms_per_pair": round(host_ms, 2), "host_pairs": k,
        "host_ms_batch_extrapolated": round(host_ms * a.batch, 1),
        "max_abs_diff_host_pairs": float(np.abs(dd[:k] - ref).max()),
        "mean_stoi": float(dd.mean()), "status_nonzero": int((info[:, 0] != 0).sum().item()),
        "workspace_bytes": ws.numel(),
    }))


if __name__ == "__main__":
    main()
