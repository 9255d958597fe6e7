#!/usr/bin/env python3
"""Time the streaming blind delay mask (avz_delay_stream_push) on --streams
streams of the device generator's scenes (one interferer, SNR 20): one hop per call and eight
hops per call, N = 512 and 1024, d = 0.08 and 0.01 (103 and 506 band bins at N = 1024).

Each figure is the median (min - max) of --calls HIP-event times after --warmup calls; the
synchronous host-clock time of the same call (call + wait: what a real-time caller waits for)
is beside it, and the hop's own duration, which a push of one hop must stay below. For scale the
streaming beamformer's push of the same hops with that mask (avz_stream_push) is timed in the
same loop, alternating.

  python tools/delay_stream_bench.py
Prints one JSON line per (N, d, hops per call)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-audio-visual-zooming_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def stats(v):
    v = sorted(v)
    med = 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2])
    return {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--hist-bins", type=int, default=65)
    ap.add_argument("--forget", type=float, default=0.98)
    a = ap.parse_args(argv)

    import torch
    import avz
    from avz import delay_mask as DM
    from avz import synth
    from avz.stream import StreamingBeamformer, StreamingDelayMask
    dev = torch.device("cuda:0")
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    B, n = a.streams, int(a.seconds * synth.FS)
    for d in (0.08, 0.01):
        mix, _, _ = synth.make_batch_device(B, start=0, n_samples=n, n_interferers=1, d=d,
                                            snr_db=20.0, device=dev, rng="philox")
        for n_fft in (512, 1024):
            H, F = n_fft // 2, n_fft // 2 + 1
            T = n // H
            plan = avz.MVDRPlan(n_fft=n_fft, sigma=1e-5, mic_d=d, mask="external",
                                postfilter="floor", normalize="none", max_batch=B,
                                max_samples=n)
            g = DM.delay_grid(n_fft, synth.FS, d, synth.C_SOUND, a.hist_bins)
            for hops in (1, 8):
                dm = StreamingDelayMask(plan, B, a.hist_bins, a.forget, device=dev)
                bf = StreamingBeamformer(plan, B, forget=0.99, device=dev)
                mask = torch.ones((B, F, hops), dtype=torch.float32, device=dev)
                out = torch.empty((B, hops * H), dtype=torch.float32, device=dev)
                ms_m, ms_b, host = [], [], []
                for i in range(a.warmup + a.calls):
                    j = (i * hops) % (T - hops)
                    x = mix[:, :, j * H:(j + hops) * H]
                    torch.cuda.synchronize()
                    e = [ev() for _ in range(4)]
                    t0 = time.perf_counter()
                    e[0].record()
                    dm.push(x, mask=mask)
                    e[1].record()
                    e[1].synchronize()
                    t1 = time.perf_counter()
                    e[2].record()
                    bf.push(x, mask=mask, out=out)
                    e[3].record()
                    e[3].synchronize()
                    if i >= a.warmup:
                        ms_m.append(e[0].elapsed_time(e[1]))
                        ms_b.append(e[2].elapsed_time(e[3]))
                        host.append((t1 - t0) * 1e3)
                m = stats(ms_m)
                print(json.dumps({"what": "delay stream push", "n_fft": n_fft, "mic_d": d,
                                  "streams": B, "hops": hops, "hist_bins": a.hist_bins,
                                  "band": [g.k_lo, g.k_hi], "calls": a.calls,
                                  "hop_ms": round(1e3 * H / synth.FS, 3),
                                  "real_time": bool(hops > 1 or m["max"] < 1e3 * H / synth.FS),
                                  "event_ms": m, "host_sync_ms": stats(host),
                                  "beamformer_event_ms": stats(ms_b),
                                  "state_mb": round(dm.state.numel() / 2 ** 20, 2),
                                  "target_share": round(float(mask.mean().item()), 3),
                                  "tf_bins_per_s": round(B * F * hops / (m["median"] * 1e-3), 0)}))
                del dm, bf


if __name__ == "__main__":
    main()
