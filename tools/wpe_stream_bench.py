#!/usr/bin/env python3
"""Time the streaming online WPE (avz_wpe_stream_push), K = 10, D = 3,
the device generator's scenes:

 (a) one push of hops = 1 for streams in {1, 64, 256} and N in {512, 1024}: the synchronous
     host-clock time (call + wait: what a real-time caller waits for) and the HIP-event time,
     each the median (min - max) of --calls pushes after warm-up, next to the hop's own
     duration;
 (b) a whole --seconds utterance per stream in one call (streams = 256), in TF-bins/s, and,
     alternating in the same loop, the offline chain plan.stft -> avz_wpe_spectral (3
     iterations) -> plan.istft on the same input.

  python tools/wpe_stream_bench.py [--only a|b] [--n-fft 512]
Prints one JSON line per measurement. The split of a push over its three kernels is read from
a kernel trace of this program (rocprofv3 --kernel-trace --stats -- python tools/...)."""
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
    ap.add_argument("--batch", type=int, default=256, help="streams of measurement (b)")
    ap.add_argument("--taps", type=int, default=10)
    ap.add_argument("--delay", type=int, default=3)
    ap.add_argument("--only", choices=("a", "b"), default=None)
    ap.add_argument("--n-fft", type=int, default=None, help="one transform size only")
    a = ap.parse_args(argv)

    import torch
    import avz
    from avz import synth
    from avz.dereverb import StreamingWPE
    from avz.engine import wpe_spectral
    dev = torch.device("cuda:0")
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    FS = synth.FS
    K, D = a.taps, a.delay
    n_rows = 2 * K
    for n_fft in ((a.n_fft,) if a.n_fft else (512, 1024)):
        H, F = n_fft // 2, n_fft // 2 + 1
        T = int(a.seconds * FS) // H
        n = T * H
        B = a.batch
        mix, _, _ = synth.make_batch_device(B, start=0, n_samples=n, n_interferers=2, device=dev,
                                            rng="philox")
        plan = avz.MVDRPlan(n_fft=n_fft, mask="ones", postfilter="none", normalize="none",
                            max_batch=2 * B, max_samples=n + n_fft)
        flops_frame = 8 * F * (2 * n_rows * n_rows + 4 * n_rows)   # per stream and frame
        # (a) one hop per push
        for streams in (1, 64, 256):
            if streams > B or a.only == "b":
                continue
            sw = StreamingWPE(plan, streams, taps=K, delay=D, forget=0.99, device=dev)
            out = torch.empty((streams, 2, H), dtype=torch.float32, device=dev)
            x = mix[:streams]
            host, event = [], []
            for i in range(a.warmup + a.calls):
                j = i % T
                xi = x[:, :, j * H:(j + 1) * H]
                torch.cuda.synchronize()
                e0, e1 = ev(), ev()
                t0 = time.perf_counter()
                e0.record()
                sw.push(xi, out=out)
                e1.record()
                e1.synchronize()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    host.append((t1 - t0) * 1e3)
                    event.append(e0.elapsed_time(e1))
            print(json.dumps({"what": "push of one hop", "n_fft": n_fft, "streams": streams,
                              "taps": K, "delay": D, "calls": a.calls,
                              "hop_ms": round(1e3 * H / FS, 3), "host_sync_ms": stats(host),
                              "event_ms": stats(event),
                              "state_mb": round(sw.state.numel() / 2 ** 20, 1),
                              "rls_gflop": round(streams * flops_frame * 1e-9, 4)}))
            del sw
        if a.only == "a":
            continue
        # (b) whole utterances in one call against the offline chain, alternating
        sw = StreamingWPE(plan, B, taps=K, delay=D, forget=0.99, device=dev)
        out_s = torch.empty((B, 2, n), dtype=torch.float32, device=dev)
        ms_s, ms_o = [], []
        for i in range(a.warmup + a.calls):
            e = [ev() for _ in range(4)]
            sw.reset()
            e[0].record()
            sw.push(mix, out=out_s)
            e[1].record()
            e[2].record()
            Y = plan.stft(mix, None, n)
            wpe_spectral(Y, K, D, 3, out=Y)
            plan.istft(Y.view(2 * B, F, Y.shape[-1]))
            e[3].record()
            e[3].synchronize()
            if i >= a.warmup:
                ms_s.append(e[0].elapsed_time(e[1]))
                ms_o.append(e[2].elapsed_time(e[3]))
        s, o = stats(ms_s), stats(ms_o)
        print(json.dumps({"what": "whole utterance per call", "n_fft": n_fft, "streams": B,
                          "taps": K, "delay": D, "seconds": a.seconds, "frames": T,
                          "calls": a.calls, "stream_ms": s, "offline_ms": o,
                          "stream_tf_bins_per_s": round(B * F * T / (s["median"] * 1e-3), 0),
                          "offline_tf_bins_per_s": round(B * F * (T + 1) / (o["median"] * 1e-3), 0),
                          "rls_gflop": round(B * T * flops_frame * 1e-9, 2)}))


if __name__ == "__main__":
    main()
