#!/usr/bin/env python3
"""Time the blind delay-histogram mask (avz_delay_mask) on --batch
utterances of --seconds at N = 1024 and N = 512 (the device generator's scenes, one
interferer, SNR 20), and, alternating in the same loop, the composition a user had before it:
avz_stft plus torch operations for the same three stages (histogram by scatter_add_, peaks by
a convolution and topk, labels by broadcast costs), all on the device without a host sync.

Each figure is the median (min - max) of --calls HIP-event times after --warmup calls. The
fused path's achieved bytes/s is set against its design traffic: 8 B read per (bin, frame) on
each of the two transform passes and 4 B written, 20 B per (bin, frame).

  python tools/delay_mask_bench.py
Prints one JSON line per transform size."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-audio-visual-zooming_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def stats(v):
    v = sorted(v)
    med = 0.5 * (v[(len(v) - 1) // 2] + v[len(v) // 2])
    return {"median": round(med, 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def composition(plan, mix, g, smooth=3, rel_height=0.25, min_sep=0.2, max_peaks=3, angle=90.0):
    """The three stages with avz_stft and torch operations: M [B, F, T] float32."""
    import torch
    Y = plan.stft(mix)                                    # [B, 2, F, T] complex64
    B, _, F, T = Y.shape
    dev = Y.device
    k = torch.arange(g.k_lo, g.k_hi + 1, device=dev)
    X = Y[:, 1, g.k_lo:g.k_hi + 1] * Y[:, 0, g.k_lo:g.k_hi + 1].conj()
    w = X.abs()
    u = torch.angle(X) * (g.n_fft / (2 * math.pi * g.bin_w) / k)[None, :, None] + (0.5 * g.nb - 0.5)
    i0 = torch.floor(u)
    phi = u - i0
    i0 = i0.long().clamp_(-1, g.nb - 1) + 1               # one guard bin on each side
    h = torch.zeros((B, g.nb + 2), dtype=torch.float64, device=dev)
    h.scatter_add_(1, i0.reshape(B, -1), ((1 - phi) * w).double().reshape(B, -1))
    h.scatter_add_(1, (i0 + 1).reshape(B, -1), (phi * w).double().reshape(B, -1))
    hs = h[:, 1:-1]
    ker = torch.tensor([[[0.25, 0.5, 0.25]]], dtype=torch.float64, device=dev)
    for _ in range(smooth):
        hs = torch.nn.functional.conv1d(hs[:, None], ker, padding=1)[:, 0]
    p = torch.nn.functional.pad(hs, (1, 1))
    l, m, r = p[:, :-2], p[:, 1:-1], p[:, 2:]
    top = m.max(dim=1, keepdim=True).values
    den = l - 2 * m + r
    o = torch.where(den == 0, torch.zeros_like(den), 0.5 * (l - r) / den)
    d = -g.R + (torch.arange(g.nb, device=dev) + 0.5 + o) * g.bin_w
    d_t = g.dmax * math.cos(math.radians(angle))
    cand = (top > 0) & (m > l) & (m >= r) & (m >= rel_height * top) \
        & ~((d - d_t).abs() <= min_sep * g.dmax)
    height, idx = torch.where(cand, m, -torch.ones_like(m)).topk(max_peaks, dim=1)
    kept = height >= 0                                    # [B, max_peaks]
    delays = torch.gather(d, 1, idx)
    kk = torch.arange(F, device=dev, dtype=torch.float64)[None, :, None]
    y0, y1 = Y[:, 0], Y[:, 1]

    def cost(dj):                                         # dj [B, 1, 1] float64
        ph = (2 * math.pi / g.n_fft) * kk * dj
        rot = torch.complex(torch.cos(ph).float(), torch.sin(ph).float())
        e = y1 - rot * y0
        return e.real * e.real + e.imag * e.imag

    c0 = cost(torch.full((B, 1, 1), d_t, dtype=torch.float64, device=dev))
    other = torch.zeros((B, F, T), dtype=torch.bool, device=dev)
    for j in range(max_peaks):
        other |= (cost(delays[:, j, None, None]) < c0) & kept[:, j, None, None]
    return (~other).float()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--mic-d", type=float, default=0.08)
    a = ap.parse_args(argv)

    import torch
    import avz
    from avz import delay_mask as DM
    from avz import engine, synth
    dev = torch.device("cuda:0")
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    B, n = a.batch, int(a.seconds * synth.FS)
    mix, _, _ = synth.make_batch_device(B, start=0, n_samples=n, n_interferers=1, d=a.mic_d,
                                        snr_db=20.0, device=dev, rng="philox")
    for n_fft in (1024, 512):
        F, T = n_fft // 2 + 1, engine.n_frames(n, n_fft // 2)
        plan = avz.MVDRPlan(n_fft=n_fft, sigma=1e-5, mic_d=a.mic_d, mask="external",
                            postfilter="floor", normalize="none", max_batch=B, max_samples=n)
        g = DM.delay_grid(n_fft, synth.FS, a.mic_d, synth.C_SOUND)
        mask = torch.zeros((B, F, T), dtype=torch.float32, device=dev)
        ws = torch.empty(engine.delay_mask_workspace_bytes(plan, B, n), dtype=torch.uint8,
                         device=dev)
        ms_f, ms_c = [], []
        agree = None
        for i in range(a.warmup + a.calls):
            e = [ev() for _ in range(4)]
            e[0].record()
            engine.delay_mask(plan, mix, mask=mask, workspace=ws)
            e[1].record()
            e[2].record()
            Mc = composition(plan, mix, g)
            e[3].record()
            e[3].synchronize()
            if i >= a.warmup:
                ms_f.append(e[0].elapsed_time(e[1]))
                ms_c.append(e[2].elapsed_time(e[3]))
            if agree is None:
                agree = float((Mc == mask).float().mean().item())
        f, c = stats(ms_f), stats(ms_c)
        design = 20.0 * B * F * T
        print(json.dumps({"what": "delay mask", "n_fft": n_fft, "batch": B, "seconds": a.seconds,
                          "mic_d": a.mic_d, "frames": T, "band": [g.k_lo, g.k_hi],
                          "calls": a.calls, "fused_ms": f, "composition_ms": c,
                          "composition_over_fused": round(c["median"] / f["median"], 2),
                          "decisions_equal": round(agree, 5),
                          "design_bytes": int(design),
                          "fused_gb_per_s": round(design / (f["median"] * 1e-3) / 1e9, 1),
                          "fused_tf_bins_per_s": round(B * F * T / (f["median"] * 1e-3), 0)}))


if __name__ == "__main__":
    main()
