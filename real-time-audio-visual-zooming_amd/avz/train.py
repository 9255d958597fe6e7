"""Training of the mask estimator on the device: mirror of
rt_av_zoom/core/full_audio_generating_pipeline/model_training.py.

Reference: ``SpatialDataset.__getitem__`` (:55-92) mixes three LJ-Speech segments of 32000
samples with far-field fractional delays (d = 0.04 m; 90 / 40 / 130 degrees), takes the STFTs
(1024 / 512) of the mic pair, of the mic-1 target and of the mic-1 interference, and returns
the U-Net input ``[log(|Y0| + 1e-7), angle(Y0) - angle(Y1)]`` with the label
``np.where(|S_t| > |S_i|, 1, 0)``; ``main`` (:139-183) runs Adam (lr 1e-4) on ``nn.BCELoss``
for 50 epochs of 3000 samples in batches of 32 and saves ``mask_estimator.pth``.

Here a batch never leaves the device: ``synth.make_batch_device(rng="philox")``
(avz_scene_generate, or avz_scene_reverb_generate with ``reverb=True``) builds the scenes and
``engine.mask_training_batch`` (avz_mask_training_batch, csrc/avz_train.hip) turns mix and
references into features and label in one kernel. The U-Net forward / backward and Adam are
PyTorch-ROCm.

Departures from the reference:
* sources are the generator's speech-like signals (synth.speech_like_philox), LJ-Speech
  cannot be fetched;
* the scene generator's SIR gain (0 dB on mic 1), AWGN (5 dB, in ``mix`` only, as it would be
  at inference) and shared peak normalisation apply; the label does not depend on the shared
  positive scale;
* angles are the generator's: target 90, first interferer 40, the others drawn uniformly in
  [0, 180] per scene (the reference fixes 90 / 40 / 130);
* the label is decided on the kernel's fp32 transforms (include/avz.h).
The scene indices alone fix the data: batch i holds scenes ``start_idx + i * batch_size ..``,
so a run is reproducible and shardable by ``start_idx``.
"""
from __future__ import annotations

import argparse
import itertools
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn

from . import neural, synth
from .engine import MVDRPlan, mask_training_batch

REF_BATCH, REF_LR, REF_EPOCHS, REF_EPOCH_SAMPLES = 32, 1e-4, 50, 3000  # model_training.py:29-31, 53
REF_STEPS = REF_EPOCHS * REF_EPOCH_SAMPLES // REF_BATCH
HELD_OUT_START = 1 << 24  # default first scene of evaluate(): far above any training index
# the reference room's mic pair (synth.MIC_LOCS, 0.08 m apart) at neural.CONF's d = 0.04 m
REVERB_MICS = [[2.43, 2.45, 1.5], [2.47, 2.45, 1.5]]


class Sample(NamedTuple):
    feat: np.ndarray    # [2, F, T] float64: log(|Y0| + 1e-7), angle(Y0) - angle(Y1)
    label: np.ndarray   # [F, T] float64 in {0, 1}
    norms: np.ndarray   # [2, T] float64: ||w tgt_t||_2, ||w itf_t||_2 (w the periodic Hann)
    mag_t: np.ndarray   # [F, T] |S_t|
    mag_i: np.ndarray   # [F, T] |S_i|


def features_labels_numpy(mix, tgt, itf, n_fft: int) -> Sample:
    """model_training.py:80-90 in float64: scipy ``stft`` (nperseg n_fft, 50 % overlap) of
    float64 copies of mix [2, S], tgt [S] and itf [S], ``np.abs``, ``np.angle``, ``np.where``.
    Also the L2 norms of the windowed reference frames (the frames scipy transforms: the
    signal zero-extended by n_fft / 2 on both sides and padded to whole hops) and the two
    reference magnitudes."""
    import scipy.signal
    hop = n_fft // 2
    mix, tgt, itf = (np.asarray(a, np.float64) for a in (mix, tgt, itf))
    kw = dict(fs=neural.CONF["fs"], nperseg=n_fft, noverlap=n_fft - hop)
    _, _, Y = scipy.signal.stft(mix, **kw)
    _, _, S_t = scipy.signal.stft(tgt, **kw)
    _, _, S_i = scipy.signal.stft(itf, **kw)
    mag = np.abs(Y)
    ipd = np.angle(Y[0]) - np.angle(Y[1])
    feat = np.stack([np.log(mag[0] + 1e-7), ipd], axis=0)
    mag_t, mag_i = np.abs(S_t), np.abs(S_i)
    label = np.where(mag_t > mag_i, 1.0, 0.0)
    T = label.shape[-1]
    w = scipy.signal.get_window("hann", n_fft)
    norms = np.empty((2, T))
    for r, x in enumerate((tgt, itf)):
        xp = np.zeros((T + 1) * hop)
        xp[hop:hop + len(x)] = x
        frames = np.lib.stride_tricks.sliding_window_view(xp, n_fft)[::hop][:T]
        norms[r] = np.linalg.norm(frames * w, axis=1)
    return Sample(feat, label, norms, mag_t, mag_i)


def make_plan(max_batch: int, n_samples: int) -> MVDRPlan:
    """A plan of neural.CONF's transform for avz_mask_training_batch (its mask mode and
    beamformer settings are not used by that call)."""
    c = neural.CONF
    return MVDRPlan(n_fft=int(c["n_fft"]), fs=int(c["fs"]), mic_d=float(c["d"]),
                    c_sound=float(c["c"]), mask="external", postfilter="none", normalize="none",
                    max_batch=max_batch, max_samples=n_samples)


def scenes(batch: int, start: int, n_samples: int, n_interferers: int = 2, seed: int = 0,
           reverb: bool = False, device=None):
    """(mix [B, 2, S], tgt [B, S], itf [B, S]) of scenes start .. start + batch - 1 at
    neural.CONF's geometry, generated on the device."""
    c = neural.CONF
    if reverb:
        room = synth.Room(mic=REVERB_MICS, c=float(c["c"]), fs=float(c["fs"]))
        return synth.make_reverb_batch_device(batch, start, n_samples, n_interferers, room=room,
                                              device=device, rng="philox", seed=seed)
    return synth.make_batch_device(batch, start, n_samples, n_interferers, d=float(c["d"]),
                                   fs=int(c["fs"]), device=device, rng="philox", seed=seed)


def training_batches(batch_size: int, start_idx: int = 0, seconds: float = 2.0,
                     n_interferers: int = 2, seed: int = 0, reverb: bool = False, plan=None,
                     device=None):
    """Infinite iterator of (feat [B, 2, F, T], label [B, F, T]) device tensors: batch i is
    scenes start_idx + i * batch_size .. (consecutive indices) through
    engine.mask_training_batch. seconds = 2.0 gives neural.CONF's 32000-sample segments."""
    n = int(round(seconds * neural.CONF["fs"]))
    plan = plan or make_plan(batch_size, n)
    for i in itertools.count():
        mix, tgt, itf = scenes(batch_size, start_idx + i * batch_size, n, n_interferers, seed,
                               reverb, device)
        yield mask_training_batch(plan, mix, tgt, itf, "unet")


def train(model: nn.Module | None = None, steps: int = REF_STEPS, batch_size: int = REF_BATCH,
          lr: float = REF_LR, seed: int = 0, start_idx: int = 0, seconds: float = 2.0,
          n_interferers: int = 2, reverb: bool = False, batches=None, log_every: int = 0,
          max_seconds: float | None = None, device=None):
    """model_training.main's loop (:152-171) for ``steps`` optimiser steps: model.train(),
    Adam(lr), nn.BCELoss on batches from ``training_batches`` (or the given iterable of
    (feat, label) pairs). ``model`` None: a FreqPreservingUNet initialised under
    torch.manual_seed(seed). ``max_seconds``: stop early once that much wall time has passed
    (looked at every 10 steps, after waiting for the device). Returns (model, losses), the
    per-step losses as floats."""
    import time
    dev = device or torch.device("cuda", torch.cuda.current_device())
    if model is None:
        torch.manual_seed(seed)
        model = neural.FreqPreservingUNet()
    model = model.to(dev)
    if batches is None:
        batches = training_batches(batch_size, start_idx, seconds, n_interferers, seed, reverb,
                                   device=dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    crit = nn.BCELoss()
    model.train()
    losses = []
    t0 = time.perf_counter()
    for step, (x, y) in enumerate(itertools.islice(batches, steps)):
        opt.zero_grad()
        loss = crit(model(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        if log_every and (step + 1) % log_every == 0:
            print(f"step {step + 1}/{steps} loss {float(losses[-1]):.6f}", flush=True)
        if max_seconds is not None and (step + 1) % 10 == 0:
            float(losses[-1])  # wait for the device: the host runs ahead of it
            if time.perf_counter() - t0 >= max_seconds:
                break
    return model, [float(v) for v in torch.stack(losses).cpu()] if losses else []


@torch.no_grad()
def evaluate(model: nn.Module, n_scenes: int = 64, start_idx: int = HELD_OUT_START,
             seconds: float = 2.0, n_interferers: int = 2, seed: int = 0, reverb: bool = False,
             batch_size: int = 32, device=None) -> dict:
    """Scores of ``model`` (run in eval mode; its mode is restored) on scenes start_idx ..
    start_idx + n_scenes - 1, which a training run from index 0 does not reach:
    bce       mean binary cross-entropy of the mask against the label;
    match     share of (bin, frame) labels equal to (mask > 0.5);
    sir       mean output SIR (dB, avz_projection_metrics' SIR column) of
              NeuralMaskBeamformer with this model;
    sir_mix   the same figure for mic 0 of the mixture."""
    from .metrics import projection_metrics
    dev = device or torch.device("cuda", torch.cuda.current_device())
    n = int(round(seconds * neural.CONF["fs"]))
    was_training = model.training
    model = model.to(dev).eval()
    plan = make_plan(batch_size, n)
    bf = neural.NeuralMaskBeamformer(model, max_items=batch_size * -(-n // (neural.CONF[
        "train_seg_samples"] // 2)), fold_bn=False, channels_last=False)
    crit = nn.BCELoss(reduction="sum")
    bce = hit = cells = 0.0
    sir, sir_mix = [], []
    for s in range(0, n_scenes, batch_size):
        nb = min(batch_size, n_scenes - s)
        mix, tgt, itf = scenes(nb, start_idx + s, n, n_interferers, seed, reverb, dev)
        feat, label = mask_training_batch(plan, mix, tgt, itf, "unet")
        pred = model(feat)
        bce += float(crit(pred, label))
        hit += float(((pred > 0.5).float() == label).sum())
        cells += label.numel()
        out, _ = bf.run(mix)
        sir.append(projection_metrics(out[:, :n], tgt, itf)[:, 3])
        sir_mix.append(projection_metrics(mix[:, 0].contiguous(), tgt, itf)[:, 3])
    if was_training:
        model.train()
    return {"bce": bce / cells, "match": hit / cells, "sir": float(torch.cat(sir).mean()),
            "sir_mix": float(torch.cat(sir_mix).mean()), "n_scenes": n_scenes}


def main(argv=None):
    ap = argparse.ArgumentParser(description="Train the mask estimator on generated scenes and "
                                 "save a state_dict that avz.neural.load_model loads.")
    ap.add_argument("--epochs", type=int, default=REF_EPOCHS,
                    help=f"epochs of {REF_EPOCH_SAMPLES} scenes (model_training.py)")
    ap.add_argument("--steps", type=int, default=None, help="optimiser steps (overrides --epochs)")
    ap.add_argument("--batch-size", type=int, default=REF_BATCH)
    ap.add_argument("--lr", type=float, default=REF_LR)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reverb", action="store_true", help="scenes in the reference room")
    ap.add_argument("--eval-scenes", type=int, default=64, help="held-out scenes (0: skip)")
    ap.add_argument("--log-every", type=int, default=100)
    ap.add_argument("--out", default="mask_estimator.pth")
    a = ap.parse_args(argv)
    steps = a.steps if a.steps is not None else a.epochs * REF_EPOCH_SAMPLES // a.batch_size
    model, losses = train(steps=steps, batch_size=a.batch_size, lr=a.lr, seed=a.seed,
                          reverb=a.reverb, log_every=a.log_every)
    if losses:
        k = min(10, len(losses))
        print(f"BCE first {k} steps {np.mean(losses[:k]):.6f}, last {k} {np.mean(losses[-k:]):.6f}")
    if a.eval_scenes > 0:
        print("held-out:", evaluate(model, a.eval_scenes, reverb=a.reverb, seed=a.seed))
    torch.save(model.state_dict(), a.out)
    print(f"Saved {a.out}")
    return model, losses


if __name__ == "__main__":
    main()
