"""Streaming causal MVDR: feed a stream hop by hop, get enhanced audio back one hop later.

``StreamingBeamformer`` drives avz_stream_push / avz_stream_reset / avz_stream_steer
(include/avz.h) over one caller-owned device state buffer; ``NumpyStream`` / ``stream_numpy``
restate the algorithm in fp64 (the tests' reference);
``enhance_stream`` runs a whole file through the device path and trims the one-hop delay:
the causal counterpart of oracle_debug.enhance / process_chunk. ``StreamingDelayMask`` drives
avz_delay_stream_push, the streaming blind delay-histogram mask;
``StreamingBlindBeamformer`` feeds its mask to a ``StreamingBeamformer`` and
``enhance_blind_stream`` runs a whole file through the pair: no references, no model.

The algorithm, with H = N / 2 and x_t the t-th pushed hop (x_-1 = 0): frame t = [x_t-1 | x_t]
under the fp32 periodic Hann scaled by 1 / sum(w) (frame t of scipy.signal.stft); the noise
weight n_t of the plan's mask mode; the sums c_t = forget c_t-1 + n_t (|y0|^2, |y1|^2,
Re y0 y1*, Im y0 y1*, 1) where the adapt flag is set, else c_t = c_t-1; the MVDR weights of
c_t with the stream's steering vector; S_t = w_t^H Y_t times the post-filter gain;
g_t = irfft(S_t) sum(w) w and output hop t = (g_t-1[H:] + g_t[:H]) / (w^2[m] + w^2[m + H])
for t >= 1, zeros for t = 0 (scipy.signal.istft of the causal S, delayed by one hop).
"""
from __future__ import annotations

import numpy as np


# ---------------------------------------------------------------------------- fp64 restatement
def hann_periodic(n: int) -> np.ndarray:
    """scipy.signal.get_window('hann', n), float64."""
    return 0.5 + 0.5 * np.cos(np.linspace(-np.pi, np.pi, n + 1)[:-1])


def steering_table(f_bins, angle_deg: float, mic_d: float, c_sound: float) -> np.ndarray:
    """masked_mvdr.get_steering_vector for every bin: [F, 2] complex128."""
    theta = np.deg2rad(angle_deg)
    tau1 = (mic_d / 2) * np.cos(theta) / c_sound
    tau2 = (mic_d / 2) * np.cos(theta - np.pi) / c_sound
    omega = 2 * np.pi * np.asarray(f_bins, dtype=np.float64)
    return np.stack([np.exp(-1j * omega * tau1), np.exp(-1j * omega * tau2)], axis=-1)


def mvdr_weights(c, f_bins, d, sigma, fmin_hz, singular_fallback="mic0"):
    """mvdr_weights_d (csrc/avz_common.hpp) for every bin: c [F, 5] sums, d [F, 2] steering
    vectors -> w [F, 2] complex128."""
    with np.errstate(all="ignore"):
        nrm = c[:, 4] + 1e-6
        a = c[:, 0] / nrm + sigma
        e = c[:, 1] / nrm + sigma
        b = (c[:, 2] + 1j * c[:, 3]) / nrm
        det = a * e - (b.real * b.real + b.imag * b.imag)
        ok = np.isfinite(det) & (det != 0)
        safe = np.where(ok, det, 1.0)
        t0 = (e * d[:, 0] - b * d[:, 1]) / safe
        t1 = (a * d[:, 1] - np.conj(b) * d[:, 0]) / safe
        den = np.conj(d[:, 0]) * t0 + np.conj(d[:, 1]) * t1 + 1e-10
        w = np.stack([t0 / den, t1 / den], axis=-1)
    w[det == 0] = {"mic0": (1.0, 0.0), "mean": (0.5, 0.5)}[singular_fallback]
    w[~np.isfinite(det)] = np.nan
    w[np.asarray(f_bins) < fmin_hz] = 0.0
    return w


class NumpyStream:
    """One stream of the algorithm in fp64, stateful: push() any number of hops at a time.
    Every frame is computed on its own, so the results do not depend on the grouping.

    mask_mode 'external' (push(mask=M [F, hops]) target probability), 'ibm' (push(ref_tgt=,
    ref_int=) or push(noise=) to impose decisions) or 'ones'. History of every frame pushed
    so far: Y [t][2, F], noise [t][F], c [t][F, 5], w [t][F, 2], S [t][F]."""

    def __init__(self, n_fft=1024, fs=16000, sigma=1.0, angle_deg=90.0, mic_d=0.01,
                 c_sound=343.0, fmin_hz=100.0, mask_mode="external", postfilter="none",
                 pf_floor=0.05, weight_eps=0.0, singular_fallback="mic0", forget=1.0,
                 y_hook=None):
        if not 0.0 < forget <= 1.0:
            raise ValueError("forget must lie in (0, 1]")
        self.N, self.H, self.F = n_fft, n_fft // 2, n_fft // 2 + 1
        self.f_bins = np.fft.rfftfreq(n_fft, 1.0 / fs)
        self.sigma, self.fmin_hz, self.forget = sigma, fmin_hz, forget
        self.mic_d, self.c_sound = mic_d, c_sound
        self.mask_mode, self.postfilter, self.pf_floor = mask_mode, postfilter, pf_floor
        self.weight_eps = float(np.float32(weight_eps))
        self.singular_fallback = singular_fallback
        self.win = hann_periodic(n_fft)                               # synthesis: fp64
        self.win32 = self.win.astype(np.float32).astype(np.float64)  # analysis: the fp32 window
        self.scale = 1.0 / self.win32.sum()
        self.y_hook = y_hook                                          # (t, Y [2, F]) -> Y
        self.angle_deg = angle_deg
        self.reset()

    def reset(self):
        self.count = 0
        self.prev = np.zeros((4, self.H))
        self.tail = np.zeros(self.H)
        self.c = np.zeros((self.F, 5))
        self.d = steering_table(self.f_bins, self.angle_deg, self.mic_d, self.c_sound)
        self.w = np.zeros((self.F, 2), dtype=complex)
        self.hist = {k: [] for k in ("Y", "noise", "c", "w", "S")}

    def steer(self, angle_deg=None, table=None):
        """New direction from the next pushed frame: an angle (the formula) or a [F, 2] table."""
        self.d = (np.asarray(table, dtype=complex) if table is not None
                  else steering_table(self.f_bins, angle_deg, self.mic_d, self.c_sound))

    def _rfft(self, prev, cur):
        return np.fft.rfft(np.concatenate([prev, cur]) * self.win32) * self.scale

    def push(self, mix, *, mask=None, ref_tgt=None, ref_int=None, noise=None, adapt=True):
        mix = np.asarray(mix, dtype=np.float64)
        H = self.H
        hops = mix.shape[-1] // H
        assert mix.shape == (2, hops * H) and hops >= 1
        out = np.zeros(hops * H)
        for j in range(hops):
            sl = slice(j * H, (j + 1) * H)
            cur = [mix[0, sl], mix[1, sl]]
            Y = np.stack([self._rfft(self.prev[m], cur[m]) for m in range(2)])
            if self.y_hook is not None:
                Y = self.y_hook(self.count, Y)
            M = None
            if self.mask_mode == "ibm" and ref_tgt is not None:
                cur += [np.asarray(ref_tgt, dtype=np.float64)[sl],
                        np.asarray(ref_int, dtype=np.float64)[sl]]
            if noise is not None:
                n = np.asarray(noise, dtype=np.float64)[:, j]
            elif self.mask_mode == "ibm":
                St, Si = self._rfft(self.prev[2], cur[2]), self._rfft(self.prev[3], cur[3])
                n = np.where(np.abs(Si) > np.abs(St), 1.0, 0.0)
            elif self.mask_mode == "ones":
                n = np.ones(self.F)
            else:
                n = None
            if self.mask_mode == "external":
                M = np.asarray(mask)[:, j].astype(np.float32)
                n = (np.float32(1.0) - M).astype(np.float64)          # float32, as numpy's 1 - M
                M = M.astype(np.float64)
            wgt = n + self.weight_eps if self.mask_mode == "external" else n
            if adapt:
                y0, y1 = Y
                x = y0 * np.conj(y1)
                upd = np.stack([wgt * np.abs(y0) ** 2, wgt * np.abs(y1) ** 2, wgt * x.real,
                                wgt * x.imag, n], axis=-1)
                self.c = self.forget * self.c + upd
            self.w = mvdr_weights(self.c, self.f_bins, self.d, self.sigma, self.fmin_hz,
                                  self.singular_fallback)
            # coef_from_w: alpha = (conj w0 - i conj w1) / 2, beta = (conj w0 + i conj w1) / 2,
            # rounded to complex64; S = alpha (y0 + i y1) + beta (y0 - i y1)
            w0c, w1c = np.conj(self.w[:, 0]), np.conj(self.w[:, 1])
            alpha = (0.5 * (w0c - 1j * w1c)).astype(np.complex64).astype(complex)
            beta = (0.5 * (w0c + 1j * w1c)).astype(np.complex64).astype(complex)
            S = alpha * (Y[0] + 1j * Y[1]) + beta * (Y[0] - 1j * Y[1])
            if self.postfilter == "ibm":
                S = S * (1.0 - n)
            elif self.postfilter == "floor":
                S = S * np.maximum(M, float(np.float32(self.pf_floor)))
            elif self.postfilter == "mul":
                S = S * M
            g = np.fft.irfft(S, n=self.N) * self.win.sum() * self.win
            if self.count > 0:
                out[sl] = (self.tail + g[:H]) / (self.win[:H] ** 2 + self.win[H:] ** 2)
            self.tail = g[H:]
            self.prev[:len(cur)] = np.stack(cur)
            self.count += 1
            for k, v in (("Y", Y), ("noise", n), ("c", self.c.copy()), ("w", self.w.copy()),
                         ("S", S)):
                self.hist[k].append(v)
        return out

    def flush(self):
        """One hop of zeros: drains the last H samples."""
        z = np.zeros(self.H)
        return self.push(np.zeros((2, self.H)), mask=np.ones((self.F, 1), np.float32),
                         ref_tgt=z, ref_int=z)


def stream_numpy(mix, *, hops_per_push=None, mask=None, ref_tgt=None, ref_int=None, noise=None,
                 adapt=None, steer=None, drain=True, **cfg):
    """A whole signal through NumpyStream: mix [2, T H] -> (out [(T + drain) H], stream).
    adapt: per-hop flags [T] (default all 1); steer: {hop index: angle in degrees or [F, 2]
    table}, applied before that hop is pushed; hops_per_push: an int or a list of group
    sizes (the grouping does not change the results). The drain hop always adapts with an
    all-target mask / zero references, as flush() pushes it."""
    st = NumpyStream(**cfg)
    H = st.H
    T = np.asarray(mix).shape[-1] // H
    groups = hops_per_push if isinstance(hops_per_push, (list, tuple)) else None
    if groups is None:
        g = hops_per_push or T
        groups = [min(g, T - i) for i in range(0, T, g)]
    assert sum(groups) == T
    adapt = np.ones(T, dtype=int) if adapt is None else np.asarray(adapt)
    steer = steer or {}
    cuts = sorted(set(np.cumsum([0] + list(groups))) | set(steer) |
                  set(np.flatnonzero(np.diff(adapt)) + 1))
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a in steer:
            v = steer[a]
            st.steer(table=v) if np.ndim(v) == 2 else st.steer(angle_deg=float(v))
        sl = slice(a * H, b * H)
        outs.append(st.push(np.asarray(mix)[:, sl],
                            mask=None if mask is None else np.asarray(mask)[:, a:b],
                            ref_tgt=None if ref_tgt is None else np.asarray(ref_tgt)[sl],
                            ref_int=None if ref_int is None else np.asarray(ref_int)[sl],
                            noise=None if noise is None else np.asarray(noise)[:, a:b],
                            adapt=bool(adapt[a])))
    if drain:
        if noise is not None and np.asarray(noise).shape[1] > T:
            z = np.zeros(H)
            outs.append(st.push(np.zeros((2, H)), noise=np.asarray(noise)[:, T:T + 1],
                                ref_tgt=z, ref_int=z))
        else:
            outs.append(st.flush())
    return np.concatenate(outs), st


# ---------------------------------------------------------------------------- device path
class StreamOwner:
    """What the objects that own a stream state buffer share: plan, streams, device, the
    zeroed uint8 buffer of ``state_bytes(plan, streams, *size_args)`` bytes (an engine
    ``*_state_bytes`` function), and the conversions of per-stream arguments."""

    def __init__(self, plan, streams: int, device, state_bytes, *size_args):
        import torch
        self.plan, self.streams = plan, int(streams)
        self.device = torch.device(device if device is not None else "cuda")
        self.state = torch.zeros(state_bytes(plan, self.streams, *size_args), dtype=torch.uint8,
                                 device=self.device)

    def _per_stream(self, v, name, dtype):
        import torch
        t = torch.as_tensor(v, device=self.device).to(dtype).contiguous()
        if tuple(t.shape) != (self.streams,):
            raise ValueError(f"{name} must have one entry per stream")
        return t

    def _flags(self, v, name):
        """int32 [streams] on the device of per-stream flags (None stays None)."""
        import torch
        return None if v is None else self._per_stream(v, name, torch.int32)

    def _angles(self, angles):
        """float64 [streams] on the device of per-stream angles in degrees."""
        import torch
        return self._per_stream(torch.as_tensor(angles, dtype=torch.float64), "angles",
                                torch.float64)

    def _block(self, mix):
        """A pushed block has one row per stream (engine checks the rest)."""
        if mix.dim() != 3 or mix.shape[0] != self.streams:
            raise ValueError("mix must be float32 [streams, 2, hops * hop] on the device")
        return mix

    def _zero_hop(self):
        """One hop of zeros, what flush() pushes."""
        import torch
        return torch.zeros((self.streams, 2, self.plan.hop), dtype=torch.float32,
                           device=self.device)


class StreamingBeamformer(StreamOwner):
    """`streams` independent causal beamformers over one device state buffer.

    plan: an MVDRPlan with beamformer 'mvdr', mask 'external', 'ibm' or 'ones', postfilter
    other than 'irm', singular_fallback 'mic0' or 'mean' and normalize 'none' (anything else
    raises AvzError: unsupported configuration); streams <= plan.cfg.max_batch."""

    def __init__(self, plan, streams: int, forget: float = 1.0, device=None):
        import torch
        from . import engine
        super().__init__(plan, streams, device, engine.stream_state_bytes)
        self.forget = float(forget)
        self.w = torch.zeros((self.streams, plan.F, 4), dtype=torch.float32, device=self.device)
        self.cov = torch.zeros((self.streams, plan.F, 5), dtype=torch.float64,
                               device=self.device)
        self.reset()

    def reset(self, select=None, stream=None):
        """Start the selected streams (flags per stream; None = all) afresh: zero history,
        the plan's direction."""
        from . import engine
        engine.stream_reset(self.plan, self.state, self.streams, self._flags(select, "select"),
                            stream)

    def steer(self, angles, stream=None):
        """New direction per stream in degrees (NaN = keep), from the next pushed frame."""
        from . import engine
        engine.stream_steer(self.plan, self.state, self.streams, self._angles(angles), stream)

    def push(self, mix, *, ref_tgt=None, ref_int=None, mask=None, active=None, adapt=None,
             out=None, mask_out=None, stream=None):
        """mix [streams, 2, hops * hop] float32 -> out [streams, hops * hop]: the hops that
        left the beamformer, one hop behind the input. mask [streams, F, hops] (external);
        ref_tgt / ref_int [streams, hops * hop] (ibm). self.w / self.cov hold the weights and
        sums after the call's last frame."""
        import torch
        from . import engine
        self._block(mix)
        if out is None:
            out = torch.empty((self.streams, mix.shape[2]), dtype=torch.float32,
                              device=mix.device)
        if ref_tgt is not None and ref_int is not None and \
                ref_int.stride(0) != ref_tgt.stride(0):
            # engine.stream_push wants one row stride for both: copies here instead of raising
            ref_tgt, ref_int = ref_tgt.contiguous(), ref_int.contiguous()
        return engine.stream_push(self.plan, self.state, mix, out, forget=self.forget,
                                  ref_tgt=ref_tgt, ref_int=ref_int, mask=mask,
                                  active=self._flags(active, "active"),
                                  adapt=self._flags(adapt, "adapt"), w_out=self.w,
                                  cov_out=self.cov, mask_out=mask_out, stream=stream)

    def flush(self, **kw):
        """Push one hop of zeros (all-target mask, zero references): returns the last hop."""
        import torch
        z = self._zero_hop()
        mode = self.plan.cfg.mask
        if mode == "external":
            kw.setdefault("mask", torch.ones((self.streams, self.plan.F, 1),
                                             dtype=torch.float32, device=self.device))
        elif mode == "ibm":
            kw.setdefault("ref_tgt", z[:, 0])
            kw.setdefault("ref_int", z[:, 1])
        return self.push(z, **kw)


def enhance_stream(y_mix, mask_fn_or_refs=None, hops_per_push: int = 1, *, n_fft: int = 1024,
                   forget: float = 1.0, angle_deg: float = 90.0, device="cuda", **plan_kw):
    """A whole file through the streaming beamformer, the one-hop delay trimmed: y_mix [2, L]
    -> [L] float32. mask_fn_or_refs: a (ref_tgt, ref_int) pair of [L] signals (IBM plan), a
    callable (hop index j0, mix block [2, hops * hop] tensor) -> target probability [F, hops]
    tensor (external plan; it sees nothing later than its block: causal), or None (mask
    'ones': MPDR). plan_kw: MVDRPlan options (sigma, mic_d, postfilter, ...)."""
    import torch
    from .engine import MVDRPlan
    y = np.asarray(y_mix, dtype=np.float32)
    L, H = y.shape[1], n_fft // 2
    T = -(-L // H)
    refs = isinstance(mask_fn_or_refs, (tuple, list))
    mode = "ibm" if refs else ("ones" if mask_fn_or_refs is None else "external")
    plan_kw.setdefault("postfilter", "ibm" if refs else "none")
    plan = MVDRPlan(n_fft=n_fft, mask=mode, normalize="none", angle_deg=angle_deg, max_batch=1,
                    max_samples=max(T * H, n_fft), **plan_kw)
    dev = torch.device(device)
    pad = lambda a: torch.from_numpy(np.pad(np.asarray(a, np.float32),  # noqa: E731
                                            [(0, 0)] * (np.ndim(a) - 1) + [(0, T * H - L)])).to(dev)
    x = pad(y)[None]
    r = [pad(a)[None] for a in mask_fn_or_refs] if refs else None
    sb = StreamingBeamformer(plan, 1, forget=forget, device=dev)
    outs = []
    for j0 in range(0, T, hops_per_push):
        sl = slice(j0 * H, min(j0 + hops_per_push, T) * H)
        kw = {}
        if refs:
            kw = dict(ref_tgt=r[0][:, sl], ref_int=r[1][:, sl])
        elif mode == "external":
            kw = dict(mask=mask_fn_or_refs(j0, x[0, :, sl])[None].to(torch.float32).contiguous())
        outs.append(sb.push(x[:, :, sl].contiguous(), **kw))
    outs.append(sb.flush())
    return torch.cat(outs, dim=1)[0, H:H + L].cpu().numpy()


# ---------------------------------------------------------------------------- blind device path
class StreamingDelayMask(StreamOwner):
    """`streams` independent streaming blind delay-histogram masks over one device state buffer
    (avz_delay_stream_push, include/avz.h). The plan supplies n_fft, fs,
    mic_d, c_sound, angle_deg and max_batch; its mask and beamformer settings play no part.
    mask_kw: smooth, rel_height, min_sep, max_peaks, f_lo (avz_delay_mask's). After a push
    self.hist [streams, hist_bins] holds h after its last frame, self.delays [streams, hops, 8]
    and self.n_peaks [streams, hops] every frame's list."""

    def __init__(self, plan, streams: int, hist_bins: int = 65, forget: float = 1.0, device=None,
                 **mask_kw):
        import torch
        from . import engine
        from .delay_mask import DEFAULTS
        unknown = set(mask_kw) - (set(DEFAULTS) - {"hist_bins"})
        if unknown:
            raise TypeError(f"unknown mask options {sorted(unknown)}")
        self.forget, self.hist_bins, self.mask_kw = float(forget), int(hist_bins), dict(mask_kw)
        super().__init__(plan, streams, device, engine.delay_stream_state_bytes, self.hist_bins)
        self.hist = torch.zeros((self.streams, self.hist_bins), dtype=torch.float64,
                                device=self.device)
        self.angles = None
        self.delays = self.n_peaks = None
        self.reset()

    def reset(self, select=None, stream=None):
        """Start the selected streams (flags per stream; None = all) afresh: zero history and
        histogram. The target azimuths stay."""
        from . import engine
        engine.delay_stream_reset(self.plan, self.state, self.streams, self.hist_bins,
                                  self._flags(select, "select"), stream)

    def steer(self, angles):
        """New target azimuth per stream in degrees (NaN = the plan's), from the next pushed
        frame; None returns every stream to the plan's."""
        self.angles = None if angles is None else self._angles(angles)

    def push(self, mix, *, active=None, adapt=None, mask=None, stream=None):
        """mix [streams, 2, hops * hop] float32 -> mask [streams, F, hops] float32: column j
        labels the frame that ends with hop j, the frame StreamingBeamformer.push of the same
        hops weights."""
        import torch
        from . import engine
        hops = self._block(mix).shape[2] // self.plan.hop
        self.delays = torch.full((self.streams, hops, 8), float("nan"), dtype=torch.float64,
                                 device=mix.device)
        self.n_peaks = torch.zeros((self.streams, hops), dtype=torch.int32, device=mix.device)
        return engine.delay_stream_push(self.plan, self.state, mix, mask, forget=self.forget,
                                        angles=self.angles, active=self._flags(active, "active"),
                                        adapt=self._flags(adapt, "adapt"),
                                        hist_bins=self.hist_bins, hist_out=self.hist,
                                        delays_out=self.delays, n_peaks=self.n_peaks,
                                        stream=stream, **self.mask_kw)


class StreamingBlindBeamformer:
    """A StreamingDelayMask feeding a StreamingBeamformer on an external-mask plan: causal
    blind enhancement from two microphones and an angle per stream. push() is the mask, then
    the beamformer, on the same hops; out is one hop behind the input. self.mask holds the
    last push's mask."""

    def __init__(self, plan, streams: int, forget: float = 0.99, hist_bins: int = 65,
                 hist_forget: float = 1.0, device=None, **mask_kw):
        if plan.cfg.mask != "external":
            raise ValueError("StreamingBlindBeamformer needs a plan with mask='external'")
        self.plan, self.streams = plan, int(streams)
        self.masker = StreamingDelayMask(plan, streams, hist_bins, hist_forget, device, **mask_kw)
        self.beamformer = StreamingBeamformer(plan, streams, forget, device)
        self.mask = None

    def reset(self, select=None, stream=None):
        self.masker.reset(select, stream)
        self.beamformer.reset(select, stream)

    def steer(self, angles, stream=None):
        """New target azimuth per stream in degrees, for the mask's anchor and the beamformer's
        steering vector alike. A NaN entry keeps the beamformer's direction and returns the
        mask's anchor to the plan's angle."""
        self.masker.steer(angles)
        self.beamformer.steer(angles, stream)

    def push(self, mix, *, active=None, adapt=None, out=None, stream=None):
        self.mask = self.masker.push(mix, active=active, adapt=adapt, stream=stream)
        return self.beamformer.push(mix, mask=self.mask, active=active, adapt=adapt, out=out,
                                    stream=stream)

    def flush(self, **kw):
        """Push one hop of zeros through both: returns the last hop."""
        return self.push(self.beamformer._zero_hop(), **kw)


def enhance_blind_stream(y_mix, hops_per_push: int = 1, dereverb: bool = False, *,
                         n_fft: int = 1024, mic_d: float = 0.08, sigma: float = 1e-5,
                         angle: float = 90.0, fs: int = 16000, c_sound: float = 343.0,
                         pf_floor: float = 0.05, forget: float = 0.99, hist_forget: float = 1.0,
                         wpe_kw=None, device="cuda", **mask_kw):
    """The causal counterpart of delay_mask.enhance_blind: y_mix [2, L] float32 -> [L] float32
    (not normalised), the file pushed ``hops_per_push`` hops at a time through
    StreamingBlindBeamformer (external mask, floor post-filter), drained, the one-hop delay
    trimmed. ``dereverb``: dereverb.StreamingWPE (options ``wpe_kw``) in front, two hops of
    delay in all. forget: the beamformer's; hist_forget: the histogram's. mask_kw:
    hist_bins, smooth, rel_height, min_sep, max_peaks, f_lo."""
    import torch
    from .engine import MVDRPlan
    y = np.ascontiguousarray(y_mix, dtype=np.float32)
    if y.ndim != 2 or y.shape[0] != 2 or y.shape[1] < 1:
        raise ValueError("y_mix must be (2, L) samples")
    L, H = y.shape[1], n_fft // 2
    T = -(-L // H)
    plan = MVDRPlan(n_fft=n_fft, fs=fs, sigma=sigma, mic_d=mic_d, c_sound=c_sound,
                    angle_deg=angle, mask="external", postfilter="floor", pf_floor=pf_floor,
                    normalize="none", max_batch=1, max_samples=max(T * H, n_fft))
    dev = torch.device(device)
    x = torch.from_numpy(np.pad(y, [(0, 0), (0, T * H - L)]))[None].to(dev)
    hist_bins = mask_kw.pop("hist_bins", 65)
    bb = StreamingBlindBeamformer(plan, 1, forget, hist_bins, hist_forget, dev, **mask_kw)
    sw = None
    if dereverb:
        from .dereverb import StreamingWPE
        sw = StreamingWPE(plan, 1, device=dev, **(wpe_kw or {}))
    outs = []
    for j0 in range(0, T, hops_per_push):
        blk = x[:, :, j0 * H:min(j0 + hops_per_push, T) * H].contiguous()
        outs.append(bb.push(sw.push(blk) if sw else blk))
    if sw:
        outs.append(bb.push(sw.flush()))
    outs.append(bb.flush())
    lag = 2 * H if sw else H
    return torch.cat(outs, dim=1)[0, lag:lag + L].cpu().numpy()
