"""Host-side plan objects over the C ABI (device memory and streams from PyTorch-ROCm).

``MVDRPlan`` is the batched form of the reference's per-utterance chain
(rt_av_zoom/core/oracle_debug.py:42-94, rt_av_zoom/core/masked_mvdr.py:76-128,
rt_av_zoom/core/full_audio_generating_pipeline/inference.py:88-118): one call runs
STFT -> mask -> masked covariance -> MVDR -> apply/post-filter -> iSTFT (-> peak
normalisation) for a whole batch of utterances in one chain of kernel launches (analysis, solve, synthesis, finalize).

Every tensor argument is checked by avz/_args.py before its address goes to the library:
dtype, shape, strides, and that it lives on the device of the call's first tensor.
"""
from __future__ import annotations

import ctypes as ct
from dataclasses import dataclass, field

import torch

from . import _args as A
from . import _lib
from ._args import ANY, FULL, ge, ptr, tensor
from ._lib import AvzBatchArgs, AvzConfig, AvzStreamArgs, check, lib

F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
C64, C128 = torch.complex64, torch.complex128

MASKS = {"ibm": _lib.MASK_IBM, "ipd": _lib.MASK_IPD, "external": _lib.MASK_EXTERNAL,
         "ones": _lib.MASK_ONES}
POSTFILTERS = {"none": _lib.PF_NONE, "ibm": _lib.PF_IBM_TARGET, "floor": _lib.PF_EXT_FLOOR,
               "mul": _lib.PF_EXT_MUL, "irm": _lib.PF_IRM}
FALLBACKS = {"mic0": _lib.FALLBACK_MIC0, "mean": _lib.FALLBACK_MEAN,
             "batch": _lib.FALLBACK_BATCH}
NORMS = {"none": _lib.NORM_NONE, "peak": _lib.NORM_PEAK}
BEAMFORMERS = {"mvdr": _lib.BF_MVDR, "hybrid_null": _lib.BF_HYBRID_NULL}


def n_frames(length: int, hop: int) -> int:
    """scipy.signal.stft frame count with boundary='zeros', padded=True."""
    return -(-length // hop) + 1


def out_length(length: int, hop: int) -> int:
    """scipy.signal.istft output length for an utterance of ``length`` samples."""
    return (n_frames(length, hop) - 1) * hop


@dataclass
class PlanConfig:
    n_fft: int = 1024
    fs: int = 16000
    sigma: float = 1.0
    angle_deg: float = 90.0
    mic_d: float = 0.01
    c_sound: float = 343.0
    fmin_hz: float = 100.0
    mask: str = "ibm"
    postfilter: str = "ibm"
    pf_floor: float = 0.05
    weight_eps: float = 0.0
    normalize: str = "peak"
    norm_eps: float = 0.0
    max_batch: int = 1
    max_samples: int = 64000
    beamformer: str = "mvdr"
    bypass_hz: float = 200.0
    cond_max: float = 10.0
    singular_fallback: str = "mic0"
    # AVZ_MASK_IBM: certificate constant of the reference-exact decisions (include/avz.h
    # avz_config.ibm_kappa): 0 = the library default, < 0 = fp32 decisions only
    ibm_kappa: float = 0.0
    extra: dict = field(default_factory=dict)


_stream_handle = A.stream_handle   # the name other code imports


class MVDRPlan:
    """Immutable engine configuration + device workspace (libavz plan)."""

    def __init__(self, cfg: PlanConfig | None = None, **kw):
        cfg = cfg or PlanConfig()
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown plan option {k!r}")
            setattr(cfg, k, v)
        self.cfg = cfg
        c = AvzConfig()
        c.fs, c.n_fft, c.hop = cfg.fs, cfg.n_fft, cfg.n_fft // 2
        c.sigma, c.angle_deg, c.mic_d = cfg.sigma, cfg.angle_deg, cfg.mic_d
        c.c_sound, c.fmin_hz = cfg.c_sound, cfg.fmin_hz
        c.mask_mode = MASKS[cfg.mask]
        c.postfilter = POSTFILTERS[cfg.postfilter]
        c.pf_floor, c.weight_eps = cfg.pf_floor, cfg.weight_eps
        c.normalize, c.norm_eps = NORMS[cfg.normalize], cfg.norm_eps
        c.max_batch, c.max_samples = cfg.max_batch, cfg.max_samples
        c.beamformer = BEAMFORMERS[cfg.beamformer]
        c.bypass_hz, c.cond_max = cfg.bypass_hz, cfg.cond_max
        c.singular_fallback = FALLBACKS[cfg.singular_fallback]
        c.ibm_kappa = cfg.ibm_kappa
        h = ct.c_void_p()
        check(lib.avz_plan_create(ct.byref(h), ct.byref(c)), "avz_plan_create")
        self._h = h
        self.hop = cfg.n_fft // 2
        self.F = cfg.n_fft // 2 + 1

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            lib.avz_plan_destroy(h)
            self._h = None

    # ------------------------------------------------------------------ diagnostics
    KERNELS = ("analysis", "solve", "synthesis", "finalize")

    def set_timing(self, enable: bool = True, analysis_only: bool = False,
                   period: int = 1) -> None:
        """Time each of the chain's four kernels with HIP events carried by their dispatches
        (analysis_only: the analysis kernel alone) on one run() in `period`."""
        mode = (2 if analysis_only else 1) if enable else 0
        check(lib.avz_plan_set_timing_period(self._h, int(period)), "avz_plan_set_timing_period")
        check(lib.avz_plan_set_timing(self._h, mode), "avz_plan_set_timing")

    def set_ibm_stats(self, counts) -> None:
        """Diagnostics of the exact IBM path: every later run() adds to counts[0] the frames
        and to counts[1] the (bin, frame) decisions taken there (a zeroed int64 CUDA tensor of
        2 elements; None = off)."""
        if counts is not None:
            assert counts.dtype == torch.int64 and counts.is_cuda and counts.numel() >= 2
        check(lib.avz_plan_set_ibm_stats(self._h, ptr(counts)), "avz_plan_set_ibm_stats")
        self._ibm_stats = counts  # keep the buffer alive

    def set_diagnostics(self, synth_variant: int = 2, ipf_mode: int = 0) -> None:
        """Kernel-path A/B of this plan's later runs (tests / tools; include/avz.h
        avz_plan_set_diagnostics): synth_variant 2 = per-utterance synthesis solving its own
        bins (default), 1 = after the solve kernel, 0 = chunk grid + finalize; ipf_mode 1 / 2
        force the in-kernel piece finalize's rare paths."""
        check(lib.avz_plan_set_diagnostics(self._h, int(synth_variant), int(ipf_mode)),
              "avz_plan_set_diagnostics")

    def timing(self) -> dict:
        """Average ms per kernel over the runs since set_timing(True) (waits for them;
        NaN for kernels not timed)."""
        ms = (ct.c_double * 4)()
        n = ct.c_int()
        check(lib.avz_plan_get_timing(self._h, ms, ct.byref(n)), "avz_plan_get_timing")
        return {"calls": n.value, **{k: ms[i] for i, k in enumerate(self.KERNELS)}}

    # ------------------------------------------------------------------ helpers
    def frames(self, length: int) -> int:
        return check(lib.avz_num_frames(self._h, int(length)), "avz_num_frames")

    def out_len(self, length: int) -> int:
        return out_length(length, self.hop)

    def alloc_out(self, batch: int, max_len: int, device) -> torch.Tensor:
        n = self.out_len(max_len)
        return torch.empty((batch, (n + 3) // 4 * 4), dtype=torch.float32, device=device)

    # ------------------------------------------------------------------ batch call
    def workspace_bytes(self, batch: int, max_len: int) -> int:
        """Device bytes of a per-call workspace (avz_mvdr_workspace_bytes)."""
        return check(lib.avz_mvdr_workspace_bytes(self._h, int(batch), int(max_len)),
                     "avz_mvdr_workspace_bytes")

    def alloc_workspace(self, batch: int, max_len: int, device) -> torch.Tensor:
        """A per-call workspace: calls given distinct workspaces may overlap on different
        streams (include/avz.h); calls without one share the plan's and must not."""
        n = self.workspace_bytes(batch, max_len)
        return torch.empty((max(n, 1) + 255) // 256 * 256, dtype=torch.uint8, device=device)

    def _batch_args(self, mix, lengths, max_len, ref_tgt, ref_int, ext_mask, out, peak,
                    cov_out, w_out, workspace, need_out=True):
        """Validated avz_batch_args of a time-domain call (shared by run and the stages)."""
        B, S, dev = A.mic_pair("mix", mix)
        lengths, max_len = A.lengths(lengths, max_len, B, S, dev)
        if max_len > S:
            raise ValueError(f"max_len {max_len} exceeds the {S} samples of mix")
        a = AvzBatchArgs()
        rows = ge(B)
        if need_out:
            if out is None:
                out = self.alloc_out(B, max_len, dev)
            else:
                # at least out_len(max_len) samples a row
                tensor("out", out, F32, (rows, ge(-(-max_len // self.hop) * self.hop)), dev)
            if peak is None:
                peak = torch.empty((B,), dtype=torch.float32, device=dev)
            else:
                tensor("peak", peak, F32, rows, dev, FULL)
            a.out = out.data_ptr()
            a.out_stride = out.stride(0)
            a.peak = peak.data_ptr()
        a.batch = B
        a.len = lengths.data_ptr()
        a.max_len = max_len
        a.mix = mix.data_ptr()
        a.mix_stride = mix.stride(0)
        a.ch_stride = mix.stride(1)
        ref = None if ref_tgt is None and ref_int is None else (rows, ge(max_len))
        if ref_tgt is not None:
            tensor("ref_tgt", ref_tgt, F32, ref, dev)
            a.ref_tgt = ref_tgt.data_ptr()
            a.ref_stride = ref_tgt.stride(0)
        if ref_int is not None:
            tensor("ref_int", ref_int, F32, ref, dev)
            a.ref_int = ref_int.data_ptr()
            if ref_tgt is not None and ref_int.stride(0) != ref_tgt.stride(0):
                raise ValueError("ref_tgt and ref_int must share a stride")
        if ext_mask is not None:
            tensor("ext_mask", ext_mask, F32, (rows, ge(self.F), ge(self.frames(max_len))), dev,
                   ANY)
            a.ext_mask = ext_mask.data_ptr()
            a.mask_stride_b, a.mask_stride_f, a.mask_stride_t = ext_mask.stride()
            a.mask_bins, a.mask_frames = ext_mask.shape[1], ext_mask.shape[2]
        if cov_out is not None:
            tensor("cov_out", cov_out, F64, ge(B * self.F * 5), dev, FULL)
            a.cov_out = cov_out.data_ptr()
        if w_out is not None:
            tensor("w_out", w_out, F32, ge(B * self.F * 4), dev, FULL)
            a.w_out = w_out.data_ptr()
        if workspace is not None:
            tensor("workspace", workspace, U8, ge(0), dev, ANY)
            a.workspace = workspace.data_ptr()
            a.workspace_bytes = workspace.numel()
        return a, out, peak

    def run(self, mix: torch.Tensor, lengths: torch.Tensor | None = None, *,
            max_len: int | None = None, ref_tgt=None, ref_int=None, ext_mask=None,
            out: torch.Tensor | None = None, peak: torch.Tensor | None = None,
            cov_out=None, w_out=None, workspace: torch.Tensor | None = None, stream=None):
        """mix: [B, 2, S] float32 (device); lengths: [B] int32 (device, default S).
        ref_tgt/ref_int: [B, S] (IBM); ext_mask: [B, F, T] target probability (EXTERNAL).
        workspace: optional uint8 device tensor of >= workspace_bytes(B, max_len) bytes.
        Returns (out [B, >= out_len], peak [B])."""
        a, out, peak = self._batch_args(mix, lengths, max_len, ref_tgt, ref_int, ext_mask, out,
                                        peak, cov_out, w_out, workspace)
        A.call("avz_mvdr_batch", self._h, ct.byref(a), stream=stream)
        return out, peak

    # ------------------------------------------------------------------ stage exports
    def covariance(self, mix, lengths=None, *, max_len=None, ref_tgt=None, ref_int=None,
                   ext_mask=None, cov_out=None, workspace=None, stream=None) -> torch.Tensor:
        """STFT -> mask -> masked covariance sums (avz_mvdr_covariance): [B, F, 5] float64
        (sum m|y0|^2, sum m|y1|^2, Re/Im sum m y0 conj(y1), sum m); oracle_debug.py:42-64."""
        B = mix.shape[0]
        if cov_out is None:
            cov_out = torch.empty((B, self.F, 5), dtype=torch.float64, device=mix.device)
        # no out, no peak: the sums are this call's only output
        a, _, _ = self._batch_args(mix, lengths, max_len, ref_tgt, ref_int, ext_mask, None, None,
                                   cov_out, None, workspace, need_out=False)
        A.call("avz_mvdr_covariance", self._h, ct.byref(a), stream=stream)
        return cov_out

    def solve_covariance(self, cov: torch.Tensor, *, steer=None, w=None, fallback=None,
                         stream=None) -> torch.Tensor:
        """Covariance sums [B, F, 5] float64 -> weights [B, F, 4] float32 (Re w0, Im w0,
        Re w1, Im w1) with the plan's beamformer (avz_solve_covariance; oracle_debug.py:66-79).
        steer: optional [F, 2] complex128 device tensor; fallback: optional [B] int32."""
        tensor("cov", cov, F64, (None, self.F, 5), "cuda", FULL)
        B, dev = cov.shape[0], cov.device
        if w is None:
            w = torch.empty((B, self.F, 4), dtype=torch.float32, device=dev)
        else:
            tensor("w", w, F32, ge(B * self.F * 4), dev, ANY)
        A.call("avz_solve_covariance", self._h, B, ptr(cov), ptr(w), self._steer_ptr(steer, dev),
               self._fallback_ptr(fallback, B, dev), stream=stream)
        return w

    def apply_istft(self, mix, w: torch.Tensor, lengths=None, *, max_len=None, gain=None,
                    out=None, peak=None, workspace=None, stream=None):
        """STFT of mix -> S = w^H y (x gain [B, F, T] when given) -> iSTFT/OLA
        (avz_apply_istft; oracle_debug.py:80-94). Returns (out, peak)."""
        a, out, peak = self._batch_args(mix, lengths, max_len, None, None, gain, out, peak, None,
                                        None, workspace)
        tensor("w", w, F32, ge(a.batch * self.F * 4), mix.device, FULL)
        A.call("avz_apply_istft", self._h, ct.byref(a), ptr(w), stream=stream)
        return out, peak

    # ------------------------------------------------------------------ spectral domain
    def _steer_ptr(self, steer, dev):
        if steer is not None:
            tensor("steer", steer, C128, (self.F, 2), dev, FULL)
        return ptr(steer)

    def _fallback_ptr(self, fallback, B, dev):
        if fallback is not None:
            tensor("fallback", fallback, I32, ge(B), dev, ANY)
        return ptr(fallback)

    def beamform_spectral(self, Y: torch.Tensor, mask: torch.Tensor, *, steer=None, S=None,
                          cov_out=None, w_out=None, fallback=None, stream=None) -> torch.Tensor:
        """Y [B, 2, F, T] complex64, mask [B, F, T] float32 target probability -> S [B, F, T]
        complex64 (avz_beamform_spectral: batch_mvdr or hybrid_hard_null_bf per the plan's
        beamformer, the plan's post-filter fused)."""
        tensor("Y", Y, C64, (None, 2, self.F, None), "cuda")
        B, _, _, T = Y.shape
        dev = Y.device
        tensor("mask", mask, F32, (B, self.F, T), dev)
        if S is None:
            S = torch.empty((B, self.F, T), dtype=torch.complex64, device=dev)
        else:
            tensor("S", S, C64, (B, self.F, T), dev)
        A.outputs((("cov_out", cov_out, ge(B * self.F * 5), F64),
                   ("w_out", w_out, ge(B * self.F * 4), F32)), dev)
        a = _lib.AvzSpectralArgs()
        a.batch, a.frames = B, T
        a.Y = ptr(Y)
        a.y_stride_b, a.y_stride_m, a.y_stride_f = Y.stride(0), Y.stride(1), Y.stride(2)
        a.mask = ptr(mask)
        a.mask_stride_b, a.mask_stride_f = mask.stride(0), mask.stride(1)
        a.steer = self._steer_ptr(steer, dev)
        a.S = ptr(S)
        a.s_stride_b, a.s_stride_f = S.stride(0), S.stride(1)
        a.cov_out, a.w_out = ptr(cov_out), ptr(w_out)
        a.fallback = self._fallback_ptr(fallback, B, dev)
        A.call("avz_beamform_spectral", self._h, ct.byref(a), stream=stream)
        return S

    def istft(self, S: torch.Tensor, *, out=None, peak=None, workspace=None, stream=None):
        """scipy.signal.istft(S, nperseg=n_fft, noverlap=n_fft/2) of S [B, F, T] complex64
        (t contiguous): (out [B, >= (T - 1) hop], peak [B]); the plan's normalisation applies."""
        tensor("S", S, C64, (None, self.F, None), "cuda")
        B, _, T = S.shape
        dev = S.device
        n = (T - 1) * self.hop
        if out is None:
            out = torch.empty((B, (n + 3) // 4 * 4), dtype=torch.float32, device=dev)
        else:
            tensor("out", out, F32, (ge(B), ge(n)), dev)
        if peak is None:
            peak = torch.empty((B,), dtype=torch.float32, device=dev)
        else:
            tensor("peak", peak, F32, ge(B), dev, ANY)
        if workspace is not None:
            tensor("workspace", workspace, U8, ge(0), dev, ANY)
        A.call("avz_istft", self._h, B, T, ptr(S), S.stride(0), S.stride(1), ptr(out),
               out.stride(0), ptr(peak), ptr(workspace),
               0 if workspace is None else workspace.numel(), stream=stream)
        return out, peak

    def stft(self, x: torch.Tensor, lengths: torch.Tensor | None = None, max_len=None,
             stream=None) -> torch.Tensor:
        """scipy.signal.stft(x, fs, nperseg=n_fft, noverlap=n_fft//2) for x [B, C, S]
        (C in {1, 2}); returns complex64 [B, C, F, T]."""
        tensor("x", x, F32, (None, None, None), "cuda")
        B, Cn, S = x.shape
        lengths, max_len = A.lengths(lengths, max_len, B, S, x.device)
        T = n_frames(max_len, self.hop)
        Y = torch.zeros((B, Cn, self.F, T), dtype=torch.complex64, device=x.device)
        A.call("avz_stft", self._h, B, Cn, ptr(lengths), max_len, ptr(x), x.stride(0),
               x.stride(1), ptr(Y), Y.stride(0), Y.stride(1), Y.stride(2), stream=stream)
        return Y


FEATURE_LAYOUTS = {"unet": _lib.FEAT_LOGMAG_IPD, "tflite": _lib.FEAT_TFLITE}


def mask_features(plan: MVDRPlan, x: torch.Tensor, layout: str = "unet", lengths=None,
                  max_len=None, stream=None) -> torch.Tensor:
    """Mask-model input features of a [B, 2, S] mic pair (avz_mask_features):
    layout "unet"   -> [B, 2, F, T]: log(|Y0| + 1e-7), angle(Y0) - angle(Y1)
                       (full_audio_generating_pipeline/inference.py:90-94);
    layout "tflite" -> [B, F, T, 4]: log_mag, sin(ipd), cos(ipd), linspace(0, 1, F)
                       (Final_pipeline/src/inference.py:198-203, 117-128)."""
    B, S, dev = A.mic_pair("x", x)
    lengths, max_len = A.lengths(lengths, max_len, B, S, dev)
    out, strides = A.features(layout, B, plan.F, n_frames(max_len, plan.hop), dev)
    A.call("avz_mask_features", plan._h, FEATURE_LAYOUTS[layout], B, ptr(lengths), max_len,
           ptr(x), x.stride(0), x.stride(1), ptr(out), *strides, stream=stream)
    return out


def mask_training_batch(plan: MVDRPlan, mix: torch.Tensor, tgt: torch.Tensor, itf: torch.Tensor,
                        layout: str = "unet", lengths=None, max_len=None, stream=None):
    """One training batch of the mask estimator in one kernel (avz_mask_training_batch):
    (feat, label) of a [B, 2, S] mic pair and its [B, S] target / interference references.
    feat: the bits mask_features(plan, mix, layout) returns; label [B, F, T] float32, 1.0
    where |STFT(tgt)| > |STFT(itf)| on the kernel's fp32 transforms, else 0.0
    (full_audio_generating_pipeline/model_training.py:80-92). Frames past an item's length
    stay 0."""
    B, S, dev = A.mic_pair("mix", mix)
    tensor("tgt", tgt, F32, (B, S), dev)
    tensor("itf", itf, F32, (B, S), dev)
    if itf.stride(0) != tgt.stride(0):
        # the kernel takes one row stride for both: copies here, where stream_push raises
        itf = itf.contiguous()
        tgt = tgt.contiguous()
    lengths, max_len = A.lengths(lengths, max_len, B, S, dev)
    T = n_frames(max_len, plan.hop)
    feat, strides = A.features(layout, B, plan.F, T, dev)
    label = torch.zeros((B, plan.F, T), dtype=torch.float32, device=dev)
    A.call("avz_mask_training_batch", plan._h, FEATURE_LAYOUTS[layout], B, ptr(lengths), max_len,
           ptr(mix), mix.stride(0), mix.stride(1), ptr(tgt), ptr(itf), tgt.stride(0),
           ptr(feat), *strides, ptr(label), *label.stride(), stream=stream)
    return feat, label


# ------------------------------------------------------------------ streaming entry points
# Thin wrappers over avz_stream_* (causal MVDR), avz_wpe_stream_* (online WPE) and
# avz_delay_stream_* (blind delay mask; include/avz.h). avz/stream.py StreamingBeamformer and
# StreamingDelayMask and avz/dereverb.py StreamingWPE own the state buffers and are the
# interfaces to use.
def _state_args(state, streams, select, name="select", dtype=I32):
    """(state pointer, its bytes, streams, select pointer) of a *_stream_reset / _steer:
    state a uint8 device buffer, select (or the angles) one entry per stream on its device."""
    tensor("state", state, U8, ge(0), "cuda", ANY)
    if select is not None:
        tensor(name, select, dtype, ge(int(streams)), state.device, ANY)
    return ptr(state), state.numel(), int(streams), ptr(select)


def _push_args(a, plan, state, mix, forget, active, adapt):
    """Fill what every *_stream_push takes of a hop block (streams, hops, forget, flags, mix,
    state): returns (streams, hops, the block's device)."""
    streams, hops = A.hop_block(mix, plan.hop)
    dev = mix.device
    tensor("state", state, U8, ge(0), dev, ANY)
    for name, t in (("active", active), ("adapt", adapt)):
        if t is not None:
            tensor(name, t, I32, ge(streams), dev, ANY)
    a.streams, a.hops, a.forget = streams, hops, float(forget)
    a.active, a.adapt = ptr(active), ptr(adapt)
    a.mix, a.mix_stride, a.ch_stride = ptr(mix), mix.stride(0), mix.stride(1)
    a.state, a.state_bytes = ptr(state), state.numel()
    return streams, hops, dev


def stream_state_bytes(plan: MVDRPlan, streams: int) -> int:
    return check(lib.avz_stream_state_bytes(plan._h, int(streams)), "avz_stream_state_bytes")


def stream_reset(plan: MVDRPlan, state: torch.Tensor, streams: int, select=None, stream=None):
    """Zero the selected streams (select: int32 [streams] device tensor, None = all) and give
    them the plan's steering table."""
    A.call("avz_stream_reset", plan._h, *_state_args(state, streams, select), stream=stream)


def stream_steer(plan: MVDRPlan, state: torch.Tensor, streams: int, angles: torch.Tensor,
                 stream=None):
    """angles: float64 [streams] device tensor, degrees; NaN keeps a stream's direction."""
    A.call("avz_stream_steer", plan._h, *_state_args(state, streams, angles, "angles", F64),
           stream=stream)


def stream_push(plan: MVDRPlan, state: torch.Tensor, mix: torch.Tensor, out: torch.Tensor, *,
                forget: float = 1.0, ref_tgt=None, ref_int=None, mask=None, active=None,
                adapt=None, w_out=None, cov_out=None, mask_out=None, stream=None):
    """One avz_stream_push: mix [streams, 2, hops * hop] -> out [streams, hops * hop] (float32
    device tensors, samples contiguous). mask [streams, F, hops] (external plans), ref_tgt /
    ref_int [streams, hops * hop] sharing a row stride (IBM plans); active / adapt int32
    [streams]; w_out [streams, F, 4] float32, cov_out [streams, F, 5] float64 and mask_out
    [streams, F, hops] float32 contiguous."""
    a = AvzStreamArgs()
    streams, hops, dev = _push_args(a, plan, state, mix, forget, active, adapt)
    n, F = hops * plan.hop, plan.F
    tensor("out", out, F32, (streams, n), dev)
    if ref_tgt is not None or ref_int is not None:
        for name, r in (("ref_tgt", ref_tgt), ("ref_int", ref_int)):
            if r is None:
                raise ValueError(f"{name} must be given with the other reference")
            tensor(name, r, F32, (streams, n), dev)
        if ref_int.stride(0) != ref_tgt.stride(0):
            raise ValueError("ref_tgt and ref_int must share a stride")
        a.ref_tgt, a.ref_int, a.ref_stride = ptr(ref_tgt), ptr(ref_int), ref_tgt.stride(0)
    if mask is not None:
        tensor("mask", mask, F32, (streams, F, hops), dev, ANY)
        a.ext_mask = ptr(mask)
        a.mask_stride_b, a.mask_stride_f, a.mask_stride_t = mask.stride()
    a.out, a.out_stride = ptr(out), out.stride(0)
    A.outputs((("w_out", w_out, (streams, F, 4), F32), ("cov_out", cov_out, (streams, F, 5), F64),
               ("mask_out", mask_out, (streams, F, hops), F32)), dev)
    a.w_out, a.cov_out, a.mask_out = ptr(w_out), ptr(cov_out), ptr(mask_out)
    A.call("avz_stream_push", plan._h, ct.byref(a), stream=stream)
    return out


def wpe_stream_state_bytes(plan: MVDRPlan, streams: int, taps: int = 10, delay: int = 3) -> int:
    return check(lib.avz_wpe_stream_state_bytes(plan._h, int(streams), int(taps), int(delay)),
                 "avz_wpe_stream_state_bytes")


def wpe_stream_reset(plan: MVDRPlan, state: torch.Tensor, streams: int, taps: int = 10,
                     delay: int = 3, q_init: float = 1.0, select=None, stream=None):
    """Start the selected streams (select: int32 [streams] device tensor, None = all): zero
    history, G = 0, Q = q_init I; fixes the buffer's taps and delay."""
    p, nbytes, streams, sel = _state_args(state, streams, select)
    A.call("avz_wpe_stream_reset", plan._h, p, nbytes, streams, int(taps), int(delay),
           float(q_init), sel, stream=stream)


def wpe_stream_push(plan: MVDRPlan, state: torch.Tensor, mix: torch.Tensor, out: torch.Tensor, *,
                    taps: int = 10, delay: int = 3, forget: float = 0.99,
                    power_floor: float = 1e-9, active=None, adapt=None, Y_out=None, Z_out=None,
                    G_out=None, stream=None):
    """One avz_wpe_stream_push: mix [streams, 2, hops * hop] -> out of the same shape (float32
    device tensors, samples contiguous). active / adapt int32 [streams]; Y_out / Z_out
    complex64 [streams, 2, F, hops] and G_out complex128 [streams, F, 2 taps, 2], contiguous."""
    a = _lib.AvzWpeStreamArgs()
    streams, hops, dev = _push_args(a, plan, state, mix, forget, active, adapt)
    tensor("out", out, F32, (streams, 2, hops * plan.hop), dev)
    a.taps, a.delay, a.power_floor = int(taps), int(delay), float(power_floor)
    a.out, a.out_stride, a.out_ch_stride = ptr(out), out.stride(0), out.stride(1)
    A.outputs((("Y_out", Y_out, (streams, 2, plan.F, hops), C64),
               ("Z_out", Z_out, (streams, 2, plan.F, hops), C64),
               ("G_out", G_out, (streams, plan.F, 2 * int(taps), 2), C128)), dev)
    a.Y_out, a.Z_out, a.G_out = ptr(Y_out), ptr(Z_out), ptr(G_out)
    A.call("avz_wpe_stream_push", plan._h, ct.byref(a), stream=stream)
    return out


def delay_mask_workspace_bytes(plan: MVDRPlan, batch: int, max_len: int,
                               hist_bins: int = 65) -> int:
    return check(lib.avz_delay_mask_workspace_bytes(plan._h, int(batch), int(max_len),
                                                    int(hist_bins)),
                 "avz_delay_mask_workspace_bytes")


def _delay_params(a, angles, hist_bins, smooth, rel_height, min_sep, max_peaks, f_lo):
    """The histogram and peak-picking fields avz_delay_mask and avz_delay_stream_push share."""
    a.angle_deg = ptr(angles)
    a.hist_bins, a.smooth, a.max_peaks = int(hist_bins), int(smooth), int(max_peaks)
    a.rel_height, a.min_sep, a.f_lo_hz = float(rel_height), float(min_sep), float(f_lo)


def delay_mask(plan: MVDRPlan, mix: torch.Tensor, lengths=None, angles=None, *, hist_bins=65,
               smooth=3, rel_height=0.25, min_sep=0.2, max_peaks=3, f_lo=100.0, max_len=None,
               mask=None, workspace=None, return_debug=False, stream=None):
    """Blind delay-histogram (DUET-style) target mask of a [B, 2, S] mic pair
    (avz_delay_mask; include/avz.h): float32 [B, F, T], the target
    probability an external-mask plan takes as ``ext_mask``. Only the plan's n_fft, fs, mic_d,
    c_sound and angle_deg matter. ``angles``: optional float64 [B] device tensor, the target
    azimuth per utterance. ``mask``: optional output (any strides; frames past an utterance's
    own count and rows shorter than n_fft are left as they are; a new one starts as zeros).
    ``workspace``: optional uint8 device tensor of delay_mask_workspace_bytes(...) bytes (one
    is allocated otherwise). With ``return_debug`` also returns hist [B, hist_bins] float64
    (before smoothing), delays [B, 8] float64 (delta_t, the kept delays, NaN) and n_peaks [B]
    int32 (-1: row shorter than n_fft)."""
    B, S, dev = A.mic_pair("mix", mix)
    lengths, max_len = A.lengths(lengths, max_len, B, S, dev, FULL)
    if angles is not None:
        tensor("angles", angles, F64, ge(B), dev, FULL)
    T = n_frames(max_len, plan.hop)
    if mask is None:
        # a new batch mask starts as zeros: the kernel leaves frames past a row's own count
        mask = torch.zeros((B, plan.F, T), dtype=torch.float32, device=dev)
    else:
        tensor("mask", mask, F32, (B, ge(plan.F), ge(T)), dev, ANY)
    ws = workspace
    if ws is None:
        # this wrapper allocates its own workspace and keeps it alive on the call's stream
        ws = torch.empty(delay_mask_workspace_bytes(plan, B, max_len, hist_bins),
                         dtype=torch.uint8, device=dev)
    else:
        tensor("workspace", ws, U8, ge(0), dev, FULL)
    a = _lib.AvzDelayMaskArgs()
    a.batch, a.len, a.max_len = B, ptr(lengths), max_len
    a.mix, a.mix_stride, a.ch_stride = ptr(mix), mix.stride(0), mix.stride(1)
    _delay_params(a, angles, hist_bins, smooth, rel_height, min_sep, max_peaks, f_lo)
    a.mask = ptr(mask)
    a.mask_stride_b, a.mask_stride_f, a.mask_stride_t = mask.stride()
    hist = delays = n_peaks = None
    if return_debug:
        hist = torch.zeros((B, int(hist_bins)), dtype=torch.float64, device=dev)
        delays = torch.full((B, 8), float("nan"), dtype=torch.float64, device=dev)
        n_peaks = torch.zeros(B, dtype=torch.int32, device=dev)
        a.hist_out, a.delays_out, a.n_peaks = ptr(hist), ptr(delays), ptr(n_peaks)
    a.workspace, a.workspace_bytes = ptr(ws), ws.numel()
    A.call("avz_delay_mask", plan._h, ct.byref(a), stream=stream, device=dev)
    if workspace is None:
        ws.record_stream(stream if stream is not None else torch.cuda.current_stream(dev))
    out = mask[:, :plan.F, :T]
    return (out, hist, delays, n_peaks) if return_debug else out


def delay_stream_state_bytes(plan: MVDRPlan, streams: int, hist_bins: int = 65) -> int:
    return check(lib.avz_delay_stream_state_bytes(plan._h, int(streams), int(hist_bins)),
                 "avz_delay_stream_state_bytes")


def delay_stream_reset(plan: MVDRPlan, state: torch.Tensor, streams: int, hist_bins: int = 65,
                       select=None, stream=None):
    """Start the selected streams (select: int32 [streams] device tensor, None = all): zero
    history, h = 0; fixes the buffer's hist_bins."""
    p, nbytes, streams, sel = _state_args(state, streams, select)
    A.call("avz_delay_stream_reset", plan._h, p, nbytes, streams, int(hist_bins), sel,
           stream=stream)


def delay_stream_push(plan: MVDRPlan, state: torch.Tensor, mix: torch.Tensor, mask=None, *,
                      forget: float = 1.0, angles=None, active=None, adapt=None, hist_bins=65,
                      smooth=3, rel_height=0.25, min_sep=0.2, max_peaks=3, f_lo=100.0,
                      hist_out=None, delays_out=None, n_peaks=None, stream=None):
    """One avz_delay_stream_push: mix [streams, 2, hops * hop] float32 -> mask [streams, F, hops]
    float32 (any strides; a new one starts as ones), the target probability the streaming
    beamformer's push of the same hops takes. angles float64 [streams] (NaN = the plan's);
    active / adapt int32 [streams]; hist_out [streams, hist_bins] float64, delays_out
    [streams, hops, 8] float64 and n_peaks [streams, hops] int32, contiguous."""
    a = _lib.AvzDelayStreamArgs()
    streams, hops, dev = _push_args(a, plan, state, mix, forget, active, adapt)
    if mask is None:
        # a new streaming mask starts as ones (all target): inactive streams keep that
        mask = torch.ones((streams, plan.F, hops), dtype=torch.float32, device=dev)
    else:
        tensor("mask", mask, F32, (streams, plan.F, hops), dev, ANY)
    if angles is not None:
        tensor("angles", angles, F64, (streams,), dev, FULL)
    _delay_params(a, angles, hist_bins, smooth, rel_height, min_sep, max_peaks, f_lo)
    a.mask = ptr(mask)
    a.mask_stride_b, a.mask_stride_f, a.mask_stride_t = mask.stride()
    A.outputs((("hist_out", hist_out, (streams, int(hist_bins)), F64),
               ("delays_out", delays_out, (streams, hops, 8), F64),
               ("n_peaks", n_peaks, (streams, hops), I32)), dev)
    a.hist_out, a.delays_out, a.n_peaks = ptr(hist_out), ptr(delays_out), ptr(n_peaks)
    A.call("avz_delay_stream_push", plan._h, ct.byref(a), stream=stream, device=dev)
    return mask


def srp_scan(plan: MVDRPlan, mix: torch.Tensor, lengths=None, max_len=None, n_angles=181,
             angle_lo=0.0, angle_hi=180.0, f_lo=200.0, f_hi=4000.0, stream=None):
    """scripts/debug_srp.py:46-62 for a [B, 2, S] batch -> power map [B, n_angles] in dB
    relative to each utterance's maximum (float64, device)."""
    B, S, dev = A.mic_pair("mix", mix)
    lengths, max_len = A.lengths(lengths, max_len, B, S, dev)
    out = torch.empty((B, n_angles), dtype=torch.float64, device=dev)
    A.call("avz_srp_scan", plan._h, B, ptr(lengths), max_len, ptr(mix), mix.stride(0),
           mix.stride(1), n_angles, float(angle_lo), float(angle_hi), float(f_lo), float(f_hi),
           ptr(out), stream=stream)
    return out


def wpe_spectral(Y: torch.Tensor, taps: int = 10, delay: int = 3, iterations: int = 3,
                 frames=None, out=None, status=None, stream=None) -> torch.Tensor:
    """WPE dereverberation of Y [B, 2, F, T] complex64 (t contiguous) -> Z of the same shape
    (avz_wpe_spectral; rt_av_zoom/core/dereverb.py:76-78 per item). ``frames``: optional
    int32 [B] valid frames per item (frames beyond it are copied); ``out`` may be Y itself;
    ``status``: optional int32 [B, F] (0 dereverberated, 1 / 2 passed through)."""
    tensor("Y", Y, C64, (None, 2, None, None), "cuda")
    B, _, F, T = Y.shape
    dev = Y.device
    if out is None:
        out = torch.empty((B, 2, F, T), dtype=torch.complex64, device=dev)
    else:
        tensor("out", out, C64, (B, 2, F, T), dev)
    A.outputs((("frames", frames, ge(B), I32), ("status", status, ge(B * F), I32)), dev)
    a = _lib.AvzWpeArgs()
    a.batch, a.bins, a.frames = B, F, T
    a.frames_b = ptr(frames)
    a.taps, a.delay, a.iterations = int(taps), int(delay), int(iterations)
    a.Y = ptr(Y)
    a.y_stride_b, a.y_stride_m, a.y_stride_f = Y.stride(0), Y.stride(1), Y.stride(2)
    a.Z = ptr(out)
    a.z_stride_b, a.z_stride_m, a.z_stride_f = out.stride(0), out.stride(1), out.stride(2)
    a.status = ptr(status)
    A.call("avz_wpe_spectral", ct.byref(a), stream=stream, device=dev)
    return out


def room_rir(room, src_pos, device=None, out=None, stream=None) -> torch.Tensor:
    """Image-source RIRs of a shoebox room (avz_room_rir; synth.room_rir is the host
    restatement): src_pos [B, S, 3] (metres; array or fp64 device tensor) -> fp64
    [B, S, 2, rir_len], one RIR per (utterance, source, mic). ``room``: synth.Room."""
    import numpy as np

    from .synth import _room_struct
    r = _room_struct(room)
    L = check(lib.avz_room_rir_len(ct.byref(r)), "avz_room_rir_len")
    if not isinstance(src_pos, torch.Tensor):
        dev = device or torch.device("cuda", torch.cuda.current_device())
        src_pos = torch.as_tensor(np.asarray(src_pos, np.float64)).to(dev)
    src_pos = tensor("src_pos", src_pos, F64, (None, None, 3), "cuda", ANY).contiguous()
    B, S, _ = src_pos.shape
    dev = src_pos.device
    if out is None:
        out = torch.empty((B, S, 2, L), dtype=torch.float64, device=dev)
    else:
        tensor("out", out, F64, (B, S, 2, L), dev, FULL)
    A.call("avz_room_rir", ct.byref(r), B, S, ptr(src_pos), ptr(out), stream=stream, device=dev)
    return out
