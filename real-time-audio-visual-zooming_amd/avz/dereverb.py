"""Mirror of rt_av_zoom/core/dereverb.py on the MI355X engine: WPE dereverberation.

``apply_wpe(y_mix)`` is the reference entry point (dereverb.py:26-106): STFT of the two
channels, WPE per bin (``avz_wpe_spectral``, taps=10, delay=3, iterations=3,
psd_context=0, full-frame statistics as dereverb.py:76-78 calls ``nara_wpe.wpe.wpe``),
inverse STFT, trim / zero-pad to the input length (:93-103). ``main(args)`` reads
``<outdir>/mixture.wav`` and writes ``<outdir>/mixture_wpe.wav`` (:108-138), the input of
``avz.oracle_reverb``. ``dereverb_batch`` is the batched device form.

The contract is the algorithm (offline batch WPE, Nakatani et al. 2010) as ``wpe_numpy``
states it in fp64, not bit parity with nara_wpe, which is not installed anywhere this
project is tested. Departures: degenerate bins pass the input through
with a status instead of NaN or an exception, and the framing is the engine's scipy
periodic-Hann STFT / iSTFT, not nara_wpe.utils.stft.

The causal counterpart is at the end of the module: ``StreamingWPE``
(``avz_wpe_stream_push``: recursive-least-squares online WPE, hop by hop over a caller-owned
state buffer), ``apply_wpe_stream`` for a whole file and ``wpe_stream_numpy``, its fp64
restatement.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

FS = 16000
N_FFT = 512
N_HOP = 256
DEFAULT_OUTDIR = "simulation_results/ljspeech_reverb_20251130_215709"

EPS_FLOOR = 1e-10      # lambda = 1 / max(p, EPS_FLOOR * max_t p)


def pivot_threshold(taps: int) -> float:
    """A Cholesky pivot <= this multiple of its original diagonal entry is singular."""
    return (2 * taps + 1) * 2.0 ** -52


def regressor(Y, taps: int, delay: int):
    """Yt [taps * D, T] of Y [D, T]: row tau * D + m at frame t is Y[m, t - delay - tau]."""
    D, T = Y.shape
    Yt = np.zeros((taps * D, T), dtype=Y.dtype)
    for tau in range(taps):
        s = delay + tau
        if s < T:
            Yt[tau * D:(tau + 1) * D, s:] = Y[:, :T - s]
    return Yt


def _cholesky(R, thr):
    """Left-looking Cholesky of a Hermitian R -> (L or None, smallest pivot / R_jj)."""
    n = R.shape[0]
    L = np.zeros_like(R)
    rel = np.inf
    for j in range(n):
        v = R[j:, j] - L[j:, :j] @ L[j, :j].conj()
        d, djj = v[0].real, R[j, j].real
        if not (d > thr * djj) or not np.isfinite(d):
            return None, (d / djj if djj > 0 and np.isfinite(d) else 0.0)
        rel = min(rel, d / djj)
        l = np.sqrt(d)
        L[j, j] = l
        L[j + 1:, j] = v[1:] / l
    return L, rel


def _solve_chol(L, P):
    """G with L L^H G = P."""
    n = L.shape[0]
    Z = np.zeros_like(P)
    for i in range(n):
        Z[i] = (P[i] - L[i, :i] @ Z[:i]) / L[i, i].real
    G = np.zeros_like(P)
    for i in range(n - 1, -1, -1):
        G[i] = (Z[i] - L[i + 1:, i].conj() @ G[i + 1:]) / L[i, i].real
    return G


def wpe_bin(Y, taps=10, delay=3, iterations=3, row_order=None):
    """One bin: Y [D, T] complex -> (X [D, T] complex128, status, smallest relative pivot).
    ``row_order``: an optional permutation of the regressor's rows (X does not depend on it
    beyond rounding)."""
    Y = np.asarray(Y, dtype=np.complex128)
    D, T = Y.shape
    n = taps * D
    if T - delay < n:          # fewer regressor frames than unknowns: by the count alone
        return Y.copy(), 2, np.nan
    Yt = regressor(Y, taps, delay)
    if row_order is not None:
        Yt = Yt[np.asarray(row_order)]
    thr = pivot_threshold(taps)
    X, rel_min = Y.copy(), np.inf
    for _ in range(iterations):
        p = np.mean(X.real ** 2 + X.imag ** 2, axis=0)
        pm = p.max()
        if pm == 0:
            return Y.copy(), 1, rel_min
        lam = 1.0 / np.maximum(p, EPS_FLOOR * pm)
        Yl = Yt * lam
        R = Yl @ Yt.conj().T
        P = Yl @ Y.conj().T
        with np.errstate(invalid="ignore", divide="ignore"):
            L, rel = _cholesky(R, thr)
        if L is None:
            return Y.copy(), 2, rel
        rel_min = min(rel_min, rel)
        G = _solve_chol(L, P)
        X = Y - G.conj().T @ Yt
    return X, 0, rel_min


def wpe_numpy(Y, taps=10, delay=3, iterations=3, frames=None, return_info=False):
    """The algorithm in fp64: Y [2, F, T] complex -> X [2, F, T] complex128 (and, with
    ``return_info``, status [F] and the smallest relative Cholesky pivot per bin). ``frames``:
    only the first ``frames`` frames are processed; the rest are copies of Y."""
    Y = np.asarray(Y)
    _, F, T = Y.shape
    Tb = T if frames is None else max(0, min(int(frames), T))
    X = Y.astype(np.complex128)
    status = np.zeros(F, dtype=np.int32)
    rel = np.full(F, np.nan)
    for k in range(F):
        X[:, k, :Tb], status[k], rel[k] = wpe_bin(Y[:, k, :Tb], taps, delay, iterations)
    return (X, status, rel) if return_info else X


def _plan(n_fft, batch, samples):
    from .engine import MVDRPlan, out_length
    return MVDRPlan(n_fft=n_fft, mask="ones", postfilter="none", normalize="none",
                    max_batch=2 * batch, max_samples=out_length(samples, n_fft // 2))


def dereverb_batch(mix, lengths=None, taps=10, delay=3, iterations=3, n_fft=N_FFT, plan=None,
                   status=None, stream=None):
    """mix [B, 2, S] float32 on the device (lengths: int32 [B] or None = S) -> dereverberated
    [B, 2, S] float32: plan.stft -> avz_wpe_spectral (in place) -> plan.istft per channel,
    trimmed to S; samples at or beyond lengths[b] are zero. ``plan``: an un-normalised
    MVDRPlan of this n_fft with max_batch >= 2 B (made here when None)."""
    import torch
    from . import _args as A
    from .engine import n_frames, wpe_spectral
    B, S, _ = A.mic_pair("mix", mix)
    if plan is None:
        plan = _plan(n_fft, B, S)
    hop = plan.hop
    # wpe_spectral checks status too, but only after plan.stft has launched
    A.outputs((("status", status, A.ge(B * plan.F), torch.int32),), mix.device)
    if lengths is None:
        frames, max_len = None, S
    else:
        lengths, max_len = A.lengths(lengths, None, B, S, mix.device)
        frames = (torch.div(lengths + (hop - 1), hop, rounding_mode="floor") + 1).to(torch.int32)
    Y = plan.stft(mix, lengths, max_len, stream=stream)
    T = n_frames(max_len, hop)
    wpe_spectral(Y, taps, delay, iterations, frames=frames, out=Y, status=status, stream=stream)
    y, _ = plan.istft(Y.view(2 * B, plan.F, T), stream=stream)
    n = min(S, (T - 1) * hop)
    out = torch.zeros((B, 2, S), dtype=torch.float32, device=mix.device)
    out[:, :, :n] = y.view(B, 2, -1)[:, :, :n]
    if lengths is not None:
        out *= (torch.arange(S, device=mix.device)[None, None, :] < lengths[:, None, None])
    return out


def apply_wpe(y_mix, taps=10, delay=3, iterations=3, n_fft=N_FFT, device="cuda"):
    """(Channels, Samples) float32 -> dereverberated (Channels, Samples) float32 numpy
    (dereverb.py:26-106). An input the STFT cannot frame is returned as it is, as the
    reference's error paths do (:37-39)."""
    import torch
    y_mix = np.ascontiguousarray(y_mix, dtype=np.float32)
    print(f"  [WPE] Input Time-Domain Shape: {y_mix.shape}")
    if y_mix.ndim != 2 or y_mix.shape[0] != 2 or y_mix.shape[1] < n_fft:
        print(f"  [Error] STFT failed: need (2, >= {n_fft}) samples")
        return y_mix
    x = torch.from_numpy(y_mix)[None].to(torch.device(device))
    out = dereverb_batch(x, None, taps, delay, iterations, n_fft)[0].cpu().numpy()
    print(f"  [WPE] Output Time-Domain Shape: {out.shape}")
    return out


# ------------------------------------------------------------------ streaming online WPE
# The causal counterpart of the above: recursive-least-squares WPE hop by hop (include/avz.h
# avz_wpe_stream_push). NumpyWPEStream / wpe_stream_numpy restate the
# contract in fp64 (the tests' reference), StreamingWPE drives the device path and
# apply_wpe_stream runs a whole file through it.
def default_power_floor(n_fft: int) -> float:
    """The floor of the frame power that scales the RLS step. Spectra carry the 1 / sum(w)
    scale, under which white noise of variance s^2 has E|Y_k|^2 = s^2 sum(w^2) / sum(w)^2 =
    1.5 s^2 / n_fft for the periodic Hann: the default is that power at s = 1e-3 (-60 dBFS),
    so digital silence and near-silence adapt as slowly as a -60 dBFS noise floor would."""
    return 1.5e-6 / n_fft


class NumpyWPEStream:
    """One stream of online WPE, stateful, every bin at once: push() hops of the two mics, or
    push_spec() one frame Y [2, F]. Arithmetic in ``dtype`` (float64, or numpy.longdouble for
    an error estimate of the fp64 run); the analysis and synthesis transforms are fp64.
    hist["Y"] / hist["Z"]: every frame so far, [2, F]; .G [F, n, 2], .Q [F, n, n]."""

    def __init__(self, n_fft=N_FFT, taps=10, delay=3, forget=0.99, power_floor=None, q_init=1.0,
                 y_hook=None, dtype=np.float64):
        if not 1 <= taps <= 16 or not 1 <= delay <= 8:
            raise ValueError("taps must lie in 1..16 and delay in 1..8")
        if not 0.0 < forget <= 1.0:
            raise ValueError("forget must lie in (0, 1]")
        from .stream import hann_periodic
        self.N, self.H, self.F = n_fft, n_fft // 2, n_fft // 2 + 1
        self.K, self.D, self.n, self.W = taps, delay, 2 * taps, taps + delay + 1
        self.rt = np.dtype(dtype).type
        self.ct = np.result_type(dtype, np.complex64).type
        self.forget = self.rt(forget)
        self.inv_forget = self.rt(1) / self.forget
        floor = default_power_floor(n_fft) if power_floor is None else power_floor
        if not floor > 0 or not q_init > 0:
            raise ValueError("power_floor and q_init must be positive")
        self.floor, self.q_init = self.rt(floor), self.rt(q_init)
        self.win = hann_periodic(n_fft)
        self.win32 = self.win.astype(np.float32).astype(np.float64)
        self.scale = 1.0 / self.win32.sum()
        self.y_hook = y_hook                                          # (t, Y [2, F]) -> Y
        self._low = np.tril(np.ones((self.n, self.n), dtype=bool))
        self.reset()

    def reset(self):
        self.count = 0
        self.prev = np.zeros((2, self.H))
        self.tail = np.zeros((2, self.H))
        self.G = np.zeros((self.F, self.n, 2), dtype=self.ct)
        self.Q = np.zeros((self.F, self.n, self.n), dtype=self.ct)
        self.Q[:, np.arange(self.n), np.arange(self.n)] = self.q_init
        self.hist = {"Y": [], "Z": []}

    def push_spec(self, Y, adapt=True):
        """One frame: Y [2, F] (rounded to complex64) -> Z [2, F] in ``dtype``."""
        t, n, W = self.count, self.n, self.W
        if self.y_hook is not None:
            Y = self.y_hook(t, np.asarray(Y))
        Y = np.asarray(Y).astype(np.complex64).astype(self.ct)
        past = self.hist["Y"]
        yt = np.zeros((self.F, n), dtype=self.ct)
        for tau in range(self.K):
            src = t - self.D - tau
            if src >= 0:
                yt[:, 2 * tau] = past[src][0]
                yt[:, 2 * tau + 1] = past[src][1]
        p = np.zeros(self.F, dtype=self.rt)
        for s in range(t, max(0, t - W + 1) - 1, -1):
            a, b = (Y if s == t else past[s])
            p = p + ((a.real * a.real + a.imag * a.imag) + (b.real * b.real + b.imag * b.imag))
        p = p / self.rt(2 * W)
        Z = Y - np.einsum("fim,fi->mf", self.G.conj(), yt)
        if adapt:
            with np.errstate(all="ignore"):
                u = np.einsum("fij,fj->fi", self.Q, yt)
                den = self.forget * np.maximum(p, self.floor) + \
                    np.sum(yt.real * u.real + yt.imag * u.imag, axis=1)
                k = u / den[:, None]
                self.G = self.G + k[:, :, None] * Z.T.conj()[:, None, :]
                Qn = k[:, :, None] * u.conj()[:, None, :]
                np.subtract(self.Q, Qn, out=Qn)
                Qn *= self.inv_forget
            # the lower triangle, mirrored; a real diagonal
            self.Q = np.where(self._low, Qn, Qn.conj().transpose(0, 2, 1))
            self.Q.imag[:, np.arange(n), np.arange(n)] = 0
        self.hist["Y"].append(Y)
        self.hist["Z"].append(Z)
        self.count += 1
        return Z

    def synth(self, Z):
        """One frame Z [2, F] through the synthesis: the hop that leaves, [2, H]."""
        H = self.H
        first = self.count <= 1          # called after push_spec: frame 0 gives zeros
        g = np.fft.irfft(np.asarray(Z).astype(np.complex128), n=self.N, axis=-1) * \
            self.win.sum() * self.win
        out = np.zeros((2, H))
        if not first:
            out = (self.tail + g[:, :H]) / (self.win[:H] ** 2 + self.win[H:] ** 2)
        self.tail = g[:, H:]
        return out

    def push(self, mix, adapt=True):
        mix = np.asarray(mix, dtype=np.float64)
        H = self.H
        hops = mix.shape[-1] // H
        assert mix.shape == (2, hops * H) and hops >= 1
        out = np.zeros((2, hops * H))
        for j in range(hops):
            cur = mix[:, j * H:(j + 1) * H]
            Y = np.fft.rfft(np.concatenate([self.prev, cur], axis=1) * self.win32, axis=1) * \
                self.scale
            out[:, j * H:(j + 1) * H] = self.synth(self.push_spec(Y, adapt))
            self.prev = cur.copy()
        return out

    def flush(self):
        """One hop of zeros: drains the last H samples."""
        return self.push(np.zeros((2, self.H)))


def wpe_stream_numpy(x, n_fft=N_FFT, taps=10, delay=3, forget=0.99, power_floor=None, q_init=1.0,
                     adapt=None, hops_per_push=None, y_hook=None, drain=True, dtype=np.float64):
    """A whole signal through NumpyWPEStream -> (out, stream). x: the two mics' samples
    [2, T H] (out [2, (T + drain) H], the drain hop always adapting), or their spectra
    [2, F, T] complex (the analysis is skipped, nothing drains: out [2, T H]). adapt: per-hop
    flags [T] (default all 1); hops_per_push: an int or a list of group sizes (every frame is
    computed on its own, so the grouping does not change the results)."""
    st = NumpyWPEStream(n_fft, taps, delay, forget, power_floor, q_init, y_hook, dtype)
    x = np.asarray(x)
    spec = np.iscomplexobj(x)
    T = x.shape[-1] if spec else x.shape[-1] // st.H
    adapt = np.ones(T, dtype=int) if adapt is None else np.asarray(adapt)
    groups = hops_per_push if isinstance(hops_per_push, (list, tuple)) else None
    if groups is None:
        g = hops_per_push or T
        groups = [min(g, T - i) for i in range(0, T, g)]
    assert sum(groups) == T
    cuts = sorted(set(np.cumsum([0] + list(groups))) | set(np.flatnonzero(np.diff(adapt)) + 1))
    outs = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if spec:
            outs += [st.synth(st.push_spec(x[:, :, t], bool(adapt[a]))) for t in range(a, b)]
        else:
            outs.append(st.push(x[:, a * st.H:b * st.H], bool(adapt[a])))
    if drain and not spec:
        outs.append(st.flush())
    return np.concatenate(outs, axis=1), st


from .stream import StreamOwner  # noqa: E402  (numpy only at import, like this module)


class StreamingWPE(StreamOwner):
    """`streams` independent online-WPE dereverberators over one device state buffer. The
    plan supplies n_fft, the window and max_batch (streams <= plan.cfg.max_batch); its mask
    and beamformer settings play no part. push() returns [streams, 2, hops * hop], one hop
    behind its input, which StreamingBeamformer.push takes as its mix: two hops of latency
    for the pair. self.G holds the filter after the last pushed frame."""

    def __init__(self, plan, streams: int, taps: int = 10, delay: int = 3, forget: float = 0.99,
                 power_floor=None, q_init: float = 1.0, device=None):
        import torch
        from . import engine
        self.taps, self.delay, self.forget = int(taps), int(delay), float(forget)
        self.power_floor = float(default_power_floor(plan.cfg.n_fft) if power_floor is None
                                 else power_floor)
        self.q_init = float(q_init)
        super().__init__(plan, streams, device, engine.wpe_stream_state_bytes, self.taps,
                         self.delay)
        self.G = torch.zeros((self.streams, plan.F, 2 * self.taps, 2), dtype=torch.complex128,
                             device=self.device)
        self.reset()

    def reset(self, select=None, stream=None):
        """Start the selected streams (flags per stream; None = all) afresh."""
        from . import engine
        engine.wpe_stream_reset(self.plan, self.state, self.streams, self.taps, self.delay,
                                self.q_init, self._flags(select, "select"), stream)

    def push(self, mix, *, active=None, adapt=None, out=None, Y_out=None, Z_out=None,
             stream=None):
        """mix [streams, 2, hops * hop] float32 -> out of the same shape: the hops that left
        the dereverberator, one hop behind the input."""
        import torch
        from . import engine
        self._block(mix)
        if out is None:
            out = torch.empty(tuple(mix.shape), dtype=torch.float32, device=mix.device)
        return engine.wpe_stream_push(self.plan, self.state, mix, out, taps=self.taps,
                                      delay=self.delay, forget=self.forget,
                                      power_floor=self.power_floor,
                                      active=self._flags(active, "active"),
                                      adapt=self._flags(adapt, "adapt"), Y_out=Y_out,
                                      Z_out=Z_out, G_out=self.G, stream=stream)

    def flush(self, **kw):
        """Push one hop of zeros: returns the last hop."""
        return self.push(self._zero_hop(), **kw)


def apply_wpe_stream(y_mix, taps=10, delay=3, forget=0.99, power_floor=None, q_init=1.0,
                     n_fft=N_FFT, hops_per_push: int = 8, device="cuda"):
    """The causal counterpart of apply_wpe: (2, L) float32 -> dereverberated (2, L) float32
    numpy, the file pushed ``hops_per_push`` hops at a time through StreamingWPE, drained, the
    one-hop delay trimmed. The grouping does not change the result."""
    import torch
    from .engine import MVDRPlan
    y = np.ascontiguousarray(y_mix, dtype=np.float32)
    if y.ndim != 2 or y.shape[0] != 2 or y.shape[1] < 1:
        raise ValueError("y_mix must be (2, L) samples")
    L, H = y.shape[1], n_fft // 2
    T = -(-L // H)
    plan = MVDRPlan(n_fft=n_fft, mask="ones", postfilter="none", normalize="none", max_batch=1,
                    max_samples=max(T * H, n_fft))
    dev = torch.device(device)
    x = torch.from_numpy(np.pad(y, [(0, 0), (0, T * H - L)]))[None].to(dev)
    sw = StreamingWPE(plan, 1, taps, delay, forget, power_floor, q_init, device=dev)
    outs = [sw.push(x[:, :, j0 * H:min(j0 + hops_per_push, T) * H].contiguous())
            for j0 in range(0, T, hops_per_push)]
    outs.append(sw.flush())
    return torch.cat(outs, dim=2)[0, :, H:H + L].cpu().numpy()


def main(args):
    from . import wavio
    outdir = args.outdir
    if outdir is None:
        print("Error: No simulation directory found.")
        return None
    print("--- Running Standalone WPE Dereverberation ---")
    print(f"Target Directory: {os.path.basename(outdir)}")
    mix_path = os.path.join(outdir, "mixture.wav")
    if not os.path.exists(mix_path):
        print(f"Error: {mix_path} not found.")
        return None
    y_mix, fs = wavio.read(mix_path, dtype="float32")
    if y_mix.ndim > 1 and y_mix.shape[0] > y_mix.shape[1]:   # (:127-129) to (channels, samples)
        print(f"  [Load] Transposing input from {y_mix.shape} to (Channels, Samples)")
        y_mix = y_mix.T
    y_clean = apply_wpe(y_mix, taps=args.taps, delay=args.delay, iterations=args.iters)
    out_path = os.path.join(outdir, "mixture_wpe.wav")
    wavio.write(out_path, y_clean.T, fs)
    print(f"Success! Saved to: {out_path}")
    return y_clean


def parse_args(argv=None):
    """The reference CLI (dereverb.py:140-148)."""
    p = argparse.ArgumentParser()
    p.add_argument("--outdir", type=str, default=DEFAULT_OUTDIR)
    p.add_argument("--taps", type=int, default=10)
    p.add_argument("--delay", type=int, default=3)
    p.add_argument("--iters", type=int, default=3)
    return p.parse_args(argv)


if __name__ == "__main__":
    main(parse_args())
