"""Shared inputs, memory layouts and fp64 references of the mask-gain and spectrum-input
synthesis tests (test_gain_reference.py, test_gpu_gain_paths.py). numpy / scipy / the oracle
only; nothing here needs the GPU or the library.

Every plan whose gain comes from memory (the external-mask post-filters `floor` and `mul`, the
caller gain of avz_apply_istft) and avz_istft's spectrum input run the chunk-grid synthesis
kernel (csrc/avz_chain_synthesis.hpp) plus avz_finalize_kernel. Per launch and per step those
kernels choose between a 16-byte read of the mask / spectrum row and scalar reads: the vector
read needs a 16-byte aligned base, stride_t == 1, stride_f % 4 == 0 and stride_b % 4 == 0 (a
spectrum: even strides in complex elements) and a full step (f0 + FB <= T). The analysis kernel
(csrc/avz_chain_analysis.hpp) makes the same choice for the noise weight 1 - M.

Geometry: H = N / 2, frames T(L) = ceil(L / H) + 1, a chunk is CHUNK = 32 frames. The
synthesis step is FB = 8 frames at N = 1024; at N = 512 it is 8 for the two external
post-filters (kSynR<512, PF_EXT_*> = 1) and 16 otherwise (spectrum input, no gain). The
analysis step is 8 frames.

FRAMES, both sizes: 3 (the smallest row); 8, 9 (one 8-step, + 1); 15, 16, 17 (two 8-steps, one
16-step, +- 1); 31, 32, 33 (a chunk +- 1); 40, 41 (a chunk and one step, + 1); 63, 64, 65 (two
chunks +- 1; 65: a last chunk of one frame, all of it the seam); 97 (three chunks and a
frame). Per T the lengths (T - 1) H (the last frame holds no sample) and (T - 2) H + 1 (it
holds one), the second only where it is >= N.
"""
import functools

import numpy as np

import stage_cases as SC
from oracle import avz_oracle as O

SIZES = (512, 1024)
CHUNK = 32
FB_GAIN = {1024: 8, 512: 8}    # SGeo<N, kSynR<N, PF_EXT_*>>::NSLOT
FB_PLAIN = {1024: 8, 512: 16}  # SGeo<N, kSynR<N, PF_NONE>>::NSLOT (spectrum input, no gain)
FB_ANALYSIS = 8
FRAMES = (3, 8, 9, 15, 16, 17, 31, 32, 33, 40, 41, 63, 64, 65, 97)

SIGMA = 1e-5
MIC_D = 0.04
PF_FLOOR = 0.05
WEIGHT_EPS = (0.0, 1e-10)
NORM_EPS = 1e-9
HYBRID = dict(mic_d=0.08, bypass_hz=200.0, cond_max=10.0, weight_eps=0.0)

WAVE_TOL = SC.WAVE_TOL     # 1e-4 of max|ref|: whole chain against fp64 (Tier 1)
PEAK_RTOL = SC.WAVE_TOL    # peak, relative
COND_MAX = SC.COND_MAX
STFT_TOL = 2e-6            # test_stft_stage: forward transform, relative to max|Y|
ISTFT_TOL = 2e-6           # test_istft_matches_oracle: inverse transform, relative to max|ref|
W_ROUND = 2.0 ** -23       # fp32 rounding of w_out
STAGE_TOL = 1e-6           # section 14's stage bound: two instances of the same arithmetic
N_PERT = 8


def n_frames(length, n_fft):
    return -(-length // (n_fft // 2)) + 1


@functools.lru_cache(maxsize=None)
def rows(n_fft):
    """[(T, L)] of the ragged batch: per T of FRAMES (T - 1) H and, where >= N, (T - 2) H + 1."""
    H = n_fft // 2
    out = []
    for T in FRAMES:
        out.append((T, (T - 1) * H))
        if (T - 2) * H + 1 >= n_fft:
            out.append((T, (T - 2) * H + 1))
    return tuple(out)


def t_pad(n_fft):
    """Tp: the longest row's frames rounded up to a multiple of 4."""
    return -(-max(FRAMES) // 4) * 4


# ----------------------------------------------------------------------------- signals, masks
@functools.lru_cache(maxsize=None)
def row_signal(n_fft, row, L):
    """[2, L] float32 as stage_cases.mpdr_batch: mic 0 white noise of standard deviation 0.1,
    mic 1 = 0.7 mic 0 + 0.05 independent noise; seeded per (N, row)."""
    rng = np.random.default_rng(9100 + n_fft + row)
    m0 = 0.1 * rng.standard_normal(L)
    m1 = 0.7 * m0 + 0.05 * rng.standard_normal(L)
    return np.stack([m0, m1]).astype(np.float32)


def batch(n_fft, lens=None):
    """(x [B, 2, S] float32 zero-padded, lens [B] int32) of rows(n_fft) (or the given lengths,
    row b seeded as row b; a length below N gives an all-zero row)."""
    lens = [L for _, L in rows(n_fft)] if lens is None else list(lens)
    S = -(-max(lens) // 4) * 4
    x = np.zeros((len(lens), 2, S), np.float32)
    for b, L in enumerate(lens):
        if L >= n_fft:
            x[b, :, :L] = row_signal(n_fft, b, L)
    return x, np.array(lens, np.int32)


ONE_BINS = slice(5, None, 7)    # mask rows of all 1: noise count 0, weight_eps sums
ZERO_BINS = slice(3, None, 11)  # mask rows of all 0 (applied after ONE_BINS: bin 47 is 0)
# (bin, frame as a fraction of T - 1, value): exactly pf_floor as the kernel holds it, one ulp
# below, one ulp above; bins outside ONE_BINS / ZERO_BINS, first / last / middle frame
_F32_FLOOR = np.float32(PF_FLOOR)
FLOOR_PLANTS = ((1, 0.0, _F32_FLOOR), (2, 1.0, _F32_FLOOR), (4, 0.5, _F32_FLOOR),
                (8, 0.0, np.nextafter(_F32_FLOOR, np.float32(0))),
                (9, 1.0, np.nextafter(_F32_FLOOR, np.float32(0))),
                (10, 0.5, np.nextafter(_F32_FLOOR, np.float32(1))),
                (11, 1.0, np.nextafter(_F32_FLOOR, np.float32(1))))


@functools.lru_cache(maxsize=None)
def row_mask(n_fft, row, T):
    """Target probability [F, T] float32, uniform [0, 1) with the rows and entries above."""
    rng = np.random.default_rng([9200, n_fft, row])
    M = rng.random((n_fft // 2 + 1, T), dtype=np.float32)
    M[ONE_BINS] = 1.0
    M[ZERO_BINS] = 0.0
    for k, frac, v in FLOOR_PLANTS:
        M[k, int(round(frac * (T - 1)))] = v
    M.setflags(write=False)
    return M


GAIN_ZERO_BIN = 6


@functools.lru_cache(maxsize=None)
def row_gain(n_fft, row, T):
    """Caller gain of avz_apply_istft [F, T] float32: uniform [0, 2), one all-zero bin."""
    rng = np.random.default_rng([9400, n_fft, row])
    G = (2.0 * rng.random((n_fft // 2 + 1, T))).astype(np.float32)
    G[GAIN_ZERO_BIN] = 0.0
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=None)
def caller_weights(n_fft, B):
    """Caller weights of avz_apply_istft: complex O(1) [B, F, 2] (no solve involved)."""
    rng = np.random.default_rng([9500, n_fft])
    F = n_fft // 2 + 1
    return rng.standard_normal((B, F, 2)) + 1j * rng.standard_normal((B, F, 2))


def weights_to_f32(W):
    """[.., F, 2] complex -> the w_out layout [.., F, 4] float32 (Re w0, Im w0, Re w1, Im w1)."""
    return np.stack([W[..., 0].real, W[..., 0].imag, W[..., 1].real, W[..., 1].imag],
                    axis=-1).astype(np.float32)


def weights_from_f32(w):
    """w_out rows [F, 4] float32 -> [F, 2] complex128."""
    w = np.asarray(w, np.float64)
    return np.stack([w[:, 0] + 1j * w[:, 1], w[:, 2] + 1j * w[:, 3]], axis=-1)


SPEC_BATCH = 3


@functools.lru_cache(maxsize=None)
def spectra(n_fft, T):
    """[3, F, T] complex64, every entry complex (DC and Nyquist too: irfft ignores those
    imaginary parts and so must the kernel)."""
    rng = np.random.default_rng([9600, n_fft, T])
    F = n_fft // 2 + 1
    S = (rng.standard_normal((SPEC_BATCH, F, T)) + 1j * rng.standard_normal((SPEC_BATCH, F, T)))
    S = S.astype(np.complex64)
    S.setflags(write=False)
    return S


@functools.lru_cache(maxsize=None)
def istft_reference(n_fft, T):
    """[3, (T - 1) H] fp64: oracle.istft of spectra(n_fft, T)."""
    return O.istft(spectra(n_fft, T).astype(np.complex128), nperseg=n_fft,
                   noverlap=n_fft // 2)[1]


# ----------------------------------------------------------------------------- layouts
# One logical array [B, F, Tl] (float32 masks / gains, Tl <= Tp valid frames per row given by
# the caller as NaN beyond them) placed into a NaN-filled flat buffer; the view the library gets
# is as_strided(buffer, shape, strides, offset) (elements). `path`: what the kernels do on a
# full step. A torch allocation is at least 256-byte aligned, so offset % 4 decides the base.
MASK_LAYOUTS = {
    "A": "contiguous [B, F, Tp], base 16-byte aligned: vector",
    "B": "stride_f = Tp + 4 and mask_frames = Tp + 4 > T: vector",
    "C": "base advanced by one float (frame 1 of rows Tp + 4 wide): scalar",
    "D": "stride_f = Tp + 1 (stride_b % 4 == 0): scalar",
    "E": "stride_f % 4 == 0 but stride_b = F stride_f + 1: scalar for every row, b = 0 too",
    "F": "bin-contiguous (stride_f = 1, stride_t = F + 3): scalar",
    "G": "mask_bins = F + 2: vector",
    "H": "stride_b = 0, one mask for all rows (expand): vector",
}
VECTOR_MASK_LAYOUTS = ("A", "B", "G", "H")


def mask_layout(lid, B, F, Tp):
    """(numel, offset, shape, strides) of layout `lid`; shape[1] / shape[2] are what the call
    states as mask_bins / mask_frames, of which [:F, :Tp] hold the logical array."""
    if lid == "A":
        return B * F * Tp, 0, (B, F, Tp), (F * Tp, Tp, 1)
    if lid == "B":
        W = Tp + 4
        return B * F * W, 0, (B, F, W), (F * W, W, 1)
    if lid == "C":
        W = Tp + 4
        return B * F * W, 1, (B, F, Tp), (F * W, W, 1)
    if lid == "D":
        W = Tp + 1
        sb = -(-F * W // 4) * 4  # a multiple of 4: stride_f alone keeps it off the vector path
        return B * sb, 0, (B, F, Tp), (sb, W, 1)
    if lid == "E":
        sb = F * Tp + 1
        return B * sb, 0, (B, F, Tp), (sb, Tp, 1)
    if lid == "F":
        st = F + 3
        return B * Tp * st, 0, (B, F, Tp), (Tp * st, 1, st)
    if lid == "G":
        return B * (F + 2) * Tp, 0, (B, F + 2, Tp), ((F + 2) * Tp, Tp, 1)
    if lid == "H":
        return F * Tp, 0, (B, F, Tp), (0, Tp, 1)
    raise KeyError(lid)


def mask_takes_vector_path(offset, strides):
    """The kernels' own condition (avz_chain_synthesis.hpp mask_vec) for a 256-byte aligned
    buffer."""
    sb, sf, st = strides
    return st == 1 and sf % 4 == 0 and sb % 4 == 0 and offset % 4 == 0


# spectra [B, F, T] complex64, t contiguous; strides in complex elements
SPEC_LAYOUTS = {
    "A": "stride_f = T rounded up to even, stride_b = F stride_f (even), aligned base: vector",
    "B": "stride_f even + 2 (wider rows), even stride_b: vector",
    "C": "stride_f odd: scalar",
    "D": "stride_f even, stride_b odd: scalar",
    "E": "base advanced by one complex element (8-byte, not 16-byte aligned): scalar",
}
VECTOR_SPEC_LAYOUTS = ("A", "B")


def spec_layout(lid, B, F, T):
    Te = T + (T & 1)
    if lid == "A":
        return B * F * Te, 0, (B, F, T), (F * Te, Te, 1)
    if lid == "B":
        W = Te + 2
        return B * F * W, 0, (B, F, T), (F * W, W, 1)
    if lid == "C":
        W = Te + 1
        return B * F * W, 0, (B, F, T), (F * W, W, 1)
    if lid == "D":
        sb = F * Te + 1
        return B * sb, 0, (B, F, T), (sb, Te, 1)
    if lid == "E":
        W = Te + 2
        return B * F * W + 1, 1, (B, F, T), (F * W, W, 1)
    raise KeyError(lid)


def spec_takes_vector_path(offset, strides):
    sb, sf, st = strides
    return st == 1 and sf % 2 == 0 and sb % 2 == 0 and offset % 2 == 0


def place(logical, spec):
    """The flat NaN-filled host buffer of layout `spec` holding `logical` ([B, F, T], or
    [F, T] for a layout of batch stride 0) in its leading bins / frames."""
    numel, offset, shape, strides = spec
    logical = np.asarray(logical)
    buf = np.full(numel, np.nan, logical.dtype)
    item = buf.itemsize
    view = np.lib.stride_tricks.as_strided(buf[offset:], shape, [s * item for s in strides])
    if strides[0] == 0:
        assert logical.ndim == 2
        view[0, :logical.shape[0], :logical.shape[1]] = logical
    else:
        view[:, :logical.shape[1], :logical.shape[2]] = logical
    return buf


def padded_masks(n_fft, lens, draw=row_mask):
    """[B, F, Tp] float32: row b's draw(n_fft, b, T_b) in its first T_b frames, NaN beyond (a
    row shorter than N: all NaN -- it is never read)."""
    F, Tp = n_fft // 2 + 1, t_pad(n_fft)
    out = np.full((len(lens), F, Tp), np.nan, np.float32)
    for b, L in enumerate(lens):
        if L >= n_fft:
            T = n_frames(int(L), n_fft)
            out[b, :, :T] = draw(n_fft, b, T)
    return out


# ----------------------------------------------------------------------------- references
def gain_of(M, pf):
    """The gain a plan states: max(M, floor), M, or None (1)."""
    if pf == "floor":
        return np.maximum(M, PF_FLOOR)
    if pf == "mul":
        return M
    assert pf == "none"
    return None


def chain_reference(x, M, G, n_fft, weight_eps=0.0, return_stages=False):
    """Tier 1: oracle.external_mask_vec (full_audio_generating_pipeline/inference.py:88-118)
    with the post-filter as a gain array G [F, T] (None: no post-filter)."""
    f, _, Y = O.stft(x, nperseg=n_fft, noverlap=n_fft // 2)
    R = O.covariance_vec(Y, 1.0 - M, weight_eps)
    W = O.mvdr_weights_vec(R, f, SIGMA, O.ANGLE_TARGET, MIC_D, O.C_SOUND)
    S = O.apply_weights(W, Y)
    if G is not None:
        S = S * G
    out = O.istft(S, nperseg=n_fft, noverlap=n_fft // 2)[1]
    return (out, dict(f=f, Y=Y, R=R, W=W)) if return_stages else out


@functools.lru_cache(maxsize=None)
def tier1(n_fft, row, L, pf, weight_eps):
    """fp64 whole-chain reference of one row of rows(n_fft): dict(out, peak, W, R, f)."""
    x = row_signal(n_fft, row, L)
    M = row_mask(n_fft, row, n_frames(L, n_fft))
    out, st = chain_reference(x, M, gain_of(M, pf), n_fft, weight_eps, return_stages=True)
    return dict(out=out, peak=float(np.abs(out).max()), W=st["W"], R=st["R"], f=st["f"])


@functools.lru_cache(maxsize=None)
def stft64(n_fft, row, L):
    """(f, Y [2, F, T] complex128): the fp64 oracle.stft of the row (no complex64 rounding)."""
    f, _, Y = O.stft(row_signal(n_fft, row, L).astype(np.float64), nperseg=n_fft,
                     noverlap=n_fft // 2)
    return f, Y


def synth_reference(Y, W, G, n_fft):
    """Tier 2 arithmetic: istft(G (w^H Y)) for Y [.., 2, F, T], W [F, 2], G [F, T] or None."""
    S = np.conj(W[:, 0])[:, None] * Y[..., 0, :, :] + np.conj(W[:, 1])[:, None] * Y[..., 1, :, :]
    if G is not None:
        S = S * G
    return O.istft(S, nperseg=n_fft, noverlap=n_fft // 2)[1]


def _tier2(n_fft, Y, W, G, seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1, 1, (N_PERT,) + Y.shape) + 1j * rng.uniform(-1, 1, (N_PERT,) + Y.shape)
    u /= np.maximum(np.abs(u), 1.0)
    stack = np.concatenate([Y[None], u * (STFT_TOL * np.abs(Y).max())])
    xs = synth_reference(stack, np.asarray(W, np.complex128), G, n_fft)
    peak = float(np.abs(xs[0]).max())
    e_pert = float(np.abs(xs[1:]).max())
    return xs[0], e_pert, 4 * e_pert + ISTFT_TOL * peak + W_ROUND * peak


def tier2(n_fft, row, L, W, G):
    """Tier 2: (x [(T - 1) H] fp64, E_pert, tol) of one row of rows(n_fft) with weights W
    [F, 2] complex and gain G [F, T] (None: 1). E_pert is the largest |dx| over N_PERT seeded
    perturbations of Y by complex noise of modulus <= STFT_TOL max|Y| (the bound
    test_stft_stage holds the forward transform to; the construction of test_gpu_wpe.py). The
    synthesis is linear in Y, so dx is the synthesis of the noise.
    tol = 4 E_pert + ISTFT_TOL max|x| + W_ROUND max|x|."""
    return _tier2(n_fft, stft64(n_fft, row, L)[1], W, G, [9300, n_fft, row])


def tier2_signal(n_fft, x, W, G):
    """tier2 of an explicit signal x [2, L] float32 (the noise seeded from its length)."""
    _, _, Y = O.stft(x.astype(np.float64), nperseg=n_fft, noverlap=n_fft // 2)
    return _tier2(n_fft, Y, W, G, [9800, n_fft, x.shape[1]])


def cond_solved_bins(R, f):
    """cond_2 of R + sigma I (R already divided by sum m + 1e-6) in the solved bins."""
    A = R[f >= O.FMIN_MVDR] + SIGMA * np.eye(2)
    return np.linalg.cond(A)


# ----------------------------------------------------------------------------- many rows
MANY_FRAMES = (3, 9, 33, 41, 65)


def many_rows(R, n_fft):
    """B = 2 R + 5 rows cycling through MANY_FRAMES (L = (T - 1) H): with the chunk grid's
    blocks per CU times R blocks there are more (chunk, row) items than blocks. Returns
    (T [B], lens [B] int32, sampled rows: first and last of each T class, rows R and 2 R)."""
    B = 2 * R + 5
    T = np.array([MANY_FRAMES[b % len(MANY_FRAMES)] for b in range(B)])
    lens = ((T - 1) * (n_fft // 2)).astype(np.int32)
    sampled = set([R, 2 * R])
    for c in range(len(MANY_FRAMES)):
        cls = np.nonzero(np.arange(B) % len(MANY_FRAMES) == c)[0]
        sampled.update([int(cls[0]), int(cls[-1])])
    return T, lens, sorted(sampled)


def many_inputs(R, n_fft):
    """(x [B, 2, S] float32, masks [B, F, Tp] float32 NaN past each row's frames) of
    many_rows: drawn whole from one generator per size (row b's signal is x[b, :, :L_b])."""
    T, lens, _ = many_rows(R, n_fft)
    B, S, F = len(lens), int(lens.max()), n_fft // 2 + 1
    Tp = -(-int(T.max()) // 4) * 4
    rng = np.random.default_rng([9700, n_fft, R])
    x = rng.standard_normal((B, 2, S), dtype=np.float32) * np.float32(0.1)
    x[:, 1] = np.float32(0.7) * x[:, 0] + np.float32(0.5) * x[:, 1]
    M = rng.random((B, F, Tp), dtype=np.float32)
    M[:, ONE_BINS] = 1.0
    M[:, ZERO_BINS] = 0.0
    x[np.broadcast_to((np.arange(S)[None, :] >= lens[:, None])[:, None, :], x.shape)] = 0.0
    M[np.broadcast_to((np.arange(Tp)[None, :] >= T[:, None])[:, None, :], M.shape)] = np.nan
    return x, M
