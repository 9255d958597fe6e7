"""Shared inputs and fp64 references of the stage tests (test_stage_reference.py,
test_gpu_stages.py): the driver-side kernels that the whole-pipeline goldens reach at one
shape only. numpy / scipy only; nothing here needs the GPU or the library.

H = N / 2, frames T = ceil(L / H) + 1, the chain's chunk is 32 frames.

1. MPDR (mask "ones" through the offline chain). Per size one ragged batch of
   L = N, N + 1, 3 N / 2 + 7, 31 H (T = 32), 31 H + 1 (T = 33: a second chunk), 64 H + 5.
   Mic 0 is white noise of standard deviation 0.1, mic 1 is 0.7 mic 0 plus independent noise
   of standard deviation 0.05 (float32). sigma 1e-5, mic_d 0.04. Reference:
   oracle.external_mask_vec with a zero target mask (noise weight 1 everywhere).
2. SRP scan. A white source at 60 degrees reaches the pair with the far-field delays
   +-(d / 2) cos(theta) / c of the steering model (an rfft phase shift over the whole signal),
   plus independent noise at 0.3 x per mic, all scaled by 0.1, float32. Per size and spacing
   (0.01, 0.08 m) one ragged batch of L = N, 3 N / 2 + 7, 31 H + 1, N - 1 (the last is
   shorter than a frame: not scanned). Reference: oracle.srp_scan's arithmetic in fp64 with
   an angle range.
3. Chunk split / merge: numpy slicing with zero padding; the kernel's stated fp32 sum
   (chunks added in ascending order, divided by float(count)) and the fp64 transcription of
   Final_pipeline/src/inference.py:224-236.
4. Projection metrics: six ragged rows at stride 8200, o = noise + 2 t.
5. Mask features: train_cases' batches, as drawn and with the mixture noise scaled up (see
   FEAT_NOISE_SCALES); the fp64 spectra behind train_cases.reference's Sample.feat, for the
   propagated tolerances of test_gpu_features._check.
"""
import math

import numpy as np

from oracle import avz_oracle as O

SIZES = (512, 1024)
FS = 16000
C_SOUND = 343.0


def n_frames(length, n_fft):
    return -(-length // (n_fft // 2)) + 1


# ----------------------------------------------------------------------------- 1. MPDR
MPDR_SIGMA = 1e-5
MPDR_D = 0.04
COV_TOL = 2e-6    # test_gpu_parity.py: covariance sums, relative to max_k R00
W_TOL = 1e-3      # test_gpu_parity.py: weights, relative to max |W|
WAVE_TOL = 1e-4   # test_gpu_parity.py: waveform, relative to max |ref|
COND_MAX = 100.0  # 2-norm condition of R / (T + 1e-6) + sigma I in every solved bin


def mpdr_lengths(n_fft):
    H = n_fft // 2
    return [n_fft, n_fft + 1, 3 * n_fft // 2 + 7, 31 * H, 31 * H + 1, 64 * H + 5]


_MPDR = {}


def mpdr_batch(n_fft):
    """(x [B, 2, S] float32 zero-padded rows, lens [B] int32)."""
    lens = mpdr_lengths(n_fft)
    S = max(lens)
    x = np.zeros((len(lens), 2, S), np.float32)
    for b, L in enumerate(lens):
        rng = np.random.default_rng(7100 + n_fft + b)
        m0 = 0.1 * rng.standard_normal(L)
        m1 = 0.7 * m0 + 0.05 * rng.standard_normal(L)
        x[b, 0, :L] = m0.astype(np.float32)
        x[b, 1, :L] = m1.astype(np.float32)
    return x, np.array(lens, np.int32)


def mpdr_reference(n_fft):
    """Per item: dict(T, cov [F, 5] fp64 sums, R [F, 2, 2], W [F, 2], out [(T - 1) H], f),
    computed once with the oracle's stages (oracle_debug.py:56-79 with every weight 1)."""
    if n_fft not in _MPDR:
        x, lens = mpdr_batch(n_fft)
        ref = []
        for b, L in enumerate(lens):
            xb = x[b, :, :L]
            f, _, Y = O.stft(xb, nperseg=n_fft, noverlap=n_fft // 2)
            T = Y.shape[-1]
            R = O.covariance_vec(Y, np.ones(Y.shape[1:]))
            s = R * (T + 1e-6)
            cov = np.stack([s[:, 0, 0].real, s[:, 1, 1].real, s[:, 0, 1].real, s[:, 0, 1].imag,
                            np.full(len(f), float(T))], axis=1)
            W = O.mvdr_weights_vec(R, f, MPDR_SIGMA, O.ANGLE_TARGET, MPDR_D, C_SOUND)
            out = O.external_mask_vec(xb, np.zeros(Y.shape[1:]), n_fft=n_fft, hop=n_fft // 2,
                                      sigma=MPDR_SIGMA, d=MPDR_D, floor=None, weight_eps=0.0)
            ref.append(dict(T=T, cov=cov, R=R, W=W, out=out, f=f))
        _MPDR[n_fft] = ref
    return _MPDR[n_fft]


# ----------------------------------------------------------------------------- 2. SRP
SRP_ANGLE = 60.0
SRP_SPACINGS = (0.01, 0.08)
SRP_BAND_ON_BINS = (312.5, 2000.0)   # both edges are bin frequencies at N = 512 and 1024
SRP_BAND_DEFAULT = (200.0, 4000.0)
SRP_BAND_EMPTY = (2.0, 10.0)         # holds no bin at either size ([10, 20] holds 15.625 Hz
                                     # of N = 1024)
SRP_N_ANGLES = (1, 2, 181, 300)


def srp_lengths(n_fft):
    H = n_fft // 2
    return [n_fft, 3 * n_fft // 2 + 7, 31 * H + 1, n_fft - 1]


def srp_scene(L, d, seed, angle=SRP_ANGLE):
    """[2, L] float32: the source delayed by tau_m = +-(d / 2) cos(theta) / c at mic m (the
    steering model of scripts/debug_srp.py:17-23) plus 0.3 x independent noise, times 0.1."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(L)
    X = np.fft.rfft(s)
    fr = np.fft.rfftfreq(L, 1.0 / FS)
    tau = (d / 2) * np.cos(np.deg2rad(angle)) / C_SOUND
    mics = [np.fft.irfft(X * np.exp(-2j * np.pi * fr * t), n=L) for t in (tau, -tau)]
    y = np.stack([m + 0.3 * rng.standard_normal(L) for m in mics])
    return (0.1 * y).astype(np.float32)


def srp_batch(n_fft, d):
    """(x [4, 2, S] float32, lens [4] int32); the last row is shorter than a frame."""
    lens = srp_lengths(n_fft)
    S = max(lens)
    x = np.zeros((len(lens), 2, S), np.float32)
    for b, L in enumerate(lens):
        x[b, :, :L] = srp_scene(L, d, 8200 + n_fft + b + int(round(1000 * d)))
    return x, np.array(lens, np.int32)


def srp_reference(y2, n_fft, d, f_lo=200.0, f_hi=4000.0, n_angles=181, angle_lo=0.0,
                  angle_hi=180.0):
    """oracle.srp_scan (scripts/debug_srp.py:46-62) in fp64 with an angle range. Returns
    (angles, dB relative to the maximum, tau): tau = 4 x 2e-6 x K_sel x max_k(R00, R11) /
    P_max, the bound on |10^(dB / 10) - 10^(ref / 10)| that the project's covariance tolerance
    (2e-6 of the largest diagonal sum, four entries per bin, K_sel scanned bins) allows."""
    f, _, Y = O.stft(y2, fs=FS, nperseg=n_fft, noverlap=n_fft // 2)
    Y = Y.astype(np.complex128)
    angles = np.linspace(angle_lo, angle_hi, n_angles)
    sel = (f >= f_lo) & (f <= f_hi)
    om = 2 * np.pi * f[sel]
    P = np.empty(n_angles)
    for i, a in enumerate(angles):
        th = np.deg2rad(a)
        t1 = (d / 2) * np.cos(0) * np.cos(th - 0) / C_SOUND
        t2 = (d / 2) * np.cos(0) * np.cos(th - np.pi) / C_SOUND
        dv = np.stack([np.exp(-1j * om * t1), np.exp(-1j * om * t2)])
        out = np.einsum("mf,mft->ft", dv.conj(), Y[:, sel, :])
        P[i] = np.sum(np.abs(out) ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        db = 10 * np.log10(P)
        db = db - db.max() if n_angles else db
        diag = np.sum(np.abs(Y[:, sel, :]) ** 2, axis=2)    # [2, K_sel]: R00, R11 per bin
        tau = (4 * COV_TOL * int(sel.sum()) * diag.max() / P.max()) if sel.any() else np.nan
    return angles, db, tau


def srp_transcription(y2, n_fft, d):
    """scripts/debug_srp.py:44-62 line by line (scipy's stft, the double loop)."""
    import scipy.signal
    f, _, Y_stft = scipy.signal.stft(y2, fs=FS, nperseg=n_fft, noverlap=n_fft // 2)
    angles = np.linspace(0, 180, 181)
    power_map = []
    for angle in angles:
        energy = 0
        for i in range(len(f)):
            if f[i] < 200 or f[i] > 4000:
                continue
            th = np.deg2rad(angle)
            t1 = (d / 2) * np.cos(0) * np.cos(th - 0) / C_SOUND
            t2 = (d / 2) * np.cos(0) * np.cos(th - np.pi) / C_SOUND
            om = 2 * np.pi * f[i]
            dv = np.array([np.exp(-1j * om * t1), np.exp(-1j * om * t2)])
            energy += np.sum(np.abs(dv.conj().T @ Y_stft[:, i, :]) ** 2)
        power_map.append(energy)
    power_map = 10 * np.log10(power_map)
    power_map -= np.max(power_map)
    return angles, power_map


# ----------------------------------------------------------------------------- 3. chunks
SPLIT_LENS = (1000, 37, 2049)
SPLIT_STRIDE = 2052
SPLIT_CHUNK = 1030   # no multiple of 4, more than one block's 1024 samples
# (utterance, start): from 0 with the end inside the chunk; mid-utterance; an utterance that
# ends in the middle of a float4 (37 = 9 x 4 + 1); a start past the end (all zeros); a full
# chunk; a start at the chunk size; an end in the middle of a float4 of the second block
SPLIT_ITEMS = ((0, 0), (0, 515), (1, 0), (1, 40), (2, 0), (2, 1030), (2, 1022))
SPLIT_ITEM_CH_STRIDES = (1032, 1033)  # 16-byte aligned rows (vector body, scalar tail); misaligned


def split_input(channels):
    """x [3, channels, SPLIT_STRIDE] float32, random beyond each length too (the padding must
    come from the kernel, not from the input)."""
    rng = np.random.default_rng(9300 + channels)
    return rng.standard_normal((len(SPLIT_LENS), channels, SPLIT_STRIDE)).astype(np.float32)


def split_reference(x, lens, items, chunk):
    """[n_items, channels, chunk]: np.pad of the tail chunk, inference.py:191-195."""
    out = np.zeros((len(items), x.shape[1], chunk), np.float32)
    for i, (u, s) in enumerate(items):
        seg = x[u, :, :lens[u]][:, s:s + chunk]
        out[i, :, :seg.shape[1]] = seg
    return out


# (hop, item_out_len, max_len): the reference's ratio over three blocks of 1024 samples; up
# to three covering chunks; gaps that no chunk covers (count 0 -> 0)
MERGE_SETS = ((16, 32, 2500), (7, 20, 100), (10, 6, 95))
# per set: max_len itself, 1, a non-multiple of the hop, one more
MERGE_LENS = {(16, 32, 2500): (2500, 1, 2387, 1203), (7, 20, 100): (100, 1, 93, 51),
              (10, 6, 95): (95, 1, 83, 42)}
MERGE_ORDER = (2, 0, 3, 1)   # the utterances' items in this order: item_base is not sorted
MERGE_PAD = 5                # item_out_stride = item_out_len + MERGE_PAD
MERGE_PLANT = 50.0


def merge_plant_positions(lens):
    """Where each utterance's largest |y| is planted: the first block; (len 1: its only
    sample); inside the last partial block; the last sample."""
    return (5, 0, lens[2] - 40, lens[3] - 1)


def merge_case(hop, iol, max_len):
    """(item_out [n_items, iol + MERGE_PAD] float32, lens, item_base): random chunk outputs
    (the padding columns too), with +-MERGE_PLANT in every chunk covering the planted samples."""
    lens = MERGE_LENS[(hop, iol, max_len)]
    rng = np.random.default_rng(9400 + hop)
    nch = [-(-L // hop) for L in lens]
    base = [0] * len(lens)
    n = 0
    for u in MERGE_ORDER:
        base[u] = n
        n += nch[u]
    io = rng.standard_normal((n, iol + MERGE_PAD)).astype(np.float32)
    for u, pos in enumerate(merge_plant_positions(lens)):
        sign = -1.0 if u % 2 else 1.0
        for c in range(nch[u]):
            if c * hop <= pos < c * hop + iol:
                io[base[u] + c, pos - c * hop] = sign * MERGE_PLANT
    return io, np.array(lens, np.int32), np.array(base, np.int32)


def merge_reference_f64(io, lens, base, hop, iol):
    """Final_pipeline/src/inference.py:224-236 per utterance in fp64: (final before the peak
    normalisation [L], sum of |terms| per sample [L]) lists."""
    ys, mags = [], []
    for u, L in enumerate(lens):
        out_buf, norm_buf, mag = np.zeros(L), np.zeros(L), np.zeros(L)
        for i in range(int(np.ceil(L / hop))):
            start = i * hop
            chunk_out = io[base[u] + i, :iol].astype(np.float64)
            w_len = min(len(chunk_out), len(out_buf[start:]))
            out_buf[start:start + w_len] += chunk_out[:w_len]
            mag[start:start + w_len] += np.abs(chunk_out[:w_len])
            norm_buf[start:start + w_len] += 1.0
        ys.append(out_buf / np.maximum(norm_buf, 1.0))
        mags.append(mag)
    return ys, mags


def merge_reference_f32(io, lens, base, hop, iol):
    """The kernel's stated sum in float32: the covering chunks added in ascending order, the
    sum divided by float(count) (count 0 -> 1). Returns ([y [L] float32], peak [B] float32)."""
    ys, peaks = [], np.zeros(len(lens), np.float32)
    for u, L in enumerate(lens):
        acc, cnt = np.zeros(L, np.float32), np.zeros(L, np.int64)
        for i in range(-(-L // hop)):
            start = i * hop
            w = min(iol, L - start)
            acc[start:start + w] = acc[start:start + w] + io[base[u] + i, :w]
            cnt[start:start + w] += 1
        y = acc / np.maximum(cnt, 1).astype(np.float32)
        assert y.dtype == np.float32
        ys.append(y)
        peaks[u] = np.max(np.abs(y))
    return ys, peaks


# ----------------------------------------------------------------------------- 4. metrics
MET_LENS = (0, 1, 3, 5, 4097, 8191)
MET_STRIDE = 8200   # a multiple of 4: with 16-byte-aligned bases the float4 path
MET_PEAKS = (0.5, 3.0, 1e-3, 1.0, 7.25, 0.125)
MET_EPS = (0.0, 1e-9)


def metrics_inputs():
    """(o, t, i) [6, MET_STRIDE] float32, o = noise + 2 t as test_device_metrics_ragged_batch."""
    rng = np.random.default_rng(3)
    o, t, i = (rng.standard_normal((len(MET_LENS), MET_STRIDE)).astype(np.float32)
               for _ in range(3))
    return o + 2.0 * t, t, i


def metrics_sums(o, t, i):
    """(sums [6] correctly rounded, bound [6] = L 2^-53 sum |a_n b_n|) of one row's first L
    samples (float32 values; a product of two is exact in fp64)."""
    a = [x.astype(np.float64) for x in (o, t, i)]
    pairs = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
    s = np.array([math.fsum(a[p] * a[q]) for p, q in pairs])
    bound = np.array([len(o) * 2.0 ** -53 * math.fsum(np.abs(a[p] * a[q])) for p, q in pairs])
    return s, bound


def metrics_reference(o, t, i, peak=None, eps=0.0):
    """[OSINR, OSIR, SDR, SIR] of the float32 values in fp64 (metrics.py:102-123,
    run_metrics.py:6-36), o / (peak + eps) formed in fp64 when a peak is given."""
    o, t, i = (x.astype(np.float64) for x in (o, t, i))
    if peak is not None:
        o = o / (float(np.float32(peak)) + eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array(list(O.osinr_osir(o, t, i)) + list(O.projection_sdr_sir(o, t, i)))


# ----------------------------------------------------------------------------- 5. features
FEAT_D_ABS = 4e-6       # test_gpu_features._check: |dY| <= 4e-6 max|Y| of the item
FEAT_IPD_LOOSE = 0.05   # rad
FEAT_CAP = 0.01         # at most this share of an item's entries may have a looser IPD bound

# The mixtures of train_cases carry noise of standard deviation 1e-3 under sources of order 1:
# in the frames whose references are silent (item 1, a third of its frames) and in the last
# frame of B's item 2 (14 H + 37 samples: 37 samples under the start of the window, 2e-3 of a
# full frame's spectrum whatever the signal) min(|Y0|, |Y1|) is below 1e-4 max|Y| and the
# propagated IPD bound is looser than FEAT_IPD_LOOSE for 33 % / 6 % of the item. Scaling that
# noise is the remedy; the short last frame comes under the cap only once the largest bin
# of the item is itself noise: x 10000 (standard deviation 10) leaves at most 0.27 % loose
# (x 3000: 3.2 %). Both sets are run: as drawn (structure, no cap) and scaled (the cap).
FEAT_NOISE_SCALES = (1, 10000)
FEAT_CAPPED_SCALE = 10000

_FEAT = {}


def feature_batch(n_fft, name, scale=1):
    """(mix [3, 2, S] float32, lens) of train_cases.batches(n_fft)[name] with the mixture noise
    (mix minus the two references, in fp64) multiplied by `scale`."""
    import train_cases as TC
    mix, tgt, itf, lens = TC.batches(n_fft)[name]
    if scale == 1:
        return mix, lens
    clean = (tgt.astype(np.float64) + itf.astype(np.float64))[:, None, :]
    return (clean + scale * (mix.astype(np.float64) - clean)).astype(np.float32), lens


def feature_reference(n_fft, name, scale=1):
    """Per item of feature_batch(n_fft, name, scale): None (len < N) or dict(feat = the
    Sample.feat of avz.train.features_labels_numpy (train_cases.reference's own at scale 1),
    Y [2, F, T] complex128, d_abs, tol_lm, tol_ipd)."""
    import scipy.signal

    import train_cases as TC
    key = (n_fft, name, scale)
    if key not in _FEAT:
        from avz import train
        mix, lens = feature_batch(n_fft, name, scale)
        _, tgt, itf, _ = TC.batches(n_fft)[name]
        out = []
        for b, ref in enumerate(TC.reference(n_fft, name)):
            if ref is None:
                out.append(None)
                continue
            L = int(lens[b])
            feat = ref[0].feat if scale == 1 else train.features_labels_numpy(
                mix[b, :, :L], tgt[b, :L], itf[b, :L], n_fft).feat
            _, _, Y = scipy.signal.stft(mix[b, :, :L].astype(np.float64), fs=FS, nperseg=n_fft,
                                        noverlap=n_fft // 2)
            mag = np.abs(Y)
            d_abs = FEAT_D_ABS * mag.max()
            out.append(dict(feat=feat, Y=Y, d_abs=d_abs,
                            tol_lm=d_abs / (mag[0] + 1e-7) + 1e-5,
                            tol_ipd=d_abs / np.minimum(mag[0], mag[1]).clip(1e-30) + 1e-5))
        _FEAT[key] = out
    return _FEAT[key]
