"""Shared layouts, inputs and fp64 references of the whole-round per-utterance synthesis tests
(test_utt_reference.py, test_gpu_utt_rounds.py). numpy / scipy / the oracle only.

The per-utterance synthesis kernels (csrc/avz_chain_utt.hpp) give one block per CU whole
utterances one after another; a block prefetches its next valid row's first step, rescales the
previous row's output in slices during the next one, skips rows shorter than a frame and
carries the seam across steps. Everything here is a function of R (the device's CU count) and
n_fft, so that a batch of ROUNDS x R rows gives every block three rows of chosen lengths.

H = N / 2, frames T(L) = ceil(L / H) + 1, a step is FB = 16 frames at N = 1024 and 32 at
N = 512, a mask chunk 32 frames.

1. First layout: B = 3 R, block g runs rows g, g + R, g + 2 R; their length classes follow
   g mod 8 (CLASS_TABLE). The longest row has T = 4 FB frames (four steps; 2 or 4 chunks), so
   nch B is a multiple of the analysis grid (2 or 3 blocks per CU): no analysis split, no
   synthesis pieces -- the whole-rounds (PIECES = false) instance at N = 1024, the N = 512
   kernel at all.
2. Second layout (N = 1024): B = R rows of up to 5 chunks. With two analysis blocks per CU the
   5 R items leave a tail of R items that the analysis splits in two pieces each
   (a_whole = 4 R); row b* = floor(4 R / 5) holds item 4 R. The rows b* - 1 .. b* + 3 take the
   classes (max, X, one, skip0, max), every other row `rand`. Two variants, because one row
   cannot be both: X = max ("straddle": b* has chunks 0 .. 4 R - 5 b* - 1 whole and the rest
   split) and X = 2fb ("whole1": b*'s one chunk is whole although its five item slots reach
   past a_whole). Rows past b* have every chunk split.

Signals: seeded Gaussian mix [2, L], tgt [L], itf [L] of standard deviation 0.1 (float32),
per row from (n_fft, key) alone, so a row keeps its samples wherever a permutation puts it.
External masks: seeded uniform [F, 4 FB] (first layout only).
"""
import functools

import numpy as np

import stage_cases as SC
from oracle import avz_oracle as O

SIZES = (512, 1024)
FB = {1024: 16, 512: 32}           # UttGeo::FB, Utt512Geo::FB
BLOCKS_PER_CU = {1024: 2, 512: 3}  # analysis blocks per CU (CGeo<N>::BLOCKS)
CHUNK = 32
ROUNDS = 3
CPU_RS = (32, 64, 256, 304)
WAVE_TOL = SC.WAVE_TOL  # 1e-4, peak-normalised waveform
SIR_TOL = 0.01          # dB
PEAK_RTOL = 1e-4
SPLIT_TOL = 2e-6        # a changed association of the fp32 partial sums
COND_MAX = SC.COND_MAX

CLASS_TABLE = (
    ("max", "max", "max"),
    ("max", "one", "max"),
    ("one", "max", "one+"),
    ("max", "skip0", "max"),
    ("skipN", "max", "skip0"),
    ("skip0", "skipN", "skip0"),
    ("fb", "fb+", "fb-"),
    ("2fb+", "2fb", "rand"),
)
# frames each class must have (None: not live / drawn)
CLASS_FRAMES = {"max": lambda fb: 4 * fb, "one": lambda fb: 3, "one+": lambda fb: 4,
                "fb-": lambda fb: fb - 1, "fb": lambda fb: fb, "fb+": lambda fb: fb + 1,
                "2fb": lambda fb: 2 * fb, "2fb+": lambda fb: 2 * fb + 1}
SKIPPED = ("skip0", "skipN")

# the plans of the GPU test (avz.MVDRPlan options) and their references
PLANS = {
    "ibm": dict(mask="ibm", postfilter="ibm", sigma=1.0, mic_d=0.01, normalize="peak"),
    "ipd": dict(mask="ipd", postfilter="none", sigma=1e-7, mic_d=0.01, normalize="peak",
                norm_eps=1e-6),
    "ext": dict(mask="external", postfilter="none", sigma=1e-5, mic_d=0.04, normalize="peak"),
    "ones": dict(mask="ones", postfilter="none", sigma=SC.MPDR_SIGMA, mic_d=SC.MPDR_D,
                 weight_eps=0.0, normalize="peak", norm_eps=0.0),
}


def n_frames(length, n_fft):
    return -(-length // (n_fft // 2)) + 1


def l_max(n_fft):
    """T = 4 FB: 32256 at N = 1024, 32512 at N = 512."""
    return (4 * FB[n_fft] - 1) * (n_fft // 2)


L2_MAX = (5 * CHUNK - 1) * 512 - 511  # second layout: T = 160 = 5 chunks


def class_length(cls, n_fft, key=0, lmax=None):
    H, fb = n_fft // 2, FB[n_fft]
    lmax = l_max(n_fft) if lmax is None else lmax
    if cls == "rand":
        return int(np.random.default_rng([4100, n_fft, key]).integers(n_fft, lmax + 1))
    return {"max": lmax, "one": n_fft, "one+": n_fft + 1, "fb-": (fb - 2) * H,
            "fb": (fb - 1) * H, "fb+": (fb - 1) * H + 1, "2fb": (2 * fb - 1) * H,
            "2fb+": (2 * fb - 1) * H + 1, "skip0": 0, "skipN": n_fft - 1}[cls]


# ----------------------------------------------------------------------------- layouts
@functools.lru_cache(maxsize=None)
def layout(R, n_fft):
    """First layout: (lens [3 R] int32, classes [3 R], keys [3 R]); key = the row's seed."""
    B = ROUNDS * R
    classes = [CLASS_TABLE[(b % R) % 8][b // R] for b in range(B)]
    lens = np.array([class_length(c, n_fft, b) for b, c in enumerate(classes)], np.int32)
    return lens, classes, np.arange(B)


def sampled_blocks(R):
    """Per g mod 8 class its first block and its last block below R."""
    out = []
    for c in range(8):
        out += [c, c + 8 * ((R - 1 - c) // 8)]
    return sorted(set(out))


def sampled_rows(R, blocks=None):
    blocks = sampled_blocks(R) if blocks is None else blocks
    return [g + r * R for g in blocks for r in range(ROUNDS)]


def reduced_blocks(R):
    """The first block of each class plus block R - 1 (the cut the cost rule allows)."""
    return sorted(set(list(range(8)) + [R - 1]))


def b_star(R):
    return 4 * R // 5


def straddles(R):
    return 5 * b_star(R) < 4 * R < 5 * b_star(R) + 5


L2_VARIANTS = {"straddle": ("max", "max", "one", "skip0", "max"),
               "whole1": ("max", "2fb", "one", "skip0", "max")}
L2_KEY0 = 100000  # row keys of the second layout


@functools.lru_cache(maxsize=None)
def layout2(R, variant):
    """Second layout (N = 1024): (lens [R], classes [R], keys [R])."""
    bs = b_star(R)
    classes = ["rand"] * R
    for i, c in enumerate(L2_VARIANTS[variant]):
        classes[bs - 1 + i] = c
    keys = L2_KEY0 + np.arange(R)
    lens = np.array([class_length(c, 1024, int(k), L2_MAX) for c, k in zip(classes, keys)],
                    np.int32)
    return lens, classes, keys


def sampled_rows2(R):
    bs = b_star(R)
    return sorted(set([0, R - 1] + list(range(bs - 1, bs + 4))))


def block_permutation(R, seed=11):
    """src [3 R]: position p of the permuted batch holds row src[p] of the first layout.
    Blocks move by a seeded single-cycle permutation (no block stays), rounds by 1 or 2 (no
    round stays), so every row changes both its block and its round."""
    rng = np.random.default_rng([seed, R])
    sigma = np.arange(R)
    for i in range(R - 1, 0, -1):  # Sattolo: one cycle of length R
        j = int(rng.integers(0, i))
        sigma[i], sigma[j] = sigma[j], sigma[i]
    shift = 1 + rng.integers(0, 2, size=R)
    src = np.empty(ROUNDS * R, np.int64)
    for g in range(R):
        for r in range(ROUNDS):
            src[int(sigma[g]) + ((r + int(shift[g])) % ROUNDS) * R] = g + r * R
    return src


# ----------------------------------------------------------------------------- signals
def row_signals(n_fft, key, L):
    """(mix [2, L], tgt [L], itf [L]) float32, standard deviation 0.1."""
    rng = np.random.default_rng([5200, n_fft, int(key)])
    z = rng.standard_normal((4, int(L)), dtype=np.float32) * np.float32(0.1)
    return z[:2], z[2], z[3]


def row_mask(n_fft, key):
    """Target probability [F, 4 FB] float32, uniform in [0, 1)."""
    rng = np.random.default_rng([6300, n_fft, int(key)])
    return rng.random((n_fft // 2 + 1, 4 * FB[n_fft]), dtype=np.float32)


def batch(n_fft, lens, keys, refs=True):
    """(mix [B, 2, S], tgt [B, S], itf [B, S]) float32, zero beyond each row's length; S = the
    longest row rounded up to 4 samples. tgt / itf are None without `refs`."""
    B, S = len(lens), (int(max(lens)) + 3) // 4 * 4
    mix = np.zeros((B, 2, S), np.float32)
    tgt = np.zeros((B, S), np.float32) if refs else None
    itf = np.zeros((B, S), np.float32) if refs else None
    for b, (L, k) in enumerate(zip(lens, keys)):
        L = int(L)
        if L == 0:
            continue
        m, t, i = row_signals(n_fft, k, L)
        mix[b, :, :L] = m
        if refs:
            tgt[b, :L] = t
            itf[b, :L] = i
    return mix, tgt, itf


def masks(n_fft, keys):
    """[B, F, 4 FB] float32."""
    return np.stack([row_mask(n_fft, k) for k in keys])


# ----------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def reference(plan, n_fft, key, L):
    """fp64 reference of one live row: dict(raw [(T - 1) H], peak = max|raw|, out = raw /
    (peak + norm_eps), tgt, itf (IBM: for the SIR), R (IBM: the normalised covariance), f)."""
    assert L >= n_fft
    H = n_fft // 2
    mix, tgt, itf = row_signals(n_fft, key, L)
    kw = PLANS[plan]
    r = {}
    if plan == "ibm":
        raw, st = O.oracle_debug_vec(mix, tgt, itf, n_fft=n_fft, hop=H, sigma=kw["sigma"],
                                     d=kw["mic_d"], normalize=False, return_stages=True)
        r.update(tgt=tgt, itf=itf, R=st["R"], f=st["f"])
    elif plan == "ipd":
        raw = O.masked_mvdr_vec(mix, n_fft=n_fft, hop=H, sigma=kw["sigma"], d=kw["mic_d"],
                                normalize=False)
    else:
        T = n_frames(L, n_fft)
        M = (row_mask(n_fft, key)[:, :T].astype(np.float64) if plan == "ext"
             else np.zeros((H + 1, T)))
        raw = O.external_mask_vec(mix, M, n_fft=n_fft, hop=H, sigma=kw["sigma"], d=kw["mic_d"],
                                  floor=None, weight_eps=0.0)
    raw = np.asarray(raw, np.float64)
    peak = float(np.abs(raw).max())
    r.update(raw=raw, peak=peak, out=raw / (peak + kw.get("norm_eps", 0.0)))
    return r


# ----------------------------------------------------------------------------- kernel paths
# which of the chain's kernels a synthesis path launches on its own (plan.set_diagnostics
# synth_variant): 2 = the per-utterance kernel solving its bins (no solve, no finalize launch),
# 1 = the per-utterance kernel after the solve kernel, 0 = chunk grid + finalize
PATHS = {2: dict(solve=False, finalize=False), 1: dict(solve=True, finalize=False),
         0: dict(solve=True, finalize=True)}


def assert_path(plan, run, solve, finalize):
    """run() once with the plan's kernel timing on and assert which kernels the call launched
    (plan.timing(): a kernel folded into another counts 0 ms); solve / finalize: True, False,
    or None (not asserted). Returns run()'s result."""
    plan.set_timing(True)
    try:
        res = run()
        t = plan.timing()
    finally:
        plan.set_timing(False)
    assert t["calls"] == 1 and t["analysis"] > 0 and t["synthesis"] > 0, t
    for k, want in (("solve", solve), ("finalize", finalize)):
        if want is not None:
            assert (t[k] > 0) if want else (t[k] == 0), (k, want, t)
    return res
