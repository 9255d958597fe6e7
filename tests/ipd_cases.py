"""Shared rows, layouts, fp64 references and bounds of the IPD-decision tests on degenerate
channel pairs (test_ipd_reference.py, test_gpu_ipd_edges.py). numpy and the oracle only.

The heuristic IPD mask (masked_mvdr.py:37-46) weights a cell 0.01 where angle(Y0) == angle(Y1)
as float32 and 1.0 otherwise. The analysis kernel (csrc/avz_chain_analysis.hpp, MASK_IPD)
decides it in five pieces -- a per-frame "channels bitwise identical" flag, a fast cross-product
test on the covariance products, a fix-up loop that adds (w - 1) p for the frames the fast test
left open, DC and Nyquist by sign on one wave, and a weight count of exact integers plus 0.01
terms -- and the rows here are the inputs on which each of them decides alone.

H = N / 2, frames T(L) = ceil(L / H) + 1, frame t covers the samples [(t - 1) H, (t + 1) H)
after the reference's zero extension, a mask chunk is 32 frames, an IPD step 8 frames. Unless
stated a row has L = 40 H + 17: T = 42, two chunks, the second ending in a partial step of two
frames. The base signal of a row is seeded Gaussian [3, L] of standard deviation 0.1 (float32)
from (n_fft, the row's draw), g0 / g1 the channels and g2 the perturbation of `near`; the level
rows share `gauss`'s draw and `ch1_mul0` shares `ch1_zero`'s.

Rows (ROWS):
  gauss           control
  ch1_zero        ch1 = +0 everywhere
  ch0_zero        ch0 = +0 everywhere
  ch1_mul0        ch1 * float32(0): every negative sample is -0.0
  ch1_dead_span   ch1 = +0 on [12 H + 37, 18 H + 101): frames 14 .. 17 silent in ch1 only
                  (both sides of the step boundary 15 | 16), 12, 13, 18, 19 partly silent
  both_zero_span  both channels +0 on [0, 3 H) (frames 0 .. 2 silent, 3 partly) and on
                  [20 H + 5, 25 H + 9) (frames 22 .. 24 silent, 20, 21, 25, 26 partly)
  ident_all       ch1 = ch0
  ident_spans     ch1 = ch0 on [0, H), [6 H, 9 H), [19 H, 21 H), [30 H, 33 H), [40 H, L): the
                  bitwise-identical frames are IDENT_FRAMES = 0, 7, 8, 20, 31, 32, 41 -- the
                  first and the last frame, both sides of a step boundary and of the chunk
                  boundary, a lone one, one of the partial last step; every step keeps a frame
                  that is not identical
  anti            ch1 = -ch0
  near            ch1 = float32(ch0 + 1e-4 g2), L = 9 H + 17 (T = 11)
  near_anti       ch1 = -float32(ch0 + 1e-4 g2), L = 9 H + 17
  lvl_m56 .. p48  gauss * float32(2^k), k = -56, -20, 20, 48
  short_zero      ch1 = +0, L = N + 1: four frames, the last holds one sample on the window's
                  zero

One cell is not the kernel's to decide (ZERO_SIGN): at N = 512 `short_zero`'s sample N is
negative, so its last frame is [-0, +0, ...] after the window's zero against +0 in ch1 -- silence
in both channels made of mixed-sign zeros. pocketfft's real transform of that frame is +0
everywhere but in bin 205, whose real part is -0: angle pi against 0, weight 1.0, where the
kernel (and the reference in every other bin of the frame) gives 0.01. The decision follows the
zero signs of pocketfft's radix passes and nothing in the input (at N = 1024 the sample is
positive and the frame all 0.01); DESIGN.md section 22.

Reference of a row (reference()): the oracle's complex64 spectra (O.stft), its mask
(O.ipd_mask_noise) with the row sums, the fp64 sums of cov_out[..., 0:4], the tie set (cells
with 0 < |d angle| < 1e-6 rad in fp64: decided by the last bit of each STFT, the criterion of
test_ipd_identical_channels), whether the reference solve at the plan's sigma is well
conditioned in every solved bin, the fp64 waveform, and the per-bin bound of the four sums.

Bound of the sums (sums_bound; u = 2^-24, m the reference weight, p a frame's product
|Y0|^2, |Y1|^2 or, for Re and Im of Y0 conj(Y1), |Y0| |Y1|):
  1. spectra: the kernel's fp32 STFT against the oracle's, the project's pinned tolerance
     delta = 2e-6 max|Y| of the row (test_stft_stage: a rounded window
     and log2 N <= 10 radix stages of a few u each, relative to the frame's largest bin):
     sum m (2 |Y0| delta + delta^2), sum m (2 |Y1| delta + delta^2), and for the cross terms
     sum m ((|Y0| + |Y1|) delta + delta^2);
  2. products: two fp32 roundings each, 2 u sum m p (the same rounded product goes in at
     weight 1 and leaves at weight 1 - w, so its error carries the final weight);
  3. weights: the fix-up's factor w - 1 = 0.01f - 1 is rounded to 2^-25 and 0.01f differs from
     the reference's 0.01 by 2.3e-10: (2^-25 + 2.3e-10) sum over the 0.01 cells of p;
  4. accumulation, inner bins: one fp32 accumulator a chunk (a split chunk: one a piece,
     starting from 0), per step first the frames' products at weight 1 in frame order, then
     (w - 1) p of the 0.01 frames in frame order (a frame at weight 1 adds 0 p: exact). Every
     fma rounds to u |acc|, and |acc| <= (sum of |step sums| so far) + sum_t coef_t p_t with
     coef the frame's weight at that moment; the bound is u times the sum of that over the
     chunk's operations, which holds for the whole chunk and for every piece of it;
  5. accumulation, DC and Nyquist: frame `lane` of each step on its own lane at its final
     weight (at most 4 terms a lane) and a 64-lane butterfly (6 levels): 10 u sum m p;
  6. the chunks' (pieces') partials are added in fp64: nothing at this scale;
  7. underflow: the kernel's window carries scipy's 2 / N and its products are 4 |Y|^2, so at
     2^-56 they are subnormal (4 |Y|^2 is 2e-38 on average, the spectra themselves 1e-19 and
     normal). Under gradual underflow a rounding of a subnormal result errs by 2^-150 at the
     most: 8 roundings a frame, T 8 2^-150 / 4 (nothing at any other level; were the products
     flushed to zero, `lvl_m56` would miss the bound by half its sums).
The bound of a bin is the sum of these; test_ipd_reference.py caps it at SUMS_CAP = 1e-4 of
max(c00, c11) of the bin, under which a flag applied one frame off still shows.

Layouts (functions of R = compute units and n_fft; G = BLOCKS_PER_CU[n_fft] R resident analysis
blocks; every row of a batch takes gx = 2 items, the chunks of the batch's longest row, so the
short rows change no count). Each layout is a list of batches, a batch a list of row names:
  pieces  the rows alone, at most G / 8 a batch: gx B <= G / 4, every item in 4 pieces;
  whole   G / 2 rows, position p holding row (p + p // 16) mod 16: gx B = G, no split, each
          copy of a row in another block and at another place of the cycle;
  mixed   the `whole` batch followed by the rows (at most G / 4 a batch) as a tail of pieces.
"""
import functools

import numpy as np

import stage_cases as SC
import utt_cases as UC
from oracle import avz_oracle as O

SIZES = UC.SIZES
STEP = 8                      # frames of an IPD step (CGeo<N>::NSLOT of the IPD kernels)
CHUNK = UC.CHUNK
PLAN = UC.PLANS["ipd"]
TIE_RAD = 1e-6
STFT_TOL = 2e-6               # BASELINE.md section 4 / test_stft_stage
SUMS_CAP = 1e-4
U32 = 2.0 ** -24
DW = 2.0 ** -25 + abs(float(np.float32(0.01)) - 0.01)
UNDERFLOW = 0.25 * 8 * 2.0 ** -150   # a frame's roundings of subnormal results, in |Y|^2 units

LEVELS = {"lvl_m56": -56, "lvl_m20": -20, "lvl_p20": 20, "lvl_p48": 48}
ROWS = ("gauss", "ch1_zero", "ch0_zero", "ch1_mul0", "ch1_dead_span", "both_zero_span",
        "ident_all", "ident_spans", "anti", "near", "near_anti", "lvl_m56", "lvl_m20", "lvl_p20",
        "lvl_p48", "short_zero")
SILENT = ("ch1_zero", "ch0_zero", "ch1_mul0", "short_zero")
IDENT_FRAMES = (0, 7, 8, 20, 31, 32, 41)
# (size, row): the cells decided by the sign of a pocketfft zero (zero_sign_cells), (bin, frame)
ZERO_SIGN = {(512, "short_zero"): ((205, 3),)}
# rows that share another row's draw: the level rows are `gauss` scaled, `ch1_mul0` keeps
# `ch1_zero`'s ch0 (their masks are compared)
DRAW = dict({k: "gauss" for k in LEVELS}, ch1_mul0="ch1_zero")


def length(n_fft, name):
    H = n_fft // 2
    if name in ("near", "near_anti"):
        return 9 * H + 17
    if name == "short_zero":
        return n_fft + 1
    return 40 * H + 17


def ident_spans(n_fft):
    H, L = n_fft // 2, length(n_fft, "ident_spans")
    return ((0, H), (6 * H, 9 * H), (19 * H, 21 * H), (30 * H, 33 * H), (40 * H, L))


def dead_span(n_fft):
    H = n_fft // 2
    return 12 * H + 37, 18 * H + 101


def both_zero_spans(n_fft):
    H = n_fft // 2
    return ((0, 3 * H), (20 * H + 5, 25 * H + 9))


def silent_frames(n_fft, spans, L):
    """Frames all of whose samples inside [0, L) lie in one of the spans."""
    H = n_fft // 2
    out = []
    for t in range(UC.n_frames(L, n_fft)):
        lo, hi = max(0, (t - 1) * H), min(L, (t + 1) * H)
        if any(a <= lo and hi <= b for a, b in spans):
            out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def row(n_fft, name):
    """mix [2, L] float32 of one row."""
    L = length(n_fft, name)
    draw = ROWS.index(DRAW.get(name, name))
    rng = np.random.default_rng([7700, n_fft, draw])
    g = rng.standard_normal((3, L), dtype=np.float32) * np.float32(0.1)
    ch0, ch1 = g[0].copy(), g[1].copy()
    zero = np.zeros(L, np.float32)
    if name in ("ch1_zero", "short_zero"):
        ch1 = zero
    elif name == "ch0_zero":
        ch0 = zero
    elif name == "ch1_mul0":
        ch1 = ch1 * np.float32(0)
    elif name == "ch1_dead_span":
        a, b = dead_span(n_fft)
        ch1[a:b] = 0
    elif name == "both_zero_span":
        for a, b in both_zero_spans(n_fft):
            ch0[a:b] = 0
            ch1[a:b] = 0
    elif name == "ident_all":
        ch1 = ch0.copy()
    elif name == "ident_spans":
        for a, b in ident_spans(n_fft):
            ch1[a:b] = ch0[a:b]
    elif name == "anti":
        ch1 = -ch0
    elif name in ("near", "near_anti"):
        ch1 = (ch0 + np.float32(1e-4) * g[2]).astype(np.float32)
        ch1 = -ch1 if name == "near_anti" else ch1
    elif name in LEVELS:
        s = np.float32(2.0 ** LEVELS[name])
        ch0, ch1 = ch0 * s, ch1 * s
    else:
        assert name == "gauss", name
    mix = np.stack([ch0, ch1])
    assert mix.dtype == np.float32
    mix.setflags(write=False)
    return mix


def identical_frames(n_fft, name):
    """Frames whose two channels are bitwise identical (zero extension included)."""
    mix = row(n_fft, name)
    H, L = n_fft // 2, mix.shape[1]
    bits = mix.view(np.uint32)
    out = []
    for t in range(UC.n_frames(L, n_fft)):
        lo, hi = max(0, (t - 1) * H), min(L, (t + 1) * H)
        if np.array_equal(bits[0, lo:hi], bits[1, lo:hi]):
            out.append(t)
    return out


# ----------------------------------------------------------------------------- references
def _acc_bound(P, m):
    """Item 4 of the module docstring: [F] from the products' magnitudes P [F, T] and the
    reference weights m [F, T]."""
    F, T = P.shape
    total = np.zeros(F)
    for c0 in range(0, T, CHUNK):
        prev = np.zeros(F)
        for s0 in range(c0, min(T, c0 + CHUNK), STEP):
            ps, ms = P[:, s0:s0 + STEP], m[:, s0:s0 + STEP]
            run = np.cumsum(ps, axis=1)                    # after each product at weight 1
            total += (prev[:, None] + run).sum(axis=1)
            fixed = ms < 1.0
            drop = np.cumsum(np.where(fixed, (1.0 - ms) * ps, 0.0), axis=1)
            after = prev[:, None] + run[:, -1:] - drop      # after each (w - 1) p
            total += np.where(fixed, after, 0.0).sum(axis=1)
            prev = prev + (ms * ps).sum(axis=1)
    return U32 * total


def sums_bound(Y, m):
    """[F, 4]: the bound of |cov_out[..., q] - fp64 sum| per bin (module docstring)."""
    Yd = Y.astype(np.complex128)
    a0, a1 = np.abs(Yd[0]), np.abs(Yd[1])
    delta = STFT_TOL * max(a0.max(), a1.max())
    P = (a0 ** 2, a1 ** 2, a0 * a1, a0 * a1)
    spec = (2 * a0 * delta + delta ** 2, 2 * a1 * delta + delta ** 2,
            (a0 + a1) * delta + delta ** 2, (a0 + a1) * delta + delta ** 2)
    out = np.empty((Y.shape[1], 4))
    for q in range(4):
        b = (m * spec[q]).sum(axis=1) + 2 * U32 * (m * P[q]).sum(axis=1)
        b += DW * np.where(m < 1.0, P[q], 0.0).sum(axis=1)
        acc = _acc_bound(P[q], m)
        acc[[0, -1]] = 10 * U32 * (m * P[q]).sum(axis=1)[[0, -1]]
        out[:, q] = b + acc + UNDERFLOW * Y.shape[2]
    return out


def fp64_sums(Y, m):
    """[F, 4]: sum_t m |Y0|^2, sum_t m |Y1|^2, Re and Im of sum_t m Y0 conj(Y1)."""
    Yd = Y.astype(np.complex128)
    c = (m * Yd[0] * Yd[1].conj()).sum(axis=1)
    return np.stack([(m * np.abs(Yd[0]) ** 2).sum(axis=1), (m * np.abs(Yd[1]) ** 2).sum(axis=1),
                     c.real, c.imag], axis=1)


def tie_cells(Y):
    """[F, T] bool: 0 < |d angle| < TIE_RAD in fp64."""
    ang = np.angle(Y.astype(np.complex128))
    dphi = np.abs(np.angle(np.exp(1j * (ang[0] - ang[1]))))
    return (dphi > 0) & (dphi < TIE_RAD)


def zero_sign_cells(n_fft, name):
    """(bin, frame) of the cells the reference weights 1.0 although both spectra are zero there:
    the angle pi of a -0 real part against the angle 0 of +0."""
    r = reference(n_fft, name)
    z = (r["mask"] == 1.0) & (np.abs(r["Y"][0]) == 0) & (np.abs(r["Y"][1]) == 0)
    return tuple((int(k), int(t)) for k, t in np.argwhere(z))


@functools.lru_cache(maxsize=None)
def reference(n_fft, name):
    """dict(Y [2, F, T] complex64, mask [F, T], rowsum [F], sums [F, 4], bound [F, 4],
    ties [F, T] bool, cond = largest cond_2 of a solved bin, well = cond <= COND_MAX,
    raw [(T - 1) H], peak, out = raw / (peak + norm_eps))."""
    mix = row(n_fft, name)
    H = n_fft // 2
    raw, st = O.masked_mvdr_vec(mix, n_fft=n_fft, hop=H, sigma=PLAN["sigma"], d=PLAN["mic_d"],
                                normalize=False, return_stages=True)
    Y, m = st["Y"], st["mask"].astype(np.float64)
    assert Y.dtype == np.complex64 and m.shape == (H + 1, UC.n_frames(mix.shape[1], n_fft))
    assert np.array_equal(m, O.ipd_mask_noise(O.stft(mix, nperseg=n_fft, noverlap=H)[2]))
    ok = st["f"] >= O.FMIN_MVDR
    cond = float(np.linalg.cond(st["R"][ok] + PLAN["sigma"] * np.eye(2), 2).max())
    raw = np.asarray(raw, np.float64)
    peak = float(np.abs(raw).max())
    return dict(Y=Y, mask=m, rowsum=m.sum(axis=1), sums=fp64_sums(Y, m), bound=sums_bound(Y, m),
                ties=tie_cells(Y), cond=cond, well=cond <= SC.COND_MAX, raw=raw, peak=peak,
                out=raw / (peak + PLAN["norm_eps"]))


# ----------------------------------------------------------------------------- layouts
GX = 2   # items a row: the chunks of a batch's longest row (T = 42)


def grid(R, n_fft):
    return UC.BLOCKS_PER_CU[n_fft] * R


def _groups(names, size):
    assert size >= 1
    return [list(names[i:i + size]) for i in range(0, len(names), size)]


def whole_rows(R, n_fft):
    B = grid(R, n_fft) // GX
    return [ROWS[(p + p // len(ROWS)) % len(ROWS)] for p in range(B)]


def layout(kind, R, n_fft):
    """The batches of one layout: a list of lists of row names."""
    G = grid(R, n_fft)
    if kind == "pieces":
        return _groups(ROWS, G // (4 * GX))
    if kind == "whole":
        return [whole_rows(R, n_fft)]
    assert kind == "mixed", kind
    return [whole_rows(R, n_fft) + tail for tail in _groups(ROWS, G // (2 * GX))]


LAYOUTS = ("pieces", "whole", "mixed")


def split_of(n_rows, R, n_fft, slots=768):
    """(whole items, pieces a tail item) of a batch of n_rows rows: analysis_tail of
    csrc/avz_chunked.hip with the IPD kernels' 4 steps a chunk and the workspace's tail slots
    (min(8 gx B, 768): never the binding term here)."""
    G, n_items = grid(R, n_fft), GX * n_rows
    whole = n_items // G * G
    tail = n_items - whole
    for q in (4, 2):
        if tail > 0 and tail * q <= G and tail * q <= min(8 * n_items, slots):
            return whole, q
    return n_items, 1


def batch(n_fft, names):
    """(mix [B, 2, S] float32 zero beyond each row's length, lens [B] int32); S = the longest
    row rounded up to 4 samples."""
    lens = np.array([length(n_fft, k) for k in names], np.int32)
    S = (int(lens.max()) + 3) // 4 * 4
    mix = np.zeros((len(names), 2, S), np.float32)
    for b, k in enumerate(names):
        mix[b, :, :lens[b]] = row(n_fft, k)
    return mix, lens
