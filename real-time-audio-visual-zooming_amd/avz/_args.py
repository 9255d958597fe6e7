"""Tensor-argument checks of the host wrappers: the one place a caller's tensor is looked at
before its address goes to the library. Needs torch and ctypes only;
the library is loaded at the first ``call``.

A shape spec is a tuple with one entry per dimension: an int is the exact extent, ``ge(n)`` at
least n, None any. A bare ``ge(n)`` in place of the tuple asks for at least n elements of any
rank. A device spec is a ``torch.device`` (that very device) or a type name ("cuda": any
GPU, what a wrapper asks of its primary input).

These run on every call of MVDRPlan.run, so they are written for speed: ``ge(n)`` is the
negative int ~n (an extent is never negative), not an object."""
from __future__ import annotations

import ctypes as ct
from operator import inv as ge  # noqa: F401  ge(n) = ~n: "at least n" in a shape spec

import torch

LAST, FULL, ANY = "last dimension contiguous", "contiguous", "any strides"


def tensor(name, t, dtype, shape, device, contig=LAST):
    """``t`` if it has the dtype, the shape (see the module text), the device and the strides
    asked for; ValueError otherwise."""
    ok = t.dtype == dtype and (t.device == device if type(device) is not str
                               else t.is_cuda if device == "cuda" else t.device.type == device)
    if ok and type(shape) is tuple:
        have = t.shape
        ok = len(have) == len(shape)
        if ok:
            for h, w in zip(have, shape):
                if w is not None and (h != w if w >= 0 else h < ~w):
                    ok = False
                    break
        if ok and contig is not ANY:
            ok = t.is_contiguous() if contig is FULL else not have or t.stride()[-1] == 1
    elif ok:
        ok = t.numel() >= ~shape and (contig is ANY or t.is_contiguous())
    if not ok:
        say = lambda w: "*" if w is None else str(w) if w >= 0 else f">= {~w}"  # noqa: E731
        want = (f"[{', '.join(map(say, shape))}]" if type(shape) is tuple
                else f"{say(shape)} elements")
        raise ValueError(f"{name} must be a {dtype} tensor of {want} ({contig}) on {device}; got "
                         f"{t.dtype} {list(t.shape)}, strides {list(t.stride())}, on {t.device}")
    return t


def mic_pair(name, x, device="cuda"):
    """A float32 [B, 2, S] mic pair, samples contiguous: (B, S, its device)."""
    B, _, S = tensor(name, x, torch.float32, (None, 2, None), device).shape
    return B, S, x.device


def lengths(lens, max_len, B, S, device, contig=ANY):
    """(lengths, max_len) of a batch of B rows of S samples: full rows when ``lens`` is None
    (a given max_len is ignored, as ever), else a checked int32 [>= B] tensor on the device
    and max_len, by default the largest of its first B entries."""
    if lens is None:
        return torch.full((B,), S, dtype=torch.int32, device=device), S
    tensor("lengths", lens, torch.int32, (ge(B),), device, contig)
    if max_len is None:
        max_len = lens[:B].max().item()
    return lens, int(max_len)


def hop_block(mix, hop, device="cuda"):
    """(streams, hops) of a pushed block: a mic pair [streams, 2, hops * hop], hops >= 1."""
    streams, n, _ = mic_pair("mix", mix, device)
    if n == 0 or n % hop:
        raise ValueError(f"mix must hold a whole number (>= 1) of hops of {hop} samples; "
                         f"got {n}")
    return streams, n // hop


def outputs(table, device):
    """Optional outputs, rows of (name, tensor or None, shape spec, dtype): every tensor
    given is contiguous, of that shape and dtype, on the device."""
    for name, t, shape, dtype in table:
        if t is not None:
            tensor(name, t, dtype, shape, device, FULL)


def features(layout, B, F, T, device):
    """A zeroed mask-model feature tensor and its (batch, channel, bin, frame) strides:
    "unet" [B, 2, F, T], "tflite" [B, F, T, 4]."""
    if layout == "unet":
        out = torch.zeros((B, 2, F, T), dtype=torch.float32, device=device)
        sb, sc, sf, st = out.stride()
    elif layout == "tflite":
        out = torch.zeros((B, F, T, 4), dtype=torch.float32, device=device)
        sb, sf, st, sc = out.stride()
    else:
        raise ValueError(f"unknown feature layout {layout!r}")
    return out, (sb, sc, sf, st)


def ptr(t):
    return None if t is None else ct.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_handle(stream):
    """The stream's handle; None: the current device's current stream (read without building
    a torch.cuda.Stream where this torch can: it is most of a small call's host time)."""
    if stream is not None:
        return ct.c_void_p(stream.cuda_stream)
    if _raw_stream is not None:
        return ct.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


_lib = None     # avz._lib, loaded by the first call


def call(name, *args, stream=None, device=None):
    """check(lib.<name>(*args, the stream's handle)); ``device``: made current for the call
    (the wrappers whose entry point launches on the current device give their tensors')."""
    global _lib
    if _lib is None:
        from . import _lib
    fn = getattr(_lib.lib, name)
    if device is None:
        rc = fn(*args, stream_handle(stream))
    else:
        with torch.cuda.device(device):     # the default stream looked up is that device's
            rc = fn(*args, stream_handle(stream))
    return rc if rc >= 0 else _lib.check(rc, name)     # check raises: rc < 0
