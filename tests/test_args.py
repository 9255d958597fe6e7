"""avz/_args.py on its own: the tensor-argument checks every host wrapper goes through. Loaded
from its file, so neither the package nor libavz.so is needed; host tensors stand in for
device ones (the device spec is a parameter)."""
import importlib.util
import os

import pytest
import torch

from conftest import PKG

_spec = importlib.util.spec_from_file_location("avz_args_alone",
                                               os.path.join(PKG, "avz", "_args.py"))
A = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(A)
ge = A.ge
CPU = torch.device("cpu")
F32, I32 = torch.float32, torch.int32


def rejects(*args, **kw):
    with pytest.raises(ValueError):
        A.tensor("t", *args, **kw)


def test_loads_without_the_library():
    assert A._lib is None


def test_dtype_and_rank():
    t = torch.zeros((3, 5), dtype=F32)
    assert A.tensor("t", t, F32, (3, 5), CPU) is t
    rejects(t, torch.float64, (3, 5), CPU)
    rejects(t.to(I32), F32, (3, 5), CPU)
    rejects(t, F32, (3, 5, 1), CPU)
    rejects(t, F32, (15,), CPU)
    rejects(t[0], F32, (3, 5), CPU)


def test_exact_and_at_least_extents():
    t = torch.zeros((3, 5), dtype=F32)
    A.tensor("t", t, F32, (3, ge(5)), CPU)
    A.tensor("t", t, F32, (ge(2), ge(4)), CPU)
    A.tensor("t", t, F32, (None, 5), CPU)
    rejects(t, F32, (2, 5), CPU)            # exact: larger is wrong too
    rejects(t, F32, (4, 5), CPU)
    rejects(t, F32, (3, ge(6)), CPU)
    rejects(t, F32, (ge(4), None), CPU)
    # a bare ge(n): that many elements, any rank
    A.tensor("t", t, F32, ge(15), CPU)
    A.tensor("t", t.reshape(15), F32, ge(0), CPU)
    rejects(t, F32, ge(16), CPU)


def test_contiguity_rules():
    base = torch.zeros((4, 6, 8), dtype=F32)
    rows = base[:, ::2]                       # last dimension dense, not contiguous
    cols = base[:, :, ::2]                    # last dimension strided
    for contig in (A.LAST, A.FULL, A.ANY):
        A.tensor("t", base, F32, (4, 6, 8), CPU, contig)
    A.tensor("t", rows, F32, (4, 3, 8), CPU)            # the default: LAST
    A.tensor("t", rows, F32, (4, 3, 8), CPU, A.ANY)
    rejects(rows, F32, (4, 3, 8), CPU, A.FULL)
    A.tensor("t", cols, F32, (4, 6, 4), CPU, A.ANY)
    rejects(cols, F32, (4, 6, 4), CPU, A.LAST)
    rejects(cols, F32, (4, 6, 4), CPU, A.FULL)


def test_device():
    t = torch.zeros((2, 3), dtype=F32)
    A.tensor("t", t, F32, (2, 3), "cpu")
    rejects(t, F32, (2, 3), "cuda")                       # any GPU: a host tensor is none
    rejects(t, F32, (2, 3), torch.device("cuda", 0))
    rejects(t.to("meta"), F32, (2, 3), CPU)


def test_mic_pair():
    x = torch.zeros((3, 2, 40), dtype=F32)
    assert A.mic_pair("x", x, "cpu") == (3, 40, CPU)
    for bad in (x[:, :1], x[0], x.double(), x[:, :, ::2], torch.zeros((3, 3, 40))):
        with pytest.raises(ValueError):
            A.mic_pair("x", bad, "cpu")
    with pytest.raises(ValueError):
        A.mic_pair("x", x)                                # the default asks for a GPU


def test_lengths_three_forms():
    B, S = 3, 100
    full, m = A.lengths(None, 17, B, S, CPU)              # None: full rows, max_len ignored
    assert m == S and full.dtype == I32 and full.tolist() == [S] * B
    lens = torch.tensor([40, 70, 55, 99], dtype=I32)      # one entry more than B
    got, m = A.lengths(lens, None, B, S, CPU)
    assert got is lens and m == 70 and type(m) is int     # the largest of the first B
    got, m = A.lengths(lens, 64, B, S, CPU)
    assert got is lens and m == 64
    for bad in (lens.long(), lens[:2], lens[None], lens.float()):
        with pytest.raises(ValueError):
            A.lengths(bad, None, B, S, CPU)
    with pytest.raises(ValueError):
        A.lengths(lens, None, B, S, "cuda")
    A.lengths(lens[::2], None, 2, S, CPU)                 # strides: the caller's rule
    with pytest.raises(ValueError):
        A.lengths(lens[::2], None, 2, S, CPU, A.FULL)


def test_hop_block():
    hop = 16
    assert A.hop_block(torch.zeros((3, 2, hop), dtype=F32), hop, "cpu") == (3, 1)
    assert A.hop_block(torch.zeros((1, 2, 9 * hop), dtype=F32), hop, "cpu") == (1, 9)
    for n in (0, hop - 1, hop + 1, 3 * hop + 8):
        with pytest.raises(ValueError):
            A.hop_block(torch.zeros((3, 2, n), dtype=F32), hop, "cpu")
    with pytest.raises(ValueError):
        A.hop_block(torch.zeros((3, 1, hop), dtype=F32), hop, "cpu")


def test_outputs_table():
    w = torch.zeros((2, 5, 4), dtype=F32)
    c = torch.zeros((2, 5, 5), dtype=torch.float64)
    A.outputs((("w", w, (2, 5, 4), F32), ("c", c, ge(50), torch.float64),
               ("absent", None, (1,), F32)), CPU)
    for row in (("w", w, (2, 5, 5), F32), ("w", w, (2, 5, 4), torch.float64),
                ("w", w.transpose(0, 1), (5, 2, 4), F32), ("c", c, ge(51), torch.float64)):
        with pytest.raises(ValueError):
            A.outputs((row,), CPU)
    with pytest.raises(ValueError):
        A.outputs((("w", w, (2, 5, 4), F32),), "cuda")


def test_features_layouts():
    out, (sb, sc, sf, st) = A.features("unet", 2, 5, 7, CPU)
    assert out.shape == (2, 2, 5, 7) and (sb, sc, sf, st) == out.stride()
    out, (sb, sc, sf, st) = A.features("tflite", 2, 5, 7, CPU)
    assert out.shape == (2, 5, 7, 4) and (sb, sf, st, sc) == out.stride()
    assert not out.any()
    with pytest.raises(ValueError):
        A.features("other", 2, 5, 7, CPU)


def test_ptr():
    t = torch.zeros(4, dtype=F32)
    assert A.ptr(None) is None
    assert A.ptr(t).value == t.data_ptr() and A.ptr(t[1:]).value == t.data_ptr() + 4
