"""The STOI restatement (avz.stoi.stoi_numpy) against an independent long-double statement,
its pinned values and properties, the edge cases of the frame rules, the host-side argument
checks of avz_stoi_batch and run_batch(..., stoi=True) on the CPU. No GPU: the kernel's
comparison with the restatement is tests/test_gpu_stoi.py."""
import ctypes as ct
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import stoi_cases as C
from avz import stoi as S
from test_distributed import oracle_enhance

needs_ld = pytest.mark.skipif(not C.HAVE_LD, reason="no extended-precision long double")


def test_band_table_and_constants():
    assert S.BANDS == C.BAND_TABLE
    h = S.resample_taps()
    assert len(h) == 581 and np.array_equal(h, h[::-1])
    assert np.array_equal(S.window(), np.hanning(258)[1:-1])


def test_library_taps_match_the_design():
    """The host-built h' the resampler kernel receives against 5 h / sum h of resample_taps:
    2^-23 of a sample is the stage's budget, the two Kaiser evaluations agree to 1e-14."""
    from avz import _lib
    t = (ct.c_double * 291)()
    assert _lib.lib.avz_stoi_taps(t) == 0
    h = S.resample_taps()
    assert np.abs(np.array(t) - (5 * h / h.sum())[290:]).max() <= 1e-14


@needs_ld
@pytest.mark.parametrize("n", [1000, 1003, 16000])
def test_polyphase_sum_is_resample_poly(n):
    s = np.random.default_rng(n).standard_normal(n)
    a, b = S.resample(s, 16000), C.resample_ld(s, 16000)
    assert len(a) == len(b) == S.resampled_len(n, 16000)
    assert np.abs(a - b).max() <= 1e-14


def test_pinned_values_of_the_test_triple():
    tgt, mix0, est = C.full_triple()
    info = S.stoi_info_numpy(tgt, mix0)
    assert (info["frames"], info["kept"]) == (641, 470)
    assert abs(info["margin_db"] - 0.11) < 0.01
    assert abs(S.stoi_numpy(tgt, tgt) - 1.0) <= 1e-12
    d_est = S.stoi_numpy(tgt, est)
    # DESIGN.md section 11 records seven decimals; the full values are pinned to 1e-9
    assert round(info["d"], 7) == C.PINNED["mix0"] and round(d_est, 7) == C.PINNED["est16"]
    assert abs(info["d"] - 0.6003809169239133) <= 1e-9
    assert abs(d_est - 0.9427482912013997) <= 1e-9
    for s, margin in zip(C.EXCERPTS, (0.048, 1.6)):
        m = S.stoi_info_numpy(tgt[s:s + 16000], mix0[s:s + 16000])["margin_db"]
        assert abs(m - margin) <= 0.05 * margin


@needs_ld
def test_restatement_against_the_independent_statement():
    """E_ref of every GPU case, and of the full triple's first 2 s: the two statements share
    no transform, resampler or segment code and agree to a few ulp of d."""
    worst = 0.0
    for c in C.GPU_CASES:
        for r in C.case_reference(c.name):
            assert r["st"]["status"] == r["ld"]["status"]
            assert r["st"]["frames"] == r["ld"]["frames"] and len(r["st"]["keep"]) == r["ld"]["kept"]
            assert r["E_res"] <= 1e-14
            worst = max(worst, r["E_ref"])
    tgt, mix0, _ = C.full_triple()
    r = C.pair_reference(tgt[:32000], mix0[:32000], 16000)
    worst = max(worst, r["E_ref"])
    print(f"worst E_ref = {worst:.2e}")
    assert worst <= 1e-12


def test_gpu_cases_meet_the_margin_condition_and_the_speech_bound():
    for c in C.GPU_CASES:
        for i, r in enumerate(C.case_reference(c.name)):
            assert r["margin_db"] >= C.MARGIN_DB, (c.name, i)
            if c.speech and r["st"]["status"] == 0:
                assert r["tol"] < 5e-5, (c.name, i, r["tol"])


def test_monotone_in_snr_and_scale_invariant():
    tgt, _, _ = C.full_triple()
    x = tgt[40000:56000]
    noise = np.random.default_rng(5).standard_normal(len(x))
    noise *= np.sqrt(np.mean(x.astype(np.float64) ** 2) / np.mean(noise ** 2))
    d = [S.stoi_numpy(x, x + 10 ** (-snr / 20) * noise) for snr in (20, 10, 0, -10)]
    assert d[0] > d[1] > d[2] > d[3], d
    y = x + 0.3 * noise
    assert abs(S.stoi_numpy(x, 1e-4 * y) - S.stoi_numpy(x, y)) <= 1e-9


def test_edge_cases_of_the_frame_rules():
    refs = C.case_reference("too-short")
    info = [(r["st"]["status"], r["st"]["frames"], len(r["st"]["keep"])) for r in refs]
    assert info == [(1, 30, 30), (0, 31, 31), (1, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0)]
    assert [r["st"]["d"] for r in refs if r["st"]["status"] == 1] == [1e-5] * 5
    assert refs[1]["st"]["xb"].shape[1] == 30                      # K = 31: one segment
    fr = C.case_reference("frame-rule")
    assert (fr[0]["st"]["frames"], fr[1]["st"]["frames"]) == (40, 41)  # the exact fit is not taken
    x = C.stationary(4000, 1).astype(np.float64)
    x[700] = np.nan
    assert np.isnan(S.stoi_numpy(x, x, 10000)) and S.stoi_stages(x, x, 10000)["status"] == 2


def test_host_side_argument_checks():
    """Validation happens before any device work: the pointers are never followed."""
    from avz import _lib
    lib = _lib.lib
    assert lib.avz_stoi_batch(None, None) == _lib.AVZ_ERR_ARG
    need = lib.avz_stoi_workspace_bytes(2, 16000, 16000.0)
    assert need > 0 and lib.avz_stoi_workspace_bytes(2, 16000, 8000.0) == _lib.AVZ_ERR_UNSUPPORTED
    assert lib.avz_stoi_workspace_bytes(-1, 16000, 16000.0) == _lib.AVZ_ERR_SHAPE

    def call(**kw):
        a = _lib.AvzStoiArgs()
        a.batch, a.max_len, a.fs = 2, 16000, 16000.0
        a.clean, a.est, a.stoi, a.workspace = 0x1000, 0x2000, 0x3000, 0x4000
        a.clean_stride = a.est_stride = 16000
        a.workspace_bytes = need
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.avz_stoi_batch(ct.byref(a), None)

    assert call(fs=8000.0) == _lib.AVZ_ERR_UNSUPPORTED
    for k in ("clean", "est", "stoi", "workspace"):
        assert call(**{k: None}) == _lib.AVZ_ERR_ARG, k
    assert call(workspace_bytes=need - 1) == _lib.AVZ_ERR_SHAPE
    assert call(clean_stride=15999) == _lib.AVZ_ERR_SHAPE
    assert call(resampled=0x5000, res_stride=9999) == _lib.AVZ_ERR_SHAPE
    assert call(tob=0x6000, tob_stride=75) == _lib.AVZ_ERR_SHAPE
    assert call(stoi=0x3004) == _lib.AVZ_ERR_ALIGN
    assert call(batch=0, clean=None) == _lib.AVZ_OK
    assert lib.avz_version() == 3


# ----------------------------------------------------------------------------
# the batch driver on the CPU
# ----------------------------------------------------------------------------
N_RUNS, START, SECONDS = 5, 3, 1.0


def _run(stoi, **kw):
    from avz import batch_run
    return batch_run.run_batch(N_RUNS, start_idx=START, n_interferers=2, seconds=SECONDS, batch=2,
                               device="cpu", enhance=oracle_enhance, stoi=stoi, **kw)


@pytest.fixture(scope="module")
def single():
    return _run(True)


def test_run_batch_cpu_rows_match_the_restatement(single):
    from avz import synth
    plain = _run(False)
    assert plain.stoi_sums is None and all(r["STOI"] == "0.0000" for r in plain.rows)
    assert np.array_equal(single.sums, plain.sums)                 # bitwise
    strip = lambda rows: [{k: v for k, v in r.items() if k != "STOI"} for r in rows]  # noqa: E731
    assert strip(single.rows) == strip(plain.rows)
    mix, tgt, itf = synth.make_batch_philox(N_RUNS, start=START, n_samples=16000, n_interferers=2)
    out = oracle_enhance(*(torch.from_numpy(a) for a in (mix, tgt, itf))).numpy()
    L = min(out.shape[-1], 16000)
    d_in = [S.stoi_numpy(tgt[b, :L], mix[b, 0, :L]) for b in range(N_RUNS)]
    d_out = [S.stoi_numpy(tgt[b, :L], out[b, :L]) for b in range(N_RUNS)]
    assert [r["STOI"] for r in single.rows] == [f"{d:.4f}" for d in d_out]
    np.testing.assert_allclose(single.stoi_sums, [sum(d_in), sum(d_out), N_RUNS], rtol=1e-12)
    assert all(0.3 < a < b <= 1.0 for a, b in zip(d_in, d_out))    # the mask helps every scene


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, outdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = _run(True)
    np.save(os.path.join(outdir, f"stoi_sums_{rank}.npy"), res.stoi_sums)
    np.save(os.path.join(outdir, f"sums_{rank}.npy"), res.sums)
    dist.destroy_process_group()


def test_two_rank_gloo_gives_the_single_process_stoi_sums(single, tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        np.testing.assert_allclose(np.load(tmp_path / f"stoi_sums_{r}.npy"), single.stoi_sums,
                                   rtol=1e-12)
        np.testing.assert_allclose(np.load(tmp_path / f"sums_{r}.npy"), single.sums, rtol=1e-12)
