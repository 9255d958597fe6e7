"""avz_stoi_batch (csrc/avz_stoi.hip) against the fp64 restatement avz.stoi.stoi_numpy.

Per pair the kernel's d must sit within 1e-6 + 4 E_ref + 4 E_pert of the restatement's
(tests/stoi_cases.py: E_ref the restatement's own error against the long-double statement,
E_pert its sensitivity to a 2e-6 max|X| perturbation of the frame spectra, the bound
test_stft_stage holds the engine's fp32 transforms to). Every case keeps its keep-decision
margin at or above 1e-3 dB (asserted), so the kernel's kept-frame count must equal the
restatement's with no allowance. Worst observed ratios: DESIGN.md section 11."""
import ctypes as ct

import numpy as np
import pytest
import torch

import stoi_cases as C
from avz import stoi as S
from conftest import golden

pytestmark = pytest.mark.gpu

FFT_BOUND = C.PERTURBATION


def run_case(name, dev, exports=False, pad=(0, 0)):
    """One kernel call on the case's batch; rows are slices of larger arrays (row strides
    longer than the rows, different for the two signals) when pad is given."""
    clean, est, lens = C.case_batch(name)
    fs = next(c.fs for c in C.GPU_CASES if c.name == name)
    B, L = clean.shape
    big_c = torch.full((B, L + pad[0]), 3.0, dtype=torch.float32, device=dev)
    big_e = torch.full((B, L + pad[1]), -3.0, dtype=torch.float32, device=dev)
    big_c[:, :L], big_e[:, :L] = torch.from_numpy(clean).to(dev), torch.from_numpy(est).to(dev)
    kw = {}
    if exports:
        n10 = S.resampled_len(L, fs)
        nf = len(S.frame_starts(n10))
        kw["resampled"] = torch.full((B, 2, n10 + 3), 9.0, dtype=torch.float32, device=dev)
        kw["tob"] = torch.full((B, 2, 15, max(nf - 1, 0) + 2), -1.0, dtype=torch.float64, device=dev)
    d, info = S.stoi_batch(big_c[:, :L], big_e[:, :L],
                           lengths=torch.tensor(lens, dtype=torch.int32, device=dev), fs=fs, **kw)
    torch.cuda.synchronize()
    return d.cpu().numpy(), info.cpu().numpy(), {k: v.cpu().numpy() for k, v in kw.items()}, lens


def check_case(name, d, info):
    worst = 0.0
    for b, r in enumerate(C.case_reference(name)):
        st = r["st"]
        assert r["margin_db"] >= C.MARGIN_DB, (name, b, r["margin_db"])
        J = len(st["keep"]) - 1
        expect = (st["status"], st["frames"], len(st["keep"]), max(J - S.SEG + 1, 0))
        assert tuple(info[b]) == expect, (name, b, tuple(info[b]), expect)
        err = abs(d[b] - st["d"])
        print(f"{name}[{b}]: d {d[b]:.10f} error {err:.3e} tolerance {r['tol']:.3e} "
              f"ratio {err / r['tol']:.3f} (E_ref {r['E_ref']:.1e}, E_pert {r['E_pert']:.1e})")
        if st["status"] == 1:
            assert d[b] == 1e-5
        assert err <= r["tol"], (name, b, err, r["tol"])
        worst = max(worst, err / r["tol"])
    return worst


@pytest.mark.parametrize("case", C.GPU_CASES, ids=lambda c: c.name)
def test_kernel_matches_the_restatement(gpu_device, case):
    pad = (5, 130) if case.name == "fs10k-ragged" else (0, 0)
    d, info, _, _ = run_case(case.name, gpu_device, pad=pad)
    check_case(case.name, d, info)
    if case.speech:                                   # the report's four printed decimals
        assert all(r["tol"] < 5e-5 for r in C.case_reference(case.name))
    if case.name == "scaled-y":                       # y 80 dB down: the same score
        assert abs(d[1] - d[0]) <= C.case_reference(case.name)[0]["tol"]
    if case.name == "identity":
        assert abs(d[0] - 1.0) <= C.case_reference(case.name)[0]["tol"]


@pytest.mark.parametrize("name", ["fs16k-excerpts", "philox-scene", "tile-plus-one", "scaled-y"])
def test_stage_exports(gpu_device, name):
    d, info, ex, lens = run_case(name, gpu_device, exports=True)
    d0, info0, _, _ = run_case(name, gpu_device)
    assert np.array_equal(d, d0) and np.array_equal(info, info0)   # the exports change nothing
    for b, r in enumerate(C.case_reference(name)):
        st = r["st"]
        n10 = len(st["x10"])
        for s, ref in enumerate((st["x10"], st["y10"])):
            got = ex["resampled"][b, s]
            tol = 2.0 ** -23 * np.abs(ref).max() + 4 * r["E_res"]
            err = np.abs(got[:n10] - ref).max()
            print(f"{name}[{b}] resampled[{s}]: error / tolerance = {err / tol:.3f}")
            assert err <= tol
            assert np.all(got[n10:] == 9.0)                        # nothing beyond the row
        J = len(st["keep"]) - 1
        spec = (S.frame_spectra(st["xs"]), S.frame_spectra(st["ys"]))
        for s, ref in enumerate((st["xb"], st["yb"])):
            got = ex["tob"][b, s]
            # a band value is the 2-norm of its bins: an error of FFT_BOUND max|X| per bin
            # moves it by at most sqrt(bins) times that
            tol = np.array([np.sqrt(hi - lo) for lo, hi in S.BANDS])[:, None] \
                * FFT_BOUND * np.abs(spec[s]).max()
            err = np.abs(got[:, :J] - ref)
            print(f"{name}[{b}] tob[{s}]: worst error / tolerance = {(err / tol).max():.3f}")
            assert np.all(err <= tol)
            assert np.all(got[:, J:] == -1.0)                      # nothing beyond frame J


def test_repeatable_and_isolated(gpu_device):
    dev = gpu_device
    clean, est, lens = C.case_batch("fs16k-excerpts")
    c, e = torch.from_numpy(clean).to(dev), torch.from_numpy(est).to(dev)
    tob = [torch.zeros((len(lens), 2, 15, 80), dtype=torch.float64, device=dev) for _ in range(2)]
    d1, i1 = S.stoi_batch(c, e, fs=16000, tob=tob[0])
    d2, i2 = S.stoi_batch(c, e, fs=16000, tob=tob[1])
    assert torch.equal(d1, d2) and torch.equal(i1, i2) and torch.equal(tob[0], tob[1])
    # one utterance of NaNs: its d is NaN, the others' bits do not move
    c2, e2 = c.clone(), e.clone()
    c2[1], e2[1] = float("nan"), float("nan")
    d3, i3 = S.stoi_batch(c2, e2, fs=16000)
    keep = [0, 2, 3]
    assert torch.equal(d3[keep], d1[keep]) and torch.equal(i3[keep], i1[keep])
    assert bool(torch.isnan(d3[1])) and int(i3[1, 0]) == S.STATUS_NONFINITE
    e2 = e.clone()
    e2[2, 5000] = float("nan")                        # a NaN in y alone stays in that row's d
    d4, i4 = S.stoi_batch(c, e2, fs=16000)
    assert bool(torch.isnan(d4[2])) and torch.equal(d4[[0, 1, 3]], d1[[0, 1, 3]])
    assert torch.equal(i4, i1)
    # lengths outside [0, max_len] are clamped
    lens_t = torch.tensor([10 ** 9, -4, 16000, 16000], dtype=torch.int32, device=dev)
    d5, i5 = S.stoi_batch(c, e, lengths=lens_t, fs=16000)
    assert torch.equal(d5[[0, 2, 3]], d1[[0, 2, 3]]) and float(d5[1]) == 1e-5
    assert i5[1].tolist() == [1, 0, 0, 0]


def test_evaluate_run_with_stoi(gpu_device, tmp_path):
    """The report folder of test_gpu_host.test_evaluate_run_report_matches_reference with
    stoi=True: every line but Date and STOI equals the golden report."""
    from avz import metrics, wavio
    g, inp = golden("report_test.npz"), golden("inputs_test.npz")
    sim = tmp_path / "simulated" / "golden_run"
    res = tmp_path / "results" / "golden_run_results"
    sim.mkdir(parents=True)
    res.mkdir(parents=True)
    f = lambda a: a.astype(np.float64) / 32768.0  # noqa: E731
    wavio.write(str(sim / "mixture.wav"), f(inp["mix"]), 16000)
    wavio.write(str(sim / "target.wav"), np.stack([f(inp["tgt"])] * 2, 1), 16000)
    wavio.write(str(sim / "interference.wav"), np.stack([f(inp["int"])] * 2, 1), 16000)
    wavio.write(str(res / "golden_run_enhanced.wav"), f(g["est16"]), 16000)
    m = metrics.evaluate_run("golden_run", sim_dir_root=str(tmp_path / "simulated"),
                             results_dir=str(tmp_path / "results"), stoi=True)
    s_est, s_tgt, _, _ = metrics.load_and_align(str(sim), str(res / "golden_run_enhanced.wav"))
    d_ref = S.stoi_numpy(s_tgt, s_est)
    print(f"evaluate_run: stoi {m['stoi']:.10f}, restatement {d_ref:.10f}, "
          f"difference {abs(m['stoi'] - d_ref):.3e}")
    got = (res / "report.txt").read_text().splitlines()
    ref = str(g["report"]).splitlines()
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        if a.startswith("  STOI:"):
            assert a == f"  STOI:  {d_ref:.4f}"
        elif not a.startswith("Date:"):
            assert a == b
    row = (tmp_path / "results" / "batch_metrics.csv").read_text().splitlines()[1].split(",")
    assert row[6] == f"{d_ref:.4f}"


def test_run_batch_with_stoi(gpu_device):
    """run_batch(4, seconds=1.0, stoi=True) against the stoi=False run and the restatement.

    The device `sums` of two runs cannot be compared bitwise, with or without STOI:
    avz_projection_metrics adds each inner product's block partials (4 blocks of 4096 samples
    here) with fp64 atomics in arrival order, and two stoi=False runs on the same bits were
    measured 7.1e-15 dB apart. So bitwise equality is asserted on every tensor that enters
    the sums (scenes, outputs, peaks), the rows' other columns must be the same strings, and
    the sums themselves must agree within that kernel's own reordering bound: per inner
    product (blocks - 1) 2^-53 of the summed magnitudes for each run, the six products
    entering a metric at most squared, 10 / ln 10 dB per unit of relative error, and an
    allowance of 1e3 for the cancellation in <o, i> (an enhanced output's interference
    projection sits up to 60 dB under sqrt(<o, o> <i, i>)). The CPU driver's sums are
    compared bitwise in test_stoi_reference.py."""
    from avz import batch_run
    n, S16 = 4, 16000
    base = batch_run.gpu_enhancer(max_batch=n, max_samples=S16, device=gpu_device)
    seen = []

    def enhance(mix, tgt, itf):
        out, peak = base(mix, tgt, itf)
        seen.append([t.clone() for t in (mix, tgt, itf, out, peak)])
        return out, peak

    with_stoi = batch_run.run_batch(n, seconds=1.0, batch=n, enhance=enhance, stoi=True)
    plain = batch_run.run_batch(n, seconds=1.0, batch=n, enhance=enhance)
    assert plain.stoi_sums is None and all(r["STOI"] == "0.0000" for r in plain.rows)
    assert all(torch.equal(a, b) for a, b in zip(seen[0], seen[1]))              # bitwise
    strip = lambda rows: [{k: v for k, v in r.items() if k != "STOI"} for r in rows]  # noqa: E731
    assert strip(with_stoi.rows) == strip(plain.rows)
    blocks = -(-S16 // 4096)
    bound = n * (10 / np.log(10)) * 2 * 6 * 2 * (blocks - 1) * 2.0 ** -53 * 1e3
    diff = np.abs(with_stoi.sums - plain.sums)
    print(f"run_batch: max |sums(stoi) - sums(plain)| = {diff.max():.3e} dB, bound {bound:.3e}")
    assert np.all(diff[:4] <= bound) and np.array_equal(with_stoi.sums[4:], plain.sums[4:])
    mix, tgt, out = (seen[0][i].cpu().numpy() for i in (0, 1, 3))
    L = min(out.shape[-1], S16)
    total = np.zeros(2)
    tol_sum = 0.0
    for b in range(n):
        r_in = C.pair_reference(tgt[b, :L], mix[b, 0, :L], 16000)
        r_out = C.pair_reference(tgt[b, :L], out[b, :L], 16000)
        assert r_in["margin_db"] >= C.MARGIN_DB
        col = float(with_stoi.rows[b]["STOI"])
        print(f"run_batch[{b}]: STOI column {col:.4f}, restatement {r_out['st']['d']:.7f}, "
              f"tolerance {r_out['tol']:.2e}")
        assert abs(col - r_out["st"]["d"]) <= r_out["tol"] + 0.5e-4     # four printed decimals
        total += r_in["st"]["d"], r_out["st"]["d"]
        tol_sum += r_in["tol"] + r_out["tol"]
    assert with_stoi.stoi_sums[2] == n
    err = np.abs(with_stoi.stoi_sums[:2] - total)
    print(f"run_batch: stoi_sums error {err.max():.3e}, summed tolerance {tol_sum:.3e}")
    assert np.all(err <= tol_sum)


def test_integration_shim_stoi(gpu_device):
    """INTEGRATION.md's reference-side `stoi`, executed as printed (library path substituted)."""
    import os
    import re
    import textwrap
    from avz import _lib
    from conftest import ROOT
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    code = textwrap.dedent(re.findall(r"```python\n(.*?)```", text, re.S)[0])
    ns = {}
    exec(compile(code.replace('"/path/to/libavz.so"', repr(_lib.LIB_PATH)), "avz_backend", "exec"),
         ns)
    x, y = C.case_pairs("fs16k-excerpts")[0]
    r = C.case_reference("fs16k-excerpts")[0]
    assert abs(ns["stoi"](x, y, 16000) - r["st"]["d"]) <= r["tol"]


def test_host_only_argument_checks(gpu_device):
    from avz import _lib
    lib = _lib.lib
    ws = torch.empty(S.workspace_bytes(1, 16000), dtype=torch.uint8, device=gpu_device)
    x = torch.zeros((1, 16000), dtype=torch.float32, device=gpu_device)
    d = torch.zeros(1, dtype=torch.float64, device=gpu_device)

    def call(**kw):
        a = _lib.AvzStoiArgs()
        a.batch, a.max_len, a.fs = 1, 16000, 16000.0
        a.clean, a.est, a.stoi, a.workspace = x.data_ptr(), x.data_ptr(), d.data_ptr(), ws.data_ptr()
        a.clean_stride = a.est_stride = 16000
        a.workspace_bytes = ws.numel()
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.avz_stoi_batch(ct.byref(a), None)

    assert call(fs=8000.0) == _lib.AVZ_ERR_UNSUPPORTED
    assert lib.avz_stoi_batch(None, None) == _lib.AVZ_ERR_ARG
    assert call(clean=None) == _lib.AVZ_ERR_ARG
    assert call(workspace_bytes=ws.numel() - 1) == _lib.AVZ_ERR_SHAPE
    assert call() == _lib.AVZ_OK
    torch.cuda.synchronize()
    assert float(d[0]) == 0.0                         # zeros against zeros: all kept, no correlation
