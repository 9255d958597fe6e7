"""bench.py's plain run and --dump-outputs: a plain run prints the headline line without the
--full figures, and the dumped arrays are what a caller of the last timed step received
(the same scenes through MVDRPlan.run directly); an output over the size budget is cut to
a fixed, seeded sample of its rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, S = 8, 64000
WARMUP, STEPS = 1, 3  # settle restarts the counter: steps visit batches 0 1 0 1, the last is 1


def test_dump_outputs_samples_rows_over_budget(tmp_path, monkeypatch):
    import torch

    import bench
    x = torch.arange(40 * 16, dtype=torch.float32).reshape(40, 16)
    peak = torch.arange(40, dtype=torch.float32)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * 16 * 4)
    info = bench.dump_outputs({"out": x, "peak": peak}, str(tmp_path / "a"), 0)
    bench.dump_outputs({"out": x, "peak": peak}, str(tmp_path / "b"), 0)
    a, b = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    assert a.dtype == np.float32 and a.shape == (10, 16) and info["out"]["shape"] == [10, 16]
    np.testing.assert_array_equal(a, b)  # the same rows on every run
    rows = (a[:, 0] / 16).astype(int)
    assert len(set(rows)) == 10 and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(a, x.numpy()[rows])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "peak.npy"), peak.numpy())
    # under the budget: the whole array
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", x.numel() * 4)
    bench.dump_outputs({"out": x}, str(tmp_path / "c"), 1)
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "out_rank1.npy"), x.numpy())


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, gpu_device):
    import torch

    import avz
    from avz import synth
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", str(STEPS), "--warmup", str(WARMUP), "--batch", str(B),
                        "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env={k: v for k, v in os.environ.items()
                            if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["full"] is False
    assert line["unit"] == "TF-bins/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    bins = B * line["config"]["tf_bins_per_utt"]
    assert line["value"] == pytest.approx(bins / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("secondary", "sir", "pcie_inclusive"):  # --full only
        assert k not in line, k
    assert line["cpu_baseline"] is None and "kernels_ms" not in line["roofline"]

    got, peak = np.load(out / "out.npy"), np.load(out / "peak.npy")
    assert got.dtype == np.float32 and peak.dtype == np.float32
    assert got.shape == (B, S) and peak.shape == (B,)
    # the last timed step ran on batch 1 = utterances B .. 2B - 1
    mix, tgt, itf = synth.make_batch_device(B, start=B, n_samples=S, n_interferers=2,
                                            device=gpu_device, rng="philox")
    plan = avz.MVDRPlan(n_fft=1024, sigma=1.0, mic_d=0.01, mask="ibm", postfilter="ibm",
                        normalize="peak", max_batch=B, max_samples=S)
    ref, ref_peak = plan.run(mix, ref_tgt=tgt, ref_int=itf)
    torch.cuda.synchronize()
    # the same kernels on the same inputs (the chain is deterministic:
    # test_gpu_properties.test_deterministic_and_order_invariant)
    np.testing.assert_array_equal(got, ref[:, :plan.out_len(S)].cpu().numpy())
    np.testing.assert_array_equal(peak, ref_peak.cpu().numpy())
