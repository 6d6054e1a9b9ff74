"""bench.py on the GPU, in-process at a small shape (the zero-copy bf16 step at G = 20,000 with a
ragged 1000-row batch, the shape tests/test_gpu_parity.py proves against the gathering path): a plain
run times exactly --steps steps and reports only the headline line; --dump-outputs writes the last
timed step's outputs as float32 / float64 .npy files, identical from run to run."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--genes", "20000", "--hidden", "1024", "--latent", "32",
        "--batch", "1000", "--strains", "2005"]
FULL_ONLY = ("c5", "presets", "c1_gpu", "precision_line", "sample", "cpu_baseline", "cpu_baseline_c1")


def _run(monkeypatch, capsys, extra):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + ARGS + extra)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(monkeypatch, capsys, tmp_path):
    from gm2 import native
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    r1 = _run(monkeypatch, capsys, ["--dump-outputs", d1])
    r2 = _run(monkeypatch, capsys, ["--dump-outputs", d2])
    for r in (r1, r2):
        assert r["steps"] == 3 and r["warmup"] == 1 and r["n_gpus"] == 1
        assert r["unit"] == "strain-vectors/s" and r["higher_is_better"] is True and r["dtype"] == "bf16"
        assert r["ms_per_step"] > 0
        # value = rows of the timed steps / their time (both rounded for the line: 1 in 1e3 at worst)
        assert r["value"] == pytest.approx(1000 / (r["ms_per_step"] * 1e-3), rel=2e-3)
        # the live-timed loss GEMM ran once per timed step: --steps is the number of timed steps
        assert r["roofline"]["launches"] == 3
        assert not [k for k in FULL_ONLY if k in r]
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2)) == ["bn.npy", "exp_avg.npy", "exp_avg_sq.npy", "grads.npy", "index.npy",
                                               "loss.npy", "params.npy"]
    assert sum(os.path.getsize(os.path.join(d1, n)) for n in names) <= 64 << 20
    a = {n[:-4]: np.load(os.path.join(d1, n)) for n in names}
    b = {n[:-4]: np.load(os.path.join(d2, n)) for n in names}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k   # seeded inputs, deterministic kernels
    n = len(a["index"])
    assert a["loss"].shape == (native.LOSS_SLOTS,) and a["loss"][0] > 0 and a["loss"][4] > 0
    for k in ("grads", "params", "exp_avg", "exp_avg_sq"):
        assert a[k].shape == (n,) and a[k].dtype == np.float32
    # the sample reaches every parameter tensor, the small ones whole, and the step really updated:
    # nonzero gradients and moments, second moments >= 0
    off = native.param_offsets(20000, 1024, 32)
    idx = a["index"].astype(np.int64)
    for lo, hi in zip(off[:-1], off[1:]):
        got = int(((idx >= lo) & (idx < hi)).sum())
        assert got == min(hi - lo, 1 << 16)
    assert np.count_nonzero(a["grads"]) > n // 2 and np.count_nonzero(a["exp_avg"]) > n // 2
    assert (a["exp_avg_sq"] >= 0).all()
