"""bench.py host logic (no GPU): the per-step scalar tables of the preset lines (round 6) follow the
reference's schedules -- v0/v1 linear KL beta at epoch 0 of a 10000-epoch run, v2/v3 cosine beta
advancing its counter once per batch (loss_components.py:76-91, 187-202), gene abundance w*gamma
(loss_components.py:111-115: v1/v2 gamma 1.0, v3 gamma 2.0 with weight 1), L1 lambda 0.01 for
v1-v3 (experiments.py:42-114, trainer.py:193-257) -- and the Adam constants of torch.optim.Adam
at lr 1e-3 (bias corrections per step)."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_and_full_options(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d", "--no-sample"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d" and a.no_sample and not a.no_c5


def test_dump_outputs_index_set(tmp_path):
    """--dump-outputs: small parameter tensors whole, a fixed DUMP_SAMPLE-element sample of each larger
    one (sorted, no repeats, the same on every call), float32 / float64 files only."""
    import types

    import torch

    import bench
    big = bench.DUMP_SAMPLE + 1000
    off = [0, 5, 5 + big, 5 + big + 70]
    n = off[-1]
    flat = lambda s: torch.arange(n, dtype=torch.float32) + s  # noqa: E731
    model = types.SimpleNamespace(offsets=off, params=flat(0.0), bn=torch.ones(2, 2, 3))
    opt = types.SimpleNamespace(exp_avg=flat(0.25), exp_avg_sq=flat(0.5))
    losses = np.arange(12, dtype=np.float64).reshape(2, 6)
    outs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), model, opt, flat(0.75), losses)
        outs.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = outs
    assert sorted(a) == ["bn", "exp_avg", "exp_avg_sq", "grads", "index", "loss", "params"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k])
    idx = a["index"].astype(np.int64)
    assert len(idx) == 5 + bench.DUMP_SAMPLE + 70 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx[:5], np.arange(5)) and np.array_equal(idx[-70:], np.arange(n - 70, n))
    assert idx[5] >= 5 and idx[-71] < 5 + big
    assert np.array_equal(a["loss"], losses[-1]) and a["bn"].shape == (2, 2, 3)
    for k, s in (("params", 0.0), ("exp_avg", 0.25), ("exp_avg_sq", 0.5), ("grads", 0.75)):
        assert np.array_equal(a[k], (idx + s).astype(np.float32))


def test_preset_scalar_tables():
    import bench
    from gm2 import native
    n = 25
    t0, t1, t2, t3 = (bench.scalar_table(n, p) for p in ("v0", "v1", "v2", "v3"))
    for t in (t0, t1):
        assert np.allclose(t[:, native.S_BETA], 0.1)
    cos = lambda k, T, lo, hi: lo + (hi - lo) / 2 * (1 + math.cos(math.pi * (k % T) / T))  # noqa: E731
    assert np.allclose(t2[:, native.S_BETA], [cos(k, 10, 0.0, 1.0) for k in range(n)])
    assert np.allclose(t3[:, native.S_BETA], [cos(k, 50, 0.1, 1.0) for k in range(n)])
    assert t2[10, native.S_BETA] == t2[0, native.S_BETA] == 1.0 and t2[5, native.S_BETA] < 0.51
    assert np.all(t0[:, native.S_WGAMMA] == 0) and np.all(t0[:, native.S_LAMBDA] == 0)
    assert np.allclose(t1[:, native.S_WGAMMA], 1.0) and np.allclose(t2[:, native.S_WGAMMA], 1.0)
    assert np.allclose(t3[:, native.S_WGAMMA], 2.0)
    for t in (t1, t2, t3):
        assert np.allclose(t[:, native.S_LAMBDA], 0.01)
    for t in (t0, t1, t2, t3):
        k = np.arange(1, n + 1)
        assert np.allclose(t[:, native.S_NEG_STEP], -(1e-3 / (1 - 0.9 ** k)))
        assert np.allclose(t[:, native.S_BC2_SQRT], np.sqrt(1 - 0.999 ** k))
        assert np.all(t[:, native.S_MAX_NORM] == 1.0)
    # the train FLOP count of SURVEY.md 8(d) at the bench's dims
    assert bench.train_flops_per_vector(55039, 1024, 64) == 2 * (3 * (2 * 55039 * 1024 + 4 * 1024 ** 2 + 3 * 1024 * 64)
                                                                  - 55039 * 1024)
    assert abs(bench.train_flops_per_vector(55039, 1024, 64) / 1e6 - 589.9) < 0.1
    assert abs(bench.train_flops_per_vector(55039, 512, 32) / 1e6 - 288.4) < 0.1
