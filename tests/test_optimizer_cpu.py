"""Calibration of the optimizer tests' reference and tolerance (gpu_helpers.adam_reference), no GPU involved.

tests/test_gpu_optimizer.py holds every element the fused L1 + clip + Adam kernel writes inside the
per-element bounds adam_reference returns. Those bounds must be (a) wide enough for an honest fp32
evaluation of the same formulas -- numpy fp32 here stays within HALF of each bound -- and (b) tight enough
that a subtly wrong update leaves them: each of six one-line mutants of the update puts more than 70 % of
the elements outside the bound of at least one of p', m', v'. If a GPU run ever needs a wider K
(gpu_helpers.ADAM_K), it is changed there and (b) must still hold here.

Measured (2e5 elements, lam 0.01, steps 1 / 7 / 1000, cc 1 / 0.0371): fp32 error / bound at most 0.13 for
m', 0.24 for v' and 0.50 for p' (the final add's own rounding against the 2 u |p'| term). Mutant shares
over the configurations: no clip 1.00, no L1 0.98, b2 / w2 swapped 1.00, v's bias correction 1.00, the
step from the old m 1.00, eps inside the square root 0.72 -- per configuration 0.68 - 0.70 at cc 1 and
0.74 - 0.76 at cc 0.0371: that mutant moves den by eps / (2 v') relatively, below den's own rounding once
sqrt(v') > ~0.01, which with sqrt(v) log-uniform over 1e-8..1 is about three elements in ten.
"""
import numpy as np
import pytest

from gpu_helpers import adam_inputs, adam_reference

N = 200_000
LAM = 0.01  # the trainer's L1 weight in the GPU tests: every mutant below changes the update with it
MUTANTS = ["no_clip", "no_l1", "b2_w2_swapped", "no_v_bias_correction", "eps_in_sqrt", "step_from_old_m"]


def _scal(step, lam=LAM, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """The fp32 scalar block, laid out as gpu_helpers.scalars does (no device)."""
    from gm2 import native
    s = np.zeros(native.NUM_SCALARS)
    s[native.S_LAMBDA] = lam
    s[native.S_NEG_STEP] = -(lr / (1 - b1 ** step))
    s[native.S_BC2_SQRT] = np.sqrt(1 - b2 ** step)
    s[native.S_ONE_MINUS_B1], s[native.S_BETA2], s[native.S_ONE_MINUS_B2], s[native.S_ADAM_EPS] = 1 - b1, b2, 1 - b2, eps
    return s.astype(np.float32)


def _update(p, g, m, v, scal, cc, dt, mutant=None):
    """The kernel's formulas, operation by operation, in dtype `dt`; `mutant` breaks one of them."""
    from gm2 import native
    p, g, m, v = (a.astype(dt) for a in (p, g, m, v))
    s = scal.astype(dt)
    lam, negstep, bc2s = s[native.S_LAMBDA], s[native.S_NEG_STEP], s[native.S_BC2_SQRT]
    w1, b2, w2, eps = s[native.S_ONE_MINUS_B1], s[native.S_BETA2], s[native.S_ONE_MINUS_B2], s[native.S_ADAM_EPS]
    cc = dt(cc)
    if mutant == "no_clip":
        cc = dt(1)
    if mutant == "no_l1":
        lam = dt(0)
    if mutant == "b2_w2_swapped":
        b2, w2 = w2, b2
    gg = (g + lam * np.sign(p)) * cc
    m2 = m + w1 * (gg - m)
    v2 = v * b2
    v2 = v2 + w2 * gg * gg
    if mutant == "no_v_bias_correction":
        den = np.sqrt(v2) + eps
    elif mutant == "eps_in_sqrt":
        den = np.sqrt(v2 + eps) / bc2s
    else:
        den = np.sqrt(v2) / bc2s + eps
    p2 = p + negstep * ((m if mutant == "step_from_old_m" else m2) / den)
    assert p2.dtype == dt and m2.dtype == dt and v2.dtype == dt
    return {"p": p2, "m": m2, "v": v2}


@pytest.fixture(scope="module")
def inputs():
    return adam_inputs(N, seed=2024)


def test_inputs_cover_the_edges(inputs):
    p, g, m, v = inputs
    assert all(a.dtype == np.float32 and a.shape == (N,) for a in inputs)
    assert np.signbit(p[p == 0]).any() and (~np.signbit(p[p == 0])).any()  # both zeros
    assert all((a == 0).sum() > N // 500 for a in inputs) and (v >= 0).all()
    nz = lambda a: np.abs(a[a != 0])  # noqa: E731
    assert 1e-4 <= nz(p).min() < 2e-4 and 0.5 < nz(p).max() <= 1
    for a in (g, m, np.sqrt(v)):
        assert 1e-8 <= nz(a).min() < 2e-8 and 0.5 < nz(a).max() <= 1


CONFIGS = [(step, cc) for step in (1, 7, 1000) for cc in (1.0, 0.0371)]


@pytest.fixture(scope="module")
def references(inputs):
    """(scalar block, cc, adam_reference result) per (step, cc), computed once for both tests below."""
    out = {}
    for step, cc in CONFIGS:
        scal, c = _scal(step), np.float32(cc)
        out[step, cc] = (scal, c, adam_reference(*inputs, scal, c))
    return out


@pytest.mark.parametrize("step,cc", CONFIGS)
def test_fp32_stays_within_half_of_the_bounds(inputs, references, step, cc):
    scal, c, ref = references[step, cc]
    got = _update(*inputs, scal, c, np.float32)
    for k in "pmv":
        r, tol = ref[k]
        assert np.isfinite(r).all() and np.isfinite(tol).all() and (tol >= 0).all()
        err = np.abs(got[k].astype(np.float64) - r)
        assert not ((tol == 0) & (err > 0)).any()
        ratio = float(np.max(err / np.where(tol > 0, tol, 1.0)))
        print(f"step {step} cc {cc}: fp32 {k}' worst error / bound {ratio:.3f}")
        assert ratio <= 0.5, (k, ratio)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_leave_the_bounds(inputs, references, mutant):
    """The share of elements a mutant puts outside the bound of at least one of p', m', v', over every
    covered (step, cc) it applies to (no_clip: cc < 1 only), must exceed 70 %. The mutant runs in fp32,
    as a wrong kernel would."""
    outside = []
    for (step, cc), (scal, c, ref) in references.items():
        if mutant == "no_clip" and cc == 1:
            continue  # (no clip to leave out)
        bad = _update(*inputs, scal, c, np.float32, mutant)
        out = np.zeros(N, dtype=bool)
        for k in "pmv":
            r, tol = ref[k]
            out |= np.abs(bad[k].astype(np.float64) - r) > tol
        print(f"step {step} cc {cc}: mutant {mutant} outside the bounds at {out.mean():.3f} of the elements")
        outside.append(out)
    share = float(np.concatenate(outside).mean())
    print(f"mutant {mutant}: {share:.3f} of the elements over {len(outside)} configurations")
    assert share > 0.7, (mutant, share)
