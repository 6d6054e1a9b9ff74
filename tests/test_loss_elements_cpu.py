"""Calibration of the loss-epilogue and latent element references (gpu_helpers.recon_reference,
gpu_helpers.latent_reference), no GPU involved.

tests/test_gpu_loss_elements.py holds what the loss GEMM's epilogue (csrc/gemm_recon.hip) returns at probe
logits (gpu_helpers.RECON_PROBES) inside recon_reference's per-element bounds. Here those bounds are
  (a) tied to the reference's own output: every bce_elem_t{0,1} / bce_grad_t{0,1} of
      tests/golden/numerics.npz lies inside them, and equals them where `exact` is set;
  (b) wide enough: an honest fp32 evaluation -- torch CPU (sigmoid, binary_cross_entropy, autograd) and a
      numpy fp32 emulation of the FAST form as recon_tile writes it -- leaves the hull by at most HALF of
      the rounding allowance at every probe;
  (c) tight enough: each one-line mutant of the element math leaves the bounds at one probe or more.
The same for latent_reference: honest fp32 inside half of the bounds, three mutants outside.
"""
import numpy as np
import pytest
import torch

from golden_io import load
from gpu_helpers import BF16_RNE, RECON_PROBES, latent_reference, recon_reference

WGAMMAS = (0.0, 0.55)
REGIMES = list(RECON_PROBES)
F32 = np.float32


def _grid(regime):
    """Every probe logit of the regime with both targets: l, x of shape [2 n]."""
    pr = RECON_PROBES[regime]
    return np.concatenate([pr, pr]), np.concatenate([np.zeros(pr.size, bool), np.ones(pr.size, bool)])


def _torch_eval(l, x, wg):
    """The reference's own operations in fp32 on the CPU: Sigmoid -> BCE(sum) + wgamma * sum p, autograd."""
    lt = torch.tensor(l, dtype=torch.float32, requires_grad=True)
    xt = torch.tensor(x.astype(np.float32))
    p = torch.sigmoid(lt)
    bce = torch.nn.functional.binary_cross_entropy(p, xt, reduction="none")
    (bce.sum() + wg * p.sum()).backward()
    return {"bce": bce.detach().numpy(), "p": p.detach().numpy(), "dl": lt.grad.numpy()}


def _exact_eval(l, x, wg, mutant=None):
    """recon_exact (csrc/gemm_recon.hip) operation by operation in numpy fp32; `mutant` breaks one line."""
    l, wg = l.astype(F32), F32(wg)
    xf = x.astype(F32)
    if mutant == "x_from_neighbour_gene":
        xf = np.roll(xf, 1)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        e = np.exp(-l).astype(F32)
        p = (F32(1) / (F32(1) + e)).astype(F32)
        omp = (F32(1) - p).astype(F32)
        if mutant == "omp_from_exp":
            omp = (e / (F32(1) + e)).astype(F32)
        clamp = F32(-88) if mutant == "clamp_88" else F32(-100)
        lg = np.where(xf > 0, np.log(p), np.log1p(-p) if mutant != "omp_from_exp" else np.log(omp)).astype(F32)
        bce = -np.maximum(lg, clamp)
        if mutant == "softplus":  # the mathematically nicer form: log(1 + e^l) - x l
            bce = (np.maximum(l, 0) - l * xf + np.log1p(np.exp(-np.abs(l)))).astype(F32)
        q = (omp * p).astype(F32)
        den = {"guard_1e-6": np.maximum(q, F32(1e-6)), "no_guard": q}.get(mutant, np.maximum(q, F32(1e-12)))
        d = (p - xf) if mutant != "sign_flipped" else (xf - p)
        dp = (d / den).astype(F32)
        if mutant == "wgamma_on_p":
            dl = (dp * omp * p + wg * p).astype(F32)
        else:
            if mutant != "wgamma_dropped":
                dp = (dp + wg).astype(F32)
            dl = ((dp * omp).astype(F32) * p).astype(F32)
    return {"bce": bce.astype(F32), "p": p, "dl": dl}


MUTANTS = ["softplus", "clamp_88", "guard_1e-6", "no_guard", "omp_from_exp", "wgamma_dropped", "wgamma_on_p",
           "sign_flipped", "x_from_neighbour_gene"]


def _fast_eval(l, x, wg, acc_share=0.0):
    """The FAST element math of recon_tile in numpy fp32: the logit arrives as acc + bias with the bias
    pre-scaled (nb = fp32(b * -log2 e)), y = fma(acc, -log2 e, nb), p = rcp(1 + exp2(y)), the selects on
    p and p - 1, log2 clamped at -100 / ln 2 and scaled by -ln 2, the guard as med3(t * -1e12, 0, 1) and
    the gene-abundance term as an FMA on -(1 - p) p. exp2 / rcp / log2 are correctly rounded here (the
    hardware's are within 1 ulp)."""
    k = F32(-1.4426950408889634)
    acc = (l.astype(np.float64) * acc_share).astype(F32)
    b = (l - acc).astype(F32)
    nb = (b * k).astype(F32)
    y = (acc.astype(np.float64) * np.float64(k) + nb.astype(np.float64)).astype(F32)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        d = (np.exp2(y.astype(np.float64)).astype(F32) + F32(1)).astype(F32)
        p = (1.0 / d.astype(np.float64)).astype(F32)
        nomp = (p - F32(1)).astype(F32)
        sel = np.abs(np.where(x, p, nomp))
        l2 = np.maximum(np.log2(sel.astype(np.float64)).astype(F32), F32(-144.26950408889634))
        bce = (l2 * F32(-0.6931471805599453)).astype(F32)
        r = np.where(x, nomp, p)
        t = (nomp * p).astype(F32)
        s = np.clip((t * F32(-1e12)).astype(F32), F32(0), F32(1))
        dl = (r * s).astype(F32)
        dl = ((-F32(wg)).astype(np.float64) * t.astype(np.float64) + dl.astype(np.float64)).astype(F32)
    return {"bce": bce, "p": p, "dl": dl}


def _excess(ref, got, k):
    """How far `got` lies beyond the hull (the bounds without their allowance), in units of the allowance
    (inf where nothing is allowed and the value differs)."""
    lo, hi = ref[k]
    a = ref["allow"][k]
    v = got[k].astype(np.float64)
    out = np.maximum(np.maximum((lo + a) - v, v - (hi - a)), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(out > 0, out / np.where(a > 0, a, 0.0), 0.0)


def _outside(ref, got):
    """Elements of `got` outside the bounds of BCE, p or dl (a NaN is outside)."""
    bad = np.zeros(got["p"].shape, dtype=bool)
    for k in ("bce", "p", "dl"):
        lo, hi = ref[k]
        v = got[k].astype(np.float64)
        bad |= ~((v >= lo) & (v <= hi))
    return bad


def test_golden_elements_inside_the_bounds():
    """The reference's recorded element values and gradients (wgamma 0) at its own probe logits, which
    include -103, -90, -88.7, 16.5, 17, 30 and 89."""
    g = load("numerics")
    l = g["bce_logits"].astype(np.float32)
    assert {-103.0, -90.0, -88.7, 16.5, 17.0, 30.0, 89.0} <= {round(float(v), 1) for v in l}
    for t in (0, 1):
        ref = recon_reference(l, np.full(l.shape, t), 0.0, fast=False)
        for k, name in (("bce", f"bce_elem_t{t}"), ("dl", f"bce_grad_t{t}")):
            lo, hi = ref[k]
            v = g[name].astype(np.float64)
            bad = ~((v >= lo) & (v <= hi))
            assert not bad.any(), (name, l[bad], v[bad], lo[bad], hi[bad])
            ex = ref["exact"]
            assert ex.sum() >= 40 and np.array_equal(v[ex], lo[ex]) and np.array_equal(lo[ex], hi[ex]), name


@pytest.mark.parametrize("wg", WGAMMAS)
@pytest.mark.parametrize("regime", REGIMES)
def test_honest_fp32_stays_within_half_of_the_allowance(regime, wg):
    l, x = _grid(regime)
    evals = [("torch", False, _torch_eval(l, x, wg)), ("exact", False, _exact_eval(l, x, wg)),
             ("fast", True, _fast_eval(l, x, wg)), ("fast acc/2", True, _fast_eval(l, x, wg, 0.5)),
             ("fast acc", True, _fast_eval(l, x, wg, 1.0))]
    for name, fast, got in evals:
        ref = recon_reference(l, x, wg, fast=fast)
        for k in ("bce", "p", "dl"):
            assert np.isfinite(got[k]).all(), (name, k)
            ex = _excess(ref, got, k)
            w = int(np.argmax(ex))
            print(f"{regime} wgamma {wg} {name}: {k} worst excess / allowance {ex[w]:.3f} at l {l[w]} x {int(x[w])}")
            assert ex[w] <= 0.5, (name, k, l[w], x[w], got[k][w], ref[k][0][w], ref[k][1][w])
        e = ref["exact"]
        assert e.all() == (regime == "saturated") and e.any() == (regime == "saturated")
        for k in ("bce", "p", "dl"):  # one value, and the honest evaluations return it
            assert np.array_equal(got[k][e].astype(np.float64), ref[k][0][e]), (name, k)


def test_the_denormal_band_contains_both_answers():
    """x = 1 at -87.5 .. -88.7: the reference's |l| (a subnormal p kept) and 100 (p flushed to 0)."""
    l = RECON_PROBES["denormal"]
    for fast in (False, True):
        lo, hi = recon_reference(l, np.ones(l.shape), 0.0, fast)["bce"]
        assert (lo <= -l.astype(np.float64)).all() and (hi >= 100.0).all() and (hi < 100.01).all()


@pytest.mark.parametrize("mutant", MUTANTS)
def test_recon_mutants_leave_the_bounds(mutant):
    """Each mutant, evaluated in fp32 as a wrong kernel would, is outside the bounds of BCE, p or dl at
    one probe or more (the honest evaluation of the same code: at none)."""
    hits = {}
    for regime in REGIMES:
        for wg in WGAMMAS:
            l, x = _grid(regime)
            # (neighbouring probes alternate targets, so a target read from the next gene is a wrong one)
            if mutant == "x_from_neighbour_gene":
                l, x = np.repeat(RECON_PROBES[regime], 2), np.tile([False, True], RECON_PROBES[regime].size)
            ref = recon_reference(l, x, wg, fast=False)
            assert not _outside(ref, _exact_eval(l, x, wg)).any()
            hits[regime, wg] = int(_outside(ref, _exact_eval(l, x, wg, mutant)).sum())
    print(f"mutant {mutant}: probes outside the bounds by (regime, wgamma): {hits}")
    assert sum(hits.values()) >= 1, mutant


def test_bf16_rounding_of_dl_needs_two_to_the_minus_eight():
    """The bf16 paths sum the bf16-rounded dl. Honest FAST values rounded to bf16 (RNE) move by up to 2^-8 of
    themselves (gpu_helpers.BF16_RNE: 8 significant bits), and at some probes by more than 2^-9, so the
    bias-gradient check of tests/test_gpu_loss_elements.py widens by 2^-8 sum |terms|; the mutants that
    change dl move it by far more than that."""
    worst = 0.0
    for regime in ("ordinary", "approach"):
        for wg in WGAMMAS:
            l, x = _grid(regime)
            dl = _fast_eval(l, x, wg)["dl"]
            rn = torch.tensor(dl).bfloat16().float().numpy()
            nz = np.abs(dl) >= np.finfo(np.float32).tiny
            rel = np.abs(rn.astype(np.float64) - dl)[nz] / np.abs(dl.astype(np.float64))[nz]
            assert (rel <= BF16_RNE).all()
            worst = max(worst, float(rel.max()))
            lo, hi = recon_reference(l, x, wg, fast=True)["dl"]
            w = BF16_RNE * np.maximum(np.abs(lo), np.abs(hi))
            mutants = ["sign_flipped"] + (["wgamma_dropped", "wgamma_on_p"] if wg else []) + \
                (["guard_1e-6"] if regime == "approach" else [])
            for mutant in mutants:
                bad = _exact_eval(l, x, wg, mutant)["dl"].astype(np.float64)
                assert ((bad < lo - w) | (bad > hi + w)).any(), (regime, wg, mutant)
    print(f"bf16 RNE of dl: worst relative move {worst:.3g} = 2^{np.log2(worst):.2f}")
    assert 2.0 ** -9 < worst <= BF16_RNE


# ------------------------------------------------------------------------------------------ the latent
MUS = np.array([0, 1e-3, -1e-3, 0.5, -0.5, 3, -3, 30, -30, 1e3, -1e3], dtype=np.float32)
LVS = np.array([-100, -30, -10, -1, -1e-3, 0, 1e-3, 1, 5, 10, 20], dtype=np.float32)
BETA = 0.37


def _latent_eval(mu, lv, beta, mutant=None):
    """k_reparam's KL term and k_reparam_bwd's head gradients at dz = 0, in numpy fp32."""
    mu, lv, beta = mu.astype(F32), lv.astype(F32), F32(beta)
    ex = np.exp(lv if mutant != "exp_half_lv" else F32(0.5) * lv).astype(F32)
    sq = mu if mutant == "mu_for_mu2" else (mu * mu).astype(F32)
    kl = ((((F32(1) + lv).astype(F32) - sq).astype(F32)) - ex).astype(F32)
    hb = beta if mutant == "no_half" else (F32(0.5) * beta)
    dmu = ((F32(0.5) * beta) * (F32(2) * mu)).astype(F32)
    dlv = (-hb + (hb * ex).astype(F32)).astype(F32)
    return {"kl": kl, "dmu": dmu, "dlv": dlv}


def _latent_ratio(ref, got):
    out = {}
    for k in ("kl", "dmu", "dlv"):
        v, tol = ref[k]
        err = np.abs(got[k].astype(np.float64) - v)
        assert not ((tol == 0) & (err > 0)).any()
        out[k] = float(np.max(err / np.where(tol > 0, tol, 1.0)))
    return out


def test_latent_fp32_stays_within_half_of_the_bounds():
    mu, lv = (a.reshape(-1) for a in np.meshgrid(MUS, LVS))
    r = _latent_ratio(latent_reference(mu, lv, BETA), _latent_eval(mu, lv, BETA))
    print(f"latent fp32 worst error / bound: {r}")
    assert max(r.values()) <= 0.5, r


@pytest.mark.parametrize("mutant", ["exp_half_lv", "no_half", "mu_for_mu2"])
def test_latent_mutants_leave_the_bounds(mutant):
    mu, lv = (a.reshape(-1) for a in np.meshgrid(MUS, LVS))
    r = _latent_ratio(latent_reference(mu, lv, BETA), _latent_eval(mu, lv, BETA, mutant))
    print(f"latent mutant {mutant}: worst error / bound {r}")
    assert max(r.values()) > 1.0, (mutant, r)
