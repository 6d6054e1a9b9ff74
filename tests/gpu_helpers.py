"""Shared helpers for the @pytest.mark.gpu parity tests (HIP path vs the CPU oracle)."""
import numpy as np
import torch

from gm2 import native
from gm2.model import VAE
from oracle import vae_oracle as O


def oracle_state(G, H, L, seed):
    torch.manual_seed(seed)
    P = O.init_params(G, H, L)
    S = O.init_bn_state(H)
    return P, S


def perturb_bn(P, S, seed):
    """Non-trivial BN affine params / running stats (fresh init has gamma=1, beta=0, rm=0, rv=1)."""
    g = torch.Generator().manual_seed(seed)
    for bn in O.BNS:
        H = P[bn + ".weight"].shape[0]
        P[bn + ".weight"] = 0.8 + 0.4 * torch.rand(H, generator=g)
        P[bn + ".bias"] = 0.2 * torch.rand(H, generator=g) - 0.1
        S[bn + ".running_mean"] = 0.4 * torch.rand(H, generator=g) - 0.2
        S[bn + ".running_var"] = 0.5 + torch.rand(H, generator=g)
    return P, S


def to_model(P, S, G, H, L, prec):
    m = VAE(G, H, L, precision=prec, init=False)
    sd = {}
    for k, v in P.items():
        sd[k] = v
    for k, v in S.items():
        sd[k] = v
    m.load_state_dict(sd)
    return m


def synth_x(n, g, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    f = rng.beta(0.1, 1.0, size=g)
    f[rng.random(g) < 0.15] = 0.98
    return (rng.random((n, g)) < f[None, :]).astype(np.uint8)


def flat(d, names):
    return torch.cat([d[n].detach().reshape(-1).float().cpu() for n in names])


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def prebn_bias(name):
    """A Linear bias in front of a BatchNorm: its true gradient is exactly zero."""
    parts = name.split(".")
    return parts[0] in ("encoder", "decoder") and parts[1] in ("0", "3", "6") and parts[2] == "bias"


def grad_bar_failures(specs, offsets, grads, exact, ref, floor, bias_tol, label):
    """The per-tensor gradient bar of the training-step tests (the C2 method, tests/test_gpu_c2.py), on
    the flat gradient buffer `grads` of a model with `specs` / `offsets`: on the norm-wise relative
    error against `exact` (the oracle's gradients in fp64),
        fro(libgm2) <= 3 * fro(reference arithmetic) + floor,
    `ref` being the same math in the path's own arithmetic; the pre-BatchNorm biases (true gradient
    zero: rounding noise on both sides) absolutely, |g| <= bias_tol * the largest gradient of their
    weight. Prints every tensor's figures and returns the lines of those that miss."""
    fails = []
    for i, (name, _) in enumerate(specs):
        got = grads[offsets[i]:offsets[i + 1]].cpu().double().numpy()
        ex = exact[name].reshape(-1).cpu().double().numpy()
        if prebn_bias(name):
            scale = max(float(np.abs(exact[name.replace("bias", "weight")].cpu().numpy()).max()), 1e-12)
            if np.abs(got).max() > bias_tol * scale:
                fails.append(f"{name}: |g|max {np.abs(got).max():.3g} vs weight scale {scale:.3g}")
            continue
        r = ref[name].reshape(-1).cpu().double().numpy()
        nrm = max(float(np.linalg.norm(ex)), 1e-30)
        f_gpu = float(np.linalg.norm(got - ex)) / nrm
        f_ref = float(np.linalg.norm(r - ex)) / nrm
        msg = f"{name}: libgm2 {label} vs exact fro {f_gpu:.3g}; reference arithmetic fro {f_ref:.3g}"
        print(msg)
        if not f_gpu <= 3 * f_ref + floor:
            fails.append(msg)
    return fails


def scalars(beta=0.5, wgamma=0.0, lam=0.0, lr=1e-3, step=1, max_norm=1.0, b1=0.9, b2=0.999, eps=1e-8):
    v = np.zeros(native.NUM_SCALARS)
    v[native.S_BETA], v[native.S_WGAMMA], v[native.S_LAMBDA] = beta, wgamma, lam
    v[native.S_NEG_STEP] = -(lr / (1 - b1 ** step))
    v[native.S_BC2_SQRT] = np.sqrt(1 - b2 ** step)
    v[native.S_MAX_NORM] = max_norm
    v[native.S_ONE_MINUS_B1], v[native.S_BETA2], v[native.S_ONE_MINUS_B2], v[native.S_ADAM_EPS] = 1 - b1, b2, 1 - b2, eps
    return torch.tensor(v, dtype=torch.float32).cuda()


ADAM_U = 2.0 ** -24  # unit roundoff of fp32
ADAM_K = 8           # roundings the kernel may stack on one quantity (tests/test_optimizer_cpu.py calibrates it)


def adam_reference(p, g, m, v, scal, cc):
    """One fused L1 + clip + Adam update (k_adam_fused) in float64, from the fp32 inputs, the fp32 scalar
    block as the kernel reads it and the fp32 clip coefficient `cc`:
        gg = (g + lam * sign(p)) * cc;  m' = m + w1 (gg - m);  v' = v * b2 + w2 * gg^2
        den = sqrt(v') / bc2s + eps;    p' = p + negstep * m' / den
    with per-element bounds on what the kernel's fp32 evaluation may differ by (u = 2^-24, K = 8: at
    most eight roundings per quantity, sqrtf and the division correctly rounded, FMA contraction allowed):
        tm = K u (|m| + |gg|);  tv = K u (v + gg^2)
        tden = tv / (2 sqrt(v') bc2s) [0 where v' = 0] + K u den
        tstep = |negstep| tm / den + step tden / den + K u step,  step = |negstep| |m'| / den
        tp = 2 u |p'| + tstep
    Returns {"p": (p', tp), "m": (m', tm), "v": (v', tv)} as float64 numpy arrays."""
    p, g, m, v = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (p, g, m, v))
    s = np.asarray(scal, dtype=np.float32).astype(np.float64)
    lam, negstep, bc2s = s[native.S_LAMBDA], s[native.S_NEG_STEP], s[native.S_BC2_SQRT]
    w1, b2, w2, eps = s[native.S_ONE_MINUS_B1], s[native.S_BETA2], s[native.S_ONE_MINUS_B2], s[native.S_ADAM_EPS]
    cc = float(np.float32(cc))
    u, K = ADAM_U, ADAM_K
    gg = (g + lam * np.sign(p)) * cc
    m2 = m + w1 * (gg - m)
    v2 = v * b2 + w2 * gg * gg
    rt = np.sqrt(v2)
    den = rt / bc2s + eps
    p2 = p + negstep * m2 / den
    tm = K * u * (np.abs(m) + np.abs(gg))
    tv = K * u * (v + gg * gg)
    tden = np.where(v2 > 0, tv / np.where(v2 > 0, 2 * rt * bc2s, 1.0), 0.0) + K * u * den
    step = abs(negstep) * np.abs(m2) / den
    tstep = abs(negstep) * tm / den + step * tden / den + K * u * step
    tp = 2 * u * np.abs(p2) + tstep
    return {"p": (p2, tp), "m": (m2, tm), "v": (v2, tv)}


def adam_inputs(n, seed, zeros=0.01):
    """fp32 p, g, m, v of n elements for the optimizer tests: random signs, log-uniform magnitudes (|p| in
    1e-4..1; |g|, |m|, sqrt(v) in 1e-8..1), with a share `zeros` of exact zeros in each and as many -0.0 in p."""
    rng = np.random.Generator(np.random.PCG64(seed))

    def mag(lo):
        return 10.0 ** rng.uniform(np.log10(lo), 0.0, n)

    def sgn():
        return np.where(rng.random(n) < 0.5, -1.0, 1.0)
    p, g, m, v = mag(1e-4) * sgn(), mag(1e-8) * sgn(), mag(1e-8) * sgn(), mag(1e-8) ** 2
    for a in (p, g, m, v):
        a[rng.random(n) < zeros] = 0.0
    p[rng.random(n) < zeros] = -0.0
    return tuple(a.astype(np.float32) for a in (p, g, m, v))


def shadow_views(ws):
    """Typed 2-D views of the eight GEMM weight shadows in ws.buf, by name. This mirrors make_layout in
    csrc/api.hip, which takes them first, in this order, each region rounded up to 256 bytes:
    sE0 [H][Gp], sE1 / sE2 [H][H], sHD [L2r][H] (rows 0..L-1 mean_layer, L..2L-1 logvar_layer), sD0 [H][Lr],
    sD1 / sD2 [H][H], sD3 [Gp][H]; elements bf16 with Gp = roundup(G, 256) for GM2_BF16, fp32 with
    Gp = roundup(G, 128) for GM2_F32 and GM2_BF16X3; L2r = roundup(2L, 128), Lr = roundup(roundup(L, 64), 128)."""
    def up(x, k):
        return (x + k - 1) // k * k
    G, H, L = int(ws.d.G), int(ws.d.H), int(ws.d.L)
    bf = ws.prec == native.GM2_BF16
    dt, es = (torch.bfloat16, 2) if bf else (torch.float32, 4)
    Gp, L2r, Lr = up(G, 256 if bf else 128), up(2 * L, 128), up(up(L, 64), 128)
    shapes = [("sE0", H, Gp), ("sE1", H, H), ("sE2", H, H), ("sHD", L2r, H), ("sD0", H, Lr), ("sD1", H, H),
              ("sD2", H, H), ("sD3", Gp, H)]
    out, cur = {}, ws.off
    for name, r, c in shapes:
        out[name] = ws.buf[cur: cur + r * c * es].view(dt).view(r, c)
        cur += up(r * c * es, 256)
    return out


# (parameter name, shadow region, first row) of the nine Linear weights (make_table in csrc/api.hip)
SHADOW_OF = [("encoder.0.weight", "sE0", 0), ("encoder.3.weight", "sE1", 0), ("encoder.6.weight", "sE2", 0),
             ("mean_layer.weight", "sHD", 0), ("logvar_layer.weight", "sHD", None), ("decoder.0.weight", "sD0", 0),
             ("decoder.3.weight", "sD1", 0), ("decoder.6.weight", "sD2", 0), ("decoder.9.weight", "sD3", 0)]


def expected_shadows(ws, params, specs, offsets):
    """The image every shadow region must hold for the flat fp32 `params`: cvt(params) at [srow0 + r][c]
    (cvt: identity for fp32 shadows, .bfloat16() for bf16 ones), zero everywhere else. CPU tensors shaped
    and typed like shadow_views(ws)."""
    views = shadow_views(ws)
    pc = params.detach().cpu()
    img = {k: torch.zeros(v.shape, dtype=v.dtype) for k, v in views.items()}
    index = {n: i for i, (n, _) in enumerate(specs)}
    for name, region, row0 in SHADOW_OF:
        i = index[name]
        r, c = specs[i][1]
        row0 = int(ws.d.L) if row0 is None else row0
        img[region][row0:row0 + r, :c] = pc[offsets[i]:offsets[i + 1]].view(r, c).to(img[region].dtype)
    return img


# ----------------------------------------------------------------------------------------------------
# The loss epilogue (csrc/gemm_recon.hip) and the latent kernels (k_reparam, k_reparam_bwd), element by
# element (tests/test_loss_elements_cpu.py calibrates both; tests/test_gpu_loss_elements.py uses them)
# ----------------------------------------------------------------------------------------------------
RECON_U = 2.0 ** -24                                  # unit roundoff of fp32
RECON_FLT_MIN = float(np.finfo(np.float32).tiny)      # smallest normal fp32
RECON_GUARD = float(np.float32(1e-12))                # the guard of BCE's backward, as fp32 holds it
RECON_SAT_HI, RECON_SAT_LO = 17.5, -89.0              # l >= / <= these: every honest evaluation gives p == 1 / p == 0

# the probe logits of the element tests, by regime. Left out on purpose: (15.5, 17.5), where 1 - p is one
# to three ulps of p, so a 2-ulp hull contains p = 1 and with it both the -100 clamp and its absence; and
# (-88.72, -89), the overflow edge of exp.
RECON_PROBES = {
    "ordinary": np.linspace(-12.0, 12.0, 97).astype(np.float32),
    "approach": np.concatenate([np.linspace(12.25, 15.5, 14), np.linspace(-13.0, -27.0, 15),
                                [-27.5, -27.63, -27.75, -28.0, -30.0, -40.0, -60.0, -80.0, -87.0]]).astype(np.float32),
    "saturated": np.array([17.5, 18, 20, 30, 60, 88, 89, 100, 200, -89, -90, -103, -104, -200], dtype=np.float32),
    "denormal": np.array([-87.5, -88.0, -88.5, -88.7], dtype=np.float32),
}


def _sigmoid64(l):
    l = np.asarray(l, dtype=np.float64)
    e = np.exp(-np.abs(l))
    return np.where(l >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _recon_formula64(p, x, wgamma):
    """The reference's element formula in float64 from an fp32 p (exact in float64): BCE and dl."""
    omp = 1.0 - p
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.where(x, np.log(p), np.log1p(-p))
    bce = -np.maximum(lg, -100.0)
    dl = ((p - x) / np.maximum(omp * p, RECON_GUARD) + wgamma) * omp * p
    return bce, dl


def recon_reference(l, x, wgamma, fast):
    """Per-element float64 bounds of what the loss epilogue may return for fp32 logits `l` and 0/1 targets
    `x` (numpy arrays of one shape): {"bce": (lo, hi), "p": (lo, hi), "dl": (lo, hi), "exact": mask,
    "allow": {"bce": a, "p": 0, "dl": a}}.

    The formula is the reference's (loss_components.py:49-50 through Sigmoid, autograd's BCE backward, the
    gene-abundance term w*gamma per p): p = fp32 sigmoid, 1 - p formed from that fp32 p,
        BCE = -max(log(x ? p : 1 - p), -100);  dl = ((p - x) / max((1 - p) p, 1e-12) + wgamma) (1 - p) p.
    [lo, hi] is the hull of that formula, in float64, over the values of p an honest fp32 evaluation can
    reach: p' = round32(sigmoid64(l')) and its neighbours within +-2 ulp (exact path: expf <= 1 ulp, the add
    0.5 ulp, the division correctly rounded; FAST path: exp2, the add and rcp <= 1 ulp each), with l' = l
    and, when `fast`, also l (1 +- 2 * 2^-23) (the FAST path forms acc * (-log2 e) + fp32(-b log2 e): two
    roundings of a number of size |l| log2 e); and p' = 0 wherever round32(sigmoid64(l)) is subnormal
    (hardware transcendentals flush, and expf itself overflows to p = 0 below -88.72). The hull is widened
    by `allow`: 4 u |BCE| + 2^-22 (log(1 - p) for log1p(-p), a hardware log's absolute error near 1) and
    8 u (|dl| + wgamma / 4) + FLT_MIN, u = 2^-24.

    `exact`: l >= 17.5 (1 + e^-l rounds to 1: p == 1, BCE 0 for x = 1 and exactly 100 for x = 0, dl == 0 for
    any wgamma) or l <= -89 (exp overflows: p == 0, BCE exactly 100 for x = 1 and 0 for x = 0, dl == +-0):
    every honest evaluation gives that one value, lo == hi and nothing is allowed on top."""
    l = np.asarray(l, dtype=np.float32)
    xb = np.asarray(x) != 0
    assert l.shape == xb.shape
    l64 = l.astype(np.float64)
    lps = [l64] + ([l64 * (1 + 2 * 2.0 ** -23), l64 * (1 - 2 * 2.0 ** -23)] if fast else [])
    one, zero = np.float32(1), np.float32(0)
    cands = []
    for lp in lps:
        p0 = _sigmoid64(lp).astype(np.float32)
        up = dn = p0
        cands.append(p0)
        for _ in range(2):
            up = np.minimum(np.nextafter(up, np.float32(2)), one)
            dn = np.maximum(np.nextafter(dn, np.float32(-1)), zero)
            cands += [up, dn]
    flush = _sigmoid64(l64).astype(np.float32) < np.float32(RECON_FLT_MIN)
    cands.append(np.where(flush, zero, cands[0]))
    lo = {k: np.full(l.shape, np.inf) for k in ("bce", "p", "dl")}
    hi = {k: np.full(l.shape, -np.inf) for k in ("bce", "p", "dl")}
    for pc in cands:
        p = pc.astype(np.float64)
        bce, dl = _recon_formula64(p, xb, float(wgamma))
        for k, v in (("bce", bce), ("p", p), ("dl", dl)):
            lo[k] = np.minimum(lo[k], v)
            hi[k] = np.maximum(hi[k], v)
    sat1, sat0 = l >= np.float32(RECON_SAT_HI), l <= np.float32(RECON_SAT_LO)
    exact = sat1 | sat0
    val = {"bce": np.where(sat1 != xb, 100.0, 0.0), "p": np.where(sat1, 1.0, 0.0), "dl": np.zeros(l.shape)}
    u = RECON_U
    allow = {"bce": 4 * u * np.maximum(np.abs(lo["bce"]), np.abs(hi["bce"])) + 2.0 ** -22,
             "p": np.zeros(l.shape),
             "dl": 8 * u * (np.maximum(np.abs(lo["dl"]), np.abs(hi["dl"])) + abs(float(wgamma)) / 4) + RECON_FLT_MIN}
    out = {"exact": exact, "allow": {}}
    for k in ("bce", "p", "dl"):
        a = np.where(exact, 0.0, allow[k])
        out["allow"][k] = a
        out[k] = (np.where(exact, val[k], lo[k] - a), np.where(exact, val[k], hi[k] + a))
    return out


# Rounding dl to bf16 (the bf16 paths store dL as bf16 and sum the stored values for the bias gradient): bf16
# keeps 8 significant bits, so round-to-nearest-even moves a value by at most half an ulp = 2^-8 of it, reached
# just above a power of two (1 + 2^-8 rounds to 1 or 1 + 2^-7), and by 2^-9 only just below one. (2^-9 is not a
# bound: tests/test_loss_elements_cpu.py shows honest values beyond it.)
BF16_RNE = 2.0 ** -8

LATENT_K = 8  # roundings the latent kernels may stack on one quantity, as ADAM_K


def latent_reference(mu, lv, beta):
    """Per latent element, in float64 from the fp32 mu, logvar and beta, what k_reparam adds to loss slot 2
    and what k_reparam_bwd returns for a zero upstream dz, each as (value, bound):
        "kl":  1 + lv - mu^2 - exp(lv),     bound K u (1 + |lv| + mu^2 + exp(lv))
        "dmu": beta mu,                     bound K u |beta mu|
        "dlv": 0.5 beta (exp(lv) - 1),      bound K u 0.5 beta (1 + exp(lv))
    u = 2^-24, K = 8. The bounds are absolute in the terms' sizes, so they cover the cancellation of
    1 + lv - exp(lv) and of exp(lv) - 1 at lv near 0."""
    mu = np.asarray(mu, dtype=np.float32).astype(np.float64)
    lv = np.asarray(lv, dtype=np.float32).astype(np.float64)
    beta = float(np.float32(beta))
    ku = LATENT_K * RECON_U
    ex = np.exp(lv)
    return {"kl": (1 + lv - mu * mu - ex, ku * (1 + np.abs(lv) + mu * mu + ex)),
            "dmu": (beta * mu, ku * np.abs(beta * mu)),
            "dlv": (0.5 * beta * (ex - 1), ku * 0.5 * abs(beta) * (1 + ex))}
