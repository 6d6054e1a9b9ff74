"""The loss GEMM's epilogue (csrc/gemm_recon.hip) and the latent kernels (k_reparam, k_reparam_bwd), element
by element at extreme logits, on every kernel path.

decoder.9.weight = 0 makes the accumulator exactly 0, so logit[b][g] = decoder.9.bias[g] for every strain
and dA5 = dL . W9 = 0: nothing behind the output layer sees the extreme values, grad(decoder.9.bias)[g] =
sum_b dl(l_g, x_bg) is a per-gene observable (the bf16 paths sum the bf16-rounded dl), loss slot 0 is sum
BCE and slot 1 sum p. mean_layer.weight = logvar_layer.weight = 0 makes mu and logvar their biases for every
row, and with the upstream dz exactly 0: grad(mean_layer.bias)[j] = B beta mu_j, grad(logvar_layer.bias)[j] =
B 0.5 beta (exp(lv_j) - 1), slot 2 = B sum_j (1 + lv_j - mu_j^2 - exp(lv_j)).

The references are gpu_helpers.recon_reference / latent_reference: the reference's formulas in float64 with
per-element bounds, calibrated without a GPU in tests/test_loss_elements_cpu.py (the reference's golden
element values lie inside, honest fp32 evaluations stay within half of the allowance, one-line mutants
leave). Sums of elements are widened for their fp32 summation: the bias gradient by B u sum |terms| (B
terms, any order), plus 2^-8 sum |terms| on the bf16 paths (RNE of dl to bf16's 8 significant bits: half an
ulp is 2^-8 of a value just above a power of two, gpu_helpers.BF16_RNE; equal strains round the same way, so
the sum can keep all of it); the loss slots by 8 u sum |terms|, the terms including the pad-gene constants an
edge tile adds and subtracts (pad_g * val_s * ln 2, resp. / 2).

Observed on an MI355X (release and GM2_DEBUG builds alike), worst error / bound over wgamma, training and
evaluation: slots 0 / 1 at most 0.14 / 0.09 (ordinary), 0.30 / 0.04 (approach), 0.21 / 0 (saturated; 0 / 0 on
bf16x3) on every path, slot 2 0.004; grad(decoder.9.bias) 0.50 on f32 and bf16x3 (the width is the hull's),
0.89 (ordinary) and 0.81 (approach) on the three bf16 paths, exactly 0 when saturated. In the denormal band
every path sits on an end of its hull (1.00): the exact paths return the reference's |l| from a subnormal p,
the FAST paths p = 0 and so 100 (recorded in the header of csrc/gemm_recon.hip).

Model: G = 880, H = 256, L = 16, B = batch_max = 130. fp32 layouts: Gp = 896, a last 128-tile of 112 valid
genes; bf16 layout: Gp = 1024, one 128-tile with pad genes and one wholly in the padding, a 256-tile of 112
valid columns; a second 128-strain tile of 2 valid rows, a 256-strain tile of 126 padded rows; H % 256 == 0
lets the bf16x3 workspace take k_gemm_recon_loss_x3 once GM2_OPT_RECON_TILE = 256 is forced. The capped
grid (GM2_OPT_GRID_CAP bit 4) only loops where the tiles outnumber the CUs, which no shape this small
reaches: those cases run at the smallest G with one tile more than CUs (128-tiles: 2 strain tiles; 256-tiles:
one) and compare bit for bit with the uncapped run.

Probe logits by regime (gpu_helpers.RECON_PROBES): each call takes all G biases from one regime, the probe
table x the four target pairs (even strains pattern A, odd strains pattern B) repeated over the genes in
seeded shuffles; the last 64 genes have random targets per strain.
"""
import numpy as np
import pytest
import torch

from gm2 import native
from gm2.data import ResidentMatrix

from gpu_helpers import (BF16_RNE, RECON_PROBES, RECON_SAT_HI, RECON_U, latent_reference, oracle_state, perturb_bn,
                         recon_reference, scalars, to_model)

pytestmark = pytest.mark.gpu

G, H, L, B = 880, 256, 16, 130
BETA = 0.37
WGAMMAS = (0.0, 0.55)
RANDOM_TAIL = 64
LN2 = 0.6931471805599453
U = RECON_U

# path -> (precision, workspace options, gene padding the loss kernel's tiles see, FAST element math)
PATHS = {
    "f32": (native.GM2_F32, {}, 128, False),
    "bf16-128": (native.GM2_BF16, {native.OPT_RECON_TILE: 128}, 256, True),
    "bf16-256-pp": (native.GM2_BF16, {native.OPT_RECON_TILE: 256, native.OPT_GEMM_PP: 1}, 256, True),
    "bf16-256": (native.GM2_BF16, {native.OPT_RECON_TILE: 256, native.OPT_GEMM_PP: 0}, 256, True),
    # (the x3 kernel skips padded genes: no pad constants)
    "bf16x3": (native.GM2_BF16X3, {native.OPT_RECON_TILE: 256, native.OPT_GEMM_PP: 1}, 1, False),
}
REGIMES = list(RECON_PROBES)
HEAD_MU = np.linspace(-1.0, 1.0, L).astype(np.float32)
HEAD_LV = np.linspace(-2.0, 1.0, L).astype(np.float32)

_SETUPS = {}
_X3_SPLIT = {}


class Setup:
    """One model of G genes with the zeroed weights, on one kernel path, with its workspace."""

    def __init__(self, path, genes):
        prec, opts, _, _ = PATHS[path]
        P, S = perturb_bn(*oracle_state(genes, H, L, 41), seed=42)
        P["decoder.9.weight"] = torch.zeros_like(P["decoder.9.weight"])
        P["mean_layer.weight"] = torch.zeros_like(P["mean_layer.weight"])
        P["logvar_layer.weight"] = torch.zeros_like(P["logvar_layer.weight"])
        P["mean_layer.bias"] = torch.from_numpy(HEAD_MU.copy())
        P["logvar_layer.bias"] = torch.from_numpy(HEAD_LV.copy())
        self.path, self.G, self.prec = path, genes, prec
        self.m = to_model(P, S, genes, H, L, prec)
        self.bn0 = self.m.bn.clone()
        self.ws = self.m.workspace(prec, B)
        for k, v in opts.items():
            self.ws.set_option(k, v)
        self.index = {n: i for i, (n, _) in enumerate(self.m.specs)}
        self.eps = torch.randn(B, L, generator=torch.Generator().manual_seed(43)).cuda()

    def set_param(self, name, values):
        with torch.no_grad():
            self.m.param_views()[name].copy_(torch.from_numpy(np.asarray(values, dtype=np.float32)).cuda())

    def grad_of(self, grads, name):
        i = self.index[name]
        return grads[self.m.offsets[i]:self.m.offsets[i + 1]].cpu().numpy()

    def call(self, X, wgamma, train, grid_cap=None):
        """One gm2_train_fwd_bwd (or gm2_eval_forward) on the 0/1 rows X; (loss slots, flat gradients)."""
        ws, m = self.ws, self.m
        if grid_cap is not None:
            ws.set_option(native.OPT_GRID_CAP, grid_cap)
        mat = ResidentMatrix(X)
        batch = native.make_batch(mat.data, mat.ld, None, B, self.eps)
        loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
        sc = scalars(beta=BETA, wgamma=wgamma)
        bn = self.bn0.clone()
        before = ws.stat(native.TSTAT_SPLIT_GEMMS) if self.path == "bf16x3" else 0
        grads = None
        if train:
            grads = torch.zeros_like(m.params)
            native.train_fwd_bwd(ws, batch, m.params, grads, bn, sc, loss)
        else:
            native.eval_forward(ws, batch, m.params, bn, sc, loss)
        ws.join()
        torch.cuda.synchronize()
        if self.path == "bf16x3":  # else the case would test the fp32 kernel a second time
            split = ws.stat(native.TSTAT_SPLIT_GEMMS) - before
            assert split == x3_split_with_loss(self, train), (split, train)
        return loss.cpu().numpy(), grads


@pytest.fixture(scope="module", autouse=True)
def _release_setups():
    """The cached models and workspaces (the capped-grid shapes hold some 100 MB each) go with the module."""
    yield
    _SETUPS.clear()


def model_setup(path, genes=G):
    if (path, genes) not in _SETUPS:
        _SETUPS[path, genes] = Setup(path, genes)
    return _SETUPS[path, genes]


def x3_split_with_loss(st, train):
    """GM2_TSTAT_SPLIT_GEMMS per call of a bf16x3 workspace of this shape whose loss GEMM is one of the
    split ones: one more than with GM2_OPT_RECON_TILE = 128, which keeps the loss GEMM (and nothing else:
    x3_plan in csrc/api.hip) on the fp32 kernel."""
    key = (st.G, train)
    if key not in _X3_SPLIT:
        ws = native.Workspace(native.dims(st.G, H, L, B), native.GM2_BF16X3, torch.device("cuda"))
        ws.set_option(native.OPT_RECON_TILE, 128)
        native.sync_shadows(ws, st.m.params)
        X = np.zeros((B, st.G), dtype=np.uint8)
        X[::2, ::3] = 1
        mat = ResidentMatrix(X)
        batch = native.make_batch(mat.data, mat.ld, None, B, st.eps)
        loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
        if train:
            native.train_fwd_bwd(ws, batch, st.m.params, torch.zeros_like(st.m.params), st.bn0.clone(),
                                 scalars(beta=BETA), loss)
        else:
            native.eval_forward(ws, batch, st.m.params, st.bn0.clone(), scalars(beta=BETA), loss)
        ws.join()
        torch.cuda.synchronize()
        total = 5 if train else 2
        assert ws.stat(native.TSTAT_SPLIT_GEMMS) + ws.stat(native.TSTAT_EXACT_GEMMS) == total
        _X3_SPLIT[key] = ws.stat(native.TSTAT_SPLIT_GEMMS) + 1
        assert _X3_SPLIT[key] <= total
    return _X3_SPLIT[key]


def probe_inputs(regime, genes, seed):
    """(decoder.9.bias [genes] fp32, X [B][genes] u8): every probe logit of the regime with (xA, xB) in 00,
    01, 10, 11 -- even strains take pattern A, odd strains pattern B -- the classes repeated over the genes
    in seeded shuffles; the last RANDOM_TAIL genes take random probes and random targets per strain."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pr = RECON_PROBES[regime]
    ncls = 4 * pr.size
    n = genes - RANDOM_TAIL
    cls = np.concatenate([rng.permutation(ncls) for _ in range(-(-n // ncls))])[:n]
    bias = np.concatenate([pr[cls >> 2], rng.choice(pr, RANDOM_TAIL)]).astype(np.float32)
    X = np.zeros((B, genes), dtype=np.uint8)
    X[0::2, :n] = (cls >> 1) & 1
    X[1::2, :n] = cls & 1
    X[:, n:] = rng.random((B, RANDOM_TAIL)) < 0.5
    return bias, X


def element_bounds(bias, X, wgamma, fast):
    """recon_reference at (bias[g], X[b][g]) for every strain: {"bce" / "p" / "dl": (lo, hi) [B][G]}, the
    reference evaluated once per (gene, target) and gathered."""
    r = [recon_reference(bias, np.full(bias.shape, t), wgamma, fast) for t in (0, 1)]
    xb = X != 0
    return {k: tuple(np.where(xb, r[1][k][i][None, :], r[0][k][i][None, :]) for i in (0, 1)) for k in ("bce", "p", "dl")}


def ratio_in(got, lo, hi):
    """|got - centre| / half-width of [lo, hi], elementwise (0 where got is the centre; inf where the
    interval is a point and got is not it)."""
    got, lo, hi = (np.asarray(a, dtype=np.float64) for a in (got, lo, hi))
    c, h = (lo + hi) / 2, (hi - lo) / 2
    d = np.abs(got - c)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d > 0, d / np.where(h > 0, h, 0.0), 0.0)
    return np.where(np.isfinite(got), r, np.inf)


def slot_failures(st, label, regime, bias, X, eb, lt):
    """Loss slots 0, 1 (sums of the element bounds, widened by 8 u sum |terms|, the pad-gene constants
    among the terms) and 2 (latent_reference at the head biases); prints each error / bound."""
    _, _, pad_to, _ = PATHS[st.path]
    pad = (-(-st.G // pad_to) * pad_to - st.G) * B  # padded (gene, valid strain) elements the tiles sum
    fails = []
    for slot, k, padc in ((0, "bce", LN2), (1, "p", 0.5)):
        lo, hi = eb[k]
        slack = 8 * U * (np.maximum(np.abs(lo), np.abs(hi)).sum() + 2 * pad * padc)
        r = float(ratio_in(lt[slot], lo.sum() - slack, hi.sum() + slack))
        print(f"{label}: slot {slot} {lt[slot]!r} in [{lo.sum() - slack!r}, {hi.sum() + slack!r}]: error / bound {r:.3f}")
        if not r <= 1:
            fails.append(f"{label}: slot {slot} {lt[slot]!r} outside [{lo.sum() - slack!r}, {hi.sum() + slack!r}]")
    if regime == "saturated":  # one value per element: sum p = B #(l >= 17.5), sum BCE = 100 mismatches
        ones = bias >= np.float32(RECON_SAT_HI)
        want = (100.0 * float((ones[None, :] != (X != 0)).sum()), float(B * ones.sum()))
        for slot, padc in ((0, LN2), (1, 0.5)):
            slack = 8 * U * (want[slot] + 2 * pad * padc)
            print(f"{label}: slot {slot} {lt[slot]!r} vs exactly {want[slot]!r} (slack {slack:.3g})")
            if not abs(lt[slot] - want[slot]) <= slack:
                fails.append(f"{label}: slot {slot} {lt[slot]!r} is not {want[slot]!r} within {slack:.3g}")
    kl, tol = latent_reference(HEAD_MU, HEAD_LV, BETA)["kl"]
    slack = B * tol.sum() + 8 * U * B * (1 + np.abs(HEAD_LV) + HEAD_MU.astype(np.float64) ** 2 + np.exp(HEAD_LV)).sum()
    r = abs(lt[2] - B * kl.sum()) / slack
    print(f"{label}: slot 2 {lt[2]!r} vs {B * kl.sum()!r}: error / bound {r:.3f}")
    if not r <= 1:
        fails.append(f"{label}: slot 2 {lt[2]!r} vs {B * kl.sum()!r}, bound {slack:.3g}")
    return fails


def gradient_failures(st, label, regime, eb, grads):
    """grad(decoder.9.bias) per gene inside the summed dl bounds (exactly 0 in the saturated regime),
    grad(decoder.9.weight) finite (all zero in the saturated regime), every other gradient finite."""
    fails = []
    lo, hi = eb["dl"]
    terms = np.maximum(np.abs(lo), np.abs(hi)).sum(axis=0)
    widen = B * U * terms + (BF16_RNE * terms if st.prec == native.GM2_BF16 else 0.0)
    gb = st.grad_of(grads, "decoder.9.bias")
    r = ratio_in(gb, lo.sum(axis=0) - widen, hi.sum(axis=0) + widen)
    w = int(np.argmax(r))
    print(f"{label}: grad(decoder.9.bias) worst error / bound {r[w]:.3f} at gene {w}")
    if not (r <= 1).all():
        fails.append(f"{label}: grad(decoder.9.bias) outside the bounds at {int((~(r <= 1)).sum())} of {r.size} genes; "
                     f"worst gene {w}: {gb[w]!r} vs [{(lo.sum(axis=0) - widen)[w]!r}, {(hi.sum(axis=0) + widen)[w]!r}]")
    gw = st.grad_of(grads, "decoder.9.weight")
    if not np.isfinite(gw).all():
        fails.append(f"{label}: grad(decoder.9.weight) has {int((~np.isfinite(gw)).sum())} non-finite elements")
    if regime == "saturated":
        if (gb != 0).any():
            fails.append(f"{label}: grad(decoder.9.bias) nonzero at {int((gb != 0).sum())} genes, e.g. {gb[gb != 0][:4]}")
        if (gw != 0).any():
            fails.append(f"{label}: grad(decoder.9.weight) nonzero at {int((gw != 0).sum())} elements")
    if not torch.isfinite(grads).all().item():
        bad = [n for n, _ in st.m.specs if not np.isfinite(st.grad_of(grads, n)).all()]
        fails.append(f"{label}: non-finite gradients in {bad}")
    return fails


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("path", list(PATHS))
def test_training_call_elementwise(path, regime):
    """gm2_train_fwd_bwd at wgamma 0 and 0.55: slots 0, 1, 2 and grad(decoder.9.bias) inside the bounds,
    the exact values in the saturated regime, every gradient finite."""
    st = model_setup(path)
    fast = PATHS[path][3]
    fails = []
    for i, wg in enumerate(WGAMMAS):
        bias, X = probe_inputs(regime, G, 100 + 10 * REGIMES.index(regime) + i)
        st.set_param("decoder.9.bias", bias)
        lt, grads = st.call(X, wg, train=True)
        eb = element_bounds(bias, X, wg, fast)
        label = f"{path} {regime} wgamma {wg} train"
        fails += slot_failures(st, label, regime, bias, X, eb, lt)
        fails += gradient_failures(st, label, regime, eb, grads)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("path", list(PATHS))
def test_eval_forward_elementwise(path, regime):
    """gm2_eval_forward (the GRAD = false kernels, the model's running statistics): slots 0, 1 and 2."""
    st = model_setup(path)
    bias, X = probe_inputs(regime, G, 200 + REGIMES.index(regime))
    st.set_param("decoder.9.bias", bias)
    lt, _ = st.call(X, 0.55, train=False)
    eb = element_bounds(bias, X, 0.55, PATHS[path][3])
    fails = slot_failures(st, f"{path} {regime} eval", regime, bias, X, eb, lt)
    assert not fails, "\n".join(fails)


def capped_genes(path):
    """The smallest gene count of this path's layout at which the loss tiles (B = 130: two 128-strain
    tiles, one 256-strain tile) outnumber the CUs by one or two, so the capped grid's workgroups loop; the
    last gene tile keeps 112 valid genes."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if PATHS[path][1].get(native.OPT_RECON_TILE) == 256:
        genes, tiles = 256 * (cus + 1) - 144, cus + 1
    else:
        gt = cus // 2 + 1
        gt += gt % 2 if PATHS[path][2] == 256 else 0  # (the bf16 layout pads the genes to 256)
        genes, tiles = 128 * gt - 16, 2 * gt
    assert cus < tiles <= cus + 4, (cus, tiles)
    return genes


@pytest.mark.parametrize("regime", ["saturated", "ordinary"])
@pytest.mark.parametrize("path", list(PATHS))
def test_capped_grid_is_the_uncapped_run(path, regime):
    """GM2_OPT_GRID_CAP bit 4: workgroups loop over tiles, reusing the LDS bias slice and image; loss slots
    and every gradient (dL through the bias gradient, dW9) are the uncapped run's bit for bit."""
    genes = capped_genes(path)
    st = model_setup(path, genes)
    base = st.ws.get_option(native.OPT_GRID_CAP) & ~4
    bias, X = probe_inputs(regime, genes, 300 + REGIMES.index(regime))
    st.set_param("decoder.9.bias", bias)
    try:
        la, ga = st.call(X, 0.55, train=True, grid_cap=base)
        lb, gb = st.call(X, 0.55, train=True, grid_cap=base | 4)
    finally:
        st.ws.set_option(native.OPT_GRID_CAP, base)
    assert np.isfinite(la[:3]).all() and la[0] > 0
    if regime == "saturated":
        assert not st.grad_of(ga, "decoder.9.bias").any()
    assert np.array_equal(la, lb), (la, lb)
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32))


def test_bf16x3_loss_gemm_is_split():
    """With GM2_OPT_RECON_TILE = 256 the bf16x3 workspace of this shape runs the loss GEMM as a split
    product (k_gemm_recon_loss_x3): every bf16x3 call above asserts the count this returns."""
    st = model_setup("bf16x3")
    for train in (True, False):
        n = x3_split_with_loss(st, train)
        print(f"bf16x3 G {G} train {train}: {n} split G-wide GEMMs with the loss GEMM among them")
        bias, X = probe_inputs("ordinary", G, 400)
        st.set_param("decoder.9.bias", bias)
        st.call(X, 0.0, train=train)  # (asserts the count)


LAT_MU = np.array([0, 1e-3, -1e-3, 0.5, -0.5, 3, -3, 30, -30, 1e3, -1e3], dtype=np.float32)
LAT_LV = np.array([-100, -30, -10, -1, -1e-3, 0, 1e-3, 1, 5, 10, 20], dtype=np.float32)


@pytest.mark.parametrize("path", ["f32", "bf16-128"])
def test_latent_elementwise(path):
    """k_reparam / k_reparam_bwd at head biases up to |mu| = 1e3 and logvar in [-100, 20], every value of
    both tables in each of two calls with different pairings: slot 2 and the two head-bias gradients
    against latent_reference, the B-term sums widened by B u sum |terms| (slot 2: 8 u, as the other slots).
    (Larger z overflows the decoder's BatchNorm variance in fp32, in the reference as well.)"""
    st = model_setup(path)
    bias, X = probe_inputs("ordinary", G, 500)
    st.set_param("decoder.9.bias", bias)
    j = np.arange(L)
    fails = []
    try:
        for call, (mi, li) in enumerate([(j % 11, j % 11), ((j + 5) % 11, (3 * j + 7) % 11)]):
            mu, lv = LAT_MU[mi], LAT_LV[li]
            assert set(mi) == set(range(11)) and set(li) == set(range(11))
            st.set_param("mean_layer.bias", mu)
            st.set_param("logvar_layer.bias", lv)
            lt, grads = st.call(X, 0.0, train=True)
            assert np.isfinite(lt[:3]).all(), lt
            ref = latent_reference(mu, lv, BETA)
            kl, tol = ref["kl"]
            terms = 1 + np.abs(lv.astype(np.float64)) + mu.astype(np.float64) ** 2 + np.exp(lv.astype(np.float64))
            slack = B * tol.sum() + 8 * U * B * terms.sum()
            r = abs(lt[2] - B * kl.sum()) / slack
            print(f"{path} latent call {call}: slot 2 {lt[2]!r} vs {B * kl.sum()!r}: error / bound {r:.3f}")
            if not r <= 1:
                fails.append(f"call {call}: slot 2 {lt[2]!r} vs {B * kl.sum()!r}, bound {slack:.3g}")
            for name, k in (("mean_layer.bias", "dmu"), ("logvar_layer.bias", "dlv")):
                v, t = ref[k]
                got = st.grad_of(grads, name).astype(np.float64)
                bound = B * t + B * U * B * np.abs(v)
                err = np.abs(got - B * v)
                rr = np.where(err > 0, err / np.where(bound > 0, bound, 1e-300), 0.0)
                w = int(np.argmax(rr))
                print(f"{path} latent call {call}: grad({name}) worst error / bound {rr[w]:.3f} at mu {mu[w]} lv {lv[w]}")
                if not (np.isfinite(got).all() and (err <= bound).all()):
                    fails.append(f"call {call}: grad({name})[{w}] {got[w]!r} vs {B * v[w]!r}, bound {bound[w]:.3g}")
    finally:
        st.set_param("mean_layer.bias", HEAD_MU)
        st.set_param("logvar_layer.bias", HEAD_LV)
    assert not fails, "\n".join(fails)
