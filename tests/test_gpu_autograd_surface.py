"""The autograd surface of libgm2 (gm2_forward / gm2_backward_outputs and the calls that share their
kernels: gm2_recon_counts, gm2_eval_forward, gm2_encode, gm2_reparameterize) in both precisions, in
train and eval BatchNorm, at ragged multi-tile shapes, with NULL heads, a padded probs pitch, a
reused workspace with stale pad rows, row index lists, and on a GM2_BF16X3 workspace.

Shapes (G, H, L, batch_max, n):
  A  517, 128, 16, 200, 130    Gp = 640 with a ragged odd G (probs rows not 16-B aligned at ld = G), two row
                               tiles, the second partial
  B  1000, 256, 32, 300, 77    n < batch_max; the 77 rows are an index list (with repeats) into 700 rows
  C  8192, 256, 32, 1024, 1024 the 256x256 tiles and the split-K input layer
  D  2500, 1024, 64, 200, 200  the presets' hidden width, L = 64

Bar (the C2 method of tests/test_gpu_c2.py, tests/test_gpu_parity.py): per output and per gradient
tensor, on the norm-wise relative error against EXACT (oracle.manual_forward_backward_emulated in
fp64 on the device, no rounding),
    fro(libgm2) <= 3 * fro(reference arithmetic) + floor,
the reference arithmetic being the same oracle in fp32 (with bf16 operand rounding for the bf16
path), floor 2e-4 (f32) / 1e-3 (bf16). Under train-mode BatchNorm the pre-BatchNorm Linear biases
have an exactly-zero gradient and are bounded absolutely (1e-3 / 2e-2 of the weight gradient's max).
"""
import math

import numpy as np
import pytest
import torch

from gpu_helpers import oracle_state, perturb_bn, rel_err, scalars, synth_x, to_model
from oracle import vae_oracle as O

pytestmark = pytest.mark.gpu

from gm2.loss_components import LossComponent

if torch.cuda.is_available():
    from gm2 import native
    from gm2.data import ResidentMatrix, StrainLoader
    from gm2.model import VAE
    from gm2.trainer import Adam, StepLR, VAETrainerBuilder

SHAPES = {"A": (517, 128, 16, 200, 130), "B": (1000, 256, 32, 300, 77), "C": (8192, 256, 32, 1024, 1024),
          "D": (2500, 1024, 64, 200, 200)}
B_ROWS = 700     # shape B's resident matrix
SENT = -777.25   # sentinel of guard rows / columns / floats
FLOOR = {"f32": 2e-4, "bf16": 1e-3}
BIAS_LIM = {"f32": 1e-3, "bf16": 2e-2}


def _prec(prec):
    return native.GM2_F32 if prec == "f32" else native.GM2_BF16


def _prebn_bias(name):
    p = name.split(".")
    return p[0] in ("encoder", "decoder") and p[1] in ("0", "3", "6") and p[2] == "bias"


_STATE, _REFS, _BN_REF = {}, {}, {}


def _state(tag):
    """Host inputs of a shape, generated once from seeds: parameters + perturbed BatchNorm, the 0/1
    matrix (shape B: 700 rows and a 77-long index list with two repeated indices), eps and the
    dense upstream gradients."""
    if tag not in _STATE:
        G, H, L, bm, n = SHAPES[tag]
        k = ord(tag)
        P, S = perturb_bn(*oracle_state(G, H, L, 100 + k), seed=k)
        X = synth_x(B_ROWS if tag == "B" else n, G, 7 * k)
        g = torch.Generator().manual_seed(k)
        rows = None
        if tag == "B":
            rows = torch.randint(0, B_ROWS, (n,), generator=g)
            rows[5], rows[41] = rows[0], rows[40]
            rows = rows.to(torch.int32)
        st = dict(P=P, S=S, X=X, rows=rows, eps=torch.randn(n, L, generator=g), dp=torch.randn(n, G, generator=g),
                  dmu=torch.randn(n, L, generator=g), dlv=torch.randn(n, L, generator=g))
        st["xb"] = X if rows is None else X[rows.numpy()]
        _STATE[tag] = st
    return _STATE[tag]


LOSS_BETA, LOSS_WG = 0.37, 0.55


def _upstream(tag, train, up="rand"):
    """Host fp32 (dprobs, dmu, dlv). 'rand': the seeded dense randn set. 'loss': the fused loss's own
    upstream gradients (BCE + beta KL + w gamma sum p) at the exact oracle's outputs, rounded to fp32
    once: dprobs = (p - x) / clamp((1 - p) p, 1e-12) + wgamma, dmu = beta mu, dlv = -0.5 beta (1 - exp(lv));
    every consumer (libgm2, the exact oracle, the reference arithmetic) is given the same tensors."""
    st = _state(tag)
    if up == "rand":
        return st["dp"], st["dmu"], st["dlv"]
    key = ("loss", bool(train))
    if key not in st:
        out = _oracle(tag, train, "exact")[0]
        p, mu, lv = out["probs"], out["mu"], out["logvar"]
        x = torch.tensor(st["xb"], dtype=torch.float64)
        st[key] = (((p - x) / torch.clamp((1 - p) * p, min=1e-12) + LOSS_WG).float(), (LOSS_BETA * mu).float(),
                   (-0.5 * LOSS_BETA * (1 - torch.exp(lv))).float())
    return st[key]


def _oracle(tag, train, kind, up="rand"):
    """(outputs, grads) of the oracle on the device, as fp64 host tensors; kind: 'exact' (fp64),
    'f32' (fp32), 'bf16' (fp32 with bf16 operand rounding); up: the upstream gradient set
    (_upstream). Computed once per (shape, mode, kind, set)."""
    key = (tag, bool(train), kind, up)
    if key not in _REFS:
        st = _state(tag)
        dev = torch.device("cuda")
        torch.backends.cuda.matmul.allow_tf32 = False
        Pd = {k: v.to(dev) for k, v in st["P"].items()}
        Sd = {k: v.to(dev) for k, v in st["S"].items()}
        kw = {} if kind == "exact" else dict(dtype=torch.float32, operand_round=O.bf16_round if kind == "bf16" else None)
        dp, dmu, dlv = _upstream(tag, train, up)
        out, gr = O.manual_forward_backward_emulated(Pd, Sd, torch.tensor(st["xb"], dtype=torch.float32, device=dev),
                                                     st["eps"].to(dev), dp.to(dev), dmu.to(dev), dlv.to(dev),
                                                     bool(train), **kw)
        _REFS[key] = ({k: out[k].double().cpu() for k in ("probs", "mu", "logvar")},
                      {k: v.double().cpu() for k, v in gr.items()})
    return _REFS[key]


def _bn_ref(tag):
    """BatchNorm running statistics after one train-mode forward (fp64 oracle forward)."""
    if tag not in _BN_REF:
        st = _state(tag)
        S2 = {k: v.double().clone() for k, v in st["S"].items()}
        with torch.no_grad():
            O.forward({k: v.double() for k, v in st["P"].items()}, S2, torch.tensor(st["xb"], dtype=torch.float64),
                      st["eps"].double(), train=True)
        _BN_REF[tag] = S2
    return _BN_REF[tag]


def _model(tag, prec, bm=None):
    G, H, L, bmax, n = SHAPES[tag]
    st = _state(tag)
    m = to_model(st["P"], st["S"], G, H, L, prec)
    ws = m.workspace(prec, bm or bmax)
    mat = ResidentMatrix(st["X"])
    rows = None if st["rows"] is None else st["rows"].cuda()
    return m, ws, mat, rows


def _dev_inputs(tag, train=1, up="rand"):
    return (_state(tag)["eps"].cuda(),) + tuple(t.cuda() for t in _upstream(tag, train, up))


def _run(m, ws, mat, rows, n, eps, dp, dmu, dlv, train, pad=False, want_mu=True, want_lv=True, bwd=True):
    """One gm2_forward (+ one gm2_backward_outputs). pad: probs / dprobs [n + 1, G + 3] filled with the
    sentinel (ld_probs = G + 3) and 8 sentinel floats on each side of the gradient window. Every
    output buffer starts as the sentinel, so an element a call leaves unwritten fails the bars."""
    G, L, dev = m.input_dim, m.latent_dim, m.device
    if pad:
        probs = torch.full((n + 1, G + 3), SENT, device=dev)
        dpb = torch.full((n + 1, G + 3), SENT, device=dev)
        dpb[:n, :G] = dp
    else:
        probs = torch.full((n, G), SENT, device=dev)
        dpb = dp.contiguous()
    gbuf = torch.full((m.n_params + 16,), SENT, device=dev)
    grads = gbuf[8:8 + m.n_params] if pad else torch.full((m.n_params,), SENT, device=dev)
    mu = torch.full((n, L), SENT, device=dev) if want_mu else None
    lv = torch.full((n, L), SENT, device=dev) if want_lv else None
    ld = probs.stride(0)
    batch = native.make_batch(mat.data, mat.ld, rows, n, eps)
    native.forward(ws, batch, m.params, m.bn, int(train), probs, ld, mu, lv)
    if bwd:
        native.backward_outputs(ws, batch, m.params, int(train), probs, ld, dpb, dmu, dlv, grads)
    torch.cuda.synchronize()
    return dict(probs=probs, mu=mu, logvar=lv, grads=grads, gbuf=gbuf, dpb=dpb, bn=m.bn.clone())


def _fro_pair(got, ex, ref):
    nrm = max(float(torch.linalg.norm(ex)), 1e-30)
    return float(torch.linalg.norm(got - ex)) / nrm, float(torch.linalg.norm(ref - ex)) / nrm


def _check_bar(tag, prec, train, m, res, outputs=("probs", "mu", "logvar"), grads=True, up="rand"):
    """The bar of the module docstring on every output and gradient tensor of `res`; prints the two
    fro numbers per tensor."""
    G, n = SHAPES[tag][0], SHAPES[tag][4]
    ex_o, ex_g = _oracle(tag, train, "exact", up)
    rf_o, rf_g = _oracle(tag, train, prec, up)
    floor = FLOOR[prec]
    fails = []

    def bar(name, got, ex, ref):
        f_gpu, f_ref = _fro_pair(got.double().cpu().reshape(-1), ex.reshape(-1), ref.reshape(-1))
        msg = (f"{tag} {prec} train={int(train)} {name}: libgm2 vs exact fro {f_gpu:.3g}; reference arithmetic "
               f"fro {f_ref:.3g}")
        print(msg)
        if not f_gpu <= 3 * f_ref + floor:
            fails.append(msg)
    for name in outputs:
        got = res[name][:n, :G] if name == "probs" else res[name]
        bar(name, got, ex_o[name], rf_o[name])
    if grads:
        off = m.offsets
        for i, (name, _) in enumerate(m.specs):
            got = res["grads"][off[i]:off[i + 1]]
            if train and _prebn_bias(name):
                scale = max(float(ex_g[name.replace("bias", "weight")].abs().max()), 1e-12)
                gmax = float(got.abs().max())
                print(f"{tag} {prec} train=1 {name}: |g|max {gmax:.3g} vs weight gradient max {scale:.3g}")
                if not gmax <= BIAS_LIM[prec] * scale:
                    fails.append(f"{name}: |g|max {gmax:.3g} vs weight gradient max {scale:.3g}")
                continue
            bar(name, got, ex_g[name], rf_g[name])
    assert not fails, "\n".join(fails)


def _check_bn(tag, prec, train, res):
    """train: the running statistics are updated (bars of test_train_step_vs_oracle); eval: untouched."""
    st = _state(tag)
    bn = res["bn"].cpu()
    if not train:
        for i, b in enumerate(O.BNS):
            assert torch.equal(bn[i, 0], st["S"][b + ".running_mean"]) and torch.equal(bn[i, 1], st["S"][b + ".running_var"])
        return
    S2 = _bn_ref(tag)
    bf = prec == "bf16"
    for i, b in enumerate(O.BNS):
        np.testing.assert_allclose(bn[i, 0].numpy(), S2[b + ".running_mean"].numpy(), rtol=1e-3 if bf else 2e-5,
                                   atol=2e-3 if bf else 2e-6)
        np.testing.assert_allclose(bn[i, 1].numpy(), S2[b + ".running_var"].numpy(), rtol=1e-2 if bf else 2e-5,
                                   atol=1e-3 if bf else 2e-6)


def _same(a, b, keys=("probs", "mu", "logvar", "grads")):
    for k in keys:
        assert torch.equal(a[k], b[k]), f"{k} differs: max |d| {float((a[k] - b[k]).abs().max()):.3g}"


# ------------------------------------------------------------------------------------------------
# a. outputs and gradients against the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["A", "B", "C", "D"])
@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_forward_backward_vs_oracle(prec, train, tag):
    """One gm2_forward then one gm2_backward_outputs with dense random upstream gradients.

    First measurement of this path in bf16 (MI355X; fro(libgm2) / fro(reference arithmetic); "worst": the
    gradient tensor with the largest fro(libgm2); the largest fro(libgm2) / fro(reference) ratio
    of any gradient tensor was 1.12):
      shape  train  probs              mu               logvar           worst gradient tensor
      A      1      1.81e-3 / 1.79e-3  5.06e-3 / 5.05e-3  5.41e-3 / 5.44e-3  decoder.1.bias   0.146 / 0.141
      A      0      3.13e-4 / 3.13e-4  5.36e-3 / 5.36e-3  3.84e-3 / 3.84e-3  decoder.0.weight 0.0999 / 0.0999
      B      1      1.72e-3 / 1.72e-3  5.52e-3 / 5.52e-3  4.85e-3 / 4.85e-3  decoder.1.bias   0.133 / 0.130
      B      0      3.53e-4 / 3.53e-4  2.92e-3 / 2.92e-3  4.56e-3 / 4.56e-3  decoder.1.bias   0.0751 / 0.0751
      C      1      7.17e-4 / 7.18e-4  5.45e-3 / 5.45e-3  5.10e-3 / 5.10e-3  decoder.4.bias   0.121 / 0.120
      C      0      1.46e-4 / 1.46e-4  4.07e-3 / 4.07e-3  3.46e-3 / 3.46e-3  decoder.1.bias   0.0843 / 0.0844
      D      1      2.06e-3 / 2.06e-3  5.39e-3 / 5.38e-3  5.19e-3 / 5.19e-3  decoder.1.bias   0.119 / 0.119
      D      0      3.29e-4 / 3.29e-4  3.87e-3 / 3.87e-3  3.87e-3 / 3.87e-3  decoder.0.weight 0.0770 / 0.0774
    (the hidden layers' gradients are ill-conditioned, as tests/test_gpu_c2.py notes for the fused
    path: bf16 operand rounding costs ~10 % norm-wise there in any evaluation, the oracle's included;
    decoder.9.weight sits at 8e-3 and the f32 path at 1e-7 .. 8e-7 on every tensor.)"""
    n = SHAPES[tag][4]
    m, ws, mat, rows = _model(tag, _prec(prec))
    res = _run(m, ws, mat, rows, n, *_dev_inputs(tag), train)
    _check_bar(tag, prec, train, m, res)
    _check_bn(tag, prec, train, res)


@pytest.mark.parametrize("tag", ["A", "C"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_forward_backward_loss_shaped_upstream(prec, tag):
    """The same call pair and bar with the upstream gradients a user's loss really sends: those of
    BCE + beta KL + w gamma sum p (_upstream 'loss'). With them the exact oracle equals
    manual_grads_emulated (tests/test_oracle_outputs_cpu.py), so the autograd path must reproduce
    the fused loss's gradient; the output layer's bf16 reference arithmetic is 10 to 30 times closer to
    exact than under random-sign gradients (decoder.9.weight: 3e-4 .. 9e-4 measured, libgm2 the
    same), which tightens the bar on k_sigmoid_bwd<bf16>'s dL; the hidden layers stay at ~0.15."""
    n = SHAPES[tag][4]
    m, ws, mat, rows = _model(tag, _prec(prec))
    res = _run(m, ws, mat, rows, n, *_dev_inputs(tag, 1, "loss"), 1)
    _check_bar(tag, prec, 1, m, res, up="loss")


def test_argument_checks():
    """Calls the library must refuse before it launches anything: each raises, and a valid call on the
    same workspace afterwards still passes the bar. (The workspace's row capacity is batch_max
    rounded up to a whole 128-row tile, api.hip make_dims: `x.Bm = round_up(d->batch_max, kTile)`.)"""
    tag = "A"
    G, H, L, bm, n = SHAPES[tag]
    m, ws, mat, rows = _model(tag, native.GM2_BF16)
    eps, dp, dmu, dlv = _dev_inputs(tag)
    over = (bm + 127) // 128 * 128 + 1
    probs, grads = torch.empty(over, G, device="cuda"), torch.empty_like(m.params)
    big = ResidentMatrix(synth_x(over, G, 1))
    e1 = torch.zeros(over, L, device="cuda")
    with pytest.raises(RuntimeError, match="ld_probs"):
        native.forward(ws, native.make_batch(mat.data, mat.ld, None, n, eps), m.params, m.bn, 1, probs, G - 1)
    with pytest.raises(RuntimeError, match="eps required"):
        native.forward(ws, native.make_batch(mat.data, mat.ld, None, n, None), m.params, m.bn, 1, probs, G)
    with pytest.raises(RuntimeError, match="batch_max"):
        native.forward(ws, native.make_batch(big.data, big.ld, None, over, e1), m.params, m.bn, 1, probs, G)
    with pytest.raises(RuntimeError, match="more than 1 value"):
        native.forward(ws, native.make_batch(mat.data, mat.ld, None, 1, eps), m.params, m.bn, 1, probs, G)
    with pytest.raises(RuntimeError, match="batch_max"):
        native.backward_outputs(ws, native.make_batch(big.data, big.ld, None, over, e1), m.params, 1, probs, G,
                                probs, None, None, grads)
    with pytest.raises(RuntimeError, match="negative n"):
        native.reparameterize(-1, e1, e1, e1, e1)
    res = _run(m, ws, mat, rows, n, eps, dp, dmu, dlv, 1)
    _check_bar(tag, "bf16", 1, m, res)


# ------------------------------------------------------------------------------------------------
# b. NULL heads
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_null_heads(prec):
    """dmu / dlogvar NULL == explicit zero tensors, bit for bit: k_reparam_bwd adds the external term
    to a finished value (gmu += dmu_ext[..]), and x + 0.0f is x. mu / logvar NULL in gm2_forward
    leave the other outputs unchanged."""
    tag = "A"
    n, L = SHAPES[tag][4], SHAPES[tag][2]
    m, ws, mat, rows = _model(tag, _prec(prec))
    eps, dp, dmu, dlv = _dev_inputs(tag)
    zero = torch.zeros(n, L, device="cuda")
    full = _run(m, ws, mat, rows, n, eps, dp, dmu, dlv, 1)
    for a, b in ((dmu, None), (None, dlv), (None, None)):
        r_null = _run(m, ws, mat, rows, n, eps, dp, a, b, 1)
        r_zero = _run(m, ws, mat, rows, n, eps, dp, zero if a is None else a, zero if b is None else b, 1)
        _same(r_null, r_zero)
        assert not torch.equal(r_null["grads"], full["grads"])  # (the head gradient is really read)
    for want_mu, want_lv in ((False, True), (True, False), (False, False)):
        r = _run(m, ws, mat, rows, n, eps, dp, dmu, dlv, 1, want_mu=want_mu, want_lv=want_lv, bwd=False)
        assert torch.equal(r["probs"], full["probs"])
        if want_mu:
            assert torch.equal(r["mu"], full["mu"])
        if want_lv:
            assert torch.equal(r["logvar"], full["logvar"])


# ------------------------------------------------------------------------------------------------
# c. pitch and guards
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_probs_pitch_and_guards(prec, train):
    tag = "A"
    G, n = SHAPES[tag][0], SHAPES[tag][4]
    m, ws, mat, rows = _model(tag, _prec(prec))
    inp = _dev_inputs(tag)
    plain = _run(m, ws, mat, rows, n, *inp, train)
    pad = _run(m, ws, mat, rows, n, *inp, train, pad=True)
    assert bool((pad["probs"][:, G:] == SENT).all()), "probs columns >= G written"
    assert bool((pad["probs"][n] == SENT).all()), "probs row n written"
    assert bool((pad["dpb"][:, G:] == SENT).all()) and bool((pad["dpb"][n] == SENT).all())
    assert bool((pad["gbuf"][:8] == SENT).all()) and bool((pad["gbuf"][-8:] == SENT).all()), "gradient guard floats written"
    assert torch.equal(pad["probs"][:n, :G], plain["probs"])
    _same(pad, plain, keys=("mu", "logvar", "grads"))
    assert not bool((plain["grads"] == SENT).any())


# ------------------------------------------------------------------------------------------------
# d. ragged reuse and row lists
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_ragged_reuse_and_row_lists(prec, train):
    tag = "B"
    G, H, L, bm, n = SHAPES[tag]
    st = _state(tag)
    pr = _prec(prec)
    eps, dp, dmu, dlv = _dev_inputs(tag)
    # 1) a 300-row call leaves its rows 77..299 behind in the workspace
    m, ws, mat, rows = _model(tag, pr)
    assert ws.d.batch_max == bm
    g = torch.Generator().manual_seed(3)
    _run(m, ws, mat, None, bm, torch.randn(bm, L, generator=g).cuda(), torch.randn(bm, G, generator=g).cuda(),
         torch.randn(bm, L, generator=g).cuda(), torch.randn(bm, L, generator=g).cuda(), train)
    assert m.workspace(pr, bm) is ws
    # 2) the 77-row batch as an index list (with repeats) into the 700-row matrix
    assert len(set(st["rows"].tolist())) <= n - 2
    reused = _run(m, ws, mat, rows, n, eps, dp, dmu, dlv, train)
    m2, ws2, mat2, rows2 = _model(tag, pr, bm=n)
    assert ws2.d.batch_max == n
    fresh = _run(m2, ws2, mat2, rows2, n, eps, dp, dmu, dlv, train)
    _same(reused, fresh)
    m3, ws3, _, _ = _model(tag, pr, bm=n)
    dense = _run(m3, ws3, ResidentMatrix(st["xb"]), None, n, eps, dp, dmu, dlv, train)
    _same(reused, dense)
    _check_bar(tag, prec, train, m, reused)


# ------------------------------------------------------------------------------------------------
# e. GM2_BF16X3 is GM2_F32 outside training and evaluation
# ------------------------------------------------------------------------------------------------
def test_bf16x3_is_f32_on_this_surface():
    """gm2.h: every entry point but training / evaluation treats GM2_BF16X3 as GM2_F32. Shape C
    (H % 256 == 0: the split plan is live there). The training call in between runs on the BF16X3
    workspace only and leaves split buffers behind; its BatchNorm update is undone on the host so
    that the running statistics of the following calls can be compared too."""
    tag = "C"
    G, H, L, bm, n = SHAPES[tag]
    eps, dp, dmu, dlv = _dev_inputs(tag)
    runs = {}
    for name, pr in (("x3", native.GM2_BF16X3), ("f32", native.GM2_F32)):
        m, ws, mat, rows = _model(tag, pr)
        stat = lambda: (ws.stat(native.TSTAT_SPLIT_GEMMS), ws.stat(native.TSTAT_EXACT_GEMMS))  # noqa: E731
        s0 = stat()
        out = [_run(m, ws, mat, rows, n, eps, dp, dmu, dlv, 1)]
        mu, lv = torch.empty(n, L, device="cuda"), torch.empty(n, L, device="cuda")
        native.encode(ws, native.make_batch(mat.data, mat.ld, rows, n, None), m.params, m.bn, mu, lv)
        counts = torch.zeros(n, 3, dtype=torch.int32, device="cuda")
        native.recon_counts(ws, native.make_batch(mat.data, mat.ld, rows, n, eps), m.params, m.bn, 0.5, counts)
        torch.cuda.synchronize()
        out.append(dict(mu=mu, logvar=lv, counts=counts, bn=m.bn.clone()))
        assert stat() == s0, "a non-training call counted G-wide GEMMs"
        if name == "x3":
            bn0 = m.bn.clone()
            tg = torch.zeros_like(m.params)
            loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
            native.train_fwd_bwd(ws, native.make_batch(mat.data, mat.ld, rows, n, eps), m.params, tg, m.bn,
                                 scalars(beta=0.37), loss)
            torch.cuda.synchronize()
            s1 = stat()
            assert (s1[0] - s0[0]) + (s1[1] - s0[1]) == 5 and s1[0] > s0[0], (s0, s1)
            m.bn.copy_(bn0)
            s0 = s1
        out.append(_run(m, ws, mat, rows, n, eps, dp, dmu, dlv, 1))
        assert stat() == s0, "a non-training call counted G-wide GEMMs"
        runs[name] = out
    for a, b in zip(runs["x3"], runs["f32"]):
        for k in a:
            if k not in ("gbuf", "dpb"):
                assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------
# f. gm2_recon_counts
# ------------------------------------------------------------------------------------------------
def _signs(G, seed):
    return (torch.rand(G, generator=torch.Generator().manual_seed(seed)) < 0.5).double() * 2 - 1


@pytest.mark.parametrize("tag", ["A", "B"])
@pytest.mark.parametrize("thr", [0.5, 0.3, 0.9])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_recon_counts(prec, thr, tag):
    """Per-row (TP, FP, FN) of (p > thr) == the fp64 eval-mode forward's, every row, on a fixture kept
    off the threshold: decoder.9.bias = logit(thr) +- 2.5 (seeded signs), and the fixture check
    min |logit64 - logit(thr)| >= 10 * max |logit_ref_arith - logit64| from the oracle alone."""
    G, H, L, bm, n = SHAPES[tag]
    st = _state(tag)
    lthr = math.log(thr / (1 - thr))
    P = dict(st["P"])
    P["decoder.9.bias"] = (lthr + 2.5 * _signs(G, G + 1)).float()
    x = torch.tensor(st["xb"], dtype=torch.float32)
    zp, zl = torch.zeros(n, G), torch.zeros(n, L)
    l64 = O.manual_forward_backward_emulated(P, st["S"], x, st["eps"], zp, zl, zl, False)[0]["logit"]
    kw = dict(dtype=torch.float32, operand_round=O.bf16_round if prec == "bf16" else None)
    lref = O.manual_forward_backward_emulated(P, st["S"], x, st["eps"], zp, zl, zl, False, **kw)[0]["logit"].double()
    gap, err = float((l64 - lthr).abs().min()), float((lref - l64).abs().max())
    print(f"{tag} {prec} thr {thr}: min |logit64 - logit(thr)| {gap:.3g}, max |logit_ref_arith - logit64| {err:.3g}")
    assert gap >= 10 * err, "fixture: a logit lies too close to the threshold"
    pred, xb = l64 > lthr, x.bool()
    want = torch.stack([(pred & xb).sum(1), (pred & ~xb).sum(1), (~pred & xb).sum(1)], 1).to(torch.int32)
    m = to_model(P, st["S"], G, H, L, _prec(prec))
    ws = m.workspace(_prec(prec), bm)
    mat = ResidentMatrix(st["X"])
    rows = None if st["rows"] is None else st["rows"].cuda()
    counts = torch.full((n + 1, 3), -7, dtype=torch.int32, device="cuda")
    bn0 = m.bn.clone()
    native.recon_counts(ws, native.make_batch(mat.data, mat.ld, rows, n, st["eps"].cuda()), m.params, m.bn, thr, counts)
    torch.cuda.synchronize()
    assert torch.equal(counts[:n].cpu(), want)
    assert bool((counts[n] == -7).all()), "guard row of counts written"
    assert torch.equal(m.bn, bn0)


# ------------------------------------------------------------------------------------------------
# g. eval forward and encode
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["A", "B"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_eval_forward_all_slots(prec, tag):
    """gm2_eval_forward's slots [0] BCE, [1] sum p, [2] sum(1 + lv - mu^2 - exp(lv)) against the
    oracle's eval-mode sums (fp64 for f32, bf16-emulated fp32 for bf16) at the bars
    test_train_step_vs_oracle applies to the same slots; [3..7] stay 0; BatchNorm untouched."""
    G, H, L, bm, n = SHAPES[tag]
    out = _oracle(tag, 0, "exact" if prec == "f32" else "bf16")[0]
    p, mu, lv = out["probs"], out["mu"], out["logvar"]
    x = torch.tensor(_state(tag)["xb"], dtype=torch.float64)
    bce = float(-(x * torch.clamp(torch.log(p), min=-100) + (1 - x) * torch.clamp(torch.log1p(-p), min=-100)).sum())
    want = [bce, float(p.sum()), float(torch.sum(1 + lv - mu.pow(2) - lv.exp()))]
    m, ws, mat, rows = _model(tag, _prec(prec))
    bn0 = m.bn.clone()
    loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
    native.eval_forward(ws, native.make_batch(mat.data, mat.ld, rows, n, _state(tag)["eps"].cuda()), m.params, m.bn,
                        scalars(beta=0.2), loss)
    torch.cuda.synchronize()
    lt = loss.cpu().numpy()
    print(f"{tag} {prec}: loss slots {lt[:3]}, oracle {want}")
    rtol = 1e-5 if prec == "f32" else 1e-4
    assert abs(lt[0] - want[0]) <= rtol * abs(want[0]), (lt[0], want[0])
    assert abs(lt[1] - want[1]) <= rtol * abs(want[1]), (lt[1], want[1])
    assert abs(lt[2] - want[2]) <= 1e-4 * abs(want[2]) + 1e-3 * n * L * (1 if prec == "bf16" else 0.01), (lt[2], want[2])
    assert (lt[3:] == 0).all()
    assert torch.equal(m.bn, bn0)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_encode_row_list(prec):
    tag = "B"
    L, n = SHAPES[tag][2], SHAPES[tag][4]
    m, ws, mat, rows = _model(tag, _prec(prec))
    batch = native.make_batch(mat.data, mat.ld, rows, n, None)
    bn0 = m.bn.clone()
    mu, lv = torch.full((n, L), SENT, device="cuda"), torch.full((n, L), SENT, device="cuda")
    native.encode(ws, batch, m.params, m.bn, mu, lv)
    mu1, lv1 = torch.full((n, L), SENT, device="cuda"), torch.full((n, L), SENT, device="cuda")
    native.encode(ws, batch, m.params, m.bn, mu1, None)
    native.encode(ws, batch, m.params, m.bn, None, lv1)
    torch.cuda.synchronize()
    _check_bar(tag, prec, 0, m, dict(mu=mu, logvar=lv), outputs=("mu", "logvar"), grads=False)
    assert torch.equal(mu1, mu) and torch.equal(lv1, lv)
    assert torch.equal(m.bn, bn0)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_encode_matches_eval_forward_bitwise(prec):
    """gm2_encode and gm2_forward(train=0) run the same encoder schedule (same gather, same GEMM plans,
    running statistics in both; mu / logvar do not depend on eps): on one workspace, the same
    parameters and the same rows, their mu and logvar are bit-identical (shape A)."""
    tag = "A"
    G, _, L, _, n = SHAPES[tag]
    m, ws, mat, rows = _model(tag, _prec(prec))
    batch = native.make_batch(mat.data, mat.ld, rows, n, _state(tag)["eps"].cuda())
    mu_e, lv_e = torch.full((n, L), SENT, device="cuda"), torch.full((n, L), SENT, device="cuda")
    native.encode(ws, batch, m.params, m.bn, mu_e, lv_e)
    probs = torch.empty((n, G), device="cuda")
    mu_f, lv_f = torch.full((n, L), SENT, device="cuda"), torch.full((n, L), SENT, device="cuda")
    native.forward(ws, batch, m.params, m.bn, 0, probs, G, mu_f, lv_f)
    torch.cuda.synchronize()
    assert not (mu_e == SENT).any() and not (lv_e == SENT).any()
    assert torch.equal(mu_e, mu_f), f"mu differs: max |d| {float((mu_e - mu_f).abs().max()):.3g}"
    assert torch.equal(lv_e, lv_f), f"logvar differs: max |d| {float((lv_e - lv_f).abs().max()):.3g}"


# ------------------------------------------------------------------------------------------------
# h. gm2_reparameterize
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 257, 4096 * 256 + 777])
def test_reparameterize_sizes(n):
    """z only, backward only (z = NULL) and both, through the grid-stride loop (n > 4096 x 256), with 8
    guard floats after element n; n = 0 is a no-op."""
    g = torch.Generator().manual_seed(n + 1)
    mu, lv, eps, dz = (torch.randn(n + 8, generator=g).cuda() for _ in range(4))
    sd = torch.exp(0.5 * lv[:n])
    z_ref, dlv_ref = mu[:n] + sd * eps[:n], 0.5 * ((dz[:n] * eps[:n]) * sd)
    for want_z, want_bwd in ((True, False), (False, True), (True, True)):
        z, dmu, dlv = (torch.full((n + 8,), SENT, device="cuda") for _ in range(3))
        native.reparameterize(n, mu, lv, eps, z if want_z else None, dz if want_bwd else None,
                              dmu if want_bwd else None, dlv if want_bwd else None)
        torch.cuda.synchronize()
        for t in (z, dmu, dlv):
            assert bool((t[n:] == SENT).all()), "guard floats written"
        if not want_z:
            assert bool((z == SENT).all())
        if not want_bwd:
            assert bool((dmu == SENT).all()) and bool((dlv == SENT).all())
        if n == 0:
            continue
        if want_z:
            assert rel_err(z[:n].cpu(), z_ref.cpu()) <= 1e-6
        if want_bwd:
            assert torch.equal(dmu[:n], dz[:n])
            assert rel_err(dlv[:n].cpu(), dlv_ref.cpu()) <= 1e-6


# ------------------------------------------------------------------------------------------------
# i. the stale-activation guard of VAE.forward's backward
# ------------------------------------------------------------------------------------------------
def _api_model(tag, precision=None):
    G, H, L = SHAPES[tag][:3]
    st = _state(tag)
    m = VAE(G, H, L, init=False) if precision is None else VAE(G, H, L, precision=precision, init=False)
    m.load_state_dict({**st["P"], **st["S"]})
    m.requires_grad_(True)
    return m


def _api_loss(tag, out):
    _, dp, dmu, dlv = _dev_inputs(tag)
    return (out[0] * dp).sum() + (out[1] * dmu).sum() + (out[2] * dlv).sum()


def test_stale_activation_guard():
    tag = "A"
    st = _state(tag)
    x = torch.tensor(st["xb"], dtype=torch.float32)
    eps = st["eps"]
    z = torch.randn(40, SHAPES[tag][2], generator=torch.Generator().manual_seed(2))
    m = _api_model(tag)
    assert m.precision == native.GM2_BF16
    out = m(x, eps=eps)
    m.encode(x)
    with pytest.raises(RuntimeError, match="overwritten by a later call"):
        _api_loss(tag, out).backward()
    m = _api_model(tag)
    first = m(x, eps=eps)
    m(x, eps=eps)
    with pytest.raises(RuntimeError, match="overwritten by a later call"):
        _api_loss(tag, first).backward()
    # a sampling decode of a bf16 model runs on its own fp32 workspace: the activations survive
    m = _api_model(tag)
    _api_loss(tag, m(x, eps=eps)).backward()
    undisturbed = m.params.grad.detach().clone()
    m = _api_model(tag)
    out = m(x, eps=eps)
    m.decode_mask(z)
    _api_loss(tag, out).backward()
    assert torch.equal(m.params.grad, undisturbed)
    # an fp32 model shares that workspace with its decodes
    m = _api_model(tag, native.GM2_F32)
    out = m(x, eps=eps)
    m.decode_mask(z)
    with pytest.raises(RuntimeError, match="overwritten by a later call"):
        _api_loss(tag, out).backward()


# ------------------------------------------------------------------------------------------------
# j. a custom loss component trained in the default precision
# ------------------------------------------------------------------------------------------------
class LatentPenalty(LossComponent):
    """A custom component (not one of the fused built-ins): c * sum(mu^2)."""

    def __init__(self, c=0.01):
        self.c = c

    def compute_loss(self, recon_x, data, mu, logvar, model, epoch, batch_idx):
        return self.c * torch.sum(mu ** 2)

    def get_name(self):
        return "latent_penalty"


def test_custom_loss_component_trains_default_precision():
    """test_custom_loss_component_trains with VAE(G, H, L) as a user builds it (bf16), two batches per
    epoch, the last one ragged (200 rows at batch_size 128). The first batch's reconstruction term
    equals the BCE of the bf16-emulating oracle at the initial parameters within rel 1e-4."""
    G, H, L, N, BS = 640, 128, 16, 200, 128
    P, S = oracle_state(G, H, L, 31)
    X = synth_x(N, G, 9)
    m = VAE(G, H, L, init=False)
    m.load_state_dict({**P, **S})
    assert m.precision == native.GM2_BF16
    opt = Adam(m, lr=1e-3)
    tr = (VAETrainerBuilder(m, opt, StepLR(opt, 20, 0.5)).epochs(4).gradient_clipping(1.0).print_every(100)
          .with_reconstruction_loss().with_kl_loss("linear", 0.1, 1.0).with_custom_loss(LatentPenalty(0.01))
          .build(eps_rng="cpu"))
    assert not tr.loss_tracker.fused
    seen = []
    inner = tr.loss_tracker.compute_total_loss

    def recording(*a, **k):
        total, parts = inner(*a, **k)
        seen.append(dict(parts))
        return total, parts
    tr.loss_tracker.compute_total_loss = recording
    torch.manual_seed(3)
    loader = StrainLoader(ResidentMatrix(X), None, BS, shuffle=False)
    assert len(loader) == 2
    first = tr.train_epoch(loader, 0)
    assert len(seen) == 2
    # oracle at the initial parameters (same host RNG: base seed draw, then the first batch's eps)
    torch.manual_seed(3)
    torch.empty((), dtype=torch.int64).random_()
    eps = torch.randn(BS, L)
    _, sums = O.manual_grads_emulated(P, S, torch.tensor(X[:BS], dtype=torch.float32), eps, 0.1, 0.0,
                                      operand_round=O.bf16_round, dtype=torch.float32)
    print(f"first batch reconstruction: libgm2 {seen[0]['reconstruction']:.6f}, bf16-emulating oracle {sums[0]:.6f}")
    assert abs(seen[0]["reconstruction"] - sums[0]) <= 1e-4 * abs(sums[0])
    hist = [first["total"]] + [tr.train_epoch(loader, e)["total"] for e in range(1, 4)]
    assert hist[-1] < hist[0], hist
    val = tr.validate_epoch(loader, 3)
    assert set(val) == {"reconstruction", "kl_divergence", "latent_penalty", "total"}
    assert all(np.isfinite(v) for v in val.values())
