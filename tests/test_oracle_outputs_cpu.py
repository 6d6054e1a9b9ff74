"""oracle.manual_forward_backward_emulated: VAE.forward and the backward of its three outputs for
given upstream gradients (what gm2_forward + gm2_backward_outputs compute), pinned on the CPU:

  * fp64, unrounded, train and eval BatchNorm: outputs == O.forward's, every gradient == torch
    autograd through O.forward of (probs * dprobs).sum() + (mu * dmu).sum() + (lv * dlv).sum(),
    within rel 1e-10 of the tensor's max;
  * train mode with the fused loss's own upstream gradients == manual_grads_emulated tensor by
    tensor, in fp64 unrounded and in fp32 with bf16 operand rounding (the same operations in the same
    order: the same floats);
  * None heads == zero tensors.
"""
import pytest
import torch

from oracle import vae_oracle as O

G, H, L, N = 37, 128, 16, 9


def _perturb_bn(P, S, seed):
    g = torch.Generator().manual_seed(seed)
    for bn in O.BNS:
        P[bn + ".weight"] = 0.8 + 0.4 * torch.rand(H, generator=g)
        P[bn + ".bias"] = 0.2 * torch.rand(H, generator=g) - 0.1
        S[bn + ".running_mean"] = 0.4 * torch.rand(H, generator=g) - 0.2
        S[bn + ".running_var"] = 0.5 + torch.rand(H, generator=g)
    return P, S


@pytest.fixture(scope="module")
def state():
    torch.manual_seed(41)
    P, S = _perturb_bn(O.init_params(G, H, L), O.init_bn_state(H), 7)
    g = torch.Generator().manual_seed(8)
    x = (torch.rand(N, G, generator=g) < 0.3).float()
    eps = torch.randn(N, L, generator=g)
    up = (torch.randn(N, G, generator=g), torch.randn(N, L, generator=g), torch.randn(N, L, generator=g))
    return P, S, x, eps, up


def _rel(a, b):
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-300))


@pytest.mark.parametrize("train", [True, False])
def test_matches_autograd_fp64(state, train):
    P, S, x, eps, (dp, dmu, dlv) = state
    out, grads = O.manual_forward_backward_emulated(P, S, x, eps, dp, dmu, dlv, train)
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    S64 = {k: (v.double().clone() if v.is_floating_point() else v.clone()) for k, v in S.items()}
    probs, mu, lv = O.forward(P64, S64, x.double(), eps.double(), train=train)
    for name, ref in (("probs", probs), ("mu", mu), ("logvar", lv)):
        assert out[name].dtype == torch.float64
        assert _rel(out[name], ref.detach()) <= 1e-12, name
    ((probs * dp.double()).sum() + (mu * dmu.double()).sum() + (lv * dlv.double()).sum()).backward()
    assert list(grads) == [n for n, _ in O.param_specs(G, H, L)]
    for n, v in P64.items():
        assert grads[n].shape == v.shape
        if train and n.split(".")[1] in ("0", "3", "6") and n.endswith("bias") and n[0] in "ed":
            # exactly zero in exact arithmetic (the batch mean is subtracted): both are rounding noise
            scale = float(P64[n.replace("bias", "weight")].grad.abs().max())
            assert float(grads[n].abs().max()) <= 1e-10 * scale and float(v.grad.abs().max()) <= 1e-10 * scale, n
            continue
        assert _rel(grads[n], v.grad) <= 1e-10, n
    if not train:  # eval-mode BatchNorm is affine: the pre-BatchNorm biases have a real gradient
        for lin in ("encoder.0", "encoder.3", "encoder.6", "decoder.0", "decoder.3", "decoder.6"):
            assert float(grads[lin + ".bias"].abs().max()) > 1e-3 * float(grads[lin + ".weight"].abs().max())


@pytest.mark.parametrize("rounding", ["fp64", "bf16"])
def test_fused_loss_upstream_equals_manual_grads_emulated(state, rounding):
    """dprobs = (p - x) / clamp((1 - p) p, 1e-12) + wgamma, dmu = beta mu, dlv = -0.5 beta (1 - exp(lv)):
    the fused loss's upstream gradients give manual_grads_emulated's gradients."""
    P, S, x, eps, _ = state
    beta, wg = 0.37, 0.55
    kw = dict(operand_round=O.bf16_round, dtype=torch.float32) if rounding == "bf16" else {}
    ref, _ = O.manual_grads_emulated(P, S, x, eps, beta, wg, **kw)
    dt = kw.get("dtype", torch.float64)
    zero = torch.zeros(N, G)
    out, _ = O.manual_forward_backward_emulated(P, S, x, eps, zero, None, None, True, **kw)
    p, mu, lv = out["probs"], out["mu"], out["logvar"]
    dp = (p - x.to(dt)) / torch.clamp((1 - p) * p, min=1e-12) + wg
    dmu = beta * mu
    dlv = -0.5 * beta * (1 - torch.exp(lv))
    out2, grads = O.manual_forward_backward_emulated(P, S, x, eps, dp, dmu, dlv, True, **kw)
    assert torch.equal(out2["probs"], p)
    for n in P:
        assert grads[n].dtype == dt
        assert torch.equal(grads[n], ref[n]), f"{n}: rel {_rel(grads[n], ref[n]):.3g}"


@pytest.mark.parametrize("train", [True, False])
def test_none_heads_are_zero_heads(state, train):
    P, S, x, eps, (dp, dmu, dlv) = state
    z = torch.zeros(N, L)
    for a, b in ((dmu, None), (None, dlv), (None, None)):
        _, g_none = O.manual_forward_backward_emulated(P, S, x, eps, dp, a, b, train, operand_round=O.bf16_round,
                                                       dtype=torch.float32)
        _, g_zero = O.manual_forward_backward_emulated(P, S, x, eps, dp, z if a is None else a, z if b is None else b,
                                                       train, operand_round=O.bf16_round, dtype=torch.float32)
        for n in P:
            assert torch.equal(g_none[n], g_zero[n]), n
