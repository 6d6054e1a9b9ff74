"""The optimizer pass, element by element: gm2_grad_norm (k_grad_stats, k_grad_finalize), gm2_adam_step
(k_adam_fused / adam_block) and the GEMM weight shadows they and gm2_sync_shadows (k_shadow_sync) write.

Inputs are synthetic (gpu_helpers.adam_inputs: nonzero moments, exact zeros, -0.0), so no GEMM runs except
where a case says so. The reference is gpu_helpers.adam_reference: the update in float64 with per-element
fp32 bounds, calibrated in tests/test_optimizer_cpu.py (an honest fp32 evaluation stays within half of
them; six one-line mutants of the update leave them). Shadows are compared bit for bit with the image
gpu_helpers.expected_shadows builds from the parameters.

Shapes (G, H, L): G mod 4 = 1, 2, 3 (partial blocks, a decoder.9.bias tail of 1..3 elements, the
element-wise shadow path with its row wrap inside a vector of four), the all-vector path, a model of more
than 2048 x 256 parameters (k_grad_stats strides and has a scalar tail), and latent widths 2 and 1, whose
tensors behind logvar_layer sit at flat offsets that are not multiples of four.
"""
import numpy as np
import pytest
import torch

from gm2 import native
from gm2.data import ResidentMatrix
from gm2.model import param_specs
from oracle import vae_oracle as O

from gpu_helpers import (adam_inputs, adam_reference, expected_shadows, grad_bar_failures, oracle_state, perturb_bn,
                         scalars, shadow_views, synth_x, to_model)

pytestmark = pytest.mark.gpu

PRECS = {"f32": native.GM2_F32, "bf16": native.GM2_BF16, "bf16x3": native.GM2_BF16X3}
SHAPES = [(517, 128, 16), (518, 128, 16), (519, 128, 16), (1024, 256, 64), (1031, 256, 32), (300, 128, 2),
          (300, 128, 1)]
CASES = [(s, p) for s in SHAPES for p in ("f32", "bf16")] + [((517, 128, 16), "bf16x3")]  # bf16x3: must behave as f32
CASE_IDS = [f"{g}-{h}-{l}-{p}" for (g, h, l), p in CASES]
GUARD = 64
U = 2.0 ** -24
LAMS = (0.0, 0.01)
MAX_NORMS = ("one", "off", "above")  # max_norm = 1 (clipped), 0 (no clipping), twice the norm (coefficient 1)


class State:
    """Synthetic p, g, m, v of one model shape on the device, each between two guards of GUARD floats,
    with a workspace of its own (fresh: no training call has recorded norm-ahead statistics)."""

    def __init__(self, G, H, L, prec, seed, batch_max=128):
        self.G, self.H, self.L = G, H, L
        self.specs = param_specs(G, H, L)
        self.offsets = native.param_offsets(G, H, L)
        self.n = self.offsets[-1]
        self.host = dict(zip("pgmv", adam_inputs(self.n, seed)))
        self.guard = torch.arange(GUARD, dtype=torch.float32) + 1024.5
        self.buf = {k: torch.empty(self.n + 2 * GUARD, device="cuda") for k in "pgmv"}
        self.reset()
        self.ws = native.Workspace(native.dims(G, H, L, batch_max), PRECS[prec], torch.device("cuda"))

    def reset(self):
        for k, a in self.host.items():
            self.buf[k].copy_(torch.cat([self.guard, torch.from_numpy(a), self.guard]))

    def dev(self, k):
        return self.buf[k][GUARD:GUARD + self.n]

    def get(self, k):
        return self.dev(k).cpu().numpy()

    def guards_untouched(self):
        for k in "pgmv":
            b = self.buf[k].cpu()
            assert torch.equal(b[:GUARD], self.guard) and torch.equal(b[-GUARD:], self.guard), f"guard of {k} written"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def assert_shadows(ws, params, specs, offsets, what, only=None):
    """Every shadow region (or the regions `only`) holds exactly cvt(params) in place and zeros elsewhere."""
    torch.cuda.synchronize()
    views, img = shadow_views(ws), expected_shadows(ws, params, specs, offsets)
    for k in only or views:
        got = views[k].cpu()
        if not torch.equal(_bits(got), _bits(img[k])):
            bad = (_bits(got) != _bits(img[k])).nonzero()
            r, c = (int(x) for x in bad[0])
            raise AssertionError(f"{what}: shadow {k} {tuple(got.shape)} differs at {len(bad)} elements, first "
                                 f"[{r}][{c}]: {got[r, c].item()!r} vs {img[k][r, c].item()!r}")


def norm_reference(p, g, lam):
    """float64 norm of fp32(g + lam * sign(p)) and float64 sum |p|."""
    a = (g + np.float32(lam) * np.sign(p)).astype(np.float32) if lam else g
    return float(np.sqrt(np.sum(a.astype(np.float64) ** 2))), float(np.sum(np.abs(p.astype(np.float64))))


def clip_coef(norm_slot, max_norm):
    """The clip coefficient as k_grad_finalize computes it, in fp32, from loss slot 4."""
    norm, mx = np.float32(norm_slot), np.float32(max_norm)
    if not mx > 0:
        return np.float32(1)
    return min(np.float32(mx / np.float32(norm + np.float32(1e-6))), np.float32(1))


def max_norm_of(case, norm):
    return {"one": 1.0, "off": 0.0, "above": 2.0 * norm}[case]


def run_grad_norm(st, lam, max_norm, step=1):
    """gm2_grad_norm with S_NORM_AHEAD = 1 (nothing recorded: the kernel must fall back to the full read);
    returns (scalar block, its host copy, loss slots 3 and 4)."""
    sc = scalars(lam=lam, step=step, max_norm=max_norm)
    sc[native.S_NORM_AHEAD] = 1.0
    loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
    native.grad_norm(st.ws, st.dev("p"), st.dev("g"), sc, loss)
    lt = loss.cpu().numpy()
    return sc, sc.cpu().numpy(), float(lt[3]), float(lt[4])


def bound_failures(ref, got, label, ranges=None):
    """Lines for every tensor class whose elements leave their bound (count and worst); prints the worst
    error / bound per class. `ranges`: only these (lo, hi) element ranges."""
    fails = []
    for k in "pmv":
        r, tol = ref[k]
        err = np.abs(got[k].astype(np.float64) - r)
        if ranges is not None:
            keep = np.zeros(err.shape, dtype=bool)
            for lo, hi in ranges:
                keep[lo:hi] = True
            err = np.where(keep, err, 0.0)
        ratio = np.where(err > 0, err / np.where(tol > 0, tol, 1e-300), 0.0)
        w = int(np.argmax(ratio))
        print(f"{label}: {k}' worst error / bound {ratio[w]:.3f}")
        out = int((err > tol).sum())
        if out or not np.isfinite(got[k]).all():
            fails.append(f"{label}: {k}' {out} of {err.size} elements outside the bound; worst at {w}: got "
                         f"{got[k][w]!r}, reference {r[w]!r}, error {err[w]:.3g}, bound {tol[w]:.3g}")
    return fails


@pytest.mark.parametrize("shape,prec", CASES, ids=CASE_IDS)
def test_grad_norm_slots(shape, prec):
    """Loss slot 4 = the norm of fp32(g + lam sign(p)) within 4 u relative (fp64 sums, one sqrt and one
    rounding to fp32 in the kernel), slot 3 = sum |p| within 1e-12 relative (fp64 sums of exact terms),
    exactly 0 without an L1 term; whatever max_norm is."""
    st = State(*shape, prec, seed=11)
    p, g = st.host["p"], st.host["g"]
    for lam in LAMS:
        norm, l1 = norm_reference(p, g, lam)
        assert norm > 1.0
        for case in MAX_NORMS:
            _, _, s3, s4 = run_grad_norm(st, lam, max_norm_of(case, norm))
            print(f"lam {lam} max_norm {case}: norm {s4!r} vs {norm!r} ({abs(s4 - norm) / (U * norm):.2f} u), "
                  f"sum |p| {s3!r} vs {l1!r}")
            assert abs(s4 - norm) <= 4 * U * norm, (lam, case, s4, norm)
            if lam:
                assert abs(s3 - l1) <= 1e-12 * l1, (lam, case, s3, l1)
            else:
                assert s3 == 0.0
    st.guards_untouched()
    for k in "pg":
        assert np.array_equal(st.get(k).view(np.int32), st.host[k].view(np.int32))


@pytest.mark.parametrize("shape,prec", CASES, ids=CASE_IDS)
def test_sync_shadows_image(shape, prec):
    st = State(*shape, prec, seed=12)
    native.sync_shadows(st.ws, st.dev("p"))
    assert_shadows(st.ws, st.dev("p"), st.specs, st.offsets, "after sync_shadows")
    st.guards_untouched()


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("shape,prec", CASES, ids=CASE_IDS)
def test_adam_step_elementwise(shape, prec, step):
    """Every element of p', m', v' inside adam_reference's bounds, for lam in {0, 0.01} and max_norm = 1
    (the norm is above it: clipped), 0 and above the norm (coefficient 1), the coefficient recomputed in
    fp32 from loss slot 4; guards untouched; every shadow the image of the new parameters."""
    st = State(*shape, prec, seed=13)
    native.sync_shadows(st.ws, st.dev("p"))
    h = st.host
    fails = []
    for lam in LAMS:
        norm, _ = norm_reference(h["p"], h["g"], lam)
        for case in MAX_NORMS:
            st.reset()
            sc, sch, _, s4 = run_grad_norm(st, lam, max_norm_of(case, norm), step)
            cc = clip_coef(s4, sch[native.S_MAX_NORM])
            assert (cc < 1) == (case == "one"), (case, cc, s4)
            native.adam_step(st.ws, st.dev("p"), st.dev("g"), st.dev("m"), st.dev("v"), sc)
            torch.cuda.synchronize()
            ref = adam_reference(h["p"], h["g"], h["m"], h["v"], sch, cc)
            label = f"step {step} lam {lam} max_norm {case} (cc {cc:.4g})"
            fails += bound_failures(ref, {k: st.get(k) for k in "pmv"}, label)
            st.guards_untouched()
            assert np.array_equal(st.get("g").view(np.int32), h["g"].view(np.int32))
            assert_shadows(st.ws, st.dev("p"), st.specs, st.offsets, "after adam_step, " + label)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_deferred_output_update_on_the_capped_grid(prec):
    """GM2_OPT_DEFER_OUTPUT_ADAM = 1: gm2_adam_step updates the first 28 tensors and queues decoder.9.*;
    the next training call launches that on CUs workgroups, fewer than its blocks, so workgroups take a
    second block and the table index advances from decoder.9.weight into decoder.9.bias inside the loop."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    H, L, B = 256, 16, 128
    G = 24 * cus + 1  # odd; about 1.5 CUs blocks of 4096 elements
    blocks = -(-G * H // 4096) + -(-G // 4096)
    assert G % 2 == 1 and cus < blocks < 2 * cus, (cus, G, blocks)
    st = State(G, H, L, prec, seed=14, batch_max=B)
    ws, h = st.ws, st.host
    assert ws.get_option(native.OPT_SIDE_STREAM) != 0
    ws.set_option(native.OPT_DEFER_OUTPUT_ADAM, 1)
    native.sync_shadows(ws, st.dev("p"))
    lam, step = 0.01, 7
    sc, sch, _, s4 = run_grad_norm(st, lam, 1.0, step)
    cc = clip_coef(s4, 1.0)
    assert cc < 1
    native.adam_step(ws, st.dev("p"), st.dev("g"), st.dev("m"), st.dev("v"), sc)
    torch.cuda.synchronize()
    o9 = st.offsets[28]
    for k in "pmv":  # the output layer waits for the next training call
        assert np.array_equal(st.get(k)[o9:].view(np.int32), h[k][o9:].view(np.int32)), k
    ref = adam_reference(h["p"], h["g"], h["m"], h["v"], sch, cc)
    fails = bound_failures(ref, {k: st.get(k) for k in "pmv"}, "first 28 tensors", [(0, o9)])
    # one training call on the same gradient buffer, as the trainer does: it launches the queued update
    mat = ResidentMatrix(synth_x(B, G, 15))
    eps = torch.randn(B, L, generator=torch.Generator().manual_seed(16)).cuda()
    bn = torch.zeros(6, 2, H)
    bn[:, 1] = 1.0
    bn = bn.cuda()
    loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
    native.train_fwd_bwd(ws, native.make_batch(mat.data, mat.ld, None, B, eps), st.dev("p"), st.dev("g"), bn,
                         scalars(beta=0.37, lam=lam, step=step + 1), loss)
    ws.join()
    torch.cuda.synchronize()
    fails += bound_failures(ref, {k: st.get(k) for k in "pmv"}, "all thirty tensors")
    assert not fails, "\n".join(fails)
    for k in "pmv":
        b = st.buf[k].cpu()
        assert torch.equal(b[:GUARD], st.guard) and torch.equal(b[-GUARD:], st.guard), f"guard of {k} written"
    assert_shadows(ws, st.dev("p"), st.specs, st.offsets, "after the deferred update")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("L", [2, 1])
def test_small_latent_training_step(L, prec):
    """A real step at latent widths 2 and 1 (default options): the flat offsets of logvar_layer.* (L = 2)
    and of every tensor behind mean_layer.bias (L = 1) are not multiples of four. The gradients pass the
    bar of test_train_step_vs_oracle (same floors), the Adam result (nonzero moments, step 7) lies inside
    the bounds from the GPU's own gradients, and the shadows are the image of the new parameters."""
    G, H, B = 300, 128, 130
    beta, wg, lam, step = 0.37, 0.55, 0.01, 7
    P, S = perturb_bn(*oracle_state(G, H, L, G + B + L), seed=9)
    X = synth_x(B, G, B)
    torch.manual_seed(1)
    eps = torch.randn(B, L)
    pr = PRECS[prec]
    m = to_model(P, S, G, H, L, pr)
    assert any(o % 4 for o in m.offsets[:-1])
    mat = ResidentMatrix(X)
    ws = m.workspace(pr, B)
    grads = torch.zeros_like(m.params)
    loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
    sc = scalars(beta=beta, wgamma=wg, lam=lam, step=step)
    ed = eps.cuda()
    native.train_fwd_bwd(ws, native.make_batch(mat.data, mat.ld, None, B, ed), m.params, grads, m.bn, sc, loss)
    native.grad_norm(ws, m.params, grads, sc, loss)
    torch.cuda.synchronize()
    dev = torch.device("cuda")
    x = torch.tensor(X, dtype=torch.float32).to(dev)
    Pd = {k: v.to(dev) for k, v in P.items()}
    Sd = {k: v.to(dev) for k, v in S.items()}
    exact, _ = O.manual_grads_emulated(Pd, Sd, x, ed, beta, wg)
    ref, _ = O.manual_grads_emulated(Pd, Sd, x, ed, beta, wg, operand_round=O.bf16_round if prec == "bf16" else None,
                                     dtype=torch.float32)
    fails = grad_bar_failures(m.specs, m.offsets, grads, exact, ref, floor=2e-4 if prec == "f32" else 1e-3,
                              bias_tol=1e-3 if prec == "f32" else 2e-2, label=prec)
    assert not fails, "\n".join(fails)
    p0, g0 = m.params.cpu().numpy(), grads.cpu().numpy()
    norm, l1 = norm_reference(p0, g0, lam)
    lt = loss.cpu().numpy()
    assert abs(lt[4] - norm) <= 4 * U * norm and abs(lt[3] - l1) <= 1e-12 * l1
    _, _, m0, v0 = adam_inputs(m.n_params, seed=17)
    mom, vel = torch.from_numpy(m0).cuda(), torch.from_numpy(v0).cuda()
    native.adam_step(ws, m.params, grads, mom, vel, sc)
    torch.cuda.synchronize()
    aref = adam_reference(p0, g0, m0, v0, sc.cpu().numpy(), clip_coef(lt[4], 1.0))
    got = {"p": m.params.cpu().numpy(), "m": mom.cpu().numpy(), "v": vel.cpu().numpy()}
    fails = bound_failures(aref, got, f"L {L} {prec}")
    assert not fails, "\n".join(fails)
    assert_shadows(ws, m.params, m.specs, m.offsets, "after the step")
