"""The row-store epilogues of the 128x128 GEMM (csrc/gemm_store.hip store_rows: plain / slab store,
bias + forward BatchNorm statistics, backward statistics) through gm2_forward(train = 1) then
gm2_backward_outputs, at the row counts where the unrolled, predicated row passes can go wrong.

Shapes: G = 300, L = 8, H in {128, 256}, B in {1, 127, 128, 129, 300}: one row, a tile short of one
row, a full tile, a second tile with one valid row, ragged multi-tile. Both precisions, with
GM2_OPT_BN_EPILOGUE 0 (every hidden GEMM a plain slab store, the statistics in their own pass) and 1
(the statistics in the GEMM's epilogue). At these sizes every GEMM plan is one K pass of 128x128
tiles (csrc/gemm_plan.hpp: fewer than 8 K-steps per slice never split).

B = 1: gm2_forward refuses train = 1 on one row ("Expected more than 1 value per channel", as
torch's BatchNorm does); the case asserts that, then runs the pair with train = 0 -- running
statistics in the forward, and the same backward statistics epilogue in the backward GEMMs.

Bars: those of tests/test_gpu_autograd_surface.py for the same quantities -- per output and gradient
tensor fro(libgm2 - exact) <= 3 * fro(reference arithmetic - exact) + floor against the float64
oracle, floor 2e-4 (f32) / 1e-3 (bf16); the pre-BatchNorm biases (true gradient zero under train-mode
BatchNorm) absolutely at 1e-3 / 2e-2 of their weight gradient's max.

Guard rows: before the calls the test fills the workspace's six pre-BatchNorm buffers Y[i]
[Bm][H] and the caller's stream's slab area (where every backward GEMM leaves dA [Bp][H]) with a
sentinel; afterwards rows >= B of each must still hold it, and rows < B of Y must not. The offsets
mirror the head of make_layout (csrc/api.hip); that the valid rows of all six Y lost the sentinel
is the check that the mirror is right.
"""
import pytest
import torch

from gpu_helpers import oracle_state, perturb_bn, synth_x, to_model
from oracle import vae_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gm2 import native
    from gm2.data import ResidentMatrix

G, L = 300, 8
HS = (128, 256)
BS = (1, 127, 128, 129, 300)
SENT = -777.25
FLOOR = {"f32": 2e-4, "bf16": 1e-3}
BIAS_LIM = {"f32": 1e-3, "bf16": 2e-2}

_STATE, _REFS = {}, {}


def _prec(prec):
    return native.GM2_F32 if prec == "f32" else native.GM2_BF16


def _prebn_bias(name):
    p = name.split(".")
    return p[0] in ("encoder", "decoder") and p[1] in ("0", "3", "6") and p[2] == "bias"


def _state(H, B):
    """Host inputs of a shape, generated once from seeds."""
    if (H, B) not in _STATE:
        k = H + B
        P, S = perturb_bn(*oracle_state(G, H, L, 100 + k), seed=k)
        g = torch.Generator().manual_seed(k)
        _STATE[(H, B)] = dict(P=P, S=S, X=synth_x(B, G, 7 * k), eps=torch.randn(B, L, generator=g),
                              dp=torch.randn(B, G, generator=g), dmu=torch.randn(B, L, generator=g),
                              dlv=torch.randn(B, L, generator=g))
    return _STATE[(H, B)]


def _oracle(H, B, train, kind):
    """(outputs, grads) of the oracle on the device as fp64 host tensors; kind 'exact' (fp64), 'f32',
    'bf16' (fp32 with bf16 operand rounding). Once per (shape, mode, kind)."""
    key = (H, B, train, kind)
    if key not in _REFS:
        st = _state(H, B)
        dev = torch.device("cuda")
        torch.backends.cuda.matmul.allow_tf32 = False
        kw = {} if kind == "exact" else dict(dtype=torch.float32, operand_round=O.bf16_round if kind == "bf16" else None)
        out, gr = O.manual_forward_backward_emulated(
            {k: v.to(dev) for k, v in st["P"].items()}, {k: v.to(dev) for k, v in st["S"].items()},
            torch.tensor(st["X"], dtype=torch.float32, device=dev), st["eps"].to(dev), st["dp"].to(dev),
            st["dmu"].to(dev), st["dlv"].to(dev), bool(train), **kw)
        _REFS[key] = ({k: out[k].double().cpu() for k in ("probs", "mu", "logvar")},
                      {k: v.double().cpu() for k, v in gr.items()})
    return _REFS[key]


def _round_up(x, m):
    return (x + m - 1) // m * m


def _regions(ws, H, prec):
    """Float views of the workspace's Y[0..5] [Bm][H] and of the first Bm * H floats of the caller's
    stream's slab area: the head of make_layout (csrc/api.hip), every region rounded up to 256 bytes."""
    es = 4 if prec == "f32" else 2
    Bm = _round_up(ws.d.batch_max, 128)
    Gp = _round_up(G, 128 if prec == "f32" else 256)
    Lr, L2r = _round_up(_round_up(L, 64), 128), _round_up(2 * L, 128)
    cur = 0

    def take(nbytes):
        nonlocal cur
        at = cur
        cur += _round_up(nbytes, 256)
        return at
    for nb in (H * Gp, H * H, H * H, L2r * H, H * Lr, H * H, H * H, Gp * H, Bm * Gp):  # shadows, X
        take(nb * es)
    take(Bm * (Gp // 32) * 4)  # XB
    y = []
    for _ in range(6):
        y.append(take(Bm * H * 4))
        take(Bm * H * es)      # A
        take(2 * H * 4)        # save
    take(Bm * 2 * L * 4)       # HD
    take(Bm * Lr * es)         # Z
    take(Bm * Gp * es)         # dL
    slabs = take(0)
    assert slabs + Bm * H * 4 <= ws.nbytes
    f = ws.buf[ws.off:ws.off + ws.nbytes].view(torch.float32)
    view = lambda at: f[at // 4: at // 4 + Bm * H].view(Bm, H)  # noqa: E731
    return [view(a) for a in y], view(slabs), Bm


def _run(H, B, prec, opt, train):
    st = _state(H, B)
    m = to_model(st["P"], st["S"], G, H, L, _prec(prec))
    ws = m.workspace(_prec(prec), B)
    ws.set_option(native.OPT_BN_EPILOGUE, opt)
    assert ws.get_option(native.OPT_BN_EPILOGUE) == opt
    mat = ResidentMatrix(st["X"])
    ys, slab, Bm = _regions(ws, H, prec)
    for t in ys + [slab]:
        t.fill_(SENT)
    dev = m.device
    probs = torch.full((B, G), SENT, device=dev)
    mu, lv = torch.full((B, L), SENT, device=dev), torch.full((B, L), SENT, device=dev)
    grads = torch.full((m.n_params,), SENT, device=dev)
    batch = native.make_batch(mat.data, mat.ld, None, B, st["eps"].cuda())
    native.forward(ws, batch, m.params, m.bn, train, probs, G, mu, lv)
    native.backward_outputs(ws, batch, m.params, train, probs, G, st["dp"].cuda(), st["dmu"].cuda(), st["dlv"].cuda(),
                            grads)
    torch.cuda.synchronize()
    return m, dict(probs=probs, mu=mu, logvar=lv, grads=grads), ys, slab, Bm


@pytest.mark.parametrize("opt", [1, 0])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H", HS)
def test_forward_backward_rows(H, B, prec, opt):
    train = 1
    if B == 1:  # one row: train-mode BatchNorm is refused; the pair runs in eval mode
        st = _state(H, B)
        m0 = to_model(st["P"], st["S"], G, H, L, _prec(prec))
        mat = ResidentMatrix(st["X"])
        with pytest.raises(RuntimeError, match="more than 1 value"):
            native.forward(m0.workspace(_prec(prec), B), native.make_batch(mat.data, mat.ld, None, B, st["eps"].cuda()),
                           m0.params, m0.bn, 1, torch.empty(B, G, device="cuda"), G)
        train = 0
    m, res, ys, slab, Bm = _run(H, B, prec, opt, train)
    fails = []
    # guard rows
    for i, y in enumerate(ys):
        if not bool((y[B:] == SENT).all()):
            fails.append(f"Y[{i}]: a row >= {B} of {Bm} was written")
        if bool((y[:B] == SENT).any()) or not bool(torch.isfinite(y[:B]).all()):
            fails.append(f"Y[{i}]: rows < {B} not all written")
    if not bool((slab[B:] == SENT).all()):
        fails.append(f"dA (slab area): a row >= {B} of {Bm} was written")
    # the bars
    ex_o, ex_g = _oracle(H, B, train, "exact")
    rf_o, rf_g = _oracle(H, B, train, prec)

    def bar(name, got, ex, ref):
        got, ex, ref = got.double().cpu().reshape(-1), ex.reshape(-1), ref.reshape(-1)
        nrm = max(float(torch.linalg.norm(ex)), 1e-30)
        f_gpu, f_ref = float(torch.linalg.norm(got - ex)) / nrm, float(torch.linalg.norm(ref - ex)) / nrm
        msg = (f"H={H} B={B} {prec} bn_epilogue={opt} train={train} {name}: libgm2 vs exact fro {f_gpu:.3g}; "
               f"reference arithmetic fro {f_ref:.3g}")
        print(msg)
        if not f_gpu <= 3 * f_ref + FLOOR[prec]:
            fails.append(msg)
    for name in ("probs", "mu", "logvar"):
        bar(name, res[name], ex_o[name], rf_o[name])
    off = m.offsets
    for i, (name, _) in enumerate(m.specs):
        got = res["grads"][off[i]:off[i + 1]]
        if train and _prebn_bias(name):
            scale = max(float(ex_g[name.replace("bias", "weight")].abs().max()), 1e-12)
            gmax = float(got.abs().max())
            print(f"H={H} B={B} {prec} bn_epilogue={opt} {name}: |g|max {gmax:.3g} vs weight gradient max {scale:.3g}")
            if not gmax <= BIAS_LIM[prec] * scale:
                fails.append(f"{name}: |g|max {gmax:.3g} vs weight gradient max {scale:.3g}")
            continue
        bar(name, got, ex_g[name], rf_g[name])
    assert not fails, "\n".join(fails)
