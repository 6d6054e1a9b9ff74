"""The bf16x3 training precision (gm2.h GM2_BF16X3) on the GPU: GM2_F32 in everything except the
five gene-wide GEMMs of a training / evaluation call, which run as split-bf16 products
(hi = bf16_rne(x), lo = bf16_rne(x - hi); hi.hi + hi.lo + lo.hi accumulated in fp32).

  1. gm2_split_operand is exact: hi / lo bit for bit torch's, at the documented positions, pads zero.
  2. gm2_gemm(GM2_BF16X3) against the fp64 sum of the same three products of the same split
     operands, elementwise within 3 (2K) 2^-24 (|Phi| + |Plo|) (|Qhi| + |Qlo|)^T: bf16 x bf16
     products are exact in fp32, so only the accumulation rounds (the factor 3 covers the three
     product streams and the split-K summation). A 0/1 P against integer-valued Q is exact.
  3. One training step (train, grad_norm, Adam) at G = 8200, H = 256, L = 32, B = 8155 with the v1
     terms live (Gp = 8448 = 33 x 256, Bp = 8192: all five GEMMs on 256 x 256 tiles, unaligned G and
     B so the zero pads of hi and lo matter along M / N and K), held to the GM2_F32 bars of
     test_gpu_c2.py: per tensor fro(libgm2) <= 3 fro(torch fp32 oracle) + 2e-4 against the fp64
     oracle, losses [0], [1] rel 1e-5, [2] 1e-4 |.| + 1e-2, clip norm rel 1e-4, sum |theta| rel 1e-6,
     pre-BN biases absolutely, Adam abs 2e-7; GM2_TSTAT_SPLIT_GEMMS advances by exactly 5. The same
     step with GM2_OPT_SIDE_STREAM = 0 (dW9 shrinks from 8 to 7 split-K slices against its scratch
     either way) is that one bit for bit.
  4. The split weights follow the parameters: three consecutive steps at lr 1e-3 (deferred output-layer
     Adam on and off) within rel 1e-4 of the fp32 oracle's BCE trajectory, then new parameters +
     sync_shadows: the next step equals a freshly built model's bit for bit.
  5. GM2_OPT_TRAIN_SPLIT = 0 is GM2_F32 bit for bit (gradients, loss slots, BatchNorm running
     statistics), at the small shape (700, 128, 16, B = 96) and the shape of 3; with the option on
     the small shape passes the bars of 3 whichever kernels it takes.
  6. gm2_eval_forward: loss slots [0..2] against the fp64 oracle's eval-mode forward.
"""
import numpy as np
import pytest
import torch

from gpu_helpers import perturb_bn, scalars, to_model
from oracle import vae_oracle as O

pytestmark = pytest.mark.gpu

BETA, WG, LAM = 0.1, 1.0, 0.01
BIG = (8200, 256, 32, 8155)
SMALL = (700, 128, 16, 96)


def _prebn_bias(name):
    p = name.split(".")
    return p[0] in ("encoder", "decoder") and p[1] in ("0", "3", "6") and p[2] == "bias"


# ------------------------------------------------------------------------------ 1. the split pass
def _split_ref(x):
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return hi, lo


def test_split_operand_exact():
    from gm2 import native
    torch.manual_seed(11)
    rows, K = 300, 96
    x = (torch.randn(rows, K) * torch.exp(3 * torch.randn(rows, K))).cuda()
    hi, lo = _split_ref(x)
    bits = lambda t: t.view(torch.int16)  # noqa: E731
    # K-major: [512][2K], element (r, k): hi at (k / 32) * 64 + k % 32, lo 32 further
    out = native.split_operand(x, kmajor=True)
    assert out.shape == (512, 2 * K) and out.dtype == torch.bfloat16
    o = out.view(512, K // 32, 2, 32)
    assert torch.equal(bits(o[:rows, :, 0, :].reshape(rows, K)), bits(hi))
    assert torch.equal(bits(o[:rows, :, 1, :].reshape(rows, K)), bits(lo))
    assert (bits(out[rows:]) == 0).all()
    # MN-major: [2K][512], element (r, k): hi at k-row (k / 32) * 64 + k % 32, lo 32 k-rows further
    out = native.split_operand(x, kmajor=False)
    assert out.shape == (2 * K, 512)
    o = out.view(K // 32, 2, 32, 512)
    assert torch.equal(bits(o[:, 0, :, :rows].reshape(K, rows)), bits(hi.t().contiguous()))
    assert torch.equal(bits(o[:, 1, :, :rows].reshape(K, rows)), bits(lo.t().contiguous()))
    assert (bits(out[:, rows:]) == 0).all()
    with pytest.raises(RuntimeError, match="multiple of 32"):
        native.split_operand(x[:, :40].contiguous())


# ------------------------------------------------------------------------------ 2. the GEMM primitive
def _parts(x):
    hi, lo = _split_ref(x)
    return hi.double(), lo.double()


@pytest.mark.parametrize("K,splits", [(32, 1), (96, 1), (1056, 3)])
@pytest.mark.parametrize("pk,qk", [(1, 1), (1, 0), (0, 0)])
def test_gemm_bf16x3(pk, qk, K, splits):
    from gm2 import native
    M, N = 300, 256
    torch.manual_seed(100 + K)
    P = torch.randn(M, K).cuda()
    Q = (torch.randn(N, K) * 0.5).cuda()
    Ps = native.split_operand(P, kmajor=bool(pk))
    Qs = native.split_operand(Q, kmajor=bool(qk))
    assert (Ps.shape[0] if pk else Ps.shape[1]) == 512
    C = torch.full((M, N), float("nan"), device="cuda")
    slab = torch.empty(splits * M * N, device="cuda") if splits > 1 else None
    native.gemm(native.GM2_BF16X3, Ps, Ps.stride(0), Qs, Qs.stride(0), C, N, M, N, K, splits=splits, slab=slab,
                p_kmajor=bool(pk), q_kmajor=bool(qk))
    torch.cuda.synchronize()
    ph, pl = _parts(P)
    qh, ql = _parts(Q)
    ref = ph @ qh.t() + ph @ ql.t() + pl @ qh.t()
    bound = 3 * (2 * K) * 2.0 ** -24 * ((ph.abs() + pl.abs()) @ (qh.abs() + ql.abs()).t())
    err = (C.double() - ref).abs()
    print(f"K={K} splits={splits} ({pk},{qk}): max err / bound {float((err / bound).max()):.3g}; "
          f"max err {float(err.max()):.3g} vs fp32-product distance {float((ref - P.double() @ Q.double().t()).abs().max()):.3g}")
    assert bool((err <= bound).all())


def test_gemm_bf16x3_exact_integers():
    """A 0/1 P operand (exact in bf16: its lo part is zero) against integer-valued bf16 Q: every
    product and every partial sum is an integer below 2^24, so the result is the integer product."""
    from gm2 import native
    M, N, K = 300, 256, 96
    g = torch.Generator().manual_seed(3)
    P = (torch.rand(M, K, generator=g) < 0.4).float().cuda()
    Q = torch.randint(-128, 129, (N, K), generator=g).float().cuda()
    for pk, qk in ((1, 1), (1, 0), (0, 0)):
        Ps = native.split_operand(P, kmajor=bool(pk))
        Qs = native.split_operand(Q, kmajor=bool(qk))
        C = torch.full((M, N), float("nan"), device="cuda")
        native.gemm(native.GM2_BF16X3, Ps, Ps.stride(0), Qs, Qs.stride(0), C, N, M, N, K, p_kmajor=bool(pk),
                    q_kmajor=bool(qk))
        assert torch.equal(C, P @ Q.t()), (pk, qk)


# ------------------------------------------------------------------------------ shared state / references
_CACHE = {}


def _state(shape):
    key = ("state", shape)
    if key not in _CACHE:
        from gm2.data import synthetic_pangenome
        G, H, L, B = shape
        torch.manual_seed(2024)
        P = O.init_params(G, H, L)
        S = O.init_bn_state(H)
        P, S = perturb_bn(P, S, 99)
        X = synthetic_pangenome(B, G, seed=12345)
        torch.manual_seed(5)
        eps = torch.randn(B, L)
        _CACHE[key] = (P, S, X, eps)
    return _CACHE[key]


def _refs(shape):
    """fp64 (exact) and torch-fp32 oracle gradients and loss sums of one step, computed once."""
    key = ("refs", shape)
    if key not in _CACHE:
        P, S, X, eps = _state(shape)
        dev = torch.device("cuda")
        Pd = {k: v.to(dev) for k, v in P.items()}
        Sd = {k: v.to(dev) for k, v in S.items()}
        x = torch.tensor(X, device=dev)
        ed = eps.to(dev)
        torch.backends.cuda.matmul.allow_tf32 = False
        exact, sums = O.manual_grads_emulated(Pd, Sd, x, ed, BETA, WG)
        ref32, _ = O.manual_grads_emulated(Pd, Sd, x, ed, BETA, WG, dtype=torch.float32)
        _CACHE[key] = ({k: v.cpu() for k, v in exact.items()}, sums, {k: v.cpu().double() for k, v in ref32.items()})
    return _CACHE[key]


def _one_step(shape, prec, split=None, side_stream=None):
    """train_fwd_bwd + grad_norm + adam_step from zero moments; returns what the checks need."""
    from gm2 import native
    from gm2.data import ResidentMatrix
    G, H, L, B = shape
    P, S, X, eps = _state(shape)
    m = to_model(P, S, G, H, L, prec)
    mat = ResidentMatrix(X)
    ws = m.workspace(prec, B)
    if split is not None:
        ws.set_option(native.OPT_TRAIN_SPLIT, split)
    if side_stream is not None:
        ws.set_option(native.OPT_SIDE_STREAM, side_stream)
    before = {k: ws.stat(v) for k, v in native.TRAIN_STATS.items()}
    grads = torch.zeros_like(m.params)
    loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
    sc = scalars(beta=BETA, wgamma=WG, lam=LAM)
    native.train_fwd_bwd(ws, native.make_batch(mat.data, mat.ld, None, B, eps.cuda()), m.params, grads, m.bn, sc, loss)
    native.grad_norm(ws, m.params, grads, sc, loss)
    p0 = m.params.clone()
    mom, vel = torch.zeros_like(m.params), torch.zeros_like(m.params)
    native.adam_step(ws, m.params, grads, mom, vel, sc)
    ws.join()
    torch.cuda.synchronize()
    stats = {k: ws.stat(v) - before[k] for k, v in native.TRAIN_STATS.items()}
    return dict(m=m, grads=grads, loss=loss.cpu().numpy(), p0=p0, mom=mom, vel=vel, bn=m.bn.clone(), stats=stats)


def _check_step(shape, r, label):
    """The GM2_F32 bars of test_gpu_c2.py:26-31, 135-172 on one step's results."""
    G, H, L, B = shape
    P, S, X, eps = _state(shape)
    exact, sums, ref32 = _refs(shape)
    m, lt = r["m"], r["loss"]
    coef = np.float32(min(1.0, 1.0 / (lt[4] + 1e-6)))
    gg = (r["grads"] + LAM * torch.sign(r["p0"])) * float(coef)
    st = O.AdamState(lr=1e-3)
    Pf = {"p": r["p0"].clone()}
    O.adam_step(Pf, {"p": gg}, st)
    assert (m.params - Pf["p"]).abs().max().item() <= 2e-7
    assert (r["mom"] - st.m["p"]).abs().max().item() <= 1e-6 * st.m["p"].abs().max().item() + 1e-12
    assert (r["vel"] - st.v["p"]).abs().max().item() <= 1e-6 * st.v["p"].abs().max().item() + 1e-20
    print(f"{label} loss slots: libgm2 {lt[:3]}, fp64 oracle {sums}")
    assert abs(lt[0] - sums[0]) <= 1e-5 * abs(sums[0]), (lt[0], sums[0])
    assert abs(lt[1] - sums[1]) <= 1e-5 * abs(sums[1]), (lt[1], sums[1])
    assert abs(lt[2] - sums[2]) <= 1e-4 * abs(sums[2]) + 1e-2, (lt[2], sums[2])
    got = r["grads"].cpu().numpy()
    off = m.offsets
    fails = []
    for i, (name, _) in enumerate(m.specs):
        g = got[off[i]:off[i + 1]]
        ex = exact[name].reshape(-1).numpy()
        scale = float(np.abs(ex).max()) or 1.0
        if _prebn_bias(name):
            wscale = float(np.abs(exact[name.replace("bias", "weight")].numpy()).max())
            if np.abs(g).max() > 1e-3 * wscale:
                fails.append(f"{name}: |g| {np.abs(g).max():.3g} vs weight scale {wscale:.3g}")
            continue
        r32 = ref32[name].reshape(-1).numpy()
        nrm = float(np.linalg.norm(ex)) or 1.0
        f_gpu = float(np.linalg.norm(g - ex)) / nrm
        f_ref = float(np.linalg.norm(r32 - ex)) / nrm
        msg = (f"{name}: libgm2 {label} vs exact fro {f_gpu:.3g} (max-elem {float(np.abs(g - ex).max()) / scale:.3g}); "
               f"torch fp32 oracle fro {f_ref:.3g} (max-elem {float(np.abs(r32 - ex).max()) / scale:.3g})")
        print(msg)
        if not f_gpu <= 3 * f_ref + 2e-4:
            fails.append(msg)
    assert not fails, "\n".join(fails)
    norm = float(np.sqrt(sum(((exact[n].double() + LAM * torch.sign(P[n]).double()) ** 2).sum().item() for n in exact)))
    assert abs(lt[4] - norm) <= 1e-4 * norm, (lt[4], norm)
    l1 = sum(v.double().abs().sum().item() for v in P.values())
    assert abs(lt[3] - l1) <= 1e-6 * l1, (lt[3], l1)


# ------------------------------------------------------------------------------ 3. one step, split path
def _big_step():
    """The step at BIG under default options: run once, read by the tests below."""
    if "big_step" not in _CACHE:
        from gm2 import native
        _CACHE["big_step"] = _one_step(BIG, native.GM2_BF16X3)
    return _CACHE["big_step"]


def test_train_step_split_path():
    r = _big_step()
    assert r["stats"] == {"split_gemms": 5, "exact_gemms": 0}, r["stats"]
    assert "bf16x3" in repr(r["m"])
    _check_step(BIG, r, "bf16x3")


def test_train_step_side_stream_off_bit_identical():
    """GM2_OPT_SIDE_STREAM = 0 at BIG, where the bf16x3 dW9 wants 8 split-K slices of 8200 x 256
    floats and shrinks to the 7 its scratch holds: the same slice count in the same scratch as with
    the side stream, so gradients, loss slots, BatchNorm running statistics and the updated
    parameters are the side-stream run's bit for bit (itself held to the oracle above)."""
    from gm2 import native
    a = _big_step()
    b = _one_step(BIG, native.GM2_BF16X3, side_stream=0)
    assert b["stats"] == {"split_gemms": 5, "exact_gemms": 0}, b["stats"]
    assert torch.equal(a["grads"], b["grads"])
    assert np.array_equal(a["loss"], b["loss"])
    assert torch.equal(a["bn"], b["bn"])
    assert torch.equal(a["m"].params, b["m"].params)


# ------------------------------------------------------------------------------ 4. weights are re-split
def _oracle_bce_trajectory(shape, steps, lr):
    key = ("traj", shape, steps, lr)
    if key not in _CACHE:
        P, S, X, eps = _state(shape)
        dev = torch.device("cuda")
        Pd = {k: v.to(dev).clone() for k, v in P.items()}
        Sd = {k: v.to(dev) for k, v in S.items()}
        x, ed = torch.tensor(X, device=dev), eps.to(dev)
        st = O.AdamState(lr=lr)
        bce = []
        for _ in range(steps):
            g, sums = O.manual_grads_emulated(Pd, Sd, x, ed, BETA, 0.0, dtype=torch.float32)
            bce.append(sums[0])
            O.clip_grads(g, 1.0)
            O.adam_step(Pd, g, st)
        _CACHE[key] = np.array(bce)
    return _CACHE[key]


@pytest.mark.parametrize("defer", [1, 0])
def test_weights_resplit(defer):
    from gm2 import native
    from gm2.data import ResidentMatrix
    G, H, L, B = BIG
    P, S, X, eps = _state(BIG)
    ref = _oracle_bce_trajectory(BIG, 3, 1e-3)
    mat = ResidentMatrix(X)
    ed = eps.cuda()

    def run_step(m, ws, mom, vel, step):
        grads = torch.zeros_like(m.params)
        loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
        sc = scalars(beta=BETA, step=step, lr=1e-3)
        native.train_fwd_bwd(ws, native.make_batch(mat.data, mat.ld, None, B, ed), m.params, grads, m.bn, sc, loss)
        native.grad_norm(ws, m.params, grads, sc, loss)
        native.adam_step(ws, m.params, grads, mom, vel, sc)
        return grads, loss

    m = to_model(P, S, G, H, L, native.GM2_BF16X3)
    ws = m.workspace(native.GM2_BF16X3, B)
    ws.set_option(native.OPT_DEFER_OUTPUT_ADAM, defer)
    mom, vel = torch.zeros_like(m.params), torch.zeros_like(m.params)
    bce = []
    for k in range(3):
        _, loss = run_step(m, ws, mom, vel, k + 1)
        bce.append(loss)
    ws.join()
    torch.cuda.synchronize()
    bce = np.array([float(v[0]) for v in bce])
    print(f"defer {defer}: BCE libgm2 bf16x3 {bce}, fp32 oracle {ref}, rel {np.abs(bce - ref) / ref}")
    assert (np.abs(bce - ref) <= 1e-4 * ref).all()
    assert ws.stat(native.TSTAT_SPLIT_GEMMS) == 15 and ws.stat(native.TSTAT_EXACT_GEMMS) == 0
    # a second init over params + sync_shadows: the next step is a freshly built model's, bit for bit
    torch.manual_seed(777)
    P2 = O.init_params(G, H, L)
    with torch.no_grad():
        for k, v in m.param_views().items():
            v.copy_(P2[k].cuda())
        m.bn.copy_(torch.stack([torch.stack([S[b + ".running_mean"], S[b + ".running_var"]]) for b in O.BNS]).cuda())
    native.sync_shadows(ws, m.params)
    mom.zero_()
    vel.zero_()
    g_a, l_a = run_step(m, ws, mom, vel, 1)
    ws.join()
    m2 = to_model(P2, S, G, H, L, native.GM2_BF16X3)
    ws2 = m2.workspace(native.GM2_BF16X3, B)
    ws2.set_option(native.OPT_DEFER_OUTPUT_ADAM, defer)
    g_b, l_b = run_step(m2, ws2, torch.zeros_like(m2.params), torch.zeros_like(m2.params), 1)
    ws2.join()
    torch.cuda.synchronize()
    assert torch.equal(g_a, g_b)
    assert torch.equal(l_a, l_b)
    assert torch.equal(m.params, m2.params) and torch.equal(m.bn, m2.bn)


# ------------------------------------------------------------------------------ 5. the option off is GM2_F32
@pytest.mark.parametrize("shape", [SMALL, BIG], ids=["small", "big"])
def test_split_off_is_f32(shape):
    from gm2 import native
    a = _one_step(shape, native.GM2_BF16X3, split=0)
    b = _one_step(shape, native.GM2_F32)
    assert a["stats"] == {"split_gemms": 0, "exact_gemms": 5}, a["stats"]
    assert b["stats"] == {"split_gemms": 0, "exact_gemms": 0}, b["stats"]  # (a GM2_F32 workspace counts nothing)
    assert torch.equal(a["grads"], b["grads"])
    assert np.array_equal(a["loss"], b["loss"])
    assert torch.equal(a["bn"], b["bn"])
    assert torch.equal(a["m"].params, b["m"].params)


def test_small_shape_split_on():
    from gm2 import native
    r = _one_step(SMALL, native.GM2_BF16X3, split=1)
    assert r["stats"]["split_gemms"] + r["stats"]["exact_gemms"] == 5, r["stats"]
    print(f"small shape: {r['stats']}")
    _check_step(SMALL, r, "bf16x3")


# ------------------------------------------------------------------------------ 6. eval_forward
def test_eval_forward():
    from gm2 import native
    from gm2.data import ResidentMatrix
    G, H, L, B = BIG
    P, S, X, eps = _state(BIG)
    m = to_model(P, S, G, H, L, native.GM2_BF16X3)
    mat = ResidentMatrix(X)
    ws = m.workspace(native.GM2_BF16X3, B)
    loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
    sc = scalars(beta=BETA, wgamma=WG, lam=LAM)
    native.eval_forward(ws, native.make_batch(mat.data, mat.ld, None, B, eps.cuda()), m.params, m.bn, sc, loss)
    torch.cuda.synchronize()
    assert ws.stat(native.TSTAT_SPLIT_GEMMS) == 2 and ws.stat(native.TSTAT_EXACT_GEMMS) == 0
    dev = torch.device("cuda")
    Pd = {k: v.to(dev).double() for k, v in P.items()}
    Sd = {k: v.to(dev).double() for k, v in S.items()}
    x = torch.tensor(X, device=dev).double()
    p, mu, lv = O.forward(Pd, Sd, x, eps.to(dev).double(), train=False)
    bce = -(x * torch.clamp(torch.log(p), min=-100) + (1 - x) * torch.clamp(torch.log1p(-p), min=-100)).sum().item()
    sums = [bce, p.sum().item(), torch.sum(1 + lv - mu.pow(2) - lv.exp()).item()]
    lt = loss.cpu().numpy()
    print(f"eval loss slots: libgm2 bf16x3 {lt[:3]}, fp64 oracle {sums}")
    assert abs(lt[0] - sums[0]) <= 1e-5 * abs(sums[0]), (lt[0], sums[0])
    assert abs(lt[1] - sums[1]) <= 1e-5 * abs(sums[1]), (lt[1], sums[1])
    assert abs(lt[2] - sums[2]) <= 1e-4 * abs(sums[2]) + 1e-2, (lt[2], sums[2])
