"""The backward schedule of csrc/api.hip only decides on which stream, and behind which event, each
launch of the backward goes: the side stream (GM2_OPT_SIDE_STREAM), the gradient-bucket events
(GM2_OPT_GRAD_BUCKETS), the next batch's staged gather (gm2_batch.next) and the environment knobs
GM2_FORK_HOLD / GM2_DW9_AT / GM2_TAIL_MAIN reorder launches across streams and change no operand:
with the side stream off the side work keeps its own split-K scratch and capacity, and every
split-K sum is taken in slice order. So two training steps (train_fwd_bwd + grad_norm + adam_step,
then ws.join()) give the same gradients, loss[:3], BatchNorm running statistics and updated
parameters bit for bit (torch.equal) under every variant, at seven small shapes that between them
take every branch of the chain and split the output-layer weight gradient dW9 in each training
precision (tests/backward_schedule_dump.py SHAPES). No shape or variant is left out.

  * The default run the variants must equal is itself held to the oracle, at every shape: step 0's
    gradients and loss sums against the fp64 oracle, under the per-tensor bar of
    test_gpu_parity.py::test_train_step_vs_oracle. "Equal to the default run" so means "right".
  * In this process: side stream {1, 0} x gradient buckets {1, 0} x gm2_batch.next {absent, present}
    (GM2_DW9_AT at its default 2: dW9 behind the first hidden dX GEMM, that result unread).
  * The environment knobs are read once per process, so those variants run the dump script in a
    child process, one at a time: the knobs with the side stream on, and the side stream off with
    dW9 behind dA5 (0, its slabs unread), behind the dX GEMM out of the latent heads (6, unread
    as well) and past the chain's end (99).
  * gm2_backward_outputs with and without the side stream, where dW9 is one pass and where it splits."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import backward_schedule_dump as D
from gpu_helpers import grad_bar_failures, to_model
from oracle import vae_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gm2 import native
    from gm2.data import ResidentMatrix

KNOBS = ("GM2_FORK_HOLD", "GM2_DW9_AT", "GM2_TAIL_MAIN")
DUMP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "backward_schedule_dump.py")
BETA, WGAMMA = 0.37, 0.55  # (the scalars of D.run; its lambda 0.01 enters at the clip / Adam passes only)


@functools.lru_cache(maxsize=None)
def _default(tag):
    """The shape's two steps under the default schedule, in this process: computed once, shared."""
    return D.run(tag, D.inputs(tag))


def _assert_same(ref, got, what):
    assert sorted(ref) == sorted(got), what
    for k in sorted(ref):
        assert torch.equal(ref[k], got[k]), f"{what}: {k} differs"


def _child(args, knobs, tmp_path):
    """The dump script in a fresh interpreter with `knobs` in its environment; the tensors it wrote."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(knobs)
    out = str(tmp_path / "dump.pt")
    r = subprocess.run([sys.executable, "-u", DUMP, out] + args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    print(r.stdout[-2000:])
    return torch.load(out, weights_only=True)


def _default_all():
    ref = {}
    for tag in D.SHAPES:
        ref.update(_default(tag))
    return ref


# ------------------------------------------------------------------------------ the default run is right
@functools.lru_cache(maxsize=None)
def _oracle(dims, rounded):
    """Step 0's gradients and loss sums from the oracle's explicit chain on the device: in fp64 (the
    exact reference; rounded None), or in fp32 with the bf16 path's operand rounding or without (the
    reference arithmetic). One evaluation per (G, H, L, B) and arithmetic, shared by the precisions."""
    inp = D._inputs(*dims)
    dev = torch.device("cuda")
    Pd = {k: v.to(dev) for k, v in inp["P"].items()}
    Sd = {k: v.to(dev) for k, v in inp["S"].items()}
    x = torch.tensor(inp["X"][inp["rows"][0].numpy()], dtype=torch.float32, device=dev)
    eps = inp["eps"][0].to(dev)
    if rounded is None:
        g, sums = O.manual_grads_emulated(Pd, Sd, x, eps, BETA, WGAMMA)
    else:
        g, sums = O.manual_grads_emulated(Pd, Sd, x, eps, BETA, WGAMMA, operand_round=O.bf16_round if rounded else None,
                                          dtype=torch.float32)
    return {k: v.cpu() for k, v in g.items()}, [float(s) for s in sums]


@pytest.mark.parametrize("tag", list(D.SHAPES))
def test_default_schedule_matches_oracle(tag):
    """Step 0 of the default run against the oracle, by the bar of test_train_step_vs_oracle: per
    tensor fro(libgm2) <= 3 fro(reference arithmetic) + floor against the fp64 gradients, the
    reference arithmetic the same math in fp32 (bf16: with the operand rounding), floor 2e-4 (f32,
    bf16x3) / 1e-3 (bf16); pre-BatchNorm biases absolutely; loss[:2] rel 1e-5 (bf16: 1e-4, against
    the sums of the rounded arithmetic)."""
    pname, G, H, L, B = D.SHAPES[tag]
    got = _default(tag)
    exact, sums = _oracle((G, H, L, B), None)
    ref, sums_r = _oracle((G, H, L, B), pname == "bf16")
    if pname == "bf16":
        sums = sums_r
    lt = got[f"{tag}.loss0"].numpy()
    rtol = 1e-4 if pname == "bf16" else 1e-5
    print(f"{tag} loss[:2]: libgm2 {lt[:2]}, oracle {sums[:2]}")
    for k in range(2):
        assert abs(lt[k] - sums[k]) <= rtol * abs(sums[k]), (k, lt[k], sums[k])
    inp = D.inputs(tag)
    m = to_model(inp["P"], inp["S"], G, H, L, native.GM2_F32)  # (the flat buffer's tensor table)
    fails = grad_bar_failures(m.specs, m.offsets, got[f"{tag}.grads0"], exact, ref,
                              floor=1e-3 if pname == "bf16" else 2e-4, bias_tol=2e-2 if pname == "bf16" else 1e-3,
                              label=f"{tag} {pname}")
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------ the variants equal it
@pytest.mark.parametrize("tag", list(D.SHAPES))
def test_schedule_options_bit_identical(tag):
    """Side stream {1, 0} x gradient buckets {1, 0} x gm2_batch.next {absent, present}; with the
    buckets on, every bucket is waited on after each step."""
    ref = _default(tag)
    inp = D.inputs(tag)
    for side in (1, 0):
        for buckets in (1, 0):
            for with_next in (False, True):
                if (side, buckets, with_next) == (1, 1, False):
                    continue  # (the reference itself)
                got = D.run(tag, inp, side=side, buckets=buckets, with_next=with_next)
                _assert_same(ref, got, f"{tag} side={side} buckets={buckets} next={with_next}")


@pytest.mark.parametrize("knobs", [dict(GM2_FORK_HOLD="6", GM2_DW9_AT="0", GM2_TAIL_MAIN="1"),
                                   dict(GM2_FORK_HOLD="1", GM2_DW9_AT="99")],
                         ids=["every_layer_forks_dw9_first_tail_main", "one_fork_dw9_last"])
def test_schedule_env_knobs_bit_identical(knobs, tmp_path):
    """The environment knobs, in a fresh interpreter each: every layer forks, dW9 right behind dA5
    and the forward's tail on the caller's stream; and one fork for all side work with dW9 at the
    fallback beside dWe0. All shapes at default options against this process's default."""
    _assert_same(_default_all(), _child([], knobs, tmp_path), f"child with {knobs}")


@pytest.mark.parametrize("at", [0, 6, 99], ids=["behind_da5", "behind_latent_dx", "past_the_chain"])
def test_side_stream_off_dw9_position_bit_identical(at, tmp_path):
    """GM2_OPT_SIDE_STREAM = 0 with dW9 elsewhere than at the default position, in a fresh interpreter
    each: behind dA5 (whose split-K slabs the first BatchNorm backward has yet to read), behind the
    dX GEMM out of the latent heads (read by layer 2's BatchNorm backward after it), and past the
    chain's end beside dWe0. All shapes against this process's default (side stream on, dW9 at 2)."""
    knobs = dict(GM2_DW9_AT=str(at))
    _assert_same(_default_all(), _child(["--side", "0"], knobs, tmp_path), f"child with side stream off, {knobs}")


def test_backward_outputs_side_stream_bit_identical():
    """gm2_backward_outputs (gradients of probs / mu / logvar from outside the fused loss), train 0
    and 1: the same gradient buffer with and without the side stream, at f32a (dW9 in one pass) and
    f32b (dW9 in split-K slabs)."""
    for tag in ("f32a", "f32b"):
        for train in (0, 1):
            _backward_outputs_both_ways(tag, train)


def _backward_outputs_both_ways(tag, train):
    _, G, H, L, B = D.SHAPES[tag]
    inp = D.inputs(tag)
    gen = torch.Generator().manual_seed(5)
    dprobs = torch.randn(B, G, generator=gen).cuda()
    dmu, dlv = torch.randn(B, L, generator=gen).cuda(), torch.randn(B, L, generator=gen).cuda()
    rows, eps = inp["rows"][0].cuda(), inp["eps"][0].cuda()
    outs = []
    for side in (1, 0):
        m = to_model(inp["P"], inp["S"], G, H, L, native.GM2_F32)
        mat = ResidentMatrix(inp["X"])
        ws = m.workspace(native.GM2_F32, B)
        ws.set_option(native.OPT_SIDE_STREAM, side)
        probs = torch.zeros(B, G, device="cuda")
        grads = torch.full_like(m.params, float("nan"))
        batch = native.make_batch(mat.data, mat.ld, rows, B, eps)
        native.forward(ws, batch, m.params, m.bn, train, probs, G)
        native.backward_outputs(ws, batch, m.params, train, probs, G, dprobs, dmu, dlv, grads)
        torch.cuda.synchronize()
        outs.append(grads.cpu())
    assert torch.isfinite(outs[0]).all(), (tag, train)
    assert torch.equal(outs[0], outs[1]), f"{tag} train={train}"
