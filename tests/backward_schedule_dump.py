"""Two training steps (train_fwd_bwd + grad_norm + adam_step, then ws.join()) at the shapes of
tests/test_gpu_backward_schedule.py, returned as named CPU tensors: per step the gradients and
loss[:3], at the end the BatchNorm running statistics and the parameters.

Imported by the test for the in-process schedule variants. Run as a script in a child process (the
schedule's environment knobs GM2_FORK_HOLD / GM2_DW9_AT / GM2_TAIL_MAIN are read once per process,
and GM2_LIB_PATH selects another build of the library) it runs every shape, or the shapes named,
and writes the tensors with torch.save:
    python tests/backward_schedule_dump.py OUT.pt [--c2] [--side 0|1] [TAG ...]
--c2 adds the bench's C2 step shape in bf16, f32 and bf16x3 (a same-results check of two builds);
--side is GM2_OPT_SIDE_STREAM (default 1), every other option at its default."""
import argparse
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "genome-minimizer-2_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from gpu_helpers import oracle_state, perturb_bn, scalars, synth_x, to_model  # noqa: E402

# tag: (precision, G, H, L, B). What each takes in the backward chain (plan_gemm_dims, K-tile 32
# elements in f32 and 64 in bf16; checked on the host against the plan rules):
#   f32a   dA5 2 split-K slices; hidden dX one pass (BatchNorm partials in its epilogue); dW9 one
#          pass (transposed direct form, clip statistics ahead)
#   f32b   hidden dX 2 slices (partial kernel summing into DA), dA5 4 slices; dW9 and the hidden weight
#          gradients 2 slices (slabs + k_slab_sum)
#   bf16a  hidden dX and dA5 2 slices; dY0 written transposed by the BatchNorm apply; dW9 one pass
#   bf16b  everything one pass; ragged batch (Bp = 384)
# The c shapes (Bp = 4096: 128 K-tiles in f32, 64 in bf16, nk / 8 caps the slices) are the smallest at
# which every precision splits dW9, the one side GEMM that can start while a dX result is unread:
#   f32c   dA5 2 slices; every other dX one pass (partials in the epilogue); dW9 (133,120-float slabs),
#          the hidden, latent and head weight gradients and dWe0 16 slices each
#   bf16c  every dX one pass; dW9, the hidden, latent and head weight gradients and dWe0 8 slices each
#   x3c    the chain and the hidden weight gradients as f32c (dA5 stays exact fp32: its bf16x3 shape is
#          no 256-tile plan); dW9 and dWe0 as bf16x3 products on 256-tiles (2 Bq = 8192 K-rows), 16
#          slices each: 2.1 M floats of slabs, the hidden dX result beside them 4096 x 256 = 1.0 M
SHAPES = {
    "f32a": ("f32", 517, 256, 16, 100),
    "f32b": ("f32", 1100, 512, 32, 500),
    "bf16a": ("bf16", 1100, 1024, 32, 100),
    "bf16b": ("bf16", 517, 256, 16, 300),
    "f32c": ("f32", 520, 256, 32, 4000),
    "bf16c": ("bf16", 520, 256, 32, 4000),
    "x3c": ("bf16x3", 520, 256, 32, 4000),
}
C2 = {p + "_c2": (p, 55039, 1024, 64, 4096) for p in ("bf16", "f32", "bf16x3")}
STEPS = 2


def inputs(tag):
    """The shape's model state, strain matrix and per-step rows / eps (deterministic, on the CPU)."""
    return _inputs(*{**SHAPES, **C2}[tag][1:])


@functools.lru_cache(maxsize=1)
def _inputs(G, H, L, B):
    S = 2 * B + 5 if B < 1024 else B + 5
    P, Sb = perturb_bn(*oracle_state(G, H, L, G + B), seed=91)
    gen = torch.Generator().manual_seed(92)
    rows = [torch.randperm(S, generator=gen)[:B].to(torch.int32) for _ in range(STEPS)]
    eps = [torch.randn(B, L, generator=gen) for _ in range(STEPS)]
    return dict(P=P, S=Sb, X=synth_x(S, G, 93), rows=rows, eps=eps)


def run(tag, inp, side=1, buckets=1, with_next=False):
    from gm2 import native
    from gm2.data import ResidentMatrix
    pname, G, H, L, B = {**SHAPES, **C2}[tag]
    prec = {"f32": native.GM2_F32, "bf16": native.GM2_BF16, "bf16x3": native.GM2_BF16X3}[pname]
    m = to_model(inp["P"], inp["S"], G, H, L, prec)
    mat = ResidentMatrix(inp["X"])
    ws = m.workspace(prec, B)
    ws.set_option(native.OPT_SIDE_STREAM, side)
    ws.set_option(native.OPT_GRAD_BUCKETS, buckets)
    grads = torch.zeros_like(m.params)
    mom, vel = torch.zeros_like(m.params), torch.zeros_like(m.params)
    rows = [r.cuda() for r in inp["rows"]]
    eps = [e.cuda() for e in inp["eps"]]
    batches = [None] * STEPS
    for i in reversed(range(STEPS)):  # (step i's batch names step i + 1's as its `next`)
        nxt = batches[i + 1] if with_next and i + 1 < STEPS else None
        batches[i] = native.make_batch(mat.data, mat.ld, rows[i], B, eps[i], next=nxt)
    waiter = torch.cuda.Stream()
    out = {}
    for i in range(STEPS):
        sc = scalars(beta=0.37, wgamma=0.55, lam=0.01, step=i + 1)
        sc[native.S_NORM_AHEAD] = 1.0
        loss = torch.zeros(native.LOSS_SLOTS, dtype=torch.float64, device="cuda")
        split0 = ws.stat(native.TRAIN_STATS["split_gemms"])
        native.train_fwd_bwd(ws, batches[i], m.params, grads, m.bn, sc, loss)
        if pname == "bf16x3":  # (at least dW9 and dWe0 as split products: not the exact-fp32 fallback)
            split = ws.stat(native.TRAIN_STATS["split_gemms"]) - split0
            print(f"{tag} side={side} step {i}: {split} split-bf16 GEMMs")
            assert split >= 2, (tag, i, split)
        if buckets:  # every bucket's event can be waited on
            for b in range(native.GRAD_BUCKETS):
                native.wait_grad_bucket(ws, b, waiter)
        native.grad_norm(ws, m.params, grads, sc, loss)
        out[f"{tag}.grads{i}"] = grads.clone()
        out[f"{tag}.loss{i}"] = loss[:3].clone()
        native.adam_step(ws, m.params, grads, mom, vel, sc)
    ws.join()
    torch.cuda.synchronize()
    out[f"{tag}.bn"] = m.bn.clone()
    out[f"{tag}.params"] = m.params.clone()
    return {k: v.cpu() for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("tags", nargs="*", help="shapes to run (default: every entry of SHAPES)")
    ap.add_argument("--c2", action="store_true")
    ap.add_argument("--side", type=int, choices=(0, 1), default=1)
    a = ap.parse_args()
    tags = (a.tags or list(SHAPES)) + (list(C2) if a.c2 else [])
    out = {}
    for tag in tags:
        out.update(run(tag, inputs(tag), side=a.side))
    torch.save(out, a.out)
    print(f"BWDDUMP {len(out)} tensors -> {a.out}")


if __name__ == "__main__":
    main()
