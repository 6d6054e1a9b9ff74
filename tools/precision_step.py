#!/usr/bin/env python3
"""C2 step time of the three training precisions: f32, bf16x3, bf16.

The v0 step of bench.py (G = 55,039, H = 1024, L = 64, B = 4096 rows of a resident 10,000-row
synthetic matrix; forward, fused loss, backward, clip statistics, Adam with the deferred
output-layer update) timed the way bench.py times it: warm-up, then K steps with ws.join() and a
device synchronise inside the timed window. The three precisions alternate within one process and
the round is repeated, so the run-to-run spread is visible next to the differences. Per precision
it also reports the live-timed kernel classes (gm2_timing_*): the output-layer loss GEMM, every
other GEMM launch, the Adam passes; and how many of the G-wide GEMMs ran split (GM2_TSTAT_*).

    python tools/precision_step.py [--steps 20] [--warmup 5] [--repeats 3] [--out FILE]

Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "genome-minimizer-2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--genes", type=int, default=55039)
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--latent", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--strains", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.steps < 20 or a.repeats < 3:
        print("note: fewer than 20 steps or 3 repeats: the spread is not meaningful", file=sys.stderr)

    from gm2 import native
    from gm2.data import ResidentMatrix, synthetic_pangenome
    from gm2.model import VAE
    from gm2.trainer import Adam

    dev = torch.device("cuda", 0)
    G, H, L, B = a.genes, a.hidden, a.latent, a.batch
    mat = ResidentMatrix(synthetic_pangenome(a.strains, G, seed=1000), device=dev)
    modes = [("f32", native.GM2_F32), ("bf16x3", native.GM2_BF16X3), ("bf16", native.GM2_BF16)]
    nsteps = a.warmup + a.steps
    gen = torch.Generator().manual_seed(100)
    rows = torch.cat([torch.randperm(a.strains, generator=gen)[:B] for _ in range(nsteps)]).to(torch.int32).to(dev)
    classes = native.KC_RECON_LOSS | native.KC_GEMM_STORE | native.KC_ADAM
    runs = {name: [] for name, _ in modes}
    torch.manual_seed(0)
    p0 = VAE(G, H, L, device=dev, precision=native.GM2_F32).params.clone()

    def one(name, prec):
        # the same initial parameters for every run (the reference initialisation, drawn once)
        model = VAE(G, H, L, device=dev, precision=prec, init=False)
        model.params.copy_(p0)
        model.touch()
        opt = Adam(model, lr=1e-3)
        ws = model.workspace(prec, B)
        ws.set_option(native.OPT_DEFER_OUTPUT_ADAM, 1)
        ws.set_option(native.OPT_GRAD_BUCKETS, 0)
        res = mat.operands(prec) if prec == native.GM2_BF16 else None  # (resident operands: bf16 mode only)
        grads = torch.zeros_like(model.params)
        tab = np.zeros((nsteps, native.NUM_SCALARS))
        for i in range(nsteps):
            t = i + 1
            tab[i, native.S_BETA] = 0.1
            tab[i, native.S_NEG_STEP] = -(1e-3 / (1 - 0.9 ** t))
            tab[i, native.S_BC2_SQRT] = np.sqrt(1 - 0.999 ** t)
            tab[i, native.S_MAX_NORM] = 1.0
            tab[i, native.S_ONE_MINUS_B1], tab[i, native.S_BETA2] = 0.1, 0.999
            tab[i, native.S_ONE_MINUS_B2], tab[i, native.S_ADAM_EPS] = 0.001, 1e-8
            tab[i, native.S_NORM_AHEAD] = 1.0
        scal = torch.tensor(tab, dtype=torch.float32, device=dev)
        loss = torch.zeros(nsteps, native.LOSS_SLOTS, dtype=torch.float64, device=dev)
        torch.cuda.manual_seed(1)

        def step(i):
            eps = torch.randn(B, L, device=dev)
            batch = native.make_batch(mat.data, mat.ld, rows[i * B:(i + 1) * B], B, eps, resident=res)
            native.train_fwd_bwd(ws, batch, model.params, grads, model.bn, scal[i], loss[i])
            native.grad_norm(ws, model.params, grads, scal[i], loss[i])
            native.adam_step(ws, model.params, grads, opt.exp_avg, opt.exp_avg_sq, scal[i])

        torch.cuda.synchronize()
        for i in range(a.warmup):
            step(i)
        ws.join()
        torch.cuda.synchronize()
        # pass 1: wall time, nothing else in the window
        t0 = time.perf_counter()
        for i in range(a.warmup, nsteps):
            step(i)
        ws.join()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / a.steps
        losses = loss.cpu().numpy()
        if not np.isfinite(losses[:, [0, 1, 2, 4]]).all():
            raise RuntimeError(f"{name}: non-finite loss or gradient norm")
        # pass 2: the same steps again with the kernel classes bracketed by events (not part of `ms`)
        native.timing_begin(classes)
        for i in range(a.warmup, nsteps):
            step(i)
        ws.join()
        torch.cuda.synchronize()
        native.timing_end()
        kc = {k: native.timing_class(v)[0] / a.steps for k, v in
              (("recon_loss_ms", native.KC_RECON_LOSS), ("gemm_store_ms", native.KC_GEMM_STORE),
               ("adam_ms", native.KC_ADAM))}
        stats = {k: ws.stat(v) for k, v in native.TRAIN_STATS.items()}
        del model, opt, ws, grads
        torch.cuda.empty_cache()
        return dict(step_ms=ms, bce_last=float(losses[-1, 0]), **kc, **stats)

    for rep in range(a.repeats):
        for name, prec in modes:
            r = one(name, prec)
            runs[name].append(r)
            print(f"repeat {rep} {name:7s} {r['step_ms']:8.3f} ms/step  (loss GEMM {r['recon_loss_ms']:.3f}, other GEMMs "
                  f"{r['gemm_store_ms']:.3f}, Adam {r['adam_ms']:.3f} ms/step; split {r['split_gemms']}, exact "
                  f"{r['exact_gemms']})", file=sys.stderr)
    out = {"shape": dict(G=G, H=H, L=L, B=B, strains=a.strains), "steps": a.steps, "warmup": a.warmup,
           "repeats": a.repeats, "modes": {}}
    for name, _ in modes:
        t = [r["step_ms"] for r in runs[name]]
        out["modes"][name] = {"step_ms": t, "median_ms": float(np.median(t)), "spread_ms": float(max(t) - min(t)),
                              "kernel_classes_ms": {k: float(np.median([r[k] for r in runs[name]]))
                                                    for k in ("recon_loss_ms", "gemm_store_ms", "adam_ms")},
                              "split_gemms_per_step": runs[name][-1]["split_gemms"] / (2 * a.steps + a.warmup),
                              "bce_last": runs[name][-1]["bce_last"]}
    f32, x3 = out["modes"]["f32"], out["modes"]["bf16x3"]
    out["f32_over_bf16x3"] = f32["median_ms"] / x3["median_ms"]
    out["bf16x3_faster_by_more_than_spread"] = bool(min(f32["step_ms"]) - max(x3["step_ms"]) >
                                                    max(f32["spread_ms"], x3["spread_ms"]))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
