#!/usr/bin/env python3
"""Times the bit transpose of packed masks and the gene x gene counts built on it (no pass / fail: a record).

Synthetic packed rows with the SURVEY.md §8 gene frequencies (tools/genefreq_bench.py synthetic_packed),
made on the device from a seed, at two shapes: the real matrix (default 7,512 x 55,039) and the sampled
set (1e6 x 55,039, 6.9 GB). Per shape:
  * transpose   gm2_mask_transpose into a preallocated gene-major buffer
  * copy        torch.Tensor.copy_ of a flat buffer of (bytes read + bytes written) / 2 bytes: the same
                traffic with no work in between, measured in the same run -- the yardstick
  * gather      index_select of the panel's rows of the transposed set
  * counts      gm2_mask_cooccur of the gathered rows (K x K over n bits)
  * torch       the route without the kernel: the panel's bits unpacked from the strain-major rows in row
                chunks, then a float32 matmul per chunk (exact: every count < 2^24)
The panel is gm2.linkage.select_panel of the set's own counts (K = --panel genes). Each leg: warmed, then
`--reps` calls, each between its own pair of device events; the median. The transposed rows and the
counts are spot-checked against numpy, and the two routes' counts compared exactly.
Prints one JSON line and writes it to profiles/transpose_times.json.

  python tools/transpose_bench.py [--samples 1000000 --strains 7512 --genes 55039 --panel 2048 --reps 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome-minimizer-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_TBS = 6.29   # MI355X_MICROARCH.md: the float4 device copy, read + written bytes per second / 1e12


def torch_panel_counts(p, panel, torch, rows=65536):
    """X[:, panel]^T X[:, panel] by unpacking the panel's bits with torch -> device int32 [K, K]."""
    byte, shift = (panel >> 3), (panel & 7).to(torch.uint8)
    acc = torch.zeros(len(panel), len(panel), dtype=torch.float32, device="cuda")
    for r0 in range(0, p.n, rows):
        x = ((p.bits[r0:r0 + rows].index_select(1, byte) >> shift) & 1).to(torch.float32)
        acc += x.T @ x
    return acc.to(torch.int32)


def measure(name, n, G, a, torch, np):
    from genefreq_bench import median_ms, synthetic_packed
    from gm2 import linkage, native
    from gm2.masks import PackedMasks
    p = synthetic_packed(n, G, 4242, torch, np)
    kb, ob = native.packed_row_bytes(G), native.packed_row_bytes(n)
    res = {"rows": n, "genes": G, "bytes_read": n * kb, "bytes_written": G * ob}
    moved = res["bytes_read"] + res["bytes_written"]
    out = torch.zeros(G, ob, dtype=torch.uint8, device="cuda")
    ms, lo, hi = median_ms(lambda: native.mask_transpose(p.bits, n, p.ld, G, out, ob), a.reps, torch)
    res.update(transpose_ms=ms, transpose_ms_min=lo, transpose_ms_max=hi, transpose_tb_per_s=moved / (ms * 1e-3) / 1e12)
    src = torch.empty(moved // 2 // 16 * 16, dtype=torch.uint8, device="cuda").random_()
    dst = torch.empty_like(src)
    ms, lo, hi = median_ms(lambda: dst.copy_(src), a.reps, torch)
    res.update(copy_bytes_each_way=src.numel(), copy_ms=ms, copy_ms_min=lo, copy_ms_max=hi,
               copy_tb_per_s=2 * src.numel() / (ms * 1e-3) / 1e12)
    res["transpose_fraction_of_copy"] = res["transpose_tb_per_s"] / res["copy_tb_per_s"]
    res["copy_fraction_of_guide_copy"] = res["copy_tb_per_s"] / COPY_TBS
    del src, dst
    t = PackedMasks(out, n)
    # spot check: the first, a middle and the last gene rows against numpy on the host
    for g in (0, G // 2, G - 1):
        col = ((p.bits[:, g >> 3] >> (g & 7)) & 1).cpu().numpy()
        want = np.zeros(ob, dtype=np.uint8)
        want[:(n + 7) // 8] = np.packbits(col, bitorder="little")
        res.setdefault("transpose_rows_equal_numpy", True)
        res["transpose_rows_equal_numpy"] &= bool((out[g].cpu().numpy() == want).all())
    panel = linkage.select_panel(p.gene_counts().cpu().numpy(), n, k=a.panel)
    idx = torch.from_numpy(panel).cuda()
    res["panel_genes"] = K = len(panel)
    ms, lo, hi = median_ms(lambda: out.index_select(0, idx), a.reps, torch)
    res.update(gather_ms=ms, gather_ms_min=lo, gather_ms_max=hi)
    sel = PackedMasks(out.index_select(0, idx), n)
    ms, lo, hi = median_ms(lambda: sel.cooccurrence(), a.reps, torch)
    res.update(counts_ms=ms, counts_ms_min=lo, counts_ms_max=hi,
               counts_tera_bit_pairs_per_s=K * K * n / (ms * 1e-3) / 1e12)
    res["gene_cooccurrence_ms"] = res["transpose_ms"] + res["gather_ms"] + res["counts_ms"]
    ms, lo, hi = median_ms(lambda: p.gene_cooccurrence(panel, transposed=t), a.reps, torch)
    res.update(gene_cooccurrence_given_transposed_ms=ms)
    counts = p.gene_cooccurrence(panel, transposed=t)
    ms, lo, hi = median_ms(lambda: torch_panel_counts(p, idx, torch), a.torch_reps, torch)
    res.update(torch_ms=ms, torch_reps=a.torch_reps, torch_over_kernel_route=ms / res["gene_cooccurrence_ms"])
    res["equals_torch"] = bool(torch.equal(torch_panel_counts(p, idx, torch), counts))
    # spot check: an 8 x 8 corner of the counts against numpy on the host
    sub = panel[:8]
    x = np.stack([((p.bits[:, int(g) >> 3] >> (int(g) & 7)) & 1).cpu().numpy() for g in sub], axis=1).astype(np.int64)
    res["counts_corner_equals_numpy"] = bool((counts[:len(sub), :len(sub)].cpu().numpy() == x.T @ x).all())
    return name, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--strains", type=int, default=7512)
    ap.add_argument("--genes", type=int, default=55039)
    ap.add_argument("--panel", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transpose_times.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("transpose_bench: needs the GPU (a host run measures nothing)")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "guide_copy_tb_per_s": COPY_TBS}
    for name, n in (("real", a.strains), ("sampled", a.samples)):
        key, r = measure(name, n, a.genes, a, torch, np)
        res[key] = r
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
