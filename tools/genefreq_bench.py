#!/usr/bin/env python3
"""Times the per-gene counts of packed masks on the GPU (no pass / fail: a record).

Synthetic packed rows with the SURVEY.md §8 gene frequencies (15 % core genes at 0.98, accessory genes
Beta(0.1, 1)), made on the device from a seed, at two shapes: the sampled set (default 1e6 x 55,039,
6.9 GB) and the real matrix (10,000 x 55,039). Per shape:
  * all rows      gm2_mask_gene_counts over every row, in order
  * half, gathered  the same through an index list of a random half of the rows (whole-row gathers)
  * torch         the route without the kernel: chunked bit unpack + sum(0) on the device over the same
                  packed rows (fewer repetitions: it is slow)
Each kernel leg: warmed, then `--reps` calls, each between its own pair of device events; the median
and the bytes the call must read (rows x roundup(G, 128) / 8) over it, beside MI355X_MICROARCH's
achievable in-order HBM read rate. The counts of the three routes are compared exactly.
Prints one JSON line and writes it to profiles/genefreq_times.json.

  python tools/genefreq_bench.py [--samples 1000000 --strains 10000 --genes 55039 --reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome-minimizer-2_amd"))

HBM_READ_TBS = 6.0        # in-order read, the lower end of the measured 6.0-6.3 TB/s
HBM_GATHER_TBS = 5.5      # whole-row gathers, the lower end of 5.5-5.8 TB/s


def median_ms(fn, reps, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return t[len(t) // 2], t[0], t[-1]


def burst_ms(fn, reps, torch):
    """Mean milliseconds of `reps` back-to-back calls between one pair of events (for calls too short
    for an event pair of their own)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def synthetic_packed(n, G, seed, torch, np):
    """PackedMasks [n, G]: X[s, g] ~ Bernoulli(f_g) on the device, f as gm2.data.synthetic_pangenome."""
    from gm2 import native
    from gm2.masks import PackedMasks, pack_rows
    rng = np.random.Generator(np.random.PCG64(seed))
    f = rng.beta(0.1, 1.0, size=G)
    f[rng.random(G) < 0.15] = 0.98
    ld = native.packed_row_bytes(G) * 8
    fd = torch.zeros(ld, device="cuda")
    fd[:G] = torch.from_numpy(f.astype(np.float32)).cuda()      # pad columns: frequency 0
    gen = torch.Generator(device="cuda").manual_seed(seed)
    p = PackedMasks.empty(n, G, "cuda")
    for r0 in range(0, n, 4096):
        m = min(4096, n - r0)
        p.bits[r0:r0 + m] = pack_rows((torch.rand(m, ld, device="cuda", generator=gen) < fd).to(torch.uint8))
    return p


def torch_counts(p, torch, rows=2048):
    """The column sums by unpacking the bits with torch, `rows` rows at a time -> device int64 [G]."""
    shifts = torch.arange(8, device="cuda", dtype=torch.uint8)
    total = torch.zeros(p.ld * 8, dtype=torch.int64, device="cuda")
    for r0 in range(0, p.n, rows):
        b = p.bits[r0:r0 + rows]
        total += ((b.unsqueeze(-1) >> shifts) & 1).sum(0, dtype=torch.int64).reshape(-1)
    return total[:p.G]


def measure(name, n, G, a, torch, np):
    from gm2 import native
    p = synthetic_packed(n, G, 4242, torch, np)
    row_bytes = (G + 127) // 128 * 16
    counts = torch.empty(G, dtype=torch.int64, device="cuda")
    res = {"rows": n, "genes": G, "bytes_read": n * row_bytes}
    ms, lo, hi = median_ms(lambda: native.mask_gene_counts(p.bits, n, p.ld, G, None, n, counts), a.reps, torch)
    res["all_ms_back_to_back"] = burst_ms(lambda: native.mask_gene_counts(p.bits, n, p.ld, G, None, n, counts), a.reps, torch)
    res.update(all_ms=ms, all_ms_min=lo, all_ms_max=hi, all_tb_per_s=n * row_bytes / (ms * 1e-3) / 1e12)
    res["all_fraction_of_hbm_read"] = res["all_tb_per_s"] / HBM_READ_TBS
    all_counts = counts.clone()
    half = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))[:n // 2]
    idx = half.to(torch.int32)
    ms, lo, hi = median_ms(lambda: native.mask_gene_counts(p.bits, n, p.ld, G, idx, idx.numel(), counts), a.reps, torch)
    res.update(half_ms=ms, half_ms_min=lo, half_ms_max=hi,
               half_tb_per_s=idx.numel() * row_bytes / (ms * 1e-3) / 1e12)
    res["half_fraction_of_hbm_gather"] = res["half_tb_per_s"] / HBM_GATHER_TBS
    rest = torch.ones(n, dtype=torch.bool, device="cuda")
    rest[half] = False
    native.mask_gene_counts(p.bits, n, p.ld, G, torch.nonzero(rest).reshape(-1).to(torch.int32), n - idx.numel(), counts,
                            accumulate=True)
    res["half_plus_rest_equals_all"] = bool(torch.equal(counts, all_counts))
    ms, lo, hi = median_ms(lambda: torch_counts(p, torch), a.torch_reps, torch)
    res.update(torch_ms=ms, torch_reps=a.torch_reps, torch_over_kernel=ms / res["all_ms"])
    res["equals_torch"] = bool(torch.equal(torch_counts(p, torch), all_counts))
    res["mean_frequency"] = float(all_counts.sum().item()) / (n * G)
    return name, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--strains", type=int, default=10_000)
    ap.add_argument("--genes", type=int, default=55039)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "genefreq_times.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("genefreq_bench: needs the GPU (a host run measures nothing)")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "hbm_read_tb_per_s": HBM_READ_TBS,
           "hbm_gather_tb_per_s": HBM_GATHER_TBS}
    for name, n in (("real", a.strains), ("sampled", a.samples)):
        key, r = measure(name, n, a.genes, a, torch, np)
        res[key] = r
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
