#!/usr/bin/env python3
"""Times the minimized genome sizes on packed masks (no pass / fail: a record).

Synthetic packed rows with the SURVEY.md §8 gene frequencies (tools/genefreq_bench.py synthetic_packed),
made on the device from a seed (default 65,536 x 55,039), and a synthetic GenBank record of --features
gene features over --length bases (an E. coli K-12 sized 4,600 over 4.64 Mbp): nine in ten features carry
the name of a dataset column, one in fifty of those is essential, neighbouring genes overlap now and then.
  * kernel   gm2_mask_minimized_stats into preallocated outputs
  * copy     torch.Tensor.copy_ of a flat buffer of half the row bytes (the same traffic with no work in
             between, measured in the same run): the yardstick
  * host     the three-step route for --host-samples of the same rows: the row's gene-name list, then
             gm2.minimizer.GenomeMinimiser on the record (interval merge + string join), per sample
Each device leg: warmed, then `--reps` calls, each between its own pair of device events; the median. The
kernel's results are compared with the numpy statement on the first 256 rows and with the host route's
string lengths. Prints one JSON line and writes it to profiles/minsizes_times.json.

  python tools/minsizes_bench.py [--samples 65536 --genes 55039 --features 4600 --reps 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome-minimizer-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_TBS = 6.29   # MI355X_MICROARCH.md: the float4 device copy, read + written bytes per second / 1e12


def synthetic_record(F, L, G, np, seed=77):
    """(GenBankRecord, column names, essential names): F gene features tiling L bases with small overlaps."""
    from gm2.minimizer import Feature, GenBankRecord
    rng = np.random.Generator(np.random.PCG64(seed))
    seq = "ACGT" * (L // 4) + "A" * (L % 4)
    cols = [f"gene{i:05d}" for i in range(G)]
    start = np.sort(rng.integers(0, L - 2000, size=F))
    length = rng.integers(150, 1800, size=F)
    named = rng.random(F) < 0.9
    pick = rng.choice(G, size=F, replace=False) if F <= G else rng.integers(0, G, size=F)
    feats, essential = [], set()
    for i in range(F):
        name = cols[pick[i]] if named[i] else f"orf{i}"
        if named[i] and rng.random() < 0.02:
            essential.add(name)
        feats.append(Feature("gene", int(start[i]), int(start[i] + length[i]), 1, {"gene": [name]}))
    return GenBankRecord(seq, feats, "SYNTH"), cols, essential


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=65536)
    ap.add_argument("--genes", type=int, default=55039)
    ap.add_argument("--features", type=int, default=4600)
    ap.add_argument("--length", type=int, default=4_641_652)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-samples", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "minsizes_times.json"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("minsizes_bench: needs the GPU (a host run measures nothing)")
    from genefreq_bench import median_ms, synthetic_packed
    from gm2 import native
    from gm2.minimizer import GenomeMinimiser, _GeneTable
    from gm2.minsizes import FeaturePlan, minimized_stats_numpy
    n, G = a.samples, a.genes
    rec, cols, essential = synthetic_record(a.features, a.length, G, np)
    plan = FeaturePlan.build(rec, cols, essential)
    p = synthetic_packed(n, G, 4242, torch, np)
    kb = native.packed_row_bytes(G)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "guide_copy_tb_per_s": COPY_TBS, "rows": n,
           "genes": G, "features": plan.F, "record_bp": plan.L, "row_bytes": n * kb, "table_bytes": 12 * plan.F}
    bp = torch.empty(n, dtype=torch.int64, device="cuda")
    gone = torch.empty(n, dtype=torch.int32, device="cuda")
    sig = torch.empty(n, dtype=torch.int64, device="cuda")
    col, start, end = plan.device_tables(p.bits.device)
    call = lambda: native.mask_minimized_stats(p.bits, n, p.ld, G, col, start, end, plan.F, bp, gone, sig)
    ms, lo, hi = median_ms(call, a.reps, torch)
    res.update(kernel_ms=ms, kernel_ms_min=lo, kernel_ms_max=hi, kernel_row_tb_per_s=n * kb / (ms * 1e-3) / 1e12,
               kernel_us_per_sample=ms * 1e3 / n, kernel_features_per_ns=n * plan.F / (ms * 1e6))
    src = torch.empty(n * kb // 2 // 16 * 16, dtype=torch.uint8, device="cuda").random_()
    dst = torch.empty_like(src)
    ms, lo, hi = median_ms(lambda: dst.copy_(src), a.reps, torch)
    res.update(copy_bytes_each_way=src.numel(), copy_ms=ms, copy_ms_min=lo, copy_ms_max=hi,
               copy_tb_per_s=2 * src.numel() / (ms * 1e-3) / 1e12)
    res["kernel_fraction_of_copy"] = res["kernel_row_tb_per_s"] / res["copy_tb_per_s"]
    del src, dst
    # the kernel against the numpy statement, and against the host route's strings
    k = min(n, 256)
    x = np.unpackbits(p.bits[:k, :(G + 7) // 8].cpu().numpy(), axis=1, count=G, bitorder="little")
    want = minimized_stats_numpy(x, plan)
    res["equals_numpy"] = bool((bp[:k].cpu().numpy() == want["removed_bp"]).all()
                               and (gone[:k].cpu().numpy() == want["genes_removed"]).all()
                               and (sig[:k].cpu().numpy().view(np.uint64) == want["signature"]).all())
    names, table = np.asarray(cols), _GeneTable(rec)
    m = min(k, a.host_samples)
    t_list = t_min = 0.0
    lens = []
    for i in range(m):
        t0 = time.perf_counter()
        needed = sorted(set(names[np.flatnonzero(x[i])].tolist()) | essential)
        t1 = time.perf_counter()
        gm = GenomeMinimiser(record=rec, needed_genes_list=needed, idx=i, model_name="bench", _table=table)
        t2 = time.perf_counter()
        t_list, t_min = t_list + (t1 - t0), t_min + (t2 - t1)
        lens.append(len(gm.reduced_genome_str))
    res.update(host_samples=m, host_gene_list_ms_per_sample=t_list / m * 1e3, host_minimizer_ms_per_sample=t_min / m * 1e3,
               host_lengths_equal_kernel=bool((plan.L - bp[:m].cpu().numpy() == np.array(lens)).all()),
               median_reduced_length=float(np.median(plan.L - bp.cpu().numpy())))
    res["host_over_kernel_per_sample"] = (t_list + t_min) / m * 1e6 / res["kernel_us_per_sample"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
