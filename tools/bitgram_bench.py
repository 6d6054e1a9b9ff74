#!/usr/bin/env python3
"""Times the bit-row cross products and BinaryPCA on the GPU (no pass / fail: a record).

On the synthetic pan-genome bench.py trains on (gm2.data.synthetic_pangenome, seed 4242), packed:
  * cooccur   the S x S self co-occurrence over G genes (gm2_mask_cooccur), default 7,512 x 55,039
  * nearest   Q generated-like rows against the S strains (gm2_mask_nearest), default 65,536 x 7,512
  * pca_fit   BinaryPCA(2).fit end to end (counts, centring, eigh, sign convention)
  * sklearn   sklearn PCA(n_components=2) on the same matrix as float64 on the host (the reference's
              route, explore_data/data_exploration.py:394-420), 16 threads
Kernel legs: warmed, then `--reps` calls between two device events. Rates are gene pairs per second
(rows x rows x G / time) beside the ceiling derived in DESIGN.md (one VALU lane-op per 32 pairs'
word: 64 lanes x 256 CUs x 2.4 GHz x 32 / 2 ops). Writes profiles/bitgram_times.json.

  python tools/bitgram_bench.py [--strains 7512 --genes 55039 --queries 65536 --reps 5 --no-sklearn]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome-minimizer-2_amd"))


def timed(fn, reps, torch):
    """Mean milliseconds of fn() over `reps` calls between two device events, after two warm-up calls."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--strains", type=int, default=7512)
    ap.add_argument("--genes", type=int, default=55039)
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bitgram_times.json"))
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    import numpy as np
    import torch

    from gm2 import native
    from gm2.data import ResidentMatrix, synthetic_pangenome
    from gm2.masks import PackedMasks, pack_rows
    from gm2.pca import BinaryPCA
    if not torch.cuda.is_available():
        raise SystemExit("bitgram_bench: needs the GPU (a host run measures nothing)")
    torch.set_num_threads(16)
    S, G, Q = a.strains, a.genes, a.queries
    x = synthetic_pangenome(S, G, seed=4242)
    mat = ResidentMatrix(x)
    real = PackedMasks.from_resident(mat)
    # queries, made on the device: strains with ~1 % of their genes flipped (the kernel's work does
    # not depend on the data)
    gen = torch.Generator(device="cuda").manual_seed(7)
    query = PackedMasks.empty(Q, G, "cuda")
    live = (torch.arange(mat.ld, device="cuda") < G)
    for q0 in range(0, Q, 4096):
        m = min(4096, Q - q0)
        rows = mat.data[torch.randint(0, S, (m,), device="cuda", generator=gen)]
        flip = (torch.rand(m, mat.ld, device="cuda", generator=gen) < 0.01) & live
        query.bits[q0:q0 + m] = pack_rows(rows ^ flip.to(torch.uint8))
    res = {"device": torch.cuda.get_device_name(0), "strains": S, "genes": G, "queries": Q, "reps": a.reps,
           "derived_ceiling_gene_pairs_per_s": 64 * 256 * 2.4e9 * 32 / 2}

    out = torch.empty(S, S, dtype=torch.int32, device="cuda")
    ms = timed(lambda: native.mask_cooccur(real.bits, S, real.ld, real.bits, S, real.ld, G, out, S), a.reps, torch)
    res["cooccur_ms"] = ms
    res["cooccur_gene_pairs_per_s"] = S * S * G / (ms * 1e-3)
    best = torch.empty(Q, dtype=torch.int64, device="cuda")
    ms = timed(lambda: native.mask_nearest(query.bits, Q, query.ld, real.bits, S, real.ld, G, best), a.reps, torch)
    res["nearest_ms"] = ms
    res["nearest_gene_pairs_per_s"] = Q * S * G / (ms * 1e-3)
    # spot check of what was timed: 64 queries against numpy
    key = best[:64].cpu().numpy()
    d = np.stack([(x != row).sum(axis=1, dtype=np.int64) for row in PackedMasks(query.bits[:64], G).unpack()])
    assert (key >> 32 == d.min(axis=1)).all() and (key & 0xFFFFFFFF == d.argmin(axis=1)).all()
    res["nearest_checked_rows"] = 64

    # warm-up at a small size (the solver's first call loads its code); the full fit is timed once
    BinaryPCA(2).fit(PackedMasks(real.bits[:512], G))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pca = BinaryPCA(2)
    pca.fit(real)
    torch.cuda.synchronize()
    res["pca_fit_ms"] = (time.perf_counter() - t0) * 1e3
    res["pca_explained_variance_ratio"] = [float(v) for v in pca.explained_variance_ratio_]
    t0 = time.perf_counter()
    pca.transform(query)
    torch.cuda.synchronize()
    res["pca_transform_ms"] = (time.perf_counter() - t0) * 1e3

    if not a.no_sklearn:
        from sklearn.decomposition import PCA
        xf = x.astype(np.float64)
        t0 = time.perf_counter()
        ref = PCA(n_components=2)
        ref.fit(xf)
        res["sklearn_pca_fit_ms"] = (time.perf_counter() - t0) * 1e3
        res["sklearn_threads"] = 16
        res["sklearn_solver"] = str(getattr(ref, "_fit_svd_solver", "auto"))
        # (no score comparison: the synthetic matrix has no cluster structure, its leading eigenvalues
        # are near-equal and their vectors not comparable; tests/test_*bitgram* compare on clustered data)
        res["sklearn_explained_variance_ratio"] = [float(v) for v in ref.explained_variance_ratio_]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
