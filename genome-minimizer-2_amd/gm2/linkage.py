"""Gene-gene linkage of a genome set, and the real-vs-sampled comparison built on it.

Which genes travel together (operons, mobile elements, mutually exclusive alleles) is the second-order
statistic of the 0/1 genomes x genes matrix: for a panel of K genes the K x K counts n11[a, b] = genomes
that carry both a and b. For a PackedMasks they are computed on the device
(PackedMasks.gene_cooccurrence: gm2_mask_transpose, then gm2_mask_cooccur on the gene-major rows);
everything here is host code on those integer matrices and never touches the device.

The measure is the phi coefficient of the 2 x 2 table of two genes, the Pearson correlation of their
0/1 columns: phi = (n n11 - n1 n2) / sqrt(n1 (n - n1) n2 (n - n2)), n1 / n2 the genes' own counts.
"""
from __future__ import annotations

import numpy as np


def select_panel(real_counts, n_real, k=2048, lo=0.05, hi=0.95):
    """The gene columns whose linkage is compared -> ascending int64 indices: of the genes present in a
    fraction lo <= f <= hi of the n_real strains (compared in integers, so a count exactly at a bound
    qualifies) the k of largest variance c (n - c), ties to the lower column; fewer when fewer qualify."""
    c, n = np.asarray(real_counts, dtype=np.int64), int(n_real)
    # count / n against a bound without a rounded product: the bound as a ratio of integers over 10^6
    lo_num, hi_num = int(round(lo * 1_000_000)), int(round(hi * 1_000_000))
    ok = np.flatnonzero((c * 1_000_000 >= lo_num * n) & (c * 1_000_000 <= hi_num * n))
    order = np.argsort(-(c[ok] * (n - c[ok])), kind="stable")  # (stable: ties keep column order)
    return np.sort(ok[order[:max(int(k), 0)]]).astype(np.int64)


def phi_matrix(both, counts, n):
    """phi of every pair of K genes -> fp64 [K, K]. both: int [K, K] genomes with both genes; counts:
    int [K] genomes per gene (the diagonal of both); n: genomes. The numerator is exact (int64); a gene
    constant in the set (count 0 or n) has no correlation: its row and column are 0.0."""
    b, c, n = np.asarray(both, dtype=np.int64), np.asarray(counts, dtype=np.int64), int(n)
    if b.ndim != 2 or b.shape != (len(c), len(c)):
        raise ValueError(f"phi_matrix: counts of {len(c)} genes for a {b.shape} matrix")
    num = n * b - c[:, None] * c[None, :]
    var = c * (n - c)
    v = var.astype(np.float64)
    den = np.sqrt(v[:, None] * v[None, :])  # (sqrt(v v) = v: a gene against itself or its copy is exactly 1.0)
    live = (var[:, None] > 0) & (var[None, :] > 0)
    return np.where(live, num / np.where(live, den, 1.0), 0.0)


def _upper(m):
    m = np.asarray(m, dtype=np.float64)
    return m[np.triu_indices(m.shape[0], 1)]


def linkage_summary(phi_real, phi_sampled, strong=0.5):
    """Headline numbers over the gene pairs a < b of two phi matrices of one panel: Pearson r of the two
    (nan when one side is constant), mean and max |delta|, the real set's strongly linked pairs
    (|phi| >= strong), how many of them the samples keep (same sign, |phi| >= strong / 2), pairs strongly
    linked in the samples alone (|phi_real| < strong / 2), and the genes constant in each set (a phi
    diagonal of 0)."""
    pr, ps = np.asarray(phi_real, dtype=np.float64), np.asarray(phi_sampled, dtype=np.float64)
    if pr.shape != ps.shape or pr.ndim != 2 or pr.shape[0] != pr.shape[1]:
        raise ValueError(f"linkage_summary: phi matrices of shapes {pr.shape} and {ps.shape}")
    r, s = _upper(pr), _upper(ps)
    d = np.abs(s - r)
    constant = len(r) < 2 or r.std() == 0 or s.std() == 0
    real_strong = np.abs(r) >= strong
    kept = real_strong & (np.sign(r) == np.sign(s)) & (np.abs(s) >= strong / 2)
    return {"pairs": int(len(r)),
            "pearson_r": float("nan") if constant else float(np.corrcoef(r, s)[0, 1]),
            "mean_abs_delta": float(d.mean()) if len(d) else 0.0,
            "max_abs_delta": float(d.max()) if len(d) else 0.0,
            "real_strong": int(real_strong.sum()),
            "real_strong_kept": int(kept.sum()),
            "sampled_strong_new": int(((np.abs(s) >= strong) & (np.abs(r) < strong / 2)).sum()),
            "real_constant": int((np.diagonal(pr) == 0).sum()),
            "sampled_constant": int((np.diagonal(ps) == 0).sum())}


def linkage_table(names, panel, both_real, counts_real, n_real, both_sampled, counts_sampled, n_sampled, top=1000):
    """The gene pairs worth reading: gene_a, gene_b (names of panel columns a < b), real_both, real_phi,
    sampled_both, sampled_phi, delta = sampled_phi - real_phi, for the union of the `top` pairs by
    |real_phi| and the `top` pairs by |delta| (ties to the lower pair), sorted by |delta| descending,
    then by (column a, column b). names: every gene column's name; panel: K column indices; both_* [K, K]
    and counts_* [K]: the panel's counts in each set."""
    import pandas as pd
    names, panel = np.asarray(names), np.asarray(panel, dtype=np.int64)
    br, bs = np.asarray(both_real, dtype=np.int64), np.asarray(both_sampled, dtype=np.int64)
    K = len(panel)
    if br.shape != (K, K) or bs.shape != (K, K):
        raise ValueError(f"linkage_table: a panel of {K} genes for matrices {br.shape} and {bs.shape}")
    pr, ps = phi_matrix(br, counts_real, n_real), phi_matrix(bs, counts_sampled, n_sampled)
    ia, ib = np.triu_indices(K, 1)
    r, s = pr[ia, ib], ps[ia, ib]
    d = s - r
    top = max(int(top), 0)
    keep = np.union1d(np.argsort(-np.abs(r), kind="stable")[:top], np.argsort(-np.abs(d), kind="stable")[:top])
    keep = keep[np.lexsort((panel[ib[keep]], panel[ia[keep]], -np.abs(d[keep])))]
    a, b = ia[keep], ib[keep]
    return pd.DataFrame({"gene_a": names[panel[a]], "gene_b": names[panel[b]], "real_both": br[a, b],
                         "real_phi": r[keep], "sampled_both": bs[a, b], "sampled_phi": s[keep], "delta": d[keep]})
