"""Per-gene frequencies of a genome set, and the real-vs-sampled table built on them.

The counts are the column sums of the 0/1 genomes x genes matrix: the reference's Figure 1a
(explore_data/data_exploration.py:119-120) and, thresholded, its Figure 1c (:213-230). For a
PackedMasks they are computed on the device (PackedMasks.gene_counts, gm2_mask_gene_counts); everything
else here is host code on int64 vectors of length G and never touches the device.
"""
from __future__ import annotations

import numpy as np


def gene_counts(x):
    """Genomes per gene -> int64 numpy [G]. x: a PackedMasks (counted on the device) or a host 0/1
    array [n, G]."""
    if hasattr(x, "gene_counts"):
        return x.gene_counts().cpu().numpy()
    return np.asarray(x).sum(axis=0, dtype=np.int64)


def threshold_curve(counts, thresholds=None):
    """Number of genes present in at least t genomes, for every t of `thresholds`
    (data_exploration.py:213-220; default np.linspace(0, 50, num=50)) -> int64 [T]."""
    t = np.linspace(0, 50, num=50) if thresholds is None else np.asarray(thresholds, dtype=np.float64)
    c = np.sort(np.asarray(counts))
    # genes with count >= t = G - (number of counts < t)
    return (len(c) - np.searchsorted(c, t, side="left")).astype(np.int64)


def pangenome_classes(counts, n, core=0.99, soft_core=0.95, shell=0.15):
    """Genes per pangenome class by the fraction of the n genomes they are present in: core
    (>= core n), soft core (>= soft_core n), shell (>= shell n), cloud (the rest); Roary's cut-offs.
    The comparisons are made in integers, so a count exactly at a cut-off belongs to the upper class."""
    c = np.asarray(counts, dtype=np.int64)

    def at_least(frac):
        # count / n >= frac without a rounded product: frac as a ratio of integers over 10^6
        num = int(round(frac * 1_000_000))
        return c * 1_000_000 >= num * int(n)

    is_core, is_soft, is_shell = at_least(core), at_least(soft_core), at_least(shell)
    return {"core": int(is_core.sum()), "soft_core": int((is_soft & ~is_core).sum()),
            "shell": int((is_shell & ~is_soft).sum()), "cloud": int((~is_shell).sum())}


def frequency_table(names, real_counts, n_real, sampled_counts, n_sampled, real_by=None, sampled_by=None):
    """One row per gene column, in column order (duplicate names kept): gene, real_count, real_freq,
    sampled_count, sampled_freq, delta = sampled_freq - real_freq; with real_by / sampled_by =
    (classes, counts [K, G], class sizes [K]) also one real_<class> / sampled_<class> frequency
    column per class."""
    import pandas as pd
    names = np.asarray(names)
    rc, sc = np.asarray(real_counts, dtype=np.int64), np.asarray(sampled_counts, dtype=np.int64)
    if not (len(names) == len(rc) == len(sc)):
        raise ValueError(f"frequency_table: {len(names)} names, {len(rc)} real and {len(sc)} sampled counts")
    rf = rc / float(n_real) if n_real else np.zeros(len(rc))
    sf = sc / float(n_sampled) if n_sampled else np.zeros(len(sc))
    cols = {"gene": names, "real_count": rc, "real_freq": rf, "sampled_count": sc, "sampled_freq": sf,
            "delta": sf - rf}
    for prefix, by in (("real", real_by), ("sampled", sampled_by)):
        if by is None:
            continue
        classes, table, sizes = by
        table = np.asarray(table, dtype=np.int64)
        if table.shape != (len(classes), len(names)) or len(sizes) != len(classes):
            raise ValueError(f"frequency_table: {prefix}_by does not hold [classes, G] counts and the class sizes")
        for k, cls in enumerate(classes):
            cols[f"{prefix}_{cls}"] = table[k] / float(sizes[k]) if sizes[k] else np.zeros(len(names))
    return pd.DataFrame(cols)


def frequency_summary(table, core=0.99, soft_core=0.95):
    """Headline numbers of a frequency_table: Pearson r of the two frequency vectors (nan when one is
    constant), mean and max |delta|, the real set's core genes and how many stay core / at least soft
    core in the sampled set, genes of the real set never sampled, genes sampled but absent from it."""
    rf, sf = table["real_freq"].to_numpy(dtype=np.float64), table["sampled_freq"].to_numpy(dtype=np.float64)
    rc, sc = table["real_count"].to_numpy(), table["sampled_count"].to_numpy()
    d = np.abs(sf - rf)
    constant = len(rf) < 2 or rf.std() == 0 or sf.std() == 0
    real_core = rf >= core
    return {"genes": int(len(rf)),
            "pearson_r": float("nan") if constant else float(np.corrcoef(rf, sf)[0, 1]),
            "mean_abs_delta": float(d.mean()) if len(d) else 0.0,
            "max_abs_delta": float(d.max()) if len(d) else 0.0,
            "real_core": int(real_core.sum()),
            "real_core_sampled_core": int((real_core & (sf >= core)).sum()),
            "real_core_sampled_soft_core": int((real_core & (sf >= soft_core)).sum()),
            "real_never_sampled": int(((rc > 0) & (sc == 0)).sum()),
            "sampled_absent_from_real": int(((sc > 0) & (rc == 0)).sum())}
