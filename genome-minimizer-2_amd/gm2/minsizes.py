"""Minimized genome sizes and duplicate groups straight from the sampled masks.

The reference reaches the numbers of its summary report (minimizer/minimizer_2.py:273-424: the size
statistics of the minimized genomes and the duplicate analysis) through three steps: --mode sample
writes masks, convert-samples turns each into a list of gene names (binary_converter.py), and the
minimizer cuts the `gene` features of the GenBank record whose /gene name is not listed and joins what
is left. Every number of the report except the bases themselves depends only on WHICH gene features a
sample removes and on the union of their intervals. `FeaturePlan` restates that decision once per
(record, dataset columns, essential set) as one int32 code per gene feature, and the sizes follow from a
bit gather per feature and a prefix-max scan over the features sorted by start:
  * on the device  PackedMasks.minimized_stats(plan)  (gm2_mask_minimized_stats, csrc/masks.hip)
  * on the host    minimized_stats_numpy(x01, plan)   (the same outputs; the CPU path and the oracle)
No sequence is written: 1e6 samples of a 4.6 Mbp record are 24 MB of results instead of 4.6 TB of FASTA.
"""
from __future__ import annotations

import os

import numpy as np

__all__ = ["FeaturePlan", "mix64", "minimized_stats_numpy", "duplicate_stats", "duplicate_groups", "sample_ids",
           "size_table", "write_report"]

ALWAYS_REMOVED, ALWAYS_KEPT = -1, -2


class FeaturePlan:
    """The record's `gene` features sorted by start (stable), as int32 arrays:
      col    >= 0: the first-occurrence dataset column of the feature's /gene name; the feature is kept
             iff that bit of the sample is set. -1: no column has its name, the feature is always
             removed. -2: the name is an essential gene, the feature is always kept.
      start, end   the feature's [start, end) clipped to [0, L]
    and L (the record's length) and G (the number of dataset columns)."""

    def __init__(self, col, start, end, L, G):
        self.col = np.ascontiguousarray(col, dtype=np.int64)
        self.start = np.ascontiguousarray(start, dtype=np.int64)
        self.end = np.ascontiguousarray(end, dtype=np.int64)
        self.L, self.G = int(L), int(G)
        F = self.col.size
        if self.col.ndim != 1 or self.start.shape != (F,) or self.end.shape != (F,):
            raise ValueError("FeaturePlan: col, start and end must be 1-D arrays of one length")
        if self.L < 0 or self.L >= 2 ** 31:
            raise ValueError(f"FeaturePlan: a record of {self.L} bases does not fit the 32-bit positions (L < 2^31)")
        if F >= 2 ** 31:
            raise ValueError(f"FeaturePlan: {F} gene features do not fit the 32-bit feature index (F < 2^31)")
        if self.G < 1:
            raise ValueError("FeaturePlan: no dataset column (G < 1)")
        if F and (self.col.min() < ALWAYS_KEPT or self.col.max() >= self.G):
            raise ValueError(f"FeaturePlan: a feature column outside [-2, {self.G})")
        if F and (self.start.min() < 0 or self.end.max() > self.L or self.start.max() > self.L or self.end.min() < 0):
            raise ValueError(f"FeaturePlan: an interval outside [0, {self.L}]")
        if F and (np.diff(self.start) < 0).any():
            raise ValueError("FeaturePlan: the features must be sorted by start")
        self.col, self.start, self.end = (a.astype(np.int32) for a in (self.col, self.start, self.end))
        self._device = {}

    @property
    def F(self):
        return int(self.col.size)

    @staticmethod
    def build(record, cols, essential_set=None):
        """What the pipeline decides for a sample of this dataset on this record.
        masks_to_gene_lists keeps a name's FIRST column only (binary_converter.py:72-83), so a sample's
        needed names are the names of its set first-occurrence columns, plus -- with `essential_set`, the
        `_with_essentials` lists of check_essential_genes -- every essential name. GenomeMinimiser removes
        every `gene` feature whose /gene value (a missing qualifier counts as "") is not needed."""
        L = len(record.seq)
        if L >= 2 ** 31:
            raise ValueError(f"FeaturePlan: a record of {L} bases does not fit the 32-bit positions (L < 2^31)")
        names = cols.tolist() if hasattr(cols, "tolist") else list(cols)
        first = {}
        for i, name in enumerate(names):
            first.setdefault(name, i)
        essential = set(essential_set) if essential_set is not None else set()
        genes = [f for f in record.features if f.type == "gene"]
        col = np.empty(len(genes), dtype=np.int64)
        for k, f in enumerate(genes):
            name = f.qualifiers.get("gene", [""])[0]
            col[k] = ALWAYS_KEPT if name in essential else first.get(name, ALWAYS_REMOVED)
        start = np.clip(np.array([int(f.location.start) for f in genes], dtype=np.int64), 0, L)
        end = np.clip(np.array([int(f.location.end) for f in genes], dtype=np.int64), 0, L)
        o = np.argsort(start, kind="stable")
        return FeaturePlan(col[o], start[o], end[o], L, len(names))

    def device_tables(self, device):
        """(col, start, end) as int32 tensors on `device`, uploaded once per device."""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = tuple(torch.from_numpy(a).to(device) for a in (self.col, self.start, self.end))
        return self._device[key]


def mix64(z):
    """The splitmix64 finalizer on a uint64 array (arithmetic mod 2^64)."""
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xbf58476d1ce4e5b9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94d049bb133111eb)
        z ^= z >> np.uint64(31)
    return z


def _empty_stats():
    return {"removed_bp": np.zeros(0, np.int64), "genes_removed": np.zeros(0, np.int64),
            "reduced_length": np.zeros(0, np.int64), "signature": np.zeros(0, np.uint64)}


def minimized_stats_numpy(x01, plan, block=512):
    """The kernel's outputs from a host 0/1 matrix [n, G] (anything non-zero is a set bit). Per sample:
      genes_removed   the removed features, empty intervals included (`len(gm.features)`)
      removed_bp      the length of the union of the removed non-empty [start, end) intervals
      reduced_length  L - removed_bp (`len(gm.reduced_genome_str)`)
      signature       uint64: over the MERGED removed intervals (a new one starts at feature i iff
                      start_i > the largest end of the removed non-empty features before it: touching
                      intervals merge, as minimizer._merged does), the sum mod 2^64 of
                      mix64(2 start) + mix64(2 end + 1); 0 when nothing is removed.
    The signature groups the samples by their removed-region SET: equal sets give identical minimized
    sequences, so its groups are the reference's sequence duplicates (check_sequence_duplicates) up to an
    accidental coincidence of two sequences cut differently and 2^-64 hash collisions."""
    x = np.asarray(x01)
    if x.ndim != 2 or x.shape[1] != plan.G:
        raise ValueError(f"minimized_stats_numpy: a mask of shape {x.shape} for a plan of {plan.G} columns")
    n, F = x.shape[0], plan.F
    out = {"removed_bp": np.zeros(n, np.int64), "genes_removed": np.zeros(n, np.int64),
           "signature": np.zeros(n, np.uint64)}
    if n and F:
        col = plan.col.astype(np.int64)
        start, end = plan.start.astype(np.int64), plan.end.astype(np.int64)
        by_bit = col >= 0
        nonempty = end > start
        for r0 in range(0, n, block):
            xb = x[r0:r0 + block]
            kept = np.empty((xb.shape[0], F), dtype=bool)
            kept[:] = col == ALWAYS_KEPT
            kept[:, by_bit] = xb[:, col[by_bit]] != 0
            cut = ~kept & nonempty
            incl = np.maximum.accumulate(np.where(cut, end, -1), axis=1)
            cover = np.concatenate([np.full((xb.shape[0], 1), -1, np.int64), incl[:, :-1]], axis=1)
            opens = cut & (start > cover)
            closes = opens & (cover >= 0)   # (the interval before this one ends at `cover`)
            last = incl[:, -1]
            with np.errstate(over="ignore"):
                sig = np.where(opens, mix64(np.broadcast_to(2 * start, opens.shape)), np.uint64(0)).sum(
                    axis=1, dtype=np.uint64)
                sig += np.where(closes, mix64(2 * np.maximum(cover, 0) + 1), np.uint64(0)).sum(axis=1, dtype=np.uint64)
                sig += np.where(last >= 0, mix64(2 * np.maximum(last, 0) + 1), np.uint64(0))
            out["removed_bp"][r0:r0 + block] = np.where(cut, np.maximum(0, end - np.maximum(start, cover)), 0).sum(axis=1)
            out["genes_removed"][r0:r0 + block] = (~kept).sum(axis=1)
            out["signature"][r0:r0 + block] = sig
    out["reduced_length"] = plan.L - out["removed_bp"]
    return out


def sample_ids(n):
    """The FASTA record ids of the batch drivers (minimizer_2.py:455)."""
    return [f"Minimized_E_coli_K12_MG1655_{i + 1}" for i in range(n)]


def duplicate_groups(signature):
    """(group id of every sample, dense in order of first appearance; the samples of each group)."""
    sig = np.asarray(signature, dtype=np.uint64)
    uniq, first, inv = np.unique(sig, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    gid = rank[inv.reshape(-1)]
    order = np.argsort(gid, kind="stable")
    members = np.split(order, np.cumsum(np.bincount(gid, minlength=len(uniq)))[:-1]) if len(sig) else []
    return gid, members


def duplicate_stats(signature):
    """check_sequence_duplicates (minimizer_2.py:257-287) on the signatures instead of the sequences: the
    same dict, `duplicates_detail` keyed by the signature (int) with the FASTA ids of its samples."""
    sig = np.asarray(signature, dtype=np.uint64)
    gid, members = duplicate_groups(sig)
    ids = sample_ids(len(sig))
    dup = {int(sig[m[0]]): [ids[i] for i in m] for m in members if len(m) > 1}
    return {"total_sequences": len(sig), "unique_sequences": len(members), "duplicate_groups": len(dup),
            "duplicated_sequences": sum(len(v) for v in dup.values()),
            "unique_only_sequences": sum(1 for m in members if len(m) == 1), "duplicates_detail": dup,
            "compression_ratio": len(members) / len(sig) if len(sig) else 0}


def size_table(stats, genome_size, L):
    """The per-sample table of --minimized-sizes: genome_size = genes of the sample (row popcount)."""
    import pandas as pd
    red = np.asarray(stats["reduced_length"], dtype=np.int64)
    gid, _ = duplicate_groups(stats["signature"])
    return pd.DataFrame({"sample": np.arange(len(red)), "genome_size": np.asarray(genome_size, dtype=np.int64),
                         "genes_removed": np.asarray(stats["genes_removed"], dtype=np.int64),
                         "reduced_length_bp": red,
                         "reduction_pct": (L - red) / L * 100.0 if L else np.zeros(len(red)),
                         "duplicate_group": gid})


def write_report(output_file, model_name, genome_path, genes_path, plan, stats, dup=None):
    """The reference's summary file (generate_summary_file, minimizer_2.py:326-424) for the FASTA name
    `output_file`, from the sizes (in Mbp, as the batch drivers hand them over) and the duplicate stats of
    the signatures: no FASTA is read or written. Returns the duplicate stats."""
    from .minimizer import generate_summary_file
    dup = duplicate_stats(stats["signature"]) if dup is None else dup
    sizes = (np.asarray(stats["reduced_length"], dtype=np.float64) / 1e6).tolist()
    generate_summary_file(output_file, model_name, os.fspath(genome_path), os.fspath(genes_path), plan.L, sizes, dup)
    return dup
