"""Packed sampled masks and their consumers on the device.

A sampled mask set lives in HBM as numpy packbits(bitorder='little') rows (bit g & 7 of byte g // 8 =
gene g; row pitch native.packed_row_bytes(G), a multiple of 16; bits beyond G zero): 1e6 F4-shaped
genomes are 6.9 GB instead of 55 GB of u8 or 440 GB of the reference's float64. The reference's
consumers run on it without leaving the device:
  * count_essential_genes (utils/extras.py:49-87)        -> PackedMasks.count_groups
  * genome sizes (main.py:376-380 statistics)             -> PackedMasks.row_sizes
  * masks_to_gene_lists (explore_data/binary_converter.py:19-76) -> PackedMasks.gene_index_csr
  * genomes per gene, `data_without_lineage.sum(axis=1)` (explore_data/data_exploration.py:119-120),
    and the genes-in-at-least-t-genomes curve built on it (:213-230)
                                                          -> PackedMasks.gene_counts / gene_counts_by
                                                             (tables and summaries: gm2/genefreq.py)
  * the minimizer's sizes and duplicate groups (minimizer/minimizer_2.py:50-101, :273-424) without
    the sequences                                         -> PackedMasks.minimized_stats
                                                             (plan, oracle, report: gm2/minsizes.py)
and `to_host` returns the packed rows (8x less PCIe than u8) for the .npy writers.
"""
from __future__ import annotations

import numpy as np
import torch

from . import native


def essential_groups(essential_gene_positions, G):
    """The pickle dict {gene: [column, ...]} as CSR (group offsets, positions) of valid columns, in
    dict order. The reference tests `pos < G` (extras.py:71-82); a negative position indexes from
    the end as numpy does there (and raises where numpy would)."""
    offs, pos = [0], []
    for _, positions in essential_gene_positions.items():
        for p in positions:
            p = int(p)
            if p < G:
                if p < 0:
                    if p < -G:
                        raise IndexError(f"index {p} is out of bounds for axis 1 with size {G}")
                    p += G
                pos.append(p)
        offs.append(len(pos))
    return np.asarray(offs, dtype=np.int32), np.asarray(pos, dtype=np.int32)


def pack_rows(rows):
    """Device u8 0/1 rows [n, ld] (ld a multiple of 128, pad columns zero) -> packed rows [n, ld / 8]."""
    n, ld = rows.shape
    if ld % 128:
        raise ValueError("pack_rows: the row length must be a multiple of 128")
    w = (1 << torch.arange(8, device=rows.device, dtype=torch.int32))
    bits = torch.empty(n, ld // 8, dtype=torch.uint8, device=rows.device)
    for r0 in range(0, n, 1024):
        r = rows[r0:r0 + 1024]
        bits[r0:r0 + 1024] = (r.reshape(r.shape[0], -1, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)
    return bits


class PackedMasks:
    """n x G packed masks on the device (a [n, ld] uint8 tensor)."""

    def __init__(self, bits: torch.Tensor, G: int):
        self.bits, self.G = bits, int(G)
        self.n, self.ld = int(bits.shape[0]), int(bits.shape[1])
        if self.ld % 16 or self.ld * 8 < self.G:
            raise ValueError("packed mask rows: pitch must be a multiple of 16 bytes covering G")

    @staticmethod
    def empty(n, G, device):
        ld = native.packed_row_bytes(G)
        return PackedMasks(torch.zeros(n, ld, dtype=torch.uint8, device=device), G)

    @staticmethod
    def from_host(mask, threshold=0.5, device=None):
        """Threshold a host [n, G] mask (any numeric dtype; `>= threshold` as binary_converter.py:55)
        and upload it packed."""
        m = np.asarray(mask)
        n, G = m.shape
        ld = native.packed_row_bytes(G)
        packed = np.zeros((n, ld), dtype=np.uint8)
        packed[:, : (G + 7) // 8] = np.packbits(m >= threshold, axis=1, bitorder="little")
        dev = device or torch.device("cuda", torch.cuda.current_device())
        return PackedMasks(torch.from_numpy(packed).to(dev), G)

    @staticmethod
    def from_resident(matrix):
        """The rows of a gm2.data.ResidentMatrix packed: the target bits of its GEMM operands when
        they are already built (the same bytes), else its u8 rows packed once on the device."""
        n, G = matrix.n, matrix.G
        for ops in matrix.__dict__.get("_operands", {}).values():
            return PackedMasks(ops.bits[:n].view(torch.uint8), G)
        return PackedMasks(pack_rows(matrix.data[:n]), G)

    def cooccurrence(self, other=None):
        """popcount(row_i AND other_j) for every pair -> device int32 [n, m] (other None: this set
        with itself, the Gram matrix X X^T of the 0/1 rows)."""
        o = self if other is None else other
        if o.G != self.G:
            raise ValueError(f"cooccurrence: {self.G} genes against {o.G}")
        out = torch.empty(self.n, o.n, dtype=torch.int32, device=self.bits.device)
        native.mask_cooccur(self.bits, self.n, self.ld, o.bits, o.n, o.ld, self.G, out, o.n)
        return out

    def nearest(self, other):
        """For every row the nearest row of `other` by Hamming distance, ties to the lowest index ->
        (hamming int64 numpy [n], index int64 numpy [n]); no n x m matrix is formed."""
        if other.G != self.G:
            raise ValueError(f"nearest: {self.G} genes against {other.G}")
        best = torch.empty(self.n, dtype=torch.int64, device=self.bits.device)
        native.mask_nearest(self.bits, self.n, self.ld, other.bits, other.n, other.ld, self.G, best)
        key = best.cpu().numpy()
        return key >> 32, key & 0xFFFFFFFF

    def transposed(self):
        """The gene-major set: a PackedMasks of G rows x n "genes", row g = the genomes that carry gene
        g as a packed bit row (gm2_mask_transpose, on the device)."""
        if self.n == 0:
            raise ValueError("transposed: no rows to transpose (n = 0)")
        ld = native.packed_row_bytes(self.n)
        out = torch.zeros(self.G, ld, dtype=torch.uint8, device=self.bits.device)
        native.mask_transpose(self.bits, self.n, self.ld, self.G, out, ld)
        return PackedMasks(out, self.n)

    def _gene_list(self, genes):
        """A column index array -> device int64 indices for index_select (None: every gene). Host
        arrays are range-checked as _row_list does; a device tensor's entries are index_select's."""
        dev = self.bits.device
        if genes is None:
            return None
        if isinstance(genes, torch.Tensor):
            return genes.reshape(-1).to(device=dev, dtype=torch.int64)
        g = np.asarray(genes)
        if g.size == 0:
            g = np.zeros(0, dtype=np.int64)
        elif g.ndim != 1 or not np.issubdtype(g.dtype, np.integer):
            raise ValueError("gene_cooccurrence: genes must be a 1-D integer index array")
        if g.size and (g.min() < 0 or g.max() >= self.G):
            raise ValueError(f"gene_cooccurrence: gene indices outside [0, {self.G})")
        return torch.from_numpy(g.astype(np.int64)).to(dev)

    def gene_cooccurrence(self, genes=None, other_genes=None, transposed=None):
        """Genomes that carry both gene a and gene b -> device int32 [Ka, Kb] (the Gram matrix X^T X
        restricted to the chosen columns). genes / other_genes: integer column index arrays, repeats
        allowed, None = every gene; other_genes None = genes. transposed: this set's transposed() when
        the caller already holds it, else it is formed here."""
        t = self.transposed() if transposed is None else transposed
        if t.n != self.G or t.G != self.n:
            raise ValueError(f"gene_cooccurrence: a transposed set of {t.n} rows x {t.G} for {self.n} x {self.G}")
        ia = self._gene_list(genes)
        ib = ia if other_genes is None else self._gene_list(other_genes)
        a = t if ia is None else PackedMasks(t.bits.index_select(0, ia), t.G)
        if other_genes is None:
            return a.cooccurrence()
        b = t if ib is None else PackedMasks(t.bits.index_select(0, ib), t.G)
        return a.cooccurrence(b)

    def _row_list(self, rows):
        """An index array or a boolean mask of length n -> device int32 indices. Host arrays are
        range-checked here; a device tensor's entries are the caller's (the debug build checks them)."""
        if isinstance(rows, torch.Tensor):
            if rows.dtype == torch.bool:
                if rows.numel() != self.n:
                    raise ValueError(f"gene_counts: a boolean mask of {rows.numel()} rows for {self.n}")
                rows = torch.nonzero(rows.reshape(-1)).reshape(-1)
            return rows.reshape(-1).to(device=self.bits.device, dtype=torch.int32).contiguous()
        r = np.asarray(rows)
        if r.dtype == bool:
            if r.shape != (self.n,):
                raise ValueError(f"gene_counts: a boolean mask of shape {r.shape} for {self.n} rows")
            r = np.flatnonzero(r)
        elif r.size == 0:
            r = np.zeros(0, dtype=np.int64)
        elif r.ndim != 1 or not np.issubdtype(r.dtype, np.integer):
            raise ValueError("gene_counts: rows must be a 1-D integer index array or a boolean mask")
        if r.size and (r.min() < 0 or r.max() >= self.n):
            raise ValueError(f"gene_counts: row indices outside [0, {self.n})")
        return torch.from_numpy(r.astype(np.int32)).to(self.bits.device)

    def gene_counts(self, rows=None, out=None):
        """Genomes per gene (binary.sum(axis=0); explore_data/data_exploration.py:119-120) -> device
        int64 [G]. rows: an integer index array (repeats counted each time) or a boolean mask of
        length n, None = every row. out (device int64 [G]) is added to and returned."""
        if out is None:
            counts, acc = torch.empty(self.G, dtype=torch.int64, device=self.bits.device), False
        else:
            if out.dtype != torch.int64 or out.numel() != self.G or not out.is_contiguous() or \
                    out.device != self.bits.device:
                raise ValueError(f"gene_counts: out must be a contiguous device int64 [{self.G}] tensor")
            counts, acc = out, True
        if rows is None:
            native.mask_gene_counts(self.bits, self.n, self.ld, self.G, None, self.n, counts, acc)
        else:
            idx = self._row_list(rows)
            native.mask_gene_counts(self.bits, self.n, self.ld, self.G, idx if idx.numel() else None, idx.numel(),
                                    counts, acc)
        return counts

    def gene_counts_by(self, labels):
        """Per-class gene counts: (classes (np.unique order), int64 numpy [K, G]), one call per class
        with that class's index list, so the matrix is read once in total; the rows of the table
        sum to gene_counts()."""
        lab = np.asarray(labels)
        if lab.shape != (self.n,):
            raise ValueError(f"gene_counts_by: {lab.shape} labels for {self.n} rows")
        classes, inv = np.unique(lab, return_inverse=True)
        table = torch.empty(len(classes), self.G, dtype=torch.int64, device=self.bits.device)
        for k in range(len(classes)):
            idx = torch.from_numpy(np.flatnonzero(inv == k).astype(np.int32)).to(self.bits.device)
            native.mask_gene_counts(self.bits, self.n, self.ld, self.G, idx, idx.numel(), table[k])
        return classes, table.cpu().numpy()

    def to_host(self):
        """numpy packbits rows [n, ceil(G/8)] (bitorder 'little')."""
        return self.bits[:, : (self.G + 7) // 8].cpu().numpy()

    def unpack(self, dtype=np.uint8):
        """The [n, G] 0/1 mask on the host in `dtype` (the reference's float64 with dtype=float)."""
        u = np.unpackbits(self.to_host(), axis=1, count=self.G, bitorder="little")
        return u if dtype == np.uint8 else u.astype(dtype)

    def count_groups(self, essential_gene_positions):
        """count_essential_genes(binary, positions) on the device -> int64 numpy [n]."""
        offs, pos = essential_groups(essential_gene_positions, self.G)
        dev = self.bits.device
        counts = torch.empty(self.n, dtype=torch.int32, device=dev)
        go = torch.from_numpy(offs).to(dev)
        po = torch.from_numpy(pos if len(pos) else np.zeros(1, np.int32)).to(dev)
        native.mask_count_groups(self.bits, self.n, self.ld, go, len(offs) - 1, po, counts)
        return counts.cpu().numpy().astype(np.int64)

    def minimized_stats(self, plan):
        """What the genome minimizer would cut from the plan's GenBank record for every row, without the
        sequences (gm2.minsizes.FeaturePlan; gm2_mask_minimized_stats on the device) -> a dict of host
        arrays [n]: removed_bp, genes_removed, reduced_length (int64) and signature (uint64; equal for rows
        with the same merged removed regions). The same outputs as minsizes.minimized_stats_numpy."""
        if plan.G != self.G:
            raise ValueError(f"minimized_stats: a plan of {plan.G} gene columns for masks of {self.G}")
        if self.n == 0:
            from .minsizes import _empty_stats
            return _empty_stats()
        dev = self.bits.device
        bp = torch.empty(self.n, dtype=torch.int64, device=dev)
        gone = torch.empty(self.n, dtype=torch.int32, device=dev)
        sig = torch.empty(self.n, dtype=torch.int64, device=dev)   # (the uint64's bytes)
        col, start, end = plan.device_tables(dev) if plan.F else (None, None, None)
        native.mask_minimized_stats(self.bits, self.n, self.ld, self.G, col, start, end, plan.F, bp, gone, sig)
        removed = bp.cpu().numpy()
        return {"removed_bp": removed, "genes_removed": gone.cpu().numpy().astype(np.int64),
                "reduced_length": plan.L - removed, "signature": sig.cpu().numpy().view(np.uint64)}

    def _keep(self, keep_cols):
        if keep_cols is None:
            return None
        k = np.zeros(self.ld, dtype=np.uint8)
        k[: (self.G + 7) // 8] = np.packbits(np.asarray(keep_cols, dtype=bool), bitorder="little")
        return torch.from_numpy(k).to(self.bits.device)

    def row_offsets(self, keep_cols=None):
        offsets = torch.empty(self.n + 1, dtype=torch.int64, device=self.bits.device)
        native.mask_row_offsets(self.bits, self.n, self.ld, self._keep(keep_cols), offsets)
        return offsets

    def row_sizes(self):
        """Genes per sample (binary.sum(axis=1)) -> int64 numpy [n]."""
        return np.diff(self.row_offsets().cpu().numpy())

    def gene_index_csr(self, keep_cols=None):
        """(offsets int64 [n+1], column indices int32) of the set genes of every row, ascending;
        keep_cols (bool [G]) restricts to the kept columns."""
        keep = self._keep(keep_cols)
        offsets = torch.empty(self.n + 1, dtype=torch.int64, device=self.bits.device)
        native.mask_row_offsets(self.bits, self.n, self.ld, keep, offsets)
        total = int(offsets[-1].item())
        idx = torch.empty(max(total, 1), dtype=torch.int32, device=self.bits.device)
        native.mask_compact(self.bits, self.n, self.ld, keep, offsets, idx)
        return offsets.cpu().numpy(), idx[:total].cpu().numpy()


def gene_lists_from_csr(offsets, idx, names):
    """[[names[i] for the row's indices] for every row] (binary_converter.py:64-66)."""
    names = np.asarray(names)
    sel = names[idx].tolist()
    return [sel[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]
