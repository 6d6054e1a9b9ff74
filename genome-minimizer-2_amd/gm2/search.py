"""Streaming search for the smallest viable distinct genomes (csrc/search.hip, gm2.h gm2_search_*).

The reference's answer to "find me a minimal genome" is focused sampling (main.py:351-370): 100 samples,
the smallest, noise around it. With a decoder that makes millions of genomes a second the other question
can be asked: screen N genomes and keep the `keep` smallest DISTINCT ones that still carry their essential
genes (count_essential_genes, utils/extras.py:49-87). Nothing of size N exists anywhere: each decoded
chunk is folded into a device-resident state of at most `keep` winners (size, essential count, packed
row, z), and the masks of the losers never leave the device.

  * smallest_distinct_numpy   the oracle on a host 0/1 matrix
  * SmallestSearch            the device state: push(PackedMasks) / merge(other) / result()
  * search_smallest           draw z per chunk, model.decode_bits, push

Order: a genome's key is (size, global index); of equal rows only the one with the lowest index counts.
The device decides "equal rows" by a 64-bit hash of the row bytes (gm2.h): different rows are taken for
equal with probability about 2^-64 per pair, as with minsizes' signature.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import native
from .masks import PackedMasks, essential_groups

__all__ = ["smallest_distinct_numpy", "essential_counts_numpy", "resolve_min_essential", "group_tables",
           "SearchResult", "SmallestSearch", "search_smallest"]

INDEX_BITS = 40


def group_tables(essential_gene_positions, G):
    """(group offsets int32 [n_groups + 1], positions int32) from the pickle's {gene: [column, ...]} dict
    (masks.essential_groups) or an (offsets, positions) pair already in that form."""
    if isinstance(essential_gene_positions, dict):
        return essential_groups(essential_gene_positions, G)
    offs, pos = essential_gene_positions
    offs, pos = np.asarray(offs, dtype=np.int32).reshape(-1), np.asarray(pos, dtype=np.int32).reshape(-1)
    if len(offs) < 1 or offs[0] != 0 or (np.diff(offs) < 0).any() or offs[-1] != len(pos):
        raise ValueError("group offsets must ascend from 0 to the number of positions")
    if len(pos) and (pos.min() < 0 or pos.max() >= G):
        raise ValueError(f"group positions outside [0, {G})")
    return offs, pos


def resolve_min_essential(group_offsets, min_essential=None):
    """The viability bound: None = every group that has a valid position must be present (the number of
    non-empty groups); a number is taken as it is (0 = no constraint)."""
    if min_essential is None:
        return int((np.diff(np.asarray(group_offsets, dtype=np.int64)) > 0).sum())
    if int(min_essential) < 0:
        raise ValueError("min_essential must be >= 0")
    return int(min_essential)


def essential_counts_numpy(x01, group_offsets, positions):
    """count_essential_genes on a host 0/1 matrix from the CSR tables -> int64 [n]."""
    x = np.asarray(x01)
    out = np.zeros(x.shape[0], dtype=np.int64)
    for g in range(len(group_offsets) - 1):
        p = np.asarray(positions[group_offsets[g]:group_offsets[g + 1]], dtype=np.int64)
        if len(p):
            out += (x[:, p] != 0).any(axis=1)
    return out


def smallest_distinct_numpy(x01, group_offsets, positions, keep, min_groups, indices=None):
    """The oracle: of the rows of the 0/1 matrix x01 [n, G] with essential count >= min_groups (viable),
    deduplicated by exact bytes keeping the lowest index, the first `keep` in (size, index) order.
    indices: the rows' global indices (default 0..n-1). Returns a dict: indices, sizes, essential (int64
    [k]), rows (uint8 [k, G]), seen, viable (ints), size_hist (int64 [G + 1], all rows seen) and ess_hist
    (int64 [n_groups + 1])."""
    x = (np.asarray(x01) != 0).astype(np.uint8)
    n, G = x.shape
    idx = np.arange(n, dtype=np.int64) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
    if idx.shape != (n,):
        raise ValueError(f"smallest_distinct_numpy: {idx.shape} indices for {n} rows")
    sizes = x.sum(axis=1, dtype=np.int64)
    ess = essential_counts_numpy(x, group_offsets, positions)
    n_groups = len(group_offsets) - 1
    viable = ess >= int(min_groups)
    cand = np.flatnonzero(viable)
    cand = cand[np.argsort(idx[cand], kind="stable")]          # by global index: the first copy is the lowest
    if len(cand):
        packed = np.packbits(x[cand], axis=1, bitorder="little")
        _, first = np.unique(packed, axis=0, return_index=True)
        cand = cand[np.sort(first)]
    order = np.lexsort((idx[cand], sizes[cand]))[: int(keep)]
    win = cand[order]
    return {"indices": idx[win], "sizes": sizes[win], "essential": ess[win], "rows": x[win],
            "seen": int(n), "viable": int(viable.sum()),
            "size_hist": np.bincount(sizes, minlength=G + 1).astype(np.int64),
            "ess_hist": np.bincount(ess, minlength=n_groups + 1).astype(np.int64)}


@dataclass
class SearchResult:
    """What SmallestSearch.result returns, the winners in (size, index) order."""
    indices: np.ndarray       # int64 [k] global indices
    sizes: np.ndarray         # int64 [k] genes per genome
    essential: np.ndarray     # int64 [k] essential counts
    masks: PackedMasks        # the k winners, on the device
    z: "torch.Tensor | None"  # fp32 [k, L] on the device
    seen: int
    viable: int
    size_hist: np.ndarray     # int64 [G + 1], over every genome seen
    ess_hist: np.ndarray      # int64 [n_groups + 1]


def hist_quantiles(hist):
    """(median, min, max) of the values a histogram counts (numpy's median of the expanded list), or None
    when it counts nothing."""
    h = np.asarray(hist, dtype=np.int64)
    total = int(h.sum())
    if total == 0:
        return None
    cum = np.cumsum(h)
    lo = int(np.searchsorted(cum, (total - 1) // 2 + 1))
    hi = int(np.searchsorted(cum, total // 2 + 1))
    nz = np.flatnonzero(h)
    return (lo + hi) / 2.0, int(nz[0]), int(nz[-1])


class SmallestSearch:
    """The device state of one streaming search: two winner buffers of `keep` entries (a push reads one
    and writes the other), the stream totals and histograms, and the scratch of a push of up to chunk_max
    rows. Every call but result() is stream-ordered on torch's current stream with no host wait."""

    def __init__(self, G, keep, essential_gene_positions, min_essential=None, latent_dim=None, device=None,
                 chunk_max=65536):
        self.G, self.K = int(G), int(keep)
        if not 1 <= self.K <= native.SEARCH_MAX_K:
            raise ValueError(f"keep {keep} outside [1, {native.SEARCH_MAX_K}]")
        if not 1 <= self.G < native.SEARCH_MAX_G:
            raise ValueError(f"G {G} outside [1, 2^23)")
        if not 1 <= int(chunk_max) <= native.SEARCH_MAX_N:
            raise ValueError(f"chunk_max {chunk_max} outside [1, 2^20]")
        self.chunk_max = int(chunk_max)
        self.group_offsets, self.positions = group_tables(essential_gene_positions, self.G)
        self.n_groups = len(self.group_offsets) - 1
        self.min_groups = resolve_min_essential(self.group_offsets, min_essential)
        self.L = None if latent_dim is None else int(latent_dim)
        dev = self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.ld = native.packed_row_bytes(self.G)
        self._goff = torch.from_numpy(self.group_offsets).to(dev)
        self._pos = torch.from_numpy(self.positions if len(self.positions) else np.zeros(1, np.int32)).to(dev)
        K = self.K
        self.totals = torch.zeros(2, dtype=torch.int64, device=dev)
        self.size_hist = torch.zeros(self.G + 1, dtype=torch.int64, device=dev)
        self.ess_hist = torch.zeros(self.n_groups + 1, dtype=torch.int64, device=dev)
        self.error = torch.zeros(1, dtype=torch.int32, device=dev)
        self._buf, self._state = [], []
        for _ in range(2):
            b = {"keys": torch.zeros(K, dtype=torch.int64, device=dev), "hashes": torch.zeros(K, dtype=torch.int64, device=dev),
                 "essential": torch.zeros(K, dtype=torch.int32, device=dev),
                 "rows": torch.zeros(K, self.ld, dtype=torch.uint8, device=dev),
                 "z": None if self.L is None else torch.zeros(K, self.L, dtype=torch.float32, device=dev),
                 "count": torch.zeros(1, dtype=torch.int32, device=dev)}
            self._buf.append(b)
            self._state.append(native.search_state(b["keys"], b["hashes"], b["essential"], b["rows"], b["z"], b["count"],
                                                   self.totals, self.size_hist, self.ess_hist, self.error))
        self._cur = 0
        self._scratch_bytes = native.search_scratch_size(max(self.chunk_max, K), K)
        self._scratch = self._aligned(self._scratch_bytes)
        self.next_index = 0
        native.search_init(self._state[0], self.G, self.n_groups)

    def _aligned(self, nbytes):
        raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-raw.data_ptr()) % 256
        return raw[off: off + nbytes]

    def push(self, packed: PackedMasks, z=None, base_index=None):
        """Fold the rows of `packed` (global indices base_index, base_index + 1, ...) into the state.
        base_index defaults to the index after the last one pushed; a range that does not lie above
        everything pushed so far is refused (the indices of one search are distinct and ascend). z: the
        rows' latent vectors, fp32 [n, L] on the device, required exactly when latent_dim was given."""
        if packed.G != self.G:
            raise ValueError(f"push: masks of {packed.G} genes into a search over {self.G}")
        n = packed.n
        base = self.next_index if base_index is None else int(base_index)
        if base < self.next_index:
            raise ValueError(f"push: indices from {base} do not lie above those pushed so far (next: {self.next_index})")
        if base + n > (1 << INDEX_BITS):
            raise ValueError(f"push: indices up to {base + n} do not fit {INDEX_BITS} bits")
        if (z is None) != (self.L is None):
            raise ValueError("push: z is required exactly when the search was built with latent_dim")
        if z is not None:
            if tuple(z.shape) != (n, self.L) or z.dtype != torch.float32 or z.device != packed.bits.device:
                raise ValueError(f"push: z must be a device fp32 [{n}, {self.L}] tensor")
            if z.stride(1) != 1:
                z = z.contiguous()
        for s in range(0, n, self.chunk_max):
            m = min(self.chunk_max, n - s)
            zc = None if z is None else z[s:s + m]
            native.search_push(self._state[self._cur], self._state[1 - self._cur], self._scratch, self._scratch_bytes,
                               packed.bits[s:s + m], m, packed.ld, self.G, zc, 0 if zc is None else zc.stride(0),
                               base + s, self._goff, self.n_groups, self._pos, self.min_groups)
            self._cur = 1 - self._cur
        self.next_index = base + n

    def merge(self, other: "SmallestSearch"):
        """Fold another search's winners, totals and histograms into this one (the reduction of the
        states of several devices). The two must have screened different indices under the same groups
        and bound; `other` is left as it is."""
        if (other.G, other.L, other.min_groups) != (self.G, self.L, self.min_groups) or \
                not np.array_equal(other.group_offsets, self.group_offsets) or \
                not np.array_equal(other.positions, self.positions):
            raise ValueError("merge: the two searches differ in genes, groups, bound or latent size")
        need = native.search_scratch_size(other.K, self.K)
        if need > self._scratch_bytes:
            self._scratch_bytes, self._scratch = need, self._aligned(need)
        native.search_merge(self._state[self._cur], self._state[1 - self._cur], self._scratch, self._scratch_bytes,
                            other._state[other._cur], self.G, self.n_groups)
        self._cur = 1 - self._cur
        self.next_index = max(self.next_index, other.next_index)

    # ---- the state as plain tensors (what a multi-rank run exchanges) ----
    STATE_FIELDS = ("keys", "hashes", "essential", "rows", "z", "count")
    SHARED_FIELDS = ("totals", "size_hist", "ess_hist", "error")

    def state_tensors(self):
        """{name: device tensor} of the current winners (every array `keep` entries long) and totals."""
        out = {k: self._buf[self._cur][k] for k in self.STATE_FIELDS if self._buf[self._cur][k] is not None}
        out.update({k: getattr(self, k) for k in self.SHARED_FIELDS})
        return out

    def load_state_tensors(self, tensors, next_index=0):
        """Overwrite this search's state with the tensors another search's state_tensors() returned."""
        for k, v in tensors.items():
            dst = self._buf[self._cur][k] if k in self.STATE_FIELDS else getattr(self, k)
            dst.copy_(v)
        self.next_index = int(next_index)

    def result(self) -> SearchResult:
        """Wait for the device and return the winners sorted by (size, index). Raises RuntimeError when
        the device raised its error flag (the duplicate table overflowed: results incomplete)."""
        b = self._buf[self._cur]
        if int(self.error.item()) != 0:
            raise RuntimeError("smallest search: the device's duplicate table overflowed; the results are incomplete")
        k = int(b["count"].item())
        keys = b["keys"][:k]
        order = torch.argsort(keys)       # (keys < 2^63: the signed order is the unsigned one)
        keys_h = keys[order].cpu().numpy()
        totals = self.totals.cpu().numpy()
        return SearchResult(indices=keys_h & ((1 << INDEX_BITS) - 1), sizes=keys_h >> INDEX_BITS,
                            essential=b["essential"][:k][order].cpu().numpy().astype(np.int64),
                            masks=PackedMasks(b["rows"][:k][order].contiguous(), self.G),
                            z=None if b["z"] is None else b["z"][:k][order].contiguous(),
                            seen=int(totals[0]), viable=int(totals[1]), size_hist=self.size_hist.cpu().numpy(),
                            ess_hist=self.ess_hist.cpu().numpy())


def search_smallest(model, num_samples, keep, essential_gene_positions, min_essential=None, chunk=65536, z=None,
                    z_center=None, noise_level=None, generator=None, base_index=0, return_search=False):
    """Screen num_samples decoded genomes and keep the `keep` smallest distinct viable ones.

    The reproducibility contract -- once per chunk c of n_c = min(chunk, rows left) genomes, in order:
      1. z_c = z[start : start + n_c]                                          when z is given, else
         z_c = torch.randn(n_c, L, device=model.device, generator=generator)   (one draw per chunk), and
         z_c = z_center + noise_level * z_c                                     when z_center is given;
      2. model.decode_bits(z_c, chunk=chunk) into a chunk buffer that is reused;
      3. push(masks, z_c) with global indices base_index + start ...
    Memory use does not depend on num_samples. Returns the SearchResult (its z: the winners' z_c rows), or
    the SmallestSearch itself with return_search (a multi-rank caller merges before it reads)."""
    N, L, dev = int(num_samples), model.latent_dim, model.device
    if z is not None and (z.dim() != 2 or z.shape[0] != N or z.shape[1] != L):
        raise ValueError(f"search_smallest: z must be [{N}, {L}]")
    if z_center is not None and noise_level is None:
        raise ValueError("search_smallest: z_center needs a noise_level")
    chunk = max(1, min(int(chunk), native.SEARCH_MAX_N))
    search = SmallestSearch(model.input_dim, keep, essential_gene_positions, min_essential, latent_dim=L, device=dev,
                            chunk_max=min(chunk, max(N, 1)))
    buf = PackedMasks.empty(min(chunk, max(N, 1)), model.input_dim, dev)
    search.next_index = int(base_index)
    with torch.no_grad():
        for s in range(0, N, chunk):
            n = min(chunk, N - s)
            if z is not None:
                zc = z[s:s + n].to(dev, torch.float32).contiguous()
            else:
                zc = torch.randn(n, L, device=dev, generator=generator)
                if z_center is not None:
                    zc = z_center + noise_level * zc
            masks, _ = model.decode_bits(zc, chunk=chunk, out=buf)
            search.push(masks, zc)
    return search if return_search else search.result()
