"""PCA of 0/1 rows from their integer co-occurrence counts (the reference's Figure 2a,
explore_data/data_exploration.py:394-420: PCA(n_components=2) of the strains x genes matrix).

For n rows X (0/1, n x G) with n << G the principal axes follow from the n x n Gram matrix
C = X X^T = popcount(x_i AND x_j), which gm2_mask_cooccur computes exactly on the packed rows:

  * Xc = X - 1 mu^T (mu the column means) has Xc Xc^T = K = C - r 1^T - 1 r^T + m, with r the row
    means of C (X mu = C 1 / n) and m its grand mean (mu^T mu = 1^T C 1 / n^2).
  * K = U diag(lambda) U^T. The SVD of Xc is U sqrt(lambda) V^T, so the scores of the fitted rows
    are U sqrt(lambda), singular_values_ = sqrt(lambda), explained_variance_ = lambda / (n - 1) and
    explained_variance_ratio_ = lambda / trace(K) (trace(K) = the total sum of squares of Xc).
  * The axes are v_k = Xc^T u_k / sqrt(lambda_k) = X^T u_k / sqrt(lambda_k): K 1 = 0, so every u_k of
    a non-zero lambda_k has 1^T u_k = 0 and the centring term drops out. They are only needed for
    sklearn's sign convention (svd_flip(u_based_decision=False)): component k is flipped so that the
    largest-magnitude entry of v_k is positive. X^T u is formed in column chunks.
  * Other rows P project as (P - 1 mu^T) V = (P X^T - P mu 1^T - 1 mu^T X^T + mu^T mu 1 1^T) U / sqrt(lambda)
    = (C(P, X) - 1 r^T) U / sqrt(lambda): the two terms with 1^T U vanish, mu^T X^T = r^T. C(P, X) is
    the cross co-occurrence, taken in row chunks so that a million samples never hold an n x S matrix.

For n >> G (a large sampled set) the n x n matrix does not fit and the same axes come from the gene
side (side="genes"): the G x G counts C' = X^T X are the co-occurrence of the transposed packed rows
(PackedMasks.transposed, gm2_mask_transpose: row g = the genomes of gene g), c = diag C' the genes'
counts, and the scatter matrix of the centred data is S = Xc^T Xc = C' - c c^T / n. S = V diag(lambda) V^T
has the same non-zero lambda as K and its eigenvectors are the axes themselves, so the sign rule applies
to V directly and the scores of any rows P are (P - 1 mu^T) V = P V - mu^T V with mu = c / n; P V is
_xt_u of P's transposed rows. side="auto" keeps the strains side whenever its buffers fit.

Everything after the integer counts is fp64 torch on the device the counts live on (the GPU for
PackedMasks, the CPU for a numpy Gram source): the eigenproblem is n x n and not a hot path.
"""
from __future__ import annotations

import numpy as np
import torch

from .masks import PackedMasks


def numpy_gram(a, b=None):
    """The integer counts of host 0/1 arrays: a (a or b)^T in int64."""
    a = np.asarray(a).astype(np.int64)
    return a @ (a if b is None else np.asarray(b).astype(np.int64)).T


def packed_gram(a, b=None):
    """The integer counts of PackedMasks on the device (gm2_mask_cooccur)."""
    return a.cooccurrence(b)


def _shape(x):
    return (x.n, x.G) if isinstance(x, PackedMasks) else tuple(np.asarray(x).shape)


def _rows(x, lo, hi):
    if isinstance(x, PackedMasks):
        return PackedMasks(x.bits[lo:hi], x.G)
    return np.asarray(x)[lo:hi]


def _xt_u(x, u, chunk=1024):
    """X^T u (fp64 [G, k]) in chunks of `chunk` gene columns."""
    n, G = _shape(x)
    out = []
    if isinstance(x, PackedMasks):
        sh = torch.arange(8, device=u.device, dtype=torch.uint8)
        for c0 in range(0, (G + 7) // 8, chunk // 8):
            by = x.bits[:, c0:c0 + chunk // 8]
            cols = ((by.unsqueeze(-1) >> sh) & 1).reshape(n, -1).to(torch.float64)
            out.append(cols.T @ u)
        return torch.cat(out)[:G]
    x = np.asarray(x)
    for c0 in range(0, G, chunk):
        out.append(torch.from_numpy(x[:, c0:c0 + chunk].astype(np.float64)).to(u.device).T @ u)
    return torch.cat(out)


def _transposed(x):
    """The gene-major view: PackedMasks.transposed() on the device, `x.T` of a host array."""
    return x.transposed() if isinstance(x, PackedMasks) else np.ascontiguousarray(np.asarray(x).T)


SIDES = ("auto", "strains", "genes")


class BinaryPCA:
    """PCA(n_components) of 0/1 rows, sklearn's attributes and sign convention, from integer counts.

    side: "strains" fits from the n x n counts of the rows, "genes" from the G x G counts of the
    transposed rows (the same PCA; for n >> G), "auto" the strains side whenever its device buffers fit
    and the genes side only where they do not.

    gram(a, b=None) -> the counts popcount(a_i AND b_j) as an integer array (numpy or torch; b None =
    a with itself) of whatever fit / transform are given: the default takes PackedMasks through
    gm2_mask_cooccur; numpy_gram takes host 0/1 arrays. There is no host fallback for PackedMasks."""

    def __init__(self, n_components=2, gram=None, transform_rows=16384, side="auto"):
        if side not in SIDES:
            raise ValueError(f"BinaryPCA: side={side!r} is not one of {SIDES}")
        self.side = side
        self.n_components = int(n_components)
        self.gram = gram or packed_gram
        self.transform_rows = int(transform_rows)

    def _counts(self, a, b=None):
        if self.gram is packed_gram and not isinstance(a, PackedMasks):
            raise TypeError("BinaryPCA: PackedMasks expected (pass gram=numpy_gram for host 0/1 arrays)")
        c = self.gram(a, b)
        return c if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c))

    def fit(self, x):
        self.fit_transform(x)
        return self

    def fit_transform(self, x):
        n, G = _shape(x)
        k = self.n_components
        if k < 1 or k > min(n, G):
            raise ValueError(f"n_components={k} must be between 1 and min(n_samples, n_features)={min(n, G)}")
        side = "strains" if self.side == "auto" else self.side
        if isinstance(x, PackedMasks) and x.bits.is_cuda:
            # C (int32), K and its eigenvectors (fp64) plus the solver's workspace, all n x n; on the
            # gene side the same G x G, plus the transposed rows
            need, free = 36 * n * n, torch.cuda.mem_get_info(x.bits.device)[0]
            need_g = 36 * G * G + G * ((n + 127) // 128 * 16)
            if self.side == "auto" and need > free:
                side = "genes"
            if side == "strains" and need > free:
                raise MemoryError(f"BinaryPCA: the {n} x {n} int32 and fp64 buffers need {need / 2**30:.1f} GiB, "
                                  f"{free / 2**30:.1f} GiB of device memory are free (side='genes' fits from "
                                  f"the {G} x {G} counts instead)")
            if side == "genes" and need_g > free:
                raise MemoryError(f"BinaryPCA: the {G} x {G} gene-side buffers need {need_g / 2**30:.1f} GiB"
                                  + (f" and the {n} x {n} strain-side buffers {need / 2**30:.1f} GiB"
                                     if self.side == "auto" else "")
                                  + f", {free / 2**30:.1f} GiB of device memory are free")
        self.side_ = side
        if side == "genes":
            return self._fit_genes(x, n, G, k)
        K = self._counts(x).to(torch.float64)
        r = K.mean(dim=1)
        K -= r[:, None]
        K -= r[None, :]
        K += r.mean()
        total = torch.diagonal(K).sum()
        lam, U = torch.linalg.eigh(K)
        lam, U = lam[-k:].flip(0).clamp_min(0.0), U[:, -k:].flip(1)
        v = _xt_u(x, U)
        top = v.abs().argmax(dim=0)
        sign = torch.sign(v[top, torch.arange(k, device=v.device)])
        sign[sign == 0] = 1.0
        self._U = U * sign
        self._sqrt_lam = lam.sqrt()
        self._col_mean = r
        self._fit_x = x
        self.n_samples_, self.n_features_in_ = n, G
        self.singular_values_ = self._sqrt_lam.cpu().numpy()
        self.explained_variance_ = (lam / max(n - 1, 1)).cpu().numpy()
        self.explained_variance_ratio_ = (lam / total).cpu().numpy()
        return (self._U * self._sqrt_lam).cpu().numpy()

    def _fit_genes(self, x, n, G, k):
        xt = _transposed(x)
        S = self._counts(xt).to(torch.float64)
        c = torch.diagonal(S).clone()
        S -= c[:, None] * (c[None, :] / n)
        total = torch.diagonal(S).sum()
        lam, V = torch.linalg.eigh(S)
        lam, V = lam[-k:].flip(0).clamp_min(0.0), V[:, -k:].flip(1)
        top = V.abs().argmax(dim=0)
        sign = torch.sign(V[top, torch.arange(k, device=V.device)])
        sign[sign == 0] = 1.0
        self._V = V * sign
        self._mean_v = (c / n) @ self._V
        self.n_samples_, self.n_features_in_ = n, G
        self.singular_values_ = lam.sqrt().cpu().numpy()
        self.explained_variance_ = (lam / max(n - 1, 1)).cpu().numpy()
        self.explained_variance_ratio_ = (lam / total).cpu().numpy()
        return (_xt_u(xt, self._V) - self._mean_v).cpu().numpy()

    def transform(self, other):
        """Scores of other rows on the fitted axes -> fp64 numpy [rows, n_components]."""
        m, G = _shape(other)
        if G != self.n_features_in_:
            raise ValueError(f"transform: {G} genes, fitted on {self.n_features_in_}")
        if self.side_ == "genes":
            out = np.empty((m, self.n_components), dtype=np.float64)
            for lo in range(0, m, self.transform_rows):
                hi = min(m, lo + self.transform_rows)
                out[lo:hi] = (_xt_u(_transposed(_rows(other, lo, hi)), self._V) - self._mean_v).cpu().numpy()
            return out
        proj = self._U / self._sqrt_lam
        out = np.empty((m, self.n_components), dtype=np.float64)
        for lo in range(0, m, self.transform_rows):
            hi = min(m, lo + self.transform_rows)
            c = self._counts(_rows(other, lo, hi), self._fit_x).to(torch.float64)
            out[lo:hi] = ((c - self._col_mean) @ proj).cpu().numpy()
        return out
