"""The bit transpose of the packed masks on the GPU (csrc/masks.hip k_bit_transpose through
PackedMasks.transposed), the gene x gene counts built on it (PackedMasks.gene_cooccurrence), BinaryPCA's
gene side on the device, and --mode sample --gene-linkage end to end. Every integer result is compared
with exact equality against numpy."""
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_bitgram_cpu import check_against_sklearn, clustered, sklearn_reference
from test_gpu_bitgram import packed, rows01

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows_cols01(n, G, seed):
    """rows01 (an all-zero and an all-one row) with, from 3 genes on, an all-zero column (G // 2) and an
    all-one column (G - 1) laid over them."""
    x = rows01(n, G, seed)
    if G >= 3:
        x[:, G // 2], x[:, G - 1] = 0, 1
    return x


def transpose_reference(x):
    """The packed rows of x.T over the written extent packed_row_bytes(n): bits >= n zero."""
    n = x.shape[0]
    want = np.zeros((x.shape[1], (n + 127) // 128 * 16), dtype=np.uint8)
    want[:, :(n + 7) // 8] = np.packbits(x.T, axis=1, bitorder="little")
    return want


# around the tile (1,024 source rows x 512 genes), the 32 x 32 block of a lane, the 128-bit pad unit;
# several tiles each way; a tall and a wide set
TRANSPOSE_SHAPES = [(1, 1), (7, 9), (8, 8), (63, 127), (64, 128), (65, 129), (127, 1023), (128, 1024), (129, 1025),
                    (255, 2047), (257, 513), (511, 130), (513, 257), (1023, 70), (1025, 1025), (70000, 9),
                    (2100, 55039), (31, 511), (33, 512)]


@pytest.mark.parametrize("n,G", TRANSPOSE_SHAPES)
def test_transposed_matches_numpy(n, G):
    from gm2 import native
    x = rows_cols01(n, G, seed=n * 7 + G)
    t = packed(x).transposed()
    assert (t.n, t.G, t.ld) == (G, n, native.packed_row_bytes(n))
    assert t.bits.dtype == torch.uint8 and t.bits.is_cuda
    np.testing.assert_array_equal(t.bits.cpu().numpy(), transpose_reference(x))


@pytest.mark.parametrize("n,G", [(65, 129), (129, 1025)])
def test_transpose_extents_and_guards(n, G):
    """Only the first roundup(G, 128) / 8 bytes of an input row are read; exactly packed_row_bytes(n)
    bytes of each of the G output rows are written."""
    from gm2 import native
    x = rows_cols01(n, G, seed=5)
    p = packed(x, extra_pitch=16)
    p.bits[:, p.ld - 16:] = 0xFF
    ob = native.packed_row_bytes(n)
    out = torch.full((G + 1, ob + 16), 0xA5, dtype=torch.uint8, device="cuda")
    native.mask_transpose(p.bits, n, p.ld, G, out, ob + 16)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:G, :ob], transpose_reference(x))   # (bits >= n inside the extent: 0)
    assert (got[:G, ob:] == 0xA5).all() and (got[G] == 0xA5).all()


@pytest.mark.parametrize("n,G", [(65, 129), (1025, 1025)])
def test_transpose_round_trip(n, G):
    from gm2 import native
    p = packed(rows_cols01(n, G, seed=8))
    back = p.transposed().transposed()
    assert (back.n, back.G) == (n, G)
    ld = native.packed_row_bytes(G)
    assert torch.equal(back.bits[:, :ld], p.bits[:, :ld])


def test_transposed_refuses_an_empty_set():
    from gm2.masks import PackedMasks
    with pytest.raises(ValueError, match="n = 0"):
        PackedMasks.empty(0, 100, "cuda").transposed()


def test_gene_cooccurrence_matches_integer_matmul():
    n, G = 300, 257
    x = rows_cols01(n, G, seed=21)
    p = packed(x)
    xi = x.astype(np.int64)
    full = p.gene_cooccurrence()
    assert full.dtype == torch.int32 and tuple(full.shape) == (G, G) and full.is_cuda
    np.testing.assert_array_equal(full.cpu().numpy().astype(np.int64), xi.T @ xi)
    assert torch.equal(torch.diagonal(full).to(torch.int64), p.gene_counts())
    # a panel with a repeated index against another list
    a, b = np.array([5, 256, 5, 0, 128]), np.array([255, 256, 1])
    want = xi[:, a].T @ xi[:, b]
    got = p.gene_cooccurrence(a, b)
    assert tuple(got.shape) == (5, 3)
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int64), want)
    np.testing.assert_array_equal(p.gene_cooccurrence(a).cpu().numpy().astype(np.int64), xi[:, a].T @ xi[:, a])
    np.testing.assert_array_equal(p.gene_cooccurrence(None, b).cpu().numpy().astype(np.int64), xi.T @ xi[:, b])
    # the caller's transposed set
    t = p.transposed()
    assert torch.equal(p.gene_cooccurrence(a, b, transposed=t), got)
    assert torch.equal(p.gene_cooccurrence(torch.from_numpy(a).cuda(), b, transposed=t), got)
    for bad in ([0, G], [-1], [[1, 2]], [0.5]):
        with pytest.raises(ValueError, match="gene"):
            p.gene_cooccurrence(np.array(bad), transposed=t)
    with pytest.raises(ValueError, match="transposed"):
        p.gene_cooccurrence(a, transposed=p)


def test_debug_build_store_checks_stay_clear():
    """The GM2_DEBUG library's store-index checks of k_bit_transpose (GM2_DBG_TRANSPOSE) on shapes with
    partial tiles each way, in a child process so that this one keeps the release library."""
    lib = os.path.join(ROOT, "genome-minimizer-2_amd", "gm2", "libgm2_debug.so")
    if not os.path.exists(lib):  # (built best effort by __graft_entry__.build())
        pytest.skip("no libgm2_debug.so: build_native.py --variant debug")
    code = """
import ctypes, json, sys
sys.path[:0] = [%r, %r]
import numpy as np
from gm2 import native
from test_gpu_transpose import packed, rows_cols01, transpose_reference
ok = True
for n, G in ((65, 8191), (1025, 129)):
    x = rows_cols01(n, G, 1)
    ok = ok and bool((packed(x).transposed().bits.cpu().numpy() == transpose_reference(x)).all())
f = ctypes.c_uint()
assert native.lib().gm2_debug_flags(ctypes.byref(f)) == 0
print("TRANSPOSE " + json.dumps({"flags": f.value, "ok": ok}))
""" % (os.path.join(ROOT, "genome-minimizer-2_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GM2_LIB_PATH=lib))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TRANSPOSE ")][-1][len("TRANSPOSE "):])
    assert res == {"flags": 0, "ok": True}


def test_gene_side_pca_on_device_matches_sklearn():
    from gm2.pca import BinaryPCA
    x, fresh = clustered(700, 129, seed=1, extra=50)
    ref, scores, fresh_scores = sklearn_reference(x, fresh)
    pca = BinaryPCA(2, side="genes", transform_rows=32)
    got = pca.fit_transform(packed(x))
    got_fresh = pca.transform(packed(fresh))
    assert pca.side_ == "genes"
    check_against_sklearn(pca, got, got_fresh, ref, scores, fresh_scores)
    auto = BinaryPCA(2)
    auto.fit(packed(x))
    assert auto.side_ == "strains"   # its buffers fit: the default is unchanged


def brute_phi(x):
    """corrcoef of the columns of a 0/1 matrix, 0.0 where a column is constant."""
    c = x.sum(axis=0)
    live = (c > 0) & (c < len(x))
    phi = np.zeros((x.shape[1], x.shape[1]))
    phi[np.ix_(live, live)] = np.corrcoef(x[:, live].astype(np.float64), rowvar=False)
    return phi


def test_cli_sample_gene_linkage(tmp_path, capsys):
    import pandas as pd

    import main as cli
    from gm2.data import load_and_validate_data, write_synthetic_csvs
    from gm2.model import VAE
    root = str(tmp_path)
    G, S, N, K = 700, 300, 256, 64
    write_synthetic_csvs(root, S, G, seed=11)
    torch.manual_seed(7)
    ckpt = os.path.join(root, "saved_VAE_v0.pt")
    torch.save(VAE(G, 1024, 64).state_dict(), ckpt)   # the v0 preset's widths, fresh weights
    pkl = os.path.join(root, "ess.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"geneA": [0, 5], "geneB": [7]}, f)
    out = os.path.join(root, "models", "v0_model", "sampling_results")
    csv = os.path.join(out, "v0_gene_linkage_default.csv")
    base = ["--mode", "sample", "--model-path", ckpt, "--genes-path", pkl, "--num-samples", str(N),
            "--project-root", root, "--mask-dtype", "uint8", "--no-csv"]
    assert cli.main(base) == 0
    assert not os.path.exists(csv)   # off by default
    capsys.readouterr()
    assert cli.main(base + ["--gene-linkage", "--linkage-genes", str(K)]) == 0
    printed = capsys.readouterr().out
    masks = np.load(os.path.join(out, "v0_binary_samples_default.npy")).astype(np.int64)
    assert masks.shape == (N, G)
    _, merged, _ = load_and_validate_data(cli.data_paths(root)["Main Dataset"], cli.data_paths(root)["Phylogroups"])
    real = merged.iloc[:, :-1].to_numpy().astype(np.int64)
    names = merged.columns[:-1].to_numpy()
    # the panel by brute force: 5 % <= f <= 95 % of the strains, the K of largest c (S - c), ties to the lower column
    c = real.sum(axis=0)
    ok = [g for g in range(G) if 20 * c[g] >= S and 20 * c[g] <= 19 * S]
    assert len(ok) >= K   # (145 qualify: the panel is full)
    panel = sorted(sorted(ok, key=lambda g: (-c[g] * (S - c[g]), g))[:K])
    br, bs = real[:, panel].T @ real[:, panel], masks[:, panel].T @ masks[:, panel]
    pr, ps = brute_phi(real[:, panel]), brute_phi(masks[:, panel])
    where = {names[g]: k for k, g in enumerate(panel)}
    df = pd.read_csv(csv)
    assert list(df.columns) == ["gene_a", "gene_b", "real_both", "real_phi", "sampled_both", "sampled_phi", "delta"]
    a = np.array([where[g] for g in df["gene_a"]])
    b = np.array([where[g] for g in df["gene_b"]])
    assert (a < b).all() and len(set(zip(a, b))) == len(df)
    np.testing.assert_array_equal(df["real_both"], br[a, b])           # counts: exact
    np.testing.assert_array_equal(df["sampled_both"], bs[a, b])
    assert np.abs(df["real_phi"] - pr[a, b]).max() <= 1e-12
    assert np.abs(df["sampled_phi"] - ps[a, b]).max() <= 1e-12
    assert np.abs(df["delta"] - (ps[a, b] - pr[a, b])).max() <= 1e-12
    # the rows: the union of the 1,000 pairs of largest |real_phi| and of largest |delta| (of 2,016), by
    # |delta| descending; a pair within 1e-12 of a cut may fall on either side
    ia, ib = np.triu_indices(K, 1)
    absr, absd = np.abs(pr[ia, ib]), np.abs(ps[ia, ib] - pr[ia, ib])
    cut_r, cut_d = np.sort(absr)[-1000], np.sort(absd)[-1000]
    got = set(zip(a, b))
    must = {(i, j) for i, j, r, d in zip(ia, ib, absr, absd) if r > cut_r + 1e-12 or d > cut_d + 1e-12}
    may = {(i, j) for i, j, r, d in zip(ia, ib, absr, absd) if r >= cut_r - 1e-12 or d >= cut_d - 1e-12}
    assert must <= got <= may and 1000 <= len(df) <= 2000
    dd = np.abs(df["delta"].to_numpy())
    assert (np.diff(dd) <= 1e-12).all()
    tie = np.flatnonzero(np.diff(dd) == 0)
    assert all((a[i], b[i]) < (a[i + 1], b[i + 1]) for i in tie)   # equal |delta|: by (column a, column b)
    # the printed summary
    r, s = pr[ia, ib], ps[ia, ib]
    line = [ln for ln in printed.splitlines() if ln.startswith("- Gene linkage, sampled vs real")][0]
    assert f"{K} genes, {K * (K - 1) // 2} pairs" in line
    m = re.search(r"Pearson r (\S+), \|delta phi\| mean (\S+), max (\S+)$", line)
    want_r = np.corrcoef(r, s)[0, 1] if r.std() > 0 and s.std() > 0 else float("nan")
    assert m.group(1) == f"{want_r:.4f}" and m.group(2) == f"{absd.mean():.4f}" and m.group(3) == f"{absd.max():.4f}"
    strong = np.abs(r) >= 0.5
    kept = strong & (np.sign(r) == np.sign(s)) & (np.abs(s) >= 0.25)
    new = (np.abs(s) >= 0.5) & (np.abs(r) < 0.25)
    assert f"(|phi| >= 0.5): {int(strong.sum())}; kept in the samples: {int(kept.sum())}; " \
           f"strong in the samples only: {int(new.sum())}" in printed
    cs = masks[:, panel].sum(axis=0)
    assert f"constant in the samples: {int(((cs == 0) | (cs == N)).sum())}" in printed
    assert f"- Gene linkage: {csv}" in printed
