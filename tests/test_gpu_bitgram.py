"""The bit-row cross products on the GPU (csrc/masks.hip k_bit_cooccur / k_bit_nearest through
PackedMasks.cooccurrence / nearest), BinaryPCA on the device, and --mode sample --nearest-strains
--pca end to end. Every integer result is compared with exact equality against numpy."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_bitgram_cpu import check_against_sklearn, clustered, sklearn_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows01(n, G, seed):
    """Random 0/1 rows of mixed densities; with >= 3 rows, row 0 is all-zero and row 1 all-one."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.random((n, G)) < rng.random((n, 1))).astype(np.uint8)
    if n >= 3:
        x[0], x[1] = 0, 1
    return x


def packed(x, extra_pitch=0):
    """PackedMasks of host 0/1 rows; extra_pitch > 0: a row pitch that many bytes above the minimum."""
    from gm2 import native
    from gm2.masks import PackedMasks
    p = PackedMasks.from_host(x)
    if extra_pitch:
        wide = torch.zeros(p.n, p.ld + extra_pitch, dtype=torch.uint8, device=p.bits.device)
        wide[:, :p.ld] = p.bits
        p = PackedMasks(wide, p.G)
        assert p.ld == native.packed_row_bytes(p.G) + extra_pitch
    return p


COOCCUR_SHAPES = [(1, 1, 1), (3, 5, 127), (64, 64, 128), (65, 130, 129), (130, 65, 8191), (70, 70, 8193),
                  (33, 257, 55039)]


@pytest.mark.parametrize("na,nb,G", COOCCUR_SHAPES)
def test_cooccurrence_matches_integer_matmul(na, nb, G):
    x = rows01(na, G, seed=na * 1000 + nb)
    same = (na, nb, G) == (70, 70, 8193)   # a is b: the Gram matrix
    y = x if same else rows01(nb, G, seed=G + 7)
    a = packed(x, extra_pitch=16 if G == 129 else 0)
    got = a.cooccurrence(None if same else packed(y))
    assert got.dtype == torch.int32 and tuple(got.shape) == (na, nb)
    want = x.astype(np.int64) @ y.astype(np.int64).T
    np.testing.assert_array_equal(got.cpu().numpy().astype(np.int64), want)
    if na >= 3:
        assert (want[0] == 0).all() and (want[1] == y.sum(axis=1)).all()  # the all-zero and all-one rows


def test_cooccurrence_leaves_pad_columns_and_guard_row():
    from gm2 import native
    na, nb, G = 65, 130, 129
    x, y = rows01(na, G, seed=3), rows01(nb, G, seed=4)
    a, b = packed(x), packed(y, extra_pitch=16)
    ldo = nb + 3
    out = torch.full((na + 1, ldo), -7, dtype=torch.int32, device="cuda")
    native.mask_cooccur(a.bits, na, a.ld, b.bits, nb, b.ld, G, out, ldo)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:na, :nb].astype(np.int64), x.astype(np.int64) @ y.astype(np.int64).T)
    assert (got[:na, nb:] == -7).all() and (got[na] == -7).all()


NEAREST_SHAPES = [(1, 1, 1), (5, 3, 127), (130, 65, 8191), (64, 1000, 700), (300, 7, 55039)]


@pytest.mark.parametrize("nq,nr,G", NEAREST_SHAPES)
def test_nearest_matches_brute_force(nq, nr, G):
    ref = rows01(nr, G, seed=nr * 31 + G)
    if nr >= 3:
        ref[nr - 1] = ref[0]             # exact duplicates (the all-zero row): ties go to the lowest index
    if nr >= 7:
        ref[5] = ref[3]                  # (and a duplicated random row)
    q = rows01(nq, G, seed=nq * 17 + 1)  # (with >= 3 queries, query 0 is all-zero)
    if nq >= 5:
        q[3] = ref[nr // 2]              # queries equal to a reference row: distance 0
        q[4] = ref[min(5, nr - 1)]       # ... to a duplicated one
    ham, idx = packed(q).nearest(packed(ref, extra_pitch=16 if G == 127 else 0))
    assert ham.dtype == np.int64 and idx.dtype == np.int64 and ham.shape == idx.shape == (nq,)
    d = (q[:, None, :] != ref[None, :, :]).sum(axis=2, dtype=np.int64) if nq * nr * G <= 1 << 27 else \
        np.stack([(ref != row).sum(axis=1, dtype=np.int64) for row in q])
    np.testing.assert_array_equal(ham, d.min(axis=1))
    np.testing.assert_array_equal(idx, d.argmin(axis=1))  # (numpy's argmin: the first minimum)
    if nq >= 5 and nr >= 3:
        assert ham[0] == 0 and idx[0] == 0            # the all-zero query: rows 0 and nr - 1 tie
        assert ham[3] == 0 and ham[4] == 0
        assert idx[4] == (3 if nr >= 7 else 0)        # the first of the duplicated rows


def test_from_resident_packs_the_matrix():
    from gm2.data import ResidentMatrix
    from gm2.masks import PackedMasks
    x = rows01(37, 300, seed=9)
    p = PackedMasks.from_resident(ResidentMatrix(x))
    assert (p.n, p.G) == (37, 300)
    np.testing.assert_array_equal(p.unpack(), x)
    np.testing.assert_array_equal(p.cooccurrence().cpu().numpy(), x.astype(np.int64) @ x.astype(np.int64).T)


@pytest.mark.parametrize("n,G", [(130, 700), (200, 8193)])
def test_binary_pca_on_device_matches_sklearn(n, G):
    from gm2.pca import BinaryPCA
    x, fresh = clustered(n, G, seed=1, extra=50)
    ref, scores, fresh_scores = sklearn_reference(x, fresh)
    pca = BinaryPCA(n_components=2, transform_rows=32)
    got = pca.fit_transform(packed(x))
    got_fresh = pca.transform(packed(fresh))
    check_against_sklearn(pca, got, got_fresh, ref, scores, fresh_scores)
    with pytest.raises(ValueError, match="n_components"):
        BinaryPCA(n_components=n + 1).fit(packed(x))


def test_debug_build_index_checks_stay_clear():
    """The GM2_DEBUG library's store-index checks of both kernels (GM2_DBG_BIT_ROWS) on shapes with
    partial tiles, in a child process so that this one keeps the release library."""
    lib = os.path.join(ROOT, "genome-minimizer-2_amd", "gm2", "libgm2_debug.so")
    if not os.path.exists(lib):  # (built best effort by __graft_entry__.build())
        pytest.skip("no libgm2_debug.so: build_native.py --variant debug")
    code = """
import ctypes, json, sys
sys.path[:0] = [%r, %r]
import numpy as np
from gm2 import native
from test_gpu_bitgram import packed, rows01
x, y = rows01(65, 8191, 1), rows01(130, 8191, 2)
c = packed(x).cooccurrence(packed(y, 16)).cpu().numpy()
ham, idx = packed(x).nearest(packed(y))
d = (x[:, None, :] != y[None, :, :]).sum(axis=2)
ok = bool((c == x.astype(np.int64) @ y.astype(np.int64).T).all() and (ham == d.min(1)).all() and (idx == d.argmin(1)).all())
f = ctypes.c_uint()
assert native.lib().gm2_debug_flags(ctypes.byref(f)) == 0
print("BITGRAM " + json.dumps({"flags": f.value, "ok": ok}))
""" % (os.path.join(ROOT, "genome-minimizer-2_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GM2_LIB_PATH=lib))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("BITGRAM ")][-1][len("BITGRAM "):])
    assert res == {"flags": 0, "ok": True}


def test_cli_sample_nearest_strains_and_pca(tmp_path, capsys):
    import pandas as pd

    import main as cli
    from gm2.data import load_and_validate_data, write_synthetic_csvs
    from gm2.masks import PackedMasks
    from gm2.model import VAE
    from gm2.pca import BinaryPCA
    root = str(tmp_path)
    G, S, N = 700, 300, 256
    write_synthetic_csvs(root, S, G, seed=11)
    torch.manual_seed(7)
    ckpt = os.path.join(root, "saved_VAE_v0.pt")
    torch.save(VAE(G, 1024, 64).state_dict(), ckpt)   # the v0 preset's widths, fresh weights
    pkl = os.path.join(root, "ess.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"geneA": [0, 5], "geneB": [7]}, f)
    out = os.path.join(root, "models", "v0_model", "sampling_results")
    near_csv = os.path.join(out, "v0_nearest_strain_default.csv")
    pca_csv = os.path.join(out, "v0_pca_real_vs_sampled_default.csv")
    base = ["--mode", "sample", "--model-path", ckpt, "--genes-path", pkl, "--num-samples", str(N),
            "--project-root", root, "--mask-dtype", "uint8", "--no-csv"]
    assert cli.main(base) == 0
    assert not os.path.exists(near_csv) and not os.path.exists(pca_csv)   # off by default
    capsys.readouterr()
    assert cli.main(base + ["--nearest-strains", "--pca"]) == 0
    printed = capsys.readouterr().out
    masks = np.load(os.path.join(out, "v0_binary_samples_default.npy"))
    assert masks.shape == (N, G) and masks.dtype == np.uint8
    _, merged, _ = load_and_validate_data(cli.data_paths(root)["Main Dataset"], cli.data_paths(root)["Phylogroups"])
    real = merged.iloc[:, :-1].to_numpy().astype(np.uint8)
    # nearest strains: brute force on the saved masks
    d = (masks[:, None, :] != real[None, :, :]).sum(axis=2, dtype=np.int64)
    near = pd.read_csv(near_csv)
    assert list(near.columns) == ["sample", "nearest_strain", "hamming", "genome_size"]
    np.testing.assert_array_equal(near["sample"], np.arange(N))
    np.testing.assert_array_equal(near["hamming"], d.min(axis=1))
    assert list(near["nearest_strain"]) == list(merged.index.to_numpy()[d.argmin(axis=1)])
    np.testing.assert_array_equal(near["genome_size"], masks.sum(axis=1))
    assert f"median {np.median(d.min(axis=1)):.0f}, range {d.min(axis=1).min()} - {d.min(axis=1).max()}" in printed
    assert f"identical to a dataset strain: {int((d.min(axis=1) == 0).sum())}" in printed
    # PCA: the strains' scores, then the samples projected onto the same axes
    df = pd.read_csv(pca_csv, keep_default_na=False)
    assert list(df.columns) == ["PC1", "PC2", "source", "phylogroup"]
    assert list(df["source"]) == ["real"] * len(real) + ["sampled"] * N
    assert list(df["phylogroup"][:len(real)]) == list(merged["Phylogroup"])
    pca = BinaryPCA(n_components=2)
    sc_real = pca.fit_transform(PackedMasks.from_host(real))
    sc = pca.transform(PackedMasks.from_host(masks))
    got = df[["PC1", "PC2"]].to_numpy()
    assert np.abs(got[:len(real)] - sc_real).max() <= 1e-9 * np.abs(sc_real).max()
    assert np.abs(got[len(real):] - sc).max() <= 1e-9 * np.abs(sc).max()
    assert f"PC1 {pca.explained_variance_ratio_[0]:.4f}, PC2 {pca.explained_variance_ratio_[1]:.4f}" in printed
    try:
        import matplotlib  # noqa: F401
        assert os.path.getsize(pca_csv[:-4] + ".pdf") > 0
    except ImportError:
        assert "no PCA scatter plot" in printed
