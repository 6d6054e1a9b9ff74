"""CPU-only checks of the gene-major side of the packed masks: the gm2_mask_transpose export and its
host-side argument checks (no GPU call is reached), gm2.linkage (panel selection, phi, summary and
table) against numpy, BinaryPCA's gene side driven by a numpy Gram source against sklearn's full-SVD
PCA, and the CLI flags' defaults."""
import ctypes
import math

import numpy as np
import pytest

from test_bitgram_cpu import check_against_sklearn, clustered, sklearn_reference


def test_export_present():
    from gm2 import native
    lib = native.lib()
    assert "gm2_mask_transpose" in native.EXPORTS
    assert hasattr(lib, "gm2_mask_transpose")
    assert lib.gm2_abi_version() == native.ABI_VERSION == 6
    assert callable(native.mask_transpose)


def test_argument_checks_need_no_gpu():
    from gm2 import native
    lib = native.lib()
    p = ctypes.c_void_p
    bits, out = p(0x10000), p(0x80000)

    def err():
        return lib.gm2_last_error().decode()

    # 4 rows of 100 genes (pitch 16) -> 100 rows of 4 bits (pitch 16): neither pointer is dereferenced
    def tr(bits=bits, n=4, ld_bits=16, G=100, out=out, ld_out=16):
        return lib.gm2_mask_transpose(bits, n, ld_bits, G, out, ld_out, None)

    for kw, word in (({"n": -1}, "negative"), ({"G": 0}, "G"), ({"G": -3}, "G"),
                     ({"ld_bits": 24}, "pitch"), ({"ld_bits": 0}, "pitch"),
                     ({"G": 129}, "pitch"),                     # ld_bits = 16 bytes covers 128 bits only
                     ({"ld_out": 24}, "pitch"), ({"ld_out": 8}, "pitch"), ({"ld_out": 0}, "pitch"),
                     ({"n": 129}, "pitch"),                     # ld_out * 8 = 128 < n
                     ({"bits": p(0x10008)}, "aligned"), ({"out": p(0x80004)}, "aligned"),
                     ({"out": p(0)}, "null"), ({"bits": p(0)}, "null"),
                     ({"out": bits}, "overlap"),
                     ({"out": p(0x10000 + 3 * 16)}, "overlap"),  # out starts on the last input row
                     ({"bits": p(0x80000 + 99 * 16)}, "overlap")):  # bits starts on the last output row
        assert tr(**kw) < 0, kw
        assert word in err(), (kw, err())
    # zero rows: nothing to do, no launch (these pointers were never device memory), even on top of each other
    assert tr(n=0) == 0 and tr(n=0, out=bits) == 0 and tr(n=0, out=p(0)) == 0


def corr_reference(x):
    return np.corrcoef(x.astype(np.float64), rowvar=False)


def test_phi_matrix_matches_corrcoef():
    from gm2.linkage import linkage_summary, phi_matrix
    x, _ = clustered(400, 60, seed=3)
    c = x.sum(axis=0, dtype=np.int64)
    assert ((c > 0) & (c < 400)).all()   # no constant gene: corrcoef is defined everywhere
    both = x.astype(np.int64).T @ x.astype(np.int64)
    phi = phi_matrix(both, c, 400)
    assert phi.dtype == np.float64 and phi.shape == (60, 60)
    dev = np.abs(phi - corr_reference(x)).max()
    print("phi vs corrcoef:", dev)
    assert dev <= 1e-12
    # an all-zero and an all-one column: no correlation is defined, their rows and columns are exactly 0.0
    y = np.concatenate([x, np.zeros((400, 1), np.uint8), np.ones((400, 1), np.uint8)], axis=1)
    both = y.astype(np.int64).T @ y.astype(np.int64)
    phi2 = phi_matrix(both, both.diagonal(), 400)
    assert (phi2[60:] == 0.0).all() and (phi2[:, 60:] == 0.0).all()
    np.testing.assert_array_equal(phi2[:60, :60], phi)
    s = linkage_summary(phi2, phi2)
    assert s["real_constant"] == 2 and s["sampled_constant"] == 2 and s["pairs"] == 62 * 61 // 2
    assert s["max_abs_delta"] == 0.0 and abs(s["pearson_r"] - 1.0) <= 1e-12
    with pytest.raises(ValueError, match="counts"):
        phi_matrix(both, c, 400)


def test_select_panel():
    from gm2.linkage import select_panel
    n = 100
    #               0  1  2   3   4   5   6   7    8  9
    c = np.array([4, 5, 95, 96, 50, 40, 60, 50, 100, 0])
    got = select_panel(c, n)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, [1, 2, 4, 5, 6, 7])          # both bounds inclusive, ascending
    np.testing.assert_array_equal(select_panel(c, n, k=1), [4])     # c (n - c): 50 wins, tie to the lower column
    np.testing.assert_array_equal(select_panel(c, n, k=2), [4, 7])
    np.testing.assert_array_equal(select_panel(c, n, k=3), [4, 5, 7])  # 40 and 60 tie: column 5
    np.testing.assert_array_equal(select_panel(c, n, k=5), [1, 4, 5, 6, 7])    # 5 and 95 tie: column 1
    np.testing.assert_array_equal(select_panel(c, n, lo=0.04, hi=0.96), [0, 1, 2, 3, 4, 5, 6, 7])
    assert len(select_panel(np.array([0, 100, 1]), n)) == 0
    # integer comparison: 3 of 60 is exactly 5 %
    np.testing.assert_array_equal(select_panel(np.array([3, 2, 57, 58]), 60), [0, 2])


def test_linkage_summary_counts():
    from gm2.linkage import linkage_summary

    def sym(u):
        m = np.eye(4)
        m[np.triu_indices(4, 1)] = u
        return m + np.triu(m, 1).T

    #                 (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
    real = sym([0.9, -0.6, 0.5, 0.1, 0.2, -0.7])
    samp = sym([0.3, 0.6, 0.25, 0.6, 0.0, -0.2])
    s = linkage_summary(real, samp)
    d = np.abs(np.array([0.3 - 0.9, 0.6 + 0.6, 0.25 - 0.5, 0.6 - 0.1, 0.0 - 0.2, -0.2 + 0.7]))
    assert s["pairs"] == 6
    assert s["real_strong"] == 4                    # 0.9, -0.6, 0.5 (inclusive), -0.7
    assert s["real_strong_kept"] == 2               # 0.3 and 0.25 (inclusive); 0.6 has the other sign, -0.2 is weak
    assert s["sampled_strong_new"] == 1             # (1,2): 0.1 -> 0.6; (0,2) was strong in the strains
    assert s["real_constant"] == 0 and s["sampled_constant"] == 0
    assert math.isclose(s["mean_abs_delta"], d.mean(), rel_tol=1e-15)
    assert math.isclose(s["max_abs_delta"], 1.2, rel_tol=1e-15)
    r = np.corrcoef(real[np.triu_indices(4, 1)], samp[np.triu_indices(4, 1)])[0, 1]
    assert math.isclose(s["pearson_r"], r, rel_tol=1e-12)
    assert linkage_summary(real, samp, strong=0.8)["real_strong"] == 1
    # one side constant over the pairs: no correlation
    assert math.isnan(linkage_summary(real, sym([0.5] * 6))["pearson_r"])
    assert math.isnan(linkage_summary(np.eye(1), np.eye(1))["pearson_r"])
    with pytest.raises(ValueError, match="shapes"):
        linkage_summary(real, np.eye(3))


def test_linkage_table_rows_and_order():
    from gm2.linkage import linkage_table, phi_matrix
    rng = np.random.Generator(np.random.PCG64(5))
    real = (rng.random((50, 9)) < 0.5).astype(np.int64)
    real[:, 6] = real[:, 2]                       # a perfectly linked pair in the strains
    samp = (rng.random((80, 9)) < 0.4).astype(np.int64)
    samp[:, 7] = 1 - samp[:, 3]                   # a mutually exclusive pair in the samples only
    names = np.array([f"g{i}" for i in range(9)])
    panel = np.array([1, 2, 3, 6, 7])
    br, bs = real[:, panel].T @ real[:, panel], samp[:, panel].T @ samp[:, panel]
    full = linkage_table(names, panel, br, br.diagonal(), 50, bs, bs.diagonal(), 80)
    assert list(full.columns) == ["gene_a", "gene_b", "real_both", "real_phi", "sampled_both", "sampled_phi", "delta"]
    assert len(full) == 10
    pr, ps = phi_matrix(br, br.diagonal(), 50), phi_matrix(bs, bs.diagonal(), 80)
    pairs = [(a, b) for a in range(5) for b in range(a + 1, 5)]
    want = sorted(pairs, key=lambda ab: (-abs(ps[ab] - pr[ab]), panel[ab[0]], panel[ab[1]]))
    assert list(zip(full["gene_a"], full["gene_b"])) == [(names[panel[a]], names[panel[b]]) for a, b in want]
    np.testing.assert_array_equal(full["real_both"], [br[ab] for ab in want])
    np.testing.assert_array_equal(full["sampled_both"], [bs[ab] for ab in want])
    np.testing.assert_array_equal(full["real_phi"], [pr[ab] for ab in want])
    np.testing.assert_array_equal(full["delta"], [ps[ab] - pr[ab] for ab in want])
    assert full["real_phi"][list(zip(full["gene_a"], full["gene_b"])).index(("g2", "g6"))] == 1.0
    assert abs(full["sampled_phi"][list(zip(full["gene_a"], full["gene_b"])).index(("g3", "g7"))] + 1.0) <= 1e-15
    # top = 1: the strongest pair of the strains and the largest change, sorted by |delta|
    top1 = linkage_table(names, panel, br, br.diagonal(), 50, bs, bs.diagonal(), 80, top=1)
    by_real = max(pairs, key=lambda ab: (abs(pr[ab]), -ab[0], -ab[1]))
    keep = sorted({by_real, want[0]}, key=want.index)
    assert list(zip(top1["gene_a"], top1["gene_b"])) == [(names[panel[a]], names[panel[b]]) for a, b in keep]
    assert by_real == (1, 3)                      # g2, g6
    with pytest.raises(ValueError, match="panel"):
        linkage_table(names, panel[:4], br, br.diagonal(), 50, bs, bs.diagonal(), 80)


@pytest.mark.parametrize("n,G", [(700, 129), (1500, 200)])
def test_gene_side_pca_numpy_gram_matches_sklearn(n, G):
    from gm2.pca import BinaryPCA, numpy_gram
    x, fresh = clustered(n, G, seed=1, extra=50)
    ref, scores, fresh_scores = sklearn_reference(x, fresh)
    calls = []

    def gram(a, b=None):
        calls.append((np.asarray(a).shape, b is None))
        return numpy_gram(a, b)

    pca = BinaryPCA(2, gram=gram, side="genes", transform_rows=32)
    got = pca.fit_transform(x)
    got_fresh = pca.transform(fresh)
    check_against_sklearn(pca, got, got_fresh, ref, scores, fresh_scores)
    assert calls == [((G, n), True)] and pca.side_ == "genes"   # the gram source got x.T, once
    # the strains side and the default are today's path
    want = BinaryPCA(2, gram=numpy_gram).fit_transform(x)
    for side in ("strains", "auto"):
        p = BinaryPCA(2, gram=numpy_gram, side=side)
        np.testing.assert_array_equal(p.fit_transform(x), want)
        assert p.side_ == "strains"
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_binary_pca_refuses_a_bad_side():
    from gm2.pca import BinaryPCA
    with pytest.raises(ValueError, match="side"):
        BinaryPCA(2, side="bogus")


def test_cli_flags_default_off():
    import main
    a = main.parse_arguments([])
    assert a.gene_linkage is False and a.linkage_genes == 2048
    a = main.parse_arguments(["--mode", "sample", "--gene-linkage", "--linkage-genes", "64"])
    assert a.gene_linkage is True and a.linkage_genes == 64
