"""CPU-only checks of the bit-row cross products (gm2_mask_cooccur / gm2_mask_nearest) and of
gm2.pca.BinaryPCA: the exports, the host-side argument checks (no GPU call is reached), BinaryPCA
driven by a numpy Gram source against sklearn's full-SVD PCA, and the CLI flags' defaults."""
import ctypes

import numpy as np
import pytest


def test_exports_present():
    from gm2 import native
    lib = native.lib()
    for name in ("gm2_mask_cooccur", "gm2_mask_nearest"):
        assert name in native.EXPORTS
        assert hasattr(lib, name)
    assert lib.gm2_abi_version() == native.ABI_VERSION == 6
    assert callable(native.mask_cooccur) and callable(native.mask_nearest)


def test_argument_checks_need_no_gpu():
    from gm2 import native
    lib = native.lib()
    p = ctypes.c_void_p
    a, b, out = p(0x10000), p(0x20000), p(0x30000)

    def err():
        return lib.gm2_last_error().decode()

    def co(a=a, na=4, lda=16, b=b, nb=5, ldb=32, G=100, out=out, ldo=5):
        return lib.gm2_mask_cooccur(a, na, lda, b, nb, ldb, G, out, ldo, None)

    def nn(q=a, nq=4, ldq=16, ref=b, nr=5, ldr=32, G=100, best=out):
        return lib.gm2_mask_nearest(q, nq, ldq, ref, nr, ldr, G, best, None)

    for call in (co, nn):
        first, second = ("na", "nb") if call is co else ("nq", "nr")
        lda, ldb = ("lda", "ldb") if call is co else ("ldq", "ldr")
        pa, pb = ("a", "b") if call is co else ("q", "ref")
        for kw, word in (({first: -1}, "negative"), ({second: -1}, "negative"), ({"G": 0}, "G"), ({"G": -3}, "G"),
                         ({lda: 24}, "pitch"), ({ldb: 40}, "pitch"), ({lda: 0}, "pitch"),
                         ({"G": 129}, "pitch"),            # lda = 16 bytes covers 128 bits only
                         ({pa: p(0x10008)}, "aligned"), ({pb: p(0x20004)}, "aligned")):
            assert call(**kw) < 0, kw
            assert word in err(), (kw, err())
    assert co(ldo=4) < 0 and "ldo" in err()
    assert nn(nr=0) < 0 and "nr" in err()
    # zero rows: nothing to do, no launch (these pointers were never device memory)
    assert co(na=0) == 0 and co(nb=0, ldo=0) == 0 and co(na=0, nb=0, ldo=0) == 0
    assert nn(nq=0) == 0


def clustered(n, G, seed, extra=0):
    """4 clusters (40 / 30 / 20 / 10 % of the rows: equal sizes give near-equal 2nd and 3rd singular
    values) with per-cluster gene frequencies u^2, u ~ U(0, 1) -> (0/1 u8 [n, G], [extra, G])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = rng.random((4, G)) ** 2
    lab = rng.choice(4, size=n + extra, p=[0.4, 0.3, 0.2, 0.1])
    x = (rng.random((n + extra, G)) < f[lab]).astype(np.uint8)
    return x[:n], x[n:]


def sklearn_reference(x, fresh):
    from sklearn.decomposition import PCA
    ref = PCA(n_components=2, svd_solver="full")
    scores = ref.fit_transform(x.astype(np.float64))
    s = PCA(n_components=3, svd_solver="full").fit(x.astype(np.float64)).singular_values_
    # eigenvectors of near-equal eigenvalues are not comparable: the data must separate PC2 from PC3
    assert (s[1] ** 2 - s[2] ** 2) / s[0] ** 2 >= 0.05, s
    return ref, scores, ref.transform(fresh.astype(np.float64))


def check_against_sklearn(pca, got, got_fresh, ref, scores, fresh_scores):
    bar = 1e-9 * np.abs(scores).max()
    assert np.abs(got - scores).max() <= bar
    assert np.abs(got_fresh - fresh_scores).max() <= 1e-9 * np.abs(fresh_scores).max()
    assert np.abs(pca.explained_variance_ratio_ - ref.explained_variance_ratio_).max() <= 1e-12
    np.testing.assert_allclose(pca.singular_values_, ref.singular_values_, rtol=1e-9)
    np.testing.assert_allclose(pca.explained_variance_, ref.explained_variance_, rtol=1e-9)


PCA_SHAPES = [(64, 129), (130, 700), (200, 8193)]


@pytest.mark.parametrize("n,G", PCA_SHAPES)
def test_binary_pca_numpy_gram_matches_sklearn(n, G):
    from gm2.pca import BinaryPCA, numpy_gram
    x, fresh = clustered(n, G, seed=1, extra=50)
    ref, scores, fresh_scores = sklearn_reference(x, fresh)
    calls = []

    def gram(a, b=None):
        calls.append((len(a), None if b is None else len(b)))
        return numpy_gram(a, b)

    pca = BinaryPCA(n_components=2, gram=gram, transform_rows=32)
    got = pca.fit_transform(x)
    got_fresh = pca.transform(fresh)
    check_against_sklearn(pca, got, got_fresh, ref, scores, fresh_scores)
    assert calls == [(n, None), (32, n), (18, n)]  # the injected source is the only route to the counts
    np.testing.assert_array_equal(BinaryPCA(2, gram=numpy_gram).fit(x).transform(x[:7]).shape, (7, 2))


def test_binary_pca_refuses_bad_sizes():
    from gm2.pca import BinaryPCA, numpy_gram
    x, _ = clustered(5, 3, seed=1)
    with pytest.raises(ValueError, match="n_components"):
        BinaryPCA(n_components=4, gram=numpy_gram).fit(x)
    with pytest.raises(TypeError, match="PackedMasks"):
        BinaryPCA(n_components=2).fit(x)
    pca = BinaryPCA(n_components=2, gram=numpy_gram).fit(x)
    with pytest.raises(ValueError, match="genes"):
        pca.transform(np.zeros((2, 4), dtype=np.uint8))


def test_cli_flags_default_off():
    import main
    a = main.parse_arguments([])
    assert a.nearest_strains is False and a.pca is False
    a = main.parse_arguments(["--mode", "sample", "--nearest-strains", "--pca"])
    assert a.nearest_strains is True and a.pca is True
