"""CPU-only checks of the per-gene counts (gm2_mask_gene_counts) and of gm2.genefreq: the export,
the host-side argument checks (no GPU call is reached), the threshold curve against a pandas
restatement of the reference's Figure 1c, the pangenome classes at their cut-offs, the
real-vs-sampled table and its summary on a hand-made case, and the CLI flag's default."""
import ctypes

import numpy as np
import pandas as pd


def test_export_present():
    from gm2 import native
    lib = native.lib()
    assert "gm2_mask_gene_counts" in native.EXPORTS
    assert hasattr(lib, "gm2_mask_gene_counts")
    assert lib.gm2_abi_version() == native.ABI_VERSION == 6
    assert callable(native.mask_gene_counts)


def test_argument_checks_need_no_gpu():
    from gm2 import native
    lib = native.lib()
    p = ctypes.c_void_p
    bits, rows, counts = p(0x10000), p(0x20000), p(0x30000)

    def err():
        return lib.gm2_last_error().decode()

    def gc(bits=bits, n_rows=4, ld=16, G=100, rows=None, n=4, counts=counts, accumulate=0):
        return lib.gm2_mask_gene_counts(bits, n_rows, ld, G, rows, n, counts, accumulate, None)

    for kw, word in (({"n": -1}, "negative"), ({"n_rows": -1, "n": 0}, "negative"),
                     ({"n": 5}, "n_rows"),                      # no index list: n <= n_rows
                     ({"G": 0}, "G"), ({"G": -3}, "G"),
                     ({"ld": 24}, "pitch"), ({"ld": 0}, "pitch"),
                     ({"G": 129}, "pitch"),                     # 16 bytes cover 128 bits only
                     ({"bits": p(0x10008)}, "aligned"), ({"counts": p(0x30004)}, "aligned"),
                     ({"counts": None}, "null"), ({"counts": None, "n": 0, "accumulate": 1}, "null")):
        assert gc(**kw) < 0, kw
        assert word in err(), (kw, err())
    # nothing to add into a kept vector: no device call (these pointers were never device memory)
    assert gc(n=0, accumulate=1) == 0
    assert gc(rows=rows, n=0, accumulate=1) == 0
    assert gc(n_rows=0, n=0, accumulate=1) == 0


def test_gene_counts_of_a_host_array():
    from gm2 import genefreq
    rng = np.random.Generator(np.random.PCG64(0))
    x = (rng.random((37, 301)) < 0.3).astype(np.uint8)
    got = genefreq.gene_counts(x)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, x.sum(axis=0, dtype=np.int64))
    np.testing.assert_array_equal(genefreq.gene_counts(x.astype(float)), got)


def test_threshold_curve_matches_the_reference_loop():
    """explore_data/data_exploration.py:213-220 restated on a genes x samples frame."""
    from gm2 import genefreq
    rng = np.random.Generator(np.random.PCG64(1))
    x = (rng.random((60, 200)) < rng.random((1, 200)) ** 2).astype(np.int64)   # samples x genes, counts 0..60
    x[:, 0], x[:, 1] = 0, 1
    data_without_lineage = pd.DataFrame(x.T, index=[f"g{i}" for i in range(200)])
    thresholds = np.linspace(0, 50, num=50)
    want = []
    for threshold in thresholds:
        gene_frequencies = data_without_lineage.sum(axis=1)
        want.append(len(data_without_lineage[gene_frequencies >= threshold]))
    got = genefreq.threshold_curve(genefreq.gene_counts(x))
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, want)
    assert got[0] == 200 and got[-1] < got[0]
    np.testing.assert_array_equal(genefreq.threshold_curve([0, 3, 3, 7], [0, 3, 3.5, 7, 8]), [4, 3, 1, 1, 0])


def test_pangenome_classes_at_the_cut_offs():
    from gm2 import genefreq
    n = 2000   # 0.99 n = 1980, 0.95 n = 1900, 0.15 n = 300
    counts = [2000, 1980, 1979, 1900, 1899, 300, 299, 0]
    assert genefreq.pangenome_classes(counts, n) == {"core": 2, "soft_core": 2, "shell": 2, "cloud": 2}
    # a set size at which the cut-offs are no integers: 0.99 * 150 = 148.5, 0.95 * 150 = 142.5, 0.15 * 150 = 22.5
    assert genefreq.pangenome_classes([149, 148, 143, 142, 23, 22], 150) == \
        {"core": 1, "soft_core": 2, "shell": 2, "cloud": 1}
    assert genefreq.pangenome_classes([5, 4, 1], 10, core=0.5, soft_core=0.4, shell=0.2) == \
        {"core": 1, "soft_core": 1, "shell": 0, "cloud": 1}
    c = np.arange(0, 1001)
    assert sum(genefreq.pangenome_classes(c, 1000).values()) == len(c)


def test_frequency_table_and_summary():
    from gm2 import genefreq
    names = ["a", "b", "a", "c", "d", "e"]          # a duplicated name keeps both of its columns
    real = np.array([100, 99, 50, 0, 10, 0])        # of 100 strains; c is absent from the real set
    samp = np.array([250, 240, 125, 5, 0, 0])       # of 250 samples; d is never sampled
    real_by = (["A", "B1"], np.array([[60, 60, 20, 0, 10, 0], [40, 39, 30, 0, 0, 0]]), [60, 40])
    t = genefreq.frequency_table(names, real, 100, samp, 250, real_by=real_by)
    assert list(t.columns) == ["gene", "real_count", "real_freq", "sampled_count", "sampled_freq", "delta",
                               "real_A", "real_B1"]
    assert list(t["gene"]) == names
    np.testing.assert_array_equal(t["real_count"], real)
    np.testing.assert_array_equal(t["sampled_count"], samp)
    np.testing.assert_array_equal(t["real_freq"], real / 100)
    np.testing.assert_array_equal(t["sampled_freq"], samp / 250)
    np.testing.assert_array_equal(t["delta"], samp / 250 - real / 100)
    np.testing.assert_array_equal(t["real_A"], real_by[1][0] / 60)
    np.testing.assert_array_equal(t["real_B1"], real_by[1][1] / 40)
    both = genefreq.frequency_table(names, real, 100, samp, 250, real_by, (["A"], samp[None, :], [250]))
    assert list(both.columns)[-3:] == ["real_A", "real_B1", "sampled_A"]
    np.testing.assert_array_equal(both["sampled_A"], samp / 250)
    s = genefreq.frequency_summary(t)
    rf, sf = real / 100, samp / 250
    assert s["genes"] == 6
    assert abs(s["pearson_r"] - np.corrcoef(rf, sf)[0, 1]) <= 1e-15
    assert s["mean_abs_delta"] == np.abs(sf - rf).mean() and s["max_abs_delta"] == np.abs(sf - rf).max()
    # core of the real set: a (1.00) and b (0.99); sampled a = 1.00 stays core, b = 0.96 is soft core only
    assert (s["real_core"], s["real_core_sampled_core"], s["real_core_sampled_soft_core"]) == (2, 1, 2)
    assert s["real_never_sampled"] == 1 and s["sampled_absent_from_real"] == 1
    flat = genefreq.frequency_summary(genefreq.frequency_table(["x", "y"], [1, 1], 2, [0, 3], 3))
    assert np.isnan(flat["pearson_r"])


def test_cli_flag_default_off():
    import main
    assert main.parse_arguments([]).gene_frequencies is False
    assert main.parse_arguments(["--mode", "sample", "--gene-frequencies"]).gene_frequencies is True
