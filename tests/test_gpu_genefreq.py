"""Per-gene counts of packed masks on the GPU (csrc/masks.hip k_gene_counts through
PackedMasks.gene_counts / gene_counts_by) and --mode sample --gene-frequencies end to end. Every
result is an integer and is compared with exact equality against numpy's column sums."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_bitgram import packed, rows01

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the kernel's geometry (csrc/masks.hip kGc*): a wave adds 8-row blocks into its bit-sliced planes and
# spills them every 31 blocks, so P = 248 rows of one wave; the 4 waves of a workgroup interleave
# their blocks, so a wave reaches P when its slab holds 4 P = 992 rows; a slab is at least 1,024 rows
BLOCK, P, WG_STRIDE, SLAB = 8, 248, 32, 1024


def colsum(x):
    return x.sum(axis=0, dtype=np.int64)


def counts_of(p, rows=None, out=None):
    got = p.gene_counts(rows, out)
    assert got.dtype == torch.int64 and tuple(got.shape) == (p.G,)
    return got.cpu().numpy()


SHAPES = [(1, 1), (3, 127), (64, 128), (65, 129), (257, 8191), (300, 8193), (33, 55039), (70000, 700)]


@pytest.mark.parametrize("n,G", SHAPES)
def test_gene_counts_match_column_sums(n, G):
    x = rows01(n, G, seed=n * 7 + G)
    want = colsum(x)
    np.testing.assert_array_equal(counts_of(packed(x)), want)
    if n >= 3:
        assert want.min() >= 1 and want.max() <= n - 1   # the all-one and the all-zero row


FLUSH_ROWS = sorted({254, 255, 256, 257, 511, 512, 513,
                     P - 1, P, P + 1, 4 * P - 1, 4 * P, 4 * P + 1,       # the plane-flush period of one wave / of a slab
                     BLOCK - 1, BLOCK, BLOCK + 1, WG_STRIDE - 1, WG_STRIDE, WG_STRIDE + 1,
                     SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 1})


@pytest.fixture(scope="module")
def dense129():
    """2,049 rows of G = 129, three quarters of them all-one: the counters pass every flush near full."""
    x = rows01(2 * SLAB + 1, 129, seed=5)
    x[np.arange(len(x)) % 4 != 2] = 1
    return x, packed(x)


@pytest.mark.parametrize("n", FLUSH_ROWS)
def test_flush_and_stride_boundaries(dense129, n):
    from gm2 import native
    x, p = dense129
    counts = torch.empty(129, dtype=torch.int64, device="cuda")
    native.mask_gene_counts(p.bits, p.n, p.ld, 129, None, n, counts)   # the first n rows
    np.testing.assert_array_equal(counts.cpu().numpy(), colsum(x[:n]))


def test_all_one_rows_do_not_saturate():
    n, G = 70000, 129
    p = packed(np.ones((n, G), dtype=np.uint8))
    got = counts_of(p)
    assert (got == n).all(), (got.min(), got.max())


@pytest.mark.parametrize("extra", [16, 48])
def test_pitch_pads_are_ignored_and_counts_stay_inside(extra):
    from gm2 import native
    n, G = 65, 129
    x = rows01(n, G, seed=extra)
    p = packed(x, extra_pitch=extra)
    p.bits[:, p.ld - extra:] = 0xFF                    # bytes beyond roundup(G, 128) / 8 are never read
    buf = torch.full((G + 9,), -7, dtype=torch.int64, device="cuda")
    native.mask_gene_counts(p.bits, n, p.ld, G, None, n, buf[3:3 + G])
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[3:3 + G], colsum(x))
    assert (got[:3] == -7).all() and (got[3 + G:] == -7).all()


def test_accumulate_and_overwrite():
    from gm2 import native
    n, G = 300, 8193
    x = rows01(n, G, seed=2)
    p, want = packed(x), colsum(x)
    counts = torch.full((G,), 12345, dtype=torch.int64, device="cuda")
    native.mask_gene_counts(p.bits, n, p.ld, G, None, n, counts)                      # overwrites a dirty vector
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    half = n // 2
    lo, hi = torch.arange(0, half, dtype=torch.int32, device="cuda"), torch.arange(half, n, dtype=torch.int32, device="cuda")
    counts.zero_()
    native.mask_gene_counts(p.bits, n, p.ld, G, lo, half, counts, accumulate=True)    # two disjoint halves into one vector
    native.mask_gene_counts(p.bits, n, p.ld, G, hi, n - half, counts, accumulate=True)
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    native.mask_gene_counts(p.bits, n, p.ld, G, lo, half, counts)                     # overwrite with one half, add the other
    native.mask_gene_counts(p.bits, n, p.ld, G, hi, n - half, counts, accumulate=True)
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    native.mask_gene_counts(p.bits, n, p.ld, G, None, 0, counts, accumulate=True)     # nothing to add
    np.testing.assert_array_equal(counts.cpu().numpy(), want)
    out = p.gene_counts(out=counts)                                                   # out is added to
    assert out is counts
    np.testing.assert_array_equal(counts.cpu().numpy(), 2 * want)
    native.mask_gene_counts(p.bits, n, p.ld, G, None, 0, counts)                      # n = 0 zeroes it
    assert (counts.cpu().numpy() == 0).all()


def test_index_lists():
    n, G = 300, 8193
    x = rows01(n, G, seed=3)
    p = packed(x)
    rng = np.random.Generator(np.random.PCG64(4))
    subset = rng.choice(n, size=77, replace=False)
    np.testing.assert_array_equal(counts_of(p, subset), colsum(x[subset]))
    repeats = np.array([5, 1, 5, 5, 299, 1, 0, 17] * 40)                              # the all-one row 80 times
    np.testing.assert_array_equal(counts_of(p, repeats), colsum(x[repeats]))
    mask = rng.random(n) < 0.4
    np.testing.assert_array_equal(counts_of(p, mask), colsum(x[mask]))
    np.testing.assert_array_equal(counts_of(p, torch.from_numpy(mask).cuda()), colsum(x[mask]))
    np.testing.assert_array_equal(counts_of(p, []), np.zeros(G, dtype=np.int64))
    np.testing.assert_array_equal(counts_of(p, np.zeros(n, dtype=bool)), np.zeros(G, dtype=np.int64))
    np.testing.assert_array_equal(counts_of(p, [n - 1]), x[n - 1].astype(np.int64))
    np.testing.assert_array_equal(counts_of(p, rng.permutation(n)), counts_of(p))
    for bad in ([n], [-1], np.ones(n - 1, dtype=bool), [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            p.gene_counts(bad)
    with pytest.raises(ValueError):
        p.gene_counts(out=torch.zeros(G, dtype=torch.int32, device="cuda"))


def test_index_list_over_many_slabs():
    """An index list longer than one slab, into a matrix of fewer rows than the list."""
    n, G = 50, 700
    x = rows01(n, G, seed=6)
    rows = np.random.Generator(np.random.PCG64(7)).integers(0, n, size=3 * SLAB + 5)
    np.testing.assert_array_equal(counts_of(packed(x), rows), colsum(x[rows]))


def test_gene_counts_by_classes():
    n, G = 257, 8191
    x = rows01(n, G, seed=8)
    labels = np.array(["B2"] * n, dtype=object)
    labels[::3], labels[1::7], labels[100] = "A", "D", "single"        # unbalanced; one class of a single row
    p = packed(x)
    classes, table = p.gene_counts_by(labels)
    assert list(classes) == ["A", "B2", "D", "single"] and table.dtype == np.int64 and table.shape == (4, G)
    for k, c in enumerate(classes):
        np.testing.assert_array_equal(table[k], colsum(x[labels == c]))
    np.testing.assert_array_equal(table.sum(axis=0), counts_of(p))
    with pytest.raises(ValueError):
        p.gene_counts_by(labels[:-1])


def test_from_resident_counts():
    from gm2 import genefreq
    from gm2.data import ResidentMatrix
    from gm2.masks import PackedMasks
    x = rows01(37, 300, seed=9)
    p = PackedMasks.from_resident(ResidentMatrix(x))
    np.testing.assert_array_equal(counts_of(p), colsum(x))
    got = genefreq.gene_counts(p)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64
    np.testing.assert_array_equal(got, colsum(x))


def test_debug_build_counts_and_flags_stay_clear():
    """The same equalities through the GM2_DEBUG library (its index-list check GM2_DBG_GENE_ROWS
    included) with no flag raised, in a child process so that this one keeps the release library."""
    lib = os.path.join(ROOT, "genome-minimizer-2_amd", "gm2", "libgm2_debug.so")
    if not os.path.exists(lib):  # (built best effort by __graft_entry__.build())
        pytest.skip("no libgm2_debug.so: build_native.py --variant debug")
    code = """
import ctypes, json, sys
sys.path[:0] = [%r, %r]
import numpy as np
from gm2 import native
from test_gpu_bitgram import packed, rows01
assert native.LIB_PATH.endswith("libgm2_debug.so"), native.LIB_PATH
ok = True
for n, G in ((3, 127), (65, 129), (300, 8193), (2049, 700)):
    x = rows01(n, G, n + G)
    p = packed(x, 16 if G == 129 else 0)
    rows = np.random.Generator(np.random.PCG64(n)).integers(0, n, size=n + 40)
    labels = np.arange(n) %% 3
    ok = ok and bool((p.gene_counts().cpu().numpy() == x.sum(0, dtype=np.int64)).all())
    ok = ok and bool((p.gene_counts(rows).cpu().numpy() == x[rows].sum(0, dtype=np.int64)).all())
    ok = ok and bool((p.gene_counts_by(labels)[1].sum(0) == x.sum(0, dtype=np.int64)).all())
f = ctypes.c_uint()
assert native.lib().gm2_debug_flags(ctypes.byref(f)) == 0
print("GENEFREQ " + json.dumps({"flags": f.value, "ok": ok}))
""" % (os.path.join(ROOT, "genome-minimizer-2_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GM2_LIB_PATH=lib))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("GENEFREQ ")][-1][len("GENEFREQ "):])
    assert res == {"flags": 0, "ok": True}


def test_cli_sample_gene_frequencies(tmp_path, capsys):
    import pandas as pd

    import main as cli
    from gm2.data import load_and_validate_data, write_synthetic_csvs
    from gm2.model import VAE
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
    freq_csv = os.path.join(out, "v0_gene_frequencies_default.csv")
    base = ["--mode", "sample", "--model-path", ckpt, "--genes-path", pkl, "--num-samples", str(N),
            "--project-root", root, "--mask-dtype", "uint8", "--no-csv"]
    assert cli.main(base) == 0
    assert not os.path.exists(freq_csv)                # off by default
    _, merged, _ = load_and_validate_data(cli.data_paths(root)["Main Dataset"], cli.data_paths(root)["Phylogroups"])
    real = merged.iloc[:, :-1].to_numpy().astype(np.uint8)
    groups = merged.iloc[:, -1].to_numpy()
    classes = sorted(set(groups))
    plain = ["gene", "real_count", "real_freq", "sampled_count", "sampled_freq", "delta"]

    def check(df, masks):
        assert list(df["gene"]) == list(merged.columns[:-1]) and len(df) == G
        np.testing.assert_array_equal(df["sampled_count"], colsum(masks))
        np.testing.assert_array_equal(df["real_count"], colsum(real))
        np.testing.assert_array_equal(df["real_freq"], colsum(real) / len(real))
        np.testing.assert_array_equal(df["sampled_freq"], colsum(masks) / N)
        np.testing.assert_array_equal(df["delta"], df["sampled_freq"] - df["real_freq"])
        for c in classes:
            np.testing.assert_array_equal(df[f"real_{c}"], colsum(real[groups == c]) / (groups == c).sum())

    capsys.readouterr()
    assert cli.main(base + ["--gene-frequencies"]) == 0
    printed = capsys.readouterr().out
    masks = np.load(os.path.join(out, "v0_binary_samples_default.npy"))
    df = pd.read_csv(freq_csv, keep_default_na=False, float_precision="round_trip")
    assert list(df.columns) == plain + [f"real_{c}" for c in classes]
    check(df, masks)
    assert "Gene frequencies, sampled vs real: Pearson r" in printed and freq_csv in printed
    os.remove(freq_csv)
    assert cli.main(base + ["--gene-frequencies", "--nearest-strains"]) == 0
    masks = np.load(os.path.join(out, "v0_binary_samples_default.npy"))
    df = pd.read_csv(freq_csv, keep_default_na=False, float_precision="round_trip")
    check(df, masks)
    d = (masks[:, None, :] != real[None, :, :]).sum(axis=2, dtype=np.int64)
    labels = groups[d.argmin(axis=1)]
    assert list(df.columns) == plain + [f"real_{c}" for c in classes] + [f"sampled_{c}" for c in sorted(set(labels))]
    for c in sorted(set(labels)):
        np.testing.assert_array_equal(df[f"sampled_{c}"], colsum(masks[labels == c]) / (labels == c).sum())
