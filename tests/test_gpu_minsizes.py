"""The minimized genome sizes on the GPU (csrc/masks.hip k_minimized_stats through
native.mask_minimized_stats / PackedMasks.minimized_stats) and --mode sample --minimized-sizes end to end.
Every result is compared with exact integer equality against gm2.minsizes.minimized_stats_numpy, one case
against GenomeMinimiser's sequences themselves."""
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


def tricky_plan(F, G, seed):
    """F features sorted by start over G columns: codes -1 / -2 / columns (repeated across features),
    duplicate, nested, equal-start, touching and empty intervals; from 260 features on, feature 1 is
    always removed and ends beyond every start of the next three chunks of 64 (the carry), and the
    whole chunk 2 (features 128..191) is always kept (the carry passes through it)."""
    from gm2.minsizes import FeaturePlan
    rng = np.random.Generator(np.random.PCG64(seed))
    start = np.sort(rng.integers(0, 40 * F + 50, size=F))
    end = start + rng.integers(0, 120, size=F) * (rng.random(F) < 0.9)      # a tenth empty
    col = rng.integers(0, G, size=F)
    code = rng.random(F)
    col[code < 0.15] = -1
    col[code > 0.85] = -2
    for k in range(0, F - 1, 7):
        kind = (k // 7) % 5
        if kind == 0:                                   # a duplicate interval on the same column
            start[k + 1], end[k + 1], col[k + 1] = start[k], end[k], col[k]
        elif kind == 1:                                 # nested, equal start
            start[k + 1], end[k + 1] = start[k], start[k] + (end[k] - start[k]) // 2
        elif kind == 2 and end[k] <= (start[k + 2] if k + 2 < F else end[k]):   # touching
            start[k + 1], end[k + 1] = end[k], end[k] + 30
        elif kind == 3:                                 # empty, inside the one before
            start[k + 1] = end[k + 1] = start[k]
    if F >= 260:
        col[1], end[1] = -1, start[255] + 7
        assert end[1] > start[64:256].max() and start[1] <= start[64]
        col[128:192] = -2
    assert (np.diff(start) >= 0).all()
    return FeaturePlan(col, start, end, int(end.max(initial=0)) + 10, G)


def guarded_call(p, plan):
    """native.mask_minimized_stats into the middle of guard-filled buffers -> the outputs as the numpy
    statement names them; the guard elements on both sides must stay untouched."""
    from gm2 import native
    n = p.n
    bp = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    gone = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
    sig = torch.full((n + 2,), -7, dtype=torch.int64, device="cuda")
    col, start, end = plan.device_tables(p.bits.device) if plan.F else (None, None, None)
    native.mask_minimized_stats(p.bits, n, p.ld, p.G, col, start, end, plan.F, bp[1:], gone[1:], sig[1:])
    bp, gone, sig = bp.cpu().numpy(), gone.cpu().numpy(), sig.cpu().numpy()
    for a in (bp, gone, sig):
        assert a[0] == -7 and a[-1] == -7
    return {"removed_bp": bp[1:-1], "genes_removed": gone[1:-1].astype(np.int64),
            "reduced_length": plan.L - bp[1:-1], "signature": sig[1:-1].view(np.uint64)}


def assert_same(got, want):
    for k in ("removed_bp", "genes_removed", "reduced_length", "signature"):
        assert got[k].dtype == want[k].dtype, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# n around the 4 waves of a workgroup and past its 16 rows; F around the chunk of 64 and the real record's
# 4,600; G around the 128-bit pad unit, several 16-byte pieces per lane (55,039 = the dataset's width), and
# one width whose four rows no longer fit the 64 KB of LDS (the gathers then read global memory)
SHAPES = [(1, 0, 1), (1, 1, 1), (3, 63, 127), (4, 64, 128), (5, 65, 129), (67, 129, 1025), (3, 4600, 55039),
          (67, 4600, 1025), (5, 129, 55039), (4, 1, 55039), (67, 0, 129), (1, 4600, 127), (3, 64, 1), (5, 63, 1025),
          (4, 65, 127), (67, 64, 128), (1, 129, 128), (3, 1, 129), (5, 4600, 128), (4, 129, 1), (3, 65, 131201)]


@pytest.mark.parametrize("n,F,G", SHAPES)
def test_minimized_stats_match_numpy(n, F, G):
    from gm2.minsizes import minimized_stats_numpy
    x = rows01(n, G, seed=n * 31 + F + G)          # (from 3 rows on: an all-zero and an all-one row)
    plan = tricky_plan(F, G, seed=F * 7 + G)
    p = packed(x, extra_pitch=16)
    p.bits[:, p.ld - 16:] = 0xFF                    # bytes of the pitch beyond the row are never read
    want = minimized_stats_numpy(x, plan)
    assert_same(guarded_call(p, plan), want)
    if F >= 65 and n >= 3:
        assert want["genes_removed"][0] > want["genes_removed"][1]      # the rows differ


def test_packed_masks_minimized_stats():
    from gm2.masks import PackedMasks
    from gm2.minsizes import minimized_stats_numpy
    x = rows01(37, 300, seed=9)
    plan = tricky_plan(200, 300, seed=4)
    p = packed(x)
    assert_same(p.minimized_stats(plan), minimized_stats_numpy(x, plan))
    with pytest.raises(ValueError, match="plan of 299"):
        p.minimized_stats(tricky_plan(5, 299, seed=1))
    empty = PackedMasks.empty(0, 300, "cuda").minimized_stats(plan)
    assert_same(empty, minimized_stats_numpy(np.zeros((0, 300), np.uint8), plan))
    assert all(v.shape == (0,) for v in empty.values())


def test_kernel_against_the_minimizer_sequences(tmp_path):
    """The device results against GenomeMinimiser run on the gene lists the pipeline would build: the
    lengths of the minimized strings, the removed positions and features, and the grouping."""
    from gm2 import minimizer as M
    from gm2.minsizes import FeaturePlan, duplicate_groups
    from test_minsizes_cpu import pipeline_names, synth_case
    rec, cols, essentials, rows = synth_case(tmp_path, seed=3)
    for ess in (None, essentials):
        plan = FeaturePlan.build(rec, cols, ess)
        gms = [M.GenomeMinimiser(record=rec, needed_genes_list=pipeline_names(r, cols, ess), idx=i, model_name="t")
               for i, r in enumerate(rows)]
        got = packed(rows).minimized_stats(plan)
        np.testing.assert_array_equal(got["reduced_length"], [len(g.reduced_genome_str) for g in gms])
        np.testing.assert_array_equal(got["removed_bp"], [g.positions_removed_count for g in gms])
        np.testing.assert_array_equal(got["genes_removed"], [len(g.features) for g in gms])
        by_seq = {}
        for i, g in enumerate(gms):
            by_seq.setdefault(g.reduced_genome_str, []).append(i)
        assert sorted(m.tolist() for m in duplicate_groups(got["signature"])[1]) == sorted(by_seq.values())


def test_debug_build_column_checks_stay_clear():
    """The GM2_DEBUG library's checks of every gathered column (GM2_DBG_MASK_POS) on two shapes with
    partial chunks, in a child process so that this one keeps the release library."""
    lib = os.path.join(ROOT, "genome-minimizer-2_amd", "gm2", "libgm2_debug.so")
    if not os.path.exists(lib):  # (built best effort by __graft_entry__.build())
        pytest.skip("no libgm2_debug.so: build_native.py --variant debug")
    code = """
import ctypes, json, sys
sys.path[:0] = [%r, %r]
import numpy as np
from gm2 import native
from gm2.minsizes import minimized_stats_numpy
from test_gpu_minsizes import packed, rows01, tricky_plan
ok = True
for n, F, G in ((5, 65, 129), (18, 300, 8191)):
    x, plan = rows01(n, G, 2), tricky_plan(F, G, 3)
    got, want = packed(x).minimized_stats(plan), minimized_stats_numpy(x, plan)
    ok = ok and all(bool((got[k] == want[k]).all()) for k in want)
f = ctypes.c_uint()
assert native.lib().gm2_debug_flags(ctypes.byref(f)) == 0
print("MINSIZES " + json.dumps({"flags": f.value, "ok": ok}))
""" % (os.path.join(ROOT, "genome-minimizer-2_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GM2_LIB_PATH=lib))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("MINSIZES ")][-1][len("MINSIZES "):])
    assert res == {"flags": 0, "ok": True}


def test_cli_sample_minimized_sizes(tmp_path, capsys):
    import pandas as pd

    import main as cli
    from gm2 import minimizer as M
    from gm2.data import write_synthetic_csvs
    from gm2.minsizes import FeaturePlan, duplicate_stats, minimized_stats_numpy
    from gm2.model import VAE
    from test_minimizer_cpu import write_genbank
    root = str(tmp_path)
    G, S, N = 700, 300, 256
    write_synthetic_csvs(root, S, G, seed=11)
    torch.manual_seed(7)
    ckpt = os.path.join(root, "saved_VAE_v0.pt")
    torch.save(VAE(G, 1024, 64).state_dict(), ckpt)   # the v0 preset's widths, fresh weights
    pkl = os.path.join(root, "ess.pkl")
    with open(pkl, "wb") as f:
        pickle.dump({"geneA": [0, 5], "geneB": [7]}, f)
    # a record of 150 genes: two of three carry a dataset gene's name (some essential), the others a
    # name of no column or none at all
    rng = np.random.default_rng(3)
    L = 30000
    seq = "".join(rng.choice(list("ACGT"), size=L))
    genes = []
    for i in range(150):
        a = int(rng.integers(1, L - 500))
        name = f"gene{int(rng.integers(0, G)):05d}" if i % 3 else (None if i % 2 else f"orf{i}")
        genes.append((name, f"{a}..{a + int(rng.integers(30, 400))}"))
    gb = os.path.join(root, "data", "wild_type_sequence.gb")
    write_genbank(gb, seq, genes)
    out = os.path.join(root, "models", "v0_model", "sampling_results")
    csv = os.path.join(out, "v0_minimized_sizes_default.csv")
    base = ["--mode", "sample", "--model-path", ckpt, "--genes-path", pkl, "--num-samples", str(N),
            "--project-root", root, "--mask-dtype", "uint8", "--no-csv"]
    assert cli.main(base) == 0
    assert not os.path.exists(csv)   # off by default
    large = pd.read_csv(cli.data_paths(root)["Main Dataset"], index_col=0)
    cols = large.drop(index=["Lineage"], errors="ignore").transpose().columns
    essentials = set(pd.read_csv(cli.data_paths(root)["Essential Genes"])["gene"].astype(str).str.strip())
    rec = M.read_genbank(gb)
    for extra, ess in ((["--minimized-sizes"], essentials),
                       (["--minimized-sizes", "--minimized-fill", "none", "--genome-path", gb], None)):
        capsys.readouterr()
        assert cli.main(base + extra) == 0
        printed = capsys.readouterr().out
        masks = np.load(os.path.join(out, "v0_binary_samples_default.npy"))
        assert masks.shape == (N, G)
        plan = FeaturePlan.build(rec, cols, ess)
        want = minimized_stats_numpy(masks, plan)
        df = pd.read_csv(csv)
        assert list(df.columns) == ["sample", "genome_size", "genes_removed", "reduced_length_bp", "reduction_pct",
                                    "duplicate_group"]
        np.testing.assert_array_equal(df["sample"], np.arange(N))
        np.testing.assert_array_equal(df["genome_size"], masks.sum(axis=1))
        np.testing.assert_array_equal(df["genes_removed"], want["genes_removed"])
        np.testing.assert_array_equal(df["reduced_length_bp"], want["reduced_length"])
        pct = (L - want["reduced_length"]) / L * 100.0
        assert np.abs(df["reduction_pct"] - pct).max() <= 1e-9
        first = {}
        gid = [first.setdefault(h, len(first)) for h in want["signature"].tolist()]   # dense, by first appearance
        np.testing.assert_array_equal(df["duplicate_group"], gid)
        red, dup = want["reduced_length"], duplicate_stats(want["signature"])
        assert f"(wild_type_sequence.gb, {L:,} bp, 150 gene features, fill: {'essentials' if ess else 'none'}): median reduced " \
               f"length {np.median(red):.0f} bp, range {red.min()} - {red.max()}" in printed
        assert f"- Mean reduction: {pct.mean():.2f}%" in printed
        assert f"- Unique minimized genomes: {len(first)} of {N}; duplicate groups: {dup['duplicate_groups']}" in printed
        assert f"- Minimized sizes: {csv}" in printed
    # a genome that is not there: the run fails before it writes
    assert cli.main(base + ["--minimized-sizes", "--genome-path", os.path.join(root, "none.gb")]) == 1
