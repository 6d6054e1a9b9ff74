"""CPU-only checks of gm2.minsizes: the feature plan and the numpy statement of the minimized sizes
against the real pipeline (masks_to_gene_lists' first-column rule + check_essential_genes' fill +
GenomeMinimiser on the sequence), the signature's grouping against the minimized strings, the duplicate
stats and report, hand cases, and the plan's refusals."""
import os

import numpy as np
import pytest

from gm2 import minimizer as M
from gm2 import minsizes as S
from test_minimizer_cpu import synth, write_genbank


def pipeline_names(row, cols, essential_set):
    """The gene list of one 0/1 row as masks_to_gene_lists (first occurrence of a duplicated name only,
    binary_converter.py:72-83) and, with an essential set, check_essential_genes build it."""
    cols = np.asarray(cols)
    _, first_idx = np.unique(cols, return_index=True)
    keep = np.zeros(len(cols), dtype=bool)
    keep[np.sort(first_idx)] = True
    names = cols[keep][np.asarray(row)[keep] >= 0.5].tolist()
    if essential_set is not None:
        names = sorted(set(names) | set(essential_set))
    return names


def synth_case(tmp_path, seed, n_rows=24, n_genes=120, L=20000):
    """(record, cols, essentials, rows): a synth record (overlapping, nested, joined, origin-spanning
    genes, genes without /gene) with added duplicate, nested, touching and empty gene features; a column
    list with duplicate names, names of no feature and features of no column; random rows with an
    all-zero, an all-one and two repeated rows."""
    p, seq, genes = synth(str(tmp_path), n_genes=n_genes, L=L, seed=seed)
    extra = [("g3", "100..400"), ("dupA", "100..400"), ("nestA", "150..200"), ("touchA", "1000..1200"),
             ("touchB", "1201..1300"), ("emptyA", "5000^5001"), (None, "7000^7001"), ("g5", "9000..9100")]
    write_genbank(p, seq, genes + extra)
    rec = M.read_genbank(p)
    rng = np.random.default_rng(1000 + seed)
    names = sorted({n for n, _ in genes + extra if n is not None})
    some = [n for n in names if rng.random() < 0.8]            # the rest: features without a column
    cols = some + [f"nofeat{i}" for i in range(15)] + list(rng.choice(some, size=10, replace=False))  # duplicates
    cols = list(rng.permutation(cols))
    essentials = set(rng.choice(names, size=8, replace=False)) | {"not_in_record"}
    G = len(cols)
    rows = (rng.random((n_rows, G)) < rng.random((n_rows, 1))).astype(np.uint8)
    rows[0], rows[1] = 0, 1
    rows[5] = rows[2]                                            # a duplicated row
    rows[7] = rows[2]
    rows[7, [i for i, c in enumerate(cols) if c.startswith("nofeat")]] ^= 1   # differs where no feature listens
    return rec, cols, essentials, rows


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    out = []
    for seed in (0, 1, 2):
        rec, cols, essentials, rows = synth_case(tmp_path_factory.mktemp(f"ms{seed}"), seed)
        for ess in (None, essentials):
            plan = S.FeaturePlan.build(rec, cols, ess)
            gms = [M.GenomeMinimiser(record=rec, needed_genes_list=pipeline_names(r, cols, ess), idx=i, model_name="t")
                   for i, r in enumerate(rows)]
            out.append((rec, cols, ess, rows, plan, gms))
    return out


def test_plan_layout(cases):
    rec, cols, ess, rows, plan, _ = cases[1]
    genes = [f for f in rec.features if f.type == "gene"]
    assert plan.F == len(genes) and plan.L == len(rec.seq) and plan.G == len(cols)
    assert plan.col.dtype == plan.start.dtype == plan.end.dtype == np.int32
    assert (np.diff(plan.start) >= 0).all() and plan.start.min() >= 0 and plan.end.max() <= plan.L
    assert {-1, -2} <= set(plan.col.tolist()) and (plan.col >= 0).any()
    for c in plan.col[plan.col >= 0]:
        assert cols.index(cols[c]) == c          # a first-occurrence column
    assert not (cases[0][4].col == -2).any()     # no essential set: no always-kept feature


def test_numpy_statement_matches_the_minimizer(cases):
    for rec, cols, ess, rows, plan, gms in cases:
        st = S.minimized_stats_numpy(rows, plan)
        assert st["signature"].dtype == np.uint64 and st["removed_bp"].dtype == np.int64
        np.testing.assert_array_equal(st["reduced_length"], [len(g.reduced_genome_str) for g in gms])
        np.testing.assert_array_equal(st["removed_bp"], [g.positions_removed_count for g in gms])
        np.testing.assert_array_equal(st["genes_removed"], [len(g.features) for g in gms])
        np.testing.assert_array_equal(st["reduced_length"], plan.L - st["removed_bp"])
        # (the rows are not all alike, and a small block size gives the same)
        assert len(set(st["reduced_length"].tolist())) > 3
        for k, v in S.minimized_stats_numpy(rows, plan, block=5).items():
            np.testing.assert_array_equal(v, st[k])


def test_signature_groups_like_the_sequences(cases):
    for rec, cols, ess, rows, plan, gms in cases:
        st = S.minimized_stats_numpy(rows, plan)
        seqs = [g.reduced_genome_str for g in gms]
        by_seq, by_sig = {}, {}
        for i, (s, h) in enumerate(zip(seqs, st["signature"].tolist())):
            by_seq.setdefault(s, []).append(i)
            by_sig.setdefault(h, []).append(i)
        assert sorted(by_seq.values()) == sorted(by_sig.values())
        # confirmed when the seeds were chosen: rows 2, 5, 7 are one group, and no two rows with
        # different removed regions give the same string
        assert any({2, 5, 7} <= set(v) for v in by_sig.values())
        regions = {}
        for i, g in enumerate(gms):
            regions.setdefault((tuple(g._rs.tolist()), tuple(g._re.tolist())), []).append(i)
        assert sorted(regions.values()) == sorted(by_seq.values())
        ids = S.sample_ids(len(seqs))
        want = M.check_sequence_duplicates(dict(zip(ids, seqs)))
        got = S.duplicate_stats(st["signature"])
        assert set(got) == set(want)
        for k in want:
            if k != "duplicates_detail":
                assert got[k] == want[k], k
        assert list(got["duplicates_detail"].values()) == list(want["duplicates_detail"].values())
        assert all(isinstance(k, int) for k in got["duplicates_detail"])
        gid, members = S.duplicate_groups(st["signature"])
        assert gid[0] == 0 and (np.diff(np.maximum.accumulate(gid)) <= 1).all()   # dense, by first appearance
        assert sorted(m.tolist() for m in members) == sorted(by_seq.values())


def rec_of(L, feats):
    return M.GenBankRecord("A" * L, [M.Feature("gene", s, e, 1, {"gene": [n]} if n is not None else {})
                                     for n, s, e in feats])


def test_hand_cases():
    mix = lambda v: int(S.mix64(np.array([v], dtype=np.uint64))[0])
    mask = (1 << 64) - 1
    # touching intervals merge into one pair of terms; an interval apart adds its own pair
    plan = S.FeaturePlan.build(rec_of(100, [("a", 10, 20), ("b", 20, 30), ("c", 40, 50)]), ["a", "b", "c", "x"])
    st = S.minimized_stats_numpy(np.array([[0, 0, 1, 1], [0, 0, 0, 0], [1, 0, 0, 0]]), plan)
    assert st["removed_bp"].tolist() == [20, 30, 20] and st["genes_removed"].tolist() == [2, 3, 2]
    assert int(st["signature"][0]) == (mix(2 * 10) + mix(2 * 30 + 1)) & mask
    assert int(st["signature"][1]) == (mix(20) + mix(61) + mix(80) + mix(101)) & mask
    assert int(st["signature"][2]) == (mix(40) + mix(61) + mix(80) + mix(101)) & mask
    # the same regions from other features: the same signature
    other = S.FeaturePlan.build(rec_of(100, [("p", 10, 30), ("q", 12, 25)]), ["z"])
    assert S.minimized_stats_numpy(np.array([[1]]), other)["signature"][0] == st["signature"][0]
    # an empty interval counts as a removed gene, not in the bases nor in the signature -- even inside
    # or right after a removed interval, and with a start beyond every removed end
    plan = S.FeaturePlan.build(rec_of(100, [("a", 10, 20), ("e1", 15, 15), ("e2", 20, 20), ("e3", 60, 60)]), ["a"])
    st = S.minimized_stats_numpy(np.array([[0], [1]]), plan)
    assert st["genes_removed"].tolist() == [4, 3] and st["removed_bp"].tolist() == [10, 0]
    assert int(st["signature"][0]) == (mix(20) + mix(41)) & mask and int(st["signature"][1]) == 0
    # nothing removed: 0 / 0 / 0 (every feature kept by its bit or as an essential; no feature at all)
    plan = S.FeaturePlan.build(rec_of(100, [("a", 10, 20), ("b", 5, 50)]), ["a", "q"], {"b"})
    st = S.minimized_stats_numpy(np.array([[1, 0]]), plan)
    assert (st["removed_bp"][0], st["genes_removed"][0], int(st["signature"][0]), st["reduced_length"][0]) == (0, 0, 0, 100)
    plan = S.FeaturePlan.build(rec_of(100, []), ["a"])
    st = S.minimized_stats_numpy(np.array([[1], [0]]), plan)
    assert plan.F == 0 and st["removed_bp"].tolist() == [0, 0] and st["signature"].tolist() == [0, 0]
    assert S.minimized_stats_numpy(np.zeros((0, 1)), plan)["reduced_length"].shape == (0,)
    # -2 wins over a column; a duplicated name listens to its first column only
    plan = S.FeaturePlan.build(rec_of(100, [("a", 10, 20), ("b", 30, 40)]), ["b", "a", "b"], {"a"})
    assert plan.col.tolist() == [-2, 0]
    assert S.minimized_stats_numpy(np.array([[0, 0, 1]]), plan)["removed_bp"].tolist() == [10]
    # intervals are clipped to the record
    plan = S.FeaturePlan.build(rec_of(50, [("a", 40, 70)]), ["x"])
    assert (plan.start.tolist(), plan.end.tolist()) == ([40], [50])


def test_plan_refusals():
    with pytest.raises(ValueError, match="column"):
        S.FeaturePlan([5], [0], [1], L=10, G=5)
    with pytest.raises(ValueError, match="column"):
        S.FeaturePlan([-3], [0], [1], L=10, G=5)
    S.FeaturePlan([4], [0], [1], L=10, G=5)
    with pytest.raises(ValueError, match="2\\^31"):
        S.FeaturePlan([0], [0], [1], L=2 ** 31, G=5)
    S.FeaturePlan([0], [0], [1], L=2 ** 31 - 1, G=5)

    class Huge:   # a record of 2^31 bases without holding them
        seq, features = range(2 ** 31), []
    with pytest.raises(ValueError, match="2\\^31"):
        S.FeaturePlan.build(Huge(), ["a"])
    with pytest.raises(ValueError, match="sorted"):
        S.FeaturePlan([0, 0], [5, 1], [6, 2], L=10, G=5)
    with pytest.raises(ValueError, match="mask of shape"):
        S.minimized_stats_numpy(np.zeros((2, 4)), S.FeaturePlan([0], [0], [1], L=10, G=5))


def test_export_and_argument_checks():
    """The C entry is exported and bound; its host-side checks answer without a GPU."""
    import ctypes
    from gm2 import native
    lib = native.lib()
    assert "gm2_mask_minimized_stats" in native.EXPORTS and hasattr(lib, "gm2_mask_minimized_stats")
    assert callable(native.mask_minimized_stats)
    buf = (ctypes.c_uint8 * 256)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    p = lambda off=0: ctypes.c_void_p(base + off)

    def call(bits=p(), n=2, ld=16, G=100, col=p(64), start=p(80), end=p(96), F=3, bp=p(128), gone=p(160), sig=p(192)):
        rc = lib.gm2_mask_minimized_stats(bits, n, ld, G, col, start, end, F, bp, gone, sig, None)
        return rc, lib.gm2_last_error().decode()

    for kw, word in ((dict(n=-1), "negative"), (dict(G=0), "G"), (dict(F=-1), "F"), (dict(ld=24), "pitch"),
                     (dict(G=129), "pitch"), (dict(bits=p(8)), "aligned"), (dict(col=p(66)), "aligned"),
                     (dict(bp=p(132)), "aligned"), (dict(gone=p(162)), "aligned"), (dict(col=None), "null"),
                     (dict(sig=None), "null"), (dict(bits=None), "null")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    assert call(n=0)[0] == 0 and call(n=0, F=0, col=None, start=None, end=None)[0] == 0


def test_report(tmp_path, monkeypatch, cases):
    rec, cols, ess, rows, plan, gms = cases[3]
    monkeypatch.setattr(M, "PROJECT_ROOT", str(tmp_path))
    st = S.minimized_stats_numpy(rows, plan)
    dup = S.write_report("minimized_genomes_v9.fasta", "v9", "wild.gb", "masks.npy", plan, st)
    text = open(os.path.join(tmp_path, "minimized_genomes", "minimized_genomes_v9_summary.txt")).read()
    lens = np.array([len(g.reduced_genome_str) for g in gms]) / 1e6
    assert f"Original genome length: {plan.L:,} bp" in text and f"Successfully processed: {len(rows):,}" in text
    assert f"Median size: {np.median(lens):.3f} Mbp ({np.median(lens) * 1e6:,.0f} bp)" in text
    assert f"Unique sequences: {dup['unique_sequences']:,}" in text and f"Duplicate groups: {dup['duplicate_groups']:,}" in text
    table = S.size_table(st, rows.sum(axis=1), plan.L)
    assert list(table.columns) == ["sample", "genome_size", "genes_removed", "reduced_length_bp", "reduction_pct",
                                   "duplicate_group"]
    np.testing.assert_array_equal(table["duplicate_group"], S.duplicate_groups(st["signature"])[0])
