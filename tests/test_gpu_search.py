"""The streaming smallest-genome search on the GPU (csrc/search.hip through native.search_push /
gm2.search.SmallestSearch / search_smallest) and --mode sample --keep-smallest end to end. Every integer
result is compared with exact equality against gm2.search.smallest_distinct_numpy."""
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
GUARD = -7


def make_groups(G, seed):
    """CSR groups on random columns: single-position groups, multi-position ones, one empty group and two
    groups on the same gene (as many of those as G has columns for)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cols = [int(c) for c in rng.choice(G, size=min(G, 12), replace=False)]
    groups = [[c] for c in cols[:5]]
    if len(cols) >= 9:
        groups += [cols[5:8], [cols[8], cols[0]]]
    if len(cols) >= 12:
        groups += [cols[9:12]]
    groups += [[], [cols[0]]]                       # an empty group; a second group on gene cols[0]
    offs = np.cumsum([0] + [len(g) for g in groups]).astype(np.int32)
    pos = np.array([p for g in groups for p in g], dtype=np.int32)
    return offs, pos


def make_rows(n, G, seed):
    """n rows drawn from a pool of P << n patterns (an all-zero and an all-one pattern among them), a third
    of them with one bit flipped: duplicates, and different rows of equal size, are certain."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P = max(1, n // 8)
    pool = rows01(P, G, seed + 1)
    x = pool[rng.integers(0, P, size=n)].copy()
    for r in range(0, n, 3):
        x[r, rng.integers(0, G)] ^= 1
    return x


def median_bound(x, offs, pos):
    """A viability bound that splits the rows: the median essential count."""
    from gm2.search import essential_counts_numpy
    return int(np.median(essential_counts_numpy(x, offs, pos)))


def guard_of(dtype):
    return GUARD % 256 if str(dtype).endswith("uint8") else GUARD      # (a torch or a numpy dtype)


def guarded(shape, dtype):
    """A device array with one guard element (row) on either side of the part the library is given."""
    t = torch.full((shape[0] + 2,) + tuple(shape[1:]), guard_of(dtype), dtype=dtype, device="cuda")
    return t, t[1:-1]


class RawState:
    """The arrays of a gm2_search_state, each between guard elements, for the C ABI itself."""

    def __init__(self, K, G, n_groups, ld, L=None, shared=None):
        from gm2 import native
        self.full, self.view = {}, {}
        spec = {"keys": ((K,), torch.int64), "hashes": ((K,), torch.int64), "essential": ((K,), torch.int32),
                "rows": ((K, ld), torch.uint8), "count": ((1,), torch.int32)}
        if L is not None:
            spec["z"] = ((K, L), torch.float32)
        if shared is None:
            spec.update({"totals": ((2,), torch.int64), "size_hist": ((G + 1,), torch.int64),
                         "ess_hist": ((n_groups + 1,), torch.int64), "error": ((1,), torch.int32)})
        for k, (shape, dt) in spec.items():
            self.full[k], self.view[k] = guarded(shape, dt)
        if shared is not None:
            for k in ("totals", "size_hist", "ess_hist", "error"):
                self.view[k] = shared.view[k]
        v = self.view
        self.desc = native.search_state(v["keys"], v["hashes"], v["essential"], v["rows"], v.get("z"), v["count"],
                                        v["totals"], v["size_hist"], v["ess_hist"], v["error"])

    def guards_intact(self, count=None):
        for k, t in self.full.items():
            h = t.cpu().numpy()
            g = guard_of(h.dtype)
            assert (h[0] == g).all() and (h[-1] == g).all(), k
            if count is not None and k in ("keys", "hashes", "essential", "rows", "z"):
                assert (h[1 + count:-1] == g).all(), k      # entries beyond the winners are not written


def raw_search(x, offs, pos, K, min_groups, z=None, extra_pitch=0, chunks=None, base=0):
    """gm2_search_init + gm2_search_push (one per chunk) on guarded arrays -> the result as the oracle
    names it, after checking every guard and the entries beyond the count."""
    from gm2 import native
    n, G = x.shape
    p = packed(x, extra_pitch=extra_pitch)
    if extra_pitch:
        p.bits[:, p.ld - extra_pitch:] = 0xFF            # bytes of the pitch beyond the row are never read
    ld = native.packed_row_bytes(G) + extra_pitch
    L = None if z is None else int(z.shape[1])
    ng = len(offs) - 1
    a = RawState(K, G, ng, ld, L)
    b = RawState(K, G, ng, ld, L, shared=a)
    go = torch.from_numpy(offs).cuda()
    po = torch.from_numpy(pos if len(pos) else np.zeros(1, np.int32)).cuda()
    chunks = chunks or [(0, n)]
    nbytes = native.search_scratch_size(max(hi - lo for lo, hi in chunks), K)
    full_scratch = torch.full((nbytes + 1024,), 0x5A, dtype=torch.uint8, device="cuda")
    off = (-full_scratch.data_ptr()) % 256 + 256
    scratch = full_scratch[off: off + nbytes]
    native.search_init(a.desc, G, ng)
    cur, other = a, b
    for lo, hi in chunks:
        zc = None if z is None else z[lo:hi]
        native.search_push(cur.desc, other.desc, scratch, nbytes, p.bits[lo:hi], hi - lo, p.ld, G, zc,
                           0 if zc is None else zc.stride(0), base + lo, go, ng, po, min_groups)
        cur, other = other, cur
    torch.cuda.synchronize()
    count = int(cur.view["count"].item())
    a.guards_intact()
    b.guards_intact()
    cur.guards_intact(count)
    fs = full_scratch.cpu().numpy()
    assert (fs[:off] == 0x5A).all() and (fs[off + nbytes:] == 0x5A).all()
    assert int(cur.view["error"].item()) == 0
    keys = cur.view["keys"][:count].cpu().numpy()
    order = np.argsort(keys, kind="stable")
    rows = cur.view["rows"][:count].cpu().numpy()[order]
    assert (rows[:, native.packed_row_bytes(G):] == GUARD % 256).all()     # only the row's own bytes are written
    totals = cur.view["totals"].cpu().numpy()
    out = {"indices": keys[order] & ((1 << 40) - 1), "sizes": keys[order] >> 40,
           "essential": cur.view["essential"][:count].cpu().numpy()[order].astype(np.int64),
           "rows": np.unpackbits(rows[:, :(G + 7) // 8], axis=1, count=G, bitorder="little"),
           "seen": int(totals[0]), "viable": int(totals[1]), "size_hist": cur.view["size_hist"].cpu().numpy(),
           "ess_hist": cur.view["ess_hist"].cpu().numpy()}
    if z is not None:
        out["z"] = cur.view["z"][:count].cpu().numpy()[order]
    return out


def assert_same(got, want):
    for k in ("indices", "sizes", "essential", "size_hist", "ess_hist"):
        assert got[k].dtype == want[k].dtype == np.int64, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_array_equal(got["rows"], want["rows"])
    assert (got["seen"], got["viable"]) == (want["seen"], want["viable"])


def as_dict(res):
    """A SearchResult as the oracle's dict (+ z on the host)."""
    return {"indices": res.indices, "sizes": res.sizes, "essential": res.essential, "rows": res.masks.unpack(),
            "seen": res.seen, "viable": res.viable, "size_hist": res.size_hist, "ess_hist": res.ess_hist,
            "z": None if res.z is None else res.z.cpu().numpy()}


# the issue's shapes, then one width whose four staged rows no longer fit 64 KB of LDS (the listed groups
# read global memory) and one whose group mask does not fit either (every group read from global memory)
SHAPES = [(1, 1, 1), (5, 127, 3), (300, 129, 7), (1000, 8191, 64), (257, 55039, 16), (2000, 300, 4096),
          (9, 131201, 4), (6, 600001, 3)]


@pytest.mark.parametrize("n,G,K", SHAPES)
def test_single_push_matches_oracle(n, G, K):
    from gm2.search import smallest_distinct_numpy
    x = make_rows(n, G, seed=n + G)
    offs, pos = make_groups(G, seed=G)
    bound = median_bound(x, offs, pos)
    z = torch.randn(n, 5, device="cuda")
    got = raw_search(x, offs, pos, K, bound, z=z, extra_pitch=16 if G == 129 else 0)
    want = smallest_distinct_numpy(x, offs, pos, K, bound)
    assert_same(got, want)
    np.testing.assert_array_equal(got["z"], z.cpu().numpy()[want["indices"]])
    if (n, G, K) == (2000, 300, 4096):       # fewer distinct viable rows than K: the count is their number
        assert 0 < len(got["indices"]) < min(K, want["viable"])
    if n >= 257:                              # the inputs do hold duplicates and ties
        assert want["viable"] > len(smallest_distinct_numpy(x, offs, pos, n, bound)["indices"])
        all_sizes = smallest_distinct_numpy(x, offs, pos, n, bound)["sizes"]
        assert len(np.unique(all_sizes)) < len(all_sizes)


def test_no_groups_and_no_z():
    """n_groups = 0: every row has essential count 0 and is viable at bound 0; a state without z."""
    from gm2.search import smallest_distinct_numpy
    x = make_rows(70, 200, seed=2)
    offs, pos = np.zeros(1, np.int32), np.zeros(0, np.int32)
    assert_same(raw_search(x, offs, pos, 9, 0), smallest_distinct_numpy(x, offs, pos, 9, 0))
    got = raw_search(x, offs, pos, 9, 1)
    assert len(got["indices"]) == 0 and got["viable"] == 0 and got["seen"] == 70


@pytest.fixture(scope="module")
def thousand():
    """1,000 rows of 300 genes, their groups, bound and z, and the oracle's answer for K = 50."""
    from gm2.search import smallest_distinct_numpy
    x = make_rows(1000, 300, seed=11)
    offs, pos = make_groups(300, seed=12)
    bound = median_bound(x, offs, pos)
    z = torch.randn(1000, 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    return x, offs, pos, bound, z, smallest_distinct_numpy(x, offs, pos, 50, bound)


@pytest.mark.parametrize("split", ["one", "ones", "37", "uneven"])
def test_chunk_invariance(thousand, split):
    x, offs, pos, bound, z, want = thousand
    cuts = {"one": [0, 1000], "ones": list(range(1001)), "37": list(range(0, 1000, 37)) + [1000],
            "uneven": [0, 13, 700, 701, 1000]}[split]
    got = raw_search(x, offs, pos, 50, bound, z=z, chunks=list(zip(cuts[:-1], cuts[1:])))
    assert_same(got, want)
    np.testing.assert_array_equal(got["z"], z.cpu().numpy()[want["indices"]])


def new_search(G, K, groups, min_essential=None, L=None, chunk_max=65536):
    from gm2.search import SmallestSearch
    return SmallestSearch(G, K, groups, min_essential=min_essential, latent_dim=L, chunk_max=chunk_max)


def test_carry_over_between_chunks():
    from gm2.search import smallest_distinct_numpy
    G = 40
    groups = (np.array([0, 1, 3], np.int32), np.array([0, 4, 5], np.int32))   # gene 0, and gene 4 or 5

    def row(*cols):
        r = np.zeros(G, np.uint8)
        r[list(cols)] = 1
        return r
    A, B, C = row(0, 4, 9, 10), row(0, 5, 9, 10, 11), row(0, 4, 5, 12, 13, 14)
    first = np.stack([A, B, C, row(1, 2)])                      # (row(1, 2) is not viable)
    later = np.stack([row(0, 4, 20, 21, 22, 23, 24), A, B])     # copies of earlier winners arrive later
    last = np.stack([row(3), row(0, 5), row(0, 4, 30)])         # strictly smaller viable genomes, and a non-viable one
    s = new_search(G, 3, groups)
    assert s.min_groups == 2
    s.push(packed(first))
    r1 = as_dict(s.result())
    assert r1["indices"].tolist() == [0, 1, 2] and r1["sizes"].tolist() == [4, 5, 6]
    s.push(packed(later))
    r2 = as_dict(s.result())
    assert r2["indices"].tolist() == [0, 1, 2]                  # the earlier indices are kept, not 5 and 6
    s.push(packed(last))
    r3 = as_dict(s.result())
    assert r3["indices"].tolist() == [8, 9, 0] and r3["sizes"].tolist() == [2, 3, 4]   # B and C are evicted
    allrows = np.concatenate([first, later, last])
    assert_same(r3, smallest_distinct_numpy(allrows, groups[0], groups[1], 3, 2))
    assert (r3["seen"], r3["viable"]) == (10, 8)
    with pytest.raises(ValueError, match="do not lie above"):
        s.push(packed(last), base_index=9)
    s.push(packed(first), base_index=100)                       # a gap in the indices is fine
    assert as_dict(s.result())["indices"].tolist() == [8, 9, 0] and s.next_index == 104

    # no viable row at all: nothing is kept; with min_essential = 0 every row is viable
    s = new_search(G, 3, groups, min_essential=3)
    s.push(packed(allrows))
    r = s.result()
    assert len(r.indices) == 0 and r.masks.n == 0 and (r.seen, r.viable) == (10, 0) and r.z is None
    s = new_search(G, 20, groups, min_essential=0)
    s.push(packed(allrows))
    r = as_dict(s.result())
    assert r["viable"] == 10
    assert_same(r, smallest_distinct_numpy(allrows, groups[0], groups[1], 20, 0))
    assert len(r["indices"]) == 8                               # 10 rows, A and B twice


def test_push_splits_at_chunk_max(thousand):
    x, offs, pos, bound, z, want = thousand
    s = new_search(300, 50, (offs, pos), min_essential=bound, L=8, chunk_max=128)
    s.push(packed(x), z)
    got = as_dict(s.result())
    assert_same(got, want)
    np.testing.assert_array_equal(got["z"], z.cpu().numpy()[want["indices"]])
    with pytest.raises(ValueError, match="z is required"):
        s.push(packed(x[:3]))


@pytest.mark.parametrize("k_other", [50, 7])
def test_merge_equals_one_state_over_the_concatenation(thousand, k_other):
    from gm2.search import smallest_distinct_numpy
    x, offs, pos, bound, z, want = thousand
    cut = 430
    for into_first in (True, False):
        a = new_search(300, 50 if into_first else k_other, (offs, pos), min_essential=bound, L=8)
        b = new_search(300, k_other if into_first else 50, (offs, pos), min_essential=bound, L=8)
        a.push(packed(x[:cut]), z[:cut])
        b.push(packed(x[cut:]), z[cut:], base_index=cut)
        dst, src = (a, b) if into_first else (b, a)      # (b.merge(a): the lower indices arrive second)
        before = as_dict(src.result())
        dst.merge(src)
        got = as_dict(dst.result())
        if k_other == 50:
            assert_same(got, want)
        else:
            # a source that kept only 7: the best of the destination's 50 and those 7, the totals of all rows
            lo, hi = (0, cut) if into_first else (cut, 1000)
            own = smallest_distinct_numpy(x[lo:hi], offs, pos, 50, bound, indices=np.arange(lo, hi))
            idx = np.concatenate([own["indices"], before["indices"]])
            both = smallest_distinct_numpy(x[idx], offs, pos, 50, bound, indices=idx)
            for k in ("indices", "sizes", "essential", "rows"):
                np.testing.assert_array_equal(got[k], both[k], err_msg=k)
            for k in ("seen", "viable"):
                assert got[k] == want[k]
            for k in ("size_hist", "ess_hist"):
                np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        np.testing.assert_array_equal(got["z"], z.cpu().numpy()[got["indices"]])
        assert_same(as_dict(src.result()), before)       # the source is left as it was


# (columns the fresh model of fresh_model() sets in 60-80 % of its samples, beside some it hardly ever sets)
ESSENTIAL = {"geneA": [0, 5, 20], "geneB": [9], "geneC": [40, 41, 7], "beyond": [5000], "geneB2": [9]}


@pytest.fixture(scope="module")
def fresh_model():
    from gm2.model import VAE
    torch.manual_seed(7)
    m = VAE(700, 1024, 64)
    m.eval()
    return m


def test_search_smallest_given_z(fresh_model):
    from gm2.search import group_tables, search_smallest, smallest_distinct_numpy
    m = fresh_model
    z = torch.randn(512, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    res = search_smallest(m, 512, 16, ESSENTIAL, z=z, chunk=64)
    x = m.decode_bits(z, chunk=64)[0].unpack()
    offs, pos = group_tables(ESSENTIAL, 700)
    want = smallest_distinct_numpy(x, offs, pos, 16, 4)          # (the default bound: the 4 non-empty groups)
    got = as_dict(res)
    assert_same(got, want)
    assert len(got["indices"]) == 16 and 16 < got["viable"] < 512
    np.testing.assert_array_equal(got["z"], z.cpu().numpy()[want["indices"]])


def replay(model, n, chunk, seed, center=None, noise=None):
    """The documented draws of search_smallest: per chunk one torch.randn(n_c, L), scaled around the centre."""
    torch.cuda.manual_seed(seed)
    if center is not None:
        center = center()
    zs, xs = [], []
    for s in range(0, n, chunk):
        zc = torch.randn(min(chunk, n - s), model.latent_dim, device=model.device)
        if center is not None:
            zc = center + noise * zc
        zs.append(zc)
        xs.append(model.decode_bits(zc, chunk=chunk)[0].unpack())
    return torch.cat(zs).cpu().numpy(), np.concatenate(xs)


def test_search_smallest_draws_replay(fresh_model):
    from gm2.search import group_tables, search_smallest, smallest_distinct_numpy
    m = fresh_model
    offs, pos = group_tables(ESSENTIAL, 700)
    torch.cuda.manual_seed(5)
    got = as_dict(search_smallest(m, 512, 16, ESSENTIAL, min_essential=3, chunk=64))
    z, x = replay(m, 512, 64, 5)
    want = smallest_distinct_numpy(x, offs, pos, 16, 3)
    assert_same(got, want)
    np.testing.assert_array_equal(got["z"], z[want["indices"]])
    # around a centre, with a partial last chunk
    c = torch.randn(1, 64, device="cuda")
    torch.cuda.manual_seed(6)
    got = as_dict(search_smallest(m, 200, 16, ESSENTIAL, min_essential=0, chunk=64, z_center=c, noise_level=0.5))
    z, x = replay(m, 200, 64, 6, center=lambda: c, noise=0.5)
    want = smallest_distinct_numpy(x, offs, pos, 16, 0)
    assert_same(got, want)
    np.testing.assert_array_equal(got["z"], z[want["indices"]])


def test_debug_build_checks_stay_clear():
    """The GM2_DEBUG library's checks of the gathered positions, table slots and histogram bins
    (GM2_DBG_MASK_POS) on two shapes with partial chunks, in a child process so that this one keeps the
    release library."""
    lib = os.path.join(ROOT, "genome-minimizer-2_amd", "gm2", "libgm2_debug.so")
    if not os.path.exists(lib):  # (built best effort by __graft_entry__.build())
        pytest.skip("no libgm2_debug.so: build_native.py --variant debug")
    code = """
import ctypes, json, sys
sys.path[:0] = [%r, %r]
import numpy as np
from gm2 import native
from gm2.search import smallest_distinct_numpy
from test_gpu_search import make_groups, make_rows, median_bound, raw_search
ok = True
for n, G, K, cuts in ((70, 129, 7, [0, 5, 70]), (150, 8191, 16, [0, 67, 131, 150])):
    x = make_rows(n, G, 2)
    offs, pos = make_groups(G, 3)
    bound = median_bound(x, offs, pos)
    got = raw_search(x, offs, pos, K, bound, chunks=list(zip(cuts[:-1], cuts[1:])))
    want = smallest_distinct_numpy(x, offs, pos, K, bound)
    ok = ok and all(bool(np.array_equal(got[k], want[k])) for k in want)
f = ctypes.c_uint()
assert native.lib().gm2_debug_flags(ctypes.byref(f)) == 0
print("SEARCH " + json.dumps({"flags": f.value, "ok": ok}))
""" % (os.path.join(ROOT, "genome-minimizer-2_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, GM2_LIB_PATH=lib))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("SEARCH ")][-1][len("SEARCH "):])
    assert res == {"flags": 0, "ok": True}


def test_cli_sample_keep_smallest(tmp_path, capsys):
    import pandas as pd

    import main as cli
    from gm2.data import write_synthetic_csvs
    from gm2.experiments import PRESETS
    from gm2.extras import load_model
    from gm2.model import VAE
    from gm2.search import group_tables, hist_quantiles, smallest_distinct_numpy
    from test_minimizer_cpu import write_genbank
    root = str(tmp_path)
    G, S, N, K, C = 700, 300, 1000, 16, 128
    write_synthetic_csvs(root, S, G, seed=11)
    torch.manual_seed(7)
    ckpt = os.path.join(root, "saved_VAE_v0.pt")
    torch.save(VAE(G, 1024, 64).state_dict(), ckpt)   # the v0 preset's widths, fresh weights
    # essential genes the fresh model sometimes samples and sometimes not: columns set in 30-70 % of a
    # probe decode (another seed than the runs below), so that the bound splits the genomes
    cfg = PRESETS["v0"]()
    torch.cuda.manual_seed(99)
    probe_model = load_model(G, cfg.hidden_dim, cfg.latent_dim, ckpt)
    freq = probe_model.decode_bits(torch.randn(512, cfg.latent_dim, device="cuda"))[0].unpack().mean(axis=0)
    mid = np.flatnonzero((freq > 0.3) & (freq < 0.7))
    assert len(mid) >= 3, "the fresh model has no gene of intermediate frequency"
    pkl = os.path.join(root, "ess.pkl")
    ess = {"geneA": [int(mid[0]), int(mid[1])], "geneB": [int(mid[2])]}
    with open(pkl, "wb") as f:
        pickle.dump(ess, f)
    rng = np.random.default_rng(3)
    seq = "".join(rng.choice(list("ACGT"), size=20000))
    genes = [(f"gene{int(rng.integers(0, G)):05d}", f"{a}..{a + 200}") for a in range(100, 19000, 300)]
    write_genbank(os.path.join(root, "data", "wild_type_sequence.gb"), seq, genes)
    out = os.path.join(root, "models", "v0_model", "sampling_results")
    base = ["--mode", "sample", "--model-path", ckpt, "--genes-path", pkl, "--num-samples", str(N),
            "--project-root", root, "--mask-dtype", "uint8", "--no-csv"]
    flags = ["--keep-smallest", str(K), "--search-chunk", str(C)]
    offs, pos = group_tables(ess, G)
    for mode, M in (("default", 2), ("focused", 1)):
        extra = ["--sampling-mode", mode, "--noise-level", "0.3"] + ([] if M == 2 else ["--min-essential", str(M)])
        torch.cuda.manual_seed(21)
        capsys.readouterr()
        assert cli.main(base + flags + extra) == 0
        printed = capsys.readouterr().out
        model = load_model(G, cfg.hidden_dim, cfg.latent_dim, ckpt)
        center = (lambda: cli.focused_center(model, cfg.latent_dim, model.device)) if mode == "focused" else None
        z, x = replay(model, N, C, 21, center=center, noise=0.3)
        want = smallest_distinct_numpy(x, offs, pos, K, M)
        k = len(want["indices"])
        assert 0 < k <= K and (mode == "focused" or k == K)
        masks = np.load(os.path.join(out, f"v0_smallest_{mode}.npy"))
        assert masks.shape == (k, G) and masks.dtype == np.uint8
        np.testing.assert_array_equal(masks, want["rows"])
        df = pd.read_csv(os.path.join(out, f"v0_smallest_{mode}.csv"))
        assert list(df.columns) == ["rank", "sample", "genome_size", "essential_genes"]
        np.testing.assert_array_equal(df["rank"], np.arange(k))
        np.testing.assert_array_equal(df["sample"], want["indices"])
        np.testing.assert_array_equal(df["genome_size"], want["sizes"])
        np.testing.assert_array_equal(df["essential_genes"], want["essential"])
        zs = np.load(os.path.join(out, f"v0_smallest_z_{mode}.npy"))
        assert zs.shape == (k, cfg.latent_dim) and zs.dtype == np.float32
        np.testing.assert_array_equal(zs, z[want["indices"]])
        assert not os.path.exists(os.path.join(out, f"v0_binary_samples_{mode}.npy"))   # nothing of size N
        sizes = x.sum(axis=1)
        assert hist_quantiles(want["size_hist"]) == (float(np.median(sizes)), sizes.min(), sizes.max())
        assert f"- Screened genomes: {N}\n- Median genome size: {np.median(sizes):.0f} genes\n" \
               f"- Genome size range: {sizes.min():.0f} - {sizes.max():.0f}" in printed
        assert f"- Viable genomes (>= {M} of 2 essential genes): {want['viable']} of {N}" in printed
        assert f"- Kept the {k} smallest distinct viable genomes: {want['sizes'].min()} - {want['sizes'].max()} genes" \
            in printed
    # the consumers run on the K winners
    torch.cuda.manual_seed(21)
    assert cli.main(base + flags + ["--minimized-sizes", "--min-essential", "1"]) == 0
    table = pd.read_csv(os.path.join(out, "v0_minimized_sizes_default.csv"))
    assert len(table) == K
    np.testing.assert_array_equal(table["genome_size"], pd.read_csv(os.path.join(out, "v0_smallest_default.csv"))["genome_size"])
    # without the flag: sample mode as before (one draw of all z, the full-set file)
    torch.cuda.manual_seed(22)
    assert cli.main(base) == 0
    torch.cuda.manual_seed(22)
    model = load_model(G, cfg.hidden_dim, cfg.latent_dim, ckpt)
    zall = torch.randn(N, cfg.latent_dim, device=model.device)
    full = np.load(os.path.join(out, "v0_binary_samples_default.npy"))
    assert full.shape == (N, G)
    np.testing.assert_array_equal(full, model.decode_bits(zall)[0].unpack())
    assert cli.main(base + ["--keep-smallest", "0"]) == 1
