"""CPU-only checks of the streaming smallest-genome search (gm2.h gm2_search_*, gm2/search.py): the
exports, every host-side argument check of the C ABI (each returns < 0 with its message before any GPU
call: this machine has no GPU), the numpy oracle against a brute-force loop, and the min_essential default."""
import ctypes

import numpy as np
import pytest

SEARCH_EXPORTS = ["gm2_search_scratch_size", "gm2_search_init", "gm2_search_push", "gm2_search_merge"]


def test_exports_and_abi_version():
    from gm2 import native
    lib = native.lib()
    for name in SEARCH_EXPORTS:
        assert name in native.EXPORTS
        assert hasattr(lib, name), name
    assert lib.gm2_abi_version() == native.ABI_VERSION == 6
    assert [f[0] for f in native.SearchState._fields_] == ["keys", "hashes", "essential", "rows", "z", "count", "totals",
                                                           "size_hist", "ess_hist", "error", "K", "ld_rows", "L", "ldz"]


def fake_state(base, K=4, ld=16, z=False, L=8):
    """A gm2_search_state of made-up, suitably aligned addresses (never dereferenced on the host)."""
    from gm2 import native
    a = [base + 0x1000 * i for i in range(10)]
    return native.SearchState(a[0], a[1], a[2], a[3], a[4] if z else None, a[5], a[6], a[7], a[8], a[9], K, ld,
                              L if z else 0, L if z else 0)


def push(s_in, s_out, scratch=0x900000, scratch_bytes=1 << 30, bits=0x800000, n=3, ld_bits=16, G=100, z=None, ldz=0,
         base_index=0, goff=0x700000, n_groups=2, pos=0x700100, min_groups=1):
    from gm2 import native
    rc = native.lib().gm2_search_push(ctypes.byref(s_in), ctypes.byref(s_out), scratch, scratch_bytes, bits, n, ld_bits,
                                      G, z, ldz, base_index, goff, n_groups, pos, min_groups, None)
    return rc, native.lib().gm2_last_error().decode()


def test_push_argument_checks_run_on_the_host():
    a, b = fake_state(0x100000), fake_state(0x200000)
    cases = [
        (dict(s_in=fake_state(0x100000, K=0), s_out=fake_state(0x200000, K=0)), "K 0 outside [1, 65536]"),
        (dict(s_in=fake_state(0x100000, K=65537), s_out=fake_state(0x200000, K=65537)), "K 65537 outside [1, 65536]"),
        (dict(G=1 << 23, ld_bits=1 << 20), "G 8388608 outside [1, 2^23)"),
        (dict(G=0), "G 0 outside [1, 2^23)"),
        (dict(ld_bits=24), "pitch of bits (24) must be a multiple of 16 bytes covering G = 100 bits"),
        (dict(G=129, ld_bits=16, s_in=fake_state(0x100000, ld=32), s_out=fake_state(0x200000, ld=32)),
         "pitch of bits (16) must be a multiple of 16 bytes covering G = 129 bits"),
        (dict(G=129, ld_bits=32), "row pitch of state_in (16) must be a multiple of 16 bytes covering G = 129 bits"),
        (dict(bits=0x800008), "rows of bits must be 16-B aligned"),
        (dict(n=-1), "negative row count of bits (-1)"),
        (dict(n=(1 << 20) + 1), "n 1048577 outside [0, 2^20]"),
        (dict(base_index=1 << 40), "base index 1099511627776 outside [0, 2^40 - n]"),
        (dict(base_index=(1 << 40) - 2), "outside [0, 2^40 - n]"),
        (dict(base_index=-1), "base index -1 outside"),
        (dict(goff=None), "null group table with n_groups > 0"),
        (dict(pos=None), "null group table with n_groups > 0"),
        (dict(n_groups=-1), "n_groups -1 outside"),
        (dict(min_groups=-1), "negative min_groups"),
        (dict(bits=None), "null bits"),
        (dict(s_out=a), "two different winner buffers"),
        (dict(s_out=fake_state(0x200000, K=5)), "differ in K, L or in having z"),
        (dict(z=0x600000, ldz=8), "z is required exactly when the state keeps z"),
        (dict(s_in=fake_state(0x100000, z=True), s_out=fake_state(0x200000, z=True)), "z is required exactly when"),
        (dict(s_in=fake_state(0x100000, z=True), s_out=fake_state(0x200000, z=True), z=0x600000, ldz=7), "ldz 7 < L 8"),
        (dict(scratch=0x900010), "scratch must be 256-B aligned"),
        (dict(scratch=None), "scratch must be 256-B aligned"),
        (dict(scratch_bytes=64), "scratch of 64 bytes"),
    ]
    for kw, message in cases:
        args = dict(s_in=a, s_out=b)
        args.update(kw)
        rc, err = push(**args)
        assert rc < 0, (kw, rc)
        assert message in err, (kw, err)
    bad = fake_state(0x100000)
    bad.rows = 0x100008
    rc, err = push(bad, b)
    assert rc < 0 and "rows of state_in must be 16-B aligned" in err
    bad = fake_state(0x200000)
    bad.hashes = None
    rc, err = push(a, bad)
    assert rc < 0 and "state_out has a null array" in err
    # an empty chunk is a no-op that returns 0 and touches nothing (no device here to touch)
    assert push(a, b, n=0)[0] == 0
    assert push(a, b, n=0, bits=None, goff=None, pos=None, n_groups=0)[0] == 0


def test_scratch_size_init_and_merge_checks():
    from gm2 import native
    lib = native.lib()
    nbytes = ctypes.c_size_t()
    for n_max, K, message in ((10, 0, "K 0 outside"), (10, 65537, "K 65537 outside"), (-1, 4, "n_max -1 outside [0, 2^20]"),
                              ((1 << 20) + 1, 4, "outside [0, 2^20]")):
        assert lib.gm2_search_scratch_size(n_max, K, ctypes.byref(nbytes)) < 0
        assert message in lib.gm2_last_error().decode()
    assert lib.gm2_search_scratch_size(10, 4, None) < 0
    sizes = []
    for n_max, K in ((0, 1), (1, 1), (100, 7), (65536, 1024), (1 << 20, 65536)):
        assert lib.gm2_search_scratch_size(n_max, K, ctypes.byref(nbytes)) == 0
        m = n_max + K
        # at least the candidates' keys and slots, the chunk's hashes and counts, the selection list and a
        # duplicate table of >= 2 (K + n) slots of 16 bytes
        assert nbytes.value >= 12 * m + 12 * n_max + 4 * K + 32 * m and nbytes.value % 256 == 0
        sizes.append(nbytes.value)
    assert sizes == sorted(sizes)
    assert native.search_scratch_size(65536, 1024) == sizes[3]
    with pytest.raises(RuntimeError, match="K 0 outside"):
        native.search_scratch_size(10, 0)

    st = fake_state(0x100000, K=0)
    assert lib.gm2_search_init(ctypes.byref(st), 100, 2, None) < 0 and "K 0 outside" in lib.gm2_last_error().decode()
    assert lib.gm2_search_init(None, 100, 2, None) < 0 and "null state" in lib.gm2_last_error().decode()
    st = fake_state(0x100000)
    assert lib.gm2_search_init(ctypes.byref(st), 1 << 23, 2, None) < 0 and "G 8388608" in lib.gm2_last_error().decode()
    assert lib.gm2_search_init(ctypes.byref(st), 129, 2, None) < 0 and "row pitch of state" in lib.gm2_last_error().decode()

    a, b, o = fake_state(0x100000), fake_state(0x200000), fake_state(0x300000, K=9)

    def merge(s_in, s_out, other, scratch=0x900000, scratch_bytes=1 << 30, G=100, n_groups=2):
        rc = lib.gm2_search_merge(ctypes.byref(s_in), ctypes.byref(s_out), scratch, scratch_bytes,
                                  None if other is None else ctypes.byref(other), G, n_groups, None)
        return rc, lib.gm2_last_error().decode()
    for args, message in (((a, a, o), "two different winner buffers"), ((a, b, None), "null other"),
                          ((a, b, fake_state(0x300000, z=True)), "other differs from the state in L or in having z"),
                          ((a, b, fake_state(0x100000)), "other must not share arrays"),
                          ((a, b, fake_state(0x300000, K=70000)), "K 70000 outside"),
                          ((a, b, fake_state(0x300000, ld=0)), "row pitch of other (0)")):
        rc, err = merge(*args)
        assert rc < 0 and message in err, (message, err)
    rc, err = merge(a, b, o, scratch_bytes=128)
    assert rc < 0 and "scratch of 128 bytes" in err
    rc, err = merge(a, b, o, G=1 << 23)
    assert rc < 0 and "G 8388608 outside" in err


def brute_force(x, offs, pos, keep, min_groups, indices=None):
    """The statement of the search as a Python loop over the rows in index order."""
    n, G = x.shape
    idx = list(range(n)) if indices is None else [int(i) for i in indices]
    seen_rows, cands = {}, []
    size_hist, ess_hist, viable = [0] * (G + 1), [0] * len(offs), 0
    for r in sorted(range(n), key=lambda r: idx[r]):
        row = x[r]
        size = int(sum(int(v) for v in row))
        ess = 0
        for g in range(len(offs) - 1):
            if any(row[p] for p in pos[offs[g]:offs[g + 1]]):
                ess += 1
        size_hist[size] += 1
        ess_hist[ess] += 1
        if ess < min_groups:
            continue
        viable += 1
        key = bytes(row.tolist())
        if key in seen_rows:
            continue
        seen_rows[key] = idx[r]
        cands.append((size, idx[r], ess, r))
    cands.sort()
    cands = cands[:keep]
    return {"indices": [c[1] for c in cands], "sizes": [c[0] for c in cands], "essential": [c[2] for c in cands],
            "rows": x[[c[3] for c in cands]] if cands else np.zeros((0, G), np.uint8), "seen": n, "viable": viable,
            "size_hist": size_hist, "ess_hist": ess_hist}


def assert_matches(got, want):
    for k in ("indices", "sizes", "essential", "size_hist", "ess_hist"):
        np.testing.assert_array_equal(got[k], np.asarray(want[k], dtype=np.int64), err_msg=k)
        assert got[k].dtype == np.int64, k
    np.testing.assert_array_equal(got["rows"], want["rows"])
    assert (got["seen"], got["viable"]) == (want["seen"], want["viable"])


def test_oracle_matches_brute_force_with_ties_and_duplicates():
    from gm2.search import smallest_distinct_numpy
    rng = np.random.Generator(np.random.PCG64(5))
    G = 13
    pool = (rng.random((6, G)) < 0.5).astype(np.uint8)
    pool[0] = 0
    x = pool[rng.integers(0, 6, size=60)]
    for r in range(0, 60, 3):                       # single-bit mutations: equal sizes on different rows
        x[r, rng.integers(0, G)] ^= 1
    offs = np.array([0, 1, 3, 3, 4, 5], dtype=np.int32)   # a multi-position group, an empty one, two on gene 2
    pos = np.array([2, 4, 7, 2, 11], dtype=np.int32)
    full = smallest_distinct_numpy(x, offs, pos, 1000, 0)
    assert len(full["indices"]) < 60 and len(set(full["sizes"].tolist())) < len(full["sizes"])   # duplicates, ties
    for keep in (1, 2, 5, 17, 1000):
        for min_groups in (0, 1, 3, 4, 5):
            assert_matches(smallest_distinct_numpy(x, offs, pos, keep, min_groups), brute_force(x, offs, pos, keep, min_groups))
    # global indices that are neither 0-based nor in row order: the lowest index of a genome wins
    idx = rng.permutation(60) * 3 + 1000
    for keep in (3, 40):
        assert_matches(smallest_distinct_numpy(x, offs, pos, keep, 2, indices=idx), brute_force(x, offs, pos, keep, 2, idx))
    # a tie across the cut: the lower index stays
    y = np.array([[1, 1, 0, 0], [1, 0, 1, 0], [0, 1, 1, 0], [1, 1, 0, 0]], dtype=np.uint8)
    got = smallest_distinct_numpy(y, np.array([0], np.int32), np.zeros(0, np.int32), 2, 0)
    assert got["indices"].tolist() == [0, 1] and got["viable"] == 4 and got["ess_hist"].tolist() == [4]
    empty = smallest_distinct_numpy(np.zeros((0, 5), np.uint8), offs[:1], pos[:0], 3, 0)
    assert empty["indices"].shape == (0,) and empty["rows"].shape == (0, 5) and empty["seen"] == 0


def test_min_essential_default_is_the_number_of_non_empty_groups():
    from gm2.search import group_tables, hist_quantiles, resolve_min_essential
    offs, pos = group_tables({"a": [0, 5], "b": [7], "gone": [900], "none": [], "b2": [7]}, 700)
    assert offs.tolist() == [0, 2, 3, 3, 3, 4] and pos.tolist() == [0, 5, 7, 7]
    assert resolve_min_essential(offs) == 3              # "gone" (beyond G) and "none" have no valid position
    assert resolve_min_essential(offs, 0) == 0 and resolve_min_essential(offs, 2) == 2
    assert resolve_min_essential(np.array([0], np.int32)) == 0
    with pytest.raises(ValueError):
        resolve_min_essential(offs, -1)
    o2, p2 = group_tables((offs, pos), 700)
    assert o2.tolist() == offs.tolist() and p2.tolist() == pos.tolist()
    with pytest.raises(ValueError):
        group_tables(([0, 2], [1, 700]), 700)
    # the summary lines' statistics from a histogram = numpy's on the expanded values
    rng = np.random.Generator(np.random.PCG64(1))
    for n in (1, 2, 5, 6, 101):
        v = rng.integers(0, 9, size=n)
        med, lo, hi = hist_quantiles(np.bincount(v, minlength=12))
        assert (med, lo, hi) == (float(np.median(v)), v.min(), v.max())
    assert hist_quantiles(np.zeros(4, np.int64)) is None
