"""The 256x256 ping-pong GEMM with an MN-major B operand (layouts nn and tn), pinned exactly.

Its operand staging forms every source address as a block-uniform base plus one 32-bit offset per
thread (pp::stage_half), and its epilogue turns (wave, fragment, lane) into a tile column; a slip in
either moves whole columns or k-rows. Exact checks through gm2_gemm in bf16, at the smallest shapes
that take the 256x256 plan (Mp, Np multiples of 256, K >= 8192, plan_gemm_dims):

  * small-integer operands: every partial sum is an integer below 2^24, so fp32 accumulation and
    the split-K slab sum are exact in any order and C must EQUAL the int64 reference;
  * an identity Q: C must equal P[:, :N], so a wrong map shows as the column it moved;
  * a row pitch the 32-bit thread offsets cannot span is refused before any launch.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gm2 import native

LAYOUTS = {"nn": (True, False), "tn": (False, False)}  # (P K-major, Q K-major); Q MN-major in both


@pytest.fixture
def pingpong():
    old = native.get_option(native.OPT_GEMM_PP)
    native.set_option(native.OPT_GEMM_PP, 1)
    yield
    native.set_option(native.OPT_GEMM_PP, old)


def _run(P, Q, M, N, K, layout, splits):
    """C [M][N] (ldc = N) = P[:M] . Q[:N]^T on the device; P [Mp][K], Q [Np][K] fp32 on the CPU, exact in
    bf16, rows past M / N zero. Stored K-major as given, MN-major as the transpose."""
    pk, qk = LAYOUTS[layout]
    Ps = (P if pk else P.T.contiguous()).bfloat16().cuda()
    Qs = (Q if qk else Q.T.contiguous()).bfloat16().cuda()
    C = torch.full((M, N), float("nan"), device="cuda")
    slab = torch.empty(32 * M * N + 4, device="cuda") if splits != 1 else None  # the plan caps at 32 slices
    native.gemm(native.GM2_BF16, Ps, Ps.stride(0), Qs, Qs.stride(0), C, N, M, N, K, splits, slab, pk, qk)
    torch.cuda.synchronize()
    return C.cpu()


_ints = {}


def _int_case(M, N, K):
    """P, Q in -2..2 from a fixed seed (pads zero) and the int64 reference, made once per shape."""
    if (M, N, K) not in _ints:
        g = torch.Generator().manual_seed(1000 * M + N)
        Mp, Np = -(-M // 256) * 256, -(-N // 256) * 256
        P = torch.zeros(Mp, K)
        Q = torch.zeros(Np, K)
        P[:M] = torch.randint(-2, 3, (M, K), generator=g).float()
        Q[:N] = torch.randint(-2, 3, (N, K), generator=g).float()
        ref = P[:M].long() @ Q[:N].long().T
        # |partial sums| <= 4 K < 2^24: exact in fp32 whatever the order
        assert 4 * K < 2 ** 24
        # a column permutation must not be able to hide: the reference's columns are pairwise distinct
        assert torch.unique(ref, dim=1).shape[1] == N
        _ints[(M, N, K)] = (P, Q, ref)
    return _ints[(M, N, K)]


@pytest.mark.parametrize("splits", [1, -1])
@pytest.mark.parametrize("M,N,K", [(256, 512, 8192), (200, 499, 8192)])
@pytest.mark.parametrize("layout", ["nn", "tn"])
def test_exact_integers(layout, M, N, K, splits, pingpong):
    """(200, 499): N pads to 512 and ldc = 499 rows are not 16-B aligned, so with one K pass the
    row-shifted store runs; splits = -1 is the plan's own split-K count, summed from slabs."""
    P, Q, ref = _int_case(M, N, K)
    C = _run(P, Q, M, N, K, layout, splits)
    assert torch.isfinite(C).all()
    bad = (C.long() != ref) | (C != C.round())
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:8].tolist())


@pytest.mark.parametrize("splits", [1, -1])
@pytest.mark.parametrize("layout", ["nn", "tn"])
def test_identity_probe(layout, splits, pingpong):
    """Q[k][n] = [k == n] in MN-major storage (K = 8192 >= N = 512), P[m][k] = (131 m + k) mod 251
    (exact in bf16): C = P[:, :N] exactly."""
    M, N, K = 256, 512, 8192
    P = ((torch.arange(M)[:, None] * 131 + torch.arange(K)[None, :]) % 251).float()
    Q = torch.zeros(N, K)
    Q[torch.arange(N), torch.arange(N)] = 1.0
    C = _run(P, Q, M, N, K, layout, splits)
    bad = C != P[:, :N]
    assert not bad.any(), (int(bad.sum()), bad.nonzero()[:8].tolist())


def test_row_pitch_limit(pingpong):
    """ld >= 2^24 elements: a thread's offset (< 128 rows * ld * 2 B) would not fit 32 bits; gm2_gemm
    refuses on the host (check_gemm), before anything is launched or read."""
    M, N, K = 256, 256, 8192
    P = torch.zeros(8, dtype=torch.bfloat16, device="cuda")
    C = torch.zeros(M, N, device="cuda")
    for ldp, ldq in [(1 << 24, K), (K, 1 << 24)]:
        with pytest.raises(RuntimeError, match="row pitch"):
            native.gemm(native.GM2_BF16, P, ldp, P, ldq, C, N, M, N, K, 1, None, True, True)
