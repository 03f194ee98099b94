"""The big-tile bf16 GEMM's default epilogue (big_epilogue_bf16, gemm.hip): packed first
stage, hoisted store addressing, interior-tile fast path.

The shapes are the smallest with 128 big tiles (big_wnb's threshold).  At a few hundred
tiles the dispatch prefers the ping-pong 256 x 256 kernel, so every big-tile launch here
runs with that path switched off (ops.gemm_set_pp), which leaves big_wnb's choice:
  (32700, 384, 64)   256 x 384 tiles, one column tile, interior tiles and a ragged last row tile
  (8100, 1536, 128)  256 x 384 tiles, four column tiles, two K-tiles
  (10900, 520, 64)   256 x 256 tiles, ragged in M and in N
"""
import contextlib
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(32700, 384, 64), (8100, 1536, 128), (10900, 520, 64)]


@contextlib.contextmanager
def _big_tile_only():
    from irc_amd import ops

    prev = ops.gemm_set_pp(False)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        ops.gemm_set_pp(prev)


@functools.lru_cache(maxsize=1)  # the epilogues of one shape run back to back
def _exact_case(M, N, K):
    """Operands as test_gemm_gpu._exact_case builds them: small integers, a bias on the 1/4
    grid, an integer residual; every sum is exact in fp32 (checked against fp64)."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-4, 5, (M, K), generator=g).to(torch.bfloat16)
    b = torch.randint(-4, 5, (N, K), generator=g).to(torch.bfloat16)
    bias = torch.randint(-8, 9, (N,), generator=g).float() / 4
    res = torch.randint(-8, 9, (M, N), generator=g).to(torch.bfloat16)
    prod = a.float() @ b.float().t()
    assert torch.equal(prod.double(), a.double() @ b.double().t())
    return a, b, bias, res, prod


@pytest.mark.parametrize("epi", [0, 1, 3, 4])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_strided_c_exact(gpu, epi, M, N, K):
    """Epilogues 0, 1, 3, 4 with bf16 C: bit-equal to the rounded CPU result.  C and the
    residual are column slices of wider buffers (ldc != N, ldr != ldc), which exercises the
    hoisted row offsets; the columns of C's buffer outside the slice must stay untouched."""
    from irc_amd import ops

    a, b, bias, res, prod = _exact_case(M, N, K)
    bias = bias if epi in (1, 3) else None
    res = res if epi in (3, 4) else None
    wide = torch.full((M, N + 24), -77.0, dtype=torch.bfloat16, device=gpu)
    out = wide[:, 8:8 + N]
    rdev = None
    if res is not None:
        rwide = torch.zeros((M, N + 40), dtype=torch.bfloat16, device=gpu)
        rdev = rwide[:, 16:16 + N]
        rdev.copy_(res)
    with _big_tile_only():
        ops.gemm(a.to(gpu), b.to(gpu), bias=None if bias is None else bias.to(gpu), epilogue=epi,
                 residual=rdev, out=out)
    ref = prod if bias is None else prod + bias
    ref = ref if res is None else ref + res.float()
    got = wide.cpu()
    assert torch.equal(got[:, 8:8 + N], ref.to(torch.bfloat16))
    assert (got[:, :8] == -77.0).all() and (got[:, 8 + N:] == -77.0).all()


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_packed_gelu_bit_identical_to_scalar(gpu, M, N, K):
    """Epilogue 2: the big tile's packed gelu_lite2 against the scalar gelu_lite of
    gemm_kernel, bit for bit.  Operands in {-1, 0, 1} with about sqrt(6 / K) of them
    nonzero keep the integer sums within about +-8; with alpha = 1 and a random fp32 bias
    the pre-activation acc + bias is one exact rounding in any kernel, and the columns'
    biases spread it densely over GELU's curved range.  The route to gemm_kernel: the same
    A in a buffer whose row stride is no multiple of 8 elements, which the big tile and the
    256 x 256 kernel both refuse (ops.gemm passes a.stride(0) as lda)."""
    from irc_amd import ops

    g = torch.Generator().manual_seed(M + N + K)
    q = (6.0 / K) ** 0.5
    a = (torch.randint(-1, 2, (M, K), generator=g) * (torch.rand((M, K), generator=g) < q * 1.5))
    b = (torch.randint(-1, 2, (N, K), generator=g) * (torch.rand((N, K), generator=g) < q * 1.5))
    a, b = a.to(torch.bfloat16).to(gpu), b.to(torch.bfloat16).to(gpu)
    bias = torch.randn((N,), generator=g).to(gpu)
    a_odd = torch.zeros((M, K + 4), dtype=torch.bfloat16, device=gpu)[:, :K]
    a_odd.copy_(a)
    assert a_odd.stride(0) % 8 != 0
    with _big_tile_only():
        big = ops.gemm(a, b, bias=bias, epilogue=2, out_dtype=torch.bfloat16)
    scalar = ops.gemm(a_odd, b, bias=bias, epilogue=2, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    pre = a.float() @ b.float().t() + bias
    print(f"pre-activation range [{pre.min().item():.2f}, {pre.max().item():.2f}], "
          f"{(pre.abs() < 3).float().mean().item():.1%} within |x| < 3")
    assert (pre.abs() < 3).float().mean().item() > 0.5  # the curved range is covered
    assert torch.equal(big.view(torch.int16), scalar.view(torch.int16))
