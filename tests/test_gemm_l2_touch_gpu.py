"""L2 touch prefetch of the big-tile 16x16x32 K loop (big::touch_lines / touch_dword, gemm.hip;
switch: ops.gemm_set_l2_touch).  The touches load values nothing reads, so every result with
the switch on must equal the result with it off, bit for bit.

The big-tile kernel takes a launch of at least 128 tiles (big_wnb), so each GEMM shape runs as
a batch of that many tiles (32 x [512 x 768], 16 x [256 x 3072], 64 x [512 x 384]) through
irc_gemm_ex, with the ping-pong 256 x 256 kernel switched off as in test_gemm_dma_addr_gpu.py.
irc_qkv_attention has no such threshold.
"""
import contextlib
import functools

import pytest
import torch

gpu_test = pytest.mark.gpu

EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID = 1, 2, 3


@contextlib.contextmanager
def _big_tile_only():
    from irc_amd import ops

    prev = ops.gemm_set_pp(False)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        ops.gemm_set_pp(prev)


def _on_and_off(run):
    """run() with the touch prefetch on for every launch that can take it (mode 2: the default
    mode leaves launches of more than two column tiles alone), then off."""
    from irc_amd import ops

    prev = ops.gemm_set_l2_touch(2)
    try:
        on = run()
        ops.gemm_set_l2_touch(0)
        off = run()
        torch.cuda.synchronize()
    finally:
        ops.gemm_set_l2_touch(prev)
    return on, off


def _batches(M, N):
    """Batch count that brings the launch to 128 tiles (256 x 384 where 384 divides N, else
    256 x 256)."""
    tiles = -(-M // 256) * (N // 384 if N % 384 == 0 else -(-N // 256))
    return -(-128 // tiles)


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, batch, pad_a=0, pad_b=0):
    """bf16 Gaussian A [batch][M][K + pad_a], B [batch][N][K + pad_b] (the pad columns hold
    a large sentinel), fp32 bias [batch][N], bf16 residual [batch][M][N], on the CPU."""
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + batch)
    a = torch.full((batch, M, K + pad_a), 16384.0, dtype=torch.bfloat16)
    b = torch.full((batch, N, K + pad_b), 16384.0, dtype=torch.bfloat16)
    a[:, :, :K] = torch.randn((batch, M, K), generator=g).to(torch.bfloat16)
    b[:, :, :K] = (torch.randn((batch, N, K), generator=g) * 0.1).to(torch.bfloat16)
    bias = torch.randn((batch, N), generator=g)
    res = torch.randn((batch, M, N), generator=g).to(torch.bfloat16)
    return a, b, bias, res


def _gemm_ex(a, b, bias, res, epi, M, N, K, batch, lda, sA, ldb, sB):
    """irc_gemm_ex, bf16 in and out, A [M][K] . B [N][K]^T per batch item."""
    from irc_amd import _lib
    from irc_amd._torch import ptr, stream_ptr

    out = torch.empty((batch, M, N), dtype=torch.bfloat16, device=a.device)
    use_res = epi == EPI_BIAS_RESID
    _lib.call("irc_gemm_ex", 0, 0, 0, 0, epi, M, N, K, 1.0, ptr(a), lda, sA, ptr(b), ldb, sB,
              ptr(bias), N, ptr(res) if use_res else None, N if use_res else 0,
              M * N if use_res else 0, ptr(out), N, M * N, 0, batch, None, 0, 0,
              stream_ptr(a.device))
    return out


def _check(gpu, M, N, K, epi, pad_a=0, pad_b=0):
    batch = _batches(M, N)
    a, b, bias, res = (t.to(gpu) for t in _operands(M, N, K, batch, pad_a, pad_b))
    lda, ldb = K + pad_a, K + pad_b
    with _big_tile_only():
        on, off = _on_and_off(lambda: _gemm_ex(a, b, bias, res, epi, M, N, K, batch, lda,
                                               M * lda, ldb, N * ldb))
    assert on.float().abs().max().item() > 1.0  # not all zeros
    assert torch.equal(on.view(torch.int16), off.view(torch.int16))
    return on


@gpu_test
@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID])
@pytest.mark.parametrize("K", [64, 128, 192, 768])
def test_k_tiles_around_the_distance(gpu, K, epi):
    """M = 512, N = 768 (two row tiles, two column tiles: two sharers per operand) with one,
    two, three and twelve K-tiles: fewer than the distance reaches, exactly one touched
    K-tile, and many.  Each epilogue of the encoder."""
    out = _check(gpu, 512, 768, K, epi)
    if epi == EPI_BIAS and K == 192:  # the launch is the product it claims to be
        a, b, bias, _ = _operands(512, 768, K, _batches(512, 768))
        ref = torch.bmm(a.float(), b.float().transpose(1, 2)) + bias[:, None, :]
        assert (out.cpu().float() - ref).abs().max().item() <= 2.0 ** -7 * ref.abs().max().item()


@gpu_test
@pytest.mark.parametrize("epi", [EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESID])
@pytest.mark.parametrize("M,N", [
    (256, 3072),  # eight sharers of A, one row tile: B unshared
    (512, 384),   # one column tile: no A sharer
    (300, 768),   # the second row tile is an edge tile: it stays on stage(), untouched
    (512, 512),   # 256 x 256 tiles (the WNB = 2 instantiation): 256 lines of B
])
def test_sharing_geometries(gpu, M, N, epi):
    _check(gpu, M, N, 192, epi)


@gpu_test
def test_batched_strided_operands(gpu):
    """lda = K + 8, ldb = K + 24 (lines that straddle 128-byte boundaries), batch strides of
    whole padded operands: the descriptor's base moves with the batch index."""
    _check(gpu, 512, 768, 192, EPI_BIAS_RESID, pad_a=8, pad_b=24)


@gpu_test
def test_row_slice_ending_the_allocation(gpu):
    """A and B are the last rows of their allocations: the descriptors end with the
    allocation, and the last owned line of the last K-tile is its last 128 bytes."""
    M, N, K = 512, 768, 192
    batch = _batches(M, N)
    a, b, bias, res = (t.to(gpu) for t in _operands(M, N, K, batch))
    big_a = torch.zeros((batch * M + 77, K), dtype=torch.bfloat16, device=gpu)
    big_b = torch.zeros((batch * N + 13, K), dtype=torch.bfloat16, device=gpu)
    av, bv = big_a[77:], big_b[13:]
    av.copy_(a.view(batch * M, K))
    bv.copy_(b.view(batch * N, K))
    assert av.data_ptr() + av.numel() * 2 == big_a.data_ptr() + big_a.numel() * 2
    with _big_tile_only():
        on, off = _on_and_off(lambda: _gemm_ex(av, bv, bias, res, EPI_BIAS, M, N, K, batch, K,
                                               M * K, K, N * K))
        whole = _gemm_ex(a, b, bias, res, EPI_BIAS, M, N, K, batch, K, M * K, K, N * K)
    assert torch.equal(on.view(torch.int16), off.view(torch.int16))
    assert torch.equal(on.view(torch.int16), whole.view(torch.int16))


@gpu_test
@pytest.mark.parametrize("L,blocked", [(64, False), (40, False), (64, True)])
def test_qkv_attention_on_equals_off(gpu, L, blocked):
    """irc_qkv_attention, 8 sequences, H = 768 (two row tiles of four sequences, six column
    tiles): full 64-row slots, slots of 40 tokens, and a mask whose keys 32 .. 63 (one whole
    key block) are hidden in every other sequence."""
    from irc_amd import ops

    B, H, heads = 8, 768, 12
    g = torch.Generator().manual_seed(L + 7 * blocked)
    x = (torch.randn(B * L, H, generator=g) * 0.5).bfloat16().to(gpu)
    w = (torch.randn(3 * H, H, generator=g) * 0.05).bfloat16().to(gpu)
    bias = (torch.randn(3 * H, generator=g) * 0.1).to(gpu)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    if blocked:
        lens[::2] = 32
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64).to(gpu)
    perm = ops.qkv_perm_index(H, gpu)
    wp, bp = w.index_select(0, perm).contiguous(), bias.index_select(0, perm).contiguous()
    on, off = _on_and_off(lambda: ops.qkv_attention(x, wp, bp, mask, B, L, H, heads))
    assert on.float().abs().max().item() > 1e-3
    assert torch.equal(on.view(torch.int16), off.view(torch.int16))
