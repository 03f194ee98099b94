"""Buffer-addressed operand staging of the big-tile 16x16x32 K loop (big::stage_buf,
gemm.hip; switch: ops.gemm_set_big_dma) against the per-lane 64-bit staging it replaces on
interior tiles.  Both build the same LDS image, so every result must be bit-identical.

The shapes are the smallest with 128 big tiles (big_wnb's threshold); the ping-pong
256 x 256 kernel is switched off (ops.gemm_set_pp) so that the big tile takes them, as in
test_gemm_epilogue_gpu.py.
"""
import contextlib
import functools

import pytest
import torch

gpu_test = pytest.mark.gpu


@contextlib.contextmanager
def _big_tile_only():
    from irc_amd import ops

    prev = ops.gemm_set_pp(False)
    try:
        yield
        torch.cuda.synchronize()
    finally:
        ops.gemm_set_pp(prev)


def _both_forms(run):
    """run() once per staging form: (buffer-addressed, per-lane addresses)."""
    from irc_amd import ops

    prev = ops.gemm_set_big_dma(True)
    try:
        new = run()
        ops.gemm_set_big_dma(False)
        old = run()
        torch.cuda.synchronize()
    finally:
        ops.gemm_set_big_dma(prev)
    return new, old


@gpu_test
@pytest.mark.parametrize("M,N,K", [
    (32768, 384, 64),    # every tile interior, one K-tile: the prologue alone
    (32700, 384, 128),   # ragged last row tile: both forms in one launch
    (8192, 1536, 768),   # four column tiles, twelve K-tiles
    (10900, 520, 64),    # 256 x 256 tiles, ragged in M and in N
])
def test_new_equals_old_random(gpu, M, N, K):
    """bf16 Gaussian operands: C with the switch on equals C with it off, bit for bit."""
    from irc_amd import ops

    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn((M, K), generator=g).to(torch.bfloat16).to(gpu)
    b = torch.randn((N, K), generator=g).to(torch.bfloat16).to(gpu)
    with _big_tile_only():
        new, old = _both_forms(lambda: ops.gemm(a, b))
    assert new.abs().max().item() > 1.0  # not all zeros
    assert torch.equal(new.view(torch.int16), old.view(torch.int16))


SENTINEL = 16384.0  # any operand element read from outside a slice wrecks the exact sums


@functools.lru_cache(maxsize=None)
def _exact_operands(M, N, K, batch):
    """Small integers, as test_gemm_epilogue_gpu._exact_case: every fp32 sum is exact."""
    g = torch.Generator().manual_seed(M + N + K + batch)
    a = torch.randint(-4, 5, (batch, M, K), generator=g).to(torch.bfloat16)
    b = torch.randint(-4, 5, (batch, N, K), generator=g).to(torch.bfloat16)
    prod = torch.bmm(a.float(), b.float().transpose(1, 2))
    assert torch.equal(prod.double(), torch.bmm(a.double(), b.double().transpose(1, 2)))
    return a, b, prod.to(torch.bfloat16)


def _sliced(t, pad, off, gpu):
    """t [batch][R][K] as the columns off .. off + K of a sentinel-filled [batch][R][K + pad]."""
    batch, R, K = t.shape
    wide = torch.full((batch, R, K + pad), SENTINEL, dtype=torch.bfloat16, device=gpu)
    wide[:, :, off:off + K].copy_(t)
    return wide, wide[:, :, off:off + K]


@gpu_test
@pytest.mark.parametrize("off", [0, 8])
def test_strided_offset_operands_exact(gpu, off):
    """A and B as column slices of wider buffers (lda = K + 8, ldb = K + 24), starting at
    the buffer's first element or 8 elements in (16-byte aligned, not 1 KB aligned): both
    forms equal the exact CPU product.  (8100, 1536, 128): interior tiles, a ragged last
    row tile, two K-tiles."""
    from irc_amd import ops

    M, N, K = 8100, 1536, 128
    a, b, ref = _exact_operands(M, N, K, 1)
    _, av = _sliced(a, 8, off, gpu)
    _, bv = _sliced(b, 24, off, gpu)
    assert av[0].stride(0) == K + 8 and bv[0].stride(0) == K + 24
    assert av[0].data_ptr() % 16 == 0 and bv[0].data_ptr() % 16 == 0
    with _big_tile_only():
        new, old = _both_forms(lambda: ops.gemm(av[0], bv[0]))
    assert torch.equal(new.cpu(), ref[0])
    assert torch.equal(old.cpu(), ref[0])


@gpu_test
def test_strided_batched_exact(gpu):
    """One batched launch (gemm_strided, batch 2, sA = M lda, sB = N ldb) over the same kind
    of slices: 17 x 4 tiles a batch, the descriptor's base moves with the batch index."""
    from irc_amd import ops

    M, N, K, batch = 4100, 1536, 64, 2
    a, b, ref = _exact_operands(M, N, K, batch)
    aw, av = _sliced(a, 8, 8, gpu)
    bw, bv = _sliced(b, 24, 8, gpu)

    def run():
        out = torch.empty((batch, M, N), dtype=torch.bfloat16, device=gpu)
        return ops.gemm_strided(av, bv, out, M=M, N=N, K=K, batch=batch, lda=K + 8,
                                sA=M * (K + 8), ldb=K + 24, sB=N * (K + 24), ldc=N, sC=M * N)

    with _big_tile_only():
        new, old = _both_forms(run)
    assert torch.equal(new.cpu(), ref)
    assert torch.equal(old.cpu(), ref)


@gpu_test
@pytest.mark.parametrize("B,L", [
    (512, 64),   # 64-row slots, full: contiguous rows
    (512, 40),   # 64-row slots of 40 tokens (as many waves of tiles as packed: slots stay):
                 # the slot layout in its buffer form
    (800, 40),   # packed tiles of six sequences: contiguous rows from a tile base of 240 tm
])
def test_qkv_attention_new_equals_old(gpu, B, L):
    """irc_qkv_attention at 20k-33k rows, H = 768: the context with the switch on equals the
    context with it off, bit for bit (test_qkv_attn_gpu.py holds it to the two-launch form)."""
    from irc_amd import ops

    H, heads = 768, 12
    g = torch.Generator().manual_seed(B + L)
    x = (torch.randn(B * L, H, generator=g) * 0.5).bfloat16().to(gpu)
    w = (torch.randn(3 * H, H, generator=g) * 0.05).bfloat16().to(gpu)
    bias = (torch.randn(3 * H, generator=g) * 0.1).to(gpu)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    mask = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int64).to(gpu)
    perm = ops.qkv_perm_index(H, gpu)
    wp, bp = w.index_select(0, perm).contiguous(), bias.index_select(0, perm).contiguous()
    new, old = _both_forms(lambda: ops.qkv_attention(x, wp, bp, mask, B, L, H, heads))
    assert new.float().abs().max().item() > 1e-3
    assert torch.equal(new.view(torch.int16), old.view(torch.int16))


def test_gate_on_the_host():
    """irc_gemm_big_dma_fits (no GPU, no allocation): the gate takes the C2 and C4 encoder
    shapes and refuses a row stride whose 256-row span passes 2^31 bytes, and operands
    whose whole span does."""
    from irc_amd import ops

    M = 32768
    for H in (768, 1024):  # C2 (BERT-base), C4 (BERT-large): QKV, out-proj, FFN1, FFN2
        for N, K in ((3 * H, H), (H, H), (4 * H, H), (H, 4 * H)):
            assert ops.gemm_big_dma_fits(M, N, K, K, K)
    assert ops.gemm_big_dma_fits(M, 384, 64, 72, 88)
    ld = (1 << 31) // (2 * 255)  # 255 rows on: just past 2^31 bytes
    assert (255 * (ld + 1) + 64) * 2 >= 1 << 31
    assert not ops.gemm_big_dma_fits(256, 384, 64, ld + 1, 64)   # A's 256-row span
    assert not ops.gemm_big_dma_fits(M, 384, 64, 64, ld + 1)     # B's
    assert not ops.gemm_big_dma_fits(1 << 24, 384, 64, 64, 64)   # A spans exactly 2^31 bytes
    assert ops.gemm_big_dma_fits((1 << 24) - 1, 384, 64, 64, 64)
    assert not ops.gemm_big_dma_fits(M, 384, 64, 1 << 40, 64)
    assert not ops.gemm_big_dma_fits(M, 384, 64, -64, 64)
