"""The fused InfoNCE kernels (csrc/nce_fused.hip) called through their C entries
(irc_nce_fused_workspace / _fwd / _bwd) on the test's own buffers, against an fp64 numpy
reference of the same loss, per row: lse, loss_row = lse - positive logit, and
dF = [dq; dk] (the queue term on the q rows).

Cases: every width D = 32 .. 256 at a batch of three waves (the last half-empty) with a
ragged queue tile; at D = 32 and 96 the batches and queues that are no multiple of the
wave, of the 128-row group, of 4 columns or of the 32-column tile, and 68 column chunks
(a second stride of the combine's lanes, eight full rounds plus a tail of the reduce's
8-way sum); the 48 MB cap on the backward partials; pair ranges [p_lo, p_hi) of one and
of two row groups; duplicated, identical, clustered and non-unit rows; and the same
cases through info_nce with the fused path on and off (IRC_NCE_FUSED), which runs the
unfused row kernels on them too.

Bounds.  They come from the reference, never from the kernel.  Next to the fp64
reference stands a plain fp32 numpy restatement of the same formula (fp32 matmul,
max-shifted logsumexp, (G + G^T) F): its distance from fp64 is what fp32 arithmetic
alone costs on the case,

  e32_lse = max_r |lse32_r - lse64_r|
  e32_dF  = max_u ||dF32_u - dF64_u|| / M_u

with M_u the sum that forms dF_u with every term replaced by its size:
M_u = 0.5 / T * (sum_{v != u} (P_uv + P_vu + [v = pos_u] + [u = pos_v]) ||F_v||
                 + [u < N] sum_j (P_uj + P_{u+N,j}) ||queue_j||).
Row-relative error is ill-conditioned where dF_u cancels (duplicated or identical
rows: the restatement itself reaches 5e-6 .. 20 there); error over M_u is not.  The
kernel differs from the restatement by a fast exp, by one more rescale per chunk merge
of the online softmax and by its summation order, each a small constant factor, so it
gets 8 x the restatement's error:

  lse, loss_row: clamp(8 e32, 2e-6 max(1, max |operand|), 2e-5)
  dF:            clamp(8 e32_dF, 2e-6, 1e-5)   (row error over M_u)

The upper clamps are the project's own bounds on this loss (1e-5 in
test_model_gpu.py::test_infonce_loss_and_dq and in the fused-vs-unfused test of
test_configs_gpu.py); the lower clamp is about 16 fp32 ulps, so that a lucky tiny e32 on
a two-row case makes no false failure.  A dropped, duplicated or mis-masked column moves
a row by about its probability, orders of magnitude more.  loss_row = lse - pos carries
the rounding of both operands (|pos| <= 1 / T = 20), so its e32 is measured on loss_row
and its lower clamp takes the larger of max |lse| and max |pos|.  Every case asserts
that the restatement itself stays within a quarter of the upper clamp.  The summed loss:
1e-5 relative, 1e-5 absolute where the oracle's loss is below 1.

Every forward and backward here runs on a workspace of exactly the reported size, filled
with NaN, followed by 4 KB of a byte pattern that must survive; lse, loss_row and dF are
followed by sentinel elements that must survive too.

Each case prints one line "nce_fused_tests| ..." with e32, the achieved error and the
bound (pytest -s); profiles/nce_fused_tests.txt is that table from an MI355X run.
"""
import functools
import types

import numpy as np
import pytest
import torch

import synth_inputs as SI
from conftest import PKG  # noqa: F401  (import paths)
from oracle import irc_oracle as O

pytestmark = pytest.mark.gpu

T = 0.05
G = 0.25          # the upstream gradient (device scalar) of every backward but one
SENT = 12345.0    # sentinel of output elements that no call may write
TAIL = 4096       # bytes after the reported workspace ...
PATTERN = 0xA5    # ... of this value
LSE_HI, DF_HI = 2e-5, 1e-5  # upper clamps: the project's own bounds
LO = 2e-6                   # lower clamp: ~16 fp32 ulps


# ------------------------------------------------------------------ references
def nce_rows64(q, k, queue):
    """fp64 per-row InfoNCE (the maths of oracle.irc_oracle.nce_info_loss): lse [2N],
    pos [2N] (the positive logit / T), dF [2N, D] = [dq; dk] and the magnitude row M [2N]."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    n = q.shape[0]
    F = np.concatenate([q, k], axis=0)
    rows = np.arange(2 * n)
    pos = (rows + n) % (2 * n)
    L = F @ F.T / T
    full = L.copy()
    full[rows, rows] = -np.inf
    Qu = None
    if queue is not None and queue.shape[1] > 0:
        Qu = np.asarray(queue, np.float64)
        lq = q @ Qu / T
        full = np.concatenate([full, np.concatenate([lq, lq], axis=0)], axis=1)
    m = full.max(axis=1)
    lse = m + np.log(np.exp(full - m[:, None]).sum(axis=1))
    P = np.exp(full - lse[:, None])
    Pb = P[:, :2 * n]  # in-batch probabilities; the diagonal is exp(-inf) = 0
    Gm = Pb.copy()
    Gm[rows, pos] -= 1.0
    c = 0.5 / T
    dF = c * ((Gm + Gm.T) @ F)
    A = Pb + Pb.T
    A[rows, pos] += 2.0  # the -1 of [v = pos_u] and of [u = pos_v], each as +1
    M = c * (A @ np.linalg.norm(F, axis=1))
    if Qu is not None:
        W = P[:n, 2 * n:] + P[n:, 2 * n:]
        dF[:n] += c * (W @ Qu.T)
        M[:n] += c * (W @ np.linalg.norm(Qu, axis=0))
    return lse, L[rows, pos], dF, M


def nce_rows32(q, k, queue):
    """The same formula in plain fp32 numpy: what fp32 arithmetic alone costs."""
    f = np.float32
    q, k = np.asarray(q, f), np.asarray(k, f)
    n = q.shape[0]
    F = np.concatenate([q, k], axis=0)
    rows = np.arange(2 * n)
    pos = (rows + n) % (2 * n)
    inv_t = f(1) / f(T)  # the kernels' 1.f / T
    L = (F @ F.T) * inv_t
    full = L.copy()
    full[rows, rows] = -np.inf
    Qu = None
    if queue is not None and queue.shape[1] > 0:
        Qu = np.asarray(queue, f)
        lq = (q @ Qu) * inv_t
        full = np.concatenate([full, np.concatenate([lq, lq], axis=0)], axis=1)
    m = full.max(axis=1)
    lse = m + np.log(np.exp(full - m[:, None]).sum(axis=1, dtype=f))
    P = np.exp(full - lse[:, None])
    Gm = P[:, :2 * n].copy()
    Gm[rows, pos] -= f(1)
    c = f(0.5) / f(T)
    dF = c * ((Gm + Gm.T) @ F)
    if Qu is not None:
        dF[:n] += c * ((P[:n, 2 * n:] + P[n:, 2 * n:]) @ Qu.T)
    assert lse.dtype == f and dF.dtype == f and L.dtype == f
    return lse, L[rows, pos], dF


def row_err(got, ref, M):
    """max_u ||got_u - ref_u|| / M_u"""
    d = np.asarray(got, np.float64) - ref
    return float(np.max(np.linalg.norm(d, axis=1) / M))


def clamp(x, lo, hi):
    return min(max(x, lo), hi)


# ------------------------------------------------------------------ cases
def _inputs(N, D, K, kind):
    seed = 100000 + 131 * N + 7 * D + K
    if kind != "unit":
        # With logits of 20 (k[5] = q[5], identical rows) e32_lse is 20 x the fp32 matmul's
        # rounding of ||q||^2 = 1: 1e-6 .. 7e-6 from seed to seed, on either side of the
        # condition that case() sets (5e-6).  This seed gives 1.5e-6 or less on all four.
        seed += 30000
    q, k = SI.unit_rows(seed, N, D), SI.unit_rows(seed + 1000, N, D)
    queue = SI.unit_cols(seed + 2000, D, K) if K > 0 else None
    rng = np.random.default_rng(seed + 3000)
    if kind == "dups":
        q[7], k[5], k[9], queue[:, 11] = q[3], q[5], k[8], q[0]
    elif kind == "same":
        q[:] = q[0]
        k[:] = q[0]
    elif kind == "cluster":  # 0.2 x + c, renormalised
        c = SI.unit_rows(seed + 4000, 1, D).astype(np.float64)
        q, k = (((0.2 * x + c) / np.linalg.norm(0.2 * x + c, axis=1, keepdims=True))
                .astype(np.float32) for x in (q.astype(np.float64), k.astype(np.float64)))
    elif kind == "norms":  # row norms from [0.25, 1]
        q = (q * rng.uniform(0.25, 1.0, (N, 1))).astype(np.float32)
        k = (k * rng.uniform(0.25, 1.0, (N, 1))).astype(np.float32)
    else:
        assert kind == "unit"
    return q, k, queue


@functools.lru_cache(maxsize=None)
def case(N, D, K, kind="unit"):
    """Inputs, the fp64 rows, the restatement's error and the kernel's bounds (computed
    once per case and shared: nothing below writes to them)."""
    q, k, queue = _inputs(N, D, K, kind)
    lse, pos, dF, M = nce_rows64(q, k, queue)
    # the helper is the oracle's maths: same loss, dq and dk
    loss, dq, dk = O.nce_info_loss(q, k, queue, T, want_dk=True)
    np.testing.assert_allclose(0.5 * np.sum(lse - pos), loss, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dF, np.concatenate([dq, dk]), rtol=1e-9, atol=1e-12)
    lse32, pos32, dF32 = nce_rows32(q, k, queue)
    e_lse = float(np.max(np.abs(lse32 - lse)))
    e_row = float(np.max(np.abs((lse32 - pos32) - (lse - pos))))
    e_dF = row_err(dF32, dF, M)
    c = types.SimpleNamespace(
        N=N, D=D, K=K, kind=kind, q=q, k=k, queue=queue, lse=lse, loss_row=lse - pos, dF=dF,
        M=M, loss=float(loss), e_lse=e_lse, e_row=e_row, e_dF=e_dF,
        b_lse=clamp(8 * e_lse, LO * max(1.0, np.max(np.abs(lse))), LSE_HI),
        b_row=clamp(8 * e_row, LO * max(1.0, np.max(np.abs(lse)), np.max(np.abs(pos))), LSE_HI),
        b_dF=clamp(8 * e_dF, LO, DF_HI))
    for a in (q, k, queue, lse, c.loss_row, dF, M):
        if a is not None:
            a.flags.writeable = False
    # a condition of the case: fp32 arithmetic alone stays within a quarter of the upper clamps
    # (on lse and dF; loss_row's e32 on clustered rows is 20 x the matmul's rounding of a
    # positive logit near 19, about 5e-6, and its bound is then the upper clamp)
    assert e_lse <= LSE_HI / 4 and e_dF <= DF_HI / 4, (e_lse, e_dF)
    return c


def name_of(c, extra=""):
    kind = "" if c.kind == "unit" else "-" + c.kind
    return f"N{c.N}-K{c.K}-D{c.D}{kind}{extra}"


def report(c, name, e_lse=None, e_row=None, e_dF=None):
    """One line of the table; returns the failures (asserted by the caller after printing)."""
    def col(e32, got, bound):
        return f"{e32:9.2e} {'-' if got is None else format(got, '.2e'):>9} {bound:9.2e}"
    print(f"nce_fused_tests| {name:<30} | {col(c.e_lse, e_lse, c.b_lse)} | "
          f"{col(c.e_row, e_row, c.b_row)} | {col(c.e_dF, e_dF, c.b_dF)}")
    bad = [f"{what} {got:.3g} > {bound:.3g}" for what, got, bound in
           (("lse", e_lse, c.b_lse), ("loss_row", e_row, c.b_row), ("dF", e_dF, c.b_dF))
           if got is not None and not got <= bound]
    return bad


# ------------------------------------------------------------------ the C entries
def ws_bytes(c, lo, hi):
    from irc_amd import _lib

    nb = int(_lib.fn("irc_nce_fused_workspace")(c.N, c.D, c.K, lo, hi))
    assert nb > 0 and nb % 4 == 0
    return nb


def upload(c, dev):
    F = torch.from_numpy(np.concatenate([c.q, c.k], axis=0)).to(dev)
    qu = torch.from_numpy(np.array(c.queue)).to(dev) if c.K > 0 else None
    return F, qu


def new_ws(nb, dev, fill):
    """The reported bytes (NaN or zero) and the guarded tail."""
    ws = torch.full((nb + TAIL,), PATTERN, dtype=torch.uint8, device=dev)
    if fill == "nan":
        ws[:nb].view(torch.float32).fill_(float("nan"))
    else:
        ws[:nb].zero_()
    return ws


def fwd(c, F, qu, lo, hi, fill="nan"):
    """lse, loss_row [2N] (numpy fp32; rows outside the range hold SENT)."""
    from irc_amd import _lib
    from irc_amd._torch import ptr, stream_ptr

    nb = ws_bytes(c, lo, hi)
    ws = new_ws(nb, F.device, fill)
    lse = torch.full((2 * c.N + 64,), SENT, dtype=torch.float32, device=F.device)
    loss_row = torch.full_like(lse, SENT)
    _lib.call("irc_nce_fused_fwd", ptr(F), ptr(qu), c.N, c.D, c.K, T, lo, hi, ptr(ws), nb,
              ptr(lse), ptr(loss_row), stream_ptr(F.device))
    torch.cuda.synchronize()
    assert bool((ws[nb:] == PATTERN).all()), "forward wrote past the reported workspace"
    assert bool((lse[2 * c.N:] == SENT).all()) and bool((loss_row[2 * c.N:] == SENT).all())
    return lse[:2 * c.N].cpu().numpy(), loss_row[:2 * c.N].cpu().numpy(), loss_row[:2 * c.N]


def bwd(c, F, qu, lse, lo, hi, g=G, fill="nan"):
    """dF [2N, D], or [2P, D] for a partial range (numpy fp32)."""
    from irc_amd import _lib
    from irc_amd._torch import ptr, stream_ptr

    nb = ws_bytes(c, lo, hi)
    ws = new_ws(nb, F.device, fill)
    rows = 2 * c.N if (lo, hi) == (0, c.N) else 2 * (hi - lo)
    dF = torch.full((rows + 2, c.D), SENT, dtype=torch.float32, device=F.device)
    gs = None if g is None else torch.tensor([g], dtype=torch.float32, device=F.device)
    lse_d = torch.from_numpy(np.ascontiguousarray(lse)).to(F.device)
    _lib.call("irc_nce_fused_bwd", ptr(F), ptr(qu), ptr(lse_d), c.N, c.D, c.K, T, ptr(gs), lo, hi,
              ptr(ws), nb, ptr(dF), stream_ptr(F.device))
    torch.cuda.synchronize()
    assert bool((ws[nb:] == PATTERN).all()), "backward wrote past the reported workspace"
    assert bool((dF[rows:] == SENT).all()), "backward wrote past its rows"
    return dF[:rows].cpu().numpy()


def check_full(c, dev, g=G, extra=""):
    """Forward and backward over [0, N) against fp64: lse, loss_row, dF, summed loss."""
    from irc_amd import ops

    F, qu = upload(c, dev)
    lse, loss_row, loss_row_d = fwd(c, F, qu, 0, c.N)
    loss = ops.dsum(loss_row_d.contiguous(), 0.5).item()
    dF = bwd(c, F, qu, lse, 0, c.N, g)
    gg = 1.0 if g is None else g
    bad = report(c, name_of(c, extra), float(np.max(np.abs(lse - c.lse))),
                 float(np.max(np.abs(loss_row - c.loss_row))), row_err(dF, gg * c.dF, gg * c.M))
    assert np.isfinite(lse).all() and np.isfinite(loss_row).all() and np.isfinite(dF).all()
    assert not bad, bad
    assert abs(loss - c.loss) <= 1e-5 * (abs(c.loss) if c.loss >= 1 else 1.0), (loss, c.loss)
    return lse, loss_row, dF


# ------------------------------------------------------------------ 1. shape grid
EDGES = [(1, 0), (1, 3), (2, 5), (33, 100), (70, 131), (64, 64), (40, 4200)]
GRID = ([(40, 36, D) for D in range(32, 257, 32)] +
        [(N, K, D) for D in (32, 96) for N, K in EDGES] +
        # the 48 MB cap on the backward partials: at (512, 4096) the C = 1 partials are exactly
        # 2 x 48 MB, so the backward keeps the forward's C = 2; one more queue tile is past
        # the cap (backward C = 3, forward C = 2: 11 + 43 chunks against 16 + 65; the plan is
        # pinned in test_nce_fused_validation_cpu.py)
        [(512, 4096, 256), (512, 4128, 256)])


@pytest.mark.parametrize("N,K,D", GRID, ids=[f"N{n}-K{k}-D{d}" for n, k, d in GRID])
def test_shape_grid(gpu, N, K, D):
    c = case(N, D, K)
    lse, loss_row, dF = check_full(c, gpu)
    if (N, K) == (1, 0):  # the only logit is the positive: loss 0, no gradient
        assert np.abs(loss_row).max() <= 1e-6 and np.abs(dF).max() <= 1e-6


def test_null_gscale_is_one(gpu):
    check_full(case(33, 96, 100), gpu, g=None, extra="-g1")


# ------------------------------------------------------------------ 2. guards
@pytest.mark.parametrize("N,K,D", [(70, 131, 96), (40, 4200, 32)])
def test_workspace_guards_and_determinism(gpu, N, K, D):
    """No partial is read that the same call did not write (a NaN-filled workspace gives
    the bits of a zero-filled one), and a second call gives the same bits.  The tail after
    the reported workspace is checked inside fwd() / bwd() after every call."""
    c = case(N, D, K)
    F, qu = upload(c, gpu)
    runs = []
    for fill in ("nan", "zero", "nan"):
        lse, loss_row, _ = fwd(c, F, qu, 0, N, fill=fill)
        dF = bwd(c, F, qu, lse, 0, N, fill=fill)
        assert np.isfinite(lse).all() and np.isfinite(loss_row).all() and np.isfinite(dF).all()
        runs.append((lse, loss_row, dF))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ 3. pair ranges
RANGES = ([(192, 64, 100, lo, hi) for lo, hi in ((0, 32), (32, 96), (32, 192), (160, 192))] +
          [(64, 160, 0, lo, hi) for lo, hi in ((0, 32), (32, 64))])
_full = {}


def full_range_run(c, dev):
    """The full-range call's lse, loss_row and dF (once per case; checked against fp64)."""
    key = (c.N, c.D, c.K)
    if key not in _full:
        _full[key] = check_full(c, dev)
    return _full[key]


@pytest.mark.parametrize("N,D,K,lo,hi", RANGES,
                         ids=[f"N{n}-K{k}-D{d}-{lo}:{hi}" for n, d, k, lo, hi in RANGES])
def test_pair_range(gpu, N, D, K, lo, hi):
    """What a data-parallel rank computes: the rows of its pairs [lo, hi) only.  The
    backward takes the full-range forward's lse (what the all-gather delivers)."""
    c = case(N, D, K)
    lse_f, loss_row_f, dF_f = full_range_run(c, gpu)
    F, qu = upload(c, gpu)
    P = hi - lo
    inside = np.concatenate([np.arange(lo, hi), N + np.arange(lo, hi)])
    outside = np.setdiff1d(np.arange(2 * N), inside)
    lse, loss_row, _ = fwd(c, F, qu, lo, hi)
    dF = bwd(c, F, qu, lse_f, lo, hi)
    assert dF.shape == (2 * P, D)  # q rows of the range, then its k rows
    bad = report(c, name_of(c, f"-{lo}:{hi}"), float(np.max(np.abs(lse[inside] - c.lse[inside]))),
                 float(np.max(np.abs(loss_row[inside] - c.loss_row[inside]))),
                 row_err(dF, G * c.dF[inside], G * c.M[inside]))
    assert (lse[outside] == SENT).all() and (loss_row[outside] == SENT).all()
    assert not bad, bad
    # both plans take the C = 2 floor of pick_chunk here, so a row meets the same tiles in
    # the same chunks as in the full-range call: the same bits
    for got, full in ((lse[inside], lse_f[inside]), (loss_row[inside], loss_row_f[inside]),
                      (dF, dF_f[inside])):
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(full).view(np.uint32))


# ------------------------------------------------------------------ 4. adversarial inputs
@pytest.mark.parametrize("kind", ["dups", "same", "cluster", "norms"])
def test_adversarial_inputs(gpu, kind):
    check_full(case(40, 64, 100, kind), gpu)


# ------------------------------------------------------------------ 5. through info_nce
NCE = ([(N, K, D, fused) for N, K, D in ((40, 36, 32), (33, 100, 96), (70, 131, 96))
        for fused in ("1", "0")] +
       [(33, 100, 48, "1"), (33, 100, 288, "1")])  # unfused whatever the variable says


@pytest.mark.parametrize("N,K,D,fused", NCE,
                         ids=[f"N{n}-K{k}-D{d}-fused{f}" for n, k, d, f in NCE])
def test_info_nce(gpu, monkeypatch, N, K, D, fused):
    """info_nce with k requiring grad, fused path on and off: the dispatcher, the autograd
    wrappers' row split and, with IRC_NCE_FUSED=0 or an unsupported width, the unfused
    row kernels (irc_nce_lse, irc_nce_grads) at ragged N and K."""
    from irc_amd import nce

    monkeypatch.setenv("IRC_NCE_FUSED", fused)
    assert nce.fused_ok(D) == (fused == "1" and D in range(32, 257, 32))
    c = case(N, D, K)
    ref_loss, ref_dq, ref_dk = O.nce_info_loss(c.q, c.k, c.queue, T, want_dk=True)
    q = torch.from_numpy(np.array(c.q)).to(gpu).requires_grad_()
    k = torch.from_numpy(np.array(c.k)).to(gpu).requires_grad_()
    loss = nce.info_nce(q, k, torch.from_numpy(np.array(c.queue)).to(gpu), T)
    (loss * G).backward()
    e_loss = abs(loss.item() - ref_loss) / abs(ref_loss)
    e_dq = row_err(q.grad.cpu().numpy(), G * ref_dq, G * c.M[:N])
    e_dk = row_err(k.grad.cpu().numpy(), G * ref_dk, G * c.M[N:])
    path = "fused" if nce.fused_ok(D) else "rows"
    bad = report(c, name_of(c, f"-nce-{path}"), e_dF=max(e_dq, e_dk))
    print(f"nce_fused_tests|   loss rel err {e_loss:.2e} (bound 1e-05)")
    assert not bad, bad
    assert e_loss <= 1e-5
