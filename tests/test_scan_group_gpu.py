"""The dense scan per group (irc_scan_topk_grouped; gemm_pp.hip EPI_GROUP) against the numpy
reference of test_rerank_group_cpu.py with every row of the shard a candidate of every query.
Integer grids with values in +-3 make every fp32 sum exact in any order and ties plentiful, so
idx, scores, n and groups must be equal bitwise, for bf16 and e4m3 operands.  The shapes cross
the 256-doc tile, the 256-query tile, the 64-query pass, the 32-column lane span and a ragged
last tile; on Gaussian data the call must return the bits of the streamed candidate top-k over
all-rows lists, whose main loop and tile origins it shares."""
import functools

import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (import paths)
from oracle import irc_oracle as O
from test_rerank_fp8_gpu import SCALE, _codes
from test_rerank_gpu import _grid, _hybrid_setup, _pack
from test_rerank_group_cpu import _reference_grouped
from test_rerank_group_gpu import _bitwise, _group_off

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "e4m3")


def _span_off(N, doc_offset):
    """Sizes cycling through 31, 32, 33, 1, 0 -- around the 32-column lane span -- from
    doc_offset - 7: a group begun in the previous shard; the last one ends past this one."""
    sizes = [31, 32, 33, 1, 0]
    go = [doc_offset - 7]
    j = 0
    while go[-1] < doc_offset + N:
        go.append(go[-1] + sizes[j % len(sizes)])
        j += 1
    return np.asarray(go, np.int64)


def _offsets(N, doc_offset, kind):
    return _span_off(N, doc_offset) if kind == "span" else _group_off(N, doc_offset, kind)


def _operands(rng, dtype, Q, N, D):
    if dtype == "e4m3":
        return _codes(rng, (Q, D)), _codes(rng, (N, D))
    return _grid(rng, (Q, D), 3), _grid(rng, (N, D), 3)


def _ref(dtype, q, d, k, go, doc_offset):
    """_reference_grouped with lists = all rows of the shard."""
    rows = [doc_offset + np.arange(d.shape[0], dtype=np.int64)] * q.shape[0]
    if dtype == "e4m3":
        i, s, n, g = _reference_grouped(O.dequantize_e4m3(q), O.dequantize_e4m3(d), rows, k, go,
                                        doc_offset)
        return i, (s * np.float32(SCALE)).astype(np.float32), n, g
    return _reference_grouped(q, d, rows, k, go, doc_offset)


@functools.lru_cache(maxsize=None)
def _case(Q, N, D, doc_offset, dtype):
    rng = np.random.default_rng(Q * 1000 + D + N)
    return _operands(rng, dtype, Q, N, D)


@functools.lru_cache(maxsize=None)
def _case_ref(Q, N, D, k, doc_offset, kind, dtype):
    """Operands, group offsets and the reference of one grid case: computed once, shared,
    left unchanged."""
    q, d = _case(Q, N, D, doc_offset, dtype)
    go = _offsets(N, doc_offset, kind)
    return q, d, go, _ref(dtype, q, d, k, go, doc_offset)


def _run(dtype, q, d, k, dev, doc_offset, go, **kw):
    from irc_amd import retrieval

    qd, dd = torch.from_numpy(q).to(dev), torch.from_numpy(d).to(dev)
    god = go if isinstance(go, torch.Tensor) else torch.from_numpy(np.asarray(go, np.int64)).to(dev)
    if dtype == "e4m3":
        out = retrieval.scan_topk_grouped_fp8(qd, dd, k, god, doc_offset, SCALE, **kw)
    else:
        out = retrieval.scan_topk_grouped(qd, dd, k, god, doc_offset, **kw)
    assert len(out) == 4
    s, i, n, g = out
    assert s.dtype == torch.float32 and i.dtype == torch.int64 and n.dtype == torch.int32
    assert g.dtype == torch.int64 and tuple(g.shape) == (q.shape[0], k)
    return i.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy(), g.cpu().numpy()


# (Q, N, D, k, doc_offset)
SHAPES = [(3, 40, 128, 8, 11), (33, 4099, 64, 10, 0), (65, 4099, 128, 100, 5),
          (257, 4099, 128, 100, 5), (7, 600, 1024, 1, 0)]
GRID_CASES = [s + (kind,) for s in SHAPES for kind in ("cycle", "span")] + \
    [(16, 20000, 768, 1024, 3, "many"), (16, 20000, 768, 1024, 3, "few")]
GRID_PARAMS = [(c, dt) for c in GRID_CASES for dt in DTYPES if not (dt == "e4m3" and c[2] % 128)]


@pytest.mark.parametrize("case,dtype", GRID_PARAMS)
def test_bit_exact_on_integer_grids(gpu, case, dtype):
    Q, N, D, k, doc_offset, kind = case
    q, d, go, ref = _case_ref(Q, N, D, k, doc_offset, kind, dtype)
    n_groups = np.count_nonzero(np.diff(go))
    assert (n_groups > 1024) if kind == "many" else (n_groups <= 1024)
    if kind == "span":
        assert go[0] == doc_offset - 7 and go[-1] >= doc_offset + N
    else:
        assert go[0] == doc_offset + 2  # the first two shard rows in no group
    got = _run(dtype, q, d, k, gpu, doc_offset, go)
    _bitwise(got, ref)
    # something was collapsed: fewer groups than eligible rows
    eligible = min(doc_offset + N, go[-1]) - max(doc_offset, go[0])
    groups_here = len(np.unique(np.searchsorted(go, np.arange(max(doc_offset, go[0]),
                                                              min(doc_offset + N, go[-1])),
                                                side="right")))
    assert groups_here < eligible
    assert (ref[2] == min(k, groups_here)).all()
    if kind == "many":
        assert ref[2].max() == k
    if kind == "few":  # trailing rows in no group are never returned
        assert go[-1] < doc_offset + N and (got[0] < go[-1]).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Q", [33, 257])
def test_singleton_groups_are_the_scan(gpu, dtype, Q):
    from irc_amd import retrieval

    N, D, k, doc_offset = 4099, 128, 100, 5
    q, d = _case(Q, N, D, doc_offset, dtype)
    go = doc_offset + np.arange(N + 1, dtype=np.int64)
    got = _run(dtype, q, d, k, gpu, doc_offset, go)
    qd, dd = torch.from_numpy(q).to(gpu), torch.from_numpy(d).to(gpu)
    if dtype == "e4m3":
        s, i = retrieval.scan_topk_fp8(qd, dd, k, doc_offset, SCALE)
    else:
        s, i = retrieval.scan_topk(qd, dd, k, doc_offset)
    np.testing.assert_array_equal(got[0], i.cpu().numpy())
    np.testing.assert_array_equal(got[1].view(np.uint32), s.cpu().numpy().view(np.uint32))
    assert (got[2] == k).all()
    np.testing.assert_array_equal(got[3], got[0] - doc_offset)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_keep_the_first_row_and_the_first_groups(gpu, dtype):
    N, D, k, doc_offset, Q = 1000, 128, 6, 9, 5  # 9 non-empty groups lie in 1000 rows
    rng = np.random.default_rng(1)
    q, row = _operands(rng, dtype, Q, 1, D)
    d = np.repeat(row, N, axis=0)  # every doc row identical: every score of a query ties
    go = _group_off(N, doc_offset, "cycle")
    i, s, n, g = _run(dtype, q, d, k, gpu, doc_offset, go)
    nonempty = np.flatnonzero(np.diff(go) > 0)[:k]
    assert nonempty.size == k and (n == k).all()
    for r in range(Q):
        np.testing.assert_array_equal(g[r], nonempty)  # the first k non-empty groups
        np.testing.assert_array_equal(i[r], go[nonempty])  # each by its first row
        assert (s[r] == s[r, 0]).all()


def _all_rows(Q, N, doc_offset, dev):
    return _pack([doc_offset + np.arange(N, dtype=np.int64)] * Q, dev)


def _stream_route(dtype, q, d, k, dev, doc_offset, go):
    """The same answer by the streamed candidate top-k over all-rows lists."""
    from irc_amd import retrieval

    cand, off = _all_rows(q.shape[0], d.shape[0], doc_offset, dev)
    qd, dd = torch.from_numpy(q).to(dev), torch.from_numpy(d).to(dev)
    god = torch.from_numpy(np.asarray(go, np.int64)).to(dev)
    if dtype == "e4m3":
        out = retrieval.rerank_topk_fp8(qd, dd, cand, off, k, doc_offset, SCALE, method="stream",
                                        ascending=True, group_off=god)
    else:
        out = retrieval.rerank_topk(qd, dd, cand, off, k, doc_offset, method="stream",
                                    ascending=True, group_off=god)
    s, i, n, g = (x.cpu().numpy() for x in out)
    return i, s, n, g


@pytest.mark.parametrize("dtype,D", [("bf16", 768), ("e4m3", 128)])
def test_gaussian_bits_are_the_streamed_candidate_route(gpu, dtype, D):
    """The main loop and tile origins are the pick's: float bits included."""
    torch.manual_seed(2026)
    Q, N, k, doc_offset = 70, 3000, 100, 7
    q = torch.nn.functional.normalize(torch.randn(Q, D))
    d = torch.nn.functional.normalize(torch.randn(N, D))
    if dtype == "e4m3":
        q, d = O.quantize_e4m3(q.numpy(), 16.0), O.quantize_e4m3(d.numpy(), 16.0)
    else:
        q, d = q.bfloat16().float().numpy(), d.bfloat16().float().numpy()
    go = _group_off(N, doc_offset, "many")
    got = _run(dtype, q, d, k, gpu, doc_offset, go)
    want = _stream_route(dtype, q, d, k, gpu, doc_offset, go)
    _bitwise(got, want)
    assert (got[2] == k).all() and len(np.unique(got[1])) > Q  # real, distinct scores


def test_poisoned_workspace(gpu):
    from irc_amd import _lib
    from irc_amd._torch import workspace

    Q, N, D, k, doc_offset, kind = 65, 4099, 128, 100, 5, "cycle"
    q, d, go, ref = _case_ref(Q, N, D, k, doc_offset, kind, "bf16")
    nbytes = int(_lib.fn("irc_scan_topk_grouped_workspace")(Q, len(go) - 1, k))
    ws = workspace(nbytes, torch.device(gpu), "scan_group_poison")
    ws.fill_(0xFF)
    got = _run("bf16", q, d, k, gpu, doc_offset, go, ws_tag="scan_group_poison")
    _bitwise(got, ref)


def test_query_chunks(gpu):
    Q, N, D, k, doc_offset = 600, 4099, 128, 10, 5
    q, d = _case(Q, N, D, doc_offset, "bf16")
    go = _group_off(N, doc_offset, "cycle")
    whole = _run("bf16", q, d, k, gpu, doc_offset, go)
    per_query = 8 * (len(go) - 1)
    assert 256 * per_query < 300 * per_query < Q * per_query  # chunks of 256: 256 + 256 + 88
    chunked = _run("bf16", q, d, k, gpu, doc_offset, go, max_workspace_bytes=300 * per_query)
    _bitwise(chunked, whole)
    tiny = _run("bf16", q, d, k, gpu, doc_offset, go, max_workspace_bytes=1)  # never below 256
    _bitwise(tiny, whole)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_shards_merge_to_the_one_shard_result(gpu, dtype):
    from irc_amd import retrieval

    Q, N, D, k, doc_offset, cut = 65, 4099, 128, 100, 5, 2000
    q, d, go, ref = _case_ref(Q, N, D, k, doc_offset, "cycle", dtype)
    g = np.searchsorted(go, doc_offset + cut, side="right") - 1
    assert go[g] < doc_offset + cut < go[g + 1]  # the boundary falls inside a group
    god = torch.from_numpy(go).to(gpu)
    ss, ii = [], []
    for lo, hi in ((0, cut), (cut, N)):
        g_lo, g_hi = retrieval.local_group_slice(god, doc_offset + lo, hi - lo)
        assert 0 <= g_lo < g_hi <= len(go) - 1 and g_hi - g_lo < len(go) - 1
        part = _run(dtype, q, d[lo:hi], k, gpu, doc_offset + lo, god[g_lo:g_hi + 1])
        ii.append(torch.from_numpy(part[0]).to(gpu))
        ss.append(torch.from_numpy(part[1]).to(gpu))
    s, i, n, grp = retrieval.topk_merge_grouped(torch.stack(ss), torch.stack(ii), k, god)
    _bitwise((i.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy(), grp.cpu().numpy()), ref)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_index_search_grouped(gpu, dtype):
    from irc_amd import retrieval

    Q, N, D, k, doc_offset = 20, 4099, 256, 50, 7
    rng = np.random.default_rng(11)
    # grid VALUES m / 256, |m| <= 15: exact in bf16; an fp8 index quantises them at scale 16
    q = torch.from_numpy(rng.integers(-15, 16, (Q, D)).astype(np.float32) / 256).to(gpu)
    d = torch.from_numpy(rng.integers(-15, 16, (N, D)).astype(np.float32) / 256).to(gpu)
    index = retrieval.ShardedDenseIndex(d, doc_offset=doc_offset, dtype=dtype)
    go = torch.from_numpy(_group_off(N, doc_offset, "cycle")).to(gpu)
    cand, off = _all_rows(Q, N, doc_offset, gpu)
    want = index.search_candidates(q, cand, off, k, method="stream", ascending=True,
                                   group_off=go)
    got = index.search(q, k, group_off=go)
    assert len(got) == 4
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and torch.equal(x, y)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert 0 < int(got[2].min()) and int(got[2].max()) < k  # fewer groups than k: padded
    again = index.search(q, k, group_off=go)  # the memoised slice of the same tensor object
    assert index._group_slice[0] is go
    for x, y in zip(again, got):
        assert torch.equal(x, y)
    # degenerate inputs: padding and n == 0, or n below k
    for name, g in (("no group", go[:1]),
                    ("every row outside", go.new_tensor([doc_offset + N, doc_offset + N + 50])),
                    ("before the shard", go.new_tensor([0, 3, doc_offset]))):
        s, i, n, grp = index.search(q, k, group_off=g)
        assert (n == 0).all() and (i == -1).all() and (grp == -1).all(), name
        assert torch.isneginf(s).all(), name
    three = go.new_tensor([doc_offset, doc_offset + 5, doc_offset + 5, doc_offset + 9,
                           doc_offset + 100])
    s, i, n, grp = index.search(q, k, group_off=three)  # k above the group count
    assert (n == 3).all() and (i[:, 3:] == -1).all() and torch.isneginf(s[:, 3:]).all()
    assert (grp[:, 3:] == -1).all()
    assert (grp[:, :3].sort(dim=1).values == grp.new_tensor([0, 2, 3])).all()


def test_main_dense_rerank_unit_page_runs(gpu, tmp_path, capsys, monkeypatch):
    import main as entry
    from irc_amd.retrieval import ShardedDenseIndex

    claims, cfg, cfg_path, ckpt = _hybrid_setup(tmp_path, gpu)
    calls = []
    search = ShardedDenseIndex.search

    def spy(self, queries, k, *a, **kw):
        out = search(self, queries, k, *a, **kw)
        calls.append((kw.get("group_off"), [x.cpu() for x in out]))
        return out

    monkeypatch.setattr(ShardedDenseIndex, "search", spy)
    entry.main(["--data", "fever", "--config", cfg_path, "--ckpt", ckpt, "--gpu", "0",
                "--retrieval", "dense", "--rerank-unit", "page"])
    out = capsys.readouterr().out
    assert "evidence recall@100 (pages): " in out
    n_claims = sum(1 for c in claims if c["label"] != "NOT ENOUGH INFO")
    assert out.count("batch of 1 claims") == n_claims and len(calls) == n_claims
    go0 = calls[0][0]
    pages = int((go0[1:] > go0[:-1]).sum())  # pages with a line
    for go, (s, i, n, g) in calls:
        assert go is go0  # one tensor object: the slice is computed once
        m = int(n[0])
        assert m == min(100, pages) and m > 0
        assert len(set(g[0, :m].tolist())) == m  # distinct pages
        assert (i[0, m:] == -1).all() and (g[0, m:] == -1).all()
        row_off = go.cpu()
        assert ((row_off[g[0, :m]] <= i[0, :m]) & (i[0, :m] < row_off[g[0, :m] + 1])).all()
