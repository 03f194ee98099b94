"""Candidate top-k over a sharded corpus on the GPU: the grouped merge
(irc_topk_merge_grouped, merge_collapse_kernel) against the numpy reference of
test_rerank_sharded_cpu.py, bit for bit; per-shard grouped calls merged against the reference
over the whole corpus; the collective ``search_candidates`` and ``predict_hybrid`` in two
ranks that share the one GPU (gloo carries the collectives, as in test_dist_gpu.py)."""
import argparse
import datetime
import functools
import os
import pickle
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG  # noqa: F401  (import paths)
from test_rerank_gpu import _hybrid_setup, _pack
from test_rerank_group_gpu import _bitwise, _call, _equal, _group_off, _lists, _operands, _ref
from test_rerank_sharded_cpu import _reference_merge_grouped

pytestmark = pytest.mark.gpu

WORLD = 2


# ---------------------------------------------------------------- the merge kernel
MERGE_SHAPES = [(1, 1, 1, 1), (2, 5, 7, 7), (3, 257, 100, 64), (2, 3, 100, 256),
                (8, 2, 1024, 1024)]  # the last: exactly the 8192 entries a query may have
MERGE_KINDS = ("scattered", "every_group_in_every_list", "no_shared_groups", "no_groups")


@functools.lru_cache(maxsize=None)
def _merge_case(shape, kind):
    """Lists made directly (no scoring): (scores [P, Q, kin], idx [P, Q, kin], group_off),
    scores from the integers -3 .. 3 so ties abound, ids unique within a query.
    "scattered": a quarter of the slots empty (-1, with a NaN score that must not be read)
    anywhere in the lists, groups of 0 .. 30 rows, rows below and above every group.
    "every_group_in_every_list": kin groups of P rows, list p holding row p of each.
    "no_shared_groups": every row a group of its own, lists sorted with their empty slots
    last, as a per-shard call returns them.  "no_groups": group_off of one entry."""
    P, Q, kin, kout = shape
    rng = np.random.default_rng(P * 100000 + Q * 1000 + kin)
    L = P * kin
    R = 4 * L + 50
    sc = rng.integers(-3, 4, (P, Q, kin)).astype(np.float32)
    if kind == "every_group_in_every_list":
        go = 7 + P * np.arange(kin + 1, dtype=np.int64)
        idx = np.empty((P, Q, kin), np.int64)
        for r in range(Q):
            for p in range(P):
                idx[p, r] = go[:-1][rng.permutation(kin)] + (p + r) % P
        return sc, idx, go
    idx = np.stack([rng.permutation(R)[:L].reshape(P, kin) for _ in range(Q)], axis=1)
    idx = idx.astype(np.int64)
    empty = rng.random((P, Q, kin)) < 0.25
    if Q > 1:
        empty[P - 1, 1] = True  # one all-empty list
    idx[empty] = -1
    if kind == "no_shared_groups":
        go = np.arange(R + 1, dtype=np.int64)
        order = np.lexsort((idx, -sc, idx < 0), axis=2)  # (score desc, id asc), empties last
        idx, sc = np.take_along_axis(idx, order, 2), np.take_along_axis(sc, order, 2)
        sc[idx < 0] = -np.inf
        return sc, idx, go
    sc[idx < 0] = np.nan
    if kind == "no_groups":
        return sc, idx, np.array([5], np.int64)
    sizes, go = [0, 1, 2, 5, 9, 30], [3]
    while go[-1] + sizes[(len(go) - 1) % 6] <= R - 20:
        go.append(go[-1] + sizes[(len(go) - 1) % 6])
    return sc, idx, np.asarray(go, np.int64)


def _merge_gpu(sc, idx, k, go, dev):
    from irc_amd import retrieval

    out = retrieval.topk_merge_grouped(torch.from_numpy(sc).to(dev), torch.from_numpy(idx).to(dev),
                                       k, torch.from_numpy(go).to(dev))
    s, i, n, g = (x.cpu().numpy() for x in out)
    assert n.dtype == np.int32 and g.dtype == np.int64
    return i, s, n, g


@pytest.mark.parametrize("kind", MERGE_KINDS)
@pytest.mark.parametrize("shape", MERGE_SHAPES)
def test_grouped_merge_is_the_reference_bit_for_bit(gpu, shape, kind):
    P, Q, kin, kout = shape
    sc, idx, go = _merge_case(shape, kind)
    want = _reference_merge_grouped(sc, idx, kout, go)
    got = _merge_gpu(sc, idx, kout, go, gpu)
    _bitwise(got, want)
    if kind == "every_group_in_every_list":
        assert (want[2] == min(kout, kin)).all()  # the count is the group count
    elif kind == "no_groups":
        assert (got[2] == 0).all() and (got[0] == -1).all() and np.isneginf(got[1]).all()
    elif kind == "no_shared_groups":
        from irc_amd import retrieval

        s, i = retrieval.topk_merge(torch.from_numpy(sc).to(gpu), torch.from_numpy(idx).to(gpu),
                                    kout)
        np.testing.assert_array_equal(got[0], i.cpu().numpy())
        np.testing.assert_array_equal(got[1].view(np.uint32), s.cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(got[2], (got[0] >= 0).sum(1))
    elif P * kin > 4:
        present = [np.unique(np.searchsorted(go, x[(x >= go[0]) & (x < go[-1])], side="right"))
                   .size for x in (idx[:, r].ravel() for r in range(Q))]
        filled = [(x >= 0).sum() for x in (idx[:, r].ravel() for r in range(Q))]
        np.testing.assert_array_equal(want[2], np.minimum(kout, present))
        assert (np.asarray(present) < np.asarray(filled)).any()  # something was collapsed


def test_grouped_merge_runs_twice_to_the_same_bits(gpu):
    # a workspace that holds the previous call's keys must not matter, nor the launch
    shape = MERGE_SHAPES[2]
    sc, idx, go = _merge_case(shape, "scattered")
    big = _merge_case(MERGE_SHAPES[4], "scattered")
    a = _merge_gpu(sc, idx, shape[3], go, gpu)
    _merge_gpu(big[0], big[1], 1024, big[2], gpu)
    b = _merge_gpu(sc, idx, shape[3], go, gpu)
    _bitwise(a, b)


# ---------------------------------------------------------------- sharded = unsharded
N, D, Q, K = 4099, 128, 20, 50


@functools.lru_cache(maxsize=None)
def _grid_corpus(dtype):
    """Integer-grid operands, "cycle" groups over the whole corpus, lists over all of it
    and the reference over the whole corpus: computed once, left unchanged."""
    rng = np.random.default_rng(4099 + len(dtype))
    q, d = _operands(rng, dtype, Q, N, D)
    go = _group_off(N, 0, "cycle")
    lists = _lists(rng, Q, N, K, 0, go)
    return q, d, lists, go, _ref(dtype, q, d, lists, K, go, 0)


def _sharded_merge(dtype, q, d, lists, go, shards, method, dev):
    from irc_amd import retrieval

    cand, off = _pack(lists, dev)
    god = torch.from_numpy(go).to(dev)
    qd = torch.from_numpy(q).to(dev)
    ss, ii = [], []
    for p in range(shards):
        lo, hi = retrieval.shard_bounds(d.shape[0], shards, p)
        if 0 < lo < d.shape[0]:  # the boundary falls inside a group
            g = np.searchsorted(go, lo, side="right") - 1
            assert go[g] < lo < go[g + 1]
        s, i, n, g = _call(dtype, qd, torch.from_numpy(d[lo:hi]).to(dev), cand, off, K, lo,
                           method, True, god)
        ss.append(s)
        ii.append(i)
    out = retrieval.topk_merge_grouped(torch.stack(ss), torch.stack(ii), K, god)
    s, i, n, g = (x.cpu().numpy() for x in out)
    return i, s, n, g


@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("method", ["gather", "stream"])
@pytest.mark.parametrize("dtype", ["bf16", "e4m3"])
def test_per_shard_calls_merge_to_the_whole_corpus_reference(gpu, dtype, method, shards):
    q, d, lists, go, ref = _grid_corpus(dtype)
    got = _sharded_merge(dtype, q, d, lists, go, shards, method, gpu)
    _equal(got, ref)
    # pages collapsed: fewer groups than eligible rows in some list
    assert (ref[2] < [min(K, np.count_nonzero(x < N)) for x in lists]).any()


@pytest.mark.parametrize("dtype", ["bf16", "e4m3"])
def test_gaussian_shards_merge_to_the_one_shard_call(gpu, dtype):
    """Gathered scoring sums in one order per (query, row) whatever the shard, so the merged
    result is the one-shard call's, bit for bit."""
    from oracle import irc_oracle as O

    torch.manual_seed(77)
    q = torch.nn.functional.normalize(torch.randn(Q, D))
    d = torch.nn.functional.normalize(torch.randn(N, D))
    if dtype == "e4m3":
        q, d = O.quantize_e4m3(q.numpy(), 16.0), O.quantize_e4m3(d.numpy(), 16.0)
    else:
        q, d = q.bfloat16().float().numpy(), d.bfloat16().float().numpy()
    go = _group_off(N, 0, "cycle")
    lists = _lists(np.random.default_rng(77), Q, N, K, 0, go)
    cand, off = _pack(lists, gpu)
    s, i, n, g = (x.cpu().numpy() for x in _call(
        dtype, torch.from_numpy(q).to(gpu), torch.from_numpy(d).to(gpu), cand, off, K, 0,
        "gather", True, torch.from_numpy(go).to(gpu)))
    one = (i, s, n, g)
    assert n.max() > 1
    for shards in (2, 3):
        _bitwise(_sharded_merge(dtype, q, d, lists, go, shards, "gather", gpu), one)


# ---------------------------------------------------------------- two ranks, one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD,
                            timeout=datetime.timedelta(seconds=60))


INDEX_CASES = [("bf16", "gather"), ("bf16", "stream"), ("fp8", "auto")]
SPLIT = (13, 7)


@functools.lru_cache(maxsize=None)
def _index_corpus():
    """Grid VALUES m / 256, |m| <= 15: exact in bf16, and an fp8 index quantises them at
    scale 16 to the codes of m / 16, so every score is exact on both kinds of index."""
    rng = np.random.default_rng(13)
    q = rng.integers(-15, 16, (Q, D)).astype(np.float32) / 256
    d = rng.integers(-15, 16, (N, D)).astype(np.float32) / 256
    go = _group_off(N, 0, "cycle")
    return q, d, _lists(rng, Q, N, K, 0, go), go


def _search_all(index, q, lists, go, method, dev):
    """Ungrouped and grouped search_candidates of one index, as numpy arrays."""
    cand, off = _pack(lists, dev, torch.int64 if len(lists) == SPLIT[0] else torch.int32)
    qd = torch.from_numpy(q).to(dev)
    out = []
    for god in (None, torch.from_numpy(go).to(dev)):
        res = index.search_candidates(qd, cand, off, K, method=method, ascending=True,
                                      group_off=god)
        assert len(res) == (3 if god is None else 4)
        out.append([x.cpu().numpy() for x in res])
    return out


def _index_worker(rank, port, out_dir):
    _init(rank, port)
    try:
        from irc_amd import retrieval

        dev = torch.device("cuda:0")
        q, d, lists, go = _index_corpus()
        lo, hi = retrieval.shard_bounds(N, WORLD, rank)
        a = sum(SPLIT[:rank])
        b = a + SPLIT[rank]
        for dtype, method in INDEX_CASES:
            index = retrieval.ShardedDenseIndex(torch.from_numpy(d[lo:hi]).to(dev), doc_offset=lo,
                                                group=dist.group.WORLD, dtype=dtype)
            res = _search_all(index, q[a:b], lists[a:b], go, method, dev)
            with open(os.path.join(out_dir, f"{dtype}_{method}_r{rank}.pkl"), "wb") as f:
                pickle.dump(res, f)
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_rank_results(gpu, tmp_path_factory):
    out = tmp_path_factory.mktemp("sharded_index")
    mp.start_processes(_index_worker, args=(_free_port(), str(out)), nprocs=WORLD, join=True,
                       start_method="spawn")
    return out


@pytest.mark.parametrize("dtype,method", INDEX_CASES)
def test_two_ranks_equal_the_single_process_index(gpu, two_rank_results, dtype, method):
    from irc_amd import retrieval

    q, d, lists, go = _index_corpus()
    g = np.searchsorted(go, retrieval.shard_bounds(N, WORLD, 1)[0], side="right") - 1
    assert go[g] < retrieval.shard_bounds(N, WORLD, 1)[0] < go[g + 1]  # a group is cut
    index = retrieval.ShardedDenseIndex(torch.from_numpy(d).to(gpu), dtype=dtype)
    want = _search_all(index, q, lists, go, method, gpu)
    assert (want[1][2] < want[0][2]).any()  # pages collapsed
    for r in range(WORLD):
        with open(two_rank_results / f"{dtype}_{method}_r{r}.pkl", "rb") as f:
            got = pickle.load(f)
        _bitwise(got[0], want[0])
        _bitwise(got[1], want[1])


# ---------------------------------------------------------------- predict_hybrid, two ranks
UNITS = ("page", "line")
HK = 5


def _predict_recorded(args):
    """predict_hybrid with every hybrid_search result recorded: ([per batch: arrays], recall)"""
    import src.evaluation as E

    seen, orig = [], E.hybrid_search

    def recording(*a, **kw):
        out = orig(*a, **kw)
        seen.append([x.cpu().numpy() for x in out])
        return out

    E.hybrid_search = recording
    try:
        recall = E.predict_hybrid(args, k=HK)
    finally:
        E.hybrid_search = orig
    return seen, recall


def _hybrid_args(cfg, ckpt, dev, unit, **kw):
    return argparse.Namespace(config=cfg, data="fever", ckpt=ckpt, device=dev, retrieval="hybrid",
                              rerank_unit=unit, **kw)


def _hybrid_worker(rank, port, cfg, ckpt, out_dir):
    _init(rank, port)
    try:
        dev = torch.device("cuda:0")
        for unit in UNITS:
            args = _hybrid_args(cfg, ckpt, dev, unit, dist_group=dist.group.WORLD, rank=rank,
                                world_size=WORLD)
            with open(os.path.join(out_dir, f"{unit}_r{rank}.pkl"), "wb") as f:
                pickle.dump(_predict_recorded(args), f)
    finally:
        dist.destroy_process_group()


def test_predict_hybrid_in_two_ranks(gpu, tmp_path):
    """The claims and the corpus are embedded in other batches than in one process (other
    padding), so a score may move in its last bits: asserted is what rounding cannot move."""
    from irc_amd.retrieval import expand_ranges
    from irc_amd.sparse import SparseIndex, load_sparse_csr
    from src.dataset import get_dataloader
    from src.evaluation import hybrid_corpus

    claims, cfg, _, ckpt = _hybrid_setup(tmp_path, gpu)
    cfg["eval"]["batch_size"] = 4
    mp.start_processes(_hybrid_worker, args=(_free_port(), cfg, ckpt, str(tmp_path)),
                       nprocs=WORLD, join=True, start_method="spawn")
    # each claim's candidate rows, and each row's page
    loader = get_dataloader(_hybrid_args(cfg, ckpt, gpu, "line"), train=False, distributed=False)
    _, meta = load_sparse_csr(cfg["dataset"]["tfidf"])
    counts, _ = load_sparse_csr(cfg["dataset"]["inverted_file"])
    sparse_index = SparseIndex(counts, ngram=meta["ngram"], device=gpu)
    titles, texts, row_off = hybrid_corpus(loader.dataset.wiki, meta["doc_dict"][1])
    row_off_d = torch.tensor(row_off, dtype=torch.int64, device=gpu)
    cand_rows = []
    for batch in loader:
        c, off = sparse_index.candidates([x["claim"] for x in batch], False)
        rows, rows_off = expand_ranges(c, off, row_off_d)
        rows, rows_off = rows.cpu().numpy(), rows_off.cpu().numpy()
        cand_rows.append([set(rows[rows_off[r]:rows_off[r + 1]].tolist())
                          for r in range(len(batch))])
    assert len(cand_rows) > 1
    for unit in UNITS:
        single, recall1 = _predict_recorded(_hybrid_args(cfg, ckpt, gpu, unit))
        got = []
        for r in range(WORLD):
            with open(tmp_path / f"{unit}_r{r}.pkl", "rb") as f:
                got.append(pickle.load(f))
        (seen0, recall0), (seen1, recall_b) = got
        assert recall0 == recall_b and 0.0 <= recall0 <= 1.0
        assert len(seen0) == len(seen1) == len(single) == len(cand_rows)
        for b, (x, y, one) in enumerate(zip(seen0, seen1, single)):
            assert len(x) == len(one) == (4 if unit == "page" else 3)
            _bitwise(x, y)  # both ranks hold the same result for the whole batch
            s, i, n = x[:3]
            assert i.shape == (len(cand_rows[b]), HK)
            np.testing.assert_array_equal(n, one[2])
            for r, rows in enumerate(cand_rows[b]):
                m = int(n[r])
                ret = i[r, :m].tolist()
                assert set(ret) <= rows and len(set(ret)) == m
                assert (i[r, m:] == -1).all()
                if unit == "page":
                    pages = [titles[j] for j in ret]
                    assert len(set(pages)) == m  # distinct pages
                    assert [titles[row_off[c]] for c in x[3][r, :m]] == pages
