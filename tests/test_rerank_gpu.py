"""Candidate-restricted dense top-k (irc_rerank_topk) against a small numpy reference:
gather the candidate rows, fp64 dot product rounded to fp32, rank by (score desc, global
id asc) -- and the sparse-filter -> dense-rerank pipeline built on it (hybrid_search,
main.py --retrieval hybrid; reference src/evaluation.py:57-83 feeding :110-112)."""
import argparse

import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (import paths)
from oracle import irc_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the project's fp32 accumulation-order tolerance on unit vectors at D = 768


def _grid(rng, shape, lim=127):  # the recipe of test_scan_gpu.py
    return rng.integers(-lim, lim + 1, shape).astype(np.float32) / 128


def _pack(lists, dev, dtype=torch.int32):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, np.int64) for x in lists]) if off[-1] else \
        np.zeros(0, np.int64)
    return torch.from_numpy(flat).to(dtype).to(dev), torch.from_numpy(off).to(dev)


def _reference(q, d, lists, k, doc_offset=0):
    """(idx [Q, k], scores [Q, k], n [Q]) of the eligible candidates of each list."""
    Q, N = q.shape[0], d.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_s = np.full((Q, k), -np.inf, np.float32)
    out_n = np.zeros(Q, np.int32)
    q64, d64 = q.astype(np.float64), d.astype(np.float64)
    for r, ids in enumerate(lists):
        ids = np.asarray(ids, np.int64)
        ok = np.sort(ids[(ids >= doc_offset) & (ids < doc_offset + N)])
        if ok.size == 0:
            continue
        sc = (d64[ok - doc_offset] @ q64[r]).astype(np.float32)
        ti, ts = O.topk_rows(sc[None, :], k)  # positions in ascending ids: ties -> lower id
        m = min(k, ok.size)
        out_i[r, :m] = ok[ti[0, :m]]
        out_s[r, :m] = ts[0, :m]
        out_n[r] = m
    return out_i, out_s, out_n


def _run(q, d, lists, k, dev, doc_offset=0, dtype=torch.int32):
    from irc_amd import retrieval

    cand, off = _pack(lists, dev, dtype)
    s, i, n = retrieval.rerank_topk(torch.from_numpy(q).to(dev), torch.from_numpy(d).to(dev),
                                    cand, off, k, doc_offset)
    return i.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()


def _lengths(k, N):
    from irc_amd.retrieval import RERANK_CHUNK as C

    return [min(max(x, 0), N) for x in (0, 1, k - 1, k, k + 1, C - 1, C, C + 1, 3 * C + 7, N)]


GRID_CASES = [(1, 1, 64, 1, 0), (3, 40, 128, 8, 11), (33, 4099, 64, 10, 0),
              (257, 4099, 128, 100, 5), (16, 20000, 768, 1024, 3), (7, 9000, 1024, 1, 0),
              # the other widths of the one scoring body; Q = 10 is the whole cycle of
              # lengths, 1393 candidates: chunks that span several owners
              (10, 300, 256, 8, 0), (10, 300, 384, 8, 7), (10, 300, 512, 8, 0)]


def _grid_case(Q, N, D, k, doc_offset):
    rng = np.random.default_rng(Q * 1000 + D)
    q = _grid(rng, (Q, D), 3)
    d = _grid(rng, (N, D), 3)
    lens = _lengths(k, N)
    # the few queries of Q = 1 / 3 / 7 start the cycle past its empty head: 1 / k - 1,
    # k, k + 1 / k .. all N
    start = {1: 1, 3: 2, 7: 3}.get(Q, 0)
    want = [lens[(r + start) % len(lens)] for r in range(Q)]
    if Q == 33:
        want[0] = want[-1] = 0  # the first and the last query empty
    if Q == 257:
        want[30:230] = [3] * 200  # many lists share one scoring chunk
    lists = [doc_offset + np.sort(rng.choice(N, n, replace=False)) for n in want]
    return q, d, lists


@pytest.mark.parametrize("Q,N,D,k,doc_offset", GRID_CASES)
def test_bit_exact_on_integer_grids(gpu, Q, N, D, k, doc_offset):
    q, d, lists = _grid_case(Q, N, D, k, doc_offset)
    ri, rs, rn = _reference(q, d, lists, k, doc_offset)
    i, s, n = _run(q, d, lists, k, gpu, doc_offset)
    np.testing.assert_array_equal(n, rn)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)


def test_all_lists_empty_fill_padding(gpu):
    rng = np.random.default_rng(1)
    q, d = _grid(rng, (5, 64), 3), _grid(rng, (9, 64), 3)
    i, s, n = _run(q, d, [[]] * 5, 7, gpu)
    assert (i == -1).all() and np.isneginf(s).all() and (n == 0).all()


def test_int64_ids_beyond_int32_are_foreign_not_wrapped(gpu):
    rng = np.random.default_rng(4)
    q, d = _grid(rng, (2, 64), 3), _grid(rng, (50, 64), 3)
    ids = np.array([3, 7, 41], np.int64)
    wide = np.concatenate([ids, ids + 2 ** 32, ids - 2 ** 32, [2 ** 31, -2 ** 31 - 1]])
    a = _run(q, d, [ids, ids[::-1].copy()], 8, gpu, dtype=torch.int64)
    b = _run(q, d, [wide, rng.permutation(wide)], 8, gpu, dtype=torch.int64)
    ri, rs, rn = _reference(q, d, [ids, ids], 8)
    for x, y, r in zip(a, b, (ri, rs, rn)):
        np.testing.assert_array_equal(x, r)
        np.testing.assert_array_equal(y, r)


def test_order_independence(gpu):
    Q, N, D, k, doc_offset = GRID_CASES[3]
    q, d, lists = _grid_case(Q, N, D, k, doc_offset)
    rng = np.random.default_rng(9)
    shuffled = [rng.permutation(x) for x in lists]
    a = _run(q, d, lists, k, gpu, doc_offset)
    b = _run(q, d, shuffled, k, gpu, doc_offset, dtype=torch.int64)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def test_sharded_calls_merge_to_the_unsharded_result(gpu):
    from irc_amd import retrieval

    rng = np.random.default_rng(3)
    Q, N, D, k = 12, 7001, 128, 64
    q, d = _grid(rng, (Q, D), 2), _grid(rng, (N, D), 2)
    want = [0, 1, 63, 64, 65, 255, 256, 257, 775, 7001, 3000, 0]
    lists = []
    for n in want:
        ids = np.sort(rng.choice(N, n, replace=False)).astype(np.int64)
        # ids no shard owns: negative, and N or above
        lists.append(np.concatenate([[-5, -1], ids, [N, N + 1, N + 4000]]))
    cand, off = _pack(lists, gpu)
    qd = torch.from_numpy(q).to(gpu)
    parts = []
    for r in range(3):
        a, b = retrieval.shard_bounds(N, 3, r)
        parts.append(retrieval.rerank_topk(qd, torch.from_numpy(d[a:b]).to(gpu), cand, off, k, a))
    ms, mi = retrieval.topk_merge(torch.stack([p[0] for p in parts]),
                                  torch.stack([p[1] for p in parts]), k)
    us, ui, un = retrieval.rerank_topk(qd, torch.from_numpy(d).to(gpu), cand, off, k, 0)
    np.testing.assert_array_equal(mi.cpu().numpy(), ui.cpu().numpy())
    np.testing.assert_array_equal(ms.cpu().numpy(), us.cpu().numpy())
    ri, rs, rn = _reference(q, d, lists, k)
    np.testing.assert_array_equal(ui.cpu().numpy(), ri)
    np.testing.assert_array_equal(us.cpu().numpy(), rs)
    np.testing.assert_array_equal(un.cpu().numpy(), rn)


@pytest.fixture(scope="module")
def gaussian():
    torch.manual_seed(2025)
    q = torch.nn.functional.normalize(torch.randn(16, 768)).bfloat16()
    d = torch.nn.functional.normalize(torch.randn(20000, 768)).bfloat16()
    q, d = q.float().numpy(), d.float().numpy()
    full = (q.astype(np.float64) @ d.astype(np.float64).T)  # fp64 scores of every pair
    return q, d, full


def test_fixed_accumulation_order(gpu, gaussian):
    """A doc's score for a query is bitwise the same in a 5-element list and at position
    12,345 of a 20,000-element list."""
    q, d, full = gaussian
    top = np.argsort(-full[0])[:5]
    rng = np.random.default_rng(7)
    rest = rng.permutation(np.setdiff1d(np.arange(20000), top))
    long_list = np.concatenate([rest[:12345], top[:1], rest[12345:15000], top[1:], rest[15000:]])
    assert long_list[12345] == top[0] and long_list.size == 20000
    qq = np.stack([q[0], q[0]])
    i, s, n = _run(qq, d, [top[::-1].copy(), long_list], 5, gpu)
    assert n.tolist() == [5, 5]
    np.testing.assert_array_equal(i[0], i[1])
    np.testing.assert_array_equal(s[0].view(np.uint32), s[1].view(np.uint32))
    assert top[0] in i[0]


def test_gaussian_margin_aware(gpu, gaussian):
    q, d, full = gaussian
    rng = np.random.default_rng(2025)
    lens = [0, 1, 99, 100, 101, 3000, 3000, 5000, 777, 2048, 2049, 4096, 10000, 20000, 256, 513]
    lists = [np.sort(rng.choice(20000, n, replace=False)) for n in lens]
    k = 100
    i, s, n = _run(q, d, lists, k, gpu)
    ri, rs, rn = _reference(q, d, lists, k)
    np.testing.assert_array_equal(n, rn)
    ndiff = 0
    for r in range(16):
        m = int(rn[r])
        assert (i[r, m:] == -1).all() and np.isneginf(s[r, m:]).all()
        assert set(i[r, :m]) <= set(lists[r].tolist())
        np.testing.assert_allclose(s[r, :m], full[r, i[r, :m]], atol=TOL)
        assert np.all(np.diff(s[r, :m]) <= 0)
        diff = set(i[r, :m]) ^ set(ri[r, :m])
        ndiff += len(diff)
        for doc in diff:
            assert abs(full[r, doc] - rs[r, m - 1]) <= 2 * TOL
    print(f"symmetric differences over the 16 queries: {ndiff}")
    assert ndiff <= 8


def _hybrid_setup(tmp_path, gpu):
    from test_predict_gpu import _checkpoint, _config, _fever_files

    claims, counts, titles = _fever_files(tmp_path)
    cfg, cfg_path = _config(tmp_path)
    ckpt = _checkpoint(tmp_path, cfg)
    return claims, cfg, cfg_path, ckpt


def test_hybrid_search_end_to_end(gpu, tmp_path):
    from irc_amd.retrieval import ShardedDenseIndex
    from irc_amd.sparse import SparseIndex, load_sparse_csr
    from src.dataset import get_dataloader
    from src.evaluation import encode_corpus, hybrid_corpus, hybrid_search
    from src.model import load_model

    claims, cfg, _, ckpt = _hybrid_setup(tmp_path, gpu)
    cfg["eval"]["batch_size"] = 4
    args = argparse.Namespace(config=cfg, data="fever", ckpt=ckpt, device=gpu,
                              retrieval="hybrid")
    _, model, _, _ = load_model(ckpt)
    model = model.to(gpu).eval()
    loader = get_dataloader(args, train=False, distributed=False)
    _, meta = load_sparse_csr(cfg["dataset"]["tfidf"])
    counts, _ = load_sparse_csr(cfg["dataset"]["inverted_file"])
    sparse_index = SparseIndex(counts, ngram=meta["ngram"], device=gpu)
    titles, texts, row_off = hybrid_corpus(loader.dataset.wiki, meta["doc_dict"][1])
    assert len(row_off) == counts.shape[1] + 1 and row_off[-1] == len(texts) > 0
    with torch.no_grad():
        emb = encode_corpus(model, texts, gpu)
    index = ShardedDenseIndex(emb)
    d64 = index.docs.float().cpu().numpy().astype(np.float64)
    row_off_d = torch.tensor(row_off, dtype=torch.int64, device=gpu)
    k, seen = 5, 0
    for batch in loader:
        texts_c = [x["claim"] for x in batch]
        s, i, n = hybrid_search(model, index, sparse_index, row_off_d, texts_c, k, gpu)
        s, i, n = s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()
        with torch.no_grad():
            q64 = model.ctx2vec(texts_c, gpu).bfloat16().float().cpu().numpy().astype(np.float64)
        cols = sparse_index.documents_filtering(texts_c, False)
        for r in range(len(batch)):
            rows = np.array([j for c in cols[r] for j in range(row_off[c], row_off[c + 1])],
                            np.int64)
            m = min(k, rows.size)
            assert n[r] == m
            assert (i[r, m:] == -1).all()
            assert set(i[r, :m]) <= set(rows.tolist())  # nothing the filter excluded
            if m == 0:
                continue
            sc = d64[rows] @ q64[r]
            ri, rs = O.topk_rows(sc.astype(np.float32)[None, :], k)
            ref_ids = rows[ri[0, :m]]
            full = dict(zip(rows.tolist(), sc))
            np.testing.assert_allclose(s[r, :m], [full[j] for j in i[r, :m]], atol=TOL)
            for doc in set(i[r, :m]) ^ set(ref_ids):
                assert abs(full[doc] - rs[0, m - 1]) <= 2 * TOL
            seen += 1 if m else 0
        assert len(batch) <= 4
    n_claims = sum(1 for c in claims if c["label"] != "NOT ENOUGH INFO")
    assert len(loader.dataset) == n_claims
    assert seen > 0


def test_main_retrieval_hybrid_runs(gpu, tmp_path, capsys):
    import main as entry
    from src.evaluation import predict

    claims, cfg, cfg_path, ckpt = _hybrid_setup(tmp_path, gpu)
    entry.main(["--data", "fever", "--config", cfg_path, "--ckpt", ckpt, "--gpu", "0",
                "--retrieval", "hybrid"])
    out = capsys.readouterr().out
    assert "evidence recall@100" in out
    n_claims = sum(1 for c in claims if c["label"] != "NOT ENOUGH INFO")
    assert out.count("batch of 1 claims") == n_claims
    cfg["eval"]["batch_size"] = 4
    hyb = predict(argparse.Namespace(config=cfg, data="fever", ckpt=ckpt, device=gpu,
                                     retrieval="hybrid"), k=100)
    assert 0.0 <= hyb <= 1.0
    import json

    with open(cfg["dataset"]["small_wiki"]) as f:
        n_rows = sum(len([x for x in p["lines"].split("\n") if x.strip()])
                     for p in json.load(f).values())
    dense = predict(argparse.Namespace(config=cfg, data="fever", ckpt=ckpt, device=gpu,
                                       retrieval="dense"), k=min(n_rows, 1024))
    assert hyb <= dense
