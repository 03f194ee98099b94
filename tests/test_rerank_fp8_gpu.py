"""Candidate-restricted top-k on e4m3 shards (irc_rerank_topk_fp8, irc_rerank_topk_stream_fp8,
retrieval.rerank_topk_fp8, ShardedDenseIndex(dtype="fp8").search_candidates) against numpy
on the decoded codes: O.dequantize_e4m3, fp64 dot products cast to fp32, O.topk_rows over
ids sorted ascending, times np.float32(score_scale) -- _reference of test_rerank_gpu.py
applied to decoded codes."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (import paths)
from oracle import irc_oracle as O
from test_rerank_gpu import _hybrid_setup, _lengths, _pack, _reference

pytestmark = pytest.mark.gpu

METHODS = ("gather", "stream")
SCALE = 1.0 / 256  # codes hold 16 x the value: 1 / 16^2
TOL = 1e-5  # test_scan_fp8_gpu.py: fp32 accumulation order on D = 768 products of e4m3 values


def _codes(rng, shape, lim=3):
    # m / 16, |m| <= lim: exact in e4m3; |sum| <= 1024 * 9 / 256 < 2^24 / 256, exact in any order
    return O.quantize_e4m3(rng.integers(-lim, lim + 1, shape).astype(np.float32) / 16)


def _ref8(qc, dc, lists, k, doc_offset=0, scale=SCALE):
    i, s, n = _reference(O.dequantize_e4m3(qc), O.dequantize_e4m3(dc), lists, k, doc_offset)
    return i, (s * np.float32(scale)).astype(np.float32), n


def _run8(qc, dc, lists, k, dev, doc_offset=0, dtype=torch.int32, method="gather",
          ascending=True, scale=SCALE):
    from irc_amd import retrieval

    cand, off = _pack(lists, dev, dtype)
    s, i, n = retrieval.rerank_topk_fp8(torch.from_numpy(qc).to(dev), torch.from_numpy(dc).to(dev),
                                        cand, off, k, doc_offset, scale, method=method,
                                        ascending=ascending)
    return i.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()


def _same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


GATHER_CASES = [(1, 1, 128, 1, 0), (3, 40, 128, 8, 11), (33, 4099, 64, 10, 0),
                (257, 4099, 128, 100, 5), (16, 20000, 768, 1024, 3), (7, 9000, 1024, 1, 0),
                # the other widths of the one scoring body; Q = 5 starts the cycle at C - 1:
                # 1368 candidates, chunks that span several owners
                (5, 300, 256, 8, 0), (5, 300, 384, 8, 7), (5, 300, 512, 8, 0)]
# (5, 200, 128): one partial doc tile; (257, 4099, 384): three K-tiles, a second query tile
# of one row, a last doc tile of 3 docs
STREAM_CASES = [c for c in GATHER_CASES if c[2] != 64] + [(5, 200, 128, 8, 0),
                                                          (257, 4099, 384, 100, 5)]


def _grid_case(Q, N, D, k, doc_offset):
    """_grid_case of test_rerank_gpu.py with e4m3 codes: lengths cycle through 0, 1, k - 1,
    k, k + 1, C - 1, C, C + 1, 3 C + 7, N (C = RERANK_CHUNK)."""
    rng = np.random.default_rng(Q * 1000 + D)
    q = _codes(rng, (Q, D))
    d = _codes(rng, (N, D))
    lens = _lengths(k, N)
    start = {1: 1, 3: 2, 7: 3, 5: 5}.get(Q, 0)  # few queries: past the cycle's empty head
    want = [lens[(r + start) % len(lens)] for r in range(Q)]
    if Q == 33:
        want[0] = want[-1] = 0  # the first and the last query empty
    if Q == 257:
        want[30:230] = [3] * 200  # many lists share one scoring chunk
    lists = [doc_offset + np.sort(rng.choice(N, n, replace=False)) for n in want]
    return q, d, lists


@pytest.mark.parametrize("Q,N,D,k,doc_offset", GATHER_CASES)
def test_gather_bit_exact_on_e4m3_grids(gpu, Q, N, D, k, doc_offset):
    q, d, lists = _grid_case(Q, N, D, k, doc_offset)
    ri, rs, rn = _ref8(q, d, lists, k, doc_offset)
    i, s, n = _run8(q, d, lists, k, gpu, doc_offset)
    np.testing.assert_array_equal(n, rn)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)


@pytest.mark.parametrize("Q,N,D,k,doc_offset", STREAM_CASES)
def test_stream_bit_exact_on_e4m3_grids(gpu, Q, N, D, k, doc_offset):
    q, d, lists = _grid_case(Q, N, D, k, doc_offset)
    ri, rs, rn = _ref8(q, d, lists, k, doc_offset)
    got = _run8(q, d, lists, k, gpu, doc_offset, method="stream")
    np.testing.assert_array_equal(got[2], rn)
    np.testing.assert_array_equal(got[0], ri)
    np.testing.assert_array_equal(got[1], rs)
    # the two methods agree bitwise wherever every fp32 order is exact
    _same(got, _run8(q, d, lists, k, gpu, doc_offset, method="gather"))


def test_stream_lists_confined_to_two_doc_tiles(gpu):
    """Every list lies in doc tiles 1 and 2 of 17: most workgroups take the early return."""
    from irc_amd.retrieval import RERANK_STREAM_TILE as T

    Q, N, D, k = 9, 16 * T + 37, 128, 32
    rng = np.random.default_rng(77)
    q, d = _codes(rng, (Q, D)), _codes(rng, (N, D))
    inside = np.arange(T, 3 * T)
    sizes = [1, 2, k - 1, k, k + 1, T, 300, inside.size, 0]
    lists = [13 + np.sort(rng.choice(inside, n, replace=False)) for n in sizes]
    got = _run8(q, d, lists, k, gpu, 13, method="stream")
    _same(got, _ref8(q, d, lists, k, 13))
    _same(got, _run8(q, d, lists, k, gpu, 13, method="gather"))


@pytest.mark.parametrize("method", METHODS)
def test_unsorted_and_int64_lists(gpu, method):
    Q, N, D, k, doc_offset = GATHER_CASES[3]
    q, d, lists = _grid_case(Q, N, D, k, doc_offset)
    rng = np.random.default_rng(9)
    shuffled = [rng.permutation(x) for x in lists]
    a = _run8(q, d, lists, k, gpu, doc_offset, method=method)
    b = _run8(q, d, shuffled, k, gpu, doc_offset, dtype=torch.int64, method=method,
              ascending=False)
    _same(a, b)
    # int64 ids that do not fit int32, and negative ids, are foreign: never wrapped
    q2, d2 = _codes(rng, (2, 128)), _codes(rng, (50, 128))
    ids = np.array([3, 7, 41], np.int64)
    wide = np.concatenate([ids, ids + 2 ** 32, ids - 2 ** 32, [2 ** 31, -2 ** 31 - 1]])
    ref = _ref8(q2, d2, [ids, ids], 8)
    _same(_run8(q2, d2, [wide, rng.permutation(wide)], 8, gpu, dtype=torch.int64, method=method,
                ascending=False), ref)
    _same(_run8(q2, d2, [np.sort(wide), np.sort(wide)], 8, gpu, dtype=torch.int64,
                method=method, ascending=True), ref)


@pytest.mark.parametrize("method", METHODS)
def test_shards_merge_to_the_unsharded_result(gpu, method):
    from irc_amd import retrieval

    rng = np.random.default_rng(3)
    Q, N, D, k = 12, 7001, 128, 64
    q, d = _codes(rng, (Q, D), 2), _codes(rng, (N, D), 2)
    want = [0, 1, 63, 64, 65, 255, 256, 257, 775, 7001, 3000, 0]
    lists = []
    for n in want:
        ids = np.sort(rng.choice(N, n, replace=False)).astype(np.int64)
        # ids no shard owns: negative, and N or above (ascending all the same)
        lists.append(np.concatenate([[-5, -1], ids, [N, N + 1, N + 4000]]))
    cand, off = _pack(lists, gpu)
    qd = torch.from_numpy(q).to(gpu)

    def call(rows, first):
        return retrieval.rerank_topk_fp8(qd, torch.from_numpy(rows).to(gpu), cand, off, k, first,
                                         SCALE, method=method, ascending=True)

    parts = []
    for r in range(3):
        a, b = retrieval.shard_bounds(N, 3, r)
        parts.append(call(d[a:b], a))
    ms, mi = retrieval.topk_merge(torch.stack([p[0] for p in parts]),
                                  torch.stack([p[1] for p in parts]), k)
    us, ui, un = call(d, 0)
    np.testing.assert_array_equal(mi.cpu().numpy(), ui.cpu().numpy())
    np.testing.assert_array_equal(ms.cpu().numpy().view(np.uint32),
                                  us.cpu().numpy().view(np.uint32))
    ri, rs, rn = _ref8(q, d, lists, k)
    np.testing.assert_array_equal(ui.cpu().numpy(), ri)
    np.testing.assert_array_equal(us.cpu().numpy(), rs)
    np.testing.assert_array_equal(un.cpu().numpy(), rn)


@pytest.fixture(scope="module")
def gaussian():
    """fp32 unit vectors, their e4m3 codes at scale 16, and the fp64 scores of the decoded
    codes over 256 (computed once, shared, left unchanged)."""
    torch.manual_seed(2025)
    q = torch.nn.functional.normalize(torch.randn(16, 768)).numpy()
    d = torch.nn.functional.normalize(torch.randn(20000, 768)).numpy()
    qc, dc = O.quantize_e4m3(q, 16.0), O.quantize_e4m3(d, 16.0)
    full = (O.dequantize_e4m3(qc).astype(np.float64) @
            O.dequantize_e4m3(dc).astype(np.float64).T) / 256
    return q, d, qc, dc, full


@pytest.mark.parametrize("method", METHODS)
def test_one_summation_order(gpu, gaussian, method):
    """A doc's score for a query is bitwise the same in a 5-element list and at position
    12,345 of a 20,000-element list; streamed, also at row 0 and row 300 of 301 queries."""
    _, _, qc, dc, full = gaussian
    # the query's best doc moves to row 12,345, so it sits at position 12,345 of the
    # ascending list of all 20,000 ids
    best = int(np.argmax(full[0]))
    dc2, sc = dc.copy(), full[0].copy()
    dc2[[best, 12345]] = dc2[[12345, best]]
    sc[[best, 12345]] = sc[[12345, best]]
    top = np.sort(np.argsort(-sc)[:5])
    long_list = np.arange(20000)
    assert 12345 in top and long_list[12345] == 12345
    qq = np.stack([qc[0], qc[0]])
    i, s, n = _run8(qq, dc2, [top, long_list], 5, gpu, method=method)
    assert n.tolist() == [5, 5]
    assert i[0, 0] == 12345
    np.testing.assert_array_equal(i[0], i[1])
    np.testing.assert_array_equal(s[0].view(np.uint32), s[1].view(np.uint32))
    assert set(i[0]) == set(top.tolist())
    if method == "stream":
        many = np.concatenate([qc[:1], np.tile(qc[1:2], (299, 1)), qc[:1]])
        assert many.shape[0] == 301
        lists = [top] + [np.zeros(0, np.int64)] * 299 + [long_list]
        i3, s3, _ = _run8(many, dc2, lists, 5, gpu, method="stream")
        np.testing.assert_array_equal(i3[0], i[0])
        np.testing.assert_array_equal(i3[300], i[0])
        np.testing.assert_array_equal(s3[0].view(np.uint32), s[0].view(np.uint32))
        np.testing.assert_array_equal(s3[300].view(np.uint32), s[0].view(np.uint32))


def test_gather_score_at_position_12345_of_an_unsorted_list(gpu, gaussian):
    """The gathered kernel takes lists in any order: the best doc at position 12,345 of a
    shuffled 20,000-element list scores bitwise as in a 5-element list."""
    _, _, qc, dc, full = gaussian
    top = np.argsort(-full[0])[:5]
    rng = np.random.default_rng(7)
    rest = rng.permutation(np.setdiff1d(np.arange(20000), top))
    long_list = np.concatenate([rest[:12345], top[:1], rest[12345:15000], top[1:], rest[15000:]])
    assert long_list[12345] == top[0] and long_list.size == 20000
    qq = np.stack([qc[0], qc[0]])
    i, s, n = _run8(qq, dc, [top[::-1].copy(), long_list], 5, gpu, method="gather",
                    ascending=False)
    assert n.tolist() == [5, 5]
    np.testing.assert_array_equal(i[0], i[1])
    np.testing.assert_array_equal(s[0].view(np.uint32), s[1].view(np.uint32))
    assert top[0] in i[0]


def _launches(lib, name):
    tot, cnt, work = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0)
    lib.irc_prof_query(name, ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(work))
    return cnt.value


@pytest.mark.parametrize("method", ["gather", "stream", "auto"])
def test_index_gaussian_margin_aware(gpu, gaussian, method):
    from irc_amd import _lib, retrieval

    lib = _lib.load()
    q, d, qc, dc, full = gaussian
    index = retrieval.ShardedDenseIndex(torch.from_numpy(d).to(gpu), dtype="fp8")
    np.testing.assert_array_equal(index.docs.cpu().numpy(), dc)
    rng = np.random.default_rng(2025)
    lens = [0, 1, 99, 100, 101, 3000, 3000, 5000, 777, 2048, 2049, 4096, 10000, 20000, 256, 513]
    lists = [np.sort(rng.choice(20000, n, replace=False)) for n in lens]
    k = 100
    cand, off = _pack(lists, gpu)
    lib.irc_prof_reset()
    lib.irc_prof_enable(1)
    try:
        s, i, n = index.search_candidates(torch.from_numpy(q).to(gpu), cand, off, k,
                                          method=method, ascending=True)
        torch.cuda.synchronize()
    finally:
        lib.irc_prof_enable(0)
    ran = (_launches(lib, b"rerank_fp8_stream_score"), _launches(lib, b"rerank_fp8_score"))
    want = method if method != "auto" else retrieval.rerank_method(16, 20000, 768, sum(lens),
                                                                   dtype="fp8")
    assert ran == ((1, 0) if want == "stream" else (0, 1))
    s, i, n = s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()
    ri, rs, rn = _ref8(qc, dc, lists, k)
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
    print(f"{method}: symmetric differences over the 16 queries: {ndiff}")


@pytest.mark.parametrize("method", METHODS)
def test_agrees_with_the_fp8_scan(gpu, method):
    """Every list all N ids ascending: search_candidates is index.search, bitwise."""
    from irc_amd import retrieval

    Q, N, D, k = 20, 4099, 256, 50
    rng = np.random.default_rng(11)
    # grid VALUES m / 256, |m| <= 15: the index quantises them at scale 16 to the codes of m / 16
    q = rng.integers(-15, 16, (Q, D)).astype(np.float32) / 256
    d = rng.integers(-15, 16, (N, D)).astype(np.float32) / 256
    index = retrieval.ShardedDenseIndex(torch.from_numpy(d).to(gpu), doc_offset=7, dtype="fp8")
    np.testing.assert_array_equal(index.docs.cpu().numpy(), O.quantize_e4m3(d * 16))
    qd = torch.from_numpy(q).to(gpu)
    cand, off = _pack([7 + np.arange(N)] * Q, gpu)
    s, i, n = index.search_candidates(qd, cand, off, k, method=method, ascending=True)
    ss, si = index.search(qd, k)
    assert (n.cpu().numpy() == k).all()
    assert torch.equal(i, si)
    assert torch.equal(s.view(torch.int32), ss.view(torch.int32))


def test_hybrid_search_fp8_end_to_end(gpu, tmp_path):
    from irc_amd.retrieval import ShardedDenseIndex, quantize_fp8
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
    with torch.no_grad():
        emb = encode_corpus(model, texts, gpu)
    index = ShardedDenseIndex(emb, dtype="fp8")
    assert index.docs.dtype == torch.uint8
    d64 = O.dequantize_e4m3(index.docs.cpu().numpy()).astype(np.float64)
    row_off_d = torch.tensor(row_off, dtype=torch.int64, device=gpu)
    k, seen = 5, 0
    for batch in loader:
        texts_c = [x["claim"] for x in batch]
        s, i, n = hybrid_search(model, index, sparse_index, row_off_d, texts_c, k, gpu)
        s, i, n = s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()
        with torch.no_grad():
            q8 = quantize_fp8(model.ctx2vec(texts_c, gpu), index.fp8_scale)
        q64 = O.dequantize_e4m3(q8.cpu().numpy()).astype(np.float64)
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
            sc = d64[rows] @ q64[r] / 256
            ri, rs = O.topk_rows(sc.astype(np.float32)[None, :], k)
            ref_ids = rows[ri[0, :m]]
            full = dict(zip(rows.tolist(), sc))
            np.testing.assert_allclose(s[r, :m], [full[j] for j in i[r, :m]], atol=TOL)
            for doc in set(i[r, :m]) ^ set(ref_ids):
                assert abs(full[doc] - rs[0, m - 1]) <= 2 * TOL
            seen += 1 if m else 0
    assert seen > 0


def test_main_index_dtype_fp8_runs(gpu, tmp_path, capsys):
    import main as entry

    claims, cfg, cfg_path, ckpt = _hybrid_setup(tmp_path, gpu)
    entry.main(["--data", "fever", "--config", cfg_path, "--ckpt", ckpt, "--gpu", "0",
                "--retrieval", "hybrid", "--index-dtype", "fp8"])
    out = capsys.readouterr().out
    assert "evidence recall@100" in out
    n_claims = sum(1 for c in claims if c["label"] != "NOT ENOUGH INFO")
    assert out.count("batch of 1 claims") == n_claims


@pytest.mark.parametrize("method", METHODS)
def test_save_load_roundtrip(gpu, tmp_path, method):
    from irc_amd import retrieval

    torch.manual_seed(3)
    d = torch.nn.functional.normalize(torch.randn(5000, 256)).to(gpu)
    q = torch.nn.functional.normalize(torch.randn(20, 256)).to(gpu)
    idx = retrieval.ShardedDenseIndex(d, doc_offset=11, dtype="fp8")
    idx.save(str(tmp_path), rank=0)
    back, _ = retrieval.ShardedDenseIndex.load(str(tmp_path), 0, gpu)
    assert back.dtype == "fp8" and back.docs.dtype == torch.uint8
    rng = np.random.default_rng(5)
    lists = [11 + np.sort(rng.choice(5000, n, replace=False))
             for n in [0, 1, 49, 50, 51, 300, 5000] * 3][:20]
    cand, off = _pack(lists, gpu)
    a = idx.search_candidates(q, cand, off, 50, method=method, ascending=True)
    b = back.search_candidates(q, cand, off, 50, method=method, ascending=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert int(a[2].sum()) == sum(min(50, len(x)) for x in lists)
