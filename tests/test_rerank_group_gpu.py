"""Candidate top-k per group (irc_rerank_topk_grouped, rerank_collapse_kernel) against the
numpy reference of test_rerank_group_cpu.py: float64 scores cast to fp32, per group the
maximum with the lower id on ties, then O.topk_rows.  Integer grids with values in +-3 make
every fp32 sum exact and ties plentiful, so idx, scores, n and groups must be equal bitwise
for both scoring methods and for bf16 and e4m3 operands."""
import argparse
import functools

import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (import paths)
from oracle import irc_oracle as O
from test_rerank_fp8_gpu import SCALE, _codes
from test_rerank_fp8_gpu import _grid_case as _grid_case8
from test_rerank_gpu import _grid, _hybrid_setup, _lengths, _pack
from test_rerank_gpu import _grid_case as _grid_case16
from test_rerank_group_cpu import _reference_grouped

pytestmark = pytest.mark.gpu

METHODS = ("gather", "stream")
DTYPES = ("bf16", "e4m3")


def _sizes():
    """0 is an empty group; the rest give runs across wave and chunk boundaries, and one
    run longer than two chunks (700 rows at a chunk of 256)."""
    from irc_amd.retrieval import RERANK_CHUNK as C

    return [0, 1, 2, 63, 64, 65, C - 1, C, C + 1, 2 * C + 188]


def _group_off(N, doc_offset, kind="cycle"):
    """Group offsets in global row ids, the sizes cycling through _sizes().  The first two
    rows of the shard are in no group.  "cycle": groups up to the shard's end, the last
    one reaching 5 ids past it (into the next shard).  "many": 30 blocks of small groups
    after every cycle, over a thousand groups in 20,000 rows.  "few": 50 groups, the rows
    after them in no group."""
    sizes = _sizes()
    if kind == "many":
        sizes = sizes + [0, 1, 2, 3, 5, 8, 13, 21, 34] * 30
    go = [doc_offset + 2]
    end = doc_offset + N
    j = 0
    while go[-1] < end and not (kind == "few" and len(go) == 51):
        go.append(go[-1] + sizes[j % len(sizes)])
        j += 1
    if kind != "few":
        go[-1] = end + 5
    assert all(a <= b for a, b in zip(go, go[1:]))
    return np.asarray(go, np.int64)


def _lists(rng, Q, N, k, doc_offset, go):
    """Per query, in turn: all rows; every second row; a random ascending list of one of
    test_rerank_gpu._lengths; a list that ends inside a group and the next query's list that
    starts inside the same group; ids of other shards before and after rows that avoid the
    last group, whose only candidates are then foreign."""
    lens = _lengths(k, N)
    rows = doc_offset + np.arange(N, dtype=np.int64)
    size = np.diff(go)
    big = np.flatnonzero((size >= 3) & (go[1:] <= doc_offset + N))
    lists = []
    r = 0
    while r < Q:
        kind = r % 6
        if kind == 0:
            lists.append(rows)
        elif kind == 1:
            lists.append(rows[::2])
        elif kind == 2:
            n = lens[(r // 6) % len(lens)]
            lists.append(doc_offset + np.sort(rng.choice(N, n, replace=False)))
        elif kind == 3:
            g = big[(r // 6) % big.size] if big.size else 0
            mid = int(go[g] + size[g] // 2) if big.size else doc_offset + N // 2
            lo = max(doc_offset, mid - 300)
            lists.append(np.arange(lo, mid, dtype=np.int64))
            if r + 1 < Q:  # the next query takes up the group where this one stopped
                lists.append(np.arange(mid, min(doc_offset + N, mid + 300), dtype=np.int64))
                r += 1
        else:
            assert kind == 5  # 4 is the second list of the pair
            own = int(max(go[-2] - doc_offset, 1))  # rows below the last group
            ids = doc_offset + np.sort(rng.choice(min(own, N), min(own, N, 400), replace=False))
            pre = np.arange(max(doc_offset - 3, 0), doc_offset, dtype=np.int64)
            end = doc_offset + N
            lists.append(np.concatenate([pre, ids, [end, end + 1, end + 4000]]))
        r += 1
    assert len(lists) == Q
    return lists


GRID_CASES = [(3, 40, 128, 8, 11, "cycle"), (33, 4099, 64, 10, 0, "cycle"),
              (257, 4099, 128, 100, 5, "cycle"),  # two query tiles for the stream
              (16, 20000, 768, 1024, 3, "many"),  # more than 1024 groups
              (16, 20000, 768, 1024, 3, "few")]  # 50 groups
# D = 64 is gather-only for e4m3
GRID_PARAMS = [(c, dt, m) for c in GRID_CASES for dt in DTYPES for m in METHODS
               if not (dt == "e4m3" and m == "stream" and c[2] % 128)]


def _operands(rng, dtype, Q, N, D):
    if dtype == "e4m3":
        return _codes(rng, (Q, D)), _codes(rng, (N, D))
    return _grid(rng, (Q, D), 3), _grid(rng, (N, D), 3)


def _ref(dtype, q, d, lists, k, go, doc_offset=0):
    if dtype == "e4m3":
        i, s, n, g = _reference_grouped(O.dequantize_e4m3(q), O.dequantize_e4m3(d), lists, k, go,
                                        doc_offset)
        return i, (s * np.float32(SCALE)).astype(np.float32), n, g
    return _reference_grouped(q, d, lists, k, go, doc_offset)


@functools.lru_cache(maxsize=None)
def _case(case, dtype):
    """Operands, lists, group offsets and the reference of one grid case: computed once,
    shared by the methods, left unchanged."""
    Q, N, D, k, doc_offset, kind = case
    rng = np.random.default_rng(Q * 1000 + D + len(kind))
    q, d = _operands(rng, dtype, Q, N, D)
    go = _group_off(N, doc_offset, kind)
    lists = _lists(rng, Q, N, k, doc_offset, go)
    return q, d, lists, go, _ref(dtype, q, d, lists, k, go, doc_offset)


def _call(dtype, q, d, cand, off, k, doc_offset, method, ascending, go):
    from irc_amd import retrieval

    if dtype == "e4m3":
        return retrieval.rerank_topk_fp8(q, d, cand, off, k, doc_offset, SCALE, method=method,
                                         ascending=ascending, group_off=go)
    return retrieval.rerank_topk(q, d, cand, off, k, doc_offset, method=method,
                                 ascending=ascending, group_off=go)


def _run(dtype, q, d, lists, k, dev, doc_offset, go, method, ascending=True, idt=torch.int32):
    cand, off = _pack(lists, dev, idt)
    god = None if go is None else torch.from_numpy(np.asarray(go, np.int64)).to(dev)
    out = _call(dtype, torch.from_numpy(q).to(dev), torch.from_numpy(d).to(dev), cand, off, k,
                doc_offset, method, ascending, god)
    s, i, n = (x.cpu().numpy() for x in out[:3])
    if go is None:
        assert len(out) == 3
        return i, s, n
    assert out[3].dtype == torch.int64 and tuple(out[3].shape) == (q.shape[0], k)
    return i, s, n, out[3].cpu().numpy()


def _equal(got, want):
    for x, y in zip((got[2], got[0], got[1], got[3]), (want[2], want[0], want[1], want[3])):
        np.testing.assert_array_equal(x, y)


def _bitwise(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("case,dtype,method", GRID_PARAMS)
def test_bit_exact_on_integer_grids(gpu, case, dtype, method):
    Q, N, D, k, doc_offset, kind = case
    q, d, lists, go, ref = _case(case, dtype)
    n_groups = np.count_nonzero(np.diff(go))
    assert (n_groups > 1024) if kind == "many" else (n_groups <= 1024)
    got = _run(dtype, q, d, lists, k, gpu, doc_offset, go, method)
    _equal(got, ref)
    # something was collapsed, and in the case of many groups k groups were there to return
    assert (ref[2] < [min(k, len(np.unique(x))) for x in lists]).any()
    if kind == "many":
        assert ref[2].max() == k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_singleton_groups_are_the_ungrouped_call(gpu, dtype, method):
    Q, N, D, k, doc_offset = 257, 4099, 128, 100, 5
    q, d, lists = (_grid_case8 if dtype == "e4m3" else _grid_case16)(Q, N, D, k, doc_offset)
    go = doc_offset + np.arange(N + 1, dtype=np.int64)
    plain = _run(dtype, q, d, lists, k, gpu, doc_offset, None, method)
    got = _run(dtype, q, d, lists, k, gpu, doc_offset, go, method)
    _bitwise(got[:3], plain)
    np.testing.assert_array_equal(got[3], np.where(got[0] < 0, -1, got[0] - doc_offset))


@pytest.fixture(scope="module")
def gaussian():
    """Unit vectors as bf16 values and as e4m3 codes at scale 16, ascending lists of at
    most 1024 rows and group offsets that leave the first two and the last rows out."""
    torch.manual_seed(2025)
    Q, N, D = 16, 4099, 768
    q = torch.nn.functional.normalize(torch.randn(Q, D))
    d = torch.nn.functional.normalize(torch.randn(N, D))
    ops = {"bf16": (q.bfloat16().float().numpy(), d.bfloat16().float().numpy()),
           "e4m3": (O.quantize_e4m3(q.numpy(), 16.0), O.quantize_e4m3(d.numpy(), 16.0))}
    rng = np.random.default_rng(2025)
    lens = [0, 1, 99, 100, 101, 1024, 1024, 777, 513, 256, 255, 257, 1000, 64, 65, 700]
    lists = [7 + np.sort(rng.choice(N, n, replace=False)) for n in lens]
    go = _group_off(N - 40, 7, "many")
    go[-1] = 7 + N - 40  # the last 40 rows in no group
    return ops, lists, go


def _collapse(i, s, k, go):
    """The numpy collapse of a full ranking (i, s) [Q, n]: rows of no group dropped, then
    the first -- best, lower id on ties -- row of every group, the first k of them."""
    Q = i.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_s = np.full((Q, k), -np.inf, np.float32)
    out_n = np.zeros(Q, np.int32)
    out_g = np.full((Q, k), -1, np.int64)
    for r in range(Q):
        keep = (i[r] >= go[0]) & (i[r] < go[-1])
        ids, sc = i[r][keep], s[r][keep]
        grp = np.searchsorted(go, ids, side="right") - 1
        _, first = np.unique(grp, return_index=True)
        first = np.sort(first)[:k]
        m = first.size
        out_i[r, :m], out_s[r, :m], out_g[r, :m], out_n[r] = ids[first], sc[first], grp[first], m
    return out_i, out_s, out_n, out_g


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_gaussian_is_the_collapse_of_the_ungrouped_ranking(gpu, gaussian, dtype, method):
    ops, lists, go = gaussian
    q, d = ops[dtype]
    full = _run(dtype, q, d, lists, 1024, gpu, 7, None, method)  # every list's whole ranking
    assert (full[2] == [len(x) for x in lists]).all()
    for k in (100, 1024):
        got = _run(dtype, q, d, lists, k, gpu, 7, go, method)
        want = _collapse(full[0], full[1], k, go)
        _bitwise(got, want)
        ret = got[0][got[0] >= 0]
        assert ((ret >= go[0]) & (ret < go[-1])).all()  # no row of no group
    assert (want[2] < full[2]).any() and want[2].max() > 100


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", METHODS)
def test_unsorted_and_int64_lists(gpu, dtype, method):
    case = GRID_CASES[2]
    Q, N, D, k, doc_offset, _ = case
    q, d, lists, go, ref = _case(case, dtype)
    rng = np.random.default_rng(9)
    shuffled = [rng.permutation(x) for x in lists]
    got = _run(dtype, q, d, shuffled, k, gpu, doc_offset, go, method, ascending=False,
               idt=torch.int64)
    _equal(got, ref)
    # int64 ids outside int32 and negative ids are foreign, never wrapped into a group
    wide = [np.concatenate([x, x[:3] + 2 ** 32, x[:3] - 2 ** 32, [2 ** 31, -2 ** 31 - 1]])
            for x in shuffled]
    got = _run(dtype, q, d, wide, k, gpu, doc_offset, go, method, ascending=False,
               idt=torch.int64)
    _equal(got, ref)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("method", ["gather", "stream", "auto"])
def test_index_search_candidates_grouped(gpu, dtype, method):
    from irc_amd import retrieval

    Q, N, D, k, doc_offset = 20, 4099, 256, 50, 7
    rng = np.random.default_rng(11)
    # grid VALUES m / 256, |m| <= 15: exact in bf16; an fp8 index quantises them at scale 16
    # to the codes of m / 16
    q = rng.integers(-15, 16, (Q, D)).astype(np.float32) / 256
    d = rng.integers(-15, 16, (N, D)).astype(np.float32) / 256
    index = retrieval.ShardedDenseIndex(torch.from_numpy(d).to(gpu), doc_offset=doc_offset,
                                        dtype=dtype)
    go = _group_off(N, doc_offset, "cycle")
    lists = _lists(rng, Q, N, k, doc_offset, go)
    cand, off = _pack(lists, gpu)
    s, i, n, g = index.search_candidates(torch.from_numpy(q).to(gpu), cand, off, k,
                                         method=method, ascending=True,
                                         group_off=torch.from_numpy(go).to(gpu))
    if dtype == "fp8":
        qv = O.dequantize_e4m3(O.quantize_e4m3(q * 16))
        dv = O.dequantize_e4m3(index.docs.cpu().numpy())
        ri, rs, rn, rg = _reference_grouped(qv, dv, lists, k, go, doc_offset)
        rs = (rs * np.float32(1.0 / 256)).astype(np.float32)
    else:
        ri, rs, rn, rg = _reference_grouped(q, d, lists, k, go, doc_offset)
    _equal((i.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy(), g.cpu().numpy()),
           (ri, rs, rn, rg))


def test_hybrid_search_one_row_per_page(gpu, tmp_path):
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
    assert len(texts) <= 1024  # so k = 1024 returns every list's whole ranking
    with torch.no_grad():
        index = ShardedDenseIndex(encode_corpus(model, texts, gpu))
    row_off_d = torch.tensor(row_off, dtype=torch.int64, device=gpu)
    k, collapsed = 5, 0
    for batch in loader:
        texts_c = [x["claim"] for x in batch]
        out = hybrid_search(model, index, sparse_index, row_off_d, texts_c, k, gpu,
                            group_off=row_off_d)
        assert len(out) == 4
        s, i, n, g = (x.cpu().numpy() for x in out)
        plain = hybrid_search(model, index, sparse_index, row_off_d, texts_c, 1024, gpu)
        assert len(plain) == 3
        fs, fi, fn = (x.cpu().numpy() for x in plain)
        for r in range(len(batch)):
            m = int(n[r])
            ranking = fi[r, :fn[r]].tolist()
            pages = [titles[j] for j in ranking]
            best = {}  # each title's best row in the ungrouped ranking
            for j, t in zip(ranking, pages):
                best.setdefault(t, j)
            assert m == min(k, len(best))
            got_titles = [titles[j] for j in i[r, :m]]
            assert len(set(got_titles)) == m  # at most one row per title
            assert i[r, :m].tolist() == list(best.values())[:m]
            assert [titles[row_off[c]] for c in g[r, :m]] == got_titles
            np.testing.assert_array_equal(s[r, :m].view(np.uint32),
                                          fs[r, [ranking.index(j) for j in i[r, :m]]]
                                          .view(np.uint32))
            assert (i[r, m:] == -1).all() and (g[r, m:] == -1).all()
            collapsed += int(len(best) < len(ranking))
    assert collapsed > 0


def test_main_rerank_unit_page_runs(gpu, tmp_path, capsys):
    import main as entry

    claims, cfg, cfg_path, ckpt = _hybrid_setup(tmp_path, gpu)
    entry.main(["--data", "fever", "--config", cfg_path, "--ckpt", ckpt, "--gpu", "0",
                "--retrieval", "hybrid", "--rerank-unit", "page"])
    out = capsys.readouterr().out
    assert "evidence recall@100 (pages): " in out
    n_claims = sum(1 for c in claims if c["label"] != "NOT ENOUGH INFO")
    assert out.count("batch of 1 claims") == n_claims
