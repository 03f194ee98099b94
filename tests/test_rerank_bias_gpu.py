"""The fused score of hybrid retrieval on the GPU (irc_rerank_biased_topk, ``bias=`` of
``rerank_topk`` / ``rerank_topk_fp8`` / ``search_candidates``, ``hybrid_search(fusion=)``).

Reference rule, the same for each method x dtype, with no tolerance: (1) the UNBIASED call
with k = the longest list gives the fp32 bits of every eligible candidate's score; (2) numpy
adds ``np.float32(bias)`` in one fp32 addition; (3) rank by (score desc, id asc); (4) cut to
k.  The biased call must equal that bitwise in scores, ids and n -- on Gaussian data too,
since a (query, row) score has one summation order per method.  Grouped: the same sums,
then the maximum of every (query, group) with the lower id on ties, before the ranking."""
import functools

import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (import paths)
from oracle import irc_oracle as O

pytestmark = pytest.mark.gpu

SCALE = 1.0 / 256  # e4m3 codes hold 16 x the value
OFFSET = 11  # first global id of the shard: flat index != eligible index != row
# (method, dtype, D): gather at D = 64 and 768 on both operand types, stream at 64 and 768
# (bf16) and at 128 and 768 (e4m3: D % 128 == 0)
KERNELS = [("gather", "bf16", 64), ("gather", "bf16", 768), ("gather", "e4m3", 64),
           ("gather", "e4m3", 768), ("stream", "bf16", 64), ("stream", "bf16", 768),
           ("stream", "e4m3", 128), ("stream", "e4m3", 768)]
NS = (255, 256, 257, 513)  # around irc_rerank_stream_tile() = 256, and three tiles
QS = (1, 65, 257)  # one query; two 64-query epilogue passes; two 256-query tiles


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same(got, want, msg=""):
    """(scores, idx, n[, groups]) equal bitwise."""
    assert len(got) == len(want)
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{msg}: ids")
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=f"{msg}: score bits")
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{msg}: n")
    for x, y in zip(got[3:], want[3:]):
        np.testing.assert_array_equal(x, y, err_msg=f"{msg}: groups")


@functools.lru_cache(maxsize=None)
def _operands(Q, N, D, dtype, grid=False):
    """Host operands, computed once per shape and left unchanged: Gaussian unit vectors (bf16
    values / e4m3 codes at scale 16), or with ``grid`` small integers whose sums are exact."""
    rng = np.random.default_rng(Q * 100003 + N * 101 + D + (7 if grid else 0))
    if grid:
        q = rng.integers(-3, 4, (Q, D)).astype(np.float32) / 16
        d = rng.integers(-3, 4, (N, D)).astype(np.float32) / 16
    else:
        q = rng.standard_normal((Q, D)).astype(np.float32)
        d = rng.standard_normal((N, D)).astype(np.float32)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
    if dtype == "e4m3":
        return O.quantize_e4m3(q, 16.0), O.quantize_e4m3(d, 16.0)
    return q, d


def _dev(x, dev, dtype):
    t = torch.from_numpy(x).to(dev)
    return t if dtype == "e4m3" else t.bfloat16()


def _lists(rng, Q, N):
    """Ascending lists in global ids.  By query, in turn: every row of the shard between ids
    of other shards (a prefix below OFFSET, a suffix past the end); empty; one candidate;
    RERANK_CHUNK - 1, + 1 and exactly RERANK_CHUNK random rows (clamped to N); every second
    row; foreign ids only.  Flattened, the lists straddle the 256-candidate chunk boundaries
    wherever those fall."""
    from irc_amd.retrieval import RERANK_CHUNK as C

    rows = OFFSET + np.arange(N, dtype=np.int64)
    pre = np.arange(OFFSET - 4, OFFSET, dtype=np.int64)
    post = np.array([OFFSET + N, OFFSET + N + 1, OFFSET + N + 4000], np.int64)
    out = []
    for r in range(Q):
        kind = r % 8
        if kind == 0:
            out.append(np.concatenate([pre, rows, post]))
        elif kind == 1:
            out.append(np.zeros(0, np.int64))
        elif kind == 2:
            out.append(rows[[int(rng.integers(N))]])
        elif kind in (3, 4, 5):
            n = min(N, (C - 1, C + 1, C)[kind - 3])
            out.append(np.concatenate([pre[2:], np.sort(rng.choice(rows, n, replace=False))]))
        elif kind == 6:
            out.append(np.concatenate([rows[::2], post[:1]]))
        else:
            out.append(np.concatenate([pre, post]))
    return out


def _pack(lists, dev, dtype=torch.int32):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate(lists) if off[-1] else np.zeros(0, np.int64)
    return torch.from_numpy(flat).to(dtype).to(dev), torch.from_numpy(off).to(dev)


def _call(method, dtype, q, d, cand, off, k, ascending=True, doc_offset=OFFSET, **kw):
    from irc_amd import retrieval

    if dtype == "e4m3":
        out = retrieval.rerank_topk_fp8(q, d, cand, off, k, doc_offset, SCALE, method=method,
                                        ascending=ascending, **kw)
    else:
        out = retrieval.rerank_topk(q, d, cand, off, k, doc_offset, method=method,
                                    ascending=ascending, **kw)
    return tuple(x.cpu().numpy() for x in out)


def _rank(ids, sc, k):
    """(scores [k], ids [k], n) of one query by (score desc, id asc), padded."""
    sc = O.canon_scores(sc)
    order = np.lexsort((ids, -sc))[:k]
    s = np.full(k, -np.inf, np.float32)
    i = np.full(k, -1, np.int64)
    s[:order.size], i[:order.size] = sc[order], ids[order]
    return s, i, order.size


def _rule(unbiased, lists, bias, k, group_off=None):
    """The reference rule.  ``unbiased``: (scores, idx, n) of the unbiased call with k = the
    longest list; ``bias``: per list, parallel to it.  With ``group_off`` the sums collapse
    to the maximum of every group (lower id on ties) before the ranking, and the groups are
    a fourth result."""
    us, ui, un = unbiased
    Q = len(lists)
    S = np.full((Q, k), -np.inf, np.float32)
    I = np.full((Q, k), -1, np.int64)
    n = np.zeros(Q, np.int32)
    G = np.full((Q, k), -1, np.int64)
    for r in range(Q):
        ids, sc = ui[r, :un[r]], us[r, :un[r]]
        where = {int(c): j for j, c in enumerate(lists[r])}
        b = np.asarray([bias[r][where[int(c)]] for c in ids], np.float32)
        fused = (sc.astype(np.float32) + b).astype(np.float32)  # one fp32 addition
        if group_off is not None:
            grp = np.searchsorted(group_off, ids, side="right") - 1
            ok = (ids >= group_off[0]) & (ids < group_off[-1])
            ids, fused, grp = ids[ok], O.canon_scores(fused[ok]), grp[ok]
            best = {}
            for j in np.lexsort((ids, -fused)):  # the first of a group is its best row
                best.setdefault(int(grp[j]), j)
            keep = np.asarray(sorted(best.values()), np.int64)
            ids, fused = ids[keep], fused[keep]
        S[r], I[r], n[r] = _rank(ids, fused, k)
        if group_off is not None:
            G[r, :n[r]] = np.searchsorted(group_off, I[r, :n[r]], side="right") - 1
    return (S, I, n) if group_off is None else (S, I, n, G)


def _bias_lists(rng, lists, scale=0.25):
    return [(rng.standard_normal(len(x)) * scale).astype(np.float32) for x in lists]


def _flat(bias, dev):
    flat = np.concatenate(bias) if sum(len(b) for b in bias) else np.zeros(0, np.float32)
    return torch.from_numpy(flat.astype(np.float32)).to(dev)


def _longest(lists):
    return max(1, max(len(x) for x in lists))


# ---------------------------------------------------------------- every kernel, every edge
@pytest.mark.parametrize("Q", QS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("method,dtype,D", KERNELS)
def test_biased_call_is_the_rule_bitwise(gpu, method, dtype, D, N, Q):
    qh, dh = _operands(Q, N, D, dtype)
    q, d = _dev(qh, gpu, dtype), _dev(dh, gpu, dtype)
    rng = np.random.default_rng(Q + N + D)
    lists = _lists(rng, Q, N)
    bias = _bias_lists(rng, lists)
    cand, off = _pack(lists, gpu)
    unbiased = _call(method, dtype, q, d, cand, off, _longest(lists))
    for k in (1, 10, min(1024, N + 5)):
        got = _call(method, dtype, q, d, cand, off, k, bias=_flat(bias, gpu))
        _same(got, _rule(unbiased, lists, bias, k), f"k={k}")
    eligible = [int(((x >= OFFSET) & (x < OFFSET + N)).sum()) for x in lists]
    assert got[2].tolist() == [min(min(1024, N + 5), e) for e in eligible]
    # a bias of zeros is the unbiased call, bit for bit
    zeros = torch.zeros(cand.numel(), device=gpu)
    _same(_call(method, dtype, q, d, cand, off, 10, bias=zeros),
          _call(method, dtype, q, d, cand, off, 10), "zero bias")


@pytest.mark.parametrize("method,dtype,D", KERNELS)
def test_unsorted_int64_lists_carry_their_bias(gpu, method, dtype, D):
    """Shuffled lists with ids of other shards in the MIDDLE and int64 ids outside int32:
    under "stream" the lists are sorted on the device and the bias goes with its candidate;
    under "gather" they are scored where they stand."""
    Q, N = 9, 513
    qh, dh = _operands(Q, N, D, dtype)
    q, d = _dev(qh, gpu, dtype), _dev(dh, gpu, dtype)
    rng = np.random.default_rng(D + 1)
    far = np.array([2 ** 40, -(2 ** 35), 2 ** 31, -1, 2 ** 31 - 1], np.int64)
    lists = []
    for x in _lists(rng, Q, N):
        x = np.concatenate([x, far])
        lists.append(x[rng.permutation(x.size)])
    bias = _bias_lists(rng, lists)
    cand, off = _pack(lists, gpu, torch.int64)
    unbiased = _call(method, dtype, q, d, cand, off, _longest(lists), ascending=False)
    for k in (3, 300):
        got = _call(method, dtype, q, d, cand, off, k, ascending=False, bias=_flat(bias, gpu))
        _same(got, _rule(unbiased, lists, bias, k), f"k={k}")
    assert (got[1] < OFFSET + N).all()  # nothing wrapped into the shard


@pytest.mark.parametrize("method,dtype,D", KERNELS)
def test_a_bias_that_reverses_the_order_and_one_that_ties_everything(gpu, method, dtype, D):
    """Integer grids, every sum exact: bias = -2 s makes the fused score -s, the unbiased
    order reversed (equal scores still by ascending id); bias = 4 - s makes every fused score
    4.0 and the order the ids'."""
    Q, N, k = 5, 300, 40
    qh, dh = _operands(Q, N, D, dtype, grid=True)
    q, d = _dev(qh, gpu, dtype), _dev(dh, gpu, dtype)
    lists = [OFFSET + np.arange(N, dtype=np.int64)[r::r + 1] for r in range(Q)]
    cand, off = _pack(lists, gpu)
    us, ui, un = _call(method, dtype, q, d, cand, off, _longest(lists))
    score_of = [dict(zip(ui[r, :un[r]].tolist(), us[r, :un[r]].tolist())) for r in range(Q)]
    s_lists = [np.asarray([score_of[r][int(c)] for c in lists[r]], np.float32)
               for r in range(Q)]
    rev = [(-2 * s).astype(np.float32) for s in s_lists]
    got = _call(method, dtype, q, d, cand, off, k, bias=_flat(rev, gpu))
    _same(got, _rule((us, ui, un), lists, rev, k), "reversed")
    for r in range(Q):
        m = got[2][r]
        worst = np.lexsort((lists[r], s_lists[r]))[:m]  # ascending score, ascending id
        assert got[1][r, :m].tolist() == lists[r][worst].tolist()
        assert _bits(got[0][r, :m]).tolist() == _bits(O.canon_scores(-s_lists[r][worst])).tolist()
    flat = [(4 - s).astype(np.float32) for s in s_lists]
    got = _call(method, dtype, q, d, cand, off, k, bias=_flat(flat, gpu))
    _same(got, _rule((us, ui, un), lists, flat, k), "all equal")
    for r in range(Q):
        m = got[2][r]
        assert got[1][r, :m].tolist() == lists[r][:m].tolist()  # equal scores: id order
        assert (got[0][r, :m] == 4.0).all()


@pytest.mark.parametrize("method,dtype,D", KERNELS)
def test_without_a_bias_the_call_is_the_native_unbiased_entry(gpu, method, dtype, D):
    """``bias=None`` takes the entries that existed before, with their bits: the wrapper's
    result against a direct call of the unbiased native entry on the same buffers."""
    from irc_amd import _lib
    from irc_amd._torch import ptr, stream_ptr

    Q, N, k = 65, 513, 10
    qh, dh = _operands(Q, N, D, dtype)
    q, d = _dev(qh, gpu, dtype).contiguous(), _dev(dh, gpu, dtype).contiguous()
    lists = _lists(np.random.default_rng(3), Q, N)
    cand, off = _pack(lists, gpu)
    got = _call(method, dtype, q, d, cand, off, k)
    entry = {("gather", "bf16"): "irc_rerank_topk", ("stream", "bf16"): "irc_rerank_topk_stream",
             ("gather", "e4m3"): "irc_rerank_topk_fp8",
             ("stream", "e4m3"): "irc_rerank_topk_stream_fp8"}[method, dtype]
    ws = torch.empty(int(_lib.fn("irc_rerank_topk_workspace")(Q, cand.numel(), k)),
                     dtype=torch.uint8, device=gpu)
    s = torch.empty((Q, k), dtype=torch.float32, device=gpu)
    i = torch.empty((Q, k), dtype=torch.int64, device=gpu)
    n = torch.empty((Q,), dtype=torch.int32, device=gpu)
    _lib.call(entry, ptr(q), ptr(d), Q, N, D, ptr(cand), ptr(off), cand.numel(), k, OFFSET,
              *((SCALE,) if dtype == "e4m3" else ()), ptr(ws), ws.numel(), ptr(s), ptr(i), ptr(n),
              stream_ptr(gpu))
    _same(got, (s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()), "bias=None")
    assert got[2].max() == k


def test_non_finite_sums_rank_as_the_keys_order_them(gpu):
    """Documented, not checked for: +inf first, then the finite sums, then -inf, NaN last of
    the eligible candidates; a candidate of another shard with a NaN bias stays out."""
    qh, dh = _operands(1, 255, 64, "bf16", grid=True)
    q, d = _dev(qh, gpu, "bf16"), _dev(dh, gpu, "bf16")
    ids = np.array([3, OFFSET + 1, OFFSET + 2, OFFSET + 3, OFFSET + 4, OFFSET + 5], np.int64)
    bias = np.array([np.nan, np.nan, -np.inf, 0.0, np.inf, 1.0], np.float32)
    cand, off = _pack([ids], gpu)
    for method in ("gather", "stream"):
        s, i, n = _call(method, "bf16", q, d, cand, off, 6, bias=torch.from_numpy(bias).to(gpu))
        assert n.tolist() == [5]
        assert i[0, 0] == OFFSET + 4 and np.isposinf(s[0, 0])
        assert set(i[0, 1:3].tolist()) == {OFFSET + 3, OFFSET + 5}
        assert i[0, 3] == OFFSET + 2 and np.isneginf(s[0, 3])
        assert i[0, 4] == OFFSET + 1 and np.isnan(s[0, 4])
        assert i[0, 5] == -1 and np.isneginf(s[0, 5])


# ---------------------------------------------------------------- grouped
GROUP_FORMS = [("gather", "bf16", 64), ("stream", "bf16", 768), ("gather", "e4m3", 768),
               ("stream", "e4m3", 128)]


@pytest.mark.parametrize("method,dtype,D", GROUP_FORMS)
def test_grouped_collapse_comes_after_the_bias(gpu, method, dtype, D):
    """Groups of 1, 2, 63, 64 and 65 rows, an empty one, and one of 300 rows that spans a
    chunk; rows before the first and after the last group are in none.  The bias changes
    which row stands for a group, and which groups win."""
    Q, N, k = 6, 700, 5
    qh, dh = _operands(Q, N, D, dtype)
    q, d = _dev(qh, gpu, dtype), _dev(dh, gpu, dtype)
    sizes = [1, 2, 63, 0, 64, 65, 300, 1, 2, 63, 64, 65]
    go = OFFSET + 3 + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert go[-1] < OFFSET + N
    rng = np.random.default_rng(D)
    rows = OFFSET + np.arange(N, dtype=np.int64)
    lists = [np.concatenate([[2, 5], rows, [OFFSET + N + 9]]), rows[::2], rows[1::3],
             np.sort(rng.choice(rows, 257, replace=False)), np.zeros(0, np.int64),
             rows[go[6] - OFFSET + 100:go[7] - OFFSET + 1]]  # mostly the 300-row group
    bias = _bias_lists(rng, lists, scale=0.5)
    cand, off = _pack(lists, gpu)
    unbiased = _call(method, dtype, q, d, cand, off, _longest(lists))
    god = torch.from_numpy(go).to(gpu)
    for kk in (1, k, 64):
        got = _call(method, dtype, q, d, cand, off, kk, group_off=god, bias=_flat(bias, gpu))
        _same(got, _rule(unbiased, lists, bias, kk, group_off=go), f"k={kk}")
    # the prior decides: another row represents some group than without it
    plain = _call(method, dtype, q, d, cand, off, 64, group_off=god)
    moved = 0
    for r in range(Q):
        a = dict(zip(plain[3][r, :plain[2][r]].tolist(), plain[1][r].tolist()))
        b = dict(zip(got[3][r, :got[2][r]].tolist(), got[1][r].tolist()))
        assert set(a) == set(b)  # the same groups are present
        moved += sum(a[g] != b[g] for g in a)
    assert moved > 0
    zeros = torch.zeros(cand.numel(), device=gpu)
    _same(_call(method, dtype, q, d, cand, off, 64, group_off=god, bias=zeros), plain,
          "zero bias, grouped")


# ---------------------------------------------------------------- the index
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("method", ["gather", "stream", "auto"])
def test_search_candidates_with_a_bias(gpu, dtype, method):
    """The index's call, per row and per group of four rows, on a bf16 and an fp8 shard (the
    bias is added to the descaled score).  N = 1000: one unbiased call at k = 1024 returns
    every eligible candidate."""
    from irc_amd.retrieval import ShardedDenseIndex

    Q, N, D, k = 7, 1000, 128, 12
    qh, dh = _operands(Q, N, D, "bf16")
    index = ShardedDenseIndex(torch.from_numpy(dh).to(gpu), doc_offset=OFFSET, dtype=dtype)
    q = torch.from_numpy(qh).to(gpu)
    rng = np.random.default_rng(5)
    lists = _lists(rng, Q, N)
    bias = _bias_lists(rng, lists)
    cand, off = _pack(lists, gpu, torch.int64)
    kw = dict(method=method, ascending=True)
    un = tuple(x.cpu().numpy() for x in index.search_candidates(q, cand, off, 1024, **kw))
    got = index.search_candidates(q, cand, off, k, bias=_flat(bias, gpu), **kw)
    assert len(got) == 3
    _same(tuple(x.cpu().numpy() for x in got), _rule(un, lists, bias, k), f"{dtype} {method}")
    go = torch.arange(OFFSET, OFFSET + N + 1, 4, device=gpu)
    out = index.search_candidates(q, cand, off, k, group_off=go, bias=_flat(bias, gpu), **kw)
    assert len(out) == 4
    _same(tuple(x.cpu().numpy() for x in out), _rule(un, lists, bias, k, go.cpu().numpy()),
          f"{dtype} {method} grouped")


# ---------------------------------------------------------------- the pipeline
class _ToyModel:
    """ctx2vec of the bi-encoder: a fixed unit vector per claim text."""

    def __init__(self, dim):
        self.dim = dim

    def ctx2vec(self, texts, device):
        out = []
        for t in texts:
            g = np.random.default_rng(sum(map(ord, t)))
            v = g.standard_normal(self.dim).astype(np.float32)
            out.append(v / np.linalg.norm(v))
        return torch.from_numpy(np.stack(out)).to(device)


@functools.lru_cache(maxsize=None)
def _toy():
    """Ten pages of 0 .. 4 lines over a 40-word vocabulary, their count and TF-IDF matrices,
    four claims (one of words no page has), and a random embedding per line."""
    from irc_amd import sparse

    rnd = np.random.RandomState(11)
    words = [f"w{i}" for i in range(40)]
    pages = [[" ".join(rnd.choice(words, rnd.randint(4, 9))) for _ in range(n)]
             for n in (3, 1, 4, 0, 2, 2, 1, 3, 4, 2)]
    texts = [" ".join(p) if p else "zz" for p in pages]
    counts = sparse.build_count_matrix(texts, 1 << 12, 2)
    tfidf = sparse.tfidf_matrix(counts)
    claims = [" ".join(pages[0][0].split()[:3] + pages[7][1].split()[:3]),
              " ".join(pages[2][1].split()[1:5]), "qq rr ss",
              " ".join(pages[8][0].split()[:2] + pages[9][0].split()[:2] + pages[4][0].split()[:2])]
    row_off = np.concatenate([[0], np.cumsum([len(p) for p in pages])]).astype(np.int64)
    emb = np.random.default_rng(1).standard_normal((int(row_off[-1]), 64)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    return counts, tfidf, sparse.doc_freqs(counts), claims, row_off, emb


@pytest.mark.parametrize("unit", ["line", "page"])
@pytest.mark.parametrize("dtype,method", [("bf16", "gather"), ("bf16", "stream"),
                                          ("fp8", "gather")])
def test_hybrid_search_fuses_the_sparse_score(gpu, dtype, method, unit):
    from irc_amd.retrieval import ShardedDenseIndex
    from irc_amd.sparse import SparseIndex
    from src.evaluation import hybrid_search

    counts, tfidf, freqs, claims, row_off, emb = _toy()
    model = _ToyModel(64)
    index = ShardedDenseIndex(torch.from_numpy(emb).to(gpu), dtype=dtype)
    filt = SparseIndex(counts, ngram=2, device=gpu)
    scorer = SparseIndex(tfidf, ngram=2, doc_freqs_=freqs, device=gpu)
    ro = torch.from_numpy(row_off).to(gpu)
    go = ro if unit == "page" else None
    k, w = 4, 0.75
    args = (model, index, filt, ro, claims, k, gpu)
    base = hybrid_search(*args, method=method, group_off=go)
    same = hybrid_search(*args, method=method, group_off=go, fusion=0.0, tfidf_index=scorer)
    _same(tuple(x.cpu().numpy() for x in same), tuple(x.cpu().numpy() for x in base), "fusion=0")
    got = tuple(x.cpu().numpy() for x in hybrid_search(*args, method=method, group_off=go,
                                                       fusion=w, tfidf_index=scorer))
    # numpy: the filter's pages, their TF-IDF scores in the order the SpMV adds them (rows
    # ascending, product and sum rounded separately), max-normalised per claim, fp32, x w
    cols = filt.documents_filtering(claims, False)
    lists, bias = [], []
    for c, claim in enumerate(claims):
        wids, wts = scorer.text2spvec(claim)
        row = np.zeros(tfidf.shape[1])
        for h, x in zip(wids, wts):
            lo, hi = tfidf.indptr[h], tfidf.indptr[h + 1]
            row[tfidf.indices[lo:hi]] += x * tfidf.data[lo:hi]
        page = row[cols[c]]
        top = page.max() if page.size else 0.0
        norm = page / top if top > 0 else np.zeros_like(page)
        b = norm.astype(np.float32) * np.float32(w)
        lists.append(np.array([j for p in cols[c] for j in range(row_off[p], row_off[p + 1])],
                              np.int64))
        bias.append(np.array([b[j] for j, p in enumerate(cols[c])
                              for _ in range(row_off[p], row_off[p + 1])], np.float32))
    assert sum(len(x) > 0 for x in lists) >= 3 and len(lists[2]) == 0  # claim 2: no candidate
    assert any(len(set(b.tolist())) > 1 for b in bias)  # pages with different priors
    un = tuple(x.cpu().numpy() for x in hybrid_search(model, index, filt, ro, claims,
                                                      _longest(lists), gpu, method=method))
    want = _rule(un, lists, bias, k, group_off=row_off if unit == "page" else None)
    _same(got, want, f"{dtype} {method} {unit}")
    # and the page scores themselves, against the SpMV's own ranking
    cand, off = filt.candidates(claims, False)
    vecs = [scorer.text2spvec(c) for c in claims]
    ps = scorer.candidate_scores([v[0] for v in vecs], [v[1] for v in vecs], cand, off)
    assert ps.dtype == torch.float64 and ps.numel() == cand.numel()
    ps, o = ps.cpu().numpy(), off.cpu().numpy()
    for c, (idx, sc) in enumerate(scorer.topk_rows([v[0] for v in vecs], [v[1] for v in vecs],
                                                   10)):
        mine = dict(zip(cols[c].tolist(), ps[o[c]:o[c + 1]].tolist()))
        assert all(mine[int(j)] == s for j, s in zip(idx, sc))  # the same fp64 bits
        assert sorted(x for x in mine.values() if x != 0) == sorted(sc.tolist())


def test_candidate_scores_in_chunks(gpu, monkeypatch):
    """A bound of one dense row per chunk gives the same scores as one chunk for all."""
    from irc_amd.sparse import SparseIndex

    counts, tfidf, freqs, claims, _, _ = _toy()
    scorer = SparseIndex(tfidf, ngram=2, doc_freqs_=freqs, device=gpu)
    cand, off = SparseIndex(counts, ngram=2, device=gpu).candidates(claims, False)
    vecs = [scorer.text2spvec(c) for c in claims]
    rows, wts = [v[0] for v in vecs], [v[1] for v in vecs]
    whole = scorer.candidate_scores(rows, wts, cand, off)
    monkeypatch.setattr(SparseIndex, "MAX_DENSE_BYTES", tfidf.shape[1] * 8)
    assert torch.equal(scorer.candidate_scores(rows, wts, cand, off), whole)
    monkeypatch.setattr(SparseIndex, "MAX_DENSE_BYTES", tfidf.shape[1] * 8 * 3)
    assert torch.equal(scorer.candidate_scores(rows, wts, cand, off), whole)
    assert (whole > 0).any()


def test_main_fusion_weight_runs(gpu, tmp_path, capsys):
    """main.py --retrieval hybrid --fusion-weight W end to end on the toy FEVER files of
    test_predict_gpu.py: the recall line names the weight; per page on an fp8 index too."""
    import main as entry
    from test_rerank_gpu import _hybrid_setup

    claims, cfg, cfg_path, ckpt = _hybrid_setup(tmp_path, gpu)
    base = ["--data", "fever", "--config", cfg_path, "--ckpt", ckpt, "--gpu", "0",
            "--retrieval", "hybrid"]
    entry.main(base + ["--fusion-weight", "0.5"])
    out = capsys.readouterr().out
    assert "evidence recall@100 (fusion weight 0.5):" in out
    n_claims = sum(1 for c in claims if c["label"] != "NOT ENOUGH INFO")
    assert out.count("batch of 1 claims") == n_claims
    # the toy encoder is 64 wide, where the e4m3 stream kernel does not run: fp8 gathered
    entry.main(base + ["--fusion-weight", "2", "--rerank-unit", "page", "--index-dtype", "fp8",
                       "--rerank-method", "gather"])
    assert "evidence recall@100 (pages) (fusion weight 2):" in capsys.readouterr().out
    entry.main(base + ["--fusion-weight", "0.25", "--rerank-unit", "page", "--rerank-method",
                       "stream"])
    assert "evidence recall@100 (pages) (fusion weight 0.25):" in capsys.readouterr().out
    entry.main(base)
    assert "fusion" not in capsys.readouterr().out
