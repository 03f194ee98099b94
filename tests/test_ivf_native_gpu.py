"""The one-call cluster-pruned search on the device: irc_ivf_plan against its oracle
``retrieval.ivf_plan`` (elementwise, on the edges of the bitmap's words, the 32-pair chunks and
the scan's span), and irc_ivf_search -- ``IVFDenseIndex.search``'s route -- bit for bit against
``ivf_topk`` over the torch plan and against a numpy reference (fp64 dot products rounded to
fp32 on integer grids, ranked by (score desc, global id asc)); then what the one call is for:
a workspace that is never cleared, query chunks under a workspace limit, and stream order
(graph capture, no host synchronisation)."""
import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (import paths)
from oracle import irc_oracle as O

pytestmark = pytest.mark.gpu

PLAN_KEYS = ("slot_off", "cand_off", "pair_order", "seg_off", "chunk_off")


# ---------------------------------------------------------------- the plan
def _check_plan(probe, list_off, dev):
    """Both probe dtypes against the torch plan (on CPU tensors), all five arrays."""
    from irc_amd.retrieval import ivf_plan, ivf_plan_native

    probe = np.asarray(probe, np.int64)
    lo = torch.tensor(np.asarray(list_off, np.int64))
    want = ivf_plan(torch.from_numpy(probe.astype(np.int32)), lo)
    for dtype in (torch.int32, torch.int64):
        got = ivf_plan_native(torch.from_numpy(probe).to(dtype).to(dev), lo.to(dev),
                              ws_tag="ivf_plan_test")
        assert set(got) == set(PLAN_KEYS)
        for name in PLAN_KEYS:
            assert got[name].dtype == want[name].dtype and got[name].device.type == "cuda"
            assert torch.equal(got[name].cpu(), want[name]), (name, dtype)
    return want


def _unique_rows(rng, Q, nprobe, nlist, holes=0.0):
    """[Q, nprobe] list ids, unique within a row, a share `holes` of the slots -1."""
    probe = np.argsort(rng.random((Q, nlist)), axis=1)[:, :nprobe]
    probe[rng.random(probe.shape) < holes] = -1
    return probe


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)])


HAND_WRITTEN = [
    # lists of 3, 0, 5, 2 rows; list 3 probed by nobody, list 1 (empty) by query 0
    ([[2, 1], [-1, 0], [0, 2], [-1, -1]], [0, 3, 3, 8, 10]),
    # 33 queries probe list 2 (and list 0 second); one more probes list 0 only
    ([[2, 0]] * 33 + [[0, -1]], [0, 4, 4, 10]),
    # an id that names no list
    ([[5, 0]], [0, 2, 3]),
]


@pytest.mark.parametrize("case", range(len(HAND_WRITTEN)))
def test_plan_on_the_hand_written_probes(gpu, case):
    probe, list_off = HAND_WRITTEN[case]
    want = _check_plan(probe, list_off, gpu)
    if case == 0:  # the oracle itself, as tests/test_ivf_cpu.py pins it
        assert want["slot_off"].tolist() == [0, 5, 5, 5, 8, 11, 16, 16, 16]
        assert want["pair_order"].tolist() == [3, 4, 1, 0, 5, 2, 6, 7]


@pytest.mark.parametrize("nprobe", [1, 3])
@pytest.mark.parametrize("Q", [1, 31, 32, 33, 64, 65])
def test_plan_on_the_bitmap_word_edges(gpu, Q, nprobe):
    rng = np.random.default_rng(100 * Q + nprobe)
    lens = rng.integers(0, 40, 7)
    _check_plan(_unique_rows(rng, Q, nprobe, 7, holes=0.15), _offsets(lens), gpu)
    # every query on one list: the ranks run through the whole row of the bitmap
    probe = np.full((Q, nprobe), -1)
    probe[:, nprobe - 1] = 4
    _check_plan(probe, _offsets(lens), gpu)


def test_plan_on_the_chunk_edges(gpu):
    # lists probed by 0, 1, 31, 32, 33 and 65 queries, the probing queries spread over the batch
    counts = [0, 1, 31, 32, 33, 65]
    rng = np.random.default_rng(5)
    Q = 65
    member = np.zeros((Q, len(counts)), bool)
    for c, n in enumerate(counts):
        member[rng.permutation(Q)[:n], c] = True
    probe = np.full((Q, 5), -1)
    for r in range(Q):
        lists = rng.permutation(np.flatnonzero(member[r]))
        probe[r, :lists.size] = lists
        probe[r] = np.roll(probe[r], r % 5)
    want = _check_plan(probe, _offsets([3, 9, 0, 40, 1, 17]), gpu)
    assert np.diff(want["seg_off"].numpy()).tolist() == counts
    assert np.diff(want["chunk_off"].numpy()).tolist() == [0, 1, 1, 1, 2, 3]


def test_plan_on_the_degenerate_layouts(gpu):
    rng = np.random.default_rng(6)
    # nprobe == nlist: every query probes every list
    _check_plan(_unique_rows(rng, 40, 9, 9), _offsets(rng.integers(0, 20, 9)), gpu)
    # nlist == 1, with and without rows, probed or not
    _check_plan([[0], [-1], [0], [0]], [0, 5], gpu)
    _check_plan([[0]] * 33, [0, 0], gpu)
    # empty lists first, in the middle and last
    _check_plan(_unique_rows(rng, 50, 4, 8, holes=0.1), [0, 0, 0, 6, 6, 6, 11, 30, 30], gpu)
    # -1 and ids >= nlist in one row, in every place of it
    probe = _unique_rows(rng, 70, 4, 6)
    probe[::3, 0] = -1
    probe[1::3, 3] = 6
    probe[2::3, 1] = 1000
    probe[5] = [6, -1, 7, -5]
    _check_plan(probe, _offsets(rng.integers(1, 20, 6)), gpu)
    # no valid id at all: pair_order is the identity
    want = _check_plan(np.where(rng.random((37, 3)) < 0.5, -1, 9), _offsets([4, 5, 6]), gpu)
    assert want["pair_order"].tolist() == list(range(111)) and want["slot_off"][-1] == 0


def _span():
    from irc_amd import _lib

    return int(_lib.load().irc_ivf_plan_span())


@pytest.mark.parametrize("more,nprobe", [(-1, 1), (0, 1), (1, 1), (0, 2), (0, 3), (1, 3)])
def test_plan_on_the_span_edges_of_the_pairs(gpu, more, nprobe):
    """Q x nprobe = S - 1, S, S + 1 with nprobe 1, S with nprobe 2, and the multiples of 3 on
    both sides of S (S - 1 when S is a power of two)."""
    S = _span()
    Q = S // nprobe + more
    assert abs(Q * nprobe - S) <= nprobe
    rng = np.random.default_rng(Q)
    lens = rng.integers(0, 25, 50)
    _check_plan(_unique_rows(rng, Q, nprobe, 50, holes=0.1), _offsets(lens), gpu)


def test_plan_over_several_spans_of_pairs(gpu):
    S = _span()
    rng = np.random.default_rng(8)
    Q = (2 * S + 5) // 3 + 40  # more than two spans of pairs, a partly filled last one
    assert 2 * S < 3 * Q < 3 * S
    _check_plan(_unique_rows(rng, Q, 3, 20, holes=0.3), _offsets(rng.integers(0, 25, 20)), gpu)


@pytest.mark.parametrize("spans,extra", [(1, -2), (1, -1), (1, 0), (3, 9)])
def test_plan_on_the_span_edges_of_the_lists(gpu, spans, extra):
    """nlist + 1 = S - 1, S, S + 1, and several spans of lists (the workgroup sums scanned)."""
    nlist = spans * _span() + extra
    rng = np.random.default_rng(nlist)
    lens = rng.integers(0, 5, nlist)
    probe = _unique_rows(rng, 40, 3, nlist - 1, holes=0.1)  # ids below the last list
    probe[::2, 0] = nlist - 1  # the last list too
    probe[1] = [0, nlist - 1, nlist]  # ... and the first; one id past the lists
    want = _check_plan(probe, _offsets(lens), gpu)
    assert want["seg_off"][-1] + (probe < 0).sum() + 1 == probe.size


# ---------------------------------------------------------------- the search
def _grid(rng, shape, lim=127):
    return rng.integers(-lim, lim + 1, shape).astype(np.float32) / 128


def _rows_of(assign, probe):
    """Per query the original rows of its probed lists, ascending."""
    out = []
    for row in np.asarray(probe):
        lists = [c for c in row if c >= 0]
        out.append(np.flatnonzero(np.isin(assign, lists)) if lists else np.zeros(0, np.int64))
    return out


def _reference(q, d, rows, k, doc_offset=0):
    """(idx [Q, k], scores [Q, k], n [Q]) over each query's rows (ascending original ids)."""
    Q = q.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_s = np.full((Q, k), -np.inf, np.float32)
    out_n = np.zeros(Q, np.int32)
    q64, d64 = q.astype(np.float64), d.astype(np.float64)
    for r, ids in enumerate(rows):
        if ids.size == 0:
            continue
        sc = (d64[ids] @ q64[r]).astype(np.float32)
        ti, ts = O.topk_rows(sc[None, :], k)  # positions in ascending ids: ties -> lower id
        m = min(k, ids.size)
        out_i[r, :m] = doc_offset + ids[ti[0, :m]]
        out_s[r, :m] = ts[0, :m]
        out_n[r] = m
    return out_i, out_s, out_n


Q_CASE, NPROBE, K, DOC_OFFSET = 70, 4, 100, 11
_CASES = {}


def _case(D, dev):
    """A cycle of list lengths 0, 1, 31, 32, 33, T - 1, T, T + 1, 2T + 7 on an integer grid, 70
    queries with -1 slots, the last probing nothing; its index, device tensors and the numpy
    reference, built once per D and left unchanged."""
    if D in _CASES:
        return _CASES[D]
    from irc_amd.retrieval import IVF_TILE_ROWS as T
    from irc_amd.retrieval import IVFDenseIndex

    lens = [0, 1, 31, 32, 33, T - 1, T, T + 1, 2 * T + 7]
    N = sum(lens)
    rng = np.random.default_rng(77 + D)
    assign = rng.permutation(np.repeat(np.arange(len(lens)), lens))
    q, d, cent = _grid(rng, (Q_CASE, D), 3), _grid(rng, (N, D), 3), _grid(rng, (len(lens), D), 3)
    probe = _unique_rows(rng, Q_CASE, NPROBE, len(lens)).astype(np.int32)
    probe[rng.random(probe.shape) < 0.15] = -1
    probe[3] = [8, 7, 6, 5]  # the four longest lists: the query that meets key_bound
    probe[-1] = -1
    index = IVFDenseIndex.from_lists(torch.from_numpy(d).to(dev), torch.from_numpy(cent).to(dev),
                                     torch.from_numpy(assign).to(dev), DOC_OFFSET)
    ref = _reference(q, d, _rows_of(assign, probe), K, DOC_OFFSET)
    assert ref[2][-1] == 0 and ref[2][3] == K
    _CASES[D] = dict(index=index, q=torch.from_numpy(q).to(dev).to(torch.bfloat16),
                     probe=torch.from_numpy(probe).to(dev), ref=ref, q_np=q, cent_np=cent)
    return _CASES[D]


def _torch_plan_route(c, probe=None):
    from irc_amd.retrieval import ivf_topk

    index = c["index"]
    return ivf_topk(c["q"], index.docs, index.row_id, index.list_off,
                    c["probe"] if probe is None else probe, K, index.max_list_rows,
                    ws_tag="ivf_torch_plan")


def _same(a, b):
    return all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b)) and \
        len(a) == len(b) == 3


@pytest.mark.parametrize("D", [64, 768])
def test_search_is_the_torch_plan_route_bit_for_bit(gpu, D):
    c = _case(D, gpu)
    index = c["index"]
    got = index.search(c["q"], K, probe=c["probe"])
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int64 and \
        got[2].dtype == torch.int32
    assert _same(got, _torch_plan_route(c))
    ri, rs, rn = c["ref"]
    np.testing.assert_array_equal(got[2].cpu().numpy(), rn)
    np.testing.assert_array_equal(got[1].cpu().numpy(), ri)
    np.testing.assert_array_equal(got[0].cpu().numpy(), rs)
    assert (got[1][-1] == -1).all() and torch.isneginf(got[0][-1]).all()


@pytest.mark.parametrize("D", [64, 768])
def test_search_probing_in_the_call_is_search_over_the_probe(gpu, D):
    from irc_amd import retrieval

    c = _case(D, gpu)
    index = c["index"]
    for nprobe in (1, 3, 9):
        pr = index.probe(c["q"], nprobe)
        np.testing.assert_array_equal(pr.cpu().numpy(),
                                      O.scan_topk(c["q_np"], c["cent_np"], nprobe)[0])
        got = index.search(c["q"], K, nprobe=nprobe)
        assert _same(got, index.search(c["q"], K, probe=pr))
        assert _same(got, _torch_plan_route(c, pr))
        # the probe the call used, as the library reports it
        used = torch.full_like(pr, -7)
        out = retrieval.ivf_search(c["q"], index.docs, index.row_id, index.list_off, K,
                                   Q_CASE * index.key_bound(nprobe), index.max_list_rows,
                                   centroids=index.centroids, nprobe=nprobe, out_probe=used)
        assert torch.equal(used, pr) and _same(out, got)


@pytest.mark.parametrize("D", [64, 768])
def test_search_on_a_workspace_of_the_reported_size_filled_with_ones(gpu, D):
    from irc_amd import _lib, retrieval

    c = _case(D, gpu)
    index = c["index"]
    nlist = index.centroids.shape[0]
    key_rows = Q_CASE * index.key_bound(NPROBE)
    nbytes = int(_lib.fn("irc_ivf_search_workspace")(Q_CASE, NPROBE, nlist, key_rows, K))
    want = _torch_plan_route(c)
    total = int(retrieval.ivf_plan(c["probe"], index.list_off)["slot_off"][-1].item())
    assert total < key_rows  # the bound has slack, and the slack is never read
    for kw in (dict(probe=c["probe"]), dict(nprobe=NPROBE, centroids=index.centroids)):
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)
        got = retrieval.ivf_search(c["q"], index.docs, index.row_id, index.list_off, K, key_rows,
                                   index.max_list_rows, ws=ws, **kw)
        if "probe" in kw:
            assert _same(got, want)
        else:
            assert _same(got, index.search(c["q"], K, nprobe=NPROBE))
    # one byte less is refused before anything runs
    with pytest.raises(_lib.IRCError, match="ivf_search: workspace"):
        retrieval.ivf_search(c["q"], index.docs, index.row_id, index.list_off, K, key_rows,
                             index.max_list_rows, probe=c["probe"], ws=ws[:nbytes - 1])


def test_search_in_query_chunks_under_a_workspace_limit(gpu, monkeypatch):
    from irc_amd import _lib, retrieval

    c = _case(64, gpu)
    index = c["index"]
    nlist = index.centroids.shape[0]
    whole = index.search(c["q"], K, probe=c["probe"])
    whole_own = index.search(c["q"], K, nprobe=NPROBE)
    sizes = []
    inner = retrieval.ivf_search

    def counted(queries, *a, **kw):
        sizes.append(queries.shape[0])
        return inner(queries, *a, **kw)

    monkeypatch.setattr(retrieval, "ivf_search", counted)
    # the limit of 32 queries' workspace: 70 run as 32 + 32 + 6
    limit = int(_lib.fn("irc_ivf_search_workspace")(32, NPROBE, nlist,
                                                    32 * index.key_bound(NPROBE), K))
    monkeypatch.setattr(index, "max_workspace_bytes", limit, raising=False)
    assert _same(index.search(c["q"], K, probe=c["probe"], ws_tag="ivf_chunks"), whole)
    assert sizes == [32, 32, 6]
    assert _same(index.search(c["q"], K, nprobe=NPROBE, ws_tag="ivf_chunks"), whole_own)
    assert sizes == [32, 32, 6] * 2
    monkeypatch.setattr(index, "max_workspace_bytes", 1 << 30, raising=False)
    assert _same(index.search(c["q"], K, probe=c["probe"]), whole) and sizes[6:] == [70]


# ---------------------------------------------------------------- stream order
def test_search_is_captured_in_a_graph_and_replayed(gpu):
    from irc_amd._torch import take_workspace

    c = _case(64, gpu)
    index = c["index"]
    rng = np.random.default_rng(99)
    draws = [torch.from_numpy(_grid(rng, (Q_CASE, 64), 3)).to(gpu).to(torch.bfloat16)
             for _ in range(2)]
    static_q = c["q"].clone()
    tag = "ivf_graph_test"
    st = torch.cuda.Stream(gpu)
    st.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(st):
        index.search(static_q, K, nprobe=3, ws_tag=tag)  # warm-up: sizes the workspace
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):  # one stream, no branches
        out = index.search(static_q, K, nprobe=3, ws_tag=tag)
    ws = take_workspace(gpu, tag)  # the graph points into it: nothing else may grow it
    assert ws is not None
    for q in draws:
        with torch.cuda.stream(st):
            static_q.copy_(q)
            g.replay()
        st.synchronize()
        eager = index.search(q, K, nprobe=3)
        assert _same(out, eager)
        assert not _same(out, index.search(c["q"], K, nprobe=3))  # the draw's own result


def test_search_makes_no_host_synchronisation(gpu):
    from irc_amd.retrieval import ivf_topk

    c = _case(64, gpu)
    index = c["index"]
    want = index.search(c["q"], K, probe=c["probe"])  # workspaces sized, nothing left to grow
    want_own = index.search(c["q"], K, nprobe=3)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        # the mode sees the torch-plan route's .item() on this build ...
        with pytest.raises(RuntimeError, match="synchroniz"):
            ivf_topk(c["q"], index.docs, index.row_id, index.list_off, c["probe"], K,
                     index.max_list_rows, ws_tag="ivf_torch_plan")
        # ... and nothing in the native route, probing included
        got = index.search(c["q"], K, probe=c["probe"])
        got_own = index.search(c["q"], K, nprobe=3)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert _same(got, want) and _same(got_own, want_own)
