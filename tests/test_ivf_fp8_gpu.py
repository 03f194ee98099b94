"""Cluster-pruned search over e4m3 lists (irc_ivf_topk_fp8, irc_ivf_search_fp8,
``IVFDenseIndex.to_fp8``) against the numpy reference of tests/test_ivf_gpu.py applied the way
tests/test_rerank_fp8_gpu.py::_ref8 applies it: per query the union of the rows of its probed
lists, the fp64 dot product of the DECODED codes rounded to fp32, times np.float32(score_scale),
ranked by (score desc, global id asc).  Given the probes and the codes every check is exact."""
import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (import paths)
from oracle import irc_oracle as O
from test_ivf_gpu import (GRID_CASES, _bf16, _gaussian_case, _grid, _grid_case, _index,
                          _reference, _rows_of, _unit)

pytestmark = pytest.mark.gpu

TOL = 1e-5  # tests/test_scan_fp8_gpu.py: fp32 accumulation order on D = 768 products of e4m3 values
FP8 = 16.0  # retrieval.FP8_SCALE
SCALE = 1.0 / 256  # the descale of two operands quantised at 16: a power of two


def _halve(*arrays):
    """The grids of tests/test_ivf_gpu.py are m / 128, |m| <= 3: halved they are the bf16 rows
    m / 256, which quantise at 16 to the codes m / 16 exactly -- the codes of
    tests/test_rerank_fp8_gpu.py::_codes, whose sums are exact in fp32 in any order."""
    return tuple((a * np.float32(0.5)).astype(np.float32) for a in arrays)


def _q8(x, scale=FP8):
    return O.quantize_e4m3(x, scale)


def _ref8(qc, dc, rows, k, doc_offset=0, scale=SCALE):
    i, s, n = _reference(O.dequantize_e4m3(qc), O.dequantize_e4m3(dc), rows, k, doc_offset)
    return i, (s * np.float32(scale)).astype(np.float32), n


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _np(out):
    """(scores, idx, n) tensors -> (idx, scores, n) arrays, the reference's order."""
    s, i, n = out
    return i.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()


def _same(a, b):
    """Two (scores, idx, n) results, bit for bit."""
    return all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a[1:], b[1:])) and \
        torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def _assert_ref(got, ref):
    i, s, n = _np(got)
    ri, rs, rn = ref
    np.testing.assert_array_equal(n, rn)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s.view(np.uint32), rs.view(np.uint32))


def _topk8(index8, qc, probe, k, dev, scale=SCALE, **kw):
    from irc_amd.retrieval import ivf_topk_fp8

    return ivf_topk_fp8(_dev(qc, dev), index8.docs, index8.row_id, index8.list_off,
                        _dev(np.asarray(probe, np.int32), dev), k, index8.max_list_rows, scale,
                        **kw)


_CASES = {}


def _case(D, npq, dev, doc_offset=0):
    """tests/test_ivf_gpu.py::_grid_case as bf16 rows m / 256 and their codes; built once."""
    key = (D, npq, doc_offset)
    if key not in _CASES:
        q, d, cent, assign, probe = _grid_case(D, npq)
        q, d = _halve(q, d)
        qc, dc = _q8(q), _q8(d)
        assert np.array_equal(O.dequantize_e4m3(qc), q * 16)  # m / 16, no rounding
        assert np.array_equal(O.dequantize_e4m3(dc), d * 16)
        index = _index(d, cent, assign, dev, doc_offset)
        index8 = index.to_fp8(FP8)
        _CASES[key] = dict(q=q, d=d, qc=qc, dc=dc, assign=assign, probe=probe, index=index,
                           index8=index8, qt=_dev(q, dev).to(torch.bfloat16),
                           pt=_dev(probe, dev), rows=_rows_of(assign, probe))
    return _CASES[key]


# ---------------------------------------------------------------- bit-exact on e4m3 grids
def test_to_fp8_shares_the_clustering_and_quantises_the_rows(gpu):
    c = _case(128, 33, gpu, 11)
    index, index8 = c["index"], c["index8"]
    assert index8.dtype == "fp8" and index8.fp8_scale == FP8 and index.dtype == "bf16"
    assert type(index8) is type(index) and index8.doc_offset == 11
    assert index8.docs.dtype == torch.uint8 and index8.docs.shape == index.docs.shape
    for name in ("row_id", "list_off", "centroids", "_key_prefix"):
        assert getattr(index8, name) is getattr(index, name)  # shared, not copied
    assert index8.max_list_rows == index.max_list_rows
    rid = index.row_id.cpu().numpy() - 11
    np.testing.assert_array_equal(index8.docs.cpu().numpy(), c["dc"][rid])  # in list order
    with pytest.raises(ValueError, match="already fp8"):
        index8.to_fp8()
    # another scale: the oracle's codes of the same rows
    np.testing.assert_array_equal(index.to_fp8(8.0).docs.cpu().numpy(), _q8(c["d"], 8.0)[rid])


@pytest.mark.parametrize("D,npq,k,doc_offset", GRID_CASES)
def test_bit_exact_on_e4m3_grids(gpu, D, npq, k, doc_offset):
    c = _case(D, npq, gpu, doc_offset)
    ref = _ref8(c["qc"], c["dc"], c["rows"], k, doc_offset)
    assert ref[2][-1] == 0 and (k < 1024 or (ref[2][:-1] < k).any())
    assert len(np.unique(ref[1][np.isfinite(ref[1])])) > 3  # the descale is in the scores
    got = _topk8(c["index8"], c["qc"], c["probe"], k, gpu)  # the torch plan, the caller's codes
    _assert_ref(got, ref)
    own = c["index8"].search(c["qt"], k, probe=c["pt"])  # one native call, quantising inside
    _assert_ref(own, ref)
    assert (own[1][-1] == -1).all() and torch.isneginf(own[0][-1]).all()


def test_another_power_of_two_only_moves_the_exponent(gpu):
    c = _case(256, 31, gpu)
    want = _topk8(c["index8"], c["qc"], c["probe"], 100, gpu)
    got = _topk8(c["index8"], c["qc"], c["probe"], 100, gpu, scale=1.0 / 64)
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert torch.equal(got[0], want[0] * 4)


def test_workspaces_of_the_reported_size_filled_with_ones(gpu):
    from irc_amd import _lib, retrieval
    from irc_amd._torch import workspace

    D, npq, k, doc_offset = 256, 33, 100, 11
    c = _case(D, npq, gpu, doc_offset)
    index8, Q, nprobe = c["index8"], c["q"].shape[0], c["probe"].shape[1]
    ref = _ref8(c["qc"], c["dc"], c["rows"], k, doc_offset)
    total = int(retrieval.ivf_plan(c["pt"], index8.list_off)["slot_off"][-1].item())
    nbytes = int(_lib.fn("irc_ivf_topk_workspace")(Q, nprobe, total, k))
    ws = workspace(nbytes, gpu, "ivf8_ff")
    assert ws.numel() == nbytes
    ws.fill_(0xFF)
    got = _topk8(index8, c["qc"], c["probe"], k, gpu, ws_tag="ivf8_ff")
    assert workspace(nbytes, gpu, "ivf8_ff") is ws  # the call ran on that buffer
    _assert_ref(got, ref)
    # the one-call entry: the bound has slack, and the slack is never read
    nlist = index8.centroids.shape[0]
    key_rows = Q * index8.key_bound(nprobe)
    assert total < key_rows
    nbytes = int(_lib.fn("irc_ivf_search_fp8_workspace")(Q, nprobe, nlist, key_rows, k))
    own = index8.search(c["qt"], k, nprobe=nprobe)
    for kw in (dict(probe=c["pt"]), dict(nprobe=nprobe, centroids=index8.centroids)):
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=gpu)
        out = retrieval.ivf_search_fp8(c["qt"], index8.docs, index8.row_id, index8.list_off, k,
                                       key_rows, index8.max_list_rows, query_scale=FP8,
                                       score_scale=SCALE, ws=ws, **kw)
        if "probe" in kw:
            _assert_ref(out, ref)
        else:
            assert _same(out, own)
    with pytest.raises(_lib.IRCError, match="ivf_search_fp8: workspace"):
        retrieval.ivf_search_fp8(c["qt"], index8.docs, index8.row_id, index8.list_off, k,
                                 key_rows, index8.max_list_rows, probe=c["pt"],
                                 ws=ws[:nbytes - 1])


def test_ties_go_to_the_lower_global_id(gpu):
    rng = np.random.default_rng(7)
    N, D, nlist, doc_offset = 1400, 64, 9, 11
    d, = _halve(_grid(rng, (N, D), 3))
    assign = rng.integers(0, nlist, N)
    copies = {1300: 2, 5: 5, 700: 7}  # original id -> list: ids and lists in opposite orders
    for row, lst in copies.items():
        d[row] = d[5]
        assign[row] = lst
    q = np.stack([d[5], _halve(_grid(rng, (D,), 3))[0]])
    probe = np.array([[7, 2, 5], [5, 7, 2]], np.int32)
    index8 = _index(d, _grid(rng, (nlist, D), 3), assign, gpu, doc_offset).to_fp8(FP8)
    ref = _ref8(_q8(q), _q8(d), _rows_of(assign, probe), 1024, doc_offset)
    assert (ref[2] < 1024).all()  # every probed row is returned
    for got in (_topk8(index8, _q8(q), probe, 1024, gpu),
                index8.search(_dev(q, gpu), 1024, probe=_dev(probe, gpu))):
        _assert_ref(got, ref)
        i, s, _ = _np(got)
        for r in range(2):
            at = [int(np.flatnonzero(i[r] == doc_offset + x)[0]) for x in (5, 700, 1300)]
            assert at[0] < at[1] < at[2] and len(set(s[r, at].tolist())) == 1
        assert i[0, :3].tolist() == [16, 711, 1311]  # a row's own pattern scores highest


def test_probing_every_list_is_the_fp8_scan(gpu):
    from irc_amd.retrieval import IVFDenseIndex, ShardedDenseIndex

    rng = np.random.default_rng(3)
    N, D, Q, k, doc_offset = 1501, 128, 33, 50, 9
    q, d = _halve(_grid(rng, (Q, D), 3), _grid(rng, (N, D), 3))
    dt, qt = _dev(d, gpu), _dev(q, gpu)
    index8 = IVFDenseIndex.train(dt, 7, doc_offset, niter=4, dtype="fp8")
    assert index8.dtype == "fp8" and index8.fp8_scale == FP8 and index8.docs.dtype == torch.uint8
    rid = index8.row_id.cpu().numpy() - doc_offset
    np.testing.assert_array_equal(index8.docs.cpu().numpy(), _q8(d)[rid])
    s, i, n = index8.search(qt, k, nprobe=7)
    ri, rs = O.scan_topk_fp8(_q8(q), _q8(d), k, doc_offset, SCALE)
    np.testing.assert_array_equal(i.cpu().numpy(), ri)
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), rs.view(np.uint32))
    assert (n == k).all()
    fs, fi = ShardedDenseIndex(dt, doc_offset, dtype="fp8").search(qt, k)
    assert torch.equal(fi, i) and torch.equal(fs.view(torch.int32), s.view(torch.int32))
    # train(dtype="fp8") is train(...).to_fp8(): the same clustering
    index = IVFDenseIndex.train(dt, 7, doc_offset, niter=4)
    assert torch.equal(index.row_id, index8.row_id) and torch.equal(index.list_off, index8.list_off)
    assert torch.equal(index.centroids, index8.centroids)
    # another scale reaches the lists and the descale
    other = IVFDenseIndex.train(dt, 7, doc_offset, niter=4, dtype="fp8", fp8_scale=32.0)
    assert other.fp8_scale == 32.0
    s2, i2, _ = other.search(qt, k, nprobe=7)
    assert torch.equal(i2, i) and torch.equal(s2, s)  # m / 8 codes, descaled by 1 / 1024


def test_one_accumulation_order_per_query_and_row(gpu):
    rng = np.random.default_rng(11)
    N, D, nlist, lst = 1200, 768, 6, 3
    d = _bf16(_unit(rng.standard_normal((N, D))))
    q = _bf16(_unit(rng.standard_normal((65, D))))
    q[40] = q[0]
    assign = rng.integers(0, nlist, N)
    index8 = _index(d, _bf16(_unit(rng.standard_normal((nlist, D)))), assign, gpu).to_fp8(FP8)
    in_c = np.flatnonzero(assign == lst)
    i1, s1, n1 = _np(index8.search(_dev(q[:1], gpu), 1024, probe=_dev(np.int32([[lst]]), gpu)))
    assert n1[0] == in_c.size and set(i1[0, :in_c.size]) == set(in_c.tolist())
    alone = dict(zip(i1[0, :in_c.size].tolist(), s1[0, :in_c.size].view(np.uint32).tolist()))
    assert len(set(alone.values())) > in_c.size // 2  # rounded sums, not a grid
    probe = np.array([np.roll([lst, (lst + 1 + r % 2) % nlist, (lst + 3) % nlist,
                               (lst + 4) % nlist], (r + 1) % 4) for r in range(65)], np.int32)
    assert probe[40, 0] != lst
    i2, s2, n2 = _np(index8.search(_dev(q, gpu), 1024, probe=_dev(probe, gpu)))
    m = int(n2[40])
    assert m == np.isin(assign, probe[40]).sum() <= 1024
    batch = dict(zip(i2[40, :m].tolist(), s2[40, :m].view(np.uint32).tolist()))
    assert all(batch[row] == bits for row, bits in alone.items())


# ---------------------------------------------------------------- Gaussian rows
_GAUSS = {}


def _gauss(dev):
    if not _GAUSS:
        q, d, cent, assign, probe = _gaussian_case()
        index = _index(d, cent, assign, dev)
        _GAUSS.update(q=q, d=d, assign=assign, probe=probe, index=index,
                      index8=index.to_fp8(FP8), qc=_q8(q), dc=_q8(d),
                      qt=_dev(q, dev).to(torch.bfloat16), pt=_dev(probe, dev))
    return _GAUSS


def test_gaussian_margin_aware(gpu):
    """tests/test_ivf_gpu.py::test_gaussian_margin_aware over the decoded codes times 1 / 256:
    a row may change sides of the k-th score only within the fp32 accumulation tolerance.  On
    the CPU the reference has 3 rows within 2 TOL of their query's k-th score, and an fp32
    emulation of the kernel's order (four slices, ascending 16-wide steps, (s0 + s1) +
    (s2 + s3)) changes no id and is off by at most 1.5e-8, so the cap of 8 has room."""
    g = _gauss(gpu)
    k = 100
    rows = _rows_of(g["assign"], g["probe"])
    ri, rs, rn = _ref8(g["qc"], g["dc"], rows, k)
    full = O.dequantize_e4m3(g["qc"]).astype(np.float64) @ \
        O.dequantize_e4m3(g["dc"]).astype(np.float64).T * SCALE
    Q = full.shape[0]
    near = sum(int((np.abs(full[r, rows[r]] - rs[r, rn[r] - 1]) <= 2 * TOL).sum()) - 1
               for r in range(Q) if rn[r] == k)
    print(f"reference rows within 2 TOL of their query's k-th score (itself excluded): {near}")
    i, s, n = _np(g["index8"].search(g["qt"], k, probe=g["pt"]))
    np.testing.assert_array_equal(n, rn)
    ndiff = 0
    for r in range(Q):
        m = int(rn[r])
        assert (i[r, m:] == -1).all() and np.isneginf(s[r, m:]).all()
        assert set(i[r, :m]) <= set(rows[r].tolist())
        np.testing.assert_allclose(s[r, :m], full[r, i[r, :m]], atol=TOL)
        assert np.all(np.diff(s[r, :m]) <= 0)
        diff = set(i[r, :m]) ^ set(ri[r, :m])
        ndiff += len(diff)
        for doc in diff:
            assert abs(full[r, doc] - rs[r, m - 1]) <= 2 * TOL
    print(f"symmetric differences over the {Q} queries: {ndiff}")
    assert ndiff <= 8


def test_the_call_quantises_the_queries_and_probes_as_its_parent(gpu):
    from irc_amd.retrieval import quantize_fp8

    g = _gauss(gpu)
    index, index8, qt, k = g["index"], g["index8"], g["qt"], 100
    codes = quantize_fp8(qt, FP8)
    np.testing.assert_array_equal(codes.cpu().numpy(), g["qc"])
    np.testing.assert_array_equal(index8.docs.cpu().numpy(),
                                  g["dc"][index.row_id.cpu().numpy()])
    from irc_amd.retrieval import ivf_topk_fp8

    want = ivf_topk_fp8(codes, index8.docs, index8.row_id, index8.list_off, g["pt"], k,
                        index8.max_list_rows, SCALE)
    got = index8.search(qt, k, probe=g["pt"])
    assert _same(got, want)
    # the probe is the bf16 parent's: bf16 queries over bf16 centroids
    for nprobe in (1, 4, 24):
        pr = index8.probe(qt, nprobe)
        assert pr.dtype == torch.int32 and torch.equal(pr, index.probe(qt, nprobe))
        assert _same(index8.search(qt, k, nprobe=nprobe), index8.search(qt, k, probe=pr))
    assert torch.equal(index8.probe(qt, 4), g["pt"])
    assert _same(index8.search(qt, k, nprobe=4), want)
    # fp32 queries that are bf16 values: the same search
    assert _same(index8.search(qt.float(), k, nprobe=4), want)
    # and the scores are the quantised embeddings', not the bf16 index's
    assert not torch.equal(index.search(qt, k, probe=g["pt"])[0], want[0])


def test_search_in_query_chunks_under_a_workspace_limit(gpu, monkeypatch):
    from irc_amd import _lib, retrieval

    c = _case(64, 33, gpu)
    index8, k, nprobe = c["index8"], 10, c["probe"].shape[1]
    nlist = index8.centroids.shape[0]
    whole = index8.search(c["qt"], k, probe=c["pt"])
    whole_own = index8.search(c["qt"], k, nprobe=nprobe)
    sizes = []
    inner = retrieval.ivf_search_fp8

    def counted(queries, *a, **kw):
        sizes.append(queries.shape[0])
        return inner(queries, *a, **kw)

    monkeypatch.setattr(retrieval, "ivf_search_fp8", counted)
    # the limit of 32 queries' workspace: 70 run as 32 + 32 + 6
    limit = int(_lib.fn("irc_ivf_search_fp8_workspace")(32, nprobe, nlist,
                                                        32 * index8.key_bound(nprobe), k))
    monkeypatch.setattr(index8, "max_workspace_bytes", limit, raising=False)
    assert _same(index8.search(c["qt"], k, probe=c["pt"], ws_tag="ivf8_chunks"), whole)
    assert sizes == [32, 32, 6]
    assert _same(index8.search(c["qt"], k, nprobe=nprobe, ws_tag="ivf8_chunks"), whole_own)
    assert sizes == [32, 32, 6] * 2
    monkeypatch.setattr(index8, "max_workspace_bytes", 1 << 30, raising=False)
    assert _same(index8.search(c["qt"], k, probe=c["pt"]), whole) and sizes[6:] == [70]


# ---------------------------------------------------------------- stream order
def test_search_is_captured_in_a_graph_and_replayed(gpu):
    from irc_amd._torch import take_workspace

    c = _case(64, 33, gpu)
    index8, k = c["index8"], 10
    rng = np.random.default_rng(99)
    draws = [_dev(_halve(_grid(rng, c["q"].shape, 3))[0], gpu).to(torch.bfloat16)
             for _ in range(2)]
    static_q = c["qt"].clone()
    tag = "ivf8_graph_test"
    st = torch.cuda.Stream(gpu)
    st.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(st):
        index8.search(static_q, k, nprobe=3, ws_tag=tag)  # warm-up: sizes the workspace
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):  # one stream, no branches
        out = index8.search(static_q, k, nprobe=3, ws_tag=tag)
    ws = take_workspace(gpu, tag)  # the graph points into it: nothing else may grow it
    assert ws is not None
    for q in draws:
        with torch.cuda.stream(st):
            static_q.copy_(q)
            g.replay()
        st.synchronize()
        assert _same(out, index8.search(q, k, nprobe=3))
        assert not _same(out, index8.search(c["qt"], k, nprobe=3))  # the draw's own result


def test_search_makes_no_host_synchronisation(gpu):
    c = _case(64, 33, gpu)
    index, index8, k = c["index"], c["index8"], 10
    want = index8.search(c["qt"], k, probe=c["pt"])  # workspaces sized, nothing left to grow
    want_own = index8.search(c["qt"], k, nprobe=3)
    index.to_fp8(FP8)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = index8.search(c["qt"], k, probe=c["pt"])
        got_own = index8.search(c["qt"], k, nprobe=3)
        again = index.to_fp8(FP8)  # no new host synchronisation either
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert _same(got, want) and _same(got_own, want_own)
    assert torch.equal(again.docs, index8.docs)


# ---------------------------------------------------------------- persistence, shards, CLI
def test_save_load_round_trip_searches_identically(gpu, tmp_path):
    from irc_amd.retrieval import IVFDenseIndex

    c = _case(128, 33, gpu, 11)
    index8 = c["index8"]
    index8.save(str(tmp_path), rank=1)
    again, _ = IVFDenseIndex.load(str(tmp_path), rank=1, device=gpu)
    assert isinstance(again, IVFDenseIndex) and again.max_list_rows == index8.max_list_rows
    assert again.dtype == "fp8" and again.fp8_scale == FP8
    for name in ("docs", "row_id", "list_off", "centroids"):
        a, b = getattr(index8, name), getattr(again, name)
        assert a.dtype == b.dtype and torch.equal(a, b)
    for kw in (dict(probe=c["pt"]), dict(nprobe=3)):
        assert _same(index8.search(c["qt"], 100, **kw), again.search(c["qt"], 100, **kw))
    _assert_ref(again.search(c["qt"], 100, probe=c["pt"]),
                _ref8(c["qc"], c["dc"], c["rows"], 100, 11))


def test_two_halves_merge_to_the_reference(gpu):
    from irc_amd import retrieval

    rng = np.random.default_rng(13)
    N, D, nlist, Q, k = 2000, 128, 6, 25, 64
    q, d = _halve(_grid(rng, (Q, D), 3), _grid(rng, (N, D), 3))
    parts, rows = [], [np.zeros(0, np.int64)] * Q
    for lo, hi in ((0, 900), (900, N)):
        assign = rng.integers(0, nlist, hi - lo)
        probe = np.stack([rng.permutation(nlist)[:2] for _ in range(Q)]).astype(np.int32)
        index8 = _index(d[lo:hi], _grid(rng, (nlist, D), 3), assign, gpu,
                        doc_offset=lo).to_fp8(FP8)
        s, i, _ = index8.search(_dev(q, gpu), k, probe=_dev(probe, gpu))
        parts.append((s, i))
        rows = [np.concatenate([a, lo + b]) for a, b in zip(rows, _rows_of(assign, probe))]
    ms, mi = retrieval.topk_merge(torch.stack([p[0] for p in parts]),
                                  torch.stack([p[1] for p in parts]), k)
    ri, rs, _ = _ref8(_q8(q), _q8(d), rows, k)
    np.testing.assert_array_equal(mi.cpu().numpy(), ri)
    np.testing.assert_array_equal(ms.cpu().numpy().view(np.uint32), rs.view(np.uint32))


def test_main_dense_ivf_fp8_lists_probing_every_list(gpu, tmp_path, capsys):
    import re

    import main as entry
    from test_predict_gpu import _checkpoint, _config, _fever_files

    _fever_files(tmp_path)
    cfg, cfg_path = _config(tmp_path)
    ckpt = _checkpoint(tmp_path, cfg)
    base = ["--data", "fever", "--config", cfg_path, "--ckpt", ckpt, "--gpu", "0",
            "--retrieval", "dense"]
    entry.main(base + ["--index", "flat", "--index-dtype", "fp8"])
    flat = re.findall(r"evidence recall@\d+: ([0-9.]+)", capsys.readouterr().out)
    entry.main(base + ["--index", "ivf", "--nlist", "4", "--nprobe", "4", "--ivf-list-dtype",
                       "fp8"])
    out = capsys.readouterr().out
    ivf = re.findall(r"evidence recall@\d+ \(ivf nlist=4 nprobe=4 lists=fp8\): ([0-9.]+)", out)
    assert len(flat) == 1 and len(ivf) == 1, out
    assert ivf == flat  # all four lists probed: the fp8 scan's ranking
