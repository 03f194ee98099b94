"""Cluster-pruned dense search (IVFDenseIndex, irc_ivf_topk) against a small numpy reference:
per query the union of the rows of its probed lists, the fp64 dot product rounded to fp32,
ranked by (score desc, global id asc) of the ORIGINAL corpus.  Everything approximate about
the index is in which lists are probed, so every check here is exact given the probes."""
import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (import paths)
from oracle import irc_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5  # the project's fp32 accumulation-order tolerance on unit vectors at D = 768


def _grid(rng, shape, lim=127):  # the recipe of tests/test_rerank_gpu.py
    return rng.integers(-lim, lim + 1, shape).astype(np.float32) / 128


def _bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


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


def _index(d, cent, assign, dev, doc_offset=0):
    from irc_amd.retrieval import IVFDenseIndex

    return IVFDenseIndex.from_lists(torch.from_numpy(d).to(dev), torch.from_numpy(cent).to(dev),
                                    torch.from_numpy(assign).to(dev), doc_offset)


def _search(index, q, k, dev, **kw):
    if "probe" in kw:
        kw["probe"] = torch.from_numpy(np.asarray(kw["probe"], np.int32)).to(dev)
    s, i, n = index.search(torch.from_numpy(q).to(dev), k, **kw)
    return i.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()


def _cycle():
    from irc_amd.retrieval import IVF_TILE_ROWS as T

    return [0, 1, 31, 32, 33, T - 1, T, T + 1, 2 * T + 7]


L33, LT1 = 4, 7  # the lists of lengths 33 and T + 1 in the cycle
OTHERS = [0, 1, 2, 3, 5, 6, 8]


def _grid_case(D, npq, Q=70, nprobe=4):
    """One cycle of list lengths (the smallest N that holds it; the last list, the longest,
    ends at row N), rows scattered over the original ids; the lists of lengths 33 and T + 1
    probed by the first npq queries, the other slots cycling through the other lists with a
    -1 here and there, each probe row rotated, the last query probing nothing."""
    lens = _cycle()
    N = sum(lens)
    assert N % 32 != 0 and lens[-1] > 0
    rng = np.random.default_rng(1000 * D + npq)
    assign = rng.permutation(np.repeat(np.arange(len(lens)), lens))
    q, d = _grid(rng, (Q, D), 3), _grid(rng, (N, D), 3)
    cent = _grid(rng, (len(lens), D), 3)
    probe = np.full((Q, nprobe), -1, np.int32)
    for r in range(Q - 1):
        row = [L33, LT1] if r < npq else []
        row += [OTHERS[(r + j) % len(OTHERS)] for j in range(nprobe - len(row))]
        if r % 5 == 3:
            row[-1] = -1
        probe[r] = np.roll(row, r % nprobe)
    assert ((probe == L33).sum(), (probe == LT1).sum()) == (npq, npq)
    return q, d, cent, assign, probe


GRID_CASES = [(64, 0, 1, 0), (128, 1, 10, 11), (256, 31, 100, 0), (384, 32, 1024, 11),
              (512, 33, 10, 0), (768, 65, 100, 11), (1024, 32, 1024, 0), (128, 65, 1024, 11)]


@pytest.mark.parametrize("D,npq,k,doc_offset", GRID_CASES)
def test_bit_exact_on_integer_grids(gpu, D, npq, k, doc_offset):
    q, d, cent, assign, probe = _grid_case(D, npq)
    rows = _rows_of(assign, probe)
    ri, rs, rn = _reference(q, d, rows, k, doc_offset)
    assert rn[-1] == 0 and (k < 1024 or (rn[:-1] < k).any())  # an empty query; k above a count
    i, s, n = _search(_index(d, cent, assign, gpu, doc_offset), q, k, gpu, probe=probe)
    np.testing.assert_array_equal(n, rn)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)
    assert (i[-1] == -1).all() and np.isneginf(s[-1]).all()


def test_workspace_of_the_reported_size_needs_no_clearing(gpu):
    from irc_amd import _lib, retrieval
    from irc_amd._torch import workspace

    D, npq, k, doc_offset = 256, 33, 100, 11
    q, d, cent, assign, probe = _grid_case(D, npq)
    index = _index(d, cent, assign, gpu, doc_offset)
    pr = torch.from_numpy(probe).to(gpu)
    total = int(retrieval.ivf_plan(pr, index.list_off)["slot_off"][-1].item())
    assert total == sum(r.size for r in _rows_of(assign, probe))
    nbytes = int(_lib.fn("irc_ivf_topk_workspace")(q.shape[0], probe.shape[1], total, k))
    ws = workspace(nbytes, gpu, "ivf_ff")
    assert ws.numel() == nbytes
    ws.fill_(0xFF)
    s, i, n = retrieval.ivf_topk(torch.from_numpy(q).to(gpu), index.docs, index.row_id,
                                 index.list_off, pr, k, index.max_list_rows, ws_tag="ivf_ff")
    assert workspace(nbytes, gpu, "ivf_ff") is ws  # the call ran on that buffer
    ri, rs, rn = _reference(q, d, _rows_of(assign, probe), k, doc_offset)
    np.testing.assert_array_equal(n.cpu().numpy(), rn)
    np.testing.assert_array_equal(i.cpu().numpy(), ri)
    np.testing.assert_array_equal(s.cpu().numpy(), rs)
    # total_rows= (an upper bound) replaces the call's one host synchronisation: same result
    s2, i2, n2 = retrieval.ivf_topk(torch.from_numpy(q).to(gpu), index.docs, index.row_id,
                                    index.list_off, pr, k, index.max_list_rows, ws_tag="ivf_ub",
                                    total_rows=total + 777)
    assert torch.equal(s2, s) and torch.equal(i2, i) and torch.equal(n2, n)


def test_ties_go_to_the_lower_global_id(gpu):
    rng = np.random.default_rng(7)
    N, D, nlist, doc_offset = 1400, 64, 9, 11
    d = _grid(rng, (N, D), 3)
    assign = rng.integers(0, nlist, N)
    copies = {1300: 2, 5: 5, 700: 7}  # original id -> list: ids and lists in opposite orders
    for row, c in copies.items():
        d[row] = d[5]
        assign[row] = c
    q = np.stack([d[5], _grid(rng, (D,), 3)])
    probe = np.array([[7, 2, 5], [5, 7, 2]], np.int32)
    i, s, n = _search(_index(d, _grid(rng, (nlist, D), 3), assign, gpu, doc_offset), q, 1024, gpu,
                      probe=probe)
    ri, rs, rn = _reference(q, d, _rows_of(assign, probe), 1024, doc_offset)
    assert (rn < 1024).all()  # every probed row is returned
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)
    for r in range(2):
        at = [int(np.flatnonzero(i[r] == doc_offset + x)[0]) for x in (5, 700, 1300)]
        assert at[0] < at[1] < at[2] and len(set(s[r, at].tolist())) == 1  # ascending global id
    assert i[0, :3].tolist() == [16, 711, 1311]  # a row's own pattern scores highest


def test_probing_every_list_is_the_scan(gpu):
    from irc_amd.retrieval import IVFDenseIndex

    rng = np.random.default_rng(3)
    N, D, Q, k, doc_offset = 1501, 128, 33, 50, 9
    q, d = _grid(rng, (Q, D), 3), _grid(rng, (N, D), 3)
    index = IVFDenseIndex.train(torch.from_numpy(d).to(gpu), 7, doc_offset, niter=4)
    i, s, n = _search(index, q, k, gpu, nprobe=7)
    ri, rs = O.scan_topk(q, d, k, doc_offset=doc_offset)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)
    assert (n == k).all()


def test_one_accumulation_order_per_query_and_row(gpu):
    rng = np.random.default_rng(11)
    N, D, nlist, c = 1200, 768, 6, 3
    d = _bf16(_unit(rng.standard_normal((N, D))))
    q = _bf16(_unit(rng.standard_normal((65, D))))
    q[40] = q[0]
    assign = rng.integers(0, nlist, N)
    index = _index(d, _bf16(_unit(rng.standard_normal((nlist, D)))), assign, gpu)
    in_c = np.flatnonzero(assign == c)
    i1, s1, n1 = _search(index, q[:1], 1024, gpu, probe=[[c]])
    assert n1[0] == in_c.size and set(i1[0, :in_c.size]) == set(in_c.tolist())
    alone = dict(zip(i1[0, :in_c.size].tolist(), s1[0, :in_c.size].view(np.uint32).tolist()))
    probe = np.array([np.roll([c, (c + 1 + r % 2) % nlist, (c + 3) % nlist, (c + 4) % nlist],
                              (r + 1) % 4) for r in range(65)], np.int32)
    assert probe[40, 0] != c and (np.sort(probe, 1)[:, 1:] != np.sort(probe, 1)[:, :-1]).all()
    i2, s2, n2 = _search(index, q, 1024, gpu, probe=probe)
    m = int(n2[40])
    assert m == np.isin(assign, probe[40]).sum() <= 1024
    batch = dict(zip(i2[40, :m].tolist(), s2[40, :m].view(np.uint32).tolist()))
    assert all(batch[row] == bits for row, bits in alone.items())


def _gaussian_case():
    rng = np.random.default_rng(2025)
    nlist, N, Q, D = 24, 6000, 40, 768
    C = _unit(rng.standard_normal((nlist, D)))
    own = rng.integers(0, nlist, N)
    d = _bf16(_unit(0.5 * C[own] + _unit(rng.standard_normal((N, D)))))
    qown = rng.integers(0, nlist, Q)
    q = _bf16(_unit(0.5 * C[qown] + _unit(rng.standard_normal((Q, D)))))
    cent = _bf16(C)
    c64 = cent.astype(np.float64)
    assign = np.argmax(d.astype(np.float64) @ c64.T, axis=1)
    probe = np.argsort(-(q.astype(np.float64) @ c64.T), axis=1, kind="stable")[:, :4]
    return q, d, cent, assign, probe.astype(np.int32)


def test_gaussian_margin_aware(gpu):
    """The checks of tests/test_rerank_gpu.py::test_gaussian_margin_aware on an IVF search:
    a row may change sides of the k-th score only within the fp32 accumulation tolerance."""
    q, d, cent, assign, probe = _gaussian_case()
    k = 100
    rows = _rows_of(assign, probe)
    ri, rs, rn = _reference(q, d, rows, k)
    full = q.astype(np.float64) @ d.astype(np.float64).T
    near = sum(int((np.abs(full[r, rows[r]] - rs[r, rn[r] - 1]) <= 2 * TOL).sum()) - 1
               for r in range(q.shape[0]) if rn[r] == k)
    print(f"reference rows within 2 TOL of their query's k-th score (itself excluded): {near}")
    i, s, n = _search(_index(d, cent, assign, gpu), q, k, gpu, probe=probe)
    np.testing.assert_array_equal(n, rn)
    ndiff = 0
    for r in range(q.shape[0]):
        m = int(rn[r])
        assert (i[r, m:] == -1).all() and np.isneginf(s[r, m:]).all()
        assert set(i[r, :m]) <= set(rows[r].tolist())
        np.testing.assert_allclose(s[r, :m], full[r, i[r, :m]], atol=TOL)
        assert np.all(np.diff(s[r, :m]) <= 0)
        diff = set(i[r, :m]) ^ set(ri[r, :m])
        ndiff += len(diff)
        for doc in diff:
            assert abs(full[r, doc] - rs[r, m - 1]) <= 2 * TOL
    print(f"symmetric differences over the {q.shape[0]} queries: {ndiff}")
    assert ndiff <= 8


def test_probe_is_the_scan_over_the_centroids(gpu):
    from irc_amd import retrieval

    rng = np.random.default_rng(5)
    nlist, D = 37, 128
    cent, q = _grid(rng, (nlist, D), 3), _grid(rng, (20, D), 3)
    cent[9] = cent[4]  # a tie between two lists: the lower list id first
    index = _index(_grid(rng, (100, D), 3), cent, rng.integers(0, nlist, 100), gpu)
    qt = torch.from_numpy(q).to(gpu)
    for nprobe in (1, 5, nlist):
        p = index.probe(qt, nprobe)
        assert p.dtype == torch.int32 and tuple(p.shape) == (20, nprobe)
        want = retrieval.scan_topk(qt, index.centroids, nprobe)[1]
        np.testing.assert_array_equal(p.cpu().numpy(), want.cpu().numpy())
        np.testing.assert_array_equal(p.cpu().numpy(), O.scan_topk(q, cent, nprobe)[0])
    assert (np.sort(p.cpu().numpy(), axis=1) == np.arange(nlist)).all()
    for bad in (0, nlist + 1):
        with pytest.raises(ValueError, match="nprobe"):
            index.probe(qt, bad)


def _check_trained(index, d, nlist, doc_offset, dev):
    from irc_amd import cluster

    N = d.shape[0]
    rid = index.row_id.cpu().numpy()
    lo = index.list_off.cpu().numpy()
    assert index.row_id.dtype == torch.int32 and index.list_off.dtype == torch.int64
    np.testing.assert_array_equal(np.sort(rid), doc_offset + np.arange(N))
    assert lo[0] == 0 and lo[-1] == N and lo.size == nlist + 1 and (np.diff(lo) >= 0).all()
    assert index.max_list_rows == np.diff(lo).max()
    np.testing.assert_array_equal(index.docs.float().cpu().numpy(), _bf16(d)[rid - doc_offset])
    assert index.centroids.dtype == torch.bfloat16 and tuple(index.centroids.shape) == \
        (nlist, d.shape[1])
    # every row sits in the list _assign gives it: the largest inner product with the
    # centroids the index keeps, which are the ones the probe ranks by
    a, _ = cluster._assign(torch.from_numpy(d).to(dev), index.centroids.float().contiguous(),
                           torch.zeros(nlist, device=dev))
    a = a.cpu().numpy()
    for c in range(nlist):
        seg = rid[lo[c]:lo[c + 1]] - doc_offset
        assert (np.diff(seg) > 0).all() and (a[seg] == c).all()
    return a


def test_train_builds_consistent_lists(gpu):
    from irc_amd.retrieval import IVFDenseIndex

    rng = np.random.default_rng(8)
    N, D, nlist, doc_offset = 3000, 128, 12, 5
    C = _unit(rng.standard_normal((nlist, D)))
    d = _unit(0.6 * C[rng.integers(0, nlist, N)] + _unit(rng.standard_normal((N, D))))
    d = d.astype(np.float32)
    index = IVFDenseIndex.train(torch.from_numpy(d).to(gpu), nlist, doc_offset, niter=5)
    _check_trained(index, d, nlist, doc_offset, gpu)


def test_train_on_a_skewed_corpus_searches_to_the_reference(gpu):
    from irc_amd.retrieval import IVFDenseIndex

    rng = np.random.default_rng(9)
    N, D, nlist, Q, k = 6000, 128, 8, 20, 50  # N / nlist > 2 T: some list is cut
    C = _unit(rng.standard_normal((nlist, D)))
    own = np.where(rng.random(N) < 0.9, 0, rng.integers(1, nlist, N))
    d = _bf16(_unit(0.7 * C[own] + _unit(rng.standard_normal((N, D)))))
    q = _bf16(_unit(0.7 * C[rng.integers(0, nlist, Q)] + _unit(rng.standard_normal((Q, D)))))
    index = IVFDenseIndex.train(torch.from_numpy(d).to(gpu), nlist, niter=5)
    a = _check_trained(index, d, nlist, 0, gpu)
    from irc_amd.retrieval import IVF_TILE_ROWS as T

    assert index.max_list_rows > 2 * T  # a long list, cut into segments
    probe = index.probe(torch.from_numpy(q).to(gpu), 2).cpu().numpy()
    i, s, n = _search(index, q, k, gpu, nprobe=2)
    rows = _rows_of(a, probe)
    ri, rs, rn = _reference(q, d, rows, k)
    full = q.astype(np.float64) @ d.astype(np.float64).T
    np.testing.assert_array_equal(n, rn)
    for r in range(Q):
        m = int(rn[r])
        np.testing.assert_allclose(s[r, :m], full[r, i[r, :m]], atol=TOL)
        for doc in set(i[r, :m]) ^ set(ri[r, :m]):
            assert abs(full[r, doc] - rs[r, m - 1]) <= 2 * TOL


def test_two_halves_merge_to_the_reference(gpu):
    from irc_amd import retrieval

    rng = np.random.default_rng(13)
    N, D, nlist, Q, k = 2000, 128, 6, 25, 64
    q, d = _grid(rng, (Q, D), 3), _grid(rng, (N, D), 3)
    parts, rows = [], [np.zeros(0, np.int64)] * Q
    for lo, hi in ((0, N // 2), (N // 2, N)):
        assign = rng.integers(0, nlist, hi - lo)
        probe = np.stack([rng.permutation(nlist)[:2] for _ in range(Q)]).astype(np.int32)
        index = _index(d[lo:hi], _grid(rng, (nlist, D), 3), assign, gpu, doc_offset=lo)
        s, i, _ = index.search(torch.from_numpy(q).to(gpu), k,
                               probe=torch.from_numpy(probe).to(gpu))
        parts.append((s, i))
        rows = [np.concatenate([a, lo + b]) for a, b in zip(rows, _rows_of(assign, probe))]
    ms, mi = retrieval.topk_merge(torch.stack([p[0] for p in parts]),
                                  torch.stack([p[1] for p in parts]), k)
    ri, rs, _ = _reference(q, d, rows, k)
    np.testing.assert_array_equal(mi.cpu().numpy(), ri)
    np.testing.assert_array_equal(ms.cpu().numpy(), rs)


def test_save_load_round_trip_searches_identically(gpu, tmp_path):
    from irc_amd.retrieval import IVFDenseIndex

    q, d, cent, assign, probe = _grid_case(128, 33)
    index = _index(d, cent, assign, gpu, doc_offset=11)
    index.save(str(tmp_path), rank=1)
    again, _ = IVFDenseIndex.load(str(tmp_path), rank=1, device=gpu)
    assert isinstance(again, IVFDenseIndex) and again.max_list_rows == index.max_list_rows
    for name in ("docs", "row_id", "list_off", "centroids"):
        a, b = getattr(index, name), getattr(again, name)
        assert a.dtype == b.dtype and torch.equal(a, b)
    for kw in (dict(probe=probe), dict(nprobe=3)):
        for x, y in zip(_search(index, q, 100, gpu, **kw), _search(again, q, 100, gpu, **kw)):
            np.testing.assert_array_equal(x, y)


def test_main_dense_ivf_probing_every_list(gpu, tmp_path, capsys):
    import re

    import main as entry
    from test_predict_gpu import _checkpoint, _config, _fever_files

    _fever_files(tmp_path)
    cfg, cfg_path = _config(tmp_path)
    ckpt = _checkpoint(tmp_path, cfg)
    base = ["--data", "fever", "--config", cfg_path, "--ckpt", ckpt, "--gpu", "0",
            "--retrieval", "dense"]
    entry.main(base + ["--index", "flat"])
    flat = re.findall(r"evidence recall@\d+: ([0-9.]+)", capsys.readouterr().out)
    entry.main(base + ["--index", "ivf", "--nlist", "4", "--nprobe", "4"])
    out = capsys.readouterr().out
    ivf = re.findall(r"evidence recall@\d+ \(ivf nlist=4 nprobe=4\): ([0-9.]+)", out)
    assert len(flat) == 1 and len(ivf) == 1, out
    assert ivf == flat  # all four lists probed: the scan's ranking
