"""CPU checks of the candidate top-k per group (irc_rerank_topk_grouped): the numpy reference
the GPU tests use, on two hand-written cases; the entry's host-side validation; the
``group_off`` checks of the Python wrappers; main.py's flag; hybrid_search's signature (no
compute without a GPU)."""
import inspect

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT  # noqa: F401  (import paths)
from oracle import irc_oracle as O

from irc_amd import _lib, retrieval


def _reference_grouped(q, d, lists, k, group_off, doc_offset=0):
    """(idx [Q, k], scores [Q, k], n [Q], groups [Q, k]): per list the eligible candidates
    (rows of this shard that lie in a group), fp64 scores cast to fp32, per group the
    maximum with the lower id on ties, then O.topk_rows over the winners in ascending id
    order.  group_off in global row ids, group g = [group_off[g], group_off[g + 1])."""
    Q, N = q.shape[0], d.shape[0]
    go = np.asarray(group_off, np.int64)
    out_i = np.full((Q, k), -1, np.int64)
    out_s = np.full((Q, k), -np.inf, np.float32)
    out_n = np.zeros(Q, np.int32)
    out_g = np.full((Q, k), -1, np.int64)
    q64, d64 = q.astype(np.float64), d.astype(np.float64)
    for r, ids in enumerate(lists):
        ids = np.asarray(ids, np.int64)
        ok = np.unique(ids[(ids >= doc_offset) & (ids < doc_offset + N) &
                           (ids >= go[0]) & (ids < go[-1])])
        if ok.size == 0:
            continue
        sc = (d64[ok - doc_offset] @ q64[r]).astype(np.float32)
        grp = np.searchsorted(go, ok, side="right") - 1
        # ok ascends, so do the groups: the first row of each stretch and its length
        first = np.flatnonzero(np.r_[True, grp[1:] != grp[:-1]])
        stop = np.r_[first[1:], ok.size]
        win = np.array([a + int(np.argmax(sc[a:b])) for a, b in zip(first, stop)])  # first max
        ti, ts = O.topk_rows(sc[win][None, :], k)  # ascending ids: ties -> lower id
        m = min(k, win.size)
        out_i[r, :m] = ok[win[ti[0, :m]]]
        out_s[r, :m] = ts[0, :m]
        out_g[r, :m] = grp[win[ti[0, :m]]]
        out_n[r] = m
    return out_i, out_s, out_n, out_g


def test_reference_on_a_hand_written_case():
    # one query along e0; rows 0..5 score 1, 3, 3, 2, 5, 4; groups {0}, {1, 2}, {}, {3, 4}
    # and row 5 in no group
    q = np.array([[1.0, 0.0]], np.float32)
    d = np.array([[1, 0], [3, 1], [3, 2], [2, 0], [5, 0], [4, 0]], np.float32)
    go = [0, 1, 3, 3, 5]
    i, s, n, g = _reference_grouped(q, d, [[0, 1, 2, 3, 4, 5]], 4, go)
    assert n.tolist() == [3]
    assert i.tolist() == [[4, 1, 0, -1]]  # the tie in group 1 goes to row 1
    assert s.tolist() == [[5.0, 3.0, 1.0, -np.inf]]
    assert g.tolist() == [[3, 1, 0, -1]]
    # k below the group count keeps the best groups only
    i, s, n, g = _reference_grouped(q, d, [[0, 1, 2, 3, 4, 5]], 2, go)
    assert (i.tolist(), n.tolist(), g.tolist()) == ([[4, 1]], [2], [[3, 1]])


def test_reference_with_an_offset_shard_foreign_rows_and_two_lists():
    # the shard holds global rows 10..13 (scores 2, 7, 7, 1 for query 0; negated for query
    # 1); groups in global ids: {8, 9, 10}, {11}, {12, 13, 14}
    q = np.array([[1.0], [-1.0]], np.float32)
    d = np.array([[2.0], [7.0], [7.0], [1.0]], np.float32)
    go = [8, 11, 12, 15]
    lists = [[9, 10, 11, 12, 13, 14, 40], [8, 9, 14]]  # list 1: foreign rows only
    i, s, n, g = _reference_grouped(q, d, lists, 3, go, doc_offset=10)
    assert n.tolist() == [3, 0]
    assert i.tolist() == [[11, 12, 10], [-1, -1, -1]]  # equal scores: the lower row first
    assert g.tolist() == [[1, 2, 0], [-1, -1, -1]]
    assert s[0].tolist() == [7.0, 7.0, 2.0] and np.isneginf(s[1]).all()
    # the same group in two lists stays two runs
    i, s, n, g = _reference_grouped(q, d, [[12], [13]], 1, go, doc_offset=10)
    assert (i.tolist(), g.tolist(), s.tolist()) == ([[12], [13]], [[2], [2]], [[7.0], [-1.0]])


def _call(lib, D, k, Q=4, N=10, n_cand=0, ws=0, doc_offset=0, group_off=None, n_groups=0,
          flags=0, scale=1.0):
    return lib.irc_rerank_topk_grouped(None, None, Q, N, D, None, None, n_cand, k, doc_offset,
                                       group_off, n_groups, flags, scale, None, ws, None, None,
                                       None, None)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_grouped_entry_rejects_bad_arguments_on_the_host(flags):
    lib = _lib.load()
    assert lib.irc_abi_version() == 2  # the additions are additive
    assert _call(lib, 100, 5, flags=flags) == 1001
    assert b"unsupported D" in lib.irc_last_error()
    assert _call(lib, 128, 0, flags=flags) == 1001
    assert b"k=0" in lib.irc_last_error()
    assert _call(lib, 128, 1025, flags=flags) == 1001
    assert b"k=1025" in lib.irc_last_error()
    assert _call(lib, 128, 5, Q=-1, flags=flags) == 1001
    assert b"negative size" in lib.irc_last_error()
    assert _call(lib, 128, 5, N=1 << 31, flags=flags) == 1001
    assert b"fit int32" in lib.irc_last_error()
    # score_scale: a power of two for e4m3, ignored for bf16
    rc = _call(lib, 128, 5, n_cand=1000, scale=3.0, flags=flags)
    assert rc == (1001 if flags & 2 else 1002)
    # D = 64 runs everywhere but in the e4m3 stream kernel
    assert _call(lib, 64, 5, n_cand=1000, flags=flags) == (1001 if flags == 3 else 1002)
    # every shape check passed: the workspace code, before the pointer and group checks
    assert _call(lib, 128, 5, n_cand=1000, flags=flags) == 1002
    assert b"workspace" in lib.irc_last_error()
    assert _call(lib, 128, 5, n_cand=1000, ws=8, flags=flags) == 1002


def test_grouped_workspace_holds_three_arrays_per_candidate():
    lib = _lib.load()
    for n in (0, 1, 255, 256, 1000, 1 << 20):
        one = int(lib.irc_rerank_topk_workspace(4, n, 10))
        grouped = int(lib.irc_rerank_topk_grouped_workspace(4, n, 10))
        assert grouped >= 3 * 8 * n and grouped >= one
    assert int(lib.irc_rerank_topk_workspace(4, 1000, 10)) == ((8000 + 255) // 256) * 256 + 256


def test_grouped_entry_is_registered():
    assert "irc_rerank_topk_grouped" in _lib.SIGNATURES
    assert "irc_rerank_topk_grouped_workspace" in _lib.SIGNATURES
    assert retrieval.RERANK_FLAG_STREAM == 1 and retrieval.RERANK_FLAG_E4M3 == 2


def _cpu_args(dtype):
    return (torch.zeros(2, 128, dtype=dtype), torch.zeros(4, 128, dtype=dtype),
            torch.zeros(3, dtype=torch.int32), torch.tensor([0, 1, 3]), 2)


BAD_GROUP_OFF = [(torch.zeros(3, dtype=torch.int32), TypeError),
                 (torch.zeros(3, dtype=torch.float32), TypeError),
                 ([0, 2, 4], TypeError),
                 (torch.zeros((2, 2), dtype=torch.int64), ValueError),
                 (torch.zeros((), dtype=torch.int64), ValueError),
                 (torch.zeros(0, dtype=torch.int64), ValueError)]


@pytest.mark.parametrize("method", ["gather", "stream"])
@pytest.mark.parametrize("bad,exc", BAD_GROUP_OFF)
def test_wrappers_check_group_off_before_the_library(monkeypatch, method, bad, exc):
    def boom(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "fn", boom)
    with pytest.raises(exc, match="group_off"):
        retrieval.rerank_topk(*_cpu_args(torch.bfloat16), method=method, group_off=bad)
    with pytest.raises(exc, match="group_off"):
        retrieval.rerank_topk_fp8(*_cpu_args(torch.uint8), method=method, group_off=bad)
    idx = retrieval.ShardedDenseIndex.__new__(retrieval.ShardedDenseIndex)
    idx.dtype, idx.group, idx.doc_offset, idx.fp8_scale = "bf16", None, 0, 16.0
    idx.docs = torch.zeros(4, 128, dtype=torch.bfloat16)
    q, _, c, off, k = _cpu_args(torch.bfloat16)
    with pytest.raises(exc, match="group_off"):
        idx.search_candidates(q, c, off, k, method=method, group_off=bad)


def test_a_good_group_off_reaches_the_device_check():
    go = torch.tensor([0, 2, 4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.rerank_topk(*_cpu_args(torch.bfloat16), group_off=go)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.rerank_topk_fp8(*_cpu_args(torch.uint8), group_off=go)


def test_main_parses_rerank_unit():
    import main as entry

    assert entry.get_args([]).rerank_unit == "line"
    assert entry.get_args(["--rerank-unit", "page"]).rerank_unit == "page"
    assert entry.get_args(["--rerank-unit", "line"]).rerank_unit == "line"
    with pytest.raises(SystemExit):
        entry.get_args(["--rerank-unit", "paragraph"])
    assert "--rerank-unit line|page" in entry.__doc__


def test_signatures_accept_group_off():
    from src.evaluation import hybrid_search

    for f in (hybrid_search, retrieval.rerank_topk, retrieval.rerank_topk_fp8,
              retrieval.ShardedDenseIndex.search_candidates):
        p = inspect.signature(f).parameters["group_off"]
        assert p.default is None
