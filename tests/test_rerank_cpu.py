"""CPU checks of the candidate-restricted top-k (sparse filter, dense rerank): the
host-side validation of irc_rerank_topk, its workspace, and the pure-torch plumbing
around it (no compute without a GPU)."""
import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (import paths)

from irc_amd import _lib, retrieval


def _call(lib, D, k, Q=4, N=10, n_cand=0, ws=0):
    return lib.irc_rerank_topk(None, None, Q, N, D, None, None, n_cand, k, 0, None, ws, None,
                               None, None, None)


def test_rerank_rejects_bad_shapes_on_the_host():
    lib = _lib.load()
    assert lib.irc_abi_version() == 2
    assert _call(lib, 100, 5) == 1001
    assert b"unsupported D" in lib.irc_last_error()
    assert _call(lib, 128, 0) == 1001
    assert b"k=0" in lib.irc_last_error()
    assert _call(lib, 128, 1025) == 1001
    assert b"k=1025" in lib.irc_last_error()
    assert _call(lib, 128, 5, Q=-1) == 1001
    assert _call(lib, 128, 5, n_cand=-1) == 1001
    assert _call(lib, 128, 5, N=1 << 31) == 1001  # doc_offset + N < 2^31
    # every shape check passed, no workspace: the workspace code
    assert _call(lib, 128, 5, n_cand=1000) == 1002


def test_rerank_workspace_monotone_in_n_cand():
    lib = _lib.load()
    sizes = [lib.irc_rerank_topk_workspace(256, n, 100)
             for n in (0, 1, 255, 256, 257, 5000, 10 ** 6, 10 ** 8)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] >= 1
    assert sizes[-1] >= 8 * 10 ** 8  # one 64-bit key per candidate


def test_rerank_chunk_constant_comes_from_the_library():
    from irc_amd.retrieval import RERANK_CHUNK

    assert RERANK_CHUNK == retrieval.RERANK_CHUNK == _lib.load().irc_rerank_chunk()
    assert RERANK_CHUNK >= 8 and RERANK_CHUNK % 8 == 0  # whole 8-lane row groups
    with pytest.raises(AttributeError):
        retrieval.NO_SUCH_NAME


def test_rerank_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.rerank_topk(torch.zeros(2, 128), torch.zeros(4, 128),
                              torch.zeros(3, dtype=torch.int32),
                              torch.tensor([0, 1, 3]), 2)


def _expand_loop(cand, off, row_off):
    rows, rows_off = [], [0]
    for q in range(len(off) - 1):
        for c in cand[off[q]:off[q + 1]]:
            rows.extend(range(row_off[c], row_off[c + 1]))
        rows_off.append(len(rows))
    return rows, rows_off


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_expand_ranges_matches_a_python_loop(dtype):
    # 7 columns: column 0 and the last own rows, columns 2 and 4 are empty ranges
    row_off = [0, 3, 4, 4, 9, 9, 10, 12]
    lists = [[], [0], [2], [0, 6], [1, 2, 3, 4, 5], [], [6], [2, 4], list(range(7)), []]
    cand = [c for lst in lists for c in lst]
    off = np.concatenate([[0], np.cumsum([len(lst) for lst in lists])]).tolist()
    rows, rows_off = retrieval.expand_ranges(torch.tensor(cand, dtype=dtype),
                                             torch.tensor(off, dtype=torch.int64),
                                             torch.tensor(row_off, dtype=torch.int64))
    ref_rows, ref_off = _expand_loop(cand, off, row_off)
    assert rows.dtype == torch.int64 and rows_off.dtype == torch.int64
    assert rows.tolist() == ref_rows
    assert rows_off.tolist() == ref_off
    for q in range(len(lists)):  # ascending and unique stays so
        r = rows[rows_off[q]:rows_off[q + 1]].tolist()
        assert r == sorted(set(r))


def test_expand_ranges_without_candidates():
    rows, rows_off = retrieval.expand_ranges(torch.zeros(0, dtype=torch.int32),
                                             torch.zeros(4, dtype=torch.int64),
                                             torch.tensor([0, 2, 5]))
    assert rows.tolist() == [] and rows_off.tolist() == [0, 0, 0, 0]


def test_main_parses_retrieval_hybrid():
    import main as entry

    assert entry.get_args(["--retrieval", "hybrid"]).retrieval == "hybrid"
    assert entry.get_args([]).retrieval == "sparse"


def test_search_candidates_refuses_fp8_and_hybrid_corpus_order():
    from src.evaluation import hybrid_corpus

    idx = retrieval.ShardedDenseIndex.__new__(retrieval.ShardedDenseIndex)
    idx.dtype, idx.group, idx.doc_offset, idx.docs = "fp8", None, 0, torch.zeros(2, 64)
    with pytest.raises(ValueError, match="fp8"):
        idx.search_candidates(torch.zeros(1, 64), torch.zeros(0, dtype=torch.int32),
                              torch.zeros(2, dtype=torch.int64), 1)
    wiki = {"B": {"lines": ["b0", "", "b2"]}, "A": {"lines": ["a0"]}}
    titles, texts, row_off = hybrid_corpus(wiki, ["A", "missing", "B"])
    assert titles == ["A", "B", "B"] and texts == ["a0", "b0", "b2"]
    assert row_off == [0, 1, 1, 3]
