"""CPU checks of the one-call cluster-pruned search: the ORDER of irc_ivf_plan's and
irc_ivf_search's host-side argument checks (they read no memory, so pointers are null or plain
host buffers), the workspace function, ``IVFDenseIndex.key_bound`` on hand-written lengths and
as a bound on ``ivf_plan``'s key total, the chunk-size function, and the wrappers' own checks
with no device (tests/test_ivf_native_gpu.py covers the kernels).

The order of the native checks:

  irc_ivf_plan    sizes, nprobe, Q x nprobe, workspace, Q == 0 return, null pointers
  irc_ivf_search  sizes, k, D, nprobe, the probe's own limit (1024 lists, when the call probes
                  itself), int32 ids (N), Q x nprobe, max_list_rows, workspace, Q == 0 return,
                  null pointers, alignment"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT  # noqa: F401  (import paths)

from irc_amd import _lib

INVALID, WORKSPACE = 1001, 1002

_BUF = ctypes.create_string_buffer(4096 + 16)
_ALIGNED = (ctypes.addressof(_BUF) + 15) & ~15  # a 16-byte aligned host address


def _ws(nbytes):
    buf = ctypes.create_string_buffer(max(int(nbytes), 1))
    return dict(ws=ctypes.addressof(buf), ws_bytes=int(nbytes), _keep=buf)


def _param(cases):
    return [pytest.param(*c[1:], id=c[0]) for c in cases]


# ---------------------------------------------------------------- irc_ivf_plan
PLAN_ARRAYS = ("probe", "list_off", "slot_off", "cand_off", "pair_order", "seg_off", "chunk_off")
PLAN_POINTERS = {name: _ALIGNED for name in PLAN_ARRAYS}


def _plan_need(lib, Q=4, nprobe=2, nlist=3):
    return int(lib.irc_ivf_plan_workspace(Q, nprobe, nlist))


def _plan_call(lib, Q=4, nprobe=2, nlist=3, i64=0, ws=None, ws_bytes=0, _keep=None, **ptrs):
    a = {name: ptrs.get(name) for name in PLAN_ARRAYS}
    return lib.irc_ivf_plan(a["probe"], i64, a["list_off"], Q, nprobe, nlist, ws, ws_bytes,
                            a["slot_off"], a["cand_off"], a["pair_order"], a["seg_off"],
                            a["chunk_off"], None)


PLAN_HAVE_WS = _ws(_plan_need(_lib.load()))
# (id, arguments, return code, text of the check that reports)
PLAN_SINGLE = [
    ("size_Q", dict(Q=-1), INVALID, b"negative size"),
    ("size_nlist", dict(nlist=-1), INVALID, b"negative size"),
    ("nprobe_low", dict(nprobe=0), INVALID, b"nprobe=0"),
    ("nprobe_high", dict(nprobe=4), INVALID, b"nprobe=4 outside [1, nlist=3]"),
    ("pairs", dict(Q=1 << 29, nprobe=2), INVALID, b"Q x nprobe too large"),
    ("workspace_null", dict(), WORKSPACE, b"workspace 0 <"),
    ("workspace_short", dict(PLAN_HAVE_WS, ws_bytes=8), WORKSPACE, b"workspace 8 <"),
    ("pointers", dict(PLAN_HAVE_WS), INVALID, b"null pointer"),
    ("pointer_probe", dict(PLAN_HAVE_WS, **dict(PLAN_POINTERS, probe=None)), INVALID,
     b"null pointer"),
    ("pointer_chunk_off", dict(PLAN_HAVE_WS, **dict(PLAN_POINTERS, chunk_off=None)), INVALID,
     b"null pointer"),
]
PLAN_PAIRS = [
    ("sizes_nprobe", dict(Q=-1, nprobe=0), INVALID, b"negative size"),
    ("nprobe_pairs", dict(Q=1 << 29, nprobe=4), INVALID, b"nprobe=4"),
    ("pairs_workspace", dict(Q=1 << 29, nprobe=2), INVALID, b"Q x nprobe too large"),
    ("workspace_pointers", dict(), WORKSPACE, b"workspace"),
]


@pytest.mark.parametrize("args,rc,text", _param(PLAN_SINGLE + PLAN_PAIRS))
def test_plan_each_check_and_the_earlier_of_two(args, rc, text):
    lib = _lib.load()
    assert _plan_call(lib, **args) == rc
    err = lib.irc_last_error()
    assert text in err, err
    assert err.startswith(b"ivf_plan:"), err


def test_plan_workspace_message_and_no_queries():
    lib = _lib.load()
    need = _plan_need(lib)
    assert _plan_call(lib, **dict(PLAN_HAVE_WS, ws_bytes=need - 1)) == WORKSPACE
    assert f"workspace {need - 1} < required {need} bytes".encode() in lib.irc_last_error()
    need0 = _plan_need(lib, Q=0)
    assert need0 > 0
    assert _plan_call(lib, Q=0, **_ws(need0)) == 0  # null arrays: nothing is touched
    assert _plan_call(lib, Q=0) == WORKSPACE  # ... but not before the workspace
    assert _plan_call(lib, Q=0, nprobe=0, **_ws(need0)) == INVALID


def test_plan_span_and_workspace_growth():
    lib = _lib.load()
    span = int(lib.irc_ivf_plan_span())
    assert span >= 64 and span % 64 == 0
    # the bitmap grows with nlist and with every 32 queries; the workgroup sums with the spans
    base = _plan_need(lib, 32, 2, 8)
    assert _plan_need(lib, 32, 2, 8000) > base and _plan_need(lib, 3300, 2, 8) > base
    sizes = [_plan_need(lib, q, 3, 1000) for q in (0, 1, 32, 33, 64, 65, 10 ** 4, 10 ** 6)]
    assert sizes == sorted(sizes) and sizes[0] > 0
    # two words per (list, 32 queries): the bits and the running counts
    assert _plan_need(lib, 64, 2, 1000) >= 2 * 1000 * 2 * 4


# ---------------------------------------------------------------- irc_ivf_search
SEARCH_ARRAYS = ("queries", "docs", "row_id", "list_off", "centroids", "probe", "out",
                 "out_probe")
SEARCH_POINTERS = {name: _ALIGNED for name in SEARCH_ARRAYS}


def _search_need(lib, Q=4, nprobe=2, nlist=3, key_rows=0, k=5):
    return int(lib.irc_ivf_search_workspace(Q, nprobe, nlist, key_rows, k))


def _search_call(lib, Q=4, nprobe=2, N=10, D=128, k=5, nlist=3, key_rows=0, max_list_rows=4,
                 ws=None, ws_bytes=0, _keep=None, **ptrs):
    a = {name: ptrs.get(name) for name in SEARCH_ARRAYS}
    return lib.irc_ivf_search(a["queries"], a["docs"], a["row_id"], a["list_off"], nlist,
                              a["centroids"], a["probe"], Q, nprobe, N, D, k, key_rows,
                              max_list_rows, ws, ws_bytes, a["out"], a["out"], a["out"],
                              a["out_probe"], None)


HAVE_WS = _ws(_search_need(_lib.load()))
SEARCH_SINGLE = [
    ("size_Q", dict(Q=-1), INVALID, b"negative size"),
    ("size_N", dict(N=-1), INVALID, b"negative size"),
    ("size_keys", dict(key_rows=-1), INVALID, b"negative size"),
    ("size_longest", dict(max_list_rows=-1), INVALID, b"negative size"),
    ("k_low", dict(k=0), INVALID, b"k=0"),
    ("k_high", dict(k=1025), INVALID, b"k=1025"),
    ("D", dict(D=100), INVALID, b"unsupported D=100"),
    ("nprobe_low", dict(nprobe=0), INVALID, b"nprobe=0"),
    ("nprobe_high", dict(nprobe=4), INVALID, b"nprobe=4 outside [1, nlist=3]"),
    ("own_probe_limit", dict(nprobe=1025, nlist=2000), INVALID, b"nprobe=1025 above 1024"),
    ("ids", dict(N=1 << 31), INVALID, b"fit int32"),
    ("pairs", dict(Q=1 << 29, nprobe=2), INVALID, b"Q x nprobe too large"),
    ("longest", dict(max_list_rows=11), INVALID, b"max_list_rows=11"),
    ("workspace_null", dict(key_rows=1000), WORKSPACE, b"workspace 0 <"),
    ("workspace_short", dict(HAVE_WS, key_rows=1000, ws_bytes=8), WORKSPACE, b"workspace 8 <"),
    ("pointers", dict(HAVE_WS), INVALID, b"null pointer"),
    ("pointer_row_id", dict(HAVE_WS, **dict(SEARCH_POINTERS, row_id=None)), INVALID,
     b"null pointer"),
    ("no_probe_no_centroids", dict(HAVE_WS, **dict(SEARCH_POINTERS, probe=None, centroids=None)),
     INVALID, b"null pointer"),
    ("alignment_queries", dict(HAVE_WS, **dict(SEARCH_POINTERS, queries=_ALIGNED + 8)), INVALID,
     b"16-byte aligned"),
    ("alignment_docs", dict(HAVE_WS, **dict(SEARCH_POINTERS, docs=_ALIGNED + 2)), INVALID,
     b"16-byte aligned"),
    ("alignment_centroids", dict(HAVE_WS, **dict(SEARCH_POINTERS, probe=None,
                                                 centroids=_ALIGNED + 4)), INVALID,
     b"16-byte aligned"),
]
SEARCH_PAIRS = [
    ("sizes_k", dict(Q=-1, k=0), INVALID, b"negative size"),
    ("k_D", dict(k=0, D=100), INVALID, b"k=0"),
    ("D_nprobe", dict(D=100, nprobe=0), INVALID, b"unsupported D=100"),
    ("nprobe_own_limit", dict(nprobe=2001, nlist=2000), INVALID, b"outside [1, nlist=2000]"),
    ("own_limit_ids", dict(nprobe=1025, nlist=2000, N=1 << 31), INVALID, b"above 1024"),
    ("ids_workspace", dict(N=1 << 31, key_rows=1000), INVALID, b"fit int32"),
    ("pairs_workspace", dict(Q=1 << 29, nprobe=2, key_rows=1000), INVALID,
     b"Q x nprobe too large"),
    ("longest_workspace", dict(max_list_rows=11, key_rows=1000), INVALID, b"max_list_rows=11"),
    ("workspace_pointers", dict(key_rows=1000), WORKSPACE, b"workspace"),
    ("pointers_alignment", dict(HAVE_WS, **dict(SEARCH_POINTERS, row_id=None,
                                                queries=_ALIGNED + 8)), INVALID,
     b"null pointer"),
]


@pytest.mark.parametrize("args,rc,text", _param(SEARCH_SINGLE + SEARCH_PAIRS))
def test_search_each_check_and_the_earlier_of_two(args, rc, text):
    lib = _lib.load()
    assert _search_call(lib, **args) == rc
    err = lib.irc_last_error()
    assert text in err, err
    assert err.startswith(b"ivf_search:"), err


def test_a_callers_probe_may_be_wider_than_the_calls_own():
    # 1025 lists cannot be probed by the call itself, but a caller's probe of them passes that
    # check: the next one that fails reports
    lib = _lib.load()
    assert _search_call(lib, nprobe=1025, nlist=2000, N=1 << 31, probe=_ALIGNED) == INVALID
    assert b"fit int32" in lib.irc_last_error()


def test_search_workspace_message_and_no_queries():
    lib = _lib.load()
    need = _search_need(lib, key_rows=1000)
    assert _search_call(lib, key_rows=1000, **dict(_ws(need), ws_bytes=need - 1)) == WORKSPACE
    assert f"workspace {need - 1} < required {need} bytes".encode() in lib.irc_last_error()
    need0 = _search_need(lib, Q=0)
    assert _search_call(lib, Q=0, **_ws(need0)) == 0  # null arrays: nothing is touched
    assert _search_call(lib, Q=0, key_rows=1000) == WORKSPACE  # ... but not before the workspace
    assert _search_call(lib, Q=0, k=0, **_ws(need0)) == INVALID


def test_search_workspace_grows_with_the_keys_the_lists_and_the_queries():
    lib = _lib.load()
    keys = (0, 1, 31, 32, 33, 1000, 10 ** 9)
    sizes = [_search_need(lib, 7, 3, 50, t, 10) for t in keys]
    assert sizes == sorted(sizes) and len(set(sizes[4:])) == 3 and sizes[0] > 0
    assert all(s >= 8 * t for s, t in zip(sizes, keys))
    by_nlist = [_search_need(lib, 7, 3, n, 1000, 10) for n in (3, 50, 5000, 500000)]
    assert by_nlist == sorted(by_nlist) and len(set(by_nlist)) == 4
    by_q = [_search_need(lib, q, 3, 50, 1000, 10) for q in (1, 32, 33, 1000, 100000)]
    assert by_q == sorted(by_q) and len(set(by_q)) == 5
    # it holds the keys, the plan's scratch and the five plan arrays of the call
    Q, nprobe, nlist = 1000, 3, 50
    plan_arrays = 8 * (Q * nprobe + 1) + 8 * (Q + 1) + 4 * Q * nprobe + 16 * (nlist + 1)
    assert _search_need(lib, Q, nprobe, nlist, 1000, 10) >= \
        int(lib.irc_ivf_topk_workspace(Q, nprobe, 1000, 10)) + plan_arrays + \
        _plan_need(lib, Q, nprobe, nlist) - 256


# ---------------------------------------------------------------- key_bound
def _index_of(lens, D=16, seed=0):
    from irc_amd.retrieval import IVFDenseIndex

    lens = list(lens)
    g = torch.Generator().manual_seed(seed)
    assign = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    assign = assign[torch.randperm(assign.numel(), generator=g)]
    return IVFDenseIndex.from_lists(torch.randn(sum(lens), D, generator=g),
                                    torch.randn(len(lens), D, generator=g), assign)


def test_key_bound_on_hand_written_lengths():
    index = _index_of([4, 4, 4])
    assert [index.key_bound(n) for n in (1, 2, 3)] == [4, 8, 12]
    assert index.max_list_rows == index.key_bound(1) == 4
    # skewed, with empty lists: the longest first whatever their place
    index = _index_of([1, 0, 50, 3, 0, 7])
    assert [index.key_bound(n) for n in range(1, 7)] == [50, 57, 60, 61, 61, 61]
    assert index.max_list_rows == 50
    assert all(isinstance(index.key_bound(n), int) for n in (1, 6))


def test_key_bound_above_the_stored_prefix_is_an_error():
    index = _index_of([4, 4, 4])
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="key_bound"):
            index.key_bound(bad)
    from irc_amd.retrieval import IVFDenseIndex

    # only the 1024 longest lists are kept
    index = _index_of([1 + c % 3 for c in range(1030)], D=4)
    # 343 lists of 3 rows, 343 of 2, and 338 of the 344 of 1
    assert IVFDenseIndex.KEY_BOUND_LISTS == 1024
    assert index.key_bound(1024) == 3 * 343 + 2 * 343 + 338
    with pytest.raises(ValueError, match="key_bound"):
        index.key_bound(1025)


def test_key_bound_survives_save_and_load(tmp_path):
    from irc_amd.retrieval import IVFDenseIndex

    index = _index_of([1, 0, 50, 3, 0, 7])
    index.save(str(tmp_path))
    again, _ = IVFDenseIndex.load(str(tmp_path), device="cpu")
    assert [again.key_bound(n) for n in range(1, 7)] == [50, 57, 60, 61, 61, 61]
    assert again.max_list_rows == 50


def test_key_bound_bounds_the_keys_of_random_probes():
    from irc_amd.retrieval import ivf_plan

    rng = np.random.default_rng(23)
    checked = 0
    for trial in range(20):
        nlist = int(rng.integers(1, 40))
        lens = rng.integers(0, 30, nlist) * (rng.random(nlist) < 0.8)
        if trial % 4 == 0:
            lens[rng.integers(0, nlist)] += 500  # a skewed layout
        if lens.sum() == 0:
            lens[0] = 1
        index = _index_of(lens.tolist(), D=4, seed=trial)
        for _ in range(10):
            nprobe = int(rng.integers(1, nlist + 1))
            Q = int(rng.integers(1, 12))
            probe = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(Q)])
            probe[rng.random(probe.shape) < 0.2] = -1
            total = int(ivf_plan(torch.from_numpy(probe.astype(np.int32)),
                                 index.list_off)["slot_off"][-1])
            assert Q * index.key_bound(nprobe) >= total
            checked += 1
    assert checked == 200
    # the bound is met: every query probing the longest lists
    index = _index_of([1, 0, 50, 3, 0, 7])
    probe = torch.tensor([[2, 5, 3]] * 4, dtype=torch.int32)
    assert int(ivf_plan(probe, index.list_off)["slot_off"][-1]) == 4 * index.key_bound(3)


# ---------------------------------------------------------------- the chunk-size function
def test_query_chunk_is_a_multiple_of_32_that_fits():
    from irc_amd.retrieval import ivf_query_chunk

    def linear(c):
        return 1000 * c + 77

    assert ivf_query_chunk(70, 10 ** 9, linear) == 70  # everything fits: one call
    assert ivf_query_chunk(70, linear(70), linear) == 70
    assert ivf_query_chunk(70, linear(70) - 1, linear) == 64
    assert ivf_query_chunk(70, linear(64) - 1, linear) == 32
    assert ivf_query_chunk(70, 0, linear) == 32  # nothing fits: the least a call is cut to
    assert ivf_query_chunk(20, 0, linear) == 20 and ivf_query_chunk(32, 0, linear) == 32
    assert ivf_query_chunk(0, 0, linear) == 0
    for Q in (33, 64, 65, 1000, 4097):
        for limit in (0, linear(32), linear(33), linear(500), linear(Q) - 1, linear(Q)):
            c = ivf_query_chunk(Q, limit, linear)
            assert c == Q or (c % 32 == 0 and 32 <= c < Q)
            assert c == 32 or linear(c) <= limit
            if c < Q and c + 32 < Q:
                assert linear(c + 32) > limit  # the largest that fits


def test_query_chunk_on_the_librarys_workspace():
    from irc_amd.retrieval import ivf_query_chunk

    lib = _lib.load()
    bound, nprobe, nlist, k = 600, 4, 9, 10

    def need(c):
        return int(lib.irc_ivf_search_workspace(c, nprobe, nlist, c * bound, k))

    assert ivf_query_chunk(70, need(32), need) == 32  # 70 queries run as 32 + 32 + 6
    assert ivf_query_chunk(70, need(64), need) == 64
    assert ivf_query_chunk(70, 1 << 30, need) == 70


# ---------------------------------------------------------------- wrapper validation
def test_the_wrappers_check_shapes_and_dtypes_before_the_library(monkeypatch):
    import irc_amd.retrieval as R

    def boom(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(R._lib, "call", boom)
    monkeypatch.setattr(R._lib, "fn", boom)
    lo = torch.tensor([0, 4, 8, 12])
    pr = torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="probe must be"):
        R.ivf_plan_native(torch.zeros(4, dtype=torch.int32), lo)
    for dtype in (torch.int16, torch.float32, torch.uint8):
        with pytest.raises(ValueError, match="int32 or int64"):
            R.ivf_plan_native(pr.to(dtype), lo)
    with pytest.raises(ValueError, match="list_off must be"):
        R.ivf_plan_native(pr, lo.reshape(2, 2))
    for p in (pr, pr.to(torch.int64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            R.ivf_plan_native(p, lo)

    q, d, cen = torch.zeros(2, 16), torch.zeros(12, 16), torch.zeros(3, 16)
    rid = torch.arange(12, dtype=torch.int32)

    def search(queries=q, docs=d, row_id=rid, **kw):
        kw.setdefault("centroids", cen)
        return R.ivf_search(queries, docs, row_id, lo, 5, 100, 4, **kw)

    with pytest.raises(ValueError, match="dim mismatch"):
        search(queries=torch.zeros(2, 8), nprobe=1)
    with pytest.raises(ValueError, match="dim mismatch"):
        search(queries=torch.zeros(16), nprobe=1)
    with pytest.raises(ValueError, match="exactly one of nprobe and probe"):
        search()
    with pytest.raises(ValueError, match="exactly one of nprobe and probe"):
        search(nprobe=1, probe=pr)
    with pytest.raises(ValueError, match="probe must be"):
        search(probe=torch.zeros(3, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="centroids must be"):
        search(nprobe=1, centroids=None)
    with pytest.raises(ValueError, match="centroids must be"):
        search(nprobe=1, centroids=torch.zeros(4, 16))
    with pytest.raises(ValueError, match="row_id has 11"):
        search(row_id=rid[:11], nprobe=1)
    with pytest.raises(ValueError, match="out must be"):
        search(nprobe=1, out=(torch.zeros(2, 5), torch.zeros(2, 5), torch.zeros(2)))
    with pytest.raises(ValueError, match="out_probe must be"):
        search(nprobe=1, out_probe=torch.zeros(2, 1, dtype=torch.int64))
    # CPU tensors raise through require_hip, as everywhere
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        search(nprobe=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        search(probe=pr, centroids=None)
