"""CPU checks of the cluster-pruned search over e4m3 lists: the ORDER of irc_ivf_topk_fp8's and
irc_ivf_search_fp8's host-side argument checks (they read no memory, so pointers are null or
plain host buffers), the scale checks, the workspace function, the wrappers' own checks with no
device and the ``--ivf-list-dtype`` flag (tests/test_ivf_fp8_gpu.py covers the kernel).

The order of the native checks:

  irc_ivf_topk_fp8    sizes, k, D, nprobe, score_scale, int32 ids (N), Q x nprobe,
                      max_list_rows, workspace, Q == 0 return, null pointers, alignment
  irc_ivf_search_fp8  sizes, k, D, nprobe, the probe's own limit (1024 lists, when the call
                      probes itself), score_scale, query_scale, int32 ids (N), Q x nprobe,
                      max_list_rows, workspace, Q == 0 return, null pointers, alignment"""
import ctypes

import pytest
import torch

from conftest import PKG, ROOT  # noqa: F401  (import paths)

from irc_amd import _lib

INVALID, WORKSPACE = 1001, 1002
NAN, INF = float("nan"), float("inf")

_BUF = ctypes.create_string_buffer(4096 + 16)
_ALIGNED = (ctypes.addressof(_BUF) + 15) & ~15  # a 16-byte aligned host address


def _ws(nbytes):
    buf = ctypes.create_string_buffer(max(int(nbytes), 1))
    return dict(ws=ctypes.addressof(buf), ws_bytes=int(nbytes), _keep=buf)


def _param(cases):
    return [pytest.param(*c[1:], id=c[0]) for c in cases]


def test_the_new_symbols_are_declared_and_bound():
    # tests/test_abi.py checks every declared symbol's export; these are declared
    with open(f"{ROOT}/include/irc.h") as f:
        header = f.read()
    lib = _lib.load()
    for name in ("irc_ivf_topk_fp8", "irc_ivf_search_fp8_workspace", "irc_ivf_search_fp8"):
        assert f" {name}(" in header
        assert getattr(lib, name) is not None


# ---------------------------------------------------------------- irc_ivf_topk_fp8
TOPK_ARRAYS = ("queries", "docs", "row_id", "list_off", "probe", "slot_off", "cand_off",
               "pair_order", "seg_off", "chunk_off", "out")
TOPK_POINTERS = {name: _ALIGNED for name in TOPK_ARRAYS}


def _topk_call(lib, Q=4, nprobe=2, N=10, D=128, k=5, nlist=3, total_rows=0, max_list_rows=4,
               score_scale=1.0 / 256, ws=None, ws_bytes=0, _keep=None, **ptrs):
    a = {name: ptrs.get(name) for name in TOPK_ARRAYS}
    return lib.irc_ivf_topk_fp8(a["queries"], a["docs"], a["row_id"], a["list_off"], nlist,
                                a["probe"], a["slot_off"], a["cand_off"], a["pair_order"],
                                a["seg_off"], a["chunk_off"], Q, nprobe, N, D, k, total_rows,
                                max_list_rows, score_scale, ws, ws_bytes, a["out"], a["out"],
                                a["out"], None)


TOPK_HAVE_WS = _ws(4096)
# (id, arguments, return code, text of the check that reports)
TOPK_SINGLE = [
    ("size_Q", dict(Q=-1), INVALID, b"negative size"),
    ("size_N", dict(N=-1), INVALID, b"negative size"),
    ("size_total", dict(total_rows=-1), INVALID, b"negative size"),
    ("size_longest", dict(max_list_rows=-1), INVALID, b"negative size"),
    ("k_low", dict(k=0), INVALID, b"k=0"),
    ("k_high", dict(k=1025), INVALID, b"k=1025"),
    ("D", dict(D=100), INVALID, b"unsupported D=100"),
    ("nprobe_low", dict(nprobe=0), INVALID, b"nprobe=0"),
    ("nprobe_high", dict(nprobe=4), INVALID, b"nprobe=4 outside [1, nlist=3]"),
    ("scale_not_pow2", dict(score_scale=3.0), INVALID, b"score_scale must be a power of two"),
    ("scale_zero", dict(score_scale=0.0), INVALID, b"score_scale must be a power of two"),
    ("scale_negative", dict(score_scale=-0.25), INVALID, b"score_scale must be a power of two"),
    ("scale_nan", dict(score_scale=NAN), INVALID, b"score_scale must be a power of two"),
    ("scale_inf", dict(score_scale=INF), INVALID, b"score_scale must be a power of two"),
    ("ids", dict(N=1 << 31), INVALID, b"fit int32"),
    ("pairs", dict(Q=1 << 29, nprobe=2), INVALID, b"Q x nprobe too large"),
    ("longest", dict(max_list_rows=11), INVALID, b"max_list_rows=11"),
    ("workspace_null", dict(total_rows=1000), WORKSPACE, b"workspace 0 <"),
    ("workspace_short", dict(TOPK_HAVE_WS, total_rows=1000, ws_bytes=8), WORKSPACE,
     b"workspace 8 <"),
    ("pointers", dict(TOPK_HAVE_WS), INVALID, b"null pointer"),
    ("pointer_probe", dict(TOPK_HAVE_WS, **dict(TOPK_POINTERS, probe=None)), INVALID,
     b"null pointer"),
    ("alignment_queries", dict(TOPK_HAVE_WS, **dict(TOPK_POINTERS, queries=_ALIGNED + 8)),
     INVALID, b"16-byte aligned"),
    ("alignment_docs", dict(TOPK_HAVE_WS, **dict(TOPK_POINTERS, docs=_ALIGNED + 2)), INVALID,
     b"16-byte aligned"),
]
# two checks broken at once: the earlier one reports
TOPK_PAIRS = [
    ("sizes_k", dict(Q=-1, k=0), INVALID, b"negative size"),
    ("k_D", dict(k=0, D=100), INVALID, b"k=0"),
    ("D_nprobe", dict(D=100, nprobe=0), INVALID, b"unsupported D=100"),
    ("nprobe_scale", dict(nprobe=9, score_scale=3.0), INVALID, b"nprobe=9"),
    ("scale_ids", dict(score_scale=3.0, N=1 << 31), INVALID, b"score_scale"),
    ("ids_workspace", dict(N=1 << 31, total_rows=1000), INVALID, b"fit int32"),
    ("pairs_workspace", dict(Q=1 << 29, nprobe=2, total_rows=1000), INVALID,
     b"Q x nprobe too large"),
    ("longest_workspace", dict(max_list_rows=11, total_rows=1000), INVALID, b"max_list_rows=11"),
    ("workspace_pointers", dict(total_rows=1000), WORKSPACE, b"workspace"),
    ("pointers_alignment", dict(TOPK_HAVE_WS, **dict(TOPK_POINTERS, row_id=None,
                                                     queries=_ALIGNED + 8)), INVALID,
     b"null pointer"),
]


@pytest.mark.parametrize("args,rc,text", _param(TOPK_SINGLE + TOPK_PAIRS))
def test_topk_each_check_and_the_earlier_of_two(args, rc, text):
    lib = _lib.load()
    assert _topk_call(lib, **args) == rc
    err = lib.irc_last_error()
    assert text in err, err
    assert err.startswith(b"ivf_topk_fp8:"), err


def test_topk_workspace_message_and_no_queries():
    lib = _lib.load()
    need = int(lib.irc_ivf_topk_workspace(4, 2, 1000, 5))  # the keys do not know the element
    assert _topk_call(lib, total_rows=1000, **dict(_ws(need), ws_bytes=need - 1)) == WORKSPACE
    assert f"workspace {need - 1} < required {need} bytes".encode() in lib.irc_last_error()
    assert _topk_call(lib, Q=0, **TOPK_HAVE_WS) == 0  # null arrays: nothing is touched
    assert _topk_call(lib, Q=0, total_rows=1000) == WORKSPACE  # ... but not before the workspace
    assert _topk_call(lib, Q=0, score_scale=3.0, **TOPK_HAVE_WS) == INVALID
    for ok in (1.0, 2.0 ** -8, 2.0 ** 20, 2.0 ** -100):
        assert _topk_call(lib, Q=0, score_scale=ok, **TOPK_HAVE_WS) == 0


# ---------------------------------------------------------------- irc_ivf_search_fp8
SEARCH_ARRAYS = ("queries", "docs", "row_id", "list_off", "centroids", "probe", "out",
                 "out_probe")
SEARCH_POINTERS = {name: _ALIGNED for name in SEARCH_ARRAYS}


def _search_need(lib, Q=4, nprobe=2, nlist=3, key_rows=0, k=5):
    return int(lib.irc_ivf_search_fp8_workspace(Q, nprobe, nlist, key_rows, k))


def _bf16_need(lib, Q=4, nprobe=2, nlist=3, key_rows=0, k=5):
    return int(lib.irc_ivf_search_workspace(Q, nprobe, nlist, key_rows, k))


def _search_call(lib, Q=4, nprobe=2, N=10, D=128, k=5, nlist=3, key_rows=0, max_list_rows=4,
                 query_scale=16.0, score_scale=1.0 / 256, ws=None, ws_bytes=0, _keep=None,
                 **ptrs):
    a = {name: ptrs.get(name) for name in SEARCH_ARRAYS}
    return lib.irc_ivf_search_fp8(a["queries"], a["docs"], a["row_id"], a["list_off"], nlist,
                                  a["centroids"], a["probe"], Q, nprobe, N, D, k, key_rows,
                                  max_list_rows, query_scale, score_scale, ws, ws_bytes,
                                  a["out"], a["out"], a["out"], a["out_probe"], None)


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
    ("score_scale_not_pow2", dict(score_scale=0.3), INVALID,
     b"score_scale must be a power of two"),
    ("score_scale_zero", dict(score_scale=0.0), INVALID, b"score_scale must be a power of two"),
    ("query_scale_zero", dict(query_scale=0.0), INVALID, b"query_scale"),
    ("query_scale_negative", dict(query_scale=-16.0), INVALID, b"query_scale"),
    ("query_scale_nan", dict(query_scale=NAN), INVALID, b"query_scale"),
    ("query_scale_inf", dict(query_scale=INF), INVALID, b"query_scale"),
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
    ("own_limit_score_scale", dict(nprobe=1025, nlist=2000, score_scale=3.0), INVALID,
     b"above 1024"),
    ("score_scale_query_scale", dict(score_scale=3.0, query_scale=0.0), INVALID,
     b"score_scale"),
    ("query_scale_ids", dict(query_scale=NAN, N=1 << 31), INVALID, b"query_scale"),
    ("score_scale_ids", dict(score_scale=3.0, N=1 << 31), INVALID, b"score_scale"),
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
    assert err.startswith(b"ivf_search_fp8:"), err


def test_a_callers_probe_may_be_wider_than_the_calls_own():
    lib = _lib.load()
    assert _search_call(lib, nprobe=1025, nlist=2000, score_scale=3.0, probe=_ALIGNED) == INVALID
    assert b"score_scale" in lib.irc_last_error()


def test_search_workspace_message_and_no_queries():
    lib = _lib.load()
    need = _search_need(lib, key_rows=1000)
    assert _search_call(lib, key_rows=1000, **dict(_ws(need), ws_bytes=need - 1)) == WORKSPACE
    assert f"workspace {need - 1} < required {need} bytes".encode() in lib.irc_last_error()
    # the bf16 entry's workspace is too small for this one
    short = _bf16_need(lib, key_rows=1000)
    assert short < need
    assert _search_call(lib, key_rows=1000, **_ws(short)) == WORKSPACE
    need0 = _search_need(lib, Q=0)
    assert _search_call(lib, Q=0, **_ws(need0)) == 0  # null arrays: nothing is touched
    assert _search_call(lib, Q=0, key_rows=1000) == WORKSPACE  # ... but not before the workspace
    assert _search_call(lib, Q=0, query_scale=0.0, **_ws(need0)) == INVALID
    # any finite positive query scale passes: only the descale has to be a power of two
    assert _search_call(lib, Q=0, query_scale=12.5, **_ws(need0)) == 0


def test_search_workspace_is_the_bf16_one_plus_the_codes():
    lib = _lib.load()
    for Q in (0, 1, 31, 32, 33, 1000, 100000):
        for nprobe, nlist, key_rows in ((1, 1, 0), (3, 50, 1000), (8, 5000, 10 ** 7)):
            got = _search_need(lib, Q, nprobe, nlist, key_rows, 10)
            # the widest row's codes per query: D does not enter
            assert got >= _bf16_need(lib, Q, nprobe, nlist, key_rows, 10) + Q * 1024
    by_q = [_search_need(lib, q, 3, 50, 1000, 10) for q in (0, 1, 32, 33, 1000, 100000)]
    assert by_q == sorted(by_q) and len(set(by_q)) == len(by_q) and by_q[0] > 0
    keys = (0, 1, 31, 32, 33, 1000, 10 ** 9)
    by_keys = [_search_need(lib, 7, 3, 50, t, 10) for t in keys]
    assert by_keys == sorted(by_keys) and all(s >= 8 * t for s, t in zip(by_keys, keys))
    # (Q, nprobe, nlist, key_rows, k): no D among the arguments
    assert lib.irc_ivf_search_fp8_workspace.argtypes is None or \
        len(lib.irc_ivf_search_fp8_workspace.argtypes) == 5


# ---------------------------------------------------------------- wrapper validation
def _cpu_index(N=12, D=16, nlist=3):
    from irc_amd.retrieval import IVFDenseIndex

    g = torch.Generator().manual_seed(0)
    return IVFDenseIndex.from_lists(torch.randn(N, D, generator=g),
                                    torch.randn(nlist, D, generator=g), torch.arange(N) % nlist,
                                    doc_offset=5)


def test_the_wrappers_refuse_other_dtypes_before_the_library(monkeypatch):
    import irc_amd.retrieval as R

    def boom(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(R._lib, "call", boom)
    monkeypatch.setattr(R._lib, "fn", boom)
    lo = torch.tensor([0, 4, 8, 12])
    pr = torch.zeros(2, 1, dtype=torch.int32)
    rid = torch.arange(12, dtype=torch.int32)
    q8, d8 = torch.zeros(2, 16, dtype=torch.uint8), torch.zeros(12, 16, dtype=torch.uint8)
    for bad in (torch.float32, torch.bfloat16, torch.int8):
        with pytest.raises(TypeError, match="e4m3 bytes"):
            R.ivf_topk_fp8(q8.to(bad), d8, rid, lo, pr, 5, 4)
        with pytest.raises(TypeError, match="e4m3 bytes"):
            R.ivf_topk_fp8(q8, d8.to(bad), rid, lo, pr, 5, 4)
        with pytest.raises(TypeError, match="e4m3 bytes"):
            R.ivf_search_fp8(torch.zeros(2, 16), d8.to(bad), rid, lo, 5, 100, 4, probe=pr)
    # then ivf_search's own checks, in its order, and the device
    q, cen = torch.zeros(2, 16), torch.zeros(3, 16)
    with pytest.raises(ValueError, match="dim mismatch"):
        R.ivf_search_fp8(torch.zeros(2, 8), d8, rid, lo, 5, 100, 4, probe=pr)
    with pytest.raises(ValueError, match="exactly one of nprobe and probe"):
        R.ivf_search_fp8(q, d8, rid, lo, 5, 100, 4, centroids=cen)
    with pytest.raises(ValueError, match="centroids must be"):
        R.ivf_search_fp8(q, d8, rid, lo, 5, 100, 4, nprobe=1)
    with pytest.raises(ValueError, match="row_id has 11"):
        R.ivf_search_fp8(q, d8, rid[:11], lo, 5, 100, 4, probe=pr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.ivf_search_fp8(q, d8, rid, lo, 5, 100, 4, probe=pr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.ivf_search_fp8(q, d8, rid, lo, 5, 100, 4, centroids=cen, nprobe=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        R.ivf_topk_fp8(q8, d8, rid, lo, pr, 5, 4, score_scale=1 / 256)


def test_to_fp8_and_the_fp8_search_have_no_cpu_fallback():
    from irc_amd.retrieval import FP8_SCALE, IVFDenseIndex

    index = _cpu_index()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.to_fp8()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        IVFDenseIndex.train(torch.zeros(12, 16), 3, dtype="fp8")
    with pytest.raises(ValueError, match="dtype must be"):
        IVFDenseIndex.train(torch.zeros(12, 16), 3, dtype="int8")
    # an fp8 index put together by hand (what to_fp8 returns on a device): the search reaches
    # the fp8 entry's wrapper, which has no CPU form either
    other = IVFDenseIndex.__new__(IVFDenseIndex)
    other.__dict__.update(index.__dict__)
    other.dtype, other.fp8_scale = "fp8", float(FP8_SCALE)
    other.docs = torch.zeros(index.docs.shape, dtype=torch.uint8)
    q = torch.zeros(2, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        other.search(q, 5, nprobe=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        other.search(q, 5, probe=torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="already fp8"):
        other.to_fp8()
    # the pinned refusals stay (tests/test_ivf_cpu.py::test_what_is_not_built_says_so)
    with pytest.raises(NotImplementedError, match="permuted"):
        other.search(q, 5, nprobe=1, group_off=torch.tensor([0, 12]))
    with pytest.raises(NotImplementedError, match="follow-up"):
        other.search_many([q], 5)


def test_a_saved_e4m3_shard_loads(tmp_path):
    from irc_amd.retrieval import IVFDenseIndex

    index = _cpu_index()
    other = IVFDenseIndex.__new__(IVFDenseIndex)
    other.__dict__.update(index.__dict__)
    other.dtype, other.fp8_scale = "fp8", 8.0
    other.docs = (torch.arange(12 * 16) % 251).to(torch.uint8).reshape(12, 16)
    other.save(str(tmp_path), rank=1)
    again, _ = IVFDenseIndex.load(str(tmp_path), rank=1, device="cpu")
    assert again.dtype == "fp8" and again.fp8_scale == 8.0
    assert again.docs.dtype == torch.uint8 and torch.equal(again.docs, other.docs)
    assert torch.equal(again.row_id, index.row_id) and torch.equal(again.list_off, index.list_off)
    assert torch.equal(again.centroids, index.centroids) and again.centroids.dtype == torch.bfloat16
    assert again.max_list_rows == index.max_list_rows == again.key_bound(1)


# ---------------------------------------------------------------- the entry point's flag
def test_main_ivf_list_dtype_flag(capsys):
    import main as entry

    base = ["--data", "fever", "--retrieval", "dense"]
    ivf = base + ["--index", "ivf", "--nlist", "16", "--nprobe", "4"]
    assert entry.get_args([]).ivf_list_dtype == "bf16"
    assert entry.get_args(ivf).ivf_list_dtype == "bf16"
    assert entry.get_args(ivf + ["--ivf-list-dtype", "fp8"]).ivf_list_dtype == "fp8"
    assert entry.get_args(ivf + ["--ivf-list-dtype", "bf16"]).ivf_list_dtype == "bf16"
    assert entry.get_args(base + ["--ivf-list-dtype", "bf16"]).index == "flat"  # the default
    for bad in (base + ["--ivf-list-dtype", "fp8"],
                base + ["--index", "flat", "--ivf-list-dtype", "fp8"],
                ["--ivf-list-dtype", "fp8"]):
        with pytest.raises(SystemExit):
            entry.get_args(bad)
        assert "--index ivf" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        entry.get_args(ivf + ["--ivf-list-dtype", "int8"])
    assert "invalid choice" in capsys.readouterr().err
    # the flat index's dtype flag still does not reach the lists
    with pytest.raises(SystemExit):
        entry.get_args(ivf + ["--index-dtype", "fp8", "--ivf-list-dtype", "fp8"])
    assert "bf16" in capsys.readouterr().err
    assert "--ivf-list-dtype" in entry.__doc__
