"""CPU checks of the dense scan per group (irc_scan_topk_grouped): the entry's host-side
validation and its order, the workspace formula, ``local_group_slice`` against brute force,
the wrappers' argument checks (before any device access), and the signatures and flags that
carry ``group_off`` from main.py to the scan (no compute without a GPU)."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT  # noqa: F401  (import paths)

from irc_amd import _lib, retrieval

_GO = (ctypes.c_int64 * 3)(0, 2, 4)
E4M3 = 2  # irc.h: IRC_RERANK_E4M3
INVALID, WORKSPACE = 1001, 1002


def _call(lib, D=128, k=5, Q=4, N=10, doc_offset=0, group_off=_GO, n_groups=2, flags=0,
          scale=1.0, ws=None, ws_bytes=0, queries=None, docs=None, outs=(None, None, None)):
    return lib.irc_scan_topk_grouped(queries, docs, Q, N, D, k, doc_offset, group_off, n_groups,
                                     flags, scale, ws, ws_bytes, *outs, None)


def _align256(x):
    return (x + 255) // 256 * 256


def test_entry_is_exported_and_bound():
    lib = _lib.load()
    assert lib.irc_abi_version() == 2  # the addition is additive
    assert "irc_scan_topk_grouped" in _lib.SIGNATURES
    assert "irc_scan_topk_grouped_workspace" in _lib.SIGNATURES
    assert _lib.fn("irc_scan_topk_grouped") is not None
    with open(f"{ROOT}/include/irc.h") as f:
        header = f.read()
    assert "int irc_scan_topk_grouped(" in header
    assert "int64_t irc_scan_topk_grouped_workspace(" in header


# one violation of each check, in the order of the interface; every later one is also broken
# in the calls of test_checks_are_reached_in_order
CHECKS = [
    ("negative", dict(N=-1), b"negative size"),
    ("k", dict(k=1025), b"k=1025"),
    ("D", dict(D=100), b"unsupported D=100"),
    ("e4m3_D", dict(D=64, flags=E4M3), b"D % 128 == 0"),
    ("flags", dict(flags=1), b"unsupported flags"),
    ("scale", dict(flags=E4M3, scale=3.0), b"power of two"),
    ("ids", dict(doc_offset=(1 << 31) + 5), b"fit int32"),  # with N = -1 too
    ("Q", dict(Q=(1 << 31) - 1), b"Q too large"),
    ("n_groups", dict(n_groups=(1 << 31) - 1), b"n_groups="),
    ("keys", dict(Q=1 << 20, n_groups=1 << 20), b"Q x n_groups too large"),
    ("tiles", dict(Q=(1 << 31) - 2, N=(1 << 31) - 20), b"Q x N too large"),
]


@pytest.mark.parametrize("name,kw,msg", CHECKS, ids=[c[0] for c in CHECKS])
def test_each_check_reports_itself(name, kw, msg):
    lib = _lib.load()
    assert _call(lib, **kw) == INVALID
    err = lib.irc_last_error()
    assert err.startswith(b"scan_topk_grouped:") and msg in err, err


def _both(a, b):
    """The arguments of a call that breaks check a and the later check b: b's, then a's on
    top (where both set one argument, a's value breaks b too: a larger Q, another bad D),
    the flag bits of both."""
    kw = dict(b)
    kw.update(a)
    kw["flags"] = a.get("flags", 0) | b.get("flags", 0)
    return kw


# every pair but (negative N, tile count): a tile count needs N > 0
PAIRS = [(i, j) for i in range(len(CHECKS)) for j in range(i + 1, len(CHECKS))
         if (CHECKS[i][0], CHECKS[j][0]) != ("negative", "tiles")]


@pytest.mark.parametrize("i,j", PAIRS, ids=[f"{CHECKS[i][0]}-{CHECKS[j][0]}" for i, j in PAIRS])
def test_checks_are_reached_in_order(i, j):
    """A call that breaks two checks reports the earlier one."""
    lib = _lib.load()
    (_, a, msg_a), (_, b, _) = CHECKS[i], CHECKS[j]
    assert _call(lib, **_both(a, b)) == INVALID
    assert msg_a in lib.irc_last_error(), lib.irc_last_error()


def test_workspace_formula_and_the_checks_after_it():
    lib = _lib.load()
    for Q, G in ((1, 1), (4, 2), (256, 25124), (600, 1), (3, 0), (0, 7)):
        assert int(lib.irc_scan_topk_grouped_workspace(Q, G, 100)) == \
            _align256(Q * G * 8) + _align256((Q + 1) * 8)
    # sizes the call rejects have no workspace
    assert int(lib.irc_scan_topk_grouped_workspace(-1, 2, 10)) == 0
    assert int(lib.irc_scan_topk_grouped_workspace(4, -1, 10)) == 0
    assert int(lib.irc_scan_topk_grouped_workspace(1 << 20, 1 << 20, 10)) == 0
    need = int(lib.irc_scan_topk_grouped_workspace(4, 2, 5))
    # every size is fine: the workspace code, before the pointer checks
    assert _call(lib) == WORKSPACE
    assert b"workspace" in lib.irc_last_error()
    buf = (ctypes.c_char * (need + 16))()
    base = ctypes.addressof(buf)
    assert _call(lib, ws=base, ws_bytes=need - 1) == WORKSPACE
    # ... which come after the Q == 0 early return
    assert _call(lib, Q=0, ws=base, ws_bytes=need) == 0
    assert _call(lib, Q=0, ws=base, ws_bytes=need, group_off=None) == 0
    assert _call(lib, ws=base, ws_bytes=need) == INVALID
    assert b"null pointer" in lib.irc_last_error()
    # a workspace that is too small wins over a null pointer, a null pointer over alignment
    arr = (ctypes.c_char * 4096)()
    a16 = (ctypes.addressof(arr) + 15) // 16 * 16
    outs = (a16 + 1024, a16 + 2048, a16 + 3072)
    assert _call(lib, ws=base, ws_bytes=need, queries=a16 + 2, docs=a16, outs=outs,
                 group_off=None) == INVALID
    assert b"null pointer" in lib.irc_last_error()
    assert _call(lib, ws=base, ws_bytes=need, queries=a16 + 2, docs=a16, outs=outs) == INVALID
    assert b"16-byte aligned" in lib.irc_last_error()
    assert _call(lib, ws=base, ws_bytes=need, queries=a16, docs=a16 + 8, outs=outs) == INVALID
    assert b"16-byte aligned" in lib.irc_last_error()


def _brute(go, doc_offset, N):
    n = len(go) - 1
    g_lo = sum(1 for g in range(n) if go[g + 1] <= doc_offset)
    g_hi = sum(1 for g in range(n) if go[g] < doc_offset + N)
    return g_lo, g_hi


def test_local_group_slice_against_brute_force():
    rng = np.random.default_rng(7)
    for _ in range(200):
        n = int(rng.integers(0, 12))
        go = np.sort(rng.integers(0, 40, n + 1))
        if n and rng.random() < 0.5:  # repeated offsets: empty groups
            go[rng.integers(0, n)] = go[rng.integers(0, n + 1)]
            go = np.sort(go)
        doc_offset, N = int(rng.integers(0, 45)), int(rng.integers(0, 20))
        got = retrieval.local_group_slice(torch.from_numpy(go.astype(np.int64)), doc_offset, N)
        assert got == _brute(go.tolist(), doc_offset, N), (go, doc_offset, N)
        assert all(isinstance(x, int) for x in got)


def test_local_group_slice_on_named_cases():
    go = torch.tensor([10, 10, 13, 13, 13, 20, 50, 50])  # groups: {} {10-12} {} {} {13-19} {20-49} {}
    cases = {
        "before all groups": ((0, 10), (0, 0)),
        "ends inside the first rows": ((5, 6), (0, 2)),
        "after all groups": ((50, 10), (7, 7)),
        "strictly inside one group": ((25, 10), (5, 6)),
        "the whole range": ((0, 100), (0, 7)),
        "cut at a group's first row": ((13, 7), (4, 5)),  # the empty groups at 13 end before it
        "an empty shard inside a group": ((15, 0), (4, 5)),
    }
    for name, ((doc_offset, N), want) in cases.items():
        got = retrieval.local_group_slice(go, doc_offset, N)
        assert got == want, name
        assert got == _brute(go.tolist(), doc_offset, N), name
    g_lo, g_hi = retrieval.local_group_slice(go, 25, 10)
    assert go[g_lo:g_hi + 1].tolist() == [20, 50]  # the one group the shard lies in
    g_lo, g_hi = retrieval.local_group_slice(go, 50, 10)
    assert g_hi <= g_lo  # empty slice


def _cpu_args(dtype):
    return torch.zeros(2, 128, dtype=dtype), torch.zeros(4, 128, dtype=dtype), 2


BAD_GROUP_OFF = [(torch.zeros(3, dtype=torch.int32), TypeError),
                 (torch.zeros(3, dtype=torch.float32), TypeError),
                 ([0, 2, 4], TypeError),
                 (None, TypeError),
                 (torch.zeros((2, 2), dtype=torch.int64), ValueError),
                 (torch.zeros((), dtype=torch.int64), ValueError),
                 (torch.zeros(0, dtype=torch.int64), ValueError),
                 (torch.zeros(3, dtype=torch.int64, device="meta"), ValueError)]


def _cpu_index(dtype="bf16", D=128):
    idx = retrieval.ShardedDenseIndex.__new__(retrieval.ShardedDenseIndex)
    idx.dtype, idx.group, idx.doc_offset, idx.fp8_scale = dtype, None, 0, 16.0
    idx.docs = torch.zeros(4, D, dtype=torch.uint8 if dtype == "fp8" else torch.bfloat16)
    return idx


@pytest.mark.parametrize("bad,exc", BAD_GROUP_OFF)
def test_wrappers_check_group_off_before_the_library(monkeypatch, bad, exc):
    def boom(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "fn", boom)
    q, d, k = _cpu_args(torch.bfloat16)
    with pytest.raises(exc, match="group_off"):
        retrieval.scan_topk_grouped(q, d, k, bad)
    q8, d8, _ = _cpu_args(torch.uint8)
    with pytest.raises(exc, match="group_off"):
        retrieval.scan_topk_grouped_fp8(q8, d8, k, bad)
    if bad is not None:  # search(group_off=None) is the ungrouped search
        with pytest.raises(exc, match="group_off"):
            _cpu_index().search(q, k, group_off=bad)


def test_a_good_group_off_reaches_the_device_check(monkeypatch):
    go = torch.tensor([0, 2, 4])
    q, d, k = _cpu_args(torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.scan_topk_grouped(q, d, k, go)
    q8, d8, _ = _cpu_args(torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.scan_topk_grouped_fp8(q8, d8, k, go)
    with pytest.raises(TypeError, match="e4m3"):
        retrieval.scan_topk_grouped_fp8(q, d, k, go)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _cpu_index().search(q, k, group_off=go)


def test_fp8_index_needs_d_128_before_any_device_work(monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "fn", boom)
    monkeypatch.setattr(retrieval, "quantize_fp8", boom)
    go = torch.tensor([0, 2, 4])
    with pytest.raises(ValueError, match="D % 128"):
        _cpu_index("fp8", 64).search(torch.zeros(2, 64), 2, group_off=go)
    with pytest.raises(ValueError, match="dim mismatch"):
        _cpu_index().search(torch.zeros(2, 64), 2, group_off=go)
    with pytest.raises(ValueError, match="k=0"):
        _cpu_index().search(torch.zeros(2, 128), 0, group_off=go)


def test_signatures_and_flags():
    import main as entry

    sig = inspect.signature(retrieval.ShardedDenseIndex.search)
    assert "group_off=None" in str(sig)
    assert list(sig.parameters)[1:] == ["queries", "k", "equal_counts", "ws_tag", "group_off"]
    assert "group_off" not in inspect.signature(retrieval.ShardedDenseIndex.search_many).parameters
    for f in (retrieval.scan_topk_grouped, retrieval.scan_topk_grouped_fp8):
        p = inspect.signature(f).parameters
        assert p["group_off"].default is inspect.Parameter.empty  # required
        assert p["doc_offset"].default == 0 and p["ws_tag"].default == "scan_group"
        assert p["max_workspace_bytes"].default == 1 << 30
    assert inspect.signature(retrieval.scan_topk_grouped_fp8).parameters["score_scale"].default == 1.0
    assert entry.get_args(["--rerank-unit", "page", "--retrieval", "dense"]).rerank_unit == "page"
    assert entry.get_args(["--retrieval", "dense"]).rerank_unit == "line"
    assert "--rerank-unit line|page" in entry.__doc__
