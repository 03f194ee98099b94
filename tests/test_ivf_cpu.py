"""CPU checks of the cluster-pruned search: the list layout and the plan of a search on
hand-written cases (pure torch, CPU tensors); the ORDER of irc_ivf_topk's host-side argument
checks (they read no memory, so pointers are null or plain host buffers); the wrapper's own
checks with no device; and the collective ``IVFDenseIndex.search`` in two gloo ranks with the
device calls replaced by the numpy reference (tests/test_ivf_gpu.py covers the kernel).

The order of the native checks:

  sizes, k, D, nprobe, int32 ids (N), Q x nprobe, max_list_rows, workspace, Q == 0 return,
  null pointers, alignment"""
import ctypes
import datetime
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT  # noqa: F401  (import paths)
from oracle import irc_oracle as O

from irc_amd import _lib

INVALID, WORKSPACE = 1001, 1002
WORLD = 2


# ---------------------------------------------------------------- ivf_layout
def test_layout_is_a_stable_sort_with_empty_lists():
    from irc_amd.retrieval import ivf_layout

    # lists 0, 3 and 6 empty: first, middle and last
    assign = torch.tensor([4, 1, 5, 1, 2, 4, 1, 5, 2])
    order, list_off = ivf_layout(assign, 7)
    assert order.dtype == torch.int64 and list_off.dtype == torch.int64
    assert order.tolist() == [1, 3, 6, 4, 8, 0, 5, 2, 7]  # ids ascend inside a list
    assert list_off.tolist() == [0, 0, 3, 5, 5, 7, 9, 9]
    order, list_off = ivf_layout(assign.to(torch.int32), 7)  # any integer dtype
    assert list_off.tolist() == [0, 0, 3, 5, 5, 7, 9, 9]


def test_layout_of_no_rows():
    from irc_amd.retrieval import ivf_layout

    order, list_off = ivf_layout(torch.zeros(0, dtype=torch.int64), 3)
    assert order.numel() == 0 and list_off.tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------- ivf_plan
def _plan(probe, list_off):
    from irc_amd.retrieval import ivf_plan

    p = ivf_plan(torch.tensor(probe, dtype=torch.int32), torch.tensor(list_off))
    assert p["slot_off"].dtype == p["cand_off"].dtype == p["seg_off"].dtype == \
        p["chunk_off"].dtype == torch.int64 and p["pair_order"].dtype == torch.int32
    return {k: v.tolist() for k, v in p.items()}


def test_plan_on_a_hand_written_probe():
    # lists of 3, 0, 5, 2 rows; list 3 is probed by nobody, list 1 (empty) by query 0
    list_off = [0, 3, 3, 8, 10]
    probe = [[2, 1], [-1, 0], [0, 2], [-1, -1]]
    p = _plan(probe, list_off)
    # pairs 0..7 = (q0: 2, 1), (q1: -1, 0), (q2: 0, 2), (q3: -1, -1), of 5, 0, 0, 3, 3, 5, 0, 0
    # rows
    assert p["slot_off"] == [0, 5, 5, 5, 8, 11, 16, 16, 16]
    assert p["cand_off"] == p["slot_off"][::2] == [0, 5, 8, 16, 16]
    assert p["seg_off"] == [0, 2, 3, 5, 5]
    n_valid = p["seg_off"][-1]
    # stable by list: list 0 <- pairs 3, 4; list 1 <- pair 1; list 2 <- pairs 0, 5
    assert p["pair_order"][:n_valid] == [3, 4, 1, 0, 5]
    assert sorted(p["pair_order"][n_valid:]) == [2, 6, 7]  # the -1 pairs, never read
    assert p["chunk_off"] == [0, 1, 2, 3, 3]


def test_plan_cuts_33_pairs_of_one_list_into_two_chunks():
    from irc_amd.retrieval import IVF_CHUNK

    assert IVF_CHUNK == 32
    list_off = [0, 4, 4, 10]
    # 33 queries probe list 2 (and list 0 second); one more probes list 0 only
    probe = [[2, 0]] * 33 + [[0, -1]]
    p = _plan(probe, list_off)
    assert p["seg_off"] == [0, 34, 34, 67]
    assert p["chunk_off"] == [0, 2, 2, 4]  # ceil(34 / 32), none, ceil(33 / 32)
    assert p["pair_order"][:34] == [2 * r + 1 for r in range(33)] + [66]
    assert p["pair_order"][34:67] == [2 * r for r in range(33)]
    assert p["cand_off"] == p["slot_off"][::2]
    assert p["slot_off"][-1] == 33 * 10 + 4
    # the chunk bound of the launch: Q nprobe / 32 + min(nlist, Q nprobe)
    assert p["chunk_off"][-1] <= 68 // 32 + min(3, 68)


def test_plan_ignores_ids_that_name_no_list():
    p = _plan([[5, 0]], [0, 2, 3])
    assert p["slot_off"] == [0, 0, 2] and p["seg_off"] == [0, 1, 1] and p["pair_order"][0] == 1


# ---------------------------------------------------------------- host validation
_BUF = ctypes.create_string_buffer(4096 + 16)
_ALIGNED = (ctypes.addressof(_BUF) + 15) & ~15  # a 16-byte aligned host address
_WS = ctypes.create_string_buffer(4096)
HAVE_WS = dict(ws=ctypes.addressof(_WS), ws_bytes=4096)
ARRAYS = ("queries", "docs", "row_id", "list_off", "probe", "slot_off", "cand_off", "pair_order",
          "seg_off", "chunk_off", "out")
ALL_POINTERS = {name: _ALIGNED for name in ARRAYS}


def _call(lib, Q=4, nprobe=2, N=10, D=128, k=5, nlist=3, total_rows=0, max_list_rows=4, ws=None,
          ws_bytes=0, **ptrs):
    a = {name: ptrs.get(name) for name in ARRAYS}
    return lib.irc_ivf_topk(a["queries"], a["docs"], a["row_id"], a["list_off"], nlist,
                            a["probe"], a["slot_off"], a["cand_off"], a["pair_order"],
                            a["seg_off"], a["chunk_off"], Q, nprobe, N, D, k, total_rows,
                            max_list_rows, ws, ws_bytes, a["out"], a["out"], a["out"], None)


# (id, arguments, return code, text of the check that reports)
SINGLE = [
    ("size_Q", dict(Q=-1), INVALID, b"negative size"),
    ("size_N", dict(N=-1), INVALID, b"negative size"),
    ("size_total", dict(total_rows=-1), INVALID, b"negative size"),
    ("size_longest", dict(max_list_rows=-1), INVALID, b"negative size"),
    ("k_low", dict(k=0), INVALID, b"k=0"),
    ("k_high", dict(k=1025), INVALID, b"k=1025"),
    ("D", dict(D=100), INVALID, b"unsupported D=100"),
    ("nprobe_low", dict(nprobe=0), INVALID, b"nprobe=0"),
    ("nprobe_high", dict(nprobe=4), INVALID, b"nprobe=4 outside [1, nlist=3]"),
    ("ids", dict(N=1 << 31), INVALID, b"fit int32"),
    ("workspace_null", dict(total_rows=1000), WORKSPACE, b"workspace 0 <"),
    ("workspace_short", dict(total_rows=1000, **dict(HAVE_WS, ws_bytes=8)), WORKSPACE,
     b"workspace 8 <"),
    ("pointers", dict(**HAVE_WS), INVALID, b"null pointer"),
    ("pointer_probe", dict(**HAVE_WS, **dict(ALL_POINTERS, probe=None)), INVALID,
     b"null pointer"),
    ("alignment_queries", dict(**HAVE_WS, **dict(ALL_POINTERS, queries=_ALIGNED + 8)), INVALID,
     b"16-byte aligned"),
    ("alignment_docs", dict(**HAVE_WS, **dict(ALL_POINTERS, docs=_ALIGNED + 2)), INVALID,
     b"16-byte aligned"),
]
# two checks broken at once: the earlier one reports
PAIRS = [
    ("sizes_k", dict(Q=-1, k=0), INVALID, b"negative size"),
    ("k_D", dict(k=0, D=100), INVALID, b"k=0"),
    ("D_nprobe", dict(D=100, nprobe=0), INVALID, b"unsupported D=100"),
    ("nprobe_ids", dict(nprobe=9, N=1 << 31), INVALID, b"nprobe=9"),
    ("ids_workspace", dict(N=1 << 31, total_rows=1000), INVALID, b"fit int32"),
    ("pairs_workspace", dict(Q=1 << 29, nprobe=2, total_rows=1000), INVALID,
     b"Q x nprobe too large"),
    ("longest_workspace", dict(max_list_rows=11, total_rows=1000), INVALID, b"max_list_rows=11"),
    ("workspace_pointers", dict(total_rows=1000), WORKSPACE, b"workspace"),
    ("pointers_alignment", dict(**HAVE_WS, **dict(ALL_POINTERS, row_id=None,
                                                  queries=_ALIGNED + 8)), INVALID,
     b"null pointer"),
]


@pytest.mark.parametrize("args,rc,text", [pytest.param(*c[1:], id=c[0]) for c in SINGLE + PAIRS])
def test_each_check_and_the_earlier_of_two(args, rc, text):
    lib = _lib.load()
    assert _call(lib, **args) == rc
    err = lib.irc_last_error()
    assert text in err, err
    assert err.startswith(b"ivf_topk:"), err


def test_the_workspace_message_carries_both_sizes():
    lib = _lib.load()
    need = int(lib.irc_ivf_topk_workspace(4, 2, 1000, 5))
    assert need >= 1000 * 8
    assert _call(lib, total_rows=1000, **dict(HAVE_WS, ws_bytes=need - 1)) == WORKSPACE
    assert f"workspace {need - 1} < required {need} bytes".encode() in lib.irc_last_error()


def test_no_queries_is_ok_after_the_checks():
    lib = _lib.load()
    assert _call(lib, Q=0, **HAVE_WS) == 0  # null arrays: nothing is touched
    assert _call(lib, Q=0, total_rows=1000) == WORKSPACE  # ... but not before the workspace
    assert _call(lib, Q=0, k=0, **HAVE_WS) == INVALID


def test_the_workspace_grows_with_the_rows():
    lib = _lib.load()
    totals = (0, 1, 31, 32, 33, 1000, 10 ** 9)
    sizes = [int(lib.irc_ivf_topk_workspace(7, 3, t, 10)) for t in totals]
    assert sizes == sorted(sizes) and sizes[0] > 0
    assert all(s >= 8 * t for s, t in zip(sizes, totals))
    # Q, nprobe and k do not enter: a key per (pair, row)
    assert int(lib.irc_ivf_topk_workspace(1, 1, 1000, 1)) == sizes[5]


def test_tile_rows_is_read_from_the_library():
    from irc_amd import retrieval

    assert retrieval.IVF_TILE_ROWS == _lib.load().irc_ivf_tile_rows() >= 32


# ---------------------------------------------------------------- wrapper validation
def _cpu_index(N=12, D=16, nlist=3, group=None):
    from irc_amd.retrieval import IVFDenseIndex

    g = torch.Generator().manual_seed(0)
    return IVFDenseIndex.from_lists(torch.randn(N, D, generator=g),
                                    torch.randn(nlist, D, generator=g), torch.arange(N) % nlist,
                                    doc_offset=5, group=group)


def test_from_lists_builds_the_layout_on_any_device():
    index = _cpu_index()
    assert index.docs.dtype == torch.bfloat16 and index.centroids.dtype == torch.bfloat16
    assert index.row_id.dtype == torch.int32
    assert index.row_id.tolist() == [5 + r for c in range(3) for r in range(c, 12, 3)]
    assert index.list_off.tolist() == [0, 4, 8, 12] and index.max_list_rows == 4
    assert index.doc_offset == 5 and index.dtype == "bf16"


def test_the_wrapper_checks_its_arguments_before_any_device_work(monkeypatch):
    import irc_amd.retrieval as R

    def boom(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(R._lib, "call", boom)
    monkeypatch.setattr(R._lib, "fn", boom)
    index = _cpu_index()
    q = torch.zeros(2, 16)
    pr = torch.zeros(2, 1, dtype=torch.int32)
    with pytest.raises(ValueError, match="exactly one of nprobe and probe"):
        index.search(q, 5)
    with pytest.raises(ValueError, match="exactly one of nprobe and probe"):
        index.search(q, 5, nprobe=1, probe=pr)
    for bad in (0, 4):
        with pytest.raises(ValueError, match="nprobe="):
            index.search(q, 5, nprobe=bad)
        with pytest.raises(ValueError, match="nprobe="):
            index.probe(q, bad)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="k="):
            index.search(q, bad, nprobe=1)
    with pytest.raises(ValueError, match="dim mismatch"):
        index.search(torch.zeros(2, 8), 5, nprobe=1)
    with pytest.raises(ValueError, match="probe must be"):
        index.search(q, 5, probe=torch.zeros(3, 1, dtype=torch.int32))
    # CPU tensors raise through require_hip, as everywhere
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.search(q, 5, nprobe=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        index.search(q, 5, probe=pr)


def test_what_is_not_built_says_so():
    from irc_amd.retrieval import IVFDenseIndex

    index = _cpu_index()
    q = torch.zeros(2, 16)
    with pytest.raises(NotImplementedError, match="permuted"):
        index.search(q, 5, nprobe=1, group_off=torch.tensor([0, 12]))
    with pytest.raises(NotImplementedError, match="permuted"):
        index.search_candidates(q, torch.zeros(0, dtype=torch.int32), torch.zeros(3), 5)
    with pytest.raises(NotImplementedError, match="follow-up"):
        index.search_many([q], 5)
    with pytest.raises(TypeError, match="from_lists"):
        IVFDenseIndex(torch.zeros(4, 16))
    with pytest.raises(ValueError, match="bf16 only"):
        IVFDenseIndex.from_lists(torch.zeros(4, 16), torch.zeros(2, 16), torch.zeros(4),
                                 dtype="fp8")


def test_main_rejects_what_the_ivf_index_does_not_do(capsys):
    import main as entry

    base = ["--data", "fever", "--retrieval", "dense", "--index", "ivf"]
    assert entry.get_args(base + ["--nlist", "16", "--nprobe", "4"]).index == "ivf"
    assert entry.get_args([]).index == "flat"
    for extra, word in ((["--rerank-unit", "page"], "per-page"),
                        (["--index-dtype", "fp8"], "bf16"), (["--nprobe", "0"], "nprobe"),
                        (["--nlist", "4", "--nprobe", "5"], "nprobe")):
        with pytest.raises(SystemExit):
            entry.get_args(base + extra)
        assert word in capsys.readouterr().err
    with pytest.raises(SystemExit):
        entry.get_args(["--data", "fever", "--retrieval", "hybrid", "--index", "ivf"])
    assert "hybrid" in capsys.readouterr().err


# ---------------------------------------------------------------- two gloo ranks
K, NPROBE, NLIST = 6, 2, 5


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _corpus():
    """Integer-grid docs [61, 16], 7 queries, a fixed assignment and fixed centroids per shard;
    exact fp32 dot products."""
    rng = np.random.default_rng(17)
    docs = (rng.integers(-4, 5, size=(61, 16)) / 8.0).astype(np.float32)
    qs = (rng.integers(-4, 5, size=(7, 16)) / 8.0).astype(np.float32)
    assign = rng.integers(0, NLIST - 1, 61)  # list 4 stays empty
    cent = (rng.integers(-4, 5, size=(WORLD, NLIST, 16)) / 8.0).astype(np.float32)
    return docs, qs, assign, cent


def _np_probe(q, cent, nprobe):
    """Inner product desc, ties to the lower list id: scan_topk over the centroids."""
    return O.scan_topk(q, cent, nprobe)[0].astype(np.int32)


def _np_search(q, docs, assign, probe, k, doc_offset):
    """The numpy reference of one shard's ivf_topk: (scores, idx, n)."""
    Q = q.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_s = np.full((Q, k), -np.inf, np.float32)
    out_n = np.zeros(Q, np.int32)
    for r in range(Q):
        ids = np.flatnonzero(np.isin(assign, [c for c in probe[r] if c >= 0]))
        if ids.size == 0:
            continue
        sc = (docs[ids].astype(np.float64) @ q[r].astype(np.float64)).astype(np.float32)
        ti, ts = O.topk_rows(sc[None, :], k)
        m = min(k, ids.size)
        out_i[r, :m], out_s[r, :m], out_n[r] = doc_offset + ids[ti[0, :m]], ts[0, :m], m
    return out_s, out_i, out_n


SPLITS = {"ragged": (5, 2), "one_empty": (7, 0)}


def _worker(rank, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD,
                            timeout=datetime.timedelta(seconds=60))
    import irc_amd.retrieval as R

    docs, qs, assign, cent = _corpus()
    lo, hi = R.shard_bounds(docs.shape[0], WORLD, rank)

    class CpuIVF(R.IVFDenseIndex):
        """The device calls as numpy references: this shard's probe and ivf_topk (over the
        index's own list layout), and the merge."""

        def _local_ivf(self, queries, k, nprobe, probe, ws_tag):
            assert probe is None
            q = queries.numpy()
            pr = _np_probe(q, self.centroids.float().numpy(), nprobe)
            rid, off = self.row_id.numpy(), self.list_off.numpy()
            where = np.empty(rid.size, np.int64)  # the list of each original row
            for c in range(off.size - 1):
                where[rid[off[c]:off[c + 1]] - self.doc_offset] = c
            d = np.empty((rid.size, q.shape[1]), np.float32)
            d[rid - self.doc_offset] = self.docs.float().numpy()
            return tuple(torch.from_numpy(x)
                         for x in _np_search(q, d, where, pr, k, self.doc_offset))

        def _merge(self, scores, idx, k):
            i, s = O.merge_topk(list(idx.numpy()), list(scores.numpy()), k)
            return torch.from_numpy(s), torch.from_numpy(i)

    index = CpuIVF.from_lists(torch.from_numpy(docs[lo:hi]), torch.from_numpy(cent[rank]),
                              torch.from_numpy(assign[lo:hi]), doc_offset=lo,
                              group=dist.group.WORLD)
    try:
        for name, counts in SPLITS.items():
            a = sum(counts[:rank])
            b = a + counts[rank]
            out = index.search(torch.from_numpy(qs[a:b]), K, nprobe=NPROBE)
            assert len(out) == 3 and out[2].dtype == torch.int32
            np.savez(os.path.join(out_dir, f"{name}_r{rank}.npz"), *[x.numpy() for x in out])
    finally:
        dist.destroy_process_group()


def test_sharded_search_gloo(tmp_path):
    docs, qs, assign, cent = _corpus()
    mp.start_processes(_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True,
                       start_method="spawn")
    # the reference over both shards' probed lists: each shard probes NPROBE of its own
    from irc_amd.retrieval import shard_bounds

    parts = []
    for rank in range(WORLD):
        lo, hi = shard_bounds(docs.shape[0], WORLD, rank)
        parts.append(_np_search(qs, docs[lo:hi], assign[lo:hi], _np_probe(qs, cent[rank], NPROBE),
                                K, lo))
    ri, rs = O.merge_topk([p[1] for p in parts], [p[0] for p in parts], K)
    rn = (ri >= 0).sum(axis=1).astype(np.int32)
    assert (rn > 0).all()
    for name in SPLITS:
        for r in range(WORLD):
            with np.load(tmp_path / f"{name}_r{r}.npz") as z:
                got = [z[f"arr_{j}"] for j in range(3)]
            for x, y in zip(got, (rs, ri, rn)):
                np.testing.assert_array_equal(x, y, err_msg=f"{name} rank {r}")


def test_probe_over_a_process_group_raises_before_any_collective(monkeypatch):
    import irc_amd.retrieval as R

    index = _cpu_index(group=object())
    monkeypatch.setattr(R.ShardedDenseIndex, "_sharded", lambda self: True)

    def boom(*a, **kw):
        raise AssertionError("a collective was started")

    monkeypatch.setattr(dist, "all_gather", boom)
    monkeypatch.setattr(dist, "get_world_size", boom)
    q = torch.zeros(2, 16)
    with pytest.raises(ValueError, match="per shard"):
        index.search(q, 5, probe=torch.zeros(2, 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="nprobe="):
        index.search(q, 5, nprobe=9)
    with pytest.raises(ValueError, match="dim mismatch"):
        index.search(torch.zeros(2, 8), 5, nprobe=1)
