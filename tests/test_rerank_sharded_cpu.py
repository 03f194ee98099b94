"""CPU checks of the candidate top-k over a sharded corpus: the numpy reference of the
grouped merge (irc_topk_merge_grouped) on hand-written cases; the entry's host-side
validation; and the collective ``ShardedDenseIndex.search_candidates`` in two gloo ranks with
the device calls replaced by the numpy references (the GPU tests cover the kernels), whose
result must equal the reference over the whole corpus, bit for bit, on both ranks."""
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
from test_rerank_group_cpu import _reference_grouped

from irc_amd import _lib

WORLD = 2


def _reference_merge_grouped(scores, idx, k, group_off):
    """(idx [Q, k], scores [Q, k], n [Q], groups [Q, k]) of the [P, Q, kin] lists: the
    entries with idx >= 0 that lie in a group, ranked by (score desc, id asc); the first --
    best -- entry of every group stays, the first k of those are returned."""
    scores, idx = np.asarray(scores, np.float32), np.asarray(idx, np.int64)
    P, Q, kin = idx.shape
    go = np.asarray(group_off, np.int64)
    out_i = np.full((Q, k), -1, np.int64)
    out_s = np.full((Q, k), -np.inf, np.float32)
    out_n = np.zeros(Q, np.int32)
    out_g = np.full((Q, k), -1, np.int64)
    for r in range(Q):
        ids, sc = idx[:, r, :].ravel(), O.canon_scores(scores[:, r, :].ravel())
        keep = (ids >= 0) & (ids >= go[0]) & (ids < go[-1])
        ids, sc = ids[keep], sc[keep]
        order = np.lexsort((ids, -sc))
        ids, sc = ids[order], sc[order]
        grp = np.searchsorted(go, ids, side="right") - 1
        _, first = np.unique(grp, return_index=True)
        first = np.sort(first)[:k]
        m = first.size
        out_i[r, :m], out_s[r, :m], out_g[r, :m], out_n[r] = ids[first], sc[first], grp[first], m
    return out_i, out_s, out_n, out_g


def test_merge_reference_on_a_hand_written_case():
    # groups {0, 1, 2}, {} , {3, 4}, {5}, {6, 7}; rows 8 and 9 in no group
    go = [0, 3, 3, 5, 6, 8]
    ninf = -np.inf
    # one query, three lists of 3: group 0 has its best rows 2 (list 0) and 1 (list 1), both
    # 5.0 -> row 1; groups 2 and 3 tie at 4.0 -> row 4 before row 5; row 9 (score 9) is in no
    # group; list 2 is all empty; an empty slot in the middle of list 1 carries a NaN score
    idx = np.array([[[2, 5, 9]], [[1, -1, 4]], [[-1, -1, -1]]], np.int64)
    sc = np.array([[[5, 4, 9]], [[5, np.nan, 4]], [[ninf, ninf, ninf]]], np.float32)
    i, s, n, g = _reference_merge_grouped(sc, idx, 4, go)  # kout above the 3 groups present
    assert n.tolist() == [3]
    assert i.tolist() == [[1, 4, 5, -1]]
    assert s.tolist() == [[5.0, 4.0, 4.0, ninf]]
    assert g.tolist() == [[0, 2, 3, -1]]
    i, s, n, g = _reference_merge_grouped(sc, idx, 2, go)  # kout below
    assert (i.tolist(), s.tolist(), n.tolist(), g.tolist()) == ([[1, 4]], [[5.0, 4.0]], [2],
                                                                [[0, 2]])


def test_merge_reference_two_queries_and_losers_of_a_shared_group():
    go = [10, 12, 12, 20]  # groups {10, 11}, {}, {12 .. 19}
    # query 0: group 2 in both lists (13 at 1.0, 17 at 2.0) and group 0 once; query 1: only
    # rows of no group (9 and 20) and empty slots
    idx = np.array([[[13, 10], [9, -1]], [[17, -1], [-1, 20]]], np.int64)
    sc = np.array([[[1, 0], [3, 0]], [[2, 0], [0, 3]]], np.float32)
    i, s, n, g = _reference_merge_grouped(sc, idx, 3, go)
    assert n.tolist() == [2, 0]
    assert i.tolist() == [[17, 10, -1], [-1, -1, -1]]
    assert g.tolist() == [[2, 0, -1], [-1, -1, -1]]
    assert s[0].tolist() == [2.0, 0.0, -np.inf] and np.isneginf(s[1]).all()
    # no groups at all: all padding
    i, s, n, g = _reference_merge_grouped(sc, idx, 3, [5])
    assert (i == -1).all() and (n == 0).all() and (g == -1).all() and np.isneginf(s).all()


# ---------------------------------------------------------------- host validation
_GO = (ctypes.c_int64 * 3)(0, 2, 4)


def _call(lib, P=2, Q=4, kin=10, kout=10, group_off=_GO, n_groups=2, ws=None, ws_bytes=0):
    return lib.irc_topk_merge_grouped(None, None, P, Q, kin, kout, group_off, n_groups, ws,
                                      ws_bytes, None, None, None, None)


def test_merge_grouped_entry_is_registered():
    assert "irc_topk_merge_grouped" in _lib.SIGNATURES
    assert "irc_topk_merge_grouped_workspace" in _lib.SIGNATURES


def test_merge_grouped_rejects_bad_arguments_on_the_host():
    lib = _lib.load()
    prefix = b"topk_merge_grouped:"

    def bad(sub, **kw):
        assert _call(lib, **kw) == 1001  # IRC_E_INVALID
        msg = lib.irc_last_error()
        assert msg.startswith(prefix) and sub in msg, msg

    bad(b"bad sizes", P=0)
    bad(b"bad sizes", Q=-1)
    bad(b"bad sizes", kin=0)
    bad(b"above 8192", P=1, kin=8193)  # P * kin = 8193
    bad(b"above 8192", P=8193, kin=1)
    bad(b"above 8192", P=3, kin=2731)  # 8193 again
    bad(b"above 8192", P=1 << 40, kin=1 << 40)  # no overflow into range
    bad(b"kout=0", kout=0)
    bad(b"kout=1025", kout=1025)
    bad(b"n_groups=-1", n_groups=-1)
    bad(b"n_groups=", n_groups=(1 << 31) - 1)
    bad(b"null group_off", group_off=None)
    # every size is fine: the workspace, before the array pointers
    need = int(lib.irc_topk_merge_grouped_workspace(2, 4, 10))
    assert need >= 2 * 4 * 10 * 8 + 5 * 8
    bad(b"workspace", ws=None, ws_bytes=need)
    buf = (ctypes.c_char * need)()
    bad(b"workspace", ws=ctypes.addressof(buf), ws_bytes=need - 1)
    bad(b"null pointer", ws=ctypes.addressof(buf), ws_bytes=need)
    # the 8192 cap itself passes the size checks (8 shards x 1024)
    bad(b"workspace", P=8, kin=1024, kout=1024)
    # Q == 0: nothing to do, nothing touched
    assert _call(lib, Q=0) == 0
    assert _call(lib, Q=0, group_off=None) == 0
    assert int(lib.irc_topk_merge_grouped_workspace(1, 1, 8193)) == 0


def test_merge_grouped_wrapper_checks_before_the_library(monkeypatch):
    from irc_amd import retrieval

    def boom(*a, **kw):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "call", boom)
    monkeypatch.setattr(_lib, "fn", boom)
    s, i = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.int64)
    for bad, exc in ((None, TypeError), (torch.zeros(3, dtype=torch.int32), TypeError),
                     ([0, 1], TypeError), (torch.zeros((2, 2), dtype=torch.int64), ValueError),
                     (torch.zeros(0, dtype=torch.int64), ValueError)):
        with pytest.raises(exc, match="group_off"):
            retrieval.topk_merge_grouped(s, i, 4, bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.topk_merge_grouped(s, i, 4, torch.tensor([0, 2, 4]))


# ---------------------------------------------------------------- two gloo ranks
K = 10


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _corpus():
    """Integer-grid corpus (exact scores, many ties), 7 queries, their candidate lists over
    the WHOLE corpus -- so every list holds ids of both shards -- and group offsets with a
    group cut by the shard boundary (151), rows 0, 1 and 297 .. 300 in no group."""
    rng = np.random.default_rng(3)
    docs = (rng.integers(-4, 5, size=(301, 16)) / 8.0).astype(np.float32)
    qs = (rng.integers(-4, 5, size=(7, 16)) / 8.0).astype(np.float32)
    lens = [301, 0, 150, 40, 7, 3, 200]  # all rows; empty; fewer than K in two lists
    lists = [np.sort(rng.choice(301, n, replace=False)).astype(np.int64) for n in lens]
    lists[4] = np.concatenate([lists[4], [301, 4000]])  # ids no shard owns
    go = [2]
    sizes = [3, 0, 7, 1, 12, 5]
    while go[-1] + sizes[(len(go) - 1) % 6] <= 297:
        go.append(go[-1] + sizes[(len(go) - 1) % 6])
    go[-1] = 297
    return docs, qs, lists, np.asarray(go, np.int64)


def _pack(lists, dtype):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate(lists) if len(lists) and off[-1] else np.zeros(0, np.int64)
    return torch.from_numpy(flat.astype(np.int64)).to(dtype), torch.from_numpy(off)


def _lists_of(cand, cand_off):
    c, o = cand.numpy(), cand_off.numpy()
    return [c[o[r]:o[r + 1]] for r in range(o.size - 1)]


SPLITS = {"ragged": (5, 2), "one_empty": (7, 0)}


def _worker(rank, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD,
                            timeout=datetime.timedelta(seconds=60))
    import irc_amd.retrieval as R

    docs, qs, lists, go = _corpus()
    lo, hi = R.shard_bounds(docs.shape[0], WORLD, rank)

    class CpuIndex(R.ShardedDenseIndex):
        """The device calls as numpy references: this shard's (grouped) candidate top-k and
        the two merges."""

        def __init__(self, docs, doc_offset, group):
            self.docs, self.doc_offset, self.group, self.dtype = docs, doc_offset, group, "bf16"

        def _local_candidates(self, queries, cand, cand_off, k, ws_tag="rerank",
                              method="gather", ascending=False, group_off=None):
            assert cand.dtype == torch.int32 and cand_off.dtype == torch.int64
            d = self.docs.numpy()
            # ungrouped: every row a group of its own
            g = np.arange(self.doc_offset, self.doc_offset + d.shape[0] + 1) \
                if group_off is None else group_off.numpy()
            i, s, n, grp = _reference_grouped(queries.numpy(), d, _lists_of(cand, cand_off), k,
                                              g, self.doc_offset)
            out = (torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(n))
            return out if group_off is None else out + (torch.from_numpy(grp),)

        def _merge(self, scores, idx, k):
            i, s = O.merge_topk(list(idx.numpy()), list(scores.numpy()), k)
            return torch.from_numpy(s), torch.from_numpy(i)

        def _merge_grouped(self, scores, idx, k, group_off):
            i, s, n, g = _reference_merge_grouped(scores.numpy(), idx.numpy(), k,
                                                  group_off.numpy())
            return (torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(n),
                    torch.from_numpy(g))

    index = CpuIndex(torch.from_numpy(docs[lo:hi]), lo, dist.group.WORLD)
    try:
        for name, counts in SPLITS.items():
            a = sum(counts[:rank])
            b = a + counts[rank]
            # the ranks need not agree on the id dtype
            cand, off = _pack(lists[a:b], torch.int64 if rank == 0 else torch.int32)
            for grouped in (False, True):
                out = index.search_candidates(torch.from_numpy(qs[a:b]), cand, off, K,
                                              ascending=True,
                                              group_off=torch.from_numpy(go) if grouped else None)
                assert len(out) == (4 if grouped else 3)
                np.savez(os.path.join(out_dir, f"{name}_{int(grouped)}_r{rank}.npz"),
                         *[x.numpy() for x in out])
    finally:
        dist.destroy_process_group()


def test_sharded_search_candidates_gloo(tmp_path):
    docs, qs, lists, go = _corpus()
    # a group is cut by the shard boundary, and some list has rows of it on both sides
    g = np.searchsorted(go, 151, side="right") - 1
    assert go[g] < 151 < go[g + 1]  # rows below 151 in shard 0, from 151 on in shard 1
    assert any(((x >= go[g]) & (x < 151)).any() and ((x >= 151) & (x < go[g + 1])).any()
               for x in lists)
    mp.start_processes(_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True,
                       start_method="spawn")
    whole = np.arange(0, docs.shape[0] + 1)
    ri, rs, rn, _ = _reference_grouped(qs, docs, lists, K, whole)
    plain = (rs, ri, rn)
    gi, gs, gn, gg = _reference_grouped(qs, docs, lists, K, go)
    assert (gn < rn).any() and (rn < K).any()  # something collapsed; a short list
    for name in SPLITS:
        for r in range(WORLD):
            with np.load(tmp_path / f"{name}_0_r{r}.npz") as z:
                got = [z[f"arr_{j}"] for j in range(3)]
            for x, y in zip(got, plain):
                np.testing.assert_array_equal(x, y, err_msg=f"{name} rank {r}")
            assert got[2].dtype == np.int32
            with np.load(tmp_path / f"{name}_1_r{r}.npz") as z:
                got = [z[f"arr_{j}"] for j in range(4)]
            for x, y in zip(got, (gs, gi, gn, gg)):
                np.testing.assert_array_equal(x, y, err_msg=f"{name} grouped rank {r}")


def test_a_bad_argument_raises_before_any_collective(monkeypatch):
    """The rank's own checks come first: with a process group that would hang or fail on
    any collective, the error is the argument's."""
    import irc_amd.retrieval as R

    index = R.ShardedDenseIndex.__new__(R.ShardedDenseIndex)
    index.dtype, index.group, index.doc_offset, index.fp8_scale = "bf16", object(), 0, 16.0
    index.docs = torch.zeros(4, 16, dtype=torch.bfloat16)
    monkeypatch.setattr(R.ShardedDenseIndex, "_sharded", lambda self: True)

    def boom(*a, **kw):
        raise AssertionError("a collective was started")

    monkeypatch.setattr(dist, "all_gather", boom)
    monkeypatch.setattr(dist, "get_world_size", boom)
    q, c, off = torch.zeros(2, 16), torch.zeros(3, dtype=torch.int32), torch.tensor([0, 1, 3])
    with pytest.raises(ValueError, match="cand_off"):
        index.search_candidates(q, c, torch.tensor([0, 3]), 2)
    with pytest.raises(TypeError, match="cand must be"):
        index.search_candidates(q, c.float(), off, 2)
    with pytest.raises(ValueError, match="method"):
        index.search_candidates(q, c, off, 2, method="scan")
    with pytest.raises(ValueError, match="dim mismatch"):
        index.search_candidates(torch.zeros(2, 8), c, off, 2)
    with pytest.raises(TypeError, match="group_off"):
        index.search_candidates(q, c, off, 2, group_off=[0, 2])
