"""The collective ``ShardedDenseIndex.search(group_off=...)`` in two gloo ranks, with the
device calls replaced by the numpy references (the GPU tests cover the kernels), after
tests/test_rerank_sharded_cpu.py: the orchestration returns the whole batch in rank order on
both ranks, the merged result equals the grouped reference over the whole corpus bit for
bit, a rank whose shard touches no group still joins every collective, and a bad argument
raises before the first collective."""
import datetime
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT  # noqa: F401  (import paths)
from test_rerank_group_cpu import _reference_grouped
from test_rerank_sharded_cpu import _free_port, _reference_merge_grouped

WORLD = 2
K = 10


def _corpus():
    """Integer-grid corpus (exact scores, many ties), 7 queries, group offsets with a group
    cut by the shard boundary (151); rows 0, 1 and 297 .. 300 in no group."""
    rng = np.random.default_rng(5)
    docs = (rng.integers(-4, 5, size=(301, 16)) / 8.0).astype(np.float32)
    qs = (rng.integers(-4, 5, size=(7, 16)) / 8.0).astype(np.float32)
    go = [2]
    sizes = [3, 0, 7, 1, 12, 5]
    while go[-1] + sizes[(len(go) - 1) % 6] <= 297:
        go.append(go[-1] + sizes[(len(go) - 1) % 6])
    go[-1] = 297
    return docs, qs, np.asarray(go, np.int64)


# group offsets of the run: "cut" the corpus-wide ones; "low" groups over rows of shard 0
# only, so rank 1's local slice is empty
GROUPS = {"cut": None, "low": np.asarray([1, 4, 4, 30, 100], np.int64)}
SPLITS = {"ragged": (5, 2), "one_empty": (7, 0)}


def _all_rows(Q, lo, hi):
    return [np.arange(lo, hi, dtype=np.int64)] * Q


def _worker(rank, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD,
                            timeout=datetime.timedelta(seconds=60))
    import irc_amd.retrieval as R

    docs, qs, go_cut = _corpus()
    lo, hi = R.shard_bounds(docs.shape[0], WORLD, rank)
    seen = []

    class CpuIndex(R.ShardedDenseIndex):
        """The device calls as numpy references: this shard's grouped scan over its own
        slice of the groups, and the grouped merge."""

        def __init__(self, docs, doc_offset, group):
            self.docs, self.doc_offset, self.group, self.dtype = docs, doc_offset, group, "bf16"

        def _local_topk(self, queries, k, ws_tag="scan", group_off=None):
            assert group_off is not None
            cut = self._local_groups(group_off)  # the memoised slice, as the device call
            seen.append(int(cut.numel()) - 1)
            d = self.docs.numpy()
            i, s, n, _ = _reference_grouped(queries.numpy(), d,
                                            _all_rows(queries.shape[0], self.doc_offset,
                                                      self.doc_offset + d.shape[0]),
                                            k, cut.numpy(), self.doc_offset)
            return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(n)

        def _merge_grouped(self, scores, idx, k, group_off):
            i, s, n, g = _reference_merge_grouped(scores.numpy(), idx.numpy(), k,
                                                  group_off.numpy())
            return (torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(n),
                    torch.from_numpy(g))

    index = CpuIndex(torch.from_numpy(docs[lo:hi]), lo, dist.group.WORLD)
    try:
        for gname, go in GROUPS.items():
            got = torch.from_numpy(go_cut if go is None else go)
            for name, counts in SPLITS.items():
                a = sum(counts[:rank])
                b = a + counts[rank]
                out = index.search(torch.from_numpy(qs[a:b]), K, group_off=got)
                assert len(out) == 4
                assert index._group_slice[0] is got  # one slice per tensor object
                np.savez(os.path.join(out_dir, f"{gname}_{name}_r{rank}.npz"),
                         *[x.numpy() for x in out])
        # the slice of each run: all the groups a shard touches, none for rank 1 under "low"
        np.save(os.path.join(out_dir, f"seen_r{rank}.npy"), np.asarray(seen))
    finally:
        dist.destroy_process_group()


def test_sharded_grouped_search_gloo(tmp_path):
    docs, qs, go_cut = _corpus()
    g = np.searchsorted(go_cut, 151, side="right") - 1
    assert go_cut[g] < 151 < go_cut[g + 1]  # rows of one group in both shards
    mp.start_processes(_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True,
                       start_method="spawn")
    rows = _all_rows(qs.shape[0], 0, docs.shape[0])
    for gname, go in GROUPS.items():
        go = go_cut if go is None else go
        gi, gs, gn, gg = _reference_grouped(qs, docs, rows, K, go)
        assert (gn == min(K, np.count_nonzero(np.diff(go)))).all()
        for name in SPLITS:
            for r in range(WORLD):
                with np.load(tmp_path / f"{gname}_{name}_r{r}.npz") as z:
                    got = [z[f"arr_{j}"] for j in range(4)]
                for x, y in zip(got, (gs, gi, gn, gg)):  # the whole batch, in rank order
                    np.testing.assert_array_equal(x, y, err_msg=f"{gname} {name} rank {r}")
                np.testing.assert_array_equal(got[0].view(np.uint32), gs.view(np.uint32))
                assert got[2].dtype == np.int32
    seen = [np.load(tmp_path / f"seen_r{r}.npy").tolist() for r in range(WORLD)]
    n_cut = len(go_cut) - 1
    assert all(0 < s < n_cut for s in seen[0][:2] + seen[1][:2])  # each its own part of "cut"
    assert seen[0][0] + seen[1][0] == n_cut + 1  # ... the cut group in both
    assert seen[0][2:] == [4, 4] and seen[1][2:] == [0, 0]  # "low": rank 1 touches no group


def test_a_bad_argument_raises_before_any_collective(monkeypatch):
    """The rank's own checks come first: with a process group that would hang or fail on any
    collective, the error is the argument's."""
    import irc_amd.retrieval as R

    index = R.ShardedDenseIndex.__new__(R.ShardedDenseIndex)
    index.dtype, index.group, index.doc_offset, index.fp8_scale = "bf16", object(), 0, 16.0
    index.docs = torch.zeros(4, 16, dtype=torch.bfloat16)
    monkeypatch.setattr(R.ShardedDenseIndex, "_sharded", lambda self: True)

    def boom(*a, **kw):
        raise AssertionError("a collective was started")

    monkeypatch.setattr(dist, "all_gather", boom)
    monkeypatch.setattr(dist, "get_world_size", boom)
    q, go = torch.zeros(2, 16), torch.tensor([0, 2, 4])
    with pytest.raises(TypeError, match="group_off"):
        index.search(q, 2, group_off=[0, 2])
    with pytest.raises(TypeError, match="group_off"):
        index.search(q, 2, group_off=go.int())
    with pytest.raises(ValueError, match="group_off"):
        index.search(q, 2, group_off=go.reshape(1, 3))
    with pytest.raises(ValueError, match="dim mismatch"):
        index.search(torch.zeros(2, 8), 2, group_off=go)
    with pytest.raises(ValueError, match="k=1025"):
        index.search(q, 1025, group_off=go)
    index.dtype, index.docs = "fp8", torch.zeros(4, 64, dtype=torch.uint8)
    with pytest.raises(ValueError, match="D % 128"):
        index.search(torch.zeros(2, 64), 2, group_off=go)
    # k * world size above the grouped merge's 8192 entries: known once the world size is
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 9)
    index.dtype, index.docs = "bf16", torch.zeros(4, 16, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="8192"):
        index.search(q, 1024, group_off=go)
