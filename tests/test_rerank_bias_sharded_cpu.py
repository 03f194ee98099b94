"""CPU check of the bias in the collective ``ShardedDenseIndex.search_candidates``: two gloo
ranks, the device calls replaced by test doubles as in test_rerank_sharded_cpu.py.  Every
candidate's bias is a function of (its query, its id), so after the ragged gather -- one rank
with more candidates than the other, and one rank with an empty slice -- each rank can tell
whether entry j of the gathered bias still belongs to gathered candidate j; the ranked result
must equal the single-process reference with the same bias on both ranks.  With ``bias=None``
the doubles keep today's signatures (no ``bias`` parameter at all) and must still be
callable: the bias is passed and returned only when one was given."""
import datetime
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PKG, ROOT  # noqa: F401  (import paths)
from oracle import irc_oracle as O
from test_rerank_sharded_cpu import SPLITS, WORLD, _corpus, _free_port, _lists_of, _pack

K = 10


def _bias_of(r, ids):
    """The bias of global query r's candidates ``ids``: exact in fp32 (multiples of 1/8),
    and large enough against the grid scores (|s| <= 4) to reorder them."""
    ids = np.asarray(ids, np.int64)
    return (((ids * 7 + r * 13) % 41) / 8.0 - 2.0).astype(np.float32)


def _reference_biased(q, d, lists, bias, k, doc_offset=0):
    """(scores, idx, n): per list the eligible candidates, fp64 scores cast to fp32 (exact on
    the grid), plus the fp32 bias in one fp32 addition, ranked by (score desc, id asc)."""
    Q, N = q.shape[0], d.shape[0]
    out_i = np.full((Q, k), -1, np.int64)
    out_s = np.full((Q, k), -np.inf, np.float32)
    out_n = np.zeros(Q, np.int32)
    for r, (ids, b) in enumerate(zip(lists, bias)):
        ids, b = np.asarray(ids, np.int64), np.asarray(b, np.float32)
        ok = (ids >= doc_offset) & (ids < doc_offset + N)
        ids, b = ids[ok], b[ok]
        if ids.size == 0:
            continue
        s = (d[ids - doc_offset].astype(np.float64) @ q[r].astype(np.float64)).astype(np.float32)
        s = O.canon_scores(s + b)
        order = np.lexsort((ids, -s))[:k]
        m = order.size
        out_i[r, :m], out_s[r, :m], out_n[r] = ids[order], s[order], m
    return out_s, out_i, out_n


def _worker(rank, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD,
                            timeout=datetime.timedelta(seconds=60))
    import irc_amd.retrieval as R

    docs, qs, lists, _ = _corpus()
    lo, hi = R.shard_bounds(docs.shape[0], WORLD, rank)
    seen = {}

    class Base(R.ShardedDenseIndex):
        def __init__(self, docs, doc_offset, group):
            self.docs, self.doc_offset, self.group, self.dtype = docs, doc_offset, group, "bf16"

        def _merge(self, scores, idx, k):
            i, s = O.merge_topk(list(idx.numpy()), list(scores.numpy()), k)
            return torch.from_numpy(s), torch.from_numpy(i)

    class BiasedIndex(Base):
        """The local call as the numpy reference with the gathered bias."""

        def _local_candidates(self, queries, cand, cand_off, k, ws_tag="rerank",
                              method="gather", ascending=False, group_off=None, bias=None):
            assert cand.dtype == torch.int32 and cand_off.dtype == torch.int64
            assert bias is not None and bias.dtype == torch.float32
            assert bias.shape == cand.shape
            ls = _lists_of(cand, cand_off)
            bs = _lists_of(bias, cand_off)
            # aligned: every gathered bias is still the one of its (query, candidate)
            for r, (ids, b) in enumerate(zip(ls, bs)):
                assert np.array_equal(ids, lists[r])
                assert np.array_equal(b, _bias_of(r, ids)), f"query {r}: the bias moved"
            seen["local"] = True
            s, i, n = _reference_biased(queries.numpy(), self.docs.numpy(), ls, bs, k,
                                        self.doc_offset)
            return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(n)

    class PlainIndex(Base):
        """Today's doubles, parameter for parameter: no ``bias`` anywhere."""

        def _local_candidates(self, queries, cand, cand_off, k, ws_tag="rerank",
                              method="gather", ascending=False, group_off=None):
            seen["plain_local"] = True
            zero = [np.zeros(len(x), np.float32) for x in _lists_of(cand, cand_off)]
            s, i, n = _reference_biased(queries.numpy(), self.docs.numpy(),
                                        _lists_of(cand, cand_off), zero, k, self.doc_offset)
            return torch.from_numpy(s), torch.from_numpy(i), torch.from_numpy(n)

        def _own_candidates(self, queries, cand, cand_off, method):
            out = super()._own_candidates(queries, cand, cand_off, method)
            assert len(out) == 2
            return out

        def _gather_candidates(self, queries, cand, cand_off):
            out = super()._gather_candidates(queries, cand, cand_off)
            assert len(out) == 3
            return out

    try:
        for name, counts in SPLITS.items():
            a = sum(counts[:rank])
            b = a + counts[rank]
            cand, off = _pack(lists[a:b], torch.int64 if rank == 0 else torch.int32)
            mine = [_bias_of(r, lists[r]) for r in range(a, b)]
            bias = torch.from_numpy(np.concatenate(mine) if mine else np.zeros(0, np.float32))
            q = torch.from_numpy(qs[a:b])
            index = BiasedIndex(torch.from_numpy(docs[lo:hi]), lo, dist.group.WORLD)
            out = index.search_candidates(q, cand, off, K, ascending=True, bias=bias)
            assert len(out) == 3 and seen.pop("local")
            np.savez(os.path.join(out_dir, f"{name}_biased_r{rank}.npz"),
                     *[x.numpy() for x in out])
            index = PlainIndex(torch.from_numpy(docs[lo:hi]), lo, dist.group.WORLD)
            out = index.search_candidates(q, cand, off, K, ascending=True)
            assert len(out) == 3 and seen.pop("plain_local")
            np.savez(os.path.join(out_dir, f"{name}_plain_r{rank}.npz"),
                     *[x.numpy() for x in out])
    finally:
        dist.destroy_process_group()


def test_the_bias_arrives_with_its_candidate_gloo(tmp_path):
    docs, qs, lists, _ = _corpus()
    assert 0 in SPLITS["one_empty"]  # a rank with an empty slice
    assert len({sum(len(x) for x in lists[:5]), sum(len(x) for x in lists[5:])}) == 2  # ragged
    mp.start_processes(_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True,
                       start_method="spawn")
    bias = [_bias_of(r, ids) for r, ids in enumerate(lists)]
    want = _reference_biased(qs, docs, lists, bias, K)
    plain = _reference_biased(qs, docs, lists, [np.zeros_like(b) for b in bias], K)
    assert not np.array_equal(want[1], plain[1])  # the bias changes the ranking
    for name in SPLITS:
        for r in range(WORLD):
            for kind, ref in (("biased", want), ("plain", plain)):
                with np.load(tmp_path / f"{name}_{kind}_r{r}.npz") as z:
                    got = [z[f"arr_{j}"] for j in range(3)]
                for x, y in zip(got, ref):
                    np.testing.assert_array_equal(x, y, err_msg=f"{name} {kind} rank {r}")
                assert got[2].dtype == np.int32


def test_single_process_doubles_see_todays_arguments():
    """Not sharded: ``_local_candidates`` is called with today's eight positional arguments
    when no bias is given, and with ``bias=`` as one more keyword when one is."""
    import irc_amd.retrieval as R

    calls = []

    class Index(R.ShardedDenseIndex):
        def __init__(self):
            self.docs, self.doc_offset, self.group, self.dtype = torch.zeros(4, 16), 0, None, "bf16"

        def _local_candidates(self, *args, **kw):
            calls.append((args, kw))
            return "out"

    q, c, off = torch.zeros(2, 16), torch.zeros(3, dtype=torch.int32), torch.tensor([0, 1, 3])
    index = Index()
    assert index.search_candidates(q, c, off, 2, "tag", "stream", True) == "out"
    args, kw = calls.pop()
    assert kw == {} and len(args) == 8
    assert args[3:] == (2, "tag", "stream", True, None)
    b = torch.ones(3)
    assert index.search_candidates(q, c, off, 2, bias=b) == "out"
    args, kw = calls.pop()
    assert list(kw) == ["bias"] and kw["bias"] is b and len(args) == 8
