"""Dense retrieval: corpus-wide cosine top-k over a (sharded) document corpus.

Semantics: scores = <e_q, e_n> of L2-normalised
``ctx2vec`` embeddings (src/evaluation.py:110-112, src/contrastor/
contrastive_module.py:96-100), per-query top-k by descending score as in
``TfidfDocRanker.closest_docs`` (preprocessing/drqa/retriever/
tfidf_doc_ranker.py:60-75); equal scores -> lower global doc index.

Multi-GPU: the corpus is split into contiguous shards, one per
rank, resident in HBM.  A search all-gathers the query embeddings over RCCL,
scans the local shard (global indices via the shard offset), all-gathers the
per-shard top-k lists and merges them with the same exact rule.  The candidate-restricted
top-k (``search_candidates``) is sharded the same way: the queries and their candidate lists
are all-gathered, every shard ranks the candidates it owns, and the per-shard lists merge by
``topk_merge``, or by ``topk_merge_grouped`` when the unit is a group of rows.  The scan has
that unit too: ``search(..., group_off=)`` returns the top-k groups of the whole corpus
(``scan_topk_grouped``), each shard over its own slice of the groups (``local_group_slice``).

Cluster-pruned search: ``IVFDenseIndex`` keeps a shard clustered into lists and a search ranks,
exactly, only the rows of the lists nearest to each query; sharded as the scan is, each shard
probing its own lists.  A search is one stream-ordered native call (``ivf_search``: probe, the
plan built on the device, scoring, select); ``ivf_plan`` + ``ivf_topk`` are the same search with
the plan built in torch, the documented form and the oracle of the native one.  The lists can
be e4m3 bytes (``IVFDenseIndex.to_fp8``; ``ivf_search_fp8`` / ``ivf_topk_fp8``): the probe stays
bf16, the queries are quantised inside the call.
"""
from __future__ import annotations

import ctypes
import itertools

import torch

from . import _lib
from ._torch import contig, ptr, require_hip, stream_ptr, workspace


def scan_topk(queries: torch.Tensor, docs: torch.Tensor, k: int, doc_offset: int = 0,
              ws_tag: str = "scan"):
    """Exact top-k of queries @ docs.T (bf16 inputs, fp32 scores).

    queries [Q, D], docs [N, D] on the same HIP device.  Returns
    (scores fp32 [Q, k], idx int64 [Q, k]) sorted by (score desc, idx asc);
    slots past N are (-inf, -1).
    """
    require_hip(queries, docs)
    q = contig(queries, torch.bfloat16)
    d = contig(docs, torch.bfloat16)
    Q, D = q.shape
    N = d.shape[0]
    if d.shape[1] != D:
        raise ValueError(f"dim mismatch: queries D={D}, docs D={d.shape[1]}")
    out_s = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=q.device)
    nbytes = int(_lib.fn("irc_scan_topk_workspace")(Q, N, D, k))
    ws = workspace(nbytes, q.device, ws_tag)
    _lib.call("irc_scan_topk", ptr(q), ptr(d), Q, N, D, k, doc_offset, ptr(ws), ws.numel(),
              ptr(out_s), ptr(out_i), stream_ptr(q.device))
    return out_s, out_i


def scan_topk_many(batches, docs: torch.Tensor, k: int, doc_offset: int, streams,
                   ws_tag: str = "scan"):
    """scan_topk over query batches of one shape [Q, D], len(streams) of them in flight
    (batch b on streams[b % depth], each stream with its own workspace), in ONE native
    call (irc_scan_topk_many): the streams wait for the current stream first and the
    current stream waits for all of them after.  Returns [(scores, idx)] per batch, views
    of two [len(batches), Q, k] tensors; identical to scan_topk per batch."""
    qs = [contig(q, torch.bfloat16) for q in batches]
    d = contig(docs, torch.bfloat16)
    require_hip(d, *qs)
    Q, D = qs[0].shape
    N = d.shape[0]
    if d.shape[1] != D or any(q.shape != qs[0].shape for q in qs):
        raise ValueError("scan_topk_many: every batch [Q, D] with the docs' D")
    nb, depth = len(qs), len(streams)
    out_s = torch.empty((nb, Q, k), dtype=torch.float32, device=d.device)
    out_i = torch.empty((nb, Q, k), dtype=torch.int64, device=d.device)
    if nb == 0:
        return []
    nbytes = int(_lib.fn("irc_scan_topk_workspace")(Q, N, D, k))
    wss = [workspace(nbytes, d.device, f"{ws_tag}{j}") for j in range(depth)]
    qp = (ctypes.c_void_p * nb)(*[q.data_ptr() for q in qs])
    wp = (ctypes.c_void_p * depth)(*[w.data_ptr() for w in wss])
    sp = (ctypes.c_void_p * depth)(*[s.cuda_stream for s in streams])
    _lib.call("irc_scan_topk_many", qp, nb, ptr(d), Q, N, D, k, doc_offset, wp, nbytes, depth,
              ptr(out_s), ptr(out_i), sp, stream_ptr(d.device))
    return list(zip(out_s.unbind(0), out_i.unbind(0)))


def scan_scores(queries: torch.Tensor, docs: torch.Tensor) -> torch.Tensor:
    """Raw fp32 score matrix from the same MFMA path (tests / diagnostics)."""
    require_hip(queries, docs)
    q = contig(queries, torch.bfloat16)
    d = contig(docs, torch.bfloat16)
    out = torch.empty((q.shape[0], d.shape[0]), dtype=torch.float32, device=q.device)
    _lib.call("irc_scan_scores", ptr(q), ptr(d), q.shape[0], d.shape[0], q.shape[1], ptr(out),
              stream_ptr(q.device))
    return out


# fp8 corpus (BASELINE config C5): e4m3fn embeddings, stored as uint8 bytes.
# Unit-norm components times 16 sit in e4m3's normal range and far below its
# 448 maximum; a power of two keeps the descale exact.
FP8_SCALE = 16.0


def quantize_fp8(x: torch.Tensor, scale: float = FP8_SCALE) -> torch.Tensor:
    """e4m3fn(RNE(x * scale)) as a uint8 tensor of x's shape (irc_quantize_fp8)."""
    require_hip(x)
    if x.dtype not in (torch.bfloat16, torch.float32):
        x = x.float()
    xc = x.contiguous()
    out = torch.empty(xc.shape, dtype=torch.uint8, device=xc.device)
    _lib.call("irc_quantize_fp8", 0 if xc.dtype == torch.bfloat16 else 1, ptr(xc), xc.numel(),
              float(scale), ptr(out), stream_ptr(xc.device))
    return out


def _require_e4m3(*tensors):
    for t in tensors:
        if t.dtype != torch.uint8:
            raise TypeError("fp8 scan operands are e4m3 bytes (torch.uint8, see quantize_fp8)")


def _fp8_operands(queries, docs):
    require_hip(queries, docs)
    _require_e4m3(queries, docs)
    q, d = queries.contiguous(), docs.contiguous()
    if d.shape[1] != q.shape[1]:
        raise ValueError(f"dim mismatch: queries D={q.shape[1]}, docs D={d.shape[1]}")
    return q, d


def scan_topk_fp8(queries: torch.Tensor, docs: torch.Tensor, k: int, doc_offset: int = 0,
                  score_scale: float = 1.0, ws_tag: str = "scan"):
    """Exact top-k over e4m3 queries [Q, D] and docs [N, D] (uint8 bytes); the
    returned scores are the fp32 dot products of the quantised values times
    score_scale (a power of two)."""
    q, d = _fp8_operands(queries, docs)
    Q, D = q.shape
    N = d.shape[0]
    out_s = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=q.device)
    nbytes = int(_lib.fn("irc_scan_topk_fp8_workspace")(Q, N, D, k))
    ws = workspace(nbytes, q.device, ws_tag)
    _lib.call("irc_scan_topk_fp8", ptr(q), ptr(d), Q, N, D, k, doc_offset, float(score_scale),
              ptr(ws), ws.numel(), ptr(out_s), ptr(out_i), stream_ptr(q.device))
    return out_s, out_i


def scan_scores_fp8(queries: torch.Tensor, docs: torch.Tensor) -> torch.Tensor:
    """Raw fp32 dot products of e4m3 operands (the fp8 filter's arithmetic)."""
    q, d = _fp8_operands(queries, docs)
    out = torch.empty((q.shape[0], d.shape[0]), dtype=torch.float32, device=q.device)
    _lib.call("irc_scan_scores_fp8", ptr(q), ptr(d), q.shape[0], d.shape[0], q.shape[1],
              ptr(out), stream_ptr(q.device))
    return out


def set_single_pass_min_q(q: int) -> int:
    """Smallest query batch of the single-pass GEMM filter (irc_scan_set_ppl_min_q:
    Q in [q, 256]; q > 256 selects the sampled-threshold pipeline).  Both are exact.
    Returns the previous value."""
    return int(_lib.load().irc_scan_set_ppl_min_q(int(q)))


SCAN_SAMPLES = ("none", "tile", "gemm")  # irc.h: IRC_SCAN_SAMPLE_*
SCAN_FILTERS = ("tile_lists", "gemm_lists", "gemm_keys", "tile_keys")  # IRC_SCAN_FILTER_*


def scan_pipeline(Q: int, N: int, D: int, k: int, dtype: str = "bf16"):
    """(sample, filter, chunk_docs): the passes ``scan_topk`` (dtype "e4m3": ``scan_topk_fp8``)
    runs for the shape under the current knobs, by name (irc_scan_topk_pipeline; tests /
    diagnostics).  chunk_docs = N, or the chunk size where the shard is scanned in chunks;
    the pair describes one chunk.  Host arithmetic only: no device is accessed."""
    import ctypes

    if dtype not in ("bf16", "e4m3"):
        raise ValueError(f"scan_pipeline: dtype {dtype!r} is neither 'bf16' nor 'e4m3'")
    s, f, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    _lib.call("irc_scan_topk_pipeline", Q, N, D, k, int(dtype == "e4m3"), ctypes.addressof(s),
              ctypes.addressof(f), ctypes.addressof(c))
    return SCAN_SAMPLES[s.value], SCAN_FILTERS[f.value], int(c.value)


def rescan_stats(reset: bool = True):
    """(queries whose single-pass select rescanned, workers rescanned) since the
    last reset -- synchronises the device (tests / diagnostics)."""
    import ctypes

    out = (ctypes.c_uint64 * 2)()
    _lib.call("irc_scan_rescan_stats", ctypes.addressof(out), 1 if reset else 0)
    return int(out[0]), int(out[1])


def topk_merge(scores: torch.Tensor, idx: torch.Tensor, k: int):
    """Merge [P, Q, kin] per-shard lists into [Q, k] with the exact rule."""
    require_hip(scores, idx)
    s = contig(scores, torch.float32)
    i = contig(idx, torch.int64)
    P, Q, kin = s.shape
    out_s = torch.empty((Q, k), dtype=torch.float32, device=s.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=s.device)
    _lib.call("irc_topk_merge", ptr(s), ptr(i), P, Q, kin, k, ptr(out_s), ptr(out_i),
              stream_ptr(s.device))
    return out_s, out_i


def topk_merge_grouped(scores: torch.Tensor, idx: torch.Tensor, k: int,
                       group_off: torch.Tensor, ws_tag: str = "merge"):
    """Merge [P, Q, kin] per-shard GROUPED lists (``rerank_topk(..., group_off=)`` of P
    shards) into the top-k distinct groups of the whole corpus (irc_topk_merge_grouped): of
    the entries of one group -- its best row in each shard that returned it -- the best one
    stays, equal scores keeping the lower row id.  ``idx`` holds global row ids, -1 in empty
    slots; ``group_off`` as for ``rerank_topk``; P * kin <= 8192.  Returns (scores [Q, k],
    idx [Q, k], n int32 [Q], groups int64 [Q, k]) as the grouped ``rerank_topk`` does."""
    if group_off is None:
        raise TypeError("group_off must be an int64 tensor, not None")
    _check_group_off(group_off, scores)
    require_hip(scores, idx, group_off)
    s = contig(scores, torch.float32)
    i = contig(idx, torch.int64)
    if s.dim() != 3 or i.shape != s.shape:
        raise ValueError(f"scores and idx must both be [P, Q, kin], not {tuple(s.shape)} and "
                         f"{tuple(i.shape)}")
    P, Q, kin = s.shape
    go = group_off.contiguous()
    out_s = torch.empty((Q, k), dtype=torch.float32, device=s.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=s.device)
    out_n = torch.empty((Q,), dtype=torch.int32, device=s.device)
    nbytes = int(_lib.fn("irc_topk_merge_grouped_workspace")(P, Q, kin))
    ws = workspace(nbytes, s.device, ws_tag)
    _lib.call("irc_topk_merge_grouped", ptr(s), ptr(i), P, Q, kin, k, ptr(go), go.numel() - 1,
              ptr(ws), ws.numel(), ptr(out_s), ptr(out_i), ptr(out_n), stream_ptr(s.device))
    return out_s, out_i, out_n, _groups_of(go, out_i)


def _groups_of(group_off, idx):
    """The group of every returned row (each lies in [group_off[0], group_off[-1])); -1 in
    padded slots."""
    groups = torch.searchsorted(group_off, idx, right=True) - 1
    return torch.where(idx < 0, groups.new_full((), -1), groups)


def __getattr__(name):
    # RERANK_CHUNK: the candidates one scoring workgroup of irc_rerank_topk takes, read from
    # the library (irc_rerank_chunk(), RR_CHUNK in csrc/rerank.hip) so it cannot drift; the
    # list lengths around it are the kernel's edge cases.
    if name == "RERANK_CHUNK":
        return int(_lib.load().irc_rerank_chunk())
    # RERANK_STREAM_TILE: the doc-tile width of irc_rerank_topk_stream
    # (irc_rerank_stream_tile(), gpp::PICK_TILE in csrc/gemm_pp.h), read the same way.
    if name == "RERANK_STREAM_TILE":
        return int(_lib.load().irc_rerank_stream_tile())
    # IVF_TILE_ROWS: the rows of one work item's segment in irc_ivf_topk (irc_ivf_tile_rows(),
    # IVF_TILE_ROWS in csrc/ivf.hip); the list lengths around it are that kernel's edge cases.
    if name == "IVF_TILE_ROWS":
        return int(_lib.load().irc_ivf_tile_rows())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


RERANK_METHODS = ("gather", "stream")

# Candidates per query, as a fraction of the shard, from which method="stream" is the
# faster call, per query count Q: the gather-against-stream ``crossover_frac`` of
# profiles/rerank_stream_probe.json (tools/rerank_probe.py; one MI355X, 250k x 768 shard,
# k = 100).  None: gather was faster in every measured cell of that Q (up to 25 %).
_STREAM_CROSSOVER = ((1, None), (16, 0.15634670821855476), (64, 0.03685017313384864),
                     (256, 0.010609454861342326))
_STREAM_MIN_TILES = 4  # below this many doc tiles the shard is too small to matter
# The same for e4m3 shards (rerank_topk_fp8): the ``crossover_frac_stream`` of
# profiles/rerank_fp8_probe.json (tools/rerank_probe.py --dtype fp8; the same shard as e4m3).
_STREAM_CROSSOVER_FP8 = ((1, None), (16, 0.24292551185132844), (64, 0.05971435860633441),
                         (256, 0.015683947640214146))


def rerank_method(Q: int, N: int, D: int, n_cand: int, dtype: str = "bf16") -> str:
    """"gather" or "stream": the faster scoring method of ``rerank_topk`` for Q queries
    with n_cand candidates in all against a shard of N docs (pure host arithmetic, no
    device access).  "stream" once the mean list length n_cand / Q reaches the measured
    crossover fraction of the shard for that Q -- the ``crossover_frac`` entries of
    profiles/rerank_stream_probe.json, interpolated log-log between the measured Q = 1,
    16, 64, 256 and held constant beyond them; where gather won every measured cell of a
    Q (Q = 1), and between such a Q and the next measured one, the answer is "gather".  A shard below 4 doc tiles (RERANK_STREAM_TILE docs each) is
    always gathered.  The crossovers were measured at D = 768; both methods' scoring cost
    is proportional to D, so D does not enter.  Monotone in n_cand.

    ``dtype="fp8"``: the choice for ``rerank_topk_fp8``, by the same rule on its own
    table (profiles/rerank_fp8_probe.json); "gather" wherever the e4m3 stream kernel does
    not run (D % 128 != 0)."""
    import math

    if dtype not in ("bf16", "fp8"):
        raise ValueError(f"dtype must be 'bf16' or 'fp8', not {dtype!r}")
    if Q <= 0 or n_cand <= 0 or N < _STREAM_MIN_TILES * 256:
        return "gather"
    if dtype == "fp8" and D % 128 != 0:
        return "gather"
    pts = _STREAM_CROSSOVER_FP8 if dtype == "fp8" else _STREAM_CROSSOVER
    if Q <= pts[0][0]:
        frac = pts[0][1]
    elif Q >= pts[-1][0]:
        frac = pts[-1][1]
    else:
        frac = None
        for (qa, fa), (qb, fb) in zip(pts, pts[1:]):
            if qa <= Q <= qb:
                if Q == qa:
                    frac = fa
                elif Q == qb:
                    frac = fb
                elif fa is not None and fb is not None:
                    t = (math.log(Q) - math.log(qa)) / (math.log(qb) - math.log(qa))
                    frac = math.exp(math.log(fa) + t * (math.log(fb) - math.log(fa)))
                break
    if frac is None:
        return "gather"
    return "stream" if n_cand >= frac * N * Q else "gather"


def _sort_lists(cand: torch.Tensor, cand_off: torch.Tensor, with_perm: bool = False):
    """Every list of the CSR pair ascending, in one device sort of (owner, id) pairs; no
    host synchronisation.  cand int32 / int64 with values in [-2^31, 2^31).  With
    ``with_perm`` also the permutation: ``(sorted, perm)`` with ``sorted[j]`` the id that
    stood at flat place ``perm[j]``, so whatever travels with a candidate (its bias) is
    ``x[perm]``."""
    n = cand.numel()
    Q = cand_off.numel() - 1
    lengths = cand_off[1:] - cand_off[:-1]
    owner = torch.repeat_interleave(torch.arange(Q, device=cand.device), lengths, output_size=n)
    key = (owner << 32) + (cand.to(torch.int64) + 2 ** 31)
    key, perm = torch.sort(key)
    ids = ((key & 0xFFFFFFFF) - 2 ** 31).to(torch.int32)
    return (ids, perm) if with_perm else ids


def _check_bias(bias, cand, queries):
    """The ``bias`` argument of the rerank calls, checked before anything touches the device:
    fp32, one entry per candidate, on the queries' device."""
    if bias is None:
        return
    if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32:
        raise TypeError("bias must be a float32 tensor, not "
                        f"{getattr(bias, 'dtype', type(bias))}")
    if bias.numel() != cand.numel():
        raise ValueError(f"bias has {bias.numel()} entries for {cand.numel()} candidates")
    if bias.device != queries.device:
        raise ValueError(f"bias is on {bias.device}, the queries on {queries.device}")


RERANK_FLAG_STREAM = 1  # irc.h: IRC_RERANK_STREAM
RERANK_FLAG_E4M3 = 2  # irc.h: IRC_RERANK_E4M3


def _check_group_off(group_off, queries):
    """The ``group_off`` argument of the rerank calls, checked before anything else runs:
    1-D int64 with at least one entry, on the queries' device."""
    if group_off is None:
        return
    if not isinstance(group_off, torch.Tensor) or group_off.dtype != torch.int64:
        raise TypeError("group_off must be an int64 tensor, not "
                        f"{getattr(group_off, 'dtype', type(group_off))}")
    if group_off.dim() != 1 or group_off.numel() < 1:
        raise ValueError("group_off must be 1-D with n_groups + 1 >= 1 entries, not shape "
                         f"{tuple(group_off.shape)}")
    if group_off.device != queries.device:
        raise ValueError(f"group_off is on {group_off.device}, the queries on {queries.device}")


def scan_topk_grouped(queries: torch.Tensor, docs: torch.Tensor, k: int, group_off,
                      doc_offset: int = 0, ws_tag: str = "scan_group",
                      max_workspace_bytes: int = 1 << 30):
    """The dense scan per group of rows (irc_scan_topk_grouped): each query's top-k distinct
    groups of the WHOLE shard, each by its best row -- what ``rerank_topk(method="stream",
    group_off=...)`` returns when every row is a candidate of every query, bit for bit, with
    no candidate list: the GEMM loop's epilogue folds each score tile into one key per (query,
    group).

    queries [Q, D], docs [N, D] (one shard, first global id ``doc_offset``), bf16 on one HIP
    device; ``group_off`` int64 [n_groups + 1] on that device, non-decreasing, in GLOBAL row
    ids, as for ``rerank_topk``: a group may begin before the shard or end past it (only its
    rows here count; ``topk_merge_grouped`` joins the halves of two shards), and shard rows
    outside [group_off[0], group_off[-1]) are never returned.  Returns (scores fp32 [Q, k],
    idx int64 [Q, k] global row ids, n int32 [Q], groups int64 [Q, k]) as the grouped
    ``rerank_topk`` does: by (score desc, row id asc), ties within a group to the lower id,
    n[q] = min(k, groups with a row in the shard), padding (-inf, -1, group -1).  Exact.

    The workspace holds 8 bytes per (query, group); when that exceeds
    ``max_workspace_bytes`` the batch runs in chunks of a multiple of 256 queries (at least
    256) and the results are concatenated -- the shard streams once per 256-query tile
    anyway, so chunking reads no more."""
    if group_off is None:
        raise TypeError("group_off must be an int64 tensor, not None")
    _check_group_off(group_off, queries)
    require_hip(queries, docs, group_off)
    q = contig(queries, torch.bfloat16)
    d = contig(docs, torch.bfloat16)
    if d.shape[1] != q.shape[1]:
        raise ValueError(f"dim mismatch: queries D={q.shape[1]}, docs D={d.shape[1]}")
    return _scan_group_call(q, d, k, group_off, doc_offset, 1.0, ws_tag, max_workspace_bytes)


def scan_topk_grouped_fp8(queries: torch.Tensor, docs: torch.Tensor, k: int, group_off,
                          doc_offset: int = 0, score_scale: float = 1.0,
                          ws_tag: str = "scan_group", max_workspace_bytes: int = 1 << 30):
    """``scan_topk_grouped`` over e4m3 operands: queries [Q, D] and docs [N, D] are uint8 codes
    (``quantize_fp8``), D % 128 == 0.  The scores are the fp32 dot products of the decoded
    values times ``score_scale`` (a power of two), as ``scan_topk_fp8`` reports them."""
    if group_off is None:
        raise TypeError("group_off must be an int64 tensor, not None")
    _check_group_off(group_off, queries)
    _require_e4m3(queries, docs)  # a wrong dtype is a TypeError on any device
    q, d = _fp8_operands(queries, docs)
    require_hip(group_off)
    return _scan_group_call(q, d, k, group_off, doc_offset, float(score_scale), ws_tag,
                            max_workspace_bytes)


def _scan_group_call(q, d, k, group_off, doc_offset, score_scale, ws_tag, max_workspace_bytes):
    """The part of ``scan_topk_grouped`` and ``scan_topk_grouped_fp8`` after their operand
    checks: the query chunks, the outputs and the native call (uint8 operands: e4m3)."""
    Q, D = q.shape
    N = d.shape[0]
    go = group_off.contiguous()
    n_groups = go.numel() - 1
    flags = RERANK_FLAG_E4M3 if q.dtype == torch.uint8 else 0
    out_s = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=q.device)
    out_n = torch.empty((Q,), dtype=torch.int32, device=q.device)
    chunk = max(Q, 1)
    if Q * n_groups * 8 > max_workspace_bytes:
        chunk = max(256, max_workspace_bytes // (8 * n_groups) // 256 * 256)
    for lo in range(0, Q, chunk):
        hi = min(Q, lo + chunk)
        nbytes = int(_lib.fn("irc_scan_topk_grouped_workspace")(hi - lo, n_groups, k))
        ws = workspace(nbytes, q.device, ws_tag)
        _lib.call("irc_scan_topk_grouped", ptr(q[lo:hi]), ptr(d), hi - lo, N, D, k, doc_offset,
                  ptr(go), n_groups, flags, score_scale, ptr(ws), ws.numel(),
                  ptr(out_s[lo:hi]), ptr(out_i[lo:hi]), ptr(out_n[lo:hi]), stream_ptr(q.device))
    return out_s, out_i, out_n, _groups_of(go, out_i)


def local_group_slice(group_off: torch.Tensor, doc_offset: int, N: int):
    """(g_lo, g_hi): the groups a shard of N rows from global id ``doc_offset`` can touch are
    ``group_off[g_lo : g_hi + 1]`` -- g_lo the number of g with group_off[g + 1] <= doc_offset
    (groups that end at or before the shard), g_hi the number of g with group_off[g] <
    doc_offset + N (groups that begin before its end).  g_hi <= g_lo: the slice is empty.
    Pure torch on the tensor's device (CPU tensors too); reading the two counts is one
    synchronisation."""
    go = group_off.reshape(-1).to(torch.int64)
    both = torch.stack([(go[1:] <= doc_offset).sum(), (go[:-1] < doc_offset + N).sum()])
    g_lo, g_hi = both.tolist()
    return int(g_lo), int(g_hi)


def rerank_topk(queries: torch.Tensor, docs: torch.Tensor, cand: torch.Tensor,
                cand_off: torch.Tensor, k: int, doc_offset: int = 0, ws_tag: str = "rerank",
                method: str = "gather", ascending: bool = False, group_off=None, bias=None):
    """Exact top-k of each query over ITS OWN candidate docs (sparse filter, dense rerank:
    src/evaluation.py:57-83 feeding :110-112).

    queries [Q, D], docs [N, D] (one shard, first global id ``doc_offset``), bf16 on one
    HIP device.  ``cand`` (int32 or int64) holds global doc ids, query q owning
    ``cand[cand_off[q]:cand_off[q + 1]]`` (``cand_off`` int64 [Q + 1]); ids are unique
    within a list, in any order; ids outside the shard are skipped (an int64 id that does
    not fit int32 is in no shard and is skipped too, never wrapped).  Returns (scores fp32
    [Q, k], idx int64 [Q, k], n int32 [Q]): each list by (score desc, id asc), slots past
    n[q] = min(k, eligible) are (-inf, -1).

    ``method="gather"`` (irc_rerank_topk) reads each candidate row once per (query,
    candidate); ``method="stream"`` (irc_rerank_topk_stream) streams the shard once per
    256-query tile through the MFMA GEMM loop and picks the candidates' scores out of the
    score tiles -- the faster one for dense lists (``rerank_method``).  Same exact ranking
    rule; a score may differ in its last bits between the two (another fp32 summation
    order, each fixed per (query, doc)).  The stream kernel needs every list ASCENDING in
    global id: ``ascending=True`` states that they are (``SparseIndex.candidates`` and
    ``expand_ranges`` leave them so); otherwise they are sorted on the device first (one
    ``torch.sort``, no host synchronisation) and the result is the same.  Under "stream"
    an int64 id outside int32 is clamped to -1 / 2^31 - 1, which no shard owns, so an
    ascending list stays ascending.

    ``group_off`` (int64 [n_groups + 1] on the queries' device, non-decreasing, in GLOBAL
    row ids whatever ``doc_offset``): the top-k per group instead of per row
    (irc_rerank_topk_grouped).  Group g owns the rows [group_off[g], group_off[g + 1]);
    each query's candidates collapse to the best row of every group -- equal scores keep
    the lower id -- and the call returns (scores, idx, n, groups): the top-k distinct
    groups, each by its best row, n[q] = min(k, groups with an eligible row), and groups
    int64 [Q, k] the group of each returned row (-1 in padded slots).  A row outside
    [group_off[0], group_off[-1]) is in no group and never returned.  The collapse needs
    ascending lists under both methods, so without ``ascending=True`` the lists are sorted
    first under "gather" too.  It happens inside this one shard; the grouped results of
    several shards merge with ``topk_merge_grouped``, which keeps one row of a group whose
    rows lie in two shards.  With ``group_off=None`` nothing changes.

    ``bias`` (fp32, ``cand.numel()`` entries on the queries' device, parallel to ``cand``):
    the fused score of hybrid retrieval (irc_rerank_biased_topk).  Candidate i is ranked by,
    and returned with, ``score_i + bias[i]`` -- one fp32 addition to exactly the score the
    call without ``bias`` computes under the same method; any weight is the caller's to
    multiply in.  ``bias[i]`` belongs to the i-th entry of ``cand`` as passed, eligible or
    not: it follows its candidate through the sort of unsorted lists.  With ``group_off``
    the bias is added before the collapse, so a group is represented by the row with the
    best fused score.  The values are not checked: a non-finite sum ranks as the keys order
    it (+inf first, -inf after every finite value, NaN last).  ``bias=None`` is the call as
    it was."""
    if method not in RERANK_METHODS:
        raise ValueError(f"method must be one of {RERANK_METHODS}, not {method!r}")
    _check_group_off(group_off, queries)
    _check_bias(bias, cand, queries)
    require_hip(queries, docs, cand, cand_off)
    q = contig(queries, torch.bfloat16)
    d = contig(docs, torch.bfloat16)
    if d.shape[1] != q.shape[1]:
        raise ValueError(f"dim mismatch: queries D={q.shape[1]}, docs D={d.shape[1]}")
    return _rerank_call(q, d, cand, cand_off, k, doc_offset, 1.0, ws_tag, method, ascending,
                        group_off, bias)


# (method, e4m3 operands) -> the ungrouped native entry and the grouped entry's flags word
_RERANK_FORMS = {
    ("gather", False): ("irc_rerank_topk", 0),
    ("stream", False): ("irc_rerank_topk_stream", RERANK_FLAG_STREAM),
    ("gather", True): ("irc_rerank_topk_fp8", RERANK_FLAG_E4M3),
    ("stream", True): ("irc_rerank_topk_stream_fp8", RERANK_FLAG_STREAM | RERANK_FLAG_E4M3),
}


def _rerank_call(q, d, cand, cand_off, k, doc_offset, score_scale, ws_tag, method, ascending,
                 group_off=None, bias=None):
    """The part of ``rerank_topk`` and ``rerank_topk_fp8`` after their operand checks: the
    id handling, the sort under "stream", the outputs and the native call.  The operands'
    dtype (uint8: e4m3 codes) and ``method`` choose the entry, or with ``group_off`` the
    flags word of the one grouped entry; ``score_scale`` counts for e4m3 operands only.
    With ``bias`` the one biased entry runs, by the same flags word, grouped or not; the
    clamp / -1 replacement of int64 ids moves no candidate, and the sort's permutation is
    applied to the bias."""
    Q, D = q.shape
    N = d.shape[0]
    grouped = group_off is not None
    e4m3 = q.dtype == torch.uint8
    entry, flags = _RERANK_FORMS[method, e4m3]
    ordered = grouped or method == "stream"  # the kernels need ascending lists
    if cand.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"cand must be int32 or int64, not {cand.dtype}")
    if cand_off.numel() != Q + 1:
        raise ValueError(f"cand_off has {cand_off.numel()} entries for {Q} queries (Q + 1)")
    if cand.dtype == torch.int64:
        # an id outside int32 is in no shard (doc_offset + N < 2^31): it must not wrap into one
        if ordered:  # order-preserving
            cand = cand.clamp(-1, 2 ** 31 - 1)
        else:
            cand = torch.where((cand < 0) | (cand >= 2 ** 31), cand.new_full((), -1), cand)
    off = contig(cand_off, torch.int64)
    if bias is not None:
        bias = bias.reshape(-1)
        if ordered and not ascending:
            cand, perm = _sort_lists(cand.reshape(-1), off, with_perm=True)
            bias = bias[perm]
    elif ordered and not ascending:
        cand = _sort_lists(cand.reshape(-1), off)
    c = contig(cand, torch.int32)
    n_cand = c.numel()
    out_s = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=q.device)
    out_n = torch.empty((Q,), dtype=torch.int32, device=q.device)
    if bias is not None:
        b = contig(bias, torch.float32)
        go = group_off.contiguous() if grouped else None
        ws_fn = "irc_rerank_topk_grouped_workspace" if grouped else "irc_rerank_topk_workspace"
        ws = workspace(int(_lib.fn(ws_fn)(Q, n_cand, k)), q.device, ws_tag)
        _lib.call("irc_rerank_biased_topk", ptr(q), ptr(d), Q, N, D, ptr(c), ptr(off), n_cand,
                  k, doc_offset, ptr(go) if grouped else None, go.numel() - 1 if grouped else 0,
                  flags, score_scale, ptr(b), ptr(ws), ws.numel(), ptr(out_s), ptr(out_i),
                  ptr(out_n), stream_ptr(q.device))
        if grouped:
            return out_s, out_i, out_n, _groups_of(go, out_i)
        return out_s, out_i, out_n
    if not grouped:  # 8 bytes of workspace per candidate, against 24 for the grouped entry
        nbytes = int(_lib.fn("irc_rerank_topk_workspace")(Q, n_cand, k))
        ws = workspace(nbytes, q.device, ws_tag)
        _lib.call(entry, ptr(q), ptr(d), Q, N, D, ptr(c), ptr(off), n_cand, k,
                  doc_offset, *((score_scale,) if e4m3 else ()), ptr(ws), ws.numel(),
                  ptr(out_s), ptr(out_i), ptr(out_n), stream_ptr(q.device))
        return out_s, out_i, out_n
    go = group_off.contiguous()
    n_groups = go.numel() - 1
    nbytes = int(_lib.fn("irc_rerank_topk_grouped_workspace")(Q, n_cand, k))
    ws = workspace(nbytes, q.device, ws_tag)
    _lib.call("irc_rerank_topk_grouped", ptr(q), ptr(d), Q, N, D, ptr(c), ptr(off), n_cand, k,
              doc_offset, ptr(go), n_groups, flags, score_scale, ptr(ws), ws.numel(),
              ptr(out_s), ptr(out_i), ptr(out_n), stream_ptr(q.device))
    return out_s, out_i, out_n, _groups_of(go, out_i)


def rerank_topk_fp8(queries: torch.Tensor, docs: torch.Tensor, cand: torch.Tensor,
                    cand_off: torch.Tensor, k: int, doc_offset: int = 0,
                    score_scale: float = 1.0, ws_tag: str = "rerank", method: str = "gather",
                    ascending: bool = False, group_off=None, bias=None):
    """``rerank_topk`` over e4m3 operands: queries [Q, D] and docs [N, D] are uint8 codes
    (``quantize_fp8``).  The scores are the fp32 dot products of the decoded values times
    ``score_scale`` (a power of two), as ``scan_topk_fp8`` reports them; candidates, ids,
    ``method``, ``ascending``, ``group_off``, ``bias`` and the outputs are ``rerank_topk``'s
    (the bias is added to the score AFTER ``score_scale``).  "gather"
    is irc_rerank_topk_fp8, "stream" irc_rerank_topk_stream_fp8 (D % 128 == 0); on values
    whose sums are exact in fp32 the two agree bitwise."""
    if method not in RERANK_METHODS:
        raise ValueError(f"method must be one of {RERANK_METHODS}, not {method!r}")
    _check_group_off(group_off, queries)
    _check_bias(bias, cand, queries)
    _require_e4m3(queries, docs)  # a wrong dtype is a TypeError on any device
    q, d = _fp8_operands(queries, docs)
    require_hip(cand, cand_off)
    return _rerank_call(q, d, cand, cand_off, k, doc_offset, float(score_scale), ws_tag, method,
                        ascending, group_off, bias)


def expand_ranges(cand: torch.Tensor, cand_off: torch.Tensor, row_off: torch.Tensor,
                  values=None):
    """Candidate columns -> candidate rows: each candidate c of the CSR pair (cand,
    cand_off) becomes the row range [row_off[c], row_off[c + 1]) (empty ranges vanish) and
    the offsets are rebuilt.  Returns (rows int64, rows_off int64 [Q + 1]); lists that
    were ascending and unique stay so (row_off is non-decreasing).  Pure torch on the
    tensors' device; the one host synchronisation is the total row count.

    ``values`` ([n_cand], any dtype, parallel to ``cand``): a third result, ``values`` of
    each row's candidate -- every row carries its page's value (the ``bias`` of
    ``rerank_topk`` over the rows).  Without it the return is the pair."""
    if values is not None and values.numel() != cand.numel():
        raise ValueError(f"values has {values.numel()} entries for {cand.numel()} candidates")
    c = cand.to(torch.int64)
    off = cand_off.to(torch.int64)
    ro = row_off.to(device=c.device, dtype=torch.int64)
    start = ro[c]
    length = ro[c + 1] - start
    ends = torch.cumsum(length, 0)  # flat end of every candidate's rows
    zero = torch.zeros(1, dtype=torch.int64, device=c.device)
    rows_off = torch.cat([zero, ends])[off]
    total = int(ends[-1].item()) if c.numel() else 0
    owner = torch.repeat_interleave(torch.arange(c.numel(), device=c.device), length,
                                    output_size=total)
    rows = start[owner] + (torch.arange(total, device=c.device) - (ends - length)[owner])
    if values is not None:
        return rows, rows_off, values.reshape(-1).to(c.device)[owner]
    return rows, rows_off


IVF_CHUNK = 32  # queries one pass over a probed list serves: the MFMA's columns (csrc/ivf.hip)


def ivf_layout(assign: torch.Tensor, nlist: int):
    """The list order of a clustered corpus: (order int64 [N], list_off int64 [nlist + 1]).
    ``order`` is the stable sort of the rows by their list ``assign`` (values in [0, nlist)),
    so original ids ascend inside a list; list c is ``order[list_off[c]:list_off[c + 1]]``.
    Empty lists are allowed.  Pure torch on the tensor's device (CPU tensors too)."""
    a = assign.reshape(-1).to(torch.int64)
    sa, order = torch.sort(a, stable=True)
    list_off = torch.searchsorted(sa, torch.arange(nlist + 1, dtype=torch.int64, device=a.device))
    return order, list_off


def ivf_plan(probe: torch.Tensor, list_off: torch.Tensor):
    """The index plumbing of one ``ivf_topk`` call, from ``probe`` (int32 [Q, nprobe]: list ids,
    unique within a row, -1 = no list, skipped) and ``list_off``.  Pure torch on the tensors'
    device (CPU tensors too), no host synchronisation.  Returns a dict of

    * ``slot_off`` int64 [Q * nprobe + 1]: pair (q, j) owns the keys
      ``[slot_off[q * nprobe + j], + len(list))``;
    * ``cand_off`` int64 [Q + 1] = ``slot_off[::nprobe]``: a query's keys are one stretch;
    * ``pair_order`` int32 [Q * nprobe]: the valid pairs, stable-sorted by list id (the -1
      pairs fill the tail past ``seg_off[-1]``, so the length is known without a sync);
    * ``seg_off`` int64 [nlist + 1]: list c's pairs are ``pair_order[seg_off[c]:seg_off[c + 1]]``;
    * ``chunk_off`` int64 [nlist + 1]: the cumulative count of chunks of ``IVF_CHUNK`` pairs per
      list -- one chunk's queries share one pass over the list."""
    Q, nprobe = probe.shape
    lo = list_off.reshape(-1).to(torch.int64)
    nlist = lo.numel() - 1
    dev = probe.device
    flat = probe.reshape(-1).to(torch.int64)
    valid = (flat >= 0) & (flat < nlist)  # an id that names no list owns no keys either
    lens = lo[1:] - lo[:-1]
    plen = torch.where(valid, lens[flat.clamp(0, max(nlist - 1, 0))], lens.new_zeros(()))
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    slot_off = torch.cat([zero, torch.cumsum(plen, 0)])
    cand_off = slot_off[::nprobe].contiguous()
    key = torch.where(valid, flat, flat.new_full((), nlist))
    skey, pair_order = torch.sort(key, stable=True)
    seg_off = torch.searchsorted(skey, torch.arange(nlist + 1, dtype=torch.int64, device=dev))
    chunks = (seg_off[1:] - seg_off[:-1] + (IVF_CHUNK - 1)) // IVF_CHUNK
    chunk_off = torch.cat([zero, torch.cumsum(chunks, 0)])
    return {"slot_off": slot_off, "cand_off": cand_off, "pair_order": pair_order.to(torch.int32),
            "seg_off": seg_off, "chunk_off": chunk_off}


def ivf_topk(queries: torch.Tensor, docs: torch.Tensor, row_id: torch.Tensor,
             list_off: torch.Tensor, probe: torch.Tensor, k: int, max_list_rows: int,
             ws_tag: str = "ivf", total_rows=None):
    """Exact top-k of each query over the rows of the lists it probes (irc_ivf_topk).

    queries [Q, D] bf16; ``docs`` [N, D] bf16 IN LIST ORDER (``ivf_layout``), ``row_id`` int32
    [N] the global id of each row, ``list_off`` int64 [nlist + 1]; ``probe`` int32 [Q, nprobe]
    (``ivf_plan``); all on one HIP device.  ``max_list_rows`` is a host int, the longest list
    (it bounds the grid).  Returns (scores fp32 [Q, k], idx int64 [Q, k] global ids, n int32
    [Q]) by (score desc, global id asc); slots past n[q] = min(k, rows in the probed lists) are
    (-inf, -1).  Each probed list is read once per 32 of the queries that probe it and scored
    on MFMA; the fp32 sum of a (query, row) has one fixed order whatever else the call holds.

    The workspace holds one key per (pair, row).  Their total is read from the plan with ONE
    host synchronisation, as ``expand_ranges`` reads its row count, unless the caller passes
    ``total_rows`` (an upper bound), which keeps the call stream-ordered."""
    return _ivf_topk_call(queries, docs, row_id, list_off, probe, k, max_list_rows, ws_tag,
                          total_rows, None)


def ivf_topk_fp8(queries: torch.Tensor, docs: torch.Tensor, row_id: torch.Tensor,
                 list_off: torch.Tensor, probe: torch.Tensor, k: int, max_list_rows: int,
                 score_scale: float = 1.0, ws_tag: str = "ivf", total_rows=None):
    """``ivf_topk`` over e4m3 lists (irc_ivf_topk_fp8): queries [Q, D] and ``docs`` [N, D] (in
    list order) are e4m3 bytes (uint8, see ``quantize_fp8``), everything else as there.  The
    scores are the fp32 sums of the decoded codes' products times ``score_scale`` (a power of
    two), one fixed order per (query, row)."""
    _require_e4m3(queries, docs)  # a wrong dtype is a TypeError on any device
    return _ivf_topk_call(queries, docs, row_id, list_off, probe, k, max_list_rows, ws_tag,
                          total_rows, float(score_scale))


def _ivf_topk_call(queries, docs, row_id, list_off, probe, k, max_list_rows, ws_tag, total_rows,
                   score_scale):
    """``ivf_topk`` (score_scale None: bf16 operands) and ``ivf_topk_fp8`` in one path."""
    require_hip(queries, docs, row_id, list_off, probe)
    elem = torch.bfloat16 if score_scale is None else torch.uint8
    q = contig(queries, elem)
    d = contig(docs, elem)
    if d.shape[1] != q.shape[1]:
        raise ValueError(f"dim mismatch: queries D={q.shape[1]}, docs D={d.shape[1]}")
    if probe.dim() != 2 or probe.shape[0] != q.shape[0]:
        raise ValueError(f"probe must be [Q, nprobe] for {q.shape[0]} queries, not "
                         f"{tuple(probe.shape)}")
    if row_id.numel() != d.shape[0]:
        raise ValueError(f"row_id has {row_id.numel()} entries for {d.shape[0]} rows")
    Q, D = q.shape
    N = d.shape[0]
    nprobe = probe.shape[1]
    pr = contig(probe, torch.int32)
    rid = contig(row_id, torch.int32)
    lo = contig(list_off, torch.int64)
    plan = ivf_plan(pr, lo)
    if total_rows is None:
        total_rows = int(plan["slot_off"][-1].item())
    out_s = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=q.device)
    out_n = torch.empty((Q,), dtype=torch.int32, device=q.device)
    nbytes = int(_lib.fn("irc_ivf_topk_workspace")(Q, nprobe, int(total_rows), k))
    ws = workspace(nbytes, q.device, ws_tag)
    scale = () if score_scale is None else (score_scale,)
    _lib.call("irc_ivf_topk" if score_scale is None else "irc_ivf_topk_fp8", ptr(q), ptr(d),
              ptr(rid), ptr(lo), lo.numel() - 1, ptr(pr), ptr(plan["slot_off"]),
              ptr(plan["cand_off"]), ptr(plan["pair_order"]), ptr(plan["seg_off"]),
              ptr(plan["chunk_off"]), Q, nprobe, N, D, k, int(total_rows), int(max_list_rows),
              *scale, ptr(ws), ws.numel(), ptr(out_s), ptr(out_i), ptr(out_n),
              stream_ptr(q.device))
    return out_s, out_i, out_n


def ivf_plan_native(probe: torch.Tensor, list_off: torch.Tensor, ws_tag: str = "ivf_plan"):
    """``ivf_plan`` built by the library's kernels (irc_ivf_plan): the same dict, elementwise
    equal for every probe with unique rows, in a handful of launches with no sort and no host
    synchronisation.  ``probe`` [Q, nprobe] int32 or int64 (``scan_topk``'s ids as they are),
    ``list_off`` [nlist + 1]; both on one HIP device.  ``ivf_plan`` stays the documented form
    of the plan and the oracle of this one."""
    if probe.dim() != 2:
        raise ValueError(f"probe must be [Q, nprobe], not {tuple(probe.shape)}")
    if probe.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"probe must be int32 or int64, not {probe.dtype}")
    if list_off.dim() != 1 or list_off.numel() < 1:
        raise ValueError(f"list_off must be [nlist + 1], not {tuple(list_off.shape)}")
    require_hip(probe, list_off)
    pr = probe.contiguous()
    lo = contig(list_off, torch.int64)
    Q, nprobe = pr.shape
    nlist = lo.numel() - 1
    dev = pr.device
    new = torch.empty if Q else torch.zeros  # the call writes every element, or (Q == 0) none
    plan = {"slot_off": new(Q * nprobe + 1, dtype=torch.int64, device=dev),
            "cand_off": new(Q + 1, dtype=torch.int64, device=dev),
            "pair_order": new(Q * nprobe, dtype=torch.int32, device=dev),
            "seg_off": new(nlist + 1, dtype=torch.int64, device=dev),
            "chunk_off": new(nlist + 1, dtype=torch.int64, device=dev)}
    nbytes = int(_lib.fn("irc_ivf_plan_workspace")(Q, nprobe, nlist))
    ws = workspace(nbytes, dev, ws_tag)
    _lib.call("irc_ivf_plan", ptr(pr), int(pr.dtype == torch.int64), ptr(lo), Q, nprobe, nlist,
              ptr(ws), ws.numel(), ptr(plan["slot_off"]), ptr(plan["cand_off"]),
              ptr(plan["pair_order"]), ptr(plan["seg_off"]), ptr(plan["chunk_off"]),
              stream_ptr(dev))
    return plan


def ivf_search(queries: torch.Tensor, docs: torch.Tensor, row_id: torch.Tensor,
               list_off: torch.Tensor, k: int, key_rows: int, max_list_rows: int,
               centroids=None, nprobe=None, probe=None, ws_tag: str = "ivf", out=None,
               out_probe=None, ws=None):
    """A whole cluster-pruned search in one native call (irc_ivf_search): the probe
    (``scan_topk`` over ``centroids`` [nlist, D] with k = ``nprobe``) unless the caller's
    ``probe`` int32 [Q, nprobe] is given, the plan on the device, ``ivf_topk``'s scoring pass
    and select.  Stream-ordered: no host synchronisation and no torch op between them, so it
    can be captured in a graph.  Same arrays and result as ``ivf_topk``, bit for bit.

    ``key_rows`` is a host bound on the keys of the call, Q x (the sum of the nprobe longest
    lists) or more (``IVFDenseIndex.key_bound``).  ``out`` = (scores [Q, k] fp32, idx [Q, k]
    int64, n [Q] int32), contiguous, is written in place when given; ``out_probe`` int32
    [Q, nprobe] receives the probe that was used; ``ws`` is the caller's own workspace (uint8,
    at least irc_ivf_search_workspace bytes) instead of the cached one."""
    return _ivf_search_call(queries, docs, row_id, list_off, k, key_rows, max_list_rows,
                            centroids, nprobe, probe, ws_tag, out, out_probe, ws, None)


def ivf_search_fp8(queries: torch.Tensor, docs: torch.Tensor, row_id: torch.Tensor,
                   list_off: torch.Tensor, k: int, key_rows: int, max_list_rows: int,
                   centroids=None, nprobe=None, probe=None, query_scale: float = FP8_SCALE,
                   score_scale: float = 1.0 / (FP8_SCALE * FP8_SCALE), ws_tag: str = "ivf",
                   out=None, out_probe=None, ws=None):
    """``ivf_search`` over e4m3 lists in one native call (irc_ivf_search_fp8): ``queries``
    [Q, D] and ``centroids`` are bf16, ``docs`` [N, D] e4m3 bytes (uint8) in list order.  The
    probe is ``ivf_search``'s (bf16 queries over bf16 centroids), the queries are then
    quantised with ``query_scale`` on the same stream and the lists scored against the codes,
    the sums times ``score_scale`` (a power of two).  Same bits as ``ivf_topk_fp8`` of
    ``quantize_fp8(queries, query_scale)``; every other argument as for ``ivf_search`` (``ws``:
    at least irc_ivf_search_fp8_workspace bytes)."""
    _require_e4m3(docs)  # a wrong dtype is a TypeError on any device
    return _ivf_search_call(queries, docs, row_id, list_off, k, key_rows, max_list_rows,
                            centroids, nprobe, probe, ws_tag, out, out_probe, ws,
                            (float(query_scale), float(score_scale)))


def _ivf_search_call(queries, docs, row_id, list_off, k, key_rows, max_list_rows, centroids,
                     nprobe, probe, ws_tag, out, out_probe, ws, scales):
    """``ivf_search`` (scales None: bf16 lists) and ``ivf_search_fp8`` in one path."""
    if queries.dim() != 2 or docs.dim() != 2 or docs.shape[1] != queries.shape[1]:
        raise ValueError(f"dim mismatch: queries {tuple(queries.shape)}, docs "
                         f"{tuple(docs.shape)}")
    if (nprobe is None) == (probe is None):
        raise ValueError("give exactly one of nprobe and probe")
    Q, D = queries.shape
    N = docs.shape[0]
    nlist = list_off.numel() - 1
    if probe is not None:
        if probe.dim() != 2 or probe.shape[0] != Q:
            raise ValueError(f"probe must be [Q, nprobe] for {Q} queries, not "
                             f"{tuple(probe.shape)}")
        nprobe = probe.shape[1]
    elif centroids is None or centroids.dim() != 2 or tuple(centroids.shape) != (nlist, D):
        raise ValueError(f"centroids must be [nlist={nlist}, D={D}] to probe {nprobe} lists, "
                         f"not {None if centroids is None else tuple(centroids.shape)}")
    if row_id.numel() != N:
        raise ValueError(f"row_id has {row_id.numel()} entries for {N} rows")
    if out is not None and (tuple(out[0].shape) != (Q, k) or out[0].dtype != torch.float32 or
                            tuple(out[1].shape) != (Q, k) or out[1].dtype != torch.int64 or
                            tuple(out[2].shape) != (Q,) or out[2].dtype != torch.int32 or
                            not all(o.is_contiguous() for o in out)):
        raise ValueError(f"out must be contiguous fp32 [{Q}, {k}], int64 [{Q}, {k}], int32 [{Q}]")
    if out_probe is not None and (tuple(out_probe.shape) != (Q, nprobe) or
                                  out_probe.dtype != torch.int32 or
                                  not out_probe.is_contiguous()):
        raise ValueError(f"out_probe must be contiguous int32 [{Q}, {nprobe}]")
    require_hip(queries, docs, row_id, list_off, centroids, probe)
    q = contig(queries, torch.bfloat16)
    d = contig(docs, torch.bfloat16 if scales is None else torch.uint8)
    rid = contig(row_id, torch.int32)
    lo = contig(list_off, torch.int64)
    pr = None if probe is None else contig(probe, torch.int32)
    cen = None if probe is not None else contig(centroids, torch.bfloat16)
    if out is None:
        out = (torch.empty((Q, k), dtype=torch.float32, device=q.device),
               torch.empty((Q, k), dtype=torch.int64, device=q.device),
               torch.empty((Q,), dtype=torch.int32, device=q.device))
    entry = "irc_ivf_search" if scales is None else "irc_ivf_search_fp8"
    nbytes = int(_lib.fn(entry + "_workspace")(Q, nprobe, nlist, int(key_rows), k))
    if ws is None:
        ws = workspace(nbytes, q.device, ws_tag)
    _lib.call(entry, ptr(q), ptr(d), ptr(rid), ptr(lo), nlist, ptr(cen), ptr(pr), Q, nprobe, N,
              D, k, int(key_rows), int(max_list_rows), *(scales or ()), ptr(ws), ws.numel(),
              ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out_probe), stream_ptr(q.device))
    return out


def ivf_query_chunk(Q: int, max_bytes: int, nbytes_of) -> int:
    """The queries one ``ivf_search`` call of a batch of Q takes under a workspace limit: Q when
    ``nbytes_of(Q)`` (the workspace of a call of that many queries, non-decreasing) fits
    ``max_bytes``, else the largest multiple of 32 that fits -- and 32 when none does: a chunk
    of the kernel's 32 query columns is the least a call is cut to."""
    if Q <= 32 or nbytes_of(Q) <= max_bytes:
        return Q
    lo, hi = 1, (Q - 1) // 32
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if nbytes_of(32 * mid) <= max_bytes:
            lo = mid
        else:
            hi = mid - 1
    return 32 * lo


def shard_bounds(n_docs: int, world: int, rank: int):
    """Contiguous shard [start, stop) of rank `rank` (first n % world ranks get +1)."""
    base, rem = divmod(n_docs, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


class ShardedDenseIndex:
    """One rank's HBM-resident shard of the corpus embedding matrix.

    ``docs`` is this rank's shard [N_local, D] (bf16), ``doc_offset`` its first
    global index.  ``search`` and ``search_candidates`` are collective over
    ``group`` when one is given: every rank passes its local query slice (may be
    empty) and receives the global top-k for ALL gathered queries (queries
    ordered by rank).

    ``dtype="fp8"`` keeps the shard as e4m3 bytes (half the HBM bytes per scan,
    BASELINE config C5): queries are quantised with the same power-of-two
    ``fp8_scale`` per search and the scores returned are those of the
    quantised embeddings, descaled exactly.
    """

    def __init__(self, docs: torch.Tensor, doc_offset: int = 0, group=None, dtype: str = "bf16",
                 fp8_scale: float = FP8_SCALE):
        if dtype not in ("bf16", "fp8"):
            raise ValueError(f"dtype must be 'bf16' or 'fp8', not {dtype!r}")
        self.dtype = dtype
        self.fp8_scale = float(fp8_scale)
        if dtype == "fp8":
            self.docs = quantize_fp8(docs, self.fp8_scale)
        else:
            self.docs = docs.to(torch.bfloat16).contiguous()
        self.doc_offset = int(doc_offset)
        self.group = group

    # ------------------------------------------------------------ persistence
    # On-disk corpus index: one .npy per shard (bf16 as
    # uint16 bits, or e4m3 bytes), a JSON header, and the DrQA-style doc-id map
    # (doc_dict = (DOC2IDX, doc_ids), preprocessing/drqa/build_tfidf.py:126,198-205).
    def save(self, directory: str, rank: int = 0, doc_ids=None) -> None:
        import json
        import os

        import numpy as np

        os.makedirs(directory, exist_ok=True)
        raw = self.docs.view(torch.uint16) if self.dtype == "bf16" else self.docs
        np.save(os.path.join(directory, f"shard_{rank}.npy"), raw.cpu().numpy())
        meta = {"dtype": self.dtype, "fp8_scale": self.fp8_scale, "doc_offset": self.doc_offset,
                "rows": int(self.docs.shape[0]), "dim": int(self.docs.shape[1])}
        with open(os.path.join(directory, f"shard_{rank}.json"), "w") as f:
            json.dump(meta, f)
        if doc_ids is not None:
            with open(os.path.join(directory, "doc_ids.json"), "w") as f:
                json.dump(list(doc_ids), f)

    @classmethod
    def load(cls, directory: str, rank: int = 0, device=None, group=None):
        """(index, doc_dict or None): the shard saved by save() for this rank,
        resident on `device` (no re-quantisation: the stored bytes are used)."""
        import json
        import os

        import numpy as np

        with open(os.path.join(directory, f"shard_{rank}.json")) as f:
            meta = json.load(f)
        raw = torch.from_numpy(np.load(os.path.join(directory, f"shard_{rank}.npy")))
        raw = raw.to(device or "cuda")
        self = cls.__new__(cls)
        self.dtype = meta["dtype"]
        self.fp8_scale = float(meta["fp8_scale"])
        self.docs = raw.view(torch.bfloat16) if self.dtype == "bf16" else raw
        self.doc_offset = int(meta["doc_offset"])
        self.group = group
        doc_dict = None
        ids_path = os.path.join(directory, "doc_ids.json")
        if os.path.exists(ids_path):
            with open(ids_path) as f:
                ids = json.load(f)
            doc_dict = ({d: i for i, d in enumerate(ids)}, ids)
        return self, doc_dict

    # The two device steps are methods so the collective orchestration can be
    # exercised on CPU (gloo) with a test double in tests/test_dist_cpu.py.
    def _local_topk(self, queries, k, ws_tag="scan", group_off=None):
        """This shard's top-k: (scores, idx), or with ``group_off`` the top-k per group
        (scores, idx, n) over the shard's own slice of the groups."""
        if group_off is not None:
            go = self._local_groups(group_off)
            if self.dtype == "fp8":
                q8 = quantize_fp8(queries, self.fp8_scale)
                return scan_topk_grouped_fp8(q8, self.docs, k, go, self.doc_offset,
                                             1.0 / (self.fp8_scale * self.fp8_scale),
                                             ws_tag=ws_tag)[:3]
            return scan_topk_grouped(queries, self.docs, k, go, self.doc_offset,
                                     ws_tag=ws_tag)[:3]
        if self.dtype == "fp8":
            q8 = quantize_fp8(queries, self.fp8_scale)
            return scan_topk_fp8(q8, self.docs, k, self.doc_offset,
                                 1.0 / (self.fp8_scale * self.fp8_scale), ws_tag=ws_tag)
        return scan_topk(queries, self.docs, k, self.doc_offset, ws_tag=ws_tag)

    def _local_groups(self, group_off):
        """``group_off`` cut to the groups this shard can touch (``local_group_slice``; one
        entry, no group, when it touches none), so the per-shard workspace is proportional to
        the shard's own groups.  Computed once per ``group_off`` tensor OBJECT and kept on the
        index: the same object passed again costs nothing, another one a host sync."""
        memo = getattr(self, "_group_slice", None)
        if memo is not None and memo[0] is group_off:
            return memo[1]
        g_lo, g_hi = local_group_slice(group_off, self.doc_offset, self.docs.shape[0])
        cut = group_off[g_lo:g_hi + 1] if g_hi > g_lo else group_off[g_lo:g_lo + 1]
        self._group_slice = (group_off, cut.contiguous())
        return self._group_slice[1]

    def _merge(self, scores, idx, k):
        return topk_merge(scores, idx, k)

    def search(self, queries: torch.Tensor, k: int, equal_counts: bool = False,
               ws_tag: str = "scan", group_off=None):
        """Global top-k of the gathered queries.  ``equal_counts``: every rank
        passes the same number of queries, so the ragged-count exchange (a host
        sync) is skipped and the whole search stays stream-ordered.

        ``group_off`` (int64 [n_groups + 1], global row ids, non-decreasing, on the queries'
        device): the top-k distinct GROUPS of the whole corpus, each by its best row, as
        ``search_candidates(..., group_off=)`` ranks them when every row is a candidate --
        (scores [Q, k], idx [Q, k] global row ids, n [Q], groups [Q, k]), by (score desc, row
        id asc), padding (-inf, -1, group -1).  Each shard runs ``scan_topk_grouped`` over
        its own slice of the groups (``local_group_slice``); the slice is computed once per
        ``group_off`` tensor object -- memoised on the index and compared with ``is`` -- and
        costs one host synchronisation on first use, so pass the same tensor again, not a
        copy.  Over a process group the per-shard lists merge by ``topk_merge_grouped``
        (k * world size <= 8192), which keeps one row of a group whose rows lie in two
        shards; ``groups`` counts in the full ``group_off``.  fp8 indexes quantise the
        queries and descale as without groups (D % 128 == 0, else ValueError).  As for
        ``search_candidates``, every argument check runs on the rank's own arguments
        BEFORE the first collective.  ``search_many`` has no grouped form."""
        if group_off is None:
            if not self._sharded():
                return self._local_topk(queries, k, ws_tag)
            allq = self._gather_queries(queries, equal_counts)  # (1)
            s, i = self._local_topk(allq, k, ws_tag)  # (2)
            return self._exchange_merge(s, i, k)  # (3)
        _check_group_off(group_off, queries)
        if self.dtype == "fp8" and self.docs.shape[1] % 128 != 0:
            raise ValueError("fp8 index: the grouped scan needs D % 128 == 0, not "
                             f"D={self.docs.shape[1]}")
        if queries.dim() != 2 or queries.shape[1] != self.docs.shape[1]:
            raise ValueError(f"dim mismatch: queries {tuple(queries.shape)}, docs "
                             f"D={self.docs.shape[1]}")
        if not 1 <= k <= 1024:
            raise ValueError(f"k={k} outside [1, 1024]")
        if not self._sharded():
            s, i, n = self._local_topk(queries, k, ws_tag, group_off)
            return s, i, n, _groups_of(group_off, i)
        import torch.distributed as dist

        world = dist.get_world_size(self.group)
        if k * world > 8192:
            raise ValueError(f"k * world size = {k} x {world} above the grouped merge's 8192 "
                             "entries per query")
        allq = self._gather_queries(queries, equal_counts)  # (1)
        s, i, _ = self._local_topk(allq, k, ws_tag, group_off)  # (2)
        return self._exchange_merge(s, i, k, group_off)  # (3)

    def search_candidates(self, queries: torch.Tensor, cand: torch.Tensor,
                          cand_off: torch.Tensor, k: int, ws_tag: str = "rerank",
                          method: str = "gather", ascending: bool = False, group_off=None,
                          bias=None):
        """Top-k of each query over its own candidate docs only (global ids, the CSR pair
        ``SparseIndex.candidates`` / ``expand_ranges`` leave on the device): (scores
        [Q, k], idx [Q, k], n [Q]) as ``rerank_topk``.  bf16 and fp8 shards (on an fp8 index
        the queries are quantised with ``fp8_scale`` and ``rerank_topk_fp8`` ranks the e4m3
        codes, scores descaled exactly as ``search`` descales them; the measured fp8 tables
        are in DESIGN.md 6e).

        Collective over ``group`` as ``search`` is, in the same three steps: (1) every rank
        passes its own query slice (may be empty) and the CSR pair of those queries'
        candidates; one count exchange carries (queries, candidates) per rank, then the
        queries, the candidate ids (as int32, the kernels' dtype, so the ranks need not
        agree on int32 against int64) and the list lengths are all-gathered in rank order
        and ``cand_off`` is rebuilt for the gathered batch; (2) every rank ranks the
        candidates its shard owns (ids of other shards are skipped by the kernels); (3) the
        per-shard lists are all-gathered and merged, by ``topk_merge`` or, with
        ``group_off``, by ``topk_merge_grouped`` (k * world size <= 8192 there).  Every rank
        receives the result for ALL gathered queries, in rank order.  The argument checks
        (``method``, ``group_off``, the dtype of ``cand``, the length of ``cand_off``, the
        queries' width) run on each rank's own arguments BEFORE the first collective: a bad
        argument raises on that rank at once and never leaves the others waiting in a
        gather it does not join (they fail on the collective's timeout instead of
        computing with half a batch).  Every rank passes queries of one dtype, the same
        ``k``, ``method`` and ``group_off``.

        ``method``: "gather" (the default), "stream", or "auto", which takes
        ``rerank_method``'s choice when ``ascending=True`` and "gather" otherwise;
        ``ascending`` as in ``rerank_topk``.

        ``group_off`` (int64 [n_groups + 1], global row ids, on the queries' device): the
        top-k distinct groups, each by its best row, and a fourth result ``groups`` [Q, k],
        as ``rerank_topk`` documents it; "auto" chooses as without it.  Over a process
        group the result is the grouped top-k of the whole corpus: merging the per-shard
        grouped lists is exact ("Across shards").

        ``bias`` (fp32, one entry per candidate, parallel to ``cand``, on the queries'
        device): the candidates are ranked by score + bias as ``rerank_topk`` documents it
        (on an fp8 index the bias is added to the descaled score).  Over a process group
        each rank passes the bias of its own candidates and it is all-gathered with their
        ids, in rank order; every rank passes one or none does.  Its checks (dtype, length,
        device) run before the first collective like the others.

        Cost model: "gather" reads the candidate rows whole, once per
        (query, candidate), with no reuse across queries -- n_cand * D * 2 bytes -- while
        ``search`` streams the shard once for the whole batch.  "stream" does the latter for
        the candidates alone: the shard goes once per 256 queries through the same MFMA
        GEMM loop and each query's candidates are picked out of the score tiles.  Measured
        on the 250k x 768 shard (profiles/rerank_stream_probe.json, call times in us,
        gather / stream; ``tools/rerank_probe.py --tables`` prints this from the file):

            candidates per query     Q = 1         Q = 16        Q = 64        Q = 256
                 250 (0.1 %)         20 / 66       26 / 126      27 / 130       32 / 152
               2,500 (1 %)           26 / 130      31 / 139      54 / 143      158 / 166
              12,500 (5 %)           36 / 146      74 / 154     199 / 159      690 / 189
              62,500 (25 %)          74 / 189     270 / 200     876 / 213    3,300 / 300

        The gathered call grows with n_cand, the streamed one stays within 1.2-1.4x of a
        full scan plus the select: they cross at 1.1 % of the shard per query at Q = 256,
        3.7 % at Q = 64, 15.6 % at Q = 16, and gather wins throughout at Q = 1.  Either way
        this is the only call that ranks the candidates alone.

        Against the scan (tools/rerank_probe.py, profiles/rerank_probe.json: one MI355X, 250k x
        768 shard, random lists redrawn call by call, k = 100; call times in us, the gathered
        call / ``search``; ``tools/rerank_probe.py --tables`` prints this from the file):

            candidates per query     Q = 1         Q = 16        Q = 64        Q = 256
                 250 (0.1 %)         20 / 80       25 / 84       27 / 95        32 / 165
               2,500 (1 %)           26 / 80       30 / 84       55 / 94       158 / 164
              12,500 (5 %)           36 / 80       74 / 84      200 / 94       691 / 164
              62,500 (25 %)          74 / 80      271 / 84      876 / 94     3,303 / 164

        These two cross at about 1.0 % of the shard per query at Q = 256, 2.0 % at Q = 64,
        5.8 % at Q = 16, and above 25 % at Q = 1.  The scoring pass gathers 4.8-7.6 TB/s of
        row bytes from 160k candidates up (lists of one call that overlap hit the caches)
        and is latency-bound below."""
        _check_group_off(group_off, queries)
        _check_bias(bias, cand, queries)
        if self.dtype == "fp8" and self.docs.dtype != torch.uint8:
            # before anything touches the queries or the device: a hand-built index or a
            # damaged header on load()
            raise ValueError("fp8 index: the shard is not e4m3 bytes (torch.uint8) but "
                             f"{self.docs.dtype}")
        # the bias is passed on, and comes back, only when one was given
        kw = {} if bias is None else {"bias": bias}
        if not self._sharded():
            return self._local_candidates(queries, cand, cand_off, k, ws_tag, method, ascending,
                                          group_off, **kw)
        own = self._own_candidates(queries, cand, cand_off, method, **kw)  # raises before (1)
        gathered = self._gather_candidates(queries, *own)  # (1)
        if bias is not None:
            kw = {"bias": gathered[3]}
        out = self._local_candidates(*gathered[:3], k, ws_tag, method, ascending, group_off,
                                     **kw)  # (2)
        return self._exchange_merge_candidates(out[0], out[1], k, group_off)  # (3)

    # The steps of a sharded search_candidates are methods as search()'s are, so the
    # collective orchestration runs on CPU (gloo) with test doubles for the device calls
    # (tests/test_rerank_sharded_cpu.py): _local_candidates, _merge, _merge_grouped.
    def _local_candidates(self, queries, cand, cand_off, k, ws_tag="rerank", method="gather",
                          ascending=False, group_off=None, bias=None):
        """This shard's candidate top-k: the whole of a single-process search_candidates,
        step (2) of a sharded one."""
        if method == "auto":
            # the stream method's sort of unsorted lists is not in the measured crossovers
            method = "gather" if not ascending else rerank_method(
                queries.shape[0], self.docs.shape[0], self.docs.shape[1], cand.numel(),
                dtype=self.dtype)
        if self.dtype == "fp8":
            q8 = quantize_fp8(queries, self.fp8_scale)
            return rerank_topk_fp8(q8, self.docs, cand, cand_off, k, self.doc_offset,
                                   1.0 / (self.fp8_scale * self.fp8_scale), ws_tag=ws_tag,
                                   method=method, ascending=ascending, group_off=group_off,
                                   bias=bias)
        return rerank_topk(queries, self.docs, cand, cand_off, k, self.doc_offset, ws_tag=ws_tag,
                           method=method, ascending=ascending, group_off=group_off, bias=bias)

    def _merge_grouped(self, scores, idx, k, group_off):
        return topk_merge_grouped(scores, idx, k, group_off)

    def _own_candidates(self, queries, cand, cand_off, method, bias=None):
        """This rank's arguments checked as the local call would check them, before any
        collective; returns the ids as flat int32 (an int64 id outside int32 is in no shard
        and is clamped to -1 / 2^31 - 1, which keeps an ascending list ascending) and the
        offsets as int64 -- and, when a ``bias`` was given, that as flat fp32 after them."""
        if method != "auto" and method not in RERANK_METHODS:
            raise ValueError(f"method must be 'auto' or one of {RERANK_METHODS}, not {method!r}")
        if queries.dim() != 2 or queries.shape[1] != self.docs.shape[1]:
            raise ValueError(f"dim mismatch: queries {tuple(queries.shape)}, docs "
                             f"D={self.docs.shape[1]}")
        if cand.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"cand must be int32 or int64, not {cand.dtype}")
        if cand_off.numel() != queries.shape[0] + 1:
            raise ValueError(f"cand_off has {cand_off.numel()} entries for {queries.shape[0]} "
                             "queries (Q + 1)")
        if cand.dtype == torch.int64:
            cand = cand.clamp(-1, 2 ** 31 - 1)
        own =(cand.reshape(-1).to(torch.int32).contiguous(),
               cand_off.reshape(-1).to(torch.int64).contiguous())
        if bias is not None:
            own += (bias.reshape(-1).contiguous(),)
        return own

    def _gather_candidates(self, queries, cand, cand_off, bias=None):
        """(1) every rank's query slice and candidate lists, all-gathered in rank order:
        (queries [Q_all, D], cand int32 [n_all], cand_off int64 [Q_all + 1]).  One count
        exchange (a host sync) carries each rank's (queries, candidates); the offsets are
        rebuilt from the gathered list lengths.  With ``bias`` (fp32, parallel to ``cand``)
        a fourth result: the ranks' biases gathered as the ids are, so entry j of it still
        belongs to gathered candidate j."""
        import torch.distributed as dist

        world = dist.get_world_size(self.group)
        mine = torch.tensor([queries.shape[0], cand.numel()], dtype=torch.int64,
                            device=queries.device)
        cnt = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(cnt, mine, group=self.group)
        cnt = torch.stack(cnt).cpu().tolist()
        nq, nc = [c[0] for c in cnt], [c[1] for c in cnt]
        allq = self._gather_ragged(queries, nq)
        allc = self._gather_ragged(cand, nc)
        lengths = self._gather_ragged(cand_off[1:] - cand_off[:-1], nq)
        alloff = torch.cat([lengths.new_zeros(1), torch.cumsum(lengths, 0)])
        if bias is not None:
            return allq, allc, alloff, self._gather_ragged(bias, nc)
        return allq, allc, alloff

    def _gather_ragged(self, x, counts):
        """Every rank's ``x`` ([counts[rank], ...]) concatenated along dim 0 in rank order:
        padded to the longest, all-gathered, cut back."""
        import torch.distributed as dist

        top = max(counts)
        pad = x.contiguous()
        if top != x.shape[0]:
            pad = torch.zeros((top,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
            pad[: x.shape[0]] = x
        parts = [torch.empty_like(pad) for _ in counts]
        dist.all_gather(parts, pad, group=self.group)
        return torch.cat([p[:c] for p, c in zip(parts, counts)], dim=0)

    def _exchange_merge_candidates(self, s, i, k, group_off=None):
        """(3) every shard's candidate top-k lists all-gathered and merged: by the scan's
        rule (n = the filled slots), or per group -- a group whose best rows lie in two
        shards is in two lists, and only its best row stays."""
        import torch.distributed as dist

        world = dist.get_world_size(self.group)
        ss = [torch.empty_like(s) for _ in range(world)]
        ii = [torch.empty_like(i) for _ in range(world)]
        dist.all_gather(ss, s.contiguous(), group=self.group)
        dist.all_gather(ii, i.contiguous(), group=self.group)
        if group_off is not None:
            return self._merge_grouped(torch.stack(ss), torch.stack(ii), k, group_off)
        ms, mi = self._merge(torch.stack(ss), torch.stack(ii), k)
        return ms, mi, (mi >= 0).sum(dim=1).to(torch.int32)

    # The three steps of a sharded search, separately callable (bench.py times each).
    def _sharded(self):
        import torch.distributed as dist

        return not (self.group is None or not dist.is_initialized() or
                    dist.get_world_size(self.group) == 1)

    def _gather_queries(self, queries, equal_counts=False):
        """(1) every rank's query slice, all-gathered in rank order (ragged: the counts
        are exchanged first, a host sync that ``equal_counts`` skips)."""
        import torch.distributed as dist

        world = dist.get_world_size(self.group)
        if equal_counts:
            counts = [queries.shape[0]] * world
        else:
            n_local = torch.tensor([queries.shape[0]], dtype=torch.int64, device=queries.device)
            cnt = [torch.zeros_like(n_local) for _ in range(world)]
            dist.all_gather(cnt, n_local, group=self.group)
            counts = [int(c.item()) for c in cnt]
        qmax = max(counts)
        if qmax == queries.shape[0]:
            qpad = queries.contiguous()
        else:
            qpad = torch.zeros((qmax, queries.shape[1]), dtype=queries.dtype,
                               device=queries.device)
            qpad[: queries.shape[0]] = queries
        gathered = [torch.empty_like(qpad) for _ in range(world)]
        dist.all_gather(gathered, qpad, group=self.group)
        return torch.cat([g[:c] for g, c in zip(gathered, counts)], dim=0)

    def _exchange_merge(self, s, i, k, group_off=None):
        """(3) every shard's exact top-k lists (global doc ids) all-gathered and merged
        by the (score desc, index asc) rule: every rank gets the global result.  With
        ``group_off`` the lists hold one row per group and merge per group
        (``_merge_grouped``, as ``_exchange_merge_candidates`` does)."""
        import torch.distributed as dist

        world = dist.get_world_size(self.group)
        ss = [torch.empty_like(s) for _ in range(world)]
        ii = [torch.empty_like(i) for _ in range(world)]
        dist.all_gather(ss, s.contiguous(), group=self.group)
        dist.all_gather(ii, i.contiguous(), group=self.group)
        if group_off is not None:
            return self._merge_grouped(torch.stack(ss), torch.stack(ii), k, group_off)
        return self._merge(torch.stack(ss), torch.stack(ii), k)

    def search_many(self, batches, k: int, depth: int = 3, equal_counts: bool = False,
                    graphs: bool = False):
        """search() over a sequence of query batches with up to ``depth`` batches
        in flight on as many HIP streams (each with its own scan workspace): one
        batch's latency-bound selects overlap the next batch's HBM-bound filter.
        Single process, bf16, batches of one shape: the whole loop is one native call
        (irc_scan_topk_many: the host issues a C2 batch in 13-17 us against 39-43 us for
        search() per batch, so the loop stays GPU-bound -- 60.6 us a batch at depth 3 on
        a box where the Python loop also kept up, profiles/r06_i_scan_depth.log; the C2
        leg on boxes since: 3.97-4.09M queries/s, profiles/r06_m/, against 3.27M with the
        Python loop in profiles/r06_fin1_bench.log).  ``graphs`` (single process, every batch of one
        shape): each stream replays a HIP graph of the whole local search captured once
        -- measured slower than direct launches at C2 (77-80 us a batch at depth 3).
        Results are identical to calling search() per batch; returned in order, usable
        on the current stream."""
        import torch.distributed as dist

        batches = list(batches)
        dev = self.docs.device
        cur = torch.cuda.current_stream(dev)
        streams = _search_streams(dev, depth)
        single = self.group is None or not dist.is_initialized() or \
            dist.get_world_size(self.group) == 1
        if graphs and not single:
            raise ValueError("graphed search_many needs a single-process index")
        if single and not graphs and self.dtype == "bf16" and batches and \
                all(q.shape == batches[0].shape for q in batches):
            # the whole loop in one native call (irc_scan_topk_many): the per-batch Python
            # of search() paced a C2 batch's ~70 us of GPU work
            return scan_topk_many(batches, self.docs, k, self.doc_offset, streams)
        slots = self._graph_slots(batches[0], k, depth, streams) if (graphs and batches) else None
        out = []
        for n, q in enumerate(batches):
            st = streams[n % depth]
            st.wait_stream(cur)  # the batch's inputs were produced on `cur`
            with torch.cuda.stream(st):
                if slots is not None:
                    g, qin, so, io, _ws = slots[n % depth]
                    qin.copy_(q)
                    g.replay()
                    res = (so.clone(), io.clone())
                else:
                    res = self.search(q, k, equal_counts=equal_counts, ws_tag=f"scan{n % depth}")
            q.record_stream(st)
            out.append(res)
        for st in streams:
            cur.wait_stream(st)
        for s, i in out:
            s.record_stream(cur)
            i.record_stream(cur)
        return out

    def _graph_slots(self, q0, k, depth, streams):
        """Per stream: (graph, static query buffer, static scores, static ids, workspace)
        of the local search for q0's shape, captured once and cached on the index.

        Each slot OWNS its scan workspace: it is taken out of the shared grow-only
        cache right after capture (under a tag no other call uses), so no later
        call on any index can grow -- and free -- memory a captured graph points
        into.  The key includes the shard tensor, so replacing ``self.docs``
        captures anew instead of replaying against the old one."""
        from ._torch import take_workspace

        key = (tuple(q0.shape), q0.dtype, int(k), depth, self.docs.data_ptr(),
               tuple(self.docs.shape), self.dtype)
        cache = self.__dict__.setdefault("_graphs", {})
        if key in cache:
            return cache[key]
        slots = []
        for st in streams:
            qin = torch.empty_like(q0)
            qin.copy_(q0)
            tag = f"gscan:{next(_GRAPH_SERIAL)}"
            with torch.cuda.stream(st):
                self._local_topk(qin, k, tag)  # warm-up: workspace sized outside the graph
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                so, io = self._local_topk(qin, k, tag)
            ws = take_workspace(self.docs.device, tag)  # owned by this slot from now on
            slots.append((g, qin, so, io, ws))
        cache[key] = slots
        return slots


class IVFDenseIndex(ShardedDenseIndex):
    """A shard of the corpus as an inverted-file (IVF) index: the rows clustered into ``nlist``
    lists, a search scoring only the ``nprobe`` lists nearest to each query.

    Everything approximate lies in WHICH lists are probed; their rows are ranked exactly.
    ``search(queries, k, nprobe)`` is, per query, the exact top-k over the union of the rows of
    its probed lists, by (score desc, global id asc), padding (-inf, -1), n[q] = min(k, rows in
    the probed lists).  With ``nprobe == nlist`` it is ``ShardedDenseIndex.search``'s ranking.
    Ids are global ids of the ORIGINAL corpus (``doc_offset`` + original row), so per-shard
    results merge with ``topk_merge`` as the scan's do.

    ``dtype`` is "bf16" or, from ``to_fp8`` / ``train(dtype="fp8")`` / a loaded e4m3 shard,
    "fp8": the lists are then e4m3 bytes (half the bytes a search streams), a search quantises
    its queries with ``fp8_scale`` inside the native call and the scores are those of the
    quantised embeddings, descaled exactly, as ``ShardedDenseIndex(dtype="fp8")`` reports them.
    The centroids and the probe stay bf16, so an fp8 index probes the lists its bf16 parent
    probes.

    Attributes: ``docs`` [N, D] bf16 (or uint8 e4m3 bytes), the rows in list order (the only
    copy); ``row_id`` int32 [N], each row's global id; ``list_off`` int64 [nlist + 1];
    ``centroids`` [nlist, D] bf16;
    ``max_list_rows`` (host int, the longest list); ``max_workspace_bytes`` (the workspace one
    native call may take; a larger batch runs in query chunks, same bits).

    Build it with ``train`` (k-means on the device) or ``from_lists`` (the caller's own
    clustering); the plain constructor is not the way in."""

    KEY_BOUND_LISTS = 1024  # the longest lists whose prefix sums are kept: the most a probe ranks
    max_workspace_bytes = 1 << 30

    def __init__(self, *args, **kwargs):
        raise TypeError("build an IVFDenseIndex with IVFDenseIndex.train(...) or "
                        "IVFDenseIndex.from_lists(...)")

    def _set_list_bounds(self):
        """One host synchronisation: the prefix sums of the longest lists' lengths, descending,
        kept on the host (``key_bound``); ``max_list_rows`` is the first."""
        lens = self.list_off[1:] - self.list_off[:-1]
        top = torch.sort(lens, descending=True)[0][:self.KEY_BOUND_LISTS]
        self._key_prefix = [int(x) for x in torch.cumsum(top, 0).tolist()]
        self.max_list_rows = self._key_prefix[0] if self._key_prefix else 0

    def key_bound(self, nprobe: int) -> int:
        """The most rows a query's ``nprobe`` probed lists can hold: the sum of the ``nprobe``
        longest lists.  A host int, no synchronisation; Q x key_bound(nprobe) bounds the keys
        of a search of Q queries whatever they probe (rows unique)."""
        if not 1 <= nprobe <= len(self._key_prefix):
            raise ValueError(f"key_bound(nprobe={nprobe}): outside [1, {len(self._key_prefix)}], "
                             "the longest lists kept")
        return self._key_prefix[nprobe - 1]

    @classmethod
    def from_lists(cls, docs: torch.Tensor, centroids: torch.Tensor, assign: torch.Tensor,
                   doc_offset: int = 0, group=None, dtype: str = "bf16"):
        """The index over a caller's clustering: ``assign`` [N] gives each row of ``docs`` its
        list in [0, nlist), ``centroids`` [nlist, D] is what ``probe`` ranks the lists by (inner
        product).  One host synchronisation (the longest lists' lengths, ``key_bound``).
        The lists are built from bf16 rows; ``to_fp8`` of the result stores them as e4m3."""
        if dtype != "bf16":
            raise ValueError(f"IVFDenseIndex is bf16 only (e4m3 lists are a follow-up), not "
                             f"dtype={dtype!r}")
        if docs.dim() != 2 or centroids.dim() != 2 or centroids.shape[1] != docs.shape[1]:
            raise ValueError(f"docs {tuple(docs.shape)} and centroids {tuple(centroids.shape)} "
                             "must be [N, D] and [nlist, D]")
        if assign.numel() != docs.shape[0]:
            raise ValueError(f"assign has {assign.numel()} entries for {docs.shape[0]} rows")
        if doc_offset < 0 or doc_offset + docs.shape[0] >= 2 ** 31:
            raise ValueError("global doc ids must fit int32 (doc_offset + N < 2^31)")
        nlist = centroids.shape[0]
        order, list_off = ivf_layout(assign.to(docs.device), nlist)
        self = cls.__new__(cls)
        self.dtype = "bf16"
        self.fp8_scale = float(FP8_SCALE)
        self.docs = docs.to(torch.bfloat16)[order].contiguous()
        self.row_id = (order + int(doc_offset)).to(torch.int32)
        self.list_off = list_off
        self.centroids = centroids.to(device=docs.device, dtype=torch.bfloat16).contiguous()
        self._set_list_bounds()
        self.doc_offset = int(doc_offset)
        self.group = group
        return self

    @classmethod
    def train(cls, docs: torch.Tensor, nlist: int, doc_offset: int = 0, group=None,
              niter: int = 20, nredo: int = 1, seed: int = 0, dtype: str = "bf16",
              fp8_scale: float = FP8_SCALE):
        """Cluster ``docs`` [N, D] into ``nlist`` lists and build the index: ``cluster.kmeans`` on
        the fp32 rows, the centroids L2-normalised as the reference's run_kmeans leaves its
        prototypes (src/contrastor/utils.py:98), then every row assigned to the centroid of
        LARGEST INNER PRODUCT -- the probe ranks lists by inner product, so the assignment
        does too (``cluster._assign`` over the normalised centroids with a zero bias).  The
        centroids are kept as bf16.  Under a launcher each rank trains over its own shard.
        ``dtype="fp8"`` trains the same way and returns ``.to_fp8(fp8_scale)``."""
        from . import cluster

        if dtype not in ("bf16", "fp8"):
            raise ValueError(f"dtype must be 'bf16' or 'fp8', not {dtype!r}")
        require_hip(docs)
        x = docs.float().contiguous()
        c, _, _ = cluster.kmeans(x, nlist, niter=niter, nredo=nredo, seed=seed)
        # the bf16 centroids are what the probe ranks by, so the rows are assigned by them too
        c = torch.nn.functional.normalize(c, dim=1).to(torch.bfloat16)
        bias = torch.zeros((nlist,), dtype=torch.float32, device=x.device)
        assign, _ = cluster._assign(x, c.float().contiguous(), bias)
        index = cls.from_lists(docs, c, assign, doc_offset, group)
        return index if dtype == "bf16" else index.to_fp8(fp8_scale)

    def to_fp8(self, fp8_scale: float = FP8_SCALE):
        """A new index over the same clustering with e4m3 lists: ``docs`` is ``quantize_fp8`` of
        this index's rows (already in list order) at ``fp8_scale``; ``row_id``, ``list_off``,
        ``centroids`` and the key bounds are shared with this one.  No host synchronisation."""
        if self.dtype != "bf16":
            raise ValueError(f"to_fp8: the lists are already {self.dtype}")
        other = type(self).__new__(type(self))
        other.__dict__.update(self.__dict__)
        other.dtype = "fp8"
        other.fp8_scale = float(fp8_scale)
        other.docs = quantize_fp8(self.docs, other.fp8_scale)
        return other

    # ------------------------------------------------------------ persistence
    def save(self, directory: str, rank: int = 0, doc_ids=None) -> None:
        """The parent's files (the rows in list order) and ``ivf_{rank}.npz``: the centroids'
        bf16 bits, ``list_off`` and ``row_id``."""
        import os

        import numpy as np

        super().save(directory, rank, doc_ids)
        np.savez(os.path.join(directory, f"ivf_{rank}.npz"),
                 centroids=self.centroids.view(torch.uint16).cpu().numpy(),
                 list_off=self.list_off.cpu().numpy(), row_id=self.row_id.cpu().numpy())

    @classmethod
    def load(cls, directory: str, rank: int = 0, device=None, group=None):
        import os

        import numpy as np

        self, doc_dict = super().load(directory, rank, device, group)
        dev = self.docs.device
        with np.load(os.path.join(directory, f"ivf_{rank}.npz")) as z:
            self.centroids = torch.from_numpy(z["centroids"]).to(dev).view(torch.bfloat16)
            self.list_off = torch.from_numpy(z["list_off"]).to(dev)
            self.row_id = torch.from_numpy(z["row_id"]).to(dev)
        self._set_list_bounds()
        return self, doc_dict

    # ------------------------------------------------------------ search
    def _check_nprobe(self, nprobe):
        nlist = self.centroids.shape[0]
        if not 1 <= nprobe <= min(nlist, 1024):
            raise ValueError(f"nprobe={nprobe} outside [1, min(nlist={nlist}, 1024)]")

    def probe(self, queries: torch.Tensor, nprobe: int) -> torch.Tensor:
        """The ``nprobe`` lists nearest to each query, int32 [Q, nprobe]: ``scan_topk`` over the
        centroids -- inner product desc, ties to the lower list id."""
        self._check_nprobe(nprobe)
        return scan_topk(queries, self.centroids, nprobe, ws_tag="ivf_probe")[1].to(torch.int32)

    def _local_ivf(self, queries, k, nprobe, probe, ws_tag):
        """This shard's probe, plan, scoring and select as one native call (``ivf_search``),
        stream-ordered: the whole of a single-process search, step (2) of a sharded one.  A
        batch whose workspace would pass ``max_workspace_bytes`` runs in query chunks
        (``ivf_query_chunk``) that write their rows of the outputs in place: a list may be
        streamed more often, no bit changes (one accumulation order per pair)."""
        require_hip(queries, self.docs, probe)
        Q = queries.shape[0]
        nlist = self.centroids.shape[0]
        if probe is not None:
            nprobe = probe.shape[1]
        kept = len(self._key_prefix)
        if nprobe <= kept:
            bound = self.key_bound(nprobe)
        else:  # a caller's wider probe: none of the other lists is longer than the last one kept
            bound = self._key_prefix[-1] + (nprobe - kept) * (
                self._key_prefix[-1] - self._key_prefix[-2])
        fp8 = self.dtype == "fp8"
        need = _lib.fn("irc_ivf_search_fp8_workspace" if fp8 else "irc_ivf_search_workspace")
        # the descale ShardedDenseIndex(dtype="fp8").search applies
        scales = dict(query_scale=self.fp8_scale,
                      score_scale=1.0 / (self.fp8_scale * self.fp8_scale)) if fp8 else {}
        search = ivf_search_fp8 if fp8 else ivf_search
        step = ivf_query_chunk(Q, self.max_workspace_bytes,
                               lambda c: int(need(c, nprobe, nlist, c * bound, k)))
        out = (torch.empty((Q, k), dtype=torch.float32, device=queries.device),
               torch.empty((Q, k), dtype=torch.int64, device=queries.device),
               torch.empty((Q,), dtype=torch.int32, device=queries.device))
        for lo in range(0, max(Q, 1), max(step, 1)):
            hi = min(Q, lo + step)
            search(queries[lo:hi], self.docs, self.row_id, self.list_off, k,
                   (hi - lo) * bound, self.max_list_rows, centroids=self.centroids,
                   nprobe=nprobe if probe is None else None,
                   probe=None if probe is None else probe[lo:hi], ws_tag=ws_tag,
                   out=tuple(o[lo:hi] for o in out), **scales)
        return out

    def search(self, queries: torch.Tensor, k: int, nprobe=None, probe=None,
               equal_counts: bool = False, ws_tag: str = "ivf", group_off=None):
        """(scores [Q, k], idx [Q, k] global ids, n [Q]): each query's exact top-k over the rows
        of its probed lists.  Exactly one of ``nprobe`` (this index's own ``probe``) and
        ``probe`` (int32 [Q, nprobe], the caller's lists, -1 = none) is given.

        Over a process group it is the scan's three steps with the middle one replaced: the
        queries are all-gathered, every shard probes ``nprobe`` of ITS OWN lists and ranks
        their rows, the per-shard lists are all-gathered and merged; n is the count of filled
        slots.  ``probe=`` is then an error (lists are per shard).  Every argument check runs
        before the first collective."""
        if group_off is not None:
            raise NotImplementedError("IVFDenseIndex.search(group_off=): the rows are permuted, "
                                      "so groups are no row ranges; a follow-up")
        if (nprobe is None) == (probe is None):
            raise ValueError("give exactly one of nprobe and probe")
        if not 1 <= k <= 1024:
            raise ValueError(f"k={k} outside [1, 1024]")
        if queries.dim() != 2 or queries.shape[1] != self.docs.shape[1]:
            raise ValueError(f"dim mismatch: queries {tuple(queries.shape)}, docs "
                             f"D={self.docs.shape[1]}")
        if nprobe is not None:
            self._check_nprobe(nprobe)
        elif self._sharded():
            raise ValueError("probe= over a process group: lists are per shard, pass nprobe")
        elif probe.dim() != 2 or probe.shape[0] != queries.shape[0] or \
                not 1 <= probe.shape[1] <= self.centroids.shape[0]:
            raise ValueError(f"probe must be [Q, 1 .. nlist] for {queries.shape[0]} queries, "
                             f"not {tuple(probe.shape)}")
        if not self._sharded():
            return self._local_ivf(queries, k, nprobe, probe, ws_tag)
        allq = self._gather_queries(queries, equal_counts)  # (1)
        s, i, _ = self._local_ivf(allq, k, nprobe, None, ws_tag)  # (2)
        ms, mi = self._exchange_merge(s, i, k)  # (3)
        return ms, mi, (mi >= 0).sum(dim=1).to(torch.int32)

    def search_candidates(self, *args, **kwargs):
        raise NotImplementedError("IVFDenseIndex.search_candidates: candidate ids name original "
                                  "rows and the rows are permuted; a follow-up")

    def search_many(self, *args, **kwargs):
        raise NotImplementedError("IVFDenseIndex.search_many: the pipelined form is built on "
                                  "the scan's native loop; a follow-up")


_GRAPH_SERIAL = itertools.count()  # unique workspace tags of captured searches
_SEARCH_STREAMS = {}


def _search_streams(dev, depth):
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), depth)
    st = _SEARCH_STREAMS.get(key)
    if st is None:
        st = _SEARCH_STREAMS[key] = [torch.cuda.Stream(dev) for _ in range(depth)]
    return st
