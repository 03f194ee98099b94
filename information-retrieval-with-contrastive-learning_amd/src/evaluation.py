"""Drop-in for src/evaluation.py: claim -> evidence retrieval.

``predict`` (src/evaluation.py:86-116) keeps the reference's behaviour by
default (``args.retrieval`` "sparse", main.py ``--retrieval``): per claim the
hashed n-gram candidate filter ``documents_filtering`` (here on the GPU,
irc_amd.sparse) with its latency and ``len(docs)`` printed, as the reference
prints them.  ``--retrieval dense`` (superset) runs the dense path the reference
sketches in its commented-out tail (:110-115): ``ctx2vec`` embeddings
(contrastive_module.py:96-100) of the evidence corpus sharded into HBM and each
claim batch scored against all of them with the exact top-k scan
(irc_amd.retrieval, closest_docs ordering, tfidf_doc_ranker.py:60-75), then
evidence recall@k printed.  ``--retrieval hybrid`` joins the two as the reference's
predict() describes: the filter's candidates (:57-83) stay on the device and the
dense scores (:110-112) rank each claim's candidates only (``hybrid_search``,
irc_rerank_topk); under a launcher the corpus is sharded over the ranks as for
``--retrieval dense`` and the per-shard lists are merged.
"""
import pickle
import time

import torch
from tqdm import tqdm

from irc_amd.retrieval import ShardedDenseIndex
from irc_amd.sparse import SparseIndex, load_sparse_csr
from src.dataset import get_dataloader
from src.model import load_model


_SPARSE_CACHE = {}


def _sparse_index(count_matrix, metadata, device):
    """The inverted count matrix resident in HBM, built once per matrix object."""
    key = (id(count_matrix), str(device))
    idx = _SPARSE_CACHE.get(key)
    if idx is None:
        idx = _SPARSE_CACHE[key] = SparseIndex(count_matrix, ngram=metadata["ngram"],
                                               device=device)
    return idx


def documents_filtering(claim, args, count_matrix, metadata, full_doc_dict, bigram_only=True):
    """src/evaluation.py:57-81: {doc_id: doc} of the docs sharing a hashed n-gram
    with the claim.  Tokenisation and hashing on the host (irc_amd.sparse, the
    reference's SimpleTokenizer / filter_ngram / murmurhash3); the row union over
    the inverted count matrix on the GPU (irc_csr_union_*)."""
    if metadata.get("tokenizer", "simple") != "simple":
        raise ValueError("only the DrQA 'simple' tokenizer is supported on this path")
    device = getattr(args, "device", None) or torch.device("cuda")
    index = _sparse_index(count_matrix, metadata, device)
    doc_ids = metadata["doc_dict"][1]
    docs = {}
    for i in index.documents_filtering([claim], bigram_only)[0]:
        doc_id = doc_ids[int(i)]
        if doc_id in full_doc_dict:  # the reference skips ids missing from the dict
            docs[doc_id] = full_doc_dict[doc_id]
    return docs


@torch.no_grad()
def encode_corpus(model, texts, device, batch_size=256):
    embs = []
    for i in range(0, len(texts), batch_size):
        embs.append(model.ctx2vec(texts[i:i + batch_size], device))
    return torch.cat(embs, 0) if embs else torch.empty(0, model.loss_config["dim"], device=device)


@torch.no_grad()
def predict(args, k=100):
    """evaluation.py:86-108: load the checkpoint, then per claim the sparse filter
    (latency and candidate count printed); ``args.retrieval == "dense"``:
    predict_dense.  Returns the per-claim candidate counts (sparse) or recall@k."""
    if getattr(args, "retrieval", "sparse") == "dense":
        return predict_dense(args, k)
    if getattr(args, "retrieval", "sparse") == "hybrid":
        return predict_hybrid(args, k)
    assert args.ckpt is not None
    _, model, _, _ = load_model(args.ckpt)
    model = model.to(args.device)
    # data parallel: each rank filters a disjoint share of the claim batches
    fever_loader = get_dataloader(args, train=False,
                                  distributed=getattr(args, "dist_group", None) is not None)
    ds = args.config["dataset"]
    _, metadata = load_sparse_csr(ds["tfidf"])
    count_matrix, _ = load_sparse_csr(ds["inverted_file"])
    with open(ds["full_docs_dict"], "rb") as f:  # the user's own preprocessing output
        full_docs_dict = pickle.load(f)
    counts = []
    for batch in tqdm(fever_loader, desc="Iteration"):
        claim = [data["claim"] for data in batch]
        s = time.time()
        docs = documents_filtering(claim[0], args, count_matrix, metadata, full_docs_dict, False)
        e = time.time()
        print(e - s)
        print(len(docs))
        counts.append(len(docs))
    return counts


@torch.no_grad()
def predict_dense(args, k=100):
    """Dense claim -> evidence-line retrieval with the trained bi-encoder: prints
    each batch's latency and the evidence recall@k; returns recall@k.

    Under data parallelism (``args.dist_group``, main.py under torchrun) the
    evidence corpus is sharded: rank r encodes and keeps only its contiguous
    slice (irc_amd.retrieval.shard_bounds) in HBM, each claim batch is split over
    the ranks, and ShardedDenseIndex.search all-gathers the claim embeddings,
    scans every shard and merges the per-shard top-k -- every rank receives the
    global result for the whole batch.

    ``args.rerank_unit == "page"`` (main.py --rerank-unit): the k best PAGES, each by its
    best line, instead of the k best lines -- ``search(..., group_off=row_off)``, the page
    -> row range map built while the lines are enumerated -- and the recall printed is
    over k pages, as the FEVER labels count.

    ``args.index == "ivf"`` (main.py --index): the shard becomes an ``IVFDenseIndex`` of
    ``args.nlist`` lists, each rank training over its own slice, and a search ranks the rows
    of the ``args.nprobe`` lists nearest to each claim (per shard); the recall line names
    both.  With every list probed it is the flat index's ranking.  ``args.ivf_list_dtype ==
    "fp8"`` (main.py --ivf-list-dtype) keeps the lists as e4m3 bytes (``train(dtype="fp8")``);
    the recall line then names that too."""
    from irc_amd.retrieval import IVFDenseIndex, shard_bounds

    assert args.ckpt is not None
    _, model, _, _ = load_model(args.ckpt)
    model = model.to(args.device).eval()
    loader = get_dataloader(args, train=False, distributed=False)
    group = getattr(args, "dist_group", None)
    world = int(getattr(args, "world_size", 1)) if group is not None else 1
    rank = int(getattr(args, "rank", 0)) if group is not None else 0
    # evidence corpus = every evidence document line of the dev set's wiki pages; row_off:
    # page p owns the rows [row_off[p], row_off[p + 1])
    titles, texts, row_off = [], [], [0]
    for title, page in loader.dataset.wiki.items():
        for line in page["lines"]:
            if line.strip():
                titles.append(title)
                texts.append(line)
        row_off.append(len(texts))
    by_page = getattr(args, "rerank_unit", "line") == "page"
    row_off = torch.tensor(row_off, dtype=torch.int64, device=args.device) if by_page else None
    lo, hi = shard_bounds(len(texts), world, rank)
    ivf = getattr(args, "index", "flat") == "ivf"
    if ivf:
        if by_page or getattr(args, "index_dtype", "bf16") != "bf16":
            raise ValueError("--index ivf: --index-dtype bf16 (e4m3 lists are "
                             "--ivf-list-dtype fp8) and the line unit only")
        list_dtype = getattr(args, "ivf_list_dtype", "bf16")
        index = IVFDenseIndex.train(encode_corpus(model, texts[lo:hi], args.device), args.nlist,
                                    doc_offset=lo, group=group, seed=getattr(args, "seed", 0),
                                    dtype=list_dtype)
    else:
        index = ShardedDenseIndex(encode_corpus(model, texts[lo:hi], args.device), doc_offset=lo,
                                  group=group, dtype=getattr(args, "index_dtype", "bf16"))
    dim = model.loss_config["dim"]
    hits = total = 0
    for batch in tqdm(loader, desc="Iteration", disable=rank != 0):
        claims = [d["claim"] for d in batch]
        s = time.time()
        c0, c1 = shard_bounds(len(claims), world, rank)
        mine = claims[c0:c1]
        q = model.ctx2vec(mine, args.device) if mine else \
            torch.empty((0, dim), dtype=torch.float32, device=args.device)
        # rows: the whole batch, in order
        if ivf:
            idx = index.search(q, k, nprobe=args.nprobe)[1]
        else:
            idx = index.search(q, k, group_off=row_off)[1] if by_page else index.search(q, k)[1]
        torch.cuda.synchronize()
        if rank == 0:
            print(f"batch of {len(claims)} claims: {time.time() - s:.4f}s")
        idx = idx.cpu().tolist()
        for d, row in zip(batch, idx):
            gold = {e["title"] for e in d["evidences"]}
            hits += int(any(titles[j] in gold for j in row if j >= 0))
            total += 1
    if rank == 0:
        lists = " lists=fp8" if ivf and list_dtype == "fp8" else ""
        unit = f" (ivf nlist={args.nlist} nprobe={args.nprobe}{lists})" if ivf else \
            (" (pages)" if by_page else "")
        print(f"evidence recall@{k}{unit}: {hits / max(total, 1):.4f}")
    return hits / max(total, 1)


def hybrid_corpus(wiki, doc_ids):
    """The dense corpus of the two-stage pipeline, in count-matrix column order: column
    i is the page ``doc_ids[i]`` (metadata["doc_dict"][1]); if the wiki has it, its
    non-empty lines become rows.  Returns (titles, texts, row_off): one title and text
    per row, and row_off [n_cols + 1] with column i owning rows [row_off[i],
    row_off[i + 1]) -- empty for a column absent from the wiki."""
    titles, texts, row_off = [], [], [0]
    for doc_id in doc_ids:
        page = wiki.get(doc_id)
        if page is not None:
            for line in page["lines"]:
                if line.strip():
                    titles.append(doc_id)
                    texts.append(line)
        row_off.append(len(texts))
    return titles, texts, row_off


@torch.no_grad()
def hybrid_search(model, dense_index, sparse_index, row_off, claims, k, device,
                  bigram_only=False, method="gather", group_off=None, fusion=0.0,
                  tfidf_index=None):
    """Sparse filter, dense rerank for a batch of claims (src/evaluation.py:57-83 feeding
    :110-112), all on the device: the claims' candidate columns (SparseIndex.candidates)
    expanded to their evidence rows (``row_off``, int64 [n_cols + 1] on the device) and
    each claim's ``ctx2vec`` embedding ranked against its own rows only.  Returns
    (scores [Q, k], idx [Q, k] corpus rows, n [Q]) as rerank_topk.  ``method``: "gather",
    "stream" or "auto" (``ShardedDenseIndex.search_candidates``); the row lists are
    ascending by construction, which the stream method needs.  ``group_off`` (int64
    [n_groups + 1] on the device; ``row_off`` itself for pages): the top-k distinct groups,
    each by its best row, and a fourth value groups [Q, k] (``rerank_topk``).

    Over a sharded ``dense_index`` (one with a process group) the call is collective:
    ``claims`` is this rank's slice of the batch (may be empty), ``row_off`` / ``group_off``
    stay in global row ids, and the result covers the whole batch, in rank order
    (``ShardedDenseIndex.search_candidates``).

    ``fusion`` > 0 with a ``tfidf_index`` (a ``SparseIndex`` over the TF-IDF matrix with its
    ``doc_freqs``, as ``TfidfDocRanker`` builds one): the rows are ranked by the FUSED score
    dense + fusion * sparse, where sparse is the claim's TF-IDF score of the row's page
    (``text2spvec`` query vector, ``SparseIndex.candidate_scores`` at the filter's
    candidates) divided by the claim's largest such score -- in [0, 1]; all zeros when that
    maximum is 0 -- cast to fp32 and multiplied by ``fusion`` in fp32.  Every row of a page
    carries the page's value (``expand_ranges(values=)``), which ``search_candidates`` adds
    as its ``bias``.  The returned scores are the fused ones.  ``fusion == 0``: no bias is
    built and the call is the one above."""
    from irc_amd.retrieval import expand_ranges

    if fusion < 0:
        raise ValueError(f"fusion must be >= 0, not {fusion}")
    fused = fusion > 0
    if fused and tfidf_index is None:
        raise ValueError("fusion > 0 needs the TF-IDF index (tfidf_index)")
    bias = None
    if claims:
        q = model.ctx2vec(claims, device)
        cand, off = sparse_index.candidates(claims, bigram_only)
        if fused:
            vecs = [tfidf_index.text2spvec(c) for c in claims]
            page = tfidf_index.candidate_scores([v[0] for v in vecs], [v[1] for v in vecs],
                                                cand, off)
            rows, rows_off, bias = expand_ranges(cand, off, row_off,
                                                 values=fusion_bias(page, off, fusion))
        else:
            rows, rows_off = expand_ranges(cand, off, row_off)
    else:  # a rank with no claim of this batch still joins the collectives
        q = torch.empty((0, dense_index.docs.shape[1]), dtype=torch.float32, device=device)
        rows = torch.empty(0, dtype=torch.int64, device=device)
        rows_off = torch.zeros(1, dtype=torch.int64, device=device)
        if fused:
            bias = torch.empty(0, dtype=torch.float32, device=device)
    kw = {} if group_off is None else {"group_off": group_off}
    if fused:
        kw["bias"] = bias
    return dense_index.search_candidates(q, rows, rows_off, k, method=method, ascending=True,
                                         **kw)


def fusion_bias(page_scores, cand_off, fusion):
    """The per-candidate prior of the fused score: fp64 ``page_scores`` [n_cand] (CSR offsets
    ``cand_off`` int64 [Q + 1]) divided by each query's largest one -- 0 where that maximum
    is not positive --, cast to fp32, times ``fusion`` in fp32.  Pure torch on the tensors'
    device, no host synchronisation."""
    n = page_scores.numel()
    Q = cand_off.numel() - 1
    owner = torch.repeat_interleave(torch.arange(Q, device=page_scores.device),
                                    cand_off[1:] - cand_off[:-1], output_size=n)
    top = torch.zeros(Q, dtype=torch.float64, device=page_scores.device)
    top = top.scatter_reduce(0, owner, page_scores, "amax", include_self=True)[owner]
    norm = torch.where(top > 0, page_scores / top, torch.zeros_like(page_scores))
    return norm.to(torch.float32) * torch.tensor(fusion, dtype=torch.float32,
                                                 device=page_scores.device)


@torch.no_grad()
def predict_hybrid(args, k=100):
    """The reference's two-stage predict: per claim batch the hashed n-gram filter, then
    the bi-encoder's exact top-k over the filter's candidates only.  Prints each batch's
    latency and the evidence recall@k (a claim with no candidates is a miss); returns
    recall@k.  ``args.rerank_method`` (default "auto") picks the scoring method per batch;
    the ranking contract is the same either way.  ``args.index_dtype`` (default "bf16"):
    "fp8" keeps the corpus as e4m3 bytes and ranks the quantised embeddings.
    ``args.fusion_weight`` (main.py --fusion-weight, default 0): above 0 the rows are ranked
    by dense + weight * (the claim's max-normalised TF-IDF page score), ``hybrid_search``'s
    fused score, over the TF-IDF matrix this function opens for its metadata.

    Under data parallelism (``args.dist_group``, main.py under torchrun) the corpus is
    sharded as in ``predict_dense``: rank r encodes and keeps only its contiguous slice of
    the rows, each claim batch is split over the ranks, every rank embeds and filters its
    own claims (the count matrix is small and replicated; ``row_off`` stays in global row
    ids) and ``search_candidates`` gathers the lists, ranks each shard's own candidates and
    merges -- per page with ``--rerank-unit page``.  Every rank receives the whole batch's
    result and scores recall over it; rank 0 prints."""
    from irc_amd.retrieval import shard_bounds

    assert args.ckpt is not None
    group = getattr(args, "dist_group", None)
    world = int(getattr(args, "world_size", 1)) if group is not None else 1
    rank = int(getattr(args, "rank", 0)) if group is not None else 0
    _, model, _, _ = load_model(args.ckpt)
    model = model.to(args.device).eval()
    loader = get_dataloader(args, train=False, distributed=False)
    ds = args.config["dataset"]
    tfidf, metadata = load_sparse_csr(ds["tfidf"])
    count_matrix, _ = load_sparse_csr(ds["inverted_file"])
    if metadata.get("tokenizer", "simple") != "simple":
        raise ValueError("only the DrQA 'simple' tokenizer is supported on this path")
    sparse_index = SparseIndex(count_matrix, ngram=metadata["ngram"], device=args.device)
    fusion = float(getattr(args, "fusion_weight", 0.0))  # main.py --fusion-weight
    tfidf_index = SparseIndex(tfidf, ngram=metadata["ngram"], doc_freqs_=metadata["doc_freqs"],
                              device=args.device) if fusion > 0 else None
    titles, texts, row_off = hybrid_corpus(loader.dataset.wiki, metadata["doc_dict"][1])
    row_off = torch.tensor(row_off, dtype=torch.int64, device=args.device)
    lo, hi = shard_bounds(len(texts), world, rank)
    index = ShardedDenseIndex(encode_corpus(model, texts[lo:hi], args.device), doc_offset=lo,
                              group=group,
                              dtype=getattr(args, "index_dtype", "bf16"))  # main.py --index-dtype
    method = getattr(args, "rerank_method", "auto")  # main.py --rerank-method
    # main.py --rerank-unit: "page" ranks each claim's k best pages, each by its best line
    # (row_off is the page -> row range map), so recall@k is over k pages
    by_page = getattr(args, "rerank_unit", "line") == "page"
    hits = total = 0
    for batch in tqdm(loader, desc="Iteration", disable=rank != 0):
        claims = [d["claim"] for d in batch]
        s = time.time()
        c0, c1 = shard_bounds(len(claims), world, rank)
        # rows: the whole batch, in order
        fuse = {"fusion": fusion, "tfidf_index": tfidf_index} if fusion > 0 else {}
        idx = hybrid_search(model, index, sparse_index, row_off, claims[c0:c1], k, args.device,
                            method=method, group_off=row_off if by_page else None, **fuse)[1]
        torch.cuda.synchronize()
        if rank == 0:
            print(f"batch of {len(claims)} claims: {time.time() - s:.4f}s")
        for d, row in zip(batch, idx.cpu().tolist()):
            gold = {e["title"] for e in d["evidences"]}
            hits += int(any(titles[j] in gold for j in row if j >= 0))
            total += 1
    if rank == 0:
        unit = (" (pages)" if by_page else "") + (f" (fusion weight {fusion:g})" if fusion > 0
                                                  else "")
        print(f"evidence recall@{k}{unit}: {hits / max(total, 1):.4f}")
    return hits / max(total, 1)
