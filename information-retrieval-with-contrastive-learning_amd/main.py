"""Drop-in for the reference main.py (same flags; main.py:14-112).

    python main.py [--config config.yaml] [--data doc|fever] [--gpu 0] [--ckpt X]
                   [--model LSTM|BERT] [--loss InfoNCE] [--opt adam] [--sample uniform|tf_idf]
                   [--seed 1337] [--logdir log] [--ckptdir ckpt] [--retrieval sparse|dense|hybrid]
                   [--rerank-method auto|gather|stream] [--rerank-unit line|page]
                   [--index-dtype bf16|fp8] [--index flat|ivf] [--nlist N] [--nprobe P]
                   [--ivf-list-dtype bf16|fp8] [--fusion-weight W]

Multi-GPU (one process per GPU):
    torchrun --nproc-per-node N --master-addr 127.0.0.1 main.py [same flags]
When the launcher sets WORLD_SIZE > 1, the process group is initialised over RCCL
(backend "nccl") on cuda:LOCAL_RANK before any other GPU call; training is data
parallel (each rank a disjoint slice of the pairs, global in-batch negatives,
gradient all-reduce; logging and checkpoints on rank 0) and ``--retrieval dense`` /
``--retrieval hybrid`` shard the evidence corpus over the ranks.  IRC_DIST_BACKEND=gloo selects gloo
(tests that share one GPU between ranks).

--data doc trains (src.train.train); --data fever runs src.evaluation.predict:
the reference's sparse candidate filter per claim (default) or, with
``--retrieval dense``, the bi-encoder's exact top-k over the evidence corpus, or, with
``--retrieval hybrid``, that top-k over each claim's filter candidates only (the
reference's two stages joined).  With either of the two, ``--rerank-unit page`` ranks the
k best pages, each by its best line, instead of the k best lines.  ``--fusion-weight W``
(hybrid only) ranks by the fused score dense + W * the claim's max-normalised TF-IDF page score.
``--index ivf`` (dense only) clusters the evidence corpus into ``--nlist`` lists and scores
only the ``--nprobe`` lists nearest to each claim -- exactly, so what it trades for speed is
which lists are looked at; ``--ivf-list-dtype fp8`` keeps those lists as e4m3 bytes (half the
bytes a search streams; the probe stays bf16).  The compute runs on the MI355X HIP kernels only:
``--gpu -1`` (CPU) is rejected -- there is no CPU fallback in this build.
"""
import argparse
import os
import random
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def get_args(argv=None):
    p = argparse.ArgumentParser(description="Argument Parser.")
    p.add_argument("--config", type=str, default=os.path.join(HERE, "config.yaml"),
                   help="Path to experiment configuration.")
    p.add_argument("--log", action="store_true", default=False,
                   help="Recording loss and metric scores.")
    p.add_argument("--logdir", default="log", type=str, help="Directory for logging.")
    p.add_argument("--data", default="doc", type=str, help="doc: train, fever: retrieve")
    p.add_argument("--ckptdir", default="ckpt", type=str, help="Checkpoint directory.")
    p.add_argument("--seed", default=1337, type=int, help="Random seed.")
    p.add_argument("--gpu", default="0", type=str, help="GPU id (-1: CPU, not supported)")
    p.add_argument("--ckpt", type=str, help="Path to load target pretrain model")
    p.add_argument("--model", default="LSTM", type=str, choices=["LSTM", "BERT"],
                   help="LSTM: frozen BERT + BiLSTM head (reference); BERT: trainable "
                        "BERT bi-encoder (superset)")
    p.add_argument("--loss", default="InfoNCE", type=str,
                   choices=["InfoNCE", "ProtoNCE", "HProtoNCE"])
    p.add_argument("--opt", default="adam", type=str, choices=["adam", "sgd"])
    p.add_argument("--sample", default="uniform", type=str, choices=["uniform", "tf_idf"])
    p.add_argument("--retrieval", default="sparse", type=str,
                   choices=["sparse", "dense", "hybrid"],
                   help="--data fever: sparse n-gram filter as the reference (default), "
                        "dense bi-encoder top-k (superset), or hybrid: the filter's "
                        "candidates reranked by the bi-encoder (the reference's two stages)")
    p.add_argument("--rerank-method", default="auto", type=str,
                   choices=["auto", "gather", "stream"],
                   help="--retrieval hybrid: how the candidates are scored. gather reads "
                        "each candidate row per claim, stream runs the corpus through the "
                        "MFMA GEMM once per 256 claims and picks the candidates' scores "
                        "(faster for dense lists), auto picks per batch from measured "
                        "crossovers. Same ranking contract either way: the exact top-k over "
                        "the candidates only; scores may differ in the last bits (another "
                        "fp32 summation order)")
    p.add_argument("--rerank-unit", default="line", type=str, choices=["line", "page"],
                   help="--retrieval dense / hybrid: what the top-k counts. line (default): "
                        "the k best evidence lines, several of which may be of one page. "
                        "page: the k best pages, each by its best line (ties: the earlier "
                        "line), collapsed on the device before the select (dense: in the "
                        "scan's GEMM epilogue); the printed recall is then over k pages")
    p.add_argument("--index-dtype", default="bf16", type=str, choices=["bf16", "fp8"],
                   help="--retrieval dense / hybrid: how the evidence corpus is kept in HBM. "
                        "bf16 (default), or fp8: e4m3 bytes at half the size, the claims "
                        "quantised with the same scale per search and the scores those of "
                        "the quantised embeddings")
    p.add_argument("--index", default="flat", type=str, choices=["flat", "ivf"],
                   help="--retrieval dense: flat (default) scans the whole evidence corpus; "
                        "ivf clusters it into --nlist lists (k-means on the device; under a "
                        "launcher each rank over its own slice) and ranks, exactly, only the "
                        "rows of the --nprobe lists nearest to each claim")
    p.add_argument("--nlist", default=1024, type=int,
                   help="--index ivf: lists the corpus (each rank's slice) is clustered into")
    p.add_argument("--nprobe", default=8, type=int,
                   help="--index ivf: lists probed per claim (per shard), 1 .. min(nlist, 1024)")
    p.add_argument("--ivf-list-dtype", default="bf16", type=str, choices=["bf16", "fp8"],
                   help="--index ivf: how the lists' rows are kept in HBM. bf16 (default), or "
                        "fp8: e4m3 bytes at half the size, the claims quantised inside the "
                        "search call and the scores those of the quantised embeddings; the "
                        "centroids and the probe stay bf16, so the same lists are probed")
    p.add_argument("--fusion-weight", default=0.0, type=float,
                   help="--retrieval hybrid: rank each candidate line by dense + W * sparse, "
                        "sparse being the claim's TF-IDF score of the line's page divided by "
                        "the claim's largest (in [0, 1]), added on the device inside the "
                        "candidate top-k. 0 (default): the dense score alone. Works with every "
                        "--rerank-method, --rerank-unit page, --index-dtype fp8 and under "
                        "torchrun")
    args = p.parse_args(argv)
    if not args.fusion_weight >= 0 or args.fusion_weight == float("inf"):
        p.error(f"--fusion-weight must be a finite number >= 0, not {args.fusion_weight}")
    if args.fusion_weight > 0 and args.retrieval != "hybrid":
        p.error("--fusion-weight fuses the sparse filter's score into the dense rerank: it "
                "goes with --retrieval hybrid only")
    if args.ivf_list_dtype != "bf16" and args.index != "ivf":
        p.error("--ivf-list-dtype is the dtype of an IVF index's lists: it goes with --index "
                "ivf only (a flat index takes --index-dtype)")
    if args.index == "ivf":
        if args.retrieval == "hybrid":
            p.error("--index ivf ranks the probed lists, not a candidate filter's rows: it "
                    "goes with --retrieval dense, not hybrid")
        if args.rerank_unit == "page":
            p.error("--index ivf has no per-page unit yet (the rows are permuted): use "
                    "--rerank-unit line")
        if args.index_dtype == "fp8":
            p.error("--index ivf takes --index-dtype bf16 only: e4m3 lists are "
                    "--ivf-list-dtype fp8")
        if args.nlist < 1 or not 1 <= args.nprobe <= min(args.nlist, 1024):
            p.error(f"--index ivf needs --nlist >= 1 and 1 <= --nprobe <= min(nlist, 1024), "
                    f"not nlist={args.nlist} nprobe={args.nprobe}")
    return args


def resolve_device(gpu: str) -> torch.device:
    first = int(gpu.split(",")[0])
    if first < 0:
        raise SystemExit("this build runs on MI355X (HIP) only: --gpu -1 (CPU) has no kernels")
    return torch.device(f"cuda:{first}")


def init_distributed():
    """(group, rank, world, local_rank, created) from the launcher's environment
    (torch.distributed.run / torchrun: WORLD_SIZE, RANK, LOCAL_RANK, MASTER_*), or
    (None, 0, 1, None, False) for a single process; created: this call initialised
    the default process group (main() then also destroys it).  Runs before any other GPU call:
    RCCL's communicator is bound to cuda:LOCAL_RANK (device_id)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return None, 0, 1, None, False
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    backend = os.environ.get("IRC_DIST_BACKEND", "nccl")
    created = not dist.is_initialized()
    if created:
        if backend == "nccl":
            dev = torch.device("cuda", local % max(torch.cuda.device_count(), 1))
            torch.cuda.set_device(dev)
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    return dist.group.WORLD, dist.get_rank(), dist.get_world_size(), local, created


def main(argv=None):
    args = get_args(argv)
    group, rank, world, local, created = init_distributed()
    args.dist_group, args.rank, args.world_size = group, rank, world
    torch.cuda.manual_seed(args.seed)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    with open(args.config, "r") as f:
        args.config = yaml.safe_load(f)
    prec = (args.config.get("bert") or {}).get("precision")
    if prec:
        from irc_amd.precision import set_precision

        set_precision(prec)
    args.device = resolve_device(args.gpu)
    if local is not None:  # one GPU per rank: cuda:LOCAL_RANK (wrapped on a shared box)
        args.device = torch.device("cuda", local % max(torch.cuda.device_count(), 1))
    if args.data == "doc":
        from src.train import train

        train(args)
    elif args.data == "fever":
        from src.evaluation import predict

        predict(args)
    else:
        raise SystemExit(f"unknown --data {args.data!r}")
    if created:
        import torch.distributed as dist

        dist.barrier(group)
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
