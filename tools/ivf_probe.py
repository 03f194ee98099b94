"""Cluster-pruned dense search (IVFDenseIndex) against the exact scan: what a probe buys.

    python tools/ivf_probe.py [--n 250000] [--d 768] [--k 100] [--out profiles/ivf_probe_native.json]
    python tools/ivf_probe.py --tables profiles/ivf_probe_native.json   # DESIGN.md's table
    python tools/ivf_probe.py --dtype fp8 [--n 250000 1000000]          # e4m3 lists, below

One MI355X, a clustered synthetic shard (N x D bf16 unit rows around N / 64 random centres,
larger than the Infinity Cache at the default size), an IVFDenseIndex trained on it per nlist.
Per cell (nlist, nprobe, Q), k = 100, by the method of tools/rerank_probe.py -- HIP-event
windows of back-to-back calls, the variants alternating window by window in one process,
medians and min-max over the rounds, the calls of a window cycling through `sets` independent
query draws so that no call finds its rows of the call before in the Infinity Cache:

  * ivf      IVFDenseIndex.search(q, k, nprobe): probe, plan, scoring and select issued by
             one native call (irc_ivf_search), the plan built on the device, no host
             synchronisation;
  * torchplan  the same search with the plan built in torch: index.probe, then ivf_topk
             (retrieval.ivf_plan's launches, its sort and the one host synchronisation) --
             the call as it was before the native one, and what the native one is accepted
             against: its median no higher than this one's median plus this one's own spread
             (the range of its window medians over the rounds), results identical;
  * scan     the exact search of the same shard (retrieval.scan_topk), the yardstick;
  * compose  what the parent commit could build from its own parts: the same probe, then
             expand_ranges over the lists and rerank_topk(method="gather") -- context for
             where the new scoring kernel matters;
  * probe    the probe alone (scan_topk over the centroids), a call time.

Then, in a profiled pass of the ivf call, the plan kernels' time (the clear and the kernels of
irc_ivf_plan as one record) and the scoring and select kernels' own times (the library's
per-launch events), and from the plan the bytes the scoring pass streams -- the sum
over lists of chunks x rows x D x 2 -- over the scoring time.  recall@k of the ivf result
against the exact scan's is reported per cell, never asserted.  Prints a table to stderr and
writes ONE JSON object to --out.

``--dtype fp8`` (default --out profiles/ivf_fp8_probe.json) measures e4m3 lists by the same
method on the same cells, the variants again alternating window by window in one process:

  * fp8      ``index.to_fp8().search(q, k, nprobe)``: one irc_ivf_search_fp8 call;
  * bf16     ``index.search(q, k, nprobe)`` of the SAME index -- the same clustering, the same
             probe -- which is what the fp8 call is accepted against: its median no higher than
             this one's median plus this one's own spread, and the fp8 results identical every
             time they are computed over the alternations;
  * scan8    the exact fp8 search of the same shard (``ShardedDenseIndex(dtype="fp8")``'s call:
             the queries quantised, then scan_topk_fp8).

Then each call's scoring kernel in a profiled pass of its own, the bytes each streams (the
bf16 figure halved), the achieved bytes/s of both and their ratio; recall@k of the fp8 result
is against the fp8 exact scan's."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "information-retrieval-with-contrastive-learning_amd"))

import torch  # noqa: E402


def _window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def _prof(lib, name):
    tot, cnt, work = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_double(0)
    lib.irc_prof_query(name, ctypes.byref(tot), ctypes.byref(cnt), ctypes.byref(work))
    return tot.value * 1e3 / max(cnt.value, 1)  # us per launch


def tables(path):
    with open(path) as f:
        r = json.load(f)
    for shape in r["shapes"]:
        print(f"\n{shape['N']:,} x {shape['D']} bf16, k = {r['k']}; call times in us "
              "(median of the windows)\n")
        if "torchplan_call_us" not in shape["cells"][0]:
            _tables_before_the_native_call(shape)
            continue
        print("| nlist | nprobe | Q | ivf call | torch-plan call (spread) | accepted | "
              "probe call | plan kernels | score kernel | select kernel | scan call | "
              "parent's parts | streamed MB | score TB/s | shard touched | recall@k | "
              "ivf / scan |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        for c in shape["cells"]:
            lo, hi = c["torchplan_call_us_minmax"]
            print(f"| {c['nlist']} | {c['nprobe']} | {c['Q']} | {c['ivf_call_us']:.0f} | "
                  f"{c['torchplan_call_us']:.0f} ({hi - lo:.0f}) | "
                  f"{'yes' if c['accepted'] else 'NO'}{'' if c['identical'] else ', DIFFERS'} | "
                  f"{c['probe_call_us']:.0f} | {c['plan_kernels_us']:.0f} | "
                  f"{c['score_kernel_us']:.0f} | "
                  f"{c['select_kernel_us']:.0f} | {c['scan_call_us']:.0f} | "
                  f"{c['compose_call_us']:.0f} | {c['streamed_bytes'] / 1e6:.1f} | "
                  f"{c['score_TBps']:.2f} | {100 * c['touched_frac']:.1f} % | "
                  f"{c['recall']:.3f} | {c['ivf_call_us'] / c['scan_call_us']:.2f} |")


def tables_fp8(r):
    for shape in r["shapes"]:
        print(f"\n{shape['N']:,} x {shape['D']} e4m3 lists, k = {r['k']}; call times in us "
              "(median of the windows)\n")
        print("| nlist | nprobe | Q | fp8 ivf call | bf16 ivf call (spread) | accepted | "
              "fp8 scan call | fp8 score kernel | bf16 score kernel | bf16 / fp8 kernel | "
              "fp8 streamed MB | fp8 score TB/s | bf16 score TB/s | recall@k vs fp8 scan | "
              "fp8 ivf / fp8 scan |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        for c in shape["cells"]:
            lo, hi = c["bf16_call_us_minmax"]
            print(f"| {c['nlist']} | {c['nprobe']} | {c['Q']} | {c['fp8_call_us']:.0f} | "
                  f"{c['bf16_call_us']:.0f} ({hi - lo:.0f}) | "
                  f"{'yes' if c['accepted'] else 'NO'}{'' if c['identical'] else ', DIFFERS'} | "
                  f"{c['scan8_call_us']:.0f} | {c['fp8_score_kernel_us']:.0f} | "
                  f"{c['bf16_score_kernel_us']:.0f} | "
                  f"{c['bf16_score_kernel_us'] / max(c['fp8_score_kernel_us'], 1e-9):.2f} | "
                  f"{c['fp8_streamed_bytes'] / 1e6:.1f} | {c['fp8_score_TBps']:.2f} | "
                  f"{c['bf16_score_TBps']:.2f} | {c['recall']:.3f} | "
                  f"{c['fp8_call_us'] / c['scan8_call_us']:.2f} |")


def _tables_before_the_native_call(shape):
    """The columns of a result file written before the torchplan variant existed."""
    print("| nlist | nprobe | Q | ivf call | probe call | score kernel | select kernel | "
          "scan call | parent's parts | streamed MB | score TB/s | shard touched | "
          "recall@k | ivf / scan |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for c in shape["cells"]:
        print(f"| {c['nlist']} | {c['nprobe']} | {c['Q']} | {c['ivf_call_us']:.0f} | "
              f"{c['probe_call_us']:.0f} | {c['score_kernel_us']:.0f} | "
              f"{c['select_kernel_us']:.0f} | {c['scan_call_us']:.0f} | "
              f"{c['compose_call_us']:.0f} | {c['streamed_bytes'] / 1e6:.1f} | "
              f"{c['score_TBps']:.2f} | {100 * c['touched_frac']:.1f} % | "
              f"{c['recall']:.3f} | {c['ivf_call_us'] / c['scan_call_us']:.2f} |")


def _clustered(n, d, centres, own, g, dev, chunk=65536):
    """unit(0.5 C[own] + unit(randn)) as bf16, built in chunks on the device."""
    out = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        x = torch.nn.functional.normalize(torch.randn(hi - lo, d, generator=g, device=dev))
        out[lo:hi] = torch.nn.functional.normalize(0.5 * centres[own[lo:hi]] + x).bfloat16()
    return out


def probe_shape(args, n, lib, dev):
    from irc_amd import retrieval

    g = torch.Generator(device=dev).manual_seed(2025)
    ncent = max(n // 64, 1)
    centres = torch.nn.functional.normalize(torch.randn(ncent, args.d, generator=g, device=dev))
    docs = _clustered(n, args.d, centres, torch.randint(0, ncent, (n,), generator=g, device=dev),
                      g, dev)
    cells = []
    for nlist in args.nlist:
        index = retrieval.IVFDenseIndex.train(docs, nlist, niter=args.niter)
        lens = (index.list_off[1:] - index.list_off[:-1])
        for Q in args.q:
            qs = [_clustered(Q, args.d, centres,
                             torch.randint(0, ncent, (Q,), generator=g, device=dev), g, dev)
                  for _ in range(args.sets)]
            for nprobe in args.nprobe:
                def cycling(fn):
                    turn = [0]

                    def call():
                        turn[0] += 1
                        return fn(qs[turn[0] % args.sets])
                    return call

                def compose(q):
                    pr = index.probe(q, nprobe).to(torch.int64).reshape(-1)
                    off = torch.arange(Q + 1, device=dev, dtype=torch.int64) * nprobe
                    rows, rows_off = retrieval.expand_ranges(pr, off, index.list_off)
                    return retrieval.rerank_topk(q, index.docs, rows, rows_off, args.k)

                def torchplan(q):
                    return retrieval.ivf_topk(q, index.docs, index.row_id, index.list_off,
                                              index.probe(q, nprobe), args.k,
                                              index.max_list_rows, ws_tag="ivf_torchplan")

                timed = [("ivf", cycling(lambda q: index.search(q, args.k, nprobe=nprobe))),
                         ("torchplan", cycling(torchplan)),
                         ("scan", cycling(lambda q: retrieval.scan_topk(q, docs, args.k))),
                         ("compose", cycling(compose)),
                         ("probe", cycling(lambda q: index.probe(q, nprobe)))]
                est = {}
                for name, fn in timed:
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    est[name] = _window_ms(fn, args.sets)
                reps = {m: max(args.sets, min(2000, int(args.window_ms / max(est[m], 1e-3))))
                        for m in est}
                for m in reps:
                    reps[m] -= reps[m] % args.sets  # every draw equally often
                t = {m: [] for m, _ in timed}
                for _ in range(args.rounds):  # alternate them window by window
                    for m, fn in timed:
                        t[m].append(_window_ms(fn, reps[m]))
                # kernel times in a pass of their own (per-launch events slow the host)
                lib.irc_prof_reset()
                lib.irc_prof_enable(1)
                for _ in range(min(reps["ivf"], 4 * args.sets)):
                    timed[0][1]()
                torch.cuda.synchronize()
                lib.irc_prof_enable(0)
                score_us, select_us = _prof(lib, b"ivf_score"), _prof(lib, b"rerank_select")
                plan_us = _prof(lib, b"ivf_plan")
                # from the plans of the draws: bytes streamed, shard touched, recall
                streamed = touched = hit = 0.0
                identical = True
                for q in qs:
                    identical = identical and all(
                        torch.equal(a, b) for a, b in
                        zip(index.search(q, args.k, nprobe=nprobe), torchplan(q)))
                    pr = index.probe(q, nprobe)
                    plan = retrieval.ivf_plan(pr, index.list_off)
                    chunks = plan["chunk_off"][1:] - plan["chunk_off"][:-1]
                    streamed += float((chunks * lens).sum().item()) * args.d * 2
                    touched += float(lens[chunks > 0].sum().item()) / n
                    got = index.search(q, args.k, probe=pr)[1]
                    want = retrieval.scan_topk(q, docs, args.k)[1]
                    hit += float((got.unsqueeze(2) == want.unsqueeze(1)).any(dim=2)
                                 .float().mean().item())
                cell = {"nlist": nlist, "nprobe": nprobe, "Q": Q,
                        "max_list_rows": index.max_list_rows,
                        "streamed_bytes": streamed / args.sets,
                        "touched_frac": touched / args.sets, "recall": hit / args.sets,
                        "score_kernel_us": score_us, "select_kernel_us": select_us,
                        "plan_kernels_us": plan_us, "identical": identical,
                        "score_TBps": streamed / args.sets / (score_us * 1e-6) / 1e12
                        if score_us else 0.0, "reps": reps}
                for m in t:
                    cell[f"{m}_call_us"] = statistics.median(t[m]) * 1e3
                    cell[f"{m}_call_us_minmax"] = [min(t[m]) * 1e3, max(t[m]) * 1e3]
                spread = max(t["torchplan"]) - min(t["torchplan"])
                cell["accepted"] = bool(identical and statistics.median(t["ivf"]) <=
                                        statistics.median(t["torchplan"]) + spread)
                cells.append(cell)
                print(f"N={n} nlist={nlist:5d} nprobe={nprobe:3d} Q={Q:5d}  ivf "
                      f"{cell['ivf_call_us']:8.1f} us (torch plan {cell['torchplan_call_us']:8.1f}"
                      f"{'' if cell['accepted'] else ' NOT ACCEPTED'}; probe "
                      f"{cell['probe_call_us']:6.1f}, plan {plan_us:6.1f}, score "
                      f"{score_us:8.1f}, select {select_us:7.1f})  scan "
                      f"{cell['scan_call_us']:8.1f} us  parts {cell['compose_call_us']:9.1f} us  "
                      f"{cell['streamed_bytes'] / 1e6:8.1f} MB {cell['score_TBps']:5.2f} TB/s  "
                      f"recall {cell['recall']:.3f}", file=sys.stderr, flush=True)
        del index
    return {"N": n, "D": args.d, "centres": ncent, "cells": cells}


def probe_shape_fp8(args, n, lib, dev):
    """The cells of probe_shape with e4m3 lists against the bf16 lists of the same index."""
    from irc_amd import retrieval

    g = torch.Generator(device=dev).manual_seed(2025)
    ncent = max(n // 64, 1)
    centres = torch.nn.functional.normalize(torch.randn(ncent, args.d, generator=g, device=dev))
    docs = _clustered(n, args.d, centres, torch.randint(0, ncent, (n,), generator=g, device=dev),
                      g, dev)
    scale = retrieval.FP8_SCALE
    docs8 = retrieval.quantize_fp8(docs, scale)
    cells = []
    for nlist in args.nlist:
        index = retrieval.IVFDenseIndex.train(docs, nlist, niter=args.niter)
        index8 = index.to_fp8(scale)
        lens = (index.list_off[1:] - index.list_off[:-1])
        for Q in args.q:
            qs = [_clustered(Q, args.d, centres,
                             torch.randint(0, ncent, (Q,), generator=g, device=dev), g, dev)
                  for _ in range(args.sets)]
            for nprobe in args.nprobe:
                def cycling(fn):
                    turn = [0]

                    def call():
                        turn[0] += 1
                        return fn(qs[turn[0] % args.sets])
                    return call

                def scan8(q):
                    return retrieval.scan_topk_fp8(retrieval.quantize_fp8(q, scale), docs8,
                                                   args.k, 0, 1.0 / (scale * scale))

                timed = [("fp8", cycling(lambda q: index8.search(q, args.k, nprobe=nprobe))),
                         ("bf16", cycling(lambda q: index.search(q, args.k, nprobe=nprobe))),
                         ("scan8", cycling(scan8))]
                est = {}
                for name, fn in timed:
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    est[name] = _window_ms(fn, args.sets)
                reps = {m: max(args.sets, min(2000, int(args.window_ms / max(est[m], 1e-3))))
                        for m in est}
                for m in reps:
                    reps[m] -= reps[m] % args.sets  # every draw equally often
                first = [tuple(x.clone() for x in index8.search(q, args.k, nprobe=nprobe))
                         for q in qs]
                identical = True
                t = {m: [] for m, _ in timed}
                for _ in range(args.rounds):  # alternate them window by window
                    for m, fn in timed:
                        t[m].append(_window_ms(fn, reps[m]))
                    # the fp8 results again, between the alternations
                    identical = identical and all(
                        torch.equal(a, b) for q, want in zip(qs, first)
                        for a, b in zip(index8.search(q, args.k, nprobe=nprobe), want))
                # kernel times in passes of their own (per-launch events slow the host)
                kern = {}
                for m, record in (("fp8", b"ivf_score_fp8"), ("bf16", b"ivf_score")):
                    fn = dict(timed)[m]
                    lib.irc_prof_reset()
                    lib.irc_prof_enable(1)
                    for _ in range(min(reps[m], 4 * args.sets)):
                        fn()
                    torch.cuda.synchronize()
                    lib.irc_prof_enable(0)
                    kern[m] = _prof(lib, record)
                streamed = hit = 0.0
                for q in qs:
                    plan = retrieval.ivf_plan(index.probe(q, nprobe), index.list_off)
                    chunks = plan["chunk_off"][1:] - plan["chunk_off"][:-1]
                    streamed += float((chunks * lens).sum().item()) * args.d
                    got = index8.search(q, args.k, nprobe=nprobe)[1]
                    want = scan8(q)[1]
                    hit += float((got.unsqueeze(2) == want.unsqueeze(1)).any(dim=2)
                                 .float().mean().item())
                streamed /= args.sets
                cell = {"nlist": nlist, "nprobe": nprobe, "Q": Q,
                        "max_list_rows": index.max_list_rows, "fp8_streamed_bytes": streamed,
                        "bf16_streamed_bytes": 2 * streamed, "recall": hit / args.sets,
                        "fp8_score_kernel_us": kern["fp8"], "bf16_score_kernel_us": kern["bf16"],
                        "fp8_score_TBps": streamed / (kern["fp8"] * 1e-6) / 1e12
                        if kern["fp8"] else 0.0,
                        "bf16_score_TBps": 2 * streamed / (kern["bf16"] * 1e-6) / 1e12
                        if kern["bf16"] else 0.0, "identical": identical, "reps": reps}
                for m in t:
                    cell[f"{m}_call_us"] = statistics.median(t[m]) * 1e3
                    cell[f"{m}_call_us_minmax"] = [min(t[m]) * 1e3, max(t[m]) * 1e3]
                spread = max(t["bf16"]) - min(t["bf16"])
                cell["accepted"] = bool(identical and statistics.median(t["fp8"]) <=
                                        statistics.median(t["bf16"]) + spread)
                cells.append(cell)
                print(f"N={n} nlist={nlist:5d} nprobe={nprobe:3d} Q={Q:5d}  fp8 "
                      f"{cell['fp8_call_us']:8.1f} us (bf16 {cell['bf16_call_us']:8.1f}"
                      f"{'' if cell['accepted'] else ' NOT ACCEPTED'}; score fp8 "
                      f"{kern['fp8']:8.1f}, bf16 {kern['bf16']:8.1f})  fp8 scan "
                      f"{cell['scan8_call_us']:8.1f} us  {streamed / 1e6:8.1f} MB "
                      f"{cell['fp8_score_TBps']:5.2f} / {cell['bf16_score_TBps']:5.2f} TB/s  "
                      f"recall {cell['recall']:.3f}", file=sys.stderr, flush=True)
        del index, index8
    return {"N": n, "D": args.d, "centres": ncent, "cells": cells}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[250_000])
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nlist", type=int, nargs="*", default=[1024, 4096])
    ap.add_argument("--nprobe", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--q", type=int, nargs="*", default=[1, 16, 64, 256, 1024])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40.0, help="timed work per window")
    ap.add_argument("--sets", type=int, default=4, help="independent query draws per cell")
    ap.add_argument("--niter", type=int, default=10, help="k-means iterations of the build")
    ap.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: e4m3 lists against the bf16 lists of the same index")
    ap.add_argument("--out", default=None,
                    help="default profiles/ivf_probe_native.json, or with --dtype fp8 "
                         "profiles/ivf_fp8_probe.json")
    ap.add_argument("--tables", metavar="FILE", help="print the tables of a result file")
    args = ap.parse_args()
    if args.tables:
        with open(args.tables) as f:
            r = json.load(f)
        return tables_fp8(r) if r.get("probe", "").startswith("ivf_fp8") else tables(args.tables)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ivf_fp8_probe.json" if args.dtype == "fp8"
                                else "ivf_probe_native.json")
    if not torch.cuda.is_available():
        raise SystemExit("ivf_probe measures on a HIP device; none is visible")
    from irc_amd import _lib

    lib = _lib.load()
    dev = torch.device("cuda:0")
    one = probe_shape_fp8 if args.dtype == "fp8" else probe_shape
    shapes = [one(args, n, lib, dev) for n in args.n]
    result = {"probe": "ivf_fp8_bf16_scan8" if args.dtype == "fp8" else
              "ivf_native_torchplan_scan_compose", "device": torch.cuda.get_device_name(0),
              "k": args.k, "rounds": args.rounds, "window_ms": args.window_ms, "sets": args.sets,
              "kmeans_niter": args.niter, "shapes": shapes}
    with open(args.out, "w") as f:
        json.dump(result, f)
        f.write("\n")


if __name__ == "__main__":
    main()
