"""Candidate-restricted top-k, gathered and streamed, against the full scan: where they
cross.

    python tools/rerank_probe.py [--n 250000] [--d 768] [--k 100] [--rounds 10] [--sets 4]
    python tools/rerank_probe.py --tables profiles/rerank_probe.json   # the documents' tables
    python tools/rerank_probe.py --tables profiles/rerank_stream_probe.json  # + stream table
    python tools/rerank_probe.py --dtype fp8 > profiles/rerank_fp8_probe.json  # e4m3 shard
    python tools/rerank_probe.py --tables profiles/rerank_fp8_probe.json  # + fp8 / bf16 table
    python tools/rerank_probe.py --grouped [--dtype fp8]   # top-k per group, see below
    python tools/rerank_probe.py --tables profiles/rerank_group_probe.json
    python tools/rerank_probe.py --merge > profiles/rerank_merge_probe.json  # see below
    python tools/rerank_probe.py --tables profiles/rerank_merge_probe.json
    python tools/rerank_probe.py --bias [--dtype fp8] [--grouped] [--parent-lib SO]  # see below
    python tools/rerank_probe.py --tables profiles/rerank_bias_probe.json

One MI355X, the C3 shard (250k x 768 bf16, larger than the Infinity Cache), random
ascending candidate lists of 0.1 / 1 / 5 / 25 % of the shard per query, Q in {1, 16, 64,
256}.  Per cell: the rerank call (retrieval.rerank_topk) and the scan call
(retrieval.scan_topk, same Q, same shard) timed with HIP events around windows of
back-to-back calls (100 ms of work each), the two alternating round by round in one
process (median over the rounds); the rerank calls of a window cycle through `sets`
independent draws of the lists, as a serving loop's batches would bring new lists; then, in a separate profiled pass, the scoring and select kernels' own times
(the library's per-launch events) and the scoring pass's achieved bytes/s, n_cand * D * 2
over its time, beside the 5.5-5.8 TB/s whole-row gather rate of 1,152-2,304-byte rows.
The streamed method (rerank_topk(method="stream", ascending=True)) is a third party to the
same alternation -- same windows, same list draws -- with its own profiled pass
(rerank_stream_score, rerank_select) and a gather-against-stream crossover per Q
(``crossover_frac_stream``, the constants of retrieval.rerank_method).
``--dtype fp8``: the same cells on the same shard quantised to e4m3 (quantize_fp8, scale
16): rerank_topk_fp8 gathered and streamed and scan_topk_fp8 take the three places above,
and the bf16 gathered and streamed calls of the same cells and list draws join the
alternation window by window (``bf16_rerank_call_us``, ``bf16_stream_call_us``), so every
fp8 time stands beside the bf16 time of the same run.  The crossovers of that file are the
constants of retrieval.rerank_method(dtype="fp8").
``--grouped``: the same cells and list draws, the grouped call (rerank_topk(group_off=...),
pages of a fixed-seed draw, mean about 10 rows) alternating with the ungrouped call, gathered
and streamed; profiles/rerank_group_probe.json holds the bf16 and the fp8 run's lines under
"bf16" and "fp8".
``--merge``: the reduce step of a sharded call, no scoring: Q = 256 queries, P per-shard
lists of kin = kout entries each, P x kin in (2, 100), (8, 100), (8, 1024) -- the call time
of topk_merge (irc_topk_merge) and of topk_merge_grouped (irc_topk_merge_grouped) on the
same lists, alternating window by window, and the grouped merge's two kernels from a
profiled pass.  What the merge adds to a sharded search_candidates.
``--scan-grouped [--dtype fp8]``: the dense scan per page, ShardedDenseIndex.search(group_off=
...), on the same shard and page draw at Q in {1, 16, 64, 256}, alternating with search (the k
best lines) and with the candidate route to the same pages, search_candidates(method="stream",
group_off=...) over lists of ALL rows; profiles/scan_group_probe.json holds the bf16 and the
fp8 run's lines under "bf16" and "fp8" (``--tables`` prints both).
``--bias [--dtype fp8] [--grouped]``: the biased call (rerank_topk(bias=...), a fixed-seed
fp32 bias per candidate) beside the unbiased call in the same cells and list draws, gathered
and streamed, alternating window by window; with ``--grouped`` both carry the page map of
``--grouped``.  ``--parent-lib SO`` (a libirc_hip.so built from the parent commit) adds the
A/B of the unbiased calls: the same native entry of that library and of this tree's, called
through ctypes on the same buffers, join the alternation (``parent_*`` / ``this_*``), and a
cell is accepted when this tree's median is no higher than the parent's median plus the
parent's own min-max window spread of that run (``ab_ok``).  profiles/rerank_bias_probe.json
holds the runs' lines under "bf16", "fp8", "bf16_grouped", "fp8_grouped".
Prints a table to stderr and ONE JSON line to stdout."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "information-retrieval-with-contrastive-learning_amd"))

import torch  # noqa: E402

GATHER_TBS = (5.5, 5.8)  # whole-row gather, 1,152-2,304-B rows


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
    n = max(cnt.value, 1)
    return tot.value * 1e3 / n, work.value / n  # us per launch, work per launch


def _crossover(rows, num, den):
    """Candidate fraction where rows[num] / rows[den] passes 1, log-log interpolated between
    the two measured fractions that bracket it; "< f" / "> f" when it never does."""
    import math

    row = sorted(rows, key=lambda c: c["frac"])
    r = [math.log(c[num] / c[den]) for c in row]
    val = None
    if r and r[0] > 0:
        val = f"< {row[0]['frac']}"
    elif r and r[-1] < 0:
        val = f"> {row[-1]['frac']}"
    for a, b, ra, rb in zip(row, row[1:], r, r[1:]):
        if ra <= 0 < rb:
            w = -ra / (rb - ra)
            val = math.exp(math.log(a["frac"]) + w * (math.log(b["frac"]) - math.log(a["frac"])))
    return val


def stream_tables(r):
    """The stream method's table of DESIGN.md 6e: per cell the stream call, the share of
    it that is the select kernel, and its ratio to the design's floor, scan call + select
    kernel."""
    cells = r["cells"]
    print("| Q | candidates / query | gather call | stream call | pick kernels | "
          "select kernel | select share | scan call | stream / (scan + select) |\n"
          "|---|---|---|---|---|---|---|---|---|")
    for c in cells:
        print(f"| {c['Q']} | {c['cand_per_query']:,} ({100 * c['frac']:g}%) | "
              f"{c['rerank_call_us']:,.1f} | {c['stream_call_us']:,.1f} | "
              f"{c['stream_score_kernel_us']:,.1f} | {c['stream_select_kernel_us']:.1f} | "
              f"{100 * c['stream_select_share']:.0f}% | {c['scan_call_us']:.1f} | "
              f"{c['stream_over_floor']:.2f} |")
    print()
    qs = sorted({c["Q"] for c in cells})
    print("    candidates per query  " + "".join(f"{'Q = ' + str(q):>18}" for q in qs))
    for frac in sorted({c["frac"] for c in cells}):
        row = {c["Q"]: c for c in cells if c["frac"] == frac}
        n = next(iter(row.values()))["cand_per_query"]
        print(f"    {n:>8,} ({100 * frac:g} %)".ljust(26) + "".join(
            f"{row[q]['rerank_call_us']:>9,.0f} / {row[q]['stream_call_us']:<6,.0f}" for q in qs))
    print()
    if r.get("dtype") == "fp8":
        print("| Q | candidates / query | fp8 gather call | bf16 gather call | fp8 score kernel | "
              "fp8 stream call | bf16 stream call | fp8 pick kernels | fp8 scan call |\n"
              "|---|---|---|---|---|---|---|---|---|")
        for c in cells:
            print(f"| {c['Q']} | {c['cand_per_query']:,} ({100 * c['frac']:g}%) | "
                  f"{c['rerank_call_us']:,.1f} | {c['bf16_rerank_call_us']:,.1f} | "
                  f"{c['score_kernel_us']:,.1f} | {c['stream_call_us']:,.1f} | "
                  f"{c['bf16_stream_call_us']:,.1f} | {c['stream_score_kernel_us']:,.1f} | "
                  f"{c['scan_call_us']:.1f} |")
        print()
        slower = [(c["Q"], c["frac"], m) for c in cells for m in ("rerank", "stream")
                  if c[f"{m}_call_us"] > c[f"bf16_{m}_call_us"]]
        print("cells where the fp8 call is slower than its bf16 counterpart:", slower or "none")
        print()
    print("gather-against-stream crossover:", r["crossover_frac_stream"])
    worst = max(cells, key=lambda c: c["spread_pct"]["stream"])
    print(f"largest min-max spread of the stream windows: {worst['spread_pct']['stream']:.2f}% "
          f"(Q = {worst['Q']}, {100 * worst['frac']:g}%); rounds per cell: {r['rounds']}")
    print()


def tables(path):
    """The tables of DESIGN.md 6e and of the search_candidates docstring, from a recorded
    JSON line (no device needed): what the documents quote is what the file holds."""
    with open(path) as f:
        r = json.load(f)
    cells = r["cells"]
    if "crossover_frac_stream" in r:
        stream_tables(r)
    print("| Q | candidates / query | rerank call | scoring kernel | scoring TB/s | "
          "select kernel | scan call |\n|---|---|---|---|---|---|---|")
    for c in cells:
        print(f"| {c['Q']} | {c['cand_per_query']:,} ({100 * c['frac']:g}%) | "
              f"{c['rerank_call_us']:,.1f} | {c['score_kernel_us']:,.1f} | "
              f"{c['score_TBps']:.2f} | {c['select_kernel_us']:.1f} | {c['scan_call_us']:.1f} |")
    print()
    qs = sorted({c["Q"] for c in cells})
    print("    candidates per query  " + "".join(f"{'Q = ' + str(q):>16}" for q in qs))
    for frac in sorted({c["frac"] for c in cells}):
        row = {c["Q"]: c for c in cells if c["frac"] == frac}
        n = next(iter(row.values()))["cand_per_query"]
        print(f"    {n:>8,} ({100 * frac:g} %)".ljust(26) + "".join(
            f"{row[q]['rerank_call_us']:>9,.0f} / {row[q]['scan_call_us']:<4.0f}" for q in qs))
    print()
    print("crossover:", r["crossover_frac"])
    for m in ("rerank", "scan"):
        worst = max(cells, key=lambda c: c["spread_pct"][m])
        print(f"largest min-max spread of the {m} windows: {worst['spread_pct'][m]:.2f}% "
              f"(Q = {worst['Q']}, {100 * worst['frac']:g}%)")
    big = [c for c in cells if c["n_cand"] >= 160000]
    print(f"scoring TB/s at n_cand >= 160k: {min(c['score_TBps'] for c in big):.2f}-"
          f"{max(c['score_TBps'] for c in big):.2f}")
    longest = [c for c in cells if c["cand_per_query"] == max(x["cand_per_query"] for x in cells)]
    print(f"select kernel at {longest[0]['cand_per_query']:,} keys: "
          f"{min(c['select_kernel_us'] for c in longest):.1f}-"
          f"{max(c['select_kernel_us'] for c in longest):.1f} us")


def grouped_tables(r):
    """The table of DESIGN.md 6e "Top-k per group": per cell and method the ungrouped call,
    the grouped call on the same lists, their ratio, and the collapse span's own time."""
    print(f"{r['dtype']}: {r['n_groups']:,} groups over {r['N']:,} rows "
          f"(mean {r['N'] / r['n_groups']:.1f}, longest {r['max_group_rows']}), k = {r['k']}\n")
    print("| Q | candidates / query | gather call | gather grouped | ratio | stream call | "
          "stream grouped | ratio | collapse span |\n|---|---|---|---|---|---|---|---|---|")
    for c in r["cells"]:
        print(f"| {c['Q']} | {c['cand_per_query']:,} ({100 * c['frac']:g}%) | "
              f"{c['gather_call_us']:,.1f} | {c['gather_grouped_call_us']:,.1f} | "
              f"{c['gather_ratio']:.3f} | {c['stream_call_us']:,.1f} | "
              f"{c['stream_grouped_call_us']:,.1f} | {c['stream_ratio']:.3f} | "
              f"{c['collapse_span_us']:,.1f} |")
    print()
    worst = max(r["cells"], key=lambda c: max(c["spread_pct"].values()))
    print(f"largest min-max spread of a cell's windows: {max(worst['spread_pct'].values()):.2f}% "
          f"(Q = {worst['Q']}, {100 * worst['frac']:g}%); rounds per cell: {r['rounds']}")


def grouped_probe(args):
    """--grouped: the grouped call (group_off: pages of a fixed-seed draw, mean about 10
    rows) next to the ungrouped call on the same lists, gathered and streamed, alternating
    window by window; the collapse span (memset excluded: the two collapse phases) from a
    profiled pass of its own.  ONE JSON line to stdout."""
    from irc_amd import _lib, retrieval

    fp8 = args.dtype == "fp8"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2025)
    docs = torch.nn.functional.normalize(
        torch.randn(args.n, args.d, generator=g)).bfloat16().to(dev)
    torch.manual_seed(2025)
    if fp8:
        docs = retrieval.quantize_fp8(docs)
    descale = 1.0 / (retrieval.FP8_SCALE * retrieval.FP8_SCALE)
    # page sizes: 1 + an exponential draw of mean 9.5, rounded down -- mean about 10 rows
    sizes = 1 + torch.empty(args.n, dtype=torch.float64).exponential_(1 / 9.5, generator=g).long()
    ends = torch.cumsum(sizes, 0)
    ends = ends[: int((ends < args.n).sum())]
    group_off = torch.cat([torch.zeros(1, dtype=torch.int64), ends,
                           torch.tensor([args.n])]).to(dev)
    max_rows = int((group_off[1:] - group_off[:-1]).max())
    cells = []
    for Q in args.q:
        qq = torch.nn.functional.normalize(
            torch.randn(Q, args.d, generator=g)).bfloat16().to(dev)
        if fp8:
            qq = retrieval.quantize_fp8(qq)
        for frac in args.frac:
            n = max(1, int(round(frac * args.n)))
            cands = [torch.cat([torch.randperm(args.n, device=dev)[:n].sort().values
                                for _ in range(Q)]).to(torch.int32) for _ in range(args.sets)]
            off = torch.arange(Q + 1, device=dev, dtype=torch.int64) * n

            def make(method, go):
                counter = [0]

                def call():
                    counter[0] += 1
                    c = cands[counter[0] % args.sets]
                    if fp8:
                        return retrieval.rerank_topk_fp8(qq, docs, c, off, args.k, 0, descale,
                                                         method=method, ascending=True,
                                                         group_off=go)
                    return retrieval.rerank_topk(qq, docs, c, off, args.k, method=method,
                                                 ascending=True, group_off=go)
                return call

            timed = [(f"{m}{s}", make(m, go)) for m in ("gather", "stream")
                     for s, go in (("", None), ("_grouped", group_off))]
            est = {}
            for name, fn in timed:
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                est[name] = _window_ms(fn, 5)
            reps = {m: max(2 * args.sets, min(4000, int(args.window_ms / max(est[m], 1e-3))))
                    for m in est}
            for m in reps:
                reps[m] -= reps[m] % args.sets  # every draw equally often
            t = {m: [] for m, _ in timed}
            for _ in range(args.rounds):  # alternate them window by window
                for m, fn in timed:
                    t[m].append(_window_ms(fn, reps[m]))
            lib.irc_prof_reset()
            lib.irc_prof_enable(1)
            for _ in range(min(reps["gather_grouped"], 12 * args.sets)):
                timed[1][1]()
            torch.cuda.synchronize()
            lib.irc_prof_enable(0)
            collapse_us, _ = _prof(lib, b"rerank_collapse")
            med = {m: statistics.median(t[m]) * 1e3 for m in t}
            cell = {"Q": Q, "frac": frac, "cand_per_query": n, "n_cand": Q * n,
                    "collapse_span_us": collapse_us, "reps": reps,
                    "spread_pct": {m: 100.0 * (max(t[m]) - min(t[m])) / statistics.median(t[m])
                                   for m in t}}
            for m in t:
                cell[f"{m}_call_us"] = med[m]
                cell[f"{m}_call_us_minmax"] = [min(t[m]) * 1e3, max(t[m]) * 1e3]
            for m in ("gather", "stream"):
                cell[f"{m}_ratio"] = med[f"{m}_grouped"] / med[m]
            cells.append(cell)
            print(f"Q={Q:4d} frac={frac:6.3f} n_cand={Q * n:9d}  gather {med['gather']:9.1f} / "
                  f"grouped {med['gather_grouped']:9.1f} us ({cell['gather_ratio']:.3f})  stream "
                  f"{med['stream']:9.1f} / grouped {med['stream_grouped']:9.1f} us "
                  f"({cell['stream_ratio']:.3f})  collapse {collapse_us:7.1f} us",
                  file=sys.stderr, flush=True)
    print(json.dumps({"probe": "rerank_grouped", "device": torch.cuda.get_device_name(0),
                      "dtype": args.dtype, "N": args.n, "D": args.d, "k": args.k,
                      "rounds": args.rounds, "window_ms": args.window_ms, "sets": args.sets,
                      "n_groups": int(group_off.numel() - 1), "max_group_rows": max_rows,
                      "cells": cells}))


def scan_group_tables(r):
    """The table of DESIGN.md 6e "Dense scan per group": per Q the line scan (a), the grouped
    scan (b) and the candidate route over all-rows lists (c), and (b)'s two spans."""
    print(f"{r['dtype']}: {r['n_groups']:,} groups over {r['N']:,} rows "
          f"(mean {r['N'] / r['n_groups']:.1f}, longest {r['max_group_rows']}), k = {r['k']}\n")
    print("| Q | (a) search, lines | (b) search, pages | (b) / (a) | (c) candidates, all rows | "
          "(c) / (b) | (b) memset + GEMM + group epilogue | share of (b) | (b) select |\n"
          "|---|---|---|---|---|---|---|---|---|")
    for c in r["cells"]:
        print(f"| {c['Q']} | {c['lines_call_us']:,.1f} | {c['pages_call_us']:,.1f} | "
              f"{c['pages_over_lines']:.2f} | {c['route_call_us']:,.1f} | "
              f"{c['route_over_pages']:.2f} | {c['group_span_us']:,.1f} | "
              f"{100 * c['group_span_share']:.0f}% | {c['select_kernel_us']:,.1f} |")
    print()
    worst = max(r["cells"], key=lambda c: max(c["spread_pct"].values()))
    print(f"largest min-max spread of a cell's windows: {max(worst['spread_pct'].values()):.2f}% "
          f"(Q = {worst['Q']}); rounds per cell: {r['rounds']}")


def scan_group_probe(args):
    """--scan-grouped: on the probe's shard and its fixed-seed page draw (mean about 10
    rows), per Q three calls of one ShardedDenseIndex alternating window by window: (a)
    search (the k best lines), (b) search(group_off=...) (the k best pages, the GEMM loop's
    group epilogue), (c) the route to (b)'s answer without it: search_candidates(method=
    "stream", ascending=True, group_off=...) over lists of ALL rows.  Then a profiled pass of
    (b): the span of the memset and the GEMM launch with the group epilogue -- launch events
    cannot time the epilogue apart from the main loop of its own kernel -- and the select.
    ONE JSON line to stdout."""
    from irc_amd import _lib, retrieval

    fp8 = args.dtype == "fp8"
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2025)
    docs = torch.nn.functional.normalize(
        torch.randn(args.n, args.d, generator=g)).bfloat16().to(dev)
    torch.manual_seed(2025)
    index = retrieval.ShardedDenseIndex(docs, dtype=args.dtype)
    del docs
    # page sizes: 1 + an exponential draw of mean 9.5, rounded down -- the draw of --grouped
    sizes = 1 + torch.empty(args.n, dtype=torch.float64).exponential_(1 / 9.5, generator=g).long()
    ends = torch.cumsum(sizes, 0)
    ends = ends[: int((ends < args.n).sum())]
    group_off = torch.cat([torch.zeros(1, dtype=torch.int64), ends,
                           torch.tensor([args.n])]).to(dev)
    max_rows = int((group_off[1:] - group_off[:-1]).max())
    span = b"scan_group_fp8_score" if fp8 else b"scan_group_score"
    cells = []
    for Q in args.q:
        qq = torch.nn.functional.normalize(
            torch.randn(Q, args.d, generator=g)).bfloat16().to(dev)
        cand = torch.arange(args.n, dtype=torch.int32, device=dev).repeat(Q)
        off = torch.arange(Q + 1, device=dev, dtype=torch.int64) * args.n
        timed = [
            ("lines", lambda: index.search(qq, args.k)),
            ("pages", lambda: index.search(qq, args.k, group_off=group_off)),
            ("route", lambda: index.search_candidates(qq, cand, off, args.k, method="stream",
                                                      ascending=True, group_off=group_off)),
        ]
        same = all(torch.equal(x, y) for x, y in zip(timed[1][1](), timed[2][1]()))
        est = {}
        for name, fn in timed:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            est[name] = _window_ms(fn, 5)
        reps = {m: max(4, min(4000, int(args.window_ms / max(est[m], 1e-3)))) for m in est}
        t = {m: [] for m, _ in timed}
        for _ in range(args.rounds):  # alternate them window by window
            for m, fn in timed:
                t[m].append(_window_ms(fn, reps[m]))
        lib.irc_prof_reset()
        lib.irc_prof_enable(1)
        for _ in range(min(reps["pages"], 48)):
            timed[1][1]()
        torch.cuda.synchronize()
        lib.irc_prof_enable(0)
        span_us, _ = _prof(lib, span)
        select_us, _ = _prof(lib, b"rerank_select")
        med = {m: statistics.median(t[m]) * 1e3 for m in t}
        cell = {"Q": Q, "group_span_us": span_us, "select_kernel_us": select_us,
                "group_span_share": span_us / med["pages"],
                "pages_over_lines": med["pages"] / med["lines"],
                "route_over_pages": med["route"] / med["pages"],
                "route_equals_pages_bitwise": bool(same), "reps": reps,
                "spread_pct": {m: 100.0 * (max(t[m]) - min(t[m])) / statistics.median(t[m])
                               for m in t}}
        for m in t:
            cell[f"{m}_call_us"] = med[m]
            cell[f"{m}_call_us_minmax"] = [min(t[m]) * 1e3, max(t[m]) * 1e3]
        cells.append(cell)
        print(f"Q={Q:4d}  lines {med['lines']:9.1f} us  pages {med['pages']:9.1f} us "
              f"({cell['pages_over_lines']:.2f})  all-rows route {med['route']:10.1f} us "
              f"({cell['route_over_pages']:.2f} x pages)  group span {span_us:8.1f} us  select "
              f"{select_us:7.1f} us  same bits {same}", file=sys.stderr, flush=True)
        del cand, off
    print(json.dumps({"probe": "scan_grouped", "device": torch.cuda.get_device_name(0),
                      "dtype": args.dtype, "N": args.n, "D": args.d, "k": args.k,
                      "rounds": args.rounds, "window_ms": args.window_ms,
                      "n_groups": int(group_off.numel() - 1), "max_group_rows": max_rows,
                      "cells": cells}))


def bias_tables(r):
    """The fused-score tables of DESIGN.md 6e from one --bias run: per cell the unbiased /
    biased call and their ratio, gathered and streamed; with a parent library the A/B of the
    unbiased native entries (parent median + its window spread against this tree's median)."""
    qs = sorted({c["Q"] for c in r["cells"]})
    fracs = sorted({c["frac"] for c in r["cells"]})
    cell = {(c["Q"], c["frac"]): c for c in r["cells"]}
    what = f"{r['dtype']}{', per group' if r.get('grouped') else ''}"
    for m in ("gather", "stream"):
        print(f"{m}, {what}: call us, unbiased / biased (ratio)")
        print("    candidates per query " + "".join(f"{'Q = ' + str(q):>24}" for q in qs))
        for f in fracs:
            c0 = cell[qs[0], f]
            line = f"    {c0['cand_per_query']:>8,} ({100 * f:g} %)".ljust(27)
            for q in qs:
                c = cell[q, f]
                line += f"{c[m + '_call_us']:9,.0f} /{c[m + '_bias_call_us']:7,.0f} " \
                        f"({c[m + '_bias_ratio']:.3f})"
            print(line)
    worst = max(r["cells"], key=lambda c: max(c["spread_pct"].values()))
    print(f"largest min-max spread of a cell's windows: {max(worst['spread_pct'].values()):.2f}% "
          f"(Q = {worst['Q']}, {100 * worst['frac']:g}%); rounds per cell: {r['rounds']}")
    if not r.get("parent_lib"):
        return
    for m in ("gather", "stream"):
        print(f"{m}, {what}: unbiased native entry, parent / this tree, us (+ parent's spread)")
        for f in fracs:
            line = f"    {cell[qs[0], f]['cand_per_query']:>8,} ({100 * f:g} %)".ljust(27)
            for q in qs:
                c = cell[q, f]
                lo, hi = c[f"parent_{m}_call_us_minmax"]
                line += f"{c['parent_' + m + '_call_us']:8,.1f} /{c['this_' + m + '_call_us']:8,.1f}" \
                        f" (+{hi - lo:5.1f}){' ' if c['ab_ok'][m] else '!'}"
            print(line)
    bad = [(c["Q"], c["frac"], m) for c in r["cells"] for m in ("gather", "stream")
           if not c["ab_ok"][m]]
    print(f"cells above the parent's median + spread: {bad if bad else 'none'}")


def bias_probe(args):
    """--bias: the biased call next to the unbiased call on the same lists, gathered and
    streamed (per group with --grouped), alternating window by window; with --parent-lib the
    unbiased native entry of the parent's library and of this tree's join the alternation on
    the same buffers.  ONE JSON line to stdout."""
    from irc_amd import _lib, retrieval
    from irc_amd._torch import ptr, stream_ptr

    fp8 = args.dtype == "fp8"
    lib = _lib.load()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(args.parent_lib)
        for name in ("irc_rerank_topk", "irc_rerank_topk_stream", "irc_rerank_topk_fp8",
                     "irc_rerank_topk_stream_fp8", "irc_rerank_topk_grouped"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2025)
    docs = torch.nn.functional.normalize(
        torch.randn(args.n, args.d, generator=g)).bfloat16().to(dev)
    torch.manual_seed(2025)
    if fp8:
        docs = retrieval.quantize_fp8(docs)
    descale = 1.0 / (retrieval.FP8_SCALE * retrieval.FP8_SCALE) if fp8 else 1.0
    group_off = None
    if args.grouped:  # the page draw of --grouped
        sizes = 1 + torch.empty(args.n, dtype=torch.float64).exponential_(1 / 9.5,
                                                                          generator=g).long()
        ends = torch.cumsum(sizes, 0)
        ends = ends[: int((ends < args.n).sum())]
        group_off = torch.cat([torch.zeros(1, dtype=torch.int64), ends,
                               torch.tensor([args.n])]).to(dev)
    n_groups = group_off.numel() - 1 if args.grouped else 0
    ws_fn = "irc_rerank_topk_grouped_workspace" if args.grouped else "irc_rerank_topk_workspace"
    cells = []
    for Q in args.q:
        qq = torch.nn.functional.normalize(
            torch.randn(Q, args.d, generator=g)).bfloat16().to(dev)
        if fp8:
            qq = retrieval.quantize_fp8(qq)
        out = (torch.empty((Q, args.k), dtype=torch.float32, device=dev),
               torch.empty((Q, args.k), dtype=torch.int64, device=dev),
               torch.empty((Q,), dtype=torch.int32, device=dev))
        for frac in args.frac:
            n = max(1, int(round(frac * args.n)))
            cands = [torch.cat([torch.randperm(args.n, device=dev)[:n].sort().values
                                for _ in range(Q)]).to(torch.int32) for _ in range(args.sets)]
            biases = [torch.randn(Q * n, device=dev) * 0.1 for _ in range(args.sets)]
            off = torch.arange(Q + 1, device=dev, dtype=torch.int64) * n
            ws = torch.empty(int(_lib.fn(ws_fn)(Q, Q * n, args.k)), dtype=torch.uint8, device=dev)

            def wrapped(method, biased):
                counter = [0]

                def call():
                    counter[0] += 1
                    c = cands[counter[0] % args.sets]
                    b = biases[counter[0] % args.sets] if biased else None
                    if fp8:
                        return retrieval.rerank_topk_fp8(qq, docs, c, off, args.k, 0, descale,
                                                         method=method, ascending=True,
                                                         group_off=group_off, bias=b)
                    return retrieval.rerank_topk(qq, docs, c, off, args.k, method=method,
                                                 ascending=True, group_off=group_off, bias=b)
                return call

            def native(which, method):
                """The unbiased native entry of one library, on this cell's buffers."""
                counter = [0]
                flags = (1 if method == "stream" else 0) | (2 if fp8 else 0)
                if args.grouped:
                    fn = which.irc_rerank_topk_grouped
                    mid = (ptr(group_off), n_groups, flags, descale)
                else:
                    fn = getattr(which, "irc_rerank_topk" + ("_stream" if method == "stream"
                                                             else "") + ("_fp8" if fp8 else ""))
                    mid = (descale,) if fp8 else ()

                def call():
                    counter[0] += 1
                    c = cands[counter[0] % args.sets]
                    rc = fn(ptr(qq), ptr(docs), Q, args.n, args.d, ptr(c), ptr(off), Q * n, args.k,
                            0, *mid, ptr(ws), ws.numel(), ptr(out[0]), ptr(out[1]), ptr(out[2]),
                            stream_ptr(dev))
                    if rc != 0:
                        raise SystemExit(f"native rerank entry failed: rc={rc}")
                return call

            timed = [(f"{m}{s}", wrapped(m, b)) for m in ("gather", "stream")
                     for s, b in (("", False), ("_bias", True))]
            if parent is not None:
                timed += [(f"{w}_{m}", native(which, m)) for m in ("gather", "stream")
                          for w, which in (("parent", parent), ("this", lib))]
            est = {}
            for name, fn in timed:
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                est[name] = _window_ms(fn, 5)
            reps = {m: max(2 * args.sets, min(4000, int(args.window_ms / max(est[m], 1e-3))))
                    for m in est}
            for m in reps:
                reps[m] -= reps[m] % args.sets  # every draw equally often
            t = {m: [] for m, _ in timed}
            for _ in range(args.rounds):  # alternate them window by window
                for m, fn in timed:
                    t[m].append(_window_ms(fn, reps[m]))
            med = {m: statistics.median(t[m]) * 1e3 for m in t}
            cell = {"Q": Q, "frac": frac, "cand_per_query": n, "n_cand": Q * n, "reps": reps,
                    "spread_pct": {m: 100.0 * (max(t[m]) - min(t[m])) / statistics.median(t[m])
                                   for m in t}}
            for m in t:
                cell[f"{m}_call_us"] = med[m]
                cell[f"{m}_call_us_minmax"] = [min(t[m]) * 1e3, max(t[m]) * 1e3]
            for m in ("gather", "stream"):
                cell[f"{m}_bias_ratio"] = med[f"{m}_bias"] / med[m]
            if parent is not None:
                cell["ab_ok"] = {
                    m: med[f"this_{m}"] <= med[f"parent_{m}"] +
                    (max(t[f"parent_{m}"]) - min(t[f"parent_{m}"])) * 1e3
                    for m in ("gather", "stream")}
            cells.append(cell)
            ab = "" if parent is None else (
                f"  A/B gather {med['parent_gather']:.1f} / {med['this_gather']:.1f}"
                f" stream {med['parent_stream']:.1f} / {med['this_stream']:.1f} {cell['ab_ok']}")
            print(f"Q={Q:4d} frac={frac:6.3f} n_cand={Q * n:9d}  gather {med['gather']:9.1f} / "
                  f"biased {med['gather_bias']:9.1f} us ({cell['gather_bias_ratio']:.3f})  stream "
                  f"{med['stream']:9.1f} / biased {med['stream_bias']:9.1f} us "
                  f"({cell['stream_bias_ratio']:.3f}){ab}", file=sys.stderr, flush=True)
    print(json.dumps({"probe": "rerank_bias", "device": torch.cuda.get_device_name(0),
                      "dtype": args.dtype, "grouped": bool(args.grouped),
                      "parent_lib": bool(args.parent_lib), "N": args.n, "D": args.d, "k": args.k,
                      "rounds": args.rounds, "window_ms": args.window_ms, "sets": args.sets,
                      "cells": cells}))


def merge_tables(r):
    """The table of DESIGN.md 6e "Across shards": per shape the two merges' call times and
    the grouped merge's kernels."""
    print(f"Q = {r['Q']}, {r['n_groups']:,} groups over {r['N']:,} rows\n")
    print("| shards P | kin = kout | entries / query | topk_merge call | topk_merge_grouped call | "
          "ratio | collapse kernel | select kernel |\n|---|---|---|---|---|---|---|---|")
    for c in r["cells"]:
        print(f"| {c['P']} | {c['kin']:,} | {c['P'] * c['kin']:,} | {c['merge_call_us']:,.1f} | "
              f"{c['merge_grouped_call_us']:,.1f} | {c['ratio']:.2f} | "
              f"{c['collapse_kernel_us']:,.1f} | {c['select_kernel_us']:,.1f} |")
    print()
    worst = max(r["cells"], key=lambda c: max(c["spread_pct"].values()))
    print(f"largest min-max spread of a cell's windows: {max(worst['spread_pct'].values()):.2f}% "
          f"(P = {worst['P']}, kin = {worst['kin']}); rounds per cell: {r['rounds']}")


MERGE_SHAPES = ((2, 100), (8, 100), (8, 1024))


def merge_probe(args):
    """--merge: topk_merge and topk_merge_grouped on the same [P, Q, kin] lists, as P shards
    of an N-row corpus would return them for Q = 256 queries: list p holds kin distinct rows
    of shard p by descending score, unit-normal scores rounded to 1/64 (ties), pages of the
    fixed-seed draw of --grouped (mean about 10 rows).  Windows of back-to-back calls, the two
    alternating round by round (median over the rounds); the grouped merge's kernels from a
    profiled pass of their own.  ONE JSON line to stdout."""
    from irc_amd import _lib, retrieval

    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2025)
    Q = 256
    sizes = 1 + torch.empty(args.n, dtype=torch.float64).exponential_(1 / 9.5, generator=g).long()
    ends = torch.cumsum(sizes, 0)
    ends = ends[: int((ends < args.n).sum())]
    group_off = torch.cat([torch.zeros(1, dtype=torch.int64), ends,
                           torch.tensor([args.n])]).to(dev)
    torch.manual_seed(2025)
    cells = []
    for P, kin in MERGE_SHAPES:
        sets = []
        for _ in range(args.sets):
            idx = torch.empty((P, Q, kin), dtype=torch.int64, device=dev)
            for p in range(P):
                lo, hi = retrieval.shard_bounds(args.n, P, p)
                idx[p] = lo + torch.rand(Q, hi - lo, device=dev).topk(kin, dim=1).indices
            sc = (torch.randn(P, Q, kin, device=dev) * 64).round() / 64
            sets.append((sc.sort(dim=2, descending=True).values.contiguous(), idx))

        def make(grouped):
            counter = [0]

            def call():
                counter[0] += 1
                sc, idx = sets[counter[0] % args.sets]
                if grouped:
                    return retrieval.topk_merge_grouped(sc, idx, kin, group_off)
                return retrieval.topk_merge(sc, idx, kin)
            return call

        timed = [("merge", make(False)), ("merge_grouped", make(True))]
        est = {}
        for name, fn in timed:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            est[name] = _window_ms(fn, 5)
        reps = {m: max(2 * args.sets, min(4000, int(args.window_ms / max(est[m], 1e-3))))
                for m in est}
        for m in reps:
            reps[m] -= reps[m] % args.sets  # every draw equally often
        t = {m: [] for m, _ in timed}
        for _ in range(args.rounds):  # alternate them window by window
            for m, fn in timed:
                t[m].append(_window_ms(fn, reps[m]))
        lib.irc_prof_reset()
        lib.irc_prof_enable(1)
        for _ in range(min(reps["merge_grouped"], 12 * args.sets)):
            timed[1][1]()
        torch.cuda.synchronize()
        lib.irc_prof_enable(0)
        collapse_us, _ = _prof(lib, b"topk_merge_collapse")
        select_us, _ = _prof(lib, b"rerank_select")
        med = {m: statistics.median(t[m]) * 1e3 for m in t}
        n_out = retrieval.topk_merge_grouped(*sets[0], kin, group_off)[2].float().mean().item()
        cell = {"P": P, "kin": kin, "kout": kin, "ratio": med["merge_grouped"] / med["merge"],
                "collapse_kernel_us": collapse_us, "select_kernel_us": select_us,
                "mean_groups_returned": n_out, "reps": reps,
                "spread_pct": {m: 100.0 * (max(t[m]) - min(t[m])) / statistics.median(t[m])
                               for m in t}}
        for m in t:
            cell[f"{m}_call_us"] = med[m]
            cell[f"{m}_call_us_minmax"] = [min(t[m]) * 1e3, max(t[m]) * 1e3]
        cells.append(cell)
        print(f"P={P} kin={kin:5d}  topk_merge {med['merge']:8.1f} us  topk_merge_grouped "
              f"{med['merge_grouped']:8.1f} us ({cell['ratio']:.2f})  collapse {collapse_us:7.1f} us "
              f"select {select_us:7.1f} us", file=sys.stderr, flush=True)
    print(json.dumps({"probe": "rerank_merge", "device": torch.cuda.get_device_name(0),
                      "Q": Q, "N": args.n, "rounds": args.rounds, "window_ms": args.window_ms,
                      "sets": args.sets, "n_groups": int(group_off.numel() - 1),
                      "cells": cells}))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--tables":
        with open(sys.argv[2]) as f:
            rec = json.load(f)
        if isinstance(rec, dict) and rec.get("probe") == "rerank_merge":
            return merge_tables(rec)
        if isinstance(rec, dict) and rec.get("probe") == "rerank_grouped":
            return grouped_tables(rec)
        if isinstance(rec, dict) and rec.get("probe") == "scan_grouped":
            return scan_group_tables(rec)
        if isinstance(rec, dict) and rec.get("probe") == "rerank_bias":
            return bias_tables(rec)
        if isinstance(rec, dict) and rec.get("bf16", {}).get("probe") == "rerank_bias":
            for key in ("bf16", "fp8", "bf16_grouped", "fp8_grouped"):
                if key in rec:
                    bias_tables(rec[key])
                    print()
            return None
        if isinstance(rec, dict) and "bf16" in rec and "fp8" in rec:  # the two runs of a probe
            show = scan_group_tables if rec["bf16"].get("probe") == "scan_grouped" else \
                grouped_tables
            show(rec["bf16"])
            print()
            return show(rec["fp8"])
        return tables(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=250_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=100.0, help="timed work per window")
    ap.add_argument("--sets", type=int, default=4,
                    help="independent candidate draws per cell, cycled call by call")
    ap.add_argument("--q", type=int, nargs="*", default=[1, 16, 64, 256])
    ap.add_argument("--frac", type=float, nargs="*", default=[0.001, 0.01, 0.05, 0.25])
    ap.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: the e4m3 calls, with the bf16 calls of the same cells alongside")
    ap.add_argument("--grouped", action="store_true",
                    help="time rerank_topk(group_off=...) next to the ungrouped call")
    ap.add_argument("--merge", action="store_true",
                    help="time topk_merge and topk_merge_grouped on the same per-shard lists")
    ap.add_argument("--scan-grouped", action="store_true",
                    help="time search(group_off=...) next to search and to the candidate "
                         "route over all-rows lists")
    ap.add_argument("--bias", action="store_true",
                    help="time rerank_topk(bias=...) next to the unbiased call (with --grouped: "
                         "both per group)")
    ap.add_argument("--parent-lib", type=str, default=None,
                    help="--bias: a libirc_hip.so of the parent commit; its unbiased native "
                         "entries join the alternation beside this tree's (the A/B)")
    args = ap.parse_args()
    fp8 = args.dtype == "fp8"
    if not torch.cuda.is_available():
        raise SystemExit("rerank_probe measures on a HIP device; none is visible")
    if args.bias:
        return bias_probe(args)
    if args.merge:
        return merge_probe(args)
    if args.scan_grouped:
        return scan_group_probe(args)
    if args.grouped:
        return grouped_probe(args)
    from irc_amd import _lib, retrieval

    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2025)
    docs = torch.nn.functional.normalize(
        torch.randn(args.n, args.d, generator=g)).bfloat16().to(dev)
    torch.manual_seed(2025)
    docs8 = retrieval.quantize_fp8(docs) if fp8 else None
    descale = 1.0 / (retrieval.FP8_SCALE * retrieval.FP8_SCALE)
    score_span, pick_span = ((b"rerank_fp8_score", b"rerank_fp8_stream_score") if fp8 else
                             (b"rerank_score", b"rerank_stream_score"))
    cells = []
    for Q in args.q:
        qq = torch.nn.functional.normalize(
            torch.randn(Q, args.d, generator=g)).bfloat16().to(dev)
        qq8 = retrieval.quantize_fp8(qq) if fp8 else None
        if fp8:
            scan = lambda: retrieval.scan_topk_fp8(qq8, docs8, args.k, 0, descale)  # noqa: E731
        else:
            scan = lambda: retrieval.scan_topk(qq, docs, args.k)  # noqa: E731
        for frac in args.frac:
            n = max(1, int(round(frac * args.n)))
            # a serving loop brings new lists with every batch: the calls of a window cycle
            # through `sets` independent draws, so a call does not find its own rows of the
            # call before in the Infinity Cache (4 draws of 5% x 16 queries already cover
            # nearly the whole 384 MB shard)
            cands = [torch.cat([torch.randperm(args.n, device=dev)[:n].sort().values
                                for _ in range(Q)]).to(torch.int32) for _ in range(args.sets)]
            off = torch.arange(Q + 1, device=dev, dtype=torch.int64) * n
            turn = [0]

            def gathered(counter, low):
                def call():
                    counter[0] += 1
                    c = cands[counter[0] % args.sets]
                    if low:
                        return retrieval.rerank_topk_fp8(qq8, docs8, c, off, args.k, 0, descale)
                    return retrieval.rerank_topk(qq, docs, c, off, args.k)
                return call

            def streamed(counter, low):
                def call():
                    counter[0] += 1
                    c = cands[counter[0] % args.sets]
                    if low:
                        return retrieval.rerank_topk_fp8(qq8, docs8, c, off, args.k, 0, descale,
                                                         method="stream", ascending=True)
                    return retrieval.rerank_topk(qq, docs, c, off, args.k, method="stream",
                                                 ascending=True)
                return call

            rer, stm = gathered(turn, fp8), streamed([0], fp8)
            timed = [("rerank", rer), ("stream", stm), ("scan", scan)]
            if fp8:  # the bf16 calls of the same cell and draws, in the same alternation
                timed += [("bf16_rerank", gathered([0], False)),
                          ("bf16_stream", streamed([0], False))]
            est = {}
            for name, fn in timed:
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                est[name] = _window_ms(fn, 5)
            reps = {m: max(2 * args.sets, min(4000, int(args.window_ms / max(est[m], 1e-3))))
                    for m in est}
            for m in reps:
                if m != "scan":
                    reps[m] -= reps[m] % args.sets  # every draw equally often
            t = {m: [] for m, _ in timed}
            for _ in range(args.rounds):  # alternate them window by window
                for m, fn in timed:
                    t[m].append(_window_ms(fn, reps[m]))
            # kernel times in a pass of their own (per-launch events slow the host)
            lib.irc_prof_reset()
            lib.irc_prof_enable(1)
            for _ in range(min(reps["rerank"], 12 * args.sets)):
                rer()
            torch.cuda.synchronize()
            lib.irc_prof_enable(0)
            score_us, score_bytes = _prof(lib, score_span)
            select_us, _ = _prof(lib, b"rerank_select")
            lib.irc_prof_reset()
            lib.irc_prof_enable(1)
            for _ in range(min(reps["stream"], 12 * args.sets)):
                stm()
            torch.cuda.synchronize()
            lib.irc_prof_enable(0)
            pick_us, _ = _prof(lib, pick_span)
            sselect_us, _ = _prof(lib, b"rerank_select")
            stream_us = statistics.median(t["stream"]) * 1e3
            scan_us = statistics.median(t["scan"]) * 1e3
            cell = {
                "Q": Q, "frac": frac, "cand_per_query": n, "n_cand": Q * n,
                "rerank_call_us": statistics.median(t["rerank"]) * 1e3,
                "rerank_call_us_minmax": [min(t["rerank"]) * 1e3, max(t["rerank"]) * 1e3],
                "scan_call_us": statistics.median(t["scan"]) * 1e3,
                "scan_call_us_minmax": [min(t["scan"]) * 1e3, max(t["scan"]) * 1e3],
                "score_kernel_us": score_us, "select_kernel_us": select_us,
                "score_bytes": score_bytes,
                "stream_call_us": stream_us,
                "stream_call_us_minmax": [min(t["stream"]) * 1e3, max(t["stream"]) * 1e3],
                # the foreign-key and pick kernels, timed as one span
                "stream_score_kernel_us": pick_us, "stream_select_kernel_us": sselect_us,
                "stream_select_share": sselect_us / stream_us,
                # the floor of the design: a full scan's call plus the select over the keys
                "stream_over_floor": stream_us / (scan_us + sselect_us),
                "score_TBps": score_bytes / (score_us * 1e-6) / 1e12 if score_us else None,
                "reps": reps,
                "spread_pct": {m: 100.0 * (max(t[m]) - min(t[m])) / statistics.median(t[m])
                               for m in t},
            }
            for m in ("bf16_rerank", "bf16_stream"):
                if m in t:
                    cell[f"{m}_call_us"] = statistics.median(t[m]) * 1e3
                    cell[f"{m}_call_us_minmax"] = [min(t[m]) * 1e3, max(t[m]) * 1e3]
            cells.append(cell)
            print(f"Q={Q:4d} frac={frac:6.3f} n_cand={Q * n:9d}  rerank {cell['rerank_call_us']:9.1f} us"
                  f"  (score {score_us:9.1f} us, {cell['score_TBps'] or 0:5.2f} TB/s; select "
                  f"{select_us:7.1f} us)  scan {cell['scan_call_us']:8.1f} us  stream "
                  f"{stream_us:9.1f} us (pick {pick_us:8.1f} us, select {sselect_us:7.1f} us)",
                  file=sys.stderr, flush=True)
    # candidate fraction where two call times cross, per Q (_crossover)
    cross, cross_stream = {}, {}
    for Q in args.q:
        row = [c for c in cells if c["Q"] == Q]
        cross[str(Q)] = _crossover(row, "rerank_call_us", "scan_call_us")
        cross_stream[str(Q)] = _crossover(row, "rerank_call_us", "stream_call_us")
    print(json.dumps({"probe": "rerank_gather_stream_scan", "device": torch.cuda.get_device_name(0),
                      "dtype": args.dtype, "N": args.n, "D": args.d, "k": args.k, "rounds": args.rounds,
                      "window_ms": args.window_ms, "sets": args.sets,
                      "gather_guide_TBps": list(GATHER_TBS), "cells": cells,
                      "crossover_frac": cross, "crossover_frac_stream": cross_stream}))


if __name__ == "__main__":
    main()
