"""CPU checks of the e4m3 candidate top-k (irc_rerank_topk_fp8, irc_rerank_topk_stream_fp8):
host-side validation, the workspace code, the operand checks of retrieval.rerank_topk_fp8,
the index's storage check, the fp8 method choice and its constants, and main.py's flag (no
compute without a GPU)."""
import json
import os

import pytest
import torch

from conftest import PKG, ROOT  # noqa: F401  (import paths)

from irc_amd import _lib, retrieval

ENTRIES = ("irc_rerank_topk_fp8", "irc_rerank_topk_stream_fp8")


def _call(lib, entry, D, k, Q=4, N=10, n_cand=0, ws=0, doc_offset=0, scale=1.0):
    return getattr(lib, entry)(None, None, Q, N, D, None, None, n_cand, k, doc_offset, scale,
                               None, ws, None, None, None, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_fp8_entries_reject_bad_arguments_on_the_host(entry):
    lib = _lib.load()
    assert lib.irc_abi_version() == 2  # the additions are additive
    assert _call(lib, entry, 100, 5) == 1001
    assert b"unsupported D" in lib.irc_last_error()
    assert _call(lib, entry, 128, 0) == 1001
    assert b"k=0" in lib.irc_last_error()
    assert _call(lib, entry, 128, 1025) == 1001
    assert b"k=1025" in lib.irc_last_error()
    assert _call(lib, entry, 128, 5, Q=-1) == 1001
    assert b"negative size" in lib.irc_last_error()
    assert _call(lib, entry, 128, 5, n_cand=-1) == 1001
    assert b"negative size" in lib.irc_last_error()
    assert _call(lib, entry, 128, 5, N=1 << 31) == 1001  # doc_offset + N < 2^31
    assert b"fit int32" in lib.irc_last_error()
    assert _call(lib, entry, 128, 5, N=(1 << 31) - 7, doc_offset=7) == 1001
    assert b"fit int32" in lib.irc_last_error()
    for bad in (3.0, 0.0, -0.5, float("inf"), float("nan")):
        assert _call(lib, entry, 128, 5, n_cand=1000, scale=bad) == 1001
        assert b"power of two" in lib.irc_last_error()


def test_d64_is_for_the_gathered_entry_only():
    lib = _lib.load()
    assert _call(lib, "irc_rerank_topk_stream_fp8", 64, 5, n_cand=1000) == 1001
    assert b"unsupported D" in lib.irc_last_error()
    assert _call(lib, "irc_rerank_topk_fp8", 64, 5, n_cand=1000) == 1002


@pytest.mark.parametrize("entry", ENTRIES)
def test_fp8_entries_ask_for_their_workspace(entry):
    """Every shape check passed, no workspace: the workspace code, before any launch."""
    lib = _lib.load()
    for D in (128, 256, 384, 512, 768, 1024):
        assert _call(lib, entry, D, 5, n_cand=1000) == 1002
    assert _call(lib, entry, 128, 1024, n_cand=1000, scale=1.0 / 256) == 1002
    assert _call(lib, entry, 128, 5, n_cand=1000, ws=8) == 1002  # short
    assert b"workspace" in lib.irc_last_error()


def _cpu_args(dtype=torch.uint8):
    return (torch.zeros(2, 128, dtype=dtype), torch.zeros(4, 128, dtype=dtype),
            torch.zeros(3, dtype=torch.int32), torch.tensor([0, 1, 3]), 2)


@pytest.mark.parametrize("method", ["gather", "stream"])
def test_rerank_topk_fp8_operand_checks(method):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.rerank_topk_fp8(*_cpu_args(), method=method)
    for dtype in (torch.float32, torch.bfloat16, torch.int8):
        with pytest.raises(TypeError, match="uint8"):
            retrieval.rerank_topk_fp8(*_cpu_args(dtype), method=method)
    q, d, c, off, k = _cpu_args()
    with pytest.raises(TypeError, match="uint8"):
        retrieval.rerank_topk_fp8(q, d.float(), c, off, k, method=method)


def test_unknown_method_is_a_value_error():
    for method in ("scan", "auto"):  # search_candidates resolves "auto"
        with pytest.raises(ValueError, match="method"):
            retrieval.rerank_topk_fp8(*_cpu_args(), method=method)


def test_fp8_index_checks_its_storage_first():
    """An fp8 index whose shard is not e4m3 bytes (a hand-built one, a damaged header on
    load) is refused before the queries or the device are touched."""
    idx = retrieval.ShardedDenseIndex.__new__(retrieval.ShardedDenseIndex)
    idx.dtype, idx.group, idx.doc_offset, idx.fp8_scale = "fp8", None, 0, 16.0
    args = (torch.zeros(1, 64), torch.zeros(0, dtype=torch.int32),
            torch.zeros(2, dtype=torch.int64), 1)
    for docs in (torch.zeros(2, 64), torch.zeros(2, 64, dtype=torch.bfloat16),
                 torch.zeros(2, 64, dtype=torch.int8)):
        idx.docs = docs
        for method in ("gather", "stream", "auto"):
            with pytest.raises(ValueError, match=r"fp8 index: the shard is not e4m3 bytes "
                                                 r"\(torch.uint8\)"):
                idx.search_candidates(*args, method=method)
    # e4m3 bytes pass the storage check; on the CPU the next stop is the device check
    idx.docs = torch.zeros(2, 64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        idx.search_candidates(*args)


def test_rerank_method_fp8_choice():
    f = retrieval.rerank_method
    assert f(1, 250_000, 768, 250, dtype="fp8") == "gather"
    assert f(0, 250_000, 768, 0, dtype="fp8") == "gather"
    assert f(16, 250_000, 768, 0, dtype="fp8") == "gather"
    # monotone in n_cand at fixed (Q, N, D): once stream, never back
    for Q in (1, 2, 16, 40, 64, 100, 256, 1000):
        for N in (1024, 20_000, 250_000):
            steps = sorted({int(Q * N * x / 400) for x in range(401)} | {1, Q, Q * N})
            got = [f(Q, N, 768, n, dtype="fp8") for n in steps]
            assert set(got) <= {"gather", "stream"}
            first = got.index("stream") if "stream" in got else len(got)
            assert all(g == "stream" for g in got[first:]), (Q, N)
            # D = 64: the e4m3 stream kernel does not run there
            assert {f(Q, N, 64, n, dtype="fp8") for n in steps} == {"gather"}
            # no dtype argument: the bf16 answers, as they were
            assert [f(Q, N, 768, n) for n in steps] == \
                [f(Q, N, 768, n, "bf16") for n in steps] == \
                [_bf16_rule(Q, N, n) for n in steps]
    # a shard of a few docs is always gathered
    for Q in (1, 16, 256, 4096):
        for n in (0, 1, 100, 100 * Q):
            assert f(Q, 100, 768, n, dtype="fp8") == "gather"
    with pytest.raises(ValueError, match="dtype"):
        f(16, 250_000, 768, 1000, dtype="fp16")


def _bf16_rule(Q, N, n_cand):
    """rerank_method as it stood before the dtype argument, restated on _STREAM_CROSSOVER."""
    import math

    if Q <= 0 or n_cand <= 0 or N < 4 * 256:
        return "gather"
    pts = retrieval._STREAM_CROSSOVER
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


def test_fp8_crossover_constants_are_the_probe_file():
    """_STREAM_CROSSOVER_FP8 is the recorded run's gather-against-stream crossovers, under
    the rules of test_rerank_method_constants_are_the_probe_files."""
    with open(os.path.join(ROOT, "profiles", "rerank_fp8_probe.json")) as fh:
        rec = json.load(fh)
    assert rec["dtype"] == "fp8" and rec["N"] == 250_000 and rec["D"] == 768
    cross = rec["crossover_frac_stream"]
    fracs = sorted({c["frac"] for c in rec["cells"]})
    assert [Q for Q, _ in retrieval._STREAM_CROSSOVER_FP8] == sorted(int(q) for q in cross)
    for Q, const in retrieval._STREAM_CROSSOVER_FP8:
        v = cross[str(Q)]
        if isinstance(v, str) and v.startswith(">"):
            assert const is None  # gather won every measured cell
        elif isinstance(v, str) and v.startswith("<"):
            assert const == fracs[0]  # stream won every measured cell: no extrapolation
        else:
            assert const == pytest.approx(v, rel=5e-3)
    for c in rec["cells"]:  # every fp8 time beside the bf16 time of the same run and cell
        assert c["bf16_rerank_call_us"] > 0 and c["bf16_stream_call_us"] > 0


def test_main_parses_index_dtype():
    import main as entry

    assert entry.get_args(["--index-dtype", "fp8"]).index_dtype == "fp8"
    assert entry.get_args(["--index-dtype", "bf16"]).index_dtype == "bf16"
    assert entry.get_args([]).index_dtype == "bf16"
    with pytest.raises(SystemExit):
        entry.get_args(["--index-dtype", "fp16"])
