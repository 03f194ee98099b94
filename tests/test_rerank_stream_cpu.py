"""CPU checks of the streaming candidate top-k (irc_rerank_topk_stream): its host-side
validation, the tile constant, the method dispatch of retrieval.rerank_topk and the
pure-host choice between the two methods (no compute without a GPU)."""
import pytest
import torch

from conftest import PKG  # noqa: F401  (import paths)

from irc_amd import _lib, retrieval


def _call(lib, D, k, Q=4, N=10, n_cand=0, ws=0, doc_offset=0):
    return lib.irc_rerank_topk_stream(None, None, Q, N, D, None, None, n_cand, k, doc_offset,
                                      None, ws, None, None, None, None)


def test_stream_rejects_bad_shapes_on_the_host():
    lib = _lib.load()
    assert lib.irc_abi_version() == 2
    assert _call(lib, 100, 5) == 1001
    assert b"unsupported D" in lib.irc_last_error()
    assert _call(lib, 128, 0) == 1001
    assert b"k=0" in lib.irc_last_error()
    assert _call(lib, 128, 1025) == 1001
    assert b"k=1025" in lib.irc_last_error()
    assert _call(lib, 128, 5, Q=-1) == 1001
    assert b"negative size" in lib.irc_last_error()
    assert _call(lib, 128, 5, n_cand=-1) == 1001
    assert b"negative size" in lib.irc_last_error()
    assert _call(lib, 128, 5, N=1 << 31) == 1001  # doc_offset + N < 2^31
    assert b"fit int32" in lib.irc_last_error()
    assert _call(lib, 128, 5, N=(1 << 31) - 7, doc_offset=7) == 1001
    assert b"fit int32" in lib.irc_last_error()
    # every shape check passed, no workspace: the workspace code, before any launch
    for D in (64, 128, 256, 384, 512, 768, 1024):
        assert _call(lib, D, 5, n_cand=1000) == 1002
    assert _call(lib, 128, 1024, n_cand=1000) == 1002
    assert _call(lib, 128, 5, n_cand=1000, ws=8) == 1002  # short
    assert b"workspace" in lib.irc_last_error()


def test_stream_tile_constant_comes_from_the_library():
    from irc_amd.retrieval import RERANK_STREAM_TILE

    assert RERANK_STREAM_TILE == retrieval.RERANK_STREAM_TILE == \
        _lib.load().irc_rerank_stream_tile()
    assert RERANK_STREAM_TILE >= 64 and RERANK_STREAM_TILE % 64 == 0


def _cpu_args():
    return (torch.zeros(2, 128), torch.zeros(4, 128), torch.zeros(3, dtype=torch.int32),
            torch.tensor([0, 1, 3]), 2)


def test_stream_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.rerank_topk(*_cpu_args(), method="stream")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        retrieval.rerank_topk(*_cpu_args(), method="stream", ascending=True)


def test_unknown_method_is_a_value_error():
    with pytest.raises(ValueError, match="method"):
        retrieval.rerank_topk(*_cpu_args(), method="scan")
    with pytest.raises(ValueError, match="method"):
        retrieval.rerank_topk(*_cpu_args(), method="auto")  # search_candidates resolves it


def test_rerank_method_choice():
    f = retrieval.rerank_method
    assert f(256, 250_000, 768, 256 * 250_000) == "stream"
    assert f(256, 250_000, 768, 256) == "gather"
    assert f(1, 250_000, 768, 250) == "gather"
    assert f(0, 250_000, 768, 0) == "gather"
    assert f(16, 250_000, 768, 0) == "gather"
    # monotone in n_cand at fixed (Q, N, D): once stream, never back
    for Q in (1, 2, 16, 40, 64, 100, 256, 1000):
        for N in (1024, 20_000, 250_000):
            steps = sorted({int(Q * N * x / 400) for x in range(401)} | {1, Q, Q * N})
            got = [f(Q, N, 768, n) for n in steps]
            assert set(got) <= {"gather", "stream"}
            first = got.index("stream") if "stream" in got else len(got)
            assert all(g == "stream" for g in got[first:]), (Q, N)
    # a shard of a few docs is always gathered
    for Q in (1, 16, 256, 4096):
        for n in (0, 1, 100, 100 * Q):
            assert f(Q, 100, 768, n) == "gather"


def test_rerank_method_constants_are_the_probe_files():
    """The dispatch constants are the gather-against-stream crossovers of the recorded
    run, not numbers of their own."""
    import json
    import os

    from conftest import ROOT

    with open(os.path.join(ROOT, "profiles", "rerank_stream_probe.json")) as fh:
        rec = json.load(fh)
    cross = rec["crossover_frac_stream"]
    fracs = sorted({c["frac"] for c in rec["cells"]})
    for Q, const in retrieval._STREAM_CROSSOVER:
        v = cross[str(Q)]
        if isinstance(v, str) and v.startswith(">"):
            assert const is None  # gather won every measured cell
        elif isinstance(v, str) and v.startswith("<"):
            assert const == fracs[0]  # stream won every measured cell: no extrapolation
        else:
            assert const == pytest.approx(v, rel=5e-3)


def test_main_parses_rerank_method():
    import main as entry

    assert entry.get_args(["--rerank-method", "stream"]).rerank_method == "stream"
    assert entry.get_args(["--rerank-method", "gather"]).rerank_method == "gather"
    assert entry.get_args([]).rerank_method == "auto"
    with pytest.raises(SystemExit):
        entry.get_args(["--rerank-method", "scan"])
