"""CPU check of the ORDER of the host-side argument checks of the five candidate top-k
entries (irc_rerank_topk, _stream, _fp8, _stream_fp8, _grouped in its four flag forms).
Every row of the table is one call that breaks two checks at once; the return code and the
irc_last_error() text must be those of the earlier one in the documented order:

  sizes, k, D, e4m3 stream D % 128, power-of-two scale, int32 ids, Q, n_cand, stream Q x N,
  workspace, Q == 0 return, null pointers, candidates / docs, alignment, group checks

The checks read no memory, so pointers are null or plain host buffers (no GPU needed)."""
import ctypes

import pytest

from conftest import PKG  # noqa: F401  (import paths)

from irc_amd import _lib

INVALID, WORKSPACE = 1001, 1002

# (name, entry, stream, e4m3, grouped, message prefix)
FORMS = [
    ("topk", "irc_rerank_topk", False, False, False, b"rerank_topk:"),
    ("stream", "irc_rerank_topk_stream", True, False, False, b"rerank_topk:"),
    ("fp8", "irc_rerank_topk_fp8", False, True, False, b"rerank_topk_fp8:"),
    ("stream_fp8", "irc_rerank_topk_stream_fp8", True, True, False, b"rerank_topk_fp8:"),
    ("grouped", "irc_rerank_topk_grouped", False, False, True, b"rerank_topk_grouped:"),
    ("grouped_stream", "irc_rerank_topk_grouped", True, False, True, b"rerank_topk_grouped:"),
    ("grouped_e4m3", "irc_rerank_topk_grouped", False, True, True, b"rerank_topk_grouped:"),
    ("grouped_e4m3_stream", "irc_rerank_topk_grouped", True, True, True,
     b"rerank_topk_grouped:"),
]

_BUF = ctypes.create_string_buffer(4096 + 16)
_ALIGNED = (ctypes.addressof(_BUF) + 15) & ~15  # a 16-byte aligned host address
_WS = ctypes.create_string_buffer(4096)
ALL_POINTERS = dict(queries=_ALIGNED, docs=_ALIGNED, cand=_ALIGNED, cand_off=_ALIGNED,
                    out=_ALIGNED, group_off=_ALIGNED)


def _call(lib, form, Q=4, N=10, D=128, k=5, n_cand=0, doc_offset=0, scale=1.0, ws=None,
          ws_bytes=0, queries=None, docs=None, cand=None, cand_off=None, out=None,
          group_off=None, n_groups=0):
    _, entry, stream, e4m3, grouped, _ = form
    head = (queries, docs, Q, N, D, cand, cand_off, n_cand, k, doc_offset)
    tail = (ws, ws_bytes, out, out, out, None)
    if grouped:
        mid = (group_off, n_groups, (1 if stream else 0) | (2 if e4m3 else 0), scale)
    else:
        mid = (scale,) if e4m3 else ()
    return getattr(lib, entry)(*head, *mid, *tail)


def _any(form):
    return True


def _e4m3(form):
    return form[3]


def _e4m3_stream(form):
    return form[2] and form[3]


def _stream(form):
    return form[2]


def _not_stream(form):
    return not form[2]


def _grouped(form):
    return form[4]


HAVE_WS = dict(ws=ctypes.addressof(_WS), ws_bytes=4096)

# (id, the forms that have both checks, arguments, return code, text of the earlier check)
PAIRS = [
    ("sizes_k", _any, dict(Q=-1, k=0), INVALID, b"negative size"),
    ("k_D", _any, dict(k=0, D=100), INVALID, b"k=0"),
    ("k_D_high", _any, dict(k=1025, D=100), INVALID, b"k=1025"),
    ("D_scale", _e4m3, dict(D=100, scale=3.0), INVALID, b"unsupported D=100"),
    ("D64_scale", _e4m3_stream, dict(D=64, scale=3.0), INVALID, b"unsupported D=64 for the"),
    ("D_ids", _any, dict(D=100, N=1 << 31), INVALID, b"unsupported D=100"),
    ("scale_ids", _e4m3, dict(scale=3.0, N=1 << 31), INVALID, b"power of two"),
    ("ids_workspace", _any, dict(N=1 << 31, n_cand=1000), INVALID, b"fit int32"),
    ("ids_Q", _any, dict(doc_offset=-1, Q=(1 << 31) - 1), INVALID, b"fit int32"),
    ("Q_ncand", _any, dict(Q=(1 << 31) - 1, n_cand=(1 << 31) * 256), INVALID, b"Q too large"),
    ("ncand_workspace", _any, dict(n_cand=(1 << 31) * 256), INVALID, b"n_cand too large"),
    ("QxN_workspace", _stream, dict(Q=1 << 30, N=1 << 30, n_cand=1000), INVALID,
     b"Q x N too large"),
    # the gathered forms have no Q x N bound: the same call stops at the workspace
    ("QxN_gathered", _not_stream, dict(Q=1 << 30, N=1 << 30, n_cand=1000), WORKSPACE,
     b"workspace"),
    ("workspace_null_pointers", _any, dict(n_cand=1000), WORKSPACE, b"workspace 0 <"),
    ("workspace_short", _any, dict(n_cand=1000, **dict(HAVE_WS, ws_bytes=8)), WORKSPACE,
     b"workspace 8 <"),
    ("workspace_group_off", _grouped, dict(n_cand=1000, n_groups=-1), WORKSPACE,
     b"workspace"),
    ("pointers_candidates", _any, dict(n_cand=10, **HAVE_WS), INVALID, b"null pointer"),
    ("pointers_group_off", _grouped, dict(**HAVE_WS), INVALID, b"null pointer"),
    ("candidates_alignment", _any,
     dict(n_cand=10, **HAVE_WS, **dict(ALL_POINTERS, cand=None, queries=_ALIGNED + 8)),
     INVALID, b"null candidates / docs"),
    ("docs_alignment", _any,
     dict(n_cand=10, **HAVE_WS, **dict(ALL_POINTERS, docs=None, queries=_ALIGNED + 8)),
     INVALID, b"null candidates / docs"),
    ("alignment_group_off", _grouped,
     dict(**HAVE_WS, **dict(ALL_POINTERS, group_off=None, docs=_ALIGNED + 8)), INVALID,
     b"16-byte aligned"),
    ("group_off_n_groups", _grouped,
     dict(n_groups=-1, **HAVE_WS, **dict(ALL_POINTERS, group_off=None)), INVALID,
     b"null group_off"),
    ("n_groups", _grouped, dict(n_groups=(1 << 31) - 1, **HAVE_WS, **ALL_POINTERS), INVALID,
     b"n_groups=2147483647"),
]

CASES = [pytest.param(form, args, rc, text, id=f"{form[0]}-{name}")
         for name, applies, args, rc, text in PAIRS for form in FORMS if applies(form)]


@pytest.mark.parametrize("form,args,rc,text", CASES)
def test_the_earlier_check_reports(form, args, rc, text):
    lib = _lib.load()
    assert _call(lib, form, **args) == rc
    err = lib.irc_last_error()
    assert text in err, err
    assert err.startswith(form[5]), err  # every entry keeps its own message prefix


@pytest.mark.parametrize("form", [pytest.param(f, id=f[0]) for f in FORMS])
def test_no_queries_is_ok_with_null_pointers(form):
    """Q == 0 returns IRC_OK once the shape and workspace checks passed: before the pointer,
    alignment and group checks, and before any launch."""
    lib = _lib.load()
    assert _call(lib, form, Q=0, **HAVE_WS) == 0
    assert _call(lib, form, Q=0, n_cand=100, n_groups=-1, **HAVE_WS) == 0
    # ... but not before the workspace check
    assert _call(lib, form, Q=0, n_cand=1000) == WORKSPACE


def test_the_table_covers_every_entry():
    assert {f[1] for f in FORMS} == {n for n in _lib.SIGNATURES
                                     if n.startswith("irc_rerank_topk") and
                                     not n.endswith("_workspace")}
    for name in ("k_D", "D_scale", "scale_ids", "ids_workspace", "workspace_group_off",
                 "D64_scale"):
        assert any(p[0] == name for p in PAIRS)
