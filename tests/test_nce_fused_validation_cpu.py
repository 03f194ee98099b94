"""CPU check of the host-side argument checks of the fused InfoNCE entries
(irc_nce_fused_workspace, irc_nce_fused_fwd, irc_nce_fused_bwd in csrc/nce_fused.hip):
which pair ranges have a plan, and that every unsupported width, temperature, queue,
batch, range or short workspace is refused with an "nce_fused" message before anything
is launched.  The checks read no memory, so the pointers are plain host buffers (no GPU
needed).  Every call here breaks one check: a fully valid argument set would launch."""
import ctypes

import pytest

from conftest import PKG  # noqa: F401  (import paths)

from irc_amd import _lib

INVALID = 1001

_BUF = ctypes.create_string_buffer(4096)
_HOST = ctypes.addressof(_BUF)

# (id, N, p_lo, p_hi): ranges without a plan
BAD_RANGES = [
    ("p_lo_unaligned", 64, 16, 64),
    ("p_hi_unaligned", 64, 0, 48),
    ("partial_N_unaligned", 72, 0, 32),
    ("partial_N_unaligned_hi", 72, 32, 64),
    ("empty", 64, 32, 32),
    ("reversed", 64, 64, 32),
    ("past_N", 64, 32, 96),
    ("full_width_past_N", 64, 0, 96),
]
GOOD_RANGES = [(1, 0, 1), (2, 0, 2), (33, 0, 33), (70, 0, 70), (64, 0, 64), (64, 0, 32),
               (64, 32, 64), (192, 32, 192), (192, 160, 192)]


def _workspace(N, D, K, lo, hi):
    return int(_lib.fn("irc_nce_fused_workspace")(N, D, K, lo, hi))


@pytest.mark.parametrize("name,N,lo,hi", BAD_RANGES, ids=[r[0] for r in BAD_RANGES])
def test_workspace_is_zero_without_a_plan(name, N, lo, hi):
    for K in (0, 100):
        assert _workspace(N, 64, K, lo, hi) == 0


@pytest.mark.parametrize("N,lo,hi", GOOD_RANGES)
def test_workspace_is_positive_with_a_plan(N, lo, hi):
    for D in (32, 256):
        for K in (0, 5, 4200):
            assert _workspace(N, D, K, lo, hi) > 0


def test_workspace_follows_the_larger_plan():
    """The reported size is the larger of the forward's (max, sum exp) partials + positives
    and the backward's dF partials, + 256; the backward's chunk C grows under the 48 MB cap
    on its partials while the forward's stays at its floor of 2 tiles."""
    # N = 40, K = 4200, D = 32: C = 2 in both, 2 in-batch + 66 queue chunks of [80][32] floats
    assert _workspace(40, 32, 4200, 0, 40) == 68 * 80 * 32 * 4 + 256
    # N = 512, K = 4096, D = 256: partials of C = 1 are exactly 2 x 48 MB, so C = 2 in both
    assert _workspace(512, 256, 4096, 0, 512) == (16 + 64) * 1024 * 256 * 4 + 256
    # one more queue tile is past the cap: the backward takes C = 3 (11 + 43 chunks)
    assert _workspace(512, 256, 4128, 0, 512) == (11 + 43) * 1024 * 256 * 4 + 256
    # K = 0, a pair range: 2 P local rows, the in-batch chunks only (2N = 128: 4 tiles, C = 2)
    assert _workspace(64, 160, 0, 32, 64) == 2 * 64 * 160 * 4 + 256


# a valid argument set (never passed as it stands) and the one thing each case breaks
BASE = dict(N=64, D=64, K=8, T=0.05, lo=0, hi=64, queue=_HOST, ws_bytes=None)
BAD_ARGS = ([(f"D{D}", dict(D=D)) for D in (0, 16, 48, 288)] +
            [("T_zero", dict(T=0.0)), ("T_negative", dict(T=-0.05)),
             ("null_queue", dict(queue=None)), ("N_zero", dict(N=0, hi=0))] +
            [(name, dict(N=N, lo=lo, hi=hi)) for name, N, lo, hi in BAD_RANGES] +
            [("workspace_short", dict(ws_bytes=-1)),
             ("workspace_short_range", dict(lo=32, ws_bytes=-1))])


def _call(entry, N, D, K, T, lo, hi, queue, ws_bytes):
    lib = _lib.load()
    if ws_bytes is None:
        ws_bytes = 1 << 40  # more than any plan here needs
    elif ws_bytes < 0:      # one byte short of the reported size
        ws_bytes = _workspace(N, D, K, lo, hi) + ws_bytes
        assert ws_bytes > 0
    if entry == "irc_nce_fused_fwd":
        return lib.irc_nce_fused_fwd(_HOST, queue, N, D, K, T, lo, hi, _HOST, ws_bytes, _HOST,
                                     _HOST, None)
    return lib.irc_nce_fused_bwd(_HOST, queue, _HOST, N, D, K, T, _HOST, lo, hi, _HOST, ws_bytes,
                                 _HOST, None)


@pytest.mark.parametrize("entry", ["irc_nce_fused_fwd", "irc_nce_fused_bwd"])
@pytest.mark.parametrize("name,broken", BAD_ARGS, ids=[a[0] for a in BAD_ARGS])
def test_bad_arguments_are_refused(entry, name, broken):
    assert any(BASE[key] != value for key, value in broken.items())
    lib = _lib.load()
    assert _call(entry, **dict(BASE, **broken)) == INVALID
    err = lib.irc_last_error()
    assert err.startswith(b"nce_fused"), err
