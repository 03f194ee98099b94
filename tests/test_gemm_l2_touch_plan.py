"""The line assignment of the big-tile K loop's L2 touch prefetch (big::touch_lines, gemm.hip),
through the host-side helper irc_gemm_l2_touch_map: it replays, with the kernel's own
arithmetic, the touches that the sharers of one operand tile issue over a K loop.  No GPU.

For every geometry of the sweep: each 128-byte line of every K-tile at or past the prefetch
distance is touched by exactly one rank, the K-tiles before it (staged before any touch could
run ahead of them) by none, and no touch addresses a line past the tile's rows or past K.
"""
import numpy as np
import pytest

TILES_N = (1, 2, 6, 8, 33)
WINDOW = (16, 32)
NK = (1, 2, 3, 12)
DIST = (1, 2, 3)
TILES_M = 128


@pytest.mark.parametrize("operand,lines", [(0, 256), (1, 256), (1, 384)])
@pytest.mark.parametrize("window", WINDOW)
@pytest.mark.parametrize("tiles_n", TILES_N)
def test_every_line_has_one_owner(operand, lines, window, tiles_n):
    from irc_amd import ops

    for nk in NK:
        for dist in DIST:
            count, owner, sharers, outside = ops.gemm_l2_touch_map(
                operand, TILES_M, tiles_n, window, lines, nk, dist)
            assert outside == 0, (nk, dist)
            want = min(tiles_n, window) if operand == 0 else max(1, window // tiles_n)
            assert sharers == want
            assert (count[:dist] == 0).all() and (owner[:dist] == -1).all(), (nk, dist)
            assert (count[dist:] == 1).all(), (nk, dist)
            own = owner[dist:]
            assert ((own >= 0) & (own < sharers)).all()
            if own.shape[0]:
                # contiguous shares in rank order, the same in every K-tile, near-equal sizes
                assert (np.diff(own, axis=1) >= 0).all() and (own == own[0]).all()
                sizes = np.bincount(own[0], minlength=sharers)
                assert sizes.max() - sizes.min() <= 1 and sizes.sum() == lines


def test_few_row_tiles_bound_the_b_sharers():
    """A launch with fewer row tiles than the window holds: B's ranks stop at tiles_m."""
    from irc_amd import ops

    count, owner, sharers, outside = ops.gemm_l2_touch_map(1, 2, 2, 32, 384, 4, 2)
    assert sharers == 2 and outside == 0
    assert (count[2:] == 1).all() and set(owner[2:].ravel()) == {0, 1}


def test_bad_arguments_are_refused():
    from irc_amd import ops

    with pytest.raises(ValueError):
        ops.gemm_l2_touch_map(2, 1, 1, 32, 256, 4, 2)
    with pytest.raises(ValueError):
        ops.gemm_l2_touch_map(0, 1, 1, 32, 513, 4, 2)  # more lines than threads
